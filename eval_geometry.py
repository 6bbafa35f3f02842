#!/usr/bin/env python3
"""eval_geometry.py -- score a reconstructed cloud or mesh against a ground-truth cloud: precision, recall and F-score per distance
threshold, the nearest-neighbour distances on the GPU (acezero_amd/cli.py, acezero_amd/geometry.py):
eval_geometry.py RECONSTRUCTION.ply GROUND_TRUTH.ply --thresholds 0.01 0.02 0.05 [--transform T.txt] [--output_json scores.json]
--icp True refines the alignment (--transform, the pose pair, or the identity) by ICP on the GPU before scoring, coarse to fine:
[--icp_distances 0.2 0.1 0.05] [--icp_voxel_sizes 0.04 0.02 0.01] [--icp_max_iterations 30] [--icp_scale True]"""
import sys

from acezero_amd.cli import eval_geometry_main

if __name__ == "__main__":
    sys.exit(eval_geometry_main())
