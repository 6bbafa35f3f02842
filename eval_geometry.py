#!/usr/bin/env python3
"""eval_geometry.py -- score a reconstructed cloud or mesh against a ground-truth cloud: precision, recall and F-score per distance
threshold, the nearest-neighbour distances on the GPU (acezero_amd/cli.py, acezero_amd/geometry.py):
eval_geometry.py RECONSTRUCTION.ply GROUND_TRUTH.ply --thresholds 0.01 0.02 0.05 [--transform T.txt] [--output_json scores.json]
--icp True refines the alignment (--transform, the pose pair, or the identity) by ICP on the GPU before scoring, coarse to fine:
[--icp_distances 0.2 0.1 0.05] [--icp_voxel_sizes 0.04 0.02 0.01] [--icp_max_iterations 30] [--icp_scale True]
A mesh is scored by its vertices unless --sample_spacing S replaces it by samples of its faces, S metres (of the ground truth's
frame) apart, drawn on the GPU: [--sample_spacing 0.005] [--gt_sample_spacing 0.005] [--sample_seed 0] [--write_samples samples.ply]
--crop_file scene.json restricts the reconstruction to the volume of a Tanks and Temples crop file (a polygon swept along an axis):
[--crop_file scene.json] [--crop_file_ground_truth True]
The order of operations: 1. read; 2. move the reconstruction's vertices by the initial alignment; 3. sample the faces; 4. polygon
crop; 5. ICP (from the identity; the reported transform is T_icp T_initial); 6. voxel; 7. box crop (--crop); 8. search."""
import sys

from acezero_amd.cli import eval_geometry_main

if __name__ == "__main__":
    sys.exit(eval_geometry_main())
