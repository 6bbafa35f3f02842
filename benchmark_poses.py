#!/usr/bin/env python3
"""benchmark_poses.py -- the command line of the reference's benchmarks/benchmark_poses.py (acezero_amd/cli.py): writes the nerfstudio
data set (transforms.json) and, with --method reproject (the default here), scores the held-out views by reprojection on the GPU
(acezero_amd/benchmark.py). The result is NOT nerfacto PSNR."""
import sys

from acezero_amd.cli import benchmark_poses_main

if __name__ == "__main__":
    sys.exit(benchmark_poses_main())
