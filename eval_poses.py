#!/usr/bin/env python3
"""eval_poses.py -- same command line as the reference's eval_poses.py (acezero_amd/cli.py); the alignment and the per-frame
errors run on the GPU (acezero_amd/evaluate.py)."""
import sys

from acezero_amd.cli import eval_poses_main

if __name__ == "__main__":
    sys.exit(eval_poses_main())
