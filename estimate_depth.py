#!/usr/bin/env python3
"""estimate_depth.py -- estimate a depth map per image of an RGB reconstruction by plane-sweep stereo over neighbouring frames
(acezero_amd/cli.py, acezero_amd/mvs.py):  estimate_depth.py POSE_FILE "scene/*.jpg" OUT_DIR --point_cloud pc_final.ply"""
import sys

from acezero_amd.cli import estimate_depth_main

if __name__ == "__main__":
    sys.exit(estimate_depth_main())
