#!/usr/bin/env python3
"""fuse_depth.py -- fuse an RGB-D reconstruction's depth maps along its poses into a TSDF volume and write the surface as a mesh
(acezero_amd/cli.py, acezero_amd/fusion.py):  fuse_depth.py POSE_FILE "scene/*.jpg" --depth_files "scene/depth/*.png" OUTPUT.ply"""
import sys

from acezero_amd.cli import fuse_depth_main

if __name__ == "__main__":
    sys.exit(fuse_depth_main())
