#!/usr/bin/env python3
"""render_mesh.py -- render a triangle mesh into the cameras of a reconstruction: one model depth map per image, seen from that
image's estimated pose (acezero_amd/cli.py, acezero_amd/meshrender.py):  render_mesh.py MESH.ply POSE_FILE "scene/*.jpg" OUT_DIR"""
import sys

from acezero_amd.cli import render_mesh_main

if __name__ == "__main__":
    sys.exit(render_mesh_main())
