#!/usr/bin/env python3
"""simplify_mesh.py -- a mesh with fewer faces: one vertex per grid cell, placed by the plane quadrics of the faces around it
(acezero_amd/cli.py, acezero_amd/simplify.py):  simplify_mesh.py IN.ply OUT.ply --cell 0.03"""
import sys

from acezero_amd.cli import simplify_mesh_main

if __name__ == "__main__":
    sys.exit(simplify_mesh_main())
