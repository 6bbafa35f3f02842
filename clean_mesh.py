#!/usr/bin/env python3
"""clean_mesh.py -- drop the floating fragments of a mesh: keep the connected components that are large enough
(acezero_amd/cli.py, acezero_amd/mesh.py):  clean_mesh.py IN.ply OUT.ply --min_component_faces 100"""
import sys

from acezero_amd.cli import clean_mesh_main

if __name__ == "__main__":
    sys.exit(clean_mesh_main())
