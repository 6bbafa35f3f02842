#!/usr/bin/env python3
"""export_cameras.py -- same command line as the reference's export_cameras.py: the cameras of a pose file as a PLY mesh
(acezero_amd/render.py)."""
import sys

from acezero_amd.render import export_cameras_main

if __name__ == "__main__":
    sys.exit(export_cameras_main())
