#!/usr/bin/env python3
"""register_mapping_rgbd.py -- register_mapping.py's command line plus --depth_files: DSAC*'s RGB-D estimator (the reference's
dsacstar.forward_rgbd) on the MI355X. --threshold and --maxpixelerror are centimetres (acezero_amd/cli.py)."""
import sys

from acezero_amd.cli import register_rgbd_main

if __name__ == "__main__":
    sys.exit(register_rgbd_main())
