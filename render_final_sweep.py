#!/usr/bin/env python3
"""render_final_sweep.py -- same command line as the reference's render_final_sweep.py, frames drawn by the HIP rasteriser
(acezero_amd/render.py)."""
import sys

from acezero_amd.render import render_final_sweep_main

if __name__ == "__main__":
    sys.exit(render_final_sweep_main())
