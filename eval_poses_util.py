"""Drop-in for `import eval_poses_util as tutil` (eval_poses.py:14 of the reference): TestEstimate and estimate_alignment with the
reference's signature, computed on the GPU (acezero_amd/evaluate.py).  Extras: evaluate_poses, and estimate_alignment's keyword-only
`seed` / `samples`."""
from acezero_amd.evaluate import TestEstimate, estimate_alignment, evaluate_poses  # noqa: F401
