"""Drop-in for `import dsacstar` (register_mapping.py:12 of the reference): the reference builds this module from
dsacstar/dsacstar.cpp with OpenCV; here it is the MI355X implementation behind the same callable.

    import dsacstar
    inliers = dsacstar.forward_rgb(scene_coordinates_1x3xHxW, out_pose_4x4, hypotheses, threshold, focal, ppX, ppY,
                                   inlier_alpha, max_reproj, subsampling, seed, max_hypotheses_tries)

Put the repository root on PYTHONPATH (or copy this directory next to register_mapping.py) and the reference's
register_mapping.py runs unchanged on this call. forward_rgbd is the reference's commented-out RGB-D binding (dsacstar.cpp:901),
same arguments. backward_rgb and backward_rgbd are the reference's commented-out gradients (dsacstar.cpp:208-490, 642-895), same
arguments. Extras (not in the reference): register_batch / register_batch_rgbd / register_batch_backward / register_batch_rgbd_backward (device-resident,
batched), expected_pose_loss_rgb / expected_pose_loss_rgbd (torch.autograd losses),
set_verbose, reset_call_counter."""
from acezero_amd.dsacstar import (backward_rgb, backward_rgbd, expected_pose_loss_rgb, expected_pose_loss_rgbd, forward_rgb,  # noqa: F401
                                  forward_rgbd, register_batch, register_batch_backward, register_batch_rgbd,
                                  register_batch_rgbd_backward, reset_call_counter, set_verbose)
