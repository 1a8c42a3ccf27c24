"""The yardstick of the frame-error tests: per-frame masked MSE reduced on the host from an x_hat that code
accepted earlier produced (tests/test_gpu_frame_errors.py), in float64 or fp32.  Held against ``oracle.ref_cpu.mse``
frame by frame in tests/test_frame_errors_cpu.py."""

import torch


def per_frame_mse(x_hat, target, mask=None, dtype=torch.float64, scale=None):
    """(N,) tensor of ``dtype``: sum over the frame of (x_hat - target)^2 * mask, times ``scale`` (default 1 / C H W:
    the reference's ``losses.mse`` of one frame).  ``target`` fp32 or uint8 (value / 255, divided in fp32 as the
    device does); ``mask`` (N, C, H, W) or one (C, H, W) mask for all frames."""
    x_hat = x_hat.detach().cpu()
    target = target.detach().cpu()
    if target.dtype == torch.uint8:
        target = target.float() / 255
    d = (x_hat.to(dtype) - target.to(dtype)) ** 2
    if mask is not None:
        d = d * mask.detach().cpu().to(dtype)          # (broadcasts a per-trial mask over the frames)
    n = d.shape[0]
    if scale is None:
        scale = 1.0 / d[0].numel()
    return d.reshape(n, -1).sum(dim=1) * torch.tensor(scale, dtype=dtype)
