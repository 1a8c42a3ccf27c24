"""The yardstick of the pixel-stats tests (csrc/pixel_stats.hip, fitting.eval.pixel_stats_device): the four per-pixel
sums over the frames in numpy.

The TERMS are computed in float32 with the IEEE operations the kernel uses -- ``d = xh - t``, ``e = (d * d) * m``,
``t = u8.astype(float32) / float32(255)`` -- so they are the kernel's bit for bit; they are then widened and summed in
float64.  The moments are computed entirely in float64 from the float32 ``t`` (``m * t`` is exact there, ``t * t``
too; ``m * (t * t)`` rounds once, as in the kernel).

What is left between this and the kernel is the ORDER of the float64 additions: on sums of non-negative terms that is
at most N * 2^-53 relative, 3.3e-14 at the N <= 300 of the GPU tests, which hold the kernel to RTOL = 1e-12.  (Checked
on the CPU in tests/test_pixel_stats_cpu.py: left-to-right, blocked and numpy's own order stay inside N * 2^-53 of
each other up to N = 4096.)"""

import numpy as np

RTOL = 1e-12


def _np(a):
    return a.detach().cpu().numpy() if hasattr(a, 'detach') else np.asarray(a)


def unit_float(target):
    """float32 frames from float32 or stored uint8 frames: value / 255 divided in float32, as the device does."""
    target = _np(target)
    if target.dtype == np.uint8:
        return target.astype(np.float32) / np.float32(255)
    assert target.dtype == np.float32, target.dtype
    return target


def pixel_sums(x_hat, target, mask=None):
    """(4, C, H, W) float64: [sse, w, s1, s2] summed over the N frames of ``target`` (N, C, H, W), float32 or uint8.
    ``x_hat`` float32 of that shape or None (plane 0 stays zero); ``mask`` float32 (N, C, H, W), one (C, H, W) mask
    for all frames, or None."""
    t = unit_float(target)
    m = np.ones(t.shape[1:], dtype=np.float32) if mask is None else _np(mask).astype(np.float32, copy=False)
    if m.ndim == t.ndim - 1:
        m = m[None]
    m = np.broadcast_to(m, t.shape)
    out = np.zeros((4,) + t.shape[1:], dtype=np.float64)
    if x_hat is not None:
        xh = _np(x_hat).reshape(t.shape)
        assert xh.dtype == np.float32
        d = xh - t                                   # float32
        e = (d * d) * m                              # float32: two roundings, the kernel's
        assert e.dtype == np.float32
        out[0] = e.astype(np.float64).sum(axis=0)
    t64, m64 = t.astype(np.float64), m.astype(np.float64)
    out[1] = m64.sum(axis=0)
    out[2] = (m64 * t64).sum(axis=0)
    out[3] = (m64 * (t64 * t64)).sum(axis=0)
    return out


def assert_close(got, want, exact_w, name=''):
    """Planes 0, 2 and 3 to RTOL (sums of non-negative terms: no absolute part), plane 1 to RTOL or, for 0/1 masks
    and no mask, exactly."""
    got, want = _np(got), np.asarray(want)
    assert got.dtype == np.float64 and got.shape == want.shape, (name, got.dtype, got.shape, want.shape)
    for p in (0, 2, 3):
        err = np.abs(got[p] - want[p])
        assert np.all(err <= RTOL * np.abs(want[p])), (name, p, float((err / np.maximum(np.abs(want[p]), 1e-300)).max()))
    if exact_w:
        assert np.array_equal(got[1], want[1]), (name, 'w')
    else:
        assert np.all(np.abs(got[1] - want[1]) <= RTOL * np.abs(want[1])), (name, 'w')
