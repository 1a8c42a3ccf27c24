"""The yardstick of the reconstruction-movie tests (no tests here): the strip ``original | reconstruction | residual``
of the reference's ``make_ae_reconstruction_movie_wrapper`` (plotting/ae_utils.py) restated in plain numpy float32.

The strip is written twice, independently, and tests/test_recon_movie_cpu.py holds the two against each other:

* ``strip_blocks``: whole float32 arrays -- ``o * m``, ``0.5 + (om - r)`` -- quantised and put together with
  ``np.concatenate`` per channel (the reference's ``concat(ims[i], axis=1)``) and per panel;
* ``strip_index_rule``: the rule of include/behavenet_hip.h, one output byte at a time.

Operands: ``orig`` and ``recon`` (N, C, H, W), each float32 unit floats or uint8 grey levels (value / 255 as numpy
divides float32 by float32); ``mask`` None, float32 (C, H, W) or float32 (N, C, H, W), applied to the original alone.
Quantisation is ``tests.recon_u8_refs.quantise_u8``.

``contraction_probes`` finds operands on which a fused multiply-subtract of ``o * m - r`` gives another grey level than
the two separately rounded float32 steps: a kernel that lets the product contract fails on them."""

import numpy as np

from tests.recon_u8_refs import quantise_u8

F255 = np.float32(255)
HALF = np.float32(0.5)


def unit(a):
    """float32 unit floats of an operand: uint8 as value / 255 (a true float32 division), float32 as it is."""
    a = np.asarray(a)
    if a.dtype == np.uint8:
        return a.astype(np.float32) / F255
    assert a.dtype == np.float32, a.dtype
    return a


# ------------------------------------------------------------------------------------------ whole arrays
def _side_by_side(x):
    """(N, C, H, W) -> (N, H, C W): the channels of a frame next to each other."""
    return np.concatenate([x[:, c] for c in range(x.shape[1])], axis=2)


def strip_blocks(orig, recon, mask=None, show_orig=True):
    """(N, H, 3 C W) uint8 from whole-array float32 arithmetic."""
    orig, recon = np.asarray(orig), np.asarray(recon)
    with np.errstate(invalid='ignore', over='ignore'):
        o, r = unit(orig), unit(recon)
        om = o if mask is None else o * np.asarray(mask, dtype=np.float32)          # ((C, H, W) broadcasts over N)
        assert om.dtype == np.float32
        if not show_orig:
            p0 = np.zeros(orig.shape, dtype=np.uint8)
        elif mask is None and orig.dtype == np.uint8:
            p0 = orig
        else:
            p0 = quantise_u8(om)
        p1 = recon if recon.dtype == np.uint8 else quantise_u8(r)
        resid = HALF + (om - r)
        assert resid.dtype == np.float32
        p2 = quantise_u8(resid)
    return np.concatenate([_side_by_side(p) for p in (p0, p1, p2)], axis=2).astype(np.uint8)


# ------------------------------------------------------------------------------------------ one byte at a time
def strip_index_rule(orig, recon, mask=None, show_orig=True):
    """(N, H, 3 C W) uint8 by the rule of include/behavenet_hip.h: every output byte (n, y, ox) finds its panel
    ``p = ox // (C W)``, channel ``c = ox % (C W) // W`` and column ``x = ox % W``, picks ITS operands
    orig / mask / recon [n, c, y, x] and computes its own grey level from them."""
    orig, recon = np.asarray(orig), np.asarray(recon)
    n_f, n_c, h, w = orig.shape
    assert recon.shape == orig.shape
    n, y, ox = np.indices((n_f, h, 3 * n_c * w))
    p, c, x = ox // (n_c * w), ox % (n_c * w) // w, ox % w
    o, r = orig[n, c, y, x], recon[n, c, y, x]
    with np.errstate(invalid='ignore', over='ignore'):
        of = o.astype(np.float32) / F255 if o.dtype == np.uint8 else o
        rf = r.astype(np.float32) / F255 if r.dtype == np.uint8 else r
        if mask is None:
            om = of
        else:
            mask = np.asarray(mask, dtype=np.float32)
            assert mask.shape in ((n_c, h, w), (n_f, n_c, h, w))
            om = of * (mask[n, c, y, x] if mask.ndim == 4 else mask[c, y, x])
        assert om.dtype == np.float32 and rf.dtype == np.float32
        if not show_orig:
            level0 = np.zeros(o.shape, dtype=np.uint8)
        else:
            level0 = o if (o.dtype == np.uint8 and mask is None) else quantise_u8(om)
        level1 = r if r.dtype == np.uint8 else quantise_u8(rf)
        d = om - rf
        level2 = quantise_u8(HALF + d)
    return np.select([p == 0, p == 1], [level0, level1], level2).astype(np.uint8)


def into_row(strip, row, n_rows, fill):
    """The strip (N, H, OW) as row ``row`` of a movie (N, n_rows H, OW) whose other rows hold ``fill``."""
    n_f, h, ow = strip.shape
    out = np.full((n_f, n_rows * h, ow), fill, dtype=np.uint8)
    out[:, row * h:(row + 1) * h] = strip
    return out


# ------------------------------------------------------------------------------------------ contraction probes
def contraction_probes(seed, want=64, draws=200_000):
    """``(o_u8, m, r)`` -- uint8 (want,), float32 (want,), float32 (want,) -- the first ``want`` of ``draws`` seeded
    random triples with a fractional mask for which the residual's grey level differs between

    * the separately rounded float32 steps ``o = o_u8 / 255; om = o * m; d = om - r; 0.5 + d``, and
    * the once-rounded ``float32(float64(o) * float64(m) - float64(r))`` of a fused multiply-subtract (the float64
      product of two float32 values is exact, so this rounds once but for the rare double rounding), followed by the
      same ``0.5 +`` and quantisation.

    The two differ only where the residual lies within an ulp of the half-way point between two grey levels: of
    triples uniform in the unit cube 6 in 10^7 qualify (measured, seed 1).  So ``o_u8`` and ``m`` are uniform and
    ``r`` is drawn where it can matter: a uniformly chosen half-way point ``(k + 0.5) / 255``, the ``r`` that puts
    the residual there, moved by -4 .. 4 float32 ulps; triples whose ``r`` leaves [0, 1] are dropped."""
    rng = np.random.default_rng(seed)
    o_u8 = rng.integers(1, 256, size=draws, dtype=np.uint8)
    m = rng.random(draws, dtype=np.float32) * np.float32(0.98) + np.float32(0.01)
    o = o_u8.astype(np.float32) / F255
    k = rng.integers(0, 255, size=draws)
    r = (o.astype(np.float64) * m.astype(np.float64) + 0.5 - (k + 0.5) / 255.0).astype(np.float32)
    r = r + rng.integers(-4, 5, size=draws).astype(np.float32) * np.spacing(np.abs(r))
    assert r.dtype == np.float32
    keep = (r >= 0) & (r <= 1)
    o_u8, m, r, o = o_u8[keep], m[keep], r[keep], o[keep]
    separate = quantise_u8(HALF + (o * m - r))
    fused = (o.astype(np.float64) * m.astype(np.float64) - r.astype(np.float64)).astype(np.float32)
    once = quantise_u8(HALF + fused)
    at = np.flatnonzero(separate != once)[:want]
    assert at.size == want, 'only %d of %d probes in %d draws' % (at.size, want, draws)
    return o_u8[at].copy(), m[at].copy(), r[at].copy()


# ------------------------------------------------------------------------------------------ the kernel's cases
# (N, C, H, W): the smallest; the element path (3 C W = 21); 3 C W = 72, no multiple of 16; all 16-byte stores and
# loads; 16-byte segments that straddle two channels (W = 8)
SHAPES = [(1, 1, 1, 1), (4, 1, 5, 7), (3, 2, 8, 12), (2, 1, 16, 32), (2, 2, 16, 8)]
MASK_FORMS = ['none', 'one', 'per-frame']


def operands(shape, seed, orig_u8, recon_u8, mask_form, specials=True):
    """Seeded ``(orig, recon, mask)`` of one case: uint8 operands uniform in 0..255, float32 ones uniform in [0, 1)
    with the half-way values, NaN and infinities of ``with_specials`` spliced in; a mask of zeros, ones and fractions."""
    from tests.recon_u8_refs import with_specials
    rng = np.random.default_rng(seed)
    size = int(np.prod(shape))

    def one(u8, k):
        if u8:
            return rng.integers(0, 256, size=shape, dtype=np.uint8)
        x = rng.random(size, dtype=np.float32)
        return (with_specials(x, seed=seed + k) if specials else x).reshape(shape)
    orig, recon = one(orig_u8, 1), one(recon_u8, 2)
    mask = None
    if mask_form != 'none':
        m_shape = shape if mask_form == 'per-frame' else shape[1:]
        mask = rng.random(m_shape, dtype=np.float32)
        kind = rng.integers(0, 3, size=m_shape)
        mask = np.where(kind == 0, np.float32(0), np.where(kind == 1, np.float32(1), mask)).astype(np.float32)
    return orig, recon, mask
