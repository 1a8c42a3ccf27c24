"""What the latent-correlation tests share (tests/test_latent_corr_cpu.py, tests/test_gpu_latent_corr.py): the
reference of ``bn_segment_gram`` in numpy float64 with ``math.fsum`` per (segment, entry) -- so the reference itself
carries no summation error --, the two derived tolerances, the input families and two emulations of the device's sums.

Sums.  Device and reference form the same float64 terms from the same fp32 operands, ``a = float64(z) - float64(c)``
and the products, and differ only in the order of the additions (and in whether a product is rounded before it is
added: one rounding a term).  The bound asserted is the project's, as tests/label_r2_refs.py states it:

    count exact;   |sum - ref| <= 4 m 2^-53 sum|term|     (m = the segment's rows)

the NaN positions must agree exactly, and ``A[i][j]`` and ``A[j][i]`` must hold the same bits.

Correlations.  Against ``np.corrcoef`` of the float64 cast of the same fp32 rows.  First-order propagation of the bound
above through ``cov = (G - s s^T / n) / (n - 1)`` and the normalisation gives

    |corr - np.corrcoef| <= 32 n 2^-53 kappa^2,     kappa^2 = max_j (1 + (mean_j - c_j)^2 / var_j)

with ``kappa^2`` computed from the data: how much larger the raw moments about the shift ``c`` are than the centred
ones."""

import functools
import math

import numpy as np

from tests.label_r2_refs import safe_offsets

U = 2.0 ** -53
LENGTHS = [0, 1, 2, 10, 257, 1023, 0, 4099]           # one call: empty, one row, two, short, odd, long
FIRST_ROW = 3                                         # offsets[0]: the rows before it belong to no segment
TRAILING = 2                                          # ... and neither do the rows after the last segment
CONSTANT = (5, 0)                                     # (segment, column) whose values are one value
KERNEL_DS = (1, 2, 3, 16, 33, 64)
# (mean, std) by column, in turn: the reference's unit latents next to columns far from zero (AE latents are not
# centred)
MIXED = ((300.0, 1.0), (0.0, 1.0), (-40.0, 5.0))


def _fsum(terms):
    return math.fsum(terms.tolist()) if np.isfinite(terms).all() else float(np.sum(terms))


def gram_ref(z, offsets, shift=None):
    """-> ``(A, mags)``, both float64 ``(S, D + 1, D + 1)``: per segment the sum over its rows of ``a^T a`` with
    ``a = (1, float64(z) - float64(shift))``, every term formed in float64 from the float32 operands and summed with
    ``math.fsum`` per entry; ``mags`` holds ``sum |term|`` for the tolerance."""
    z = np.asarray(z, dtype=np.float32)
    n, D = z.shape
    c = np.zeros(D) if shift is None else np.asarray(shift, dtype=np.float32).astype(np.float64)
    e = safe_offsets(offsets, n)
    S = len(e) - 1
    A, mags = np.zeros((S, D + 1, D + 1)), np.zeros((S, D + 1, D + 1))
    for s in range(S):
        rows = slice(int(e[s]), int(e[s + 1]))
        with np.errstate(invalid='ignore', over='ignore'):
            a = np.concatenate([np.ones((rows.stop - rows.start, 1)), z[rows].astype(np.float64) - c], axis=1)
            for i in range(D + 1):
                for j in range(i, D + 1):
                    terms = a[:, i] * a[:, j]
                    A[s, i, j] = A[s, j, i] = _fsum(terms)
                    mags[s, i, j] = mags[s, j, i] = _fsum(np.abs(terms))
    return A, mags


def assert_gram_close(got, want, mags, what=''):
    got = np.asarray(got)
    assert got.shape == want.shape and got.dtype == np.float64, what
    assert np.array_equal(got[:, 0, 0], want[:, 0, 0]), (what, 'counts')
    assert np.array_equal(got.view(np.int64), np.swapaxes(got, 1, 2).view(np.int64)), (what, 'A[i][j] is not A[j][i]')
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, 'NaN positions')
    m = want[:, :1, :1]
    with np.errstate(invalid='ignore'):
        bound = 4 * m * U * mags
        bad = np.abs(got - want) > bound
    bad &= np.isfinite(want)
    assert not bad.any(), (what, np.argwhere(bad)[:5], got[bad][:5], want[bad][:5])
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), (what, 'infinities')


def corr_bound(z, shift=None):
    """``32 n 2^-53 kappa^2`` for the rows ``z`` (fp32, at least two of them, no constant column) and the shift."""
    z64 = np.asarray(z, dtype=np.float32).astype(np.float64)
    c = 0.0 if shift is None else np.asarray(shift, dtype=np.float32).astype(np.float64)
    kappa2 = np.max(1.0 + (z64.mean(axis=0) - c) ** 2 / z64.var(axis=0, ddof=1))
    return 32.0 * len(z64) * U * kappa2


def assert_corr_close(got, z, shift=None, what=''):
    """``got`` (D, D) against ``np.corrcoef`` of the float64 cast of the rows, within ``corr_bound``."""
    z64 = np.asarray(z, dtype=np.float32).astype(np.float64)
    want = np.corrcoef(z64.T).reshape(z64.shape[1], z64.shape[1])
    bound = corr_bound(z, shift)
    err = np.abs(np.asarray(got) - want).max()
    assert err <= bound, (what, err, bound)
    return err, bound


def mixed(n, D, seed=0, means=None):
    """float32 ``(n, D)``: column j of mean and deviation ``MIXED[j % 3]`` (or of mean ``means`` and deviation 1),
    mildly correlated with its neighbour."""
    rng = np.random.default_rng([seed, n, D])
    x = rng.standard_normal((n, D))
    x[:, 1:] += 0.5 * x[:, :-1]
    if means is None:
        mean = np.array([MIXED[j % 3][0] for j in range(D)])
        std = np.array([MIXED[j % 3][1] for j in range(D)])
    else:
        mean, std = np.full(D, float(means)), np.ones(D)
    return (mean + std * x).astype(np.float32)


@functools.lru_cache(maxsize=None)
def kernel_case(D):
    """The table of the kernel test, ``(z, offsets, shift)``, made once and shared (copy before writing): ``LENGTHS``
    rows a segment after ``FIRST_ROW`` leading rows, the ``mixed`` columns, one column constant within one segment, and
    NaNs in the rows that belong to no segment.  The shift is the first row of the first segment that has one."""
    n = FIRST_ROW + sum(LENGTHS) + TRAILING
    offsets = FIRST_ROW + np.concatenate(([0], np.cumsum(LENGTHS))).astype(np.int64)
    z = mixed(n, D, seed=100 + D)
    seg, col = CONSTANT
    z[offsets[seg]:offsets[seg + 1], col] = np.float32(317.25 if MIXED[col % 3][0] else 0.75)
    shift = z[FIRST_ROW].copy()
    z[:FIRST_ROW] = np.nan
    z[offsets[-1]:] = np.nan
    return z, offsets, shift          # (shared between tests: not to be written)


@functools.lru_cache(maxsize=None)
def kernel_case_ref(D, shifted):
    z, offsets, shift = kernel_case(D)
    return gram_ref(z, offsets, shift if shifted else None)


# ------------------------------------------------------------------------------------------ emulations
EMULATION_CASES = ((10, 3, 0), (257, 16, 300), (4099, 64, 300), (4099, 2, 0), (70001, 16, 300))          # (n, D, mean)


def gram_emulated(z, shift=None, acc=np.float64, block=256):
    """One segment's matrix as a device might add it: 256-row blocks, each summed on its own, the blocks' partials
    added in REVERSED order, every product and sum in ``acc`` (float64: what the kernel does, in another order;
    float32: what it must not do)."""
    z = np.asarray(z, dtype=np.float32)
    c = np.zeros(z.shape[1]) if shift is None else np.asarray(shift, dtype=np.float32).astype(np.float64)
    a = np.concatenate([np.ones((len(z), 1)), z.astype(np.float64) - c], axis=1).astype(acc)
    total = np.zeros((a.shape[1], a.shape[1]), dtype=acc)
    for start in reversed(range(0, len(a), block)):
        blk = a[start:start + block]
        part = np.zeros_like(total)
        for r in range(0, len(blk), 16):          # (sixteen rows a step: a matmul of ``acc`` operands)
            part = (part + blk[r:r + 16].T @ blk[r:r + 16]).astype(acc)
        total = (total + part).astype(acc)
    return total.astype(np.float64)[None]
