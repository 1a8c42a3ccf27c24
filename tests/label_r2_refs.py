"""What the label-score tests share (tests/test_label_r2_cpu.py, tests/test_gpu_label_r2.py): the reference of
``bn_segment_label_sums`` in numpy float64 with ``math.fsum`` per (segment, column) -- so the reference itself carries
no summation error --, the derived tolerance, the input families, and a synthetic generator that serves label masks.

Tolerance.  Device and reference form the same float64 terms from the same fp32 operands and differ only in the order
of the additions (and in whether ``d * d`` is rounded before it is added: one rounding a term).  A sum of m terms added
in any order is within ``(m - 1) u sum|term|`` of the exact one to first order, ``u = 2^-53``; the bound asserted is

    count exact;   |sum - ref| <= 4 m 2^-53 sum|term|     (m = the segment's valid count)

and the NaN positions must agree exactly."""

import functools
import math

import numpy as np

from behavenet_amd.data.data_generator import SyntheticSessionsGenerator

U = 2.0 ** -53
LENGTHS = [0, 1, 10, 11, 257, 1023, 0, 4099]          # one call: empty, single-row, at and over min_valid, long
FIRST_ROW = 3                                         # offsets[0]: the rows before it belong to no segment
TRAILING = 2                                          # ... and neither do the rows after the last segment
ALL_ZERO_SEGMENT = 4                                  # the segment (257 rows) whose mask is all zero
CONSTANT = (5, 0)                                     # (segment, column) whose labels are one value


def safe_offsets(offsets, n):
    """The offsets as the kernel reads them: clamped into [0, n], then the running maximum."""
    return np.maximum.accumulate(np.clip(np.asarray(offsets, dtype=np.int64), 0, n))


def _fsum(terms):
    return math.fsum(terms) if np.isfinite(terms).all() else float(np.sum(terms))


def sums_ref(pred, truth, mask, offsets, L):
    """-> ``(sums, mags)``, both float64 ``(S, L, 4)``: per segment and column the count, ``sum y``, ``sum y^2`` and
    ``sum (y - p)^2`` over the entries whose mask is exactly 1 (all, without a mask), every term formed in float64 from
    the float32 operands and summed with ``math.fsum``; ``mags`` holds ``sum |term|`` for the tolerance."""
    pred, truth = np.asarray(pred, dtype=np.float32), np.asarray(truth, dtype=np.float32)
    n = truth.shape[0]
    e = safe_offsets(offsets, n)
    S = len(e) - 1
    sums, mags = np.zeros((S, L, 4)), np.zeros((S, L, 4))
    for s in range(S):
        rows = slice(int(e[s]), int(e[s + 1]))
        for j in range(L):
            y, p = truth[rows, j].astype(np.float64), pred[rows, j].astype(np.float64)
            if mask is not None:
                ok = np.asarray(mask)[rows, j] == np.float32(1)
                y, p = y[ok], p[ok]
            with np.errstate(invalid='ignore', over='ignore'):
                d = y - p
                terms = (y, y * y, d * d)
            sums[s, j, 0] = mags[s, j, 0] = len(y)
            for k, t in enumerate(terms):
                sums[s, j, k + 1] = _fsum(t)
                mags[s, j, k + 1] = _fsum(np.abs(t))
    return sums, mags


def assert_sums_close(got, want, mags, what=''):
    got = np.asarray(got)
    assert got.shape == want.shape and got.dtype == np.float64, what
    assert np.array_equal(got[..., 0], want[..., 0]), (what, 'counts')
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, 'NaN positions')
    m = want[..., :1]
    with np.errstate(invalid='ignore'):
        bound = 4 * m * U * mags
        bad = np.abs(got - want) > bound
    bad &= ~np.isnan(want)
    assert not bad.any(), (what, np.argwhere(bad)[:5], got[bad][:5], want[bad][:5])


@functools.lru_cache(maxsize=None)
def kernel_case(L, with_mask):
    """The tables of the kernel test, ``(pred, truth, mask, offsets)``, made once and shared (copy before writing):
    ``LENGTHS`` rows a segment after ``FIRST_ROW`` leading rows, labels of mean 300 and standard deviation 50, predictions off by N(0, 20), a mask
    of about 80 % ones with one all-zero segment, one column constant within one segment, and NaNs with a one mask in
    the rows that belong to no segment."""
    rng = np.random.default_rng(100 + L)
    n = FIRST_ROW + sum(LENGTHS) + TRAILING
    offsets = FIRST_ROW + np.concatenate(([0], np.cumsum(LENGTHS))).astype(np.int64)
    truth = (300 + 50 * rng.standard_normal((n, L))).astype(np.float32)
    seg, col = CONSTANT
    if col < L:
        truth[offsets[seg]:offsets[seg + 1], col] = np.float32(317.25)
    pred = (truth + 20 * rng.standard_normal((n, L))).astype(np.float32)
    mask = None
    if with_mask:
        mask = (rng.random((n, L)) < 0.8).astype(np.float32)
        mask[offsets[ALL_ZERO_SEGMENT]:offsets[ALL_ZERO_SEGMENT + 1]] = 0
        mask[:FIRST_ROW] = 1
        mask[offsets[-1]:] = 1
    for rows in (slice(0, FIRST_ROW), slice(int(offsets[-1]), n)):          # never read: they would show
        truth[rows] = np.nan
        pred[rows] = np.nan
    return pred, truth, mask, offsets          # (shared between tests: not to be written)


@functools.lru_cache(maxsize=None)
def kernel_case_ref(L, with_mask):
    pred, truth, mask, offsets = kernel_case(L, with_mask)
    return sums_ref(pred, truth, mask, offsets, L)


def family(name, n, L, seed=0):
    """``(pred, truth)`` float32 ``(n, L)`` of a value family: the labels' mean over their standard deviation is what
    the raw-moment form of ``SStot`` loses digits to."""
    rng = np.random.default_rng([seed, n, L])
    mean, std = {'unit': (0.0, 1.0), 'mean 300 std 50': (300.0, 50.0), 'mean 1000 std 1': (1000.0, 1.0)}[name]
    truth = (mean + std * rng.standard_normal((n, L))).astype(np.float32)
    pred = (truth + 0.4 * std * rng.standard_normal((n, L))).astype(np.float32)
    return pred, truth


FAMILIES = ('unit', 'mean 300 std 50', 'mean 1000 std 1')


class MaskedSessionsGenerator(SyntheticSessionsGenerator):
    """A synthetic generator that serves ``labels_masks`` for the sessions that have them (a list of (T, L) float32
    arrays a session, as tests/test_gpu_ranges.py attaches them), next to the labels and on their device."""

    def _extra_signals(self, sample, sess, trial):
        import torch
        masks = getattr(self.datasets[sess], 'labels_masks', None)
        if masks is not None:
            sample['labels_masks'] = torch.from_numpy(masks[trial]).to(self.device)[None]
