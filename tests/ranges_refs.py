"""References and inputs for the range tests (tests/test_ranges_cpu.py, tests/test_gpu_ranges.py): the selection
rule by ``np.sort`` and the value families that go wrong in different passes of the radix select."""

import numpy as np

PERCENTILES = [0, 5, 15, 50, 85, 95, 100, 33.3]
SIZES = [1, 2, 3, 7, 64, 255, 256, 257, 1000, 4099, 70001]


def select_ref(x, ranks):
    """out[k, j] = np.sort(the non-NaN values of column j)[ranks[k, j]], NaN for a rank outside the column."""
    x = np.asarray(x, dtype=np.float32)
    ranks = np.asarray(ranks, dtype=np.int64)
    out = np.full(ranks.shape, np.nan, dtype=np.float32)
    for j in range(x.shape[1]):
        col = x[:, j]
        srt = np.sort(col[~np.isnan(col)])
        for k in range(ranks.shape[0]):
            if 0 <= ranks[k, j] < srt.size:
                out[k, j] = srt[ranks[k, j]]
    return out


def count_ref(x):
    return np.sum(~np.isnan(np.asarray(x)), axis=0).astype(np.int64)


def _from_bits(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def family(name, n, d, seed=0):
    """An (n, d) float32 table of one of the FAMILIES."""
    rng = np.random.default_rng(seed + 1000 * len(name) + n + 7 * d)
    shape = (n, d)
    if name == 'normal':
        x = rng.standard_normal(shape).astype(np.float32)
    elif name == 'all equal':
        x = np.full(shape, np.float32(-1.25))
    elif name == 'two values':
        x = np.where(rng.random(shape) < 0.3, np.float32(2.5), np.float32(-0.75)).astype(np.float32)
    elif name == 'lowest byte':           # the first three digits of every key agree
        x = _from_bits(np.uint32(0x3fc00000) + rng.integers(0, 256, size=shape).astype(np.uint32))
    elif name == 'highest byte':          # the last three digits of every key agree
        # (non-negative values, so the key is the bits with the sign set; 0x7f345678 is finite)
        x = _from_bits((rng.integers(0, 128, size=shape).astype(np.uint32) << np.uint32(24)) | np.uint32(0x00345678))
    elif name == 'signs and zeros':
        x = rng.standard_normal(shape).astype(np.float32) * np.float32(1e-3)
        pick = rng.random(shape)
        x = np.where(pick < 0.15, np.float32(0.0), x)
        x = np.where((pick >= 0.15) & (pick < 0.3), np.float32(-0.0), x).astype(np.float32)
    elif name == 'infinities and denormals':
        x = _from_bits(rng.integers(0, 64, size=shape).astype(np.uint32))          # denormals and +0
        x = np.where(rng.random(shape) < 0.5, -x, x)
        pick = rng.random(shape)
        x = np.where(pick < 0.1, np.float32(np.inf), x)
        x = np.where((pick >= 0.1) & (pick < 0.2), np.float32(-np.inf), x)
        x = np.where((pick >= 0.2) & (pick < 0.4), rng.standard_normal(shape).astype(np.float32), x).astype(np.float32)
    elif name == 'ascending':
        x = (np.arange(n * d, dtype=np.float32).reshape(shape) - np.float32(n * d / 3)) * np.float32(0.37)
    elif name == 'descending':
        x = (np.float32(n * d / 3) - np.arange(n * d, dtype=np.float32).reshape(shape)) * np.float32(0.37)
    elif name == 'ten percent nan':
        x = rng.standard_normal(shape).astype(np.float32)
        nan = _from_bits(np.where(rng.random(shape) < 0.5, 0x7fc00000, 0xffc00123).astype(np.uint32))
        x = np.where(rng.random(shape) < 0.1, nan, x)          # both signs, with a payload
    elif name == 'all-nan column':
        x = rng.standard_normal(shape).astype(np.float32)
        x[:, d // 2] = np.nan
    elif name == 'single valid value':
        x = rng.standard_normal(shape).astype(np.float32)
        x[:, 0] = np.nan
        x[n // 2, 0] = np.float32(3.5)
    else:
        raise KeyError(name)
    x = np.ascontiguousarray(x, dtype=np.float32)
    assert x.shape == shape
    return x


FAMILIES = ['normal', 'all equal', 'two values', 'lowest byte', 'highest byte', 'signs and zeros',
            'infinities and denormals', 'ascending', 'descending', 'ten percent nan', 'all-nan column',
            'single valid value']


def ranks_for(n_valid, r):
    """(r, d) ranks per column: 0, n_valid - 1, the middle, the middle again, -1, n_valid, then quartiles."""
    m = np.asarray(n_valid, dtype=np.int64)
    rows = [np.zeros_like(m), m - 1, m // 2, m // 2, np.full_like(m, -1), m, m // 4, (3 * m) // 4]
    return np.ascontiguousarray(np.stack(rows[:r]))
