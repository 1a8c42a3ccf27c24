"""The yardstick of the uint8 reconstruction tests: the rounding rule as one numpy statement.

``u8 = NaN -> 0, else clamp(rint(x * 255), 0, 255)`` with the product in fp32 and rint to nearest even -- the IEEE
operations ``bn_unit_float_to_u8`` performs, so the device result is checked bit for bit."""

import numpy as np

# (value, grey level): ties go to the even level, everything outside [0, 1] saturates, NaN is black
SPECIALS = [(np.float32(0.5) / np.float32(255), 0), (np.float32(1.5) / np.float32(255), 2),
            (np.float32(2.5) / np.float32(255), 2), (np.float32(254.5) / np.float32(255), 254),
            (np.float32(-0.0), 0), (np.float32(-0.3), 0), (np.float32(-1e30), 0), (np.float32(-np.inf), 0),
            (np.float32(np.nan), 0), (np.float32(1.0), 255), (np.float32(1.002), 255), (np.float32(7.5), 255),
            (np.float32(3e38), 255), (np.float32(np.inf), 255), (np.float32(0.0), 0)]


def quantise_u8(x):
    """numpy array (any float dtype; the value is taken as fp32) -> uint8 of the same shape."""
    x = np.asarray(x).astype(np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        r = np.rint(x * np.float32(255))
        r = np.where(np.isnan(r), np.float32(0), np.clip(r, np.float32(0), np.float32(255)))
    return r.astype(np.uint8)


def with_specials(x, seed=0):
    """A copy of the flat fp32 array ``x`` with SPECIALS spliced in at random places (as many as fit)."""
    x = np.array(x, dtype=np.float32).reshape(-1)
    vals = np.array([v for v, _ in SPECIALS], dtype=np.float32)[:x.size]
    at = np.random.default_rng(seed).permutation(x.size)[:vals.size]
    x[at] = vals
    return x
