"""The host side of ARHMM sampling (models/arhmm.py: generative, sample) and the float64 restatements the GPU tests
compare ``bn_arhmm_sample`` against (tests/arhmm_sample_refs.py).  No GPU."""

import ctypes

import numpy as np
import pytest

from behavenet_amd import _hip
from behavenet_amd.models.arhmm import ARHMM
from tests import arhmm_sample_refs as sr


@pytest.mark.parametrize('D,L,K', [(1, 0, 1), (3, 1, 5), (4, 2, 3), (7, 8, 32)])
def test_generative_against_the_counting_rule_and_cholesky(D, L, K):
    m = sr.shape_model(D, L, K)
    W, C, cdf0, cdf = m.generative()
    assert W.shape == (K, D, 1 + L * D) and C.shape == (K, D, D) and cdf0.shape == (K,) and cdf.shape == (K, K)
    assert all(a.dtype == np.float64 and a.flags['C_CONTIGUOUS'] for a in (W, C, cdf0, cdf))
    assert np.array_equal(W[:, :, 0], m.bs) and np.array_equal(W[:, :, 1:], m.As)
    for k in range(K):
        assert np.array_equal(C[k], np.linalg.cholesky(m.Sigmas[k]))
        np.testing.assert_allclose(C[k] @ C[k].T, m.Sigmas[k], rtol=1e-13, atol=1e-13)
    # the cumulative sums in state order, and what the counting rule makes of them: u in [cdf[j - 1], cdf[j]) is
    # state j, u at or past the last compared entry is state K - 1 even where the row sums below 1
    Ps, pi0 = np.exp(m.log_Ps), np.exp(m.log_pi0)
    for row, p in [(cdf0, pi0)] + [(cdf[k], Ps[k]) for k in range(K)]:
        acc = 0.0
        for j in range(K):
            acc += p[j]
            assert row[j] == acc
            lo = row[j - 1] if j else 0.0
            assert sr.count_state(lo, row) == j
            assert sr.count_state(0.5 * (lo + row[j]), row) == j
            if j < K - 1:
                assert sr.count_state(np.nextafter(row[j], 0.0), row) == j
        assert sr.count_state(np.nextafter(1.0, 0.0), row) == K - 1
        assert sr.count_state(0.0, row) == 0


def test_generative_rejects_an_indefinite_covariance():
    m = ARHMM(2, 2, lags=1)
    m.Sigmas[1] = np.asarray([[1.0, 2.0], [2.0, 1.0]])
    with pytest.raises(ValueError, match=r'Sigmas\[1\] is not positive definite'):
        m.generative()


@pytest.mark.parametrize('n,S,D,L,K', [(0, 0, 4, 1, 3), (10, 1, 1, 0, 1), (4000, 7, 16, 1, 16), (100, 3, 7, 8, 32),
                                       (60000, 50, 32, 1, 32), (5, 1000, 64, 0, 2)])
def test_the_workspace_is_the_offsets_an_int_a_trial_and_a_row_and_c_transposed(n, S, D, L, K):
    pad16 = lambda b: (b + 15) // 16 * 16
    want = pad16((S + 1) * 4) + pad16(S * 4) + pad16(n * 4) + K * D * D * 8
    assert _hip.load().bn_arhmm_sample_ws_bytes(n, S, D, L, K) == want


def test_the_query_refuses_what_the_call_refuses():
    lib = _hip.load()
    null = [None] * 5
    for n, S, D, L, K in ((10, 1, 4, 1, 33), (10, 1, 4, 1, 0), (10, 1, 4, 9, 2), (10, 1, 33, 1, 2), (10, 1, 65, 0, 2),
                          (10, 1, 0, 0, 2), (-1, 1, 4, 1, 2), (10, -1, 4, 1, 2), (10, 1, 4, -1, 2)):
        assert lib.bn_arhmm_sample_ws_bytes(n, S, D, L, K) == 0
        assert lib.bn_arhmm_sample(*null, S, D, L, K, n, None, None, None, None, D, None, None, None, 0, None) == -2
    # NULL operands with shapes that are served
    assert lib.bn_arhmm_sample(*null, 1, 4, 1, 2, 10, None, None, None, None, 4, None, None, None, 0, None) == -1

    # pointers that are never followed: every refusal below comes before any launch
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    p += -p % 16
    ops = [p] * 5
    need = lib.bn_arhmm_sample_ws_bytes(10, 1, 4, 1, 2)

    def call(u, states_in, init=None, ld=4, ws=p, ws_bytes=need, S=1, x=p):
        return lib.bn_arhmm_sample(*ops, S, 4, 1, 2, 10, p, u, states_in, init, ld, x, p, ws, ws_bytes, None)
    assert call(None, None) == -1                          # neither of u and states_in
    assert call(p, p) == -1                                # both
    assert call(p, None, x=None) == -1
    assert call(p, None, ws=None) == -1
    assert call(p, None, ws_bytes=need - 1) == -2          # a workspace that is too small
    assert call(p, None, init=p, ld=3) == -2               # a row stride below D
    assert call(p + 4, None) == -2 and call(p, None, ws=p + 8) == -2 and call(None, p + 2) == -2       # alignment
    assert call(p, None, S=0) == 0                         # no trials: nothing is launched


def test_sample_checks_the_dimensions_before_anything_else():
    m = ARHMM(3, 2, lags=1)
    m.K = 33
    with pytest.raises(ValueError, match='33 states'):
        m.sample(10)
    m.K, m.lags = 3, 9
    with pytest.raises(ValueError, match='9 lags'):
        m.sample(10)
    m.lags, m.D = 1, 33
    with pytest.raises(ValueError, match=r'\(lags \+ 1\) \* columns = 66'):
        m.sample(10)
    m.D = 2
    with pytest.raises(ValueError, match='burn_in -1'):
        m.sample(10, burn_in=-1)
    states, latents = m.sample(0, n_samples=2, burn_in=0)              # nothing to draw: no device is touched
    assert [s.shape for s in states] == [(0,)] * 2 and [x.shape for x in latents] == [(0, 2)] * 2


def test_arhmm_sample_has_no_cpu_fallback():
    import torch
    m = sr.shape_model(3, 1, 2)
    W, C, cdf0, cdf = m.generative()
    eps = torch.zeros((10, 3), dtype=torch.float64)
    with pytest.raises(ValueError, match='no CPU fallback'):
        _hip.arhmm_sample(W, C, cdf0, cdf, [0, 10], eps, u=torch.zeros(10, dtype=torch.float64))
    with pytest.raises(ValueError, match='float64'):
        _hip.arhmm_sample(W, C, cdf0, cdf, [0, 10], eps.float(), u=torch.zeros(10, dtype=torch.float64))


@pytest.mark.parametrize('K', sr.STATES)
@pytest.mark.parametrize('D,L', sr.SHAPES)
def test_the_restatements_agree(D, L, K):
    """A and B to 1e-10 of scale at every shape of the GPU tests, in both modes, with and without init: the noise floor
    the GPU tests take their bound from is real and small.  The companion matrices are stable."""
    m = sr.shape_model(D, L, K)
    W, C, cdf0, cdf = m.generative()
    assert sr.spectral_radii(W).max() < 0.99
    offsets, n, eps, u, init = sr.shape_noise(D, L, K)
    given = np.random.RandomState(D + L + K).randint(0, K, size=n).astype(np.int32)
    for kw in ({'u': u}, {'states': given}):
        for ini in (None, init[:, :D]):
            xa, za = sr.sample_a(W, C, cdf0, cdf, offsets, eps, init=ini, fill=-7.0, state_fill=-7, **kw)
            xb, zb = sr.sample_b(W, C, cdf0, cdf, offsets, eps, init=ini, fill=-7.0, state_fill=-7, **kw)
            scale = sr.sample_scale(W, C, offsets, eps, za, init=ini)
            assert np.array_equal(za, zb)
            assert np.all(np.isfinite(xa)) and np.all(np.abs(xa - xb) <= 1e-10 * scale)
            outside = np.ones(n, dtype=bool)
            outside[offsets[0]:offsets[-1]] = False
            assert np.all(xa[outside] == -7.0) and np.all(za[outside] == -7) and outside.sum() == 5
            if 'states' in kw:
                assert np.array_equal(za[~outside], given[~outside])


def test_the_restatements_make_a_bad_state_and_the_rest_of_its_trial_nan():
    m = sr.shape_model(3, 1, 5)
    W, C, cdf0, cdf = m.generative()
    offsets, n, eps, u, _ = sr.shape_noise(3, 1, 5)
    given = np.zeros(n, dtype=np.int32)
    bad = int(offsets[3]) + 10                              # row 10 of the trial of 37 rows
    given[bad] = 5
    for fn in (sr.sample_a, sr.sample_b):
        x, z = fn(W, C, cdf0, cdf, offsets, eps, states=given)
        expect = np.zeros(n, dtype=bool)
        expect[bad:offsets[4]] = True
        assert np.array_equal(np.isnan(x).all(axis=1), expect) and np.array_equal(np.isnan(x).any(axis=1), expect)
        assert z[bad] == 5
