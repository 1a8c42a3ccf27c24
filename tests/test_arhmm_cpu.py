"""The host side of the ARHMM fit (models/arhmm.py) and the float64 restatements the GPU tests compare the kernels
against (tests/arhmm_refs.py).  No GPU."""

import pickle

import numpy as np
import pytest
import torch

from behavenet_amd import _hip
from behavenet_amd.models.arhmm import ARHMM
from tests import arhmm_refs as refs


def _random_hmm(rng, K):
    Ps = rng.rand(K, K) + 0.1
    Ps /= Ps.sum(axis=1, keepdims=True)
    pi0 = rng.rand(K) + 0.1
    pi0 /= pi0.sum()
    return np.log(Ps), np.log(pi0)


@pytest.mark.parametrize('K,T', [(2, 5), (2, 6), (3, 5), (3, 6)])
def test_refs_against_every_path(K, T):
    rng = np.random.RandomState(10 * K + T)
    log_Ps, log_pi0 = _random_hmm(rng, K)
    ll = 3.0 * rng.randn(T, K) - 20.0
    gamma, xi, Z, best, score = refs.brute_force(ll, log_Ps, log_pi0)
    for fb in (refs.fb_log, refs.fb_scaled):
        g, x, z = fb(ll, log_Ps, log_pi0)
        assert abs(z - Z) <= 1e-12 * abs(Z)
        np.testing.assert_allclose(g, gamma, rtol=0, atol=1e-13)
        np.testing.assert_allclose(x, xi, rtol=0, atol=1e-13)
        np.testing.assert_allclose(g.sum(axis=1), 1.0, rtol=0, atol=1e-13)
        np.testing.assert_allclose(x.sum(), T - 1.0, rtol=0, atol=1e-12)
    path, s = refs.viterbi(ll, log_Ps, log_pi0)
    assert abs(s - score) <= 1e-12 * abs(score)
    assert path.tolist() == best.tolist()
    assert abs(refs.path_score(ll, log_Ps, log_pi0, path) - score) <= 1e-12 * abs(score)


def test_viterbi_ref_ties_go_to_the_lowest_state():
    K, T = 3, 6
    ll = np.zeros((T, K))
    log_Ps, log_pi0 = np.full((K, K), -np.log(K)), np.full((K,), -np.log(K))
    assert refs.viterbi(ll, log_Ps, log_pi0)[0].tolist() == [0] * T
    assert refs.brute_force(ll, log_Ps, log_pi0)[3].tolist() == [0] * T


def test_fb_refs_on_short_and_empty_trials():
    log_Ps, log_pi0 = _random_hmm(np.random.RandomState(0), 3)
    for fb in (refs.fb_log, refs.fb_scaled):
        g, x, z = fb(np.zeros((0, 3)), log_Ps, log_pi0)
        assert g.shape == (0, 3) and not x.any() and z == 0.0
        ll = np.asarray([[-1.0, -2.0, -3.0]])
        g, x, z = fb(ll, log_Ps, log_pi0)
        assert not x.any()
        assert abs(z - refs.brute_force(ll, log_Ps, log_pi0)[2]) < 1e-13


def _model(rng, K, D, L, shift=True, **kw):
    m = ARHMM(K, D, lags=L, **kw)
    m.As = 0.3 * rng.randn(K, D, L * D)
    m.bs = rng.randn(K, D)
    for k in range(K):
        B = rng.randn(D, D)
        m.Sigmas[k] = B @ B.T / D + 0.2 * np.eye(D)
    m.log_Ps, m.log_pi0 = _random_hmm(rng, K)
    if shift:
        m.shift = rng.randn(D)
    return m


@pytest.mark.parametrize('D,L', [(1, 0), (3, 1), (4, 2), (2, 3)])
def test_fold_reproduces_the_direct_density(D, L):
    rng = np.random.RandomState(D + 7 * L)
    m = _model(rng, 3, D, L)
    offsets = [0, 0, L, 2 * L + 1, 2 * L + 30]
    table = (rng.randn(offsets[-1], D) + 2.0).astype(np.float32)
    G, cst = m.fold()
    assert G.shape == (3, D, m.P) and cst.shape == (3,)
    direct = refs.loglik_direct(table, offsets, m.As, m.bs, m.Sigmas, L)
    folded = refs.loglik_folded(table, offsets, G, cst, L, m.shift)
    np.testing.assert_allclose(folded, direct, rtol=1e-11, atol=1e-11)


def test_fold_rejects_an_indefinite_covariance():
    m = ARHMM(2, 2, lags=1)
    m.Sigmas[1] = np.asarray([[1.0, 2.0], [2.0, 1.0]])
    with pytest.raises(ValueError, match=r'Sigmas\[1\] is not positive definite'):
        m.fold()


@pytest.mark.parametrize('D,L', [(2, 0), (3, 1), (2, 2)])
def test_m_step_against_weighted_least_squares(D, L):
    rng = np.random.RandomState(3 + D + L)
    K, T = 2, 300
    m = ARHMM(K, D, lags=L, l2_penalty_A=0.0, l2_penalty_b=0.0, transitions='sticky', kappa=5.0, alpha=2.0)
    m.shift = rng.randn(D)
    x = (rng.randn(T, D).cumsum(axis=0) * 0.1 + 1.0).astype(np.float32)
    offsets = [0, 140, T]
    gamma = rng.rand(T, K)
    gamma /= gamma.sum(axis=1, keepdims=True)
    mom, _ = refs.moments(x, offsets, gamma, L, m.shift)
    xi_sum, g0 = rng.rand(K, K) * 10, rng.rand(K)
    m.m_step(mom, xi_sum, g0)
    # the same fit from the rows themselves, in the un-shifted coordinates
    rows, ys, ws = [], [], []
    for beg, end in refs.trials_of(offsets):
        for t in range(beg + L, end):
            rows.append(np.concatenate([[1.0]] + [x[t - 1 - l].astype(np.float64) for l in range(L)]))
            ys.append(x[t].astype(np.float64))
            ws.append(gamma[t])
    rows, ys, ws = np.asarray(rows), np.asarray(ys), np.asarray(ws)
    for k in range(K):
        sw = np.sqrt(ws[:, k])[:, None]
        W = np.linalg.lstsq(rows * sw, ys * sw, rcond=None)[0].T
        np.testing.assert_allclose(m.bs[k], W[:, 0], rtol=1e-8, atol=1e-8)
        np.testing.assert_allclose(m.As[k], W[:, 1:], rtol=1e-8, atol=1e-8)
        res = ys - rows @ W.T
        scatter = (res * ws[:, k:k + 1]).T @ res
        Sigma = (scatter + m.Psi0 * np.eye(D)) / (ws[:, k].sum() + m.nu0 + D + 1)
        np.testing.assert_allclose(m.Sigmas[k], Sigma, rtol=1e-8, atol=1e-10)
        assert np.array_equal(m.Sigmas[k], m.Sigmas[k].T)
    Ps = xi_sum + 5.0 * np.eye(K) + 1.0
    np.testing.assert_allclose(np.exp(m.log_Ps), Ps / Ps.sum(axis=1, keepdims=True), rtol=1e-13)
    np.testing.assert_allclose(np.exp(m.log_pi0), (g0 + 1e-8) / (g0 + 1e-8).sum(), rtol=1e-13)


def test_m_step_keeps_a_state_without_data():
    m = ARHMM(2, 2, lags=1)
    before = (m.As.copy(), m.bs.copy(), m.Sigmas.copy())
    mom = np.zeros((2, m.P, m.P))
    mom[0] = np.eye(m.P) * 50.0
    mom[1, 0, 0] = 2.5                                      # fewer than D + 1 expected rows
    m.m_step_observations(mom)
    assert np.array_equal(m.As[1], before[0][1]) and np.array_equal(m.bs[1], before[1][1])
    assert np.array_equal(m.Sigmas[1], before[2][1])
    assert not np.array_equal(m.Sigmas[0], before[2][0])


def test_em_objective_of_the_reference_iteration_does_not_decrease():
    rng = np.random.RandomState(5)
    K, D, L = 3, 2, 1
    datas, _ = refs.sample_arhmm(rng, K, D, L, [60, 45, 80])
    table = np.concatenate(datas)
    offsets = np.cumsum([0] + [len(d) for d in datas])
    m = _model(np.random.RandomState(6), K, D, L, shift=False, transitions='sticky', kappa=2.0, alpha=1.5,
               l2_penalty_A=1e-3, l2_penalty_b=1e-3, nu0=0.5, Psi0=0.1)
    m.shift = table.mean(axis=0).astype(np.float64)
    objective = []
    for _ in range(10):
        prior = m.log_prior()
        lls = refs.em_iteration(m, table, offsets)
        objective.append(float(lls.sum()) + prior)
    objective.append(float(refs.trial_logliks(m, table, offsets).sum()) + m.log_prior())
    steps = np.diff(objective)
    assert np.all(steps >= -1e-9 * np.abs(objective[:-1])), objective
    assert objective[-1] > objective[0] + 1.0


def test_pickle_round_trip_holds_numpy_members_only():
    m = _model(np.random.RandomState(1), 3, 2, 2, transitions='sticky', kappa=10.0)
    for v in vars(m).values():
        assert isinstance(v, (int, float, str, np.ndarray)), type(v)
    m2 = pickle.loads(pickle.dumps(m))
    for name in ('As', 'bs', 'Sigmas', 'log_Ps', 'log_pi0', 'shift'):
        assert np.array_equal(getattr(m, name), getattr(m2, name))
    assert (m2.K, m2.D, m2.lags, m2.transitions, m2.kappa) == (3, 2, 2, 'sticky', 10.0)
    assert m2.As.shape == (3, 2, 4) and m2.bs.shape == (3, 2) and m2.Sigmas.shape == (3, 2, 2)
    assert m2.log_Ps.shape == (3, 3) and m2.log_pi0.shape == (3,)


def test_permute_relabels_the_states():
    rng = np.random.RandomState(2)
    m = _model(rng, 3, 2, 1)
    table = rng.randn(40, 2).astype(np.float32)
    offsets = [0, 25, 40]
    before = refs.trial_logliks(m, table, offsets)
    old = pickle.loads(pickle.dumps(m))
    perm = [2, 0, 1]
    m.permute(perm)
    for k, src in enumerate(perm):
        assert np.array_equal(m.As[k], old.As[src]) and np.array_equal(m.Sigmas[k], old.Sigmas[src])
        assert m.log_pi0[k] == old.log_pi0[src]
        for j, srcj in enumerate(perm):
            assert m.log_Ps[k, j] == old.log_Ps[src, srcj]
    np.testing.assert_allclose(refs.trial_logliks(m, table, offsets), before, rtol=1e-12)


def test_types_that_are_not_served_are_named():
    for kw in ({'transitions': 'recurrent'}, {'transitions': 'recurrent_only'}, {'observations': 'studentst'},
               {'observations': 'diagonal_ar'}, {'observations': 'diagonal_robust_ar'}):
        with pytest.raises(NotImplementedError, match=list(kw.values())[0]):
            ARHMM(2, 2, **kw)
    with pytest.raises(NotImplementedError, match='sgd'):
        ARHMM(2, 2).fit([np.zeros((5, 2))], method='sgd')
    assert ARHMM(2, 3, lags=4, observations='gaussian').lags == 0


def test_limits_are_checked_before_a_launch():
    with pytest.raises(ValueError, match='33 states'):
        ARHMM(33, 2)
    with pytest.raises(ValueError, match='9 lags'):
        ARHMM(2, 2, lags=9)
    with pytest.raises(ValueError, match=r'\(lags \+ 1\) \* columns = 66'):
        ARHMM(2, 33, lags=1)
    table = torch.zeros((10, 3))
    G, cst = np.zeros((2, 3, 7)), np.zeros(2)
    with pytest.raises(ValueError, match='no CPU fallback'):
        _hip.arhmm_loglik(table, [0, 10], G, cst, 1)
    with pytest.raises(ValueError, match='float32'):
        _hip.arhmm_loglik(table.double(), [0, 10], G, cst, 1)
    with pytest.raises(ValueError, match='no CPU fallback'):
        _hip.arhmm_moments(table, [0, 10], torch.zeros((10, 2), dtype=torch.float64), 1)
    ll = torch.zeros((10, 2), dtype=torch.float64)
    for fn in (_hip.hmm_forward_backward, _hip.hmm_viterbi):
        with pytest.raises(ValueError, match='no CPU fallback'):
            fn(ll, [0, 10], np.zeros((2, 2)), np.zeros(2))
        with pytest.raises(ValueError, match='float64'):
            fn(ll.float(), [0, 10], np.zeros((2, 2)), np.zeros(2))
        with pytest.raises(ValueError, match='33 states'):
            fn(torch.zeros((4, 33), dtype=torch.float64), [0, 4], np.zeros((33, 33)), np.zeros(33))


@pytest.mark.parametrize('n,D,L,K', [(0, 4, 1, 3), (1, 1, 0, 1), (511, 3, 1, 2), (513, 3, 1, 2), (4000, 16, 1, 16),
                                     (100000, 32, 1, 32), (2000000, 8, 7, 32), (3000, 7, 8, 5)])
def test_the_restated_plan_is_the_library_s(n, D, L, K):
    lib = _hip.load()
    S = 7
    blocks, rows = _hip._arhmm_moments_plan(n, D, L, K)
    P = 1 + (L + 1) * D
    pad16 = lambda b: (b + 15) // 16 * 16
    assert blocks * K * P * P * 8 <= 60 << 20
    assert blocks == 0 or (blocks - 1) * rows < n <= blocks * rows
    assert lib.bn_arhmm_moments_ws_bytes(n, S, D, L, K) == pad16((S + 1) * 4) + pad16(n) + blocks * K * P * P * 8
    assert lib.bn_arhmm_loglik_ws_bytes(n, S, D, L, K) == pad16((S + 1) * 4) + pad16(n)
    assert lib.bn_hmm_forward_backward_ws_bytes(n, S, K) == pad16((S + 1) * 4) + 16 * n
    assert lib.bn_hmm_viterbi_ws_bytes(n, S, K) == pad16((S + 1) * 4) + pad16(n * K)


def test_the_queries_refuse_what_the_calls_refuse():
    lib = _hip.load()
    for args in ((10, 1, 4, 1, 33), (10, 1, 4, 9, 2), (10, 1, 33, 1, 2), (10, 1, 0, 0, 2), (-1, 1, 4, 1, 2),
                 (10, -1, 4, 1, 2)):
        assert lib.bn_arhmm_loglik_ws_bytes(*args) == 0 and lib.bn_arhmm_moments_ws_bytes(*args) == 0
        assert lib.bn_arhmm_loglik(None, 4, None, None, *args[1:], args[0], None, None, None, None, 0, None) == -2
    assert lib.bn_hmm_viterbi_ws_bytes(10, 1, 33) == 0 and lib.bn_hmm_forward_backward_ws_bytes(10, 1, 0) == 0
    # NULL operands with shapes that are served
    assert lib.bn_arhmm_loglik(None, 4, None, None, 1, 4, 1, 2, 10, None, None, None, None, 0, None) == -1
    assert lib.bn_hmm_forward_backward(None, None, 1, 2, 10, None, None, 1, None, None, None, None, 0, None) == -1
    assert lib.bn_hmm_viterbi(None, None, 1, 2, 10, None, None, None, None, 0, None) == -1
    assert lib.bn_arhmm_moments(None, 4, None, None, 1, 4, 1, 2, 10, None, None, None, None, 0, None) == -1
