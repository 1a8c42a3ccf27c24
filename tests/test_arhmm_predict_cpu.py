"""One-step-ahead predictions of an ARHMM without a GPU: the restatements of tests/arhmm_predict_refs.py against each
other and against a brute force over every state path, the properties the definitions promise, and the argument checks
of the two wrappers."""

import numpy as np
import pytest
import torch

from behavenet_amd import _hip
from behavenet_amd.models.arhmm import ARHMM
from tests import arhmm_predict_refs as prefs


def _random_hmm(rng, K):
    Ps = rng.rand(K, K) + 0.1
    Ps /= Ps.sum(axis=1, keepdims=True)
    pi0 = rng.rand(K) + 0.1
    pi0 /= pi0.sum()
    return np.log(Ps), np.log(pi0)


def _weights_of(rng, n, K):
    w = rng.rand(n, K)
    return w / w.sum(axis=1, keepdims=True)


@pytest.mark.parametrize('K,T', [(1, 4), (2, 6), (3, 5), (3, 1)])
def test_weight_refs_against_every_path(K, T):
    rng = np.random.RandomState(10 * K + T)
    log_Ps, log_pi0 = _random_hmm(rng, K)
    ll = -5.0 + 3.0 * rng.randn(T, K)
    brute = prefs.weights_brute_force(ll, log_Ps, log_pi0)
    for form in (prefs.weights_log, prefs.weights_scaled):
        w = form(ll, log_Ps, log_pi0)
        assert np.abs(w - brute).max() <= 1e-13
        assert np.abs(w.sum(axis=1) - 1.0).max() <= 1e-13
    assert np.array_equal(prefs.weights_log(ll, log_Ps, log_pi0)[0], np.exp(log_pi0))


def test_weight_refs_agree_on_long_trials_far_from_zero():
    rng = np.random.RandomState(3)
    K = 5
    log_Ps, log_pi0 = _random_hmm(rng, K)
    offsets = np.asarray([1, 1, 2, 302, 302], dtype=np.int64)
    ll = -1e4 + 50.0 * rng.rand(304, K)
    a = prefs.weights_table(ll, offsets, log_Ps, log_pi0, prefs.weights_log)
    b = prefs.weights_table(ll, offsets, log_Ps, log_pi0, prefs.weights_scaled)
    assert np.abs(a - b).max() <= 1e-12
    assert not a[0].any() and not a[302:].any()             # rows outside the trials
    assert np.abs(a[1:302].sum(axis=1) - 1.0).max() <= 1e-12


@pytest.mark.parametrize('form', [prefs.weights_log, prefs.weights_scaled])
def test_row_t_of_ll_does_not_reach_w_t(form):
    rng = np.random.RandomState(4)
    K, T = 4, 30
    log_Ps, log_pi0 = _random_hmm(rng, K)
    ll = rng.randn(T, K)
    w = form(ll, log_Ps, log_pi0)
    for t in (0, 7, T - 1):
        other = ll.copy()
        other[t] = 10.0 * rng.randn(K)
        w2 = form(other, log_Ps, log_pi0)
        assert np.array_equal(w2[:t + 1], w[:t + 1])
        if t + 1 < T:
            assert np.abs(w2[t + 1] - w[t + 1]).max() > 1e-3


def _regression(rng, K, D, L):
    return 0.5 * rng.randn(K, D, 1 + L * D)


def _offsets(L):
    return np.cumsum([2, 0, L, L + 1, 37, 0, 1]).astype(np.int64)


@pytest.mark.parametrize('D,L', [(1, 0), (3, 1), (5, 3)])
def test_prediction_refs_agree(D, L):
    rng = np.random.RandomState(D + L)
    K = 4
    offsets = _offsets(L)
    n = int(offsets[-1]) + 2
    table = rng.randn(n, D).astype(np.float32)
    W, w = _regression(rng, K, D, L), _weights_of(rng, n, K)
    a = prefs.predict_loop(table, offsets, W, w, L)
    b = prefs.predict_einsum(table, offsets, W, w, L)
    scale = prefs.predict_scale(table, offsets, W, w, L)
    assert np.all(np.abs(a - b) <= 1e-14 * scale)
    in_trial = np.zeros(n, dtype=bool)
    in_trial[offsets[0]:offsets[-1]] = True
    assert not a[~in_trial].any()
    for beg, end in prefs.trials_of(offsets):               # initial rows: the row's own values
        assert np.array_equal(a[beg:min(beg + L, end)], table[beg:min(beg + L, end)].astype(np.float64))


def test_one_state_is_the_plain_ar_regression():
    rng = np.random.RandomState(8)
    D, L, T = 3, 2, 40
    x = rng.randn(T, D).astype(np.float32)
    W = _regression(rng, 1, D, L)
    offsets = np.asarray([0, T], dtype=np.int64)
    w = prefs.weights_table(rng.randn(T, 1), offsets, np.zeros((1, 1)), np.zeros(1))
    assert np.array_equal(w, np.ones((T, 1)))
    assert np.array_equal(prefs.weights_table(rng.randn(T, 1), offsets, np.zeros((1, 1)), np.zeros(1),
                                              prefs.weights_scaled), np.ones((T, 1)))
    got = prefs.predict_einsum(x, offsets, W, w, L)
    x64 = x.astype(np.float64)
    for t in range(L, T):
        want = W[0][:, 0] + W[0][:, 1:1 + D] @ x64[t - 1] + W[0][:, 1 + D:] @ x64[t - 2]
        assert np.abs(got[t] - want).max() <= 1e-13


@pytest.mark.parametrize('form', [prefs.predict_loop, prefs.predict_einsum])
def test_one_hot_weights_select_that_state_s_regression(form):
    rng = np.random.RandomState(9)
    K, D, L, T = 3, 2, 1, 25
    x = rng.randn(T, D).astype(np.float32)
    W = _regression(rng, K, D, L)
    offsets = np.asarray([0, T], dtype=np.int64)
    states = rng.randint(K, size=T)
    got = form(x, offsets, W, np.eye(K)[states], L)
    for t in range(L, T):
        want = W[states[t]][:, 0] + W[states[t]][:, 1:] @ x[t - 1].astype(np.float64)
        assert np.abs(got[t] - want).max() <= 1e-14


def test_sums_and_scores_from_the_definitions():
    rng = np.random.RandomState(12)
    D, L = 2, 2
    offsets = _offsets(L)
    n = int(offsets[-1]) + 1
    x = np.cumsum(0.1 * rng.randn(n, D), axis=0).astype(np.float32)
    pred = x + 0.01 * rng.randn(n, D).astype(np.float32)
    sums, scale = prefs.prediction_sums(x, pred, offsets, L)
    valid = prefs.valid_rows(n, offsets, L)
    assert sums.shape == (2, len(offsets) - 1, D, 4) and np.all(scale >= np.abs(sums))
    assert sums[0, :, 0, 0].tolist() == [0, 0, 1, 35, 0, 0]   # rows with t >= max(L, 1)
    assert valid.sum() == 36
    s = 3
    rows = np.arange(offsets[s] + L, offsets[s + 1])
    x64 = x.astype(np.float64)
    sc = prefs.scores(sums)
    assert np.allclose(sc['mse'][0, s], np.mean((x64[rows] - pred[rows].astype(np.float64)) ** 2, axis=0), rtol=1e-12)
    assert np.allclose(sc['mse'][1, s], np.mean((x64[rows] - x64[rows - 1]) ** 2, axis=0), rtol=1e-12)
    ss_tot = np.sum((x64[rows] - x64[rows].mean(axis=0)) ** 2, axis=0)
    assert np.allclose(sc['r2'][1, s], 1.0 - np.sum((x64[rows] - x64[rows - 1]) ** 2, axis=0) / ss_tot, rtol=1e-9)
    # the host summary of the same sums: the same numbers, pooled ones from the added sums
    from behavenet_amd.fitting.eval import summarise_prediction_sums
    out = summarise_prediction_sums(sums)
    assert np.allclose(out['mse'][s], sc['mse'][0, s], rtol=1e-14) and np.allclose(out['r2'][s], sc['r2'][0, s])
    assert np.allclose(out['mse_persistence'][s], sc['mse'][1, s], rtol=1e-14)
    assert np.isnan(out['mse'][2]).all() and out['n'][2].tolist() == [1, 1]         # too few rows for a score
    tot = sums.sum(axis=1)
    assert np.allclose(out['pooled']['mse'], tot[0, :, 3] / tot[0, :, 0], rtol=1e-14)
    assert np.allclose(out['pooled']['mse_persistence'], tot[1, :, 3] / tot[1, :, 0], rtol=1e-14)
    assert np.isclose(out['pooled']['mse_all'], tot[0, :, 3].sum() / tot[0, :, 0].sum(), rtol=1e-14)
    ss = tot[0, :, 2] - tot[0, :, 1] ** 2 / tot[0, :, 0]
    assert np.isclose(out['pooled']['r2_all'], 1.0 - tot[0, :, 3].sum() / ss.sum(), rtol=1e-9)
    with pytest.raises(ValueError, match=r'\(2, S, D, 4\)'):
        summarise_prediction_sums(sums[0])


def test_both_entry_points_are_bound():
    for name in ('bn_hmm_predictive', 'bn_hmm_predictive_ws_bytes', 'bn_arhmm_predict', 'bn_arhmm_predict_ws_bytes'):
        assert name in _hip.SIGNATURES
    lib = _hip.load()
    assert lib.bn_hmm_predictive_ws_bytes(10, 3, 33) == 0 and lib.bn_hmm_predictive_ws_bytes(10, 3, 32) == 16
    assert lib.bn_arhmm_predict_ws_bytes(10, 3, 33, 1, 2) == 0 and lib.bn_arhmm_predict_ws_bytes(10, 3, 4, 9, 2) == 0
    # the offsets, one byte a row and the folded operand: K Q = 34 padded to 48 rows of D = 16 padded doubles
    assert lib.bn_arhmm_predict_ws_bytes(100, 3, 16, 1, 2) == 16 + 112 + 48 * 16 * 8
    assert lib.bn_hmm_predictive(None, None, 1, 2, 10, None, None, None, None, 0, None) == -1       # BN_E_BADARG
    assert lib.bn_arhmm_predict(None, 4, None, 1, 4, 1, 2, 10, None, None, None, None, 0, None) == -1
    assert lib.bn_arhmm_predict(None, 3, None, 1, 4, 1, 2, 10, None, None, None, None, 0, None) == -2  # ld < D


def test_argument_errors_of_the_wrappers():
    ll = torch.zeros((10, 2), dtype=torch.float64)
    with pytest.raises(ValueError, match='no CPU fallback'):
        _hip.hmm_predictive(ll, [0, 10], np.zeros((2, 2)), np.zeros(2))
    with pytest.raises(ValueError, match='float64'):
        _hip.hmm_predictive(ll.float(), [0, 10], np.zeros((2, 2)), np.zeros(2))
    with pytest.raises(ValueError, match='33 states'):
        _hip.hmm_predictive(torch.zeros((4, 33), dtype=torch.float64), [0, 4], np.zeros((33, 33)), np.zeros(33))
    table = torch.zeros((10, 3))
    W, w = np.zeros((2, 3, 4)), torch.zeros((10, 2), dtype=torch.float64)
    with pytest.raises(ValueError, match='no CPU fallback'):
        _hip.arhmm_predict(table, [0, 10], W, w, 1)
    with pytest.raises(ValueError, match='float32'):
        _hip.arhmm_predict(table.double(), [0, 10], W, w, 1)
    # (the limits of check_arhmm_dims are reached with a device table only: tests/test_gpu_arhmm_predict.py)
    with pytest.raises(ValueError, match="weights 'filtered' are not served"):
        ARHMM(2, 3).table_weights(table, [0, 10], weights='filtered')
