"""Exact multi-step forecasts of an ARHMM without a GPU: ``ARHMM.forecast_maps`` against an enumeration of every state
path, the restatements of tests/arhmm_forecast_refs.py against each other, the host summaries on hand-made sums, the
``fit()`` hook's check and the C ABI's argument rules."""

import csv

import numpy as np
import pytest
import torch

from behavenet_amd import _hip
from behavenet_amd.fitting.eval import (check_export_arhmm_forecasts, summarise_forecast_sums,
                                        summarise_prediction_sums, write_forecasts_csv)
from behavenet_amd.models.arhmm import ARHMM
from tests import arhmm_forecast_refs as frefs


def _model(rng, K, D, L, identity=False):
    m = ARHMM(K, D, lags=L)
    m.As = 0.6 / max(L, 1) * rng.randn(K, D, L * D)
    m.bs = rng.randn(K, D)
    Ps = np.eye(K) if identity else rng.rand(K, K) + 0.1
    Ps /= Ps.sum(axis=1, keepdims=True)
    with np.errstate(divide='ignore'):
        m.log_Ps = np.log(Ps)
    return m


@pytest.mark.parametrize('K,D,L,H', [(2, 3, 1, 4), (3, 2, 2, 4), (3, 2, 3, 3), (3, 2, 0, 3)])
def test_forecast_maps_against_every_state_path(K, D, L, H):
    rng = np.random.RandomState(1000 * K + 100 * D + 10 * L + H)
    m = _model(rng, K, D, L)
    N = m.forecast_maps(H)
    W = m.generative()[0]
    assert N.shape == (H, K, D, 1 + L * D) and N.dtype == np.float64
    assert np.array_equal(N[0], W)                          # element for element
    Ps = np.exp(m.log_Ps)
    worst = 0.0
    for _ in range(3):
        w = rng.rand(K)
        w /= w.sum()
        phi = np.concatenate([[1.0], rng.randn(L * D)])
        brute, scale = frefs.forecast_brute_force(W, Ps, w, phi, H)
        got = np.einsum('k,hkdq,q->hd', w, N, phi)
        assert np.all(np.abs(got - brute) <= 1e-13 * scale)
        worst = max(worst, float(np.max(np.abs(got - brute) / scale)))
    # a one-hot weight is the map of that state alone
    for k in range(K):
        brute, scale = frefs.forecast_brute_force(W, Ps, np.eye(K)[k], phi, H)
        assert np.all(np.abs(N[:, k] @ phi - brute) <= 1e-13 * scale)
    print('forecast_maps K=%d D=%d L=%d H=%d: largest error / sum |terms| %.2e' % (K, D, L, H, worst))


@pytest.mark.parametrize('D,L', [(3, 1), (2, 3)])
def test_without_transitions_the_map_is_the_power_of_the_state_s_own_companion(D, L):
    rng = np.random.RandomState(D + L)
    K, H, Q = 3, 5, 1 + L * D
    m = _model(rng, K, D, L, identity=True)
    N = m.forecast_maps(H)
    W = m.generative()[0]
    for k in range(K):
        C = np.zeros((Q, Q))
        C[0, 0] = 1.0
        C[1:1 + D] = W[k]
        C[1 + D:, 1:1 + (L - 1) * D] = np.eye((L - 1) * D)
        power = np.eye(Q)
        for h in range(H):
            power = C @ power
            assert np.abs(N[h, k] - power[1:1 + D]).max() <= 1e-13 * max(np.abs(power).max(), 1.0)


def test_without_lags_the_map_is_the_reach_of_the_biases():
    rng = np.random.RandomState(5)
    m = _model(rng, 4, 3, 0)
    N = m.forecast_maps(6)
    P = np.exp(m.log_Ps)
    for h in range(6):
        assert np.abs(N[h, :, :, 0] - np.linalg.matrix_power(P, h) @ m.bs).max() <= 1e-14


def test_forecast_maps_refuses():
    m = _model(np.random.RandomState(0), 2, 3, 1)
    for bad in (0, 33, -1, 2.0, '3', None, True):
        with pytest.raises(ValueError, match='horizons'):
            m.forecast_maps(bad)
    assert m.forecast_maps(32).shape == (32, 2, 3, 4)
    assert m.forecast_maps(np.int64(2)).shape == (2, 2, 3, 4)
    m.As = m.As * 1e60                                      # spectral radius far above 1: 1e60^h leaves float64
    with pytest.raises(ValueError, match=r'horizon \d+ is not finite'):
        m.forecast_maps(32)
    m.forecast_maps(2)
    m.bs[1, 0] = np.nan
    with pytest.raises(ValueError, match='horizon 1 is not finite'):
        m.forecast_maps(1)


def _offsets(L):
    return np.cumsum([2, 0, L, L + 1, 37, 0, 1]).astype(np.int64)


@pytest.mark.parametrize('D,L,H', [(1, 0, 3), (3, 1, 5), (2, 3, 40)])
def test_forecast_refs_agree_and_follow_the_validity_rule(D, L, H):
    rng = np.random.RandomState(D + L + H)
    K = 3
    offsets = _offsets(L)
    n = int(offsets[-1]) + 2
    table = rng.randn(n, D).astype(np.float32)
    N = 0.5 * rng.randn(H, K, D, 1 + L * D)
    w = rng.rand(n, K)
    w /= w.sum(axis=1, keepdims=True)
    a = frefs.forecast_loop(table, offsets, N, w, L)
    b = frefs.forecast_einsum(table, offsets, N, w, L)
    assert np.abs(a - b).max() <= 1e-13 * (1 + L * D)
    assert np.abs(a - frefs.forecast_loop_trials(table, offsets, N, w, L)).max() <= 1e-13 * (1 + L * D)
    sums, scale = frefs.forecast_sums(table, a, offsets, L)
    assert sums.shape == (H, len(offsets) - 1, D, 5) and np.all(scale >= np.abs(sums))
    m = max(L, 1)
    for s, (beg, end) in enumerate(zip(offsets[:-1], offsets[1:])):
        for h in range(1, H + 1):
            assert sums[h - 1, s, 0, 0] == max(int(end - beg) - m - (h - 1), 0)
    # h = 1 is the one-step sums of the same forecasts
    from tests.arhmm_predict_refs import prediction_sums
    one, _ = prediction_sums(table, a[:, 0], offsets, L)
    both = frefs.as_model_and_persistence(sums)
    assert both.shape == (2, H, len(offsets) - 1, D, 4)
    assert np.allclose(both[:, 0], one, rtol=1e-13, atol=0)


def _hand_made_sums():
    """(2, H = 3, S = 2, D = 2, 4): the model's error grows with the horizon and passes the baseline's at h = 3."""
    H, S, D = 3, 2, 2
    sums = np.zeros((2, H, S, D, 4))
    for h in range(H):
        n = 20.0 - h
        sums[:, h, :, :, 0] = n
        sums[:, h, :, :, 1] = 2.0 * n                         # mean 2
        sums[:, h, :, :, 2] = 4.0 * n + 3.0 * n               # variance 3
        sums[0, h, :, :, 3] = n * (0.5 + 0.5 * h)             # mse 0.5, 1.0, 1.5
        sums[1, h, :, :, 3] = n * 1.25
    sums[:, :, 1, :, 0] = 5.0                                 # (a trial with too few rows for a score)
    return sums


def test_summarise_forecast_sums_and_the_csv(tmp_path):
    sums = _hand_made_sums()
    out = summarise_forecast_sums(sums)
    assert out['n'].shape == out['mse'].shape == out['r2_persistence'].shape == (3, 2, 2)
    assert np.allclose(out['mse'][:, 0, 0], [0.5, 1.0, 1.5]) and np.allclose(out['mse_persistence'][:, 0, 0], 1.25)
    assert np.allclose(out['r2'][:, 0, 0], 1.0 - np.asarray([0.5, 1.0, 1.5]) / 3.0)
    assert np.isnan(out['mse'][:, 1]).all() and out['n'][0, 1].tolist() == [5, 5]
    for h in range(3):
        one = summarise_prediction_sums(sums[:, h])
        assert np.array_equal(out['mse'][h], one['mse'], equal_nan=True)
        assert np.array_equal(out['pooled']['r2'][h], one['pooled']['r2'])
        assert out['pooled']['mse_all'][h] == one['pooled']['mse_all']
    assert out['pooled']['mse'].shape == (3, 2) and out['pooled']['mse_all'].shape == (3,)
    assert out['horizon_of_no_gain'] == 3
    better = sums.copy()
    better[0, ..., 3] *= 0.1
    assert summarise_forecast_sums(better)['horizon_of_no_gain'] is None
    worse = sums.copy()
    worse[0, ..., 3] = worse[1, ..., 3]                     # a tie is no gain
    assert summarise_forecast_sums(worse)['horizon_of_no_gain'] == 1
    with pytest.raises(ValueError, match=r'\(2, H, S, D, 4\)'):
        summarise_forecast_sums(sums[:, 0])
    out.update({'session': np.asarray([0, 1]), 'trial': np.asarray([7, 3])})
    path = str(tmp_path / 'f.csv')
    write_forecasts_csv(path, out)
    with open(path, newline='') as f:
        rows = list(csv.reader(f))
    assert rows[0] == ['Horizon', 'Session', 'Trial', 'Dim', 'N', 'MSE', 'R2', 'MSE_persistence', 'R2_persistence']
    assert len(rows) == 1 + 3 * 2 * 2
    assert rows[1][:5] == ['1', '0', '7', '0', '20']
    assert [float(v) for v in rows[1][5:]] == [float(out[k][0, 0, 0]) for k in ('mse', 'r2', 'mse_persistence',
                                                                                'r2_persistence')]
    assert rows[3] == ['1', '1', '3', '0', '5', '', '', '', '']
    assert rows[1 + 2 * 4 + 1][:5] == ['3', '0', '7', '1', '18']


def test_check_export_arhmm_forecasts():
    who = "fit: hparams['export_arhmm_forecasts']"
    check_export_arhmm_forecasts(who, {'horizons': 10})
    check_export_arhmm_forecasts(who, {'horizons': 32, 'dtype': ['train', 'test']}, {'n_states': 2})
    for bad in (10, {}, {'dtype': 'test'}, {'horizons': 3, 'weights': 'smoothed'}):
        with pytest.raises(ValueError, match='expected a dict with horizons'):
            check_export_arhmm_forecasts(who, bad)
    for bad in (0, 33, 2.5, '4'):
        with pytest.raises(ValueError, match='horizons'):
            check_export_arhmm_forecasts(who, {'horizons': bad})
    with pytest.raises(ValueError, match='dtype must be'):
        check_export_arhmm_forecasts(who, {'horizons': 3, 'dtype': 'all'})
    with pytest.raises(ValueError, match="hparams\\['export_arhmm'\\] fits, and that key is not set"):
        check_export_arhmm_forecasts(who, {'horizons': 3}, None)


def test_the_entry_point_is_bound():
    for name in ('bn_arhmm_forecast_sums', 'bn_arhmm_forecast_sums_ws_bytes'):
        assert name in _hip.SIGNATURES
    lib = _hip.load()
    q = lib.bn_arhmm_forecast_sums_ws_bytes
    assert q(10, 3, 4, 1, 33, 2) == 0 and q(10, 3, 4, 9, 2, 2) == 0 and q(10, 3, 4, 1, 2, 33) == 0
    assert q(10, 3, 4, 1, 2, 0) == 0 and q(10, 3, 33, 1, 2, 2) == 0
    # the offsets and the block plan (16 bytes each at S = 3); N folded: K Q = 34 padded to 48 rows of H D = 160 padded
    # to 192 doubles; one (H, D, 5) partial for each of 1000 // 256 + 3 row blocks at most
    assert q(1000, 3, 16, 1, 2, 10) == 2 * 16 + 48 * 192 * 8 + 6 * 10 * 16 * 5 * 8
    assert q(2, 3, 16, 1, 2, 10) == 2 * 16 + 48 * 192 * 8 + 2 * 10 * 16 * 5 * 8         # (a block holds a row at least)
    f = lib.bn_arhmm_forecast_sums
    assert f(None, 4, None, 1, 4, 1, 2, 3, 10, None, None, None, None, 0, None) == -1     # BN_E_BADARG
    assert f(None, 3, None, 1, 4, 1, 2, 3, 10, None, None, None, None, 0, None) == -2     # ld < D
    assert f(None, 4, None, 1, 4, 1, 2, 33, 10, None, None, None, None, 0, None) == -2    # H = 33
    assert f(None, 4, None, 1, 4, 1, 33, 3, 10, None, None, None, None, 0, None) == -2


def test_argument_errors_of_the_wrapper_and_the_model():
    table = torch.zeros((10, 3))
    N, w = np.zeros((2, 2, 3, 4)), torch.zeros((10, 2), dtype=torch.float64)
    with pytest.raises(ValueError, match='no CPU fallback'):
        _hip.arhmm_forecast_sums(table, [0, 10], N, w, 1)
    with pytest.raises(ValueError, match='float32'):
        _hip.arhmm_forecast_sums(table.double(), [0, 10], N, w, 1)
    with pytest.raises(ValueError, match="weights 'smoothed' are not served"):
        ARHMM(2, 3).forecast_sums(table, [0, 10], 4, weights='smoothed')
    with pytest.raises(ValueError, match='horizons'):
        ARHMM(2, 3).forecast_sums(table, [0, 10], 40)
