"""One-step-ahead predictions of an ARHMM on the device (bn_hmm_predictive, bn_arhmm_predict in csrc/arhmm.hip,
ARHMM.table_predictions / prediction_sums, fitting.eval.arhmm_predictions) against the float64 restatements of
tests/arhmm_predict_refs.py.

Tolerances for the two kernels: the rule of tests/test_gpu_arhmm.py (its ``_held``).  Everything is float64, the two
INDEPENDENT restatements (log-space and scaled weights; looped and einsum predictions) give the noise floor at the
shape, the device's bound is 100 x their disagreement and never less than 1e-12 of the quantity's scale: 1 for the
weights, ``sum_k |w_k| sum_q |W_k[d, q] phi[q]|`` for the predictions.  The bound comes from the restatements alone;
every check prints error, bound and their ratio.  ``prediction_sums`` is held against numpy sums over the device's OWN
fp32-rounded predictions (the reduction alone) at 1e-12 of ``sum |terms|``, the segment-sum tests' scale.

Largest error / bound seen on an MI355X (first run of this file): weights 0.004 (absorbing transitions; 0.000 to
0.001 otherwise), weight row sums 0.001, xhat 0.001 at every shape, the whole chain of ``table_predictions`` 0.001
with predictive and 0.010 with smoothed weights, prediction_sums 0.001 -- the device sits at the restatements' own
noise floor (error / noise about 1) everywhere.
"""

import csv
import os

import numpy as np
import pytest
import torch

from behavenet_amd import _hip
from behavenet_amd.models.arhmm import ARHMM
from tests import arhmm_predict_refs as prefs
from tests import arhmm_refs as refs
from tests.test_gpu_arhmm import _held, _model, _offsets, _random_hmm

pytestmark = pytest.mark.gpu
DEV = 'cuda'


# ------------------------------------------------------------------------------------------------------------
# bn_hmm_predictive
# ------------------------------------------------------------------------------------------------------------
PRED_LENGTHS = [0, 1, 2, 65, 257, 3000, 0]


@pytest.fixture(scope='module')
def pred_tables():
    """ll in [-1e4, -1e4 + 50] per K with two rows in front that belong to no trial (never written)."""
    out = {}
    offsets = np.cumsum([2] + PRED_LENGTHS).astype(np.int64)
    for K in (1, 2, 5, 32):
        rng = np.random.RandomState(K)
        out[K] = (-1e4 + 50.0 * rng.rand(int(offsets[-1]) + 2, K), offsets)
    return out


@pytest.mark.parametrize('kind', ['random', 'uniform', 'absorbing'])
@pytest.mark.parametrize('K', [1, 2, 5, 32])
def test_predictive_weights(pred_tables, K, kind):
    ll, offsets = pred_tables[K]
    log_Ps, log_pi0 = _random_hmm(np.random.RandomState(K + 70), K, kind)
    w1 = prefs.weights_table(ll, offsets, log_Ps, log_pi0, prefs.weights_log)
    w2 = prefs.weights_table(ll, offsets, log_Ps, log_pi0, prefs.weights_scaled)
    ll_d = torch.from_numpy(ll).to(DEV)
    n = ll.shape[0]
    out = torch.full((n, K), -7.0, dtype=torch.float64, device=DEV)
    got_d = _hip.hmm_predictive(ll_d, offsets, log_Ps, log_pi0, out=out)
    assert got_d is out
    got = got_d.cpu().numpy()
    in_trial = np.zeros(n, dtype=bool)
    in_trial[offsets[0]:offsets[-1]] = True
    assert np.all(got[~in_trial] == -7.0)                   # rows of no trial keep the sentinel
    tag = 'K=%d %s' % (K, kind)
    _held('weights ' + tag, np.abs(got - w1)[in_trial], np.abs(w1 - w2).max(), 1.0)
    _held('weight row sums ' + tag, np.abs(got[in_trial].sum(axis=1) - 1.0),
          np.abs(w1.sum(axis=1)[in_trial] - w2.sum(axis=1)[in_trial]).max(), 1.0)
    # the first row is the initial distribution itself: one exp a value, the device's and numpy's each within one
    # unit in the last place of the true value
    for beg, end in refs.trials_of(offsets):
        if end > beg:
            assert np.all(np.abs(got[beg] - np.exp(log_pi0)) <= 2.0 ** -51 * np.exp(log_pi0))
    again = _hip.hmm_predictive(ll_d, offsets, log_Ps, log_pi0).cpu().numpy()
    assert np.array_equal(again[in_trial], got[in_trial])   # the same bits on a second call
    assert not again[~in_trial].any()                       # (a fresh out: zeros)


@pytest.mark.parametrize('K', [2, 5, 32])
def test_row_t_of_ll_does_not_reach_w_t_and_a_nan_row_poisons_the_later_rows_of_its_trial(K):
    rng = np.random.RandomState(K + 5)
    offsets = np.asarray([1, 70, 71, 200, 330], dtype=np.int64)
    n = 331
    ll = -50.0 + 10.0 * rng.rand(n, K)
    log_Ps, log_pi0 = _random_hmm(rng, K)
    clean = _hip.hmm_predictive(torch.from_numpy(ll).to(DEV), offsets, log_Ps, log_pi0).cpu().numpy()
    # another row t: w up to and including row t keeps its bits, the next row moves
    other = ll.copy()
    other[150] = -50.0 + 10.0 * rng.rand(K)
    moved = _hip.hmm_predictive(torch.from_numpy(other).to(DEV), offsets, log_Ps, log_pi0).cpu().numpy()
    assert np.array_equal(moved[:151], clean[:151]) and np.array_equal(moved[200:], clean[200:])
    assert np.abs(moved[151] - clean[151]).max() > 1e-6
    # NaN rows: mid-trial (one entry), a trial's last row, a one-row trial, a trial's first row (every entry), and Inf
    bad = ll.copy()
    bad[30, rng.randint(K)] = np.nan
    bad[199, 0] = np.nan
    bad[70, :] = np.nan
    bad[200, :] = np.nan
    expect = np.zeros(n, dtype=bool)
    expect[31:70] = True
    expect[201:330] = True
    got = _hip.hmm_predictive(torch.from_numpy(bad).to(DEV), offsets, log_Ps, log_pi0).cpu().numpy()
    assert np.array_equal(~np.isfinite(got).all(axis=1), expect)
    assert np.array_equal(~np.isfinite(got).any(axis=1), expect)      # all K values of such a row
    assert np.array_equal(got[~expect], clean[~expect])
    inf = ll.copy()
    inf[250, K - 1] = np.inf
    got = _hip.hmm_predictive(torch.from_numpy(inf).to(DEV), offsets, log_Ps, log_pi0).cpu().numpy()
    assert np.isfinite(got[:251]).all() and not np.isfinite(got[251:330]).any() and np.isfinite(got[330:]).all()


# ------------------------------------------------------------------------------------------------------------
# bn_arhmm_predict
# ------------------------------------------------------------------------------------------------------------
def _weights_of(rng, n, K):
    w = rng.rand(n, K)
    return w / w.sum(axis=1, keepdims=True)


@pytest.mark.parametrize('K', [1, 2, 5, 17, 32])
@pytest.mark.parametrize('D,L', [(1, 0), (3, 1), (16, 1), (17, 1), (32, 1), (12, 4), (7, 8)])
def test_predict(D, L, K):
    rng = np.random.RandomState(2000 + 100 * D + 10 * L + K)
    offsets = _offsets(L)                                   # trials of 0, L, L + 1, 37, 150, 0 and 1 rows after two
    n = int(offsets[-1]) + 3
    wide = torch.from_numpy((rng.randn(n, D + 3) + 1.5).astype(np.float32)).to(DEV)
    W = rng.randn(K, D, 1 + L * D) / np.sqrt(1 + L * D)
    w = _weights_of(rng, n, K)
    w_d = torch.from_numpy(w).to(DEV)
    in_trial = np.zeros(n, dtype=bool)
    in_trial[offsets[0]:offsets[-1]] = True
    initial = np.zeros(n, dtype=bool)
    for beg, end in refs.trials_of(offsets):
        initial[beg:min(beg + L, end)] = True
    host = wide[:, :D].cpu().numpy()
    looped = prefs.predict_loop(host, offsets, W, w, L)
    other = prefs.predict_einsum(host, offsets, W, w, L)
    scale = prefs.predict_scale(host, offsets, W, w, L)
    noise = np.abs(looped - other)[in_trial].max()
    results = []
    for table in (wide[:, :D], wide[:, :D].contiguous()):                               # ld > D, and ld = D
        out = torch.full((n, D), -7.0, dtype=torch.float64, device=DEV)
        got = _hip.arhmm_predict(table, offsets, W, w_d, L, out=out).cpu().numpy()
        assert np.all(got[~in_trial] == -7.0)               # rows of no trial are not written
        assert np.array_equal(got[initial], host[initial].astype(np.float64))           # the row's own values
        ar = in_trial & ~initial
        _held('xhat D=%d L=%d K=%d ld=%d' % (D, L, K, table.stride(0)), np.abs(got - looped)[ar], noise,
              np.maximum(scale[ar], 1e-300))
        again = _hip.arhmm_predict(table, offsets, W, w_d, L).cpu().numpy()
        assert np.array_equal(again[in_trial], got[in_trial])
        results.append(got)
    assert np.array_equal(results[0], results[1])           # the stride is not in the arithmetic


@pytest.mark.parametrize('D,L', [(3, 1), (12, 4), (5, 0), (17, 2)])
def test_predict_contains_a_nan_row(D, L):
    rng = np.random.RandomState(D + L)
    K = 5
    offsets = np.asarray([0, 40, 40 + L + 2, 100], dtype=np.int64)
    n = 100
    host = rng.randn(n, D).astype(np.float32)
    W = rng.randn(K, D, 1 + L * D)
    w_d = torch.from_numpy(_weights_of(rng, n, K)).to(DEV)
    clean = _hip.arhmm_predict(torch.from_numpy(host).to(DEV), offsets, W, w_d, L).cpu().numpy()
    bad_rows = [20, 39, 40, 99] + ([0] if L else [])       # mid-trial, a trial's last row, an initial row, the end
    expect = np.zeros(n, dtype=bool)
    for r in bad_rows:
        host[r, rng.randint(D)] = np.nan if r != 39 else np.inf
        s = int(np.searchsorted(offsets, r, side='right')) - 1
        expect[r] = expect[r] or r - int(offsets[s]) < L               # (an initial row is its own prediction)
        for t in range(r + 1, min(r + L + 1, int(offsets[s + 1]))):
            expect[t] = expect[t] or t - int(offsets[s]) >= L          # (an initial row does not look back)
    got = _hip.arhmm_predict(torch.from_numpy(host).to(DEV), offsets, W, w_d, L).cpu().numpy()
    assert np.array_equal(~np.isfinite(got).all(axis=1), expect)
    ar = expect.copy()
    for beg, end in refs.trials_of(offsets):
        ar[beg:min(beg + L, end)] = False
    assert not np.isfinite(got[ar]).any()                   # all D values of a poisoned AR row
    assert np.array_equal(got[~expect], clean[~expect])
    # a NaN among the weights of row t stays in row t
    w_bad = w_d.clone()
    w_bad[60, 2] = float('nan')
    host = np.nan_to_num(host, nan=0.5, posinf=0.5)
    a = _hip.arhmm_predict(torch.from_numpy(host).to(DEV), offsets, W, w_d, L).cpu().numpy()
    b = _hip.arhmm_predict(torch.from_numpy(host).to(DEV), offsets, W, w_bad, L).cpu().numpy()
    assert not np.isfinite(b[60]).any() and np.array_equal(np.delete(a, 60, axis=0), np.delete(b, 60, axis=0))


def test_limits_are_checked_with_a_device_table():
    table = torch.zeros((10, 3), device=DEV)
    w = torch.zeros((10, 2), dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match=r'expected W float64 \(K, D, 1 \+ lags D\)'):
        _hip.arhmm_predict(table, [0, 10], np.zeros((2, 3)), w, 1)
    with pytest.raises(ValueError, match='9 lags'):
        _hip.arhmm_predict(table, [0, 10], np.zeros((2, 3, 28)), w, 9)
    with pytest.raises(ValueError, match='33 states'):
        _hip.arhmm_predict(table, [0, 10], np.zeros((33, 3, 4)), w, 1)
    with pytest.raises(ValueError, match=r'\(lags \+ 1\) \* columns = 66'):
        _hip.arhmm_predict(torch.zeros((10, 33), device=DEV), [0, 10], np.zeros((2, 33, 34)), w, 1)
    with pytest.raises(ValueError, match='no CPU fallback'):
        _hip.arhmm_predict(table, [0, 10], np.zeros((2, 3, 4)), w.cpu(), 1)
    with pytest.raises(ValueError, match=r'expected weights float64 \(10, 2\)'):
        _hip.arhmm_predict(table, [0, 10], np.zeros((2, 3, 4)), w[:9], 1)
    with pytest.raises(ValueError, match=r'expected out float64 \(10, 3\)'):
        _hip.arhmm_predict(table, [0, 10], np.zeros((2, 3, 4)), w, 1, out=torch.zeros((10, 3), device=DEV))


# ------------------------------------------------------------------------------------------------------------
# the model's methods
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('weights', ['predictive', 'smoothed'])
@pytest.mark.parametrize('D,L', [(3, 1), (4, 0), (6, 2)])
def test_table_predictions_and_prediction_sums(D, L, weights):
    rng = np.random.RandomState(31 + D + L)
    K = 3
    m = _model(rng, K, D, L, True)
    offsets = _offsets(L, n_long=(37, 90))
    n = int(offsets[-1]) + 3
    wide = torch.from_numpy(np.cumsum(0.3 * rng.randn(n, D + 2), axis=0).astype(np.float32)).to(DEV)
    table = wide[:, :D]
    host = table.cpu().numpy()
    xhat_d, valid_d = m.table_predictions(table, offsets, weights)
    xhat, valid = xhat_d.cpu().numpy(), valid_d.cpu().numpy()
    assert valid.dtype == np.bool_ and np.array_equal(valid, prefs.valid_rows(n, offsets, L))
    # two restatements of the whole chain, no step shared: the direct density, log-space weights and the looped
    # mixture; the folded density, scaled weights and the einsum
    ll = refs.loglik_direct(host, offsets, m.As, m.bs, m.Sigmas, L)
    ll2 = refs.loglik_folded(host, offsets, *m.fold(), L, m.shift)
    if weights == 'predictive':
        w1 = prefs.weights_table(ll, offsets, m.log_Ps, m.log_pi0, prefs.weights_log)
        w2 = prefs.weights_table(ll2, offsets, m.log_Ps, m.log_pi0, prefs.weights_scaled)
    else:
        w1 = refs.forward_backward(ll, offsets, m.log_Ps, m.log_pi0, refs.fb_log)[0]
        w2 = refs.forward_backward(ll2, offsets, m.log_Ps, m.log_pi0, refs.fb_scaled)[0]
    W = m.generative()[0]
    x1 = prefs.predict_loop(host, offsets, W, w1, L)
    x2 = prefs.predict_einsum(host, offsets, W, w2, L)
    in_trial = np.zeros(n, dtype=bool)
    in_trial[offsets[0]:offsets[-1]] = True
    # (the weights are a function of ll: their error is the density's, carried through the recursion, and the two
    # chains' disagreement holds that too)
    _held('table_predictions D=%d L=%d %s' % (D, L, weights), np.abs(xhat - x1)[in_trial],
          np.abs(x1 - x2)[in_trial].max(), np.maximum(prefs.predict_scale(host, offsets, W, np.abs(w1), L), 1.0)[in_trial])
    assert not xhat[~in_trial].any()
    one = int(offsets[4])
    assert np.array_equal(m.predict(host[one:offsets[5]], weights), xhat[one:offsets[5]])
    if weights == 'smoothed':
        assert np.array_equal(m.smooth(host[one:offsets[5]]), xhat[one:offsets[5]])
    # the reduction alone: numpy sums over the device's own fp32-rounded predictions
    sums = m.prediction_sums(table, offsets, weights)
    want, scale = prefs.prediction_sums(host, xhat.astype(np.float32), offsets, L)
    assert sums.shape == want.shape == (2, len(offsets) - 1, D, 4)
    err, bound = np.abs(sums - want), 1e-12 * scale
    print('prediction_sums D=%d L=%d %s: worst error / bound %.3f'
          % (D, L, weights, float(np.max(err[bound > 0] / bound[bound > 0]))))
    assert np.all(err <= bound)
    assert np.array_equal(sums[0, ..., :3], sums[1, ..., :3])          # count, sum x and sum x^2 do not know the guess
    assert np.array_equal(m.prediction_sums(table, offsets, weights), sums)
    with pytest.raises(ValueError, match="weights 'causal' are not served"):
        m.table_predictions(table, offsets, 'causal')


# ------------------------------------------------------------------------------------------------------------
# fitting.eval.arhmm_predictions on a generator
# ------------------------------------------------------------------------------------------------------------
def test_arhmm_predictions_on_the_synthetic_generator(tmp_path):
    from behavenet_amd.fitting.eval import (arhmm_predictions, export_arhmm_predictions, fit_arhmm,
                                            real_vs_sampled_movie, summarise_prediction_sums)
    from tests.test_gpu_latent_corr import _per_trial_latents
    from tests.test_gpu_ranges import LENS, _generator, _model as _ae
    root = str(tmp_path)
    model, meta = _ae('ae_cfg1', root)
    gen = _generator(meta, n_sessions=2, n_labels=3)
    arhmm, _ = fit_arhmm(gen, model, n_states=2, n_lags=1, n_iters=3, rng_seed_model=1)
    D, L = arhmm.D, arhmm.lags
    dtypes = ['train', 'test']
    out = arhmm_predictions(gen, model, arhmm, dtype=dtypes, return_latents=True)
    keys = [(s, int(t)) for s, ds in enumerate(gen.datasets) for dt in dtypes for t in ds.batch_idxs[dt]]
    assert list(zip(out['session'].tolist(), out['trial'].tolist())) == keys
    assert [x.shape for x in out['latents']] == [(LENS[t], D) for _, t in keys]
    assert [x.shape for x in out['latents_pred']] == [(LENS[t], D) for _, t in keys]
    assert all(x.dtype == np.float64 for x in out['latents_pred'])
    per_trial = np.concatenate([_per_trial_latents(model, gen, dtypes, [s])[0] for s in (0, 1)], axis=0)
    host = np.concatenate(out['latents'], axis=0)
    assert np.abs(host - per_trial).max() <= 1e-5 * np.abs(per_trial).max()            # (another encoder batching)
    # the restatement on the encoded latents
    offsets = np.concatenate(([0], np.cumsum([LENS[t] for _, t in keys]))).astype(np.int64)
    ll = refs.loglik_direct(host, offsets, arhmm.As, arhmm.bs, arhmm.Sigmas, L)
    w = prefs.weights_table(ll, offsets, arhmm.log_Ps, arhmm.log_pi0)
    W = arhmm.generative()[0]
    xhat = prefs.predict_einsum(host, offsets, W, w, L)
    got = np.concatenate(out['latents_pred'], axis=0)
    # ll carries 2^-53 of its terms (1e-12 at |ll| of 1e4), a weight moves by no more than ll does and the
    # recursion forgets old rows: 1e-9 of the prediction's scale is three digits above that
    assert np.all(np.abs(got - xhat) <= 1e-9 * np.maximum(prefs.predict_scale(host, offsets, W, w, L), 1.0))
    want, scale = prefs.prediction_sums(host, xhat.astype(np.float32), offsets, L)
    assert out['sums'].shape == (2, len(keys), D, 4)
    assert np.all(np.abs(out['sums'] - want)[..., :3] <= 1e-12 * scale[..., :3])
    assert np.all(np.abs(out['sums'][1] - want[1]) <= 1e-12 * scale[1])                 # the baseline: the table alone
    # sum (x - p)^2 with p rounded to fp32 from two float64 values that agree to 1e-9: the roundings differ by one
    # fp32 step of |p| at most, 2^-23 |p|, so the sum moves by 2^-22 sum |x - p| |p| <= 2^-22 sqrt(sd sum p^2) (and
    # the square of the step, far below)
    p2 = np.stack([np.sum(xhat[a + max(L, 1):b] ** 2, axis=0) for a, b in refs.trials_of(offsets)])
    sd_bound = 2.0 ** -22 * np.sqrt(want[0, ..., 3] * p2) + 1e-12 * scale[0, ..., 3]
    assert np.all(np.abs(out['sums'][0, ..., 3] - want[0, ..., 3]) <= sd_bound)
    sc = prefs.scores(want)
    scored = want[0, ..., 0] > 10
    assert scored.all() and np.array_equal(out['n'], want[0, ..., 0].astype(np.int64))
    assert np.all(np.abs(out['mse'] - sc['mse'][0]) <= sd_bound / want[0, ..., 0])
    ss_tot = want[0, ..., 2] - want[0, ..., 1] ** 2 / want[0, ..., 0]
    assert np.all(np.abs(out['r2'] - sc['r2'][0]) <= sd_bound / ss_tot + 1e-9)
    assert np.allclose(out['mse_persistence'], sc['mse'][1], rtol=1e-10, atol=0)
    assert np.all(np.abs(out['r2_persistence'] - sc['r2'][1]) <= 1e-9)
    # the pooled values are the recombined per-trial sums
    tot = out['sums'].sum(axis=1)
    assert np.array_equal(out['pooled']['n'], tot[0, :, 0].astype(np.int64))
    for tag, i in (('', 0), ('_persistence', 1)):
        assert np.allclose(out['pooled']['mse' + tag], tot[i, :, 3] / tot[i, :, 0], rtol=1e-14, atol=0)
        ss = tot[i, :, 2] - tot[i, :, 1] ** 2 / tot[i, :, 0]
        assert np.allclose(out['pooled']['r2' + tag], 1.0 - tot[i, :, 3] / ss, rtol=1e-12, atol=1e-12)
        assert np.isclose(out['pooled']['mse%s_all' % tag], tot[i, :, 3].sum() / tot[i, :, 0].sum(), rtol=1e-14)
        assert np.isclose(out['pooled']['r2%s_all' % tag], 1.0 - tot[i, :, 3].sum() / ss.sum(), rtol=1e-12)
    again = summarise_prediction_sums(out['sums'])
    assert all(np.array_equal(again[k], out[k], equal_nan=True) for k in ('n', 'mse', 'r2', 'mse_persistence'))
    print('pooled one-step R2 %.4f against persistence %.4f' % (out['pooled']['r2_all'],
                                                               out['pooled']['r2_persistence_all']))
    # one session, the smoothed weights, no latents
    one = arhmm_predictions(gen, model, arhmm, dtype='test', weights='smoothed', sess_idx=1)
    assert 'latents' not in one and one['session'].tolist() == [1]
    assert one['trial'].tolist() == [int(t) for t in gen.datasets[1].batch_idxs['test']]
    # the csv round-trips
    hp = {'expt_dir': root, 'version': 0, 'model_class': 'arhmm'}
    path = export_arhmm_predictions(hp, gen, arhmm, model=model, dtype=dtypes)
    assert path == os.path.join(root, 'version_0', 'arhmm_predictions.csv')
    with open(path, newline='') as f:
        rows = list(csv.reader(f))
    assert rows[0] == ['Session', 'Trial', 'Dim', 'N', 'MSE', 'R2', 'MSE_persistence', 'R2_persistence']
    assert len(rows) == 1 + len(keys) * D
    for k, (s, t) in enumerate(keys):
        for d in range(D):
            row = rows[1 + k * D + d]
            assert [int(v) for v in row[:4]] == [s, t, d, int(out['n'][k, d])]
            assert [float(v) for v in row[4:]] == [float(out[name][k, d]) for name in
                                                   ('mse', 'r2', 'mse_persistence', 'r2_persistence')]
    # a real-versus-predicted movie from the existing movie code
    movie = real_vs_sampled_movie(model, out['latents'], out['latents_pred'], max_frames=10, n_buffer=1)
    assert movie.dtype == np.uint8 and movie.shape[1:] == (32, 64) and movie.shape[0] >= 10
    with pytest.raises(ValueError, match='dtype must be'):
        arhmm_predictions(gen, model, arhmm, dtype='all')
