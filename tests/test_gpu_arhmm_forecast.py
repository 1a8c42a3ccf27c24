"""Exact multi-step forecasts of an ARHMM on the device (bn_arhmm_forecast_sums in csrc/arhmm.hip,
ARHMM.forecast_sums / table_forecast, fitting.eval.arhmm_forecasts and the fit() hook) against the float64
restatements of tests/arhmm_forecast_refs.py.

The launch writes sums only, so the sums are what is held: the five sums from the looped forecasts against the device
under the rule of tests/test_gpu_arhmm.py (its ``_held``), trial by trial -- the bound is 100 x the disagreement of the
sums from the looped and from the einsum forecasts in that trial and never less than 1e-12 of ``sum |terms|``.  The
bound comes from the restatements alone; every check prints error, bound and their ratio.  One reference a shape, made
at H = 32: the sums of a horizon do not depend on how many horizons are asked for, so the first H horizons of it serve
every H.  The horizon group of the kernel is four column tiles, 64 columns (h, d): four horizons at D = 16, so H = 5 is
one above it there, and H = 32 crosses a group at every D but 1.

``ARHMM.forecast_sums`` is held against numpy sums over ``table_forecast``'s own float64 forecasts (the unfused device
route: bn_arhmm_predict with the map of one horizon, shifted inside the trials) at 1e-12 of ``sum |terms|``, and at
h = 1 against ``prediction_sums`` within what rounding xhat to fp32 allows.

Largest error / bound seen on an MI355X (first run of this file): the launch's sums 0.005 in every trial with more
than one pair at every shape and H, 0.091 in the trial of L + 1 rows (ONE pair: the bound is 1e-12 of a single squared
error, and the error is the forecast's own rounding, 5e-15); ``forecast_sums`` against ``table_forecast`` 0.003.
"""

import csv
import os
import pickle

import numpy as np
import pytest
import torch

from behavenet_amd import _hip
from behavenet_amd.models.arhmm import ARHMM
from tests import arhmm_forecast_refs as frefs
from tests import arhmm_refs as refs
from tests.test_gpu_arhmm import _held, _model, _offsets

pytestmark = pytest.mark.gpu
DEV = 'cuda'
H_MAX = 32
SHAPES = [(1, 0, 1), (3, 1, 2), (16, 1, 16), (17, 1, 5), (32, 1, 32), (12, 4, 3), (7, 8, 4)]


def _trials(L):
    """``_offsets(L)`` -- trials of 0, L, L + 1, 37, 150, 0 and 1 rows after two rows of no trial -- and one trial of
    1,500 rows, several row blocks of the kernel."""
    offsets = _offsets(L)
    return np.concatenate([offsets, [offsets[-1] + 1500]]).astype(np.int64)


def _weights_of(rng, n, K):
    w = rng.rand(n, K)
    return w / w.sum(axis=1, keepdims=True)


_CASES = {}


def _case(D, L, K):
    """The table (three columns wider than D), maps, weights and the reference sums at H = 32 of a shape, made once."""
    if (D, L, K) not in _CASES:
        rng = np.random.RandomState(3000 + 100 * D + 10 * L + K)
        offsets = _trials(L)
        n = int(offsets[-1]) + 3
        wide = (rng.randn(n, D + 3) + 1.5).astype(np.float32)
        Q = 1 + L * D
        N = rng.randn(H_MAX, K, D, Q) / np.sqrt(Q)
        w = _weights_of(rng, n, K)
        host = np.ascontiguousarray(wide[:, :D])
        looped, scale = frefs.forecast_sums(host, frefs.forecast_loop_trials(host, offsets, N, w, L), offsets, L)
        other, _ = frefs.forecast_sums(host, frefs.forecast_einsum(host, offsets, N, w, L), offsets, L)
        _CASES[(D, L, K)] = {'offsets': offsets, 'n': n, 'wide': wide, 'N': N, 'w': w, 'sums': looped, 'scale': scale,
                             'noise': np.abs(looped - other).max(axis=(0, 2, 3))}
    return _CASES[(D, L, K)]


@pytest.mark.parametrize('H', [1, 2, 5, 32])
@pytest.mark.parametrize('D,L,K', SHAPES)
def test_forecast_sums(D, L, K, H):
    c = _case(D, L, K)
    offsets, n = c['offsets'], c['n']
    S = len(offsets) - 1
    wide = torch.from_numpy(c['wide']).to(DEV)
    w_d = torch.from_numpy(c['w']).to(DEV)
    N = np.ascontiguousarray(c['N'][:H])
    want, scale = c['sums'][:H], c['scale'][:H]
    results = []
    for table in (wide[:, :D], wide[:, :D].contiguous()):                               # ld > D, and ld = D
        out = torch.full((H, S, D, 5), -7.0, dtype=torch.float64, device=DEV)
        got_d = _hip.arhmm_forecast_sums(table, offsets, N, w_d, L, out=out)
        assert got_d is out
        got = got_d.cpu().numpy()
        assert np.array_equal(got[..., 0], want[..., 0])    # the counts: the validity rule itself, and every element
        for s in range(S):                                  # is written (a trial without a pair: zeros)
            if not want[0, s, 0, 0]:
                assert not got[:, s].any()
                continue
            _held('forecast sums D=%d L=%d K=%d H=%d ld=%d trial %d' % (D, L, K, H, table.stride(0), s),
                  np.abs(got - want)[:, s], c['noise'][s], np.maximum(scale[:, s], 1e-300))
        again = _hip.arhmm_forecast_sums(table, offsets, N, w_d, L).cpu().numpy()
        assert np.array_equal(again, got)                   # the same bits on a second call
        results.append(got)
    assert np.array_equal(results[0], results[1])           # the stride is not in the arithmetic


def test_a_horizon_s_sums_do_not_depend_on_the_horizons_asked_for():
    c = _case(16, 1, 16)
    table = torch.from_numpy(np.ascontiguousarray(c['wide'][:, :16])).to(DEV)
    w_d = torch.from_numpy(c['w']).to(DEV)
    full = _hip.arhmm_forecast_sums(table, c['offsets'], c['N'], w_d, 1).cpu().numpy()
    for H in (1, 4, 5, 9):
        part = _hip.arhmm_forecast_sums(table, c['offsets'], np.ascontiguousarray(c['N'][:H]), w_d, 1).cpu().numpy()
        assert np.array_equal(part, full[:H])


@pytest.mark.parametrize('D,L', [(3, 1), (16, 1), (12, 4), (5, 0)])
def test_a_bad_row_or_weight_stays_in_its_trial(D, L):
    rng = np.random.RandomState(50 + D + L)
    K, H = 4, 5
    offsets = _trials(L)
    S = len(offsets) - 1
    n = int(offsets[-1]) + 3
    host = (rng.randn(n, D) + 0.5).astype(np.float32)
    N = rng.randn(H, K, D, 1 + L * D) / np.sqrt(1 + L * D)
    w = _weights_of(rng, n, K)
    w_d = torch.from_numpy(w).to(DEV)

    def run(x, weights=w_d):
        return _hip.arhmm_forecast_sums(torch.from_numpy(x).to(DEV), offsets, N, weights, L).cpu().numpy()
    clean = run(host)
    assert np.isfinite(clean).all()
    # rows of no trial are never read
    outside = host.copy()
    outside[:offsets[0]] = np.nan
    outside[offsets[-1]:] = np.nan
    w_out = w.copy()
    w_out[:offsets[0]] = np.nan
    w_out[offsets[-1]:] = np.nan
    assert np.array_equal(run(outside, torch.from_numpy(w_out).to(DEV)), clean)
    # a NaN row in the middle of the 150-row trial (s = 4), an Inf row in the 1,500-row trial (s = 7, in its second row
    # block) and a NaN weight of an origin row of the 37-row trial (s = 3): one at a time
    for s, row, what in ((4, int(offsets[4]) + 70, np.nan), (7, int(offsets[7]) + 400, np.inf)):
        bad = host.copy()
        bad[row] = what
        got = run(bad)
        others = [i for i in range(S) if i != s]
        assert np.array_equal(got[:, others], clean[:, others])
        assert np.array_equal(got[:, s, :, 0], clean[:, s, :, 0])                      # (the count is no sum of values)
        assert not np.isfinite(got[:, s, :, 1:]).any()      # row t is a target at every horizon and in x_{t-1}
    w_bad = w.copy()
    row = int(offsets[3]) + max(L, 1) + 5
    w_bad[row, 1] = np.nan
    got = run(host, torch.from_numpy(w_bad).to(DEV))
    others = [i for i in range(S) if i != 3]
    assert np.array_equal(got[:, others], clean[:, others])
    assert not np.isfinite(got[:, 3, :, 3]).any()           # the forecasts of that origin, every horizon and dimension
    assert np.array_equal(got[:, 3][..., [0, 1, 2, 4]], clean[:, 3][..., [0, 1, 2, 4]])
    # a weight of a row that is no origin is not read
    w_bad = w.copy()
    w_bad[int(offsets[3])] = np.nan
    assert np.array_equal(run(host, torch.from_numpy(w_bad).to(DEV)), clean)


def test_limits_are_checked_with_a_device_table():
    table = torch.zeros((10, 3), device=DEV)
    w = torch.zeros((10, 2), dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match=r'expected N float64 \(H, K, D, 1 \+ lags D\)'):
        _hip.arhmm_forecast_sums(table, [0, 10], np.zeros((2, 3, 4)), w, 1)
    with pytest.raises(ValueError, match='9 lags'):
        _hip.arhmm_forecast_sums(table, [0, 10], np.zeros((2, 2, 3, 28)), w, 9)
    with pytest.raises(ValueError, match='33 states'):
        _hip.arhmm_forecast_sums(table, [0, 10], np.zeros((2, 33, 3, 4)), w, 1)
    with pytest.raises(ValueError, match=r'\(lags \+ 1\) \* columns = 66'):
        _hip.arhmm_forecast_sums(torch.zeros((10, 33), device=DEV), [0, 10], np.zeros((2, 2, 33, 34)), w, 1)
    with pytest.raises(ValueError, match='33 horizons'):
        _hip.arhmm_forecast_sums(table, [0, 10], np.zeros((33, 2, 3, 4)), w, 1)
    with pytest.raises(ValueError, match='no CPU fallback'):
        _hip.arhmm_forecast_sums(table, [0, 10], np.zeros((2, 2, 3, 4)), w.cpu(), 1)
    with pytest.raises(ValueError, match=r'expected weights float64 \(10, 2\)'):
        _hip.arhmm_forecast_sums(table, [0, 10], np.zeros((2, 2, 3, 4)), w[:9], 1)
    with pytest.raises(ValueError, match=r'expected out float64 \(2, 1, 3, 5\)'):
        _hip.arhmm_forecast_sums(table, [0, 10], np.zeros((2, 2, 3, 4)), w, 1,
                                 out=torch.zeros((2, 1, 3, 5), device=DEV))
    assert not _hip.arhmm_forecast_sums(table, [0, 10], np.zeros((2, 2, 3, 4)), w, 1)[..., 1:].any()


# ------------------------------------------------------------------------------------------------------------
# the model's methods
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D,L', [(3, 1), (4, 0), (6, 2)])
def test_forecast_sums_of_a_model_against_its_table_forecasts(D, L):
    rng = np.random.RandomState(61 + D + L)
    K, H = 3, 6
    offsets = _offsets(L, n_long=(37, 300))
    S = len(offsets) - 1
    n = int(offsets[-1]) + 3
    wide = torch.from_numpy(np.cumsum(0.3 * rng.randn(n, D + 2), axis=0).astype(np.float32)).to(DEV)
    table = wide[:, :D]
    host = table.cpu().numpy().astype(np.float64)
    m = ARHMM(K, D, lags=L)
    m.initialize(table.contiguous(), offsets, seed=0)
    m.em_step(table.contiguous(), offsets)
    m.em_step(table.contiguous(), offsets)
    sums = m.forecast_sums(table, offsets, H)
    assert sums.shape == (2, H, S, D, 4) and sums.dtype == np.float64
    assert np.array_equal(sums[0, ..., :3], sums[1, ..., :3])
    assert np.array_equal(m.forecast_sums(table, offsets, H), sums)
    first = max(L, 1)
    worst = 0.0
    for h in range(1, H + 1):
        xh_d, valid_d = m.table_forecast(table, offsets, h)
        xh, valid = xh_d.cpu().numpy(), valid_d.cpu().numpy()
        assert xh.dtype == np.float64 and valid.dtype == np.bool_
        expect = np.zeros(n, dtype=bool)
        for s, (beg, end) in enumerate(refs.trials_of(offsets)):
            expect[min(beg + first + h - 1, end):end] = True
        assert np.array_equal(valid, expect)
        inside = np.zeros(n, dtype=bool)
        inside[offsets[0]:offsets[-1]] = True
        assert np.array_equal(xh[inside & ~valid], host[inside & ~valid]) and not xh[~inside].any()
        for s, (beg, end) in enumerate(refs.trials_of(offsets)):
            t = np.arange(min(beg + first + h - 1, end), end)          # the TARGET rows; their origin is t - h + 1
            y = host[t]
            for which, guess in ((0, xh[t]), (1, host[t - h])):
                terms = np.stack([np.ones_like(y), y, y * y, (y - guess) ** 2], axis=2)
                want, scale = terms.sum(axis=0), np.abs(terms).sum(axis=0)
                err = np.abs(sums[which, h - 1, s] - want)
                assert np.all(err <= 1e-12 * scale), (h, s, which)
                if t.size:
                    worst = max(worst, float(np.max(err / (1e-12 * scale))))
    print('forecast_sums against table_forecast D=%d L=%d: worst error / bound %.3f' % (D, L, worst))
    one = int(offsets[4])
    assert np.array_equal(m.forecast(host[one:offsets[5]].astype(np.float32), 3),
                          m.table_forecast(table, offsets, 3)[0].cpu().numpy()[one:offsets[5]])
    # h = 1 against prediction_sums, which rounds xhat to fp32 before it takes the difference: with p = fl32(xhat),
    # |p - xhat| <= 2^-24 |xhat| and (x - p)^2 - (x - xhat)^2 = (xhat - p) (2 (x - xhat) + (xhat - p)), so a trial's sum
    # moves by sum 2^-24 |xhat| (2 |x - xhat| + 2^-24 |xhat|) at most; the other sums know no xhat and both sides add
    # the same float64 terms in another order, 1e-12 of sum |terms|
    ps = m.prediction_sums(table, offsets)
    xh = m.table_forecast(table, offsets, 1)[0].cpu().numpy()
    for s, (beg, end) in enumerate(refs.trials_of(offsets)):
        t = np.arange(min(beg + first, end), end)
        y, p = host[t], xh[t]
        scale = np.stack([np.ones_like(y), np.abs(y), y * y, (y - p) ** 2], axis=2).sum(axis=0)
        base = np.stack([np.ones_like(y), np.abs(y), y * y, (y - host[t - 1]) ** 2], axis=2).sum(axis=0)
        rounding = (2.0 ** -24 * np.abs(p) * (2.0 * np.abs(y - p) + 2.0 ** -24 * np.abs(p))).sum(axis=0)
        assert np.all(np.abs(sums[0, 0, s] - ps[0, s])[:, :3] <= 1e-12 * scale[:, :3])
        assert np.all(np.abs(sums[0, 0, s] - ps[0, s])[:, 3] <= rounding + 1e-12 * scale[:, 3])
        assert np.all(np.abs(sums[1, 0, s] - ps[1, s]) <= 1e-12 * base)
    with pytest.raises(ValueError, match="weights 'smoothed' are not served"):
        m.forecast_sums(table, offsets, H, weights='smoothed')
    with pytest.raises(ValueError, match='horizons'):
        m.table_forecast(table, offsets, 0)


# ------------------------------------------------------------------------------------------------------------
# fitting.eval.arhmm_forecasts on a generator, and the fit() hook
# ------------------------------------------------------------------------------------------------------------
def test_arhmm_forecasts_on_the_synthetic_generator(tmp_path):
    from behavenet_amd.fitting.eval import (arhmm_forecasts, arhmm_predictions, export_arhmm_forecasts, fit_arhmm,
                                            real_vs_sampled_movie, summarise_forecast_sums)
    from tests.test_gpu_ranges import LENS, _generator, _model as _ae
    root = str(tmp_path)
    model, meta = _ae('ae_cfg1', root)
    gen = _generator(meta, n_sessions=2, n_labels=3)
    arhmm, _ = fit_arhmm(gen, model, n_states=2, n_lags=1, n_iters=3, rng_seed_model=1)
    D, H = arhmm.D, 4
    dtypes = ['train', 'test']
    out = arhmm_forecasts(gen, model, arhmm, horizons=H, dtype=dtypes)
    keys = [(s, int(t)) for s, ds in enumerate(gen.datasets) for dt in dtypes for t in ds.batch_idxs[dt]]
    assert list(zip(out['session'].tolist(), out['trial'].tolist())) == keys
    assert out['sums'].shape == (2, H, len(keys), D, 4)
    for name in ('n', 'mse', 'r2', 'mse_persistence', 'r2_persistence'):
        assert out[name].shape == (H, len(keys), D)
    for h in range(H):                                      # origins t >= 1 with t + h still in the trial
        assert out['n'][h, :, 0].tolist() == [LENS[t] - 1 - h for _, t in keys]
    # horizon 1 is arhmm_predictions' own table but for the fp32 rounding of its xhat: with p = fl32(xhat) a trial's
    # sum of squared errors moves by sum 2^-24 |xhat| (2 |x - xhat| + 2^-24 |xhat|) at most (derived in
    # test_forecast_sums_of_a_model_against_its_table_forecasts), and both sides add float64 terms in their own order
    one = arhmm_predictions(gen, model, arhmm, dtype=dtypes, return_latents=True)
    assert np.allclose(out['sums'][:, 0, ..., :3], one['sums'][..., :3], rtol=1e-12, atol=0)
    assert np.allclose(out['mse_persistence'][0], one['mse_persistence'], rtol=1e-10, atol=0)
    for k, (x, p) in enumerate(zip(one['latents'], one['latents_pred'])):
        x, p = x[1:].astype(np.float64), p[1:]
        rounding = (2.0 ** -24 * np.abs(p) * (2.0 * np.abs(x - p) + 2.0 ** -24 * np.abs(p))).sum(axis=0)
        sd = ((x - p) ** 2).sum(axis=0)
        assert np.all(np.abs(out['sums'][0, 0, k, :, 3] - one['sums'][0, k, :, 3]) <= rounding + 2e-12 * sd)
        assert np.all(np.abs(out['mse'][0, k] - one['mse'][k]) <= (rounding + 2e-12 * sd) / (len(x) * (1 - 1e-12)))
    assert out['pooled']['mse_all'].shape == (H,) and out['pooled']['r2'].shape == (H, D)
    gain = out['horizon_of_no_gain']
    assert gain is None or 1 <= gain <= H
    again = summarise_forecast_sums(out['sums'])
    assert again['horizon_of_no_gain'] == gain and np.array_equal(again['mse'], out['mse'], equal_nan=True)
    print('pooled R2 per horizon %s against persistence %s; horizon of no gain: %s'
          % (np.round(out['pooled']['r2_all'], 4).tolist(), np.round(out['pooled']['r2_persistence_all'], 4).tolist(),
             gain))
    single = arhmm_forecasts(gen, model, arhmm, horizons=2, dtype='test', sess_idx=1)
    assert single['session'].tolist() == [1] and single['n'].shape[0] == 2
    hp = {'expt_dir': root, 'version': 0, 'model_class': 'arhmm'}
    path = export_arhmm_forecasts(hp, gen, arhmm, model=model, horizons=H, dtype=dtypes)
    assert path == os.path.join(root, 'version_0', 'arhmm_forecasts.csv')
    with open(path, newline='') as f:
        rows = list(csv.reader(f))
    assert rows[0] == ['Horizon', 'Session', 'Trial', 'Dim', 'N', 'MSE', 'R2', 'MSE_persistence', 'R2_persistence']
    assert len(rows) == 1 + H * len(keys) * D
    for h in range(H):
        for k, (s, t) in enumerate(keys):
            for d in range(D):
                row = rows[1 + (h * len(keys) + k) * D + d]
                assert [int(v) for v in row[:5]] == [h + 1, s, t, d, int(out['n'][h, k, d])]
                want = [float(out[name][h, k, d]) for name in ('mse', 'r2', 'mse_persistence', 'r2_persistence')]
                assert row[5:] == ['' if np.isnan(v) else repr(v) for v in want]        # (a short trial: no score)
    # the forecast of one horizon beside the real latents, in the existing movie code
    pred = [arhmm.forecast(x, 3) for x in one['latents'][:2]]
    assert pred[0].shape == one['latents'][0].shape and pred[0].dtype == np.float64
    movie = real_vs_sampled_movie(model, one['latents'][:2], pred, max_frames=10, n_buffer=1)
    assert movie.dtype == np.uint8 and movie.shape[1:] == (32, 64)
    with pytest.raises(ValueError, match='horizons'):
        arhmm_forecasts(gen, model, arhmm, horizons=33)


def test_fit_writes_the_forecast_scores_and_refuses_before_the_first_epoch(tmp_path):
    from behavenet_amd.data.data_generator import SyntheticSession, SyntheticSessionsGenerator
    from behavenet_amd.fitting.eval import ARHMM_MODEL_FILE
    from behavenet_amd.fitting.training import fit
    from tests.cases import case_hparams, load_case, seeded_build
    from tests.test_gpu_model import BUILDERS
    _, meta = load_case('psvae_cfg4')
    meta = dict(meta, extra_hp=dict(meta['extra_hp']))
    meta['extra_hp'].update({'expt_dir': str(tmp_path), 'max_n_epochs': 1, 'min_n_epochs': 0, 'val_check_interval': 1,
                             'enable_early_stop': False, 'early_stop_history': 10, 'rng_seed_train': 0,
                             'export_latents': False, 'progress_bar': False, 'device': 'cuda',
                             'export_arhmm': {'n_states': 2, 'n_lags': 1, 'n_iters': 2},
                             'export_arhmm_forecasts': {'horizons': 3, 'dtype': 'train'}})
    hp = case_hparams(meta)
    os.makedirs(os.path.join(str(tmp_path), 'version_0'))
    sess = SyntheticSession(6, 40, meta['dim'], seed=0, n_labels=meta['n_labels'], trial_splits='4;1;1;0')
    gen = SyntheticSessionsGenerator([sess], device=DEV, placement='device_u8')
    model = seeded_build(BUILDERS['ps-vae'], hp).to(DEV)
    model.version = 0
    logged = []

    class Exp(object):
        version = 0

        def log(self, row):
            logged.append(row)

        def save(self):
            pass
    fit(hp, model, gen, Exp(), method='ae')
    assert logged
    with open(os.path.join(str(tmp_path), 'version_0', 'arhmm_forecasts.csv'), newline='') as f:
        rows = list(csv.reader(f))
    with open(os.path.join(str(tmp_path), 'version_0', ARHMM_MODEL_FILE), 'rb') as f:
        D = pickle.load(f).D
    trials = [int(t) for t in gen.datasets[0].batch_idxs['train']]
    assert rows[0][0] == 'Horizon' and len(rows) == 1 + 3 * len(trials) * D
    assert [int(r[0]) for r in rows[1::len(trials) * D]] == [1, 2, 3]
    assert [int(r[4]) for r in rows[1::len(trials) * D]] == [39, 38, 37]
    del logged[:]
    with pytest.raises(ValueError, match="export_arhmm_forecasts"):
        fit(dict(hp, export_arhmm_forecasts={'horizons': 33}), model, gen, Exp(), method='ae')
    with pytest.raises(ValueError, match="expected a dict with horizons"):
        fit(dict(hp, export_arhmm_forecasts={'horizons': 3, 'weights': 'smoothed'}), model, gen, Exp(), method='ae')
    no_model = dict(hp)
    del no_model['export_arhmm']
    with pytest.raises(ValueError, match="that key is not set"):
        fit(no_model, model, gen, Exp(), method='ae')
    assert not logged                                       # refused before the first epoch
