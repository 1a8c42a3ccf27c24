"""The decoding half of a grid of ARHMMs: bn_hmm_grid_viterbi, _hip.state_runs_grid, ARHMMGroup.table_states /
table_runs, the relabelling of fit_arhmm_grid from one decoding, and the grid exporters.

What must be equal is compared integer for integer: a model's path against bn_hmm_viterbi on that model's own columns
of the SAME ll, in another slot, next to other models, on a second call.  Against float64 the rule is the one of
tests/test_gpu_arhmm.py (copied, not imported): the restatement's score of the device's path is held to the restated
maximum within max(100 x the disagreement of two float64 restatements of that maximum, 1e-12 x sum_t max |ll_t|).  The
bound comes from the restatements alone; every check prints error, bound and their ratio.

Largest error / bound seen on an MI355X (first run of this file): path score 0.006 / 0.003 / 0.005 / 0.001 / 0.005 for
the classes 4 / 8 / 16 / 32 / all mixed -- the device's path scores what the restatement's own path scores (error =
noise floor) -- and 0.000 against every path of the tiny trials.
"""

import os
import pickle

import numpy as np
import pytest
import torch

from behavenet_amd import _hip
from behavenet_amd.models.arhmm import ARHMM, ARHMMGroup
from tests import hmm_grid_viterbi_refs as refs
from tests import state_runs_refs as srefs

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENTINEL = -5


def _held(name, err, noise, scale):
    """err <= max(100 noise, 1e-12 scale) element by element; prints the worst ratio."""
    err, scale = np.asarray(err, dtype=np.float64), np.asarray(scale, dtype=np.float64)
    bound = np.maximum(100.0 * float(noise), 1e-12 * scale) * np.ones_like(err)
    assert np.all(np.isfinite(err)), name
    ratio = float(np.max(err / bound)) if err.size else 0.0
    print('%s: max error %.3e, noise floor %.3e, smallest bound %.3e, worst error / bound %.3f'
          % (name, float(err.max()) if err.size else 0.0, float(noise), float(bound.min()) if err.size else 0.0, ratio))
    assert ratio <= 1.0, (name, ratio)
    return ratio


def _in_trial(n, offsets):
    mask = np.zeros(n, dtype=bool)
    mask[offsets[0]:offsets[-1]] = True
    return mask


def _decode(ll, offsets, Ks, hmms, out=None):
    log_Ps, log_pi0 = refs.packed(hmms)
    ll_d = ll if torch.is_tensor(ll) else torch.from_numpy(ll).to(DEV)
    return _hip.hmm_grid_viterbi(ll_d, offsets, Ks, log_Ps, log_pi0, out=out)


CASES = {'class 4': refs.class_ks(4), 'class 8': refs.class_ks(8), 'class 16': refs.class_ks(16),
         'class 32': refs.class_ks(32), 'all classes': refs.mixed_ks()}


@pytest.fixture(scope='module', params=list(CASES))
def decoded(request):
    """One grid per class (two full waves and a partly filled one) and one with all classes mixed: the operands and
    the device's paths (never written by the tests)."""
    Ks = CASES[request.param]
    ll, offsets, hmms = refs.hmm_grid(len(Ks), Ks)
    ll_d = torch.from_numpy(ll).to(DEV)
    out = torch.full((len(Ks), ll.shape[0]), SENTINEL, dtype=torch.int32, device=DEV)
    got = _decode(ll_d, offsets, Ks, hmms, out=out)
    assert got is out
    return request.param, Ks, ll, ll_d, offsets, hmms, got.cpu().numpy()


def test_the_plan_fills_two_waves_and_part_of_a_third():
    for KP in refs.CLASSES:
        cls, wave, slot = _hip.hmm_grid_plan(refs.class_ks(KP))
        assert set(cls.tolist()) == {KP} and wave.max() == 2
        assert np.sum(wave == 2) < 64 // KP and np.sum(wave == 0) == np.sum(wave == 1) == 64 // KP
        assert set(refs.class_ks(KP)) == set(refs.CLASS_ENDS[KP])
    assert set(_hip.hmm_grid_plan(refs.mixed_ks())[0].tolist()) == set(refs.CLASSES)


def test_every_model_has_the_single_model_kernel_s_integers(decoded):
    tag, Ks, ll, ll_d, offsets, hmms, got = decoded
    n = ll.shape[0]
    inside = _in_trial(n, offsets)
    assert got.dtype == np.int32 and got.shape == (len(Ks), n)
    assert np.all(got[:, ~inside] == SENTINEL)              # rows of no trial are not written
    for m, (k0, k1) in enumerate(refs.columns(Ks)):
        single = _hip.hmm_viterbi(ll_d[:, k0:k1].contiguous(), offsets, hmms[m][0], hmms[m][1]).cpu().numpy()
        assert np.array_equal(got[m][inside], single[inside]), (tag, m, Ks[m])
        assert got[m][inside].min() >= 0 and got[m][inside].max() < Ks[m]
    # a second call, into a fresh output: the same integers, zeros outside the trials
    again = _decode(ll_d, offsets, Ks, hmms).cpu().numpy()
    assert np.array_equal(again[:, inside], got[:, inside]) and not again[:, ~inside].any()


def test_every_path_scores_the_restated_maximum(decoded):
    """Tie-proof: the restatement's score of the device's path against the restated maximum."""
    tag, Ks, ll, ll_d, offsets, hmms, got = decoded
    errs, noises, scales = [], [], []
    for m, (k0, k1) in enumerate(refs.columns(Ks)):
        llm = ll[:, k0:k1]
        for a, b in refs.trials_of(offsets):
            path, best = refs.viterbi(llm[a:b], *hmms[m])
            errs.append(abs(refs.path_score(llm[a:b], hmms[m][0], hmms[m][1], got[m, a:b]) - best))
            noises.append(max(abs(refs.path_score(llm[a:b], hmms[m][0], hmms[m][1], path) - best),
                              abs(refs.viterbi_backward(llm[a:b], *hmms[m]) - best)))
            scales.append(max(np.abs(llm[a:b]).max(axis=1).sum() if b > a else 1.0, 1.0))
    _held('grid viterbi score, %s' % tag, errs, max(noises), scales)


def test_tiny_trials_against_every_path():
    Ks = [1, 2, 3, 3, 2, 1, 3]
    ll, offsets, hmms = refs.hmm_grid(5, Ks, lengths=[0, 1, 2, 6, 5, 3, 4])
    got = _decode(ll, offsets, Ks, hmms).cpu().numpy()
    errs, noises = [], []
    for m, (k0, k1) in enumerate(refs.columns(Ks)):
        for a, b in refs.trials_of(offsets):
            if b == a:
                continue
            path, score = refs.brute_force(ll[a:b, k0:k1], *hmms[m])
            assert np.array_equal(got[m, a:b], path), (m, a, b)
            errs.append(abs(refs.path_score(ll[a:b, k0:k1], hmms[m][0], hmms[m][1], got[m, a:b]) - score))
            noises.append(abs(refs.viterbi(ll[a:b, k0:k1], *hmms[m])[1] - score))
    _held('grid viterbi against every path', errs, max(noises), 6 * 1e4)


def test_exact_ties_go_to_the_lowest_state_in_every_slot():
    for Ks in (refs.mixed_ks(), refs.class_ks(4), refs.class_ks(16)):
        offsets = np.cumsum([refs.FRONT] + refs.LENGTHS).astype(np.int64)
        n = int(offsets[-1]) + refs.BACK
        hmms = [(np.full((K, K), -np.log(K)), np.full((K,), -np.log(K))) for K in Ks]
        out = torch.full((len(Ks), n), SENTINEL, dtype=torch.int32, device=DEV)
        got = _decode(np.zeros((n, sum(Ks))), offsets, Ks, hmms, out=out).cpu().numpy()
        inside = _in_trial(n, offsets)
        assert not got[:, inside].any() and np.all(got[:, ~inside] == SENTINEL)
    # two states tie above the others (the same column twice): the lower one, in every slot of two waves
    K = 4
    Ks = [K] * 20
    ll, offsets, hmms = refs.hmm_grid(3, Ks)
    hmms = [(np.full((K, K), -np.log(K)), np.full((K,), -np.log(K)))] * len(Ks)
    ll = ll - 100.0
    for k0, _ in refs.columns(Ks):
        ll[:, k0 + 2] = -1e4 + 60.0 + np.random.RandomState(k0).rand(len(ll))
        ll[:, k0 + 3] = ll[:, k0 + 2]
    got = _decode(ll, offsets, Ks, hmms).cpu().numpy()
    assert np.all(got[:, _in_trial(len(ll), offsets)] == 2)


@pytest.mark.parametrize('KP', refs.CLASSES)
def test_a_model_s_path_does_not_depend_on_its_slot(KP):
    """One model in every slot position of its class, among different neighbours and repeated."""
    slots = 64 // KP
    lo, hi = refs.CLASS_ENDS[KP]
    Kx = hi - 1 if hi - 1 >= lo else hi
    llx, offsets, (x,) = refs.hmm_grid(100 + KP, [Kx])
    alone = _hip.hmm_viterbi(torch.from_numpy(llx).to(DEV), offsets, x[0], x[1]).cpu().numpy()
    inside = _in_trial(len(llx), offsets)
    rng = np.random.RandomState(KP)
    seen = set()
    for shift in (0, 1, None):                              # X on the even slots, on the odd slots, on all of them
        Ks, cols, hmms, where = [], [], [], []
        for p in range(2 * slots + 1):
            if shift is None or p % 2 == shift:
                Ks.append(Kx)
                cols.append(llx)
                hmms.append(x)
                where.append(p)
            else:
                K = int(rng.randint(lo, hi + 1))
                Ks.append(K)
                cols.append(-1e4 + 50.0 * rng.rand(len(llx), K))
                hmms.append(refs.random_hmm(rng, K))
        got = _decode(np.ascontiguousarray(np.concatenate(cols, axis=1)), offsets, Ks, hmms).cpu().numpy()
        _, wave, slot = _hip.hmm_grid_plan(Ks)
        for p in where:
            assert np.array_equal(got[p][inside], alone[inside]), (KP, shift, p)
            seen.add(int(slot[p]))
    assert seen == set(range(slots))                        # every slot position held the model
    assert len(np.unique(alone[inside])) > 1


def test_a_nan_stays_in_its_model():
    """A value test: nothing faults, the NaN is an operand."""
    Ks = refs.mixed_ks()
    ll, offsets, hmms = refs.hmm_grid(77, Ks)
    clean = _decode(ll, offsets, Ks, hmms).cpu().numpy()
    cols = refs.columns(Ks)
    inside = _in_trial(len(ll), offsets)
    for bad in (1, 4, 7, 15):                               # K = 4 (shares its wave with K = 1), 9, 32 and 32 again
        dirty = ll.copy()
        k0, k1 = cols[bad]
        dirty[offsets[7] + 100, k0 + Ks[bad] // 2] = np.nan           # in the trial of 257 rows
        dirty[offsets[4] + 1, k0] = np.nan                            # ... and in the one of 64
        got = _decode(dirty, offsets, Ks, hmms).cpu().numpy()
        for m in range(len(Ks)):
            if m != bad:
                assert np.array_equal(got[m], clean[m]), (bad, m)
        assert got[bad][inside].min() >= 0 and got[bad][inside].max() < Ks[bad]
        assert not got[bad][~inside].any()


# ------------------------------------------------------------------------------------------------------------
# ARHMMGroup.table_states / table_runs, _hip.state_runs_grid
# ------------------------------------------------------------------------------------------------------------
def _model(rng, K, D, L, shift):
    m = ARHMM(K, D, lags=L)
    m.As = 0.3 / max(L, 1) * rng.randn(K, D, L * D)
    m.bs = rng.randn(K, D)
    for k in range(K):
        B = rng.randn(D, D)
        m.Sigmas[k] = B @ B.T / D + 0.2 * np.eye(D)
    m.log_Ps, m.log_pi0 = refs.random_hmm(rng, K)
    m.shift = shift.copy()
    return m


def _group(seed, Ks, D, L):
    """Trials of length 0, L, L + 1, longer ones and 1, two rows in front and three behind that belong to none."""
    rng = np.random.RandomState(seed)
    offsets = np.cumsum([2, 0, L, L + 1, 37, 150, 0, 1]).astype(np.int64)
    host = (rng.randn(int(offsets[-1]) + 3, D) + 1.5).astype(np.float32)
    shift = rng.randn(D) + 1.0
    return [_model(rng, K, D, L, shift) for K in Ks], torch.from_numpy(host).to(DEV), offsets


@pytest.mark.parametrize('D,L', [(3, 1), (16, 1), (7, 8)])
def test_the_group_s_states_are_every_model_s_own(D, L):
    """ll from the grid log-likelihood kernel: if this fails the two log-likelihood routes differ in bits."""
    Ks = [1, 4, 5, 8, 9, 16, 17, 32]
    models, table, offsets = _group(10 * D + L, Ks, D, L)
    group = ARHMMGroup(models)
    dev = group.table_states_device(table, offsets)
    assert dev.is_cuda and dev.dtype == torch.int32 and tuple(dev.shape) == (len(Ks), len(table))
    states = group.table_states(table, offsets)
    assert len(states) == len(Ks)
    for m, model in enumerate(models):
        own = model.table_states(table, offsets)
        assert states[m].dtype == np.int32 and np.array_equal(states[m], own), (D, L, m)
        assert np.array_equal(dev[m].cpu().numpy(), own)
    assert sum(len(np.unique(s)) > 1 for s in states) >= 4


def _sticky(rng, n, K, mean=5):
    out = np.zeros(n, dtype=np.int32)
    i = 0
    while i < n:
        step = 1 + int(rng.geometric(1.0 / mean))
        out[i:i + step] = rng.randint(0, K)
        i += step
    return out


def _check_triple(got, states, offsets, K):
    runs, frames, trans = got
    assert runs.dtype == np.int32 and frames.dtype == np.int64 and trans.dtype == np.int64
    assert np.array_equal(runs, srefs.runs_of(states, offsets))
    assert np.array_equal(frames, srefs.frames_of(states, offsets, K))
    assert np.array_equal(frames, np.bincount(states[offsets[0]:offsets[-1]], minlength=K))
    assert np.array_equal(trans, srefs.trans_of(states, offsets, K))


def test_state_runs_grid_against_the_restatements(monkeypatch):
    rng = np.random.RandomState(8)
    Ks = [1, 3, 32, 7, 2]
    offsets = np.cumsum([2] + refs.LENGTHS + [1100]).astype(np.int64)         # the last trial crosses a tile
    n = int(offsets[-1]) + 2
    states = np.stack([_sticky(rng, n, K) for K in Ks])
    states[:, :2] = 99                                      # rows of no trial are not read
    states[:, -2:] = -4
    states_d = torch.from_numpy(states).to(DEV)
    got = _hip.state_runs_grid(states_d, offsets, Ks)
    assert len(got) == len(Ks)
    for m, K in enumerate(Ks):
        _check_triple(got[m], states[m], offsets, K)
        one = _hip.state_runs(states_d[m], offsets, K)
        for a, b in zip(got[m], one):
            assert np.array_equal(a, b.cpu().numpy())
    # run buffers for two models at a time, and for one: the same results chunk by chunk
    for models_a_chunk in (2, 1):
        monkeypatch.setattr(_hip, 'STATE_RUNS_GRID_BYTES', 16 * n * models_a_chunk)
        again = _hip.state_runs_grid(states_d, offsets, Ks)
        for a, b in zip(got, again):
            assert all(np.array_equal(u, v) for u, v in zip(a, b))
    # a model with states outside its own is named
    bad = states.copy()
    bad[3, offsets[4]] = 7
    bad[3, offsets[8] + 5] = -1
    with pytest.raises(ValueError, match=r'state_runs_grid: model 3: 2 rows in trials hold a state outside \[0, 7\)'):
        _hip.state_runs_grid(torch.from_numpy(bad).to(DEV), offsets, Ks)
    # no trials, no rows
    empty = _hip.state_runs_grid(states_d, [0], Ks)
    assert all(r.shape == (0, 4) and not f.any() and t.shape == (K, K) for (r, f, t), K in zip(empty, Ks))


def test_table_runs_of_a_group():
    Ks = [2, 5, 9, 17, 4]
    models, table, offsets = _group(5, Ks, 4, 2)
    group = ARHMMGroup(models)
    got = group.table_runs(table, offsets)
    states = group.table_states(table, offsets)
    for m, model in enumerate(models):
        _check_triple(got[m], states[m], offsets, Ks[m])
        own = model.table_runs(table, offsets)
        assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(got[m], own))


# ------------------------------------------------------------------------------------------------------------
# fit_arhmm_grid_tables: the relabelling from one decoding of the group
# ------------------------------------------------------------------------------------------------------------
PARAMS = ('As', 'bs', 'Sigmas', 'log_Ps', 'log_pi0')


def _fit_data(seed=41, D=3, n_train=6, T=(50, 71)):
    """The data shape of the grid's end-to-end test (tests/test_gpu_arhmm_grid.py)."""
    from tests import arhmm_refs
    rng = np.random.RandomState(seed)
    lens = list(rng.randint(T[0], T[1], size=n_train + 4))
    datas, _ = arhmm_refs.sample_arhmm(rng, 3, D, 1, lens, sep=1.5)
    return datas[:n_train], datas[n_train:n_train + 2], datas[n_train + 2:]


def test_the_group_relabelling_is_the_per_model_relabelling(monkeypatch):
    from behavenet_amd.fitting import eval as ev
    train, val, test = _fit_data()
    grid = ev.arhmm_grid([2, 3, 4], n_lags=(1, 2), rng_seed_model=1)
    fits = ev.fit_arhmm_grid_tables(train, val, test, grid=grid, n_iters=5)
    calls = []

    def one_by_one(models, table, offsets):
        for m in models:
            ev._arhmm_relabel(m, table, offsets)
        calls.append(len(models))
    monkeypatch.setattr(ev, '_arhmm_grid_relabel', one_by_one)
    want = ev.fit_arhmm_grid_tables(train, val, test, grid=grid, n_iters=5)
    assert calls == [3, 3]                                  # two groups (one n_lags each) went through _arhmm_relabel
    table, t_off = ARHMM.as_table(train)
    permuted = 0
    for (a, rows_a), (b, rows_b) in zip(fits, want):
        for name in PARAMS:
            assert np.array_equal(getattr(a, name), getattr(b, name)), name
        assert rows_a == rows_b
        usage = np.bincount(a.table_states(table, t_off), minlength=a.K)
        assert np.all(np.diff(usage) <= 0), usage
        permuted += 1
    assert permuted == 6


# ------------------------------------------------------------------------------------------------------------
# the exporters and the fit() hook
# ------------------------------------------------------------------------------------------------------------
GRID = [{'n_states': 2, 'n_lags': 1, 'rng_seed_model': 1}, {'n_states': 3, 'n_lags': 2},
        {'n_states': 4, 'n_lags': 1, 'transitions': 'sticky', 'kappa': 10}]
RUN_FIELDS = ('usage', 'n_states_used', 'n_states_99', 'n_runs', 'median_duration', 'mean_duration')


def _same_selection(a, b):
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        assert set(ra) == set(rb)
        for key in ra:
            if key == 'usage':
                assert np.array_equal(ra[key], rb[key])
            elif isinstance(ra[key], float) and np.isnan(ra[key]):
                assert np.isnan(rb[key]), key
            else:
                assert ra[key] == rb[key], key


def _check_grid_files(vdir, gen, model, n_models, encode, exact=True):
    gdir = os.path.join(vdir, 'arhmm_grid')
    assert sorted(os.listdir(gdir)) == ['model_%03d' % i for i in range(n_models)] + ['selection.pkl']
    with open(os.path.join(gdir, 'selection.pkl'), 'rb') as f:
        sel = pickle.load(f)
    assert set(sel) == {'grid', 'rows', 'selection'} and len(sel['rows']) == len(sel['selection']) == n_models
    arhmms = []
    for i in range(n_models):
        mdir = os.path.join(gdir, 'model_%03d' % i)
        with open(os.path.join(mdir, 'arhmm_best_val_model.pt'), 'rb') as f:
            arhmm = pickle.load(f)
        assert isinstance(arhmm, ARHMM) and (arhmm.K, arhmm.lags) == (sel['grid'][i]['n_states'], sel['grid'][i]['n_lags'])
        arhmms.append(arhmm)
        files = sorted(f for f in os.listdir(mdir) if f.endswith('_states.pkl'))
        assert len(files) == len(gen.datasets)
        for s, name in enumerate(files):
            ds = gen.datasets[s]
            assert name == '%s_%s_%s_%s_states.pkl' % (ds.lab, ds.expt, ds.animal, ds.session)
            with open(os.path.join(mdir, name), 'rb') as f:
                d = pickle.load(f)
            assert set(d) == {'states', 'trials'} and len(d['states']) == ds.n_trials
            in_split = set(int(t) for dt in ('train', 'val', 'test') for t in ds.batch_idxs[dt])
            for t in range(ds.n_trials):
                if t in in_split:
                    z = encode(ds, t, s)
                    assert d['states'][t].dtype == np.int32 and d['states'][t].shape == (len(z),)
                    assert d['states'][t].min() >= 0 and d['states'][t].max() < arhmm.K
                    if exact:
                        assert np.array_equal(d['states'][t], arhmm.most_likely_states(z)), (i, s, t)
                else:
                    assert d['states'][t].size == 0          # gap trials
    return sel, arhmms


def _encode_one(model, ds, t, s):
    from behavenet_amd.fitting.eval import encode_trial
    return np.asarray(encode_trial(model, torch.from_numpy(ds.images_u8[int(t)]).to(DEV), s), dtype=np.float32)


def test_export_arhmm_grid_on_the_synthetic_generator(tmp_path):
    from behavenet_amd.fitting.eval import arhmm_grid_selection, arhmm_grid_states, export_arhmm_grid
    from tests.test_gpu_ranges import LENS, _generator, _model as _ae
    root = str(tmp_path)
    model, meta = _ae('ae_cfg1', root)
    gen = _generator(meta, n_sessions=2)
    fits, selection, path, files = export_arhmm_grid(gen, model, GRID, n_iters=2)
    vdir = os.path.join(root, 'version_0')
    assert path == os.path.join(vdir, 'arhmm_grid', 'selection.pkl')
    assert [len(f) for f in files] == [2, 2, 2] and all(os.path.exists(p) for f in files for p in f)
    assert not [f for f in os.listdir(vdir) if f.endswith('_states.pkl') or f.endswith('.pt')]    # nothing beside it
    sel, arhmms = _check_grid_files(vdir, gen, model, 3, lambda ds, t, s: _encode_one(model, ds, t, s))
    assert sel['grid'] == GRID
    for (a, rows), b, rows_b in zip(fits, arhmms, sel['rows']):
        assert rows == rows_b and np.array_equal(a.As, b.As) and np.array_equal(a.log_Ps, b.log_Ps)
    # the selection table recomputed: runs of the val trials decoded again, the test trials' own frames
    stats = arhmm_grid_states(gen, model, fits, dtype='val')
    frames = {(s, int(t)): LENS[int(t)] for s, ds in enumerate(gen.datasets) for t in ds.batch_idxs['test']}
    _same_selection(selection, arhmm_grid_selection(GRID, fits, stats, test_frames=frames))
    _same_selection(selection, sel['selection'])
    n_val = sum(LENS[int(t)] for ds in gen.datasets for t in ds.batch_idxs['val'])
    for cfg, row, (runs, fr, trans) in zip(GRID, selection, stats):
        assert all(row[k] == v for k, v in cfg.items()) and row['epochs'] == 2
        assert np.isfinite([row['tr_loss'], row['val_loss'], row['test_loss']]).all()
        assert fr.sum() == n_val and row['n_runs'] == len(runs) and abs(row['usage'].sum() - 1.0) < 1e-12
        assert 1 <= row['n_states_99'] <= row['n_states_used'] <= cfg['n_states']
        assert row['mean_duration'] == n_val / len(runs)
    # one session, another split
    one = arhmm_grid_states(gen, model, fits, dtype='test', sess_idx=1)
    assert one[0][1].sum() == sum(LENS[int(t)] for t in gen.datasets[1].batch_idxs['test'])


def test_fit_runs_the_grid_export_and_leaves_export_arhmm_as_it_was(tmp_path):
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
                             'export_arhmm': {'n_states': 2, 'n_lags': 1, 'n_iters': 2}})
    hp = case_hparams(meta)
    vdir = os.path.join(str(tmp_path), 'version_0')
    os.makedirs(vdir)
    sess = SyntheticSession(6, 40, meta['dim'], seed=0, n_labels=meta['n_labels'], trial_splits='4;1;1;0')
    gen = SyntheticSessionsGenerator([sess], device=DEV, placement='device_u8')
    model = seeded_build(BUILDERS['ps-vae'], hp).to(DEV)
    model.version = 0

    class Exp(object):
        version = 0

        def log(self, row):
            pass

        def save(self):
            pass
    # export_arhmm alone: its two files, and no grid directory
    fit(hp, model, gen, Exp(), method='ae')
    with open(os.path.join(vdir, ARHMM_MODEL_FILE), 'rb') as f:
        arhmm = pickle.load(f)
    assert isinstance(arhmm, ARHMM) and (arhmm.K, arhmm.lags) == (2, 1)
    assert len([f for f in os.listdir(vdir) if f.endswith('_states.pkl')]) == 1
    assert not os.path.exists(os.path.join(vdir, 'arhmm_grid'))
    # the grid hook
    hp_grid = dict(hp, export_arhmm_grid={'grid': GRID, 'n_iters': 2, 'dtype': 'test'})
    del hp_grid['export_arhmm']
    best = fit(hp_grid, model, gen, Exp(), method='ae')
    # (files, shapes and ranges here; the states themselves are held in the test above)
    sel, _ = _check_grid_files(vdir, gen, best, 3, lambda ds, t, s: np.zeros((40, 1)), exact=False)
    assert [r['epochs'] for r in sel['selection']] == [2, 2, 2]
    assert all(r['usage'].shape == (c['n_states'],) for r, c in zip(sel['selection'], GRID))
    # refused before the first epoch
    with pytest.raises(ValueError, match='export_arhmm_grid'):
        fit(dict(hp, export_arhmm_grid={'n_iters': 2}), model, gen, Exp(), method='ae')
    with pytest.raises(ValueError, match='33 states'):
        fit(dict(hp, export_arhmm_grid={'grid': [{'n_states': 33}]}), model, gen, Exp(), method='ae')
    with pytest.raises(NotImplementedError, match='studentst'):
        fit(dict(hp, export_arhmm_grid={'grid': [{'n_states': 2, 'noise_type': 'studentst'}]}), model, gen, Exp(),
            method='ae')
