"""The ARHMM launches (csrc/arhmm.hip) and the EM fit built on them against the float64 restatements of
tests/arhmm_refs.py.

Tolerances: everything is float64, so for every compared quantity the two INDEPENDENT restatements (direct and folded
density; log-space and scaled forward-backward; looped and einsum moments) give the noise floor at the shape, the
device's bound is 100 x their disagreement -- another summation order over at most 3,000 x 32 terms -- and never less
than 1e-12 of the quantity's scale (sum |terms| for sums, 1 for probabilities).  The bound comes from the restatements
alone; every check prints error, bound and their ratio.

Largest error / bound seen on an MI355X (first run of this file): ll 0.001, gamma 0.010, gamma row sums < 0.001,
xi 0.010, loglik 0.011, moments 0.003, gamma0 and counts < 0.001, Viterbi score 0.010, EM parameters and losses
0.012 -- the device sits at the restatements' own noise floor (error / noise about 1) everywhere.
"""

import os
import pickle

import numpy as np
import pytest
import torch

from behavenet_amd import _hip
from behavenet_amd.models.arhmm import ARHMM
from tests import arhmm_refs as refs

pytestmark = pytest.mark.gpu
DEV = 'cuda'


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


def _random_hmm(rng, K, kind='random'):
    if kind == 'uniform':
        Ps = np.full((K, K), 1.0 / K)
    elif kind == 'absorbing':
        Ps = np.full((K, K), 1e-9) + np.eye(K)
    else:
        Ps = rng.rand(K, K) + 0.1
    Ps /= Ps.sum(axis=1, keepdims=True)
    pi0 = rng.rand(K) + 0.1
    pi0 /= pi0.sum()
    return np.log(Ps), np.log(pi0)


def _model(rng, K, D, L, shift):
    m = ARHMM(K, D, lags=L)
    m.As = 0.3 / max(L, 1) * rng.randn(K, D, L * D)
    m.bs = rng.randn(K, D)
    for k in range(K):
        B = rng.randn(D, D)
        m.Sigmas[k] = B @ B.T / D + 0.2 * np.eye(D)
    m.log_Ps, m.log_pi0 = _random_hmm(rng, K)
    if shift:
        m.shift = rng.randn(D) + 1.0
    return m


def _offsets(L, n_long=(37, 150)):
    """Trials of length 0, L (initial rows only), L + 1 and longer ones, with two rows in front that belong to none."""
    lens = [0, L, L + 1] + list(n_long) + [0, 1]
    return np.cumsum([2] + lens).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------
# bn_arhmm_loglik
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [1, 2, 5, 32])
@pytest.mark.parametrize('D,L', [(1, 0), (3, 1), (16, 1), (32, 1), (12, 4), (7, 8)])
def test_loglik(D, L, K):
    rng = np.random.RandomState(100 * D + 10 * L + K)
    offsets = _offsets(L)
    n = int(offsets[-1]) + 3
    wide = torch.from_numpy((rng.randn(n, D + 3) + 1.5).astype(np.float32)).to(DEV)
    worst = 0.0
    for shift, table in ((True, wide[:, :D]), (False, wide[:, :D].contiguous())):          # ld > D, and ld = D
        m = _model(rng, K, D, L, shift)
        G, cst = m.fold()
        host = table.cpu().numpy()
        direct = refs.loglik_direct(host, offsets, m.As, m.bs, m.Sigmas, L)
        folded = refs.loglik_folded(host, offsets, G, cst, L, m.shift)
        scale = refs.loglik_scale(host, offsets, G, cst, L, m.shift)
        out = torch.full((n, K), -7.0, dtype=torch.float64, device=DEV)
        got = _hip.arhmm_loglik(table, offsets, G, cst, L, shift=m.shift if shift else None, out=out).cpu().numpy()
        in_trial = np.zeros(n, dtype=bool)
        in_trial[offsets[0]:offsets[-1]] = True
        assert np.all(got[~in_trial] == -7.0)              # rows of no trial are not written
        noise = np.abs(direct - folded)[in_trial].max()
        worst = max(worst, _held('ll D=%d L=%d K=%d shift=%s' % (D, L, K, shift),
                                 np.abs(got - direct)[in_trial], noise, scale[in_trial]))
        again = _hip.arhmm_loglik(table, offsets, G, cst, L, shift=m.shift if shift else None).cpu().numpy()
        assert np.array_equal(again[in_trial], got[in_trial])


@pytest.mark.parametrize('D,L', [(3, 1), (12, 4), (5, 0)])
def test_loglik_contains_a_nan_row(D, L):
    rng = np.random.RandomState(D + L)
    K = 5
    offsets = np.asarray([0, 40, 40 + L + 2, 100], dtype=np.int64)
    n = 100
    host = rng.randn(n, D).astype(np.float32)
    m = _model(rng, K, D, L, True)
    G, cst = m.fold()
    clean = _hip.arhmm_loglik(torch.from_numpy(host).to(DEV), offsets, G, cst, L, shift=m.shift).cpu().numpy()
    bad_rows = [20, 39, 40, 99] + ([0] if L else [])       # mid-trial, a trial's last row, an initial row, the end
    expect = np.zeros(n, dtype=bool)
    for r in bad_rows:
        host[r, rng.randint(D)] = np.nan if r != 39 else np.inf
        s = int(np.searchsorted(offsets, r, side='right')) - 1
        expect[r] = True
        for t in range(r + 1, min(r + L + 1, int(offsets[s + 1]))):
            expect[t] = expect[t] or t - int(offsets[s]) >= L          # (an initial row does not look back)
    got = _hip.arhmm_loglik(torch.from_numpy(host).to(DEV), offsets, G, cst, L, shift=m.shift).cpu().numpy()
    assert np.array_equal(~np.isfinite(got).all(axis=1), expect)
    assert np.array_equal(~np.isfinite(got).any(axis=1), expect)      # all K values of such a row
    assert np.array_equal(got[~expect], clean[~expect])


# ------------------------------------------------------------------------------------------------------------
# bn_hmm_forward_backward
# ------------------------------------------------------------------------------------------------------------
FB_LENGTHS = [0, 1, 2, 257, 3000, 0]


@pytest.fixture(scope='module')
def fb_tables():
    """ll in [-1e4, -1e4 + 50] per K, shared by the forward-backward and Viterbi tests (never written)."""
    out = {}
    offsets = np.cumsum([1] + FB_LENGTHS).astype(np.int64)
    for K in (1, 2, 5, 32):
        rng = np.random.RandomState(K)
        ll = -1e4 + 50.0 * rng.rand(int(offsets[-1]) + 2, K)
        out[K] = (ll, offsets)
    return out


@pytest.mark.parametrize('kind', ['absorbing', 'uniform'])
@pytest.mark.parametrize('K', [1, 2, 5, 32])
def test_forward_backward(fb_tables, K, kind):
    ll, offsets = fb_tables[K]
    log_Ps, log_pi0 = _random_hmm(np.random.RandomState(K + 50), K, kind)
    g1, x1, z1 = refs.forward_backward(ll, offsets, log_Ps, log_pi0, refs.fb_log)
    g2, x2, z2 = refs.forward_backward(ll, offsets, log_Ps, log_pi0, refs.fb_scaled)
    ll_d = torch.from_numpy(ll).to(DEV)
    n, S = ll.shape[0], len(offsets) - 1
    gamma = torch.full((n, K), -7.0, dtype=torch.float64, device=DEV)
    g, x, z = _hip.hmm_forward_backward(ll_d, offsets, log_Ps, log_pi0, gamma=gamma)
    g, x, z = g.cpu().numpy(), x.cpu().numpy(), z.cpu().numpy()
    lens = np.diff(offsets)
    in_trial = np.zeros(n, dtype=bool)
    in_trial[offsets[0]:offsets[-1]] = True
    assert np.all(g[~in_trial] == -7.0)
    tag = 'K=%d %s' % (K, kind)
    _held('gamma ' + tag, np.abs(g - g1)[in_trial], np.abs(g1 - g2).max(), 1.0)
    _held('gamma row sums ' + tag, np.abs(g[in_trial].sum(axis=1) - 1.0), np.abs(g2.sum(axis=1)[in_trial] - 1).max(), 1.0)
    _held('xi ' + tag, np.abs(x - x1).max(axis=(1, 2)), np.abs(x1 - x2).max(), np.maximum(lens - 1.0, 1.0))
    zscale = np.asarray([np.abs(ll[a:b]).max(axis=1).sum() if b > a else 1.0 for a, b in refs.trials_of(offsets)])
    _held('loglik ' + tag, np.abs(z - z1), np.abs(z1 - z2).max(), zscale)
    assert z[0] == 0.0 and z[-1] == 0.0                     # empty trials
    assert not x[lens < 2].any()
    # the same bits on a second call
    g_b, x_b, z_b = _hip.hmm_forward_backward(ll_d, offsets, log_Ps, log_pi0)
    assert np.array_equal(g_b.cpu().numpy()[in_trial], g[in_trial])
    assert np.array_equal(x_b.cpu().numpy(), x) and np.array_equal(z_b.cpu().numpy(), z)
    # likelihood only: the same likelihoods, and canary-filled posteriors are not touched
    lib = _hip.load()
    gam_c = torch.full((n, K), 3.25, dtype=torch.float64, device=DEV)
    xi_c = torch.full((S, K, K), 3.25, dtype=torch.float64, device=DEV)
    none_g, none_x, z_only = _hip.hmm_forward_backward(ll_d, offsets, log_Ps, log_pi0, want_posteriors=False,
                                                       gamma=gam_c, xi=xi_c)
    assert none_g is None and none_x is None
    assert np.array_equal(z_only.cpu().numpy(), z)
    # (and through the C entry point with the canaries handed over)
    off_d = torch.from_numpy(offsets).to(DEV)
    lp, l0 = torch.from_numpy(log_Ps).to(DEV), torch.from_numpy(log_pi0).to(DEV)
    z_c = torch.full((S,), 3.25, dtype=torch.float64, device=DEV)
    nbytes = lib.bn_hmm_forward_backward_ws_bytes(n, S, K)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    assert lib.bn_hmm_forward_backward(ll_d.data_ptr(), off_d.data_ptr(), S, K, n, lp.data_ptr(), l0.data_ptr(), 0,
                                       gam_c.data_ptr(), xi_c.data_ptr(), z_c.data_ptr(), ws.data_ptr(), nbytes,
                                       None) == 0
    torch.cuda.synchronize()
    assert bool((gam_c == 3.25).all()) and bool((xi_c == 3.25).all())
    assert np.array_equal(z_c.cpu().numpy(), z)


# ------------------------------------------------------------------------------------------------------------
# bn_arhmm_moments
# ------------------------------------------------------------------------------------------------------------
def _check_moments(tag, host, offsets, gamma, L, shift):
    table = torch.from_numpy(host).to(DEV)
    gamma_d = torch.from_numpy(gamma).to(DEV)
    out_d, g0_d = _hip.arhmm_moments(table, offsets, gamma_d, L, shift=shift)
    out, g0 = out_d.cpu().numpy(), g0_d.cpu().numpy()
    want, want0 = refs.moments(host, offsets, gamma, L, shift)
    other = refs.moments_einsum(host, offsets, gamma, L, shift)
    scale = np.maximum(refs.moments_abs(host, offsets, gamma, L, shift), 1e-300)
    r = _held('moments ' + tag, np.abs(out - want), np.abs(want - other).max(), scale)
    assert np.array_equal(out, out.transpose(0, 2, 1))                  # the same bits in both triangles
    rows_in_trials = float(sum(b - a for a, b in refs.trials_of(offsets)))
    _held('gamma0 ' + tag, np.abs(g0 - want0), 0.0, np.maximum(np.abs(want0), 1.0))
    _held('counts ' + tag, np.abs(out[:, 0, 0].sum() + g0.sum() - rows_in_trials), 0.0, max(rows_in_trials, 1.0))
    out_b, g0_b = _hip.arhmm_moments(table, offsets, gamma_d, L, shift=shift)
    assert torch.equal(out_b, out_d) and torch.equal(g0_b, g0_d)
    return r


@pytest.mark.parametrize('K', [1, 2, 5, 32])
@pytest.mark.parametrize('D,L', [(1, 0), (3, 1), (16, 1), (32, 1), (12, 4), (7, 8)])
def test_moments(D, L, K):
    rng = np.random.RandomState(1000 + 100 * D + 10 * L + K)
    offsets = _offsets(L, n_long=(37, 90))
    n = int(offsets[-1]) + 3
    host = (rng.randn(n, D) + 1.5).astype(np.float32)
    gamma = rng.rand(n, K)
    gamma /= gamma.sum(axis=1, keepdims=True)
    _check_moments('D=%d L=%d K=%d shift' % (D, L, K), host, offsets, gamma, L, rng.randn(D) + 1.5)
    if K == 2:
        _check_moments('D=%d L=%d K=%d no shift' % (D, L, K), host, offsets, gamma, L, None)


@pytest.mark.parametrize('delta', [-1, 0, 1])
def test_moments_at_row_block_boundaries(delta):
    """Three row blocks by the restated plan; a trial boundary one row before, on and one row after each block's
    first row, and a table that ends one row before, on and one row after a block's last row."""
    D, L, K = 3, 2, 5
    blocks, rows = _hip._arhmm_moments_plan(1500, D, L, K)
    assert blocks == 3 and rows == 500
    n = 3 * rows + delta
    assert _hip._arhmm_moments_plan(n, D, L, K)[0] == 3
    rows = _hip._arhmm_moments_plan(n, D, L, K)[1]
    rng = np.random.RandomState(7 + delta)
    host = rng.randn(n, D).astype(np.float32)
    gamma = rng.rand(n, K)
    gamma /= gamma.sum(axis=1, keepdims=True)
    offsets = np.asarray([0, rows + delta, 2 * rows - 1, 2 * rows, 2 * rows + 1, n], dtype=np.int64)
    _check_moments('row blocks %+d' % delta, host, offsets, gamma, L, None)


@pytest.mark.parametrize('D,L,group', [(3, 1, 4), (15, 1, 4), (16, 1, 2), (21, 2, 2), (32, 1, 1)])
def test_moments_at_state_group_boundaries(D, L, group):
    """One state fewer than a workgroup's group of states, a whole group, one more, and two groups and one."""
    assert _hip._arhmm_moments_group(D, L) == group
    rng = np.random.RandomState(D + L)
    offsets = np.asarray([0, 70, 75, 140], dtype=np.int64)
    host = rng.randn(140, D).astype(np.float32)
    for K in sorted({max(group - 1, 1), group, group + 1, 2 * group + 1}):
        gamma = rng.rand(140, K)
        gamma /= gamma.sum(axis=1, keepdims=True)
        _check_moments('state groups D=%d L=%d K=%d' % (D, L, K), host, offsets, gamma, L, None)


def test_moments_ld_and_column_slice():
    rng = np.random.RandomState(3)
    D, L, K = 5, 1, 3
    offsets = np.asarray([0, 50, 120], dtype=np.int64)
    wide = torch.from_numpy(rng.randn(120, 9).astype(np.float32)).to(DEV)
    gamma = rng.rand(120, K)
    gamma /= gamma.sum(axis=1, keepdims=True)
    a = _hip.arhmm_moments(wide[:, :D], offsets, torch.from_numpy(gamma).to(DEV), L)
    b = _hip.arhmm_moments(wide[:, :D].contiguous(), offsets, torch.from_numpy(gamma).to(DEV), L)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------------------
# bn_hmm_viterbi
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [1, 2, 5, 32])
def test_viterbi_path_scores_the_maximum(fb_tables, K):
    """Tie-proof: the restatement's score of the device's path equals the restatement's best score."""
    ll, offsets = fb_tables[K]
    log_Ps, log_pi0 = _random_hmm(np.random.RandomState(K + 9), K)
    ll_d = torch.from_numpy(ll).to(DEV)
    states_d = _hip.hmm_viterbi(ll_d, offsets, log_Ps, log_pi0)
    states = states_d.cpu().numpy()
    assert states.dtype == np.int32 and states.min() >= 0 and states.max() < K
    errs, noises, scales = [], [], []
    for a, b in refs.trials_of(offsets):
        path, best = refs.viterbi(ll[a:b], log_Ps, log_pi0)
        errs.append(abs(refs.path_score(ll[a:b], log_Ps, log_pi0, states[a:b]) - best))
        noises.append(abs(refs.path_score(ll[a:b], log_Ps, log_pi0, path) - best))
        scales.append(max(np.abs(ll[a:b]).max(axis=1).sum() if b > a else 1.0, 1.0))
    _held('viterbi score K=%d' % K, errs, max(noises), scales)
    assert torch.equal(_hip.hmm_viterbi(ll_d, offsets, log_Ps, log_pi0), states_d)


def test_viterbi_on_well_separated_data():
    rng = np.random.RandomState(11)
    K, D, L = 4, 3, 1
    datas, _ = refs.sample_arhmm(rng, K, D, L, [0, 1, 2, 130, 300], sep=4.0)
    m = _model(rng, K, D, L, True)
    m.bs = 4.0 * rng.randn(K, D)
    m.log_Ps, m.log_pi0 = _random_hmm(rng, K, 'absorbing')[0], m.log_pi0
    table, offsets = ARHMM.as_table(datas)
    host = table.cpu().numpy()
    ll = refs.loglik_direct(host, offsets, m.As, m.bs, m.Sigmas, L)
    want = refs.viterbi_table(ll, offsets, m.log_Ps, m.log_pi0)
    got = _hip.hmm_viterbi(torch.from_numpy(ll).to(DEV), offsets, m.log_Ps, m.log_pi0).cpu().numpy()
    assert np.array_equal(got, want)
    assert len(np.unique(want)) > 1
    assert np.array_equal(m.table_states(table, offsets), want)
    assert np.array_equal(m.most_likely_states(datas[4]), want[offsets[4]:offsets[5]])


@pytest.mark.parametrize('K', [2, 5, 32])
def test_viterbi_exact_ties_go_to_the_lowest_state(K):
    T = 200
    offsets = np.asarray([0, T, T + 1], dtype=np.int64)
    log_Ps, log_pi0 = np.full((K, K), -np.log(K)), np.full((K,), -np.log(K))
    ll = np.zeros((T + 1, K))
    got = _hip.hmm_viterbi(torch.from_numpy(ll).to(DEV), offsets, log_Ps, log_pi0).cpu().numpy()
    assert not got.any()
    # states K - 2 and K - 1 tie above the others (exact: the same column twice)
    ll = np.random.RandomState(K).randn(T + 1, K) - 30.0
    ll[:, K - 2] = 5.0 * np.random.RandomState(K + 1).rand(T + 1)
    ll[:, K - 1] = ll[:, K - 2]
    got = _hip.hmm_viterbi(torch.from_numpy(ll).to(DEV), offsets, log_Ps, log_pi0).cpu().numpy()
    assert np.all(got == K - 2)


# ------------------------------------------------------------------------------------------------------------
# EM
# ------------------------------------------------------------------------------------------------------------
def _param_errs(a, b):
    return {name: np.abs(getattr(a, name) - getattr(b, name)).max()
            for name in ('As', 'bs', 'Sigmas', 'log_Ps', 'log_pi0')}


def test_five_em_iterations_against_the_reference_iteration():
    rng = np.random.RandomState(21)
    K, D, L = 4, 6, 1
    train, _ = refs.sample_arhmm(rng, K, D, L, list(rng.randint(150, 301, size=12)), sep=1.5)
    rng2 = np.random.RandomState(22)
    val = [refs.sample_arhmm(rng2, K, D, L, [int(t)], sep=1.5)[0][0] for t in rng2.randint(150, 301, size=3)]
    table, offsets = ARHMM.as_table(train)
    vtable, voffsets = ARHMM.as_table(val)
    host, vhost = table.cpu().numpy(), vtable.cpu().numpy()
    dev = ARHMM(K, D, lags=L)
    dev.initialize(table, offsets, seed=3)
    ref1, ref2 = pickle.loads(pickle.dumps(dev)), pickle.loads(pickle.dumps(dev))
    frames, vframes = float(offsets[-1] * D), float(voffsets[-1] * D)
    tr_dev, priors = [], []
    for it in range(5):
        priors.append(dev.log_prior())
        v1 = refs.trial_logliks(ref1, vhost, voffsets).sum()
        v2 = refs.trial_logliks(ref2, vhost, voffsets, second_form=True).sum()
        vd = dev.trial_logliks(vtable, voffsets).sum()
        t1 = refs.em_iteration(ref1, host, offsets).sum()
        t2 = refs.em_iteration(ref2, host, offsets, second_form=True).sum()
        td = dev.em_step(table, offsets).sum()
        tr_dev.append(td)
        _held('EM %d tr_loss' % it, abs(td - t1) / frames, abs(t1 - t2) / frames, abs(t1) / frames)
        _held('EM %d val_loss' % it, abs(vd - v1) / vframes, abs(v1 - v2) / vframes, abs(v1) / vframes)
        noise = _param_errs(ref1, ref2)
        for name, err in _param_errs(dev, ref1).items():
            _held('EM %d %s' % (it, name), err, noise[name], max(np.abs(getattr(ref1, name)).max(), 1.0))
    tr_dev.append(dev.trial_logliks(table, offsets).sum())
    priors.append(dev.log_prior())
    # EM never lowers likelihood + log prior (1e-12 of the likelihood's scale for the device's rounding), so the
    # training likelihood alone can fall by no more than the prior rose
    tr_dev, priors = np.asarray(tr_dev), np.asarray(priors)
    print('training log-likelihood per iteration', tr_dev, 'log prior', priors)
    assert np.all(np.diff(tr_dev + priors) >= -1e-12 * np.abs(tr_dev[:-1]) * 100), (tr_dev, priors)
    assert np.all(np.diff(tr_dev) >= -np.maximum(np.diff(priors), 0.0) - 1e-10 * np.abs(tr_dev[:-1]))
    assert tr_dev[-1] > tr_dev[0]


# ------------------------------------------------------------------------------------------------------------
# fit_arhmm, export_states, the fit() hook
# ------------------------------------------------------------------------------------------------------------
def _row_layout(rows, n_epochs, sessions, test_trials):
    """The reference's exp.log layout: per epoch one pooled row and one a session, then one row a test trial."""
    k = 0
    for epoch in range(n_epochs):
        for d in [-1] + sessions:
            assert set(rows[k]) == {'epoch', 'dataset', 'tr_loss', 'val_loss', 'trial'}
            assert (rows[k]['epoch'], rows[k]['dataset'], rows[k]['trial']) == (epoch, d, -1)
            assert np.isfinite(rows[k]['tr_loss']) and np.isfinite(rows[k]['val_loss'])
            k += 1
    for d, trial in test_trials:
        assert set(rows[k]) == {'epoch', 'dataset', 'test_loss', 'trial'}
        assert (rows[k]['epoch'], rows[k]['dataset'], rows[k]['trial']) == (n_epochs - 1, d, trial)
        assert np.isfinite(rows[k]['test_loss'])
        k += 1
    assert k == len(rows)


def test_fit_arhmm_and_export_states_on_the_synthetic_generator(tmp_path):
    from behavenet_amd.fitting.eval import (export_states, fit_arhmm, fit_arhmm_tables)
    from tests.test_gpu_latent_corr import _per_trial_latents
    from tests.test_gpu_ranges import LENS, _generator, _model as _ae
    root = str(tmp_path)
    model, meta = _ae('ae_cfg1', root)
    gen = _generator(meta, n_sessions=2, n_labels=3)
    kw = dict(n_states=2, n_lags=1, n_iters=3, rng_seed_model=1)
    arhmm, rows = fit_arhmm(gen, model, **kw)
    tests = [(s, int(t)) for s, ds in enumerate(gen.datasets) for t in ds.batch_idxs['test']]
    _row_layout(rows, 4, [0, 1], tests)
    assert (arhmm.K, arhmm.D, arhmm.lags) == (2, int(model.hparams['n_ae_latents']), 1)
    # the same fit from the per-trial latents, with no generator: the same rows and parameters
    splits = {dt: [torch.from_numpy(_per_trial_latents(model, gen, [dt], [s])[0][a:b]).to(DEV)
                   for s in (0, 1) for a, b in _trial_bounds(_per_trial_latents(model, gen, [dt], [s])[1])]
              for dt in ('train', 'val', 'test')}
    arhmm_t, rows_t = fit_arhmm_tables(splits['train'], splits['val'], splits['test'], **kw)
    pooled = [r for r in rows if r['dataset'] == -1]
    pooled_t = [r for r in rows_t if r['dataset'] == -1]
    for a, b in zip(pooled, pooled_t):
        assert abs(a['tr_loss'] - b['tr_loss']) <= 1e-6 * abs(b['tr_loss'])          # (another encoder batching)
        assert abs(a['val_loss'] - b['val_loss']) <= 1e-6 * abs(b['val_loss'])
    # the pooled loss is the frame-weighted mean of the sessions'
    frames = [sum(LENS[int(t)] for t in ds.batch_idxs['train']) for ds in gen.datasets]
    for epoch in range(4):
        per = [r['tr_loss'] for r in rows if r['epoch'] == epoch and r['dataset'] >= 0 and 'tr_loss' in r]
        assert abs(np.dot(per, frames) / sum(frames) - pooled[epoch]['tr_loss']) <= 1e-12 * abs(pooled[epoch]['tr_loss'])
    one = fit_arhmm(gen, model, sess_idx=1, **kw)[1]
    _row_layout(one, 4, [1], [k for k in tests if k[0] == 1])

    hp = {'expt_dir': root, 'version': 0, 'model_class': 'arhmm'}
    files = export_states(hp, gen, arhmm, model=model)
    assert files == [os.path.join(root, 'version_0', 'lab_expt_animal_sess%d_states.pkl' % s) for s in (0, 1)]
    for s, path in enumerate(files):
        with open(path, 'rb') as f:
            d = pickle.load(f)
        ds = gen.datasets[s]
        assert set(d) == {'states', 'trials'} and len(d['states']) == ds.n_trials
        assert all(np.array_equal(d['trials'][dt], ds.batch_idxs[dt]) for dt in ('train', 'val', 'test'))
        in_split = set(int(t) for dt in ('train', 'val', 'test') for t in ds.batch_idxs[dt])
        assert len(in_split) == ds.n_trials - 3
        for t in range(ds.n_trials):
            if t in in_split:
                assert d['states'][t].shape == (LENS[t],) and d['states'][t].dtype == np.int32
                z = _encode_one(model, ds, t, s)
                assert np.array_equal(d['states'][t], arhmm.most_likely_states(z))
            else:
                assert d['states'][t].size == 0              # gap trials
    # labels in place of latents
    arhmm_l, rows_l = fit_arhmm(gen, None, data_key='labels', n_states=2, n_lags=2, n_iters=2)
    assert (arhmm_l.D, arhmm_l.lags) == (3, 2)
    _row_layout(rows_l, 3, [0, 1], tests)
    files = export_states(dict(hp, model_class='arhmm-labels'), gen, arhmm_l,
                          filename=os.path.join(root, 'label_states.pkl'))
    with open(files[-1], 'rb') as f:
        d = pickle.load(f)
    t = int(gen.datasets[1].batch_idxs['val'][0])
    assert np.array_equal(d['states'][t], arhmm_l.most_likely_states(gen.datasets[1].labels[t]))
    with pytest.raises(NotImplementedError, match='studentst'):
        fit_arhmm(gen, model, n_states=2, noise_type='studentst')
    with pytest.raises(NotImplementedError, match='recurrent'):
        fit_arhmm(gen, model, n_states=2, transitions='recurrent')


def _trial_bounds(keys):
    pos = 0
    for _, _, rows in keys:
        yield pos, pos + rows
        pos += rows


def _encode_one(model, ds, t, s):
    from behavenet_amd.fitting.eval import encode_trial
    return np.asarray(encode_trial(model, torch.from_numpy(ds.images_u8[int(t)]).to(DEV), s), dtype=np.float32)


def test_fit_writes_the_arhmm_and_its_states(tmp_path):
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
    os.makedirs(os.path.join(str(tmp_path), 'version_0'))
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
    fit(hp, model, gen, Exp(), method='ae')
    vdir = os.path.join(str(tmp_path), 'version_0')
    with open(os.path.join(vdir, ARHMM_MODEL_FILE), 'rb') as f:
        arhmm = pickle.load(f)
    assert isinstance(arhmm, ARHMM) and (arhmm.K, arhmm.lags) == (2, 1)
    states = [f for f in os.listdir(vdir) if f.endswith('_states.pkl')]
    assert len(states) == 1
    with open(os.path.join(vdir, states[0]), 'rb') as f:
        d = pickle.load(f)
    assert [len(s) for s in d['states']] == [40] * 6
    with pytest.raises(ValueError, match="export_arhmm"):
        fit(dict(hp, export_arhmm={'n_lags': 1}), model, gen, Exp(), method='ae')
    with pytest.raises(ValueError, match="40 states"):
        fit(dict(hp, export_arhmm={'n_states': 40}), model, gen, Exp(), method='ae')
