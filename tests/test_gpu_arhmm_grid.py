"""A grid of ARHMMs on one table (bn_arhmm_grid_loglik, bn_hmm_grid_forward_backward, bn_arhmm_grid_moments;
models.arhmm.ARHMMGroup; fitting.eval.fit_arhmm_grid_tables) against the float64 restatements of tests/arhmm_refs.py.

Tolerances are those of tests/test_gpu_arhmm.py and nothing new: for every compared quantity two INDEPENDENT float64
restatements (direct and folded density; log-space and scaled forward-backward; looped and einsum moments) give the
noise floor at the shape, and the device is held to max(100 x their disagreement, 1e-12 x the quantity's scale).  Every
check prints error, bound and their ratio.  What must be equal bit for bit -- a model's results in another slot, in
another wave, next to other models -- is compared with array_equal.
"""

import pickle

import numpy as np
import pytest
import torch

from behavenet_amd import _hip
from behavenet_amd.models.arhmm import ARHMM, ARHMMGroup
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


def _model(rng, K, D, L, shift=None):
    m = ARHMM(K, D, lags=L)
    m.As = 0.3 / max(L, 1) * rng.randn(K, D, L * D)
    m.bs = rng.randn(K, D)
    for k in range(K):
        B = rng.randn(D, D)
        m.Sigmas[k] = B @ B.T / D + 0.2 * np.eye(D)
    m.log_Ps, m.log_pi0 = _random_hmm(rng, K)
    if shift is not None:
        m.shift = shift.copy()
    return m


def _offsets(L, n_long=(37, 150)):
    """Trials of length 0, L (initial rows only), L + 1 and longer ones, with two rows in front that belong to none."""
    lens = [0, L, L + 1] + list(n_long) + [0, 1]
    return np.cumsum([2] + lens).astype(np.int64)


KINDS = ('random', 'absorbing', 'uniform')


def _hmm_grid(seed, Ks, lengths):
    """ll in [-1e4, -1e4 + 50], the transition kinds in turn: (ll (n, KT), offsets, [(log_Ps, log_pi0)])."""
    rng = np.random.RandomState(seed)
    offsets = np.cumsum([2] + list(lengths)).astype(np.int64)
    ll = -1e4 + 50.0 * rng.rand(int(offsets[-1]) + 2, int(np.sum(Ks)))
    hmms = [_random_hmm(rng, K, KINDS[m % 3]) for m, K in enumerate(Ks)]
    return ll, offsets, hmms


def _run_grid(ll, offsets, Ks, hmms, want=True, canary=-7.0):
    log_Ps = np.concatenate([h[0].reshape(-1) for h in hmms])
    log_pi0 = np.concatenate([h[1] for h in hmms])
    gamma = torch.full(tuple(ll.shape), canary, dtype=torch.float64, device=DEV)
    g, x, z = _hip.hmm_grid_forward_backward(torch.from_numpy(ll).to(DEV), offsets, Ks, log_Ps, log_pi0,
                                             want_posteriors=want, gamma=gamma if want else None)
    if not want:
        assert g is None and x is None
        return None, None, z.cpu().numpy()
    return g.cpu().numpy(), x.cpu().numpy(), z.cpu().numpy()


def _per_model(Ks, g, x, z):
    koff = np.concatenate(([0], np.cumsum(Ks)))
    xoff = np.concatenate(([0], np.cumsum(np.asarray(Ks) ** 2)))
    S = x.shape[0]
    return [(g[:, koff[m]:koff[m + 1]], x[:, xoff[m]:xoff[m + 1]].reshape(S, K, K), z[m]) for m, K in enumerate(Ks)]


def _check_fb_against_refs(tag, ll, offsets, Ks, hmms, g, x, z, z_only):
    n = ll.shape[0]
    lens = np.diff(offsets)
    in_trial = np.zeros(n, dtype=bool)
    in_trial[offsets[0]:offsets[-1]] = True
    assert np.all(g[~in_trial] == -7.0)                     # rows of no trial are not written
    koff = np.concatenate(([0], np.cumsum(Ks)))
    for m, (gm, xm, zm) in enumerate(_per_model(Ks, g, x, z)):
        K = Ks[m]
        llm = np.ascontiguousarray(ll[:, koff[m]:koff[m + 1]])
        g1, x1, z1 = refs.forward_backward(llm, offsets, hmms[m][0], hmms[m][1], refs.fb_log)
        g2, x2, z2 = refs.forward_backward(llm, offsets, hmms[m][0], hmms[m][1], refs.fb_scaled)
        t = '%s model %d K=%d %s' % (tag, m, K, KINDS[m % 3])
        _held('gamma ' + t, np.abs(gm - g1)[in_trial], np.abs(g1 - g2).max(), 1.0)
        _held('gamma row sums ' + t, np.abs(gm[in_trial].sum(axis=1) - 1.0),
              np.abs(g2.sum(axis=1)[in_trial] - 1).max(), 1.0)
        _held('xi ' + t, np.abs(xm - x1).max(axis=(1, 2)), np.abs(x1 - x2).max(), np.maximum(lens - 1.0, 1.0))
        zscale = np.asarray([np.abs(llm[a:b]).max(axis=1).sum() if b > a else 1.0 for a, b in refs.trials_of(offsets)])
        _held('loglik ' + t, np.abs(zm - z1), np.abs(z1 - z2).max(), zscale)
        _held('loglik, forward only ' + t, np.abs(z_only[m] - z1), np.abs(z1 - z2).max(), zscale)
        assert np.array_equal(z_only[m], zm)                # the same sweep
        assert zm[0] == 0.0 and zm[-1] == 0.0               # empty trials
        assert not xm[lens < 2].any()


# ------------------------------------------------------------------------------------------------------------
# bn_hmm_grid_forward_backward
# ------------------------------------------------------------------------------------------------------------
CLASS_KS = {4: [1, 2, 3, 4], 8: [5, 6, 7, 8], 16: [9, 16, 12, 10, 13], 32: [17, 32, 25]}


@pytest.mark.parametrize('KP', [4, 8, 16, 32])
def test_packed_forward_backward_one_class(KP):
    """64 / KP + 1 models of one class: a full wave and a wave with a single filled slot; the state counts span the
    class's range, both ends included."""
    n_models = 64 // KP + 1
    Ks = [CLASS_KS[KP][m % len(CLASS_KS[KP])] for m in range(n_models)]
    assert min(Ks) == KP // 2 + 1 if KP > 4 else min(Ks) == 1
    assert max(Ks) == KP
    cls, wave, slot = _hip.hmm_grid_plan(Ks)
    assert set(cls.tolist()) == {KP} and wave.tolist() == [0] * (64 // KP) + [1] and slot[-1] == 0
    ll, offsets, hmms = _hmm_grid(KP, Ks, [0, 1, 2, KP - 1, KP, KP + 1, 65, 257, 0])
    g, x, z = _run_grid(ll, offsets, Ks, hmms)
    z_only = _run_grid(ll, offsets, Ks, hmms, want=False)[2]
    _check_fb_against_refs('KP=%d' % KP, ll, offsets, Ks, hmms, g, x, z, z_only)
    g_b, x_b, z_b = _run_grid(ll, offsets, Ks, hmms)        # the same bits on a second call
    assert np.array_equal(g_b, g) and np.array_equal(x_b, x) and np.array_equal(z_b, z)


MIXED_KS = [1, 4, 5, 8, 9, 16, 17, 32]
MIXED_LENGTHS = [0, 1, 2, 7, 33, 65, 130, 0]


def test_packed_forward_backward_all_classes_in_one_call():
    assert sum(MIXED_KS) == 92 and _hip.hmm_grid_plan(MIXED_KS)[0].tolist() == [4, 4, 8, 8, 16, 16, 32, 32]
    ll, offsets, hmms = _hmm_grid(92, MIXED_KS, MIXED_LENGTHS)
    g, x, z = _run_grid(ll, offsets, MIXED_KS, hmms)
    z_only = _run_grid(ll, offsets, MIXED_KS, hmms, want=False)[2]
    _check_fb_against_refs('mixed', ll, offsets, MIXED_KS, hmms, g, x, z, z_only)


def test_forward_only_touches_neither_gamma_nor_xi():
    ll, offsets, hmms = _hmm_grid(5, MIXED_KS, MIXED_LENGTHS)
    lib = _hip.load()
    n, S, M, KT, XT = ll.shape[0], len(offsets) - 1, len(MIXED_KS), 92, int(np.sum(np.asarray(MIXED_KS) ** 2))
    z = _run_grid(ll, offsets, MIXED_KS, hmms)[2]
    order, counts = _hip._hmm_grid_order(MIXED_KS)
    koff, xoff = _hip.check_arhmm_grid_states('test', MIXED_KS)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    gam_c = torch.full((n, KT), 3.25, dtype=torch.float64, device=DEV)
    xi_c = torch.full((S, XT), 3.25, dtype=torch.float64, device=DEV)
    z_c = torch.full((M, S), 3.25, dtype=torch.float64, device=DEV)
    ops = [dev(ll), dev(offsets), dev(koff), dev(xoff), dev(order), dev(np.concatenate([h[0].reshape(-1) for h in hmms])),
           dev(np.concatenate([h[1] for h in hmms]))]
    nbytes = lib.bn_hmm_grid_forward_backward_ws_bytes(n, S, M, KT, XT)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    assert lib.bn_hmm_grid_forward_backward(ops[0].data_ptr(), ops[1].data_ptr(), S, M, KT, XT, n, ops[2].data_ptr(),
                                            ops[3].data_ptr(), ops[4].data_ptr(), *counts, ops[5].data_ptr(),
                                            ops[6].data_ptr(), 0, gam_c.data_ptr(), xi_c.data_ptr(), z_c.data_ptr(),
                                            ws.data_ptr(), nbytes, None) == 0
    torch.cuda.synchronize()
    assert bool((gam_c == 3.25).all()) and bool((xi_c == 3.25).all())
    assert np.array_equal(z_c.cpu().numpy(), z)
    # a workspace one byte short is refused and nothing is written
    z_c.fill_(3.25)
    assert lib.bn_hmm_grid_forward_backward(ops[0].data_ptr(), ops[1].data_ptr(), S, M, KT, XT, n, ops[2].data_ptr(),
                                            ops[3].data_ptr(), ops[4].data_ptr(), *counts, ops[5].data_ptr(),
                                            ops[6].data_ptr(), 0, None, None, z_c.data_ptr(), ws.data_ptr(),
                                            nbytes - 1, None) == -2
    torch.cuda.synchronize()
    assert bool((z_c == 3.25).all())


# ------------------------------------------------------------------------------------------------------------
# a model's bits do not depend on its slot, its wave or its neighbours
# ------------------------------------------------------------------------------------------------------------
def _mixed_group(seed, Ks, D=3, L=1):
    rng = np.random.RandomState(seed)
    offsets = _offsets(L, n_long=(37, 70))
    n = int(offsets[-1]) + 3
    host = (rng.randn(n, D) + 1.5).astype(np.float32)
    shift = rng.randn(D) + 1.0
    return [_model(rng, K, D, L, shift) for K in Ks], host, offsets


def _group_e_step(models, host, offsets):
    """(ll, gamma, xi, loglik) per model through the three wrappers, host arrays."""
    group = ARHMMGroup(models)
    table = torch.from_numpy(host).to(DEV)
    G, cst = group.fold()
    ll = _hip.arhmm_grid_loglik(table, offsets, G, cst, group.lags, shift=models[0].shift)
    log_Ps, log_pi0 = group._transitions()
    gamma, xi, z = _hip.hmm_grid_forward_backward(ll, offsets, group.Ks, log_Ps, log_pi0)
    mom, g0 = _hip.arhmm_grid_moments(table, offsets, gamma, group.lags, shift=models[0].shift)
    ll, gamma, xi, z, mom, g0 = (t.cpu().numpy() for t in (ll, gamma, xi, z, mom, g0))
    out = []
    for m in range(group.M):
        k0, k1, x0, x1 = group.koff[m], group.koff[m + 1], group.xoff[m], group.xoff[m + 1]
        out.append((ll[:, k0:k1], gamma[:, k0:k1], xi[:, x0:x1], z[m], mom[k0:k1], g0[k0:k1]))
    return out


def _same_bits(a, b, in_trial):
    for u, v in zip(a[:2], b[:2]):
        assert np.array_equal(u[in_trial], v[in_trial])
    for u, v in zip(a[2:], b[2:]):
        assert np.array_equal(u, v)


def test_a_model_s_bits_do_not_depend_on_its_slot():
    models, host, offsets = _mixed_group(31, MIXED_KS)
    in_trial = np.zeros(len(host), dtype=bool)
    in_trial[offsets[0]:offsets[-1]] = True
    forward = _group_e_step(models, host, offsets)
    backward = _group_e_step(models[::-1], host, offsets)[::-1]
    plan_f, plan_b = _hip.hmm_grid_plan(MIXED_KS), _hip.hmm_grid_plan(MIXED_KS[::-1])
    moved = [m for m in range(8) if (plan_f[1][m], plan_f[2][m]) != (plan_b[1][7 - m], plan_b[2][7 - m])]
    assert len(moved) == 8                                  # every model sits in another slot
    for a, b in zip(forward, backward):
        assert np.isfinite(a[1][in_trial]).all() and np.isfinite(a[3]).all()
        _same_bits(a, b, in_trial)
    # the same configuration twice in one group, and next to other neighbours: identical bits
    twice = _group_e_step([models[2], models[7], models[2], models[0]], host, offsets)
    _same_bits(twice[0], twice[2], in_trial)
    _same_bits(twice[0], forward[2], in_trial)
    _same_bits(twice[1], forward[7], in_trial)
    # ... and 17 models of one class: the first slot of the second wave against a slot of the first
    many = _group_e_step([models[1]] * 17, host, offsets)
    _same_bits(many[16], many[3], in_trial)
    _same_bits(many[16], forward[1], in_trial)
    # forward-backward of a model alone in a group is the grid's
    alone = _group_e_step([models[5]], host, offsets)
    _same_bits(alone[0], forward[5], in_trial)


def test_a_nan_stays_in_its_model():
    """A value test: nothing faults, the NaN is an operand."""
    ll, offsets, hmms = _hmm_grid(77, MIXED_KS, MIXED_LENGTHS)
    clean = _per_model(MIXED_KS, *_run_grid(ll, offsets, MIXED_KS, hmms))
    lens = np.diff(offsets)
    for bad in (1, 4, 7):                                   # K = 4 (shares its wave with K = 1), 9 and 32
        dirty = [(h[0].copy(), h[1]) for h in hmms]
        dirty[bad][0][0, 0] = np.nan
        got = _per_model(MIXED_KS, *_run_grid(ll, offsets, MIXED_KS, dirty))
        for m in range(len(MIXED_KS)):
            if m != bad:
                for u, v in zip(got[m], clean[m]):
                    assert np.array_equal(u, v)             # (rows of no trial hold the canary in both)
                continue
            g, x, z = got[m]
            for s, (a, b) in enumerate(refs.trials_of(offsets)):
                if lens[s] >= 2:                            # the transition matrix enters from the second row on
                    assert not np.isfinite(z[s]) and not np.isfinite(g[a:b]).any() and not np.isfinite(x[s]).any()
                else:
                    assert np.array_equal(g[a:b], clean[m][0][a:b]) and z[s] == clean[m][2][s]


# ------------------------------------------------------------------------------------------------------------
# bn_arhmm_grid_loglik and bn_arhmm_grid_moments above 32 states
# ------------------------------------------------------------------------------------------------------------
def _split_states(KT):
    Ks = []
    while KT > 0:
        Ks.append(min(KT, 32 if len(Ks) % 2 == 0 else 12))
        KT -= Ks[-1]
    return Ks


@pytest.mark.parametrize('KT', [33, 77])
@pytest.mark.parametrize('D,L', [(3, 1), (16, 1), (32, 1), (7, 8), (5, 0)])
def test_loglik_and_moments_above_32_states(D, L, KT):
    rng = np.random.RandomState(100 * D + 10 * L + KT)
    offsets = _offsets(L, n_long=(37, 90))
    n = int(offsets[-1]) + 3
    host = (rng.randn(n, D) + 1.5).astype(np.float32)
    shift = rng.randn(D) + 1.0
    Ks = _split_states(KT)
    assert sum(Ks) == KT and KT % 16 and KT % 4 and KT % 2
    models = [_model(rng, K, D, L, shift) for K in Ks]
    group = ARHMMGroup(models)
    G, cst = group.fold()
    table = torch.from_numpy(host).to(DEV)
    in_trial = np.zeros(n, dtype=bool)
    in_trial[offsets[0]:offsets[-1]] = True
    out = torch.full((n, KT), -7.0, dtype=torch.float64, device=DEV)
    got = _hip.arhmm_grid_loglik(table, offsets, G, cst, L, shift=shift, out=out).cpu().numpy()
    assert np.all(got[~in_trial] == -7.0)
    direct = np.concatenate([refs.loglik_direct(host, offsets, m.As, m.bs, m.Sigmas, L) for m in models], axis=1)
    folded = refs.loglik_folded(host, offsets, G, cst, L, shift)
    scale = refs.loglik_scale(host, offsets, G, cst, L, shift)
    tag = 'D=%d L=%d KT=%d' % (D, L, KT)
    _held('ll ' + tag, np.abs(got - direct)[in_trial], np.abs(direct - folded)[in_trial].max(), scale[in_trial])
    # a model's columns are the single-model launch's, bit for bit
    k0 = int(group.koff[1])
    single = _hip.arhmm_loglik(table, offsets, *models[1].fold(), L, shift=shift).cpu().numpy()
    assert np.array_equal(got[in_trial, k0:k0 + Ks[1]], single[in_trial])

    gamma = rng.rand(n, KT)
    gamma /= gamma.sum(axis=1, keepdims=True)
    gamma_d = torch.from_numpy(gamma).to(DEV)
    mom_d, g0_d = _hip.arhmm_grid_moments(table, offsets, gamma_d, L, shift=shift)
    mom, g0 = mom_d.cpu().numpy(), g0_d.cpu().numpy()
    want, want0 = refs.moments(host, offsets, gamma, L, shift)
    other = refs.moments_einsum(host, offsets, gamma, L, shift)
    mscale = np.maximum(refs.moments_abs(host, offsets, gamma, L, shift), 1e-300)
    _held('moments ' + tag, np.abs(mom - want), np.abs(want - other).max(), mscale)
    assert np.array_equal(mom, mom.transpose(0, 2, 1))
    rows_in_trials = float(sum(b - a for a, b in refs.trials_of(offsets)))
    _held('gamma0 ' + tag, np.abs(g0 - want0), 0.0, np.maximum(np.abs(want0), 1.0))
    _held('counts ' + tag, np.abs(mom[:, 0, 0].sum() + g0.sum() - rows_in_trials), 0.0, max(rows_in_trials, 1.0))
    again = _hip.arhmm_grid_moments(table, offsets, gamma_d, L, shift=shift)
    assert torch.equal(again[0], mom_d) and torch.equal(again[1], g0_d)


def test_the_limits_hold_on_the_device_too():
    table = torch.zeros((10, 3), device=DEV)
    with pytest.raises(ValueError, match='513 states'):
        _hip.arhmm_grid_loglik(table, [0, 10], np.zeros((513, 3, 7)), np.zeros(513), 1)
    with pytest.raises(ValueError, match='513 states'):
        _hip.arhmm_grid_moments(table, [0, 10], torch.zeros((10, 513), dtype=torch.float64, device=DEV), 1)
    with pytest.raises(ValueError, match='33 states'):
        _hip.arhmm_loglik(table, [0, 10], np.zeros((33, 3, 7)), np.zeros(33), 1)


def _ar_rows(host, offsets, gamma, L, shift):
    """(a (R, P), gamma (R, KT)) of the AR rows of every trial, float64."""
    a, g = [], []
    for beg, end in refs.trials_of(offsets):
        if end - beg > L:
            a.append(refs.lagged_rows(host[beg:end], L, shift))
            g.append(gamma[beg + L:end])
    return np.concatenate(a), np.concatenate(g)


def test_moments_where_the_row_blocks_must_grow():
    """KT = 512 at P = 65: a set of partials is 17.3 MB, so 60 MiB hold three row blocks and 2,100 rows are cut into
    blocks of 700, not of 512.  The trial boundaries sit around the block boundaries of the host's restatement of the
    plan; the workspace query -- the launch's own partition -- is held against the same restatement.  References:
    the weights folded into the rows, one matrix product a state; and the rows' outer products formed first, one
    matrix product for all states (4.5 GFLOP of float64 each, through BLAS)."""
    D, L, KT, n = 32, 1, 512, 2100
    P = 1 + (L + 1) * D
    blocks, rows = _hip._arhmm_moments_plan(n, D, L, KT)
    assert (blocks, rows) == (3, 700)
    lib = _hip.load()
    offsets = np.asarray([0, rows - 1, rows, rows + 1, 2 * rows, n], dtype=np.int64)
    S = len(offsets) - 1
    assert lib.bn_arhmm_grid_moments_ws_bytes(n, S, D, L, KT) == 32 + (n + 15) // 16 * 16 + blocks * KT * P * P * 8
    rng = np.random.RandomState(512)
    host = (rng.randn(n, D) + 0.5).astype(np.float32)
    shift = rng.randn(D)
    gamma = rng.rand(n, KT)
    gamma /= gamma.sum(axis=1, keepdims=True)
    table, gamma_d = torch.from_numpy(host).to(DEV), torch.from_numpy(gamma).to(DEV)
    mom_d, g0_d = _hip.arhmm_grid_moments(table, offsets, gamma_d, L, shift=shift)
    mom, g0 = mom_d.cpu().numpy(), g0_d.cpu().numpy()
    a, g = _ar_rows(host, offsets, gamma, L, shift)
    want = np.stack([(a * g[:, k:k + 1]).T @ a for k in range(KT)])
    outer = (a[:, :, None] * a[:, None, :]).reshape(len(a), P * P)
    other = (g.T @ outer).reshape(KT, P, P)
    scale = np.maximum((np.abs(g).T @ np.abs(outer)).reshape(KT, P, P), 1e-300)
    _held('moments KT=512', np.abs(mom - want), np.abs(want - other).max(), scale)
    assert np.array_equal(mom, mom.transpose(0, 2, 1))
    want0 = np.zeros(KT)
    for beg, end in refs.trials_of(offsets):
        want0 += gamma[beg:min(beg + L, end)].sum(axis=0)
    _held('gamma0 KT=512', np.abs(g0 - want0), 0.0, np.maximum(np.abs(want0), 1.0))
    _held('counts KT=512', np.abs(mom[:, 0, 0].sum() + g0.sum() - float(n)), 0.0, float(n))
    # the log-likelihoods of 512 states: 32 tiles of 16 a wave
    models = [_model(rng, 32, D, L, shift) for _ in range(2)]
    G, cst = ARHMMGroup(models * 8).fold()
    got = _hip.arhmm_grid_loglik(table, offsets, G, cst, L, shift=shift).cpu().numpy()
    direct = np.concatenate([refs.loglik_direct(host, offsets, m.As, m.bs, m.Sigmas, L) for m in models], axis=1)
    folded = refs.loglik_folded(host, offsets, G[:64], cst[:64], L, shift)
    lscale = refs.loglik_scale(host, offsets, G[:64], cst[:64], L, shift)
    for rep in range(8):
        assert np.array_equal(got[:, 64 * rep:64 * rep + 64], got[:, :64])      # the same states in other tiles
    _held('ll KT=512', np.abs(got[:, :64] - direct), np.abs(direct - folded).max(), lscale)


# ------------------------------------------------------------------------------------------------------------
# EM
# ------------------------------------------------------------------------------------------------------------
PARAMS = ('As', 'bs', 'Sigmas', 'log_Ps', 'log_pi0')
EM_CONFIGS = [(2, 0), (2, 100), (4, 0), (4, 100)]            # (K, kappa)


def _em_data():
    """The data of tests/test_gpu_arhmm.py::test_five_em_iterations_against_the_reference_iteration."""
    rng = np.random.RandomState(21)
    K, D, L = 4, 6, 1
    train, _ = refs.sample_arhmm(rng, K, D, L, list(rng.randint(150, 301, size=12)), sep=1.5)
    rng2 = np.random.RandomState(22)
    val = [refs.sample_arhmm(rng2, K, D, L, [int(t)], sep=1.5)[0][0] for t in rng2.randint(150, 301, size=3)]
    return train, val


def _em_model(K, kappa, D=6, L=1):
    return ARHMM(K, D, lags=L, transitions='sticky' if kappa else 'stationary', kappa=kappa)


@pytest.fixture(scope='module')
def em_run():
    """Five EM iterations of the group on the device, run ONCE: per iteration the models as they were before it,
    their training and validation log-likelihoods and log priors; and the state after the last iteration."""
    train, val = _em_data()
    table, offsets = ARHMM.as_table(train)
    vtable, voffsets = ARHMM.as_table(val)
    models = [_em_model(K, kappa) for K, kappa in EM_CONFIGS]
    for m in models:
        m.initialize(table, offsets, seed=3)
    group = ARHMMGroup(models)
    start = pickle.dumps(models)
    steps = []
    for it in range(5):
        priors = [m.log_prior() for m in models]
        vd = group.trial_logliks(vtable, voffsets).sum(axis=1)
        td = group.em_step(table, offsets).sum(axis=1)
        steps.append({'prior': priors, 'val': vd, 'train': td, 'after': pickle.dumps(models)})
    final = {'train': group.trial_logliks(table, offsets).sum(axis=1), 'prior': [m.log_prior() for m in models]}
    return {'host': table.cpu().numpy(), 'offsets': offsets, 'vhost': vtable.cpu().numpy(), 'voffsets': voffsets,
            'start': start, 'steps': steps, 'final': final}


def _param_errs(a, b):
    return {name: np.abs(getattr(a, name) - getattr(b, name)).max() for name in PARAMS}


@pytest.mark.parametrize('which', range(4))
def test_five_em_iterations_of_a_group_against_the_reference_iteration(em_run, which):
    K, kappa = EM_CONFIGS[which]
    host, offsets, vhost, voffsets = (em_run[k] for k in ('host', 'offsets', 'vhost', 'voffsets'))
    ref1 = pickle.loads(em_run['start'])[which]
    ref2 = pickle.loads(em_run['start'])[which]
    assert (ref1.K, ref1.kappa) == (K, float(kappa))
    frames, vframes = float(offsets[-1] * ref1.D), float(voffsets[-1] * ref1.D)
    tr_dev, priors = [], []
    for it, step in enumerate(em_run['steps']):
        v1 = refs.trial_logliks(ref1, vhost, voffsets).sum()
        v2 = refs.trial_logliks(ref2, vhost, voffsets, second_form=True).sum()
        t1 = refs.em_iteration(ref1, host, offsets).sum()
        t2 = refs.em_iteration(ref2, host, offsets, second_form=True).sum()
        td, vd = step['train'][which], step['val'][which]
        tr_dev.append(td)
        priors.append(step['prior'][which])
        tag = 'K=%d kappa=%d EM %d ' % (K, kappa, it)
        _held(tag + 'tr_loss', abs(td - t1) / frames, abs(t1 - t2) / frames, abs(t1) / frames)
        _held(tag + 'val_loss', abs(vd - v1) / vframes, abs(v1 - v2) / vframes, abs(v1) / vframes)
        dev = pickle.loads(step['after'])[which]
        noise = _param_errs(ref1, ref2)
        for name, err in _param_errs(dev, ref1).items():
            _held(tag + name, err, noise[name], max(np.abs(getattr(ref1, name)).max(), 1.0))
    tr_dev.append(em_run['final']['train'][which])
    priors.append(em_run['final']['prior'][which])
    tr_dev, priors = np.asarray(tr_dev), np.asarray(priors)
    print('training log-likelihood per iteration', tr_dev, 'log prior', priors)
    assert np.all(np.diff(tr_dev + priors) >= -1e-12 * np.abs(tr_dev[:-1]) * 100), (tr_dev, priors)
    assert np.all(np.diff(tr_dev) >= -np.maximum(np.diff(priors), 0.0) - 1e-10 * np.abs(tr_dev[:-1]))
    assert tr_dev[-1] > tr_dev[0]


def test_the_group_s_e_step_is_the_models_own_layout():
    """The five-tuples of ARHMMGroup.e_step have ARHMM.e_step's shapes (the values are held in the tests around this
    one), and trial_logliks is the same forward sweep."""
    train, _ = _em_data()
    table, offsets = ARHMM.as_table(train[:3])
    models = [_em_model(K, kappa) for K, kappa in EM_CONFIGS]
    for m in models:
        m.initialize(table, offsets, seed=1)
    stats = ARHMMGroup(models).e_step(table, offsets)
    assert len(stats) == 4
    for m, st in zip(models, stats):
        own = m.e_step(table, offsets)
        assert [np.shape(v) for v in st] == [np.shape(v) for v in own]
        assert all(np.all(np.isfinite(v)) for v in st)
    lls = ARHMMGroup(models).trial_logliks(table, offsets)
    assert lls.shape == (4, 3) and np.array_equal(lls, np.stack([st[4] for st in stats]))


# ------------------------------------------------------------------------------------------------------------
# fit_arhmm_grid_tables
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


def _fit_data(seed=41, D=3, n_train=6, T=(50, 71)):
    rng = np.random.RandomState(seed)
    lens = list(rng.randint(T[0], T[1], size=n_train + 4))
    datas, _ = refs.sample_arhmm(rng, 3, D, 1, lens, sep=1.5)
    return datas[:n_train], datas[n_train:n_train + 2], datas[n_train + 2:]


def test_fit_arhmm_grid_tables_end_to_end():
    from behavenet_amd.fitting.eval import arhmm_grid, arhmm_grid_groups, fit_arhmm_grid_tables, fit_arhmm_tables
    train, val, test = _fit_data()
    grid = arhmm_grid([2, 3, 4], n_lags=(1, 2), rng_seed_model=1)
    assert len(grid) == 6 and len(arhmm_grid_groups(grid, sum(len(t) for t in train))) == 2
    n_iters = 5
    fits = fit_arhmm_grid_tables(train, val, test, grid=grid, n_iters=n_iters)
    assert len(fits) == 6
    table, t_off = ARHMM.as_table(train)
    host, vhost, thost = np.concatenate(train), np.concatenate(val), np.concatenate(test)
    v_off = np.cumsum([0] + [len(v) for v in val])
    s_off = np.cumsum([0] + [len(v) for v in test])
    D = host.shape[1]
    for cfg, (arhmm, rows) in zip(grid, fits):
        tag = 'K=%d L=%d ' % (cfg['n_states'], cfg['n_lags'])
        _row_layout(rows, n_iters + 1, [0], [(0, 0), (0, 1)])
        assert (arhmm.K, arhmm.lags, arhmm.D) == (cfg['n_states'], cfg['n_lags'], D)
        usage = np.bincount(arhmm.table_states(table, t_off), minlength=arhmm.K)
        assert np.all(np.diff(usage) <= 0), usage            # permuted by usage
        own_model, own = fit_arhmm_tables(train, val, test, n_iters=n_iters, **cfg)
        assert [set(r) for r in own] == [set(r) for r in rows]
        # the float64 iteration from the same start gives the bound per epoch: both routes are within it
        ref1 = ARHMM(cfg['n_states'], D, lags=cfg['n_lags'])
        ref1.initialize(table, t_off, seed=cfg['rng_seed_model'])
        ref2 = pickle.loads(pickle.dumps(ref1))
        frames, vframes = float(len(host) * D), float(len(vhost) * D)
        bounds, test_bound = [], None
        for epoch in range(n_iters + 1):
            if epoch == n_iters:                            # the parameters the test trials are scored with
                s1 = refs.trial_logliks(ref1, thost, s_off)
                s2 = refs.trial_logliks(ref2, thost, s_off, second_form=True)
                per = np.diff(s_off) * float(D)
                test_bound = np.maximum(100 * np.abs(s1 - s2), 1e-12 * np.abs(s1)) / per
                test_ref = -s1 / per
            v1 = refs.trial_logliks(ref1, vhost, v_off).sum()
            v2 = refs.trial_logliks(ref2, vhost, v_off, second_form=True).sum()
            t1 = refs.em_iteration(ref1, host, t_off).sum()
            t2 = refs.em_iteration(ref2, host, t_off, second_form=True).sum()
            bounds.append((max(100 * abs(t1 - t2) / frames, 1e-12 * abs(t1) / frames),
                           max(100 * abs(v1 - v2) / vframes, 1e-12 * abs(v1) / vframes), -t1 / frames, -v1 / vframes))
        worst = 0.0
        for a, b in zip(rows, own):
            assert (a['epoch'], a['dataset'], a['trial']) == (b['epoch'], b['dataset'], b['trial'])
            if 'test_loss' in a:
                i = a['trial']
                assert abs(a['test_loss'] - test_ref[i]) <= test_bound[i], (tag, a, test_ref[i], test_bound[i])
                assert abs(b['test_loss'] - test_ref[i]) <= test_bound[i], (tag, b, test_ref[i], test_bound[i])
                assert abs(a['test_loss'] - b['test_loss']) <= 2 * test_bound[i]
                continue
            bt, bv, t1, v1 = bounds[a['epoch']]
            for key, bound, ref in (('tr_loss', bt, t1), ('val_loss', bv, v1)):
                assert abs(a[key] - ref) <= bound and abs(b[key] - ref) <= bound, (tag, a, b, ref, bound)
                assert abs(a[key] - b[key]) <= 2 * bound, (tag, a, b, bound)
                worst = max(worst, abs(a[key] - b[key]) / (2 * bound))
        print(tag + 'largest |grid - single| / (2 x bound) over the epochs: %.3e' % worst)
        for name, err in _param_errs(arhmm, own_model).items():
            print(tag + '%s: largest difference between the two routes %.3e' % (name, err))


def test_a_model_that_stops_on_tol_is_frozen_and_the_others_go_on():
    from behavenet_amd.fitting.eval import fit_arhmm_grid_tables, fit_arhmm_tables
    train, val, test = _fit_data(seed=43)
    grid = [{'n_states': K, 'n_lags': 1, 'rng_seed_model': 2} for K in (2, 3, 4)]
    n_iters = 13
    free = fit_arhmm_grid_tables(train, val, test, grid=grid, n_iters=n_iters)
    change = []
    for _, rows in free:
        v = {r['epoch']: r['val_loss'] for r in rows if r['dataset'] == 0 and 'val_loss' in r}
        change.append(abs((v[11] - v[10]) / v[11]))
    order = np.argsort(change)
    assert change[order[0]] < change[order[1]]
    tol = float(np.sqrt(change[order[0]] * change[order[1]]))           # between the smallest and the next
    first = int(order[0])
    fits = fit_arhmm_grid_tables(train, val, test, grid=grid, n_iters=n_iters, tol=tol)
    for i, (arhmm, rows) in enumerate(fits):
        last = max(r['epoch'] for r in rows)
        if i == first:
            _row_layout(rows, 12, [0], [(0, 0), (0, 1)])    # epochs 0 .. 11, the test rows at epoch 11
            own_model, own = fit_arhmm_tables(train, val, test, n_iters=n_iters, tol=tol, **grid[i])
            assert [(r['epoch'], r['dataset'], r['trial']) for r in own] == \
                [(r['epoch'], r['dataset'], r['trial']) for r in rows]
            for name, err in _param_errs(arhmm, own_model).items():
                print('stopped model, %s: largest difference from fit_arhmm_tables %.3e' % (name, err))
        else:
            assert last >= 12
            _row_layout(rows, last + 1, [0], [(0, 0), (0, 1)])
        # up to its last epoch a model's rows are those of the run without tol, bit for bit: leaving or staying in
        # the launches changes nobody's numbers
        n_same = 2 * (last + 1)
        assert rows[:n_same] == free[i][1][:n_same]
