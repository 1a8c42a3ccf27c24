"""The ARHMM sampling launch (bn_arhmm_sample, csrc/arhmm.hip), the model's sample methods and the real-vs-sampled
movie against the float64 restatements of tests/arhmm_sample_refs.py.

Tolerances, the convention of tests/test_gpu_arhmm.py: everything is float64, the two INDEPENDENT restatements (A: the
plain loop; B: the drive for all rows at once, then the recursion in companion form) give the noise floor at the shape,
the device's bound is 100 x their disagreement and never less than 1e-12 of the element's scale (the same recursion on
absolute values).  The bound comes from the restatements alone; every check prints error, bound and their ratio.  State
paths are compared exactly, the movie byte for byte.

Largest error / bound seen on an MI355X (first run of this file): x below 0.001 in every case of test_sample, in
sample_table and in sample_conditional -- the 1e-12-of-scale floor is the bound there (errors 0.9 to 2.7e-15, noise
floors 0.9 to 3.6e-15, scales of a few units); against 100 x the noise floor alone the largest error is 0.021.  State
paths equal, movies equal byte for byte; sampled usage 0.348 / 0.333 / 0.320 against 1/3 with standard errors 0.007.
"""

import numpy as np
import pytest
import torch

from behavenet_amd import _hip
from behavenet_amd.fitting.eval import (decode_points_device, real_vs_sampled_movie, real_vs_sampled_movie_device)
from behavenet_amd.models.arhmm import ARHMM
from tests import arhmm_refs as refs
from tests import arhmm_sample_refs as sr
from tests.test_gpu_traversals import _case_of

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


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _in_trial(offsets, n):
    mask = np.zeros(n, dtype=bool)
    mask[offsets[0]:offsets[-1]] = True
    return mask


def _run(gen, offsets, eps_d, n, D, **kw):
    """One launch into sentinel-filled outputs -> host (x, states)."""
    x0 = torch.full((n, D), -7.0, dtype=torch.float64, device=DEV)
    s0 = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    x, z = _hip.arhmm_sample(*gen, offsets, eps_d, x=x0, states_out=s0, **kw)
    assert x is x0 and z is s0
    return x.cpu().numpy(), z.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------
# bn_arhmm_sample
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', sr.STATES)
@pytest.mark.parametrize('D,L', sr.SHAPES)
def test_sample(D, L, K):
    m = sr.shape_model(D, L, K)
    gen = m.generative()
    assert sr.spectral_radii(gen[0]).max() < 0.99
    offsets, n, eps, u, init = sr.shape_noise(D, L, K)
    given = np.random.RandomState(D + L + K).randint(0, K, size=n).astype(np.int32)
    eps_d, u_d, given_d, wide = _dev(eps), _dev(u), _dev(given), _dev(init)
    inside = _in_trial(offsets, n)
    for mode, host_kw, dev_kw in (('sampled', {'u': u}, {'u': u_d}), ('given', {'states': given}, {'states': given_d})):
        for ini, init_h, init_d in (('none', None, None), ('strided', init[:, :D], wide[:, :D]),
                                    ('contiguous', init[:, :D], wide[:, :D].contiguous())):
            xa, za = sr.sample_a(*gen, offsets, eps, init=init_h, fill=-7.0, state_fill=-7, **host_kw)
            xb, zb = sr.sample_b(*gen, offsets, eps, init=init_h, fill=-7.0, state_fill=-7, **host_kw)
            scale = sr.sample_scale(gen[0], gen[1], offsets, eps, za, init=init_h)
            x, z = _run(gen, offsets, eps_d, n, D, init=init_d, **dev_kw)
            assert np.array_equal(za, zb) and np.array_equal(z, za)            # (the sentinel rows included)
            assert np.all(x[~inside] == -7.0)
            if K == 1:
                assert not z[inside].any()
            if mode == 'given':
                assert np.array_equal(z[inside], given[inside])
            for beg, end in refs.trials_of(offsets):                           # initial rows: init widened, or eps
                head = slice(beg, min(beg + L, end))
                assert np.array_equal(x[head], eps[head] if init_h is None else init_h[head].astype(np.float64))
            noise = np.abs(xa - xb)[inside].max()
            _held('x D=%d L=%d K=%d %s init=%s' % (D, L, K, mode, ini), np.abs(x - xa)[inside], noise, scale[inside])
            x2, z2 = _run(gen, offsets, eps_d, n, D, init=init_d, **dev_kw)
            assert np.array_equal(x2, x) and np.array_equal(z2, z)             # the same bits on a second call


def test_one_state_whatever_u_is():
    m = sr.shape_model(3, 1, 1)
    gen = m.generative()
    offsets, n, eps, u, _ = sr.shape_noise(3, 1, 1)
    u[::3], u[1::3] = 0.0, np.nextafter(1.0, 0.0)
    x, z = _run(gen, offsets, _dev(eps), n, 3, u=_dev(u))
    inside = _in_trial(offsets, n)
    assert not z[inside].any() and np.all(z[~inside] == -7)
    assert np.array_equal(z, sr.sample_a(*gen, offsets, eps, u=u, state_fill=-7)[1])


@pytest.mark.parametrize('K', [2, 5, 32])
def test_u_on_a_cdf_entry_and_at_zero_follow_the_counting_rule(K):
    D, L = 3, 1
    m = sr.shape_model(D, L, K)
    gen = m.generative()
    cdf0, cdf = gen[2], gen[3]
    offsets, n, eps, u, _ = sr.shape_noise(D, L, K)
    want = np.full(n, -7, dtype=np.int32)
    count = 0
    for beg, end in refs.trials_of(offsets):
        z = 0
        for t in range(beg, end):
            row = cdf0 if t == beg else cdf[z]
            if t % 4 == 3:
                u[t], z = 0.0, 0
            else:
                j = count % K
                count += 1
                if j < K - 1:
                    u[t], z = row[j], j + 1                # u >= row[j] counts: exactly on the entry is the next state
                else:
                    u[t], z = np.nextafter(row[K - 2], 0.0), K - 2             # just below the last compared entry
            want[t] = z
    assert np.array_equal(sr.sample_states(cdf0, cdf, offsets, u, n, state_fill=-7), want)
    x, z = _run(gen, offsets, _dev(eps), n, D, u=_dev(u))
    assert np.array_equal(z, want)
    assert len(np.unique(want[_in_trial(offsets, n)])) == K


@pytest.mark.parametrize('D,L', [(3, 1), (12, 4)])
def test_a_nan_stays_inside_its_trial(D, L):
    K = 5
    m = sr.shape_model(D, L, K)
    gen = m.generative()
    offsets, n, eps, u, init = sr.shape_noise(D, L, K)
    init = np.ascontiguousarray(init[:, :D])
    u_d = _dev(u)
    clean, zc = _run(gen, offsets, _dev(eps), n, D, u=u_d, init=_dev(init))
    assert np.all(np.isfinite(clean[_in_trial(offsets, n)]))
    t37, t150 = (int(offsets[3]), int(offsets[4])), (int(offsets[4]), int(offsets[5]))
    bad_init, bad_eps = t37[0], t150[0] + 70               # an initial row of one trial, an AR row of the next
    init2, eps2 = init.copy(), eps.copy()
    init2[bad_init, D - 1] = np.nan
    eps2[bad_eps, 0] = np.nan
    x, z = _run(gen, offsets, _dev(eps2), n, D, u=u_d, init=_dev(init2))
    assert np.array_equal(z, zc)
    touched = np.zeros(n, dtype=bool)
    touched[t37[0]:t37[1]] = True
    touched[t150[0]:t150[1]] = True
    assert np.array_equal(x[~touched], clean[~touched])                        # the other trials: the same bits
    assert np.array_equal(x[t150[0]:bad_eps], clean[t150[0]:bad_eps])          # and the rows before the NaN
    assert np.isnan(x[bad_eps:t150[1]]).all()              # every column of C and of A is multiplied
    assert np.isnan(x[bad_init, D - 1]) and np.array_equal(x[bad_init, :D - 1], clean[bad_init, :D - 1])
    assert np.isnan(x[t37[0] + L:t37[1]]).all()


def test_the_wrapper_refuses_states_outside_the_model_before_any_launch():
    D, L, K = 3, 1, 5
    m = sr.shape_model(D, L, K)
    gen = m.generative()
    offsets, n, eps, u, _ = sr.shape_noise(D, L, K)
    eps_d = _dev(eps)
    good = np.random.RandomState(0).randint(0, K, size=n).astype(np.int32)
    for bad in (-1, K):
        states = good.copy()
        states[int(offsets[4]) + 5] = bad
        x0 = torch.full((n, D), -7.0, dtype=torch.float64, device=DEV)
        s0 = torch.full((n,), -7, dtype=torch.int32, device=DEV)
        with pytest.raises(ValueError, match='the model has the states 0 to 4'):
            _hip.arhmm_sample(*gen, offsets, eps_d, states=_dev(states), x=x0, states_out=s0)
        torch.cuda.synchronize()
        assert bool((x0 == -7.0).all()) and bool((s0 == -7).all())             # nothing was launched
    states = good.copy()
    states[0], states[n - 1] = -1, K                       # rows of no trial are not read
    x, z = _run(gen, offsets, eps_d, n, D, states=_dev(states))
    assert np.array_equal(x, _run(gen, offsets, eps_d, n, D, states=_dev(good))[0])
    with pytest.raises(ValueError, match='exactly one of u'):
        _hip.arhmm_sample(*gen, offsets, eps_d)
    with pytest.raises(ValueError, match='exactly one of u'):
        _hip.arhmm_sample(*gen, offsets, eps_d, u=_dev(u), states=_dev(good))


# ------------------------------------------------------------------------------------------------------------
# ARHMM.sample, sample_table, sample_conditional
# ------------------------------------------------------------------------------------------------------------
def _separated(K=3, D=2, L=1, seed=11, sep=3.0):
    """The parameters of ``refs.sample_arhmm`` (well-separated states, sticky rows) as a model."""
    rng = np.random.RandomState(seed)
    m = ARHMM(K, D, lags=L)
    for k in range(K):
        m.As[k] = np.concatenate([0.5 / L * np.eye(D) + 0.05 * rng.randn(D, D) for _ in range(L)], axis=1)
        m.bs[k] = sep * rng.randn(D)
        m.Sigmas[k] = 0.09 * np.eye(D)
    Ps = np.full((K, K), 0.05 / (K - 1)) + (0.95 - 0.05 / (K - 1)) * np.eye(K)
    m.log_Ps = np.log(Ps / Ps.sum(axis=1, keepdims=True))
    return m


def _noise_of(seed, n, D, with_u=True):
    """The draws of ``ARHMM.sample_table``: eps first, then u, float64, one device generator."""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    eps = torch.randn((n, D), dtype=torch.float64, device=DEV, generator=g)
    u = torch.rand((n,), dtype=torch.float64, device=DEV, generator=g) if with_u else None
    return eps.cpu().numpy(), None if u is None else u.cpu().numpy()


def test_sample_shapes_and_the_tail_of_sample_table():
    m = sr.shape_model(3, 1, 5)
    states, latents = m.sample(20, n_samples=3, burn_in=5, seed=3)
    assert len(states) == 3 and len(latents) == 3
    assert all(s.shape == (20,) and s.dtype == np.int32 for s in states)
    assert all(x.shape == (20, 3) and x.dtype == np.float64 for x in latents)
    offsets = np.arange(4, dtype=np.int64) * 25
    x, z = m.sample_table(offsets, seed=3)
    assert x.is_cuda and x.dtype == torch.float64 and z.dtype == torch.int32
    x, z = x.cpu().numpy(), z.cpu().numpy()
    for i in range(3):
        assert np.array_equal(states[i], z[25 * i + 5:25 * (i + 1)])
        assert np.array_equal(latents[i], x[25 * i + 5:25 * (i + 1)])
    # the launch on the generator's draws is the restatement's
    eps, u = _noise_of(3, 75, 3)
    gen = m.generative()
    xa, za = sr.sample_a(*gen, offsets, eps, u=u)
    xb, _ = sr.sample_b(*gen, offsets, eps, u=u)
    assert np.array_equal(z, za)
    _held('sample_table', np.abs(x - xa), np.abs(xa - xb).max(), sr.sample_scale(gen[0], gen[1], offsets, eps, za))
    other = m.sample(20, n_samples=3, burn_in=5, seed=4)[1]
    assert not np.array_equal(other[0], latents[0])
    assert m.sample(20, n_samples=1)[1][0].shape == (20, 3)                   # the default burn-in of 200 rows


def test_sampled_state_usage_is_the_stationary_distribution():
    m = _separated()
    T, n_samples, burn = 500, 200, 200
    states, latents = m.sample(T, n_samples=n_samples, burn_in=burn, seed=5)
    per = T + burn
    offsets = np.arange(n_samples + 1, dtype=np.int64) * per
    gen = m.generative()
    _, u = _noise_of(5, n_samples * per, m.D)
    chain = sr.sample_states(gen[2], gen[3], offsets, u, n_samples * per).reshape(n_samples, per)[:, burn:]
    assert np.array_equal(np.stack(states), chain)         # the device's path is the host's, bit for bit
    per_trial = np.stack([(chain == k).mean(axis=1) for k in range(m.K)], axis=1)             # (trials, K)
    se = per_trial.std(axis=0, ddof=1) / np.sqrt(n_samples)
    freq = np.bincount(np.concatenate(states), minlength=m.K) / float(n_samples * T)
    pi = sr.stationary(np.exp(m.log_Ps))
    np.testing.assert_allclose(pi @ np.exp(m.log_Ps), pi, atol=1e-12)
    print('usage %s, stationary %s, standard errors %s' % (freq, pi, se))
    assert np.all(se > 0) and np.all(np.abs(freq - pi) <= 5.0 * se)
    # well-separated states: the latents sit near their state's fixed point
    for k in range(m.K):
        rows = np.concatenate(latents)[np.concatenate(states) == k]
        fixed = np.linalg.solve(np.eye(m.D) - m.As[k], m.bs[k])
        assert np.linalg.norm(np.median(rows, axis=0) - fixed) < 0.25 * np.linalg.norm(fixed) + 0.5


@pytest.mark.parametrize('L', [1, 2])
def test_sample_conditional(L):
    K, D = 3, 2
    m = _separated(K, D, L)
    datas, _ = refs.sample_arhmm(np.random.RandomState(2), K, D, L, [40, 0, 25, 60])
    table, offsets = ARHMM.as_table(datas)
    path = m.table_states(table, offsets)
    states, latents = m.sample_conditional(datas, seed=9)
    assert len(states) == 4 and len(latents) == 4
    for i, (s, x) in enumerate(zip(states, latents)):
        assert np.array_equal(s, path[offsets[i]:offsets[i + 1]])
        assert x.shape == datas[i].shape and x.dtype == np.float64
        assert np.array_equal(x[:L], datas[i][:L].astype(np.float64))          # the real trial's first rows
    eps, _ = _noise_of(9, int(offsets[-1]), D, with_u=False)
    gen = m.generative()
    host = table.cpu().numpy()
    xa, _ = sr.sample_a(*gen, offsets, eps, states=path, init=host)
    xb, _ = sr.sample_b(*gen, offsets, eps, states=path, init=host)
    _held('sample_conditional L=%d' % L, np.abs(np.concatenate(latents) - xa), np.abs(xa - xb).max(),
          sr.sample_scale(gen[0], gen[1], offsets, eps, path, init=host))


# ------------------------------------------------------------------------------------------------------------
# the real-vs-sampled movie
# ------------------------------------------------------------------------------------------------------------
def _movie_by_hand(case, real, sampled, max_frames, n_buffer, chunk_size):
    """The numpy mosaic of ONE ``decode_points_device`` call on the rows of the trials the movie uses."""
    cols, tables, rows = [], [], 0
    for trials in (real, sampled):
        src, used = [], 0
        while len(src) < max_frames:
            src += list(range(rows, rows + len(trials[used]))) + [-1] * n_buffer
            rows += len(trials[used])
            tables.append(trials[used])
            used += 1
        cols.append(src)
    table = np.concatenate(tables).astype(np.float32)
    frames = decode_points_device(case.model, table, None, True, chunk_size)
    assert frames.dtype == torch.float32
    q = _hip.unit_float_to_u8(frames.contiguous()).cpu().numpy()
    C, H, W = q.shape[1:]
    T = min(len(cols[0]), len(cols[1]))
    movie = np.zeros((T, C * H, 2 * W), dtype=np.uint8)
    for t in range(T):
        for side in range(2):
            if cols[side][t] >= 0:
                for c in range(C):
                    movie[t, c * H:(c + 1) * H, side * W:(side + 1) * W] = q[cols[side][t], c]
    return movie, cols


def test_movie_is_the_mosaic_of_one_decode():
    case = _case_of('ae_cfg1')
    assert case.dim == (1, 32, 32)
    rng = np.random.RandomState(4)
    real = [rng.randn(7, case.n_lat).astype(np.float32), rng.randn(9, case.n_lat).astype(np.float32)]
    sampled = [rng.randn(7, case.n_lat), rng.randn(9, case.n_lat)]             # float64, as ARHMM.sample returns them
    want, cols = _movie_by_hand(case, real, sampled, 12, 2, 200)
    movie = real_vs_sampled_movie(case.model, real, sampled, max_frames=12, n_buffer=2)
    dev = real_vs_sampled_movie_device(case.model, real, sampled, max_frames=12, n_buffer=2)
    assert movie.dtype == np.uint8 and movie.shape == (20, 32, 64)             # 7 + 2 < 12 <= 7 + 2 + 9 + 2
    assert dev.is_cuda and dev.dtype == torch.uint8 and np.array_equal(dev.cpu().numpy(), movie)
    assert np.array_equal(movie, want)
    assert len(np.unique(movie)) > 8, 'the movie draws an almost constant grey'
    for blank in (7, 8, 18, 19):                           # the buffer frames, after the last trial too
        assert not movie[blank].any()
    assert movie[6].any() and movie[9].any()
    assert not np.array_equal(movie[:, :, :32], movie[:, :, 32:])
    # one launch per chunk of movie frames: the same bytes (1x32x32 decodes do not depend on the batch)
    assert np.array_equal(real_vs_sampled_movie(case.model, real, sampled, 12, 2, chunk_size=7), want)
    # T is the smaller of the two columns' counts: one sampled trial of 13 frames gives 15
    longer = [rng.randn(13, case.n_lat)]
    want15, _ = _movie_by_hand(case, real, longer, 12, 2, 200)
    got15 = real_vs_sampled_movie(case.model, real, longer, max_frames=12, n_buffer=2)
    assert got15.shape == (15, 32, 64) and np.array_equal(got15, want15)
    with pytest.raises(ValueError, match='2 trials give 20 frames, max_frames is 30'):
        real_vs_sampled_movie(case.model, real, sampled, max_frames=30, n_buffer=2)
    with pytest.raises(ValueError, match='1 trials give 15 frames, max_frames is 16'):
        real_vs_sampled_movie(case.model, real + real, longer, max_frames=16, n_buffer=2)


def test_movie_stacks_the_channels_vertically():
    case = _case_of('psvae_cfg4')
    assert case.dim[0] == 2
    H, W = case.dim[1:]
    rng = np.random.RandomState(6)
    real = [rng.randn(3, case.n_lat).astype(np.float32)]
    sampled = [rng.randn(3, case.n_lat)]
    want, _ = _movie_by_hand(case, real, sampled, 4, 1, 200)
    movie = real_vs_sampled_movie(case.model, real, sampled, max_frames=4, n_buffer=1)
    assert movie.shape == (4, 2 * H, 2 * W) and np.array_equal(movie, want)
    assert not movie[3].any() and movie[2, :H].any() and movie[2, H:].any()
    assert not np.array_equal(movie[:3, :H], movie[:3, H:])                    # two views, one above the other


# ------------------------------------------------------------------------------------------------------------
# fitting.eval.sample_arhmm on a generator
# ------------------------------------------------------------------------------------------------------------
def test_sample_arhmm_on_the_synthetic_generator(tmp_path):
    from behavenet_amd.fitting.eval import fit_arhmm, sample_arhmm
    from tests.test_gpu_ranges import LENS, _generator, _model as _ae
    model, meta = _ae('ae_cfg1', str(tmp_path))
    gen = _generator(meta, n_sessions=2, n_labels=3)
    arhmm, _ = fit_arhmm(gen, model, n_states=2, n_lags=1, n_iters=2, rng_seed_model=1)
    D = int(model.hparams['n_ae_latents'])
    out = sample_arhmm(gen, model, arhmm, n_samples=3, conditional=True, dtype='test', sess_idx=1, seed=1)
    assert set(out) == {'latents', 'states', 'trial_idxs', 'latents_gen', 'states_gen'}
    ds = gen.datasets[1]
    for dt in ('train', 'val', 'test'):
        trials = [int(t) for t in ds.batch_idxs[dt]]
        assert np.array_equal(out['trial_idxs'][dt], trials)
        assert [x.shape for x in out['latents'][dt]] == [(LENS[t], D) for t in trials]
        assert [z.shape for z in out['states'][dt]] == [(LENS[t],) for t in trials]
        assert all(x.dtype == np.float32 for x in out['latents'][dt])
    first = out['latents']['test'][0]
    assert np.array_equal(out['states']['test'][0], arhmm.most_likely_states(first))
    # conditional: one sampled trial a test trial, along its Viterbi path, from the real first row; no sampled states
    assert out['states_gen'] == [] and len(out['latents_gen']) == len(out['latents']['test'])
    states, latents = arhmm.sample_conditional(out['latents']['test'], seed=1)
    for x, real, mine, z, path in zip(out['latents_gen'], out['latents']['test'], latents, states,
                                      out['states']['test']):
        assert x.shape == real.shape and np.array_equal(x[:1], real[:1].astype(np.float64))
        assert np.array_equal(x, mine) and np.array_equal(z, path) and np.all(np.isfinite(x))
    # unconditional: n_samples trials as long as the first test trial, with their states
    free = sample_arhmm(gen, model, arhmm, n_samples=3, conditional=False, dtype='test', sess_idx=1, seed=1)
    assert [x.shape for x in free['latents_gen']] == [first.shape] * 3
    assert [z.shape for z in free['states_gen']] == [(len(first),)] * 3
    want = arhmm.sample(len(first), n_samples=3, burn_in=200, seed=1)
    assert all(np.array_equal(a, b) for a, b in zip(free['latents_gen'], want[1]))
    assert all(np.array_equal(a, b) for a, b in zip(free['states_gen'], want[0]))
    both = sample_arhmm(gen, model, arhmm, n_samples=0, dtype='val')
    assert both['latents_gen'] == [] and both['states_gen'] == []
    assert both['trial_idxs']['val'][0] == (0, int(gen.datasets[0].batch_idxs['val'][0]))        # two sessions: pairs
    movie = real_vs_sampled_movie(model, out['latents']['test'], out['latents_gen'], max_frames=10, n_buffer=1)
    assert movie.dtype == np.uint8 and movie.shape[1:] == (32, 64) and movie.shape[0] >= 10
    with pytest.raises(ValueError, match="dtype must be"):
        sample_arhmm(gen, model, arhmm, dtype='all')
