"""The host side of a grid of ARHMMs fitted at once (fitting.eval.arhmm_grid, arhmm_grid_groups, fit_arhmm_grid_tables;
models.arhmm.ARHMMGroup; _hip.hmm_grid_plan and the limits of the grid launches).  No GPU."""

import itertools
import pickle

import numpy as np
import pytest
import torch

from behavenet_amd import _hip
from behavenet_amd.fitting.eval import ARHMM_GRID_TABLE_BYTES, arhmm_grid, arhmm_grid_groups, fit_arhmm_grid_tables
from behavenet_amd.models.arhmm import ARHMM, ARHMMGroup


def test_arhmm_grid_is_the_product_in_order_without_what_the_reference_refuses():
    grid = arhmm_grid([2, 4], n_lags=(1, 2), transitions=('stationary', 'sticky'), kappa=(0, 100), rng_seed_model=(0, 1))
    full = list(itertools.product([2, 4], (1, 2), ('stationary', 'sticky'), (0, 100), (0, 1)))
    kept = [c for c in full if (c[2] == 'sticky') == (c[3] > 0)]
    assert len(full) == 32 and len(kept) == 16
    assert [(g['n_states'], g['n_lags'], g['transitions'], g['kappa'], g['rng_seed_model']) for g in grid] == kept
    assert all(set(g) == {'n_states', 'n_lags', 'transitions', 'kappa', 'rng_seed_model'} for g in grid)
    # sticky with kappa == 0 and anything else with kappa > 0 are left out
    assert arhmm_grid(3, transitions='sticky') == []
    assert arhmm_grid(3, kappa=5) == []
    assert arhmm_grid(3, transitions='recurrent', kappa=(0, 1)) == [
        {'n_states': 3, 'n_lags': 1, 'transitions': 'recurrent', 'kappa': 0, 'rng_seed_model': 0}]
    assert arhmm_grid(3) == [{'n_states': 3, 'n_lags': 1, 'transitions': 'stationary', 'kappa': 0,
                              'rng_seed_model': 0}]


def test_plan_classes():
    cls, wave, slot = _hip.hmm_grid_plan([4, 5, 8, 9, 16, 17, 32])
    assert cls.tolist() == [4, 8, 8, 16, 16, 32, 32]
    assert _hip.hmm_grid_plan([1, 2, 3])[0].tolist() == [4, 4, 4]
    with pytest.raises(ValueError):
        _hip.hmm_grid_plan([33])
    with pytest.raises(ValueError):
        _hip.hmm_grid_plan([0])


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_plan_puts_every_model_into_exactly_one_slot(seed):
    rng = np.random.RandomState(seed)
    Ks = rng.randint(1, 33, size=[1, 40, 200][seed]).tolist() + [3] * (17 * seed)
    cls, wave, slot = _hip.hmm_grid_plan(Ks)
    assert len(set(zip(cls.tolist(), wave.tolist(), slot.tolist()))) == len(Ks)          # no slot twice
    for m, K in enumerate(Ks):
        assert cls[m] in (4, 8, 16, 32) and cls[m] >= K and (cls[m] == 4 or cls[m] // 2 < K)
        assert 0 <= slot[m] < 64 // cls[m] and wave[m] >= 0
    for c in (4, 8, 16, 32):
        members = np.flatnonzero(cls == c)
        # the slots of a class are filled in the models' order with no gap: a wave holds one class only
        assert (wave[members] * (64 // c) + slot[members]).tolist() == list(range(len(members)))
    # the launcher's order is the plan's
    order, counts = _hip._hmm_grid_order(Ks)
    assert sorted(order.tolist()) == list(range(len(Ks))) and sum(counts) == len(Ks)
    pos = 0
    for c, cnt in zip((4, 8, 16, 32), counts):
        for p, m in enumerate(order[pos:pos + cnt]):
            assert (cls[m], wave[m], slot[m]) == (c, p // (64 // c), p % (64 // c))
        pos += cnt


def test_grouping_rule():
    cfg = lambda K, L=1: {'n_states': K, 'n_lags': L}
    # lags: one n_lags a group, the grid's order inside a group
    grid = [cfg(2, 1), cfg(3, 2), cfg(4, 1), cfg(5, 2), cfg(6, 0)]
    assert arhmm_grid_groups(grid, 1000) == [[0, 2], [1, 3], [4]]
    # the cap of 512 states: 16 models of 32 states fill a group
    grid = [cfg(32)] * 17 + [cfg(1)]
    assert arhmm_grid_groups(grid, 1000) == [list(range(16)), [16, 17]]
    assert _hip.ARHMM_GRID_MAX_STATES == 512
    # the byte budget: ll and gamma are 16 bytes a (row, state)
    assert ARHMM_GRID_TABLE_BYTES == 8 << 30
    rows = 10 ** 7
    fit = ARHMM_GRID_TABLE_BYTES // (16 * rows)             # 53 states
    assert fit == 53
    grid = [cfg(32), cfg(21), cfg(1), cfg(32)]
    assert arhmm_grid_groups(grid, rows) == [[0, 1], [2, 3]]
    assert arhmm_grid_groups(grid, rows, max_bytes=16 * rows * 54) == [[0, 1, 2], [3]]
    # a configuration beyond the budget alone is a group of its own
    assert arhmm_grid_groups([cfg(32), cfg(32)], 10 ** 9) == [[0], [1]]
    # the bench's grid: 60 models, 744 states, two groups
    grid = arhmm_grid([2, 4, 8, 16, 32], transitions='sticky', kappa=(1, 10, 100, 1000), rng_seed_model=(0, 1, 2))
    groups = arhmm_grid_groups(grid, 10 ** 6)
    assert len(grid) == 60 and sum(g['n_states'] for g in grid) == 744 and len(groups) == 2
    assert sorted(i for g in groups for i in g) == list(range(60))
    assert all(sum(grid[i]['n_states'] for i in g) <= 512 for g in groups)


def test_limits_are_checked_before_a_launch():
    with pytest.raises(ValueError, match='513 states in all models together'):
        ARHMMGroup([ARHMM(32, 2) for _ in range(16)] + [ARHMM(1, 2)])
    assert ARHMMGroup([ARHMM(32, 2) for _ in range(16)]).KT == 512
    with pytest.raises(ValueError, match='share D and lags'):
        ARHMMGroup([ARHMM(2, 2), ARHMM(2, 3)])
    with pytest.raises(ValueError, match='share D and lags'):
        ARHMMGroup([ARHMM(2, 2, lags=1), ARHMM(2, 2, lags=2)])
    with pytest.raises(ValueError, match='no models'):
        ARHMMGroup([])
    with pytest.raises(ValueError, match='33 states'):       # a single model keeps its limit
        ARHMM(33, 2)
    table = torch.zeros((10, 3))
    with pytest.raises(ValueError, match='513 states in all models together'):
        _hip.check_arhmm_grid_dims('arhmm_grid_loglik', 3, 1, 513)
    _hip.check_arhmm_grid_dims('arhmm_grid_loglik', 3, 1, 512)
    with pytest.raises(ValueError, match='9 lags'):
        _hip.check_arhmm_grid_dims('arhmm_grid_loglik', 3, 9, 40)
    with pytest.raises(ValueError, match='no CPU fallback'):
        _hip.arhmm_grid_loglik(table, [0, 10], np.zeros((40, 3, 7)), np.zeros(40), 1)
    with pytest.raises(ValueError, match='no CPU fallback'):
        _hip.arhmm_grid_moments(table, [0, 10], torch.zeros((10, 40), dtype=torch.float64), 1)
    ll = torch.zeros((10, 40), dtype=torch.float64)
    Ks = [8] * 5
    with pytest.raises(ValueError, match='no CPU fallback'):
        _hip.hmm_grid_forward_backward(ll, [0, 10], Ks, np.zeros(5 * 64), np.zeros(40))
    with pytest.raises(ValueError, match='float64'):
        _hip.hmm_grid_forward_backward(ll.float(), [0, 10], Ks, np.zeros(5 * 64), np.zeros(40))
    with pytest.raises(ValueError, match=r'\(n, 41\)'):
        _hip.hmm_grid_forward_backward(ll, [0, 10], Ks + [1], np.zeros(5 * 64 + 1), np.zeros(41))
    with pytest.raises(ValueError, match='33 states'):
        _hip.hmm_grid_forward_backward(ll, [0, 10], [33, 7], np.zeros(33 * 33 + 49), np.zeros(40))
    with pytest.raises(ValueError, match='513 states'):
        _hip.hmm_grid_forward_backward(torch.zeros((4, 513), dtype=torch.float64), [0, 4], [27] * 19,
                                       np.zeros(19 * 27 * 27), np.zeros(513))


def test_an_unserved_type_inside_a_grid_is_refused_before_the_first_epoch():
    train = [np.zeros((20, 2), dtype=np.float32)]
    ok = {'n_states': 2}
    with pytest.raises(NotImplementedError, match='recurrent'):
        fit_arhmm_grid_tables(train, grid=[ok, {'n_states': 2, 'transitions': 'recurrent'}], n_iters=1)
    with pytest.raises(NotImplementedError, match="noise_type 'studentst'"):
        fit_arhmm_grid_tables(train, grid=[ok, {'n_states': 2, 'noise_type': 'studentst'}], n_iters=1)
    with pytest.raises(ValueError, match='33 states'):
        fit_arhmm_grid_tables(train, grid=[ok, {'n_states': 33}], n_iters=1)
    with pytest.raises(ValueError, match='9 lags'):
        fit_arhmm_grid_tables(train, grid=[ok, {'n_states': 2, 'n_lags': 9}], n_iters=1)
    with pytest.raises(ValueError, match='a configuration is a dict'):
        fit_arhmm_grid_tables(train, grid=[{'n_lags': 1}], n_iters=1)
    with pytest.raises(ValueError, match='a configuration is a dict'):
        fit_arhmm_grid_tables(train, grid=[{'n_states': 2, 'n_iters': 3}], n_iters=1)


def test_the_group_pickles_and_holds_models_and_numpy_only():
    rng = np.random.RandomState(0)
    models = [ARHMM(K, 3, lags=2, transitions='sticky', kappa=10.0) for K in (2, 5, 32)]
    for m in models:
        m.bs = rng.randn(m.K, 3)
    g = ARHMMGroup(models)
    assert (g.M, g.KT, g.P, g.D, g.lags) == (3, 39, 10, 3, 2)
    assert g.koff.tolist() == [0, 2, 7, 39] and g.xoff.tolist() == [0, 4, 29, 29 + 1024]
    for name, v in vars(g).items():
        assert isinstance(v, (int, np.ndarray)) or name == 'models', (name, type(v))
    assert all(m is n for m, n in zip(g.models, models))     # references, not copies
    g2 = pickle.loads(pickle.dumps(g))
    assert g2.Ks.tolist() == [2, 5, 32] and g2.koff.tolist() == g.koff.tolist()
    for a, b in zip(g.models, g2.models):
        assert np.array_equal(a.bs, b.bs) and (a.K, a.kappa) == (b.K, b.kappa)
    # fold(): the models' folds one after the other
    G, cst = g.fold()
    assert G.shape == (39, 3, 10) and cst.shape == (39,)
    assert np.array_equal(G[2:7], models[1].fold()[0]) and np.array_equal(cst[7:], models[2].fold()[1])
    # one shift for the group
    models[1].shift = np.ones(3)
    with pytest.raises(ValueError, match='share the shift'):
        g._shift()


@pytest.mark.parametrize('n,D,L,KT', [(0, 4, 1, 33), (2100, 32, 1, 512), (100000, 32, 1, 512), (4000, 16, 1, 372),
                                      (10 ** 6, 16, 1, 372), (3000, 7, 8, 77), (513, 3, 1, 33)])
def test_the_restated_plan_is_the_library_s_above_32_states(n, D, L, KT):
    lib = _hip.load()
    S, M = 7, 20
    blocks, rows = _hip._arhmm_moments_plan(n, D, L, KT)
    P = 1 + (L + 1) * D
    pad16 = lambda b: (b + 15) // 16 * 16
    assert blocks * KT * P * P * 8 <= 60 << 20
    assert blocks == 0 or (blocks - 1) * rows < n <= blocks * rows
    assert lib.bn_arhmm_grid_moments_ws_bytes(n, S, D, L, KT) == pad16((S + 1) * 4) + pad16(n) + blocks * KT * P * P * 8
    assert lib.bn_arhmm_grid_loglik_ws_bytes(n, S, D, L, KT) == pad16((S + 1) * 4) + pad16(n)
    assert lib.bn_hmm_grid_forward_backward_ws_bytes(n, S, M, KT, KT * 8) == pad16((S + 1) * 4) + 16 * n * M
    if KT > 32:                                              # the single-model entry points keep their limit
        assert lib.bn_arhmm_moments_ws_bytes(n, S, D, L, KT) == 0 and lib.bn_arhmm_loglik_ws_bytes(n, S, D, L, KT) == 0


def test_the_row_blocks_grow_at_512_states():
    """P = 65: one set of 512 partials is 17.3 MB, three fit into 60 MiB, so 2,100 rows are cut into three blocks of
    700 and not into five of at least 512."""
    assert _hip._arhmm_moments_plan(2100, 32, 1, 512) == (3, 700)
    assert _hip._arhmm_moments_plan(2100, 32, 1, 32) == (5, 420)


def test_the_grid_queries_refuse_what_the_calls_refuse():
    lib = _hip.load()
    for args in ((10, 1, 4, 1, 513), (10, 1, 4, 1, 0), (10, 1, 4, 9, 40), (10, 1, 33, 1, 40), (-1, 1, 4, 1, 40)):
        assert lib.bn_arhmm_grid_loglik_ws_bytes(*args) == 0 and lib.bn_arhmm_grid_moments_ws_bytes(*args) == 0
        assert lib.bn_arhmm_grid_loglik(None, 4, None, None, *args[1:], args[0], None, None, None, None, 0, None) == -2
        assert lib.bn_arhmm_grid_moments(None, 4, None, None, *args[1:], args[0], None, None, None, None, 0,
                                         None) == -2
    # (n, S, M, KT, XT): no models, more models than states, 513 states, XT outside [KT, 32 KT]
    for args in ((10, 1, 0, 40, 100), (10, 1, 41, 40, 100), (10, 1, 20, 513, 600), (10, 1, 20, 40, 39),
                 (10, 1, 20, 40, 1281), (10, 1, 513, 513, 513)):
        assert lib.bn_hmm_grid_forward_backward_ws_bytes(*args) == 0
    fb = lambda M, KT, XT, counts, want=1: lib.bn_hmm_grid_forward_backward(
        None, None, 1, M, KT, XT, 10, None, None, None, *counts, None, None, want, None, None, None, None, 0, None)
    assert fb(20, 513, 600, (20, 0, 0, 0)) == -2
    assert fb(20, 40, 100, (19, 0, 0, 0)) == -2              # the classes do not add up to the models
    assert fb(20, 40, 100, (21, -1, 0, 0)) == -2
    assert fb(20, 40, 100, (20, 0, 0, 0), want=2) == -2
    # NULL operands with shapes that are served
    assert fb(20, 40, 100, (20, 0, 0, 0)) == -1
    assert lib.bn_arhmm_grid_loglik(None, 4, None, None, 1, 4, 1, 40, 10, None, None, None, None, 0, None) == -1
    assert lib.bn_arhmm_grid_moments(None, 4, None, None, 1, 4, 1, 40, 10, None, None, None, None, 0, None) == -1
