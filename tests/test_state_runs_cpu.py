"""The host half of the state runs and the syllable movie (fitting.eval: discrete_chunks, state_durations,
syllable_instances, syllable_movie_plan) against the restatements of tests/state_runs_refs.py and against what the
reference's get_discrete_chunks returned (tests/golden/discrete_chunks.json).  Integers throughout: every comparison
is exact.  No GPU."""

import json
import os

import numpy as np
import pytest

from behavenet_amd import _hip
from behavenet_amd.fitting.eval import (discrete_chunks, state_durations, syllable_instances, syllable_movie_plan)
from tests import state_runs_refs as refs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'discrete_chunks.json')

# hand-made paths: (trials, K)
PATHS = {
    'a single run': ([[0, 0, 0, 0]], 2),
    'alternating': ([[0, 1, 0, 1, 0, 1]], 2),
    'a state that never occurs': ([[0, 0, 2, 2, 2, 0]], 3),
    'runs at each edge': ([[1, 1, 0, 0, 1], [1, 0, 0, 0, 0], [0, 1, 1, 1, 1]], 2),
    'a one-frame trial': ([[2], [0, 0, 1], [], [1]], 4),
    'one state': ([[0, 0, 0], [0]], 1),
}


def _table(paths):
    lengths = np.asarray([len(p) for p in paths], dtype=np.int64)
    offsets = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    states = np.concatenate([np.asarray(p, dtype=np.int32) for p in paths])
    return states, offsets, lengths


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == np.int64 and g.shape == w.shape, (g, w)
        assert np.array_equal(g, w), (g, w)


@pytest.mark.parametrize('name', sorted(PATHS))
@pytest.mark.parametrize('include_edges', [True, False])
def test_chunks_and_durations(name, include_edges):
    paths, K = PATHS[name]
    states, offsets, lengths = _table(paths)
    runs = refs.runs_of(states, offsets)
    got = discrete_chunks(runs, K, lengths, include_edges)
    assert len(got) == K and all(g.ndim == 2 and g.shape[1] == 3 for g in got)
    _same(got, refs.chunks_of(paths, K, include_edges))
    durations = state_durations(runs, K, lengths, include_edges)
    want = refs.durations_of(paths, K, include_edges)
    if K == 1:
        assert durations == [] and want == []
    else:
        _same(durations, want)
    if include_edges:
        # every frame of every trial lies in exactly one chunk
        assert sum(int((g[:, 2] - g[:, 1]).sum()) for g in got) == int(lengths.sum())


def test_chunks_refuse_runs_outside_the_trials_or_the_model():
    runs = np.asarray([[0, 0, 2, 1]], dtype=np.int32)
    with pytest.raises(ValueError, match='trial 1 of 1'):
        discrete_chunks(np.asarray([[1, 0, 2, 1]]), 2, [2])
    with pytest.raises(ValueError, match='state 1 of 1'):
        discrete_chunks(runs, 1, [2])
    assert [c.shape for c in discrete_chunks(np.zeros((0, 4), dtype=np.int32), 3, [])] == [(0, 3)] * 3


def test_the_reference_s_chunks():
    """What the reference's get_discrete_chunks returned on the recorded paths; it has max(state) + 1 entries, and
    an empty (0,) array where this project has (0, 3)."""
    with open(GOLDEN) as f:
        cases = json.load(f)
    assert len(cases) >= 12
    for case in cases:
        paths = case['states']
        states, offsets, lengths = _table(paths)
        K = int(states.max()) + 1
        assert len(case['chunks']) == K
        got = discrete_chunks(refs.runs_of(states, offsets), K, lengths, case['include_edges'])
        _same(got, [np.asarray(c, dtype=np.int64).reshape(-1, 3) for c in case['chunks']])


def test_the_restated_tile_is_the_kernel_s():
    """STATE_RUNS_TILE against the workspace query: the offsets and two ints per tile of rows."""
    lib = _hip.load()
    pad16 = lambda b: (b + 15) // 16 * 16
    T = _hip.STATE_RUNS_TILE
    for n in (0, 1, T - 1, T, T + 1, 9 * T + 5, 2 ** 31 - 1):
        for S in (1, 4, 7):
            assert lib.bn_state_runs_ws_bytes(n, S, 3) == pad16(4 * (S + 1)) + 2 * pad16(4 * (-(-n // T))), (n, S)
    assert lib.bn_state_runs_ws_bytes(-1, 1, 3) == 0
    assert lib.bn_state_runs_ws_bytes(5, 1, 0) == 0
    assert lib.bn_state_runs_ws_bytes(5, 1, _hip.ARHMM_MAX_K + 1) == 0
    assert lib.bn_state_runs_ws_bytes(5, 1, _hip.ARHMM_MAX_K) > 0
    # argument errors are reported, not thrown (nothing is launched)
    assert lib.bn_state_runs(None, None, 1, 0, 5, None, 0, None, None, None, None, None, 0, None) == -2
    assert lib.bn_state_runs(None, None, 1, 2, 5, None, 0, None, None, None, None, None, 0, None) == -1
    assert lib.bn_stamp_boxes_u8(None, 1, 1, 1, 0, 4, None, 0, 0, 1, 1, 255, None) == -2
    assert lib.bn_stamp_boxes_u8(None, 1, 1, 1, 4, 4, None, 0, 0, 1, 1, 256, None) == -2
    assert lib.bn_stamp_boxes_u8(None, 1, 1, 1, 4, 4, None, 0, 0, 1, 1, 255, None) == -1
    assert lib.bn_stamp_boxes_u8(None, 0, 1, 1, 4, 4, None, 0, 0, 1, 1, 255, None) == 0


# ------------------------------------------------------------------------------------------------------------
def _chunks(*per_state):
    return [np.asarray(c, dtype=np.int64).reshape(-1, 3) for c in per_state]


def test_instances_threshold_is_strict_and_the_shuffle_is_seeded():
    chunks = _chunks([[0, 0, 3], [0, 5, 7], [1, 2, 3], [1, 4, 9], [2, 0, 4], [2, 6, 8]], [], [[0, 3, 5], [1, 0, 2]])
    kept = syllable_instances(chunks, min_threshold=2, seed=3)
    assert len(kept) == 3 and [k.shape for k in kept] == [(3, 3), (0, 3), (0, 3)]
    assert sorted(map(tuple, kept[0])) == [(0, 0, 3), (1, 4, 9), (2, 0, 4)]           # length 2 is not "> 2"
    everything = syllable_instances(chunks, min_threshold=0, seed=3)
    assert [sorted(map(tuple, k)) for k in everything] == [sorted(map(tuple, c)) for c in chunks]
    again = syllable_instances(chunks, min_threshold=0, seed=3)
    assert all(np.array_equal(a, b) for a, b in zip(everything, again))
    # ONE generator, the states in order
    rng = np.random.RandomState(3)
    for c, got in zip(chunks, everything):
        want = c.copy()
        rng.shuffle(want)
        assert np.array_equal(got, want)
    orders = {tuple(map(tuple, syllable_instances(chunks, seed=s)[0])) for s in range(8)}
    assert len(orders) > 1
    assert np.array_equal(chunks[0][0], [0, 0, 3])                                    # the input is not shuffled


PLANS = {
    # name: (state_list, kwargs)
    'instances run out: a blank tail': (_chunks([[0, 4, 6]], [[1, 3, 9], [0, 10, 12]]), dict(max_frames=30)),
    'a clip passes max_frames': (_chunks([[0, 5, 25]], [[1, 3, 5]]), dict(max_frames=10)),
    'beg < n_pre_frames shifts the mark': (_chunks([[0, 1, 4], [1, 0, 3], [2, 2, 5]], [[0, 7, 9]]),
                                          dict(max_frames=12, n_pre_frames=3)),
    'a mark on a one-frame clip': (_chunks([[0, 0, 1], [1, 0, 1]], [[0, 1, 2]]), dict(max_frames=6, n_pre_frames=0)),
    'n_buffer = 0': (_chunks([[0, 3, 5], [1, 4, 8]], [[0, 5, 9], [1, 0, 2]]), dict(max_frames=9, n_buffer=0)),
    'single_syllable': (_chunks([[0, 3, 5]], [[1, 4, 8], [0, 6, 7]], []), dict(max_frames=8, single_syllable=1)),
    'n_rows given': (_chunks([[0, 3, 5]], [[1, 4, 8]], [[0, 0, 2]], [], [[2, 1, 3]]), dict(max_frames=7, n_rows=1)),
    'five states, one absent': (_chunks([[0, 3, 5]], [[1, 4, 8]], [[0, 0, 2]], [], [[2, 1, 3]]),
                                dict(max_frames=7, n_buffer=2, n_pre_frames=1)),
}


def plan_case(name):
    state_list, kw = PLANS[name]
    kw = dict(dict(max_frames=400, n_buffer=5, n_pre_frames=3, n_rows=None, single_syllable=None), **kw)
    return state_list, kw


@pytest.mark.parametrize('name', sorted(PLANS))
def test_plan(name):
    state_list, kw = plan_case(name)
    src, mark, n_rows, n_cols = syllable_movie_plan(state_list, **kw)
    want_src, want_mark, want_rows, want_cols = refs.plan_of(state_list, **kw)
    assert (n_rows, n_cols) == (want_rows, want_cols)
    assert src.dtype == np.int64 and mark.dtype == np.uint8
    assert src.shape == want_src.shape == (len(mark), n_rows, n_cols, 2) and mark.shape == want_mark.shape
    assert np.array_equal(src, want_src) and np.array_equal(mark, want_mark)
    assert len(mark) >= kw['max_frames']
    assert not np.any(mark[src[..., 0] < 0])                                          # no mark on a blank panel


def test_plan_by_hand():
    """The cases a reader can check on paper."""
    src, mark, n_rows, n_cols = syllable_movie_plan(_chunks([[0, 1, 4], [2, 5, 6]]), max_frames=9, n_buffer=2,
                                                    n_pre_frames=3)
    assert (n_rows, n_cols) == (1, 1)
    # beg 1 < 3: the clip starts at row 0 and its marks sit on clip frames 1 and 2; then rows 2 .. 5 of chunk 2
    assert src[:, 0, 0].tolist() == [[0, 0], [0, 1], [0, 2], [0, 3], [-1, -1], [-1, -1],
                                     [2, 2], [2, 3], [2, 4], [2, 5], [-1, -1], [-1, -1]]
    assert mark[:, 0, 0].tolist() == [0, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0]
    # a clip is never cut: 12 frames for max_frames = 9.  The grid of five states: floor(sqrt(5)) = 2 rows of 3
    five = _chunks([[0, 3, 5]], [[1, 4, 8]], [[0, 0, 2]], [], [[2, 1, 3]])
    src, mark, n_rows, n_cols = syllable_movie_plan(five, max_frames=7, n_buffer=0, n_pre_frames=0)
    assert (n_rows, n_cols) == (2, 3) and src.shape == (7, 2, 3, 2)
    assert src[:, 1, 0, 0].tolist() == [-1] * 7 and src[:, 1, 2, 0].tolist() == [-1] * 7      # state 3; no sixth state
    assert src[:, 1, 1].tolist() == [[2, 1], [2, 2]] + [[-1, -1]] * 5                           # state 4
    assert mark[:, 0, 1].tolist() == [1, 1, 0, 0, 0, 0, 0]


def test_plan_refusals():
    with pytest.raises(ValueError, match='no state has an instance'):
        syllable_movie_plan(_chunks([], [], []))
    with pytest.raises(ValueError, match='state 2 has no instances'):
        syllable_movie_plan(_chunks([[0, 3, 5]], [[1, 4, 8]], []), single_syllable=2)
    with pytest.raises(ValueError, match='state 7 has no instances'):
        syllable_movie_plan(_chunks([[0, 3, 5]]), single_syllable=7)
    with pytest.raises(ValueError, match='n_rows'):
        syllable_movie_plan(_chunks([[0, 3, 5]]), n_rows=0)
    with pytest.raises(ValueError, match='max_frames'):
        syllable_movie_plan(_chunks([[0, 3, 5]]), max_frames=0)
