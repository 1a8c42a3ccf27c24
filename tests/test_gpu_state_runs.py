"""bn_state_runs (csrc/state_runs.hip), its wrapper and ARHMM.table_runs against the loops of
tests/state_runs_refs.py.  Every output is an integer: all comparisons are exact, and the launches write into
sentinel-filled outputs so that a row past the last run, or a byte past the outputs, shows.

Shapes are named by the kernel's partition (T = _hip.STATE_RUNS_TILE rows a workgroup, _hip.STATE_RUNS_SCAN tile
counts a step of the scan): runs across tile boundaries, a trial boundary on one, and a table long enough that the
scan over the tiles' counts carries from one step to the next."""

import numpy as np
import pytest
import torch

from behavenet_amd import _hip
from behavenet_amd.models.arhmm import ARHMM
from tests import arhmm_refs
from tests import state_runs_refs as refs

pytestmark = pytest.mark.gpu
DEV = 'cuda'
T = _hip.STATE_RUNS_TILE
SENTINEL = -9
GUARD = 3               # rows of runs past the capacity


def _launch(states, offsets, K, cap=None, skew=0):
    """One bn_state_runs call into sentinel-filled outputs -> host (runs incl. guard rows, frames, trans, R, bad).
    ``skew``: elements the states start off a 16-byte boundary (the kernel's element-by-element loads)."""
    states = np.asarray(states, dtype=np.int32)
    n, S = len(states), len(offsets) - 1
    cap = n if cap is None else cap
    buf = torch.full((n + 4,), -7, dtype=torch.int32, device=DEV)
    st = buf[skew:skew + n]
    st.copy_(torch.from_numpy(states))
    assert st.data_ptr() % 16 == (4 * skew) % 16
    off = torch.from_numpy(np.asarray(offsets, dtype=np.int64)).to(DEV)
    runs = torch.full((cap + GUARD, 4), SENTINEL, dtype=torch.int32, device=DEV)
    stats = torch.full((K + K * K + 2 + GUARD,), SENTINEL, dtype=torch.int64, device=DEV)
    lib = _hip.load()
    nbytes = lib.bn_state_runs_ws_bytes(n, S, K)
    assert nbytes > 0
    ws = torch.empty((nbytes + 16,), dtype=torch.uint8, device=DEV)
    at = stats.data_ptr()
    rc = lib.bn_state_runs(st.data_ptr(), off.data_ptr(), S, K, n, runs.data_ptr(), cap, at, at + 8 * K,
                           at + 8 * (K + K * K), at + 8 * (K + K * K + 1), ws.data_ptr(), nbytes,
                           torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    stats = stats.cpu().numpy()
    assert np.all(stats[K + K * K + 2:] == SENTINEL)
    return (runs.cpu().numpy(), stats[:K], stats[K:K + K * K].reshape(K, K), int(stats[K + K * K]),
            int(stats[K + K * K + 1]))


def _check(states, offsets, K, skew=0, wrapper=True):
    states = np.asarray(states, dtype=np.int32)
    offsets = np.asarray(offsets, dtype=np.int64)
    want = refs.runs_of(states, offsets)
    runs, frames, trans, R, bad = _launch(states, offsets, K, skew=skew)
    assert R == len(want) and bad == 0
    assert np.array_equal(runs[:R], want)
    assert np.all(runs[R:] == SENTINEL)                      # nothing past the last run
    assert np.array_equal(frames, refs.frames_of(states, offsets, K))
    assert np.array_equal(trans, refs.trans_of(states, offsets, K))
    assert int(frames.sum()) == int(offsets[-1] - offsets[0])
    assert int(trans.sum()) == int(frames.sum()) - int(np.count_nonzero(np.diff(offsets)))
    if wrapper:
        r, f, t = _hip.state_runs(torch.from_numpy(states).to(DEV), offsets, K)
        assert r.dtype == torch.int32 and f.dtype == torch.int64 and t.dtype == torch.int64
        assert r.is_cuda and tuple(r.shape) == (R, 4) and tuple(f.shape) == (K,) and tuple(t.shape) == (K, K)
        assert np.array_equal(r.cpu().numpy(), want)
        assert np.array_equal(f.cpu().numpy(), frames) and np.array_equal(t.cpu().numpy(), trans)
    return want


def _sticky(rng, n, K, mean=6):
    """A path of n states whose runs last about ``mean`` rows."""
    if K == 1:
        return np.zeros(n, dtype=np.int32)
    out = np.zeros(n, dtype=np.int32)
    i, z = 0, int(rng.randint(K))
    while i < n:
        d = 1 + int(rng.geometric(1.0 / mean))
        out[i:i + d] = z
        i += d
        z = (z + 1 + int(rng.randint(K - 1))) % K
    return out


def test_one_row():
    assert _check([1], [0, 1], 2).tolist() == [[0, 0, 1, 1]]


def test_one_trial_of_one_state():
    assert _check(np.full(300, 2), [0, 300], 3).tolist() == [[0, 0, 300, 2]]


def test_alternating_states_every_row_is_a_run():
    n = 2 * T + 3
    want = _check(np.arange(n) % 2, [0, n], 2)
    assert len(want) == n


def test_one_row_trials():
    n = T + 7
    rng = np.random.RandomState(0)
    want = _check(rng.randint(0, 2, size=n), np.arange(n + 1), 2)
    assert len(want) == n and np.array_equal(want[:, 0], np.arange(n)) and np.all(want[:, 1] == 0)


def test_empty_trials_first_in_the_middle_and_last():
    rng = np.random.RandomState(1)
    lengths = [0, 0, 5, 0, 0, 0, 40, 1, 0, 9, 0, 0]
    offsets = np.concatenate(([0], np.cumsum(lengths)))
    states = _sticky(rng, int(offsets[-1]), 3, mean=3)
    states[4] = states[5]                                    # trials 2 and 6 meet in the same state: two runs
    want = _check(states, offsets, 3)
    assert sorted(set(want[:, 0].tolist())) == [2, 6, 7, 9]
    last_of_2, first_of_6 = want[want[:, 0] == 2][-1], want[want[:, 0] == 6][0]
    assert last_of_2[2] == 5 and first_of_6[1] == 0 and last_of_2[3] == first_of_6[3]


@pytest.mark.parametrize('skew', [0, 1])
def test_rows_outside_the_trials_are_neither_counted_nor_bad(skew):
    n = 2 * T + 11
    rng = np.random.RandomState(2)
    states = _sticky(rng, n, 4)
    states[:3] = -7
    states[n - 2:] = -7
    offsets = [3, 50, 50, T + 2, n - 2]
    want = _check(states, offsets, 4, skew=skew, wrapper=(skew == 0))
    assert want[0, 0] == 0 and want[0, 1] == 0 and int(want[-1, 2]) == n - 2 - (T + 2)


@pytest.mark.parametrize('n', [T - 1, T, T + 1, 3 * T + 5])
def test_tile_boundaries(n):
    rng = np.random.RandomState(n)
    states = _sticky(rng, n, 3)
    if n > T:
        # a trial boundary exactly on the tile boundary with the same state on both sides: it must split the run
        states[T - 4:min(T + 4, n)] = 1
        offsets = [0, 17, T, n]
        if n > 2 * T + 4:
            states[2 * T - 3:2 * T + 3] = 2                  # ... and one run across the next tile boundary
    else:
        states[n - 6:] = 1                                    # a run into the last rows of the tile
        offsets = [0, 17, n]
    want = _check(states, offsets, 3)
    if n > T:
        ends = {(int(r[0]), int(r[2])) for r in want}
        begs = {(int(r[0]), int(r[1]), int(r[3])) for r in want}
        assert (1, T - 17) in ends and (2, 0, 1) in begs
    if n > 2 * T + 4:
        assert any(r[0] == 2 and r[1] <= T - 3 and r[2] >= T + 3 and r[3] == 2 for r in want)


@pytest.mark.parametrize('K', [1, 2, 32])
def test_states(K):
    n = T + 300
    rng = np.random.RandomState(K)
    _check(_sticky(rng, n, K, mean=2), [0, 100, 100, 700, n], K)


def test_the_scan_over_tile_counts_carries():
    """More tiles than one step of k_sr_scan takes: about a million rows."""
    n = T * _hip.STATE_RUNS_SCAN + T + 5
    rng = np.random.RandomState(7)
    states = _sticky(rng, n, 32, mean=9)
    cuts = np.sort(rng.choice(np.arange(1, n), size=37, replace=False))
    offsets = np.concatenate(([0, 0], cuts, [cuts[-1]], [n]))
    want = _check(states, offsets, 32, wrapper=False)
    assert len(want) > 2 * _hip.STATE_RUNS_SCAN                 # runs behind the first step of the scan


def test_a_smaller_capacity_drops_rows_but_counts_them():
    rng = np.random.RandomState(3)
    n = T + 50
    states = _sticky(rng, n, 3, mean=2)
    want = refs.runs_of(states, np.asarray([0, n]))
    cap = len(want) // 2
    runs, frames, _, R, bad = _launch(states, [0, n], 3, cap=cap)
    assert R == len(want) and bad == 0 and int(frames.sum()) == n
    assert np.array_equal(runs[:cap], want[:cap]) and np.all(runs[cap:] == SENTINEL)


@pytest.mark.parametrize('value', [3, -1])
def test_a_state_outside_the_model_is_refused_with_its_count(value):
    rng = np.random.RandomState(4)
    n = T + 20
    states = _sticky(rng, n, 3)
    states[[0, 5, T, T + 1]] = value                          # four rows, and ...
    states[n - 1] = value                                     # ... one outside the trials, which does not count
    *_, bad = _launch(states, [0, 40, n - 1], 3)
    assert bad == 4
    with pytest.raises(ValueError, match=r'state_runs: 4 rows'):
        _hip.state_runs(torch.from_numpy(states).to(DEV), np.asarray([0, 40, n - 1]), 3)


def test_the_wrapper_s_checks_and_empty_results():
    states = torch.zeros((5,), dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match='int32'):
        _hip.state_runs(states.to(torch.int64), [0, 5], 2)
    with pytest.raises(ValueError, match='on the GPU'):
        _hip.state_runs(states.cpu(), [0, 5], 2)
    with pytest.raises(ValueError, match='contiguous'):
        _hip.state_runs(torch.zeros((10,), dtype=torch.int32, device=DEV)[::2], [0, 5], 2)
    with pytest.raises(ValueError, match='states'):
        _hip.state_runs(states, [0, 5], _hip.ARHMM_MAX_K + 1)
    for st, off in ((states, [0]), (states[:0], [0, 0])):
        runs, frames, trans = _hip.state_runs(st, np.asarray(off), 2)
        assert tuple(runs.shape) == (0, 4) and runs.dtype == torch.int32
        assert frames.cpu().tolist() == [0, 0] and trans.cpu().tolist() == [[0, 0], [0, 0]]


def test_table_runs_of_a_fitted_model():
    K, D, L = 3, 2, 1
    datas, _ = arhmm_refs.sample_arhmm(np.random.RandomState(2), K, D, L, [40, 0, 25, 60, 1])
    m = ARHMM(K, D, lags=L)
    m.fit(datas, num_iters=3, seed=1)
    table, offsets = ARHMM.as_table(datas)
    path = m.table_states(table, offsets)
    runs, frames, trans = m.table_runs(table, offsets)
    assert isinstance(runs, np.ndarray) and runs.dtype == np.int32
    assert frames.dtype == np.int64 and trans.dtype == np.int64
    assert np.array_equal(runs, refs.runs_of(path, offsets))
    assert np.array_equal(frames, refs.frames_of(path, offsets, K))
    assert np.array_equal(trans, refs.trans_of(path, offsets, K))
    assert len(runs) > 4                                      # (the separated states are found: not one run a trial)
