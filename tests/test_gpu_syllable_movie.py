"""bn_stamp_boxes_u8 (csrc/frame_mosaic.hip), the syllable movie (fitting.eval.syllable_movie) and
plotting.arhmm_utils on the synthetic generator, byte for byte against the slicing of tests/state_runs_refs.py."""

import os

import numpy as np
import pytest
import torch

from behavenet_amd import _hip
from behavenet_amd.fitting.eval import (discrete_chunks, syllable_instances, syllable_movie, syllable_movie_device)
from behavenet_amd.plotting import arhmm_utils
from tests import state_runs_refs as refs
from tests.test_state_runs_cpu import PLANS, PATHS, plan_case

pytestmark = pytest.mark.gpu
DEV = 'cuda'


# ------------------------------------------------------------------------------------------------------------
# bn_stamp_boxes_u8
# ------------------------------------------------------------------------------------------------------------
def _movie(rng, T, R, Cc, Hp, Wp):
    return rng.randint(0, 200, size=(T, R * Hp, Cc * Wp)).astype(np.uint8)


STAMPS = {
    # name: (T, R, Cc, Hp, Wp, box, value)
    'a panel smaller than the box': (3, 2, 3, 8, 8, (5, 5, 10, 10), 255),
    'the box at the far corner': (2, 2, 2, 24, 40, (14, 30, 10, 10), 255),
    'the box passes the far corner': (2, 2, 2, 24, 40, (20, 35, 10, 10), 7),
    'a row length that is no multiple of 16': (4, 1, 3, 17, 7, (5, 5, 10, 10), 255),
    'one frame': (1, 3, 2, 16, 16, (5, 5, 10, 10), 255),
    'a negative origin is clipped': (2, 1, 2, 16, 20, (-3, -4, 10, 10), 128),
    'the whole panel': (2, 2, 2, 12, 20, (0, 0, 12, 20), 1),
}


@pytest.mark.parametrize('name', sorted(STAMPS))
def test_stamp(name):
    T, R, Cc, Hp, Wp, box, value = STAMPS[name]
    rng = np.random.RandomState(len(name))
    movie = _movie(rng, T, R, Cc, Hp, Wp)
    for mark in (rng.randint(0, 2, size=(T, R, Cc)).astype(np.uint8) * 3,          # (any non-zero byte marks)
                 np.zeros((T, R, Cc), dtype=np.uint8), np.ones((T, R, Cc), dtype=np.uint8)):
        dev = torch.from_numpy(movie).to(DEV)
        out = _hip.stamp_boxes_u8(dev, torch.from_numpy(mark).to(DEV), (Hp, Wp), box, value)
        assert out is dev                                                          # in place
        want = refs.stamped(movie, mark, (Hp, Wp), box, value)
        assert np.array_equal(out.cpu().numpy(), want)
        if not mark.any():
            assert np.array_equal(want, movie)                                     # no marks: untouched
        else:
            assert not np.array_equal(want, movie)
        # a host mark is uploaded
        assert np.array_equal(_hip.stamp_boxes_u8(torch.from_numpy(movie).to(DEV), mark, (Hp, Wp), box, value)
                              .cpu().numpy(), want)


def test_stamp_default_box_and_no_ops():
    rng = np.random.RandomState(0)
    movie = _movie(rng, 2, 1, 2, 20, 24)
    mark = np.ones((2, 1, 2), dtype=np.uint8)
    got = _hip.stamp_boxes_u8(torch.from_numpy(movie).to(DEV), mark, (20, 24)).cpu().numpy()
    want = movie.copy()
    for c in range(2):
        want[:, 5:15, c * 24 + 5:c * 24 + 15] = 255
    assert np.array_equal(got, want)
    # a box wholly outside the panel, an empty box, an empty movie
    for box in ((20, 0, 5, 5), (0, 24, 5, 5), (-10, 0, 10, 5), (3, 3, 0, 4)):
        assert np.array_equal(_hip.stamp_boxes_u8(torch.from_numpy(movie).to(DEV), mark, (20, 24), box).cpu().numpy(),
                              movie)
    empty = torch.zeros((0, 20, 48), dtype=torch.uint8, device=DEV)
    assert _hip.stamp_boxes_u8(empty, np.zeros((0, 1, 2), dtype=np.uint8), (20, 24)) is empty


def test_stamp_refusals():
    movie = torch.zeros((2, 20, 48), dtype=torch.uint8, device=DEV)
    mark = np.ones((2, 1, 2), dtype=np.uint8)
    with pytest.raises(ValueError, match='uint8 movie'):
        _hip.stamp_boxes_u8(movie.to(torch.float32), mark, (20, 24))
    with pytest.raises(ValueError, match='uint8 movie'):
        _hip.stamp_boxes_u8(movie[0], mark, (20, 24))
    with pytest.raises(ValueError, match='uint8 movie'):
        _hip.stamp_boxes_u8(torch.zeros((2, 20, 96), dtype=torch.uint8, device=DEV)[:, :, ::2], mark, (20, 24))
    with pytest.raises(ValueError, match='on the GPU'):
        _hip.stamp_boxes_u8(movie.cpu(), mark, (20, 24))
    for bad_mark, hw in ((mark, (20, 16)), (mark, (10, 24)), (np.ones((1, 1, 2), dtype=np.uint8), (20, 24)),
                         (np.ones((2, 2), dtype=np.uint8), (20, 24)), (np.ones((2, 2, 1), dtype=np.uint8), (20, 24))):
        with pytest.raises(ValueError, match='does not divide'):
            _hip.stamp_boxes_u8(movie, bad_mark, hw)
    with pytest.raises(ValueError, match='uint8'):
        _hip.stamp_boxes_u8(movie, torch.ones((2, 1, 2), dtype=torch.int32, device=DEV), (20, 24))
    with pytest.raises(ValueError, match='value'):
        _hip.stamp_boxes_u8(movie, mark, (20, 24), value=256)
    assert not movie.any()                                                         # nothing was written


# ------------------------------------------------------------------------------------------------------------
# syllable_movie
# ------------------------------------------------------------------------------------------------------------
N_TRIALS, N_FRAMES = 3, 26           # the plans of tests/test_state_runs_cpu.py name chunks 0 .. 2, rows 0 .. 24


def _trials(dims, dtype, seed=0):
    rng = np.random.RandomState(seed)
    C, H, W = dims
    if dtype == np.uint8:
        return [rng.randint(0, 255, size=(N_FRAMES, C, H, W)).astype(np.uint8) for _ in range(N_TRIALS)]
    # unit floats with a few values beyond [0, 1]
    return [(rng.rand(N_FRAMES, C, H, W) * 1.2 - 0.1).astype(np.float32) for _ in range(N_TRIALS)]


@pytest.mark.parametrize('name', sorted(PLANS))
@pytest.mark.parametrize('dtype', [np.uint8, np.float32])
@pytest.mark.parametrize('dims', [(2, 12, 20), (1, 16, 16)])
def test_movie(dims, dtype, name):
    state_list, kw = plan_case(name)
    trials = _trials(dims, dtype)
    src, mark, n_rows, n_cols = refs.plan_of(state_list, **kw)
    want = refs.movie_of(trials, src, mark)
    C, H, W = dims
    asked = []

    def frames_of(chunk):
        asked.append(chunk)
        return trials[chunk]
    # chunk_size smaller than the movie: several mosaic launches
    movie, got_mark = syllable_movie(frames_of, state_list, chunk_size=4, **kw)
    assert movie.dtype == np.uint8 and movie.shape == (len(src), n_rows * C * H, n_cols * W)
    assert len(src) > 4
    assert np.array_equal(got_mark, mark)
    assert np.array_equal(movie, want)
    # only the planned chunks are asked for, each once
    assert sorted(asked) == sorted(set(int(c) for c in src[..., 0].ravel() if c >= 0))
    # a list of device tensors, one mosaic launch
    on_dev = [torch.from_numpy(t).to(DEV) for t in trials]
    movie_d, _ = syllable_movie_device(on_dev, state_list, **kw)
    assert movie_d.is_cuda and movie_d.dtype == torch.uint8 and np.array_equal(movie_d.cpu().numpy(), want)
    assert want[mark.astype(bool).any(axis=(1, 2))].max() == 255


def test_movie_of_three_states_with_one_absent():
    paths, K = PATHS['a state that never occurs']
    paths = [paths[0], [2, 2, 0, 0, 0, 2, 2, 2]]
    lengths = [len(p) for p in paths]
    offsets = np.concatenate(([0], np.cumsum(lengths)))
    runs = refs.runs_of(np.concatenate(paths), offsets)
    instances = syllable_instances(discrete_chunks(runs, K, lengths), min_threshold=1, seed=2)
    assert [len(i) for i in instances] == [2, 0, 3]
    trials = [t[:n] for t, n in zip(_trials((2, 12, 20), np.uint8, seed=5), lengths)]
    kw = dict(max_frames=12, n_buffer=1, n_pre_frames=2, n_rows=None, single_syllable=None)
    src, mark, n_rows, n_cols = refs.plan_of(instances, **kw)
    assert (n_rows, n_cols) == (1, 3) and np.all(src[:, 0, 1] == -1)
    movie, _ = syllable_movie(trials, instances, **kw)
    assert np.array_equal(movie, refs.movie_of(trials, src, mark))
    assert not movie[:, :, 20:40].any()                                            # the absent state's panel is black


def test_movie_refusals():
    trials = _trials((1, 16, 16), np.uint8)
    inst = [np.asarray([[0, 3, 5]]), np.asarray([[1, 20, 30]])]
    with pytest.raises(ValueError, match='ends at frame 30'):
        syllable_movie(trials, inst, max_frames=5)
    with pytest.raises(ValueError, match='no state has an instance'):
        syllable_movie(trials, [np.zeros((0, 3)), np.zeros((0, 3))])
    with pytest.raises(ValueError, match='chunk_size'):
        syllable_movie(trials, inst[:1], chunk_size=0)
    mixed = [trials[0], trials[1][:, :, :8]]
    with pytest.raises(ValueError, match='the first trial shown'):
        syllable_movie(mixed, [np.asarray([[0, 3, 5]]), np.asarray([[1, 2, 4]])], max_frames=5)


# ------------------------------------------------------------------------------------------------------------
# plotting.arhmm_utils
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('include_edges', [True, False])
def test_get_discrete_chunks(include_edges):
    for name in sorted(PATHS):
        paths, _ = PATHS[name]
        got = arhmm_utils.get_discrete_chunks([np.asarray(p, dtype=np.int64) for p in paths], include_edges)
        K = max(max(p) for p in paths if len(p)) + 1                               # the reference's count
        want = refs.chunks_of(paths, K, include_edges)
        assert len(got) == K
        assert all(np.array_equal(g, w) and g.shape == w.shape for g, w in zip(got, want))
    with pytest.raises(ValueError, match='no frames'):
        arhmm_utils.get_discrete_chunks([[], []])
    with pytest.raises(ValueError, match='1 rows'):
        arhmm_utils.get_discrete_chunks([[0, -1, 2]])


def test_make_syllable_movies_on_the_synthetic_generator(tmp_path):
    from behavenet_amd.fitting.eval import fit_arhmm, sample_arhmm
    from tests.test_gpu_ranges import LENS, _generator, _model as _ae
    model, meta = _ae('ae_cfg1', str(tmp_path))
    gen = _generator(meta, n_sessions=2)
    arhmm, _ = fit_arhmm(gen, model, n_states=3, n_lags=1, n_iters=2, rng_seed_model=1)
    C, H, W = meta['dim']
    path = os.path.join(str(tmp_path), 'syllables.npy')
    kw = dict(max_frames=30, min_threshold=0, n_buffer=2, n_pre_frames=2)
    movie = arhmm_utils.make_syllable_movies(model, gen, arhmm, sess_idx=1, dtype='train', seed=4, save_file=path, **kw)
    assert movie.dtype == np.uint8 and movie.ndim == 3 and movie.shape[0] >= 30
    assert movie.shape[1:] == (1 * C * H, 3 * W)                                  # floor(sqrt(3)) = 1 row of 3
    assert np.array_equal(np.load(path), movie)
    # the same movie from the states sample_arhmm exports and the stored frames
    out = sample_arhmm(gen, model, arhmm, n_samples=0, dtype='train', sess_idx=1)
    paths, trials = out['states']['train'], [int(t) for t in out['trial_idxs']['train']]
    lengths = [len(p) for p in paths]
    assert lengths == [LENS[t] for t in trials]
    runs = refs.runs_of(np.concatenate(paths), np.concatenate(([0], np.cumsum(lengths))))
    instances = syllable_instances(discrete_chunks(runs, 3, lengths), min_threshold=0, seed=4)
    frames = [gen.datasets[1].images_u8[t] for t in trials]
    want, _ = syllable_movie(frames, instances, max_frames=30, n_buffer=2, n_pre_frames=2)
    assert np.array_equal(movie, want)
    src, mark, _, _ = refs.plan_of(instances, 30, 2, 2)
    assert np.array_equal(movie, refs.movie_of([np.asarray(f) for f in frames], src, mark))
    # durations: every train frame of the session is in one run
    durations = arhmm_utils.get_state_durations(out['latents']['train'], arhmm)
    assert sum(int(d.sum()) for d in durations) == sum(lengths)
    assert arhmm_utils.get_state_durations(out['latents']['train'], type('One', (), {'K': 1})()) == []
    single = arhmm_utils.make_syllable_movies(model, gen, arhmm, sess_idx=1, dtype='train', seed=4,
                                              single_syllable=int(runs[0, 3]), **kw)
    assert single.shape[1:] == (C * H, W)
    with pytest.raises(ValueError, match='dtype must be'):
        arhmm_utils.make_syllable_movies(model, gen, arhmm, dtype='all')
