"""Point-path movies and session-swap movies, the host side (no GPU): ``fitting.eval.path_points``, ``swap_points``,
the source tables and layouts against the plain loops of tests/point_path_refs.py, and the argument errors that are
raised before anything reaches the device (a stub model fails on any use)."""

import numpy as np
import pytest
import torch

from behavenet_amd import _hip
from behavenet_amd.fitting import eval as bn_eval
from behavenet_amd.fitting.eval import (path_movie_src, path_points, point_path_movie, session_swap_movie, swap_layout,
                                        swap_points)
from behavenet_amd.plotting import cond_ae_utils as cau
from tests import point_path_refs as refs

D = 7
RNG = np.random.default_rng(11)
BASE = RNG.normal(size=(3, D)).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_path_points_is_the_plain_loop_bit_for_bit(dtype):
    seen = 0
    for n_points in (2, 3):
        points = RNG.normal(size=(n_points, D)).astype(dtype) * 3
        for n_frames in (1, 3, 10, [7] * (n_points - 1), list(range(2, n_points + 1))):
            want = refs.path_loop(points, n_frames)
            got = path_points(points, n_frames)
            counts = [n_frames] * (n_points - 1) if isinstance(n_frames, int) else n_frames
            assert got.dtype == dtype and got.shape == (sum(n + 1 for n in counts), D)
            assert all(w.dtype == dtype and w.shape == (1, D) for w in want)
            assert np.array_equal(_bits(got), _bits(np.concatenate(want, axis=0))), (n_points, n_frames)
            assert np.array_equal(got[0], points[0])          # a path starts at its first point
            if n_points == 3:          # the join appears twice: the end of one leg and the start of the next
                assert np.array_equal(got[counts[0] + 1], points[1])
                assert np.allclose(got[counts[0]], points[1], rtol=1e-5, atol=1e-6)
            seen += 1
    assert seen == 10
    # lists of points and numpy integers are taken as the arrays and ints they are
    assert np.array_equal(path_points([[0.0, 1.0], [1.0, 3.0]], np.int64(2)), [[0, 1], [0.5, 2], [1, 3]])


def test_path_points_refusals():
    points = np.zeros((3, D), dtype=np.float32)
    for n_frames in ([4], [4, 4, 4], []):
        with pytest.raises(AssertionError):
            path_points(points, n_frames)
        with pytest.raises(AssertionError):
            refs.path_loop(points, n_frames)
    with pytest.raises(ValueError, match='at least one frame'):
        path_points(points, [3, 0])
    with pytest.raises(ValueError, match='n_points, D'):
        path_points(np.zeros(D), 3)


def test_swap_points_is_the_per_session_overwrite():
    for dtype in (np.float32, np.float64):
        latents = RNG.normal(size=(5, D)).astype(dtype)
        for idxs, n_sess in [([2], 1), ([4, 5], 3), (np.arange(3, 6), 6)]:
            medians = RNG.normal(size=(n_sess, len(idxs))).astype(np.float32)
            keep = np.copy(latents)
            got = swap_points(latents, idxs, medians)
            want = refs.swap_loop(latents, idxs, medians)
            assert got.dtype == dtype and got.shape == (n_sess * 5, D)
            assert np.array_equal(_bits(got), _bits(want))
            assert np.array_equal(latents, keep)          # the trial's own table is not written
            rest = [d for d in range(D) if d not in list(idxs)]
            assert np.array_equal(got[:, rest], np.tile(latents[:, rest], (n_sess, 1)))
    with pytest.raises(ValueError, match='medians'):
        swap_points(latents, [1, 2], np.zeros((3, 3)))
    with pytest.raises(ValueError, match='background columns'):
        swap_points(latents, [D], np.zeros((3, 1)))
    with pytest.raises(ValueError, match='latents'):
        swap_points(latents[0], [1], np.zeros((3, 1)))


def test_movie_source_tables():
    # (n_base, n_panels, n_frames, n_buffer_frames, n_cols, order_idxs)
    cases = [(1, 4, 3, 5, 3, None), (3, 4, 3, 2, 3, None), (3, 5, 2, 4, 2, [4, 0, 2, 1, 3]), (3, 5, 1, 0, 3, [1, 3]),
             (1, 1, 1, 9, 1, None), (2, 7, 10, 5, 3, None)]
    for n_base, n_panels, n_frames, n_buf, n_cols, order in cases:
        n_steps = 2 * (n_frames + 1)
        want = refs.path_movie_src_loop(n_base, n_panels, n_steps, n_buf, n_cols, order)
        got = path_movie_src(n_base, n_panels, n_steps, n_buf, n_cols, order)
        shown = n_panels if order is None else len(order)
        n_t = n_base * (n_steps + (n_buf if n_base > 1 else 0))
        assert got.dtype == np.int32 and got.shape == (n_t, -(-shown // n_cols), n_cols)
        assert np.array_equal(got, want), (n_base, n_panels, n_frames, n_buf, n_cols, order)
        flat = got.reshape(n_t, -1)
        assert (flat[:, shown:] == -1).all()          # trailing panels are blank
        if n_base == 1:          # no buffer frames: every frame shows every panel
            assert (flat[:, :shown] >= 0).all()
        else:          # ... and the buffer frames after every base point, the last included, are all -1
            per = n_steps + n_buf
            for b in range(n_base):
                assert (flat[b * per + n_steps:(b + 1) * per] == -1).all()
                assert (flat[b * per:b * per + n_steps, :shown] >= 0).all()
        if order is not None:          # position j shows panel order[j]
            assert np.array_equal(flat[0, :shown], np.asarray(order) * n_steps)
        assert int((got >= 0).sum()) == n_base * n_steps * shown
        assert np.array_equal(path_movie_src(n_base, n_panels, n_steps, n_buf, n_cols, order, 1, n_t - 1), want[1:-1])
    # the table the movie decodes: base by base, panel by panel, step by step
    panels = [(2, -1.5, 2.0), (0, -3.0, 1.0)]
    table = refs.movie_table(BASE, panels, 3)
    assert table.shape == (3 * 2 * 8, D)
    assert table[8 + 3, 0] == np.float32(1.0) and table[8 + 4, 0] == np.float32(1.0) and table[8, 0] == np.float32(-3.0)


def test_session_layouts():
    shapes = {2: (1, 2), 3: (1, 3), 4: (2, 2), 5: (2, 3), 6: (2, 3)}
    for n_sess, shape in shapes.items():
        for sess_idx in range(n_sess):
            got = swap_layout(n_sess, sess_idx)
            assert got.shape == shape
            assert np.array_equal(got, refs.swap_grid_loop(n_sess, sess_idx))
            flat = got.reshape(-1)
            assert flat[0] == sess_idx and flat[sess_idx] == 0          # the trial's own session comes first
            assert sorted(flat[:n_sess]) == list(range(n_sess)) and (flat[n_sess:] == -1).all()
    # a pattern with holes
    pattern = np.array([[True, False, True], [False, True, False], [True, False, False]])
    got = swap_layout(4, 2, pattern)
    assert np.array_equal(got, [[2, -1, 1], [-1, 0, -1], [3, -1, -1]])
    assert np.array_equal(got, refs.swap_grid_loop(4, 2, pattern))
    seven = np.ones((2, 4), dtype=bool)
    seven[1, 3] = False
    assert np.array_equal(swap_layout(7, 0, seven), refs.swap_grid_loop(7, 0, seven))
    for n_sess, sess_idx, pat, what in [(7, 0, None, 'layout_pattern'), (4, 0, pattern[:2], 'true entries'),
                                        (3, 0, pattern, 'true entries'), (3, 3, None, 'session 3 of 3'),
                                        (3, -1, None, 'session -1'), (3, 0, np.ones(3, dtype=bool), 'true entries')]:
        with pytest.raises(ValueError, match=what):
            swap_layout(n_sess, sess_idx, pat)


class _Stub(object):
    """What the host-side checks read of a model."""

    def __init__(self, model_class, dim=(2, 8, 12), **hp):
        self.hparams = dict({'model_class': model_class, 'n_input_channels': dim[0], 'y_pixels': dim[1],
                             'x_pixels': dim[2]}, **hp)

    def parameters(self):
        raise AssertionError('the device was reached')

    def eval(self):
        raise AssertionError('the device was reached')


def test_channel_arguments():
    assert _hip.mosaic_channels(0, 3) == (0, 1) and _hip.mosaic_channels(np.int64(2), 3) == (2, 1)
    assert _hip.mosaic_channels(None, 3) == (0, 3) and _hip.mosaic_channels((1, 2), 3) == (1, 2)
    assert _hip.mosaic_channels([0, 3], 3) == (0, 3)
    for ch in (3, -1, (0, 4), (2, 2), (-1, 2), (1, 0), (0, -1)):
        with pytest.raises(ValueError, match='channel'):
            _hip.mosaic_channels(ch, 3)
    for ch in (1.0, 'all', (0, 1, 2), (0.0, 2), slice(0, 2), [1]):
        with pytest.raises(ValueError, match='ch must be'):
            _hip.mosaic_channels(ch, 3)
    assert _hip.check_mosaic_args((3, 2, 8, 12), None, (5, 9, 6, 8)) == (5, 9, 6, 8)
    assert _hip.check_mosaic_args((3, 2, 8, 12), (0, 2), None) == (0, 0, 8, 12)
    # the wrapper refuses before any call (host frames: the library would be the next thing reached)
    frames = torch.zeros((2, 2, 4, 4))
    for ch, what in [('all', 'ch must be'), ((1, 2), 'channels'), (2, 'channel 2')]:
        with pytest.raises(ValueError, match=what):
            _hip.frame_mosaic_u8(frames, [[[0, 1]]], ch=ch)


def test_argument_errors_are_raised_on_the_host():
    model = _Stub('ps-vae')
    panels = [(0, -1.0, 1.0), (3, -2.0, 2.0)]
    for kw, what in [(dict(ch=2), 'channel'), (dict(ch=(1, 2)), 'channels'), (dict(ch='all'), 'ch must be'),
                     (dict(crop_kwargs={'y_0': 1, 'y_ext': 2, 'x_0': 6, 'x_ext': 3}), 'negative origin'),
                     (dict(n_cols=0), 'columns'), (dict(n_frames=0), 'n_frames 0'),
                     (dict(n_buffer_frames=-1), 'n_buffer_frames -1'), (dict(order_idxs=[0, 2]), 'order_idxs'),
                     (dict(order_idxs=[]), 'order_idxs'), (dict(chunk_size=0), 'chunk_size 0')]:
        with pytest.raises(ValueError, match=what):
            point_path_movie(model, BASE, panels, **kw)
    with pytest.raises(ValueError, match='dimension 7'):
        point_path_movie(model, BASE, [(7, 0.0, 1.0)])
    with pytest.raises(ValueError, match='panels'):
        point_path_movie(model, BASE, [])
    with pytest.raises(ValueError, match='base points'):
        point_path_movie(model, BASE[None], panels)
    # session swaps
    model = _Stub('msps-vae')
    trials = [BASE, BASE[:2]]
    for n_sess, kw, what in [(7, {}, 'layout_pattern'), (3, dict(layout_pattern=np.ones((2, 2), dtype=bool)), 'true'),
                             (3, dict(sess_idx=3), 'session 3 of 3'), (3, dict(n_buffer_frames=-2), 'n_buffer'),
                             (3, dict(chunk_size=0), 'chunk_size')]:
        with pytest.raises(ValueError, match=what):
            session_swap_movie(model, trials, [4, 5], np.zeros((n_sess, 2), dtype=np.float32), **kw)
    with pytest.raises(ValueError, match='medians'):
        session_swap_movie(model, trials, [4, 5], np.zeros((3, 1), dtype=np.float32))
    with pytest.raises(ValueError, match='without frames'):
        session_swap_movie(model, [BASE, BASE[:0]], [4, 5], np.zeros((3, 2), dtype=np.float32))
    with pytest.raises(ValueError, match='0 trials'):
        session_swap_movie(model, [], [4, 5], np.zeros((3, 2), dtype=np.float32))
    # the reference-signature entry points
    points = np.stack([BASE[0], BASE[1], BASE[0]])
    with pytest.raises(NotImplementedError):
        cau.interpolate_point_path('latents', _Stub('cond-ae', conditional_encoder=True), None, None, points)
    with pytest.raises(NotImplementedError):
        cau.interpolate_point_path('points', _Stub('ae'), None, None, points)
    with pytest.raises(ValueError, match='"ch" must be an integer to use crop_kwargs'):
        cau.interpolate_point_path('latents', _Stub('ae'), None, None, points, ch=None,
                                   crop_kwargs={'y_0': 4, 'y_ext': 2, 'x_0': 6, 'x_ext': 3})
    with pytest.raises(AssertionError):
        cau.interpolate_point_path('latents', _Stub('ae'), None, None, points, n_frames=[3])


def test_interpolate_point_path_lists():
    """The lists need no decoder: ``get_reconstruction`` is replaced by frames that name their point and channel."""
    h, w = 8, 12
    calls = []

    def fake(model, inputs, **kw):
        calls.append((len(inputs), kw))
        n = len(inputs)
        return (np.arange(n, dtype=np.float32)[:, None, None, None] + np.array([0.0, 0.5], np.float32)[:, None, None]
                + np.zeros((n, 2, h, w), dtype=np.float32))
    points = np.stack([BASE[0], BASE[1], BASE[0]])
    old = cau.get_reconstruction
    cau.get_reconstruction = fake
    try:
        ims, inputs = cau.interpolate_point_path('latents', _Stub('ae'), None, None, points, n_frames=[2, 3], ch=1)
        want = refs.path_loop(points, [2, 3])
        assert len(ims) == len(inputs) == 7 and calls == [(7, dict(labels=None, apply_inverse_transform=True))]
        for i, (im, vec) in enumerate(zip(ims, inputs)):
            assert im.dtype == np.float32 and im.shape == (h, w) and (im == i + 0.5).all()
            assert vec.dtype == np.float32 and vec.shape == (1, D) and np.array_equal(_bits(vec), _bits(want[i]))
        # a non-int channel: all channels next to each other
        ims, _ = cau.interpolate_point_path('labels', _Stub('ps-vae'), None, None, points, n_frames=1, ch=None,
                                            apply_inverse_transform=False)
        assert calls[-1] == (4, dict(apply_inverse_transform=True))          # labels: always mapped back
        assert ims[2].shape == (h, 2 * w) and (ims[2][:, :w] == 2.0).all() and (ims[2][:, w:] == 2.5).all()
        # a crop: get_crop's float64 window, zero past the right edge
        ims, _ = cau.interpolate_point_path('latents', _Stub('vae'), None, None, points, n_frames=1, ch=0,
                                            crop_kwargs={'y_0': 4, 'y_ext': 2, 'x_0': 10, 'x_ext': 4})
        assert ims[3].dtype == np.float64 and ims[3].shape == (4, 8)
        assert (ims[3][:, :6] == 3.0).all() and not ims[3][:, 6:].any()
    finally:
        cau.get_reconstruction = old


def test_the_names_are_public():
    assert set(bn_eval.__all__) >= {'path_points', 'path_movie_src', 'point_path_movie', 'point_path_movie_device',
                                    'swap_points', 'swap_layout', 'session_swap_movie', 'session_swap_movie_device',
                                    'background_medians'}
    assert set(cau.__all__) >= {'interpolate_point_path', 'make_session_swap_movie'}
    assert 'bn_frame_mosaic_ch_u8' in _hip.SIGNATURES
    assert len(_hip.SIGNATURES['bn_frame_mosaic_ch_u8'][1]) == len(_hip.SIGNATURES['bn_frame_mosaic_u8'][1]) + 1
