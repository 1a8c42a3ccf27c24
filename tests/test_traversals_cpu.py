"""Latent traversals, the host side (no GPU): the yardstick of tests/traversal_refs.py against itself, then
``fitting.eval.traversal_points``, ``plotting.get_crop``, the marker lists of ``plotting.cond_ae_utils`` and the
argument errors that are raised before anything reaches the device."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from behavenet_amd import _hip
from behavenet_amd.fitting import eval as bn_eval
from behavenet_amd.fitting.eval import movie_src, traversal_points, traverse_latents, traversal_movie
from behavenet_amd.plotting import get_crop
from behavenet_amd.plotting import cond_ae_utils as cau
from tests import traversal_refs as refs
from tests.recon_u8_refs import with_specials

D = 9
RNG = np.random.default_rng(5)
BASE = RNG.normal(size=(1, D)).astype(np.float32)
MINS, MAXES = RNG.uniform(-3, -1, size=D), RNG.uniform(1, 3, size=D)
SWEPT = {1: [4], 2: [7, 2], 5: [0, 8, 3, 5, 1]}


def _tables():
    for mode in ('1d', '2d'):
        for n_dims, idxs in SWEPT.items():
            if mode == '2d' and n_dims != 2:
                continue
            for n_frames in (1, 2, 7):
                for base in (BASE, BASE.astype(np.float64)):
                    yield mode, idxs, n_frames, base


def test_the_two_point_tables_agree_and_traversal_points_is_them():
    seen = 0
    for mode, idxs, n_frames, base in _tables():
        loop, shape_l = refs.points_loop(base, MINS, MAXES, idxs, n_frames, mode)
        closed, shape_c = refs.points_closed(base, MINS, MAXES, idxs, n_frames, mode)
        got, shape = traversal_points(base, MINS, MAXES, idxs, n_frames, mode)
        assert shape_l == shape_c == shape == refs.grid_shape(idxs, n_frames, mode)
        assert loop.dtype == closed.dtype == got.dtype == np.float32
        assert loop.shape == (shape[0] * shape[1], D)
        assert np.array_equal(loop.view(np.uint32), closed.view(np.uint32)), (mode, idxs, n_frames)
        assert np.array_equal(got.view(np.uint32), loop.view(np.uint32)), (mode, idxs, n_frames)
        assert np.array_equal(traversal_points(base[0], MINS, MAXES, idxs, n_frames, mode)[0], got)
        seen += 1
    assert seen == 2 * (3 * 3 + 3)
    # the end points are the percentiles themselves, and nothing but the swept columns moves
    got, _ = traversal_points(BASE, MINS, MAXES, [7, 2], 7, '2d')
    assert got[0, 7] == np.float32(MINS[7]) and got[-1, 2] == np.float32(MAXES[2])
    rest = [d for d in range(D) if d not in (7, 2)]
    assert np.array_equal(got[:, rest], np.repeat(BASE[:, rest], 49, axis=0))


def _frames(p, c, h, w, seed, u8=False):
    rng = np.random.default_rng(seed)
    if u8:
        return rng.integers(0, 256, size=(p, c, h, w), dtype=np.uint8)
    return with_specials(rng.random(p * c * h * w, dtype=np.float32), seed=seed).reshape(p, c, h, w)


MOSAICS = [  # (P, C, H, W), ch, crop, src
    ((1, 1, 1, 1), 0, None, [[[0]]]),
    ((4, 1, 5, 7), 0, None, [[[0, 1], [2, 3]]]),
    ((3, 2, 8, 12), 1, (2, 3, 4, 6), [[[2, 0, 1]]]),
    ((3, 2, 8, 12), 0, (5, 9, 6, 8), [[[0, 1, 2]], [[2, -1, 0]]]),
    ((5, 1, 4, 6), 0, (1, 0, 3, 5), [[[4, -1, 4], [0, 1, 2]], [[3, 3, 3], [-1, -1, -1]], [[2, 0, 1], [1, 4, 3]]]),
    ((2, 1, 6, 4), 0, (6, 4, 2, 2), [[[0, 1]]]),          # a window wholly outside: zeros
]


@pytest.mark.parametrize('u8', [False, True], ids=['fp32', 'u8'])
def test_the_two_mosaics_agree(u8):
    for shape, ch, crop, src in MOSAICS:
        frames = _frames(*shape, seed=sum(shape), u8=u8)
        a, b = refs.mosaic_blocks(frames, src, ch, crop), refs.mosaic_index_rule(frames, src, ch, crop)
        hc, wc = (shape[2], shape[3]) if crop is None else crop[2:]
        assert a.dtype == b.dtype == np.uint8
        assert a.shape == b.shape == (len(src), len(src[0]) * hc, len(src[0][0]) * wc)
        assert np.array_equal(a, b), (shape, crop)
    assert int(refs.mosaic_index_rule(_frames(2, 1, 6, 4, 3, u8), [[[0, 1]]], 0, (6, 4, 2, 2)).max()) == 0


def test_source_tables():
    assert np.array_equal(refs.grid_src(2, 3)[0], [[0, 1, 2], [3, 4, 5]])
    for n_base, n_dims, n_frames, n_cols in [(1, 1, 1, 1), (2, 4, 3, 3), (5, 16, 30, 3), (3, 5, 4, 5), (2, 3, 2, 7)]:
        want = refs.movie_src_ref(n_base, n_dims, n_frames, n_cols)
        got = movie_src(n_base, n_dims, n_frames, n_cols)
        assert got.dtype == np.int32 and np.array_equal(got, want)
        assert int((want >= 0).sum()) == n_base * n_dims * n_frames
        if n_base * n_frames > 2:          # a chunk of time is a slice of the whole
            assert np.array_equal(movie_src(n_base, n_dims, n_frames, n_cols, 1, 3), want[1:3])


def test_get_crop_is_the_restatement():
    im = np.random.default_rng(2).random((9, 13)).astype(np.float32)
    for y_0, y_ext, x_0, x_ext in [(4, 2, 6, 3), (4, 4, 6, 6), (7, 3, 11, 4), (8, 1, 12, 1), (5, 5, 7, 7)]:
        want = refs.get_crop_ref(im, y_0, y_ext, x_0, x_ext)
        got = get_crop(im, y_0, y_ext, x_0, x_ext)
        assert got.dtype == np.float64 and got.shape == (2 * y_ext, 2 * x_ext)
        assert np.array_equal(got, want)
        assert np.array_equal(got, refs.crop_window(im, y_0 - y_ext, x_0 - x_ext, 2 * y_ext, 2 * x_ext))
    past = get_crop(im, 7, 3, 11, 4)          # rows 4..9 and columns 7..14 of a 9 x 13 image
    assert np.array_equal(past[:5, :6], im[4:, 7:]) and not past[5:].any() and not past[:, 6:].any()
    with pytest.raises(ValueError, match='outside'):
        get_crop(im, 1, 2, 6, 3)


class _Stub(object):
    """What the host-side checks read of a model."""

    def __init__(self, model_class, dim=(2, 8, 12)):
        self.hparams = {'model_class': model_class, 'n_input_channels': dim[0], 'y_pixels': dim[1], 'x_pixels': dim[2]}

    def parameters(self):
        raise AssertionError('the device was reached')

    def eval(self):
        raise AssertionError('the device was reached')


def test_marker_lists():
    """Markers need no reconstruction: ``get_reconstruction`` is replaced by zeros."""
    n_frames, h, w = 3, 8, 12
    calls = []

    def fake(model, inputs, **kw):
        calls.append(len(inputs))
        return np.zeros((len(inputs), 2, h, w), dtype=np.float32)
    labels_1d = np.array([[3.5, 6.0, 2.25, 7.0]])
    maps = refs.one_hot_maps([9, 2], [5, 1], h, w)          # x 9, 2 and y 5, 1 -> [[9, 2, 5, 1]]
    assert np.array_equal(cau._get_updated_scaled_labels(maps), [[9, 2, 5, 1]])
    assert cau._get_updated_scaled_labels(None) is None
    assert np.array_equal(cau._get_updated_scaled_labels(labels_1d, 2, 0.5), [[3.5, 6.0, 0.5, 7.0]])
    assert np.array_equal(cau._get_updated_scaled_labels(labels_1d, [0, 3], [1.0, 2.0]), [[1.0, 6.0, 2.25, 2.0]])
    assert labels_1d[0, 2] == 2.25          # a copy
    crop_kwargs = {'y_0': 4, 'y_ext': 2, 'x_0': 7, 'x_ext': 3}
    mins_sc, maxes_sc = np.array([1.0, 2.0, 0.0, 3.0]), np.array([6.0, 9.0, 7.0, 11.0])
    old = cau.get_reconstruction
    cau.get_reconstruction = fake
    try:
        model = _Stub('ae')
        for mode, fn, idxs in [('1d', cau.interpolate_1d, [2, 0, 3]), ('2d', cau.interpolate_2d, [2, 0])]:
            rows, cols = refs.grid_shape(idxs, n_frames, mode)
            for labels_sc_0, marker_idxs in [(labels_1d, [1, 3]), (maps, [2, 0]), (None, None)]:
                for crop_type, origin in [(None, (0, 0)), ('fixed', (2, 4))]:
                    ims, markers, crops = fn('latents', model, None, BASE, None, labels_sc_0, MINS, MAXES, idxs,
                                             n_frames, crop_type=crop_type, crop_kwargs=crop_kwargs,
                                             marker_idxs=marker_idxs)
                    want = refs.marker_lists('latents', mode, labels_sc_0, idxs, n_frames, marker_idxs=marker_idxs,
                                             origin=origin)
                    assert len(ims) == len(markers) == len(crops) == rows and len(markers[0]) == cols
                    assert np.array_equal(np.array(markers, dtype=np.float64), np.array(want, dtype=np.float64),
                                          equal_nan=True)
                    if labels_sc_0 is None:
                        assert np.isnan(np.array(markers)).all()
                    assert ims[0][0].dtype == np.float32 and ims[0][0].shape == (h, w)
                    if crop_type:
                        assert crops[0][0].dtype == np.float64 and crops[0][0].shape == (4, 6)
                    else:
                        assert crops[0][0] == []
            # labels of a ps-vae: the latents change, the markers follow the scaled range
            ims, markers, _ = fn('labels', _Stub('ps-vae'), None, BASE, None, labels_1d, MINS, MAXES, idxs, n_frames,
                                 crop_type='fixed', mins_sc=mins_sc, maxes_sc=maxes_sc, crop_kwargs=crop_kwargs)
            want = refs.marker_lists('labels', mode, labels_1d, idxs, n_frames, mins_sc, maxes_sc, origin=(2, 4))
            assert np.array_equal(np.array(markers), np.array(want))
        assert set(calls) == {9} and len(calls) == 2 * (3 * 2 + 1)          # ONE batched call per traversal
    finally:
        cau.get_reconstruction = old


def test_argument_errors_are_raised_on_the_host():
    with pytest.raises(ValueError, match='exactly two'):
        traversal_points(BASE, MINS, MAXES, [0, 1, 2], 3, '2d')
    with pytest.raises(ValueError, match='mode'):
        traversal_points(BASE, MINS, MAXES, [0, 1], 3, '3d')
    with pytest.raises(ValueError, match='dimension 9'):
        traversal_points(BASE, MINS, MAXES, [9], 3, '1d')
    with pytest.raises(ValueError, match='n_frames'):
        traversal_points(BASE, MINS, MAXES, [1], 0, '1d')
    # the mosaic's arguments
    assert _hip.check_mosaic_args((3, 2, 8, 12), 1, None) == (0, 0, 8, 12)
    assert _hip.check_mosaic_args((3, 2, 8, 12), 0, (5, 9, 6, 8)) == (5, 9, 6, 8)
    for ch, crop, what in [(2, None, 'channel'), (-1, None, 'channel'), (0, (-1, 0, 4, 4), 'negative origin'),
                           (0, (0, -2, 4, 4), 'negative origin'), (0, (0, 0, 0, 4), 'crop window'),
                           (0, (0, 0, 4, -4), 'crop window')]:
        with pytest.raises(ValueError, match=what):
            _hip.check_mosaic_args((3, 2, 8, 12), ch, crop)
    src = _hip.check_mosaic_src([[0, 2], [-1, -7]], 3)
    assert src.dtype == np.int32 and np.array_equal(src, [[[0, 2], [-1, -1]]])
    with pytest.raises(ValueError, match='frame 3 of 3'):
        _hip.check_mosaic_src([[0, 3]], 3)
    with pytest.raises(ValueError, match='src'):
        _hip.check_mosaic_src([0, 1], 3)
    with pytest.raises(ValueError, match='src names'):          # before any upload, whatever the frames are
        _hip.frame_mosaic_u8(torch.zeros((2, 1, 4, 4)), [[[0, 2]]])
    # the public functions refuse before they decode (the stub fails on any use of the model)
    model = _Stub('ae')
    with pytest.raises(ValueError, match='negative origin'):
        traverse_latents(model, BASE, MINS, MAXES, [0, 1], 3, crop_kwargs={'y_0': 1, 'y_ext': 2, 'x_0': 6, 'x_ext': 3})
    with pytest.raises(ValueError, match='channel'):
        traverse_latents(model, BASE, MINS, MAXES, [0, 1], 3, ch=2)
    with pytest.raises(ValueError, match='exactly two'):
        traverse_latents(model, BASE, MINS, MAXES, [0, 1, 2], 3, mode='2d')
    with pytest.raises(ValueError, match='channel'):
        traversal_movie(model, np.repeat(BASE, 2, axis=0), MINS, MAXES, [0, 1], 3, ch=5)
    # the reference-signature entry points
    maps = refs.one_hot_maps([9, 2], [5, 1], 8, 12)
    sc = dict(mins_sc=np.zeros(D), maxes_sc=np.ones(D))
    for cls in ('cond-ae', 'cond-vae'):
        for fn, idxs in [(cau.interpolate_1d, [0, 1, 2]), (cau.interpolate_2d, [0, 1])]:
            with pytest.raises(NotImplementedError, match='conditional encoder'):
                fn('labels', _Stub(cls), None, BASE, BASE[:, :4], maps, MINS, MAXES, idxs, 3, **sc)
    for fn in (cau.interpolate_1d, cau.interpolate_2d):
        with pytest.raises(NotImplementedError, match='mins_sc'):
            fn('labels', _Stub('ps-vae'), None, BASE, None, BASE, MINS, MAXES, [0, 1], 3)
        with pytest.raises(NotImplementedError):
            fn('points', _Stub('ae'), None, BASE, None, None, MINS, MAXES, [0, 1], 3)
    with pytest.raises(AssertionError):
        cau.interpolate_2d('latents', _Stub('ae'), None, BASE, None, None, MINS, MAXES, [0, 1, 2], 3)


def test_nothing_imports_matplotlib():
    code = ('import sys; import behavenet_amd.plotting.cond_ae_utils, behavenet_amd.fitting.eval; '
            'sys.exit(int("matplotlib" in sys.modules))')
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert subprocess.run([sys.executable, '-c', code], cwd=repo).returncode == 0
    assert set(bn_eval.__all__) >= {'traversal_points', 'traverse_latents', 'traverse_latents_device',
                                    'traversal_movie', 'traversal_movie_device'}
