"""Point-path traversal movies and session-swap movies, end to end on the small golden models.

Everything is byte-exact.  The fp32 decoder's last bits depend on the batch at 2x128x128 (tests/test_gpu_traversals.py,
"Batches"), so every comparison decodes EQUAL batches: the yardstick of a movie is the numpy mosaic
(``tests/point_path_refs.mosaic_channels_rule``) of one ``decode_points_device`` call on the same table with the same
``chunk_size``, and the per-point loop of single-frame ``get_reconstruction`` calls is held to the 1x32x32 cases, whose
bits do not depend on the batch."""

import os
import warnings

import numpy as np
import pytest
import torch

from behavenet_amd.fitting.eval import (background_medians, decode_points_device, export_latents, get_reconstruction,
                                        point_path_movie, point_path_movie_device, session_swap_movie,
                                        session_swap_movie_device)
from behavenet_amd.plotting import get_crop
from behavenet_amd.plotting.cond_ae_utils import interpolate_point_path, make_session_swap_movie
from tests import point_path_refs as refs
from tests.cases import case_data
from tests.golden_utils import make_frames
from tests.recon_u8_refs import quantise_u8
from tests.test_gpu_kernels import close
from tests.test_gpu_ranges import _generator, _model, _pickled
from tests.test_gpu_traversals import BF16_GOLDENS, GOLDENS, _Case, _case_of

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MSP = ('cond-ae-msp', 'ps-vae', 'msps-vae')


@pytest.fixture(scope='module', params=GOLDENS)
def case(request):
    return _case_of(request.param)


@pytest.fixture(scope='module', params=[g for g in GOLDENS if g != 'psvae_cfg4'])
def small_case(request):
    return _case_of(request.param)


def _panels(case, dims):
    return [(d, float(case.mins[d]), float(case.maxes[d])) for d in dims]


def _setup(case):
    """(bases, labels, panels, n_frames, n_buffer_frames, n_cols, order_idxs, chunk_size) of the case's movie."""
    if case.dim[1] == 32:          # two base points, four panels in three columns, reordered: 48 points
        n_base, dims, n_frames, order = 2, [2, 0, case.n_lat - 1, 1], 2, [3, 0, 2, 1]
    else:          # 2x128x128: one base point, three panels in two columns, 12 points
        n_base, dims, n_frames, order = 1, [2, 0, case.n_lat - 1], 1, None
    bases = np.concatenate([case.base, case.base[:, ::-1]], axis=0)[:n_base]
    labels = np.concatenate([case.labels, -case.labels], axis=0)[:n_base] if case.cond else None
    return bases, labels, _panels(case, dims), n_frames, 2, 3 if n_base == 2 else 2, order, 7


def _decoded(case, table, labels, n_base, chunk_size, apply_inverse_transform=True):
    """ONE ``decode_points_device`` call on the table, the labels repeated as the movie repeats them."""
    per_point = None
    if labels is not None:
        per_point = torch.from_numpy(labels).to(DEV).repeat_interleave(len(table) // n_base, dim=0)
    return decode_points_device(case.model, table, per_point, apply_inverse_transform, chunk_size).cpu().numpy()


def test_movie_is_the_mosaic_of_one_decode(case):
    bases, labels, panels, n_frames, n_buf, n_cols, order, chunk = _setup(case)
    n_base, n_steps = len(bases), 2 * (n_frames + 1)
    table = refs.movie_table(bases, panels, n_frames)
    frames = _decoded(case, table, labels, n_base, chunk)
    assert frames.dtype == np.float32 and frames.shape == (n_base * len(panels) * n_steps,) + case.dim
    src = refs.path_movie_src_loop(n_base, len(panels), n_steps, n_buf, n_cols, order)
    n_t = n_base * (n_steps + (n_buf if n_base > 1 else 0))
    assert src.shape == (n_t, 2, n_cols)
    variants = [(0, (0, 1), None, None), (case.dim[0] - 1, (case.dim[0] - 1, 1), case.crop_kwargs, case.crop),
                (None, (0, case.dim[0]), None, None), (None, (0, case.dim[0]), case.crop_kwargs, case.crop)]
    for ch, (ch0, n_ch), crop_kwargs, crop in variants:
        kw = dict(n_frames=n_frames, n_buffer_frames=n_buf, n_cols=n_cols, order_idxs=order, labels_0=labels,
                  crop_kwargs=crop_kwargs, ch=ch, chunk_size=chunk)
        with warnings.catch_warnings():
            warnings.simplefilter('error', UserWarning)
            movie = point_path_movie(case.model, bases, panels, **kw)
            dev = point_path_movie_device(case.model, bases, panels, **kw)
        hc, wc = case.dim[1:] if crop is None else crop[2:]
        assert movie.dtype == np.uint8 and movie.shape == (n_t, 2 * hc, n_cols * n_ch * wc)
        assert dev.is_cuda and dev.dtype == torch.uint8 and np.array_equal(dev.cpu().numpy(), movie)
        assert np.array_equal(movie, refs.mosaic_channels_rule(frames, src, ch0, n_ch, crop)), (case.cls, ch, crop)
        assert len(np.unique(movie)) > 8, 'the movie draws an almost constant grey'
        if n_base > 1:          # the buffer frames after every base point, the last included
            for b in range(n_base):
                assert not movie[b * (n_steps + n_buf) + n_steps:(b + 1) * (n_steps + n_buf)].any()
        # min -> max -> min: the return leg plays the outward leg backwards, up to the rounding of its points
        first = movie[:n_steps].astype(int)
        assert np.abs(first[:n_frames + 1] - first[n_steps - 1:n_frames:-1]).max() <= 1
        assert not np.array_equal(first[0], first[n_frames])
    if case.dim[0] == 2:          # two views: the sub-panels of a panel are the channels of one frame
        both = point_path_movie(case.model, bases, panels, n_frames=n_frames, n_cols=n_cols, ch=None, chunk_size=chunk)
        w = case.dim[2]
        for c in range(2):
            one = point_path_movie(case.model, bases, panels, n_frames=n_frames, n_cols=n_cols, ch=c, chunk_size=chunk)
            for k in range(n_cols):
                assert np.array_equal(both[:, :, (2 * k + c) * w:(2 * k + c + 1) * w], one[:, :, k * w:(k + 1) * w])
    # the defaults are the reference's: ten frames a leg, five buffer frames, three columns
    if case.cls == 'ae':
        default = point_path_movie(case.model, bases, panels[:2])
        assert default.shape == (n_base * (22 + 5), case.dim[1], 3 * case.dim[2])


def _one_point(case, vec, label_row, apply_inverse_transform=True):
    labels = None if label_row is None else torch.from_numpy(label_row[None]).float().to(DEV)
    return get_reconstruction(case.model, np.asarray(vec, dtype=np.float32).reshape(1, -1), labels=labels,
                              apply_inverse_transform=apply_inverse_transform)[0]


def test_movie_is_the_loop_of_single_point_calls(small_case):
    case = small_case
    bases, labels, panels, n_frames, n_buf, n_cols, order, chunk = _setup(case)
    n_steps = 2 * (n_frames + 1)
    table = refs.movie_table(bases, panels, n_frames)
    per = len(panels) * n_steps
    frames = np.stack([_one_point(case, vec, None if labels is None else labels[i // per])
                       for i, vec in enumerate(table)])
    src = refs.path_movie_src_loop(len(bases), len(panels), n_steps, n_buf, n_cols, order)
    want = refs.mosaic_channels_rule(quantise_u8(frames), src, 0, 1, case.crop)
    for chunk_size in (chunk, 200):
        got = point_path_movie(case.model, bases, panels, n_frames, n_buf, n_cols, order, labels, True,
                               case.crop_kwargs, 0, chunk_size)
        assert np.array_equal(got, want), (case.cls, chunk_size)


def test_interpolate_point_path_has_the_reference_lists(small_case):
    case = small_case
    d = case.n_lat - 1
    points = refs.three_point_path(case.base[0], d, case.mins[d], case.maxes[d])
    assert points.dtype == np.float32
    steps = refs.path_loop(points, [2, 3])
    ck = case.crop_kwargs
    kinds = ['latents'] + (['labels'] if case.cls in MSP else [])
    for interp_type in kinds:
        ims, inputs = interpolate_point_path(interp_type, case.model, None, case.labels, points, n_frames=[2, 3])
        crops, _ = interpolate_point_path(interp_type, case.model, None, case.labels, points, n_frames=[2, 3], ch=0,
                                          crop_kwargs=ck)
        wide, _ = interpolate_point_path(interp_type, case.model, None, case.labels, points, n_frames=[2, 3], ch=None)
        assert len(ims) == len(inputs) == len(crops) == len(wide) == 7
        for i in range(7):
            want = _one_point(case, steps[i], None if case.labels is None else case.labels[0])
            assert isinstance(ims[i], np.ndarray) and ims[i].dtype == np.float32 and ims[i].shape == case.dim[1:]
            assert np.array_equal(ims[i], want[0]), (case.cls, interp_type, i)
            assert inputs[i].dtype == np.float32 and inputs[i].shape == (1, case.n_lat)
            assert np.array_equal(inputs[i].view(np.uint32), steps[i].view(np.uint32))
            assert crops[i].dtype == np.float64 and crops[i].shape == (2 * ck['y_ext'], 2 * ck['x_ext'])
            assert np.array_equal(crops[i], get_crop(want[0], ck['y_0'], ck['y_ext'], ck['x_0'], ck['x_ext']))
            assert wide[i].dtype == np.float32 and np.array_equal(wide[i], np.concatenate(list(want), axis=1))
        assert np.array_equal(ims[3], _one_point(case, points[1], None if case.labels is None else case.labels[0])[0])
        assert not np.array_equal(ims[0], ims[3])          # (step 3 starts the second leg: the middle point itself)
    if case.cls in MSP:          # 'latents' without the inverse transform is another picture
        raw, _ = interpolate_point_path('latents', case.model, None, None, points, n_frames=1,
                                        apply_inverse_transform=False)
        assert np.array_equal(raw[2], _one_point(case, points[1], None, apply_inverse_transform=False)[0])
        assert not np.array_equal(raw[2], ims[3])
    if case.cls == 'cond-ae':          # a label path goes with ims_0, repeated, through the whole model
        ims_0 = case_data(case.meta, device=DEV)['images'][0][:1].float()
        ims_0 = ims_0 / 255 if ims_0.max() > 1 else ims_0
        label_points = refs.three_point_path(case.labels[0], 1, -2.0, 2.0)
        ims, inputs = interpolate_point_path('labels', case.model, ims_0, case.labels, label_points, n_frames=2)
        assert len(ims) == 6 and inputs[1].shape == (1, case.labels.shape[1])
        want = [get_reconstruction(case.model, ims_0, labels=torch.from_numpy(v).float().to(DEV))[0, 0]
                for v in refs.path_loop(label_points, 2)]
        # (the encoder sees six frames here and one there: the tolerance tests/test_gpu_traversals.py holds
        # interpolate_1d's label branch to)
        close(torch.from_numpy(np.stack(ims)), torch.from_numpy(np.stack(want)), name='cond-ae label path')


# ------------------------------------------------------------------------------------------ session swaps
def _swap_loop_movie(case, trials, idxs, medians, sess_idx, n_buf, pattern):
    """The host loop: per trial and session one ``get_reconstruction`` call on the swapped latents, quantised, the
    sessions' panels placed by the grid, every channel of a frame side by side, zero frames between the trials."""
    grid = refs.swap_grid_loop(len(medians), sess_idx, pattern)
    c, h, w = case.dim
    out = []
    for i, z in enumerate(trials):
        block = np.zeros((len(z), grid.shape[0] * h, grid.shape[1] * c * w), dtype=np.uint8)
        for s in range(len(medians)):
            swapped = np.copy(z)
            swapped[:, idxs] = medians[s]
            grey = quantise_u8(get_reconstruction(case.model, swapped, apply_inverse_transform=False))
            (r,), (k,) = np.nonzero(grid == s)
            side_by_side = np.concatenate(list(grey.transpose(1, 0, 2, 3)), axis=2)          # (T, H, C W)
            block[:, r * h:(r + 1) * h, k * c * w:(k + 1) * c * w] = side_by_side
        out.append(block)
        if i + 1 < len(trials):
            out.append(np.zeros((n_buf,) + block.shape[1:], dtype=np.uint8))
    return np.concatenate(out, axis=0)


def test_session_swap_movie_is_the_host_loop_over_sessions():
    case = _case_of('mspsvae_cfg1')
    n_labels, n_bg = int(case.model.hparams['n_labels']), int(case.model.hparams['n_background'])
    idxs = np.arange(n_labels, n_labels + n_bg)
    rng = np.random.default_rng(17)
    # two trials of the golden case's frames (tests/test_oracle_golden.py::_msps_case: make_frames, seeds 1 and 2)
    trials = [case.model.get_transformed_latents(torch.from_numpy(make_frames(t, case.dim, seed=1 + i)).to(DEV),
                                                 dataset=0, as_numpy=True) for i, t in enumerate((5, 3))]
    assert [z.shape for z in trials] == [(5, case.n_lat), (3, case.n_lat)] and trials[0].dtype == np.float32
    medians = (2.0 * rng.normal(size=(3, n_bg))).astype(np.float32)
    pattern = np.array([[True, False], [True, True]])
    for pat in (None, pattern):
        want = _swap_loop_movie(case, trials, idxs, medians, 1, 2, pat)
        got = session_swap_movie(case.model, trials, idxs, medians, sess_idx=1, n_buffer_frames=2, layout_pattern=pat)
        rows, cols = (1, 3) if pat is None else (2, 2)
        assert got.dtype == np.uint8 and got.shape == (5 + 2 + 3, rows * case.dim[1], cols * case.dim[0] * case.dim[2])
        assert np.array_equal(got, want), pat
        assert not got[5:7].any() and got[:5].any() and got[7:].any()
        dev = session_swap_movie_device(case.model, trials, idxs, medians, sess_idx=1, n_buffer_frames=2,
                                        layout_pattern=pat, chunk_size=4)          # (chunks: the same bytes)
        assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), got)
    # the sessions' panels differ (the background latents reach the decoder), and sess_idx moves them
    h, w = case.dim[1:]
    first = session_swap_movie(case.model, trials[:1], idxs, medians, sess_idx=1)
    assert not np.array_equal(first[:, :, :w], first[:, :, w:2 * w])
    zero = session_swap_movie(case.model, trials[:1], idxs, medians, sess_idx=0)
    assert np.array_equal(zero[:, :, :w], first[:, :, w:2 * w]) and np.array_equal(zero[:, :, w:2 * w], first[:, :, :w])
    # the consistent alternative maps the supervised block back first: another picture
    back = session_swap_movie(case.model, trials[:1], idxs, medians, sess_idx=1, apply_inverse_transform=True)
    assert back.shape == first.shape and not np.array_equal(back, first)


def test_make_session_swap_movie_on_a_two_session_generator(tmp_path):
    model, meta = _model('mspsvae_cfg1', str(tmp_path))
    n_labels, n_bg = int(model.hparams['n_labels']), int(model.hparams['n_background'])
    gen = _generator(meta, n_sessions=2, n_labels=n_labels)
    idxs = np.arange(n_labels, n_labels + n_bg)
    # the medians are those of the session's exported latents, bit for bit
    medians = background_medians(gen, model, idxs)
    assert medians.dtype == np.float32 and medians.shape == (2, n_bg)
    exported = _pickled(export_latents(gen, model))
    for s in range(2):
        table = np.vstack([l for l in exported[s] if len(l)])
        want = np.nanpercentile(table, 50, axis=0)[idxs]
        assert np.array_equal(medians[s].view(np.uint32), want.astype(np.float32).view(np.uint32)), s
    assert not np.array_equal(medians[0], medians[1])
    # two trials of session 1: one named by its number, one by its place among the test trials
    ds = gen.datasets[1]
    numbers = [int(ds.batch_idxs['train'][0]), int(ds.batch_idxs['test'][0])]
    save_file = os.path.join(str(tmp_path), 'swap.npy')
    movie = make_session_swap_movie(model, gen, n_labels, n_bg, 1, [numbers[0], None], [None, 0], n_buffer_frames=3,
                                    save_file=save_file, max_frames=10)
    latents = []
    for t in numbers:
        ims = torch.from_numpy(ds.images_u8[t][:10]).to(DEV).float().div(255.0)
        latents.append(model.get_transformed_latents(ims, dataset=1, as_numpy=True))
    assert [len(z) for z in latents] == [10, 10]
    want = session_swap_movie(model, latents, idxs, medians, sess_idx=1, n_buffer_frames=3)
    c, h, w = meta['dim']
    assert movie.dtype == np.uint8 and movie.shape == (23, h, 2 * c * w)
    assert np.array_equal(movie, want)
    assert np.array_equal(np.load(save_file), movie)
    assert not movie[10:13].any() and movie[:10].any()
    # trials alone, trial_idxs alone
    by_number = make_session_swap_movie(model, gen, n_labels, n_bg, 1, numbers[1:], max_frames=10)
    by_place = make_session_swap_movie(model, gen, n_labels, n_bg, 1, None, [0], max_frames=10)
    assert np.array_equal(by_number, movie[13:]) and np.array_equal(by_place, by_number)
    with pytest.raises(ValueError, match='exactly one'):
        make_session_swap_movie(model, gen, n_labels, n_bg, 1, [numbers[0]], [0])


# ------------------------------------------------------------------------------------------ bf16
@pytest.mark.parametrize('golden', BF16_GOLDENS)
def test_bf16_route_takes_the_last_layers_grey_levels(golden):
    case = _Case(golden, bf16=True)
    bases, labels, panels, n_frames, n_buf, n_cols, order, _ = _setup(case)
    n_steps = 2 * (n_frames + 1)
    table = refs.movie_table(bases, panels, n_frames)
    assert len(table) <= 200          # one chunk: the decoder sees the batch of the one call below
    kw = dict(n_frames=n_frames, n_buffer_frames=n_buf, n_cols=n_cols, order_idxs=order, crop_kwargs=case.crop_kwargs,
              ch=None)
    with warnings.catch_warnings():
        warnings.simplefilter('error', UserWarning)          # (an unserved stack would warn and run in fp32)
        u8, _ = case.one_call(table, as_uint8=True)
        got = point_path_movie(case.model, bases, panels, **kw)
    assert u8.dtype == np.uint8
    src = refs.path_movie_src_loop(len(bases), len(panels), n_steps, n_buf, n_cols, order)
    assert np.array_equal(got, refs.mosaic_channels_rule(u8, src, 0, case.dim[0], case.crop))
    case.model.hparams['hip_decode_dtype'] = 'f32'
    assert not np.array_equal(got, point_path_movie(case.model, bases, panels, **kw))          # the bf16 code ran
