"""Latent traversals as uint8 mosaics and movies ("traversals").

1. ``bn_frame_mosaic_u8`` by direct C calls on operands between guard bands, the output pre-filled with a sentinel:
   every comparison is ``torch.equal`` against ``tests/traversal_refs.mosaic_index_rule`` (held against the
   ``get_crop`` + ``np.block`` restatement in tests/test_traversals_cpu.py), fp32 and uint8 frames, the fp32 frames
   with the half-way values, NaN and infinities of ``with_specials``.
2. Whole models (the small golden cases): ``traverse_latents`` against the mosaic of ONE ``get_reconstruction`` call on
   the same table (exactly) and against 255 x the float64 oracle decoder on what the decoder was handed (GREY_TOL of
   tests/test_gpu_reconstructions.py; under the bf16 key 0.5 for the rounding plus 255 x the bound of
   tests/test_gpu_decode_bf16.py, twice the float64 emulation's own distance from the oracle); chunking; movies;
   ``interpolate_1d`` / ``interpolate_2d`` against the per-point loop (``close``'s default 1e-4 of the maximum, the
   tolerance tests/test_gpu_model.py holds x_hat to: a batch of one may take another kernel route).

Batches.  The fp32 decoder's kernels choose their route by the batch they are given, and at 2x128x128 a frame's x_hat
then depends on it in the last bits (measured on psvae_cfg4: 25 frames decoded at once against the same frames in batches
of 1 to 16 differ by up to 2.2e-6, all 25 frames; a batch of 24 has the bits of 25; the 1x32x32 cases do not move for
any batch) -- enough to turn a grey level where x_hat * 255 lies at a half.  That belongs to the existing decoder,
which ``get_reconstruction`` shows in the same way, not to the mosaic.  So every exact comparison here decodes the SAME
batch on both sides: psvae_cfg4 stays at nine frames per decode everywhere, and the chunking case (P = 25 in chunks of
8) runs on the 1x32x32 cases.
"""

import warnings

import numpy as np
import pytest
import torch

from behavenet_amd import _hip
from behavenet_amd.fitting.eval import (get_reconstruction, traversal_movie, traversal_movie_device, traversal_points,
                                        traverse_latents, traverse_latents_device)
from behavenet_amd.plotting import get_crop
from behavenet_amd.plotting.cond_ae_utils import interpolate_1d, interpolate_2d
from tests import traversal_refs as refs
from tests.bf16_decode_cases import apply_gain, span_1_99
from tests.cases import case_data
from tests.recon_u8_refs import with_specials
from tests.test_gpu_decode_bf16 import _emulations
from tests.test_gpu_encode_bf16 import _rel, _small, guarded_u8
from tests.test_gpu_frame_errors import _oracle64
from tests.test_gpu_guard_bands import guarded, _bands_stay_untouched  # noqa: F401
from tests.test_gpu_kernels import close
from tests.test_gpu_reconstructions import GREY_TOL, SENTINEL

pytestmark = pytest.mark.gpu
DEV = 'cuda'
E_ARG, E_SHAPE = -1, -2
REPORT = []     # figures printed at the end of the module (pytest -s)


def teardown_module(module):
    if REPORT:
        print('\n' + '\n'.join(REPORT))


# ------------------------------------------------------------------------------------------ 1: the kernel
def _frames(shape, seed, u8):
    rng = np.random.default_rng(seed)
    if u8:
        return rng.integers(0, 256, size=shape, dtype=np.uint8)
    return with_specials(rng.random(int(np.prod(shape)), dtype=np.float32), seed=seed).reshape(shape)


def _place(frames, offset=0):
    """The frames on the device between guard bands, ``offset`` ELEMENTS off their 16-byte boundary."""
    t = torch.from_numpy(frames).flatten()
    pad = torch.zeros(offset, dtype=t.dtype)
    whole = (guarded_u8 if t.dtype == torch.uint8 else guarded)(torch.cat([pad, t]))
    assert whole.data_ptr() % 16 == 0
    return whole[offset:].view(frames.shape)


def _place_src(src):
    src = torch.from_numpy(np.ascontiguousarray(src, dtype=np.int32))
    d = guarded(torch.zeros(max(src.numel(), 1))).view(torch.int32)[:src.numel()].view(src.shape)
    d.copy_(src)
    return d


def _out(shape, offset=0):
    n = int(np.prod(shape))
    whole = guarded_u8(torch.full((n + 16,), SENTINEL, dtype=torch.uint8))
    assert whole.data_ptr() % 16 == 0
    return whole[offset:offset + n].view(shape), whole


def _call(fd, src_d, ch, crop, out, dims=None, src_shape=None):
    p, c, h, w = dims or fd.shape
    y_min, x_min, hc, wc = (0, 0, h, w) if crop is None else crop
    t, r, cc = src_shape or src_d.shape
    return _hip.load().bn_frame_mosaic_u8(fd.data_ptr(), int(fd.dtype == torch.uint8), p, c, h, w, ch, y_min, x_min, hc,
                                          wc, src_d.data_ptr(), t, r, cc, out.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream)


def _check(frames, src, ch=0, crop=None, in_off=0, out_off=0):
    src = np.asarray(src, dtype=np.int32)
    want = refs.mosaic_index_rule(frames, src, ch, crop)
    out, whole = _out(want.shape, out_off)
    assert _call(_place(frames, in_off), _place_src(src), ch, crop, out) == 0
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.from_numpy(want)), (frames.shape, crop, in_off, out_off)
    n = want.size
    assert bool((whole[:out_off] == SENTINEL).all()) and bool((whole[out_off + n:] == SENTINEL).all())
    return want


CASES = [  # name, (P, C, H, W), ch, crop (y_min, x_min, Hc, Wc), src
    ('smallest', (1, 1, 1, 1), 0, None, [[[0]]]),
    ('element path 5x7', (4, 1, 5, 7), 0, None, [[[0, 1], [2, 3]]]),
    ('unaligned loads', (3, 2, 8, 12), 1, (2, 3, 4, 6), [[[2, 0, 1]]]),
    ('16-byte stores and loads', (2, 1, 16, 32), 0, None, [[[0, 1]]]),
    ('aligned crop', (2, 1, 16, 32), 0, (0, 4, 16, 16), [[[1, 0]]]),
    ('unaligned loads, aligned stores', (2, 1, 16, 32), 0, (0, 5, 16, 16), [[[1, 0]]]),
    ('zero fill', (2, 1, 8, 12), 0, (5, 9, 6, 8), [[[0, 1]]]),
    ('zero fill, a row of 32 past 24 columns', (2, 1, 8, 24), 0, (3, 0, 8, 32), [[[1], [0]]]),
    ('blanks, repeats, permutation', (5, 1, 8, 16), 0, None,
     [[[4, -1, 4], [0, 1, 2]], [[3, 3, 3], [-1, -1, -1]], [[2, 0, 1], [1, 4, 3]]]),
    ('blanks, repeats, permutation, elements', (5, 1, 4, 6), 0, (1, 0, 3, 5),
     [[[4, -1, 4], [0, 1, 2]], [[3, 3, 3], [-1, -1, -1]], [[2, 0, 1], [1, 4, 3]]]),
    ('300 panels of 4x4', (300, 1, 4, 4), 0, None, np.arange(300).reshape(1, 15, 20)),
    ('66,000 output rows', (1, 1, 60, 1), 0, None, np.zeros((1100, 1, 1))),
    ('the workload\'s plane', (4, 2, 128, 128), 1, None, [[[0, 1], [2, 3]]]),
    ('a row wider than a block', (1, 1, 2, 4128), 0, None, [[[0]]]),
]


@pytest.mark.parametrize('u8', [False, True], ids=['fp32', 'u8'])
@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_kernel_against_the_index_rule(case, u8):
    name, shape, ch, crop, src = case
    want = _check(_frames(shape, len(name), u8), src, ch, crop)
    if name.startswith('zero fill'):
        assert not want[:, -1].any() and want.any()          # the bottom row is past the frame


@pytest.mark.parametrize('u8', [False, True], ids=['fp32', 'u8'])
def test_misaligned_pointers_give_the_same_bytes(u8):
    for name, shape, ch, crop, src in (CASES[3], CASES[4], CASES[12], CASES[8]):
        frames = _frames(shape, 7, u8)
        want = _check(frames, src, ch, crop)
        for in_off, out_off in [(1, 0), (0, 1), (1, 1), (3, 5)]:
            assert np.array_equal(_check(frames, src, ch, crop, in_off, out_off), want), (name, in_off, out_off)


def test_empty_result_and_refusals_write_nothing():
    frames = _place(_frames((3, 2, 8, 12), 1, False))
    frames_u8 = _place(_frames((3, 2, 8, 12), 1, True))
    src = _place_src(np.zeros((2, 2, 2)))
    out, whole = _out((2, 16, 24))
    # T = 0, R = 0, Cc = 0: an empty result
    for shape in [(0, 2, 2), (2, 0, 2), (2, 2, 0)]:
        assert _call(frames, src, 0, None, out, src_shape=shape) == 0
    big = 1 << 30
    refused = [
        dict(ch=2), dict(ch=-1),                                             # the channel
        dict(crop=(-1, 0, 4, 4)), dict(crop=(0, -1, 4, 4)),                  # a negative origin
        dict(crop=(0, 0, 0, 4)), dict(crop=(0, 0, 4, 0)), dict(crop=(0, 0, -3, 4)),          # an empty window
        dict(dims=(3, 0, 8, 12)), dict(dims=(3, 2, 0, 12)), dict(dims=(3, 2, 8, 0)), dict(dims=(-1, 2, 8, 12)),
        dict(src_shape=(-1, 2, 2)), dict(src_shape=(2, -2, 2)), dict(src_shape=(2, 2, -2)),
        dict(src_shape=(big, 2, 2)),                                         # T R Hc = 2^34 rows
        dict(crop=(0, 0, 8, big), src_shape=(2, 2, 2)),                      # Cc Wc = 2^31 columns
        dict(crop=(0, 0, big, 12), src_shape=(1, 2, 2)),                     # R Hc = 2^31
        dict(crop=(0, 0, 1, 4096), src_shape=(big, 1, 1)),                   # 2^30 rows of one thread row each: 2^38 threads
    ]
    for kw in refused:
        kw = dict(dict(ch=0, crop=None), **kw)
        assert _call(frames, src, kw['ch'], kw['crop'], out, kw.get('dims'), kw.get('src_shape')) == E_SHAPE, kw
        assert _call(frames_u8, src, kw['ch'], kw['crop'], out, kw.get('dims'), kw.get('src_shape')) == E_SHAPE, kw
    lib, st = _hip.load(), torch.cuda.current_stream().cuda_stream
    args = (3, 2, 8, 12, 0, 0, 0, 8, 12)
    assert lib.bn_frame_mosaic_u8(None, 0, *args, src.data_ptr(), 2, 2, 2, out.data_ptr(), st) == E_ARG
    assert lib.bn_frame_mosaic_u8(frames.data_ptr(), 0, *args, None, 2, 2, 2, out.data_ptr(), st) == E_ARG
    assert lib.bn_frame_mosaic_u8(frames.data_ptr(), 0, *args, src.data_ptr(), 2, 2, 2, None, st) == E_ARG
    assert lib.bn_frame_mosaic_u8(frames.data_ptr() + 2, 0, *args, src.data_ptr(), 2, 2, 2, out.data_ptr(), st) == E_SHAPE
    assert lib.bn_frame_mosaic_u8(frames.data_ptr(), 0, *args, src.data_ptr() + 2, 2, 2, 2, out.data_ptr(), st) == E_SHAPE
    torch.cuda.synchronize()
    assert bool((whole == SENTINEL).all())


def test_wrapper():
    for u8 in (False, True):
        frames = _frames((5, 2, 8, 16), 3, u8)
        src = [[[4, -1, 4], [0, 1, 2]], [[3, 3, 3], [-1, -1, -1]]]
        fd = _place(frames)
        got = _hip.frame_mosaic_u8(fd, src, ch=1, crop=(2, 4, 6, 16))
        assert got.is_cuda and got.dtype == torch.uint8 and got.shape == (2, 12, 48)
        assert np.array_equal(got.cpu().numpy(), refs.mosaic_index_rule(frames, src, 1, (2, 4, 6, 16)))
        grid = _hip.frame_mosaic_u8(fd, src[0])          # (R, Cc): one image
        assert np.array_equal(grid.cpu().numpy(), refs.mosaic_blocks(frames, [src[0]]))
        dev_src = torch.tensor(src, dtype=torch.int32, device=DEV)
        assert torch.equal(_hip.frame_mosaic_u8(fd, dev_src, ch=1, crop=(2, 4, 6, 16)), got)
        with pytest.raises(ValueError, match='src names frame 5 of 5'):
            _hip.frame_mosaic_u8(fd, [[[0, 5]]])
        with pytest.raises(ValueError, match='channel'):
            _hip.frame_mosaic_u8(fd, src, ch=2)
        with pytest.raises(ValueError, match='negative origin'):
            _hip.frame_mosaic_u8(fd, src, crop=(0, -1, 4, 4))
    with pytest.raises(ValueError, match='uint8 or float32'):
        _hip.frame_mosaic_u8(torch.zeros((1, 1, 4, 4), dtype=torch.float64, device=DEV), [[[0]]])


# ------------------------------------------------------------------------------------------ 2: whole models
GOLDENS = ['ae_cfg1', 'vae_cfg1', 'condae_cfg1', 'condvae_cfg1', 'aemsp_cfg1', 'mspsvae_cfg1', 'psvae_cfg4']
BF16_GOLDENS = ['ae_cfg1', 'aemsp_cfg1', 'psvae_cfg4']
N_STEPS = 3          # psvae_cfg4 is 2x128x128: nine frames


class _Case(object):
    """One golden model with a decoder that draws more than a constant grey, one base point and its ranges."""

    def __init__(self, golden, bf16=False):
        self.model, self.meta = _small(golden=golden, n=8)
        self.model.eval()
        apply_gain(self.model.decoding.decoder)
        if bf16:
            self.model.hparams['hip_decode_dtype'] = 'bf16'
        self.cls = self.meta['model_class']
        self.cond = self.cls in ('cond-ae', 'cond-vae')
        self.n_lat = int(self.model.hparams['n_ae_latents'])
        self.dim = tuple(self.meta['dim'])
        rng = np.random.default_rng(len(golden))
        self.base = rng.normal(size=(1, self.n_lat)).astype(np.float32)
        self.mins, self.maxes = -2.0 - rng.random(self.n_lat), 2.0 + rng.random(self.n_lat)
        self.labels = rng.normal(size=(1, self.meta['n_labels'])).astype(np.float32) if self.cond else None
        h, w = self.dim[1:]
        # rows 7 .. h - 1, columns w - 12 .. w + 3: four columns past the right edge
        self.crop_kwargs = {'y_0': h // 2 + 3, 'y_ext': h // 2 - 4, 'x_0': w - 4, 'x_ext': 8}
        self.crop = (7, w - 12, h - 8, 16)

    def labels_for(self, n):
        if not self.cond:
            return None
        return torch.from_numpy(self.labels).to(DEV).expand(n, -1).contiguous()

    def one_call(self, table, as_uint8=False):
        """ONE ``get_reconstruction`` call on the table -> (frames, what the decoder was handed)."""
        seen = []
        hook = self.model.decoding.register_forward_pre_hook(lambda m, a: seen.append(a[0].detach().double().cpu()))
        try:
            frames = get_reconstruction(self.model, table, labels=self.labels_for(len(table)), as_uint8=as_uint8)
        finally:
            hook.remove()
        assert len(seen) == 1
        return frames, seen[0]


_CASES = {}


def _case_of(golden):
    if golden not in _CASES:
        _CASES[golden] = _Case(golden)
    return _CASES[golden]


@pytest.fixture(scope='module', params=GOLDENS)
def case(request):
    return _case_of(request.param)


@pytest.fixture(scope='module', params=[g for g in GOLDENS if g != 'psvae_cfg4'])
def small_case(request):
    """The 1x32x32 cases: what is decoded in other batches on the two sides of an exact comparison."""
    return _case_of(request.param)


def test_fp32_route_is_the_mosaic_of_one_call_and_close_to_the_oracle(case):
    idxs = [case.n_lat - 1, 0, 2]
    for mode, ii, ch, crop_kwargs, crop in [('1d', idxs, 0, None, None), ('2d', idxs[:2], case.dim[0] - 1,
                                                                          case.crop_kwargs, case.crop)]:
        table, (rows, cols) = traversal_points(case.base, case.mins, case.maxes, ii, N_STEPS, mode)
        frames, z_dec = case.one_call(table)
        assert frames.dtype == np.float32 and frames.shape == (rows * cols,) + case.dim
        want = refs.mosaic_index_rule(frames, refs.grid_src(rows, cols), ch, crop)[0]
        with warnings.catch_warnings():
            warnings.simplefilter('error', UserWarning)
            got = traverse_latents(case.model, case.base, case.mins, case.maxes, ii, N_STEPS, mode, labels_0=case.labels,
                                   crop_kwargs=crop_kwargs, ch=ch)
            dev = traverse_latents_device(case.model, case.base, case.mins, case.maxes, ii, N_STEPS, mode,
                                          labels_0=case.labels, crop_kwargs=crop_kwargs, ch=ch)
        hc, wc = case.dim[1:] if crop is None else crop[2:]
        assert got.dtype == np.uint8 and got.shape == (rows * hc, cols * wc)
        assert dev.is_cuda and dev.dtype == torch.uint8 and np.array_equal(dev.cpu().numpy(), got)
        assert np.array_equal(got, want), (case.cls, mode)
        assert np.array_equal(got, refs.mosaic_blocks(frames, refs.grid_src(rows, cols), ch, crop)[0])
        # the float64 oracle decoder on what the decoder was handed
        with torch.no_grad():
            ora = _oracle64(case.meta, case.model).decoding(z_dec, dataset=0).reshape(frames.shape).numpy()
        span = span_1_99(torch.from_numpy(ora))
        exact = _float_mosaic(255.0 * ora, rows, cols, ch, crop)
        err = float(np.abs(got.astype(np.float64) - exact).max())
        REPORT.append('fp32 route %s %s: grey levels %d..%d, oracle 1..99%% span %.3f, max |u8 - 255 oracle| %.4f (bound '
                      '%.4f)' % (case.cls, mode, int(got.min()), int(got.max()), span, err, GREY_TOL))
        assert len(np.unique(got)) > 8, 'the traversal draws an almost constant grey'
        assert err <= GREY_TOL, err


def _float_mosaic(x, rows, cols, ch, crop):
    """float64 frames (P, C, H, W) tiled as the mosaic tiles them, zeros where it zero-fills."""
    y_min, x_min, hc, wc = (0, 0) + x.shape[2:] if crop is None else crop
    return np.block([[refs.crop_window(x[i0 * cols + i1, ch], y_min, x_min, hc, wc) for i1 in range(cols)]
                     for i0 in range(rows)])


@pytest.mark.parametrize('golden', BF16_GOLDENS)
def test_bf16_route_takes_the_last_layers_grey_levels(golden):
    case = _Case(golden, bf16=True)
    idxs = [1, case.n_lat - 1]
    table, (rows, cols) = traversal_points(case.base, case.mins, case.maxes, idxs, N_STEPS, '2d')
    with warnings.catch_warnings():
        warnings.simplefilter('error', UserWarning)          # (an unserved stack would warn and run in fp32)
        u8, z_dec = case.one_call(table, as_uint8=True)
        got = traverse_latents(case.model, case.base, case.mins, case.maxes, idxs, N_STEPS, '2d',
                               crop_kwargs=case.crop_kwargs)
    assert u8.dtype == np.uint8
    assert np.array_equal(got, refs.mosaic_index_rule(u8, refs.grid_src(rows, cols), 0, case.crop)[0])
    case.model.hparams['hip_decode_dtype'] = 'f32'
    f32 = traverse_latents(case.model, case.base, case.mins, case.maxes, idxs, N_STEPS, '2d', crop_kwargs=case.crop_kwargs)
    assert not np.array_equal(got, f32)          # the bf16 code ran
    # the decoder's existing bound (tests/test_gpu_decode_bf16.py): max |x16 - oracle| <= 2 x the float64 emulation's
    # own distance from the oracle, both over max |oracle|; the rounding to grey levels adds 0.5
    ora64 = _oracle64(case.meta, case.model)
    x_e64, _, x_exact = _emulations(case.model.decoding, ora64.decoding, z_dec)
    bound = 0.5 + 255.0 * 2.0 * _rel(x_e64, x_exact) * float(x_exact.abs().max())
    exact = _float_mosaic(255.0 * x_exact.reshape(u8.shape).numpy(), rows, cols, 0, case.crop)
    err = float(np.abs(got.astype(np.float64) - exact).max())
    REPORT.append('bf16 route %s: max |u8 - 255 oracle| %.4f (bound %.4f), %d grey levels at most from the fp32 route, '
                  'oracle 1..99%% span %.3f' % (case.cls, err, bound, int(np.abs(got.astype(int) - f32.astype(int)).max()),
                                                span_1_99(x_exact)))
    assert err <= bound, (err, bound)


def test_chunking_does_not_change_a_byte(small_case):
    case = small_case
    idxs = [0, 1, 2, 3, case.n_lat - 1]          # P = 25
    args = (case.model, case.base, case.mins, case.maxes, idxs, 5, '1d')
    kw = dict(labels_0=case.labels, crop_kwargs=case.crop_kwargs)
    whole = traverse_latents(*args, **kw)
    assert whole.shape == (5 * case.crop[2], 5 * 16)
    assert np.array_equal(traverse_latents(*args, chunk_size=8, **kw), whole)


def test_movie_is_the_1d_traversals_in_time(case):
    if case.dim[1] == 32:
        n_base, n_frames, n_cols = 2, 3, 3
        idxs = [2, 0, case.n_lat - 1, 1]          # four panels in three columns: two rows, two blanks
    else:
        # (2x128x128: nine frames in the movie's decode and in the traversal's, see "Batches" above)
        n_base, n_frames, n_cols = 1, 3, 2
        idxs = [2, 0, case.n_lat - 1]             # three panels in two columns: two rows, one blank
    bases = np.concatenate([case.base, case.base[:, ::-1]], axis=0)[:n_base]
    labels = None
    if case.cond:
        labels = np.concatenate([case.labels, -case.labels], axis=0)[:n_base]
    kw = dict(crop_kwargs=case.crop_kwargs, ch=case.dim[0] - 1)
    movie = traversal_movie(case.model, bases, case.mins, case.maxes, idxs, n_frames, n_cols, labels_0=labels, **kw)
    hc, wc = case.crop[2:]
    assert movie.dtype == np.uint8 and movie.shape == (n_base * n_frames, 2 * hc, n_cols * wc)
    dev = traversal_movie_device(case.model, bases, case.mins, case.maxes, idxs, n_frames, n_cols, labels_0=labels, **kw)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), movie)
    if case.dim[1] == 32:          # (one decode and one launch per chunk: the same bytes)
        assert np.array_equal(traversal_movie(case.model, bases, case.mins, case.maxes, idxs, n_frames, n_cols,
                                              labels_0=labels, chunk_size=4, **kw), movie)
    for b in range(n_base):
        grid = traverse_latents(case.model, bases[b], case.mins, case.maxes, idxs, n_frames, '1d',
                                labels_0=None if labels is None else labels[b:b + 1], **kw)
        for i in range(n_frames):
            frame = movie[b * n_frames + i]
            for k in range(len(idxs)):
                r, c = divmod(k, n_cols)
                assert np.array_equal(frame[r * hc:(r + 1) * hc, c * wc:(c + 1) * wc],
                                      grid[k * hc:(k + 1) * hc, i * wc:(i + 1) * wc]), (b, i, k)
            for k in range(len(idxs), 2 * n_cols):          # the trailing panels are blank
                r, c = divmod(k, n_cols)
                assert not frame[r * hc:(r + 1) * hc, c * wc:(c + 1) * wc].any()
    assert movie[:, :hc].any()
    # the default is the reference's three columns
    three = traversal_movie(case.model, bases, case.mins, case.maxes, idxs, n_frames, 3, labels_0=labels, **kw)
    assert np.array_equal(traversal_movie(case.model, bases, case.mins, case.maxes, idxs, n_frames, labels_0=labels,
                                          **kw), three)


def _assert_lists(case, got, mode, interp_type, idxs, rows, cols, ch, want_frames, want_markers, sampled=False):
    ims, markers, crops = got
    ck = case.crop_kwargs
    assert len(ims) == len(markers) == len(crops) == rows
    for i0 in range(rows):
        assert len(ims[i0]) == len(markers[i0]) == len(crops[i0]) == cols
        for i1 in range(cols):
            im, crop = ims[i0][i1], crops[i0][i1]
            assert isinstance(im, np.ndarray) and im.dtype == np.float32 and im.shape == case.dim[1:]
            assert crop.dtype == np.float64 and crop.shape == (2 * ck['y_ext'], 2 * ck['x_ext'])
            assert float(im.min()) >= 0.0 and float(im.max()) <= 1.0
            if case.dim[0] == 1:          # (the reference crops channel 0)
                assert np.array_equal(crop, get_crop(im, ck['y_0'], ck['y_ext'], ck['x_0'], ck['x_ext']))
            assert not crop[:, -(ck['x_0'] + ck['x_ext'] - case.dim[2]):].any()
    assert np.array_equal(np.array(markers, dtype=np.float64), np.array(want_markers, dtype=np.float64), equal_nan=True)
    if not sampled:
        got_t = torch.from_numpy(np.stack([im for row in ims for im in row]))
        want_t = torch.from_numpy(np.stack([f[ch] for row in want_frames for f in row]))
        close(got_t, want_t, name='%s %s %s' % (case.cls, mode, interp_type))
        # the crops come from channel 0 of the same decode
        want_c = np.stack([refs.get_crop_ref(f[0], ck['y_0'], ck['y_ext'], ck['x_0'], ck['x_ext'])
                           for row in want_frames for f in row])
        close(torch.from_numpy(np.stack([c for row in crops for c in row])), torch.from_numpy(want_c), name='crops')


def test_interpolate_has_the_reference_lists(case):
    ch = case.dim[0] - 1
    labels_sc_0 = np.array([[11.0, 4.0, 9.0, 2.5]])
    origin = (case.crop_kwargs['y_0'] - case.crop_kwargs['y_ext'], case.crop_kwargs['x_0'] - case.crop_kwargs['x_ext'])
    for mode, fn, idxs in [('1d', interpolate_1d, [2, 0, 1]), ('2d', interpolate_2d, [2, 0])]:
        rows, cols = refs.grid_shape(idxs, N_STEPS, mode)
        # latents
        got = fn('latents', case.model, None, case.base, case.labels, labels_sc_0, case.mins, case.maxes, idxs, N_STEPS,
                 crop_type='fixed', crop_kwargs=case.crop_kwargs, marker_idxs=[3, 1], ch=ch)
        want = refs.frames_loop(get_reconstruction, 'latents', mode, case.model, None, case.base, case.labels, case.mins,
                                case.maxes, idxs, N_STEPS, DEV)
        markers = refs.marker_lists('latents', mode, labels_sc_0, idxs, N_STEPS, marker_idxs=[3, 1], origin=origin)
        _assert_lists(case, got, mode, 'latents', idxs, rows, cols, ch, want, markers)
        # labels: of the label-aware classes
        if case.cond:
            ims_0 = case_data(case.meta, device=DEV)['images'][0][:1].float()
            ims_0 = ims_0 / 255 if ims_0.max() > 1 else ims_0
            mins, maxes = case.mins[:4], case.maxes[:4]
        elif case.cls in ('cond-ae-msp', 'ps-vae', 'msps-vae'):
            ims_0, mins, maxes = None, case.mins, case.maxes
        else:
            continue
        mins_sc, maxes_sc = np.array([1.0, 2.0, 0.0, 3.0]), np.array([6.0, 9.0, 7.0, 11.0])
        got = fn('labels', case.model, ims_0, case.base, case.labels, labels_sc_0, mins, maxes, idxs, N_STEPS,
                 crop_type='fixed', mins_sc=mins_sc, maxes_sc=maxes_sc, crop_kwargs=case.crop_kwargs, ch=ch)
        markers = refs.marker_lists('labels', mode, labels_sc_0, idxs, N_STEPS, mins_sc, maxes_sc, origin=origin)
        sampled = case.cls == 'cond-vae'          # (its get_reconstruction samples from images: shape, range, dtype)
        want = None if sampled else refs.frames_loop(get_reconstruction, 'labels', mode, case.model, ims_0, case.base,
                                                     case.labels, mins, maxes, idxs, N_STEPS, DEV)
        _assert_lists(case, got, mode, 'labels', idxs, rows, cols, ch, want, markers, sampled=sampled)
