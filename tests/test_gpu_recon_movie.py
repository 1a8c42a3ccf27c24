"""Reconstruction movies: original | reconstruction | residual as uint8 strips (DESIGN.md section 4,
"reconstruction movies").

1. ``bn_recon_panels_u8`` by direct C calls on operands between guard bands, the output pre-filled with a sentinel:
   every comparison is ``torch.equal`` against ``tests/recon_movie_refs.strip_index_rule`` (held against the
   whole-array restatement in tests/test_recon_movie_cpu.py) over {orig uint8, fp32} x {recon fp32, uint8} x {no mask,
   one mask, per-frame masks}, the fp32 operands with the half-way values, NaN and infinities of ``with_specials``;
   operands and output off their 16-byte boundaries; one row of a two-row movie; the contraction probes, on which a
   kernel that fuses ``o * mask - r`` gives another grey level.
2. Whole models (the small golden cases of tests/test_gpu_traversals.py): ``reconstruction_movie`` against the
   yardstick fed the stored frames and the fp32 ``x_hat`` of ``model(x)[0]`` -- or, under the bf16 key, the uint8
   levels of ``reconstruct_trial`` -- and ``make_ae_reconstruction_movie`` on the synthetic generator.

Batches.  The fp32 decoder's last bits depend on the batch it is given at 2x128x128 (the docstring of
tests/test_gpu_traversals.py), so every exact comparison decodes the SAME batch on both sides: ``x_hat`` comes from
``model(x[beg:end])`` on the movie's own chunks, and the cases that compare different batches (``max_frames``) run at
1x32x32, where the bits do not move.
"""

import os
import warnings

import numpy as np
import pytest
import torch

from behavenet_amd import _hip
from behavenet_amd.data.data_generator import SyntheticSession, SyntheticSessionsGenerator
from behavenet_amd.fitting.eval import (reconstruct_trial, reconstruction_movie, reconstruction_movie_device)
from behavenet_amd.plotting.ae_utils import make_ae_reconstruction_movie
from tests import recon_movie_refs as refs
from tests.bf16_decode_cases import apply_gain
from tests.test_gpu_encode_bf16 import _frames, _small, guarded_u8
from tests.test_gpu_guard_bands import guarded, _bands_stay_untouched  # noqa: F401
from tests.test_gpu_reconstructions import SENTINEL
from tests.test_recon_movie_cpu import probe_case

pytestmark = pytest.mark.gpu
DEV = 'cuda'
E_ARG, E_SHAPE = -1, -2


# ------------------------------------------------------------------------------------------ 1: the kernel
def _place(arr, offset=0):
    """A numpy operand on the device between guard bands, ``offset`` ELEMENTS off its 16-byte boundary."""
    t = torch.from_numpy(np.ascontiguousarray(arr)).flatten()
    whole = (guarded_u8 if t.dtype == torch.uint8 else guarded)(torch.cat([torch.zeros(offset, dtype=t.dtype), t]))
    assert whole.data_ptr() % 16 == 0
    return whole[offset:].view(arr.shape)


def _out(nbytes, offset=0):
    """``nbytes`` sentinel bytes on the device, ``offset`` bytes off a 16-byte boundary, inside a guarded buffer with
    16 bytes of slack -> (the bytes, the whole buffer)."""
    whole = guarded_u8(torch.full((nbytes + 16,), SENTINEL, dtype=torch.uint8))
    assert whole.data_ptr() % 16 == 0
    return whole[offset:offset + nbytes], whole


def _call(orig, recon, mask, out, show_orig=1, dims=None, stride=None, mask_per_frame=None):
    n, c, h, w = dims or orig.shape
    per_frame = int(mask is not None and mask.dim() == 4) if mask_per_frame is None else mask_per_frame
    return _hip.load().bn_recon_panels_u8(
        orig.data_ptr(), int(orig.dtype == torch.uint8), recon.data_ptr(), int(recon.dtype == torch.uint8),
        None if mask is None else mask.data_ptr(), per_frame, n, c, h, w, show_orig, out.data_ptr(),
        3 * c * h * w if stride is None else stride, torch.cuda.current_stream().cuda_stream)


def _check(orig, recon, mask, show_orig=True, in_off=0, out_off=0):
    want = refs.strip_index_rule(orig, recon, mask, show_orig)
    out, whole = _out(want.size, out_off)
    od, rd = _place(orig, in_off), _place(recon, in_off)
    md = None if mask is None else _place(mask, in_off)
    assert _call(od, rd, md, out, int(show_orig)) == 0
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().view(want.shape), torch.from_numpy(want)), (orig.shape, in_off, out_off)
    assert bool((whole[:out_off] == SENTINEL).all()) and bool((whole[out_off + want.size:] == SENTINEL).all())
    return want


@pytest.mark.parametrize('mask_form', refs.MASK_FORMS)
@pytest.mark.parametrize('recon_u8', [False, True], ids=['recon-fp32', 'recon-u8'])
@pytest.mark.parametrize('orig_u8', [False, True], ids=['orig-fp32', 'orig-u8'])
def test_kernel_against_the_index_rule(orig_u8, recon_u8, mask_form):
    for shape in refs.SHAPES:
        orig, recon, mask = refs.operands(shape, sum(shape), orig_u8, recon_u8, mask_form)
        _check(orig, recon, mask)
    # operands 1 and 4 elements off their 16-byte boundary, the output 1 byte off: the same bytes
    shape = (2, 1, 16, 16)
    orig, recon, mask = refs.operands(shape, sum(shape), orig_u8, recon_u8, mask_form)
    want = _check(orig, recon, mask)
    for in_off, out_off in [(1, 0), (4, 0), (0, 1), (4, 1)]:
        assert np.array_equal(_check(orig, recon, mask, in_off=in_off, out_off=out_off), want)
    assert np.array_equal(_check(orig, recon, mask, show_orig=False)[:, :, 16:], want[:, :, 16:])


@pytest.mark.parametrize('mask_form', refs.MASK_FORMS)
@pytest.mark.parametrize('recon_u8', [False, True], ids=['recon-fp32', 'recon-u8'])
@pytest.mark.parametrize('orig_u8', [False, True], ids=['orig-fp32', 'orig-u8'])
def test_one_row_of_a_two_row_movie(orig_u8, recon_u8, mask_form):
    shape = (5, 1, 8, 16)
    n, c, h, w = shape
    orig, recon, mask = refs.operands(shape, 21, orig_u8, recon_u8, mask_form)
    strip = 3 * c * h * w
    want = refs.into_row(refs.strip_index_rule(orig, recon, mask, show_orig=False), 1, 2, SENTINEL)
    out, whole = _out(n * 2 * strip)
    md = None if mask is None else _place(mask)
    assert _call(_place(orig), _place(recon), md, out[strip:], 0, stride=2 * strip) == 0
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().view(want.shape), torch.from_numpy(want))          # (row 0 is sentinel still)
    assert not want[:, h:, :c * w].any() and bool((whole[n * 2 * strip:] == SENTINEL).all())


def test_the_product_does_not_contract():
    o_u8, m, r = refs.contraction_probes(1)
    orig, recon, mask = probe_case(o_u8, m, r)
    want = _check(orig, recon, mask)
    o = o_u8.astype(np.float32) / np.float32(255)
    fused = (o.astype(np.float64) * m - r.astype(np.float64)).astype(np.float32)
    from tests.recon_u8_refs import quantise_u8
    assert not (want[0].reshape(8, 3, 16)[:, 2].reshape(-1)[:64] == quantise_u8(np.float32(0.5) + fused)).any()
    # one mask for all frames takes the same arithmetic
    _check(orig, recon, mask[0])


def test_empty_result_and_refusals_write_nothing():
    shape = (3, 2, 8, 12)
    n, c, h, w = shape
    orig, recon, mask = (_place(a) for a in refs.operands(shape, 1, False, False, 'per-frame'))
    orig_u8, recon_u8, _ = (None if a is None else _place(a) for a in refs.operands(shape, 1, True, True, 'none'))
    out, whole = _out(3 * n * c * h * w)
    assert _call(orig, recon, mask, out, dims=(0, c, h, w)) == 0          # N = 0: an empty movie
    assert _call(orig_u8, recon_u8, None, out, dims=(0, c, h, w)) == 0
    big = 1 << 30
    refused = [
        dict(dims=(-1, c, h, w)), dict(dims=(n, 0, h, w)), dict(dims=(n, c, 0, w)), dict(dims=(n, c, h, 0)),
        dict(dims=(n, -2, h, w)), dict(dims=(n, c, -8, w)), dict(dims=(n, c, h, -12)),
        dict(stride=3 * c * h * w - 1), dict(stride=0),                     # a stride below 3 C H W
        dict(dims=(big, c, h, w), stride=3 * c * h * w),                    # N H = 2^33 rows
        dict(dims=(n, c, 1, big), stride=3 * c * big),                      # 3 C W = 3 * 2^31 columns
        dict(dims=(n, 1, 1 << 16, 1 << 15), stride=3 << 31),                # C H W = 2^31 elements in a frame
    ]
    for kw in refused:
        assert _call(orig, recon, mask, out, **kw) == E_SHAPE, kw
        assert _call(orig_u8, recon_u8, None, out, **kw) == E_SHAPE, kw
    lib, st = _hip.load(), torch.cuda.current_stream().cuda_stream
    args = (n, c, h, w, 1)
    stride = 3 * c * h * w
    po, pr, pm, pout = orig.data_ptr(), recon.data_ptr(), mask.data_ptr(), out.data_ptr()
    assert lib.bn_recon_panels_u8(None, 0, pr, 0, pm, 1, *args, pout, stride, st) == E_ARG
    assert lib.bn_recon_panels_u8(po, 0, None, 0, pm, 1, *args, pout, stride, st) == E_ARG
    assert lib.bn_recon_panels_u8(po, 0, pr, 0, pm, 1, *args, None, stride, st) == E_ARG
    # fp32 operands off a 4-byte boundary cannot be read at all
    assert lib.bn_recon_panels_u8(po + 2, 0, pr, 0, pm, 1, *args, pout, stride, st) == E_SHAPE
    assert lib.bn_recon_panels_u8(po, 0, pr + 1, 0, pm, 1, *args, pout, stride, st) == E_SHAPE
    assert lib.bn_recon_panels_u8(po, 0, pr, 0, pm + 2, 1, *args, pout, stride, st) == E_SHAPE
    torch.cuda.synchronize()
    assert bool((whole == SENTINEL).all())


def test_wrapper():
    shape = (5, 2, 8, 16)
    n, c, h, w = shape
    for orig_u8, recon_u8, mask_form in [(True, False, 'one'), (False, True, 'per-frame'), (True, True, 'none')]:
        orig, recon, mask = refs.operands(shape, 9, orig_u8, recon_u8, mask_form)
        od, rd = _place(orig), _place(recon)
        md = None if mask is None else _place(mask)
        got = _hip.recon_panels_u8(od, rd, md)
        assert got.is_cuda and got.dtype == torch.uint8 and got.shape == (n, h, 3 * c * w)
        top = refs.strip_index_rule(orig, recon, mask)
        assert np.array_equal(got.cpu().numpy(), top)
        # a second row into the same movie: a blank first panel, the first row left alone
        movie = torch.full((n, 2 * h, 3 * c * w), SENTINEL, dtype=torch.uint8, device=DEV)
        assert _hip.recon_panels_u8(od, rd, md, out=movie, row=0, n_rows=2) is movie
        assert bool((movie[:, h:] == SENTINEL).all())
        _hip.recon_panels_u8(od, od, md, show_orig=False, out=movie, row=1, n_rows=2)
        bottom = refs.strip_index_rule(orig, orig, mask, show_orig=False)
        assert np.array_equal(movie.cpu().numpy(), np.concatenate([top, bottom], axis=1))
    with pytest.raises(ValueError, match='on the GPU'):
        _hip.recon_panels_u8(od, rd.cpu())
    with pytest.raises(ValueError, match='on the GPU'):
        _hip.recon_panels_u8(od, rd, out=torch.zeros((n, h, 3 * c * w), dtype=torch.uint8))


# ------------------------------------------------------------------------------------------ 2: whole models
class _Case(object):
    """One golden model with a decoder that draws more than a constant grey, and a trial of stored uint8 frames."""

    def __init__(self, golden, n, bf16=False, gain=True):
        self.model, self.meta = _small(golden=golden, n=n)
        self.model.eval()
        if gain:
            apply_gain(self.model.decoding.decoder)
        if bf16:
            self.model.hparams['hip_decode_dtype'] = 'bf16'
        self.cls = self.meta['model_class']
        self.dim = tuple(self.meta['dim'])
        self.frames = _frames(n, self.dim, len(golden), smooth=True)
        self.xd = self.frames.to(DEV)
        g = torch.Generator().manual_seed(n)
        self.labels = None
        if self.cls in ('cond-ae', 'cond-vae'):
            self.labels = torch.randn((n, self.meta['n_labels']), generator=g).to(DEV)
        self.one_mask = (torch.rand(self.dim, generator=g) > 0.3).float()
        self.frame_masks = torch.rand((n,) + self.dim, generator=g) * (torch.rand((n,) + self.dim, generator=g) > 0.3)

    def kwargs(self, beg, end):
        kw = {'dataset': 0}
        if self.cls in ('vae', 'beta-tcvae', 'ps-vae', 'msps-vae', 'cond-vae'):
            kw['use_mean'] = True
        if self.labels is not None:
            kw.update(labels=self.labels[beg:end], labels_2d=None)
        return kw

    def x_hat(self, chunk_size=200, model=None, n=None):
        """The fp32 reconstruction of ``model(x)[0]`` on the movie's own chunks, on the host."""
        n = self.xd.shape[0] if n is None else n
        model = self.model if model is None else model
        # (a linear model takes float frames: the conversion reconstruction_movie makes for it)
        x = self.xd if model.hparams.get('model_type', 'conv') == 'conv' else _hip.u8_to_unit_float(self.xd)
        with torch.no_grad():
            parts = [model(x[b:min(b + chunk_size, n)], **self.kwargs(b, min(b + chunk_size, n)))[0]
                     .reshape((-1,) + self.dim) for b in range(0, n, chunk_size)]
        return torch.cat(parts).cpu().numpy()


def _panels(movie, c, w, row=0, h=None):
    h = movie.shape[1] if h is None else h
    rows = movie[:, row * h:(row + 1) * h]
    return [rows[:, :, p * c * w:(p + 1) * c * w] for p in range(3)]


@pytest.mark.parametrize('golden', ['ae_cfg1', 'vae_cfg1', 'aemsp_cfg1', 'psvae_cfg4'])
def test_movie_of_stored_frames(golden):
    case = _Case(golden, 9)
    c, h, w = case.dim
    frames = case.frames.numpy()
    x_hat = case.x_hat()
    assert x_hat.dtype == np.float32
    recon = reconstruct_trial(case.model, case.xd, 0, chunk_size=200)
    for masks in (None, case.one_mask, case.frame_masks):
        with warnings.catch_warnings():
            warnings.simplefilter('error', UserWarning)
            movie = reconstruction_movie(case.model, case.xd, 0, masks=None if masks is None else masks.to(DEV))
        assert movie.dtype == np.uint8 and movie.shape == (9, h, 3 * c * w)
        m = None if masks is None else masks.numpy()
        assert np.array_equal(movie, refs.strip_index_rule(frames, x_hat, m))
        p0, p1, p2 = _panels(movie, c, w)
        if masks is None:          # the stored bytes themselves
            assert np.array_equal(p0, np.concatenate([frames[:, k] for k in range(c)], axis=2))
        assert np.array_equal(p1, np.concatenate([recon[:, k] for k in range(c)], axis=2))
        assert len(np.unique(p1)) > 8 and len(np.unique(p2)) > 8, 'an almost constant grey'
    dev = reconstruction_movie_device(case.model, case.xd, 0, masks=case.frame_masks.to(DEV))
    assert dev.is_cuda and dev.dtype == torch.uint8 and np.array_equal(dev.cpu().numpy(), movie)
    # fp32 frames of the same values give the same movie but for the first panel's route
    xf = (case.xd.float() / 255).contiguous()
    with torch.no_grad():
        x_hat_f = case.model(xf, **case.kwargs(0, 9))[0].reshape((-1,) + case.dim).cpu().numpy()
    assert np.array_equal(reconstruction_movie(case.model, xf, 0),
                          refs.strip_index_rule(xf.cpu().numpy(), x_hat_f))


def test_chunks_and_max_frames():
    case = _Case('ae_cfg1', 25)          # 1x32x32: the decoder's bits do not depend on the batch
    c, h, w = case.dim
    frames, masks = case.frames.numpy(), case.frame_masks
    movie = reconstruction_movie(case.model, case.xd, 0, masks=masks.to(DEV), chunk_size=8)
    assert movie.shape == (25, h, 3 * w)
    assert np.array_equal(movie, refs.strip_index_rule(frames, case.x_hat(chunk_size=8), masks.numpy()))
    assert np.array_equal(_panels(movie, c, w)[1][:, :, :w], reconstruct_trial(case.model, case.xd, 0, chunk_size=8)[:, 0])
    assert np.array_equal(reconstruction_movie(case.model, case.xd, 0, masks=masks.to(DEV)), movie)
    cut = reconstruction_movie(case.model, case.xd, 0, masks=masks.to(DEV), max_frames=10, chunk_size=8)
    assert cut.shape == (10, h, 3 * w) and np.array_equal(cut, movie[:10])
    assert reconstruction_movie(case.model, case.xd, 0, max_frames=0).shape == (0, h, 3 * w)
    assert reconstruction_movie(case.model, case.xd, 0).shape[0] == 25          # (the default is 400 frames)


def test_cond_ae_with_labels():
    case = _Case('condae_cfg1', 8)
    movie = reconstruction_movie(case.model, case.xd, 0, labels=case.labels, masks=case.one_mask.to(DEV))
    assert np.array_equal(movie, refs.strip_index_rule(case.frames.numpy(), case.x_hat(), case.one_mask.numpy()))
    other = reconstruction_movie(case.model, case.xd, 0, labels=-case.labels, masks=case.one_mask.to(DEV))
    assert not np.array_equal(other, movie)          # the labels reach the decoder
    # max_frames cuts the labels with the frames
    assert np.array_equal(reconstruction_movie(case.model, case.xd, 0, labels=case.labels, max_frames=5,
                                               masks=case.one_mask.to(DEV)), movie[:5])


def test_extra_models_add_rows_with_a_blank_first_panel():
    case = _Case('ae_cfg1', 8)
    linear, _ = _small(golden='ae_linear', n=8)
    linear.eval()
    c, h, w = case.dim
    frames, mask = case.frames.numpy(), case.one_mask
    movie = reconstruction_movie(case.model, case.xd, 0, masks=mask.to(DEV), extra_models=(linear,))
    assert movie.shape == (8, 2 * h, 3 * w)
    top = refs.strip_index_rule(frames, case.x_hat(), mask.numpy())
    bottom = refs.strip_index_rule(frames, case.x_hat(model=linear), mask.numpy(), show_orig=False)
    assert np.array_equal(movie, np.concatenate([top, bottom], axis=1))
    assert not movie[:, h:, :w].any() and movie[:, h:, w:].any()
    assert np.array_equal(movie[:, :h], reconstruction_movie(case.model, case.xd, 0, masks=mask.to(DEV)))
    three = reconstruction_movie(case.model, case.xd, 0, extra_models=(linear, case.model))
    assert three.shape == (8, 3 * h, 3 * w) and np.array_equal(three[:, 2 * h:, w:], three[:, :h, w:])


@pytest.mark.parametrize('golden', ['ae_cfg1', 'psvae_cfg4'])
def test_bf16_decoder_feeds_its_grey_levels(golden):
    case = _Case(golden, 9, bf16=True)
    c, h, w = case.dim
    with warnings.catch_warnings():
        warnings.simplefilter('error', UserWarning)          # (an unserved stack would warn and run in fp32)
        levels = reconstruct_trial(case.model, case.xd, 0)
        movie = reconstruction_movie(case.model, case.xd, 0, masks=case.frame_masks.to(DEV))
    assert levels.dtype == np.uint8
    assert np.array_equal(movie, refs.strip_index_rule(case.frames.numpy(), levels, case.frame_masks.numpy()))
    assert np.array_equal(_panels(movie, c, w)[1], np.concatenate([levels[:, k] for k in range(c)], axis=2))
    case.model.hparams['hip_decode_dtype'] = 'f32'
    f32 = reconstruction_movie(case.model, case.xd, 0, masks=case.frame_masks.to(DEV))
    assert not np.array_equal(f32, movie)          # the bf16 code ran
    assert np.array_equal(_panels(f32, c, w)[0], _panels(movie, c, w)[0])


class _MaskedGenerator(SyntheticSessionsGenerator):
    """The synthetic generator with the one mask per trial a file-backed generator serves as ``masks``."""

    def _extra_signals(self, sample, sess, trial):
        shape = tuple(sample['images'].shape[2:])
        g = torch.Generator().manual_seed(100 + int(trial))
        sample['masks'] = (torch.rand(shape, generator=g) > 0.3).float().to(self.device)[None]


def test_make_ae_reconstruction_movie(tmp_path):
    case = _Case('ae_cfg1', 8)
    c, h, w = case.dim
    sess = SyntheticSession(7, [6, 9, 6, 9, 6, 9, 6], list(case.dim), seed=4, trial_splits='2;1;1;1')
    gen = _MaskedGenerator([sess], device=DEV, placement='device_u8')
    first = int(sess.batch_idxs['test'][0])
    stored = sess.images_u8[first]
    path = os.path.join(str(tmp_path), 'movie.npy')
    movie = make_ae_reconstruction_movie(case.model, gen, save_file=path)
    xd = torch.from_numpy(stored).to(DEV)
    assert movie.dtype == np.uint8 and movie.shape == (stored.shape[0], h, 3 * w)
    assert np.array_equal(movie, reconstruction_movie(case.model, xd, 0))
    assert np.array_equal(movie[:, :, :w], stored[:, 0])          # the first test trial, unmasked
    assert np.array_equal(np.load(path), movie)
    assert gen.serve_uint8 is False
    # another trial, cut short; the masks of the batch under use_output_mask; the linear AE below
    other = int(sess.batch_idxs['train'][0])
    assert np.array_equal(make_ae_reconstruction_movie(case.model, gen, trial=other, max_frames=4)[:, :, :w],
                          sess.images_u8[other][:4, 0])
    case.model.hparams['use_output_mask'] = True
    linear, _ = _small(golden='ae_linear', n=8)
    masked = make_ae_reconstruction_movie(case.model, gen, linear_model=linear.eval())
    mask = gen._sample(0, first, 'test')['masks'][0]
    assert masked.shape == (stored.shape[0], 2 * h, 3 * w)
    assert np.array_equal(masked, reconstruction_movie(case.model, xd, 0, masks=mask, extra_models=(linear,)))
    assert not np.array_equal(masked[:, :h], movie)
    # a cond-ae takes the batch's labels
    cond = _Case('condae_cfg1', 8)
    sess_l = SyntheticSession(7, [6, 9, 6, 9, 6, 9, 6], list(cond.dim), seed=4, n_labels=cond.meta['n_labels'],
                              trial_splits='2;1;1;1')
    gen_l = SyntheticSessionsGenerator([sess_l], device=DEV, placement='device_u8')
    first = int(sess_l.batch_idxs['test'][0])
    got = make_ae_reconstruction_movie(cond.model, gen_l)
    want = reconstruction_movie(cond.model, torch.from_numpy(sess_l.images_u8[first]).to(DEV), 0,
                                labels=torch.from_numpy(sess_l.labels[first]).to(DEV))
    assert np.array_equal(got, want)
