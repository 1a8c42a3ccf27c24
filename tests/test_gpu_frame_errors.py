"""Per-frame reconstruction errors on the GPU (csrc/frame_err.hip, the scored last layer of csrc/conv_bf16_dec.hip,
fitting.eval.frame_errors_device / export_frame_errors).

The yardstick throughout is the COMPOSED value: the per-frame masked MSE reduced on the host in float64 (``ref64``)
and in fp32 (``ref32``) from an x_hat that code accepted earlier produced (tests/frame_error_refs.py, held against
``oracle.ref_cpu.mse`` in tests/test_frame_errors_cpu.py).  Bound: ``tests.test_gpu_kernels.close(got, ref32, ref64)``.

Operands sit between NaN guard bands, LDS starts poisoned (conftest).

Figures of the first GPU run (profiles/frame_errors.txt has all of them; this module prints them with pytest -s):
* ``bn_frame_sq_err`` alone: per-frame MSE 0.08 .. 0.22 (x_hat uniform in (0, 1) against uniform uint8 targets), ref32
  4e-9 .. 1.6e-7 of the maximum from ref64, the kernel 4e-9 .. 1.8e-7: ``close`` grants its 3e-6 floor;
* the scored last layer: per-frame MSE 0.05 .. 0.13, ref32 1e-9 .. 1.8e-7, the kernel 1e-9 .. 2.7e-7;
* whole models (24 frames of 64x48): per-frame MSE 0.03 .. 0.09 on the fp32 lane (noise 0.055 .. 0.089, smooth
  0.028 .. 0.064) and 0.04 .. 0.11 on the bf16 lanes, ref32 7e-8 .. 1.7e-7 from ref64, the lanes 8e-8 .. 1.4e-7.
"""

import os
import pickle
import warnings

import numpy as np
import pytest
import torch

from behavenet_amd import _hip
from behavenet_amd import hip_functions as hf
from behavenet_amd.data.data_generator import ConcatSessionsGenerator, SyntheticSession, SyntheticSessionsGenerator
from behavenet_amd.data.trial_store import write_npz_session
from behavenet_amd.fitting.eval import (encode_trial_device, export_frame_errors, frame_errors, frame_errors_device,
                                        get_reconstruction)
from behavenet_amd.fitting.training import fit
from behavenet_amd.models.ae_model_architecture_generator import load_handcrafted_arch
from oracle import ref_cpu
from tests.bf16_decode_cases import MIN_SPAN, apply_gain, body_operands, decoder_plan, span_1_99
from tests.cases import case_data, case_hparams, seeded_build
from tests.frame_error_refs import per_frame_mse
from tests.golden_utils import base_hparams
from tests.test_gpu_decode_bf16 import LAST_CASES, _last_geom
from tests.test_gpu_encode_bf16 import _frames, _small, guarded_bf16, guarded_u8
from tests.test_gpu_guard_bands import guarded, finite, _bands_stay_untouched  # noqa: F401
from tests.test_gpu_kernels import close
from tests.test_gpu_model import BUILDERS

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SIGMOID, SLOPE = _hip.ACT_SIGMOID, 0.05
REPORT = []     # figures printed at the end of the module (pytest -s) for profiles/frame_errors.txt


def teardown_module(module):
    for line in REPORT:
        print('FRAME-ERR-FIGURE ' + line)


def _rel_to(a, b, scale):
    return float((a.double() - b.double()).abs().max()) / max(float(scale), 1e-30)


# ------------------------------------------------------------------------------------------ operands
def _target_and_mask(shape, seed, u8, masked):
    """Uniform random uint8 frames (as uint8 or as fp32 value / 255) and a ``rand > 0.3`` mask, on the CPU."""
    g = torch.Generator().manual_seed(seed)
    tu = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
    mask = (torch.rand(shape, generator=g) > 0.3).float() if masked else None
    return (tu if u8 else tu.float() / 255), mask


def _dev_target(t):
    return guarded_u8(t) if t.dtype == torch.uint8 else guarded(t)


def _refs(x_hat, target, mask, scale):
    return (per_frame_mse(x_hat, target, mask, torch.float32, scale).float(),
            per_frame_mse(x_hat, target, mask, torch.float64, scale))


# ------------------------------------------------------------------------------------------ 1: bn_frame_sq_err
FRAME_SHAPES = [(1, 7, 5), (3, 10, 14), (1, 64, 48), (2, 192, 160)]          # 35 (no multiple of 4), 420, 3072, 61440


def _run_frame_sq_err(x_hat, target, mask, scale, offset=0):
    """The kernel between guard bands -> (N,) on the CPU.  ``offset``: the operands start that many ELEMENTS off
    their 16-byte boundary (the element-by-element loads)."""
    def place(t):
        if not offset:
            return _dev_target(t)
        flat = torch.cat([t.flatten()[:offset], t.flatten()])
        return _dev_target(flat)[offset:].view(t.shape)
    xd, td = place(x_hat), place(target)
    md = place(mask) if mask is not None else None
    out = guarded(torch.zeros(x_hat.shape[0]))
    got = _hip.frame_sq_err(xd, td, md, scale, out=out)
    assert got is out
    finite(out, 'frame_sq_err')
    return out.cpu()


@pytest.mark.parametrize('masked', [False, True], ids=['nomask', 'mask'])
@pytest.mark.parametrize('u8', [False, True], ids=['fp32', 'u8'])
@pytest.mark.parametrize('n', [1, 7])
@pytest.mark.parametrize('shape', FRAME_SHAPES, ids=['x'.join(map(str, s)) for s in FRAME_SHAPES])
def test_frame_sq_err(shape, n, u8, masked):
    d = int(np.prod(shape))
    g = torch.Generator().manual_seed(d + n)
    x_hat = torch.rand((n,) + shape, generator=g)
    target, mask = _target_and_mask((n,) + shape, d + 3 * n, u8, masked)
    for scale in (1.0, 1.0 / d):
        ref32, ref64 = _refs(x_hat, target, mask, scale)
        got = _run_frame_sq_err(x_hat, target, mask, scale)
        mse = ref64 / (scale * d)
        REPORT.append('frame_sq_err %s N=%d %s %s scale=%.3g: mse %.4f..%.4f, ref32 vs ref64 %.1e, hip vs ref64 %.1e'
                      % (shape, n, 'u8' if u8 else 'fp32', 'mask' if masked else 'nomask', scale, float(mse.min()),
                         float(mse.max()), _rel_to(ref32, ref64, ref64.max()), _rel_to(got, ref64, ref64.max())))
        close(got, ref32, ref64, name='frame_sq_err %s N=%d scale=%g' % (shape, n, scale))


# ------------------------------------------------------------------------------------------ 2: the scored last layer
FUSED_CASES = [(c[0], c[1], c[2], None) for c in LAST_CASES] + \
              [('default [1, 64, 48] convT4 N=3', 61, (1, 64, 48), 3), ('default [2, 192, 160] convT4 N=3', 62,
                                                                        (2, 192, 160), 3)]


def _fused_geom(case):
    if case[3] is None:
        return _last_geom(case)
    return decoder_plan(case[2])[4].geom(case[3])


class _Fused(object):
    """Device operands of one case, the x_hat of the EXISTING ``_hip.convT2d_last_bf16`` on them, and the scored
    layer on any range of the frames."""

    def __init__(self, case):
        self.geom = _fused_geom(case)
        N, Ci, Hi, Wi, Co, R, S, st, ct, cl, Ho, Wo = self.geom
        assert _hip.convT2d_bf16_ok(self.geom, last=True), (case[0], self.geom)
        x, w, b = body_operands(self.geom, case[1], exact_weights=False)
        self.xd = guarded_bf16(x.permute(0, 2, 3, 1).contiguous())
        self.wd, self.bd = guarded(w), guarded(b)
        y = guarded(torch.zeros(N, Co, Ho, Wo))
        _hip.convT2d_last_bf16(self.xd, self.wd, self.bd, self.geom, SIGMOID, SLOPE, out=y)
        finite(y, 'bf16 last layer')
        self.x_hat = y.cpu()
        self.shape = (N, Co, Ho, Wo)

    def score(self, td, md, scale, beg=0, end=None):
        end = self.geom[0] if end is None else end
        geom = (end - beg,) + tuple(self.geom[1:])
        out = guarded(torch.zeros(end - beg))
        _hip.convT2d_last_bf16_sqerr(self.xd[beg:end], self.wd, self.bd, td[beg:end],
                                     None if md is None else md[beg:end], geom, SIGMOID, SLOPE, scale, out=out)
        finite(out, 'scored last layer')
        return out.cpu()


@pytest.mark.parametrize('case', FUSED_CASES, ids=[c[0] for c in FUSED_CASES])
def test_scored_last_layer(case):
    """x_hat of the unfused kernel, reduced on the host, against the fused kernel: only the summation differs."""
    f = _Fused(case)
    d = int(np.prod(f.shape[1:]))
    for u8, masked, scale in [(True, True, 1.0 / d), (False, False, 1.0), (True, False, 1.0), (False, True, 1.0 / d)]:
        target, mask = _target_and_mask(f.shape, case[1] + 2 * u8 + masked, u8, masked)
        ref32, ref64 = _refs(f.x_hat, target, mask, scale)
        got = f.score(_dev_target(target), None if mask is None else guarded(mask), scale)
        mse = ref64 / (scale * d)
        REPORT.append('scored last layer %s %s %s: mse %.4f..%.4f, ref32 vs ref64 %.1e, hip vs ref64 %.1e'
                      % (case[0], 'u8' if u8 else 'fp32', 'mask' if masked else 'nomask', float(mse.min()),
                         float(mse.max()), _rel_to(ref32, ref64, ref64.max()), _rel_to(got, ref64, ref64.max())))
        close(got, ref32, ref64, name='scored last layer %s u8=%d mask=%d' % (case[0], u8, masked))


# ------------------------------------------------------------------------------------------ 3: frame independence
@pytest.mark.parametrize('shape', FRAME_SHAPES, ids=['x'.join(map(str, s)) for s in FRAME_SHAPES])
def test_frame_sq_err_scores_a_frame_alone_as_in_a_batch(shape):
    d, n = int(np.prod(shape)), 7
    g = torch.Generator().manual_seed(d)
    x_hat = torch.rand((n,) + shape, generator=g)
    for u8, masked in [(False, False), (True, True), (False, True), (True, False)]:
        target, mask = _target_and_mask((n,) + shape, d + 1, u8, masked)
        full = _run_frame_sq_err(x_hat, target, mask, 1.0 / d)
        assert torch.equal(full, _run_frame_sq_err(x_hat, target, mask, 1.0 / d))
        for beg, end in [(0, 1), (3, 7)]:
            part = _run_frame_sq_err(x_hat[beg:end], target[beg:end], None if mask is None else mask[beg:end], 1.0 / d)
            assert torch.equal(part, full[beg:end]), (shape, u8, masked, beg)
        # off the 16-byte boundary: other loads, the same arithmetic
        assert torch.equal(_run_frame_sq_err(x_hat, target, mask, 1.0 / d, offset=1), full), (shape, u8, masked)


@pytest.mark.parametrize('case', [c for c in FUSED_CASES if _fused_geom(c)[0] == 7], ids=lambda c: c[0])
def test_scored_last_layer_scores_a_frame_alone_as_in_a_batch(case):
    f = _Fused(case)
    d = int(np.prod(f.shape[1:]))
    for u8, masked in [(True, True), (False, False)]:
        target, mask = _target_and_mask(f.shape, case[1], u8, masked)
        td, md = _dev_target(target), None if mask is None else guarded(mask)
        full = f.score(td, md, 1.0 / d)
        assert torch.equal(full, f.score(td, md, 1.0 / d))
        for beg, end in [(0, 1), (3, 7)]:
            assert torch.equal(f.score(td, md, 1.0 / d, beg, end), full[beg:end]), (case[0], u8, beg)


def test_refused_calls_write_nothing():
    lib = _hip.load()
    x = torch.zeros((4, 8, 8, 32), dtype=torch.bfloat16, device=DEV)
    w = torch.zeros(32 * 5 * 25, device=DEV)
    target = torch.zeros((4, 5, 16, 16), device=DEV)
    out = torch.full((64,), 7.0, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    ok1 = (4, 32, 8, 8, 1, 5, 5, 2, 1, 1, 16, 16)
    c8 = (4, 8, 8, 8, 1, 5, 5, 2, 1, 1, 16, 16)                     # 8 input channels: not a multiple of 16
    co5 = (4, 32, 8, 8, 5, 5, 5, 2, 1, 1, 16, 16)                   # five channels on the layer onto the frame

    def call(geom, act, xp=None):
        return lib.bn_convT2d_last_bf16_sqerr(xp or x.data_ptr(), w.data_ptr(), None, target.data_ptr(), 0, None,
                                              out.data_ptr(), *geom, act, SLOPE, 1.0, None, 0, st)
    assert call(c8, SIGMOID) == -2 and call(co5, SIGMOID) == -2
    assert call(ok1, 9) == -2                                        # an activation the epilogue does not have
    assert call(ok1, SIGMOID, x.data_ptr() + 2) == -2                # a misaligned operand
    for g in (c8, co5):
        assert lib.bn_convT2d_last_bf16_sqerr_ws_bytes(*g) == 0 and not _hip.convT2d_bf16_ok(g, last=True)
    # fp32 operands off a 4-byte boundary cannot be read at all
    assert lib.bn_frame_sq_err(target.data_ptr() + 2, target.data_ptr(), 0, None, out.data_ptr(), 4, 1280, 1.0, None,
                               0, st) == -2
    # a workspace that is too small
    assert lib.bn_frame_sq_err_ws_bytes(4, 5000) == 4 * 2 * 4
    assert lib.bn_frame_sq_err(target.data_ptr(), target.data_ptr(), 0, None, out.data_ptr(), 1, 5000, 1.0, None, 0,
                               st) == -3
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ------------------------------------------------------------------------------------------ whole models
CLASS_DIMS = [('ae', (1, 64, 48)), ('vae', (1, 64, 48)), ('ps-vae', (1, 64, 48)), ('ps-vae', (2, 64, 48)),
              ('cond-ae-msp', (1, 64, 48))]
N_FRAMES = 24


def _fwd_kwargs(model_class):
    return {'dataset': 0, 'use_mean': True} if model_class in ('vae', 'ps-vae') else {'dataset': 0}


def _trial_mask(dim, seed):
    return (torch.rand(tuple(dim), generator=torch.Generator().manual_seed(seed)) > 0.3).float()


def _oracle64(meta, hip):
    """The float64 oracle with the HIP model's parameters as they are now."""
    ora64 = seeded_build(ref_cpu.build_model, case_hparams(meta)).double().eval()
    ora64.load_state_dict({k: v.detach().double().cpu() for k, v in hip.state_dict().items()})
    return ora64


# 4
@pytest.mark.parametrize('smooth', [False, True], ids=['noise', 'smooth'])
@pytest.mark.parametrize('model_class,dim', CLASS_DIMS, ids=['%s-%d' % (c, d[0]) for c, d in CLASS_DIMS])
def test_fp32_lane(model_class, dim, smooth):
    model, meta = _small(model_class, dim, N_FRAMES)
    model.eval()
    xu = _frames(N_FRAMES, dim, 7, smooth=smooth)
    with torch.no_grad():
        x_hat = model(xu.to(DEV), **_fwd_kwargs(model_class))[0].cpu()
        ora = _oracle64(meta, model)(xu.double() / 255, **_fwd_kwargs(model_class))[0]
    for mask in (None, _trial_mask(dim, 5)):
        ref32, ref64 = _refs(x_hat, xu, mask, None)
        with warnings.catch_warnings():
            warnings.simplefilter('error', UserWarning)
            got = frame_errors_device(model, xu.to(DEV), 0, None if mask is None else mask.to(DEV))
        assert got.is_cuda and got.dtype == torch.float32 and got.shape == (N_FRAMES,)
        close(got, ref32, ref64, name='fp32 lane %s' % model_class)
        # the same from fp32 frames, as numpy, in chunks: the same bits
        again = frame_errors(model, (xu.float() / 255).to(DEV), 0, None if mask is None else mask.to(DEV),
                             chunk_size=7)
        assert again.dtype == np.float32 and np.array_equal(again, got.cpu().numpy())
        # against the float64 oracle: what the lane adds to the x_hat error it inherits
        exact = per_frame_mse(ora, xu, mask, torch.float64)
        e_got, e_yard = _rel_to(got.cpu(), exact, exact.max()), _rel_to(ref64, exact, exact.max())
        REPORT.append('fp32 lane %s %s %s %s: mse %.4f..%.4f, ref32 vs ref64 %.1e, hip vs ref64 %.1e, vs float64 oracle: '
                      'hip %.2e yardstick %.2e' % (model_class, dim, 'smooth' if smooth else 'noise',
                                                   'mask' if mask is not None else 'nomask', float(ref64.min()),
                                                   float(ref64.max()), _rel_to(ref32, ref64, ref64.max()),
                                                   _rel_to(got.cpu(), ref64, ref64.max()), e_got, e_yard))
        assert e_got <= 2 * e_yard + 3e-6, (e_got, e_yard)


@pytest.mark.parametrize('golden', ['ae_cfg1_bn', 'ae_maxpool', 'ae_linear', 'ae_cfg1_lastff', 'condae_cfg1',
                                    'condvae_cfg1'])
def test_fp32_lane_serves_every_route(golden):
    """Batch norm, max pooling (tests/golden/arch_maxpool.json), the linear AE, a dense last layer and the
    label-conditioned classes all land on the fp32 lane."""
    n = 12
    model, meta = _small(golden=golden, n=n)
    model.eval()
    data = case_data(meta, device=DEV)
    x = data['images'][0].contiguous()
    labels = data['labels'][0] if 'labels' in data else None
    kwargs = {'dataset': 0}
    if meta['model_class'] in ('cond-ae', 'cond-vae'):
        kwargs.update(labels=labels, labels_2d=None)
    if meta['model_class'] == 'cond-vae':
        kwargs['use_mean'] = True
    with torch.no_grad():
        x_hat = model(x, **kwargs)[0].cpu()
    ref32, ref64 = _refs(x_hat.view(x.shape), x, None, None)
    got = frame_errors_device(model, x, 0, labels=labels)
    close(got, ref32, ref64, name='fp32 lane %s' % golden)
    assert torch.equal(got, frame_errors_device(model, x, 0, labels=labels, chunk_size=5))


# 5
def _decoder_input_bf16(model_class, model, xu):
    """What the class's ``forward`` hands its decoder when the encoder runs on its bf16 stack."""
    if model_class in ('ae', 'vae'):
        return encode_trial_device(model, xu, 0, None, 1024)          # (under the model's hip_encode_dtype key)
    with torch.no_grad(), hf.encode_precision('bf16'):
        out = model.encoding(xu, dataset=0)
    return torch.cat([out[0], out[1]], dim=1) if model_class == 'ps-vae' else out[0]


LATENT_STD = 2.0


def _scaled_latents(model_class, model, xd):
    """A freshly initialised encoder hands its decoder latents of a few hundredths, and the decoder then draws an
    almost constant grey whatever its gain (measured: a 1..99% span of 0.21 where the decoder tests, which feed
    N(0, 1) latents, ask for MIN_SPAN).  The encoder's dense layer is rewritten so that every latent the decoder
    takes has zero mean and a standard deviation of LATENT_STD over these frames; the oracle gets the same
    parameters.  LATENT_STD = 2: the decoder is positively homogeneous but for its biases, so the latents' scale sets
    the contrast of the frames, and at these small frames unit latents left the PS-VAE decoders at a span of 0.45
    (AE / VAE: 0.56).  (PS-VAE: the decoder takes [A h | B h] of the dense layer's output h; the square matrix
    [A; B] is undone around the scaling.)"""
    from behavenet_amd.fitting.eval import _LATENTS_AT
    enc = model.encoding
    with torch.no_grad():
        lat = model(xd, **_fwd_kwargs(model_class))[_LATENTS_AT[model_class]].double().cpu()
        w, b = enc.FF.weight.double().cpu(), enc.FF.bias.double().cpu()
        m = torch.eye(w.shape[0], dtype=torch.float64)
        if model_class == 'ps-vae':
            m = torch.cat([enc.A.weight, enc.B.weight], dim=0).double().cpu()
        d = torch.diag(LATENT_STD / lat.std(dim=0))
        mi = torch.linalg.inv(m)
        enc.FF.weight.copy_((mi @ d @ m @ w).float())
        enc.FF.bias.copy_((mi @ d @ (m @ b - lat.mean(dim=0))).float())
        lat = model(xd, **_fwd_kwargs(model_class))[_LATENTS_AT[model_class]]
        assert float((lat.std(dim=0) - LATENT_STD).abs().max()) < 2e-2 and float(lat.mean(dim=0).abs().max()) < 2e-2


@pytest.mark.parametrize('model_class,dim', CLASS_DIMS, ids=['%s-%d' % (c, d[0]) for c, d in CLASS_DIMS])
def test_bf16_lanes(model_class, dim):
    model, meta = _small(model_class, dim, N_FRAMES)
    model.eval()
    apply_gain(model.decoding.decoder)
    xu = _frames(N_FRAMES, dim, 9, smooth=True)
    xd = xu.to(DEV)
    _scaled_latents(model_class, model, xd)
    with torch.no_grad():
        ora = _oracle64(meta, model)(xu.double() / 255, **_fwd_kwargs(model_class))[0]
    span = span_1_99(ora)
    mask = _trial_mask(dim, 6)
    f32 = {m is None: frame_errors_device(model, xd, 0, None if m is None else m.to(DEV)).clone() for m in (None, mask)}
    for keys in (('hip_decode_dtype',), ('hip_decode_dtype', 'hip_encode_dtype')):
        for k in keys:
            model.hparams[k] = 'bf16'
        with warnings.catch_warnings():
            warnings.simplefilter('error', UserWarning)
            if len(keys) == 1:
                x_hat = torch.from_numpy(get_reconstruction(model, xd, dataset=0))
            else:
                z = _decoder_input_bf16(model_class, model, xd)
                x_hat = torch.from_numpy(get_reconstruction(model, z, apply_inverse_transform=False))
            for m in (None, mask):
                ref32, ref64 = _refs(x_hat, xu, m, None)
                got = frame_errors_device(model, xd, 0, None if m is None else m.to(DEV))
                REPORT.append('bf16 lane %s %s %s %s: mse %.4f..%.4f, ref32 vs ref64 %.1e, hip vs ref64 %.1e, oracle '
                              'x_hat 1..99%% span %.3f' % (model_class, dim, '+'.join(keys),
                                                          'mask' if m is not None else 'nomask', float(ref64.min()),
                                                          float(ref64.max()), _rel_to(ref32, ref64, ref64.max()),
                                                          _rel_to(got.cpu(), ref64, ref64.max()), span))
                close(got, ref32, ref64, name='bf16 lane %s %s' % (model_class, keys))
                assert not torch.equal(got, f32[m is None])          # the bf16 code ran
                assert torch.equal(got, frame_errors_device(model, xd, 0, None if m is None else m.to(DEV),
                                                            chunk_size=5))
    assert span >= MIN_SPAN, 'the oracle reconstruction spans %.3f: not a usable yardstick' % span


# 6
def _tiny_generator(dim, device=DEV):
    sess = SyntheticSession(7, [6, 9, 6, 9, 6, 9, 6], list(dim), seed=4, trial_splits='2;1;1;1')
    return SyntheticSessionsGenerator([sess], device=device, placement='device_u8')


@pytest.mark.parametrize('model_class', ['ae', 'vae', 'ps-vae'])
def test_scoring_frames_moves_nothing_else(model_class, tmp_path):
    """loss() in eval and training mode (with gradients), forward(), a bare model.decoding(z), encode_trial_device and
    get_reconstruction from latents and from images give the same bits with calls of frame_errors_device and
    export_frame_errors in between as without, both keys set."""
    dim = (2, 64, 48) if model_class == 'ps-vae' else (1, 64, 48)
    n = 24
    xu = _frames(n, dim, 5).to(DEV)
    xf = (xu.float() / 255).contiguous()
    res = {}
    for scoring in (False, True):
        model, meta = _small(model_class, dim, n)
        model.hparams.update(hip_decode_dtype='bf16', hip_encode_dtype='bf16')
        model.version = 0

        def score():
            if not scoring:
                return
            frame_errors_device(model, xu, 0, _trial_mask(dim, 1).to(DEV))
            frame_errors_device(model, xf, 0)
            export_frame_errors(_tiny_generator(dim), model, filename=os.path.join(str(tmp_path), 'e.pkl'))
        data = {'images': xf[None]}
        if meta['n_labels']:
            g = torch.Generator().manual_seed(2)
            data['labels'] = torch.randn((1, n, meta['n_labels']), generator=g).to(DEV)
        z = torch.randn((n, model.decoding.FF.in_features), generator=torch.Generator().manual_seed(3)).to(DEV)
        out = {}
        score()
        model.eval()
        torch.manual_seed(1)
        ev = model.loss(data, dataset=0, accumulate_grad=False)
        out['eval_loss'] = {k: float(v) for k, v in dict(ev).items()}
        score()
        model.eval()
        torch.manual_seed(1)
        with torch.no_grad():
            fw = model(xf, dataset=0, use_mean=True) if model_class != 'ae' else model(xf, dataset=0)
            out['decoding'] = model.decoding(z, None, None, dataset=0).clone()
        out['forward'] = [t.clone() for t in fw if torch.is_tensor(t)]
        score()
        out['latents'] = encode_trial_device(model, xu, 0, None, 1024).clone()
        out['recon'] = torch.from_numpy(get_reconstruction(model, z, apply_inverse_transform=False))
        out['recon_img'] = torch.from_numpy(get_reconstruction(model, xf, dataset=0))
        score()
        model.train()
        model.zero_grad()
        torch.manual_seed(1)
        tr = model.loss(data, dataset=0, accumulate_grad=True)
        out['train_loss'] = {k: float(v) for k, v in dict(tr).items()}
        out['grads'] = [p.grad.clone() for p in model.parameters() if p.grad is not None]
        res[scoring] = out
    a, b = res[False], res[True]
    assert a['eval_loss'] == b['eval_loss'] and a['train_loss'] == b['train_loss']
    for k in ('decoding', 'latents', 'recon', 'recon_img'):
        assert torch.equal(a[k], b[k]), k
    assert len(a['forward']) == len(b['forward']) and len(a['grads']) == len(b['grads']) > 0
    for s, t in zip(a['forward'] + a['grads'], b['forward'] + b['grads']):
        assert torch.equal(s, t)
    # the request reaches nobody outside its block, and nobody without the decode key
    assert hf.frame_err_request() is None
    model.eval()
    with torch.no_grad(), hf.scoring_frames(xu, None, 1.0) as req:
        x_hat = model.decoding(z, None, None, dataset=0)
    assert req.scores is None and torch.equal(x_hat, a['decoding'])


# 7
@pytest.mark.parametrize('golden,why', [('ae_cfg1_lastff', 'ae_decoding_last_FF_layer'), ('ae_cfg1_bn', 'batch-norm')])
def test_unserved_decoder_under_the_bf16_key(golden, why):
    n = 12
    model, meta = _small(golden=golden, n=n)
    x = case_data(meta, device=DEV)['images'][0].contiguous()
    want = frame_errors_device(model, x, 0).clone()
    model.hparams['hip_decode_dtype'] = 'bf16'
    with pytest.warns(UserWarning, match=why) as rec:
        got = frame_errors_device(model, x, 0)
        again = frame_errors_device(model, x[:5], 0)
    assert len([w for w in rec if 'bf16 decoding' in str(w.message)]) == 1
    assert torch.equal(got, want) and torch.equal(again, want[:5])


# 8
@pytest.mark.parametrize('keys', [(), ('hip_decode_dtype', 'hip_encode_dtype')], ids=['f32', 'bf16'])
def test_export_frame_errors_end_to_end(tmp_path, keys):
    dim = [1, 64, 48]
    root = str(tmp_path)
    arch = load_handcrafted_arch(list(dim), 6, None, check_memory=False)
    hp = base_hparams(arch, 'ae', {'expt_dir': root, 'device': 'cuda'})
    torch.manual_seed(0)
    hip = BUILDERS['ae'](hp).to(DEV)
    hip.version = 0
    os.makedirs(os.path.join(root, 'version_0'))
    apply_gain(hip.decoding.decoder)
    for k in keys:
        hip.hparams[k] = 'bf16'
    rng = np.random.default_rng(3)
    lens = [24, 31, 24, 31, 24, 31, 24, 31, 24, 31]
    ids, paths, trials = [], [], []
    for s in range(2):
        trials.append([rng.integers(0, 255, size=(t,) + tuple(dim), dtype=np.uint8) for t in lens])
        sess_dir = os.path.join(root, 'lab', 'expt', 'animal', 'sess%d' % s)
        write_npz_session(os.path.join(sess_dir, 'data.npz'), {'images': trials[s]})
        ids.append({'lab': 'lab', 'expt': 'expt', 'animal': 'animal', 'session': 'sess%d' % s})
        paths.append([os.path.join(sess_dir, 'data.npz')])

    def run(chunk):
        gen = ConcatSessionsGenerator(root, ids, signals_list=[['images']] * 2, transforms_list=[[None]] * 2,
                                      paths_list=paths, device='cuda', placement='host_u8', keep_in_memory=False,
                                      trial_splits={'train_tr': 5, 'val_tr': 1, 'test_tr': 1, 'gap_tr': 1})
        hip.hparams['export_chunk_frames'] = chunk
        with warnings.catch_warnings():
            warnings.simplefilter('error', UserWarning)
            files = export_frame_errors(gen, hip)
        assert files == [os.path.join(root, 'version_0', 'lab_expt_animal_sess%d_frame_errors.pkl' % s)
                         for s in range(2)]
        out = []
        for f in files:
            with open(f, 'rb') as fh:
                out.append(pickle.load(fh))
        return out, gen
    a, gen = run(16)
    b, _ = run(1024)
    n_gap = 0
    for s in range(2):
        assert sorted(a[s]) == sorted(b[s]) == ['mse', 'trials']
        used = set(int(t) for k in ('train', 'val', 'test') for t in gen.datasets[s].batch_idxs[k])
        assert len(a[s]['mse']) == len(b[s]['mse']) == len(lens)
        for i, t in enumerate(lens):
            ea, eb = a[s]['mse'][i], b[s]['mse'][i]
            if i not in used:
                n_gap += 1
                assert ea.size == 0 and eb.size == 0
                continue
            assert ea.dtype == np.float32 and ea.shape == (t,)
            assert np.array_equal(ea, eb), (s, i)                       # a frame's bits do not depend on the chunks
            want = frame_errors(hip, torch.from_numpy(trials[s][i]).to(DEV), s, chunk_size=1024)
            assert np.array_equal(ea, want), (s, i)
    assert n_gap > 0
    REPORT.append('export end to end %s: mse %.4f..%.4f' % ('+'.join(keys) or 'f32',
                                                           min(float(e.min()) for e in a[0]['mse'] if e.size),
                                                           max(float(e.max()) for e in a[0]['mse'] if e.size)))


def test_fit_writes_the_frame_errors(tmp_path):
    dim = [1, 32, 32]
    arch = load_handcrafted_arch(list(dim), 8, None, check_memory=False)
    hp = base_hparams(arch, 'ae', None)
    hp.update({'expt_dir': str(tmp_path), 'max_n_epochs': 2, 'min_n_epochs': 0, 'val_check_interval': 1,
               'enable_early_stop': False, 'early_stop_history': 10, 'rng_seed_train': 0, 'export_latents': False,
               'export_frame_errors': True, 'progress_bar': False, 'device': 'cuda'})
    os.makedirs(os.path.join(str(tmp_path), 'version_0'))
    sess = SyntheticSession(10, 32, dim, seed=0, trial_splits='8;1;1;0')
    gen = SyntheticSessionsGenerator([sess], device=DEV, placement='device_u8')
    torch.manual_seed(0)
    model = BUILDERS['ae'](hp).to(DEV)
    model.version = 0

    class Exp(object):
        version = 0

        def log(self, row):
            pass

        def save(self):
            pass
    best = fit(hp, model, gen, Exp(), method='ae')
    path = os.path.join(str(tmp_path), 'version_0', 'lab_expt_animal_sess_frame_errors.pkl')
    assert os.path.exists(path) and not os.path.exists(path.replace('frame_errors', 'latents'))
    with open(path, 'rb') as f:
        got = pickle.load(f)
    assert len(got['mse']) == 10 and all(e.shape == (32,) and e.dtype == np.float32 for e in got['mse'])
    gen.reset_iterators('test')
    data, s_ = gen.next_batch('test')
    want = frame_errors(best, data['images'][0], s_)
    assert np.array_equal(got['mse'][int(data['batch_idx'])], want)
