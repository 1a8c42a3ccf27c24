"""Reconstructions as stored uint8 grey levels ("reconstructions").

The rule is ``tests/recon_u8_refs.quantise_u8``: NaN -> 0, else clamp(rint(x * 255), 0, 255), the product in fp32 and
rint to nearest even -- the IEEE operations the kernels perform, so every comparison with it is ``torch.equal``.

1. ``_hip.unit_float_to_u8`` is exactly ``quantise_u8``: every size, both operands on and 1..3 elements / bytes off
   their 16-byte boundary, the special values spliced in.
2. The fused layer ``_hip.convT2d_last_bf16_u8`` equals ``unit_float_to_u8(convT2d_last_bf16(...))`` exactly on
   the same operands, on even and odd output addresses, and stays within 0.5 + 255e-4 grey levels of 255 x the float64
   emulation (0.5 is the rounding itself, 1e-4 is ``close``'s ``norm_tol`` on an x_hat of magnitude at most 1; where
   the operands are scaled to saturate, the yardstick is clamped to [0, 255] as the rule clamps -- the bound is the
   same, and no pixel is exempt).
3. Whole models: ``reconstruct_trial_device`` against the model's own ``forward`` (exactly) and against the float64
   oracle (the bound of 2), on the fp32 lane and with both keys.
4. ``get_reconstruction(as_uint8=True)``, 5. nothing else moves, 6. ``export_reconstructions`` end to end.
"""

import os
import warnings

import numpy as np
import pytest
import torch

from behavenet_amd import _hip
from behavenet_amd import hip_functions as hf
from behavenet_amd.data.data_generator import ConcatSessionsGenerator, SyntheticSession, SyntheticSessionsGenerator
from behavenet_amd.data.trial_store import open_trial_store, write_npz_session
from behavenet_amd.fitting import distributed as bdist
from behavenet_amd.fitting.eval import (encode_trial_device, export_reconstructions, frame_errors_device,
                                        get_reconstruction, reconstruct_trial, reconstruct_trial_device)
from behavenet_amd.fitting.training import fit
from behavenet_amd.models.ae_model_architecture_generator import load_handcrafted_arch
from tests import bf16_decode_emulation as demu
from tests.bf16_decode_cases import MIN_SPAN, apply_gain, body_operands, span_1_99
from tests.cases import case_data, load_case
from tests.golden_utils import base_hparams
from tests.recon_u8_refs import quantise_u8, with_specials
from tests.test_gpu_encode_bf16 import GOLDEN_OF, _frames, _small, guarded_bf16, guarded_u8
from tests.test_gpu_frame_errors import FUSED_CASES, _fused_geom, _oracle64
from tests.test_gpu_guard_bands import guarded, _bands_stay_untouched  # noqa: F401
from tests.test_gpu_model import BUILDERS

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SLOPE, NONE, LRELU, SIGMOID = 0.05, _hip.ACT_NONE, _hip.ACT_LRELU, _hip.ACT_SIGMOID
SENTINEL = 0xAB
GREY_TOL = 0.5 + 255e-4
REPORT = []     # figures printed at the end of the module (pytest -s)


def teardown_module(module):
    if REPORT:
        print('\n' + '\n'.join(REPORT))


def _u8_out(shape, offset=0):
    """A sentinel-filled uint8 device tensor of ``shape`` between guard bands, ``offset`` bytes off its 16-byte
    boundary -> (the tensor, the whole guarded byte buffer)."""
    n = int(np.prod(shape))
    whole = guarded_u8(torch.full((n + 16,), SENTINEL, dtype=torch.uint8))
    assert whole.data_ptr() % 16 == 0
    return whole[offset:offset + n].view(shape), whole


def _rest_is_sentinel(whole, offset, n):
    assert bool((whole[:offset] == SENTINEL).all()) and bool((whole[offset + n:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------ 1: the conversion
@pytest.mark.parametrize('n', [1, 35, 4099, 2 * 192 * 160])
def test_unit_float_to_u8_is_the_rule(n):
    x = with_specials(np.random.default_rng(n).random(n, dtype=np.float32), seed=n)
    want = torch.from_numpy(quantise_u8(x))
    xt = torch.from_numpy(x)
    for in_off in range(4):
        xd = guarded(torch.cat([torch.zeros(in_off), xt]))[in_off:]
        assert xd.data_ptr() % 16 == 4 * in_off
        for out_off in range(4):
            out, whole = _u8_out((n,), out_off)
            got = _hip.unit_float_to_u8(xd, out=out)
            assert got is out and torch.equal(out.cpu(), want), (n, in_off, out_off)
            _rest_is_sentinel(whole, out_off, n)
    # any shape, a fresh output
    if n == 2 * 192 * 160:
        got = _hip.unit_float_to_u8(guarded(xt.view(2, 192, 160)))
        assert got.dtype == torch.uint8 and got.shape == (2, 192, 160) and torch.equal(got.cpu().flatten(), want)


def test_unit_float_to_u8_refuses_a_misaligned_fp32_pointer():
    lib = _hip.load()
    x = torch.rand(64, device=DEV)
    out, whole = _u8_out((32,))
    st = torch.cuda.current_stream().cuda_stream
    assert lib.bn_unit_float_to_u8(x.data_ptr() + 2, out.data_ptr(), 32, st) == -2
    assert lib.bn_unit_float_to_u8(x.data_ptr() + 1, out.data_ptr(), 1, st) == -2
    assert lib.bn_unit_float_to_u8(None, out.data_ptr(), 32, st) == -1
    assert lib.bn_unit_float_to_u8(x.data_ptr(), out.data_ptr(), 0, st) == 0
    torch.cuda.synchronize()
    _rest_is_sentinel(whole, 0, 0)


# ------------------------------------------------------------------------------------------ 2: the fused layer
class _Layer(object):
    """Device operands of one geometry, the fp32 x_hat of the EXISTING ``_hip.convT2d_last_bf16`` on them, and the
    quantising layer on any range of the frames."""

    def __init__(self, geom, seed, act=SIGMOID, gain=1.0):
        self.geom, self.act = geom, act
        N, Ci, Hi, Wi, Co, R, S, st, ct, cl, Ho, Wo = geom
        assert _hip.convT2d_bf16_ok(geom, last=True), geom
        x, w, b = body_operands(geom, seed, exact_weights=False)
        self.x, self.w, self.b = x, w * gain, b
        self.xd = guarded_bf16(x.permute(0, 2, 3, 1).contiguous())
        self.wd, self.bd = guarded(self.w), guarded(b)
        self.shape = (N, Co, Ho, Wo)
        y = guarded(torch.zeros(self.shape))
        _hip.convT2d_last_bf16(self.xd, self.wd, self.bd, geom, act, SLOPE, out=y)
        self.x_hat = y

    def u8(self, beg=0, end=None, offset=0):
        end = self.geom[0] if end is None else end
        geom = (end - beg,) + tuple(self.geom[1:])
        shape = (end - beg,) + self.shape[1:]
        out, whole = _u8_out(shape, offset)
        got = _hip.convT2d_last_bf16_u8(self.xd[beg:end], self.wd, self.bd, geom, self.act, SLOPE, out=out)
        assert got is out
        res = out.cpu()
        _rest_is_sentinel(whole, offset, int(np.prod(shape)))
        return res

    def check(self, name):
        want = _hip.unit_float_to_u8(self.x_hat).cpu()
        for offset in (0, 1):          # (an odd base: the stride-2 kernel's pairs fall on the other parity)
            assert torch.equal(self.u8(offset=offset), want), (name, offset)
        assert np.array_equal(want.numpy(), quantise_u8(self.x_hat.cpu().numpy())), name
        ref64 = demu.convT_layer(self.x, self.w, self.b, self.geom, self.act, torch.float64)
        err = float((want.double() - (255.0 * ref64).clamp(0.0, 255.0)).abs().max())
        REPORT.append('fused layer %s: grey levels %d..%d, max |u8 - 255 ref64| %.4f (bound %.4f)'
                      % (name, int(want.min()), int(want.max()), err, GREY_TOL))
        assert err <= GREY_TOL, (name, err)
        return want


@pytest.mark.parametrize('case', FUSED_CASES, ids=[c[0] for c in FUSED_CASES])
def test_fused_layer_writes_the_bytes_of_the_unfused_route(case):
    layer = _Layer(_fused_geom(case), case[1])
    want = layer.check(case[0])
    if layer.geom[0] == 7:
        # frames [2, 5) of the batch, run alone, have the bytes they have in the batch
        assert torch.equal(layer.u8(2, 5), want[2:5]), case[0]
        assert torch.equal(layer.u8(2, 5, offset=1), want[2:5]), case[0]


@pytest.mark.parametrize('act', [LRELU, NONE], ids=['lrelu', 'none'])
@pytest.mark.parametrize('case', [FUSED_CASES[1], FUSED_CASES[3], FUSED_CASES[8]], ids=lambda c: c[0])
def test_fused_layer_saturates(case, act):
    """Linear decoders have no sigmoid: pre-activations of a few units leave below 0 and above 1."""
    layer = _Layer(_fused_geom(case), case[1] + 1, act=act, gain=4.0)
    assert float(layer.x_hat.min()) < 0.0 and float(layer.x_hat.max()) > 1.0
    want = layer.check('%s act %d' % (case[0], act))
    assert int(want.min()) == 0 and int(want.max()) == 255 and 0 < int(((want > 0) & (want < 255)).sum())


def test_fused_layer_refusals_write_nothing():
    lib = _hip.load()
    x = torch.zeros((4, 8, 8, 32), dtype=torch.bfloat16, device=DEV)
    w = torch.zeros(32 * 5 * 49, device=DEV)
    out, whole = _u8_out((4, 5, 16, 16))
    st = torch.cuda.current_stream().cuda_stream
    ok1 = (4, 32, 8, 8, 1, 5, 5, 2, 1, 1, 16, 16)
    c8 = (4, 8, 8, 8, 1, 5, 5, 2, 1, 1, 16, 16)                     # 8 input channels: not a multiple of 16
    k7 = (4, 32, 8, 8, 1, 7, 7, 2, 1, 1, 16, 16)                    # 7x7 kernel
    co5 = (4, 32, 8, 8, 5, 5, 5, 2, 1, 1, 16, 16)                   # five channels on the layer onto the frame

    def call(geom, act, xp=None):
        return lib.bn_convT2d_last_bf16_u8(xp or x.data_ptr(), w.data_ptr(), None, out.data_ptr(), *geom, act, SLOPE, st)
    for g in (c8, k7, co5):
        assert call(g, SIGMOID) == -2 and not _hip.convT2d_bf16_ok(g, last=True)
    assert call(ok1, 9) == -2                                        # an activation the epilogue does not have
    assert call(ok1, SIGMOID, x.data_ptr() + 2) == -2                # a misaligned x
    torch.cuda.synchronize()
    _rest_is_sentinel(whole, 0, 0)


# ------------------------------------------------------------------------------------------ 3: whole models
N_FRAMES = 24
GOLDEN_OF_ALL = dict(GOLDEN_OF, **{'cond-ae': 'condae_cfg1', 'cond-vae': 'condvae_cfg1'})
CLASS_DIMS = [(c, (1, 64, 48)) for c in BUILDERS if c != 'conv-decoder'] + [('ps-vae', (2, 64, 48))]
LATENT_STD = 2.0          # (tests/test_gpu_frame_errors.py: what its _scaled_latents gives the decoder)


def test_every_model_class_is_covered():
    assert sorted(c for c, _ in CLASS_DIMS[:-1]) == sorted(GOLDEN_OF_ALL)


def _model(model_class, dim):
    _, meta = load_case(GOLDEN_OF_ALL[model_class])
    meta = dict(meta, dim=list(dim), n_frames=N_FRAMES, extra_hp=dict(meta['extra_hp']))
    meta['extra_hp'].pop('device', None)
    meta.pop('arch_json', None)
    from tests.cases import case_hparams, seeded_build
    model = seeded_build(BUILDERS[model_class], case_hparams(meta)).to(DEV)
    model.eval()
    labels = case_data(meta, device=DEV).get('labels')
    return model, meta, None if labels is None else labels[0].contiguous()


def _kwargs(model_class, labels, double=False):
    kw = {'dataset': 0}
    if model_class in ('vae', 'beta-tcvae', 'ps-vae', 'msps-vae', 'cond-vae'):
        kw['use_mean'] = True
    if model_class in ('cond-ae', 'cond-vae'):
        kw.update(labels=labels.double().cpu() if double else labels, labels_2d=None)
    return kw


def _widen_decoder_input(model, xd, kw):
    """A freshly initialised encoder hands its decoder latents of a few hundredths, and the decoder then draws an
    almost constant grey whatever its gain (``_scaled_latents`` of tests/test_gpu_frame_errors.py, which rewrites
    the encoders of four classes).  For EVERY class: the decoder's dense layer is rewritten so that it sees each
    column of its input -- latents, [A h | B h], [latents | labels] -- with zero mean and a standard deviation of
    LATENT_STD over these frames:  W' = W diag(s),  b' = b - W' mean,  s = LATENT_STD / std.  The oracle is loaded
    with the same parameters."""
    seen = []
    hook = model.decoding.register_forward_pre_hook(lambda mod, args: seen.append(args[0].detach().double().cpu()))
    try:
        with torch.no_grad():
            model(xd, **kw)
    finally:
        hook.remove()
    assert len(seen) == 1 and seen[0].dim() == 2 and seen[0].shape[1] == model.decoding.FF.in_features
    std, mean = seen[0].std(dim=0), seen[0].mean(dim=0)
    assert float(std.min()) > 0.0
    with torch.no_grad():
        ff = model.decoding.FF
        w = ff.weight.double().cpu() * (LATENT_STD / std)[None, :]
        ff.bias.copy_((ff.bias.double().cpu() - w @ mean).float())
        ff.weight.copy_(w.float())


@pytest.mark.parametrize('model_class,dim', CLASS_DIMS, ids=['%s-%d' % (c, d[0]) for c, d in CLASS_DIMS])
def test_whole_models(model_class, dim):
    model, meta, labels = _model(model_class, dim)
    apply_gain(model.decoding.decoder)
    xu = _frames(N_FRAMES, dim, 9, smooth=True)
    xd = xu.to(DEV)
    xf = (xd.float() / 255).contiguous()
    lab = labels if model_class in ('cond-ae', 'cond-vae') else None
    kw = _kwargs(model_class, labels)
    _widen_decoder_input(model, xd, kw)
    with torch.no_grad():
        ora = _oracle64(meta, model)(xu.double() / 255, **_kwargs(model_class, labels, double=True))[0]
    ora = ora.reshape(xu.shape)
    span = span_1_99(ora)
    # the fp32 lane: the model's own forward, quantised
    with warnings.catch_warnings():
        warnings.simplefilter('error', UserWarning)
        got = reconstruct_trial_device(model, xd, 0, labels=lab)
    assert got.is_cuda and got.dtype == torch.uint8 and got.shape == xu.shape
    with torch.no_grad():
        want = _hip.unit_float_to_u8(model(xd, **kw)[0].contiguous()).view(xu.shape)
        want_f = _hip.unit_float_to_u8(model(xf, **kw)[0].contiguous()).view(xu.shape)
    assert torch.equal(got, want)
    assert torch.equal(reconstruct_trial_device(model, xf, 0, labels=lab), want_f)
    assert torch.equal(reconstruct_trial_device(model, xd, 0, labels=lab, chunk_size=5), want)
    host = reconstruct_trial(model, xd, 0, labels=lab, chunk_size=200)
    assert host.dtype == np.uint8 and np.array_equal(host, want.cpu().numpy())
    err = float((want.cpu().double() - 255.0 * ora).abs().max())
    REPORT.append('fp32 lane %s %s: grey levels %d..%d, oracle x_hat 1..99%% span %.3f, max |u8 - 255 oracle| %.4f '
                  '(bound %.4f)' % (model_class, dim, int(want.min()), int(want.max()), span, err, GREY_TOL))
    assert span >= MIN_SPAN, 'the oracle reconstruction spans %.3f: not a usable yardstick' % span
    assert err <= GREY_TOL, err
    # both keys: the bf16 stacks, the grey levels written by the layer onto the frame
    with torch.no_grad(), hf.encode_precision('bf16'), hf.decode_precision('bf16'):
        want16 = _hip.unit_float_to_u8(model(xd, **kw)[0].contiguous()).view(xu.shape)
    with torch.no_grad(), hf.encode_precision('bf16'), hf.decode_precision('bf16'):
        want16_f = _hip.unit_float_to_u8(model(xf, **kw)[0].contiguous()).view(xu.shape)
    model.hparams.update(hip_encode_dtype='bf16', hip_decode_dtype='bf16')
    with warnings.catch_warnings():
        warnings.simplefilter('error', UserWarning)          # (an unserved stack would warn and run in fp32)
        got16 = reconstruct_trial_device(model, xd, 0, labels=lab)
        assert torch.equal(got16, want16)
        assert torch.equal(reconstruct_trial_device(model, xf, 0, labels=lab), want16_f)
        assert torch.equal(reconstruct_trial_device(model, xd, 0, labels=lab, chunk_size=5), want16)
        assert torch.equal(reconstruct_trial_device(model, xd[3:10], 0, labels=None if lab is None else lab[3:10]),
                           want16[3:10])
    diff = (got16.int() - want.int()).abs()
    REPORT.append('both keys %s %s: %.1f%% of the bytes differ from the fp32 lane, by %d grey levels at most'
                  % (model_class, dim, 100.0 * float((diff > 0).float().mean()), int(diff.max())))
    assert not torch.equal(got16, want)          # the bf16 code ran


@pytest.mark.parametrize('golden,why', [('ae_cfg1_bn', 'batch-norm'), ('ae_maxpool', 'max-pooling')])
def test_unserved_decoder_under_the_bf16_key(golden, why):
    n = 12
    model, meta = _small(golden=golden, n=n)
    x = case_data(meta, device=DEV)['images'][0].contiguous()
    want = reconstruct_trial_device(model, x, 0).clone()
    with torch.no_grad():
        assert torch.equal(want, _hip.unit_float_to_u8(model(x, dataset=0)[0].contiguous()).view(want.shape))
    model.hparams['hip_decode_dtype'] = 'bf16'
    with pytest.warns(UserWarning, match=why) as rec:
        got = reconstruct_trial_device(model, x, 0)
        again = reconstruct_trial_device(model, x[:5], 0)
    assert len([w for w in rec if 'bf16 decoding' in str(w.message)]) == 1
    assert torch.equal(got, want) and torch.equal(again, want[:5])


# ------------------------------------------------------------------------------------------ 4: get_reconstruction
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('model_class', ['ae', 'ps-vae'])
def test_get_reconstruction_as_uint8(model_class, dtype):
    dim = (2, 64, 48) if model_class == 'ps-vae' else (1, 64, 48)
    model, meta = _small(model_class, dim, N_FRAMES)
    apply_gain(model.decoding.decoder)
    if dtype == 'bf16':
        model.hparams['hip_decode_dtype'] = 'bf16'
    xf = (_frames(N_FRAMES, dim, 4, smooth=True).float() / 255).to(DEV)
    z = torch.randn((N_FRAMES, model.decoding.FF.in_features), generator=torch.Generator().manual_seed(3)).to(DEV)
    before_img = get_reconstruction(model, xf, dataset=0)
    before_lat, lat0 = get_reconstruction(model, z, apply_inverse_transform=False, return_latents=True)
    with warnings.catch_warnings():
        warnings.simplefilter('error', UserWarning)
        u8_img, lat_img = get_reconstruction(model, xf, dataset=0, return_latents=True, as_uint8=True)
        u8_lat, lat1 = get_reconstruction(model, z, apply_inverse_transform=False, return_latents=True, as_uint8=True)
    assert u8_img.dtype == np.uint8 and u8_lat.dtype == np.uint8
    assert np.array_equal(u8_img, quantise_u8(before_img)) and np.array_equal(u8_lat, quantise_u8(before_lat))
    assert lat_img.dtype == np.float32 and np.array_equal(lat0, lat1)
    assert len(np.unique(u8_img)) > 8
    # the default call has the bits it had before any uint8 call
    assert np.array_equal(get_reconstruction(model, xf, dataset=0), before_img)
    assert np.array_equal(get_reconstruction(model, z, apply_inverse_transform=False), before_lat)
    assert before_img.dtype == np.float32 and hf.frame_u8_request() is None


# ------------------------------------------------------------------------------------------ 5: nothing else moves
def _tiny_generator(dim, device=DEV):
    sess = SyntheticSession(7, [6, 9, 6, 9, 6, 9, 6], list(dim), seed=4, trial_splits='2;1;1;1')
    return SyntheticSessionsGenerator([sess], device=device, placement='device_u8')


@pytest.mark.parametrize('model_class', ['ae', 'ps-vae'])
def test_quantising_frames_moves_nothing_else(model_class, tmp_path):
    """loss() in eval and training mode (with gradients), forward(), a bare model.decoding(z), encode_trial_device,
    frame_errors_device and the default get_reconstruction give the same bits with quantising calls in between as
    without, both keys set."""
    dim = (2, 64, 48) if model_class == 'ps-vae' else (1, 64, 48)
    n = 24
    xu = _frames(n, dim, 5).to(DEV)
    xf = (xu.float() / 255).contiguous()
    res = {}
    for quantising in (False, True):
        model, meta = _small(model_class, dim, n)
        model.hparams.update(hip_decode_dtype='bf16', hip_encode_dtype='bf16')
        model.version = 0
        z = torch.randn((n, model.decoding.FF.in_features), generator=torch.Generator().manual_seed(3)).to(DEV)

        def quantise():
            if not quantising:
                return
            reconstruct_trial_device(model, xu, 0)
            reconstruct_trial_device(model, xf, 0, chunk_size=7)
            get_reconstruction(model, xf, dataset=0, as_uint8=True)
            get_reconstruction(model, z, apply_inverse_transform=False, as_uint8=True)
            export_reconstructions(_tiny_generator(dim), model, filename=os.path.join(str(tmp_path), 'r.npz'))
        data = {'images': xf[None]}
        if meta['n_labels']:
            g = torch.Generator().manual_seed(2)
            data['labels'] = torch.randn((1, n, meta['n_labels']), generator=g).to(DEV)
        out = {}
        quantise()
        model.eval()
        torch.manual_seed(1)
        ev = model.loss(data, dataset=0, accumulate_grad=False)
        out['eval_loss'] = {k: float(v) for k, v in dict(ev).items()}
        quantise()
        model.eval()
        torch.manual_seed(1)
        with torch.no_grad():
            fw = model(xf, dataset=0, use_mean=True) if model_class != 'ae' else model(xf, dataset=0)
            out['decoding'] = model.decoding(z, None, None, dataset=0).clone()
        out['forward'] = [t.clone() for t in fw if torch.is_tensor(t)]
        quantise()
        out['latents'] = encode_trial_device(model, xu, 0, None, 1024).clone()
        out['errors'] = frame_errors_device(model, xu, 0).clone()
        out['recon'] = torch.from_numpy(get_reconstruction(model, z, apply_inverse_transform=False))
        out['recon_img'] = torch.from_numpy(get_reconstruction(model, xf, dataset=0))
        quantise()
        model.train()
        model.zero_grad()
        torch.manual_seed(1)
        tr = model.loss(data, dataset=0, accumulate_grad=True)
        out['train_loss'] = {k: float(v) for k, v in dict(tr).items()}
        out['grads'] = [p.grad.clone() for p in model.parameters() if p.grad is not None]
        res[quantising] = out
    a, b = res[False], res[True]
    assert a['eval_loss'] == b['eval_loss'] and a['train_loss'] == b['train_loss']
    for k in ('decoding', 'latents', 'errors', 'recon', 'recon_img'):
        assert torch.equal(a[k], b[k]), k
    assert len(a['forward']) == len(b['forward']) and len(a['grads']) == len(b['grads']) > 0
    for s, t in zip(a['forward'] + a['grads'], b['forward'] + b['grads']):
        assert torch.equal(s, t)
    # the request reaches nobody outside its block, and nobody without the decode key
    assert hf.frame_u8_request() is None
    model.eval()
    with torch.no_grad(), hf.quantising_frames() as req:
        x_hat = model.decoding(z, None, None, dataset=0)
    assert req.frames is None and x_hat.dtype == torch.float32 and torch.equal(x_hat, a['decoding'])
    # inside the decode context it is served ...
    with torch.no_grad(), hf.decode_precision('bf16'):
        x16 = model.decoding(z, None, None, dataset=0)
        with hf.quantising_frames() as req:
            assert model.decoding(z, None, None, dataset=0) is None
    assert torch.equal(req.frames, _hip.unit_float_to_u8(x16))
    # ... but never together with a scoring request
    with torch.no_grad(), hf.decode_precision('bf16'), hf.quantising_frames() as req:
        with pytest.raises(RuntimeError, match='quantising request is open'):
            with hf.scoring_frames(xu, None, 1.0):
                model.decoding(z, None, None, dataset=0)
    with hf.scoring_frames(xu, None, 1.0) as sreq:
        with pytest.raises(RuntimeError, match='scoring request is open'):
            with hf.quantising_frames():
                pass
    assert req.frames is None and sreq.scores is None
    assert hf.frame_u8_request() is None and hf.frame_err_request() is None


# ------------------------------------------------------------------------------------------ 6: the export
@pytest.mark.parametrize('keys', [(), ('hip_decode_dtype', 'hip_encode_dtype')], ids=['f32', 'bf16'])
def test_export_reconstructions_end_to_end(tmp_path, keys, monkeypatch):
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
    lens = [24, 7, 24, 7, 24, 7, 24, 7, 24, 7]
    ids, paths, trials = [], [], []
    for s in range(2):
        trials.append([rng.integers(0, 255, size=(t,) + tuple(dim), dtype=np.uint8) for t in lens])
        sess_dir = os.path.join(root, 'lab', 'expt', 'animal', 'sess%d' % s)
        write_npz_session(os.path.join(sess_dir, 'data.npz'), {'images': trials[s]})
        ids.append({'lab': 'lab', 'expt': 'expt', 'animal': 'animal', 'session': 'sess%d' % s})
        paths.append([os.path.join(sess_dir, 'data.npz')])

    def generator(paths_list):
        return ConcatSessionsGenerator(root, ids, signals_list=[['images']] * 2, transforms_list=[[None]] * 2,
                                       paths_list=paths_list, device='cuda', placement='host_u8', keep_in_memory=False,
                                       trial_splits={'train_tr': 5, 'val_tr': 1, 'test_tr': 1, 'gap_tr': 1})
    gen = generator(paths)
    want_files = [os.path.join(root, 'version_0', 'lab_expt_animal_sess%d_reconstructions.npz' % s) for s in range(2)]
    # a rank that is not rank 0 does nothing at all
    asked = []
    real = gen.next_batch
    with monkeypatch.context() as m:
        m.setattr(gen, 'next_batch', lambda *a, **k: (asked.append(a), real(*a, **k))[1])
        m.setattr(bdist, 'world_size', lambda: 2)
        m.setattr(bdist, 'rank', lambda: 1)
        assert export_reconstructions(gen, hip) == [] and asked == []
        assert os.listdir(os.path.join(root, 'version_0')) == []
        # rank 0 of 2 writes every trial (checked below like the single-process files)
        m.setattr(bdist, 'rank', lambda: 0)
        with warnings.catch_warnings():
            warnings.simplefilter('error', UserWarning)
            files0 = export_reconstructions(gen, hip)
    assert files0 == want_files

    def check(files):
        n_gap = 0
        for s, path in enumerate(files):
            used = set(int(t) for k in ('train', 'val', 'test') for t in gen.datasets[s].batch_idxs[k])
            store = open_trial_store(path)
            try:
                assert store.signals() == ['images'] and store.n_trials('images') == len(lens)
                for i, t in enumerate(lens):
                    got = store.read('images', i)
                    assert store.layout('images', i) is not None and got.dtype == np.uint8
                    if i not in used:
                        n_gap += 1
                        assert got.shape == (0,) + tuple(dim)
                        continue
                    want = reconstruct_trial(hip, torch.from_numpy(trials[s][i]).to(DEV), s, chunk_size=1024)
                    assert got.shape == (t,) + tuple(dim) and np.array_equal(got, want), (s, i)
            finally:
                store.close()
        assert n_gap > 0
    check(files0)
    for f in files0:
        os.remove(f)
    hip.hparams['export_chunk_frames'] = 16          # (24-frame trials in two passes: the same bytes)
    with warnings.catch_warnings():
        warnings.simplefilter('error', UserWarning)
        files = export_reconstructions(gen, hip)
    assert files == want_files and sorted(os.listdir(os.path.join(root, 'version_0'))) == sorted(
        os.path.basename(f) for f in files)
    check(files)
    # a generator built on the written files serves the reconstructions as images
    again = generator([[f] for f in files])
    again.reset_iterators('val')
    data, s_ = again.next_batch('val')
    idx = int(data['batch_idx'])
    served = data['images'][0]
    store = open_trial_store(files[s_])
    try:
        stored = torch.from_numpy(store.read('images', idx))
    finally:
        store.close()
    assert stored.shape[0] == lens[idx]
    if served.dtype == torch.uint8:
        assert torch.equal(served.cpu(), stored)
    else:
        assert torch.equal(served.cpu(), stored.float() / 255)


def test_fit_writes_the_reconstructions(tmp_path):
    dim = [1, 32, 32]
    arch = load_handcrafted_arch(list(dim), 8, None, check_memory=False)
    hp = base_hparams(arch, 'ae', None)
    hp.update({'expt_dir': str(tmp_path), 'max_n_epochs': 2, 'min_n_epochs': 0, 'val_check_interval': 1,
               'enable_early_stop': False, 'early_stop_history': 10, 'rng_seed_train': 0, 'export_latents': False,
               'export_reconstructions': True, 'progress_bar': False, 'device': 'cuda'})
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
    path = os.path.join(str(tmp_path), 'version_0', 'lab_expt_animal_sess_reconstructions.npz')
    assert os.path.exists(path) and not os.path.exists(path + '.tmp')
    assert not os.path.exists(path.replace('reconstructions.npz', 'latents.pkl'))
    store = open_trial_store(path)
    try:
        assert store.n_trials('images') == 10
        assert all(store.layout('images', t) == (np.dtype(np.uint8), (32, 1, 32, 32)) for t in range(10))
        gen.reset_iterators('test')
        data, s_ = gen.next_batch('test')
        want = reconstruct_trial(best, data['images'][0], s_)
        assert np.array_equal(store.read('images', int(data['batch_idx'])), want)
    finally:
        store.close()
