"""The opt-in bf16 decoder on the GPU (csrc/conv_bf16_dec.hip, hip_functions.convT_stack_bf16,
hparams['hip_decode_dtype']).

The yardstick is tests/bf16_decode_emulation.py: torch CPU ops in float64 on operands rounded to bf16, rounded again
wherever the HIP path rounds (checked against a per-pixel gather loop in tests/test_decode_bf16_cpu.py).  Bounds, the
encoder's (tests/test_gpu_encode_bf16.py), unchanged:

* fp32 output of one layer on bf16-exact operands: ``tests.test_gpu_kernels.close``;
* bf16 output: ``check_bf16_output`` -- every element within 2^-8 |ref64| plus what ``close`` grants, at most 2e-3 of
  the elements on another bf16 value than RNE(ref64) (the CPU fp32 reference is held to 1e-3 first);
* whole decoder, on max|dx_hat| / max|x_hat|: against the emulation 4 x the spread the emulation itself shows between
  fp32 and float64 accumulation for the case at hand; against the exact float64 oracle 2 x the emulation's own error.
  A freshly initialised decoder draws an almost constant grey, so every transposed-conv weight is multiplied by GAIN
  first and the oracle's 1st-to-99th percentile span is asserted (tests/bf16_decode_cases.py).
"""

import warnings

import pytest
import torch
import torch.nn.functional as F

from behavenet_amd import _hip
from behavenet_amd import hip_functions as hf
from behavenet_amd.fitting.eval import encode_trial_device, get_reconstruction
from behavenet_amd.fitting.optim import FlatAdamAMSGrad
from oracle import ref_cpu
from tests import bf16_decode_emulation as demu
from tests import test_gpu_encode_bf16 as enc_tests
from tests.bf16_decode_cases import (BODY_CASES, DEC_CLASSES, DEC_FRAMES, DEFAULT_DIMS, MIN_SPAN, apply_gain, body_geom,
                                     body_operands, dec_dim, decoder_latents, decoder_plan, span_1_99)
from tests.cases import case_data, case_hparams, load_case, seeded_build
from tests.test_gpu_encode_bf16 import _frames, _meta, _rel, _small, check_bf16_output, guarded_bf16
from tests.test_gpu_guard_bands import guarded, finite, _bands_stay_untouched  # noqa: F401
from tests.test_gpu_kernels import close
from tests.test_gpu_model import _pair

pytestmark = pytest.mark.gpu
DEV = 'cuda'
LRELU, SIGMOID, SLOPE = _hip.ACT_LRELU, _hip.ACT_SIGMOID, 0.05
REPORT = []     # figures printed at the end of the module (pytest -s) for profiles/decode_bf16.txt


def teardown_module(module):
    for line in REPORT:
        print('DECODE-FIGURE ' + line)


# ------------------------------------------------------------------------------------------ helpers
def packed_weights(w):
    nb = _hip.convT_pack_w_bf16_bytes(w.shape)
    wp = guarded(torch.zeros(nb // 4)).view(torch.uint8)
    return _hip.convT_pack_w_bf16(guarded(w), wp)


def run_body(geom, x, w, b, out_f32, act=LRELU):
    """One body layer between guard bands -> CPU fp32 (N, Co, Ho, Wo)."""
    N, Ci, Hi, Wi, Co, R, S, st, ct, cl, Ho, Wo = geom
    xd = guarded_bf16(x.permute(0, 2, 3, 1).contiguous())
    wp, bd = packed_weights(w), guarded(b)
    if out_f32:
        y = guarded(torch.zeros(N, Co, Ho, Wo))
        _hip.convT2d_fwd_bf16(xd, wp, bd, geom, act, SLOPE, True, out=y)
        finite(y, 'bf16 convT fp32 out')
        return y.cpu()
    assert Co % 2 == 0
    y = guarded(torch.zeros(N, Ho, Wo, Co // 2)).view(torch.bfloat16)
    _hip.convT2d_fwd_bf16(xd, wp, bd, geom, act, SLOPE, False, out=y)
    finite(y.float(), 'bf16 convT bf16 out')
    return y.float().permute(0, 3, 1, 2).contiguous().cpu()


def run_last(geom, x, w, b, act=SIGMOID):
    N, Ci, Hi, Wi, Co, R, S, st, ct, cl, Ho, Wo = geom
    xd = guarded_bf16(x.permute(0, 2, 3, 1).contiguous())
    y = guarded(torch.zeros(N, Co, Ho, Wo))
    _hip.convT2d_last_bf16(xd, guarded(w), guarded(b), geom, act, SLOPE, out=y)
    finite(y, 'bf16 last layer')
    return y.cpu()


def bf16_check(got16, ref32, ref64, name):
    """``check_bf16_output`` of the encoder tests; its report lines are copied under this module's prefix."""
    n0 = len(enc_tests.REPORT)
    try:
        check_bf16_output(got16, ref32, ref64, name)
    finally:
        REPORT.extend(enc_tests.REPORT[n0:])
        del enc_tests.REPORT[n0:]


# ------------------------------------------------------------------------------------------ helpers of the stack
def test_weight_pack_is_the_transposed_layout_bit_for_bit():
    for shape in [(80, 40, 5, 5), (16, 3, 4, 4), (48, 17, 3, 3), (512, 256, 5, 5)]:
        g = torch.Generator().manual_seed(shape[0])
        w = torch.randn(shape, generator=g)
        wp = packed_weights(w)
        got = wp.view(torch.bfloat16)[:w.numel()].view(shape[1], shape[2], shape[3], shape[0]).cpu()
        assert torch.equal(got, w.permute(1, 2, 3, 0).contiguous().to(torch.bfloat16)), shape


def test_stack_input_is_rounded_once_into_the_private_layout():
    for shape in [(7, 512, 2, 2), (3, 48, 5, 7), (1, 16, 1, 1)]:
        g = torch.Generator().manual_seed(shape[1])
        x = torch.randn(shape, generator=g) * 3
        y = guarded(torch.zeros(shape[0], shape[2], shape[3], shape[1] // 2)).view(torch.bfloat16)
        _hip.to_nhwc_bf16(guarded(x), out=y)
        assert torch.equal(y.cpu(), x.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)), shape


# ------------------------------------------------------------------------------------------ single body layers
@pytest.mark.parametrize('case', BODY_CASES, ids=[c[0] for c in BODY_CASES])
def test_body_layer(case):
    """bf16-exact operands between NaN guard bands, on poisoned LDS (conftest): fp32 and bf16 output."""
    name, seed = case[0], case[1]
    geom = body_geom(case)
    assert _hip.convT2d_bf16_ok(geom), (name, geom)
    x, w, b = body_operands(geom, seed)
    ref64 = demu.convT_layer(x, w, b, geom, demu.ACT_LRELU, torch.float64)
    ref32 = demu.convT_layer(x, w, b, geom, demu.ACT_LRELU, torch.float32)
    assert tuple(ref64.shape) == (geom[0], geom[4], geom[10], geom[11]), (name, ref64.shape, geom)
    got = run_body(geom, x, w, b, True)
    close(got, ref32, ref64, name=name + ' fp32 out')
    got16 = run_body(geom, x, w, b, False)
    bf16_check(got16, ref32, ref64, name + ' bf16 out')


def test_body_layer_sigmoid_and_no_activation():
    geom = body_geom(BODY_CASES[0])
    x, w, b = body_operands(geom, 77)
    for act in (demu.ACT_NONE, demu.ACT_SIGMOID):
        ref64 = demu.convT_layer(x, w, b, geom, act, torch.float64)
        ref32 = demu.convT_layer(x, w, b, geom, act, torch.float32)
        close(run_body(geom, x, w, b, True, act=act), ref32, ref64, name='body act %d' % act)


# ------------------------------------------------------------------------------------------ last layer
LAST_CASES = [('default %s convT4' % dim, 40 + dim[1], tuple(dim)) for dim in DEFAULT_DIMS] + \
             [('three channels 5x7 -> 10x14', 44, (7, 16, 5, 7, 3, 5, 5, 2, 1, 1, 10, 14)),
              # beyond the default: the stride-2 block kernel on an even kernel, on odd outputs behind a crop of 2 and
              # on 'valid' padding with output_padding; the per-phase kernel that serves every other stride
              ('k4 s2 6x6 -> 12x12', 45, (7, 16, 6, 6, 1, 4, 4, 2, 1, 1, 12, 12)),
              ('four channels, crop 2, odd 7x5', 46, (7, 16, 4, 3, 4, 5, 5, 2, 2, 2, 7, 5)),
              ('valid with output_padding', 47, (1, 16, 3, 3, 1, 5, 5, 2, 0, 0, 10, 10)),
              ('stride 1 k3 two channels', 48, (7, 16, 9, 5, 2, 3, 3, 1, 1, 1, 9, 5)),
              ('stride 5 k5', 49, (3, 32, 2, 3, 1, 5, 5, 5, 1, 1, 8, 13)),
              ('stride 3 k5 three channels 200 pixels a phase', 50, (2, 16, 14, 15, 3, 5, 5, 3, 1, 2, 42, 44))]


def _last_geom(case):
    return decoder_plan(case[2])[4].geom(7) if len(case[2]) == 3 else case[2]


@pytest.mark.parametrize('case', LAST_CASES, ids=[c[0] for c in LAST_CASES])
def test_last_layer(case):
    """bf16 activations, fp32 weights that are NOT rounded, sigmoid: fp32 accuracy against float64."""
    name, seed = case[0], case[1]
    geom = _last_geom(case)
    assert _hip.convT2d_bf16_ok(geom, last=True), (name, geom)
    x, w, b = body_operands(geom, seed, exact_weights=False)
    assert not torch.equal(w, demu.rne_bf16(w))
    ref64 = demu.convT_layer(x, w, b, geom, demu.ACT_SIGMOID, torch.float64)
    ref32 = demu.convT_layer(x, w, b, geom, demu.ACT_SIGMOID, torch.float32)
    close(run_last(geom, x, w, b), ref32, ref64, name=name)


def test_last_layer_with_per_session_weights():
    """The layer onto the frame of a ``fit_sess_io_layers`` model, dataset 1."""
    model, meta = _small('ae', (1, 64, 48), 8, extra={'fit_sess_io_layers': True, 'n_datasets': 2})
    dec = model.decoding
    w0, w1 = dec._stack_params(0)[-2], dec._stack_params(1)[-2]
    assert not torch.equal(w0, w1)
    geom = dec._plan[-1].geom(7)
    x, _, _ = body_operands(geom, 9)
    w, b = (w1 * 8).detach().cpu(), dec._stack_params(1)[-1].detach().cpu()
    ref64 = demu.convT_layer(x, w, b, geom, demu.ACT_SIGMOID, torch.float64)
    ref32 = demu.convT_layer(x, w, b, geom, demu.ACT_SIGMOID, torch.float32)
    assert span_1_99(ref64) > 0.1
    close(run_last(geom, x, w, b), ref32, ref64, name='per-session last layer')


# ------------------------------------------------------------------------------------------ refusals
def test_unserved_geometry_is_refused_and_writes_nothing():
    lib = _hip.load()
    x = torch.zeros((4, 8, 8, 32), dtype=torch.bfloat16, device=DEV)
    wp = torch.zeros(32 * 32 * 49 * 4, dtype=torch.uint8, device=DEV)
    y = torch.full((4, 32, 16, 16), 7.0, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    ok = (4, 32, 8, 8, 32, 5, 5, 2, 1, 1, 16, 16)
    c8 = (4, 8, 8, 8, 32, 5, 5, 2, 1, 1, 16, 16)                    # 8 input channels: not a multiple of 16
    k7 = (4, 32, 8, 8, 32, 7, 7, 2, 1, 1, 16, 16)                   # 7x7 kernel
    co5 = (4, 32, 8, 8, 5, 5, 5, 2, 1, 1, 16, 16)                   # five channels on the layer onto the frame
    for g in (c8, k7):
        assert lib.bn_convT2d_fwd_bf16(x.data_ptr(), wp.data_ptr(), None, y.data_ptr(), 1, *g, LRELU, SLOPE, st) == -2
        assert lib.bn_convT2d_fwd_bf16(x.data_ptr(), wp.data_ptr(), None, y.data_ptr(), 0, *g, LRELU, SLOPE, st) == -2
    for g in (c8, k7, co5):
        assert lib.bn_convT2d_last_bf16(x.data_ptr(), wp.data_ptr(), None, y.data_ptr(), *g, SIGMOID, SLOPE, st) == -2
    # an activation the epilogue does not have
    assert lib.bn_convT2d_fwd_bf16(x.data_ptr(), wp.data_ptr(), None, y.data_ptr(), 1, *ok, 9, SLOPE, st) == -2
    ok1 = ok[:4] + (1,) + ok[5:]
    assert lib.bn_convT2d_last_bf16(x.data_ptr(), wp.data_ptr(), None, y.data_ptr(), *ok1, 9, SLOPE, st) == -2
    # a misaligned operand
    assert lib.bn_convT2d_fwd_bf16(x.data_ptr() + 2, wp.data_ptr(), None, y.data_ptr(), 1, *ok, LRELU, SLOPE, st) == -2
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())


# ------------------------------------------------------------------------------------------ whole decoder
def _apply_gain(decoding):
    apply_gain(decoding.decoder)


def _oracle64(meta, hip):
    """The float64 oracle with the HIP model's parameters as they are now."""
    ora64 = seeded_build(ref_cpu.build_model, case_hparams(meta)).double().eval()
    ora64.load_state_dict({k: v.detach().double().cpu() for k, v in hip.state_dict().items()})
    return ora64


def _emulations(decoding, ora_dec, lat):
    """(emulation float64, emulation fp32, exact float64 oracle) for the latents ``lat`` (CPU)."""
    lat = lat.double()
    start = decoding.hparams['ae_decoding_starting_dim']
    with torch.no_grad():
        h = F.linear(lat, ora_dec.FF.weight, ora_dec.FF.bias).view(-1, start[0], start[1], start[2])
        layers = demu.plan_layers(decoding)
        return (demu.stack_output(layers, h, torch.float64), demu.stack_output(layers, h.float(), torch.float32),
                ora_dec(lat, dataset=0))


DEC_CASES = [(mc, n) for mc in DEC_CLASSES for n in DEC_FRAMES]


@pytest.mark.parametrize('model_class,n', DEC_CASES)
def test_whole_decoder_against_emulation_and_oracle(model_class, n):
    """``get_reconstruction`` from latents.  (apply_inverse_transform=False: the N(0, 1) latents reach every class's
    decoder as they are -- the label-aware classes' inverse transforms divide by freshly initialised weights and
    would hand their decoders other ranges; they are fp32 code that this feature does not touch.)"""
    dim = dec_dim(model_class)
    meta = _meta(model_class, dim, n)
    hip, _, hp = _pair(meta)
    hip.eval()
    _apply_gain(hip.decoding)
    ora64 = _oracle64(meta, hip)
    z = decoder_latents(n, hip.decoding.FF.in_features).to(DEV)
    hip.hparams['hip_decode_dtype'] = 'bf16'
    with warnings.catch_warnings():
        warnings.simplefilter('error', UserWarning)
        x16, lat = get_reconstruction(hip, z, return_latents=True, apply_inverse_transform=False)
    x16, lat = torch.from_numpy(x16), torch.from_numpy(lat)
    assert torch.equal(lat, z.cpu())
    x_e64, x_e32, x_exact = _emulations(hip.decoding, ora64.decoding, lat)
    assert x16.shape == x_exact.shape == (n,) + tuple(dim)
    span = span_1_99(x_exact)
    spread, e_emul = _rel(x_e32, x_e64), _rel(x_e64, x_exact)
    e_hip_emul, e_hip_exact = _rel(x16, x_e64), _rel(x16, x_exact)
    hip.hparams['hip_decode_dtype'] = 'f32'
    x32 = torch.from_numpy(get_reconstruction(hip, z, apply_inverse_transform=False))
    REPORT.append('%s N=%d: hip vs emulation %.2e (emulation fp32-vs-f64 spread %.2e), hip vs float64 oracle %.2e '
                  '(emulation vs oracle %.2e), fp32 path vs oracle %.2e, oracle x_hat 1..99%% span %.3f'
                  % (model_class, n, e_hip_emul, spread, e_hip_exact, e_emul, _rel(x32, x_exact), span))
    assert span >= MIN_SPAN, 'the oracle reconstruction spans %.3f: not a usable yardstick' % span
    assert _rel(x32, x_exact) <= 1e-4
    assert not torch.equal(x32, x16)
    assert e_hip_emul <= 4 * spread, 'hip vs emulation %.3e, allowed 4 x %.3e' % (e_hip_emul, spread)
    assert e_hip_exact <= 2 * e_emul, 'hip vs oracle %.3e, allowed 2 x %.3e' % (e_hip_exact, e_emul)


def test_conv_decoder_is_served_inside_the_context():
    """``ConvDecoder`` (labels -> frames): its forward inside ``decode_precision('bf16')``."""
    _, meta = load_case('convdecoder_cfg1')
    hip, _, hp = _pair(meta)
    hip.eval()
    _apply_gain(hip.decoding)
    ora64 = _oracle64(meta, hip)
    labels = case_data(meta)['labels'][0][:40]
    with torch.no_grad():
        x32 = hip(labels.to(DEV), dataset=0).cpu()
        with warnings.catch_warnings():
            warnings.simplefilter('error', UserWarning)
            with hf.decode_precision('bf16'):
                x16 = hip(labels.to(DEV), dataset=0).cpu()
    x_e64, x_e32, x_exact = _emulations(hip.decoding, ora64.decoding, labels)
    spread, e_emul = _rel(x_e32, x_e64), _rel(x_e64, x_exact)
    REPORT.append('conv-decoder N=40: hip vs emulation %.2e (spread %.2e), hip vs float64 oracle %.2e (emulation vs '
                  'oracle %.2e)' % (_rel(x16, x_e64), spread, _rel(x16, x_exact), e_emul))
    assert _rel(x32, x_exact) <= 1e-4 and not torch.equal(x32, x16)
    assert _rel(x16, x_e64) <= 4 * spread
    assert _rel(x16, x_exact) <= 2 * e_emul


# ------------------------------------------------------------------------------------------ nothing existing moves
@pytest.mark.parametrize('model_class', ['ae', 'vae', 'ps-vae'])
def test_hparam_changes_nothing_but_get_reconstruction(model_class):
    """loss() in eval and training mode (with gradients), forward(), a bare model.decoding(z) and the latent
    exporters give the same bits with hparams['hip_decode_dtype'] = 'bf16' as without the key; without the key or
    with 'f32', get_reconstruction is the bare fp32 decoder."""
    dim = (2, 64, 48) if model_class == 'ps-vae' else (1, 64, 48)
    n = 24
    xf = (_frames(n, dim, 5).float() / 255).to(DEV)
    res = {}
    for key in (None, 'bf16'):
        model, meta = _small(model_class, dim, n)
        if key:
            model.hparams['hip_decode_dtype'] = key
        data = {'images': xf[None]}
        if meta['n_labels']:
            g = torch.Generator().manual_seed(2)
            data['labels'] = torch.randn((1, n, meta['n_labels']), generator=g).to(DEV)
        z = torch.randn((n, model.decoding.FF.in_features), generator=torch.Generator().manual_seed(3)).to(DEV)
        out = {}
        model.eval()
        torch.manual_seed(1)
        ev = model.loss(data, dataset=0, accumulate_grad=False)
        out['eval_loss'] = {k: float(v) for k, v in dict(ev).items()}
        torch.manual_seed(1)
        with torch.no_grad():
            fw = model(xf, dataset=0, use_mean=True) if model_class != 'ae' else model(xf, dataset=0)
            out['decoding'] = model.decoding(z, None, None, dataset=0).clone()
        out['forward'] = [t.clone() for t in fw if torch.is_tensor(t)]
        out['latents'] = encode_trial_device(model, xf, 0, None, 1024).clone()
        out['recon'] = torch.from_numpy(get_reconstruction(model, z, apply_inverse_transform=False))
        out['recon_img'] = torch.from_numpy(get_reconstruction(model, xf, dataset=0))
        model.train()
        model.zero_grad()
        torch.manual_seed(1)
        tr = model.loss(data, dataset=0, accumulate_grad=True)
        out['train_loss'] = {k: float(v) for k, v in dict(tr).items()}
        out['grads'] = [p.grad.clone() for p in model.parameters() if p.grad is not None]
        if key is None:
            model.hparams['hip_decode_dtype'] = 'f32'
            out['recon_f32_key'] = torch.from_numpy(get_reconstruction(model, z, apply_inverse_transform=False))
        res[key] = out
    a, b = res[None], res['bf16']
    assert a['eval_loss'] == b['eval_loss'] and a['train_loss'] == b['train_loss']
    assert torch.equal(a['decoding'], b['decoding']) and torch.equal(a['latents'], b['latents'])
    assert len(a['forward']) == len(b['forward']) and len(a['grads']) == len(b['grads']) > 0
    for s, t in zip(a['forward'] + a['grads'], b['forward'] + b['grads']):
        assert torch.equal(s, t)
    # without the key, and with 'f32': the parent's path, which is the bare decoder
    assert torch.equal(a['recon'], a['decoding'].cpu()) and torch.equal(a['recon_f32_key'], a['recon'])
    assert torch.equal(a['recon_img'], a['forward'][0].cpu())
    # with the key only get_reconstruction moves, in both of its branches
    assert not torch.equal(b['recon'], a['recon']) and not torch.equal(b['recon_img'], a['recon_img'])
    assert float((b['recon'] - a['recon']).abs().max()) < 0.02


def test_image_branch_keeps_the_encoder_in_fp32():
    """Images through the whole model: the latents are the fp32 encoder's whatever either key says, and the
    reconstruction is the bf16 decoder's of those latents."""
    model, meta = _small('ae', (1, 64, 48), 16)
    xf = (_frames(16, meta['dim'], 8).float() / 255).to(DEV)
    model.eval()
    with torch.no_grad():
        z32 = model.encoding(xf, dataset=0)[0].clone()
    model.hparams.update(hip_decode_dtype='bf16', hip_encode_dtype='bf16')
    recon, lat = get_reconstruction(model, xf, dataset=0, return_latents=True)
    assert torch.equal(torch.from_numpy(lat), z32.cpu())
    assert torch.equal(torch.from_numpy(recon), torch.from_numpy(get_reconstruction(model, z32)))


def test_context_manager_is_the_way_to_bf16_from_model_decoding():
    model, meta = _small('ae', (1, 64, 48), 16)
    model.eval()
    z = torch.randn((16, model.decoding.FF.in_features), generator=torch.Generator().manual_seed(4)).to(DEV)
    model.hparams['hip_decode_dtype'] = 'bf16'
    with torch.no_grad():
        bare = model.decoding(z, None, None, dataset=None).clone()
        with hf.decode_precision('bf16'):
            wrapped = model.decoding(z, None, None, dataset=None).clone()
        with hf.encode_precision('bf16'):                # the encoder's switch is not the decoder's
            other = model.decoding(z, None, None, dataset=None).clone()
    assert torch.equal(wrapped.cpu(), torch.from_numpy(get_reconstruction(model, z)))
    assert not torch.equal(bare, wrapped) and torch.equal(bare, other)
    # training mode: fp32 and exactly one warning
    model.train()
    with torch.no_grad(), hf.decode_precision('bf16'):
        with pytest.warns(UserWarning, match='training mode') as rec:
            t1 = model.decoding(z, None, None, dataset=None).clone()
            t2 = model.decoding(z, None, None, dataset=None).clone()
    assert len([w for w in rec if 'bf16 decoding' in str(w.message)]) == 1
    # (train() and eval() run the same kernels for a model without batch norm)
    assert torch.equal(t1, bare) and torch.equal(t2, bare)


# ------------------------------------------------------------------------------------------ fallbacks
@pytest.mark.parametrize('golden,why', [('ae_maxpool', 'max-pooling'), ('ae_cfg1_bn', 'batch-norm'),
                                        ('ae_linear', 'linear'), ('ae_cfg1_lastff', 'ae_decoding_last_FF_layer')])
def test_unserved_models_fall_back_to_fp32_with_one_warning(golden, why):
    n = 12
    model, meta = _small(golden=golden, n=n)
    model.eval()
    x = case_data(meta, device=DEV)['images'][0].contiguous()
    want = get_reconstruction(model, x, dataset=0)
    model.hparams['hip_decode_dtype'] = 'bf16'
    with pytest.warns(UserWarning, match=why) as rec:
        got = get_reconstruction(model, x, dataset=0)
        again = get_reconstruction(model, x[:5], dataset=0)
    assert len([w for w in rec if 'bf16 decoding' in str(w.message)]) == 1
    assert (got == want).all() and (again == want[:5]).all()


# ------------------------------------------------------------------------------------------ repeatability
def test_two_bf16_reconstructions_identical_bits():
    model, meta = _small('vae', (1, 128, 128), 64)
    model.eval()
    _apply_gain(model.decoding)
    model.hparams['hip_decode_dtype'] = 'bf16'
    z = torch.randn((64, model.decoding.FF.in_features), generator=torch.Generator().manual_seed(31)).to(DEV)
    a = torch.from_numpy(get_reconstruction(model, z))
    b = torch.from_numpy(get_reconstruction(model, z))
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------ no stale weights
def test_in_place_adam_steps_reach_the_next_reconstruction():
    model, meta = _small('ae', (1, 64, 48), 24)
    model.hparams['hip_decode_dtype'] = 'bf16'
    xf = (_frames(24, meta['dim'], 41).float() / 255).to(DEV).contiguous()
    z = torch.randn((24, model.decoding.FF.in_features), generator=torch.Generator().manual_seed(6)).to(DEV)
    first = torch.from_numpy(get_reconstruction(model, z))
    model.train()
    opt = FlatAdamAMSGrad(model.get_parameters(), lr=1e-2, weight_decay=0)
    for _ in range(2):
        opt.zero_grad()
        model.loss({'images': xf[None]}, dataset=0, accumulate_grad=True)
        opt.step()
    second = torch.from_numpy(get_reconstruction(model, z))
    fresh, _ = _small('ae', (1, 64, 48), 24)
    fresh.load_state_dict({k: v.clone() for k, v in model.state_dict().items()})
    fresh.hparams['hip_decode_dtype'] = 'bf16'
    assert torch.equal(second, torch.from_numpy(get_reconstruction(fresh, z)))
    assert not torch.equal(first, second)
