"""The opt-in bf16 decoder, host side (no GPU): which layers the library serves (bn_convT2d_*_bf16_ok), the
``decode_precision`` context and its independence of ``encode_precision``, the hparam's validation, the float64
emulation the GPU tests measure against (tests/bf16_decode_emulation.py) checked against a per-pixel gather loop
written here, and the share of the GPU tests' bounds that the CPU reference itself uses up."""

import os
import threading

import pytest
import torch
import torch.nn.functional as F

from behavenet_amd import _hip
from behavenet_amd import hip_functions as hf
from behavenet_amd.fitting import eval as hip_eval
from behavenet_amd.models import AE
from behavenet_amd.models.ae_model_architecture_generator import load_handcrafted_arch
from tests import bf16_decode_emulation as demu
from tests.bf16_decode_cases import (BODY_CASES, CPU_FLIP_CAP, DEC_CLASSES, DEC_FRAMES, MIN_SPAN, apply_gain, body_geom,
                                     body_operands, dec_dim, decoder_latents, decoder_plan, span_1_99)
from tests.bf16_emulation import rne_bf16
from tests.cases import seeded_build
from tests.golden_utils import base_hparams

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARCH2 = os.path.join(REPO, 'behavenet_amd', 'configs', 'ae_jsons', 'ae_arch_2.json')


# -- what is served ---------------------------------------------------------------------------
@pytest.mark.parametrize('dim', [[1, 128, 128], [2, 128, 128], [1, 64, 48], [2, 192, 160]])
def test_default_architecture_is_served(dim):
    plan = decoder_plan(dim)
    assert len(plan) == 5
    for layer in plan[:-1]:
        assert _hip.convT2d_bf16_ok(layer.geom(256)), layer
        assert _hip.convT2d_bf16_ok(layer.geom(1)), layer
    assert _hip.convT2d_bf16_ok(plan[-1].geom(256), last=True)
    assert hf.stack_unserved_reason_bf16_dec(plan) is None


def test_arch_2_is_served():
    plan = decoder_plan([1, 128, 128], ARCH2)
    assert hf.stack_unserved_reason_bf16_dec(plan) is None


def test_unserved_geometries_answer_no():
    # (N, Ci, Hi, Wi, Co, R, S, stride, crop_t, crop_l, Ho, Wo)
    assert _hip.convT2d_bf16_ok((4, 16, 8, 8, 32, 5, 5, 2, 1, 1, 16, 16))
    assert not _hip.convT2d_bf16_ok((4, 8, 8, 8, 32, 5, 5, 2, 1, 1, 16, 16))              # 8 input channels
    assert not _hip.convT2d_bf16_ok((4, 24, 8, 8, 32, 5, 5, 2, 1, 1, 16, 16))             # 24: not a multiple of 16
    assert not _hip.convT2d_bf16_ok((4, 32, 8, 8, 32, 7, 7, 2, 1, 1, 16, 16))             # kernel larger than 5x5
    assert not _hip.convT2d_bf16_ok((0, 32, 8, 8, 32, 5, 5, 2, 1, 1, 16, 16))             # empty batch
    assert _hip.convT2d_bf16_ok((4, 32, 8, 8, 3, 5, 5, 2, 1, 1, 16, 16), last=True)
    assert not _hip.convT2d_bf16_ok((4, 32, 8, 8, 5, 5, 5, 2, 1, 1, 16, 16), last=True)   # five frame channels
    assert not _hip.convT2d_bf16_ok((4, 8, 8, 8, 1, 5, 5, 2, 1, 1, 16, 16), last=True)
    lib = _hip.load()
    assert lib.bn_convT2d_fwd_bf16(None, None, None, None, 0, *([1] * 12), 0, 0.0, None) == -1
    assert lib.bn_convT2d_last_bf16(None, None, None, None, *([1] * 12), 0, 0.0, None) == -1
    assert lib.bn_convT_pack_w_bf16(None, None, 1, 1, 1, 1, None) == -1
    assert lib.bn_to_nhwc_bf16(None, None, 1, 1, 1, 1, None) == -1
    assert lib.bn_convT_pack_w_bf16_bytes(64, 32, 5, 5) == 64 * 32 * 25 * 2


def test_a_stack_names_the_layer_it_cannot_serve():
    plan = decoder_plan([1, 64, 48])
    bad = [hf.ConvLayerPlan('convT', 8, 4, 4, 16, 8, 8, 5, 5, 2, 1, 1, _hip.ACT_LRELU)] + plan[1:]
    assert 'layer 0' in hf.stack_unserved_reason_bf16_dec(bad)
    assert 'no transposed-conv stack' in hf.stack_unserved_reason_bf16_dec([])


# -- the switch -------------------------------------------------------------------------------
def test_decode_precision_nests_restores_and_is_independent_of_encode_precision():
    assert hf.decode_dtype() == 'f32' and hf.encode_dtype() == 'f32'
    with hf.decode_precision('bf16'):
        assert hf.decode_dtype() == 'bf16' and hf.encode_dtype() == 'f32'
        with hf.decode_precision('f32'):
            assert hf.decode_dtype() == 'f32'
        assert hf.decode_dtype() == 'bf16'
        with hf.encode_precision('bf16'):
            assert hf.decode_dtype() == 'bf16' and hf.encode_dtype() == 'bf16'
            with hf.decode_precision('f32'):
                assert hf.decode_dtype() == 'f32' and hf.encode_dtype() == 'bf16'
        assert hf.decode_dtype() == 'bf16' and hf.encode_dtype() == 'f32'
    assert hf.decode_dtype() == 'f32'
    with hf.encode_precision('bf16'):
        assert hf.decode_dtype() == 'f32' and hf.encode_dtype() == 'bf16'
    with pytest.raises(RuntimeError):
        with hf.decode_precision('bf16'):
            raise RuntimeError('x')
    assert hf.decode_dtype() == 'f32'
    with pytest.raises(ValueError):
        with hf.decode_precision('fp16'):
            pass
    seen = []
    with hf.decode_precision('bf16'):
        t = threading.Thread(target=lambda: seen.append(hf.decode_dtype()))
        t.start()
        t.join()
    assert seen == ['f32']
    assert hf.DECODE_DTYPES == ('f32', 'bf16')


def test_unknown_dtype_raises_before_any_device_call(monkeypatch):
    arch = load_handcrafted_arch([1, 32, 32], 8, None, check_memory=False)
    model = seeded_build(AE, base_hparams(arch, 'ae', {}))
    model.hparams['hip_decode_dtype'] = 'fp16'

    def no_library():
        raise AssertionError('the library was reached')
    monkeypatch.setattr(_hip, 'load', no_library)
    with pytest.raises(ValueError, match='hip_decode_dtype'):
        hip_eval.get_reconstruction(model, torch.zeros(4, 8))
    with pytest.raises(ValueError, match='hip_decode_dtype'):
        hip_eval.get_reconstruction(model, torch.zeros(4, 1, 32, 32))
    model.hparams.pop('hip_decode_dtype')
    monkeypatch.setenv('BN_DECODE_DTYPE', 'half')
    with pytest.raises(ValueError, match='BN_DECODE_DTYPE'):
        hip_eval.get_reconstruction(model, torch.zeros(4, 8))
    # the encoder's key is not the decoder's
    monkeypatch.delenv('BN_DECODE_DTYPE')
    model.hparams['hip_encode_dtype'] = 'bf16'
    assert hip_eval.decode_dtype_of(model) == 'f32'
    model.hparams['hip_decode_dtype'] = 'bf16'
    assert hip_eval.decode_dtype_of(model) == 'bf16'


def test_convT_stack_bf16_refuses_gradients():
    plan = decoder_plan([1, 32, 32])
    w = torch.zeros(1, requires_grad=True)
    with pytest.raises(RuntimeError, match='inference only'):
        hf.convT_stack_bf16(plan, torch.zeros(2, plan[0].cin, plan[0].hin, plan[0].win), [w] * (2 * len(plan)))


# -- the yardstick itself ---------------------------------------------------------------------
def gather_layer(x, w, b, geom):
    """The gather formula of the kernels, one output pixel at a time, float64, no activation: with f = o + crop,
    tap r contributes iff f - r >= 0, (f - r) % stride == 0 and (f - r) / stride < Hin."""
    N, Ci, Hi, Wi, Co, R, S, st, ct, cl, Ho, Wo = geom
    x, w = x.double(), w.double()
    y = torch.zeros((N, Co, Ho, Wo), dtype=torch.float64)
    for oy in range(Ho):
        for ox in range(Wo):
            fy, fx = oy + ct, ox + cl
            acc = torch.zeros((N, Co), dtype=torch.float64)
            for r in range(R):
                if fy - r < 0 or (fy - r) % st or (fy - r) // st >= Hi:
                    continue
                for s in range(S):
                    if fx - s < 0 or (fx - s) % st or (fx - s) // st >= Wi:
                        continue
                    acc += x[:, :, (fy - r) // st, (fx - s) // st] @ w[:, :, r, s]
            y[:, :, oy, ox] = acc + b.double()
    return y


def _module_output(x, w, b, k, st, padding, output_padding, crop):
    """nn.ConvTranspose2d as the models build it (ConvAEDecoder._get_convtranspose2d_args), then the reference's
    crop with negative F.pad."""
    y = F.conv_transpose2d(x.double(), w.double(), b.double(), stride=st, padding=padding, output_padding=output_padding)
    if crop is not None:
        y = F.pad(y, [-c for c in crop])
    return y


PADDING_MODES = [
    # name, k, stride, Hi, Wi, module padding, output_padding, crop [x0, x1, y0, y1] or None, (crop_t, crop_l)
    ('same symmetric', 5, 5, 2, 3, (1, 1), 0, None, (1, 1)),
    ('same asymmetric', 5, 2, 4, 3, 0, 0, [1, 2, 1, 2], (1, 1)),
    ('same asymmetric k4', 4, 2, 3, 4, 0, 0, [0, 2, 2, 0], (2, 0)),
    ('valid', 5, 2, 3, 3, (0, 0), (1, 1), None, (0, 0)),
    ('valid padded', 3, 2, 4, 3, (1, 1), (1, 0), None, (1, 1)),
    ('stride 1', 3, 1, 5, 4, (1, 1), 0, None, (1, 1)),
]


@pytest.mark.parametrize('mode', PADDING_MODES, ids=[m[0] for m in PADDING_MODES])
def test_gather_formula_module_and_emulation_agree(mode):
    name, k, st, hi, wi, padding, opad, crop, (ct, cl) = mode
    g = torch.Generator().manual_seed(len(name))
    x = torch.randn((2, 3, hi, wi), generator=g)
    w = torch.randn((3, 4, k, k), generator=g)
    b = torch.randn((4,), generator=g)
    want = _module_output(x, w, b, k, st, padding, opad, crop)
    geom = (2, 3, hi, wi, 4, k, k, st, ct, cl, want.shape[2], want.shape[3])
    got = gather_layer(x, w, b, geom)
    assert float((got - want).abs().max()) <= 1e-12
    em = demu.convT_layer(x, w, b, geom, demu.ACT_NONE, torch.float64)
    assert float((em - want).abs().max()) <= 1e-12
    if 'valid' in name:
        # pixels past the full size hold the bias alone
        full_h = (hi - 1) * st + k
        if ct + want.shape[2] > full_h:
            assert torch.equal(got[:, :, full_h - ct:, :], b.double().view(1, 4, 1, 1).expand(2, 4, -1, want.shape[3]))


def test_emulated_stack_rounds_where_the_device_rounds():
    """Two 1x1 stride-1 layers worked out by hand.  t = 1 + 2^-8 is a tie that goes to 1, u = 1 + 2^-7 is a bf16
    value.  Body layer then frame layer: input rounded, body weight rounded, body output rounded; the frame
    layer's weight and output are NOT."""
    t, u = 1.00390625, 1.0078125
    g1 = (1, 1, 1, 1, 8, 1, 1, 1, 0, 0, 1, 1)          # 1 -> 8 channels: a body layer
    g2 = (1, 8, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1)          # 8 -> 1 channel: the layer onto the frame
    w1 = torch.zeros(1, 8, 1, 1)
    w1[0, 0] = t                                       # rounded to 1
    w1[0, 1] = u
    w2 = torch.zeros(8, 1, 1, 1)
    w2[0, 0] = t                                       # kept
    w2[1, 0] = 0.5
    layers = [(w1, torch.zeros(8), g1, demu.ACT_NONE), (w2, torch.tensor([0.25]), g2, demu.ACT_NONE)]
    # input t -> 1; channel 0: 1 * 1 = 1, channel 1: 1 * u = u (a bf16 value); frame: 1 * t + u * 0.5 + 0.25
    out = demu.stack_output(layers, torch.tensor([[[[t]]]]))
    assert out.item() == 1.0 * t + u * 0.5 + 0.25
    # input u: channel 1 = u * u = 1 + 2^-6 + 2^-14 -> rounded to 1 + 2^-6
    out = demu.stack_output(layers, torch.tensor([[[[u]]]]))
    assert out.item() == u * t + (1 + 2.0 ** -6) * 0.5 + 0.25
    # a stack that ends in a body layer (more than 4 channels) keeps that layer's output unrounded
    out = demu.stack_output(layers[:1], torch.tensor([[[[u]]]]))
    assert out[0, 1, 0, 0].item() == u * u and out[0, 0, 0, 0].item() == u
    # the activation follows in the accumulator's precision, before the rounding
    neg = [(w1, torch.zeros(8), g1, demu.ACT_LRELU), (w2, torch.tensor([0.0]), g2, demu.ACT_SIGMOID)]
    out = demu.stack_output(neg, torch.tensor([[[[-1.0]]]]))
    c0, c1 = rne_bf16(torch.tensor(-0.05, dtype=torch.float64)), rne_bf16(torch.tensor(-0.05 * u, dtype=torch.float64))
    assert out.item() == torch.sigmoid(c0 * t + c1 * 0.5).item()


# -- the reference's own share of the GPU bounds -------------------------------------------------
@pytest.mark.parametrize('case', BODY_CASES, ids=[c[0] for c in BODY_CASES])
def test_cpu_fp32_accumulation_stays_under_its_flip_cap(case):
    """For every single-layer case of the GPU file: CPU fp32 accumulation puts at most CPU_FLIP_CAP of the bf16
    outputs on another value than RNE(ref64) -- the reference's own share of the 2e-3 the GPU test allows."""
    name, seed = case[0], case[1]
    geom = body_geom(case)
    x, w, b = body_operands(geom, seed)
    ref64 = demu.convT_layer(x, w, b, geom, demu.ACT_LRELU, torch.float64)
    ref32 = demu.convT_layer(x, w, b, geom, demu.ACT_LRELU, torch.float32)
    assert tuple(ref64.shape) == (geom[0], geom[4], geom[10], geom[11])
    flips = float((rne_bf16(ref32.double()) != rne_bf16(ref64)).double().mean())
    assert flips <= CPU_FLIP_CAP, '%s: CPU fp32 accumulation flips %.2e of the bf16 outputs' % (name, flips)


@pytest.mark.parametrize('model_class', DEC_CLASSES)
def test_gain_gives_the_oracle_a_usable_range(model_class):
    """A freshly initialised decoder reconstructs an almost constant grey; with every transposed-conv weight times
    GAIN the float64 oracle's reconstruction of the GPU test's own latents spans at least MIN_SPAN between its 1st
    and 99th percentile, for every model class of the whole-decoder cases (the GPU test asserts the same again)."""
    from oracle import ref_cpu
    from tests.cases import case_hparams
    from tests.test_gpu_encode_bf16 import _meta
    meta = _meta(model_class, dec_dim(model_class), 40)
    ora = seeded_build(ref_cpu.build_model, case_hparams(meta)).double().eval()
    z = decoder_latents(40, ora.decoding.FF.in_features).double()
    with torch.no_grad():
        assert span_1_99(ora.decoding(z[:8], dataset=0)) < 0.1
        apply_gain(ora.decoding.decoder)
        for n in DEC_FRAMES:
            x = ora.decoding(decoder_latents(n, ora.decoding.FF.in_features).double(), dataset=0)
            assert span_1_99(x) >= MIN_SPAN, (n, span_1_99(x))
            assert 0.0 < float(x.min()) and float(x.max()) < 1.0
