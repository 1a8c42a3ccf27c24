"""The opt-in bf16 encoder, host side (no GPU): which layers the library serves (bn_conv2d_bf16_ok), the
``encode_precision`` context, the hparam's validation, and the float64 emulation the GPU tests measure against
(tests/bf16_emulation.py) checked on cases computed by hand."""

import os

import pytest
import torch

from behavenet_amd import _hip
from behavenet_amd import hip_functions as hf
from behavenet_amd.fitting import eval as hip_eval
from behavenet_amd.models import AE
from behavenet_amd.models.ae_model_architecture_generator import load_handcrafted_arch
from tests import bf16_emulation as emu
from tests.cases import seeded_build
from tests.golden_utils import base_hparams

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARCH2 = os.path.join(REPO, 'behavenet_amd', 'configs', 'ae_jsons', 'ae_arch_2.json')


def _plan(dim, arch_json=None):
    arch = load_handcrafted_arch(list(dim), 8, arch_json, check_memory=False)
    model = seeded_build(AE, base_hparams(arch, 'ae', {}))
    return model.encoding._plan


@pytest.mark.parametrize('dim', [[1, 128, 128], [2, 128, 128], [1, 64, 48], [2, 192, 160]])
def test_default_architecture_is_served(dim):
    plan = _plan(dim)
    assert len(plan) == 5
    assert _hip.conv2d_bf16_ok(plan[0].geom(256), first=True)
    for layer in plan[1:]:
        assert _hip.conv2d_bf16_ok(layer.geom(256)), layer
        assert _hip.conv2d_bf16_ok(layer.geom(1)), layer
    assert hf.stack_served_bf16(plan)


def test_arch_2_is_served():
    plan = _plan([1, 128, 128], ARCH2)
    assert len(plan) >= 5
    for layer in plan[1:]:
        assert _hip.conv2d_bf16_ok(layer.geom(256)), layer
    assert hf.stack_served_bf16(plan)


@pytest.mark.parametrize('cin', [1, 3, 8, 24])
def test_body_layers_need_sixteen_channels(cin):
    # (N, C, H, W, K, R, S, stride, pad_t, pad_l, P, Q)
    assert not _hip.conv2d_bf16_ok((4, cin, 16, 16, 32, 5, 5, 2, 1, 1, 8, 8))
    assert _hip.conv2d_bf16_ok((4, 16 * cin, 16, 16, 32, 5, 5, 2, 1, 1, 8, 8))


def test_unserved_geometries_answer_no():
    assert not _hip.conv2d_bf16_ok((4, 32, 16, 16, 32, 7, 7, 2, 1, 1, 8, 8))            # kernel larger than 5x5
    assert not _hip.conv2d_bf16_ok((0, 32, 16, 16, 32, 5, 5, 2, 1, 1, 8, 8))            # empty batch
    assert not _hip.conv2d_bf16_ok((4, 32, 16, 16, 32, 5, 5, 2, 1, 1, 40, 8))           # rows beyond the padded map
    assert not _hip.conv2d_bf16_ok((4, 5, 16, 16, 32, 5, 5, 2, 1, 1, 8, 8), first=True)   # 5 frame channels
    assert not _hip.conv2d_bf16_ok((4, 1, 16, 16, 24, 5, 5, 2, 1, 1, 8, 8), first=True)   # K not a multiple of 16
    lib = _hip.load()
    assert lib.bn_conv2d_fwd_bf16(None, None, None, None, 0, *([1] * 12), 0, 0.0, None) == -1
    assert lib.bn_conv2d_first_bf16(None, 0, None, None, None, *([1] * 12), 0, 0.0, None) == -1
    assert lib.bn_conv_pack_w_bf16(None, None, 1, 1, 1, 1, None) == -1
    assert lib.bn_conv_pack_w_bf16_bytes(64, 32, 5, 5) == 64 * 32 * 25 * 2


def test_encode_precision_nests_and_restores():
    assert hf.encode_dtype() == 'f32'
    with hf.encode_precision('bf16'):
        assert hf.encode_dtype() == 'bf16'
        with hf.encode_precision('f32'):
            assert hf.encode_dtype() == 'f32'
            with hf.encode_precision('bf16'):
                assert hf.encode_dtype() == 'bf16'
            assert hf.encode_dtype() == 'f32'
        assert hf.encode_dtype() == 'bf16'
    assert hf.encode_dtype() == 'f32'
    with pytest.raises(RuntimeError):
        with hf.encode_precision('bf16'):
            raise RuntimeError('x')
    assert hf.encode_dtype() == 'f32'
    with pytest.raises(ValueError):
        with hf.encode_precision('fp16'):
            pass
    # thread-local: another thread starts at the default
    import threading
    seen = []
    with hf.encode_precision('bf16'):
        t = threading.Thread(target=lambda: seen.append(hf.encode_dtype()))
        t.start()
        t.join()
    assert seen == ['f32']


def test_unknown_dtype_raises_before_any_device_call(monkeypatch):
    arch = load_handcrafted_arch([1, 32, 32], 8, None, check_memory=False)
    model = seeded_build(AE, base_hparams(arch, 'ae', {}))
    model.hparams['hip_encode_dtype'] = 'fp8'

    def no_library():
        raise AssertionError('the library was reached')
    monkeypatch.setattr(_hip, 'load', no_library)
    with pytest.raises(ValueError, match='hip_encode_dtype'):
        hip_eval.encode_trial_device(model, torch.zeros(4, 1, 32, 32))
    model.hparams.pop('hip_encode_dtype')
    monkeypatch.setenv('BN_ENCODE_DTYPE', 'half')
    with pytest.raises(ValueError, match='BN_ENCODE_DTYPE'):
        hip_eval.encode_trial_device(model, torch.zeros(4, 1, 32, 32))


def test_conv_stack_bf16_refuses_gradients():
    plan = _plan([1, 32, 32])
    w = torch.zeros(1, requires_grad=True)
    with pytest.raises(RuntimeError, match='inference only'):
        hf.conv_stack_bf16(plan, torch.zeros(2, 1, 32, 32), [w] * (2 * len(plan)))


# -- the yardstick itself ------------------------------------------------------------------
def test_rne_bf16_by_hand():
    """bf16 keeps 8 significant bits: the spacing in [1, 2) is 2^-7."""
    u = 2.0 ** -7
    vals = [1.0, 1.0 + 0.5 * u, 1.0 + 1.5 * u, 1.0 + 0.5 * u + 2.0 ** -20, 1.0 + 0.49 * u, -3.0 - 2 * u, 0.0, 255.0, 257.0]
    want = [1.0, 1.0, 1.0 + 2 * u, 1.0 + u, 1.0, -3.0 - 2 * u, 0.0, 255.0, 256.0]      # ties go to the even mantissa
    for dt in (torch.float32, torch.float64):
        got = emu.rne_bf16(torch.tensor(vals, dtype=dt))
        assert got.dtype == dt
        assert got.tolist() == want, dt
    # both routes agree on every fp32 value; float64 is not rounded twice
    x = torch.randn(100000, generator=torch.Generator().manual_seed(0)) * 37.0
    assert torch.equal(emu.rne_bf16(x).double(), emu.rne_bf16(x.double()))
    tie_plus = torch.tensor([1.0 + 0.5 * u + 2.0 ** -40], dtype=torch.float64)    # fp32 would round it to the tie
    assert emu.rne_bf16(tie_plus).item() == 1.0 + u


def test_emulated_layer_by_hand():
    """A 1x1 convolution of two pixels and two input channels, worked out by hand:
    x = [[1, 2], [3, -4]] (channel, pixel), w = [[0.5, 0.25], [-1, 1]], b = [0.125, -2], no padding.
      k0: p0 = 0.5 + 0.75 + 0.125 = 1.375;   p1 = 1 - 1 + 0.125 = 0.125
      k1: p0 = -1 + 3 - 2 = 0;               p1 = -2 - 4 - 2 = -8 -> LeakyReLU: -0.4"""
    x = torch.tensor([[[[1.0, 2.0]], [[3.0, -4.0]]]])
    w = torch.tensor([[0.5, 0.25], [-1.0, 1.0]]).view(2, 2, 1, 1)
    b = torch.tensor([0.125, -2.0])
    y = emu.conv_layer(x, w, b, 1, (0, 0, 0, 0), True, torch.float64)
    assert y.dtype == torch.float64
    assert y.view(2, 2).tolist() == [[1.375, 0.125], [0.0, -8.0 * 0.05]]
    # rounded where the device rounds: -0.4 is not a bf16 value, its neighbours are 2^-9 apart
    r = emu.rne_bf16(y).view(2, 2)
    assert r[0].tolist() == [1.375, 0.125]
    assert abs(r[1, 1].item() + 0.4) <= 2.0 ** -10 and r[1, 1].item() != -0.4
    assert r[1, 1].item() == float(torch.tensor(-0.4).to(torch.bfloat16))


def test_emulated_stack_rounds_where_the_device_rounds():
    """Two 1x1 layers: layer 1 multiplies UNROUNDED fp32 operands and rounds its output, layer 2 multiplies the
    rounded weight and keeps its output.  1.0078125 = 1 + 2^-7 is a bf16 value, 1.00390625 = 1 + 2^-8 is a tie
    that goes to 1."""
    x = torch.tensor([[[[1.0]]]])
    l1 = (torch.tensor([[[[1.00390625]]]]), torch.tensor([0.0]), 1, (0, 0, 0, 0))
    l2 = (torch.tensor([[[[1.00390625]]]]), torch.tensor([0.0]), 1, (0, 0, 0, 0))
    # layer 1: 1 * 1.00390625 -> rounded to 1.0; layer 2: weight rounded to 1.0 -> 1.0 exactly
    assert emu.stack_features([l1, l2], x).item() == 1.0
    # a single layer is the last one: fp32 operands, no rounding at all
    assert emu.stack_features([l1], x).item() == 1.00390625
    l1b = (torch.tensor([[[[1.0078125]]]]), torch.tensor([0.0]), 1, (0, 0, 0, 0))
    l2b = (torch.tensor([[[[3.0]]]]), torch.tensor([0.5]), 1, (0, 0, 0, 0))
    assert emu.stack_features([l1b, l2b], x).item() == 3.0 * 1.0078125 + 0.5


def test_pads_of_matches_the_plans():
    plan = _plan([1, 128, 128])
    assert emu.pads_of(plan[1].geom(3)) == (1, 2, 1, 2)         # the asymmetric 5x5 / stride 2 layers
    assert emu.pads_of(plan[4].geom(3)) == (1, 1, 1, 1)         # 5x5 / stride 5
