"""The opt-in bf16 encoder on the GPU (csrc/conv_bf16.hip, hip_functions.conv_stack_bf16, hparams['hip_encode_dtype']).

The yardstick is tests/bf16_emulation.py: torch CPU ops in float64 on operands rounded to bf16, rounded again
wherever the HIP path rounds (checked by hand in tests/test_encode_bf16_cpu.py).  Bounds:

* fp32 output of one layer on bf16-exact operands: ``tests.test_gpu_kernels.close`` -- products of bf16 values are
  exact in fp32, the kernel owes fp32 accuracy;
* bf16 output: every element within 2^-8 |ref64| plus what ``close`` grants of the maximum, and at most 2e-3 of the
  elements on another bf16 value than RNE(ref64) (CPU fp32 accumulation flips 1.5e-4..3.1e-4 of them and is held
  to 1e-3 first; a dropped tap or channel chunk flips a large share);
* whole encoder against the emulation: 4 x the spread the emulation itself shows between fp32 and float64
  accumulation for the case at hand; against the exact float64 oracle: 2 x the emulation's own error.
"""

import os
import pickle
import warnings

import numpy as np
import pytest
import torch

from behavenet_amd import _hip
from behavenet_amd import hip_functions as hf
from behavenet_amd.fitting.eval import encode_trial_device, export_latents, get_reconstruction, _GraphedTrialEncoder
from behavenet_amd.fitting.optim import FlatAdamAMSGrad
from behavenet_amd.models.ae_model_architecture_generator import load_handcrafted_arch
from oracle import ref_cpu
from tests import bf16_emulation as emu
from tests.cases import case_hparams, load_case, seeded_build
from tests.golden_utils import base_hparams
from tests.test_gpu_guard_bands import guarded, finite, _bands_stay_untouched  # noqa: F401
from tests.test_gpu_kernels import close
from tests.test_gpu_model import BUILDERS, _pair

pytestmark = pytest.mark.gpu
DEV = 'cuda'
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARCH2 = os.path.join(REPO, 'behavenet_amd', 'configs', 'ae_jsons', 'ae_arch_2.json')
LRELU, SLOPE = _hip.ACT_LRELU, 0.05
FLIP_CAP, CPU_FLIP_CAP = 2e-3, 1e-3
REPORT = []     # figures printed at the end of the module (pytest -s) for profiles/encode_bf16.txt


def teardown_module(module):
    for line in REPORT:
        print('BF16-FIGURE ' + line)


# ------------------------------------------------------------------------------------------ helpers
def geom_of(N, C, H, W, K, R, stride, pt, pl, pb, pr):
    P = (H + pt + pb - R) // stride + 1
    Q = (W + pl + pr - R) // stride + 1
    return (N, C, H, W, K, R, R, stride, pt, pl, P, Q)


def guarded_bf16(t):
    """Device bf16 copy of ``t`` (last dimension even) between NaN guard bands."""
    t = t.to(torch.bfloat16)
    g = guarded(torch.zeros(t.shape[:-1] + (t.shape[-1] // 2,)))
    v = g.view(torch.bfloat16)
    v.copy_(t)
    return v


def guarded_u8(t):
    n = t.numel()
    g = guarded(torch.zeros((n + 3) // 4 + 4))
    v = g.view(torch.uint8)[:n].view(t.shape)
    v.copy_(t)
    return v


def operands(geom, seed):
    """bf16-exact operands: N(0,1) through LeakyReLU as activations, N(0,1) / sqrt(fan-in) weights."""
    N, C, H, W, K, R, S, st, pt, pl, P, Q = geom
    g = torch.Generator().manual_seed(seed)
    x = emu.rne_bf16(torch.nn.functional.leaky_relu(torch.randn((N, C, H, W), generator=g), SLOPE))
    w = emu.rne_bf16(torch.randn((K, C, R, S), generator=g) / float(C * R * S) ** 0.5)
    b = torch.randn((K,), generator=g) * 0.1
    return x, w, b


def run_body(geom, x, w, b, out_f32):
    """One body layer between guard bands -> CPU fp32 (N, K, P, Q)."""
    N, C, H, W, K, R, S, st, pt, pl, P, Q = geom
    xd = guarded_bf16(x.permute(0, 2, 3, 1).contiguous())
    nb = _hip.conv_pack_w_bf16_bytes(w.shape)
    wp = guarded(torch.zeros(nb // 4)).view(torch.uint8)
    _hip.conv_pack_w_bf16(guarded(w), wp)
    bd = guarded(b)
    if out_f32:
        y = guarded(torch.zeros(N, K, P, Q))
        _hip.conv2d_fwd_bf16(xd, wp, bd, geom, LRELU, SLOPE, True, out=y)
        finite(y, 'bf16 conv fp32 out')
        return y.cpu()
    # (bf16 guard bands: a NaN-filled fp32 buffer viewed as bf16 is NaN too)
    assert K % 2 == 0
    y = guarded(torch.zeros(N, P, Q, K // 2)).view(torch.bfloat16)
    _hip.conv2d_fwd_bf16(xd, wp, bd, geom, LRELU, SLOPE, False, out=y)
    finite(y.float(), 'bf16 conv bf16 out')
    return y.float().permute(0, 3, 1, 2).contiguous().cpu()


def references(geom, x, w, b):
    pads = emu.pads_of(geom)
    ref64 = emu.crop_to(emu.conv_layer(x, w, b, geom[7], pads, True, torch.float64), geom)
    ref32 = emu.crop_to(emu.conv_layer(x, w, b, geom[7], pads, True, torch.float32), geom)
    return ref32, ref64


def check_bf16_output(got, want32, ref64, name, ref_for_flips=None):
    """Item 2 of the issue's list: ``got`` holds bf16 values (as fp32).  want32: CPU fp32 accumulation."""
    ref64 = ref64.double()
    scale = max(float(ref64.abs().max()), 1e-30)
    e_cpu = float((want32.double() - ref64).abs().max()) / scale
    allowance = min(1e-4, max(8 * e_cpu, 3e-6)) * scale          # what close() grants of the maximum
    r = emu.rne_bf16(ref64 if ref_for_flips is None else ref_for_flips.double())
    cpu_flips = float((emu.rne_bf16(want32.double()) != r).double().mean())
    hip_flips = float((got.double() != r).double().mean())
    worst = float(((got.double() - ref64).abs() - 2.0 ** -8 * ref64.abs()).max())
    REPORT.append('%s: flips hip %.2e cpu-fp32 %.2e, worst excess over 2^-8|ref| %.2e (allowance %.2e)'
                  % (name, hip_flips, cpu_flips, worst, allowance))
    assert cpu_flips <= CPU_FLIP_CAP, '%s: the CPU fp32 result itself flips %.2e of the elements' % (name, cpu_flips)
    assert worst <= allowance, '%s: an element is %.3e beyond 2^-8 |ref| (allowance %.3e)' % (name, worst, allowance)
    assert hip_flips <= FLIP_CAP, '%s: %.2e of the elements differ from RNE(ref64)' % (name, hip_flips)


def check_layer(geom, seed, name):
    assert _hip.conv2d_bf16_ok(geom), (name, geom)
    x, w, b = operands(geom, seed)
    ref32, ref64 = references(geom, x, w, b)
    assert tuple(ref64.shape) == (geom[0], geom[4], geom[10], geom[11]), (name, ref64.shape, geom)
    got = run_body(geom, x, w, b, True)
    close(got, ref32, ref64, name=name + ' fp32 out')
    if geom[4] % 2 == 0:
        got16 = run_body(geom, x, w, b, False)
        check_bf16_output(got16, ref32, ref64, name + ' bf16 out')


def _plan(dim, arch_json=None):
    arch = load_handcrafted_arch(list(dim), 8, arch_json, check_memory=False)
    return seeded_build(BUILDERS['ae'], base_hparams(arch, 'ae', {})).encoding._plan


# ------------------------------------------------------------------------------------------ 1-3: single layers
@pytest.mark.parametrize('dim', [[1, 128, 128], [2, 128, 128], [1, 64, 48], [2, 192, 160]])
def test_default_architecture_body_layers(dim):
    """conv1..conv4 of the default architecture (5x5 stride 2 padded 1,2,1,2; 5x5 stride 5), fp32 and bf16 output."""
    plan = _plan(dim)
    for i, layer in enumerate(plan[1:], 1):
        n = 7 if i < 3 else 64
        check_layer(layer.geom(n), 100 * i + dim[1], 'default %s conv%d N=%d' % (dim, i, n))


def test_arch_2_body_layers():
    plan = _plan([1, 128, 128], ARCH2)
    for i, layer in enumerate(plan[1:], 1):
        check_layer(layer.geom(7), 300 + i, 'arch2 layer %d %r' % (i + 1, layer))


SWEEP = [
    # name, N, C, H, W, K, R, stride, (pt, pl, pb, pr)
    ('k3 s1 same 13x9', 7, 32, 13, 9, 64, 3, 1, (1, 1, 1, 1)),
    ('k3 s2 asym 13x9', 7, 48, 13, 9, 24, 3, 2, (0, 0, 1, 1)),
    ('k4 s1 asym 16x16', 7, 64, 16, 16, 64, 4, 1, (1, 1, 2, 2)),
    ('k4 s2 sym 16x16', 7, 64, 16, 16, 64, 4, 2, (1, 1, 1, 1)),
    ('k5 s1 valid 13x9', 7, 16, 13, 9, 8, 5, 1, (0, 0, 0, 0)),
    ('k5 s2 asym 5x7', 189, 32, 5, 7, 24, 5, 2, (1, 1, 2, 2)),
    ('k5 s5 sym 8x8', 256, 256, 8, 8, 512, 5, 5, (1, 1, 1, 1)),
    ('k5 s5 13x9', 7, 80, 13, 9, 512, 5, 5, (1, 1, 1, 1)),
    ('k5 s2 N=1 64x48', 1, 32, 64, 48, 64, 5, 2, (1, 1, 2, 2)),
    ('k3 s1 N=1 cout 8', 1, 16, 31, 33, 8, 3, 1, (1, 1, 1, 1)),
    ('k5 s2 N=189', 189, 128, 16, 16, 24, 5, 2, (1, 1, 2, 2)),
    ('k5 s2 N=256 cout 8', 256, 64, 8, 6, 8, 5, 2, (2, 2, 1, 1)),
    ('k4 s5 5x7', 7, 16, 5, 7, 64, 4, 5, (0, 0, 0, 0)),
    ('k1 s1', 7, 144, 9, 5, 40, 1, 1, (0, 0, 0, 0)),
]


@pytest.mark.parametrize('case', SWEEP, ids=[c[0] for c in SWEEP])
def test_layer_sweep(case):
    """Kernels 1 / 3 / 4 / 5, strides 1 / 2 / 5, symmetric and asymmetric padding, odd maps, every tile tail; each
    operand between NaN guard bands and (conftest) on poisoned LDS."""
    name, N, C, H, W, K, R, stride, (pt, pl, pb, pr) = case
    check_layer(geom_of(N, C, H, W, K, R, stride, pt, pl, pb, pr), 7 + len(name) + N, name)


def test_unserved_geometry_is_refused_and_writes_nothing():
    lib = _hip.load()
    geom = (4, 8, 16, 16, 32, 5, 5, 2, 1, 1, 8, 8)                  # 8 input channels: not a multiple of 16
    x = torch.zeros((4, 16, 16, 8), dtype=torch.bfloat16, device=DEV)
    wp = torch.zeros(32 * 8 * 25 * 2, dtype=torch.uint8, device=DEV)
    y = torch.full((4, 32, 8, 8), 7.0, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.bn_conv2d_fwd_bf16(x.data_ptr(), wp.data_ptr(), None, y.data_ptr(), 1, *geom, LRELU, SLOPE, st) == -2
    g7 = (4, 32, 16, 16, 32, 7, 7, 2, 1, 1, 6, 6)
    assert lib.bn_conv2d_fwd_bf16(x.data_ptr(), wp.data_ptr(), None, y.data_ptr(), 1, *g7, LRELU, SLOPE, st) == -2
    gf = (4, 5, 16, 16, 32, 5, 5, 2, 1, 1, 8, 8)                    # five frame channels
    assert lib.bn_conv2d_first_bf16(x.data_ptr(), 0, wp.data_ptr(), None, y.data_ptr(), *gf, LRELU, SLOPE, st) == -2
    # an activation the epilogue does not have
    ok = (4, 32, 16, 16, 32, 5, 5, 2, 1, 1, 8, 8)
    assert lib.bn_conv2d_fwd_bf16(x.data_ptr(), wp.data_ptr(), None, y.data_ptr(), 1, *ok, _hip.ACT_SIGMOID, SLOPE,
                                  st) == -2
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())


def test_layer_repeats_bit_for_bit():
    geom = geom_of(64, 64, 32, 32, 128, 5, 2, 1, 1, 2, 2)
    x, w, b = operands(geom, 5)
    a, c = run_body(geom, x, w, b, False), run_body(geom, x, w, b, False)
    assert torch.equal(a, c)
    a, c = run_body(geom, x, w, b, True), run_body(geom, x, w, b, True)
    assert torch.equal(a, c)


# ------------------------------------------------------------------------------------------ 4: first layer
@pytest.mark.parametrize('u8', [False, True], ids=['fp32', 'uint8'])
@pytest.mark.parametrize('dim', [[1, 128, 128], [2, 128, 128], [1, 64, 48]])
def test_first_layer(dim, u8):
    """fp32 arithmetic, one rounding: RNE_bf16 of the existing fp32 first layer's output, under the rule for bf16
    outputs (the two fp32 kernels sum in different orders)."""
    plan = _plan(dim)
    layer = plan[0]
    n = 7
    geom = layer.geom(n)
    assert _hip.conv2d_bf16_ok(geom, first=True)
    g = torch.Generator().manual_seed(dim[0] * 10 + dim[2])
    xu = torch.randint(0, 256, (n,) + tuple(dim), generator=g, dtype=torch.uint8)
    xf = xu.float() / 255
    w = torch.randn((layer.cout, layer.cin, layer.R, layer.S), generator=g) / float(layer.cin * layer.R * layer.S) ** 0.5
    b = torch.randn((layer.cout,), generator=g) * 0.1
    wd, bd = guarded(w), guarded(b)
    xd = guarded_u8(xu) if u8 else guarded(xf)
    y = guarded(torch.zeros(n, layer.hout, layer.wout, layer.cout // 2)).view(torch.bfloat16)
    _hip.conv2d_first_bf16(xd, wd, bd, geom, LRELU, SLOPE, out=y)
    finite(y.float(), 'first layer')
    got = y.float().permute(0, 3, 1, 2).contiguous().cpu()
    existing = hf.first_layer_forward(plan, xu.to(DEV) if u8 else xf.to(DEV), [w.to(DEV), b.to(DEV)]).cpu()
    ref32, ref64 = references(geom, xf, w, b)
    close(existing, ref32, ref64, name='existing first layer')
    check_bf16_output(got, ref32, ref64, 'first layer %s %s' % (dim, 'u8' if u8 else 'fp32'), ref_for_flips=existing)


# ------------------------------------------------------------------------------------------ whole encoder
GOLDEN_OF = {'ae': 'ae_cfg1', 'vae': 'vae_cfg1', 'beta-tcvae': 'betatc_cfg1', 'ps-vae': 'psvae_cfg4',
             'msps-vae': 'mspsvae_cfg1', 'cond-ae-msp': 'aemsp_cfg1'}


def _meta(model_class, dim, n):
    _, meta = load_case(GOLDEN_OF[model_class])
    meta = dict(meta, dim=list(dim), n_frames=n, extra_hp=dict(meta['extra_hp']))
    meta['extra_hp'].pop('device', None)
    meta.pop('arch_json', None)
    return meta


def _frames(n, dim, seed, smooth=False):
    g = torch.Generator().manual_seed(seed)
    if smooth:
        yy, xx = torch.meshgrid(torch.linspace(0, 1, dim[1]), torch.linspace(0, 1, dim[2]), indexing='ij')
        ph = torch.rand((n, dim[0], 1, 1), generator=g) * 6.28
        img = 0.5 + 0.45 * torch.sin(6.0 * yy + ph) * torch.cos(4.0 * xx - ph)
        return (img * 255).round().clamp(0, 255).to(torch.uint8)
    return torch.randint(0, 256, (n,) + tuple(dim), generator=g, dtype=torch.uint8)


def _latents_of(mc, model, out):
    if mc == 'ps-vae':
        cur = torch.cat([out[0], out[1]], dim=1)
    elif mc == 'msps-vae':
        cur = torch.cat([out[0], out[1], out[2]], dim=1)
    else:
        cur = out[0]
    if mc == 'cond-ae-msp':
        cur = model.U(cur)
    return cur


def _oracle_latents(mc, ora64, x, feats=None):
    """Latents of the float64 oracle; with ``feats`` its conv stack is replaced by these features."""
    enc = ora64.encoding
    if feats is not None:
        def fixed(x_, dataset=None, taps=None):
            enc.pool_idx, enc.pool_sizes = [], []
            return feats.double()
        enc.features = fixed
    try:
        with torch.no_grad():
            return _latents_of(mc, ora64, enc(x.double(), dataset=0))
    finally:
        if feats is not None:
            del enc.features


def _rel(a, b):
    return float((a.double() - b.double()).abs().max()) / max(float(b.double().abs().max()), 1e-30)


ENC_CASES = [(mc, n) for mc in ('ae', 'vae', 'beta-tcvae', 'ps-vae', 'msps-vae', 'cond-ae-msp') for n in (189, 256)]


@pytest.mark.parametrize('model_class,n', ENC_CASES)
def test_whole_encoder_against_emulation_and_oracle(model_class, n):
    dim = [2, 128, 128] if model_class in ('ps-vae', 'msps-vae') else [1, 128, 128]
    meta = _meta(model_class, dim, n)
    hip, ora, hp = _pair(meta)
    hip.eval()
    ora64 = seeded_build(ref_cpu.build_model, case_hparams(meta)).double().eval()
    xu = _frames(n, dim, 11 + n, smooth=(n == 256))
    xf = xu.float() / 255
    layers = emu.oracle_layers(ora.encoding)
    with torch.no_grad():
        z_e64 = _oracle_latents(model_class, ora64, xf, emu.stack_features(layers, xf, torch.float64))
        z_e32 = _oracle_latents(model_class, ora64, xf, emu.stack_features(layers, xf, torch.float32))
        z_exact = _oracle_latents(model_class, ora64, xf)
    spread = _rel(z_e32, z_e64)
    e_emul = _rel(z_e64, z_exact)
    hip.hparams['hip_encode_dtype'] = 'bf16'
    with warnings.catch_warnings():
        warnings.simplefilter('error', UserWarning)
        z_u8 = encode_trial_device(hip, xu.to(DEV), 0, None, 1024).cpu()
        z_f = encode_trial_device(hip, xf.to(DEV), 0, None, 1024).cpu()
    assert torch.equal(z_u8, z_f)           # value / 255 is the same division on both routes
    e_hip_emul, e_hip_exact = _rel(z_u8, z_e64), _rel(z_u8, z_exact)
    REPORT.append('%s N=%d: hip vs emulation %.2e (emulation fp32-vs-f64 spread %.2e), hip vs float64 oracle %.2e '
                  '(emulation vs oracle %.2e)' % (model_class, n, e_hip_emul, spread, e_hip_exact, e_emul))
    hip.hparams['hip_encode_dtype'] = 'f32'
    z_32 = encode_trial_device(hip, xu.to(DEV), 0, None, 1024).cpu()
    assert _rel(z_32, z_exact) <= 1e-4
    assert not torch.equal(z_32, z_u8)
    assert e_hip_emul <= 4 * spread, 'hip vs emulation %.3e, allowed 4 x %.3e' % (e_hip_emul, spread)
    assert e_hip_exact <= 2 * e_emul, 'hip vs oracle %.3e, allowed 2 x %.3e' % (e_hip_exact, e_emul)


def _small(model_class='ae', dim=(1, 64, 48), n=40, extra=None, golden=None):
    if golden is not None:
        _, meta = load_case(golden)
        meta = dict(meta, n_frames=n, extra_hp=dict(meta['extra_hp']))
        meta['extra_hp'].pop('device', None)
    else:
        meta = _meta(model_class, dim, n)
    meta['extra_hp'].update(extra or {})
    hp = case_hparams(meta)
    model = seeded_build(BUILDERS[meta['model_class']], hp).to(DEV)
    return model, meta


# ------------------------------------------------------------------------------------------ 6: nothing existing moves
def test_fp32_paths_keep_their_bits():
    model, meta = _small('vae', (1, 64, 48), 40)
    model.eval()
    dim = meta['dim']
    xu = _frames(40, dim, 3).to(DEV)
    xf = (xu.float() / 255).contiguous()

    def direct(x):
        with torch.no_grad():
            return model.encoding(x, dataset=0)[0].clone()
    want_u8, want_f = direct(xu), direct(xf)
    for key in (None, 'f32'):
        model.hparams.pop('hip_encode_dtype', None)
        if key:
            model.hparams['hip_encode_dtype'] = key
        assert torch.equal(encode_trial_device(model, xu, 0, None, 1024), want_u8)
        assert torch.equal(encode_trial_device(model, xf, 0, None, 1024), want_f)
    model.hparams['hip_encode_dtype'] = 'bf16'
    z16 = encode_trial_device(model, xu, 0, None, 1024)
    assert not torch.equal(z16, want_u8)
    model.hparams.pop('hip_encode_dtype')
    assert torch.equal(encode_trial_device(model, xu, 0, None, 1024), want_u8)
    assert torch.equal(direct(xu), want_u8)


@pytest.mark.parametrize('model_class', ['ae', 'vae', 'ps-vae'])
def test_hparam_changes_nothing_but_the_exporters(model_class):
    """loss() in eval and training mode (with gradients), forward(), get_reconstruction and a bare model.encoding
    give the same bits with hparams['hip_encode_dtype'] = 'bf16' as without the key."""
    dim = (2, 64, 48) if model_class == 'ps-vae' else (1, 64, 48)
    n = 24
    xf = (_frames(n, dim, 5).float() / 255).to(DEV)
    res = {}
    for key in (None, 'bf16'):
        model, meta = _small(model_class, dim, n)
        if key:
            model.hparams['hip_encode_dtype'] = key
        data = {'images': xf[None]}
        if meta['n_labels']:
            g = torch.Generator().manual_seed(2)
            data['labels'] = torch.randn((1, n, meta['n_labels']), generator=g).to(DEV)
        out = {}
        model.eval()
        torch.manual_seed(1)
        ev = model.loss(data, dataset=0, accumulate_grad=False)
        out['eval_loss'] = {k: float(v) for k, v in dict(ev).items()}
        torch.manual_seed(1)
        with torch.no_grad():
            fw = model(xf, dataset=0, use_mean=True) if model_class != 'ae' else model(xf, dataset=0)
        out['forward'] = [t.clone() for t in fw if torch.is_tensor(t)]
        out['recon'] = torch.from_numpy(get_reconstruction(model, xf, dataset=0))
        with torch.no_grad():
            out['encoding'] = model.encoding(xf, dataset=0)[0].clone()
        model.train()
        model.zero_grad()
        torch.manual_seed(1)
        tr = model.loss(data, dataset=0, accumulate_grad=True)
        out['train_loss'] = {k: float(v) for k, v in dict(tr).items()}
        out['grads'] = [p.grad.clone() for p in model.parameters() if p.grad is not None]
        res[key] = out
    a, b = res[None], res['bf16']
    assert a['eval_loss'] == b['eval_loss'] and a['train_loss'] == b['train_loss']
    assert torch.equal(a['recon'], b['recon']) and torch.equal(a['encoding'], b['encoding'])
    assert len(a['forward']) == len(b['forward']) and len(a['grads']) == len(b['grads']) > 0
    for s, t in zip(a['forward'] + a['grads'], b['forward'] + b['grads']):
        assert torch.equal(s, t)


def test_context_manager_is_the_way_to_bf16_from_model_encoding():
    model, meta = _small('ae', (1, 64, 48), 16)
    model.eval()
    xu = _frames(16, meta['dim'], 9).to(DEV)
    model.hparams['hip_encode_dtype'] = 'bf16'
    with torch.no_grad():
        bare = model.encoding(xu, dataset=0)[0].clone()
        with hf.encode_precision('bf16'):
            wrapped = model.encoding(xu, dataset=0)[0].clone()
    assert torch.equal(wrapped, encode_trial_device(model, xu, 0, None, 1024))
    assert not torch.equal(bare, wrapped)
    # training mode: fp32 and one warning
    model.train()
    with pytest.warns(UserWarning, match='training mode'):
        z = encode_trial_device(model, xu, 0, None, 1024)
    with warnings.catch_warnings():
        warnings.simplefilter('error', UserWarning)
        z2 = encode_trial_device(model, xu, 0, None, 1024)
    model.eval()
    model.hparams.pop('hip_encode_dtype')
    with torch.no_grad():
        # (train() and eval() run the same kernels for a model without batch norm)
        assert torch.equal(z, model.encoding(xu, dataset=0)[0]) and torch.equal(z, z2)


# ------------------------------------------------------------------------------------------ 7, 8: graph, repeatability
def test_graphed_bf16_encode_replays_the_eager_bits():
    model, meta = _small('ae', (1, 64, 48), 30)
    model.eval()
    model.hparams.update(hip_graph_encode=True, hip_encode_dtype='bf16')
    trials = [_frames(30, meta['dim'], 20 + i).to(DEV) for i in range(4)]
    enc = _GraphedTrialEncoder(model)
    got = [enc(t, 0).clone() for t in trials]
    assert enc.n_replays > 0
    eager = [encode_trial_device(model, t, 0, None, 1024) for t in trials]
    for a, b in zip(got, eager):
        assert torch.equal(a, b)
    n16 = len(enc._graphs)
    model.hparams['hip_encode_dtype'] = 'f32'
    got32 = [enc(t, 0).clone() for t in trials]
    assert len(enc._graphs) == n16 + 1                    # the same shape in fp32 is another graph
    for a, t in zip(got32, trials):
        with torch.no_grad():
            assert torch.equal(a, model.encoding(t, dataset=0)[0])
    model.hparams['hip_encode_dtype'] = 'bf16'
    assert torch.equal(enc(trials[0], 0), eager[0])


def test_two_bf16_encodes_identical_bits():
    model, meta = _small('vae', (1, 128, 128), 64)
    model.eval()
    model.hparams['hip_encode_dtype'] = 'bf16'
    xu = _frames(64, meta['dim'], 31).to(DEV)
    a = encode_trial_device(model, xu, 0, None, 1024).clone()
    b = encode_trial_device(model, xu, 0, None, 1024).clone()
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------ 9: no stale weights
def test_in_place_adam_steps_reach_the_next_encode():
    model, meta = _small('ae', (1, 64, 48), 24)
    model.hparams['hip_encode_dtype'] = 'bf16'
    xu = _frames(24, meta['dim'], 41).to(DEV)
    xf = (xu.float() / 255).contiguous()
    model.eval()
    first = encode_trial_device(model, xu, 0, None, 1024).clone()
    model.train()
    opt = FlatAdamAMSGrad(model.get_parameters(), lr=1e-2, weight_decay=0)
    for _ in range(2):
        opt.zero_grad()
        model.loss({'images': xf[None]}, dataset=0, accumulate_grad=True)
        opt.step()
    model.eval()
    second = encode_trial_device(model, xu, 0, None, 1024).clone()
    fresh, _ = _small('ae', (1, 64, 48), 24)
    fresh.load_state_dict({k: v.clone() for k, v in model.state_dict().items()})
    fresh.hparams['hip_encode_dtype'] = 'bf16'
    fresh.eval()
    assert torch.equal(second, encode_trial_device(fresh, xu, 0, None, 1024))
    assert not torch.equal(first, second)


# ------------------------------------------------------------------------------------------ 10: fallbacks
@pytest.mark.parametrize('golden,why', [('ae_maxpool', 'max-pooling'), ('ae_cfg1_bn', 'batch-norm'),
                                        ('condae_enc_cfg1', 'conditional_encoder'), ('ae_linear', 'linear')])
def test_unserved_models_fall_back_to_fp32_with_one_warning(golden, why):
    from tests.cases import case_data
    n = 12
    model, meta = _small(golden=golden, n=n)
    model.eval()
    data = case_data(meta, device=DEV)
    x = data['images'][0].contiguous()
    labels_2d = data['labels_sc'][0] if 'labels_sc' in data else None
    want = encode_trial_device(model, x, 0, labels_2d, 200).clone()
    model.hparams['hip_encode_dtype'] = 'bf16'
    with pytest.warns(UserWarning, match=why) as rec:
        got = encode_trial_device(model, x, 0, labels_2d, 200)
        again = encode_trial_device(model, x[:5], 0, None if labels_2d is None else labels_2d[:5], 200)
    assert len([w for w in rec if 'bf16' in str(w.message)]) == 1
    assert torch.equal(got, want) and torch.equal(again, want[:5])


# ------------------------------------------------------------------------------------------ 11: export_latents
def test_export_latents_with_the_key(tmp_path):
    from behavenet_amd.data.data_generator import ConcatSessionsGenerator
    from behavenet_amd.data.trial_store import write_npz_session
    dim = [1, 64, 48]
    arch = load_handcrafted_arch(list(dim), 6, None, check_memory=False)
    hp = base_hparams(arch, 'ae', {'expt_dir': str(tmp_path), 'device': 'cuda'})
    torch.manual_seed(0)
    hip = BUILDERS['ae'](hp).to(DEV)
    hip.version = 0
    rng = np.random.default_rng(3)
    lens = [30, 30, 17, 30, 17, 30, 30, 17, 30, 30, 30, 17]
    trials = [rng.integers(0, 255, size=(t,) + tuple(dim), dtype=np.uint8) for t in lens]
    sess_dir = os.path.join(str(tmp_path), 'lab', 'expt', 'animal', 'sess')
    write_npz_session(os.path.join(sess_dir, 'data.npz'), {'images': trials})
    ids = {'lab': 'lab', 'expt': 'expt', 'animal': 'animal', 'session': 'sess'}

    def run(dtype, name):
        gen = ConcatSessionsGenerator(str(tmp_path), [ids], signals_list=[['images']], transforms_list=[[None]],
                                      paths_list=[[os.path.join(sess_dir, 'data.npz')]], device='cuda',
                                      placement='host_u8', keep_in_memory=False)
        hip.hparams.pop('hip_encode_dtype', None)
        if dtype:
            hip.hparams['hip_encode_dtype'] = dtype
        out = os.path.join(str(tmp_path), name)
        with warnings.catch_warnings():
            warnings.simplefilter('error', UserWarning)
            export_latents(gen, hip, filename=out)
        with open(out, 'rb') as f:
            return pickle.load(f)
    a, b = run(None, 'f32.pkl'), run('bf16', 'bf16.pkl')
    assert sorted(a) == sorted(b) == ['latents', 'trials']
    assert sorted(a['trials']) == sorted(b['trials'])
    for k in a['trials']:
        assert np.array_equal(np.asarray(a['trials'][k]), np.asarray(b['trials'][k]))
    assert len(a['latents']) == len(b['latents']) == len(lens)
    # the bound of the whole-encoder test for this model: the emulation's own error against exact arithmetic
    torch.manual_seed(0)
    ora = ref_cpu.AE(base_hparams(dict(arch), 'ae')).eval()
    ora64 = ref_cpu.AE(base_hparams(dict(arch), 'ae')).double().eval()
    ora64.load_state_dict({k: v.double() for k, v in ora.state_dict().items()})
    differ = 0
    for i, t in enumerate(lens):
        assert a['latents'][i].shape == b['latents'][i].shape and a['latents'][i].dtype == b['latents'][i].dtype
        if a['latents'][i].size == 0:
            continue
        xf = torch.from_numpy(trials[i].astype(np.float32) / 255)
        with torch.no_grad():
            z_exact = _oracle_latents('ae', ora64, xf)
            z_e64 = _oracle_latents('ae', ora64, xf, emu.stack_features(emu.oracle_layers(ora.encoding), xf))
        e_emul = _rel(z_e64, z_exact)
        za, zb = torch.from_numpy(a['latents'][i]), torch.from_numpy(b['latents'][i])
        assert _rel(za, z_exact) <= 1e-4
        assert _rel(zb, z_exact) <= 2 * e_emul, (i, _rel(zb, z_exact), e_emul)
        differ += int(not torch.equal(za, zb))
    assert differ > 0
