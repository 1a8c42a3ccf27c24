"""Cases and constants that tests/test_decode_bf16_cpu.py and tests/test_gpu_decode_bf16.py share (no tests here):
the single-layer geometries of the bf16 decoder, their bf16-exact operands, and the gain that gives a freshly
initialised decoder a usable output range."""

import functools

import torch

from behavenet_amd.models import AE
from behavenet_amd.models.ae_model_architecture_generator import load_handcrafted_arch
from tests.bf16_emulation import SLOPE, rne_bf16
from tests.cases import seeded_build
from tests.golden_utils import base_hparams

CPU_FLIP_CAP = 1e-3     # tests/test_gpu_encode_bf16.py: the CPU fp32 reference's own share of FLIP_CAP = 2e-3
# A freshly initialised decoder's x_hat stays within a few hundredths of 0.46: bf16 error would be measured against
# an almost constant image.  Every transposed-conv weight times GAIN spreads the float64 oracle's x_hat over at
# least MIN_SPAN between its 1st and 99th percentile.
GAIN, MIN_SPAN = 3.0, 0.5

# name, seed, N, Cin, Hin, Win, Cout, k, stride, (crop_t, crop_l), (Hout, Wout)
_SWEEP = [
    ('four phases 3x3/3x2/2x3/2x2 taps, M and Cout tails', 1, 7, 32, 5, 7, 24, 5, 2, (1, 1), (10, 14)),
    ('odd output, Cin 80: a 64-deep step straddles taps', 2, 7, 80, 4, 3, 40, 5, 2, (2, 2), (7, 5)),
    ('default convT0: 25 one-tap phases', 3, 64, 512, 2, 2, 256, 5, 5, (1, 1), (8, 8)),
    ('arch2 kernel 4', 4, 7, 16, 6, 6, 64, 4, 2, (1, 1), (12, 12)),
    ('one phase', 5, 7, 48, 9, 5, 16, 3, 1, (1, 1), (9, 5)),
    ('valid with output_padding, N=1', 6, 1, 16, 3, 3, 8, 5, 2, (0, 0), (10, 10)),
]
DEFAULT_DIMS = [[1, 128, 128], [1, 64, 48], [2, 192, 160]]
BODY_CASES = list(_SWEEP) + [('default %s convT%d N=7' % (dim, i), 100 * i + dim[1], 'plan', tuple(dim), i)
                             for dim in DEFAULT_DIMS for i in range(4)]


@functools.lru_cache(maxsize=None)
def _decoder_plan(dim, arch_json):
    arch = load_handcrafted_arch(list(dim), 8, arch_json, check_memory=False)
    return seeded_build(AE, base_hparams(arch, 'ae', {})).decoding._plan


def decoder_plan(dim, arch_json=None):
    return list(_decoder_plan(tuple(dim), arch_json))


def body_geom(case):
    """The twelve integers (N, Ci, Hi, Wi, Co, R, S, stride, crop_t, crop_l, Ho, Wo) of a BODY_CASES entry."""
    if case[2] == 'plan':
        return decoder_plan(case[3])[case[4]].geom(7)
    name, seed, N, Ci, Hi, Wi, Co, k, st, (ct, cl), (Ho, Wo) = case
    return (N, Ci, Hi, Wi, Co, k, k, st, ct, cl, Ho, Wo)


def body_operands(geom, seed, exact_weights=True):
    """bf16-exact operands: N(0,1) through LeakyReLU as activations, N(0,1) / sqrt(taps reaching a pixel x Ci)
    weights (Ci, Co, R, S); ``exact_weights=False`` leaves the weights fp32 (the layer onto the frame)."""
    N, Ci, Hi, Wi, Co, R, S, st, ct, cl, Ho, Wo = geom
    g = torch.Generator().manual_seed(seed)
    x = rne_bf16(torch.nn.functional.leaky_relu(torch.randn((N, Ci, Hi, Wi), generator=g), SLOPE))
    fan = Ci * ((R + st - 1) // st) * ((S + st - 1) // st)
    w = torch.randn((Ci, Co, R, S), generator=g) / float(fan) ** 0.5
    if exact_weights:
        w = rne_bf16(w)
    b = torch.randn((Co,), generator=g) * 0.1
    return x, w, b


def span_1_99(x):
    q = torch.quantile(x.double().flatten()[:4000000], torch.tensor([0.01, 0.99], dtype=torch.float64))
    return float(q[1] - q[0])


DEC_CLASSES = ('ae', 'vae', 'ps-vae', 'cond-ae-msp')
DEC_FRAMES = (40, 67)


def dec_dim(model_class):
    return [2, 128, 128] if model_class == 'ps-vae' else [1, 128, 128]


def decoder_latents(n, width):
    """The latents of the whole-decoder cases: N(0, 1), handed to the decoder as they are."""
    return torch.randn((n, width), generator=torch.Generator().manual_seed(17 + n))


def apply_gain(decoder_modules):
    """Every transposed-conv weight of ``decoder_modules`` (a decoder's ``.decoder`` ModuleList) times GAIN."""
    with torch.no_grad():
        for mod in decoder_modules.modules():
            if isinstance(mod, torch.nn.ConvTranspose2d):
                mod.weight.mul_(GAIN)
