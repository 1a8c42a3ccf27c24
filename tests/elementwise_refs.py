"""References and inputs for the kernels of csrc/elementwise.hip and csrc/decomposed_kl.hip (CPU only).

Every reference evaluates the operation of one entry point of behavenet_amd/_hip.py with plain torch operators in
``dtype``: float64 (the default) on float64 copies of the fp32 inputs is the yardstick, float32 is the "fp32 CPU
result" that ``tests.test_gpu_kernels.close`` weighs the device's error against.  tests/test_elementwise_refs_cpu.py
checks the references against torch autograd of the defining formulas; tests/test_gpu_elementwise.py compares the
kernels with them.  The input generators at the end are shared by both files, so both draw the same tensors.

The decomposed KL has one reference, ``oracle.ref_cpu.decomposed_kl``; ``dkl_reference`` only runs it (and the
logsumexps of the same ``_log_q_pairs``) in both precisions.
"""
import functools

import numpy as np
import torch

from oracle import ref_cpu

ACT_NONE, ACT_LRELU, ACT_SIGMOID = 0, 1, 2          # behavenet_amd._hip.ACT_*
ACTS = (ACT_LRELU, ACT_SIGMOID, ACT_NONE)
ACT_IDS = {ACT_LRELU: 'lrelu', ACT_SIGMOID: 'sigmoid', ACT_NONE: 'none'}
SLOPE = 0.05
F32, F64 = torch.float32, torch.float64

# The streaming kernels run EW_THREADS = 256 threads per block on at most EW_MAX_BLOCKS = 2048 blocks, 524288
# threads, and stride by that.  The float4 path gives thread t the vectors t, t + 524288, ... of n >> 2 and then
# the n & 3 scalars after them; the scalar path gives it the floats t, t + 524288, ...
EW_THREADS, EW_MAX_BLOCKS = 256, 2048
EW_GRID_THREADS = EW_THREADS * EW_MAX_BLOCKS                       # 524288
# 524288 + 256 vectors and 3 scalars: the threads of block 0 run the float4 loop a second time, n % 4 == 3
N_VEC_STRIDE = 4 * EW_GRID_THREADS + 4 * EW_THREADS + 3            # 2 098 179
# 524288 + 259 floats: 259 threads (block 0 and three of block 1) run the scalar loop a second time
N_SCALAR_STRIDE = EW_GRID_THREADS + EW_THREADS + 3                 # 524 547
# one thread; a tail alone; one vector; one vector and a tail; more than one block, with 3 tail floats each way
TAIL_SIZES = (1, 3, 4, 5, 1023, 1027)
assert N_VEC_STRIDE == 2098179 and N_SCALAR_STRIDE == 524547


def _c(t, dtype):
    return None if t is None else t.detach().to('cpu', dtype)


# ---------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------
def act_fwd(x, act, slope=SLOPE, dtype=F64):
    x = _c(x, dtype)
    if act == ACT_LRELU:
        return torch.where(x > 0, x, x * slope)
    if act == ACT_SIGMOID:
        return 1.0 / (1.0 + torch.exp(-x))
    return x.clone()


def act_bwd(dy, y, act, slope=SLOPE, dtype=F64):
    """dL/dpre from dL/dy and the OUTPUT y of the activation."""
    dy, y = _c(dy, dtype), _c(y, dtype)
    if act == ACT_LRELU:
        return dy * torch.where(y > 0, torch.ones_like(y), torch.full_like(y, slope))
    if act == ACT_SIGMOID:
        return dy * (y * (1.0 - y))
    return dy.clone()


def sqerr_frame_sums(pred, target, mask=None, dtype=F64):
    d = (_c(pred, dtype) - _c(target, dtype)) ** 2
    if mask is not None:
        d = d * _c(mask, dtype)
    return d.reshape(d.shape[0], -1).sum(dim=1)


def sqerr_bwd(pred, target, mask, scale, gscale=None, dtype=F64):
    s = 2.0 * scale
    if gscale is not None:
        s = s * _c(gscale, dtype)
    out = s * (_c(pred, dtype) - _c(target, dtype))
    if mask is not None:
        out = out * _c(mask, dtype)
    return out


def scale_frames(t, frame_scale, group_scale=None, group_of_frame=None, dtype=F64):
    sc = _c(frame_scale, dtype)
    if group_scale is not None:
        sc = sc * _c(group_scale, dtype)[group_of_frame.detach().cpu().long()]
    t = _c(t, dtype)
    return t * sc.reshape((-1,) + (1,) * (t.dim() - 1))


def reduce_sum(t, scale=1.0, dtype=F64):
    return _c(t, dtype).sum() * scale


def reparam_fwd(mu, logvar, eps, dtype=F64):
    """std = exp(logvar), the project's convention (k_reparam_fwd)."""
    return _c(eps, dtype) * torch.exp(_c(logvar, dtype)) + _c(mu, dtype)


def reparam_bwd(dz, z, mu, dtype=F64):
    """dL/dlogvar = dz * eps * exp(logvar) = dz * (z - mu)."""
    return _c(dz, dtype) * (_c(z, dtype) - _c(mu, dtype))


def kl_rows(mu, logvar, dtype=F64):
    mu, lv = _c(mu, dtype), _c(logvar, dtype)
    return 0.5 * torch.sum(torch.exp(lv) - lv + mu * mu - 1.0, dim=1)


def kl_bwd(mu, logvar, scale, gscale=None, dtype=F64):
    """Gradient of scale * gscale * sum(kl_rows) -> (dmu, dlogvar)."""
    mu, lv = _c(mu, dtype), _c(logvar, dtype)
    s = scale if gscale is None else scale * _c(gscale, dtype)
    return s * mu, s * 0.5 * (torch.exp(lv) - 1.0)


def adam_amsgrad(p, g, m, v, vmax, lr, b1, b2, eps, wd, step, dtype=F64):
    """One step of torch.optim.Adam(amsgrad=True) in its single-tensor order -> new (p, m, v, vmax)."""
    p, g, m, v, vmax = (_c(t, dtype) for t in (p, g, m, v, vmax))
    if wd != 0:
        g = g + wd * p
    m = m + (g - m) * (1 - b1)
    v = v * b2 + (1 - b2) * g * g
    vmax = torch.maximum(vmax, v)
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step           # Python floats
    denom = torch.sqrt(vmax) / (bc2 ** 0.5) + eps
    p = p - (lr / bc1) * (m / denom)
    return p, m, v, vmax


def adam_amsgrad_emulated(p, g, m, v, vmax, lr, b1, b2, eps, wd, step):
    """k_adam_amsgrad term by term in fp32 numpy, with the host's part of bn_launch_adam: step_size and sqrt(bc2)
    rounded from double, 1 - b1 and 1 - b2 subtracted IN fp32 from the fp32 betas the entry point receives.
    (fmaf as the double product and sum rounded once more: the product of two floats is exact in double.)"""
    f = np.float32
    p, g, m, v, vmax = (np.asarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t, dtype=f)
                        for t in (p, g, m, v, vmax))
    b1, b2, eps, wd = f(b1), f(b2), f(eps), f(wd)
    step_size = f(float(f(lr)) / (1.0 - float(b1) ** step))
    bc2_sqrt = f(np.sqrt(1.0 - float(b2) ** step))
    omb1, omb2 = f(1) - b1, f(1) - b2

    def fmaf(a, b, c):
        return (a.astype(np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f)

    gg = fmaf(p, wd, g) if wd != 0 else g
    m = m + omb1 * (gg - m)
    v = fmaf(omb2 * gg, gg, v * b2)
    vmax = np.maximum(vmax, v)
    denom = np.sqrt(vmax) / bc2_sqrt + eps
    p = p - step_size * (m / denom)
    return tuple(torch.from_numpy(np.ascontiguousarray(t, dtype=f)) for t in (p, m, v, vmax))


def u8_to_unit_float(u8):
    return np.asarray(u8, dtype=np.uint8).astype(np.float32) / np.float32(255)


decomposed_kl = ref_cpu.decomposed_kl


def dkl_logsumexps(z, mu, logvar, dtype=F64):
    """(log_qz (N,), lse (N, D)) of the oracle's pair table: what bn_decomposed_kl_fwd saves for the backward."""
    lq = ref_cpu._log_q_pairs(_c(z, dtype), _c(mu, dtype), _c(logvar, dtype))
    return torch.logsumexp(lq.sum(dim=2), dim=1), torch.logsumexp(lq, dim=1)


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def act_inputs(n, act, seed=0):
    """(pre, y, dy): pre-activations with exact zeros among them, the fp32 output, an upstream gradient."""
    g = _gen(seed * 7919 + n)
    pre = torch.randn((n,), generator=g) * 2.0
    pre[3::17] = 0.0
    y = act_fwd(pre, act, dtype=F32)
    dy = torch.rand((n,), generator=g) - 0.5
    return pre, y, dy


def sqerr_inputs(shape, masked, seed=3):
    g = _gen(seed * 7919 + int(np.prod(shape)))
    pred = torch.rand(shape, generator=g)
    target = torch.rand(shape, generator=g)
    mask = (torch.rand(shape, generator=g) > 0.3).float() if masked else None     # about 30 % zeros
    return pred, target, mask


def positive_inputs(n, seed=5):
    return torch.rand((n,), generator=_gen(seed * 7919 + n)) + 0.1


def scale_frames_inputs(N, D, grouped, seed=9):
    """(t, frame_scale, group_scale | None, group_of_frame | None): three groups, each used, not sorted."""
    g = _gen(seed * 7919 + N * D)
    t = torch.rand((N, D), generator=g) - 0.5
    fs = torch.rand((N,), generator=g) + 0.5
    if not grouped:
        return t, fs, None, None
    gs = torch.tensor([0.7, 1.9, -1.2])
    gof = torch.tensor([(2, 0, 1, 0, 2)[n % 5] for n in range(N)], dtype=torch.int32)
    assert N < 3 or set(gof.tolist()) == {0, 1, 2}
    return t, fs, gs, gof


def latent_inputs(shape, seed=11):
    """(mu, logvar, eps, dz): logvar uniform in [-8, 3], mu normal x 2."""
    g = _gen(seed * 7919 + int(np.prod(shape)))
    mu = torch.randn(shape, generator=g) * 2.0
    lv = torch.rand(shape, generator=g) * 11.0 - 8.0
    eps = torch.randn(shape, generator=g)
    dz = torch.rand(shape, generator=g) - 0.5
    return mu, lv, eps, dz


ADAM_HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)


def adam_start(n, seed=6):
    return torch.rand((n,), generator=_gen(seed * 7919 + n)) - 0.5


def adam_grad(n, step, seed=6):
    """Uniform in [-0.5, 0.5]; x 0.01 at steps 3 and 4 (vmax holds its value); every 7th exactly 0 at step 5."""
    g = torch.rand((n,), generator=_gen((seed * 7919 + n) * 64 + step)) - 0.5
    if step in (3, 4):
        g = g * 0.01
    if step == 5:
        g[::7] = 0.0
    return g


def grey_levels(n):
    """n bytes in which every grey level occurs (n >= 256), in no regular order of period 4 or 256."""
    i = np.arange(n, dtype=np.int64)
    u8 = ((i * 37 + (i // 256) * 101 + 11) % 256).astype(np.uint8)
    assert n < 256 or len(np.unique(u8)) == 256
    return u8


DKL_WEIGHTS = (1.3, -0.4, 2.1)
DKL_REGIMES = ('prior', 'posterior', 'separated')
# both generations at N just below, at and just above their row-loop strides: 256 threads over i (D <= 32), two
# halves of 128 rows (32 < D <= 64), and the wide loop on its third trip; D at 1, below, at the generation's width
DKL_SHAPES = [(N, D) for N in (255, 256, 257) for D in (1, 31, 32)] + \
             [(N, D) for N in (127, 128, 129, 257) for D in (33, 63, 64)]
DKL_CASES = [(N, D, r) for (N, D) in DKL_SHAPES for r in DKL_REGIMES]
DKL_IDS = ['%dx%d-%s' % c for c in DKL_CASES]


def dkl_inputs(N, D, regime):
    """(z, mu, logvar) with seed N * 100 + D.  'prior': z drawn independently of mu, as the older tests do;
    'posterior': z on its own posterior, joint[j, i] dominated by i == j; 'separated': posteriors so narrow and
    far apart that every off-diagonal exp() underflows."""
    g = _gen(N * 100 + D)
    if regime == 'prior':
        z = torch.randn((N, D), generator=g)
        mu = torch.randn((N, D), generator=g) * 0.7
        lv = torch.randn((N, D), generator=g) * 0.5 - 0.3
        return z, mu, lv
    spread, lo, hi = {'posterior': (1.5, -4.0, -1.0), 'separated': (3.0, -8.0, -4.0)}[regime]
    mu = spread * torch.randn((N, D), generator=g)
    lv = torch.rand((N, D), generator=g) * (hi - lo) + lo
    z = mu + torch.randn((N, D), generator=g) * torch.exp(0.5 * lv)
    return z, mu, lv


@functools.lru_cache(maxsize=None)
def dkl_reference(N, D, regime):
    """{'f32' | 'f64': (terms (3,), dz, dmu, dlogvar, log_qz, lse)} of the oracle under DKL_WEIGHTS; computed once
    per case and shared (treat as read-only)."""
    z, mu, lv = dkl_inputs(N, D, regime)
    res = {}
    for key, dt in (('f32', F32), ('f64', F64)):
        zi, mi, li = (t.detach().clone().to(dt).requires_grad_(True) for t in (z, mu, lv))
        terms = torch.stack(decomposed_kl(zi, mi, li))
        (terms * torch.tensor(DKL_WEIGHTS, dtype=dt)).sum().backward()
        res[key] = (terms.detach(), zi.grad, mi.grad, li.grad) + dkl_logsumexps(z, mu, lv, dtype=dt)
    return res


def rel_err(got, want64):
    """max |got - f64| / max |f64|, the figure ``close`` bounds."""
    w = want64.detach().cpu().double().numpy()
    g = got.detach().cpu().double().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    return float(np.abs(g - w).max() / max(np.abs(w).max(), 1e-30))
