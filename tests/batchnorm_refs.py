"""Batch norm outside the chunked training step, restated in plain Python: the routing of csrc/batchnorm.hip (which
kernel a call runs and how it cuts the frames into slices), the case lists of tests/test_gpu_batchnorm_split.py, the
inputs of a case, the CPU reference of the rank-split forms and the harness that replays the ranks of a
frame-sharded step one after another.

Nothing here calls the library: tests/test_batchnorm_routes_host.py holds ``bn_splits`` against
``bn_batchnorm_ws_bytes``, asserts that the case lists reach every fact of ``route`` in both values, checks
``split_reference`` against the batch-norm formulas written out in float64 and runs ``replay`` over a numpy
stand-in for the device calls; tests/test_gpu_batchnorm_split.py runs the same lists on the device.
"""
import collections

import torch
import torch.nn.functional as F

# The library's activation codes (behavenet_amd._hip.ACT_*), the slope of tests.test_gpu_kernels.SLOPE and, below,
# ``activation`` (tests.test_gpu_kernels.act_ref with an optional mask) are RESTATED, not imported: this module must
# not load the library, which importing tests/test_gpu_kernels.py does.  test_constants_are_the_librarys
# (tests/test_batchnorm_routes_host.py) holds every one of them equal to the original, so a copy cannot drift.
ACT_NONE, ACT_LRELU, ACT_SIGMOID = 0, 1, 2
SLOPE = 0.05
EPS = 1e-5

BNK_THREADS = 256
BNK_MAX_CHUNKS = 4
BNO_THREADS = 1024
BNO_NV = 8


# ---------------------------------------------------------------------------------------------------------------
# routing
# ---------------------------------------------------------------------------------------------------------------
def bn_splits(N, C):
    """Frame slices per channel of the (channel, slice) grids."""
    s = min(1024 // C, 64, N)
    return max(s, 1)


def ws_bytes(N, C):
    """bn_batchnorm_ws_bytes: per chunk two partial arrays [C][S] and two combined vectors [C]."""
    if N <= 0 or C <= 0:
        return 0
    return BNK_MAX_CHUNKS * (2 * C * bn_splits(N, C) + 2 * C) * 4


def set_slices(N, S):
    """bnk_set_slices for ONE chunk of N frames asked to take S slices -> the slices it gets."""
    S = max(S, 1)
    k = (S * N + N // 2) // N if N > 0 else 1
    k = max(k, 1)
    if k > N and N > 0:
        k = N
    used = k
    if used > S and k - (used - S) >= 1:
        k -= used - S
        used = S
    if used < S:
        add = min(S - used, max(N - k, 0))
        k += add
    return k


def moment_slices(N, S, end=None):
    """Frames [beg, end) of every slice of k_bn_moment_part: contiguous.  ``end(sp, N, S)``: another upper bound
    (the host test shows that a wrong one is caught)."""
    end = end or (lambda sp, N, S: (sp + 1) * N // S)
    return [(sp * N // S, end(sp, N, S)) for sp in range(S)]


def interleaved_slices(N, S):
    """Frames of every slice of k_bn_bwd_part / k_bn_bwd_apply_fin (bnk_slice): slice sp takes sp, sp + S, ..."""
    return [[sp + k * S for k in range((N - sp + S - 1) // S)] for sp in range(S)]


def bno_fits(N, C, HW, aligned):
    """One workgroup owns a channel and holds it in registers."""
    if HW % 4 != 0 or N * C * HW >= 0xffffffff or not aligned:
        return False
    if N * (HW // 4) > BNO_THREADS * BNO_NV:
        return False
    return C >= 64 or N * C * HW * 4 <= (2 << 20)


def bno_threads(N, HW):
    return 256 if N * (HW // 4) <= 256 * BNO_NV else BNO_THREADS


def moment_loop(frames, HW, vec):
    """(fill, trips) of one slice of k_bn_moment_part: does a live thread of the two-groups-per-trip loop meet
    ``e2 >= cnt``, and how many trips does thread 0 make.  The scalar loop has no second group."""
    if not vec:
        return False, -(-frames * HW // BNK_THREADS)
    cnt = frames * (HW // 4)
    trips = -(-cnt // (2 * BNK_THREADS))
    # thread t is live in trip k if e = t + 512 k < cnt; its second group is past the end if e + 256 >= cnt
    fill = any(e + BNK_THREADS >= cnt
               for k in range(trips) for e in range(2 * BNK_THREADS * k, min(cnt, 2 * BNK_THREADS * k + BNK_THREADS)))
    return fill, trips


Route = collections.namedtuple('Route', [
    'N', 'S',               # frames of this call, slices per channel
    'owned',                # k_bn_bwd_owned takes the backward pass of batchnorm_bwd (never the rank-split forms)
    'threads', 'lin',       # of the owned kernel (None where it does not run)
    'moment_vec',           # k_bn_moment_part reads 16-byte groups
    'apply_vec',            # k_bn_act_fwd / k_bn_bwd_part / k_bn_bwd_apply(_fin) read 16-byte groups
    'even',                 # S divides N
    'fill', 'multi_trip',   # of the moment loop, over all slices
    'combine_blocks',       # workgroups of k_bn_combine
])


def route_call(N, C, H, W, aligned=True):
    """The facts of one call on N frames (one rank of a split case, or a whole eval / two-pass case)."""
    HW = H * W
    S = bn_splits(N, C)
    vec = HW % 4 == 0 and aligned
    owned = N > 0 and bno_fits(N, C, HW, aligned)
    threads = bno_threads(N, HW) if owned else None
    lin = threads % (HW // 4) == 0 if owned else None
    loops = [moment_loop(e - b, HW, vec) for b, e in moment_slices(N, S)] if N else []
    return Route(N, S, owned, threads, lin, vec, vec, N % S == 0, any(f for f, _ in loops),
                 any(t > 1 for _, t in loops), (C + 63) // 64)


def route(case, aligned=True):
    """``case``: an EVAL_CASES row (N, C, H, W) -> its Route; a SYNC_CASES row (C, H, W, parts) -> one per rank."""
    if isinstance(case[3], tuple):
        C, H, W, parts = case
        return [route_call(n, C, H, W, aligned) for n in parts]
    return route_call(*case, aligned=aligned)


# ---------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------
# (C, H, W, frames per rank)
SYNC_CASES = [
    (32, 8, 8, (5, 3)),             # vector paths, one frame per slice, cnt = 16: the fill branch on every thread
    (3, 7, 3, (70, 9)),             # HW = 21: scalar paths; S = 64 over 70 frames: uneven slices
    (1200, 1, 4, (3, 1, 2)),        # C > 1024: S = 1; hw4 = 1; three ranks; k_bn_combine in 19 workgroups
    (33, 2, 2, (130, 0, 7)),        # a rank without frames; odd channel count; S = 31
    (16, 16, 16, (33, 32)),         # S = 33 and 32, 64 groups per slice
    (600, 1, 4, (590, 10)),         # S = 1, 590 groups: two trips of the moment loop
    (512, 4, 4, (40,)),             # one rank: also equals the two-pass public API
    (4, 2, 2, (1,)),                # one frame, 4 values per channel: unbiased factor 4 / 3
]

# one run of a split case: LeakyReLU, momentum 0.1 and affine parameters unless said otherwise; ``tracked``: the
# batch counter before the step when momentum is None (the cumulative factor is 1 / (tracked + 1)); ``shifted``:
# rank r's frames moved by +3, -3, ... after drawing, so that the global mean is foreign to every rank's data
SyncRun = collections.namedtuple('SyncRun', ['case', 'act', 'momentum', 'affine', 'shifted', 'tracked'])
SyncRun.__new__.__defaults__ = (ACT_LRELU, 0.1, True, False, 0)

SYNC_RUNS = [SyncRun(c) for c in SYNC_CASES] + [
    SyncRun(SYNC_CASES[0], act=ACT_NONE),
    SyncRun(SYNC_CASES[0], act=ACT_SIGMOID),
    SyncRun(SYNC_CASES[3], momentum=None, tracked=2),
    SyncRun(SYNC_CASES[3], affine=False),
    SyncRun(SYNC_CASES[0], shifted=True),
]
SINGLE_RANK_CASE = (512, 4, 4, (40,))

# (N, C, H, W)
EVAL_CASES = [
    (5, 16, 8, 8),                  # owned, 256 threads
    (200, 64, 8, 8),                # owned, 1024 threads
    (210, 96, 2, 2),                # owned, hw4 = 1
    (23, 70, 6, 4),                 # owned, lin == false
    (3, 1200, 1, 4),                # owned, C > 1024
    (40, 8, 32, 32),                # sliced, vector: 10240 groups per channel
    (36, 3, 33, 31),                # sliced, scalar
    (7, 64, 9, 5),                  # sliced, scalar
    (2, 1200, 1, 3),                # sliced, scalar, S = 1
]
# run a second time on views one float past a 16-byte boundary: an owned and a sliced-vector case
EVAL_OFFSET_CASES = [(200, 64, 8, 8), (40, 8, 32, 32)]

TWO_PASS_CASES = [(7, 64, 9, 5), (40, 8, 32, 32), (3, 512, 2, 2)]
TWO_PASS_OFFSET_CASE = (24, 16, 16, 12)         # x * 0.5 - 40: the second pass around the mean keeps the variance

ACTS = (ACT_LRELU, ACT_NONE, ACT_SIGMOID)


def run_id(run):
    C, H, W, parts = run.case
    s = '%dx%dx%d_%s_%s' % (C, H, W, '+'.join(str(n) for n in parts), ('none', 'lrelu', 'sigmoid')[run.act])
    if run.momentum is None:
        s += '_cumulative'
    if not run.affine:
        s += '_noaffine'
    if run.shifted:
        s += '_shifted'
    return s


def bounds_of(parts):
    out, pos = [], 0
    for n in parts:
        out.append((pos, pos + n))
        pos += n
    return out


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
Inputs = collections.namedtuple('Inputs', ['x', 'gy', 'gamma', 'beta', 'rm', 'rv'])


def inputs(N, C, H, W, shifted_parts=None):
    """One recipe for every case (N: the total over ranks)."""
    g = torch.Generator().manual_seed(1000 * N + C + H * W)
    x = torch.randn((N, C, H, W), generator=g) * 0.7 + torch.randn((1, C, 1, 1), generator=g)
    gy = torch.randn((N, C, H, W), generator=g)
    if shifted_parts is not None:
        for r, (b, e) in enumerate(bounds_of(shifted_parts)):
            x[b:e] += 3.0 if r % 2 == 0 else -3.0
    gamma = torch.rand((C,), generator=torch.Generator().manual_seed(5)) + 0.5
    beta = torch.rand((C,), generator=torch.Generator().manual_seed(6)) - 0.5
    rm = torch.rand((C,), generator=torch.Generator().manual_seed(7))
    rv = torch.rand((C,), generator=torch.Generator().manual_seed(8)) + 0.5
    return Inputs(x, gy, gamma, beta, rm, rv)


def run_inputs(run):
    C, H, W, parts = run.case
    ins = inputs(sum(parts), C, H, W, parts if run.shifted else None)
    if not run.affine:
        ins = ins._replace(gamma=None, beta=None)
    return ins


def factor_of(run):
    """The running-estimate factor the wrapper is handed."""
    return 1.0 / (run.tracked + 1) if run.momentum is None else run.momentum


# ---------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------
def activation(z, act, mask=None):
    """act(z); LeakyReLU on the branches of ``mask`` where one is given."""
    if act == ACT_LRELU:
        return F.leaky_relu(z, SLOPE) if mask is None else torch.where(mask, z, SLOPE * z)
    if act == ACT_SIGMOID:
        return torch.sigmoid(z)
    return z


def bn_module(C, gamma, beta, rm, rv, momentum, eps, dtype, tracked=0):
    """nn.BatchNorm2d with the given state; without affine parameters gamma = 1 and beta = 0 stand in, so that
    their gradients are the sums the rank-split backward returns either way."""
    m = torch.nn.BatchNorm2d(C, momentum=momentum, eps=eps)
    with torch.no_grad():
        if gamma is not None:
            m.weight.copy_(gamma)
            m.bias.copy_(beta)
        else:
            m.weight.fill_(1.0)
            m.bias.zero_()
        m.running_mean.copy_(rm)
        m.running_var.copy_(rv)
        m.num_batches_tracked.fill_(tracked)
    return m.to(dtype)


def split_reference(x, gy, gamma, beta, rm, rv, momentum, eps, act, parts, dtype, mask=None, tracked=0):
    """nn.BatchNorm2d of ``dtype`` in train mode over the CONCATENATED batch, the activation, backward.  -> dict:
    per-rank slices ``y`` and ``dx``, the global ``dgamma``, ``dbeta``, ``running_mean`` and ``running_var`` (the
    unbiased variance over the global count), ``mean``, ``invstd`` and ``count``, the pre-activation ``z`` and the
    terms ``dz`` / ``dzx`` of dbeta / dgamma."""
    C = x.shape[1]
    m = bn_module(C, gamma, beta, rm, rv, momentum, eps, dtype, tracked).train()
    xi = x.detach().clone().to(dtype).requires_grad_(True)
    z = m(xi)
    z.retain_grad()
    y = activation(z, act, mask)
    y.backward(gy.to(dtype))
    xd = xi.detach()
    mean = xd.mean(dim=(0, 2, 3))
    invstd = 1.0 / torch.sqrt(xd.var(dim=(0, 2, 3), unbiased=False) + eps)
    xhat = (xd - mean[None, :, None, None]) * invstd[None, :, None, None]
    bounds = bounds_of(parts)
    return {'y': [y.detach()[b:e] for b, e in bounds], 'dx': [xi.grad[b:e] for b, e in bounds],
            'dgamma': m.weight.grad, 'dbeta': m.bias.grad, 'running_mean': m.running_mean.clone(),
            'running_var': m.running_var.clone(), 'mean': mean, 'invstd': invstd,
            'count': float(x.shape[0] * x.shape[2] * x.shape[3]), 'z': z.detach(), 'dz': z.grad,
            'dzx': z.grad * xhat, 'tracked': int(m.num_batches_tracked)}


def eval_reference(x, gy, gamma, beta, rm, rv, eps, act, dtype, mask=None):
    """nn.BatchNorm2d of ``dtype`` in eval mode, the activation, backward."""
    m = bn_module(x.shape[1], gamma, beta, rm, rv, 0.1, eps, dtype).eval()
    xi = x.detach().clone().to(dtype).requires_grad_(True)
    z = m(xi)
    z.retain_grad()
    y = activation(z, act, mask)
    y.backward(gy.to(dtype))
    xhat = (xi.detach() - m.running_mean[None, :, None, None]) / torch.sqrt(m.running_var + eps)[None, :, None, None]
    return {'y': y.detach(), 'dx': xi.grad, 'dgamma': m.weight.grad, 'dbeta': m.bias.grad, 'z': z.detach(),
            'dz': z.grad, 'dzx': z.grad * xhat, 'running_mean': m.running_mean, 'running_var': m.running_var,
            'tracked': int(m.num_batches_tracked)}


def lrelu_ties(z64, mask):
    """The elements whose device branch differs from the float64 one, checked against the cap: a condition, not a
    measurement.  At most max(2, 1e-6 numel) of them, each with |z| <= 2e-6 max|z|.  -> their number."""
    ties = (z64 > 0) != mask
    n = int(ties.sum())
    assert n <= max(2, 1e-6 * z64.numel()), '%d branches differ from float64' % n
    if n:
        worst = float(z64[ties].abs().max())
        assert worst <= 2e-6 * float(z64.abs().max()), 'a branch differs at |z| = %.3e' % worst
    return n


# ---------------------------------------------------------------------------------------------------------------
# replay of the ranks of one frame-sharded step in one process
# ---------------------------------------------------------------------------------------------------------------
def replay(world, n_calls, step):
    """Run ``step(rank, all_reduce)`` for every rank, one after another, in ``n_calls + 1`` passes; -> the last
    pass's results.  ``all_reduce(t)`` of rank r records, at its k-th call of a pass, the tensor it is given, then
    overwrites it IN PLACE with the sum over ranks -- its own tensor and what the other ranks recorded at call k of
    the PREVIOUS pass (nothing in the first) -- added in rank order on every rank, as a real all-reduce hands every
    rank the same bits; it returns the tensor.  Call k depends on the sums of the calls before it, so its record is
    right from pass k + 1 on and its sum from pass k + 2 on: with ``n_calls`` calls per step the last of
    ``n_calls + 1`` passes is the step every rank of a real process group would have run.  ``step`` must start from
    fresh state in every pass."""
    prev = [[] for _ in range(world)]
    results = None
    for _ in range(n_calls + 1):
        cur = [[] for _ in range(world)]

        def make(r):
            def all_reduce(t, op=None):
                k = len(cur[r])
                cur[r].append(t.detach().clone())
                total = torch.zeros_like(t)
                for o in range(world):
                    if o == r:
                        total += cur[r][k]
                    elif k < len(prev[o]):
                        total += prev[o][k]
                with torch.no_grad():
                    t.copy_(total)
                return t
            return all_reduce
        results = [step(r, make(r)) for r in range(world)]
        for r in range(world):
            assert len(cur[r]) == n_calls, 'rank %d made %d all-reduce calls, not %d' % (r, len(cur[r]), n_calls)
        prev = cur
    return results


def run_split(run, ins, fwd, bwd, prepare=lambda t: t):
    """One rank-split step of ``run`` through ``replay``: ``fwd`` / ``bwd`` have the signatures of
    ``_hip.batchnorm_sync_train_fwd`` / ``_hip.batchnorm_sync_bwd``, ``prepare`` puts a CPU tensor where they want
    it.  -> per rank a dict: y, mean, invstd, count, running_mean, running_var, dx, sum_dz, sum_dzx.  Three passes
    for the two all-reduce calls of the forward pass, then two for the one of the backward pass; the running
    statistics are fresh clones in every pass."""
    C, H, W, parts = run.case
    bounds = bounds_of(parts)
    xs = [prepare(ins.x[b:e].contiguous()) for b, e in bounds]
    gys = [prepare(ins.gy[b:e].contiguous()) for b, e in bounds]
    gamma = prepare(ins.gamma) if ins.gamma is not None else None
    beta = prepare(ins.beta) if ins.beta is not None else None

    def forward(r, all_reduce):
        rm, rv = prepare(ins.rm.clone()), prepare(ins.rv.clone())
        y, mean, invstd, count = fwd(xs[r], gamma, beta, rm, rv, factor_of(run), EPS, run.act, SLOPE, all_reduce)
        return {'y': y, 'mean': mean, 'invstd': invstd, 'count': count, 'running_mean': rm, 'running_var': rv}
    out = replay(len(parts), 2, forward)

    def backward(r, all_reduce):
        f = out[r]
        dx, sum_dz, sum_dzx = bwd(xs[r], f['y'], gys[r], f['mean'], f['invstd'], gamma, f['count'], run.act, SLOPE,
                                  all_reduce)
        return {'dx': dx, 'sum_dz': sum_dz, 'sum_dzx': sum_dzx}
    for f, b in zip(out, replay(len(parts), 1, backward)):
        f.update(b)
    return out
