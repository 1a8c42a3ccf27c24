"""Batch norm outside the chunked training step against float64 on the MI355X (csrc/batchnorm.hip), on the case
lists of tests/batchnorm_refs.py -- tests/test_batchnorm_routes_host.py asserts, without a GPU, which kernel and
which slices each case runs, and checks the references and the replay harness used here.

* The rank-split forms behind frame-sharded data parallelism (``_hip.batchnorm_sync_train_fwd`` /
  ``_hip.batchnorm_sync_bwd``: k_bn_moment_part<1>, <2> about a foreign centre, k_bn_bwd_part<false>, k_bn_combine,
  k_bn_bwd_apply<4 / 1, false>): the ranks of a case run one after another in this process (``refs.replay``), no
  process group and no second process.
* Eval mode (``batchnorm_eval_fwd`` + ``batchnorm_bwd(batch_stats=0)``) on the owned and on the sliced path.
* The two-pass public API (``batchnorm_train_fwd`` + ``batchnorm_bwd(batch_stats=1)``).

Every output is compared with the fp32 CPU result and with a float64 evaluation by ``tests.test_gpu_kernels.close``
as it stands (error against float64 at most 1e-4 of the result's maximum and at most max(8 x the fp32 CPU error,
3e-6); sums pass their terms as ``sum_of``).  LeakyReLU gradients are compared on the DEVICE's branches, as
test_batchnorm_chunked_paths does; ``refs.lrelu_ties`` caps what may differ from the float64 branches.

Figures measured on the MI355X (largest over all cases of a family; e_hip / e_cpu = max error against float64 over
the result's maximum, of the device and of the fp32 CPU result):

    output                   e_hip     e_cpu     case of the largest e_hip
    split y                  1.7e-07   5.7e-08   3x7x3_70+9_lrelu
    split dx                 3.7e-07   2.7e-07   4x2x2_1_lrelu
    split dgamma             7.0e-07   2.2e-07   3x7x3_70+9_lrelu
    split dbeta              2.6e-07   8.0e-08   16x16x16_33+32_lrelu
    split mean               2.3e-07   8.2e-08   3x7x3_70+9_lrelu
    split invstd             1.5e-07   7.1e-08   3x7x3_70+9_lrelu
    split rmean              1.2e-07   6.4e-08   33x2x2_130+0+7_lrelu_cumulative
    split rvar               1.0e-07   1.0e-07   512x4x4_40_lrelu
    two-pass y               2.3e-07   1.2e-07   8x32x32_40_sigmoid
    two-pass dx              3.0e-07   2.0e-07   8x32x32_40_sigmoid
    two-pass dgamma          3.4e-07   1.6e-07   8x32x32_40_sigmoid
    two-pass dbeta           2.1e-07   1.8e-07   8x32x32_40_sigmoid
    two-pass mean            1.5e-07   1.4e-07   8x32x32_40_lrelu
    two-pass invstd          1.3e-07   1.1e-07   512x4x4_40_lrelu (split as two-pass)
    two-pass rmean           9.6e-08   6.3e-08   8x32x32_40_lrelu
    two-pass rvar            1.0e-07   6.1e-08   64x9x5_7_lrelu
    two-pass offset y        4.5e-06   1.8e-06   16x16x12_24_lrelu
    two-pass offset dx       2.5e-07   1.6e-07   16x16x12_24_lrelu
    two-pass offset dgamma   9.1e-06   3.9e-06   16x16x12_24_lrelu
    two-pass offset dbeta    8.8e-08   5.7e-08   16x16x12_24_lrelu
    two-pass offset mean     1.6e-07   2.0e-07   16x16x12_24_lrelu
    two-pass offset invstd   8.6e-08   5.3e-08   16x16x12_24_lrelu
    two-pass offset rmean    1.8e-07   6.5e-08   16x16x12_24_lrelu
    two-pass offset rvar     6.2e-08   6.2e-08   16x16x12_24_lrelu
    autograd y               1.3e-07   8.9e-08   33x2x2_130+0+7_lrelu_cumulative two steps
    autograd dx              1.3e-07   1.2e-07   33x2x2_130+0+7_lrelu_cumulative two steps
    autograd dgamma          2.9e-07   9.7e-08   33x2x2_130+0+7_lrelu_cumulative two steps
    autograd dbeta           1.3e-07   1.3e-07   33x2x2_130+0+7_lrelu_cumulative two steps
    autograd rmean           1.0e-07   6.0e-08   33x2x2_130+0+7_lrelu_cumulative two steps
    autograd rvar            9.1e-08   9.8e-08   33x2x2_130+0+7_lrelu_cumulative two steps
    eval y                   1.2e-07   1.0e-07   200x64x8x8 sigmoid
    eval dx                  3.1e-07   3.0e-07   210x96x2x2 sigmoid
    eval dgamma              4.5e-07   5.0e-07   36x3x33x31 sigmoid
    eval dbeta               5.0e-07   5.8e-07   36x3x33x31 lrelu

(Cases read C x H x W _ frames per rank _ activation, eval cases N x C x H x W.  two-pass = batchnorm_train_fwd +
batchnorm_bwd(batch_stats=1), the single-rank split case included; two-pass offset = the same on x * 0.5 - 40;
autograd = BatchNormActFn over the replayed ranks; eval = the autograd node and the direct calls, accumulating,
overwriting and on the offset views.)  ``close`` asks for e_hip <= max(8 x e_cpu, 3e-6).  On the split, two-pass,
autograd and eval rows every e_hip lies under the 3e-6 floor alone, with 4.3x room at the least (the split dgamma
of (3, 7, 3, (70, 9)), before the allowance its terms add); where 8 x e_cpu is the larger bound (eval dgamma and
dbeta, for instance) the check is looser still.  On the offset channels the fp32 CPU result itself is 1.8e-6 (y) and
3.9e-6 (dgamma) away from float64 -- the cancellation in x - mean more than a hundred standard deviations from zero
-- so e_hip is above the floor and 8 x e_cpu is the bound, with 3.2x room (y) and 3.4x (dgamma).  In eval mode y
equals the fp32 CPU result to the last bit on most rows.
"""
import copy

import pytest
import torch

from behavenet_amd import _hip
from tests import batchnorm_refs as refs
from tests.measured import measured_close
from tests.test_gpu_kernels import SLOPE
from tests.test_gpu_guard_bands import guarded, finite, _bands_stay_untouched  # noqa: F401 (autouse fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
EPS = refs.EPS
F32, F64 = torch.float32, torch.float64
SYNC_IDS = [refs.run_id(r) for r in refs.SYNC_RUNS]
EVAL_IDS = ['%dx%dx%dx%d' % c for c in refs.EVAL_CASES]
ACT_IDS = {refs.ACT_LRELU: 'lrelu', refs.ACT_NONE: 'none', refs.ACT_SIGMOID: 'sigmoid'}

SYNC_GUARD_CASES = [(32, 8, 8, (5, 3)), (3, 7, 3, (70, 9)), (1200, 1, 4, (3, 1, 2))]     # vector, scalar, S = 1
EVAL_GUARD_CASES = [(40, 8, 32, 32), (7, 64, 9, 5), (2, 1200, 1, 3)]
TWO_PASS_GUARD_CASES = [(40, 8, 32, 32), (7, 64, 9, 5), (2, 1200, 1, 3)]


def to_dev(t):
    return t.to(DEV).contiguous()


def one_float_past_16_bytes(t):
    """A contiguous device copy of ``t`` that starts 4 bytes past a 16-byte boundary."""
    buf = torch.empty((t.numel() + 8,), dtype=torch.float32, device=DEV)
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def terms_with(terms, *priors):
    """The terms of a per-channel sum (N, C, H, W) with one more frame per prior vector (C,)."""
    extra = []
    for p in priors:
        e = torch.zeros((1,) + tuple(terms.shape[1:]), dtype=terms.dtype)
        e[0, :, 0, 0] = p.to(terms.dtype)
        extra.append(e)
    return torch.cat([terms] + extra, dim=0)


# ---------------------------------------------------------------------------------------------------------------
# the rank-split forms
# ---------------------------------------------------------------------------------------------------------------
def device_split(run, ins, prepare=to_dev):
    return refs.run_split(run, ins, _hip.batchnorm_sync_train_fwd, _hip.batchnorm_sync_bwd, prepare=prepare)


def check_split(run, ins, got, family):
    """Every output of the ranks ``got`` of ``run`` against the fp32 and float64 references."""
    parts = run.case[3]
    tag = ' [%s]' % refs.run_id(run)
    mask = None
    if run.act == refs.ACT_LRELU:
        mask = torch.cat([g['y'].detach().cpu() for g in got]) > 0
    r32, r64 = (refs.split_reference(*ins, run.momentum, EPS, run.act, parts, dt, mask=mask, tracked=run.tracked)
                for dt in (F32, F64))
    if mask is not None:
        refs.lrelu_ties(r64['z'], mask)
    for r, g in enumerate(got):
        assert g['y'].shape == g['dx'].shape == r64['y'][r].shape
        if parts[r] == 0:
            # a rank without frames: empty outputs, zero local sums, the statistics of everyone else (below)
            assert g['y'].numel() == 0 and g['dx'].numel() == 0
            assert not bool(g['sum_dz'].any()) and not bool(g['sum_dzx'].any())
            continue
        measured_close(g['y'], r32['y'][r], r64['y'][r], family + ' y' + tag)
        measured_close(g['dx'], r32['dx'][r], r64['dx'][r], family + ' dx' + tag)
    measured_close(sum(g['sum_dzx'] for g in got), r32['dgamma'], r64['dgamma'], family + ' dgamma' + tag,
                   sum_of=r64['dzx'])
    measured_close(sum(g['sum_dz'] for g in got), r32['dbeta'], r64['dbeta'], family + ' dbeta' + tag,
                   sum_of=r64['dz'])
    for key, name in (('mean', ' mean'), ('invstd', ' invstd'), ('running_mean', ' rmean'), ('running_var', ' rvar')):
        measured_close(got[0][key], r32[key], r64[key], family + name + tag)
        for r, g in enumerate(got):
            assert torch.equal(g[key], got[0][key]), '%s of rank %d differs from rank 0' % (key, r)
    for g in got:
        assert g.get('count', r64['count']) == r64['count']


@pytest.mark.parametrize('run', refs.SYNC_RUNS, ids=SYNC_IDS)
def test_rank_split_forms_against_float64(run):
    ins = refs.run_inputs(run)
    check_split(run, ins, device_split(run, ins), 'split')


def two_pass(ins, momentum, act, prepare=to_dev, out=None):
    """batchnorm_train_fwd + batchnorm_bwd(batch_stats=1) -> the dict of one rank of ``device_split``."""
    x, gy, rm, rv = (prepare(t) for t in (ins.x, ins.gy, ins.rm.clone(), ins.rv.clone()))
    gamma, beta = (prepare(t) if t is not None else None for t in (ins.gamma, ins.beta))
    y, mean, invstd = _hip.batchnorm_train_fwd(x, gamma, beta, rm, rv, momentum, EPS, act, SLOPE,
                                               y=out[0] if out else None)
    C = x.shape[1]
    mean, invstd = prepare(mean), prepare(invstd)
    dgamma, dbeta = (prepare(torch.full((C,), float('nan'))) for _ in range(2))
    dx = _hip.batchnorm_bwd(x, y, gy, mean, invstd, gamma, dgamma, dbeta, False, 1, act, SLOPE,
                            dx=out[1] if out else None)
    return {'y': y, 'mean': mean, 'invstd': invstd, 'running_mean': rm, 'running_var': rv, 'dx': dx,
            'sum_dz': dbeta, 'sum_dzx': dgamma}


def test_single_rank_equals_the_two_pass_api():
    """One rank: the same data through batchnorm_train_fwd + batchnorm_bwd(batch_stats=1), within the same
    tolerance of the same reference."""
    run = refs.SyncRun(refs.SINGLE_RANK_CASE)
    ins = refs.run_inputs(run)
    check_split(run, ins, [two_pass(ins, run.momentum, run.act)], 'split as two-pass')


@pytest.mark.parametrize('act', refs.ACTS, ids=[ACT_IDS[a] for a in refs.ACTS])
@pytest.mark.parametrize('case', refs.TWO_PASS_CASES, ids=['%dx%dx%dx%d' % c for c in refs.TWO_PASS_CASES])
def test_two_pass_api_against_float64(case, act):
    N, C, H, W = case
    run = refs.SyncRun((C, H, W, (N,)), act=act)
    ins = refs.inputs(N, C, H, W)
    check_split(run, ins, [two_pass(ins, run.momentum, act)], 'two-pass')


def test_two_pass_statistics_keep_the_variance_of_an_offset_channel():
    """Channels more than a hundred standard deviations away from zero: the second pass about the mean keeps the
    variance."""
    N, C, H, W = refs.TWO_PASS_OFFSET_CASE
    run = refs.SyncRun((C, H, W, (N,)))
    ins = refs.inputs(N, C, H, W)
    ins = ins._replace(x=ins.x * 0.5 - 40.0)
    check_split(run, ins, [two_pass(ins, run.momentum, run.act)], 'two-pass offset')


def test_autograd_node_over_the_replayed_ranks(monkeypatch):
    """BatchNormActFn on its frame-sharded branch, two training steps with momentum=None: y, the gradients added
    into the .grad buffers (the ``direct`` branch), the cumulative running estimates and the batch counter.  Every
    pass of the replay gets a fresh deep copy of the module.  The counter starts at 2, so the steps' factors are
    1 / 3 and 1 / 4 and the running estimates end at rm0 / 2 + mean / 2: they depend on the initial buffers and on
    BOTH factors (from a counter of 0 the first factor, 1, would overwrite the buffers with the batch statistics
    and hide whatever factor the second step used on the same data)."""
    from behavenet_amd.fitting import distributed as bdist
    from behavenet_amd.hip_functions import BatchNormActFn, accumulate_into_param_grads
    C, H, W, parts = case = (33, 2, 2, (130, 0, 7))
    world, steps, tracked = len(parts), 2, 2
    ins = refs.inputs(sum(parts), C, H, W)
    bounds = refs.bounds_of(parts)
    g = torch.Generator().manual_seed(17)
    prior_g, prior_b = torch.rand((C,), generator=g) - 0.5, torch.rand((C,), generator=g) - 0.5

    def module(dt, device):
        m = refs.bn_module(C, ins.gamma, ins.beta, ins.rm, ins.rv, None, EPS, dt, tracked).to(device).train()
        return with_prior_grads(m)

    def with_prior_grads(m):
        for p, prior in ((m.weight, prior_g), (m.bias, prior_b)):
            p.grad = prior.to(p.dtype).to(p.device).clone()
        return m
    base = module(F32, DEV)
    xs = [to_dev(ins.x[b:e]) for b, e in bounds]
    gys = [to_dev(ins.gy[b:e]) for b, e in bounds]
    monkeypatch.setattr(bdist, 'frames_sharded', lambda: True)

    def step(r, all_reduce):
        monkeypatch.setattr(bdist, 'all_reduce_', all_reduce)
        m = with_prior_grads(copy.deepcopy(base))
        x = xs[r].clone().requires_grad_(True)
        for _ in range(steps):
            y = BatchNormActFn.apply(x, m.weight, m.bias, m, _hip.ACT_LRELU)
            with accumulate_into_param_grads():
                y.backward(gys[r])
        return {'y': y.detach(), 'dx': x.grad, 'm': m}
    got = refs.replay(world, 3 * steps, step)
    assert int(base.num_batches_tracked) == tracked and torch.equal(base.weight.grad.cpu(), prior_g)

    mask = torch.cat([o['y'].cpu() for o in got]) > 0
    want = {}
    for dt in (F32, F64):
        m = module(dt, 'cpu')
        xi = ins.x.detach().clone().to(dt).requires_grad_(True)
        for _ in range(steps):
            z = m(xi)
            y = torch.where(mask, z, SLOPE * z)
            y.backward(ins.gy.to(dt))
        want[dt] = (y.detach(), xi.grad, m, z.detach())
    refs.lrelu_ties(want[F64][3], mask)
    tag = ' [%s two steps]' % refs.run_id(refs.SyncRun(case, momentum=None))
    for r, (b, e) in enumerate(bounds):
        assert got[r]['y'].shape[0] == got[r]['dx'].shape[0] == e - b
        if e > b:
            measured_close(got[r]['y'], want[F32][0][b:e], want[F64][0][b:e], 'autograd y' + tag)
            measured_close(got[r]['dx'], want[F32][1][b:e], want[F64][1][b:e], 'autograd dx' + tag)
    # every rank's buffer holds the prior and its own share of the two steps' sums
    r64 = refs.split_reference(*ins, None, EPS, _hip.ACT_LRELU, parts, F64, mask=mask)
    for name, attr, prior, terms in (('dgamma', 'weight', prior_g, r64['dzx']), ('dbeta', 'bias', prior_b, r64['dz'])):
        total = sum(getattr(o['m'], attr).grad for o in got)
        w32, w64 = (getattr(want[dt][2], attr).grad + (world - 1) * prior.to(dt) for dt in (F32, F64))
        measured_close(total, w32, w64, 'autograd ' + name + tag,
                       sum_of=terms_with(torch.cat([terms] * steps), *([prior] * world)))
    # (the reference's own estimates sit where factors 1 / 3 and 1 / 4 put them: half the initial buffer, half the
    # batch statistic; with a second factor of 1 / 3 or 1 / 2 they would be 4 / 9 or 1 / 3 of the buffer)
    assert torch.allclose(want[F64][2].running_mean, 0.5 * ins.rm.double() + 0.5 * r64['mean'], rtol=1e-12, atol=0)
    for name, key in (('rmean', 'running_mean'), ('rvar', 'running_var')):
        first = getattr(got[0]['m'], key)
        measured_close(first, getattr(want[F32][2], key), getattr(want[F64][2], key), 'autograd ' + name + tag)
        for o in got:
            assert torch.equal(getattr(o['m'], key), first)
            assert int(o['m'].num_batches_tracked) == tracked + steps == int(want[F64][2].num_batches_tracked)


# ---------------------------------------------------------------------------------------------------------------
# eval mode
# ---------------------------------------------------------------------------------------------------------------
def check_eval(case, act, ins, y, dx, dgamma, dbeta, family, prior=None):
    """``prior``: what dgamma / dbeta held before an accumulating call."""
    tag = ' [%dx%dx%dx%d %s]' % (case + (ACT_IDS[act],))
    mask = (y.detach().cpu() > 0) if act == refs.ACT_LRELU else None
    r32, r64 = (refs.eval_reference(*ins, EPS, act, dt, mask=mask) for dt in (F32, F64))
    if mask is not None:
        refs.lrelu_ties(r64['z'], mask)
    measured_close(y, r32['y'], r64['y'], family + ' y' + tag)
    measured_close(dx, r32['dx'], r64['dx'], family + ' dx' + tag)
    for name, got, terms, p in (('dgamma', dgamma, r64['dzx'], prior and prior[0]),
                                ('dbeta', dbeta, r64['dz'], prior and prior[1])):
        w32, w64 = r32[name], r64[name]
        if p is not None:
            w32, w64, terms = w32 + p, w64 + p.double(), terms_with(terms, p)
        measured_close(got, w32, w64, family + ' ' + name + tag, sum_of=terms)


@pytest.mark.parametrize('act', refs.ACTS, ids=[ACT_IDS[a] for a in refs.ACTS])
@pytest.mark.parametrize('case', refs.EVAL_CASES, ids=EVAL_IDS)
def test_eval_mode_through_the_autograd_node(case, act):
    from behavenet_amd.hip_functions import BatchNormActFn
    N, C, H, W = case
    ins = refs.inputs(*case)
    m = refs.bn_module(C, ins.gamma, ins.beta, ins.rm, ins.rv, 0.1, EPS, F32).to(DEV).eval()
    xh = to_dev(ins.x).requires_grad_(True)
    yh = BatchNormActFn.apply(xh, m.weight, m.bias, m, act)
    yh.backward(to_dev(ins.gy))
    check_eval(case, act, ins, yh, xh.grad, m.weight.grad, m.bias.grad, 'eval')
    # eval mode leaves the running buffers and the counter alone, bit for bit
    assert torch.equal(m.running_mean.cpu(), ins.rm) and torch.equal(m.running_var.cpu(), ins.rv)
    assert int(m.num_batches_tracked) == 0


def eval_direct(ins, act, accumulate, fill, place=to_dev):
    """batchnorm_eval_fwd + batchnorm_bwd(batch_stats=0) through _hip; dgamma / dbeta start as ``fill``."""
    x, gy = place(ins.x), place(ins.gy)
    gamma, beta, rm, rv = (to_dev(t) for t in (ins.gamma, ins.beta, ins.rm, ins.rv))
    y, invstd = _hip.batchnorm_eval_fwd(x, gamma, beta, rm, rv, EPS, act, SLOPE)
    dgamma, dbeta = to_dev(fill[0].clone()), to_dev(fill[1].clone())
    dx = _hip.batchnorm_bwd(x, y, gy, rm, invstd, gamma, dgamma, dbeta, accumulate, 0, act, SLOPE)
    return y, dx, dgamma, dbeta


@pytest.mark.parametrize('case', [(200, 64, 8, 8), (40, 8, 32, 32)], ids=['owned', 'sliced'])
def test_eval_backward_accumulates_or_overwrites(case):
    """accumulate=True onto a known vector leaves prior + gradient, accumulate=False onto NaN the gradient alone."""
    assert refs.route(case).owned == (case == (200, 64, 8, 8))
    C = case[1]
    ins = refs.inputs(*case)
    g = torch.Generator().manual_seed(23)
    prior = (torch.rand((C,), generator=g) - 0.5, torch.rand((C,), generator=g) - 0.5)
    check_eval(case, refs.ACT_LRELU, ins, *eval_direct(ins, refs.ACT_LRELU, True, prior), 'eval accumulate',
               prior=prior)
    nan = (torch.full((C,), float('nan')),) * 2
    check_eval(case, refs.ACT_LRELU, ins, *eval_direct(ins, refs.ACT_LRELU, False, nan), 'eval overwrite')


@pytest.mark.parametrize('act', [refs.ACT_LRELU, refs.ACT_SIGMOID], ids=['lrelu', 'sigmoid'])
@pytest.mark.parametrize('case', refs.EVAL_OFFSET_CASES, ids=['%dx%dx%dx%d' % c for c in refs.EVAL_OFFSET_CASES])
def test_eval_mode_on_views_one_float_past_a_16_byte_boundary(case, act):
    """x and dy start 4 bytes past a 16-byte boundary: the owned and the vector forms must refuse them (the host
    test holds the routing), and the scalar forms that take over must be right."""
    assert not refs.route(case, aligned=False).owned and not refs.route(case, aligned=False).apply_vec
    ins = refs.inputs(*case)
    nan = (torch.full((case[1],), float('nan')),) * 2
    check_eval(case, act, ins, *eval_direct(ins, act, False, nan, place=one_float_past_16_bytes), 'eval offset view')


# ---------------------------------------------------------------------------------------------------------------
# guard bands
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', SYNC_GUARD_CASES, ids=['vector', 'scalar', 'one_slice'])
def test_rank_split_forms_under_guard_bands(case):
    assert [r.moment_vec for r in refs.route(case)] == [case != (3, 7, 3, (70, 9))] * len(case[3])
    assert all(r.S == 1 for r in refs.route(case)) == (case == (1200, 1, 4, (3, 1, 2)))
    run = refs.SyncRun(case)

    def fwd(*args):
        # (y, mean and invstd are operands of the backward pass: between bands as well)
        y, mean, invstd, count = _hip.batchnorm_sync_train_fwd(*args)
        finite(y, 'y of %s' % (case,))
        return guarded(y), guarded(mean), guarded(invstd), count
    for g in refs.run_split(run, refs.run_inputs(run), fwd, _hip.batchnorm_sync_bwd, prepare=guarded):
        for key in ('y', 'dx', 'mean', 'invstd', 'running_mean', 'running_var', 'sum_dz', 'sum_dzx'):
            finite(g[key], '%s of %s' % (key, case))


@pytest.mark.parametrize('case', EVAL_GUARD_CASES, ids=['vector', 'scalar', 'one_slice'])
def test_eval_mode_under_guard_bands(case):
    r = refs.route(case)
    assert not r.owned and r.apply_vec == (case == (40, 8, 32, 32)) and (r.S == 1) == (case == (2, 1200, 1, 3))
    N, C, H, W = case
    ins = refs.inputs(*case)
    x, gy, gamma, beta, rm, rv = (guarded(t) for t in ins)
    for act in refs.ACTS:
        y, invstd = _hip.batchnorm_eval_fwd(x, gamma, beta, rm, rv, EPS, act, SLOPE)
        finite(y, 'y of %s' % (case,))
        y, invstd = guarded(y), guarded(invstd)
        nan = torch.full((C,), float('nan'))
        dgamma, dbeta, dx = guarded(nan), guarded(nan), guarded(torch.full(case, float('nan')))
        _hip.batchnorm_bwd(x, y, gy, rm, invstd, gamma, dgamma, dbeta, False, 0, act, SLOPE, dx=dx)
        for name, t in (('dx', dx), ('dgamma', dgamma), ('dbeta', dbeta)):
            finite(t, '%s of %s' % (name, case))


@pytest.mark.parametrize('case', TWO_PASS_GUARD_CASES, ids=['vector', 'scalar', 'one_slice'])
def test_two_pass_api_under_guard_bands(case):
    r = refs.route(case)
    assert r.moment_vec == (case == (40, 8, 32, 32)) and (r.S == 1) == (case == (2, 1200, 1, 3))
    N, C, H, W = case
    ins = refs.inputs(*case)
    for act in refs.ACTS:
        out = (guarded(torch.full(case, float('nan'))), guarded(torch.full(case, float('nan'))))
        for key, t in two_pass(ins, 0.1, act, prepare=guarded, out=out).items():
            finite(t, '%s of %s' % (key, case))


# ---------------------------------------------------------------------------------------------------------------
# determinism: fixed-order reductions, no atomics
# ---------------------------------------------------------------------------------------------------------------
def test_rank_split_forms_repeat_bit_for_bit():
    run = refs.SyncRun((3, 7, 3, (70, 9)))
    ins = refs.run_inputs(run)
    first, second = device_split(run, ins), device_split(run, ins)
    for a, b in zip(first, second):
        for key in a:
            assert a[key] == b[key] if key == 'count' else torch.equal(a[key], b[key]), key


def test_eval_mode_repeats_bit_for_bit():
    case = (40, 8, 32, 32)
    ins = refs.inputs(*case)
    zero = (torch.zeros((case[1],)),) * 2
    first, second = (eval_direct(ins, refs.ACT_LRELU, False, zero) for _ in range(2))
    assert all(torch.equal(a, b) for a, b in zip(first, second))


def test_two_pass_api_repeats_bit_for_bit():
    case = (7, 64, 9, 5)
    ins = refs.inputs(*case)
    first, second = (two_pass(ins, 0.1, refs.ACT_LRELU) for _ in range(2))
    for key in first:
        assert torch.equal(first[key], second[key]), key
