"""Host side of the batch-norm tests outside the chunked training step (tests/batchnorm_refs.py) WITHOUT a GPU.

1. ``bn_batchnorm_ws_bytes`` equals the restated scratch on the case lists and on a sweep of (N, C): the slice count
   enters that number as ``BNK_MAX_CHUNKS * (2 C S + 2 C) * 4``, so a restated ``bn_splits`` that drifts from
   batchnorm.hip fails here.
2. The case lists together reach every fact of ``route`` in both values.  A routing change in batchnorm.hip that
   moves a case fails THIS file instead of silently emptying a row of the device test.
3. ``split_reference`` (nn.BatchNorm2d) in float64 equals the batch-norm formulas written out in float64 on the
   concatenated batch: forward, the three gradients, the running estimates.
4. ``replay`` / ``run_split`` over a numpy stand-in for the three device calls of the rank-split forms (moment,
   backward sums, backward apply) reproduce the reference: the bookkeeping of the device test, checked here.  The
   stand-in walks the RESTATED slices, so the same test holds the restated slices to a partition of the frames --
   and shows that a wrong slice bound fails exactly the uneven cases.
5. The fp32 CPU reference takes the float64 LeakyReLU branch at every element of every listed case, so whatever
   differs on the device is the device's.
"""
import numpy as np
import pytest
import torch

from behavenet_amd import _hip
from tests import batchnorm_refs as refs

SYNC_IDS = [refs.run_id(r) for r in refs.SYNC_RUNS]
EVAL_IDS = ['%dx%dx%dx%d' % c for c in refs.EVAL_CASES]


def test_constants_are_the_librarys():
    from tests.test_gpu_kernels import SLOPE, act_ref
    assert (refs.ACT_NONE, refs.ACT_LRELU, refs.ACT_SIGMOID) == (_hip.ACT_NONE, _hip.ACT_LRELU, _hip.ACT_SIGMOID)
    assert refs.SLOPE == SLOPE
    assert refs.EPS == torch.nn.BatchNorm2d(1).eps
    z = torch.linspace(-3, 3, 25)
    for act in refs.ACTS:
        assert torch.equal(refs.activation(z, act), act_ref(z, act))


# ---------------------------------------------------------------------------------------------------------------
# 1. scratch
# ---------------------------------------------------------------------------------------------------------------
def _calls():
    """(N, C) of every library call the device test makes."""
    out = [(n, C) for C, H, W, parts in refs.SYNC_CASES for n in parts if n]
    out += [(N, C) for N, C, H, W in refs.EVAL_CASES + refs.TWO_PASS_CASES + [refs.TWO_PASS_OFFSET_CASE]]
    return out


def test_scratch_query_equals_the_restated_scratch_on_the_case_lists():
    lib = _hip.load()
    for N, C in _calls():
        assert lib.bn_batchnorm_ws_bytes(N, C) == refs.ws_bytes(N, C), (N, C)


def test_scratch_query_equals_the_restated_scratch_on_a_sweep():
    lib = _hip.load()
    for N in (1, 2, 3, 7, 31, 32, 33, 63, 64, 65, 70, 200, 590):
        for C in (1, 3, 8, 15, 16, 17, 31, 32, 33, 64, 70, 511, 512, 513, 1023, 1024, 1025, 1200):
            assert lib.bn_batchnorm_ws_bytes(N, C) == refs.ws_bytes(N, C), (N, C)
    assert lib.bn_batchnorm_ws_bytes(0, 8) == 0 == refs.ws_bytes(0, 8)


def test_slices_of_one_chunk():
    """bnk_set_slices hands one chunk min(S, N) slices (bn_splits never asks for more than N), and both slice
    walks are partitions of the frames."""
    for N, C in _calls():
        S = refs.bn_splits(N, C)
        assert refs.set_slices(N, S) == S <= N
        assert sorted(n for sl in refs.interleaved_slices(N, S) for n in sl) == list(range(N))
        assert [n for b, e in refs.moment_slices(N, S) for n in range(b, e)] == list(range(N))
    assert refs.set_slices(5, 9) == 5 and refs.set_slices(0, 1) == 1


# ---------------------------------------------------------------------------------------------------------------
# 2. coverage
# ---------------------------------------------------------------------------------------------------------------
def test_largest_tensor_is_a_few_mb():
    sizes = [sum(parts) * C * H * W * 4 for C, H, W, parts in refs.SYNC_CASES]
    sizes += [N * C * H * W * 4 for N, C, H, W in refs.EVAL_CASES + refs.TWO_PASS_CASES]
    assert max(sizes) == 600 * 600 * 4 * 4 < 6e6


def test_case_lists_reach_every_fact_of_route_in_both_values():
    sync = [r for case in refs.SYNC_CASES for r in refs.route(case)]
    evals = [refs.route(case) for case in refs.EVAL_CASES]
    # owned with 256 and with 1024 threads, and the sliced backward
    assert {r.threads for r in evals if r.owned} == {256, 1024}
    assert any(not r.owned for r in evals)
    # lin true and false
    assert {r.lin for r in evals if r.owned} == {True, False}
    # sliced vector and sliced scalar
    assert {r.apply_vec for r in evals if not r.owned} == {True, False}
    # the rank-split kernels on 16-byte groups and on scalars
    assert {r.moment_vec for r in sync if r.N} == {True, False}
    # S == 1 (with more than one frame), S == N, and 1 < S < N with N % S != 0: among the rank-split calls
    # (contiguous and interleaved slices) and among the sliced eval calls
    for group in ([r for r in sync if r.N], [r for r in evals if not r.owned]):
        assert any(r.S == 1 and r.N > 1 for r in group)
        assert any(r.S == r.N and r.N > 1 for r in group)
    # (uneven INTERLEAVED slices are reached only through k_bn_bwd_part<false> of (3, 7, 3, (70, 9)) and
    # (33, 2, 2, (130, 0, 7)): every sliced EVAL_CASES row has S == N or S == 1, so k_bn_bwd_apply_fin<false> never
    # walks uneven slices here -- the chunked train-mode tests of tests/test_gpu_kernels.py do that)
    assert any(1 < r.S < r.N and r.N % r.S != 0 and not r.even for r in sync)
    assert not any(1 < r.S < r.N for r in evals if not r.owned)
    assert any(r.even for r in sync if r.N)
    # a fill branch, on a slice that does and one that does not make a second trip
    assert any(r.fill and not r.multi_trip for r in sync)
    assert any(r.fill and r.multi_trip for r in sync)
    # k_bn_combine in one and in several workgroups
    assert {r.combine_blocks > 1 for r in sync} == {True, False}
    # a zero-frame rank, a single rank, two and three ranks
    assert any(0 in parts and len(parts) > 1 for C, H, W, parts in refs.SYNC_CASES)
    assert {len(parts) for C, H, W, parts in refs.SYNC_CASES} == {1, 2, 3}
    assert refs.SINGLE_RANK_CASE in refs.SYNC_CASES
    # every activation, both kinds of factor, with and without affine parameters, a foreign centre
    assert {r.act for r in refs.SYNC_RUNS} == set(refs.ACTS)
    assert {r.momentum for r in refs.SYNC_RUNS} == {0.1, None}
    assert {r.affine for r in refs.SYNC_RUNS} == {True, False}
    assert any(r.shifted for r in refs.SYNC_RUNS)


# what each row was chosen for: (N, S, vec, even, fill, multi_trip) per rank
SYNC_TABLE = {
    (32, 8, 8, (5, 3)): [(5, 5, True, True, True, False), (3, 3, True, True, True, False)],
    (3, 7, 3, (70, 9)): [(70, 64, False, False, False, False), (9, 9, False, True, False, False)],
    (1200, 1, 4, (3, 1, 2)): [(3, 1, True, True, True, False), (1, 1, True, True, True, False),
                              (2, 1, True, True, True, False)],
    (33, 2, 2, (130, 0, 7)): [(130, 31, True, False, True, False), (0, 1, True, True, False, False),
                              (7, 7, True, True, True, False)],
    (16, 16, 16, (33, 32)): [(33, 33, True, True, True, False), (32, 32, True, True, True, False)],
    (600, 1, 4, (590, 10)): [(590, 1, True, True, True, True), (10, 1, True, True, True, False)],
    (512, 4, 4, (40,)): [(40, 2, True, True, True, False)],
    (4, 2, 2, (1,)): [(1, 1, True, True, True, False)],
}
EVAL_TABLE = {      # (S, owned, threads, lin, vec)
    (5, 16, 8, 8): (5, True, 256, True, True),
    (200, 64, 8, 8): (16, True, 1024, True, True),
    (210, 96, 2, 2): (10, True, 256, True, True),
    (23, 70, 6, 4): (14, True, 256, False, True),
    (3, 1200, 1, 4): (1, True, 256, True, True),
    (40, 8, 32, 32): (40, False, None, None, True),
    (36, 3, 33, 31): (36, False, None, None, False),
    (7, 64, 9, 5): (7, False, None, None, False),
    (2, 1200, 1, 3): (1, False, None, None, False),
}


def test_routes_of_the_case_lists():
    assert sorted(SYNC_TABLE) == sorted(refs.SYNC_CASES) and sorted(EVAL_TABLE) == sorted(refs.EVAL_CASES)
    for case, want in SYNC_TABLE.items():
        got = [(r.N, r.S, r.moment_vec, r.even, r.fill, r.multi_trip) for r in refs.route(case)]
        assert got == want, (case, got)
    for case, want in EVAL_TABLE.items():
        r = refs.route(case)
        assert (r.S, r.owned, r.threads, r.lin, r.apply_vec) == want, (case, r)
    # two-pass API: sliced scalar, sliced vector, owned
    assert [refs.route(c).owned for c in refs.TWO_PASS_CASES] == [False, False, True]
    assert [refs.route(c).apply_vec for c in refs.TWO_PASS_CASES] == [False, True, True]
    # its statistics (k_bn_moment_part on a 3-d grid): one frame of 256 groups per slice fills on every thread
    r = refs.route((40, 8, 32, 32))
    assert r.fill and not r.multi_trip
    # (600, 1, 4, (590, 10)): the second trip of rank 0 holds 78 live threads, all of them without a second group
    assert refs.moment_loop(590, 4, True) == (True, 2)


def test_views_past_a_16_byte_boundary_are_refused_the_owned_and_vector_forms():
    for case in refs.EVAL_OFFSET_CASES:
        assert case in refs.EVAL_CASES
        r = refs.route(case, aligned=False)
        assert not r.owned and not r.apply_vec and not r.moment_vec
    assert [refs.route(c).owned for c in refs.EVAL_OFFSET_CASES] == [True, False]
    assert all(refs.route(c).apply_vec for c in refs.EVAL_OFFSET_CASES)


# ---------------------------------------------------------------------------------------------------------------
# 3. the reference against the formulas
# ---------------------------------------------------------------------------------------------------------------
def formulas(x, gy, gamma, beta, rm, rv, factor, eps, act, train):
    """Batch norm + activation + backward written out, in numpy float64 on the whole batch."""
    x, gy, rm, rv = (t.double().numpy() for t in (x, gy, rm, rv))
    C = x.shape[1]
    gamma = gamma.double().numpy() if gamma is not None else np.ones(C)
    beta = beta.double().numpy() if beta is not None else np.zeros(C)
    n = x.shape[0] * x.shape[2] * x.shape[3]
    bc = lambda v: v[None, :, None, None]
    if train:
        mean = x.sum(axis=(0, 2, 3)) / n
        var = ((x - bc(mean)) ** 2).sum(axis=(0, 2, 3)) / n
    else:
        mean, var = rm, rv
    invstd = 1.0 / np.sqrt(var + eps)
    xhat = (x - bc(mean)) * bc(invstd)
    z = xhat * bc(gamma) + bc(beta)
    if act == refs.ACT_LRELU:
        y, d = np.where(z > 0, z, refs.SLOPE * z), np.where(z > 0, 1.0, refs.SLOPE)
    elif act == refs.ACT_SIGMOID:
        y = 1.0 / (1.0 + np.exp(-z))
        d = y * (1.0 - y)
    else:
        y, d = z, np.ones_like(z)
    dz = gy * d
    dbeta = dz.sum(axis=(0, 2, 3))
    dgamma = (dz * xhat).sum(axis=(0, 2, 3))
    k = 1.0 / n if train else 0.0
    dx = bc(gamma * invstd) * (dz - bc(dbeta) * k - xhat * bc(dgamma) * k)
    out = {'y': y, 'dx': dx, 'dgamma': dgamma, 'dbeta': dbeta, 'mean': mean, 'invstd': invstd}
    if train:
        out['running_mean'] = (1 - factor) * rm + factor * mean
        out['running_var'] = (1 - factor) * rv + factor * var * (n / (n - 1.0) if n > 1 else 1.0)
    return out


def same(got, want, name, tol=1e-11):
    got = got.detach().double().numpy() if torch.is_tensor(got) else np.asarray(got)
    assert got.shape == want.shape, name
    assert np.abs(got - want).max() <= tol * max(np.abs(want).max(), 1e-30), (name, np.abs(got - want).max())


@pytest.mark.parametrize('run', refs.SYNC_RUNS, ids=SYNC_IDS)
def test_split_reference_in_float64_equals_the_formulas(run):
    ins = refs.run_inputs(run)
    parts = run.case[3]
    ref = refs.split_reference(*ins, run.momentum, refs.EPS, run.act, parts, torch.float64, tracked=run.tracked)
    want = formulas(*ins, refs.factor_of(run), refs.EPS, run.act, True)
    for key in ('y', 'dx'):
        assert [t.shape[0] for t in ref[key]] == list(parts)
        same(torch.cat(ref[key]), want[key], key)
    for key in ('dgamma', 'dbeta', 'mean', 'invstd', 'running_mean', 'running_var'):
        same(ref[key], want[key], key)
    same(ref['dz'].sum(dim=(0, 2, 3)), want['dbeta'], 'terms of dbeta')
    same(ref['dzx'].sum(dim=(0, 2, 3)), want['dgamma'], 'terms of dgamma')
    assert ref['count'] == sum(parts) * run.case[1] * run.case[2]
    assert ref['tracked'] == run.tracked + 1
    if parts == (1,):
        # 4 values per channel: the running variance moved by the biased variance times 4 / 3
        var = 1.0 / want['invstd'] ** 2 - refs.EPS
        same(ref['running_var'], 0.9 * ins.rv.double().numpy() + 0.1 * var * 4.0 / 3.0, 'unbiased factor')


@pytest.mark.parametrize('act', refs.ACTS)
@pytest.mark.parametrize('case', refs.EVAL_CASES, ids=EVAL_IDS)
def test_eval_reference_in_float64_equals_the_formulas(case, act):
    ins = refs.inputs(*case)
    ref = refs.eval_reference(*ins, refs.EPS, act, torch.float64)
    want = formulas(*ins, 0.0, refs.EPS, act, False)
    for key in ('y', 'dx', 'dgamma', 'dbeta'):
        same(ref[key], want[key], key)
    same(ref['dz'].sum(dim=(0, 2, 3)), want['dbeta'], 'terms of dbeta')
    same(ref['dzx'].sum(dim=(0, 2, 3)), want['dgamma'], 'terms of dgamma')
    assert torch.equal(ref['running_mean'], ins.rm.double()) and torch.equal(ref['running_var'], ins.rv.double())
    assert ref['tracked'] == 0


def test_a_passed_mask_replaces_the_references_own_branches():
    run = refs.SYNC_RUNS[0]
    ins = refs.run_inputs(run)
    args = (*ins, run.momentum, refs.EPS, run.act, run.case[3], torch.float64)
    plain = refs.split_reference(*args)
    same_mask = refs.split_reference(*args, mask=plain['z'] > 0)
    assert torch.equal(torch.cat(plain['dx']), torch.cat(same_mask['dx']))
    flipped = plain['z'] > 0
    flipped[0, 0, 0, 0] = ~flipped[0, 0, 0, 0]
    other = refs.split_reference(*args, mask=flipped)
    assert not torch.equal(torch.cat(plain['dx']), torch.cat(other['dx']))
    assert refs.lrelu_ties(plain['z'], plain['z'] > 0) == 0
    with pytest.raises(AssertionError):
        refs.lrelu_ties(plain['z'], flipped)


# ---------------------------------------------------------------------------------------------------------------
# 4. the replay harness over a numpy stand-in for the device calls
# ---------------------------------------------------------------------------------------------------------------
def _np(t):
    return t.detach().double().numpy()


def _act_grad_from_output(y, act):
    if act == refs.ACT_LRELU:
        return np.where(y > 0, 1.0, refs.SLOPE)
    if act == refs.ACT_SIGMOID:
        return y * (1.0 - y)
    return np.ones_like(y)


class StandIn(object):
    """bn_batchnorm_moment, bn_batchnorm_bwd_reduce and bn_batchnorm_bwd_apply in numpy float64 over the restated
    slices, behind wrappers that treat ``all_reduce`` as ``_hip.batchnorm_sync_train_fwd`` (in place) and
    ``_hip.batchnorm_sync_bwd`` (return value) do."""

    def __init__(self, slice_end=None):
        self.slice_end = slice_end

    def moment(self, x, center):
        N, C = x.shape[:2]
        xs = _np(x).reshape(N, C, -1)
        out = np.zeros(C)
        for b, e in refs.moment_slices(N, refs.bn_splits(N, C), self.slice_end):
            v = xs[b:e] - (center[None, :, None] if center is not None else 0.0)
            out += (v * v if center is not None else v).sum(axis=(0, 2))
        return out

    def bwd_reduce(self, x, y, dy, mean, invstd, act):
        N, C = x.shape[:2]
        xs, ys, ds = (_np(t).reshape(N, C, -1) for t in (x, y, dy))
        s0, s1 = np.zeros(C), np.zeros(C)
        for frames in refs.interleaved_slices(N, refs.set_slices(N, refs.bn_splits(N, C))):
            dz = ds[frames] * _act_grad_from_output(ys[frames], act)
            s0 += dz.sum(axis=(0, 2))
            s1 += (dz * (xs[frames] - mean[None, :, None]) * invstd[None, :, None]).sum(axis=(0, 2))
        return s0, s1

    def bwd_apply(self, x, y, dy, mean, invstd, gamma, sum_dz, sum_dzx, inv_count, act):
        bc = lambda v: v[None, :, None, None]
        dz = _np(dy) * _act_grad_from_output(_np(y), act)
        xhat = (_np(x) - bc(mean)) * bc(invstd)
        g = (gamma if gamma is not None else 1.0) * invstd
        return bc(g) * (dz - bc(sum_dz) * inv_count - xhat * bc(sum_dzx) * inv_count)

    def sync_train_fwd(self, x, gamma, beta, running_mean, running_var, momentum, eps, act, slope, all_reduce):
        n, c = x.shape[0], x.shape[1]
        hw = x.shape[2] * x.shape[3]
        s1 = torch.zeros((c + 1,), dtype=torch.float64)
        if n:
            s1[:c] = torch.from_numpy(self.moment(x, None))
            s1[c] = float(n)
        all_reduce(s1)
        count = float(s1[c]) * hw
        with np.errstate(all='ignore'):
            mean = _np(s1[:c]) / count
            s2 = torch.zeros((c,), dtype=torch.float64)
            if n:
                s2.copy_(torch.from_numpy(self.moment(x, mean)))
            all_reduce(s2)
            var = _np(s2) / count
            unbias = count / (count - 1.0) if count > 1 else 1.0
            invstd = 1.0 / np.sqrt(var + eps)
            running_mean.copy_(torch.from_numpy((1 - momentum) * _np(running_mean) + momentum * mean))
            running_var.copy_(torch.from_numpy((1 - momentum) * _np(running_var) + momentum * var * unbias))
            z = (_np(x) - mean[None, :, None, None]) * invstd[None, :, None, None]
        if gamma is not None:
            z = z * _np(gamma)[None, :, None, None] + _np(beta)[None, :, None, None]
        y = refs.activation(torch.from_numpy(z), act)
        return y, torch.from_numpy(mean), torch.from_numpy(invstd), count

    def sync_bwd(self, x, y, dy, mean, invstd, gamma, count, act, slope, all_reduce):
        n, c = x.shape[0], x.shape[1]
        local = torch.zeros((2, c), dtype=torch.float64)
        if n:
            s0, s1 = self.bwd_reduce(x, y, dy, _np(mean), _np(invstd), act)
            local[0], local[1] = torch.from_numpy(s0), torch.from_numpy(s1)
        total = all_reduce(local.clone())
        dx = torch.from_numpy(self.bwd_apply(x, y, dy, _np(mean), _np(invstd),
                                             _np(gamma) if gamma is not None else None, _np(total[0]),
                                             _np(total[1]), 1.0 / float(count), act))
        return dx, local[0], local[1]


def standin_errors(run, standin):
    """{output: error of run_split over the stand-in against the float64 reference, over the reference's maximum}"""
    ins = refs.run_inputs(run)
    parts = run.case[3]
    ref = refs.split_reference(*ins, run.momentum, refs.EPS, run.act, parts, torch.float64, tracked=run.tracked)
    got = refs.run_split(run, ins, standin.sync_train_fwd, standin.sync_bwd, prepare=lambda t: t.double())
    assert len(got) == len(parts)

    def err(a, b):
        return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
    errs = {'y': err(torch.cat([g['y'] for g in got]), torch.cat(ref['y'])),
            'dx': err(torch.cat([g['dx'] for g in got]), torch.cat(ref['dx'])),
            'dgamma': err(sum(g['sum_dzx'] for g in got), ref['dgamma']),
            'dbeta': err(sum(g['sum_dz'] for g in got), ref['dbeta'])}
    for r, g in enumerate(got):
        assert g['y'].shape[0] == g['dx'].shape[0] == parts[r]
        for key in ('mean', 'invstd', 'running_mean', 'running_var'):
            errs[key] = max(errs.get(key, 0.0), err(g[key], ref[key]))
            assert torch.equal(g[key], got[0][key]), (key, r)
        assert g['count'] == ref['count']
        if parts[r] == 0:
            assert not g['sum_dz'].any() and not g['sum_dzx'].any()
    return errs


@pytest.mark.parametrize('run', refs.SYNC_RUNS, ids=SYNC_IDS)
def test_replay_over_the_stand_in_reproduces_the_reference(run):
    errs = standin_errors(run, StandIn())
    assert max(errs.values()) <= 1e-11, errs


def test_replay_hands_every_rank_the_same_bits_and_needs_all_its_passes():
    """Three ranks whose fp32 sums depend on the order of addition: every rank gets the sum in rank order; a
    chain of two dependent calls is right after three passes and not after two."""
    vals = [torch.tensor([1e8], dtype=torch.float32), torch.tensor([-1e8], dtype=torch.float32),
            torch.tensor([1.0], dtype=torch.float32)]
    seen = refs.replay(3, 1, lambda r, ar: ar(vals[r].clone()))
    assert all(torch.equal(s, seen[0]) for s in seen) and float(seen[0]) == 1.0
    assert float(vals[2]) == 1.0                        # the caller's tensor is not what is recorded

    def chain(r, ar):
        a = ar(torch.tensor([float(r + 1)]))            # 1 + 2 + 3
        return ar(a * (r + 1))                          # 6 * (1 + 2 + 3)
    assert [float(t) for t in refs.replay(3, 2, chain)] == [36.0] * 3
    with pytest.raises(AssertionError):
        refs.replay(3, 1, chain)                        # (a step that makes more calls than it declared)


def test_a_wrong_slice_bound_fails_the_uneven_cases_and_no_even_one():
    """The moment kernel's bound ``(sp + 1) * N / S`` written as ``sp * N / S + N / S`` drops frames wherever S does
    not divide N: the stand-in with that bound misses the reference on every run with such a rank -- the
    (3, 7, 3, (70, 9)) row (S = 64 over 70 frames) and the (33, 2, 2, (130, 0, 7)) rows (S = 31 over 130) -- and on
    no other."""
    wrong = StandIn(slice_end=lambda sp, N, S: sp * N // S + N // S)
    failed = [run for run in refs.SYNC_RUNS if max(standin_errors(run, wrong).values()) > 1e-6]
    uneven = [run for run in refs.SYNC_RUNS if not all(r.even for r in refs.route(run.case) if r.N)]
    assert failed == uneven
    assert {run.case for run in failed} == {(3, 7, 3, (70, 9)), (33, 2, 2, (130, 0, 7))}


# ---------------------------------------------------------------------------------------------------------------
# 5. the fp32 CPU reference takes the float64 branches
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('run', [r for r in refs.SYNC_RUNS if r.act == refs.ACT_LRELU],
                         ids=[refs.run_id(r) for r in refs.SYNC_RUNS if r.act == refs.ACT_LRELU])
def test_fp32_reference_flips_no_branch_in_train_mode(run):
    ins = refs.run_inputs(run)
    z = [refs.split_reference(*ins, run.momentum, refs.EPS, run.act, run.case[3], dt, tracked=run.tracked)['z']
         for dt in (torch.float32, torch.float64)]
    assert torch.equal(z[0] > 0, z[1] > 0)


@pytest.mark.parametrize('case', refs.EVAL_CASES, ids=EVAL_IDS)
def test_fp32_reference_flips_no_branch_in_eval_mode(case):
    ins = refs.inputs(*case)
    z = [refs.eval_reference(*ins, refs.EPS, refs.ACT_LRELU, dt)['z'] for dt in (torch.float32, torch.float64)]
    assert torch.equal(z[0] > 0, z[1] > 0)
    if case == (200, 64, 8, 8):
        # one pre-activation at ~2e-8 of the maximum: a device tie there falls under the cap of lrelu_ties
        assert float(z[1].abs().min()) <= 2e-6 * float(z[1].abs().max())
