"""The nn.Linear job kernel (``k_linear_jobs`` + ``k_gemm_combine``, csrc/gemm.hip, behind ``bn_linear_fwd`` /
``bn_linear_bwd``) against float64 on the MI355X, on the case list of tests/linear_refs.py --
tests/test_linear_routes_host.py asserts, without a GPU, which path of the kernel each case runs.

Every output is compared with the fp32 CPU result and with a float64 evaluation of the same expression, by
``tests.test_gpu_kernels.close`` as it stands: the error against float64 is at most 1e-4 of the result's maximum
and at most max(8 x the fp32 CPU error, 3e-6); the column sums ``db`` pass their terms as ``sum_of``.

Figures measured on the MI355X (largest over all cases; e_hip / e_cpu = max error against float64 over the
result's maximum, of the device and of the fp32 CPU result):

    output          e_hip      e_cpu      case of the largest e_hip
    fwd             1.5e-7     5.8e-7     (5, 32768, 12)
    fwd nobias      2.6e-7     1.4e-6     (5, 32768, 12)
    dx              2.1e-7     3.8e-7     (200, 2048, 64)
    dx*lrelu'       2.1e-7     3.8e-7     (200, 2048, 64)
    dx*sigmoid'     1.9e-7     3.9e-7     (5, 37, 65)
    dw              2.3e-7     3.7e-7     (200, 2048, 12)
    dw, no dx       5.2e-7     3.3e-7     (1024, 1024, 12), the 1024-deep weight gradient in one slice
    db              3.1e-7     1.3e-7     (1024, 1024, 12)
    dw accumulated  2.2e-7     3.3e-7     (70, 100, 12)
    db accumulated  3.1e-7     1.0e-7     (1024, 1024, 12)

so the 3e-6 floor of ``close`` governs every check, with 5.8x room at the least (dw without a data gradient).
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from behavenet_amd import _hip
from tests import linear_refs as refs
from tests.measured import measured_close
from tests.test_gpu_kernels import act_ref, SLOPE
from tests.test_gpu_guard_bands import guarded, finite, _bands_stay_untouched  # noqa: F401 (autouse fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
IDS = ['%dx%dx%d' % c for c in refs.CASES]
SIGMOID_CASES = [(5, 16, 1024), (5, 37, 65)]            # the split data gradient, and everything odd
GUARD_CASES = [(1024, 1024, 12), (5, 16, 1024), (33, 1030, 8), (5, 32768, 12), (5, 8200, 12)]


@functools.lru_cache(maxsize=None)
def reference(case, act=_hip.ACT_LRELU):
    """Inputs and the fp32 / float64 CPU results of a case, computed once and shared (nobody writes to them).
    ``xin`` = act(pre) plays the role of the post-activation output of the layer below: it is the layer's input,
    and ``dpre`` = dxin * act'(xin) is what the fused epilogue hands down."""
    M, K, N = case
    g = torch.Generator().manual_seed(M + K + N)
    pre0 = torch.rand((M, K), generator=g) - 0.4
    w0 = (torch.rand((N, K), generator=g) - 0.5) / np.sqrt(K)
    b0 = torch.rand((N,), generator=g) - 0.5
    dy = torch.rand((M, N), generator=g) - 0.5
    out = {'w': w0, 'b': b0, 'dy': dy}
    for key, dt in (('f32', torch.float32), ('f64', torch.float64)):
        pre, w, b = (t.detach().clone().to(dt).requires_grad_(True) for t in (pre0, w0, b0))
        xin = act_ref(pre, act)
        xin.retain_grad()
        y = F.linear(xin, w, b)
        y.backward(dy.to(dt))
        out[key] = {'y': y.detach(), 'y_nobias': F.linear(xin, w).detach(), 'dxin': xin.grad, 'dpre': pre.grad,
                    'dw': w.grad, 'db': b.grad}
        if dt == torch.float32:
            out['xin'] = xin.detach()
    return out


def device_inputs(ref):
    return tuple(ref[k].to(DEV).contiguous() for k in ('xin', 'w', 'b', 'dy'))


@pytest.mark.parametrize('case', refs.CASES, ids=IDS)
def test_every_output_against_float64(case):
    M, K, N = case
    ref = reference(case)
    r32, r64 = ref['f32'], ref['f64']
    xd, wd, bd, dyd = device_inputs(ref)
    tag = '%dx%dx%d ' % case
    measured_close(_hip.linear_fwd(xd, wd, bd), r32['y'], r64['y'], tag + 'fwd')
    measured_close(_hip.linear_fwd(xd, wd, None), r32['y_nobias'], r64['y_nobias'], tag + 'fwd nobias')
    dw = torch.full((N, K), 7.0, device=DEV)
    db = torch.full((N,), 7.0, device=DEV)
    dx = _hip.linear_bwd(xd, wd, dyd, True, None, _hip.ACT_NONE, 0.0, dw, db, False)
    measured_close(dx, r32['dxin'], r64['dxin'], tag + 'dx')
    measured_close(dw, r32['dw'], r64['dw'], tag + 'dw')
    measured_close(db, r32['db'], r64['db'], tag + 'db', sum_of=ref['dy'])
    # the fused epilogue dx * lrelu'(input), next to the other two jobs again: they do not change
    dw2 = torch.full((N, K), -3.0, device=DEV)
    db2 = torch.full((N,), -3.0, device=DEV)
    dx = _hip.linear_bwd(xd, wd, dyd, True, xd, _hip.ACT_LRELU, SLOPE, dw2, db2, False)
    measured_close(dx, r32['dpre'], r64['dpre'], tag + "dx*lrelu'")
    assert torch.equal(dw2, dw) and torch.equal(db2, db)


@pytest.mark.parametrize('case', SIGMOID_CASES, ids=['%dx%dx%d' % c for c in SIGMOID_CASES])
def test_sigmoid_epilogue_against_float64(case):
    ref = reference(case, _hip.ACT_SIGMOID)
    xd, wd, bd, dyd = device_inputs(ref)
    dx = _hip.linear_bwd(xd, wd, dyd, True, xd, _hip.ACT_SIGMOID, SLOPE, None, None, False)
    measured_close(dx, ref['f32']['dpre'], ref['f64']['dpre'], "%dx%dx%d dx*sigmoid'" % case)
    measured_close(_hip.linear_fwd(xd, wd, bd), ref['f32']['y'], ref['f64']['y'], '%dx%dx%d fwd (sigmoid input)' % case)


@pytest.mark.parametrize('case', [(70, 100, 12), (1024, 1024, 12)], ids=['unsplit', 'split_dw'])
def test_accumulate_onto_prefilled_dw_and_db(case):
    """Two calls with ``accumulate`` onto a prefill leave prefill + 2 x gradient, in ``dw`` (through
    k_gemm_combine where the weight gradient is split) and in ``db``."""
    M, K, N = case
    assert (refs.routes(*case)['dw'].slices > 1) == (case == (1024, 1024, 12))
    ref = reference(case)
    xd, wd, bd, dyd = device_inputs(ref)
    g = torch.Generator().manual_seed(11)
    pw, pb = torch.rand((N, K), generator=g) - 0.5, torch.rand((N,), generator=g) - 0.5
    dw, db = pw.to(DEV), pb.to(DEV)
    for _ in range(2):
        _hip.linear_bwd(xd, wd, dyd, True, None, _hip.ACT_NONE, 0.0, dw, db, True)
    r32, r64 = ref['f32'], ref['f64']
    tag = '%dx%dx%d ' % case
    measured_close(dw, pw + 2 * r32['dw'], pw.double() + 2 * r64['dw'], tag + 'dw acc')
    # the terms of db: the prefill and every row of dy twice
    terms = torch.cat([pb[None, :], ref['dy'], ref['dy']], dim=0)
    measured_close(db, pb + 2 * r32['db'], pb.double() + 2 * r64['db'], tag + 'db acc', sum_of=terms)


@pytest.mark.parametrize('case', [(70, 100, 12), (1024, 1024, 12), (5, 16, 1024)],
                         ids=['unsplit', 'split_dw', 'split_dx'])
def test_each_output_alone_left_out(case):
    M, K, N = case
    ref = reference(case)
    r32, r64 = ref['f32'], ref['f64']
    xd, wd, bd, dyd = device_inputs(ref)
    tag = '%dx%dx%d ' % case
    # no data gradient (the first layer of a network): the wrapper passes no scratch, dW runs unsplit
    dw, db = torch.full((N, K), 7.0, device=DEV), torch.full((N,), 7.0, device=DEV)
    assert _hip.linear_bwd(xd, wd, dyd, False, None, _hip.ACT_NONE, 0.0, dw, db, False) is None
    measured_close(dw, r32['dw'], r64['dw'], tag + 'dw (no dx)')
    measured_close(db, r32['db'], r64['db'], tag + 'db (no dx)', sum_of=ref['dy'])
    # no weight gradient
    db = torch.full((N,), 7.0, device=DEV)
    dx = _hip.linear_bwd(xd, wd, dyd, True, xd, _hip.ACT_LRELU, SLOPE, None, db, False)
    measured_close(dx, r32['dpre'], r64['dpre'], tag + "dx*lrelu' (no dw)")
    measured_close(db, r32['db'], r64['db'], tag + 'db (no dw)', sum_of=ref['dy'])
    # no bias gradient
    dw = torch.full((N, K), 7.0, device=DEV)
    dx = _hip.linear_bwd(xd, wd, dyd, True, None, _hip.ACT_NONE, 0.0, dw, None, False)
    measured_close(dx, r32['dxin'], r64['dxin'], tag + 'dx (no db)')
    measured_close(dw, r32['dw'], r64['dw'], tag + 'dw (no db)')


def _all_outputs(xd, wd, bd, dyd):
    N, K = wd.shape
    y = _hip.linear_fwd(xd, wd, bd)
    dw, db = torch.empty((N, K), device=DEV), torch.empty((N,), device=DEV)
    dx = _hip.linear_bwd(xd, wd, dyd, True, xd, _hip.ACT_LRELU, SLOPE, dw, db, False)
    return y, dx, dw, db


@pytest.mark.parametrize('case', refs.SPLIT_CASES, ids=['%dx%dx%d' % c for c in refs.SPLIT_CASES])
def test_split_reductions_repeat_bit_for_bit(case):
    """The split reductions are combined in a fixed order: the same call gives the same bits, also after another
    layer's partial tiles went through the arena in between."""
    other = (256, 12, 2048) if case != (256, 12, 2048) else (200, 2048, 12)
    assert refs.has_split(*case) and refs.has_split(*other)
    ins, ins_other = device_inputs(reference(case)), device_inputs(reference(other))
    first = _all_outputs(*ins)
    _all_outputs(*ins_other)
    second = _all_outputs(*ins)
    for name, a, b in zip(('y', 'dx', 'dw', 'db'), first, second):
        assert torch.equal(a, b), '%s of %s: %d elements differ' % (name, case, int((a != b).sum()))


@pytest.mark.parametrize('case', GUARD_CASES, ids=['%dx%dx%d' % c for c in GUARD_CASES])
def test_c_abi_under_guard_bands_with_a_nan_filled_scratch(case):
    """bn_linear_fwd / bn_linear_bwd through the C ABI: every operand and output between NaN guard bands, the
    scratch of exactly bn_linear_ws_bytes bytes, NaN-filled and guarded too -- k_gemm_combine reads
    slices x M x N partial values, so a partial tile that no wave wrote (an empty share, a slice past K) or one
    read past the scratch comes out as NaN.  Results: finite and the bits of the _hip wrapper's."""
    M, K, N = case
    assert case in refs.SPLIT_CASES
    lib = _hip.load()
    nbytes = lib.bn_linear_ws_bytes(M, K, N)
    assert nbytes == refs.linear_ws_bytes(M, K, N) and nbytes > 0 and nbytes % 4 == 0
    ref = reference(case)
    plain = device_inputs(ref)
    want = _all_outputs(*plain)
    xd, wd, bd, dyd = (guarded(t) for t in plain)
    y, dx = guarded(torch.full((M, N), float('nan'))), guarded(torch.full((M, K), float('nan')))
    dw, db = guarded(torch.full((N, K), float('nan'))), guarded(torch.full((N,), float('nan')))
    ws = guarded(torch.full((nbytes // 4,), float('nan')))
    p, st = _hip._ptr, _hip._stream()
    _hip._check(lib.bn_linear_fwd(p(xd, 'x'), p(wd, 'w'), p(bd, 'b'), p(y, 'y'), M, K, N, p(ws, 'ws'), nbytes,
                                  st), 'bn_linear_fwd')
    ws.fill_(float('nan'))
    _hip._check(lib.bn_linear_bwd(p(xd, 'x'), p(wd, 'w'), p(dyd, 'dy'), p(dx, 'dx'), p(xd, 'dact_src'),
                                  _hip.ACT_LRELU, SLOPE, p(dw, 'dw'), p(db, 'db'), 0, M, K, N, p(ws, 'ws'),
                                  nbytes, st), 'bn_linear_bwd')
    for name, got, w in zip(('y', 'dx', 'dw', 'db'), (y, dx, dw, db), want):
        finite(got, '%s of %s' % (name, case))
        assert torch.equal(got, w), '%s of %s: %d elements differ from the wrapper\'s' % (
            name, case, int((got != w).sum()))
