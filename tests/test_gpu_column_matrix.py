"""The column-matrix rung of the convolution ladder (k_im2col / k_nchw_to_rows / k_col2im + one GEMM through
bn_launch_gemm, csrc/conv_pad.hip and csrc/gemm.hip) against float64 -- the rung every convolution ends on
that the specialised kernels do not take: strides other than 1, 2 and the kernel size, 1x1 kernels, odd
channel counts.

The cases (tests/column_matrix_refs.CASES) are chosen by the GEMM they make: tests/test_column_matrix_host.py
asserts, without a GPU, that they reach k_gemm_mfma<1>, <4>, <8> and k_gemm_tiled<0,0>, <0,1>, <1,1> with and
without a split of the reduction, the tiled kernel's ragged tiles in M, N and K, and the pass loop of
bn_launch_col_* (two cases of two passes, one of them with exactly 2^21 rows = grid.y 65536 in its first).
Here:

* numbers: the checks of tests/test_gpu_kernels.py (forward, both data-gradient forms, dW, db, the accumulating
  call; error against float64 <= 1e-4 of the result's maximum and <= max(8 x the CPU fp32 error, 3e-6)) on
  every case and on the transposed layer between the same maps (k_col2im with bias and activation);
* the rung: the profiling hook must name the column-matrix kernels for all three roles of every case -- a
  dispatch change that moves a case elsewhere fails here instead of silently emptying this file;
* bit repeat: every role whose reduction is split gives the same bits twice (fixed-order combination);
* guard bands: the two cases with ragged tiles in all of M, N and K, called through the C ABI with every
  operand, every output and a NaN-filled scratch of exactly the queried size between NaN bands (the tiled
  kernel fetches 8 floats per thread: a ragged edge is where it would over-read);
* the 17 geometries of tests/ladder_cases.LADDER_EXTRA, whose kernel NAMES test_dispatch_ladder_is_pinned
  pins, get their numbers checked.

k_gemm_tiled<1,0> has no caller (no role has A i-contiguous with B k-contiguous) and no test.
"""
import pytest
import torch

from behavenet_amd import _hip
from tests import column_matrix_refs as refs
from tests.ladder_cases import LADDER_EXTRA, kernel_names
from tests.test_gpu_guard_bands import guarded, finite, _bands_stay_untouched  # noqa: F401
from tests.test_gpu_kernels import DEV, SLOPE, _conv_setup, _convT_setup, close  # noqa: F401
from tests.test_gpu_kernels import test_conv2d_fwd as check_conv2d_fwd, test_conv2d_bwd as check_conv2d_bwd
from tests.test_gpu_kernels import test_convT2d_fwd as check_convT2d_fwd, test_convT2d_bwd as check_convT2d_bwd

pytestmark = pytest.mark.gpu

CASES = refs.CASES
IDS = [c[0] for c in CASES]
T_CASES = [refs.transposed(c) for c in CASES]
T_IDS = [c[0] for c in T_CASES]


@pytest.mark.parametrize('case', CASES, ids=IDS)
@pytest.mark.parametrize('act', [_hip.ACT_LRELU, _hip.ACT_NONE])
def test_conv_forward(case, act):
    check_conv2d_fwd(case, act)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_conv_backward(case):
    check_conv2d_bwd(case)


@pytest.mark.parametrize('case', T_CASES, ids=T_IDS)
@pytest.mark.parametrize('act', [_hip.ACT_LRELU, _hip.ACT_SIGMOID])
def test_transposed_forward(case, act):
    check_convT2d_fwd(case, act)


@pytest.mark.parametrize('case', T_CASES, ids=T_IDS)
def test_transposed_backward(case):
    check_convT2d_bwd(case)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_cases_run_on_the_column_matrix_rung(case):
    assert kernel_names(case) == refs.RUNG_NAMES


# ------------------------------------------------------------------------------------------------------
# bit repeat of the split reductions
# ------------------------------------------------------------------------------------------------------
SPLIT = [(c, role) for c in CASES for role in refs.ROLES if any(s > 1 for _, s in refs.routes(c)[role])]


def _run_role(role, x, w, b, dy, geom):
    if role == 'down':
        return _hip.conv2d_fwd(x, w, b, geom, _hip.ACT_LRELU, SLOPE)
    if role == 'up':
        return _hip.conv2d_bwd_data(dy, w, geom, x, _hip.ACT_LRELU, SLOPE)
    dw, db = torch.full_like(w, 0.25), torch.full_like(b, 0.25)
    _hip.conv2d_bwd_weight(x, dy, dw, db, geom, True)
    return dw


@pytest.mark.parametrize('case,role', SPLIT, ids=['%s-%s' % (c[0], r) for c, r in SPLIT])
def test_split_reductions_repeat_their_bits(case, role):
    x, w, b, geom, _ = _conv_setup(case, seed=3)
    N, C, H, W, K, R, S, st, pt, pl, P, Q = geom
    dy = torch.rand((N, K, P, Q), generator=torch.Generator().manual_seed(4)) - 0.5
    x, w, b, dy = (t.to(DEV) for t in (x, w, b, dy))
    first = _run_role(role, x, w, b, dy, geom)
    # (other scratch contents in between: the partial tiles must all be rewritten, not merely left over)
    _hip.conv2d_fwd(x, w, b, geom, _hip.ACT_NONE, SLOPE)
    second = _run_role(role, x, w, b, dy, geom)
    assert torch.equal(first, second), (case[0], role, float((first - second).abs().max()))


def test_every_split_kernel_has_a_repeat_case():
    kernels = {k for c, role in SPLIT for k, s in refs.routes(c)[role] if s > 1}
    assert kernels == {'k_gemm_mfma<8>', 'k_gemm_tiled<0,0>', 'k_gemm_tiled<0,1>', 'k_gemm_tiled<1,1>'}


# ------------------------------------------------------------------------------------------------------
# guard bands: operands, outputs and the scratch
# ------------------------------------------------------------------------------------------------------
def _scratch(op, geom):
    nbytes = _hip.load().bn_conv_ws_bytes(op, *geom)
    assert nbytes > 0 and nbytes % 4 == 0
    ws = guarded(torch.full((nbytes // 4,), float('nan')))
    assert ws.data_ptr() % 16 == 0
    return ws.data_ptr(), nbytes


@pytest.mark.parametrize('name', ['s3_k3_c72_c72', 'k1_c72_c136_33x31'])
def test_ragged_tiles_stay_inside_their_operands(name):
    case = [c for c in CASES if c[0] == name][0]
    # (both run the tiled kernel with M % 64, N % 128 and K % 32 all non-zero)
    for role in ('down', 'up'):
        (kernel, _), = refs.routes(case)[role]
        assert kernel.startswith('k_gemm_tiled'), (name, role, kernel)
    lib, stream = _hip.load(), torch.cuda.current_stream().cuda_stream
    x0, w0, b0, geom, _ = _conv_setup(case, seed=2)
    N, C, H, W, K, R, S, st, pt, pl, P, Q = geom
    dy0 = torch.rand((N, K, P, Q), generator=torch.Generator().manual_seed(6)) - 0.5
    x, w, b, dy = guarded(x0), guarded(w0), guarded(b0), guarded(dy0)

    y = guarded(torch.zeros(N, K, P, Q))
    ws, nb = _scratch(_hip.OP_CONV_FWD, geom)
    assert lib.bn_conv2d_fwd(x.data_ptr(), w.data_ptr(), None, b.data_ptr(), y.data_ptr(), *geom, _hip.ACT_LRELU,
                             SLOPE, ws, nb, stream) == 0
    finite(y, name + ' fwd')
    assert torch.equal(y, _hip.conv2d_fwd(x, w, b, geom, _hip.ACT_LRELU, SLOPE))

    for src, dact in ((None, _hip.ACT_NONE), (x, _hip.ACT_LRELU)):
        dx = guarded(torch.zeros(N, C, H, W))
        ws, nb = _scratch(_hip.OP_CONV_BWD_D, geom)
        assert lib.bn_conv2d_bwd_data(dy.data_ptr(), w.data_ptr(), None, dx.data_ptr(),
                                      src.data_ptr() if src is not None else None, *geom, dact, SLOPE, ws, nb,
                                      stream) == 0
        finite(dx, name + ' bwd-data')
        assert torch.equal(dx, _hip.conv2d_bwd_data(dy, w, geom, src, dact, SLOPE))

    dw, db = guarded(torch.zeros(K, C, R, S)), guarded(torch.zeros(K))
    want_dw, want_db = torch.zeros(K, C, R, S, device=DEV), torch.zeros(K, device=DEV)
    for accumulate in (False, True):
        ws, nb = _scratch(_hip.OP_CONV_BWD_W, geom)
        assert lib.bn_conv2d_bwd_weight(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), db.data_ptr(), *geom,
                                        int(accumulate), ws, nb, stream) == 0
        finite(dw, name + ' dw')
        finite(db, name + ' db')
        _hip.conv2d_bwd_weight(x, dy, want_dw, want_db, geom, accumulate)
        assert torch.equal(dw, want_dw) and torch.equal(db, want_db)


# ------------------------------------------------------------------------------------------------------
# the rungs nobody asks for by name
# ------------------------------------------------------------------------------------------------------
EXTRA_IDS = [c[0] for c in LADDER_EXTRA]


@pytest.mark.parametrize('case', LADDER_EXTRA, ids=EXTRA_IDS)
def test_ladder_extra_forward(case):
    check_conv2d_fwd(case, _hip.ACT_LRELU)


@pytest.mark.parametrize('case', LADDER_EXTRA, ids=EXTRA_IDS)
def test_ladder_extra_backward(case):
    check_conv2d_bwd(case)
