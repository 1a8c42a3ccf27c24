"""Host side of the column-matrix rung (tests/column_matrix_refs.py) WITHOUT a GPU.

1. ``bn_conv_ws_bytes`` of the three conv ops equals the restated ``bn_col_ws_bytes`` (+ the bias gradient's
   partial sums for the weight gradient) on every case of tests/test_gpu_column_matrix.py.  The split counts
   of all three products enter that number as ``slices * M * N * 4``, and the frames per pass as the sizes of
   the column and row matrices: a restatement that drifts from the C code fails here.
2. The case list reaches every (kernel, split?) pair ``bn_launch_gemm`` can take from this rung, and the
   tiled kernel's ragged tiles in all three dimensions -- so the device test's numbers cover them.
"""
import pytest

from behavenet_amd import _hip
from tests import column_matrix_refs as refs

IDS = [c[0] for c in refs.CASES]


@pytest.mark.parametrize('case', refs.CASES, ids=IDS)
@pytest.mark.parametrize('op', [_hip.OP_CONV_FWD, _hip.OP_CONV_BWD_D, _hip.OP_CONV_BWD_W])
def test_scratch_query_equals_the_restated_column_matrix_scratch(case, op):
    got = _hip.load().bn_conv_ws_bytes(op, *refs.conv_geom(case))
    assert got == refs.conv_ws_bytes(op, case), (case[0], op, got, refs.col_ws_bytes(case))


def test_bias_scratch_term_applies_to_the_two_long_cases_only():
    """The weight gradient's query asks for N * Cs * 4 bytes more (one partial sum per channel and frame)
    where the bias reduction is 8192 elements long and has more than one frame: the two multi-pass cases."""
    for case in refs.CASES:
        N, Cb, Cs, PQ, RS = refs.geom_of(case)
        extra = refs.conv_ws_bytes(3, case) - refs.col_ws_bytes(case)
        assert extra == (N * Cs * 4 if case[0] in refs.MULTI_PASS else 0), (case[0], extra)
    by_name = {c[0]: c for c in refs.CASES}
    assert refs.conv_ws_bytes(3, by_name['k1_c3_c5_300x300_n24']) - refs.col_ws_bytes(
        by_name['k1_c3_c5_300x300_n24']) == 480
    assert refs.conv_ws_bytes(3, by_name['k1_c3_c5_256x256_n33']) - refs.col_ws_bytes(
        by_name['k1_c3_c5_256x256_n33']) == 660


def test_passes_of_the_two_long_cases():
    by_name = {c[0]: c for c in refs.CASES}
    assert refs.passes(by_name['k1_c3_c5_300x300_n24']) == [23, 1]
    # exactly 2^21 rows in the first pass: k_gemm_mfma's grid is (1, 65536, z)
    assert refs.passes(by_name['k1_c3_c5_256x256_n33']) == [32, 1]
    M, N, K, strides = refs.roles(by_name['k1_c3_c5_256x256_n33'])[0]
    assert M == 1 << 21 and refs.gemm_grid(M, N, K, *strides)[:2] == (1, 65536)
    for case in refs.CASES:
        assert (len(refs.passes(case)) > 1) == (case[0] in refs.MULTI_PASS), case[0]


def _all_routes():
    """[(case name, role, pass, (M, N, K), kernel, slices)] of the case list, plus the one pair the named cases
    of tests/test_gpu_kernels.py already check (k7s2_same_24x20's weight gradient)."""
    from tests.test_gpu_kernels import CONV_CASES
    out = []
    k7 = [c for c in CONV_CASES if c[0] == 'k7s2_same_24x20']
    assert len(k7) == 1
    for case in list(refs.CASES) + k7:
        for i, nf in enumerate(refs.passes(case)):
            for role, (M, N, K, strides) in zip(refs.ROLES, refs.roles(case, nf)):
                if case[0] == 'k7s2_same_24x20' and role != 'wgrad':
                    continue            # (its other two roles run specialised kernels)
                kernel, slices = refs.gemm_route(M, N, K, *strides)
                out.append((case[0], role, i, (M, N, K), kernel, slices))
    return out


def test_case_list_reaches_every_kernel_and_split():
    seen = {(kernel, slices > 1) for _, _, _, _, kernel, slices in _all_routes()}
    want = {('k_gemm_mfma<1>', False), ('k_gemm_mfma<4>', False), ('k_gemm_mfma<8>', False),
            ('k_gemm_mfma<8>', True)}
    for t in ('k_gemm_tiled<0,0>', 'k_gemm_tiled<0,1>', 'k_gemm_tiled<1,1>'):
        want |= {(t, False), (t, True)}
    assert want <= seen, sorted(want - seen)
    # (no role sets A i-contiguous with B k-contiguous)
    assert not any(kernel == 'k_gemm_tiled<1,0>' for kernel, _ in seen)
    # the one pair left to the named cases really is what they run
    k7 = [r for r in _all_routes() if r[0] == 'k7s2_same_24x20']
    assert [(r[4], r[5]) for r in k7] == [('k_gemm_tiled<1,1>', 1)]


def test_case_list_reaches_the_tiled_kernels_ragged_tiles():
    tiled = [r for r in _all_routes() if r[4].startswith('k_gemm_tiled') and r[0] != 'k7s2_same_24x20']
    assert any(M % refs.GT_M for _, _, _, (M, N, K), _, _ in tiled)
    # a column tile that ends inside its first half (N % 128 < 64) and one inside its second (> 64)
    assert any(0 < N % refs.GT_N < 64 for _, _, _, (M, N, K), _, _ in tiled)
    assert any(N % refs.GT_N > 64 for _, _, _, (M, N, K), _, _ in tiled)
    assert any(K % refs.GT_K for _, _, _, (M, N, K), _, _ in tiled)
    # ... and a split whose last slice is shorter than the others
    assert any(s > 1 and K % (refs._cdiv(refs._cdiv(K, s), refs.GT_K) * refs.GT_K)
               for _, _, _, (M, N, K), _, s in tiled)


# the routes the case list was chosen for (first pass), checked so that a change of the split heuristics
# that empties a row of the table is seen here and not only as a weaker device test
TABLE = {
    's3_k3_c72_c72': (('k_gemm_tiled<0,0>', 5), ('k_gemm_mfma<8>', None), ('k_gemm_tiled<0,1>', None)),
    's3_k5_c64_c64': (('k_gemm_mfma<8>', None), ('k_gemm_tiled<1,1>', 6), ('k_gemm_tiled<0,1>', None)),
    's3_k3_c64_c128': (('k_gemm_tiled<0,0>', 4), ('k_gemm_tiled<1,1>', 6), ('k_gemm_tiled<0,1>', None)),
    'k1_c64_c64_32x32': (('k_gemm_tiled<0,0>', 1), ('k_gemm_mfma<8>', 8), ('k_gemm_tiled<0,1>', None)),
    'k1_c72_c136_33x31': (('k_gemm_tiled<0,0>', None), ('k_gemm_mfma<8>', None), ('k_gemm_tiled<0,1>', None)),
    'k1_c64_c512_32x32': (('k_gemm_tiled<0,0>', None), ('k_gemm_mfma<8>', 8), ('k_gemm_tiled<0,1>', 4)),
    's4_k5_c64_c64': (('k_gemm_mfma<8>', 12), ('k_gemm_tiled<1,1>', 4), ('k_gemm_tiled<0,1>', None)),
    's3_k3_c16_c32_n40': (('k_gemm_mfma<4>', None), ('k_gemm_mfma<8>', 16), ('k_gemm_mfma<1>', None)),
    's3_k5_c48_c24': (('k_gemm_mfma<8>', 9), (None, None), (None, None)),
}


@pytest.mark.parametrize('name', sorted(TABLE))
def test_routes_of_the_case_list(name):
    case = [c for c in refs.CASES if c[0] == name][0]
    got = refs.routes(case)
    for role, (kernel, slices) in zip(refs.ROLES, TABLE[name]):
        assert len(got[role]) == 1
        if kernel is not None:
            assert got[role][0][0] == kernel, (name, role, got[role])
        if slices is not None:
            assert got[role][0][1] == slices, (name, role, got[role])


def test_ragged_rows_of_the_table():
    by_name = {c[0]: c for c in refs.CASES}
    M, N, K, _ = refs.roles(by_name['s3_k3_c72_c72'])[0]
    assert (M % 64, N, K % 32) == (34, 72, 8)
    M, N, K, _ = refs.roles(by_name['k1_c72_c136_33x31'])[0]
    assert (M % 64, N, K) == (63, 136, 72)
    # the 2.07 M-row weight gradient in 128 slices
    M, N, K, strides = refs.roles(by_name['k1_c3_c5_300x300_n24'])[1]
    assert K == 23 * 300 * 300 and refs.gemm_route(M, N, K, *strides) == ('k_gemm_mfma<8>', 128)
