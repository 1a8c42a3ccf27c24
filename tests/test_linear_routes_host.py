"""Host side of the nn.Linear job kernel (tests/linear_refs.py) WITHOUT a GPU.

1. ``bn_linear_ws_bytes`` equals the restated scratch on every case of tests/test_gpu_linear.py (and on a sweep of
   other shapes): the split counts enter that number as ``slices * M * N * 4``, so a restatement that drifts from
   gemm.hip's split heuristics fails here.
2. The case list reaches every path of ``k_linear_jobs`` / ``gemm_tile`` / ``k_gemm_combine`` that the device test
   is there for.  A routing change in gemm.hip that moves a case fails THIS file instead of silently emptying a row
   of the device test.
"""
import pytest

from behavenet_amd import _hip
from tests import linear_refs as refs

IDS = ['%dx%dx%d' % c for c in refs.CASES]


@pytest.mark.parametrize('case', refs.CASES, ids=IDS)
def test_scratch_query_equals_the_restated_scratch(case):
    assert _hip.load().bn_linear_ws_bytes(*case) == refs.linear_ws_bytes(*case)


def test_scratch_query_equals_the_restated_scratch_on_a_sweep():
    lib = _hip.load()
    for M in (1, 5, 33, 200, 256, 1024, 1500):
        for K in (1, 12, 64, 100, 1023, 1024, 1030, 2048, 8200, 32768):
            for N in (1, 8, 12, 64, 65, 1024, 2048):
                assert lib.bn_linear_ws_bytes(M, K, N) == refs.linear_ws_bytes(M, K, N), (M, K, N)
    assert lib.bn_linear_ws_bytes(0, 12, 12) == 0 == refs.linear_ws_bytes(0, 12, 12)


def test_no_case_exceeds_about_8_mb_of_operands():
    for case in refs.CASES:
        assert refs.operand_bytes(*case) <= 9e6, case


def _all_jobs():
    return [(case, name, job) for case in refs.CASES for name, job in refs.routes(*case).items()]


def test_case_list_reaches_every_path_of_the_job_kernel():
    jobs = _all_jobs()
    # waves per unit, and the three load loops of gemm_tile
    assert {j.nw for _, _, j in jobs} == {1, 2, 4}
    assert {j.load for _, _, j in jobs} == {'vec', 'veca', 'scalar'}
    # a split forward, data gradient and weight gradient
    for name in refs.JOBS:
        assert any(n == name and j.slices > 1 for _, n, j in jobs), name
    # k_gemm_combine: more than one trip of 16 partial tiles, and a ragged last trip never (slices are
    # powers of two there), so only the count is asked for
    assert any(j.slices > refs.COMBINE_TRIP for _, _, j in jobs)
    # a slice that begins past K, a wave with an empty share in the last slice that has one
    assert any(j.slices_past_end for _, _, j in jobs)
    assert any(j.empty_waves for _, _, j in jobs)
    # the `live = false` branch, alone in its wave (nw = 1) and as a pair of waves behind a barrier (nw = 2)
    for nw in (1, 2):
        assert any(j.nw == nw and j.dead_groups for _, _, j in jobs), nw
    # (four waves share a unit at nw = 4: a workgroup holds one unit and none is ever spare)
    assert not any(j.nw == 4 and j.dead_groups for _, _, j in jobs)


def test_case_list_reaches_the_column_sum_jobs_edges():
    sums = [refs.column_sum_job(M, N) for M, K, N in refs.CASES]
    assert any(cols < refs.DB_COLS for _, cols, _ in sums)            # N not a multiple of 64
    assert any(blocks > 1 for blocks, _, _ in sums)                   # N above 64: two column blocks
    assert any(blocks > 1 and cols < refs.DB_COLS for blocks, cols, _ in sums)
    assert any(rows < refs.DB_ROWS for _, _, rows in sums)            # M not a multiple of 64
    assert any(M > refs.DB_ROWS for M, K, N in refs.CASES)            # more than one trip over the rows


# what each case was chosen for: {case: {job: (slices, kslice, nw, units, blocks, dead, past, empty, load)}}
TABLE = {
    (200, 2048, 12): {'fwd': (16, 128, 4, 112, 112, 0, 0, 0, 'vec'), 'dx': (1, 16, 1, 448, 112, 0, 0, 0, 'veca'),
                      'dw': (1, 208, 4, 64, 64, 0, 0, 0, 'scalar')},
    (200, 2048, 64): {'fwd': (16, 128, 4, 224, 224, 0, 0, 0, 'vec'), 'dx': (1, 64, 2, 448, 224, 0, 0, 0, 'veca'),
                      'dw': (1, 208, 4, 128, 128, 0, 0, 0, 'scalar')},
    (256, 12, 2048): {'fwd': (1, 16, 1, 512, 128, 0, 0, 0, 'vec'), 'dx': (16, 128, 4, 128, 128, 0, 0, 0, 'veca'),
                      'dw': (1, 256, 4, 64, 64, 0, 0, 0, 'scalar')},
    (70, 100, 12): {'fwd': (1, 112, 2, 3, 2, 1, 0, 0, 'vec'), 'dx': (1, 16, 1, 12, 3, 0, 0, 0, 'veca'),
                    'dw': (1, 80, 2, 4, 2, 0, 0, 0, 'scalar')},
    (70, 40, 12): {'fwd': (1, 48, 1, 3, 1, 1, 0, 0, 'vec'), 'dx': (1, 16, 1, 6, 2, 2, 0, 0, 'veca'),
                   'dw': (1, 80, 2, 2, 1, 0, 0, 0, 'scalar')},
    (5, 8200, 12): {'fwd': (32, 272, 4, 32, 32, 0, 1, 1, 'vec'), 'dx': (1, 16, 1, 257, 65, 3, 0, 0, 'veca'),
                    'dw': (1, 16, 1, 257, 65, 3, 0, 0, 'scalar')},
    (5, 32768, 12): {'fwd': (128, 256, 4, 128, 128, 0, 0, 0, 'vec'), 'dx': (1, 16, 1, 1024, 256, 0, 0, 0, 'veca'),
                     'dw': (1, 16, 1, 1024, 256, 0, 0, 0, 'scalar')},
    (1024, 1024, 12): {'fwd': (8, 128, 4, 256, 256, 0, 0, 0, 'vec'), 'dx': (1, 16, 1, 1024, 256, 0, 0, 0, 'veca'),
                       'dw': (8, 128, 4, 256, 256, 0, 0, 0, 'scalar')},
    (5, 16, 1024): {'fwd': (1, 16, 1, 32, 8, 0, 0, 0, 'vec'), 'dx': (8, 128, 4, 8, 8, 0, 0, 0, 'veca'),
                    'dw': (1, 16, 1, 32, 8, 0, 0, 0, 'scalar')},
    (33, 1030, 8): {'fwd': (8, 144, 4, 16, 16, 0, 0, 1, 'scalar'), 'dx': (1, 16, 1, 66, 17, 2, 0, 0, 'veca'),
                    'dw': (1, 48, 1, 33, 9, 3, 0, 0, 'scalar')},
    (5, 37, 65): {'fwd': (1, 48, 1, 3, 1, 1, 0, 0, 'scalar'), 'dx': (1, 80, 2, 2, 1, 0, 0, 0, 'scalar'),
                  'dw': (1, 16, 1, 6, 2, 2, 0, 0, 'scalar')},
}


@pytest.mark.parametrize('case', refs.CASES, ids=IDS)
def test_routes_of_the_case_list(case):
    got = refs.routes(*case)
    assert sorted(got) == sorted(refs.JOBS)
    for name, want in TABLE[case].items():
        j = got[name]
        assert (j.slices, j.kslice, j.nw, j.units, j.blocks, j.dead_groups, j.slices_past_end, j.empty_waves,
                j.load) == want, (case, name, j)
        # every wave with a share runs the same loop in these cases: the figure above is the job's
        assert j.loads == {j.load}, (case, name, j.loads)


def test_table_covers_the_case_list():
    assert sorted(TABLE) == sorted(refs.CASES)
    assert len(set(refs.CASES)) == len(refs.CASES)


def test_shares_of_the_ragged_slices():
    """The three reductions the list has for their last slices, spelled out."""
    # K = 8200 in 32 slices of 272: slice 30 holds 40 elements in shares of 16 (wave 3 has none), slice 31 begins
    # at 8432 and all four of its waves must still write zero partial tiles
    j = refs.routes(5, 8200, 12)['fwd']
    assert [refs.wave_share(j.K, j.kslice, j.nw, 30, w) for w in range(4)] == [
        (8160, 8176), (8176, 8192), (8192, 8200), (8208, 8200)]
    assert all(e <= b for b, e in (refs.wave_share(j.K, j.kslice, j.nw, 31, w) for w in range(4)))
    # K = 1030 in 8 slices of 144: the last one holds 22 elements in shares of 8
    j = refs.routes(33, 1030, 8)['fwd']
    assert [refs.wave_share(j.K, j.kslice, j.nw, 7, w) for w in range(4)] == [
        (1008, 1016), (1016, 1024), (1024, 1030), (1032, 1030)]
    # K = 32768: eight full trips of the combine
    j = refs.routes(5, 32768, 12)['fwd']
    assert j.slices == 8 * refs.COMBINE_TRIP and j.slices * j.kslice == j.K


def test_scratch_goes_to_the_data_gradient_first():
    """bn_launch_linear_jobs: dx takes its partial tiles from the front of the scratch, dW from what is left, and
    a product whose need does not fit runs unsplit."""
    # the forward's 8 x 1024 x 12 floats are exactly what the weight gradient's 8 slices need; dx does not split
    r = refs.routes(1024, 1024, 12)
    assert refs.linear_ws_bytes(1024, 1024, 12) == r['fwd'].ws_bytes == r['dw'].ws_bytes == 393216
    assert r['dx'].ws_bytes == 0
    # without a data gradient the wrapper passes no scratch, and the weight gradient runs in one slice
    assert refs.routes(1024, 1024, 12, need_dx=False)['dw'].slices == 1
    # dx split: its need is the whole scratch
    r = refs.routes(5, 16, 1024)
    assert r['dx'].ws_bytes == refs.linear_ws_bytes(5, 16, 1024) == 2560
    # a layer where dx and dW would both split and only dx fits: the restatement must leave dW unsplit
    M, K, N = 1024, 12, 1024
    ops = refs.operands(M, K, N)
    assert refs.jobs_ws_bytes(*ops['dx'][:3]) > 0 and refs.jobs_ws_bytes(*ops['dw'][:3]) > 0
    r = refs.routes(M, K, N)
    assert r['dx'].slices > 1 and r['dw'].slices == 1
    assert refs.linear_ws_bytes(M, K, N) < r['dx'].ws_bytes + refs.jobs_ws_bytes(*ops['dw'][:3])


def test_split_cases():
    assert refs.SPLIT_CASES == [c for c in refs.CASES if c not in ((70, 100, 12), (70, 40, 12), (5, 37, 65))]
