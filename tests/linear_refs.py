"""The nn.Linear job kernel, restated in plain Python: how ``bn_linear_fwd`` / ``bn_linear_bwd`` (csrc/capi.hip)
set the operands of their products, how ``gemm_job`` (csrc/gemm.hip) cuts a product into units for
``k_linear_jobs``, how ``gemm_tile`` deals a unit's reduction to its waves and which of its three load loops a
wave runs, and how ``bn_launch_linear_jobs`` hands the scratch to the data gradient first and the weight gradient
second.

Nothing here calls the library: tests/test_linear_routes_host.py holds the restatement against
``bn_linear_ws_bytes`` and asserts that the case list reaches every path of the kernel, and
tests/test_gpu_linear.py runs the same list on the device.  ``gemm_slices`` and ``gemm_ws_bytes`` are the ones of
tests/column_matrix_refs.py (one restatement of gemm.hip's split heuristics, not two).
"""
import collections

from tests.column_matrix_refs import gemm_slices, gemm_ws_bytes, _cdiv

GJ_WAVES = 4                                # waves of a k_linear_jobs workgroup
COMBINE_TRIP = 16                           # partial tiles k_gemm_combine has in flight per trip
DB_COLS = 64                                # columns per workgroup of the column-sum job
DB_ROWS = 16 * GJ_WAVES                     # rows per trip of the column-sum job

# (M, K, N) of y (M x N) = x (M x K) w^T (N x K): the issue's list, in its order
CASES = [
    (200, 2048, 12),        # the default architecture's latent layer
    (200, 2048, 64),        # the widest latent layer; dx at nw = 2
    (256, 12, 2048),        # the decoder's first layer
    (70, 100, 12),          # forward nw = 2, 3 units: one dead pair of waves
    (70, 40, 12),           # forward nw = 1; dx with 6 units, 2 dead waves
    (5, 8200, 12),          # 32 slices, the last one begins past K
    (5, 32768, 12),         # 128 slices
    (1024, 1024, 12),       # forward split and dW split
    (5, 16, 1024),          # dx split
    (33, 1030, 8),          # K % 4 != 0: scalar forward loads; 8 slices, wave 3 empty in the last one
    (5, 37, 65),            # everything odd; two column blocks in the db job
]
JOBS = ('fwd', 'dx', 'dw')

Job = collections.namedtuple('Job', [
    'M', 'N', 'K',          # of the product C (M x N) = A (M x K) B (K x N)
    'slices', 'kslice', 'nw', 'tiles', 'units', 'upb', 'blocks',
    'dead_groups',          # wave groups of the last workgroup past the last unit (the `live = false` branch)
    'slices_past_end',      # slices that begin at or past K: all their waves write zero partial tiles
    'empty_waves',          # waves with an empty share in the last non-empty slice
    'load',                 # the load loop of wave 0 of slice 0: 'vec', 'veca' or 'scalar'
    'loads',                # the loops of all waves with a share
    'ws_bytes',             # of its partial tiles (0 if it runs unsplit)
])


def operands(M, K, N):
    """{job: (Mj, Nj, Kj, (sai, sak, sbk, sbj))} as bn_linear_fwd / bn_linear_bwd fill GemmArgs."""
    return {'fwd': (M, N, K, (K, 1, 1, K)),         # y[m, n] = sum_k x[m, k] w[n, k]
            'dx': (M, K, N, (N, 1, K, 1)),          # dx[m, k] = sum_n dy[m, n] w[n, k]
            'dw': (N, K, M, (1, N, K, 1))}          # dw[n, k] = sum_m dy[m, n] x[m, k]


def jobs_ws_bytes(M, N, K):
    """bn_linear_jobs_ws_bytes of one product."""
    s = gemm_slices(M, N, K)
    return s * M * N * 4 if s > 1 else 0


def linear_ws_bytes(M, K, N):
    """bn_linear_ws_bytes: the larger of what the forward and the data gradient may ask for."""
    if M <= 0 or K <= 0 or N <= 0:
        return 0
    return max(gemm_ws_bytes(M, N, K), gemm_ws_bytes(M, K, N))


def _cdiv_trunc(a, b):
    """C's a / b for a of either sign (b > 0)."""
    return a // b if a >= 0 else -((-a) // b)


def wave_share(K, kslice, nw, z, ws):
    """(kbeg, kend) of wave ``ws`` of slice ``z`` (gemm_tile); empty where kend <= kbeg."""
    zbeg = z * kslice
    zend = min(K, zbeg + kslice)
    kper = _cdiv_trunc(zend - zbeg + nw - 1, nw)
    kper = (kper + 7) & ~7
    kbeg = zbeg + ws * kper
    return kbeg, min(zend, kbeg + kper)


def load_path(strides, kbeg, kend):
    """The load loop gemm_tile runs on a share, operands 16-byte aligned."""
    sai, sak, sbk, sbj = strides
    ranged = kbeg % 8 == 0 and kend % 4 == 0 and kend - kbeg >= 4
    if sak == 1 and sbk == 1 and ranged and sai % 4 == 0 and sbj % 4 == 0:
        return 'vec'
    if sak == 1 and ranged and sai % 4 == 0:
        return 'veca'
    return 'scalar'


def gemm_job(M, N, K, strides, split):
    """gemm_job of one product; ``split``: a scratch for its partial tiles was handed to it."""
    tiles = _cdiv(N, 32) * _cdiv(M, 32)
    slices = gemm_slices(M, N, K) if split else 1
    kslice = (_cdiv(K, slices) + 15) & ~15
    kw = kslice // 32
    nw = 4 if kw >= 4 else 2 if kw >= 2 else 1
    upb = GJ_WAVES // nw
    units = tiles * slices
    blocks = _cdiv(units, upb)
    past = sum(1 for z in range(slices) if z * kslice >= K)
    last = slices - 1 - past
    shares = [[wave_share(K, kslice, nw, z, ws) for ws in range(nw)] for z in range(slices)]
    empty = sum(1 for kbeg, kend in shares[last] if kend <= kbeg)
    loads = frozenset(load_path(strides, kbeg, kend) for row in shares for kbeg, kend in row if kend > kbeg)
    return Job(M, N, K, slices, kslice, nw, tiles, units, upb, blocks, blocks * upb - units, past, empty,
               load_path(strides, *shares[0][0]), loads, slices * M * N * 4 if slices > 1 else 0)


def routes(M, K, N, need_dx=True, need_dw=True):
    """{job: Job} of one linear layer with a scratch of exactly bn_linear_ws_bytes(M, K, N) in both directions, as
    _hip.linear_fwd / linear_bwd pass it (the backward pass takes none without a data gradient).  A product splits
    only if its partial tiles fit what is left: the data gradient is served first, the weight gradient second."""
    ops = operands(M, K, N)
    out = {}
    ws = linear_ws_bytes(M, K, N)
    need = jobs_ws_bytes(*ops['fwd'][:3])
    out['fwd'] = gemm_job(*ops['fwd'], split=bool(need) and ws >= need)
    left = ws if need_dx else 0
    for job, wanted in (('dx', need_dx), ('dw', need_dw)):
        if not wanted:
            continue
        need = jobs_ws_bytes(*ops[job][:3])
        split = bool(need) and left >= need
        if split:
            left -= need
        out[job] = gemm_job(*ops[job], split=split)
    return out


def has_split(M, K, N):
    return any(j.slices > 1 for j in routes(M, K, N).values())


SPLIT_CASES = [c for c in CASES if has_split(*c)]


def column_sum_job(M, N):
    """(workgroups, columns of the last one, rows of the last trip) of the db job of k_linear_jobs."""
    return _cdiv(N, DB_COLS), N - (_cdiv(N, DB_COLS) - 1) * DB_COLS, M - (_cdiv(M, DB_ROWS) - 1) * DB_ROWS


def operand_bytes(M, K, N):
    """x, w, b, y / dy, dx, dw, db."""
    return 4 * (2 * M * K + 2 * N * K + 2 * N + 2 * M * N)
