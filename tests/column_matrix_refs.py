"""The column-matrix rung of the convolution ladder, restated in plain Python: which GEMM kernel
``bn_launch_gemm`` (csrc/gemm.hip) picks for a product, in how many reduction slices, and how
``bn_launch_col_down / _wgrad / _up`` (csrc/conv_pad.hip) cut a batch into passes and size their scratch.

Nothing here calls the library: tests/test_column_matrix_host.py holds the restatement against
``bn_conv_ws_bytes`` (the split counts enter that number as ``slices * M * N * 4``), so a drift between this
file and the C code fails without a GPU, and tests/test_gpu_column_matrix.py uses it to say which kernel a
case's numbers vouch for.

``k_gemm_tiled<1,0>`` (A i-contiguous with B k-contiguous) has no caller: none of the three roles sets its
operands that way.  ``gemm_route`` names it for completeness; no case reaches it and no test asks for it.
"""

GT_M, GT_N, GT_K = 64, 128, 32              # the tiled kernel's tile (gemm.hip)
COL_MAX_BYTES = 512 << 20                   # conv_pad.hip
COL_MAX_ROWS = 1 << 21                      # col_frames' cap on the rows of a pass

# (name, N, C, H, W, K, R, stride, (pt, pb), (pl, pr)) as tests/test_gpu_kernels.py CONV_CASES
CASES = [
    ('s3_k3_c72_c72', 2, 72, 69, 69, 72, 3, 3, (0, 0), (0, 0)),
    ('s3_k5_c64_c64', 2, 64, 62, 62, 64, 5, 3, (1, 1), (1, 1)),
    ('s3_k3_c64_c128', 3, 64, 48, 48, 128, 3, 3, (0, 0), (0, 0)),
    ('k1_c64_c64_32x32', 1, 64, 32, 32, 64, 1, 1, (0, 0), (0, 0)),
    ('k1_c72_c136_33x31', 1, 72, 33, 31, 136, 1, 1, (0, 0), (0, 0)),
    ('k1_c64_c512_32x32', 1, 64, 32, 32, 512, 1, 1, (0, 0), (0, 0)),
    ('s4_k5_c64_c64', 2, 64, 64, 64, 64, 5, 4, (1, 2), (1, 2)),
    ('s3_k3_c16_c32_n40', 40, 16, 27, 27, 32, 3, 3, (0, 0), (0, 0)),
    ('s3_k5_c48_c24', 2, 48, 30, 30, 24, 5, 3, (1, 1), (1, 1)),
    ('k1_c3_c5_300x300_n24', 24, 3, 300, 300, 5, 1, 1, (0, 0), (0, 0)),
    ('k1_c3_c5_256x256_n33', 33, 3, 256, 256, 5, 1, 1, (0, 0), (0, 0)),
]
# the two whose batch does not fit one pass (col_frames < N)
MULTI_PASS = ('k1_c3_c5_300x300_n24', 'k1_c3_c5_256x256_n33')

ROLES = ('down', 'wgrad', 'up')
# the entry point of bn_conv2d_* that runs a role, as tests/ladder_cases.kernel_names keys it, and the name
# the profiling hook reports on this rung
ENTRY = {'down': 'fwd', 'wgrad': 'bwd_weight', 'up': 'bwd_data'}
RUNG_NAMES = {'fwd': 'k_im2col + k_gemm_mfma', 'bwd_data': 'k_gemm_mfma + k_col2im',
              'bwd_weight': 'k_im2col + k_gemm_mfma (dW)'}


def _cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------
# gemm.hip
# ------------------------------------------------------------------------------------------------------
def gemm_slices(M, N, K):
    """Reduction slices of k_gemm_mfma (gemm_slices)."""
    tiles = _cdiv(N, 32) * _cdiv(M, 32)
    if K < 1024 or tiles > 32:
        return 1
    s = K // 128
    cap = 16
    while cap < 128 and tiles * cap < 512 and K // (2 * cap) >= 256:
        cap *= 2
    return max(min(s, cap), 1)


def gemm_tiled_slices(M, N, K):
    """Reduction slices of k_gemm_tiled (gemm_tiled_slices)."""
    tiles = _cdiv(N, GT_N) * _cdiv(M, GT_M)
    if tiles >= 256 or K < 512:
        return 1
    return max(min(512 // tiles, K // 128, 64), 1)


def gemm_tiled_ok(M, N, K, sai, sak, sbk, sbj):
    """(ta, tb) if the tiled kernel takes the product (16-byte aligned operands assumed), else None."""
    if M < 64 or N < 64 or K < 64 or M * N < 64 * 1024:
        return None
    if sak == 1:
        ta = 0
        if K & 7 or sai & 3:
            return None
    elif sai == 1:
        ta = 1
        if M & 7 or sak & 3:
            return None
    else:
        return None
    if sbk == 1:
        tb = 0
        if K & 7 or sbj & 3:
            return None
    elif sbj == 1:
        tb = 1
        if N & 7 or sbk & 3:
            return None
    else:
        return None
    return ta, tb


def gemm_route(M, N, K, sai, sak, sbk, sbj):
    """(kernel, slices) of bn_launch_gemm on C (M x N) = A (M x K) B (K x N) with a scratch as large as
    bn_gemm_ws_bytes asks for."""
    t = gemm_tiled_ok(M, N, K, sai, sak, sbk, sbj)
    if t is not None and _cdiv(M, GT_M) < 65536:
        return 'k_gemm_tiled<%d,%d>' % t, gemm_tiled_slices(M, N, K)
    waves = 8 if K >= 512 else 4 if K >= 128 else 1
    return 'k_gemm_mfma<%d>' % waves, gemm_slices(M, N, K)


def gemm_grid(M, N, K, sai, sak, sbk, sbj):
    """The launch grid (x, y, z) of the kernel gemm_route names."""
    kernel, slices = gemm_route(M, N, K, sai, sak, sbk, sbj)
    if kernel.startswith('k_gemm_tiled'):
        return _cdiv(N, GT_N), _cdiv(M, GT_M), slices
    return _cdiv(N, 32), _cdiv(M, 32), slices


def gemm_ws_bytes(M, N, K):
    """bn_gemm_ws_bytes: the partial tiles of whichever kernel may take the product."""
    s = gemm_slices(M, N, K)
    need = s * M * N * 4 if s > 1 else 0
    if M >= 64 and N >= 64 and K >= 64:
        ts = gemm_tiled_slices(M, N, K)
        if ts > 1:
            need = max(need, ts * M * N * 4)
    return need


# ------------------------------------------------------------------------------------------------------
# conv_pad.hip / capi.hip
# ------------------------------------------------------------------------------------------------------
def geom_of(case):
    """(N, Cb, Cs, PQ, RS) of a CONV_CASES-style tuple: frames, channels of the big and the small side,
    pixels of the small map, taps."""
    name, N, C, H, W, K, R, st, (pt, pb), (pl, pr) = case
    P, Q = (H + pt + pb - R) // st + 1, (W + pl + pr - R) // st + 1
    return N, C, K, P * Q, R * R


def conv_geom(case):
    """The 12 integers bn_conv_ws_bytes / bn_conv2d_* take after the op."""
    name, N, C, H, W, K, R, st, (pt, pb), (pl, pr) = case
    P, Q = (H + pt + pb - R) // st + 1, (W + pl + pr - R) // st + 1
    return N, C, H, W, K, R, R, st, pt, pl, P, Q


def transposed(case):
    """The transposed layer between the same maps (small (K, P, Q) -> big (C, H, W), cropped by the conv's
    pads), as tests/test_gpu_kernels.py RANDOM_T_CASES builds its CONVT_CASES-style tuples."""
    c = case
    return (c[0] + 'T', c[1], c[5], (c[3] + sum(c[8]) - c[6]) // c[7] + 1, (c[4] + sum(c[9]) - c[6]) // c[7] + 1,
            c[2], c[6], c[7], 0, (c[9][0], c[9][1], c[8][0], c[8][1]), 0)


def col_frames(case):
    """Frames per pass: the column matrix stays below 512 MB and its rows at or below 2^21."""
    N, Cb, Cs, PQ, RS = geom_of(case)
    per = PQ * Cb * RS * 4
    return min(COL_MAX_BYTES // max(per, 1), COL_MAX_ROWS // PQ, N)


def passes(case):
    """Frames of every pass of the bn_launch_col_* loop."""
    N, nb = geom_of(case)[0], col_frames(case)
    return [min(nb, N - n0) for n0 in range(0, N, nb)]


def roles(case, frames=None):
    """[(M, N, K, (sai, sak, sbk, sbj))] of down, wgrad and up, as bn_launch_col_down / _wgrad / _up set
    GemmArgs for a pass of ``frames`` frames (default: the first pass)."""
    N, Cb, Cs, PQ, RS = geom_of(case)
    rows = (col_frames(case) if frames is None else frames) * PQ
    K = Cb * RS
    return [(rows, Cs, K, (K, 1, 1, K)),            # tmp[i, m] = sum_k col[i, k] W[m, k]
            (Cs, K, rows, (1, Cs, K, 1)),           # dW[m, k] += sum_i srows[i, m] col[i, k]
            (rows, K, Cs, (Cs, 1, K, 1))]           # colg[i, k] = sum_m srows[i, m] W[m, k]


def routes(case):
    """{role: [(kernel, slices) per pass]}."""
    out = {r: [] for r in ROLES}
    for nf in passes(case):
        for role, (M, N, K, strides) in zip(ROLES, roles(case, nf)):
            out[role].append(gemm_route(M, N, K, *strides))
    return out


def _align256(n):
    return (n + 255) & ~255


def col_ws_bytes(case):
    """bn_col_ws_bytes: column matrix + row matrix + the largest split scratch of the three products."""
    N, Cb, Cs, PQ, RS = geom_of(case)
    rows, K = col_frames(case) * PQ, Cb * RS
    gw = max(gemm_ws_bytes(rows, Cs, K), gemm_ws_bytes(Cs, K, rows), gemm_ws_bytes(rows, K, Cs))
    return _align256(rows * K * 4) + _align256(rows * Cs * 4) + gw


def channel_sum_ws_bytes(N, C, npix):
    """bn_channel_sum_ws_bytes (conv_generic.hip): the bias gradient's partial sums, one per channel and
    frame slice, once the reduction is 8192 elements long."""
    if N * npix < 8192:
        return 0
    s = max(min(1024 // C, 256, N), 1)
    return C * s * 4 if s > 1 else 0


def conv_ws_bytes(op, case):
    """bn_conv_ws_bytes(op, ...) for a geometry on the column-matrix rung; ops 1, 2, 3 = bn_conv2d_fwd,
    _bwd_data, _bwd_weight.  The weight gradient's query adds the scratch of the bias gradient that runs
    after it (capi.hip: ``role_ws_need(role, g) + (role == 2 ? bias_ws : 0)``)."""
    N, Cb, Cs, PQ, RS = geom_of(case)
    need = col_ws_bytes(case)
    if op == 3:
        need += channel_sum_ws_bytes(N, Cs, PQ)
    return need
