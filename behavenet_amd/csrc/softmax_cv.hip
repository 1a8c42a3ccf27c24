// Loss, gradient and held-out score of M multinomial logistic models at once over the rows of a row-major fp32 table
// ("session classifier"): the device side of the cross-validated session classifier, whose
// (fold, C) models differ only in their weights and in the fold they leave out.  With l = W_m (z, 1) in float64,
//
//   bn_softmax_cv_lossgrad   loss[m]  = sum over the rows m includes of logsumexp_k(l_k) - l_y
//                            grad[m]  = sum over those rows of (softmax(l) - onehot(y)) (x) (z, 1)       (S, D + 1)
//                            count[m] = the number of those rows
//   bn_softmax_cv_score      out[m]   = (rows of m's held-out fold whose argmax_k l_k is y, rows of that fold)
//
// A row is included by model m when its y lies in [0, S) and its fold is not leave[m] (no fold array: a row belongs
// to no fold); it is scored by model m when its y lies in [0, S) and leave[m] is -1 or the row's fold.
//
// Partition (segment_gram.hip's scheme): sc_plan cuts the n rows into row blocks and the M models into groups of at
// most 128 / S models as a function of (n, D, S, M) alone -- the ONE plan the workspace query and the launch go by.
// Workgroup (block, group) leaves one partial a model of its group in the block's slab, and k_sc_combine adds the
// slabs in block order: every output element is written exactly once, there are no global atomics, and the order of
// every sum is fixed by (n, D, S, M).
//
// Inner products: v_mfma_f64_16x16x4_f64, twice a chunk of 32 staged rows.  The group's (model, class) pairs are
// the "columns" c, 128 at most, in 8 tiles of 16; tile t belongs to wave t & 3, which keeps the tile's weights as B
// fragments in registers for the whole block (column c of the group is row m0 S + c of W: the groups need no index
// table).  D is padded with zeros to DP = 16 TB.
//   logits (32 x 128) = rows (32 x DP) . W^T (DP x 128):  A = the staged rows (lane l: row l & 15, k = l >> 4), the
//       accumulator starts at the intercept; the result -- column l & 15, row (l >> 4) + 4 reg, the f64 map -- goes
//       to LDS.
//   softmax: one thread a (row, model): the row maximum is subtracted, exp and log are the float64 ones, and the
//       residual softmax - onehot replaces the logits in LDS -- zeros for a row the model does not include.
//   gradient (128 x DP) += residual^T (128 x 32) . rows (32 x DP): A = the residuals (lane l: column l & 15, row
//       l >> 4), B = the staged rows as segment_gram.hip reads them; the lane's A values summed are the intercept's
//       gradient.  A wave owns its tiles' accumulators over the whole block: no sum crosses waves.
// A row with a NaN or Inf in its D columns is staged as zeros and marked: the models that include it get NaN as its
// loss and residual (NaN times the staged zero is NaN in every column and the intercept), the others 0 times 0; the
// score reads its argmax as class 0, as np.argmax of a row of NaNs does.  The inputs are never written.
#include "bn_common.h"
#include "bn_launch.h"

#define SC_THREADS 256
#define SC_WAVES (SC_THREADS / BN_WAVE)
#define SC_MAX_D 64
#define SC_MAX_S 8
#define SC_MAX_M 64
#define SC_ROWS 32                          // rows of a staged chunk: two row tiles, eight k-steps of the gradient
#define SC_CT 2                             // column tiles a wave
#define SC_GC (16 * SC_CT * SC_WAVES)       // columns (model, class) a group holds at most: 128
#define SC_LG (SC_GC + 16)                  // leading dimension of the logits in LDS (a k-step's rows on other banks)
#define SC_MIN_ROWS 128                     // rows a row block holds at least (but for the last)
#define SC_TARGET_BLOCKS 1024               // row blocks at most ...
#define SC_SLAB_BYTES (32u << 20)           // ... and no more than fit their partials into 32 MiB
#define SC_COMBINE_ENTRIES 32               // entries a combine workgroup sums ...
#define SC_COMBINE_PARTS 8                  // ... with this many threads an entry
#define SC_COMBINE_THREADS (SC_COMBINE_ENTRIES * SC_COMBINE_PARTS)

typedef float sc_f4 __attribute__((ext_vector_type(4)));
typedef double sc_d4 __attribute__((ext_vector_type(4)));

struct ScPlan {
    int blocks;       // row blocks
    int rows;         // rows per block (the last block takes what is left)
    int mg;           // models a group (the last group takes what is left)
    int mgp;          // mg rounded up to a power of two: the softmax pass gives a model 256 / mgp threads
    int groups;       // model groups
};

// the ONE partition the workspace query, the launches and the combine go by; pm = doubles of a model's partial
static ScPlan sc_plan(int n, int S, int M, int pm) {
    ScPlan p;
    p.mg = SC_GC / S < M ? SC_GC / S : M;
    p.mgp = 1;
    while (p.mgp < p.mg) p.mgp <<= 1;
    p.groups = (M + p.mg - 1) / p.mg;
    if (n < 1) {
        p.blocks = 0;
        p.rows = 1;
        return p;
    }
    const long by_bytes = SC_SLAB_BYTES / ((long)M * pm * (long)sizeof(double));      // 125 at M = 64, S = 8, D = 64
    const long cap = by_bytes < SC_TARGET_BLOCKS ? by_bytes : SC_TARGET_BLOCKS;
    const long by_rows = ((long)n + SC_MIN_ROWS - 1) / SC_MIN_ROWS;
    const long want = by_rows < cap ? by_rows : cap;
    p.rows = (int)(((long)n + want - 1) / want);
    p.blocks = (int)(((long)n + p.rows - 1) / p.rows);
    return p;
}

static int sc_pm(int D, int S, bool score) { return score ? 2 : S * (D + 1) + 2; }

// slabs: (blocks, M, pm) doubles; a model's partial is its gradient (S, D + 1), loss and count -- or, SCORE, the
// hits and the rows of its fold
template <int TB, bool SCORE>
__global__ __launch_bounds__(SC_THREADS) void k_sc_stream(const float* __restrict__ z, int ld,
                                                          const int* __restrict__ y, const int* __restrict__ fold,
                                                          const double* __restrict__ Wt,
                                                          const int* __restrict__ leave, int n, int D, int S, int M,
                                                          int mg, int mgp, int rows, int pm,
                                                          double* __restrict__ slabs) {
    constexpr int DP = 16 * TB, LW = DP + 2, KS = 4 * TB;                  // (LW: a tile's sixteen rows on other banks)
    __shared__ double stage[SC_ROWS * LW];
    __shared__ double lg[SC_ROWS * SC_LG];
    __shared__ double csum[4][SC_GC];
    __shared__ double red[2][SC_THREADS];
    __shared__ int poison[2][SC_ROWS], ys[SC_ROWS], fs[SC_ROWS];
    const int tid = threadIdx.x, lane = tid & (BN_WAVE - 1), wave = tid / BN_WAVE;
    const int kk = lane >> 4, col = lane & 15;
    const int W1 = D + 1;
    const bool vec = !((uintptr_t)z & 15) && !(ld & 3);
    const int Q = vec ? D >> 2 : 0;                        // whole quads of a row, read as 16 bytes
    const int rest = D - 4 * Q;                            // columns read one by one
    const int row0 = blockIdx.x * rows;
    const int row1 = n - row0 > rows ? row0 + rows : n;
    const int m0 = blockIdx.y * mg;
    const int mc = M - m0 < mg ? M - m0 : mg;              // models of this group
    const int ncols = mc * S;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);

    // the weights of the wave's column tiles as B fragments of the logits' product: column 16 t + (lane & 15),
    // k = 4 ks + (lane >> 4); zeros past the group's columns and past D
    double wf[SC_CT][KS], bias[SC_CT];
    bool act[SC_CT];
#pragma unroll
    for (int ct = 0; ct < SC_CT; ++ct) {
        const int t = ct * SC_WAVES + wave, c = 16 * t + col;
        act[ct] = 16 * t < ncols;                          // (the same for all lanes of the wave)
        const double* wr = c < ncols ? Wt + ((size_t)m0 * S + c) * W1 : nullptr;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) wf[ct][ks] = wr && 4 * ks + kk < D ? wr[4 * ks + kk] : 0.0;
        bias[ct] = wr ? wr[D] : 0.0;
    }
    // the padding columns of every staged row: written once, the staging never touches them
    for (int idx = tid; idx < SC_ROWS * (LW - D); idx += SC_THREADS) {
        const int r = idx / (LW - D);
        stage[r * LW + D + idx - r * (LW - D)] = 0.0;
    }
    if (tid < 2 * SC_ROWS) poison[tid / SC_ROWS][tid % SC_ROWS] = 0;

    // the softmax pass: thread (part, mi) takes model m0 + mi and every tpm-th row of the chunk
    const int mi = tid & (mgp - 1), part = tid / mgp, tpm = SC_THREADS / mgp;
    const int lv = mi < mc ? leave[m0 + mi] : -1;
    double acc0 = 0.0, acc1 = 0.0;                         // loss and count, or hits and rows
    sc_d4 g[SC_CT][TB];
    double rs[SC_CT];
#pragma unroll
    for (int ct = 0; ct < SC_CT; ++ct) {
        rs[ct] = 0.0;
#pragma unroll
        for (int q = 0; q < TB; ++q) g[ct][q] = sc_d4{0.0, 0.0, 0.0, 0.0};
    }

    int par = 0;
    for (long r0 = row0; r0 < row1; r0 += SC_ROWS, par ^= 1) {
        const int cnt = row1 - r0 < SC_ROWS ? (int)(row1 - r0) : SC_ROWS;
        __syncthreads();                                   // (the chunk before this one has been read)
        for (int idx = tid; idx < cnt * Q; idx += SC_THREADS) {
            const int r = idx / Q, q = idx - r * Q;
            const sc_f4 v = __builtin_nontemporal_load(
                reinterpret_cast<const sc_f4*>(z + (size_t)(r0 + r) * ld + 4 * q));
            double* d = stage + r * LW + 4 * q;
            d[0] = (double)v.x;
            d[1] = (double)v.y;
            d[2] = (double)v.z;
            d[3] = (double)v.w;
            if (!(isfinite(v.x) && isfinite(v.y) && isfinite(v.z) && isfinite(v.w))) poison[par][r] = 1;
        }
        for (int idx = tid; idx < cnt * rest; idx += SC_THREADS) {
            const int r = idx / rest, j = 4 * Q + idx - r * rest;
            const float v = __builtin_nontemporal_load(z + (size_t)(r0 + r) * ld + j);
            stage[r * LW + j] = (double)v;
            if (!isfinite(v)) poison[par][r] = 1;
        }
        // the rows past the block's end: zeros, and a class no model includes
        for (int idx = tid; idx < (SC_ROWS - cnt) * D; idx += SC_THREADS) {
            const int r = idx / D;
            stage[(cnt + r) * LW + idx - r * D] = 0.0;
        }
        if (tid < SC_ROWS) {
            ys[tid] = tid < cnt ? y[r0 + tid] : -1;
            fs[tid] = tid < cnt && fold ? fold[r0 + tid] : -1;
        }
        __syncthreads();
        // a marked row enters the products as zeros
        for (int idx = tid; idx < SC_ROWS * D; idx += SC_THREADS) {
            const int r = idx / D;
            if (poison[par][r]) stage[r * LW + idx - r * D] = 0.0;
        }
        if (tid < SC_ROWS) poison[par ^ 1][tid] = 0;       // (read last before this chunk's first barrier)
        __syncthreads();
        // logits
#pragma unroll
        for (int rt = 0; rt < SC_ROWS / 16; ++rt) {
            double af[KS];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) af[ks] = stage[(16 * rt + col) * LW + 4 * ks + kk];
#pragma unroll
            for (int ct = 0; ct < SC_CT; ++ct) {
                if (!act[ct]) continue;
                sc_d4 a = sc_d4{bias[ct], bias[ct], bias[ct], bias[ct]};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks)
                    a = __builtin_amdgcn_mfma_f64_16x16x4f64(af[ks], wf[ct][ks], a, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    lg[(16 * rt + kk + 4 * r) * SC_LG + 16 * (ct * SC_WAVES + wave) + col] = a[r];
            }
        }
        __syncthreads();
        if (mi < mc) {
            for (int r = part; r < SC_ROWS; r += tpm) {
                const int yy = ys[r], ff = fs[r];
                const bool valid = (unsigned)yy < (unsigned)S;
                double* l = lg + r * SC_LG + mi * S;
                if (SCORE) {
                    if (!valid || (lv >= 0 && ff != lv)) continue;
                    int best = 0;
                    if (!poison[par][r]) {
                        double top = l[0];
                        for (int s = 1; s < S; ++s)
                            if (l[s] > top) {              // (a tie stays with the lowest class)
                                top = l[s];
                                best = s;
                            }
                    }
                    acc0 += best == yy ? 1.0 : 0.0;
                    acc1 += 1.0;
                } else if (!valid || (lv >= 0 && ff == lv)) {
                    for (int s = 0; s < S; ++s) l[s] = 0.0;
                } else if (poison[par][r]) {
                    for (int s = 0; s < S; ++s) l[s] = nan;
                    acc0 += nan;
                    acc1 += 1.0;
                } else {
                    double top = l[0];
                    for (int s = 1; s < S; ++s) top = l[s] > top ? l[s] : top;
                    const double ly = l[yy];
                    double sum = 0.0;
                    for (int s = 0; s < S; ++s) {
                        const double e = exp(l[s] - top);
                        l[s] = e;
                        sum += e;
                    }
                    for (int s = 0; s < S; ++s) l[s] = l[s] / sum - (s == yy ? 1.0 : 0.0);
                    acc0 += (top - ly) + log(sum);
                    acc1 += 1.0;
                }
            }
        }
        if (SCORE) continue;
        __syncthreads();
        // gradient: the residuals' transpose times the staged rows, four rows a step
#pragma unroll
        for (int ks = 0; ks < SC_ROWS / 4; ++ks) {
            double bf[TB];
#pragma unroll
            for (int q = 0; q < TB; ++q) bf[q] = stage[(4 * ks + kk) * LW + 16 * q + col];
#pragma unroll
            for (int ct = 0; ct < SC_CT; ++ct) {
                if (!act[ct]) continue;
                const double a = lg[(4 * ks + kk) * SC_LG + 16 * (ct * SC_WAVES + wave) + col];
                rs[ct] += a;
#pragma unroll
                for (int q = 0; q < TB; ++q)
                    g[ct][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bf[q], g[ct][q], 0, 0, 0);
            }
        }
    }

    // a model's partial: the sums of its threads of the softmax pass in thread order ...
    double* slab = slabs + ((size_t)blockIdx.x * M + m0) * pm;
    const int tail = SCORE ? 0 : S * W1;
    __syncthreads();
    red[0][tid] = acc0;
    red[1][tid] = acc1;
    if (!SCORE) {
#pragma unroll
        for (int ct = 0; ct < SC_CT; ++ct) csum[kk][16 * (ct * SC_WAVES + wave) + col] = act[ct] ? rs[ct] : 0.0;
    }
    __syncthreads();
    if (tid < mc) {
        double a = 0.0, b = 0.0;
        for (int p = 0; p < tpm; ++p) {
            a += red[0][p * mgp + tid];
            b += red[1][p * mgp + tid];
        }
        slab[(size_t)tid * pm + tail] = a;
        slab[(size_t)tid * pm + tail + 1] = b;
    }
    if (SCORE) return;
    // ... the intercept's gradient in row-of-the-k-step order, and the tiles: column 16 t + (lane >> 4) + 4 reg of
    // the group, latent 16 q + (lane & 15)
    if (tid < ncols) {
        const double v = ((csum[0][tid] + csum[1][tid]) + csum[2][tid]) + csum[3][tid];
        slab[(size_t)(tid / S) * pm + (tid % S) * W1 + D] = v;
    }
#pragma unroll
    for (int ct = 0; ct < SC_CT; ++ct) {
        if (!act[ct]) continue;
#pragma unroll
        for (int q = 0; q < TB; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = 16 * (ct * SC_WAVES + wave) + kk + 4 * r, d = 16 * q + col;
                if (c < ncols && d < D) slab[(size_t)(c / S) * pm + (c % S) * W1 + d] = g[ct][q][r];
            }
    }
}

// entry o = m pm + e of the M pm entries of a slab, summed over the blocks in block order: eight threads an entry
// take every eighth block and their sums are added in thread order.  e < split goes to o0[m split + e], e == split to
// o1[m], e == split + 1 to o2[m].  No blocks (n == 0): zeros.
__global__ __launch_bounds__(SC_COMBINE_THREADS) void k_sc_combine(const double* __restrict__ slabs, int blocks,
                                                                   int M, int pm, int split, double* __restrict__ o0,
                                                                   double* __restrict__ o1, double* __restrict__ o2) {
    __shared__ double part[SC_COMBINE_PARTS][SC_COMBINE_ENTRIES];
    const int lo = threadIdx.x % SC_COMBINE_ENTRIES, p = threadIdx.x / SC_COMBINE_ENTRIES;
    const int E = M * pm;
    const int o = blockIdx.x * SC_COMBINE_ENTRIES + lo;
    double sum = 0.0;
    if (o < E) {
#pragma unroll 4
        for (int i = p; i < blocks; i += SC_COMBINE_PARTS) sum += slabs[(size_t)i * E + o];
    }
    part[p][lo] = sum;
    __syncthreads();
    if (p == 0 && o < E) {
        double total = part[0][lo];
#pragma unroll
        for (int k = 1; k < SC_COMBINE_PARTS; ++k) total += part[k][lo];
        const int m = o / pm, e = o - m * pm;
        if (e < split) o0[(size_t)m * split + e] = total;
        else if (e == split) o1[m] = total;
        else o2[m] = total;
    }
}

// ------------------------------------------------------------------------------------------------------------
bool bn_softmax_cv_ok(int n, int D, int S, int M) {
    return n >= 0 && D >= 1 && D <= SC_MAX_D && S >= 2 && S <= SC_MAX_S && M >= 1 && M <= SC_MAX_M;
}

size_t bn_softmax_cv_ws_bytes_impl(int n, int D, int S, int M, bool score) {
    if (!bn_softmax_cv_ok(n, D, S, M)) return 0;
    const int pm = sc_pm(D, S, score);
    const size_t bytes = (size_t)sc_plan(n, S, M, pm).blocks * M * pm * sizeof(double);
    return bytes ? bytes : 16;                             // (n == 0: nothing is kept, and 0 says "not served")
}

template <bool SCORE>
static int sc_launch(const float* z, int ld, const int* y, const int* fold, const double* W, const int* leave, int n,
                     int D, int S, int M, double* o0, double* o1, double* o2, void* ws, hipStream_t st) {
    if (!bn_softmax_cv_ok(n, D, S, M)) return BN_E_SHAPE;
    const int pm = sc_pm(D, S, SCORE);
    const ScPlan p = sc_plan(n, S, M, pm);
    double* slabs = reinterpret_cast<double*>(ws);
    if (p.blocks) {
        const dim3 grid((unsigned)p.blocks, (unsigned)p.groups), block(SC_THREADS);
        switch ((D + 15) / 16) {                           // column blocks of 16
            case 1: hipLaunchKernelGGL((k_sc_stream<1, SCORE>), grid, block, 0, st, z, ld, y, fold, W, leave, n, D, S, M, p.mg, p.mgp, p.rows, pm, slabs); break;
            case 2: hipLaunchKernelGGL((k_sc_stream<2, SCORE>), grid, block, 0, st, z, ld, y, fold, W, leave, n, D, S, M, p.mg, p.mgp, p.rows, pm, slabs); break;
            case 3: hipLaunchKernelGGL((k_sc_stream<3, SCORE>), grid, block, 0, st, z, ld, y, fold, W, leave, n, D, S, M, p.mg, p.mgp, p.rows, pm, slabs); break;
            default: hipLaunchKernelGGL((k_sc_stream<4, SCORE>), grid, block, 0, st, z, ld, y, fold, W, leave, n, D, S, M, p.mg, p.mgp, p.rows, pm, slabs); break;
        }
        BN_LAUNCH_CHECK();
    }
    const unsigned groups = (unsigned)((M * pm + SC_COMBINE_ENTRIES - 1) / SC_COMBINE_ENTRIES);
    hipLaunchKernelGGL(k_sc_combine, dim3(groups), dim3(SC_COMBINE_THREADS), 0, st, (const double*)slabs, p.blocks, M,
                       pm, SCORE ? 2 : S * (D + 1), o0, o1, o2);
    BN_LAUNCH_CHECK();
    return 0;
}

int bn_launch_softmax_cv_lossgrad(const float* z, int ld, const int* y, const int* fold, const double* W,
                                  const int* leave, int n, int D, int S, int M, double* loss, double* grad,
                                  double* count, void* ws, hipStream_t st) {
    return sc_launch<false>(z, ld, y, fold, W, leave, n, D, S, M, grad, loss, count, ws, st);
}

int bn_launch_softmax_cv_score(const float* z, int ld, const int* y, const int* fold, const double* W,
                               const int* leave, int n, int D, int S, int M, double* out, void* ws, hipStream_t st) {
    return sc_launch<true>(z, ld, y, fold, W, leave, n, D, S, M, out, nullptr, nullptr, ws, st);
}
