// Augmented second-moment matrices per row segment of a row-major fp32 table ("latent
// correlations"): for every segment s -- the rows [e[s], e[s+1]) -- with the row vector
//
//   a = (1, (double)z_0 - (double)c_0, ..., (double)z_{D-1} - (double)c_{D-1})            c = the shift, or zeros
//
//   out[s] = sum over the segment's rows of a^T a           float64 (D + 1, D + 1)
//
// so out[s][0][0] is the row count, out[s][0][1 + j] = out[s][1 + j][0] the column sums and out[s][1 + i][1 + j] the
// second moments.  Every term is formed in float64 from the fp32 operands and every sum is float64.  A NaN or Inf in
// column j reaches the products with a_j alone: row and column 1 + j of its segment; the count is the number of rows.
//
// Segments and partition are those of segment_sums.hip: the offsets are clamped and made non-decreasing by the same
// launch (bn_launch_segment_offsets), sg_plan cuts the n rows into row blocks as a function of (n, D) alone, a
// segment inside a block is finished there (k_sg_stream) and one that crosses blocks leaves a "head" or "tail"
// partial in the block's own slab, summed in block order by k_sg_combine, which also writes the zeros of the empty
// segments.  Every out element is written exactly once, there are no global atomics, and the order of every sum is
// fixed by (n, S, D) and the offsets.  A partial is (D + 1)^2 doubles, 33 KB at D = 64, so the block count is
// capped by SG_SLAB_BYTES as well.
//
// Inner product: v_mfma_f64_16x16x4_f64 (a vector-FMA variant measured 1.1 to 1.6 times slower).
// The D columns are padded with zeros to DP = 16 TB, TB = 1 .. 4 (a template argument: the accumulators need constant
// indices), and the D x D second moments are the TB (TB + 1) / 2 tiles of 16 x 16 with ti <= tj.  A chunk of 32 rows
// is staged in LDS as shifted doubles (16-byte loads of whole quads where base and leading dimension allow, element
// by element otherwise; the columns from D on are never read from the table, the rows past the segment's end are
// zeros, not rows of the table: zero times a NaN would be a NaN).  A k-step is four rows; lane l of a wave reads ONE
// double a column block -- row l >> 4 of the step, column l & 15 of the block: the A fragment of the block as a tile
// row and the B fragment of it as a tile column --, adds it to its column sum and issues the TB (TB + 1) / 2 MFMAs.
// The four waves take the k-steps of a chunk in turn; at the end of a segment their tiles are added through LDS in
// wave order and the column sums in (wave, row-of-step) order.  The count is the number of rows, from the offsets.
// A tile's result sits at col = lane & 15, row = (lane >> 4) + 4 * reg (the f64 map, not the f32 one); an element
// with i <= j is written to [1 + i][1 + j] and mirrored: A[i][j] and A[j][i] are one value.  A NaN in column j is an
// operand of the products with a_j alone.  The inputs are never written.
#include "bn_common.h"
#include "bn_launch.h"

#define SG_THREADS 256
#define SG_MAX_D 64
#define SG_WAVES (SG_THREADS / BN_WAVE)
#define SG_ROWS 32                          // rows of a staged chunk: eight k-steps of four rows, two a wave
#define SG_MIN_ELEMS (1 << 14)              // elements a row block holds at least (but for the last)
#define SG_TARGET_GROUPS 1024               // row blocks at most ...
#define SG_SLAB_BYTES (32u << 20)           // ... and no more than fit two partials each into 32 MiB
#define SG_COMBINE_ENTRIES 32              // entries of a matrix a combine workgroup sums ...
#define SG_COMBINE_PARTS 8                 // ... with this many threads an entry
#define SG_COMBINE_THREADS (SG_COMBINE_ENTRIES * SG_COMBINE_PARTS)
#define SG_COMBINE_GROUPS 4096             // combine workgroups aimed at

typedef float sg_f4 __attribute__((ext_vector_type(4)));
typedef double sg_d4 __attribute__((ext_vector_type(4)));

struct SgPlan {
    int blocks;       // row blocks
    int rows;         // rows per block (the last block takes what is left)
};

// the ONE partition the workspace query, the launches and the combine go by
static SgPlan sg_plan(int n, int D) {
    SgPlan p;
    if (n < 1) {
        p.blocks = 0;
        p.rows = 1;
        return p;
    }
    const long W = D + 1;
    const long by_bytes = SG_SLAB_BYTES / (2 * W * W * (long)sizeof(double));         // 496 at D = 64
    const long cap = by_bytes < SG_TARGET_GROUPS ? by_bytes : SG_TARGET_GROUPS;
    const long min_rows = SG_MIN_ELEMS / D;                                            // D <= 64: at least 256
    const long by_rows = ((long)n + min_rows - 1) / min_rows;
    const long want = by_rows < cap ? by_rows : cap;
    p.rows = (int)(((long)n + want - 1) / want);
    p.blocks = (int)(((long)n + p.rows - 1) / p.rows);
    return p;
}

static size_t sg_offsets_bytes(int S) { return (((size_t)S + 1) * sizeof(int) + 15) & ~(size_t)15; }

template <int TB>
__global__ __launch_bounds__(SG_THREADS) void k_sg_stream(const float* __restrict__ z, int ld,
                                                          const float* __restrict__ c, const int* __restrict__ e,
                                                          int S, int D, int n, int rows, double* __restrict__ out,
                                                          double* __restrict__ slabs) {
    constexpr int DP = 16 * TB, LW = DP + 4, NT = TB * (TB + 1) / 2;          // (LW: a k-step's four rows on other banks)
    __shared__ __attribute__((aligned(32))) double stage[SG_ROWS * LW];
    __shared__ double red[SG_WAVES - 1][4 * BN_WAVE];
    __shared__ double csum[SG_WAVES][4][DP];
    __shared__ double shift[DP];
    const int tid = threadIdx.x, lane = tid & (BN_WAVE - 1), wave = tid / BN_WAVE;
    const int kk = lane >> 4, col = lane & 15;
    const int W = D + 1;
    const bool vec = !((uintptr_t)z & 15) && !(ld & 3);
    const int Q = vec ? D >> 2 : 0;                        // whole quads of a row, read as 16 bytes
    const int rest = D - 4 * Q;                            // columns read one by one
    const size_t outs = (size_t)W * W;
    const int row0 = blockIdx.x * rows;
    const int row1 = n - row0 > rows ? row0 + rows : n;

    if (tid < D) shift[tid] = c ? (double)c[tid] : 0.0;
    // the padding columns of every staged row: written once, the staging never touches them
    for (int idx = tid; idx < SG_ROWS * (LW - D); idx += SG_THREADS) {
        const int r = idx / (LW - D);
        stage[r * LW + D + idx - r * (LW - D)] = 0.0;
    }

    // the first segment that ends after row0
    int s;
    {
        int lo = 0, hi = S;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (e[mid + 1] > row0) hi = mid; else lo = mid + 1;
        }
        s = lo;
    }
    for (; s < S; ++s) {
        const int beg = e[s], end = e[s + 1];
        if (beg >= row1) break;
        const int a = beg > row0 ? beg : row0, b = end < row1 ? end : row1;
        if (b <= a) continue;                              // an empty segment: k_sg_combine writes its zeros
        sg_d4 acc[NT];
        double sum[TB];
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = sg_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int q = 0; q < TB; ++q) sum[q] = 0.0;
        for (long r0 = a; r0 < b; r0 += SG_ROWS) {
            const int cnt = b - r0 < SG_ROWS ? (int)(b - r0) : SG_ROWS;
            const int steps = (cnt + 3) >> 2;
            __syncthreads();                               // (the chunk before this one has been read; shift is there)
            for (int idx = tid; idx < cnt * Q; idx += SG_THREADS) {
                const int r = idx / Q, q = idx - r * Q;
                const sg_f4 v = __builtin_nontemporal_load(
                    reinterpret_cast<const sg_f4*>(z + (size_t)(r0 + r) * ld + 4 * q));
                double* d = stage + r * LW + 4 * q;
                d[0] = (double)v.x - shift[4 * q];
                d[1] = (double)v.y - shift[4 * q + 1];
                d[2] = (double)v.z - shift[4 * q + 2];
                d[3] = (double)v.w - shift[4 * q + 3];
            }
            for (int idx = tid; idx < cnt * rest; idx += SG_THREADS) {
                const int r = idx / rest, j = 4 * Q + idx - r * rest;
                stage[r * LW + j] = (double)__builtin_nontemporal_load(z + (size_t)(r0 + r) * ld + j) - shift[j];
            }
            // the rows that fill the last k-step: zeros
            for (int idx = tid; idx < (4 * steps - cnt) * D; idx += SG_THREADS) {
                const int r = idx / D;
                stage[(cnt + r) * LW + idx - r * D] = 0.0;
            }
            __syncthreads();
            for (int ks = wave; ks < steps; ks += SG_WAVES) {
                double frag[TB];
#pragma unroll
                for (int q = 0; q < TB; ++q) {
                    frag[q] = stage[(4 * ks + kk) * LW + 16 * q + col];
                    sum[q] += frag[q];
                }
                int t = 0;
#pragma unroll
                for (int ti = 0; ti < TB; ++ti)
#pragma unroll
                    for (int tj = ti; tj < TB; ++tj, ++t)
                        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(frag[ti], frag[tj], acc[t], 0, 0, 0);
            }
        }
        double* dst = beg >= row0 && end <= row1 ? out + (size_t)s * outs
                                                 : slabs + ((size_t)blockIdx.x * 2 + (beg < row0 ? 0 : 1)) * outs;
        // the tiles, one at a time: the waves' partials added in wave order.  C/D of the f64 MFMA: column lane & 15,
        // row (lane >> 4) + 4 * reg
        int t = 0;
#pragma unroll
        for (int ti = 0; ti < TB; ++ti)
#pragma unroll
            for (int tj = ti; tj < TB; ++tj, ++t) {
                __syncthreads();                           // (red has been read)
                if (wave) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) red[wave - 1][r * BN_WAVE + lane] = acc[t][r];
                }
                if (t == 0) {
#pragma unroll
                    for (int q = 0; q < TB; ++q) csum[wave][kk][16 * q + col] = sum[q];
                }
                __syncthreads();
                if (!wave) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        double v = acc[t][r];
#pragma unroll
                        for (int w = 0; w < SG_WAVES - 1; ++w) v += red[w][r * BN_WAVE + lane];
                        const int i = 16 * ti + kk + 4 * r, j = 16 * tj + col;
                        if (i <= j && j < D) {             // (the upper triangle, mirrored; i <= j < D)
                            dst[(size_t)(1 + i) * W + 1 + j] = v;
                            if (i != j) dst[(size_t)(1 + j) * W + 1 + i] = v;
                        }
                    }
                }
            }
        // the count and the column sums, the latter in (wave, row of the k-step) order; csum was written before the
        // first tile's second barrier and is written again only after the next segment's barriers
        if (tid == 0) dst[0] = (double)(b - a);
        if (tid < D) {
            double v = 0.0;
#pragma unroll
            for (int w = 0; w < SG_WAVES; ++w)
#pragma unroll
                for (int k = 0; k < 4; ++k) v += csum[w][k][tid];
            dst[1 + tid] = v;
            dst[(size_t)(1 + tid) * W] = v;
        }
    }
}

// grid (segment, y): zeros for an empty segment, the partials of one that crosses row blocks summed in block order.
// A workgroup takes 32 entries of the matrix at a time, every gridDim.y-th such chunk; eight threads an entry take
// every eighth piece and their sums are added in thread order (the grid's shape does not enter any sum).
__global__ __launch_bounds__(SG_COMBINE_THREADS) void k_sg_combine(const int* __restrict__ e, int D, int rows,
                                                                   const double* __restrict__ slabs,
                                                                   double* __restrict__ out) {
    __shared__ double part[SG_COMBINE_PARTS][SG_COMBINE_ENTRIES];
    const int s = blockIdx.x, W = D + 1;
    const int lo = threadIdx.x % SG_COMBINE_ENTRIES, p = threadIdx.x / SG_COMBINE_ENTRIES;
    const size_t outs = (size_t)W * W;
    const int beg = e[s], end = e[s + 1];
    double* dst = out + (size_t)s * outs;
    if (end <= beg) {
        for (size_t o = (size_t)blockIdx.y * SG_COMBINE_THREADS + threadIdx.x; o < outs;
             o += (size_t)gridDim.y * SG_COMBINE_THREADS)
            dst[o] = 0.0;
        return;
    }
    const int b0 = beg / rows, b1 = (end - 1) / rows;
    if (b0 == b1) return;                                  // (k_sg_stream has written it)
    // piece 0 is the tail of block b0, piece i the head of block b0 + i
    const int pieces = b1 - b0 + 1;
    for (size_t base = (size_t)blockIdx.y * SG_COMBINE_ENTRIES; base < outs;
         base += (size_t)gridDim.y * SG_COMBINE_ENTRIES) {
        const size_t o = base + lo;
        double sum = 0.0;
        if (o < outs) {
#pragma unroll 4
            for (int i = p; i < pieces; i += SG_COMBINE_PARTS)
                sum += slabs[((size_t)(b0 + i) * 2 + (i == 0 ? 1 : 0)) * outs + o];
        }
        part[p][lo] = sum;
        __syncthreads();
        if (p == 0 && o < outs) {
            double total = part[0][lo];
#pragma unroll
            for (int k = 1; k < SG_COMBINE_PARTS; ++k) total += part[k][lo];
            dst[o] = total;
        }
        __syncthreads();                                   // (part is written again)
    }
}

// ------------------------------------------------------------------------------------------------------------
bool bn_segment_gram_ok(int n, int S, int D) {
    return n >= 0 && S >= 0 && S < INT32_MAX && D >= 1 && D <= SG_MAX_D;      // (S + 1 offsets are counted in an int)
}

size_t bn_segment_gram_ws_bytes_impl(int n, int S, int D) {
    if (!bn_segment_gram_ok(n, S, D)) return 0;
    return sg_offsets_bytes(S) + (size_t)sg_plan(n, D).blocks * 2 * (D + 1) * (D + 1) * sizeof(double);
}

int bn_launch_segment_gram(const float* z, int ld, const float* c, const long long* offsets, int S, int D, int n,
                           double* out, void* ws, hipStream_t st) {
    if (!bn_segment_gram_ok(n, S, D)) return BN_E_SHAPE;
    if (S == 0) return 0;
    const SgPlan p = sg_plan(n, D);
    int* e = reinterpret_cast<int*>(ws);
    double* slabs = reinterpret_cast<double*>(reinterpret_cast<char*>(ws) + sg_offsets_bytes(S));
    const int rc = bn_launch_segment_offsets(offsets, S + 1, n, e, st);
    if (rc) return rc;
    if (p.blocks) {
        const dim3 grid((unsigned)p.blocks), block(SG_THREADS);
        const int* ce = e;
        switch ((D + 15) / 16) {                           // column blocks of 16
            case 1: hipLaunchKernelGGL(k_sg_stream<1>, grid, block, 0, st, z, ld, c, ce, S, D, n, p.rows, out, slabs); break;
            case 2: hipLaunchKernelGGL(k_sg_stream<2>, grid, block, 0, st, z, ld, c, ce, S, D, n, p.rows, out, slabs); break;
            case 3: hipLaunchKernelGGL(k_sg_stream<3>, grid, block, 0, st, z, ld, c, ce, S, D, n, p.rows, out, slabs); break;
            default: hipLaunchKernelGGL(k_sg_stream<4>, grid, block, 0, st, z, ld, c, ce, S, D, n, p.rows, out, slabs); break;
        }
        BN_LAUNCH_CHECK();
    }
    // one workgroup a 32 entries for a few segments, one a segment for thousands (most of which it only looks at)
    const unsigned chunks = (unsigned)(((D + 1) * (D + 1) + SG_COMBINE_ENTRIES - 1) / SG_COMBINE_ENTRIES);
    const unsigned fit = SG_COMBINE_GROUPS / (unsigned)S;
    const unsigned gy = fit < 1 ? 1 : (fit < chunks ? fit : chunks);
    hipLaunchKernelGGL(k_sg_combine, dim3((unsigned)S, gy), dim3(SG_COMBINE_THREADS), 0, st, (const int*)e, D,
                       p.rows, (const double*)slabs, out);
    BN_LAUNCH_CHECK();
    return 0;
}
