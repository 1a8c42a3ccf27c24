// Masked column sums per row segment of three row-major fp32 tables ("label scores"): for every
// segment s -- the rows [e[s], e[s+1]) -- and every column j < L, over the entries (i, j) that are valid (no mask, or
// mask[i, j] == 1.0f exactly; any other value, NaN included, is not),
//
//   out[s][j] = { count, sum y, sum y^2, sum (y - p)^2 }        y = (double)truth[i, j], p = (double)pred[i, j]
//
// Every term is formed in float64 from the fp32 operands and every sum is float64.  An invalid entry is selected out,
// not multiplied by zero: what lies under a zero mask never reaches a sum.  A NaN under a one mask propagates.
//
// Segments.  e is the offsets vector made safe: e[i] = max over k <= i of clamp(offsets[k], 0, n).  The segments are
// then disjoint and ascending, an offset that steps back gives an empty segment, and the rows outside
// [e[0], e[S]) belong to no segment and are never read.  k_sl_offsets writes e (int32) to the workspace first.
//
// Partition.  sl_plan cuts the n rows into row blocks, a function of (n, L) alone; the workspace query, the launches
// and the combine go by it.  k_sl_stream: one workgroup per row block walks the segments that meet its block (found by
// a binary search in e).  A segment that lies inside the block is reduced there and written to out.  A segment that
// crosses a block boundary leaves one partial per block it meets, in that block's own slab of the workspace: "head"
// for a segment that began in an earlier block, "tail" for one that begins here and goes on (a block has at most one
// of each, the segments being disjoint).  k_sl_combine (one workgroup per segment) sums a crossing segment's partials
// in block order -- tail of its first block, heads of the others -- and writes the zeros of the empty segments.  So a
// long segment is spread over all row blocks, thousands of short ones are finished where they are streamed, every
// out element is written exactly once, there are no global atomics, and every sum is formed in an order that
// (n, S, L) and the offsets fix: the same bits on every call, whatever order the workgroups run in.
//
// Threads.  A thread owns four consecutive columns (a "quad") of every SL_THREADS / Q2-th row, Q2 = the quads of a
// row rounded up to a power of two: its column never changes, so the 16 running sums live in registers and the next
// element is one pointer addition away.  A whole quad of a table whose base and leading dimension are multiples of
// 16 bytes is one non-temporal 16-byte load (the tables are read once); a partial quad (L not a multiple of 4: the
// columns from L on are not read, the last row may end there) and a table that is not so aligned are read element
// by element.  Four rows are in flight per thread.  A segment's partials are reduced over the rows' lanes by
// xor-shuffles inside a wave and over the four waves through LDS, in fixed order.  The inputs are never written.
#include "bn_common.h"
#include "bn_launch.h"

#define SL_THREADS 256
#define SL_WAVES (SL_THREADS / BN_WAVE)
#define SL_MAX_L 64
#define SL_MAX_QUADS (SL_MAX_L / 4)
#define SL_MIN_ELEMS (1 << 14)     // elements of one table a row block holds at least (but for the last): 64 KiB a table
#define SL_TARGET_GROUPS 1024      // row blocks the rows are cut into at most: four workgroups a CU
#define SL_SCAN_THREADS 1024
#define SL_COMBINE_THREADS 1024

typedef float sl_f4 __attribute__((ext_vector_type(4)));

struct SlPlan {
    int blocks;       // row blocks
    int rows;         // rows per block (the last block takes what is left)
};

// the ONE partition the workspace query, the launches and the combine go by
static SlPlan sl_plan(int n, int L) {
    SlPlan p;
    if (n < 1) {
        p.blocks = 0;
        p.rows = 1;
        return p;
    }
    const long min_rows = SL_MIN_ELEMS / L;                // L <= 64: at least 256
    const long by_rows = ((long)n + min_rows - 1) / min_rows;
    const long want = by_rows < SL_TARGET_GROUPS ? by_rows : SL_TARGET_GROUPS;
    p.rows = (int)(((long)n + want - 1) / want);
    p.blocks = (int)(((long)n + p.rows - 1) / p.rows);
    return p;
}

// bytes of e, rounded to the 16-byte boundary the slabs start on
static size_t sl_offsets_bytes(int S) { return (((size_t)S + 1) * sizeof(int) + 15) & ~(size_t)15; }

// ------------------------------------------------------------------------------------------------------------
// e[i] = max_{k <= i} clamp(offsets[k], 0, n): thread t takes the t-th run of consecutive offsets
__global__ __launch_bounds__(SL_SCAN_THREADS) void k_sl_offsets(const long long* __restrict__ offsets, int count, int n,
                                                                 int* __restrict__ e) {
    __shared__ int top[2][SL_SCAN_THREADS];
    const int t = threadIdx.x;
    const long per = ((long)count + SL_SCAN_THREADS - 1) / SL_SCAN_THREADS;
    const long i0 = t * per;
    const long i1 = i0 + per < count ? i0 + per : count;
    int mine = 0;
    for (long i = i0; i < i1; ++i) {
        const long long o = offsets[i];
        const int c = o < 0 ? 0 : (o > n ? n : (int)o);
        mine = c > mine ? c : mine;
    }
    top[0][t] = mine;
    __syncthreads();
    int cur = 0;
    for (int off = 1; off < SL_SCAN_THREADS; off <<= 1) {
        const int a = top[cur][t], b = t >= off ? top[cur][t - off] : 0;
        top[cur ^ 1][t] = a > b ? a : b;
        __syncthreads();
        cur ^= 1;
    }
    int run = t ? top[cur][t - 1] : 0;                     // the maximum of the runs before this one
    for (long i = i0; i < i1; ++i) {
        const long long o = offsets[i];
        const int c = o < 0 ? 0 : (o > n ? n : (int)o);
        run = c > run ? c : run;
        e[i] = run;
    }
}

// ------------------------------------------------------------------------------------------------------------
// ncol (1 to 4) elements at p: one 16-byte load where the caller found the quad whole and aligned
__device__ __forceinline__ void sl_load(const float* __restrict__ p, bool vec, int ncol, float v[4]) {
    if (vec) {
        const sl_f4 q = __builtin_nontemporal_load(reinterpret_cast<const sl_f4*>(p));
        v[0] = q.x;
        v[1] = q.y;
        v[2] = q.z;
        v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < ncol ? __builtin_nontemporal_load(p + j) : 0.f;
    }
}

struct SlRow {
    float p[4], y[4], m[4];
};

__device__ __forceinline__ bool sl_vec_ok(const float* x, int ld) { return x && !((uintptr_t)x & 15) && !(ld & 3); }

__global__ __launch_bounds__(SL_THREADS) void k_sl_stream(const float* __restrict__ pred, int ld_pred,
                                                          const float* __restrict__ truth, int ld_truth,
                                                          const float* __restrict__ mask, int ld_mask,
                                                          const int* __restrict__ e, int S, int L, int n, int rows,
                                                          double* __restrict__ out, double* __restrict__ slabs) {
    __shared__ double red[2][SL_WAVES][SL_MAX_QUADS][16];
    const int quads = (L + 3) >> 2;
    int q2 = 1;
    while (q2 < quads) q2 <<= 1;                           // 1, 2, 4, 8 or 16: a wave holds 64 / q2 rows
    const int tid = threadIdx.x;
    const int q = tid & (q2 - 1), lane_row = tid / q2, rpi = SL_THREADS / q2;
    int ncol = L - 4 * q;
    ncol = ncol < 0 ? 0 : (ncol > 4 ? 4 : ncol);           // (0: a quad past the last column, its thread only reduces)
    const bool whole = ncol == 4;
    const bool vp = whole && sl_vec_ok(pred, ld_pred), vy = whole && sl_vec_ok(truth, ld_truth);
    const bool vm = whole && sl_vec_ok(mask, ld_mask);
    const int row0 = blockIdx.x * rows;                    // (blocks * rows < n + rows: no overflow for n < 2^31 - rows)
    const int row1 = n - row0 > rows ? row0 + rows : n;

    // the first segment that ends after row0
    int s = S;
    {
        int lo = 0, hi = S;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (e[mid + 1] > row0) hi = mid; else lo = mid + 1;
        }
        s = lo;
    }
    int buf = 0;
    for (; s < S; ++s) {
        const int beg = e[s], end = e[s + 1];
        if (beg >= row1) break;
        const int a = beg > row0 ? beg : row0, z = end < row1 ? end : row1;
        if (z <= a) continue;                              // an empty segment: k_sl_combine writes its zeros
        double acc[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[k] = 0.0;
        if (ncol) {
            const float* pp = pred + ((size_t)a + lane_row) * ld_pred + 4 * q;
            const float* py = truth + ((size_t)a + lane_row) * ld_truth + 4 * q;
            const float* pm = mask ? mask + ((size_t)a + lane_row) * ld_mask + 4 * q : nullptr;
            const size_t sp = (size_t)rpi * ld_pred, sy = (size_t)rpi * ld_truth, sm = (size_t)rpi * ld_mask;
            auto load = [&](SlRow& r) {
                sl_load(pp, vp, ncol, r.p);
                sl_load(py, vy, ncol, r.y);
                if (pm) {
                    sl_load(pm, vm, ncol, r.m);
                    pm += sm;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) r.m[j] = j < ncol ? 1.f : 0.f;
                }
                pp += sp;
                py += sy;
            };
            auto add = [&](const SlRow& r) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (r.m[j] == 1.f) {                   // selected, not weighted
                        const double y = (double)r.y[j], d = y - (double)r.p[j];
                        acc[4 * j] += 1.0;
                        acc[4 * j + 1] += y;
                        acc[4 * j + 2] += y * y;
                        acc[4 * j + 3] += d * d;
                    }
                }
            };
            // (long: i + 3 rpi may pass 2^31 near the end of the largest table)
            long i = (long)a + lane_row;
            for (; i + 3 * rpi < z; i += 4 * rpi) {        // four rows in flight
                SlRow r0, r1, r2, r3;
                load(r0);
                load(r1);
                load(r2);
                load(r3);
                add(r0);
                add(r1);
                add(r2);
                add(r3);
            }
            for (; i < z; i += rpi) {
                SlRow r;
                load(r);
                add(r);
            }
        }
        // over the rows of a wave (lanes that differ in the bits from q2 up), then over the waves
        for (int m = q2; m < BN_WAVE; m <<= 1) {
#pragma unroll
            for (int k = 0; k < 16; ++k) acc[k] += __shfl_xor(acc[k], m);
        }
        if ((tid & (BN_WAVE - 1)) < q2) {
#pragma unroll
            for (int k = 0; k < 16; ++k) red[buf][tid / BN_WAVE][q][k] = acc[k];
        }
        __syncthreads();
        if (tid < 16 * q2) {
            const int oq = tid >> 4, k = tid & 15, c = 4 * oq + (k >> 2);
            if (c < L) {
                double total = red[buf][0][oq][k];
#pragma unroll
                for (int w = 1; w < SL_WAVES; ++w) total += red[buf][w][oq][k];
                double* dst = beg >= row0 && end <= row1 ? out + (size_t)s * L * 4
                                                         : slabs + ((size_t)blockIdx.x * 2 + (beg < row0 ? 0 : 1)) * L * 4;
                dst[c * 4 + (k & 3)] = total;
            }
        }
        buf ^= 1;                                          // (the next segment's partials go to the other half: one
                                                           // barrier a segment is enough)
    }
}

// one workgroup per segment: zeros for an empty one, the partials of one that crosses row blocks summed in block order
__global__ __launch_bounds__(SL_COMBINE_THREADS) void k_sl_combine(const int* __restrict__ e, int L, int rows,
                                                                   const double* __restrict__ slabs,
                                                                   double* __restrict__ out) {
    __shared__ double part[SL_COMBINE_THREADS];
    const int s = blockIdx.x, t = threadIdx.x, outs = 4 * L;
    const int beg = e[s], end = e[s + 1];
    double* dst = out + (size_t)s * outs;
    if (end <= beg) {
        if (t < outs) dst[t] = 0.0;
        return;
    }
    const int b0 = beg / rows, b1 = (end - 1) / rows;
    if (b0 == b1) return;                                  // (k_sl_stream has written it)
    int o2 = 4;
    while (o2 < outs) o2 <<= 1;                            // 4 .. 256
    const int parts = SL_COMBINE_THREADS / o2, mine = t / o2, o = t & (o2 - 1);
    const int pieces = b1 - b0 + 1;
    double sum = 0.0;
    if (o < outs) {
        // piece 0 is the tail of block b0, piece i the head of block b0 + i
#pragma unroll 8
        for (int i = mine; i < pieces; i += parts)
            sum += slabs[((size_t)(b0 + i) * 2 + (i == 0 ? 1 : 0)) * outs + o];
    }
    part[t] = sum;
    __syncthreads();
    if (t < outs) {
        double total = part[t];
        for (int k = 1; k < parts; ++k) total += part[k * o2 + t];
        dst[t] = total;
    }
}

// ------------------------------------------------------------------------------------------------------------
bool bn_segment_label_sums_ok(int n, int S, int L) {
    return n >= 0 && S >= 0 && S < INT32_MAX && L >= 1 && L <= SL_MAX_L;      // (S + 1 offsets are counted in an int)
}

size_t bn_segment_label_sums_ws_bytes_impl(int n, int S, int L) {
    if (!bn_segment_label_sums_ok(n, S, L)) return 0;
    return sl_offsets_bytes(S) + (size_t)sl_plan(n, L).blocks * 2 * L * 4 * sizeof(double);
}

// e[i] = max_{k <= i} clamp(offsets[k], 0, n) for count offsets (segment_gram.hip makes its segments safe by it too)
int bn_launch_segment_offsets(const long long* offsets, int count, int n, int* e, hipStream_t st) {
    hipLaunchKernelGGL(k_sl_offsets, dim3(1), dim3(SL_SCAN_THREADS), 0, st, offsets, count, n, e);
    BN_LAUNCH_CHECK();
    return 0;
}

int bn_launch_segment_label_sums(const float* pred, int ld_pred, const float* truth, int ld_truth, const float* mask,
                                 int ld_mask, const long long* offsets, int S, int L, int n, double* out, void* ws,
                                 hipStream_t st) {
    if (!bn_segment_label_sums_ok(n, S, L)) return BN_E_SHAPE;
    if (S == 0) return 0;
    const SlPlan p = sl_plan(n, L);
    int* e = reinterpret_cast<int*>(ws);
    double* slabs = reinterpret_cast<double*>(reinterpret_cast<char*>(ws) + sl_offsets_bytes(S));
    const int rc = bn_launch_segment_offsets(offsets, S + 1, n, e, st);
    if (rc) return rc;
    if (p.blocks) {
        hipLaunchKernelGGL(k_sl_stream, dim3((unsigned)p.blocks), dim3(SL_THREADS), 0, st, pred, ld_pred, truth,
                           ld_truth, mask, ld_mask, (const int*)e, S, L, n, p.rows, out, slabs);
        BN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_sl_combine, dim3((unsigned)S), dim3(SL_COMBINE_THREADS), 0, st, (const int*)e, L, p.rows,
                       (const double*)slabs, out);
    BN_LAUNCH_CHECK();
    return 0;
}
