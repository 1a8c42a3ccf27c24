// A table of discrete states -> its runs, per trial ("state runs and syllable movies"): what the
// reference's get_discrete_chunks finds with np.pad / np.ediff1d per trial on the host, as a stream compaction.
//
//   states  int32 (n)      the Viterbi table (bn_hmm_viterbi)
//   e       int32 (S + 1)  the trials, made safe by bn_launch_segment_offsets (clamped into [0, n], ascending); rows
//                          outside [e[0], e[S]) belong to no trial and are never loaded
//
// Row i of trial s STARTS a run iff i == e[s] or states[i] != states[i - 1], and ENDS one iff i + 1 == e[s + 1] or
// states[i + 1] != states[i].  The run a row belongs to is (starts at or before it) - 1, so
//
//   runs[p] = (trial, beg, end, state)     beg, end relative to e[trial], end exclusive
//
// is filled from two sides: the row that starts run p writes trial, beg and state, the row that ends it writes end
// (a one-row run is one 16-byte store).  Nobody needs to look ahead for a run's end, and no atomic decides an order.
//
// Three launches over tiles of SR_TILE rows (256 threads of four consecutive rows each):
//   k_sr_count   start flags of a tile -> counts[tile]; frames[k], trans[j][k] and bad through an LDS histogram
//                (integer atomics: the sums do not depend on their order) that is flushed with one 64-bit global
//                atomic per non-zero bin.  A thread folds equal neighbouring keys of its four rows into one LDS
//                atomic, so a table of long runs does not serialise on one bin.
//   k_sr_scan    ONE workgroup: the exclusive prefix sum of counts, SR_SCAN counts a step with a carry -> bases, n_runs
//   k_sr_write   the flags again, an exclusive scan inside the tile, and the stores above at bases[tile] + rank.
// The trial of a thread's first row is a binary search in e for the first trial that ends after it -- which skips
// empty trials -- and is searched again (from the trial after) only when a row passes the trial's end.
//
// HBM-bound, no matrix cores: the states are read twice (4 n bytes each; the neighbours' loads hit the cache), 16 R
// bytes are written.  Every output is an integer and every position comes from the prefix sums: the same values
// whatever the launch geometry or the order in which workgroups run.
#include <limits.h>
#include "bn_common.h"
#include "bn_launch.h"

#define SR_THREADS 256
#define SR_WAVES (SR_THREADS / BN_WAVE)
#define SR_PER 4                            // consecutive rows a thread owns
#define SR_TILE (SR_THREADS * SR_PER)       // rows a workgroup takes (_hip.STATE_RUNS_TILE)
#define SR_SCAN 1024                        // tile counts k_sr_scan takes a step (_hip.STATE_RUNS_SCAN)
#define SR_MAX_K 32                         // (arhmm.hip's AR_MAX_K)
#define SR_BINS (SR_MAX_K * SR_MAX_K + SR_MAX_K + 1)

#define SR_IN 1
#define SR_START 2
#define SR_END 4

static size_t sr_pad16(size_t b) { return (b + 15) & ~(size_t)15; }
static size_t sr_offsets_bytes(int S) { return sr_pad16(((size_t)S + 1) * sizeof(int)); }
static long sr_tiles(int n) { return ((long)n + SR_TILE - 1) / SR_TILE; }

struct SrRows {
    int v[SR_PER + 2];          // states of the rows r0 - 1 .. r0 + SR_PER (0 where the row is in no trial)
    int trial[SR_PER];
    int rel[SR_PER];            // the row's index inside its trial
    int fl[SR_PER];             // SR_IN | SR_START | SR_END
};

// the first trial of [lo, hi] that ends after row r (e[lo] <= r < e[hi + 1]): never an empty one
__device__ __forceinline__ int sr_trial(const int* __restrict__ e, int lo, int hi, long r) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (e[mid + 1] > r) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// the thread's rows r0 .. r0 + SR_PER - 1: states, trial, flags.  Only rows of [e[0], e[S]) are loaded.
__device__ __forceinline__ void sr_rows(const int* __restrict__ states, const int* __restrict__ e, int S, int vec,
                                        long r0, SrRows& w) {
    const long a = e[0], z = e[S];
    if (vec && r0 >= a && r0 + SR_PER <= z) {
        const int4 q = *reinterpret_cast<const int4*>(states + r0);
        w.v[1] = q.x, w.v[2] = q.y, w.v[3] = q.z, w.v[4] = q.w;
    } else {
#pragma unroll
        for (int j = 1; j <= SR_PER; ++j) {
            const long i = r0 - 1 + j;
            w.v[j] = (i >= a && i < z) ? states[i] : 0;
        }
    }
    w.v[0] = (r0 - 1 >= a && r0 - 1 < z) ? states[r0 - 1] : 0;
    w.v[SR_PER + 1] = (r0 + SR_PER >= a && r0 + SR_PER < z) ? states[r0 + SR_PER] : 0;
    int s = -1;
    long es = 0, es1 = 0;
#pragma unroll
    for (int j = 0; j < SR_PER; ++j) {
        const long i = r0 + j;
        int fl = 0;
        if (i >= a && i < z) {
            if (s < 0 || i >= es1) {
                s = sr_trial(e, s + 1, S - 1, i);
                es = e[s], es1 = e[s + 1];
            }
            fl = SR_IN;
            if (i == es || w.v[j + 1] != w.v[j]) fl |= SR_START;
            if (i + 1 == es1 || w.v[j + 2] != w.v[j + 1]) fl |= SR_END;
            w.trial[j] = s;
            w.rel[j] = (int)(i - es);
        } else {
            w.trial[j] = 0, w.rel[j] = 0;
        }
        w.fl[j] = fl;
    }
}

// exclusive prefix sum of `mine` over the workgroup's threads, and the workgroup's total
__device__ __forceinline__ long sr_block_scan(long mine, long* waves, long& total) {
    const int lane = threadIdx.x & (BN_WAVE - 1), wv = threadIdx.x / BN_WAVE;
    long inc = mine;
#pragma unroll
    for (int off = 1; off < BN_WAVE; off <<= 1) {
        const long o = __shfl_up(inc, off, BN_WAVE);
        if (lane >= off) inc += o;
    }
    if (lane == BN_WAVE - 1) waves[wv] = inc;
    __syncthreads();
    long before = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < SR_WAVES; ++k) {
        const long c = waves[k];
        if (k < wv) before += c;
        total += c;
    }
    __syncthreads();          // (waves may be written again)
    return before + inc - mine;
}

__global__ __launch_bounds__(256) void k_sr_zero(long long* __restrict__ frames, long long* __restrict__ trans, int K,
                                                 long long* __restrict__ n_runs, long long* __restrict__ bad) {
    const int t = threadIdx.x;
    for (int i = t; i < K; i += 256) frames[i] = 0;
    for (int i = t; i < K * K; i += 256) trans[i] = 0;
    if (t == 0) *n_runs = 0, *bad = 0;
}

// equal neighbouring keys of a thread fold into one LDS atomic
struct SrFold {
    int key, cnt;
    __device__ __forceinline__ void add(int* bins, int k) {
        if (k == key) {
            ++cnt;
        } else {
            if (cnt) atomicAdd(&bins[key], cnt);
            key = k, cnt = 1;
        }
    }
    __device__ __forceinline__ void flush(int* bins) {
        if (cnt) atomicAdd(&bins[key], cnt);
        cnt = 0;
    }
};

__global__ __launch_bounds__(SR_THREADS) void k_sr_count(const int* __restrict__ states, const int* __restrict__ e,
                                                         int S, int K, int vec, int* __restrict__ counts,
                                                         long long* __restrict__ frames, long long* __restrict__ trans,
                                                         long long* __restrict__ bad) {
    __shared__ int bins[SR_BINS];           // trans (K K), frames (K), bad
    __shared__ long waves[SR_WAVES];
    const int t = threadIdx.x, KK = K * K, n_bins = KK + K + 1;
    for (int i = t; i < n_bins; i += SR_THREADS) bins[i] = 0;
    __syncthreads();
    SrRows w;
    sr_rows(states, e, S, vec, (long)blockIdx.x * SR_TILE + (long)t * SR_PER, w);
    int starts = 0;
    SrFold pair = {0, 0}, one = {0, 0};
#pragma unroll
    for (int j = 0; j < SR_PER; ++j) {
        if (!(w.fl[j] & SR_IN)) continue;
        starts += (w.fl[j] & SR_START) ? 1 : 0;
        const int v = w.v[j + 1], p = w.v[j];
        const bool ok = (unsigned)v < (unsigned)K;
        one.add(bins, ok ? KK + v : KK + K);
        // (rel > 0: the row before is a row of the same trial)
        if (ok && w.rel[j] > 0 && (unsigned)p < (unsigned)K) pair.add(bins, p * K + v);
    }
    one.flush(bins);
    pair.flush(bins);
    long total;
    sr_block_scan(starts, waves, total);            // (its barriers also order the LDS atomics before the flush)
    if (t == 0) counts[blockIdx.x] = (int)total;
    for (int i = t; i < n_bins; i += SR_THREADS) {
        const int c = bins[i];
        if (!c) continue;
        long long* dst = i < KK ? trans + i : (i < KK + K ? frames + (i - KK) : bad);
        atomicAdd(reinterpret_cast<unsigned long long*>(dst), (unsigned long long)c);
    }
}

__global__ __launch_bounds__(SR_THREADS) void k_sr_scan(const int* __restrict__ counts, long tiles,
                                                        int* __restrict__ bases, long long* __restrict__ n_runs) {
    __shared__ long waves[SR_WAVES];
    const int t = threadIdx.x;
    constexpr int PER = SR_SCAN / SR_THREADS;
    long carry = 0;
    for (long c0 = 0; c0 < tiles; c0 += SR_SCAN) {
        int c[PER];
        long mine = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const long i = c0 + (long)t * PER + j;
            c[j] = i < tiles ? counts[i] : 0;
            mine += c[j];
        }
        long total;
        long at = carry + sr_block_scan(mine, waves, total);
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const long i = c0 + (long)t * PER + j;
            if (i < tiles) bases[i] = (int)at;          // (at most n < 2^31 runs)
            at += c[j];
        }
        carry += total;
    }
    if (t == 0) *n_runs = carry;
}

__global__ __launch_bounds__(SR_THREADS) void k_sr_write(const int* __restrict__ states, const int* __restrict__ e,
                                                         int S, int vec, const int* __restrict__ bases,
                                                         int* __restrict__ runs, long long cap) {
    __shared__ long waves[SR_WAVES];
    SrRows w;
    sr_rows(states, e, S, vec, (long)blockIdx.x * SR_TILE + (long)threadIdx.x * SR_PER, w);
    int starts = 0;
#pragma unroll
    for (int j = 0; j < SR_PER; ++j) starts += (w.fl[j] & SR_START) ? 1 : 0;
    long total;
    long pos = (long)bases[blockIdx.x] + sr_block_scan(starts, waves, total);       // starts before the thread's rows
#pragma unroll
    for (int j = 0; j < SR_PER; ++j) {
        const int fl = w.fl[j];
        if (!(fl & SR_IN)) continue;
        if (fl & SR_START) ++pos;
        // (the first row of the trials starts a run: pos >= 1 here)
        const long q = pos - 1;
        if (q >= cap) continue;
        int* row = runs + q * 4;
        if ((fl & SR_START) && (fl & SR_END)) {
            *reinterpret_cast<int4*>(row) = make_int4(w.trial[j], w.rel[j], w.rel[j] + 1, w.v[j + 1]);
        } else if (fl & SR_START) {
            row[0] = w.trial[j], row[1] = w.rel[j], row[3] = w.v[j + 1];
        } else if (fl & SR_END) {
            row[2] = w.rel[j] + 1;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------
bool bn_state_runs_ok(int n, int S, int K) {
    return n >= 0 && S >= 0 && S < INT32_MAX && K >= 1 && K <= SR_MAX_K;
}

size_t bn_state_runs_ws_bytes_impl(int n, int S, int K) {
    if (!bn_state_runs_ok(n, S, K)) return 0;
    return sr_offsets_bytes(S) + 2 * sr_pad16((size_t)sr_tiles(n) * sizeof(int));
}

int bn_launch_state_runs(const int* states, const long long* offsets, int S, int K, int n, int* runs,
                         long long runs_cap, long long* frames, long long* trans, long long* n_runs, long long* bad,
                         void* ws, hipStream_t st) {
    if (!bn_state_runs_ok(n, S, K) || runs_cap < 0) return BN_E_SHAPE;
    if (S == 0) return 0;
    hipLaunchKernelGGL(k_sr_zero, dim3(1), dim3(256), 0, st, frames, trans, K, n_runs, bad);
    BN_LAUNCH_CHECK();
    if (!n) return 0;
    const long tiles = sr_tiles(n);
    int* e = reinterpret_cast<int*>(ws);
    int* counts = reinterpret_cast<int*>(reinterpret_cast<char*>(ws) + sr_offsets_bytes(S));
    int* bases = reinterpret_cast<int*>(reinterpret_cast<char*>(counts) + sr_pad16((size_t)tiles * sizeof(int)));
    const int rc = bn_launch_segment_offsets(offsets, S + 1, n, e, st);
    if (rc) return rc;
    const int vec = (((uintptr_t)states) & 15u) == 0 ? 1 : 0;
    const dim3 grid((unsigned)tiles), block(SR_THREADS);
    hipLaunchKernelGGL(k_sr_count, grid, block, 0, st, states, (const int*)e, S, K, vec, counts, frames, trans, bad);
    BN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sr_scan, dim3(1), block, 0, st, (const int*)counts, tiles, bases, n_runs);
    BN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sr_write, grid, block, 0, st, states, (const int*)e, S, vec, (const int*)bases, runs,
                       runs_cap);
    BN_LAUNCH_CHECK();
    return 0;
}
