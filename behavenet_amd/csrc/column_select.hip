// Exact per-column order statistics of a row-major fp32 table x (n, d), leading dimension ld >= d (DESIGN.md
// section 4, "ranges"): a most-significant-digit radix select over four 8-bit digits.
//
//   key(v) = ~bits(v)               v negative (sign bit set)
//          = bits(v) ^ 0x80000000   otherwise
// orders as the floats do.  Infinities and denormals are ordinary values; a NaN of any sign or payload takes no part.
// -0.0 sorts directly below +0.0, so a selected zero may carry either sign: the two compare equal under ==, which is
// how the tests (and numpy's interpolation) see them.
//
// bn_column_count: one pass counts the NaNs of every column (they are rare, so the LDS adds do not pile up on one
// address), a second launch writes n_valid[j] = n - (the slabs' NaN counts, summed).
//
// bn_column_select, for r rank slots a column: for digit p = 0 .. 3, most significant first,
//   k_cs_hist  streams the table once and counts digit p of every key whose higher digits equal a slot's prefix into
//              that slot's 256-bin LDS histogram; a workgroup owns a block of consecutive rows and a group of
//              columns and stores its histograms to its own slab of the workspace;
//   k_cs_scan  (one workgroup per slot) sums the slot's histogram over the slabs, finds the bin that holds the rank,
//              appends it to the prefix and reduces the rank to the rank inside the bin.
// After the fourth digit the prefix is the key; the last scan converts it back and writes out.  Slots of a column
// that share a prefix share a histogram: the first of them (the "leader") is counted, the others read the leader's.
// Before the first digit all slots share the empty prefix, so the first pass counts one histogram per column; its
// total is the column's number of valid values, against which the ranks are checked (outside -> NaN).
// Counts are integers and every slab is written by exactly one workgroup with plain stores: no global atomics, and
// the result does not depend on the order in which workgroups run.
//
// LDS.  A histogram is 256 uint32 counters = 1 KiB and a column needs r of them.  CS_HISTS = 60 histograms = 60 KiB
// (plus 240 bytes of prefixes) stay under the 64 KiB of static LDS a workgroup may declare and leave room for two
// workgroups on a CU's 160 KiB.  A workgroup therefore takes floor(60 / r) columns: 60 for r = 1, 10 for r = 6 (the
// three percentiles of compute_range), 7 for r = 8.  With d above that the column groups each stream the rows again
// and count their own columns.
//
// The table is read with 16-byte loads from the first 16-byte boundary of a workgroup's rows on (the few elements
// before it and after the last whole vector one by one); an element's column is its flat index modulo ld, carried
// along by additions.  The input is never written.
#include "bn_common.h"
#include "bn_launch.h"

#define CS_THREADS 256
#define CS_BINS 256
#define CS_HISTS 60                // LDS histograms of a workgroup (see "LDS" above)
#define CS_MAX_R 8
#define CS_MAX_D 1024
#define CS_MIN_ELEMS (1 << 16)     // table elements a workgroup streams at least (but for the last row block): 256 KiB
#define CS_TARGET_GROUPS 512       // workgroups the row blocks are cut for: two a CU
#define CS_SCAN_PARTS 4            // k_cs_scan: 4 x 256 threads, each part sums every fourth slab
#define CS_NO_MATCH 0xffffffffu    // "prefix" of a slot that is not counted (no 24-bit prefix equals it)

__device__ __forceinline__ bool cs_is_nan(unsigned b) { return (b & 0x7fffffffu) > 0x7f800000u; }
__device__ __forceinline__ unsigned cs_key(unsigned b) { return (b & 0x80000000u) ? ~b : (b ^ 0x80000000u); }
__device__ __forceinline__ unsigned cs_unkey(unsigned k) { return (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k; }

struct CsPlan {
    int cols;         // columns of a column group
    int col_groups;
    int slabs;        // row blocks
    int rows;         // rows per block (the last block takes what is left)
};

// the ONE partition the workspace query, the launches and the scans go by: a function of (n, d, r) alone
// (r == 0: the count pass, every column in one group)
static CsPlan cs_plan(int n, int d, int r) {
    CsPlan p;
    p.cols = r ? CS_HISTS / r : d;
    if (p.cols > d) p.cols = d;
    p.col_groups = (d + p.cols - 1) / p.cols;
    long for_chip = CS_TARGET_GROUPS / p.col_groups;
    if (for_chip < 1) for_chip = 1;
    long min_rows = CS_MIN_ELEMS / d;
    if (min_rows < 1) min_rows = 1;
    const long by_rows = ((long)n + min_rows - 1) / min_rows;
    const long want = for_chip < by_rows ? for_chip : by_rows;
    p.rows = (int)(((long)n + want - 1) / want);
    p.slabs = (int)(((long)n + p.rows - 1) / p.rows);
    return p;
}

// f(bits, column) for every element of rows [row0, row1) with a column below ld (the caller tells columns >= d apart)
template <class F>
__device__ __forceinline__ void cs_stream(const unsigned* __restrict__ x, long row0, long row1, int d, unsigned ld,
                                          F f) {
    const size_t e0 = (size_t)row0 * ld, e1 = (size_t)(row1 - 1) * ld + (size_t)d;
    const unsigned mis = (unsigned)(((uintptr_t)(x + e0) >> 2) & 3);
    size_t head = mis ? 4 - mis : 0;
    if (head > e1 - e0) head = e1 - e0;
    const size_t v0 = e0 + head;
    const size_t nvec = (e1 - v0) / 4;
    const size_t t0 = v0 + nvec * 4;
    const unsigned tid = threadIdx.x;
    // the elements before the first and after the last whole vector
    if (tid < head) f(x[e0 + tid], (unsigned)((e0 + tid) % ld));
    if (tid < e1 - t0) f(x[t0 + tid], (unsigned)((t0 + tid) % ld));
    if (nvec == 0) return;
    unsigned col = (unsigned)((v0 + 4 * (size_t)tid) % ld);
    const unsigned step = (4 * CS_THREADS) % ld;
    const uint4* __restrict__ xv = reinterpret_cast<const uint4*>(x + v0);
    size_t v = tid;
#define CS_FOUR(q, c0)                                   \
    do {                                                 \
        unsigned c = (c0);                               \
        f((q).x, c); c = c + 1 == ld ? 0 : c + 1;        \
        f((q).y, c); c = c + 1 == ld ? 0 : c + 1;        \
        f((q).z, c); c = c + 1 == ld ? 0 : c + 1;        \
        f((q).w, c);                                     \
    } while (0)
#define CS_NEXT(c) ((c) + step >= ld ? (c) + step - ld : (c) + step)
    // four loads in flight
    for (; v + 3 * CS_THREADS < nvec; v += 4 * CS_THREADS) {
        const uint4 q0 = xv[v], q1 = xv[v + CS_THREADS], q2 = xv[v + 2 * CS_THREADS], q3 = xv[v + 3 * CS_THREADS];
        const unsigned c1 = CS_NEXT(col), c2 = CS_NEXT(c1), c3 = CS_NEXT(c2);
        CS_FOUR(q0, col);
        CS_FOUR(q1, c1);
        CS_FOUR(q2, c2);
        CS_FOUR(q3, c3);
        col = CS_NEXT(c3);
    }
    for (; v < nvec; v += CS_THREADS) {
        const uint4 q = xv[v];
        CS_FOUR(q, col);
        col = CS_NEXT(col);
    }
#undef CS_FOUR
#undef CS_NEXT
}

// ------------------------------------------------------------------------------------------------------------
// count: part[b][j] = NaNs of column j in row block b
__global__ __launch_bounds__(CS_THREADS) void k_cs_count(const unsigned* __restrict__ x, int n, int d, unsigned ld,
                                                         int rows, unsigned* __restrict__ part) {
    __shared__ unsigned nans[CS_MAX_D];
    for (int j = threadIdx.x; j < d; j += CS_THREADS) nans[j] = 0;
    __syncthreads();
    const long row0 = (long)blockIdx.x * rows;
    const long row1 = row0 + rows < n ? row0 + rows : n;
    cs_stream(x, row0, row1, d, ld, [&](unsigned bits, unsigned c) {
        if (c < (unsigned)d && cs_is_nan(bits)) atomicAdd(&nans[c], 1u);
    });
    __syncthreads();
    for (int j = threadIdx.x; j < d; j += CS_THREADS) part[(size_t)blockIdx.x * d + j] = nans[j];
}

__global__ __launch_bounds__(CS_THREADS) void k_cs_count_finish(const unsigned* __restrict__ part, int n, int d,
                                                                int slabs, long long* __restrict__ n_valid) {
    const int j = blockIdx.x * CS_THREADS + threadIdx.x;
    if (j >= d) return;
    long long nan = 0;
    for (int b = 0; b < slabs; ++b) nan += part[(size_t)b * d + j];
    n_valid[j] = (long long)n - nan;
}

// ------------------------------------------------------------------------------------------------------------
// The slots' state between the digits, two copies (digit p reads copy (p - 1) & 1 and writes copy p & 1: a scan
// workgroup reads its column's other slots while theirs write).  Slot (j, s) sits at j * r + s.
struct CsState {
    unsigned* prefix;      // the digits found so far
    long long* rem;        // the rank among the keys that share the prefix; < 0: the rank was outside the column
};

__device__ __forceinline__ CsState cs_state(void* ws, int copy, int slots) {
    CsState s;
    s.rem = reinterpret_cast<long long*>(ws) + (size_t)copy * slots;
    s.prefix = reinterpret_cast<unsigned*>(reinterpret_cast<long long*>(ws) + 2 * (size_t)slots) + (size_t)copy * slots;
    return s;
}

// bytes of the two copies, rounded to the 16-byte boundary the slabs start on
static size_t cs_state_bytes(int d, int r) { return (((size_t)d * r * 2 * (sizeof(long long) + sizeof(unsigned))) + 15) & ~(size_t)15; }

// the slot that slot (j, s) reads its histogram from: the first valid slot of the column with the same prefix
__device__ __forceinline__ int cs_leader(const CsState& st, int j, int s, int r) {
    const unsigned mine = st.prefix[j * r + s];
    for (int k = 0; k < s; ++k)
        if (st.rem[j * r + k] >= 0 && st.prefix[j * r + k] == mine) return k;
    return s;
}

// digit P (0: most significant) of the keys of columns [c0, c0 + cols) in rows [row0, row1) -> slab blockIdx / groups
template <bool FIRST>
__global__ __launch_bounds__(CS_THREADS) void k_cs_hist(const unsigned* __restrict__ x, int n, int d, unsigned ld,
                                                        int r, int pass, int rows, int cols, int col_groups,
                                                        void* __restrict__ ws, size_t state_bytes) {
    __shared__ unsigned hist[CS_HISTS * CS_BINS];
    __shared__ unsigned match[CS_HISTS];
    const int b = blockIdx.x / col_groups, g = blockIdx.x - b * col_groups;
    const int c0 = g * cols;
    const int nc = c0 + cols <= d ? cols : d - c0;
    const int nh = nc * r;                                 // <= CS_HISTS
    for (int i = threadIdx.x; i < nh * CS_BINS; i += CS_THREADS) hist[i] = 0;
    if (!FIRST && (int)threadIdx.x < nh) {
        const CsState st = cs_state(ws, (pass - 1) & 1, d * r);
        const int j = c0 + (int)threadIdx.x / r, s = (int)threadIdx.x % r;
        const bool counted = st.rem[j * r + s] >= 0 && cs_leader(st, j, s, r) == s;
        match[threadIdx.x] = counted ? st.prefix[j * r + s] : CS_NO_MATCH;
    }
    __syncthreads();
    const long row0 = (long)b * rows;
    const long row1 = row0 + rows < n ? row0 + rows : n;
    const int shift = 24 - 8 * pass;
    cs_stream(x, row0, row1, d, ld, [&](unsigned bits, unsigned c) {
        const unsigned cr = c - (unsigned)c0;              // (columns below c0 wrap to large values)
        if (cr >= (unsigned)nc || cs_is_nan(bits)) return;
        const unsigned key = cs_key(bits);
        if (FIRST) {
            atomicAdd(&hist[(cr * r) * CS_BINS + (key >> 24)], 1u);
        } else {
            const unsigned hi = key >> (shift + 8), digit = (key >> shift) & 255u;
            for (int s = 0; s < r; ++s)
                if (match[cr * r + s] == hi) atomicAdd(&hist[(cr * r + s) * CS_BINS + digit], 1u);
        }
    });
    __syncthreads();
    // the slab of row block b: (d r) histograms; this workgroup's are [c0 r, c0 r + nh)
    uint4* dst = reinterpret_cast<uint4*>(reinterpret_cast<char*>(ws) + state_bytes) +
                 ((size_t)b * d * r + (size_t)c0 * r) * (CS_BINS / 4);
    const uint4* src = reinterpret_cast<const uint4*>(hist);
    for (int i = threadIdx.x; i < nh * (CS_BINS / 4); i += CS_THREADS) dst[i] = src[i];
}

// one workgroup per slot: thread (part, bin) sums its bin over the slabs part, part + 4, ...
__global__ __launch_bounds__(CS_SCAN_PARTS * CS_BINS) void k_cs_scan(void* __restrict__ ws, size_t state_bytes,
                                                                     int d, int r, int slabs, int pass,
                                                                     const long long* __restrict__ ranks,
                                                                     float* __restrict__ out) {
    __shared__ unsigned part[CS_SCAN_PARTS][CS_BINS];
    __shared__ unsigned incl[2][CS_BINS];
    const int slot = blockIdx.x, j = slot / r, s = slot - j * r;
    const int bin = threadIdx.x & (CS_BINS - 1), q = threadIdx.x / CS_BINS;
    const bool last = pass == 3;
    const CsState in = cs_state(ws, (pass - 1) & 1, d * r), to = cs_state(ws, pass & 1, d * r);
    unsigned prefix = 0;
    long long rem;
    int leader = 0;
    if (pass == 0) {
        rem = ranks[(size_t)s * d + j];
    } else {
        prefix = in.prefix[slot];
        rem = in.rem[slot];
        if (rem < 0) {                                     // (the whole workgroup: rem is the slot's)
            if (threadIdx.x == 0) {
                to.prefix[slot] = prefix;
                to.rem[slot] = -1;
                if (last) out[(size_t)s * d + j] = __uint_as_float(0x7fc00000u);
            }
            return;
        }
        leader = cs_leader(in, j, s, r);
    }
    const unsigned* slab0 = reinterpret_cast<const unsigned*>(reinterpret_cast<const char*>(ws) + state_bytes) +
                            ((size_t)j * r + leader) * CS_BINS + bin;
    const size_t slab_stride = (size_t)d * r * CS_BINS;
    unsigned sum = 0;
#pragma unroll 8
    for (int b = q; b < slabs; b += CS_SCAN_PARTS) sum += slab0[(size_t)b * slab_stride];
    part[q][bin] = sum;
    __syncthreads();
    // inclusive scan of the 256 bins (a column holds fewer than 2^31 values: uint32 does not wrap)
    unsigned h = 0;
    if (q == 0) {
        h = part[0][bin] + part[1][bin] + part[2][bin] + part[3][bin];
        incl[0][bin] = h;
    }
    __syncthreads();
    int cur = 0;
    for (int off = 1; off < CS_BINS; off <<= 1) {
        if (q == 0) incl[cur ^ 1][bin] = incl[cur][bin] + (bin >= off ? incl[cur][bin - off] : 0u);
        __syncthreads();
        cur ^= 1;
    }
    if (q != 0) return;
    const long long above = (long long)incl[cur][bin], below = above - (long long)h;
    const long long total = (long long)incl[cur][CS_BINS - 1];
    if (rem < 0 || rem >= total) {                         // outside the column (first digit: total = n_valid)
        if (bin == 0) {
            to.prefix[slot] = prefix;
            to.rem[slot] = -1;
            if (last) out[(size_t)s * d + j] = __uint_as_float(0x7fc00000u);
        }
        return;
    }
    if (below <= rem && rem < above) {                     // exactly one bin
        const unsigned now = (prefix << 8) | (unsigned)bin;
        to.prefix[slot] = now;
        to.rem[slot] = rem - below;
        if (last) out[(size_t)s * d + j] = __uint_as_float(cs_unkey(now));
    }
}

// ------------------------------------------------------------------------------------------------------------
bool bn_column_select_ok(int n, int d, int ld, int r) {
    return n >= 1 && d >= 1 && d <= CS_MAX_D && ld >= d && r >= 1 && r <= CS_MAX_R;
}

static size_t cs_count_bytes(int n, int d) { return (size_t)cs_plan(n, d, 0).slabs * d * sizeof(unsigned); }

size_t bn_column_count_ws_bytes_impl(int n, int d) {
    if (!bn_column_select_ok(n, d, d, 1)) return 0;
    return cs_count_bytes(n, d);
}

size_t bn_column_select_ws_bytes_impl(int n, int d, int r) {
    if (!bn_column_select_ok(n, d, d, r)) return 0;
    const size_t select = cs_state_bytes(d, r) + (size_t)cs_plan(n, d, r).slabs * d * r * CS_BINS * sizeof(unsigned);
    const size_t count = cs_count_bytes(n, d);
    return select > count ? select : count;               // (one workspace serves both entry points)
}

int bn_launch_column_count(const float* x, int n, int d, int ld, long long* n_valid, void* ws, hipStream_t st) {
    if (!bn_column_select_ok(n, d, ld, 1)) return BN_E_SHAPE;
    const CsPlan p = cs_plan(n, d, 0);
    hipLaunchKernelGGL(k_cs_count, dim3((unsigned)p.slabs), dim3(CS_THREADS), 0, st, (const unsigned*)x, n, d,
                       (unsigned)ld, p.rows, (unsigned*)ws);
    BN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_cs_count_finish, dim3((unsigned)((d + CS_THREADS - 1) / CS_THREADS)), dim3(CS_THREADS), 0, st,
                       (const unsigned*)ws, n, d, p.slabs, n_valid);
    BN_LAUNCH_CHECK();
    return 0;
}

int bn_launch_column_select(const float* x, int n, int d, int ld, const long long* ranks, int r, float* out, void* ws,
                            hipStream_t st) {
    if (!bn_column_select_ok(n, d, ld, r)) return BN_E_SHAPE;
    const CsPlan p = cs_plan(n, d, r);
    const size_t state_bytes = cs_state_bytes(d, r);
    const dim3 grid((unsigned)(p.slabs * p.col_groups));
    for (int pass = 0; pass < 4; ++pass) {
        if (pass == 0)
            hipLaunchKernelGGL((k_cs_hist<true>), grid, dim3(CS_THREADS), 0, st, (const unsigned*)x, n, d, (unsigned)ld,
                               r, pass, p.rows, p.cols, p.col_groups, ws, state_bytes);
        else
            hipLaunchKernelGGL((k_cs_hist<false>), grid, dim3(CS_THREADS), 0, st, (const unsigned*)x, n, d,
                               (unsigned)ld, r, pass, p.rows, p.cols, p.col_groups, ws, state_bytes);
        BN_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_cs_scan, dim3((unsigned)(d * r)), dim3(CS_SCAN_PARTS * CS_BINS), 0, st, ws, state_bytes, d,
                           r, p.slabs, pass, ranks, out);
        BN_LAUNCH_CHECK();
    }
    return 0;
}
