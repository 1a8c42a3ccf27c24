// EM for autoregressive hidden Markov models on a table of latents ("ARHMM"): the four launches
// of one EM iteration and of the state export.  The table z is fp32 (n, D); everything else is float64.  The rows are
// cut into trials by offsets made safe as segment_sums.hip makes them (bn_launch_segment_offsets: clamped into [0, n]
// and non-decreasing); rows outside [e[0], e[S]) belong to no trial and are neither read nor written by any launch.
// Row t of a trial (counted from the trial's first row) is an INITIAL row if t < L and an AR row otherwise; for an AR
// row
//
//   a_t = (1, x_t - c, x_{t-1} - c, ..., x_{t-L} - c)        float64, P = 1 + (L + 1) D entries, c the shift or zeros
//
// k_ar_kind      one byte a row: 0 outside the trials, 1 initial, 2 AR (a binary search in the offsets a row; the
//                staging loops of the two table kernels read the byte, not the offsets)
// k_ar_loglik    ll[t][k] = cst[k] - 1/2 |G_k a_t|^2 for AR rows: the (n x P) (P x K D) product on
//                v_mfma_f64_16x16x4_f64.  A wave takes 32 rows (two row tiles of 16, staged in LDS as float64 rows
//                a_t, zeros for the rows that are not AR rows and for the padding of P to a multiple of four).  The
//                tile COLUMNS are states (16 a tile) and the D output dimensions are taken one after the other: the
//                MFMA chain over P for dimension d leaves (G_k a_t)[d] for 16 rows x 16 states, which is squared and
//                added into the lane's own four sums -- the squared norm over D needs no cross-lane step.  B comes
//                straight from G (at most 1 MiB, resident in L2).  Initial rows: -D/2 log 2 pi - 1/2 |x_t|^2 for
//                every state, one lane a row.  A NaN in row t is in the staged rows a_t .. a_{t+L} of its trial and
//                nowhere else, and a row of A reaches its own row of the product only.
// k_hmm_fb       forward-backward, one wave (one workgroup of 64) a trial.  Lane j is state j; it keeps column j of
//                P = exp(logP) in registers for the forward sweep and row j for the backward sweep.  The K values of
//                the step before reach every lane through LDS: one write, one barrier, K broadcast reads (double
//                buffered, so one barrier a step).  Scaled recursion: b_t = exp(ll_t - max_k ll_t), u_t[j] =
//                sum_i ahat_{t-1}[i] P[i][j] b_t[j], s_t = sum_j u_t[j], ahat_t = u_t / s_t and
//                loglik = sum_t (log s_t + max_t); the division by s_t is done by the readers of the next step (they
//                sum the K values they read anyway), and log s_t is taken once per 64 steps: lane (t & 63) keeps s_t
//                and all lanes take one log when the 64 are full.  Row maximum and exp of row t + 1 are formed
//                during step t and row t + 2 is asked for then, in both sweeps.  gamma's storage holds ahat between the sweeps; the
//                workspace holds (s_t, max_t) a row.  Backward: v_t[j] = b_t[j] bhat_t[j] / s_t, bhat_t[i] =
//                sum_j P[i][j] v_{t+1}[j], xi += ahat_t[i] P[i][j] v_{t+1}[j] and gamma_t = ahat_t bhat_t, divided
//                by its own sum over the states (read from LDS with v).  The sums over states run in state order in
//                four interleaved accumulators: the same bits on every call.
// k_ar_moments   out[k] = sum_t gamma[t][k] a_t^T a_t over the AR rows: segment_gram.hip's scheme (32 staged rows,
//                four waves taking the k-steps in turn, tiles with ti <= tj only and mirrored on the way out) with
//                the weight folded into the A fragment.  The grid is (row blocks, state groups): a workgroup stages
//                its rows ONCE for a group of 4, 2 or 1 states (by the registers 2 TB (TB + 1) accumulators a state
//                leave) and leaves one (P, P) partial a state, k_ar_combine adds the partials in block order.  The 1
//                of a_t is a column of the product like the others, so out[k][0][0] is the sum of the weights.
// k_ar_gamma0    the sum of gamma over the initial rows, one workgroup a state, in (thread, trial) order.
// k_hmm_viterbi  max-sum, one wave a trial, the lane layout of k_hmm_fb; uint8 back-pointers (n, K) in the workspace;
//                a tie goes to the lowest state (strict > in ascending order).  The walk back runs on lane 0 over
//                64 rows of back-pointers at a time, copied into LDS by the whole wave.
// Sampling (bn_arhmm_sample; the caller brings the noise, no random number is drawn here):
// k_ars_states   the state chain of a trial from its uniforms, one wave a trial.  The K cumulative rows and cdf0 sit
//                in LDS; lane j < K - 1 compares u_t with entry j of row z_{t-1} and the state is the number of lanes
//                that say u_t >= cdf (a ballot and a bit count: comparisons only, the host's path bit for bit).  64
//                uniforms are staged a time and lane i keeps the state of the chunk's row i, so the stores coalesce.
//                The wave walks every row of its trial, so it leaves the trial's number a row in the workspace too.
// k_ars_given    given states: copied out, one wave a trial, with the trial's number a row, and the first row whose
//                state is outside [0, K) is left in the workspace (INT_MAX for none, which k_ars_states writes).
// k_ars_drive    every row at once, one thread an element (the row's trial is in the workspace: no search): NaN from
//                the trial's first bad state on, init or eps for an initial row, else v_t = b_z + C_z eps_t (j
//                ascending, one FMA a term), written into x.  It reads C transposed (k_ars_transpose, into the
//                workspace): the threads of a row then read neighbouring doubles where the rows of C_z lie D apart
//                (measured on 4.8 10^6 x 16: 3.0 ms with C as it comes, one cache line a lane and load).
// k_ars_recur    x_t = v_t + sum_l A_z[l] x_{t-1-l}, one wave a trial, L > 0 only.  A window of 64 rows of v and the L
//                rows before it sit in LDS and the rows are finished in place, so a step reads and writes LDS only
//                and the window leaves in one coalesced sweep.  Lane (d, p) = (lane / NP, lane % NP) takes the
//                history entries p, p + NP, ... of output row d (NP = 8, 4, 2 for D up to 8, 16, 32) in ascending
//                order; the NP partial sums of a row are neighbours and are added by DPP moves (xor 1, xor 2, the
//                other half of eight): a fixed tree, the same bits on every call.  Row z of A comes from global
//                memory (L2) into registers one step ahead, and only when the state changes.
// A GRID of models on one table (bn_arhmm_grid_*, bn_hmm_grid_forward_backward): M models with the same D and L, their
// states side by side as KT = sum K_m columns of G, cst, ll and gamma (model m: columns koff[m] .. koff[m + 1]).
// k_ar_loglik and k_ar_moments take the KT columns as they take K: full 16-state tiles and whole state groups, the
// table read once for all models, ar_plan's row blocks growing as the KT partials of a block grow.
// k_hmm_gfb      forward-backward for the grid, one wave a (trial, 64 / KP models of one CLASS KP = 4, 8, 16, 32 --
//                the smallest that holds K_m).  The wave is cut into SLOTS of KP lanes; lane slot * KP + j is state j
//                of the slot's model, and the recursion inside a slot is k_hmm_fb's, with everything that was
//                wave-wide made slot-wide: the row maximum is a butterfly over the slot's KP lanes (xor KP / 2 .. 1),
//                the broadcast reads go to the slot's own KP doubles in LDS, s_t is kept by lane (t % KP) of the slot
//                with one log per KP steps, and the final sum is a butterfly over the slot.  No value crosses a slot's
//                boundary, so a model's bits do not depend on its slot or on its neighbours, and a NaN stays in its
//                model.  A padding state (j >= K_m) and an empty slot carry probability zero and write nothing.
//                One launch a class, the grid (trials, waves of the class); (s_t, max_t) a (model, row) in the
//                workspace.
// k_hmm_gviterbi max-sum for the grid (bn_hmm_grid_viterbi): k_hmm_gfb's packing -- the same order, counts, koff, xoff
//                and empty-slot rules, one launch a class -- and k_hmm_viterbi's arithmetic term for term inside a
//                slot: delta = best + ll, predecessors in ascending order with strict >, the last row's argmax the
//                same, the slot's KP deltas read from its own KP doubles in LDS (double buffered, one barrier a step).
//                A model's path has k_hmm_viterbi's integers wherever it sits.  uint8 back-pointers at
//                bp[row * KT + koff[m] + j] in the workspace; every lane reads back only bytes it wrote itself.  The
//                walk back takes all slots at once: 64 rows of the wave's 64 back-pointer bytes are staged in LDS
//                (4 KiB), the first lane of every slot walks its own chain and leaves the chunk's states in LDS, and
//                the wave writes them slot after slot as states[m * n + row], neighbouring lanes on neighbouring rows.
// One-step-ahead predictions (bn_hmm_predictive, bn_arhmm_predict):
// k_hmm_pred     the causal weights w_t = p(z_t | x_0 .. x_{t-1}), one wave a trial: k_hmm_fb's forward sweep (the same
//                lane layout, LDS exchange and scaling) with ONE store added and the likelihood left out.  The readers
//                of step t form dot[j] = sum_i u_t[i] P[i][j] / sum_i u_t[i] anyway; that is w_{t+1}[j], written before
//                row t + 1 of ll enters (w_0 = exp(logpi0)), so row t of ll never reaches w_t.  The last step is not
//                run: nobody reads it.
// k_arp_fold     W (K, D, Q), Q = 1 + L D, into the workspace as the B operand wt[j][d], j = k Q + q: JP = K Q padded
//                to a multiple of 16 rows of DP = D padded to a multiple of 16 doubles, zeros in the padding, so
//                the B loads of k_ar_predict are whole tile rows (128 B a k-index) and need no bounds.
// k_ar_predict   xhat_t = sum_k w_t[k] (b_k + sum_l A_k[l] x_{t-1-l}) for AR rows: the (n x K Q) (K Q x D) product on
//                v_mfma_f64_16x16x4_f64.  A wave takes 32 rows (two row tiles of 16); phi_t = (1, x_{t-1}, ..,
//                x_{t-L}) is staged in LDS as float64 rows as k_ar_loglik stages a_t, and the rows' K weights beside
//                them (zeros for the rows that are not AR rows).  The A entry (row, j = k Q + q) is w[k] phi[q], the
//                weight folded into the fragment as k_ar_moments folds gamma; lane (col, kk) walks j = kk, kk + 4,
//                ... with k = j / Q by the fp32 reciprocal (exact for these sizes), four B loads in flight.  The tile COLUMNS are the output dimensions d (16 a
//                tile, D / 16 tiles one after the other): the chain over j leaves xhat for 16 rows x 16 dimensions in
//                the accumulators, no cross-lane step.  Initial rows get the row's own values, one lane a row.  A NaN
//                in row t is in the staged rows phi_{t+1} .. phi_{t+L} of its trial and nowhere else, and a row of A
//                reaches its own row of the product only.
// Multi-step forecasts (bn_arhmm_forecast_sums): E[x_{t+h-1} | x_0 .. x_{t-1}] = sum_k w_t[k] N_h[k] phi_t, h = 1 .. H,
// scored in the epilogue; the (n, H, D) forecasts never go to memory.
// k_arf_plan     the row blocks, none across a trial boundary: trial s has its origin rows beg + max(L, 1) .. end - 1
//                cut
//                into blocks of AR_FC_BLOCK_ROWS; first[s] is the exclusive prefix sum of the blocks per trial (one
//                workgroup, thread i the trials of chunk i, 256 chunk sums added in thread order).
// k_arf_fold     N (H, K, D, Q) into the B operand bt[j][c], j = k Q + q, c = (h - 1) D + d (the horizons packed, no
//                padding between them): JP = K Q padded to 16 rows of CP = H D padded to AR_FC_COLS doubles, zeros in
//                the padding.
// k_ar_forecast  a workgroup (x, y) takes row block x and the column group y of AR_FC_CT = 4 column tiles (64 columns
//                (h, d); four horizons at D = 16).  A wave takes 32 origin rows at a time, staged as k_ar_predict
//                stages
//                them; the A entry w[k] phi[q] of a k-step is formed ONCE and feeds the 2 x 4 accumulator tiles of the
//                group, four B loads a k-step.  The group is register-bound: 2 x 4 tiles x 8 VGPRs of accumulators and
//                5 x 4 x 2 of running sums are 104 registers before any address or operand, and the compiler ends at
//                238 (two waves a SIMD); eight tiles would pass 256 and leave one.  With four, eight MFMAs follow the
//                two LDS reads and the multiply of every A entry where k_ar_predict at D = 16 issues two.  The last
//                group's tiles without a column (H D not a multiple of 64) are skipped, the same for the workgroup.
//                Epilogue: lane (col, kk) owns column c and the rows kk + 4 r; the target y = x_{t+h-1} and x_{t-1} are
//                read as fp32 and widened, the five terms formed in float64 and kept only where t + h - 1 < end.  The
//                lane adds its rows in row order, the four lanes of a column by two exchanges, the two waves through
//                LDS in wave order: one (columns, 5) partial a block.
// k_arf_combine  sums[h][s][d][term] = the partials of trial s added in block order; zeros for a trial without blocks.
// No global atomics; every output element is written exactly once by each kernel that owns it.
#include <limits.h>
#include <math.h>
#include "bn_common.h"
#include "bn_launch.h"

#define AR_MAX_K 32
#define AR_MAX_L 8
#define AR_MAX_LD 64                        // (L + 1) D at most
#define AR_LL_THREADS 128                   // k_ar_loglik: two waves ...
#define AR_LL_WAVES (AR_LL_THREADS / BN_WAVE)
#define AR_LL_ROWS 32                       // ... of 32 rows (two row tiles) each
#define AR_LL_LW 72                         // doubles a staged row at most: P <= 65 padded to 68, plus 4
#define AR_MO_THREADS 256
#define AR_MO_WAVES (AR_MO_THREADS / BN_WAVE)
#define AR_MO_ROWS 32                       // rows of a staged chunk: eight k-steps of four rows, two a wave
#define AR_MO_MIN_ROWS 512                  // rows a row block holds at least (but for the last)
#define AR_MO_TARGET_BLOCKS 1024            // row blocks at most ...
#define AR_MO_SLAB_BYTES (60u << 20)        // ... and no more than fit K partials each into 60 MiB
#define AR_BT_ROWS 64                       // rows of back-pointers the walk back holds in LDS
#define AR_S_ROWS 64                        // sampling: rows of a window (k_ars_recur), uniforms of a chunk
#define AR_S_MAX_D 32                       // D at most where L > 0
#define AR_GRID_MAX_KT 512                  // a grid of models: states of all models together at most ...
#define AR_GRID_MAX_M 512                   // ... and models
#define AR_PR_THREADS 128                   // k_ar_predict: two waves ...
#define AR_PR_WAVES (AR_PR_THREADS / BN_WAVE)
#define AR_PR_ROWS 32                       // ... of 32 rows (two row tiles) each
#define AR_FC_MAX_H 32                      // k_ar_forecast: horizons at most
#define AR_FC_THREADS 128                   // two waves ...
#define AR_FC_WAVES (AR_FC_THREADS / BN_WAVE)
#define AR_FC_ROWS 32                       // ... of 32 origin rows (two row tiles) at a time
#define AR_FC_BLOCK_ROWS 256                // origin rows of a row block at most, all of one trial
#define AR_FC_CT 4                          // column tiles of a column group ...
#define AR_FC_COLS (16 * AR_FC_CT)          // ... and its columns (h, d)
#define AR_FC_TERMS 5                       // count, sum y, sum y^2, sum (y - xhat)^2, sum (y - x_{t-1})^2

typedef double ar_d4 __attribute__((ext_vector_type(4)));

struct ArPlan {
    int blocks;       // row blocks
    int rows;         // rows per block (the last block takes what is left)
};

static bool ar_dims_ok(int D, int L, int K, int max_k = AR_MAX_K) {
    return K >= 1 && K <= max_k && L >= 0 && L <= AR_MAX_L && D >= 1 && (L + 1) * (long)D <= AR_MAX_LD;
}

// the ONE partition of k_ar_moments the workspace query, the launch and the combine go by
static ArPlan ar_plan(int n, int D, int L, int K) {
    ArPlan p;
    if (n < 1) {
        p.blocks = 0;
        p.rows = 1;
        return p;
    }
    const long P = 1 + (long)(L + 1) * D;
    const long by_bytes = AR_MO_SLAB_BYTES / ((long)K * P * P * (long)sizeof(double));       // 58 at K = 32, P = 65
    const long cap = by_bytes < AR_MO_TARGET_BLOCKS ? by_bytes : AR_MO_TARGET_BLOCKS;
    const long by_rows = ((long)n + AR_MO_MIN_ROWS - 1) / AR_MO_MIN_ROWS;
    const long want = by_rows < cap ? by_rows : cap;
    p.rows = (int)(((long)n + want - 1) / want);
    p.blocks = (int)(((long)n + p.rows - 1) / p.rows);
    return p;
}

static size_t ar_pad16(size_t b) { return (b + 15) & ~(size_t)15; }
static size_t ar_offsets_bytes(int S) { return ar_pad16(((size_t)S + 1) * sizeof(int)); }

// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ar_kind(const int* __restrict__ e, int S, int L, int n,
                                                 unsigned char* __restrict__ kind) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    unsigned char v = 0;
    if (r >= e[0] && r < e[S]) {
        int lo = 0, hi = S - 1;                            // the first trial that ends after r
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (e[mid + 1] > r) hi = mid; else lo = mid + 1;
        }
        v = r - e[lo] < L ? 1 : 2;
    }
    kind[r] = v;
}

// the staged entry p of a_t for the AR row `row` (p < P)
__device__ __forceinline__ double ar_entry(const float* __restrict__ z, int ld, const double* shift, int D, long row,
                                           int p) {
    if (p == 0) return 1.0;
    const int q = p - 1, lag = q / D, j = q - lag * D;
    return (double)z[(size_t)(row - lag) * ld + j] - shift[j];
}

__global__ __launch_bounds__(AR_LL_THREADS) void k_ar_loglik(const float* __restrict__ z, int ld,
                                                             const double* __restrict__ c,
                                                             const unsigned char* __restrict__ kind, int D, int L,
                                                             int K, int n, const double* __restrict__ G,
                                                             const double* __restrict__ cst, double* __restrict__ ll) {
    __shared__ double stage[AR_LL_WAVES][AR_LL_ROWS * AR_LL_LW];
    __shared__ double shift[AR_MAX_LD];
    const int tid = threadIdx.x, lane = tid & (BN_WAVE - 1), wave = tid / BN_WAVE;
    const int kk = lane >> 4, col = lane & 15;
    const int P = 1 + (L + 1) * D, PP = (P + 3) & ~3, LW = PP + 4, KS = PP >> 2;
    const long row0 = ((long)blockIdx.x * AR_LL_WAVES + wave) * AR_LL_ROWS;
    double* st = stage[wave];

    if (tid < D) shift[tid] = c ? c[tid] : 0.0;
    __syncthreads();
    for (int idx = lane; idx < AR_LL_ROWS * PP; idx += BN_WAVE) {
        const int r = idx / PP, p = idx - r * PP;
        const long row = row0 + r;
        double v = 0.0;
        if (row < n && p < P && kind[row] == 2) v = ar_entry(z, ld, shift, D, row, p);
        st[r * LW + p] = v;
    }
    __syncthreads();

    for (int kt = 0; kt * 16 < K; ++kt) {
        const int state = kt * 16 + col;
        const bool live = state < K;
        ar_d4 q0 = {0.0, 0.0, 0.0, 0.0}, q1 = {0.0, 0.0, 0.0, 0.0};
        for (int d = 0; d < D; ++d) {
            const double* g = G + ((size_t)(live ? state : 0) * D + d) * P;
            ar_d4 c0 = {0.0, 0.0, 0.0, 0.0}, c1 = {0.0, 0.0, 0.0, 0.0};
            for (int ks = 0; ks < KS; ++ks) {
                const int p = 4 * ks + kk;
                // A: row `col` of the tile, entry p; B: entry p of row d of G_state
                const double b = live && p < P ? g[p] : 0.0;
                const double a0 = st[col * LW + p], a1 = st[(16 + col) * LW + p];
                c0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b, c0, 0, 0, 0);
                c1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b, c1, 0, 0, 0);
            }
            q0 += c0 * c0;
            q1 += c1 * c1;
        }
        // C/D of the f64 MFMA: column lane & 15 (the state), row (lane >> 4) + 4 * reg
        if (live) {
            const double cs = cst[state];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long ra = row0 + kk + 4 * r, rb = ra + 16;
                if (ra < n && kind[ra] == 2) ll[(size_t)ra * K + state] = cs - 0.5 * q0[r];
                if (rb < n && kind[rb] == 2) ll[(size_t)rb * K + state] = cs - 0.5 * q1[r];
            }
        }
    }
    // the initial rows: the standard normal density of the row, the same for every state
    if (lane < AR_LL_ROWS) {
        const long row = row0 + lane;
        if (row < n && kind[row] == 1) {
            double s = 0.0;
            for (int j = 0; j < D; ++j) {
                const double x = (double)z[(size_t)row * ld + j];
                s += x * x;
            }
            const double v = -0.5 * D * 1.8378770664093453 - 0.5 * s;          // log 2 pi
            for (int k = 0; k < K; ++k) ll[(size_t)row * K + k] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double ar_wave_max(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

__device__ __forceinline__ double ar_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <int KP>
__global__ __launch_bounds__(BN_WAVE) void k_hmm_fb(const double* __restrict__ ll, const int* __restrict__ e, int K,
                                                    const double* __restrict__ logP,
                                                    const double* __restrict__ logpi0, int want,
                                                    double* __restrict__ gamma, double* __restrict__ xi,
                                                    double* __restrict__ loglik, double* __restrict__ cm) {
    __shared__ __attribute__((aligned(16))) double buf[2][2][KP];              // [parity][v or g][state]
    const int s = blockIdx.x, lane = threadIdx.x;
    const int beg = e[s], T = e[s + 1] - beg;
    const bool active = lane < K, writer = lane < KP;
    if (T <= 0) {
        if (lane == 0) loglik[s] = 0.0;
        if (want)
            for (int o = lane; o < K * K; o += BN_WAVE) xi[(size_t)s * K * K + o] = 0.0;
        return;
    }
    const double* l = ll + (size_t)beg * K;
    double* gam = gamma + (size_t)beg * K;
    double* cmt = cm + (size_t)beg * 2;
    const double ninf = -INFINITY;

    double Pc[KP];
#pragma unroll
    for (int i = 0; i < KP; ++i) Pc[i] = active && i < K ? exp(logP[i * K + lane]) : 0.0;
    const double pi = active ? exp(logpi0[lane]) : 0.0;

    double lsum = 0.0, msum = 0.0, pend = 1.0, dot = 0.0;
    // the row maximum and exp of row t + 1 are formed during step t and the row t + 2 is asked for then: only
    // u -> LDS -> sums -> division is on the chain from step to step
    double m, b;
    {
        const double lv = active ? l[lane] : ninf;
        m = ar_wave_max(lv);
        b = active ? exp(lv - m) : 0.0;
    }
    double l1 = active && T > 1 ? l[(size_t)K + lane] : ninf;
    for (int t = 0; t < T; ++t) {
        const double l2 = active && t + 2 < T ? l[(size_t)(t + 2) * K + lane] : ninf;
        const double u = t == 0 ? pi * b : dot * b;
        const int par = t & 1;
        if (writer) buf[par][0][lane] = u;
        __syncthreads();
        const double mn = ar_wave_max(l1);
        const double bn = active ? exp(l1 - mn) : 0.0;     // (row T: -inf - -inf, a NaN nobody reads)
        double s4[4] = {0.0, 0.0, 0.0, 0.0}, d4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < KP; ++i) {
            const double ui = buf[par][0][i];
            s4[i & 3] += ui;
            d4[i & 3] += ui * Pc[i];
        }
        const double st = (s4[0] + s4[1]) + (s4[2] + s4[3]);
        const double inv = 1.0 / st;
        dot = ((d4[0] + d4[1]) + (d4[2] + d4[3])) * inv;
        if (want) {
            if (active) gam[(size_t)t * K + lane] = u * inv;
            if (lane == 0) {
                cmt[2 * (size_t)t] = st;
                cmt[2 * (size_t)t + 1] = m;
            }
        }
        msum += m;
        pend = lane == (t & 63) ? st : pend;
        if ((t & 63) == 63) {
            lsum += log(pend);
            pend = 1.0;
        }
        m = mn;
        b = bn;
        l1 = l2;
    }
    lsum += log(pend);
    const double total = ar_wave_sum(lsum) + msum;
    if (lane == 0) loglik[s] = total;
    if (!want) return;

    // ---- backward: gamma holds ahat, cm holds (s_t, max_t); lane i is the SOURCE state now
    __syncthreads();                                       // (cm, written by lane 0, is read by every lane)
    double Pr[KP], acc[KP];
#pragma unroll
    for (int j = 0; j < KP; ++j) {
        Pr[j] = active && j < K ? exp(logP[lane * K + j]) : 0.0;
        acc[j] = 0.0;
    }
    int par = 0;
    {
        const int t = T - 1;
        const double b = active ? exp(l[(size_t)t * K + lane] - cmt[2 * (size_t)t + 1]) : 0.0;
        if (writer) buf[par][0][lane] = b / cmt[2 * (size_t)t];
        __syncthreads();
    }
    // row t's ahat and b_t / s_t are ready when step t begins: b_{t-1} / s_{t-1} is formed during step t from the
    // values asked for during step t + 1, and row t - 2 is asked for
    double a = 0.0, bq = 0.0, a1 = 0.0, q1 = ninf, s1 = 1.0, m1 = 0.0;
    if (T >= 2) {
        const size_t t = T - 2;
        a = active ? gam[t * K + lane] : 0.0;
        bq = active ? exp(l[t * K + lane] - cmt[2 * t + 1]) / cmt[2 * t] : 0.0;
    }
    if (T >= 3) {
        const size_t t = T - 3;
        a1 = active ? gam[t * K + lane] : 0.0;
        q1 = active ? l[t * K + lane] : ninf;
        s1 = cmt[2 * t];
        m1 = cmt[2 * t + 1];
    }
    for (int t = T - 2; t >= 0; --t) {
        double a2 = 0.0, q2 = ninf, s2 = 1.0, m2 = 0.0;
        if (t > 1) {
            const size_t r = t - 2;
            a2 = active ? gam[r * K + lane] : 0.0;
            q2 = active ? l[r * K + lane] : ninf;
            s2 = cmt[2 * r];
            m2 = cmt[2 * r + 1];
        }
        const double bq1 = active ? exp(q1 - m1) / s1 : 0.0;
        double b4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int j = 0; j < KP; ++j) {
            const double pv = Pr[j] * buf[par][0][j];
            b4[j & 3] += pv;
            acc[j] += a * pv;
        }
        const double beta = (b4[0] + b4[1]) + (b4[2] + b4[3]);
        const double g = a * beta;
        par ^= 1;
        if (writer) {
            buf[par][0][lane] = bq * beta;
            buf[par][1][lane] = g;
        }
        __syncthreads();
        double z4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < KP; ++i) z4[i & 3] += buf[par][1][i];
        const double Z = (z4[0] + z4[1]) + (z4[2] + z4[3]);
        if (active) gam[(size_t)t * K + lane] = g / Z;
        a = a1;
        bq = bq1;
        a1 = a2;
        q1 = q2;
        s1 = s2;
        m1 = m2;
    }
    if (active) {
#pragma unroll
        for (int j = 0; j < KP; ++j)
            if (j < K) xi[((size_t)s * K + lane) * K + j] = acc[j];
    }
}

// ---- the grid of models: slots of KP lanes
template <int KP>
__device__ __forceinline__ double ar_slot_max(double v) {
#pragma unroll
    for (int o = KP / 2; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

template <int KP>
__device__ __forceinline__ double ar_slot_sum(double v) {
#pragma unroll
    for (int o = KP / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// `order` lists the `count` models of the class KP; wave blockIdx.y takes the models order[blockIdx.y * SL + slot].
// A model number outside [0, M), a state count outside [1, KP] or columns outside [0, KT) / [0, XT) make an empty
// slot: whatever the tables hold, nothing is read or written outside the operands.
template <int KP>
__global__ __launch_bounds__(BN_WAVE) void k_hmm_gfb(const double* __restrict__ ll, const int* __restrict__ e, int n,
                                                     int S, int M, int KT, int XT, const int* __restrict__ koff,
                                                     const int* __restrict__ xoff, const int* __restrict__ order,
                                                     int count, const double* __restrict__ logP,
                                                     const double* __restrict__ logpi0, int want,
                                                     double* __restrict__ gamma, double* __restrict__ xi,
                                                     double* __restrict__ loglik, double* __restrict__ cm) {
    constexpr int SL = BN_WAVE / KP;
    __shared__ __attribute__((aligned(16))) double buf[2][2][BN_WAVE];         // [parity][v or g][slot * KP + state]
    const int s = blockIdx.x, lane = threadIdx.x;
    const int slot = lane / KP, base = slot * KP, j = lane - base;
    const int beg = e[s], T = e[s + 1] - beg;
    const int idx = blockIdx.y * SL + slot;
    int m = idx < count ? order[idx] : -1;
    int K = 0, k0 = 0, x0 = 0;
    if (m >= 0 && m < M) {
        k0 = koff[m];
        K = koff[m + 1] - k0;
        x0 = xoff[m];
        if (K < 1 || K > KP || k0 < 0 || k0 > KT - K || x0 < 0 || x0 > XT - K * K) K = 0;
    }
    if (!K) m = 0;                                         // (an empty slot: no lane of it is active)
    const bool active = j < K, head = active && j == 0;
    if (T <= 0) {
        if (head) loglik[(size_t)m * S + s] = 0.0;
        if (want)
            for (int o = j; o < K * K; o += KP) xi[(size_t)s * XT + x0 + o] = 0.0;
        return;
    }
    const double* l = ll + (size_t)beg * KT + k0 + j;
    double* gam = gamma + (size_t)beg * KT + k0 + j;
    double* cmt = cm + ((size_t)m * n + beg) * 2;
    const double* lp = logP + x0;
    const double ninf = -INFINITY;

    double Pc[KP];
#pragma unroll
    for (int i = 0; i < KP; ++i) Pc[i] = active && i < K ? exp(lp[i * K + j]) : 0.0;
    const double pi = active ? exp(logpi0[k0 + j]) : 0.0;

    double lsum = 0.0, msum = 0.0, pend = 1.0, dot = 0.0;
    double mx, b;
    {
        const double lv = active ? l[0] : ninf;
        mx = ar_slot_max<KP>(lv);
        b = active ? exp(lv - mx) : 0.0;
    }
    double l1 = active && T > 1 ? l[(size_t)KT] : ninf;
    for (int t = 0; t < T; ++t) {
        const double l2 = active && t + 2 < T ? l[(size_t)(t + 2) * KT] : ninf;
        const double u = t == 0 ? pi * b : dot * b;
        const int par = t & 1;
        buf[par][0][lane] = u;
        __syncthreads();
        const double mn = ar_slot_max<KP>(l1);
        const double bn = active ? exp(l1 - mn) : 0.0;     // (row T: -inf - -inf, a NaN nobody reads)
        double s4[4] = {0.0, 0.0, 0.0, 0.0}, d4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < KP; ++i) {
            const double ui = buf[par][0][base + i];
            s4[i & 3] += ui;
            d4[i & 3] += ui * Pc[i];
        }
        const double st = (s4[0] + s4[1]) + (s4[2] + s4[3]);
        const double inv = 1.0 / st;
        dot = ((d4[0] + d4[1]) + (d4[2] + d4[3])) * inv;
        if (want) {
            if (active) gam[(size_t)t * KT] = u * inv;
            if (head) {
                cmt[2 * (size_t)t] = st;
                cmt[2 * (size_t)t + 1] = mx;
            }
        }
        msum += mx;
        pend = j == (t & (KP - 1)) ? st : pend;            // lane t % KP of the slot keeps s_t
        if ((t & (KP - 1)) == KP - 1) {
            lsum += log(pend);
            pend = 1.0;
        }
        mx = mn;
        b = bn;
        l1 = l2;
    }
    lsum += log(pend);
    const double total = ar_slot_sum<KP>(lsum) + msum;
    if (head) loglik[(size_t)m * S + s] = total;
    if (!want) return;

    // ---- backward: gamma holds ahat, cm holds (s_t, max_t); lane (slot, i) is the SOURCE state now
    __syncthreads();                                       // (cm, written by the slot's first lane, is read by all of it)
    double Pr[KP], acc[KP];
#pragma unroll
    for (int i = 0; i < KP; ++i) {
        Pr[i] = active && i < K ? exp(lp[j * K + i]) : 0.0;
        acc[i] = 0.0;
    }
    int par = 0;
    {
        const size_t t = T - 1;
        const double bl = active ? exp(l[t * KT] - cmt[2 * t + 1]) : 0.0;
        buf[par][0][lane] = active ? bl / cmt[2 * t] : 0.0;
        __syncthreads();
    }
    double a = 0.0, bq = 0.0, a1 = 0.0, q1 = ninf, s1 = 1.0, m1 = 0.0;
    if (T >= 2) {
        const size_t t = T - 2;
        a = active ? gam[t * KT] : 0.0;
        bq = active ? exp(l[t * KT] - cmt[2 * t + 1]) / cmt[2 * t] : 0.0;
    }
    if (T >= 3 && K) {
        const size_t t = T - 3;
        a1 = active ? gam[t * KT] : 0.0;
        q1 = active ? l[t * KT] : ninf;
        s1 = cmt[2 * t];
        m1 = cmt[2 * t + 1];
    }
    for (int t = T - 2; t >= 0; --t) {
        double a2 = 0.0, q2 = ninf, s2 = 1.0, m2 = 0.0;
        if (t > 1 && K) {
            const size_t r = t - 2;
            a2 = active ? gam[r * KT] : 0.0;
            q2 = active ? l[r * KT] : ninf;
            s2 = cmt[2 * r];
            m2 = cmt[2 * r + 1];
        }
        const double bq1 = active ? exp(q1 - m1) / s1 : 0.0;
        double b4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < KP; ++i) {
            const double pv = Pr[i] * buf[par][0][base + i];
            b4[i & 3] += pv;
            acc[i] += a * pv;
        }
        const double beta = (b4[0] + b4[1]) + (b4[2] + b4[3]);
        const double g = a * beta;
        par ^= 1;
        buf[par][0][lane] = bq * beta;
        buf[par][1][lane] = g;
        __syncthreads();
        double z4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < KP; ++i) z4[i & 3] += buf[par][1][base + i];
        const double Z = (z4[0] + z4[1]) + (z4[2] + z4[3]);
        if (active) gam[(size_t)t * KT] = g / Z;
        a = a1;
        bq = bq1;
        a1 = a2;
        q1 = q2;
        s1 = s2;
        m1 = m2;
    }
    if (active) {
#pragma unroll
        for (int i = 0; i < KP; ++i)
            if (i < K) xi[(size_t)s * XT + x0 + j * K + i] = acc[i];
    }
}

template <int KP>
__global__ __launch_bounds__(BN_WAVE) void k_hmm_viterbi(const double* __restrict__ ll, const int* __restrict__ e,
                                                         int K, const double* __restrict__ logP,
                                                         const double* __restrict__ logpi0, int* __restrict__ states,
                                                         unsigned char* __restrict__ bp) {
    __shared__ __attribute__((aligned(16))) double buf[2][KP];
    __shared__ unsigned char chunk[AR_BT_ROWS * AR_MAX_K];
    const int s = blockIdx.x, lane = threadIdx.x;
    const int beg = e[s], T = e[s + 1] - beg;
    if (T <= 0) return;
    const bool active = lane < K, writer = lane < KP;
    const double ninf = -INFINITY;
    const double* l = ll + (size_t)beg * K;
    unsigned char* back = bp + (size_t)beg * K;
    int* out = states + beg;

    double Pc[KP];
#pragma unroll
    for (int i = 0; i < KP; ++i) Pc[i] = active && i < K ? logP[i * K + lane] : ninf;
    double delta = active ? logpi0[lane] + l[lane] : ninf;
    double lv = active && T > 1 ? l[(size_t)K + lane] : ninf;
    for (int t = 1; t < T; ++t) {
        const double lnext = active && t + 1 < T ? l[(size_t)(t + 1) * K + lane] : ninf;
        const int par = t & 1;
        if (writer) buf[par][lane] = delta;
        __syncthreads();
        double best = buf[par][0] + Pc[0];
        int arg = 0;
#pragma unroll
        for (int i = 1; i < KP; ++i) {
            const double v = buf[par][i] + Pc[i];
            if (v > best) {
                best = v;
                arg = i;
            }
        }
        if (active) back[(size_t)t * K + lane] = (unsigned char)arg;
        delta = best + lv;
        lv = lnext;
    }
    const int par = T & 1;
    if (writer) buf[par][lane] = delta;
    __syncthreads();                                       // (and the back-pointers are visible to the wave)
    int cur = 0;
    {
        double best = buf[par][0];
        for (int j = 1; j < K; ++j)
            if (buf[par][j] > best) {
                best = buf[par][j];
                cur = j;
            }
    }
    for (int hi = T; hi > 0; hi -= AR_BT_ROWS) {
        const int lo = hi > AR_BT_ROWS ? hi - AR_BT_ROWS : 0;
        __syncthreads();                                   // (the chunk before this one has been walked)
        for (int idx = lane; idx < (hi - lo) * K; idx += BN_WAVE) {
            const size_t o = (size_t)lo * K + idx;
            chunk[idx] = o >= (size_t)K ? back[o] : 0;     // (row 0 has no back-pointers)
        }
        __syncthreads();
        if (lane == 0) {
            for (int t = hi - 1; t >= lo; --t) {
                out[t] = cur;
                if (t > 0) cur = chunk[(t - lo) * K + cur];
            }
        }
        cur = __shfl(cur, 0);
    }
}

// The grid form: k_hmm_gfb's slots (same order / koff / xoff rules, an empty slot reads and writes nothing) around
// k_hmm_viterbi's recursion.  states is (M, n); bp holds one byte a (row, state column).
template <int KP>
__global__ __launch_bounds__(BN_WAVE) void k_hmm_gviterbi(const double* __restrict__ ll, const int* __restrict__ e,
                                                          int n, int M, int KT, int XT, const int* __restrict__ koff,
                                                          const int* __restrict__ xoff, const int* __restrict__ order,
                                                          int count, const double* __restrict__ logP,
                                                          const double* __restrict__ logpi0, int* __restrict__ states,
                                                          unsigned char* __restrict__ bp) {
    constexpr int SL = BN_WAVE / KP;
    __shared__ __attribute__((aligned(16))) double buf[2][BN_WAVE];            // [parity][slot * KP + state]
    __shared__ unsigned char chunk[AR_BT_ROWS * BN_WAVE];                      // [row of the chunk][lane]
    __shared__ unsigned char path[SL * AR_BT_ROWS];                            // [slot][row of the chunk]
    __shared__ int model[SL];                                                  // the slot's model, -1 for none
    const int s = blockIdx.x, lane = threadIdx.x;
    const int slot = lane / KP, base = slot * KP, j = lane - base;
    const int beg = e[s], T = e[s + 1] - beg;
    if (T <= 0) return;
    const int idx = blockIdx.y * SL + slot;
    int m = idx < count ? order[idx] : -1;
    int K = 0, k0 = 0, x0 = 0;
    if (m >= 0 && m < M) {
        k0 = koff[m];
        K = koff[m + 1] - k0;
        x0 = xoff[m];
        if (K < 1 || K > KP || k0 < 0 || k0 > KT - K || x0 < 0 || x0 > XT - K * K) K = 0;
    }
    if (!K) m = -1;                                        // (an empty slot: no lane of it is active)
    const bool active = j < K, head = active && j == 0;
    if (j == 0) model[slot] = m;
    const double ninf = -INFINITY;
    const double* l = ll + (size_t)beg * KT + k0 + j;
    unsigned char* back = bp + (size_t)beg * KT + k0 + j;
    const double* lp = logP + x0;

    double Pc[KP];
#pragma unroll
    for (int i = 0; i < KP; ++i) Pc[i] = active && i < K ? lp[i * K + j] : ninf;
    double delta = active ? logpi0[k0 + j] + l[0] : ninf;
    double lv = active && T > 1 ? l[(size_t)KT] : ninf;
    for (int t = 1; t < T; ++t) {
        const double lnext = active && t + 1 < T ? l[(size_t)(t + 1) * KT] : ninf;
        const int par = t & 1;
        buf[par][lane] = delta;
        __syncthreads();
        double best = buf[par][base] + Pc[0];
        int arg = 0;
#pragma unroll
        for (int i = 1; i < KP; ++i) {
            const double v = buf[par][base + i] + Pc[i];
            if (v > best) {
                best = v;
                arg = i;
            }
        }
        if (active) back[(size_t)t * KT] = (unsigned char)arg;
        delta = best + lv;
        lv = lnext;
    }
    const int par = T & 1;
    buf[par][lane] = delta;
    __syncthreads();                                       // (and model[] is visible to the wave)
    int cur = 0;
    if (head) {
        double best = buf[par][base];
        for (int i = 1; i < K; ++i)
            if (buf[par][base + i] > best) {
                best = buf[par][base + i];
                cur = i;
            }
    }
    for (int hi = T; hi > 0; hi -= AR_BT_ROWS) {
        const int lo = hi > AR_BT_ROWS ? hi - AR_BT_ROWS : 0;
        const int cnt = hi - lo;
        __syncthreads();                                   // (the chunk before this one has been walked and written)
        // every lane stages the bytes it wrote itself (row 0 has no back-pointers)
#pragma unroll 8
        for (int r = 0; r < cnt; ++r)
            chunk[r * BN_WAVE + lane] = active && lo + r > 0 ? back[(size_t)(lo + r) * KT] : 0;
        __syncthreads();
        if (head) {
            for (int t = hi - 1; t >= lo; --t) {
                path[slot * AR_BT_ROWS + (t - lo)] = (unsigned char)cur;
                if (t > 0) cur = chunk[(t - lo) * BN_WAVE + base + cur];
            }
        }
        __syncthreads();
        if (lane < cnt) {
#pragma unroll
            for (int q = 0; q < SL; ++q) {
                const int mq = model[q];
                if (mq >= 0) states[(size_t)mq * n + beg + lo + lane] = path[q * AR_BT_ROWS + lane];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------
// states a workgroup of k_ar_moments takes with ONE staging of its rows (the accumulators of a state are
// 2 TB (TB + 1) registers a lane; at TB = 3 four states measured slower than two: one wave a SIMD)
__host__ __device__ constexpr int ar_mo_group(int TB) { return TB <= 2 ? 4 : (TB <= 4 ? 2 : 1); }

template <int TB>
__global__ __launch_bounds__(AR_MO_THREADS) void k_ar_moments(const float* __restrict__ z, int ld,
                                                              const double* __restrict__ c,
                                                              const unsigned char* __restrict__ kind,
                                                              const double* __restrict__ gamma, int D, int L, int K,
                                                              int n, int rows, double* __restrict__ slabs) {
    constexpr int PT = 16 * TB, LW = PT + 4, NT = TB * (TB + 1) / 2, SG = ar_mo_group(TB);
    __shared__ double stage[AR_MO_ROWS * LW];
    __shared__ double wgt[SG][AR_MO_ROWS];
    __shared__ double red[AR_MO_WAVES - 1][4 * BN_WAVE];
    __shared__ double shift[AR_MAX_LD];
    const int tid = threadIdx.x, lane = tid & (BN_WAVE - 1), wave = tid / BN_WAVE;
    const int kk = lane >> 4, col = lane & 15;
    const int P = 1 + (L + 1) * D, k0 = blockIdx.y * SG;
    const long row0 = (long)blockIdx.x * rows;
    const long row1 = n - row0 > rows ? row0 + rows : n;

    if (tid < D) shift[tid] = c ? c[tid] : 0.0;
    ar_d4 acc[SG][NT];
#pragma unroll
    for (int g = 0; g < SG; ++g)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[g][t] = ar_d4{0.0, 0.0, 0.0, 0.0};
    for (long r0 = row0; r0 < row1; r0 += AR_MO_ROWS) {
        __syncthreads();                                   // (the chunk before this one has been read; shift is there)
        for (int idx = tid; idx < AR_MO_ROWS * PT; idx += AR_MO_THREADS) {
            const int r = idx / PT, p = idx - r * PT;
            const long row = r0 + r;
            double v = 0.0;
            if (row < row1 && p < P && kind[row] == 2) v = ar_entry(z, ld, shift, D, row, p);
            stage[r * LW + p] = v;
        }
        if (tid < AR_MO_ROWS * SG) {
            const int g = tid / AR_MO_ROWS, r = tid - g * AR_MO_ROWS;
            const long row = r0 + r;
            wgt[g][r] = k0 + g < K && row < row1 && kind[row] == 2 ? gamma[(size_t)row * K + k0 + g] : 0.0;
        }
        __syncthreads();
        for (int ks = wave; ks < AR_MO_ROWS / 4; ks += AR_MO_WAVES) {
            double frag[TB];
#pragma unroll
            for (int q = 0; q < TB; ++q) frag[q] = stage[(4 * ks + kk) * LW + 16 * q + col];
#pragma unroll
            for (int g = 0; g < SG; ++g) {
                const double w = wgt[g][4 * ks + kk];
                double wf[TB];
#pragma unroll
                for (int q = 0; q < TB; ++q) wf[q] = w * frag[q];
                int t = 0;
#pragma unroll
                for (int ti = 0; ti < TB; ++ti)
#pragma unroll
                    for (int tj = ti; tj < TB; ++tj, ++t)
                        acc[g][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(wf[ti], frag[tj], acc[g][t], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int g = 0; g < SG; ++g) {
        if (k0 + g >= K) break;                            // (the same for the whole workgroup)
        double* dst = slabs + ((size_t)blockIdx.x * K + k0 + g) * P * P;
        int t = 0;
#pragma unroll
        for (int ti = 0; ti < TB; ++ti)
#pragma unroll
            for (int tj = ti; tj < TB; ++tj, ++t) {
                __syncthreads();                           // (red has been read)
                if (wave) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) red[wave - 1][r * BN_WAVE + lane] = acc[g][t][r];
                }
                __syncthreads();
                if (!wave) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        double v = acc[g][t][r];
#pragma unroll
                        for (int w = 0; w < AR_MO_WAVES - 1; ++w) v += red[w][r * BN_WAVE + lane];
                        const int i = 16 * ti + kk + 4 * r, j = 16 * tj + col;
                        if (i <= j && j < P) {             // (the upper triangle, mirrored)
                            dst[(size_t)i * P + j] = v;
                            if (i != j) dst[(size_t)j * P + i] = v;
                        }
                    }
                }
            }
    }
}

// out[k][o] = the partials of the row blocks added in block order; one thread an element
__global__ __launch_bounds__(256) void k_ar_combine(const double* __restrict__ slabs, int blocks, size_t total,
                                                    double* __restrict__ out) {
    const size_t o = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    double sum = 0.0;
    for (int b = 0; b < blocks; ++b) sum += slabs[(size_t)b * total + o];
    out[o] = sum;
}

// gamma0[k] = the sum of gamma[t][k] over the initial rows; thread i takes the trials i, i + 256, ... in order and
// thread 0 adds the 256 sums in thread order
__global__ __launch_bounds__(256) void k_ar_gamma0(const double* __restrict__ gamma, const int* __restrict__ e, int S,
                                                   int L, int K, double* __restrict__ gamma0) {
    __shared__ double part[256];
    const int k = blockIdx.x;
    double sum = 0.0;
    for (int s = threadIdx.x; s < S; s += 256) {
        const int beg = e[s], end = e[s + 1];
        const int stop = end - beg > L ? beg + L : end;
        for (int t = beg; t < stop; ++t) sum += gamma[(size_t)t * K + k];
    }
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int i = 0; i < 256; ++i) total += part[i];
        gamma0[k] = total;
    }
}

// ------------------------------------------------------------------------------------------------------------
// sampling
template <int KP>
__global__ __launch_bounds__(BN_WAVE) void k_ars_states(const double* __restrict__ u, const int* __restrict__ e, int K,
                                                        const double* __restrict__ cdf0,
                                                        const double* __restrict__ cdf, int* __restrict__ states,
                                                        int* __restrict__ bad, int* __restrict__ trial) {
    __shared__ double rows[(KP + 1) * KP];                 // row K: cdf0
    __shared__ double ub[AR_S_ROWS];
    const int s = blockIdx.x, lane = threadIdx.x;
    const int beg = e[s], T = e[s + 1] - beg;
    if (lane == 0) bad[s] = INT_MAX;
    if (T <= 0) return;
    for (int idx = lane; idx < (K + 1) * K; idx += BN_WAVE) rows[idx] = idx < K * K ? cdf[idx] : cdf0[idx - K * K];
    const bool cmp = lane < K - 1;                         // (the last column is never compared)
    int z = K;
    for (int t0 = 0; t0 < T; t0 += AR_S_ROWS) {
        const int cnt = T - t0 < AR_S_ROWS ? T - t0 : AR_S_ROWS;
        __syncthreads();                                   // (the chunk before this one has been read; rows is there)
        if (lane < cnt) ub[lane] = u[(size_t)beg + t0 + lane];
        __syncthreads();
        int mine = 0;
        for (int i = 0; i < cnt; ++i) {
            const double uu = ub[i];
            const bool ge = cmp && uu >= rows[z * K + (cmp ? lane : 0)];
            z = __popcll(__ballot(ge));
            mine = lane == i ? z : mine;
        }
        if (lane < cnt) {
            states[(size_t)beg + t0 + lane] = mine;
            trial[(size_t)beg + t0 + lane] = s;
        }
    }
}

__global__ __launch_bounds__(BN_WAVE) void k_ars_given(const int* __restrict__ zin, const int* __restrict__ e, int K,
                                                       int* __restrict__ states, int* __restrict__ bad,
                                                       int* __restrict__ trial) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const int beg = e[s], T = e[s + 1] - beg;
    int first = INT_MAX;
    for (int t = lane; t < T; t += BN_WAVE) {
        const int z = zin[(size_t)beg + t];
        states[(size_t)beg + t] = z;
        trial[(size_t)beg + t] = s;
        if ((z < 0 || z >= K) && first == INT_MAX) first = t;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const int other = __shfl_xor(first, o);
        first = other < first ? other : first;
    }
    if (lane == 0) bad[s] = first;
}

// ct[k][j][d] = C[k][d][j]: the threads of k_ars_drive that share a row are neighbours in d
__global__ __launch_bounds__(256) void k_ars_transpose(const double* __restrict__ C, int D, int total,
                                                       double* __restrict__ ct) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    const int d = o % D, kj = o / D, j = kj % D, k = kj / D;
    ct[o] = C[((size_t)k * D + d) * D + j];
}

__global__ __launch_bounds__(256) void k_ars_drive(const double* __restrict__ W, const double* __restrict__ ct,
                                                   const int* __restrict__ e, const int* __restrict__ bad,
                                                   const int* __restrict__ trial, int S, int D, int L, int n,
                                                   const double* __restrict__ eps,
                                                   const float* __restrict__ init, int ldi,
                                                   const int* __restrict__ states, double* __restrict__ x) {
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    const long r = gid / D;
    if (r >= n || r < e[0] || r >= e[S]) return;
    const int d = (int)(gid - r * D);
    const int lo = trial[r];                               // (left by the state pass, which walks every row of a trial)
    const long t = r - e[lo];
    double v;
    if (t >= bad[lo]) {
        v = __builtin_nan("");
    } else if (t < L) {
        v = init ? (double)init[(size_t)r * ldi + d] : eps[(size_t)r * D + d];
    } else {
        const int z = states[r];
        const double* c = ct + (size_t)z * D * D + d;
        const double* ep = eps + (size_t)r * D;
        v = W[((size_t)z * D + d) * (1 + (size_t)L * D)];
        for (int j = 0; j < D; ++j) v = fma(c[(size_t)j * D], ep[j], v);
    }
    x[(size_t)r * D + d] = v;
}

// the value of the lane a DPP control names (quad_perm, row_half_mirror), both halves of the double
template <int CTRL>
__device__ __forceinline__ double ars_dpp(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}

template <int EL>
__global__ __launch_bounds__(BN_WAVE) void k_ars_recur(const double* __restrict__ W, const int* __restrict__ e,
                                                       const int* __restrict__ bad, int D, int L, int NP,
                                                       const int* __restrict__ states, double* __restrict__ x) {
    constexpr int ZERO = (AR_S_ROWS + AR_MAX_L) * AR_S_MAX_D;          // a 0.0 for the lanes without an entry
    __shared__ double xb[ZERO + 1];                                    // rows t0 - L .. t0 + 63 of the trial
    __shared__ int zb[AR_S_ROWS + 1];                                  // states of rows t0 .. t0 + 64
    const int s = blockIdx.x, lane = threadIdx.x;
    const int beg = e[s];
    int T = e[s + 1] - beg;
    T = bad[s] < T ? bad[s] : T;                           // (the rows from a bad state on are NaN already)
    if (T <= L) return;
    const int H = L * D, P1 = 1 + H;
    const int d = lane / NP, p = lane - d * NP;
    const bool row = d < D;
    // every lane reads EL history entries and EL entries of A a step, all of them at addresses that exist: a lane
    // without an entry (h >= H, or no output row) reads the 0.0 at ZERO and column 0 of A and multiplies by 0.0
    int off[EL], col[EL];
    bool ok[EL];
#pragma unroll
    for (int i = 0; i < EL; ++i) {
        const int h = p + i * NP;
        ok[i] = row && h < H;
        const int l = ok[i] ? h / D : 0, j = ok[i] ? h - l * D : 0;
        off[i] = j - l * D;                                // x_{t-1-l}[j] from the row of x_{t-1}
        col[i] = ok[i] ? 1 + h : 0;
    }
    double* xg = x + (size_t)beg * D;
    const int* zs = states + beg;
    for (int idx = lane; idx < H; idx += BN_WAVE) xb[idx] = xg[idx];
    if (lane == 0) xb[ZERO] = 0.0;

    int zc = zs[L];
    const double* wz = W + ((size_t)zc * D + (row ? d : 0)) * P1;
    double a[EL];
#pragma unroll
    for (int i = 0; i < EL; ++i) {
        const double w = wz[col[i]];
        a[i] = ok[i] ? w : 0.0;
    }

    for (int t0 = L; t0 < T; t0 += AR_S_ROWS) {
        const int cnt = T - t0 < AR_S_ROWS ? T - t0 : AR_S_ROWS;
        for (int idx = lane; idx < cnt * D; idx += BN_WAVE) xb[H + idx] = xg[(size_t)t0 * D + idx];
        for (int idx = lane; idx <= cnt; idx += BN_WAVE) zb[idx] = t0 + idx < T ? zs[t0 + idx] : zc;
        __syncthreads();
        for (int i = 0; i < cnt; ++i) {
            const int base = (L + i - 1) * D;              // the row of x_{t-1}
            const int zn = zb[i + 1];
            const double v = xb[row ? base + D + d : ZERO];
            double hv[EL];
#pragma unroll
            for (int k = 0; k < EL; ++k) hv[k] = xb[ok[k] ? base + off[k] : ZERO];
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < EL; ++k) acc = fma(a[k], hv[k], acc);
            // A of the next row, asked for before the partial sums are added (same state: same registers)
            if (zn != zc) {
                zc = zn;
                wz = W + ((size_t)zc * D + (row ? d : 0)) * P1;
#pragma unroll
                for (int k = 0; k < EL; ++k) {
                    const double w = wz[col[k]];
                    a[k] = ok[k] ? w : 0.0;
                }
            }
            acc += ars_dpp<0xB1>(acc);                     // quad_perm [1, 0, 3, 2]: lane ^ 1
            if (NP >= 4) acc += ars_dpp<0x4E>(acc);        // quad_perm [2, 3, 0, 1]: lane ^ 2
            if (NP >= 8) acc += ars_dpp<0x141>(acc);       // row_half_mirror: the other four of the eight
            if (row && p == 0) xb[base + D + d] = v + acc;
            __syncthreads();
        }
        for (int idx = lane; idx < cnt * D; idx += BN_WAVE) xg[(size_t)t0 * D + idx] = xb[H + idx];
        if (t0 + cnt < T) {                                // the window's last L rows are the next one's history
            const double keep = lane < H ? xb[cnt * D + lane] : 0.0;
            __syncthreads();
            if (lane < H) xb[lane] = keep;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------
// one-step-ahead predictions
template <int KP>
__global__ __launch_bounds__(BN_WAVE) void k_hmm_pred(const double* __restrict__ ll, const int* __restrict__ e, int K,
                                                      const double* __restrict__ logP,
                                                      const double* __restrict__ logpi0, double* __restrict__ w) {
    __shared__ __attribute__((aligned(16))) double buf[2][KP];                 // [parity][state]
    const int s = blockIdx.x, lane = threadIdx.x;
    const int beg = e[s], T = e[s + 1] - beg;
    if (T <= 0) return;
    const bool active = lane < K, writer = lane < KP;
    const double* l = ll + (size_t)beg * K;
    double* wt = w + (size_t)beg * K;
    const double ninf = -INFINITY;

    double Pc[KP];
#pragma unroll
    for (int i = 0; i < KP; ++i) Pc[i] = active && i < K ? exp(logP[i * K + lane]) : 0.0;
    const double pi = active ? exp(logpi0[lane]) : 0.0;
    if (active) wt[lane] = pi;

    // k_hmm_fb's pipeline: the row maximum and exp of row t + 1 are formed during step t, row t + 2 is asked for then
    double b, dot = 0.0;
    {
        const double lv = active ? l[lane] : ninf;
        const double m = ar_wave_max(lv);
        b = active ? exp(lv - m) : 0.0;
    }
    double l1 = active && T > 1 ? l[(size_t)K + lane] : ninf;
    for (int t = 0; t + 1 < T; ++t) {
        const double l2 = active && t + 2 < T ? l[(size_t)(t + 2) * K + lane] : ninf;
        const double u = t == 0 ? pi * b : dot * b;
        const int par = t & 1;
        if (writer) buf[par][lane] = u;
        __syncthreads();
        const double mn = ar_wave_max(l1);
        const double bn = active ? exp(l1 - mn) : 0.0;
        double s4[4] = {0.0, 0.0, 0.0, 0.0}, d4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < KP; ++i) {
            const double ui = buf[par][i];
            s4[i & 3] += ui;
            d4[i & 3] += ui * Pc[i];
        }
        const double st = (s4[0] + s4[1]) + (s4[2] + s4[3]);
        const double inv = 1.0 / st;
        dot = ((d4[0] + d4[1]) + (d4[2] + d4[3])) * inv;
        if (active) wt[(size_t)(t + 1) * K + lane] = dot;  // the ONE store: p(z_{t+1} = lane | x_0 .. x_t)
        b = bn;
        l1 = l2;
    }
}

// wt[j][d] = W[k][d][q] for j = k Q + q < K Q and d < D, zeros in the padding; one thread an element
__global__ __launch_bounds__(256) void k_arp_fold(const double* __restrict__ W, int D, int Q, int K, int DP, int total,
                                                  double* __restrict__ wt) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    const int j = o / DP, d = o - j * DP;
    const int k = j / Q, q = j - k * Q;
    wt[o] = k < K && d < D ? W[((size_t)k * D + d) * Q + q] : 0.0;
}

// doubles a staged row of phi: Q padded to a multiple of four, plus 4 (k_ar_loglik's row stride)
__host__ __device__ constexpr int arp_lw(int Q) { return ((Q + 3) & ~3) + 4; }

__global__ __launch_bounds__(AR_PR_THREADS) void k_ar_predict(const float* __restrict__ z, int ld,
                                                              const unsigned char* __restrict__ kind, int D, int L,
                                                              int K, int n, const double* __restrict__ wt, int DP,
                                                              const double* __restrict__ w,
                                                              double* __restrict__ xhat) {
    // a wave's 32 rows of phi (LW doubles a row) and of weights (WW a row), sized by the launch: a
    // few KiB at D = 16 and one lag, so that many waves share a CU and hide the B loads of each other
    extern __shared__ double arp_lds[];
    const int tid = threadIdx.x, lane = tid & (BN_WAVE - 1), wave = tid / BN_WAVE;
    const int kk = lane >> 4, col = lane & 15;
    const int Q = 1 + L * D, LW = arp_lw(Q), WW = K + 1, JS = (K * Q + 3) >> 2;     // (taken four at a time: wt has the rows)
    const long row0 = ((long)blockIdx.x * AR_PR_WAVES + wave) * AR_PR_ROWS;
    double* st = arp_lds + (size_t)wave * AR_PR_ROWS * (LW + WW);
    double* wg = st + AR_PR_ROWS * LW;
    const float rq = 1.0f / (float)Q;

    for (int idx = lane; idx < AR_PR_ROWS * Q; idx += BN_WAVE) {
        const int r = idx / Q, q = idx - r * Q;
        const long row = row0 + r;
        double v = 0.0;
        if (row < n && kind[row] == 2) {
            if (q == 0) {
                v = 1.0;
            } else {
                const int lag = (q - 1) / D, j = q - 1 - lag * D;
                v = (double)z[(size_t)(row - 1 - lag) * ld + j];
            }
        }
        st[r * LW + q] = v;
    }
    for (int idx = lane; idx < AR_PR_ROWS * K; idx += BN_WAVE) {
        const int r = idx / K, k = idx - r * K;
        const long row = row0 + r;
        wg[r * WW + k] = row < n && kind[row] == 2 ? w[(size_t)row * K + k] : 0.0;
    }
    __syncthreads();

    for (int ct = 0; ct * 16 < D; ++ct) {
        const int d = ct * 16 + col;
        const double* bp = wt + (size_t)kk * DP + d;       // row j = 4 step + kk of the folded operand
        ar_d4 c0 = {0.0, 0.0, 0.0, 0.0}, c1 = {0.0, 0.0, 0.0, 0.0};
        // A: row `col` of the tile, entry j = k Q + q: w[k] phi[q]; B: entry j of column d.  k = j / Q by the fp32
        // reciprocal: (j + 1/2) / Q is at least 1 / (2 Q) >= 0.008 away from an integer and j < 2048, far more than
        // the product's rounding (2048 x 2^-23).  Four k-steps at a time without a branch (the operand's rows are
        // padded to 16 with zeros), so four B loads are in flight
        for (int s4 = 0; s4 < JS; s4 += 4) {
#pragma unroll
            for (int step = s4; step < s4 + 4; ++step) {
                const int j = 4 * step + kk;
                const int k = (int)(((float)j + 0.5f) * rq), q = j - k * Q;
                const bool live = k < K;
                const int kc = live ? k : 0, qc = live ? q : 0;
                const double b = bp[(size_t)step * 4 * DP];
                const double a0 = live ? wg[col * WW + kc] * st[col * LW + qc] : 0.0;
                const double a1 = live ? wg[(16 + col) * WW + kc] * st[(16 + col) * LW + qc] : 0.0;
                c0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b, c0, 0, 0, 0);
                c1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b, c1, 0, 0, 0);
            }
        }
        // C/D of the f64 MFMA: column lane & 15 (the dimension), row (lane >> 4) + 4 * reg
        if (d < D) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long ra = row0 + kk + 4 * r, rb = ra + 16;
                if (ra < n && kind[ra] == 2) xhat[(size_t)ra * D + d] = c0[r];
                if (rb < n && kind[rb] == 2) xhat[(size_t)rb * D + d] = c1[r];
            }
        }
    }
    // the initial rows: nothing to predict from, the row's own values
    if (lane < AR_PR_ROWS) {
        const long row = row0 + lane;
        if (row < n && kind[row] == 1)
            for (int j = 0; j < D; ++j) xhat[(size_t)row * D + j] = (double)z[(size_t)row * ld + j];
    }
}

// ------------------------------------------------------------------------------------------------------------
// multi-step forecasts and their sums
// first[s] = the row blocks of the trials before s (first[S]: of all); m = max(L, 1) rows of a trial are no origins
__global__ __launch_bounds__(256) void k_arf_plan(const int* __restrict__ e, int S, int m, int* __restrict__ first) {
    __shared__ long part[256];
    const int tid = threadIdx.x;
    const long per = ((long)S + 255) / 256;
    const long s0 = tid * per < S ? tid * per : S, s1 = s0 + per < S ? s0 + per : S;
    long sum = 0;
    for (long s = s0; s < s1; ++s) {
        const long no = (long)e[s + 1] - e[s] - m;
        if (no > 0) sum += (no + AR_FC_BLOCK_ROWS - 1) / AR_FC_BLOCK_ROWS;
    }
    part[tid] = sum;
    __syncthreads();
    long run = 0;
    for (int i = 0; i < tid; ++i) run += part[i];
    for (long s = s0; s < s1; ++s) {
        first[s] = (int)run;
        const long no = (long)e[s + 1] - e[s] - m;
        if (no > 0) run += (no + AR_FC_BLOCK_ROWS - 1) / AR_FC_BLOCK_ROWS;
    }
    if (tid == 255) first[S] = (int)run;
}

// bt[j][c] = N[h][k][d][q] for j = k Q + q < K Q and c = h D + d < H D, zeros in the padding; one thread an element
__global__ __launch_bounds__(256) void k_arf_fold(const double* __restrict__ N, int D, int Q, int K, int H, int CP,
                                                  long total, double* __restrict__ bt) {
    const long o = (long)blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    const int j = (int)(o / CP), c = (int)(o - (long)j * CP);
    const int k = j / Q, q = j - k * Q;
    const int h = c / D, d = c - h * D;
    bt[o] = k < K && h < H ? N[(((size_t)h * K + k) * D + d) * Q + q] : 0.0;
}

__global__ __launch_bounds__(AR_FC_THREADS) void k_ar_forecast(const float* __restrict__ z, int ld,
                                                               const int* __restrict__ e, int S,
                                                               const int* __restrict__ first, int D, int L, int K,
                                                               int H, const double* __restrict__ bt, int CP,
                                                               const double* __restrict__ w,
                                                               double* __restrict__ slabs) {
    extern __shared__ double arf_lds[];                    // a wave's 32 rows of phi and of weights, as k_ar_predict's
    __shared__ double red[AR_FC_COLS * AR_FC_TERMS];
    const int blk = blockIdx.x;
    if (blk >= first[S]) return;                           // (the grid is the host's upper bound)
    int s;
    {
        int lo = 0, hi = S - 1;                            // the first trial whose blocks end after blk
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (first[mid + 1] > blk) hi = mid; else lo = mid + 1;
        }
        s = lo;
    }
    const int tid = threadIdx.x, lane = tid & (BN_WAVE - 1), wave = tid / BN_WAVE;
    const int kk = lane >> 4, col = lane & 15;
    const int Q = 1 + L * D, LW = arp_lw(Q), WW = K + 1, JS = (K * Q + 3) >> 2, HD = H * D;
    const long end = e[s + 1];
    const long b0 = (long)e[s] + (L > 1 ? L : 1) + (long)(blk - first[s]) * AR_FC_BLOCK_ROWS;
    const long b1 = b0 + AR_FC_BLOCK_ROWS < end ? b0 + AR_FC_BLOCK_ROWS : end;        // the block's origin rows
    double* st = arf_lds + (size_t)wave * AR_FC_ROWS * (LW + WW);
    double* wg = st + AR_FC_ROWS * LW;
    const float rq = 1.0f / (float)Q;
    const int c0 = blockIdx.y * AR_FC_COLS;
    const int nct = (HD - c0 + 15) / 16;                   // the group's tiles with a column in them (the last group)

    int hh[AR_FC_CT], dd[AR_FC_CT];                        // the lane's column of every tile: horizon - 1, dimension
    bool cl[AR_FC_CT];
#pragma unroll
    for (int ct = 0; ct < AR_FC_CT; ++ct) {
        const int c = c0 + ct * 16 + col;
        cl[ct] = c < HD;
        hh[ct] = cl[ct] ? c / D : 0;
        dd[ct] = cl[ct] ? c - hh[ct] * D : 0;
    }
    double sums[AR_FC_CT][AR_FC_TERMS];
#pragma unroll
    for (int ct = 0; ct < AR_FC_CT; ++ct)
#pragma unroll
        for (int i = 0; i < AR_FC_TERMS; ++i) sums[ct][i] = 0.0;

    // the same number of rounds for both waves (the barrier); a wave without rows in a round has nothing to add
    for (long base = b0; base < b1; base += AR_FC_WAVES * AR_FC_ROWS) {
        const long row0 = base + (long)wave * AR_FC_ROWS;
        __syncthreads();
        for (int idx = lane; idx < AR_FC_ROWS * Q; idx += BN_WAVE) {
            const int r = idx / Q, q = idx - r * Q;
            const long row = row0 + r;
            double v = 0.0;
            if (row < b1) {
                if (q == 0) {
                    v = 1.0;
                } else {
                    const int lag = (q - 1) / D, j = q - 1 - lag * D;
                    v = (double)z[(size_t)(row - 1 - lag) * ld + j];
                }
            }
            st[r * LW + q] = v;
        }
        for (int idx = lane; idx < AR_FC_ROWS * K; idx += BN_WAVE) {
            const int r = idx / K, k = idx - r * K;
            const long row = row0 + r;
            wg[r * WW + k] = row < b1 ? w[(size_t)row * K + k] : 0.0;
        }
        __syncthreads();
        if (row0 >= b1) continue;

        ar_d4 acc[AR_FC_CT][2];
#pragma unroll
        for (int ct = 0; ct < AR_FC_CT; ++ct) {
            acc[ct][0] = ar_d4{0.0, 0.0, 0.0, 0.0};
            acc[ct][1] = ar_d4{0.0, 0.0, 0.0, 0.0};
        }
        const double* bp = bt + (size_t)kk * CP + c0 + col;    // row j = 4 step + kk of the folded operand
        // A as in k_ar_predict (k = j / Q by the fp32 reciprocal, exact for j < 2048), built once a k-step for the
        // 2 x AR_FC_CT tiles; bt's rows are padded to 16 and its columns to AR_FC_COLS with zeros: no bounds
        for (int s4 = 0; s4 < JS; s4 += 4) {
#pragma unroll
            for (int step = s4; step < s4 + 4; ++step) {
                const int j = 4 * step + kk;
                const int k = (int)(((float)j + 0.5f) * rq), q = j - k * Q;
                const bool live = k < K;
                const int kc = live ? k : 0, qc = live ? q : 0;
                const double a0 = live ? wg[col * WW + kc] * st[col * LW + qc] : 0.0;
                const double a1 = live ? wg[(16 + col) * WW + kc] * st[(16 + col) * LW + qc] : 0.0;
                double b[AR_FC_CT];
#pragma unroll
                for (int ct = 0; ct < AR_FC_CT; ++ct) b[ct] = bp[(size_t)step * 4 * CP + ct * 16];
#pragma unroll
                for (int ct = 0; ct < AR_FC_CT; ++ct)
                    if (ct < nct) {                        // (the same for the whole workgroup)
                        acc[ct][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b[ct], acc[ct][0], 0, 0, 0);
                        acc[ct][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b[ct], acc[ct][1], 0, 0, 0);
                    }
            }
        }
        // C/D of the f64 MFMA: column lane & 15, row (lane >> 4) + 4 * reg.  The pair (t, h) counts iff t is an origin
        // row of the block and t + h - 1 < end; nothing is read for a pair that does not count
#pragma unroll
        for (int ct = 0; ct < AR_FC_CT; ++ct) {
#pragma unroll
            for (int half = 0; half < 2; ++half) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const long row = row0 + half * 16 + kk + 4 * r;
                    if (cl[ct] && row < b1 && row + hh[ct] < end) {
                        const double y = (double)z[(size_t)(row + hh[ct]) * ld + dd[ct]];
                        const double pv = (double)z[(size_t)(row - 1) * ld + dd[ct]];
                        const double em = y - acc[ct][half][r], ep = y - pv;
                        sums[ct][0] += 1.0;
                        sums[ct][1] += y;
                        sums[ct][2] += y * y;
                        sums[ct][3] += em * em;
                        sums[ct][4] += ep * ep;
                    }
                }
            }
        }
    }
    // the four lanes of a column: (kk 0 + kk 1) + (kk 2 + kk 3) in every one of them
#pragma unroll
    for (int ct = 0; ct < AR_FC_CT; ++ct)
#pragma unroll
        for (int i = 0; i < AR_FC_TERMS; ++i) {
            double v = sums[ct][i];
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            sums[ct][i] = v;
        }
    __syncthreads();
    if (wave == 1 && kk == 0)
#pragma unroll
        for (int ct = 0; ct < AR_FC_CT; ++ct)
#pragma unroll
            for (int i = 0; i < AR_FC_TERMS; ++i) red[(ct * 16 + col) * AR_FC_TERMS + i] = sums[ct][i];
    __syncthreads();
    if (wave == 0 && kk == 0)
#pragma unroll
        for (int ct = 0; ct < AR_FC_CT; ++ct)
            if (cl[ct]) {
                double* o = slabs + ((size_t)blk * HD + c0 + ct * 16 + col) * AR_FC_TERMS;
#pragma unroll
                for (int i = 0; i < AR_FC_TERMS; ++i) o[i] = sums[ct][i] + red[(ct * 16 + col) * AR_FC_TERMS + i];
            }
}

// sums[h][s][d][i] = the partials of trial s's row blocks added in block order; one thread an element
__global__ __launch_bounds__(256) void k_arf_combine(const double* __restrict__ slabs, const int* __restrict__ first,
                                                     int S, int D, int H, size_t total, double* __restrict__ sums) {
    const size_t o = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    const int i = (int)(o % AR_FC_TERMS);
    size_t rest = o / AR_FC_TERMS;
    const int d = (int)(rest % D);
    rest /= D;
    const int s = (int)(rest % S), h = (int)(rest / S);
    double sum = 0.0;
    const size_t c = (size_t)h * D + d, HD = (size_t)H * D;
    for (int b = first[s]; b < first[s + 1]; ++b) sum += slabs[((size_t)b * HD + c) * AR_FC_TERMS + i];
    sums[o] = sum;
}

// ------------------------------------------------------------------------------------------------------------
bool bn_arhmm_ok(int n, int S, int D, int L, int K) {
    return n >= 0 && S >= 0 && S < INT32_MAX && ar_dims_ok(D, L, K);
}

// the grid's limits: KT states of all models together, M models, XT = sum K_m^2 transition entries
bool bn_arhmm_grid_ok(int n, int S, int D, int L, int KT) {
    return n >= 0 && S >= 0 && S < INT32_MAX && ar_dims_ok(D, L, KT, AR_GRID_MAX_KT);
}

bool bn_hmm_grid_ok(int n, int S, int M, int KT, int XT) {
    return n >= 0 && S >= 0 && S < INT32_MAX && M >= 1 && M <= AR_GRID_MAX_M && KT >= M && KT <= AR_GRID_MAX_KT &&
           XT >= KT && XT <= AR_MAX_K * KT;
}

bool bn_hmm_ok(int n, int S, int K) { return n >= 0 && S >= 0 && S < INT32_MAX && K >= 1 && K <= AR_MAX_K; }

size_t bn_arhmm_loglik_ws_bytes_impl(int n, int S, int D, int L, int K) {
    if (!bn_arhmm_ok(n, S, D, L, K)) return 0;
    return ar_offsets_bytes(S) + ar_pad16((size_t)n);
}

size_t bn_arhmm_moments_ws_bytes_impl(int n, int S, int D, int L, int K) {
    if (!bn_arhmm_ok(n, S, D, L, K)) return 0;
    const size_t P = 1 + (size_t)(L + 1) * D;
    return ar_offsets_bytes(S) + ar_pad16((size_t)n) + (size_t)ar_plan(n, D, L, K).blocks * K * P * P * sizeof(double);
}

size_t bn_arhmm_grid_loglik_ws_bytes_impl(int n, int S, int D, int L, int KT) {
    if (!bn_arhmm_grid_ok(n, S, D, L, KT)) return 0;
    return ar_offsets_bytes(S) + ar_pad16((size_t)n);
}

size_t bn_arhmm_grid_moments_ws_bytes_impl(int n, int S, int D, int L, int KT) {
    if (!bn_arhmm_grid_ok(n, S, D, L, KT)) return 0;
    const size_t P = 1 + (size_t)(L + 1) * D;
    return ar_offsets_bytes(S) + ar_pad16((size_t)n) + (size_t)ar_plan(n, D, L, KT).blocks * KT * P * P * sizeof(double);
}

size_t bn_hmm_grid_forward_backward_ws_bytes_impl(int n, int S, int M, int KT, int XT) {
    if (!bn_hmm_grid_ok(n, S, M, KT, XT)) return 0;
    return ar_offsets_bytes(S) + (size_t)M * n * 2 * sizeof(double);
}

size_t bn_hmm_forward_backward_ws_bytes_impl(int n, int S, int K) {
    if (!bn_hmm_ok(n, S, K)) return 0;
    return ar_offsets_bytes(S) + (size_t)n * 2 * sizeof(double);
}

size_t bn_hmm_viterbi_ws_bytes_impl(int n, int S, int K) {
    if (!bn_hmm_ok(n, S, K)) return 0;
    return ar_offsets_bytes(S) + ar_pad16((size_t)n * K);
}

size_t bn_hmm_grid_viterbi_ws_bytes_impl(int n, int S, int M, int KT, int XT) {
    if (!bn_hmm_grid_ok(n, S, M, KT, XT)) return 0;
    return ar_offsets_bytes(S) + ar_pad16((size_t)n * KT);
}

static int ar_launch_kind(const long long* offsets, int S, int L, int n, void* ws, hipStream_t st) {
    int* e = reinterpret_cast<int*>(ws);
    unsigned char* kind = reinterpret_cast<unsigned char*>(ws) + ar_offsets_bytes(S);
    const int rc = bn_launch_segment_offsets(offsets, S + 1, n, e, st);
    if (rc) return rc;
    if (n) {
        hipLaunchKernelGGL(k_ar_kind, dim3((unsigned)(((long)n + 255) / 256)), dim3(256), 0, st, (const int*)e, S, L,
                           n, kind);
        BN_LAUNCH_CHECK();
    }
    return 0;
}

// (the callers have checked K against their own limit: 32 for a model, AR_GRID_MAX_KT for a grid)
static int ar_launch_loglik(const float* z, int ld, const double* c, const long long* offsets, int S, int D, int L,
                            int K, int n, const double* G, const double* cst, double* ll, void* ws, hipStream_t st) {
    if (S == 0) return 0;
    const int rc = ar_launch_kind(offsets, S, L, n, ws, st);
    if (rc) return rc;
    if (!n) return 0;
    const unsigned char* kind = reinterpret_cast<const unsigned char*>(ws) + ar_offsets_bytes(S);
    const long per = AR_LL_WAVES * AR_LL_ROWS;
    hipLaunchKernelGGL(k_ar_loglik, dim3((unsigned)(((long)n + per - 1) / per)), dim3(AR_LL_THREADS), 0, st, z, ld, c,
                       kind, D, L, K, n, G, cst, ll);
    BN_LAUNCH_CHECK();
    return 0;
}

int bn_launch_arhmm_loglik(const float* z, int ld, const double* c, const long long* offsets, int S, int D, int L,
                           int K, int n, const double* G, const double* cst, double* ll, void* ws, hipStream_t st) {
    if (!bn_arhmm_ok(n, S, D, L, K)) return BN_E_SHAPE;
    return ar_launch_loglik(z, ld, c, offsets, S, D, L, K, n, G, cst, ll, ws, st);
}

int bn_launch_arhmm_grid_loglik(const float* z, int ld, const double* c, const long long* offsets, int S, int D,
                                int L, int KT, int n, const double* G, const double* cst, double* ll, void* ws,
                                hipStream_t st) {
    if (!bn_arhmm_grid_ok(n, S, D, L, KT)) return BN_E_SHAPE;
    return ar_launch_loglik(z, ld, c, offsets, S, D, L, KT, n, G, cst, ll, ws, st);
}

static int ar_launch_moments(const float* z, int ld, const double* c, const long long* offsets, int S, int D, int L,
                             int K, int n, const double* gamma, double* out, double* gamma0, void* ws,
                             hipStream_t st) {
    if (S == 0) return 0;
    const int rc = ar_launch_kind(offsets, S, L, n, ws, st);
    if (rc) return rc;
    const int* e = reinterpret_cast<const int*>(ws);
    const unsigned char* kind = reinterpret_cast<const unsigned char*>(ws) + ar_offsets_bytes(S);
    double* slabs = reinterpret_cast<double*>(reinterpret_cast<char*>(ws) + ar_offsets_bytes(S) + ar_pad16((size_t)n));
    const ArPlan p = ar_plan(n, D, L, K);
    const int P = 1 + (L + 1) * D;
    if (p.blocks) {
        const int TB = (P + 15) / 16, SG = ar_mo_group(TB);        // column blocks of 16; states a workgroup
        const dim3 grid((unsigned)p.blocks, (unsigned)((K + SG - 1) / SG)), block(AR_MO_THREADS);
        switch (TB) {
            case 1: hipLaunchKernelGGL(k_ar_moments<1>, grid, block, 0, st, z, ld, c, kind, gamma, D, L, K, n, p.rows, slabs); break;
            case 2: hipLaunchKernelGGL(k_ar_moments<2>, grid, block, 0, st, z, ld, c, kind, gamma, D, L, K, n, p.rows, slabs); break;
            case 3: hipLaunchKernelGGL(k_ar_moments<3>, grid, block, 0, st, z, ld, c, kind, gamma, D, L, K, n, p.rows, slabs); break;
            case 4: hipLaunchKernelGGL(k_ar_moments<4>, grid, block, 0, st, z, ld, c, kind, gamma, D, L, K, n, p.rows, slabs); break;
            default: hipLaunchKernelGGL(k_ar_moments<5>, grid, block, 0, st, z, ld, c, kind, gamma, D, L, K, n, p.rows, slabs); break;
        }
        BN_LAUNCH_CHECK();
    }
    const size_t total = (size_t)K * P * P;
    hipLaunchKernelGGL(k_ar_combine, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const double*)slabs,
                       p.blocks, total, out);
    BN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ar_gamma0, dim3((unsigned)K), dim3(256), 0, st, gamma, e, S, L, K, gamma0);
    BN_LAUNCH_CHECK();
    return 0;
}

int bn_launch_arhmm_moments(const float* z, int ld, const double* c, const long long* offsets, int S, int D, int L,
                            int K, int n, const double* gamma, double* out, double* gamma0, void* ws,
                            hipStream_t st) {
    if (!bn_arhmm_ok(n, S, D, L, K)) return BN_E_SHAPE;
    return ar_launch_moments(z, ld, c, offsets, S, D, L, K, n, gamma, out, gamma0, ws, st);
}

int bn_launch_arhmm_grid_moments(const float* z, int ld, const double* c, const long long* offsets, int S, int D,
                                 int L, int KT, int n, const double* gamma, double* out, double* gamma0, void* ws,
                                 hipStream_t st) {
    if (!bn_arhmm_grid_ok(n, S, D, L, KT)) return BN_E_SHAPE;
    return ar_launch_moments(z, ld, c, offsets, S, D, L, KT, n, gamma, out, gamma0, ws, st);
}

int bn_launch_hmm_forward_backward(const double* ll, const long long* offsets, int S, int K, int n,
                                   const double* logP, const double* logpi0, int want, double* gamma, double* xi,
                                   double* loglik, void* ws, hipStream_t st) {
    if (!bn_hmm_ok(n, S, K)) return BN_E_SHAPE;
    if (S == 0) return 0;
    int* e = reinterpret_cast<int*>(ws);
    double* cm = reinterpret_cast<double*>(reinterpret_cast<char*>(ws) + ar_offsets_bytes(S));
    const int rc = bn_launch_segment_offsets(offsets, S + 1, n, e, st);
    if (rc) return rc;
    const dim3 grid((unsigned)S), block(BN_WAVE);
    const int* ce = e;
    if (K <= 4) hipLaunchKernelGGL(k_hmm_fb<4>, grid, block, 0, st, ll, ce, K, logP, logpi0, want, gamma, xi, loglik, cm);
    else if (K <= 8) hipLaunchKernelGGL(k_hmm_fb<8>, grid, block, 0, st, ll, ce, K, logP, logpi0, want, gamma, xi, loglik, cm);
    else if (K <= 16) hipLaunchKernelGGL(k_hmm_fb<16>, grid, block, 0, st, ll, ce, K, logP, logpi0, want, gamma, xi, loglik, cm);
    else hipLaunchKernelGGL(k_hmm_fb<32>, grid, block, 0, st, ll, ce, K, logP, logpi0, want, gamma, xi, loglik, cm);
    BN_LAUNCH_CHECK();
    return 0;
}

// order: the models of class 4, then of 8, 16 and 32 (counts[0..3] of them), every model once; one launch a class
int bn_launch_hmm_grid_forward_backward(const double* ll, const long long* offsets, int S, int M, int KT, int XT, int n,
                                        const int* koff, const int* xoff, const int* order, const int* counts,
                                        const double* logP, const double* logpi0, int want, double* gamma, double* xi,
                                        double* loglik, void* ws, hipStream_t st) {
    if (!bn_hmm_grid_ok(n, S, M, KT, XT)) return BN_E_SHAPE;
    long sum = 0;
    for (int c = 0; c < 4; ++c) {
        if (counts[c] < 0 || counts[c] > M) return BN_E_SHAPE;
        sum += counts[c];
    }
    if (sum != M) return BN_E_SHAPE;
    if (S == 0) return 0;
    int* e = reinterpret_cast<int*>(ws);
    double* cm = reinterpret_cast<double*>(reinterpret_cast<char*>(ws) + ar_offsets_bytes(S));
    const int rc = bn_launch_segment_offsets(offsets, S + 1, n, e, st);
    if (rc) return rc;
    const int* ce = e;
    const dim3 block(BN_WAVE);
    int first = 0;
    for (int c = 0; c < 4; ++c) {
        const int cnt = counts[c], KP = 4 << c, SL = BN_WAVE / KP;
        if (!cnt) continue;
        const dim3 grid((unsigned)S, (unsigned)((cnt + SL - 1) / SL));
        const int* ord = order + first;
        switch (KP) {
            case 4: hipLaunchKernelGGL(k_hmm_gfb<4>, grid, block, 0, st, ll, ce, n, S, M, KT, XT, koff, xoff, ord, cnt, logP, logpi0, want, gamma, xi, loglik, cm); break;
            case 8: hipLaunchKernelGGL(k_hmm_gfb<8>, grid, block, 0, st, ll, ce, n, S, M, KT, XT, koff, xoff, ord, cnt, logP, logpi0, want, gamma, xi, loglik, cm); break;
            case 16: hipLaunchKernelGGL(k_hmm_gfb<16>, grid, block, 0, st, ll, ce, n, S, M, KT, XT, koff, xoff, ord, cnt, logP, logpi0, want, gamma, xi, loglik, cm); break;
            default: hipLaunchKernelGGL(k_hmm_gfb<32>, grid, block, 0, st, ll, ce, n, S, M, KT, XT, koff, xoff, ord, cnt, logP, logpi0, want, gamma, xi, loglik, cm); break;
        }
        BN_LAUNCH_CHECK();
        first += cnt;
    }
    return 0;
}

int bn_launch_hmm_viterbi(const double* ll, const long long* offsets, int S, int K, int n, const double* logP,
                          const double* logpi0, int* states, void* ws, hipStream_t st) {
    if (!bn_hmm_ok(n, S, K)) return BN_E_SHAPE;
    if (S == 0) return 0;
    int* e = reinterpret_cast<int*>(ws);
    unsigned char* bp = reinterpret_cast<unsigned char*>(ws) + ar_offsets_bytes(S);
    const int rc = bn_launch_segment_offsets(offsets, S + 1, n, e, st);
    if (rc) return rc;
    const dim3 grid((unsigned)S), block(BN_WAVE);
    const int* ce = e;
    if (K <= 4) hipLaunchKernelGGL(k_hmm_viterbi<4>, grid, block, 0, st, ll, ce, K, logP, logpi0, states, bp);
    else if (K <= 8) hipLaunchKernelGGL(k_hmm_viterbi<8>, grid, block, 0, st, ll, ce, K, logP, logpi0, states, bp);
    else if (K <= 16) hipLaunchKernelGGL(k_hmm_viterbi<16>, grid, block, 0, st, ll, ce, K, logP, logpi0, states, bp);
    else hipLaunchKernelGGL(k_hmm_viterbi<32>, grid, block, 0, st, ll, ce, K, logP, logpi0, states, bp);
    BN_LAUNCH_CHECK();
    return 0;
}

// order and counts as bn_launch_hmm_grid_forward_backward takes them; one launch a class
int bn_launch_hmm_grid_viterbi(const double* ll, const long long* offsets, int S, int M, int KT, int XT, int n,
                               const int* koff, const int* xoff, const int* order, const int* counts,
                               const double* logP, const double* logpi0, int* states, void* ws, hipStream_t st) {
    if (!bn_hmm_grid_ok(n, S, M, KT, XT)) return BN_E_SHAPE;
    long sum = 0;
    for (int c = 0; c < 4; ++c) {
        if (counts[c] < 0 || counts[c] > M) return BN_E_SHAPE;
        sum += counts[c];
    }
    if (sum != M) return BN_E_SHAPE;
    if (S == 0) return 0;
    int* e = reinterpret_cast<int*>(ws);
    unsigned char* bp = reinterpret_cast<unsigned char*>(ws) + ar_offsets_bytes(S);
    const int rc = bn_launch_segment_offsets(offsets, S + 1, n, e, st);
    if (rc) return rc;
    const int* ce = e;
    const dim3 block(BN_WAVE);
    int first = 0;
    for (int c = 0; c < 4; ++c) {
        const int cnt = counts[c], KP = 4 << c, SL = BN_WAVE / KP;
        if (!cnt) continue;
        const dim3 grid((unsigned)S, (unsigned)((cnt + SL - 1) / SL));
        const int* ord = order + first;
        switch (KP) {
            case 4: hipLaunchKernelGGL(k_hmm_gviterbi<4>, grid, block, 0, st, ll, ce, n, M, KT, XT, koff, xoff, ord, cnt, logP, logpi0, states, bp); break;
            case 8: hipLaunchKernelGGL(k_hmm_gviterbi<8>, grid, block, 0, st, ll, ce, n, M, KT, XT, koff, xoff, ord, cnt, logP, logpi0, states, bp); break;
            case 16: hipLaunchKernelGGL(k_hmm_gviterbi<16>, grid, block, 0, st, ll, ce, n, M, KT, XT, koff, xoff, ord, cnt, logP, logpi0, states, bp); break;
            default: hipLaunchKernelGGL(k_hmm_gviterbi<32>, grid, block, 0, st, ll, ce, n, M, KT, XT, koff, xoff, ord, cnt, logP, logpi0, states, bp); break;
        }
        BN_LAUNCH_CHECK();
        first += cnt;
    }
    return 0;
}

size_t bn_arhmm_sample_ws_bytes_impl(int n, int S, int D, int L, int K) {
    if (!bn_arhmm_ok(n, S, D, L, K)) return 0;
    return ar_offsets_bytes(S) + ar_pad16((size_t)S * sizeof(int)) + ar_pad16((size_t)n * sizeof(int)) +
           (size_t)K * D * D * sizeof(double);
}

int bn_launch_arhmm_sample(const double* W, const double* C, const double* cdf0, const double* cdf,
                           const long long* offsets, int S, int D, int L, int K, int n, const double* eps,
                           const double* u, const int* states_in, const float* init, int ld_init, double* x,
                           int* states, void* ws, hipStream_t st) {
    if (!bn_arhmm_ok(n, S, D, L, K)) return BN_E_SHAPE;
    if (S == 0) return 0;
    int* e = reinterpret_cast<int*>(ws);
    int* bad = reinterpret_cast<int*>(reinterpret_cast<char*>(ws) + ar_offsets_bytes(S));
    int* trial = bad + ar_pad16((size_t)S * sizeof(int)) / sizeof(int);
    double* ct = reinterpret_cast<double*>(trial + ar_pad16((size_t)n * sizeof(int)) / sizeof(int));
    const int rc = bn_launch_segment_offsets(offsets, S + 1, n, e, st);
    if (rc) return rc;
    const dim3 grid((unsigned)S), block(BN_WAVE);
    const int* ce = e;
    const int* cbad = bad;
    if (states_in) hipLaunchKernelGGL(k_ars_given, grid, block, 0, st, states_in, ce, K, states, bad, trial);
    else if (K <= 4) hipLaunchKernelGGL(k_ars_states<4>, grid, block, 0, st, u, ce, K, cdf0, cdf, states, bad, trial);
    else if (K <= 8) hipLaunchKernelGGL(k_ars_states<8>, grid, block, 0, st, u, ce, K, cdf0, cdf, states, bad, trial);
    else if (K <= 16) hipLaunchKernelGGL(k_ars_states<16>, grid, block, 0, st, u, ce, K, cdf0, cdf, states, bad, trial);
    else hipLaunchKernelGGL(k_ars_states<32>, grid, block, 0, st, u, ce, K, cdf0, cdf, states, bad, trial);
    BN_LAUNCH_CHECK();
    if (!n) return 0;
    const int cells = K * D * D;
    hipLaunchKernelGGL(k_ars_transpose, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, C, D, cells, ct);
    BN_LAUNCH_CHECK();
    const long elems = (long)n * D;
    hipLaunchKernelGGL(k_ars_drive, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, st, W, (const double*)ct, ce,
                       cbad, (const int*)trial, S, D, L, n, eps, init, ld_init, (const int*)states, x);
    BN_LAUNCH_CHECK();
    if (L == 0) return 0;
    // lanes (d, p): NP partial sums a row, EL history entries a lane at most
    const int NP = D <= 8 ? 8 : (D <= 16 ? 4 : 2), EL = (L * D + NP - 1) / NP;
    const int* cs = states;
    if (EL <= 1) hipLaunchKernelGGL(k_ars_recur<1>, grid, block, 0, st, W, ce, cbad, D, L, NP, cs, x);
    else if (EL <= 2) hipLaunchKernelGGL(k_ars_recur<2>, grid, block, 0, st, W, ce, cbad, D, L, NP, cs, x);
    else if (EL <= 4) hipLaunchKernelGGL(k_ars_recur<4>, grid, block, 0, st, W, ce, cbad, D, L, NP, cs, x);
    else if (EL <= 8) hipLaunchKernelGGL(k_ars_recur<8>, grid, block, 0, st, W, ce, cbad, D, L, NP, cs, x);
    else if (EL <= 16) hipLaunchKernelGGL(k_ars_recur<16>, grid, block, 0, st, W, ce, cbad, D, L, NP, cs, x);
    else hipLaunchKernelGGL(k_ars_recur<24>, grid, block, 0, st, W, ce, cbad, D, L, NP, cs, x);
    BN_LAUNCH_CHECK();
    return 0;
}

// ---- one-step-ahead predictions
static int arp_dp(int D) { return (D + 15) & ~15; }
static int arp_jp(int D, int L, int K) { return (K * (1 + L * D) + 15) & ~15; }   // four k-steps of four rows

size_t bn_hmm_predictive_ws_bytes_impl(int n, int S, int K) {
    if (!bn_hmm_ok(n, S, K)) return 0;
    return ar_offsets_bytes(S);
}

size_t bn_arhmm_predict_ws_bytes_impl(int n, int S, int D, int L, int K) {
    if (!bn_arhmm_ok(n, S, D, L, K)) return 0;
    return ar_offsets_bytes(S) + ar_pad16((size_t)n) + (size_t)arp_jp(D, L, K) * arp_dp(D) * sizeof(double);
}

int bn_launch_hmm_predictive(const double* ll, const long long* offsets, int S, int K, int n, const double* logP,
                             const double* logpi0, double* w, void* ws, hipStream_t st) {
    if (!bn_hmm_ok(n, S, K)) return BN_E_SHAPE;
    if (S == 0) return 0;
    int* e = reinterpret_cast<int*>(ws);
    const int rc = bn_launch_segment_offsets(offsets, S + 1, n, e, st);
    if (rc) return rc;
    const dim3 grid((unsigned)S), block(BN_WAVE);
    const int* ce = e;
    if (K <= 4) hipLaunchKernelGGL(k_hmm_pred<4>, grid, block, 0, st, ll, ce, K, logP, logpi0, w);
    else if (K <= 8) hipLaunchKernelGGL(k_hmm_pred<8>, grid, block, 0, st, ll, ce, K, logP, logpi0, w);
    else if (K <= 16) hipLaunchKernelGGL(k_hmm_pred<16>, grid, block, 0, st, ll, ce, K, logP, logpi0, w);
    else hipLaunchKernelGGL(k_hmm_pred<32>, grid, block, 0, st, ll, ce, K, logP, logpi0, w);
    BN_LAUNCH_CHECK();
    return 0;
}

int bn_launch_arhmm_predict(const float* z, int ld, const long long* offsets, int S, int D, int L, int K, int n,
                            const double* W, const double* w, double* xhat, void* ws, hipStream_t st) {
    if (!bn_arhmm_ok(n, S, D, L, K)) return BN_E_SHAPE;
    if (S == 0) return 0;
    const int rc = ar_launch_kind(offsets, S, L, n, ws, st);
    if (rc) return rc;
    if (!n) return 0;
    const unsigned char* kind = reinterpret_cast<const unsigned char*>(ws) + ar_offsets_bytes(S);
    double* wt = reinterpret_cast<double*>(reinterpret_cast<char*>(ws) + ar_offsets_bytes(S) + ar_pad16((size_t)n));
    const int DP = arp_dp(D), total = arp_jp(D, L, K) * DP;
    hipLaunchKernelGGL(k_arp_fold, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, W, D, 1 + L * D, K, DP,
                       total, wt);
    BN_LAUNCH_CHECK();
    const long per = AR_PR_WAVES * AR_PR_ROWS;
    // LDS a workgroup: at most 2 x 32 x (64 + 33) doubles = 48.5 KiB (Q <= 57, K <= 32)
    const size_t lds = (size_t)AR_PR_WAVES * AR_PR_ROWS * (arp_lw(1 + L * D) + K + 1) * sizeof(double);
    hipLaunchKernelGGL(k_ar_predict, dim3((unsigned)(((long)n + per - 1) / per)), dim3(AR_PR_THREADS), lds, st, z, ld,
                       kind, D, L, K, n, (const double*)wt, DP, w, xhat);
    BN_LAUNCH_CHECK();
    return 0;
}

// ---- multi-step forecasts and their sums
static bool arf_ok(int n, int S, int D, int L, int K, int H) {
    return bn_arhmm_ok(n, S, D, L, K) && H >= 1 && H <= AR_FC_MAX_H;
}
static int arf_cp(int D, int H) { return (H * D + AR_FC_COLS - 1) / AR_FC_COLS * AR_FC_COLS; }
// row blocks at most: every trial with origin rows ends with one block that may not be full, and a block holds an
// origin row at least
static long arf_blocks(int n, int S) {
    const long by_rows = (long)n / AR_FC_BLOCK_ROWS + S;
    return by_rows < n ? by_rows : n;
}

size_t bn_arhmm_forecast_sums_ws_bytes_impl(int n, int S, int D, int L, int K, int H) {
    if (!arf_ok(n, S, D, L, K, H)) return 0;
    return 2 * ar_offsets_bytes(S) + (size_t)arp_jp(D, L, K) * arf_cp(D, H) * sizeof(double) +
           (size_t)arf_blocks(n, S) * H * D * AR_FC_TERMS * sizeof(double);
}

int bn_launch_arhmm_forecast_sums(const float* z, int ld, const long long* offsets, int S, int D, int L, int K, int H,
                                  int n, const double* N, const double* w, double* sums, void* ws, hipStream_t st) {
    if (!arf_ok(n, S, D, L, K, H)) return BN_E_SHAPE;
    if (S == 0) return 0;
    int* e = reinterpret_cast<int*>(ws);
    int* first = reinterpret_cast<int*>(reinterpret_cast<char*>(ws) + ar_offsets_bytes(S));
    double* bt = reinterpret_cast<double*>(reinterpret_cast<char*>(ws) + 2 * ar_offsets_bytes(S));
    const int CP = arf_cp(D, H), JP = arp_jp(D, L, K);
    double* slabs = bt + (size_t)JP * CP;
    const int rc = bn_launch_segment_offsets(offsets, S + 1, n, e, st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_arf_plan, dim3(1), dim3(256), 0, st, (const int*)e, S, L > 1 ? L : 1, first);
    BN_LAUNCH_CHECK();
    const long blocks = arf_blocks(n, S);
    if (blocks) {
        const long total = (long)JP * CP;
        hipLaunchKernelGGL(k_arf_fold, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, N, D, 1 + L * D, K, H,
                           CP, total, bt);
        BN_LAUNCH_CHECK();
        // LDS a workgroup: k_ar_predict's, at most 48.5 KiB, and 2.5 KiB of partial sums
        const size_t lds = (size_t)AR_FC_WAVES * AR_FC_ROWS * (arp_lw(1 + L * D) + K + 1) * sizeof(double);
        hipLaunchKernelGGL(k_ar_forecast, dim3((unsigned)blocks, (unsigned)(CP / AR_FC_COLS)), dim3(AR_FC_THREADS), lds,
                           st, z, ld, (const int*)e, S, (const int*)first, D, L, K, H, (const double*)bt, CP, w, slabs);
        BN_LAUNCH_CHECK();
    }
    const size_t total = (size_t)H * S * D * AR_FC_TERMS;
    hipLaunchKernelGGL(k_arf_combine, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const double*)slabs,
                       (const int*)first, S, D, H, total, sums);
    BN_LAUNCH_CHECK();
    return 0;
}
