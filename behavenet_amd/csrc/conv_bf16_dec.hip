// Inference-only transposed-conv decoder stack on bf16 operands with fp32 accumulation (DESIGN.md section 4,
// "bf16 decoder").  The counterpart of conv_bf16.hip; the private activation layout (bf16 (N, H, W, C), channels
// last), the rounding rule, the buffer loads and the MFMA tile are the same (bn_bf16.h).
//
//   k_bf16_packT_w  fp32 nn.ConvTranspose2d weights (Cin, Cout, R, S) -> bf16 [co][(r * S + s) * Cin + ci]: the
//                   operand layout of the encoder's body kernel from a source with the channel axes swapped
//   k_bf16_to_nhwc  the stack's input, fp32 (N, C, H, W) (the dense layer's output) -> bf16 (N, H, W, C), one rounding
//   k_bf16_convT    body layers: the transposed convolution as a GATHER, implicit GEMM on v_mfma_f32_32x32x16_bf16
//   k_bf16_lastT    the layer onto the frame (1..4 output channels): bf16 activations, fp32 weights that are NOT
//                   rounded, fp32 FMAs on the vector unit, bias + activation, fp32 (N, Cout, Ho, Wo)
//
// Geometry (BnBf16Geom read as a transposed convolution): (C, H, W) -> (K, P, Q), kernel R x S, `stride`, and
// (pt, pl) the crop: output pixel o is pixel f = o + crop of the full-size map.  Tap r of the kernel reaches f from
// input row (f - r) / stride iff f - r >= 0, (f - r) % stride == 0 and (f - r) / stride < H.  All output pixels with
// the same (f_y % stride, f_x % stride) -- one PHASE -- have the same list of taps r = f_y % stride + i * stride.
// No scatter, no atomics, no split reductions: two launches on the same operands give the same bits.
#include "bn_bf16.h"

// ------------------------------------------------------------------------------------------ phases
// One axis of one phase: the output coordinates o0, o0 + stride, .. (cnt of them), the taps ph, ph + stride, ..
// (ntap of them), and b0 such that output number j of the phase reads input coordinate b0 + j - i for tap number i.
struct BfTAxis { int o0, cnt, ntap, b0; };
__host__ __device__ __forceinline__ BfTAxis bft_axis(int ph, int stride, int crop, int out, int ksize) {
    BfTAxis a;
    a.o0 = ((ph - crop) % stride + stride) % stride;
    a.cnt = a.o0 < out ? (out - a.o0 + stride - 1) / stride : 0;
    a.ntap = ph < ksize ? (ksize - ph + stride - 1) / stride : 0;
    a.b0 = (a.o0 + crop - ph) / stride;          // (exact: o0 + crop = ph modulo stride, and not below ph)
    return a;
}

// ------------------------------------------------------------------------------------------ weights
// One workgroup: PKT_CI input channels x PKT_CO output channels.  For one input channel the PKT_CO x RS floats are
// contiguous in the source; for one (output channel, tap) the PKT_CI bf16 are contiguous in the destination: read
// in source order into LDS (rows of an odd length: the transposed read is free of bank conflicts), written in
// destination order.
#define PKT_CI 32
#define PKT_CO 8
__global__ __launch_bounds__(256) void k_bf16_packT_w(const float* __restrict__ w, unsigned short* __restrict__ wp,
                                                      int Ci, int Co, int RS) {
    __shared__ float s_t[PKT_CI * (PKT_CO * 25 + 1)];
    const int co0 = blockIdx.x * PKT_CO, ci0 = blockIdx.y * PKT_CI;
    const int nco = min(PKT_CO, Co - co0), nci = min(PKT_CI, Ci - ci0);
    const int run = nco * RS, ld = PKT_CO * 25 + 1;
    for (int i = threadIdx.x; i < nci * run; i += 256) {
        const int ci = i / run, e = i - ci * run;
        s_t[ci * ld + e] = w[((size_t)(ci0 + ci) * Co + co0) * RS + e];          // [ci][co][tap]
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nci * run; i += 256) {
        const int ci = i % nci, e = i / nci;                                     // e = co * RS + tap
        const int co = e / RS, tap = e - co * RS;
        wp[((size_t)(co0 + co) * RS + tap) * Ci + ci0 + ci] = (unsigned short)bn_f32_to_bf16(s_t[ci * ld + e]);
    }
}

int bn_launch_bf16_packT_w(const float* w, void* wp, int Ci, int Co, int R, int S, hipStream_t st) {
    if (R * S > 25 || (Ci + PKT_CI - 1) / PKT_CI > 65535) return BN_E_SHAPE;
    const dim3 grid((unsigned)((Co + PKT_CO - 1) / PKT_CO), (unsigned)((Ci + PKT_CI - 1) / PKT_CI));
    hipLaunchKernelGGL(k_bf16_packT_w, grid, dim3(256), 0, st, w, (unsigned short*)wp, Ci, Co, R * S);
    BN_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------ stack input
// About 2 K values per frame: one thread per output value, neighbouring threads neighbouring channels.
__global__ __launch_bounds__(256) void k_bf16_to_nhwc(const float* __restrict__ x, unsigned short* __restrict__ y,
                                                      size_t total, int C, int HW) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    const size_t rest = i / C;
    const int hw = (int)(rest % HW);
    const size_t n = rest / HW;
    y[i] = (unsigned short)bn_f32_to_bf16(x[(n * C + c) * HW + hw]);
}

int bn_launch_bf16_to_nhwc(const float* x, void* y, int N, int C, int H, int W, hipStream_t st) {
    const size_t total = (size_t)N * C * H * W;
    if ((total + 255) / 256 >= ((size_t)1 << 31)) return BN_E_SHAPE;
    hipLaunchKernelGGL(k_bf16_to_nhwc, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, (unsigned short*)y,
                       total, C, H * W);
    BN_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------ body layers
// Implicit GEMM per phase: D[m][k] = sum_kk A[m][kk] B[kk][k]; m = (n, jy, jx) numbers the output pixels of the
// phase (blockIdx.z), kk = (ty * ntx + tx) * C + c walks the phase's taps in that fixed order.  Tile, LDS rows and
// the two named register sets as in k_bf16_conv.  C % 16 == 0: one MFMA step is 16 consecutive kk of one tap and
// every 16-byte piece is aligned and within one pixel; a 64-deep step may straddle taps (each thread tracks the
// tap of its own piece).  Out-of-range pieces (an input row outside the map, the tails of m, k and kk) are staged as
// zeros and never read from memory.  A phase without taps (stride beyond the kernel, or output pixels past the
// full size through output_padding) gets the bias alone.
bool bn_bf16_convT_ok(const BnBf16Geom& g) {
    // (both operands are addressed with 32-bit byte offsets)
    return g.C % 16 == 0 && g.K >= 1 && g.R <= 5 && g.S <= 5 && g.stride <= 5 &&
           (size_t)g.N * g.H * g.W * g.C * 2 < ((size_t)1 << 31) && (size_t)g.K * g.R * g.S * g.C * 2 < ((size_t)1 << 31) &&
           (size_t)g.N * g.P * g.Q < ((size_t)1 << 31) && (size_t)g.N * g.P * g.Q * g.K < ((size_t)1 << 40);
}

template <int WM, bool OUT_F32>
__global__ __launch_bounds__(256) void k_bf16_convT(const unsigned short* __restrict__ x,
                                                    const unsigned short* __restrict__ wp,
                                                    const float* __restrict__ bias, void* __restrict__ yv,
                                                    BnBf16Geom g, int act, float slope) {
    constexpr int BM = 64 * WM;
    constexpr int NA = BM / 32, NB = BFC_BN / 32;
    __shared__ __attribute__((aligned(16))) unsigned short s_all[(BM + BFC_BN) * BFC_LD];
    __shared__ int s_n[BM], s_pq[BM];          // where the tile's rows go (epilogue)
    unsigned short* s_a = s_all;
    unsigned short* s_b = s_all + BM * BFC_LD;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int pc = tid & 7, row0 = tid >> 3;
    const int phy = blockIdx.z / g.stride, phx = blockIdx.z - phy * g.stride;
    const BfTAxis ay = bft_axis(phy, g.stride, g.pt, g.P, g.R), ax = bft_axis(phx, g.stride, g.pl, g.Q, g.S);
    const int JJ = ay.cnt * ax.cnt;
    const int Mtot = g.N * JJ;
    const int m0 = blockIdx.x * BM, k0blk = blockIdx.y * BFC_BN;
    if (m0 >= Mtot) return;                    // (the grid is sized for the largest phase; uniform for the workgroup)
    const int PQ = g.P * g.Q;
    const int Ktot = ay.ntap * ax.ntap * g.C;

    if (tid < BM) {
        const int m = m0 + tid;
        int n = -1, pq = 0;
        if (m < Mtot) {
            n = m / JJ;
            const int j = m - n * JJ;
            const int jy = j / ax.cnt, jx = j - jy * ax.cnt;
            pq = (ay.o0 + jy * g.stride) * g.Q + ax.o0 + jx * g.stride;
        }
        s_n[tid] = n;
        s_pq[tid] = pq;
    }

    // the rows this thread stages: input coordinate of tap (ty, tx) is (iy0 - ty, ix0 - tx)
    int iy0[NA], ix0[NA];
    size_t abase[NA];
    bool mok[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int m = m0 + row0 + 32 * i;
        mok[i] = m < Mtot;
        const int mm = mok[i] ? m : 0;
        const int n = mm / JJ, j = mm - n * JJ;
        const int jy = j / ax.cnt, jx = j - jy * ax.cnt;
        iy0[i] = ay.b0 + jy;
        ix0[i] = ax.b0 + jx;
        abase[i] = (size_t)n * g.H * g.W * g.C;
    }
    const int RSC = g.R * g.S * g.C;
    size_t bbase[NB];
    bool kok[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int k = k0blk + row0 + 32 * j;
        kok[j] = k < g.K;
        bbase[j] = (size_t)(kok[j] ? k : 0) * RSC;
    }
    // position of this thread's piece in the reduction: kk = (ty * ntx + tx) * C + c
    int kk = pc * 8;
    int c = kk % g.C, tap = kk / g.C;
    int ty = ax.ntap > 0 ? tap / ax.ntap : 0, tx = ax.ntap > 0 ? tap - ty * ax.ntap : 0;

    const bn_rsrc_t xr = bn_make_rsrc(x, (size_t)g.N * g.H * g.W * g.C * 2);
    const bn_rsrc_t wr = bn_make_rsrc(wp, (size_t)g.K * RSC * 2);
    auto fetch = [&](uint4 (&ra)[NA], uint4 (&rb)[NB]) {
        const bool kin = kk < Ktot;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int ih = iy0[i] - ty, iw = ix0[i] - tx;
            const bool ok = kin && mok[i] && ih >= 0 && ih < g.H && iw >= 0 && iw < g.W;
            // an offset past the operand's last byte reads as zeros without touching memory (k_bf16_conv)
            const unsigned off = ok ? (unsigned)((abase[i] + ((size_t)ih * g.W + iw) * g.C + c) * 2) : 0xffffffffu;
            ra[i] = bn_buf_load16(xr, off);
        }
        const int wk = ((phy + ty * g.stride) * g.S + phx + tx * g.stride) * g.C + c;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const unsigned off = (kin && kok[j]) ? (unsigned)((bbase[j] + wk) * 2) : 0xffffffffu;
            rb[j] = bn_buf_load16(wr, off);
        }
    };
    auto advance = [&]() {
        kk += BFC_BK;
        c += BFC_BK;
        while (c >= g.C) {
            c -= g.C;
            if (++tx == ax.ntap) { tx = 0; ++ty; }
        }
    };

    f32x16_t acc[WM];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;

    const int nsteps = (Ktot + BFC_BK - 1) / BFC_BK;
    const int fr = lane & 31, fh = lane >> 5;
    auto do_step = [&](uint4 (&ra)[NA], uint4 (&rb)[NB], bool refill) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NA; ++i) *(uint4*)(s_a + (row0 + 32 * i) * BFC_LD + pc * 8) = ra[i];
#pragma unroll
        for (int j = 0; j < NB; ++j) *(uint4*)(s_b + (row0 + 32 * j) * BFC_LD + pc * 8) = rb[j];
        __syncthreads();
        if (refill) {
            advance();
            fetch(ra, rb);
        }
#pragma unroll
        for (int ks = 0; ks < BFC_BK / 16; ++ks) {
            const uint4 bq = *(const uint4*)(s_b + (wn * 32 + fr) * BFC_LD + ks * 16 + fh * 8);
            bf16x8_t bf;
            __builtin_memcpy(&bf, &bq, 16);
#pragma unroll
            for (int i = 0; i < WM; ++i) {
                const uint4 aq = *(const uint4*)(s_a + (wm * 32 * WM + i * 32 + fr) * BFC_LD + ks * 16 + fh * 8);
                bf16x8_t af;
                __builtin_memcpy(&af, &aq, 16);
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, acc[i], 0, 0, 0);
            }
        }
    };
    uint4 ra0[NA], rb0[NB], ra1[NA], rb1[NB];
    if (nsteps > 0) fetch(ra0, rb0);
    if (nsteps > 1) {
        advance();
        fetch(ra1, rb1);
    }
    for (int step = 0; step < nsteps; step += 2) {
        do_step(ra0, rb0, step + 2 < nsteps);
        if (step + 1 < nsteps) do_step(ra1, rb1, step + 3 < nsteps);
    }
    __syncthreads();          // s_n / s_pq (a phase without taps has not met a barrier yet)

    // epilogue: lane = output channel, registers = output pixels
    const int k = k0blk + wn * 32 + fr;
    if (k >= g.K) return;
    const float bv = bias ? bias[k] : 0.f;
#pragma unroll
    for (int i = 0; i < WM; ++i) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int row = wm * 32 * WM + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * fh;
            const int n = s_n[row];
            if (n < 0) continue;
            const int pq = s_pq[row];
            const float v = bn_apply_act(acc[i][e] + bv, act, slope);
            if (OUT_F32)
                ((float*)yv)[((size_t)n * g.K + k) * PQ + pq] = v;
            else
                ((unsigned short*)yv)[((size_t)n * PQ + pq) * g.K + k] = (unsigned short)bn_f32_to_bf16(v);
        }
    }
}

int bn_launch_bf16_convT(const void* x, const void* wp, const float* bias, void* y, int out_f32, const BnBf16Geom& g,
                         int act, float slope, hipStream_t st) {
    // the grid's x covers the rows of the largest phase; workgroups beyond a smaller phase's rows leave at once
    int cy = 0, cx = 0;
    for (int ph = 0; ph < g.stride; ++ph) {
        cy = max(cy, bft_axis(ph, g.stride, g.pt, g.P, g.R).cnt);
        cx = max(cx, bft_axis(ph, g.stride, g.pl, g.Q, g.S).cnt);
    }
    const size_t M = (size_t)g.N * cy * cx;
    const unsigned gy = (unsigned)((g.K + BFC_BN - 1) / BFC_BN), gz = (unsigned)(g.stride * g.stride);
    if (gy > 65535) return BN_E_SHAPE;
    const unsigned short* xs = (const unsigned short*)x;
    const unsigned short* ws = (const unsigned short*)wp;
    // the large tile where it still fills the chip twice over, the small one otherwise (as bn_launch_bf16_conv)
    if (((M + 127) / 128) * gy * gz >= 512) {
        const dim3 grid((unsigned)((M + 127) / 128), gy, gz);
        if (out_f32)
            BN_LAUNCH_MAIN((k_bf16_convT<2, true>), grid, dim3(256), 0, st, xs, ws, bias, y, g, act, slope);
        else
            BN_LAUNCH_MAIN((k_bf16_convT<2, false>), grid, dim3(256), 0, st, xs, ws, bias, y, g, act, slope);
    } else {
        const dim3 grid((unsigned)((M + 63) / 64), gy, gz);
        if (out_f32)
            BN_LAUNCH_MAIN((k_bf16_convT<1, true>), grid, dim3(256), 0, st, xs, ws, bias, y, g, act, slope);
        else
            BN_LAUNCH_MAIN((k_bf16_convT<1, false>), grid, dim3(256), 0, st, xs, ws, bias, y, g, act, slope);
    }
    BN_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------ last layer
// Onto the frame: K = 1..4 output channels would use 1..4 of the 64 columns of a matrix-core tile, so this layer
// runs on the vector unit like the encoder's first one -- and keeps its weights in fp32.  It is bound by reading
// the input map (bf16: half the bytes of the fp32 path).  The whole weight tensor is staged ONCE per workgroup in
// LDS as [tap][co][ci] floats; a workgroup then walks many work items.  A work item is BFL_PX x 64 output pixels of
// ONE phase of one frame and belongs to one wave, so the tap loop and the weight reads are uniform over the wave
// (an LDS read of one address by all lanes is a broadcast, free of bank conflicts); a lane owns BFL_PX pixels of
// all output channels and reads its input pixels' channels as 16-byte pieces (8 channels) through the same
// bounds-checked buffer loads (a tap outside the map reads zeros, nothing outside the operand is touched).
#define BFL_PX 2
#define BFL_LDS_MAX (48 * 1024)
#define BFL_MAX_BLOCKS 2048          // 8 workgroups for each of 256 CUs: the weights are staged 2048 times at most
bool bn_bf16_lastT_ok(const BnBf16Geom& g) {
    return g.C % 16 == 0 && g.K >= 1 && g.K <= 4 && g.R <= 5 && g.S <= 5 && g.stride <= 5 &&
           (size_t)g.R * g.S * g.K * g.C * sizeof(float) <= BFL_LDS_MAX &&
           (size_t)g.N * g.H * g.W * g.C * 2 < ((size_t)1 << 31) && (size_t)g.N * g.P * g.Q < ((size_t)1 << 31);
}

// The whole weight tensor into LDS as [(r * S + s)][co][ci] floats (every thread of the workgroup; a barrier follows)
template <int CO>
__device__ __forceinline__ void bfl_stage_weights(const float* __restrict__ w, float* s_w, const BnBf16Geom& g) {
    const int RS = g.R * g.S;
    for (int i = threadIdx.x; i < g.C * CO * RS; i += 256) {
        const int ci = i / (CO * RS), e = i - ci * (CO * RS);          // source order: (Cin, Cout, R, S)
        const int co = e / RS, tap = e - co * RS;
        s_w[(tap * CO + co) * g.C + ci] = w[i];
    }
    __syncthreads();
}

// One work item of k_bf16_lastT -- and of k_bf16_lastT_sqerr, which scores the SAME pre-activations: the BFL_PX x 64
// pixels number `chunk` of phase `ph` of frame `n`.  acc[t][co] is the bias plus the taps in the order (ty, tx, ci);
// pixel t of this lane is (jy[t], jx[t]) of the phase where ok[t].  False (nothing set) for a chunk past the phase.
template <int CO>
__device__ __forceinline__ bool bfl_item(const bn_rsrc_t& xr, const float* s_w, const float (&bv)[CO],
                                         const BnBf16Geom& g, int n, int ph, int chunk, int lane, BfTAxis& ay,
                                         BfTAxis& ax, int (&jy)[BFL_PX], int (&jx)[BFL_PX], bool (&ok)[BFL_PX],
                                         float (&acc)[BFL_PX][CO]) {
    const int phy = ph / g.stride, phx = ph - phy * g.stride;
    ay = bft_axis(phy, g.stride, g.pt, g.P, g.R);
    ax = bft_axis(phx, g.stride, g.pl, g.Q, g.S);
    const int JJ = ay.cnt * ax.cnt;
    if (chunk * (64 * BFL_PX) >= JJ) return false;
#pragma unroll
    for (int t = 0; t < BFL_PX; ++t) {
        const int j = chunk * (64 * BFL_PX) + t * 64 + lane;
        ok[t] = j < JJ;
        const int jj = ok[t] ? j : 0;
        jy[t] = jj / ax.cnt;
        jx[t] = jj - jy[t] * ax.cnt;
#pragma unroll
        for (int co = 0; co < CO; ++co) acc[t][co] = bv[co];
    }
    const size_t nbase = (size_t)n * g.H * g.W * g.C;
    for (int ty = 0; ty < ay.ntap; ++ty) {
        for (int tx = 0; tx < ax.ntap; ++tx) {
            const float* wt = s_w + (size_t)((phy + ty * g.stride) * g.S + phx + tx * g.stride) * CO * g.C;
            unsigned off[BFL_PX];
            bool in[BFL_PX];
#pragma unroll
            for (int t = 0; t < BFL_PX; ++t) {
                const int ih = ay.b0 + jy[t] - ty, iw = ax.b0 + jx[t] - tx;
                in[t] = ok[t] && ih >= 0 && ih < g.H && iw >= 0 && iw < g.W;
                off[t] = (unsigned)((nbase + ((size_t)ih * g.W + iw) * g.C) * 2);
            }
            for (int c8 = 0; c8 < g.C; c8 += 8) {
                float xf[BFL_PX][8];
#pragma unroll
                for (int t = 0; t < BFL_PX; ++t) {
                    // (selected per piece: an out-of-range marker plus a channel offset would wrap into range)
                    const uint4 v = bn_buf_load16(xr, in[t] ? off[t] + (unsigned)c8 * 2 : 0xffffffffu);
                    xf[t][0] = __uint_as_float(v.x << 16);
                    xf[t][1] = __uint_as_float(v.x & 0xffff0000u);
                    xf[t][2] = __uint_as_float(v.y << 16);
                    xf[t][3] = __uint_as_float(v.y & 0xffff0000u);
                    xf[t][4] = __uint_as_float(v.z << 16);
                    xf[t][5] = __uint_as_float(v.z & 0xffff0000u);
                    xf[t][6] = __uint_as_float(v.w << 16);
                    xf[t][7] = __uint_as_float(v.w & 0xffff0000u);
                }
#pragma unroll
                for (int co = 0; co < CO; ++co) {
                    const float4 w0 = *(const float4*)(wt + co * g.C + c8);
                    const float4 w1 = *(const float4*)(wt + co * g.C + c8 + 4);
#pragma unroll
                    for (int t = 0; t < BFL_PX; ++t) {
                        float a = acc[t][co];
                        a = fmaf(xf[t][0], w0.x, a);
                        a = fmaf(xf[t][1], w0.y, a);
                        a = fmaf(xf[t][2], w0.z, a);
                        a = fmaf(xf[t][3], w0.w, a);
                        a = fmaf(xf[t][4], w1.x, a);
                        a = fmaf(xf[t][5], w1.y, a);
                        a = fmaf(xf[t][6], w1.z, a);
                        a = fmaf(xf[t][7], w1.w, a);
                        acc[t][co] = a;
                    }
                }
            }
        }
    }
    return true;
}

// What the layer onto the frame stores per pixel, Y: float stores x_hat = act(acc); unsigned char stores the grey
// level bn_quantise_u8(act(acc)) and x_hat is never written.  Kernels, walks and grids are the SAME templates for
// both, so the bytes are bn_unit_float_to_u8 of the fp32 output by construction.
template <typename Y>
__device__ __forceinline__ Y bfl_out(float v);
template <>
__device__ __forceinline__ float bfl_out<float>(float v) { return v; }
template <>
__device__ __forceinline__ unsigned char bfl_out<unsigned char>(float v) { return (unsigned char)bn_quantise_u8(v); }

template <int CO, typename Y>
__global__ __launch_bounds__(256) void k_bf16_lastT(const unsigned short* __restrict__ x, const float* __restrict__ w,
                                                    const float* __restrict__ bias, Y* __restrict__ y,
                                                    BnBf16Geom g, int act, float slope, int nchunk, unsigned nitems) {
    extern __shared__ __attribute__((aligned(16))) float s_w[];          // [(r * S + s)][co][ci]
    bfl_stage_weights<CO>(w, s_w, g);
    float bv[CO];
#pragma unroll
    for (int co = 0; co < CO; ++co) bv[co] = bias ? bias[co] : 0.f;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nph = g.stride * g.stride;
    const bn_rsrc_t xr = bn_make_rsrc(x, (size_t)g.N * g.H * g.W * g.C * 2);
    const size_t PQ = (size_t)g.P * g.Q;
    for (unsigned item = blockIdx.x * 4 + wave; item < nitems; item += gridDim.x * 4) {
        const int chunk = (int)(item % nchunk);
        const unsigned rest = item / nchunk;
        const int ph = (int)(rest % nph), n = (int)(rest / nph);
        BfTAxis ay, ax;
        int jy[BFL_PX], jx[BFL_PX];
        bool ok[BFL_PX];
        float acc[BFL_PX][CO];
        if (!bfl_item<CO>(xr, s_w, bv, g, n, ph, chunk, lane, ay, ax, jy, jx, ok, acc)) continue;
#pragma unroll
        for (int t = 0; t < BFL_PX; ++t) {
            if (!ok[t]) continue;
            const size_t pq = (size_t)(ay.o0 + jy[t] * g.stride) * g.Q + ax.o0 + jx[t] * g.stride;
#pragma unroll
            for (int co = 0; co < CO; ++co)
                y[((size_t)n * CO + co) * PQ + pq] = bfl_out<Y>(bn_apply_act(acc[t][co], act, slope));
        }
    }
}

// Stride 2 (the last layer of every shipped architecture): the four phases of one 2 x 2 output block f = 2 q + p read
// the same ceil(R / 2) x ceil(S / 2) input pixels (q - t), so a lane owns one block q of all output channels, reads
// each of those input pixels ONCE (k_bf16_lastT reads it once per phase that uses it) and feeds it to every tap
// (r, s) = (p + 2 t) inside the kernel: 25 tap products from 9 pixel reads for a 5x5 kernel.  Nothing depends on
// the lane but the addresses: the tap loop and the weight reads (LDS broadcasts) are uniform over the workgroup.
// Neighbouring lanes own neighbouring blocks: their input pixels and their 8-byte output pairs are contiguous.
// The reduction order per output pixel is fixed: (t_y, t_x, ci) for the even and for the odd input channels (the two
// halves of one packed FMA), the halves added at the end.  Measured: bound by its LDS weight reads, 200 of 16 bytes per
// block (padding the taps to 6x6 to drop the branches made them 288 and took 1.55 x as long): several blocks per lane
// for every weight read is the next thing to measure.
typedef __attribute__((ext_vector_type(2))) float f32x2_t;
// The 2 x 2 output block q = (qy, qx) of frame n -- shared by k_bf16_lastT_s2 and k_bf16_lastT_s2_sqerr, which scores
// the SAME pre-activations: acc[py][px][co] holds the (even ci, odd ci) halves of output pixel 2 q + p - crop.
template <int CO>
__device__ __forceinline__ void bfl_s2_block(const bn_rsrc_t& xr, const float* s_w, const float (&bv)[CO],
                                             const BnBf16Geom& g, int nty, int ntx, int n, int qy, int qx,
                                             f32x2_t (&acc)[2][2][CO]) {
    // (even ci, odd ci) halves of every sum: the two are one packed FMA (v_pk_fma_f32), added at the end
#pragma unroll
    for (int py = 0; py < 2; ++py)
#pragma unroll
        for (int px = 0; px < 2; ++px)
#pragma unroll
            for (int co = 0; co < CO; ++co) acc[py][px][co] = f32x2_t{bv[co], 0.f};
    const size_t nbase = (size_t)n * g.H * g.W * g.C;
    for (int ty = 0; ty < nty; ++ty) {
        for (int tx = 0; tx < ntx; ++tx) {
            const int ih = qy - ty, iw = qx - tx;
            const bool in = ih >= 0 && ih < g.H && iw >= 0 && iw < g.W;
            const unsigned off = (unsigned)((nbase + ((size_t)ih * g.W + iw) * g.C) * 2);
            for (int c16 = 0; c16 < g.C; c16 += 16) {
                // (selected per piece: an out-of-range marker plus a channel offset would wrap into range)
                const uint4 v0 = bn_buf_load16(xr, in ? off + (unsigned)c16 * 2 : 0xffffffffu);
                const uint4 v1 = bn_buf_load16(xr, in ? off + (unsigned)c16 * 2 + 16 : 0xffffffffu);
                f32x2_t xf[8];
                const unsigned u[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    xf[e] = f32x2_t{__uint_as_float(u[e] << 16), __uint_as_float(u[e] & 0xffff0000u)};
#pragma unroll
                for (int py = 0; py < 2; ++py) {
                    const int r = py + 2 * ty;
                    if (r >= g.R) continue;
#pragma unroll
                    for (int px = 0; px < 2; ++px) {
                        const int sx = px + 2 * tx;
                        if (sx >= g.S) continue;
                        const float* wt = s_w + (size_t)(r * g.S + sx) * CO * g.C + c16;
#pragma unroll
                        for (int co = 0; co < CO; ++co) {
                            f32x2_t a = acc[py][px][co];
#pragma unroll
                            for (int e4 = 0; e4 < 4; ++e4) {
                                const float4 ww = *(const float4*)(wt + co * g.C + 4 * e4);
                                a = __builtin_elementwise_fma(xf[2 * e4], f32x2_t{ww.x, ww.y}, a);
                                a = __builtin_elementwise_fma(xf[2 * e4 + 1], f32x2_t{ww.z, ww.w}, a);
                            }
                            acc[py][px][co] = a;
                        }
                    }
                }
            }
        }
    }
}

// (Y = unsigned char: a lane's two pixels of a row leave as ONE 2-byte store where both are inside the frame and the
// pair sits on a 2-byte boundary, as single bytes otherwise -- odd crops, odd widths, odd bases.)
template <int CO, typename Y>
__global__ __launch_bounds__(256) void k_bf16_lastT_s2(const unsigned short* __restrict__ x,
                                                       const float* __restrict__ w, const float* __restrict__ bias,
                                                       Y* __restrict__ y, BnBf16Geom g, int act, float slope,
                                                       int qy0, int nqy, int qx0, int nqx) {
    extern __shared__ __attribute__((aligned(16))) float s_w[];          // [(r * S + s)][co][ci]
    bfl_stage_weights<CO>(w, s_w, g);
    float bv[CO];
#pragma unroll
    for (int co = 0; co < CO; ++co) bv[co] = bias ? bias[co] : 0.f;
    const bn_rsrc_t xr = bn_make_rsrc(x, (size_t)g.N * g.H * g.W * g.C * 2);
    const size_t PQ = (size_t)g.P * g.Q;
    const int nty = (g.R + 1) / 2, ntx = (g.S + 1) / 2;
    const size_t total = (size_t)g.N * nqy * nqx;
    for (size_t item = (size_t)blockIdx.x * 256 + threadIdx.x; item < total; item += (size_t)gridDim.x * 256) {
        const int qx = qx0 + (int)(item % nqx);
        const size_t rest = item / nqx;
        const int qy = qy0 + (int)(rest % nqy), n = (int)(rest / nqy);
        f32x2_t acc[2][2][CO];
        bfl_s2_block<CO>(xr, s_w, bv, g, nty, ntx, n, qy, qx, acc);
        if constexpr (sizeof(Y) == 1) {
            const int ox = 2 * qx - g.pl;          // px = 0; px = 1 is ox + 1
            const bool in0 = ox >= 0 && ox < g.Q, in1 = ox + 1 >= 0 && ox + 1 < g.Q;
#pragma unroll
            for (int py = 0; py < 2; ++py) {
                const int oy = 2 * qy + py - g.pt;
                if (oy < 0 || oy >= g.P) continue;
#pragma unroll
                for (int co = 0; co < CO; ++co) {
                    const unsigned u0 = bfl_out<Y>(bn_apply_act(acc[py][0][co].x + acc[py][0][co].y, act, slope));
                    const unsigned u1 = bfl_out<Y>(bn_apply_act(acc[py][1][co].x + acc[py][1][co].y, act, slope));
                    // (pointer arithmetic only: with in0 false, p is the byte before the row and is not touched)
                    Y* p = y + (ptrdiff_t)(((size_t)n * CO + co) * PQ + (size_t)oy * g.Q) + ox;
                    if (in0 && in1 && (((uintptr_t)p) & 1u) == 0) {
                        *reinterpret_cast<unsigned short*>(p) = (unsigned short)(u0 | (u1 << 8));
                    } else {
                        if (in0) p[0] = (Y)u0;
                        if (in1) p[1] = (Y)u1;
                    }
                }
            }
        } else {
#pragma unroll
            for (int py = 0; py < 2; ++py) {
                const int oy = 2 * qy + py - g.pt;
                if (oy < 0 || oy >= g.P) continue;
#pragma unroll
                for (int px = 0; px < 2; ++px) {
                    const int ox = 2 * qx + px - g.pl;
                    if (ox < 0 || ox >= g.Q) continue;
#pragma unroll
                    for (int co = 0; co < CO; ++co)
                        y[((size_t)n * CO + co) * PQ + (size_t)oy * g.Q + ox] =
                            bfl_out<Y>(bn_apply_act(acc[py][px][co].x + acc[py][px][co].y, act, slope));
                }
            }
        }
    }
}

template <typename Y>
static int bf16_lastT_s2(const unsigned short* xs, const float* w, const float* bias, Y* y, const BnBf16Geom& g,
                         int act, float slope, hipStream_t st) {
    // blocks q with an output pixel: 2 q + p - crop in [0, P) for p = 0 or 1
    const int qy0 = g.pt / 2, qy1 = (g.pt + g.P - 1) / 2, qx0 = g.pl / 2, qx1 = (g.pl + g.Q - 1) / 2;
    const int nqy = qy1 - qy0 + 1, nqx = qx1 - qx0 + 1;
    const size_t total = (size_t)g.N * nqy * nqx;
    const size_t blocks = (total + 255) / 256 < BFL_MAX_BLOCKS ? (total + 255) / 256 : BFL_MAX_BLOCKS;
    const size_t lds = (size_t)g.R * g.S * g.K * g.C * sizeof(float);
    const dim3 grid((unsigned)blocks);
#define BFL_GO2(CO)                                                                                             \
    BN_LAUNCH_MAIN((k_bf16_lastT_s2<CO, Y>), grid, dim3(256), lds, st, xs, w, bias, y, g, act, slope, qy0, nqy, qx0, nqx)
    switch (g.K) {
        case 1: BFL_GO2(1); break;
        case 2: BFL_GO2(2); break;
        case 3: BFL_GO2(3); break;
        default: BFL_GO2(4); break;
    }
#undef BFL_GO2
    BN_LAUNCH_CHECK();
    return 0;
}

template <typename Y>
static int bf16_lastT(const void* x, const float* w, const float* bias, Y* y, const BnBf16Geom& g, int act,
                      float slope, hipStream_t st) {
    if (!bn_bf16_lastT_ok(g)) return BN_E_SHAPE;
    if (g.stride == 2) return bf16_lastT_s2<Y>((const unsigned short*)x, w, bias, y, g, act, slope, st);
    const int cy = (g.P + g.stride - 1) / g.stride, cx = (g.Q + g.stride - 1) / g.stride;
    const int nchunk = (cy * cx + 64 * BFL_PX - 1) / (64 * BFL_PX);
    const size_t items = (size_t)g.N * g.stride * g.stride * nchunk;
    if (items >= ((size_t)1 << 31)) return BN_E_SHAPE;
    const size_t blocks = (items + 3) / 4 < BFL_MAX_BLOCKS ? (items + 3) / 4 : BFL_MAX_BLOCKS;
    const size_t lds = (size_t)g.R * g.S * g.K * g.C * sizeof(float);
    const dim3 grid((unsigned)blocks);
    const unsigned short* xs = (const unsigned short*)x;
#define BFL_GO(CO)                                                                                              \
    BN_LAUNCH_MAIN((k_bf16_lastT<CO, Y>), grid, dim3(256), lds, st, xs, w, bias, y, g, act, slope, nchunk,       \
                   (unsigned)items)
    switch (g.K) {
        case 1: BFL_GO(1); break;
        case 2: BFL_GO(2); break;
        case 3: BFL_GO(3); break;
        default: BFL_GO(4); break;
    }
#undef BFL_GO
    BN_LAUNCH_CHECK();
    return 0;
}

int bn_launch_bf16_lastT(const void* x, const float* w, const float* bias, float* y, const BnBf16Geom& g, int act,
                         float slope, hipStream_t st) {
    return bf16_lastT<float>(x, w, bias, y, g, act, slope, st);
}

// The layer onto the frame writing stored grey levels (uint8) instead of x_hat.
int bn_launch_bf16_lastT_u8(const void* x, const float* w, const float* bias, unsigned char* y, const BnBf16Geom& g,
                            int act, float slope, hipStream_t st) {
    return bf16_lastT<unsigned char>(x, w, bias, y, g, act, slope, st);
}

// ------------------------------------------------------------------------------------------ last layer, scored
// The layer onto the frame fused with the per-frame squared error: the epilogue forms (act(acc) - target)^2 * mask
// where the kernels above store act(acc), and x_hat is never written.  acc comes from bfl_s2_block / bfl_item, the
// device code of the unfused kernels.  What differs is the walk: a workgroup's 256 lanes (4 waves) cover ONE piece
// of ONE frame at a time -- piece blockIdx.x of P, frames blockIdx.y, blockIdx.y + gridDim.y, .. (the weights are
// still staged once per workgroup) -- and leave that piece's sum in part[n][piece]: lane order (py, px, co) or
// (t, co), wave shuffle tree, fixed LDS combine.  P and the pieces depend on the geometry of one frame alone, so a
// frame scored alone gives the bits it gives in a batch.  bn_launch_frame_err_finish adds the P partials left to
// right (P == 1: the workgroup writes out[n] itself).  No atomics.
__device__ __forceinline__ float bfl_sq_term(float v, const void* __restrict__ target, bool u8,
                                             const float* __restrict__ mask, size_t i) {
    const float t = u8 ? (float)((const unsigned char*)target)[i] / 255.f : ((const float*)target)[i];
    const float d = v - t;
    const float e = d * d;
    return mask ? e * mask[i] : e;
}

__device__ __forceinline__ float bfl_block_sum(float acc, float* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

template <int CO, bool U8>
__global__ __launch_bounds__(256) void k_bf16_lastT_s2_sqerr(const unsigned short* __restrict__ x,
                                                             const float* __restrict__ w,
                                                             const float* __restrict__ bias,
                                                             const void* __restrict__ target,
                                                             const float* __restrict__ mask, float* __restrict__ dst,
                                                             BnBf16Geom g, int act, float slope, int qy0, int nqy,
                                                             int qx0, int nqx, float scale) {
    extern __shared__ __attribute__((aligned(16))) float s_w[];          // [(r * S + s)][co][ci]
    __shared__ float red[4];
    bfl_stage_weights<CO>(w, s_w, g);
    float bv[CO];
#pragma unroll
    for (int co = 0; co < CO; ++co) bv[co] = bias ? bias[co] : 0.f;
    const bn_rsrc_t xr = bn_make_rsrc(x, (size_t)g.N * g.H * g.W * g.C * 2);
    const size_t PQ = (size_t)g.P * g.Q;
    const int nty = (g.R + 1) / 2, ntx = (g.S + 1) / 2;
    const unsigned q = blockIdx.x * 256 + threadIdx.x;          // this lane's block of every frame
    const bool have = q < (unsigned)(nqy * nqx);
    const int qy = qy0 + (int)(q / nqx), qx = qx0 + (int)(q % nqx);
    for (int n = blockIdx.y; n < g.N; n += gridDim.y) {          // (uniform over the workgroup: barriers inside)
        float s = 0.f;
        if (have) {
            f32x2_t acc[2][2][CO];
            bfl_s2_block<CO>(xr, s_w, bv, g, nty, ntx, n, qy, qx, acc);
#pragma unroll
            for (int py = 0; py < 2; ++py) {
                const int oy = 2 * qy + py - g.pt;
                if (oy < 0 || oy >= g.P) continue;
#pragma unroll
                for (int px = 0; px < 2; ++px) {
                    const int ox = 2 * qx + px - g.pl;
                    if (ox < 0 || ox >= g.Q) continue;
#pragma unroll
                    for (int co = 0; co < CO; ++co)
                        s += bfl_sq_term(bn_apply_act(acc[py][px][co].x + acc[py][px][co].y, act, slope), target, U8,
                                         mask, ((size_t)n * CO + co) * PQ + (size_t)oy * g.Q + ox);
                }
            }
        }
        const float tot = bfl_block_sum(s, red);
        if (threadIdx.x == 0) dst[(size_t)n * gridDim.x + blockIdx.x] = gridDim.x == 1 ? tot * scale : tot;
        __syncthreads();          // red is written again for the next frame
    }
}

template <int CO, bool U8>
__global__ __launch_bounds__(256) void k_bf16_lastT_sqerr(const unsigned short* __restrict__ x,
                                                          const float* __restrict__ w, const float* __restrict__ bias,
                                                          const void* __restrict__ target,
                                                          const float* __restrict__ mask, float* __restrict__ dst,
                                                          BnBf16Geom g, int act, float slope, int nchunk,
                                                          unsigned frame_items, float scale) {
    extern __shared__ __attribute__((aligned(16))) float s_w[];          // [(r * S + s)][co][ci]
    __shared__ float red[4];
    bfl_stage_weights<CO>(w, s_w, g);
    float bv[CO];
#pragma unroll
    for (int co = 0; co < CO; ++co) bv[co] = bias ? bias[co] : 0.f;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bn_rsrc_t xr = bn_make_rsrc(x, (size_t)g.N * g.H * g.W * g.C * 2);
    const size_t PQ = (size_t)g.P * g.Q;
    const unsigned item = blockIdx.x * 4 + wave;          // this wave's (phase, chunk) of every frame
    const int chunk = (int)(item % nchunk), ph = (int)(item / nchunk);
    for (int n = blockIdx.y; n < g.N; n += gridDim.y) {          // (uniform over the workgroup: barriers inside)
        float s = 0.f;
        BfTAxis ay, ax;
        int jy[BFL_PX], jx[BFL_PX];
        bool ok[BFL_PX];
        float acc[BFL_PX][CO];
        if (item < frame_items && bfl_item<CO>(xr, s_w, bv, g, n, ph, chunk, lane, ay, ax, jy, jx, ok, acc)) {
#pragma unroll
            for (int t = 0; t < BFL_PX; ++t) {
                if (!ok[t]) continue;
                const size_t pq = (size_t)(ay.o0 + jy[t] * g.stride) * g.Q + ax.o0 + jx[t] * g.stride;
#pragma unroll
                for (int co = 0; co < CO; ++co)
                    s += bfl_sq_term(bn_apply_act(acc[t][co], act, slope), target, U8, mask,
                                     ((size_t)n * CO + co) * PQ + pq);
            }
        }
        const float tot = bfl_block_sum(s, red);
        if (threadIdx.x == 0) dst[(size_t)n * gridDim.x + blockIdx.x] = gridDim.x == 1 ? tot * scale : tot;
        __syncthreads();          // red is written again for the next frame
    }
}

// How the scored layer cuts ONE frame up: the ONE plan that the workspace query and the launch both go by.
struct BflErrPlan { int qy0, nqy, qx0, nqx, nchunk; unsigned frame_items, parts; };
static BflErrPlan bfl_err_plan(const BnBf16Geom& g) {
    BflErrPlan p{};
    if (g.stride == 2) {
        // blocks q with an output pixel: 2 q + p - crop in [0, P) for p = 0 or 1 (bf16_lastT_s2)
        p.qy0 = g.pt / 2;
        p.qx0 = g.pl / 2;
        p.nqy = (g.pt + g.P - 1) / 2 - p.qy0 + 1;
        p.nqx = (g.pl + g.Q - 1) / 2 - p.qx0 + 1;
        p.parts = (unsigned)(((size_t)p.nqy * p.nqx + 255) / 256);
    } else {
        const int cy = (g.P + g.stride - 1) / g.stride, cx = (g.Q + g.stride - 1) / g.stride;
        p.nchunk = (cy * cx + 64 * BFL_PX - 1) / (64 * BFL_PX);
        p.frame_items = (unsigned)(g.stride * g.stride * p.nchunk);
        p.parts = (p.frame_items + 3) / 4;
    }
    return p;
}

size_t bn_bf16_lastT_sqerr_ws_bytes(const BnBf16Geom& g) {
    if (!bn_bf16_lastT_ok(g)) return 0;
    const unsigned parts = bfl_err_plan(g).parts;
    return parts == 1 ? 0 : (size_t)g.N * parts * sizeof(float);
}

int bn_launch_bf16_lastT_sqerr(const void* x, const float* w, const float* bias, const void* target, int target_is_u8,
                               const float* mask, float* out, const BnBf16Geom& g, int act, float slope, float scale,
                               void* ws, hipStream_t st) {
    if (!bn_bf16_lastT_ok(g)) return BN_E_SHAPE;
    const BflErrPlan p = bfl_err_plan(g);
    // (bn_bf16_lastT_ok bounds N P Q below 2^31, so parts is far below the grid's limit)
    const unsigned gy = (unsigned)min(g.N, max(1, (int)(BFL_MAX_BLOCKS / p.parts)));
    const dim3 grid(p.parts, gy);
    const size_t lds = (size_t)g.R * g.S * g.K * g.C * sizeof(float);
    const unsigned short* xs = (const unsigned short*)x;
    float* dst = p.parts == 1 ? out : (float*)ws;
#define BFL_ERR2(CO, U8)                                                                                          \
    BN_LAUNCH_MAIN((k_bf16_lastT_s2_sqerr<CO, U8>), grid, dim3(256), lds, st, xs, w, bias, target, mask, dst, g, act, \
                   slope, p.qy0, p.nqy, p.qx0, p.nqx, scale)
#define BFL_ERR(CO, U8)                                                                                           \
    BN_LAUNCH_MAIN((k_bf16_lastT_sqerr<CO, U8>), grid, dim3(256), lds, st, xs, w, bias, target, mask, dst, g, act,    \
                   slope, p.nchunk, p.frame_items, scale)
#define BFL_ERR_CO(GO, U8)                                                                                        \
    switch (g.K) {                                                                                                \
        case 1: GO(1, U8); break;                                                                                 \
        case 2: GO(2, U8); break;                                                                                 \
        case 3: GO(3, U8); break;                                                                                 \
        default: GO(4, U8); break;                                                                                \
    }
    if (g.stride == 2) {
        if (target_is_u8) { BFL_ERR_CO(BFL_ERR2, true) } else { BFL_ERR_CO(BFL_ERR2, false) }
    } else {
        if (target_is_u8) { BFL_ERR_CO(BFL_ERR, true) } else { BFL_ERR_CO(BFL_ERR, false) }
    }
#undef BFL_ERR_CO
#undef BFL_ERR
#undef BFL_ERR2
    BN_LAUNCH_CHECK();
    if (p.parts > 1) return bn_launch_frame_err_finish(dst, out, g.N, p.parts, scale, st);
    return 0;
}
