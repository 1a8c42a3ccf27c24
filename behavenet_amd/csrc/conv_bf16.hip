// Inference-only conv encoder stack on bf16 operands with fp32 accumulation ("bf16 encoder").
//
//   k_bf16_pack_w   fp32 weights (K, C, R, S) -> bf16 [K][(r * S + s) * C + c]: the reduction index of the
//                   implicit GEMM contiguous per output channel
//   k_bf16_first    layer 1 (1..4 frame channels, fp32 or uint8 / 255 frames, NCHW): fp32 FMAs on the vector
//                   unit, bias + activation, ONE rounding to bf16, output in the private layout
//   k_bf16_conv     body layers: implicit GEMM on v_mfma_f32_32x32x16_bf16, rows = output pixels, columns =
//                   output channels, reduction over (tap, input channel) in that fixed order; stride, kernel
//                   size, padding and map sizes are run-time arguments
//
// Private activation layout: bf16 (N, H, W, C), channels last, so that the 8 input channels a lane feeds to
// one MFMA are one 16-byte load.  It exists between the layers of one bn_conv2d_*_bf16 chain only.
// No atomics and no split reductions: two launches on the same operands give the same bits.
#include "bn_bf16.h"      // the rounding rule, the buffer loads and the tile shape, shared with conv_bf16_dec.hip

// ------------------------------------------------------------------------------------------ weights
// One workgroup: PACK_CC input channels of one output channel k.  Their C x RS floats are contiguous in the source
// and their RS x C bf16 are rows of the destination: read in source order into LDS, written in destination order.
#define PACK_CC 64
__global__ __launch_bounds__(256) void k_bf16_pack_w(const float* __restrict__ w, unsigned short* __restrict__ wp,
                                                     int K, int C, int RS) {
    __shared__ float s_t[PACK_CC * 25];
    const int k = blockIdx.x, c0 = blockIdx.y * PACK_CC;
    const int cc = min(PACK_CC, C - c0);
    const float* src = w + ((size_t)k * C + c0) * RS;
    for (int i = threadIdx.x; i < cc * RS; i += 256) s_t[i] = src[i];          // [c][tap]
    __syncthreads();
    unsigned short* dst = wp + (size_t)k * C * RS + c0;
    for (int i = threadIdx.x; i < cc * RS; i += 256) {
        const int tap = i / cc, c = i - tap * cc;
        dst[(size_t)tap * C + c] = (unsigned short)bn_f32_to_bf16(s_t[c * RS + tap]);
    }
}

int bn_launch_bf16_pack_w(const float* w, void* wp, const BnBf16Geom& g, hipStream_t st) {
    if (g.R * g.S > 25 || (g.C + PACK_CC - 1) / PACK_CC > 65535) return BN_E_SHAPE;
    const dim3 grid((unsigned)g.K, (unsigned)((g.C + PACK_CC - 1) / PACK_CC));
    hipLaunchKernelGGL(k_bf16_pack_w, grid, dim3(256), 0, st, w, (unsigned short*)wp, g.K, g.C, g.R * g.S);
    BN_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------ first layer
// A workgroup owns TP output rows x 4 TQ4 output columns of one frame for all K output channels.  It stages the
// input patch those need ONCE into LDS as floats (the uint8 / 255 division happens there, once per input value,
// padding as zeros) next to the layer's weights, [c][r][s][k] floats with the bias behind them.  A thread owns
// 16 output channels of 4 output columns TQ4 apart (so that neighbouring lanes read neighbouring patch columns
// and write neighbouring 32-byte pieces of the channels-last output).
#define BF1_PX 4
#define BF1_CO 16
struct Bf1Plan { int TQ4, TP, IH, IW; size_t lds; bool ok; };
static Bf1Plan bf16_first_plan(const BnBf16Geom& g) {
    Bf1Plan p{};
    if (!(g.C >= 1 && g.C <= 4 && g.K % BF1_CO == 0 && g.K / BF1_CO <= 64 && g.R <= 5 && g.S <= 5 &&
          (size_t)g.N * g.P * g.Q * g.K < ((size_t)1 << 40)))
        return p;
    const int ncg = g.K / BF1_CO, q4 = (g.Q + BF1_PX - 1) / BF1_PX;
    p.TQ4 = q4 < 256 / ncg ? q4 : 256 / ncg;
    int tp = 256 / (p.TQ4 * ncg);
    if (tp > g.P) tp = g.P;
    for (; tp >= 1; --tp) {
        p.TP = tp;
        p.IH = (tp - 1) * g.stride + g.R;
        p.IW = (BF1_PX * p.TQ4 - 1) * g.stride + g.S;
        p.lds = ((size_t)g.C * g.R * g.S * g.K + g.K + (size_t)g.C * p.IH * p.IW) * sizeof(float);
        if (p.lds <= 60 * 1024) {
            p.ok = true;
            return p;
        }
    }
    return p;
}
bool bn_bf16_first_ok(const BnBf16Geom& g) { return bf16_first_plan(g).ok; }

template <bool U8>
__global__ __launch_bounds__(256) void k_bf16_first(const void* __restrict__ xv, const float* __restrict__ w,
                                                    const float* __restrict__ bias, unsigned short* __restrict__ y,
                                                    BnBf16Geom g, int TQ4, int TP, int IH, int IW, int act,
                                                    float slope) {
    extern __shared__ float s_w[];
    const int taps = g.C * g.R * g.S;
    float* s_b = s_w + taps * g.K;
    float* s_x = s_b + g.K;
    // which tile
    const int ntq = ((g.Q + BF1_PX - 1) / BF1_PX + TQ4 - 1) / TQ4, ntp = (g.P + TP - 1) / TP;
    unsigned bid = blockIdx.x;
    const int qs = (int)(bid % ntq) * BF1_PX * TQ4;
    bid /= ntq;
    const int p0 = (int)(bid % ntp) * TP;
    const int n = (int)(bid / ntp);

    for (int i = threadIdx.x; i < taps * g.K; i += 256) {
        const int k = i % g.K, t = i / g.K;
        s_w[i] = w[(size_t)k * taps + t];          // (K, C, R, S) -> [c r s][k]
    }
    for (int i = threadIdx.x; i < g.K; i += 256) s_b[i] = bias ? bias[i] : 0.f;
    const size_t plane = (size_t)g.H * g.W;
    const float* xf = (const float*)xv + (size_t)n * g.C * plane;
    const unsigned char* xb = (const unsigned char*)xv + (size_t)n * g.C * plane;
    for (int i = threadIdx.x; i < g.C * IH * IW; i += 256) {
        const int ix = i % IW, rest = i / IW;
        const int iy = rest % IH, c = rest / IH;
        const int ih = p0 * g.stride - g.pt + iy, iw = qs * g.stride - g.pl + ix;
        float f = 0.f;
        if (ih >= 0 && ih < g.H && iw >= 0 && iw < g.W) {
            const size_t off = c * plane + (size_t)ih * g.W + iw;
            f = U8 ? (float)xb[off] / 255.f : xf[off];
        }
        s_x[i] = f;
    }
    __syncthreads();

    const int ncg = g.K / BF1_CO;
    const int cg = threadIdx.x % ncg;
    const int q4 = (threadIdx.x / ncg) % TQ4;
    const int row = threadIdx.x / (ncg * TQ4);
    const int p = p0 + row;
    if (row >= TP || p >= g.P) return;

    float acc[BF1_PX][BF1_CO];
#pragma unroll
    for (int t = 0; t < BF1_PX; ++t)
#pragma unroll
        for (int k = 0; k < BF1_CO; ++k) acc[t][k] = s_b[cg * BF1_CO + k];

    const float* wrow = s_w + cg * BF1_CO;
    for (int c = 0; c < g.C; ++c) {
        for (int r = 0; r < g.R; ++r) {
            const float* xrow = s_x + (c * IH + row * g.stride + r) * IW + q4 * g.stride;
            for (int s = 0; s < g.S; ++s) {
                float v[BF1_PX];
#pragma unroll
                for (int t = 0; t < BF1_PX; ++t) v[t] = xrow[t * TQ4 * g.stride + s];
                const float4* w4 = (const float4*)(wrow + (size_t)((c * g.R + r) * g.S + s) * g.K);
#pragma unroll
                for (int k4 = 0; k4 < BF1_CO / 4; ++k4) {
                    const float4 ww = w4[k4];
#pragma unroll
                    for (int t = 0; t < BF1_PX; ++t) {
                        acc[t][4 * k4 + 0] = fmaf(v[t], ww.x, acc[t][4 * k4 + 0]);
                        acc[t][4 * k4 + 1] = fmaf(v[t], ww.y, acc[t][4 * k4 + 1]);
                        acc[t][4 * k4 + 2] = fmaf(v[t], ww.z, acc[t][4 * k4 + 2]);
                        acc[t][4 * k4 + 3] = fmaf(v[t], ww.w, acc[t][4 * k4 + 3]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < BF1_PX; ++t) {
        const int q = qs + q4 + t * TQ4;
        if (q >= g.Q) continue;
        unsigned pk[BF1_CO / 2];
#pragma unroll
        for (int k = 0; k < BF1_CO; k += 2) {
            const unsigned lo = bn_f32_to_bf16(bn_apply_act(acc[t][k], act, slope));
            const unsigned hi = bn_f32_to_bf16(bn_apply_act(acc[t][k + 1], act, slope));
            pk[k / 2] = lo | (hi << 16);
        }
        uint4* dst = (uint4*)(y + (((size_t)n * g.P + p) * g.Q + q) * g.K + cg * BF1_CO);
        dst[0] = make_uint4(pk[0], pk[1], pk[2], pk[3]);
        dst[1] = make_uint4(pk[4], pk[5], pk[6], pk[7]);
    }
}

int bn_launch_bf16_first(const void* x, int x_is_u8, const float* w, const float* bias, void* y, const BnBf16Geom& g,
                         int act, float slope, hipStream_t st) {
    const Bf1Plan pl = bf16_first_plan(g);
    if (!pl.ok) return BN_E_SHAPE;
    const size_t ntq = ((g.Q + BF1_PX - 1) / BF1_PX + pl.TQ4 - 1) / pl.TQ4, ntp = (g.P + pl.TP - 1) / pl.TP;
    const size_t blocks = ntq * ntp * g.N;
    if (blocks >= ((size_t)1 << 31)) return BN_E_SHAPE;
    const dim3 grid((unsigned)blocks);
    if (x_is_u8)
        BN_LAUNCH_MAIN(k_bf16_first<true>, grid, dim3(256), pl.lds, st, x, w, bias, (unsigned short*)y, g, pl.TQ4, pl.TP,
                       pl.IH, pl.IW, act, slope);
    else
        BN_LAUNCH_MAIN(k_bf16_first<false>, grid, dim3(256), pl.lds, st, x, w, bias, (unsigned short*)y, g, pl.TQ4, pl.TP,
                       pl.IH, pl.IW, act, slope);
    BN_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------ body layers
// Implicit GEMM: D[m][k] = sum_kk A[m][kk] B[kk][k], m = (n, p, q) an output pixel, kk = (r * S + s) * C + c.
// A workgroup of 4 waves (2 x 2) owns a (64 WM) x 64 tile; a wave WM x 1 MFMA tiles of 32 x 32.  Per step 64
// values of kk are staged through LDS (rows padded to 72 bf16 = 144 bytes: the 16-byte fragment reads of 16
// consecutive rows fall on 16 distinct 4-bank slots); the loads of steps t + 1 and t + 2 are in flight while step t
// runs on the matrix cores.  C % 16 == 0: one MFMA step is 16 consecutive kk, which then never straddle a tap, and
// every 16-byte piece (8 channels) is aligned and within one pixel.  Out-of-range pieces (zero padding, the
// tails of m, k and kk) are staged as zeros and never read from memory (bounds-checked buffer loads).
// (BFC_BK / BFC_LD / BFC_BN and the buffer-load helpers: bn_bf16.h)
bool bn_bf16_conv_ok(const BnBf16Geom& g) {
    // (both operands are addressed with 32-bit byte offsets)
    return g.C % 16 == 0 && g.K >= 1 && g.R <= 5 && g.S <= 5 &&
           (size_t)g.N * g.H * g.W * g.C * 2 < ((size_t)1 << 31) && (size_t)g.K * g.R * g.S * g.C * 2 < ((size_t)1 << 31) &&
           (size_t)g.N * g.P * g.Q < ((size_t)1 << 31) && (size_t)g.N * g.P * g.Q * g.K < ((size_t)1 << 40);
}

template <int WM, bool OUT_F32>
__global__ __launch_bounds__(256) void k_bf16_conv(const unsigned short* __restrict__ x,
                                                   const unsigned short* __restrict__ wp,
                                                   const float* __restrict__ bias, void* __restrict__ yv,
                                                   BnBf16Geom g, int act, float slope) {
    constexpr int BM = 64 * WM;
    constexpr int NA = BM / 32, NB = BFC_BN / 32;
    __shared__ __attribute__((aligned(16))) unsigned short s_all[(BM + BFC_BN) * BFC_LD];
    unsigned short* s_a = s_all;
    unsigned short* s_b = s_all + BM * BFC_LD;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int pc = tid & 7, row0 = tid >> 3;
    const int PQ = g.P * g.Q;
    const int Mtot = g.N * PQ;
    const int Ktot = g.R * g.S * g.C;
    const int m0 = blockIdx.x * BM, k0blk = blockIdx.y * BFC_BN;

    // the rows this thread stages
    int ih0[NA], iw0[NA];
    size_t abase[NA];
    bool mok[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int m = m0 + row0 + 32 * i;
        mok[i] = m < Mtot;
        const int mm = mok[i] ? m : 0;
        const int n = mm / PQ, pq = mm - n * PQ;
        const int p = pq / g.Q, q = pq - p * g.Q;
        ih0[i] = p * g.stride - g.pt;
        iw0[i] = q * g.stride - g.pl;
        abase[i] = (size_t)n * g.H * g.W * g.C;
    }
    size_t bbase[NB];
    bool kok[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int k = k0blk + row0 + 32 * j;
        kok[j] = k < g.K;
        bbase[j] = (size_t)(kok[j] ? k : 0) * Ktot;
    }
    // position of this thread's piece in the reduction: kk = (r * S + s) * C + c
    int kk = pc * 8;
    int c = kk % g.C, tap = kk / g.C;
    int r = tap / g.S, s = tap - r * g.S;

    const bn_rsrc_t xr = bn_make_rsrc(x, (size_t)g.N * g.H * g.W * g.C * 2);
    const bn_rsrc_t wr = bn_make_rsrc(wp, (size_t)g.K * Ktot * 2);
    auto fetch = [&](uint4 (&ra)[NA], uint4 (&rb)[NB]) {
        const bool kin = kk < Ktot;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int ih = ih0[i] + r, iw = iw0[i] + s;
            const bool ok = kin && mok[i] && ih >= 0 && ih < g.H && iw >= 0 && iw < g.W;
            // buffer loads: a piece that is padding or a tail gets an offset past the operand's last byte, for
            // which the hardware returns zeros without touching memory -- no branch around the load (the compiler
            // would wait for each such load on its own) and nothing outside the operand is ever read
            const unsigned off = ok ? (unsigned)((abase[i] + ((size_t)ih * g.W + iw) * g.C + c) * 2) : 0xffffffffu;
            ra[i] = bn_buf_load16(xr, off);
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const unsigned off = (kin && kok[j]) ? (unsigned)((bbase[j] + kk) * 2) : 0xffffffffu;
            rb[j] = bn_buf_load16(wr, off);
        }
    };
    auto advance = [&]() {
        kk += BFC_BK;
        c += BFC_BK;
        while (c >= g.C) {
            c -= g.C;
            if (++s == g.S) { s = 0; ++r; }
        }
    };

    f32x16_t acc[WM];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;

    const int nsteps = (Ktot + BFC_BK - 1) / BFC_BK;
    const int fr = lane & 31, fh = lane >> 5;
    // one step: the register set loaded two steps ago goes to LDS and is refilled for the step after next, so
    // that two steps' loads are in flight while the matrix cores work (the short top layers run one workgroup
    // per CU and would otherwise pay a full memory latency per step).  Two NAMED sets: no run-time indexing.
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
    fetch(ra0, rb0);
    if (nsteps > 1) {
        advance();
        fetch(ra1, rb1);
    }
    for (int step = 0; step < nsteps; step += 2) {
        do_step(ra0, rb0, step + 2 < nsteps);
        if (step + 1 < nsteps) do_step(ra1, rb1, step + 3 < nsteps);
    }

    // epilogue: lane = output channel, registers = output pixels
    const int k = k0blk + wn * 32 + fr;
    if (k >= g.K) return;
    const float bv = bias ? bias[k] : 0.f;
#pragma unroll
    for (int i = 0; i < WM; ++i) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int m = m0 + wm * 32 * WM + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * fh;
            if (m >= Mtot) continue;
            const float v = bn_apply_act(acc[i][e] + bv, act, slope);
            if (OUT_F32) {
                const int n = m / PQ, pq = m - n * PQ;
                ((float*)yv)[((size_t)n * g.K + k) * PQ + pq] = v;
            } else {
                ((unsigned short*)yv)[(size_t)m * g.K + k] = (unsigned short)bn_f32_to_bf16(v);
            }
        }
    }
}

int bn_launch_bf16_conv(const void* x, const void* wp, const float* bias, void* y, int out_f32, const BnBf16Geom& g,
                        int act, float slope, hipStream_t st) {
    const size_t M = (size_t)g.N * g.P * g.Q;
    const unsigned gy = (unsigned)((g.K + BFC_BN - 1) / BFC_BN);
    const unsigned short* xs = (const unsigned short*)x;
    const unsigned short* ws = (const unsigned short*)wp;
    // the large tile where it still fills the chip twice over, the small one for the short layers at the top
    if (((M + 127) / 128) * gy >= 512) {
        const dim3 grid((unsigned)((M + 127) / 128), gy);
        if (out_f32)
            BN_LAUNCH_MAIN((k_bf16_conv<2, true>), grid, dim3(256), 0, st, xs, ws, bias, y, g, act, slope);
        else
            BN_LAUNCH_MAIN((k_bf16_conv<2, false>), grid, dim3(256), 0, st, xs, ws, bias, y, g, act, slope);
    } else {
        const dim3 grid((unsigned)((M + 63) / 64), gy);
        if (out_f32)
            BN_LAUNCH_MAIN((k_bf16_conv<1, true>), grid, dim3(256), 0, st, xs, ws, bias, y, g, act, slope);
        else
            BN_LAUNCH_MAIN((k_bf16_conv<1, false>), grid, dim3(256), 0, st, xs, ws, bias, y, g, act, slope);
    }
    BN_LAUNCH_CHECK();
    return 0;
}
