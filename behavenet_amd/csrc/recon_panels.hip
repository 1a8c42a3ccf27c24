// Frames and their reconstruction -> the strips of a reconstruction movie in one pass (DESIGN.md section 4,
// "reconstruction movies"): per frame n and row y three panels of C W bytes, the channels side by side,
//
//   o  = orig[n, c, y, x]                       fp32 unit float, or stored uint8 as value / 255.f
//   om = mask ? o * mask[n or 0, c, y, x] : o   (the original alone is masked)
//   r  = recon[n, c, y, x]                      fp32 unit float, or uint8 grey level as value / 255.f
//
//   panel 0: show_orig ? bn_quantise_u8(om) : 0          (no mask + uint8 orig: the stored byte, the same value)
//   panel 1: recon uint8 ? the byte : bn_quantise_u8(r)
//   panel 2: bn_quantise_u8(0.5f + (om - r))
//
//   out[n out_frame_stride + y (3 C W) + p (C W) + c W + x]
//
// Every step is an fp32 operation of its own -- o * mask does not contract with the subtraction -- so the rule is
// numpy's float32 arithmetic bit for bit.  A launch writes each byte of its strip once and nothing else: with
// out_frame_stride > 3 C H W it fills one row of a movie of several rows.
//
// HBM-bound: C H W (4 or 1) bytes of each operand read per frame, 3 C H W written.  A thread owns 16 consecutive
// pixels j = c W + x of one row, i.e. 16 consecutive output bytes in each of the three panels: it reads its operands
// ONCE and every thread does the same work (a thread per panel would read orig and mask twice, and the three panels'
// paths would serialise inside a wave).  With `out`, the stride and the panel width C W on 16-byte boundaries the
// panels leave in three 16-byte stores; where the 16 pixels lie inside one channel and the operands sit on a 16-byte
// boundary they arrive in 16-byte loads (four per fp32 operand, one per uint8 one), otherwise -- a segment that
// straddles two channels (W % 16 != 0), an operand off alignment -- pixel by pixel.  Without that alignment of the
// output the bytes are stored one by one.  rp_level is the only arithmetic, so every route gives the same bytes.
//
// value / 255.f of a uint8 operand is a true division, a dozen instructions of which 16 or 32 per thread cost as much
// as the memory traffic (measured: 22.7 us whatever the bytes).  It is a function of the byte alone, so each block
// computes the 256 quotients once, by that same division, into LDS and a pixel looks its quotient up: the same bits.
//
// The block is (bx, 256 / bx) as in frame_mosaic.hip: bx threads walk the segments of a row, blockIdx.x counts row
// groups.  32-bit arithmetic inside a frame, size_t across frames.
#include "bn_common.h"
#include "bn_launch.h"

#define RP_THREADS 256
#define RP_SEG 16          // pixels a thread owns: 16 output bytes in each panel

struct RpArgs {
    const void* orig;
    const void* recon;
    const float* mask;
    unsigned char* out;
    size_t out_frame_stride;
    int H, W, show_orig, mask_per_frame;
    unsigned rows, PW, OW, CHW, segs;          // rows = N H, PW = C W, OW = 3 PW, segs = ceil(PW / 16)
};

// one grey level of panel p from the raw operands (the *_f of fp32 operands, the *_b of uint8 ones; m for a mask);
// unit[b] = (float)b / 255.f
template <bool OU8, bool RU8>
__device__ __forceinline__ unsigned rp_level(unsigned p, bool show_orig, bool masked, const float* unit, float o_f,
                                             unsigned o_b, float m, float r_f, unsigned r_b) {
#pragma clang fp contract(off)
    if (p == 1) return RU8 ? r_b : bn_quantise_u8(r_f);
    if (p == 0 && !show_orig) return 0u;
    const float o = OU8 ? unit[o_b] : o_f;
    const float om = masked ? o * m : o;
    if (p == 0) return (OU8 && !masked) ? o_b : bn_quantise_u8(om);
    const float r = RU8 ? unit[r_b] : r_f;
    const float d = om - r;
    return bn_quantise_u8(0.5f + d);
}

// the raw operands of pixel j = c W + x of row y of the frame whose operands start at element `at` (its mask at `mat`)
template <bool OU8, bool RU8>
__device__ __forceinline__ void rp_pixel(const RpArgs& a, size_t at, size_t mat, unsigned y, unsigned j, float& o_f,
                                         unsigned& o_b, float& m, float& r_f, unsigned& r_b) {
    const unsigned c = j / (unsigned)a.W, x = j - c * (unsigned)a.W;
    const unsigned i = (c * (unsigned)a.H + y) * (unsigned)a.W + x;
    o_f = 0.f, m = 1.f, r_f = 0.f, o_b = 0u, r_b = 0u;
    if (OU8) o_b = ((const unsigned char*)a.orig)[at + i]; else o_f = ((const float*)a.orig)[at + i];
    if (a.mask) m = a.mask[mat + i];
    if (RU8) r_b = ((const unsigned char*)a.recon)[at + i]; else r_f = ((const float*)a.recon)[at + i];
}

template <bool U8>
__device__ __forceinline__ bool rp_aligned(const void* base, size_t at) {
    return (((uintptr_t)base + at * (U8 ? 1 : 4)) & 15u) == 0;
}

// 16 consecutive elements from a 16-byte boundary
template <bool U8>
__device__ __forceinline__ void rp_load16(const void* base, size_t at, float* f, unsigned* b) {
    if (U8) {
        const uint4 v = *reinterpret_cast<const uint4*>((const unsigned char*)base + at);
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < RP_SEG; ++k) b[k] = (w[k >> 2] >> (8 * (k & 3))) & 255u;
    } else {
        const float4* q = reinterpret_cast<const float4*>((const float*)base + at);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float4 v = q[k];
            f[4 * k] = v.x, f[4 * k + 1] = v.y, f[4 * k + 2] = v.z, f[4 * k + 3] = v.w;
        }
    }
}

template <bool OU8, bool RU8, bool VEC>
__global__ __launch_bounds__(RP_THREADS) void k_recon_panels(const RpArgs a) {
    // true division: the expression of k_u8_to_unit_float, once per byte value and block (256 threads)
    __shared__ float unit[256];
    if (OU8 || RU8) {
        const unsigned b = threadIdx.y * blockDim.x + threadIdx.x;
        unit[b] = (float)b / 255.f;
        __syncthreads();
    }
    const unsigned row = blockIdx.x * blockDim.y + threadIdx.y;
    if (row >= a.rows) return;
    const unsigned n = row / (unsigned)a.H, y = row - n * (unsigned)a.H;
    const size_t at = (size_t)n * (size_t)a.CHW;
    const size_t mat = a.mask_per_frame ? at : 0;
    const bool show = a.show_orig != 0, masked = a.mask != nullptr;
    unsigned char* o = a.out + (size_t)n * a.out_frame_stride + (size_t)y * (size_t)a.OW;
    for (unsigned seg = threadIdx.x; seg < a.segs; seg += blockDim.x) {
        const unsigned j0 = seg * RP_SEG;
        if (VEC) {
            // (PW is a multiple of 16: the segment is whole, and so are its three copies in the panels)
            unsigned w[3][4] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
            const unsigned c = j0 / (unsigned)a.W, x = j0 - c * (unsigned)a.W;
            const size_t i = (size_t)((c * (unsigned)a.H + y) * (unsigned)a.W + x);
            // inside one channel, every operand on a 16-byte boundary
            const bool vec = x + RP_SEG <= (unsigned)a.W && rp_aligned<OU8>(a.orig, at + i) &&
                             rp_aligned<RU8>(a.recon, at + i) && (!masked || rp_aligned<false>(a.mask, mat + i));
            if (vec) {
                float o_f[RP_SEG], m[RP_SEG], r_f[RP_SEG];
                unsigned o_b[RP_SEG], r_b[RP_SEG];
#pragma unroll
                for (int k = 0; k < RP_SEG; ++k) o_f[k] = 0.f, m[k] = 1.f, r_f[k] = 0.f, o_b[k] = 0u, r_b[k] = 0u;
                rp_load16<OU8>(a.orig, at + i, o_f, o_b);
                rp_load16<RU8>(a.recon, at + i, r_f, r_b);
                if (masked) rp_load16<false>(a.mask, mat + i, m, nullptr);
#pragma unroll
                for (int k = 0; k < RP_SEG; ++k) {
#pragma unroll
                    for (unsigned p = 0; p < 3; ++p)
                        w[p][k >> 2] |= rp_level<OU8, RU8>(p, show, masked, unit, o_f[k], o_b[k], m[k], r_f[k], r_b[k])
                                        << (8 * (k & 3));
                }
            } else {
#pragma unroll
                for (int k = 0; k < RP_SEG; ++k) {
                    float o_f, m, r_f;
                    unsigned o_b, r_b;
                    rp_pixel<OU8, RU8>(a, at, mat, y, j0 + k, o_f, o_b, m, r_f, r_b);
#pragma unroll
                    for (unsigned p = 0; p < 3; ++p)
                        w[p][k >> 2] |= rp_level<OU8, RU8>(p, show, masked, unit, o_f, o_b, m, r_f, r_b) << (8 * (k & 3));
                }
            }
#pragma unroll
            for (unsigned p = 0; p < 3; ++p)
                *reinterpret_cast<uint4*>(o + p * a.PW + j0) = make_uint4(w[p][0], w[p][1], w[p][2], w[p][3]);
        } else {
            const unsigned j1 = j0 + RP_SEG < a.PW ? j0 + RP_SEG : a.PW;
            for (unsigned j = j0; j < j1; ++j) {
                float o_f, m, r_f;
                unsigned o_b, r_b;
                rp_pixel<OU8, RU8>(a, at, mat, y, j, o_f, o_b, m, r_f, r_b);
#pragma unroll
                for (unsigned p = 0; p < 3; ++p)
                    o[p * a.PW + j] = (unsigned char)rp_level<OU8, RU8>(p, show, masked, unit, o_f, o_b, m, r_f, r_b);
            }
        }
    }
}

// threads along a row: the power of two that covers its segments, 256 at the most
static inline unsigned rp_block_x(size_t PW) {
    const size_t segs = (PW + RP_SEG - 1) / RP_SEG;
    unsigned bx = 1;
    while (bx < segs && bx < RP_THREADS) bx <<= 1;
    return bx;
}

bool bn_recon_panels_ok(int N, int C, int H, int W, size_t out_frame_stride) {
    if (N < 0 || C <= 0 || H <= 0 || W <= 0) return false;
    // the launch counts rows, columns and the elements of a frame in 32 bits
    const size_t lim = (size_t)1 << 31;
    const size_t PW = (size_t)C * (size_t)W;
    if ((size_t)N * (size_t)H >= lim || 3 * PW >= lim || PW * (size_t)H >= lim) return false;
    if (out_frame_stride < 3 * PW * (size_t)H) return false;
    // ... and a grid holds fewer than 2^32 threads
    const size_t by = RP_THREADS / rp_block_x(PW);
    if (((size_t)N * (size_t)H + by - 1) / by * RP_THREADS >= ((size_t)1 << 32)) return false;
    // (output offsets stay inside 64 bits)
    return N == 0 || out_frame_stride <= ((size_t)1 << 62) / (size_t)N;
}

int bn_launch_recon_panels(const void* orig, int orig_u8, const void* recon, int recon_u8, const float* mask,
                           int mask_per_frame, int N, int C, int H, int W, int show_orig, unsigned char* out,
                           size_t out_frame_stride, hipStream_t st) {
    if (!bn_recon_panels_ok(N, C, H, W, out_frame_stride)) return BN_E_SHAPE;
    if (N == 0) return 0;
    RpArgs a;
    a.orig = orig, a.recon = recon, a.mask = mask, a.out = out, a.out_frame_stride = out_frame_stride;
    a.H = H, a.W = W, a.show_orig = show_orig, a.mask_per_frame = mask ? mask_per_frame : 0;
    a.rows = (unsigned)N * (unsigned)H, a.PW = (unsigned)C * (unsigned)W, a.OW = 3 * a.PW;
    a.CHW = a.PW * (unsigned)H;
    a.segs = (a.PW + RP_SEG - 1) / RP_SEG;
    const unsigned bx = rp_block_x(a.PW);
    const dim3 block(bx, RP_THREADS / bx);
    const dim3 grid((a.rows + block.y - 1) / block.y);
    // (3 PW on a 16-byte boundary means PW on one: each panel's copy of a segment is aligned then)
    const bool vec = a.PW % RP_SEG == 0 && out_frame_stride % RP_SEG == 0 && (((uintptr_t)out) & 15u) == 0;
#define RP_GO(OU8, RU8)                                                                          \
    do {                                                                                         \
        if (vec) hipLaunchKernelGGL((k_recon_panels<OU8, RU8, true>), grid, block, 0, st, a);    \
        else hipLaunchKernelGGL((k_recon_panels<OU8, RU8, false>), grid, block, 0, st, a);       \
    } while (0)
    if (orig_u8) {
        if (recon_u8) RP_GO(true, true); else RP_GO(true, false);
    } else {
        if (recon_u8) RP_GO(false, true); else RP_GO(false, false);
    }
#undef RP_GO
    BN_LAUNCH_CHECK();
    return 0;
}
