// Per-frame squared reconstruction error ("frame errors"):
//
//   out[n] = scale * sum_i (xhat[n, i] - target[n, i])^2 * mask[n, i]        i < D = C H W
//
// target fp32, or stored uint8 frames (value / 255, the division of k_u8_to_unit_float); mask optional.
//
// The summation order of a frame is a function of D alone -- not of the frame's position in the batch, of the batch
// size or of the operands' alignment -- so a frame scored alone gives the bits it gives inside a trial:
//   * a workgroup owns FE_BLOCK consecutive elements of ONE frame, a thread 16 consecutive ones of them, summed as the
//     fixed tree ((e0 + e1) + (e2 + e3)) + ... ; elements past D count as +0 in the same tree;
//   * the 256 thread sums go through the wave shuffle tree and a fixed LDS combine;
//   * a frame of more than FE_BLOCK elements leaves P = ceil(D / FE_BLOCK) partials in the (N, P) workspace, which
//     k_frame_err_finish adds from left to right.  No atomics.
// Aligned operands are read with 16-byte loads, anything else (and the group that straddles D) element by element:
// the loads differ, the arithmetic does not.
#include "bn_common.h"
#include "bn_launch.h"

// (a product folded into the addition that follows it would round once where the other path rounds twice)
#pragma clang fp contract(off)

#define FE_THREADS 256
#define FE_PER_THREAD 16
#define FE_BLOCK (FE_THREADS * FE_PER_THREAD)

__device__ __forceinline__ float fe_term(float p, float t, float m) {
    const float d = p - t;
    return d * d * m;
}

// 256 thread values -> one, the same order on every call; valid on thread 0
__device__ __forceinline__ float fe_block_sum(float acc, float* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

template <bool U8, bool VEC>
__global__ __launch_bounds__(FE_THREADS) void k_frame_sq_err(const float* __restrict__ xhat,
                                                             const void* __restrict__ target,
                                                             const float* __restrict__ mask, float* __restrict__ dst,
                                                             size_t D, unsigned P, float scale) {
    __shared__ float red[FE_THREADS / BN_WAVE];
    const size_t n = blockIdx.x / P;
    const unsigned b = blockIdx.x - (unsigned)n * P;
    const size_t i0 = (size_t)b * FE_BLOCK + (size_t)threadIdx.x * FE_PER_THREAD;
    const float* p = xhat + n * D;
    const float* tf = (const float*)target + n * D;
    const unsigned char* tu = (const unsigned char*)target + n * D;
    const float* m = mask ? mask + n * D : nullptr;
    float e[FE_PER_THREAD];
    if (VEC && i0 + FE_PER_THREAD <= D) {
        float pv[FE_PER_THREAD], tv[FE_PER_THREAD], mv[FE_PER_THREAD];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 a = *reinterpret_cast<const float4*>(p + i0 + 4 * q);
            pv[4 * q] = a.x; pv[4 * q + 1] = a.y; pv[4 * q + 2] = a.z; pv[4 * q + 3] = a.w;
        }
        if (U8) {
            const uint4 u = *reinterpret_cast<const uint4*>(tu + i0);
            const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
            for (int k = 0; k < FE_PER_THREAD; ++k)
                tv[k] = (float)((w[k >> 2] >> (8 * (k & 3))) & 0xffu) / 255.f;          // true division
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 a = *reinterpret_cast<const float4*>(tf + i0 + 4 * q);
                tv[4 * q] = a.x; tv[4 * q + 1] = a.y; tv[4 * q + 2] = a.z; tv[4 * q + 3] = a.w;
            }
        }
        if (m) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 a = *reinterpret_cast<const float4*>(m + i0 + 4 * q);
                mv[4 * q] = a.x; mv[4 * q + 1] = a.y; mv[4 * q + 2] = a.z; mv[4 * q + 3] = a.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < FE_PER_THREAD; ++k) mv[k] = 1.f;
        }
#pragma unroll
        for (int k = 0; k < FE_PER_THREAD; ++k) e[k] = fe_term(pv[k], tv[k], mv[k]);
    } else {
#pragma unroll
        for (int k = 0; k < FE_PER_THREAD; ++k) {
            const size_t i = i0 + k;
            e[k] = 0.f;
            if (i < D) e[k] = fe_term(p[i], U8 ? (float)tu[i] / 255.f : tf[i], m ? m[i] : 1.f);
        }
    }
    float q4[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) q4[q] = (e[4 * q] + e[4 * q + 1]) + (e[4 * q + 2] + e[4 * q + 3]);
    const float s = fe_block_sum((q4[0] + q4[1]) + (q4[2] + q4[3]), red);
    if (threadIdx.x == 0) dst[blockIdx.x] = P == 1 ? s * scale : s;
}

// out[n] = scale * (part[n][0] + part[n][1] + ...), left to right
__global__ __launch_bounds__(FE_THREADS) void k_frame_err_finish(const float* __restrict__ part,
                                                                 float* __restrict__ out, int N, unsigned P,
                                                                 float scale) {
    const int n = blockIdx.x * FE_THREADS + threadIdx.x;
    if (n >= N) return;
    float acc = 0.f;
    for (unsigned j = 0; j < P; ++j) acc += part[(size_t)n * P + j];
    out[n] = acc * scale;
}

int bn_launch_frame_err_finish(const float* part, float* out, int N, unsigned P, float scale, hipStream_t st) {
    hipLaunchKernelGGL(k_frame_err_finish, dim3((unsigned)((N + FE_THREADS - 1) / FE_THREADS)), dim3(FE_THREADS), 0, st,
                       part, out, N, P, scale);
    BN_LAUNCH_CHECK();
    return 0;
}

// partials per frame: the ONE number the workspace query and the launch both go by
static size_t fe_parts(size_t D) { return (D + FE_BLOCK - 1) / FE_BLOCK; }

bool bn_frame_sq_err_ok(int N, size_t D) {
    return N > 0 && D > 0 && fe_parts(D) * (size_t)N < ((size_t)1 << 31);
}

size_t bn_frame_sq_err_ws_bytes_impl(int N, size_t D) {
    if (!bn_frame_sq_err_ok(N, D)) return 0;
    const size_t P = fe_parts(D);
    return P == 1 ? 0 : (size_t)N * P * sizeof(float);
}

static inline bool fe_aligned16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }

int bn_launch_frame_sq_err(const float* xhat, const void* target, int target_is_u8, const float* mask, float* out,
                           int N, size_t D, float scale, void* ws, hipStream_t st) {
    if (!bn_frame_sq_err_ok(N, D)) return BN_E_SHAPE;
    const unsigned P = (unsigned)fe_parts(D);
    // every frame starts on a 16-byte boundary of every operand, or the element-by-element loads serve the call
    const bool vec = fe_aligned16(xhat) && fe_aligned16(target) && (!mask || fe_aligned16(mask)) &&
                     D % (target_is_u8 ? 16 : 4) == 0;
    float* dst = P == 1 ? out : (float*)ws;
    const dim3 grid((unsigned)((size_t)N * P));
#define FE_GO(U8, VEC)                                                                                            \
    hipLaunchKernelGGL((k_frame_sq_err<U8, VEC>), grid, dim3(FE_THREADS), 0, st, xhat, target, mask, dst, D, P, scale)
    if (target_is_u8) {
        if (vec) FE_GO(true, true); else FE_GO(true, false);
    } else {
        if (vec) FE_GO(false, true); else FE_GO(false, false);
    }
#undef FE_GO
    BN_LAUNCH_CHECK();
    if (P > 1) return bn_launch_frame_err_finish(dst, out, N, P, scale, st);
    return 0;
}
