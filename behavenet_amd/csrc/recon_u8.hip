// fp32 unit-float frames -> stored uint8 grey levels ("reconstructions"):
//
//   out[i] = bn_quantise_u8(in[i])          NaN -> 0, else clamp(rint(in[i] * 255), 0, 255)
//
// A thread owns RU_PER_THREAD = 16 consecutive values: four 16-byte loads and one 16-byte store where both operands
// sit on a 16-byte boundary, element by element otherwise and in the group that straddles n.  The loads and the
// store differ, the arithmetic does not.  The grid is sized to the data.
#include "bn_common.h"
#include "bn_launch.h"

#define RU_THREADS 256
#define RU_PER_THREAD 16

template <bool VEC>
__global__ __launch_bounds__(RU_THREADS) void k_unit_float_to_u8(const float* __restrict__ in,
                                                                 unsigned char* __restrict__ out, size_t n) {
    const size_t i0 = ((size_t)blockIdx.x * RU_THREADS + threadIdx.x) * RU_PER_THREAD;
    if (i0 >= n) return;
    if (VEC && i0 + RU_PER_THREAD <= n) {
        unsigned w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 a = *reinterpret_cast<const float4*>(in + i0 + 4 * q);
            w[q] = bn_quantise_u8(a.x) | (bn_quantise_u8(a.y) << 8) | (bn_quantise_u8(a.z) << 16) |
                   (bn_quantise_u8(a.w) << 24);
        }
        *reinterpret_cast<uint4*>(out + i0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        const size_t i1 = i0 + RU_PER_THREAD < n ? i0 + RU_PER_THREAD : n;
        for (size_t i = i0; i < i1; ++i) out[i] = (unsigned char)bn_quantise_u8(in[i]);
    }
}

bool bn_unit_float_to_u8_ok(size_t n) {
    return (n + RU_PER_THREAD * RU_THREADS - 1) / (RU_PER_THREAD * RU_THREADS) < ((size_t)1 << 31);
}

int bn_launch_unit_float_to_u8(const float* in, unsigned char* out, size_t n, hipStream_t st) {
    if (!bn_unit_float_to_u8_ok(n)) return BN_E_SHAPE;
    const dim3 grid((unsigned)((n + RU_PER_THREAD * RU_THREADS - 1) / (RU_PER_THREAD * RU_THREADS)));
    if (((((uintptr_t)in) | ((uintptr_t)out)) & 15u) == 0)
        hipLaunchKernelGGL((k_unit_float_to_u8<true>), grid, dim3(RU_THREADS), 0, st, in, out, n);
    else
        hipLaunchKernelGGL((k_unit_float_to_u8<false>), grid, dim3(RU_THREADS), 0, st, in, out, n);
    BN_LAUNCH_CHECK();
    return 0;
}
