// The input of a conditional encoder in one pass ("label maps"):
//
//   out[n, c]     = frames[n, c]                        c < C: fp32 frames copied, stored uint8 frames as value / 255
//   out[n, C + l] = one-hot map of label l of frame n   l < L: zeros but for one 1.0f at (y, x)
//
// with x from column l and y from column L + l of the frame's row of coordinates, each through the rule of
// data.transforms.MakeOneHot2D._pixel: NaN counts as 0, clip to [0, size - 1], round half to even.  out is what
// torch.cat((frames as fp32, MakeOneHot2D(H, W)(coords)), 1) holds, bit for bit.
//
// HBM-bound: (C + L) H W 4 bytes written and C H W (four times that for fp32 frames) read per frame.  A workgroup
// owns a segment of one (frame, channel) plane; it reads the plane's two coordinates from device memory (no host
// read, nothing to synchronise: the call is capturable), and the thread that owns the hot pixel's group of four puts
// the 1.0f into the 16-byte store that writes the group -- one pass, every output byte written once, no atomics.
// Plain stores: the first conv layer reads the tensor next.
#include "bn_common.h"
#include "bn_launch.h"

#define CI_THREADS 256
#define CI_PER_THREAD 4
#define CI_SEG (CI_THREADS * CI_PER_THREAD)   // units of a segment: 16-byte groups (vector path) or elements
#define CI_MAX_BLOCKS 65536                   // more segments than this are walked by the grid-stride loop

// MakeOneHot2D._pixel in its own arithmetic, float64 (for sizes below 2^24 this is rintf of the fp32 clip, bit for bit)
__device__ __forceinline__ size_t ci_pixel(float v, int size) {
    double d = (double)v;
    if (d != d) d = 0.0;
    d = fmin(fmax(d, 0.0), (double)(size - 1));
    return (size_t)rint(d);          // round half to even
}

template <bool U8, bool VEC>
__global__ __launch_bounds__(CI_THREADS) void k_cond_input(const void* __restrict__ frames,
                                                           const float* __restrict__ coords, size_t ld,
                                                           float* __restrict__ out, size_t planes, int C, int L, int H,
                                                           int W, size_t units, size_t segs) {
    const size_t HW = (size_t)H * (size_t)W;
    const size_t CL = (size_t)C + (size_t)L;
    const size_t items = planes * segs;
    for (size_t item = blockIdx.x; item < items; item += gridDim.x) {
        const size_t plane = item / segs, seg = item - plane * segs;
        const size_t n = plane / CL, ch = plane - n * CL;
        float* o = out + plane * HW;
        const size_t u0 = seg * CI_SEG + threadIdx.x;
        if (ch < (size_t)C) {
            const size_t src = (n * (size_t)C + ch) * HW;
            if (VEC) {
                float4 v[CI_PER_THREAD];
#pragma unroll
                for (int k = 0; k < CI_PER_THREAD; ++k) {
                    const size_t u = u0 + (size_t)k * CI_THREADS;
                    if (u >= units) continue;
                    if (U8) {
                        const uchar4 b = reinterpret_cast<const uchar4*>((const unsigned char*)frames + src)[u];
                        // true division: the expression of k_u8_to_unit_float
                        v[k] = make_float4(b.x / 255.f, b.y / 255.f, b.z / 255.f, b.w / 255.f);
                    } else {
                        v[k] = reinterpret_cast<const float4*>((const float*)frames + src)[u];
                    }
                }
#pragma unroll
                for (int k = 0; k < CI_PER_THREAD; ++k) {
                    const size_t u = u0 + (size_t)k * CI_THREADS;
                    if (u < units) reinterpret_cast<float4*>(o)[u] = v[k];
                }
            } else {
#pragma unroll
                for (int k = 0; k < CI_PER_THREAD; ++k) {
                    const size_t u = u0 + (size_t)k * CI_THREADS;
                    if (u >= units) continue;
                    o[u] = U8 ? ((const unsigned char*)frames)[src + u] / 255.f : ((const float*)frames)[src + u];
                }
            }
        } else {
            const size_t l = ch - (size_t)C;
            const float* row = coords + n * ld;
            const size_t hot = ci_pixel(row[(size_t)L + l], H) * (size_t)W + ci_pixel(row[l], W);
#pragma unroll
            for (int k = 0; k < CI_PER_THREAD; ++k) {
                const size_t u = u0 + (size_t)k * CI_THREADS;
                if (u >= units) continue;
                if (VEC) {
                    // the component of this group that is the hot pixel (4: none)
                    const unsigned at = u == (hot >> 2) ? (unsigned)(hot & 3) : 4u;
                    reinterpret_cast<float4*>(o)[u] = make_float4(at == 0 ? 1.f : 0.f, at == 1 ? 1.f : 0.f,
                                                                  at == 2 ? 1.f : 0.f, at == 3 ? 1.f : 0.f);
                } else {
                    o[u] = u == hot ? 1.f : 0.f;
                }
            }
        }
    }
}

bool bn_cond_input_ok(int N, int C, int H, int W, int L) {
    if (N < 0 || C <= 0 || H <= 0 || W <= 0 || L < 0) return false;
    // (the output's element count, and with it every index of the kernel, stays far inside 64 bits)
    const size_t HW = (size_t)H * (size_t)W, CL = (size_t)C + (size_t)L, lim = (size_t)1 << 40;
    return CL <= lim / HW && (size_t)N <= lim / (CL * HW);
}

static inline bool ci_aligned(const void* p, unsigned to) { return (((uintptr_t)p) & (to - 1)) == 0; }

int bn_launch_cond_input(const void* frames, int frames_is_u8, const float* coords, int ld, int N, int C, int H, int W,
                         int L, float* out, hipStream_t st) {
    if (!bn_cond_input_ok(N, C, H, W, L)) return BN_E_SHAPE;
    const size_t HW = (size_t)H * (size_t)W;
    const size_t planes = (size_t)N * ((size_t)C + (size_t)L);
    // every plane of the output starts on a 16-byte boundary and every plane of the frames on a 16-byte one (4 bytes:
    // uint8 frames), or the element-by-element path serves the call -- decided per launch
    const bool vec = HW % 4 == 0 && ci_aligned(out, 16) && ci_aligned(frames, frames_is_u8 ? 4 : 16);
    const size_t units = vec ? HW / 4 : HW;
    const size_t segs = (units + CI_SEG - 1) / CI_SEG;
    const size_t items = planes * segs;
    if (items == 0) return 0;
    const dim3 grid((unsigned)(items < CI_MAX_BLOCKS ? items : CI_MAX_BLOCKS));
#define CI_GO(U8, VEC)                                                                                         \
    hipLaunchKernelGGL((k_cond_input<U8, VEC>), grid, dim3(CI_THREADS), 0, st, frames, coords, (size_t)ld, out, \
                       planes, C, L, H, W, units, segs)
    if (frames_is_u8) {
        if (vec) CI_GO(true, true); else CI_GO(true, false);
    } else {
        if (vec) CI_GO(false, true); else CI_GO(false, false);
    }
#undef CI_GO
    BN_LAUNCH_CHECK();
    return 0;
}
