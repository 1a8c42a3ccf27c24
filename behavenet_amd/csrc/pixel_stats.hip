// Per-pixel error and moment sums over the frames of a trial ("pixel stats"):
//
//   acc[0][i] += sum_n ((xhat[n, i] - t[n, i]) * (xhat[n, i] - t[n, i])) * m[n, i]     (not touched without xhat)
//   acc[1][i] += sum_n m[n, i]
//   acc[2][i] += sum_n m[n, i] * t[n, i]
//   acc[3][i] += sum_n m[n, i] * (t[n, i] * t[n, i])                                  i < D = C H W
//
// t = target: fp32, or stored uint8 frames (value / 255, the division of k_u8_to_unit_float); m = mask (one per
// frame or one for all frames) or 1.  Plane 0's term is fe_term of frame_err.hip in fp32, widened; the moments are
// products of the widened fp32 t and m.  Every sum is float64.
//
// The order of every pixel's sum is a function of (N, D) alone -- no atomics:
//   * a thread owns PS_PER_THREAD consecutive pixels, a workgroup a tile of PS_TILE pixels and one block of
//     consecutive frames, which it walks in ascending order, each pixel's four sums in registers;
//   * with one frame block the sums are added onto acc as they are; with B > 1 they go to the (B, 4, D) workspace and
//     k_pixel_stats_finish adds a pixel's B partials from left to right, then that sum onto acc.
// Aligned operands are read with 16-byte loads (4 bytes of a uint8 target), anything else element by element: the
// loads differ, the arithmetic does not.
#include "bn_common.h"
#include "bn_launch.h"

// (a product folded into the addition that follows it would round once where the other path rounds twice)
#pragma clang fp contract(off)

#define PS_THREADS 256
#define PS_PER_THREAD 4
#define PS_TILE (PS_THREADS * PS_PER_THREAD)
#define PS_MIN_FRAMES 16       // frames a workgroup walks at least (but for the trial's tail)
#define PS_TARGET_GROUPS 512   // workgroups the frame blocks are cut for: two a CU

// the same expression as fe_term of frame_err.hip
__device__ __forceinline__ float ps_term(float p, float t, float m) {
    const float d = p - t;
    return d * d * m;
}

struct PsPlan {
    size_t tiles;      // pixel tiles of PS_TILE
    int blocks;        // frame blocks B
    int frames;        // frames per block (the last block takes what is left)
};

// the ONE partition the workspace query, the launch and the finish go by: a function of (N, D) alone
static PsPlan ps_plan(int N, size_t D) {
    PsPlan p;
    p.tiles = (D + PS_TILE - 1) / PS_TILE;
    const size_t for_chip = (PS_TARGET_GROUPS + p.tiles - 1) / p.tiles;
    const size_t by_frames = ((size_t)N + PS_MIN_FRAMES - 1) / PS_MIN_FRAMES;
    const size_t want = for_chip < by_frames ? for_chip : by_frames;
    p.frames = (int)(((size_t)N + want - 1) / want);
    p.blocks = (N + p.frames - 1) / p.frames;
    return p;
}

template <bool U8, bool VEC>
__global__ __launch_bounds__(PS_THREADS) void k_pixel_stats(const float* __restrict__ xhat,
                                                            const void* __restrict__ target,
                                                            const float* __restrict__ mask, int mask_per_frame,
                                                            double* __restrict__ dst, int add_onto, int N, size_t D,
                                                            unsigned tiles, int frames) {
    const unsigned b = blockIdx.x / tiles;
    const unsigned tile = blockIdx.x - b * tiles;
    const size_t i0 = (size_t)tile * PS_TILE + (size_t)threadIdx.x * PS_PER_THREAD;
    if (i0 >= D) return;
    const int n0 = (int)b * frames;
    const int n1 = n0 + frames < N ? n0 + frames : N;
    const float* tf = (const float*)target;
    const unsigned char* tu = (const unsigned char*)target;

    double sse[PS_PER_THREAD], w[PS_PER_THREAD], s1[PS_PER_THREAD], s2[PS_PER_THREAD];
    float mv[PS_PER_THREAD];
#pragma unroll
    for (int k = 0; k < PS_PER_THREAD; ++k) {
        sse[k] = w[k] = s1[k] = s2[k] = 0.0;
        mv[k] = 1.f;
    }
    // one mask for all frames: read once
    if (mask && !mask_per_frame) {
        if (VEC) {
            const float4 a = *reinterpret_cast<const float4*>(mask + i0);
            mv[0] = a.x; mv[1] = a.y; mv[2] = a.z; mv[3] = a.w;
        } else {
#pragma unroll
            for (int k = 0; k < PS_PER_THREAD; ++k)
                if (i0 + k < D) mv[k] = mask[i0 + k];
        }
    }
#pragma unroll 4
    for (int n = n0; n < n1; ++n) {
        const size_t at = (size_t)n * D + i0;
        float pv[PS_PER_THREAD] = {0.f, 0.f, 0.f, 0.f}, tv[PS_PER_THREAD];
        if (VEC) {
            if (U8) {
                const unsigned u = *reinterpret_cast<const unsigned*>(tu + at);
#pragma unroll
                for (int k = 0; k < PS_PER_THREAD; ++k) tv[k] = (float)((u >> (8 * k)) & 0xffu) / 255.f;   // true division
            } else {
                const float4 a = *reinterpret_cast<const float4*>(tf + at);
                tv[0] = a.x; tv[1] = a.y; tv[2] = a.z; tv[3] = a.w;
            }
            if (xhat) {
                const float4 a = *reinterpret_cast<const float4*>(xhat + at);
                pv[0] = a.x; pv[1] = a.y; pv[2] = a.z; pv[3] = a.w;
            }
            if (mask && mask_per_frame) {
                const float4 a = *reinterpret_cast<const float4*>(mask + at);
                mv[0] = a.x; mv[1] = a.y; mv[2] = a.z; mv[3] = a.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < PS_PER_THREAD; ++k) {
                // (pixels past D: any finite values, their sums are not stored)
                tv[k] = 0.f;
                pv[k] = 0.f;
                if (i0 + k < D) {
                    tv[k] = U8 ? (float)tu[at + k] / 255.f : tf[at + k];
                    if (xhat) pv[k] = xhat[at + k];
                    if (mask && mask_per_frame) mv[k] = mask[at + k];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < PS_PER_THREAD; ++k) {
            const double td = (double)tv[k], md = (double)mv[k];
            if (xhat) sse[k] += (double)ps_term(pv[k], tv[k], mv[k]);
            w[k] += md;
            s1[k] += md * td;
            s2[k] += md * (td * td);
        }
    }

    // plane p of this frame block: dst + (b * 4 + p) * D with the workspace, acc + p * D (b == 0) without
    double* base = dst + (size_t)b * 4 * D + i0;
    double* const planes[4] = {base, base + D, base + 2 * D, base + 3 * D};
    const double* const sums[4] = {sse, w, s1, s2};
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        if (p == 0 && !xhat) continue;
        if (VEC) {
            double2* q = reinterpret_cast<double2*>(planes[p]);
            double2 lo = make_double2(sums[p][0], sums[p][1]), hi = make_double2(sums[p][2], sums[p][3]);
            if (add_onto) {
                const double2 a = q[0], c = q[1];
                lo.x = a.x + lo.x; lo.y = a.y + lo.y; hi.x = c.x + hi.x; hi.y = c.y + hi.y;
            }
            q[0] = lo;
            q[1] = hi;
        } else {
#pragma unroll
            for (int k = 0; k < PS_PER_THREAD; ++k)
                if (i0 + k < D) planes[p][k] = add_onto ? planes[p][k] + sums[p][k] : sums[p][k];
        }
    }
}

// acc[e] += part[0][e] + part[1][e] + ... (left to right), e over the planes [p0, 4) of D pixels each
__global__ __launch_bounds__(PS_THREADS) void k_pixel_stats_finish(const double* __restrict__ part,
                                                                   double* __restrict__ acc, size_t e0, size_t e1,
                                                                   size_t plane_elems, int B) {
    const size_t e = e0 + (size_t)blockIdx.x * PS_THREADS + threadIdx.x;
    if (e >= e1) return;
    double s = part[e];
    for (int j = 1; j < B; ++j) s += part[(size_t)j * plane_elems + e];
    acc[e] = acc[e] + s;
}

bool bn_pixel_stats_ok(int N, size_t D) {
    if (N <= 0 || D == 0 || D > ((size_t)1 << 40)) return false;
    const PsPlan p = ps_plan(N, D);
    // (the grids' x extents; the finish kernel walks 4 D elements, 256 a workgroup)
    return p.tiles * (size_t)p.blocks < ((size_t)1 << 31) && (4 * D + PS_THREADS - 1) / PS_THREADS < ((size_t)1 << 31);
}

size_t bn_pixel_stats_ws_bytes_impl(int N, size_t D) {
    if (!bn_pixel_stats_ok(N, D)) return 0;
    const PsPlan p = ps_plan(N, D);
    return p.blocks == 1 ? 0 : (size_t)p.blocks * 4 * D * sizeof(double);
}

static inline bool ps_aligned(const void* p, unsigned to) { return (((uintptr_t)p) & (to - 1)) == 0; }

int bn_launch_pixel_stats(const float* xhat, const void* target, int target_is_u8, const float* mask, int mask_frames,
                          double* acc, int N, size_t D, void* ws, hipStream_t st) {
    if (!bn_pixel_stats_ok(N, D)) return BN_E_SHAPE;
    const PsPlan p = ps_plan(N, D);
    // every frame of every operand starts on a 16-byte boundary (4 bytes: the uint8 target), and so does every plane
    // of acc and of the workspace, or the element-by-element loads serve the call
    const bool vec = D % 4 == 0 && (!xhat || ps_aligned(xhat, 16)) && ps_aligned(target, target_is_u8 ? 4 : 16) &&
                     (!mask || ps_aligned(mask, 16));
    const int per_frame = mask && mask_frames != 1;
    double* dst = p.blocks == 1 ? acc : (double*)ws;
    const int add_onto = p.blocks == 1;
    const dim3 grid((unsigned)(p.tiles * (size_t)p.blocks));
#define PS_GO(U8, VEC)                                                                                             \
    hipLaunchKernelGGL((k_pixel_stats<U8, VEC>), grid, dim3(PS_THREADS), 0, st, xhat, target, mask, per_frame, dst, \
                       add_onto, N, D, (unsigned)p.tiles, p.frames)
    if (target_is_u8) {
        if (vec) PS_GO(true, true); else PS_GO(true, false);
    } else {
        if (vec) PS_GO(false, true); else PS_GO(false, false);
    }
#undef PS_GO
    BN_LAUNCH_CHECK();
    if (p.blocks > 1) {
        const size_t e0 = xhat ? 0 : D, e1 = 4 * D;
        hipLaunchKernelGGL(k_pixel_stats_finish, dim3((unsigned)((e1 - e0 + PS_THREADS - 1) / PS_THREADS)),
                           dim3(PS_THREADS), 0, st, (const double*)ws, acc, e0, e1, 4 * D, p.blocks);
        BN_LAUNCH_CHECK();
    }
    return 0;
}
