// Frames -> a uint8 mosaic of cropped panels in one pass ("traversals"):
//
//   out[t, r Hc + y, (c n_ch + q) Wc + x] = 0                                         blank panel or outside the frame
//                              = bn_quantise_u8(frames[s, ch0 + q, y_min + y, x_min + x])   fp32 frames (unit floats)
//                              = frames[s, ch0 + q, y_min + y, x_min + x]                   uint8 frames (grey levels)
//
// with s = src[t, r, c]; a panel is blank for s < 0 (and for s >= P, which the Python wrapper refuses before any
// call), a pixel is outside for y_min + y >= H or x_min + x >= W -- the zero fill of the reference's get_crop.  A
// panel is n_ch sub-panels of Wc columns, the channels ch0 .. ch0 + n_ch - 1 of ONE frame side by side (the
// reference's concat(ims[i])): one index read per panel, whatever n_ch is.  bn_frame_mosaic_u8 is n_ch = 1, where a
// sub-panel is the panel.  Channels are picked, cropped, quantised and tiled; every output byte is written once, no
// memset is relied on.
//
// HBM-bound: Hc Wc (4 or 1) bytes read per sub-panel shown, Hc Wc written.  A thread owns 16 consecutive bytes of one
// output row.  With `out` and the row length Cc n_ch Wc on 16-byte boundaries it writes them with one 16-byte store;
// where the 16 bytes lie inside one sub-panel, inside the frame and their source sits on a 16-byte boundary they come
// from four 16-byte loads (uint8 frames: one), otherwise -- a segment that straddles two sub-panels, the frame's
// edge, a window or a pointer off alignment -- byte by byte.  Without that alignment of the output the bytes are
// stored one by one.  mo_byte is the only arithmetic, so every route gives the same bytes.
//
// The block is (bx, 256 / bx): bx threads walk the 16-byte segments of a row, 256 / bx rows share a block, and
// blockIdx.x counts row groups -- a movie has far more than 65,535 rows, which grid.y could not hold.  No 64-bit
// division: a row's (t, r, y) come from 32-bit ones.
#include "bn_common.h"
#include "bn_launch.h"

#define MO_THREADS 256
#define MO_SEG 16          // output bytes a thread owns

struct MoArgs {
    const void* frames;
    const int* src;
    unsigned char* out;
    int P, C, H, W, ch0, n_ch, y_min, x_min, Hc, Wc, R, Cc;
    unsigned rows, OH, OW, segs;          // rows = T R Hc, OH = R Hc, OW = Cc n_ch Wc, segs = ceil(OW / 16)
};

// the frame plane of sub-panel u = c n_ch + q of panel row (t, r) -- channel ch0 + q of frame src[t, r, c] -- or
// nullptr for a blank one (u < Cc n_ch, so c < Cc and ch0 + q < C).  ONE: n_ch == 1, where u is the panel and the
// division is not paid (measured: 18.8 against 17.1 us on the uint8 route of the traversal movie with it)
template <bool U8, bool ONE>
__device__ __forceinline__ const void* mo_plane(const MoArgs& a, size_t panel_row, unsigned u) {
    const unsigned c = ONE ? u : u / (unsigned)a.n_ch, q = ONE ? 0u : u - c * (unsigned)a.n_ch;
    const int s = a.src[panel_row * (size_t)a.Cc + c];
    if (s < 0 || s >= a.P) return nullptr;
    const size_t at = ((size_t)s * (size_t)a.C + (size_t)a.ch0 + q) * (size_t)a.H * (size_t)a.W;
    return U8 ? (const void*)((const unsigned char*)a.frames + at) : (const void*)((const float*)a.frames + at);
}

// one output byte: column ox of the output row whose source row is ys (ys < H checked by the caller)
template <bool U8, bool ONE>
__device__ __forceinline__ unsigned mo_byte(const MoArgs& a, size_t panel_row, size_t row_at, unsigned ox) {
    const unsigned u = ox / (unsigned)a.Wc;
    const unsigned xs = (unsigned)a.x_min + (ox - u * (unsigned)a.Wc);
    if (xs >= (unsigned)a.W) return 0u;
    const void* p = mo_plane<U8, ONE>(a, panel_row, u);
    if (!p) return 0u;
    return U8 ? (unsigned)((const unsigned char*)p)[row_at + xs] : bn_quantise_u8(((const float*)p)[row_at + xs]);
}

template <bool U8, bool VEC, bool ONE>
__global__ __launch_bounds__(MO_THREADS) void k_frame_mosaic(const MoArgs a) {
    const unsigned row = blockIdx.x * blockDim.y + threadIdx.y;
    if (row >= a.rows) return;
    const unsigned t = row / a.OH, oy = row - t * a.OH;
    const unsigned r = oy / (unsigned)a.Hc, y = oy - r * (unsigned)a.Hc;
    const unsigned ys = (unsigned)a.y_min + y;
    const size_t panel_row = (size_t)t * (size_t)a.R + r;
    const size_t row_at = (size_t)ys * (size_t)a.W;
    unsigned char* o = a.out + (size_t)row * (size_t)a.OW;
    for (unsigned seg = threadIdx.x; seg < a.segs; seg += blockDim.x) {
        const unsigned x0 = seg * MO_SEG;
        if (VEC) {
            // (OW is a multiple of 16: the segment is whole)
            unsigned w[4] = {0u, 0u, 0u, 0u};
            if (ys < (unsigned)a.H) {
                const unsigned u = x0 / (unsigned)a.Wc, x = x0 - u * (unsigned)a.Wc;
                const unsigned xs = (unsigned)a.x_min + x;
                bool done = false;
                if (x + MO_SEG <= (unsigned)a.Wc && xs + MO_SEG <= (unsigned)a.W) {
                    const void* p = mo_plane<U8, ONE>(a, panel_row, u);
                    if (!p) {
                        done = true;          // a blank panel: zeros
                    } else if (U8) {
                        const unsigned char* q = (const unsigned char*)p + row_at + xs;
                        if ((((uintptr_t)q) & 15u) == 0) {
                            const uint4 v = *reinterpret_cast<const uint4*>(q);
                            w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
                            done = true;
                        }
                    } else {
                        const float* q = (const float*)p + row_at + xs;
                        if ((((uintptr_t)q) & 15u) == 0) {
                            float4 v[4];
#pragma unroll
                            for (int k = 0; k < 4; ++k) v[k] = reinterpret_cast<const float4*>(q)[k];
#pragma unroll
                            for (int k = 0; k < 4; ++k)
                                w[k] = bn_quantise_u8(v[k].x) | (bn_quantise_u8(v[k].y) << 8) |
                                       (bn_quantise_u8(v[k].z) << 16) | (bn_quantise_u8(v[k].w) << 24);
                            done = true;
                        }
                    }
                }
                if (!done) {
#pragma unroll
                    for (int k = 0; k < MO_SEG; ++k)
                        w[k >> 2] |= mo_byte<U8, ONE>(a, panel_row, row_at, x0 + k) << (8 * (k & 3));
                }
            }
            *reinterpret_cast<uint4*>(o + x0) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
            const unsigned x1 = x0 + MO_SEG < a.OW ? x0 + MO_SEG : a.OW;
            for (unsigned ox = x0; ox < x1; ++ox)
                o[ox] = (unsigned char)(ys < (unsigned)a.H ? mo_byte<U8, ONE>(a, panel_row, row_at, ox) : 0u);
        }
    }
}

// threads along a row: the power of two that covers its segments, 256 at the most
static inline unsigned mo_block_x(size_t OW) {
    const size_t segs = (OW + MO_SEG - 1) / MO_SEG;
    unsigned bx = 1;
    while (bx < segs && bx < MO_THREADS) bx <<= 1;
    return bx;
}

bool bn_frame_mosaic_ok(int P, int C, int H, int W, int ch0, int n_ch, int y_min, int x_min, int Hc, int Wc, int T,
                        int R, int Cc) {
    if (P < 0 || C <= 0 || H <= 0 || W <= 0 || T < 0 || R < 0 || Cc < 0) return false;
    if (n_ch < 1 || ch0 < 0 || (long long)ch0 + (long long)n_ch > (long long)C) return false;
    if (y_min < 0 || x_min < 0 || Hc <= 0 || Wc <= 0) return false;
    // the launch counts output rows and columns in 32 bits (and y_min + y, x_min + x with them)
    const size_t lim = (size_t)1 << 31;
    const size_t TR = (size_t)T * (size_t)R;
    if (TR >= lim || TR * (size_t)Hc >= lim || (size_t)Cc * (size_t)Wc >= lim) return false;
    const size_t OW = (size_t)Cc * (size_t)Wc * (size_t)n_ch;          // (n_ch <= C < 2^31: below 2^62)
    if (OW >= lim) return false;
    if ((size_t)y_min + (size_t)Hc >= lim || (size_t)x_min + (size_t)Wc >= lim) return false;
    // ... and a grid holds fewer than 2^32 threads
    const size_t by = MO_THREADS / mo_block_x(OW);
    if ((TR * (size_t)Hc + by - 1) / by * MO_THREADS >= ((size_t)1 << 32)) return false;
    // (frame and output offsets stay far inside 64 bits)
    const size_t HW = (size_t)H * (size_t)W, big = (size_t)1 << 44;
    return (size_t)C <= big / HW && (size_t)P <= big / ((size_t)C * HW);
}

int bn_launch_frame_mosaic(const void* frames, int frames_u8, int P, int C, int H, int W, int ch0, int n_ch, int y_min,
                           int x_min, int Hc, int Wc, const int* src, int T, int R, int Cc, unsigned char* out,
                           hipStream_t st) {
    if (!bn_frame_mosaic_ok(P, C, H, W, ch0, n_ch, y_min, x_min, Hc, Wc, T, R, Cc)) return BN_E_SHAPE;
    MoArgs a;
    a.frames = frames, a.src = src, a.out = out;
    a.P = P, a.C = C, a.H = H, a.W = W, a.ch0 = ch0, a.n_ch = n_ch, a.y_min = y_min, a.x_min = x_min;
    a.Hc = Hc, a.Wc = Wc, a.R = R, a.Cc = Cc;
    a.OH = (unsigned)R * (unsigned)Hc, a.OW = (unsigned)Cc * (unsigned)n_ch * (unsigned)Wc;
    a.rows = (unsigned)T * a.OH;
    a.segs = (a.OW + MO_SEG - 1) / MO_SEG;
    if (a.rows == 0 || a.OW == 0) return 0;
    const unsigned bx = mo_block_x(a.OW);
    const dim3 block(bx, MO_THREADS / bx);
    const dim3 grid((a.rows + block.y - 1) / block.y);
    const bool vec = a.OW % MO_SEG == 0 && (((uintptr_t)out) & 15u) == 0;
#define MO_ONE(U8, VEC, ONE) hipLaunchKernelGGL((k_frame_mosaic<U8, VEC, ONE>), grid, block, 0, st, a)
#define MO_GO(U8, VEC) do { if (n_ch == 1) MO_ONE(U8, VEC, true); else MO_ONE(U8, VEC, false); } while (0)
    if (frames_u8) {
        if (vec) MO_GO(true, true); else MO_GO(true, false);
    } else {
        if (vec) MO_GO(false, true); else MO_GO(false, false);
    }
#undef MO_GO
#undef MO_ONE
    BN_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------------------
// Marker boxes into a finished mosaic, in place (the syllable movie's "first frames of an instance" mark, the
// reference's Rectangle((5, 5), 10, 10) in grey): for every panel (t, r, c) with mark[t, r, c] != 0 the pixels
// [y0, y0 + h) x [x0, x0 + w) of the panel, clipped to it, are set to `value`; nothing else is written.  One wave per
// panel: a wave reads its panel's mark and leaves at once where it is 0 (most panels of a movie), else its lanes walk
// the box's pixels with byte stores.  The box is a few hundred bytes a marked panel: the launch is latency, not
// bandwidth.
#define MO_BOX_THREADS 64

__global__ __launch_bounds__(MO_BOX_THREADS) void k_stamp_boxes(unsigned char* __restrict__ movie, int Cc, int Hp, int Wp,
                                                                const unsigned char* __restrict__ mark, int ya,
                                                                int xa, int hb, int wb, unsigned char value) {
    const unsigned panel = blockIdx.x;                      // (t R + r) Cc + c
    if (!mark[panel]) return;
    const unsigned tr = panel / (unsigned)Cc, c = panel - tr * (unsigned)Cc;
    // (tr Hp counts the mosaic's rows above the panel: t R Hp + r Hp)
    unsigned char* o = movie + ((size_t)tr * (size_t)Hp + (size_t)ya) * ((size_t)Cc * (size_t)Wp) + (size_t)c * (size_t)Wp
                       + (size_t)xa;
    const int px = hb * wb;
    for (int i = threadIdx.x; i < px; i += MO_BOX_THREADS) {
        const int y = i / wb, x = i - y * wb;
        o[(size_t)y * ((size_t)Cc * (size_t)Wp) + (size_t)x] = value;
    }
}

bool bn_stamp_boxes_ok(int T, int R, int Cc, int Hp, int Wp, int y0, int x0, int h, int w, int value) {
    if (T < 0 || R < 0 || Cc < 0 || Hp <= 0 || Wp <= 0 || h < 0 || w < 0 || value < 0 || value > 255) return false;
    const size_t lim = (size_t)1 << 31;
    const size_t panels = (size_t)T * (size_t)R * (size_t)Cc;
    if ((size_t)T * (size_t)R >= lim || panels >= lim) return false;          // (one workgroup a panel, counted in 32 bits)
    // (... and a box's pixels in an int)
    return (size_t)R * (size_t)Hp < lim && (size_t)Cc * (size_t)Wp < lim && (size_t)Hp * (size_t)Wp < lim;
}

int bn_launch_stamp_boxes(unsigned char* movie, int T, int R, int Cc, int Hp, int Wp, const unsigned char* mark, int y0,
                          int x0, int h, int w, int value, hipStream_t st) {
    if (!bn_stamp_boxes_ok(T, R, Cc, Hp, Wp, y0, x0, h, w, value)) return BN_E_SHAPE;
    const size_t panels = (size_t)T * (size_t)R * (size_t)Cc;
    // the box clipped to the panel
    const long long ya = y0 > 0 ? y0 : 0, xa = x0 > 0 ? x0 : 0;
    const long long yb = (long long)y0 + h < Hp ? (long long)y0 + h : Hp;
    const long long xb = (long long)x0 + w < Wp ? (long long)x0 + w : Wp;
    if (panels == 0 || yb <= ya || xb <= xa) return 0;
    hipLaunchKernelGGL(k_stamp_boxes, dim3((unsigned)panels), dim3(MO_BOX_THREADS), 0, st, movie, Cc, Hp, Wp, mark,
                       (int)ya, (int)xa, (int)(yb - ya), (int)(xb - xa), (unsigned char)value);
    BN_LAUNCH_CHECK();
    return 0;
}
