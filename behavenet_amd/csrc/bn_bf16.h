// What the two inference-only bf16 stacks share (conv_bf16.hip: encoder, conv_bf16_dec.hip: decoder): the vector
// types of the 32x32x16 bf16 MFMA, the one rounding rule, the bounds-checked buffer loads and the LDS tile shape.
// (BnBf16Geom, the twelve integers of the C ABI, is in bn_launch.h.)
#pragma once
#include "bn_common.h"
#include "bn_launch.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;

// round to nearest even, NaN stays NaN
__device__ __forceinline__ unsigned bn_f32_to_bf16(float f) {
    unsigned u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// implicit-GEMM tile of the body kernels: 64 reduction values per step, LDS rows padded to 72 bf16 = 144 bytes
// (the 16-byte fragment reads of 16 consecutive rows fall on 16 distinct 4-bank slots), 64 output channels
#define BFC_BK 64
#define BFC_LD 72
#define BFC_BN 64

typedef __amdgpu_buffer_rsrc_t bn_rsrc_t;
typedef __attribute__((ext_vector_type(4))) unsigned bn_u32x4_t;
// bounds-checked view of `bytes` bytes at p (raw buffer, no stride: offsets >= bytes read as zero)
__device__ __forceinline__ bn_rsrc_t bn_make_rsrc(const void* p, size_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ uint4 bn_buf_load16(bn_rsrc_t r, unsigned off) {
    const bn_u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 0);
    return make_uint4(v.x, v.y, v.z, v.w);
}
