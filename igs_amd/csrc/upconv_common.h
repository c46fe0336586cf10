// upconv_common.h -- what the forward (upconv.hip) and the backward (upconv_bwd.hip) of the fused 2x upsample + 3x3 convolution share:
// the 8 x 32 product tile, the per-dtype configuration, the bilinear source rule and the operand / product wrappers.  upconv.hip states
// the tile layout.
#pragma once
#include "mlp_common.h"

#define UC_TY 8                            // the output tile: rows
#define UC_TX 32                           // and columns (a wave's 32 pixels)
#define UC_UH (UC_TY + 2)                  // the upsampled tile with its one-pixel halo
#define UC_UW (UC_TX + 2)
#define UC_LH (UC_TY / 2 + 2)              // the low-resolution patch under it
#define UC_LW (UC_TX / 2 + 2)
#define UC_LCS (UC_LH * UC_LW + 1)         // its channel stride: odd, so 32 channels fall into 32 banks

// rows per wave, waves, and the stride of an upsampled pixel in elements: 16-byte aligned and an odd number of 16-byte units, so that
// the 128-bit operand reads of 32 neighbouring pixels spread over the banks
template <typename T> struct UcCfg;
// NV: the 16-byte vectors of a lane's share of one weight tile.  RING: the vectors a lane holds, one in use and RING - 1 on their way (float32:
// 5 x 4 products of 64 cycles ahead, float16: 17 x 2 of 32); it divides the 9 OT NV vectors of a k step for every OT, so the ring's slots
// are compile-time registers.  PER_SIMD: the waves per SIMD the registers are held to, two workgroups per compute unit either way
template <> struct UcCfg<float> { enum { ROWS = 1, WAVES = 8, PS = 36, NV = 4, RING = 6, PER_SIMD = 4 }; };
template <> struct UcCfg<_Float16> { enum { ROWS = 2, WAVES = 4, PS = 40, NV = 2, RING = 18, PER_SIMD = 2 }; };

// destination index d of a 2x upsampled axis of length 2 L: source (d + 0.5) / 2 - 0.5 clamped at 0, its neighbour at L - 1.
// w1 is the neighbour's weight; where it is zero (d = 0) the neighbour is the sample itself and takes no part.
__device__ __forceinline__ void uc_source(int d, int L, int& i0, int& i1, float& w1)
{
    const int m = d >> 1;
    if (d & 1) { i0 = m; i1 = m + 1 < L ? m + 1 : L - 1; w1 = 0.25f; }
    else if (m == 0) { i0 = 0; i1 = 0; w1 = 0.f; }
    else { i0 = m - 1; i1 = m; w1 = 0.75f; }
}
__device__ __forceinline__ float uc_lerp(float a, float b, float w1) { return w1 == 0.f ? a : fmaf(1.f - w1, a, w1 * b); }

__device__ __forceinline__ void uc_operand(MlpIn<float>& in, const float* p)
{
#pragma unroll
    for (int g = 0; g < 4; g++) {
        const attn_f4 v = *(const attn_f4*)(p + 4 * g);
#pragma unroll
        for (int u = 0; u < 4; u++) in.v[0][4 * g + u] = v[u];
    }
}
__device__ __forceinline__ void uc_operand(MlpIn<_Float16>& in, const _Float16* p)
{
#pragma unroll
    for (int s = 0; s < 2; s++) in.v[0][s] = *(const attn_h8*)(p + 8 * s);
}

// o += vector v of a lane's share of a weight tile x the operand: mlp_mm's products in mlp_mm's order, the weights in registers
__device__ __forceinline__ attn_acc uc_mm(attn_f4 w, const MlpIn<float>& in, int v, attn_acc o)
{
#pragma unroll
    for (int u = 0; u < 4; u++) o = __builtin_amdgcn_mfma_f32_32x32x2f32(w[u], in.v[0][4 * v + u], o, 0, 0, 0);
    return o;
}
__device__ __forceinline__ attn_acc uc_mm(attn_h8 w, const MlpIn<_Float16>& in, int v, attn_acc o)
{
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(w, in.v[0][v], o, 0, 0, 0);
}
