// attn_common.h -- what the attention kernels share (attn.hip, wattn.hip): the vector types, the accumulator tile's row order
// and the wrappers of the matrix instructions.  attn.hip states the tile layout.
#pragma once
#include "elem_common.h"      // wg_barrier, h4_t

typedef _Float16 attn_h8 __attribute__((ext_vector_type(8)));
typedef float attn_f4 __attribute__((ext_vector_type(4)));
typedef float attn_acc __attribute__((ext_vector_type(16)));

template <typename T> struct AttnCfg;
template <> struct AttnCfg<_Float16> { enum { LS = 72, EPC = 8, CPR = 8, NCH = 2, HALF = 1 }; typedef attn_h8 vec; };
template <> struct AttnCfg<float> { enum { LS = 68, EPC = 4, CPR = 16, NCH = 4, HALF = 0 }; typedef attn_f4 vec; };

__device__ __forceinline__ constexpr int attn_row(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }
__device__ __forceinline__ float attn_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// a lane's share of one 64-channel row: the half h of every k-step
template <typename T> struct AttnRow { typename AttnCfg<T>::vec v[8 / (AttnCfg<T>::HALF + 1)]; };
__device__ __forceinline__ void attn_load_row(AttnRow<_Float16>& f, const _Float16* row, int h)
{
#pragma unroll
    for (int s = 0; s < 4; s++) f.v[s] = *(const attn_h8*)(row + 16 * s + 8 * h);
}
__device__ __forceinline__ void attn_load_row(AttnRow<float>& f, const float* row, int h)
{
#pragma unroll
    for (int t = 0; t < 8; t++) f.v[t] = *(const attn_f4*)(row + 32 * h + 4 * t);
}
// X[i][j] += sum_d A[i][d] B[j][d]
__device__ __forceinline__ attn_acc attn_mm_rows(const AttnRow<_Float16>& a, const AttnRow<_Float16>& b, attn_acc x)
{
#pragma unroll
    for (int s = 0; s < 4; s++) x = __builtin_amdgcn_mfma_f32_32x32x16_f16(a.v[s], b.v[s], x, 0, 0, 0);
    return x;
}
__device__ __forceinline__ attn_acc attn_mm_rows(const AttnRow<float>& a, const AttnRow<float>& b, attn_acc x)
{
#pragma unroll
    for (int t = 0; t < 8; t++)
#pragma unroll
        for (int u = 0; u < 4; u++) x = __builtin_amdgcn_mfma_f32_32x32x2f32(a.v[t][u], b.v[t][u], x, 0, 0, 0);
    return x;
}

// The tile x image product over the 32 image rows ro .. ro + 31, both halves of the 64 channels.
//   XA = false:  Y[d][c] += sum_row M[row][d] X[row][c]   (rows d in registers, column c on the lane: y0 = channels 0-31, y1 = 32-63)
//   XA = true:   Z[c][d] += sum_row X[row][c] M[row][d]   (rows c in registers, channel d on the lane)
template <bool XA>
__device__ __forceinline__ void attn_mm_image(const attn_acc& x, const _Float16* img, int ro, int r, int h, attn_acc& y0, attn_acc& y1)
{
#pragma unroll
    for (int s = 0; s < 2; s++) {
        attn_h8 xf;
#pragma unroll
        for (int j = 0; j < 8; j++) xf[j] = (_Float16)x[8 * s + j];
        const attn_h8 m0 = *(const attn_h8*)(img + r * 72 + ro + 16 * s + 8 * h);
        const attn_h8 m1 = *(const attn_h8*)(img + (r + 32) * 72 + ro + 16 * s + 8 * h);
        if (XA) {
            y0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(xf, m0, y0, 0, 0, 0);
            y1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(xf, m1, y1, 0, 0, 0);
        } else {
            y0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(m0, xf, y0, 0, 0, 0);
            y1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(m1, xf, y1, 0, 0, 0);
        }
    }
}
template <bool XA>
__device__ __forceinline__ void attn_mm_image(const attn_acc& x, const float* img, int ro, int r, int h, attn_acc& y0, attn_acc& y1)
{
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const float* row = img + (ro + attn_row(i, 0) + 4 * h) * 68 + r;
        const float m0 = row[0], m1 = row[32];
        if (XA) {
            y0 = __builtin_amdgcn_mfma_f32_32x32x2f32(x[i], m0, y0, 0, 0, 0);
            y1 = __builtin_amdgcn_mfma_f32_32x32x2f32(x[i], m1, y1, 0, 0, 0);
        } else {
            y0 = __builtin_amdgcn_mfma_f32_32x32x2f32(m0, x[i], y0, 0, 0, 0);
            y1 = __builtin_amdgcn_mfma_f32_32x32x2f32(m1, x[i], y1, 0, 0, 0);
        }
    }
}
