// mlp_common.h -- what the kernels that chain Linears on 32x32 MFMA tiles share (mlp.hip, cond_fused.hip, cond_fused_bwd.hip): the operand registers of
// 32 data rows, the tile product over a packed weight tile, the finite SiLU and its derivative, the weight-gradient product over rows and the
// compute-unit count.  mlp.hip states the tile layout.
#pragma once
#include "attn_common.h"

#define MLP_CUS 256                        // the compute units of an MI355X, where the device cannot be asked (mlp_cus)
#define MLP_TILE 1024                      // elements of one packed 32x32 weight tile

// the activations of 32 rows as the next product's B operand: element e of 32-channel tile k is channel 32 k + attn_row(e, h)
template <typename T> struct MlpIn;
template <> struct MlpIn<float> {
    float v[4][16];
    __device__ __forceinline__ void set(int k, int e, float f) { v[k][e] = f; }
};
template <> struct MlpIn<_Float16> {
    attn_h8 v[4][2];
    __device__ __forceinline__ void set(int k, int e, float f) { v[k][e >> 3][e & 7] = (_Float16)f; }     // the one rounding to half
};

// o += W tile x the activations' tile k
__device__ __forceinline__ attn_acc mlp_mm(const _Float16* tile, int lane, const MlpIn<_Float16>& in, int k, attn_acc o)
{
#pragma unroll
    for (int s = 0; s < 2; s++) o = __builtin_amdgcn_mfma_f32_32x32x16_f16(*(const attn_h8*)(tile + (s * 64 + lane) * 8), in.v[k][s], o, 0, 0, 0);
    return o;
}
__device__ __forceinline__ attn_acc mlp_mm(const float* tile, int lane, const MlpIn<float>& in, int k, attn_acc o)
{
#pragma unroll
    for (int g = 0; g < 4; g++) {
        const attn_f4 w = *(const attn_f4*)(tile + (g * 64 + lane) * 4);
#pragma unroll
        for (int u = 0; u < 4; u++) o = __builtin_amdgcn_mfma_f32_32x32x2f32(w[u], in.v[k][4 * g + u], o, 0, 0, 0);
    }
    return o;
}

// v sigmoid(v).  exp(-v) = exp2(t) (1 + tl ln 2) with t + tl = -v log2(e) to about 2^-48 relative: the product's rounding error comes back
// through the fma, so the argument's error does not grow with |v|.  v_exp_f32 and v_rcp_f32 are within 1 ulp each; with the rounding of
// 1 + e and of the last product the result is within 6 u (1 + small) of v sigmoid(v), u = 2^-24 (tests/decoder_restatement.py takes a = 8).
// sigmoid is taken of v held to [-128, 128] (beyond, it is 0 or 1 to float32 anyway) and the exponent is held at 126, so that t, tl, e,
// its correction and 1 + e stay finite for every v: below v = -87.3 the result is v / (1 + 2^126 (1 + tl ln 2)), within |v| 2^-126 of the
// true value (which is smaller still), never inf * c + inf = NaN; above 128 exp2 underflows to 0 and the result is v.  The last product
// takes v itself, so an infinity stays one on the positive side (-inf gives -inf * tiny = -inf where PyTorch gives NaN) and a NaN a NaN.
__device__ __forceinline__ float mlp_silu(float v)
{
    const float L = -1.4426950408889634f, Ll = -1.9259629911266175e-8f;      // -log2(e) = L + Ll
    const float c = __builtin_amdgcn_fmed3f(v, -128.f, 128.f);
    const float t = c * L;
    const float tl = fmaf(c, L, -t) + c * Ll;
    float e = attn_exp2(t > 126.f ? 126.f : t);
    e = fmaf(e, tl * 0.6931471805599453f, e);
    return v * __builtin_amdgcn_rcpf(1.f + e);
}

// d silu(v) / d v = s (1 + v (1 - s)), s = sigmoid(v), on mlp_silu's clamped evaluation of e = exp(-v); 1 - s is taken as e s (no
// cancellation where s is close to 1) and the result as fma(v e s, s, s).  For finite v every term is finite: e <= 2^126 (1 + small),
// s >= 2^-127, e s <= 1, |v e s| <= |v|.  s is within 6 u of sigmoid, e s within 10 u, t = v e s within 11 u; |s t| <= 0.224, so the
// result is within 8 u |silu'| + 3 u of silu'(v) (tests/decoder_grad_restatement.py: SILUP_C, SILUP_ABS).
__device__ __forceinline__ float mlp_silu_grad(float v)
{
    const float L = -1.4426950408889634f, Ll = -1.9259629911266175e-8f;
    const float c = __builtin_amdgcn_fmed3f(v, -128.f, 128.f);
    const float t = c * L;
    const float tl = fmaf(c, L, -t) + c * Ll;
    float e = attn_exp2(t > 126.f ? 126.f : t);
    e = fmaf(e, tl * 0.6931471805599453f, e);
    const float s = __builtin_amdgcn_rcpf(1.f + e);
    return fmaf(v * (e * s), s, s);
}

// sixteen rows of a product over rows: element j of lane half h is row n0 + 8 h + j (half: one v_mfma_f32_32x32x16_f16) or row
// n0 + 2 j + h (float: the j-th of eight v_mfma_f32_32x32x2_f32)
template <typename T> __device__ __forceinline__ constexpr int mlp_wgrad_row(int j, int h) { return AttnCfg<T>::HALF ? 8 * h + j : 2 * j + h; }
__device__ __forceinline__ attn_acc mlp_wgrad_mm(_Float16, const float (&av)[8], const float (&bv)[8], attn_acc o)
{
    attn_h8 a8, b8;
#pragma unroll
    for (int j = 0; j < 8; j++) { a8[j] = (_Float16)av[j]; b8[j] = (_Float16)bv[j]; }
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a8, b8, o, 0, 0, 0);
}
__device__ __forceinline__ attn_acc mlp_wgrad_mm(float, const float (&av)[8], const float (&bv)[8], attn_acc o)
{
#pragma unroll
    for (int j = 0; j < 8; j++) o = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], bv[j], o, 0, 0, 0);
    return o;
}

__host__ __device__ static inline int mlp_tiles(int c) { return (c + 31) / 32; }

// the compute units of the current device (a partition in the CPX modes has fewer than the whole chip), asked once per device
static inline int mlp_cus()
{
    static int cus[64];
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) return MLP_CUS;
    if (cus[d] == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, d) != hipSuccess || n < 1) return MLP_CUS;
        cus[d] = n;
    }
    return cus[d];
}
