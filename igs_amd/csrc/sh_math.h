// sh_math.h -- spherical harmonics of the per-Gaussian kernels (device only): the constants, the basis, the SH backward, and how the
// staged factors of dL_dsh are read back and applied.  Used by preprocess.hip (constants), geom_bwd.hip and sh_exchange.hip.
// Includes geom_math.h first: everything here is compiled with its `#pragma clang fp contract(off)`.
#pragma once
#include "geom_math.h"

// (not static: a constant the compiler could see through would be folded into the products, e.g. SH_C2[2] * 2.f, and the kernels
// would no longer be the ones that were measured; the host-side shadows are local to every file that includes this)
__constant__ float SH_C0 = 0.28209479177387814f;
__constant__ float SH_C1 = 0.4886025119029199f;
__constant__ float SH_C2[5] = { 1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f, -1.0925484305920792f,
                                0.5462742152960396f };
__constant__ float SH_C3[7] = { -0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f, 0.3731763325901154f,
                                -0.4570457994644658f, 1.445305721320277f, -0.5900435899266435f };

// x clamped to +-c by comparisons: a NaN stays a NaN, as through torch.clamp (fminf / fmaxf would return the bound)
__device__ __forceinline__ float clamp_keep_nan(float x, float c) { return x < -c ? -c : (x > c ? c : x); }

__device__ __forceinline__ float3 dnormvdv(float3 v, float3 dv) {   // auxiliary.h:123-133
    const float sum2 = v.x * v.x + v.y * v.y + v.z * v.z;
    const float invsum32 = 1.0f / sqrtf(sum2 * sum2 * sum2);
    float3 r;
    r.x = ((+sum2 - v.x * v.x) * dv.x - v.y * v.x * dv.y - v.z * v.x * dv.z) * invsum32;
    r.y = (-v.x * v.y * dv.x + (sum2 - v.y * v.y) * dv.y - v.z * v.y * dv.z) * invsum32;
    r.z = (-v.x * v.z * dv.x - v.y * v.z * dv.y + (sum2 - v.z * v.z) * dv.z) * invsum32;
    return r;
}

// The SH basis of the unit direction (x, y, z) up to degree `deg` (backward.cu:21-140): W(k, b_k) for every row k < (deg + 1)^2 and,
// behind the rows of every degree l >= 1 it reaches, after_degree(l, xx, yy, zz, xy, yz, xz) (the products from l = 2 on) for a caller
// with more to do there: a second walk over the degrees would form the products twice.
struct ShNoHook { __device__ __forceinline__ void operator()(int, float, float, float, float, float, float) const {} };
template <class WF, class HF = ShNoHook>
__device__ __forceinline__ void sh_basis(int deg, float x, float y, float z, WF W, HF after_degree = HF())
{
    W(0, SH_C0);
    if (deg > 0) {
        W(1, -SH_C1 * y); W(2, SH_C1 * z); W(3, -SH_C1 * x);
        after_degree(1, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f);
        if (deg > 1) {
            const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
            W(4, SH_C2[0] * xy); W(5, SH_C2[1] * yz); W(6, SH_C2[2] * (2.f * zz - xx - yy)); W(7, SH_C2[3] * xz);
            W(8, SH_C2[4] * (xx - yy));
            after_degree(2, xx, yy, zz, xy, yz, xz);
            if (deg > 2) {
                W(9, SH_C3[0] * y * (3.f * xx - yy)); W(10, SH_C3[1] * xy * z); W(11, SH_C3[2] * y * (4.f * zz - xx - yy));
                W(12, SH_C3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy)); W(13, SH_C3[4] * x * (4.f * zz - xx - yy));
                W(14, SH_C3[5] * z * (xx - yy)); W(15, SH_C3[6] * x * (xx - 3.f * yy));
                after_degree(3, xx, yy, zz, xy, yz, xz);
            }
        }
    }
}

// SH backward (backward.cu:21-140): returns the contribution to dL_dmean through the view direction.  STAGE also stages the factors of
// dL_dsh[M][3] in `bas` (a row of M + 4 floats): bas[k] = basis value b_k for the rows of the active degree, bas[M + c] = the
// clamp-masked dL/dcolour g_c.  dL_dsh[k][c] = b_k * g_c, +0 for rows beyond the active degree: sh_grad4 / sh_grad1 below form
// it where it is consumed (the reference's W(k, b) product, the same single rounding).
// STAGE = false (masked refine step with the SH group frozen): xyz is still trained, so dL/dcolour still reaches the mean through the
// view direction, but no SH gradient is formed; M and bas are not looked at.
template <bool STAGE>
__device__ __forceinline__ float3 sh_backward(int deg, int M, const float* __restrict__ sh, float3 dir_orig, uint32_t clamped,
                                              float3 dL_dcolor, float* __restrict__ bas)
{
    const float len = sqrtf(dot3(dir_orig, dir_orig));
    const float x = dir_orig.x / len, y = dir_orig.y / len, z = dir_orig.z / len;
    const float3 g = make_float3((clamped & 1u) ? 0.f : dL_dcolor.x, (clamped & 2u) ? 0.f : dL_dcolor.y, (clamped & 4u) ? 0.f : dL_dcolor.z);
    auto L = [&](int k) { return make_float3(sh[3 * k], sh[3 * k + 1], sh[3 * k + 2]); };
    auto W = [&](int k, float b) { if constexpr (STAGE) bas[k] = b; };
    if constexpr (STAGE) { bas[M] = g.x; bas[M + 1] = g.y; bas[M + 2] = g.z; }
    float3 dx = make_float3(0, 0, 0), dy = make_float3(0, 0, 0), dz = make_float3(0, 0, 0);      // d colour / d (x, y, z)
    sh_basis(deg, x, y, z, W, [&](int l, float xx, float yy, float zz, float xy, float yz, float xz) {
        if (l == 1) {
            dx = L(3) * (-SH_C1); dy = L(1) * (-SH_C1); dz = L(2) * SH_C1;
        } else if (l == 2) {
            dx = dx + (L(4) * (SH_C2[0] * y) + L(6) * (SH_C2[2] * 2.f * -x) + L(7) * (SH_C2[3] * z) + L(8) * (SH_C2[4] * 2.f * x));
            dy = dy + (L(4) * (SH_C2[0] * x) + L(5) * (SH_C2[1] * z) + L(6) * (SH_C2[2] * 2.f * -y) + L(8) * (SH_C2[4] * 2.f * -y));
            dz = dz + (L(5) * (SH_C2[1] * y) + L(6) * (SH_C2[2] * 2.f * 2.f * z) + L(7) * (SH_C2[3] * x));
        } else {
            dx = dx + (L(9) * (SH_C3[0] * 3.f * 2.f * xy) + L(10) * (SH_C3[1] * yz) + L(11) * (SH_C3[2] * -2.f * xy)
                       + L(12) * (SH_C3[3] * -3.f * 2.f * xz) + L(13) * (SH_C3[4] * (-3.f * xx + 4.f * zz - yy))
                       + L(14) * (SH_C3[5] * 2.f * xz) + L(15) * (SH_C3[6] * 3.f * (xx - yy)));
            dy = dy + (L(9) * (SH_C3[0] * 3.f * (xx - yy)) + L(10) * (SH_C3[1] * xz)
                       + L(11) * (SH_C3[2] * (-3.f * yy + 4.f * zz - xx)) + L(12) * (SH_C3[3] * -3.f * 2.f * yz)
                       + L(13) * (SH_C3[4] * -2.f * xy) + L(14) * (SH_C3[5] * -2.f * yz) + L(15) * (SH_C3[6] * -3.f * 2.f * xy));
            dz = dz + (L(10) * (SH_C3[1] * xy) + L(11) * (SH_C3[2] * 4.f * 2.f * yz) + L(12) * (SH_C3[3] * 3.f * (2.f * zz - xx - yy))
                       + L(13) * (SH_C3[4] * 4.f * 2.f * xz) + L(14) * (SH_C3[5] * (xx - yy)));
        }
    });
    const float3 dL_ddir = make_float3(dot3(dx, g), dot3(dy, g), dot3(dz, g));
    return dnormvdv(dir_orig, dL_ddir);
}

// dL_dsh of one Gaussian from its staged row (sh_backward): elements (row kr, channel kc) onwards in span order, clamped to +-clamp
// when clamp > 0 (clamp variant).  Rows at or beyond `used` = (deg + 1)^2 are an explicit +0 (0 * a negative g_c would be -0).
__device__ __forceinline__ float sh_grad1(const float* bas, int M, int used, int kr, int kc, float clamp)
{
    float x = kr < used ? bas[kr] * bas[M + kc] : 0.f;
    if (clamp > 0.f) x = clamp_keep_nan(x, clamp);
    return x;
}
__device__ __forceinline__ float4 sh_grad4(const float* bas, int M, int used, int kr, int kc, float clamp)
{
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        v[j] = sh_grad1(bas, M, used, kr, kc, clamp);
        if (++kc == 3) { kc = 0; kr++; }
    }
    return make_float4(v[0], v[1], v[2], v[3]);
}
// Adam (common.h: adam_update) on one SH coefficient with its contractions spelled out: m = fma(b1, m, (1 - b1) g),
// v = fma(b2, v, ((1 - b2) g) g), p -= lr m / fma(sqrt(v), inv_sqrt_bc2, eps).  That is what the compiler made of adam_update in this
// sweep while the gradient came from LDS; once the sweep formed b_k * g_c itself the contraction heuristics picked fma(1 - b1, g, b1 m)
// instead -- the same at step 1 (zero moments), one rounding apart from step 2 on.
__device__ __forceinline__ void adam_update_sh(float& p, float& m, float& v, float g, float lr, float b1, float b2, float eps, float inv_sqrt_bc2)
{
#pragma clang fp contract(off)
    m = __builtin_fmaf(b1, m, (1.f - b1) * g);
    v = __builtin_fmaf(b2, v, (1.f - b2) * g * g);
    p -= lr * m / __builtin_fmaf(sqrtf(v), inv_sqrt_bc2, eps);
}
// Walks a workgroup's SH span [ng][M][3] by a fixed stride of elements: element e is Gaussian gl, row kr, channel kc (no division per step).
struct ShCursor {
    int gl, kr, kc, dg, dkr, dkc;
    __device__ __forceinline__ ShCursor(int e0, int step, int M) {
        const int F = 3 * M;
        gl = e0 / F; const int k = e0 - gl * F; kr = k / 3; kc = k - 3 * kr;
        dg = step / F; const int dk = step - dg * F; dkr = dk / 3; dkc = dk - 3 * dkr;
    }
    __device__ __forceinline__ void next(int M) {
        kc += dkc; if (kc >= 3) { kc -= 3; kr++; }
        kr += dkr; gl += dg; if (kr >= M) { kr -= M; gl++; }
    }
};
