// cond_common.h -- one pixel's 33 conditioning channels of IGS.condition3D, shared by ray_condition_kernel (cond.hip), which stores
// them, and condition3d_fused_kernel (cond_fused.hip), which keeps them in registers: the same statements, so the same bits.
// cond_fused.hip and cond_fused_bwd.hip also share how an element of x is loaded and widened (CfRaw, cf_load, cf_widen).
// Device only.  include/igs_rast.h (igs_ray_condition_fwd) defines the channels.
#pragma once
#include <hip/hip_runtime.h>

#define COND_CH 33

// The 16 real spherical harmonics of degree <= 3 as polynomials in (x, y, z), index n (n + 1) + m, Condon-Shortley sign (odd m negative).
// K0 = 1 / (2 sqrt(pi)); K1 = sqrt(3 / (4 pi)); K2 = sqrt(15 / (4 pi)); K20 = sqrt(5 / (16 pi)); K3a = sqrt(35 / (32 pi));
// K3b = sqrt(105 / (4 pi)); K3c = sqrt(21 / (32 pi)); K30 = sqrt(7 / (16 pi)).
__device__ __forceinline__ void cond_sh3(float x, float y, float z, float* o)
{
    const float K0 = 0.282094791773878f, K1 = 0.48860251190292f, K2 = 1.09254843059208f, K20 = 0.31539156525252f;
    const float K3a = 0.590043589926644f, K3b = 2.89061144264055f, K3c = 0.457045799464466f, K30 = 0.373176332590115f;
    const float x2 = x * x, y2 = y * y, z2 = z * z;
    o[0] = K0;
    o[1] = -K1 * y;
    o[2] = K1 * z;
    o[3] = -K1 * x;
    o[4] = K2 * (x * y);
    o[5] = -K2 * (y * z);
    o[6] = fmaf(3.f * K20, z2, -K20);                          // K20 (3 z^2 - 1)
    o[7] = -K2 * (x * z);
    o[8] = (0.5f * K2) * (x2 - y2);
    o[9] = -K3a * y * fmaf(3.f, x2, -y2);
    o[10] = K3b * (x * y) * z;
    o[11] = K3c * y * fmaf(-5.f, z2, 1.f);                     // -K3c y (5 z^2 - 1)
    o[12] = K30 * z * fmaf(5.f, z2, -3.f);
    o[13] = K3c * x * fmaf(-5.f, z2, 1.f);
    o[14] = (0.5f * K3b) * z * (x2 - y2);
    o[15] = -K3a * x * fmaf(-3.f, y2, x2);
}

// t[0 .. 32] of pixel (yo, xo): r = the pixel's (origin, direction), dm = its view's depth map [Hd, Wd]; sy = Hd / H, sx = Wd / W in float32
__device__ __forceinline__ void cond_pixel(const float* __restrict__ r, const float* __restrict__ dm, uint32_t yo, uint32_t xo, int Hd, int Wd,
                                           float sy, float sx, float* t)
{
    const float ox = r[0], oy = r[1], oz = r[2];
    float dx = r[3], dy = r[4], dz = r[5];
    const float len = sqrtf(dx * dx + dy * dy + dz * dz), den = fmaxf(len, 1e-12f);
    dx /= den; dy /= den; dz /= den;
    const float mx = oy * dz - oz * dy, my = oz * dx - ox * dz, mz = ox * dy - oy * dx;      // origin x direction, not normalised
    cond_sh3(dx, dy, dz, t);
    cond_sh3(mx, my, mz, t + 16);
    // bilinear resize, half-pixel centres, the source coordinate clamped at zero, the upper neighbour clamped at the last row / column
    const float fy = fmaxf(sy * ((float)yo + 0.5f) - 0.5f, 0.f), fx = fmaxf(sx * ((float)xo + 0.5f) - 0.5f, 0.f);
    const int y0 = min((int)fy, Hd - 1), x0 = min((int)fx, Wd - 1);
    const int y1 = y0 + (y0 < Hd - 1 ? 1 : 0), x1 = x0 + (x0 < Wd - 1 ? 1 : 0);
    const float ly = fy - (float)y0, lx = fx - (float)x0, hy = 1.f - ly, hx = 1.f - lx;
    const float v00 = dm[(size_t)y0 * Wd + x0], v01 = dm[(size_t)y0 * Wd + x1];
    const float v10 = dm[(size_t)y1 * Wd + x0], v11 = dm[(size_t)y1 * Wd + x1];
    t[32] = hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11);
}

// an element of x as it is loaded (float16: its 16 bits), and widened
template <typename TX> struct CfRaw;
template <> struct CfRaw<float> { typedef float type; };
template <> struct CfRaw<_Float16> { typedef unsigned short type; };
__device__ __forceinline__ float cf_load(const float* p) { return *p; }
__device__ __forceinline__ unsigned short cf_load(const _Float16* p) { return *(const unsigned short*)p; }
__device__ __forceinline__ float cf_widen(float v) { return v; }
__device__ __forceinline__ float cf_widen(unsigned short v) { return (float)__builtin_bit_cast(_Float16, v); }
