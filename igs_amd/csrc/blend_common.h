// blend_common.h -- helpers shared by the forward and backward tile-blend kernels (device only).
#pragma once
#include "common.h"
#include "elem_common.h"      // wg_barrier

// Gaussian exponent exactly as the reference associates it (forward.cu:555, backward.cu:847), WITHOUT fused
// multiply-adds: the sign of a power that rounds to +-1e-8 next to a splat centre decides `if (power > 0) continue`,
// so the operation order is kept identical to the oracle's to keep such threshold flips as rare as they can be.
__device__ __forceinline__ float gauss_power(float cx, float cy, float cz, float dx, float dy)
{
#pragma clang fp contract(off)
    return -0.5f * (cx * dx * dx + cz * dy * dy) - cy * dx * dy;
}

// Which of the four 8x8 quads of a tile can this splat contribute to at all?  bit q = (qy << 1) | qx.
// A pair contributes only if alpha = min(0.99, o * exp(power)) >= 1/255, i.e. power >= -tau with tau = ln(255 o):
// the pixel must lie inside the ellipse  d^T conic d <= 2 tau.  Two conservative tests (margins on tau and on the
// rectangle; any non-finite / non-positive-definite conic means "all quads"), so a pair the reference would blend is
// never removed:
//  1. bounding box of the ellipse (half extents sqrt(2 tau conic.z / det), sqrt(2 tau conic.x / det)) against the quad's
//     pixel-centre rectangle;
//  2. for the quads that survive, the exact minimum of the quadratic form over that rectangle: the form is convex with
//     its minimum (0) at the splat centre, so over a rectangle that does not contain the centre the minimum lies on a
//     face turned towards the centre -- at most two edges, each a 1-D clamped parabola.
// On the bench scene test 2 removes another 17 % of the (quad, splat) rows; 98.8 % of the rows left have a contributing pixel.
__device__ __forceinline__ uint32_t quad_reach_mask(float4 q0, float4 q1, float tile_x0, float tile_y0)
{
    const float o = q1.y;
    if (o < (1.0f / 255.0f)) return 0u;                       // alpha <= o < 1/255 for every pixel
    const float cx = q0.z, cy = q0.w, cz = q1.x;
    const float det = cx * cz - cy * cy;
    if (!(det > 0.f) || !(cx > 0.f) || !(cz > 0.f) || !(det < 3.0e38f)) return 0xFu;
    const float two_tau = 2.0f * __logf(255.0f * o) * 1.002f + 1e-3f;
    if (!(two_tau < 3.0e38f)) return 0xFu;
    // (v_rcp_f32 / v_sqrt_f32, 1 ulp each, instead of the IEEE sequences of `/` and sqrtf: the margins below are a thousand times wider,
    //  and this test runs once per staged splat -- 11 % of the forward's instructions went here)
    const float inv = __builtin_amdgcn_rcpf(det);
    const float ex = __builtin_amdgcn_sqrtf(two_tau * cz * inv) * 1.001f + 0.02f;
    const float ey = __builtin_amdgcn_sqrtf(two_tau * cx * inv) * 1.001f + 0.02f;
    if (!(ex < 3.0e38f) || !(ey < 3.0e38f)) return 0xFu;
    const float lx = q0.x - ex - tile_x0, hx = q0.x + ex - tile_x0;      // reach interval in tile-local pixel coordinates
    const float ly = q0.y - ey - tile_y0, hy = q0.y + ey - tile_y0;
    const bool x0 = (hx >= 0.f) && (lx <= 7.f), x1 = (hx >= 8.f) && (lx <= 15.f);
    const bool y0 = (hy >= 0.f) && (ly <= 7.f), y1 = (hy >= 8.f) && (ly <= 15.f);
    uint32_t m = (x0 && y0 ? 1u : 0u) | (x1 && y0 ? 2u : 0u) | (x0 && y1 ? 4u : 0u) | (x1 && y1 ? 8u : 0u);
    if (m == 0u) return 0u;
    // ---- test 2 (coordinates relative to the splat centre; rectangle inflated by 0.02 px)
    const float nbc = -cy * __builtin_amdgcn_rcpf(cz), nba = -cy * __builtin_amdgcn_rcpf(cx);      // argmin of the form along a vertical / horizontal line
    const float bx = (tile_x0 - 0.02f) - q0.x, by = (tile_y0 - 0.02f) - q0.y;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const float xl = bx + (float)((q & 1) * 8), xh = xl + 7.04f;
        const float yl = by + (float)((q >> 1) * 8), yh = yl + 7.04f;
        const bool xin = (xl <= 0.f) && (xh >= 0.f), yin = (yl <= 0.f) && (yh >= 0.f);
        const float fx = xl > 0.f ? xl : xh;                                   // x of the vertical edge facing the centre
        const float dyv = fminf(fmaxf(nbc * fx, yl), yh);
        const float qv = cx * fx * fx + 2.0f * cy * fx * dyv + cz * dyv * dyv;
        const float fy = yl > 0.f ? yl : yh;                                   // y of the horizontal edge facing the centre
        const float dxh = fminf(fmaxf(nba * fy, xl), xh);
        const float qh = cx * dxh * dxh + 2.0f * cy * dxh * fy + cz * fy * fy;
        float qmin = 3.0e38f;
        if (!xin) qmin = qv;
        if (!yin) qmin = fminf(qmin, qh);
        if (xin && yin) qmin = 0.f;
        if (qmin > two_tau) m &= ~(1u << q);                                   // (a NaN keeps the quad)
    }
    return m;
}

// Six-step reduction trees over the 64 lanes of a wave whose result is wanted in LANE 0 ONLY, in the vector ALU: v_permlane32_swap /
// v_permlane16_swap (gfx950) for the steps of 32 and 16 lanes, DPP row shifts and quad permutes below a row -- no ds_bpermute_b32
// (24 cycles each through the LDS crossbar, tools/ubench; twelve of them per wave and tile were more than one whole splat row).
// The pairing is that of `for (off = 32; off > 0; off >>= 1) x = op(x, __shfl_down(x, off))`: after the step `off` lane i < off holds
// op(x[i], x[i + off]), so lane 0 ends with the same float, bit for bit.  Lanes other than 0 end with values of no meaning.
// DPP controls: row_shl:n = 0x100 + n (lane i reads lane i + n of its row of 16), quad_perm:[2,3,0,1] = 0x4e, quad_perm:[1,0,3,2] = 0xb1;
// a lane whose source lies outside its row reads 0 (bound_ctrl) -- such lanes are never ones lane 0's tree depends on.
template <int CTRL> __device__ __forceinline__ uint32_t dpp_read(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);
}
__device__ __forceinline__ float wave_sum_lane0(float x)
{
    const auto s32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    x = __uint_as_float(s32[0]) + __uint_as_float(s32[1]);
    const auto s16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    x = __uint_as_float(s16[0]) + __uint_as_float(s16[1]);
    x += __uint_as_float(dpp_read<0x108>(__float_as_uint(x)));
    x += __uint_as_float(dpp_read<0x104>(__float_as_uint(x)));
    x += __uint_as_float(dpp_read<0x4e>(__float_as_uint(x)));
    x += __uint_as_float(dpp_read<0xb1>(__float_as_uint(x)));
    return x;
}
__device__ __forceinline__ int wave_max_lane0(int m)      // m >= 0 (a lane reading outside its row takes part with 0)
{
    const auto s32 = __builtin_amdgcn_permlane32_swap((uint32_t)m, (uint32_t)m, false, false);
    m = max((int)s32[0], (int)s32[1]);
    const auto s16 = __builtin_amdgcn_permlane16_swap((uint32_t)m, (uint32_t)m, false, false);
    m = max((int)s16[0], (int)s16[1]);
    m = max(m, (int)dpp_read<0x108>((uint32_t)m));
    m = max(m, (int)dpp_read<0x104>((uint32_t)m));
    m = max(m, (int)dpp_read<0x4e>((uint32_t)m));
    m = max(m, (int)dpp_read<0xb1>((uint32_t)m));
    return m;
}

// wave-uniform copy of a 64-bit value (readfirstlane returns a SIGNED int: widen through uint32_t, not int)
__device__ __forceinline__ uint64_t uniform64(uint64_t v)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return (uint64_t)lo | ((uint64_t)hi << 32);
}
