// geom_bwd.hip -- per-Gaussian backward (one thread per Gaussian), gfx950.
// Fuses what the reference runs as two kernels plus 14 zero-filled temporaries:
//   computeCov2DCUDA (DGR/cuda_rasterizer/backward.cu:145-488), preprocessCUDA backward (:560-628) with the SH
//   backward (:21-140, sh_math.h) and computeCov3D backward (:492-555).
// Input is the 128-byte raw-moment accumulator line written by blend_bwd.hip; every output element is written
// (zeros for culled Gaussians), so the caller needs no memsets.
// The kernel (geom_bwd_kernel, below its phases) is a sequence of phases, each a function of its own here (the plane-fit backward: two, and a tail).
// geom_bwd_views_kernel, further down, runs the same phases once per view of a multi-view call and writes the sum (igs_rast_backward_views).
//
// Quirks of the reference reproduced on purpose:
//  * computeCov2DCUDA is handed dL_dconic in its `conic_opacity` parameter (rasterizer_impl.cu:569), so what it calls
//    combined_opacity is dL_dconic.w;
//  * the conic backward adds kernel_size to a and c, the forward conic does not (backward.cu:377-379);
//  * no quaternion-normalisation backward (backward.cu:554).
#include "sh_math.h"
#include "host_api.h"      // (also include/igs_rast.h: IGS_GROUP_*, masked refine step)

struct GBArgs { GeomBwdArgs a; RefineFuse f; };

// Launch bounds (waves per SIMD).  The colour-only instances (the bench's refine step) fit 128 VGPRs: 4 waves per SIMD and 5 KiB of SH
// rows + 3 KiB of small-group rows per 64-Gaussian workgroup hold 4,096 workgroups on the chip at once, so a 200k-Gaussian grid
// (3,125 workgroups) runs in one round.  The general instances need the plane-fit backward's registers and stay at 2.
#ifndef GEOM_WAVES_PER_EU
#define GEOM_WAVES_PER_EU 2
#endif
#ifndef GEOM_WAVES_PER_EU_COLOUR
#define GEOM_WAVES_PER_EU_COLOUR 4
#endif
#ifdef GEOM_TIMELINE
// debug build only (tools/debug/geom_timeline.py): per workgroup, the 100 MHz clock at the marks of its life
#define GEOM_TL_MARKS 8
#define GEOM_TL_WGS 8192
__device__ unsigned long long g_geom_tl[GEOM_TL_WGS * GEOM_TL_MARKS];
extern "C" int igs_debug_geom_timeline(unsigned long long* host, int n)
{
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_geom_tl), (size_t)n * 8);
}
#define GTL(k) do { if (threadIdx.x == 0 && blockIdx.x < GEOM_TL_WGS) g_geom_tl[blockIdx.x * GEOM_TL_MARKS + (k)] = wall_clock64(); } while (0)
#else
#define GTL(k) do { } while (0)
#endif

// ---------------------------------------------------------------------------------------------
// the values the phases hand on
// ---------------------------------------------------------------------------------------------
// one Gaussian's gradients: zeros for a culled one
struct GaussGrads {
    float3 m2d = make_float3(0, 0, 0), color = make_float3(0, 0, 0), mean = make_float3(0, 0, 0), scale = make_float3(0, 0, 0);
    float opacity = 0.f, cov[6] = { 0, 0, 0, 0, 0, 0 };
    float4 rot = make_float4(0, 0, 0, 0);
};
// the record and accumulator rows of one Gaussian unpacked: what the reference accumulated with atomics (backward.cu:878-1013), camera-plane / ray-plane sums already over fx, fy
struct Moments {
    float Sv0, Sv1, Sv2, c0x, c0y, c1x, c1y, c2x, c2y, drx, dry, dL_dts;
    float3 dL_dnormal;
    float dLc_x, dLc_y, dLc_z, dL_dopacity;      // dL_dconic .x .y .w; dL_dopacity before coef
    float3 mean; float cov3D[6]; uint32_t clamped;
    bool need_planes;        // some plane / depth / normal gradient arrived
};
// what the plane-fit backward hands to the conic and the mean backward (the values of a Gaussian it skips)
struct PlaneFitGrads {
    float dVs[6] = { 0, 0, 0, 0, 0, 0 };            // symmetric sums of dL_dVrk: [00, 01+10, 02+20, 11, 12+21, 22]
    float DN[3][3] = { { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 } };   // dL_dnJ as a math matrix: DN[r][c] = dL_dcnv[r] * rnv[c]
    float plane0 = 0.f, plane1 = 0.f, dL_du = 0.f, dL_dv = 0.f, dL_dl = 0.f, l = 1.f, nl = 1.f;
};
// squares and product of the projected direction (u, v) = (t.x / t.z, t.y / t.z), formed once for the plane fit and the mean backward
struct UvProducts { float u2, v2, uv; };
struct ConicGrads { float dL_da = 0, dL_db = 0, dL_dc = 0; };
// a workgroup's group of Gaussians [g0, g0 + ng) as the sweeps see it: F = 3 M floats of SH per Gaussian, staged rows of SS floats in
// sh_lds (sh_backward) and of 12 floats in small_lds (stage_small_grads)
struct GroupSpan { int g0, ng, M, F, SS, sh_used; float sh_clamp; bool sh_frozen; const float* sh_lds; const float* small_lds; };

// ---------------------------------------------------------------------------------------------
// the phases of the per-Gaussian backward
// ---------------------------------------------------------------------------------------------
// loss_out[0] = loss_bias + sum_k loss_scale_k * sum(loss_shards_k), by the first wave of workgroup 0
__device__ __forceinline__ void post_loss_value(const RefineFuse& fz)
{
    if (blockIdx.x == 0 && threadIdx.x < 64 && fz.loss_out) {
        float v = fz.loss_scale * fz.loss_shards[16 * threadIdx.x];
        if (fz.loss_shards2) v += fz.loss_scale2 * fz.loss_shards2[16 * threadIdx.x];
        if (fz.loss_shards3) v += fz.loss_scale3 * fz.loss_shards3[16 * threadIdx.x];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (threadIdx.x == 0) fz.loss_out[0] = fz.loss_bias + v;
    }
}

// Loads the record and accumulator rows of one Gaussian (and its plane-cache entry) and unpacks them: the raw moments by name, dL_dcolor
// and dL_dmean2D (final as they arrive), the Gaussian's mean and cov3D.  One function: the rows stay values, not a struct in memory
// whose loads the optimiser merges with those of cov3D_precomp into six dword loads through selected addresses.
template <bool COLOUR_ONLY>
__device__ __forceinline__ void load_moments(const GeomBwdArgs& a, int idx, Moments& mo, GaussGrads& o, PlaneCacheEntry& pce)
{
    float4 r0, r1, r2, r4, r5, r6, r7, g0, g1, g2, g3, g4, g5, g6;
    const float4* R4 = (const float4*)(a.rec + (size_t)idx * REC_F);
    const double2* G2 = (const double2*)(a.gacc + (size_t)idx * ((COLOUR_ONLY || a.gacc_compact) ? GACC_COMPACT_F : GACC_F));
    auto G4 = [&](int k) { const double2 u = G2[2 * k], v = G2[2 * k + 1]; return make_float4((float)u.x, (float)u.y, (float)v.x, (float)v.y); };
    r0 = R4[0]; r1 = R4[1]; r2 = R4[2]; r4 = R4[4]; r5 = R4[5]; r6 = R4[6]; r7 = R4[7];
    pce.have = false;
    if (!COLOUR_ONLY && a.plane_cache) pce = plane_cache_fetch(a.plane_cache + (size_t)idx * PLANE_CACHE_F);      // (kernel-uniform condition)
    if (COLOUR_ONLY || a.gacc_compact) {
        // colour-only blend instance: {c0 c1 c2 Q0} {Qx Qy Qxx Qxy} {Qyy Z - -}; every plane / depth / normal moment is zero
        const float4 c0 = G4(0), c1 = G4(1), c2 = G4(2);
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        g0 = make_float4(c0.x, c0.y, c0.z, 0.f); g1 = z; g2 = z; g3 = z;
        g4 = make_float4(0.f, 0.f, c0.w, c1.x); g5 = make_float4(c1.y, c1.z, c1.w, c2.x); g6 = make_float4(c2.y, 0.f, 0.f, 0.f);
    } else {
        g0 = G4(0); g1 = G4(1); g2 = G4(2); g3 = G4(3); g4 = G4(4); g5 = G4(5); g6 = G4(6);
    }
    GTL(1);
    o.color = make_float3(g0.x, g0.y, g0.z);
    const float Sv0 = g0.w, Sv1 = g1.x, Sv2 = g1.y;
    const float Sx0 = g1.z, Sx1 = g1.w, Sx2 = g2.x, Sy0 = g2.y, Sy1 = g2.z, Sy2 = g2.w;
    const float St = g3.x, Stx = g3.y, Sty = g3.z;
    const float3 dL_dnormal = make_float3(g3.w, g4.x, g4.y);
    const float Q0 = g4.z, Qx = g4.w, Qy = g5.x, Qxx = g5.y, Qxy = g5.z, Qyy = g5.w, Z = g6.x;
    const float conx = r0.z, cony = r0.w, conz = r1.x, opac = r1.y;
    const float cpl[6] = { r4.x, r4.y, r4.z, r4.w, r5.x, r5.y };
    const float rplx = r2.z, rply = r2.w;
    const float halfW = 0.5f * a.W, halfH = 0.5f * a.H;                                   // ddelx_dx, ddely_dy (backward.cu:792-793)
    o.m2d.x = (-(conx * Qx + cony * Qy) + cpl[0] * Sv0 + cpl[2] * Sv1 + cpl[4] * Sv2 + rplx * St) * halfW;
    o.m2d.y = (-(conz * Qy + cony * Qx) + cpl[1] * Sv0 + cpl[3] * Sv1 + cpl[5] * Sv2 + rply * St) * halfH;
    o.m2d.z = Z;
    mo.Sv0 = Sv0; mo.Sv1 = Sv1; mo.Sv2 = Sv2; mo.dL_dnormal = dL_dnormal;
    mo.dLc_x = -0.5f * Qxx; mo.dLc_y = -0.5f * Qxy; mo.dLc_z = -0.5f * Qyy;
    mo.c0x = Sx0 / a.fx; mo.c0y = Sy0 / a.fy; mo.c1x = Sx1 / a.fx; mo.c1y = Sy1 / a.fy; mo.c2x = Sx2 / a.fx; mo.c2y = Sy2 / a.fy;
    mo.drx = Stx / a.fx; mo.dry = Sty / a.fy;
    mo.dL_dts = St;
    mo.dL_dopacity = (opac != 0.f) ? Q0 / opac : 0.f;

    mo.mean = make_float3(a.means3D[3 * idx], a.means3D[3 * idx + 1], a.means3D[3 * idx + 2]);
    float (&cov3D)[6] = mo.cov3D;
    if (a.cov3D_precomp) {
#pragma unroll
        for (int k = 0; k < 6; k++) cov3D[k] = a.cov3D_precomp[6 * (size_t)idx + k];
    } else { cov3D[0] = r6.x; cov3D[1] = r6.y; cov3D[2] = r6.z; cov3D[3] = r6.w; cov3D[4] = r7.x; cov3D[5] = r7.y; }
    mo.clamped = __float_as_uint(r7.z);
    // With no plane / depth / normal gradient arriving (e.g. a colour-only loss) every term of the plane-fit backward is an
    // exact zero: skip the eigen-decomposition and that whole block.
    mo.need_planes = !COLOUR_ONLY && ((Sv0 != 0.f) | (Sv1 != 0.f) | (Sv2 != 0.f) | (Sx0 != 0.f) | (Sx1 != 0.f) | (Sx2 != 0.f)
                                      | (Sy0 != 0.f) | (Sy1 != 0.f) | (Sy2 != 0.f) | (St != 0.f) | (Stx != 0.f) | (Sty != 0.f)
                                      | (dL_dnormal.x != 0.f) | (dL_dnormal.y != 0.f) | (dL_dnormal.z != 0.f));
}

// The RaDe-GS plane fit (backward.cu:193-365) for a Gaussian whose fit is not degenerate (`pf` keeps its defaults otherwise): two
// functions and a tail in the kernel's body.  With the tail taken out too, or the whole fit as one function, the compiler builds all
// five instances differently (by the counts, it keeps cov2d_ctx's view-space mean for mean_backward, across the fit): 9 v_add_f32
// and 10 v_mul_f32 fewer in each, two more VGPRs in the fused ones, 36 bytes of scratch in the general masked one.
// What part 1 hands on:
struct PlaneFitMid { float3 m, Wu, NiT_dpa; float dpx, dpy, dL_dnl, tmp, clamp_vb; };
// part 1: through the ray plane, the normal and the camera planes: plane0/1, l, nl, DN, dL_dl, and dL/d(plane) = (dpx, dpy)
__device__ __forceinline__ void plane_fit_planes(const Cov2DCtx& c, const Moments& mo, const UvProducts& p2, PlaneFitGrads& pf, PlaneFitMid& mid)
{
    const float3 t = c.t, dL_dnormal = mo.dL_dnormal;
    const float u = c.txtz, v = c.tytz, u2 = p2.u2, v2 = p2.v2, uv = p2.uv;
    const float c0x = mo.c0x, c0y = mo.c0y, c1x = mo.c1x, c1y = mo.c1y, c2x = mo.c2x, c2y = mo.c2y, drx = mo.drx, dry = mo.dry;
    float (&DN)[3][3] = pf.DN; float &plane0 = pf.plane0, &plane1 = pf.plane1, &dL_dl = pf.dL_dl, &l = pf.l, &nl = pf.nl;
    float3 &m = mid.m, &Wu = mid.Wu, &NiT_dpa = mid.NiT_dpa; float &dpx = mid.dpx, &dpy = mid.dpy, &dL_dnl = mid.dL_dnl, &tmp = mid.tmp, &clamp_vb = mid.clamp_vb;
    const float vb = dot3(c.uvh_m, c.uvh), vbn = dot3(c.uvh_mn, c.uvh);
    l = sqrtf(t.x * t.x + t.y * t.y + t.z * t.z);
    clamp_vb = fmaxf(vb, 0.0000001f); const float clamp_vbn = fmaxf(vbn, 0.0000001f);
    nl = u2 + v2 + 1;
    const float factor_normal = l / nl;
    m = make_float3(c.uvh_mn.x / clamp_vbn, c.uvh_mn.y / clamp_vbn, c.uvh_mn.z / clamp_vbn);   // uvh_m_vb
    plane0 = (v2 + 1) * m.x + (-uv) * m.y + (-u) * m.z;
    plane1 = (-uv) * m.x + (u2 + 1) * m.y + (-v) * m.z;
    const float cp0x = (-(v2 + 1) * t.z + plane0 * t.x) / nl, cp0y = (uv * t.z + plane1 * t.x) / nl;
    const float cp1x = (uv * t.z + plane0 * t.y) / nl,        cp1y = (-(u2 + 1) * t.z + plane1 * t.y) / nl;
    const float cp2x = (t.x + plane0 * t.z) / nl,             cp2y = (t.y + plane1 * t.z) / nl;
    const float rpx = plane0 * factor_normal, rpy = plane1 * factor_normal;
    const float3 rnv = make_float3(-plane0 * factor_normal, -plane1 * factor_normal, -1.f);
    // N (rows): (1/z, 0, x/l), (0, 1/z, y/l), (-x/z^2, -y/z^2, z/l)
    const float n00 = 1 / t.z, n02 = t.x / l, n11 = 1 / t.z, n12 = t.y / l;
    const float n20 = -(t.x) / (t.z * t.z), n21 = -(t.y) / (t.z * t.z), n22 = t.z / l;
    const float3 cnv = make_float3(n00 * rnv.x + 0.0f * rnv.y + n02 * rnv.z, 0.0f * rnv.x + n11 * rnv.y + n12 * rnv.z,
                                   n20 * rnv.x + n21 * rnv.y + n22 * rnv.z);
    const float lv = sqrtf(dot3(cnv, cnv));
    const float3 nv = cnv * (1.0f / lv);
    const float3 dLn_lv = make_float3(dL_dnormal.x / lv, dL_dnormal.y / lv, dL_dnormal.z / lv);
    const float3 dL_dcnv = dLn_lv - nv * dot3(nv, dLn_lv);
    // N^T * dL_dcnv
    const float3 dL_drnv = make_float3(n00 * dL_dcnv.x + 0.0f * dL_dcnv.y + n20 * dL_dcnv.z,
                                       0.0f * dL_dcnv.x + n11 * dL_dcnv.y + n21 * dL_dcnv.z,
                                       n02 * dL_dcnv.x + n12 * dL_dcnv.y + n22 * dL_dcnv.z);
    const float cn[3] = { dL_dcnv.x, dL_dcnv.y, dL_dcnv.z }, rn[3] = { rnv.x, rnv.y, rnv.z };
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int q = 0; q < 3; q++) DN[r][q] = cn[r] * rn[q];
    dL_dl = (-plane0 * dL_drnv.x - plane1 * dL_drnv.y + plane0 * drx + plane1 * dry) / nl;
    dpx = (t.x * c0x + t.y * c1x + t.z * c2x - l * dL_drnv.x + drx * l) / nl;
    dpy = (t.x * c0y + t.y * c1y + t.z * c2y - l * dL_drnv.y + dry * l) / nl;
    dL_dnl = (-c0x * cp0x - c0y * cp0y - c1x * cp1x - c1y * cp1y - c2x * cp2x - c2y * cp2y
                          - dL_drnv.x * rnv.x - dL_drnv.y * rnv.y - drx * rpx - dry * rpy) / nl;
    tmp = dpx * plane0 + dpy * plane1;
    Wu = m3T_vec(c.Rwc, c.uvh);                      // W * uvh = Rwc^T uvh
    // Ni^T * (dpx, dpy, 0):  Ni rows (v2+1,-uv,-u), (-uv,u2+1,-v), (0,0,0)
    NiT_dpa = make_float3((v2 + 1) * dpx + (-uv) * dpy, (-uv) * dpx + (u2 + 1) * dpy, (-u) * dpx + (-v) * dpy);
}
// part 2: to Sigma^-1 (dVs), through the inverse where Sigma is well conditioned and through the smallest eigen-pair where not
__device__ __forceinline__ void plane_fit_sigma(const Cov2DCtx& c, const UvProducts& p2, const PlaneFitMid& mid, float (&dVs)[6])
{
    const float u = c.txtz, v = c.tytz, u2 = p2.u2, v2 = p2.v2, uv = p2.uv;
    const float3 Wu = mid.Wu, NiT_dpa = mid.NiT_dpa; const float dpx = mid.dpx, dpy = mid.dpy, tmp = mid.tmp, clamp_vb = mid.clamp_vb;
    if (c.well) {
        const float3 av = m3_vec(c.Vinv, Wu);
        const float3 inner = Wu * (-tmp) + m3T_vec(c.Rwc, NiT_dpa);
        M3 Vd;
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int q = 0; q < 3; q++) Vd.m[r][q] = c.Vinv.m[r][q] / clamp_vb;
        const float3 bv = m3_vec(Vd, inner);
        const float A_[3] = { av.x, av.y, av.z }, B_[3] = { bv.x, bv.y, bv.z };
        dVs[0] = -(A_[0] * B_[0]); dVs[3] = -(A_[1] * B_[1]); dVs[5] = -(A_[2] * B_[2]);
        dVs[1] = -(A_[1] * B_[0]) + -(A_[0] * B_[1]);
        dVs[2] = -(A_[2] * B_[0]) + -(A_[0] * B_[2]);
        dVs[4] = -(A_[2] * B_[1]) + -(A_[1] * B_[2]);
    } else {
        const float dL_dvb = -tmp / clamp_vb;
        const float3 qv = make_float3((v2 + 1) * (dpx / clamp_vb) + (-uv) * (dpy / clamp_vb),
                                      (-uv) * (dpx / clamp_vb) + (u2 + 1) * (dpy / clamp_vb),
                                      (-u) * (dpx / clamp_vb) + (-v) * (dpy / clamp_vb));
        const float3 rv = Wu * dL_dvb + m3T_vec(c.Rwc, qv);       // dVi = Wu rv^T
        // (dVi + dVi^T) emin = Wu (rv.emin) + rv (Wu.emin)
        const float3 dLv = Wu * dot3(rv, c.emin) + rv * dot3(Wu, c.emin);
        const float evj[3] = { c.ev0, c.ev1, c.ev2 };
        const float3 vcj[3] = { c.vc0, c.vc1, c.vc2 };
        float acc[3][3] = { { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 } };
        const float em[3] = { c.emin.x, c.emin.y, c.emin.z };
#pragma unroll
        for (int j = 0; j < 3; j++) {
            if (j != c.min_id) {
                const float sc = dot3(vcj[j], dLv) / fminf(c.evmin - evj[j], -0.0000001f);
                const float vj[3] = { vcj[j].x * sc, vcj[j].y * sc, vcj[j].z * sc };
#pragma unroll
                for (int r = 0; r < 3; r++)
#pragma unroll
                    for (int q = 0; q < 3; q++) acc[r][q] += vj[r] * em[q];
            }
        }
        dVs[0] = acc[0][0]; dVs[3] = acc[1][1]; dVs[5] = acc[2][2];
        dVs[1] = acc[1][0] + acc[0][1]; dVs[2] = acc[2][0] + acc[0][2]; dVs[4] = acc[2][1] + acc[1][2];
    }
}
// conic and coef backward to the 2D covariance (a, b, c), and from there to dL_dcov3D and dL_dopacity (backward.cu:367-430)
__device__ __forceinline__ void conic_backward(const Cov2DCtx& c, const Moments& mo, const PlaneFitGrads& pf, float ks, ConicGrads& cg, GaussGrads& o)
{
    const float dLc_x = mo.dLc_x, dLc_y = mo.dLc_y, dLc_z = mo.dLc_z;
    const float combined_opacity = dLc_z;          // sic: dL_dconic.w, see header
    float dL_dopacity = mo.dL_dopacity;
    float &dL_da = cg.dL_da, &dL_db = cg.dL_db, &dL_dc = cg.dL_dc;
    float (&o_cov)[6] = o.cov; const float (&dVs)[6] = pf.dVs;
    auto T_ = [&](int c_, int r_) { return c.A[c_][r_]; };
    // backward.cu:367-375 (double literals)
    const float coef = c.coef, det_0 = c.det0, det_1 = c.det1;
    const float opacity = (float)((double)combined_opacity / ((double)coef + 1e-6));
    const float dL_dcoef = dL_dopacity * opacity;
    const float dL_dsqrtcoef = (float)((double)dL_dcoef * 0.5 * 1. / ((double)coef + 1e-6));
    const float dL_ddet0 = (float)((double)dL_dsqrtcoef / ((double)det_1 + 1e-6));
    const float dL_ddet1 = (float)((double)(dL_dsqrtcoef * det_0) * (double)(-1.f / ((double)(det_1 * det_1) + 1e-6)));
    const float dcoef_da = dL_ddet0 * c.cov2[2] + dL_ddet1 * (c.cov2[2] + ks);
    const float dcoef_db = (float)((double)dL_ddet0 * (-2. * (double)c.cov2[1]) + (double)dL_ddet1 * (-2. * (double)c.cov2[1]));
    const float dcoef_dc = dL_ddet0 * c.cov2[0] + dL_ddet1 * (c.cov2[0] + ks);
    const float ca = c.cov2[0] + ks, cb = c.cov2[1], cc = c.cov2[2] + ks;
    const float denom = ca * cc - cb * cb;
    const float denom2inv = 1.0f / ((denom * denom) + 0.0000001f);
    if (denom2inv != 0) {
        dL_da = denom2inv * (-cc * cc * dLc_x + 2 * cb * cc * dLc_y + (denom - ca * cc) * dLc_z);
        dL_dc = denom2inv * (-ca * ca * dLc_z + 2 * ca * cb * dLc_y + (denom - ca * cc) * dLc_x);
        dL_db = denom2inv * 2 * (cb * cc * dLc_x - (denom + 2 * cb * cb) * dLc_y + ca * cb * dLc_z);
        if (c.coef_zero) {
            dL_dopacity = 0;
        } else {
            dL_da += dcoef_da; dL_dc += dcoef_dc; dL_db += dcoef_db;
            dL_dopacity = dL_dopacity * coef;
        }
        o_cov[0] = (T_(0, 0) * T_(0, 0) * dL_da + T_(0, 0) * T_(1, 0) * dL_db + T_(1, 0) * T_(1, 0) * dL_dc);
        o_cov[3] = (T_(0, 1) * T_(0, 1) * dL_da + T_(0, 1) * T_(1, 1) * dL_db + T_(1, 1) * T_(1, 1) * dL_dc);
        o_cov[5] = (T_(0, 2) * T_(0, 2) * dL_da + T_(0, 2) * T_(1, 2) * dL_db + T_(1, 2) * T_(1, 2) * dL_dc);
        o_cov[1] = 2 * T_(0, 0) * T_(0, 1) * dL_da + (T_(0, 0) * T_(1, 1) + T_(0, 1) * T_(1, 0)) * dL_db + 2 * T_(1, 0) * T_(1, 1) * dL_dc;
        o_cov[2] = 2 * T_(0, 0) * T_(0, 2) * dL_da + (T_(0, 0) * T_(1, 2) + T_(0, 2) * T_(1, 0)) * dL_db + 2 * T_(1, 0) * T_(1, 2) * dL_dc;
        o_cov[4] = 2 * T_(0, 2) * T_(0, 1) * dL_da + (T_(0, 1) * T_(1, 2) + T_(0, 2) * T_(1, 1)) * dL_db + 2 * T_(1, 1) * T_(1, 2) * dL_dc;
    }
    o_cov[0] += dVs[0]; o_cov[3] += dVs[3]; o_cov[5] += dVs[5];
    o_cov[1] += dVs[1]; o_cov[2] += dVs[2]; o_cov[4] += dVs[4];
    o.opacity = dL_dopacity;
}

// dL_dT -> dL_dJ -> the view-space mean t -> dL_dmean3D (backward.cu:432-488), plus what reaches the mean through the projection to
// the screen and the view-space depth (preprocessCUDA backward, backward.cu:560-628)
__device__ __forceinline__ void mean_backward(const GeomBwdArgs& a, const Cov2DCtx& c, const Moments& mo, const PlaneFitGrads& pf, const UvProducts& p2,
                                              const ConicGrads& cg, GaussGrads& o)
{
    const float3 t = c.t, mean = mo.mean;
    const float u2 = p2.u2, v2 = p2.v2, uv = p2.uv;
    const float c0x = mo.c0x, c0y = mo.c0y, c1x = mo.c1x, c1y = mo.c1y, c2x = mo.c2x, c2y = mo.c2y;
    const float Sv0 = mo.Sv0, Sv1 = mo.Sv1, Sv2 = mo.Sv2, dL_dts = mo.dL_dts;
    const float dL_da = cg.dL_da, dL_db = cg.dL_db, dL_dc = cg.dL_dc;
    const float (&DN)[3][3] = pf.DN;
    const float plane0 = pf.plane0, plane1 = pf.plane1, dL_du = pf.dL_du, dL_dv = pf.dL_dv, dL_dl = pf.dL_dl, l = pf.l, nl = pf.nl;
    auto T_ = [&](int c_, int r_) { return c.A[c_][r_]; };
    auto V_ = [&](int c_, int r_) { return c.Sigma.m[c_][r_]; };
    const float dL_dT00 = 2 * (T_(0, 0) * V_(0, 0) + T_(0, 1) * V_(0, 1) + T_(0, 2) * V_(0, 2)) * dL_da + (T_(1, 0) * V_(0, 0) + T_(1, 1) * V_(0, 1) + T_(1, 2) * V_(0, 2)) * dL_db;
    const float dL_dT01 = 2 * (T_(0, 0) * V_(1, 0) + T_(0, 1) * V_(1, 1) + T_(0, 2) * V_(1, 2)) * dL_da + (T_(1, 0) * V_(1, 0) + T_(1, 1) * V_(1, 1) + T_(1, 2) * V_(1, 2)) * dL_db;
    const float dL_dT02 = 2 * (T_(0, 0) * V_(2, 0) + T_(0, 1) * V_(2, 1) + T_(0, 2) * V_(2, 2)) * dL_da + (T_(1, 0) * V_(2, 0) + T_(1, 1) * V_(2, 1) + T_(1, 2) * V_(2, 2)) * dL_db;
    const float dL_dT10 = 2 * (T_(1, 0) * V_(0, 0) + T_(1, 1) * V_(0, 1) + T_(1, 2) * V_(0, 2)) * dL_dc + (T_(0, 0) * V_(0, 0) + T_(0, 1) * V_(0, 1) + T_(0, 2) * V_(0, 2)) * dL_db;
    const float dL_dT11 = 2 * (T_(1, 0) * V_(1, 0) + T_(1, 1) * V_(1, 1) + T_(1, 2) * V_(1, 2)) * dL_dc + (T_(0, 0) * V_(1, 0) + T_(0, 1) * V_(1, 1) + T_(0, 2) * V_(1, 2)) * dL_db;
    const float dL_dT12 = 2 * (T_(1, 0) * V_(2, 0) + T_(1, 1) * V_(2, 1) + T_(1, 2) * V_(2, 2)) * dL_dc + (T_(0, 0) * V_(2, 0) + T_(0, 1) * V_(2, 1) + T_(0, 2) * V_(2, 2)) * dL_db;
    // glm W[c][r] = Rwc[c][r]
    const float dL_dJ00 = c.Rwc.m[0][0] * dL_dT00 + c.Rwc.m[0][1] * dL_dT01 + c.Rwc.m[0][2] * dL_dT02;
    const float dL_dJ02 = c.Rwc.m[2][0] * dL_dT00 + c.Rwc.m[2][1] * dL_dT01 + c.Rwc.m[2][2] * dL_dT02;
    const float dL_dJ11 = c.Rwc.m[1][0] * dL_dT10 + c.Rwc.m[1][1] * dL_dT11 + c.Rwc.m[1][2] * dL_dT12;
    const float dL_dJ12 = c.Rwc.m[2][0] * dL_dT10 + c.Rwc.m[2][1] * dL_dT11 + c.Rwc.m[2][2] * dL_dT12;
    const float tz = 1.f / t.z, tz2 = tz * tz, tz3 = tz2 * tz;
    const float l3 = l * l * l;
    // glm dL_dnJ[a][b] = DN[b][a]
    const float dL_dtx = c.xgm * (-a.fx * tz2 * dL_dJ02 + dL_du * tz
                                  - DN[2][0] * tz2 + DN[0][2] * (1 / l - t.x * t.x / l3) + DN[1][2] * (-t.x * t.y / l3) + DN[2][2] * (-t.x * t.z / l3)
                                  + (c0x * plane0 + c0y * plane1 + c2x) / nl
                                  + dL_dl * t.x / l);
    const float dL_dty = c.ygm * (-a.fy * tz2 * dL_dJ12 + dL_dv * tz
                                  - DN[2][1] * tz2 + DN[0][2] * (-t.x * t.y / l3) + DN[1][2] * (1 / l - t.y * t.y / l3) + DN[2][2] * (-t.y * t.z / l3)
                                  + (c1x * plane0 + c1y * plane1 + c2y) / nl
                                  + dL_dl * t.y / l);
    const float dL_dtz = -a.fx * tz2 * dL_dJ00 - a.fy * tz2 * dL_dJ11 + (2 * a.fx * t.x) * tz3 * dL_dJ02 + (2 * a.fy * t.y) * tz3 * dL_dJ12
                         - (dL_du * t.x + dL_dv * t.y) * tz2
                         + (DN[0][0] + DN[1][1]) * (-tz2) + DN[2][0] * (2 * t.x * tz3) + DN[2][1] * (2 * t.y * tz3)
                         + (DN[0][2] * t.x + DN[1][2] * t.y) * (-t.z / l3) + DN[2][2] * (1 / l - t.z * t.z / l3)
                         + (c0x * (-(v2 + 1)) + c0y * uv + c1x * uv + c1y * (-(u2 + 1)) + c2x * plane0 + c2y * plane1) / nl
                         + dL_dl * t.z / l;
    // transformVec4x3Transpose (auxiliary.h:105-113)
    o.mean = make_float3(a.view[0] * dL_dtx + a.view[1] * dL_dty + a.view[2] * dL_dtz,
                         a.view[4] * dL_dtx + a.view[5] * dL_dty + a.view[6] * dL_dtz,
                         a.view[8] * dL_dtx + a.view[9] * dL_dty + a.view[10] * dL_dtz);

    // ================= preprocessCUDA backward (backward.cu:560-628) =================
    const float4 m_hom = xform4x4(mean, a.proj);
    const float m_w = 1.0f / (m_hom.w + 0.0000001f);
    const float* pr = a.proj;
    const float mul1 = (pr[0] * mean.x + pr[4] * mean.y + pr[8] * mean.z + pr[12]) * m_w * m_w;
    const float mul2 = (pr[1] * mean.x + pr[5] * mean.y + pr[9] * mean.z + pr[13]) * m_w * m_w;
    const float gx = o.m2d.x, gy = o.m2d.y;
    const float d1x = (pr[0] * m_w - pr[3] * mul1) * gx + (pr[1] * m_w - pr[3] * mul2) * gy;
    const float d1y = (pr[4] * m_w - pr[7] * mul1) * gx + (pr[5] * m_w - pr[7] * mul2) * gy;
    const float d1z = (pr[8] * m_w - pr[11] * mul1) * gx + (pr[9] * m_w - pr[11] * mul2) * gy;
    const float3 mv = xform4x3(mean, a.view);
    const float tt = sqrtf(mv.x * mv.x + mv.y * mv.y + mv.z * mv.z);
    const float3 q = make_float3(Sv0 + mv.x / tt * dL_dts, Sv1 + mv.y / tt * dL_dts, Sv2 + mv.z / tt * dL_dts);
    const float3 d2 = make_float3(a.view[0] * q.x + a.view[1] * q.y + a.view[2] * q.z,
                                  a.view[4] * q.x + a.view[5] * q.y + a.view[6] * q.z,
                                  a.view[8] * q.x + a.view[9] * q.y + a.view[10] * q.z);
    o.mean.x += d1x + d2.x; o.mean.y += d1y + d2.y; o.mean.z += d1z + d2.z;
}

// SH step: dL_dcolor reaches the mean through the view direction, and its factors of dL_dsh are staged in `dsh` (true) unless the SH
// group is frozen (false); fused kernel, N > 1 exchange: this view's clamp-masked dL_dcolor goes to color_out
template <bool FUSED>
__device__ __forceinline__ bool sh_step(const GeomBwdArgs& a, const RefineFuse& fz, int idx, const Moments& mo, bool sh_frozen, float* dsh, GaussGrads& o)
{
    const float3 dir_orig = mo.mean - make_float3(a.campos[0], a.campos[1], a.campos[2]);
    const float* sh = a.shs + (size_t)idx * a.M * 3;
    if (sh_frozen) o.mean = o.mean + sh_backward<false>(a.D, a.M, sh, dir_orig, mo.clamped, o.color, nullptr);
    else o.mean = o.mean + sh_backward<true>(a.D, a.M, sh, dir_orig, mo.clamped, o.color, dsh);
    if constexpr (FUSED) {
        if (fz.color_out) {
            fz.color_out[3 * (size_t)idx] = (mo.clamped & 1u) ? 0.f : o.color.x;
            fz.color_out[3 * (size_t)idx + 1] = (mo.clamped & 2u) ? 0.f : o.color.y;
            fz.color_out[3 * (size_t)idx + 2] = (mo.clamped & 4u) ? 0.f : o.color.z;
        }
    }
    return !sh_frozen;
}

// computeCov3D backward (backward.cu:492-555): dL_dcov3D -> dL_dscale, dL_drot.  FUSED: scales / rotations are the raw leaves
template <bool FUSED>
__device__ __forceinline__ void cov3d_backward(const GeomBwdArgs& a, int idx, GaussGrads& o)
{
    const float (&o_cov)[6] = o.cov;
    float3 sc = make_float3(a.scales[3 * idx], a.scales[3 * idx + 1], a.scales[3 * idx + 2]);
    float4 qr = make_float4(a.rotations[4 * idx], a.rotations[4 * idx + 1], a.rotations[4 * idx + 2], a.rotations[4 * idx + 3]);
    if constexpr (FUSED) {                   // raw leaves -> activated values, exactly as the forward pass did
        sc = make_float3(act_exp(sc.x), act_exp(sc.y), act_exp(sc.z));
        const float inv = act_inv_norm4(qr.x, qr.y, qr.z, qr.w);
        qr = make_float4(qr.x * inv, qr.y * inv, qr.z * inv, qr.w * inv);
    }
    const float r = qr.x, x = qr.y, y = qr.z, z = qr.w;
    const M3 Rq = quat_rot(qr);
    const float s[3] = { a.scale_modifier * sc.x, a.scale_modifier * sc.y, a.scale_modifier * sc.z };
    float dS[3][3];
    dS[0][0] = o_cov[0]; dS[0][1] = 0.5f * o_cov[1]; dS[0][2] = 0.5f * o_cov[2];
    dS[1][0] = 0.5f * o_cov[1]; dS[1][1] = o_cov[3]; dS[1][2] = 0.5f * o_cov[4];
    dS[2][0] = 0.5f * o_cov[2]; dS[2][1] = 0.5f * o_cov[4]; dS[2][2] = o_cov[5];
    // M = S Rq^T : M[k][j] = s_k Rq[j][k];  dM = (2 M) dSigma
    float dM[3][3];
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int b = 0; b < 3; b++)
            dM[k][b] = (2.0f * (s[k] * Rq.m[0][k])) * dS[0][b] + (2.0f * (s[k] * Rq.m[1][k])) * dS[1][b] + (2.0f * (s[k] * Rq.m[2][k])) * dS[2][b];
    const float ds0 = Rq.m[0][0] * dM[0][0] + Rq.m[1][0] * dM[0][1] + Rq.m[2][0] * dM[0][2];
    const float ds1 = Rq.m[0][1] * dM[1][0] + Rq.m[1][1] * dM[1][1] + Rq.m[2][1] * dM[1][2];
    const float ds2 = Rq.m[0][2] * dM[2][0] + Rq.m[1][2] * dM[2][1] + Rq.m[2][2] * dM[2][2];
    o.scale = make_float3(ds0, ds1, ds2);
    // X[a][b] = glm dL_dMt[a][b] after the column scaling = s_a * dM[a][b]
    auto X_ = [&](int a_, int b_) { return dM[a_][b_] * s[a_]; };
    o.rot.x = 2 * z * (X_(0, 1) - X_(1, 0)) + 2 * y * (X_(2, 0) - X_(0, 2)) + 2 * x * (X_(1, 2) - X_(2, 1));
    o.rot.y = 2 * y * (X_(1, 0) + X_(0, 1)) + 2 * z * (X_(2, 0) + X_(0, 2)) + 2 * r * (X_(1, 2) - X_(2, 1)) - 4 * x * (X_(2, 2) + X_(1, 1));
    o.rot.z = 2 * x * (X_(1, 0) + X_(0, 1)) + 2 * r * (X_(2, 0) - X_(0, 2)) + 2 * z * (X_(1, 2) + X_(2, 1)) - 4 * y * (X_(2, 2) + X_(0, 0));
    o.rot.w = 2 * r * (X_(0, 1) - X_(1, 0)) + 2 * x * (X_(2, 0) + X_(0, 2)) + 2 * y * (X_(1, 2) + X_(2, 1)) - 4 * z * (X_(1, 1) + X_(0, 0));
}

// diff_gaussian_rasterization_rade_clamp/__init__.py:156-162 (means2D, colours, cov3D are not clamped)
__device__ __forceinline__ void clamp_grads(GaussGrads& o, float c)
{
    auto cl = [c](float x) { return clamp_keep_nan(x, c); };
    o.mean = make_float3(cl(o.mean.x), cl(o.mean.y), cl(o.mean.z));
    o.opacity = cl(o.opacity);
    o.scale = make_float3(cl(o.scale.x), cl(o.scale.y), cl(o.scale.z));
    o.rot = make_float4(cl(o.rot.x), cl(o.rot.y), cl(o.rot.z), cl(o.rot.w));
}

// unfused kernel: the gradient arrays (dL_dmean2D and dL_dsh are written elsewhere); true if one of them got a NaN and the caller asked
__device__ __forceinline__ bool write_grads(const GeomBwdArgs& a, int idx, const GaussGrads& o)
{
    a.dL_dcolor[3 * idx] = o.color.x; a.dL_dcolor[3 * idx + 1] = o.color.y; a.dL_dcolor[3 * idx + 2] = o.color.z;
    a.dL_dopacity[idx] = o.opacity;
    a.dL_dmean3D[3 * idx] = o.mean.x; a.dL_dmean3D[3 * idx + 1] = o.mean.y; a.dL_dmean3D[3 * idx + 2] = o.mean.z;
#pragma unroll
    for (int k = 0; k < 6; k++) a.dL_dcov3D[6 * (size_t)idx + k] = o.cov[k];
    a.dL_dscale[3 * idx] = o.scale.x; a.dL_dscale[3 * idx + 1] = o.scale.y; a.dL_dscale[3 * idx + 2] = o.scale.z;
    a.dL_drot[4 * idx] = o.rot.x; a.dL_drot[4 * idx + 1] = o.rot.y; a.dL_drot[4 * idx + 2] = o.rot.z; a.dL_drot[4 * idx + 3] = o.rot.w;
    bool found_nan = false;
    if (a.nan_host) {
        // x != x for every element of means2D, colors, opacity, means3D, scales, rotations (not cov3D: the reference does not look at it)
        const float chk[17] = { o.m2d.x, o.m2d.y, o.m2d.z, o.color.x, o.color.y, o.color.z, o.opacity, o.mean.x, o.mean.y, o.mean.z,
                                o.scale.x, o.scale.y, o.scale.z, o.rot.x, o.rot.y, o.rot.z, o.rot.w };
#pragma unroll
        for (int k = 0; k < 17; k++) found_nan |= chk[k] != chk[k];
    }
    return found_nan;
}

// fused kernel: activation backward (gaussian_model.py:90-127) for this Gaussian's 11 small parameters, staged in its LDS row
// sg[12] = xyz 3 | rotation 4 | opacity 1 | scale 3: the sweeps walk each parameter group's contiguous span of the workgroup with
// coalesced accesses (per-thread 4-byte updates at strides of 12 / 16 bytes cost 30 us for 11 of the 59 parameters)
__device__ __forceinline__ void stage_small_grads(const RefineFuse& fz, int idx, const GaussGrads& o, float* sg)
{
    const float4 o_rot = o.rot;
    const float g_xyz[3] = { o.mean.x, o.mean.y, o.mean.z };
    const float s_op = act_sigmoid(fz.param[fz.off_opacity + idx]);
    const float g_logit = o.opacity * s_op * (1.0f - s_op);
    float g_ls[3], g_rot[4];
    {
        const float* ls = fz.param + fz.off_scale + 3 * (size_t)idx;
        const float go[3] = { o.scale.x, o.scale.y, o.scale.z };
#pragma unroll
        for (int k = 0; k < 3; k++) g_ls[k] = go[k] * act_exp(ls[k]);
        const float* rq = fz.param + fz.off_rot + 4 * (size_t)idx;
        const float q0 = rq[0], q1 = rq[1], q2 = rq[2], q3 = rq[3];
        const float len = sqrtf(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
        const float nrm = fmaxf(len, 1e-12f);
        const float inv = 1.0f / nrm;
        const float n0 = q0 * inv, n1 = q1 * inv, n2 = q2 * inv, n3 = q3 * inv;
        const float dt = n0 * o_rot.x + n1 * o_rot.y + n2 * o_rot.z + n3 * o_rot.w;
        g_rot[0] = (o_rot.x - n0 * dt) * inv; g_rot[1] = (o_rot.y - n1 * dt) * inv;
        g_rot[2] = (o_rot.z - n2 * dt) * inv; g_rot[3] = (o_rot.w - n3 * dt) * inv;
        if (len < 1e-12f) {           // F.normalize below eps: q / eps, and clamp_min passes no gradient -- g / eps, no projection
            g_rot[0] = o_rot.x * inv; g_rot[1] = o_rot.y * inv; g_rot[2] = o_rot.z * inv; g_rot[3] = o_rot.w * inv;
        }
    }
    sg[0] = g_xyz[0]; sg[1] = g_xyz[1]; sg[2] = g_xyz[2];
    sg[3] = g_rot[0]; sg[4] = g_rot[1]; sg[5] = g_rot[2]; sg[6] = g_rot[3];
    sg[7] = g_logit; sg[8] = g_ls[0]; sg[9] = g_ls[1]; sg[10] = g_ls[2];
}

// ---------------------------------------------------------------------------------------------
// the sweeps over a workgroup's spans (all threads, behind the barrier that follows the staging)
// ---------------------------------------------------------------------------------------------
// Adam (common.h: adam_update) on the small groups' parameters with its contractions spelled out, as adam_update_sh does for the SH
// coefficients: m = fma(1 - b1, g, b1 m), v = fma((1 - b2) g, g, b2 v), p -= lr m / fma(sqrt(v), inv_sqrt_bc2, eps).  That is what the
// compiler made of adam_update in these sweeps while they stood in the kernel's body; as functions of their own the contraction
// heuristics picked fma(b2, v, ((1 - b2) g) g) at some of the sites -- one rounding apart, and the count of every opcode the same.
// (Bit for bit against the earlier kernel this was measured on the fast sweep only; for small_group_sweep the evidence is the
// instruction stream -- the same fma operand forms at every site -- and the tolerance tests.)
__device__ __forceinline__ void adam_update_small(float& p, float& m, float& v, float g, float lr, float b1, float b2, float eps, float inv_sqrt_bc2)
{
#pragma clang fp contract(off)
    m = __builtin_fmaf(1.f - b1, g, b1 * m);
    v = __builtin_fmaf((1.f - b2) * g, g, b2 * v);
    p -= lr * m / __builtin_fmaf(sqrtf(v), inv_sqrt_bc2, eps);
}

// Fast path of the in-place update (every span 16-byte aligned, no gradient output; false = not taken): float4 items, the loads of
// two of them in flight per thread before the first is needed.  Only LDS carries state from the per-Gaussian phase into this sweep,
// and one set of item registers is live at a time: that is what fits the colour-only instances in 128 VGPRs (4 waves per SIMD), and
// the other waves of the SIMD cover the rest of the HBM latency.
template <int NT, bool PARTIAL>
__device__ __forceinline__ bool fused_fast_sweep(const RefineFuse& fz, const GroupSpan& sp)
{
    const int g0 = sp.g0, ng = sp.ng, F = sp.F;
    const float* small_lds = sp.small_lds;
    const size_t bx = fz.off_xyz + (size_t)g0 * 3, br = fz.off_rot + (size_t)g0 * 4, bo = fz.off_opacity + (size_t)g0,
                 bs = fz.off_scale + (size_t)g0 * 3, bh = fz.off_sh + (size_t)g0 * F;
    const uintptr_t pa = (uintptr_t)fz.param, ma = (uintptr_t)fz.exp_avg, va = (uintptr_t)fz.exp_avg_sq;
    const bool al = !fz.grad_out && ((F & 3) == 0) && (((pa | ma | va) & 15) == 0) && (((bx | br | bo | bs | bh) & 3) == 0)
                    && ((ng & 3) == 0);
    if (!al) return false;
    constexpr int UB = 2;
    float4 HP[UB], HM[UB], HV[UB];
    auto load = [&](int u, size_t o) {
        HP[u] = ((const float4*)fz.param)[o]; HM[u] = ld_moment((const float4*)fz.exp_avg + o); HV[u] = ld_moment((const float4*)fz.exp_avg_sq + o);
    };
    auto store = [&](int u, size_t o) {
        st_param((float4*)fz.param + o, HP[u]); st_moment((float4*)fz.exp_avg + o, HM[u]); st_moment((float4*)fz.exp_avg_sq + o, HV[u]);
    };
    // -- the four small groups, two at a time: one float4 item per thread and group at most (NT threads, <= 4 NT floats per group)
    const size_t sb[4] = { bx, br, bo, bs };
    const int sk[4] = { 3, 4, 1, 3 }, sfirst[4] = { 0, 3, 7, 8 };
    const float slr[4] = { fz.lr_xyz, fz.lr_rot, fz.lr_opacity, fz.lr_scale };
    // masked refine step: frozen groups (opacity q = 2, scale q = 3) are neither read nor written (kernel-uniform)
    const bool qlive[4] = { true, true, !PARTIAL || (fz.frozen_groups & IGS_GROUP_OPACITY) == 0u, !PARTIAL || (fz.frozen_groups & IGS_GROUP_SCALE) == 0u };
#pragma unroll
    for (int q0 = 0; q0 < 4; q0 += UB) {
#pragma unroll
        for (int u = 0; u < UB; u++)
            if (qlive[q0 + u] && (int)threadIdx.x < (ng * sk[q0 + u]) / 4) load(u, sb[q0 + u] / 4 + threadIdx.x);
#pragma unroll
        for (int u = 0; u < UB; u++) {
            const int q = q0 + u;
            if (qlive[q] && (int)threadIdx.x < (ng * sk[q]) / 4) {
                float g[4];
#pragma unroll
                for (int c = 0; c < 4; c++) { const int e = 4 * (int)threadIdx.x + c, gl = e / sk[q]; g[c] = small_lds[gl * 12 + sfirst[q] + (e - gl * sk[q])]; }
                adam_update4(adam_update_small, HP[u], HM[u], HV[u], make_float4(g[0], g[1], g[2], g[3]), slr[q], fz.b1, fz.b2, fz.eps, fz.inv_sqrt_bc2);
                store(u, sb[q] / 4 + threadIdx.x);
            }
        }
    }
    GTL(4);
    // -- the SH span: float4 item i = Gaussian cur.gl, elements from (row cur.kr, channel cur.kc) on
    const int total4 = sp.sh_frozen ? 0 : (ng * F) >> 2;
    ShCursor cur(4 * (int)threadIdx.x, 4 * NT, sp.M);
    for (int i0 = threadIdx.x; i0 < total4; i0 += UB * NT) {
#pragma unroll
        for (int u = 0; u < UB; u++)
            if (i0 + u * NT < total4) load(u, bh / 4 + i0 + u * NT);
#pragma unroll
        for (int u = 0; u < UB; u++) {
            if (i0 + u * NT < total4) {
                const float4 g = sh_grad4(sp.sh_lds + cur.gl * sp.SS, sp.M, sp.sh_used, cur.kr, cur.kc, sp.sh_clamp);
                adam_update4(adam_update_sh, HP[u], HM[u], HV[u], g, fz.lr_sh, fz.b1, fz.b2, fz.eps, fz.inv_sqrt_bc2);
                store(u, bh / 4 + i0 + u * NT);
            }
            cur.next(sp.M);
        }
    }
    return true;
}

// Fallback of the fused kernel for one small group (any alignment; multi-GPU: the gradient goes to grad_out for the all-reduce
// instead).  Element e of the workgroup's span of group (off, k) belongs to Gaussian e / k, component e % k; `first` = the group's
// place in the staged 12-float rows.
template <int NT>
__device__ __forceinline__ void small_group_sweep(const RefineFuse& fz, const GroupSpan& sp, size_t off, int k, int first, float lr)
{
    const float* small_lds = sp.small_lds;
    const size_t base = off + (size_t)sp.g0 * k;
    const int n = sp.ng * k;
    float* P = fz.grad_out ? fz.grad_out + base : fz.param + base;
    float* Mo = fz.exp_avg + base; float* Vo = fz.exp_avg_sq + base;
    const bool al = (((uintptr_t)P | (uintptr_t)Mo | (uintptr_t)Vo) & 15) == 0;
    const int n4 = al ? n >> 2 : 0;
    for (int i = threadIdx.x; i < n4; i += NT) {
        float g[4];
#pragma unroll
        for (int q = 0; q < 4; q++) { const int e = 4 * i + q, gl = e / k; g[q] = small_lds[gl * 12 + first + (e - gl * k)]; }
        if (fz.grad_out) { ((float4*)P)[i] = make_float4(g[0], g[1], g[2], g[3]); continue; }      // multi-GPU: gradient for the all-reduce
        float4 P4 = ((float4*)P)[i], M4 = ((float4*)Mo)[i], V4 = ((float4*)Vo)[i];
        adam_update4(adam_update_small, P4, M4, V4, make_float4(g[0], g[1], g[2], g[3]), lr, fz.b1, fz.b2, fz.eps, fz.inv_sqrt_bc2);
        ((float4*)P)[i] = P4; ((float4*)Mo)[i] = M4; ((float4*)Vo)[i] = V4;
    }
    for (int e = 4 * n4 + threadIdx.x; e < n; e += NT) {
        const int gl = e / k;
        const float g = small_lds[gl * 12 + first + (e - gl * k)];
        if (fz.grad_out) { P[e] = g; continue; }
        float p = P[e], m = Mo[e], v = Vo[e];
        adam_update_small(p, m, v, g, lr, fz.b1, fz.b2, fz.eps, fz.inv_sqrt_bc2);
        P[e] = p; Mo[e] = m; Vo[e] = v;
    }
}

// The SH span of the workgroup from the staged rows, any alignment: dL_dsh itself (unfused; true if a NaN was written and the caller
// asked), the flat gradient (fused, multi-GPU) or Adam on the SH coefficients of the workgroup's NT Gaussians: one contiguous,
// coalesced span of each buffer
template <bool FUSED, int NT>
__device__ __forceinline__ bool sh_sweep(const GeomBwdArgs& a, const RefineFuse& fz, const GroupSpan& sp)
{
    const int g0 = sp.g0, F = sp.F;
    bool found_nan = false;
    const int total = sp.ng * F;
    float* dst = FUSED ? fz.param + fz.off_sh + (size_t)g0 * F : a.dL_dsh + (size_t)g0 * F;
    float* dst_m = FUSED ? fz.exp_avg + fz.off_sh + (size_t)g0 * F : nullptr;
    float* dst_v = FUSED ? fz.exp_avg_sq + fz.off_sh + (size_t)g0 * F : nullptr;
    bool aligned = ((F & 3) == 0) && ((((uintptr_t)dst) & 15) == 0);
    if constexpr (FUSED) aligned = aligned && (((((uintptr_t)dst_m) | ((uintptr_t)dst_v)) & 15) == 0)
                                   && (!fz.grad_out || (((uintptr_t)(fz.grad_out + fz.off_sh + (size_t)g0 * F)) & 15) == 0);
    if (aligned) {
        const int total4 = total >> 2;
        ShCursor cur(4 * (int)threadIdx.x, 4 * NT, sp.M);
        for (int i = threadIdx.x; i < total4; i += NT, cur.next(sp.M)) {
            const float4 g = sh_grad4(sp.sh_lds + cur.gl * sp.SS, sp.M, sp.sh_used, cur.kr, cur.kc, sp.sh_clamp);
            if (FUSED && fz.grad_out) {
                ((float4*)(fz.grad_out + fz.off_sh + (size_t)g0 * F))[i] = g;
            } else if constexpr (FUSED) {
                float4 P4 = ((float4*)dst)[i], M4 = ((float4*)dst_m)[i], V4 = ((float4*)dst_v)[i];
                adam_update4(adam_update_sh, P4, M4, V4, g, fz.lr_sh, fz.b1, fz.b2, fz.eps, fz.inv_sqrt_bc2);
                ((float4*)dst)[i] = P4; ((float4*)dst_m)[i] = M4; ((float4*)dst_v)[i] = V4;
            } else {
                ((float4*)dst)[i] = g;
                if (a.nan_host) found_nan |= (g.x != g.x) | (g.y != g.y) | (g.z != g.z) | (g.w != g.w);
            }
        }
    } else {
        ShCursor cur((int)threadIdx.x, NT, sp.M);
        for (int i = threadIdx.x; i < total; i += NT, cur.next(sp.M)) {
            const float gv = sh_grad1(sp.sh_lds + cur.gl * sp.SS, sp.M, sp.sh_used, cur.kr, cur.kc, sp.sh_clamp);
            if (FUSED && fz.grad_out) {
                fz.grad_out[fz.off_sh + (size_t)g0 * F + i] = gv;
            } else if constexpr (FUSED) {
                float p = dst[i], m = dst_m[i], v = dst_v[i];
                adam_update_sh(p, m, v, gv, fz.lr_sh, fz.b1, fz.b2, fz.eps, fz.inv_sqrt_bc2);
                dst[i] = p; dst_m[i] = m; dst_v[i] = v;
            } else {
                dst[i] = gv;
                if (a.nan_host) found_nan |= gv != gv;
            }
        }
    }
    return found_nan;
}

// COLOUR_ONLY: the blend backward ran its colour-only instance (compact accumulator rows): every plane / depth / normal moment is an
// exact zero for every Gaussian, so the plane-fit backward and its eigen-decomposition are not even compiled in.  The fused general
// instance takes 152 VGPRs (no scratch) at 2 waves per SIMD for a block this one never executes; this one takes 90 and runs 4 waves
// per SIMD (tests/test_geom_bwd_resources.py holds it to 128).
// PARTIAL: masked refine step with frozen groups (RefineFuse::frozen_groups); false compiles exactly the unmasked kernel.
template <bool FUSED, int NT, bool COLOUR_ONLY, bool PARTIAL = false>
__global__ void __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(COLOUR_ONLY ? GEOM_WAVES_PER_EU_COLOUR : GEOM_WAVES_PER_EU)))
geom_bwd_kernel(const GBArgs args)
{
    const GeomBwdArgs& a = args.a;
    const RefineFuse& fz = args.f;
    if constexpr (FUSED) {
        if ((fz.guard_overflow && *fz.guard_overflow) || (fz.guard_prefilter && *fz.guard_prefilter)) return;   // frame to be redone
        post_loss_value(fz);
    }
    // one workgroup per group of NT Gaussians.  (No grid-stride loop: the compiler hoisted the loop-invariant work out of one and kept
    // it live across the whole body -- 236 VGPRs and 171 spilled SGPRs for the colour-only instance instead of 90 and none.)
    GTL(0);
    const int grp = blockIdx.x;
    const int idx = grp * NT + threadIdx.x;
    // the factors of dL_dsh are staged in LDS (sh_backward: M basis values + 3 masked colour gradients + 1 pad per Gaussian) and the
    // sweep at the end forms the products as it walks the span with coalesced accesses
    extern __shared__ __attribute__((aligned(16))) float sh_lds[];
    __shared__ float small_lds[FUSED ? NT * 12 : 1];      // xyz 3 | rotation 4 | opacity 1 | scale 3 gradients of every thread
    // (masked refine step with the SH group frozen: no SH gradient is formed, the launch gives this kernel no LDS rows for it)
    const bool sh_frozen = PARTIAL && FUSED && (fz.frozen_groups & IGS_GROUP_SH) != 0u;
    const GroupSpan sp = { grp * NT, min(NT, a.P - grp * NT), a.M, 3 * a.M, a.M + 4, min((a.D + 1) * (a.D + 1), a.M),
                           FUSED ? fz.clamp : a.clamp, sh_frozen, sh_lds, small_lds };
    const bool active = idx < a.P;

    GaussGrads o;
    float* dsh = (a.M && !sh_frozen) ? sh_lds + threadIdx.x * sp.SS : nullptr;
    bool sh_written = false;
    bool found_nan = false;          // (!FUSED, a.nan_host: any NaN among the gradients the reference asserts on, __init__.py:156-162)

    if (active && a.radii[idx] > 0) {
        Moments mo;
        PlaneCacheEntry pce;
        load_moments<COLOUR_ONLY>(a, idx, mo, o, pce);          // (GTL(1) between its loads and the unpacking)
        // ================= computeCov2DCUDA (backward.cu:145-488) =================
        Cov2DCtx c;
        cov2d_ctx(c, mo.mean, mo.cov3D, a.view, a.fx, a.fy, a.tan_fovx, a.tan_fovy, a.kernel_size, mo.need_planes,
                  &pce, a.plane_tag);
        PlaneFitGrads pf;
        const float u = c.txtz, v = c.tytz, u2 = u * u, v2 = v * v, uv = u * v;
        const UvProducts p2 = { u2, v2, uv };
        if (!c.degenerate) {
            PlaneFitMid mid;
            plane_fit_planes(c, mo, p2, pf, mid);
            plane_fit_sigma(c, p2, mid, pf.dVs);
            const float3 t = c.t, m = mid.m, NiT_dpa = mid.NiT_dpa; const float nl = pf.nl;
            const float c0x = mo.c0x, c0y = mo.c0y, c1x = mo.c1x, c1y = mo.c1y;
            const float dpx = mid.dpx, dpy = mid.dpy, dL_dnl = mid.dL_dnl, tmp = mid.tmp, clamp_vb = mid.clamp_vb; float &dL_du = pf.dL_du, &dL_dv = pf.dL_dv;
            // the tail: to the projected direction (dL_du, dL_dv).  dL_duvh = 2(-tmp) m + (Cinv/clamp_vb) Ni^T dpa
            M3 Cd;
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int q = 0; q < 3; q++) Cd.m[r][q] = c.Cinv.m[r][q] / clamp_vb;
            const float3 dL_duvh = m * (2 * (-tmp)) + m3_vec(Cd, NiT_dpa);
            // DI = dpa m^T
            const float DI01 = dpx * m.y, DI10 = dpy * m.x, DI11 = dpy * m.y, DI02 = dpx * m.z, DI00 = dpx * m.x, DI12 = dpy * m.z;
            dL_du = dL_dnl * 2 * u + dL_duvh.x + (DI10 + DI01) * (-v) + 2 * DI11 * u - DI02
                    + (c0y * t.y + c1x * t.y + c1y * (-2 * t.x)) / nl;
            dL_dv = dL_dnl * 2 * v + dL_duvh.y + (DI10 + DI01) * (-u) + 2 * DI00 * v - DI12
                    + (c0x * (-2 * t.y) + c0y * t.x + c1x * t.x) / nl;
        }
        ConicGrads cg;
        conic_backward(c, mo, pf, a.kernel_size, cg, o);
        mean_backward(a, c, mo, pf, p2, cg, o);
        GTL(2);
        if (a.shs) sh_written = sh_step<FUSED>(a, fz, idx, mo, sh_frozen, dsh, o);
        if (a.scales) cov3d_backward<FUSED>(a, idx, o);
    }
    if constexpr (FUSED) {
        if (active && fz.color_out && !sh_written) {
            fz.color_out[3 * (size_t)idx] = 0.f; fz.color_out[3 * (size_t)idx + 1] = 0.f; fz.color_out[3 * (size_t)idx + 2] = 0.f;
        }
    }
    if (active) {
        if (!FUSED || a.dL_dmean2D) {
            a.dL_dmean2D[3 * idx] = o.m2d.x; a.dL_dmean2D[3 * idx + 1] = o.m2d.y; a.dL_dmean2D[3 * idx + 2] = o.m2d.z;
        }
        if (sp.sh_clamp > 0.f) clamp_grads(o, sp.sh_clamp);
        if constexpr (FUSED) stage_small_grads(fz, idx, o, small_lds + threadIdx.x * 12);
        else found_nan = write_grads(a, idx, o);
        if (dsh && !sh_written) for (int k = 0; k < a.M + 3; k++) dsh[k] = 0.f;         // (0 * 0: every product +0)
    }
    GTL(3);
    if (a.M) {
        __syncthreads();
        bool fast_done = false;
        if constexpr (FUSED) fast_done = fused_fast_sweep<NT, PARTIAL>(fz, sp);          // (GTL(4) between its small groups and its SH span)
        if (!fast_done) {
            if constexpr (FUSED) {
                small_group_sweep<NT>(fz, sp, fz.off_xyz, 3, 0, fz.lr_xyz);
                small_group_sweep<NT>(fz, sp, fz.off_rot, 4, 3, fz.lr_rot);
                if (!PARTIAL || !(fz.frozen_groups & IGS_GROUP_OPACITY)) small_group_sweep<NT>(fz, sp, fz.off_opacity, 1, 7, fz.lr_opacity);
                if (!PARTIAL || !(fz.frozen_groups & IGS_GROUP_SCALE)) small_group_sweep<NT>(fz, sp, fz.off_scale, 3, 8, fz.lr_scale);
            }
            // N > 1 colour exchange: the SH gradient of the step is rebuilt from the gathered colour gradients, this view's is not needed;
            // masked refine step with the SH group frozen: nothing to update
            const bool skip_sh = sh_frozen || (FUSED && fz.grad_out && (fz.color_out || fz.colors_extracted));
            if (!skip_sh) found_nan |= sh_sweep<FUSED, NT>(a, fz, sp);
        }
    }
    GTL(5);
    if constexpr (!FUSED) {
        // a NaN was written: say so in the caller's verdict word (pinned host memory; the host reads it once an event recorded behind
        // this kernel has completed -- the end of the kernel releases the store system-wide).  No counters: a "last workgroup" scheme
        // (__threadfence() + a done-counter per workgroup) was measured at +37 us for this kernel -- the fence is an L2 write-back on
        // this GPU, and the kernel has just stored 70 MB through that L2 (refine_ops.hip: l1_mean_kernel).
        if (a.nan_host && found_nan) __atomic_store_n(a.nan_host, a.nan_seq, __ATOMIC_RELAXED);
    }
}

hipError_t launch_geom_bwd(hipStream_t s, const GeomBwdArgs& a)
{
    GBArgs g; g.a = a; g.f = RefineFuse();
    const size_t lds = a.M ? (size_t)256 * (a.M + 4) * sizeof(float) : 0;
    hipLaunchKernelGGL((geom_bwd_kernel<false, 256, false>), dim3((a.P + 255) / 256), dim3(256), lds, s, g);
    return hipGetLastError();
}
// The fused kernel alternates a latency-bound phase (per-Gaussian math) with a bandwidth-bound one (Adam over the SH span):
// small workgroups put more of them on a CU, so the two phases of different workgroups overlap.  Per 64-Gaussian workgroup (M = 16):
// 5 KiB of SH rows + 3 KiB of small-group rows = 20 workgroups per CU by LDS (160 KiB), 16 by the colour-only instances' 4 waves per SIMD.
#ifndef GEOM_ADAM_THREADS
#define GEOM_ADAM_THREADS 64
#endif
// dynamic LDS of the fused launch: the staged SH rows (sh_backward), M + 4 floats per Gaussian (tests/test_geom_bwd_resources.py reads it)
extern "C" size_t igs_geom_bwd_adam_dyn_lds(int M) { return (size_t)GEOM_ADAM_THREADS * (M + 4) * sizeof(float); }
hipError_t launch_geom_bwd_adam(hipStream_t s, const GeomBwdArgs& a, const RefineFuse& f)
{
    GBArgs g; g.a = a; g.f = f;
    if (f.first > 0) {
        // masked refine step: the kernel sees the P - first trainable Gaussians as a problem of their own -- every per-Gaussian array
        // and group offset starts at Gaussian `first`; the accumulator rows already do (row gid - first)
        const size_t F0 = (size_t)f.first;
        if (f.first > a.P || f.grad_out || f.color_out || a.dL_dmean2D) return hipErrorInvalidValue;
        g.a.P = a.P - f.first;
        g.a.radii = a.radii + F0; g.a.rec = a.rec + F0 * REC_F;
        g.a.means3D = a.means3D + 3 * F0; g.a.scales = a.scales ? a.scales + 3 * F0 : nullptr;
        g.a.rotations = a.rotations ? a.rotations + 4 * F0 : nullptr; g.a.shs = a.shs ? a.shs + F0 * 3 * a.M : nullptr;
        if (a.plane_cache) g.a.plane_cache = a.plane_cache + F0 * PLANE_CACHE_F;
        if (a.cov3D_precomp) g.a.cov3D_precomp = a.cov3D_precomp + 6 * F0;
        g.f.off_xyz += 3 * F0; g.f.off_rot += 4 * F0; g.f.off_sh += F0 * 3 * a.M; g.f.off_opacity += F0; g.f.off_scale += 3 * F0;
    }
    constexpr int NT = GEOM_ADAM_THREADS;
    const size_t lds = (a.M && !(f.frozen_groups & IGS_GROUP_SH)) ? igs_geom_bwd_adam_dyn_lds(a.M) : 0;
    int blocks = (g.a.P + NT - 1) / NT;
    if (blocks < 1) blocks = 1;          // (everything frozen: workgroup 0 still posts the loss value)
    if (f.frozen_groups) {          // (masked refine step with frozen groups: the instances that test the group bits)
        if (a.gacc_compact) hipLaunchKernelGGL((geom_bwd_kernel<true, NT, true, true>), dim3(blocks), dim3(NT), lds, s, g);
        else                hipLaunchKernelGGL((geom_bwd_kernel<true, NT, false, true>), dim3(blocks), dim3(NT), lds, s, g);
    } else if (a.gacc_compact) hipLaunchKernelGGL((geom_bwd_kernel<true, NT, true>), dim3(blocks), dim3(NT), lds, s, g);
    else                       hipLaunchKernelGGL((geom_bwd_kernel<true, NT, false>), dim3(blocks), dim3(NT), lds, s, g);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// V views of one Gaussian set in one launch (igs_rast_backward_views): the sum over the views of what geom_bwd_kernel<false> writes
// for each of them (gs.py:839-847 renders the same Gaussians once per camera and leaves the sum to autograd's AccumulateGrad).
// ---------------------------------------------------------------------------------------------
// the plane fit's tail as a function, for the view loop below (geom_bwd_kernel keeps it in its body: see plane_fit_planes)
__device__ __forceinline__ void plane_fit_tail(const Cov2DCtx& c, const Moments& mo, const UvProducts& p2, const PlaneFitMid& mid, PlaneFitGrads& pf)
{
    const float u = c.txtz, v = c.tytz;
    const float3 t = c.t, m = mid.m, NiT_dpa = mid.NiT_dpa; const float nl = pf.nl;
    const float c0x = mo.c0x, c0y = mo.c0y, c1x = mo.c1x, c1y = mo.c1y;
    const float dpx = mid.dpx, dpy = mid.dpy, dL_dnl = mid.dL_dnl, tmp = mid.tmp, clamp_vb = mid.clamp_vb;
    M3 Cd;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int q = 0; q < 3; q++) Cd.m[r][q] = c.Cinv.m[r][q] / clamp_vb;
    const float3 dL_duvh = m * (2 * (-tmp)) + m3_vec(Cd, NiT_dpa);
    const float DI01 = dpx * m.y, DI10 = dpy * m.x, DI11 = dpy * m.y, DI02 = dpx * m.z, DI00 = dpx * m.x, DI12 = dpy * m.z;
    pf.dL_du = dL_dnl * 2 * u + dL_duvh.x + (DI10 + DI01) * (-v) + 2 * DI11 * u - DI02 + (c0y * t.y + c1x * t.y + c1y * (-2 * t.x)) / nl;
    pf.dL_dv = dL_dnl * 2 * v + dL_duvh.y + (DI10 + DI01) * (-u) + 2 * DI00 * v - DI12 + (c0x * (-2 * t.y) + c0y * t.x + c1x * t.x) / nl;
}
// one visible Gaussian's gradients under the camera and the rows of `a`: the phases in geom_bwd_kernel's order, dL_dsh left out
__device__ __forceinline__ void view_grads(const GeomBwdArgs& a, int idx, GaussGrads& o)
{
    Moments mo;
    PlaneCacheEntry pce;
    load_moments<false>(a, idx, mo, o, pce);
    Cov2DCtx c;
    cov2d_ctx(c, mo.mean, mo.cov3D, a.view, a.fx, a.fy, a.tan_fovx, a.tan_fovy, a.kernel_size, mo.need_planes, &pce, a.plane_tag);
    PlaneFitGrads pf;
    const float u = c.txtz, v = c.tytz;
    const UvProducts p2 = { u * u, v * v, u * v };
    if (!c.degenerate) {
        PlaneFitMid mid;
        plane_fit_planes(c, mo, p2, pf, mid);
        plane_fit_sigma(c, p2, mid, pf.dVs);
        plane_fit_tail(c, mo, p2, mid, pf);
    }
    ConicGrads cg;
    conic_backward(c, mo, pf, a.kernel_size, cg, o);
    mean_backward(a, c, mo, pf, p2, cg, o);
    if (a.shs) {
        const float3 dir_orig = mo.mean - make_float3(a.campos[0], a.campos[1], a.campos[2]);
        o.mean = o.mean + sh_backward<false>(a.D, a.M, a.shs + (size_t)idx * a.M * 3, dir_orig, mo.clamped, o.color, nullptr);
    }
    if (a.scales) cov3d_backward<false>(a, idx, o);
}

struct GBVArgs { GeomBwdArgs a; GeomBwdViews w; };

// One thread per Gaussian, two loops over the views in index order, each adding into registers; every output row is written once and no
// atomics are involved, so the result depends on the inputs and the view order alone.  A Gaussian that no view sees keeps the +0 its
// sums start from.
//  loop 1: the seven small gradients.  A view's gradients are clamped (clamp variant) before they are added: two single-view calls of
//          the clamp package clamp each view's tensors and autograd adds them afterwards.  dL_dmean2D is per view and is not summed.
//  loop 2: dL_dsh = sum_v basis(direction_v) x masked colour gradient_v, with sh_exchange.hip's convention (b_k * g_c, clamp, add; rows
//          at or beyond (D + 1)^2 stay +0).  It reads three moments and the clamp mask of every view again: 28 bytes per view, against
//          48 more live registers in loop 1.  The two loops' registers overlap instead of adding up: loop 1 holds the general
//          instance's body and 20 sums, loop 2 holds 48 sums and little else.
// The view loop has nothing to hoist but the Gaussian's own mean, scale and rotation -- the cameras are uniform (SGPRs) and the rows
// are a view's own -- which is what kept it clear of the grid-stride loop's register blow-up recorded at geom_bwd_kernel.
template <int NT>
__global__ void __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(GEOM_WAVES_PER_EU)))
geom_bwd_views_kernel(const GBVArgs args)
{
    const GeomBwdArgs& a = args.a;
    const GeomBwdViews& w = args.w;
    const int idx = blockIdx.x * NT + threadIdx.x;
    if (idx >= a.P) return;
    GaussGrads sum;
    bool found_nan = false;
    for (int v = 0; v < w.V; v++) {
        GaussGrads o;
        if (w.radii[(size_t)v * a.P + idx] > 0) {
            GeomBwdArgs av = a;
            av.view = w.views + 16 * v; av.proj = w.projs + 16 * v; av.campos = w.campos + 3 * v;
            av.rec = w.rec[v]; av.gacc = w.gacc[v];
            view_grads(av, idx, o);
        }
        if (w.dL_dmean2D) {
            float* m2d = w.dL_dmean2D + ((size_t)v * a.P + idx) * 3;
            m2d[0] = o.m2d.x; m2d[1] = o.m2d.y; m2d[2] = o.m2d.z;
        }
        if (a.nan_host) found_nan |= (o.m2d.x != o.m2d.x) | (o.m2d.y != o.m2d.y) | (o.m2d.z != o.m2d.z);
        if (a.clamp > 0.f) clamp_grads(o, a.clamp);
        sum.color = sum.color + o.color; sum.mean = sum.mean + o.mean; sum.scale = sum.scale + o.scale;
        sum.opacity += o.opacity;
#pragma unroll
        for (int k = 0; k < 6; k++) sum.cov[k] += o.cov[k];
        sum.rot = make_float4(sum.rot.x + o.rot.x, sum.rot.y + o.rot.y, sum.rot.z + o.rot.z, sum.rot.w + o.rot.w);
    }
    found_nan |= write_grads(a, idx, sum);
    if (a.M) {
        float acc[48];
#pragma unroll
        for (int k = 0; k < 48; k++) acc[k] = 0.f;
        const float3 mean = make_float3(a.means3D[3 * idx], a.means3D[3 * idx + 1], a.means3D[3 * idx + 2]);
        const int used = min((a.D + 1) * (a.D + 1), a.M);
        const int stride = a.gacc_compact ? GACC_COMPACT_F : GACC_F;
        for (int v = 0; v < w.V; v++) {
            if (w.radii[(size_t)v * a.P + idx] <= 0) continue;
            const double* gr = w.gacc[v] + (size_t)idx * stride;
            const uint32_t clamped = __float_as_uint(w.rec[v][(size_t)idx * REC_F + 30]);      // record word 7.z (preprocess.hip)
            const float3 g = make_float3((clamped & 1u) ? 0.f : (float)gr[0], (clamped & 2u) ? 0.f : (float)gr[1], (clamped & 4u) ? 0.f : (float)gr[2]);
            const float3 dir = mean - make_float3(w.campos[3 * v], w.campos[3 * v + 1], w.campos[3 * v + 2]);
            const float len = sqrtf(dot3(dir, dir));
            const float x = dir.x / len, y = dir.y / len, z = dir.z / len;
            float b[16];
#pragma unroll
            for (int k = 0; k < 16; k++) b[k] = 0.f;
            sh_basis(a.D, x, y, z, [&](int k, float bk) { b[k] = bk; });
#pragma unroll
            for (int k = 0; k < 16; k++) {
                if (k < used) {
                    float t0 = b[k] * g.x, t1 = b[k] * g.y, t2 = b[k] * g.z;
                    if (a.clamp > 0.f) { t0 = clamp_keep_nan(t0, a.clamp); t1 = clamp_keep_nan(t1, a.clamp); t2 = clamp_keep_nan(t2, a.clamp); }
                    acc[3 * k] += t0; acc[3 * k + 1] += t1; acc[3 * k + 2] += t2;
                }
            }
        }
        if (a.nan_host) {
#pragma unroll
            for (int k = 0; k < 48; k++) found_nan |= acc[k] != acc[k];
        }
        float* dst = a.dL_dsh + (size_t)idx * a.M * 3;
        if (a.M == 16 && (((uintptr_t)a.dL_dsh) & 15) == 0) {
#pragma unroll
            for (int k = 0; k < 12; k++) ((float4*)dst)[k] = make_float4(acc[4 * k], acc[4 * k + 1], acc[4 * k + 2], acc[4 * k + 3]);
        } else {
#pragma unroll
            for (int k = 0; k < 16; k++)
                if (k < a.M) { dst[3 * k] = acc[3 * k]; dst[3 * k + 1] = acc[3 * k + 1]; dst[3 * k + 2] = acc[3 * k + 2]; }
        }
    }
    if (a.nan_host && found_nan) __atomic_store_n(a.nan_host, a.nan_seq, __ATOMIC_RELAXED);      // (as geom_bwd_kernel reports)
}
#ifndef GEOM_VIEWS_THREADS
#define GEOM_VIEWS_THREADS 128
#endif
hipError_t launch_geom_bwd_views(hipStream_t s, const GeomBwdArgs& a, const GeomBwdViews& w)
{
    if (a.M > 16 || w.V < 1 || w.V > IGS_VIEWS_MAX) return hipErrorInvalidValue;
    GBVArgs g; g.a = a; g.w = w;
    constexpr int NT = GEOM_VIEWS_THREADS;
    hipLaunchKernelGGL((geom_bwd_views_kernel<NT>), dim3((a.P + NT - 1) / NT), dim3(NT), 0, s, g);
    return hipGetLastError();
}

// dL/d(colour) of this view per Gaussian, straight from the blend backward's accumulator rows (moments 0..2), with the semantics of the
// per-Gaussian kernel's `color_out`: channels the SH evaluation clamped at zero (forward.cu:71-73 -> backward.cu:36-40) and
// Gaussians the view does not see give zero.  Lets the N > 1 exchange start one kernel earlier (RefineFuse::color_event).
__global__ void __launch_bounds__(256)
extract_view_colors_kernel(int P, const int* __restrict__ radii, const float* __restrict__ rec, const double* __restrict__ gacc,
                           int stride, int have_sh, float* __restrict__ color_out)
{
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= P) return;
    float3 c = make_float3(0.f, 0.f, 0.f);
    if (have_sh && radii[idx] > 0) {
        const double* gr = gacc + (size_t)idx * stride;
        const float3 g = make_float3((float)gr[0], (float)gr[1], (float)gr[2]);
        const uint32_t clamped = __float_as_uint(rec[(size_t)idx * REC_F + 30]);      // record word 7.z (preprocess.hip)
        c = make_float3((clamped & 1u) ? 0.f : g.x, (clamped & 2u) ? 0.f : g.y, (clamped & 4u) ? 0.f : g.z);
    }
    color_out[3 * (size_t)idx] = c.x; color_out[3 * (size_t)idx + 1] = c.y; color_out[3 * (size_t)idx + 2] = c.z;
}
hipError_t launch_extract_view_colors(hipStream_t s, int P, const int* radii, const float* rec, const double* gacc, int gacc_compact, bool have_sh,
                                      float* color_out)
{
    hipLaunchKernelGGL(extract_view_colors_kernel, dim3((P + 255) / 256), dim3(256), 0, s, P, radii, rec, gacc,
                       gacc_compact ? GACC_COMPACT_F : GACC_F, have_sh ? 1 : 0, color_out);
    return hipGetLastError();
}
