// sh_exchange.hip -- the N > 1 colour exchange, gfx950.
// dL/dSH of a step = sum over the views of basis(direction_v) x dL/dcolour_v.  The ranks gather the 3-float colour gradients of every
// view (12 bytes per Gaussian and view) instead of all-reducing the 48-float SH gradients, and every rank rebuilds the sum here, views
// in rank order -- the same bits everywhere.  The basis expressions and the order of operations are those of sh_backward (sh_math.h;
// W(k, b): b * g, then clamp for the clamp variant, then the sum).
#include "sh_math.h"
#include "host_api.h"

#define IGS_MAX_EXCHANGE_VIEWS 64
struct ShViewCams { float pos[3 * IGS_MAX_EXCHANGE_VIEWS]; };
struct ShAdam { float *param, *exp_avg, *exp_avg_sq; float lr_over_bc1, b1, b2, eps, inv_sqrt_bc2;     // SH spans ([P][M][3]) of the optimiser state
                // optional: the four small groups (xyz 3 | rotation 4 | opacity 1 | scale 3 floats per Gaussian) updated by the same
                // launch from their (already all-reduced) gradients -- one kernel per N > 1 step instead of two: flat optimiser state
                // + flat gradient and the float offsets of the groups in them (lr already divided by bias_correction1)
                float *sm_param = nullptr, *sm_exp_avg = nullptr, *sm_exp_avg_sq = nullptr; const float* sm_grad = nullptr;
                size_t sm_off[4] = {0, 0, 0, 0}; float sm_lr_over_bc1[4] = {0, 0, 0, 0}; };
template <bool ADAM>
__global__ void __launch_bounds__(128)
sh_grad_views_kernel(int P, int D, int M, int V, const float* __restrict__ means3D, const ShViewCams cams,
                     const float* __restrict__ gc, float clamp, float* __restrict__ dsh_out, const ShAdam ad)
{
    const float* campos = cams.pos;
    const int idx = blockIdx.x * 128 + threadIdx.x;
    const bool live = idx < P;
    if (!ADAM && !live) return;                       // (the ADAM variant has a workgroup barrier further down)
    float acc[48];
#pragma unroll
    for (int k = 0; k < 48; k++) acc[k] = 0.f;
    const size_t ci = live ? (size_t)idx : 0;
    const float3 mean = make_float3(means3D[3 * ci], means3D[3 * ci + 1], means3D[3 * ci + 2]);
    for (int v = 0; v < (live ? V : 0); v++) {
        const float* gp = gc + ((size_t)v * P + idx) * 3;
        const float3 g = make_float3(gp[0], gp[1], gp[2]);
        if (g.x == 0.f && g.y == 0.f && g.z == 0.f) continue;          // not seen by this view: exact zeros
        const float3 dir = mean - make_float3(campos[3 * v], campos[3 * v + 1], campos[3 * v + 2]);
        const float len = sqrtf(dot3(dir, dir));
        const float x = dir.x / len, y = dir.y / len, z = dir.z / len;
        float b[16];
#pragma unroll
        for (int k = 0; k < 16; k++) b[k] = 0.f;
        sh_basis(D, x, y, z, [&](int k, float bk) { b[k] = bk; });
        const int used = (D + 1) * (D + 1);
#pragma unroll
        for (int k = 0; k < 16; k++) {
            if (k < used && k < M) {
                float t0 = b[k] * g.x, t1 = b[k] * g.y, t2 = b[k] * g.z;
                if (clamp > 0.f) { t0 = clamp_keep_nan(t0, clamp); t1 = clamp_keep_nan(t1, clamp); t2 = clamp_keep_nan(t2, clamp); }
                acc[3 * k] += t0; acc[3 * k + 1] += t1; acc[3 * k + 2] += t2;
            }
        }
    }
    if constexpr (ADAM) {
        // the Adam update of the workgroup's 128 Gaussians right here (the rebuilt gradient never goes to HBM): rows through LDS
        // (49-float padded), then one coalesced float4 sweep over the contiguous 128 x 3M span of param / exp_avg / exp_avg_sq
        __shared__ float rows[128 * 49];
        const int F = 3 * M;
#pragma unroll
        for (int k = 0; k < 48; k++)
            if (k < F) rows[threadIdx.x * 49 + k] = acc[k];
        __syncthreads();
        const int g0 = blockIdx.x * 128, ng = min(128, P - g0);
        const size_t base = (size_t)g0 * F;
        const int total = ng * F;
        const bool al = ((F & 3) == 0) && ((((uintptr_t)(ad.param + base)) | ((uintptr_t)(ad.exp_avg + base)) | ((uintptr_t)(ad.exp_avg_sq + base))) & 15) == 0;
        const int total4 = al ? total >> 2 : 0;
        float4* P4p = (float4*)(ad.param + base); float4* M4p = (float4*)(ad.exp_avg + base); float4* V4p = (float4*)(ad.exp_avg_sq + base);
        auto row4 = [&](int i) { const int f = 4 * i, g = f / F, k = f - g * F; const float* sp = rows + g * 49 + k; return make_float4(sp[0], sp[1], sp[2], sp[3]); };
        for (int i0 = threadIdx.x; i0 < total4; i0 += 2 * 128) {
            const int i1 = i0 + 128;
            const bool two = i1 < total4;
            float4 Pa = P4p[i0], Ma = ld_moment(M4p + i0), Va = ld_moment(V4p + i0), Pb, Mb, Vb;
            if (two) { Pb = P4p[i1]; Mb = ld_moment(M4p + i1); Vb = ld_moment(V4p + i1); }
            adam_update4(adam_update, Pa, Ma, Va, row4(i0), ad.lr_over_bc1, ad.b1, ad.b2, ad.eps, ad.inv_sqrt_bc2);
            P4p[i0] = Pa; st_moment(M4p + i0, Ma); st_moment(V4p + i0, Va);
            if (two) {
                adam_update4(adam_update, Pb, Mb, Vb, row4(i1), ad.lr_over_bc1, ad.b1, ad.b2, ad.eps, ad.inv_sqrt_bc2);
                P4p[i1] = Pb; st_moment(M4p + i1, Mb); st_moment(V4p + i1, Vb);
            }
        }
        for (int e = 4 * total4 + threadIdx.x; e < total; e += 128) {
            const int g = e / F, k = e - g * F;
            float pp = ad.param[base + e], mm = ad.exp_avg[base + e], vv = ad.exp_avg_sq[base + e];
            adam_update(pp, mm, vv, rows[g * 49 + k], ad.lr_over_bc1, ad.b1, ad.b2, ad.eps, ad.inv_sqrt_bc2);
            ad.param[base + e] = pp; ad.exp_avg[base + e] = mm; ad.exp_avg_sq[base + e] = vv;
        }
        if (ad.sm_param && live) {
            // this Gaussian's 11 small parameters (its position was read above, before it moves)
            constexpr int KS[4] = { 3, 4, 1, 3 };
#pragma unroll
            for (int gk = 0; gk < 4; gk++) {
                const size_t o = ad.sm_off[gk] + (size_t)idx * KS[gk];
#pragma unroll
                for (int c = 0; c < KS[gk]; c++) {
                    float pp = ad.sm_param[o + c], mm = ad.sm_exp_avg[o + c], vv = ad.sm_exp_avg_sq[o + c];
                    adam_update(pp, mm, vv, ad.sm_grad[o + c], ad.sm_lr_over_bc1[gk], ad.b1, ad.b2, ad.eps, ad.inv_sqrt_bc2);
                    ad.sm_param[o + c] = pp; ad.sm_exp_avg[o + c] = mm; ad.sm_exp_avg_sq[o + c] = vv;
                }
            }
        }
        return;
    }
    float* dst = dsh_out + (size_t)idx * M * 3;
    if (M == 16 && (((uintptr_t)dsh_out) & 15) == 0) {
#pragma unroll
        for (int k = 0; k < 12; k++) ((float4*)dst)[k] = make_float4(acc[4 * k], acc[4 * k + 1], acc[4 * k + 2], acc[4 * k + 3]);
        return;
    }
#pragma unroll
    for (int k = 0; k < 16; k++)
        if (k < M) { dst[3 * k] = acc[3 * k]; dst[3 * k + 1] = acc[3 * k + 1]; dst[3 * k + 2] = acc[3 * k + 2]; }
}

// ad == nullptr: the rebuilt gradient goes to dsh_out; otherwise it is applied in place (dsh_out is not looked at)
static hipError_t launch_sh_grad_views(hipStream_t s, int P, int D, int M, int V, const float* means3D, const float* campos_host, const float* gc,
                                       float clamp, float* dsh_out, const ShAdam* ad)
{
    ShViewCams cams;                                  // camera centres travel in the kernel arguments: no device buffer, no copy
    for (int i = 0; i < 3 * V; i++) cams.pos[i] = campos_host[i];
    const dim3 grid((P + 127) / 128), block(128);
    if (ad) hipLaunchKernelGGL(sh_grad_views_kernel<true>, grid, block, 0, s, P, D, M, V, means3D, cams, gc, clamp, (float*)nullptr, *ad);
    else    hipLaunchKernelGGL(sh_grad_views_kernel<false>, grid, block, 0, s, P, D, M, V, means3D, cams, gc, clamp, dsh_out, ShAdam());
    return hipGetLastError();
}

// the sizes every entry point below takes; 0 when they are fine
static int exchange_size_error(const char* fn, int P, int D, int M, int n_views)
{
    if (P < 0 || M < 0 || M > 16 || D < 0 || D > 3 || n_views < 0 || n_views > IGS_MAX_EXCHANGE_VIEWS)
        return fail_in(fn, "bad sizes (at most 64 views)");
    return 0;
}

// the N > 1 exchange's entry points (the contracts are in include/igs_rast.h)
extern "C" int igs_sh_grad_from_view_colors(void* stream, int P, int D, int M, int n_views, const float* means3D, const float* campos,
                                            const float* color_grads, float clamp_grads, float* dL_dsh)
{
    if (const int e = exchange_size_error("igs_sh_grad_from_view_colors", P, D, M, n_views)) return e;
    if (P == 0 || M == 0) return 0;
    if (!means3D || !dL_dsh || (n_views > 0 && (!campos || !color_grads))) return fail_in("igs_sh_grad_from_view_colors", "NULL pointer");
    HIP_TRY(launch_sh_grad_views((hipStream_t)stream, P, D, M, n_views, means3D, campos, color_grads, clamp_grads, dL_dsh, nullptr), "sh_grad_views launch");
    return 0;
}

extern "C" int igs_adam_sh_from_view_colors(void* stream, int P, int D, int M, int n_views, const float* means3D, const float* campos,
                                            const float* color_grads, float clamp_grads, float* param_sh, float* exp_avg_sh, float* exp_avg_sq_sh,
                                            float lr, float beta1, float beta2, float eps, float bias_correction1, float bias_correction2_sqrt)
{
    if (const int e = exchange_size_error("igs_adam_sh_from_view_colors", P, D, M, n_views)) return e;
    if (P == 0 || M == 0) return 0;
    if (!means3D || !param_sh || !exp_avg_sh || !exp_avg_sq_sh || (n_views > 0 && (!campos || !color_grads)))
        return fail_in("igs_adam_sh_from_view_colors", "NULL pointer");
    ShAdam ad; ad.param = param_sh; ad.exp_avg = exp_avg_sh; ad.exp_avg_sq = exp_avg_sq_sh;
    ad.lr_over_bc1 = lr / bias_correction1; ad.b1 = beta1; ad.b2 = beta2; ad.eps = eps; ad.inv_sqrt_bc2 = 1.0f / bias_correction2_sqrt;
    HIP_TRY(launch_sh_grad_views((hipStream_t)stream, P, D, M, n_views, means3D, campos, color_grads, clamp_grads, nullptr, &ad), "sh_adam_views launch");
    return 0;
}

// The whole optimiser step of an N > 1 rank in ONE launch (after the exchange): dL/dSH rebuilt from the gathered per-view colour
// gradients and applied as in igs_adam_sh_from_view_colors, and the four small groups updated from their all-reduced gradients in
// `grad` -- same arithmetic as igs_adam_step_groups.  param / exp_avg / exp_avg_sq / grad are the flat buffers of igs_refine_step,
// off_* float offsets into them.  The directions use the positions as they are BEFORE this update (every thread reads its own
// Gaussian's position first).
extern "C" int igs_adam_exchange_step(void* stream, int P, int D, int M, int n_views, const float* campos, const float* color_grads,
                                      float clamp_grads, float* param, float* exp_avg, float* exp_avg_sq, const float* grad,
                                      size_t off_xyz, size_t off_rot, size_t off_sh, size_t off_opacity, size_t off_scale,
                                      float lr_xyz, float lr_rot, float lr_sh, float lr_opacity, float lr_scale,
                                      float beta1, float beta2, float eps, float bias_correction1, float bias_correction2_sqrt)
{
    if (const int e = exchange_size_error("igs_adam_exchange_step", P, D, M, n_views)) return e;
    if (P == 0) return 0;
    if (!param || !exp_avg || !exp_avg_sq || !grad || (n_views > 0 && (!campos || !color_grads)))
        return fail_in("igs_adam_exchange_step", "NULL pointer");
    ShAdam ad; ad.param = param + off_sh; ad.exp_avg = exp_avg + off_sh; ad.exp_avg_sq = exp_avg_sq + off_sh;
    ad.lr_over_bc1 = lr_sh / bias_correction1; ad.b1 = beta1; ad.b2 = beta2; ad.eps = eps; ad.inv_sqrt_bc2 = 1.0f / bias_correction2_sqrt;
    ad.sm_param = param; ad.sm_exp_avg = exp_avg; ad.sm_exp_avg_sq = exp_avg_sq; ad.sm_grad = grad;
    ad.sm_off[0] = off_xyz; ad.sm_off[1] = off_rot; ad.sm_off[2] = off_opacity; ad.sm_off[3] = off_scale;
    ad.sm_lr_over_bc1[0] = lr_xyz / bias_correction1; ad.sm_lr_over_bc1[1] = lr_rot / bias_correction1;
    ad.sm_lr_over_bc1[2] = lr_opacity / bias_correction1; ad.sm_lr_over_bc1[3] = lr_scale / bias_correction1;
    HIP_TRY(launch_sh_grad_views((hipStream_t)stream, P, D, M, n_views, param + off_xyz, campos, color_grads, clamp_grads, nullptr, &ad),
            "adam_exchange_step launch");
    return 0;
}
