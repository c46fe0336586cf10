// cond.hip -- IGS.condition3D's non-GEMM parts for gfx950 (igs/IGS.py:185-210 with ray_to_plucker :286-295, rsh_cart_3 :297-344 and
// ModLN :259-284).  include/igs_rast.h states the contract, DESIGN.md section 15 the byte budget and the figures.
//
//   (1) ray_condition_kernel: per pixel the 33 conditioning channels (degree <= 3 real spherical harmonics of the unit direction and of the
//       raw moment origin x direction, and the bilinearly resized depth).  One thread computes one pixel into an LDS row of 33 floats
//       (an odd stride: no bank conflict); the workgroup then writes its 256 x 33 floats as one contiguous run, lanes across addresses.
//   (2) modln_fwd_kernel: out = LayerNorm_C(x) * (1 + scale) + shift.  x and out are NCHW (a channel's pixels are consecutive), the
//       modulation is pixel-major (a pixel's 2 C values are consecutive), so the two want opposite lane mappings.  A workgroup takes P
//       consecutive pixels of one image and all C channels: x comes in with lanes across pixels into xs[c][P + 1]; each pixel's mean and
//       centred variance are sequential sums over its column (256 / P threads per pixel, combined in a fixed order); the modulation pass
//       runs with lanes across channels (16 lanes x 4 channels, four pixels per wave, so that the transposed LDS access touches 64
//       different banks) and overwrites xs in place; the result leaves with lanes across pixels again.
//   (3) modln_bwd_kernel: the same tile with d out next to x (so half the pixels).  d shift / d scale leave in the channel pass, d x in
//       the pixel pass; every workgroup leaves one row of d weight / d bias partial sums, param_reduce.h adds the rows in
//       workgroup order (in two rounds): no float atomics, bitwise reproducible.
#include "common.h"
#include "elem_common.h"
#include "cond_common.h"                  // COND_CH, cond_sh3, cond_pixel
#include "host_api.h"
#include "param_reduce.h"

#define COND_THREADS 256
#define MODLN_THREADS 256
#define MODLN_LDS_BYTES 65536

// ---------------------------------------------------------------------------------------------------------------------------------
// (1) the ray condition
// ---------------------------------------------------------------------------------------------------------------------------------
// rays [NPIX, 6] = origin, direction; depth [N, Hd, Wd]; cond [NPIX, 33]; NPIX = N * H * W; sy = Hd / H, sx = Wd / W in float32
__global__ void __launch_bounds__(COND_THREADS)
ray_condition_kernel(uint32_t NPIX, int H, int W, int Hd, int Wd, float sy, float sx, const float* __restrict__ rays,
                     const float* __restrict__ depth, float* __restrict__ cond)
{
    __shared__ float tile[COND_THREADS * COND_CH];
    const uint32_t tid = threadIdx.x, pix0 = blockIdx.x * COND_THREADS, pix = pix0 + tid;
    if (pix < NPIX) {
        const uint32_t xo = pix % (uint32_t)W, yo = (pix / (uint32_t)W) % (uint32_t)H, n = pix / (uint32_t)(W * H);
        cond_pixel(rays + (size_t)pix * 6, depth + (size_t)n * Hd * Wd, yo, xo, Hd, Wd, sy, sx, tile + tid * COND_CH);
    }
    wg_barrier();
    const uint32_t left = NPIX - pix0;
    const uint32_t count = (left < COND_THREADS ? left : COND_THREADS) * COND_CH;
    float* dst = cond + (size_t)pix0 * COND_CH;
    for (uint32_t i = tid; i < count; i += COND_THREADS) dst[i] = tile[i];
}

static hipError_t launch_ray_condition(hipStream_t s, int N, int H, int W, int Hd, int Wd, const float* rays, const float* depth, float* cond)
{
    const uint32_t NPIX = (uint32_t)((size_t)N * H * W);
    hipLaunchKernelGGL(ray_condition_kernel, dim3((NPIX + COND_THREADS - 1) / COND_THREADS), dim3(COND_THREADS), 0, s, NPIX, H, W, Hd, Wd,
                       (float)Hd / (float)H, (float)Wd / (float)W, rays, depth, cond);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (2) LayerNorm + modulation, forward
// ---------------------------------------------------------------------------------------------------------------------------------
// the tile's pixel count: the largest power of two <= pmax whose `planes` padded operand tiles and the small arrays fit the LDS budget
static size_t modln_lds_bytes(int C, int P, int planes) { return ((size_t)planes * C * (P + 1) + 2 * MODLN_THREADS + 4 * P) * 4; }
static int modln_tile_log2(int C, int planes, int lp_max)
{
    int lp = lp_max;
    while (lp > 2 && modln_lds_bytes(C, 1 << lp, planes) > MODLN_LDS_BYTES) lp--;
    return lp;                                                 // C = 1024: 8 pixels forward, 4 backward (40 KB)
}

// a tile of `planes` NCHW operands into LDS, lanes across pixels: dst[c * S + p] = src[c * sc + p], p < npix
template <typename T>
__device__ __forceinline__ void modln_load_tile(float* dst, const T* src, size_t sc, int C, int lp, int npix, int vec)
{
    const int S = (1 << lp) + 1;
    if (vec) {
        const int lq = lp - 2, nq = C << lq;
        for (int i = threadIdx.x; i < nq; i += MODLN_THREADS) {
            const int c = i >> lq, p = (i - (c << lq)) << 2;
            if (p < npix) {                                    // (vec: npix is a multiple of four)
                const float4 v = ld4(src + (size_t)c * sc + p);
                float* d = dst + c * S + p;
                d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
            }
        }
    } else {
        const int ne = C << lp;
        for (int i = threadIdx.x; i < ne; i += MODLN_THREADS) {
            const int c = i >> lp, p = i - (c << lp);
            if (p < npix) dst[c * S + p] = ld(src + (size_t)c * sc + p);
        }
    }
}

// the sum of red[k * P + p] over the 256 / P parts of pixel p, in part order (every thread of the pixel gets the same bits)
__device__ __forceinline__ float modln_sum_parts(const float* red, int p, int lp)
{
    float s = 0.f;
    for (int k = 0; k < (MODLN_THREADS >> lp); k++) s += red[(k << lp) + p];
    return s;
}

template <typename TX, typename TM>
__global__ void __launch_bounds__(MODLN_THREADS)
modln_fwd_kernel(int C, int HW, int lp, int tiles_per_img, int vx, int vm, int vo, const TX* __restrict__ x, size_t xs_n, size_t xs_c,
                 const TM* __restrict__ mod, const float* __restrict__ w, const float* __restrict__ b, float eps, float* __restrict__ out,
                 float* __restrict__ mean, float* __restrict__ rstd)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int P = 1 << lp, S = P + 1, tid = threadIdx.x;
    float* xs = lds;
    float* red = xs + (size_t)C * S;
    float* mu = red + 2 * MODLN_THREADS;
    float* rs = mu + P;
    const int n = blockIdx.x / tiles_per_img, p0 = (blockIdx.x - n * tiles_per_img) << lp;
    const int npix = min(P, HW - p0);
    modln_load_tile(xs, x + (size_t)n * xs_n + p0, xs_c, C, lp, npix, vx);
    wg_barrier();
    // statistics: thread (p, q) sums channels q, q + parts, ... of pixel p; the mean first, then the squares of the centred values
    const int p = tid & (P - 1), q = tid >> lp, parts = MODLN_THREADS >> lp;
    float s = 0.f;
    if (p < npix) for (int c = q; c < C; c += parts) s += xs[c * S + p];
    red[tid] = s;
    wg_barrier();
    const float m = modln_sum_parts(red, p, lp) / (float)C;
    float v = 0.f;
    if (p < npix) for (int c = q; c < C; c += parts) { const float a = xs[c * S + p] - m; v = fmaf(a, a, v); }
    red[MODLN_THREADS + tid] = v;
    wg_barrier();
    if (q == 0 && p < npix) {
        const float r = 1.f / sqrtf(modln_sum_parts(red + MODLN_THREADS, p, lp) / (float)C + eps);
        mu[p] = m; rs[p] = r;
        if (mean) { mean[(size_t)n * HW + p0 + p] = m; rstd[(size_t)n * HW + p0 + p] = r; }
    }
    wg_barrier();
    // modulation, lanes across channels: a wave takes four pixels, 16 lanes each
    const int wv = tid >> 6, lane = tid & 63, pg = lane >> 4, l = lane & 15;
    for (int pb = 0; pb < npix; pb += 16) {
        const int pp = pb + wv * 4 + pg;
        if (pp >= npix) continue;
        const float pm = mu[pp], pr = rs[pp];
        const TM* row = mod + ((size_t)n * HW + p0 + pp) * 2 * C;
        if (vm) {
            for (int c = 4 * l; c < C; c += 64) {
                const float4 sh = ld4(row + c), sc = ld4(row + C + c), ww = *(const float4*)(w + c), bb = *(const float4*)(b + c);
                float* d = xs + c * S + pp;
                d[0] = fmaf(fmaf((d[0] - pm) * pr, ww.x, bb.x), 1.f + sc.x, sh.x);
                d[S] = fmaf(fmaf((d[S] - pm) * pr, ww.y, bb.y), 1.f + sc.y, sh.y);
                d[2 * S] = fmaf(fmaf((d[2 * S] - pm) * pr, ww.z, bb.z), 1.f + sc.z, sh.z);
                d[3 * S] = fmaf(fmaf((d[3 * S] - pm) * pr, ww.w, bb.w), 1.f + sc.w, sh.w);
            }
        } else {
            for (int c = l; c < C; c += 16) {
                float* d = xs + c * S + pp;
                d[0] = fmaf(fmaf((d[0] - pm) * pr, w[c], b[c]), 1.f + ld(row + C + c), ld(row + c));
            }
        }
    }
    wg_barrier();
    // the result, lanes across pixels again
    float* ob = out + (size_t)n * C * HW + p0;
    if (vo) {
        const int lq = lp - 2, nq = C << lq;
        for (int i = tid; i < nq; i += MODLN_THREADS) {
            const int c = i >> lq, pp = (i - (c << lq)) << 2;
            if (pp < npix) {
                const float* d = xs + c * S + pp;
                *(float4*)(ob + (size_t)c * HW + pp) = make_float4(d[0], d[1], d[2], d[3]);
            }
        }
    } else {
        const int ne = C << lp;
        for (int i = tid; i < ne; i += MODLN_THREADS) {
            const int c = i >> lp, pp = i - (c << lp);
            if (pp < npix) ob[(size_t)c * HW + pp] = xs[c * S + pp];
        }
    }
}

struct ModlnVec { int x, m, hw; };
// which operands take the four-element path: x planes (16 / 8 byte aligned, strides and H W multiples of four), the modulation rows
// with weight and bias (C a multiple of four), and the float32 NCHW-contiguous tensors (H W a multiple of four)
static ModlnVec modln_vec(int C, int HW, int x_dtype, const void* x, size_t xs_n, size_t xs_c, int mod_dtype, const void* mod, const float* w,
                          const float* b)
{
    ModlnVec v;
    v.hw = (HW & 3) == 0;
    v.x = v.hw && (xs_n & 3) == 0 && (xs_c & 3) == 0 && ptr_aligned(x, vec_grid_bytes(x_dtype));
    v.m = (C & 3) == 0 && ptr_aligned(mod, vec_grid_bytes(mod_dtype)) && ptr_aligned(w, 16) && ptr_aligned(b, 16);
    return v;
}

static hipError_t launch_modln_fwd(hipStream_t s, int N, int C, int HW, int x_dtype, const void* x, size_t xs_n, size_t xs_c, int mod_dtype,
                                   const void* mod, const float* w, const float* b, float eps, float* out, float* mean, float* rstd)
{
    const int lp = modln_tile_log2(C, 1, 6), P = 1 << lp, tpi = (HW + P - 1) / P;
    const size_t lds = modln_lds_bytes(C, P, 1);
    const ModlnVec v = modln_vec(C, HW, x_dtype, x, xs_n, xs_c, mod_dtype, mod, w, b);
    const int vo = v.hw && ptr_aligned(out, 16);
    const dim3 g((unsigned)((size_t)N * tpi)), blk(MODLN_THREADS);
#define MODLN_FWD(TX, TM) hipLaunchKernelGGL((modln_fwd_kernel<TX, TM>), g, blk, lds, s, C, HW, lp, tpi, v.x, v.m, vo, (const TX*)x, xs_n, xs_c, \
                                             (const TM*)mod, w, b, eps, out, mean, rstd)
    if (x_dtype == IGS_DTYPE_F16) { if (mod_dtype == IGS_DTYPE_F16) MODLN_FWD(_Float16, _Float16); else MODLN_FWD(_Float16, float); }
    else { if (mod_dtype == IGS_DTYPE_F16) MODLN_FWD(float, _Float16); else MODLN_FWD(float, float); }
#undef MODLN_FWD
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (3) backward
// ---------------------------------------------------------------------------------------------------------------------------------
static int modln_bwd_log2(int C) { return modln_tile_log2(C, 2, 5); }
static size_t modln_bwd_tiles(int N, int C, int HW) { const int P = 1 << modln_bwd_log2(C); return (size_t)N * ((HW + P - 1) / P); }
static size_t modln_bwd_scratch_bytes(int N, int C, int HW) { return align_up((modln_bwd_tiles(N, C, HW) + PARAM_REDUCE_GROUPS) * 2 * C * 4, 256) + 256; }

// With xh = (x - mu) r, y = xh w + b, gh = g (1 + scale):  d shift = g, d scale = g y, d weight = sum gh xh, d bias = sum gh,
// d x = r (gh w - mean_c(gh w) - xh mean_c(gh w xh)).  part[(tile * 2 + 0) * C + c] / [(tile * 2 + 1) * C + c]: the tile's sums over its pixels.
template <typename TX, typename TM>
__global__ void __launch_bounds__(MODLN_THREADS)
modln_bwd_kernel(int C, int HW, int lp, int tiles_per_img, int vx, int vm, int vg, int vd, const TX* __restrict__ x, size_t xs_n, size_t xs_c,
                 const TM* __restrict__ mod, const float* __restrict__ w, const float* __restrict__ b, const float* __restrict__ mean,
                 const float* __restrict__ rstd, const float* __restrict__ g, TX* __restrict__ dx, TM* __restrict__ dmod,
                 float* __restrict__ part)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int P = 1 << lp, S = P + 1, tid = threadIdx.x;
    float* xs = lds;
    float* gs = xs + (size_t)C * S;
    float* red = gs + (size_t)C * S;
    float* mu = red + 2 * MODLN_THREADS;
    float* rs = mu + P;
    float* m1 = rs + P;
    float* m2 = m1 + P;
    const int n = blockIdx.x / tiles_per_img, p0 = (blockIdx.x - n * tiles_per_img) << lp;
    const int npix = min(P, HW - p0);
    if (tid < npix) { mu[tid] = mean[(size_t)n * HW + p0 + tid]; rs[tid] = rstd[(size_t)n * HW + p0 + tid]; }
    modln_load_tile(xs, x + (size_t)n * xs_n + p0, xs_c, C, lp, npix, vx);
    modln_load_tile(gs, g + (size_t)n * C * HW + p0, (size_t)HW, C, lp, npix, vg);
    wg_barrier();
    // channel pass: xs <- xh, gs <- gh; d shift and d scale leave as rows
    const int wv = tid >> 6, lane = tid & 63, pg = lane >> 4, l = lane & 15;
    for (int pb = 0; pb < npix; pb += 16) {
        const int pp = pb + wv * 4 + pg;
        if (pp >= npix) continue;
        const float pm = mu[pp], pr = rs[pp];
        const size_t ro = ((size_t)n * HW + p0 + pp) * 2 * C;
        const TM* row = mod + ro;
        if (vm) {
            for (int c = 4 * l; c < C; c += 64) {
                const float4 sc = ld4(row + C + c), ww = *(const float4*)(w + c), bb = *(const float4*)(b + c);
                float* d = xs + c * S + pp;
                float* e = gs + c * S + pp;
                const float4 xh = make_float4((d[0] - pm) * pr, (d[S] - pm) * pr, (d[2 * S] - pm) * pr, (d[3 * S] - pm) * pr);
                const float4 gg = make_float4(e[0], e[S], e[2 * S], e[3 * S]);
                if (dmod) {
                    st4(dmod + ro + c, gg);
                    st4(dmod + ro + C + c, make_float4(gg.x * fmaf(xh.x, ww.x, bb.x), gg.y * fmaf(xh.y, ww.y, bb.y),
                                                            gg.z * fmaf(xh.z, ww.z, bb.z), gg.w * fmaf(xh.w, ww.w, bb.w)));
                }
                d[0] = xh.x; d[S] = xh.y; d[2 * S] = xh.z; d[3 * S] = xh.w;
                e[0] = gg.x * (1.f + sc.x); e[S] = gg.y * (1.f + sc.y); e[2 * S] = gg.z * (1.f + sc.z); e[3 * S] = gg.w * (1.f + sc.w);
            }
        } else {
            for (int c = l; c < C; c += 16) {
                float* d = xs + c * S + pp;
                float* e = gs + c * S + pp;
                const float xh = (d[0] - pm) * pr, gg = e[0];
                if (dmod) { st(dmod + ro + c, gg); st(dmod + ro + C + c, gg * fmaf(xh, w[c], b[c])); }
                d[0] = xh;
                e[0] = gg * (1.f + ld(row + C + c));
            }
        }
    }
    wg_barrier();
    // the tile's row of parameter partial sums: one thread per channel, pixels in order
    if (part) {
        float* pw = part + (size_t)blockIdx.x * 2 * C;
        for (int c = tid; c < C; c += MODLN_THREADS) {
            float sw = 0.f, sb = 0.f;
            for (int pp = 0; pp < npix; pp++) { const float gh = gs[c * S + pp]; sw = fmaf(gh, xs[c * S + pp], sw); sb += gh; }
            pw[c] = sw; pw[C + c] = sb;
        }
    }
    if (!dx) return;                                           // (uniform)
    // per pixel: mean_c(gh w) and mean_c(gh w xh)
    const int p = tid & (P - 1), q = tid >> lp, parts = MODLN_THREADS >> lp;
    float s1 = 0.f, s2 = 0.f;
    if (p < npix)
        for (int c = q; c < C; c += parts) { const float gw = gs[c * S + p] * w[c]; s1 += gw; s2 = fmaf(gw, xs[c * S + p], s2); }
    red[tid] = s1; red[MODLN_THREADS + tid] = s2;
    wg_barrier();
    if (q == 0 && p < npix) {
        m1[p] = modln_sum_parts(red, p, lp) / (float)C;
        m2[p] = modln_sum_parts(red + MODLN_THREADS, p, lp) / (float)C;
    }
    wg_barrier();
    TX* db = dx + (size_t)n * C * HW + p0;
    if (vd) {
        const int lq = lp - 2, nq = C << lq;
        for (int i = tid; i < nq; i += MODLN_THREADS) {
            const int c = i >> lq, pp = (i - (c << lq)) << 2;
            if (pp < npix) {
                const float* d = xs + c * S + pp;
                const float* e = gs + c * S + pp;
                const float wc = w[c];
                float4 o;
                o.x = rs[pp] * (fmaf(e[0], wc, -m1[pp]) - d[0] * m2[pp]);
                o.y = rs[pp + 1] * (fmaf(e[1], wc, -m1[pp + 1]) - d[1] * m2[pp + 1]);
                o.z = rs[pp + 2] * (fmaf(e[2], wc, -m1[pp + 2]) - d[2] * m2[pp + 2]);
                o.w = rs[pp + 3] * (fmaf(e[3], wc, -m1[pp + 3]) - d[3] * m2[pp + 3]);
                st4(db + (size_t)c * HW + pp, o);
            }
        }
    } else {
        const int ne = C << lp;
        for (int i = tid; i < ne; i += MODLN_THREADS) {
            const int c = i >> lp, pp = i - (c << lp);
            if (pp < npix) st(db + (size_t)c * HW + pp, rs[pp] * (fmaf(gs[c * S + pp], w[c], -m1[pp]) - xs[c * S + pp] * m2[pp]));
        }
    }
}

static hipError_t launch_modln_bwd(hipStream_t s, int N, int C, int HW, int x_dtype, const void* x, size_t xs_n, size_t xs_c, int mod_dtype,
                                   const void* mod, const float* w, const float* b, const float* mean, const float* rstd, const float* gout, void* dx,
                                   void* dmod, float* dw, float* db, void* scratch)
{
    const int lp = modln_bwd_log2(C), P = 1 << lp, tpi = (HW + P - 1) / P;
    const size_t lds = modln_lds_bytes(C, P, 2);
    const ModlnVec v = modln_vec(C, HW, x_dtype, x, xs_n, xs_c, mod_dtype, mod, w, b);
    const int vm = v.m && (!dmod || ptr_aligned(dmod, vec_grid_bytes(mod_dtype)));
    const int vg = v.hw && ptr_aligned(gout, 16);
    const int vd = v.hw && ptr_aligned(dx, vec_grid_bytes(x_dtype));
    float* part = (dw || db) ? (float*)align_ptr((const char*)scratch) : nullptr;
    const uint32_t T = (uint32_t)((size_t)N * tpi);
    const dim3 g(T), blk(MODLN_THREADS);
#define MODLN_BWD(TX, TM) hipLaunchKernelGGL((modln_bwd_kernel<TX, TM>), g, blk, lds, s, C, HW, lp, tpi, v.x, vm, vg, vd, (const TX*)x, xs_n, xs_c, \
                                             (const TM*)mod, w, b, mean, rstd, gout, (TX*)dx, (TM*)dmod, part)
    if (x_dtype == IGS_DTYPE_F16) { if (mod_dtype == IGS_DTYPE_F16) MODLN_BWD(_Float16, _Float16); else MODLN_BWD(_Float16, float); }
    else { if (mod_dtype == IGS_DTYPE_F16) MODLN_BWD(float, _Float16); else MODLN_BWD(float, float); }
#undef MODLN_BWD
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !part) return e;
    return launch_param_reduce(s, C, T, part, part + (size_t)T * 2 * C, dw, db);      // (staged behind the workgroups' rows)
}

// the entry points (the contract is in include/igs_rast.h)
extern "C" int igs_ray_condition_fwd(void* stream, int N, int H, int W, int Hd, int Wd, const float* rays, const float* depth, float* cond)
{
    const char* fn = "igs_ray_condition_fwd";
    if (N < 0 || N > IGS_COND_MAX_PIXELS) return fail_in(fn, "N out of range");
    if (H < 1 || H > IGS_COND_MAX_HW) return fail_in(fn, "H out of range (1..IGS_COND_MAX_HW)");
    if (W < 1 || W > IGS_COND_MAX_HW) return fail_in(fn, "W out of range (1..IGS_COND_MAX_HW)");
    if (Hd < 1 || Hd > IGS_COND_MAX_HW) return fail_in(fn, "Hd out of range (1..IGS_COND_MAX_HW)");
    if (Wd < 1 || Wd > IGS_COND_MAX_HW) return fail_in(fn, "Wd out of range (1..IGS_COND_MAX_HW)");
    if ((long long)N * H * W > IGS_COND_MAX_PIXELS) return fail_in(fn, "N * H * W out of range (IGS_COND_MAX_PIXELS)");
    if (N == 0) return 0;
    if (!rays || !depth || !cond) return fail_in(fn, "NULL pointer");
    HIP_TRY(launch_ray_condition((hipStream_t)stream, N, H, W, Hd, Wd, rays, depth, cond), "ray condition launch");
    return 0;
}
static const char* modln_size_error(int N, int C, int H, int W)
{
    if (N < 0 || N > IGS_COND_MAX_PIXELS) return "N out of range";
    if (C < 1 || C > IGS_MODLN_MAX_C) return "C out of range (1..IGS_MODLN_MAX_C)";
    if (H < 1 || H > IGS_COND_MAX_HW) return "H out of range (1..IGS_COND_MAX_HW)";
    if (W < 1 || W > IGS_COND_MAX_HW) return "W out of range (1..IGS_COND_MAX_HW)";
    if ((long long)N * H * W > IGS_COND_MAX_PIXELS) return "N * H * W out of range (IGS_COND_MAX_PIXELS)";
    return nullptr;
}
extern "C" size_t igs_modln_bwd_scratch_bytes(int N, int C, int H, int W)
{
    if (modln_size_error(N, C, H, W)) return 0;
    return modln_bwd_scratch_bytes(N, C, H * W) + 256;
}
extern "C" int igs_modln_fwd(void* stream, int N, int C, int H, int W, int x_dtype, const void* x, long long xs_n, long long xs_c, long long xs_h,
                             long long xs_w, int mod_dtype, const void* mod, const float* weight, const float* bias, float eps, float* out,
                             float* mean, float* rstd)
{
    const char* fn = "igs_modln_fwd";
    if (const char* w = modln_size_error(N, C, H, W)) return fail_in(fn, w);
    if (!dtype_ok(x_dtype) || !dtype_ok(mod_dtype)) return fail_in(fn, "unknown dtype code");
    if (const char* w = plane_stride_error(C, H, W, xs_n, xs_c, xs_h, xs_w)) return fail_in(fn, w);
    if (!(eps >= 0.f)) return fail_in(fn, "eps must be >= 0");
    if ((mean == nullptr) != (rstd == nullptr)) return fail_in(fn, "mean and rstd go together (both or neither)");
    if (N == 0) return 0;
    if (!x || !mod || !weight || !bias || !out) return fail_in(fn, "NULL pointer");
    HIP_TRY(launch_modln_fwd((hipStream_t)stream, N, C, H * W, x_dtype, x, (size_t)xs_n, (size_t)xs_c, mod_dtype, mod, weight, bias, eps, out, mean,
                             rstd), "modln fwd launch");
    return 0;
}
extern "C" int igs_modln_bwd(void* stream, int N, int C, int H, int W, int x_dtype, const void* x, long long xs_n, long long xs_c, long long xs_h,
                             long long xs_w, int mod_dtype, const void* mod, const float* weight, const float* bias, const float* mean,
                             const float* rstd, const float* gout, void* dx, void* dmod, float* dweight, float* dbias, void* scratch)
{
    const char* fn = "igs_modln_bwd";
    if (const char* w = modln_size_error(N, C, H, W)) return fail_in(fn, w);
    if (!dtype_ok(x_dtype) || !dtype_ok(mod_dtype)) return fail_in(fn, "unknown dtype code");
    if (const char* w = plane_stride_error(C, H, W, xs_n, xs_c, xs_h, xs_w)) return fail_in(fn, w);
    if (N == 0 || (!dx && !dmod && !dweight && !dbias)) return 0;
    if (!x || !mod || !weight || !bias || !mean || !rstd || !gout) return fail_in(fn, "NULL pointer");
    if ((dweight || dbias) && !scratch) return fail_in(fn, "NULL pointer (scratch is required for d weight / d bias)");
    HIP_TRY(launch_modln_bwd((hipStream_t)stream, N, C, H * W, x_dtype, x, (size_t)xs_n, (size_t)xs_c, mod_dtype, mod, weight, bias, mean, rstd, gout,
                             dx, dmod, dweight, dbias, scratch), "modln bwd launch");
    return 0;
}
