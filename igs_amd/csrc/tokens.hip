// tokens.hip -- the per-token work of AGM-Net's two transformers for gfx950, up to their GEMMs: the LayerNorms of BasicTransformerBlock
// (igs/models/transformers.py:304-365: norm1, norm3 over dim 512) and of the unimatch TransformerLayer (igs/models/unimatch/transformer.py:
// 140-146: norm1 / norm2 over 128 channels, with the `source + message` add behind them), and the GEGLU of the block's feed-forward
// (transformers.py:503-506).  Forward and backward.  include/igs_rast.h states the contract, DESIGN.md section 19 the lane mapping, the
// byte budgets and the figures.
//
//   (1) ln_fwd_kernel / ln_bwd_kernel: a row of C elements belongs to LPR = 16 or 64 neighbouring lanes of one wave, lane l holding the
//       four-element groups l, l + LPR, ... (NV of them) in registers between the statistics and the write: the row is read once.  C <= 64
//       and <= 128 take 16 lanes (four rows per wave; the unimatch width), C <= 256 / 512 / 1024 a whole wave with 1 / 2 / 4
//       groups per lane (512: the anchor transformer).  Every reduction is a butterfly over the row's lanes whose two operands commute:
//       the same bits in every lane, no LDS, no barrier.  Statistics, all float32: m = sum / C, then from the CENTRED registers d = v - m
//       the sums s1 = sum d and s2 = sum d d; mean = m + s1 / C and var = s2 / C - (s1 / C)^2 (inorm.hip's corrected two-pass form: s1 / C
//       is the rounding error of m, so a constant row gives d = s1 / C exactly, and so exactly `bias`).  A row that holds a NaN or an
//       infinity comes out all NaN.  The backward recomputes the statistics from the row it has to read anyway; per workgroup the lanes
//       keep the column sums of dout x_hat and dout over the rows they meet, the workgroup's row groups are added through LDS in a fixed
//       order into one partial row of the caller's scratch, and param_reduce.h adds the partial rows in workgroup order (one round).
//       Four-element loads where every base pointer, every row stride and C allow them (VEC), scalar loads of the same lane mapping
//       otherwise.  The three dtypes of a call are wave-uniform runtime codes: one kernel per (LPR, NV, VEC).
//   (2) geglu_fwd_kernel / geglu_bwd_kernel: elementwise over [N, D], four columns per thread where D, the stride and the pointers allow.
//       Exact GELU: g Phi(g) with Phi(g) = 0.5 (1 + erf(g / sqrt 2)); the backward writes both halves of d p in one launch.
#include "common.h"
#include "elem_common.h"
#include "host_api.h"
#include "param_reduce.h"

#define LN_THREADS 256
#define LN_BWD_MAX_GROUPS 1024                                 // workgroups (= partial parameter rows) of one backward
#define GEGLU_THREADS 256

// ---------------------------------------------------------------------------------------------------------------------------------
// (1) LayerNorm
// ---------------------------------------------------------------------------------------------------------------------------------
// The registers of one lane of a row: group j holds columns 4 (j LPR + l) .. + 3; slots outside the row hold zero.
template <int LPR, int NV, bool VEC>
struct LnRow {
    float v[NV][4];
    static __device__ __forceinline__ int col(int j, int l) { return 4 * (j * LPR + l); }
    __device__ __forceinline__ void load(TokPtr t, size_t base, int C, int l)
    {
#pragma unroll
        for (int j = 0; j < NV; j++) {
            const int c = col(j, l);
            if (VEC) {
                float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
                if (c < C) q = ld4(t, base + c);
                v[j][0] = q.x; v[j][1] = q.y; v[j][2] = q.z; v[j][3] = q.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++) v[j][k] = c + k < C ? ld(t, base + c + k) : 0.f;
            }
        }
    }
    // [C] float32 parameters; NULL gives `fill`
    __device__ __forceinline__ void load_param(const float* p, float fill, int C, int l)
    {
#pragma unroll
        for (int j = 0; j < NV; j++) {
            const int c = col(j, l);
            if (VEC) {
                float4 q = make_float4(fill, fill, fill, fill);
                if (p && c < C) q = *(const float4*)(p + c);
                v[j][0] = q.x; v[j][1] = q.y; v[j][2] = q.z; v[j][3] = q.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++) v[j][k] = (p && c + k < C) ? p[c + k] : fill;
            }
        }
    }
    __device__ __forceinline__ void store(TokPtr t, size_t base, int C, int l) const
    {
#pragma unroll
        for (int j = 0; j < NV; j++) {
            const int c = col(j, l);
            if (VEC) {
                if (c < C) st4(t, base + c, make_float4(v[j][0], v[j][1], v[j][2], v[j][3]));
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (c + k < C) st(t, base + c + k, v[j][k]);
            }
        }
    }
};

// r.v <- x_hat = (v - mean) * rstd (zero outside the row); returns rstd
template <int LPR, int NV, bool VEC>
__device__ __forceinline__ float ln_normalise(LnRow<LPR, NV, VEC>& r, int C, int l, float eps)
{
    const float n = (float)C;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NV; j++)
#pragma unroll
        for (int k = 0; k < 4; k++) s[k] += r.v[j][k];                  // (the slots outside the row hold zero)
    const float m = lane_sum<LPR>((s[0] + s[1]) + (s[2] + s[3])) / n;
    float a[4] = {0.f, 0.f, 0.f, 0.f}, b[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NV; j++)
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float d = r.col(j, l) + k < C ? r.v[j][k] - m : 0.f;
            a[k] += d; b[k] = fmaf(d, d, b[k]);
        }
    float c[2] = {(a[0] + a[1]) + (a[2] + a[3]), (b[0] + b[1]) + (b[2] + b[3])};
    lane_sum<LPR>(c);
    float mean, rstd;
    norm_finish(m, c[0], c[1], n, eps, mean, rstd);
#pragma unroll
    for (int j = 0; j < NV; j++)
#pragma unroll
        for (int k = 0; k < 4; k++) r.v[j][k] = r.col(j, l) + k < C ? (r.v[j][k] - mean) * rstd : 0.f;
    return rstd;
}

// out and res are NOT __restrict__: out == res is part of the contract (every lane reads its own elements before it writes them)
template <int LPR, int NV, bool VEC>
__global__ void __launch_bounds__(LN_THREADS)
ln_fwd_kernel(uint32_t N, int C, TokPtr x, size_t xs, TokPtr res, size_t rs, const float* __restrict__ w, const float* __restrict__ b, float eps,
              TokPtr out, size_t os)
{
    constexpr int RPB = LN_THREADS / LPR;
    const int l = threadIdx.x % LPR;
    const uint32_t row = blockIdx.x * RPB + threadIdx.x / LPR;
    if (row >= N) return;                                              // (the whole row group: its lanes shuffle among themselves only)
    LnRow<LPR, NV, VEC> r, q;
    r.load(x, (size_t)row * xs, C, l);
    ln_normalise(r, C, l, eps);
    if (w) {
        LnRow<LPR, NV, VEC> pw;
        pw.load_param(w, 1.f, C, l);
        q.load_param(b, 0.f, C, l);
#pragma unroll
        for (int j = 0; j < NV; j++)
#pragma unroll
            for (int k = 0; k < 4; k++) r.v[j][k] = fmaf(r.v[j][k], pw.v[j][k], q.v[j][k]);
    }
    if (res.p) {
        q.load(res, (size_t)row * rs, C, l);
#pragma unroll
        for (int j = 0; j < NV; j++)
#pragma unroll
            for (int k = 0; k < 4; k++) r.v[j][k] += q.v[j][k];
    }
    r.store(out, (size_t)row * os, C, l);
}

// With xh = (x - mean) rstd and gw = dout w:  d x = rstd (gw - mean_c(gw) - xh mean_c(gw xh)),  d weight = sum_n dout xh,  d bias = sum_n dout.
// Workgroup b takes the row groups b, b + gridDim.x, ...; part[(b * 2 + 0) * C + c] / [(b * 2 + 1) * C + c]: its sums over those rows.
template <int LPR, int NV, bool VEC>
__global__ void __launch_bounds__(LN_THREADS)
ln_bwd_kernel(uint32_t N, int C, TokPtr x, size_t xs, const float* __restrict__ w, float eps, TokPtr g, size_t gs, TokPtr dx, size_t dxs,
              float* __restrict__ part)
{
    constexpr int RPB = LN_THREADS / LPR;
    __shared__ float red[8 * LN_THREADS];
    const int l = threadIdx.x % LPR, sub = threadIdx.x / LPR;
    const uint32_t groups = (N + RPB - 1) / RPB;
    const float n = (float)C;
    LnRow<LPR, NV, VEC> pw, aw, ab;
    pw.load_param(w, 1.f, C, l);
    aw.load_param(nullptr, 0.f, C, l);
    ab.load_param(nullptr, 0.f, C, l);
    for (uint32_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const uint32_t row = grp * RPB + sub;
        if (row >= N) continue;                                        // (the whole row group)
        LnRow<LPR, NV, VEC> r, q;
        r.load(x, (size_t)row * xs, C, l);
        q.load(g, (size_t)row * gs, C, l);
        const float rstd = ln_normalise(r, C, l, eps);
        float a[4] = {0.f, 0.f, 0.f, 0.f}, b[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < NV; j++)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (part) { aw.v[j][k] = fmaf(q.v[j][k], r.v[j][k], aw.v[j][k]); ab.v[j][k] += q.v[j][k]; }
                const float gw = q.v[j][k] * pw.v[j][k];               // (zero outside the row: dout's slots hold zero)
                q.v[j][k] = gw;
                a[k] += gw; b[k] = fmaf(gw, r.v[j][k], b[k]);
            }
        if (!dx.p) continue;                                           // (uniform)
        float c[2] = {(a[0] + a[1]) + (a[2] + a[3]), (b[0] + b[1]) + (b[2] + b[3])};
        lane_sum<LPR>(c);
        const float m1 = c[0] / n, m2 = c[1] / n;
#pragma unroll
        for (int j = 0; j < NV; j++)
#pragma unroll
            for (int k = 0; k < 4; k++) r.v[j][k] = rstd * ((q.v[j][k] - m1) - r.v[j][k] * m2);
        r.store(dx, (size_t)row * dxs, C, l);
    }
    if (!part) return;                                                 // (uniform)
    // the workgroup's RPB row groups, added in group order by the lanes of group 0; one round of 8 values per lane and register group
    float* pd = part + (size_t)blockIdx.x * 2 * C;
#pragma unroll
    for (int j = 0; j < NV; j++) {
#pragma unroll
        for (int k = 0; k < 4; k++) { red[k * LN_THREADS + threadIdx.x] = aw.v[j][k]; red[(4 + k) * LN_THREADS + threadIdx.x] = ab.v[j][k]; }
        wg_barrier();
        if (sub == 0) {
            float t[8];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                float s = 0.f;
#pragma unroll
                for (int i = 0; i < RPB; i++) s += red[k * LN_THREADS + i * LPR + l];
                t[k] = s;
            }
            const int c = aw.col(j, l);
            if (VEC) {
                if (c < C) { *(float4*)(pd + c) = make_float4(t[0], t[1], t[2], t[3]); *(float4*)(pd + C + c) = make_float4(t[4], t[5], t[6], t[7]); }
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (c + k < C) { pd[c + k] = t[k]; pd[C + c + k] = t[4 + k]; }
            }
        }
        wg_barrier();
    }
}

// rows per workgroup of the shape that takes C
static int ln_rows_per_group(int C) { return C <= 128 ? LN_THREADS / 16 : LN_THREADS / 64; }
static uint32_t ln_bwd_groups(long long N, int C)
{
    const long long rpb = ln_rows_per_group(C), groups = (N + rpb - 1) / rpb;
    return (uint32_t)(groups < LN_BWD_MAX_GROUPS ? groups : LN_BWD_MAX_GROUPS);
}
// the four-element path of an operand: base on the 4-element grid of its dtype, row stride a multiple of four
static bool ln_vec_ok(const void* p, int dtype, long long stride) { return !p || (ptr_aligned(p, vec_grid_bytes(dtype)) && (stride & 3) == 0); }

#define LN_LAUNCH(KERNEL, GRID, ...)                                                                                                        \
    do {                                                                                                                                    \
        const dim3 g_(GRID), b_(LN_THREADS);                                                                                                \
        if (vec) {                                                                                                                          \
            if (C <= 64) hipLaunchKernelGGL((KERNEL<16, 1, true>), g_, b_, 0, s, __VA_ARGS__);                                              \
            else if (C <= 128) hipLaunchKernelGGL((KERNEL<16, 2, true>), g_, b_, 0, s, __VA_ARGS__);                                        \
            else if (C <= 256) hipLaunchKernelGGL((KERNEL<64, 1, true>), g_, b_, 0, s, __VA_ARGS__);                                        \
            else if (C <= 512) hipLaunchKernelGGL((KERNEL<64, 2, true>), g_, b_, 0, s, __VA_ARGS__);                                        \
            else hipLaunchKernelGGL((KERNEL<64, 4, true>), g_, b_, 0, s, __VA_ARGS__);                                                      \
        } else {                                                                                                                            \
            if (C <= 64) hipLaunchKernelGGL((KERNEL<16, 1, false>), g_, b_, 0, s, __VA_ARGS__);                                             \
            else if (C <= 128) hipLaunchKernelGGL((KERNEL<16, 2, false>), g_, b_, 0, s, __VA_ARGS__);                                       \
            else if (C <= 256) hipLaunchKernelGGL((KERNEL<64, 1, false>), g_, b_, 0, s, __VA_ARGS__);                                       \
            else if (C <= 512) hipLaunchKernelGGL((KERNEL<64, 2, false>), g_, b_, 0, s, __VA_ARGS__);                                       \
            else hipLaunchKernelGGL((KERNEL<64, 4, false>), g_, b_, 0, s, __VA_ARGS__);                                                     \
        }                                                                                                                                   \
    } while (0)

static hipError_t launch_ln_fwd(hipStream_t s, long long N, int C, int x_dtype, const void* x, long long xs, int res_dtype, const void* res,
                                long long rs, const float* w, const float* b, float eps, int out_dtype, void* out, long long os)
{
    const bool vec = (C & 3) == 0 && ln_vec_ok(x, x_dtype, xs) && ln_vec_ok(res, res_dtype, rs) && ln_vec_ok(out, out_dtype, os) &&
                     (!w || (ptr_aligned(w, 16) && ptr_aligned(b, 16)));
    const TokPtr tx = {x, x_dtype == IGS_DTYPE_F16}, tr = {res, res && res_dtype == IGS_DTYPE_F16}, to = {out, out_dtype == IGS_DTYPE_F16};
    const long long rpb = ln_rows_per_group(C);
    LN_LAUNCH(ln_fwd_kernel, (unsigned)((N + rpb - 1) / rpb), (uint32_t)N, C, tx, (size_t)xs, tr, (size_t)rs, w, b, eps, to, (size_t)os);
    return hipGetLastError();
}

static hipError_t launch_ln_bwd(hipStream_t s, long long N, int C, int x_dtype, const void* x, long long xs, const float* w, float eps, int g_dtype,
                                const void* dout, long long gs, int dx_dtype, void* dx, long long dxs, float* dw, float* db, void* scratch)
{
    const bool vec = (C & 3) == 0 && ln_vec_ok(x, x_dtype, xs) && ln_vec_ok(dout, g_dtype, gs) && ln_vec_ok(dx, dx_dtype, dxs) &&
                     (!w || ptr_aligned(w, 16));
    const TokPtr tx = {x, x_dtype == IGS_DTYPE_F16}, tg = {dout, g_dtype == IGS_DTYPE_F16}, td = {dx, dx && dx_dtype == IGS_DTYPE_F16};
    float* part = (dw || db) ? (float*)align_ptr((const char*)scratch) : nullptr;
    const uint32_t T = ln_bwd_groups(N, C);
    LN_LAUNCH(ln_bwd_kernel, T, (uint32_t)N, C, tx, (size_t)xs, w, eps, tg, (size_t)gs, td, (size_t)dxs, part);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !part) return e;
    return launch_param_reduce(s, C, T, part, nullptr, dw, db);      // (T <= LN_BWD_MAX_GROUPS: no wave walks more than 64 rows)
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (2) GEGLU
// ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float geglu_pdf(float g) { return 0.3989422804014327f * expf(-0.5f * g * g); }

// thread i takes the V columns (i mod dv) V .. of row i / dv, dv = D / V
template <typename T, int V>
__global__ void __launch_bounds__(GEGLU_THREADS)
geglu_fwd_kernel(uint32_t total, uint32_t dv, int D, const T* __restrict__ p, size_t ps, T* __restrict__ out)
{
    const uint32_t i = blockIdx.x * GEGLU_THREADS + threadIdx.x;
    if (i >= total) return;
    const uint32_t n = i / dv, d = (i - n * dv) * V;
    const T* row = p + (size_t)n * ps + d;
    T* o = out + (size_t)n * D + d;
    if (V == 4) {
        const float4 h = ld4(row), g = ld4(row + D);
        st4(o, make_float4(h.x * (g.x * gelu_cdf(g.x)), h.y * (g.y * gelu_cdf(g.y)), h.z * (g.z * gelu_cdf(g.z)), h.w * (g.w * gelu_cdf(g.w))));
    } else {
        const float h = ld(row), g = ld(row + D);
        st(o, h * (g * gelu_cdf(g)));
    }
}

// d h = dout gelu(g), d g = dout h (Phi(g) + g phi(g))
__device__ __forceinline__ void geglu_grad(float h, float g, float u, float& dh, float& dg)
{
    const float cdf = gelu_cdf(g);
    dh = u * (g * cdf);
    dg = (u * h) * fmaf(g, geglu_pdf(g), cdf);
}

template <typename T, int V>
__global__ void __launch_bounds__(GEGLU_THREADS)
geglu_bwd_kernel(uint32_t total, uint32_t dv, int D, const T* __restrict__ p, size_t ps, const T* __restrict__ dout, T* __restrict__ dp)
{
    const uint32_t i = blockIdx.x * GEGLU_THREADS + threadIdx.x;
    if (i >= total) return;
    const uint32_t n = i / dv, d = (i - n * dv) * V;
    const T* row = p + (size_t)n * ps + d;
    const T* u = dout + (size_t)n * D + d;
    T* o = dp + (size_t)n * 2 * D + d;
    if (V == 4) {
        const float4 h = ld4(row), g = ld4(row + D), uu = ld4(u);
        float4 dh, dg;
        geglu_grad(h.x, g.x, uu.x, dh.x, dg.x);
        geglu_grad(h.y, g.y, uu.y, dh.y, dg.y);
        geglu_grad(h.z, g.z, uu.z, dh.z, dg.z);
        geglu_grad(h.w, g.w, uu.w, dh.w, dg.w);
        st4(o, dh);
        st4(o + D, dg);
    } else {
        float dh, dg;
        geglu_grad(ld(row), ld(row + D), ld(u), dh, dg);
        st(o, dh);
        st(o + D, dg);
    }
}

template <typename T>
static hipError_t launch_geglu(hipStream_t s, long long N, int D, const T* p, long long ps, const T* dout, T* dst)
{
    const size_t grid = 4 * sizeof(T);
    const bool v4 = (D & 3) == 0 && (ps & 3) == 0 && ptr_aligned(p, grid) && ptr_aligned(dst, grid) && (!dout || ptr_aligned(dout, grid));
    const uint32_t dv = (uint32_t)(v4 ? D / 4 : D), total = (uint32_t)N * dv;
    const dim3 g((total + GEGLU_THREADS - 1) / GEGLU_THREADS), blk(GEGLU_THREADS);
    if (dout) {
        if (v4) hipLaunchKernelGGL((geglu_bwd_kernel<T, 4>), g, blk, 0, s, total, dv, D, p, (size_t)ps, dout, dst);
        else hipLaunchKernelGGL((geglu_bwd_kernel<T, 1>), g, blk, 0, s, total, dv, D, p, (size_t)ps, dout, dst);
    } else {
        if (v4) hipLaunchKernelGGL((geglu_fwd_kernel<T, 4>), g, blk, 0, s, total, dv, D, p, (size_t)ps, dst);
        else hipLaunchKernelGGL((geglu_fwd_kernel<T, 1>), g, blk, 0, s, total, dv, D, p, (size_t)ps, dst);
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the entry points (the contract is in include/igs_rast.h)
// ---------------------------------------------------------------------------------------------------------------------------------
// the bytes [lo, hi) that N rows of `len` elements at a row stride of `stride` elements span
static ByteSpan tok_span(const void* p, long long N, long long len, long long stride, int dtype)
{
    return byte_span(p, ((size_t)(N - 1) * (size_t)stride + (size_t)len) * dtype_bytes(dtype));
}
static bool tok_misaligned(const void* p, int dtype) { return !ptr_aligned(p, dtype_bytes(dtype)); }

static const char* ln_size_error(long long N, int C)
{
    if (C < 1 || C > IGS_LN_MAX_C) return "C out of range (1..IGS_LN_MAX_C)";
    if (N < 0 || N > IGS_LN_MAX_ROWS) return "N out of range (0..IGS_LN_MAX_ROWS)";
    return nullptr;
}
static bool tok_stride_bad(long long stride, long long len) { return stride < len || stride > IGS_TOKENS_MAX_STRIDE; }

extern "C" int igs_layer_norm_fwd(void* stream, long long N, int C, int x_dtype, const void* x, long long xs, int res_dtype, const void* res,
                                  long long rs, const float* weight, const float* bias, float eps, int out_dtype, void* out, long long os)
{
    const char* fn = "igs_layer_norm_fwd";
    if (!dtype_ok(x_dtype) || !dtype_ok(out_dtype) || (res && !dtype_ok(res_dtype))) return fail_in(fn, "unknown dtype code");
    if (const char* w = ln_size_error(N, C)) return fail_in(fn, w);
    if (tok_stride_bad(xs, C) || tok_stride_bad(os, C) || (res && tok_stride_bad(rs, C)))
        return fail_in(fn, "a row stride is below the row length C or above IGS_TOKENS_MAX_STRIDE");
    if (!eps_ok(eps)) return fail_in(fn, "eps must be finite and >= 0");
    if ((weight == nullptr) != (bias == nullptr)) return fail_in(fn, "weight and bias go together (both or neither)");
    if (N == 0) return 0;
    if (!x || !out) return fail_in(fn, "NULL pointer");
    if (tok_misaligned(x, x_dtype) || tok_misaligned(out, out_dtype) || (res && tok_misaligned(res, res_dtype)) || !ptr_aligned(weight, 4) ||
        !ptr_aligned(bias, 4))
        return fail_in(fn, "a pointer is not aligned to its element size");
    const ByteSpan sx = tok_span(x, N, C, xs, x_dtype), so = tok_span(out, N, C, os, out_dtype);
    if (spans_overlap(sx, so)) return fail_in(fn, "out overlaps x (only out == res may alias)");
    if (res && spans_overlap(tok_span(res, N, C, rs, res_dtype), so) && !(res == (const void*)out && rs == os && res_dtype == out_dtype))
        return fail_in(fn, "out overlaps res without being res (only out == res with one dtype and one row stride may alias)");
    if (weight) {
        const ByteSpan sw = tok_span(weight, 1, C, C, IGS_DTYPE_F32), sb = tok_span(bias, 1, C, C, IGS_DTYPE_F32);
        if (spans_overlap(sw, so) || spans_overlap(sb, so)) return fail_in(fn, "out overlaps weight or bias");
    }
    HIP_TRY(launch_ln_fwd((hipStream_t)stream, N, C, x_dtype, x, xs, res_dtype, res, rs, weight, bias, eps, out_dtype, out, os), "layer norm fwd launch");
    return 0;
}

extern "C" size_t igs_layer_norm_bwd_scratch_bytes(long long N, int C)
{
    if (ln_size_error(N, C)) return 0;
    return align_up((size_t)ln_bwd_groups(N, C) * 2 * C * 4, 256) + 256;
}

extern "C" int igs_layer_norm_bwd(void* stream, long long N, int C, int x_dtype, const void* x, long long xs, const float* weight, float eps,
                                  int dout_dtype, const void* dout, long long gs, int dx_dtype, void* dx, long long dxs, float* dweight, float* dbias,
                                  void* scratch)
{
    const char* fn = "igs_layer_norm_bwd";
    if (!dtype_ok(x_dtype) || !dtype_ok(dout_dtype) || (dx && !dtype_ok(dx_dtype))) return fail_in(fn, "unknown dtype code");
    if (const char* w = ln_size_error(N, C)) return fail_in(fn, w);
    if (tok_stride_bad(xs, C) || tok_stride_bad(gs, C) || (dx && tok_stride_bad(dxs, C)))
        return fail_in(fn, "a row stride is below the row length C or above IGS_TOKENS_MAX_STRIDE");
    if (!eps_ok(eps)) return fail_in(fn, "eps must be finite and >= 0");
    if (N == 0 || (!dx && !dweight && !dbias)) return 0;
    if (!x || !dout) return fail_in(fn, "NULL pointer");
    if ((dweight || dbias) && !scratch) return fail_in(fn, "NULL pointer (scratch is required for d weight / d bias)");
    if (tok_misaligned(x, x_dtype) || tok_misaligned(dout, dout_dtype) || (dx && tok_misaligned(dx, dx_dtype)) || !ptr_aligned(weight, 4) ||
        !ptr_aligned(dweight, 4) || !ptr_aligned(dbias, 4))
        return fail_in(fn, "a pointer is not aligned to its element size");
    const ByteSpan sx = tok_span(x, N, C, xs, x_dtype), sg = tok_span(dout, N, C, gs, dout_dtype);
    const ByteSpan outs[4] = {dx ? tok_span(dx, N, C, dxs, dx_dtype) : ByteSpan{0, 0}, dweight ? tok_span(dweight, 1, C, C, IGS_DTYPE_F32) : ByteSpan{0, 0},
                              dbias ? tok_span(dbias, 1, C, C, IGS_DTYPE_F32) : ByteSpan{0, 0},
                              (dweight || dbias) ? byte_span(scratch, igs_layer_norm_bwd_scratch_bytes(N, C)) : ByteSpan{0, 0}};
    for (int i = 0; i < 4; i++) {
        if (spans_overlap(outs[i], sx) || spans_overlap(outs[i], sg) || (weight && spans_overlap(outs[i], tok_span(weight, 1, C, C, IGS_DTYPE_F32))))
            return fail_in(fn, "an output overlaps x, dout or weight");
        for (int k = i + 1; k < 4; k++)
            if (spans_overlap(outs[i], outs[k])) return fail_in(fn, "the outputs (dx, dweight, dbias, scratch) overlap one another");
    }
    HIP_TRY(launch_ln_bwd((hipStream_t)stream, N, C, x_dtype, x, xs, weight, eps, dout_dtype, dout, gs, dx_dtype, dx, dxs, dweight, dbias, scratch),
            "layer norm bwd launch");
    return 0;
}

static const char* geglu_size_error(long long N, int D, long long ps)
{
    if (D < 1 || D > IGS_GEGLU_MAX_D) return "D out of range (1..IGS_GEGLU_MAX_D)";
    if (N < 0 || N > IGS_GEGLU_MAX_ELEMS / D) return "N out of range (N >= 0, N * D <= IGS_GEGLU_MAX_ELEMS)";
    if (tok_stride_bad(ps, 2LL * D)) return "the row stride is below the row length 2 D or above IGS_TOKENS_MAX_STRIDE";
    return nullptr;
}

extern "C" int igs_geglu_fwd(void* stream, long long N, int D, int dtype, const void* p, long long ps, void* out)
{
    const char* fn = "igs_geglu_fwd";
    if (!dtype_ok(dtype)) return fail_in(fn, "unknown dtype code");
    if (const char* w = geglu_size_error(N, D, ps)) return fail_in(fn, w);
    if (N == 0) return 0;
    if (!p || !out) return fail_in(fn, "NULL pointer");
    if (tok_misaligned(p, dtype) || tok_misaligned(out, dtype)) return fail_in(fn, "a pointer is not aligned to its element size");
    if (spans_overlap(tok_span(p, N, 2LL * D, ps, dtype), tok_span(out, N, D, D, dtype))) return fail_in(fn, "out overlaps p");
    hipError_t e;
    if (dtype == IGS_DTYPE_F16) e = launch_geglu((hipStream_t)stream, N, D, (const _Float16*)p, ps, (const _Float16*)nullptr, (_Float16*)out);
    else e = launch_geglu((hipStream_t)stream, N, D, (const float*)p, ps, (const float*)nullptr, (float*)out);
    HIP_TRY(e, "geglu fwd launch");
    return 0;
}

extern "C" int igs_geglu_bwd(void* stream, long long N, int D, int dtype, const void* p, long long ps, const void* dout, void* dp)
{
    const char* fn = "igs_geglu_bwd";
    if (!dtype_ok(dtype)) return fail_in(fn, "unknown dtype code");
    if (const char* w = geglu_size_error(N, D, ps)) return fail_in(fn, w);
    if (N == 0) return 0;
    if (!p || !dout || !dp) return fail_in(fn, "NULL pointer");
    if (tok_misaligned(p, dtype) || tok_misaligned(dout, dtype) || tok_misaligned(dp, dtype)) return fail_in(fn, "a pointer is not aligned to its element size");
    const ByteSpan sd = tok_span(dp, N, 2LL * D, 2LL * D, dtype);
    if (spans_overlap(tok_span(p, N, 2LL * D, ps, dtype), sd) || spans_overlap(tok_span(dout, N, D, D, dtype), sd)) return fail_in(fn, "dp overlaps p or dout");
    hipError_t e;
    if (dtype == IGS_DTYPE_F16) e = launch_geglu((hipStream_t)stream, N, D, (const _Float16*)p, ps, (const _Float16*)dout, (_Float16*)dp);
    else e = launch_geglu((hipStream_t)stream, N, D, (const float*)p, ps, (const float*)dout, (float*)dp);
    HIP_TRY(e, "geglu bwd launch");
    return 0;
}
