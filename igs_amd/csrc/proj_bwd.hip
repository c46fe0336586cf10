// proj_bwd.hip -- the backward of proj.hip's fused projections ("The backward").  Per row t of x and output j, g_j[t] is the
// upstream gradient of what the forward wrote for input row t: row (t + rot[j]) mod T of output j's gradient.
//
//   d x[t] = sum_j W_j^T g_j[t]            (j ascending, one accumulator chain)
//   d W_j  = sum_t g_j[t] (x) x[t]         (t ascending)
//
//   token_proj_bwd_dx_kernel      the forward's loop with the roles turned: a wave owns 32 rows, loads the rolled gradient row of output j
//                                 as the B operand, multiplies by the transposed matrix j (pack_projections of W_j^T, staged and streamed
//                                 through LDS exactly as the forward stages its pack) and keeps accumulating into the same four output
//                                 tiles across j; one store of d x per row.  Outputs without a gradient are skipped.
//   token_proj_bwd_wgrad_kernel   mlp_bwd_wgrad_kernel's scheme: a wave owns (row slice, output j, input tile, the four output tiles),
//                                 reads x and g_j from the caller's tensors through their strides and the roll, and writes its float32
//                                 partial into the scratch.
//   token_proj_bwd_reduce_kernel  adds the slices' partials in slice order.
// No float atomics; the order of every sum depends on T, n and rot only.
#include "proj_common.h"

#define PB_WG_WAVES 4
#define PB_WG_THREADS (64 * PB_WG_WAVES)
#define PB_MIN_SLICE_ROWS 512
#define PB_DW (128 * 128)                                                        // elements of one weight gradient
static_assert(PB_MIN_SLICE_ROWS % FFN_TRIP_ROWS == 0, "a slice is whole trips");

struct ProjBwdDxArgs {
    long long T;
    int na;                                // the outputs that have a gradient, ascending
    TokPtr g[IGS_TOKEN_PROJ_MAX_OUT], dx;
    long long gs[IGS_TOKEN_PROJ_MAX_OUT], dxs;
    int g_vec[IGS_TOKEN_PROJ_MAX_OUT], dx_vec;
    int mat[IGS_TOKEN_PROJ_MAX_OUT];       // which matrix of the pack
    long long rot[IGS_TOKEN_PROJ_MAX_OUT];
    const void* wt;                        // the transposed pack: n matrices of 16 tiles
};

template <typename T>
__global__ __launch_bounds__(FFN_THREADS, (ProjCfg<T>::WAVES_PER_SIMD)) void token_proj_bwd_dx_kernel(const ProjBwdDxArgs a)
{
    typedef ProjCfg<T> Cfg;
    __shared__ __attribute__((aligned(16))) T wl[2 * PROJ_MAT];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const T* wg = (const T*)a.wt;
    const bool stream = a.na > 2;                                                // (uniform)
    const long long trips = (a.T + FFN_TRIP_ROWS - 1) / FFN_TRIP_ROWS;
    // the matrices this workgroup walks, over all its trips: s = 0 .. stages - 1 is active matrix s % na in buffer s & 1
    const long long stages = (trips - blockIdx.x + gridDim.x - 1) / gridDim.x * a.na;

    if (stream) {
        ffn_stage(wl, wg + (size_t)a.mat[0] * PROJ_MAT, PROJ_MAT);
    } else {
        for (int j = 0; j < a.na; j++) ffn_stage(wl + j * PROJ_MAT, wg + (size_t)a.mat[j] * PROJ_MAT, PROJ_MAT);
    }
    wg_barrier();

    long long s = 0;
    for (long long trip = blockIdx.x; trip < trips; trip += gridDim.x) {         // (uniform over the workgroup: every wave takes every trip)
        const long long row = trip * FFN_TRIP_ROWS + wave * 32 + r;
        const bool live = row < a.T;
        attn_acc o[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
#pragma unroll
            for (int i = 0; i < 16; i++) o[t][i] = 0.f;
        }

        for (int j = 0; j < a.na; j++, s++) {
            long long grow = live ? row + a.rot[j] : 0;                          // a row past T reads row 0 and is never stored
            if (grow >= a.T) grow -= a.T;
            MlpIn<T> in;
            ffn_load_row(in, a.g[j], (size_t)grow * a.gs[j], a.g_vec[j], h);
            const T* buf = wl + (stream ? (int)(s & 1) : j) * PROJ_MAT;
            const bool more = stream && s + 1 < stages;
            const T* next = wg + (size_t)a.mat[j + 1 == a.na ? 0 : j + 1] * PROJ_MAT;
            T* other = wl + (int)((s + 1) & 1) * PROJ_MAT;
#pragma unroll
            for (int t = 0; t < 4; t++) {
                attn_f4 stg[Cfg::PIECES];
                if (more) {
#pragma unroll
                    for (int q = 0; q < Cfg::PIECES; q++) stg[q] = ((const attn_f4*)(next + t * Cfg::QUARTER))[q * FFN_THREADS + threadIdx.x];
                }
#pragma unroll
                for (int k = 0; k < 4; k++) o[t] = mlp_mm(buf + (t * 4 + k) * MLP_TILE, lane, in, k, o[t]);
                if (more) {
#pragma unroll
                    for (int q = 0; q < Cfg::PIECES; q++) ((attn_f4*)(other + t * Cfg::QUARTER))[q * FFN_THREADS + threadIdx.x] = stg[q];
                }
            }
            if (stream) wg_barrier();
        }
        if (live) {
            float4 f[16];
#pragma unroll
            for (int t = 0; t < 4; t++) {
#pragma unroll
                for (int g = 0; g < 4; g++) f[4 * t + g] = make_float4(o[t][4 * g], o[t][4 * g + 1], o[t][4 * g + 2], o[t][4 * g + 3]);
            }
            ffn_write_groups(f, a.dx, (size_t)row * a.dxs, a.dx_vec, h);
        }
    }
}

struct ProjBwdWgradArgs {
    long long T, slice_rows;
    int nw, slices;                        // the outputs whose weight gradient is wanted and has a gradient to sum, ascending
    uint32_t pstride;                      // floats of one slice's partials
    TokPtr x, g[IGS_TOKEN_PROJ_MAX_OUT];
    long long xs, gs[IGS_TOKEN_PROJ_MAX_OUT], rot[IGS_TOKEN_PROJ_MAX_OUT];
    int out[IGS_TOKEN_PROJ_MAX_OUT];       // which output: its partial is at out[i] * PB_DW
    float* part;
};

template <typename T>
__global__ __launch_bounds__(PB_WG_THREADS) void token_proj_bwd_wgrad_kernel(const ProjBwdWgradArgs a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const long long u = (long long)blockIdx.x * PB_WG_WAVES + wave;
    const int per_slice = 4 * a.nw;
    if (u >= (long long)per_slice * a.slices) return;                            // (no barrier in this kernel)
    const int slice = (int)(u / per_slice), idx = (int)(u - (long long)slice * per_slice), i = idx >> 2, kt = idx & 3;
    const long long lr0 = slice * a.slice_rows, lr1 = min(lr0 + a.slice_rows, a.T);
    const TokPtr g = a.g[i];
    const long long gs = a.gs[i], rot = a.rot[i];
    float* pw = a.part + (size_t)slice * a.pstride + (size_t)a.out[i] * PB_DW;
    const int col = 32 * kt + r;

    attn_acc acc[4];
#pragma unroll
    for (int t = 0; t < 4; t++) {
#pragma unroll
        for (int e = 0; e < 16; e++) acc[t][e] = 0.f;
    }
    for (long long n0 = lr0; n0 < lr1; n0 += 16) {
        float bv[8], av[4][8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const long long n = n0 + mlp_wgrad_row<T>(j, h);
            const bool ok = n < lr1;
            long long gn = n + rot;
            if (gn >= a.T) gn -= a.T;
            bv[j] = ok ? ld(a.x, (size_t)n * a.xs + col) : 0.f;
#pragma unroll
            for (int t = 0; t < 4; t++) av[t][j] = ok ? ld(g, (size_t)gn * gs + 32 * t + r) : 0.f;
        }
#pragma unroll
        for (int t = 0; t < 4; t++) acc[t] = mlp_wgrad_mm(T(0), av[t], bv, acc[t]);
    }
#pragma unroll
    for (int t = 0; t < 4; t++) {
#pragma unroll
        for (int e = 0; e < 16; e++) pw[(size_t)(32 * t + attn_row(e, h)) * 128 + col] = acc[t][e];
    }
}

// the weight gradients: the slices' partials added in slice order (blockIdx.y: which of the nw outputs)
struct ProjBwdReduceArgs {
    int slices;
    uint32_t pstride;
    const float* part;
    int out[IGS_TOKEN_PROJ_MAX_OUT];
    float* dW[IGS_TOKEN_PROJ_MAX_OUT];
};
__global__ __launch_bounds__(256) void token_proj_bwd_reduce_kernel(const ProjBwdReduceArgs a)
{
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;                           // (the grid is exactly PB_DW / 256 blocks wide)
    const float* p = a.part + (size_t)a.out[blockIdx.y] * PB_DW + e;
    float s = 0.f;
    for (int z = 0; z < a.slices; z++) s += p[(size_t)z * a.pstride];
    a.dW[blockIdx.y][e] = s;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the entry points (the contract is in include/igs_rast.h)
// ---------------------------------------------------------------------------------------------------------------------------------
struct ProjBwdSlices { long long rows; int count, room; };                      // room: the slices the scratch has room for
static ProjBwdSlices proj_bwd_slices(long long T)
{
    ProjBwdSlices z = {PB_MIN_SLICE_ROWS, 0, 0};
    const long long least = (T + PB_MIN_SLICE_ROWS - 1) / PB_MIN_SLICE_ROWS;
    z.room = (int)(least < IGS_TOKEN_PROJ_BWD_MAX_SLICES ? least : IGS_TOKEN_PROJ_BWD_MAX_SLICES);
    if (least > IGS_TOKEN_PROJ_BWD_MAX_SLICES) {                                 // above the cap the slices get longer, in whole trips
        const long long per = (T + IGS_TOKEN_PROJ_BWD_MAX_SLICES - 1) / IGS_TOKEN_PROJ_BWD_MAX_SLICES;
        z.rows = (per + FFN_TRIP_ROWS - 1) / FFN_TRIP_ROWS * FFN_TRIP_ROWS;
    }
    z.count = (int)((T + z.rows - 1) / z.rows);
    return z;
}

extern "C" long long igs_token_proj_bwd_scratch_bytes(long long T, int n)
{
    if (n < 1 || n > IGS_TOKEN_PROJ_MAX_OUT || T < 0 || T > IGS_TOKEN_PROJ_MAX_ROWS) return -1;
    return (long long)proj_bwd_slices(T).room * n * PB_DW * (long long)sizeof(float);
}

extern "C" int igs_token_proj_bwd(void* stream, long long T, int n, int compute_dtype, const void* x, int x_dtype, long long x_stride,
                                  const void* const* g, int g_dtype, const long long* g_stride, const long long* rot, const void* wpack_t,
                                  void* scratch, long long scratch_bytes, void* dx, int dx_dtype, long long dx_stride, float* const* dW)
{
    const char* fn = "igs_token_proj_bwd";
    if (!dtype_ok(compute_dtype) || !dtype_ok(x_dtype) || !dtype_ok(g_dtype) || !dtype_ok(dx_dtype)) return fail_in(fn, "unknown dtype code");
    if (n < 1 || n > IGS_TOKEN_PROJ_MAX_OUT) return fail_in(fn, "n out of range (1..IGS_TOKEN_PROJ_MAX_OUT)");
    if (T < 0 || T > IGS_TOKEN_PROJ_MAX_ROWS) return fail_in(fn, "T out of range (0..IGS_TOKEN_PROJ_MAX_ROWS)");
    if (ffn_stride_bad(x_stride) || ffn_stride_bad(dx_stride)) return fail_in(fn, "a row stride is below the row length 128 or above IGS_TOKENS_MAX_STRIDE");
    const void* gp[IGS_TOKEN_PROJ_MAX_OUT] = {};
    float* wp[IGS_TOKEN_PROJ_MAX_OUT] = {};
    bool any_g = false, any_w = false;
    for (int j = 0; j < n; j++) {
        gp[j] = g ? g[j] : nullptr;
        wp[j] = dW ? dW[j] : nullptr;
        any_g = any_g || gp[j];
        any_w = any_w || wp[j];
    }
    if (any_g && !g_stride) return fail_in(fn, "NULL pointer: g_stride");
    for (int j = 0; j < n; j++)
        if (gp[j] && ffn_stride_bad(g_stride[j])) return fail_in(fn, "a row stride is below the row length 128 or above IGS_TOKENS_MAX_STRIDE");
    if (rot)
        for (int j = 0; j < n; j++)
            if (rot[j] < 0 || (rot[j] >= T && !(T == 0 && rot[j] == 0))) return fail_in(fn, "a rot[j] is outside 0..T-1");
    for (int j = 0; j < n; j++)
        if (!ptr_aligned(wp[j], 16)) return fail_in(fn, "a dW[j] must be aligned to 16 bytes");
    hipStream_t st_ = (hipStream_t)stream;
    if (T == 0) {
        for (int j = 0; j < n; j++)
            if (wp[j]) HIP_TRY(hipMemsetAsync(wp[j], 0, PB_DW * sizeof(float), st_), "token projection bwd zero-fill");
        return 0;
    }
    if (!dx && !any_w) return 0;
    if (any_w && !x) return fail_in(fn, "NULL pointer: x is read for the weight gradients");
    if (dx && !wpack_t) return fail_in(fn, "NULL pointer: wpack_t is read for dx");
    const long long need = igs_token_proj_bwd_scratch_bytes(T, n);
    if (any_w && !scratch) return fail_in(fn, "NULL pointer: scratch");
    if (!ptr_aligned(x, dtype_bytes(x_dtype)) || !ptr_aligned(dx, dtype_bytes(dx_dtype))) return fail_in(fn, "a pointer is not aligned to its element size");
    for (int j = 0; j < n; j++)
        if (!ptr_aligned(gp[j], dtype_bytes(g_dtype))) return fail_in(fn, "a pointer is not aligned to its element size");
    if (!ptr_aligned(wpack_t, 16)) return fail_in(fn, "wpack_t must be aligned to 16 bytes");
    if (!ptr_aligned(scratch, 16)) return fail_in(fn, "scratch must be aligned to 16 bytes");
    if (any_w && scratch_bytes < need) return fail_in(fn, "scratch is smaller than igs_token_proj_bwd_scratch_bytes");
    {
        // every output against every input and every other output
        ByteSpan in[IGS_TOKEN_PROJ_MAX_OUT + 2], out[IGS_TOKEN_PROJ_MAX_OUT + 2];
        const char* out_name[IGS_TOKEN_PROJ_MAX_OUT + 2];
        int ni = 0, no = 0;
        if (x) in[ni++] = ffn_span(x, x_dtype, T, x_stride);
        if (wpack_t) in[ni++] = byte_span(wpack_t, (size_t)n * PROJ_MAT * dtype_bytes(compute_dtype));
        for (int j = 0; j < n; j++)
            if (gp[j]) in[ni++] = ffn_span(gp[j], g_dtype, T, g_stride[j]);
        if (dx) { out_name[no] = "dx overlaps an input or another output"; out[no++] = ffn_span(dx, dx_dtype, T, dx_stride); }
        if (any_w) { out_name[no] = "scratch overlaps an input or another output"; out[no++] = byte_span(scratch, (size_t)need); }
        for (int j = 0; j < n; j++)
            if (wp[j]) { out_name[no] = "a dW[j] overlaps an input or another output"; out[no++] = byte_span(wp[j], PB_DW * sizeof(float)); }
        for (int o = 0; o < no; o++) {
            for (int i = 0; i < ni; i++)
                if (spans_overlap(out[o], in[i])) return fail_in(fn, out_name[o]);
            for (int p = 0; p < o; p++)
                if (spans_overlap(out[o], out[p])) return fail_in(fn, out_name[o]);
        }
    }

    const bool half = compute_dtype == IGS_DTYPE_F16;
    if (dx) {
        ProjBwdDxArgs k = {};
        k.T = T;
        for (int j = 0; j < n; j++) {
            if (!gp[j]) continue;
            const int i = k.na++;
            k.g[i] = TokPtr{gp[j], g_dtype == IGS_DTYPE_F16};
            k.gs[i] = g_stride[j];
            k.g_vec[i] = ffn_vec(gp[j], g_dtype, g_stride[j]);
            k.mat[i] = j;
            k.rot[i] = rot ? rot[j] : 0;
        }
        k.dx = TokPtr{dx, dx_dtype == IGS_DTYPE_F16};
        k.dxs = dx_stride;
        k.dx_vec = ffn_vec(dx, dx_dtype, dx_stride);
        k.wt = wpack_t;
        // the forward's launch rule: min(trips, compute units x workgroups per compute unit) workgroups
        const long long trips = (T + FFN_TRIP_ROWS - 1) / FFN_TRIP_ROWS;
        const long long groups = (long long)mlp_cus() * (half ? ProjCfg<_Float16>::GROUPS_PER_CU : ProjCfg<float>::GROUPS_PER_CU);
        const dim3 grid((unsigned)(trips < groups ? trips : groups)), block(FFN_THREADS);
        if (half) hipLaunchKernelGGL((token_proj_bwd_dx_kernel<_Float16>), grid, block, 0, st_, k);
        else hipLaunchKernelGGL((token_proj_bwd_dx_kernel<float>), grid, block, 0, st_, k);
    }
    if (any_w) {
        const ProjBwdSlices z = proj_bwd_slices(T);
        ProjBwdWgradArgs w = {};
        ProjBwdReduceArgs q = {};
        w.T = T; w.slice_rows = z.rows; w.slices = z.count;
        w.pstride = (uint32_t)n * PB_DW;
        w.x = TokPtr{x, x_dtype == IGS_DTYPE_F16};
        w.xs = x_stride;
        w.part = (float*)scratch;
        for (int j = 0; j < n; j++) {
            if (!wp[j]) continue;
            if (!gp[j]) {                                                        // no gradient reached output j: its weight gradient is zero
                HIP_TRY(hipMemsetAsync(wp[j], 0, PB_DW * sizeof(float), st_), "token projection bwd zero-fill");
                continue;
            }
            const int i = w.nw++;
            w.g[i] = TokPtr{gp[j], g_dtype == IGS_DTYPE_F16};
            w.gs[i] = g_stride[j];
            w.rot[i] = rot ? rot[j] : 0;
            w.out[i] = j;
            q.out[i] = j;
            q.dW[i] = wp[j];
        }
        if (w.nw > 0) {
            const long long units = 4LL * w.nw * w.slices;
            const dim3 wgrid((unsigned)((units + PB_WG_WAVES - 1) / PB_WG_WAVES)), wblock(PB_WG_THREADS);
            if (half) hipLaunchKernelGGL((token_proj_bwd_wgrad_kernel<_Float16>), wgrid, wblock, 0, st_, w);
            else hipLaunchKernelGGL((token_proj_bwd_wgrad_kernel<float>), wgrid, wblock, 0, st_, w);
            q.slices = z.count; q.pstride = w.pstride; q.part = w.part;
            hipLaunchKernelGGL(token_proj_bwd_reduce_kernel, dim3(PB_DW / 256, (unsigned)w.nw), dim3(256), 0, st_, q);
        }
    }
    HIP_TRY(hipGetLastError(), "token projection bwd launch");
    return 0;
}
