// proj.hip -- up to five bias-free 128 -> 128 projections of one [T, 128] activation in one launch: the q / k / v heads of the unimatch
// TransformerLayers (igs/models/unimatch/transformer.py:25-27, 104-106; a FeatureTransformer block's five products of its input at once,
// :274-289).  DESIGN.md 28.  Per row t and matrix j:
//
//   out[(t + rot[j]) mod T][128 j .. 128 j + 127] = W_j x[t]
//
// so the matrices' results lie side by side in one buffer whose column slices wattn.hip reads in place, and rot[j] = T / 2 writes a
// projection of the batch-swapped activation without the swap ever being built.
//
// Tile layout: ffn.hip's, with its helpers (ffn_common.h).  One wave owns 32 rows and holds them in registers as the B operand of all n
// matrices, so x is read once; H^T = W X^T on 32x32 MFMA tiles with the output channel as the accumulator's row and the data row as its
// column.  A row's result depends on that row and the weights only, in a fixed order.
//
// The matrices go through LDS one at a time (a matrix is 16 tiles: 64 KB in float32, 32 KB in float16).  With n <= 2 they are staged once
// and stay.  With n > 2 they stream through two buffers, matrix after matrix and trip after trip: while the products of one matrix run, a
// thread fetches its 16-byte pieces of the next into registers, a quarter (one output tile's four tiles) in front of each output tile's
// products, and writes them to the other buffer behind them; one workgroup barrier per matrix.  The buffer written during matrix s was
// last read during matrix s - 1, which every wave left through that matrix's barrier.  float32 holds one workgroup of 4 waves per compute
// unit (128 KB of LDS), float16 two (64 KB each).  A workgroup loops over trips of 128 rows; the grid is at most what the chip holds at
// once.  Rows past T read row 0 instead and are never stored.
#include "proj_common.h"                  // PROJ_MAT, ProjCfg; ffn_common.h's row loads and stores, staging and argument checks

struct ProjArgs {
    long long T;
    int n;
    TokPtr x, out;
    long long xs, os;                      // row strides in elements
    int x_vec, o_vec;                      // four-element access allowed (base and stride on the grid)
    const void* w;                         // the pack: n matrices of 16 tiles
    long long rot[IGS_TOKEN_PROJ_MAX_OUT];
};

template <typename T>
__global__ __launch_bounds__(FFN_THREADS, (ProjCfg<T>::WAVES_PER_SIMD)) void token_proj_kernel(const ProjArgs a)
{
    typedef ProjCfg<T> Cfg;
    __shared__ __attribute__((aligned(16))) T wl[2 * PROJ_MAT];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const T* wg = (const T*)a.w;
    const bool stream = a.n > 2;                                                 // (uniform)
    const long long trips = (a.T + FFN_TRIP_ROWS - 1) / FFN_TRIP_ROWS;
    // the matrices this workgroup walks, over all its trips: s = 0 .. stages - 1 is matrix s % n in buffer s & 1
    const long long stages = (trips - blockIdx.x + gridDim.x - 1) / gridDim.x * a.n;

    ffn_stage(wl, wg, (stream ? 1 : a.n) * PROJ_MAT);
    wg_barrier();

    long long s = 0;
    for (long long trip = blockIdx.x; trip < trips; trip += gridDim.x) {         // (uniform over the workgroup: every wave takes every trip)
        const long long row = trip * FFN_TRIP_ROWS + wave * 32 + r;
        const bool live = row < a.T;
        MlpIn<T> in;
        ffn_load_row(in, a.x, (size_t)(live ? row : 0) * a.xs, a.x_vec, h);      // a row past T reads row 0 and is never stored

        for (int j = 0; j < a.n; j++, s++) {
            const T* buf = wl + (stream ? (int)(s & 1) : j) * PROJ_MAT;
            const bool more = stream && s + 1 < stages;
            const T* next = wg + (size_t)(j + 1 == a.n ? 0 : j + 1) * PROJ_MAT;
            T* other = wl + (int)((s + 1) & 1) * PROJ_MAT;
            float4 f[16];
#pragma unroll
            for (int t = 0; t < 4; t++) {
                attn_f4 stg[Cfg::PIECES];
                if (more) {
#pragma unroll
                    for (int q = 0; q < Cfg::PIECES; q++) stg[q] = ((const attn_f4*)(next + t * Cfg::QUARTER))[q * FFN_THREADS + threadIdx.x];
                }
                attn_acc o;
#pragma unroll
                for (int i = 0; i < 16; i++) o[i] = 0.f;
#pragma unroll
                for (int k = 0; k < 4; k++) o = mlp_mm(buf + (t * 4 + k) * MLP_TILE, lane, in, k, o);
#pragma unroll
                for (int g = 0; g < 4; g++) f[4 * t + g] = make_float4(o[4 * g], o[4 * g + 1], o[4 * g + 2], o[4 * g + 3]);
                if (more) {
#pragma unroll
                    for (int q = 0; q < Cfg::PIECES; q++) ((attn_f4*)(other + t * Cfg::QUARTER))[q * FFN_THREADS + threadIdx.x] = stg[q];
                }
            }
            if (live) {
                long long orow = row + a.rot[j];
                if (orow >= a.T) orow -= a.T;
                ffn_write_groups(f, a.out, (size_t)orow * a.os + 128 * j, a.o_vec, h);
            }
            if (stream) wg_barrier();
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the entry points (the contract is in include/igs_rast.h)
// ---------------------------------------------------------------------------------------------------------------------------------

extern "C" long long igs_token_proj_pack_elems(int n)
{
    if (n < 1 || n > IGS_TOKEN_PROJ_MAX_OUT) return -1;
    return (long long)n * PROJ_MAT;
}

extern "C" int igs_token_proj_fwd(void* stream, long long T, int n, int compute_dtype, const void* x, int x_dtype, long long x_stride, const void* wpack,
                                  const long long* rot, void* out, int out_dtype, long long out_stride)
{
    const char* fn = "igs_token_proj_fwd";
    if (!dtype_ok(compute_dtype) || !dtype_ok(x_dtype) || !dtype_ok(out_dtype)) return fail_in(fn, "unknown dtype code");
    if (n < 1 || n > IGS_TOKEN_PROJ_MAX_OUT) return fail_in(fn, "n out of range (1..IGS_TOKEN_PROJ_MAX_OUT)");
    if (T < 0 || T > IGS_TOKEN_PROJ_MAX_ROWS) return fail_in(fn, "T out of range (0..IGS_TOKEN_PROJ_MAX_ROWS)");
    if (ffn_stride_bad(x_stride)) return fail_in(fn, "x's row stride is below the row length 128 or above IGS_TOKENS_MAX_STRIDE");
    if (out_stride < 128LL * n || out_stride > IGS_TOKENS_MAX_STRIDE) return fail_in(fn, "out's row stride is below the row length 128 n or above IGS_TOKENS_MAX_STRIDE");
    if (rot)
        for (int j = 0; j < n; j++)
            if (rot[j] < 0 || (rot[j] >= T && !(T == 0 && rot[j] == 0))) return fail_in(fn, "a rot[j] is outside 0..T-1");
    if (T == 0) return 0;
    if (!x || !wpack || !out) return fail_in(fn, "NULL pointer");
    if (!ptr_aligned(x, dtype_bytes(x_dtype)) || !ptr_aligned(out, dtype_bytes(out_dtype))) return fail_in(fn, "a pointer is not aligned to its element size");
    if (!ptr_aligned(wpack, 16)) return fail_in(fn, "wpack must be aligned to 16 bytes");
    const ByteSpan so = byte_span(out, (size_t)((T - 1) * out_stride + 128LL * n) * dtype_bytes(out_dtype));
    if (spans_overlap(so, ffn_span(x, x_dtype, T, x_stride))) return fail_in(fn, "out overlaps x");

    ProjArgs k = {};
    k.T = T;
    k.n = n;
    k.x = TokPtr{x, x_dtype == IGS_DTYPE_F16}; k.out = TokPtr{out, out_dtype == IGS_DTYPE_F16};
    k.xs = x_stride; k.os = out_stride;
    k.x_vec = ffn_vec(x, x_dtype, x_stride); k.o_vec = ffn_vec(out, out_dtype, out_stride);
    k.w = wpack;
    for (int j = 0; j < n; j++) k.rot[j] = rot ? rot[j] : 0;

    // the launch rule (include/igs_rast.h): min(trips, compute units x workgroups per compute unit) workgroups
    const bool half = compute_dtype == IGS_DTYPE_F16;
    const long long trips = (T + FFN_TRIP_ROWS - 1) / FFN_TRIP_ROWS;
    const long long groups = (long long)mlp_cus() * (half ? ProjCfg<_Float16>::GROUPS_PER_CU : ProjCfg<float>::GROUPS_PER_CU);
    const dim3 grid((unsigned)(trips < groups ? trips : groups)), block(FFN_THREADS);
    hipStream_t st_ = (hipStream_t)stream;
    if (half) hipLaunchKernelGGL((token_proj_kernel<_Float16>), grid, block, 0, st_, k);
    else hipLaunchKernelGGL((token_proj_kernel<float>), grid, block, 0, st_, k);
    HIP_TRY(hipGetLastError(), "token projection launch");
    return 0;
}
