// ffn.hip -- the tail of a unimatch TransformerLayer in one launch (igs/models/unimatch/transformer.py:34-40, 117-146): everything behind
// the attention.  DESIGN.md 27.  Per token row, with a the attention's output and s the layer's `source` (128 channels each):
//
//   m = Wm a;  n1 = LN1(m);  without FFN: out = s + n1;  with FFN: h = gelu(W1 [s ; n1]),  y = W2 h,  out = s + LN2(y)
//
// The forward; ffn_bwd.hip is its backward and ffn_common.h what the two share.  A row is read once (s a second time for the residual,
// which is float32 whatever the operands are), the [rows, hidden] activations never leave registers and only `out` is written.
//
// Tile layout: mlp.hip's.  One wave owns 32 rows; the products are H^T = W X^T on 32x32 MFMA tiles with the output channel as the
// accumulator's row and the data row as its column, so an accumulator tile is the next product's B operand as it stands (float32) or
// after one rounding to half (float16), and a row's result depends on nothing but that row and the weights.  A row's LayerNorm is a sum
// over the lane's own 64 accumulator registers and one exchange with lane ^ 32: no LDS, a fixed order.
//
// The hidden dimension is streamed in chunks of 32 units.  Chunk j needs the 8 tiles of W1's output tile j (256 inputs) and the 4 tiles
// of W2's input tile j (128 outputs): 12 tiles, 48 KB in float32, 24 KB in float16, contiguous in the pack (include/igs_rast.h).  The
// chunks go through two LDS buffers: a thread fetches its 16-byte pieces of chunk j + 1 into registers before the products of chunk j
// and writes them to the other buffer behind them, so the fetch lies under the MFMAs; one workgroup barrier per chunk.  The buffer
// written in iteration j was last read in iteration j - 1, which every wave left through that iteration's barrier.
//
// LDS plan.  float16: Wm (32 KB) resident beside the two chunk buffers (48 KB).  float32 with FFN: the two chunk buffers (96 KB); Wm
// (64 KB) does not fit beside them and is staged into them at the start of every trip, between two barriers.  Without FFN: Wm alone,
// staged once.  Plus 2 KB of LayerNorm parameters.  With FFN one workgroup of 4 waves per compute unit (one wave per SIMD, up to 512
// registers), without FFN two.  A workgroup loops over trips of 128 rows; the grid is at most what the chip holds at once.  Rows past T
// read row 0 instead and are never stored.
#include "ffn_common.h"                   // the row loads, the row statistics, the chunk staging, the argument checks

template <typename T, bool FFN> struct FfnCfg {
    enum {
        HALF = AttnCfg<T>::HALF,
        RESIDENT = HALF || !FFN,                                                   // Wm is staged once per workgroup
        PIECES = FFN_CHUNK_TILES * MLP_TILE * (int)sizeof(T) / 16 / FFN_THREADS,   // a thread's 16-byte pieces of a chunk: 12 / 6
        W1_PIECES = PIECES * FFN_W1_TILES / FFN_CHUNK_TILES,
        LDS_TILES = FFN ? 2 * FFN_CHUNK_TILES + (HALF ? FFN_WM_TILES : 0) : FFN_WM_TILES,
        GROUPS_PER_CU = FFN ? 1 : 2,                                               // what the LDS and the registers let a compute unit hold
        WAVES_PER_SIMD = GROUPS_PER_CU * FFN_WAVES / 4,                            // ... on its four SIMDs: the kernel's register bound
    };
};

struct FfnArgs {
    long long T;
    TokPtr a, s, out;
    long long as, ss, os;                  // row strides in elements
    int a_vec, s_vec, o_vec;               // four-element access allowed (base and stride on the grid)
    const void* w;                         // the pack: Wm, then W1 by output tile, then W2 by input tile
    const float *ln1w, *ln1b, *ln2w, *ln2b;
    float eps1, eps2;
    int ht;                                // hidden / 32
};

// out = s + LN(o) w + b for the lane's channels of its row
__device__ __forceinline__ void ffn_store_row(const FfnArgs& a, const attn_acc (&o)[4], float mean, float rstd, const float* w, const float* b,
                                              long long row, int h)
{
    float4 f[16];
    ffn_read_groups(f, a.s, (size_t)row * a.ss, a.s_vec, h);
#pragma unroll
    for (int q = 0; q < 16; q++) {
        const int t = q >> 2, g = q & 3, c = 32 * t + 8 * g + 4 * h;
        const attn_f4 wv = *(const attn_f4*)(w + c), bv = *(const attn_f4*)(b + c);
        f[q].x += fmaf((o[t][4 * g] - mean) * rstd, wv[0], bv[0]);
        f[q].y += fmaf((o[t][4 * g + 1] - mean) * rstd, wv[1], bv[1]);
        f[q].z += fmaf((o[t][4 * g + 2] - mean) * rstd, wv[2], bv[2]);
        f[q].w += fmaf((o[t][4 * g + 3] - mean) * rstd, wv[3], bv[3]);
    }
    ffn_write_groups(f, a.out, (size_t)row * a.os, a.o_vec, h);
}

template <typename T, bool FFN>
__global__ __launch_bounds__(FFN_THREADS, (FfnCfg<T, FFN>::WAVES_PER_SIMD)) void layer_tail_kernel(const FfnArgs a)
{
    typedef FfnCfg<T, FFN> Cfg;
    constexpr int CHUNK = FFN_CHUNK_TILES * MLP_TILE;
    __shared__ __attribute__((aligned(16))) T wl[Cfg::LDS_TILES * MLP_TILE];
    __shared__ __attribute__((aligned(16))) float lnp[4 * 128];                  // LN1's weight and bias, LN2's weight and bias

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const T* wg = (const T*)a.w;
    const T* w1 = wg + FFN_WM_TILES * MLP_TILE;
    const T* w2 = w1 + (size_t)a.ht * FFN_W1_TILES * MLP_TILE;
    T* wm = wl + (FFN && Cfg::HALF ? 2 * CHUNK : 0);                             // float32 with FFN: Wm borrows the chunk buffers

    if (threadIdx.x < 128) {
        lnp[threadIdx.x] = a.ln1w[threadIdx.x];
        lnp[128 + threadIdx.x] = a.ln1b[threadIdx.x];
        lnp[256 + threadIdx.x] = FFN ? a.ln2w[threadIdx.x] : 0.f;
        lnp[384 + threadIdx.x] = FFN ? a.ln2b[threadIdx.x] : 0.f;
    }
    if (Cfg::RESIDENT) ffn_stage(wm, wg, FFN_WM_TILES * MLP_TILE);
    wg_barrier();

    const long long trips = (a.T + FFN_TRIP_ROWS - 1) / FFN_TRIP_ROWS;
    for (long long trip = blockIdx.x; trip < trips; trip += gridDim.x) {         // (uniform over the workgroup: every wave takes every trip)
        const long long row = trip * FFN_TRIP_ROWS + wave * 32 + r;
        const bool live = row < a.T;
        const long long rd = live ? row : 0;                                     // a row past T reads row 0 and is never stored

        // every wave left the trip before through the barrier behind its last chunk: the chunk buffers are free
        if (!Cfg::RESIDENT) ffn_stage(wm, wg, FFN_WM_TILES * MLP_TILE);
        MlpIn<T> in_a, in_s, in_n;
        ffn_load_row(in_a, a.a, (size_t)rd * a.as, a.a_vec, h);
        attn_f4 stg[Cfg::PIECES];
        if (FFN) {
            ffn_load_row(in_s, a.s, (size_t)rd * a.ss, a.s_vec, h);
            ffn_fetch<T, Cfg::PIECES, Cfg::W1_PIECES>(stg, w1, w2, 0);
        }
        if (!Cfg::RESIDENT) wg_barrier();

        // m = Wm a, n1 = LN1(m)
        attn_acc o[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
#pragma unroll
            for (int i = 0; i < 16; i++) o[t][i] = 0.f;
#pragma unroll
            for (int k = 0; k < 4; k++) o[t] = mlp_mm(wm + (t * 4 + k) * MLP_TILE, lane, in_a, k, o[t]);
        }
        float mean, rstd;
        ffn_row_stats(o, a.eps1, mean, rstd);
        if (!FFN) {
            if (live) ffn_store_row(a, o, mean, rstd, lnp, lnp + 128, row, h);
            continue;
        }
#pragma unroll
        for (int t = 0; t < 4; t++) {
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const int c = 32 * t + 8 * g + 4 * h;
                const attn_f4 wv = *(const attn_f4*)(lnp + c), bv = *(const attn_f4*)(lnp + 128 + c);
#pragma unroll
                for (int j = 0; j < 4; j++) in_n.set(t, 4 * g + j, fmaf((o[t][4 * g + j] - mean) * rstd, wv[j], bv[j]));
            }
        }
        if (!Cfg::RESIDENT) wg_barrier();                                        // everybody is done with Wm
        ffn_put<T, Cfg::PIECES>(wl, stg);
        wg_barrier();

        // y = sum over the chunks of W2_j gelu(W1_j [s ; n1])
#pragma unroll
        for (int t = 0; t < 4; t++) {
#pragma unroll
            for (int i = 0; i < 16; i++) o[t][i] = 0.f;
        }
        for (int j = 0; j < a.ht; j++) {
            const T* buf = wl + (j & 1) * CHUNK;
            if (j + 1 < a.ht) ffn_fetch<T, Cfg::PIECES, Cfg::W1_PIECES>(stg, w1, w2, j + 1);
            attn_acc hv;
#pragma unroll
            for (int i = 0; i < 16; i++) hv[i] = 0.f;
#pragma unroll
            for (int k = 0; k < 4; k++) hv = mlp_mm(buf + k * MLP_TILE, lane, in_s, k, hv);
#pragma unroll
            for (int k = 0; k < 4; k++) hv = mlp_mm(buf + (4 + k) * MLP_TILE, lane, in_n, k, hv);
            MlpIn<T> hin;                                                        // (tile 0 only)
#pragma unroll
            for (int i = 0; i < 16; i++) hin.set(0, i, hv[i] * gelu_cdf(hv[i]));
#pragma unroll
            for (int t = 0; t < 4; t++) o[t] = mlp_mm(buf + (FFN_W1_TILES + t) * MLP_TILE, lane, hin, 0, o[t]);
            if (j + 1 < a.ht) ffn_put<T, Cfg::PIECES>(wl + ((j + 1) & 1) * CHUNK, stg);
            wg_barrier();
        }
        ffn_row_stats(o, a.eps2, mean, rstd);
        if (live) ffn_store_row(a, o, mean, rstd, lnp + 256, lnp + 384, row, h);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the entry points (the contract is in include/igs_rast.h)
// ---------------------------------------------------------------------------------------------------------------------------------

extern "C" long long igs_layer_tail_pack_elems(int hidden, int has_ffn)
{
    if (!has_ffn) return (long long)FFN_WM_TILES * MLP_TILE;
    if (!ffn_hidden_ok(hidden)) return -1;
    return (long long)(FFN_WM_TILES + FFN_CHUNK_TILES * (hidden / 32)) * MLP_TILE;
}

extern "C" int igs_layer_tail_fwd(void* stream, long long T, int compute_dtype, int has_ffn, int hidden, const void* a, int a_dtype, long long a_stride,
                                  const void* s, int s_dtype, long long s_stride, const void* wpack, const float* ln1_w, const float* ln1_b, float eps1,
                                  const float* ln2_w, const float* ln2_b, float eps2, void* out, int out_dtype, long long out_stride)
{
    const char* fn = "igs_layer_tail_fwd";
    if (!dtype_ok(compute_dtype) || !dtype_ok(a_dtype) || !dtype_ok(s_dtype) || !dtype_ok(out_dtype)) return fail_in(fn, "unknown dtype code");
    if (T < 0 || T > IGS_LAYER_TAIL_MAX_ROWS) return fail_in(fn, "T out of range (0..IGS_LAYER_TAIL_MAX_ROWS)");
    if (has_ffn && !ffn_hidden_ok(hidden)) return fail_in(fn, "hidden must be a multiple of 32 in 32..IGS_LAYER_TAIL_MAX_HIDDEN");
    if (ffn_stride_bad(a_stride) || ffn_stride_bad(s_stride) || ffn_stride_bad(out_stride))
        return fail_in(fn, "a row stride is below the row length 128 or above IGS_TOKENS_MAX_STRIDE");
    if (!eps_ok(eps1) || (has_ffn && !eps_ok(eps2))) return fail_in(fn, "eps must be finite and >= 0");
    if (T == 0) return 0;
    if (!a || !s || !wpack || !ln1_w || !ln1_b || !out || (has_ffn && (!ln2_w || !ln2_b))) return fail_in(fn, "NULL pointer");
    if (!ptr_aligned(a, dtype_bytes(a_dtype)) || !ptr_aligned(s, dtype_bytes(s_dtype)) || !ptr_aligned(out, dtype_bytes(out_dtype)) ||
        !ptr_aligned(ln1_w, 4) || !ptr_aligned(ln1_b, 4) || (has_ffn && (!ptr_aligned(ln2_w, 4) || !ptr_aligned(ln2_b, 4))))
        return fail_in(fn, "a pointer is not aligned to its element size");
    if (!ptr_aligned(wpack, 16)) return fail_in(fn, "wpack must be aligned to 16 bytes");
    const ByteSpan so = ffn_span(out, out_dtype, T, out_stride);
    if (spans_overlap(so, ffn_span(a, a_dtype, T, a_stride)) || spans_overlap(so, ffn_span(s, s_dtype, T, s_stride)))
        return fail_in(fn, "out overlaps an input");

    FfnArgs k = {};
    k.T = T;
    k.a = TokPtr{a, a_dtype == IGS_DTYPE_F16}; k.s = TokPtr{s, s_dtype == IGS_DTYPE_F16}; k.out = TokPtr{out, out_dtype == IGS_DTYPE_F16};
    k.as = a_stride; k.ss = s_stride; k.os = out_stride;
    k.a_vec = ffn_vec(a, a_dtype, a_stride); k.s_vec = ffn_vec(s, s_dtype, s_stride); k.o_vec = ffn_vec(out, out_dtype, out_stride);
    k.w = wpack;
    k.ln1w = ln1_w; k.ln1b = ln1_b; k.ln2w = ln2_w; k.ln2b = ln2_b;
    k.eps1 = eps1; k.eps2 = eps2;
    k.ht = has_ffn ? hidden / 32 : 0;

    // the launch rule (include/igs_rast.h): min(trips, compute units x workgroups per compute unit) workgroups
    const long long trips = (T + FFN_TRIP_ROWS - 1) / FFN_TRIP_ROWS;
    const long long groups = (long long)mlp_cus() * (has_ffn ? FfnCfg<float, true>::GROUPS_PER_CU : FfnCfg<float, false>::GROUPS_PER_CU);
    const dim3 grid((unsigned)(trips < groups ? trips : groups)), block(FFN_THREADS);
    hipStream_t st_ = (hipStream_t)stream;
    const bool half = compute_dtype == IGS_DTYPE_F16;
    if (has_ffn) {
        if (half) hipLaunchKernelGGL((layer_tail_kernel<_Float16, true>), grid, block, 0, st_, k);
        else hipLaunchKernelGGL((layer_tail_kernel<float, true>), grid, block, 0, st_, k);
    } else {
        if (half) hipLaunchKernelGGL((layer_tail_kernel<_Float16, false>), grid, block, 0, st_, k);
        else hipLaunchKernelGGL((layer_tail_kernel<float, false>), grid, block, 0, st_, k);
    }
    HIP_TRY(hipGetLastError(), "layer tail launch");
    return 0;
}
