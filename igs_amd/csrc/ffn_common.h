// ffn_common.h -- what the layer tail's forward and backward share (ffn.hip, ffn_bwd.hip): the trip and chunk constants, the loads and stores of a
// row's four-channel groups, a row as a B operand, the LayerNorm statistics of a row held in four accumulator tiles, the staging of weight
// tiles through LDS and the entry points' checks of sizes, strides and spans.  ffn.hip states the tile layout.
#pragma once
#include "mlp_common.h"                   // MlpIn, mlp_mm, MLP_TILE, mlp_cus
#include "host_api.h"

#define FFN_WAVES 4
#define FFN_THREADS (64 * FFN_WAVES)
#define FFN_TRIP_ROWS IGS_LAYER_TAIL_TRIP_ROWS
#define FFN_WM_TILES 16                    // Wm [128, 128]
#define FFN_W1_TILES 8                     // of one chunk: W1's output tile j over [s ; n1]
#define FFN_W2_TILES 4                     // of one chunk: W2's input tile j
#define FFN_CHUNK_TILES (FFN_W1_TILES + FFN_W2_TILES)
static_assert(FFN_TRIP_ROWS == 32 * FFN_WAVES, "a trip is 32 rows per wave");

// The lane's 16 four-channel groups of one row (group 4 k + g: channels 32 k + 8 g + 4 h ..), read and written in one straight run per
// (dtype, access width) so that the loads are all in flight together: the dtype and the width are uniform, decided once per row.
template <typename E, bool VEC>
__device__ __forceinline__ void ffn_read_groups(float4 (&f)[16], const E* row, int h)
{
#pragma unroll
    for (int q = 0; q < 16; q++) {
        const E* p = row + 32 * (q >> 2) + 8 * (q & 3) + 4 * h;
        if (VEC) f[q] = ld4(p);
        else f[q] = make_float4(ld(p), ld(p + 1), ld(p + 2), ld(p + 3));
    }
}
__device__ __forceinline__ void ffn_read_groups(float4 (&f)[16], TokPtr t, size_t base, bool vec, int h)
{
    if (t.half) {
        if (vec) ffn_read_groups<_Float16, true>(f, (const _Float16*)t.p + base, h);
        else ffn_read_groups<_Float16, false>(f, (const _Float16*)t.p + base, h);
    } else {
        if (vec) ffn_read_groups<float, true>(f, (const float*)t.p + base, h);
        else ffn_read_groups<float, false>(f, (const float*)t.p + base, h);
    }
}
template <typename E, bool VEC>
__device__ __forceinline__ void ffn_write_groups(const float4 (&f)[16], E* row, int h)
{
#pragma unroll
    for (int q = 0; q < 16; q++) {
        E* p = row + 32 * (q >> 2) + 8 * (q & 3) + 4 * h;
        if (VEC) st4(p, f[q]);
        else { st(p, f[q].x); st(p + 1, f[q].y); st(p + 2, f[q].z); st(p + 3, f[q].w); }
    }
}
__device__ __forceinline__ void ffn_write_groups(const float4 (&f)[16], TokPtr t, size_t base, bool vec, int h)
{
    if (t.half) {
        if (vec) ffn_write_groups<_Float16, true>(f, (_Float16*)t.p + base, h);
        else ffn_write_groups<_Float16, false>(f, (_Float16*)t.p + base, h);
    } else {
        if (vec) ffn_write_groups<float, true>(f, (float*)t.p + base, h);
        else ffn_write_groups<float, false>(f, (float*)t.p + base, h);
    }
}

// a row of 128 channels as a B operand
template <typename T>
__device__ __forceinline__ void ffn_load_row(MlpIn<T>& in, TokPtr p, size_t base, bool vec, int h)
{
    float4 f[16];
    ffn_read_groups(f, p, base, vec, h);
#pragma unroll
    for (int q = 0; q < 16; q++) {
        const int k = q >> 2, e = 4 * (q & 3);
        in.set(k, e, f[q].x); in.set(k, e + 1, f[q].y); in.set(k, e + 2, f[q].z); in.set(k, e + 3, f[q].w);
    }
}

// mean and 1 / sqrt(var + eps) of the row this lane and lane ^ 32 hold as four accumulator tiles: the corrected two-pass form of
// elem_common.h.  Both lanes add the same two halves, so they hold the same bits; the order depends on nothing.
__device__ __forceinline__ void ffn_row_stats(const attn_acc (&o)[4], float eps, float& mean, float& rstd)
{
    float p[4];
#pragma unroll
    for (int t = 0; t < 4; t++) {
        p[t] = 0.f;
#pragma unroll
        for (int i = 0; i < 16; i++) p[t] += o[t][i];
    }
    float sum = (p[0] + p[1]) + (p[2] + p[3]);
    sum += __shfl_xor(sum, 32, 64);
    const float m = sum * (1.f / 128.f);
    float q1[4], q2[4];
#pragma unroll
    for (int t = 0; t < 4; t++) {
        q1[t] = 0.f; q2[t] = 0.f;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const float d = o[t][i] - m;
            q1[t] += d;
            q2[t] = fmaf(d, d, q2[t]);
        }
    }
    float s1 = (q1[0] + q1[1]) + (q1[2] + q1[3]), s2 = (q2[0] + q2[1]) + (q2[2] + q2[3]);
    s1 += __shfl_xor(s1, 32, 64);
    s2 += __shfl_xor(s2, 32, 64);
    norm_finish(m, s1, s2, 128.f, eps, mean, rstd);
}

// `n` elements (a multiple of 8 halves / 4 floats) from global memory into LDS, 16 bytes per thread and step
template <typename T>
__device__ __forceinline__ void ffn_stage(T* dst, const T* src, uint32_t n)
{
    const uint32_t pieces = n * (uint32_t)sizeof(T) / 16;
    for (uint32_t i = threadIdx.x; i < pieces; i += FFN_THREADS) ((attn_f4*)dst)[i] = ((const attn_f4*)src)[i];
}

// this thread's pieces of chunk j into registers, and from there into a chunk buffer ([W1's 8 tiles][W2's 4 tiles])
template <typename T, int PIECES, int W1_PIECES>
__device__ __forceinline__ void ffn_fetch(attn_f4 (&stg)[PIECES], const T* w1, const T* w2, int j)
{
    const attn_f4* p1 = (const attn_f4*)(w1 + (size_t)j * FFN_W1_TILES * MLP_TILE) + threadIdx.x;
    const attn_f4* p2 = (const attn_f4*)(w2 + (size_t)j * FFN_W2_TILES * MLP_TILE) + threadIdx.x;
#pragma unroll
    for (int q = 0; q < PIECES; q++) stg[q] = q < W1_PIECES ? p1[q * FFN_THREADS] : p2[(q - W1_PIECES) * FFN_THREADS];
}
template <typename T, int PIECES>
__device__ __forceinline__ void ffn_put(T* buf, const attn_f4 (&stg)[PIECES])
{
#pragma unroll
    for (int q = 0; q < PIECES; q++) ((attn_f4*)buf)[q * FFN_THREADS + threadIdx.x] = stg[q];
}

static inline bool ffn_hidden_ok(int hidden) { return hidden >= 32 && hidden <= IGS_LAYER_TAIL_MAX_HIDDEN && hidden % 32 == 0; }
static inline bool ffn_stride_bad(long long stride) { return stride < 128 || stride > IGS_TOKENS_MAX_STRIDE; }
// four-element access: the base on the dtype's four-element grid and the stride a multiple of four
static inline int ffn_vec(const void* p, int dtype, long long stride) { return ptr_aligned(p, vec_grid_bytes(dtype)) && (stride & 3) == 0; }
static inline ByteSpan ffn_span(const void* p, int dtype, long long T, long long stride)
{
    return byte_span(p, (size_t)((T - 1) * stride + 128) * dtype_bytes(dtype));
}
