// param_reduce.h -- the deterministic sum of a backward's partial parameter rows (cond.hip: ModLN, tokens.hip: LayerNorm): every
// workgroup of the backward leaves one row of d weight / d bias partial sums, and these rows are added in row order.  No float atomics,
// bitwise reproducible.  The kernel is static: every file that includes this gets its own copy.
#pragma once
#include "elem_common.h"

#define PARAM_REDUCE_WAVES 16
#define PARAM_REDUCE_GROUPS 64                                 // rows of the staging block between the two rounds

// Adds rows of parameter partial sums in row order.  blockIdx.y = 0: d weight, 1: d bias; blockIdx.z = g: the g-th contiguous share of
// the T rows of `part` ([T][2][C]) goes to out0 / out1 + g * out_stride.  A workgroup owns 64 channels; wave k adds its contiguous part
// of the share in row order (eight loads in flight, added in order), then the 16 waves' sums are added in wave order.
static __global__ void __launch_bounds__(64 * PARAM_REDUCE_WAVES)
param_reduce_kernel(int C, uint32_t T, const float* __restrict__ part, float* __restrict__ out0, float* __restrict__ out1, size_t out_stride)
{
    __shared__ float sm[PARAM_REDUCE_WAVES * 64];
    const int which = blockIdx.y;
    float* dst = which ? out1 : out0;
    if (!dst) return;                                          // (uniform)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, c = blockIdx.x * 64 + lane;
    const uint32_t gshare = (T + gridDim.z - 1) / gridDim.z;
    const uint32_t g0 = min(blockIdx.z * gshare, T), g1 = min(g0 + gshare, T);
    const uint32_t share = (g1 - g0 + PARAM_REDUCE_WAVES - 1) / PARAM_REDUCE_WAVES;
    const uint32_t t0 = min(g0 + (uint32_t)wv * share, g1), t1 = min(t0 + share, g1);
    float s = 0.f;
    if (c < C) {
        const float* src = part + (size_t)which * C + c;
        uint32_t t = t0;
        for (; t + 8 <= t1; t += 8) {
            float a[8];
#pragma unroll
            for (int k = 0; k < 8; k++) a[k] = src[(size_t)(t + k) * 2 * C];
#pragma unroll
            for (int k = 0; k < 8; k++) s += a[k];
        }
        for (; t < t1; t++) s += src[(size_t)t * 2 * C];
    }
    sm[wv * 64 + lane] = s;
    wg_barrier();
    if (wv == 0 && c < C) {
        float tot = 0.f;
        for (int k = 0; k < PARAM_REDUCE_WAVES; k++) tot += sm[k * 64 + lane];
        dst[(size_t)blockIdx.z * out_stride + c] = tot;
    }
}

// dw / db (either may be NULL) <- the sum of the T rows of `part`.  With `stage` (room for PARAM_REDUCE_GROUPS rows) in two rounds,
// T rows -> PARAM_REDUCE_GROUPS rows -> one, so that no wave walks more than T / 1024 rows behind one another's latency; without, in
// one round (for T of a thousand or so).
static inline hipError_t launch_param_reduce(hipStream_t s, int C, uint32_t T, const float* part, float* stage, float* dw, float* db)
{
    const dim3 blk(64 * PARAM_REDUCE_WAVES);
    const unsigned cg = (C + 63) / 64;
    if (stage) {
        hipLaunchKernelGGL(param_reduce_kernel, dim3(cg, 2, PARAM_REDUCE_GROUPS), blk, 0, s, C, T, part, stage, stage + C, (size_t)2 * C);
        part = stage;
        T = PARAM_REDUCE_GROUPS;
    }
    hipLaunchKernelGGL(param_reduce_kernel, dim3(cg, 2, 1), blk, 0, s, C, T, part, dw, db, (size_t)0);
    return hipGetLastError();
}
