// knn_common.h -- the device helpers that knn.hip (distCUDA2) and anchors.hip (FPS, kNN, bbox select) share: the one distance
// expression, the box distance derived from it, wave reductions and the 63-bit Morton key.
#pragma once
#include "common.h"

#define KNN_BITS 21                // Morton bits per axis
#define KNN_BBOX_PARTS 1024        // phase-1 partial boxes (one wave each)
// knn.hip, phase 1 alone: lohi[6] = box of the finite points of xyz[P], part: KNN_BBOX_PARTS * 8 floats of scratch
hipError_t launch_knn_bbox(hipStream_t s, int P, const float* xyz, float* part, float* lohi);

__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// THE distance: every candidate of every phase goes through this expression
__device__ __forceinline__ float dist2(float qx, float qy, float qz, float cx, float cy, float cz)
{
    const float dx = qx - cx, dy = qy - cy, dz = qz - cz;
    return __fmaf_rn(dz, dz, __fmaf_rn(dy, dy, __fmul_rn(dx, dx)));
}
// lower bound of dist2(q, c) over the box {lo, hi}: per-axis gaps (0 inside), same expression; +inf for an empty box (lo = +inf)
__device__ __forceinline__ float box_dist2(float qx, float qy, float qz, const float4& lo, const float4& hi)
{
    const float gx = fmaxf(fmaxf(lo.x - qx, qx - hi.x), 0.f);
    const float gy = fmaxf(fmaxf(lo.y - qy, qy - hi.y), 0.f);
    const float gz = fmaxf(fmaxf(lo.z - qz, qz - hi.z), 0.f);
    return __fmaf_rn(gz, gz, __fmaf_rn(gy, gy, __fmul_rn(gx, gx)));
}

__device__ __forceinline__ float wave_min(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

__device__ __forceinline__ uint64_t spread21(uint32_t v)
{
    uint64_t x = v & 0x1FFFFFull;
    x = (x | (x << 32)) & 0x1F00000000FFFFull;
    x = (x | (x << 16)) & 0x1F0000FF0000FFull;
    x = (x | (x << 8)) & 0x100F00F00F00F00Full;
    x = (x | (x << 4)) & 0x10C30C30C30C30C3ull;
    return (x | (x << 2)) & 0x1249249249249249ull;
}
// position quantised to KNN_BITS bits per axis inside lohi; a degenerate extent gives cell 0, non-finite input some cell in range
__device__ __forceinline__ uint64_t knn_key(const float* __restrict__ xyz, uint32_t i, const float* __restrict__ lohi)
{
    const float top = (float)((1u << KNN_BITS) - 1u);
    uint64_t key = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float lo = lohi[k], ext = fmaxf(lohi[3 + k] - lo, 1e-30f);
        const float t = fminf(fmaxf((xyz[3 * (size_t)i + k] - lo) / ext * top, 0.f), top);     // (fmaxf drops a NaN to 0)
        key |= spread21((uint32_t)t) << k;
    }
    return key;
}
