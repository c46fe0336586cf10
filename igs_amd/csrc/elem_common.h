// elem_common.h -- the small device helpers that every kernel file shares: the workgroup barrier, the float32 / float16 element access
// (typed, or by a runtime dtype code), the exact GELU's Phi, the lane-sum butterfly and the tail of the corrected two-pass statistics.  Device only; nothing
// of the rasterizer is included.
#pragma once
#include <hip/hip_runtime.h>

// The workgroup barrier of every kernel that hands data through LDS: __syncthreads() with its release side spelled out.
// Round 3: the forward's round loop ends with `wave_done[wid] = ...` (ds_write_b32) and begins with __syncthreads() followed by the
// read of all four flags that decides `break` -- and hipcc emitted a bare s_barrier at that loop header, with no s_waitcnt lgkmcnt(0)
// behind the store (its waitcnt scoreboard took the counter for zero across the back edge).  A wave whose store is still queued
// when the barrier opens lets the waves that read first see a stale 0: they go round again while the others break.  In the
// stand-alone forward that only costs the stragglers a redundant round (their pixels are finished; waves that have ended no
// longer count at barriers).  In the fused forward + backward kernel it is fatal: the stragglers stage FORWARD records into the LDS
// the others already use for the BACKWARD -- Gaussian ids read from that are garbage, and the accumulator atomic faults
// (dense diagnostic scene, where nearly every tile ends its forward early; found with the ROCm debug agent: LDS dump of the faulting
// workgroup).  The wait costs nothing where the compiler would have put it anyway.
// -DIGS_NO_RELEASE_WAIT leaves the wait to the compiler again, in every kernel that calls this: the control of tools/audit_barriers.py.
__device__ __forceinline__ void wg_barrier()
{
#ifndef IGS_NO_RELEASE_WAIT
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
    __syncthreads();
}

// One element, or four consecutive ones on the 4-element grid of the type (16 / 8 bytes), as float32.  A float16 store rounds to
// nearest even, once.
typedef _Float16 h4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float ld(const float* p) { return *p; }
__device__ __forceinline__ float ld(const _Float16* p) { return (float)*p; }
__device__ __forceinline__ void st(float* p, float v) { *p = v; }
__device__ __forceinline__ void st(_Float16* p, float v) { *p = (_Float16)v; }
__device__ __forceinline__ float4 ld4(const float* p) { return *(const float4*)p; }
__device__ __forceinline__ float4 ld4(const _Float16* p)
{
    const h4_t h = *(const h4_t*)p;
    return make_float4((float)h.x, (float)h.y, (float)h.z, (float)h.w);
}
__device__ __forceinline__ void st4(float* p, float4 v) { *(float4*)p = v; }
__device__ __forceinline__ void st4(_Float16* p, float4 v)
{
    h4_t h;
    h.x = (_Float16)v.x; h.y = (_Float16)v.y; h.z = (_Float16)v.z; h.w = (_Float16)v.w;
    *(h4_t*)p = h;
}

// an operand whose dtype is a runtime code (half != 0: float16), addressed in elements
struct TokPtr { const void* p; int half; };
__device__ __forceinline__ float ld(TokPtr t, size_t i) { return t.half ? ld((const _Float16*)t.p + i) : ld((const float*)t.p + i); }
__device__ __forceinline__ float4 ld4(TokPtr t, size_t i) { return t.half ? ld4((const _Float16*)t.p + i) : ld4((const float*)t.p + i); }
__device__ __forceinline__ void st(TokPtr t, size_t i, float v) { if (t.half) st((_Float16*)t.p + i, v); else st((float*)t.p + i, v); }
__device__ __forceinline__ void st4(TokPtr t, size_t i, float4 v) { if (t.half) st4((_Float16*)t.p + i, v); else st4((float*)t.p + i, v); }

// Phi(g) = 0.5 (1 + erf(g / sqrt 2)): the exact GELU is g Phi(g) (tokens.hip's GEGLU and its backward, ffn.hip's feed-forward)
__device__ __forceinline__ float gelu_cdf(float g) { return 0.5f * (1.f + erff(g * 0.70710678118654752f)); }

// The sums of N values over every group of LANES neighbouring lanes of a wave (a power of two), the same bits in every lane of the
// group: an xor butterfly, largest offset first, whose two operands commute.  A fixed order: the same result on every run.
template <int LANES, int N>
__device__ __forceinline__ void lane_sum(float (&a)[N])
{
#pragma unroll
    for (int off = LANES / 2; off > 0; off >>= 1) {
#pragma unroll
        for (int i = 0; i < N; i++) a[i] += __shfl_xor(a[i], off, 64);
    }
}
template <int LANES>
__device__ __forceinline__ float lane_sum(float v)
{
    float a[1] = {v};
    lane_sum<LANES>(a);
    return a[0];
}

// mean and 1 / sqrt(var + eps) from the centre m and the sums s1 of d = v - m and s2 of d d over the n elements: the corrected two-pass
// form, in which s1 / n is the rounding error of m and the subtracted term a correction of that order, not a cancellation
__device__ __forceinline__ void norm_finish(float m, float s1, float s2, float n, float eps, float& mean, float& rstd)
{
    const float dm = s1 / n;
    float var = s2 / n - dm * dm;
    var = var < 0.f ? 0.f : var;                               // (keeps a NaN)
    mean = m + dm;
    rstd = 1.f / sqrtf(var + eps);
}
