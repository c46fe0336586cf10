// inorm.hip -- the non-GEMM steps of the unimatch CNN encoder for gfx950: the 15 InstanceNorm2d layers of CNNEncoder / ResidualBlock
// (igs/models/unimatch/backbone.py:25-36,103-107; affine = False, no running statistics) fused with the ReLU, the residual add and the
// downsample branch's norm that follow them, and feature_add_position (igs/models/unimatch/utils.py:111-131 with position.py:29-46).
// Forward only: the backbone is frozen in IGS.  include/igs_rast.h states the contract, DESIGN.md section 18 the byte budget and the figures.
//
//   (1) inorm_resident_kernel: one workgroup per H W plane, the whole plane in registers (one global read, one global write).  The
//       workgroup is sized by the plane: 64 threads up to 1024 elements, 256 up to 4096 (4 values per thread) and up to 16384 (64 per
//       thread), 1024 threads up to 65536; the mode with a normalised skip holds two planes and stops at 32768.
//       Statistics, all float32: the plane's sum (per thread four running sums in register order, the wave by a butterfly whose two
//       operands commute, the waves' sums added in wave order by every thread: the same bits everywhere), m = sum / n; then from the
//       CENTRED registers d = v - m the two sums s1 = sum d and s2 = sum d d; mean = m + s1 / n and var = s2 / n - (s1 / n)^2, the
//       corrected two-pass form: s1 / n is the rounding error of m, a few ulp of the mean, so the subtracted term is a correction of the
//       order of the rounding, not a cancellation of two large numbers.  A constant plane gives d = s1 / n exactly and so exactly zero.
//   (2) inorm_streamed_kernel: planes above the resident limit, one 1024-thread workgroup per plane reading it twice (the second read
//       comes from L2 / the Infinity Cache).  The first read accumulates s1, s2 of d = v - m about a provisional centre m taken from the
//       plane itself (the mean of its first four elements), then the same two formulas.
//   In both, a plane base that is not 16 bytes aligned (an odd H W misaligns every second plane) gets a scalar head and tail of at most
//   three elements each around aligned four-element vectors; operands whose addresses are not congruent modulo 16 bytes (slices on
//   different offsets) go to the streamed kernel's scalar form at any size.  Nothing outside the plane is read.  No atomics and no cross-workgroup reduction.
//   (3) position_add_kernel: both features in one launch; the sine embedding is a function of (channel, y mod wh) or (channel, x mod ww),
//       evaluated in float32 with the accurate sinf / cosf, never stored.
#include "common.h"
#include "elem_common.h"
#include "host_api.h"

#define INORM_MAX_THREADS 1024
#define INORM_RESIDENT_MAX_ONE 65536
#define INORM_RESIDENT_MAX_TWO 32768
#define POSADD_THREADS 256

// torch.relu: a NaN stays a NaN (fmaxf would drop it)
__device__ __forceinline__ float inorm_relu(float v) { return v < 0.f ? 0.f : v; }

// How a plane of hw elements maps to the lanes.  Vector form: elements [0, head) and [head + 4 nvec, hw) are the scalar edges (thread t <
// head takes element t, thread head <= t < head + tail takes element 4 nvec + t), vector i is elements head + 4 i .. + 3.  Scalar form
// (vec == 0, the streamed kernel only): element i of thread t is i * THREADS + t.
struct InormGeom { uint32_t hw, head, nvec, tail; int vec; };
template <typename T>
__device__ __forceinline__ InormGeom inorm_geom(const T* plane, uint32_t hw, int vec)
{
    InormGeom g;
    g.hw = hw; g.vec = vec;
    const uint32_t mis = (uint32_t)(((uintptr_t)plane) & (4 * sizeof(T) - 1)) / (uint32_t)sizeof(T);      // elements past the vector grid
    g.head = min((4u - mis) & 3u, hw);
    g.nvec = (hw - g.head) >> 2;
    g.tail = hw - g.head - 4 * g.nvec;
    return g;
}
__device__ __forceinline__ uint32_t inorm_edge_index(const InormGeom& g, uint32_t t) { return t < g.head ? t : 4 * g.nvec + t; }

// the sums of N values over the workgroup, the same bits in every thread; `red` holds N * THREADS / 64 floats and is used once
template <int THREADS, int N>
__device__ __forceinline__ void inorm_block_sum(float (&a)[N], float* red)
{
    lane_sum<64>(a);
    if (THREADS == 64) return;
    constexpr int NW = THREADS / 64;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < N; i++) red[i * NW + wv] = a[i];
    }
    wg_barrier();
#pragma unroll
    for (int i = 0; i < N; i++) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < NW; k++) s += red[i * NW + k];
        a[i] = s;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (1) the resident path
// ---------------------------------------------------------------------------------------------------------------------------------
template <typename T, int THREADS, int NV>
struct InormPlane {
    float v[NV][4];
    float e;
    __device__ __forceinline__ bool vec_ok(const InormGeom& g, int j) const { return (uint32_t)(j * THREADS) + threadIdx.x < g.nvec; }
    __device__ __forceinline__ bool edge_ok(const InormGeom& g) const { return threadIdx.x < g.head + g.tail; }
    __device__ __forceinline__ void load(const T* p, const InormGeom& g)
    {
        e = 0.f;
#pragma unroll
        for (int j = 0; j < NV; j++) {
            float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
            if (vec_ok(g, j)) q = ld4(p + g.head + 4 * ((uint32_t)(j * THREADS) + threadIdx.x));
            v[j][0] = q.x; v[j][1] = q.y; v[j][2] = q.z; v[j][3] = q.w;
        }
        if (edge_ok(g)) e = ld(p + inorm_edge_index(g, threadIdx.x));
    }
    __device__ __forceinline__ float sum() const                // (the slots outside the plane hold zero)
    {
        float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < NV; j++)
#pragma unroll
            for (int k = 0; k < 4; k++) s[k] += v[j][k];
        return ((s[0] + s[1]) + (s[2] + s[3])) + e;
    }
    __device__ __forceinline__ void centred(const InormGeom& g, float m, float& s1, float& s2) const
    {
        float a[4] = {0.f, 0.f, 0.f, 0.f}, b[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < NV; j++) {
            const bool ok = vec_ok(g, j);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const float d = ok ? v[j][k] - m : 0.f;
                a[k] += d; b[k] = fmaf(d, d, b[k]);
            }
        }
        const float d = edge_ok(g) ? e - m : 0.f;
        s1 = ((a[0] + a[1]) + (a[2] + a[3])) + d;
        s2 = fmaf(d, d, (b[0] + b[1]) + (b[2] + b[3]));
    }
};

#define INORM_PLAIN IGS_INORM_PLAIN
#define INORM_RELU IGS_INORM_RELU
#define INORM_RELU_ADD_RELU IGS_INORM_RELU_ADD_RELU
#define INORM_RELU_ADDNORM_RELU IGS_INORM_RELU_ADDNORM_RELU

// one element's result from its normalised value y (and the skip operand k: raw for RELU_ADD_RELU, normalised for RELU_ADDNORM_RELU)
__device__ __forceinline__ float inorm_apply(int mode, float y, float k)
{
    if (mode == INORM_PLAIN) return y;
    y = inorm_relu(y);
    if (mode == INORM_RELU) return y;
    return inorm_relu(k + y);
}

// x, skip and out are NOT __restrict__: out == x is part of the contract (every thread reads its own elements before it writes them)
template <typename T, int THREADS, int NV, bool TWO>
__global__ void __launch_bounds__(THREADS, THREADS >= 256 ? 4 : 1)
inorm_resident_kernel(const T* x, const T* skip, T* out, uint32_t hw, int mode, float eps)
{
    constexpr int NW = THREADS / 64, NP = TWO ? 2 : 1;
    __shared__ float red[3 * NP * NW];
    const size_t base = (size_t)blockIdx.x * hw;
    const InormGeom g = inorm_geom(x + base, hw, 1);
    const float n = (float)hw;
    InormPlane<T, THREADS, NV> px, pk;
    px.load(x + base, g);
    if (TWO) pk.load(skip + base, g);
    float s[NP];
    s[0] = px.sum();
    if (TWO) s[NP - 1] = pk.sum();
    inorm_block_sum<THREADS, NP>(s, red);
    float m[NP];
#pragma unroll
    for (int i = 0; i < NP; i++) m[i] = s[i] / n;
    float c[2 * NP];
    px.centred(g, m[0], c[0], c[1]);
    if (TWO) pk.centred(g, m[NP - 1], c[2 * NP - 2], c[2 * NP - 1]);
    inorm_block_sum<THREADS, 2 * NP>(c, red + NP * NW);
    float mean, rstd, kmean = 0.f, krstd = 1.f;
    norm_finish(m[0], c[0], c[1], n, eps, mean, rstd);
    if (TWO) norm_finish(m[NP - 1], c[2 * NP - 2], c[2 * NP - 1], n, eps, kmean, krstd);
    const bool raw_skip = !TWO && mode == INORM_RELU_ADD_RELU;
    T* op = out + base;
    const T* kp = skip + base;                                 // (dereferenced only in the two modes that have a skip)
#pragma unroll
    for (int j = 0; j < NV; j++) {
        if (!px.vec_ok(g, j)) continue;
        const uint32_t at = g.head + 4 * ((uint32_t)(j * THREADS) + threadIdx.x);
        float k[4] = {0.f, 0.f, 0.f, 0.f};
        if (TWO) {
#pragma unroll
            for (int i = 0; i < 4; i++) k[i] = (pk.v[j][i] - kmean) * krstd;
        } else if (raw_skip) {
            const float4 q = ld4(kp + at);
            k[0] = q.x; k[1] = q.y; k[2] = q.z; k[3] = q.w;
        }
        float4 o;
        o.x = inorm_apply(mode, (px.v[j][0] - mean) * rstd, k[0]);
        o.y = inorm_apply(mode, (px.v[j][1] - mean) * rstd, k[1]);
        o.z = inorm_apply(mode, (px.v[j][2] - mean) * rstd, k[2]);
        o.w = inorm_apply(mode, (px.v[j][3] - mean) * rstd, k[3]);
        st4(op + at, o);
    }
    if (px.edge_ok(g)) {
        const uint32_t at = inorm_edge_index(g, threadIdx.x);
        const float k = TWO ? (pk.e - kmean) * krstd : raw_skip ? ld(kp + at) : 0.f;
        st(op + at, inorm_apply(mode, (px.e - mean) * rstd, k));
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (2) the streamed path
// ---------------------------------------------------------------------------------------------------------------------------------
// s1 = sum (v - m), s2 = sum (v - m)^2 over the plane, this thread's share; m = the mean of the plane's first four elements (the first
// one in a plane of fewer)
template <typename T>
__device__ __forceinline__ void inorm_stream_sums(const T* p, const InormGeom& g, float& m, float& s1, float& s2)
{
    m = g.hw >= 4 ? ((ld(p) + ld(p + 1)) + (ld(p + 2) + ld(p + 3))) * 0.25f : ld(p);
    float a[4] = {0.f, 0.f, 0.f, 0.f}, b[4] = {0.f, 0.f, 0.f, 0.f};
    if (g.vec) {
        for (uint32_t i = threadIdx.x; i < g.nvec; i += INORM_MAX_THREADS) {
            const float4 q = ld4(p + g.head + 4 * i);
            const float d0 = q.x - m, d1 = q.y - m, d2 = q.z - m, d3 = q.w - m;
            a[0] += d0; a[1] += d1; a[2] += d2; a[3] += d3;
            b[0] = fmaf(d0, d0, b[0]); b[1] = fmaf(d1, d1, b[1]); b[2] = fmaf(d2, d2, b[2]); b[3] = fmaf(d3, d3, b[3]);
        }
        if (threadIdx.x < g.head + g.tail) {
            const float d = ld(p + inorm_edge_index(g, threadIdx.x)) - m;
            a[0] += d; b[0] = fmaf(d, d, b[0]);
        }
    } else {
        uint32_t k = 0;
        for (uint32_t i = threadIdx.x; i < g.hw; i += INORM_MAX_THREADS, k = (k + 1) & 3) {
            const float d = ld(p + i) - m;
            if (k == 0) { a[0] += d; b[0] = fmaf(d, d, b[0]); }
            else if (k == 1) { a[1] += d; b[1] = fmaf(d, d, b[1]); }
            else if (k == 2) { a[2] += d; b[2] = fmaf(d, d, b[2]); }
            else { a[3] += d; b[3] = fmaf(d, d, b[3]); }
        }
    }
    s1 = (a[0] + a[1]) + (a[2] + a[3]);
    s2 = (b[0] + b[1]) + (b[2] + b[3]);
}

template <typename T, bool TWO>
__global__ void __launch_bounds__(INORM_MAX_THREADS, 4)
inorm_streamed_kernel(const T* x, const T* skip, T* out, uint32_t hw, int mode, int vec, float eps)
{
    constexpr int NW = INORM_MAX_THREADS / 64, NP = TWO ? 2 : 1;
    __shared__ float red[2 * NP * NW];
    const size_t base = (size_t)blockIdx.x * hw;
    const T* xp = x + base;
    const T* kp = skip + base;                                 // (dereferenced only in the two modes that have a skip)
    T* op = out + base;
    const InormGeom g = inorm_geom(xp, hw, vec);
    const float n = (float)hw;
    float m[NP], c[2 * NP];
    inorm_stream_sums(xp, g, m[0], c[0], c[1]);
    if (TWO) inorm_stream_sums(kp, g, m[NP - 1], c[2 * NP - 2], c[2 * NP - 1]);
    inorm_block_sum<INORM_MAX_THREADS, 2 * NP>(c, red);       // (its barrier also orders every first read before any write of out == x)
    float mean, rstd, kmean = 0.f, krstd = 1.f;
    norm_finish(m[0], c[0], c[1], n, eps, mean, rstd);
    if (TWO) norm_finish(m[NP - 1], c[2 * NP - 2], c[2 * NP - 1], n, eps, kmean, krstd);
    const bool has_skip = TWO || mode == INORM_RELU_ADD_RELU;
    if (g.vec) {
        for (uint32_t i = threadIdx.x; i < g.nvec; i += INORM_MAX_THREADS) {
            const uint32_t at = g.head + 4 * i;
            const float4 q = ld4(xp + at);
            float4 k = make_float4(0.f, 0.f, 0.f, 0.f);
            if (has_skip) k = ld4(kp + at);
            if (TWO) { k.x = (k.x - kmean) * krstd; k.y = (k.y - kmean) * krstd; k.z = (k.z - kmean) * krstd; k.w = (k.w - kmean) * krstd; }
            float4 o;
            o.x = inorm_apply(mode, (q.x - mean) * rstd, k.x);
            o.y = inorm_apply(mode, (q.y - mean) * rstd, k.y);
            o.z = inorm_apply(mode, (q.z - mean) * rstd, k.z);
            o.w = inorm_apply(mode, (q.w - mean) * rstd, k.w);
            st4(op + at, o);
        }
        if (threadIdx.x < g.head + g.tail) {
            const uint32_t at = inorm_edge_index(g, threadIdx.x);
            float k = has_skip ? ld(kp + at) : 0.f;
            if (TWO) k = (k - kmean) * krstd;
            st(op + at, inorm_apply(mode, (ld(xp + at) - mean) * rstd, k));
        }
    } else {
        for (uint32_t i = threadIdx.x; i < g.hw; i += INORM_MAX_THREADS) {
            float k = has_skip ? ld(kp + i) : 0.f;
            if (TWO) k = (k - kmean) * krstd;
            st(op + i, inorm_apply(mode, (ld(xp + i) - mean) * rstd, k));
        }
    }
}

// the workgroup shapes of the resident path: {threads, vectors per thread}; capacity 4 * threads * vectors elements
static long long inorm_resident_max(int mode) { return mode == INORM_RELU_ADDNORM_RELU ? INORM_RESIDENT_MAX_TWO : INORM_RESIDENT_MAX_ONE; }

template <typename T>
static hipError_t launch_inorm(hipStream_t s, const T* x, const T* skip, T* out, uint32_t planes, uint32_t hw, int mode, float eps)
{
    // the vector form needs every operand on the same offset from the 4-element grid (the plane offsets are common to all of them)
    const uintptr_t grid = 4 * sizeof(T) - 1;
    const bool has_skip = mode == INORM_RELU_ADD_RELU || mode == INORM_RELU_ADDNORM_RELU;
    const int vec = (((uintptr_t)x ^ (uintptr_t)out) & grid) == 0 && (!has_skip || (((uintptr_t)x ^ (uintptr_t)skip) & grid) == 0);
    const dim3 g(planes);
#define INORM_RES(THREADS, NV, TWO) hipLaunchKernelGGL((inorm_resident_kernel<T, THREADS, NV, TWO>), g, dim3(THREADS), 0, s, x, skip, out, hw, mode, eps)
    if (!vec) {                                                // (rare: slices on different offsets; the streamed kernel has the scalar form)
        if (mode == INORM_RELU_ADDNORM_RELU) hipLaunchKernelGGL((inorm_streamed_kernel<T, true>), g, dim3(INORM_MAX_THREADS), 0, s, x, skip, out, hw, mode, 0, eps);
        else hipLaunchKernelGGL((inorm_streamed_kernel<T, false>), g, dim3(INORM_MAX_THREADS), 0, s, x, skip, out, hw, mode, 0, eps);
    } else if (mode == INORM_RELU_ADDNORM_RELU) {
        if (hw <= 1024) INORM_RES(64, 4, true);
        else if (hw <= 4096) INORM_RES(256, 4, true);
        else if (hw <= 16384) INORM_RES(1024, 4, true);
        else if (hw <= INORM_RESIDENT_MAX_TWO) INORM_RES(1024, 8, true);
        else hipLaunchKernelGGL((inorm_streamed_kernel<T, true>), g, dim3(INORM_MAX_THREADS), 0, s, x, skip, out, hw, mode, 1, eps);
    } else {
        if (hw <= 1024) INORM_RES(64, 4, false);
        else if (hw <= 4096) INORM_RES(256, 4, false);
        else if (hw <= 16384) INORM_RES(256, 16, false);
        else if (hw <= INORM_RESIDENT_MAX_ONE) INORM_RES(1024, 16, false);
        else hipLaunchKernelGGL((inorm_streamed_kernel<T, false>), g, dim3(INORM_MAX_THREADS), 0, s, x, skip, out, hw, mode, 1, eps);
    }
#undef INORM_RES
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (3) feature_add_position
// ---------------------------------------------------------------------------------------------------------------------------------
// s(i, p, L) = f(p / (L + 1e-6) * 2 pi / 10000^(2 floor(i / 2) / n)), f = sin for even i, cos for odd i; every step in float32, in the
// reference's order (position.py:35-44), with the accurate sinf / cosf
__device__ __forceinline__ float posadd_value(int i, float dim, int p, int L)
{
    const float a = ((float)p / ((float)L + 1e-6f)) * 6.283185307179586f / dim;
    return (i & 1) ? cosf(a) : sinf(a);
}

// V consecutive elements of one row per thread (V = 4 needs W % 4 == 0 and aligned operands); out0 == f0 and out1 == f1 are allowed
template <typename T, int V>
__global__ void __launch_bounds__(POSADD_THREADS)
position_add_kernel(const T* f0, const T* f1, T* out0, T* out1, int C, int W, uint32_t hw, int wh, int ww, uint32_t chunks)
{
    const uint32_t plane = blockIdx.x / chunks, chunk = blockIdx.x - plane * chunks;
    const uint32_t el = (chunk * POSADD_THREADS + threadIdx.x) * V;
    if (el >= hw) return;                                      // (hw is a multiple of V: no partial group)
    const int c = (int)(plane % (uint32_t)C), n = C >> 1;
    const bool along_y = c < n;
    const int i = along_y ? c : c - n;
    const float dim = powf(10000.f, (float)(2 * (i >> 1)) / (float)n);
    const uint32_t y = el / (uint32_t)W, x0 = el - y * (uint32_t)W;
    float add[V];
    if (along_y) {
        const float a = posadd_value(i, dim, (int)(y % (uint32_t)wh) + 1, wh);
#pragma unroll
        for (int k = 0; k < V; k++) add[k] = a;
    } else {
#pragma unroll
        for (int k = 0; k < V; k++) add[k] = posadd_value(i, dim, (int)((x0 + k) % (uint32_t)ww) + 1, ww);
    }
    const size_t at = (size_t)plane * hw + el;
    if (V == 4) {
        float4 a = ld4(f0 + at), b = ld4(f1 + at);
        a.x += add[0]; a.y += add[1]; a.z += add[2]; a.w += add[3];
        b.x += add[0]; b.y += add[1]; b.z += add[2]; b.w += add[3];
        st4(out0 + at, a);
        st4(out1 + at, b);
    } else {
        st(out0 + at, ld(f0 + at) + add[0]);
        st(out1 + at, ld(f1 + at) + add[0]);
    }
}

template <typename T>
static hipError_t launch_position_add(hipStream_t s, const T* f0, const T* f1, T* out0, T* out1, uint32_t planes, int C, int H, int W, int splits)
{
    const uint32_t hw = (uint32_t)H * (uint32_t)W;
    const uintptr_t grid = 4 * sizeof(T) - 1;
    const bool v4 = (W & 3) == 0 && ((((uintptr_t)f0) | ((uintptr_t)f1) | ((uintptr_t)out0) | ((uintptr_t)out1)) & grid) == 0;
    const uint32_t per = POSADD_THREADS * (v4 ? 4 : 1), chunks = (hw + per - 1) / per;
    const dim3 g(planes * chunks), blk(POSADD_THREADS);
    if (v4) hipLaunchKernelGGL((position_add_kernel<T, 4>), g, blk, 0, s, f0, f1, out0, out1, C, W, hw, H / splits, W / splits, chunks);
    else hipLaunchKernelGGL((position_add_kernel<T, 1>), g, blk, 0, s, f0, f1, out0, out1, C, W, hw, H / splits, W / splits, chunks);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the entry points (the contract is in include/igs_rast.h)
// ---------------------------------------------------------------------------------------------------------------------------------
static bool inorm_mode_ok(int mode) { return mode >= INORM_PLAIN && mode <= INORM_RELU_ADDNORM_RELU; }
// [a, a + bytes) and [b, b + bytes) share a byte without being the same range
static bool inorm_partial_overlap(const void* a, const void* b, size_t bytes) { return a != b && spans_overlap(byte_span(a, bytes), byte_span(b, bytes)); }

extern "C" long long igs_instance_norm_resident_max(int dtype, int mode)
{
    if (!dtype_ok(dtype) || !inorm_mode_ok(mode)) return 0;
    return inorm_resident_max(mode);
}

extern "C" int igs_instance_norm_fwd(void* stream, const void* x, const void* skip, void* out, long long planes, long long hw, int dtype, int mode,
                                     float eps)
{
    const char* fn = "igs_instance_norm_fwd";
    if (!dtype_ok(dtype)) return fail_in(fn, "unknown dtype code");
    if (!inorm_mode_ok(mode)) return fail_in(fn, "unknown mode");
    if (hw < 2) return fail_in(fn, "hw < 2: an instance norm needs more than 1 spatial element");
    if (hw > IGS_INORM_MAX_HW) return fail_in(fn, "hw out of range (IGS_INORM_MAX_HW)");
    if (planes < 0 || planes > IGS_INORM_MAX_PLANES) return fail_in(fn, "planes out of range (0..IGS_INORM_MAX_PLANES)");
    if (!eps_ok(eps)) return fail_in(fn, "eps must be finite and >= 0");
    if (planes == 0) return 0;
    const bool has_skip = mode == INORM_RELU_ADD_RELU || mode == INORM_RELU_ADDNORM_RELU;
    if (!x || !out) return fail_in(fn, "NULL pointer");
    if (has_skip && !skip) return fail_in(fn, "NULL pointer (this mode needs skip)");
    const size_t es = dtype_bytes(dtype), bytes = (size_t)planes * (size_t)hw * es;
    if ((((uintptr_t)x) | ((uintptr_t)out) | (has_skip ? (uintptr_t)skip : 0)) & (es - 1)) return fail_in(fn, "a pointer is not aligned to its element size");
    if (inorm_partial_overlap(x, out, bytes)) return fail_in(fn, "out overlaps x without being x (only out == x may alias)");
    if (has_skip && (skip == (const void*)out || inorm_partial_overlap(skip, out, bytes))) return fail_in(fn, "out overlaps skip (only out == x may alias)");
    hipError_t e;
    if (dtype == IGS_DTYPE_F16)
        e = launch_inorm((hipStream_t)stream, (const _Float16*)x, (const _Float16*)skip, (_Float16*)out, (uint32_t)planes, (uint32_t)hw, mode, eps);
    else
        e = launch_inorm((hipStream_t)stream, (const float*)x, (const float*)skip, (float*)out, (uint32_t)planes, (uint32_t)hw, mode, eps);
    HIP_TRY(e, "instance norm launch");
    return 0;
}

extern "C" int igs_position_add(void* stream, const void* f0, const void* f1, void* out0, void* out1, int B, int C, int H, int W, int splits, int dtype)
{
    const char* fn = "igs_position_add";
    if (!dtype_ok(dtype)) return fail_in(fn, "unknown dtype code");
    if (B < 0 || C < 1 || H < 1 || W < 1) return fail_in(fn, "B, C, H, W out of range");
    if (C % 4 != 0) return fail_in(fn, "C must be a multiple of 4 (sine and cosine pairs for y and for x)");
    if (splits < 1) return fail_in(fn, "splits must be >= 1");
    if (H % splits != 0 || W % splits != 0) return fail_in(fn, "H and W must be multiples of splits");
    if ((long long)H * W > IGS_INORM_MAX_HW) return fail_in(fn, "H * W out of range (IGS_INORM_MAX_HW)");
    const long long planes = (long long)B * C, chunks = ((long long)H * W + POSADD_THREADS - 1) / POSADD_THREADS;
    if (planes * chunks > IGS_INORM_MAX_PLANES) return fail_in(fn, "B * C * H * W out of range");
    if (B == 0) return 0;
    if (!f0 || !f1 || !out0 || !out1) return fail_in(fn, "NULL pointer");
    const size_t es = dtype_bytes(dtype), bytes = (size_t)planes * H * W * es;
    if ((((uintptr_t)f0) | ((uintptr_t)f1) | ((uintptr_t)out0) | ((uintptr_t)out1)) & (es - 1)) return fail_in(fn, "a pointer is not aligned to its element size");
    if (inorm_partial_overlap(f0, out0, bytes) || inorm_partial_overlap(f1, out1, bytes) || out0 == out1 || inorm_partial_overlap(out0, out1, bytes) ||
        (const void*)out0 == f1 || inorm_partial_overlap(f1, out0, bytes) || (const void*)out1 == f0 || inorm_partial_overlap(f0, out1, bytes))
        return fail_in(fn, "the outputs overlap (only out0 == f0 and out1 == f1 may alias)");
    hipError_t e;
    if (dtype == IGS_DTYPE_F16)
        e = launch_position_add((hipStream_t)stream, (const _Float16*)f0, (const _Float16*)f1, (_Float16*)out0, (_Float16*)out1, (uint32_t)planes, C, H, W, splits);
    else
        e = launch_position_add((hipStream_t)stream, (const float*)f0, (const float*)f1, (float*)out0, (float*)out1, (uint32_t)planes, C, H, W, splits);
    HIP_TRY(e, "position add launch");
    return 0;
}
