// densify.hip -- the densify-and-prune decision of the refine loop on the device (igs/models/gaussian_model.py:586-663 as restated by
// igs_amd/densify.py: plan): candidate selection, max-points bound, clone / split classification, split children, opacity and
// world-size prune, and the output rows in the order of the reference's cat / mask sequence.  include/igs_rast.h states the contract,
// DESIGN.md section 23 the design and the figures.
//
// Launches of one igs_densify_plan call: 9 with the max-points bound armed (control_max != 0), 4 without.
//   1  zero-fill of the four 256-bin histograms                                                        (bound only)
//   2  classify: g = accum / denom, key = bits(g) of a candidate (else 0), the flag byte {big, opacity ok, world size ok of the row
//      and of its children}; histogram of the keys' top byte
//   3-5  histogram of the next byte over the keys that share the cut's prefix so far                   (bound only)
//   6  per-block count of the keys equal to the cut                                                    (bound only)
//   7  admit (key > cut, or key == cut among the first r such keys by index), per-block counts of the row kinds
//   8  the library's exclusive scan over one array of six segments: surviving originals | surviving clones | surviving children
//      (c = 0) | the same again (c = 1) | split sources | clones.  The segments lie in output order, so a scanned entry IS the first
//      output row of its block, the entry behind the fourth segment is P_new, and the last two give n_split and n_clone.
//   9  emit: rows {src, fresh, ovr}, the children of every split source, the four counts
// The cut is never stored: every block of launches 3-7 derives it again from the finished histograms (one 256-lane suffix scan per
// level), so no launch needs a "last block finishes" hand-off and no kernel here contains a fence.  Whether the bound applies
// (candidates > max_num_add) is decided by the same code on the device; launches 3-6 return at once when it does not.
// Order comes from the scans only; the atomics add integers into histograms, whose sums do not depend on the order.  Two runs give
// identical bits.  Non-negative floats order as their bit patterns, so the select works on the keys as unsigned integers.
#include "common.h"
#include "host_api.h"
#include <math.h>

#define DP_BIG 1u          // largest scale > split_scale_limit
#define DP_OPA_OK 2u       // not pruned for opacity
#define DP_SELF_OK 4u      // the row itself (original or clone) passes the world-size test
#define DP_CHILD_OK 8u     // its split children pass it
#define DP_CAND 16u        // admitted candidate (set by launch 7)
#define DP_MAX_POINTS (1 << 28)      // row positions and the scanned sums stay inside 32 bits

struct PlanLayout {        // byte offsets from a 256-byte aligned base
    size_t key, flags, hist, tie, seg, total;
    int nb;
    explicit PlanLayout(int P) {
        nb = (P + 255) / 256;
        size_t o = 0;
        key = o;   o += align_up((size_t)P * 4, 256);
        flags = o; o += align_up((size_t)P, 256);
        hist = o;  o += 4 * 256 * 4;
        tie = o;   o += align_up((size_t)nb * 4, 256);
        seg = o;   o += align_up(((size_t)6 * nb + 1) * 4, 256);
        total = o + 256;
    }
};

// max that keeps a NaN, as torch.max does
__device__ __forceinline__ float max_nan(float m, float a) { return (a > m || a != a) ? a : m; }

__global__ void __launch_bounds__(256)
plan_classify_kernel(int P, const float* __restrict__ opacity_logit, const float* __restrict__ log_scale,
                     const float* __restrict__ grad_accum, const float* __restrict__ denom, float grad_threshold, float min_opacity,
                     float split_scale_limit, float world_scale_limit, uint32_t* __restrict__ key, uint8_t* __restrict__ flags,
                     uint32_t* __restrict__ sel_hist0)
{
    __shared__ uint32_t h[256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (sel_hist0) { h[threadIdx.x] = 0u; __syncthreads(); }
    if (i < P) {
        float g = grad_accum[i] / denom[i];
        if (!(g > 0.f)) g = 0.f;                                   // 0/0, and the negative values the statistics cannot take
        const uint32_t k = g >= grad_threshold ? __float_as_uint(g) : 0u;
        const float s0 = expf(log_scale[3 * (size_t)i]), s1 = expf(log_scale[3 * (size_t)i + 1]), s2 = expf(log_scale[3 * (size_t)i + 2]);
        const float smax = max_nan(max_nan(s0, s1), s2);
        // a child's scale as the prune of `plan` sees it: exp of the stored log(s / 1.6)
        const float cmax = max_nan(max_nan(expf(logf(s0 / 1.6f)), expf(logf(s1 / 1.6f))), expf(logf(s2 / 1.6f)));
        const float opa = 1.0f / (1.0f + expf(-opacity_logit[i]));
        uint32_t f = 0u;
        if (smax > split_scale_limit) f |= DP_BIG;
        if (!(opa < min_opacity)) f |= DP_OPA_OK;
        if (!(world_scale_limit > 0.f && smax > world_scale_limit)) f |= DP_SELF_OK;
        if (!(world_scale_limit > 0.f && cmax > world_scale_limit)) f |= DP_CHILD_OK;
        key[i] = k;
        flags[i] = (uint8_t)f;
        if (sel_hist0 && k) atomicAdd(&h[k >> 24], 1u);
    }
    if (sel_hist0) {
        __syncthreads();
        if (h[threadIdx.x]) atomicAdd(&sel_hist0[threadIdx.x], h[threadIdx.x]);
    }
}

// The cut of the max-points bound from the first `levels` histograms, by all 256 threads of a block (the result is block-uniform).
//   bounded == false: the candidates fit (or fewer exist than the bound): every key != 0 stays  -> T = 0, r = 0
//   bounded, max_num_add <= 0: none stay                                                        -> T = 0xFFFFFFFF, r = 0
//   else: T = the top 8 * levels bits of the k-th largest key, r = how many keys with that prefix stay (levels == 4: T is the cut
//   itself, keys above it stay, and r >= 1 of the keys equal to it)
struct Cut { uint32_t T, r; bool bounded; };
__device__ __forceinline__ Cut resolve_cut(const uint32_t* __restrict__ hist, int levels, long long max_num_add, uint32_t* sh /* 8 words */)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6, d = 255u - tid;      // descending digits: a suffix sum as a prefix scan
    Cut c; c.T = 0u; c.r = 0u; c.bounded = false;
    uint32_t k = 0u;
    for (int l = 0; l < levels; l++) {
        const uint32_t hv = hist[l * 256 + d];
        uint32_t incl = hv;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const uint32_t t = __shfl_up(incl, off, 64); if (lane >= (uint32_t)off) incl += t; }
        if (lane == 63u) sh[wid] = incl;
        __syncthreads();
        const uint32_t total = sh[0] + sh[1] + sh[2] + sh[3];
        for (uint32_t w = 0; w < wid; w++) incl += sh[w];
        const uint32_t excl = incl - hv;
        __syncthreads();                                                                // sh[0..3] are read: the caller may reuse them after a return
        if (l == 0) {
            if ((long long)total <= max_num_add) return c;                              // (uniform: every thread holds the same total)
            c.bounded = true;
            if (max_num_add <= 0) { c.T = 0xFFFFFFFFu; return c; }
            k = (uint32_t)max_num_add;                                                  // 1 <= k < total
        }
        if (excl < k && k <= incl) { sh[4] = d; sh[5] = k - excl; }                     // exactly one thread
        __syncthreads();
        c.T = (c.T << 8) | sh[4];
        k = sh[5];
        __syncthreads();
    }
    c.r = k;
    return c;
}

// level l in 1..3: histogram of byte (3 - l) over the keys whose top l bytes equal the cut's
__global__ void __launch_bounds__(256)
plan_hist_kernel(int P, const uint32_t* __restrict__ key, uint32_t* __restrict__ hist, int l, long long max_num_add)
{
    __shared__ uint32_t h[256];
    __shared__ uint32_t sh[8];
    const Cut c = resolve_cut(hist, l, max_num_add, sh);
    if (!c.bounded || c.r == 0u) return;
    h[threadIdx.x] = 0u;
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < P) {
        const uint32_t k = key[i];
        if (k && (k >> (32 - 8 * l)) == c.T) atomicAdd(&h[(k >> (24 - 8 * l)) & 255u], 1u);
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&hist[l * 256 + threadIdx.x], h[threadIdx.x]);
}

// number of set flags in the block, returned to every thread; ws: 4 words
__device__ __forceinline__ uint32_t block_count(bool f, uint32_t* ws)
{
    const uint64_t m = __ballot(f);
    if ((threadIdx.x & 63u) == 0u) ws[threadIdx.x >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    const uint32_t n = ws[0] + ws[1] + ws[2] + ws[3];
    __syncthreads();
    return n;
}
// rank of a set flag among the block's set flags in thread order; ws: 4 words
__device__ __forceinline__ uint32_t block_rank(bool f, uint32_t* ws)
{
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    const uint64_t m = __ballot(f);
    if (lane == 0u) ws[wid] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t r = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    for (uint32_t w = 0; w < wid; w++) r += ws[w];
    __syncthreads();
    return r;
}

__global__ void __launch_bounds__(256)
plan_tie_kernel(int P, const uint32_t* __restrict__ key, const uint32_t* __restrict__ hist, long long max_num_add, uint32_t* __restrict__ tie)
{
    __shared__ uint32_t sh[8];
    const Cut c = resolve_cut(hist, 4, max_num_add, sh);
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool t = c.bounded && c.r > 0u && i < P && key[i] == c.T;
    const uint32_t n = block_count(t, sh);
    if (threadIdx.x == 0) tie[blockIdx.x] = n;
}

__device__ __forceinline__ void row_kinds(bool valid, uint32_t f, bool& orig, bool& clone_s, bool& child_s, bool& split, bool& clone)
{
    const bool cand = (f & DP_CAND) != 0u, big = (f & DP_BIG) != 0u, opa = (f & DP_OPA_OK) != 0u;
    split = valid && cand && big;
    clone = valid && cand && !big;
    orig = valid && !split && opa && (f & DP_SELF_OK);
    clone_s = clone && opa && (f & DP_SELF_OK);
    child_s = split && opa && (f & DP_CHILD_OK);
}

__global__ void __launch_bounds__(256)
plan_count_kernel(int P, int nb, const uint32_t* __restrict__ key, uint8_t* __restrict__ flags, const uint32_t* __restrict__ hist,
                  long long max_num_add, const uint32_t* __restrict__ tie, uint32_t* __restrict__ seg)
{
    __shared__ uint32_t sh[8];
    __shared__ uint32_t cnt[5];
    Cut c; c.T = 0u; c.r = 0u; c.bounded = false;
    if (hist) c = resolve_cut(hist, 4, max_num_add, sh);
    const int i = blockIdx.x * 256 + threadIdx.x;
    const uint32_t k = i < P ? key[i] : 0u;
    bool cand = k > c.T;
    if (c.bounded && c.r > 0u) {
        const bool t = i < P && k == c.T;
        if (__syncthreads_or(t)) {                                 // ties at the cut: the lowest indices are admitted
            uint32_t part = 0u;
            for (int j = threadIdx.x; j < (int)blockIdx.x; j += 256) part += tie[j];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) part += __shfl_down(part, off, 64);
            if ((threadIdx.x & 63u) == 0u) sh[threadIdx.x >> 6] = part;
            __syncthreads();
            const uint32_t base = sh[0] + sh[1] + sh[2] + sh[3];
            __syncthreads();
            const uint32_t rank = block_rank(t, sh);
            if (t && (unsigned long long)base + rank < (unsigned long long)c.r) cand = true;
        }
    }
    uint32_t f = 0u;
    if (i < P) {
        f = flags[i] | (cand ? DP_CAND : 0u);
        flags[i] = (uint8_t)f;
    }
    bool kind[5];
    row_kinds(i < P, f, kind[0], kind[1], kind[2], kind[3], kind[4]);
#pragma unroll
    for (int q = 0; q < 5; q++) {
        const uint32_t n = block_count(kind[q], sh);
        if (threadIdx.x == 0) cnt[q] = n;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int q = threadIdx.x < 3 ? threadIdx.x : threadIdx.x - 1;      // segments: orig, clone_s, child_s, child_s, split, clone
        seg[(size_t)threadIdx.x * nb + blockIdx.x] = cnt[q];
    }
    if (blockIdx.x == 0 && threadIdx.x == 6) seg[(size_t)6 * nb] = 0u;
}

__global__ void __launch_bounds__(256)
plan_emit_kernel(int P, int nb, const float* __restrict__ xyz, const float* __restrict__ rotation, const float* __restrict__ log_scale,
                 const float* __restrict__ normals, const uint8_t* __restrict__ flags, const uint32_t* __restrict__ seg,
                 int* __restrict__ src, int* __restrict__ fresh, int* __restrict__ ovr, float* __restrict__ ovr_xyz,
                 float* __restrict__ ovr_scale, int* __restrict__ counts)
{
    __shared__ uint32_t sh[8];
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.x;
    const uint32_t f = i < P ? flags[i] : 0u;
    bool orig, clone_s, child_s, split, clone;
    row_kinds(i < P, f, orig, clone_s, child_s, split, clone);
    const uint32_t r_orig = block_rank(orig, sh), r_clone = block_rank(clone_s, sh), r_child = block_rank(child_s, sh), r_split = block_rank(split, sh);
    const uint32_t P_new = seg[(size_t)4 * nb], n_split = seg[(size_t)5 * nb] - P_new, n_clone = seg[(size_t)6 * nb] - seg[(size_t)5 * nb];
    if (b == 0 && threadIdx.x == 0) {
        counts[0] = (int)P_new; counts[1] = (int)n_clone; counts[2] = (int)n_split;
        counts[3] = (int)((uint32_t)P + n_clone + n_split - P_new);
    }
    if (orig) { const uint32_t o = seg[b] + r_orig; src[o] = i; fresh[o] = 0; ovr[o] = -1; }
    if (clone_s) { const uint32_t o = seg[(size_t)nb + b] + r_clone; src[o] = i; fresh[o] = 1; ovr[o] = -1; }
    if (split) {
        const uint32_t j = seg[(size_t)4 * nb + b] - P_new + r_split;                   // rank among the split sources
        const float s[3] = { expf(log_scale[3 * (size_t)i]), expf(log_scale[3 * (size_t)i + 1]), expf(log_scale[3 * (size_t)i + 2]) };
        const float q0 = rotation[4 * (size_t)i], q1 = rotation[4 * (size_t)i + 1], q2 = rotation[4 * (size_t)i + 2], q3 = rotation[4 * (size_t)i + 3];
        const float n = sqrtf(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);                   // build_rotation: q / |q|, no epsilon
        const float r = q0 / n, x = q1 / n, y = q2 / n, z = q3 / n;
        const float R[3][3] = { { 1.f - 2.f * (y * y + z * z), 2.f * (x * y - r * z), 2.f * (x * z + r * y) },
                                { 2.f * (x * y + r * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z - r * x) },
                                { 2.f * (x * z - r * y), 2.f * (y * z + r * x), 1.f - 2.f * (x * x + y * y) } };
        const float px = xyz[3 * (size_t)i], py = xyz[3 * (size_t)i + 1], pz = xyz[3 * (size_t)i + 2];
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const size_t row = (size_t)c * n_split + j;
            float v[3] = { 0.f, 0.f, 0.f };
            if (normals) {
#pragma unroll
                for (int a = 0; a < 3; a++) v[a] = normals[((size_t)i * 2 + c) * 3 + a] * s[a];
            }
            ovr_xyz[3 * row] = R[0][0] * v[0] + R[0][1] * v[1] + R[0][2] * v[2] + px;
            ovr_xyz[3 * row + 1] = R[1][0] * v[0] + R[1][1] * v[1] + R[1][2] * v[2] + py;
            ovr_xyz[3 * row + 2] = R[2][0] * v[0] + R[2][1] * v[1] + R[2][2] * v[2] + pz;
#pragma unroll
            for (int a = 0; a < 3; a++) ovr_scale[3 * row + a] = logf(s[a] / 1.6f);
            if (child_s) {
                const uint32_t o = seg[(size_t)(2 + c) * nb + b] + r_child;
                src[o] = i; fresh[o] = 1; ovr[o] = (int)row;
            }
        }
    }
}

// the entry points (the contracts are in include/igs_rast.h)
extern "C" size_t igs_densify_plan_scratch_bytes(int P)
{
    if (P < 0 || P > DP_MAX_POINTS) return 0;
    return PlanLayout(P).total;
}
extern "C" int igs_densify_plan(void* stream, int P, const float* xyz, const float* rotation, const float* opacity_logit,
                                const float* log_scale, const float* grad_accum, const float* denom, const float* normals,
                                float grad_threshold, float min_opacity, float split_scale_limit, float world_scale_limit,
                                long long max_num_add, int control_max, void* scratch, int* src, int* fresh, int* ovr, float* ovr_xyz,
                                float* ovr_scale, int* counts)
{
    if (P < 0 || P > DP_MAX_POINTS) return fail_in("igs_densify_plan", "P out of range");
    if (!(grad_threshold > 0.f) || !(grad_threshold < INFINITY)) return fail_in("igs_densify_plan", "grad_threshold must be finite and > 0");
    if (P == 0) return 0;
    if (!xyz || !rotation || !opacity_logit || !log_scale || !grad_accum || !denom || !scratch || !src || !fresh || !ovr || !ovr_xyz ||
        !ovr_scale || !counts)
        return fail_in("igs_densify_plan", "NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    const PlanLayout L(P);
    char* base = align_ptr((const char*)scratch);
    uint32_t* key = (uint32_t*)(base + L.key);
    uint8_t* flags = (uint8_t*)(base + L.flags);
    uint32_t* hist = control_max ? (uint32_t*)(base + L.hist) : nullptr;
    uint32_t* tie = (uint32_t*)(base + L.tie);
    uint32_t* seg = (uint32_t*)(base + L.seg);
    const dim3 grid(L.nb), block(256);
    if (hist) HIP_TRY(zero_fill_async(s, hist, 4 * 256 * 4), "densify plan: histogram zero-fill");
    hipLaunchKernelGGL(plan_classify_kernel, grid, block, 0, s, P, opacity_logit, log_scale, grad_accum, denom, grad_threshold, min_opacity,
                       split_scale_limit, world_scale_limit, key, flags, hist);
    if (hist) {
        for (int l = 1; l < 4; l++) hipLaunchKernelGGL(plan_hist_kernel, grid, block, 0, s, P, (const uint32_t*)key, hist, l, max_num_add);
        hipLaunchKernelGGL(plan_tie_kernel, grid, block, 0, s, P, (const uint32_t*)key, (const uint32_t*)hist, max_num_add, tie);
    }
    hipLaunchKernelGGL(plan_count_kernel, grid, block, 0, s, P, L.nb, (const uint32_t*)key, flags, (const uint32_t*)hist, max_num_add,
                       (const uint32_t*)tie, seg);
    HIP_TRY(hipGetLastError(), "densify plan: count launches");
    HIP_TRY(launch_exclusive_scan(s, 6 * L.nb + 1, seg), "densify plan: scan launch");
    hipLaunchKernelGGL(plan_emit_kernel, grid, block, 0, s, P, L.nb, xyz, rotation, log_scale, normals, (const uint8_t*)flags,
                       (const uint32_t*)seg, src, fresh, ovr, ovr_xyz, ovr_scale, counts);
    HIP_TRY(hipGetLastError(), "densify plan: emit launch");
    return 0;
}
