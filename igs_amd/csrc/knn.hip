// knn.hip -- simple-knn's distCUDA2 for gfx950: for every point, the mean of its three smallest squared distances to the other points
// (include/igs_rast.h: igs_knn_mean_dist2 states the contract).  Exact search over a Morton-sorted copy of the cloud, pruned by boxes.
//
// Five phases, one launch each (the launch boundary is the only hand-off between workgroups; no fence; LDS only for one histogram):
//   1. bounding box of the finite points: one partial per wave, then one wave folds the partials (device memory, no read-back);
//   2. 63-bit Morton keys (21 bits per axis) sorted by the library's stable LSD radix sort in two rounds: low 32 bits, then high 31
//      bits -- together a stable sort on the full key.  21 bits per axis keep clustered clouds with far outliers (COLMAP sky points)
//      from collapsing onto a few keys, which the 10-bit key of igs_morton_order would do;
//   3. gather: the sorted points into a padded float4 array (non-finite points and the padding become (+inf, +inf, +inf)), one leaf
//      box per 64 consecutive sorted points (one wave) over its finite points;
//   4. node boxes: one per 64 leaves;
//   5. query: one wave per leaf, one query per lane, best[3] in registers.  The wave seeds from its own leaf, then visits its own
//      node, then sweeps all nodes: 64 node boxes per step against the box of the wave's queries and the wave's largest best[2], then
//      each surviving node against every lane's own query and best[2]; in a node that some lane can gain from, its 64 leaf boxes the
//      same two ways, and a leaf some lane can gain from is visited.  A visited leaf's index is wave-uniform, so its 64 candidates come in through
//      scalar loads and every lane tests all of them against SGPR operands.
//
// Exactness: every candidate distance -- seed or search -- is dist2(q, c) below, one expression of q - c.  A box is skipped only when
// its box distance, computed with the same expression from per-axis gaps, is >= the bound it is compared to: per axis the gap
// lo - q (or q - hi) is at most |c - q| for every c in the box before rounding, rounding is monotone, and so are the square and the
// fused sums, so the float box distance never exceeds a float candidate distance.  A candidate >= best[2] cannot change the three
// smallest values.  The result is the same multiset of three values whatever the visiting order, hence bit-identical from run to run
// and under any permutation of the input.
#include "common.h"
#include "knn_common.h"
#include "host_api.h"
#include <float.h>

#define KNN_K 3                    // neighbours averaged (simple-knn: best[3]); the insertion below is written for 3
static_assert(KNN_K == 3, "knn_insert keeps exactly three values");

// scratch layout (offsets from a 256-byte aligned base)
struct KnnLayout {
    size_t lohi, part, pts, leaf, node, total;
    RadixOffsets sort;                 // two rounds: two adjacent histogram blocks
    int L, Nn;
    explicit KnnLayout(int P) {
        const size_t n = (size_t)(P > 0 ? P : 0);
        L = (int)((n + 63) / 64); Nn = (L + 63) / 64;
        size_t o = 0;
        lohi = o;  o += 256;
        part = o;  o += align_up((size_t)KNN_BBOX_PARTS * 8 * 4, 256);
        sort = radix_layout_append(o, n, 2);
        pts = o;   o += align_up((size_t)L * 64 * 16, 256);
        leaf = o;  o += align_up((size_t)L * 32, 256);
        node = o;  o += align_up((size_t)Nn * 32, 256);
        total = o + 256;
    }
};

// lower bound of dist2(q, c) over q in box a, c in box b
__device__ __forceinline__ float boxbox_dist2(const float4& alo, const float4& ahi, const float4& blo, const float4& bhi)
{
    const float gx = fmaxf(fmaxf(blo.x - ahi.x, alo.x - bhi.x), 0.f);
    const float gy = fmaxf(fmaxf(blo.y - ahi.y, alo.y - bhi.y), 0.f);
    const float gz = fmaxf(fmaxf(blo.z - ahi.z, alo.z - bhi.z), 0.f);
    return __fmaf_rn(gz, gz, __fmaf_rn(gy, gy, __fmul_rn(gx, gx)));
}
// d into the sorted b0 <= b1 <= b2 (d never NaN for a finite query: candidates are finite or +inf)
__device__ __forceinline__ void knn_insert(float d, float& b0, float& b1, float& b2)
{
    b2 = __builtin_amdgcn_fmed3f(b1, d, b2);
    b1 = __builtin_amdgcn_fmed3f(b0, d, b1);
    b0 = fminf(b0, d);
}

// ---- phase 1: bounding box of the finite points (empty: lo = +inf, hi = -inf) ----
__global__ void __launch_bounds__(64)
knn_bbox_partial_kernel(int P, const float* __restrict__ xyz, float* __restrict__ part)
{
    float lx = INFINITY, ly = INFINITY, lz = INFINITY, hx = -INFINITY, hy = -INFINITY, hz = -INFINITY;
    for (int i = blockIdx.x * 64 + threadIdx.x; i < P; i += gridDim.x * 64) {
        const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
        if (finite3(x, y, z)) { lx = fminf(lx, x); ly = fminf(ly, y); lz = fminf(lz, z); hx = fmaxf(hx, x); hy = fmaxf(hy, y); hz = fmaxf(hz, z); }
    }
    lx = wave_min(lx); ly = wave_min(ly); lz = wave_min(lz); hx = wave_max(hx); hy = wave_max(hy); hz = wave_max(hz);
    if (threadIdx.x == 0) {
        float* o = part + 8 * (size_t)blockIdx.x;
        o[0] = lx; o[1] = ly; o[2] = lz; o[3] = hx; o[4] = hy; o[5] = hz;
    }
}
__global__ void __launch_bounds__(64)
knn_bbox_final_kernel(int nparts, const float* __restrict__ part, float* __restrict__ lohi)
{
    float lx = INFINITY, ly = INFINITY, lz = INFINITY, hx = -INFINITY, hy = -INFINITY, hz = -INFINITY;
    for (int b = threadIdx.x; b < nparts; b += 64) {
        const float* p = part + 8 * (size_t)b;
        lx = fminf(lx, p[0]); ly = fminf(ly, p[1]); lz = fminf(lz, p[2]); hx = fmaxf(hx, p[3]); hy = fmaxf(hy, p[4]); hz = fmaxf(hz, p[5]);
    }
    lx = wave_min(lx); ly = wave_min(ly); lz = wave_min(lz); hx = wave_max(hx); hy = wave_max(hy); hz = wave_max(hz);
    if (threadIdx.x == 0) { lohi[0] = lx; lohi[1] = ly; lohi[2] = lz; lohi[3] = hx; lohi[4] = hy; lohi[5] = hz; }
}

// ---- phase 2: 63-bit Morton keys ----
// round 1: key bits [0, 32) with the identity as values; fills the first radix pass's per-block histogram
__global__ void __launch_bounds__(256)
knn_keys_lo_kernel(int P, const float* __restrict__ xyz, const float* __restrict__ lohi, uint32_t* __restrict__ keys,
                   uint32_t* __restrict__ vals, uint32_t* __restrict__ hist0, uint32_t per_block)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const uint32_t k = (uint32_t)knn_key(xyz, (uint32_t)i, lohi);
    keys[i] = k; vals[i] = (uint32_t)i;
    radix_count_first(hist0, (uint32_t)i, per_block, k);
}
// round 2: key bits [32, 63) of the points in round-1 order
__global__ void __launch_bounds__(256)
knn_keys_hi_kernel(int P, const float* __restrict__ xyz, const float* __restrict__ lohi, const uint32_t* __restrict__ order,
                   uint32_t* __restrict__ keys, uint32_t* __restrict__ vals, uint32_t* __restrict__ hist0, uint32_t per_block)
{
    // the high key bits are coarse: a block's keys share few digits, so they are counted in LDS first (one global add per digit)
    const int s = blockIdx.x * 256 + threadIdx.x;
    radix_count_first_lds(hist0, per_block, [&](uint32_t& k) {
        if (s >= P) return false;
        const uint32_t v = order[s];
        k = (uint32_t)(knn_key(xyz, v, lohi) >> 32);
        keys[s] = k; vals[s] = v;
        return true;
    });
}

// ---- phase 3: sorted points and leaf boxes (one wave per leaf) ----
__global__ void __launch_bounds__(256)
knn_gather_kernel(int P, int L, const float* __restrict__ xyz, const uint32_t* __restrict__ perm, float4* __restrict__ pts,
                  float4* __restrict__ leafbox)
{
    const int leaf = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (leaf >= L) return;
    const int s = leaf * 64 + lane;
    float x = INFINITY, y = INFINITY, z = INFINITY;
    if (s < P) {
        const uint32_t v = perm[s];
        x = xyz[3 * (size_t)v]; y = xyz[3 * (size_t)v + 1]; z = xyz[3 * (size_t)v + 2];
    }
    const bool fin = finite3(x, y, z);
    if (!fin) { x = INFINITY; y = INFINITY; z = INFINITY; }
    pts[s] = make_float4(x, y, z, 0.f);
    float lx = fin ? x : INFINITY, ly = fin ? y : INFINITY, lz = fin ? z : INFINITY;
    float hx = fin ? x : -INFINITY, hy = fin ? y : -INFINITY, hz = fin ? z : -INFINITY;
    lx = wave_min(lx); ly = wave_min(ly); lz = wave_min(lz); hx = wave_max(hx); hy = wave_max(hy); hz = wave_max(hz);
    if (lane == 0) { leafbox[2 * (size_t)leaf] = make_float4(lx, ly, lz, 0.f); leafbox[2 * (size_t)leaf + 1] = make_float4(hx, hy, hz, 0.f); }
}

// ---- phase 4: node boxes (one wave per 64 leaves) ----
__global__ void __launch_bounds__(256)
knn_node_kernel(int L, int Nn, const float4* __restrict__ leafbox, float4* __restrict__ nodebox)
{
    const int node = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (node >= Nn) return;
    const int l = node * 64 + lane;
    float4 lo = make_float4(INFINITY, INFINITY, INFINITY, 0.f), hi = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f);
    if (l < L) { lo = leafbox[2 * (size_t)l]; hi = leafbox[2 * (size_t)l + 1]; }
    lo.x = wave_min(lo.x); lo.y = wave_min(lo.y); lo.z = wave_min(lo.z); hi.x = wave_max(hi.x); hi.y = wave_max(hi.y); hi.z = wave_max(hi.z);
    if (lane == 0) { nodebox[2 * (size_t)node] = make_float4(lo.x, lo.y, lo.z, 0.f); nodebox[2 * (size_t)node + 1] = make_float4(hi.x, hi.y, hi.z, 0.f); }
}

// ---- phase 5: the search ----
struct KnnWave {
    float qx, qy, qz;            // this lane's query
    bool active;                 // a real, finite query
    float b0, b1, b2;            // its three smallest distances so far
    float4 qlo, qhi;             // box of the wave's active queries
    float R2;                    // max of best[2] over the active lanes (0: no active lane), refreshed after every node
};

// all 64 candidates of leaf l (wave-uniform) against every lane's query
__device__ __forceinline__ void knn_visit_leaf(KnnWave& w, const float4* __restrict__ pts, int l)
{
    const float4* c = pts + (size_t)l * 64;
#pragma unroll 8
    for (int j = 0; j < 64; j++) {
        const float4 p = c[j];
        knn_insert(dist2(w.qx, w.qy, w.qz, p.x, p.y, p.z), w.b0, w.b1, w.b2);
    }
}

// box of lane `src` (wave-uniform) out of the lanes' registers: no memory round trip in the serial walks below
__device__ __forceinline__ bool knn_lane_box_hit(const KnnWave& w, const float4& lo, const float4& hi, int src)
{
    float4 blo, bhi;
    blo.x = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(lo.x), src));
    blo.y = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(lo.y), src));
    blo.z = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(lo.z), src));
    bhi.x = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(hi.x), src));
    bhi.y = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(hi.y), src));
    bhi.z = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(hi.z), src));
    return __ballot(w.active && box_dist2(w.qx, w.qy, w.qz, blo, bhi) < w.b2) != 0;
}

// the leaves of node n other than `own`: 64 leaf boxes at once against the wave's query box and R2, then each survivor against every
// lane's own query and best[2]; a leaf some lane can gain from is visited
__device__ __forceinline__ void knn_visit_node(KnnWave& w, const float4* __restrict__ pts, const float4* __restrict__ leafbox, int L,
                                               int n, int own, int lane)
{
    const int l0 = n * 64;
    const int l = l0 + lane;
    float4 lo = make_float4(INFINITY, INFINITY, INFINITY, 0.f), hi = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f);
    if (l < L && l != own) { lo = leafbox[2 * (size_t)l]; hi = leafbox[2 * (size_t)l + 1]; }
    uint64_t m = __ballot(boxbox_dist2(w.qlo, w.qhi, lo, hi) < w.R2);
    while (m) {
        const int src = (int)__builtin_ctzll(m);
        m &= m - 1;
        if (knn_lane_box_hit(w, lo, hi, src)) knn_visit_leaf(w, pts, l0 + src);
    }
    w.R2 = wave_max(w.active ? w.b2 : 0.f);
}

__global__ void __launch_bounds__(256)
knn_query_kernel(int P, int L, int Nn, const float4* __restrict__ pts, const float4* __restrict__ leafbox,
                 const float4* __restrict__ nodebox, const uint32_t* __restrict__ perm, float* __restrict__ out)
{
    // neighbouring leaves share candidates: give each XCD (blocks with equal blockIdx % 8) a contiguous run of them (bijective remap)
    const int nwg = gridDim.x, orig = blockIdx.x, xcd = orig % 8, q8 = nwg / 8, r8 = nwg % 8;
    const int wg = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + orig / 8;
    const int leaf = wg * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (leaf >= L) return;
    const int s = leaf * 64 + lane;
    KnnWave w;
    const float4 q = pts[s];                     // padding and non-finite points hold +inf
    w.qx = q.x; w.qy = q.y; w.qz = q.z;
    w.active = s < P && isfinite(q.x);
    w.b0 = FLT_MAX; w.b1 = FLT_MAX; w.b2 = FLT_MAX;   // simple-knn: best[3] = {FLT_MAX, FLT_MAX, FLT_MAX}

    // seed: the wave's own leaf, itself excluded by index (a duplicate elsewhere counts, at distance 0)
    {
        const float4* c = pts + (size_t)leaf * 64;
#pragma unroll 8
        for (int j = 0; j < 64; j++) {
            const float4 p = c[j];
            const float d = dist2(w.qx, w.qy, w.qz, p.x, p.y, p.z);
            knn_insert(j == lane ? INFINITY : d, w.b0, w.b1, w.b2);
        }
    }
    w.qlo = make_float4(wave_min(w.active ? w.qx : INFINITY), wave_min(w.active ? w.qy : INFINITY), wave_min(w.active ? w.qz : INFINITY), 0.f);
    w.qhi = make_float4(wave_max(w.active ? w.qx : -INFINITY), wave_max(w.active ? w.qy : -INFINITY), wave_max(w.active ? w.qz : -INFINITY), 0.f);
    w.R2 = wave_max(w.active ? w.b2 : 0.f);

    const int own_node = leaf / 64;
    knn_visit_node(w, pts, leafbox, L, own_node, leaf, lane);             // the nearest 4096 points first: tightens best[2] early
    for (int nb = 0; nb < Nn; nb += 64) {
        const int n = nb + lane;
        float4 lo = make_float4(INFINITY, INFINITY, INFINITY, 0.f), hi = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f);
        if (n < Nn && n != own_node) { lo = nodebox[2 * (size_t)n]; hi = nodebox[2 * (size_t)n + 1]; }
        uint64_t m = __ballot(boxbox_dist2(w.qlo, w.qhi, lo, hi) < w.R2);
        while (m) {
            const int src = (int)__builtin_ctzll(m);
            m &= m - 1;
            if (knn_lane_box_hit(w, lo, hi, src)) knn_visit_node(w, pts, leafbox, L, nb + src, leaf, lane);    // (far outliers stop here)
        }
    }
    if (s < P) out[perm[s]] = (w.b0 + w.b1 + w.b2) / 3.0f;       // simple-knn: (best[0] + best[1] + best[2]) / 3.0f, left to right
}

static size_t knn_scratch_bytes(int P) { return KnnLayout(P).total; }

static hipError_t launch_knn_mean_dist2(hipStream_t s, int P, const float* xyz, void* scratch, float* out)
{
    if (P <= 0) return hipSuccess;
    const KnnLayout K(P);
    char* b = align_ptr((const char*)scratch);
    float* lohi = (float*)(b + K.lohi);
    float* part = (float*)(b + K.part);
    RadixBufs r1 = K.sort.at(b);                      // low 32 key bits, then (r2) the high 31
    float4 *pts = (float4*)(b + K.pts), *leafbox = (float4*)(b + K.leaf), *nodebox = (float4*)(b + K.node);

    hipError_t e = radix_sort_begin(s, (uint32_t)P, r1, 2);
    if (e != hipSuccess) return e;
    const RadixBufs r2 = r1.second_round(32);
    int parts = (P + 63) / 64;
    if (parts > KNN_BBOX_PARTS) parts = KNN_BBOX_PARTS;
    hipLaunchKernelGGL(knn_bbox_partial_kernel, dim3(parts), dim3(64), 0, s, P, xyz, part);
    hipLaunchKernelGGL(knn_bbox_final_kernel, dim3(1), dim3(64), 0, s, parts, (const float*)part, lohi);
    const dim3 g256((P + 255) / 256);
    hipLaunchKernelGGL(knn_keys_lo_kernel, g256, dim3(256), 0, s, P, xyz, (const float*)lohi, r1.ka, r1.va, r1.hist, r1.per_block);
    e = radix_sort_pairs(s, (uint32_t)P, r1, 0, 32);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(knn_keys_hi_kernel, g256, dim3(256), 0, s, P, xyz, (const float*)lohi, (const uint32_t*)r1.sorted_vals(32), r2.ka, r2.va,
                       r2.hist, r2.per_block);
    e = radix_sort_pairs(s, (uint32_t)P, r2, 0, 3 * KNN_BITS - 32);
    if (e != hipSuccess) return e;
    const uint32_t* sv = r2.sorted_vals(3 * KNN_BITS - 32);

    const dim3 gl((K.L + 3) / 4), gn((K.Nn + 3) / 4);
    hipLaunchKernelGGL(knn_gather_kernel, gl, dim3(256), 0, s, P, K.L, xyz, sv, pts, leafbox);
    hipLaunchKernelGGL(knn_node_kernel, gn, dim3(256), 0, s, K.L, K.Nn, (const float4*)leafbox, nodebox);
    hipLaunchKernelGGL(knn_query_kernel, gl, dim3(256), 0, s, P, K.L, K.Nn, (const float4*)pts, (const float4*)leafbox,
                       (const float4*)nodebox, sv, out);
    return hipGetLastError();
}
// the entry points (the contract is in include/igs_rast.h)
extern "C" size_t igs_knn_scratch_bytes(int P)
{
    if (P < 0 || P > IGS_KNN_MAX_POINTS) return 0;
    return knn_scratch_bytes(P) + 256;
}
extern "C" int igs_knn_mean_dist2(void* stream, int P, const float* xyz, void* scratch, float* out)
{
    if (P < 0 || P > IGS_KNN_MAX_POINTS) return fail(IGS_RAST_E_INVALID, "igs_knn_mean_dist2: P out of range (0..IGS_KNN_MAX_POINTS)");
    if (P == 0) return 0;
    if (!xyz || !scratch || !out) return fail(IGS_RAST_E_INVALID, "igs_knn_mean_dist2: NULL pointer");
    HIP_TRY(launch_knn_mean_dist2((hipStream_t)stream, P, xyz, scratch, out), "knn launch");
    return 0;
}

// phase 1 alone, for anchors.hip: lohi[6] = box of the finite points of xyz[P], part: KNN_BBOX_PARTS * 8 floats of scratch
hipError_t launch_knn_bbox(hipStream_t s, int P, const float* xyz, float* part, float* lohi)
{
    int parts = (P + 63) / 64;
    if (parts > KNN_BBOX_PARTS) parts = KNN_BBOX_PARTS;
    if (parts < 1) parts = 1;
    hipLaunchKernelGGL(knn_bbox_partial_kernel, dim3(parts), dim3(64), 0, s, P, xyz, part);
    hipLaunchKernelGGL(knn_bbox_final_kernel, dim3(1), dim3(64), 0, s, parts, (const float*)part, lohi);
    return hipGetLastError();
}
