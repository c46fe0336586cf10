// anchors.hip -- the anchor graph of IGS's AGM-Net (igs/models/gs.py get_mask_fpsample) for gfx950: in-box selection, exact
// farthest-point sampling and batched k-nearest neighbours with torch_cluster's semantics (include/igs_rast.h states the contracts,
// DESIGN.md section 12 the design, the exactness argument and the figures).
//
// (a) select: flag -> per-block count -> the library's exclusive scan -> scatter; ascending index order, as torch.where.
// (b) fps: per launch, the points of all examples are sorted by (example, 30-bit Morton code) with the library's stable radix sort
//     (Morton round, then example round), copied into leaf-aligned float4 rows {x, y, z, cur} and cut into leaves of LS = 64 m points,
//     each with a box and a record (max cur, original index of that point, its xyz).  One workgroup of 16 waves per example; leaf l of
//     the example lives in wave l % 16, lane (l / 16) % 64, register slot l / 1024 -- adjacent leaves land in different waves.  Each
//     iteration: (1) every wave tests its leaves' boxes against the new point and updates the surviving leaves from their rows (lane =
//     point; the rows stay with the wave that owns the leaf); (2) the wave's argmax over its records (DPP inside rows of 16 lanes, then
//     four lane reads); (3) one LDS slot per wave and one barrier; every wave folds the 16 slots itself.  No cross-workgroup
//     communication; the launch boundary is the only hand-off.
// (c) knn: brute force in index order, one query per lane, k sorted slots in registers, x staged in LDS tiles.
#include "common.h"
#include "knn_common.h"
#include "host_api.h"
#include <float.h>

#define FPS_WAVES 16                 // waves of the FPS workgroup
#define FPS_MAX_SLOTS 4              // leaf records per lane: 11 VGPRs each under the 128 of a 1024-thread workgroup (8 spill)
#define KNNQ_THREADS 256             // queries per kNN workgroup
#define KNNQ_TILE 2048               // x points per LDS tile (32 KiB)
#define KNNQ_NONE 1e10f              // torch_cluster's initial best_dist: a candidate counts only when d2 < 1e10

// ---------------------------------------------------------------------------------------------------------------------------------
// shared helpers
// ---------------------------------------------------------------------------------------------------------------------------------
// example of element i given the sorted offsets ptr[0..B]: the b with ptr[b] <= i < ptr[b + 1] (last such b for empty examples)
__device__ __forceinline__ int example_of(const int* __restrict__ ptr, int B, int i)
{
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (ptr[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// FPS key of a cur value: order-preserving for cur in [0, +inf], 0 for -inf (non-finite points and padding never win over a finite one)
__device__ __forceinline__ uint32_t cur_key(float c) { return c >= 0.f ? __float_as_uint(c) + 1u : 0u; }
__device__ __forceinline__ float key_cur(uint32_t k) { return k ? __uint_as_float(k - 1u) : -INFINITY; }

// reductions over the 16 lanes of every DPP row (quad swaps, half-row mirror, row mirror), then over the four rows (lane reads)
template <bool MAX>
__device__ __forceinline__ uint32_t wave_fold_u32(uint32_t v)
{
    auto op = [](uint32_t a, uint32_t b) { return MAX ? (a > b ? a : b) : (a < b ? a : b); };
    v = op(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, false));     // quad_perm [1, 0, 3, 2]
    v = op(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, false));     // quad_perm [2, 3, 0, 1]
    v = op(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x141, 0xF, 0xF, false));    // row_half_mirror
    v = op(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x140, 0xF, 0xF, false));    // row_mirror
    const uint32_t r0 = __builtin_amdgcn_readlane(v, 0), r1 = __builtin_amdgcn_readlane(v, 16);
    const uint32_t r2 = __builtin_amdgcn_readlane(v, 32), r3 = __builtin_amdgcn_readlane(v, 48);
    return op(op(r0, r1), op(r2, r3));
}

// argmax of (key desc, orig asc) over the wave (all 64 lanes active); the winner's key, orig and xyz become wave-uniform
__device__ __forceinline__ void wave_argmax(uint32_t& key, uint32_t& orig, float& x, float& y, float& z)
{
    const uint32_t K = wave_fold_u32<true>(key);
    const uint32_t O = wave_fold_u32<false>(key == K ? orig : 0xFFFFFFFFu);
    const uint64_t m = __ballot(key == K && orig == O);
    const int src = (int)__builtin_ctzll(m);
    x = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), src));
    y = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(y), src));
    z = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(z), src));
    key = K; orig = O;
}
__device__ __forceinline__ bool beats(uint32_t k, uint32_t o, uint32_t bk, uint32_t bo) { return k > bk || (k == bk && o < bo); }

// ---------------------------------------------------------------------------------------------------------------------------------
// (a) in-box selection
// ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool in_box(const float* __restrict__ xyz, const float* __restrict__ box, int i, int b, float& x, float& y, float& z)
{
    x = xyz[3 * (size_t)i]; y = xyz[3 * (size_t)i + 1]; z = xyz[3 * (size_t)i + 2];
    const float* q = box + 6 * (size_t)b;        // select_points_bbox: lo <= p <= hi on every axis (NaN: outside)
    return x >= q[0] && x <= q[3] && y >= q[1] && y <= q[4] && z >= q[2] && z <= q[5];
}

__global__ void __launch_bounds__(256)
select_count_kernel(int N, int B, const float* __restrict__ xyz, const int* __restrict__ ptr, const float* __restrict__ box,
                    uint32_t* __restrict__ blocksum, int* __restrict__ count)
{
    __shared__ uint32_t ws[4];
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    bool f = false;
    int b = 0;
    if (i < N) {
        float x, y, z;
        b = example_of(ptr, B, i);
        f = in_box(xyz, box, i, b, x, y, z);
    }
    const uint64_t m = __ballot(f);
    // per-example counts: one add per wave when the wave lies in one example (the usual case), else one per flagged lane
    const int b0 = __builtin_amdgcn_readfirstlane(b);
    const bool uniform = __ballot(i < N && b != b0) == 0;
    if (uniform) { if (lane == 0 && m) atomicAdd(&count[b0], (int)__popcll(m)); }
    else if (f) atomicAdd(&count[b], 1);
    if (lane == 0) ws[threadIdx.x >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) blocksum[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}

__global__ void __launch_bounds__(256)
select_scatter_kernel(int N, int B, const float* __restrict__ xyz, const int* __restrict__ ptr, const float* __restrict__ box,
                      const uint32_t* __restrict__ blockoff, float* __restrict__ out_xyz, int64_t* __restrict__ out_idx)
{
    __shared__ uint32_t ws[4];
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    bool f = false;
    int b = 0;
    float x = 0.f, y = 0.f, z = 0.f;
    if (i < N) {
        b = example_of(ptr, B, i);
        f = in_box(xyz, box, i, b, x, y, z);
    }
    const uint64_t m = __ballot(f);
    if (lane == 0) ws[w] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t o = blockoff[blockIdx.x];
    for (int k = 0; k < w; k++) o += ws[k];
    o += (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (f) {
        out_xyz[3 * (size_t)o] = x; out_xyz[3 * (size_t)o + 1] = y; out_xyz[3 * (size_t)o + 2] = z;
        out_idx[o] = (int64_t)(i - ptr[b]);
    }
}

static size_t select_scratch_bytes(int N) { return align_up(((size_t)N / 256 + 2) * 4, 256) + 256; }

static hipError_t launch_bbox_select(hipStream_t s, int B, int N, const float* xyz, const int* ptr, const float* box, void* scratch,
                                     float* out_xyz, int64_t* out_idx, int* count)
{
    hipError_t e = zero_fill_async(s, count, (size_t)B * 4);
    if (e != hipSuccess || N == 0) return e;
    uint32_t* blocksum = (uint32_t*)align_ptr((const char*)scratch);
    const int nb = (N + 255) / 256;
    hipLaunchKernelGGL(select_count_kernel, dim3(nb), dim3(256), 0, s, N, B, xyz, ptr, box, blocksum, count);
    e = launch_exclusive_scan(s, nb, blocksum);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(select_scatter_kernel, dim3(nb), dim3(256), 0, s, N, B, xyz, ptr, box, (const uint32_t*)blocksum, out_xyz, out_idx);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (b) farthest-point sampling
// ---------------------------------------------------------------------------------------------------------------------------------
// leaf size and register slots for the largest example: LS = 64 m points per leaf, at most FPS_WAVES * 64 * R leaves per example
// (LS = 64 up to 262144 points, 128 up to 524288, 256 up to 1048576, ...)
static void fps_geometry(int max_n, int* LS, int* R)
{
    int m = 1;
    while ((long long)max_n > (long long)FPS_WAVES * 64 * FPS_MAX_SLOTS * 64 * m) m *= 2;     // at most FPS_MAX_SLOTS, then wider leaves
    const long long leaves = ((long long)max_n + 64 * m - 1) / (64 * m);
    int r = 1;
    while ((long long)FPS_WAVES * 64 * r < leaves) r *= 2;
    *LS = 64 * m; *R = r;
}

struct FpsLayout {
    size_t lohi, part, rowoff, rows, ord, leaf, total;
    RadixOffsets sort;                 // two rounds: two adjacent histogram blocks
    int LS, R;
    long long nrows, nleaves;
    FpsLayout(int B, int N, int max_n) {
        fps_geometry(max_n, &LS, &R);
        const size_t n = (size_t)(N > 0 ? N : 0);
        nrows = (long long)n + (long long)B * (LS - 1);          // every example padded to whole leaves
        nrows = (nrows + LS - 1) / LS * LS;
        nleaves = nrows / LS;
        size_t o = 0;
        lohi = o;   o += 256;
        part = o;   o += align_up((size_t)KNN_BBOX_PARTS * 8 * 4, 256);
        sort = radix_layout_append(o, n, 2);
        rowoff = o; o += align_up(((size_t)B + 1) * 4, 256);
        rows = o;   o += align_up((size_t)nrows * 16, 256);
        ord = o;    o += align_up((size_t)nrows * 4, 256);
        leaf = o;   o += align_up((size_t)nleaves * 48, 256);
        total = o + 256;
    }
};

// round 1: the top 30 bits of the 63-bit Morton key (10 per axis) over the box of all points, identity values
__global__ void __launch_bounds__(256)
fps_keys_morton_kernel(int N, const float* __restrict__ xyz, const float* __restrict__ lohi, uint32_t* __restrict__ keys,
                       uint32_t* __restrict__ vals, uint32_t* __restrict__ hist0, uint32_t per_block)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const uint32_t k = (uint32_t)(knn_key(xyz, (uint32_t)i, lohi) >> 33);
    keys[i] = k; vals[i] = (uint32_t)i;
    radix_count_first(hist0, (uint32_t)i, per_block, k);
}
// round 2: the example of every point, in round-1 order (stable: Morton order inside each example)
__global__ void __launch_bounds__(256)
fps_keys_example_kernel(int N, int B, const int* __restrict__ ptr, const uint32_t* __restrict__ order, uint32_t* __restrict__ keys,
                        uint32_t* __restrict__ vals, uint32_t* __restrict__ hist0, uint32_t per_block)
{
    // few distinct keys per block: counted in LDS first (one global add per digit), as knn.hip's high-bit round
    const int s = blockIdx.x * 256 + threadIdx.x;
    radix_count_first_lds(hist0, per_block, [&](uint32_t& k) {
        if (s >= N) return false;
        const uint32_t v = order[s];
        k = (uint32_t)example_of(ptr, B, (int)v);
        keys[s] = k; vals[s] = v;
        return true;
    });
}
// leaf-aligned row offsets of the examples (one thread: B is small beside N)
__global__ void __launch_bounds__(64)
fps_rowoff_kernel(int B, int LS, const int* __restrict__ ptr, int* __restrict__ rowoff)
{
    if (threadIdx.x != 0) return;
    int o = 0;
    for (int b = 0; b < B; b++) {
        rowoff[b] = o;
        const int n = max(ptr[b + 1] - ptr[b], 0);
        o += (n + LS - 1) / LS * LS;
    }
    rowoff[B] = o;
}
// rows {x, y, z, cur} in sorted order: cur = init for a finite point, -inf (never selected, never lowered) for a non-finite point and
// for the padding, whose xyz is +inf and whose original index is ~0
__global__ void __launch_bounds__(256)
fps_rows_kernel(int nrows, int N, int B, float init_d2, const float* __restrict__ xyz, const int* __restrict__ ptr,
                const int* __restrict__ rowoff, const uint32_t* __restrict__ perm, float4* __restrict__ rows, uint32_t* __restrict__ ord)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= nrows || r >= rowoff[B]) return;
    const int b = example_of(rowoff, B, r);
    const int local = r - rowoff[b];
    float4 p = make_float4(INFINITY, INFINITY, INFINITY, -INFINITY);
    uint32_t v = 0xFFFFFFFFu;
    if (local < ptr[b + 1] - ptr[b] && ptr[b] + local < N) {
        v = perm[ptr[b] + local];
        p.x = xyz[3 * (size_t)v]; p.y = xyz[3 * (size_t)v + 1]; p.z = xyz[3 * (size_t)v + 2];
        if (finite3(p.x, p.y, p.z)) p.w = init_d2;
        else { p.x = INFINITY; p.y = INFINITY; p.z = INFINITY; }
    }
    rows[r] = p;
    ord[r] = v;
}

// a leaf's record from its rows (wave-uniform leaf, lane = point); returns the wave-uniform record, bounds the finite points if `box`
__device__ __forceinline__ void fps_leaf_scan(float4* __restrict__ rows, const uint32_t* __restrict__ ord, size_t base, int m, int lane,
                                              bool update, float qx, float qy, float qz, uint32_t& bk, uint32_t& bo,
                                              float& bx, float& by, float& bz)
{
    bk = 0; bo = 0xFFFFFFFFu; bx = INFINITY; by = INFINITY; bz = INFINITY;
    for (int j = 0; j < m; j++) {
        const size_t r = base + (size_t)j * 64 + lane;
        const float4 p = rows[r];
        const uint32_t o = ord[r];
        float c = p.w;
        if (update) {
            c = fminf(c, dist2(qx, qy, qz, p.x, p.y, p.z));      // fminf: a NaN distance (non-finite operand) lowers nothing
            if (c < p.w) ((float*)rows)[4 * r + 3] = c;
        }
        const uint32_t k = cur_key(c);
        if (beats(k, o, bk, bo)) { bk = k; bo = o; bx = p.x; by = p.y; bz = p.z; }
    }
    wave_argmax(bk, bo, bx, by, bz);
}

// initial leaf records: {lo.xyz, max cur}, {hi.xyz, bits(original index)}, {xyz of that point, 0}; one wave per leaf
__global__ void __launch_bounds__(256)
fps_leaf_kernel(int nleaves, int B, int LS, const int* __restrict__ rowoff, float4* __restrict__ rows, const uint32_t* __restrict__ ord,
                float4* __restrict__ leaf)
{
    const int l = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (l >= nleaves || (long long)l * LS >= rowoff[B]) return;
    const size_t base = (size_t)l * LS;
    float lx = INFINITY, ly = INFINITY, lz = INFINITY, hx = -INFINITY, hy = -INFINITY, hz = -INFINITY;
    for (int j = 0; j < LS / 64; j++) {
        const float4 p = rows[base + (size_t)j * 64 + lane];
        if (finite3(p.x, p.y, p.z)) { lx = fminf(lx, p.x); ly = fminf(ly, p.y); lz = fminf(lz, p.z); hx = fmaxf(hx, p.x); hy = fmaxf(hy, p.y); hz = fmaxf(hz, p.z); }
    }
    lx = wave_min(lx); ly = wave_min(ly); lz = wave_min(lz); hx = wave_max(hx); hy = wave_max(hy); hz = wave_max(hz);
    uint32_t bk, bo;
    float bx, by, bz;
    fps_leaf_scan(rows, ord, base, LS / 64, lane, false, 0.f, 0.f, 0.f, bk, bo, bx, by, bz);
    if (lane == 0) {
        leaf[3 * (size_t)l] = make_float4(lx, ly, lz, key_cur(bk));
        leaf[3 * (size_t)l + 1] = make_float4(hx, hy, hz, __uint_as_float(bo));
        leaf[3 * (size_t)l + 2] = make_float4(bx, by, bz, 0.f);
    }
}

// the FPS loop: one workgroup per example, R register slots of leaf records per lane
template <int R>
__global__ void __launch_bounds__(1024)
fps_kernel(int N, int nrows, int total, int LS, const int* __restrict__ ptr, const int* __restrict__ rowoff, const int* __restrict__ start,
           const int* __restrict__ out_ptr, const float* __restrict__ xyz, float4* __restrict__ rows, const uint32_t* __restrict__ ord,
           const float4* __restrict__ leaf, int64_t* __restrict__ out)
{
    __shared__ uint32_t s_ko[2][FPS_WAVES][2];
    __shared__ float s_p[2][FPS_WAVES][4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = ptr[b + 1] - ptr[b], o0 = out_ptr[b];
    const int S = min(out_ptr[b + 1], total) - o0;       // (samples past `total` are not written)
    if (S <= 0 || o0 < 0) return;
    int64_t* o = out + o0;
    const int m = LS / 64;
    const int L = (rowoff[b + 1] - rowoff[b]) / LS;
    // nothing to sample, an example larger than the launch was sized for, or offsets that do not describe N points
    if (n <= 0 || L > FPS_WAVES * 64 * R || ptr[b] < 0 || ptr[b + 1] > N || rowoff[b + 1] > nrows) {
        for (int i = tid; i < S; i += 1024) o[i] = -1;
        return;
    }
    const size_t row0 = (size_t)rowoff[b];
    const int leaf0 = rowoff[b] / LS;

    float mx[R], px[R], py[R], pz[R];
    uint32_t oi[R];
    float4 lo[R], hi[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int l = (r * 64 + lane) * FPS_WAVES + w;
        if (l < L) {
            const float4 a = leaf[3 * (size_t)(leaf0 + l)], c = leaf[3 * (size_t)(leaf0 + l) + 1], p = leaf[3 * (size_t)(leaf0 + l) + 2];
            lo[r] = a; hi[r] = c; mx[r] = a.w; oi[r] = __float_as_uint(c.w); px[r] = p.x; py[r] = p.y; pz[r] = p.z;
        } else {
            lo[r] = make_float4(INFINITY, INFINITY, INFINITY, 0.f); hi[r] = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f);
            mx[r] = -INFINITY; oi[r] = 0xFFFFFFFFu; px[r] = INFINITY; py[r] = INFINITY; pz[r] = INFINITY;
        }
    }
    int st = start[b];
    if (st < 0 || st >= n) st = 0;
    float qx = xyz[3 * (size_t)(ptr[b] + st)], qy = xyz[3 * (size_t)(ptr[b] + st) + 1], qz = xyz[3 * (size_t)(ptr[b] + st) + 2];
    if (tid == 0) o[0] = ptr[b] + st;

    for (int s = 1; s < S; s++) {
        // 1. leaves whose box can hold a point closer to q than the leaf's max cur: the owning wave updates them (lane = point)
#pragma unroll
        for (int r = 0; r < R; r++) {
            uint64_t need = __ballot(box_dist2(qx, qy, qz, lo[r], hi[r]) < mx[r]);
            while (need) {
                const int src = (int)__builtin_ctzll(need);
                need &= need - 1;
                const int l = (r * 64 + src) * FPS_WAVES + w;
                uint32_t bk, bo;
                float bx, by, bz;
                fps_leaf_scan(rows, ord, row0 + (size_t)l * LS, m, lane, true, qx, qy, qz, bk, bo, bx, by, bz);
                if (lane == src) { mx[r] = key_cur(bk); oi[r] = bo; px[r] = bx; py[r] = by; pz[r] = bz; }
            }
        }
        // 2. the wave's best record
        uint32_t bk = cur_key(mx[0]), bo = oi[0];
        float bx = px[0], by = py[0], bz = pz[0];
#pragma unroll
        for (int r = 1; r < R; r++) {
            const uint32_t k = cur_key(mx[r]);
            if (beats(k, oi[r], bk, bo)) { bk = k; bo = oi[r]; bx = px[r]; by = py[r]; bz = pz[r]; }
        }
        wave_argmax(bk, bo, bx, by, bz);
        // 3. the 16 wave winners through LDS (two buffers: one barrier per iteration), folded by every wave
        const int par = s & 1;
        if (lane == 0) {
            s_ko[par][w][0] = bk; s_ko[par][w][1] = bo;
            s_p[par][w][0] = bx; s_p[par][w][1] = by; s_p[par][w][2] = bz;
        }
        __syncthreads();
        bk = 0; bo = 0xFFFFFFFFu; bx = by = bz = INFINITY;
        if (lane < FPS_WAVES) {
            bk = s_ko[par][lane][0]; bo = s_ko[par][lane][1];
            bx = s_p[par][lane][0]; by = s_p[par][lane][1]; bz = s_p[par][lane][2];
        }
        wave_argmax(bk, bo, bx, by, bz);
        qx = bx; qy = by; qz = bz;
        if (tid == 0) o[s] = (int64_t)bo;
    }
}

static size_t fps_scratch_bytes(int B, int N, int max_n) { return FpsLayout(B, N, max_n).total; }

static hipError_t launch_fps(hipStream_t s, int B, int N, int max_n, const float* xyz, const int* ptr, const int* start, const int* out_ptr,
                             int total, float init_d2, void* scratch, int64_t* out)
{
    if (B <= 0) return hipSuccess;
    const FpsLayout F(B, N, max_n);
    char* base = align_ptr((const char*)scratch);
    float* lohi = (float*)(base + F.lohi);
    float* part = (float*)(base + F.part);
    RadixBufs r1 = F.sort.at(base);                  // Morton bits, then (r2) the example
    int* rowoff = (int*)(base + F.rowoff);
    float4* rows = (float4*)(base + F.rows);
    uint32_t* ord = (uint32_t*)(base + F.ord);
    float4* leaf = (float4*)(base + F.leaf);

    hipError_t e = radix_sort_begin(s, (uint32_t)N, r1, 2);
    if (e != hipSuccess) return e;
    const RadixBufs r2 = r1.second_round(30);
    hipLaunchKernelGGL(fps_rowoff_kernel, dim3(1), dim3(64), 0, s, B, F.LS, ptr, rowoff);
    const uint32_t* perm = r1.va;
    if (N > 0) {
        e = launch_knn_bbox(s, N, xyz, part, lohi);
        if (e != hipSuccess) return e;
        const dim3 g256((N + 255) / 256);
        hipLaunchKernelGGL(fps_keys_morton_kernel, g256, dim3(256), 0, s, N, xyz, (const float*)lohi, r1.ka, r1.va, r1.hist, r1.per_block);
        e = radix_sort_pairs(s, (uint32_t)N, r1, 0, 30);
        if (e != hipSuccess) return e;
        perm = r1.sorted_vals(30);
        if (B > 1) {
            int bits = 0;
            while ((1 << bits) < B) bits++;
            hipLaunchKernelGGL(fps_keys_example_kernel, g256, dim3(256), 0, s, N, B, ptr, perm, r2.ka, r2.va, r2.hist, r2.per_block);
            e = radix_sort_pairs(s, (uint32_t)N, r2, 0, bits);
            if (e != hipSuccess) return e;
            perm = r2.sorted_vals(bits);
        }
        hipLaunchKernelGGL(fps_rows_kernel, dim3((unsigned)((F.nrows + 255) / 256)), dim3(256), 0, s, (int)F.nrows, N, B, init_d2, xyz, ptr,
                           (const int*)rowoff, perm, rows, ord);
        hipLaunchKernelGGL(fps_leaf_kernel, dim3((unsigned)((F.nleaves + 3) / 4)), dim3(256), 0, s, (int)F.nleaves, B, F.LS,
                           (const int*)rowoff, rows, (const uint32_t*)ord, leaf);
    }
    switch (F.R) {
    case 1: hipLaunchKernelGGL(fps_kernel<1>, dim3(B), dim3(1024), 0, s, N, (int)F.nrows, total, F.LS, ptr, (const int*)rowoff, start, out_ptr, xyz, rows, (const uint32_t*)ord, (const float4*)leaf, out); break;
    case 2: hipLaunchKernelGGL(fps_kernel<2>, dim3(B), dim3(1024), 0, s, N, (int)F.nrows, total, F.LS, ptr, (const int*)rowoff, start, out_ptr, xyz, rows, (const uint32_t*)ord, (const float4*)leaf, out); break;
    default: hipLaunchKernelGGL(fps_kernel<4>, dim3(B), dim3(1024), 0, s, N, (int)F.nrows, total, F.LS, ptr, (const int*)rowoff, start, out_ptr, xyz, rows, (const uint32_t*)ord, (const float4*)leaf, out); break;
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (c) k nearest neighbours (torch_cluster knn)
// ---------------------------------------------------------------------------------------------------------------------------------
// K slots (K >= k): the k nearest of the K nearest are the k nearest.  A workgroup streams the x range of the examples of its queries;
// when they span several examples each lane masks the candidates outside its own.
template <int K, bool MASK>
__global__ void __launch_bounds__(KNNQ_THREADS)
knnq_kernel(int Nx, int Ny, int B, int k, const float* __restrict__ x, const float* __restrict__ y, const int* __restrict__ ptr_x,
            const int* __restrict__ ptr_y, float scale, int64_t* __restrict__ out_idx, float* __restrict__ out_d2,
            float* __restrict__ out_w)
{
    __shared__ float4 tile[KNNQ_TILE];
    const int j = blockIdx.x * KNNQ_THREADS + threadIdx.x;
    const int jq = j < Ny ? j : Ny - 1;
    const int jfirst = blockIdx.x * KNNQ_THREADS;
    const int jlast = min(jfirst + KNNQ_THREADS, Ny) - 1;
    const int bf = example_of(ptr_y, B, jfirst), bl = example_of(ptr_y, B, jlast);
    if (!MASK && bf != bl) return;            // (the launcher runs the masked instantiation for those workgroups)
    if (MASK && bf == bl) return;
    const int b = example_of(ptr_y, B, jq);
    const int xbeg = max(ptr_x[bf], 0), xend = min(ptr_x[bl + 1], Nx);          // (clamped: offsets never lead outside x)
    const int mybeg = ptr_x[b], myend = ptr_x[b + 1];
    const float qx = y[3 * (size_t)jq], qy = y[3 * (size_t)jq + 1], qz = y[3 * (size_t)jq + 2];
    float d[K];
    int id[K];
#pragma unroll
    for (int s = 0; s < K; s++) { d[s] = KNNQ_NONE; id[s] = -1; }

    for (int t0 = xbeg; t0 < xend; t0 += KNNQ_TILE) {
        const int cnt = min(KNNQ_TILE, xend - t0);
        __syncthreads();
        for (int i = threadIdx.x; i < cnt; i += KNNQ_THREADS)
            tile[i] = make_float4(x[3 * (size_t)(t0 + i)], x[3 * (size_t)(t0 + i) + 1], x[3 * (size_t)(t0 + i) + 2], 0.f);
        __syncthreads();
#pragma unroll 4
        for (int i = 0; i < cnt; i++) {
            const float4 p = tile[i];
            const float dd = dist2(qx, qy, qz, p.x, p.y, p.z);
            const int c = t0 + i;
            bool ok = dd < d[K - 1];                           // strictly below the last slot: an equal distance keeps the lower index
            if (MASK) ok = ok && c >= mybeg && c < myend;
            if (ok) {
#pragma unroll
                for (int s = K - 1; s > 0; s--) {
                    const bool sh = dd < d[s - 1];
                    const bool put = dd < d[s];
                    d[s] = sh ? d[s - 1] : (put ? dd : d[s]);
                    id[s] = sh ? id[s - 1] : (put ? c : id[s]);
                }
                if (dd < d[0]) { d[0] = dd; id[0] = c; }
            }
        }
    }
    if (j >= Ny) return;
    // weights: softmax(-scale * sqrt(d2)) over the filled slots (gs.py:1009 with scale 10); empty slots: index -1, d2 +inf, weight 0
    float mxv = -INFINITY;
#pragma unroll
    for (int s = 0; s < K; s++) if (s < k && id[s] >= 0) mxv = fmaxf(mxv, -scale * sqrtf(d[s]));
    float sum = 0.f;
#pragma unroll
    for (int s = 0; s < K; s++) if (s < k && id[s] >= 0) sum += expf(-scale * sqrtf(d[s]) - mxv);
#pragma unroll
    for (int s = 0; s < K; s++) {
        if (s >= k) break;
        const bool has = id[s] >= 0;
        out_idx[(size_t)j * k + s] = has ? (int64_t)id[s] : (int64_t)-1;
        if (out_d2) out_d2[(size_t)j * k + s] = has ? d[s] : INFINITY;
        if (out_w) out_w[(size_t)j * k + s] = has ? expf(-scale * sqrtf(d[s]) - mxv) / sum : 0.f;
    }
}

template <int K>
static void knnq_launch(hipStream_t s, int Nx, int Ny, int B, int k, const float* x, const float* y, const int* ptr_x, const int* ptr_y,
                        float scale, int64_t* out_idx, float* out_d2, float* out_w)
{
    const dim3 g((Ny + KNNQ_THREADS - 1) / KNNQ_THREADS);
    hipLaunchKernelGGL((knnq_kernel<K, false>), g, dim3(KNNQ_THREADS), 0, s, Nx, Ny, B, k, x, y, ptr_x, ptr_y, scale, out_idx, out_d2, out_w);
    if (B > 1)
        hipLaunchKernelGGL((knnq_kernel<K, true>), g, dim3(KNNQ_THREADS), 0, s, Nx, Ny, B, k, x, y, ptr_x, ptr_y, scale, out_idx, out_d2, out_w);
}

static hipError_t launch_knn_query(hipStream_t s, int Nx, int Ny, int B, const float* x, const float* y, const int* ptr_x, const int* ptr_y,
                                   int k, float scale, int64_t* out_idx, float* out_d2, float* out_w)
{
    if (Ny <= 0) return hipSuccess;
    if (k <= 8) knnq_launch<8>(s, Nx, Ny, B, k, x, y, ptr_x, ptr_y, scale, out_idx, out_d2, out_w);
    else if (k <= 16) knnq_launch<16>(s, Nx, Ny, B, k, x, y, ptr_x, ptr_y, scale, out_idx, out_d2, out_w);
    else if (k <= 32) knnq_launch<32>(s, Nx, Ny, B, k, x, y, ptr_x, ptr_y, scale, out_idx, out_d2, out_w);
    else knnq_launch<100>(s, Nx, Ny, B, k, x, y, ptr_x, ptr_y, scale, out_idx, out_d2, out_w);
    return hipGetLastError();
}

// the entry points (the contracts are in include/igs_rast.h)
extern "C" size_t igs_bbox_select_scratch_bytes(int N)
{
    if (N < 0 || N > IGS_ANCHOR_MAX_POINTS) return 0;
    return select_scratch_bytes(N) + 256;
}
extern "C" int igs_bbox_select(void* stream, int B, int N, const float* xyz, const int* ptr, const float* box, void* scratch,
                               float* out_xyz, int64_t* out_idx, int* out_count)
{
    if (B < 1 || B > IGS_ANCHOR_MAX_EXAMPLES || N < 0 || N > IGS_ANCHOR_MAX_POINTS)
        return fail(IGS_RAST_E_INVALID, "igs_bbox_select: B or N out of range");
    if (!ptr || !box || !out_count || (N > 0 && (!xyz || !scratch || !out_xyz || !out_idx)))
        return fail(IGS_RAST_E_INVALID, "igs_bbox_select: NULL pointer");
    HIP_TRY(launch_bbox_select((hipStream_t)stream, B, N, xyz, ptr, box, scratch, out_xyz, out_idx, out_count), "bbox select launch");
    return 0;
}
extern "C" size_t igs_fps_scratch_bytes(int B, int N, int max_n)
{
    if (B < 1 || B > IGS_ANCHOR_MAX_EXAMPLES || N < 0 || N > IGS_ANCHOR_MAX_POINTS || max_n < 0 || max_n > IGS_FPS_MAX_EXAMPLE_POINTS) return 0;
    return fps_scratch_bytes(B, N, max_n) + 256;
}
extern "C" int igs_fps(void* stream, int B, int N, int max_n, const float* xyz, const int* ptr, const int* start, const int* out_ptr,
                       int total, float init_d2, void* scratch, int64_t* out)
{
    if (B < 1 || B > IGS_ANCHOR_MAX_EXAMPLES || N < 0 || N > IGS_ANCHOR_MAX_POINTS || max_n < 0 || max_n > IGS_FPS_MAX_EXAMPLE_POINTS)
        return fail(IGS_RAST_E_INVALID, "igs_fps: B, N or max_n out of range");
    if (total < 0 || total > IGS_ANCHOR_MAX_POINTS) return fail(IGS_RAST_E_INVALID, "igs_fps: total out of range");
    if (total == 0) return 0;
    if (!(init_d2 >= 0.f)) return fail(IGS_RAST_E_INVALID, "igs_fps: init_d2 must be >= 0");
    if (!ptr || !start || !out_ptr || !scratch || !out || (N > 0 && !xyz)) return fail(IGS_RAST_E_INVALID, "igs_fps: NULL pointer");
    HIP_TRY(launch_fps((hipStream_t)stream, B, N, max_n, xyz, ptr, start, out_ptr, total, init_d2, scratch, out), "fps launch");
    return 0;
}
extern "C" int igs_knn_query(void* stream, int B, int Nx, int Ny, const float* x, const float* y, const int* ptr_x, const int* ptr_y,
                             int k, float weight_scale, int64_t* out_idx, float* out_d2, float* out_w)
{
    if (B < 1 || B > IGS_ANCHOR_MAX_EXAMPLES || Nx < 0 || Nx > IGS_ANCHOR_MAX_POINTS || Ny < 0 || Ny > IGS_ANCHOR_MAX_POINTS)
        return fail(IGS_RAST_E_INVALID, "igs_knn_query: B, Nx or Ny out of range");
    if (k < 1 || k > IGS_KNN_QUERY_MAX_K) return fail(IGS_RAST_E_INVALID, "igs_knn_query: k out of range (1..IGS_KNN_QUERY_MAX_K)");
    if (Ny == 0) return 0;
    if (!y || !ptr_x || !ptr_y || !out_idx || (Nx > 0 && !x)) return fail(IGS_RAST_E_INVALID, "igs_knn_query: NULL pointer");
    HIP_TRY(launch_knn_query((hipStream_t)stream, Nx, Ny, B, x, y, ptr_x, ptr_y, k, weight_scale, out_idx, out_d2, out_w), "knn query launch");
    return 0;
}
