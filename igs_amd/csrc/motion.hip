// motion.hip -- the two consumers of the anchor graph in IGS's AGM-Net for gfx950 (include/igs_rast.h states the contracts, DESIGN.md
// section 13 the design and the figures):
//
// (a) anchor feature interpolation, the tail of GS3DRenderer.query_ir_grid (igs/models/gs.py:812-822):
//     out[n, :] = sum_k w[n, k] * F[col[n, k], :].  Forward: one wave per row n, lanes across D, the slots' rows gathered four at a time
//     and summed in slot order.  Backward without float atomics: the edges e = n * K + k are stably sorted by anchor (the library's
//     radix sort), so every anchor's list of incoming edges is in ascending e order; the lists are cut into chunks of IC edges, one
//     wave per chunk sums w * dout over its chunk (and writes dw[e] = <dout[n], F[a]> on the way); a second launch adds each anchor's
//     chunk partials in chunk order.  Every sum has a fixed order, so dF and dw are bitwise reproducible.
// (b) Gaussian deform, GaussianModel.deform (gs.py:347-375) with quaternion_multiply (igs/utils/general_utils.py:177-200):
//     xyz[mask] += dxyz, rot[mask] = qmul(nrm(rot[mask]), nrm(drot)), and its backward through both normalisations.
#include "common.h"
#include "elem_common.h"
#include "host_api.h"

#define IW 4                          // waves per workgroup of the row / chunk kernels
#define ISLOTS 4                      // slots whose rows are in flight together in the forward (and edges in the backward)

// ---------------------------------------------------------------------------------------------------------------------------------
// shared helpers
// ---------------------------------------------------------------------------------------------------------------------------------
// chunk length of the backward's edge lists: a quarter of one wave's share of the edges with 16 waves on each of 256 CUs, as a power of
// two in [64, 512] (cdna_hip_programming.md Appendix B: split the long lists, add the partials in chunk order)
static uint32_t interp_chunk(uint64_t E)
{
    uint32_t c = 64;
    while (c < 512 && (uint64_t)c * 4 * 16 * 256 < E) c *= 2;
    return c;
}

struct InterpLayout {          // the inverse index and the backward's partial sums, offsets from a 256-byte aligned base
    RadixOffsets sort;         // edges by anchor: the result is where radix_lands_in_b(bits) says, for the index build and the backward alike
    size_t start, choff, part, total;
    uint64_t E, max_chunks;
    uint32_t chunk;
    int bits;
    InterpLayout(int N, int K, int A, int D) {
        E = (uint64_t)N * (uint64_t)K;
        chunk = interp_chunk(E);
        max_chunks = (E + chunk - 1) / chunk + (uint64_t)A;         // every anchor adds at most one partly filled chunk
        bits = 1;
        while (((uint64_t)1 << bits) <= (uint64_t)A) bits++;       // keys 0..A (A = an empty or out-of-range slot)
        size_t o = 0;
        sort = radix_layout_append(o, E);
        start = o; o += align_up(((size_t)A + 1) * 4, 256);         // start[a]: first sorted position of anchor a; start[A] = valid edges
        choff = o; o += align_up(((size_t)A + 1) * 4, 256);         // exclusive scan of the chunks per anchor; choff[A] = all chunks
        part = o;  o += align_up((size_t)max_chunks * (size_t)D * 4, 256);
        total = o + 256;
    }
};

// ---------------------------------------------------------------------------------------------------------------------------------
// (a) interpolation forward
// ---------------------------------------------------------------------------------------------------------------------------------
template <int DV, typename T>
__global__ void __launch_bounds__(IW * 64)
interp_fwd_kernel(int N, int K, int D, int A, const T* __restrict__ F, const int64_t* __restrict__ col, const float* __restrict__ w,
                  float* __restrict__ out)
{
    const int n = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * IW + (threadIdx.x >> 6)));
    const int lane = threadIdx.x & 63;
    if (n >= N) return;
    const int64_t* c = col + (size_t)n * K;
    const float* wr = w + (size_t)n * K;
    float acc[DV];
#pragma unroll
    for (int j = 0; j < DV; j++) acc[j] = 0.f;
    for (int k0 = 0; k0 < K; k0 += ISLOTS) {
        float v[ISLOTS][DV], wk[ISLOTS];
        bool ok[ISLOTS];
#pragma unroll
        for (int q = 0; q < ISLOTS; q++) {
            const int k = k0 + q;
            const int64_t a = k < K ? c[k] : -1;
            ok[q] = a >= 0 && a < A;
            wk[q] = ok[q] ? wr[k] : 0.f;
            const T* row = F + (ok[q] ? (size_t)a * D : 0);
#pragma unroll
            for (int j = 0; j < DV; j++) {
                const int d = lane + 64 * j;
                v[q][j] = (ok[q] && d < D) ? ld(row + d) : 0.f;
            }
        }
#pragma unroll
        for (int q = 0; q < ISLOTS; q++)            // slot order k = 0 .. K-1; a -1 or out-of-range slot adds nothing (not even 0 * NaN)
            if (ok[q]) {
#pragma unroll
                for (int j = 0; j < DV; j++) acc[j] = fmaf(wk[q], v[q][j], acc[j]);
            }
    }
    float* o = out + (size_t)n * D;
#pragma unroll
    for (int j = 0; j < DV; j++) {
        const int d = lane + 64 * j;
        if (d < D) o[d] = acc[j];
    }
}

static int interp_dv(int D) { return D <= 64 ? 1 : D <= 128 ? 2 : D <= 256 ? 4 : D <= 512 ? 8 : 16; }

template <typename T>
static hipError_t interp_fwd_t(hipStream_t s, int N, int K, int D, int A, const T* F, const int64_t* col, const float* w, float* out)
{
    const dim3 g((unsigned)((N + IW - 1) / IW)), b(IW * 64);
    switch (interp_dv(D)) {
    case 1: hipLaunchKernelGGL((interp_fwd_kernel<1, T>), g, b, 0, s, N, K, D, A, F, col, w, out); break;
    case 2: hipLaunchKernelGGL((interp_fwd_kernel<2, T>), g, b, 0, s, N, K, D, A, F, col, w, out); break;
    case 4: hipLaunchKernelGGL((interp_fwd_kernel<4, T>), g, b, 0, s, N, K, D, A, F, col, w, out); break;
    case 8: hipLaunchKernelGGL((interp_fwd_kernel<8, T>), g, b, 0, s, N, K, D, A, F, col, w, out); break;
    default: hipLaunchKernelGGL((interp_fwd_kernel<16, T>), g, b, 0, s, N, K, D, A, F, col, w, out); break;
    }
    return hipGetLastError();
}

static hipError_t launch_interp_fwd(hipStream_t s, int N, int K, int D, int A, int dtype, const void* F, const int64_t* col, const float* w,
                                    float* out)
{
    if (dtype == IGS_DTYPE_F16) return interp_fwd_t(s, N, K, D, A, (const _Float16*)F, col, w, out);
    return interp_fwd_t(s, N, K, D, A, (const float*)F, col, w, out);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (a) the inverse index: edges sorted by anchor, per-anchor starts and chunk offsets
// ---------------------------------------------------------------------------------------------------------------------------------
static size_t interp_scratch_bytes(int N, int K, int A, int D) { return InterpLayout(N, K, A, D).total; }

__global__ void __launch_bounds__(256)
interp_keys_kernel(uint32_t E, int A, const int64_t* __restrict__ col, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                   uint32_t* __restrict__ hist0, uint32_t per_block)
{
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const int64_t a = col[e];
    const uint32_t k = (a >= 0 && a < A) ? (uint32_t)a : (uint32_t)A;
    keys[e] = k; vals[e] = e;
    radix_count_first(hist0, e, per_block, k);
}

// start[a] for every a in (key[i - 1], key[i]]; the last position also closes (key[E - 1], A] with E
__global__ void __launch_bounds__(256)
interp_start_kernel(uint32_t E, int A, const uint32_t* __restrict__ sk, uint32_t* __restrict__ start)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= E) return;
    const int k = (int)sk[i];
    const int prev = i > 0 ? (int)sk[i - 1] : -1;
    for (int a = prev + 1; a <= k; a++) start[a] = i;
    if (i == E - 1)
        for (int a = k + 1; a <= A; a++) start[a] = E;
}

__global__ void __launch_bounds__(256)
interp_nchunks_kernel(int A, uint32_t chunk, const uint32_t* __restrict__ start, uint32_t* __restrict__ choff)
{
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a > A) return;
    choff[a] = a < A ? (start[a + 1] - start[a] + chunk - 1) / chunk : 0u;
}

static hipError_t launch_interp_index(hipStream_t s, int N, int K, int A, int D, const int64_t* col, void* scratch)
{
    const InterpLayout L(N, K, A, D);
    char* base = align_ptr((const char*)scratch);
    RadixBufs r = L.sort.at(base);
    uint32_t* start = (uint32_t*)(base + L.start);
    uint32_t* choff = (uint32_t*)(base + L.choff);
    const uint32_t E = (uint32_t)L.E;
    hipError_t e = radix_sort_begin(s, E, r);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(interp_keys_kernel, dim3((E + 255) / 256), dim3(256), 0, s, E, A, col, r.ka, r.va, r.hist, r.per_block);
    e = radix_sort_pairs(s, E, r, 0, L.bits);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(interp_start_kernel, dim3((E + 255) / 256), dim3(256), 0, s, E, A, (const uint32_t*)r.sorted_keys(L.bits), start);
    hipLaunchKernelGGL(interp_nchunks_kernel, dim3((unsigned)((A + 1 + 255) / 256)), dim3(256), 0, s, A, L.chunk, (const uint32_t*)start, choff);
    return launch_exclusive_scan(s, A + 1, choff);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (a) interpolation backward
// ---------------------------------------------------------------------------------------------------------------------------------
// one wave per chunk c of the sorted edges: anchor a = the last a with choff[a] <= c (a non-empty list), edges
// [start[a] + j * chunk, min(start[a + 1], start[a] + (j + 1) * chunk)), j = c - choff[a].  A list of one chunk writes dF[a] directly.
template <int DV, typename T>
__global__ void __launch_bounds__(IW * 64)
interp_chunk_kernel(int K, int D, int A, uint32_t chunk, const T* __restrict__ F, const float* __restrict__ w,
                    const float* __restrict__ dout, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ start,
                    const uint32_t* __restrict__ choff, float* __restrict__ part, T* __restrict__ dF, float* __restrict__ dw)
{
    const uint32_t c = __builtin_amdgcn_readfirstlane(blockIdx.x * IW + (threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    if (c >= choff[A]) return;
    int lo = 0, hi = A - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (choff[mid] <= c) lo = mid; else hi = mid - 1;
    }
    const int a = lo;
    const uint32_t j = c - choff[a], nch = choff[a + 1] - choff[a];
    const uint32_t beg = start[a] + j * chunk, end = min(start[a + 1], beg + chunk);
    float fr[DV], acc[DV];
#pragma unroll
    for (int q = 0; q < DV; q++) {
        const int d = lane + 64 * q;
        fr[q] = (dw && d < D) ? ld(F + (size_t)a * D + d) : 0.f;
        acc[q] = 0.f;
    }
    for (uint32_t p0 = beg; p0 < end; p0 += ISLOTS) {
        float g[ISLOTS][DV], wt[ISLOTS];
        uint32_t ed[ISLOTS];
#pragma unroll
        for (int q = 0; q < ISLOTS; q++) {
            const uint32_t p = p0 + q;
            const bool ok = p < end;
            ed[q] = ok ? perm[p] : 0u;
            const uint32_t n = ed[q] / (uint32_t)K;
            wt[q] = ok ? w[ed[q]] : 0.f;
#pragma unroll
            for (int v = 0; v < DV; v++) {
                const int d = lane + 64 * v;
                g[q][v] = (ok && d < D) ? dout[(size_t)n * D + d] : 0.f;
            }
        }
#pragma unroll
        for (int q = 0; q < ISLOTS; q++) {
            if (p0 + q >= end) break;
            if (dF) {
#pragma unroll
                for (int v = 0; v < DV; v++) acc[v] = fmaf(wt[q], g[q][v], acc[v]);
            }
            if (dw) {
                float t = 0.f;
#pragma unroll
                for (int v = 0; v < DV; v++) t = fmaf(g[q][v], fr[v], t);
                t = lane_sum<64>(t);
                if (lane == 0) dw[ed[q]] = t;
            }
        }
    }
    if (!dF) return;
#pragma unroll
    for (int v = 0; v < DV; v++) {
        const int d = lane + 64 * v;
        if (d >= D) continue;
        if (nch == 1) st(dF + (size_t)a * D + d, acc[v]);
        else part[(size_t)c * D + d] = acc[v];
    }
}

// dF[a, d] = the anchor's chunk partials added in chunk order (lists of one chunk were written by the chunk kernel; empty lists: 0)
template <typename T>
__global__ void __launch_bounds__(256)
interp_fold_kernel(int A, int D, const uint32_t* __restrict__ choff, const float* __restrict__ part, T* __restrict__ dF)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)A * D) return;
    const int a = (int)(i / D), d = (int)(i % D);
    const uint32_t c0 = choff[a], c1 = choff[a + 1];
    if (c1 - c0 == 1) return;
    float s = 0.f;
    for (uint32_t c = c0; c < c1; c++) s += part[(size_t)c * D + d];
    st(dF + i, s);
}

template <typename T>
static hipError_t interp_bwd_t(hipStream_t s, int N, int K, int D, int A, const T* F, const float* w, const float* dout,
                               void* scratch, T* dF, float* dw)
{
    const InterpLayout L(N, K, A, D);
    char* base = align_ptr((const char*)scratch);
    const uint32_t* perm = L.sort.at(base).sorted_vals(L.bits);
    const uint32_t* start = (const uint32_t*)(base + L.start);
    const uint32_t* choff = (const uint32_t*)(base + L.choff);
    float* part = (float*)(base + L.part);
    if (dw) {      // slots that contribute nothing get a zero gradient (the chunks never visit them)
        hipError_t e = zero_fill_async(s, dw, (size_t)L.E * 4);
        if (e != hipSuccess) return e;
    }
    const dim3 g((unsigned)((L.max_chunks + IW - 1) / IW)), b(IW * 64);
    switch (interp_dv(D)) {
    case 1: hipLaunchKernelGGL((interp_chunk_kernel<1, T>), g, b, 0, s, K, D, A, L.chunk, F, w, dout, perm, start, choff, part, dF, dw); break;
    case 2: hipLaunchKernelGGL((interp_chunk_kernel<2, T>), g, b, 0, s, K, D, A, L.chunk, F, w, dout, perm, start, choff, part, dF, dw); break;
    case 4: hipLaunchKernelGGL((interp_chunk_kernel<4, T>), g, b, 0, s, K, D, A, L.chunk, F, w, dout, perm, start, choff, part, dF, dw); break;
    case 8: hipLaunchKernelGGL((interp_chunk_kernel<8, T>), g, b, 0, s, K, D, A, L.chunk, F, w, dout, perm, start, choff, part, dF, dw); break;
    default: hipLaunchKernelGGL((interp_chunk_kernel<16, T>), g, b, 0, s, K, D, A, L.chunk, F, w, dout, perm, start, choff, part, dF, dw); break;
    }
    if (dF) {
        const size_t n = (size_t)A * D;
        hipLaunchKernelGGL((interp_fold_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, A, D, choff, (const float*)part, dF);
    }
    return hipGetLastError();
}

static hipError_t launch_interp_bwd(hipStream_t s, int N, int K, int D, int A, int dtype, const void* F, const float* w, const float* dout,
                                    void* scratch, void* dF, float* dw)
{
    if (dtype == IGS_DTYPE_F16) return interp_bwd_t(s, N, K, D, A, (const _Float16*)F, w, dout, scratch, (_Float16*)dF, dw);
    return interp_bwd_t(s, N, K, D, A, (const float*)F, w, dout, scratch, (float*)dF, dw);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (b) Gaussian deform
// ---------------------------------------------------------------------------------------------------------------------------------
#define DEFORM_EPS 1e-12f             // F.normalize's eps

struct Quat { float w, x, y, z; };
__device__ __forceinline__ Quat qload(const float* p) { return { p[0], p[1], p[2], p[3] }; }
template <typename T> __device__ __forceinline__ Quat qload_t(const T* p) { return { ld(p), ld(p + 1), ld(p + 2), ld(p + 3) }; }
__device__ __forceinline__ float qnorm(const Quat& q) { return sqrtf(fmaf(q.z, q.z, fmaf(q.y, q.y, fmaf(q.x, q.x, q.w * q.w)))); }
__device__ __forceinline__ Quat qscale(const Quat& q, float s) { return { q.w * s, q.x * s, q.y * s, q.z * s }; }
// F.normalize: q / max(|q|, eps)
__device__ __forceinline__ Quat qnrm(const Quat& q, float& r) { r = fmaxf(qnorm(q), DEFORM_EPS); return { q.w / r, q.x / r, q.y / r, q.z / r }; }
// Hamilton product in quaternion_multiply's order (general_utils.py:196-199)
__device__ __forceinline__ Quat qmul(const Quat& a, const Quat& b)
{
    return { a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z,
             a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
             a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z,
             a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x };
}
// gradient of F.normalize at q (|q| = nq, r = max(nq, eps), n = q / r) for the output gradient g: (g - n <n, g>) / |q| where the norm
// passes the clamp, g / eps below it (the clamp's gradient is zero there: division by a constant)
__device__ __forceinline__ Quat qnrm_bwd(const Quat& q, const Quat& n, float r, const Quat& g)
{
    if (qnorm(q) < DEFORM_EPS) return qscale(g, 1.f / DEFORM_EPS);
    const float t = n.w * g.w + n.x * g.x + n.y * g.y + n.z * g.z;
    return { (g.w - n.w * t) / r, (g.x - n.x * t) / r, (g.y - n.y * t) / r, (g.z - n.z * t) / r };
}

// pass-through rows: dst0 <- src0 (n0 floats), dst1 <- src1 (n1 floats), either pair may be absent
__global__ void __launch_bounds__(256)
copy2_kernel(size_t n0, const float* __restrict__ src0, float* __restrict__ dst0, size_t n1, const float* __restrict__ src1,
             float* __restrict__ dst1)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n0) dst0[i] = src0[i];
    else if (i - n0 < n1) dst1[i - n0] = src1[i - n0];
}

static hipError_t launch_copy2(hipStream_t s, size_t n0, const float* src0, float* dst0, size_t n1, const float* src1, float* dst1)
{
    if (!dst0 || dst0 == src0) n0 = 0;
    if (!dst1 || dst1 == src1) n1 = 0;
    if (n0 + n1 == 0) return hipSuccess;
    hipLaunchKernelGGL(copy2_kernel, dim3((unsigned)((n0 + n1 + 255) / 256)), dim3(256), 0, s, n0, src0, dst0, n1, src1, dst1);
    return hipGetLastError();
}

template <typename T>
__global__ void __launch_bounds__(256)
deform_fwd_kernel(int P, int M, const float* __restrict__ xyz, const float* __restrict__ rot, const int64_t* __restrict__ mask,
                  const T* __restrict__ dxyz, const T* __restrict__ drot, float* __restrict__ xyz_out, float* __restrict__ rot_out)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    const int64_t i = mask[j];
    if (i < 0 || i >= P) return;                // (the entry point's contract excludes it; no write outside the rows)
#pragma unroll
    for (int a = 0; a < 3; a++) xyz_out[3 * i + a] = xyz[3 * i + a] + ld(dxyz + 3 * (size_t)j + a);
    float ra, rb;
    const Quat q = qmul(qnrm(qload(rot + 4 * i), ra), qnrm(qload_t(drot + 4 * (size_t)j), rb));
    float* o = rot_out + 4 * i;
    o[0] = q.w; o[1] = q.x; o[2] = q.y; o[3] = q.z;
}

static hipError_t launch_deform_fwd(hipStream_t s, int P, int M, int dtype, const float* xyz, const float* rot, const int64_t* mask,
                                    const void* dxyz, const void* drot, float* xyz_out, float* rot_out)
{
    hipError_t e = launch_copy2(s, (size_t)P * 3, xyz, xyz_out, (size_t)P * 4, rot, rot_out);
    if (e != hipSuccess || M == 0) return e;
    const dim3 g((M + 255) / 256);
    if (dtype == IGS_DTYPE_F16)
        hipLaunchKernelGGL((deform_fwd_kernel<_Float16>), g, dim3(256), 0, s, P, M, xyz, rot, mask, (const _Float16*)dxyz, (const _Float16*)drot, xyz_out, rot_out);
    else
        hipLaunchKernelGGL((deform_fwd_kernel<float>), g, dim3(256), 0, s, P, M, xyz, rot, mask, (const float*)dxyz, (const float*)drot, xyz_out, rot_out);
    return hipGetLastError();
}

template <typename T>
__global__ void __launch_bounds__(256)
deform_bwd_kernel(int P, int M, const float* __restrict__ rot, const int64_t* __restrict__ mask, const T* __restrict__ drot,
                  const float* __restrict__ g_xyz, const float* __restrict__ g_rot, float* __restrict__ d_rot, T* __restrict__ d_dxyz,
                  T* __restrict__ d_drot)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    const int64_t i = mask[j];
    if (i < 0 || i >= P) {                      // a skipped row took no part in the forward: its residuals' gradients are zero
        if (d_dxyz) {
#pragma unroll
            for (int a = 0; a < 3; a++) st(d_dxyz + 3 * (size_t)j + a, 0.f);
        }
        if (d_drot) {
#pragma unroll
            for (int a = 0; a < 4; a++) st(d_drot + 4 * (size_t)j + a, 0.f);
        }
        return;
    }
    if (d_dxyz) {
#pragma unroll
        for (int a = 0; a < 3; a++) st(d_dxyz + 3 * (size_t)j + a, g_xyz ? g_xyz[3 * i + a] : 0.f);
    }
    if (!d_rot && !d_drot) return;
    const Quat g = g_rot ? qload(g_rot + 4 * i) : Quat{ 0.f, 0.f, 0.f, 0.f };
    const Quat qa = qload(rot + 4 * i), qb = qload_t(drot + 4 * (size_t)j);
    float ra, rb;
    const Quat p = qnrm(qa, ra), q = qnrm(qb, rb);
    if (d_rot) {      // d<g, p (x) q>/dp
        const Quat gp = { g.w * q.w + g.x * q.x + g.y * q.y + g.z * q.z,
                          -g.w * q.x + g.x * q.w - g.y * q.z + g.z * q.y,
                          -g.w * q.y + g.x * q.z + g.y * q.w - g.z * q.x,
                          -g.w * q.z - g.x * q.y + g.y * q.x + g.z * q.w };
        const Quat r = qnrm_bwd(qa, p, ra, gp);
        float* o = d_rot + 4 * i;
        o[0] = r.w; o[1] = r.x; o[2] = r.y; o[3] = r.z;
    }
    if (d_drot) {     // d<g, p (x) q>/dq
        const Quat gq = { g.w * p.w + g.x * p.x + g.y * p.y + g.z * p.z,
                          -g.w * p.x + g.x * p.w + g.y * p.z - g.z * p.y,
                          -g.w * p.y - g.x * p.z + g.y * p.w + g.z * p.x,
                          -g.w * p.z + g.x * p.y - g.y * p.x + g.z * p.w };
        const Quat r = qnrm_bwd(qb, q, rb, gq);
        T* o = d_drot + 4 * (size_t)j;
        st(o, r.w); st(o + 1, r.x); st(o + 2, r.y); st(o + 3, r.z);
    }
}

static hipError_t launch_deform_bwd(hipStream_t s, int P, int M, int dtype, const float* rot, const int64_t* mask, const void* drot,
                                    const float* g_xyz, const float* g_rot, float* d_xyz, float* d_rot, void* d_dxyz, void* d_drot)
{
    // pass-through: d_xyz = g_xyz everywhere, d_rot = g_rot outside the mask (a missing upstream gradient is zero)
    hipError_t e = hipSuccess;
    if (d_xyz && !g_xyz) e = zero_fill_async(s, d_xyz, (size_t)P * 12);
    if (e == hipSuccess && d_rot && !g_rot) e = zero_fill_async(s, d_rot, (size_t)P * 16);
    if (e != hipSuccess) return e;
    e = launch_copy2(s, g_xyz ? (size_t)P * 3 : 0, g_xyz, d_xyz, g_rot ? (size_t)P * 4 : 0, g_rot, d_rot);
    if (e != hipSuccess || M == 0) return e;
    const dim3 g((M + 255) / 256);
    if (dtype == IGS_DTYPE_F16)
        hipLaunchKernelGGL((deform_bwd_kernel<_Float16>), g, dim3(256), 0, s, P, M, rot, mask, (const _Float16*)drot, g_xyz, g_rot, d_rot,
                           (_Float16*)d_dxyz, (_Float16*)d_drot);
    else
        hipLaunchKernelGGL((deform_bwd_kernel<float>), g, dim3(256), 0, s, P, M, rot, mask, (const float*)drot, g_xyz, g_rot, d_rot,
                           (float*)d_dxyz, (float*)d_drot);
    return hipGetLastError();
}

// the entry points (the contracts are in include/igs_rast.h)
static const char* interp_size_error(int N, int K, int D, int A)
{
    if (N < 0 || N > IGS_INTERP_MAX_ROWS) return "N out of range (0..IGS_INTERP_MAX_ROWS)";
    if (K < 1 || K > IGS_INTERP_MAX_K) return "K out of range (1..IGS_INTERP_MAX_K)";
    if (D < 1 || D > IGS_INTERP_MAX_D) return "D out of range (1..IGS_INTERP_MAX_D)";
    if (A < 1 || A > IGS_INTERP_MAX_ANCHORS) return "A_total out of range (1..IGS_INTERP_MAX_ANCHORS)";
    if ((long long)N * K > IGS_INTERP_MAX_EDGES) return "N * K out of range (IGS_INTERP_MAX_EDGES)";
    return nullptr;
}
extern "C" int igs_anchor_interp_fwd(void* stream, int N, int K, int D, int A_total, int dtype, const void* F, const int64_t* col,
                                     const float* w, float* out)
{
    if (const char* e = interp_size_error(N, K, D, A_total)) return fail_in("igs_anchor_interp_fwd", e);
    if (!dtype_ok(dtype)) return fail(IGS_RAST_E_INVALID, "igs_anchor_interp_fwd: unknown dtype code");
    if (N == 0) return 0;
    if (!F || !col || !w || !out) return fail(IGS_RAST_E_INVALID, "igs_anchor_interp_fwd: NULL pointer");
    HIP_TRY(launch_interp_fwd((hipStream_t)stream, N, K, D, A_total, dtype, F, col, w, out), "anchor interp fwd launch");
    return 0;
}
extern "C" size_t igs_anchor_interp_index_bytes(int N, int K, int A_total, int D)
{
    if (interp_size_error(N, K, D, A_total)) return 0;
    return interp_scratch_bytes(N, K, A_total, D) + 256;
}
extern "C" int igs_anchor_interp_index(void* stream, int N, int K, int A_total, int D, const int64_t* col, void* scratch)
{
    if (const char* e = interp_size_error(N, K, D, A_total)) return fail_in("igs_anchor_interp_index", e);
    if (N == 0) return 0;
    if (!col || !scratch) return fail(IGS_RAST_E_INVALID, "igs_anchor_interp_index: NULL pointer");
    HIP_TRY(launch_interp_index((hipStream_t)stream, N, K, A_total, D, col, scratch), "anchor interp index launch");
    return 0;
}
extern "C" int igs_anchor_interp_bwd(void* stream, int N, int K, int D, int A_total, int dtype, const void* F, const float* w,
                                     const float* dout, void* scratch, void* dF, float* dw)
{
    if (const char* e = interp_size_error(N, K, D, A_total)) return fail_in("igs_anchor_interp_bwd", e);
    if (!dtype_ok(dtype)) return fail(IGS_RAST_E_INVALID, "igs_anchor_interp_bwd: unknown dtype code");
    if (!dF && !dw) return 0;
    if (N == 0) {       // no edges: every anchor's gradient is zero
        if (dF) HIP_TRY(zero_fill_async((hipStream_t)stream, dF, (size_t)A_total * D * (dtype == IGS_DTYPE_F16 ? 2 : 4)), "zero dF");
        return 0;
    }
    if (!w || !dout || !scratch || (dw && !F)) return fail(IGS_RAST_E_INVALID, "igs_anchor_interp_bwd: NULL pointer");
    HIP_TRY(launch_interp_bwd((hipStream_t)stream, N, K, D, A_total, dtype, F, w, dout, scratch, dF, dw), "anchor interp bwd launch");
    return 0;
}
extern "C" int igs_gaussian_deform_fwd(void* stream, int P, int M, int dtype, const float* xyz, const float* rot, const int64_t* mask,
                                       const void* dxyz, const void* drot, float* xyz_out, float* rot_out)
{
    if (P < 0 || P > IGS_DEFORM_MAX_POINTS) return fail(IGS_RAST_E_INVALID, "igs_gaussian_deform_fwd: P out of range (0..IGS_DEFORM_MAX_POINTS)");
    if (M < 0 || M > P) return fail(IGS_RAST_E_INVALID, "igs_gaussian_deform_fwd: M out of range (0..P)");
    if (!dtype_ok(dtype)) return fail(IGS_RAST_E_INVALID, "igs_gaussian_deform_fwd: unknown dtype code");
    if (P == 0) return 0;
    if (!xyz || !rot || !xyz_out || !rot_out || (M > 0 && (!mask || !dxyz || !drot)))
        return fail(IGS_RAST_E_INVALID, "igs_gaussian_deform_fwd: NULL pointer");
    HIP_TRY(launch_deform_fwd((hipStream_t)stream, P, M, dtype, xyz, rot, mask, dxyz, drot, xyz_out, rot_out), "gaussian deform fwd launch");
    return 0;
}
extern "C" int igs_gaussian_deform_bwd(void* stream, int P, int M, int dtype, const float* rot, const int64_t* mask, const void* drot,
                                       const float* g_xyz, const float* g_rot, float* d_xyz, float* d_rot, void* d_dxyz, void* d_drot)
{
    if (P < 0 || P > IGS_DEFORM_MAX_POINTS) return fail(IGS_RAST_E_INVALID, "igs_gaussian_deform_bwd: P out of range (0..IGS_DEFORM_MAX_POINTS)");
    if (M < 0 || M > P) return fail(IGS_RAST_E_INVALID, "igs_gaussian_deform_bwd: M out of range (0..P)");
    if (!dtype_ok(dtype)) return fail(IGS_RAST_E_INVALID, "igs_gaussian_deform_bwd: unknown dtype code");
    if (P == 0 || (!d_xyz && !d_rot && !d_dxyz && !d_drot)) return 0;
    if (M > 0 && (!mask || ((d_rot || d_drot) && (!rot || !drot))))
        return fail(IGS_RAST_E_INVALID, "igs_gaussian_deform_bwd: NULL pointer");
    HIP_TRY(launch_deform_bwd((hipStream_t)stream, P, M, dtype, rot, mask, drot, g_xyz, g_rot, d_xyz, d_rot, d_dxyz, d_drot),
            "gaussian deform bwd launch");
    return 0;
}
