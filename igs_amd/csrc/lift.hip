// lift.hip -- multi-view anchor feature lifting for gfx950: GridEncoder.forward's "perspective_projection" branch
// (igs/models/grid_encoder.py:66-88 over perspective_projection, igs/utils/ops.py:444-477).  include/igs_rast.h states the contract,
// DESIGN.md section 14 the byte budget and the figures.
//
//   out[b, a, c] = (1 / V) * sum_v bilinear_zero_pad(feat[b * V + v, c], ix, iy),   (ix, iy) = the projection of points[b, a] by view v
//
// The features are NCHW: the C channels of one bilinear corner lie H * W elements apart, so a gather with lanes across channels would
// touch one cache line per useful element.  Instead the work is plane-major:
//   (1) lift_project_kernel, one thread per (b, v, a): the projection once, into a sample table (cell, tx, ty) that all channels reuse;
//   (2) lift_fwd_kernel, one workgroup per (b, channel, chunk of LIFT_CHUNK anchors): each of the V planes of that channel is brought
//       into LDS by coalesced row loads (in bands of whole rows when it is larger than the LDS budget), the threads take the four
//       corners of their anchors from LDS, the views are accumulated in registers in view order, out[b, c, a0 ..] is one contiguous run;
//   (3) backward without float atomics: the (sample, corner) edges e = 4 * s + corner are stably sorted by the pixel they touch (the
//       library's radix sort), so a pixel's incoming edges are in ascending (a, corner) order; lift_edge_kernel leaves (anchor, weight)
//       per sorted edge; lift_bwd_kernel, one workgroup per (b, v, LIFT_BWD_CH channels), holds d out[b, c, :] in LDS and every thread
//       sums the edges of its pixels in list order and writes d feat coalesced, every element (zero where no sample landed).
#include "common.h"
#include "elem_common.h"
#include "host_api.h"

#define LIFT_THREADS 512              // forward workgroup
#define LIFT_APT 8                    // anchors per thread, accumulated in registers
#define LIFT_CHUNK (LIFT_THREADS * LIFT_APT)
#define LIFT_LDS_FLOATS 16384         // 64 KB: one 128 x 128 float plane; two workgroups share a CU's 160 KB
#define LIFT_BWD_THREADS 1024
#define LIFT_BWD_CH 2                 // channels per backward workgroup: 2 x 8192 anchors of d out = 64 KB
#define LIFT_OUTSIDE 0xFFFFFFFFu      // cell mark of a sample that touches no pixel (or is not finite)

// corner q of a sample: 0 = (x0, y0), 1 = (x0 + 1, y0), 2 = (x0, y0 + 1), 3 = (x0 + 1, y0 + 1); tx = ix - x0, ty = iy - y0
__device__ __forceinline__ float lift_weight(int q, float tx, float ty)
{
    const float wx = (q & 1) ? tx : 1.f - tx, wy = (q & 2) ? ty : 1.f - ty;
    return wx * wy;
}

struct LiftLayout {            // offsets from a 256-byte aligned base; the index part only when `backward`
    size_t cell, tx, ty, start, total;
    RadixOffsets sort = {};    // edges by pixel (backward only)
    uint64_t S, E, NPIX;
    int bits;
    LiftLayout(int B, int V, int A, int H, int W, bool backward) {
        S = (uint64_t)B * V * A;
        E = 4 * S;
        NPIX = (uint64_t)B * V * H * W;
        bits = 1;
        while (((uint64_t)1 << bits) <= NPIX) bits++;              // keys 0 .. NPIX (NPIX = a corner outside the map)
        size_t o = 0;
        cell = o; o += align_up(S * 4, 256);
        tx = o;   o += align_up(S * 4, 256);
        ty = o;   o += align_up(S * 4, 256);
        start = o;
        if (backward) {
            sort = radix_layout_append(o, E);
            start = o; o += align_up((NPIX + 1) * 4, 256);        // start[p]: first sorted edge of pixel p; start[NPIX] = valid edges
        }
        total = o + 256;
    }
};

static size_t lift_scratch_bytes(int B, int V, int A, int H, int W, bool backward) { return LiftLayout(B, V, A, H, W, backward).total; }

// ---------------------------------------------------------------------------------------------------------------------------------
// (1) the sample table
// ---------------------------------------------------------------------------------------------------------------------------------
// The reference's arithmetic: p_cam = R p + T; K p_cam, then the division by its z; 2 u / W - 1; grid_sample's ((g + 1) W - 1) / 2.
__global__ void __launch_bounds__(256)
lift_project_kernel(int V, int A, int H, int W, uint32_t S, const float* __restrict__ points, const float* __restrict__ w2c,
                    const float* __restrict__ intr, uint32_t* __restrict__ cell, float* __restrict__ tx, float* __restrict__ ty)
{
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= S) return;
    const uint32_t bv = s / (uint32_t)A, a = s - bv * (uint32_t)A, b = bv / (uint32_t)V;
    const float* p = points + ((size_t)b * A + a) * 3;
    const float* m = w2c + (size_t)bv * 16;
    const float* k = intr + (size_t)bv * 4;
    const float px = p[0], py = p[1], pz = p[2];
    const float xc = m[0] * px + m[1] * py + m[2] * pz + m[3];
    const float yc = m[4] * px + m[5] * py + m[6] * pz + m[7];
    const float zc = m[8] * px + m[9] * py + m[10] * pz + m[11];
    const float u = (k[0] * xc + k[2] * zc) / zc;            // no culling: a negative z divides like any other
    const float v = (k[1] * yc + k[3] * zc) / zc;
    const float gx = 2.f * u / (float)W - 1.f, gy = 2.f * v / (float)H - 1.f;
    const float ix = ((gx + 1.f) * (float)W - 1.f) / 2.f, iy = ((gy + 1.f) * (float)H - 1.f) / 2.f;
    // range test in float before any conversion to integer; NaN fails every comparison, +-inf the bounds
    const bool in = ix > -1.f && ix < (float)W && iy > -1.f && iy < (float)H;
    uint32_t c = LIFT_OUTSIDE;
    float fx = 0.f, fy = 0.f;
    if (in) {
        const float x0 = floorf(ix), y0 = floorf(iy);          // in [-1, W - 1] x [-1, H - 1]
        fx = ix - x0; fy = iy - y0;                            // exact
        c = ((uint32_t)((int)y0 + 1) << 16) | (uint32_t)((int)x0 + 1);
    }
    cell[s] = c; tx[s] = fx; ty[s] = fy;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (2) forward
// ---------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(LIFT_THREADS)
lift_fwd_kernel(int V, int A, int C, int H, int W, int band_rows, int nchunk, const T* __restrict__ feat, size_t fs_n, size_t fs_c,
                const uint32_t* __restrict__ cell, const float* __restrict__ tx, const float* __restrict__ ty, float* __restrict__ out,
                size_t os_a, size_t os_c)
{
    extern __shared__ __attribute__((aligned(16))) float plane[];
    const int tid = threadIdx.x;
    const int chunk = blockIdx.x % nchunk;
    const int c = (blockIdx.x / nchunk) % C;
    const int b = blockIdx.x / (nchunk * C);
    const int a0 = chunk * LIFT_CHUNK;
    float acc[LIFT_APT];
#pragma unroll
    for (int j = 0; j < LIFT_APT; j++) acc[j] = 0.f;
    for (int v = 0; v < V; v++) {
        const size_t bv = (size_t)b * V + v;
        const T* src = feat + bv * fs_n + (size_t)c * fs_c;
        uint32_t cl[LIFT_APT];
        float fx[LIFT_APT], fy[LIFT_APT];
#pragma unroll
        for (int j = 0; j < LIFT_APT; j++) {
            const int a = a0 + j * LIFT_THREADS + tid;
            const bool ok = a < A;
            const size_t s = bv * A + (ok ? a : 0);
            cl[j] = ok ? cell[s] : LIFT_OUTSIDE;
            fx[j] = ok ? tx[s] : 0.f;
            fy[j] = ok ? ty[s] : 0.f;
        }
        for (int r0 = 0; r0 < H; r0 += band_rows) {
            const int rows = min(band_rows, H - r0);
            const int n = rows * W;
            __syncthreads();                                   // the previous band's gathers are done
            const T* band = src + (size_t)r0 * W;
            int done = 0;                                      // four elements per lane where the band starts on a 16- / 8-byte boundary
            if ((((uintptr_t)band) & (4 * sizeof(T) - 1)) == 0) {
                const int n4 = n >> 2;
                for (int i = tid; i < n4; i += LIFT_THREADS) {
                    float4 f;
                    if constexpr (sizeof(T) == 4) f = ((const float4*)band)[i];
                    else {
                        const h4_t h = ((const h4_t*)band)[i];
                        f = make_float4((float)h.x, (float)h.y, (float)h.z, (float)h.w);
                    }
                    ((float4*)plane)[i] = f;
                }
                done = n4 << 2;
            }
            for (int i = done + tid; i < n; i += LIFT_THREADS) plane[i] = ld(band + i);
            __syncthreads();
#pragma unroll
            for (int j = 0; j < LIFT_APT; j++) {
                if (cl[j] == LIFT_OUTSIDE) continue;
                const int x0 = (int)(cl[j] & 0xFFFFu) - 1, y0 = (int)(cl[j] >> 16) - 1;
#pragma unroll
                for (int q = 0; q < 4; q++) {                  // corner order 0 .. 3; a corner outside the map or the band adds nothing
                    const int x = x0 + (q & 1), y = y0 + (q >> 1) - r0;
                    if (x >= 0 && x < W && y >= 0 && y < rows) acc[j] = fmaf(lift_weight(q, fx[j], fy[j]), plane[y * W + x], acc[j]);
                }
            }
        }
    }
    float* o = out + ((size_t)b * A * C) + (size_t)c * os_c;
#pragma unroll
    for (int j = 0; j < LIFT_APT; j++) {
        const int a = a0 + j * LIFT_THREADS + tid;
        if (a < A) o[(size_t)a * os_a] = acc[j] / (float)V;
    }
}

static int lift_band_rows(int H, int W) { const int r = LIFT_LDS_FLOATS / W; return r < H ? r : H; }

static hipError_t launch_lift_fwd(hipStream_t s, int B, int V, int A, int C, int H, int W, int dtype, const void* feat, size_t fs_n, size_t fs_c,
                                  const float* points, const float* w2c, const float* intr, float* out, size_t os_a, size_t os_c, void* scratch)
{
    const LiftLayout L(B, V, A, H, W, false);
    char* base = align_ptr((const char*)scratch);
    uint32_t* cell = (uint32_t*)(base + L.cell);
    float *tx = (float*)(base + L.tx), *ty = (float*)(base + L.ty);
    const uint32_t S = (uint32_t)L.S;
    hipLaunchKernelGGL(lift_project_kernel, dim3((S + 255) / 256), dim3(256), 0, s, V, A, H, W, S, points, w2c, intr, cell, tx, ty);
    const int band = lift_band_rows(H, W), nchunk = (A + LIFT_CHUNK - 1) / LIFT_CHUNK;
    const size_t lds = (size_t)band * W * 4;
    const dim3 g((unsigned)((size_t)B * C * nchunk)), blk(LIFT_THREADS);
    if (dtype == IGS_DTYPE_F16)
        hipLaunchKernelGGL((lift_fwd_kernel<_Float16>), g, blk, lds, s, V, A, C, H, W, band, nchunk, (const _Float16*)feat, fs_n, fs_c,
                           (const uint32_t*)cell, (const float*)tx, (const float*)ty, out, os_a, os_c);
    else
        hipLaunchKernelGGL((lift_fwd_kernel<float>), g, blk, lds, s, V, A, C, H, W, band, nchunk, (const float*)feat, fs_n, fs_c,
                           (const uint32_t*)cell, (const float*)tx, (const float*)ty, out, os_a, os_c);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (3) backward
// ---------------------------------------------------------------------------------------------------------------------------------
// edge e = 4 * s + corner, key = the pixel it touches (bv * H * W + y * W + x) or NPIX; the first radix pass's digit counts on the way
__global__ void __launch_bounds__(256)
lift_keys_kernel(uint32_t E, int A, int H, int W, uint32_t NPIX, const uint32_t* __restrict__ cell, uint32_t* __restrict__ keys,
                 uint32_t* __restrict__ vals, uint32_t* __restrict__ hist0, uint32_t per_block)
{
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const uint32_t s = e >> 2, q = e & 3u, cl = cell[s];
    uint32_t k = NPIX;
    if (cl != LIFT_OUTSIDE) {
        const int x = (int)(cl & 0xFFFFu) - 1 + (int)(q & 1u), y = (int)(cl >> 16) - 1 + (int)(q >> 1);
        if (x >= 0 && x < W && y >= 0 && y < H) k = (s / (uint32_t)A) * (uint32_t)(H * W) + (uint32_t)(y * W + x);
    }
    keys[e] = k; vals[e] = e;
    radix_count_first(hist0, e, per_block, k);
}

// start[p] = the first sorted position whose key is >= p, for p = 0 .. NPIX: a lower bound per pixel.  (motion.hip's boundary walk fills
// the gap between two neighbouring keys in one thread: fine for dense anchor keys, serial over the whole map when few samples land.)
__global__ void __launch_bounds__(256)
lift_start_kernel(uint32_t E, uint32_t NPIX, const uint32_t* __restrict__ sk, uint32_t* __restrict__ start)
{
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p > NPIX) return;
    uint32_t lo = 0, hi = E;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (sk[mid] < p) lo = mid + 1; else hi = mid;
    }
    start[p] = lo;
}

// per sorted edge: its anchor and its bilinear weight (the channels share them)
__global__ void __launch_bounds__(256)
lift_edge_kernel(uint32_t E, int A, const uint32_t* __restrict__ perm, const float* __restrict__ tx, const float* __restrict__ ty,
                 uint32_t* __restrict__ ea, float* __restrict__ ew)
{
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= E) return;
    const uint32_t e = perm[j], s = e >> 2;
    ea[j] = s % (uint32_t)A;
    ew[j] = lift_weight((int)(e & 3u), tx[s], ty[s]);
}

template <typename T>
__global__ void __launch_bounds__(LIFT_BWD_THREADS)
lift_bwd_kernel(int V, int A, int C, int HW, int ncg, int use_lds, const uint32_t* __restrict__ start, const uint32_t* __restrict__ ea,
                const float* __restrict__ ew, const float* __restrict__ dout, size_t gs_a, size_t gs_c, T* __restrict__ dfeat, size_t fs_n,
                size_t fs_c)
{
    extern __shared__ __attribute__((aligned(16))) float gl[];
    const int tid = threadIdx.x;
    const int cg = blockIdx.x % ncg;
    const int v = (blockIdx.x / ncg) % V;
    const int b = blockIdx.x / (ncg * V);
    const int c0 = cg * LIFT_BWD_CH;
    const size_t bv = (size_t)b * V + v;
    const float* g = dout + (size_t)b * A * C;
    if (use_lds) {
#pragma unroll
        for (int ch = 0; ch < LIFT_BWD_CH; ch++)
            if (c0 + ch < C)
                for (int a = tid; a < A; a += LIFT_BWD_THREADS) gl[ch * A + a] = g[(size_t)a * gs_a + (size_t)(c0 + ch) * gs_c];
        __syncthreads();
    }
    const uint32_t* first = start + bv * HW;
    for (int p = tid; p < HW; p += LIFT_BWD_THREADS) {
        const uint32_t lo = first[p], hi = first[p + 1];
        float acc[LIFT_BWD_CH];
#pragma unroll
        for (int ch = 0; ch < LIFT_BWD_CH; ch++) acc[ch] = 0.f;
        for (uint32_t j = lo; j < hi; j++) {                   // ascending (a, corner): the stable sort kept the edge order
            const uint32_t a = ea[j];
            const float w = ew[j];
#pragma unroll
            for (int ch = 0; ch < LIFT_BWD_CH; ch++) {
                if (c0 + ch >= C) continue;
                const float gv = use_lds ? gl[ch * A + a] : g[(size_t)a * gs_a + (size_t)(c0 + ch) * gs_c];
                acc[ch] = fmaf(w, gv, acc[ch]);
            }
        }
#pragma unroll
        for (int ch = 0; ch < LIFT_BWD_CH; ch++)
            if (c0 + ch < C) st(dfeat + bv * fs_n + (size_t)(c0 + ch) * fs_c + p, acc[ch] / (float)V);
    }
}

static hipError_t launch_lift_bwd(hipStream_t s, int B, int V, int A, int C, int H, int W, int dtype, const float* points, const float* w2c,
                                  const float* intr, const float* dout, size_t gs_a, size_t gs_c, void* dfeat, size_t fs_n, size_t fs_c,
                                  void* scratch)
{
    const LiftLayout L(B, V, A, H, W, true);
    char* base = align_ptr((const char*)scratch);
    uint32_t* cell = (uint32_t*)(base + L.cell);
    float *tx = (float*)(base + L.tx), *ty = (float*)(base + L.ty);
    RadixBufs r = L.sort.at(base);
    uint32_t* start = (uint32_t*)(base + L.start);
    const uint32_t S = (uint32_t)L.S, E = (uint32_t)L.E, NPIX = (uint32_t)L.NPIX;
    hipError_t e = radix_sort_begin(s, E, r);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lift_project_kernel, dim3((S + 255) / 256), dim3(256), 0, s, V, A, H, W, S, points, w2c, intr, cell, tx, ty);
    hipLaunchKernelGGL(lift_keys_kernel, dim3((E + 255) / 256), dim3(256), 0, s, E, A, H, W, NPIX, (const uint32_t*)cell, r.ka, r.va, r.hist, r.per_block);
    e = radix_sort_pairs(s, E, r, 0, L.bits);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lift_start_kernel, dim3(NPIX / 256 + 1), dim3(256), 0, s, E, NPIX, (const uint32_t*)r.sorted_keys(L.bits), start);
    const bool in_b = radix_lands_in_b(L.bits);
    uint32_t* ea = in_b ? r.ka : r.kb;                                 // the sort's other pair of buffers is free now
    float* ew = (float*)(in_b ? r.va : r.vb);
    hipLaunchKernelGGL(lift_edge_kernel, dim3((E + 255) / 256), dim3(256), 0, s, E, A, (const uint32_t*)r.sorted_vals(L.bits), (const float*)tx,
                       (const float*)ty, ea, ew);
    const int ncg = (C + LIFT_BWD_CH - 1) / LIFT_BWD_CH;
    const int use_lds = (size_t)A * LIFT_BWD_CH <= LIFT_LDS_FLOATS ? 1 : 0;
    const size_t lds = use_lds ? (size_t)A * LIFT_BWD_CH * 4 : 0;
    const dim3 g((unsigned)((size_t)B * V * ncg)), blk(LIFT_BWD_THREADS);
    if (dtype == IGS_DTYPE_F16)
        hipLaunchKernelGGL((lift_bwd_kernel<_Float16>), g, blk, lds, s, V, A, C, H * W, ncg, use_lds, (const uint32_t*)start, (const uint32_t*)ea,
                           (const float*)ew, dout, gs_a, gs_c, (_Float16*)dfeat, fs_n, fs_c);
    else
        hipLaunchKernelGGL((lift_bwd_kernel<float>), g, blk, lds, s, V, A, C, H * W, ncg, use_lds, (const uint32_t*)start, (const uint32_t*)ea,
                           (const float*)ew, dout, gs_a, gs_c, (float*)dfeat, fs_n, fs_c);
    return hipGetLastError();
}

// the entry points (the contract is in include/igs_rast.h)
static const char* lift_size_error(int B, int V, int A, int C, int H, int W)
{
    if (B < 0 || B > IGS_LIFT_MAX_SAMPLES) return "B out of range";
    if (V < 1 || V > IGS_LIFT_MAX_V) return "V out of range (1..IGS_LIFT_MAX_V)";
    if (A < 0 || A > IGS_LIFT_MAX_SAMPLES) return "A out of range";
    if (C < 1 || C > IGS_LIFT_MAX_C) return "C out of range (1..IGS_LIFT_MAX_C)";
    if (H < 1 || H > IGS_LIFT_MAX_HW) return "H out of range (1..IGS_LIFT_MAX_HW)";
    if (W < 1 || W > IGS_LIFT_MAX_HW) return "W out of range (1..IGS_LIFT_MAX_HW)";
    if ((long long)B * A > IGS_LIFT_MAX_SAMPLES) return "B * A out of range (IGS_LIFT_MAX_SAMPLES)";
    if ((long long)B * V * H * W > IGS_LIFT_MAX_PIXELS) return "B * V * H * W out of range (IGS_LIFT_MAX_PIXELS)";
    return nullptr;
}
extern "C" size_t igs_anchor_lift_scratch_bytes(int B, int V, int A, int C, int H, int W, int dtype)
{
    if (lift_size_error(B, V, A, C, H, W) || !dtype_ok(dtype)) return 0;
    return lift_scratch_bytes(B, V, A, H, W, false) + 256;
}
extern "C" size_t igs_anchor_lift_bwd_scratch_bytes(int B, int V, int A, int C, int H, int W, int dtype)
{
    if (lift_size_error(B, V, A, C, H, W) || !dtype_ok(dtype)) return 0;
    return lift_scratch_bytes(B, V, A, H, W, true) + 256;
}
extern "C" int igs_anchor_lift_fwd(void* stream, int B, int V, int A, int C, int H, int W, int dtype, const void* feat, long long fs_n,
                                   long long fs_c, long long fs_h, long long fs_w, const float* points, const float* w2c, const float* intr,
                                   float* out, long long os_a, long long os_c, void* scratch)
{
    const char* fn = "igs_anchor_lift_fwd";
    if (const char* w = lift_size_error(B, V, A, C, H, W)) return fail_in(fn, w);
    if (!dtype_ok(dtype)) return fail_in(fn, "unknown dtype code");
    if (const char* w = plane_stride_error(C, H, W, fs_n, fs_c, fs_h, fs_w)) return fail_in(fn, w);
    if (!((os_a == 1 && os_c == A) || (os_c == 1 && os_a == C))) return fail_in(fn, "output strides must be (os_a, os_c) = (1, A) or (C, 1)");
    if (A == 0 || B == 0) return 0;
    if (!feat || !points || !w2c || !intr || !out || !scratch) return fail_in(fn, "NULL pointer");
    HIP_TRY(launch_lift_fwd((hipStream_t)stream, B, V, A, C, H, W, dtype, feat, (size_t)fs_n, (size_t)fs_c, points, w2c, intr, out, (size_t)os_a,
                            (size_t)os_c, scratch), "anchor lift fwd launch");
    return 0;
}
extern "C" int igs_anchor_lift_bwd(void* stream, int B, int V, int A, int C, int H, int W, int dtype, const float* points, const float* w2c,
                                   const float* intr, const float* dout, long long gs_a, long long gs_c, void* dfeat, long long fs_n,
                                   long long fs_c, long long fs_h, long long fs_w, void* scratch)
{
    const char* fn = "igs_anchor_lift_bwd";
    if (const char* w = lift_size_error(B, V, A, C, H, W)) return fail_in(fn, w);
    if (!dtype_ok(dtype)) return fail_in(fn, "unknown dtype code");
    if (const char* w = plane_stride_error(C, H, W, fs_n, fs_c, fs_h, fs_w)) return fail_in(fn, w);
    if (fs_c < (long long)H * W || fs_n < fs_c * C) return fail_in(fn, "d feat planes overlap (fs_c >= H * W and fs_n >= C * fs_c required)");
    if (!((gs_a == 1 && gs_c == A) || (gs_c == 1 && gs_a == C))) return fail_in(fn, "d out strides must be (gs_a, gs_c) = (1, A) or (C, 1)");
    if (B == 0) return 0;
    if (!dfeat) return fail_in(fn, "NULL pointer");
    if (A == 0) {       // no samples: every element of d feat is zero (one fill per plane-contiguous tensor, else per image)
        const size_t es = dtype == IGS_DTYPE_F16 ? 2 : 4;
        if (fs_c == (long long)H * W && fs_n == fs_c * C)
            HIP_TRY(zero_fill_async((hipStream_t)stream, dfeat, (size_t)B * V * C * H * W * es), "zero d feat");
        else
            for (long long n = 0; n < (long long)B * V; n++)
                for (int c = 0; c < C; c++)
                    HIP_TRY(zero_fill_async((hipStream_t)stream, (char*)dfeat + ((size_t)n * fs_n + (size_t)c * fs_c) * es, (size_t)H * W * es), "zero d feat");
        return 0;
    }
    if (!points || !w2c || !intr || !dout || !scratch) return fail_in(fn, "NULL pointer");
    HIP_TRY(launch_lift_bwd((hipStream_t)stream, B, V, A, C, H, W, dtype, points, w2c, intr, dout, (size_t)gs_a, (size_t)gs_c, dfeat, (size_t)fs_n,
                            (size_t)fs_c, scratch), "anchor lift bwd launch");
    return 0;
}
