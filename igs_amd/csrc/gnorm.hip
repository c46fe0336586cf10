// gnorm.hip -- the two ends of Transformer1D.forward (igs/models/transformers.py:860-908) for gfx950: nn.GroupNorm over channel-major
// [B, C, A] written token-major [B, A, C] in front of proj_in, and proj_out's token-major result plus the channel-major residual written
// token-major behind it.  Forward and backward.  include/igs_rast.h states the contract, DESIGN.md section 20 the budgets and the figures.
//
//   (1) gn_stats_kernel: one workgroup of 1024 lanes per (example, group) walks the cpg * A elements of the group twice: the sum for the
//       centre m, then the sums of d = x - m and d d, and norm_finish (the corrected two-pass form of inorm.hip and tokens.hip: a constant
//       group gives exactly `bias`).  Lane t takes the elements (four at a time where the layout allows) t, t + 1024, ... in that order;
//       the lanes of a wave are added by a butterfly, the 16 waves in wave order through LDS.  stats[b, g] = (mean, rstd).
//   (2) A tile of 64 channels x 64 tokens belongs to 256 lanes, 16 values each, in one of two mappings with tx = lane & 15, ty = lane >> 4:
//       channel-major, slot (i, k) = channel ty + 16 i, token 4 tx + k (global access along the tokens), and token-major, slot (i, k) =
//       token ty + 16 i, channel 4 tx + k (global access along the channels).  An LDS tile turns one into the other, element (r, q) at
//       65 r + 2 (r >> 2) + q floats: a 4-byte LDS access is banked per half wave (32 lanes = 16 tx x 2 ty, 32 banks); the column reads
//       (r = 4 tx + k, q = ty + 16 i) land on bank 6 tx + ty + const, 32 different ones, and the row writes (r = ty + 16 i, q = 4 tx + k)
//       on 4 tx + ty + const, two lanes per bank, which a 4-byte LDS store absorbs (its register transfer takes as long).  Four-element
//       global access where C, A, the strides and the bases allow it (VEC), scalar access of the same mapping otherwise.
//       gn_apply_kernel:          x channel-major -> (x - mean_g) rstd_g gamma_c + beta_c -> tile -> out token-major
//       tok_add_residual_kernel:  res channel-major -> tile -> + tok -> out token-major
//       gn_bwd_sums_kernel:       dy token-major -> tile -> beside x: per tile and channel the sums over its tokens of dy x_hat and dy
//       gn_bwd_dx_kernel:         dy token-major -> tile -> dx = rstd_g (gamma_c dy - (s1 + x_hat s2) / (cpg A)) channel-major
//   (3) The backward's sums: the tile rows [B][tiles of A][2][C] are added in tile order per example by param_reduce.h (one share per
//       example) into p [B][2][C]; gn_bwd_group_kernel adds gamma_c p over the channels of a group into s [B][G][2]; d weight and d bias are
//       the rows of p added in example order (param_reduce.h again).  No float atomics; every split depends on the shapes only.
#include "common.h"
#include "elem_common.h"
#include "host_api.h"
#include "param_reduce.h"

#define GN_STATS_THREADS 1024
#define GN_STATS_MAX_GROUPS (1u << 20)                         // workgroups of a statistics or group-sum launch (they stride over the rest)
#define GN_TILE 64
#define GN_TILE_FLOATS (GN_TILE * 65 + 32)
#define GN_THREADS 256
#define GN_REDUCE_MAX_Z 32768                                  // examples per param_reduce launch (gridDim.z)

// ---------------------------------------------------------------------------------------------------------------------------------
// (1) the statistics
// ---------------------------------------------------------------------------------------------------------------------------------
// the sum of one value per lane over the workgroup, the same bits in every lane: butterfly per wave, then the waves in wave order
__device__ __forceinline__ float gn_block_sum(float v, float* red)
{
    v = lane_sum<64>(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    wg_barrier();
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < GN_STATS_THREADS / 64; k++) s += red[k];
    return s;
}

// W = 4 (VEC) or 1 elements per step; per = A / W steps per channel
template <bool VEC>
__global__ void __launch_bounds__(GN_STATS_THREADS)
gn_stats_kernel(unsigned long long BG, int G, int cpg, uint32_t A, TokPtr x, size_t xbs, size_t xcs, float eps, float* __restrict__ stats)
{
    constexpr uint32_t W = VEC ? 4 : 1;
    __shared__ float red[3][GN_STATS_THREADS / 64];
    const uint32_t per = A / W, total = (uint32_t)cpg * per;
    const float n = (float)cpg * (float)A;
    for (unsigned long long bg = blockIdx.x; bg < BG; bg += gridDim.x) {
        const size_t base = (size_t)(bg / G) * xbs + (size_t)(bg % G) * cpg * xcs;
        float s = 0.f;
        for (uint32_t e = threadIdx.x; e < total; e += GN_STATS_THREADS) {
            const uint32_t c = e / per;
            const size_t at = base + (size_t)c * xcs + (size_t)(e - c * per) * W;
            if (VEC) {
                const float4 q = ld4(x, at);
                s += (q.x + q.y) + (q.z + q.w);
            } else {
                s += ld(x, at);
            }
        }
        const float m = gn_block_sum(s, red[0]) / n;
        float s1 = 0.f, s2 = 0.f;
        for (uint32_t e = threadIdx.x; e < total; e += GN_STATS_THREADS) {
            const uint32_t c = e / per;
            const size_t at = base + (size_t)c * xcs + (size_t)(e - c * per) * W;
            if (VEC) {
                const float4 q = ld4(x, at);
                const float d0 = q.x - m, d1 = q.y - m, d2 = q.z - m, d3 = q.w - m;
                s1 += (d0 + d1) + (d2 + d3);
                s2 += fmaf(d0, d0, d1 * d1) + fmaf(d2, d2, d3 * d3);
            } else {
                const float d = ld(x, at) - m;
                s1 += d;
                s2 = fmaf(d, d, s2);
            }
        }
        s1 = gn_block_sum(s1, red[1]);
        s2 = gn_block_sum(s2, red[2]);
        if (threadIdx.x == 0) {
            float mean, rstd;
            norm_finish(m, s1, s2, n, eps, mean, rstd);
            stats[2 * bg] = mean;
            stats[2 * bg + 1] = rstd;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (2) the tile
// ---------------------------------------------------------------------------------------------------------------------------------
// The 16 values of a lane.  `lead` is the stride between the tile's rows in global memory (the channel stride of a channel-major
// operand, the row stride of a token-major one), `rows` x `cols` what of the tile lies inside the tensor; slots outside hold zero.
__device__ __forceinline__ int gn_tile_at(int r, int q) { return 65 * r + 2 * (r >> 2) + q; }
struct GnTile {
    float v[4][4];
    template <bool VEC>
    __device__ __forceinline__ void load(TokPtr p, size_t base, size_t lead, int rows, int cols)
    {
        const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int r = ty + 16 * i;
            const size_t at = base + (size_t)r * lead + 4 * tx;
            if (VEC) {
                float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
                if (r < rows && 4 * tx < cols) q = ld4(p, at);
                v[i][0] = q.x; v[i][1] = q.y; v[i][2] = q.z; v[i][3] = q.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++) v[i][k] = (r < rows && 4 * tx + k < cols) ? ld(p, at + k) : 0.f;
            }
        }
    }
    template <bool VEC>
    __device__ __forceinline__ void store(TokPtr p, size_t base, size_t lead, int rows, int cols) const
    {
        const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int r = ty + 16 * i;
            const size_t at = base + (size_t)r * lead + 4 * tx;
            if (VEC) {
                if (r < rows && 4 * tx < cols) st4(p, at, make_float4(v[i][0], v[i][1], v[i][2], v[i][3]));
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (r < rows && 4 * tx + k < cols) st(p, at + k, v[i][k]);
            }
        }
    }
    // from one mapping to the other (the exchange is its own inverse): slot (i, k) of row ty + 16 i, column 4 tx + k becomes the value
    // of row 4 tx + k, column ty + 16 i.  One barrier; `tile` is not used again by the caller.
    __device__ __forceinline__ void transpose(float* tile)
    {
        const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int k = 0; k < 4; k++) tile[gn_tile_at(ty + 16 * i, 4 * tx + k)] = v[i][k];
        wg_barrier();
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int k = 0; k < 4; k++) v[i][k] = tile[gn_tile_at(4 * tx + k, ty + 16 * i)];
    }
};

// where a workgroup's tile lies: blockIdx.x = b * tilesA + token tile, blockIdx.y = channel tile
struct GnAt {
    uint32_t b, ta;
    int c0, nc, na;
    size_t a0;
    __device__ __forceinline__ GnAt(uint32_t tilesA, int C, uint32_t A)
    {
        b = blockIdx.x / tilesA;
        ta = blockIdx.x - b * tilesA;
        a0 = (size_t)ta * GN_TILE;
        c0 = blockIdx.y * GN_TILE;
        nc = min(GN_TILE, C - c0);
        na = A - a0 < GN_TILE ? (int)(A - a0) : GN_TILE;
    }
};

// a [B, C, A] operand: pointer, batch stride, channel stride; a [B * A, C] operand: pointer, row stride
struct GnCm { TokPtr p; size_t bs, cs; };
struct GnTm { TokPtr p; size_t rs; };
__device__ __forceinline__ size_t gn_at(const GnCm& t, const GnAt& w) { return (size_t)w.b * t.bs + (size_t)w.c0 * t.cs + w.a0; }
__device__ __forceinline__ size_t gn_at(const GnTm& t, const GnAt& w, uint32_t A) { return ((size_t)w.b * A + w.a0) * t.rs + w.c0; }

// x_hat of the channel-major slots of a lane, in place; rstd[i] and (with `w`) gamma[i] of its four channels.  Channels outside the
// tensor are left alone (their slots hold zero) with rstd = gamma = 0.
__device__ __forceinline__ void gn_normalise(GnTile& t, const GnAt& w, int G, int cpg, const float* __restrict__ stats, const float* __restrict__ wgt,
                                             float (&rstd)[4], float (&gamma)[4], int (&group)[4])
{
    const int ty = threadIdx.x >> 4;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int c = w.c0 + ty + 16 * i;
        rstd[i] = gamma[i] = 0.f;
        group[i] = 0;
        if (ty + 16 * i >= w.nc) continue;
        group[i] = c / cpg;
        const float* st = stats + 2 * ((size_t)w.b * G + group[i]);
        const float mean = st[0];
        rstd[i] = st[1];
        gamma[i] = wgt ? wgt[c] : 1.f;
#pragma unroll
        for (int k = 0; k < 4; k++) t.v[i][k] = (t.v[i][k] - mean) * rstd[i];
    }
}

template <bool VEC>
__global__ void __launch_bounds__(GN_THREADS)
gn_apply_kernel(uint32_t tilesA, int C, int G, uint32_t A, GnCm x, const float* __restrict__ stats, const float* __restrict__ wgt,
                const float* __restrict__ bias, GnTm out)
{
    __shared__ float tile[GN_TILE_FLOATS];
    const GnAt w(tilesA, C, A);
    GnTile t;
    t.load<VEC>(x.p, gn_at(x, w), x.cs, w.nc, w.na);
    float rstd[4], gamma[4];
    int group[4];
    gn_normalise(t, w, G, C / G, stats, wgt, rstd, gamma, group);
    if (wgt) {
        const int ty = threadIdx.x >> 4;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const float beta = ty + 16 * i < w.nc ? bias[w.c0 + ty + 16 * i] : 0.f;
#pragma unroll
            for (int k = 0; k < 4; k++) t.v[i][k] = fmaf(t.v[i][k], gamma[i], beta);
        }
    }
    t.transpose(tile);
    t.store<VEC>(out.p, gn_at(out, w, A), out.rs, w.na, w.nc);
}

template <bool VEC>
__global__ void __launch_bounds__(GN_THREADS)
tok_add_residual_kernel(uint32_t tilesA, int C, uint32_t A, GnTm tok, GnCm res, GnTm out)
{
    __shared__ float tile[GN_TILE_FLOATS];
    const GnAt w(tilesA, C, A);
    GnTile r, t;
    r.load<VEC>(res.p, gn_at(res, w), res.cs, w.nc, w.na);
    t.load<VEC>(tok.p, gn_at(tok, w, A), tok.rs, w.na, w.nc);
    r.transpose(tile);
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int k = 0; k < 4; k++) t.v[i][k] += r.v[i][k];
    t.store<VEC>(out.p, gn_at(out, w, A), out.rs, w.na, w.nc);
}

// part[((b * tilesA + ta) * 2 + 0) * C + c] = the sum over the tile's tokens of dy x_hat, [... + 1) * C + c] of dy: the four tokens of a
// lane, then a butterfly over the 16 lanes of the channel
template <bool VEC>
__global__ void __launch_bounds__(GN_THREADS)
gn_bwd_sums_kernel(uint32_t tilesA, int C, int G, uint32_t A, GnCm x, const float* __restrict__ stats, GnTm dy, float* __restrict__ part)
{
    __shared__ float tile[GN_TILE_FLOATS];
    const GnAt w(tilesA, C, A);
    GnTile t, g;
    g.load<VEC>(dy.p, gn_at(dy, w, A), dy.rs, w.na, w.nc);
    t.load<VEC>(x.p, gn_at(x, w), x.cs, w.nc, w.na);
    g.transpose(tile);
    float rstd[4], gamma[4];
    int group[4];
    gn_normalise(t, w, G, C / G, stats, nullptr, rstd, gamma, group);
    float s[8];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        s[i] = fmaf(g.v[i][0], t.v[i][0], g.v[i][1] * t.v[i][1]) + fmaf(g.v[i][2], t.v[i][2], g.v[i][3] * t.v[i][3]);
        s[4 + i] = (g.v[i][0] + g.v[i][1]) + (g.v[i][2] + g.v[i][3]);
    }
    lane_sum<16>(s);
    if ((threadIdx.x & 15) == 0) {
        const int ty = threadIdx.x >> 4;
        float* row = part + (size_t)blockIdx.x * 2 * C + w.c0;
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (ty + 16 * i < w.nc) { row[ty + 16 * i] = s[i]; row[C + ty + 16 * i] = s[4 + i]; }
    }
}

// sg[b, g] = (sum over the channels of the group of gamma_c p[b, 1, c], the same of gamma_c p[b, 0, c]): (s1, s2) of the dx formula.
// One wave per (b, g): lane l adds the channels l, l + 64, ... of the group in that order, then a butterfly.
__global__ void __launch_bounds__(64)
gn_bwd_group_kernel(unsigned long long BG, int C, int G, const float* __restrict__ p, const float* __restrict__ wgt, float* __restrict__ sg)
{
    const int cpg = C / G;
    for (unsigned long long bg = blockIdx.x; bg < BG; bg += gridDim.x) {
        const float* row = p + (size_t)(bg / G) * 2 * C;
        const int c0 = (int)(bg % G) * cpg;
        float s[2] = {0.f, 0.f};
        for (int c = threadIdx.x; c < cpg; c += 64) {
            const float gm = wgt ? wgt[c0 + c] : 1.f;
            s[0] = fmaf(gm, row[C + c0 + c], s[0]);
            s[1] = fmaf(gm, row[c0 + c], s[1]);
        }
        lane_sum<64>(s);
        if (threadIdx.x == 0) { sg[2 * bg] = s[0]; sg[2 * bg + 1] = s[1]; }
    }
}

template <bool VEC>
__global__ void __launch_bounds__(GN_THREADS)
gn_bwd_dx_kernel(uint32_t tilesA, int C, int G, uint32_t A, GnCm x, const float* __restrict__ stats, const float* __restrict__ wgt, GnTm dy,
                 const float* __restrict__ sg, GnCm dx)
{
    __shared__ float tile[GN_TILE_FLOATS];
    const GnAt w(tilesA, C, A);
    GnTile t, g;
    g.load<VEC>(dy.p, gn_at(dy, w, A), dy.rs, w.na, w.nc);
    t.load<VEC>(x.p, gn_at(x, w), x.cs, w.nc, w.na);
    g.transpose(tile);
    float rstd[4], gamma[4];
    int group[4];
    gn_normalise(t, w, G, C / G, stats, wgt, rstd, gamma, group);
    const float n = (float)(C / G) * (float)A;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const float* s = sg + 2 * ((size_t)w.b * G + group[i]);      // (group 0 of the example for a channel outside the tensor: not stored)
        const float s1 = s[0], s2 = s[1];
#pragma unroll
        for (int k = 0; k < 4; k++) t.v[i][k] = rstd[i] * (gamma[i] * g.v[i][k] - fmaf(t.v[i][k], s2, s1) / n);
    }
    t.store<VEC>(dx.p, gn_at(dx, w), dx.cs, w.nc, w.na);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// launches
// ---------------------------------------------------------------------------------------------------------------------------------
static uint32_t gn_tiles(long long n) { return (uint32_t)((n + GN_TILE - 1) / GN_TILE); }
// the four-element path of a channel-major operand (along A) and of a token-major one (along C)
static bool gn_cm_vec_ok(const void* p, int dtype, long long A, long long bs, long long cs)
{
    return !p || (ptr_aligned(p, vec_grid_bytes(dtype)) && ((A | bs | cs) & 3) == 0);
}
static bool gn_tm_vec_ok(const void* p, int dtype, int C, long long rs) { return !p || (ptr_aligned(p, vec_grid_bytes(dtype)) && ((C | rs) & 3) == 0); }
static GnCm gn_cm(const void* p, int dtype, long long bs, long long cs) { return GnCm{TokPtr{p, p && dtype == IGS_DTYPE_F16}, (size_t)bs, (size_t)cs}; }
static GnTm gn_tm(const void* p, int dtype, long long rs) { return GnTm{TokPtr{p, p && dtype == IGS_DTYPE_F16}, (size_t)rs}; }
static unsigned gn_group_grid(unsigned long long BG) { return (unsigned)(BG < GN_STATS_MAX_GROUPS ? BG : GN_STATS_MAX_GROUPS); }

#define GN_LAUNCH(KERNEL, VEC, GRID, THREADS, ...)                                                                                          \
    do {                                                                                                                                    \
        if (VEC) hipLaunchKernelGGL((KERNEL<true>), GRID, dim3(THREADS), 0, s, __VA_ARGS__);                                                \
        else hipLaunchKernelGGL((KERNEL<false>), GRID, dim3(THREADS), 0, s, __VA_ARGS__);                                                   \
    } while (0)

static hipError_t launch_gn_fwd(hipStream_t s, int B, int C, int G, long long A, int x_dtype, const void* x, long long x_bs, long long x_cs,
                                const float* w, const float* b, float eps, int out_dtype, void* out, long long os, float* stats)
{
    const bool xv = gn_cm_vec_ok(x, x_dtype, A, x_bs, x_cs);
    const unsigned long long BG = (unsigned long long)B * G;
    GN_LAUNCH(gn_stats_kernel, xv, dim3(gn_group_grid(BG)), GN_STATS_THREADS, BG, G, C / G, (uint32_t)A, TokPtr{x, x_dtype == IGS_DTYPE_F16},
              (size_t)x_bs, (size_t)x_cs, eps, stats);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const uint32_t tilesA = gn_tiles(A);
    GN_LAUNCH(gn_apply_kernel, xv && gn_tm_vec_ok(out, out_dtype, C, os), dim3(tilesA * (uint32_t)B, gn_tiles(C)), GN_THREADS, tilesA, C, G, (uint32_t)A,
              gn_cm(x, x_dtype, x_bs, x_cs), (const float*)stats, w, b, gn_tm(out, out_dtype, os));
    return hipGetLastError();
}

// the scratch of the backward: the tile rows, p, sg and the staging rows of the last reduction, each on a 256-byte grid
struct GnScratch { size_t part, p, sg, stage, bytes; };
static GnScratch gn_scratch(int B, int C, int G, long long A)
{
    GnScratch l;
    l.part = 0;
    l.p = l.part + align_up((size_t)B * gn_tiles(A) * 2 * C * 4, 256);
    l.sg = l.p + align_up((size_t)B * 2 * C * 4, 256);
    l.stage = l.sg + align_up((size_t)B * G * 2 * 4, 256);
    l.bytes = l.stage + align_up((size_t)PARAM_REDUCE_GROUPS * 2 * C * 4, 256) + 256;
    return l;
}

static hipError_t launch_gn_bwd(hipStream_t s, int B, int C, int G, long long A, int x_dtype, const void* x, long long x_bs, long long x_cs,
                                const float* w, const float* stats, int g_dtype, const void* dout, long long gs, int dx_dtype, void* dx,
                                long long dx_bs, long long dx_cs, float* dw, float* db, void* scratch)
{
    const GnScratch l = gn_scratch(B, C, G, A);
    char* base = (char*)align_ptr((const char*)scratch);
    float *part = (float*)(base + l.part), *p = (float*)(base + l.p), *sg = (float*)(base + l.sg), *stage = (float*)(base + l.stage);
    const uint32_t tilesA = gn_tiles(A);
    const dim3 grid(tilesA * (uint32_t)B, gn_tiles(C));
    const bool vec = gn_cm_vec_ok(x, x_dtype, A, x_bs, x_cs) && gn_tm_vec_ok(dout, g_dtype, C, gs);
    const GnCm tx = gn_cm(x, x_dtype, x_bs, x_cs);
    const GnTm tg = gn_tm(dout, g_dtype, gs);
    GN_LAUNCH(gn_bwd_sums_kernel, vec, grid, GN_THREADS, tilesA, C, G, (uint32_t)A, tx, stats, tg, part);
    hipError_t e = hipGetLastError();
    // p[b] <- the tile rows of example b in tile order: one share of tilesA rows per example
    const dim3 blk(64 * PARAM_REDUCE_WAVES);
    for (int b0 = 0; b0 < B && e == hipSuccess; b0 += GN_REDUCE_MAX_Z) {
        const int nb = B - b0 < GN_REDUCE_MAX_Z ? B - b0 : GN_REDUCE_MAX_Z;
        float* dst = p + (size_t)b0 * 2 * C;
        hipLaunchKernelGGL(param_reduce_kernel, dim3((C + 63) / 64, 2, nb), blk, 0, s, C, (uint32_t)nb * tilesA, part + (size_t)b0 * tilesA * 2 * C,
                           dst, dst + C, (size_t)2 * C);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return e;
    if (dx) {
        const unsigned long long BG = (unsigned long long)B * G;
        hipLaunchKernelGGL(gn_bwd_group_kernel, dim3(gn_group_grid(BG)), dim3(64), 0, s, BG, C, G, (const float*)p, w, sg);
        GN_LAUNCH(gn_bwd_dx_kernel, vec && gn_cm_vec_ok(dx, dx_dtype, A, dx_bs, dx_cs), grid, GN_THREADS, tilesA, C, G, (uint32_t)A, tx, stats, w, tg,
                  (const float*)sg, gn_cm(dx, dx_dtype, dx_bs, dx_cs));
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (dw || db) return launch_param_reduce(s, C, (uint32_t)B, p, B > 1024 ? stage : nullptr, dw, db);
    return hipSuccess;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the entry points (the contract is in include/igs_rast.h)
// ---------------------------------------------------------------------------------------------------------------------------------
static ByteSpan gn_cm_span(const void* p, int B, int C, long long A, long long bs, long long cs, int dtype)
{
    return byte_span(p, ((size_t)(B - 1) * (size_t)bs + (size_t)(C - 1) * (size_t)cs + (size_t)A) * dtype_bytes(dtype));
}
static ByteSpan gn_tm_span(const void* p, int B, int C, long long A, long long rs, int dtype)
{
    return byte_span(p, (((size_t)B * (size_t)A - 1) * (size_t)rs + (size_t)C) * dtype_bytes(dtype));
}
static ByteSpan gn_f32_span(const void* p, size_t n) { return p ? byte_span(p, n * 4) : ByteSpan{0, 0}; }
static bool gn_misaligned(const void* p, int dtype) { return !ptr_aligned(p, dtype_bytes(dtype)); }

static const char* gn_size_error(int B, int C, int G, long long A)
{
    if (C < 1 || C > IGS_GN_MAX_C) return "C out of range (1..IGS_GN_MAX_C)";
    if (G < 1 || C % G != 0) return "G must be at least 1 and divide C";
    if (A < 1 || A > IGS_GN_MAX_GROUP_ELEMS / (C / G)) return "A out of range (A >= 1, (C / G) * A <= IGS_GN_MAX_GROUP_ELEMS)";
    if (B < 0 || B > IGS_GN_MAX_TOKENS / A) return "B out of range (B >= 0, B * A <= IGS_GN_MAX_TOKENS)";
    return nullptr;
}
static bool gn_cm_stride_bad(int C, long long A, long long bs, long long cs)
{
    return cs < A || cs > IGS_TOKENS_MAX_STRIDE || bs < (C - 1) * cs + A || bs > IGS_GN_MAX_BATCH_STRIDE;
}
static bool gn_tm_stride_bad(int C, long long rs) { return rs < C || rs > IGS_TOKENS_MAX_STRIDE; }
static const char* const GN_STRIDES = "a stride is below the extent it steps over (channel stride < A, batch stride < (C - 1) channel stride + A, row stride < C) "
                                      "or above IGS_TOKENS_MAX_STRIDE / IGS_GN_MAX_BATCH_STRIDE";

extern "C" int igs_group_norm_tokens_fwd(void* stream, int B, int C, int G, long long A, int x_dtype, const void* x, long long x_bs, long long x_cs,
                                         const float* weight, const float* bias, float eps, int out_dtype, void* out, long long os, float* stats)
{
    const char* fn = "igs_group_norm_tokens_fwd";
    if (!dtype_ok(x_dtype) || !dtype_ok(out_dtype)) return fail_in(fn, "unknown dtype code");
    if (const char* w = gn_size_error(B, C, G, A)) return fail_in(fn, w);
    if (gn_cm_stride_bad(C, A, x_bs, x_cs) || gn_tm_stride_bad(C, os)) return fail_in(fn, GN_STRIDES);
    if (!eps_ok(eps)) return fail_in(fn, "eps must be finite and >= 0");
    if ((weight == nullptr) != (bias == nullptr)) return fail_in(fn, "weight and bias go together (both or neither)");
    if (B == 0) return 0;
    if (!x || !out || !stats) return fail_in(fn, "NULL pointer");
    if (gn_misaligned(x, x_dtype) || gn_misaligned(out, out_dtype) || !ptr_aligned(weight, 4) || !ptr_aligned(bias, 4) || !ptr_aligned(stats, 4))
        return fail_in(fn, "a pointer is not aligned to its element size");
    const ByteSpan ins[3] = {gn_cm_span(x, B, C, A, x_bs, x_cs, x_dtype), gn_f32_span(weight, C), gn_f32_span(bias, C)};
    const ByteSpan outs[2] = {gn_tm_span(out, B, C, A, os, out_dtype), gn_f32_span(stats, (size_t)B * G * 2)};
    for (int i = 0; i < 2; i++)
        for (int k = 0; k < 3; k++)
            if (spans_overlap(outs[i], ins[k])) return fail_in(fn, "an output (out, stats) overlaps x, weight or bias");
    if (spans_overlap(outs[0], outs[1])) return fail_in(fn, "out and stats overlap one another");
    HIP_TRY(launch_gn_fwd((hipStream_t)stream, B, C, G, A, x_dtype, x, x_bs, x_cs, weight, bias, eps, out_dtype, out, os, stats), "group norm fwd launch");
    return 0;
}

extern "C" size_t igs_group_norm_tokens_bwd_scratch_bytes(int B, int C, int G, long long A)
{
    if (gn_size_error(B, C, G, A)) return 0;
    return gn_scratch(B, C, G, A).bytes;
}

extern "C" int igs_group_norm_tokens_bwd(void* stream, int B, int C, int G, long long A, int x_dtype, const void* x, long long x_bs, long long x_cs,
                                         const float* weight, const float* stats, int dout_dtype, const void* dout, long long gs, int dx_dtype,
                                         void* dx, long long dx_bs, long long dx_cs, float* dweight, float* dbias, void* scratch)
{
    const char* fn = "igs_group_norm_tokens_bwd";
    if (!dtype_ok(x_dtype) || !dtype_ok(dout_dtype) || (dx && !dtype_ok(dx_dtype))) return fail_in(fn, "unknown dtype code");
    if (const char* w = gn_size_error(B, C, G, A)) return fail_in(fn, w);
    if (gn_cm_stride_bad(C, A, x_bs, x_cs) || gn_tm_stride_bad(C, gs) || (dx && gn_cm_stride_bad(C, A, dx_bs, dx_cs))) return fail_in(fn, GN_STRIDES);
    if (B == 0 || (!dx && !dweight && !dbias)) return 0;
    if (!x || !dout || !stats || !scratch) return fail_in(fn, "NULL pointer");
    if (gn_misaligned(x, x_dtype) || gn_misaligned(dout, dout_dtype) || (dx && gn_misaligned(dx, dx_dtype)) || !ptr_aligned(weight, 4) ||
        !ptr_aligned(stats, 4) || !ptr_aligned(dweight, 4) || !ptr_aligned(dbias, 4))
        return fail_in(fn, "a pointer is not aligned to its element size");
    const ByteSpan ins[4] = {gn_cm_span(x, B, C, A, x_bs, x_cs, x_dtype), gn_tm_span(dout, B, C, A, gs, dout_dtype), gn_f32_span(weight, C),
                             gn_f32_span(stats, (size_t)B * G * 2)};
    const ByteSpan outs[4] = {dx ? gn_cm_span(dx, B, C, A, dx_bs, dx_cs, dx_dtype) : ByteSpan{0, 0}, gn_f32_span(dweight, C), gn_f32_span(dbias, C),
                              byte_span(scratch, gn_scratch(B, C, G, A).bytes)};
    for (int i = 0; i < 4; i++) {
        for (int k = 0; k < 4; k++)
            if (spans_overlap(outs[i], ins[k])) return fail_in(fn, "an output overlaps x, dout, weight or stats");
        for (int k = i + 1; k < 4; k++)
            if (spans_overlap(outs[i], outs[k])) return fail_in(fn, "the outputs (dx, dweight, dbias, scratch) overlap one another");
    }
    HIP_TRY(launch_gn_bwd((hipStream_t)stream, B, C, G, A, x_dtype, x, x_bs, x_cs, weight, stats, dout_dtype, dout, gs, dx_dtype, dx, dx_bs, dx_cs, dweight,
                          dbias, scratch),
            "group norm bwd launch");
    return 0;
}

extern "C" int igs_tokens_add_residual(void* stream, int B, int C, long long A, int tok_dtype, const void* tok, long long ts, int res_dtype,
                                       const void* res, long long r_bs, long long r_cs, int out_dtype, void* out, long long os)
{
    const char* fn = "igs_tokens_add_residual";
    if (!dtype_ok(tok_dtype) || !dtype_ok(res_dtype) || !dtype_ok(out_dtype)) return fail_in(fn, "unknown dtype code");
    if (const char* w = gn_size_error(B, C, 1, A)) return fail_in(fn, w);
    if (gn_tm_stride_bad(C, ts) || gn_cm_stride_bad(C, A, r_bs, r_cs) || gn_tm_stride_bad(C, os)) return fail_in(fn, GN_STRIDES);
    if (B == 0) return 0;
    if (!tok || !res || !out) return fail_in(fn, "NULL pointer");
    if (gn_misaligned(tok, tok_dtype) || gn_misaligned(res, res_dtype) || gn_misaligned(out, out_dtype))
        return fail_in(fn, "a pointer is not aligned to its element size");
    const ByteSpan so = gn_tm_span(out, B, C, A, os, out_dtype);
    if (spans_overlap(so, gn_tm_span(tok, B, C, A, ts, tok_dtype)) || spans_overlap(so, gn_cm_span(res, B, C, A, r_bs, r_cs, res_dtype)))
        return fail_in(fn, "out overlaps tok or res");
    hipStream_t s = (hipStream_t)stream;
    const uint32_t tilesA = gn_tiles(A);
    const bool vec = gn_tm_vec_ok(tok, tok_dtype, C, ts) && gn_cm_vec_ok(res, res_dtype, A, r_bs, r_cs) && gn_tm_vec_ok(out, out_dtype, C, os);
    GN_LAUNCH(tok_add_residual_kernel, vec, dim3(tilesA * (uint32_t)B, gn_tiles(C)), GN_THREADS, tilesA, C, (uint32_t)A, gn_tm(tok, tok_dtype, ts),
              gn_cm(res, res_dtype, r_bs, r_cs), gn_tm(out, out_dtype, os));
    HIP_TRY(hipGetLastError(), "tokens add residual launch");
    return 0;
}
