// upconv_bwd.hip -- the backward of upconv.hip's fused 2x bilinear upsample + 3x3 convolution (igs/IGS.py:132-134):
//     up = U x,  out = conv(up, W) + b,  g = d out [N, Cout, 2H, 2W]
//     db[o]            = sum_{n,Y,X} g[n,o,Y,X]
//     dW[o,c,dy,dx]    = sum_{n,Y,X} g[n,o,Y,X] up[n,c,Y+dy-1,X+dx-1]            (up zero outside the map, recomputed from x, never stored)
//     dup[n,c,y,x]     = sum_{o,dy,dx} W[o,c,dy,dx] g[n,o,y-dy+1,x-dx+1]         (g zero outside the map; never stored)
//     dx               = U^T dup
// include/igs_rast.h states the contract (igs_upconv_bwd), DESIGN.md section 25 the budgets and the figures.  Three kernels.
//
// dgrad (upconv_dgrad_kernel): the forward's kernel with another source and another end.  A workgroup owns a 3 x 15 low-resolution tile of
//   one image's dx and all Cin channels: U^T reaches the upsampled rows 2i - 1 .. 2i + 2 of a low-resolution row i, so the tile needs
//   exactly the 8 x 32 dup pixels from (2 i0 - 1, 2 j0 - 1) on -- the forward's product shape; neighbouring tiles recompute the one-pixel
//   overlap (1.42 x the forward's matrix work) instead of exchanging it, so there are no atomics and no second pass.  Per 32-channel tile k
//   of Cout it stages the 10 x 34 g pixels under the tile (zeros outside the map and past Cout) in LDS in the forward's operand order and
//   runs the forward's 9 taps x ceil(Cin / 32) tile products against wpack_t, the convolution transposed in (o, c) and flipped in (dy, dx),
//   with the forward's ring-prefetched weight stream.  Behind the loop each 32-channel tile of dup goes from the accumulators through LDS,
//   and one lane per dx element gathers its (at most) 4 x 4 dup values: columns first, then rows, both as fma chains in a fixed order.
//   The weight of upsampled row Y for low-resolution row i is what uc_source(Y) gives to i, both of its two samples counted: that
//   is where the forward's clamp folds back onto the first and the last row.
// wgrad (upconv_wgrad_kernel): a GEMM Cout x (9 Cin) contracted over the pixels.  A workgroup owns one 32-channel tile k of Cin and one
//   slice of the 4 x 32 pixel tiles of the batch (at most IGS_UPCONV_BWD_SLICES slices, tiles in order); wave t owns output tile t of Cout
//   and keeps its 9 taps' 32 x 32 partial dW in 144 float32 accumulators for the whole slice.  Per pixel tile the workgroup stages g for
//   all of Cout (channel-major: a lane supplies consecutive pixels of ONE channel, the contraction index) and rebuilds the 6 x 34 upsampled
//   pixels of its 32 input channels from x exactly as the forward does (float16: rounded to half once), channel-major as well.  A lane's
//   operand is one aligned 16-byte vector of a row (4 float32 / 8 half pixels); the three column shifts of the taps come from that vector
//   and the 32-bit word on either side of it, put together in registers (float16: funnel shifts of whole words), so the product loop has
//   no sub-dword and no misaligned LDS read.  db rides along: every lane adds up the g values it supplies.  The partials go to scratch.
// reduce (upconv_wreduce_kernel): adds the slices' partials in slice order and writes dw [Cout, Cin, 3, 3] and db.
// Every sum has a fixed order, nothing is atomic, every output element is stored by exactly one lane; all barriers are on the workgroup's
// straight path.
#include "upconv_common.h"
#include "host_api.h"

#define UCB_LY 3                           // dgrad: the low-resolution tile
#define UCB_LX 15
#define UCB_DCS (UC_TY * UC_TX + 1)        // the channel stride of a dup tile in LDS (odd)
#define UCB_BATCH(T) (sizeof(T) == 2 ? 8 : 4)      // global loads a thread has in flight while staging (the float32 instance is held to 128 registers)

#define UCW_TY 4                           // wgrad: the pixel tile
#define UCW_TX 32
#define UCW_UH (UCW_TY + 2)
#define UCW_UW (UCW_TX + 2)
#define UCW_LH (UCW_TY / 2 + 2)
#define UCW_LW (UCW_TX / 2 + 2)
#define UCW_LCS (UCW_LH * UCW_LW + 1)
#define UCW_THREADS 256                    // four waves: one per output tile of Cout
#define UCW_DB 128                         // the db partials behind a slice's dW partials
#define UCW_BATCH 8                        // global loads of g a thread has in flight while staging (2 UCW_BATCH divides 32)
static_assert(UCW_THREADS == 2 * UCW_TY * UCW_TX, "the g staging gives a thread one pixel and every second channel");

// V: the pixels of a lane's 16-byte operand.  GS: the channel stride of the staged g (4 x 32 pixels and one vector).  OFF: the index of the
// tile's first column in an upsampled row (the halo column sits in the word in front of it), RS the row's stride, CS the channel's.  GS
// and CS are odd numbers of 16-byte units, so the 128-bit reads of 32 neighbouring channels spread over the banks
template <typename T> struct UcwCfg;
template <> struct UcwCfg<float> { enum { V = 4, GS = 132, OFF = 4, RS = 40, CS = UCW_UH * 40 + 4 }; };
template <> struct UcwCfg<_Float16> { enum { V = 8, GS = 136, OFF = 8, RS = 48, CS = UCW_UH * 48 + 8 }; };

struct UpconvDgradArgs {
    int Cin, Cout, H, W;
    uint32_t tx, ty;                       // low-resolution tiles per row and column
    const void* g;                         // d out [N, Cout, 2H, 2W]
    const void* w;                         // wpack_t: [9][kt of Cin][ot of Cout] tiles
    void* dx;
};

struct UpconvWgradArgs {
    int Cin, Cout, H, W;
    uint32_t tx, ty, tiles, slices;        // pixel tiles per row, per column and in the batch; the slices they are cut into
    int want_w;                            // 0: db only (no x, no products)
    const void* x;
    long long xs_n, xs_c;
    const void* g;
    float* part;                           // [slices][ot kt 9 1024 + UCW_DB]
};

struct UpconvWreduceArgs {
    int Cin, Cout;
    uint32_t slices;
    const float* part;
    float* dw;
    float* db;
};

// what upsampled index Y of an axis of length 2 L gives to low-resolution index i: both samples of uc_source counted
__device__ __forceinline__ float ucb_weight(int Y, int i, int L)
{
    int i0, i1;
    float w1;
    uc_source(Y, L, i0, i1, w1);
    return (i0 == i ? 1.f - w1 : 0.f) + (i1 == i ? w1 : 0.f);
}

template <typename T, typename TX, int OT>
__global__ __launch_bounds__(64 * UcCfg<T>::WAVES, UcCfg<T>::PER_SIMD) void upconv_dgrad_kernel(const UpconvDgradArgs a)
{
    constexpr int ROWS = UcCfg<T>::ROWS, THREADS = 64 * UcCfg<T>::WAVES, PS = UcCfg<T>::PS, NV = UcCfg<T>::NV, RING = UcCfg<T>::RING;
    constexpr int STEPS = 9 * OT * NV, BATCH = UCB_BATCH(T);
    typedef typename AttnCfg<T>::vec wvec;
    static_assert(STEPS % RING == 0 && RING - 1 <= STEPS, "the ring's slots must come round with the k step");
    constexpr int GB = UC_UH * UC_UW * PS * (int)sizeof(T), DB = 32 * UCB_DCS * 4;
    __shared__ __attribute__((aligned(16))) char smem[GB > DB ? GB : DB];
    T* gt = (T*)smem;                                            // the staged g tile, then
    float* dup = (float*)smem;                                   // one 32-channel tile of dup [c][8][32]

    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int KT = mlp_tiles(a.Cout), OH = 2 * a.H, OW = 2 * a.W;
    const uint32_t bx = blockIdx.x % a.tx, byn = blockIdx.x / a.tx, by = byn % a.ty, n = byn / a.ty;
    const int i0 = (int)by * UCB_LY, j0 = (int)bx * UCB_LX;
    const int Y0 = 2 * i0 - 1, X0 = 2 * j0 - 1;                  // the dup tile's first row and column (-1 at the map's edge)

    attn_acc acc[ROWS][OT];
#pragma unroll
    for (int t = 0; t < OT; t++)
#pragma unroll
        for (int j = 0; j < ROWS; j++)
#pragma unroll
            for (int i = 0; i < 16; i++) acc[j][t][i] = 0.f;

    const char* wg = (const char*)a.w;
    const uint32_t wl = (uint32_t)lane * 16u;
#define UC_WVEC(k, q) (*(const wvec*)(wg + ((size_t)(((q) / NV) * KT + (k)) * (MLP_TILE * sizeof(T)) + ((q) % NV) * 1024) + wl))
    wvec ring[RING];
#pragma unroll
    for (int q = 0; q < RING - 1; q++) ring[q] = UC_WVEC(0, q);

    const T* gn = (const T*)a.g + (size_t)n * (size_t)a.Cout * (size_t)OH * (size_t)OW;
    for (int k = 0; k < KT; k++) {
        wg_barrier();                                            // (ends the reads of the tile of k - 1)
        // ---- 1. the g pixels under the tile and its halo, channels 32 k .. 32 k + 31: thread -> (channel, pixel), rows of g contiguous ----
        // (BATCH loads are issued before the first of their LDS stores: one global round trip per batch, not per element)
        for (int ib = threadIdx.x; ib < 32 * UC_UH * UC_UW; ib += BATCH * THREADS) {
            T v[BATCH];
            int at[BATCH];
#pragma unroll
            for (int j = 0; j < BATCH; j++) {
                const int i = ib + j * THREADS;
                const int c = i / (UC_UH * UC_UW), pix = i - c * (UC_UH * UC_UW), uy = pix / UC_UW, ux = pix - uy * UC_UW;
                const int Y = Y0 - 1 + uy, X = X0 - 1 + ux, o = 32 * k + c;
                v[j] = (T)0.f;                                   // outside the map: the transposed convolution's zero padding
                if (c < 32 && o < a.Cout && Y >= 0 && Y < OH && X >= 0 && X < OW) v[j] = gn[((size_t)o * OH + Y) * OW + X];
                at[j] = c < 32 ? pix * PS + (c & 3) + 4 * ((c >> 3) & 3) + 16 * ((c >> 2) & 1) : -1;      // position 16 h + e holds channel attn_row(e, h)
            }
#pragma unroll
            for (int j = 0; j < BATCH; j++)
                if (at[j] >= 0) gt[at[j]] = v[j];
        }
        wg_barrier();

        // ---- 2. the products, as the forward runs them ----
        const int kn = k + 1 < KT ? k + 1 : k;
        MlpIn<T> in[ROWS];
#pragma unroll
        for (int q = 0; q < STEPS; q++) {
            const int tile = q / NV, v = q - tile * NV, tap = tile / OT, t = tile - tap * OT, dy = tap / 3, dx = tap - 3 * dy, ahead = q + RING - 1;
            if (t == 0 && v == 0) {
#pragma unroll
                for (int j = 0; j < ROWS; j++) uc_operand(in[j], gt + ((wave * ROWS + j + dy) * UC_UW + r + dx) * PS + 16 * h);
            }
            if (ahead < STEPS) ring[ahead % RING] = UC_WVEC(k, ahead);
            else ring[ahead % RING] = UC_WVEC(kn, ahead - STEPS);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < ROWS; j++) acc[j][t] = uc_mm(ring[q % RING], in[j], v, acc[j][t]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#undef UC_WVEC

    // ---- 3. U^T: per 32-channel tile of Cin, dup through LDS, then one lane per dx element ----
    TX* dxn = (TX*)a.dx + (size_t)n * (size_t)a.Cin * (size_t)a.H * (size_t)a.W;
#pragma unroll
    for (int t = 0; t < OT; t++) {
        wg_barrier();                                            // (ends the reads of g, or of tile t - 1)
#pragma unroll
        for (int j = 0; j < ROWS; j++)
#pragma unroll
            for (int i = 0; i < 16; i++) dup[attn_row(i, h) * UCB_DCS + (wave * ROWS + j) * UC_TX + r] = acc[j][t][i];
        wg_barrier();
        for (int e = threadIdx.x; e < 32 * UCB_LY * UCB_LX; e += THREADS) {
            const int c = e / (UCB_LY * UCB_LX), p = e - c * (UCB_LY * UCB_LX), li = p / UCB_LX, lj = p - li * UCB_LX;
            const int gi = i0 + li, gj = j0 + lj, ch = 32 * t + c;
            if (gi >= a.H || gj >= a.W || ch >= a.Cin) continue;
            float wx[4];
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const int X = 2 * gj - 1 + b;
                wx[b] = X >= 0 && X < OW ? ucb_weight(X, gj, a.W) : 0.f;
            }
            const float* d = dup + c * UCB_DCS + 2 * li * UC_TX + 2 * lj;
            float s = 0.f;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int Y = 2 * gi - 1 + q;
                if (Y < 0 || Y >= OH) continue;
                float rs = 0.f;
#pragma unroll
                for (int b = 0; b < 4; b++)
                    if (wx[b] != 0.f) rs = fmaf(wx[b], d[q * UC_TX + b], rs);      // (a column outside the map takes no part)
                s = fmaf(ucb_weight(Y, gi, a.H), rs, s);
            }
            dxn[((size_t)ch * a.H + gi) * a.W + gj] = (TX)s;     // (float16: the one rounding to half)
        }
    }
}

// the three shifted operands of a lane from the aligned vector at p and the word on either side of it
__device__ __forceinline__ void ucw_taps(const float* p, float e[3][4])
{
    const float m = p[-1], n = p[4];
    const attn_f4 v = *(const attn_f4*)p;
    e[0][0] = m; e[0][1] = v[0]; e[0][2] = v[1]; e[0][3] = v[2];
    e[1][0] = v[0]; e[1][1] = v[1]; e[1][2] = v[2]; e[1][3] = v[3];
    e[2][0] = v[1]; e[2][1] = v[2]; e[2][2] = v[3]; e[2][3] = n;
}
typedef uint32_t ucw_u4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void ucw_taps(const _Float16* p, attn_h8 e[3])
{
    const uint32_t m = *(const uint32_t*)(p - 2), n = *(const uint32_t*)(p + 8);
    const ucw_u4 v = *(const ucw_u4*)p;
    ucw_u4 lo, hi;
    lo[0] = (m >> 16) | (v[0] << 16); lo[1] = (v[0] >> 16) | (v[1] << 16); lo[2] = (v[1] >> 16) | (v[2] << 16); lo[3] = (v[2] >> 16) | (v[3] << 16);
    hi[0] = (v[0] >> 16) | (v[1] << 16); hi[1] = (v[1] >> 16) | (v[2] << 16); hi[2] = (v[2] >> 16) | (v[3] << 16); hi[3] = (v[3] >> 16) | (n << 16);
    e[0] = __builtin_bit_cast(attn_h8, lo);
    e[1] = __builtin_bit_cast(attn_h8, v);
    e[2] = __builtin_bit_cast(attn_h8, hi);
}

// acc[3 dy + dx] += g's vector x the row's three shifts; returns the sum of g's vector (for db)
__device__ __forceinline__ float ucw_mm(const float* gp, const float* up, int dy, attn_acc* acc)
{
    const attn_f4 g = *(const attn_f4*)gp;
    float e[3][4];
    ucw_taps(up, e);
#pragma unroll
    for (int dx = 0; dx < 3; dx++)
#pragma unroll
        for (int u = 0; u < 4; u++) acc[3 * dy + dx] = __builtin_amdgcn_mfma_f32_32x32x2f32(g[u], e[dx][u], acc[3 * dy + dx], 0, 0, 0);
    return ((g[0] + g[1]) + g[2]) + g[3];
}
__device__ __forceinline__ float ucw_mm(const _Float16* gp, const _Float16* up, int dy, attn_acc* acc)
{
    const attn_h8 g = *(const attn_h8*)gp;
    attn_h8 e[3];
    ucw_taps(up, e);
#pragma unroll
    for (int dx = 0; dx < 3; dx++) acc[3 * dy + dx] = __builtin_amdgcn_mfma_f32_32x32x16_f16(g, e[dx], acc[3 * dy + dx], 0, 0, 0);
    float s = 0.f;
#pragma unroll
    for (int u = 0; u < 8; u++) s += (float)g[u];
    return s;
}
__device__ __forceinline__ float ucw_gsum(const float* gp)
{
    const attn_f4 g = *(const attn_f4*)gp;
    return ((g[0] + g[1]) + g[2]) + g[3];
}
__device__ __forceinline__ float ucw_gsum(const _Float16* gp)
{
    const attn_h8 g = *(const attn_h8*)gp;
    float s = 0.f;
#pragma unroll
    for (int u = 0; u < 8; u++) s += (float)g[u];
    return s;
}

template <typename T, typename TX>
__global__ __launch_bounds__(UCW_THREADS, 1) void upconv_wgrad_kernel(const UpconvWgradArgs a)
{
    constexpr int V = UcwCfg<T>::V, GS = UcwCfg<T>::GS, OFF = UcwCfg<T>::OFF, RS = UcwCfg<T>::RS, CS = UcwCfg<T>::CS;
    constexpr int RSTEPS = UCW_TX / (2 * V);                     // a step: the 2 V pixels the two lane halves supply
    __shared__ float lo[32 * UCW_LCS];
    __shared__ __attribute__((aligned(16))) T gs[IGS_UPCONV_MAX_WIDTH * GS];
    __shared__ __attribute__((aligned(16))) T ups[32 * CS];

    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int OT = mlp_tiles(a.Cout), KT = mlp_tiles(a.Cin), OH = 2 * a.H, OW = 2 * a.W;
    const uint32_t sl = blockIdx.x % a.slices, k = blockIdx.x / a.slices;
    const uint32_t t0 = (uint32_t)((uint64_t)sl * a.tiles / a.slices), t1 = (uint32_t)((uint64_t)(sl + 1) * a.tiles / a.slices);

    attn_acc acc[9];
#pragma unroll
    for (int q = 0; q < 9; q++)
#pragma unroll
        for (int i = 0; i < 16; i++) acc[q][i] = 0.f;
    float bsum = 0.f;

    // the words of `ups` the operand reads touch and the staging never writes (their halves are shifted out) hold zeros, not leftovers
    for (int i = threadIdx.x; i < 32 * CS; i += UCW_THREADS) ups[i] = (T)0.f;

    for (uint32_t tile = t0; tile < t1; tile++) {
        const uint32_t bx = tile % a.tx, byn = tile / a.tx, by = byn % a.ty, n = byn / a.ty;
        const int Y0 = (int)by * UCW_TY, X0 = (int)bx * UCW_TX;
        const int m0 = Y0 / 2 - 1, n0 = X0 / 2 - 1;
        wg_barrier();                                            // (ends the reads of the tile before)
        // ---- 1. g of every output channel, channel-major (zeros past the map and past Cout), and the low-resolution patch of x ----
        const T* gn = (const T*)a.g + (size_t)n * (size_t)a.Cout * (size_t)OH * (size_t)OW;
        // a thread keeps one pixel of the tile and takes every second channel, UCW_BATCH loads in flight before their LDS stores; the
        // patch of x is loaded before g's stores as well, so the tile costs three global round trips and not one per element
        constexpr int PB = (32 * UCW_LH * UCW_LW + UCW_THREADS - 1) / UCW_THREADS;
        float xv[PB];
        if (a.want_w) {
            const TX* xn = (const TX*)a.x + (size_t)n * (size_t)a.xs_n;
#pragma unroll
            for (int j = 0; j < PB; j++) {
                const int i = threadIdx.x + j * UCW_THREADS;
                const int c = i / (UCW_LH * UCW_LW), p = i - c * (UCW_LH * UCW_LW), ly = p / UCW_LW, lx = p - ly * UCW_LW;
                const int gy = min(max(m0 + ly, 0), a.H - 1), gx = min(max(n0 + lx, 0), a.W - 1);
                xv[j] = 0.f;
                if (c < 32 && 32 * (int)k + c < a.Cin) xv[j] = (float)xn[(size_t)(32 * k + c) * (size_t)a.xs_c + (size_t)(gy * a.W + gx)];
            }
        }
        {
            const int p = threadIdx.x & (UCW_TY * UCW_TX - 1), o0 = threadIdx.x / (UCW_TY * UCW_TX);
            const int Y = Y0 + p / UCW_TX, X = X0 + p % UCW_TX;
            const bool in = Y < OH && X < OW;
            const T* gpix = gn + ((size_t)(in ? Y : 0) * OW + (in ? X : 0));
            for (int ob = 0; ob < 32 * OT; ob += 2 * UCW_BATCH) {
                T v[UCW_BATCH];
#pragma unroll
                for (int j = 0; j < UCW_BATCH; j++) {
                    const int o = ob + 2 * j + o0;
                    v[j] = (T)0.f;
                    if (in && o < a.Cout) v[j] = gpix[(size_t)o * OH * OW];
                }
#pragma unroll
                for (int j = 0; j < UCW_BATCH; j++) gs[(ob + 2 * j + o0) * GS + p] = v[j];
            }
        }
        if (a.want_w) {
#pragma unroll
            for (int j = 0; j < PB; j++) {
                const int i = threadIdx.x + j * UCW_THREADS;
                if (i < 32 * UCW_LH * UCW_LW) lo[(i / (UCW_LH * UCW_LW)) * UCW_LCS + i % (UCW_LH * UCW_LW)] = xv[j];
            }
        }
        wg_barrier();
        // ---- 2. the upsampled tile with its halo, the forward's arithmetic, channel-major ----
        if (a.want_w) {
            for (int i = threadIdx.x; i < 32 * UCW_UH * UCW_UW; i += UCW_THREADS) {
                const int c = i / (UCW_UH * UCW_UW), p = i - c * (UCW_UH * UCW_UW), uy = p / UCW_UW, ux = p - uy * UCW_UW;
                const int Y = Y0 - 1 + uy, X = X0 - 1 + ux;
                float v = 0.f;                                   // outside the map: the convolution's zero padding
                if (Y >= 0 && Y < OH && X >= 0 && X < OW) {
                    int y0, y1, x0, x1;
                    float wy, wx;
                    uc_source(Y, a.H, y0, y1, wy);
                    uc_source(X, a.W, x0, x1, wx);
                    const float* l0 = lo + c * UCW_LCS + (y0 - m0) * UCW_LW - n0;
                    const float* l1 = lo + c * UCW_LCS + (y1 - m0) * UCW_LW - n0;
                    v = uc_lerp(uc_lerp(l0[x0], l0[x1], wx), uc_lerp(l1[x0], l1[x1], wx), wy);
                }
                ups[c * CS + uy * RS + OFF - 1 + ux] = (T)v;     // (float16: the one rounding to half, as the forward rounds it)
            }
        }
        wg_barrier();
        // ---- 3. wave t: dW[32 t + row][tap][32 k + r] += sum over the tile's pixels ----
        if (wave < OT) {
            const T* gp = gs + (32 * wave + r) * GS + h * V;
            const T* up = ups + r * CS + OFF + h * V;
            if (a.want_w) {
#pragma unroll 1
                for (int y = 0; y < UCW_TY; y++) {
#pragma unroll
                    for (int st = 0; st < RSTEPS; st++) {
                        float s = 0.f;
#pragma unroll
                        for (int dy = 0; dy < 3; dy++) s = ucw_mm(gp + y * UCW_TX + 2 * V * st, up + (y + dy) * RS + 2 * V * st, dy, acc);
                        bsum += s;
                    }
                }
            } else {
                for (int y = 0; y < UCW_TY; y++)
#pragma unroll
                    for (int st = 0; st < RSTEPS; st++) bsum += ucw_gsum(gp + y * UCW_TX + 2 * V * st);
            }
        }
    }

    // ---- the slice's partials: register-major, so that the reduction reads them coalesced ----
    if (wave < OT) {
        float* ps = a.part + (size_t)sl * ((size_t)OT * KT * 9 * MLP_TILE + UCW_DB);
        if (a.want_w) {
#pragma unroll
            for (int q = 0; q < 9; q++)
#pragma unroll
                for (int i = 0; i < 16; i++) ps[((size_t)(wave * KT + k) * 9 + q) * MLP_TILE + i * 64 + lane] = acc[q][i];
        }
        const float other = __shfl_xor(bsum, 32);
        if (k == 0 && h == 0) ps[(size_t)OT * KT * 9 * MLP_TILE + 32 * wave + r] = bsum + other;
    }
}

__global__ __launch_bounds__(256) void upconv_wreduce_kernel(const UpconvWreduceArgs a)
{
    const int OT = mlp_tiles(a.Cout), KT = mlp_tiles(a.Cin);
    const uint32_t nw = (uint32_t)(OT * KT * 9 * MLP_TILE), idx = blockIdx.x * 256u + threadIdx.x;
    const size_t stride = (size_t)nw + UCW_DB;
    if (idx < nw) {
        if (!a.dw) return;
        const uint32_t tile = idx >> 10, e = idx & 1023u, i = e >> 6, lane = e & 63u, tap = tile % 9u, tk = tile / 9u, k = tk % (uint32_t)KT, t = tk / (uint32_t)KT;
        const int o = 32 * (int)t + attn_row((int)i, (int)(lane >> 5)), c = 32 * (int)k + (int)(lane & 31u);
        if (o >= a.Cout || c >= a.Cin) return;
        float s = 0.f;
        for (uint32_t sl = 0; sl < a.slices; sl++) s += a.part[sl * stride + idx];
        a.dw[((size_t)o * a.Cin + c) * 9 + tap] = s;
    } else if (idx < nw + UCW_DB) {
        const int o = (int)(idx - nw);
        if (!a.db || o >= a.Cout) return;
        float s = 0.f;
        for (uint32_t sl = 0; sl < a.slices; sl++) s += a.part[sl * stride + idx];
        a.db[o] = s;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the entry points (the contract is in include/igs_rast.h)
// ---------------------------------------------------------------------------------------------------------------------------------
template <int OT> static void upconv_dgrad_launch(bool half, bool xhalf, dim3 grid, hipStream_t s, const UpconvDgradArgs& a)
{
    const dim3 bh(64 * UcCfg<_Float16>::WAVES), bf(64 * UcCfg<float>::WAVES);
    if (xhalf) {
        if (half) hipLaunchKernelGGL((upconv_dgrad_kernel<_Float16, _Float16, OT>), grid, bh, 0, s, a);
        else hipLaunchKernelGGL((upconv_dgrad_kernel<float, _Float16, OT>), grid, bf, 0, s, a);
    } else {
        if (half) hipLaunchKernelGGL((upconv_dgrad_kernel<_Float16, float, OT>), grid, bh, 0, s, a);
        else hipLaunchKernelGGL((upconv_dgrad_kernel<float, float, OT>), grid, bf, 0, s, a);
    }
}

// the pixel tiles of the wgrad kernel in the batch, and the slices they are cut into
static long long upconv_wgrad_tiles(int N, int H, int W) { return (long long)N * ((2 * H + UCW_TY - 1) / UCW_TY) * ((2 * W + UCW_TX - 1) / UCW_TX); }
static const char* upconv_size_error(int N, int Cin, int Cout, int H, int W)
{
    if (N < 0 || N > IGS_UPCONV_MAX_PIXELS) return "N out of range";
    if (Cin < 1 || Cin > IGS_UPCONV_MAX_WIDTH) return "Cin out of range (1..IGS_UPCONV_MAX_WIDTH)";
    if (Cout < 1 || Cout > IGS_UPCONV_MAX_WIDTH) return "Cout out of range (1..IGS_UPCONV_MAX_WIDTH)";
    if (H < 1 || H > IGS_UPCONV_MAX_HW) return "H out of range (1..IGS_UPCONV_MAX_HW)";
    if (W < 1 || W > IGS_UPCONV_MAX_HW) return "W out of range (1..IGS_UPCONV_MAX_HW)";
    if ((long long)N * H * W > IGS_UPCONV_MAX_PIXELS) return "N * H * W out of range (IGS_UPCONV_MAX_PIXELS)";
    return nullptr;
}

extern "C" long long igs_upconv_bwd_scratch_bytes(int N, int Cin, int Cout, int H, int W, int conv_dtype)
{
    if (upconv_size_error(N, Cin, Cout, H, W) || !dtype_ok(conv_dtype)) return -1;
    const long long tiles = upconv_wgrad_tiles(N, H, W), slices = tiles < IGS_UPCONV_BWD_SLICES ? tiles : IGS_UPCONV_BWD_SLICES;
    return slices * (9LL * mlp_tiles(Cout) * mlp_tiles(Cin) * MLP_TILE + UCW_DB) * (long long)sizeof(float);
}

extern "C" int igs_upconv_bwd(void* stream, int N, int Cin, int Cout, int H, int W, int x_dtype, const void* x, long long xs_n, long long xs_c,
                              long long xs_h, long long xs_w, int conv_dtype, const void* wpack_t, const void* dout, void* scratch,
                              long long scratch_bytes, void* dx, float* dw, float* db)
{
    const char* fn = "igs_upconv_bwd";
    if (const char* w = upconv_size_error(N, Cin, Cout, H, W)) return fail_in(fn, w);
    if (!dtype_ok(x_dtype) || !dtype_ok(conv_dtype)) return fail_in(fn, "unknown dtype code");
    if (const char* w = plane_stride_error(Cin, H, W, xs_n, xs_c, xs_h, xs_w)) return fail_in(fn, w);
    if (!ptr_aligned(dw, 4) || !ptr_aligned(db, 4)) return fail_in(fn, "dw and db must be aligned to 4 bytes");
    if (!ptr_aligned(x, dtype_bytes(x_dtype)) || !ptr_aligned(dx, dtype_bytes(x_dtype)) || !ptr_aligned(dout, dtype_bytes(conv_dtype)))
        return fail_in(fn, "a pointer is not aligned to its element size");
    if (!ptr_aligned(wpack_t, 16) || !ptr_aligned(scratch, 16)) return fail_in(fn, "wpack_t and scratch must be aligned to 16 bytes");
    if (dw && !x) return fail_in(fn, "x is NULL and dw is wanted");
    const long long need = igs_upconv_bwd_scratch_bytes(N, Cin, Cout, H, W, conv_dtype);
    if (N > 0) {
        if (!wpack_t || !dout || !scratch) return fail_in(fn, "NULL pointer (wpack_t, dout and scratch are required)");
        if (scratch_bytes < need) return fail_in(fn, "scratch_bytes below igs_upconv_bwd_scratch_bytes(...)");
    }
    if (!dx && !dw && !db) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (N == 0) {
        if (dw) HIP_TRY(hipMemsetAsync(dw, 0, (size_t)Cout * Cin * 9 * sizeof(float), s), "upconv_bwd: zero-fill of dw");
        if (db) HIP_TRY(hipMemsetAsync(db, 0, (size_t)Cout * sizeof(float), s), "upconv_bwd: zero-fill of db");
        return 0;
    }
    const bool half = conv_dtype == IGS_DTYPE_F16, xhalf = x_dtype == IGS_DTYPE_F16;
    if (dx) {
        UpconvDgradArgs a = {};
        a.Cin = Cin; a.Cout = Cout; a.H = H; a.W = W;
        a.tx = (uint32_t)((W + UCB_LX - 1) / UCB_LX); a.ty = (uint32_t)((H + UCB_LY - 1) / UCB_LY);
        a.g = dout; a.w = wpack_t; a.dx = dx;
        const dim3 grid(a.tx * a.ty * (uint32_t)N);              // (at most N H W <= 2^22)
        switch (mlp_tiles(Cin)) {
        case 1: upconv_dgrad_launch<1>(half, xhalf, grid, s, a); break;
        case 2: upconv_dgrad_launch<2>(half, xhalf, grid, s, a); break;
        case 3: upconv_dgrad_launch<3>(half, xhalf, grid, s, a); break;
        default: upconv_dgrad_launch<4>(half, xhalf, grid, s, a); break;
        }
        HIP_TRY(hipGetLastError(), "upconv dgrad launch");
    }
    if (dw || db) {
        UpconvWgradArgs a = {};
        a.Cin = Cin; a.Cout = Cout; a.H = H; a.W = W;
        a.tx = (uint32_t)((2 * W + UCW_TX - 1) / UCW_TX); a.ty = (uint32_t)((2 * H + UCW_TY - 1) / UCW_TY);
        a.tiles = (uint32_t)upconv_wgrad_tiles(N, H, W);
        a.slices = a.tiles < IGS_UPCONV_BWD_SLICES ? a.tiles : IGS_UPCONV_BWD_SLICES;
        a.want_w = dw != nullptr;
        a.x = x; a.xs_n = xs_n; a.xs_c = xs_c; a.g = dout; a.part = (float*)scratch;
        const dim3 grid(a.slices * (uint32_t)(dw ? mlp_tiles(Cin) : 1)), block(UCW_THREADS);
        if (xhalf) {
            if (half) hipLaunchKernelGGL((upconv_wgrad_kernel<_Float16, _Float16>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((upconv_wgrad_kernel<float, _Float16>), grid, block, 0, s, a);
        } else {
            if (half) hipLaunchKernelGGL((upconv_wgrad_kernel<_Float16, float>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((upconv_wgrad_kernel<float, float>), grid, block, 0, s, a);
        }
        HIP_TRY(hipGetLastError(), "upconv wgrad launch");
        UpconvWreduceArgs ra = {};
        ra.Cin = Cin; ra.Cout = Cout; ra.slices = a.slices; ra.part = (const float*)scratch; ra.dw = dw; ra.db = db;
        const uint32_t items = (uint32_t)(9 * mlp_tiles(Cout) * mlp_tiles(Cin) * MLP_TILE + UCW_DB);
        hipLaunchKernelGGL(upconv_wreduce_kernel, dim3((items + 255) / 256), dim3(256), 0, s, ra);
        HIP_TRY(hipGetLastError(), "upconv wreduce launch");
    }
    return 0;
}
