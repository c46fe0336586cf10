// ffn_bwd.hip -- the backward of the fused layer tail (ffn.hip): d a, d s and the gradients of merge, norm1, mlp[0], mlp[2] and norm2 from a, s,
// the packs and d out, with the forward recomputed.  include/igs_rast.h states the contract (igs_layer_tail_bwd), DESIGN.md section 27 the
// budget and the figures.  Per row, with g = d out:
//
//   FFN:    q = g w2;  dy = r2 (q - mean q - xh2 mean(q xh2));  dh = W2^T dy;  dz = dh gelu'(z);  du = W1^T dz;  ds = g + du[0:128];  dn1 = du[128:256]
//   no FFN: ds = g;  dn1 = g
//   both:   p = dn1 w1;  dm = r1 (p - mean p - xh1 mean(p xh1));  da = Wm^T dm
//
// The rows are walked in chunks of IGS_LAYER_TAIL_BWD_CHUNK_ROWS; a chunk's rows live in float32 slots of the scratch, row-major, one slot
// per quantity.  Per chunk:
//   layer_tail_bwd_rows_kernel    the forward's layout and staging (4 waves, a wave owns 32 rows, an accumulator tile is the next operand as
//                                 it stands).  Pass 1 is the forward up to y and spills every hidden chunk's z_j from the accumulators; then
//                                 the LN2 backward gives dy.  Pass 2 streams the hidden chunks of the TRANSPOSED pack: dh_j = W2_j^T dy (4
//                                 tiles), z_j read back by the lane that wrote it (no barrier), dz_j = dh_j gelu'(z_j), du += W1_j^T dz_j (8
//                                 tiles).  Then ds, the LN1 backward, da = Wm^T dm.  Where a parameter gradient is wanted it stores a,
//                                 [s ; n1], dz, dy, dm and the four LayerNorm rows' terms.  24 tile products per hidden chunk.
//   layer_tail_bwd_wgrad_kernel   mlp_bwd_wgrad_kernel's scheme: a wave owns (slice of FB_SLICE_ROWS rows, product, input tile, group of up
//                                 to four output tiles): dW2 = sum dy (x) gelu(z), dW1 = sum dz (x) [s ; n1], dWm = sum dm (x) a, and as
//                                 column sums the four LayerNorm rows.  Its float32 accumulators start from the slice's partial of the
//                                 chunk before: a slice's partial is the sum over its rows in row order, chunk after chunk.
// and at the end layer_tail_bwd_reduce_kernel adds the slices' partials in slice order.  No float atomics; the order of every sum depends
// on the sizes only.
//
// A trip's rows past the chunk's end compute on the chunk's first row and write their own slot rows (the slots are sized to whole trips),
// which the weight-gradient kernel never reads; their da / ds are not stored.
#include "ffn_common.h"

#define FB_CHUNK_ROWS IGS_LAYER_TAIL_BWD_CHUNK_ROWS
#define FB_SLICE_ROWS 512
#define FB_WG_WAVES 4
#define FB_WG_THREADS (64 * FB_WG_WAVES)
#define FB_MAX_PRODUCTS 7
#define FB_OUTPUTS 7
static_assert(FB_CHUNK_ROWS % FB_SLICE_ROWS == 0 && FB_SLICE_ROWS % FFN_TRIP_ROWS == 0, "a chunk is whole slices, a slice whole trips");

template <typename T, bool FFN> struct FfnBwdCfg {
    enum {
        HALF = AttnCfg<T>::HALF,
        RESIDENT = HALF || !FFN,                                                   // Wm and Wm^T are staged once per workgroup
        PIECES = FFN_CHUNK_TILES * MLP_TILE * (int)sizeof(T) / 16 / FFN_THREADS,
        W1_PIECES = PIECES * FFN_W1_TILES / FFN_CHUNK_TILES,
        LDS_TILES = FFN ? 2 * FFN_CHUNK_TILES + (HALF ? 2 * FFN_WM_TILES : 0) : 2 * FFN_WM_TILES,
    };
};

struct FfnBwdArgs {
    long long row0;                        // the chunk's first row
    int rows;                              // ... and how many it has
    TokPtr a, s, g, da, ds;
    long long as, ss, gs, das, dss;        // row strides in elements
    int a_vec, s_vec, g_vec, da_vec, ds_vec;
    int want_da, want_ds, want_par;        // want_par: the slots that only the weight-gradient kernel reads are stored
    const void *w, *wt;                    // the forward's pack and the transposed one
    const float *ln1w, *ln1b, *ln2w;
    float eps1, eps2;
    int ht;                                // hidden / 32
    // the chunk's slots, float32 row-major: z, dz [rows][hidden]; u [rows][256]; the others [rows][128]
    float *z, *dz, *u, *sa, *dy, *dm, *gx2, *gg, *dnx1, *dn1;
};

// exact GELU': Phi(z) + z phi(z).  z z may overflow to +inf: the exponential is then 0 and the finite z times 0 is 0, never inf * 0.
__device__ __forceinline__ float ffn_gelu_grad(float z) { return fmaf(z * 0.3989422804014327f, expf(-0.5f * z * z), gelu_cdf(z)); }

// the lane's share of a 128-wide slot row: four accumulator tiles, or the 16 four-channel groups of ffn_read_groups (the same channels)
__device__ __forceinline__ void fb_spill(float* row, const attn_acc (&o)[4], int h)
{
#pragma unroll
    for (int t = 0; t < 4; t++) {
#pragma unroll
        for (int g = 0; g < 4; g++) *(float4*)(row + 32 * t + 8 * g + 4 * h) = make_float4(o[t][4 * g], o[t][4 * g + 1], o[t][4 * g + 2], o[t][4 * g + 3]);
    }
}
__device__ __forceinline__ void fb_spill(float* row, const float4 (&f)[16], int h)
{
#pragma unroll
    for (int q = 0; q < 16; q++) *(float4*)(row + 32 * (q >> 2) + 8 * (q & 3) + 4 * h) = f[q];
}
__device__ __forceinline__ void fb_fill(attn_acc (&o)[4], const float* row, int h)
{
#pragma unroll
    for (int t = 0; t < 4; t++) {
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const float4 f = *(const float4*)(row + 32 * t + 8 * g + 4 * h);
            o[t][4 * g] = f.x; o[t][4 * g + 1] = f.y; o[t][4 * g + 2] = f.z; o[t][4 * g + 3] = f.w;
        }
    }
}
template <typename T>
__device__ __forceinline__ void fb_operand(MlpIn<T>& in, const float4 (&f)[16])
{
#pragma unroll
    for (int q = 0; q < 16; q++) {
        const int k = q >> 2, e = 4 * (q & 3);
        in.set(k, e, f[q].x); in.set(k, e + 1, f[q].y); in.set(k, e + 2, f[q].z); in.set(k, e + 3, f[q].w);
    }
}
template <typename T>
__device__ __forceinline__ void fb_operand(MlpIn<T>& in, const attn_acc (&o)[4])
{
#pragma unroll
    for (int t = 0; t < 4; t++) {
#pragma unroll
        for (int i = 0; i < 16; i++) in.set(t, i, o[t][i]);
    }
}

// The LayerNorm backward of the row this lane and lane ^ 32 hold: d <- rstd (p - mean p - xh mean(p xh)), p = d w.  float32, a fixed order.
__device__ __forceinline__ void fb_ln_bwd(attn_acc (&d)[4], const attn_acc (&xh)[4], const float* w, float rstd, int h)
{
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int t = 0; t < 4; t++) {
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const attn_f4 wv = *(const attn_f4*)(w + 32 * t + 8 * g + 4 * h);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const float p = d[t][4 * g + j] * wv[j];
                d[t][4 * g + j] = p;
                s1 += p;
                s2 = fmaf(p, xh[t][4 * g + j], s2);
            }
        }
    }
    s1 += __shfl_xor(s1, 32, 64);
    s2 += __shfl_xor(s2, 32, 64);
    const float m1 = s1 * (1.f / 128.f), m2 = s2 * (1.f / 128.f);
#pragma unroll
    for (int t = 0; t < 4; t++) {
#pragma unroll
        for (int i = 0; i < 16; i++) d[t][i] = rstd * fmaf(-xh[t][i], m2, d[t][i] - m1);
    }
}

template <typename T, bool FFN>
__global__ __launch_bounds__(FFN_THREADS, 1) void layer_tail_bwd_rows_kernel(const FfnBwdArgs a)
{
    typedef FfnBwdCfg<T, FFN> Cfg;
    constexpr int CHUNK = FFN_CHUNK_TILES * MLP_TILE, WM = FFN_WM_TILES * MLP_TILE;
    __shared__ __attribute__((aligned(16))) T wl[Cfg::LDS_TILES * MLP_TILE];
    __shared__ __attribute__((aligned(16))) float lnp[3 * 128];                  // LN1's weight and bias, LN2's weight

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const T* wg = (const T*)a.w;
    const T* wtg = (const T*)a.wt;
    const T* w1 = wg + WM;
    const T* w2 = w1 + (size_t)a.ht * FFN_W1_TILES * MLP_TILE;
    const T* w1t = wtg + WM;
    const T* w2t = w1t + (size_t)a.ht * FFN_W1_TILES * MLP_TILE;
    // resident: Wm and Wm^T behind the chunk buffers; float32 with FFN: both borrow the chunk buffers in turn
    T* wm = wl + (FFN && Cfg::HALF ? 2 * CHUNK : 0);
    T* wmt = Cfg::RESIDENT ? wm + WM : wm;
    const size_t H = (size_t)a.ht * 32;

    if (threadIdx.x < 128) {
        lnp[threadIdx.x] = a.ln1w[threadIdx.x];
        lnp[128 + threadIdx.x] = a.ln1b[threadIdx.x];
        lnp[256 + threadIdx.x] = FFN ? a.ln2w[threadIdx.x] : 0.f;
    }
    if (Cfg::RESIDENT) {
        ffn_stage(wm, wg, WM);
        ffn_stage(wmt, wtg, WM);
    }
    wg_barrier();

    const int trips = (a.rows + FFN_TRIP_ROWS - 1) / FFN_TRIP_ROWS;
    for (int trip = blockIdx.x; trip < trips; trip += gridDim.x) {                // (uniform over the workgroup: every wave takes every trip)
        const int lr = trip * FFN_TRIP_ROWS + wave * 32 + r;                     // the row's place in the chunk's slots
        const bool live = lr < a.rows;
        const long long row = a.row0 + (live ? lr : 0);
        const size_t o128 = (size_t)lr * 128;                                    // the row's offset in a 128-wide slot

        // every wave left the trip before through its last barrier: the chunk buffers are free
        if (!Cfg::RESIDENT) ffn_stage(wm, wg, WM);
        MlpIn<T> in_a, in_s, in_n;
        {
            float4 f[16];
            ffn_read_groups(f, a.a, (size_t)row * a.as, a.a_vec, h);
            if (a.want_par) fb_spill(a.sa + o128, f, h);
            fb_operand(in_a, f);
        }
        attn_f4 stg[Cfg::PIECES];
        if (FFN) {
            float4 f[16];
            ffn_read_groups(f, a.s, (size_t)row * a.ss, a.s_vec, h);
            if (a.want_par) fb_spill(a.u + (size_t)lr * 256, f, h);
            fb_operand(in_s, f);
            ffn_fetch<T, Cfg::PIECES, Cfg::W1_PIECES>(stg, w1, w2, 0);
        }
        if (!Cfg::RESIDENT) wg_barrier();

        // ---- m = Wm a and its statistics; xh1 stays in o ----
        attn_acc o[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
#pragma unroll
            for (int i = 0; i < 16; i++) o[t][i] = 0.f;
#pragma unroll
            for (int k = 0; k < 4; k++) o[t] = mlp_mm(wm + (t * 4 + k) * MLP_TILE, lane, in_a, k, o[t]);
        }
        float mean1, rstd1, mean2, rstd2;
        ffn_row_stats(o, a.eps1, mean1, rstd1);
#pragma unroll
        for (int t = 0; t < 4; t++) {
#pragma unroll
            for (int i = 0; i < 16; i++) o[t][i] = (o[t][i] - mean1) * rstd1;
        }

        attn_acc dn[4];                                                          // d n1, then d m
        if (!FFN) {
            float4 f[16];
            ffn_read_groups(f, a.g, (size_t)row * a.gs, a.g_vec, h);
            if (a.want_ds && live) ffn_write_groups(f, a.ds, (size_t)row * a.dss, a.ds_vec, h);
#pragma unroll
            for (int q = 0; q < 16; q++) {
                dn[q >> 2][4 * (q & 3)] = f[q].x; dn[q >> 2][4 * (q & 3) + 1] = f[q].y;
                dn[q >> 2][4 * (q & 3) + 2] = f[q].z; dn[q >> 2][4 * (q & 3) + 3] = f[q].w;
            }
        } else {
            // n1 as the forward's operand; xh1 waits in the lane's own row of the dnx1 slot
            {
                attn_acc n1[4];
#pragma unroll
                for (int t = 0; t < 4; t++) {
#pragma unroll
                    for (int g = 0; g < 4; g++) {
                        const int c = 32 * t + 8 * g + 4 * h;
                        const attn_f4 wv = *(const attn_f4*)(lnp + c), bv = *(const attn_f4*)(lnp + 128 + c);
#pragma unroll
                        for (int j = 0; j < 4; j++) n1[t][4 * g + j] = fmaf(o[t][4 * g + j], wv[j], bv[j]);
                    }
                }
                fb_operand(in_n, n1);
                if (a.want_par) fb_spill(a.u + (size_t)lr * 256 + 128, n1, h);
            }
            fb_spill(a.dnx1 + o128, o, h);
            if (!Cfg::RESIDENT) wg_barrier();                                    // everybody is done with Wm
            ffn_put<T, Cfg::PIECES>(wl, stg);
            wg_barrier();

            // ---- pass 1: y = sum over the chunks of W2_j gelu(z_j), z_j = W1_j [s ; n1] spilled ----
#pragma unroll
            for (int t = 0; t < 4; t++) {
#pragma unroll
                for (int i = 0; i < 16; i++) o[t][i] = 0.f;
            }
            float* zr = a.z + (size_t)lr * H + 4 * h;
            for (int j = 0; j < a.ht; j++) {
                const T* buf = wl + (j & 1) * CHUNK;
                if (j + 1 < a.ht) ffn_fetch<T, Cfg::PIECES, Cfg::W1_PIECES>(stg, w1, w2, j + 1);
                else ffn_fetch<T, Cfg::PIECES, Cfg::W1_PIECES>(stg, w1t, w2t, 0);       // the transposed pack's first chunk for pass 2
                attn_acc hv;
#pragma unroll
                for (int i = 0; i < 16; i++) hv[i] = 0.f;
#pragma unroll
                for (int k = 0; k < 4; k++) hv = mlp_mm(buf + k * MLP_TILE, lane, in_s, k, hv);
#pragma unroll
                for (int k = 0; k < 4; k++) hv = mlp_mm(buf + (4 + k) * MLP_TILE, lane, in_n, k, hv);
#pragma unroll
                for (int g = 0; g < 4; g++) *(float4*)(zr + 32 * j + 8 * g) = make_float4(hv[4 * g], hv[4 * g + 1], hv[4 * g + 2], hv[4 * g + 3]);
                MlpIn<T> hin;                                                    // (tile 0 only)
#pragma unroll
                for (int i = 0; i < 16; i++) hin.set(0, i, hv[i] * gelu_cdf(hv[i]));
#pragma unroll
                for (int t = 0; t < 4; t++) o[t] = mlp_mm(buf + (FFN_W1_TILES + t) * MLP_TILE, lane, hin, 0, o[t]);
                ffn_put<T, Cfg::PIECES>(wl + ((j + 1) & 1) * CHUNK, stg);
                wg_barrier();
            }
            ffn_row_stats(o, a.eps2, mean2, rstd2);

            // ---- the LN2 backward: dy, in o's place ----
            MlpIn<T> in_dy;
            {
                attn_acc q[4];
                float4 f[16];
                ffn_read_groups(f, a.g, (size_t)row * a.gs, a.g_vec, h);
#pragma unroll
                for (int t = 0; t < 4; t++) {
#pragma unroll
                    for (int i = 0; i < 16; i++) o[t][i] = (o[t][i] - mean2) * rstd2;
                }
#pragma unroll
                for (int qq = 0; qq < 16; qq++) {
                    const int t = qq >> 2, e = 4 * (qq & 3);
                    q[t][e] = f[qq].x; q[t][e + 1] = f[qq].y; q[t][e + 2] = f[qq].z; q[t][e + 3] = f[qq].w;
                }
                if (a.want_par) {
                    fb_spill(a.gg + o128, q, h);
                    attn_acc gx[4];
#pragma unroll
                    for (int t = 0; t < 4; t++) gx[t] = q[t] * o[t];
                    fb_spill(a.gx2 + o128, gx, h);
                }
                fb_ln_bwd(q, o, lnp + 256, rstd2, h);
                if (a.want_par) fb_spill(a.dy + o128, q, h);
                fb_operand(in_dy, q);
            }

            // ---- pass 2 over the transposed chunks: dh_j = W2_j^T dy, dz_j = dh_j gelu'(z_j), du += W1_j^T dz_j ----
            attn_acc du[8];
#pragma unroll
            for (int t = 0; t < 8; t++) {
#pragma unroll
                for (int i = 0; i < 16; i++) du[t][i] = 0.f;
            }
            float* dzr = a.dz + (size_t)lr * H + 4 * h;
            for (int j = 0; j < a.ht; j++) {
                const T* buf = wl + ((a.ht + j) & 1) * CHUNK;
                if (j + 1 < a.ht) ffn_fetch<T, Cfg::PIECES, Cfg::W1_PIECES>(stg, w1t, w2t, j + 1);
                float4 zv[4];
#pragma unroll
                for (int g = 0; g < 4; g++) zv[g] = *(const float4*)(zr + 32 * j + 8 * g);
                attn_acc dh;
#pragma unroll
                for (int i = 0; i < 16; i++) dh[i] = 0.f;
#pragma unroll
                for (int k = 0; k < 4; k++) dh = mlp_mm(buf + (FFN_W1_TILES + k) * MLP_TILE, lane, in_dy, k, dh);
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    dh[4 * g] *= ffn_gelu_grad(zv[g].x); dh[4 * g + 1] *= ffn_gelu_grad(zv[g].y);
                    dh[4 * g + 2] *= ffn_gelu_grad(zv[g].z); dh[4 * g + 3] *= ffn_gelu_grad(zv[g].w);
                }
                if (a.want_par) {
#pragma unroll
                    for (int g = 0; g < 4; g++) *(float4*)(dzr + 32 * j + 8 * g) = make_float4(dh[4 * g], dh[4 * g + 1], dh[4 * g + 2], dh[4 * g + 3]);
                }
                MlpIn<T> hin;                                                    // (tile 0 only)
#pragma unroll
                for (int i = 0; i < 16; i++) hin.set(0, i, dh[i]);
#pragma unroll
                for (int t = 0; t < 8; t++) du[t] = mlp_mm(buf + t * MLP_TILE, lane, hin, 0, du[t]);
                if (j + 1 < a.ht) ffn_put<T, Cfg::PIECES>(wl + ((a.ht + j + 1) & 1) * CHUNK, stg);
                wg_barrier();
            }
            if (!Cfg::RESIDENT) ffn_stage(wmt, wtg, WM);                         // (every wave is past the last chunk's barrier)

            // ---- ds = g + du[0:128] (g itself, not an operand); dn1 = du[128:256]; xh1 back from its slot ----
            if (a.want_ds && live) {
                float4 f[16];
                ffn_read_groups(f, a.g, (size_t)row * a.gs, a.g_vec, h);
#pragma unroll
                for (int qq = 0; qq < 16; qq++) {
                    const int t = qq >> 2, e = 4 * (qq & 3);
                    f[qq].x += du[t][e]; f[qq].y += du[t][e + 1]; f[qq].z += du[t][e + 2]; f[qq].w += du[t][e + 3];
                }
                ffn_write_groups(f, a.ds, (size_t)row * a.dss, a.ds_vec, h);
            }
#pragma unroll
            for (int t = 0; t < 4; t++) dn[t] = du[4 + t];
            fb_fill(o, a.dnx1 + o128, h);
        }

        // ---- the LN1 backward and da = Wm^T dm ----
        if (a.want_par) {
            fb_spill(a.dn1 + o128, dn, h);
            attn_acc nx[4];
#pragma unroll
            for (int t = 0; t < 4; t++) nx[t] = dn[t] * o[t];
            fb_spill(a.dnx1 + o128, nx, h);
        }
        fb_ln_bwd(dn, o, lnp, rstd1, h);
        if (a.want_par) fb_spill(a.dm + o128, dn, h);
        if (FFN && !Cfg::RESIDENT) wg_barrier();                                 // Wm^T is staged
        if (a.want_da) {                                                         // (uniform)
            MlpIn<T> in_dm;
            fb_operand(in_dm, dn);
#pragma unroll
            for (int t = 0; t < 4; t++) {
#pragma unroll
                for (int i = 0; i < 16; i++) o[t][i] = 0.f;
#pragma unroll
                for (int k = 0; k < 4; k++) o[t] = mlp_mm(wmt + (t * 4 + k) * MLP_TILE, lane, in_dm, k, o[t]);
            }
            if (live) {
                float4 f[16];
#pragma unroll
                for (int q = 0; q < 16; q++) f[q] = make_float4(o[q >> 2][4 * (q & 3)], o[q >> 2][4 * (q & 3) + 1], o[q >> 2][4 * (q & 3) + 2], o[q >> 2][4 * (q & 3) + 3]);
                ffn_write_groups(f, a.da, (size_t)row * a.das, a.da_vec, h);
            }
        }
        if (FFN && !Cfg::RESIDENT) wg_barrier();                                 // everybody is done with Wm^T before the next trip stages Wm
    }
}

// one product of the weight-gradient kernel: d W[O][I] += dz^T act(in) over the rows (colsum == 0), or the column sums of dz (colsum != 0)
struct FfnBwdProduct {
    const float* in;
    const float* dz;
    int in_stride, dz_stride, I, kts, ots, act, colsum, unit_end;      // ots: output tiles; a unit takes up to four of them
    uint32_t woff;
};
struct FfnBwdUnits {
    int nproducts, units_per_slice, slices, chunk, rows;
    float* part;
    uint32_t pstride;
    FfnBwdProduct p[FB_MAX_PRODUCTS];
};

template <typename T>
__global__ __launch_bounds__(FB_WG_THREADS) void layer_tail_bwd_wgrad_kernel(const FfnBwdUnits a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int u = blockIdx.x * FB_WG_WAVES + wave;
    if (u >= a.units_per_slice * a.slices) return;               // (no barrier in this kernel)
    const int slice = u / a.units_per_slice;
    int idx = u - slice * a.units_per_slice, pi = 0, first = 0;
    for (int i = 0; i < a.nproducts; i++)
        if (idx >= a.p[i].unit_end) { pi = i + 1; first = a.p[i].unit_end; }
    const FfnBwdProduct q = a.p[pi];
    idx -= first;
    const int lr0 = slice * FB_SLICE_ROWS, lr1 = min(lr0 + FB_SLICE_ROWS, a.rows);
    if (lr0 >= lr1) return;                                      // (the last chunk's empty slices keep the partial they have)
    const int kt = idx % q.kts, ot0 = 4 * (idx / q.kts), ot = min(4, q.ots - ot0);
    const float* hs = q.in + 32 * kt + r;
    const float* ds = q.dz + 32 * ot0 + r;
    float* pw = a.part + (size_t)slice * a.pstride + q.woff;
    const int col = 32 * kt + r, I = q.I;

    attn_acc acc[4];
    float bs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 4; t++) {
#pragma unroll
        for (int i = 0; i < 16; i++)
            acc[t][i] = (a.chunk > 0 && !q.colsum && t < ot) ? pw[(size_t)(32 * (ot0 + t) + attn_row(i, h)) * I + col] : 0.f;
    }
    for (int n0 = lr0; n0 < lr1; n0 += 16) {
        float bv[8], av[4][8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int n = n0 + mlp_wgrad_row<T>(j, h);
            const bool ok = n < lr1;
            float v = (ok && !q.colsum) ? hs[(size_t)n * q.in_stride] : 0.f;
            if (q.act) v = v * gelu_cdf(v);
            bv[j] = v;
#pragma unroll
            for (int t = 0; t < 4; t++) av[t][j] = (ok && t < ot) ? ds[(size_t)n * q.dz_stride + 32 * t] : 0.f;
        }
#pragma unroll
        for (int t = 0; t < 4; t++) {
            if (t < ot) {
                if (q.colsum) {
#pragma unroll
                    for (int j = 0; j < 8; j++) bs[t] += av[t][j];
                } else {
                    acc[t] = mlp_wgrad_mm(T(0), av[t], bv, acc[t]);
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 4; t++) {
        if (t < ot) {
            if (q.colsum) {                                      // (uniform over the wave)
                const float s = bs[t] + __shfl_xor(bs[t], 32, 64);
                const int o = 32 * (ot0 + t) + r;
                if (h == 0) pw[o] = (a.chunk > 0 ? pw[o] : 0.f) + s;
            } else {
#pragma unroll
                for (int i = 0; i < 16; i++) pw[(size_t)(32 * (ot0 + t) + attn_row(i, h)) * I + col] = acc[t][i];
            }
        }
    }
}

// the seven gradients, each where wanted: the slices' partials added in slice order
struct FfnBwdOut { uint32_t end[FB_OUTPUTS]; float* ptr[FB_OUTPUTS]; };
__global__ __launch_bounds__(256) void layer_tail_bwd_reduce_kernel(const float* __restrict__ part, uint32_t pstride, int slices, const FfnBwdOut o)
{
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= o.end[FB_OUTPUTS - 1]) return;
    float* dst = nullptr;
    uint32_t start = 0;
    bool found = false;
#pragma unroll
    for (int i = 0; i < FB_OUTPUTS; i++) {
        if (!found && j < o.end[i]) { dst = o.ptr[i]; start = i ? o.end[i ? i - 1 : 0] : 0; found = true; }
    }
    if (!dst) return;
    float s = 0.f;
    for (int z = 0; z < slices; z++) s += part[(size_t)z * pstride + j];
    dst[j - start] = s;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the entry points (the contract is in include/igs_rast.h)
// ---------------------------------------------------------------------------------------------------------------------------------
// a slice's partial: d Wm [128, 128], d ln1_w, d ln1_b, and with FFN d W1 [hidden, 256], d W2 [128, hidden], d ln2_w, d ln2_b
struct FfnBwdSizes { uint32_t end[FB_OUTPUTS], pstride; long long slot_rows, row_floats; int slices; };
static FfnBwdSizes ffn_bwd_sizes(long long T, int has_ffn, int hidden)
{
    FfnBwdSizes z = {};
    const uint32_t H = has_ffn ? (uint32_t)hidden : 0u;
    const uint32_t len[FB_OUTPUTS] = {128u * 128u, 128u, 128u, H * 256u, 128u * H, has_ffn ? 128u : 0u, has_ffn ? 128u : 0u};
    uint32_t e = 0;
    for (int i = 0; i < FB_OUTPUTS; i++) { e += len[i]; z.end[i] = e; }
    z.pstride = (e + 3u) & ~3u;
    const long long rows = T < FB_CHUNK_ROWS ? T : FB_CHUNK_ROWS;
    z.slot_rows = (rows + FFN_TRIP_ROWS - 1) / FFN_TRIP_ROWS * FFN_TRIP_ROWS;       // whole trips
    z.row_floats = has_ffn ? 2LL * H + 256 + 7 * 128 : 4 * 128;
    z.slices = (int)((z.slot_rows + FB_SLICE_ROWS - 1) / FB_SLICE_ROWS);
    return z;
}
static long long ffn_bwd_scratch(const FfnBwdSizes& z)
{
    return (z.slot_rows * z.row_floats + (long long)z.slices * z.pstride) * (long long)sizeof(float);
}

extern "C" long long igs_layer_tail_bwd_scratch_bytes(long long T, int compute_dtype, int has_ffn, int hidden)
{
    if (!dtype_ok(compute_dtype) || T < 0 || T > IGS_LAYER_TAIL_MAX_ROWS || (has_ffn && !ffn_hidden_ok(hidden))) return -1;
    return ffn_bwd_scratch(ffn_bwd_sizes(T, has_ffn, hidden));
}

extern "C" int igs_layer_tail_bwd(void* stream, long long T, int compute_dtype, int has_ffn, int hidden, const void* a, int a_dtype, long long a_stride,
                                  const void* s, int s_dtype, long long s_stride, const void* g, int g_dtype, long long g_stride, const void* wpack,
                                  const void* wpack_t, const float* ln1_w, const float* ln1_b, float eps1, const float* ln2_w, const float* ln2_b,
                                  float eps2, void* scratch, long long scratch_bytes, void* da, int da_dtype, long long da_stride, void* ds,
                                  int ds_dtype, long long ds_stride, float* dWm, float* dln1_w, float* dln1_b, float* dW1, float* dW2, float* dln2_w,
                                  float* dln2_b)
{
    const char* fn = "igs_layer_tail_bwd";
    if (!dtype_ok(compute_dtype) || !dtype_ok(a_dtype) || !dtype_ok(s_dtype) || !dtype_ok(g_dtype) || !dtype_ok(da_dtype) || !dtype_ok(ds_dtype))
        return fail_in(fn, "unknown dtype code");
    if (T < 0 || T > IGS_LAYER_TAIL_MAX_ROWS) return fail_in(fn, "T out of range (0..IGS_LAYER_TAIL_MAX_ROWS)");
    if (has_ffn && !ffn_hidden_ok(hidden)) return fail_in(fn, "hidden must be a multiple of 32 in 32..IGS_LAYER_TAIL_MAX_HIDDEN");
    if (ffn_stride_bad(a_stride) || ffn_stride_bad(s_stride) || ffn_stride_bad(g_stride) || ffn_stride_bad(da_stride) || ffn_stride_bad(ds_stride))
        return fail_in(fn, "a row stride is below the row length 128 or above IGS_TOKENS_MAX_STRIDE");
    if (!eps_ok(eps1) || (has_ffn && !eps_ok(eps2))) return fail_in(fn, "eps must be finite and >= 0");
    if (!ptr_aligned(dWm, 4) || !ptr_aligned(dln1_w, 4) || !ptr_aligned(dln1_b, 4) || !ptr_aligned(dW1, 4) || !ptr_aligned(dW2, 4) ||
        !ptr_aligned(dln2_w, 4) || !ptr_aligned(dln2_b, 4))
        return fail_in(fn, "a parameter gradient is not aligned to 4 bytes");
    if (!has_ffn) dW1 = dW2 = dln2_w = dln2_b = nullptr;                          // (nothing of the FFN exists: not written)
    const FfnBwdSizes z = ffn_bwd_sizes(T, has_ffn, hidden);
    float* const outs[FB_OUTPUTS] = {dWm, dln1_w, dln1_b, dW1, dW2, dln2_w, dln2_b};
    hipStream_t st_ = (hipStream_t)stream;
    if (T == 0) {
        for (int i = 0; i < FB_OUTPUTS; i++)
            if (outs[i]) HIP_TRY(hipMemsetAsync(outs[i], 0, (size_t)(z.end[i] - (i ? z.end[i - 1] : 0)) * sizeof(float), st_), "layer tail bwd zero-fill");
        return 0;
    }
    if (!a || !g || !wpack || !wpack_t || !ln1_w || !ln1_b || !scratch || (has_ffn && (!s || !ln2_w || !ln2_b))) return fail_in(fn, "NULL pointer");
    if (!ptr_aligned(a, dtype_bytes(a_dtype)) || !ptr_aligned(s, dtype_bytes(s_dtype)) || !ptr_aligned(g, dtype_bytes(g_dtype)) ||
        !ptr_aligned(da, dtype_bytes(da_dtype)) || !ptr_aligned(ds, dtype_bytes(ds_dtype)) || !ptr_aligned(ln1_w, 4) || !ptr_aligned(ln1_b, 4) ||
        (has_ffn && (!ptr_aligned(ln2_w, 4) || !ptr_aligned(ln2_b, 4))))
        return fail_in(fn, "a pointer is not aligned to its element size");
    if (!ptr_aligned(wpack, 16) || !ptr_aligned(wpack_t, 16)) return fail_in(fn, "wpack and wpack_t must be aligned to 16 bytes");
    if (!ptr_aligned(scratch, 16)) return fail_in(fn, "scratch must be aligned to 16 bytes");
    if (scratch_bytes < ffn_bwd_scratch(z)) return fail_in(fn, "scratch is smaller than igs_layer_tail_bwd_scratch_bytes");
    {
        const ByteSpan in[3] = {ffn_span(a, a_dtype, T, a_stride), s ? ffn_span(s, s_dtype, T, s_stride) : ByteSpan{0, 0},
                                ffn_span(g, g_dtype, T, g_stride)};
        for (int i = 0; i < 3; i++) {
            if (da && spans_overlap(ffn_span(da, da_dtype, T, da_stride), in[i])) return fail_in(fn, "da overlaps an input");
            if (ds && spans_overlap(ffn_span(ds, ds_dtype, T, ds_stride), in[i])) return fail_in(fn, "ds overlaps an input");
        }
    }
    bool want_par = false;
    for (int i = 0; i < FB_OUTPUTS; i++) want_par = want_par || outs[i];
    if (!da && !ds && !want_par) return 0;

    FfnBwdArgs k = {};
    k.a = TokPtr{a, a_dtype == IGS_DTYPE_F16}; k.s = TokPtr{s, s_dtype == IGS_DTYPE_F16}; k.g = TokPtr{g, g_dtype == IGS_DTYPE_F16};
    k.da = TokPtr{da, da_dtype == IGS_DTYPE_F16}; k.ds = TokPtr{ds, ds_dtype == IGS_DTYPE_F16};
    k.as = a_stride; k.ss = s_stride; k.gs = g_stride; k.das = da_stride; k.dss = ds_stride;
    k.a_vec = ffn_vec(a, a_dtype, a_stride); k.s_vec = ffn_vec(s, s_dtype, s_stride); k.g_vec = ffn_vec(g, g_dtype, g_stride);
    k.da_vec = ffn_vec(da, da_dtype, da_stride); k.ds_vec = ffn_vec(ds, ds_dtype, ds_stride);
    k.want_da = da != nullptr; k.want_ds = ds != nullptr; k.want_par = want_par;
    k.w = wpack; k.wt = wpack_t;
    k.ln1w = ln1_w; k.ln1b = ln1_b; k.ln2w = ln2_w;
    k.eps1 = eps1; k.eps2 = eps2;
    k.ht = has_ffn ? hidden / 32 : 0;
    const long long R = z.slot_rows, H = has_ffn ? hidden : 0;
    float* p = (float*)scratch;
    if (has_ffn) {
        k.z = p; p += R * H;
        k.dz = p; p += R * H;
        k.u = p; p += R * 256;
        k.dy = p; p += R * 128;
        k.gx2 = p; p += R * 128;
        k.gg = p; p += R * 128;
    }
    k.sa = p; p += R * 128;
    k.dm = p; p += R * 128;
    k.dnx1 = p; p += R * 128;
    k.dn1 = p; p += R * 128;

    // the weight-gradient kernel's products, in the order of a slice's partial
    FfnBwdUnits wu = {};
    wu.part = p; wu.pstride = z.pstride; wu.slices = z.slices;
    auto add = [&](const float* in, int in_stride, const float* dz, int dz_stride, int I, int kts, int ots, int act, int colsum, uint32_t woff) {
        FfnBwdProduct& q = wu.p[wu.nproducts++];
        q.in = in; q.in_stride = in_stride; q.dz = dz; q.dz_stride = dz_stride; q.I = I; q.kts = kts; q.ots = ots; q.act = act; q.colsum = colsum;
        q.woff = woff;
        wu.units_per_slice += kts * ((ots + 3) / 4);
        q.unit_end = wu.units_per_slice;
    };
    if (dWm) add(k.sa, 128, k.dm, 128, 128, 4, 4, 0, 0, 0);
    if (dln1_w) add(k.dnx1, 128, k.dnx1, 128, 1, 1, 4, 0, 1, z.end[0]);
    if (dln1_b) add(k.dn1, 128, k.dn1, 128, 1, 1, 4, 0, 1, z.end[1]);
    if (dW1) add(k.u, 256, k.dz, (int)H, 256, 8, k.ht, 0, 0, z.end[2]);
    if (dW2) add(k.z, (int)H, k.dy, 128, (int)H, k.ht, 4, 1, 0, z.end[3]);
    if (dln2_w) add(k.gx2, 128, k.gx2, 128, 1, 1, 4, 0, 1, z.end[4]);
    if (dln2_b) add(k.gg, 128, k.gg, 128, 1, 1, 4, 0, 1, z.end[5]);

    const bool half = compute_dtype == IGS_DTYPE_F16;
    const long long cus = mlp_cus();
    const dim3 block(FFN_THREADS);
    for (long long r0 = 0; r0 < T; r0 += FB_CHUNK_ROWS) {
        k.row0 = r0;
        k.rows = (int)(T - r0 < FB_CHUNK_ROWS ? T - r0 : FB_CHUNK_ROWS);
        const long long trips = (k.rows + FFN_TRIP_ROWS - 1) / FFN_TRIP_ROWS;
        const dim3 grid((unsigned)(trips < cus ? trips : cus));
        if (has_ffn) {
            if (half) hipLaunchKernelGGL((layer_tail_bwd_rows_kernel<_Float16, true>), grid, block, 0, st_, k);
            else hipLaunchKernelGGL((layer_tail_bwd_rows_kernel<float, true>), grid, block, 0, st_, k);
        } else {
            if (half) hipLaunchKernelGGL((layer_tail_bwd_rows_kernel<_Float16, false>), grid, block, 0, st_, k);
            else hipLaunchKernelGGL((layer_tail_bwd_rows_kernel<float, false>), grid, block, 0, st_, k);
        }
        if (want_par) {
            wu.chunk = (int)(r0 / FB_CHUNK_ROWS); wu.rows = k.rows;
            const int units = wu.units_per_slice * wu.slices;
            const dim3 wgrid((unsigned)((units + FB_WG_WAVES - 1) / FB_WG_WAVES)), wblock(FB_WG_THREADS);
            if (half) hipLaunchKernelGGL((layer_tail_bwd_wgrad_kernel<_Float16>), wgrid, wblock, 0, st_, wu);
            else hipLaunchKernelGGL((layer_tail_bwd_wgrad_kernel<float>), wgrid, wblock, 0, st_, wu);
        }
    }
    if (want_par) {
        FfnBwdOut o = {};
        for (int i = 0; i < FB_OUTPUTS; i++) { o.end[i] = z.end[i]; o.ptr[i] = outs[i]; }
        hipLaunchKernelGGL(layer_tail_bwd_reduce_kernel, dim3((z.end[FB_OUTPUTS - 1] + 255) / 256), dim3(256), 0, st_, wu.part, z.pstride, z.slices, o);
    }
    HIP_TRY(hipGetLastError(), "layer tail bwd launch");
    return 0;
}
