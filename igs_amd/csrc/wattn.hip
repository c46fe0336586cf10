// wattn.hip -- swin window attention softmax(scale Q K^T + mask) V for the motion-feature transformers (unimatch: one head of 128 channels
// over the K x K windows of an h x w feature map, optionally shifted by half a window; igs/models/unimatch/attention.py:8-16 and 45-104,
// the mask of igs/models/unimatch/utils.py:84-108), forward and backward, on the gfx950 matrix cores.  include/igs_rast.h states the
// contract, DESIGN.md section 17 the budget and the figures.
//
// attn.hip's scheme with two changes.  (a) The roll, the window split, the merge and the roll back are index arithmetic: a workgroup is
// given a window (wy, wx); the token j of that window is the original token ((y' + sh) mod h) w + (x' + sw) mod w with y' = wy wh + j / ww,
// x' = wx ww + j mod ww, computed once per staged row (wattn_token) and once per owned row.  Inputs are read and outputs written at
// the original positions, so q, k, v, out, lse and the gradients are all [B, h w, 128] in the caller's order.  The region of a rolled
// position (0..8) travels with the staged rows into LDS; a pair of tokens of different regions gets -100 added to its scaled score (a
// finite addend, as the reference has it), folded into the fma that scales the score.  A window that holds one region (every window of an
// unshifted call, every window off the last row and column of a shifted one) never looks at the regions: a workgroup-uniform branch.
// (b) D = 128 is two 64-channel halves: a row fragment of attn_common.h covers 64 channels, a score is the sum of two fragment products
// in one accumulator (one fma chain of 128), and the tile x image products run once per block of 64 output channels.  The float32 d K /
// d V pass owns 64 output channels per workgroup (WATTN_DKDV_BLOCKS; twice the workgroups, each recomputes S and d P).
//   (1) wattn_fwd_kernel    owns 128 queries of a window, walks the window's keys 64 at a time: S^T = K Q^T, online softmax per lane,
//                           O^T += V^T P^T in four accumulator tiles.
//   (2) wattn_delta_kernel  delta = rowsum(d O * O), float32, one thread per token (no window arithmetic: original order).
//   (3) wattn_dkdv_kernel   owns 128 keys of a window, walks its queries: P recomputed from lse, d V += P^T d O, d K += d S^T Q.
//   (4) wattn_dq_kernel     owns 128 queries, walks the keys: d Q += d S K.
// No float atomics: every output element has one owner that adds in a fixed order, so two runs agree bit for bit.
#include "common.h"
#include "host_api.h"
#include "attn_common.h"
#include <math.h>

#define WATTN_THREADS 256
#define WATTN_D 128
#define WATTN_ROWS 64                   // rows of one LDS image
#define WATTN_OWN 128                   // queries (keys) owned by a workgroup: 32 per wave
#define WATTN_TS 72                     // row length of the transposed half image [128 d][72]
#define WATTN_MASK_LOG2 (-144.26950408889634f)      // -100 log2(e): the reference's addend in the exp2 domain
#define WATTN_MAX_TOKENS (1 << 24)      // B h w

struct WattnGeom { int h, w, K, wh, ww, sh, sw, Lw, tiles; };        // (sh, sw) = (wh / 2, ww / 2) when shifted, else 0; Lw = wh ww
struct WattnView { void* p; long long sb, st; };                      // [B, h w, 128] with element strides; the stride on d is 1
struct WattnArgs {
    WattnGeom g;
    float c, scale;                                                   // c = scale * log2(e)
    WattnView q, k, v, o, go, dq, dk, dv;
    float* lse;                                                       // [B, h w] in original token order, like delta
    float* delta;
};

template <typename T> struct WattnCfg;
// LS: row length of a row-major image (128 channels + 16 bytes); EPC elements per 16-byte piece, CPR pieces per row, NCH pieces per thread
template <> struct WattnCfg<_Float16> { enum { LS = 136, EPC = 8, CPR = 16, NCH = 4, HALF = 1, COLS = WATTN_D * WATTN_TS }; typedef attn_h8 vec; };
template <> struct WattnCfg<float> { enum { LS = 132, EPC = 4, CPR = 32, NCH = 8, HALF = 0, COLS = WATTN_ROWS * 132 }; typedef attn_f4 vec; };
// channel blocks (of 64) that one workgroup of the d K / d V pass owns
template <typename T> struct WattnDkdv { enum { BLOCKS = AttnCfg<T>::HALF ? 2 : 1 }; };

template <typename T> __device__ __forceinline__ T* wattn_at(const WattnView& t, int b) { return (T*)t.p + (long long)b * t.sb; }

// the original token of token j of the window whose first rolled position is (y0, x0), and the region of its rolled position
__device__ __forceinline__ int wattn_token(const WattnGeom& g, int y0, int x0, int j, int& region)
{
    const int jy = j / g.ww, jx = j - jy * g.ww;
    const int yp = y0 + jy, xp = x0 + jx;
    int y = yp + g.sh, x = xp + g.sw;
    if (y >= g.h) y -= g.h;
    if (x >= g.w) x -= g.w;
    region = 3 * ((yp >= g.h - g.wh) + (yp >= g.h - g.sh)) + (xp >= g.w - g.ww) + (xp >= g.w - g.sw);
    return y * g.w + x;
}

// what a workgroup works on: the example, the window and the tile of 128 owned rows; `masked`: the window holds more than one region
struct WattnBlock { int b, y0, x0, tile; bool masked; };
__device__ __forceinline__ WattnBlock wattn_decode(const WattnGeom& g, unsigned idx)
{
    WattnBlock k;
    k.tile = idx % (unsigned)g.tiles;
    const unsigned rest = idx / (unsigned)g.tiles, nw = (unsigned)(g.K * g.K), win = rest % nw;
    k.b = rest / nw;
    const int wy = win / (unsigned)g.K, wx = win % (unsigned)g.K;
    k.y0 = wy * g.wh;
    k.x0 = wx * g.ww;
    k.masked = (g.sh | g.sw) != 0 && (wy == g.K - 1 || wx == g.K - 1);
    return k;
}

// The rows of one 64-row tile that this thread stages: their original tokens (-1 behind the window's end) and their regions, 4 bits each.
template <typename T> struct WattnRows {
    typedef WattnCfg<T> C;
    int tok[C::NCH];
    unsigned regions;
    __device__ __forceinline__ void find(const WattnGeom& g, const WattnBlock& k, int row0)
    {
        regions = 0;
#pragma unroll
        for (int u = 0; u < C::NCH; u++) {
            const int j = row0 + (threadIdx.x + WATTN_THREADS * u) / C::CPR;
            int reg = 0;
            tok[u] = j < g.Lw ? wattn_token(g, k.y0, k.x0, j, reg) : -1;
            regions |= (unsigned)reg << (4 * u);
        }
    }
    // the regions of the tile's rows: one writer per row
    __device__ __forceinline__ void write_regions(int* tab) const
    {
        if (threadIdx.x % C::CPR == 0) {
#pragma unroll
            for (int u = 0; u < C::NCH; u++) tab[(threadIdx.x + WATTN_THREADS * u) / C::CPR] = (regions >> (4 * u)) & 15;
        }
    }
};

// 64 rows of a [.., h w, 128] operand on their way into LDS: 16-byte pieces in registers (rows behind the window's end are zeros), then
// either image.  where(row) of the transposed image: the accumulator's register order inside every group of 16 rows (attn.hip).
template <typename T> struct WattnStage {
    typedef WattnCfg<T> C;
    typename C::vec v[C::NCH];
    __device__ __forceinline__ void load(const T* base, long long st, const WattnRows<T>& rows)
    {
#pragma unroll
        for (int u = 0; u < C::NCH; u++) {
            const int col = ((threadIdx.x + WATTN_THREADS * u) % C::CPR) * C::EPC;
            typename C::vec z = {};
            v[u] = rows.tok[u] >= 0 ? *(const typename C::vec*)(base + (long long)rows.tok[u] * st + col) : z;
        }
    }
    __device__ __forceinline__ void write_rows(T* img) const
    {
#pragma unroll
        for (int u = 0; u < C::NCH; u++) {
            const int c = threadIdx.x + WATTN_THREADS * u, row = c / C::CPR, col = (c % C::CPR) * C::EPC;
            *(typename C::vec*)(img + row * C::LS + col) = v[u];
        }
    }
    __device__ __forceinline__ void write_transposed(T* img) const
    {
#pragma unroll
        for (int u = 0; u < C::NCH; u++) {
            const int c = threadIdx.x + WATTN_THREADS * u, row = c / C::CPR, col = (c % C::CPR) * C::EPC;
            const int where = (row & ~15) | (((row >> 2) & 1) << 3) | (((row >> 3) & 1) << 2) | (row & 3);
#pragma unroll
            for (int e = 0; e < C::EPC; e++) img[(col + e) * WATTN_TS + where] = v[u][e];
        }
    }
    // the image that wattn_mm_image reads
    __device__ __forceinline__ void write_columns(T* img) const { if constexpr (C::HALF != 0) write_transposed(img); else write_rows(img); }
};

// a lane's share of one 128-channel row
template <typename T> struct WattnRow { AttnRow<T> lo, hi; };
template <typename T> __device__ __forceinline__ void wattn_load_row(WattnRow<T>& f, const T* row, int h)
{
    attn_load_row(f.lo, row, h);
    attn_load_row(f.hi, row + 64, h);
}
// X[i][j] = sum_d A[i][d] B[j][d] over the 128 channels, A's row read from an LDS row image one half at a time
template <typename T> __device__ __forceinline__ attn_acc wattn_mm_rows(const T* arow, int h, const WattnRow<T>& b)
{
    attn_acc x = {};
    AttnRow<T> f;
    attn_load_row(f, arow, h);
    x = attn_mm_rows(f, b.lo, x);
    attn_load_row(f, arow + 64, h);
    return attn_mm_rows(f, b.hi, x);
}

// The tile x image product of attn_common.h for the block cb of 64 channels of a column image (half: [128 d][72] transposed; float: the
// row image [64][132] itself).
template <bool XA>
__device__ __forceinline__ void wattn_mm_image(const attn_acc& x, const _Float16* img, int cb, int ro, int r, int h, attn_acc& y0, attn_acc& y1)
{
    attn_mm_image<XA>(x, img + cb * 64 * WATTN_TS, ro, r, h, y0, y1);
}
template <bool XA>
__device__ __forceinline__ void wattn_mm_image(const attn_acc& x, const float* img, int cb, int ro, int r, int h, attn_acc& y0, attn_acc& y1)
{
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const float* row = img + (ro + attn_row(i, 0) + 4 * h) * WattnCfg<float>::LS + 64 * cb + r;
        const float m0 = row[0], m1 = row[32];
        if (XA) {
            y0 = __builtin_amdgcn_mfma_f32_32x32x2f32(x[i], m0, y0, 0, 0, 0);
            y1 = __builtin_amdgcn_mfma_f32_32x32x2f32(x[i], m1, y1, 0, 0, 0);
        } else {
            y0 = __builtin_amdgcn_mfma_f32_32x32x2f32(m0, x[i], y0, 0, 0, 0);
            y1 = __builtin_amdgcn_mfma_f32_32x32x2f32(m1, x[i], y1, 0, 0, 0);
        }
    }
}

// the scaled score in the exp2 domain, with the mask's addend where the regions differ
__device__ __forceinline__ float wattn_score(float s, float c, int kreg, int qreg) { return fmaf(s, c, kreg != qreg ? WATTN_MASK_LOG2 : 0.f); }

// rows j = j0 + row(i, h) of the window, as original tokens, of a Z tile pair (channel on the lane) for the channel block cb, scaled; rows
// behind the window's end stay unwritten
template <typename T>
__device__ __forceinline__ void wattn_store_z(T* base, long long st, const WattnGeom& g, const WattnBlock& k, int j0, int cb, int r, int h,
                                              const attn_acc& z0, const attn_acc& z1, float f)
{
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int j = j0 + attn_row(i, 0) + 4 * h;
        if (j < g.Lw) {
            int reg;
            T* p = base + (long long)wattn_token(g, k.y0, k.x0, j, reg) * st + 64 * cb + r;
            p[0] = (T)(z0[i] * f);
            p[32] = (T)(z1[i] * f);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (1) forward
// ---------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(WATTN_THREADS)
wattn_fwd_kernel(WattnArgs a)
{
    typedef WattnCfg<T> C;
    __shared__ __attribute__((aligned(16))) T kimg[WATTN_ROWS * C::LS];
    __shared__ __attribute__((aligned(16))) T vimg[C::COLS];
    __shared__ __attribute__((aligned(16))) int kreg[WATTN_ROWS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const WattnGeom& g = a.g;
    const WattnBlock blk = wattn_decode(g, blockIdx.x);
    const int q0 = blk.tile * WATTN_OWN + 32 * w, jq = q0 + r;
    const bool live = q0 < g.Lw;                              // (wave-uniform; a dead wave still stages and meets the barriers)
    int qreg;
    const int qtok = wattn_token(g, blk.y0, blk.x0, min(jq, g.Lw - 1), qreg);
    WattnRow<T> qf;
    wattn_load_row(qf, wattn_at<const T>(a.q, blk.b) + (long long)qtok * a.q.st, h);
    const T* kb = wattn_at<const T>(a.k, blk.b);
    const T* vb = wattn_at<const T>(a.v, blk.b);
    WattnRows<T> rows;
    WattnStage<T> sk, sv;
    rows.find(g, blk, 0);
    sk.load(kb, a.k.st, rows);
    sv.load(vb, a.v.st, rows);
    attn_acc o[4] = {};
    float m = -INFINITY, l = 0.f;                             // the running max of the exp2-domain scores; this lane's share of the sum
    for (int k0 = 0; k0 < g.Lw; k0 += WATTN_ROWS) {
        wg_barrier();
        sk.write_rows(kimg);
        sv.write_columns(vimg);
        if (blk.masked) rows.write_regions(kreg);
        wg_barrier();
        if (k0 + WATTN_ROWS < g.Lw) {
            rows.find(g, blk, k0 + WATTN_ROWS);
            sk.load(kb, a.k.st, rows);
            sv.load(vb, a.v.st, rows);
        }
        if (!live) continue;
#pragma unroll
        for (int sub = 0; sub < 2; sub++) {
            const int ro = 32 * sub, kk = k0 + ro;
            if (kk >= g.Lw) break;                            // (uniform)
            attn_acc s = wattn_mm_rows(kimg + (ro + r) * C::LS, h, qf);      // rows: key, column: query
            const bool ragged = kk + 32 > g.Lw;
            float mx = m;
#pragma unroll
            for (int gq = 0; gq < 4; gq++) {
                int kr[4] = {qreg, qreg, qreg, qreg};
                if (blk.masked) {                             // (uniform)
#pragma unroll
                    for (int e = 0; e < 4; e++) kr[e] = kreg[ro + 8 * gq + 4 * h + e];
                }
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const int i = 4 * gq + e;
                    float t = wattn_score(s[i], a.c, kr[e], qreg);
                    if (ragged && kk + attn_row(i, 0) + 4 * h >= g.Lw) t = -INFINITY;
                    s[i] = t;
                    mx = fmaxf(mx, t);
                }
            }
            mx = fmaxf(mx, __shfl_xor(mx, 32));               // finite: key kk itself is real
            if (__any(mx > m)) {                              // (wave-uniform) some query's max grew; otherwise every factor is exactly 1
                const float alpha = attn_exp2(m - mx);        // (0 at the first tile)
                m = mx;
                l *= alpha;
#pragma unroll
                for (int t = 0; t < 4; t++) o[t] *= alpha;
            }
            float ls = 0.f;
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const float p = attn_exp2(s[i] - mx);
                s[i] = p;
                ls += p;
            }
            l += ls;
            // O^T[d][query] += sum_key V[key][d] P^T[key][query]
#pragma unroll
            for (int cb = 0; cb < 2; cb++) {
                if constexpr (C::HALF != 0) {
                    wattn_mm_image<false>(s, vimg, cb, ro, r, h, o[2 * cb], o[2 * cb + 1]);
                } else {                                      // float32: the fma chain of the matrix unit restarts with every 32 keys
                    attn_acc t0 = {}, t1 = {};
                    wattn_mm_image<false>(s, vimg, cb, ro, r, h, t0, t1);
                    o[2 * cb] += t0;
                    o[2 * cb + 1] += t1;
                }
            }
        }
    }
    if (!live || jq >= g.Lw) return;
    const float lt = l + __shfl_xor(l, 32);
    T* op = wattn_at<T>(a.o, blk.b) + (long long)qtok * a.o.st;
#pragma unroll
    for (int t = 0; t < 4; t++) {
#pragma unroll
        for (int gq = 0; gq < 4; gq++) {
            const int d = 32 * t + 8 * gq + 4 * h;
            if constexpr (C::HALF != 0) {
                h4_t x;
#pragma unroll
                for (int e = 0; e < 4; e++) x[e] = (_Float16)(o[t][4 * gq + e] / lt);
                *(h4_t*)(op + d) = x;
            } else {
                attn_f4 x;
#pragma unroll
                for (int e = 0; e < 4; e++) x[e] = o[t][4 * gq + e] / lt;
                *(attn_f4*)(op + d) = x;
            }
        }
    }
    if (a.lse && h == 0) a.lse[(size_t)blk.b * g.h * g.w + qtok] = (m + log2f(lt)) * 0.6931471805599453f;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (2) delta = rowsum(d O * O): one thread per token, channels in order
// ---------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(WATTN_THREADS)
wattn_delta_kernel(WattnArgs a, int B)
{
    typedef WattnCfg<T> C;
    const size_t L = (size_t)a.g.h * a.g.w, idx = (size_t)blockIdx.x * WATTN_THREADS + threadIdx.x;
    if (idx >= (size_t)B * L) return;
    const int b = idx / L;
    const long long t = idx % L;
    const T* o = wattn_at<const T>(a.o, b) + t * a.o.st;
    const T* gr = wattn_at<const T>(a.go, b) + t * a.go.st;
    float s = 0.f;
    for (int d = 0; d < WATTN_D; d += C::EPC) {
        const typename C::vec x = *(const typename C::vec*)(o + d), y = *(const typename C::vec*)(gr + d);
#pragma unroll
        for (int e = 0; e < C::EPC; e++) s = fmaf((float)x[e], (float)y[e], s);
    }
    a.delta[idx] = s;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (3) d K and d V: the workgroup owns 128 keys of a window (and NB of the two channel blocks) and walks the window's queries
// ---------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(WATTN_THREADS)
wattn_dkdv_kernel(WattnArgs a)
{
    typedef WattnCfg<T> C;
    enum { NB = WattnDkdv<T>::BLOCKS };
    __shared__ __attribute__((aligned(16))) T qimg[WATTN_ROWS * C::LS];
    __shared__ __attribute__((aligned(16))) T gimg[WATTN_ROWS * C::LS];
    __shared__ __attribute__((aligned(16))) T qcol[C::HALF ? C::COLS : 8];               // the transposed images (half only: the float
    __shared__ __attribute__((aligned(16))) T gcol[C::HALF ? C::COLS : 8];               // images are read both ways)
    __shared__ __attribute__((aligned(16))) float lse2[WATTN_ROWS];
    __shared__ __attribute__((aligned(16))) float dlt[WATTN_ROWS];
    __shared__ __attribute__((aligned(16))) int qreg[WATTN_ROWS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const WattnGeom& g = a.g;
    const WattnBlock blk = wattn_decode(g, blockIdx.x / (2 / NB));
    const int cb0 = NB == 2 ? 0 : (int)(blockIdx.x & 1);      // the first channel block of this workgroup
    const int kbase = blk.tile * WATTN_OWN + 32 * w;
    const bool live = kbase < g.Lw;
    int kreg;
    const int ktok = wattn_token(g, blk.y0, blk.x0, min(kbase + r, g.Lw - 1), kreg);
    WattnRow<T> kf, vf;
    wattn_load_row(kf, wattn_at<const T>(a.k, blk.b) + (long long)ktok * a.k.st, h);
    wattn_load_row(vf, wattn_at<const T>(a.v, blk.b) + (long long)ktok * a.v.st, h);
    const T* qb = wattn_at<const T>(a.q, blk.b);
    const T* gb = wattn_at<const T>(a.go, blk.b);
    const float* lb = a.lse + (size_t)blk.b * g.h * g.w;
    const float* db = a.delta + (size_t)blk.b * g.h * g.w;
    WattnRows<T> rows;
    WattnStage<T> sq, sg;
    float nl = INFINITY, nd = 0.f;                            // a row behind the last query: lse = +inf, so that its P is zero
    int nr = 0;
    auto side = [&](int q0) {                                 // lse, delta and region of the tile's row threadIdx.x
        nl = INFINITY; nd = 0.f; nr = 0;
        if (threadIdx.x < WATTN_ROWS && q0 + (int)threadIdx.x < g.Lw) {
            const int t = wattn_token(g, blk.y0, blk.x0, q0 + threadIdx.x, nr);
            nl = lb[t] * 1.4426950408889634f;
            nd = db[t];
        }
    };
    rows.find(g, blk, 0);
    sq.load(qb, a.q.st, rows);
    sg.load(gb, a.go.st, rows);
    side(0);
    attn_acc dk[2 * NB] = {}, dv[2 * NB] = {};
    for (int q0 = 0; q0 < g.Lw; q0 += WATTN_ROWS) {
        wg_barrier();
        sq.write_rows(qimg);
        sg.write_rows(gimg);
        if constexpr (C::HALF != 0) { sq.write_transposed(qcol); sg.write_transposed(gcol); }
        if (threadIdx.x < WATTN_ROWS) { lse2[threadIdx.x] = nl; dlt[threadIdx.x] = nd; qreg[threadIdx.x] = nr; }
        wg_barrier();
        if (q0 + WATTN_ROWS < g.Lw) {
            rows.find(g, blk, q0 + WATTN_ROWS);
            sq.load(qb, a.q.st, rows);
            sg.load(gb, a.go.st, rows);
            side(q0 + WATTN_ROWS);
        }
        if (!live) continue;
#pragma unroll
        for (int sub = 0; sub < 2; sub++) {
            const int ro = 32 * sub;
            if (q0 + ro >= g.Lw) break;                       // (uniform)
            attn_acc s = wattn_mm_rows(qimg + (ro + r) * C::LS, h, kf);      // rows: query, column: key
            attn_acc dp = wattn_mm_rows(gimg + (ro + r) * C::LS, h, vf);
#pragma unroll
            for (int gq = 0; gq < 4; gq++) {
                const attn_f4 l4 = *(const attn_f4*)(lse2 + ro + 8 * gq + 4 * h), d4 = *(const attn_f4*)(dlt + ro + 8 * gq + 4 * h);
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const int i = 4 * gq + e;
                    float p;
                    if (blk.masked) p = attn_exp2(wattn_score(s[i], a.c, kreg, qreg[ro + 8 * gq + 4 * h + e]) - l4[e]);      // (uniform)
                    else p = attn_exp2(fmaf(s[i], a.c, -l4[e]));
                    s[i] = p;
                    dp[i] = p * (dp[i] - d4[e]);
                }
            }
#pragma unroll
            for (int n = 0; n < NB; n++) {
                wattn_mm_image<true>(s, C::HALF ? gcol : gimg, cb0 + n, ro, r, h, dv[2 * n], dv[2 * n + 1]);      // d V[key][d] += sum_q P[q][key] d O[q][d]
                wattn_mm_image<true>(dp, C::HALF ? qcol : qimg, cb0 + n, ro, r, h, dk[2 * n], dk[2 * n + 1]);     // d K[key][d] += sum_q d S[q][key] Q[q][d]
            }
        }
    }
    if (!live) return;
#pragma unroll
    for (int n = 0; n < NB; n++) {
        if (a.dk.p) wattn_store_z(wattn_at<T>(a.dk, blk.b), a.dk.st, g, blk, kbase, cb0 + n, r, h, dk[2 * n], dk[2 * n + 1], a.scale);
        if (a.dv.p) wattn_store_z(wattn_at<T>(a.dv, blk.b), a.dv.st, g, blk, kbase, cb0 + n, r, h, dv[2 * n], dv[2 * n + 1], 1.f);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (4) d Q: the workgroup owns 128 queries of a window and walks the window's keys
// ---------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(WATTN_THREADS)
wattn_dq_kernel(WattnArgs a)
{
    typedef WattnCfg<T> C;
    __shared__ __attribute__((aligned(16))) T kimg[WATTN_ROWS * C::LS];
    __shared__ __attribute__((aligned(16))) T vimg[WATTN_ROWS * C::LS];
    __shared__ __attribute__((aligned(16))) T kcol[C::HALF ? C::COLS : 8];
    __shared__ __attribute__((aligned(16))) int kreg[WATTN_ROWS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const WattnGeom& g = a.g;
    const WattnBlock blk = wattn_decode(g, blockIdx.x);
    const int q0 = blk.tile * WATTN_OWN + 32 * w;
    const bool live = q0 < g.Lw;
    int qreg;
    const int qtok = wattn_token(g, blk.y0, blk.x0, min(q0 + r, g.Lw - 1), qreg);
    WattnRow<T> qf, gf;
    wattn_load_row(qf, wattn_at<const T>(a.q, blk.b) + (long long)qtok * a.q.st, h);
    wattn_load_row(gf, wattn_at<const T>(a.go, blk.b) + (long long)qtok * a.go.st, h);
    const float l2 = a.lse[(size_t)blk.b * g.h * g.w + qtok] * 1.4426950408889634f;
    const float dl = a.delta[(size_t)blk.b * g.h * g.w + qtok];
    const T* kb = wattn_at<const T>(a.k, blk.b);
    const T* vb = wattn_at<const T>(a.v, blk.b);
    WattnRows<T> rows;
    WattnStage<T> sk, sv;
    rows.find(g, blk, 0);
    sk.load(kb, a.k.st, rows);
    sv.load(vb, a.v.st, rows);
    attn_acc dq[4] = {};
    for (int k0 = 0; k0 < g.Lw; k0 += WATTN_ROWS) {
        wg_barrier();
        sk.write_rows(kimg);
        sv.write_rows(vimg);
        if constexpr (C::HALF != 0) sk.write_transposed(kcol);
        if (blk.masked) rows.write_regions(kreg);
        wg_barrier();
        if (k0 + WATTN_ROWS < g.Lw) {
            rows.find(g, blk, k0 + WATTN_ROWS);
            sk.load(kb, a.k.st, rows);
            sv.load(vb, a.v.st, rows);
        }
        if (!live) continue;
#pragma unroll
        for (int sub = 0; sub < 2; sub++) {
            const int ro = 32 * sub, kk = k0 + ro;
            if (kk >= g.Lw) break;                            // (uniform)
            attn_acc s = wattn_mm_rows(kimg + (ro + r) * C::LS, h, qf);      // rows: key, column: query
            attn_acc dp = wattn_mm_rows(vimg + (ro + r) * C::LS, h, gf);
            const bool ragged = kk + 32 > g.Lw;
#pragma unroll
            for (int i = 0; i < 16; i++) {
                float p;
                if (blk.masked) p = attn_exp2(wattn_score(s[i], a.c, kreg[ro + attn_row(i, 0) + 4 * h], qreg) - l2);      // (uniform)
                else p = attn_exp2(fmaf(s[i], a.c, -l2));
                if (ragged && kk + attn_row(i, 0) + 4 * h >= g.Lw) p = 0.f;
                s[i] = p * (dp[i] - dl);
            }
#pragma unroll
            for (int cb = 0; cb < 2; cb++)                    // d Q[q][d] += sum_key d S^T[key][q] K[key][d]
                wattn_mm_image<true>(s, C::HALF ? kcol : kimg, cb, ro, r, h, dq[2 * cb], dq[2 * cb + 1]);
        }
    }
    if (!live) return;
#pragma unroll
    for (int cb = 0; cb < 2; cb++) wattn_store_z(wattn_at<T>(a.dq, blk.b), a.dq.st, g, blk, q0, cb, r, h, dq[2 * cb], dq[2 * cb + 1], a.scale);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------------------
static const char* wattn_size_error(int B, int h, int w, int K, int shift, int D, int dtype)
{
    if (D != WATTN_D) return "D must be 128 (the only channel count provided)";
    if (!dtype_ok(dtype)) return "unknown dtype code (IGS_DTYPE_F32 or IGS_DTYPE_F16)";
    if (B < 0 || B > IGS_WINDOW_ATTN_MAX_BATCH) return "B out of range (0..IGS_WINDOW_ATTN_MAX_BATCH)";
    if (h < 1 || w < 1 || h > WATTN_MAX_TOKENS || w > WATTN_MAX_TOKENS || (long long)h * w > WATTN_MAX_TOKENS) return "h, w out of range (1 <= h, w; h * w <= 2^24)";
    if ((long long)B * h * w > WATTN_MAX_TOKENS) return "B * h * w out of range (at most 2^24)";
    if (K < 1 || K > h || K > w) return "K out of range (1..min(h, w))";
    if (h % K || w % K) return "h and w must be multiples of K";
    if (shift && (h / K < 2 || w / K < 2)) return "a shifted call needs windows of at least 2 x 2 tokens";
    return nullptr;
}
static const char* wattn_view_error(int dtype, long long sb, long long st)
{
    const long long es = dtype == IGS_DTYPE_F16 ? 2 : 4;
    if (sb < 0 || st < 0) return "negative stride";
    if ((sb * es) % 16 || (st * es) % 16) return "the b / token strides must be multiples of 16 bytes";
    return nullptr;
}
// an output view: rows must not alias one another (every element has one owner that writes it)
static const char* wattn_out_error(int B, long long L, long long sb, long long st)
{
    if ((L > 1 && st < WATTN_D) || (B > 1 && sb < WATTN_D)) return "output strides overlap (a stride below D on a dimension longer than 1)";
    return nullptr;
}
static WattnView wattn_view(const void* p, long long sb, long long st) { WattnView t; t.p = (void*)p; t.sb = sb; t.st = st; return t; }
static WattnGeom wattn_geom(int h, int w, int K, int shift)
{
    WattnGeom g;
    g.h = h; g.w = w; g.K = K; g.wh = h / K; g.ww = w / K;
    g.sh = shift ? g.wh / 2 : 0; g.sw = shift ? g.ww / 2 : 0;
    g.Lw = g.wh * g.ww;
    g.tiles = (g.Lw + WATTN_OWN - 1) / WATTN_OWN;
    return g;
}

extern "C" size_t igs_window_attn_bwd_scratch_bytes(int B, int h, int w, int K, int D, int dtype)
{
    if (wattn_size_error(B, h, w, K, 0, D, dtype)) return 0;
    return align_up((size_t)B * h * w * 4, 256) + 256;        // delta [B, h w] float32 behind an aligned start
}

// replaces igs/models/unimatch/attention.py:8-16 (K = 1) and 45-104 with the mask of igs/models/unimatch/utils.py:84-108
extern "C" int igs_window_attn_fwd(void* stream, int B, int h, int w, int K, int shift, int D, int dtype, const void* q, long long qs_b,
                                   long long qs_t, const void* k, long long ks_b, long long ks_t, const void* v, long long vs_b, long long vs_t,
                                   float scale, void* out, long long os_b, long long os_t, float* lse)
{
    const char* fn = "igs_window_attn_fwd";
    if (const char* e = wattn_size_error(B, h, w, K, shift, D, dtype)) return fail_in(fn, e);
    if (const char* e = wattn_view_error(dtype, qs_b, qs_t)) return fail_in(fn, e);
    if (const char* e = wattn_view_error(dtype, ks_b, ks_t)) return fail_in(fn, e);
    if (const char* e = wattn_view_error(dtype, vs_b, vs_t)) return fail_in(fn, e);
    if (const char* e = wattn_view_error(dtype, os_b, os_t)) return fail_in(fn, e);
    if (const char* e = wattn_out_error(B, (long long)h * w, os_b, os_t)) return fail_in(fn, e);
    if (!(fabsf(scale) <= 3.0e38f)) return fail_in(fn, "scale must be finite");
    if (B == 0) return 0;
    if (!q || !k || !v || !out) return fail_in(fn, "NULL pointer");
    if (!ptr_aligned(q, 16) || !ptr_aligned(k, 16) || !ptr_aligned(v, 16) || !ptr_aligned(out, 16)) return fail_in(fn, "base pointers must be 16-byte aligned");
    WattnArgs a = {};
    a.g = wattn_geom(h, w, K, shift);
    a.scale = scale; a.c = (float)((double)scale * 1.4426950408889634);
    a.q = wattn_view(q, qs_b, qs_t); a.k = wattn_view(k, ks_b, ks_t); a.v = wattn_view(v, vs_b, vs_t); a.o = wattn_view(out, os_b, os_t);
    a.lse = lse;
    const dim3 grid((unsigned)((size_t)B * K * K * a.g.tiles)), blk(WATTN_THREADS);
    if (dtype == IGS_DTYPE_F16) hipLaunchKernelGGL(wattn_fwd_kernel<_Float16>, grid, blk, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(wattn_fwd_kernel<float>, grid, blk, 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError(), "window attention forward launch");
    return 0;
}

// the backward of the same lines (autograd through them in the reference)
extern "C" int igs_window_attn_bwd(void* stream, int B, int h, int w, int K, int shift, int D, int dtype, const void* q, long long qs_b,
                                   long long qs_t, const void* k, long long ks_b, long long ks_t, const void* v, long long vs_b, long long vs_t,
                                   const void* out, long long os_b, long long os_t, const float* lse, const void* dout, long long gs_b,
                                   long long gs_t, float scale, void* dq, long long dqs_b, long long dqs_t, void* dk, long long dks_b,
                                   long long dks_t, void* dv, long long dvs_b, long long dvs_t, void* scratch)
{
    const char* fn = "igs_window_attn_bwd";
    const long long L = (long long)h * w;
    if (const char* e = wattn_size_error(B, h, w, K, shift, D, dtype)) return fail_in(fn, e);
    if (const char* e = wattn_view_error(dtype, qs_b, qs_t)) return fail_in(fn, e);
    if (const char* e = wattn_view_error(dtype, ks_b, ks_t)) return fail_in(fn, e);
    if (const char* e = wattn_view_error(dtype, vs_b, vs_t)) return fail_in(fn, e);
    if (const char* e = wattn_view_error(dtype, os_b, os_t)) return fail_in(fn, e);
    if (const char* e = wattn_view_error(dtype, gs_b, gs_t)) return fail_in(fn, e);
    if (dq) if (const char* e = wattn_view_error(dtype, dqs_b, dqs_t)) return fail_in(fn, e);
    if (dk) if (const char* e = wattn_view_error(dtype, dks_b, dks_t)) return fail_in(fn, e);
    if (dv) if (const char* e = wattn_view_error(dtype, dvs_b, dvs_t)) return fail_in(fn, e);
    if (dq) if (const char* e = wattn_out_error(B, L, dqs_b, dqs_t)) return fail_in(fn, e);
    if (dk) if (const char* e = wattn_out_error(B, L, dks_b, dks_t)) return fail_in(fn, e);
    if (dv) if (const char* e = wattn_out_error(B, L, dvs_b, dvs_t)) return fail_in(fn, e);
    if (!(fabsf(scale) <= 3.0e38f)) return fail_in(fn, "scale must be finite");
    if (B == 0 || (!dq && !dk && !dv)) return 0;
    if (!q || !k || !v || !out || !lse || !dout || !scratch) return fail_in(fn, "NULL pointer");
    if (!ptr_aligned(q, 16) || !ptr_aligned(k, 16) || !ptr_aligned(v, 16) || !ptr_aligned(out, 16) || !ptr_aligned(dout, 16) || !ptr_aligned(dq, 16) ||
        !ptr_aligned(dk, 16) || !ptr_aligned(dv, 16))
        return fail_in(fn, "base pointers must be 16-byte aligned");
    WattnArgs a = {};
    a.g = wattn_geom(h, w, K, shift);
    a.scale = scale; a.c = (float)((double)scale * 1.4426950408889634);
    a.q = wattn_view(q, qs_b, qs_t); a.k = wattn_view(k, ks_b, ks_t); a.v = wattn_view(v, vs_b, vs_t);
    a.o = wattn_view(out, os_b, os_t); a.go = wattn_view(dout, gs_b, gs_t);
    a.dq = wattn_view(dq, dqs_b, dqs_t); a.dk = wattn_view(dk, dks_b, dks_t); a.dv = wattn_view(dv, dvs_b, dvs_t);
    a.lse = (float*)lse;
    a.delta = (float*)align_ptr((const char*)scratch);
    hipStream_t s = (hipStream_t)stream;
    const dim3 blk(WATTN_THREADS);
    const size_t rows = (size_t)B * L, owners = (size_t)B * K * K * a.g.tiles;
    const dim3 gd((unsigned)((rows + WATTN_THREADS - 1) / WATTN_THREADS));
    if (dtype == IGS_DTYPE_F16) hipLaunchKernelGGL(wattn_delta_kernel<_Float16>, gd, blk, 0, s, a, B);
    else hipLaunchKernelGGL(wattn_delta_kernel<float>, gd, blk, 0, s, a, B);
    HIP_TRY(hipGetLastError(), "window attention delta launch");
    if (dk || dv) {
        if (dtype == IGS_DTYPE_F16) hipLaunchKernelGGL(wattn_dkdv_kernel<_Float16>, dim3((unsigned)(owners * (2 / WattnDkdv<_Float16>::BLOCKS))), blk, 0, s, a);
        else hipLaunchKernelGGL(wattn_dkdv_kernel<float>, dim3((unsigned)(owners * (2 / WattnDkdv<float>::BLOCKS))), blk, 0, s, a);
        HIP_TRY(hipGetLastError(), "window attention d K / d V launch");
    }
    if (dq) {
        if (dtype == IGS_DTYPE_F16) hipLaunchKernelGGL(wattn_dq_kernel<_Float16>, dim3((unsigned)owners), blk, 0, s, a);
        else hipLaunchKernelGGL(wattn_dq_kernel<float>, dim3((unsigned)owners), blk, 0, s, a);
        HIP_TRY(hipGetLastError(), "window attention d Q launch");
    }
    return 0;
}
