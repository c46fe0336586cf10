// attn.hip -- fused attention softmax(scale Q K^T) V for the anchor transformer (GridEncoder.conv, a Transformer1D of 4 blocks, 8 heads of
// 64 channels over 8192 anchors; igs/models/transformers.py:673-907), forward and backward, on the gfx950 matrix cores.  include/igs_rast.h
// states the contract, DESIGN.md section 16 the budget and the figures.
//
// One product shape everywhere: a 32 x 32 float32 accumulator tile of a wave (v_mfma_f32_32x32x16_f16 for half inputs, the exact
// v_mfma_f32_32x32x2_f32 for float inputs: no half value exists in the float instances).  Lane (r, h) = (lane & 31, lane >> 5) of a tile X
// holds column r and the rows row(i, h) = (i & 3) + 8 (i >> 2) + 4 h in registers i = 0..15.  Two kinds of product are built on it:
//   rows x rows   X[i][j] = sum_d A[i][d] B[j][d]: lane (r, h) brings row r of A and row r of B (64 channels, the half h of every k-step);
//   tile x image  a product that sums over X's ROW index takes X straight from the accumulator registers as one operand (rounded to half once
//                 in the half instances); the other operand is read from an LDS image of 64 rows by column: float images as they are
//                 ([row][68]), half images transposed ([d][72], the rows inside a group of 16 permuted to the accumulator's register order,
//                 so that a lane's 8 k-values are 16 consecutive bytes).
//   (1) attn_fwd_kernel   a workgroup owns 128 queries (4 waves x 32), walks the keys 64 at a time: S^T = K Q^T (rows key, column query), so a
//                         query's running max / sum / rescale are per-lane scalars (two lanes per query, one __shfl_xor), and O^T += V^T P^T
//                         takes P^T from the registers.  exp2 with scale log2(e) folded into the scores.
//   (2) attn_delta_kernel delta = rowsum(d O * O), float32.
//   (3) attn_dkdv_kernel  a workgroup owns 128 keys, walks the queries: S = Q K^T and d P = d O V^T (rows query, column key), P recomputed from
//                         lse, d V += P^T d O and d K += d S^T Q accumulate in the owner's registers.
//   (4) attn_dq_kernel    a workgroup owns 128 queries, walks the keys: S^T and d P^T again, d Q += d S K in the owner's registers.
// No float atomics: every output element has one owner that adds in a fixed order, so two runs agree bit for bit.  Every global -> LDS tile
// is loaded into registers one tile ahead of its use and written after the barrier.
#include "common.h"
#include "host_api.h"
#include "attn_common.h"
#include <math.h>

#define ATTN_THREADS 256
#define ATTN_D 64
#define ATTN_ROWS 64                    // rows of one LDS image
#define ATTN_OWN 128                    // queries (keys) owned by a workgroup: 32 per wave

struct AttnView { void* p; long long sb, sh, sa; };          // [B, H, A, 64] with element strides; the stride on d is 1
struct AttnArgs {
    int H, Aq, Ak, tiles;
    float c, scale;                                           // c = scale * log2(e)
    AttnView q, k, v, o, go, dq, dk, dv;
    float* lse;
    float* delta;
};

template <typename T> __device__ __forceinline__ T* attn_at(const AttnView& t, int b, int h) { return (T*)t.p + (long long)b * t.sb + (long long)h * t.sh; }

// 64 rows of a [.., A, 64] operand on their way into LDS: 16-byte pieces in registers (rows at or behind `nrows` are zeros), then either
// image.  where(row) of the transposed image: the accumulator's register order inside every group of 16 rows.
template <typename T> struct AttnStage {
    typedef AttnCfg<T> C;
    typename C::vec v[C::NCH];
    __device__ __forceinline__ void load(const T* base, long long sa, int row0, int nrows)
    {
#pragma unroll
        for (int u = 0; u < C::NCH; u++) {
            const int c = threadIdx.x + ATTN_THREADS * u, row = row0 + c / C::CPR, col = (c % C::CPR) * C::EPC;
            typename C::vec z = {};
            v[u] = row < nrows ? *(const typename C::vec*)(base + (long long)row * sa + col) : z;
        }
    }
    __device__ __forceinline__ void write_rows(T* img) const
    {
#pragma unroll
        for (int u = 0; u < C::NCH; u++) {
            const int c = threadIdx.x + ATTN_THREADS * u, row = c / C::CPR, col = (c % C::CPR) * C::EPC;
            *(typename C::vec*)(img + row * C::LS + col) = v[u];
        }
    }
    __device__ __forceinline__ void write_transposed(T* img) const
    {
#pragma unroll
        for (int u = 0; u < C::NCH; u++) {
            const int c = threadIdx.x + ATTN_THREADS * u, row = c / C::CPR, col = (c % C::CPR) * C::EPC;
            const int where = (row & ~15) | (((row >> 2) & 1) << 3) | (((row >> 3) & 1) << 2) | (row & 3);
#pragma unroll
            for (int e = 0; e < C::EPC; e++) img[(col + e) * C::LS + where] = v[u][e];
        }
    }
    // the image that attn_mm_image reads
    __device__ __forceinline__ void write_columns(T* img) const { if constexpr (C::HALF != 0) write_transposed(img); else write_rows(img); }
};

// rows c = c0 + row(i, h) of a [.., A, 64] output from a Z tile pair (channel on the lane), scaled; rows at or behind `nrows` stay unwritten
template <typename T>
__device__ __forceinline__ void attn_store_z(T* base, long long sa, int c0, int nrows, int r, int h, const attn_acc& z0, const attn_acc& z1, float f)
{
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int c = c0 + attn_row(i, 0) + 4 * h;
        if (c < nrows) {
            T* p = base + (long long)c * sa + r;
            p[0] = (T)(z0[i] * f);
            p[32] = (T)(z1[i] * f);
        }
    }
}

__device__ __forceinline__ void attn_decode(const AttnArgs& a, int& b, int& hd, int& tile)
{
    const unsigned idx = blockIdx.x;                          // the head is the fastest index: with 8 heads a head's keys stay in one L2
    hd = idx % (unsigned)a.H;
    const unsigned rest = idx / (unsigned)a.H;
    tile = rest % (unsigned)a.tiles;
    b = rest / (unsigned)a.tiles;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (1) forward
// ---------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(ATTN_THREADS)
attn_fwd_kernel(AttnArgs a)
{
    typedef AttnCfg<T> C;
    __shared__ __attribute__((aligned(16))) T kimg[ATTN_ROWS * C::LS];
    __shared__ __attribute__((aligned(16))) T vimg[ATTN_ROWS * C::LS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    int b, hd, tile;
    attn_decode(a, b, hd, tile);
    const int q0 = tile * ATTN_OWN + 32 * w, qrow = q0 + r;
    const bool live = q0 < a.Aq;                              // (wave-uniform; a dead wave still stages and meets the barriers)
    AttnRow<T> qf;
    attn_load_row(qf, attn_at<const T>(a.q, b, hd) + (long long)min(qrow, a.Aq - 1) * a.q.sa, h);
    const T* kb = attn_at<const T>(a.k, b, hd);
    const T* vb = attn_at<const T>(a.v, b, hd);
    AttnStage<T> sk, sv;
    sk.load(kb, a.k.sa, 0, a.Ak);
    sv.load(vb, a.v.sa, 0, a.Ak);
    attn_acc o0 = {}, o1 = {};
    float m = -INFINITY, l = 0.f;                             // the running max of the log2-domain scores; this lane's share of the sum
    for (int k0 = 0; k0 < a.Ak; k0 += ATTN_ROWS) {
        wg_barrier();
        sk.write_rows(kimg);
        sv.write_columns(vimg);
        wg_barrier();
        if (k0 + ATTN_ROWS < a.Ak) {
            sk.load(kb, a.k.sa, k0 + ATTN_ROWS, a.Ak);
            sv.load(vb, a.v.sa, k0 + ATTN_ROWS, a.Ak);
        }
        if (!live) continue;
#pragma unroll
        for (int sub = 0; sub < 2; sub++) {
            const int ro = 32 * sub, kk = k0 + ro;
            if (kk >= a.Ak) break;                            // (uniform)
            AttnRow<T> kf;
            attn_load_row(kf, kimg + (ro + r) * C::LS, h);
            attn_acc s = {};
            s = attn_mm_rows(kf, qf, s);                      // rows: key, column: query
            const bool ragged = kk + 32 > a.Ak;
            float mx = m;
#pragma unroll
            for (int i = 0; i < 16; i++) {
                float t = s[i] * a.c;
                if (ragged && kk + attn_row(i, 0) + 4 * h >= a.Ak) t = -INFINITY;
                s[i] = t;
                mx = fmaxf(mx, t);
            }
            mx = fmaxf(mx, __shfl_xor(mx, 32));               // finite: key kk itself is real
            if (__any(mx > m)) {                              // (wave-uniform) some query's max grew; otherwise every factor is exactly 1
                const float alpha = attn_exp2(m - mx);        // (0 at the first tile)
                m = mx;
                l *= alpha;
                o0 *= alpha;
                o1 *= alpha;
            }
            float ls = 0.f;                                   // the 32 keys' own sums, then one addition each: the chain over all
#pragma unroll                                                // keys is Ak / 32 additions long, not Ak
            for (int i = 0; i < 16; i++) {
                const float p = attn_exp2(s[i] - mx);
                s[i] = p;
                ls += p;
            }
            l += ls;
            // O^T[d][query] += sum_key V[key][d] P^T[key][query]
            if constexpr (C::HALF != 0) {
                attn_mm_image<false>(s, vimg, ro, r, h, o0, o1);
            } else {                                          // float32: the fma chain of the matrix unit restarts with every 32 keys
                attn_acc t0 = {}, t1 = {};
                attn_mm_image<false>(s, vimg, ro, r, h, t0, t1);
                o0 += t0;
                o1 += t1;
            }
        }
    }
    if (!live || qrow >= a.Aq) return;
    const float lt = l + __shfl_xor(l, 32);
    T* op = attn_at<T>(a.o, b, hd) + (long long)qrow * a.o.sa;
#pragma unroll
    for (int g = 0; g < 4; g++) {
        const int d = 8 * g + 4 * h;
        if constexpr (C::HALF != 0) {
            h4_t x0, x1;
#pragma unroll
            for (int e = 0; e < 4; e++) { x0[e] = (_Float16)(o0[4 * g + e] / lt); x1[e] = (_Float16)(o1[4 * g + e] / lt); }
            *(h4_t*)(op + d) = x0;
            *(h4_t*)(op + 32 + d) = x1;
        } else {
            attn_f4 x0, x1;
#pragma unroll
            for (int e = 0; e < 4; e++) { x0[e] = o0[4 * g + e] / lt; x1[e] = o1[4 * g + e] / lt; }
            *(attn_f4*)(op + d) = x0;
            *(attn_f4*)(op + 32 + d) = x1;
        }
    }
    if (a.lse && h == 0) a.lse[((size_t)b * a.H + hd) * a.Aq + qrow] = (m + log2f(lt)) * 0.6931471805599453f;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (2) delta = rowsum(d O * O): one thread per row, channels in order
// ---------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(ATTN_THREADS)
attn_delta_kernel(AttnArgs a, int B)
{
    typedef AttnCfg<T> C;
    const size_t idx = (size_t)blockIdx.x * ATTN_THREADS + threadIdx.x, n = (size_t)B * a.H * a.Aq;
    if (idx >= n) return;
    const int qrow = idx % a.Aq, hd = (idx / a.Aq) % a.H, b = idx / ((size_t)a.Aq * a.H);
    const T* o = attn_at<const T>(a.o, b, hd) + (long long)qrow * a.o.sa;
    const T* g = attn_at<const T>(a.go, b, hd) + (long long)qrow * a.go.sa;
    float s = 0.f;
    for (int d = 0; d < ATTN_D; d += C::EPC) {
        const typename C::vec x = *(const typename C::vec*)(o + d), y = *(const typename C::vec*)(g + d);
#pragma unroll
        for (int e = 0; e < C::EPC; e++) s = fmaf((float)x[e], (float)y[e], s);
    }
    a.delta[idx] = s;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (3) d K and d V: the workgroup owns 128 keys and walks the queries
// ---------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(ATTN_THREADS)
attn_dkdv_kernel(AttnArgs a)
{
    typedef AttnCfg<T> C;
    __shared__ __attribute__((aligned(16))) T qimg[ATTN_ROWS * C::LS];
    __shared__ __attribute__((aligned(16))) T gimg[ATTN_ROWS * C::LS];
    __shared__ __attribute__((aligned(16))) T qcol[C::HALF ? ATTN_ROWS * C::LS : 8];     // the transposed images (half only: the float
    __shared__ __attribute__((aligned(16))) T gcol[C::HALF ? ATTN_ROWS * C::LS : 8];     // images are read both ways)
    __shared__ __attribute__((aligned(16))) float lse2[ATTN_ROWS];
    __shared__ __attribute__((aligned(16))) float dlt[ATTN_ROWS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    int b, hd, tile;
    attn_decode(a, b, hd, tile);
    const int kbase = tile * ATTN_OWN + 32 * w;
    const bool live = kbase < a.Ak;
    AttnRow<T> kf, vf;
    attn_load_row(kf, attn_at<const T>(a.k, b, hd) + (long long)min(kbase + r, a.Ak - 1) * a.k.sa, h);
    attn_load_row(vf, attn_at<const T>(a.v, b, hd) + (long long)min(kbase + r, a.Ak - 1) * a.v.sa, h);
    const T* qb = attn_at<const T>(a.q, b, hd);
    const T* gb = attn_at<const T>(a.go, b, hd);
    const float* lb = a.lse + ((size_t)b * a.H + hd) * a.Aq;
    const float* db = a.delta + ((size_t)b * a.H + hd) * a.Aq;
    AttnStage<T> sq, sg;
    float nl = 0.f, nd = 0.f;
    sq.load(qb, a.q.sa, 0, a.Aq);
    sg.load(gb, a.go.sa, 0, a.Aq);
    if (threadIdx.x < ATTN_ROWS) {                            // a row behind the last query: lse = +inf, so that its P is zero
        const int q = threadIdx.x;
        nl = q < a.Aq ? lb[q] * 1.4426950408889634f : INFINITY;
        nd = q < a.Aq ? db[q] : 0.f;
    }
    attn_acc dk0 = {}, dk1 = {}, dv0 = {}, dv1 = {};
    for (int q0 = 0; q0 < a.Aq; q0 += ATTN_ROWS) {
        wg_barrier();
        sq.write_rows(qimg);
        sg.write_rows(gimg);
        if constexpr (C::HALF != 0) { sq.write_transposed(qcol); sg.write_transposed(gcol); }
        if (threadIdx.x < ATTN_ROWS) { lse2[threadIdx.x] = nl; dlt[threadIdx.x] = nd; }
        wg_barrier();
        if (q0 + ATTN_ROWS < a.Aq) {
            sq.load(qb, a.q.sa, q0 + ATTN_ROWS, a.Aq);
            sg.load(gb, a.go.sa, q0 + ATTN_ROWS, a.Aq);
            if (threadIdx.x < ATTN_ROWS) {
                const int q = q0 + ATTN_ROWS + threadIdx.x;
                nl = q < a.Aq ? lb[q] * 1.4426950408889634f : INFINITY;
                nd = q < a.Aq ? db[q] : 0.f;
            }
        }
        if (!live) continue;
#pragma unroll
        for (int sub = 0; sub < 2; sub++) {
            const int ro = 32 * sub;
            if (q0 + ro >= a.Aq) break;                       // (uniform)
            AttnRow<T> qf, gf;
            attn_load_row(qf, qimg + (ro + r) * C::LS, h);
            attn_load_row(gf, gimg + (ro + r) * C::LS, h);
            attn_acc s = {}, dp = {};
            s = attn_mm_rows(qf, kf, s);                      // rows: query, column: key
            dp = attn_mm_rows(gf, vf, dp);
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const attn_f4 l4 = *(const attn_f4*)(lse2 + ro + 8 * g + 4 * h), d4 = *(const attn_f4*)(dlt + ro + 8 * g + 4 * h);
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const float p = attn_exp2(fmaf(s[4 * g + e], a.c, -l4[e]));
                    s[4 * g + e] = p;
                    dp[4 * g + e] = p * (dp[4 * g + e] - d4[e]);
                }
            }
            attn_mm_image<true>(s, C::HALF ? gcol : gimg, ro, r, h, dv0, dv1);      // d V[key][d] += sum_q P[q][key] d O[q][d]
            attn_mm_image<true>(dp, C::HALF ? qcol : qimg, ro, r, h, dk0, dk1);     // d K[key][d] += sum_q d S[q][key] Q[q][d]
        }
    }
    if (!live) return;
    if (a.dk.p) attn_store_z(attn_at<T>(a.dk, b, hd), a.dk.sa, kbase, a.Ak, r, h, dk0, dk1, a.scale);
    if (a.dv.p) attn_store_z(attn_at<T>(a.dv, b, hd), a.dv.sa, kbase, a.Ak, r, h, dv0, dv1, 1.f);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (4) d Q: the workgroup owns 128 queries and walks the keys
// ---------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(ATTN_THREADS)
attn_dq_kernel(AttnArgs a)
{
    typedef AttnCfg<T> C;
    __shared__ __attribute__((aligned(16))) T kimg[ATTN_ROWS * C::LS];
    __shared__ __attribute__((aligned(16))) T vimg[ATTN_ROWS * C::LS];
    __shared__ __attribute__((aligned(16))) T kcol[C::HALF ? ATTN_ROWS * C::LS : 8];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    int b, hd, tile;
    attn_decode(a, b, hd, tile);
    const int q0 = tile * ATTN_OWN + 32 * w, qrow = min(q0 + r, a.Aq - 1);
    const bool live = q0 < a.Aq;
    AttnRow<T> qf, gf;
    attn_load_row(qf, attn_at<const T>(a.q, b, hd) + (long long)qrow * a.q.sa, h);
    attn_load_row(gf, attn_at<const T>(a.go, b, hd) + (long long)qrow * a.go.sa, h);
    const float l2 = a.lse[((size_t)b * a.H + hd) * a.Aq + qrow] * 1.4426950408889634f;
    const float dl = a.delta[((size_t)b * a.H + hd) * a.Aq + qrow];
    const T* kb = attn_at<const T>(a.k, b, hd);
    const T* vb = attn_at<const T>(a.v, b, hd);
    AttnStage<T> sk, sv;
    sk.load(kb, a.k.sa, 0, a.Ak);
    sv.load(vb, a.v.sa, 0, a.Ak);
    attn_acc dq0 = {}, dq1 = {};
    for (int k0 = 0; k0 < a.Ak; k0 += ATTN_ROWS) {
        wg_barrier();
        sk.write_rows(kimg);
        sv.write_rows(vimg);
        if constexpr (C::HALF != 0) sk.write_transposed(kcol);
        wg_barrier();
        if (k0 + ATTN_ROWS < a.Ak) {
            sk.load(kb, a.k.sa, k0 + ATTN_ROWS, a.Ak);
            sv.load(vb, a.v.sa, k0 + ATTN_ROWS, a.Ak);
        }
        if (!live) continue;
#pragma unroll
        for (int sub = 0; sub < 2; sub++) {
            const int ro = 32 * sub, kk = k0 + ro;
            if (kk >= a.Ak) break;                            // (uniform)
            AttnRow<T> kf, vf;
            attn_load_row(kf, kimg + (ro + r) * C::LS, h);
            attn_load_row(vf, vimg + (ro + r) * C::LS, h);
            attn_acc s = {}, dp = {};
            s = attn_mm_rows(kf, qf, s);                      // rows: key, column: query
            dp = attn_mm_rows(vf, gf, dp);
            const bool ragged = kk + 32 > a.Ak;
#pragma unroll
            for (int i = 0; i < 16; i++) {
                float p = attn_exp2(fmaf(s[i], a.c, -l2));
                if (ragged && kk + attn_row(i, 0) + 4 * h >= a.Ak) p = 0.f;
                s[i] = p * (dp[i] - dl);
            }
            attn_mm_image<true>(s, C::HALF ? kcol : kimg, ro, r, h, dq0, dq1);      // d Q[q][d] += sum_key d S^T[key][q] K[key][d]
        }
    }
    if (!live) return;
    attn_store_z(attn_at<T>(a.dq, b, hd), a.dq.sa, q0, a.Aq, r, h, dq0, dq1, a.scale);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------------------
static const char* attn_size_error(int B, int H, int Aq, int Ak, int D, int dtype)
{
    if (D != ATTN_D) return "D must be 64 (the only head size provided)";
    if (!dtype_ok(dtype)) return "unknown dtype code (IGS_DTYPE_F32 or IGS_DTYPE_F16)";
    if (B < 0 || B > IGS_ATTN_MAX_BATCH) return "B out of range (0..IGS_ATTN_MAX_BATCH)";
    if (H < 1 || H > IGS_ATTN_MAX_HEADS) return "H out of range (1..IGS_ATTN_MAX_HEADS)";
    if (Aq < 1 || Aq > IGS_ATTN_MAX_TOKENS) return "Aq out of range (1..IGS_ATTN_MAX_TOKENS)";
    if (Ak < 1 || Ak > IGS_ATTN_MAX_TOKENS) return "Ak out of range (1..IGS_ATTN_MAX_TOKENS)";
    const long long amax = Aq > Ak ? Aq : Ak;
    if ((long long)B * H * ((amax + ATTN_OWN - 1) / ATTN_OWN) > 0x7fffffffLL) return "B * H * A out of range";
    return nullptr;
}
static const char* attn_view_error(int dtype, long long sb, long long sh, long long sa)
{
    const long long es = dtype == IGS_DTYPE_F16 ? 2 : 4;
    if (sb < 0 || sh < 0 || sa < 0) return "negative stride";
    if ((sb * es) % 16 || (sh * es) % 16 || (sa * es) % 16) return "the b / h / a strides must be multiples of 16 bytes";
    return nullptr;
}
// an output view: rows must not alias one another (every element has one owner that writes it)
static const char* attn_out_error(int B, int H, int A, long long sb, long long sh, long long sa)
{
    if ((A > 1 && sa < ATTN_D) || (H > 1 && sh < ATTN_D) || (B > 1 && sb < ATTN_D)) return "output strides overlap (a stride below D on a dimension longer than 1)";
    return nullptr;
}
static AttnView attn_view(const void* p, long long sb, long long sh, long long sa) { AttnView t; t.p = (void*)p; t.sb = sb; t.sh = sh; t.sa = sa; return t; }

extern "C" size_t igs_attn_bwd_scratch_bytes(int B, int H, int Aq, int Ak, int D, int dtype)
{
    if (attn_size_error(B, H, Aq, Ak, D, dtype)) return 0;
    return align_up((size_t)B * H * Aq * 4, 256) + 256;       // delta [B, H, Aq] float32 behind an aligned start
}

extern "C" int igs_attn_fwd(void* stream, int B, int H, int Aq, int Ak, int D, int dtype, const void* q, long long qs_b, long long qs_h,
                            long long qs_a, const void* k, long long ks_b, long long ks_h, long long ks_a, const void* v, long long vs_b,
                            long long vs_h, long long vs_a, float scale, void* out, long long os_b, long long os_h, long long os_a, float* lse)
{
    const char* fn = "igs_attn_fwd";
    if (const char* w = attn_size_error(B, H, Aq, Ak, D, dtype)) return fail_in(fn, w);
    if (const char* w = attn_view_error(dtype, qs_b, qs_h, qs_a)) return fail_in(fn, w);
    if (const char* w = attn_view_error(dtype, ks_b, ks_h, ks_a)) return fail_in(fn, w);
    if (const char* w = attn_view_error(dtype, vs_b, vs_h, vs_a)) return fail_in(fn, w);
    if (const char* w = attn_view_error(dtype, os_b, os_h, os_a)) return fail_in(fn, w);
    if (const char* w = attn_out_error(B, H, Aq, os_b, os_h, os_a)) return fail_in(fn, w);
    if (!(fabsf(scale) <= 3.0e38f)) return fail_in(fn, "scale must be finite");
    if (B == 0) return 0;
    if (!q || !k || !v || !out) return fail_in(fn, "NULL pointer");
    if (!ptr_aligned(q, 16) || !ptr_aligned(k, 16) || !ptr_aligned(v, 16) || !ptr_aligned(out, 16)) return fail_in(fn, "base pointers must be 16-byte aligned");
    AttnArgs a = {};
    a.H = H; a.Aq = Aq; a.Ak = Ak; a.tiles = (Aq + ATTN_OWN - 1) / ATTN_OWN;
    a.scale = scale; a.c = (float)((double)scale * 1.4426950408889634);
    a.q = attn_view(q, qs_b, qs_h, qs_a); a.k = attn_view(k, ks_b, ks_h, ks_a); a.v = attn_view(v, vs_b, vs_h, vs_a);
    a.o = attn_view(out, os_b, os_h, os_a);
    a.lse = lse;
    const dim3 g((unsigned)((size_t)B * H * a.tiles)), blk(ATTN_THREADS);
    if (dtype == IGS_DTYPE_F16) hipLaunchKernelGGL(attn_fwd_kernel<_Float16>, g, blk, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(attn_fwd_kernel<float>, g, blk, 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError(), "attention forward launch");
    return 0;
}

extern "C" int igs_attn_bwd(void* stream, int B, int H, int Aq, int Ak, int D, int dtype, const void* q, long long qs_b, long long qs_h,
                            long long qs_a, const void* k, long long ks_b, long long ks_h, long long ks_a, const void* v, long long vs_b,
                            long long vs_h, long long vs_a, const void* out, long long os_b, long long os_h, long long os_a, const float* lse,
                            const void* dout, long long gs_b, long long gs_h, long long gs_a, float scale, void* dq, long long dqs_b,
                            long long dqs_h, long long dqs_a, void* dk, long long dks_b, long long dks_h, long long dks_a, void* dv,
                            long long dvs_b, long long dvs_h, long long dvs_a, void* scratch)
{
    const char* fn = "igs_attn_bwd";
    if (const char* w = attn_size_error(B, H, Aq, Ak, D, dtype)) return fail_in(fn, w);
    if (const char* w = attn_view_error(dtype, qs_b, qs_h, qs_a)) return fail_in(fn, w);
    if (const char* w = attn_view_error(dtype, ks_b, ks_h, ks_a)) return fail_in(fn, w);
    if (const char* w = attn_view_error(dtype, vs_b, vs_h, vs_a)) return fail_in(fn, w);
    if (const char* w = attn_view_error(dtype, os_b, os_h, os_a)) return fail_in(fn, w);
    if (const char* w = attn_view_error(dtype, gs_b, gs_h, gs_a)) return fail_in(fn, w);
    if (dq) if (const char* w = attn_view_error(dtype, dqs_b, dqs_h, dqs_a)) return fail_in(fn, w);
    if (dk) if (const char* w = attn_view_error(dtype, dks_b, dks_h, dks_a)) return fail_in(fn, w);
    if (dv) if (const char* w = attn_view_error(dtype, dvs_b, dvs_h, dvs_a)) return fail_in(fn, w);
    if (dq) if (const char* w = attn_out_error(B, H, Aq, dqs_b, dqs_h, dqs_a)) return fail_in(fn, w);
    if (dk) if (const char* w = attn_out_error(B, H, Ak, dks_b, dks_h, dks_a)) return fail_in(fn, w);
    if (dv) if (const char* w = attn_out_error(B, H, Ak, dvs_b, dvs_h, dvs_a)) return fail_in(fn, w);
    if (!(fabsf(scale) <= 3.0e38f)) return fail_in(fn, "scale must be finite");
    if (B == 0 || (!dq && !dk && !dv)) return 0;
    if (!q || !k || !v || !out || !lse || !dout || !scratch) return fail_in(fn, "NULL pointer");
    if (!ptr_aligned(q, 16) || !ptr_aligned(k, 16) || !ptr_aligned(v, 16) || !ptr_aligned(out, 16) || !ptr_aligned(dout, 16) || !ptr_aligned(dq, 16) ||
        !ptr_aligned(dk, 16) || !ptr_aligned(dv, 16))
        return fail_in(fn, "base pointers must be 16-byte aligned");
    AttnArgs a = {};
    a.H = H; a.Aq = Aq; a.Ak = Ak;
    a.scale = scale; a.c = (float)((double)scale * 1.4426950408889634);
    a.q = attn_view(q, qs_b, qs_h, qs_a); a.k = attn_view(k, ks_b, ks_h, ks_a); a.v = attn_view(v, vs_b, vs_h, vs_a);
    a.o = attn_view(out, os_b, os_h, os_a); a.go = attn_view(dout, gs_b, gs_h, gs_a);
    a.dq = attn_view(dq, dqs_b, dqs_h, dqs_a); a.dk = attn_view(dk, dks_b, dks_h, dks_a); a.dv = attn_view(dv, dvs_b, dvs_h, dvs_a);
    a.lse = (float*)lse;
    a.delta = (float*)align_ptr((const char*)scratch);
    hipStream_t s = (hipStream_t)stream;
    const dim3 blk(ATTN_THREADS);
    const size_t rows = (size_t)B * H * Aq;
    const dim3 gd((unsigned)((rows + ATTN_THREADS - 1) / ATTN_THREADS));
    if (dtype == IGS_DTYPE_F16) hipLaunchKernelGGL(attn_delta_kernel<_Float16>, gd, blk, 0, s, a, B);
    else hipLaunchKernelGGL(attn_delta_kernel<float>, gd, blk, 0, s, a, B);
    HIP_TRY(hipGetLastError(), "attention delta launch");
    if (dk || dv) {
        a.tiles = (Ak + ATTN_OWN - 1) / ATTN_OWN;
        const dim3 g((unsigned)((size_t)B * H * a.tiles));
        if (dtype == IGS_DTYPE_F16) hipLaunchKernelGGL(attn_dkdv_kernel<_Float16>, g, blk, 0, s, a);
        else hipLaunchKernelGGL(attn_dkdv_kernel<float>, g, blk, 0, s, a);
        HIP_TRY(hipGetLastError(), "attention d K / d V launch");
    }
    if (dq) {
        a.tiles = (Aq + ATTN_OWN - 1) / ATTN_OWN;
        const dim3 g((unsigned)((size_t)B * H * a.tiles));
        if (dtype == IGS_DTYPE_F16) hipLaunchKernelGGL(attn_dq_kernel<_Float16>, g, blk, 0, s, a);
        else hipLaunchKernelGGL(attn_dq_kernel<float>, g, blk, 0, s, a);
        HIP_TRY(hipGetLastError(), "attention d Q launch");
    }
    return 0;
}
