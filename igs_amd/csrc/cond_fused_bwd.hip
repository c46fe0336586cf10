// cond_fused_bwd.hip -- the backward of IGS.condition3D's fused forward (cond_fused.hip): d x, d W1, d b1, d W2, d b2 and the LayerNorm's
// d weight / d bias from x, rays, depth, the packs and d out, with the forward recomputed.  include/igs_rast.h states the contract
// (igs_condition3d_bwd), DESIGN.md section 15.8 the budget and the figures.
//
// The pixels are walked in chunks of CB_CHUNK_GROUPS 32-pixel groups (a group is 32 consecutive pixels of ONE image, the last group of an
// image masked per lane, as in the forward); a chunk's rows live in `slots`, float32 [CB_SLOTS][rows][128], row = 32 (group - first group)
// + lane & 31.  A lane without a pixel writes +0 to every slot it would have written, so it adds +0 to every sum below.  Per chunk:
//   condition3d_bwd_pixels_kernel   cond, z1 = W1 cond + b1, h = SiLU(z1), scale = W2[C:] h + b2[C:] as the forward computes them (the
//                                   shift half of W2 is not needed: d shift = g), the LayerNorm statistics as the forward, then
//                                   d scale = g n, d n = g (1 + scale), d xh = d n weight and d x, which leaves in x's dtype.  It stores
//                                   cond, z1, d shift, d scale, d n xh and d n where a parameter gradient needs them.
//   condition3d_bwd_hidden_kernel   d h = W2[:C]^T d shift + W2[C:]^T d scale (the transposed pack resident in LDS), d z1 = d h silu'(z1).
//                                   Only where d W1 / d b1 is wanted.
//   condition3d_bwd_wgrad_kernel    a wave owns (slice of CB_SLICE_ROWS rows, product, input tile): d W1 = sum d z1 (x) cond, d W2[:C] =
//                                   sum d shift (x) h, d W2[C:] = sum d scale (x) h, and as column sums d b1, d b2, d weight, d bias.  Its
//                                   float32 accumulators start from the slice's partial of the chunk before: a slice's partial is the sum
//                                   over its rows in row order, chunk after chunk (mlp.hip's scheme; at most CB_SLICES partials).
// and at the end condition3d_bwd_reduce_kernel adds the slices' partials in slice order.  No float atomics; the order of every sum
// depends on the sizes only.
//
// Why separate launches and not one kernel that restages per phase: the float32 W2 pack and its transpose are 128 KB each, so one kernel
// would restage 64 + 128 KB per trip of 256 pixels behind barriers that every wave has to reach; as launches each workgroup stages its
// weights once per chunk and a wave without a group skips its trip.  The price is the chunk's slots (3.5 KB per row) going through L2.
#include "mlp_common.h"
#include "cond_common.h"
#include "host_api.h"

#define CB_WAVES 8
#define CB_THREADS (64 * CB_WAVES)
#define CB_CHUNK_GROUPS (IGS_COND_BWD_CHUNK_ROWS / 32)
#define CB_SLICE_ROWS 256
#define CB_SLICES (IGS_COND_BWD_CHUNK_ROWS / CB_SLICE_ROWS)
#define CB_WG_WAVES 4
#define CB_WG_THREADS (64 * CB_WG_WAVES)
#define CB_SLOTS 7
enum { CB_S_COND = 0, CB_S_Z1, CB_S_DZ1, CB_S_DSHIFT, CB_S_DSCALE, CB_S_DNXH, CB_S_DN };
#define CB_MAX_UNITS 12

// one (product, input tile) pair of the weight-gradient kernel: d W[O][I] += dz^T in, column sums of dz where sum_b
struct CondBwdUnit {
    unsigned char in_slot, dz_slot, kt, ot, act, want_w, want_b, pad;
    int O, I;
    uint32_t woff, boff;                   // in a slice's partial
};

struct CondBwdArgs {
    int C, hidden, H, W, Hd, Wd;
    float sy, sx, eps;
    uint32_t gpi, grp0, ngroups;           // 32-pixel groups per image; the chunk is groups grp0 .. grp0 + ngroups - 1
    int chunk, rows;                       // rows = 32 ngroups
    const void* x;
    long long xs_n, xs_c;
    const float* rays;
    const float* depth;
    const void* w;
    const void* wt;                        // W2^T: [ht][2 ct] tiles, inputs = shift channels (padded to 32 ct), then scale channels
    const float* b;
    const float* nw;
    const float* nb;
    const float* g;                        // d out [N, C, H, W] contiguous
    void* dx;                              // [N, C, H, W] contiguous in x's dtype, or NULL
    int want_mlp, want_ln;
    float* slots;
    long long slot_stride;
    float* part;
    uint32_t pstride;
};
// the weight-gradient kernel's work (kept out of CondBwdArgs: the other kernels would hold the table in scalar registers)
struct CondBwdUnits {
    int npairs, units, chunk, rows;
    float* slots;
    long long slot_stride;
    float* part;
    uint32_t pstride;
    CondBwdUnit unit[CB_MAX_UNITS];
};

__device__ __forceinline__ void cb_store(float* p, float v) { *p = v; }
__device__ __forceinline__ void cb_store(_Float16* p, float v) { *p = (_Float16)v; }          // the one rounding of d x

template <typename T, typename TX>
__global__ __launch_bounds__(CB_THREADS, 2) void condition3d_bwd_pixels_kernel(const CondBwdArgs a)
{
    constexpr bool HALF = AttnCfg<T>::HALF;
    constexpr int KT1 = HALF ? 2 : 1;
    __shared__ __attribute__((aligned(16))) T w1[4 * KT1 * MLP_TILE];
    __shared__ __attribute__((aligned(16))) T w2[16 * MLP_TILE];         // the scale half of W2
    __shared__ __attribute__((aligned(16))) float bl[2 * 128];           // b1, b2[C:]
    __shared__ __attribute__((aligned(16))) float wd[128];               // float32: W1[:, 32], the depth column
    __shared__ float nw[128], nb[128];

    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int HT = mlp_tiles(a.hidden), CT = mlp_tiles(a.C), HW = a.H * a.W;
    const T* wg = (const T*)a.w;

    // ---- the weights, once per workgroup (the forward's staging without the shift half) ----
    {
        constexpr uint32_t TC = MLP_TILE * sizeof(T) / 16;
        const attn_f4* src = (const attn_f4*)wg;
        for (uint32_t i = threadIdx.x; i < (uint32_t)(HT * KT1) * TC; i += CB_THREADS) {
            const uint32_t tile = i / TC, j = i - tile * TC;
            ((attn_f4*)w1)[i] = src[(HALF ? tile : 2 * tile) * TC + j];
        }
        const attn_f4* src2 = src + (size_t)(2 * HT + CT * HT) * TC;
        for (uint32_t i = threadIdx.x; i < (uint32_t)(CT * HT) * TC; i += CB_THREADS) ((attn_f4*)w2)[i] = src2[i];
        if (threadIdx.x < 128) {
            const int c = threadIdx.x;
            bl[c] = a.b[c];
            bl[128 + c] = a.b[256 + c];
            nw[c] = c < a.C ? a.nw[c] : 0.f;
            nb[c] = c < a.C ? a.nb[c] : 0.f;
            if (!HALF) wd[c] = (c >> 5) < HT ? (float)wg[(size_t)(2 * (c >> 5) + 1) * MLP_TILE + 4 * (c & 31)] : 0.f;
        }
    }
    wg_barrier();

    const uint32_t trips = (a.ngroups + CB_WAVES - 1) / CB_WAVES;
    for (uint32_t trip = blockIdx.x; trip < trips; trip += gridDim.x) {
        const uint32_t lg = trip * CB_WAVES + wave;
        if (lg >= a.ngroups) continue;                           // (uniform over the wave; no barrier below)
        const uint32_t grp = a.grp0 + lg;
        const uint32_t n = grp / a.gpi, p = (grp - n * a.gpi) * 32 + r;
        const bool live = p < (uint32_t)HW;
        float* row = a.slots + (size_t)(lg * 32 + r) * 128;      // this lane's row of slot 0
        float* slot = row + 4 * h;                               // ... and its 4-channel groups in the accumulators' order

        float cv[COND_CH];
#pragma unroll
        for (int i = 0; i < COND_CH; i++) cv[i] = 0.f;
        if (live) {
            const uint32_t yo = p / (uint32_t)a.W, xo = p - yo * (uint32_t)a.W;
            cond_pixel(a.rays + ((size_t)n * HW + p) * 6, a.depth + (size_t)n * a.Hd * a.Wd, yo, xo, a.Hd, a.Wd, a.sy, a.sx, cv);
        }
        if (a.want_mlp) {                                        // cond, columns 0 .. 63 of its slot (zeros behind column 32)
            float* cs = row + CB_S_COND * a.slot_stride;
#pragma unroll
            for (int q = 0; q < 4; q++)
                *(float4*)(cs + 16 * h + 4 * q) = h ? make_float4(cv[16 + 4 * q], cv[17 + 4 * q], cv[18 + 4 * q], cv[19 + 4 * q])
                                                    : make_float4(cv[4 * q], cv[4 * q + 1], cv[4 * q + 2], cv[4 * q + 3]);
#pragma unroll
            for (int q = 0; q < 4; q++)
                *(float4*)(cs + 32 + 16 * h + 4 * q) = make_float4((q == 0 && h == 0) ? cv[32] : 0.f, 0.f, 0.f, 0.f);
        }

        // ---- layer 1, the forward's statements: z1 = W1 cond + b1, h = SiLU(z1) ----
        MlpIn<T> cin, in;
#pragma unroll
        for (int e = 0; e < 16; e++) cin.set(0, e, h ? cv[attn_row(e, 1)] : cv[attn_row(e, 0)]);
        if (HALF) {
#pragma unroll
            for (int e = 0; e < 16; e++) cin.set(1, e, (e == 0 && h == 0) ? cv[32] : 0.f);
        }
#pragma unroll
        for (int t = 0; t < 4; t++) {
            if (t < HT) {
                attn_acc o;
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    const attn_f4 bv = *(const attn_f4*)(bl + 32 * t + 8 * g + 4 * h);
                    o[4 * g] = bv[0]; o[4 * g + 1] = bv[1]; o[4 * g + 2] = bv[2]; o[4 * g + 3] = bv[3];
                }
#pragma unroll
                for (int k = 0; k < KT1; k++) o = mlp_mm(w1 + (t * KT1 + k) * MLP_TILE, lane, cin, k, o);
                if (!HALF) {
#pragma unroll
                    for (int g = 0; g < 4; g++) {
                        const attn_f4 dv = *(const attn_f4*)(wd + 32 * t + 8 * g + 4 * h);
#pragma unroll
                        for (int j = 0; j < 4; j++) o[4 * g + j] = fmaf(dv[j], cv[32], o[4 * g + j]);
                    }
                }
                if (a.want_mlp) {
                    float* zs = slot + CB_S_Z1 * a.slot_stride + 32 * t;
#pragma unroll
                    for (int g = 0; g < 4; g++)
                        *(float4*)(zs + 8 * g) = live ? make_float4(o[4 * g], o[4 * g + 1], o[4 * g + 2], o[4 * g + 3]) : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
                for (int i = 0; i < 16; i++) in.set(t, i, mlp_silu(o[i]));
            } else {
#pragma unroll
                for (int i = 0; i < 16; i++) in.set(t, i, 0.f);  // (defined on every path: no value of the trip before stays live)
            }
        }

        // ---- scale = W2[C:] h + b2[C:], every channel tile, before x is loaded.  It waits in the lane's own row of the d scale slot (the
        // lane that wrote it reads it back below and overwrites it with d scale): held in registers beside x and d xh it would not fit ----
#pragma unroll
        for (int t = 0; t < 4; t++) {
            if (t < CT) {
                attn_acc sc;
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    const attn_f4 b1 = *(const attn_f4*)(bl + 128 + 32 * t + 8 * g + 4 * h);
#pragma unroll
                    for (int j = 0; j < 4; j++) sc[4 * g + j] = b1[j];
                }
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (k < HT) sc = mlp_mm(w2 + (t * HT + k) * MLP_TILE, lane, in, k, sc);
                float* ss = slot + CB_S_DSCALE * a.slot_stride + 32 * t;
#pragma unroll
                for (int g = 0; g < 4; g++) *(float4*)(ss + 8 * g) = make_float4(sc[4 * g], sc[4 * g + 1], sc[4 * g + 2], sc[4 * g + 3]);
            }
        }
        asm volatile("" ::: "memory");                           // (the values go through memory, not through registers)

        // ---- x in the forward's order, and the forward's statistics ----
        __builtin_amdgcn_sched_barrier(0);                       // (no load of x rises above the products: their registers are still taken)
        const char* xn = (const char*)a.x + (size_t)n * (size_t)a.xs_n * sizeof(TX);
        const size_t xcb = (size_t)a.xs_c * sizeof(TX);
        const uint32_t xo = (uint32_t)((4 * h * (uint32_t)a.xs_c + (live ? p : 0u)) * (uint32_t)sizeof(TX));
        typename CfRaw<TX>::type xr[4][16];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            if (t < CT && 32 * t + 32 <= a.C) {
#pragma unroll
                for (int i = 0; i < 16; i++) xr[t][i] = cf_load((const TX*)(xn + (32 * t + attn_row(i, 0)) * xcb + xo));
            } else {
#pragma unroll
                for (int i = 0; i < 16; i++) {
                    xr[t][i] = 0;
                    if (32 * t + attn_row(i, h) < a.C) xr[t][i] = cf_load((const TX*)(xn + (32 * t + attn_row(i, 0)) * xcb + xo));
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        float xv[4][16];
#pragma unroll
        for (int t = 0; t < 4; t++) {
#pragma unroll
            for (int i = 0; i < 16; i++) xv[t][i] = cf_widen(xr[t][i]);
        }
        float s = 0.f;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            if (t < CT) {
#pragma unroll
                for (int i = 0; i < 16; i++) s += xv[t][i];
            }
        }
        s += __shfl_xor(s, 32, 64);
        const float m = s / (float)a.C;
        float v = 0.f;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            if (t < CT) {
#pragma unroll
                for (int i = 0; i < 16; i++) {
                    const float d = 32 * t + attn_row(i, h) < a.C ? xv[t][i] - m : 0.f;
                    v = fmaf(d, d, v);
                }
            }
        }
        v += __shfl_xor(v, 32, 64);
        const float rs = 1.f / sqrtf(v / (float)a.C + a.eps);

        // ---- per channel tile: g, d scale = g n, d n = g (1 + scale), d xh = d n weight; dxv holds d xh ----
        const char* gn = (const char*)a.g + (size_t)n * (size_t)a.C * HW * sizeof(float);
        const size_t ocb = (size_t)HW * sizeof(float);
        const uint32_t oo = (uint32_t)((4 * h * (uint32_t)HW + (live ? p : 0u)) * (uint32_t)sizeof(float));      // (H W <= 2^24)
        const float* nwh = nw + 4 * h;
        const float* nbh = nb + 4 * h;
        float s1 = 0.f, s2 = 0.f, dxv[4][16];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            if (t < CT) {
                float* ts = slot + 32 * t;
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    float dsh[4], dsc[4], dnx[4], dnn[4];
                    const float4 scv = *(const float4*)(ts + CB_S_DSCALE * a.slot_stride + 8 * g);
                    const float sc[4] = {scv.x, scv.y, scv.z, scv.w};
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const int i = 4 * g + j, c0 = 32 * t + attn_row(i, 0);
                        const bool ok = live && 32 * t + attn_row(i, h) < a.C;
                        const float gv = ok ? *(const float*)(gn + (size_t)c0 * ocb + oo) : 0.f;
                        const float xh = ok ? (xv[t][i] - m) * rs : 0.f;
                        const float nrm = fmaf(xh, nwh[c0], nbh[c0]);
                        const float dn = gv * (1.f + sc[j]);
                        const float dxh = dn * nwh[c0];
                        dsh[j] = gv;
                        dsc[j] = ok ? gv * nrm : 0.f;
                        dnx[j] = ok ? dn * xh : 0.f;
                        dnn[j] = ok ? dn : 0.f;
                        s1 += ok ? dxh : 0.f;
                        s2 += ok ? dxh * xh : 0.f;
                        dxv[t][i] = dxh;
                    }
                    if (a.want_mlp) {
                        *(float4*)(ts + CB_S_DSHIFT * a.slot_stride + 8 * g) = make_float4(dsh[0], dsh[1], dsh[2], dsh[3]);
                        *(float4*)(ts + CB_S_DSCALE * a.slot_stride + 8 * g) = make_float4(dsc[0], dsc[1], dsc[2], dsc[3]);
                    }
                    if (a.want_ln) {
                        *(float4*)(ts + CB_S_DNXH * a.slot_stride + 8 * g) = make_float4(dnx[0], dnx[1], dnx[2], dnx[3]);
                        *(float4*)(ts + CB_S_DN * a.slot_stride + 8 * g) = make_float4(dnn[0], dnn[1], dnn[2], dnn[3]);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }

        // ---- d x = r (d xh - mean(d xh) - xh mean(d xh xh)) ----
        if (a.dx) {                                              // (uniform)
            s1 += __shfl_xor(s1, 32, 64);
            s2 += __shfl_xor(s2, 32, 64);
            const float m1 = s1 / (float)a.C, m2 = s2 / (float)a.C;
            char* dn = (char*)a.dx + (size_t)n * (size_t)a.C * HW * sizeof(TX);
            const size_t dcb = (size_t)HW * sizeof(TX);
            const uint32_t dof = (uint32_t)((4 * h * (uint32_t)HW + (live ? p : 0u)) * (uint32_t)sizeof(TX));
#pragma unroll
            for (int t = 0; t < 4; t++) {
                if (t < CT) {
#pragma unroll
                    for (int i = 0; i < 16; i++) {
                        if (live && 32 * t + attn_row(i, h) < a.C) {     // x once more (its registers went to d xh): the same xh bits
                            const float xh = (cf_widen(cf_load((const TX*)(xn + (32 * t + attn_row(i, 0)) * xcb + xo))) - m) * rs;
                            cb_store((TX*)(dn + (size_t)(32 * t + attn_row(i, 0)) * dcb + dof), rs * fmaf(-xh, m2, dxv[t][i] - m1));
                        }
                    }
                }
            }
        }
    }
}

// d h = W2^T [d shift ; d scale], d z1 = d h silu'(z1), over the chunk's rows
template <typename T>
__global__ __launch_bounds__(CB_THREADS, 2) void condition3d_bwd_hidden_kernel(const CondBwdArgs a)
{
    __shared__ __attribute__((aligned(16))) T wt[32 * MLP_TILE];
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int HT = mlp_tiles(a.hidden), CT = mlp_tiles(a.C);
    {
        const uint32_t chunks = (uint32_t)(2 * CT * HT) * (MLP_TILE * (uint32_t)sizeof(T) / 16);
        for (uint32_t i = threadIdx.x; i < chunks; i += CB_THREADS) ((attn_f4*)wt)[i] = ((const attn_f4*)a.wt)[i];
    }
    wg_barrier();

    const uint32_t trips = (a.ngroups + CB_WAVES - 1) / CB_WAVES;
    for (uint32_t trip = blockIdx.x; trip < trips; trip += gridDim.x) {
        const uint32_t lg = trip * CB_WAVES + wave;
        if (lg >= a.ngroups) continue;                           // (uniform over the wave; no barrier below)
        float* slot = a.slots + (size_t)(lg * 32 + r) * 128 + 4 * h;
        attn_acc dh[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
#pragma unroll
            for (int i = 0; i < 16; i++) dh[t][i] = 0.f;
        }
#pragma unroll
        for (int kk = 0; kk < 8; kk++) {
            const int half = kk >> 2, k = kk & 3;
            if (k < CT) {
                MlpIn<T> in;                                     // (tile 0 only: one k tile of the operand at a time)
                const float* ds = slot + (half ? CB_S_DSCALE : CB_S_DSHIFT) * a.slot_stride + 32 * k;
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    const float4 f = *(const float4*)(ds + 8 * g);
                    in.set(0, 4 * g, f.x); in.set(0, 4 * g + 1, f.y); in.set(0, 4 * g + 2, f.z); in.set(0, 4 * g + 3, f.w);
                }
#pragma unroll
                for (int t = 0; t < 4; t++)
                    if (t < HT) dh[t] = mlp_mm(wt + (t * 2 * CT + half * CT + k) * MLP_TILE, lane, in, 0, dh[t]);
            }
        }
#pragma unroll
        for (int t = 0; t < 4; t++) {
            if (t < HT) {
                const float* zs = slot + CB_S_Z1 * a.slot_stride + 32 * t;
                float* dz = slot + CB_S_DZ1 * a.slot_stride + 32 * t;
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    const float4 z = *(const float4*)(zs + 8 * g);
                    *(float4*)(dz + 8 * g) = make_float4(dh[t][4 * g] * mlp_silu_grad(z.x), dh[t][4 * g + 1] * mlp_silu_grad(z.y),
                                                         dh[t][4 * g + 2] * mlp_silu_grad(z.z), dh[t][4 * g + 3] * mlp_silu_grad(z.w));
                }
            }
        }
    }
}

// mlp_bwd_wgrad_kernel's scheme over the unit table
template <typename T>
__global__ __launch_bounds__(CB_WG_THREADS) void condition3d_bwd_wgrad_kernel(const CondBwdUnits a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int u = blockIdx.x * CB_WG_WAVES + wave;
    if (u >= a.units) return;                                    // (no barrier in this kernel)
    const int slice = u / a.npairs;
    const CondBwdUnit q = a.unit[u % a.npairs];
    const int lr0 = slice * CB_SLICE_ROWS, lr1 = min(lr0 + CB_SLICE_ROWS, a.rows);
    if (lr0 >= lr1) return;                                      // (the last chunk's empty slices keep the partial they have)
    const int ot = q.ot, kt = q.kt, O = q.O, I = q.I;
    const float* hs = a.slots + (size_t)q.in_slot * a.slot_stride + 32 * kt + r;
    const float* ds = a.slots + (size_t)q.dz_slot * a.slot_stride + r;
    float* pw = a.part + (size_t)slice * a.pstride + q.woff;
    float* pb = a.part + (size_t)slice * a.pstride + q.boff;
    const int col = 32 * kt + r;

    attn_acc acc[4];
    float bs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 4; t++) {
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int o = 32 * t + attn_row(i, h);
            acc[t][i] = (a.chunk > 0 && q.want_w && t < ot && o < O && col < I) ? pw[(size_t)o * I + col] : 0.f;
        }
    }
    for (int n0 = lr0; n0 < lr1; n0 += 16) {
        float bv[8], av[4][8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int n = n0 + mlp_wgrad_row<T>(j, h);
            const bool ok = n < lr1;
            float v = (ok && q.want_w) ? hs[(size_t)n * 128] : 0.f;
            if (q.act) v = mlp_silu(v);
            bv[j] = v;
#pragma unroll
            for (int t = 0; t < 4; t++) av[t][j] = (ok && t < ot) ? ds[(size_t)n * 128 + 32 * t] : 0.f;
        }
#pragma unroll
        for (int t = 0; t < 4; t++) {
            if (t < ot) {
#pragma unroll
                for (int j = 0; j < 8; j++) bs[t] += av[t][j];
                if (q.want_w) acc[t] = mlp_wgrad_mm(T(0), av[t], bv, acc[t]);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 4; t++) {
        if (t < ot) {
            if (q.want_w) {
#pragma unroll
                for (int i = 0; i < 16; i++) {
                    const int o = 32 * t + attn_row(i, h);
                    if (o < O && col < I) pw[(size_t)o * I + col] = acc[t][i];
                }
            }
            if (q.want_b) {                                      // (uniform over the wave)
                const float s = bs[t] + __shfl_xor(bs[t], 32, 64);
                const int o = 32 * t + r;
                if (h == 0 && o < O) pb[o] = (a.chunk > 0 ? pb[o] : 0.f) + s;
            }
        }
    }
}

// the six gradients, each where wanted: the slices' partials added in slice order
struct CondBwdOut { uint32_t end[6]; float* ptr[6]; };
__global__ __launch_bounds__(256) void condition3d_bwd_reduce_kernel(const float* __restrict__ part, uint32_t pstride, int slices, const CondBwdOut o)
{
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= o.end[5]) return;
    int k = 0;
#pragma unroll
    for (int i = 0; i < 5; i++) k += j >= o.end[i] ? 1 : 0;
    float* dst = nullptr;
    uint32_t start = 0;
#pragma unroll
    for (int i = 0; i < 6; i++)
        if (i == k) { dst = o.ptr[i]; start = i ? o.end[i ? i - 1 : 0] : 0; }
    if (!dst) return;
    float s = 0.f;
    for (int z = 0; z < slices; z++) s += part[(size_t)z * pstride + j];
    dst[j - start] = s;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the entry points (the contract is in include/igs_rast.h)
// ---------------------------------------------------------------------------------------------------------------------------------
// a slice's partial: d W1 [hidden, 33], d W2 [2 C, hidden], d b1 [hidden], d b2 [2 C], d weight [C], d bias [C]
struct CondBwdSizes { uint32_t end[6], pstride; long long rows, slot_rows; int slices; };
static CondBwdSizes cond_bwd_sizes(int N, int C, int hidden, int H, int W)
{
    CondBwdSizes z = {};
    const uint32_t len[6] = {(uint32_t)hidden * COND_CH, 2u * C * hidden, (uint32_t)hidden, 2u * C, (uint32_t)C, (uint32_t)C};
    uint32_t e = 0;
    for (int i = 0; i < 6; i++) { e += len[i]; z.end[i] = e; }
    z.pstride = (e + 3u) & ~3u;
    z.rows = (((long long)H * W + 31) / 32) * 32 * N;
    z.slot_rows = z.rows < IGS_COND_BWD_CHUNK_ROWS ? z.rows : IGS_COND_BWD_CHUNK_ROWS;
    z.slices = (int)((z.slot_rows + CB_SLICE_ROWS - 1) / CB_SLICE_ROWS);
    return z;
}
static long long cond_bwd_scratch(const CondBwdSizes& z)
{
    return ((long long)CB_SLOTS * z.slot_rows * 128 + (long long)z.slices * z.pstride) * (long long)sizeof(float);
}
static const char* cond_bwd_size_error(int N, int C, int hidden, int H, int W)
{
    if (N < 0 || N > IGS_COND_MAX_PIXELS) return "N out of range";
    if (C < 1 || C > IGS_COND_MLP_MAX_WIDTH) return "C out of range (1..IGS_COND_MLP_MAX_WIDTH)";
    if (hidden < 1 || hidden > IGS_COND_MLP_MAX_WIDTH) return "hidden out of range (1..IGS_COND_MLP_MAX_WIDTH)";
    if (H < 1 || H > IGS_COND_MAX_HW) return "H out of range (1..IGS_COND_MAX_HW)";
    if (W < 1 || W > IGS_COND_MAX_HW) return "W out of range (1..IGS_COND_MAX_HW)";
    if ((long long)N * H * W > IGS_COND_MAX_PIXELS) return "N * H * W out of range (IGS_COND_MAX_PIXELS)";
    return nullptr;
}

extern "C" long long igs_condition3d_bwd_scratch_bytes(int N, int C, int hidden, int H, int W)
{
    if (cond_bwd_size_error(N, C, hidden, H, W)) return -1;
    return cond_bwd_scratch(cond_bwd_sizes(N, C, hidden, H, W));
}

extern "C" int igs_condition3d_bwd(void* stream, int N, int C, int hidden, int H, int W, int Hd, int Wd, int x_dtype, const void* x, long long xs_n,
                                   long long xs_c, long long xs_h, long long xs_w, const float* rays, const float* depth, int mlp_dtype,
                                   const void* wpack, const void* wpack_t, const float* bpack, const float* weight, const float* bias, float eps,
                                   const float* gout, void* scratch, long long scratch_bytes, void* dx, float* dW1, float* db1, float* dW2,
                                   float* db2, float* dweight, float* dbias)
{
    const char* fn = "igs_condition3d_bwd";
    if (const char* w = cond_bwd_size_error(N, C, hidden, H, W)) return fail_in(fn, w);
    if (Hd < 1 || Hd > IGS_COND_MAX_HW) return fail_in(fn, "Hd out of range (1..IGS_COND_MAX_HW)");
    if (Wd < 1 || Wd > IGS_COND_MAX_HW) return fail_in(fn, "Wd out of range (1..IGS_COND_MAX_HW)");
    if (!dtype_ok(x_dtype) || !dtype_ok(mlp_dtype)) return fail_in(fn, "unknown dtype code");
    if (const char* w = plane_stride_error(C, H, W, xs_n, xs_c, xs_h, xs_w)) return fail_in(fn, w);
    if (xs_c > IGS_COND_FUSED_MAX_STRIDE) return fail_in(fn, "xs_c above IGS_COND_FUSED_MAX_STRIDE");
    if (!(eps >= 0.f)) return fail_in(fn, "eps must be >= 0");
    if (N == 0) return 0;
    if (!x || !rays || !depth || !wpack || !wpack_t || !bpack || !weight || !bias || !gout || !scratch) return fail_in(fn, "NULL pointer");
    if (!ptr_aligned(x, dtype_bytes(x_dtype)) || !ptr_aligned(dx, dtype_bytes(x_dtype)) || !ptr_aligned(rays, 4) || !ptr_aligned(depth, 4) ||
        !ptr_aligned(bpack, 4) || !ptr_aligned(weight, 4) || !ptr_aligned(bias, 4) || !ptr_aligned(gout, 4) || !ptr_aligned(dW1, 4) ||
        !ptr_aligned(db1, 4) || !ptr_aligned(dW2, 4) || !ptr_aligned(db2, 4) || !ptr_aligned(dweight, 4) || !ptr_aligned(dbias, 4))
        return fail_in(fn, "a pointer is not aligned to its element size");
    if (!ptr_aligned(wpack, 16) || !ptr_aligned(wpack_t, 16)) return fail_in(fn, "wpack and wpack_t must be aligned to 16 bytes");
    if (!ptr_aligned(scratch, 16)) return fail_in(fn, "scratch must be aligned to 16 bytes");
    const CondBwdSizes z = cond_bwd_sizes(N, C, hidden, H, W);
    if (scratch_bytes < cond_bwd_scratch(z)) return fail_in(fn, "scratch is smaller than igs_condition3d_bwd_scratch_bytes");
    const bool want_w1 = dW1 || db1, want_w2 = dW2 || db2, want_ln = dweight || dbias;
    if (!dx && !want_w1 && !want_w2 && !want_ln) return 0;

    CondBwdArgs a = {};
    a.C = C; a.hidden = hidden; a.H = H; a.W = W; a.Hd = Hd; a.Wd = Wd;
    a.sy = (float)Hd / (float)H; a.sx = (float)Wd / (float)W; a.eps = eps;
    a.gpi = (uint32_t)(((long long)H * W + 31) / 32);
    a.x = x; a.xs_n = xs_n; a.xs_c = xs_c; a.rays = rays; a.depth = depth; a.w = wpack; a.wt = wpack_t; a.b = bpack; a.nw = weight; a.nb = bias;
    a.g = gout; a.dx = dx;
    a.want_mlp = want_w1 || want_w2; a.want_ln = want_ln;
    a.slots = (float*)scratch;
    a.slot_stride = z.slot_rows * 128;
    a.part = a.slots + (long long)CB_SLOTS * a.slot_stride;
    a.pstride = z.pstride;
    const int ht = mlp_tiles(hidden), ct = mlp_tiles(C);
    CondBwdUnits wu = {};
    wu.slots = a.slots; wu.slot_stride = a.slot_stride; wu.part = a.part; wu.pstride = a.pstride;
    auto add = [&](int in_slot, int dz_slot, int kt, int ot, int act, int want_w, int want_b, int O, int I, uint32_t woff, uint32_t boff) {
        CondBwdUnit& q = wu.unit[wu.npairs++];
        q.in_slot = (unsigned char)in_slot; q.dz_slot = (unsigned char)dz_slot; q.kt = (unsigned char)kt; q.ot = (unsigned char)ot;
        q.act = (unsigned char)act; q.want_w = (unsigned char)want_w; q.want_b = (unsigned char)want_b; q.O = O; q.I = I; q.woff = woff; q.boff = boff;
    };
    if (want_w1)
        for (int k = 0; k < 2; k++) add(CB_S_COND, CB_S_DZ1, k, ht, 0, 1, k == 0, hidden, COND_CH, 0, z.end[1]);
    if (want_w2)
        for (int k = 0; k < ht; k++) {
            add(CB_S_Z1, CB_S_DSHIFT, k, ct, 1, 1, k == 0, C, hidden, z.end[0], z.end[2]);
            add(CB_S_Z1, CB_S_DSCALE, k, ct, 1, 1, k == 0, C, hidden, z.end[0] + (uint32_t)(C * hidden), z.end[2] + (uint32_t)C);
        }
    if (want_ln) {
        add(CB_S_DNXH, CB_S_DNXH, 0, ct, 0, 0, 1, C, 1, 0, z.end[3]);
        add(CB_S_DN, CB_S_DN, 0, ct, 0, 0, 1, C, 1, 0, z.end[4]);
    }
    wu.units = z.slices * wu.npairs;

    hipStream_t s = (hipStream_t)stream;
    const bool half = mlp_dtype == IGS_DTYPE_F16, xhalf = x_dtype == IGS_DTYPE_F16;
    const uint32_t groups = a.gpi * (uint32_t)N, cus = (uint32_t)mlp_cus();
    const dim3 block(CB_THREADS);
    for (uint32_t g0 = 0; g0 < groups; g0 += CB_CHUNK_GROUPS) {
        a.grp0 = g0;
        a.ngroups = groups - g0 < CB_CHUNK_GROUPS ? groups - g0 : CB_CHUNK_GROUPS;
        a.rows = (int)(a.ngroups * 32);
        a.chunk = (int)(g0 / CB_CHUNK_GROUPS);
        const uint32_t trips = (a.ngroups + CB_WAVES - 1) / CB_WAVES;
        const dim3 grid(trips < cus ? trips : cus);
        if (xhalf) {
            if (half) hipLaunchKernelGGL((condition3d_bwd_pixels_kernel<_Float16, _Float16>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((condition3d_bwd_pixels_kernel<float, _Float16>), grid, block, 0, s, a);
        } else {
            if (half) hipLaunchKernelGGL((condition3d_bwd_pixels_kernel<_Float16, float>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((condition3d_bwd_pixels_kernel<float, float>), grid, block, 0, s, a);
        }
        if (want_w1) {
            if (half) hipLaunchKernelGGL((condition3d_bwd_hidden_kernel<_Float16>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((condition3d_bwd_hidden_kernel<float>), grid, block, 0, s, a);
        }
        if (wu.units > 0) {
            wu.chunk = a.chunk; wu.rows = a.rows;
            const dim3 wgrid((unsigned)((wu.units + CB_WG_WAVES - 1) / CB_WG_WAVES)), wblock(CB_WG_THREADS);
            if (half) hipLaunchKernelGGL((condition3d_bwd_wgrad_kernel<_Float16>), wgrid, wblock, 0, s, wu);
            else hipLaunchKernelGGL((condition3d_bwd_wgrad_kernel<float>), wgrid, wblock, 0, s, wu);
        }
    }
    if (wu.units > 0) {
        CondBwdOut o = {};
        for (int i = 0; i < 6; i++) o.end[i] = z.end[i];
        o.ptr[0] = dW1; o.ptr[1] = dW2; o.ptr[2] = db1; o.ptr[3] = db2; o.ptr[4] = dweight; o.ptr[5] = dbias;
        hipLaunchKernelGGL(condition3d_bwd_reduce_kernel, dim3((z.end[5] + 255) / 256), dim3(256), 0, s, a.part, z.pstride, z.slices, o);
    }
    HIP_TRY(hipGetLastError(), "condition3d bwd launch");
    return 0;
}
