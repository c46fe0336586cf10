// cond_fused.hip -- IGS.condition3D's forward in one launch (igs/IGS.py:185-210 with ModLN :259-284; local_ray False): per pixel of
// x [N, C, H, W] the 33 conditioning channels (cond_common.h, the statements of ray_condition_kernel), ModLN's MLP
// Linear(33, hidden) . SiLU . Linear(hidden, 2 C) on the matrix cores, LayerNorm over the pixel's C channels and the modulation
//     out = ((x - mu) r weight + bias) (1 + scale) + shift.
// Neither the condition, the hidden activations nor the modulation reaches memory.  Forward only (cond_fused_bwd.hip is the backward,
// which recomputes this forward with the same statements).  include/igs_rast.h states the
// contract (igs_condition3d_fwd), DESIGN.md section 15.7 the budget and the figures.
//
// Tile layout: mlp.hip's.  One wave owns 32 consecutive pixels of ONE image (the last group of an image is masked per lane, so a group
// never straddles two images); the output channel is the accumulator's row (register i of lane half h is channel 32 t + attn_row(i, h)),
// the pixel its column (lane & 31).  Both lane halves compute their pixel's 33 condition values and keep the k-slots of their half, so
// layer 1's operand needs no lane movement; its accumulators, after SiLU, are layer 2's operand as they stand (float32) or after one
// rounding to half (float16).  Layer 2 is packed as two Linears, shift = W2[:C] and scale = W2[C:], so that tile t of either holds the
// channels 32 t .. 32 t + 31 of x whatever C is.  x is loaded in that same order (lanes across pixels: 128 contiguous bytes per channel
// and half-wave), a lane holds up to 64 of its pixel's channels; the mean and the centred sum of squares are in-lane sums plus one
// exchange with lane ^ 32 (a + b = b + a: both halves hold the same bits), and the result leaves as x came.  Nothing goes through LDS
// but the weights.
//
// LDS plan.  float16: W1 at K = 64 (the depth channel is k-slot 0 of the second tile) 16 KB + W2 64 KB.  float32: W2 alone is 128 KB, so
// the depth channel is taken out of the matrix product: W1's first 32 columns run on the matrix cores (K = 32, 16 KB) and column 32
// is a rank-one fma on the accumulators, h += W1[:, 32] depth -- still one float32 fma chain per output that starts from the bias.
// 16 + 128 KB of weights, 3 KB of biases, the depth column and the LayerNorm's affine: 147 KB of the 160 KB a compute unit has.
// One workgroup of 8 waves per compute unit stages the weights once and loops over trips of 256 pixels, 2 waves per SIMD at up to
// 256 registers; the only barrier is the one behind the staging, so a wave without a group simply skips its trip.
#include "mlp_common.h"
#include "cond_common.h"
#include "host_api.h"

#define CF_WAVES 8
#define CF_THREADS (64 * CF_WAVES)

struct CondFusedArgs {
    int C, hidden, H, W, Hd, Wd;
    float sy, sx, eps;
    uint32_t gpi, groups;                  // 32-pixel groups per image, and in all
    const void* x;
    long long xs_n, xs_c;
    const float* rays;
    const float* depth;
    const void* w;                         // W1 [ht][2], shift [ct][ht], scale [ct][ht] tiles
    const float* b;                        // [3][128]: b1, b2[:C], b2[C:]
    const float* nw;
    const float* nb;
    float* out;
};

template <typename T, typename TX>
__global__ __launch_bounds__(CF_THREADS, 2) void condition3d_fused_kernel(const CondFusedArgs a)
{
    constexpr bool HALF = AttnCfg<T>::HALF;
    constexpr int KT1 = HALF ? 2 : 1;                            // the k tiles of layer 1 that run on the matrix cores
    __shared__ __attribute__((aligned(16))) T w1[4 * KT1 * MLP_TILE];
    __shared__ __attribute__((aligned(16))) T w2[2 * 16 * MLP_TILE];
    __shared__ __attribute__((aligned(16))) float bl[3 * 128];
    __shared__ __attribute__((aligned(16))) float wd[128];       // float32: W1[:, 32], the depth column
    __shared__ float nw[128], nb[128];

    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int HT = mlp_tiles(a.hidden), CT = mlp_tiles(a.C), HW = a.H * a.W;
    const T* wg = (const T*)a.w;

    // ---- the weights, once per workgroup ----
    {
        constexpr uint32_t TC = MLP_TILE * sizeof(T) / 16;       // 16-byte chunks per tile
        const attn_f4* src = (const attn_f4*)wg;
        for (uint32_t i = threadIdx.x; i < (uint32_t)(HT * KT1) * TC; i += CF_THREADS) {
            const uint32_t tile = i / TC, j = i - tile * TC;
            ((attn_f4*)w1)[i] = src[(HALF ? tile : 2 * tile) * TC + j];
        }
        const attn_f4* src2 = src + (size_t)(2 * HT) * TC;
        for (uint32_t i = threadIdx.x; i < (uint32_t)(2 * CT * HT) * TC; i += CF_THREADS) ((attn_f4*)w2)[i] = src2[i];
        for (int i = threadIdx.x; i < 3 * 128; i += CF_THREADS) bl[i] = a.b[i];
        if (threadIdx.x < 128) {
            const int c = threadIdx.x;
            nw[c] = c < a.C ? a.nw[c] : 0.f;
            nb[c] = c < a.C ? a.nb[c] : 0.f;
            // element 0 of lane (r, 0), chunk 0 of tile (ot, 1) is W1[32 ot + r][32]
            if (!HALF) wd[c] = (c >> 5) < HT ? (float)wg[(size_t)(2 * (c >> 5) + 1) * MLP_TILE + 4 * (c & 31)] : 0.f;
        }
    }
    wg_barrier();

    const uint32_t trips = (a.groups + CF_WAVES - 1) / CF_WAVES;
    for (uint32_t trip = blockIdx.x; trip < trips; trip += gridDim.x) {
        const uint32_t grp = trip * CF_WAVES + wave;
        if (grp >= a.groups) continue;                           // (uniform over the wave; no barrier below)
        const uint32_t n = grp / a.gpi, p = (grp - n * a.gpi) * 32 + r;
        const bool live = p < (uint32_t)HW;

        float cv[COND_CH];
#pragma unroll
        for (int i = 0; i < COND_CH; i++) cv[i] = 0.f;
        if (live) {
            const uint32_t yo = p / (uint32_t)a.W, xo = p - yo * (uint32_t)a.W;
            cond_pixel(a.rays + ((size_t)n * HW + p) * 6, a.depth + (size_t)n * a.Hd * a.Wd, yo, xo, a.Hd, a.Wd, a.sy, a.sx, cv);
        }

        // ---- layer 1: h = SiLU(W1 cond + b1) ----
        MlpIn<T> cin, in;                                        // the condition as layer 1's operand; the hidden activations as layer 2's
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
#pragma unroll
                for (int i = 0; i < 16; i++) in.set(t, i, mlp_silu(o[i]));
            }
        }

        // x, behind layer 1 (before it, its 64 registers and layer 1's accumulators do not fit beside each other).  The address is a
        // uniform base (image, channel 32 t + attn_row(i, 0)) plus a 32-bit lane offset (the half's 4 channels and the pixel; xs_c is at
        // most IGS_COND_FUSED_MAX_STRIDE), so no load needs a 64-bit address of its own.  A lane without a pixel reads pixel 0 of its
        // image and stores nothing; a full tile needs no per-channel test.
        const char* xn = (const char*)a.x + (size_t)n * (size_t)a.xs_n * sizeof(TX);
        const size_t xcb = (size_t)a.xs_c * sizeof(TX);
        const uint32_t xo = (uint32_t)((4 * h * (uint32_t)a.xs_c + (live ? p : 0u)) * (uint32_t)sizeof(TX));
        typename CfRaw<TX>::type xr[4][16];                      // as loaded: the widening waits behind the last load, not behind each
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

        // ---- the pixel's statistics over its real channels: the mean, then the squares of the centred values ----
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

        // ---- layer 2 and the modulation, one channel tile at a time: shift and scale of channels 32 t .. 32 t + 31 ----
        char* on = (char*)a.out + (size_t)n * (size_t)a.C * HW * sizeof(float);
        const size_t ocb = (size_t)HW * sizeof(float);
        const uint32_t oo = (uint32_t)((4 * h * (uint32_t)HW + p) * (uint32_t)sizeof(float));      // (H W <= 2^24)
        const float* nwh = nw + 4 * h;
        const float* nbh = nb + 4 * h;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            if (t < CT) {
                attn_acc sh, sc;
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    const attn_f4 b0 = *(const attn_f4*)(bl + 128 + 32 * t + 8 * g + 4 * h), b1 = *(const attn_f4*)(bl + 256 + 32 * t + 8 * g + 4 * h);
#pragma unroll
                    for (int j = 0; j < 4; j++) { sh[4 * g + j] = b0[j]; sc[4 * g + j] = b1[j]; }
                }
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if (k < HT) {
                        sh = mlp_mm(w2 + (t * HT + k) * MLP_TILE, lane, in, k, sh);
                        sc = mlp_mm(w2 + ((CT + t) * HT + k) * MLP_TILE, lane, in, k, sc);
                    }
                }
                float y[16];
#pragma unroll
                for (int i = 0; i < 16; i++) {
                    const int c0 = 32 * t + attn_row(i, 0);
                    y[i] = fmaf(fmaf((xv[t][i] - m) * rs, nwh[c0], nbh[c0]), 1.f + sc[i], sh[i]);
                }
                if (32 * t + 32 <= a.C) {
                    if (live) {
#pragma unroll
                        for (int i = 0; i < 16; i++) *(float*)(on + (32 * t + attn_row(i, 0)) * ocb + oo) = y[i];
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 16; i++)
                        if (live && 32 * t + attn_row(i, h) < a.C) *(float*)(on + (32 * t + attn_row(i, 0)) * ocb + oo) = y[i];
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the entry points (the contract is in include/igs_rast.h)
// ---------------------------------------------------------------------------------------------------------------------------------
static bool cond_fused_widths_ok(int C, int hidden)
{
    return C >= 1 && C <= IGS_COND_MLP_MAX_WIDTH && hidden >= 1 && hidden <= IGS_COND_MLP_MAX_WIDTH;
}

extern "C" long long igs_condition3d_pack_elems(int C, int hidden, int mlp_dtype)
{
    if (!cond_fused_widths_ok(C, hidden) || !dtype_ok(mlp_dtype)) return -1;
    const long long ht = mlp_tiles(hidden), ct = mlp_tiles(C);
    return (2 * ht + 2 * ct * ht) * MLP_TILE;
}

extern "C" int igs_condition3d_fwd(void* stream, int N, int C, int hidden, int H, int W, int Hd, int Wd, int x_dtype, const void* x, long long xs_n,
                                   long long xs_c, long long xs_h, long long xs_w, const float* rays, const float* depth, int mlp_dtype,
                                   const void* wpack, const float* bpack, const float* weight, const float* bias, float eps, float* out)
{
    const char* fn = "igs_condition3d_fwd";
    if (N < 0 || N > IGS_COND_MAX_PIXELS) return fail_in(fn, "N out of range");
    if (C < 1 || C > IGS_COND_MLP_MAX_WIDTH) return fail_in(fn, "C out of range (1..IGS_COND_MLP_MAX_WIDTH)");
    if (hidden < 1 || hidden > IGS_COND_MLP_MAX_WIDTH) return fail_in(fn, "hidden out of range (1..IGS_COND_MLP_MAX_WIDTH)");
    if (H < 1 || H > IGS_COND_MAX_HW) return fail_in(fn, "H out of range (1..IGS_COND_MAX_HW)");
    if (W < 1 || W > IGS_COND_MAX_HW) return fail_in(fn, "W out of range (1..IGS_COND_MAX_HW)");
    if (Hd < 1 || Hd > IGS_COND_MAX_HW) return fail_in(fn, "Hd out of range (1..IGS_COND_MAX_HW)");
    if (Wd < 1 || Wd > IGS_COND_MAX_HW) return fail_in(fn, "Wd out of range (1..IGS_COND_MAX_HW)");
    if ((long long)N * H * W > IGS_COND_MAX_PIXELS) return fail_in(fn, "N * H * W out of range (IGS_COND_MAX_PIXELS)");
    if (!dtype_ok(x_dtype) || !dtype_ok(mlp_dtype)) return fail_in(fn, "unknown dtype code");
    if (const char* w = plane_stride_error(C, H, W, xs_n, xs_c, xs_h, xs_w)) return fail_in(fn, w);
    if (xs_c > IGS_COND_FUSED_MAX_STRIDE) return fail_in(fn, "xs_c above IGS_COND_FUSED_MAX_STRIDE");
    if (!(eps >= 0.f)) return fail_in(fn, "eps must be >= 0");
    if (N == 0) return 0;
    if (!x || !rays || !depth || !wpack || !bpack || !weight || !bias || !out) return fail_in(fn, "NULL pointer");
    if (!ptr_aligned(x, dtype_bytes(x_dtype)) || !ptr_aligned(rays, 4) || !ptr_aligned(depth, 4) || !ptr_aligned(bpack, 4) ||
        !ptr_aligned(weight, 4) || !ptr_aligned(bias, 4) || !ptr_aligned(out, 4))
        return fail_in(fn, "a pointer is not aligned to its element size");
    if (!ptr_aligned(wpack, 16)) return fail_in(fn, "wpack must be aligned to 16 bytes");

    CondFusedArgs a = {};
    a.C = C; a.hidden = hidden; a.H = H; a.W = W; a.Hd = Hd; a.Wd = Wd;
    a.sy = (float)Hd / (float)H; a.sx = (float)Wd / (float)W; a.eps = eps;
    a.gpi = (uint32_t)(((long long)H * W + 31) / 32);
    a.groups = a.gpi * (uint32_t)N;                              // (below 2^24 + N: N * H * W <= 2^24)
    a.x = x; a.xs_n = xs_n; a.xs_c = xs_c; a.rays = rays; a.depth = depth; a.w = wpack; a.b = bpack; a.nw = weight; a.nb = bias; a.out = out;
    const uint32_t trips = (a.groups + CF_WAVES - 1) / CF_WAVES, cus = (uint32_t)mlp_cus();
    const dim3 grid(trips < cus ? trips : cus), block(CF_THREADS);
    hipStream_t s = (hipStream_t)stream;
    const bool half = mlp_dtype == IGS_DTYPE_F16;
    if (x_dtype == IGS_DTYPE_F16) {
        if (half) hipLaunchKernelGGL((condition3d_fused_kernel<_Float16, _Float16>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((condition3d_fused_kernel<float, _Float16>), grid, block, 0, s, a);
    } else {
        if (half) hipLaunchKernelGGL((condition3d_fused_kernel<_Float16, float>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((condition3d_fused_kernel<float, float>), grid, block, 0, s, a);
    }
    HIP_TRY(hipGetLastError(), "condition3d fused launch");
    return 0;
}
