// upconv.hip -- the step between the motion transformer and condition3D (igs/IGS.py:132-134, up_sample True) in one launch:
//     up  = F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=False)            x [N, Cin, H, W]
//     out = Conv2d(Cin, Cout, 3, stride 1, padding 1)(up)                                     out [N, Cout, 2H, 2W]
// The upsampled map never reaches memory.  Forward only.  include/igs_rast.h states the contract (igs_upconv_fwd), DESIGN.md section 25
// the budget and the figures.  upconv_bwd.hip is the backward.
//
// A workgroup owns an 8 x 32 tile of one image's output and all its output channels.  Per 32-channel tile k of the input it
//   1. stages the 6 x 18 low-resolution pixels under the tile and its halo (indices clamped into the map, channels past Cin as zeros),
//   2. builds the 10 x 34 upsampled pixels in LDS in float32, zeros outside the 2H x 2W map (the convolution's padding), rounded once
//      to half in the float16 instance, each pixel's 32 channels in the order the B operand wants them (position 16 h + e holds
//      channel attn_row(e, h)), so a lane's operand for one tap is 16 consecutive elements of ONE pixel,
//   3. runs 9 taps x ceil(Cout / 32) tile products: mlp.hip's layout, the output channel is the accumulator's row, the pixel (lane & 31,
//      32 consecutive columns of one output row) its column.  The weights are packed (tap, output tile, input tile) and come from L2:
//      a lane's share of a tile, 16 bytes at a time, is loaded RING - 1 such vectors ahead of its product (across the taps and into the
//      next k, so the staging of k + 1 runs under loads already in flight) and the schedule is pinned there: with the load right in
//      front of its product, where the compiler puts it when left alone, every vector costs one L2 round trip.
// An output's sum is one chain: the bias, then k outermost, the tap, the tile's channels.  A float32 wave owns one output row of the tile
// (8 waves); a float16 wave owns two (4 waves), so that a weight tile it has read feeds twice the matrix work.  Two barriers per k, both
// on the workgroup's straight path.  No atomics; every output element is stored by exactly one lane.
#include "upconv_common.h"
#include "host_api.h"

struct UpconvArgs {
    int Cin, Cout, H, W;
    uint32_t tx, ty;                       // tiles per output row and column
    const void* x;
    long long xs_n, xs_c;
    const void* w;                         // [9][ot][kt] tiles
    const float* b;                        // [128]
    void* out;
};

template <typename T, typename TX, int OT>
__global__ __launch_bounds__(64 * UcCfg<T>::WAVES, UcCfg<T>::PER_SIMD) void upconv_kernel(const UpconvArgs a)
{
    constexpr int ROWS = UcCfg<T>::ROWS, THREADS = 64 * UcCfg<T>::WAVES, PS = UcCfg<T>::PS, NV = UcCfg<T>::NV, RING = UcCfg<T>::RING;
    constexpr int EPC = AttnCfg<T>::EPC, STEPS = 9 * OT * NV;    // a step: one vector of tile (tap * OT + t)
    typedef typename AttnCfg<T>::vec wvec;
    static_assert(STEPS % RING == 0 && RING - 1 <= STEPS, "the ring's slots must come round with the k step");
    __shared__ float lo[32 * UC_LCS];
    __shared__ __attribute__((aligned(16))) T up[UC_UH * UC_UW * PS];

    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int KT = mlp_tiles(a.Cin), OH = 2 * a.H, OW = 2 * a.W;
    const uint32_t bx = blockIdx.x % a.tx, byn = blockIdx.x / a.tx, by = byn % a.ty, n = byn / a.ty;
    const int Y0 = (int)by * UC_TY, X0 = (int)bx * UC_TX;        // (both even)
    const int m0 = Y0 / 2 - 1, n0 = X0 / 2 - 1;                  // the patch's first low-resolution row and column (-1 at the map's edge)

    attn_acc acc[ROWS][OT];
#pragma unroll
    for (int t = 0; t < OT; t++) {
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const attn_f4 bv = *(const attn_f4*)(a.b + 32 * t + 8 * g + 4 * h);
#pragma unroll
            for (int j = 0; j < ROWS; j++) { acc[j][t][4 * g] = bv[0]; acc[j][t][4 * g + 1] = bv[1]; acc[j][t][4 * g + 2] = bv[2]; acc[j][t][4 * g + 3] = bv[3]; }
        }
    }

    // vector q % NV of tile q / NV = tap * OT + t, input tile k: a uniform address plus the lane's 32-bit byte offset
    const char* wg = (const char*)a.w;
    const uint32_t wl = (uint32_t)lane * 16u;
#define UC_WVEC(k, q) (*(const wvec*)(wg + ((size_t)(((q) / NV) * KT + (k)) * (MLP_TILE * sizeof(T)) + ((q) % NV) * 1024) + wl))
    wvec ring[RING];
#pragma unroll
    for (int q = 0; q < RING - 1; q++) ring[q] = UC_WVEC(0, q);

    const TX* xn = (const TX*)a.x + (size_t)n * (size_t)a.xs_n;
    for (int k = 0; k < KT; k++) {
        // ---- 1. the low-resolution patch of channels 32 k .. 32 k + 31 (the barrier behind it also ends the reads of `up` for k - 1) ----
        for (int i = threadIdx.x; i < 32 * UC_LH * UC_LW; i += THREADS) {
            const int c = i / (UC_LH * UC_LW), p = i - c * (UC_LH * UC_LW), ly = p / UC_LW, lx = p - ly * UC_LW;
            const int gy = min(max(m0 + ly, 0), a.H - 1), gx = min(max(n0 + lx, 0), a.W - 1);
            float v = 0.f;
            if (32 * k + c < a.Cin) v = (float)xn[(size_t)(32 * k + c) * (size_t)a.xs_c + (size_t)(gy * a.W + gx)];
            lo[c * UC_LCS + p] = v;
        }
        wg_barrier();

        // ---- 2. the upsampled tile: thread -> (pixel, position in the pixel's operand order) ----
        for (int i = threadIdx.x; i < UC_UH * UC_UW * 32; i += THREADS) {
            const int pix = i >> 5, pos = i & 31, uy = pix / UC_UW, ux = pix - uy * UC_UW;
            const int c = 8 * ((pos >> 2) & 3) + 4 * (pos >> 4) + (pos & 3);
            const int Y = Y0 - 1 + uy, X = X0 - 1 + ux;
            float v = 0.f;                                       // outside the map: the convolution's zero padding
            if (Y >= 0 && Y < OH && X >= 0 && X < OW) {
                int y0, y1, x0, x1;
                float wy, wx;
                uc_source(Y, a.H, y0, y1, wy);
                uc_source(X, a.W, x0, x1, wx);
                const float* l0 = lo + c * UC_LCS + (y0 - m0) * UC_LW - n0;
                const float* l1 = lo + c * UC_LCS + (y1 - m0) * UC_LW - n0;
                v = uc_lerp(uc_lerp(l0[x0], l0[x1], wx), uc_lerp(l1[x0], l1[x1], wx), wy);
            }
            up[pix * PS + pos] = (T)v;                           // (float16: the one rounding to half)
        }
        wg_barrier();

        // ---- 3. the products; the loads run RING - 1 vectors ahead, behind the last k once more into its own tiles (in bounds, unused) ----
        const int kn = k + 1 < KT ? k + 1 : k;
        MlpIn<T> in[ROWS];
#pragma unroll
        for (int q = 0; q < STEPS; q++) {
            const int tile = q / NV, v = q - tile * NV, tap = tile / OT, t = tile - tap * OT, dy = tap / 3, dx = tap - 3 * dy, ahead = q + RING - 1;
            if (t == 0 && v == 0) {
#pragma unroll
                for (int j = 0; j < ROWS; j++) uc_operand(in[j], up + ((wave * ROWS + j + dy) * UC_UW + r + dx) * PS + 16 * h);
            }
            if (ahead < STEPS) ring[ahead % RING] = UC_WVEC(k, ahead);
            else ring[ahead % RING] = UC_WVEC(kn, ahead - STEPS);
            __builtin_amdgcn_sched_barrier(0);                   // (the load stays this far ahead of its product)
#pragma unroll
            for (int j = 0; j < ROWS; j++) acc[j][t] = uc_mm(ring[q % RING], in[j], v, acc[j][t]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#undef UC_WVEC

    const int X = X0 + r;
#pragma unroll
    for (int j = 0; j < ROWS; j++) {
        const int Y = Y0 + wave * ROWS + j;
        if (Y < OH && X < OW) {
            T* o = (T*)a.out + ((size_t)n * (size_t)a.Cout * OH + (size_t)Y) * OW + X;
#pragma unroll
            for (int t = 0; t < OT; t++) {
#pragma unroll
                for (int i = 0; i < 16; i++) {
                    const int c = 32 * t + attn_row(i, h);
                    if (c < a.Cout) o[(size_t)c * OH * OW] = (T)acc[j][t][i];
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the entry points (the contract is in include/igs_rast.h)
// ---------------------------------------------------------------------------------------------------------------------------------
template <int OT> static void upconv_launch(bool half, bool xhalf, dim3 grid, hipStream_t s, const UpconvArgs& a)
{
    const dim3 bh(64 * UcCfg<_Float16>::WAVES), bf(64 * UcCfg<float>::WAVES);
    if (xhalf) {
        if (half) hipLaunchKernelGGL((upconv_kernel<_Float16, _Float16, OT>), grid, bh, 0, s, a);
        else hipLaunchKernelGGL((upconv_kernel<float, _Float16, OT>), grid, bf, 0, s, a);
    } else {
        if (half) hipLaunchKernelGGL((upconv_kernel<_Float16, float, OT>), grid, bh, 0, s, a);
        else hipLaunchKernelGGL((upconv_kernel<float, float, OT>), grid, bf, 0, s, a);
    }
}

extern "C" long long igs_upconv_pack_elems(int Cin, int Cout, int conv_dtype)
{
    if (Cin < 1 || Cin > IGS_UPCONV_MAX_WIDTH || Cout < 1 || Cout > IGS_UPCONV_MAX_WIDTH || !dtype_ok(conv_dtype)) return -1;
    return 9LL * mlp_tiles(Cout) * mlp_tiles(Cin) * MLP_TILE;
}

extern "C" int igs_upconv_fwd(void* stream, int N, int Cin, int Cout, int H, int W, int x_dtype, const void* x, long long xs_n, long long xs_c,
                              long long xs_h, long long xs_w, int conv_dtype, const void* wpack, const float* bpack, void* out)
{
    const char* fn = "igs_upconv_fwd";
    if (N < 0 || N > IGS_UPCONV_MAX_PIXELS) return fail_in(fn, "N out of range");
    if (Cin < 1 || Cin > IGS_UPCONV_MAX_WIDTH) return fail_in(fn, "Cin out of range (1..IGS_UPCONV_MAX_WIDTH)");
    if (Cout < 1 || Cout > IGS_UPCONV_MAX_WIDTH) return fail_in(fn, "Cout out of range (1..IGS_UPCONV_MAX_WIDTH)");
    if (H < 1 || H > IGS_UPCONV_MAX_HW) return fail_in(fn, "H out of range (1..IGS_UPCONV_MAX_HW)");
    if (W < 1 || W > IGS_UPCONV_MAX_HW) return fail_in(fn, "W out of range (1..IGS_UPCONV_MAX_HW)");
    if ((long long)N * H * W > IGS_UPCONV_MAX_PIXELS) return fail_in(fn, "N * H * W out of range (IGS_UPCONV_MAX_PIXELS)");
    if (!dtype_ok(x_dtype) || !dtype_ok(conv_dtype)) return fail_in(fn, "unknown dtype code");
    if (const char* w = plane_stride_error(Cin, H, W, xs_n, xs_c, xs_h, xs_w)) return fail_in(fn, w);
    if (N == 0) return 0;
    if (!x || !wpack || !bpack || !out) return fail_in(fn, "NULL pointer");
    if (!ptr_aligned(x, dtype_bytes(x_dtype)) || !ptr_aligned(out, dtype_bytes(conv_dtype)))
        return fail_in(fn, "a pointer is not aligned to its element size");
    if (!ptr_aligned(wpack, 16) || !ptr_aligned(bpack, 16)) return fail_in(fn, "wpack and bpack must be aligned to 16 bytes");

    UpconvArgs a = {};
    a.Cin = Cin; a.Cout = Cout; a.H = H; a.W = W;
    a.tx = (uint32_t)((2 * W + UC_TX - 1) / UC_TX); a.ty = (uint32_t)((2 * H + UC_TY - 1) / UC_TY);
    a.x = x; a.xs_n = xs_n; a.xs_c = xs_c; a.w = wpack; a.b = bpack; a.out = out;
    // (tiles: at most N * ceil(H / 4) * ceil(W / 16) <= N H W <= 2^22)
    const dim3 grid(a.tx * a.ty * (uint32_t)N);
    hipStream_t s = (hipStream_t)stream;
    const bool half = conv_dtype == IGS_DTYPE_F16, xhalf = x_dtype == IGS_DTYPE_F16;
    switch (mlp_tiles(Cout)) {
    case 1: upconv_launch<1>(half, xhalf, grid, s, a); break;
    case 2: upconv_launch<2>(half, xhalf, grid, s, a); break;
    case 3: upconv_launch<3>(half, xhalf, grid, s, a); break;
    default: upconv_launch<4>(half, xhalf, grid, s, a); break;
    }
    HIP_TRY(hipGetLastError(), "upconv launch");
    return 0;
}
