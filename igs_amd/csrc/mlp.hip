// mlp.hip -- the residual decoder of AGM-Net in one launch (GS3DRenderer.decode_residual_feature, igs/models/gs.py:858-869): the small MLP
// (igs/models/networks.py:60-108) and the per-feature output Linears behind it, applied to one row per in-box Gaussian.  DESIGN.md 21.
//
//   h0 = x[n];  h_{l+1} = act_l(W_l h_l + b_l)  for the hidden Linears;  y = W_heads h_L + b_heads, split into one tensor per head
//
// Forward only.  A row is read from memory once, every layer runs in registers and only the heads' outputs are written.
//
// Tile layout.  One wave owns 32 rows.  The products are H^T = W X^T on 32x32 MFMA tiles: the output CHANNEL is the accumulator's row
// (register i of lane half h is channel 32 t + attn_row(i, h) of tile t), the data ROW is its column (lane & 31).  The next layer sums
// over the channel, i.e. over the accumulator's row index, so an accumulator tile is the next layer's B operand as it stands (float32)
// or after one rounding to half (float16): no lane movement, no LDS round trip.  The input rows are loaded straight into that same
// register order, so layer 0 is no special case.  The k order of such an operand is permuted (k-slot (e, h) is channel attn_row(e, h) of
// its 32-channel tile), so the weights are staged in the matching order: igs_amd/motion.py packs them once per parameter version, per
// 32x32 tile (ot, kt) as [chunk][lane 64][EPC] with EPC = 8 (half: chunk = k-step of v_mfma_f32_32x32x16_f16) or 4 (float: four
// v_mfma_f32_32x32x2_f32 per chunk), element e = chunk EPC + j of lane (r, h) = W[32 ot + r][32 kt + attn_row(e, h)], zero where the
// matrix ends.  A lane reads 16 consecutive bytes at lane * 16: no bank conflict.  Biases are float32 [layer][128], zero-padded; the
// accumulators start from them.  Both activations map 0 to 0, so padded channels stay 0.
//
// LDS plan.  float16: every layer at once (at most 4 x 32 KB, the shipped decoder 104 KB).  float32: one layer (at most 64 KB), staged
// between two workgroup barriers per layer and trip; with a single Linear it is staged once.  Plus 2 KB of biases and the 1.5 KB
// table that sends an output channel to its head.  float16: one workgroup of 16 waves per compute unit around the one copy of the
// weights, 4 waves per SIMD at up to 128 registers (8 waves measured 1.3 x slower: the kernel is bound by the activations' VALU work and
// the latency of its loads, which more waves hide).  float32: two workgroups of 4 waves per compute unit (2 x 67.5 KB of LDS), 2 waves
// per SIMD at up to 256 registers, so that one workgroup computes while the other stages its next layer, and so that the rows are dealt
// in trips of 128 (this kernel is bound by the matrix pipe: a SIMD's share of the tiles is what its time is made of).  A workgroup loops
// over trips of 32 rows per wave; the grid is at most what the chip holds at once.
#include "attn_common.h"
#include "host_api.h"

#define MLP_CUS 256                        // the compute units of an MI355X, where the device cannot be asked (mlp_cus)
// GROUPS_PER_CU: the workgroups a compute unit holds at once; more than that would only stage the weights again
template <typename T> struct MlpCfg { enum { WAVES = AttnCfg<T>::HALF ? 16 : 4, THREADS = 64 * WAVES, TRIP_ROWS = 32 * WAVES, GROUPS_PER_CU = AttnCfg<T>::HALF ? 1 : 2 }; };
#define MLP_TILE 1024                      // elements of one packed 32x32 weight tile
#define MLP_MAX_LINEARS (IGS_MLP_MAX_HIDDEN + 1)

struct MlpArgs {
    long long N;
    const void* x;
    long long xs;                          // row stride of x in elements
    const void* w;                         // packed weights in x's dtype, layer after layer
    const float* b;                        // [nl][128]
    int C0, nl;                            // nl: the hidden Linears plus the heads' one
    uint32_t kts, ots, acts;               // 4 bits per Linear: its input tiles, its output tiles, whether an activation follows
    int act;                               // IGS_MLP_ACT_*
    int nh;
    int hstart[IGS_MLP_MAX_HEADS + 1];     // the heads' first channels, and the end
    void* out[IGS_MLP_MAX_HEADS];
};

// the activations of 32 rows as the next product's B operand: element e of 32-channel tile k is channel 32 k + attn_row(e, h)
template <typename T> struct MlpIn;
template <> struct MlpIn<float> {
    float v[4][16];
    __device__ __forceinline__ void set(int k, int e, float f) { v[k][e] = f; }
};
template <> struct MlpIn<_Float16> {
    attn_h8 v[4][2];
    __device__ __forceinline__ void set(int k, int e, float f) { v[k][e >> 3][e & 7] = (_Float16)f; }     // the one rounding to half
};

// o += W tile x the activations' tile k
__device__ __forceinline__ attn_acc mlp_mm(const _Float16* tile, int lane, const MlpIn<_Float16>& in, int k, attn_acc o)
{
#pragma unroll
    for (int s = 0; s < 2; s++) o = __builtin_amdgcn_mfma_f32_32x32x16_f16(*(const attn_h8*)(tile + (s * 64 + lane) * 8), in.v[k][s], o, 0, 0, 0);
    return o;
}
__device__ __forceinline__ attn_acc mlp_mm(const float* tile, int lane, const MlpIn<float>& in, int k, attn_acc o)
{
#pragma unroll
    for (int g = 0; g < 4; g++) {
        const attn_f4 w = *(const attn_f4*)(tile + (g * 64 + lane) * 4);
#pragma unroll
        for (int u = 0; u < 4; u++) o = __builtin_amdgcn_mfma_f32_32x32x2f32(w[u], in.v[k][4 * g + u], o, 0, 0, 0);
    }
    return o;
}

// v sigmoid(v).  exp(-v) = exp2(t) (1 + tl ln 2) with t + tl = -v log2(e) to about 2^-48 relative: the product's rounding error comes back
// through the fma, so the argument's error does not grow with |v|.  v_exp_f32 and v_rcp_f32 are within 1 ulp each; with the rounding of
// 1 + e and of the last product the result is within 6 u (1 + small) of v sigmoid(v), u = 2^-24 (tests/decoder_restatement.py takes a = 8).
// sigmoid is taken of v held to [-128, 128] (beyond, it is 0 or 1 to float32 anyway) and the exponent is held at 126, so that t, tl, e,
// its correction and 1 + e stay finite for every v: below v = -87.3 the result is v / (1 + 2^126 (1 + tl ln 2)), within |v| 2^-126 of the
// true value (which is smaller still), never inf * c + inf = NaN; above 128 exp2 underflows to 0 and the result is v.  The last product
// takes v itself, so an infinity stays one on the positive side (-inf gives -inf * tiny = -inf where PyTorch gives NaN) and a NaN a NaN.
__device__ __forceinline__ float mlp_silu(float v)
{
    const float L = -1.4426950408889634f, Ll = -1.9259629911266175e-8f;      // -log2(e) = L + Ll
    const float c = __builtin_amdgcn_fmed3f(v, -128.f, 128.f);
    const float t = c * L;
    const float tl = fmaf(c, L, -t) + c * Ll;
    float e = attn_exp2(t > 126.f ? 126.f : t);
    e = fmaf(e, tl * 0.6931471805599453f, e);
    return v * __builtin_amdgcn_rcpf(1.f + e);
}
// max(v, 0) that keeps a NaN, as torch.relu does
__device__ __forceinline__ float mlp_relu(float v) { return v < 0.f ? 0.f : v; }

// `n` elements (a multiple of 8 halves / 4 floats) from global memory into LDS, 16 bytes per thread and step
template <typename T>
__device__ __forceinline__ void mlp_stage(T* dst, const T* src, uint32_t n)
{
    const uint32_t chunks = n * (uint32_t)sizeof(T) / 16;
    for (uint32_t i = threadIdx.x; i < chunks; i += MlpCfg<T>::THREADS) ((attn_f4*)dst)[i] = ((const attn_f4*)src)[i];
}

template <typename T, bool VEC>
__global__ __launch_bounds__(MlpCfg<T>::THREADS, AttnCfg<T>::HALF ? 4 : 2) void mlp_heads_kernel(const MlpArgs a)      // (registers: 128 at 4 waves per SIMD, 256 at 2)
{
    constexpr bool HALF = AttnCfg<T>::HALF;
    constexpr int MLP_THREADS = MlpCfg<T>::THREADS, MLP_TRIP_ROWS = MlpCfg<T>::TRIP_ROWS;
    __shared__ __attribute__((aligned(16))) T wl[(HALF ? MLP_MAX_LINEARS : 1) * 16 * MLP_TILE];
    __shared__ __attribute__((aligned(16))) float bl[MLP_MAX_LINEARS * 128];
    __shared__ unsigned long long ch_ptr[128];           // where output channel c of row 0 goes (0: a padded channel), and its head's width
    __shared__ int ch_w[128];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const T* wg = (const T*)a.w;

    for (int i = threadIdx.x; i < a.nl * 128; i += MLP_THREADS) bl[i] = a.b[i];
    if (threadIdx.x < 128) {
        const int c = threadIdx.x;
        unsigned long long p = 0;
        int w = 0;
#pragma unroll
        for (int k = 0; k < IGS_MLP_MAX_HEADS; k++)
            if (k < a.nh && c >= a.hstart[k] && c < a.hstart[k + 1]) {
                p = (unsigned long long)((T*)a.out[k] + (c - a.hstart[k]));
                w = a.hstart[k + 1] - a.hstart[k];
            }
        ch_ptr[c] = p;
        ch_w[c] = w;
    }
    uint32_t total = 0;
    for (int l = 0; l < a.nl; l++) total += ((a.kts >> (4 * l)) & 15) * ((a.ots >> (4 * l)) & 15) * MLP_TILE;
    if (HALF || a.nl == 1) mlp_stage(wl, wg, total);
    wg_barrier();

    const long long trips = (a.N + MLP_TRIP_ROWS - 1) / MLP_TRIP_ROWS;
    for (long long trip = blockIdx.x; trip < trips; trip += gridDim.x) {
        const long long row = trip * MLP_TRIP_ROWS + wave * 32 + r;
        const bool live = row < a.N;
        const T* xr = (const T*)a.x + (live ? row : 0) * a.xs;

        MlpIn<T> in;
#pragma unroll
        for (int k = 0; k < 4; k++) {
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const int c = 32 * k + 8 * g + 4 * h;
                float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
                if (VEC) {                                       // C0 is a multiple of 4: the four channels are inside or outside together
                    if (live && c < a.C0) f = ld4(xr + c);
                } else if (live) {
                    if (c < a.C0) f.x = ld(xr + c);
                    if (c + 1 < a.C0) f.y = ld(xr + c + 1);
                    if (c + 2 < a.C0) f.z = ld(xr + c + 2);
                    if (c + 3 < a.C0) f.w = ld(xr + c + 3);
                }
                in.set(k, 4 * g, f.x); in.set(k, 4 * g + 1, f.y); in.set(k, 4 * g + 2, f.z); in.set(k, 4 * g + 3, f.w);
            }
        }

        uint32_t woff = 0;
        for (int l = 0; l < a.nl; l++) {
            const int kt = (a.kts >> (4 * l)) & 15, ot = (a.ots >> (4 * l)) & 15;
            const uint32_t elems = (uint32_t)(kt * ot) * MLP_TILE;
            if (!HALF && a.nl > 1) {                             // (uniform over the workgroup: every wave takes every trip)
                wg_barrier();                                    // everybody is done with the layer before
                mlp_stage(wl, wg + woff, elems);
                wg_barrier();
            }
            const T* wp = (HALF || a.nl == 1) ? wl + woff : wl;
            woff += elems;

            attn_acc o[4];
#pragma unroll
            for (int t = 0; t < 4; t++) {
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    const attn_f4 bv = *(const attn_f4*)(bl + l * 128 + 32 * t + 8 * g + 4 * h);
                    o[t][4 * g] = bv[0]; o[t][4 * g + 1] = bv[1]; o[t][4 * g + 2] = bv[2]; o[t][4 * g + 3] = bv[3];
                }
            }
#pragma unroll
            for (int t = 0; t < 4; t++) {
                if (t < ot) {
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        if (k < kt) o[t] = mlp_mm(wp + (t * kt + k) * MLP_TILE, lane, in, k, o[t]);
                }
            }

            if (l + 1 < a.nl) {
                const bool on = (a.acts >> (4 * l)) & 1;
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    if (t < ot) {
#pragma unroll
                        for (int i = 0; i < 16; i++) {
                            float v = o[t][i];
                            if (on) v = a.act == IGS_MLP_ACT_RELU ? mlp_relu(v) : mlp_silu(v);
                            in.set(t, i, v);
                        }
                    }
                }
            } else if (live) {
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    if (t < ot) {
#pragma unroll
                        for (int i = 0; i < 16; i++) {
                            const int c = 32 * t + attn_row(i, h);
                            const unsigned long long p = ch_ptr[c];
                            if (p) st((T*)p + row * ch_w[c], o[t][i]);
                        }
                    }
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the entry points (the contract is in include/igs_rast.h)
// ---------------------------------------------------------------------------------------------------------------------------------
static int mlp_tiles(int c) { return (c + 31) / 32; }

// the compute units of the current device (a partition in the CPX modes has fewer than the whole chip), asked once per device
static int mlp_cus()
{
    static int cus[64];
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) return MLP_CUS;
    if (cus[d] == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, d) != hipSuccess || n < 1) return MLP_CUS;
        cus[d] = n;
    }
    return cus[d];
}

// the sizes of a decoder, or what is wrong with them
static const char* mlp_size_error(int n_hidden, const int* widths, int n_heads, const int* head_widths, int* head_sum)
{
    if (n_hidden < 0 || n_hidden > IGS_MLP_MAX_HIDDEN) return "n_hidden out of range (0..IGS_MLP_MAX_HIDDEN)";
    if (n_heads < 1 || n_heads > IGS_MLP_MAX_HEADS) return "n_heads out of range (1..IGS_MLP_MAX_HEADS)";
    if (!widths || !head_widths) return "NULL widths or head_widths";
    for (int l = 0; l <= n_hidden; l++)
        if (widths[l] < 1 || widths[l] > IGS_MLP_MAX_WIDTH) return "a width is out of range (1..IGS_MLP_MAX_WIDTH)";
    int sum = 0;
    for (int k = 0; k < n_heads; k++) {
        if (head_widths[k] < 1 || head_widths[k] > IGS_MLP_MAX_WIDTH) return "a head width is out of range (1..IGS_MLP_MAX_WIDTH)";
        sum += head_widths[k];
    }
    if (sum > IGS_MLP_MAX_WIDTH) return "the head widths add up to more than IGS_MLP_MAX_WIDTH";
    *head_sum = sum;
    return nullptr;
}

extern "C" long long igs_mlp_heads_pack_elems(int n_hidden, const int* widths, int n_heads, const int* head_widths)
{
    int head_sum = 0;
    if (mlp_size_error(n_hidden, widths, n_heads, head_widths, &head_sum)) return -1;
    long long n = 0;
    for (int l = 0; l <= n_hidden; l++) n += (long long)mlp_tiles(widths[l]) * mlp_tiles(l < n_hidden ? widths[l + 1] : head_sum) * MLP_TILE;
    return n;
}

extern "C" int igs_mlp_heads_fwd(void* stream, long long N, int dtype, int act, int n_hidden, const int* widths, const int* act_after,
                                 int n_heads, const int* head_widths, const void* x, long long x_rs, const void* wpack, const float* bpack,
                                 void* const* outs)
{
    const char* fn = "igs_mlp_heads_fwd";
    if (!dtype_ok(dtype)) return fail_in(fn, "unknown dtype code");
    if (act != IGS_MLP_ACT_SILU && act != IGS_MLP_ACT_RELU) return fail_in(fn, "unknown activation code");
    if (N < 0 || N > IGS_MLP_MAX_ROWS) return fail_in(fn, "N out of range (0..IGS_MLP_MAX_ROWS)");
    int head_sum = 0;
    if (const char* w = mlp_size_error(n_hidden, widths, n_heads, head_widths, &head_sum)) return fail_in(fn, w);
    if (n_hidden > 0 && !act_after) return fail_in(fn, "NULL act_after");
    if (x_rs < widths[0] || x_rs > IGS_TOKENS_MAX_STRIDE) return fail_in(fn, "row stride below the input width or above IGS_TOKENS_MAX_STRIDE");
    if (N == 0) return 0;
    if (!x || !wpack || !bpack || !outs) return fail_in(fn, "NULL pointer");
    for (int k = 0; k < n_heads; k++) {
        if (!outs[k]) return fail_in(fn, "NULL output pointer");
        if (!ptr_aligned(outs[k], dtype_bytes(dtype))) return fail_in(fn, "a pointer is not aligned to its element size");
    }
    if (!ptr_aligned(x, dtype_bytes(dtype)) || !ptr_aligned(bpack, 4)) return fail_in(fn, "a pointer is not aligned to its element size");
    if (!ptr_aligned(wpack, 16)) return fail_in(fn, "wpack must be aligned to 16 bytes");

    MlpArgs a = {};
    a.N = N; a.x = x; a.xs = x_rs; a.w = wpack; a.b = bpack;
    a.C0 = widths[0]; a.nl = n_hidden + 1; a.act = act; a.nh = n_heads;
    for (int l = 0; l <= n_hidden; l++) {
        a.kts |= (uint32_t)mlp_tiles(widths[l]) << (4 * l);
        a.ots |= (uint32_t)mlp_tiles(l < n_hidden ? widths[l + 1] : head_sum) << (4 * l);
        if (l < n_hidden && act_after[l]) a.acts |= 1u << (4 * l);
    }
    for (int k = 0; k < n_heads; k++) {
        a.hstart[k + 1] = a.hstart[k] + head_widths[k];
        a.out[k] = outs[k];
    }
    const bool half = dtype == IGS_DTYPE_F16;
    const int trip_rows = half ? MlpCfg<_Float16>::TRIP_ROWS : MlpCfg<float>::TRIP_ROWS;
    const int groups = mlp_cus() * (half ? MlpCfg<_Float16>::GROUPS_PER_CU : MlpCfg<float>::GROUPS_PER_CU);
    const long long trips = (N + trip_rows - 1) / trip_rows;
    const dim3 grid((unsigned)(trips < groups ? trips : groups)), block(half ? MlpCfg<_Float16>::THREADS : MlpCfg<float>::THREADS);
    const bool vec = (widths[0] & 3) == 0 && (x_rs & 3) == 0 && ptr_aligned(x, vec_grid_bytes(dtype));
    hipStream_t s = (hipStream_t)stream;
    if (half) {
        if (vec) hipLaunchKernelGGL((mlp_heads_kernel<_Float16, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((mlp_heads_kernel<_Float16, false>), grid, block, 0, s, a);
    } else {
        if (vec) hipLaunchKernelGGL((mlp_heads_kernel<float, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((mlp_heads_kernel<float, false>), grid, block, 0, s, a);
    }
    HIP_TRY(hipGetLastError(), "mlp heads launch");
    return 0;
}
