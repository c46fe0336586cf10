// mlp.hip -- the residual decoder of AGM-Net in one launch (GS3DRenderer.decode_residual_feature, igs/models/gs.py:858-869): the small MLP
// (igs/models/networks.py:60-108) and the per-feature output Linears behind it, applied to one row per in-box Gaussian.  DESIGN.md 21.
//
//   h0 = x[n];  h_{l+1} = act_l(W_l h_l + b_l)  for the hidden Linears;  y = W_heads h_L + b_heads, split into one tensor per head
//
// Forward: a row is read from memory once, every layer runs in registers and only the heads' outputs are written.  The backward
// (igs_mlp_heads_bwd, behind the forward kernel) recomputes the forward from x chunk by chunk: nothing of N rows but x is kept.
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
#include "mlp_common.h"                   // MlpIn, mlp_mm, mlp_silu, MLP_TILE, mlp_tiles, mlp_cus
#include "host_api.h"

// GROUPS_PER_CU: the workgroups a compute unit holds at once; more than that would only stage the weights again
template <typename T> struct MlpCfg { enum { WAVES = AttnCfg<T>::HALF ? 16 : 4, THREADS = 64 * WAVES, TRIP_ROWS = 32 * WAVES, GROUPS_PER_CU = AttnCfg<T>::HALF ? 1 : 2 }; };
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
// The backward.  N is walked in chunks of MLP_BWD_CHUNK_ROWS rows; per chunk two launches, after the last chunk one more:
//   mlp_bwd_rows_kernel    a wave owns 32 rows, as in the forward.  It recomputes the hidden layers and leaves every Linear's input
//                          (x, then the pre-activations z_l) in the chunk scratch as float32 rows [row][128]; then it runs the dgrad chain
//                          dh_l = W_l^T dz_l on the same tile scheme with the transposed packs (an accumulator tile is the next product's
//                          B operand as it stands), reading back its own z_l for the derivative (the lane that wrote an element is the
//                          lane that reads it: no barrier), leaves every dz_l (the heads' d Y included) beside them and writes d x.
//   mlp_bwd_wgrad_kernel   d W_l = dz_l^T h_l contracts over the data row.  The row-major scratch is the transpose both operands need:
//                          lane r of a wave reads channel r of a row, which is the A / B operand of a product over rows as it stands.
//                          A wave owns (slice of MLP_BWD_SLICE_ROWS rows, Linear, input tile): it applies the activation to its 32 input
//                          channels on load, forms the up to four 32x32 tiles of its column of d W, and for input tile 0 the bias sums.
//                          Its float32 accumulators start from the slice's partial of the chunk before, so a slice's partial is the
//                          sum over its rows in row order, chunk after chunk.
//   mlp_bwd_reduce_kernel  adds the slices' partials in slice order into d W / d b.
// No float atomics anywhere; the order of every sum depends on the sizes only.  All gradients of parameters are float32.
#define MLP_BWD_CHUNK_ROWS 16384           // R: the rows whose z_l and dz_l exist at once (67 MB of scratch for the shipped decoder; 32768
                                           // measured 1.5 x faster at twice the scratch, 65536 no faster than that: DESIGN.md 21)
#define MLP_BWD_SLICE_ROWS 256             // rows per wgrad partial: 64 slices x (Linear, input tile) pairs fill the chip's SIMDs once
#define MLP_BWD_SLICES (MLP_BWD_CHUNK_ROWS / MLP_BWD_SLICE_ROWS)
#define MLP_BWD_WAVES 4
#define MLP_BWD_THREADS (64 * MLP_BWD_WAVES)
#define MLP_BWD_TRIP_ROWS (32 * MLP_BWD_WAVES)

struct MlpBwdArgs {
    long long row0;                        // the chunk is rows row0 .. row0 + rows - 1
    int rows, chunk;
    const void* x;
    long long xs;
    const void* w;                         // packed W_l
    const void* wt;                        // packed W_l^T: the same tile counts per Linear
    const float* b;
    int C0, nl;
    uint32_t kts, ots, acts;
    int act, nh;
    int hstart[IGS_MLP_MAX_HEADS + 1];
    const void* dout[IGS_MLP_MAX_HEADS];   // NULL: zeros
    void* dx;                              // [N][C0] contiguous, or NULL
    int dx_vec, want_w;
    float* slots;                          // [2 nl][slot rows][128]: the Linears' inputs, then their outputs' gradients
    long long slot_stride;
    float* part;                           // [slice][pstride]: d W of every Linear in nn.Linear's layout, then d b
    uint32_t pstride, tw;
    int O[MLP_MAX_LINEARS], I[MLP_MAX_LINEARS], woff[MLP_MAX_LINEARS], boff[MLP_MAX_LINEARS];
    int npairs, units;
    unsigned char pair_l[16], pair_k[16];  // the (Linear, input tile) pairs
};

// dz = g act'(z).  ReLU: 0 at z <= 0 whatever g is (as torch's threshold_backward), g above 0, and a NaN z stays one.
__device__ __forceinline__ float mlp_act_grad(int act, float z, float g)
{
    if (act == IGS_MLP_ACT_RELU) return z <= 0.f ? 0.f : (z == z ? g : z);
    return g * mlp_silu_grad(z);
}

template <typename T>
__device__ __forceinline__ void mlp_bwd_stage(T* dst, const T* src, uint32_t n)
{
    const uint32_t chunks = n * (uint32_t)sizeof(T) / 16;
    for (uint32_t i = threadIdx.x; i < chunks; i += MLP_BWD_THREADS) ((attn_f4*)dst)[i] = ((const attn_f4*)src)[i];
}

template <typename T, bool VEC>
__global__ __launch_bounds__(MLP_BWD_THREADS, 2) void mlp_bwd_rows_kernel(const MlpBwdArgs a)
{
    __shared__ __attribute__((aligned(16))) T wl[16 * MLP_TILE];           // one Linear at a time, staged between two barriers
    __shared__ __attribute__((aligned(16))) float bl[MLP_MAX_LINEARS * 128];
    __shared__ unsigned long long ch_ptr[128];           // where channel c of d Y, row 0, is read (0: a padded channel or an absent head)
    __shared__ int ch_w[128];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    for (int i = threadIdx.x; i < a.nl * 128; i += MLP_BWD_THREADS) bl[i] = a.b[i];
    if (threadIdx.x < 128) {
        const int c = threadIdx.x;
        unsigned long long p = 0;
        int w = 0;
#pragma unroll
        for (int k = 0; k < IGS_MLP_MAX_HEADS; k++)
            if (k < a.nh && c >= a.hstart[k] && c < a.hstart[k + 1] && a.dout[k]) {
                p = (unsigned long long)((const T*)a.dout[k] + (c - a.hstart[k]));
                w = a.hstart[k + 1] - a.hstart[k];
            }
        ch_ptr[c] = p;
        ch_w[c] = w;
    }
    wg_barrier();

    const int trips = (a.rows + MLP_BWD_TRIP_ROWS - 1) / MLP_BWD_TRIP_ROWS;
    for (int trip = blockIdx.x; trip < trips; trip += gridDim.x) {      // (uniform over the workgroup: every wave takes every trip)
        const int lr = trip * MLP_BWD_TRIP_ROWS + wave * 32 + r;
        const bool live = lr < a.rows;
        const long long row = a.row0 + lr;
        const T* xr = (const T*)a.x + (live ? row : 0) * a.xs;
        float* slot = a.slots + (size_t)lr * 128 + 4 * h;                 // this lane's 4-channel groups of its row, in slot 0

        MlpIn<T> in;
#pragma unroll
        for (int k = 0; k < 4; k++) {
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const int c = 32 * k + 8 * g + 4 * h;
                float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
                if (VEC) {
                    if (live && c < a.C0) f = ld4(xr + c);
                } else if (live) {
                    if (c < a.C0) f.x = ld(xr + c);
                    if (c + 1 < a.C0) f.y = ld(xr + c + 1);
                    if (c + 2 < a.C0) f.z = ld(xr + c + 2);
                    if (c + 3 < a.C0) f.w = ld(xr + c + 3);
                }
                in.set(k, 4 * g, f.x); in.set(k, 4 * g + 1, f.y); in.set(k, 4 * g + 2, f.z); in.set(k, 4 * g + 3, f.w);
                if (a.want_w && live) *(float4*)(slot + 32 * k + 8 * g) = f;
            }
        }

        // the hidden layers again; z_l goes to slot l + 1
        uint32_t woff = 0;
        for (int l = 0; l + 1 < a.nl; l++) {
            const int kt = (a.kts >> (4 * l)) & 15, ot = (a.ots >> (4 * l)) & 15;
            wg_barrier();                                        // everybody is done with the Linear before
            mlp_bwd_stage(wl, (const T*)a.w + woff, (uint32_t)(kt * ot) * MLP_TILE);
            wg_barrier();
            woff += (uint32_t)(kt * ot) * MLP_TILE;
            const bool on = (a.acts >> (4 * l)) & 1;
            float* zs = slot + (size_t)(l + 1) * a.slot_stride;
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
                        if (k < kt) o[t] = mlp_mm(wl + (t * kt + k) * MLP_TILE, lane, in, k, o[t]);
                }
            }
#pragma unroll
            for (int t = 0; t < 4; t++) {
                if (t < ot) {
#pragma unroll
                    for (int g = 0; g < 4; g++) {
                        if (live) *(float4*)(zs + 32 * t + 8 * g) = make_float4(o[t][4 * g], o[t][4 * g + 1], o[t][4 * g + 2], o[t][4 * g + 3]);
#pragma unroll
                        for (int j = 0; j < 4; j++) {
                            float v = o[t][4 * g + j];
                            if (on) v = a.act == IGS_MLP_ACT_RELU ? mlp_relu(v) : mlp_silu(v);
                            in.set(t, 4 * g + j, v);
                        }
                    }
                }
            }
        }

        // d Y in the operand order, and as the last Linear's dz in slot nl + (nl - 1)
        {
            const int ot = (a.ots >> (4 * (a.nl - 1))) & 15;
            float* ds = slot + (size_t)(2 * a.nl - 1) * a.slot_stride;
#pragma unroll
            for (int t = 0; t < 4; t++) {
                if (t < ot) {
#pragma unroll
                    for (int g = 0; g < 4; g++) {
                        float f[4];
#pragma unroll
                        for (int j = 0; j < 4; j++) {
                            const int c = 32 * t + 8 * g + 4 * h + j;
                            const unsigned long long p = ch_ptr[c];
                            f[j] = (p && live) ? ld((const T*)p + row * ch_w[c]) : 0.f;
                            in.set(t, 4 * g + j, f[j]);
                        }
                        if (a.want_w && live) *(float4*)(ds + 32 * t + 8 * g) = make_float4(f[0], f[1], f[2], f[3]);
                    }
                }
            }
        }

        // the dgrad chain: dh_l = W_l^T dz_l, then dz_{l-1} = dh_l act'(z_{l-1})
        for (int l = a.nl - 1; l >= 0; l--) {
            if (l == 0 && !a.dx) break;                          // (uniform)
            const int kt = (a.kts >> (4 * l)) & 15, ot = (a.ots >> (4 * l)) & 15;
            woff = 0;
            for (int j = 0; j < l; j++) woff += ((a.kts >> (4 * j)) & 15) * ((a.ots >> (4 * j)) & 15) * MLP_TILE;
            wg_barrier();
            mlp_bwd_stage(wl, (const T*)a.wt + woff, (uint32_t)(kt * ot) * MLP_TILE);
            wg_barrier();
            attn_acc o[4];
#pragma unroll
            for (int t = 0; t < 4; t++) {
#pragma unroll
                for (int i = 0; i < 16; i++) o[t][i] = 0.f;
            }
#pragma unroll
            for (int t = 0; t < 4; t++) {                        // W^T is a Linear of ot input tiles and kt output tiles
                if (t < kt) {
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        if (k < ot) o[t] = mlp_mm(wl + (t * ot + k) * MLP_TILE, lane, in, k, o[t]);
                }
            }
            if (l == 0) {
                T* dxr = (T*)a.dx + row * a.C0;
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    if (t < kt && live) {
#pragma unroll
                        for (int g = 0; g < 4; g++) {
                            const int c = 32 * t + 8 * g + 4 * h;
                            if (a.dx_vec) {
                                if (c < a.C0) st4(dxr + c, make_float4(o[t][4 * g], o[t][4 * g + 1], o[t][4 * g + 2], o[t][4 * g + 3]));
                            } else {
#pragma unroll
                                for (int j = 0; j < 4; j++)
                                    if (c + j < a.C0) st(dxr + c + j, o[t][4 * g + j]);
                            }
                        }
                    }
                }
            } else {
                const bool on = (a.acts >> (4 * (l - 1))) & 1;
                const float* zs = slot + (size_t)l * a.slot_stride;
                float* ds = slot + (size_t)(a.nl + l - 1) * a.slot_stride;
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    if (t < kt) {
#pragma unroll
                        for (int g = 0; g < 4; g++) {
                            float f[4] = {o[t][4 * g], o[t][4 * g + 1], o[t][4 * g + 2], o[t][4 * g + 3]};
                            if (on) {
                                float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
                                if (live) z = *(const float4*)(zs + 32 * t + 8 * g);
                                f[0] = mlp_act_grad(a.act, z.x, f[0]); f[1] = mlp_act_grad(a.act, z.y, f[1]);
                                f[2] = mlp_act_grad(a.act, z.z, f[2]); f[3] = mlp_act_grad(a.act, z.w, f[3]);
                            }
                            if (a.want_w && live) *(float4*)(ds + 32 * t + 8 * g) = make_float4(f[0], f[1], f[2], f[3]);
#pragma unroll
                            for (int j = 0; j < 4; j++) in.set(t, 4 * g + j, f[j]);
                        }
                    }
                }
            }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(MLP_BWD_THREADS) void mlp_bwd_wgrad_kernel(const MlpBwdArgs a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int u = blockIdx.x * MLP_BWD_WAVES + wave;
    if (u >= a.units) return;                                    // (no barrier in this kernel)
    const int slice = u / a.npairs, l = a.pair_l[u % a.npairs], kt = a.pair_k[u % a.npairs];
    const int lr0 = slice * MLP_BWD_SLICE_ROWS, lr1 = min(lr0 + MLP_BWD_SLICE_ROWS, a.rows);
    if (lr0 >= lr1) return;                                      // (the last chunk's empty slices keep the partial they have)
    const int ot = (a.ots >> (4 * l)) & 15, O = a.O[l], I = a.I[l];
    const bool on = l > 0 && ((a.acts >> (4 * (l - 1))) & 1);
    const float* hs = a.slots + (size_t)l * a.slot_stride + 32 * kt + r;
    const float* ds = a.slots + (size_t)(a.nl + l) * a.slot_stride + r;
    float* pw = a.part + (size_t)slice * a.pstride + a.woff[l];
    float* pb = a.part + (size_t)slice * a.pstride + a.tw + a.boff[l];
    const int col = 32 * kt + r;

    attn_acc acc[4];
    float bs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 4; t++) {
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int o = 32 * t + attn_row(i, h);
            acc[t][i] = (a.chunk > 0 && t < ot && o < O && col < I) ? pw[(size_t)o * I + col] : 0.f;
        }
    }
    for (int n0 = lr0; n0 < lr1; n0 += 16) {
        float bv[8], av[4][8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int n = n0 + mlp_wgrad_row<T>(j, h);
            const bool ok = n < lr1;
            float v = ok ? hs[(size_t)n * 128] : 0.f;
            if (on) v = a.act == IGS_MLP_ACT_RELU ? mlp_relu(v) : mlp_silu(v);
            bv[j] = v;
#pragma unroll
            for (int t = 0; t < 4; t++) av[t][j] = (ok && t < ot) ? ds[(size_t)n * 128 + 32 * t] : 0.f;
        }
#pragma unroll
        for (int t = 0; t < 4; t++) {
            if (t < ot) {
#pragma unroll
                for (int j = 0; j < 8; j++) bs[t] += av[t][j];
                acc[t] = mlp_wgrad_mm(T(0), av[t], bv, acc[t]);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 4; t++) {
        if (t < ot) {
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int o = 32 * t + attn_row(i, h);
                if (o < O && col < I) pw[(size_t)o * I + col] = acc[t][i];
            }
            if (kt == 0) {                                       // (uniform over the wave)
                const float s = bs[t] + __shfl_xor(bs[t], 32, 64);
                const int o = 32 * t + r;
                if (h == 0 && o < O) pb[o] = (a.chunk > 0 ? pb[o] : 0.f) + s;
            }
        }
    }
}

// d W and d b, each where wanted: the slices' partials added in slice order
__global__ __launch_bounds__(256) void mlp_bwd_reduce_kernel(const float* __restrict__ part, uint32_t pstride, int slices, uint32_t tw, uint32_t tb,
                                                             float* __restrict__ dw, float* __restrict__ db)
{
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= tw + tb) return;
    float s = 0.f;
    for (int k = 0; k < slices; k++) s += part[(size_t)k * pstride + j];
    if (j < tw) { if (dw) dw[j] = s; }
    else if (db) db[j - tw] = s;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the entry points (the contract is in include/igs_rast.h)
// ---------------------------------------------------------------------------------------------------------------------------------
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

// ---- the backward ----
struct MlpBwdSizes { int nl, head_sum, O[MLP_MAX_LINEARS], I[MLP_MAX_LINEARS], woff[MLP_MAX_LINEARS], boff[MLP_MAX_LINEARS]; uint32_t tw, tb, pstride; };
static MlpBwdSizes mlp_bwd_sizes(int n_hidden, const int* widths, int head_sum)
{
    MlpBwdSizes z = {};
    z.nl = n_hidden + 1;
    z.head_sum = head_sum;
    for (int l = 0; l < z.nl; l++) {
        z.I[l] = widths[l];
        z.O[l] = l < n_hidden ? widths[l + 1] : head_sum;
        z.woff[l] = (int)z.tw;
        z.boff[l] = (int)z.tb;
        z.tw += (uint32_t)(z.O[l] * z.I[l]);
        z.tb += (uint32_t)z.O[l];
    }
    z.pstride = (z.tw + z.tb + 3u) & ~3u;
    return z;
}
static long long mlp_bwd_scratch(long long N, const MlpBwdSizes& z)
{
    const long long slot_rows = N < MLP_BWD_CHUNK_ROWS ? N : MLP_BWD_CHUNK_ROWS;
    const long long slices = (slot_rows + MLP_BWD_SLICE_ROWS - 1) / MLP_BWD_SLICE_ROWS;
    return (2LL * z.nl * slot_rows * 128 + slices * z.pstride) * (long long)sizeof(float);
}

extern "C" long long igs_mlp_heads_bwd_scratch_bytes(long long N, int dtype, int n_hidden, const int* widths, int n_heads, const int* head_widths)
{
    int head_sum = 0;
    if (!dtype_ok(dtype) || N < 0 || N > IGS_MLP_MAX_ROWS || mlp_size_error(n_hidden, widths, n_heads, head_widths, &head_sum)) return -1;
    return mlp_bwd_scratch(N, mlp_bwd_sizes(n_hidden, widths, head_sum));
}

extern "C" int igs_mlp_heads_bwd(void* stream, long long N, int dtype, int act, int n_hidden, const int* widths, const int* act_after, int n_heads,
                                 const int* head_widths, const void* x, long long x_rs, const void* wpack, const void* wpack_t, const float* bpack,
                                 const void* const* douts, void* scratch, long long scratch_bytes, void* dx, float* dw, float* db)
{
    const char* fn = "igs_mlp_heads_bwd";
    if (!dtype_ok(dtype)) return fail_in(fn, "unknown dtype code");
    if (act != IGS_MLP_ACT_SILU && act != IGS_MLP_ACT_RELU) return fail_in(fn, "unknown activation code");
    if (N < 0 || N > IGS_MLP_MAX_ROWS) return fail_in(fn, "N out of range (0..IGS_MLP_MAX_ROWS)");
    int head_sum = 0;
    if (const char* w = mlp_size_error(n_hidden, widths, n_heads, head_widths, &head_sum)) return fail_in(fn, w);
    if (n_hidden > 0 && !act_after) return fail_in(fn, "NULL act_after");
    if (x_rs < widths[0] || x_rs > IGS_TOKENS_MAX_STRIDE) return fail_in(fn, "row stride below the input width or above IGS_TOKENS_MAX_STRIDE");
    if (!ptr_aligned(dw, 4) || !ptr_aligned(db, 4)) return fail_in(fn, "a pointer is not aligned to its element size");
    const MlpBwdSizes z = mlp_bwd_sizes(n_hidden, widths, head_sum);
    hipStream_t s = (hipStream_t)stream;
    if (N == 0) {
        if (dw) HIP_TRY(hipMemsetAsync(dw, 0, (size_t)z.tw * sizeof(float), s), "mlp heads bwd zero-fill");
        if (db) HIP_TRY(hipMemsetAsync(db, 0, (size_t)z.tb * sizeof(float), s), "mlp heads bwd zero-fill");
        return 0;
    }
    if (!x || !wpack || !wpack_t || !bpack || !douts || !scratch) return fail_in(fn, "NULL pointer");
    for (int k = 0; k < n_heads; k++)
        if (!ptr_aligned(douts[k], dtype_bytes(dtype))) return fail_in(fn, "a pointer is not aligned to its element size");
    if (!ptr_aligned(x, dtype_bytes(dtype)) || !ptr_aligned(dx, dtype_bytes(dtype)) || !ptr_aligned(bpack, 4))
        return fail_in(fn, "a pointer is not aligned to its element size");
    if (!ptr_aligned(wpack, 16) || !ptr_aligned(wpack_t, 16)) return fail_in(fn, "wpack and wpack_t must be aligned to 16 bytes");
    if (!ptr_aligned(scratch, 16)) return fail_in(fn, "scratch must be aligned to 16 bytes");
    if (scratch_bytes < mlp_bwd_scratch(N, z)) return fail_in(fn, "scratch is smaller than igs_mlp_heads_bwd_scratch_bytes");
    if (!dx && !dw && !db) return 0;

    MlpBwdArgs a = {};
    a.x = x; a.xs = x_rs; a.w = wpack; a.wt = wpack_t; a.b = bpack;
    a.C0 = widths[0]; a.nl = z.nl; a.act = act; a.nh = n_heads;
    for (int l = 0; l < z.nl; l++) {
        const int kt = mlp_tiles(z.I[l]);
        a.kts |= (uint32_t)kt << (4 * l);
        a.ots |= (uint32_t)mlp_tiles(z.O[l]) << (4 * l);
        if (l < n_hidden && act_after[l]) a.acts |= 1u << (4 * l);
        a.O[l] = z.O[l]; a.I[l] = z.I[l]; a.woff[l] = z.woff[l]; a.boff[l] = z.boff[l];
        for (int k = 0; k < kt; k++) { a.pair_l[a.npairs] = (unsigned char)l; a.pair_k[a.npairs] = (unsigned char)k; a.npairs++; }
    }
    for (int k = 0; k < n_heads; k++) {
        a.hstart[k + 1] = a.hstart[k] + head_widths[k];
        a.dout[k] = douts[k];
    }
    a.dx = dx;
    a.dx_vec = (widths[0] & 3) == 0 && ptr_aligned(dx, vec_grid_bytes(dtype));
    a.want_w = dw || db;
    const long long slot_rows = N < MLP_BWD_CHUNK_ROWS ? N : MLP_BWD_CHUNK_ROWS;
    a.slots = (float*)scratch;
    a.slot_stride = slot_rows * 128;
    a.part = a.slots + 2LL * z.nl * a.slot_stride;
    a.pstride = z.pstride; a.tw = z.tw;
    const int slices = (int)((slot_rows + MLP_BWD_SLICE_ROWS - 1) / MLP_BWD_SLICE_ROWS);
    a.units = slices * a.npairs;

    const bool half = dtype == IGS_DTYPE_F16;
    const bool vec = (widths[0] & 3) == 0 && (x_rs & 3) == 0 && ptr_aligned(x, vec_grid_bytes(dtype));
    const int groups = mlp_cus() * 2;
    const dim3 block(MLP_BWD_THREADS);
    for (long long row0 = 0; row0 < N; row0 += MLP_BWD_CHUNK_ROWS) {
        a.row0 = row0;
        a.rows = (int)(N - row0 < MLP_BWD_CHUNK_ROWS ? N - row0 : MLP_BWD_CHUNK_ROWS);
        a.chunk = (int)(row0 / MLP_BWD_CHUNK_ROWS);
        const int trips = (a.rows + MLP_BWD_TRIP_ROWS - 1) / MLP_BWD_TRIP_ROWS;
        const dim3 grid((unsigned)(trips < groups ? trips : groups));
        if (half) {
            if (vec) hipLaunchKernelGGL((mlp_bwd_rows_kernel<_Float16, true>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((mlp_bwd_rows_kernel<_Float16, false>), grid, block, 0, s, a);
        } else {
            if (vec) hipLaunchKernelGGL((mlp_bwd_rows_kernel<float, true>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((mlp_bwd_rows_kernel<float, false>), grid, block, 0, s, a);
        }
        if (a.want_w) {
            const dim3 wgrid((unsigned)((a.units + MLP_BWD_WAVES - 1) / MLP_BWD_WAVES));
            if (half) hipLaunchKernelGGL((mlp_bwd_wgrad_kernel<_Float16>), wgrid, block, 0, s, a);
            else hipLaunchKernelGGL((mlp_bwd_wgrad_kernel<float>), wgrid, block, 0, s, a);
        }
    }
    if (a.want_w)
        hipLaunchKernelGGL(mlp_bwd_reduce_kernel, dim3((z.tw + z.tb + 255) / 256), dim3(256), 0, s, a.part, z.pstride, slices, z.tw, z.tb, dw, db);
    HIP_TRY(hipGetLastError(), "mlp heads bwd launch");
    return 0;
}
