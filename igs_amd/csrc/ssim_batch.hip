// ssim_batch.hip -- SSIM (and L1) of a BATCH of images, forward + backward, for the AGM-Net training loss, gfx950.
//   loss = lambda_rgb * mean|x - y| + lambda_ssim * (1 - mean SSIM(x, y))          (main.py:252-265; x, y: [B V, 3, H, W])
// SSIM as igs/utils/loss_utils.py:33-63 (11x11 Gaussian window, sigma 1.5, zero padding 5, C1 = 0.01^2, C2 = 0.03^2); the kernels are
// those of loss_ops.hip (ssim_stats_kernel<GT_INLINE>, ssim_grad_body: same tile, halo, separable register-blocked blur and the same
// algebra, see the header of that file) over planes = images * channels planes, with what a batch needs:
//   - a value per image.  Every workgroup leaves the sum of its tile in scratch (part[plane][tile row][tile col]); no atomics and no
//     hand-off between workgroups inside a launch.  ssim_batch_finish_kernel, one workgroup behind the others, adds the partial sums of
//     every image in an order that depends on (channels, width, height) alone, so an image's value has the same bits alone and at any
//     position of any batch, and two runs agree bit for bit;
//   - instances by what is wanted: the three derivative maps only with a gradient, the SSIM map only when asked for, the L1 sum in the
//     stats kernel only when there is no gradient launch to carry it (the same pixels per thread in the same order: the same bits).
//     Every product-sum of the blurs is an explicit fmaf and the value of a pixel is formed with contraction off, so the instances
//     cannot round a shared expression differently.
// Launches: stats, grad, finish with a gradient; stats, finish without.  All offsets are 64-bit.
#include "common.h"
#include "host_api.h"
#include "ssim_common.h"

// sum of `v` over the 256 threads of the workgroup in a fixed order (wave tree, then the four waves in index order); called by all
// threads, the result is valid in thread 0.  `red`: 4 floats of LDS of this call's own
__device__ __forceinline__ float tile_sum(float v, float* red)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// DERIV: write the three derivative maps (maps [planes][3][H][W]);  MAP: write the SSIM value of every pixel (ssim_map [planes][H][W]);
// L1: also leave the tile's sum of |x - y| in part_l1 (forward-only calls: no gradient launch follows)
template <bool DERIV, bool MAP, bool L1>
__global__ void __launch_bounds__(256)
ssim_batch_stats_kernel(const SsimWin win, int W, int H, unsigned planes, const float* __restrict__ x, const float* __restrict__ y,
                        float* __restrict__ maps, float* __restrict__ ssim_map, float* __restrict__ part_ssim, float* __restrict__ part_l1)
{
    // LDS as ssim_stats_kernel<GT_INLINE>: the halo of x and y, blurred in place, and three planes of their own (x x, y y, x y)
    __shared__ __attribute__((aligned(16))) float sx[SSIM_H][SSIM_HS], sy[SSIM_H][SSIM_HS];
    __shared__ __attribute__((aligned(16))) float hbx[3][SSIM_H][SSIM_BS];
    __shared__ float red[8];
    const unsigned gxt = (unsigned)(W + SSIM_T - 1) / SSIM_T, gyt = (unsigned)(H + SSIM_T - 1) / SSIM_T;
    unsigned bx, by, bz;
    if (!band_tile(blockIdx.x, gxt, gyt, planes, bx, by, bz)) return;
    const int tid = threadIdx.x;
    const int x0 = (int)bx * SSIM_T - SSIM_R, y0 = (int)by * SSIM_T - SSIM_R;
    const size_t HW = (size_t)W * H;
    const float* xc = x + (size_t)bz * HW; const float* yc = y + (size_t)bz * HW;
    {
        // halo load: every global load of the tile is issued before the first one is waited for
        constexpr int NIT = (SSIM_H * SSIM_H + 255) / 256;
        float tx[NIT], ty[NIT];
#pragma unroll
        for (int it = 0; it < NIT; it++) {
            const int i = tid + it * 256;
            const int r = i / SSIM_H, q = i - r * SSIM_H;
            const int gx = x0 + q, gy = y0 + r;
            const bool in = i < SSIM_H * SSIM_H && gx >= 0 && gx < W && gy >= 0 && gy < H;      // zero padding (F.conv2d padding=5)
            const size_t o = in ? (size_t)gy * W + gx : 0;
            const float a = xc[o], b = yc[o];
            tx[it] = in ? a : 0.f; ty[it] = in ? b : 0.f;
        }
#pragma unroll
        for (int it = 0; it < NIT; it++) {
            const int i = tid + it * 256;
            if (i < SSIM_H * SSIM_H) { const int r = i / SSIM_H, q = i - r * SSIM_H; sx[r][q] = tx[it]; sy[r][q] = ty[it]; }
        }
    }
    __syncthreads();
    // horizontal: work item = (halo row r, group of 8 output columns): 42 x 4 = 168 items; consecutive lanes = consecutive rows
    const bool hitem = tid < SSIM_H * (SSIM_T / 8);
    const int hqg = tid / SSIM_H, hr = hitem ? tid - hqg * SSIM_H : 0, hq = hitem ? hqg * 8 : 0;
    float o0[8], o1[8], o2[8], o3[8], o4[8];              // blur of x, y, x x, y y, x y at the item's eight columns
    if (hitem) {
        float u[20], v[20], uu[18], vv[18], uv[18];
#pragma unroll
        for (int k = 0; k < 5; k++) {
            const float4 a = *(const float4*)&sx[hr][hq + 4 * k], b = *(const float4*)&sy[hr][hq + 4 * k];
            u[4 * k] = a.x; u[4 * k + 1] = a.y; u[4 * k + 2] = a.z; u[4 * k + 3] = a.w;
            v[4 * k] = b.x; v[4 * k + 1] = b.y; v[4 * k + 2] = b.z; v[4 * k + 3] = b.w;
        }
#pragma unroll
        for (int k = 0; k < 18; k++) { uu[k] = u[k] * u[k]; vv[k] = v[k] * v[k]; uv[k] = u[k] * v[k]; }
#pragma unroll
        for (int o = 0; o < 8; o++) {
            o0[o] = 0.f; o1[o] = 0.f; o2[o] = 0.f; o3[o] = 0.f; o4[o] = 0.f;
#pragma unroll
            for (int k = 0; k <= 2 * SSIM_R; k++) {
                const float w = win.g[k]; const int j = o + k;
                o0[o] = fmaf(w, u[j], o0[o]); o1[o] = fmaf(w, v[j], o1[o]); o2[o] = fmaf(w, uu[j], o2[o]);
                o3[o] = fmaf(w, vv[j], o3[o]); o4[o] = fmaf(w, uv[j], o4[o]);
            }
        }
    }
    __syncthreads();                                      // every thread has its rows in registers: the halo rows may be overwritten
    // plane -> storage: blur(x) in sx, blur(y) in sy, x x / y y / x y in hbx[0..2]
    if (hitem) {
#pragma unroll
        for (int h = 0; h < 2; h++) {
            *(float4*)&sx[hr][hq + 4 * h] = make_float4(o0[4 * h], o0[4 * h + 1], o0[4 * h + 2], o0[4 * h + 3]);
            *(float4*)&sy[hr][hq + 4 * h] = make_float4(o1[4 * h], o1[4 * h + 1], o1[4 * h + 2], o1[4 * h + 3]);
            *(float4*)&hbx[0][hr][hq + 4 * h] = make_float4(o2[4 * h], o2[4 * h + 1], o2[4 * h + 2], o2[4 * h + 3]);
            *(float4*)&hbx[1][hr][hq + 4 * h] = make_float4(o3[4 * h], o3[4 * h + 1], o3[4 * h + 2], o3[4 * h + 3]);
            *(float4*)&hbx[2][hr][hq + 4 * h] = make_float4(o4[4 * h], o4[4 * h + 1], o4[4 * h + 2], o4[4 * h + 3]);
        }
    }
    __syncthreads();
    // vertical: work item = (column lx, group of 4 output rows)
    const int lx = tid & 31, ly = (tid >> 5) * 4;
    const int px = (int)bx * SSIM_T + lx;
    float m1[4] = { 0, 0, 0, 0 }, m2[4] = { 0, 0, 0, 0 }, e1[4] = { 0, 0, 0, 0 }, e2[4] = { 0, 0, 0, 0 }, e12[4] = { 0, 0, 0, 0 };
#pragma unroll
    for (int k = 0; k < 14; k++) {
        const float h0 = sx[ly + k][lx], h1 = sy[ly + k][lx], h2 = hbx[0][ly + k][lx], h3 = hbx[1][ly + k][lx], h4 = hbx[2][ly + k][lx];
#pragma unroll
        for (int o = 0; o < 4; o++) {
            if (k - o >= 0 && k - o <= 2 * SSIM_R) {
                const float w = win.g[k - o];
                m1[o] = fmaf(w, h0, m1[o]); m2[o] = fmaf(w, h1, m2[o]); e1[o] = fmaf(w, h2, e1[o]);
                e2[o] = fmaf(w, h3, e2[o]); e12[o] = fmaf(w, h4, e12[o]);
            }
        }
    }
    float* mc = DERIV ? maps + (size_t)bz * 3 * HW : nullptr;
    float val = 0.f, l1 = 0.f;
#pragma unroll
    for (int o = 0; o < 4; o++) {
        const int py = (int)by * SSIM_T + ly + o;
        if (px < W && py < H) {
#pragma clang fp contract(off)
            const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
            const float m1s = m1[o] * m1[o], m2s = m2[o] * m2[o], m12 = m1[o] * m2[o];
            const float s1 = e1[o] - m1s, s2 = e2[o] - m2s, s12 = e12[o] - m12;
            const float A = 2.f * m12 + C1, B = 2.f * s12 + C2, Cc = m1s + m2s + C1, D = s1 + s2 + C2;
            const float inv_cd = 1.f / (Cc * D);
            const float s = A * B * inv_cd;
            val += s;
            const size_t off = (size_t)py * W + px;
            if constexpr (MAP) ssim_map[(size_t)bz * HW + off] = s;
            if constexpr (DERIV) {
                mc[off] = 2.f * m2[o] * (B - A) * inv_cd - 2.f * m1[o] * A * B * (D - Cc) * inv_cd * inv_cd;     // d/d blur(x)
                mc[HW + off] = -A * B * inv_cd / D;                                                              // d/d blur(xx)
                mc[2 * HW + off] = 2.f * A * inv_cd;                                                             // d/d blur(xy)
            }
            if constexpr (L1) l1 += fabsf(xc[off] - yc[off]);
        }
    }
    const size_t slot = ((size_t)bz * gyt + by) * gxt + bx;
    const float tile_val = tile_sum(val, red);
    if (tid == 0) part_ssim[slot] = tile_val;
    if constexpr (L1) {
        const float tile_l1 = tile_sum(l1, red + 4);
        if (tid == 0) part_l1[slot] = tile_l1;
    }
}

// the adjoint (ssim_grad_body): the same separable blur of the three derivative maps, combined with x and y into
//   grad = k_ssim * d(sum SSIM of the plane)/dx + k_l1 * sign(x - y),   every element written;
// part_l1 (NULL = not wanted): the tile's sum of |x - y|
__global__ void __launch_bounds__(256)
ssim_batch_grad_kernel(const SsimWin win, int W, int H, unsigned planes, const float* __restrict__ x, const float* __restrict__ y,
                       const float* __restrict__ maps, float k_ssim, float k_l1, float* __restrict__ grad, float* __restrict__ part_l1)
{
    __shared__ __attribute__((aligned(16))) float sm[3][SSIM_H][SSIM_HS];
    __shared__ float red[4];
    const unsigned gxt = (unsigned)(W + SSIM_T - 1) / SSIM_T, gyt = (unsigned)(H + SSIM_T - 1) / SSIM_T;
    unsigned bx, by, bz;
    if (!band_tile(blockIdx.x, gxt, gyt, planes, bx, by, bz)) return;
    const int tid = threadIdx.x;
    const int x0 = (int)bx * SSIM_T - SSIM_R, y0 = (int)by * SSIM_T - SSIM_R;
    const size_t HW = (size_t)W * H;
    const float* mc = maps + (size_t)bz * 3 * HW;
    {
        constexpr int NIT = (SSIM_H * SSIM_H + 255) / 256;
        float t0[NIT], t1[NIT], t2[NIT];
#pragma unroll
        for (int it = 0; it < NIT; it++) {
            const int i = tid + it * 256;
            const int r = i / SSIM_H, q = i - r * SSIM_H;
            const int gx = x0 + q, gy = y0 + r;
            const bool in = i < SSIM_H * SSIM_H && gx >= 0 && gx < W && gy >= 0 && gy < H;      // no SSIM value exists outside the image
            const size_t o = in ? (size_t)gy * W + gx : 0;
            const float a = mc[o], b = mc[HW + o], d = mc[2 * HW + o];
            t0[it] = in ? a : 0.f; t1[it] = in ? b : 0.f; t2[it] = in ? d : 0.f;
        }
#pragma unroll
        for (int it = 0; it < NIT; it++) {
            const int i = tid + it * 256;
            if (i < SSIM_H * SSIM_H) { const int r = i / SSIM_H, q = i - r * SSIM_H; sm[0][r][q] = t0[it]; sm[1][r][q] = t1[it]; sm[2][r][q] = t2[it]; }
        }
    }
    __syncthreads();
    const bool hitem = tid < SSIM_H * (SSIM_T / 8);
    const int hqg = tid / SSIM_H, hr = hitem ? tid - hqg * SSIM_H : 0, hq = hitem ? hqg * 8 : 0;
    float hacc[3][8];
    if (hitem) {
#pragma unroll
        for (int m = 0; m < 3; m++) {
            float u[20];
#pragma unroll
            for (int k = 0; k < 5; k++) {
                const float4 a = *(const float4*)&sm[m][hr][hq + 4 * k];
                u[4 * k] = a.x; u[4 * k + 1] = a.y; u[4 * k + 2] = a.z; u[4 * k + 3] = a.w;
            }
#pragma unroll
            for (int o = 0; o < 8; o++) {
                hacc[m][o] = 0.f;
#pragma unroll
                for (int k = 0; k <= 2 * SSIM_R; k++) hacc[m][o] = fmaf(win.g[k], u[o + k], hacc[m][o]);
            }
        }
    }
    __syncthreads();                                      // all reads of the halo rows are done: overwrite them
    if (hitem) {
#pragma unroll
        for (int m = 0; m < 3; m++)
#pragma unroll
            for (int h = 0; h < 2; h++)
                *(float4*)&sm[m][hr][hq + 4 * h] = make_float4(hacc[m][4 * h], hacc[m][4 * h + 1], hacc[m][4 * h + 2], hacc[m][4 * h + 3]);
    }
    __syncthreads();
    const int lx = tid & 31, ly = (tid >> 5) * 4;
    const int px = (int)bx * SSIM_T + lx;
    float b0[4] = { 0, 0, 0, 0 }, b1[4] = { 0, 0, 0, 0 }, b2[4] = { 0, 0, 0, 0 };
#pragma unroll
    for (int k = 0; k < 14; k++) {
        const float h0 = sm[0][ly + k][lx], h1 = sm[1][ly + k][lx], h2 = sm[2][ly + k][lx];
#pragma unroll
        for (int o = 0; o < 4; o++) {
            if (k - o >= 0 && k - o <= 2 * SSIM_R) {
                const float w = win.g[k - o];
                b0[o] = fmaf(w, h0, b0[o]); b1[o] = fmaf(w, h1, b1[o]); b2[o] = fmaf(w, h2, b2[o]);
            }
        }
    }
    float l1 = 0.f;
#pragma unroll
    for (int o = 0; o < 4; o++) {
        const int py = (int)by * SSIM_T + ly + o;
        if (px < W && py < H) {
            const size_t off = (size_t)bz * HW + (size_t)py * W + px;
            const float xv = x[off], yv = y[off], d = xv - yv;
            l1 += fabsf(d);
            const float g_l1 = d > 0.f ? k_l1 : (d < 0.f ? -k_l1 : 0.f);
            grad[off] = k_ssim * (b0[o] + 2.f * xv * b1[o] + yv * b2[o]) + g_l1;
        }
    }
    if (part_l1) {                                        // (uniform over the workgroup)
        const float tile_l1 = tile_sum(l1, red);
        if (tid == 0) part_l1[((size_t)bz * gyt + by) * gxt + bx] = tile_l1;
    }
}

// sum of part[0 .. cnt) by one wave in a fixed order: lane l adds elements l, l + 64, ... in groups of eight, then the wave tree.
// The same in every lane of the wave after the call
__device__ __forceinline__ float wave_sum_fixed(const float* __restrict__ part, long long cnt)
{
    const int lane = threadIdx.x & 63;
    float acc = 0.f;
    for (long long i = lane; i < cnt; i += 64 * 8) {
        float a[8];
#pragma unroll
        for (int k = 0; k < 8; k++) { const long long j = i + 64 * k; a[k] = j < cnt ? part[j] : 0.f; }
        acc += ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    return acc;
}
// ONE workgroup of 16 waves behind the tile kernels: wave w finishes images w, w + 16, ...: means[n] = (sum of the image's `per_image`
// partial sums) / n_elems; then thread 0 adds means[0 .. images) in index order: means[images] = that / images.  The same for the L1
// partial sums when wanted
__global__ void __launch_bounds__(1024)
ssim_batch_finish_kernel(int images, long long per_image, float n_elems, const float* __restrict__ part_ssim, const float* __restrict__ part_l1,
                         float* means, float* l1_means)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int n = wave; n < images; n += 16) {
        const float s = wave_sum_fixed(part_ssim + (size_t)n * per_image, per_image);
        if (lane == 0) means[n] = s / n_elems;
        if (l1_means) {
            const float a = wave_sum_fixed(part_l1 + (size_t)n * per_image, per_image);
            if (lane == 0) l1_means[n] = a / n_elems;
        }
    }
    __syncthreads();                                      // (the image means were written by waves of this workgroup)
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int n = 0; n < images; n++) s += ((const volatile float*)means)[n];
        means[images] = s / (float)images;
    }
    if (threadIdx.x == 64 && l1_means) {
        float s = 0.f;
        for (int n = 0; n < images; n++) s += ((const volatile float*)l1_means)[n];
        l1_means[images] = s / (float)images;
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
// scratch = { derivative maps [planes][3][H][W] (want_grad only) | SSIM partial sums [planes][gy][gx] | L1 partial sums [planes][gy][gx] },
// each part on a 256-byte boundary
struct SsimBatchLayout { unsigned gx, gy; unsigned long long planes, tiles, grid; size_t maps, part_ssim, part_l1, total; };
static const char* ssim_batch_size_error(int width, int height, int images, int channels, int want_grad, SsimBatchLayout* L)
{
    if (width <= 0 || height <= 0 || images <= 0 || channels <= 0) return "width, height, images and channels must be positive";
    const unsigned long long planes = (unsigned long long)images * (unsigned long long)channels;
    if (planes > (unsigned long long)IGS_SSIM_BATCH_MAX_PLANES) return "images * channels above IGS_SSIM_BATCH_MAX_PLANES";
    const unsigned long long gx = ((unsigned long long)width + SSIM_T - 1) / SSIM_T, gy = ((unsigned long long)height + SSIM_T - 1) / SSIM_T;
    const unsigned long long grid = 8ull * planes * ((gy + 7) / 8) * gx;
    if (grid > 0x7fffffffull) return "the grid 8 * planes * ceil(tile rows / 8) * tile columns does not fit in 31 bits";
    L->gx = (unsigned)gx; L->gy = (unsigned)gy; L->planes = planes; L->tiles = gx * gy; L->grid = grid;
    const size_t HW = (size_t)width * (size_t)height;
    size_t o = 0;
    L->maps = o;      o += want_grad ? align_up((size_t)planes * 3 * HW * 4, 256) : 0;
    L->part_ssim = o; o += align_up((size_t)(planes * L->tiles) * 4, 256);
    L->part_l1 = o;   o += align_up((size_t)(planes * L->tiles) * 4, 256);
    L->total = o;
    return nullptr;
}

extern "C" long long igs_ssim_batch_scratch_bytes(int width, int height, int images, int channels, int want_grad)
{
    SsimBatchLayout L;
    if (ssim_batch_size_error(width, height, images, channels, want_grad, &L)) return -1;
    return (long long)L.total;
}

template <bool DERIV, bool MAP, bool L1>
static void launch_batch_stats(hipStream_t s, const SsimBatchLayout& L, const SsimWin& win, int W, int H, const float* pred, const float* gt,
                               float* maps, float* ssim_map, float* part_ssim, float* part_l1)
{
    hipLaunchKernelGGL((ssim_batch_stats_kernel<DERIV, MAP, L1>), dim3((unsigned)L.grid), dim3(256), 0, s, win, W, H, (unsigned)L.planes, pred, gt,
                       maps, ssim_map, part_ssim, part_l1);
}

extern "C" int igs_ssim_batch_fwd_bwd(void* stream, int width, int height, int images, int channels, const float* pred, const float* gt,
                                      float c_ssim, float c_l1, void* scratch, float* means, float* l1_means, float* grad, float* ssim_map)
{
    const char* fn = "igs_ssim_batch_fwd_bwd";
    SsimBatchLayout L;
    if (const char* w = ssim_batch_size_error(width, height, images, channels, grad != nullptr, &L)) return fail_in(fn, w);
    if (!pred || !gt || !scratch || !means) return fail_in(fn, "NULL pointer (pred, gt, scratch and means are required)");
    static const SsimWin win = make_window();
    hipStream_t s = (hipStream_t)stream;
    float* maps = (float*)((char*)scratch + L.maps);
    float* part_ssim = (float*)((char*)scratch + L.part_ssim);
    float* part_l1 = l1_means ? (float*)((char*)scratch + L.part_l1) : nullptr;
    const bool deriv = grad != nullptr, map = ssim_map != nullptr, l1_fwd = l1_means && !grad;
    switch ((deriv ? 4 : 0) | (map ? 2 : 0) | (l1_fwd ? 1 : 0)) {
    case 0: launch_batch_stats<false, false, false>(s, L, win, width, height, pred, gt, maps, ssim_map, part_ssim, part_l1); break;
    case 1: launch_batch_stats<false, false, true>(s, L, win, width, height, pred, gt, maps, ssim_map, part_ssim, part_l1); break;
    case 2: launch_batch_stats<false, true, false>(s, L, win, width, height, pred, gt, maps, ssim_map, part_ssim, part_l1); break;
    case 3: launch_batch_stats<false, true, true>(s, L, win, width, height, pred, gt, maps, ssim_map, part_ssim, part_l1); break;
    case 4: launch_batch_stats<true, false, false>(s, L, win, width, height, pred, gt, maps, ssim_map, part_ssim, part_l1); break;
    default: launch_batch_stats<true, true, false>(s, L, win, width, height, pred, gt, maps, ssim_map, part_ssim, part_l1); break;
    }
    HIP_TRY(hipGetLastError(), "igs_ssim_batch_fwd_bwd: stats launch");
    // mean over the C * H * W elements of an image (exact in float up to 2^24 elements, rounded once beyond)
    const float n_elems = (float)((double)channels * (double)width * (double)height);
    if (deriv) {
        hipLaunchKernelGGL(ssim_batch_grad_kernel, dim3((unsigned)L.grid), dim3(256), 0, s, win, width, height, (unsigned)L.planes, pred, gt,
                           (const float*)maps, c_ssim / n_elems, c_l1 / n_elems, grad, part_l1);
        HIP_TRY(hipGetLastError(), "igs_ssim_batch_fwd_bwd: gradient launch");
    }
    hipLaunchKernelGGL(ssim_batch_finish_kernel, dim3(1), dim3(1024), 0, s, images, (long long)((unsigned long long)channels * L.tiles), n_elems,
                       (const float*)part_ssim, (const float*)part_l1, means, l1_means);
    HIP_TRY(hipGetLastError(), "igs_ssim_batch_fwd_bwd: finishing launch");
    return 0;
}
