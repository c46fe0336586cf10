// blend_count.hip -- the count pass of the compress rasterizer (count_gaussians), gfx950 (wave64).
// Replaces renderCUDA_count (compress-diff-gaussian-rasterization cuda_rasterizer/forward.cu:379-503): the colour-only front-to-back
// blend of blend_fwd_tile.h, plus, per Gaussian, the number of image pixels it is blended into.
//
// The reference increments gaussian_count[id] / important_score[id] with plain read-modify-writes from 256 threads at once (racy: it
// undercounts).  Here the count is exact and the score is count x opacity, written once by a finishing pass over P (deterministic):
//   * a quad's contributing lanes for one splat are one ballot popcount (wave-uniform), stored into LDS by lane 0 of that wave;
//   * the four quads of the tile meet in LDS: when the tile stages its next chunk (or leaves), the thread that staged a splat sums its
//     four quad counts and issues ONE relaxed, agent-scope integer add per (tile, splat) with a nonzero count.
// Integer adds commute, so the counts do not depend on the order the atomics land in.
#include "blend_fwd_tile.h"

__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8)))
blend_count_kernel(const BlendFwdArgs a, int* __restrict__ count)
{
    constexpr int NQ = 3;                                   // float4 per staged record: xy, conic, opacity, rgb
    __shared__ float4 chunk[FWD_CHUNK * NQ];
    __shared__ uint64_t quad_bits[FWD_NLIST][FWD_NSW];      // [quad][staging wave]
    __shared__ int wave_done[4];
    __shared__ uint32_t hits[4][FWD_CHUNK];                 // [quad][staged splat]: pixels of that quad the splat was blended into

    if (blockIdx.x == 0 && threadIdx.x == 0 && a.host_dst) {
        // slab binning: {R, overflow, prefilter flag}, then the sequence word the host polls (as in blend_fwd.hip)
        __hip_atomic_store(&a.host_dst[0], a.stats_src[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&a.host_dst[1], a.stats_src[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&a.host_dst[2], a.flag_src[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(&a.host_dst[3], a.host_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    uint32_t tile;
    if (!tile_for_block(blockIdx.x, a.gx, a.gy, tile)) return;

    const uint32_t tx = tile % a.gx, ty = tile / a.gx;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const uint32_t px = tx * TILE + (wid & 1) * 8 + (lane & 7);
    const uint32_t py = ty * TILE + (wid >> 1) * 8 + (lane >> 3);
    const bool inside = px < (uint32_t)a.W && py < (uint32_t)a.H;
    const float pixfx = (float)px, pixfy = (float)py;      // pixf = pix (no +0.5), forward.cu:399
    const float tile_x0 = (float)(tx * TILE), tile_y0 = (float)(ty * TILE);

    const uint2 range = ((const uint2*)a.ranges)[tile];
    const int n = (int)(range.y - range.x);      // (a tile that overflowed its slab has an empty range; the frame is then redone)
    const int rounds = (n + FWD_CHUNK - 1) / FWD_CHUNK;

    float T = 1.0f;
    float Tl = inside ? 1.0f : 0.0f;      // live transmittance: T while the pixel still takes splats, 0 once it is finished / outside
    float C0 = 0, C1 = 0, C2 = 0;
    uint32_t staged_id = 0xFFFFFFFFu;     // the Gaussian this thread staged into the current chunk (none: all ones)

    // the staging thread's share of the count: the four quads' pixels for its splat, one global add if any
    auto flush = [&]() {
        if (staged_id != 0xFFFFFFFFu) {
            const uint32_t c = hits[0][tid] + hits[1][tid] + hits[2][tid] + hits[3][tid];
            if (c) __hip_atomic_fetch_add(&count[staged_id], (int)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            staged_id = 0xFFFFFFFFu;
        }
    };

    if (tid < 4) wave_done[tid] = 0;
    for (int i = 0; i < rounds; i++) {
        wg_barrier();                                           // previous chunk consumed (and its hits written), wave_done published
        flush();
        if (wave_done[0] & wave_done[1] & wave_done[2] & wave_done[3]) break;
        const int progress = i * FWD_CHUNK + (int)tid;
        uint32_t qmask = 0;
        if (tid < FWD_CHUNK) {
            hits[0][tid] = 0u; hits[1][tid] = 0u; hits[2][tid] = 0u; hits[3][tid] = 0u;
            if (progress < n) {
                const uint32_t id = a.point_list[range.x + progress];
                const float4* src = (const float4*)(a.rec + (size_t)id * REC_F);
                float4 q0 = src[0], q1 = src[1], q2 = src[2];
                if (a.colors_precomp) {                           // features = colors_precomp (rasterizer_impl.cu forwardCount)
                    q1.z = a.colors_precomp[3 * (size_t)id]; q1.w = a.colors_precomp[3 * (size_t)id + 1];
                    q2.x = a.colors_precomp[3 * (size_t)id + 2];
                }
                chunk[tid * NQ + 0] = q0; chunk[tid * NQ + 1] = q1; chunk[tid * NQ + 2] = q2;
                qmask = quad_reach_mask(q0, q1, tile_x0, tile_y0);
                staged_id = id;
            }
        }
        if (wid < FWD_NSW) {
#pragma unroll
            for (int q = 0; q < FWD_NLIST; q++) {
                const uint64_t b = __ballot((qmask >> q) & 1u);
                if (lane == 0) quad_bits[q][wid] = b;
            }
        }
        wg_barrier();
        if (__ballot(Tl != 0.0f) != 0ull) {
            bool wave_finished = false;
            for (int sw = 0; sw < FWD_NSW && !wave_finished; sw++) {
                uint64_t bits = uniform64(quad_bits[wid][sw]);     // wave-uniform
                while (bits != 0ull) {
                    const int jj = __builtin_ctzll(bits);
                    asm("s_bitset0_b64 %0, %1" : "+s"(bits) : "s"(jj));
                    const int j = sw * 64 + jj;
                    uint32_t addr;                                  // LDS byte offset of the record
                    asm("v_mul_u32_u24 %0, %1, %2" : "=v"(addr) : "s"(j), "n"(NQ * 16));
                    const float4* r = (const float4*)((const char*)chunk + addr);
                    const float4 q0 = r[0], q1 = r[1], q2 = r[2];
                    const float dx = q0.x - pixfx, dy = q0.y - pixfy;
                    const float power = gauss_power(q0.z, q0.w, q1.x, dx, dy);
                    const float alpha = fminf(0.99f, q1.y * __expf(power));
                    // forward.cu:470-487 without boolean state (blend_fwd_tile.h: blend_row): a skipped splat blends with alpha 0, a
                    // finished pixel has Tl = 0; the splat is blended (and counted) iff alpha T > 0
                    const float alpha_e = (!(power > 0.0f) && !(alpha < 1.0f / 255.0f)) ? alpha : 0.0f;
                    const float test_T = Tl * (1.0f - alpha_e);
                    const bool alive = !(test_T < 0.0001f);
                    const float aT = alive ? alpha_e * Tl : 0.0f;
                    C0 += q1.z * aT; C1 += q1.w * aT; C2 += q2.x * aT;
                    T = alive ? test_T : T;
                    Tl = alive ? test_T : 0.0f;
                    const uint32_t c = (uint32_t)__popcll(__ballot(aT > 0.0f));       // scalar: this quad's pixels for splat j
                    if (lane == 0 && c) hits[wid][j] = c;
                }
                if (__ballot(Tl != 0.0f) == 0ull) wave_finished = true;
            }
        }
        const bool all_done = __ballot(Tl != 0.0f) == 0ull;
        if (lane == 0) wave_done[wid] = all_done ? 1 : 0;
    }
    wg_barrier();                                               // the last chunk's hits (a no-op for a tile that left early)
    flush();

    if (inside) {
        const size_t HW = (size_t)a.H * a.W;
        const size_t pix = (size_t)a.W * py + px;
        a.out_color[pix] = C0 + T * a.bg[0];
        a.out_color[HW + pix] = C1 + T * a.bg[1];
        a.out_color[2 * HW + pix] = C2 + T * a.bg[2];
    }
}

hipError_t launch_blend_count(hipStream_t s, const BlendFwdArgs& a, int* count)
{
    hipLaunchKernelGGL(blend_count_kernel, dim3(tile_grid_blocks(a.gx, a.gy)), dim3(256), 0, s, a, count);
    return hipGetLastError();
}

// important_score = count x opacity, rounded once (the reference adds opacity[id] once per counted pixel: the same value up to its
// float accumulation error)
__global__ void __launch_bounds__(256) count_score_kernel(int P, const int* __restrict__ count, const float* __restrict__ opacities,
                                                          float* __restrict__ score)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < P) score[i] = (float)count[i] * opacities[i];
}

hipError_t launch_count_score(hipStream_t s, int P, const int* count, const float* opacities, float* score)
{
    hipLaunchKernelGGL(count_score_kernel, dim3((P + 255) / 256), dim3(256), 0, s, P, count, opacities, score);
    return hipGetLastError();
}
