// radix_sort.hip -- the stable LSD radix sort of (key, value) pairs (protocol: radix_sort.h), the one-workgroup scan, the Morton order.
#include "common.h"
#include "host_api.h"

__device__ __forceinline__ uint32_t digit_of(uint32_t key, int shift, uint32_t mask) { return (key >> shift) & mask; }

// Geometry of a sort of n pairs: ceil(n / per) blocks, each owning `per` consecutive elements (a multiple of the 2048-element sub-tile)
static uint32_t sort_per_block(uint32_t n)
{
    uint32_t nb = (n + SORT_TILE - 1) / SORT_TILE;
    if (nb > SORT_MAX_BLOCKS) nb = SORT_MAX_BLOCKS;
    if (nb == 0) nb = 1;
    uint32_t per = (n + nb - 1) / nb;
    per = (per + SORT_TILE - 1) / SORT_TILE * SORT_TILE;
    return per ? per : SORT_TILE;
}

// ---- single-block exclusive scan (in place) of up to a few 100k uint32 (instance counts per 256 Gaussians, chunks per anchor, ...) ----
__global__ void __launch_bounds__(1024)
exclusive_scan_kernel(uint32_t* __restrict__ data, uint32_t n, uint32_t* __restrict__ total)
{
    __shared__ uint32_t wave_sums[16];
    __shared__ uint32_t carry_s;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const uint32_t per = (n + 1023) / 1024;
    const uint32_t beg = min(n, tid * per), end = min(n, beg + per);
    uint32_t sum = 0;
    for (uint32_t i = beg; i < end; i++) sum += data[i];
    uint32_t v = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { uint32_t t = __shfl_up(v, off, 64); if (lane >= (uint32_t)off) v += t; }
    if (lane == 63) wave_sums[wid] = v;
    __syncthreads();
    if (tid == 0) { uint32_t c = 0; for (int w = 0; w < 16; w++) { uint32_t t = wave_sums[w]; wave_sums[w] = c; c += t; } carry_s = c; }
    __syncthreads();
    uint32_t run = v - sum + wave_sums[wid];
    for (uint32_t i = beg; i < end; i++) { uint32_t t = data[i]; data[i] = run; run += t; }
    if (total && tid == 0) *total = carry_s;
}

// ---- per-block digit histogram for the passes after the first (LDS atomics absorb low-entropy digits) ----
__global__ void __launch_bounds__(256)
radix_hist_kernel(const uint32_t* __restrict__ keys, uint32_t n, uint32_t per_block, int shift, uint32_t mask, uint32_t* __restrict__ hist)
{
    __shared__ uint32_t h[RADIX];
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t beg = blockIdx.x * per_block;
    const uint32_t end = min(n, beg + per_block);
    for (uint32_t e = beg + threadIdx.x; e < end; e += 256) atomicAdd(&h[digit_of(keys[e], shift, mask)], 1u);
    __syncthreads();
    hist[blockIdx.x * RADIX + threadIdx.x] = h[threadIdx.x];
}

// ---- one stable radix pass ----
// hist_cur[b * 256 + d] = number of keys with digit d in block b's slice (for the first pass it was accumulated with
// atomics by the kernel that PRODUCED the keys -- radix_sort.h: radix_count_first --, for later passes stored by radix_hist_kernel).
// There is no scan launch: every block derives its digit bases from the table itself, then ranks its keys stably
// (wave-level match-any + per-wave LDS counters) and scatters.
__global__ void __launch_bounds__(256)
radix_scatter_kernel(const uint32_t* __restrict__ keys_in, const uint32_t* __restrict__ vals_in, uint32_t* __restrict__ keys_out,
                     uint32_t* __restrict__ vals_out, uint32_t n, uint32_t per_block, int shift, uint32_t mask,
                     const uint32_t* __restrict__ hist_cur)
{
    __shared__ uint32_t wave_cnt[4][RADIX];
    __shared__ uint32_t base[RADIX];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    {   // base[d] = (keys with a smaller digit, all blocks) + (keys with digit d in earlier blocks)
        // wave w sums the rows b = w, w+4, ... of the table, 4 digits (16 B) per lane, several rows in flight
        const uint32_t nb = gridDim.x, me = blockIdx.x;
        uint4 tot = make_uint4(0, 0, 0, 0), bef = make_uint4(0, 0, 0, 0);
        const uint4* tab = (const uint4*)hist_cur;
#pragma unroll 4
        for (uint32_t b = wid; b < nb; b += 4) {
            const uint4 c = tab[b * (RADIX / 4) + lane];
            tot.x += c.x; tot.y += c.y; tot.z += c.z; tot.w += c.w;
            if (b < me) { bef.x += c.x; bef.y += c.y; bef.z += c.z; bef.w += c.w; }
        }
        // wave_cnt[w][0..255] <- totals, base (via a second pass) <- befores
        ((uint4*)wave_cnt[wid])[lane] = tot;
        __syncthreads();
        const uint32_t total = wave_cnt[0][tid] + wave_cnt[1][tid] + wave_cnt[2][tid] + wave_cnt[3][tid];
        __syncthreads();
        ((uint4*)wave_cnt[wid])[lane] = bef;
        __syncthreads();
        const uint32_t before = wave_cnt[0][tid] + wave_cnt[1][tid] + wave_cnt[2][tid] + wave_cnt[3][tid];
        // exclusive scan of `total` over the 256 digits
        uint32_t v = total;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const uint32_t t = __shfl_up(v, off, 64); if (lane >= (uint32_t)off) v += t; }
        __syncthreads();
        if (lane == 63) base[wid] = v;
        __syncthreads();
        uint32_t woff = 0;
        for (uint32_t w = 0; w < wid; w++) woff += base[w];
        __syncthreads();
        base[tid] = (v - total) + woff + before;
    }
    const uint32_t beg = blockIdx.x * per_block;
    const uint32_t end = min(n, beg + per_block);
    for (uint32_t sub = beg; sub < end; sub += SORT_TILE) {
        __syncthreads();
#pragma unroll
        for (int w = 0; w < 4; w++) wave_cnt[w][tid] = 0;
        __syncthreads();
        uint32_t key[SORT_ITEMS], val[SORT_ITEMS], rank[SORT_ITEMS];
        const uint32_t e0 = sub + wid * (SORT_ITEMS * 64) + lane;
#pragma unroll
        for (int i = 0; i < SORT_ITEMS; i++) {
            const uint32_t e = e0 + i * 64;
            const bool valid = e < end;
            key[i] = valid ? keys_in[e] : 0xFFFFFFFFu;
            val[i] = valid ? vals_in[e] : 0u;
        }
#pragma unroll
        for (int i = 0; i < SORT_ITEMS; i++) {
            const uint32_t e = e0 + i * 64;
            const bool valid = e < end;
            const uint32_t d = digit_of(key[i], shift, mask);
            uint64_t peers = __ballot(valid);
#pragma unroll
            for (int b = 0; b < 8; b++) {
                const bool bit = (d >> b) & 1u;
                const uint64_t bal = __ballot(bit);
                peers &= bit ? bal : ~bal;
            }
            const uint32_t r = __popcll(peers & lt_mask);
            uint32_t old = 0;
            if (valid) {
                old = wave_cnt[wid][d];                       // every peer reads before the leader updates
                if (r == 0) wave_cnt[wid][d] = old + __popcll(peers);
            }
            rank[i] = old + r;
        }
        __syncthreads();
        {   // digit `tid`: turn per-wave counts into per-wave bases, advance the running base
            uint32_t run = base[tid];
#pragma unroll
            for (int w = 0; w < 4; w++) { const uint32_t t = wave_cnt[w][tid]; wave_cnt[w][tid] = run; run += t; }
            base[tid] = run;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < SORT_ITEMS; i++) {
            const uint32_t e = e0 + i * 64;
            if (e < end) {
                const uint32_t pos = wave_cnt[wid][digit_of(key[i], shift, mask)] + rank[i];
                keys_out[pos] = key[i];
                vals_out[pos] = val[i];
            }
        }
    }
}

hipError_t radix_sort_begin(hipStream_t s, uint32_t n, RadixBufs& b, int rounds)
{
    b.per_block = sort_per_block(n);
    return zero_fill_async(s, b.hist, (size_t)(rounds - 1) * radix_hist_bytes() + radix_table_bytes());
}

// b.hist: table 0 already holds the first pass's histogram, accumulated by the kernel that wrote b.ka; tables 1.. are written here.
// One pass per 8 key bits swaps the pairs, so the result ends where radix_lands_in_b(bit_hi - bit_lo) says.
hipError_t radix_sort_pairs(hipStream_t s, uint32_t n, const RadixBufs& b, int bit_lo, int bit_hi)
{
    uint32_t *kin = b.ka, *kout = b.kb, *vin = b.va, *vout = b.vb;
    if (n > 0) {
        const uint32_t per = b.per_block, nb = (n + per - 1) / per;      // (radix_sort_begin set it)
        int pass = 0;
        for (int lo = bit_lo; lo < bit_hi; lo += 8, pass++) {
            const int nbits = (bit_hi - lo) < 8 ? (bit_hi - lo) : 8;
            const uint32_t mask = (1u << nbits) - 1u;
            uint32_t* hcur = b.hist + (size_t)pass * RADIX * SORT_MAX_BLOCKS;
            if (pass > 0) hipLaunchKernelGGL(radix_hist_kernel, dim3(nb), dim3(256), 0, s, kin, n, per, lo, mask, hcur);
            hipLaunchKernelGGL(radix_scatter_kernel, dim3(nb), dim3(256), 0, s, kin, vin, kout, vout, n, per, lo, mask, hcur);
            uint32_t* t = kin; kin = kout; kout = t;
            t = vin; vin = vout; vout = t;
        }
    }
    return hipGetLastError();
}
hipError_t launch_exclusive_scan(hipStream_t s, int n, uint32_t* data)
{
    hipLaunchKernelGGL(exclusive_scan_kernel, dim3(1), dim3(1024), 0, s, data, (uint32_t)n, (uint32_t*)nullptr);
    return hipGetLastError();
}

// ---- Morton (Z-order) ordering of the Gaussians' positions (GaussianParams.spatial_sort; no reference counterpart: the binning
// stage reserves its slots per (workgroup, tile), which pays when consecutive Gaussians project to neighbouring tiles) ----------
// key = 3 x `bits` interleaved bits of the position quantised inside the bounding box lohi = {lo.xyz, hi.xyz} (device memory: no
// host read-back); written with the identity permutation and the first radix pass's per-block histogram, then sorted by the
// library's own stable LSD radix sort -- the order torch.argsort(code, stable=True) gives.
__device__ __forceinline__ uint32_t spread3(uint32_t v)
{
    v = (v | (v << 16)) & 0x30000FFu;
    v = (v | (v << 8)) & 0x300F00Fu;
    v = (v | (v << 4)) & 0x30C30C3u;
    return (v | (v << 2)) & 0x9249249u;
}
__global__ void __launch_bounds__(256)
morton_keys_kernel(int P, const float* __restrict__ xyz, const float* __restrict__ lohi, int bits, uint32_t* __restrict__ keys,
                   uint32_t* __restrict__ vals, uint32_t* __restrict__ hist0, uint32_t per_block)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const float top = (float)((1u << bits) - 1u);
    uint32_t q[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float lo = lohi[k], ext = fmaxf(lohi[3 + k] - lo, 1e-12f);
        const float t = (xyz[3 * (size_t)i + k] - lo) / ext * top;          // (same expression, same order as the PyTorch form it replaces)
        const long long v = (long long)t;                                     // truncation towards zero, as .long()
        q[k] = (uint32_t)(v < 0 ? 0 : (v > (long long)top ? (long long)top : v));
    }
    const uint32_t code = spread3(q[0]) | (spread3(q[1]) << 1) | (spread3(q[2]) << 2);
    keys[i] = code; vals[i] = (uint32_t)i;
    radix_count_first(hist0, (uint32_t)i, per_block, code);
}
static size_t morton_scratch_bytes(int P) { size_t o = 0; radix_layout_append(o, (size_t)(P > 0 ? P : 0)); return o + 256; }
static hipError_t launch_morton_order(hipStream_t s, int P, const float* xyz, const float* lohi, int bits, void* scratch, int* perm)
{
    size_t o = 0;
    RadixBufs b = radix_layout_append(o, (size_t)P).at(align_ptr((const char*)scratch));
    hipError_t e = radix_sort_begin(s, (uint32_t)P, b);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(morton_keys_kernel, dim3((P + 255) / 256), dim3(256), 0, s, P, xyz, lohi, bits, b.ka, b.va, b.hist, b.per_block);
    e = radix_sort_pairs(s, (uint32_t)P, b, 0, 3 * bits);
    if (e != hipSuccess) return e;
    return hipMemcpyAsync(perm, b.sorted_vals(3 * bits), (size_t)P * 4, hipMemcpyDeviceToDevice, s);
}
// The entry points (contract in include/igs_rast.h): perm[i] = index of the Gaussian that comes i-th along the Z-order curve of
// xyz quantised to `bits` bits per axis inside the box lohi = {lo.x, lo.y, lo.z, hi.x, hi.y, hi.z} (device memory).
extern "C" size_t igs_morton_order_scratch_bytes(int P) { return morton_scratch_bytes(P) + 256; }
extern "C" int igs_morton_order(void* stream, int P, const float* xyz, const float* lohi, int bits, void* scratch, int* perm)
{
    if (P < 0 || bits < 1 || bits > 10) return fail(IGS_RAST_E_INVALID, "igs_morton_order: bad sizes (1..10 bits per axis)");
    if (P == 0) return 0;
    if (!xyz || !lohi || !scratch || !perm) return fail(IGS_RAST_E_INVALID, "igs_morton_order: NULL pointer");
    HIP_TRY(launch_morton_order((hipStream_t)stream, P, xyz, lohi, bits, scratch, perm), "morton order launch");
    return 0;
}
