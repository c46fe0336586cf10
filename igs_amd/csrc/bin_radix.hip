// bin_radix.hip -- global radix binning for gfx950, the slab binning's fallback (api.hip: bin_radix): counts, instance emission, tile ranges.
//
// The reference builds 64-bit (tile | depth) keys for every (Gaussian, tile) instance and sorts all R of them with
// cub::DeviceRadixSort over 32+log2(T) bits (rasterizer_impl.cu:70-111, 373-381): 6 passes over 12-byte pairs at
// 1352x1014.  Here the same ORDER is produced with far less traffic:
//   1. sort the P Gaussians by depth bits (32-bit keys, 4 passes over P pairs);
//   2. emit the instances in that order (coalesced, load-balanced: a block of 256 Gaussians scatters its instances
//      cooperatively instead of one thread looping over its tiles);
//   3. stable-sort the R instances by tile id only (ceil(log2 T / 8) = 2 passes over 8-byte pairs).
// Stability of every pass makes the result identical to a stable sort on (tile, depth) with ties in Gaussian-index
// order, which is what the reference's stable LSD sort yields.
#include "common.h"

// ---- instance counts in depth order: blocksum[b] = sum over sorted positions [256b, 256b+256) of tiles[order[s]] ----
__global__ void __launch_bounds__(256)
count_sorted_kernel(int P, const uint32_t* __restrict__ order, const uint32_t* __restrict__ tiles, uint32_t* __restrict__ blocksum)
{
    __shared__ uint32_t ws[4];
    const int s = blockIdx.x * 256 + threadIdx.x;
    uint32_t v = (s < P) ? tiles[order[s]] : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) blocksum[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}
hipError_t launch_count_sorted(hipStream_t s, int P, const uint32_t* order, const uint32_t* tiles, uint32_t* blocksum)
{
    hipLaunchKernelGGL(count_sorted_kernel, dim3((P + 255) / 256), dim3(256), 0, s, P, order, tiles, blocksum);
    return hipGetLastError();
}

// ---- emission: a block owns 256 depth-consecutive Gaussians and writes all their (tile, id) pairs cooperatively ----
__global__ void __launch_bounds__(256)
emit_instances_kernel(int P, int gx, int gy, const uint32_t* __restrict__ order, const uint32_t* __restrict__ tiles,
                      const uint32_t* __restrict__ blocksum, const float* __restrict__ rec, const int* __restrict__ radii,
                      uint32_t* __restrict__ tile_keys, uint32_t* __restrict__ vals, uint32_t* __restrict__ hist0,
                      uint32_t per_block, uint32_t mask0)
{
    __shared__ uint32_t incl[256];     // inclusive scan of instance counts
    __shared__ uint32_t gid[256];
    __shared__ int rx0[256], ry0[256], rw[256];
    __shared__ uint32_t ws[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int s = blockIdx.x * 256 + tid;
    uint32_t cnt = 0, g = 0;
    int x0 = 0, y0 = 0, x1 = 0, y1 = 0;
    if (s < P) {
        g = order[s];
        cnt = tiles[g];
        if (cnt) {
            const float2 xy = *(const float2*)(rec + (size_t)g * REC_F);
            get_rect(xy.x, xy.y, radii[g], gx, gy, x0, y0, x1, y1);    // same call as the reference's duplicateWithKeys
        }
    }
    uint32_t v = cnt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { uint32_t t = __shfl_up(v, off, 64); if (lane >= (uint32_t)off) v += t; }
    if (lane == 63) ws[wid] = v;
    __syncthreads();
    uint32_t woff = 0;
    for (uint32_t w = 0; w < wid; w++) woff += ws[w];
    const uint32_t total = ws[0] + ws[1] + ws[2] + ws[3];
    incl[tid] = v + woff;
    gid[tid] = g; rx0[tid] = x0; ry0[tid] = y0; rw[tid] = x1 - x0;
    __syncthreads();
    const uint32_t base = blocksum[blockIdx.x];
    for (uint32_t k = tid; k < total; k += 256) {
        // smallest j with incl[j] > k
        uint32_t lo = 0, hi = 255;
#pragma unroll
        for (int it = 0; it < 8; it++) { const uint32_t mid = (lo + hi) >> 1; if (incl[mid] > k) hi = mid; else lo = mid + 1; }
        const uint32_t j = lo;
        const uint32_t local = k - (j ? incl[j - 1] : 0u);
        const int w = rw[j];
        const int ty = ry0[j] + (int)(local / (uint32_t)w), tx = rx0[j] + (int)(local % (uint32_t)w);
        const uint32_t tkey = (uint32_t)(ty * gx + tx);
        tile_keys[base + k] = tkey;
        vals[base + k] = gid[j];
        if (hist0) radix_count_first(hist0, base + k, per_block, tkey, mask0);      // first radix pass's histogram
    }
}
hipError_t launch_emit_instances(hipStream_t s, int P, int gx, int gy, const uint32_t* order, const uint32_t* tiles,
                                 const uint32_t* blocksum, const float* rec, const int* radii, uint32_t* tile_keys,
                                 uint32_t* vals, uint32_t* hist0, uint32_t per_block, uint32_t mask0)
{
    hipLaunchKernelGGL(emit_instances_kernel, dim3((P + 255) / 256), dim3(256), 0, s, P, gx, gy, order, tiles, blocksum, rec,
                       radii, tile_keys, vals, hist0, per_block, mask0);
    return hipGetLastError();
}

// ---- per-tile [start,end) in the sorted list (identifyTileRanges, rasterizer_impl.cu:151-173; ranges pre-zeroed) ----
__global__ void __launch_bounds__(256)
tile_ranges_kernel(uint32_t R, const uint32_t* __restrict__ tile_keys, uint32_t* __restrict__ ranges)
{
    const uint32_t idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= R) return;
    const uint32_t cur = tile_keys[idx];
    if (idx == 0) ranges[2 * cur] = 0;
    else {
        const uint32_t prev = tile_keys[idx - 1];
        if (cur != prev) { ranges[2 * prev + 1] = idx; ranges[2 * cur] = idx; }
    }
    if (idx == R - 1) ranges[2 * cur + 1] = R;
}
hipError_t launch_tile_ranges(hipStream_t s, uint32_t R, const uint32_t* tile_keys, uint32_t* ranges)
{
    if (R == 0) return hipSuccess;
    hipLaunchKernelGGL(tile_ranges_kernel, dim3((R + 255) / 256), dim3(256), 0, s, R, tile_keys, ranges);
    return hipGetLastError();
}
