// radix_sort.h -- the library's stable LSD radix sort of (key, value) pairs of uint32 (radix_sort.hip): the calling protocol.
//   1. lay the buffers out (radix_layout_append) and point a RadixBufs at them;
//   2. radix_sort_begin zeroes what must be zero and sets per_block;
//   3. the caller's own kernel writes keys into ka, values into va, and counts every key's lowest digit into table 0 of `hist` per
//      block of per_block consecutive elements (radix_count_first, or radix_count_first_lds when a block's keys share few digits);
//   4. radix_sort_pairs sorts on key bits [bit_lo, bit_hi), 8 bits per pass, ping-pong between (ka, va) and (kb, vb);
//   5. the result is in (kb, vb) if radix_lands_in_b(bit_hi - bit_lo), else in (ka, va): RadixBufs::sorted_keys / sorted_vals.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#define RADIX 256                          // 8-bit digits
#define SORT_ITEMS 8                       // elements per thread per sort sub-tile
#define SORT_TILE (256 * SORT_ITEMS)       // 2048 elements per block sub-tile
#define SORT_MAX_PASSES 5                  // histogram tables kept per sort (32-bit keys: 4 passes)
#define SORT_MAX_BLOCKS 256                // one block per CU

// `hist`: SORT_MAX_PASSES tables of RADIX * SORT_MAX_BLOCKS counters, table p for pass p.  Table 0 is ACCUMULATED with atomics by the
// kernel that produces the keys, so it is the one table that must be zero before that kernel runs (radix_sort_begin).  The tables of
// the later passes are stored whole by radix_hist_kernel (rows [0, nb)) and only those rows are read: they need no initialisation.
static inline size_t radix_table_bytes() { return (size_t)RADIX * SORT_MAX_BLOCKS * 4; }
static inline size_t radix_hist_bytes() { return SORT_MAX_PASSES * radix_table_bytes(); }
// true: a sort over `bits` key bits ends in (kb, vb) -- an odd number of passes; false: in (ka, va)
static inline bool radix_lands_in_b(int bits) { return (((bits + 7) / 8) & 1) != 0; }
struct RadixBufs {             // plain pointers: they need not be contiguous (bin_radix sorts straight into its point list)
    uint32_t *ka, *kb, *va, *vb, *hist;
    uint32_t per_block = 0;    // elements per block of the sort, a multiple of SORT_TILE (radix_sort_begin)
    uint32_t* sorted_keys(int bits) const { return radix_lands_in_b(bits) ? kb : ka; }
    uint32_t* sorted_vals(int bits) const { return radix_lands_in_b(bits) ? vb : va; }
    // A second sort over this one's result (two rounds make one stable sort on a wider key): it writes its keys into the pair this
    // sort over `bits` bits did NOT end in, ping-pongs with the pair that holds the result, and owns the histogram block after `hist`.
    RadixBufs second_round(int bits) const {
        uint32_t* h2 = hist + radix_hist_bytes() / 4;
        return radix_lands_in_b(bits) ? RadixBufs{ka, kb, va, vb, h2, per_block} : RadixBufs{kb, ka, vb, va, h2, per_block};
    }
};
// scratch layout of a sort of n pairs: ka, kb, va, vb, then `rounds` adjacent histogram blocks, 256-byte aligned, appended at offset o
struct RadixOffsets {
    size_t ka, kb, va, vb, hist;
    RadixBufs at(char* b) const { return RadixBufs{(uint32_t*)(b + ka), (uint32_t*)(b + kb), (uint32_t*)(b + va), (uint32_t*)(b + vb), (uint32_t*)(b + hist)}; }
};
static inline RadixOffsets radix_layout_append(size_t& o, size_t n, int rounds = 1)
{
    const size_t seg = (n * 4 + 255) & ~(size_t)255, at = o;
    o += 4 * seg + rounds * radix_hist_bytes();
    return RadixOffsets{at, at + seg, at + 2 * seg, at + 3 * seg, at + 4 * seg};
}
// sets b.per_block for n pairs; ONE fill launch zeroes table 0 of b.hist (rounds = 2: from its start through table 0 of the next block)
hipError_t radix_sort_begin(hipStream_t s, uint32_t n, RadixBufs& b, int rounds = 1);
hipError_t radix_sort_pairs(hipStream_t s, uint32_t n, const RadixBufs& b, int bit_lo, int bit_hi);      // (n = 0 launches nothing)
hipError_t launch_exclusive_scan(hipStream_t s, int n, uint32_t* data);      // in place, data[0, n), one workgroup (up to a few 100k entries)
#ifdef __HIPCC__
// Step 3, by the thread that wrote element e: one global atomic.  mask: the first pass's digit mask ((1 << bits) - 1 below 8 key bits).
__device__ __forceinline__ void radix_count_first(uint32_t* __restrict__ hist0, uint32_t e, uint32_t per_block, uint32_t key, uint32_t mask = 255u)
{
    atomicAdd(&hist0[(e / per_block) * RADIX + (key & mask)], 1u);
}
// Step 3 for keys that share few digits inside a block: the workgroup of 256 threads owns elements [256 blockIdx.x, +256), counts
// them in LDS first and adds every non-zero digit count once.  Called by ALL 256 threads; produce(key) writes the thread's element
// and returns its key, or returns false when the thread has none.  Precondition: per_block is a multiple of 256 (it is one of
// SORT_TILE), so the workgroup's elements lie in one block of the sort.
template <class Produce>
__device__ __forceinline__ void radix_count_first_lds(uint32_t* __restrict__ hist0, uint32_t per_block, Produce produce)
{
    __shared__ uint32_t h[RADIX];
    h[threadIdx.x] = 0;
    __syncthreads();
    uint32_t key;
    if (produce(key)) atomicAdd(&h[key & 255u], 1u);
    __syncthreads();
    const uint32_t c = h[threadIdx.x];
    if (c) atomicAdd(&hist0[(blockIdx.x * 256u / per_block) * RADIX + threadIdx.x], c);
}
#endif
