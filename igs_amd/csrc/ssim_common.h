// ssim_common.h -- what the image-space loss kernels of loss_ops.hip (one image, the refine loop) and ssim_batch.hip (a batch, the AGM-Net
// training loss) share: the tile geometry, the 11-tap window and the XCD-band tile assignment.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#define SSIM_R 5                       // window radius
#define SSIM_T 32                      // tile edge (outputs per workgroup: 32 x 32)
#define SSIM_H (SSIM_T + 2 * SSIM_R)   // halo edge (42): 1.72x the tile area (2.6x at 16 x 16)
#define SSIM_HS 44                     // floats per halo row (16-byte aligned rows)
#define SSIM_BS 36                     // floats per row of the horizontally blurred arrays
// LDS banks: in the horizontal pass consecutive lanes take consecutive ROWS and move float4s; with row strides of 44 and 36
// floats (11 and 9 float4s, both odd) 16 consecutive rows start in 16 different 4-bank groups, so the b128 reads and writes
// are conflict-free (one output column group per lane and scalar accesses put 64 lanes on 16 banks: 4-way conflicts, 2.5x slower)
// Both passes are register-blocked: a work item produces 4 adjacent outputs from 14 loaded inputs (3x fewer LDS reads than one
// output per thread); the vertical pass has exactly 32 columns x 8 row groups = 256 work items.

struct SsimWin { float g[2 * SSIM_R + 1]; };

// XCD-aware tile assignment of the image-space loss kernels.  Workgroups are dealt round-robin over the 8 XCDs (b % 8), each with its
// own L2; a tile's halo is the interior of its neighbours, so neighbours should run on the SAME L2: XCD x takes a contiguous BAND of tile
// rows (rows [x * rpb, (x + 1) * rpb) of every plane), row-major inside the band.  Launched as a 1-D grid of 8 * planes * rpb * gx
// workgroups; the few that map past the last row exit at once (whole workgroups, before any barrier).  Speed only, never correctness.
__device__ __forceinline__ bool band_tile(unsigned b, unsigned gx, unsigned gy, unsigned planes, unsigned& col, unsigned& row, unsigned& plane)
{
    const unsigned rpb = (gy + 7u) / 8u;
    const unsigned xcd = b & 7u, k = b >> 3;
    const unsigned per = rpb * gx;
    plane = k / per;
    const unsigned rem = k - plane * per;
    row = xcd * rpb + rem / gx;
    col = rem % gx;
    return plane < planes && row < gy;
}
static inline unsigned band_grid(unsigned gx, unsigned gy, unsigned planes) { return 8u * planes * ((gy + 7u) / 8u) * gx; }

static SsimWin make_window()
{
    // loss_utils.py:21-24: gauss = Tensor([exp(-(x - 5)^2 / (2 * 1.5^2))]) ; gauss / gauss.sum()   (float32 tensor arithmetic)
    SsimWin w; float sum = 0.f;
    for (int i = 0; i <= 2 * SSIM_R; i++) { w.g[i] = (float)exp(-(double)((i - SSIM_R) * (i - SSIM_R)) / (2.0 * 1.5 * 1.5)); sum += w.g[i]; }
    for (int i = 0; i <= 2 * SSIM_R; i++) w.g[i] = w.g[i] / sum;
    return w;
}
