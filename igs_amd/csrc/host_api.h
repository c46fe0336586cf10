// host_api.h -- the error plumbing of the C entry points (include/igs_rast.h) and the argument checks they share, for every .hip file that
// defines some next to its kernels.
// Host code only.  The message buffer behind igs_rast_last_error() is thread-local in api.hip, which defines fail() and fail_in().
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/igs_rast.h"

// both store the message that igs_rast_last_error() returns on this thread and return the code for the entry point to hand back
int fail(int code, const char* what, hipError_t e = hipSuccess);      // "<what>", or "<what>: <HIP error string>" for e != hipSuccess
int fail_in(const char* fn, const char* what);                        // IGS_RAST_E_INVALID, "<fn>: <what>"
#define HIP_TRY(expr, what) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail(IGS_RAST_E_HIP, what, e_); } while (0)

static inline bool dtype_ok(int dtype) { return dtype == IGS_DTYPE_F32 || dtype == IGS_DTYPE_F16; }
static inline size_t dtype_bytes(int dtype) { return dtype == IGS_DTYPE_F16 ? 2 : 4; }
// the grid that the kernels' four-element loads and stores of a dtype need their addresses on
static inline size_t vec_grid_bytes(int dtype) { return 4 * dtype_bytes(dtype); }
static inline bool ptr_aligned(const void* p, size_t bytes) { return (((uintptr_t)p) & (bytes - 1)) == 0; }      // (bytes: a power of two)
static inline bool eps_ok(float eps) { return eps >= 0.f && eps < 3.0e38f; }                                     // finite and >= 0; a NaN is not
// the bytes [lo, hi) of an operand
struct ByteSpan { uintptr_t lo, hi; };
static inline ByteSpan byte_span(const void* p, size_t bytes) { return ByteSpan{(uintptr_t)p, (uintptr_t)p + bytes}; }
static inline bool spans_overlap(ByteSpan a, ByteSpan b) { return a.lo < b.hi && b.lo < a.hi; }
// the [n][c][H][W] layouts read in place: every H x W plane contiguous (NCHW and any slicing of n or c); channels-last has no kernels here
static inline const char* plane_stride_error(int C, int H, int W, long long fs_n, long long fs_c, long long fs_h, long long fs_w)
{
    if (fs_n < 0 || fs_c < 0) return "negative feature stride";
    if ((W > 1 && fs_w != 1) || (H > 1 && fs_h != W)) {
        if (fs_c == 1 && C > 1) return "channels-last features (fs_c == 1) are not read in place: pass plane-contiguous NCHW";
        return "feature strides not supported: every H x W plane must be contiguous (fs_w == 1, fs_h == W)";
    }
    return nullptr;
}
