/*
 * igs_rast.h -- C ABI of the MI355X-native differentiable Gaussian-splat rasterizer.
 *
 * This is the drop-in boundary for the hot path of asd56585452/IGS: the entry points are what the
 * reference's torch glue binds to (DGR = submodules/RaDe-GS/submodules/diff-gaussian-rasterization):
 *
 *   igs_rast_forward       <-> CudaRasterizer::Rasterizer::forward   (DGR/cuda_rasterizer/rasterizer.h:31-65,
 *                              called from RasterizeGaussiansCUDA, DGR/rasterize_points.cu:98-130)
 *   igs_rast_backward      <-> CudaRasterizer::Rasterizer::backward  (rasterizer.h:67-112,
 *                              called from RasterizeGaussiansBackwardCUDA, rasterize_points.cu:197-242)
 *   igs_rast_mark_visible  <-> CudaRasterizer::Rasterizer::markVisible (rasterizer.h:24-29, rasterize_points.cu:259-263)
 *
 * Conventions (identical to the reference unless stated):
 *   - plain device pointers to contiguous fp32 / int32 data, row-major; no torch types;
 *   - optional inputs are signalled by NULL (the reference relies on data_ptr()==nullptr of empty tensors);
 *   - viewmatrix / projmatrix are the TRANSPOSED 4x4 matrices the callers build (row-vector convention);
 *   - the three scratch buffers are opaque byte buffers grown through callbacks; they must stay alive and
 *     unmodified until the matching backward call, and P, R (= the value forward returned), W, H must be the same;
 *   - `stream` is a hipStream_t (pass the framework's current stream; NULL = default stream).  All work is
 *     enqueued on it.  The host wait is bounded: IGS_RAST_WAIT_TIMEOUT_S seconds (default 10) without the status, a stream
 *     error, or a drained stream without it return IGS_RAST_E_HIP.  forward performs ONE host wait (for the 12-byte frame status {num_rendered, slab overflow, prefilter
 *     flag} that the blend kernel posts into pinned host memory; the reference reads its count back at
 *     rasterizer_impl.cu:354); backward performs none;
 *   - threading: the library keeps a little state PER HOST THREAD (the pinned status slot, the per-tile slab size that worked
 *     for the last frames, the pending frame of igs_rast_forward_async, the last error text); calls from different threads
 *     do not interfere, a frame started on one thread must be finished / differentiated on the same thread.  The optional
 *     stage profiler (igs_rast_profile_*) is process-wide and meant for single-threaded benchmarking;
 *   - image outputs of forward must be zero-filled by the caller when P == 0 (nothing is launched, as in
 *     rasterize_points.cu:90); for P > 0 every pixel of every output is written;
 *   - any of backward's seven upstream image gradients may be NULL, meaning all zeros (the output did not take part in
 *     the loss); geometry branches without any upstream gradient are skipped, the result is the same;
 *   - backward writes every element of its eight outputs (no pre-zeroing needed) and uses a caller-provided
 *     workspace of igs_rast_backward_workspace_bytes(P) bytes (contents undefined on entry).
 *
 * Return values: forward returns num_rendered (>= 0) or a negative IGS_RAST_E_* code; the others return 0 or a
 * negative code.  igs_rast_last_error() returns a static, thread-local description of the last failure.
 */
#ifndef IGS_RAST_H
#define IGS_RAST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IGS_RAST_VERSION 4

#define IGS_RAST_E_INVALID   (-1)   /* bad argument (NULL required pointer, negative size, ...) */
#define IGS_RAST_E_HIP       (-2)   /* a HIP runtime call or kernel launch failed */
#define IGS_RAST_E_ALLOC     (-3)   /* a scratch callback returned NULL */
#define IGS_RAST_E_PREFILTER (-4)   /* `prefiltered` set but a point was culled (the reference __trap()s, auxiliary.h:172-176) */
#define IGS_RAST_E_CHANNELS  (-5)   /* reserved: non-RGB without precomputed colours (rasterizer_impl.cu:308-311) */

#define IGS_RAST_E_RETRY     (-6)   /* igs_rast_forward_finish: a tile overflowed its instance slab: redo the frame */

/* Scratch growth callback: make the buffer at least `bytes` long and return its device address
 * (the reference's std::function<char*(size_t)> resizeFunctional, rasterize_points.cu:27-33). */
typedef char* (*igs_rast_alloc_fn)(void* user, size_t bytes);

int igs_rast_version(void);
const char* igs_rast_last_error(void);

int igs_rast_forward(
    void* stream,
    igs_rast_alloc_fn geometry_buffer, void* geometry_user,
    igs_rast_alloc_fn binning_buffer, void* binning_user,
    igs_rast_alloc_fn image_buffer, void* image_user,
    int P, int D, int M,
    const float* background,              /* [3] */
    int width, int height,
    const float* means3D,                 /* [P,3] */
    const float* shs,                     /* [P,M,3] or NULL */
    const float* colors_precomp,          /* [P,3] or NULL */
    const float* opacities,               /* [P] */
    const float* scales,                  /* [P,3] or NULL */
    float scale_modifier,
    const float* rotations,               /* [P,4] (w,x,y,z) or NULL */
    const float* cov3D_precomp,           /* [P,6] or NULL */
    const float* viewmatrix,              /* [16] */
    const float* projmatrix,              /* [16] */
    const float* cam_pos,                 /* [3] */
    float tan_fovx, float tan_fovy,
    float kernel_size,
    int prefiltered,
    float* out_color,                     /* [3,H,W] */
    float* out_coord,                     /* [3,H,W] */
    float* out_mcoord,                    /* [3,H,W] */
    float* out_depth,                     /* [1,H,W] */
    float* out_mdepth,                    /* [1,H,W] */
    float* out_alpha,                     /* [1,H,W] */
    float* out_normal,                    /* [3,H,W] */
    int* radii,                           /* [P] */
    int require_coord, int require_depth,
    int debug);                           /* debug != 0: synchronise and check after every launch (auxiliary.h:404-411) */

/* Asynchronous pair (no reference counterpart; used by the native refine step so the GPU never waits for the host):
 * igs_rast_forward_async = igs_rast_forward without the final wait for the instance count; it returns INT_MAX ("not known
 * yet"), which igs_rast_backward accepts as R.  igs_rast_forward_finish() waits for the 12-byte
 * read-back (done right after the tile scan) and returns the true num_rendered, or IGS_RAST_E_RETRY when the guessed
 * per-tile instance slabs were too small: whatever was enqueued on top of the frame must then be discarded and the frame
 * redone with igs_rast_forward. */
int igs_rast_forward_async(
    void* stream,
    igs_rast_alloc_fn geometry_buffer, void* geometry_user, igs_rast_alloc_fn binning_buffer, void* binning_user,
    igs_rast_alloc_fn image_buffer, void* image_user,
    int P, int D, int M, const float* background, int width, int height,
    const float* means3D, const float* shs, const float* colors_precomp, const float* opacities,
    const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
    const float* viewmatrix, const float* projmatrix, const float* cam_pos,
    float tan_fovx, float tan_fovy, float kernel_size, int prefiltered,
    float* out_color, float* out_coord, float* out_mcoord, float* out_depth, float* out_mdepth, float* out_alpha,
    float* out_normal, int* radii, int require_coord, int require_depth, int debug);
int igs_rast_forward_finish(void);

/* Forward for stream capture (hipGraph / torch.cuda.graph; no reference counterpart -- the reference's forward reads its
 * instance count back in the middle, rasterizer_impl.cu:354, and cannot be captured): the launches of igs_rast_forward with no
 * host-side wait and no pending latch; returns INT_MAX like igs_rast_forward_async.  Nothing it does is illegal on a capturing
 * stream PROVIDED one ordinary igs_rast_forward has run on this host thread and device before (the pinned status slot is
 * allocated then) and the scratch callbacks do not allocate illegally (PyTorch's graph-pool allocations are fine).
 * Every replay posts {num_rendered, overflow, prefilter flag} into the thread's status slot; igs_rast_last_status() returns
 * them once the caller has synchronised the stream.  overflow != 0 means the per-tile instance slabs baked into the capture
 * were too small for that replay: its results are invalid, the slab hint has been raised, capture again.
 * igs_rast_last_status() checks the slot's sequence word against the number baked into the calling thread's last
 * igs_rast_forward_nowait: before the first replay has run (or when an eager forward has posted since) it returns
 * IGS_RAST_E_RETRY instead of an older frame's numbers. */
int igs_rast_forward_nowait(
    void* stream,
    igs_rast_alloc_fn geometry_buffer, void* geometry_user, igs_rast_alloc_fn binning_buffer, void* binning_user,
    igs_rast_alloc_fn image_buffer, void* image_user,
    int P, int D, int M, const float* background, int width, int height,
    const float* means3D, const float* shs, const float* colors_precomp, const float* opacities,
    const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
    const float* viewmatrix, const float* projmatrix, const float* cam_pos,
    float tan_fovx, float tan_fovy, float kernel_size, int prefiltered,
    float* out_color, float* out_coord, float* out_mcoord, float* out_depth, float* out_mdepth, float* out_alpha,
    float* out_normal, int* radii, int require_coord, int require_depth, int debug);
int igs_rast_last_status(int* num_rendered, unsigned* overflow, unsigned* prefilter_flag);
/* The same without the sequence check, for callers who replay SEVERAL captured graphs in turn (only the last capture's number is
 * remembered) and know that a forward has run since: what the last forward that EXECUTED on this thread's slot posted. */
int igs_rast_last_posted_status(int* num_rendered, unsigned* overflow, unsigned* prefilter_flag);

/* One-shot promise for the NEXT igs_rast_forward / _async / _nowait of the calling thread: the image buffer its callback will hand out
 * was zero-filled when it was allocated and has been used by this library only since.  Every slab-binned forward leaves the binning
 * counters in the image buffer zeroed behind it, so such a forward needs no zero-fill launch (igs_refine_step_args::scratch_clean is
 * the same promise for the fused step).  A broken promise costs a wrong or redone frame or an error code, never a fault. */
void igs_rast_hint_scratch_clean(int on);

/* Count pass of the compress rasterizer (diff_gaussian_rasterization_compress, CountGaussiansCUDA / forwardCount of
 * compress-diff-gaussian-rasterization rasterize_points.cu:130-217, rasterizer_impl.cu:441-530): vanilla-3DGS preprocess (2-D covariance
 * dilated by 0.3, raw opacity), the same binning as igs_rast_forward, a colour-only blend into out_color [3,H,W] (background included),
 * and per Gaussian:
 *   count[i] = the exact number of pixels into which Gaussian i is blended (the reference's non-atomic increments undercount),
 *   score[i] = (float)count[i] * opacities[i], rounded once.
 * radii [P] as the vanilla preprocess computes them.  Returns num_rendered or a negative IGS_RAST_E_* code (bad sizes / NULL outputs:
 * IGS_RAST_E_INVALID before any HIP call; prefiltered with a culled point: IGS_RAST_E_PREFILTER).  P == 0 launches nothing. */
int igs_rast_count_gaussians(
    void* stream,
    igs_rast_alloc_fn geometry_buffer, void* geometry_user,
    igs_rast_alloc_fn binning_buffer, void* binning_user,
    igs_rast_alloc_fn image_buffer, void* image_user,
    int P, int D, int M,
    const float* background,              /* [3] */
    int width, int height,
    const float* means3D,                 /* [P,3] */
    const float* shs,                     /* [P,M,3] or NULL */
    const float* colors_precomp,          /* [P,3] or NULL */
    const float* opacities,               /* [P] */
    const float* scales,                  /* [P,3] or NULL */
    float scale_modifier,
    const float* rotations,               /* [P,4] or NULL */
    const float* cov3D_precomp,           /* [P,6] or NULL */
    const float* viewmatrix,              /* [16] */
    const float* projmatrix,              /* [16] */
    const float* cam_pos,                 /* [3] */
    float tan_fovx, float tan_fovy,
    int prefiltered,
    float* out_color,                     /* [3,H,W] */
    int* count,                           /* [P] */
    float* score,                         /* [P] */
    int* radii,                           /* [P] */
    int debug);

/* Binning scratch tuning (no reference counterpart).  The default path gives every 16x16 tile a slab of `slots_per_tile`
 * instance slots (12 bytes each) in binningBuffer; a frame in which some tile needs more is redone automatically with larger
 * slabs (and, beyond 16384 per tile, with the global radix sort), and the size then sticks for the calling thread.  Setting the
 * hint up front avoids that first redo; 0 restores the default (1024).  get returns the current value. */
void igs_rast_set_slab_hint(unsigned slots_per_tile);
unsigned igs_rast_get_slab_hint(void);

size_t igs_rast_backward_workspace_bytes(int P);

int igs_rast_backward(
    void* stream,
    int P, int D, int M, int R,
    const float* background,
    int width, int height,
    const float* means3D,
    const float* shs,
    const float* colors_precomp,
    const float* alphas,                  /* forward's out_alpha */
    const float* scales,
    float scale_modifier,
    const float* rotations,
    const float* cov3D_precomp,
    const float* viewmatrix,
    const float* projmatrix,
    const float* campos,
    float tan_fovx, float tan_fovy,
    float kernel_size,
    const int* radii,
    const float* normalmap,               /* forward's out_normal */
    const char* geom_buffer,
    const char* binning_buffer,
    const char* image_buffer,
    const float* dL_dpix,                 /* [3,H,W] */
    const float* dL_dpix_coord,           /* [3,H,W] */
    const float* dL_dpix_mcoord,          /* [3,H,W] */
    const float* dL_dpix_depth,           /* [1,H,W] */
    const float* dL_dpix_mdepth,          /* [1,H,W] */
    const float* dL_dalphas,              /* [1,H,W] */
    const float* dL_dpixel_normals,       /* [3,H,W] */
    void* workspace,
    float* dL_dmean2D,                    /* [P,3]  (z = sum |.|, the GOF densification statistic) */
    float* dL_dcolor,                     /* [P,3] */
    float* dL_dopacity,                   /* [P] */
    float* dL_dmean3D,                    /* [P,3] */
    float* dL_dcov3D,                     /* [P,6] */
    float* dL_dsh,                        /* [P,M,3] (ignored when M == 0) */
    float* dL_dscale,                     /* [P,3] */
    float* dL_drot,                       /* [P,4] */
    int require_coord, int require_depth,
    int debug);

/* ---- V views of one Gaussian set in one call (no reference counterpart as ONE call: it replaces the view loop of
 * GS3DRenderer.forward_single_batch, igs/models/gs.py:839-847, every pass of which is one RasterizeGaussiansCUDA /
 * RasterizeGaussiansBackwardCUDA, rasterize_points.cu:35-246, and the AccumulateGrad adds autograd runs from the second view on) ----
 *
 * igs_rast_views_max(): the largest V one call accepts (16).
 *
 * igs_rast_forward_views: the argument list of igs_rast_forward with
 *   viewmatrix [V][16], projmatrix [V][16], cam_pos [V][3]       device arrays, one camera per view;
 *   out_color .. out_normal [V][c][H][W], radii [V][P]           view v's slice is what igs_rast_forward writes for camera v, bit for bit;
 *   geometry_user / binning_user / image_user [V]                HOST arrays of `user` words: view v's scratch is requested as
 *                                                                geometry_buffer(geometry_user[v], bytes) and so on -- one callback per
 *                                                                kind, V distinct buffers, which igs_rast_backward_views takes back;
 *   num_rendered [V]                                             HOST array: view v's instance count.
 * Shared by all views: image size, tan_fovx/y, background, scale_modifier, kernel_size, SH degree (M <= 16), prefiltered, require_*.
 * All V pipelines are enqueued before the host looks at a status, view v posting into status slot 1 + v of the calling thread (slot 0
 * stays the single-view entry points'): one host wait per call.  A view whose per-tile slabs overflowed is redone alone once every
 * status is in; the slab hint is raised once, to what the densest tile of any view needs; the other views' results stand.  With
 * IGS_BINNING=radix (or slabs beyond the scratch limits) the views run one after the other through the global sort.
 * igs_rast_hint_scratch_clean before the call is a promise about all V image buffers.
 * Returns 0 or a negative IGS_RAST_E_* code.  IGS_RAST_E_INVALID before any HIP call: V < 1 or V > igs_rast_views_max(), bad sizes, a
 * NULL camera array, a NULL callback or user array, a NULL output or num_rendered.  P == 0 launches nothing, zeroes num_rendered and
 * returns 0.  On a capturing stream: IGS_RAST_E_INVALID (capture single views with igs_rast_forward_nowait).
 *
 * igs_rast_backward_views: the argument list of igs_rast_backward with
 *   R [V]                                                        HOST array: num_rendered of igs_rast_forward_views;
 *   viewmatrix / projmatrix / campos, radii [V][P]               as above;
 *   alphas [V][1][H][W], normalmap [V][3][H][W]                  the forward's out_alpha / out_normal;
 *   geom_buffer / binning_buffer / image_buffer [V]              HOST arrays of the V views' scratch addresses;
 *   dL_dpix .. dL_dpixel_normals [V][c][H][W]                    any may be NULL = zeros for ALL views;
 *   workspace                                                    V x igs_rast_backward_workspace_bytes(P) bytes, view v's part at v x that;
 *   dL_dmean2D [V][P][3] or NULL                                 per view (the densification statistics take it per view); NULL skips it;
 *   dL_dcolor .. dL_drot                                         ONE set: the sum over the views, views added in index order.
 * The V blend backwards (the existing kernels) are enqueued, then one per-Gaussian kernel forms every view's gradients and adds them
 * in registers: no float atomics, every row written once, +0 everywhere for a Gaussian no view sees.  With clamp_grads
 * (igs_rast_next_backward_options) each VIEW's dL_dmean3D, dL_dsh, dL_dopacity, dL_dscale, dL_drot are clamped before they are added,
 * which is what V single-view calls of the clamp package followed by autograd's adds compute.  nan_report: one word for the whole call.
 * Returns 0 or a negative code; IGS_RAST_E_INVALID before any HIP call as above, and for a NULL entry of the per-view scratch arrays. */
int igs_rast_views_max(void);
int igs_rast_forward_views(
    void* stream, int V,
    igs_rast_alloc_fn geometry_buffer, void* const* geometry_user, igs_rast_alloc_fn binning_buffer, void* const* binning_user,
    igs_rast_alloc_fn image_buffer, void* const* image_user,
    int P, int D, int M, const float* background, int width, int height,
    const float* means3D, const float* shs, const float* colors_precomp, const float* opacities,
    const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
    const float* viewmatrix, const float* projmatrix, const float* cam_pos,
    float tan_fovx, float tan_fovy, float kernel_size, int prefiltered,
    float* out_color, float* out_coord, float* out_mcoord, float* out_depth, float* out_mdepth, float* out_alpha,
    float* out_normal, int* radii, int* num_rendered, int require_coord, int require_depth, int debug);
int igs_rast_backward_views(
    void* stream, int V, int P, int D, int M, const int* R, const float* background, int width, int height,
    const float* means3D, const float* shs, const float* colors_precomp, const float* alphas,
    const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
    const float* viewmatrix, const float* projmatrix, const float* campos,
    float tan_fovx, float tan_fovy, float kernel_size, const int* radii, const float* normalmap,
    const char* const* geom_buffer, const char* const* binning_buffer, const char* const* image_buffer,
    const float* dL_dpix, const float* dL_dpix_coord, const float* dL_dpix_mcoord, const float* dL_dpix_depth,
    const float* dL_dpix_mdepth, const float* dL_dalphas, const float* dL_dpixel_normals,
    void* workspace,
    float* dL_dmean2D, float* dL_dcolor, float* dL_dopacity, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh,
    float* dL_dscale, float* dL_drot, int require_coord, int require_depth, int debug);

int igs_rast_mark_visible(void* stream, int P, const float* means3D, const float* viewmatrix,
                          const float* projmatrix, uint8_t* present /* [P], 0/1 */);

/* ---- introspection for tests and the roofline harness (no reference counterpart) ---- */

/* Copies per-stage scratch contents into caller-provided DEVICE arrays (any may be NULL) so that the HIP
 * stages can be compared one by one with the CPU oracle's intermediates:
 *   rec32     [P,32] the packed per-Gaussian record (layout in igs_amd/csrc/common.h)
 *   tiles     [P]    tiles touched
 *   point_list[R]    sorted Gaussian ids
 *   ranges    [T,2]  per-tile [start,end)
 *   n_contrib [2,H,W] last / median contributor counts */
int igs_rast_debug_dump(void* stream, int P, int R, int width, int height,
                        const char* geom_buffer, const char* binning_buffer, const char* image_buffer,
                        float* rec32, uint32_t* tiles, uint32_t* point_list, uint32_t* ranges, uint32_t* n_contrib);

/* Optional per-stage timing with HIP events recorded on the caller's stream (used by bench.py for the roofline line).
 * Stage order of the arrays (IGS_RAST_NSTAGES entries): preprocess, depth_sort, scan, emit, tile_sort, ranges,
 * blend_fwd, memset, blend_bwd, geom_bwd.  igs_rast_profile_read synchronises on the last recorded event; r_sum is the
 * sum of num_rendered over the forward calls seen, calls their number.
 * igs_rast_profile_enable(N): 0 = off, N > 0 = mark every N-th frame (forward call / refine step); an event record costs a
 * few microseconds of stream time, so marking every frame slows a 0.35 ms refine step by about 10 %, every 8th by about 1 %.
 * In igs_refine_step the geom_bwd stage includes the activation backward and the Adam update. */
#define IGS_RAST_NSTAGES 10
/* Which backward tile-blend instance the last igs_rast_backward / igs_refine_step of this process launched (any thread): bit 0 coord, bit 1
 * depth, bit 2 normal gradients present, bit 3 the |screen-space gradient| moment; -1 = none.  (The reference instantiates from
 * require_coord / require_depth alone, backward.cu:1153-1160; here branches whose upstream gradients are all NULL are left out.) */
/* Options of the NEXT igs_rast_backward of this host thread (extension; one-shot, consumed by that call): the reference's argument
 * list has no room for them and stays as it is.
 *  nan_report != 0: the reference's Python backward ends with seven `assert not torch.isnan(grad).any()` -- seven reductions and host
 *   syncs (DGR/diff_gaussian_rasterization_rade/__init__.py:156-162).  The per-Gaussian kernel instead tests every element it writes of
 *   dL_dmean2D, dL_dcolor, dL_dopacity, dL_dmean3D, dL_dsh, dL_dscale, dL_drot (not dL_dcov3D: the reference does not look at it either)
 *   and, if it wrote a NaN, says so in one word of pinned host memory; an event is recorded behind the kernel.  igs_rast_nan_report_wait()
 *   blocks until that event has completed and returns 1 (a NaN was written), 0 (none) or a negative error code.  Bounded like the forward's status wait (IGS_RAST_WAIT_TIMEOUT_S).
 *  clamp_grads > 0: dL_dmean3D, dL_dsh, dL_dopacity, dL_dscale, dL_drot are clamped to +-clamp_grads as they are written (what the clamp
 *   package does with five torch.clamp calls afterwards, DGRC/diff_gaussian_rasterization_rade_clamp/__init__.py:156-162); a NaN stays
 *   a NaN for the report, as it does through torch.clamp. */
void igs_rast_next_backward_options(int nan_report, float clamp_grads);
int igs_rast_nan_report_wait(void);
/* The same wait from ANOTHER host thread or at a later time (PyTorch runs a Function's backward on its own worker thread and the
 * assert is better raised once the whole backward pass has been enqueued): right after the igs_rast_backward that was asked for a report,
 * on the thread that called it, igs_rast_nan_report_handle() returns a ticket for the verdict (valid for the life of the process; the
 * last 256 reports of a thread stay readable) and its sequence number, instead of waiting;
 * igs_rast_nan_report_wait_at(word, seq) then blocks (bounded by IGS_RAST_WAIT_TIMEOUT_S) and returns 1 / 0 / a negative code. */
int igs_rast_nan_report_handle(const void** ticket, unsigned* seq);
int igs_rast_nan_report_wait_at(const void* ticket, unsigned seq);
int igs_rast_last_backward_instance(void);
/* Test hook: overwrites the LDS of every CU with NaN bit patterns (a kernel that reads LDS it never wrote then fails small parity
 * tests instead of passing on a fresh device's zeros). */
int igs_rast_debug_poison_lds(void* stream);
int igs_rast_profile_enable(int on);
int igs_rast_profile_read(double* ms_sum, long long* count, double* r_sum, long long* calls, int reset);

/* ---- refine-loop helpers ("next" rows of SURVEY.md 8f: fused loss / fused multi-group Adam) ---- */

/* One Adam step over a flat fp32 parameter span, torch.optim.Adam semantics without weight decay / amsgrad, as
 * built by GaussianModel.load_fromstream (igs/models/gaussian_model.py:295-348: Adam(lr=0, eps=1e-15), per-group lr).
 * bias_correction1 = 1 - beta1^t, bias_correction2_sqrt = sqrt(1 - beta2^t). */
int igs_adam_step(void* stream, size_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                  float lr, float beta1, float beta2, float eps, float bias_correction1, float bias_correction2_sqrt);

/* The same for up to 8 parameter groups in ONE launch: group k covers param[offset[k] .. offset[k]+count[k]) with lr[k]. */
int igs_adam_step_groups(void* stream, int ngroups, const size_t* offset, const size_t* count, const float* lr, float* param,
                         const float* grad, float* exp_avg, float* exp_avg_sq, float beta1, float beta2, float eps,
                         float bias_correction1, float bias_correction2_sqrt);

/* The same for up to 8 SEPARATE tensors in one launch (each parameter of the reference's optimiser is its own nn.Parameter with its own
 * gradient and state tensors, torch.optim.Adam keeps one step count per parameter: gaussian_model.py:303-348): arrays of `ntensors`
 * device pointers / element counts / learning rates / bias corrections in HOST memory, read before the call returns. */
int igs_adam_step_multi(void* stream, int ntensors, float* const* param, const float* const* grad, float* const* exp_avg,
                        float* const* exp_avg_sq, const size_t* count, const float* lr, const float* bias_correction1,
                        const float* bias_correction2_sqrt, float beta1, float beta2, float eps);

/* The same with the step counts in DEVICE memory (step[k]: one float per tensor = the number of COMPLETED steps, the layout of
 * torch.optim.Adam(capturable=True)): every workgroup computes its bias corrections from step + 1, the workgroup that finishes last
 * advances the counts.  Nothing of the call depends on host state that changes from step to step, so it can be captured into a
 * hipGraph and replayed.  done_scratch: igs_adam_step_multi_dev_scratch_words() 32-bit words, zero before the first call and zero
 * again after every call (a buffer the caller zero-fills once and keeps; calls that share it must be ordered on one stream). */
size_t igs_adam_step_multi_dev_scratch_words(void);
int igs_adam_step_multi_dev(void* stream, int ntensors, float* const* param, const float* const* grad, float* const* exp_avg,
                            float* const* exp_avg_sq, const size_t* count, const float* lr, float* const* step, unsigned* done_scratch,
                            float beta1, float beta2, float eps);

/* ---- one whole refine iteration on one view, single GPU --------------------------------------------------------------
 * Native form of the body of the reference's per-frame refine loop (infer_batch.py:279-324 with the L1 photometric loss,
 * igs/utils/loss_utils.py:17; activations of igs/models/gaussian_model.py:90-127; torch.optim.Adam of :295-348):
 *   opacity = sigmoid, scale = exp, rotation = normalize  ->  render  ->  loss = loss_weight * mean|color - gt|
 *   ->  backward through rasterizer and activations  ->  Adam update of the five parameter groups, in place.
 * Everything is enqueued on `stream` without a host wait; the gradients never reach HBM (the per-Gaussian backward kernel
 * applies the update itself).  `param` / `exp_avg` / `exp_avg_sq` are flat fp32 buffers holding the five groups at the given
 * float offsets: xyz [P][3], rotation [P][4] (raw quaternion), shs [P][M][3], opacity [P] (logit), scale [P][3] (log).
 * Multi-GPU runs need the gradients for the exchange: with `grad_out` set the same launches end in the flat gradient
 * instead of the update (then all-reduce it and call igs_adam_step_groups -- or, with `color_grad_out` set as well, gather the
 * per-view colour gradients, all-reduce only the 11 small-group floats, and let igs_adam_sh_from_view_colors update the SH
 * coefficients: the SH span of `grad_out` is then left untouched).
 * Returns num_rendered or a negative error code. */
typedef struct igs_refine_step_args {
    void* stream;
    igs_rast_alloc_fn geometry_buffer; void* geometry_user;
    igs_rast_alloc_fn binning_buffer;  void* binning_user;
    igs_rast_alloc_fn image_buffer;    void* image_user;
    void* workspace;                          /* igs_rast_backward_workspace_bytes(P) */
    int P, D, M, width, height;
    const float* background;                  /* [3] device */
    float *param, *exp_avg, *exp_avg_sq;      /* flat optimiser state, device */
    float* grad_out;                          /* NULL: apply Adam in place.  Non-NULL (multi-GPU): write the flat gradient of the raw
                                                 leaves here (same offsets) and leave param / exp_avg / exp_avg_sq untouched */
    size_t off_xyz, off_rot, off_sh, off_opacity, off_scale;
    float lr_xyz, lr_rot, lr_sh, lr_opacity, lr_scale;
    float beta1, beta2, eps;
    int step;                                 /* 1-based number of this update (bias correction) */
    const float *viewmatrix, *projmatrix, *cam_pos;   /* device */
    float tan_fovx, tan_fovy;
    const float* gt;                          /* [3][H][W] device */
    float loss_weight;                        /* loss = loss_weight * ((1 - lambda_dssim) * mean|color - gt| + lambda_dssim * (1 - mean SSIM)) */
    float lambda_dssim;                       /* 0: pure L1 (fused into the blend backward); the reference uses 0.2 (loss_utils.py:34-63) */
    float lambda_depth_normal;                /* > 0 adds loss_weight * lambda_depth_normal * depth-normal regulariser (RaDe-GS train.py:143-160;
                                                 needs require_depth): the backward then runs its <depth, normal> instance */
    float depth_ratio;                        /* weight of the median-depth term of the regulariser (0 = the reference's 0.6) */
    void* loss_scratch;                       /* lambda_dssim > 0 or lambda_depth_normal > 0: igs_refine_loss_scratch_bytes(width, height) bytes */
    float* out_images;                        /* [15][H][W]: color 3 | coord 3 | mcoord 3 | depth 1 | mdepth 1 | alpha 1 | normal 3 */
    int* radii;                               /* [P] */
    float* dL_dmean2D;                        /* [P][3] view-space gradient (densification statistic) or NULL = not wanted: the
                                                 blend backward then leaves out the |gradient| sum nothing else reads */
    float* loss_out;                          /* device, 1 float: the loss value, or NULL */
    int require_coord, require_depth;
    float clamp_grads;                        /* > 0: the rasterizer's gradients w.r.t. means3D / sh / opacities / scales / rotations are clamped to
                                                 +-clamp_grads before they go on (diff_gaussian_rasterization_rade_clamp, 15); 0: off */
    float* color_grad_out;                    /* [P][3] or NULL: dL/d(colour) of this view per Gaussian (clamped channels and unseen Gaussians
                                                 zero) -- what the ranks of a multi-GPU step gather instead of all-reducing dL/dSH */
    int scratch_clean;                        /* != 0: the caller vouches that the image buffer the callback hands out was zero-filled when
                                                 it was allocated and has since been used by this library only (every slab-binned forward
                                                 leaves the binning counters in it zeroed again): the per-frame zero-fill launch is skipped.
                                                 0: no assumption (a fresh, uninitialised buffer is fine) */
    float* gt_stats;                          /* lambda_dssim > 0, optional (NULL = off): igs_ssim_gt_stats_bytes(width, height) bytes that belong to
                                                 THIS ground-truth image.  loss_utils.py:34-63 blurs gt and gt^2 again in every iteration; with a
                                                 buffer the step that finds gt_stats_valid == 0 stores the two maps in it and every later step on the
                                                 same gt (gt_stats_valid != 0) reads them instead of recomputing them -- same values, 3 blurs for 5 */
    int gt_stats_valid;
    void* color_ready_event;                  /* optional hipEvent_t (with grad_out and color_grad_out, multi-GPU): color_grad_out is then written
                                                 right after the blend backward -- one kernel before the step ends -- and this event is recorded on
                                                 `stream` behind it, so that the caller can start the all-gather of the colour gradients on another
                                                 stream underneath the per-Gaussian kernel.  NULL: written by the last kernel of the step.
                                                 Queue the wait on the event only AFTER igs_refine_step has returned: in the rare frame that is
                                                 redone with larger slabs the event is recorded twice, and only the second record is behind valid data */
} igs_refine_step_args;
int igs_refine_step(const igs_refine_step_args* args);
size_t igs_refine_step_args_size(void);       /* sizeof(igs_refine_step_args) of the loaded library: bindings check it before the first call */

/* Masked refinement (the `refine_item` of the reference's GaussianModel.load_fromstream): only part of the model is trained.
 * The store is partitioned by the caller: Gaussians [0, first_trainable) are frozen, [first_trainable, P) are trained.  A frozen
 * Gaussian still renders and still occludes the others; its parameters and Adam moments are not touched.  `frozen_groups` freezes
 * whole parameter groups of the trained Gaussians as well (no_shs / no_opacity / no_scaling); xyz and rotation are always trained.
 * The blend backward forms no moments for frozen splats, the per-Gaussian backward and Adam run over [first_trainable, P) only, and
 * only those rows of the accumulator workspace are used.  m == NULL or {0, 0}: exactly igs_refine_step.
 * IGS_RAST_E_INVALID (before any HIP call) for first_trainable outside [0, P], unknown group bits, a frozen xyz / rotation,
 * and for grad_out / color_grad_out / dL_dmean2D combined with a mask that freezes anything. */
#define IGS_GROUP_XYZ      1u
#define IGS_GROUP_ROT      2u
#define IGS_GROUP_SH       4u
#define IGS_GROUP_OPACITY  8u
#define IGS_GROUP_SCALE   16u
typedef struct igs_refine_mask_args {
    int first_trainable;                      /* Gaussians [0, first_trainable) are frozen; 0 = all trainable */
    unsigned frozen_groups;                   /* IGS_GROUP_SH | IGS_GROUP_OPACITY | IGS_GROUP_SCALE (xyz / rotation cannot be frozen) */
} igs_refine_mask_args;
int igs_refine_step_masked(const igs_refine_step_args* args, const igs_refine_mask_args* m);
size_t igs_refine_mask_args_size(void);       /* sizeof(igs_refine_mask_args) of the loaded library */

/* Multi-GPU refine step (extension; views are sharded over the ranks): dL/dSH of the step = sum over its views of
 * basis(direction_v) x dL/dcolour_v (backward.cu:21-140, the W(k, b) rows of the SH backward).  Every rank all-gathers the
 * 3-float colour gradients of all views (`color_grad_out` of igs_refine_step: 12 bytes per Gaussian and view instead of a
 * 192-byte SH gradient in an all-reduce) and rebuilds the sum itself, views in the order given -- identical bits on every rank.
 *   campos [n_views][3] in HOST memory (read before the call returns; n_views <= 64), color_grads [n_views][P][3] and means3D on the
 *   device, dL_dsh [P][M][3] (overwritten), clamp_grads as in igs_refine_step.  A view whose three colour gradients of a Gaussian are
 *   zero (either sign) does not see it; rows at or beyond (D + 1)^2 and Gaussians no view sees are +0; a NaN colour gradient makes
 *   that Gaussian's rows NaN, through the clamp too (as torch.clamp), and touches no other Gaussian. */
int igs_sh_grad_from_view_colors(void* stream, int P, int D, int M, int n_views, const float* means3D, const float* campos,
                                 const float* color_grads, float clamp_grads, float* dL_dsh);
/* The same sum applied directly as the Adam update of the SH coefficients (torch.optim.Adam semantics as igs_adam_step_groups:
 * lr / bias_correction1, sqrt(v) / bias_correction2_sqrt + eps); param_sh / exp_avg_sh / exp_avg_sq_sh = the [P][M][3] SH spans of
 * the optimiser state.  The rebuilt gradient is never written to memory. */
int igs_adam_sh_from_view_colors(void* stream, int P, int D, int M, int n_views, const float* means3D, const float* campos,
                                 const float* color_grads, float clamp_grads, float* param_sh, float* exp_avg_sh, float* exp_avg_sq_sh,
                                 float lr, float beta1, float beta2, float eps, float bias_correction1, float bias_correction2_sqrt);
/* The whole optimiser step of an N > 1 rank in one launch, after the exchange: the SH update as igs_adam_sh_from_view_colors plus the
 * four small groups (xyz, rotation, opacity, scale) from their all-reduced gradients in the flat `grad` buffer (same arithmetic as
 * igs_adam_step_groups).  Flat buffers and float offsets as in igs_refine_step_args; M = 0 skips the SH part. */
int igs_adam_exchange_step(void* stream, int P, int D, int M, int n_views, const float* campos, const float* color_grads,
                           float clamp_grads, float* param, float* exp_avg, float* exp_avg_sq, const float* grad,
                           size_t off_xyz, size_t off_rot, size_t off_sh, size_t off_opacity, size_t off_scale,
                           float lr_xyz, float lr_rot, float lr_sh, float lr_opacity, float lr_scale,
                           float beta1, float beta2, float eps, float bias_correction1, float bias_correction2_sqrt);
size_t igs_refine_loss_scratch_bytes(int width, int height);

/* Photometric loss of the refine loop, forward + backward in two launches (igs/utils/loss_utils.py:17-63; infer_batch.py:300-306):
 *   loss = weight * ((1 - lambda_dssim) * mean|pred - gt| + lambda_dssim * (1 - mean SSIM(pred, gt))),   grad = dloss/dpred.
 * SSIM: 11x11 Gaussian window (sigma 1.5), zero padding, C1 = 1e-4, C2 = 9e-4, mean over all elements.  `scratch` holds
 * igs_ssim_l1_scratch_bytes(width, height) bytes.  `sums` (device, 2048 floats, or NULL) receives the 64 SSIM-sum shards at
 * [16*s] and the 64 L1-sum shards at [1024 + 16*s]; the caller adds them up and forms the loss value. */
size_t igs_ssim_l1_scratch_bytes(int width, int height);
int igs_ssim_l1_loss_fwd_bwd(void* stream, int width, int height, const float* pred, const float* gt, float lambda_dssim, float weight,
                             void* scratch, float* grad, float* sums);
/* The same with a cache of the two statistics that depend on the ground truth alone, blur(gt) and blur(gt^2) (the reference blurs them
 * again in every iteration; gt does not change while a frame is refined): `gt_stats` = igs_ssim_gt_stats_bytes(width, height) bytes
 * owned by the caller, one buffer per ground-truth image.  gt_stats_valid == 0: computed as usual AND stored; != 0: read (3 blurs
 * instead of 5).  Same values either way.  gt_stats == NULL: igs_ssim_l1_loss_fwd_bwd. */
size_t igs_ssim_gt_stats_bytes(int width, int height);
int igs_ssim_l1_loss_fwd_bwd_cached(void* stream, int width, int height, const float* pred, const float* gt, float lambda_dssim, float weight,
                                    void* scratch, float* grad, float* sums, float* gt_stats, int gt_stats_valid);
/* The SSIM term alone with its VALUE finished on the device: mean_out[0] = mean SSIM(pred, gt) over all 3 * width * height elements,
 * grad = d(mean SSIM)/d pred; same scratch as igs_ssim_l1_loss_fwd_bwd, two launches, nothing for the host to add up
 * (igs_amd.losses.ssim; loss_utils.py:34-63). */
int igs_ssim_mean_fwd_bwd(void* stream, int width, int height, const float* pred, const float* gt, void* scratch, float* grad,
                          float* mean_out);

/* SSIM and L1 of a BATCH of images, forward + backward: the AGM-Net training loss (igs/utils/loss_utils.py:17-18,33-63; main.py:252-265;
 * ssim_batch.hip).  pred, gt: [images][channels][H][W] float32, contiguous (4-byte alignment is enough).
 *   means    [images + 1]: mean SSIM of every image over its channels * H * W elements, then the mean of those, added in index order.
 *   l1_means [images + 1] (NULL allowed): the same for |pred - gt|.
 *   grad     (NULL = forward only: the derivative maps are neither written nor read and the gradient launch is skipped; a wanted
 *            l1_means then comes from the first launch): [images][channels][H][W], every element written,
 *              grad[n] = c_ssim * d(mean SSIM of image n)/d pred + c_l1 * d(mean |pred - gt| of image n)/d pred.
 *   ssim_map (NULL allowed): [images][channels][H][W], the SSIM value at every pixel.
 *   scratch  igs_ssim_batch_scratch_bytes(width, height, images, channels, grad != NULL) bytes, 256-byte aligned; need not be initialised.
 * Three launches with a gradient, two without; no host synchronisation and no allocation, so the call can be captured into a graph.
 * Every workgroup leaves its tile's sums in scratch and one workgroup of the last launch adds them per image in an order that depends on
 * (channels, width, height) alone: no atomics, two runs agree bit for bit, and an image's mean, map and gradient have the same bits alone
 * and at any position of any batch.  The forward-only instances give the means and the map of the gradient instances bit for bit.
 *   - Refused with IGS_RAST_E_INVALID and a message before any HIP call: a non-positive width, height, images or channels; images * channels
 *     above IGS_SSIM_BATCH_MAX_PLANES; a grid 8 * images * channels * ceil(ceil(H / 32) / 8) * ceil(W / 32) that does not fit in 31 bits;
 *     a NULL pred, gt, scratch or means.  igs_ssim_batch_scratch_bytes returns -1 for the sizes the call would refuse; without want_grad it
 *     holds the tile sums only (no derivative maps). */
#define IGS_SSIM_BATCH_MAX_PLANES (1 << 16)
long long igs_ssim_batch_scratch_bytes(int width, int height, int images, int channels, int want_grad);
int igs_ssim_batch_fwd_bwd(void* stream, int width, int height, int images, int channels, const float* pred, const float* gt,
                           float c_ssim, float c_l1, void* scratch, float* means, float* l1_means, float* grad, float* ssim_map);

/* RaDe-GS depth-normal consistency regulariser, value and gradients in one launch
 * (submodules/RaDe-GS/utils/graphics_utils.py:97-126, train.py:143-160):
 *   loss = weight * ((1 - depth_ratio) * mean(1 - normal . n(depth)) + depth_ratio * mean(1 - normal . n(mdepth))),
 * n(d) = normalised cross product of the central differences of the back-projected depth map (zero on the image border).
 * Writes dloss/ddepth [H][W], dloss/dmdepth [H][W], dloss/dnormal [3][H][W]; the loss value is left as 64 partial sums at
 * loss_shards[16*s] (1024 floats, zero-filled here). */
int igs_depth_normal_loss_fwd_bwd(void* stream, int width, int height, float tan_fovx, float tan_fovy, const float* depth,
                                  const float* mdepth, const float* normal, float weight, float depth_ratio, float* g_depth,
                                  float* g_mdepth, float* g_normal, float* loss_shards);

/* Fused L1 loss forward + backward (igs/utils/loss_utils.py:17-18): grad[i] = sign(pred[i] - gt[i]) * scale, and
 * sum |pred - gt| is accumulated into 64 shards loss_sum[16*s], s = 0..63 (1024 floats, zeroed by the caller, summed by
 * the caller: same-address atomics would serialise). */
int igs_l1_loss_fwd_bwd(void* stream, size_t n, const float* pred, const float* gt, float* grad, float* loss_sum, float scale);
/* The same with the VALUE finished on the device, in one launch: mean_out[0] = mean |pred - gt|, grad[i] = sign(pred[i] - gt[i]) / n.
 * partials: 1024 floats of scratch; counter: 33 * 64 words (2112) that are zero on entry and zero again on exit (a buffer the caller zero-fills once
 * and keeps; calls that share it must be ordered on one stream). */
int igs_l1_mean_fwd_bwd(void* stream, size_t n, const float* pred, const float* gt, float* grad, float* mean_out, float* partials,
                        unsigned* counter);

/* On-disk format <-> parameter store on the device (extension).  The host reads / writes the file; these do the
 * per-Gaussian re-layout and arithmetic of igs/models/gs.py:400-462 (load_ply) and :297-343 (save_ply) in one pass each.
 *   igs_ply_to_params: `table` = the PLY's vertex element as [P][stride] float32 on the device; `cols` (HOST memory, n_cols = 15 + 3 (K - 1)
 *     entries) = the column of x y z | f_dc_0..2 | f_rest_0 .. f_rest_{3(K-1)-1} | opacity | scale_0..2 | rot_0..3 | filter_3D (-1: absent).
 *     Writes xyz [P,3], rotation [P,4], shs [P,K,3] (the file is channel-major), opacity [P] (logit), scaling [P,3] (log); with a filter_3D
 *     column the Mip-Splatting filter is folded in exactly as gs.py:480-490 + inverse_sigmoid / log (:451-455).
 *   igs_params_to_ply: the [P][14 + 3 K] table save_ply writes (normals zero, f_dc / f_rest channel-major). */
int igs_ply_to_params(void* stream, int P, const float* table, int stride, const int* cols, int n_cols, int K,
                      float* xyz, float* rotation, float* shs, float* opacity, float* scaling);
int igs_params_to_ply(void* stream, int P, int K, const float* xyz, const float* rotation, const float* shs, const float* opacity,
                      const float* scaling, float* table);

/* Morton (Z-order) permutation of the Gaussians' positions (extension, no reference counterpart; used by the refine loop's store so
 * that consecutive Gaussians project to neighbouring tiles -- the binning stage then reserves instance slots once per (workgroup,
 * tile) instead of once per instance).  perm[i] = index of the Gaussian that comes i-th; ties keep their order (stable radix sort
 * of the library itself, no PyTorch / rocPRIM sort on the stream path).  lohi: {lo.xyz, hi.xyz} of the positions, 6 floats in
 * DEVICE memory; bits: 1..10 per axis; scratch: igs_morton_order_scratch_bytes(P) bytes. */
size_t igs_morton_order_scratch_bytes(int P);

/* Test support: the per-tile sort of the slab binning (the replacement of cub::DeviceRadixSort::SortPairs + identifyTileRanges,
 * rasterizer_impl.cu:373-391, for instances that were binned per tile) on caller-made slabs.  tile_count[T]: instances per tile (reset
 * to zero by the call); pairs[T * slab]: depth bits << 32 | Gaussian id; out: point_list[T * slab] = the ids of every tile's slab in
 * ascending key order, ranges[2 T] = {t * slab, t * slab + count} (empty for a tile whose count exceeds `slab`), stats[4]: [1] = the
 * largest such count.  ids are clamped to P - 1.  All pointers DEVICE memory. */
int igs_debug_tile_sort(void* stream, int T, unsigned int* tile_count, const unsigned long long* pairs, unsigned int* point_list,
                        unsigned int* ranges, int slab, unsigned int* stats, int P);
int igs_morton_order(void* stream, int P, const float* xyz, const float* lohi, int bits, void* scratch, int* perm);

/* Mean squared distance to the three nearest neighbours: simple-knn's distCUDA2 (the "simple-knn" package of 3DGS, spatial.cu), which
 * RaDe-GS's create_from_pcd uses for the initial scales: out[i] = (b0 + b1 + b2) / 3.0f in float32, left to right, where b0 <= b1 <= b2
 * are the three smallest SQUARED distances |p_i - p_j|^2 over j != i (a different index: duplicates count, at distance 0).
 *   - N <= 3: the slots without a neighbour hold FLT_MAX (simple-knn's best[3] = {FLT_MAX, ...}): N = 1 and N = 2 give +inf, N = 3
 *     gives (b0 + b1 + FLT_MAX) / 3.0f = FLT_MAX / 3.
 *   - non-finite input (a NaN or +-inf coordinate): such a point is never a neighbour of a finite point, so a finite point with at
 *     least three finite neighbours gets the value it would get without the non-finite points; the non-finite points' own outputs are
 *     unspecified.  No fault, no hang.
 *   - exact search (boxes only skip candidates that provably cannot enter the three smallest), bit-identical from run to run and
 *     under any permutation of the points.
 * xyz: P x 3 float32, out: P float32, scratch: igs_knn_scratch_bytes(P) bytes, all DEVICE memory; everything is enqueued on `stream`,
 * no host synchronisation, no device allocation.  0 <= P <= IGS_KNN_MAX_POINTS; P == 0 returns 0 and launches nothing (NULL pointers
 * allowed); otherwise a NULL pointer or a P out of range returns IGS_RAST_E_INVALID before any HIP call.  igs_knn_scratch_bytes
 * returns 0 for a P out of range. */
#define IGS_KNN_MAX_POINTS (1 << 25)
size_t igs_knn_scratch_bytes(int P);
int igs_knn_mean_dist2(void* stream, int P, const float* xyz, void* scratch, float* out);

/* The anchor graph of IGS's AGM-Net (igs/models/gs.py get_mask_fpsample; the torch_cluster and fpsample drop-ins): in-box selection,
 * exact farthest-point sampling and batched k nearest neighbours (anchors.hip).  Common rules of the three entry points:
 *   - points are float32 xyz triples (D = 3 only); examples are contiguous runs given by ptr[B + 1] (int32, ptr[0] = 0, ascending,
 *     ptr[B] = the number of points), read on the device only;
 *   - every pointer is DEVICE memory, everything is enqueued on `stream`, no host synchronisation, no device allocation;
 *   - sizes out of range or a NULL required pointer return IGS_RAST_E_INVALID before any HIP call; a call with nothing to compute
 *     returns 0 and launches nothing.  The *_scratch_bytes functions return 0 for sizes out of range.
 *   - distances: d2 = fma(dz, dz, fma(dy, dy, dx * dx)) in float32 for every candidate (knn.hip's expression).
 *
 * igs_bbox_select: for every example b keeps the points with box[6b + a] <= p[a] <= box[6b + 3 + a] on all three axes (a NaN
 *   coordinate is outside), in ascending index order (torch.where): out_xyz [N x 3] and out_idx [N] (int64, the index inside the
 *   example) hold example 0's points, then example 1's, ...; out_count[B] (int32) the counts.  Entries past the total are unwritten.
 *   scratch: igs_bbox_select_scratch_bytes(N).  1 <= B <= IGS_ANCHOR_MAX_EXAMPLES, 0 <= N <= IGS_ANCHOR_MAX_POINTS.
 *
 * igs_fps: vanilla farthest-point sampling per example: sel[0] = start[b] (an index inside the example; out of range: 0); cur[i] =
 *   init_d2 for every finite point (-inf for a point with a non-finite coordinate: never selected while a finite point is left, never
 *   lowers another); step s: cur[i] = min(cur[i], d2(i, sel[s-1])), sel[s] = argmax cur, ties to the lowest index.  Example b takes
 *   out_ptr[b + 1] - out_ptr[b] samples into out[out_ptr[b] ...] (int64, indices into the whole xyz array, selection order); out
 *   holds `total` entries (normally out_ptr[B]) and nothing past them is written; total == 0 launches nothing.  Exact: the
 *   same sequence as the restatement whatever the spatial order.  max_n must bound every example's size (the
 *   launch is shaped by it); an example larger than max_n, or an empty one, gets -1 samples.  init_d2 >= 0 (+inf allowed).
 *   scratch: igs_fps_scratch_bytes(B, N, max_n).  1 <= B <= IGS_ANCHOR_MAX_EXAMPLES, 0 <= N <= IGS_ANCHOR_MAX_POINTS,
 *   0 <= max_n <= IGS_FPS_MAX_EXAMPLE_POINTS.
 *
 * igs_knn_query: torch_cluster's knn: for every query y[j] of example b the k nearest x[i] of the same example (ptr_x / ptr_y give the
 *   examples of x and y), ordered by (d2, i) ascending; a candidate counts only if d2 < 1e10 (NaN never).  out_idx [Ny x k] int64:
 *   indices into x, -1 in the slots without a neighbour; out_d2 [Ny x k] (or NULL): d2, +inf in empty slots; out_w [Ny x k] (or
 *   NULL): softmax(-weight_scale * sqrt(d2)) over the filled slots, 0 in empty ones.  No scratch.  1 <= k <= IGS_KNN_QUERY_MAX_K,
 *   1 <= B <= IGS_ANCHOR_MAX_EXAMPLES, 0 <= Nx, Ny <= IGS_ANCHOR_MAX_POINTS. */
#define IGS_ANCHOR_MAX_POINTS (1 << 26)
#define IGS_ANCHOR_MAX_EXAMPLES (1 << 16)
#define IGS_FPS_MAX_EXAMPLE_POINTS (1 << 22)
#define IGS_KNN_QUERY_MAX_K 100
size_t igs_bbox_select_scratch_bytes(int N);
int igs_bbox_select(void* stream, int B, int N, const float* xyz, const int* ptr, const float* box, void* scratch, float* out_xyz,
                    int64_t* out_idx, int* out_count);
size_t igs_fps_scratch_bytes(int B, int N, int max_n);
int igs_fps(void* stream, int B, int N, int max_n, const float* xyz, const int* ptr, const int* start, const int* out_ptr, int total,
            float init_d2, void* scratch, int64_t* out);
int igs_knn_query(void* stream, int B, int Nx, int Ny, const float* x, const float* y, const int* ptr_x, const int* ptr_y, int k,
                  float weight_scale, int64_t* out_idx, float* out_d2, float* out_w);

/* The two consumers of the anchor graph (motion.hip): anchor feature interpolation (the tail of
 * GS3DRenderer.query_ir_grid, igs/models/gs.py:812-822) and the Gaussian deform (GaussianModel.deform, gs.py:347-375, with
 * quaternion_multiply, igs/utils/general_utils.py:177-200).  Common rules of the six entry points:
 *   - every pointer is DEVICE memory, everything is enqueued on `stream`, no host synchronisation, no device allocation;
 *   - sizes out of range, an unknown dtype code or a NULL required pointer return IGS_RAST_E_INVALID before any HIP call; a call with
 *     nothing to compute (N == 0, M == 0 and P == 0, ...) returns 0 and launches nothing.  igs_anchor_interp_index_bytes returns 0 for
 *     sizes out of range;
 *   - dtype codes: IGS_DTYPE_F32 (float) or IGS_DTYPE_F16 (IEEE half); arithmetic is float32 throughout, half inputs are widened on
 *     load and half outputs rounded once, to nearest even.
 *
 * igs_anchor_interp_fwd: out[n, d] = sum over k = 0 .. K-1 of w[n, k] * F[col[n, k], d], accumulated in float32 in slot order
 *   (fmaf).  F [A_total x D] in `dtype` (the flattened [B, A, D] anchor features; col indexes the flattened rows, so example i's
 *   columns are offset by i * A as in IGS.forward), col [N x K] int64, w [N x K] float32, out [N x D] float32.  A slot whose col is -1
 *   or outside [0, A_total) contributes nothing (its weight is not read).  No scratch.
 *   0 <= N <= IGS_INTERP_MAX_ROWS, 1 <= K <= IGS_INTERP_MAX_K, 1 <= D <= IGS_INTERP_MAX_D, 1 <= A_total <= IGS_INTERP_MAX_ANCHORS,
 *   N * K <= IGS_INTERP_MAX_EDGES.
 * igs_anchor_interp_index: builds the inverse index of col (per anchor, its incoming edges e = n * K + k in ascending e order: a stable
 *   radix sort by anchor, per-anchor starts and chunk offsets) into `scratch` of igs_anchor_interp_index_bytes(N, K, A_total, D) bytes;
 *   the same scratch also holds the backward's chunk partials for that D.  Limits as for the forward.
 * igs_anchor_interp_bwd: dF[a, d] = sum over the edges (n, k) with col[n, k] = a, in ascending (n, k) order, of w[n, k] * dout[n, d]
 *   (lists of more than one chunk are summed per chunk, then the chunk sums in chunk order), written in `dtype` (NULL: skipped; an
 *   anchor without edges gets 0); dw[n, k] = <dout[n, :], F[col[n, k], :]> in float32 (NULL: skipped; 0 for a -1 or out-of-range
 *   slot).  No float atomics: bitwise reproducible.  `scratch` must hold the index igs_anchor_interp_index built for the same col,
 *   N, K, A_total and D (the index is read, not changed: several backward calls may share it).
 *
 * igs_gaussian_deform_fwd: xyz [P x 3] and rot [P x 4] float32; mask [M] int64, distinct indices in [0, P) (an index outside is
 *   skipped); dxyz [M x 3] and drot [M x 4] in `dtype`.  Row i = mask[j] of xyz_out gets xyz[i] + dxyz[j], of rot_out
 *   qmul(nrm(rot[i]), nrm(drot[j])) with nrm(q) = q / max(|q|, 1e-12) (F.normalize) and qmul the Hamilton product in
 *   quaternion_multiply's order; every other row is copied bit for bit (nothing is copied when xyz_out == xyz, rot_out == rot: in place).
 *   Two launches: the pass-through copy of both tensors, then the masked rows.  0 <= M <= P <= IGS_DEFORM_MAX_POINTS.
 * igs_gaussian_deform_bwd: the gradients of that map for the upstream g_xyz [P x 3] and g_rot [P x 4] (float32; NULL = zero):
 *   d_xyz [P x 3] = g_xyz; d_rot [P x 4] = g_rot outside the mask and the gradient through qmul and nrm(rot[i]) on it; d_dxyz [M x 3]
 *   = g_xyz[mask[j]] and d_drot [M x 4] through qmul and nrm(drot[j]), both in `dtype` (zero rows for a skipped index).  Through
 *   nrm: (g - n <n, g>) / |q| where |q| >= 1e-12, g / 1e-12 below (F.normalize's clamp: division by the constant eps).  Any output
 *   may be NULL.  Two launches: the pass-through copy, then the masked rows.  Same limits as the forward. */
#define IGS_DTYPE_F32 0
#define IGS_DTYPE_F16 1
#define IGS_INTERP_MAX_ROWS (1 << 24)
#define IGS_INTERP_MAX_K 100
#define IGS_INTERP_MAX_D 1024
#define IGS_INTERP_MAX_ANCHORS (1 << 24)
#define IGS_INTERP_MAX_EDGES (1 << 30)
#define IGS_DEFORM_MAX_POINTS (1 << 26)
int igs_anchor_interp_fwd(void* stream, int N, int K, int D, int A_total, int dtype, const void* F, const int64_t* col, const float* w,
                          float* out);
size_t igs_anchor_interp_index_bytes(int N, int K, int A_total, int D);
int igs_anchor_interp_index(void* stream, int N, int K, int A_total, int D, const int64_t* col, void* scratch);
int igs_anchor_interp_bwd(void* stream, int N, int K, int D, int A_total, int dtype, const void* F, const float* w, const float* dout,
                          void* scratch, void* dF, float* dw);
int igs_gaussian_deform_fwd(void* stream, int P, int M, int dtype, const float* xyz, const float* rot, const int64_t* mask,
                            const void* dxyz, const void* drot, float* xyz_out, float* rot_out);
int igs_gaussian_deform_bwd(void* stream, int P, int M, int dtype, const float* rot, const int64_t* mask, const void* drot,
                            const float* g_xyz, const float* g_rot, float* d_xyz, float* d_rot, void* d_dxyz, void* d_drot);

/* Multi-view anchor feature lifting (lift.hip): GridEncoder.forward's "perspective_projection" branch
 * (igs/models/grid_encoder.py:66-88) through perspective_projection (igs/utils/ops.py:444-477) and the mean over the views.
 * For example b, anchor a, channel c, with (R_v, T_v) the top three rows of w2c[b * V + v] and (fx, fy, cx, cy) = intr[b * V + v]:
 *
 *   out[b, a, c] = (1 / V) * sum over v = 0 .. V-1 of bilinear_zero_pad(feat[b * V + v, c, :, :], ix, iy)
 *   p_cam = R_v * p[b, a] + T_v
 *   u = (fx * p_cam.x + cx * p_cam.z) / p_cam.z,  v = (fy * p_cam.y + cy * p_cam.z) / p_cam.z      (K * p_cam first, then / z)
 *   ix = ((2 u / W - 1 + 1) * W - 1) / 2,  iy likewise with H      (grid_sample: bilinear, align_corners=False, padding_mode="zeros")
 *
 *   - no culling: a point with negative p_cam.z is divided by it like any other and its mirrored projection is sampled;
 *   - the mean is over all V views, including those whose sample fell outside the map (they add zero);
 *   - a corner outside the map contributes zero, the other corners of the sample still count;
 *   - deviation: a sample whose ix or iy is not finite (z = 0, overflow) contributes zero (the reference hands NaN / inf to grid_sample);
 *     the coordinates are range-tested in float (-1 < ix < W, -1 < iy < H) before any conversion to integer;
 *   - float32 arithmetic throughout; per anchor the views are added in view order and the corners in the order (x0, y0), (x0 + 1, y0),
 *     (x0, y0 + 1), (x0 + 1, y0 + 1) with fmaf (maps larger than one LDS band: band by band in row order), then one division by V.
 * Common rules: every pointer is DEVICE memory, everything is enqueued on `stream`, no host synchronisation, no device allocation;
 * sizes out of range, an unknown dtype code, a stride pattern that is not supported or a NULL required pointer return
 * IGS_RAST_E_INVALID with a message (igs_rast_last_error) before any HIP call; a call with nothing to do (A == 0 or B == 0) returns 0
 * without a launch (the backward with A == 0 and B > 0 zero-fills d feat).  The two *_scratch_bytes return 0 for sizes out of range.
 * Limits: 0 <= B, 0 <= A, B * A <= IGS_LIFT_MAX_SAMPLES, 1 <= V <= IGS_LIFT_MAX_V, 1 <= C <= IGS_LIFT_MAX_C,
 * 1 <= H, W <= IGS_LIFT_MAX_HW, B * V * H * W <= IGS_LIFT_MAX_PIXELS.
 *
 * igs_anchor_lift_fwd: feat [B*V, C, H, W] in `dtype` (IGS_DTYPE_F32 / IGS_DTYPE_F16, widened on load) with element strides fs_*: every
 *   H x W plane must be contiguous (fs_w == 1, fs_h == W; fs_n and fs_c are free, so slices of n and c are read in place).
 *   Channels-last (fs_c == 1) and every other pattern are refused with a message: there are no kernels for them in this version, the
 *   caller makes the tensor plane-contiguous.  points [B, A, 3] float32; w2c [B*V, 4, 4] float32 row-major (the inverse of the
 *   camera-to-world matrices); intr [B*V, 4] float32 = fx, fy, cx, cy.  out float32 at out[b * A * C + a * os_a + c * os_c] with
 *   (os_a, os_c) = (1, A) (a [B, C, A] buffer, what GridEncoder's conv reads) or (C, 1) ([B, A, C]).  `scratch` of
 *   igs_anchor_lift_scratch_bytes(...) bytes receives the sample table.  Two launches.
 * igs_anchor_lift_bwd: d feat[n, c, y, x] = (1 / V) * sum of w * d out[b, a, c] over the (anchor, corner) pairs of view n = b * V + v
 *   that touch pixel (y, x), in ascending (a, corner) order with fmaf, then one division by V, rounded once to `dtype`.  No float
 *   atomics: bitwise reproducible.  EVERY element of d feat is written (zero where no sample landed), so the caller need not clear it.
 *   d out float32 at dout[b * A * C + a * gs_a + c * gs_c], (gs_a, gs_c) = (1, A) or (C, 1); d feat in `dtype` with strides as the
 *   forward's, planes not overlapping (fs_c >= H * W, fs_n >= C * fs_c).  The sample table is recomputed from points / w2c / intr (the
 *   features themselves are not needed), so nothing has to be kept from the forward; `scratch` of
 *   igs_anchor_lift_bwd_scratch_bytes(...) bytes holds the table and the inverse index (edges sorted by pixel with the library's
 *   stable radix sort).  A workgroup keeps two channels of d out[b] in 64 KB of LDS while 2 * A floats fit (A <= 8192); for larger A it
 *   reads d out from global memory per edge instead (same result, slower).  Gradients to points, poses and intrinsics are not provided. */
#define IGS_LIFT_MAX_C 1024
#define IGS_LIFT_MAX_V 16
#define IGS_LIFT_MAX_HW 2048
#define IGS_LIFT_MAX_PIXELS (1 << 24)
#define IGS_LIFT_MAX_SAMPLES (1 << 24)
size_t igs_anchor_lift_scratch_bytes(int B, int V, int A, int C, int H, int W, int dtype);
size_t igs_anchor_lift_bwd_scratch_bytes(int B, int V, int A, int C, int H, int W, int dtype);
int igs_anchor_lift_fwd(void* stream, int B, int V, int A, int C, int H, int W, int dtype, const void* feat, long long fs_n, long long fs_c,
                        long long fs_h, long long fs_w, const float* points, const float* w2c, const float* intr, float* out,
                        long long os_a, long long os_c, void* scratch);
int igs_anchor_lift_bwd(void* stream, int B, int V, int A, int C, int H, int W, int dtype, const float* points, const float* w2c,
                        const float* intr, const float* dout, long long gs_a, long long gs_c, void* dfeat, long long fs_n, long long fs_c,
                        long long fs_h, long long fs_w, void* scratch);

/* Ray conditioning and fused LayerNorm + modulation (cond.hip): the non-GEMM parts of IGS.condition3D
 * (igs/IGS.py:185-210 with ray_to_plucker :286-295, rsh_cart_3 :297-344, ModLN :259-284; local_ray False).  Everything runs on `stream`,
 * reads nothing back and allocates nothing.  Sizes out of range, an unknown dtype code, a stride pattern that is not supported or a NULL
 * required pointer return IGS_RAST_E_INVALID with a message before any HIP call; N == 0 returns 0 without a launch.
 * Limits: 0 <= N, N * H * W <= IGS_COND_MAX_PIXELS, 1 <= H, W, Hd, Wd <= IGS_COND_MAX_HW, 1 <= C <= IGS_MODLN_MAX_C.
 *
 * igs_ray_condition_fwd: rays [N, H, W, 6] float32 = (origin, direction) per pixel of the N = B * V views, depth [N, Hd, Wd] float32, both
 *   contiguous; cond [N, H, W, 33] float32.  d = direction / max(|direction|, 1e-12), m = origin x d (not normalised).  Channels 0-15: the
 *   real spherical harmonics of degree <= 3 of d, index n (n + 1) + m, odd orders negated; 16-31: the same polynomials of m; 32: depth
 *   resized bilinearly to H x W with half-pixel centres (source coordinate max((i + 0.5) Hd / H - 0.5, 0), upper neighbour clamped to the
 *   last row / column, no antialiasing).  One launch; every 132-byte row leaves through LDS as part of one contiguous run per workgroup.
 * igs_modln_fwd: x [N, C, H, W] in x_dtype (IGS_DTYPE_F32 / IGS_DTYPE_F16, widened on load) with element strides xs_* under
 *   igs_anchor_lift_fwd's rule (every H x W plane contiguous; xs_n, xs_c free); mod [N, H, W, 2 C] contiguous in mod_dtype, shift =
 *   mod[..., :C], scale = mod[..., C:]; weight, bias [C] float32; out [N, C, H, W] float32 contiguous:
 *     out = ((x - mu) * r * weight + bias) * (1 + scale) + shift,  mu = mean_c x,  r = 1 / sqrt(mean_c (x - mu)^2 + eps)
 *   (the biased variance, from centred values), all in float32.  mean, rstd [N, H, W] float32 receive mu and r for the backward when both
 *   are given (both or neither).  One launch; a workgroup takes 64 consecutive pixels and all channels while C <= 244, fewer pixels above.
 * igs_modln_bwd: from x, mod, weight, bias, the saved mean / rstd and gout = d out [N, C, H, W] float32 contiguous, each output optional
 *   (NULL = not wanted): dx [N, C, H, W] contiguous in x_dtype; dmod [N, H, W, 2 C] in mod_dtype (d shift = gout, d scale = gout * y, y the
 *   normalised value with the affine applied); dweight, dbias [C] float32, summed without float atomics: every workgroup leaves a row of
 *   partial sums in `scratch` (igs_modln_bwd_scratch_bytes(...) bytes, needed only for these two), a second launch adds the rows in
 *   workgroup order, so two runs agree bit for bit. */
#define IGS_COND_MAX_PIXELS (1 << 24)
#define IGS_COND_MAX_HW 8192
#define IGS_MODLN_MAX_C 1024
int igs_ray_condition_fwd(void* stream, int N, int H, int W, int Hd, int Wd, const float* rays, const float* depth, float* cond);
size_t igs_modln_bwd_scratch_bytes(int N, int C, int H, int W);
int igs_modln_fwd(void* stream, int N, int C, int H, int W, int x_dtype, const void* x, long long xs_n, long long xs_c, long long xs_h,
                  long long xs_w, int mod_dtype, const void* mod, const float* weight, const float* bias, float eps, float* out, float* mean,
                  float* rstd);
int igs_modln_bwd(void* stream, int N, int C, int H, int W, int x_dtype, const void* x, long long xs_n, long long xs_c, long long xs_h,
                  long long xs_w, int mod_dtype, const void* mod, const float* weight, const float* bias, const float* mean, const float* rstd,
                  const float* gout, void* dx, void* dmod, float* dweight, float* dbias, void* scratch);

/* IGS.condition3D's forward in one launch (cond_fused.hip).  Per pixel of x [N, C, H, W]:
 *     cond = the 33 channels of igs_ray_condition_fwd, bit for bit (the two kernels share the statements)
 *     h    = SiLU(W1 cond + b1)                     W1 [hidden, 33]          (ModLN.mlp[0], SiLU = v / (1 + exp(-v)) as igs_mlp_heads_fwd's)
 *     mod  = W2 h + b2                              W2 [2 C, hidden]         (ModLN.mlp[2]); shift = mod[:C], scale = mod[C:]
 *     out  = ((x - mu) r weight + bias) (1 + scale) + shift                  mu, r as igs_modln_fwd defines them
 * Neither cond, h nor mod is stored.  Forward only: no saved statistics, no backward.  Runs on `stream`, reads nothing back, allocates
 * nothing, uses no atomics: two runs agree bit for bit, and a pixel's result depends on no other pixel, not on the grid and not on N.
 *   - x in x_dtype (IGS_DTYPE_F32 / IGS_DTYPE_F16, widened on load) under igs_modln_fwd's stride rule (every H x W plane contiguous; xs_n,
 *     xs_c free); rays [N, H, W, 6], depth [N, Hd, Wd] float32 contiguous as igs_ray_condition_fwd takes them; weight, bias [C] float32 (the
 *     LayerNorm's); out [N, C, H, W] float32 contiguous.
 *   - mlp_dtype selects the MLP instance, independently of x_dtype.  IGS_DTYPE_F32: v_mfma_f32_32x32x2_f32 over the first 32 condition
 *     channels and one fma per hidden channel for the depth channel, an exact float32 fma chain of 34 terms that starts from the bias, then
 *     v_mfma_f32_32x32x2_f32 for W2; no reduced-precision value anywhere.  IGS_DTYPE_F16: v_mfma_f32_32x32x16_f16, float32 accumulators that
 *     start from the bias, SiLU in float32; cond and h are rounded to half once each as the next product's operand (a condition value
 *     beyond the half range becomes inf), mod is NOT rounded: it goes from the accumulators into the float32 modulation.
 *   - wpack, in mlp_dtype: three Linears, each in igs_mlp_heads_fwd's tile order (ceil(O / 32) x ceil(I / 32) tiles of 1024 elements, output
 *     tile outermost, tile (ot, kt) = [chunk][lane 64][E], E = 8 (half) or 4 (float), element e = chunk E + j of lane (r, h) =
 *     W[32 ot + r][32 kt + (e & 3) + 8 (e >> 2) + 4 h], zero outside W), one after another: W1 [hidden, 33] (two k tiles per output tile),
 *     W2[:C] [C, hidden], W2[C:] [C, hidden].  igs_condition3d_pack_elems(C, hidden, mlp_dtype) = (2 ht + 2 ct ht) 1024 with
 *     ht = ceil(hidden / 32), ct = ceil(C / 32) is the element count (-1: C or hidden outside 1 .. IGS_COND_MLP_MAX_WIDTH, or an unknown
 *     dtype code).  bpack: float32 [3][128] = b1, b2[:C], b2[C:], zero-padded.
 *   - Refused with IGS_RAST_E_INVALID and a message before any HIP call: N, H, W, Hd, Wd outside igs_ray_condition_fwd's limits; C or
 *     hidden outside 1 .. IGS_COND_MLP_MAX_WIDTH; an unknown dtype code; a stride pattern igs_modln_fwd refuses; xs_c above
 *     IGS_COND_FUSED_MAX_STRIDE (the kernel adds a lane's channel and pixel offset in 32 bits); eps < 0 or NaN; with N > 0
 *     a NULL pointer, a pointer not aligned to its element, a wpack not aligned to 16 bytes.  N == 0 returns 0 without a launch.
 * One persistent workgroup of 8 waves per compute unit keeps the weights in LDS (float32: 147 KB); a wave owns 32 pixels of one image. */
#define IGS_COND_MLP_MAX_WIDTH 128
#define IGS_COND_FUSED_MAX_STRIDE (1LL << 27)
long long igs_condition3d_pack_elems(int C, int hidden, int mlp_dtype);
int igs_condition3d_fwd(void* stream, int N, int C, int hidden, int H, int W, int Hd, int Wd, int x_dtype, const void* x, long long xs_n,
                        long long xs_c, long long xs_h, long long xs_w, const float* rays, const float* depth, int mlp_dtype, const void* wpack,
                        const float* bpack, const float* weight, const float* bias, float eps, float* out);

/* The backward of igs_condition3d_fwd (cond_fused_bwd.hip).  The forward is recomputed from x, rays, depth and the
 * packs; with g = gout[:, p] the upstream gradient of a pixel and n = (x - mu) r weight + bias:
 *     d shift = g, d scale = g n, d n = g (1 + scale);  d weight += d n xh, d bias += d n;  d xh = d n weight,
 *     d x = r (d xh - mean_C(d xh) - xh mean_C(d xh xh));  d h = W2[:C]^T d shift + W2[C:]^T d scale, d z1 = d h silu'(z1);
 *     d W2 += [d shift ; d scale] (x) h, d b2 += [d shift ; d scale], d W1 += d z1 (x) cond, d b1 += d z1.
 * rays and depth get no gradient.  Every output may be NULL and is then neither computed nor stored: with only dx no weight-gradient or
 * reduce launch happens, without dx nothing of d x is computed, without dW1 and db1 the product with W2^T is left out.
 *   - x, rays, depth, mlp_dtype, wpack, bpack, weight, bias, eps: as igs_condition3d_fwd takes them, under the same limits and stride rule.
 *     gout [N, C, H, W] float32 contiguous.
 *   - wpack_t, in mlp_dtype: W2^T as ONE Linear in igs_mlp_heads_fwd's tile order, ht x 2 ct tiles with ht = ceil(hidden / 32),
 *     ct = ceil(C / 32): output j = hidden unit j, input 32 ct s + c = channel c of W2[:C] (s = 0) or of W2[C:] (s = 1), that is
 *     M[j][32 ct s + c] = W2[s C + c][j], zero elsewhere; 2 ct ht 1024 elements.  W1^T is never needed.
 *   - Outputs: dx [N, C, H, W] contiguous in x_dtype, rounded once; float32 row-major dW1 [hidden, 33], db1 [hidden], dW2 [2 C, hidden],
 *     db2 [2 C], dweight [C], dbias [C] -- nn.Linear's and nn.LayerNorm's layouts.
 *   - Numerics.  IGS_DTYPE_F32: v_mfma_f32_32x32x2_f32 everywhere, every output a float32 fma chain in a fixed order (the depth column of
 *     d W1 runs through the same product as the other 32).  IGS_DTYPE_F16: float32 accumulation, silu', LayerNorm backward and parameter
 *     sums; a value is rounded to half once, only as a matrix operand: cond and h as in the forward, g and g n for the product with W2^T
 *     and for d W2, d z1 for d W1.  silu' is igs_mlp_heads_bwd's clamped evaluation: finite inputs give finite results.
 *   - No float atomics: per-slice partials in pixel order, then a reduce launch in slice order; two runs agree bit for bit, and d x of an
 *     image depends on no other image.  A NaN in x or a ray of one pixel makes that pixel's d x NaN and leaves every other pixel's d x as
 *     it was; the parameter gradients become NaN.
 *   - scratch: as many bytes as igs_condition3d_bwd_scratch_bytes returns for these sizes (-1: out of range), aligned to 16.  The pixels are
 *     walked in chunks of IGS_COND_BWD_CHUNK_ROWS rows (a row is a lane of a 32-pixel group of one image, so an image takes
 *     32 ceil(H W / 32) rows): 7 float32 [rows][128] slots of one chunk plus at most IGS_COND_BWD_CHUNK_ROWS / 256 partials of the
 *     parameter gradients.  Above one chunk the size does not depend on N, H, W.
 *   - Refused with IGS_RAST_E_INVALID and a message before any HIP call: what igs_condition3d_fwd refuses, a misaligned output, wpack_t or
 *     scratch, scratch_bytes below the required size.  N == 0 returns 0 without a launch (the caller zero-fills). */
#define IGS_COND_BWD_CHUNK_ROWS 16384
long long igs_condition3d_bwd_scratch_bytes(int N, int C, int hidden, int H, int W);
int igs_condition3d_bwd(void* stream, int N, int C, int hidden, int H, int W, int Hd, int Wd, int x_dtype, const void* x, long long xs_n,
                        long long xs_c, long long xs_h, long long xs_w, const float* rays, const float* depth, int mlp_dtype, const void* wpack,
                        const void* wpack_t, const float* bpack, const float* weight, const float* bias, float eps, const float* gout,
                        void* scratch, long long scratch_bytes, void* dx, float* dW1, float* db1, float* dW2, float* db2, float* dweight,
                        float* dbias);

/* The 2x bilinear upsample and the 3x3 convolution of the motion features in one launch (upconv.hip; DESIGN.md section 25;
 * igs/IGS.py:132-134 with up_sample True).  For x [N, Cin, H, W]:
 *     up[n, c, Y, X]  = the bilinear sample of x[n, c] at ((Y + 0.5) / 2 - 0.5, (X + 0.5) / 2 - 0.5), the source clamped at 0 and the
 *                       neighbour index at H - 1 / W - 1 (F.interpolate(scale_factor=2, mode='bilinear', align_corners=False)) for
 *                       0 <= Y < 2 H, 0 <= X < 2 W, and ZERO outside: the convolution pads at the upsampled resolution
 *     out[n, o, Y, X] = bias[o] + sum_{c, dy, dx} weight[o, c, dy, dx] up[n, c, Y + dy - 1, X + dx - 1]          out [N, Cout, 2 H, 2 W]
 * up is never stored.  Forward only.  Runs on `stream`, reads nothing back, allocates nothing, uses no atomics; every output element is
 * written by one lane: two runs agree bit for bit, and an image's result does not depend on N or on its place in the batch.
 *   - x in x_dtype (IGS_DTYPE_F32 / IGS_DTYPE_F16, widened on load), every H x W plane contiguous (xs_w == 1, xs_h == W); xs_n and xs_c,
 *     in elements, are free (>= 0), so slices of n and c of a larger buffer are read in place.  Channels-last is refused.
 *   - conv_dtype selects the instance, independently of x_dtype, and is the dtype of wpack and of out (NCHW contiguous).
 *     IGS_DTYPE_F32: the interpolation in float32 (two fma per axis), then v_mfma_f32_32x32x2_f32: one float32 fma chain per output that
 *     starts from the bias and runs over the 9 Cin products in a fixed order (input tile, tap, channel).  IGS_DTYPE_F16: the float32
 *     upsampled value is rounded once to half, the weights are half, v_mfma_f32_32x32x16_f16 accumulates in float32 from the float32 bias,
 *     and the result is rounded once to half.
 *   - wpack: 9 Linears [Cout, Cin], tap dy * 3 + dx = weight[:, :, dy, dx], each in igs_mlp_heads_fwd's tile order (see
 *     igs_condition3d_fwd), one after another: tile ((tap * ot) + o) * kt + k.  igs_upconv_pack_elems(Cin, Cout, conv_dtype) =
 *     9 ot kt 1024 with ot = ceil(Cout / 32), kt = ceil(Cin / 32) is the element count (-1: a width outside 1 .. IGS_UPCONV_MAX_WIDTH or
 *     an unknown dtype code).  bpack: float32 [128], the bias zero-padded.
 *   - Refused with IGS_RAST_E_INVALID and a message before any HIP call: Cin or Cout outside 1 .. IGS_UPCONV_MAX_WIDTH; H or W outside
 *     1 .. IGS_UPCONV_MAX_HW; N < 0 or N * H * W above IGS_UPCONV_MAX_PIXELS; an unknown dtype code; a stride pattern other than the one
 *     above; with N > 0 a NULL pointer, x or out not aligned to its element, wpack or bpack not aligned to 16 bytes.  N == 0 returns 0
 *     without a launch.
 * A workgroup owns an 8 x 32 output tile of one image and all output channels; the weights stream from L2. */
#define IGS_UPCONV_MAX_WIDTH 128
#define IGS_UPCONV_MAX_HW 4096
#define IGS_UPCONV_MAX_PIXELS (1 << 22)
long long igs_upconv_pack_elems(int Cin, int Cout, int conv_dtype);
int igs_upconv_fwd(void* stream, int N, int Cin, int Cout, int H, int W, int x_dtype, const void* x, long long xs_n, long long xs_c,
                   long long xs_h, long long xs_w, int conv_dtype, const void* wpack, const float* bpack, void* out);

/* The backward of igs_upconv_fwd (upconv_bwd.hip).  With g = dout = d out [N, Cout, 2 H, 2 W]:
 *     db[o]             = sum_{n, Y, X} g[n, o, Y, X]
 *     dw[o, c, dy, dx]  = sum_{n, Y, X} g[n, o, Y, X] up[n, c, Y + dy - 1, X + dx - 1]        up as igs_upconv_fwd defines it, zero outside
 *     dup[n, c, y, x]   = sum_{o, dy, dx} weight[o, c, dy, dx] g[n, o, y - dy + 1, x - dx + 1]  g zero outside the map
 *     dx                = U^T dup: low-resolution row i gathers the upsampled rows 2 i - 1 .. 2 i + 2 with 1/4, 3/4, 3/4, 1/4, columns
 *                         likewise, and what the forward's clamp folded onto the first / last row or column comes back to it
 * up is recomputed from x and dup lives in registers and LDS: neither reaches memory.  Runs on `stream`, reads nothing back, allocates
 * nothing, uses no atomics; every sum has a fixed order and every output element is written by one lane: two runs agree bit for bit, and
 * an image's dx does not depend on N or on its place in the batch.
 *   - x, xs_*, x_dtype as igs_upconv_fwd takes them; x is read only for dw and may be NULL when dw is NULL.  dout: contiguous, in
 *     conv_dtype.  dx [N, Cin, H, W] contiguous in x_dtype; dw float32 [Cout, Cin, 3, 3] row-major; db float32 [Cout].  Each of dx, dw, db
 *     may be NULL (not wanted): no work is launched for a NULL output, nothing at all with all three NULL.  Every element of a non-NULL
 *     output is written.  N == 0 zero-fills dw and db where given and launches nothing else.
 *   - wpack_t, in conv_dtype: igs_upconv_fwd's layout of the convolution weight_t[c, o, dy, dx] = weight[o, c, 2 - dy, 2 - dx], a
 *     [Cin, Cout, 3, 3] convolution: tile ((tap * kt) + k) * ot + o with kt = ceil(Cin / 32) now the output tiles;
 *     igs_upconv_pack_elems(Cout, Cin, conv_dtype) elements.
 *   - IGS_DTYPE_F32: v_mfma_f32_32x32x2_f32 in both product phases.  A dx element is one float32 fma chain over the 9 Cout products (output
 *     tile of Cout, tap, channel) per dup value and at most 8 more fma of the gather (4 per column pass, 4 for the rows; the weights and
 *     their products are exact).  dw and db are float32 sums over the N 4 H W pixels in a fixed order: a slice's pixels in order in one
 *     chain per lane half, the two halves added by the matrix instruction, then the slices in order.  IGS_DTYPE_F16:
 *     v_mfma_f32_32x32x16_f16; wpack_t and dout are half as given, the recomputed upsampled value is rounded to half once exactly as
 *     the forward rounds it, all sums are float32, dx is rounded once where x_dtype is half.
 *   - scratch: igs_upconv_bwd_scratch_bytes(N, Cin, Cout, H, W, conv_dtype) bytes (-1: sizes out of range or an unknown dtype code),
 *     16-byte aligned: the float32 partial dw and db of the slices the 4 x 32 pixel tiles of the batch are cut into, at most
 *     IGS_UPCONV_BWD_SLICES of them, so it does not grow with N beyond that: min(tiles, IGS_UPCONV_BWD_SLICES) *
 *     (9 ot kt 1024 + 128) * 4 with tiles = N ceil(2 H / 4) ceil(2 W / 32).  Needed (and checked) whatever is wanted.
 *   - Refused with IGS_RAST_E_INVALID and a message before any HIP call: everything igs_upconv_fwd refuses about sizes, dtype codes and
 *     strides; with N > 0 a NULL wpack_t, dout or scratch; a NULL x with a non-NULL dw; x, dx or dout not aligned to its element; dw or db
 *     not aligned to 4 bytes; wpack_t or scratch not aligned to 16 bytes; scratch_bytes below the needed size.
 * dgrad: a workgroup owns a 3 x 15 low-resolution tile of one image (8 x 32 dup pixels, the forward's product shape).  wgrad: a
 * workgroup owns 32 input channels and one slice of the pixel tiles; a second launch adds the slices in order. */
#define IGS_UPCONV_BWD_SLICES 64
long long igs_upconv_bwd_scratch_bytes(int N, int Cin, int Cout, int H, int W, int conv_dtype);
int igs_upconv_bwd(void* stream, int N, int Cin, int Cout, int H, int W, int x_dtype, const void* x, long long xs_n, long long xs_c,
                   long long xs_h, long long xs_w, int conv_dtype, const void* wpack_t, const void* dout, void* scratch,
                   long long scratch_bytes, void* dx, float* dw, float* db);

/* Fused attention for the anchor transformer (attn.hip): out = softmax(scale * Q K^T) V in one pass over the keys, the
 * self-attention of GridEncoder.conv's Transformer1D (igs/models/transformers.py:673-907: 8 heads of 64 channels over 8192 anchors, no mask,
 * no dropout).  The score matrix is never stored.  Everything runs on `stream`, reads nothing back and allocates nothing.
 *   - q [B, H, Aq, D], k and v [B, H, Ak, D], out [B, H, Aq, D] in `dtype` (IGS_DTYPE_F32 / IGS_DTYPE_F16), each given by its base pointer and
 *     the element strides of b, h and a; the stride of d is 1.  Head-major [B, H, A, D] tensors, the token-major [B, A, H * D] tensors that
 *     to_q / to_k / to_v produce (strides A * H * D, D, H * D) and slices of one fused QKV buffer are all read in place, and out can be
 *     written token-major.  Base pointers and the three strides (in bytes) must be multiples of 16.  Aq != Ak is allowed.
 *   - D must be 64; 1 <= Aq, Ak <= IGS_ATTN_MAX_TOKENS; 1 <= H <= IGS_ATTN_MAX_HEADS; 0 <= B <= IGS_ATTN_MAX_BATCH.  Anything else, an
 *     unknown dtype code, a negative or misaligned stride, an output whose rows alias (a stride below D on a dimension longer than 1), a
 *     scale that is not finite, a NULL required pointer or a misaligned pointer returns
 *     IGS_RAST_E_INVALID with a message before any HIP call; B == 0 returns 0 without a launch.
 *   - IGS_DTYPE_F16: v_mfma_f32_32x32x16_f16 with float32 accumulation; scores, running max, running sum and rescale are float32; P is rounded
 *     to half once, as the operand of the P V product; out is half.  IGS_DTYPE_F32: the exact v_mfma_f32_32x32x2_f32 (a float32 fma chain),
 *     no half value anywhere; out is float32.  exp is exp2 with scale * log2(e) folded into the scores.
 * igs_attn_fwd: lse [B, H, Aq] float32 contiguous receives log(sum_j exp(scale * q_i . k_j)) for the backward; NULL when none follows.
 * igs_attn_bwd: from q, k, v, out, lse and dout (= d out, laid out like out with its own strides) the gradients dq [B, H, Aq, D], dk and
 *   dv [B, H, Ak, D] in `dtype`, each with its own strides and each optional (NULL = not wanted); every element of a non-NULL output is
 *   written.  P is recomputed from lse.  No float atomics: d K / d V accumulate in the registers of the workgroup that owns the key tile, d Q
 *   in a second pass that owns the query tile, each in a fixed order, so two runs agree bit for bit.  `scratch`
 *   (igs_attn_bwd_scratch_bytes(...) bytes, at most 4 B H Aq + 512) holds rowsum(dout * out). */
#define IGS_ATTN_MAX_BATCH 65535
#define IGS_ATTN_MAX_HEADS 1024
#define IGS_ATTN_MAX_TOKENS (1 << 20)
size_t igs_attn_bwd_scratch_bytes(int B, int H, int Aq, int Ak, int D, int dtype);
int igs_attn_fwd(void* stream, int B, int H, int Aq, int Ak, int D, int dtype, const void* q, long long qs_b, long long qs_h, long long qs_a,
                 const void* k, long long ks_b, long long ks_h, long long ks_a, const void* v, long long vs_b, long long vs_h, long long vs_a,
                 float scale, void* out, long long os_b, long long os_h, long long os_a, float* lse);
int igs_attn_bwd(void* stream, int B, int H, int Aq, int Ak, int D, int dtype, const void* q, long long qs_b, long long qs_h, long long qs_a,
                 const void* k, long long ks_b, long long ks_h, long long ks_a, const void* v, long long vs_b, long long vs_h, long long vs_a,
                 const void* out, long long os_b, long long os_h, long long os_a, const float* lse, const void* dout, long long gs_b,
                 long long gs_h, long long gs_a, float scale, void* dq, long long dqs_b, long long dqs_h, long long dqs_a, void* dk,
                 long long dks_b, long long dks_h, long long dks_a, void* dv, long long dvs_b, long long dvs_h, long long dvs_a, void* scratch);

/* Swin window attention for the motion-feature transformers (wattn.hip): out = softmax(scale * Q K^T + mask) V
 * inside every one of the K x K windows of an h x w feature map, one head of D = 128 channels: single_head_split_window_attention
 * (igs/models/unimatch/attention.py:45-104) with the mask of generate_shift_window_attn_mask (igs/models/unimatch/utils.py:84-108), and
 * with K = 1 single_head_full_attention (attention.py:8-16).  The rolls, the window split, the merge and the score matrix are never
 * stored.  Everything runs on `stream`, reads nothing back and allocates nothing.
 *   - q, k, v, out, dout and the gradients are [B, h * w, D] in `dtype` (IGS_DTYPE_F32 / IGS_DTYPE_F16) in the ORIGINAL token order
 *     (token y * w + x), each given by its base pointer and the element strides of b and of the token; the stride of d is 1, so
 *     slices of one fused [B, h * w, 3 D] buffer are read in place.  Base pointers and strides (in bytes) must be multiples of 16.
 *   - Token j of window (wy, wx) is the original token ((y' + sh) mod h) * w + (x' + sw) mod w with y' = wy * wh + j / ww,
 *     x' = wx * ww + j mod ww, wh = h / K, ww = w / K and (sh, sw) = (wh / 2, ww / 2) when `shift` != 0, else (0, 0).
 *   - The region of a rolled position is 3 rh + rw, rh = (y' >= h - wh) + (y' >= h - sh), rw likewise in x.  When shifted, a pair of
 *     tokens of different regions gets -100 added to its scaled score: a finite addend, as in the reference, not -inf.
 *   - D must be 128; 0 <= B <= IGS_WINDOW_ATTN_MAX_BATCH; 1 <= h, w; B * h * w <= 2^24; 1 <= K with h % K == 0 and w % K == 0; a
 *     shifted call needs wh >= 2 and ww >= 2 (the reference's mask degenerates below).  Anything else, an unknown dtype code, a negative
 *     or misaligned stride, an output whose rows alias (a stride below D on a dimension longer than 1), a scale that is not finite, a
 *     NULL required pointer or a misaligned pointer returns IGS_RAST_E_INVALID with a message before any HIP call; B == 0 returns 0.
 *   - Arithmetic as in igs_attn_*: IGS_DTYPE_F16 runs v_mfma_f32_32x32x16_f16 with float32 scores, softmax and accumulation and P rounded
 *     to half once; IGS_DTYPE_F32 runs the exact v_mfma_f32_32x32x2_f32 with no half value anywhere.
 * igs_window_attn_fwd: lse [B, h * w] float32 contiguous, in original token order, receives the log-sum-exp of every token's masked
 *   scores for the backward; NULL when none follows.
 * igs_window_attn_bwd: the gradients dq, dk, dv, each with its own strides and each optional (NULL = not wanted; none wanted returns 0);
 *   every element of a non-NULL output is written.  P is recomputed from lse.  No float atomics: two runs agree bit for bit.  `scratch`
 *   (igs_window_attn_bwd_scratch_bytes(...) bytes, at most 4 B h w + 4 h w + 512) holds rowsum(dout * out). */
#define IGS_WINDOW_ATTN_MAX_BATCH 65535
size_t igs_window_attn_bwd_scratch_bytes(int B, int h, int w, int K, int D, int dtype);
int igs_window_attn_fwd(void* stream, int B, int h, int w, int K, int shift, int D, int dtype, const void* q, long long qs_b, long long qs_t,
                        const void* k, long long ks_b, long long ks_t, const void* v, long long vs_b, long long vs_t, float scale, void* out,
                        long long os_b, long long os_t, float* lse);
int igs_window_attn_bwd(void* stream, int B, int h, int w, int K, int shift, int D, int dtype, const void* q, long long qs_b, long long qs_t,
                        const void* k, long long ks_b, long long ks_t, const void* v, long long vs_b, long long vs_t, const void* out,
                        long long os_b, long long os_t, const float* lse, const void* dout, long long gs_b, long long gs_t, float scale,
                        void* dq, long long dqs_b, long long dqs_t, void* dk, long long dks_b, long long dks_t, void* dv, long long dvs_b,
                        long long dvs_t, void* scratch);

/* The unimatch CNN encoder's instance norms and position add (inorm.hip).  Forward only: the backbone is frozen in
 * IGS (igs/IGS.py:76-77) and its inputs are images, so no backward exists.  Everything runs on `stream`, reads nothing back and allocates
 * nothing.  Every refusal below returns IGS_RAST_E_INVALID with a message before any HIP call.
 * igs_instance_norm_fwd: nn.InstanceNorm2d with affine = False and no running statistics (igs/models/unimatch/backbone.py:17-20,51) fused
 *   with what follows it.  x, skip, out: `planes` = N * C contiguous runs of `hw` = H * W elements of an NCHW tensor, all in `dtype`
 *   (IGS_DTYPE_F32 / IGS_DTYPE_F16); arithmetic is float32.  IN(t) = (t - mean) / sqrt(var + eps) per plane with the biased variance
 *   taken from centred values.  `mode`:
 *     IGS_INORM_PLAIN              IN(x)                           a bare norm
 *     IGS_INORM_RELU               relu(IN(x))                     the stem and norm1 of every block (backbone.py:30,105-107)
 *     IGS_INORM_RELU_ADD_RELU      relu(skip + relu(IN(x)))        the tail of a block with an identity skip (backbone.py:31,36)
 *     IGS_INORM_RELU_ADDNORM_RELU  relu(IN(skip) + relu(IN(x)))    the tail of a block with a downsample branch (backbone.py:25-26,31-36)
 *   - out == x is allowed and gives bitwise what a separate out gives (the reference's ReLU is in place); any other overlap of out with
 *     x or skip is refused.  relu is torch.relu: a NaN stays a NaN.  A plane that holds a NaN or an infinity comes out all NaN, as in
 *     PyTorch; the other planes are untouched by it.  No atomics; two runs agree bit for bit.
 *   - Refused: hw < 2 (PyTorch: "Expected more than 1 spatial element"), hw > IGS_INORM_MAX_HW, planes < 0 or > IGS_INORM_MAX_PLANES, a
 *     NULL x or out, a NULL skip in the two modes that read it (ignored in the others), a pointer not aligned to its element size, an
 *     unknown mode or dtype code, an eps that is negative or not finite.  planes == 0 returns 0 without a launch.
 *   - Planes of at most igs_instance_norm_resident_max(dtype, mode) elements are read once (the workgroup holds its plane in registers);
 *     larger ones are read twice by the same workgroup.  Plane bases need no alignment beyond the element size.
 * igs_instance_norm_resident_max: that limit (two planes are live in IGS_INORM_RELU_ADDNORM_RELU, so it is lower there); 0 for an
 *   unknown dtype or mode.
 * igs_position_add: feature_add_position (igs/models/unimatch/utils.py:111-131) for both features in one launch, no split, position or
 *   merge tensor: f0, f1, out0, out1 [B, C, H, W] contiguous in `dtype`; with n = C / 2, wh = H / splits, ww = W / splits channel c < n adds
 *   s(c, (y mod wh) + 1, wh) and channel c >= n adds s(c - n, (x mod ww) + 1, ww), s(i, p, L) = f(p / (L + 1e-6) * 2 pi /
 *   10000^(2 floor(i / 2) / n)) with f = sin for even i and cos for odd i (igs/models/unimatch/position.py:29-46), in float32.
 *   out0 == f0 and out1 == f1 are allowed; any other overlap with an output is refused, as are C % 4 != 0, H or W not divisible by
 *   splits, splits < 1, sizes out of range, an unknown dtype code and a NULL pointer.  B == 0 returns 0 without a launch. */
#define IGS_INORM_PLAIN 0
#define IGS_INORM_RELU 1
#define IGS_INORM_RELU_ADD_RELU 2
#define IGS_INORM_RELU_ADDNORM_RELU 3
#define IGS_INORM_MAX_HW (1LL << 30)
#define IGS_INORM_MAX_PLANES 2147483647LL
int igs_instance_norm_fwd(void* stream, const void* x, const void* skip, void* out, long long planes, long long hw, int dtype, int mode,
                          float eps);
long long igs_instance_norm_resident_max(int dtype, int mode);
int igs_position_add(void* stream, const void* f0, const void* f1, void* out0, void* out1, int B, int C, int H, int W, int splits, int dtype);

/* The per-token work of the two transformers up to their GEMMs (tokens.hip): the LayerNorms of BasicTransformerBlock
 * (igs/models/transformers.py:304-365) and of the unimatch TransformerLayer with the add behind them (igs/models/unimatch/transformer.py:
 * 140-146), and the GEGLU of the block's feed-forward (transformers.py:503-506).  Everything runs on `stream`, reads nothing back and
 * allocates nothing; arithmetic is float32, half operands are widened on load and rounded once on store; no float atomics, two runs
 * agree bit for bit.  Every refusal below returns IGS_RAST_E_INVALID with a message before any HIP call.  Rows are given by a base pointer
 * and a row stride in elements (the stride inside a row is 1), so slices of a wider buffer are read and written in place.  "Overlap"
 * means the byte ranges from an operand's first to its last element.
 * igs_layer_norm_fwd: out[n, :] = (res[n, :] +) LN(x[n, :]) * weight + bias over x [N, C], LN(t) = (t - mean) / sqrt(var + eps) per row
 *   with the biased variance taken from centred values.  x, res and out each have their own dtype code (IGS_DTYPE_F32 / IGS_DTYPE_F16) and
 *   row stride; res is optional (NULL; its dtype code and stride are then ignored); weight and bias are [C] float32, both given or both
 *   NULL (no affine step).  A row is read once and stays in registers between the statistics and the write.  A constant row gives exactly
 *   bias (+ res); a row that holds a NaN or an infinity comes out all NaN, as in PyTorch; the other rows are untouched by it.
 *   - out == res with one dtype and one row stride is allowed (the in-place residual update) and gives the bits of a separate out; every
 *     other overlap of out with x, res, weight or bias is refused.
 *   - Refused: C < 1 or > IGS_LN_MAX_C, N < 0 or > IGS_LN_MAX_ROWS, a row stride below C or above IGS_TOKENS_MAX_STRIDE, an unknown dtype
 *     code, an eps that is negative or not finite, weight without bias or bias without weight, a NULL x or out, a pointer not aligned to
 *     its element size.  N == 0 returns 0 without a launch.  Four-element loads are used when C, every row stride and every base pointer
 *     (16 bytes for float32, 8 for float16) allow them, scalar loads otherwise: nothing else depends on alignment.
 * igs_layer_norm_bwd: from x, weight (NULL = ones) and dout = d out [N, C] the gradients dx [N, C] (own dtype and stride), dweight and
 *   dbias [C] float32; each is optional (NULL = not wanted; none wanted returns 0) and every element of a non-NULL output is written.
 *   The statistics are recomputed from x: the forward saves nothing.  d res is dout itself.  dweight and dbias need `scratch`
 *   (igs_layer_norm_bwd_scratch_bytes(N, C) bytes; 0 for sizes out of range): one partial row per workgroup, added in workgroup order by a
 *   second launch.  Refusals as above, plus a NULL dout, a NULL scratch when dweight or dbias is wanted, and any overlap of an output or
 *   the scratch with an input or with one another.
 * igs_geglu_fwd: out[n, d] = p[n, d] * gelu(p[n, D + d]) over p [N, 2 D] with a row stride, out [N, D] contiguous, one dtype for both;
 *   gelu(g) = 0.5 g (1 + erf(g / sqrt 2)), the exact form.
 * igs_geglu_bwd: from p and dout [N, D] contiguous, dp [N, 2 D] contiguous in one launch, both halves written:
 *   dp[n, d] = dout gelu(g), dp[n, D + d] = dout h (Phi(g) + g phi(g)) with h = p[n, d], g = p[n, D + d].
 *   Refused by both: D < 1 or > IGS_GEGLU_MAX_D, N < 0 or N * D > IGS_GEGLU_MAX_ELEMS, a row stride below 2 D or above
 *   IGS_TOKENS_MAX_STRIDE, an unknown dtype code, a NULL or misaligned pointer, an output that overlaps an input.  N == 0 returns 0. */
#define IGS_LN_MAX_C 1024
#define IGS_LN_MAX_ROWS (1LL << 24)
#define IGS_TOKENS_MAX_STRIDE (1LL << 31)
#define IGS_GEGLU_MAX_D 8192
#define IGS_GEGLU_MAX_ELEMS (1LL << 30)
int igs_layer_norm_fwd(void* stream, long long N, int C, int x_dtype, const void* x, long long xs, int res_dtype, const void* res,
                       long long rs, const float* weight, const float* bias, float eps, int out_dtype, void* out, long long os);
size_t igs_layer_norm_bwd_scratch_bytes(long long N, int C);
int igs_layer_norm_bwd(void* stream, long long N, int C, int x_dtype, const void* x, long long xs, const float* weight, float eps,
                       int dout_dtype, const void* dout, long long gs, int dx_dtype, void* dx, long long dxs, float* dweight, float* dbias,
                       void* scratch);
int igs_geglu_fwd(void* stream, long long N, int D, int dtype, const void* p, long long ps, void* out);
int igs_geglu_bwd(void* stream, long long N, int D, int dtype, const void* p, long long ps, const void* dout, void* dp);

/* The two ends of Transformer1D.forward around its blocks (gnorm.hip; igs/models/transformers.py:860-908): the
 * GroupNorm whose result goes token-major to proj_in, and proj_out's result plus the residual.  Everything runs on `stream`, reads nothing
 * back and allocates nothing; arithmetic is float32, half operands are widened on load and rounded once on store; no float atomics, every
 * split of a sum depends on the shapes only, two runs agree bit for bit.  Every refusal below returns IGS_RAST_E_INVALID with a message
 * before any HIP call.
 *   - Channel-major operands (x, res, dx) are [B, C, A] with stride 1 on A and their own batch and channel strides in elements, so a
 *     slice of a wider buffer is read or written in place.  Token-major operands (out, tok, dout) are rows [B * A, C] with stride 1 on C
 *     and a row stride in elements; example b owns the rows b A .. b A + A - 1.  Each operand has its own dtype code (IGS_DTYPE_F32 /
 *     IGS_DTYPE_F16).  weight, bias, dweight, dbias are [C] float32; stats is [B, G, 2] float32 = (mean, 1 / sqrt(var + eps)) per group.
 * igs_group_norm_tokens_fwd: out[b, a, c] = (x[b, c, a] - mean[b, g]) rstd[b, g] weight[c] + bias[c], g = c / (C / G), with the biased
 *   variance of the (C / G) A elements of a group taken from centred values; writes out and stats (two launches: the statistics, then
 *   the tile transpose).  weight and bias both given or both NULL (no affine step).  A constant group gives exactly bias; a group that
 *   holds a NaN or an infinity comes out all NaN, as in PyTorch, and no other group is touched by it.
 * igs_group_norm_tokens_bwd: from x, weight (NULL = ones), the forward's stats and dout = d out the gradients dx (channel-major, own
 *   dtype and strides), dweight and dbias; each is optional (NULL = not wanted; none wanted returns 0) and every element of a non-NULL
 *   output is written.  `scratch` (igs_group_norm_tokens_bwd_scratch_bytes(B, C, G, A) bytes; 0 for sizes out of range) is always needed:
 *   per tile of 64 tokens one row of the sums over its tokens of dout x_hat and dout, added in tile order per example, then over the
 *   channels of a group (dx) and over the examples (dweight, dbias).
 * igs_tokens_add_residual: out[b, a, c] = tok[b, a, c] + res[b, c, a] in float32, rounded once; one launch.
 *   - Refused: C < 1 or > IGS_GN_MAX_C, G < 1 or not a divisor of C, A < 1 or (C / G) A > IGS_GN_MAX_GROUP_ELEMS (igs_tokens_add_residual:
 *     G = 1), B < 0 or B A > IGS_GN_MAX_TOKENS; a channel stride below A, a batch stride below (C - 1) channel stride + A, a row stride
 *     below C, a row or channel stride above IGS_TOKENS_MAX_STRIDE, a batch stride above IGS_GN_MAX_BATCH_STRIDE; an unknown dtype code;
 *     an eps that is negative or not finite; weight without bias or bias without weight; a NULL x, out, stats, dout, tok, res or scratch;
 *     a pointer not aligned to its element size; any overlap of an output or the scratch with an input or with one another.  B == 0
 *     returns 0 without a launch.  Four-element access is used where C, A, the strides and the base pointers (16 bytes for float32, 8 for
 *     float16) allow it, scalar access of the same lane mapping otherwise: nothing else depends on alignment. */
#define IGS_GN_MAX_C 1024
#define IGS_GN_MAX_TOKENS (1LL << 24)
#define IGS_GN_MAX_GROUP_ELEMS (1LL << 30)
#define IGS_GN_MAX_BATCH_STRIDE (1LL << 36)
int igs_group_norm_tokens_fwd(void* stream, int B, int C, int G, long long A, int x_dtype, const void* x, long long x_bs, long long x_cs,
                              const float* weight, const float* bias, float eps, int out_dtype, void* out, long long os, float* stats);
size_t igs_group_norm_tokens_bwd_scratch_bytes(int B, int C, int G, long long A);
int igs_group_norm_tokens_bwd(void* stream, int B, int C, int G, long long A, int x_dtype, const void* x, long long x_bs, long long x_cs,
                              const float* weight, const float* stats, int dout_dtype, const void* dout, long long gs, int dx_dtype, void* dx,
                              long long dx_bs, long long dx_cs, float* dweight, float* dbias, void* scratch);
int igs_tokens_add_residual(void* stream, int B, int C, long long A, int tok_dtype, const void* tok, long long ts, int res_dtype,
                            const void* res, long long r_bs, long long r_cs, int out_dtype, void* out, long long os);

/* The residual decoder of AGM-Net in one launch (mlp.hip): GS3DRenderer.decode_residual_feature (igs/models/gs.py:
 * 858-869), i.e. the MLP of igs/models/networks.py:60-108 and the per-feature output Linears behind it, per row n of x [N, widths[0]]:
 *     h0 = x[n];  h_{l+1} = act_l(W_l h_l + b_l) for l = 0 .. n_hidden - 1;  y = W_heads h + b_heads, no activation,
 * where W_heads, b_heads are the heads' weights and biases one after another, and head k's share of y is written to outs[k], a contiguous
 * [N, head_widths[k]] tensor.  Forward only.  Runs on `stream`, reads nothing back, allocates nothing, uses no atomics: two runs agree
 * bit for bit and a row's result does not depend on the other rows.  Each row of x is read once; no intermediate reaches memory.
 *   - widths[0 .. n_hidden]: the input width and the output width of each hidden Linear; act_after[l] != 0: the activation `act`
 *     (IGS_MLP_ACT_SILU = v / (1 + exp(-v)), IGS_MLP_ACT_RELU) follows hidden Linear l (the reference's MLP has none behind its last one).
 *     SiLU is finite for every finite v (below v = -87.3, where exp(-v) leaves float32, the result is below |v| 2^-126 in size); both
 *     activations keep a NaN, which therefore stays in its own row.
 *   - x is in `dtype` (IGS_DTYPE_F32 / IGS_DTYPE_F16) with stride 1 inside a row and x_rs elements between rows, so a slice of a wider
 *     buffer is read in place; the outputs are in `dtype` too.  IGS_DTYPE_F16: v_mfma_f32_32x32x16_f16, float32 accumulators that start
 *     from the bias, activation in float32, one rounding to half when an activation becomes the next operand and one on store.
 *     IGS_DTYPE_F32: v_mfma_f32_32x32x2_f32, an exact float32 fma chain, no half value anywhere.
 *   - wpack: the weights in `dtype`, in the order the kernel's operands want them.  Linear l (the heads' last), W [O, I] row-major as
 *     nn.Linear keeps it, becomes ceil(O / 32) x ceil(I / 32) tiles of 1024 elements, output tile outermost; tile (ot, kt) is
 *     [chunk][lane 64][E] with E = 8 (half, 2 chunks) or 4 (float, 4 chunks), and element e = chunk E + j of lane (r = lane & 31,
 *     h = lane >> 5) is W[32 ot + r][32 kt + (e & 3) + 8 (e >> 2) + 4 h], zero outside W.  igs_mlp_heads_pack_elems gives the element
 *     count (-1 for sizes out of range).  bpack: float32 [n_hidden + 1][128], the biases zero-padded (an absent bias: zeros).
 *   - Refused with IGS_RAST_E_INVALID and a message before any HIP call: an unknown dtype or activation code; N < 0 or > IGS_MLP_MAX_ROWS;
 *     n_hidden outside 0 .. IGS_MLP_MAX_HIDDEN; n_heads outside 1 .. IGS_MLP_MAX_HEADS; a width or head width outside
 *     1 .. IGS_MLP_MAX_WIDTH, or head widths that add up to more; NULL widths, head_widths or (n_hidden > 0) act_after; a row stride
 *     below widths[0] or above IGS_TOKENS_MAX_STRIDE; with N > 0 a NULL x, wpack, bpack, outs or outs[k], a pointer not aligned to its
 *     element size, a wpack not aligned to 16 bytes.  N == 0 returns 0 without a launch.  Four-element loads of x are used when
 *     widths[0], x_rs and the base pointer allow them, scalar loads otherwise. */
#define IGS_MLP_MAX_WIDTH 128
#define IGS_MLP_MAX_HIDDEN 3
#define IGS_MLP_MAX_HEADS 8
#define IGS_MLP_MAX_ROWS (1LL << 32)
#define IGS_MLP_ACT_SILU 0
#define IGS_MLP_ACT_RELU 1
long long igs_mlp_heads_pack_elems(int n_hidden, const int* widths, int n_heads, const int* head_widths);
int igs_mlp_heads_fwd(void* stream, long long N, int dtype, int act, int n_hidden, const int* widths, const int* act_after, int n_heads,
                      const int* head_widths, const void* x, long long x_rs, const void* wpack, const float* bpack, void* const* outs);

/* The residual decoder's backward (mlp.hip).  The forward is recomputed from x: between igs_mlp_heads_fwd, which is
 * also the training forward, and this call nothing of N rows has to be kept but x.  From the heads' upstream gradients
 *     dh_L = Wh^T dY,  dWh = dY^T h_L,  dbh = sum_rows dY;   for l = L-1 .. 0:  dz_l = dh_{l+1} act'(z_l) (dh_{l+1} where act_after[l] == 0),
 *     dW_l = dz_l^T h_l,  db_l = sum_rows dz_l,  dh_l = W_l^T dz_l;   dx = dh_0.
 * ReLU' is 0 at z <= 0 and keeps a NaN; SiLU' = s (1 + z (1 - s)), s = sigmoid(z), on the forward's clamped exponent: finite for every
 * finite z.  Runs on `stream`, reads nothing back, allocates nothing, uses no float atomics: every sum has a fixed order (the rows of a
 * slice of 256, chunk after chunk, then the slices), two runs agree bit for bit, and a row's dx does not depend on the other rows.
 *   - sizes, dtype, act, act_after, x, x_rs, wpack, bpack as igs_mlp_heads_fwd takes them.  wpack_t: every Linear's TRANSPOSE packed the
 *     same way (W^T [I, O] in place of W [O, I]; the same element count per Linear, so the same offsets).  The products use the forward's
 *     matrix instructions (float16: float32 accumulation, operands rounded to half once; float32: exact fma chains).
 *   - douts[k]: d outs[k], [N, head_widths[k]] contiguous in `dtype`, or NULL for zeros.  dx: [N, widths[0]] contiguous in `dtype`, or NULL
 *     if not wanted.  dw: float32 whatever the dtype, every Linear's [O, I] row-major as nn.Linear keeps it, layer after layer, then the
 *     heads concatenated along the output; db: float32, every Linear's outputs concatenated in the same order; each NULL if not wanted.
 *     Every element of a non-NULL output is written.  With all three NULL nothing is launched.
 *   - scratch: igs_mlp_heads_bwd_scratch_bytes(N, ...) bytes (-1 for sizes out of range), 16-byte aligned, not initialised by the caller.
 *     It holds the pre-activations and their gradients of one chunk of 16384 rows as float32 and the slices' partial sums, so it does
 *     not grow with N above 16384.  The launches: two per chunk (rows, weight gradients) and one reduction.
 *   - Refused with IGS_RAST_E_INVALID and a message before any HIP call: what igs_mlp_heads_fwd refuses about codes, sizes, N, act_after
 *     and the row stride; a dw or db not aligned to 4 bytes; with N > 0 a NULL x, wpack, wpack_t, bpack, douts or scratch, an x, douts[k]
 *     or dx not aligned to its element size, a wpack, wpack_t or scratch not aligned to 16 bytes, a scratch_bytes below the needed size.
 *     N == 0 zero-fills dw and db where given and launches nothing else. */
long long igs_mlp_heads_bwd_scratch_bytes(long long N, int dtype, int n_hidden, const int* widths, int n_heads, const int* head_widths);
int igs_mlp_heads_bwd(void* stream, long long N, int dtype, int act, int n_hidden, const int* widths, const int* act_after, int n_heads,
                      const int* head_widths, const void* x, long long x_rs, const void* wpack, const void* wpack_t, const float* bpack,
                      const void* const* douts, void* scratch, long long scratch_bytes, void* dx, float* dw, float* db);

/* The tail of a unimatch TransformerLayer in one launch (ffn.hip): everything behind the attention
 * (igs/models/unimatch/transformer.py:34-40, 117-146).  Per row t of a (the attention's output) and s (the layer's source), 128 channels:
 *     m = Wm a;  n1 = LN1(m);  has_ffn == 0: out = s + n1;  has_ffn != 0: h = gelu(W1 [s ; n1]),  y = W2 h,  out = s + LN2(y),
 * with Wm [128, 128], W1 [hidden, 256] (columns 0..127 multiply s, 128..255 multiply n1), W2 [128, hidden], no biases, gelu the exact
 * (erf) one and LN(v) = (v - mean) / sqrt(var + eps) * weight + bias with float32 statistics and the biased variance taken from centred
 * values.  Forward only.  Runs on `stream`, reads nothing back, allocates nothing, uses no atomics: two runs agree bit for bit, and a
 * row's result depends on that row and the weights only (not on T, on the row's position or on the other rows), so a NaN stays in its row.
 *   - a, s and out each have their own dtype code (IGS_DTYPE_F32 / IGS_DTYPE_F16; widened on load, rounded once on store) and their own row
 *     stride in elements (>= 128; stride 1 inside a row), so slices of wider buffers are read and written in place.  Four-element accesses
 *     are used for an operand whose base lies on its dtype's four-element grid and whose stride is a multiple of 4, scalar ones otherwise.
 *   - compute_dtype is the matrix operand type.  IGS_DTYPE_F32: v_mfma_f32_32x32x2_f32, an exact float32 fma chain, no half value anywhere.
 *     IGS_DTYPE_F16: v_mfma_f32_32x32x16_f16 with float32 accumulation; the only roundings to half are those of the three operands a,
 *     [s ; n1] and h (after the float32 GELU).  The LayerNorms, the GELU and the residual add are float32 in both; the residual reads s
 *     itself, not the rounded operand.
 *   - wpack, in compute_dtype, 16-byte aligned, igs_layer_tail_pack_elems(hidden, has_ffn) elements (-1 for a hidden out of range;
 *     hidden is ignored without FFN), in tiles of 1024 elements in igs_mlp_heads_fwd's per-tile layout (tile (ot, kt) of W is [chunk][lane 64][E]
 *     with E = 8 (half) or 4 (float), element e = chunk E + j of lane (r, h) = W[32 ot + r][32 kt + (e & 3) + 8 (e >> 2) + 4 h]):
 *       Wm:  16 tiles, output tile outermost: tile 4 ot + kt;
 *       W1:  hidden / 32 x 8 tiles, output tile outermost: tile 8 j + kt (has_ffn only);
 *       W2:  hidden / 32 x 4 tiles, INPUT tile outermost: tile 4 j + ot, so that the 12 tiles of hidden units 32 j .. 32 j + 31 are two
 *            contiguous pieces (has_ffn only).
 *   - ln1_w, ln1_b, ln2_w, ln2_b: float32 [128]; ln2_* and eps2 are not read without FFN.
 *   - The launch: workgroups of 4 waves take trips of IGS_LAYER_TAIL_TRIP_ROWS rows (32 per wave); the grid is
 *     min(ceil(T / IGS_LAYER_TAIL_TRIP_ROWS), compute units x (has_ffn ? 1 : 2)) workgroups, each looping over its trips.
 *   - Refused with IGS_RAST_E_INVALID and a message before any HIP call: an unknown dtype code; T < 0 or > IGS_LAYER_TAIL_MAX_ROWS; with FFN a
 *     hidden that is not a multiple of 32 in 32 .. IGS_LAYER_TAIL_MAX_HIDDEN; a row stride below 128 or above IGS_TOKENS_MAX_STRIDE; an eps
 *     that is not finite and >= 0; with T > 0 a NULL required pointer, a pointer not aligned to its element size, a wpack not aligned to
 *     16 bytes, an out that overlaps a or s.  T == 0 returns 0 without a launch. */
#define IGS_LAYER_TAIL_MAX_HIDDEN 2048
#define IGS_LAYER_TAIL_MAX_ROWS (1LL << 24)
#define IGS_LAYER_TAIL_TRIP_ROWS 128
long long igs_layer_tail_pack_elems(int hidden, int has_ffn);
int igs_layer_tail_fwd(void* stream, long long T, int compute_dtype, int has_ffn, int hidden, const void* a, int a_dtype, long long a_stride,
                       const void* s, int s_dtype, long long s_stride, const void* wpack, const float* ln1_w, const float* ln1_b, float eps1,
                       const float* ln2_w, const float* ln2_b, float eps2, void* out, int out_dtype, long long out_stride);

/* The backward of igs_layer_tail_fwd (ffn_bwd.hip; DESIGN.md section 27, "The backward"): the forward is recomputed from a and s, nothing of
 * T rows is kept between the two but the inputs.  Per row, with g = d out, xh = (v - mean) rstd of each LayerNorm and Phi, phi the normal
 * distribution and density:
 *     FFN:     d ln2_w = sum_t g xh2;  d ln2_b = sum_t g;  q = g ln2_w;  dy = r2 (q - mean q - xh2 mean(q xh2));  d W2 = sum_t dy h^T;
 *              dh = W2^T dy;  dz = dh (Phi(z) + z phi(z));  d W1 = sum_t dz [s ; n1]^T;  du = W1^T dz;  ds = g + du[0:128];  dn1 = du[128:256]
 *     no FFN:  ds = g;  dn1 = g
 *     both:    d ln1_w = sum_t dn1 xh1;  d ln1_b = sum_t dn1;  p = dn1 ln1_w;  dm = r1 (p - mean p - xh1 mean(p xh1));
 *              d Wm = sum_t dm a^T;  da = Wm^T dm
 * Runs on `stream`, reads nothing back, allocates nothing.  No float atomics in memory or LDS; every sum has a fixed order (the rows of a
 * slice of 512, chunk after chunk, then the slices), two runs agree bit for bit on every output, and a row's da and ds depend on that row
 * of a, s, g and on the weights only (not on T, on the row's position or on the other rows): a NaN in a row makes that row's da / ds NaN,
 * leaves every other row's bits as they were, and makes the parameter gradients NaN.  GELU' is finite for every finite z.
 *   - T, compute_dtype, has_ffn, hidden, a, s, wpack, ln1_*, ln2_*, eps1, eps2 as igs_layer_tail_fwd takes them (s is not read, and may be
 *     NULL, without FFN).  g: d out, [T, 128] with its own dtype code and row stride.
 *   - wpack_t, in compute_dtype, 16-byte aligned, igs_layer_tail_pack_elems(hidden, has_ffn) elements: the TRANSPOSES in wpack's per-tile
 *     layout (element e = chunk E + j of lane (r, h) of tile (ot, kt) of a matrix M is M[32 ot + r][32 kt + (e & 3) + 8 (e >> 2) + 4 h]):
 *       Wm^T [128, 128]:      16 tiles, output tile outermost: tile 4 ot + kt;
 *       W1^T [256, hidden]:   hidden / 32 x 8 tiles, INPUT tile outermost: tile 8 j + ot (has_ffn only);
 *       W2^T [hidden, 128]:   hidden / 32 x 4 tiles, output tile outermost: tile 4 j + kt (has_ffn only),
 *     so that, as in wpack, the 12 tiles of hidden units 32 j .. 32 j + 31 are two contiguous pieces at the same offsets.
 *   - Every output may be NULL; every element of a non-NULL output is written; with all of them NULL nothing is launched.  da and ds:
 *     [T, 128], each with a dtype code and a row stride like the forward's out (rounded once on store); da's product is skipped when da is
 *     NULL.  d Wm [128, 128], d ln1_w, d ln1_b [128], d W1 [hidden, 256], d W2 [128, hidden], d ln2_w, d ln2_b [128]: float32 whatever the
 *     dtypes, row-major as nn.Linear and nn.LayerNorm keep them; the last four are not written without FFN.  When no parameter gradient
 *     is wanted, the stores that only the weight gradients read and the weight-gradient launches are skipped.
 *   - compute_dtype IGS_DTYPE_F32: v_mfma_f32_32x32x2_f32 everywhere, no half value anywhere.  IGS_DTYPE_F16: v_mfma_f32_32x32x16_f16 with
 *     float32 accumulation; a value is rounded to half once, only as a matrix operand: a, [s ; n1] and h as in the forward, dy, dz and dm
 *     for their two products each.  The LayerNorm backwards, GELU' and all parameter sums are float32; the residual part of ds reads g itself.
 *   - T is walked in chunks of IGS_LAYER_TAIL_BWD_CHUNK_ROWS rows.  scratch: igs_layer_tail_bwd_scratch_bytes(T, compute_dtype, has_ffn,
 *     hidden) bytes (-1 for sizes out of range), 16-byte aligned, not initialised by the caller: one chunk's spilled values as float32
 *     (per row 2 hidden + 1152 values with FFN, 512 without) and the slices' partial sums, so it does not grow with T above one chunk.
 *     The launches: per chunk one over the rows and, when a parameter gradient is wanted, one for the weight gradients; then one reduction.
 *   - Refused with IGS_RAST_E_INVALID and a message naming igs_layer_tail_bwd before any HIP call: everything igs_layer_tail_fwd refuses
 *     about codes, T, hidden, strides and eps (g, da and ds included); a parameter gradient not aligned to 4 bytes; with T > 0 a NULL a,
 *     g, wpack, wpack_t, ln1_w, ln1_b or scratch (with FFN also s, ln2_w, ln2_b), an a, s, g, da or ds not aligned to its element size, a
 *     wpack, wpack_t or scratch not aligned to 16 bytes, a scratch_bytes below the needed size, a da or ds that overlaps a, s or g.
 *     T == 0 zero-fills the parameter gradients that are given and launches nothing else. */
#ifndef IGS_LAYER_TAIL_BWD_CHUNK_ROWS              /* (a build may choose another multiple of 512: DESIGN.md section 27 has the table) */
#define IGS_LAYER_TAIL_BWD_CHUNK_ROWS 8192
#endif
long long igs_layer_tail_bwd_scratch_bytes(long long T, int compute_dtype, int has_ffn, int hidden);
int igs_layer_tail_bwd(void* stream, long long T, int compute_dtype, int has_ffn, int hidden, const void* a, int a_dtype, long long a_stride,
                       const void* s, int s_dtype, long long s_stride, const void* g, int g_dtype, long long g_stride, const void* wpack,
                       const void* wpack_t, const float* ln1_w, const float* ln1_b, float eps1, const float* ln2_w, const float* ln2_b,
                       float eps2, void* scratch, long long scratch_bytes, void* da, int da_dtype, long long da_stride, void* ds,
                       int ds_dtype, long long ds_stride, float* dWm, float* dln1_w, float* dln1_b, float* dW1, float* dW2, float* dln2_w,
                       float* dln2_b);

/* Up to IGS_TOKEN_PROJ_MAX_OUT bias-free 128 -> 128 projections of one activation in one launch (proj.hip): the
 * q_proj / k_proj / v_proj of the unimatch TransformerLayers (igs/models/unimatch/transformer.py:25-27, 104-106).  For j = 0 .. n - 1 and
 * every row t of x:
 *     out[(t + rot[j]) mod T][128 j .. 128 j + 127] = W_j x[t],   W_j [128, 128] as nn.Linear keeps it,
 * so the n results lie side by side in one buffer whose column slices igs_window_attn_fwd reads in place, and rot[j] = T / 2 is the
 * projection of x with its two batch halves swapped (a FeatureTransformer block's `concat1`, :274-289) without the swap being built.
 * Forward only.  Runs on `stream`, reads nothing back, allocates nothing, uses no atomics: two runs agree bit for bit, and a row's 128 n
 * results depend on that row and the weights only (not on T, on the row's position, on rot, or on which workgroup took it), so a NaN
 * stays in its row.
 *   - x: [T, 128] and out: [T, >= 128 n], each with its own dtype code (IGS_DTYPE_F32 / IGS_DTYPE_F16; widened on load, rounded once on
 *     store) and its own row stride in elements (x: >= 128, out: >= 128 n; stride 1 inside a row).  Columns of an out row beyond 128 n are
 *     not touched.  Four-element accesses are used for an operand whose base lies on its dtype's four-element grid and whose stride is a
 *     multiple of 4, scalar ones otherwise.
 *   - compute_dtype is the matrix operand type.  IGS_DTYPE_F32: v_mfma_f32_32x32x2_f32, an exact float32 fma chain over the 128 inputs in
 *     ascending order, no half value anywhere.  IGS_DTYPE_F16: v_mfma_f32_32x32x16_f16 with float32 accumulation; x is rounded to half
 *     once, as an operand.
 *   - wpack, in compute_dtype, 16-byte aligned, igs_token_proj_pack_elems(n) = n x 16 x 1024 elements (-1 for an n out of range): the n
 *     matrices one after the other, each as igs_layer_tail_fwd's Wm (16 tiles, output tile outermost: tile 4 ot + kt, in that
 *     function's per-tile layout).
 *   - rot: n host values, read before the call returns; NULL means all zero.
 *   - The launch: workgroups of 4 waves take trips of IGS_LAYER_TAIL_TRIP_ROWS rows (32 per wave); the grid is
 *     min(ceil(T / IGS_LAYER_TAIL_TRIP_ROWS), compute units x (compute_dtype == IGS_DTYPE_F16 ? 2 : 1)) workgroups, each looping over its
 *     trips.
 *   - Refused with IGS_RAST_E_INVALID and a message naming igs_token_proj_fwd before any HIP call: an unknown dtype code; n < 1 or
 *     > IGS_TOKEN_PROJ_MAX_OUT; T < 0 or > IGS_TOKEN_PROJ_MAX_ROWS; an x stride below 128, an out stride below 128 n, either above
 *     IGS_TOKENS_MAX_STRIDE; a rot[j] outside [0, T) (with T == 0: other than 0); with T > 0 a NULL x, wpack or out, an x or out not
 *     aligned to its element size, a wpack not aligned to 16 bytes, an out span that overlaps x.  T == 0 returns 0 without a launch. */
#define IGS_TOKEN_PROJ_MAX_OUT 5
#define IGS_TOKEN_PROJ_MAX_ROWS (1LL << 24)
long long igs_token_proj_pack_elems(int n);
int igs_token_proj_fwd(void* stream, long long T, int n, int compute_dtype, const void* x, int x_dtype, long long x_stride, const void* wpack,
                       const long long* rot, void* out, int out_dtype, long long out_stride);

/* The backward of igs_token_proj_fwd (proj_bwd.hip; DESIGN.md section 28, "The backward").  Per row t of x and output j, g_j[t] is the
 * upstream gradient of what the forward wrote for input row t, i.e. row (t + rot[j]) mod T of g[j]:
 *     d x[t] = sum_j W_j^T g_j[t]   (j ascending, one accumulator chain),      d W_j = sum_t g_j[t] (x) x[t]   (t ascending).
 * Runs on `stream`, reads nothing back, allocates nothing.  No float atomics: every sum has a fixed order (the rows of a slice, then the
 * slices), two runs agree bit for bit, and a row's d x depends on that row's gradients and the weights only (not on T, the row's
 * position, rot or x): a NaN in a row of a g[j] makes that row's d x and d W_j NaN, one in a row of x makes every wanted d W_j NaN, and
 * either leaves every other row's d x as it was.
 *   - T, n, compute_dtype, x, rot as igs_token_proj_fwd takes them.  g: n pointers to [T, 128] rows, all of g_dtype, each with its own row
 *     stride g_stride[j] >= 128 (column slices of the forward's buffer are read in place); g[j] == NULL means that output j had no
 *     gradient: it is skipped, and g_stride[j] is not read.  The array g itself may be NULL (no output had one).
 *   - wpack_t, in compute_dtype, 16-byte aligned, igs_token_proj_pack_elems(n) elements: the pack of the TRANSPOSES, matrix j being W_j^T in
 *     wpack's layout (16 tiles, output tile outermost).  Read only when dx is wanted.
 *   - dx: [T, 128] with its dtype code and row stride (rounded once on store), or NULL: then the d x kernel is not launched.  With every
 *     g[j] NULL it is written as zeros.  dW: n pointers to [128, 128] float32, row-major as nn.Linear keeps its weight, 16-byte aligned, or
 *     NULL where not wanted; the array itself may be NULL.  A dW[j] whose g[j] is NULL is written as zeros.
 *   - compute_dtype IGS_DTYPE_F32: v_mfma_f32_32x32x2_f32, operands widened on load, no half value anywhere.  IGS_DTYPE_F16:
 *     v_mfma_f32_32x32x16_f16 with float32 accumulation; x, g and W^T are rounded to half once, as operands; d W is never rounded to half.
 *   - The launches: for dx one launch by igs_token_proj_fwd's rule; for the weight gradients one launch in which a wave owns (slice of
 *     rows, output, input tile) and one reduction.  A slice is 512 rows, or, where that would give more than
 *     IGS_TOKEN_PROJ_BWD_MAX_SLICES slices, ceil(T / IGS_TOKEN_PROJ_BWD_MAX_SLICES) rows rounded up to a multiple of 128.  scratch:
 *     igs_token_proj_bwd_scratch_bytes(T, n) = min(ceil(T / 512), IGS_TOKEN_PROJ_BWD_MAX_SLICES) x n x 65536 bytes (-1 for a T or n out of
 *     range), 16-byte aligned, not initialised by the caller, read and written only when a dW[j] is wanted.
 *   - Refused with IGS_RAST_E_INVALID and a message naming igs_token_proj_bwd before any HIP call: an unknown dtype code; n, T out of range;
 *     a row stride (x, dx, a non-NULL g[j]'s) below 128 or above IGS_TOKENS_MAX_STRIDE; a rot[j] outside [0, T); a dW[j] not aligned to 16
 *     bytes; with T > 0 and something wanted: a NULL x or scratch while some dW[j] is wanted, a NULL wpack_t while dx is wanted, a NULL
 *     g_stride beside a non-NULL g[j], an x, g[j] or dx not aligned to its element size, a wpack_t or scratch not aligned to 16 bytes, a
 *     scratch_bytes below the needed size, and any output (dx, a dW[j], the scratch) that overlaps an input (x, a g[j], wpack_t) or
 *     another output.  T == 0 zero-fills the dW[j] that are given and writes no dx; with dx and every dW[j] NULL the call returns 0 and
 *     launches nothing. */
#define IGS_TOKEN_PROJ_BWD_MAX_SLICES 64
long long igs_token_proj_bwd_scratch_bytes(long long T, int n);
int igs_token_proj_bwd(void* stream, long long T, int n, int compute_dtype, const void* x, int x_dtype, long long x_stride,
                       const void* const* g, int g_dtype, const long long* g_stride, const long long* rot, const void* wpack_t,
                       void* scratch, long long scratch_bytes, void* dx, int dx_dtype, long long dx_stride, float* const* dW);

/* Densification support (igs/models/gaussian_model.py:586-663,865-868; driven by infer_batch.py:308-321).
 * igs_densify_stats: per-step statistics of add_densification_stats + the max_radii2D update, for Gaussians with radii > 0:
 *   grad_accum += ||dL_dmean2D[:2]||, denom += 1, max_radii = max(max_radii, radii).
 * igs_densify_remap: rebuilds the flat optimiser state (param / exp_avg / exp_avg_sq, five groups at off_*[5] = xyz, rotation,
 *   shs, opacity, scaling) after clone / split / prune in one pass: new Gaussian i copies old Gaussian src[i]; fresh[i] != 0
 *   zeroes its Adam moments; ovr[i] >= 0 takes position and log-scale from row ovr[i] of ovr_xyz / ovr_scale (split children).
 *   The selection itself (masks, top-k, sampling) is host logic (igs_amd/densify.py: plan) or igs_densify_plan below. */
int igs_densify_stats(void* stream, int P, const float* dL_dmean2D, const int* radii, float* grad_accum, float* denom, float* max_radii);
int igs_densify_remap(void* stream, int P_new, int M, const int* src, const int* fresh, const int* ovr, const float* ovr_xyz,
                      const float* ovr_scale, const float* param_old, const float* exp_avg_old, const float* exp_avg_sq_old,
                      const size_t* off_old, float* param_new, float* exp_avg_new, float* exp_avg_sq_new, const size_t* off_new);

/* igs_densify_plan (densify.hip): the densify-and-prune decision on the device -- what igs_amd/densify.py: plan computes with PyTorch
 * (gaussian_model.py:586-663), as the gather plan igs_densify_remap executes.  All inputs are float32 device arrays of the P current
 * Gaussians: the raw leaves xyz [P,3], rotation [P,4] (w, x, y, z; normalised here), opacity_logit [P], log_scale [P,3], the statistics
 * grad_accum [P] and denom [P], and normals [P,2,3], the standard-normal draw of child c of Gaussian i at [i][c] (NULL: zeros, for calls
 * in which nothing can split).
 *   - g = grad_accum / denom; a NaN (0/0) and a negative value count as 0, +inf stays.  Candidate: g >= grad_threshold.
 *   - control_max != 0 and more than max_num_add candidates: only the max_num_add candidates with the largest g stay, ties at the cut
 *     going to the lowest index (torch.topk leaves them unspecified); none stay for max_num_add <= 0.
 *   - big = max_c exp(log_scale[c]) > split_scale_limit (= percent_dense * extent).  A candidate that is not big is cloned (the row is kept
 *     and copied), a big one is split: the original leaves and two children take its place.  Child c of the j-th split source (ascending
 *     index) is row c * n_split + j of ovr_xyz / ovr_scale:  ovr_xyz = R(q / |q|) (normals[i][c] * exp(log_scale)) + xyz,
 *     ovr_scale = log(exp(log_scale) / 1.6).  All 2 n_split rows are written.
 *   - A row is pruned when sigmoid(opacity_logit) of its source < min_opacity, and, with world_scale_limit > 0 (= 0.1 * extent), when its
 *     own largest scale (the child's for children) exceeds that limit.
 *   - Output: rows 0 .. P_new - 1 of src / fresh / ovr (capacity 2 P each; ovr_xyz / ovr_scale: [2 P, 3]) in the order of `plan`: the
 *     surviving originals by index, the surviving clones by index, the surviving children with c = 0, then those with c = 1.
 *     src = source row, fresh = 1 for clones and children, ovr = the child's row of ovr_xyz / ovr_scale, else -1.
 *     counts (device int[4]) = {P_new, n_clone, n_split, n_pruned}; n_pruned counts the removed rows other than the split originals.
 *   - scratch: igs_densify_plan_scratch_bytes(P) bytes (0 for P out of range: 0 <= P <= 2^28), not initialised by the caller.
 *   - 9 launches with control_max, 4 without; no host wait, no atomics that decide an order: two calls give identical bits.
 *   - Refused with IGS_RAST_E_INVALID and a message before any HIP call: P out of range, a grad_threshold that is not finite and > 0,
 *     with P > 0 a NULL pointer other than normals.  P == 0 returns 0, launches nothing and writes nothing. */
size_t igs_densify_plan_scratch_bytes(int P);
int igs_densify_plan(void* stream, int P, const float* xyz, const float* rotation, const float* opacity_logit, const float* log_scale,
                     const float* grad_accum, const float* denom, const float* normals, float grad_threshold, float min_opacity,
                     float split_scale_limit, float world_scale_limit, long long max_num_add, int control_max, void* scratch,
                     int* src, int* fresh, int* ovr, float* ovr_xyz, float* ovr_scale, int* counts);

/* Fused activations applied outside the rasterizer (igs/models/gaussian_model.py:90-127): opacity = sigmoid(logit),
 * scale = exp(log_scale), rotation = F.normalize(rot) (eps 1e-12); and their backward. */
int igs_activate_fwd(void* stream, int P, const float* logit, const float* log_scale, const float* rot, float* opacity,
                     float* scale, float* rot_n);
int igs_activate_bwd(void* stream, int P, const float* opacity, const float* scale, const float* rot, const float* d_opacity,
                     const float* d_scale, const float* d_rot, float* g_logit, float* g_log_scale, float* g_rot);

#ifdef __cplusplus
}
#endif
#endif
