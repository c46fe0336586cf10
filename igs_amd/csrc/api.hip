// api.hip -- the rasterizer and the refine step: their C-ABI entry points (include/igs_rast.h) and host-side orchestration on a HIP
// stream (status slots, binning, forward, backward, fused refine step), plus the error message behind igs_rast_last_error().
// Every other subsystem's entry points are defined next to its kernels (host_api.h: the error plumbing they share).
// Counterpart of CudaRasterizer::Rasterizer::{forward,backward,markVisible}
// (DGR/cuda_rasterizer/rasterizer_impl.cu:176-188, 254-425, 429-571).
#include <atomic>
#include "common.h"
#include "host_api.h"
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <time.h>

static thread_local char g_err[512] = "";
int fail(int code, const char* what, hipError_t e)
{
    if (e != hipSuccess) snprintf(g_err, sizeof g_err, "%s: %s", what, hipGetErrorString(e));
    else snprintf(g_err, sizeof g_err, "%s", what);
    return code;
}
int fail_in(const char* fn, const char* what)
{
    snprintf(g_err, sizeof g_err, "%s: %s", fn, what);
    return IGS_RAST_E_INVALID;
}
// IGS_TRACE_LAUNCHES=1 (debugging aid): synchronise after every launch like debug mode and name it on stderr once it has completed --
// after a GPU memory fault (which aborts the process) the launch that follows the last name printed is the one that faulted
static const bool g_trace_launches = getenv("IGS_TRACE_LAUNCHES") != nullptr;
#define DBG_SYNC(what) do { if (debug || g_trace_launches) { hipError_t e_ = hipStreamSynchronize(s); if (e_ != hipSuccess) return fail(IGS_RAST_E_HIP, what, e_); \
                                                              if (g_trace_launches) { fprintf(stderr, "[igs] completed: %s\n", what); fflush(stderr); } } } while (0)

// pinned status slot + event: one per host thread AND device, kept until the thread ends (a blend kernel still running on the
// device used before may yet post into its slot, so switching devices never frees one)
// Slot 0 (`pinned`) is the single-view entry points'; the multi-view forward (igs_rast_forward_views) posts view v's status into slot
// 1 + v of `views`, one 64-byte line each, allocated by the first such call.
struct HostSlot { uint32_t* pinned = nullptr; uint32_t* pinned_dev = nullptr; hipEvent_t ev = nullptr; uint32_t* views = nullptr; uint32_t* views_dev = nullptr; };
#define IGS_MAX_DEVICES 64
#define VIEW_SLOT_WORDS 16
struct HostSlots {
    HostSlot slot[IGS_MAX_DEVICES];
    ~HostSlots() { for (auto& h : slot) { if (h.pinned) { (void)hipHostFree(h.pinned); (void)hipEventDestroy(h.ev); } if (h.views) (void)hipHostFree(h.views); } }
};
static thread_local HostSlots g_slots;
static thread_local HostSlot g_slot;                // the current device's slot (a copy of the table entry)
static thread_local hipStream_t g_status_stream = nullptr;
static thread_local uint32_t g_host_seq = 0;      // sequence number of the last status the blend kernel was asked to post
static thread_local uint32_t g_nowait_seq = 0;    // ... and the one baked into the last igs_rast_forward_nowait (a capture): what igs_rast_last_status expects
static int ensure_slot()
{
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev), "hipGetDevice");
    if (dev < 0 || dev >= IGS_MAX_DEVICES) return fail(IGS_RAST_E_INVALID, "device ordinal out of range");
    HostSlot& h = g_slots.slot[dev];
    if (!h.pinned) {
        HIP_TRY(hipHostMalloc((void**)&h.pinned, (COUNTER_SHARDS + 1) * COUNTER_SHARD_STRIDE * 4, hipHostMallocDefault), "hipHostMalloc");
        HIP_TRY(hipHostGetDevicePointer((void**)&h.pinned_dev, h.pinned, 0), "hipHostGetDevicePointer");
        HIP_TRY(hipEventCreateWithFlags(&h.ev, hipEventDisableTiming), "hipEventCreate");
    }
    g_slot = h;
    return 0;
}
// ... and the current device's view slots 1 .. IGS_VIEWS_MAX
static int ensure_view_slots()
{
    if (int rc = ensure_slot()) return rc;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev), "hipGetDevice");
    HostSlot& h = g_slots.slot[dev];
    if (!h.views) {
        HIP_TRY(hipHostMalloc((void**)&h.views, IGS_VIEWS_MAX * VIEW_SLOT_WORDS * 4, hipHostMallocDefault), "hipHostMalloc");
        HIP_TRY(hipHostGetDevicePointer((void**)&h.views_dev, h.views, 0), "hipHostGetDevicePointer");
        memset(h.views, 0, IGS_VIEWS_MAX * VIEW_SLOT_WORDS * 4);
    }
    g_slot = h;
    return 0;
}
// status slot k of the current device as the host and as the device address it (k = 0: the single-view slot)
static uint32_t* slot_host(int k) { return k ? g_slot.views + (size_t)(k - 1) * VIEW_SLOT_WORDS : g_slot.pinned; }
static uint32_t* slot_dev(int k) { return k ? g_slot.views_dev + (size_t)(k - 1) * VIEW_SLOT_WORDS : g_slot.pinned_dev; }

static double now_s() { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec; }
static double wait_limit_s()
{
    static double lim = -1.0;
    if (lim < 0.0) { const char* e = getenv("IGS_RAST_WAIT_TIMEOUT_S"); lim = e ? atof(e) : 10.0; if (!(lim > 0.0)) lim = 10.0; }
    return lim;
}

// Waits until the blend kernel of the current slab-binned frame has posted {R, overflow, prefilter flag} into pinned host
// memory: a poll on the sequence word instead of an event -- an event record between blend_fwd and blend_bwd costs the stream
// a ~6 us bubble per step, and the first workgroup posts at the START of the kernel, so the host is released earlier too.
// Bounded: a stream that reports an error, a stream that drains without the post, or IGS_RAST_WAIT_TIMEOUT_S (default 10)
// seconds of wall clock without it all end the wait with IGS_RAST_E_HIP.
static int wait_status(hipStream_t s, const uint32_t* pinned, uint32_t want)
{
    volatile uint32_t* seq = (volatile uint32_t*)&pinned[3];
    double t0 = 0.0;
    for (long spins = 0;; spins++) {
        if (__atomic_load_n(seq, __ATOMIC_ACQUIRE) == want) return 0;
        if ((spins & 0x3FFF) == 0x3FFF) {
            const hipError_t q = hipStreamQuery(s);
            if (q != hipSuccess && q != hipErrorNotReady) return fail(IGS_RAST_E_HIP, "stream error while waiting for the frame status", q);
            if (q == hipSuccess && __atomic_load_n(seq, __ATOMIC_ACQUIRE) != want)
                return fail(IGS_RAST_E_HIP, "the frame status was never posted");
            const double t = now_s();
            if (t0 == 0.0) t0 = t;
            else if (t - t0 > wait_limit_s())
                return fail(IGS_RAST_E_HIP, "timed out waiting for the frame status (IGS_RAST_WAIT_TIMEOUT_S)");
        }
    }
}

static int ceil_log2(uint32_t n) { int b = 0; while ((1u << b) < n) b++; return b; }

// ---- optional per-stage timing with HIP events on the caller's stream (roofline harness, bench.py) ----
enum { ST_PREPROCESS = 0, ST_DEPTH_SORT, ST_SCAN, ST_EMIT, ST_TILE_SORT, ST_RANGES, ST_BLEND_FWD, ST_MEMSET, ST_BLEND_BWD,
       ST_GEOM_BWD, ST_COUNT, ST_GAP = -1 };
struct Prof {
    bool on = false;
    int every = 1; long long frame = 0; bool active = false;     // marks are recorded on every `every`-th frame only
    static const int CAP = 1024;
    hipEvent_t ev[CAP]; int tag[CAP]; int n = 0; bool created = false;
    double ms[ST_COUNT] = {0}; long long cnt[ST_COUNT] = {0}; double r_sum = 0; long long calls = 0;
};
static Prof g_prof;
static void prof_collect()
{
    if (g_prof.n == 0) return;
    (void)hipEventSynchronize(g_prof.ev[g_prof.n - 1]);
    for (int i = 1; i < g_prof.n; i++) {
        const int t = g_prof.tag[i];
        if (t < 0) continue;                       // a mark that only starts a new interval
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, g_prof.ev[i - 1], g_prof.ev[i]) == hipSuccess) { g_prof.ms[t] += ms; g_prof.cnt[t]++; }
    }
    g_prof.n = 0;
}
// records "stage `tag` ended here" (tag = ST_GAP: only a start mark)
static void prof_mark(hipStream_t s, int tag)
{
    if (!g_prof.on || !g_prof.active) return;
    if (g_prof.n >= Prof::CAP - 1) {                // keep the last mark as the start of the next interval
        const hipEvent_t last = g_prof.ev[g_prof.n - 1];
        prof_collect();
        (void)last;
        (void)hipEventRecord(g_prof.ev[0], s); g_prof.tag[0] = ST_GAP; g_prof.n = 1;
        if (tag == ST_GAP) return;
    }
    (void)hipEventRecord(g_prof.ev[g_prof.n], s); g_prof.tag[g_prof.n] = tag; g_prof.n++;
}
// on = 0: off; on = N > 0: record stage marks on every N-th frame (an event record costs a few microseconds of stream time:
// marking every frame slows a 0.35 ms refine step by 10 %, marking every 8th by about 1 %)
extern "C" int igs_rast_profile_enable(int on)
{
    if (!on) prof_collect();
    // (the events are created here, not at the first mark: a thousand hipEventCreate calls take over a millisecond)
    if (on && !g_prof.created) { for (int i = 0; i < Prof::CAP; i++) (void)hipEventCreate(&g_prof.ev[i]); g_prof.created = true; }
    g_prof.on = on != 0; g_prof.every = on > 0 ? on : 1; g_prof.frame = 0; g_prof.active = g_prof.on;
    return 0;
}
static void prof_new_frame() { if (g_prof.on) { g_prof.active = (g_prof.frame % g_prof.every) == 0; g_prof.frame++; } }
extern "C" int igs_rast_profile_read(double* ms_sum, long long* count, double* r_sum, long long* calls, int reset)
{
    prof_collect();
    for (int i = 0; i < ST_COUNT; i++) { if (ms_sum) ms_sum[i] = g_prof.ms[i]; if (count) count[i] = g_prof.cnt[i]; }
    if (r_sum) *r_sum = g_prof.r_sum;
    if (calls) *calls = g_prof.calls;
    if (reset) { for (int i = 0; i < ST_COUNT; i++) { g_prof.ms[i] = 0; g_prof.cnt[i] = 0; } g_prof.r_sum = 0; g_prof.calls = 0; }
    return ST_COUNT;
}

extern "C" int igs_rast_version(void) { return IGS_RAST_VERSION; }
extern "C" const char* igs_rast_last_error(void) { return g_err; }
// workspace = 256-byte aligned { gacc[P][32] doubles | 64 loss shards one cache line apart (refine step) }
static inline size_t ws_gacc_bytes(int P) { return ((size_t)(P > 0 ? P : 0) * GACC_F * 8 + 255) & ~(size_t)255; }
#define WS_LOSS_BYTES 4096
extern "C" size_t igs_rast_backward_workspace_bytes(int P) { return ws_gacc_bytes(P) + WS_LOSS_BYTES + 512; }

// what the previous forward on this host thread saw: sizes the binning buffer before R is known
struct BinHint { uint32_t slab = 0; };              // instance slots per tile used by the last frames (0 = default)
#define SLAB_MAX_BYTES (8ull << 30)                 // beyond this much slab scratch the global-sort path is used
static thread_local BinHint g_hint;
// a frame's largest tile needed `overflow` instance slots, more than its slab had: the slab that fits it with a quarter to spare (at
// most TILE_SORT_BIG: denser tiles take the global sort)
static uint32_t slab_hint_for(uint32_t overflow)
{
    const uint64_t want = ((uint64_t)overflow + overflow / 4 + 255) / 256 * 256;
    return (uint32_t)(want > TILE_SORT_BIG ? TILE_SORT_BIG : want);
}
// igs_rast_forward_async leaves its host-side check of R to igs_rast_forward_finish
struct PendingFwd { bool active = false; uint32_t slab = 0; };
static thread_local PendingFwd g_pending;

// the reference's forward argument list (CudaRasterizer::Rasterizer::forward), in the order of igs_rast_forward's parameters
struct FwdIn {
    hipStream_t s; igs_rast_alloc_fn geometry_buffer; void* geometry_user; igs_rast_alloc_fn binning_buffer; void* binning_user;
    igs_rast_alloc_fn image_buffer; void* image_user; int P, D, M; const float* background; int width, height;
    const float *means3D, *shs, *colors_precomp, *opacities, *scales; float scale_modifier; const float *rotations, *cov3D_precomp;
    const float *viewmatrix, *projmatrix, *cam_pos; float tan_fovx, tan_fovy, kernel_size; int prefiltered;
    float *out_color, *out_coord, *out_mcoord, *out_depth, *out_mdepth, *out_alpha, *out_normal; int* radii; int require_coord, require_depth, debug;
};
// the parameter list of igs_rast_forward, _async and _nowait (include/igs_rast.h), and the FwdIn made from it
#define FWD_PARAMS                                                                                                                        \
    void* stream, igs_rast_alloc_fn geometry_buffer, void* geometry_user, igs_rast_alloc_fn binning_buffer, void* binning_user,           \
    igs_rast_alloc_fn image_buffer, void* image_user, int P, int D, int M, const float* background, int width, int height,               \
    const float* means3D, const float* shs, const float* colors_precomp, const float* opacities, const float* scales,                     \
    float scale_modifier, const float* rotations, const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,          \
    const float* cam_pos, float tan_fovx, float tan_fovy, float kernel_size, int prefiltered, float* out_color, float* out_coord,        \
    float* out_mcoord, float* out_depth, float* out_mdepth, float* out_alpha, float* out_normal, int* radii, int require_coord,            \
    int require_depth, int debug
#define FWD_IN                                                                                                                            \
    FwdIn{ (hipStream_t)stream, geometry_buffer, geometry_user, binning_buffer, binning_user, image_buffer, image_user, P, D, M,          \
           background, width, height, means3D, shs, colors_precomp, opacities, scales, scale_modifier, rotations, cov3D_precomp,           \
           viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy, kernel_size, prefiltered, out_color, out_coord, out_mcoord, out_depth,     \
           out_mdepth, out_alpha, out_normal, radii, require_coord, require_depth, debug }

// what the extended entry points ask of the forward on top of the reference's argument list
struct FwdExtra {
    bool defer_status = false;          // igs_rast_forward_async / igs_refine_step: do not wait for {R, overflow}
    bool no_latch = false;              // igs_rast_forward_nowait: ... and do not expect an igs_rast_forward_finish either
    bool raw_activations = false;       // igs_refine_step: opacities / scales / rotations are the raw optimiser leaves
    double* zero_gacc = nullptr;        // ... backward accumulators / loss shards the preprocess kernel zero-fills on the side
    float* zero_loss = nullptr;
    float* zero_loss2 = nullptr;
    bool scratch_clean = false;         // igs_refine_step_args::scratch_clean: the image buffer's binning counters are known clean
    int zero_gacc_first = 0;            // ... masked refine step: accumulator rows exist for Gaussians [zero_gacc_first, P) only
    bool skip_bwd_state = false;        // ... the loss is colour-only: blend_fwd need not store the geometry branches' backward state
    uint32_t plane_tag = 0;             // ... nonzero: a plane / depth / normal gradient will come back: keep Sigma^-1 per Gaussian under this tag
    // igs_refine_step with the L1 loss: run the colour-only blend backward inside the forward's tile kernel (blend_step.hip).  The
    // caller fills everything of the backward's arguments that the forward does not know (bg, gacc, l1_*, want_absgrad); the
    // list / record / geometry fields are set by launch_blend.  *fused_ran reports whether that kernel was used (slab binning only).
    BlendBwdArgs* fused_bwd = nullptr;
    bool* fused_ran = nullptr;
    int* fused_instance = nullptr;
    // igs_rast_count_gaussians: vanilla preprocess (dilated conic, raw opacity) and the counting colour-only blend (blend_count.hip);
    // the per-Gaussian pixel counts land here (zeroed by the preprocess of every attempt, so a redone frame counts once)
    int* count = nullptr;
    int status_slot = 0;                // igs_rast_forward_views: the pinned slot view v's blend kernel posts into (1 + v)
};
// where the last slab-binned forward left its device-side validity words (refine step guards)
struct LastFwd { const uint32_t* overflow = nullptr; const uint32_t* prefilter = nullptr; };
static thread_local LastFwd g_last_fwd;
// a slab-binned forward of this thread got as far as its binning kernel but not to its tile sort: some buffer's counters are not clean
static thread_local bool g_counters_dirty = false;
// one-shot promise for the NEXT forward of this thread (igs_rast_hint_scratch_clean)
static thread_local bool g_hint_clean = false;
extern "C" void igs_rast_hint_scratch_clean(int on) { g_hint_clean = on != 0; }

// one forward frame: its sizes, the caller's geometry and image scratch (requested anew by every attempt) and the preprocess parameters
struct Frame {
    const FwdIn& in; const FwdExtra& ex; int gx, gy; size_t Tn; GeomLayout GL; ImgLayout IL;
    char* gbase = nullptr; char* ibase = nullptr; FwdParams fp;
    Frame(const FwdIn& i, const FwdExtra& e)
        : in(i), ex(e), gx((i.width + TILE - 1) / TILE), gy((i.height + TILE - 1) / TILE), Tn((size_t)gx * gy), GL(i.P),
          IL((size_t)i.width * i.height, Tn) {}
    uint32_t* gbuf(size_t off) const { return (uint32_t*)(gbase + off); }
    uint32_t* ibuf(size_t off) const { return (uint32_t*)(ibase + off); }
    float* rec() const { return (float*)(gbase + GL.rec); }
};
static int carve_frame(Frame& f)
{
    const FwdIn& in = f.in; const FwdExtra& ex = f.ex;
    char* gbase = in.geometry_buffer(in.geometry_user, f.GL.total);
    if (!gbase) return fail(IGS_RAST_E_ALLOC, "geometry buffer callback returned NULL");
    f.gbase = align_ptr(gbase);
    char* ibase = in.image_buffer(in.image_user, f.IL.total);
    if (!ibase) return fail(IGS_RAST_E_ALLOC, "image buffer callback returned NULL");
    f.ibase = align_ptr(ibase);
    FwdParams& fp = f.fp = FwdParams();
    fp.P = in.P; fp.D = in.D; fp.M = in.M; fp.W = in.width; fp.H = in.height; fp.gx = f.gx; fp.gy = f.gy;
    fp.means3D = in.means3D; fp.shs = in.shs; fp.colors_precomp = in.colors_precomp; fp.opacities = in.opacities; fp.scales = in.scales;
    fp.rotations = in.rotations; fp.cov3D_precomp = in.cov3D_precomp; fp.scale_modifier = in.scale_modifier; fp.tan_fovx = in.tan_fovx;
    fp.tan_fovy = in.tan_fovy; fp.fy = in.height / (2.0f * in.tan_fovy); fp.fx = in.width / (2.0f * in.tan_fovx);       // rasterizer_impl.cu:288-289
    fp.kernel_size = in.kernel_size; fp.prefiltered = in.prefiltered; fp.view = in.viewmatrix; fp.proj = in.projmatrix; fp.campos = in.cam_pos;
    fp.raw_activations = ex.raw_activations ? 1 : 0;
    fp.zero_gacc = ex.zero_gacc; fp.zero_loss = ex.zero_loss; fp.zero_loss2 = ex.zero_loss2; fp.zero_gacc_first = ex.zero_gacc_first;
    if (ex.plane_tag) { fp.plane_cache = (float*)(f.gbase + f.GL.planes); fp.plane_tag = ex.plane_tag; }
    fp.zero_gacc_stride = ex.skip_bwd_state ? GACC_COMPACT_F : GACC_F;      // (colour-only loss <=> compact accumulator rows)
    g_last_fwd = LastFwd();
    return 0;
}

// what a binning stage leaves for the blend
struct Binned {
    uint32_t* ranges = nullptr; uint32_t* point_list = nullptr; uint32_t R = 0;      // (R: global sort only)
    const uint32_t* slab_stats = nullptr;    // slab binning: {R, overflow, prefilter flag} on the device, posted by the blend kernel
    uint32_t slab_size = 0;
    bool pending = false;                    // slab binning: the host has not looked at R yet
    bool fuse_tiles = false, step_order = false;      // ... the fused refine step's tile kernel runs; the tile sort wrote its dispatch order
};

// slab binning (default): nothing here needs the host to know R
static int bin_slab(Frame& f, uint32_t slab, Binned& b)
{
    const hipStream_t s = f.in.s; const int debug = f.in.debug;
    uint32_t *tile_count = f.ibuf(f.IL.tile_count), *stats = f.ibuf(f.IL.stats), *counters = f.ibuf(f.IL.counters);
    const SlabLayout KL(f.Tn, slab);
    char* bbase = f.in.binning_buffer(f.in.binning_user, KL.total);
    if (!bbase) return fail(IGS_RAST_E_ALLOC, "binning buffer callback returned NULL");
    bbase = align_ptr(bbase);
    b.ranges = f.ibuf(f.IL.ranges); b.point_list = (uint32_t*)(bbase + KL.point_list); b.slab_size = slab;
    uint64_t* pairs = (uint64_t*)(bbase + KL.pairs);
    // The tile sort leaves the fill cursors and the count shards zeroed behind it, so a buffer that was clean before a frame is clean
    // after it: a caller that vouches for its buffer (igs_refine_step_args::scratch_clean) skips the zero-fill launch, unless
    // something on this thread was cut short between a binning kernel and its tile sort (g_counters_dirty).
    if (f.ex.scratch_clean && !g_counters_dirty) f.fp.zero_stats = stats;
    else HIP_TRY(zero_fill_async(s, tile_count, f.IL.zero_end - f.IL.tile_count), "zero tile counters");   // tile_count + stats + counters
    g_counters_dirty = true;
    prof_mark(s, ST_GAP);
    HIP_TRY(launch_preprocess_fwd(s, f.fp, f.rec(), f.gbuf(f.GL.tiles), nullptr, nullptr, f.in.radii, counters, nullptr, 0, tile_count,
                                  pairs, slab, f.ex.count), "preprocess_fwd launch");
    DBG_SYNC("preprocess_fwd");
    prof_mark(s, ST_PREPROCESS);
    // fused refine step: the tile sort also writes the blend kernel's dispatch order and leaves the fill cursors for that kernel to zero
    static const bool no_step_order = getenv("IGS_NO_STEP_ORDER") != nullptr;      // (A/B switch for measurements)
    b.fuse_tiles = f.ex.fused_bwd && f.ex.skip_bwd_state && !f.in.colors_precomp && (f.in.require_coord != 0) == (f.in.require_depth != 0);
    b.step_order = b.fuse_tiles && !no_step_order && step_order_usable((uint32_t)f.gx, (uint32_t)f.gy, slab);
    HIP_TRY(launch_tile_sort(s, (uint32_t)f.Tn, tile_count, pairs, b.point_list, b.ranges, slab, stats, counters, (uint32_t)f.in.P,
                             b.step_order ? f.ibuf(f.IL.tile_order) : nullptr, (uint32_t)f.gx, (uint32_t)f.gy), "tile_sort launch");
    g_counters_dirty = b.step_order;          // (then clean only once the blend kernel has been launched)
    DBG_SYNC("tile_sort");
    prof_mark(s, ST_TILE_SORT);
    b.slab_stats = stats; b.pending = true;
    g_last_fwd.overflow = stats + 1; g_last_fwd.prefilter = stats + 2;      // (the tile sort moved the flag there)
    return 0;
}

// global radix binning (fallback for tiles denser than TILE_SORT_BIG): the host reads R back before it sizes the binning buffer
static int bin_radix(Frame& f, Binned& b)
{
    const hipStream_t s = f.in.s; const int debug = f.in.debug; const int P = f.in.P;
    const size_t counter_bytes = (COUNTER_SHARDS + 1) * COUNTER_SHARD_STRIDE * 4;
    uint32_t *counters = f.gbuf(f.GL.counters), *tiles = f.gbuf(f.GL.tiles), *ghist = f.gbuf(f.GL.hist), *blocksum = f.gbuf(f.GL.blocksum);
    RadixBufs dsort{f.gbuf(f.GL.keys_a), f.gbuf(f.GL.keys_b), f.gbuf(f.GL.vals_a), f.gbuf(f.GL.vals_b), ghist};      // the depth sort
    HIP_TRY(hipMemsetAsync(counters, 0, counter_bytes, s), "memset counters");

    HIP_TRY(radix_sort_begin(s, (uint32_t)P, dsort), "zero depth-sort histogram 0");
    prof_mark(s, ST_GAP);
    HIP_TRY(launch_preprocess_fwd(s, f.fp, f.rec(), tiles, dsort.ka, dsort.va, f.in.radii, counters, ghist, dsort.per_block, nullptr, nullptr, 0, f.ex.count),
            "preprocess_fwd launch");
    DBG_SYNC("preprocess_fwd");
    prof_mark(s, ST_PREPROCESS);
    // instance count: read back while the depth sort runs
    HIP_TRY(hipMemcpyAsync(g_slot.pinned, counters, counter_bytes, hipMemcpyDeviceToHost, s), "memcpy count");
    HIP_TRY(hipEventRecord(g_slot.ev, s), "event record");
    prof_mark(s, ST_GAP);

    HIP_TRY(radix_sort_pairs(s, (uint32_t)P, dsort, 0, 32), "depth sort launch");
    const uint32_t* order = dsort.sorted_vals(32);
    DBG_SYNC("depth sort");
    prof_mark(s, ST_DEPTH_SORT);
    const int nblk = (P + 255) / 256;
    HIP_TRY(launch_count_sorted(s, P, order, tiles, blocksum), "count_sorted launch");
    HIP_TRY(launch_exclusive_scan(s, nblk, blocksum), "exclusive scan launch");
    DBG_SYNC("scan");
    prof_mark(s, ST_SCAN);

    HIP_TRY(hipEventSynchronize(g_slot.ev), "event sync");
    uint64_t R64 = 0;
    for (int sh = 0; sh < COUNTER_SHARDS; sh++) R64 += g_slot.pinned[COUNTER_SHARD_STRIDE * (1 + sh)];
    if (R64 > 0x7FFFFFFFull) return fail(IGS_RAST_E_INVALID, "instance count overflows int");
    const uint32_t R = b.R = (uint32_t)R64;
    if (g_slot.pinned[1]) return fail(IGS_RAST_E_PREFILTER, "Point is filtered although prefiltered is set. This shouldn't happen!");

    const BinLayout BL(R);
    char* bbase = f.in.binning_buffer(f.in.binning_user, BL.total);
    if (!bbase) return fail(IGS_RAST_E_ALLOC, "binning buffer callback returned NULL");
    bbase = align_ptr(bbase);
    uint32_t* point_list = b.point_list = (uint32_t*)(bbase + BL.point_list);
    uint32_t *bkeys_a = (uint32_t*)(bbase + BL.keys_a), *bkeys_b = (uint32_t*)(bbase + BL.keys_b), *bvals_b = (uint32_t*)(bbase + BL.vals_b);
    uint32_t* bhist = (uint32_t*)(bbase + BL.hist);
    uint32_t* ranges = b.ranges = f.ibuf(f.IL.ranges);

    HIP_TRY(hipMemsetAsync(ranges, 0, f.Tn * 8, s), "memset ranges");               // rasterizer_impl.cu:383
    prof_mark(s, ST_GAP);
    if (R == 0) return 0;
    const int bits = ceil_log2((uint32_t)f.Tn);
    // arrange the ping-pong so that the sorted ids land in point_list
    RadixBufs tsort = radix_lands_in_b(bits) ? RadixBufs{bkeys_b, bkeys_a, bvals_b, point_list, bhist}
                                             : RadixBufs{bkeys_a, bkeys_b, point_list, bvals_b, bhist};
    HIP_TRY(radix_sort_begin(s, R, tsort), "zero tile-sort histogram 0");
    const uint32_t mask0 = bits >= 8 ? 255u : ((1u << bits) - 1u);
    HIP_TRY(launch_emit_instances(s, P, f.gx, f.gy, order, tiles, blocksum, f.rec(), f.in.radii, tsort.ka, tsort.va, bits ? bhist : nullptr,
                                  tsort.per_block, mask0), "emit launch");
    DBG_SYNC("emit");
    prof_mark(s, ST_EMIT);
    HIP_TRY(radix_sort_pairs(s, R, tsort, 0, bits), "tile sort launch");
    DBG_SYNC("tile sort");
    prof_mark(s, ST_TILE_SORT);
    HIP_TRY(launch_tile_ranges(s, R, tsort.sorted_keys(bits), ranges), "tile_ranges launch");
    DBG_SYNC("tile_ranges");
    prof_mark(s, ST_RANGES);
    return 0;
}

// the blend kernel of the frame: the count pass's, the fused refine step's (forward + colour-only backward of a tile) or the plain one
static int launch_blend(const Frame& f, const Binned& b)
{
    const FwdIn& in = f.in; const FwdExtra& ex = f.ex; const hipStream_t s = in.s; const int debug = in.debug;
    BlendFwdArgs ba;
    ba.W = in.width; ba.H = in.height; ba.gx = f.gx; ba.gy = f.gy; ba.fx = f.fp.fx; ba.fy = f.fp.fy; ba.bg = in.background;
    ba.ranges = b.ranges; ba.point_list = b.point_list; ba.rec = f.rec(); ba.colors_precomp = in.colors_precomp;
    ba.out_color = in.out_color; ba.out_coord = in.out_coord; ba.out_mcoord = in.out_mcoord; ba.out_depth = in.out_depth;
    ba.out_mdepth = in.out_mdepth; ba.out_alpha = in.out_alpha; ba.out_normal = in.out_normal;
    ba.n_contrib = f.ibuf(f.IL.n_contrib);
    ba.accum_coord = (float*)f.ibuf(f.IL.accum_coord); ba.accum_depth = (float*)f.ibuf(f.IL.accum_depth);
    ba.normal_length = (float*)f.ibuf(f.IL.normal_length);
    ba.stats_src = b.slab_stats; ba.flag_src = b.slab_stats ? b.slab_stats + 2 : f.gbuf(f.GL.counters) + 1;
    ba.host_dst = b.pending ? slot_dev(ex.status_slot) : nullptr;
    ba.tile_order = f.ibuf(f.IL.tile_order);          // built on the side for the backward (both binning paths)
    ba.skip_bwd_state = ex.skip_bwd_state ? 1 : 0;
    if (b.pending) { g_host_seq = g_host_seq + 1 ? g_host_seq + 1 : 1; slot_host(ex.status_slot)[3] = 0; }
    ba.host_seq = g_host_seq;
    if (b.pending && ex.no_latch) g_nowait_seq = g_host_seq;
    g_status_stream = s;
    if (ex.fused_ran) *ex.fused_ran = b.fuse_tiles;
    if (ex.count) {
        ba.tile_order = nullptr;                 // (no backward follows a count pass)
        HIP_TRY(launch_blend_count(s, ba, ex.count), "blend_count launch");
    } else if (b.fuse_tiles) {
        BlendBwdArgs& bb = *ex.fused_bwd;
        bb.W = in.width; bb.H = in.height; bb.gx = f.gx; bb.gy = f.gy; bb.fx = f.fp.fx; bb.fy = f.fp.fy; bb.bg = in.background;
        bb.ranges = b.ranges; bb.point_list = b.point_list; bb.rec = f.rec(); bb.colors_precomp = nullptr;
        bb.tile_order = nullptr;
        ba.tile_order = nullptr;                 // (no separate backward kernel that could use a load order)
        if (b.step_order) { ba.step_order = f.ibuf(f.IL.tile_order); ba.reset_cursors = f.ibuf(f.IL.tile_count); }
        HIP_TRY(launch_blend_step(s, ba, bb, in.require_coord != 0, in.require_depth != 0, ex.fused_instance), "blend_step launch");
        if (b.step_order) g_counters_dirty = false;
    } else {
        HIP_TRY(launch_blend_fwd(s, ba, in.require_coord != 0, in.require_depth != 0), "blend_fwd launch");
    }
    DBG_SYNC("blend_fwd");
    prof_mark(s, ST_BLEND_FWD);
    return 0;
}

// what the blend kernel of a slab-binned frame posts into pinned host memory: R, the largest tile that overflowed its slab (0 = none),
// the prefilter flag -- and, stored last, the sequence number p[3]
struct FrameStatus { uint32_t R, overflow, prefilter; };
static FrameStatus read_status(const uint32_t* p) { return { __atomic_load_n(&p[0], __ATOMIC_ACQUIRE), __atomic_load_n(&p[1], __ATOMIC_ACQUIRE), p[2] }; }
// waits for the status of the current slab-binned frame and checks it: returns R or an error; *overflow as posted
static int collect_status(hipStream_t s, uint32_t* overflow, int slot = 0, uint32_t seq = g_host_seq)
{
    const uint32_t* pinned = slot_host(slot);
    if (int rc = wait_status(s, pinned, seq)) return rc;
    const FrameStatus st = read_status(pinned);
    *overflow = st.overflow;
    if (st.prefilter) return fail(IGS_RAST_E_PREFILTER, "Point is filtered although prefiltered is set. This shouldn't happen!");
    if (st.R > 0x7FFFFFFFu) return fail(IGS_RAST_E_INVALID, "instance count overflows int");
    return (int)st.R;
}

// Checks the arguments, then renders the frame: binning, blend and -- unless it is deferred -- the host's look at the status.  The
// attempts, in order: slabs of the sticky size; the global sort at once if those slabs would exceed 32-bit list positions or
// SLAB_MAX_BYTES; after a slab overflow, slabs of at least the overflowing tile's count, or the global sort above TILE_SORT_BIG.
static int forward_impl(const FwdIn& in, const FwdExtra& ex, bool radix)
{
    if (in.P < 0 || in.width <= 0 || in.height <= 0) return fail(IGS_RAST_E_INVALID, "igs_rast_forward: bad sizes");
    if (in.P == 0) return 0;                                       // rasterize_points.cu:90: nothing is launched
    if (!in.geometry_buffer || !in.binning_buffer || !in.image_buffer) return fail(IGS_RAST_E_INVALID, "igs_rast_forward: NULL scratch callback");
    if (!in.means3D || !in.opacities || !in.viewmatrix || !in.projmatrix || !in.cam_pos || !in.background || !in.radii)
        return fail(IGS_RAST_E_INVALID, "igs_rast_forward: NULL required input");
    if (!in.out_color || (!ex.count && (!in.out_coord || !in.out_mcoord || !in.out_depth || !in.out_mdepth || !in.out_alpha || !in.out_normal)))
        return fail(IGS_RAST_E_INVALID, "igs_rast_forward: NULL output");
    if (!in.colors_precomp && !in.shs) return fail(IGS_RAST_E_INVALID, "igs_rast_forward: neither shs nor colors_precomp");
    if (!in.cov3D_precomp && (!in.scales || !in.rotations)) return fail(IGS_RAST_E_INVALID, "igs_rast_forward: neither scales/rotations nor cov3D_precomp");
    if (!in.colors_precomp && (in.M < (in.D + 1) * (in.D + 1) || in.D < 0 || in.D > 3))
        return fail(IGS_RAST_E_INVALID, "igs_rast_forward: SH degree / coefficient count mismatch");
    if (int rc = ensure_slot()) return rc;

    Frame f(in, ex);
    uint64_t min_capacity = 0;
    for (;;) {
        // slab size: sticky per thread, grown when a frame overflowed (the refine loop renders similar views over and over)
        uint64_t slab = g_hint.slab ? g_hint.slab : 1024;
        if (min_capacity > slab) slab = (min_capacity + 255) / 256 * 256;
        if (slab > TILE_SORT_BIG) slab = TILE_SORT_BIG;
        if (f.Tn * slab > 0x7FFFFFFFull || f.Tn * slab * 12 > SLAB_MAX_BYTES) radix = true;      // (32-bit list positions / a sane scratch size)
        if (int rc = carve_frame(f)) return rc;
        Binned b;
        if (int rc = radix ? bin_radix(f, b) : bin_slab(f, (uint32_t)slab, b)) return rc;
        if (int rc = launch_blend(f, b)) return rc;
        if (b.pending && ex.defer_status) {
            if (!ex.no_latch) { g_pending.active = true; g_pending.slab = b.slab_size; }
            if (g_prof.on) g_prof.calls++;
            return 0x7FFFFFFF;                   // "unknown yet": an upper bound that igs_rast_backward accepts as R
        }
        // slab binning: only now does the host look at R -- the whole pipeline above was enqueued without waiting for it
        uint32_t overflow = 0;
        const int R = b.pending ? collect_status(in.s, &overflow) : (int)b.R;
        if (R < 0) return R;
        if (!overflow) { if (g_prof.on) { g_prof.r_sum += (double)R; g_prof.calls++; } return R; }
        // a tile holds more instances than its slab (overflow = the largest such tile): redo with what is now known
        g_hint.slab = slab_hint_for(overflow);
        radix = overflow > (uint32_t)TILE_SORT_BIG;
        min_capacity = overflow;
    }
}

// IGS_BINNING=radix forces the global-sort path (tests)
static bool radix_forced() { const char* e = getenv("IGS_BINNING"); return e && strcmp(e, "radix") == 0; }

// the common preamble of igs_rast_forward (Sync), igs_rast_forward_async (Deferred) and igs_rast_forward_nowait (Capture)
enum class FwdMode { Sync, Deferred, Capture };
static int forward_entry(FwdMode mode, const FwdIn& in)
{
    const bool hint_clean = g_hint_clean; g_hint_clean = false;      // one-shot promise: consumed by THIS call, even a refused one
    if (g_pending.active)          // (the status slot is single: a second frame must not start before the first one's count is collected)
        return fail(IGS_RAST_E_INVALID,
                    mode == FwdMode::Sync ? "igs_rast_forward: an asynchronous forward is pending on this thread; call igs_rast_forward_finish() first"
                    : mode == FwdMode::Deferred ? "igs_rast_forward_async: the previous asynchronous forward has not been finished (igs_rast_forward_finish)"
                    : "igs_rast_forward_nowait: an asynchronous forward is pending on this thread; call igs_rast_forward_finish() first");
    if (mode == FwdMode::Capture) {
        if (in.debug) return fail(IGS_RAST_E_INVALID, "igs_rast_forward_nowait: debug (a synchronisation after every launch) cannot be captured");
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= IGS_MAX_DEVICES || !g_slots.slot[dev].pinned)
            return fail(IGS_RAST_E_INVALID, "igs_rast_forward_nowait: no status slot on this thread and device yet (run one igs_rast_forward first: pinned memory cannot be allocated during capture)");
    }
    prof_new_frame();
    FwdExtra ex;
    ex.scratch_clean = hint_clean;
    ex.defer_status = mode != FwdMode::Sync;
    ex.no_latch = mode == FwdMode::Capture;
    return forward_impl(in, ex, mode == FwdMode::Sync && radix_forced());
}

extern "C" int igs_rast_forward(FWD_PARAMS) { return forward_entry(FwdMode::Sync, FWD_IN); }

// The count pass of the compress rasterizer (CudaRasterizer::Rasterizer::forwardCount, compress rasterizer_impl.cu:441-530): vanilla
// preprocess, the same binning (slab, or the global sort), the counting colour-only blend, then score = count x opacity over P.
// Returns num_rendered or a negative code; every argument is checked before the first HIP call.
extern "C" int igs_rast_count_gaussians(
    void* stream,
    igs_rast_alloc_fn geometry_buffer, void* geometry_user, igs_rast_alloc_fn binning_buffer, void* binning_user,
    igs_rast_alloc_fn image_buffer, void* image_user,
    int P, int D, int M, const float* background, int width, int height,
    const float* means3D, const float* shs, const float* colors_precomp, const float* opacities,
    const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
    const float* viewmatrix, const float* projmatrix, const float* cam_pos,
    float tan_fovx, float tan_fovy, int prefiltered,
    float* out_color, int* count, float* score, int* radii, int debug)
{
    hipStream_t s = (hipStream_t)stream;
    const bool hint_clean = g_hint_clean; g_hint_clean = false;      // (consumed by this call, even a refused one)
    if (P < 0 || width <= 0 || height <= 0) return fail(IGS_RAST_E_INVALID, "igs_rast_count_gaussians: bad sizes");
    if (g_pending.active) return fail(IGS_RAST_E_INVALID, "igs_rast_count_gaussians: an asynchronous forward is pending on this thread; call igs_rast_forward_finish() first");
    if (P == 0) return 0;                                       // rasterize_points.cu CountGaussiansCUDA: nothing is launched
    if (!out_color || !count || !score || !radii) return fail(IGS_RAST_E_INVALID, "igs_rast_count_gaussians: NULL output");
    prof_new_frame();
    FwdIn in{};                                                 // (no kernel_size, no geometry maps)
    in.s = s; in.geometry_buffer = geometry_buffer; in.geometry_user = geometry_user; in.binning_buffer = binning_buffer;
    in.binning_user = binning_user; in.image_buffer = image_buffer; in.image_user = image_user; in.P = P; in.D = D; in.M = M;
    in.background = background; in.width = width; in.height = height; in.means3D = means3D; in.shs = shs; in.colors_precomp = colors_precomp;
    in.opacities = opacities; in.scales = scales; in.scale_modifier = scale_modifier; in.rotations = rotations; in.cov3D_precomp = cov3D_precomp;
    in.viewmatrix = viewmatrix; in.projmatrix = projmatrix; in.cam_pos = cam_pos; in.tan_fovx = tan_fovx; in.tan_fovy = tan_fovy;
    in.prefiltered = prefiltered; in.out_color = out_color; in.radii = radii; in.debug = debug;
    FwdExtra ex; ex.scratch_clean = hint_clean; ex.count = count;
    const int R = forward_impl(in, ex, radix_forced());
    if (R < 0) return R;
    // (after the frame is final: a slab overflow has redone it inside forward_impl)
    HIP_TRY(launch_count_score(s, P, count, opacities, score), "count_score launch");
    DBG_SYNC("count_score");
    return R;
}

// Asynchronous variant for callers that keep enqueueing work (the native refine step): identical to igs_rast_forward but
// returns right after the last launch WITHOUT waiting for the instance count; the return value is INT_MAX ("not known
// yet", which igs_rast_backward accepts as R).  igs_rast_forward_finish() then waits for the small
// read-back (which completed right after the tile scan, long before the blend) and returns the true num_rendered, or
// IGS_RAST_E_RETRY if a tile overflowed its instance slab: everything enqueued since must then be discarded and
// the frame redone with igs_rast_forward (the hints are updated, so it will fit).
extern "C" int igs_rast_forward_async(FWD_PARAMS) { return forward_entry(FwdMode::Deferred, FWD_IN); }
extern "C" int igs_rast_forward_finish(void)
{
    if (!g_pending.active) return fail(IGS_RAST_E_INVALID, "igs_rast_forward_finish: no asynchronous forward pending");
    g_pending.active = false;
    uint32_t overflow = 0;
    const int R = collect_status(g_status_stream, &overflow);
    if (R < 0) return R;
    if (overflow) {
        g_hint.slab = slab_hint_for(overflow);       // igs_rast_forward falls back further if needed
        return fail(IGS_RAST_E_RETRY, "a tile overflowed its instance slab: redo the frame");
    }
    if (g_prof.on) g_prof.r_sum += (double)R;
    return R;
}

// Forward for stream capture (hipGraph): identical launches, NO host-side wait, no pending latch -- nothing in it is illegal
// while the stream is capturing (the pinned status slot must exist already: run one ordinary forward on this thread and device
// first).  Every replay of the captured launches posts its {R, overflow, prefilter flag} into the slot;
// igs_rast_last_status() reads it back once the caller has synchronised the stream.
extern "C" int igs_rast_forward_nowait(FWD_PARAMS) { return forward_entry(FwdMode::Capture, FWD_IN); }
// What the last slab-binned forward of this thread and device posted.  *overflow != 0: a tile needed that many instance slots and
// the per-tile slabs were smaller -- the frame (and everything computed from it) is invalid; the slab hint has been raised, so a
// new capture / an ordinary igs_rast_forward will fit.  Only meaningful once the stream has been synchronised.
static int last_status(int* num_rendered, unsigned* overflow, unsigned* prefilter_flag, bool check_seq)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= IGS_MAX_DEVICES || !g_slots.slot[dev].pinned)
        return fail(IGS_RAST_E_INVALID, "igs_rast_last_status: no forward has run on this thread and device");
    const uint32_t* p = g_slots.slot[dev].pinned;
    // the sequence word is stored last by the kernel (release): if it is not the number baked into the last igs_rast_forward_nowait of this
    // thread (the last capture), no replay of that capture has posted yet and the other three words still belong to an EARLIER (eager) frame
    const uint32_t seq = __atomic_load_n(&p[3], __ATOMIC_ACQUIRE);
    if (check_seq && seq != (g_nowait_seq ? g_nowait_seq : g_host_seq))
        return fail(IGS_RAST_E_RETRY, "igs_rast_last_status: the captured forward has not posted its status yet (replay the graph and synchronise the stream first)");
    const FrameStatus st = read_status(p);
    if (num_rendered) *num_rendered = st.R > 0x7FFFFFFFu ? 0x7FFFFFFF : (int)st.R;
    if (overflow) *overflow = st.overflow;
    if (prefilter_flag) *prefilter_flag = st.prefilter;
    if (st.overflow && slab_hint_for(st.overflow) > g_hint.slab) g_hint.slab = slab_hint_for(st.overflow);      // (only ever grows it)
    return 0;
}
extern "C" int igs_rast_last_status(int* num_rendered, unsigned* overflow, unsigned* prefilter) { return last_status(num_rendered, overflow, prefilter, true); }
extern "C" int igs_rast_last_posted_status(int* num_rendered, unsigned* overflow, unsigned* prefilter) { return last_status(num_rendered, overflow, prefilter, false); }

// ---------------------------------------------------------------------------------------------------------------------
// V views of one Gaussian set (the view loop of GS3DRenderer.forward_single_batch, igs/models/gs.py:839-847, each pass of which is
// one RasterizeGaussiansCUDA, rasterize_points.cu:35-133): all V slab-binned pipelines are enqueued, view v posting into status
// slot 1 + v, before the host looks at the first status -- one host wait per call.  A view whose slabs overflowed is redone alone
// through forward_impl (slot 0) once every status is in and the slab hint has been raised to fit the largest of them.
// ---------------------------------------------------------------------------------------------------------------------
extern "C" int igs_rast_views_max(void) { return IGS_VIEWS_MAX; }

// view v's FwdIn: the shared arguments, camera v, scratch set v and slice v of every output
static FwdIn view_fwd_in(const FwdIn& in, int v, void* const* geometry_user, void* const* binning_user, void* const* image_user)
{
    FwdIn f = in;
    const size_t HW = (size_t)in.width * in.height;
    f.geometry_user = geometry_user[v]; f.binning_user = binning_user[v]; f.image_user = image_user[v];
    f.viewmatrix = in.viewmatrix + 16 * v; f.projmatrix = in.projmatrix + 16 * v; f.cam_pos = in.cam_pos + 3 * v;
    f.out_color = in.out_color + 3 * HW * v; f.out_coord = in.out_coord + 3 * HW * v; f.out_mcoord = in.out_mcoord + 3 * HW * v;
    f.out_depth = in.out_depth + HW * v; f.out_mdepth = in.out_mdepth + HW * v; f.out_alpha = in.out_alpha + HW * v;
    f.out_normal = in.out_normal + 3 * HW * v; f.radii = in.radii + (size_t)in.P * v;
    return f;
}

extern "C" int igs_rast_forward_views(
    void* stream, int V, igs_rast_alloc_fn geometry_buffer, void* const* geometry_user, igs_rast_alloc_fn binning_buffer, void* const* binning_user,
    igs_rast_alloc_fn image_buffer, void* const* image_user, int P, int D, int M, const float* background, int width, int height,
    const float* means3D, const float* shs, const float* colors_precomp, const float* opacities, const float* scales,
    float scale_modifier, const float* rotations, const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
    const float* cam_pos, float tan_fovx, float tan_fovy, float kernel_size, int prefiltered, float* out_color, float* out_coord,
    float* out_mcoord, float* out_depth, float* out_mdepth, float* out_alpha, float* out_normal, int* radii, int* num_rendered,
    int require_coord, int require_depth, int debug)
{
    const char* fn = "igs_rast_forward_views";
    if (V < 1 || V > IGS_VIEWS_MAX) return fail_in(fn, "V must be 1 .. igs_rast_views_max()");
    if (P < 0 || width <= 0 || height <= 0) return fail_in(fn, "bad sizes");
    if (!num_rendered) return fail_in(fn, "NULL num_rendered");
    for (int v = 0; v < V; v++) num_rendered[v] = 0;
    if (P == 0) return 0;
    if (!viewmatrix || !projmatrix || !cam_pos) return fail_in(fn, "NULL camera array");
    if (!geometry_buffer || !binning_buffer || !image_buffer || !geometry_user || !binning_user || !image_user)
        return fail_in(fn, "NULL scratch callback or per-view user array");
    if (!out_color || !out_coord || !out_mcoord || !out_depth || !out_mdepth || !out_alpha || !out_normal || !radii) return fail_in(fn, "NULL output");
    if (M > 16) return fail_in(fn, "more than 16 SH coefficients per channel are not supported");
    if (g_pending.active) return fail_in(fn, "an asynchronous forward is pending on this thread; call igs_rast_forward_finish() first");
    const hipStream_t s = (hipStream_t)stream;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
        return fail_in(fn, "the stream is capturing: capture of the multi-view forward is not supported (capture single views with igs_rast_forward_nowait)");
    const FwdIn in{ s, geometry_buffer, nullptr, binning_buffer, nullptr, image_buffer, nullptr, P, D, M, background, width, height, means3D,
                    shs, colors_precomp, opacities, scales, scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix, cam_pos, tan_fovx,
                    tan_fovy, kernel_size, prefiltered, out_color, out_coord, out_mcoord, out_depth, out_mdepth, out_alpha, out_normal, radii,
                    require_coord, require_depth, debug };
    const bool hint_clean = g_hint_clean; g_hint_clean = false;      // (igs_rast_hint_scratch_clean: here a promise about all V image buffers)
    FwdIn vin[IGS_VIEWS_MAX];
    for (int v = 0; v < V; v++) vin[v] = view_fwd_in(in, v, geometry_user, binning_user, image_user);
    const uint64_t slab = g_hint.slab ? g_hint.slab : 1024;
    const uint64_t Tn = (uint64_t)((width + TILE - 1) / TILE) * ((height + TILE - 1) / TILE);
    if (radix_forced() || Tn * slab > 0x7FFFFFFFull || Tn * slab * 12 > SLAB_MAX_BYTES) {
        // the global sort reads its instance count back in the middle of every frame: one view after the other
        for (int v = 0; v < V; v++) {
            prof_new_frame();
            const int R = forward_impl(vin[v], FwdExtra(), radix_forced());
            if (R < 0) return R;
            num_rendered[v] = R;
        }
        return 0;
    }
    // forward_impl's argument checks on view 0 (the views differ in pointers offset from the same bases), without launching anything
    if (!means3D || !opacities || !background) return fail_in(fn, "NULL required input");
    if (!colors_precomp && !shs) return fail_in(fn, "neither shs nor colors_precomp");
    if (!cov3D_precomp && (!scales || !rotations)) return fail_in(fn, "neither scales/rotations nor cov3D_precomp");
    if (!colors_precomp && (M < (D + 1) * (D + 1) || D < 0 || D > 3)) return fail_in(fn, "SH degree / coefficient count mismatch");
    if (int rc = ensure_view_slots()) return rc;
    uint32_t seq[IGS_VIEWS_MAX];
    for (int v = 0; v < V; v++) {
        prof_new_frame();
        FwdExtra ex; ex.status_slot = 1 + v; ex.scratch_clean = hint_clean;
        Frame f(vin[v], ex);
        if (int rc = carve_frame(f)) return rc;
        Binned b;
        if (int rc = bin_slab(f, (uint32_t)slab, b)) return rc;
        if (int rc = launch_blend(f, b)) return rc;
        seq[v] = g_host_seq;
    }
    uint32_t overflow[IGS_VIEWS_MAX], worst = 0;
    for (int v = 0; v < V; v++) {
        const int R = collect_status(s, &overflow[v], 1 + v, seq[v]);
        if (R < 0) return R;
        num_rendered[v] = R;
        if (overflow[v] > worst) worst = overflow[v];
        if (g_prof.on && !overflow[v]) { g_prof.r_sum += (double)R; g_prof.calls++; }
    }
    if (!worst) return 0;
    g_hint.slab = slab_hint_for(worst);              // raised once, to what the densest tile of any view needs
    for (int v = 0; v < V; v++) {
        if (!overflow[v]) continue;
        const int R = forward_impl(vin[v], FwdExtra(), false);
        if (R < 0) return R;
        num_rendered[v] = R;
    }
    return 0;
}

extern "C" void igs_rast_set_slab_hint(unsigned slots_per_tile) { g_hint.slab = slots_per_tile > TILE_SORT_BIG ? TILE_SORT_BIG : slots_per_tile; }
extern "C" unsigned igs_rast_get_slab_hint(void) { return g_hint.slab; }

// which blend_bwd_kernel<COORD, DEPTH, NORMAL, ABS> the last backward of this PROCESS launched (not per thread: PyTorch runs
// autograd backward functions on its own worker thread): bit 0 coord, 1 depth, 2 normal, 3 abs-gradient moment; -1 = none
// (R == 0 / no backward yet).  Tests use it to prove that absent upstream gradients select the cheaper instance.
static int g_last_bwd_instance = -1;
extern "C" int igs_rast_last_backward_instance(void) { return __atomic_load_n(&g_last_bwd_instance, __ATOMIC_RELAXED); }

// NaN report of the per-Gaussian backward kernel (replaces the reference's seven `assert not torch.isnan(g).any()` host syncs,
// DGR/diff_gaussian_rasterization_rade/__init__.py:156-162): a thread that writes a NaN stores the report's sequence number into a word
// of pinned host memory; an event recorded behind the kernel tells the host when the word is final.  One TICKET per report, a ring of
// NAN_RING per host thread and device (two renders in one backward pass, ...): memory and events are never freed -- the thread that
// runs autograd backward functions may outlive the HIP runtime.
#define NAN_RING 256
struct NanTicket { volatile uint32_t* word = nullptr; hipEvent_t ev = nullptr; uint32_t seq = 0; };
struct NanSlot { uint32_t* pinned = nullptr; uint32_t* pinned_dev = nullptr; NanTicket* tickets = nullptr; uint32_t seq = 0; bool requested = false; bool pending = false; };
static thread_local NanSlot g_nan[IGS_MAX_DEVICES];
static thread_local int g_nan_dev = -1;          // device of the last backward that was asked for a report
static thread_local float g_next_clamp = 0.f;     // one-shot: clamp of the NEXT igs_rast_backward of this thread (clamp package)
extern "C" void igs_rast_next_backward_options(int nan_report, float clamp_grads)
{
    g_next_clamp = clamp_grads > 0.f ? clamp_grads : 0.f;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= IGS_MAX_DEVICES) return;
    g_nan[dev].requested = nan_report != 0;
}
// the NaN report asked for this backward, if any (one-shot: the request is consumed here, even if the call fails later)
static int take_nan_request(NanSlot** slot)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= IGS_MAX_DEVICES || !g_nan[dev].requested) return 0;
    NanSlot& n = g_nan[dev]; n.requested = false;
    if (!n.pinned) {
        HIP_TRY(hipHostMalloc((void**)&n.pinned, NAN_RING * 4, hipHostMallocDefault), "hipHostMalloc");
        HIP_TRY(hipHostGetDevicePointer((void**)&n.pinned_dev, n.pinned, 0), "hipHostGetDevicePointer");
        memset(n.pinned, 0, NAN_RING * 4);
        n.tickets = new NanTicket[NAN_RING];
    }
    *slot = &n; g_nan_dev = dev;
    return 0;
}
// the next ticket of `n` for the per-Gaussian kernel about to be launched with `ga`
static int next_nan_ticket(NanSlot& n, GeomBwdArgs& ga, NanTicket** ticket)
{
    n.seq = n.seq + 1 ? n.seq + 1 : 1;
    NanTicket* t = &n.tickets[n.seq % NAN_RING];
    if (!t->ev) HIP_TRY(hipEventCreateWithFlags(&t->ev, hipEventDisableTiming), "hipEventCreate");
    t->word = n.pinned + (n.seq % NAN_RING); t->seq = n.seq;
    ga.nan_host = n.pinned_dev + (n.seq % NAN_RING); ga.nan_seq = n.seq;
    *ticket = t; return 0;
}
static int nan_wait_ticket(const NanTicket* t, uint32_t seq)
{
    if (!t || !t->ev) return fail(IGS_RAST_E_INVALID, "NaN report: bad ticket");
    double t0 = 0.0;
    for (long spins = 0;; spins++) {
        if (t->seq != seq) return fail(IGS_RAST_E_INVALID, "the NaN report was overwritten by a later one before it was read");
        const hipError_t q = hipEventQuery(t->ev);
        if (q == hipSuccess) return (__atomic_load_n(t->word, __ATOMIC_ACQUIRE) == seq) ? 1 : 0;
        if (q != hipErrorNotReady) return fail(IGS_RAST_E_HIP, "error while waiting for the NaN report", q);
        if ((spins & 0xFF) == 0xFF) {
            const double now = now_s();
            if (t0 == 0.0) t0 = now;
            else if (now - t0 > wait_limit_s()) return fail(IGS_RAST_E_HIP, "timed out waiting for the NaN report (IGS_RAST_WAIT_TIMEOUT_S)");
        }
    }
}
extern "C" int igs_rast_nan_report_wait(void)
{
    if (g_nan_dev < 0 || !g_nan[g_nan_dev].pending) return fail(IGS_RAST_E_INVALID, "igs_rast_nan_report_wait: no backward with a NaN report pending on this thread");
    NanSlot& n = g_nan[g_nan_dev];
    n.pending = false;
    return nan_wait_ticket(&n.tickets[n.seq % NAN_RING], n.seq);
}
extern "C" int igs_rast_nan_report_handle(const void** ticket, unsigned* seq)
{
    if (g_nan_dev < 0 || !g_nan[g_nan_dev].pending || !ticket || !seq) return fail(IGS_RAST_E_INVALID, "igs_rast_nan_report_handle: no backward with a NaN report pending on this thread");
    NanSlot& n = g_nan[g_nan_dev];
    n.pending = false;
    *ticket = &n.tickets[n.seq % NAN_RING]; *seq = n.seq;
    return 0;
}
extern "C" int igs_rast_nan_report_wait_at(const void* ticket, unsigned seq)
{
    if (!ticket) return fail(IGS_RAST_E_INVALID, "igs_rast_nan_report_wait_at: NULL handle");
    return nan_wait_ticket((const NanTicket*)ticket, seq);
}

// the reference's backward argument list (CudaRasterizer::Rasterizer::backward), in the order of igs_rast_backward's parameters
struct BwdIn {
    hipStream_t s; int P, D, M, R; const float* background; int width, height;
    const float *means3D, *shs, *colors_precomp, *alphas, *scales; float scale_modifier; const float *rotations, *cov3D_precomp;
    const float *viewmatrix, *projmatrix, *campos; float tan_fovx, tan_fovy, kernel_size; const int* radii; const float* normalmap;
    const char *geom_buffer, *binning_buffer, *image_buffer;
    const float *dL_dpix, *dL_dpix_coord, *dL_dpix_mcoord, *dL_dpix_depth, *dL_dpix_mdepth, *dL_dalphas, *dL_dpixel_normals; void* workspace;
    float *dL_dmean2D, *dL_dcolor, *dL_dopacity, *dL_dmean3D, *dL_dcov3D, *dL_dsh, *dL_dscale, *dL_drot; int require_coord, require_depth, debug;
};
// what igs_refine_step fuses into the backward: the activation backward + Adam into the per-Gaussian kernel (no gradient outputs except
// the optional dL_dmean2D), and with l1_gt != NULL the L1 loss into the blend backward (dL_dpix ignored)
struct BwdFused { const RefineFuse& adam; const float* l1_gt; const float* l1_color; float l1_scale; };

static int backward_impl(const BwdIn& in, const BwdFused* fz)
{
    const hipStream_t s = in.s; const int debug = in.debug; const int P = in.P;
    const RefineFuse* fuse = fz ? &fz->adam : nullptr;
    if (P < 0 || in.R < 0 || in.width <= 0 || in.height <= 0) return fail(IGS_RAST_E_INVALID, "igs_rast_backward: bad sizes");
    if (P == 0) return 0;                                       // rasterize_points.cu:195
    if (!in.geom_buffer || !in.image_buffer || (!in.binning_buffer && in.R > 0) || !in.workspace)
        return fail(IGS_RAST_E_INVALID, "igs_rast_backward: NULL scratch buffer");
    if (!in.means3D || !in.alphas || !in.viewmatrix || !in.projmatrix || !in.campos || !in.background || !in.radii || !in.normalmap)
        return fail(IGS_RAST_E_INVALID, "igs_rast_backward: NULL required input");
    // any of the seven upstream gradients may be NULL = "all zeros" (an output that did not take part in the loss)
    if (!fuse && (!in.dL_dmean2D || !in.dL_dcolor || !in.dL_dopacity || !in.dL_dmean3D || !in.dL_dcov3D || !in.dL_dscale || !in.dL_drot
                  || (in.M > 0 && !in.dL_dsh)))
        return fail(IGS_RAST_E_INVALID, "igs_rast_backward: NULL output");

    if ((uint64_t)P * GACC_F * 8 >= (1ull << 32))      // (the blend backward addresses its accumulator rows with 32-bit byte offsets)
        return fail(IGS_RAST_E_INVALID, "igs_rast_backward: more than 16 million Gaussians are not supported");
    const int gx = (in.width + TILE - 1) / TILE, gy = (in.height + TILE - 1) / TILE;
    const size_t Tn = (size_t)gx * gy, HW = (size_t)in.width * in.height;
    const GeomLayout GL(P);
    const ImgLayout IL(HW, Tn);
    const BinLayout BL(in.R);
    const char* gbase = align_ptr(in.geom_buffer);
    const char* ibase = align_ptr(in.image_buffer);
    const char* bbase = in.binning_buffer ? align_ptr(in.binning_buffer) : nullptr;
    double* gacc = (double*)align_ptr((const char*)in.workspace);
    const float fy = in.height / (2.0f * in.tan_fovy), fx = in.width / (2.0f * in.tan_fovx);

    const float clamp_next = g_next_clamp; g_next_clamp = 0.f;       // (one-shot, consumed here even if the call fails later)
    NanSlot* nan = nullptr;
    if (!fuse) { if (int rc = take_nan_request(&nan)) return rc; }
    prof_mark(s, ST_GAP);
    float* loss_shards = (float*)((char*)gacc + ws_gacc_bytes(P));
    // which blend instance will run (launch_blend_bwd decides the same way): the colour-only one packs its moments into 64-byte rows
    const bool will_compact = !(in.require_coord && (in.dL_dpix_coord || in.dL_dpix_mcoord)) && !(in.require_depth && (in.dL_dpix_depth || in.dL_dpix_mdepth))
                              && !((in.require_coord || in.require_depth) && in.dL_dpixel_normals);
    if (!(fuse && fuse->prezeroed)) {              // (igs_refine_step: the forward's preprocess kernel zero-filled the accumulators)
        HIP_TRY(zero_fill_async(s, gacc, (size_t)P * (will_compact ? GACC_COMPACT_F : GACC_F) * 8), "zero gacc");
        if (fz && fz->l1_gt) HIP_TRY(zero_fill_async(s, loss_shards, WS_LOSS_BYTES), "zero loss shards");
    }
    prof_mark(s, ST_MEMSET);
    BlendBwdArgs ba;
    ba.W = in.width; ba.H = in.height; ba.gx = gx; ba.gy = gy; ba.fx = fx; ba.fy = fy; ba.bg = in.background;
    ba.ranges = (const uint32_t*)(ibase + IL.ranges);
    ba.point_list = bbase ? (const uint32_t*)(bbase + BL.point_list) : nullptr;
    ba.rec = (const float*)(gbase + GL.rec); ba.colors_precomp = in.colors_precomp;
    ba.alphas = in.alphas; ba.normalmap = in.normalmap;
    ba.accum_coord = (const float*)(ibase + IL.accum_coord); ba.accum_depth = (const float*)(ibase + IL.accum_depth);
    ba.normal_length = (const float*)(ibase + IL.normal_length); ba.n_contrib = (const uint32_t*)(ibase + IL.n_contrib);
    ba.dL_dpix = in.dL_dpix; ba.dL_dcoord = in.dL_dpix_coord; ba.dL_dmcoord = in.dL_dpix_mcoord; ba.dL_ddepth = in.dL_dpix_depth;
    ba.dL_dmdepth = in.dL_dpix_mdepth; ba.dL_dalpha = in.dL_dalphas; ba.dL_dnormal = in.dL_dpixel_normals;
    ba.gacc = gacc;
    ba.l1_gt = fz ? fz->l1_gt : nullptr; ba.l1_color = fz ? fz->l1_color : nullptr; ba.l1_scale = fz ? fz->l1_scale : 0.f; ba.l1_loss = loss_shards;
    ba.want_absgrad = (fuse && !in.dL_dmean2D) ? 0 : 1;
    ba.tile_order = (const uint32_t*)(ibase + IL.tile_order);    // the forward's blend kernel ordered the tiles heaviest-first
    ba.first_trainable = fuse ? fuse->first : 0;                 // (masked refine step: frozen splats form no moments)
    bool gacc_compact = will_compact;
    int inst_bits = -1;
    if (fuse && fuse->blend_done) {
        // the blend backward ran inside the forward's tile kernel (blend_step.hip): colour-only moments in compact rows
        if (!will_compact) return fail(IGS_RAST_E_INVALID, "internal: fused tile kernel with a non-compact accumulator layout");
        prof_mark(s, ST_BLEND_BWD);
    } else if (in.R > 0) {
        HIP_TRY(launch_blend_bwd(s, ba, in.require_coord != 0, in.require_depth != 0, &gacc_compact, &inst_bits), "blend_bwd launch");
        if (gacc_compact != will_compact) return fail(IGS_RAST_E_INVALID, "internal: accumulator layout mismatch");
        __atomic_store_n(&g_last_bwd_instance, inst_bits, __ATOMIC_RELAXED);
        DBG_SYNC("blend_bwd");
        prof_mark(s, ST_BLEND_BWD);
    } else __atomic_store_n(&g_last_bwd_instance, -1, __ATOMIC_RELAXED);
    GeomBwdArgs ga;
    ga.P = P; ga.D = in.D; ga.M = in.shs ? in.M : 0; ga.W = in.width; ga.H = in.height;
    ga.means3D = in.means3D; ga.shs = in.shs; ga.scales = in.scales; ga.rotations = in.rotations; ga.cov3D_precomp = in.cov3D_precomp;
    ga.radii = in.radii; ga.scale_modifier = in.scale_modifier; ga.tan_fovx = in.tan_fovx; ga.tan_fovy = in.tan_fovy;
    ga.fx = fx; ga.fy = fy; ga.kernel_size = in.kernel_size;
    ga.view = in.viewmatrix; ga.proj = in.projmatrix; ga.campos = in.campos;
    ga.rec = ba.rec; ga.gacc = gacc; ga.gacc_compact = gacc_compact ? 1 : 0;
    if (fuse && fuse->plane_tag) { ga.plane_cache = (const float*)(gbase + GL.planes); ga.plane_tag = fuse->plane_tag; }
    ga.dL_dmean2D = in.dL_dmean2D; ga.dL_dcolor = in.dL_dcolor; ga.dL_dopacity = in.dL_dopacity; ga.dL_dmean3D = in.dL_dmean3D;
    ga.dL_dcov3D = in.dL_dcov3D; ga.dL_dsh = in.dL_dsh; ga.dL_dscale = in.dL_dscale; ga.dL_drot = in.dL_drot;
    if (fuse) {
        RefineFuse f = *fuse;
        if (!f.loss_shards) f.loss_shards = loss_shards;
        if (f.color_event && f.color_out && f.grad_out) {
            // N > 1: this view's colour gradients leave one kernel early, the all-gather runs underneath the per-Gaussian kernel
            HIP_TRY(launch_extract_view_colors(s, P, in.radii, ba.rec, gacc, gacc_compact ? 1 : 0, in.shs != nullptr && in.M > 0, f.color_out),
                    "extract_view_colors launch");
            HIP_TRY(hipEventRecord((hipEvent_t)f.color_event, s), "record colour event");
            f.color_out = nullptr; f.colors_extracted = 1;
        }
        HIP_TRY(launch_geom_bwd_adam(s, ga, f), "geom_bwd_adam launch");
    } else {
        ga.clamp = clamp_next;
        NanTicket* ticket = nullptr;
        if (nan) { if (int rc = next_nan_ticket(*nan, ga, &ticket)) return rc; }
        HIP_TRY(launch_geom_bwd(s, ga), "geom_bwd launch");
        if (ticket) { HIP_TRY(hipEventRecord(ticket->ev, s), "record NaN-report event"); nan->pending = true; }
    }
    DBG_SYNC("geom_bwd");
    prof_mark(s, ST_GEOM_BWD);
    return 0;
}

extern "C" int igs_rast_backward(
    void* stream, int P, int D, int M, int R, const float* background, int width, int height,
    const float* means3D, const float* shs, const float* colors_precomp, const float* alphas,
    const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
    const float* viewmatrix, const float* projmatrix, const float* campos,
    float tan_fovx, float tan_fovy, float kernel_size, const int* radii, const float* normalmap,
    const char* geom_buffer, const char* binning_buffer, const char* image_buffer,
    const float* dL_dpix, const float* dL_dpix_coord, const float* dL_dpix_mcoord, const float* dL_dpix_depth,
    const float* dL_dpix_mdepth, const float* dL_dalphas, const float* dL_dpixel_normals,
    void* workspace,
    float* dL_dmean2D, float* dL_dcolor, float* dL_dopacity, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh,
    float* dL_dscale, float* dL_drot, int require_coord, int require_depth, int debug)
{
    const BwdIn in{ (hipStream_t)stream, P, D, M, R, background, width, height, means3D, shs, colors_precomp, alphas, scales, scale_modifier,
                    rotations, cov3D_precomp, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, kernel_size, radii, normalmap, geom_buffer,
                    binning_buffer, image_buffer, dL_dpix, dL_dpix_coord, dL_dpix_mcoord, dL_dpix_depth, dL_dpix_mdepth, dL_dalphas,
                    dL_dpixel_normals, workspace, dL_dmean2D, dL_dcolor, dL_dopacity, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale, dL_drot,
                    require_coord, require_depth, debug };
    return backward_impl(in, nullptr);
}

// The backward of igs_rast_forward_views (V times RasterizeGaussiansBackwardCUDA, rasterize_points.cu:135-246, and the AccumulateGrad
// adds of gs.py:839-847's loop): every view's blend backward into its own accumulator rows, then ONE per-Gaussian kernel that sums
// over the views (geom_bwd.hip: geom_bwd_views_kernel).  Nothing between the launches involves the host.
extern "C" int igs_rast_backward_views(
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
    float* dL_dscale, float* dL_drot, int require_coord, int require_depth, int debug)
{
    const char* fn = "igs_rast_backward_views";
    const hipStream_t s = (hipStream_t)stream;
    if (V < 1 || V > IGS_VIEWS_MAX) return fail_in(fn, "V must be 1 .. igs_rast_views_max()");
    if (P < 0 || width <= 0 || height <= 0) return fail_in(fn, "bad sizes");
    if (P == 0) return 0;
    if (!viewmatrix || !projmatrix || !campos) return fail_in(fn, "NULL camera array");
    if (!R || !geom_buffer || !binning_buffer || !image_buffer || !workspace) return fail_in(fn, "NULL per-view scratch");
    for (int v = 0; v < V; v++) {
        if (R[v] < 0) return fail_in(fn, "negative instance count");
        if (!geom_buffer[v] || !image_buffer[v] || (!binning_buffer[v] && R[v] > 0)) return fail_in(fn, "NULL per-view scratch");
    }
    if (!means3D || !alphas || !background || !radii || !normalmap) return fail_in(fn, "NULL required input");
    if (!dL_dcolor || !dL_dopacity || !dL_dmean3D || !dL_dcov3D || !dL_dscale || !dL_drot || (shs && M > 0 && !dL_dsh)) return fail_in(fn, "NULL output");
    if (M > 16) return fail_in(fn, "more than 16 SH coefficients per channel are not supported");
    if ((uint64_t)P * GACC_F * 8 >= (1ull << 32)) return fail_in(fn, "more than 16 million Gaussians are not supported");
    const int gx = (width + TILE - 1) / TILE, gy = (height + TILE - 1) / TILE;
    const size_t Tn = (size_t)gx * gy, HW = (size_t)width * height;
    const GeomLayout GL(P);
    const ImgLayout IL(HW, Tn);
    const float fy = height / (2.0f * tan_fovy), fx = width / (2.0f * tan_fovx);
    const size_t ws_view = igs_rast_backward_workspace_bytes(P);

    const float clamp_next = g_next_clamp; g_next_clamp = 0.f;       // (one-shot, consumed here even if the call fails later)
    NanSlot* nan = nullptr;
    if (int rc = take_nan_request(&nan)) return rc;
    // one layout for the call, as backward_impl picks it for a view: an upstream gradient is present for all views or for none
    const bool will_compact = !(require_coord && (dL_dpix_coord || dL_dpix_mcoord)) && !(require_depth && (dL_dpix_depth || dL_dpix_mdepth))
                              && !((require_coord || require_depth) && dL_dpixel_normals);
    GeomBwdViews w;
    w.V = V; w.views = viewmatrix; w.projs = projmatrix; w.campos = campos; w.radii = radii; w.dL_dmean2D = dL_dmean2D;
    int inst_last = -1;
    prof_mark(s, ST_GAP);
    for (int v = 0; v < V; v++) {
        const char* gbase = align_ptr(geom_buffer[v]);
        const char* ibase = align_ptr(image_buffer[v]);
        const char* bbase = binning_buffer[v] ? align_ptr(binning_buffer[v]) : nullptr;
        double* gacc = (double*)align_ptr((const char*)workspace + ws_view * v);
        HIP_TRY(zero_fill_async(s, gacc, (size_t)P * (will_compact ? GACC_COMPACT_F : GACC_F) * 8), "zero gacc");
        auto img = [&](const float* p, size_t c) { return p ? p + c * HW * v : nullptr; };
        BlendBwdArgs ba;
        ba.W = width; ba.H = height; ba.gx = gx; ba.gy = gy; ba.fx = fx; ba.fy = fy; ba.bg = background;
        ba.ranges = (const uint32_t*)(ibase + IL.ranges);
        ba.point_list = bbase ? (const uint32_t*)(bbase + BinLayout(R[v]).point_list) : nullptr;
        ba.rec = (const float*)(gbase + GL.rec); ba.colors_precomp = colors_precomp;
        ba.alphas = alphas + HW * v; ba.normalmap = normalmap + 3 * HW * v;
        ba.accum_coord = (const float*)(ibase + IL.accum_coord); ba.accum_depth = (const float*)(ibase + IL.accum_depth);
        ba.normal_length = (const float*)(ibase + IL.normal_length); ba.n_contrib = (const uint32_t*)(ibase + IL.n_contrib);
        ba.dL_dpix = img(dL_dpix, 3); ba.dL_dcoord = img(dL_dpix_coord, 3); ba.dL_dmcoord = img(dL_dpix_mcoord, 3); ba.dL_ddepth = img(dL_dpix_depth, 1);
        ba.dL_dmdepth = img(dL_dpix_mdepth, 1); ba.dL_dalpha = img(dL_dalphas, 1); ba.dL_dnormal = img(dL_dpixel_normals, 3);
        ba.gacc = gacc;
        ba.l1_gt = nullptr; ba.l1_color = nullptr; ba.l1_scale = 0.f; ba.l1_loss = nullptr;
        ba.want_absgrad = dL_dmean2D ? 1 : 0;
        ba.tile_order = (const uint32_t*)(ibase + IL.tile_order);
        if (R[v] > 0) {
            bool gacc_compact = will_compact;
            HIP_TRY(launch_blend_bwd(s, ba, require_coord != 0, require_depth != 0, &gacc_compact, &inst_last), "blend_bwd launch");
            if (gacc_compact != will_compact) return fail(IGS_RAST_E_INVALID, "internal: accumulator layout mismatch");
            DBG_SYNC("blend_bwd");
        }
        w.rec[v] = ba.rec; w.gacc[v] = gacc;
    }
    __atomic_store_n(&g_last_bwd_instance, inst_last, __ATOMIC_RELAXED);
    prof_mark(s, ST_BLEND_BWD);
    GeomBwdArgs ga;
    ga.P = P; ga.D = D; ga.M = shs ? M : 0; ga.W = width; ga.H = height;
    ga.means3D = means3D; ga.shs = shs; ga.scales = scales; ga.rotations = rotations; ga.cov3D_precomp = cov3D_precomp;
    ga.radii = nullptr; ga.scale_modifier = scale_modifier; ga.tan_fovx = tan_fovx; ga.tan_fovy = tan_fovy;
    ga.fx = fx; ga.fy = fy; ga.kernel_size = kernel_size;
    ga.view = nullptr; ga.proj = nullptr; ga.campos = nullptr; ga.rec = nullptr; ga.gacc = nullptr; ga.gacc_compact = will_compact ? 1 : 0;
    ga.dL_dmean2D = nullptr; ga.dL_dcolor = dL_dcolor; ga.dL_dopacity = dL_dopacity; ga.dL_dmean3D = dL_dmean3D;
    ga.dL_dcov3D = dL_dcov3D; ga.dL_dsh = dL_dsh; ga.dL_dscale = dL_dscale; ga.dL_drot = dL_drot;
    ga.clamp = clamp_next;
    NanTicket* ticket = nullptr;
    if (nan) { if (int rc = next_nan_ticket(*nan, ga, &ticket)) return rc; }
    HIP_TRY(launch_geom_bwd_views(s, ga, w), "geom_bwd_views launch");
    if (ticket) { HIP_TRY(hipEventRecord(ticket->ev, s), "record NaN-report event"); nan->pending = true; }
    DBG_SYNC("geom_bwd_views");
    prof_mark(s, ST_GEOM_BWD);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// One refine iteration on one view, single GPU (infer_batch.py:279-324 with the L1 loss): activations -> render -> L1 ->
// backward -> Adam, 6 launches, no gradient array in HBM, no host wait before the last launch is enqueued.
// ---------------------------------------------------------------------------------------------------------------------
struct ScratchCapture { igs_rast_alloc_fn fn; void* user; char* last; };
static char* capture_alloc(void* user, size_t n) { ScratchCapture* c = (ScratchCapture*)user; c->last = c->fn(c->user, n); return c->last; }

// igs_refine_step_args::loss_scratch, byte offsets: { SSIM kernels' own scratch (nine maps, then 2 x 64 shards) | dL/dcolor [3][H][W] |
// depth-normal regulariser: dL/ddepth [H][W], dL/dmdepth [H][W], dL/dnormal [3][H][W] | its 64 shards (at the next 256-byte address) }
struct LossScratchLayout {
    size_t ssim_shards, grad_img, dn_depth, dn_mdepth, dn_normal, dn_shards, total;
    LossScratchLayout(int width, int height)
    {
        const size_t HW = (size_t)(width > 0 ? width : 0) * (size_t)(height > 0 ? height : 0);
        ssim_shards = align_up(9 * HW * 4, 256);
        grad_img = align_up(igs_ssim_l1_scratch_bytes(width, height), 256);
        dn_depth = grad_img + 3 * HW * 4; dn_mdepth = dn_depth + HW * 4; dn_normal = dn_mdepth + HW * 4; dn_shards = dn_normal + 3 * HW * 4;
        total = dn_shards + 4096 + 512;
    }
};
extern "C" size_t igs_refine_loss_scratch_bytes(int width, int height) { return LossScratchLayout(width, height).total; }

extern "C" size_t igs_refine_step_args_size(void) { return sizeof(igs_refine_step_args); }

extern "C" size_t igs_refine_mask_args_size(void) { return sizeof(igs_refine_mask_args); }

static int refine_step_impl(const igs_refine_step_args* a, int first, unsigned frozen);

extern "C" int igs_refine_step(const igs_refine_step_args* a) { return refine_step_impl(a, 0, 0u); }

// igs_refine_step on a partitioned store (include/igs_rast.h): Gaussians [0, first_trainable) frozen, whole groups frozen by bit.
// Every check comes before any HIP call; m == NULL or {0, 0} is igs_refine_step itself.
extern "C" int igs_refine_step_masked(const igs_refine_step_args* a, const igs_refine_mask_args* m)
{
    if (!a) return fail(IGS_RAST_E_INVALID, "igs_refine_step_masked: NULL args");
    if (!m || (m->first_trainable == 0 && m->frozen_groups == 0u)) return refine_step_impl(a, 0, 0u);
    if (m->first_trainable < 0 || m->first_trainable > a->P)
        return fail(IGS_RAST_E_INVALID, "igs_refine_step_masked: first_trainable outside [0, P]");
    const unsigned known = IGS_GROUP_XYZ | IGS_GROUP_ROT | IGS_GROUP_SH | IGS_GROUP_OPACITY | IGS_GROUP_SCALE;
    if (m->frozen_groups & ~known) return fail(IGS_RAST_E_INVALID, "igs_refine_step_masked: unknown group bits");
    if (m->frozen_groups & (IGS_GROUP_XYZ | IGS_GROUP_ROT))
        return fail(IGS_RAST_E_INVALID, "igs_refine_step_masked: xyz and rotation are always trained (refine_item cannot freeze them)");
    if (a->grad_out || a->color_grad_out)
        return fail(IGS_RAST_E_INVALID, "igs_refine_step_masked: grad_out / color_grad_out (the multi-GPU exchange) cannot be combined with a mask");
    if (a->dL_dmean2D)
        return fail(IGS_RAST_E_INVALID, "igs_refine_step_masked: dL_dmean2D (densification) cannot be combined with a mask");
    return refine_step_impl(a, m->first_trainable, m->frozen_groups);
}

// what the refine step fuses into its per-Gaussian kernel: Adam with this step's bias corrections folded into the learning rates, and the
// loss read back from its shards (ssim_shards / dn_shards: the SSIM and depth-normal losses' shards, NULL = that loss is off)
static RefineFuse refine_fuse(const igs_refine_step_args* a, int first, unsigned frozen, const float* ssim_shards, const float* dn_shards)
{
    const int stepno = a->step < 1 ? 1 : a->step;
    const double bc1 = 1.0 - pow((double)a->beta1, (double)stepno), bc2 = 1.0 - pow((double)a->beta2, (double)stepno);
    RefineFuse f;
    f.param = a->param; f.exp_avg = a->exp_avg; f.exp_avg_sq = a->exp_avg_sq; f.grad_out = a->grad_out;
    f.off_xyz = a->off_xyz; f.off_rot = a->off_rot; f.off_sh = a->off_sh; f.off_opacity = a->off_opacity; f.off_scale = a->off_scale;
    f.lr_xyz = (float)(a->lr_xyz / bc1); f.lr_rot = (float)(a->lr_rot / bc1); f.lr_sh = (float)(a->lr_sh / bc1);
    f.lr_opacity = (float)(a->lr_opacity / bc1); f.lr_scale = (float)(a->lr_scale / bc1);
    f.clamp = a->clamp_grads;
    f.first = first; f.frozen_groups = frozen;
    f.color_out = a->color_grad_out;
    f.color_event = a->color_ready_event;
    f.b1 = a->beta1; f.b2 = a->beta2; f.eps = a->eps; f.inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
    const float inv_n = 1.0f / (float)(3 * (size_t)a->width * a->height);
    f.loss_out = a->loss_out; f.loss_shards2 = nullptr; f.loss_bias = 0.f; f.loss_scale2 = 0.f;
    f.loss_shards3 = dn_shards; f.loss_scale3 = 1.0f;       // (the kernel's shards already carry weight * lambda / HW)
    if (ssim_shards) {    // loss = lambda w (1 - mean ssim) + (1 - lambda) w mean|d|
        f.loss_shards = ssim_shards; f.loss_scale = -a->lambda_dssim * a->loss_weight * inv_n;
        f.loss_shards2 = ssim_shards + 1024; f.loss_scale2 = (1.f - a->lambda_dssim) * a->loss_weight * inv_n;
        f.loss_bias = a->lambda_dssim * a->loss_weight;
    } else {
        f.loss_shards = nullptr; f.loss_scale = a->loss_weight * inv_n;
    }
    return f;
}

static int refine_step_impl(const igs_refine_step_args* a, int first, unsigned frozen)
{
    if (!a) return fail(IGS_RAST_E_INVALID, "igs_refine_step: NULL args");
    if (g_pending.active) return fail(IGS_RAST_E_INVALID, "igs_refine_step: an asynchronous forward is pending on this thread; call igs_rast_forward_finish() first");
    if (a->P <= 0 || a->M <= 0 || a->width <= 0 || a->height <= 0 || (a->step < 1 && !a->grad_out))
        return fail(IGS_RAST_E_INVALID, "igs_refine_step: bad sizes");
    if (!a->param || (!a->grad_out && (!a->exp_avg || !a->exp_avg_sq)) || !a->gt || !a->out_images || !a->radii || !a->workspace || !a->background)
        return fail(IGS_RAST_E_INVALID, "igs_refine_step: NULL pointer");
    const bool dssim = a->lambda_dssim > 0.f, dn = a->lambda_depth_normal > 0.f;
    if ((dssim || dn) && !a->loss_scratch) return fail(IGS_RAST_E_INVALID, "igs_refine_step: lambda_dssim / lambda_depth_normal > 0 need loss_scratch");
    if (dn && !a->require_depth) return fail(IGS_RAST_E_INVALID, "igs_refine_step: the depth-normal regulariser needs require_depth");
    const hipStream_t s = (hipStream_t)a->stream;
    const size_t HW = (size_t)a->width * a->height;
    float* img = a->out_images;
    float *color = img, *depth = img + 9 * HW, *mdepth = img + 10 * HW, *alpha = img + 11 * HW, *normal = img + 12 * HW;
    ScratchCapture cg{ a->geometry_buffer, a->geometry_user, nullptr }, cb{ a->binning_buffer, a->binning_user, nullptr },
                   ci{ a->image_buffer, a->image_user, nullptr };
    const LossScratchLayout LS(a->width, a->height);
    char* ls = (char*)a->loss_scratch;
    float *ssim_shards = dssim ? (float*)(ls + LS.ssim_shards) : nullptr, *grad_img = dssim ? (float*)(ls + LS.grad_img) : nullptr;
    float *dn_gd = dn ? (float*)(ls + LS.dn_depth) : nullptr, *dn_gm = dn ? (float*)(ls + LS.dn_mdepth) : nullptr;
    float *dn_gn = dn ? (float*)(ls + LS.dn_normal) : nullptr, *dn_shards = dn ? (float*)align_ptr(ls + LS.dn_shards) : nullptr;
    RefineFuse f = refine_fuse(a, first, frozen, ssim_shards, dn_shards);
    const float l1_scale = a->loss_weight * (1.0f / (float)(3 * HW));
    const BwdFused fused{ f, dssim ? nullptr : a->gt, color, l1_scale };
    // depth-normal regulariser on the maps the forward renders: its three gradient maps switch the blend backward to the <depth, normal> instance
    DepthNormalJob dnj;
    dnj.fx = a->width / (2.0f * a->tan_fovx); dnj.fy = a->height / (2.0f * a->tan_fovy); dnj.depth = depth; dnj.mdepth = mdepth; dnj.normal = normal;
    dnj.weight = a->loss_weight * a->lambda_depth_normal; dnj.depth_ratio = a->depth_ratio > 0.f ? a->depth_ratio : 0.6f;
    dnj.g_depth = dn_gd; dnj.g_mdepth = dn_gm; dnj.g_normal = dn_gn; dnj.loss_shards = dn_shards;

    FwdIn in{};          // (the parameters are the raw optimiser leaves inside `param`)
    in.s = s; in.geometry_buffer = capture_alloc; in.geometry_user = &cg; in.binning_buffer = capture_alloc; in.binning_user = &cb;
    in.image_buffer = capture_alloc; in.image_user = &ci; in.P = a->P; in.D = a->D; in.M = a->M; in.background = a->background;
    in.width = a->width; in.height = a->height; in.means3D = a->param + a->off_xyz; in.shs = a->param + a->off_sh;
    in.opacities = a->param + a->off_opacity; in.scales = a->param + a->off_scale; in.scale_modifier = 1.0f; in.rotations = a->param + a->off_rot;
    in.viewmatrix = a->viewmatrix; in.projmatrix = a->projmatrix; in.cam_pos = a->cam_pos; in.tan_fovx = a->tan_fovx; in.tan_fovy = a->tan_fovy;
    in.out_color = color; in.out_coord = img + 3 * HW; in.out_mcoord = img + 6 * HW; in.out_depth = depth; in.out_mdepth = mdepth;
    in.out_alpha = alpha; in.out_normal = normal; in.radii = a->radii; in.require_coord = a->require_coord; in.require_depth = a->require_depth;
    BwdIn bw{};
    bw.s = s; bw.P = a->P; bw.D = a->D; bw.M = a->M; bw.background = a->background; bw.width = a->width; bw.height = a->height;
    bw.means3D = in.means3D; bw.shs = in.shs; bw.alphas = alpha; bw.scales = in.scales; bw.scale_modifier = 1.0f; bw.rotations = in.rotations;
    bw.viewmatrix = a->viewmatrix; bw.projmatrix = a->projmatrix; bw.campos = a->cam_pos; bw.tan_fovx = a->tan_fovx; bw.tan_fovy = a->tan_fovy;
    bw.radii = a->radii; bw.normalmap = normal; bw.dL_dpix = grad_img; bw.dL_dpix_depth = dn_gd; bw.dL_dpix_mdepth = dn_gm;
    bw.dL_dpixel_normals = dn_gn; bw.workspace = a->workspace; bw.dL_dmean2D = a->dL_dmean2D; bw.require_coord = a->require_coord;
    bw.require_depth = a->require_depth;

    prof_new_frame();
    for (int attempt = 0; attempt < 2; attempt++) {
        g_pending.active = false;
        f.prezeroed = 1;
        FwdExtra ex;
        ex.zero_gacc = (double*)align_ptr((const char*)a->workspace);
        ex.zero_loss = dssim ? ssim_shards : (float*)((char*)ex.zero_gacc + ws_gacc_bytes(a->P));
        ex.zero_loss2 = dssim ? ssim_shards + 1024 : nullptr;
        ex.zero_gacc_first = first;
        ex.defer_status = attempt == 0;            // second attempt: synchronous forward, which sorts out its scratch sizes itself
        ex.raw_activations = true;
        ex.skip_bwd_state = !dn;                   // (colour-only backward instance: see BlendFwdArgs)
        static const bool no_plane_cache = getenv("IGS_NO_PLANE_CACHE") != nullptr;      // (A/B switch for measurements)
        if (dn && !no_plane_cache) {
            // the regulariser sends depth / normal gradients back: the forward keeps Sigma^-1 of every visible Gaussian, the
            // per-Gaussian backward takes it from there instead of running the eigen-solver again (geom_math.h: PlaneCache)
            static std::atomic<uint32_t> nonce{0};
            uint32_t t = ++nonce;
            if (t == 0) t = ++nonce;
            ex.plane_tag = t; f.plane_tag = t;
        } else f.plane_tag = 0;
        ex.scratch_clean = a->scratch_clean != 0;
        // L1 loss, colour-only backward: forward and backward blend of a tile in one kernel (blend_step.hip)
        BlendBwdArgs fused_bwd{};
        bool fused_ran = false;
        int fused_inst = -1;
        static const bool no_fuse = getenv("IGS_NO_TILE_FUSION") != nullptr;      // (A/B switch for measurements)
        if (!dssim && !dn && !no_fuse) {
            fused_bwd.gacc = ex.zero_gacc;
            fused_bwd.l1_gt = a->gt; fused_bwd.l1_color = color; fused_bwd.l1_scale = l1_scale;
            fused_bwd.l1_loss = (float*)((char*)ex.zero_gacc + ws_gacc_bytes(a->P));
            fused_bwd.want_absgrad = a->dL_dmean2D ? 1 : 0;
            fused_bwd.first_trainable = first;
            ex.fused_bwd = &fused_bwd; ex.fused_ran = &fused_ran; ex.fused_instance = &fused_inst;
        }
        const int R = forward_impl(in, ex, false);
        if (R < 0) return R;
        f.guard_overflow = g_last_fwd.overflow; f.guard_prefilter = g_last_fwd.prefilter;
        f.blend_done = fused_ran ? 1 : 0;
        if (fused_ran) __atomic_store_n(&g_last_bwd_instance, fused_inst, __ATOMIC_RELAXED);
        static const bool no_mix = getenv("IGS_NO_LOSS_MIX") != nullptr;      // (A/B switch for measurements)
        const bool mix = dssim && dn && !no_mix;       // both image-space losses: the regulariser rides in the SSIM gradient's launch
        if (dssim) {
            prof_mark(s, ST_GAP);
            if (launch_ssim_l1(s, a->width, a->height, color, a->gt, a->lambda_dssim, a->loss_weight, a->loss_scratch,
                               grad_img, false, a->gt_stats, a->gt_stats_valid != 0, mix ? &dnj : nullptr) != hipSuccess)
                return fail(IGS_RAST_E_HIP, "ssim loss launch");
            prof_mark(s, ST_MEMSET);          // (the stage slot the fused step does not otherwise use: "loss")
        }
        if (dn && !mix) {
            HIP_TRY(zero_fill_async(s, dn_shards, 4096), "zero shards");
            HIP_TRY(launch_depth_normal(s, a->width, a->height, dnj.fx, dnj.fy, depth, mdepth, normal, dnj.weight, dnj.depth_ratio, dn_gd, dn_gm,
                                        dn_gn, dn_shards), "depth_normal launch");
        }
        bw.R = R; bw.geom_buffer = cg.last; bw.binning_buffer = cb.last; bw.image_buffer = ci.last;
        const int rc = backward_impl(bw, &fused);
        if (rc < 0) return rc;
        if (!g_pending.active) return R;           // synchronous forward: R is already the true count
        const int Rt = igs_rast_forward_finish();
        if (Rt != IGS_RAST_E_RETRY) return Rt;     // the true count, or an error
        // a tile overflowed its slab: the guarded update kernel has done nothing; go again with the enlarged slabs
    }
    return fail(IGS_RAST_E_INVALID, "igs_refine_step: internal retry failure");
}


extern "C" int igs_rast_mark_visible(void* stream, int P, const float* means3D, const float* viewmatrix,
                                     const float* projmatrix, uint8_t* present)
{
    (void)projmatrix;
    if (P < 0) return fail(IGS_RAST_E_INVALID, "igs_rast_mark_visible: bad size");
    if (P == 0) return 0;
    if (!means3D || !viewmatrix || !present) return fail(IGS_RAST_E_INVALID, "igs_rast_mark_visible: NULL pointer");
    HIP_TRY(launch_mark_visible((hipStream_t)stream, P, means3D, viewmatrix, present), "mark_visible launch");
    return 0;
}

extern "C" int igs_rast_debug_dump(void* stream, int P, int R, int width, int height, const char* geom_buffer,
                                   const char* binning_buffer, const char* image_buffer, float* rec32, uint32_t* tiles,
                                   uint32_t* point_list, uint32_t* ranges, uint32_t* n_contrib)
{
    hipStream_t s = (hipStream_t)stream;
    const int gx = (width + TILE - 1) / TILE, gy = (height + TILE - 1) / TILE;
    const size_t Tn = (size_t)gx * gy, HW = (size_t)width * height;
    const GeomLayout GL(P); const ImgLayout IL(HW, Tn); const BinLayout BL(R);
    if (geom_buffer && P > 0) {
        const char* g = align_ptr(geom_buffer);
        if (rec32) HIP_TRY(hipMemcpyAsync(rec32, g + GL.rec, (size_t)P * REC_F * 4, hipMemcpyDeviceToDevice, s), "dump rec");
        if (tiles) HIP_TRY(hipMemcpyAsync(tiles, g + GL.tiles, (size_t)P * 4, hipMemcpyDeviceToDevice, s), "dump tiles");
    }
    if (image_buffer) {
        const char* i = align_ptr(image_buffer);
        // per-tile lists are gathered into the reference's compact layout (identical already on the global-sort path)
        if (ranges)
            HIP_TRY(launch_compact_lists(s, (uint32_t)Tn, (const uint32_t*)(i + IL.ranges),
                                         binning_buffer ? (const uint32_t*)(align_ptr(binning_buffer) + BL.point_list) : nullptr, ranges,
                                         point_list, (uint32_t)(R > 0 ? R : 0)), "dump lists");
        if (n_contrib) HIP_TRY(hipMemcpyAsync(n_contrib, i + IL.n_contrib, HW * 8, hipMemcpyDeviceToDevice, s), "dump n_contrib");
    }
    return 0;
}

// Test hook: fills the LDS of every CU with signalling garbage (NaN bit patterns), so that a kernel which reads LDS it never wrote
// -- invisible on a fresh device, whose LDS reads as zeros -- shows up in small parity tests (round 2 found such a read only through
// the PSNR of a long run: a missing wait state left one moment of each wave's first row unwritten).
__global__ void __launch_bounds__(256) poison_lds_kernel(float* sink)
{
    extern __shared__ uint32_t lds_all[];
    for (int i = threadIdx.x; i < 16000; i += 256) lds_all[i] = 0x7FC0BEEFu + (uint32_t)i;
    __syncthreads();
    if (lds_all[(threadIdx.x * 7) % 16000] == 1u && sink) sink[0] = 1.f;      // (keeps the stores alive)
}
extern "C" int igs_rast_debug_poison_lds(void* stream)
{
    // 64000 bytes per workgroup: two workgroups per CU cover most of the 160 KB; 2048 workgroups = 8 per CU, so every CU's LDS
    // is swept several times whatever the placement
    hipLaunchKernelGGL(poison_lds_kernel, dim3(2048), dim3(256), 64000, (hipStream_t)stream, (float*)nullptr);
    return hipGetLastError() == hipSuccess ? 0 : IGS_RAST_E_HIP;
}
