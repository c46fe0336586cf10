// igs_torch_ext.cpp -- the compiled `_C` module of the drop-in packages: torch glue over the C ABI of include/igs_rast.h.  Tensor checks,
// output allocation, pointer extraction, PyTorch's CURRENT stream -- no arithmetic.  Built by igs_amd/build_ext.py with the host compiler
// (no device code in this file, ONE translation unit: every TU pays for torch/extension.h); links libigs_rast.so.
//
// Sections, in file order, and the kernels behind them:
//   shared                                      errors and check(), tensor checks, GpuCall, ptr_or_null / HeadView
//   rasterizer          api.hip                 ScratchSet, In; rasterize_gaussians, rasterize_gaussians_backward[_ex], mark_visible: the
//                                               four functions of the reference's pybind module (DGR/ext.cpp:15-20, DGR/rasterize_points.cu:
//                                               35-267; DGR = submodules/RaDe-GS/submodules/diff-gaussian-rasterization); count_gaussians of
//                                               the compress package (compress-diff-gaussian-rasterization rasterize_points.cu:130-217)
//   multi-view          api.hip, geom_bwd.hip   ViewsCall; _views.rasterize_views, _views.rasterize_views_backward: V cameras on one Gaussian set, one C call each
//   simple_knn          knn.hip                 distCUDA2
//   anchor graph        anchors.hip             anchors_bbox_select, anchors_fps, anchors_knn (fixed output shapes, no host synchronisation)
//   interpolation       motion.hip              motion_interp_fwd / _index / _bwd
//   lifting             lift.hip                motion_lift_fwd / _bwd
//   condition3D         cond.hip                cond_ray_fwd, modln_fwd / _bwd
//                       cond_fused.hip          _cond.condition3d_fwd, _cond.pack_elems: the forward in one launch, ModLN's MLP included
//                       cond_fused_bwd.hip      _cond.condition3d_bwd, _cond.bwd_scratch_bytes: its backward, the forward recomputed
//   upsample + conv     upconv.hip              _upconv.upconv_fwd, _upconv.pack_elems: 2x bilinear upsample and 3x3 convolution in one launch
//                       upconv_bwd.hip          _upconv.upconv_bwd: its backward, d x / d weight / d bias from x and d out
//   attention           attn.hip                attn_fwd / _bwd on [B, H, A, 64] views of any acceptable strides
//   window attention    wattn.hip               _window.window_attn_fwd / _bwd on [B, h w, 128] views of any acceptable strides
//   encoder norms       inorm.hip               _encoder.instance_norm_fwd, _encoder.position_add on contiguous [N, C, H, W] tensors
//   token ops           tokens.hip              _tokens.layer_norm_fwd / _bwd, _tokens.geglu_fwd / _bwd on [N, C] rows with a row stride
//   transformer ends    gnorm.hip               _gnorm.group_norm_tokens_fwd / _bwd, _gnorm.tokens_add_residual: [B, C, A] in, [B, A, C] out
//   residual decoder    mlp.hip                 _mlp.mlp_heads_fwd, _mlp.pack_elems: [N, C0] rows with a row stride in, one [N, ch] per head out;
//                                               _mlp.mlp_heads_bwd, _mlp.bwd_scratch_bytes: d x and flat float32 d w / d b from x alone
//   layer tail          ffn.hip                 _ffn.layer_tail_fwd, _ffn.layer_tail_bwd, _ffn.pack_elems, _ffn.bwd_scratch_bytes: merge, LayerNorms and FFN of a unimatch TransformerLayer on [T, 128] rows
//   projections         proj.hip                _proj.token_proj_fwd, _proj.pack_elems: up to five 128 -> 128 projections of [T, 128] rows side by side in one [T, 128 n] buffer;
//                       proj_bwd.hip            _proj.token_proj_bwd, _proj.bwd_scratch_bytes: d x and the float32 d W_j from each output's own gradient rows
//   deform             motion.hip              motion_deform_fwd / _bwd
//   Adam                refine_ops.hip          adam_step_multi
//   losses              refine_ops, loss_ops    l1_mean; ssim_mean
//   training loss       ssim_batch.hip          _loss.ssim_batch on [N, C, H, W] float32 batches
//   module                                      names, defaults, GIL release
//
// A new op's glue follows one order: argument checks (dtype, shape, ranges) -> GpuCall on its anchor tensor ("no CPU fallback", device
// guard, stream, the other tensors on the same device) -> outputs -> contiguous inputs -> ONE C call through check().  Refusals build
// their text only when they throw; unsupported dtypes raise NotImplemented (Python: NotImplementedError), everything else RasterizerError.
//
// Extensions over the reference's signatures are keyword-only extras with defaults (the positional lists are the reference's):
//   rasterize_gaussians(..., scratch=None, out_images=None, out_radii=None, mode=0, scratch_clean=False)
//   rasterize_gaussians_backward(..., workspace=None, out_*=None)         any upstream gradient may be None (= zeros)
//   rasterize_gaussians_backward_ex(...same..., nan_report=0|1|2, clamp=0.0) -> (8 gradients, nan flag, verdict word, sequence number)
#include <torch/extension.h>
// PyTorch-ROCm presents its HIP devices under the device type "cuda" (so that `device="cuda"` callers run unchanged): guards and
// the current stream come from the classes that know about that
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <limits.h>
#include <map>
#include <mutex>

#include "../../include/igs_rast.h"

namespace {

using at::Tensor;
using OptTensor = c10::optional<Tensor>;

struct RasterizerError : public std::runtime_error { using std::runtime_error::runtime_error; };
struct NotImplemented : public std::runtime_error { using std::runtime_error::runtime_error; };      // an unsupported dtype
// the C call's return code: negative = refused or failed, with the library's text
void check(int rc, const char* what)
{
    if (rc < 0) throw RasterizerError(std::string(what) + " failed (" + std::to_string(rc) + "): " + igs_rast_last_error());
}

// ---- tensor checks ----
// IGS_DTYPE_* of a float32 / float16 tensor
int dtype_code(const Tensor& t, const char* fn, const char* name)
{
    if (t.scalar_type() == at::kFloat) return IGS_DTYPE_F32;
    if (t.scalar_type() == at::kHalf) return IGS_DTYPE_F16;
    throw NotImplemented(std::string(fn) + ": " + name + " must be float32 or float16 (got " + c10::toString(t.scalar_type()) + ")");
}
// dtype and shape (-1: any size)
void expect(const Tensor& t, const char* fn, const char* name, at::ScalarType dt, std::initializer_list<int64_t> shape)
{
    if (t.scalar_type() != dt)
        throw NotImplemented(std::string(fn) + ": " + name + " must be " + c10::toString(dt) + " (got " + c10::toString(t.scalar_type()) + ")");
    bool ok = t.dim() == (int64_t)shape.size();
    int i = 0;
    for (int64_t n : shape) { if (ok && n >= 0 && t.size(i) != n) ok = false; i++; }
    if (!ok) throw RasterizerError(std::string(fn) + ": " + name + " has shape " + c10::str(t.sizes()) + ", expected " + c10::str(at::IntArrayRef(shape)) + " (-1: any)");
}
// every one of `others` on `like`'s device
struct Named { const Tensor& t; const char* name; };
void same_device(const Tensor& like, const char* fn, std::initializer_list<Named> others)
{
    for (const Named& o : others)
        if (o.t.device() != like.device()) throw RasterizerError(std::string(fn) + ": " + o.name + " must be on " + c10::str(like.device()));
}
// [N, 3] float32 points, at most max_points of them
void check_points(const Tensor& t, const char* fn, const char* name, int64_t max_points)
{
    if (t.scalar_type() != at::kFloat)
        throw RasterizerError(std::string(fn) + ": " + name + " must be float32 (got " + c10::toString(t.scalar_type()) + ")");
    if (t.dim() != 2 || t.size(1) != 3)
        throw RasterizerError(std::string(fn) + ": " + name + " must have shape [N, 3] (got " + c10::str(t.sizes()) + ")");
    if (t.size(0) > max_points)
        throw RasterizerError(std::string(fn) + ": " + std::to_string(t.size(0)) + " points is more than the supported " + std::to_string(max_points));
}
// [n] example offsets on the points' device, as contiguous int32
Tensor offsets_i32(const Tensor& t, const char* fn, const char* name, const Tensor& like, int64_t n)
{
    if (t.dim() != 1 || t.size(0) != n)
        throw RasterizerError(std::string(fn) + ": " + name + " must have shape [" + std::to_string(n) + "] (got " + c10::str(t.sizes()) + ")");
    if (t.device() != like.device()) throw RasterizerError(std::string(fn) + ": " + name + " must be on the points' device");
    return t.to(at::kInt).contiguous();
}

// ---- the context of one native call ----
// Refuses an anchor tensor that is not on a GPU, makes its device current for the rest of the call and yields PyTorch's current stream
// there; then the same-device check of the other tensors.  Constructed after the argument checks.  With `name` the refusal reads
// "<what>: <name> must be on a GPU (no CPU fallback)"; without, `what` is the whole text.
const char* const RASTERIZER_ON_CPU = "igs_amd rasterizer: tensors must be on a GPU (no CPU fallback)";
struct GpuCall {
    c10::Device dev;
    c10::hip::HIPGuardMasqueradingAsCUDA guard;
    GpuCall(const Tensor& t, const char* what, const char* name = nullptr, std::initializer_list<Named> others = {})
        : dev(on_gpu(t, what, name).device()), guard(dev) { same_device(t, what, others); }
    hipStream_t stream() const { return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(dev.index()).stream(); }
    static const Tensor& on_gpu(const Tensor& t, const char* what, const char* name)
    {
        if (!t.is_cuda()) throw RasterizerError(name ? std::string(what) + ": " + name + " must be on a GPU (no CPU fallback)" : std::string(what));
        return t;
    }
};

// ---- pointers for the C call ----
// an output (or input) the caller may not have: its data pointer, or NULL
void* ptr_or_null(const OptTensor& t) { return t ? t->data_ptr() : nullptr; }
template <class T> T* ptr_or_null(const OptTensor& t) { return t ? t->data_ptr<T>() : nullptr; }
// a [B, H, A, 64] view as the attention entry points take it: data pointer and the three outer strides (NULL and zeros when absent)
struct HeadView {
    void* p = nullptr; int64_t sb = 0, sh = 0, sa = 0;
    HeadView(const Tensor& t) : p(t.data_ptr()), sb(t.stride(0)), sh(t.stride(1)), sa(t.stride(2)) {}
    HeadView(const OptTensor& t) { if (t) *this = HeadView(*t); }
};

// ---- the rasterizer (api.hip) ----
// uint8 scratch tensors grown on demand by the library (rasterize_points.cu:27-33, resizeFunctional).  `persistent` sets are born
// zero-filled and only grow (by 25 %): the library leaves its binning counters zeroed after every frame, which lets a caller that
// keeps its set skip the per-frame zero-fill launch (igs_rast_hint_scratch_clean).
struct Grow { at::Tensor* t; bool persistent; };
char* grow_cb(void* user, size_t n)
{
    Grow* g = (Grow*)user;
    try {
        if ((size_t)g->t->numel() < n) {
            auto o = g->t->options();
            *g->t = g->persistent ? at::zeros({(int64_t)(n + n / 4)}, o) : at::empty({(int64_t)n}, o);
        }
        return (char*)g->t->data_ptr();
    } catch (...) {                    // an exception must not cross the C frame
        return nullptr;
    }
}
struct ScratchSet {
    Tensor geom, binning, img, workspace;
    bool persistent;
    c10::Device device;
    Grow g_geom, g_binning, g_img;      // the `user` words of the three growth callbacks (also handed to igs_refine_step by address)
    ScratchSet(c10::Device dev, bool persistent_) : persistent(persistent_), device(dev)
    {
        auto o = at::TensorOptions().dtype(at::kByte).device(dev);
        geom = at::empty({0}, o); binning = at::empty({0}, o); img = at::empty({0}, o); workspace = at::empty({0}, o);
        g_geom = Grow{ &geom, persistent }; g_binning = Grow{ &binning, persistent }; g_img = Grow{ &img, persistent };
    }
    ScratchSet(const ScratchSet&) = delete;
    ScratchSet& operator=(const ScratchSet&) = delete;
    Tensor& ensure_workspace(int64_t P)
    {
        const int64_t need = (int64_t)igs_rast_backward_workspace_bytes((int)P);
        if (workspace.numel() < need) workspace = at::empty({need}, at::TensorOptions().dtype(at::kByte).device(device));
        return workspace;
    }
};

// float32, contiguous, on `dev`; the reference's "empty tensor = absent" convention gives NULL
struct In {
    Tensor keep; const float* p = nullptr;
    In() {}
    In(const OptTensor& t, const c10::Device& dev, const char* what)
    {
        if (!t.has_value() || !t->defined() || t->numel() == 0) return;
        if (t->device() != dev) throw RasterizerError(std::string(what) + " must live on " + dev.str() + " (got " + t->device().str() + ")");
        keep = (t->scalar_type() == at::kFloat && t->is_contiguous()) ? *t : t->to(at::kFloat).contiguous();
        p = keep.data_ptr<float>();
    }
};

// a caller-provided destination tensor: right device, dtype, size, and contiguous (the kernels write raw pointers)
void check_out(const Tensor& t, int64_t numel, at::ScalarType dt, const c10::Device& dev, const char* what)
{
    if (!t.defined() || t.device() != dev || t.scalar_type() != dt || t.numel() != numel || !t.is_contiguous())
        throw RasterizerError(std::string(what) + ": must be a contiguous " + c10::toString(dt) + " tensor of " + std::to_string(numel) +
                              " elements on " + dev.str());
}

// what rasterize_gaussians and count_gaussians share: checks, call context, the eleven float inputs, M, scratch set
struct FwdCall : GpuCall {
    int64_t P, H, W;
    In m3, col, op, sc, rot, cov, shs, bg, view, proj, cam; int64_t M; std::shared_ptr<ScratchSet> ss;
    static const Tensor& points(const Tensor& means3D)
    {
        if (means3D.dim() != 2 || means3D.size(1) != 3) throw RasterizerError("means3D must have dimensions (num_points, 3)");
        return means3D;
    }
    FwdCall(const Tensor& background, const Tensor& means3D, const Tensor& colors, const Tensor& opacity, const Tensor& scales,
            const Tensor& rotations, const Tensor& cov3D_precomp, const Tensor& viewmatrix, const Tensor& projmatrix, const Tensor& sh,
            const Tensor& campos, int64_t image_height, int64_t image_width, const std::shared_ptr<ScratchSet>& scratch)
        : GpuCall(points(means3D), RASTERIZER_ON_CPU), P(means3D.size(0)), H(image_height), W(image_width),
          m3(means3D, dev, "means3D"), col(colors, dev, "colors_precomp"), op(opacity, dev, "opacities"), sc(scales, dev, "scales"),
          rot(rotations, dev, "rotations"), cov(cov3D_precomp, dev, "cov3D_precomp"), shs(sh, dev, "shs"), bg(background, dev, "bg"),
          view(viewmatrix, dev, "viewmatrix"), proj(projmatrix, dev, "projmatrix"), cam(campos, dev, "campos"), M(shs.p ? shs.keep.size(1) : 0),
          ss(scratch ? scratch : std::make_shared<ScratchSet>(dev, false))
    {
        if (H <= 0 || W <= 0) throw RasterizerError("image_height and image_width must be positive");
        if (scratch && scratch->device != dev) throw RasterizerError("scratch set lives on " + scratch->device.str() + ", the tensors on " + dev.str());
    }
};

using FwdTuple = std::tuple<int64_t, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor>;

// _C.rasterize_gaussians (RasterizeGaussiansCUDA, DGR/rasterize_points.cu:35-133).
// Returns (num_rendered, color, coord, mcoord, alpha, normal, depth, mdepth, radii, geomBuffer, binningBuffer, imgBuffer).
// mode 0: one host wait for the instance count (as the reference); 1: igs_rast_forward_async (caller must call forward_finish);
// 2: igs_rast_forward_nowait (stream capture).  In modes 1 / 2 num_rendered is INT_MAX, which the backward accepts.
FwdTuple rasterize_gaussians(
    const Tensor& background, const Tensor& means3D, const Tensor& colors, const Tensor& opacity, const Tensor& scales,
    const Tensor& rotations, double scale_modifier, const Tensor& cov3D_precomp, const Tensor& viewmatrix, const Tensor& projmatrix,
    double tan_fovx, double tan_fovy, double kernel_size, int64_t image_height, int64_t image_width, const Tensor& sh, int64_t degree,
    const Tensor& campos, bool prefiltered, bool require_coord, bool require_depth, bool debug,
    const std::shared_ptr<ScratchSet>& scratch, const OptTensor& out_images, const OptTensor& out_radii, int64_t mode, bool scratch_clean)
{
    const FwdCall c(background, means3D, colors, opacity, scales, rotations, cov3D_precomp, viewmatrix, projmatrix, sh, campos, image_height, image_width, scratch);
    const int64_t P = c.P, H = c.H, W = c.W;
    auto fopt = at::TensorOptions().dtype(at::kFloat).device(c.dev);
    // one allocation for the seven images; every pixel is written by the kernels when P > 0
    if (out_images.has_value()) check_out(*out_images, 15 * H * W, at::kFloat, c.dev, "out_images");
    if (out_radii.has_value()) check_out(*out_radii, P, at::kInt, c.dev, "out_radii");
    Tensor imgs = out_images.has_value() ? *out_images : (P > 0 ? at::empty({15, H, W}, fopt) : at::zeros({15, H, W}, fopt));
    Tensor radii = out_radii.has_value() ? *out_radii : (P > 0 ? at::empty({P}, fopt.dtype(at::kInt)) : at::zeros({0}, fopt.dtype(at::kInt)));
    Tensor color = imgs.narrow(0, 0, 3), coord = imgs.narrow(0, 3, 3), mcoord = imgs.narrow(0, 6, 3), depth = imgs.narrow(0, 9, 1),
           mdepth = imgs.narrow(0, 10, 1), alpha = imgs.narrow(0, 11, 1), normal = imgs.narrow(0, 12, 3);
    int64_t rendered = 0;
    if (P != 0) {
        auto fwd = mode == 1 ? igs_rast_forward_async : (mode == 2 ? igs_rast_forward_nowait : igs_rast_forward);
        if (scratch_clean) igs_rast_hint_scratch_clean(1);
        float* ib = imgs.data_ptr<float>(); const size_t HW = (size_t)H * W;
        rendered = fwd(c.stream(), grow_cb, &c.ss->g_geom, grow_cb, &c.ss->g_binning, grow_cb, &c.ss->g_img, (int)P, (int)degree, (int)c.M, c.bg.p,
                       (int)W, (int)H, c.m3.p, c.shs.p, c.col.p, c.op.p, c.sc.p, (float)scale_modifier, c.rot.p, c.cov.p, c.view.p, c.proj.p,
                       c.cam.p, (float)tan_fovx, (float)tan_fovy, (float)kernel_size, prefiltered ? 1 : 0, ib, ib + 3 * HW, ib + 6 * HW, ib + 9 * HW,
                       ib + 10 * HW, ib + 11 * HW, ib + 12 * HW, radii.data_ptr<int>(), require_coord ? 1 : 0, require_depth ? 1 : 0, debug ? 1 : 0);
        check((int)rendered, "igs_rast_forward");
    }
    return FwdTuple(rendered, color, coord, mcoord, alpha, normal, depth, mdepth, radii, c.ss->geom, c.ss->binning, c.ss->img);
}

using CountTuple = std::tuple<Tensor, Tensor, int64_t, Tensor, Tensor, Tensor, Tensor, Tensor>;

// _C.count_gaussians of the compress package (CountGaussiansCUDA, compress-diff-gaussian-rasterization rasterize_points.cu:130-217):
// the reference's 20 positional arguments (no kernel_size: vanilla 3DGS; f_count is accepted and, as there, not read).
// Returns (gaussians_count [P] int32, important_score [P] float32, num_rendered, color [3,H,W], radii [P] int32, geomBuffer,
// binningBuffer, imgBuffer).  The count is exact and the score is count x opacity (include/igs_rast.h: igs_rast_count_gaussians).
CountTuple count_gaussians(
    const Tensor& background, const Tensor& means3D, const Tensor& colors, const Tensor& opacity, const Tensor& scales,
    const Tensor& rotations, double scale_modifier, const Tensor& cov3D_precomp, const Tensor& viewmatrix, const Tensor& projmatrix,
    double tan_fovx, double tan_fovy, int64_t image_height, int64_t image_width, const Tensor& sh, int64_t degree,
    const Tensor& campos, bool prefiltered, bool debug, bool /*f_count*/, const std::shared_ptr<ScratchSet>& scratch)
{
    const FwdCall c(background, means3D, colors, opacity, scales, rotations, cov3D_precomp, viewmatrix, projmatrix, sh, campos, image_height, image_width, scratch);
    const int64_t P = c.P, H = c.H, W = c.W;
    auto fopt = at::TensorOptions().dtype(at::kFloat).device(c.dev), iopt = fopt.dtype(at::kInt);
    // every element is written by the kernels when P > 0 (counts: zeroed by the preprocess; colour: every pixel)
    Tensor color = P > 0 ? at::empty({3, H, W}, fopt) : at::zeros({3, H, W}, fopt);
    Tensor radii = P > 0 ? at::empty({P}, iopt) : at::zeros({0}, iopt);
    Tensor count = P > 0 ? at::empty({P}, iopt) : at::zeros({0}, iopt);
    Tensor score = P > 0 ? at::empty({P}, fopt) : at::zeros({0}, fopt);
    int64_t rendered = 0;
    if (P != 0) {
        rendered = igs_rast_count_gaussians(c.stream(), grow_cb, &c.ss->g_geom, grow_cb, &c.ss->g_binning, grow_cb, &c.ss->g_img, (int)P, (int)degree,
                                            (int)c.M, c.bg.p, (int)W, (int)H, c.m3.p, c.shs.p, c.col.p, c.op.p, c.sc.p, (float)scale_modifier,
                                            c.rot.p, c.cov.p, c.view.p, c.proj.p, c.cam.p, (float)tan_fovx, (float)tan_fovy, prefiltered ? 1 : 0,
                                            color.data_ptr<float>(), count.data_ptr<int>(), score.data_ptr<float>(), radii.data_ptr<int>(),
                                            debug ? 1 : 0);
        check((int)rendered, "igs_rast_count_gaussians");
    }
    return CountTuple(count, score, rendered, color, radii, c.ss->geom, c.ss->binning, c.ss->img);
}

using BwdTuple = std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor>;

// Body of _C.rasterize_gaussians_backward[_ex] (RasterizeGaussiansBackwardCUDA, DGR/rasterize_points.cu:135-246).  After the two options
// of _ex, its parameters ARE the Python-visible list -- the reference's 32 positional arguments, then the 9 keyword extras: the two
// bound functions take their types from this declaration (BackwardFns below) and their names from def_backward.  The seven small
// gradients are carved from ONE [23 P] block (m2d 3 | colors 3 | opacity 1 | means3D 3 | scales 3 | rot 4 | cov3D 6); every element is
// written by the kernels (no zero fills).  Returns the reference's 8-tuple and, with nan_report, whether a NaN was written.
struct BwdResult { BwdTuple grads; int64_t nan = 0; int64_t nan_word = 0; int64_t nan_seq = 0; };
BwdResult backward_body(
    int64_t nan_report, double clamp,
    const Tensor& background, const Tensor& means3D, const Tensor& radii, const Tensor& colors, const Tensor& scales, const Tensor& rotations,
    double scale_modifier, const Tensor& cov3D_precomp, const Tensor& viewmatrix, const Tensor& projmatrix, double tan_fovx, double tan_fovy,
    double kernel_size, const OptTensor& dL_dout_color, const OptTensor& dL_dout_coord, const OptTensor& dL_dout_mcoord,
    const OptTensor& dL_dout_depth, const OptTensor& dL_dout_mdepth, const OptTensor& dL_dout_alpha, const OptTensor& dL_dout_normal,
    const Tensor& normalmap, const Tensor& sh, int64_t degree, const Tensor& campos, const Tensor& geomBuffer, int64_t R,
    const Tensor& binningBuffer, const Tensor& imageBuffer, const Tensor& alphas, bool require_coord, bool require_depth, bool debug,
    const OptTensor& workspace, const OptTensor& out_means2D, const OptTensor& out_colors, const OptTensor& out_opacity,
    const OptTensor& out_means3D, const OptTensor& out_cov3D, const OptTensor& out_sh, const OptTensor& out_scales,
    const OptTensor& out_rotations)
{
    const GpuCall c(means3D, RASTERIZER_ON_CPU);
    const c10::Device& dev = c.dev;
    const int64_t P = means3D.size(0);
    const int64_t H = alphas.size(-2), W = alphas.size(-1);
    In shs(sh, dev, "shs");
    const int64_t M = shs.p ? shs.keep.size(1) : 0;
    auto fopt = at::TensorOptions().dtype(at::kFloat).device(dev);
    Tensor dL_dsh = out_sh.has_value() ? *out_sh : (P > 0 ? at::empty({P, M, 3}, fopt) : at::zeros({P, M, 3}, fopt));
    Tensor block = P > 0 ? at::empty({23 * P}, fopt) : at::zeros({0}, fopt);
    int64_t o = 0;
    if (out_sh.has_value()) check_out(*out_sh, P * M * 3, at::kFloat, dev, "out_sh");
    auto carve = [&](int64_t k, const OptTensor& given) {
        if (given.has_value()) check_out(*given, k * P, at::kFloat, dev, "gradient destination");
        Tensor t = given.has_value() ? *given : block.narrow(0, o, k * P).view({P, k});
        o += k * P;
        return t;
    };
    Tensor dL_dmeans2D = carve(3, out_means2D), dL_dcolors = carve(3, out_colors), dL_dopacity = carve(1, out_opacity),
           dL_dmeans3D = carve(3, out_means3D), dL_dscales = carve(3, out_scales), dL_drotations = carve(4, out_rotations),
           dL_dcov3D = carve(6, out_cov3D);
    BwdResult res;
    if (P != 0) {
        In m3(means3D, dev, "means3D"), col(colors, dev, "colors_precomp"), sc(scales, dev, "scales"), rot(rotations, dev, "rotations"),
           cov(cov3D_precomp, dev, "cov3D_precomp"), bg(background, dev, "bg"), view(viewmatrix, dev, "viewmatrix"),
           proj(projmatrix, dev, "projmatrix"), cam(campos, dev, "campos"), al(alphas, dev, "alphas"), nm(normalmap, dev, "normalmap");
        In g0(dL_dout_color, dev, "grad"), g1(dL_dout_coord, dev, "grad"), g2(dL_dout_mcoord, dev, "grad"), g3(dL_dout_depth, dev, "grad"),
           g4(dL_dout_mdepth, dev, "grad"), g5(dL_dout_alpha, dev, "grad"), g6(dL_dout_normal, dev, "grad");
        Tensor radii_c = radii.contiguous();
        const int64_t need = (int64_t)igs_rast_backward_workspace_bytes((int)P);
        Tensor ws = (workspace.has_value() && workspace->numel() >= need) ? *workspace
                                                                           : at::empty({need}, at::TensorOptions().dtype(at::kByte).device(dev));
        if (nan_report || clamp > 0.0) igs_rast_next_backward_options(nan_report ? 1 : 0, (float)clamp);
        auto bp = [](const Tensor& t) { return t.numel() ? (const char*)t.data_ptr() : nullptr; };
        const int rc = igs_rast_backward(
            c.stream(), (int)P, (int)degree, (int)M, (int)std::min<int64_t>(R, INT_MAX), bg.p, (int)W, (int)H, m3.p, shs.p, col.p, al.p, sc.p,
            (float)scale_modifier, rot.p, cov.p, view.p, proj.p, cam.p, (float)tan_fovx, (float)tan_fovy, (float)kernel_size,
            radii_c.data_ptr<int>(), nm.p, bp(geomBuffer), bp(binningBuffer), bp(imageBuffer), g0.p, g1.p, g2.p, g3.p, g4.p, g5.p, g6.p,
            ws.data_ptr(), dL_dmeans2D.data_ptr<float>(), dL_dcolors.data_ptr<float>(), dL_dopacity.data_ptr<float>(),
            dL_dmeans3D.data_ptr<float>(), dL_dcov3D.data_ptr<float>(), M > 0 ? dL_dsh.data_ptr<float>() : nullptr,
            dL_dscales.data_ptr<float>(), dL_drotations.data_ptr<float>(), require_coord ? 1 : 0, require_depth ? 1 : 0, debug ? 1 : 0);
        check(rc, "igs_rast_backward");
        if (nan_report == 1) {                 // wait here (the reference's place for its asserts)
            const int v = igs_rast_nan_report_wait();
            check(v, "igs_rast_nan_report_wait");
            res.nan = v;
        } else if (nan_report == 2) {          // hand the verdict's address out: the caller waits once the whole backward pass is enqueued
            const void* word = nullptr; unsigned seq = 0;
            check(igs_rast_nan_report_handle(&word, &seq), "igs_rast_nan_report_handle");
            res.nan_word = (int64_t)(uintptr_t)word; res.nan_seq = (int64_t)seq;
        }
    }
    res.grads = BwdTuple(dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations);
    return res;
}

// the two functions Python sees, over backward_body's own parameter types A...
template <class Body> struct BackwardFns;
template <class... A> struct BackwardFns<BwdResult(int64_t, double, A...)> {
    static BwdTuple plain(A... a) { return backward_body(0, 0.0, a...).grads; }
    // nan_report: 0 none; 1 wait for the kernel's verdict here -> (grads, 0 / 1, 0, 0); 2 deferred -> (grads, 0, word, seq) for nan_report_wait
    static std::tuple<BwdTuple, int64_t, int64_t, int64_t> ex(A... a, int64_t nan_report, double clamp)
    {
        BwdResult r = backward_body(nan_report, clamp, a...);
        return std::make_tuple(r.grads, r.nan, r.nan_word, r.nan_seq);
    }
};

// ---- V views of one Gaussian set (api.hip: igs_rast_forward_views / igs_rast_backward_views; no reference counterpart as one call: the
// view loop of igs/models/gs.py:839-847 over RasterizeGaussiansCUDA / RasterizeGaussiansBackwardCUDA, DGR/rasterize_points.cu:35-246) ----
// what the two functions check alike: float32 everywhere, V cameras, V scratch sets, P rows in every per-Gaussian input
struct ViewsCall : GpuCall {
    int64_t V, P;
    static const Tensor& checked(const char* fn, const Tensor& means3D, const Tensor& viewmatrices, const Tensor& projmatrices, const Tensor& camposes,
                                 size_t n_scratch, std::initializer_list<Named> per_gaussian, std::initializer_list<Named> floats)
    {
        const std::string f(fn);
        if (means3D.dim() != 2 || means3D.size(1) != 3) throw RasterizerError(f + ": means3D must have dimensions (num_points, 3)");
        const int64_t V = viewmatrices.dim() >= 1 ? viewmatrices.size(0) : 0, P = means3D.size(0);
        if (V < 1 || V > igs_rast_views_max())
            throw RasterizerError(f + ": " + std::to_string(V) + " views; one call takes 1 .. " + std::to_string(igs_rast_views_max()));
        if (viewmatrices.numel() != 16 * V || projmatrices.numel() != 16 * V || projmatrices.size(0) != V || camposes.numel() != 3 * V || camposes.size(0) != V)
            throw RasterizerError(f + ": viewmatrices / projmatrices / camposes must be [V, 4, 4], [V, 4, 4], [V, 3] with the same V");
        if ((int64_t)n_scratch != V) throw RasterizerError(f + ": " + std::to_string(n_scratch) + " scratch sets for " + std::to_string(V) + " views");
        for (const Named& o : per_gaussian)
            if (o.t.numel() && o.t.size(0) != P) throw RasterizerError(f + ": " + o.name + " has " + std::to_string(o.t.size(0)) + " rows, means3D " + std::to_string(P));
        for (const Named& o : floats)
            if (o.t.defined() && o.t.numel() && o.t.scalar_type() != at::kFloat)
                throw RasterizerError(f + ": " + o.name + " must be float32 (got " + c10::toString(o.t.scalar_type()) + ")");
        return means3D;
    }
    ViewsCall(const char* fn, const Tensor& means3D, const Tensor& viewmatrices, const Tensor& projmatrices, const Tensor& camposes, size_t n_scratch,
              std::initializer_list<Named> per_gaussian, std::initializer_list<Named> floats)
        : GpuCall(checked(fn, means3D, viewmatrices, projmatrices, camposes, n_scratch, per_gaussian, floats), RASTERIZER_ON_CPU),
          V(viewmatrices.size(0)), P(means3D.size(0)) {}
};
using ScratchSets = std::vector<std::shared_ptr<ScratchSet>>;
using ViewsFwdTuple = std::tuple<std::vector<int64_t>, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor>;

// _C._views.rasterize_views: rasterize_gaussians' arguments with [V, 4, 4] / [V, 4, 4] / [V, 3] cameras and one scratch set per view.
// Returns (num_rendered [V], color, coord, mcoord, alpha, normal, depth, mdepth -- each [V, c, H, W] -- and radii [V, P]).
ViewsFwdTuple rasterize_views(
    const Tensor& background, const Tensor& means3D, const Tensor& colors, const Tensor& opacity, const Tensor& scales,
    const Tensor& rotations, double scale_modifier, const Tensor& cov3D_precomp, const Tensor& viewmatrices, const Tensor& projmatrices,
    double tan_fovx, double tan_fovy, double kernel_size, int64_t image_height, int64_t image_width, const Tensor& sh, int64_t degree,
    const Tensor& camposes, bool prefiltered, bool require_coord, bool require_depth, bool debug, const ScratchSets& scratch, bool scratch_clean)
{
    const char* fn = "rasterize_views";
    const ViewsCall c(fn, means3D, viewmatrices, projmatrices, camposes, scratch.size(),
                      { {colors, "colors_precomp"}, {opacity, "opacities"}, {scales, "scales"}, {rotations, "rotations"}, {cov3D_precomp, "cov3D_precomp"}, {sh, "shs"} },
                      { {background, "bg"}, {means3D, "means3D"}, {colors, "colors_precomp"}, {opacity, "opacities"}, {scales, "scales"}, {rotations, "rotations"},
                        {cov3D_precomp, "cov3D_precomp"}, {sh, "shs"}, {viewmatrices, "viewmatrices"}, {projmatrices, "projmatrices"}, {camposes, "camposes"} });
    const int64_t V = c.V, P = c.P, H = image_height, W = image_width;
    if (H <= 0 || W <= 0) throw RasterizerError("image_height and image_width must be positive");
    for (const auto& ss : scratch)
        if (!ss || ss->device != c.dev) throw RasterizerError("rasterize_views: every scratch set must live on " + c.dev.str());
    auto fopt = at::TensorOptions().dtype(at::kFloat).device(c.dev);
    // one allocation for the seven image stacks ([V][c][H][W] each, as the C call writes them); every pixel is written when P > 0
    Tensor imgs = P > 0 ? at::empty({15 * V * H * W}, fopt) : at::zeros({15 * V * H * W}, fopt);
    Tensor radii = P > 0 ? at::empty({V, P}, fopt.dtype(at::kInt)) : at::zeros({V, 0}, fopt.dtype(at::kInt));
    const int64_t HW = H * W;
    auto stack = [&](int64_t first, int64_t ch) { return imgs.narrow(0, first * V * HW, ch * V * HW).view({V, ch, H, W}); };
    Tensor color = stack(0, 3), coord = stack(3, 3), mcoord = stack(6, 3), depth = stack(9, 1), mdepth = stack(10, 1), alpha = stack(11, 1),
           normal = stack(12, 3);
    std::vector<int64_t> rendered((size_t)V, 0);
    if (P != 0) {
        In m3(means3D, c.dev, "means3D"), col(colors, c.dev, "colors_precomp"), op(opacity, c.dev, "opacities"), sc(scales, c.dev, "scales"),
           rot(rotations, c.dev, "rotations"), cov(cov3D_precomp, c.dev, "cov3D_precomp"), shs(sh, c.dev, "shs"), bg(background, c.dev, "bg"),
           view(viewmatrices, c.dev, "viewmatrices"), proj(projmatrices, c.dev, "projmatrices"), cam(camposes, c.dev, "camposes");
        const int64_t M = shs.p ? shs.keep.size(1) : 0;
        std::vector<void*> ug, ub, ui;
        for (const auto& ss : scratch) { ug.push_back(&ss->g_geom); ub.push_back(&ss->g_binning); ui.push_back(&ss->g_img); }
        std::vector<int> nr((size_t)V, 0);
        if (scratch_clean) igs_rast_hint_scratch_clean(1);
        check(igs_rast_forward_views(c.stream(), (int)V, grow_cb, ug.data(), grow_cb, ub.data(), grow_cb, ui.data(), (int)P, (int)degree, (int)M, bg.p,
                                     (int)W, (int)H, m3.p, shs.p, col.p, op.p, sc.p, (float)scale_modifier, rot.p, cov.p, view.p, proj.p, cam.p,
                                     (float)tan_fovx, (float)tan_fovy, (float)kernel_size, prefiltered ? 1 : 0, color.data_ptr<float>(),
                                     coord.data_ptr<float>(), mcoord.data_ptr<float>(), depth.data_ptr<float>(), mdepth.data_ptr<float>(),
                                     alpha.data_ptr<float>(), normal.data_ptr<float>(), radii.data_ptr<int>(), nr.data(), require_coord ? 1 : 0,
                                     require_depth ? 1 : 0, debug ? 1 : 0),
              "igs_rast_forward_views");
        for (int64_t v = 0; v < V; v++) rendered[(size_t)v] = nr[(size_t)v];
    }
    return ViewsFwdTuple(rendered, color, coord, mcoord, alpha, normal, depth, mdepth, radii);
}

// _C._views.rasterize_views_backward: the upstream gradients are [V, c, H, W] stacks or None (= zeros for every view); `scratch` and `R` are the
// forward's sets and counts.  Returns ((dL_dmeans2D [V, P, 3] or an empty tensor, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh,
// dL_dscales, dL_drotations -- summed over the views), nan flag, verdict word, sequence number) as rasterize_gaussians_backward_ex does.
std::tuple<BwdTuple, int64_t, int64_t, int64_t> rasterize_views_backward(
    const Tensor& background, const Tensor& means3D, const Tensor& radii, const Tensor& colors, const Tensor& scales, const Tensor& rotations,
    double scale_modifier, const Tensor& cov3D_precomp, const Tensor& viewmatrices, const Tensor& projmatrices, double tan_fovx, double tan_fovy,
    double kernel_size, const OptTensor& dL_dout_color, const OptTensor& dL_dout_coord, const OptTensor& dL_dout_mcoord,
    const OptTensor& dL_dout_depth, const OptTensor& dL_dout_mdepth, const OptTensor& dL_dout_alpha, const OptTensor& dL_dout_normal,
    const Tensor& normalmap, const Tensor& sh, int64_t degree, const Tensor& camposes, const ScratchSets& scratch, const std::vector<int64_t>& R,
    const Tensor& alphas, bool require_coord, bool require_depth, bool debug, bool want_means2D, int64_t nan_report, double clamp)
{
    const char* fn = "rasterize_views_backward";
    const ViewsCall c(fn, means3D, viewmatrices, projmatrices, camposes, scratch.size(),
                      { {colors, "colors_precomp"}, {scales, "scales"}, {rotations, "rotations"}, {cov3D_precomp, "cov3D_precomp"}, {sh, "shs"} },
                      { {background, "bg"}, {means3D, "means3D"}, {colors, "colors_precomp"}, {scales, "scales"}, {rotations, "rotations"},
                        {cov3D_precomp, "cov3D_precomp"}, {sh, "shs"}, {viewmatrices, "viewmatrices"}, {projmatrices, "projmatrices"}, {camposes, "camposes"},
                        {normalmap, "normalmap"}, {alphas, "alphas"} });
    const c10::Device& dev = c.dev;
    const int64_t V = c.V, P = c.P;
    if ((int64_t)R.size() != V) throw RasterizerError("rasterize_views_backward: R must hold one instance count per view");
    if (alphas.dim() != 4 || alphas.size(0) != V || normalmap.dim() != 4 || normalmap.size(0) != V)
        throw RasterizerError("rasterize_views_backward: alphas / normalmap must be the forward's [V, c, H, W] stacks");
    if (P > 0 && (radii.dim() != 2 || radii.size(0) != V || radii.size(1) != P || radii.scalar_type() != at::kInt))
        throw RasterizerError("rasterize_views_backward: radii must be int32 [V, P]");
    const int64_t H = alphas.size(-2), W = alphas.size(-1);
    const int64_t ch[7] = { 3, 3, 3, 1, 1, 1, 3 };
    const OptTensor* ups[7] = { &dL_dout_color, &dL_dout_coord, &dL_dout_mcoord, &dL_dout_depth, &dL_dout_mdepth, &dL_dout_alpha, &dL_dout_normal };
    for (int k = 0; k < 7; k++)
        if (ups[k]->has_value() && (*ups[k])->defined() && (*ups[k])->numel() != V * ch[k] * H * W)
            throw RasterizerError("rasterize_views_backward: an upstream gradient is not a [V, c, H, W] stack of the forward's size");
    In shs(sh, dev, "shs");
    const int64_t M = shs.p ? shs.keep.size(1) : 0;
    auto fopt = at::TensorOptions().dtype(at::kFloat).device(dev);
    Tensor dL_dsh = P > 0 ? at::empty({P, M, 3}, fopt) : at::zeros({P, M, 3}, fopt);
    Tensor block = P > 0 ? at::empty({20 * P}, fopt) : at::zeros({0}, fopt);
    Tensor dL_dmeans2D = (want_means2D && P > 0) ? at::empty({V, P, 3}, fopt) : at::zeros({want_means2D ? V : 0, want_means2D ? P : 0, 3}, fopt);
    int64_t o = 0;
    auto carve = [&](int64_t k) { Tensor t = block.narrow(0, o, k * P).view({P, k}); o += k * P; return t; };
    Tensor dL_dcolors = carve(3), dL_dopacity = carve(1), dL_dmeans3D = carve(3), dL_dscales = carve(3), dL_drotations = carve(4), dL_dcov3D = carve(6);
    int64_t nan = 0, nan_word = 0, nan_seq = 0;
    if (P != 0) {
        In m3(means3D, dev, "means3D"), col(colors, dev, "colors_precomp"), sc(scales, dev, "scales"), rot(rotations, dev, "rotations"),
           cov(cov3D_precomp, dev, "cov3D_precomp"), bg(background, dev, "bg"), view(viewmatrices, dev, "viewmatrices"),
           proj(projmatrices, dev, "projmatrices"), cam(camposes, dev, "camposes"), al(alphas, dev, "alphas"), nm(normalmap, dev, "normalmap");
        In g0(dL_dout_color, dev, "grad"), g1(dL_dout_coord, dev, "grad"), g2(dL_dout_mcoord, dev, "grad"), g3(dL_dout_depth, dev, "grad"),
           g4(dL_dout_mdepth, dev, "grad"), g5(dL_dout_alpha, dev, "grad"), g6(dL_dout_normal, dev, "grad");
        Tensor radii_c = radii.contiguous();
        Tensor ws = at::empty({V * (int64_t)igs_rast_backward_workspace_bytes((int)P)}, at::TensorOptions().dtype(at::kByte).device(dev));
        std::vector<const char*> pg, pb, pi; std::vector<int> nr;
        auto bp = [](const Tensor& t) { return t.numel() ? (const char*)t.data_ptr() : nullptr; };
        for (int64_t v = 0; v < V; v++) {
            const auto& ss = scratch[(size_t)v];
            if (!ss || ss->device != dev) throw RasterizerError("rasterize_views_backward: every scratch set must live on " + dev.str());
            pg.push_back(bp(ss->geom)); pb.push_back(bp(ss->binning)); pi.push_back(bp(ss->img));
            nr.push_back((int)std::min<int64_t>(R[(size_t)v], INT_MAX));
        }
        if (nan_report || clamp > 0.0) igs_rast_next_backward_options(nan_report ? 1 : 0, (float)clamp);
        check(igs_rast_backward_views(
                  c.stream(), (int)V, (int)P, (int)degree, (int)M, nr.data(), bg.p, (int)W, (int)H, m3.p, shs.p, col.p, al.p, sc.p, (float)scale_modifier,
                  rot.p, cov.p, view.p, proj.p, cam.p, (float)tan_fovx, (float)tan_fovy, (float)kernel_size, radii_c.data_ptr<int>(), nm.p, pg.data(),
                  pb.data(), pi.data(), g0.p, g1.p, g2.p, g3.p, g4.p, g5.p, g6.p, ws.data_ptr(), want_means2D ? dL_dmeans2D.data_ptr<float>() : nullptr,
                  dL_dcolors.data_ptr<float>(), dL_dopacity.data_ptr<float>(), dL_dmeans3D.data_ptr<float>(), dL_dcov3D.data_ptr<float>(),
                  M > 0 ? dL_dsh.data_ptr<float>() : nullptr, dL_dscales.data_ptr<float>(), dL_drotations.data_ptr<float>(), require_coord ? 1 : 0,
                  require_depth ? 1 : 0, debug ? 1 : 0),
              "igs_rast_backward_views");
        if (nan_report == 1) {
            const int v = igs_rast_nan_report_wait();
            check(v, "igs_rast_nan_report_wait");
            nan = v;
        } else if (nan_report == 2) {
            const void* word = nullptr; unsigned seq = 0;
            check(igs_rast_nan_report_handle(&word, &seq), "igs_rast_nan_report_handle");
            nan_word = (int64_t)(uintptr_t)word; nan_seq = (int64_t)seq;
        }
    }
    return std::make_tuple(BwdTuple(dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations), nan, nan_word, nan_seq);
}

// _C.mark_visible (DGR/rasterize_points.cu:248-267)
Tensor mark_visible(const Tensor& means3D, const Tensor& viewmatrix, const Tensor& projmatrix)
{
    const GpuCall c(means3D, RASTERIZER_ON_CPU);
    const int64_t P = means3D.size(0);
    Tensor present = at::zeros({P}, at::TensorOptions().dtype(at::kBool).device(c.dev));
    if (P != 0) {
        In m(means3D, c.dev, "means3D"), v(viewmatrix, c.dev, "viewmatrix"), p(projmatrix, c.dev, "projmatrix");
        check(igs_rast_mark_visible(c.stream(), (int)P, m.p, v.p, p.p, (uint8_t*)present.data_ptr()), "igs_rast_mark_visible");
    }
    return present;
}

// ---- simple_knn (knn.hip) ----
// simple_knn._C.distCUDA2 (simple-knn ext.cpp / spatial.cu): mean squared distance of every point to its three nearest neighbours
Tensor distCUDA2(const Tensor& points)
{
    const char* fn = "distCUDA2";
    check_points(points, fn, "points", IGS_KNN_MAX_POINTS);
    const GpuCall c(points, fn, "points");
    const int64_t P = points.size(0);
    Tensor out = at::empty({P}, points.options());
    if (P == 0) return out;
    const Tensor xyz = points.contiguous();
    Tensor scratch = at::empty({(int64_t)igs_knn_scratch_bytes((int)P)}, points.options().dtype(at::kByte));
    check(igs_knn_mean_dist2(c.stream(), (int)P, xyz.data_ptr<float>(), scratch.data_ptr(), out.data_ptr<float>()), "igs_knn_mean_dist2");
    return out;
}

// ---- the anchor graph (anchors.hip; contracts in include/igs_rast.h) ----
// select_points_bbox for B examples at once: (xyz_in_box [N, 3], index inside the example [N] int64, count [B] int32); the first
// sum(count) rows are example 0's in-box points in index order, then example 1's, ...
std::tuple<Tensor, Tensor, Tensor> anchors_bbox_select(const Tensor& xyz, const Tensor& ptr, const Tensor& box)
{
    const char* fn = "anchors_bbox_select";
    check_points(xyz, fn, "xyz", IGS_ANCHOR_MAX_POINTS);
    const int64_t B = ptr.dim() == 1 ? ptr.size(0) - 1 : -1;
    if (B < 1 || B > IGS_ANCHOR_MAX_EXAMPLES) throw RasterizerError("anchors_bbox_select: ptr must have shape [B + 1], 1 <= B <= IGS_ANCHOR_MAX_EXAMPLES");
    if (box.scalar_type() != at::kFloat || box.numel() != B * 6 || box.device() != xyz.device())
        throw RasterizerError("anchors_bbox_select: box must be float32 [B, 2, 3] on the points' device");
    const GpuCall c(xyz, fn, "xyz");
    const int64_t N = xyz.size(0);
    const Tensor p = offsets_i32(ptr, fn, "ptr", xyz, B + 1), bx = box.contiguous(), x = xyz.contiguous();
    Tensor out_xyz = at::empty({N, 3}, xyz.options()), out_idx = at::empty({N}, xyz.options().dtype(at::kLong));
    Tensor count = at::empty({B}, xyz.options().dtype(at::kInt));
    Tensor scratch = at::empty({(int64_t)igs_bbox_select_scratch_bytes((int)N)}, xyz.options().dtype(at::kByte));
    check(igs_bbox_select(c.stream(), (int)B, (int)N, x.data_ptr<float>(), p.data_ptr<int>(), bx.data_ptr<float>(), scratch.data_ptr(),
                          out_xyz.data_ptr<float>(), out_idx.data_ptr<int64_t>(), count.data_ptr<int>()), "igs_bbox_select");
    return {out_xyz, out_idx, count};
}

// farthest-point sampling: `total` samples, example b's at [out_ptr[b], out_ptr[b + 1]) (indices into xyz, selection order); max_n
// bounds every example's size
Tensor anchors_fps(const Tensor& xyz, const Tensor& ptr, const Tensor& start, const Tensor& out_ptr, int64_t total, int64_t max_n, double init_d2)
{
    const char* fn = "anchors_fps";
    check_points(xyz, fn, "xyz", IGS_ANCHOR_MAX_POINTS);
    const int64_t B = ptr.dim() == 1 ? ptr.size(0) - 1 : -1;
    if (B < 1 || B > IGS_ANCHOR_MAX_EXAMPLES) throw RasterizerError("anchors_fps: ptr must have shape [B + 1], 1 <= B <= IGS_ANCHOR_MAX_EXAMPLES");
    if (max_n < 0 || max_n > IGS_FPS_MAX_EXAMPLE_POINTS)
        throw RasterizerError("anchors_fps: an example of " + std::to_string(max_n) + " points is more than the supported " + std::to_string(IGS_FPS_MAX_EXAMPLE_POINTS));
    if (total < 0 || total > IGS_ANCHOR_MAX_POINTS) throw RasterizerError("anchors_fps: total out of range");
    if (!(init_d2 >= 0.0)) throw RasterizerError("anchors_fps: init_d2 must be >= 0");
    const GpuCall c(xyz, fn, "xyz");
    const Tensor p = offsets_i32(ptr, fn, "ptr", xyz, B + 1), st = offsets_i32(start, fn, "start", xyz, B);
    const Tensor op = offsets_i32(out_ptr, fn, "out_ptr", xyz, B + 1), x = xyz.contiguous();
    Tensor out = at::empty({total}, xyz.options().dtype(at::kLong));
    if (total == 0) return out;
    const int N = (int)xyz.size(0);
    Tensor scratch = at::empty({(int64_t)igs_fps_scratch_bytes((int)B, N, (int)max_n)}, xyz.options().dtype(at::kByte));
    check(igs_fps(c.stream(), (int)B, N, (int)max_n, x.data_ptr<float>(), p.data_ptr<int>(), st.data_ptr<int>(), op.data_ptr<int>(),
                  (int)total, (float)init_d2, scratch.data_ptr(), out.data_ptr<int64_t>()), "igs_fps");
    return out;
}

// torch_cluster knn as fixed shapes: (index into x [Ny, k] int64 with -1 padding, d2 [Ny, k] or None, weights [Ny, k] or None)
std::tuple<Tensor, OptTensor, OptTensor> anchors_knn(const Tensor& x, const Tensor& y, const Tensor& ptr_x, const Tensor& ptr_y, int64_t k,
                                                     bool with_d2, c10::optional<double> weight_scale)
{
    const char* fn = "anchors_knn";
    check_points(x, fn, "x", IGS_ANCHOR_MAX_POINTS);
    check_points(y, fn, "y", IGS_ANCHOR_MAX_POINTS);
    if (x.device() != y.device()) throw RasterizerError("anchors_knn: x and y must be on one device");
    if (k < 1 || k > IGS_KNN_QUERY_MAX_K) throw RasterizerError("anchors_knn: k must be in [1, " + std::to_string(IGS_KNN_QUERY_MAX_K) + "] (got " + std::to_string(k) + ")");
    const int64_t B = ptr_x.dim() == 1 ? ptr_x.size(0) - 1 : -1;
    if (B < 1 || B > IGS_ANCHOR_MAX_EXAMPLES) throw RasterizerError("anchors_knn: ptr_x must have shape [B + 1], 1 <= B <= IGS_ANCHOR_MAX_EXAMPLES");
    const GpuCall c(x, fn, "x");
    const Tensor px = offsets_i32(ptr_x, fn, "ptr_x", x, B + 1), py = offsets_i32(ptr_y, fn, "ptr_y", x, B + 1);
    const Tensor xc = x.contiguous(), yc = y.contiguous();
    const int64_t Ny = y.size(0);
    Tensor idx = at::empty({Ny, k}, x.options().dtype(at::kLong));
    OptTensor d2, w;
    if (with_d2) d2 = at::empty({Ny, k}, x.options());
    if (weight_scale) w = at::empty({Ny, k}, x.options());
    if (Ny == 0) return {idx, d2, w};
    check(igs_knn_query(c.stream(), (int)B, (int)x.size(0), (int)Ny, xc.data_ptr<float>(), yc.data_ptr<float>(), px.data_ptr<int>(),
                        py.data_ptr<int>(), (int)k, weight_scale ? (float)*weight_scale : 0.f, idx.data_ptr<int64_t>(),
                        ptr_or_null<float>(d2), ptr_or_null<float>(w)), "igs_knn_query");
    return {idx, d2, w};
}

// ---- anchor feature interpolation (motion.hip; contracts in include/igs_rast.h) ----
// out [N, D] float32 = sum_k w[n, k] * F[col[n, k]]: F [A_total, D] float32 / float16, col [N, K] int64, w [N, K] float32
Tensor motion_interp_fwd(const Tensor& F, const Tensor& col, const Tensor& w)
{
    const char* fn = "motion_interp_fwd";
    const int dt = dtype_code(F, fn, "features");
    if (F.dim() != 2) throw RasterizerError(std::string(fn) + ": features must have shape [A_total, D] (got " + c10::str(F.sizes()) + ")");
    expect(col, fn, "col", at::kLong, {-1, -1});
    expect(w, fn, "weights", at::kFloat, {col.size(0), col.size(1)});
    const int64_t N = col.size(0), K = col.size(1), A = F.size(0), D = F.size(1);
    if (K < 1 || K > IGS_INTERP_MAX_K || D < 1 || D > IGS_INTERP_MAX_D || A < 1 || A > IGS_INTERP_MAX_ANCHORS || N > IGS_INTERP_MAX_ROWS ||
        N * K > IGS_INTERP_MAX_EDGES)
        throw RasterizerError(std::string(fn) + ": sizes out of range (1 <= K <= 100, 1 <= D <= 1024, 1 <= A_total <= 2^24, N <= 2^24, N * K <= 2^30)");
    const GpuCall c(F, fn, "features", {{col, "col"}, {w, "weights"}});
    Tensor out = at::empty({N, D}, F.options().dtype(at::kFloat));
    if (N == 0) return out;
    const Tensor Fc = F.contiguous(), cc = col.contiguous(), wc = w.contiguous();
    check(igs_anchor_interp_fwd(c.stream(), (int)N, (int)K, (int)D, (int)A, dt, Fc.data_ptr(), cc.data_ptr<int64_t>(), wc.data_ptr<float>(),
                                out.data_ptr<float>()), "igs_anchor_interp_fwd");
    return out;
}

// the inverse index of col (and room for the backward's partials at width D): a uint8 tensor to hand to motion_interp_bwd
Tensor motion_interp_index(const Tensor& col, int64_t A, int64_t D)
{
    const char* fn = "motion_interp_index";
    expect(col, fn, "col", at::kLong, {-1, -1});
    const int64_t N = col.size(0), K = col.size(1);
    const size_t bytes = (N <= INT_MAX && K <= INT_MAX && A <= INT_MAX && D <= INT_MAX) ? igs_anchor_interp_index_bytes((int)N, (int)K, (int)A, (int)D) : 0;
    if (bytes == 0) throw RasterizerError(std::string(fn) + ": sizes out of range");
    const GpuCall c(col, fn, "col");
    Tensor scratch = at::empty({(int64_t)bytes}, col.options().dtype(at::kByte));
    const Tensor cc = col.contiguous();
    check(igs_anchor_interp_index(c.stream(), (int)N, (int)K, (int)A, (int)D, cc.data_ptr<int64_t>(), scratch.data_ptr()), "igs_anchor_interp_index");
    return scratch;
}

// (dF [A_total, D] in F's dtype or None, dw [N, K] float32 or None) from the index of motion_interp_index
std::tuple<OptTensor, OptTensor> motion_interp_bwd(const Tensor& F, const Tensor& w, const Tensor& dout, const Tensor& index, bool want_dF,
                                                   bool want_dw)
{
    const char* fn = "motion_interp_bwd";
    const int dt = dtype_code(F, fn, "features");
    if (F.dim() != 2) throw RasterizerError(std::string(fn) + ": features must have shape [A_total, D] (got " + c10::str(F.sizes()) + ")");
    expect(w, fn, "weights", at::kFloat, {-1, -1});
    const int64_t N = w.size(0), K = w.size(1), A = F.size(0), D = F.size(1);
    expect(dout, fn, "grad_out", at::kFloat, {N, D});
    expect(index, fn, "index", at::kByte, {-1});
    const GpuCall c(F, fn, "features", {{w, "weights"}, {dout, "grad_out"}, {index, "index"}});
    const size_t need = igs_anchor_interp_index_bytes((int)N, (int)K, (int)A, (int)D);
    if (need == 0 || (size_t)index.numel() < need) throw RasterizerError(std::string(fn) + ": index too small for these sizes (or sizes out of range)");
    OptTensor dF, dw;
    if (want_dF) dF = at::empty({A, D}, F.options());
    if (want_dw) dw = at::empty({N, K}, w.options());
    const Tensor Fc = F.contiguous(), wc = w.contiguous(), gc = dout.contiguous();
    check(igs_anchor_interp_bwd(c.stream(), (int)N, (int)K, (int)D, (int)A, dt, Fc.data_ptr(), wc.data_ptr<float>(), gc.data_ptr<float>(),
                                index.data_ptr(), ptr_or_null(dF), ptr_or_null<float>(dw)), "igs_anchor_interp_bwd");
    return {dF, dw};
}

// ---- multi-view anchor feature lifting (lift.hip) ----
struct LiftSizes { int64_t B, V, A, C, H, W; };
LiftSizes lift_check(const char* fn, const Tensor& points, const Tensor& w2c, const Tensor& intr, int64_t C, int64_t H, int64_t W, int dt)
{
    expect(points, fn, "anchor_points", at::kFloat, {-1, -1, 3});
    expect(w2c, fn, "w2c", at::kFloat, {-1, 4, 4});
    expect(intr, fn, "intrinsics", at::kFloat, {w2c.size(0), 4});
    const int64_t B = points.size(0), A = points.size(1), BV = w2c.size(0);
    if (B < 1 || BV % B != 0 || BV / B < 1)
        throw RasterizerError(std::string(fn) + ": " + std::to_string(BV) + " views do not divide into " + std::to_string(B) + " examples");
    const int64_t V = BV / B;
    if (B > INT_MAX || A > INT_MAX || C > INT_MAX || H > INT_MAX || W > INT_MAX || V > INT_MAX ||
        igs_anchor_lift_scratch_bytes((int)B, (int)V, (int)A, (int)C, (int)H, (int)W, dt) == 0)
        throw RasterizerError(std::string(fn) + ": sizes out of range (C <= 1024, V <= 16, H, W <= 2048, B * V * H * W <= 2^24, B * A <= 2^24)");
    return {B, V, A, C, H, W};
}
// out [B, C, A] float32 (the caller views it as [B, A, C]): feat [B*V, C, H, W] float32 / float16 with contiguous H x W planes,
// points [B, A, 3], w2c [B*V, 4, 4], intr [B*V, 4] = fx, fy, cx, cy (float32)
Tensor motion_lift_fwd(const Tensor& feat, const Tensor& points, const Tensor& w2c, const Tensor& intr)
{
    const char* fn = "motion_lift_fwd";
    const int dt = dtype_code(feat, fn, "motion_feature");
    if (feat.dim() != 4) throw RasterizerError(std::string(fn) + ": motion_feature must have shape [B*V, C, H, W] (got " + c10::str(feat.sizes()) + ")");
    if (feat.size(0) != w2c.size(0))
        throw RasterizerError(std::string(fn) + ": motion_feature has shape " + c10::str(feat.sizes()) + " for " + std::to_string(w2c.size(0)) + " views");
    const LiftSizes z = lift_check(fn, points, w2c, intr, feat.size(1), feat.size(2), feat.size(3), dt);
    const GpuCall c(feat, fn, "motion_feature", {{points, "anchor_points"}, {w2c, "w2c"}, {intr, "intrinsics"}});
    Tensor out = at::empty({z.B, z.C, z.A}, feat.options().dtype(at::kFloat));
    if (z.A == 0) return out;
    Tensor scratch = at::empty({(int64_t)igs_anchor_lift_scratch_bytes((int)z.B, (int)z.V, (int)z.A, (int)z.C, (int)z.H, (int)z.W, dt)},
                               feat.options().dtype(at::kByte));
    const Tensor pc = points.contiguous(), wc = w2c.contiguous(), ic = intr.contiguous();
    check(igs_anchor_lift_fwd(c.stream(), (int)z.B, (int)z.V, (int)z.A, (int)z.C, (int)z.H, (int)z.W, dt, feat.data_ptr(), feat.stride(0),
                              feat.stride(1), feat.stride(2), feat.stride(3), pc.data_ptr<float>(), wc.data_ptr<float>(), ic.data_ptr<float>(),
                              out.data_ptr<float>(), 1, z.A, scratch.data_ptr()), "igs_anchor_lift_fwd");
    return out;
}

// d motion_feature [B*V, C, H, W] contiguous, float16 when `half`, from grad_bca = d out viewed [B, C, A] (any strides; read in place when
// it is [B, C, A]- or [B, A, C]-contiguous).  Every element is written.
Tensor motion_lift_bwd(const Tensor& grad_bca, const Tensor& points, const Tensor& w2c, const Tensor& intr, int64_t H, int64_t W, bool half)
{
    const char* fn = "motion_lift_bwd";
    const int dt = half ? IGS_DTYPE_F16 : IGS_DTYPE_F32;
    expect(grad_bca, fn, "grad_out", at::kFloat, {-1, -1, -1});
    const LiftSizes z = lift_check(fn, points, w2c, intr, grad_bca.size(1), H, W, dt);
    if (grad_bca.size(0) != z.B || grad_bca.size(2) != z.A)
        throw RasterizerError(std::string(fn) + ": grad_out has shape " + c10::str(grad_bca.sizes()) + ", expected [B, C, A]");
    const GpuCall c(grad_bca, fn, "grad_out", {{points, "anchor_points"}, {w2c, "w2c"}, {intr, "intrinsics"}});
    Tensor dfeat = at::empty({z.B * z.V, z.C, z.H, z.W}, grad_bca.options().dtype(half ? at::kHalf : at::kFloat));
    const bool bac = grad_bca.stride(0) == z.A * z.C && grad_bca.stride(1) == 1 && grad_bca.stride(2) == z.C;      // [B, A, C]-contiguous
    const Tensor g = (bac || z.A == 0) ? grad_bca : grad_bca.contiguous();
    const size_t bytes = igs_anchor_lift_bwd_scratch_bytes((int)z.B, (int)z.V, (int)z.A, (int)z.C, (int)z.H, (int)z.W, dt);
    Tensor scratch = at::empty({z.A == 0 ? 0 : (int64_t)bytes}, grad_bca.options().dtype(at::kByte));
    const Tensor pc = points.contiguous(), wc = w2c.contiguous(), ic = intr.contiguous();
    check(igs_anchor_lift_bwd(c.stream(), (int)z.B, (int)z.V, (int)z.A, (int)z.C, (int)z.H, (int)z.W, dt, pc.data_ptr<float>(),
                              wc.data_ptr<float>(), ic.data_ptr<float>(), g.data_ptr<float>(), bac ? z.C : 1, bac ? 1 : z.A, dfeat.data_ptr(),
                              z.C * z.H * z.W, z.H * z.W, z.W, 1, scratch.data_ptr()), "igs_anchor_lift_bwd");
    return dfeat;
}

// ---- ray conditioning and fused LayerNorm + modulation (cond.hip) ----
// cond [N, H, W, 33] float32 from rays [N, H, W, 6] and depth [N, Hd, Wd] (float32; N = B * V views)
Tensor cond_ray_fwd(const Tensor& rays, const Tensor& depth)
{
    const char* fn = "cond_ray_fwd";
    expect(rays, fn, "rays", at::kFloat, {-1, -1, -1, 6});
    expect(depth, fn, "depth", at::kFloat, {rays.size(0), -1, -1});
    const int64_t N = rays.size(0), H = rays.size(1), W = rays.size(2), Hd = depth.size(1), Wd = depth.size(2);
    if (H < 1 || W < 1 || Hd < 1 || Wd < 1 || H > IGS_COND_MAX_HW || W > IGS_COND_MAX_HW || Hd > IGS_COND_MAX_HW || Wd > IGS_COND_MAX_HW ||
        N * H * W > IGS_COND_MAX_PIXELS)
        throw RasterizerError(std::string(fn) + ": sizes out of range (1 <= H, W, Hd, Wd <= 8192, N * H * W <= 2^24)");
    const GpuCall c(rays, fn, "rays", {{depth, "depth"}});
    Tensor cond = at::empty({N, H, W, 33}, rays.options());
    const Tensor rc = rays.contiguous(), dc = depth.contiguous();
    check(igs_ray_condition_fwd(c.stream(), (int)N, (int)H, (int)W, (int)Hd, (int)Wd, rc.data_ptr<float>(), dc.data_ptr<float>(),
                                cond.data_ptr<float>()), "igs_ray_condition_fwd");
    return cond;
}

struct ModlnSizes { int64_t N, C, H, W; int xdt, mdt; };
ModlnSizes modln_check(const char* fn, const Tensor& x, const Tensor& mod, const Tensor& weight, const Tensor& bias)
{
    ModlnSizes z;
    z.xdt = dtype_code(x, fn, "x");
    z.mdt = dtype_code(mod, fn, "mod");
    if (x.dim() != 4) throw RasterizerError(std::string(fn) + ": x must have shape [N, C, H, W] (got " + c10::str(x.sizes()) + ")");
    z.N = x.size(0); z.C = x.size(1); z.H = x.size(2); z.W = x.size(3);
    expect(mod, fn, "mod", mod.scalar_type(), {z.N, z.H, z.W, 2 * z.C});
    expect(weight, fn, "weight", at::kFloat, {z.C});
    expect(bias, fn, "bias", at::kFloat, {z.C});
    if (z.C < 1 || z.C > IGS_MODLN_MAX_C || z.H < 1 || z.W < 1 || z.H > IGS_COND_MAX_HW || z.W > IGS_COND_MAX_HW ||
        z.N * z.H * z.W > IGS_COND_MAX_PIXELS)
        throw RasterizerError(std::string(fn) + ": sizes out of range (1 <= C <= 1024, 1 <= H, W <= 8192, N * H * W <= 2^24)");
    return z;
}
// (out [N, C, H, W] float32 contiguous, mean, rstd [N, H, W] float32 or None): x [N, C, H, W] float32 / float16 with contiguous H x W
// planes, mod [N, H, W, 2 C] float32 / float16, weight, bias [C] float32
std::tuple<Tensor, OptTensor, OptTensor> modln_fwd(const Tensor& x, const Tensor& mod, const Tensor& weight, const Tensor& bias, double eps,
                                                    bool save_stats)
{
    const char* fn = "modln_fwd";
    const ModlnSizes z = modln_check(fn, x, mod, weight, bias);
    const GpuCall c(x, fn, "x", {{mod, "mod"}, {weight, "weight"}, {bias, "bias"}});
    const auto fo = x.options().dtype(at::kFloat);
    Tensor out = at::empty({z.N, z.C, z.H, z.W}, fo);
    OptTensor mean, rstd;
    if (save_stats) { mean = at::empty({z.N, z.H, z.W}, fo); rstd = at::empty({z.N, z.H, z.W}, fo); }
    if (z.N == 0) return {out, mean, rstd};
    const Tensor mc = mod.contiguous(), wc = weight.contiguous(), bc = bias.contiguous();
    check(igs_modln_fwd(c.stream(), (int)z.N, (int)z.C, (int)z.H, (int)z.W, z.xdt, x.data_ptr(), x.stride(0), x.stride(1), x.stride(2),
                        x.stride(3), z.mdt, mc.data_ptr(), wc.data_ptr<float>(), bc.data_ptr<float>(), (float)eps, out.data_ptr<float>(),
                        ptr_or_null<float>(mean), ptr_or_null<float>(rstd)), "igs_modln_fwd");
    return {out, mean, rstd};
}

// (d x in x's dtype, d mod in mod's dtype, d weight, d bias), each None unless wanted
std::tuple<OptTensor, OptTensor, OptTensor, OptTensor> modln_bwd(const Tensor& x, const Tensor& mod, const Tensor& weight, const Tensor& bias,
                                                                  const Tensor& mean, const Tensor& rstd, const Tensor& grad_out, bool want_x,
                                                                  bool want_mod, bool want_weight, bool want_bias)
{
    const char* fn = "modln_bwd";
    const ModlnSizes z = modln_check(fn, x, mod, weight, bias);
    expect(mean, fn, "mean", at::kFloat, {z.N, z.H, z.W});
    expect(rstd, fn, "rstd", at::kFloat, {z.N, z.H, z.W});
    expect(grad_out, fn, "grad_out", at::kFloat, {z.N, z.C, z.H, z.W});
    const GpuCall c(x, fn, "x", {{mod, "mod"}, {weight, "weight"}, {bias, "bias"}, {mean, "mean"}, {rstd, "rstd"}, {grad_out, "grad_out"}});
    OptTensor dx, dmod, dw, db, scratch;
    const auto fo = x.options().dtype(at::kFloat);
    if (want_x) dx = at::empty({z.N, z.C, z.H, z.W}, x.options());
    if (want_mod) dmod = at::empty({z.N, z.H, z.W, 2 * z.C}, mod.options());
    if (want_weight) dw = z.N == 0 ? at::zeros({z.C}, fo) : at::empty({z.C}, fo);
    if (want_bias) db = z.N == 0 ? at::zeros({z.C}, fo) : at::empty({z.C}, fo);
    if (z.N == 0 || !(want_x || want_mod || want_weight || want_bias)) return {dx, dmod, dw, db};
    if (want_weight || want_bias)
        scratch = at::empty({(int64_t)igs_modln_bwd_scratch_bytes((int)z.N, (int)z.C, (int)z.H, (int)z.W)}, x.options().dtype(at::kByte));
    const Tensor mc = mod.contiguous(), wc = weight.contiguous(), bc = bias.contiguous(), mu = mean.contiguous(), rs = rstd.contiguous(),
                 gc = grad_out.contiguous();
    check(igs_modln_bwd(c.stream(), (int)z.N, (int)z.C, (int)z.H, (int)z.W, z.xdt, x.data_ptr(), x.stride(0), x.stride(1), x.stride(2),
                        x.stride(3), z.mdt, mc.data_ptr(), wc.data_ptr<float>(), bc.data_ptr<float>(), mu.data_ptr<float>(), rs.data_ptr<float>(),
                        gc.data_ptr<float>(), ptr_or_null(dx), ptr_or_null(dmod), ptr_or_null<float>(dw), ptr_or_null<float>(db),
                        ptr_or_null(scratch)), "igs_modln_bwd");
    return {dx, dmod, dw, db};
}

// ---- condition3D in one launch (cond_fused.hip) ----
int64_t cond_fused_pack_elems(int64_t C, int64_t hidden, bool half)
{
    return igs_condition3d_pack_elems((int)C, (int)hidden, half ? IGS_DTYPE_F16 : IGS_DTYPE_F32);
}
// out [N, C, H, W] float32 contiguous.  x [N, C, H, W] float32 / float16 with contiguous H x W planes, rays [N, H, W, 6] and depth
// [N, Hd, Wd] float32, wpack (float32 or float16: the MLP instance) and bpack [3, 128] as igs_condition3d_fwd takes them
// (igs_amd/motion.py packs and caches them), weight, bias [C] float32: the LayerNorm's
Tensor condition3d_fwd(const Tensor& x, const Tensor& rays, const Tensor& depth, const Tensor& wpack, const Tensor& bpack, int64_t hidden,
                       const Tensor& weight, const Tensor& bias, double eps)
{
    const char* fn = "condition3d_fwd";
    const int xdt = dtype_code(x, fn, "x"), mdt = dtype_code(wpack, fn, "wpack");
    if (x.dim() != 4) throw RasterizerError(std::string(fn) + ": x must have shape [N, C, H, W] (got " + c10::str(x.sizes()) + ")");
    const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
    expect(rays, fn, "rays", at::kFloat, {N, H, W, 6});
    expect(depth, fn, "depth", at::kFloat, {N, -1, -1});
    expect(weight, fn, "weight", at::kFloat, {C});
    expect(bias, fn, "bias", at::kFloat, {C});
    const int64_t Hd = depth.size(1), Wd = depth.size(2);
    if (H < 1 || W < 1 || Hd < 1 || Wd < 1 || H > IGS_COND_MAX_HW || W > IGS_COND_MAX_HW || Hd > IGS_COND_MAX_HW || Wd > IGS_COND_MAX_HW ||
        N * H * W > IGS_COND_MAX_PIXELS)
        throw RasterizerError(std::string(fn) + ": sizes out of range (1 <= H, W, Hd, Wd <= 8192, N * H * W <= 2^24)");
    const int64_t elems = C >= 1 && C <= INT_MAX && hidden >= 1 && hidden <= INT_MAX ? igs_condition3d_pack_elems((int)C, (int)hidden, mdt) : -1;
    if (elems < 0) throw RasterizerError(std::string(fn) + ": C and hidden must be in 1..128 (got " + std::to_string(C) + ", " + std::to_string(hidden) + ")");
    expect(wpack, fn, "wpack", wpack.scalar_type(), {elems});
    expect(bpack, fn, "bpack", at::kFloat, {3, IGS_COND_MLP_MAX_WIDTH});
    if (!wpack.is_contiguous() || !bpack.is_contiguous()) throw RasterizerError(std::string(fn) + ": wpack and bpack must be contiguous");
    const GpuCall c(x, fn, "x", {{rays, "rays"}, {depth, "depth"}, {wpack, "wpack"}, {bpack, "bpack"}, {weight, "weight"}, {bias, "bias"}});
    Tensor out = at::empty({N, C, H, W}, x.options().dtype(at::kFloat));
    if (N == 0) return out;
    const Tensor rc = rays.contiguous(), dc = depth.contiguous(), wc = weight.contiguous(), bc = bias.contiguous();
    check(igs_condition3d_fwd(c.stream(), (int)N, (int)C, (int)hidden, (int)H, (int)W, (int)Hd, (int)Wd, xdt, x.data_ptr(), x.stride(0), x.stride(1),
                              x.stride(2), x.stride(3), rc.data_ptr<float>(), dc.data_ptr<float>(), mdt, wpack.data_ptr(), bpack.data_ptr<float>(),
                              wc.data_ptr<float>(), bc.data_ptr<float>(), (float)eps, out.data_ptr<float>()), "igs_condition3d_fwd");
    return out;
}
int64_t cond_fused_bwd_scratch_bytes(int64_t N, int64_t C, int64_t hidden, int64_t H, int64_t W)
{
    if (N < 0 || N > INT_MAX || C < 1 || C > INT_MAX || hidden < 1 || hidden > INT_MAX || H < 1 || H > INT_MAX || W < 1 || W > INT_MAX) return -1;
    return igs_condition3d_bwd_scratch_bytes((int)N, (int)C, (int)hidden, (int)H, (int)W);
}
// (d x [N, C, H, W] in x's dtype, d W1 [hidden, 33], d b1 [hidden], d W2 [2C, hidden], d b2 [2C], d weight [C], d bias [C] float32), each None
// unless wanted.  The inputs of condition3d_fwd, wpack_t as igs_condition3d_bwd takes it, and grad_out [N, C, H, W] float32 contiguous
std::tuple<OptTensor, OptTensor, OptTensor, OptTensor, OptTensor, OptTensor, OptTensor>
condition3d_bwd(const Tensor& x, const Tensor& rays, const Tensor& depth, const Tensor& wpack, const Tensor& wpack_t, const Tensor& bpack, int64_t hidden,
                const Tensor& weight, const Tensor& bias, double eps, const Tensor& grad_out, bool want_x, bool want_w1, bool want_b1, bool want_w2,
                bool want_b2, bool want_weight, bool want_bias)
{
    const char* fn = "condition3d_bwd";
    const int xdt = dtype_code(x, fn, "x"), mdt = dtype_code(wpack, fn, "wpack");
    if (x.dim() != 4) throw RasterizerError(std::string(fn) + ": x must have shape [N, C, H, W] (got " + c10::str(x.sizes()) + ")");
    const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
    expect(rays, fn, "rays", at::kFloat, {N, H, W, 6});
    expect(depth, fn, "depth", at::kFloat, {N, -1, -1});
    expect(weight, fn, "weight", at::kFloat, {C});
    expect(bias, fn, "bias", at::kFloat, {C});
    expect(grad_out, fn, "grad_out", at::kFloat, {N, C, H, W});
    const int64_t Hd = depth.size(1), Wd = depth.size(2);
    if (H < 1 || W < 1 || Hd < 1 || Wd < 1 || H > IGS_COND_MAX_HW || W > IGS_COND_MAX_HW || Hd > IGS_COND_MAX_HW || Wd > IGS_COND_MAX_HW ||
        N * H * W > IGS_COND_MAX_PIXELS)
        throw RasterizerError(std::string(fn) + ": sizes out of range (1 <= H, W, Hd, Wd <= 8192, N * H * W <= 2^24)");
    const int64_t elems = C >= 1 && C <= INT_MAX && hidden >= 1 && hidden <= INT_MAX ? igs_condition3d_pack_elems((int)C, (int)hidden, mdt) : -1;
    if (elems < 0) throw RasterizerError(std::string(fn) + ": C and hidden must be in 1..128 (got " + std::to_string(C) + ", " + std::to_string(hidden) + ")");
    const int64_t ht = (hidden + 31) / 32, ct = (C + 31) / 32;
    expect(wpack, fn, "wpack", wpack.scalar_type(), {elems});
    expect(wpack_t, fn, "wpack_t", wpack.scalar_type(), {2 * ct * ht * 1024});
    expect(bpack, fn, "bpack", at::kFloat, {3, IGS_COND_MLP_MAX_WIDTH});
    if (!wpack.is_contiguous() || !wpack_t.is_contiguous() || !bpack.is_contiguous() || !grad_out.is_contiguous())
        throw RasterizerError(std::string(fn) + ": wpack, wpack_t, bpack and grad_out must be contiguous");
    const GpuCall c(x, fn, "x", {{rays, "rays"}, {depth, "depth"}, {wpack, "wpack"}, {wpack_t, "wpack_t"}, {bpack, "bpack"}, {weight, "weight"},
                                 {bias, "bias"}, {grad_out, "grad_out"}});
    OptTensor dx, dw1, db1, dw2, db2, dnw, dnb;
    const auto fo = x.options().dtype(at::kFloat);
    const bool empty = N == 0;                                   // (no pixel: the sums are zero and nothing is launched)
    auto make = [&](at::IntArrayRef shape) { return empty ? at::zeros(shape, fo) : at::empty(shape, fo); };
    if (want_x) dx = at::empty({N, C, H, W}, x.options());
    if (want_w1) dw1 = make({hidden, 33});
    if (want_b1) db1 = make({hidden});
    if (want_w2) dw2 = make({2 * C, hidden});
    if (want_b2) db2 = make({2 * C});
    if (want_weight) dnw = make({C});
    if (want_bias) dnb = make({C});
    if (empty || !(want_x || want_w1 || want_b1 || want_w2 || want_b2 || want_weight || want_bias)) return {dx, dw1, db1, dw2, db2, dnw, dnb};
    const Tensor rc = rays.contiguous(), dc = depth.contiguous(), wc = weight.contiguous(), bc = bias.contiguous();
    const Tensor scratch = at::empty({igs_condition3d_bwd_scratch_bytes((int)N, (int)C, (int)hidden, (int)H, (int)W)}, x.options().dtype(at::kByte));
    check(igs_condition3d_bwd(c.stream(), (int)N, (int)C, (int)hidden, (int)H, (int)W, (int)Hd, (int)Wd, xdt, x.data_ptr(), x.stride(0), x.stride(1),
                              x.stride(2), x.stride(3), rc.data_ptr<float>(), dc.data_ptr<float>(), mdt, wpack.data_ptr(), wpack_t.data_ptr(),
                              bpack.data_ptr<float>(), wc.data_ptr<float>(), bc.data_ptr<float>(), (float)eps, grad_out.data_ptr<float>(),
                              scratch.data_ptr(), scratch.numel(), ptr_or_null(dx), ptr_or_null<float>(dw1), ptr_or_null<float>(db1),
                              ptr_or_null<float>(dw2), ptr_or_null<float>(db2), ptr_or_null<float>(dnw), ptr_or_null<float>(dnb)),
          "igs_condition3d_bwd");
    return {dx, dw1, db1, dw2, db2, dnw, dnb};
}

// ---- 2x bilinear upsample + 3x3 convolution in one launch (upconv.hip) ----
int64_t upconv_pack_elems(int64_t Cin, int64_t Cout, bool half)
{
    if (Cin < 1 || Cin > INT_MAX || Cout < 1 || Cout > INT_MAX) return -1;
    return igs_upconv_pack_elems((int)Cin, (int)Cout, half ? IGS_DTYPE_F16 : IGS_DTYPE_F32);
}
// out [N, Cout, 2H, 2W] contiguous in wpack's dtype (the compute dtype).  x [N, Cin, H, W] float32 / float16 with contiguous H x W planes,
// wpack and bpack [128] as igs_upconv_fwd takes them (igs_amd/motion.py packs and caches them)
Tensor upconv_fwd(const Tensor& x, const Tensor& wpack, const Tensor& bpack, int64_t Cout)
{
    const char* fn = "upconv_fwd";
    const int xdt = dtype_code(x, fn, "x"), cdt = dtype_code(wpack, fn, "wpack");
    if (x.dim() != 4) throw RasterizerError(std::string(fn) + ": x must have shape [N, Cin, H, W] (got " + c10::str(x.sizes()) + ")");
    const int64_t N = x.size(0), Cin = x.size(1), H = x.size(2), W = x.size(3);
    if (H < 1 || W < 1 || H > IGS_UPCONV_MAX_HW || W > IGS_UPCONV_MAX_HW || N * H * W > IGS_UPCONV_MAX_PIXELS)
        throw RasterizerError(std::string(fn) + ": sizes out of range (1 <= H, W <= 4096, N * H * W <= 2^22)");
    const int64_t elems = upconv_pack_elems(Cin, Cout, cdt == IGS_DTYPE_F16);
    if (elems < 0) throw RasterizerError(std::string(fn) + ": Cin and Cout must be in 1..128 (got " + std::to_string(Cin) + ", " + std::to_string(Cout) + ")");
    expect(wpack, fn, "wpack", wpack.scalar_type(), {elems});
    expect(bpack, fn, "bpack", at::kFloat, {IGS_UPCONV_MAX_WIDTH});
    if (!wpack.is_contiguous() || !bpack.is_contiguous()) throw RasterizerError(std::string(fn) + ": wpack and bpack must be contiguous");
    const GpuCall c(x, fn, "x", {{wpack, "wpack"}, {bpack, "bpack"}});
    Tensor out = at::empty({N, Cout, 2 * H, 2 * W}, x.options().dtype(wpack.scalar_type()));
    if (N == 0) return out;
    check(igs_upconv_fwd(c.stream(), (int)N, (int)Cin, (int)Cout, (int)H, (int)W, xdt, x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), x.stride(3),
                         cdt, wpack.data_ptr(), bpack.data_ptr<float>(), out.data_ptr()), "igs_upconv_fwd");
    return out;
}
// (d x [N, Cin, H, W] in x's dtype, d weight [Cout, Cin, 3, 3] and d bias [Cout] float32), each None unless wanted.  dout [N, Cout, 2H, 2W]
// contiguous in wpack_t's dtype (the compute dtype); wpack_t: the transposed, flipped convolution packed like wpack (igs_upconv_bwd)
std::tuple<OptTensor, OptTensor, OptTensor> upconv_bwd(const Tensor& x, const Tensor& wpack_t, const Tensor& dout, bool want_x, bool want_w, bool want_b)
{
    const char* fn = "upconv_bwd";
    const int xdt = dtype_code(x, fn, "x"), cdt = dtype_code(wpack_t, fn, "wpack_t");
    if (x.dim() != 4) throw RasterizerError(std::string(fn) + ": x must have shape [N, Cin, H, W] (got " + c10::str(x.sizes()) + ")");
    if (dout.dim() != 4) throw RasterizerError(std::string(fn) + ": dout must have shape [N, Cout, 2H, 2W] (got " + c10::str(dout.sizes()) + ")");
    const int64_t N = x.size(0), Cin = x.size(1), H = x.size(2), W = x.size(3), Cout = dout.size(1);
    if (H < 1 || W < 1 || H > IGS_UPCONV_MAX_HW || W > IGS_UPCONV_MAX_HW || N * H * W > IGS_UPCONV_MAX_PIXELS)
        throw RasterizerError(std::string(fn) + ": sizes out of range (1 <= H, W <= 4096, N * H * W <= 2^22)");
    const int64_t elems = upconv_pack_elems(Cout, Cin, cdt == IGS_DTYPE_F16);
    if (elems < 0) throw RasterizerError(std::string(fn) + ": Cin and Cout must be in 1..128 (got " + std::to_string(Cin) + ", " + std::to_string(Cout) + ")");
    expect(wpack_t, fn, "wpack_t", wpack_t.scalar_type(), {elems});
    expect(dout, fn, "dout", wpack_t.scalar_type(), {N, Cout, 2 * H, 2 * W});
    if (!wpack_t.is_contiguous() || !dout.is_contiguous()) throw RasterizerError(std::string(fn) + ": wpack_t and dout must be contiguous");
    const GpuCall c(x, fn, "x", {{wpack_t, "wpack_t"}, {dout, "dout"}});
    OptTensor dx, dw, db;
    const auto fo = x.options().dtype(at::kFloat);
    if (want_x) dx = at::empty({N, Cin, H, W}, x.options());
    if (want_w) dw = at::empty({Cout, Cin, 3, 3}, fo);
    if (want_b) db = at::empty({Cout}, fo);
    if (!(want_x || want_w || want_b)) return {dx, dw, db};
    const Tensor scratch = at::empty({igs_upconv_bwd_scratch_bytes((int)N, (int)Cin, (int)Cout, (int)H, (int)W, cdt)}, x.options().dtype(at::kByte));
    check(igs_upconv_bwd(c.stream(), (int)N, (int)Cin, (int)Cout, (int)H, (int)W, xdt, x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), x.stride(3),
                         cdt, wpack_t.data_ptr(), dout.data_ptr(), scratch.data_ptr(), scratch.numel(), ptr_or_null(dx), ptr_or_null<float>(dw),
                         ptr_or_null<float>(db)), "igs_upconv_bwd");
    return {dx, dw, db};
}

// ---- fused attention for the anchor transformer (attn.hip; contract in include/igs_rast.h) ----
struct AttnSizes { int64_t B, H, Aq, Ak; int dt; };
void attn_view_check(const char* fn, const Tensor& t, const char* name, const Tensor& like, int64_t B, int64_t H, int64_t A)
{
    if (t.dim() != 4 || t.size(0) != B || t.size(1) != H || t.size(2) != A || t.size(3) != 64)
        throw RasterizerError(std::string(fn) + ": " + name + " has shape " + c10::str(t.sizes()) + ", expected " +
                              c10::str(at::IntArrayRef({B, H, A, (int64_t)64})));
    if (t.scalar_type() != like.scalar_type()) throw NotImplemented(std::string(fn) + ": " + name + " must have q's dtype");
    if (t.stride(3) != 1) throw RasterizerError(std::string(fn) + ": " + name + " must have stride 1 on its last dimension");
}
AttnSizes attn_check(const char* fn, const Tensor& q, const Tensor& k, const Tensor& v)
{
    AttnSizes z;
    z.dt = dtype_code(q, fn, "q");
    if (q.dim() != 4 || k.dim() != 4 || v.dim() != 4)
        throw RasterizerError(std::string(fn) + ": q, k, v must be [B, H, A, D] views (got " + c10::str(q.sizes()) + ", " + c10::str(k.sizes()) +
                              ", " + c10::str(v.sizes()) + ")");
    if (q.size(3) != 64) throw NotImplemented(std::string(fn) + ": the head size must be 64 (got " + std::to_string(q.size(3)) + ")");
    z.B = q.size(0); z.H = q.size(1); z.Aq = q.size(2); z.Ak = k.size(2);
    attn_view_check(fn, q, "q", q, z.B, z.H, z.Aq);
    attn_view_check(fn, k, "k", q, z.B, z.H, z.Ak);
    attn_view_check(fn, v, "v", q, z.B, z.H, z.Ak);
    if (z.Aq < 1 || z.Ak < 1 || z.Aq > IGS_ATTN_MAX_TOKENS || z.Ak > IGS_ATTN_MAX_TOKENS || z.H < 1 || z.H > IGS_ATTN_MAX_HEADS ||
        z.B > IGS_ATTN_MAX_BATCH)
        throw RasterizerError(std::string(fn) + ": sizes out of range (B <= 65535, 1 <= H <= 1024, 1 <= Aq, Ak <= 2^20)");
    return z;
}
// [B, H, A, 64] as indexed; token-major ([B, A, H, 64] in memory) or head-major
Tensor attn_empty(const Tensor& like, int64_t B, int64_t H, int64_t A, bool token_major)
{
    return token_major ? at::empty({B, A, H, 64}, like.options()).permute({0, 2, 1, 3}) : at::empty({B, H, A, 64}, like.options());
}

// (out, lse or None): q [B, H, Aq, 64], k, v [B, H, Ak, 64] float32 / float16 views with stride 1 on the last dimension
std::tuple<Tensor, OptTensor> attn_fwd(const Tensor& q, const Tensor& k, const Tensor& v, double scale, bool token_major, bool want_lse)
{
    const char* fn = "attn_fwd";
    const AttnSizes z = attn_check(fn, q, k, v);
    const GpuCall c(q, fn, "q", {{k, "k"}, {v, "v"}});
    Tensor out = attn_empty(q, z.B, z.H, z.Aq, token_major);
    OptTensor lse;
    if (want_lse) lse = at::empty({z.B, z.H, z.Aq}, q.options().dtype(at::kFloat));
    if (z.B == 0) return {out, lse};
    const HeadView Q(q), K(k), V(v), O(out);
    check(igs_attn_fwd(c.stream(), (int)z.B, (int)z.H, (int)z.Aq, (int)z.Ak, 64, z.dt, Q.p, Q.sb, Q.sh, Q.sa, K.p, K.sb, K.sh, K.sa,
                       V.p, V.sb, V.sh, V.sa, (float)scale, O.p, O.sb, O.sh, O.sa, ptr_or_null<float>(lse)), "igs_attn_fwd");
    return {out, lse};
}

// (d q, d k, d v), each None unless wanted, laid out like attn_fwd's out
std::tuple<OptTensor, OptTensor, OptTensor> attn_bwd(const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& out, const Tensor& lse,
                                                     const Tensor& grad_out, double scale, bool token_major, bool want_q, bool want_k,
                                                     bool want_v)
{
    const char* fn = "attn_bwd";
    const AttnSizes z = attn_check(fn, q, k, v);
    attn_view_check(fn, out, "out", q, z.B, z.H, z.Aq);
    attn_view_check(fn, grad_out, "grad_out", q, z.B, z.H, z.Aq);
    expect(lse, fn, "lse", at::kFloat, {z.B, z.H, z.Aq});
    const GpuCall c(q, fn, "q", {{k, "k"}, {v, "v"}, {out, "out"}, {lse, "lse"}, {grad_out, "grad_out"}});
    OptTensor dq, dk, dv;
    if (want_q) dq = attn_empty(q, z.B, z.H, z.Aq, token_major);
    if (want_k) dk = attn_empty(q, z.B, z.H, z.Ak, token_major);
    if (want_v) dv = attn_empty(q, z.B, z.H, z.Ak, token_major);
    if (z.B == 0 || !(want_q || want_k || want_v)) return {dq, dk, dv};
    const Tensor ls = lse.contiguous();
    Tensor scratch = at::empty({(int64_t)igs_attn_bwd_scratch_bytes((int)z.B, (int)z.H, (int)z.Aq, (int)z.Ak, 64, z.dt)}, q.options().dtype(at::kByte));
    const HeadView Q(q), K(k), V(v), O(out), G(grad_out), DQ(dq), DK(dk), DV(dv);
    check(igs_attn_bwd(c.stream(), (int)z.B, (int)z.H, (int)z.Aq, (int)z.Ak, 64, z.dt, Q.p, Q.sb, Q.sh, Q.sa, K.p, K.sb, K.sh, K.sa,
                       V.p, V.sb, V.sh, V.sa, O.p, O.sb, O.sh, O.sa, ls.data_ptr<float>(), G.p, G.sb, G.sh, G.sa, (float)scale,
                       DQ.p, DQ.sb, DQ.sh, DQ.sa, DK.p, DK.sb, DK.sh, DK.sa, DV.p, DV.sb, DV.sh, DV.sa, scratch.data_ptr()), "igs_attn_bwd");
    return {dq, dk, dv};
}

// ---- swin window attention for the motion-feature transformers (wattn.hip; contract in include/igs_rast.h) ----
// a [B, L, 128] view as the window attention entry points take it: data pointer and the two outer strides (NULL and zeros when absent)
struct TokenView {
    void* p = nullptr; int64_t sb = 0, st = 0;
    TokenView(const Tensor& t) : p(t.data_ptr()), sb(t.stride(0)), st(t.stride(1)) {}
    TokenView(const OptTensor& t) { if (t) *this = TokenView(*t); }
};
struct WindowSizes { int64_t B, L; int dt; };
void window_view_check(const char* fn, const Tensor& t, const char* name, const Tensor& like, int64_t B, int64_t L)
{
    if (t.dim() != 3 || t.size(0) != B || t.size(1) != L || t.size(2) != 128)
        throw RasterizerError(std::string(fn) + ": " + name + " has shape " + c10::str(t.sizes()) + ", expected " +
                              c10::str(at::IntArrayRef({B, L, (int64_t)128})));
    if (t.scalar_type() != like.scalar_type()) throw NotImplemented(std::string(fn) + ": " + name + " must have q's dtype");
    if (t.stride(2) != 1) throw RasterizerError(std::string(fn) + ": " + name + " must have stride 1 on its last dimension");
}
WindowSizes window_check(const char* fn, const Tensor& q, const Tensor& k, const Tensor& v, int64_t h, int64_t w, int64_t K)
{
    WindowSizes z;
    z.dt = dtype_code(q, fn, "q");
    if (q.dim() != 3) throw RasterizerError(std::string(fn) + ": q, k, v must be [B, h * w, 128] views (got " + c10::str(q.sizes()) + ")");
    if (q.size(2) != 128) throw NotImplemented(std::string(fn) + ": the channel count must be 128 (got " + std::to_string(q.size(2)) + ")");
    z.B = q.size(0); z.L = q.size(1);
    if (h < 1 || w < 1 || K < 1 || h * w != z.L || h % K || w % K || z.B > IGS_WINDOW_ATTN_MAX_BATCH || z.B * z.L > ((int64_t)1 << 24))
        throw RasterizerError(std::string(fn) + ": sizes out of range (h * w = L, h % K = w % K = 0, B <= 65535, B * L <= 2^24; got h " +
                              std::to_string(h) + ", w " + std::to_string(w) + ", K " + std::to_string(K) + ", L " + std::to_string(z.L) + ")");
    window_view_check(fn, q, "q", q, z.B, z.L);
    window_view_check(fn, k, "k", q, z.B, z.L);
    window_view_check(fn, v, "v", q, z.B, z.L);
    return z;
}

// (out, lse or None): q, k, v [B, h * w, 128] float32 / float16 views with stride 1 on the last dimension; out contiguous
std::tuple<Tensor, OptTensor> window_attn_fwd(const Tensor& q, const Tensor& k, const Tensor& v, int64_t h, int64_t w, int64_t num_splits,
                                              bool with_shift, double scale, bool want_lse)
{
    const char* fn = "window_attn_fwd";
    const WindowSizes z = window_check(fn, q, k, v, h, w, num_splits);
    const GpuCall c(q, fn, "q", {{k, "k"}, {v, "v"}});
    Tensor out = at::empty({z.B, z.L, 128}, q.options());
    OptTensor lse;
    if (want_lse) lse = at::empty({z.B, z.L}, q.options().dtype(at::kFloat));
    if (z.B == 0) return {out, lse};
    const TokenView Q(q), K(k), V(v), O(out);
    check(igs_window_attn_fwd(c.stream(), (int)z.B, (int)h, (int)w, (int)num_splits, with_shift ? 1 : 0, 128, z.dt, Q.p, Q.sb, Q.st, K.p, K.sb,
                              K.st, V.p, V.sb, V.st, (float)scale, O.p, O.sb, O.st, ptr_or_null<float>(lse)), "igs_window_attn_fwd");
    return {out, lse};
}

// (d q, d k, d v), each None unless wanted, contiguous [B, h * w, 128]
std::tuple<OptTensor, OptTensor, OptTensor> window_attn_bwd(const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& out,
                                                            const Tensor& lse, const Tensor& grad_out, int64_t h, int64_t w,
                                                            int64_t num_splits, bool with_shift, double scale, bool want_q, bool want_k,
                                                            bool want_v)
{
    const char* fn = "window_attn_bwd";
    const WindowSizes z = window_check(fn, q, k, v, h, w, num_splits);
    window_view_check(fn, out, "out", q, z.B, z.L);
    window_view_check(fn, grad_out, "grad_out", q, z.B, z.L);
    expect(lse, fn, "lse", at::kFloat, {z.B, z.L});
    const GpuCall c(q, fn, "q", {{k, "k"}, {v, "v"}, {out, "out"}, {lse, "lse"}, {grad_out, "grad_out"}});
    OptTensor dq, dk, dv;
    if (want_q) dq = at::empty({z.B, z.L, 128}, q.options());
    if (want_k) dk = at::empty({z.B, z.L, 128}, q.options());
    if (want_v) dv = at::empty({z.B, z.L, 128}, q.options());
    if (z.B == 0 || !(want_q || want_k || want_v)) return {dq, dk, dv};
    const Tensor ls = lse.contiguous();
    Tensor scratch = at::empty({(int64_t)igs_window_attn_bwd_scratch_bytes((int)z.B, (int)h, (int)w, (int)num_splits, 128, z.dt)}, q.options().dtype(at::kByte));
    const TokenView Q(q), K(k), V(v), O(out), G(grad_out), DQ(dq), DK(dk), DV(dv);
    check(igs_window_attn_bwd(c.stream(), (int)z.B, (int)h, (int)w, (int)num_splits, with_shift ? 1 : 0, 128, z.dt, Q.p, Q.sb, Q.st, K.p, K.sb,
                              K.st, V.p, V.sb, V.st, O.p, O.sb, O.st, ls.data_ptr<float>(), G.p, G.sb, G.st, (float)scale, DQ.p, DQ.sb, DQ.st,
                              DK.p, DK.sb, DK.st, DV.p, DV.sb, DV.st, scratch.data_ptr()), "igs_window_attn_bwd");
    return {dq, dk, dv};
}

// ---- the unimatch CNN encoder's instance norms and position add (inorm.hip; contract in include/igs_rast.h) ----
// [N, C, H, W], float32 / float16, contiguous (the Python layer copies what is not)
int encoder_check(const char* fn, const Tensor& t, const char* name)
{
    const int dt = dtype_code(t, fn, name);
    if (t.dim() != 4) throw RasterizerError(std::string(fn) + ": " + name + " must have shape [N, C, H, W] (got " + c10::str(t.sizes()) + ")");
    if (!t.is_contiguous()) throw RasterizerError(std::string(fn) + ": " + name + " must be contiguous");
    return dt;
}
void encoder_same(const char* fn, const Tensor& t, const char* name, const Tensor& like)
{
    if (t.scalar_type() != like.scalar_type()) throw NotImplemented(std::string(fn) + ": " + name + " must have x's dtype");
    if (t.sizes() != like.sizes())
        throw RasterizerError(std::string(fn) + ": " + name + " has shape " + c10::str(t.sizes()) + ", expected " + c10::str(like.sizes()));
    if (t.dim() != 4 || !t.is_contiguous()) throw RasterizerError(std::string(fn) + ": " + name + " must be contiguous");
}
// out (x itself when inplace): mode is an IGS_INORM_* code; skip is read in the two modes that have one
Tensor instance_norm_fwd(const Tensor& x, const OptTensor& skip, int64_t mode, double eps, bool inplace)
{
    const char* fn = "instance_norm_fwd";
    const int dt = encoder_check(fn, x, "x");
    const bool has_skip = mode == IGS_INORM_RELU_ADD_RELU || mode == IGS_INORM_RELU_ADDNORM_RELU;
    if (has_skip && !skip) throw RasterizerError(std::string(fn) + ": this mode needs skip");
    if (has_skip) encoder_same(fn, *skip, "skip", x);
    if (x.size(2) * x.size(3) < 2) throw RasterizerError(std::string(fn) + ": Expected more than 1 spatial element (got " + c10::str(x.sizes()) + ")");
    const GpuCall c(x, fn, "x");
    if (has_skip) same_device(x, fn, {{*skip, "skip"}});
    Tensor out = inplace ? x : at::empty_like(x);
    check(igs_instance_norm_fwd(c.stream(), x.data_ptr(), has_skip ? skip->data_ptr() : nullptr, out.data_ptr(), x.size(0) * x.size(1),
                                x.size(2) * x.size(3), dt, (int)mode, (float)eps), "igs_instance_norm_fwd");
    return out;
}
// (feature0 + position, feature1 + position), written into the inputs when inplace
std::tuple<Tensor, Tensor> position_add(const Tensor& f0, const Tensor& f1, int64_t splits, bool inplace)
{
    const char* fn = "position_add";
    const int dt = encoder_check(fn, f0, "feature0");
    encoder_same(fn, f1, "feature1", f0);
    if (f0.size(0) > INT_MAX || f0.size(1) > INT_MAX || f0.size(2) > INT_MAX || f0.size(3) > INT_MAX || splits > INT_MAX || splits < INT_MIN)
        throw RasterizerError(std::string(fn) + ": sizes out of range");
    const GpuCall c(f0, fn, "feature0", {{f1, "feature1"}});
    Tensor o0 = inplace ? f0 : at::empty_like(f0), o1 = inplace ? f1 : at::empty_like(f1);
    check(igs_position_add(c.stream(), f0.data_ptr(), f1.data_ptr(), o0.data_ptr(), o1.data_ptr(), (int)f0.size(0), (int)f0.size(1), (int)f0.size(2),
                           (int)f0.size(3), (int)splits, dt), "igs_position_add");
    return {o0, o1};
}

// ---- LayerNorm and GEGLU of the two transformers (tokens.hip; contract in include/igs_rast.h) ----
// [N, C] rows, float32 / float16, stride 1 inside a row and a row stride of at least C (the Python layer copies what is not)
int token_rows_check(const char* fn, const Tensor& t, const char* name)
{
    const int dt = dtype_code(t, fn, name);
    if (t.dim() != 2) throw RasterizerError(std::string(fn) + ": " + name + " must have shape [N, C] (got " + c10::str(t.sizes()) + ")");
    if ((t.size(1) > 1 && t.stride(1) != 1) || (t.size(0) > 1 && t.stride(0) < t.size(1)))
        throw RasterizerError(std::string(fn) + ": " + name + " must have stride 1 inside a row and a row stride of at least the row length");
    return dt;
}
// the row stride for the C call (a single row's own stride is arbitrary in PyTorch)
int64_t token_row_stride(const Tensor& t) { return t.size(0) > 1 ? t.stride(0) : t.size(1); }
void token_param_check(const char* fn, const OptTensor& p, const char* name, int64_t C)
{
    if (p) expect(*p, fn, name, at::kFloat, {C});
}
// out [N, C] contiguous, float16 when out_half, else float32: (residual +) LN(x) * weight + bias
Tensor layer_norm_fwd(const Tensor& x, const OptTensor& weight, const OptTensor& bias, double eps, const OptTensor& residual, bool out_half)
{
    const char* fn = "layer_norm_fwd";
    const int xdt = token_rows_check(fn, x, "x");
    const int64_t N = x.size(0), C = x.size(1);
    token_param_check(fn, weight, "weight", C);
    token_param_check(fn, bias, "bias", C);
    if (weight.has_value() != bias.has_value()) throw RasterizerError(std::string(fn) + ": weight and bias go together (both or neither)");
    int rdt = IGS_DTYPE_F32;
    if (residual) {
        rdt = token_rows_check(fn, *residual, "residual");
        if (residual->sizes() != x.sizes())
            throw RasterizerError(std::string(fn) + ": residual has shape " + c10::str(residual->sizes()) + ", expected " + c10::str(x.sizes()));
    }
    if (C < 1 || C > IGS_LN_MAX_C || N > IGS_LN_MAX_ROWS)
        throw RasterizerError(std::string(fn) + ": sizes out of range (1 <= C <= " + std::to_string(IGS_LN_MAX_C) + ", N <= 2^24)");
    const GpuCall c(x, fn, "x");
    if (weight) same_device(x, fn, {{*weight, "weight"}, {*bias, "bias"}});
    if (residual) same_device(x, fn, {{*residual, "residual"}});
    Tensor out = at::empty({N, C}, x.options().dtype(out_half ? at::kHalf : at::kFloat));
    if (N == 0) return out;
    OptTensor wc, bc;
    if (weight) { wc = weight->contiguous(); bc = bias->contiguous(); }
    check(igs_layer_norm_fwd(c.stream(), N, (int)C, xdt, x.data_ptr(), token_row_stride(x), rdt, ptr_or_null(residual), residual ? token_row_stride(*residual) : C,
                             ptr_or_null<float>(wc), ptr_or_null<float>(bc), (float)eps, out_half ? IGS_DTYPE_F16 : IGS_DTYPE_F32, out.data_ptr(), C),
          "igs_layer_norm_fwd");
    return out;
}
// (d x [N, C] contiguous in x's dtype, d weight, d bias [C] float32), each None unless wanted; d residual is grad_out itself
std::tuple<OptTensor, OptTensor, OptTensor> layer_norm_bwd(const Tensor& x, const OptTensor& weight, double eps, const Tensor& grad_out, bool want_x,
                                                           bool want_weight, bool want_bias)
{
    const char* fn = "layer_norm_bwd";
    const int xdt = token_rows_check(fn, x, "x"), gdt = token_rows_check(fn, grad_out, "grad_out");
    const int64_t N = x.size(0), C = x.size(1);
    token_param_check(fn, weight, "weight", C);
    if (grad_out.sizes() != x.sizes())
        throw RasterizerError(std::string(fn) + ": grad_out has shape " + c10::str(grad_out.sizes()) + ", expected " + c10::str(x.sizes()));
    if (C < 1 || C > IGS_LN_MAX_C || N > IGS_LN_MAX_ROWS)
        throw RasterizerError(std::string(fn) + ": sizes out of range (1 <= C <= " + std::to_string(IGS_LN_MAX_C) + ", N <= 2^24)");
    const GpuCall c(x, fn, "x", {{grad_out, "grad_out"}});
    if (weight) same_device(x, fn, {{*weight, "weight"}});
    OptTensor dx, dw, db, scratch, wc;
    const auto fo = x.options().dtype(at::kFloat);
    if (want_x) dx = at::empty({N, C}, x.options());
    if (want_weight) dw = N == 0 ? at::zeros({C}, fo) : at::empty({C}, fo);
    if (want_bias) db = N == 0 ? at::zeros({C}, fo) : at::empty({C}, fo);
    if (N == 0 || !(want_x || want_weight || want_bias)) return {dx, dw, db};
    if (want_weight || want_bias) scratch = at::empty({(int64_t)igs_layer_norm_bwd_scratch_bytes(N, (int)C)}, x.options().dtype(at::kByte));
    if (weight) wc = weight->contiguous();
    check(igs_layer_norm_bwd(c.stream(), N, (int)C, xdt, x.data_ptr(), token_row_stride(x), ptr_or_null<float>(wc), (float)eps, gdt, grad_out.data_ptr(),
                             token_row_stride(grad_out), xdt, ptr_or_null(dx), C, ptr_or_null<float>(dw), ptr_or_null<float>(db), ptr_or_null(scratch)),
          "igs_layer_norm_bwd");
    return {dx, dw, db};
}
int64_t geglu_check(const char* fn, const Tensor& proj)
{
    if (proj.size(1) % 2) throw RasterizerError(std::string(fn) + ": proj must have an even row length 2 D (got " + c10::str(proj.sizes()) + ")");
    const int64_t D = proj.size(1) / 2;
    if (D < 1 || D > IGS_GEGLU_MAX_D || proj.size(0) * D > IGS_GEGLU_MAX_ELEMS)
        throw RasterizerError(std::string(fn) + ": sizes out of range (1 <= D <= " + std::to_string(IGS_GEGLU_MAX_D) + ", N * D <= 2^30)");
    return D;
}
// out [N, D] contiguous in proj's dtype: proj[:, :D] * gelu(proj[:, D:])
Tensor geglu_fwd(const Tensor& proj)
{
    const char* fn = "geglu_fwd";
    const int dt = token_rows_check(fn, proj, "proj");
    const int64_t N = proj.size(0), D = geglu_check(fn, proj);
    const GpuCall c(proj, fn, "proj");
    Tensor out = at::empty({N, D}, proj.options());
    if (N == 0) return out;
    check(igs_geglu_fwd(c.stream(), N, (int)D, dt, proj.data_ptr(), token_row_stride(proj), out.data_ptr()), "igs_geglu_fwd");
    return out;
}
// d proj [N, 2 D] contiguous in proj's dtype, both halves
Tensor geglu_bwd(const Tensor& proj, const Tensor& grad_out)
{
    const char* fn = "geglu_bwd";
    const int dt = token_rows_check(fn, proj, "proj");
    const int64_t N = proj.size(0), D = geglu_check(fn, proj);
    expect(grad_out, fn, "grad_out", proj.scalar_type(), {N, D});
    const GpuCall c(proj, fn, "proj", {{grad_out, "grad_out"}});
    Tensor dp = at::empty({N, 2 * D}, proj.options());
    if (N == 0) return dp;
    const Tensor gc = grad_out.contiguous();
    check(igs_geglu_bwd(c.stream(), N, (int)D, dt, proj.data_ptr(), token_row_stride(proj), gc.data_ptr(), dp.data_ptr()), "igs_geglu_bwd");
    return dp;
}

// ---- the two ends of Transformer1D: GroupNorm to token-major, token-major plus residual (gnorm.hip; contract in include/igs_rast.h) ----
// [B, C, A] channel-major with stride 1 on A, a channel stride of at least A and a batch stride of at least a batch's extent, and
// [B, A, C] token-major rows at one row stride through the batches (the Python layer copies what is not)
struct ChannelMajor { int dt; int64_t bs, cs; };
ChannelMajor channel_major_check(const char* fn, const Tensor& t, const char* name)
{
    ChannelMajor v;
    v.dt = dtype_code(t, fn, name);
    if (t.dim() != 3) throw RasterizerError(std::string(fn) + ": " + name + " must have shape [B, C, A] (got " + c10::str(t.sizes()) + ")");
    const int64_t C = t.size(1), A = t.size(2);
    v.cs = C > 1 ? t.stride(1) : A;
    v.bs = t.size(0) > 1 ? t.stride(0) : (C - 1) * v.cs + A;
    if ((A > 1 && t.stride(2) != 1) || v.cs < A || v.bs < (C - 1) * v.cs + A)
        throw RasterizerError(std::string(fn) + ": " + name + " must have stride 1 on A, a channel stride of at least A and a batch stride of at least a batch's extent");
    return v;
}
struct TokenMajor { int dt; int64_t rs; };
TokenMajor token_major_check(const char* fn, const Tensor& t, const char* name)
{
    TokenMajor v;
    v.dt = dtype_code(t, fn, name);
    if (t.dim() != 3) throw RasterizerError(std::string(fn) + ": " + name + " must have shape [B, A, C] (got " + c10::str(t.sizes()) + ")");
    const int64_t A = t.size(1), C = t.size(2);
    v.rs = A > 1 ? t.stride(1) : C;
    if ((C > 1 && t.stride(2) != 1) || v.rs < C || (t.size(0) > 1 && t.stride(0) != A * v.rs))
        throw RasterizerError(std::string(fn) + ": " + name + " must be rows with stride 1 inside a row and one row stride of at least the row length through the batches");
    return v;
}
void group_norm_sizes_check(const char* fn, int64_t B, int64_t C, int64_t G, int64_t A)
{
    if (C < 1 || C > IGS_GN_MAX_C || G < 1 || C % G != 0 || A < 1 || (C / G) * A > IGS_GN_MAX_GROUP_ELEMS || B * A > IGS_GN_MAX_TOKENS)
        throw RasterizerError(std::string(fn) + ": sizes out of range (1 <= C <= " + std::to_string(IGS_GN_MAX_C) + ", G >= 1 dividing C, A >= 1, (C / G) * A <= 2^30, B * A <= 2^24)");
}
// (out [B, A, C] contiguous, float16 when out_half, else float32; stats [B, G, 2] float32): GroupNorm(x) * weight + bias, written token-major
std::tuple<Tensor, Tensor> group_norm_tokens_fwd(const Tensor& x, int64_t num_groups, const OptTensor& weight, const OptTensor& bias, double eps, bool out_half)
{
    const char* fn = "group_norm_tokens_fwd";
    const ChannelMajor xv = channel_major_check(fn, x, "x");
    const int64_t B = x.size(0), C = x.size(1), A = x.size(2);
    token_param_check(fn, weight, "weight", C);
    token_param_check(fn, bias, "bias", C);
    if (weight.has_value() != bias.has_value()) throw RasterizerError(std::string(fn) + ": weight and bias go together (both or neither)");
    group_norm_sizes_check(fn, B, C, num_groups, A);
    const GpuCall c(x, fn, "x");
    if (weight) same_device(x, fn, {{*weight, "weight"}, {*bias, "bias"}});
    Tensor out = at::empty({B, A, C}, x.options().dtype(out_half ? at::kHalf : at::kFloat));
    Tensor stats = at::empty({B, num_groups, 2}, x.options().dtype(at::kFloat));
    if (B == 0) return {out, stats};
    OptTensor wc, bc;
    if (weight) { wc = weight->contiguous(); bc = bias->contiguous(); }
    check(igs_group_norm_tokens_fwd(c.stream(), (int)B, (int)C, (int)num_groups, A, xv.dt, x.data_ptr(), xv.bs, xv.cs, ptr_or_null<float>(wc), ptr_or_null<float>(bc),
                                    (float)eps, out_half ? IGS_DTYPE_F16 : IGS_DTYPE_F32, out.data_ptr(), C, stats.data_ptr<float>()),
          "igs_group_norm_tokens_fwd");
    return {out, stats};
}
// (d x [B, C, A] contiguous in x's dtype, d weight, d bias [C] float32), each None unless wanted
std::tuple<OptTensor, OptTensor, OptTensor> group_norm_tokens_bwd(const Tensor& x, int64_t num_groups, const OptTensor& weight, const Tensor& stats,
                                                                  const Tensor& grad_out, bool want_x, bool want_weight, bool want_bias)
{
    const char* fn = "group_norm_tokens_bwd";
    const ChannelMajor xv = channel_major_check(fn, x, "x");
    const TokenMajor gv = token_major_check(fn, grad_out, "grad_out");
    const int64_t B = x.size(0), C = x.size(1), A = x.size(2);
    token_param_check(fn, weight, "weight", C);
    group_norm_sizes_check(fn, B, C, num_groups, A);
    expect(stats, fn, "stats", at::kFloat, {B, num_groups, 2});
    if (grad_out.size(0) != B || grad_out.size(1) != A || grad_out.size(2) != C)
        throw RasterizerError(std::string(fn) + ": grad_out has shape " + c10::str(grad_out.sizes()) + ", expected " + c10::str(at::IntArrayRef({B, A, C})));
    const GpuCall c(x, fn, "x", {{grad_out, "grad_out"}, {stats, "stats"}});
    if (weight) same_device(x, fn, {{*weight, "weight"}});
    OptTensor dx, dw, db, wc;
    const auto fo = x.options().dtype(at::kFloat);
    if (want_x) dx = at::empty({B, C, A}, x.options());
    if (want_weight) dw = B == 0 ? at::zeros({C}, fo) : at::empty({C}, fo);
    if (want_bias) db = B == 0 ? at::zeros({C}, fo) : at::empty({C}, fo);
    if (B == 0 || !(want_x || want_weight || want_bias)) return {dx, dw, db};
    const Tensor scratch = at::empty({(int64_t)igs_group_norm_tokens_bwd_scratch_bytes((int)B, (int)C, (int)num_groups, A)}, x.options().dtype(at::kByte));
    const Tensor sc = stats.contiguous();
    if (weight) wc = weight->contiguous();
    check(igs_group_norm_tokens_bwd(c.stream(), (int)B, (int)C, (int)num_groups, A, xv.dt, x.data_ptr(), xv.bs, xv.cs, ptr_or_null<float>(wc), sc.data_ptr<float>(),
                                    gv.dt, grad_out.data_ptr(), gv.rs, xv.dt, ptr_or_null(dx), C * A, A, ptr_or_null<float>(dw), ptr_or_null<float>(db),
                                    scratch.data_ptr()),
          "igs_group_norm_tokens_bwd");
    return {dx, dw, db};
}
// out [B, A, C] contiguous, float16 when out_half, else float32: tokens + residual read channel-major
Tensor tokens_add_residual(const Tensor& tokens, const Tensor& residual, bool out_half)
{
    const char* fn = "tokens_add_residual";
    const TokenMajor tv = token_major_check(fn, tokens, "tokens");
    const ChannelMajor rv = channel_major_check(fn, residual, "residual");
    const int64_t B = tokens.size(0), A = tokens.size(1), C = tokens.size(2);
    if (residual.size(0) != B || residual.size(1) != C || residual.size(2) != A)
        throw RasterizerError(std::string(fn) + ": residual has shape " + c10::str(residual.sizes()) + ", expected " + c10::str(at::IntArrayRef({B, C, A})));
    group_norm_sizes_check(fn, B, C, 1, A);
    const GpuCall c(tokens, fn, "tokens", {{residual, "residual"}});
    Tensor out = at::empty({B, A, C}, tokens.options().dtype(out_half ? at::kHalf : at::kFloat));
    if (B == 0) return out;
    check(igs_tokens_add_residual(c.stream(), (int)B, (int)C, A, tv.dt, tokens.data_ptr(), tv.rs, rv.dt, residual.data_ptr(), rv.bs, rv.cs,
                                  out_half ? IGS_DTYPE_F16 : IGS_DTYPE_F32, out.data_ptr(), C),
          "igs_tokens_add_residual");
    return out;
}

// ---- the residual decoder (mlp.hip) ----
std::vector<int> mlp_ints(const std::vector<int64_t>& v) { return std::vector<int>(v.begin(), v.end()); }
int64_t mlp_pack_elems(const std::vector<int64_t>& widths, const std::vector<int64_t>& head_widths)
{
    const std::vector<int> w = mlp_ints(widths), hw = mlp_ints(head_widths);
    return igs_mlp_heads_pack_elems((int)w.size() - 1, w.data(), (int)hw.size(), hw.data());
}
// one contiguous [N, head_widths[k]] tensor per head in x's dtype.  x [N, widths[0]] with stride 1 inside a row; wpack, bpack as
// igs_mlp_heads_fwd takes them (igs_amd/motion.py packs and caches them)
std::vector<Tensor> mlp_heads_fwd(const Tensor& x, const Tensor& wpack, const Tensor& bpack, const std::vector<int64_t>& widths,
                                  const std::vector<int64_t>& act_after, const std::vector<int64_t>& head_widths, int64_t act)
{
    const char* fn = "mlp_heads_fwd";
    const int dt = dtype_code(x, fn, "x");
    if (widths.empty() || act_after.size() + 1 != widths.size()) throw RasterizerError(std::string(fn) + ": widths needs one entry more than act_after");
    expect(x, fn, "x", x.scalar_type(), {-1, widths[0]});
    const int64_t N = x.size(0), C0 = x.size(1);
    const int64_t rs = N > 1 ? x.stride(0) : C0;
    if ((C0 > 1 && x.stride(1) != 1) || rs < C0) throw RasterizerError(std::string(fn) + ": x must have stride 1 inside a row and a row stride of at least the row length");
    const int64_t elems = mlp_pack_elems(widths, head_widths);
    if (elems < 0) throw RasterizerError(std::string(fn) + ": sizes out of range (0..3 hidden Linears, 1..8 heads, every width and the heads' sum in 1..128)");
    expect(wpack, fn, "wpack", x.scalar_type(), {elems});
    expect(bpack, fn, "bpack", at::kFloat, {(int64_t)widths.size(), IGS_MLP_MAX_WIDTH});
    if (!wpack.is_contiguous() || !bpack.is_contiguous()) throw RasterizerError(std::string(fn) + ": wpack and bpack must be contiguous");
    const GpuCall c(x, fn, "x", {{wpack, "wpack"}, {bpack, "bpack"}});
    std::vector<Tensor> outs;
    std::vector<void*> ptrs;
    for (int64_t ch : head_widths) {
        outs.push_back(at::empty({N, ch}, x.options()));
        ptrs.push_back(outs.back().data_ptr());
    }
    if (N == 0) return outs;
    const std::vector<int> w = mlp_ints(widths), aa = mlp_ints(act_after), hw = mlp_ints(head_widths);
    check(igs_mlp_heads_fwd(c.stream(), N, dt, (int)act, (int)aa.size(), w.data(), aa.data(), (int)hw.size(), hw.data(), x.data_ptr(), rs, wpack.data_ptr(),
                            bpack.data_ptr<float>(), ptrs.data()),
          "igs_mlp_heads_fwd");
    return outs;
}
int64_t mlp_bwd_scratch_bytes(int64_t N, bool half, const std::vector<int64_t>& widths, const std::vector<int64_t>& head_widths)
{
    const std::vector<int> w = mlp_ints(widths), hw = mlp_ints(head_widths);
    return igs_mlp_heads_bwd_scratch_bytes(N, half ? IGS_DTYPE_F16 : IGS_DTYPE_F32, (int)w.size() - 1, w.data(), (int)hw.size(), hw.data());
}
// (d x [N, widths[0]] in x's dtype, d w, d b float32 and flat as igs_mlp_heads_bwd lays them out), each None unless wanted.  douts[k]:
// [N, head_widths[k]] contiguous in x's dtype, or None for zeros; wpack_t: the transposed Linears packed like wpack
std::tuple<OptTensor, OptTensor, OptTensor> mlp_heads_bwd(const Tensor& x, const Tensor& wpack, const Tensor& wpack_t, const Tensor& bpack,
                                                          const std::vector<int64_t>& widths, const std::vector<int64_t>& act_after,
                                                          const std::vector<int64_t>& head_widths, int64_t act, const std::vector<OptTensor>& douts,
                                                          bool want_x, bool want_w, bool want_b)
{
    const char* fn = "mlp_heads_bwd";
    const int dt = dtype_code(x, fn, "x");
    if (widths.empty() || act_after.size() + 1 != widths.size()) throw RasterizerError(std::string(fn) + ": widths needs one entry more than act_after");
    expect(x, fn, "x", x.scalar_type(), {-1, widths[0]});
    const int64_t N = x.size(0), C0 = x.size(1);
    const int64_t rs = N > 1 ? x.stride(0) : C0;
    if ((C0 > 1 && x.stride(1) != 1) || rs < C0) throw RasterizerError(std::string(fn) + ": x must have stride 1 inside a row and a row stride of at least the row length");
    const int64_t elems = mlp_pack_elems(widths, head_widths);
    if (elems < 0) throw RasterizerError(std::string(fn) + ": sizes out of range (0..3 hidden Linears, 1..8 heads, every width and the heads' sum in 1..128)");
    expect(wpack, fn, "wpack", x.scalar_type(), {elems});
    expect(wpack_t, fn, "wpack_t", x.scalar_type(), {elems});
    expect(bpack, fn, "bpack", at::kFloat, {(int64_t)widths.size(), IGS_MLP_MAX_WIDTH});
    if (!wpack.is_contiguous() || !wpack_t.is_contiguous() || !bpack.is_contiguous()) throw RasterizerError(std::string(fn) + ": wpack, wpack_t and bpack must be contiguous");
    if (douts.size() != head_widths.size()) throw RasterizerError(std::string(fn) + ": one upstream gradient (or None) per head");
    for (size_t k = 0; k < douts.size(); k++)
        if (douts[k]) {
            expect(*douts[k], fn, "an upstream gradient", x.scalar_type(), {N, head_widths[k]});
            if (!douts[k]->is_contiguous()) throw RasterizerError(std::string(fn) + ": the upstream gradients must be contiguous");
        }
    const GpuCall c(x, fn, "x", {{wpack, "wpack"}, {wpack_t, "wpack_t"}, {bpack, "bpack"}});
    for (const OptTensor& g : douts)
        if (g) same_device(x, fn, {{*g, "an upstream gradient"}});
    int64_t tw = 0, tb = 0;
    for (size_t l = 0; l + 1 < widths.size(); l++) { tw += widths[l + 1] * widths[l]; tb += widths[l + 1]; }
    for (int64_t ch : head_widths) { tw += ch * widths.back(); tb += ch; }
    OptTensor dx, dw, db;
    const auto fo = x.options().dtype(at::kFloat);
    if (want_x) dx = at::empty({N, C0}, x.options());
    if (want_w) dw = at::empty({tw}, fo);
    if (want_b) db = at::empty({tb}, fo);
    if (!(want_x || want_w || want_b)) return {dx, dw, db};
    const Tensor scratch = at::empty({N == 0 ? 0 : mlp_bwd_scratch_bytes(N, dt == IGS_DTYPE_F16, widths, head_widths)}, x.options().dtype(at::kByte));
    std::vector<const void*> ptrs;
    for (const OptTensor& g : douts) ptrs.push_back(ptr_or_null(g));
    const std::vector<int> w = mlp_ints(widths), aa = mlp_ints(act_after), hw = mlp_ints(head_widths);
    check(igs_mlp_heads_bwd(c.stream(), N, dt, (int)act, (int)aa.size(), w.data(), aa.data(), (int)hw.size(), hw.data(), x.data_ptr(), rs, wpack.data_ptr(),
                            wpack_t.data_ptr(), bpack.data_ptr<float>(), ptrs.data(), scratch.data_ptr(), scratch.numel(), ptr_or_null(dx),
                            ptr_or_null<float>(dw), ptr_or_null<float>(db)),
          "igs_mlp_heads_bwd");
    return {dx, dw, db};
}

// ---- the tail of a unimatch TransformerLayer in one launch (ffn.hip; contract in include/igs_rast.h) ----
int64_t layer_tail_pack_elems(int64_t hidden, bool has_ffn) { return igs_layer_tail_pack_elems((int)std::min<int64_t>(hidden, INT_MAX), has_ffn ? 1 : 0); }
// out [T, 128] contiguous, float16 when out_half, else float32.  attn_out, source: [T, 128] rows (token_rows_check), float32 / float16 each;
// wpack in the compute dtype as igs_layer_tail_fwd takes it (igs_amd/tokens.py packs and caches it); hidden == 0: no FFN, and ln2_* absent
Tensor layer_tail_fwd(const Tensor& attn_out, const Tensor& source, const Tensor& wpack, int64_t hidden, const Tensor& ln1_w, const Tensor& ln1_b,
                      double eps1, const OptTensor& ln2_w, const OptTensor& ln2_b, double eps2, bool out_half)
{
    const char* fn = "layer_tail_fwd";
    const int adt = token_rows_check(fn, attn_out, "attn_out"), sdt = token_rows_check(fn, source, "source");
    const int cdt = dtype_code(wpack, fn, "wpack");
    const int64_t T = attn_out.size(0);
    if (attn_out.size(1) != 128 || source.sizes() != attn_out.sizes())
        throw RasterizerError(std::string(fn) + ": attn_out and source must both be [T, 128] (got " + c10::str(attn_out.sizes()) + " and " + c10::str(source.sizes()) + ")");
    const bool has_ffn = hidden != 0;
    const int64_t elems = layer_tail_pack_elems(hidden, has_ffn);
    if (hidden < 0 || elems < 0 || T > IGS_LAYER_TAIL_MAX_ROWS)
        throw RasterizerError(std::string(fn) + ": sizes out of range (hidden a multiple of 32 in 32.." + std::to_string(IGS_LAYER_TAIL_MAX_HIDDEN) + ", T <= 2^24)");
    expect(wpack, fn, "wpack", wpack.scalar_type(), {elems});
    if (!wpack.is_contiguous()) throw RasterizerError(std::string(fn) + ": wpack must be contiguous");
    expect(ln1_w, fn, "ln1_w", at::kFloat, {128});
    expect(ln1_b, fn, "ln1_b", at::kFloat, {128});
    if (has_ffn != (ln2_w.has_value() && ln2_b.has_value())) throw RasterizerError(std::string(fn) + ": ln2_w and ln2_b go with the FFN (both or neither)");
    token_param_check(fn, ln2_w, "ln2_w", 128);
    token_param_check(fn, ln2_b, "ln2_b", 128);
    const GpuCall c(attn_out, fn, "attn_out", {{source, "source"}, {wpack, "wpack"}, {ln1_w, "ln1_w"}, {ln1_b, "ln1_b"}});
    if (has_ffn) same_device(attn_out, fn, {{*ln2_w, "ln2_w"}, {*ln2_b, "ln2_b"}});
    Tensor out = at::empty({T, 128}, attn_out.options().dtype(out_half ? at::kHalf : at::kFloat));
    if (T == 0) return out;
    const Tensor w1 = ln1_w.contiguous(), b1 = ln1_b.contiguous();
    OptTensor w2, b2;
    if (has_ffn) { w2 = ln2_w->contiguous(); b2 = ln2_b->contiguous(); }
    check(igs_layer_tail_fwd(c.stream(), T, cdt, has_ffn ? 1 : 0, (int)hidden, attn_out.data_ptr(), adt, token_row_stride(attn_out), source.data_ptr(), sdt,
                             token_row_stride(source), wpack.data_ptr(), w1.data_ptr<float>(), b1.data_ptr<float>(), (float)eps1, ptr_or_null<float>(w2),
                             ptr_or_null<float>(b2), (float)eps2, out.data_ptr(), out_half ? IGS_DTYPE_F16 : IGS_DTYPE_F32, 128),
          "igs_layer_tail_fwd");
    return out;
}

int64_t layer_tail_bwd_scratch_bytes(int64_t T, bool half, int64_t hidden)
{
    return igs_layer_tail_bwd_scratch_bytes(T, half ? IGS_DTYPE_F16 : IGS_DTYPE_F32, hidden != 0 ? 1 : 0, (int)std::min<int64_t>(hidden, INT_MAX));
}
// (d attn_out, d source [T, 128] contiguous, float16 when da_half / ds_half, else float32; d merge [128, 128], d ln1_w, d ln1_b [128],
// d mlp[0] [hidden, 256], d mlp[2] [128, hidden], d ln2_w, d ln2_b [128], float32), each None unless its `want` entry is set (in that
// order; the last four need an FFN).  attn_out, source, wpack, ln*: as layer_tail_fwd read them; wpack_t: the transposed pack; dout: [T, 128] rows
std::vector<OptTensor> layer_tail_bwd(const Tensor& attn_out, const Tensor& source, const Tensor& dout, const Tensor& wpack, const Tensor& wpack_t,
                                      int64_t hidden, const Tensor& ln1_w, const Tensor& ln1_b, double eps1, const OptTensor& ln2_w,
                                      const OptTensor& ln2_b, double eps2, const std::vector<bool>& want, bool da_half, bool ds_half)
{
    const char* fn = "layer_tail_bwd";
    const int adt = token_rows_check(fn, attn_out, "attn_out"), sdt = token_rows_check(fn, source, "source"), gdt = token_rows_check(fn, dout, "dout");
    const int cdt = dtype_code(wpack, fn, "wpack");
    const int64_t T = attn_out.size(0);
    if (attn_out.size(1) != 128 || source.sizes() != attn_out.sizes() || dout.sizes() != attn_out.sizes())
        throw RasterizerError(std::string(fn) + ": attn_out, source and dout must all be [T, 128] (got " + c10::str(attn_out.sizes()) + ", " +
                              c10::str(source.sizes()) + " and " + c10::str(dout.sizes()) + ")");
    const bool has_ffn = hidden != 0;
    const int64_t elems = layer_tail_pack_elems(hidden, has_ffn);
    if (hidden < 0 || elems < 0 || T > IGS_LAYER_TAIL_MAX_ROWS)
        throw RasterizerError(std::string(fn) + ": sizes out of range (hidden a multiple of 32 in 32.." + std::to_string(IGS_LAYER_TAIL_MAX_HIDDEN) + ", T <= 2^24)");
    if (want.size() != 9) throw RasterizerError(std::string(fn) + ": want needs nine entries");
    expect(wpack, fn, "wpack", wpack.scalar_type(), {elems});
    expect(wpack_t, fn, "wpack_t", wpack.scalar_type(), {elems});
    if (!wpack.is_contiguous() || !wpack_t.is_contiguous()) throw RasterizerError(std::string(fn) + ": wpack and wpack_t must be contiguous");
    expect(ln1_w, fn, "ln1_w", at::kFloat, {128});
    expect(ln1_b, fn, "ln1_b", at::kFloat, {128});
    if (has_ffn != (ln2_w.has_value() && ln2_b.has_value())) throw RasterizerError(std::string(fn) + ": ln2_w and ln2_b go with the FFN (both or neither)");
    token_param_check(fn, ln2_w, "ln2_w", 128);
    token_param_check(fn, ln2_b, "ln2_b", 128);
    const GpuCall c(attn_out, fn, "attn_out", {{source, "source"}, {dout, "dout"}, {wpack, "wpack"}, {wpack_t, "wpack_t"}, {ln1_w, "ln1_w"}, {ln1_b, "ln1_b"}});
    if (has_ffn) same_device(attn_out, fn, {{*ln2_w, "ln2_w"}, {*ln2_b, "ln2_b"}});
    const auto fo = attn_out.options().dtype(at::kFloat);
    std::vector<OptTensor> out(9);
    if (want[0]) out[0] = at::empty({T, 128}, attn_out.options().dtype(da_half ? at::kHalf : at::kFloat));
    if (want[1]) out[1] = at::empty({T, 128}, attn_out.options().dtype(ds_half ? at::kHalf : at::kFloat));
    if (want[2]) out[2] = at::empty({128, 128}, fo);
    if (want[3]) out[3] = at::empty({128}, fo);
    if (want[4]) out[4] = at::empty({128}, fo);
    if (has_ffn) {
        if (want[5]) out[5] = at::empty({hidden, 256}, fo);
        if (want[6]) out[6] = at::empty({128, hidden}, fo);
        if (want[7]) out[7] = at::empty({128}, fo);
        if (want[8]) out[8] = at::empty({128}, fo);
    }
    bool any = false;
    for (const OptTensor& t : out) any = any || t.has_value();
    if (!any) return out;
    const Tensor w1 = ln1_w.contiguous(), b1 = ln1_b.contiguous();
    OptTensor w2, b2;
    if (has_ffn) { w2 = ln2_w->contiguous(); b2 = ln2_b->contiguous(); }
    const Tensor scratch = at::empty({layer_tail_bwd_scratch_bytes(T, cdt == IGS_DTYPE_F16, hidden)}, attn_out.options().dtype(at::kByte));
    check(igs_layer_tail_bwd(c.stream(), T, cdt, has_ffn ? 1 : 0, (int)hidden, attn_out.data_ptr(), adt, token_row_stride(attn_out), source.data_ptr(), sdt,
                             token_row_stride(source), dout.data_ptr(), gdt, token_row_stride(dout), wpack.data_ptr(), wpack_t.data_ptr(),
                             w1.data_ptr<float>(), b1.data_ptr<float>(), (float)eps1, ptr_or_null<float>(w2), ptr_or_null<float>(b2), (float)eps2,
                             scratch.data_ptr(), scratch.numel(), ptr_or_null(out[0]), da_half ? IGS_DTYPE_F16 : IGS_DTYPE_F32, 128, ptr_or_null(out[1]),
                             ds_half ? IGS_DTYPE_F16 : IGS_DTYPE_F32, 128, ptr_or_null<float>(out[2]), ptr_or_null<float>(out[3]),
                             ptr_or_null<float>(out[4]), ptr_or_null<float>(out[5]), ptr_or_null<float>(out[6]), ptr_or_null<float>(out[7]),
                             ptr_or_null<float>(out[8])),
          "igs_layer_tail_bwd");
    return out;
}

// ---- the q / k / v projections of the unimatch TransformerLayers in one launch (proj.hip; contract in include/igs_rast.h) ----
int64_t token_proj_pack_elems(int64_t n) { return igs_token_proj_pack_elems((int)std::max<int64_t>(std::min<int64_t>(n, INT_MAX), INT_MIN)); }
// out [T, 128 n] contiguous, float16 when out_half, else float32: columns 128 j .. of row (t + rot[j]) mod T are W_j x[t].  x: [T, 128] rows
// (token_rows_check), float32 / float16; wpack in the compute dtype as igs_token_proj_fwd takes it (igs_amd/tokens.py packs and caches it);
// rot: n values in [0, T), or empty for zeros
Tensor token_proj_fwd(const Tensor& x, const Tensor& wpack, int64_t n, const std::vector<int64_t>& rot, bool out_half)
{
    const char* fn = "token_proj_fwd";
    const int xdt = token_rows_check(fn, x, "x");
    const int cdt = dtype_code(wpack, fn, "wpack");
    const int64_t T = x.size(0);
    if (x.size(1) != 128) throw RasterizerError(std::string(fn) + ": x must be [T, 128] (got " + c10::str(x.sizes()) + ")");
    const int64_t elems = token_proj_pack_elems(n);
    if (elems < 0 || T > IGS_TOKEN_PROJ_MAX_ROWS)
        throw RasterizerError(std::string(fn) + ": sizes out of range (n in 1.." + std::to_string(IGS_TOKEN_PROJ_MAX_OUT) + ", T <= 2^24)");
    expect(wpack, fn, "wpack", wpack.scalar_type(), {elems});
    if (!wpack.is_contiguous()) throw RasterizerError(std::string(fn) + ": wpack must be contiguous");
    if (!rot.empty() && (int64_t)rot.size() != n) throw RasterizerError(std::string(fn) + ": rot must have one entry per matrix, or none");
    for (int64_t v : rot)
        if (v < 0 || (v >= T && !(T == 0 && v == 0))) throw RasterizerError(std::string(fn) + ": a rot entry is outside 0..T-1");
    const GpuCall c(x, fn, "x", {{wpack, "wpack"}});
    Tensor out = at::empty({T, 128 * n}, x.options().dtype(out_half ? at::kHalf : at::kFloat));
    if (T == 0) return out;
    long long r[IGS_TOKEN_PROJ_MAX_OUT] = {};
    for (size_t j = 0; j < rot.size(); j++) r[j] = rot[j];
    check(igs_token_proj_fwd(c.stream(), T, (int)n, cdt, x.data_ptr(), xdt, token_row_stride(x), wpack.data_ptr(), r, out.data_ptr(),
                             out_half ? IGS_DTYPE_F16 : IGS_DTYPE_F32, 128 * n),
          "igs_token_proj_fwd");
    return out;
}

int64_t token_proj_bwd_scratch_bytes(int64_t T, int64_t n)
{
    return igs_token_proj_bwd_scratch_bytes(T, (int)std::max<int64_t>(std::min<int64_t>(n, INT_MAX), INT_MIN));
}
// (d x [T, 128] contiguous, float16 when dx_half, else float32, or None unless want_dx; n d W_j [128, 128] float32, each None unless
// want_dw[j]).  x: as token_proj_fwd read it; grads: n entries, each the gradient of output j as [T, 128] rows (column slices of a wider
// buffer included), all of one dtype, or None where output j had none; wpack_t: the pack of the transposes; rot: as the forward's
std::tuple<OptTensor, std::vector<OptTensor>> token_proj_bwd(const Tensor& x, const std::vector<OptTensor>& grads, const Tensor& wpack_t,
                                                             const std::vector<int64_t>& rot, bool want_dx, const std::vector<bool>& want_dw,
                                                             bool dx_half)
{
    const char* fn = "token_proj_bwd";
    const int xdt = token_rows_check(fn, x, "x");
    const int cdt = dtype_code(wpack_t, fn, "wpack_t");
    const int64_t T = x.size(0), n = (int64_t)grads.size();
    if (x.size(1) != 128) throw RasterizerError(std::string(fn) + ": x must be [T, 128] (got " + c10::str(x.sizes()) + ")");
    const int64_t elems = token_proj_pack_elems(n);
    if (elems < 0 || T > IGS_TOKEN_PROJ_MAX_ROWS)
        throw RasterizerError(std::string(fn) + ": sizes out of range (n in 1.." + std::to_string(IGS_TOKEN_PROJ_MAX_OUT) + ", T <= 2^24)");
    expect(wpack_t, fn, "wpack_t", wpack_t.scalar_type(), {elems});
    if (!wpack_t.is_contiguous()) throw RasterizerError(std::string(fn) + ": wpack_t must be contiguous");
    if ((int64_t)want_dw.size() != n) throw RasterizerError(std::string(fn) + ": want_dw must have one entry per matrix");
    if (!rot.empty() && (int64_t)rot.size() != n) throw RasterizerError(std::string(fn) + ": rot must have one entry per matrix, or none");
    for (int64_t v : rot)
        if (v < 0 || (v >= T && !(T == 0 && v == 0))) throw RasterizerError(std::string(fn) + ": a rot entry is outside 0..T-1");
    int gdt = IGS_DTYPE_F32;
    bool first = true;
    for (const OptTensor& g : grads) {
        if (!g) continue;
        const int dt = token_rows_check(fn, *g, "a gradient");
        if (g->sizes() != x.sizes()) throw RasterizerError(std::string(fn) + ": a gradient has shape " + c10::str(g->sizes()) + ", expected " + c10::str(x.sizes()));
        if (!first && dt != gdt) throw RasterizerError(std::string(fn) + ": the gradients must all have one dtype");
        gdt = dt;
        first = false;
    }
    const GpuCall c(x, fn, "x", {{wpack_t, "wpack_t"}});
    for (const OptTensor& g : grads)
        if (g) same_device(x, fn, {{*g, "a gradient"}});
    OptTensor dx;
    std::vector<OptTensor> dw(n);
    const auto fo = x.options().dtype(at::kFloat);
    bool any_dw = false;
    if (want_dx) dx = at::empty({T, 128}, x.options().dtype(dx_half ? at::kHalf : at::kFloat));
    for (int64_t j = 0; j < n; j++)
        if (want_dw[j]) { dw[j] = at::empty({128, 128}, fo); any_dw = true; }
    if (!want_dx && !any_dw) return {dx, dw};
    OptTensor scratch;
    if (any_dw) scratch = at::empty({token_proj_bwd_scratch_bytes(T, n)}, x.options().dtype(at::kByte));
    const void* gp[IGS_TOKEN_PROJ_MAX_OUT] = {};
    float* wp[IGS_TOKEN_PROJ_MAX_OUT] = {};
    long long gs[IGS_TOKEN_PROJ_MAX_OUT] = {}, r[IGS_TOKEN_PROJ_MAX_OUT] = {};
    for (int64_t j = 0; j < n; j++) {
        if (grads[j]) { gp[j] = grads[j]->data_ptr(); gs[j] = token_row_stride(*grads[j]); }
        wp[j] = ptr_or_null<float>(dw[j]);
        if (!rot.empty()) r[j] = rot[j];
    }
    check(igs_token_proj_bwd(c.stream(), T, (int)n, cdt, x.data_ptr(), xdt, token_row_stride(x), gp, gdt, gs, r, wpack_t.data_ptr(),
                             ptr_or_null(scratch), scratch ? scratch->numel() : 0, ptr_or_null(dx), dx_half ? IGS_DTYPE_F16 : IGS_DTYPE_F32, 128, wp),
          "igs_token_proj_bwd");
    return {dx, dw};
}

// ---- the Gaussian deform (motion.hip) ----
void deform_checks(const char* fn, const Tensor& rot, const Tensor& mask, const Tensor& dxyz, const Tensor& drot, int* dt)
{
    expect(rot, fn, "rotation", at::kFloat, {-1, 4});
    expect(mask, fn, "mask", at::kLong, {-1});
    *dt = dtype_code(drot, fn, "res_rotation");
    if (dxyz.scalar_type() != drot.scalar_type()) throw NotImplemented(std::string(fn) + ": res_xyz and res_rotation must share a dtype");
    expect(dxyz, fn, "res_xyz", dxyz.scalar_type(), {mask.size(0), 3});
    expect(drot, fn, "res_rotation", drot.scalar_type(), {mask.size(0), 4});
    if (rot.size(0) > IGS_DEFORM_MAX_POINTS || mask.size(0) > rot.size(0))
        throw RasterizerError(std::string(fn) + ": sizes out of range (M <= P <= 2^26)");
}

// (xyz_out, rotation_out): xyz[mask] += res_xyz, rotation[mask] = qmul(nrm(rotation[mask]), nrm(res_rotation))
std::tuple<Tensor, Tensor> motion_deform_fwd(const Tensor& xyz, const Tensor& rot, const Tensor& mask, const Tensor& dxyz, const Tensor& drot)
{
    const char* fn = "motion_deform_fwd";
    int dt;
    expect(xyz, fn, "xyz", at::kFloat, {-1, 3});
    deform_checks(fn, rot, mask, dxyz, drot, &dt);
    if (rot.size(0) != xyz.size(0)) throw RasterizerError(std::string(fn) + ": xyz and rotation must have the same number of rows");
    const GpuCall c(xyz, fn, "xyz", {{rot, "every input"}, {mask, "every input"}, {dxyz, "every input"}, {drot, "every input"}});
    const int64_t P = xyz.size(0), M = mask.size(0);
    Tensor xo = at::empty({P, 3}, xyz.options()), ro = at::empty({P, 4}, xyz.options());
    if (P == 0) return {xo, ro};
    const Tensor xc = xyz.contiguous(), rc = rot.contiguous(), mc = mask.contiguous(), dxc = dxyz.contiguous(), drc = drot.contiguous();
    check(igs_gaussian_deform_fwd(c.stream(), (int)P, (int)M, dt, xc.data_ptr<float>(), rc.data_ptr<float>(), mc.data_ptr<int64_t>(),
                                  dxc.data_ptr(), drc.data_ptr(), xo.data_ptr<float>(), ro.data_ptr<float>()), "igs_gaussian_deform_fwd");
    return {xo, ro};
}

// (d_xyz, d_rotation, d_res_xyz, d_res_rotation), each None unless asked for; g_xyz / g_rot may be None (zero)
std::tuple<OptTensor, OptTensor, OptTensor, OptTensor> motion_deform_bwd(const Tensor& rot, const Tensor& mask, const Tensor& dxyz,
                                                                         const Tensor& drot, const OptTensor& g_xyz, const OptTensor& g_rot,
                                                                         bool want_xyz, bool want_rot, bool want_dxyz, bool want_drot)
{
    const char* fn = "motion_deform_bwd";
    int dt;
    deform_checks(fn, rot, mask, dxyz, drot, &dt);
    const int64_t P = rot.size(0), M = mask.size(0);
    if (g_xyz) expect(*g_xyz, fn, "grad_xyz", at::kFloat, {P, 3});
    if (g_rot) expect(*g_rot, fn, "grad_rotation", at::kFloat, {P, 4});
    const GpuCall c(rot, fn, "rotation", {{mask, "every input"}, {dxyz, "every input"}, {drot, "every input"}});
    if (g_xyz) same_device(rot, fn, {{*g_xyz, "grad_xyz"}});
    if (g_rot) same_device(rot, fn, {{*g_rot, "grad_rotation"}});
    OptTensor dx, dr, ddx, ddr;
    if (want_xyz) dx = at::empty({P, 3}, rot.options());
    if (want_rot) dr = at::empty({P, 4}, rot.options());
    if (want_dxyz) ddx = at::empty({M, 3}, drot.options());
    if (want_drot) ddr = at::empty({M, 4}, drot.options());
    if (P == 0) return {dx, dr, ddx, ddr};
    const Tensor rc = rot.contiguous(), mc = mask.contiguous(), drc = drot.contiguous();
    OptTensor gx, gr;
    if (g_xyz) gx = g_xyz->contiguous();
    if (g_rot) gr = g_rot->contiguous();
    check(igs_gaussian_deform_bwd(c.stream(), (int)P, (int)M, dt, rc.data_ptr<float>(), mc.data_ptr<int64_t>(), drc.data_ptr(),
                                  ptr_or_null<float>(gx), ptr_or_null<float>(gr), ptr_or_null<float>(dx), ptr_or_null<float>(dr),
                                  ptr_or_null(ddx), ptr_or_null(ddr)), "igs_gaussian_deform_bwd");
    return {dx, dr, ddx, ddr};
}

// ---- Adam over lists of tensors (refine_ops.hip) ----
// igs_adam_step_multi (igs_amd/optim.py): one launch for up to 8 parameters
void adam_step_multi(const std::vector<Tensor>& params, const std::vector<Tensor>& grads, const std::vector<Tensor>& exp_avgs,
                     const std::vector<Tensor>& exp_avg_sqs, const std::vector<double>& lrs, const std::vector<double>& bc1,
                     const std::vector<double>& bc2_sqrt, double beta1, double beta2, double eps, const std::vector<Tensor>& steps,
                     const OptTensor& done_scratch)
{
    // `steps` (optional): one float32 GPU scalar per tensor = the step count, advanced on the device (igs_adam_step_multi_dev; bc1 /
    // bc2_sqrt are then ignored) -- the form a hipGraph can replay; `done_scratch`: int32 GPU tensor of
    // igs_adam_step_multi_dev_scratch_words() zeros the caller keeps between calls
    const size_t n = params.size();
    if (n == 0) return;
    const bool dev_step = !steps.empty();
    if (n > 8 || grads.size() != n || exp_avgs.size() != n || exp_avg_sqs.size() != n || lrs.size() != n
        || (dev_step ? steps.size() != n : (bc1.size() != n || bc2_sqrt.size() != n)))
        throw RasterizerError("adam_step_multi: between 1 and 8 tensors, all lists of the same length");
    float* p[8]; const float* g[8]; float* m[8]; float* v[8]; size_t cnt[8]; float lr[8], b1c[8], b2c[8]; float* st[8];
    std::vector<Tensor> keep;
    const char* bad = "adam_step_multi: parameters and state must be contiguous float32 tensors on one GPU (no CPU fallback)";
    const GpuCall c(params[0], bad);
    for (size_t k = 0; k < n; k++) {
        const Tensor& P_ = params[k];
        if (!P_.is_cuda() || P_.device() != c.dev || P_.scalar_type() != at::kFloat || !P_.is_contiguous() || !exp_avgs[k].is_contiguous()
            || !exp_avg_sqs[k].is_contiguous() || grads[k].numel() != P_.numel() || exp_avgs[k].numel() != P_.numel() || exp_avg_sqs[k].numel() != P_.numel())
            throw RasterizerError(bad);
        Tensor G = (grads[k].is_contiguous() && grads[k].scalar_type() == at::kFloat) ? grads[k] : grads[k].to(at::kFloat).contiguous();
        keep.push_back(G);
        p[k] = P_.data_ptr<float>(); g[k] = G.data_ptr<float>(); m[k] = exp_avgs[k].data_ptr<float>(); v[k] = exp_avg_sqs[k].data_ptr<float>();
        cnt[k] = (size_t)P_.numel(); lr[k] = (float)lrs[k];
        if (dev_step) {
            const Tensor& S_ = steps[k];
            if (!S_.is_cuda() || S_.device() != c.dev || S_.scalar_type() != at::kFloat || S_.numel() != 1)
                throw RasterizerError("adam_step_multi: every step count must be a one-element float32 tensor on the parameters' GPU");
            st[k] = S_.data_ptr<float>();
        } else {
            b1c[k] = (float)bc1[k]; b2c[k] = (float)bc2_sqrt[k];
        }
    }
    unsigned* done = nullptr;
    if (dev_step) {
        if (!done_scratch.has_value() || !done_scratch->is_cuda() || done_scratch->device() != c.dev || done_scratch->scalar_type() != at::kInt
            || (size_t)done_scratch->numel() < igs_adam_step_multi_dev_scratch_words() || !done_scratch->is_contiguous())
            throw RasterizerError("adam_step_multi: device-side step counts need `done_scratch`, an int32 tensor of adam_dev_scratch_words() zeros on the parameters' GPU");
        done = (unsigned*)done_scratch->data_ptr<int>();
    }
    const int rc = dev_step ? igs_adam_step_multi_dev(c.stream(), (int)n, p, g, m, v, cnt, lr, st, done, (float)beta1, (float)beta2, (float)eps)
                            : igs_adam_step_multi(c.stream(), (int)n, p, g, m, v, cnt, lr, b1c, b2c, (float)beta1, (float)beta2, (float)eps);
    if (rc != 0) throw RasterizerError("igs_adam_step_multi failed: " + std::to_string(rc));
}

// ---- the two image losses of the refine loop as single calls (refine_ops.hip, loss_ops.hip; igs_amd/losses.py wraps them in autograd Functions) ----
bool stream_is_capturing(hipStream_t stream)
{
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(stream, &st) == hipSuccess && st != hipStreamCaptureStatusNone;
}
// The kernels' small scratch, kept per (device, stream) for the life of the process -- except on a capturing stream, where it must be
// memory the graph owns (allocated here, from the capture's private pool; the L1 words zeroed by a node of the graph).
//   L1: 1024 partial sums | the self-resetting counter words, born zero;  SSIM: igs_ssim_l1_scratch_bytes of the last W x H asked for.
// Get-or-create happens under the table's lock and the Tensor is handed back by value, so host threads that share a stream never
// touch a table entry unlocked, and a caller's scratch outlives its replacement by a thread with another image size.
enum class LossKind { L1, Ssim };
struct LossScratch { Tensor l1; Tensor ssim; int64_t ssim_w = 0, ssim_h = 0; };
Tensor loss_scratch(LossKind kind, const GpuCall& c, hipStream_t stream, int64_t W = 0, int64_t H = 0)
{
    const auto make = [&] {
        return kind == LossKind::L1 ? at::zeros({1024 + 33 * 64}, at::TensorOptions().dtype(at::kFloat).device(c.dev))
                                    : at::empty({(int64_t)igs_ssim_l1_scratch_bytes((int)W, (int)H)}, at::TensorOptions().dtype(at::kByte).device(c.dev));
    };
    if (stream_is_capturing(stream)) return make();
    static std::mutex mu;
    static std::map<std::pair<int, void*>, LossScratch> table;
    std::lock_guard<std::mutex> lock(mu);
    LossScratch& sc = table[{ (int)c.dev.index(), (void*)stream }];
    if (kind == LossKind::L1) {
        if (!sc.l1.defined()) sc.l1 = make();
        return sc.l1;
    }
    if (!sc.ssim.defined() || sc.ssim_w != W || sc.ssim_h != H) {
        sc.ssim = make();
        sc.ssim_w = W; sc.ssim_h = H;
    }
    return sc.ssim;
}

// mean |a - b| and sign(a - b) / n in one launch (igs_l1_mean_fwd_bwd; loss_utils.py:17-18)
std::tuple<Tensor, Tensor> l1_mean(const Tensor& a, const Tensor& b)
{
    const char* bad = "l1_mean: two GPU tensors of the same, non-zero size (no CPU fallback)";
    if (!b.is_cuda() || a.numel() == 0 || a.numel() != b.numel()) throw RasterizerError(bad);
    const GpuCall c(a, bad);
    In x(a, c.dev, "a"), y(b, c.dev, "b");
    hipStream_t stream = c.stream();
    Tensor l1s = loss_scratch(LossKind::L1, c, stream);
    Tensor grad = at::empty_like(x.keep), out = at::empty({}, at::TensorOptions().dtype(at::kFloat).device(c.dev));
    const int rc = igs_l1_mean_fwd_bwd(stream, (size_t)x.keep.numel(), x.p, y.p, grad.data_ptr<float>(), out.data_ptr<float>(),
                                       l1s.data_ptr<float>(), (unsigned*)(l1s.data_ptr<float>() + 1024));
    if (rc != 0) throw RasterizerError("igs_l1_mean_fwd_bwd failed: " + std::to_string(rc));
    return { out, grad };
}

// mean SSIM(a, b) over all elements (finished on the device) and d(mean SSIM)/da in two launches (igs_ssim_mean_fwd_bwd; loss_utils.py:34-63 with the 11x11 window).  a, b: [3, H, W] (or anything that reshapes to it)
std::tuple<Tensor, Tensor> ssim_mean(const Tensor& a, const Tensor& b)
{
    const char* bad = "ssim_mean: two GPU images of the same size (no CPU fallback)";
    if (!b.is_cuda() || a.dim() < 3 || a.numel() != b.numel()) throw RasterizerError(bad);
    const GpuCall c(a, bad);
    In x(a, c.dev, "a"), y(b, c.dev, "b");
    const int64_t H = a.size(-2), W = a.size(-1);
    if (a.numel() != 3 * H * W) throw RasterizerError("ssim_mean: one 3-channel image per side");
    hipStream_t stream = c.stream();
    Tensor scratch = loss_scratch(LossKind::Ssim, c, stream, W, H);
    Tensor grad = at::empty_like(x.keep), mean = at::empty({}, at::TensorOptions().dtype(at::kFloat).device(c.dev));
    const int rc = igs_ssim_mean_fwd_bwd(stream, (int)W, (int)H, x.p, y.p, scratch.data_ptr(), grad.data_ptr<float>(), mean.data_ptr<float>());
    if (rc != 0) throw RasterizerError("igs_ssim_mean_fwd_bwd failed: " + std::to_string(rc));
    return { mean, grad };               // grad = d(mean SSIM)/da
}

// ---- the AGM-Net training loss (ssim_batch.hip) ----
// (means [N + 1], l1_means [N + 1] | None, grad [N, C, H, W] | None, ssim_map [N, C, H, W] | None) of two [N, C, H, W] float32 batches
// (igs_ssim_batch_fwd_bwd; loss_utils.py:17-18,33-63, main.py:252-265): means[n] = mean SSIM of image n, means[N] = their mean;
// grad[n] = c_ssim * d means[n] / d a + c_l1 * d l1_means[n] / d a.  The scratch is this call's own, from the caching allocator (the
// stream-ordered free keeps it alive for the launches; under capture it belongs to the graph's pool)
int64_t ssim_batch_scratch_bytes(int64_t W, int64_t H, int64_t N, int64_t C, bool want_grad)
{
    if (W > INT_MAX || H > INT_MAX || N > INT_MAX || C > INT_MAX) return -1;
    return igs_ssim_batch_scratch_bytes((int)W, (int)H, (int)N, (int)C, want_grad ? 1 : 0);
}
std::tuple<Tensor, OptTensor, OptTensor, OptTensor> ssim_batch(const Tensor& a, const Tensor& b, double c_ssim, double c_l1, bool want_grad,
                                                                bool want_map, bool want_l1)
{
    const char* fn = "ssim_batch";
    expect(a, fn, "a", at::kFloat, {-1, -1, -1, -1});
    expect(b, fn, "b", at::kFloat, {a.size(0), a.size(1), a.size(2), a.size(3)});
    const int64_t N = a.size(0), C = a.size(1), H = a.size(2), W = a.size(3);
    const int64_t bytes = ssim_batch_scratch_bytes(W, H, N, C, want_grad);
    if (bytes < 0)
        throw RasterizerError(std::string(fn) + ": sizes out of range for " + c10::str(a.sizes()) + " (every size >= 1, N * C <= " +
                              std::to_string(IGS_SSIM_BATCH_MAX_PLANES) + ", 8 * N * C * ceil(ceil(H / 32) / 8) * ceil(W / 32) < 2^31)");
    const GpuCall c(a, fn, "a", {{b, "b"}});
    const auto fo = a.options();
    Tensor means = at::empty({N + 1}, fo);
    OptTensor l1_means, grad, map;
    if (want_l1) l1_means = at::empty({N + 1}, fo);
    if (want_grad) grad = at::empty({N, C, H, W}, fo);
    if (want_map) map = at::empty({N, C, H, W}, fo);
    const Tensor scratch = at::empty({bytes}, a.options().dtype(at::kByte));
    const Tensor x = a.contiguous(), y = b.contiguous();
    check(igs_ssim_batch_fwd_bwd(c.stream(), (int)W, (int)H, (int)N, (int)C, x.data_ptr<float>(), y.data_ptr<float>(), (float)c_ssim, (float)c_l1,
                                 scratch.data_ptr(), means.data_ptr<float>(), ptr_or_null<float>(l1_means), ptr_or_null<float>(grad),
                                 ptr_or_null<float>(map)),
          "igs_ssim_batch_fwd_bwd");
    return {means, l1_means, grad, map};
}

// ---- the module ----
// m.def for a function that runs with the GIL released: every function that reaches a kernel (host threads drive streams side by side)
using namespace pybind11::literals;      // "name"_a = py::arg("name")
template <class F, class... Extra> void def_nogil(py::module_& m, const char* name, F&& f, const Extra&... extra)
{
    m.def(name, std::forward<F>(f), extra..., py::call_guard<py::gil_scoped_release>());
}
// the names of backward_body's parameters, in its order; `more` appends _ex's two options
template <class F, class... More> void def_backward(py::module_& m, const char* name, F f, const More&... more)
{
    const auto none = py::none();
    def_nogil(m, name, f, "background"_a, "means3D"_a, "radii"_a, "colors"_a, "scales"_a, "rotations"_a, "scale_modifier"_a, "cov3D_precomp"_a,
              "viewmatrix"_a, "projmatrix"_a, "tan_fovx"_a, "tan_fovy"_a, "kernel_size"_a, "dL_dout_color"_a, "dL_dout_coord"_a, "dL_dout_mcoord"_a,
              "dL_dout_depth"_a, "dL_dout_mdepth"_a, "dL_dout_alpha"_a, "dL_dout_normal"_a, "normalmap"_a, "sh"_a, "degree"_a, "campos"_a,
              "geomBuffer"_a, "R"_a, "binningBuffer"_a, "imageBuffer"_a, "alphas"_a, "require_coord"_a, "require_depth"_a, "debug"_a, py::kw_only(),
              "workspace"_a = none, "out_means2D"_a = none, "out_colors"_a = none, "out_opacity"_a = none, "out_means3D"_a = none,
              "out_cov3D"_a = none, "out_sh"_a = none, "out_scales"_a = none, "out_rotations"_a = none, more...);
}

}      // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m)
{
    py::register_exception<RasterizerError>(m, "RasterizerError", PyExc_RuntimeError);
    py::register_exception<NotImplemented>(m, "NotImplementedDtype", PyExc_NotImplementedError);
    py::class_<ScratchSet, std::shared_ptr<ScratchSet>>(m, "ScratchSet")
        .def(py::init([](const py::object& device, bool persistent) {
                 return std::make_shared<ScratchSet>(torch::python::detail::py_object_to_device(device), persistent);
             }), "device"_a, "persistent"_a = true)
        .def_readonly("geom", &ScratchSet::geom).def_readonly("binning", &ScratchSet::binning).def_readonly("img", &ScratchSet::img)
        .def_readonly("persistent", &ScratchSet::persistent)
        .def("workspace", [](ScratchSet& s, int64_t P) { return s.ensure_workspace(P); }, "P"_a)
        // (callback address, user word) x 3 for callers that fill a C struct themselves (igs_refine_step_args through ctypes);
        // valid for as long as this object lives
        .def("callbacks", [](ScratchSet& s) {
            return std::make_tuple((uintptr_t)&grow_cb, (uintptr_t)&s.g_geom, (uintptr_t)&s.g_binning, (uintptr_t)&s.g_img);
        });

    const auto none = py::none();
    using Backward = BackwardFns<decltype(backward_body)>;
    def_nogil(m, "rasterize_gaussians", &rasterize_gaussians, "background"_a, "means3D"_a, "colors"_a, "opacity"_a, "scales"_a, "rotations"_a,
              "scale_modifier"_a, "cov3D_precomp"_a, "viewmatrix"_a, "projmatrix"_a, "tan_fovx"_a, "tan_fovy"_a, "kernel_size"_a, "image_height"_a,
              "image_width"_a, "sh"_a, "degree"_a, "campos"_a, "prefiltered"_a, "require_coord"_a, "require_depth"_a, "debug"_a, py::kw_only(),
              "scratch"_a = std::shared_ptr<ScratchSet>(), "out_images"_a = none, "out_radii"_a = none, "mode"_a = 0, "scratch_clean"_a = false);
    def_backward(m, "rasterize_gaussians_backward", &Backward::plain);
    def_backward(m, "rasterize_gaussians_backward_ex", &Backward::ex, "nan_report"_a = 0, "clamp"_a = 0.0);
    def_nogil(m, "nan_report_wait", [](int64_t word, int64_t seq) {
        const int v = igs_rast_nan_report_wait_at((const void*)(uintptr_t)word, (unsigned)seq);
        check(v, "igs_rast_nan_report_wait_at");
        return v != 0;
    }, "word"_a, "seq"_a);
    py::module_ vw = m.def_submodule("_views", "V views of one Gaussian set in one call (api.hip, geom_bwd.hip)");
    def_nogil(vw, "rasterize_views", &rasterize_views, "background"_a, "means3D"_a, "colors"_a, "opacity"_a, "scales"_a, "rotations"_a,
              "scale_modifier"_a, "cov3D_precomp"_a, "viewmatrices"_a, "projmatrices"_a, "tan_fovx"_a, "tan_fovy"_a, "kernel_size"_a, "image_height"_a,
              "image_width"_a, "sh"_a, "degree"_a, "camposes"_a, "prefiltered"_a, "require_coord"_a, "require_depth"_a, "debug"_a, py::kw_only(),
              "scratch"_a, "scratch_clean"_a = false);
    def_nogil(vw, "rasterize_views_backward", &rasterize_views_backward, "background"_a, "means3D"_a, "radii"_a, "colors"_a, "scales"_a, "rotations"_a,
              "scale_modifier"_a, "cov3D_precomp"_a, "viewmatrices"_a, "projmatrices"_a, "tan_fovx"_a, "tan_fovy"_a, "kernel_size"_a, "dL_dout_color"_a,
              "dL_dout_coord"_a, "dL_dout_mcoord"_a, "dL_dout_depth"_a, "dL_dout_mdepth"_a, "dL_dout_alpha"_a, "dL_dout_normal"_a, "normalmap"_a, "sh"_a,
              "degree"_a, "camposes"_a, "scratch"_a, "R"_a, "alphas"_a, "require_coord"_a, "require_depth"_a, "debug"_a, py::kw_only(),
              "want_means2D"_a = true, "nan_report"_a = 0, "clamp"_a = 0.0);
    vw.def("views_max", []() { return igs_rast_views_max(); });
    def_nogil(m, "count_gaussians", &count_gaussians, "background"_a, "means3D"_a, "colors"_a, "opacity"_a, "scales"_a, "rotations"_a,
              "scale_modifier"_a, "cov3D_precomp"_a, "viewmatrix"_a, "projmatrix"_a, "tan_fovx"_a, "tan_fovy"_a, "image_height"_a, "image_width"_a,
              "sh"_a, "degree"_a, "campos"_a, "prefiltered"_a, "debug"_a, "f_count"_a, py::kw_only(), "scratch"_a = std::shared_ptr<ScratchSet>());
    def_nogil(m, "mark_visible", &mark_visible, "means3D"_a, "viewmatrix"_a, "projmatrix"_a);
    def_nogil(m, "distCUDA2", &distCUDA2, "points"_a);
    def_nogil(m, "anchors_bbox_select", &anchors_bbox_select, "xyz"_a, "ptr"_a, "box"_a);
    def_nogil(m, "anchors_fps", &anchors_fps, "xyz"_a, "ptr"_a, "start"_a, "out_ptr"_a, "total"_a, "max_n"_a, "init_d2"_a);
    def_nogil(m, "anchors_knn", &anchors_knn, "x"_a, "y"_a, "ptr_x"_a, "ptr_y"_a, "k"_a, "with_d2"_a = false, "weight_scale"_a = none);
    def_nogil(m, "motion_interp_fwd", &motion_interp_fwd, "features"_a, "col"_a, "weights"_a);
    def_nogil(m, "motion_interp_index", &motion_interp_index, "col"_a, "A"_a, "D"_a);
    def_nogil(m, "motion_interp_bwd", &motion_interp_bwd, "features"_a, "weights"_a, "grad_out"_a, "index"_a, "want_features"_a = true,
              "want_weights"_a = true);
    def_nogil(m, "motion_lift_fwd", &motion_lift_fwd, "motion_feature"_a, "anchor_points"_a, "w2c"_a, "intrinsics"_a);
    def_nogil(m, "motion_lift_bwd", &motion_lift_bwd, "grad_out"_a, "anchor_points"_a, "w2c"_a, "intrinsics"_a, "H"_a, "W"_a, "half"_a = false);
    def_nogil(m, "cond_ray_fwd", &cond_ray_fwd, "rays"_a, "depth"_a);
    def_nogil(m, "modln_fwd", &modln_fwd, "x"_a, "mod"_a, "weight"_a, "bias"_a, "eps"_a = 1e-6, "save_stats"_a = false);
    def_nogil(m, "modln_bwd", &modln_bwd, "x"_a, "mod"_a, "weight"_a, "bias"_a, "mean"_a, "rstd"_a, "grad_out"_a, "want_x"_a = true,
              "want_mod"_a = true, "want_weight"_a = true, "want_bias"_a = true);
    def_nogil(m, "attn_fwd", &attn_fwd, "q"_a, "k"_a, "v"_a, "scale"_a, "token_major"_a = false, "want_lse"_a = false);
    def_nogil(m, "attn_bwd", &attn_bwd, "q"_a, "k"_a, "v"_a, "out"_a, "lse"_a, "grad_out"_a, "scale"_a, "token_major"_a = false, "want_q"_a = true,
              "want_k"_a = true, "want_v"_a = true);
    // the window attention lives in a private submodule: the top-level names of `_C` are a pinned list (tests/test_ext_binding_host.py)
    py::module_ wa = m.def_submodule("_window", "swin window attention (wattn.hip)");
    def_nogil(wa, "window_attn_fwd", &window_attn_fwd, "q"_a, "k"_a, "v"_a, "h"_a, "w"_a, "num_splits"_a = 1, "with_shift"_a = false,
              "scale"_a = 0.08838834764831845, "want_lse"_a = false);
    def_nogil(wa, "window_attn_bwd", &window_attn_bwd, "q"_a, "k"_a, "v"_a, "out"_a, "lse"_a, "grad_out"_a, "h"_a, "w"_a, "num_splits"_a = 1,
              "with_shift"_a = false, "scale"_a = 0.08838834764831845, "want_q"_a = true, "want_k"_a = true, "want_v"_a = true);
    // ... and so do the encoder's norms and position add
    py::module_ en = m.def_submodule("_encoder", "unimatch CNN encoder: fused instance norms and position add (inorm.hip)");
    def_nogil(en, "instance_norm_fwd", &instance_norm_fwd, "x"_a, "skip"_a = none, "mode"_a = 0, "eps"_a = 1e-5, "inplace"_a = false);
    def_nogil(en, "position_add", &position_add, "feature0"_a, "feature1"_a, "splits"_a, "inplace"_a = false);
    en.def("resident_max", [](int64_t dtype, int64_t mode) { return (int64_t)igs_instance_norm_resident_max((int)dtype, (int)mode); }, "dtype"_a, "mode"_a);
    // ... and the transformers' LayerNorm and GEGLU
    py::module_ tk = m.def_submodule("_tokens", "LayerNorm and GEGLU of the two transformers (tokens.hip)");
    def_nogil(tk, "layer_norm_fwd", &layer_norm_fwd, "x"_a, "weight"_a = none, "bias"_a = none, "eps"_a = 1e-5, "residual"_a = none, "out_half"_a = false);
    def_nogil(tk, "layer_norm_bwd", &layer_norm_bwd, "x"_a, "weight"_a, "eps"_a, "grad_out"_a, "want_x"_a = true, "want_weight"_a = true,
              "want_bias"_a = true);
    def_nogil(tk, "geglu_fwd", &geglu_fwd, "proj"_a);
    def_nogil(tk, "geglu_bwd", &geglu_bwd, "proj"_a, "grad_out"_a);
    // ... and the two ends of Transformer1D
    py::module_ gn = m.def_submodule("_gnorm", "GroupNorm to token-major and token-major plus residual: the ends of Transformer1D (gnorm.hip)");
    def_nogil(gn, "group_norm_tokens_fwd", &group_norm_tokens_fwd, "x"_a, "num_groups"_a, "weight"_a = none, "bias"_a = none, "eps"_a = 1e-5, "out_half"_a = false);
    def_nogil(gn, "group_norm_tokens_bwd", &group_norm_tokens_bwd, "x"_a, "num_groups"_a, "weight"_a, "stats"_a, "grad_out"_a, "want_x"_a = true,
              "want_weight"_a = true, "want_bias"_a = true);
    def_nogil(gn, "tokens_add_residual", &tokens_add_residual, "tokens"_a, "residual"_a, "out_half"_a = false);
    // ... and the residual decoder
    py::module_ cf = m.def_submodule("_cond", "condition3D in one launch, ModLN's MLP included, and its backward (cond_fused.hip, cond_fused_bwd.hip)");
    def_nogil(cf, "condition3d_fwd", &condition3d_fwd, "x"_a, "rays"_a, "depth"_a, "wpack"_a, "bpack"_a, "hidden"_a, "weight"_a, "bias"_a, "eps"_a = 1e-6);
    def_nogil(cf, "pack_elems", &cond_fused_pack_elems, "C"_a, "hidden"_a, "half"_a = false);
    def_nogil(cf, "condition3d_bwd", &condition3d_bwd, "x"_a, "rays"_a, "depth"_a, "wpack"_a, "wpack_t"_a, "bpack"_a, "hidden"_a, "weight"_a, "bias"_a,
              "eps"_a, "grad_out"_a, "want_x"_a = true, "want_w1"_a = true, "want_b1"_a = true, "want_w2"_a = true, "want_b2"_a = true,
              "want_weight"_a = true, "want_bias"_a = true);
    def_nogil(cf, "bwd_scratch_bytes", &cond_fused_bwd_scratch_bytes, "N"_a, "C"_a, "hidden"_a, "H"_a, "W"_a);
    py::module_ uc = m.def_submodule("_upconv", "2x bilinear upsample + 3x3 convolution in one launch (upconv.hip)");
    def_nogil(uc, "upconv_fwd", &upconv_fwd, "x"_a, "wpack"_a, "bpack"_a, "Cout"_a);
    def_nogil(uc, "upconv_bwd", &upconv_bwd, "x"_a, "wpack_t"_a, "dout"_a, "want_x"_a, "want_w"_a, "want_b"_a);
    def_nogil(uc, "pack_elems", &upconv_pack_elems, "Cin"_a, "Cout"_a, "half"_a = false);
    py::module_ ml = m.def_submodule("_mlp", "the residual decoder: MLP and output heads in one launch (mlp.hip)");
    def_nogil(ml, "mlp_heads_fwd", &mlp_heads_fwd, "x"_a, "wpack"_a, "bpack"_a, "widths"_a, "act_after"_a, "head_widths"_a, "act"_a = 0);
    ml.def("pack_elems", &mlp_pack_elems, "widths"_a, "head_widths"_a);
    def_nogil(ml, "mlp_heads_bwd", &mlp_heads_bwd, "x"_a, "wpack"_a, "wpack_t"_a, "bpack"_a, "widths"_a, "act_after"_a, "head_widths"_a, "act"_a, "douts"_a,
              "want_x"_a = true, "want_w"_a = true, "want_b"_a = true);
    ml.def("bwd_scratch_bytes", &mlp_bwd_scratch_bytes, "N"_a, "half"_a, "widths"_a, "head_widths"_a);
    py::module_ ff = m.def_submodule("_ffn", "the tail of a unimatch TransformerLayer in one launch: merge, LayerNorms and FFN (ffn.hip)");
    def_nogil(ff, "layer_tail_fwd", &layer_tail_fwd, "attn_out"_a, "source"_a, "wpack"_a, "hidden"_a, "ln1_w"_a, "ln1_b"_a, "eps1"_a, "ln2_w"_a = none,
              "ln2_b"_a = none, "eps2"_a = 1e-5, "out_half"_a = false);
    def_nogil(ff, "pack_elems", &layer_tail_pack_elems, "hidden"_a, "has_ffn"_a = true);
    def_nogil(ff, "layer_tail_bwd", &layer_tail_bwd, "attn_out"_a, "source"_a, "dout"_a, "wpack"_a, "wpack_t"_a, "hidden"_a, "ln1_w"_a, "ln1_b"_a, "eps1"_a,
              "ln2_w"_a, "ln2_b"_a, "eps2"_a, "want"_a, "da_half"_a = false, "ds_half"_a = false);
    ff.def("bwd_scratch_bytes", &layer_tail_bwd_scratch_bytes, "T"_a, "half"_a, "hidden"_a);
    py::module_ pj = m.def_submodule("_proj", "the q / k / v projections of the unimatch TransformerLayers in one launch (proj.hip)");
    def_nogil(pj, "token_proj_fwd", &token_proj_fwd, "x"_a, "wpack"_a, "n"_a, "rot"_a = std::vector<int64_t>(), "out_half"_a = false);
    def_nogil(pj, "pack_elems", &token_proj_pack_elems, "n"_a);
    def_nogil(pj, "token_proj_bwd", &token_proj_bwd, "x"_a, "grads"_a, "wpack_t"_a, "rot"_a, "want_dx"_a, "want_dw"_a, "dx_half"_a = false);
    def_nogil(pj, "bwd_scratch_bytes", &token_proj_bwd_scratch_bytes, "T"_a, "n"_a);
    py::module_ ls = m.def_submodule("_loss", "SSIM and L1 of a batch of images: the AGM-Net training loss (ssim_batch.hip)");
    def_nogil(ls, "ssim_batch", &ssim_batch, "a"_a, "b"_a, "c_ssim"_a, "c_l1"_a, "want_grad"_a, "want_map"_a, "want_l1"_a);

    def_nogil(m, "motion_deform_fwd", &motion_deform_fwd, "xyz"_a, "rotation"_a, "mask"_a, "res_xyz"_a, "res_rotation"_a);
    def_nogil(m, "motion_deform_bwd", &motion_deform_bwd, "rotation"_a, "mask"_a, "res_xyz"_a, "res_rotation"_a, "grad_xyz"_a, "grad_rotation"_a,
              "want_xyz"_a = true, "want_rotation"_a = true, "want_res_xyz"_a = true, "want_res_rotation"_a = true);
    def_nogil(m, "adam_step_multi", &adam_step_multi, "params"_a, "grads"_a, "exp_avgs"_a, "exp_avg_sqs"_a, "lrs"_a, "bias_correction1"_a,
              "bias_correction2_sqrt"_a, "beta1"_a, "beta2"_a, "eps"_a, "steps"_a = std::vector<Tensor>(), "done_scratch"_a = none);
    def_nogil(m, "l1_mean", &l1_mean, "a"_a, "b"_a);
    def_nogil(m, "ssim_mean", &ssim_mean, "a"_a, "b"_a);
    // the four that keep the GIL: they touch Python objects or never reach a kernel
    m.def("integrate_gaussians_to_points", [](const py::args&, const py::kwargs&) -> py::object {
        // GOF tetrahedra integration (DGR/rasterize_points.cu:269-387): mesh extraction only, never reached from IGS
        PyErr_SetString(PyExc_NotImplementedError, "integrate_gaussians_to_points is outside the IGS hot path and is not implemented");
        throw py::error_already_set();
    });
    m.def("forward_finish", []() -> py::object {
        const int rc = igs_rast_forward_finish();
        if (rc == IGS_RAST_E_RETRY) return py::none();
        check(rc, "igs_rast_forward_finish");
        return py::int_(rc);
    });
    m.def("adam_dev_scratch_words", []() { return (int64_t)igs_adam_step_multi_dev_scratch_words(); });
    m.def("abi_version", []() { return igs_rast_version(); });
}
