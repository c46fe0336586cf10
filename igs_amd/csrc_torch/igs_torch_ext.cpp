// igs_torch_ext.cpp -- the compiled `_C` module of the drop-in packages: the four functions the reference's pybind module exports
// (DGR/ext.cpp:15-20; DGR = submodules/RaDe-GS/submodules/diff-gaussian-rasterization) as torch glue over the C ABI of
// include/igs_rast.h.  Counterpart of DGR/rasterize_points.cu:35-267 (RasterizeGaussiansCUDA, RasterizeGaussiansBackwardCUDA,
// markVisible): tensor checks, output allocation, pointer extraction, PyTorch's CURRENT stream -- no arithmetic.
//
// Built by igs_amd/build_ext.py with the host compiler (no device code in this file); links libigs_rast.so.
//
// It also carries count_gaussians, the count pass of the compress package (compress-diff-gaussian-rasterization rasterize_points.cu:130-217).
// And distCUDA2, the one function of simple-knn (mean squared distance to the three nearest neighbours, create_from_pcd's initial scales).
// And the anchor graph natives under the torch_cluster / fpsample drop-ins and igs_amd.anchors: anchors_bbox_select, anchors_fps,
// anchors_knn (fixed output shapes, no host synchronisation).
// And the two consumers of the anchor graph under igs_amd.motion: motion_interp_fwd / _index / _bwd (anchor feature interpolation) and
// motion_deform_fwd / _bwd (GaussianModel.deform); unsupported dtypes raise NotImplementedError.
// And IGS.condition3D's native parts: cond_ray_fwd (the ray / depth condition) and modln_fwd / modln_bwd (LayerNorm + adaLN modulation).
// And the anchor transformer's fused attention: attn_fwd / attn_bwd (attn.hip) on [B, H, A, 64] views of any acceptable strides.
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

void check(int rc, const char* what)
{
    if (rc < 0) throw RasterizerError(std::string(what) + " failed (" + std::to_string(rc) + "): " + igs_rast_last_error());
}

// what rasterize_gaussians and count_gaussians share: checks, device guard, the eleven float inputs, M, scratch set, current stream
struct FwdCall {
    c10::Device dev; c10::hip::HIPGuardMasqueradingAsCUDA guard; int64_t P, H, W;
    In m3, col, op, sc, rot, cov, shs, bg, view, proj, cam; int64_t M; std::shared_ptr<ScratchSet> ss; hipStream_t stream;
    static const Tensor& points(const Tensor& means3D)
    {
        if (means3D.dim() != 2 || means3D.size(1) != 3) throw RasterizerError("means3D must have dimensions (num_points, 3)");
        if (!means3D.is_cuda()) throw RasterizerError("igs_amd rasterizer: tensors must be on a GPU (no CPU fallback)");
        return means3D;
    }
    FwdCall(const Tensor& background, const Tensor& means3D, const Tensor& colors, const Tensor& opacity, const Tensor& scales,
            const Tensor& rotations, const Tensor& cov3D_precomp, const Tensor& viewmatrix, const Tensor& projmatrix, const Tensor& sh,
            const Tensor& campos, int64_t image_height, int64_t image_width, const std::shared_ptr<ScratchSet>& scratch)
        : dev(points(means3D).device()), guard(dev), P(means3D.size(0)), H(image_height), W(image_width),
          m3(means3D, dev, "means3D"), col(colors, dev, "colors_precomp"), op(opacity, dev, "opacities"), sc(scales, dev, "scales"),
          rot(rotations, dev, "rotations"), cov(cov3D_precomp, dev, "cov3D_precomp"), shs(sh, dev, "shs"), bg(background, dev, "bg"),
          view(viewmatrix, dev, "viewmatrix"), proj(projmatrix, dev, "projmatrix"), cam(campos, dev, "campos"), M(shs.p ? shs.keep.size(1) : 0),
          ss(scratch ? scratch : std::make_shared<ScratchSet>(dev, false)), stream(c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(dev.index()).stream())
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
        rendered = fwd(c.stream, grow_cb, &c.ss->g_geom, grow_cb, &c.ss->g_binning, grow_cb, &c.ss->g_img, (int)P, (int)degree, (int)c.M, c.bg.p,
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
        rendered = igs_rast_count_gaussians(c.stream, grow_cb, &c.ss->g_geom, grow_cb, &c.ss->g_binning, grow_cb, &c.ss->g_img, (int)P, (int)degree,
                                            (int)c.M, c.bg.p, (int)W, (int)H, c.m3.p, c.shs.p, c.col.p, c.op.p, c.sc.p, (float)scale_modifier,
                                            c.rot.p, c.cov.p, c.view.p, c.proj.p, c.cam.p, (float)tan_fovx, (float)tan_fovy, prefiltered ? 1 : 0,
                                            color.data_ptr<float>(), count.data_ptr<int>(), score.data_ptr<float>(), radii.data_ptr<int>(),
                                            debug ? 1 : 0);
        check((int)rendered, "igs_rast_count_gaussians");
    }
    return CountTuple(count, score, rendered, color, radii, c.ss->geom, c.ss->binning, c.ss->img);
}

using BwdTuple = std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor>;

// Body of _C.rasterize_gaussians_backward (RasterizeGaussiansBackwardCUDA, DGR/rasterize_points.cu:135-246).  The seven small
// gradients are carved from ONE [23 P] block (m2d 3 | colors 3 | opacity 1 | means3D 3 | scales 3 | rot 4 | cov3D 6); every element is
// written by the kernels (no zero fills).  Returns the reference's 8-tuple and, with nan_report, whether a NaN was written.
struct BwdResult { BwdTuple grads; int64_t nan = 0; int64_t nan_word = 0; int64_t nan_seq = 0; };
BwdResult backward_body(
    const Tensor& background, const Tensor& means3D, const Tensor& radii, const Tensor& colors, const Tensor& scales, const Tensor& rotations,
    double scale_modifier, const Tensor& cov3D_precomp, const Tensor& viewmatrix, const Tensor& projmatrix, double tan_fovx, double tan_fovy,
    double kernel_size, const OptTensor& dL_dout_color, const OptTensor& dL_dout_coord, const OptTensor& dL_dout_mcoord,
    const OptTensor& dL_dout_depth, const OptTensor& dL_dout_mdepth, const OptTensor& dL_dout_alpha, const OptTensor& dL_dout_normal,
    const Tensor& normalmap, const Tensor& sh, int64_t degree, const Tensor& campos, const Tensor& geomBuffer, int64_t R,
    const Tensor& binningBuffer, const Tensor& imageBuffer, const Tensor& alphas, bool require_coord, bool require_depth, bool debug,
    const OptTensor& workspace, const OptTensor& out_means2D, const OptTensor& out_colors, const OptTensor& out_opacity,
    const OptTensor& out_means3D, const OptTensor& out_cov3D, const OptTensor& out_sh, const OptTensor& out_scales,
    const OptTensor& out_rotations, int64_t nan_report, double clamp)
{
    if (!means3D.is_cuda()) throw RasterizerError("igs_amd rasterizer: tensors must be on a GPU (no CPU fallback)");
    const c10::Device dev = means3D.device();
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
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
        hipStream_t stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(dev.index()).stream();
        if (nan_report || clamp > 0.0) igs_rast_next_backward_options(nan_report ? 1 : 0, (float)clamp);
        auto bp = [](const Tensor& t) { return t.numel() ? (const char*)t.data_ptr() : nullptr; };
        const int rc = igs_rast_backward(
            stream, (int)P, (int)degree, (int)M, (int)std::min<int64_t>(R, INT_MAX), bg.p, (int)W, (int)H, m3.p, shs.p, col.p, al.p, sc.p,
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

// _C.mark_visible (DGR/rasterize_points.cu:248-267)
Tensor mark_visible(const Tensor& means3D, const Tensor& viewmatrix, const Tensor& projmatrix)
{
    if (!means3D.is_cuda()) throw RasterizerError("igs_amd rasterizer: tensors must be on a GPU (no CPU fallback)");
    const c10::Device dev = means3D.device();
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    const int64_t P = means3D.size(0);
    Tensor present = at::zeros({P}, at::TensorOptions().dtype(at::kBool).device(dev));
    if (P != 0) {
        In m(means3D, dev, "means3D"), v(viewmatrix, dev, "viewmatrix"), p(projmatrix, dev, "projmatrix");
        check(igs_rast_mark_visible(c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(dev.index()).stream(), (int)P, m.p, v.p, p.p, (uint8_t*)present.data_ptr()),
              "igs_rast_mark_visible");
    }
    return present;
}

// simple_knn._C.distCUDA2 (simple-knn ext.cpp / spatial.cu): mean squared distance of every point to its three nearest neighbours
Tensor distCUDA2(const Tensor& points)
{
    if (points.scalar_type() != at::kFloat)
        throw RasterizerError(std::string("distCUDA2: points must be float32 (got ") + c10::toString(points.scalar_type()) + ")");
    if (points.dim() != 2 || points.size(1) != 3) throw RasterizerError("distCUDA2: points must have shape [N, 3] (got " + c10::str(points.sizes()) + ")");
    const int64_t P = points.size(0);
    if (P > IGS_KNN_MAX_POINTS)
        throw RasterizerError("distCUDA2: " + std::to_string(P) + " points is more than the supported " + std::to_string(IGS_KNN_MAX_POINTS));
    if (!points.is_cuda()) throw RasterizerError("distCUDA2: points must be on a GPU (no CPU fallback)");
    const c10::Device dev = points.device();
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    Tensor out = at::empty({P}, points.options());
    if (P == 0) return out;
    const Tensor xyz = points.contiguous();
    Tensor scratch = at::empty({(int64_t)igs_knn_scratch_bytes((int)P)}, at::TensorOptions().dtype(at::kByte).device(dev));
    check(igs_knn_mean_dist2(c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(dev.index()).stream(), (int)P, xyz.data_ptr<float>(),
                             scratch.data_ptr(), out.data_ptr<float>()), "igs_knn_mean_dist2");
    return out;
}

// ---- the anchor graph (anchors.hip; contracts in include/igs_rast.h) ----
static void check_points(const Tensor& t, const char* fn, const char* name)
{
    if (t.scalar_type() != at::kFloat)
        throw RasterizerError(std::string(fn) + ": " + name + " must be float32 (got " + c10::toString(t.scalar_type()) + ")");
    if (t.dim() != 2 || t.size(1) != 3)
        throw RasterizerError(std::string(fn) + ": " + name + " must have shape [N, 3] (got " + c10::str(t.sizes()) + ")");
    if (t.size(0) > IGS_ANCHOR_MAX_POINTS)
        throw RasterizerError(std::string(fn) + ": " + std::to_string(t.size(0)) + " points is more than the supported " + std::to_string(IGS_ANCHOR_MAX_POINTS));
}
static void require_gpu(const Tensor& t, const char* fn, const char* name)      // after the argument checks
{
    if (!t.is_cuda()) throw RasterizerError(std::string(fn) + ": " + name + " must be on a GPU (no CPU fallback)");
}
static Tensor offsets_i32(const Tensor& t, const char* fn, const char* name, const Tensor& like, int64_t n)
{
    if (t.dim() != 1 || t.size(0) != n)
        throw RasterizerError(std::string(fn) + ": " + name + " must have shape [" + std::to_string(n) + "] (got " + c10::str(t.sizes()) + ")");
    if (t.device() != like.device()) throw RasterizerError(std::string(fn) + ": " + name + " must be on the points' device");
    return t.to(at::kInt).contiguous();
}
static hipStream_t cur_stream(const c10::Device& dev) { return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(dev.index()).stream(); }

// select_points_bbox for B examples at once: (xyz_in_box [N, 3], index inside the example [N] int64, count [B] int32); the first
// sum(count) rows are example 0's in-box points in index order, then example 1's, ...
std::tuple<Tensor, Tensor, Tensor> anchors_bbox_select(const Tensor& xyz, const Tensor& ptr, const Tensor& box)
{
    check_points(xyz, "anchors_bbox_select", "xyz");
    const int64_t B = ptr.dim() == 1 ? ptr.size(0) - 1 : -1;
    if (B < 1 || B > IGS_ANCHOR_MAX_EXAMPLES) throw RasterizerError("anchors_bbox_select: ptr must have shape [B + 1], 1 <= B <= IGS_ANCHOR_MAX_EXAMPLES");
    if (box.scalar_type() != at::kFloat || box.numel() != B * 6 || box.device() != xyz.device())
        throw RasterizerError("anchors_bbox_select: box must be float32 [B, 2, 3] on the points' device");
    require_gpu(xyz, "anchors_bbox_select", "xyz");
    const c10::Device dev = xyz.device();
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    const int64_t N = xyz.size(0);
    const Tensor p = offsets_i32(ptr, "anchors_bbox_select", "ptr", xyz, B + 1), bx = box.contiguous(), x = xyz.contiguous();
    Tensor out_xyz = at::empty({N, 3}, xyz.options()), out_idx = at::empty({N}, xyz.options().dtype(at::kLong));
    Tensor count = at::empty({B}, xyz.options().dtype(at::kInt));
    Tensor scratch = at::empty({(int64_t)igs_bbox_select_scratch_bytes((int)N)}, xyz.options().dtype(at::kByte));
    check(igs_bbox_select(cur_stream(dev), (int)B, (int)N, x.data_ptr<float>(), p.data_ptr<int>(), bx.data_ptr<float>(), scratch.data_ptr(),
                          out_xyz.data_ptr<float>(), out_idx.data_ptr<int64_t>(), count.data_ptr<int>()), "igs_bbox_select");
    return {out_xyz, out_idx, count};
}

// farthest-point sampling: `total` samples, example b's at [out_ptr[b], out_ptr[b + 1]) (indices into xyz, selection order); max_n
// bounds every example's size
Tensor anchors_fps(const Tensor& xyz, const Tensor& ptr, const Tensor& start, const Tensor& out_ptr, int64_t total, int64_t max_n, double init_d2)
{
    check_points(xyz, "anchors_fps", "xyz");
    const int64_t B = ptr.dim() == 1 ? ptr.size(0) - 1 : -1;
    if (B < 1 || B > IGS_ANCHOR_MAX_EXAMPLES) throw RasterizerError("anchors_fps: ptr must have shape [B + 1], 1 <= B <= IGS_ANCHOR_MAX_EXAMPLES");
    if (max_n < 0 || max_n > IGS_FPS_MAX_EXAMPLE_POINTS)
        throw RasterizerError("anchors_fps: an example of " + std::to_string(max_n) + " points is more than the supported " + std::to_string(IGS_FPS_MAX_EXAMPLE_POINTS));
    if (total < 0 || total > IGS_ANCHOR_MAX_POINTS) throw RasterizerError("anchors_fps: total out of range");
    if (!(init_d2 >= 0.0)) throw RasterizerError("anchors_fps: init_d2 must be >= 0");
    require_gpu(xyz, "anchors_fps", "xyz");
    const c10::Device dev = xyz.device();
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    const Tensor p = offsets_i32(ptr, "anchors_fps", "ptr", xyz, B + 1), st = offsets_i32(start, "anchors_fps", "start", xyz, B);
    const Tensor op = offsets_i32(out_ptr, "anchors_fps", "out_ptr", xyz, B + 1), x = xyz.contiguous();
    Tensor out = at::empty({total}, xyz.options().dtype(at::kLong));
    if (total == 0) return out;
    const int N = (int)xyz.size(0);
    Tensor scratch = at::empty({(int64_t)igs_fps_scratch_bytes((int)B, N, (int)max_n)}, xyz.options().dtype(at::kByte));
    check(igs_fps(cur_stream(dev), (int)B, N, (int)max_n, x.data_ptr<float>(), p.data_ptr<int>(), st.data_ptr<int>(), op.data_ptr<int>(),
                  (int)total, (float)init_d2, scratch.data_ptr(), out.data_ptr<int64_t>()), "igs_fps");
    return out;
}

// torch_cluster knn as fixed shapes: (index into x [Ny, k] int64 with -1 padding, d2 [Ny, k] or None, weights [Ny, k] or None)
std::tuple<Tensor, c10::optional<Tensor>, c10::optional<Tensor>> anchors_knn(const Tensor& x, const Tensor& y, const Tensor& ptr_x,
                                                                              const Tensor& ptr_y, int64_t k, bool with_d2,
                                                                              c10::optional<double> weight_scale)
{
    check_points(x, "anchors_knn", "x");
    check_points(y, "anchors_knn", "y");
    if (x.device() != y.device()) throw RasterizerError("anchors_knn: x and y must be on one device");
    if (k < 1 || k > IGS_KNN_QUERY_MAX_K) throw RasterizerError("anchors_knn: k must be in [1, " + std::to_string(IGS_KNN_QUERY_MAX_K) + "] (got " + std::to_string(k) + ")");
    const int64_t B = ptr_x.dim() == 1 ? ptr_x.size(0) - 1 : -1;
    if (B < 1 || B > IGS_ANCHOR_MAX_EXAMPLES) throw RasterizerError("anchors_knn: ptr_x must have shape [B + 1], 1 <= B <= IGS_ANCHOR_MAX_EXAMPLES");
    require_gpu(x, "anchors_knn", "x");
    const c10::Device dev = x.device();
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    const Tensor px = offsets_i32(ptr_x, "anchors_knn", "ptr_x", x, B + 1), py = offsets_i32(ptr_y, "anchors_knn", "ptr_y", x, B + 1);
    const Tensor xc = x.contiguous(), yc = y.contiguous();
    const int64_t Ny = y.size(0);
    Tensor idx = at::empty({Ny, k}, x.options().dtype(at::kLong));
    c10::optional<Tensor> d2, w;
    if (with_d2) d2 = at::empty({Ny, k}, x.options());
    if (weight_scale) w = at::empty({Ny, k}, x.options());
    if (Ny == 0) return {idx, d2, w};
    check(igs_knn_query(cur_stream(dev), (int)B, (int)x.size(0), (int)Ny, xc.data_ptr<float>(), yc.data_ptr<float>(), px.data_ptr<int>(),
                        py.data_ptr<int>(), (int)k, weight_scale ? (float)*weight_scale : 0.f, idx.data_ptr<int64_t>(),
                        d2 ? d2->data_ptr<float>() : nullptr, w ? w->data_ptr<float>() : nullptr), "igs_knn_query");
    return {idx, d2, w};
}

// ---- anchor feature interpolation and the Gaussian deform (motion.hip; contracts in include/igs_rast.h) ----
struct NotImplemented : public std::runtime_error { using std::runtime_error::runtime_error; };

static int motion_dtype(const Tensor& t, const char* fn, const char* name)
{
    if (t.scalar_type() == at::kFloat) return IGS_DTYPE_F32;
    if (t.scalar_type() == at::kHalf) return IGS_DTYPE_F16;
    throw NotImplemented(std::string(fn) + ": " + name + " must be float32 or float16 (got " + c10::toString(t.scalar_type()) + ")");
}
static void motion_expect(const Tensor& t, const char* fn, const char* name, at::ScalarType dt, std::initializer_list<int64_t> shape)
{
    if (t.scalar_type() != dt)
        throw NotImplemented(std::string(fn) + ": " + name + " must be " + c10::toString(dt) + " (got " + c10::toString(t.scalar_type()) + ")");
    bool ok = t.dim() == (int64_t)shape.size();
    int i = 0;
    for (int64_t n : shape) { if (ok && n >= 0 && t.size(i) != n) ok = false; i++; }
    if (!ok) throw RasterizerError(std::string(fn) + ": " + name + " has shape " + c10::str(t.sizes()) + ", expected " + c10::str(at::IntArrayRef(shape)) + " (-1: any)");
}
static void same_device(const Tensor& t, const Tensor& like, const char* fn, const char* name)
{
    if (t.device() != like.device()) throw RasterizerError(std::string(fn) + ": " + name + " must be on " + c10::str(like.device()));
}

// out [N, D] float32 = sum_k w[n, k] * F[col[n, k]]: F [A_total, D] float32 / float16, col [N, K] int64, w [N, K] float32
Tensor motion_interp_fwd(const Tensor& F, const Tensor& col, const Tensor& w)
{
    const char* fn = "motion_interp_fwd";
    const int dt = motion_dtype(F, fn, "features");
    if (F.dim() != 2) throw RasterizerError(std::string(fn) + ": features must have shape [A_total, D] (got " + c10::str(F.sizes()) + ")");
    motion_expect(col, fn, "col", at::kLong, {-1, -1});
    motion_expect(w, fn, "weights", at::kFloat, {col.size(0), col.size(1)});
    const int64_t N = col.size(0), K = col.size(1), A = F.size(0), D = F.size(1);
    if (K < 1 || K > IGS_INTERP_MAX_K || D < 1 || D > IGS_INTERP_MAX_D || A < 1 || A > IGS_INTERP_MAX_ANCHORS || N > IGS_INTERP_MAX_ROWS ||
        N * K > IGS_INTERP_MAX_EDGES)
        throw RasterizerError(std::string(fn) + ": sizes out of range (1 <= K <= 100, 1 <= D <= 1024, 1 <= A_total <= 2^24, N <= 2^24, N * K <= 2^30)");
    require_gpu(F, fn, "features");
    same_device(col, F, fn, "col");
    same_device(w, F, fn, "weights");
    const c10::Device dev = F.device();
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    Tensor out = at::empty({N, D}, F.options().dtype(at::kFloat));
    if (N == 0) return out;
    const Tensor Fc = F.contiguous(), cc = col.contiguous(), wc = w.contiguous();
    check(igs_anchor_interp_fwd(cur_stream(dev), (int)N, (int)K, (int)D, (int)A, dt, Fc.data_ptr(), cc.data_ptr<int64_t>(), wc.data_ptr<float>(),
                                out.data_ptr<float>()), "igs_anchor_interp_fwd");
    return out;
}

// the inverse index of col (and room for the backward's partials at width D): a uint8 tensor to hand to motion_interp_bwd
Tensor motion_interp_index(const Tensor& col, int64_t A, int64_t D)
{
    const char* fn = "motion_interp_index";
    motion_expect(col, fn, "col", at::kLong, {-1, -1});
    const int64_t N = col.size(0), K = col.size(1);
    const size_t bytes = (N <= INT_MAX && K <= INT_MAX && A <= INT_MAX && D <= INT_MAX) ? igs_anchor_interp_index_bytes((int)N, (int)K, (int)A, (int)D) : 0;
    if (bytes == 0) throw RasterizerError(std::string(fn) + ": sizes out of range");
    require_gpu(col, fn, "col");
    const c10::Device dev = col.device();
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    Tensor scratch = at::empty({(int64_t)bytes}, col.options().dtype(at::kByte));
    const Tensor cc = col.contiguous();
    check(igs_anchor_interp_index(cur_stream(dev), (int)N, (int)K, (int)A, (int)D, cc.data_ptr<int64_t>(), scratch.data_ptr()), "igs_anchor_interp_index");
    return scratch;
}

// (dF [A_total, D] in F's dtype or None, dw [N, K] float32 or None) from the index of motion_interp_index
std::tuple<OptTensor, OptTensor> motion_interp_bwd(const Tensor& F, const Tensor& w, const Tensor& dout, const Tensor& index, bool want_dF,
                                                   bool want_dw)
{
    const char* fn = "motion_interp_bwd";
    const int dt = motion_dtype(F, fn, "features");
    if (F.dim() != 2) throw RasterizerError(std::string(fn) + ": features must have shape [A_total, D] (got " + c10::str(F.sizes()) + ")");
    motion_expect(w, fn, "weights", at::kFloat, {-1, -1});
    const int64_t N = w.size(0), K = w.size(1), A = F.size(0), D = F.size(1);
    motion_expect(dout, fn, "grad_out", at::kFloat, {N, D});
    motion_expect(index, fn, "index", at::kByte, {-1});
    require_gpu(F, fn, "features");
    same_device(w, F, fn, "weights");
    same_device(dout, F, fn, "grad_out");
    same_device(index, F, fn, "index");
    const size_t need = igs_anchor_interp_index_bytes((int)N, (int)K, (int)A, (int)D);
    if (need == 0 || (size_t)index.numel() < need) throw RasterizerError(std::string(fn) + ": index too small for these sizes (or sizes out of range)");
    const c10::Device dev = F.device();
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    OptTensor dF, dw;
    if (want_dF) dF = at::empty({A, D}, F.options());
    if (want_dw) dw = at::empty({N, K}, w.options());
    const Tensor Fc = F.contiguous(), wc = w.contiguous(), gc = dout.contiguous();
    check(igs_anchor_interp_bwd(cur_stream(dev), (int)N, (int)K, (int)D, (int)A, dt, Fc.data_ptr(), wc.data_ptr<float>(), gc.data_ptr<float>(),
                                index.data_ptr(), dF ? dF->data_ptr() : nullptr, dw ? dw->data_ptr<float>() : nullptr), "igs_anchor_interp_bwd");
    return {dF, dw};
}

// ---- multi-view anchor feature lifting (lift.hip) ----
struct LiftSizes { int64_t B, V, A, C, H, W; };
static LiftSizes lift_check(const char* fn, const Tensor& points, const Tensor& w2c, const Tensor& intr, int64_t C, int64_t H, int64_t W, int dt)
{
    motion_expect(points, fn, "anchor_points", at::kFloat, {-1, -1, 3});
    motion_expect(w2c, fn, "w2c", at::kFloat, {-1, 4, 4});
    motion_expect(intr, fn, "intrinsics", at::kFloat, {w2c.size(0), 4});
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
    const int dt = motion_dtype(feat, fn, "motion_feature");
    if (feat.dim() != 4) throw RasterizerError(std::string(fn) + ": motion_feature must have shape [B*V, C, H, W] (got " + c10::str(feat.sizes()) + ")");
    if (feat.size(0) != w2c.size(0))
        throw RasterizerError(std::string(fn) + ": motion_feature has shape " + c10::str(feat.sizes()) + " for " + std::to_string(w2c.size(0)) + " views");
    const LiftSizes z = lift_check(fn, points, w2c, intr, feat.size(1), feat.size(2), feat.size(3), dt);
    require_gpu(feat, fn, "motion_feature");
    same_device(points, feat, fn, "anchor_points");
    same_device(w2c, feat, fn, "w2c");
    same_device(intr, feat, fn, "intrinsics");
    const c10::Device dev = feat.device();
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    Tensor out = at::empty({z.B, z.C, z.A}, feat.options().dtype(at::kFloat));
    if (z.A == 0) return out;
    Tensor scratch = at::empty({(int64_t)igs_anchor_lift_scratch_bytes((int)z.B, (int)z.V, (int)z.A, (int)z.C, (int)z.H, (int)z.W, dt)},
                               feat.options().dtype(at::kByte));
    const Tensor pc = points.contiguous(), wc = w2c.contiguous(), ic = intr.contiguous();
    check(igs_anchor_lift_fwd(cur_stream(dev), (int)z.B, (int)z.V, (int)z.A, (int)z.C, (int)z.H, (int)z.W, dt, feat.data_ptr(), feat.stride(0),
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
    motion_expect(grad_bca, fn, "grad_out", at::kFloat, {-1, -1, -1});
    const LiftSizes z = lift_check(fn, points, w2c, intr, grad_bca.size(1), H, W, dt);
    if (grad_bca.size(0) != z.B || grad_bca.size(2) != z.A)
        throw RasterizerError(std::string(fn) + ": grad_out has shape " + c10::str(grad_bca.sizes()) + ", expected [B, C, A]");
    require_gpu(grad_bca, fn, "grad_out");
    same_device(points, grad_bca, fn, "anchor_points");
    same_device(w2c, grad_bca, fn, "w2c");
    same_device(intr, grad_bca, fn, "intrinsics");
    const c10::Device dev = grad_bca.device();
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    Tensor dfeat = at::empty({z.B * z.V, z.C, z.H, z.W}, grad_bca.options().dtype(half ? at::kHalf : at::kFloat));
    const bool bac = grad_bca.stride(0) == z.A * z.C && grad_bca.stride(1) == 1 && grad_bca.stride(2) == z.C;      // [B, A, C]-contiguous
    const Tensor g = (bac || z.A == 0) ? grad_bca : grad_bca.contiguous();
    const size_t bytes = igs_anchor_lift_bwd_scratch_bytes((int)z.B, (int)z.V, (int)z.A, (int)z.C, (int)z.H, (int)z.W, dt);
    Tensor scratch = at::empty({z.A == 0 ? 0 : (int64_t)bytes}, grad_bca.options().dtype(at::kByte));
    const Tensor pc = points.contiguous(), wc = w2c.contiguous(), ic = intr.contiguous();
    check(igs_anchor_lift_bwd(cur_stream(dev), (int)z.B, (int)z.V, (int)z.A, (int)z.C, (int)z.H, (int)z.W, dt, pc.data_ptr<float>(),
                              wc.data_ptr<float>(), ic.data_ptr<float>(), g.data_ptr<float>(), bac ? z.C : 1, bac ? 1 : z.A, dfeat.data_ptr(),
                              z.C * z.H * z.W, z.H * z.W, z.W, 1, scratch.data_ptr()), "igs_anchor_lift_bwd");
    return dfeat;
}

// ---- ray conditioning and fused LayerNorm + modulation (cond.hip) ----
// cond [N, H, W, 33] float32 from rays [N, H, W, 6] and depth [N, Hd, Wd] (float32; N = B * V views)
Tensor cond_ray_fwd(const Tensor& rays, const Tensor& depth)
{
    const char* fn = "cond_ray_fwd";
    motion_expect(rays, fn, "rays", at::kFloat, {-1, -1, -1, 6});
    motion_expect(depth, fn, "depth", at::kFloat, {rays.size(0), -1, -1});
    const int64_t N = rays.size(0), H = rays.size(1), W = rays.size(2), Hd = depth.size(1), Wd = depth.size(2);
    if (H < 1 || W < 1 || Hd < 1 || Wd < 1 || H > IGS_COND_MAX_HW || W > IGS_COND_MAX_HW || Hd > IGS_COND_MAX_HW || Wd > IGS_COND_MAX_HW ||
        N * H * W > IGS_COND_MAX_PIXELS)
        throw RasterizerError(std::string(fn) + ": sizes out of range (1 <= H, W, Hd, Wd <= 8192, N * H * W <= 2^24)");
    require_gpu(rays, fn, "rays");
    same_device(depth, rays, fn, "depth");
    const c10::Device dev = rays.device();
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    Tensor cond = at::empty({N, H, W, 33}, rays.options());
    const Tensor rc = rays.contiguous(), dc = depth.contiguous();
    check(igs_ray_condition_fwd(cur_stream(dev), (int)N, (int)H, (int)W, (int)Hd, (int)Wd, rc.data_ptr<float>(), dc.data_ptr<float>(),
                                cond.data_ptr<float>()), "igs_ray_condition_fwd");
    return cond;
}

struct ModlnSizes { int64_t N, C, H, W; int xdt, mdt; };
static ModlnSizes modln_check(const char* fn, const Tensor& x, const Tensor& mod, const Tensor& weight, const Tensor& bias)
{
    ModlnSizes z;
    z.xdt = motion_dtype(x, fn, "x");
    z.mdt = motion_dtype(mod, fn, "mod");
    if (x.dim() != 4) throw RasterizerError(std::string(fn) + ": x must have shape [N, C, H, W] (got " + c10::str(x.sizes()) + ")");
    z.N = x.size(0); z.C = x.size(1); z.H = x.size(2); z.W = x.size(3);
    motion_expect(mod, fn, "mod", mod.scalar_type(), {z.N, z.H, z.W, 2 * z.C});
    motion_expect(weight, fn, "weight", at::kFloat, {z.C});
    motion_expect(bias, fn, "bias", at::kFloat, {z.C});
    if (z.C < 1 || z.C > IGS_MODLN_MAX_C || z.H < 1 || z.W < 1 || z.H > IGS_COND_MAX_HW || z.W > IGS_COND_MAX_HW ||
        z.N * z.H * z.W > IGS_COND_MAX_PIXELS)
        throw RasterizerError(std::string(fn) + ": sizes out of range (1 <= C <= 1024, 1 <= H, W <= 8192, N * H * W <= 2^24)");
    return z;
}
static void modln_devices(const char* fn, const Tensor& x, const Tensor& mod, const Tensor& weight, const Tensor& bias)      // after the shape checks
{
    require_gpu(x, fn, "x");
    same_device(mod, x, fn, "mod");
    same_device(weight, x, fn, "weight");
    same_device(bias, x, fn, "bias");
}

// (out [N, C, H, W] float32 contiguous, mean, rstd [N, H, W] float32 or None): x [N, C, H, W] float32 / float16 with contiguous H x W
// planes, mod [N, H, W, 2 C] float32 / float16, weight, bias [C] float32
std::tuple<Tensor, OptTensor, OptTensor> modln_fwd(const Tensor& x, const Tensor& mod, const Tensor& weight, const Tensor& bias, double eps,
                                                    bool save_stats)
{
    const char* fn = "modln_fwd";
    const ModlnSizes z = modln_check(fn, x, mod, weight, bias);
    modln_devices(fn, x, mod, weight, bias);
    const c10::Device dev = x.device();
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    const auto fo = x.options().dtype(at::kFloat);
    Tensor out = at::empty({z.N, z.C, z.H, z.W}, fo);
    OptTensor mean, rstd;
    if (save_stats) { mean = at::empty({z.N, z.H, z.W}, fo); rstd = at::empty({z.N, z.H, z.W}, fo); }
    if (z.N == 0) return {out, mean, rstd};
    const Tensor mc = mod.contiguous(), wc = weight.contiguous(), bc = bias.contiguous();
    check(igs_modln_fwd(cur_stream(dev), (int)z.N, (int)z.C, (int)z.H, (int)z.W, z.xdt, x.data_ptr(), x.stride(0), x.stride(1), x.stride(2),
                        x.stride(3), z.mdt, mc.data_ptr(), wc.data_ptr<float>(), bc.data_ptr<float>(), (float)eps, out.data_ptr<float>(),
                        mean ? mean->data_ptr<float>() : nullptr, rstd ? rstd->data_ptr<float>() : nullptr), "igs_modln_fwd");
    return {out, mean, rstd};
}

// (d x in x's dtype, d mod in mod's dtype, d weight, d bias), each None unless wanted
std::tuple<OptTensor, OptTensor, OptTensor, OptTensor> modln_bwd(const Tensor& x, const Tensor& mod, const Tensor& weight, const Tensor& bias,
                                                                  const Tensor& mean, const Tensor& rstd, const Tensor& grad_out, bool want_x,
                                                                  bool want_mod, bool want_weight, bool want_bias)
{
    const char* fn = "modln_bwd";
    const ModlnSizes z = modln_check(fn, x, mod, weight, bias);
    motion_expect(mean, fn, "mean", at::kFloat, {z.N, z.H, z.W});
    motion_expect(rstd, fn, "rstd", at::kFloat, {z.N, z.H, z.W});
    motion_expect(grad_out, fn, "grad_out", at::kFloat, {z.N, z.C, z.H, z.W});
    modln_devices(fn, x, mod, weight, bias);
    same_device(mean, x, fn, "mean");
    same_device(rstd, x, fn, "rstd");
    same_device(grad_out, x, fn, "grad_out");
    const c10::Device dev = x.device();
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    OptTensor dx, dmod, dw, db;
    const auto fo = x.options().dtype(at::kFloat);
    if (want_x) dx = at::empty({z.N, z.C, z.H, z.W}, x.options());
    if (want_mod) dmod = at::empty({z.N, z.H, z.W, 2 * z.C}, mod.options());
    if (want_weight) dw = z.N == 0 ? at::zeros({z.C}, fo) : at::empty({z.C}, fo);
    if (want_bias) db = z.N == 0 ? at::zeros({z.C}, fo) : at::empty({z.C}, fo);
    if (z.N == 0 || !(want_x || want_mod || want_weight || want_bias)) return {dx, dmod, dw, db};
    Tensor scratch;
    if (want_weight || want_bias)
        scratch = at::empty({(int64_t)igs_modln_bwd_scratch_bytes((int)z.N, (int)z.C, (int)z.H, (int)z.W)}, x.options().dtype(at::kByte));
    const Tensor mc = mod.contiguous(), wc = weight.contiguous(), bc = bias.contiguous(), mu = mean.contiguous(), rs = rstd.contiguous(),
                 gc = grad_out.contiguous();
    check(igs_modln_bwd(cur_stream(dev), (int)z.N, (int)z.C, (int)z.H, (int)z.W, z.xdt, x.data_ptr(), x.stride(0), x.stride(1), x.stride(2),
                        x.stride(3), z.mdt, mc.data_ptr(), wc.data_ptr<float>(), bc.data_ptr<float>(), mu.data_ptr<float>(), rs.data_ptr<float>(),
                        gc.data_ptr<float>(), dx ? dx->data_ptr() : nullptr, dmod ? dmod->data_ptr() : nullptr,
                        dw ? dw->data_ptr<float>() : nullptr, db ? db->data_ptr<float>() : nullptr,
                        scratch.defined() ? scratch.data_ptr() : nullptr), "igs_modln_bwd");
    return {dx, dmod, dw, db};
}

// ---- fused attention for the anchor transformer (attn.hip; contract in include/igs_rast.h) ----
struct AttnSizes { int64_t B, H, Aq, Ak; int dt; };
static void attn_view_check(const char* fn, const Tensor& t, const char* name, const Tensor& like, int64_t B, int64_t H, int64_t A)
{
    if (t.dim() != 4 || t.size(0) != B || t.size(1) != H || t.size(2) != A || t.size(3) != 64)
        throw RasterizerError(std::string(fn) + ": " + name + " has shape " + c10::str(t.sizes()) + ", expected " +
                              c10::str(at::IntArrayRef({B, H, A, (int64_t)64})));
    if (t.scalar_type() != like.scalar_type()) throw NotImplemented(std::string(fn) + ": " + name + " must have q's dtype");
    if (t.stride(3) != 1) throw RasterizerError(std::string(fn) + ": " + name + " must have stride 1 on its last dimension");
}
static AttnSizes attn_check(const char* fn, const Tensor& q, const Tensor& k, const Tensor& v)
{
    AttnSizes z;
    z.dt = motion_dtype(q, fn, "q");
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
static Tensor attn_empty(const Tensor& like, int64_t B, int64_t H, int64_t A, bool token_major)
{
    return token_major ? at::empty({B, A, H, 64}, like.options()).permute({0, 2, 1, 3}) : at::empty({B, H, A, 64}, like.options());
}

// (out, lse or None): q [B, H, Aq, 64], k, v [B, H, Ak, 64] float32 / float16 views with stride 1 on the last dimension
std::tuple<Tensor, OptTensor> attn_fwd(const Tensor& q, const Tensor& k, const Tensor& v, double scale, bool token_major, bool want_lse)
{
    const char* fn = "attn_fwd";
    const AttnSizes z = attn_check(fn, q, k, v);
    require_gpu(q, fn, "q");
    same_device(k, q, fn, "k");
    same_device(v, q, fn, "v");
    const c10::Device dev = q.device();
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    Tensor out = attn_empty(q, z.B, z.H, z.Aq, token_major);
    OptTensor lse;
    if (want_lse) lse = at::empty({z.B, z.H, z.Aq}, q.options().dtype(at::kFloat));
    if (z.B == 0) return {out, lse};
    check(igs_attn_fwd(cur_stream(dev), (int)z.B, (int)z.H, (int)z.Aq, (int)z.Ak, 64, z.dt, q.data_ptr(), q.stride(0), q.stride(1), q.stride(2),
                       k.data_ptr(), k.stride(0), k.stride(1), k.stride(2), v.data_ptr(), v.stride(0), v.stride(1), v.stride(2), (float)scale,
                       out.data_ptr(), out.stride(0), out.stride(1), out.stride(2), lse ? lse->data_ptr<float>() : nullptr), "igs_attn_fwd");
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
    motion_expect(lse, fn, "lse", at::kFloat, {z.B, z.H, z.Aq});
    require_gpu(q, fn, "q");
    same_device(k, q, fn, "k");
    same_device(v, q, fn, "v");
    same_device(out, q, fn, "out");
    same_device(lse, q, fn, "lse");
    same_device(grad_out, q, fn, "grad_out");
    const c10::Device dev = q.device();
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    OptTensor dq, dk, dv;
    if (want_q) dq = attn_empty(q, z.B, z.H, z.Aq, token_major);
    if (want_k) dk = attn_empty(q, z.B, z.H, z.Ak, token_major);
    if (want_v) dv = attn_empty(q, z.B, z.H, z.Ak, token_major);
    if (z.B == 0 || !(want_q || want_k || want_v)) return {dq, dk, dv};
    const Tensor ls = lse.contiguous();
    Tensor scratch = at::empty({(int64_t)igs_attn_bwd_scratch_bytes((int)z.B, (int)z.H, (int)z.Aq, (int)z.Ak, 64, z.dt)}, q.options().dtype(at::kByte));
    const Tensor none;
    const Tensor& tq = dq ? *dq : none; const Tensor& tk = dk ? *dk : none; const Tensor& tv = dv ? *dv : none;
#define ATTN_VIEW(t) (t).data_ptr(), (t).stride(0), (t).stride(1), (t).stride(2)
#define ATTN_OPT(t) (t).defined() ? (t).data_ptr() : nullptr, (t).defined() ? (t).stride(0) : 0, (t).defined() ? (t).stride(1) : 0, (t).defined() ? (t).stride(2) : 0
    check(igs_attn_bwd(cur_stream(dev), (int)z.B, (int)z.H, (int)z.Aq, (int)z.Ak, 64, z.dt, ATTN_VIEW(q), ATTN_VIEW(k), ATTN_VIEW(v), ATTN_VIEW(out),
                       ls.data_ptr<float>(), ATTN_VIEW(grad_out), (float)scale, ATTN_OPT(tq), ATTN_OPT(tk), ATTN_OPT(tv), scratch.data_ptr()),
          "igs_attn_bwd");
#undef ATTN_VIEW
#undef ATTN_OPT
    return {dq, dk, dv};
}

static void deform_checks(const char* fn, const Tensor& rot, const Tensor& mask, const Tensor& dxyz, const Tensor& drot, int* dt)
{
    motion_expect(rot, fn, "rotation", at::kFloat, {-1, 4});
    motion_expect(mask, fn, "mask", at::kLong, {-1});
    *dt = motion_dtype(drot, fn, "res_rotation");
    if (dxyz.scalar_type() != drot.scalar_type()) throw NotImplemented(std::string(fn) + ": res_xyz and res_rotation must share a dtype");
    motion_expect(dxyz, fn, "res_xyz", dxyz.scalar_type(), {mask.size(0), 3});
    motion_expect(drot, fn, "res_rotation", drot.scalar_type(), {mask.size(0), 4});
    if (rot.size(0) > IGS_DEFORM_MAX_POINTS || mask.size(0) > rot.size(0))
        throw RasterizerError(std::string(fn) + ": sizes out of range (M <= P <= 2^26)");
}

// (xyz_out, rotation_out): xyz[mask] += res_xyz, rotation[mask] = qmul(nrm(rotation[mask]), nrm(res_rotation))
std::tuple<Tensor, Tensor> motion_deform_fwd(const Tensor& xyz, const Tensor& rot, const Tensor& mask, const Tensor& dxyz, const Tensor& drot)
{
    const char* fn = "motion_deform_fwd";
    int dt;
    motion_expect(xyz, fn, "xyz", at::kFloat, {-1, 3});
    deform_checks(fn, rot, mask, dxyz, drot, &dt);
    if (rot.size(0) != xyz.size(0)) throw RasterizerError(std::string(fn) + ": xyz and rotation must have the same number of rows");
    require_gpu(xyz, fn, "xyz");
    for (const Tensor* t : { &rot, &mask, &dxyz, &drot }) same_device(*t, xyz, fn, "every input");
    const c10::Device dev = xyz.device();
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    const int64_t P = xyz.size(0), M = mask.size(0);
    Tensor xo = at::empty({P, 3}, xyz.options()), ro = at::empty({P, 4}, xyz.options());
    if (P == 0) return {xo, ro};
    const Tensor xc = xyz.contiguous(), rc = rot.contiguous(), mc = mask.contiguous(), dxc = dxyz.contiguous(), drc = drot.contiguous();
    check(igs_gaussian_deform_fwd(cur_stream(dev), (int)P, (int)M, dt, xc.data_ptr<float>(), rc.data_ptr<float>(), mc.data_ptr<int64_t>(),
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
    if (g_xyz) motion_expect(*g_xyz, fn, "grad_xyz", at::kFloat, {P, 3});
    if (g_rot) motion_expect(*g_rot, fn, "grad_rotation", at::kFloat, {P, 4});
    require_gpu(rot, fn, "rotation");
    for (const Tensor* t : { &mask, &dxyz, &drot }) same_device(*t, rot, fn, "every input");
    if (g_xyz) same_device(*g_xyz, rot, fn, "grad_xyz");
    if (g_rot) same_device(*g_rot, rot, fn, "grad_rotation");
    const c10::Device dev = rot.device();
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    OptTensor dx, dr, ddx, ddr;
    if (want_xyz) dx = at::empty({P, 3}, rot.options());
    if (want_rot) dr = at::empty({P, 4}, rot.options());
    if (want_dxyz) ddx = at::empty({M, 3}, drot.options());
    if (want_drot) ddr = at::empty({M, 4}, drot.options());
    if (P == 0) return {dx, dr, ddx, ddr};
    const Tensor rc = rot.contiguous(), mc = mask.contiguous(), drc = drot.contiguous();
    Tensor gx, gr;
    if (g_xyz) gx = g_xyz->contiguous();
    if (g_rot) gr = g_rot->contiguous();
    check(igs_gaussian_deform_bwd(cur_stream(dev), (int)P, (int)M, dt, rc.data_ptr<float>(), mc.data_ptr<int64_t>(), drc.data_ptr(),
                                  g_xyz ? gx.data_ptr<float>() : nullptr, g_rot ? gr.data_ptr<float>() : nullptr, dx ? dx->data_ptr<float>() : nullptr,
                                  dr ? dr->data_ptr<float>() : nullptr, ddx ? ddx->data_ptr() : nullptr, ddr ? ddr->data_ptr() : nullptr),
          "igs_gaussian_deform_bwd");
    return {dx, dr, ddx, ddr};
}

// igs_adam_step_multi over lists of tensors (igs_amd/optim.py): one launch for up to 8 parameters
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
    const c10::Device dev = params[0].device();
    for (size_t k = 0; k < n; k++) {
        const Tensor& P_ = params[k];
        if (!P_.is_cuda() || P_.device() != dev || P_.scalar_type() != at::kFloat || !P_.is_contiguous() || !exp_avgs[k].is_contiguous()
            || !exp_avg_sqs[k].is_contiguous() || grads[k].numel() != P_.numel() || exp_avgs[k].numel() != P_.numel() || exp_avg_sqs[k].numel() != P_.numel())
            throw RasterizerError("adam_step_multi: parameters and state must be contiguous float32 tensors on one GPU (no CPU fallback)");
        Tensor G = (grads[k].is_contiguous() && grads[k].scalar_type() == at::kFloat) ? grads[k] : grads[k].to(at::kFloat).contiguous();
        keep.push_back(G);
        p[k] = P_.data_ptr<float>(); g[k] = G.data_ptr<float>(); m[k] = exp_avgs[k].data_ptr<float>(); v[k] = exp_avg_sqs[k].data_ptr<float>();
        cnt[k] = (size_t)P_.numel(); lr[k] = (float)lrs[k];
        if (dev_step) {
            const Tensor& S_ = steps[k];
            if (!S_.is_cuda() || S_.device() != dev || S_.scalar_type() != at::kFloat || S_.numel() != 1)
                throw RasterizerError("adam_step_multi: every step count must be a one-element float32 tensor on the parameters' GPU");
            st[k] = S_.data_ptr<float>();
        } else {
            b1c[k] = (float)bc1[k]; b2c[k] = (float)bc2_sqrt[k];
        }
    }
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    hipStream_t stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(dev.index()).stream();
    unsigned* done = nullptr;
    if (dev_step) {
        if (!done_scratch.has_value() || !done_scratch->is_cuda() || done_scratch->device() != dev || done_scratch->scalar_type() != at::kInt
            || (size_t)done_scratch->numel() < igs_adam_step_multi_dev_scratch_words() || !done_scratch->is_contiguous())
            throw RasterizerError("adam_step_multi: device-side step counts need `done_scratch`, an int32 tensor of adam_dev_scratch_words() zeros on the parameters' GPU");
        done = (unsigned*)done_scratch->data_ptr<int>();
    }
    const int rc = dev_step ? igs_adam_step_multi_dev(stream, (int)n, p, g, m, v, cnt, lr, st, done, (float)beta1, (float)beta2, (float)eps)
                            : igs_adam_step_multi(stream, (int)n, p, g, m, v, cnt, lr, b1c, b2c, (float)beta1, (float)beta2, (float)eps);
    if (rc != 0) throw RasterizerError("igs_adam_step_multi failed: " + std::to_string(rc));
}

// ---- the two image losses of the refine loop as single calls (igs_amd/losses.py wraps them in autograd Functions) ----
// small per-(device, stream) scratch kept for the life of the process
struct LossScratch { Tensor l1; Tensor ssim; int64_t ssim_w = 0, ssim_h = 0; };
bool stream_is_capturing(hipStream_t stream)
{
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(stream, &st) == hipSuccess && st != hipStreamCaptureStatusNone;
}
LossScratch& loss_scratch(const c10::Device& dev, hipStream_t stream)
{
    static std::mutex mu;
    static std::map<std::pair<int, void*>, LossScratch> table;
    std::lock_guard<std::mutex> lock(mu);
    return table[{ (int)dev.index(), (void*)stream }];
}

// mean |a - b| and sign(a - b) / n in one launch (igs_l1_mean_fwd_bwd; loss_utils.py:17-18)
std::tuple<Tensor, Tensor> l1_mean(const Tensor& a, const Tensor& b)
{
    if (!a.is_cuda() || !b.is_cuda() || a.numel() == 0 || a.numel() != b.numel()) throw RasterizerError("l1_mean: two GPU tensors of the same, non-zero size (no CPU fallback)");
    const c10::Device dev = a.device();
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    In x(a, dev, "a"), y(b, dev, "b");
    hipStream_t stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(dev.index()).stream();
    auto fopt = at::TensorOptions().dtype(at::kFloat).device(dev);
    // 1024 partial sums | the self-resetting counter words: kept per (device, stream) -- except on a capturing stream, where the scratch
    // must be memory the graph owns (allocated here, from the capture's private pool, zeroed by a node of the graph)
    Tensor l1s;
    if (stream_is_capturing(stream)) l1s = at::zeros({1024 + 33 * 64}, fopt);
    else {
        LossScratch& sc = loss_scratch(dev, stream);
        if (!sc.l1.defined()) sc.l1 = at::zeros({1024 + 33 * 64}, fopt);
        l1s = sc.l1;
    }
    Tensor grad = at::empty_like(x.keep), out = at::empty({}, fopt);
    const int rc = igs_l1_mean_fwd_bwd(stream, (size_t)x.keep.numel(), x.p, y.p, grad.data_ptr<float>(), out.data_ptr<float>(),
                                       l1s.data_ptr<float>(), (unsigned*)(l1s.data_ptr<float>() + 1024));
    if (rc != 0) throw RasterizerError("igs_l1_mean_fwd_bwd failed: " + std::to_string(rc));
    return { out, grad };
}

// mean SSIM(a, b) over all elements (finished on the device) and d(mean SSIM)/da in two launches (igs_ssim_mean_fwd_bwd; loss_utils.py:34-63 with the 11x11 window).  a, b: [3, H, W] (or anything that reshapes to it)
std::tuple<Tensor, Tensor> ssim_mean(const Tensor& a, const Tensor& b)
{
    if (!a.is_cuda() || !b.is_cuda() || a.dim() < 3 || a.numel() != b.numel()) throw RasterizerError("ssim_mean: two GPU images of the same size (no CPU fallback)");
    const c10::Device dev = a.device();
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    In x(a, dev, "a"), y(b, dev, "b");
    const int64_t H = a.size(-2), W = a.size(-1);
    if (a.numel() != 3 * H * W) throw RasterizerError("ssim_mean: one 3-channel image per side");
    hipStream_t stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(dev.index()).stream();
    Tensor scratch;
    const auto bopt = at::TensorOptions().dtype(at::kByte).device(dev);
    if (stream_is_capturing(stream)) scratch = at::empty({(int64_t)igs_ssim_l1_scratch_bytes((int)W, (int)H)}, bopt);      // (graph-owned, as in l1_mean)
    else {
        LossScratch& sc = loss_scratch(dev, stream);
        if (!sc.ssim.defined() || sc.ssim_w != W || sc.ssim_h != H) {
            sc.ssim = at::empty({(int64_t)igs_ssim_l1_scratch_bytes((int)W, (int)H)}, bopt);
            sc.ssim_w = W; sc.ssim_h = H;
        }
        scratch = sc.ssim;
    }
    auto fopt = at::TensorOptions().dtype(at::kFloat).device(dev);
    Tensor grad = at::empty_like(x.keep), mean = at::empty({}, fopt);
    const int rc = igs_ssim_mean_fwd_bwd(stream, (int)W, (int)H, x.p, y.p, scratch.data_ptr(), grad.data_ptr<float>(), mean.data_ptr<float>());
    if (rc != 0) throw RasterizerError("igs_ssim_mean_fwd_bwd failed: " + std::to_string(rc));
    return { mean, grad };               // grad = d(mean SSIM)/da
}

}      // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m)
{
    namespace py = pybind11;
    py::register_exception<RasterizerError>(m, "RasterizerError", PyExc_RuntimeError);
    py::register_exception<NotImplemented>(m, "NotImplementedDtype", PyExc_NotImplementedError);
    py::class_<ScratchSet, std::shared_ptr<ScratchSet>>(m, "ScratchSet")
        .def(py::init([](const py::object& device, bool persistent) {
                 return std::make_shared<ScratchSet>(torch::python::detail::py_object_to_device(device), persistent);
             }), py::arg("device"), py::arg("persistent") = true)
        .def_readonly("geom", &ScratchSet::geom).def_readonly("binning", &ScratchSet::binning).def_readonly("img", &ScratchSet::img)
        .def_readonly("persistent", &ScratchSet::persistent)
        .def("workspace", [](ScratchSet& s, int64_t P) { return s.ensure_workspace(P); }, py::arg("P"))
        // (callback address, user word) x 3 for callers that fill a C struct themselves (igs_refine_step_args through ctypes);
        // valid for as long as this object lives
        .def("callbacks", [](ScratchSet& s) {
            return std::make_tuple((uintptr_t)&grow_cb, (uintptr_t)&s.g_geom, (uintptr_t)&s.g_binning, (uintptr_t)&s.g_img);
        });

    const auto none = py::none();
    m.def("rasterize_gaussians", &rasterize_gaussians, py::arg("background"), py::arg("means3D"), py::arg("colors"), py::arg("opacity"),
          py::arg("scales"), py::arg("rotations"), py::arg("scale_modifier"), py::arg("cov3D_precomp"), py::arg("viewmatrix"),
          py::arg("projmatrix"), py::arg("tan_fovx"), py::arg("tan_fovy"), py::arg("kernel_size"), py::arg("image_height"),
          py::arg("image_width"), py::arg("sh"), py::arg("degree"), py::arg("campos"), py::arg("prefiltered"), py::arg("require_coord"),
          py::arg("require_depth"), py::arg("debug"), py::kw_only(), py::arg("scratch") = std::shared_ptr<ScratchSet>(),
          py::arg("out_images") = none, py::arg("out_radii") = none, py::arg("mode") = 0, py::arg("scratch_clean") = false,
          py::call_guard<py::gil_scoped_release>());

#define BWD_ARGS \
    py::arg("background"), py::arg("means3D"), py::arg("radii"), py::arg("colors"), py::arg("scales"), py::arg("rotations"), \
    py::arg("scale_modifier"), py::arg("cov3D_precomp"), py::arg("viewmatrix"), py::arg("projmatrix"), py::arg("tan_fovx"), py::arg("tan_fovy"), \
    py::arg("kernel_size"), py::arg("dL_dout_color"), py::arg("dL_dout_coord"), py::arg("dL_dout_mcoord"), py::arg("dL_dout_depth"), \
    py::arg("dL_dout_mdepth"), py::arg("dL_dout_alpha"), py::arg("dL_dout_normal"), py::arg("normalmap"), py::arg("sh"), py::arg("degree"), \
    py::arg("campos"), py::arg("geomBuffer"), py::arg("R"), py::arg("binningBuffer"), py::arg("imageBuffer"), py::arg("alphas"), \
    py::arg("require_coord"), py::arg("require_depth"), py::arg("debug"), py::kw_only(), py::arg("workspace") = none, \
    py::arg("out_means2D") = none, py::arg("out_colors") = none, py::arg("out_opacity") = none, py::arg("out_means3D") = none, \
    py::arg("out_cov3D") = none, py::arg("out_sh") = none, py::arg("out_scales") = none, py::arg("out_rotations") = none

    m.def("rasterize_gaussians_backward",
          [](const Tensor& a0, const Tensor& a1, const Tensor& a2, const Tensor& a3, const Tensor& a4, const Tensor& a5, double a6, const Tensor& a7,
             const Tensor& a8, const Tensor& a9, double a10, double a11, double a12, const OptTensor& a13, const OptTensor& a14, const OptTensor& a15,
             const OptTensor& a16, const OptTensor& a17, const OptTensor& a18, const OptTensor& a19, const Tensor& a20, const Tensor& a21, int64_t a22,
             const Tensor& a23, const Tensor& a24, int64_t a25, const Tensor& a26, const Tensor& a27, const Tensor& a28, bool a29, bool a30, bool a31,
             const OptTensor& ws, const OptTensor& o0, const OptTensor& o1, const OptTensor& o2, const OptTensor& o3, const OptTensor& o4,
             const OptTensor& o5, const OptTensor& o6, const OptTensor& o7) {
              return backward_body(a0, a1, a2, a3, a4, a5, a6, a7, a8, a9, a10, a11, a12, a13, a14, a15, a16, a17, a18, a19, a20, a21, a22, a23,
                                   a24, a25, a26, a27, a28, a29, a30, a31, ws, o0, o1, o2, o3, o4, o5, o6, o7, 0, 0.0).grads;
          }, BWD_ARGS, py::call_guard<py::gil_scoped_release>());
    m.def("rasterize_gaussians_backward_ex",
          [](const Tensor& a0, const Tensor& a1, const Tensor& a2, const Tensor& a3, const Tensor& a4, const Tensor& a5, double a6, const Tensor& a7,
             const Tensor& a8, const Tensor& a9, double a10, double a11, double a12, const OptTensor& a13, const OptTensor& a14, const OptTensor& a15,
             const OptTensor& a16, const OptTensor& a17, const OptTensor& a18, const OptTensor& a19, const Tensor& a20, const Tensor& a21, int64_t a22,
             const Tensor& a23, const Tensor& a24, int64_t a25, const Tensor& a26, const Tensor& a27, const Tensor& a28, bool a29, bool a30, bool a31,
             const OptTensor& ws, const OptTensor& o0, const OptTensor& o1, const OptTensor& o2, const OptTensor& o3, const OptTensor& o4,
             const OptTensor& o5, const OptTensor& o6, const OptTensor& o7, int64_t nan_report, double clamp) {
              // nan_report: 0 none; 1 wait for the kernel's verdict here -> (grads, 0 / 1, 0, 0); 2 deferred -> (grads, 0, word, seq) for nan_report_wait
              BwdResult r = backward_body(a0, a1, a2, a3, a4, a5, a6, a7, a8, a9, a10, a11, a12, a13, a14, a15, a16, a17, a18, a19, a20, a21, a22, a23,
                                          a24, a25, a26, a27, a28, a29, a30, a31, ws, o0, o1, o2, o3, o4, o5, o6, o7, nan_report, clamp);
              return std::make_tuple(r.grads, r.nan, r.nan_word, r.nan_seq);
          }, BWD_ARGS, py::arg("nan_report") = 0, py::arg("clamp") = 0.0, py::call_guard<py::gil_scoped_release>());
    m.def("nan_report_wait", [](int64_t word, int64_t seq) {
        const int v = igs_rast_nan_report_wait_at((const void*)(uintptr_t)word, (unsigned)seq);
        check(v, "igs_rast_nan_report_wait_at");
        return v != 0;
    }, py::arg("word"), py::arg("seq"), py::call_guard<py::gil_scoped_release>());
    m.def("count_gaussians", &count_gaussians, py::arg("background"), py::arg("means3D"), py::arg("colors"), py::arg("opacity"),
          py::arg("scales"), py::arg("rotations"), py::arg("scale_modifier"), py::arg("cov3D_precomp"), py::arg("viewmatrix"),
          py::arg("projmatrix"), py::arg("tan_fovx"), py::arg("tan_fovy"), py::arg("image_height"), py::arg("image_width"), py::arg("sh"),
          py::arg("degree"), py::arg("campos"), py::arg("prefiltered"), py::arg("debug"), py::arg("f_count"), py::kw_only(),
          py::arg("scratch") = std::shared_ptr<ScratchSet>(), py::call_guard<py::gil_scoped_release>());
    m.def("mark_visible", &mark_visible, py::arg("means3D"), py::arg("viewmatrix"), py::arg("projmatrix"), py::call_guard<py::gil_scoped_release>());
    m.def("distCUDA2", &distCUDA2, py::arg("points"), py::call_guard<py::gil_scoped_release>());
    m.def("anchors_bbox_select", &anchors_bbox_select, py::arg("xyz"), py::arg("ptr"), py::arg("box"), py::call_guard<py::gil_scoped_release>());
    m.def("anchors_fps", &anchors_fps, py::arg("xyz"), py::arg("ptr"), py::arg("start"), py::arg("out_ptr"), py::arg("total"), py::arg("max_n"),
          py::arg("init_d2"), py::call_guard<py::gil_scoped_release>());
    m.def("anchors_knn", &anchors_knn, py::arg("x"), py::arg("y"), py::arg("ptr_x"), py::arg("ptr_y"), py::arg("k"), py::arg("with_d2") = false,
          py::arg("weight_scale") = py::none(), py::call_guard<py::gil_scoped_release>());
    m.def("motion_interp_fwd", &motion_interp_fwd, py::arg("features"), py::arg("col"), py::arg("weights"), py::call_guard<py::gil_scoped_release>());
    m.def("motion_interp_index", &motion_interp_index, py::arg("col"), py::arg("A"), py::arg("D"), py::call_guard<py::gil_scoped_release>());
    m.def("motion_interp_bwd", &motion_interp_bwd, py::arg("features"), py::arg("weights"), py::arg("grad_out"), py::arg("index"),
          py::arg("want_features") = true, py::arg("want_weights") = true, py::call_guard<py::gil_scoped_release>());
    m.def("motion_lift_fwd", &motion_lift_fwd, py::arg("motion_feature"), py::arg("anchor_points"), py::arg("w2c"), py::arg("intrinsics"),
          py::call_guard<py::gil_scoped_release>());
    m.def("motion_lift_bwd", &motion_lift_bwd, py::arg("grad_out"), py::arg("anchor_points"), py::arg("w2c"), py::arg("intrinsics"), py::arg("H"),
          py::arg("W"), py::arg("half") = false, py::call_guard<py::gil_scoped_release>());
    m.def("cond_ray_fwd", &cond_ray_fwd, py::arg("rays"), py::arg("depth"), py::call_guard<py::gil_scoped_release>());
    m.def("modln_fwd", &modln_fwd, py::arg("x"), py::arg("mod"), py::arg("weight"), py::arg("bias"), py::arg("eps") = 1e-6,
          py::arg("save_stats") = false, py::call_guard<py::gil_scoped_release>());
    m.def("modln_bwd", &modln_bwd, py::arg("x"), py::arg("mod"), py::arg("weight"), py::arg("bias"), py::arg("mean"), py::arg("rstd"),
          py::arg("grad_out"), py::arg("want_x") = true, py::arg("want_mod") = true, py::arg("want_weight") = true, py::arg("want_bias") = true,
          py::call_guard<py::gil_scoped_release>());
    m.def("attn_fwd", &attn_fwd, py::arg("q"), py::arg("k"), py::arg("v"), py::arg("scale"), py::arg("token_major") = false,
          py::arg("want_lse") = false, py::call_guard<py::gil_scoped_release>());
    m.def("attn_bwd", &attn_bwd, py::arg("q"), py::arg("k"), py::arg("v"), py::arg("out"), py::arg("lse"), py::arg("grad_out"), py::arg("scale"),
          py::arg("token_major") = false, py::arg("want_q") = true, py::arg("want_k") = true, py::arg("want_v") = true,
          py::call_guard<py::gil_scoped_release>());
    m.def("motion_deform_fwd", &motion_deform_fwd, py::arg("xyz"), py::arg("rotation"), py::arg("mask"), py::arg("res_xyz"),
          py::arg("res_rotation"), py::call_guard<py::gil_scoped_release>());
    m.def("motion_deform_bwd", &motion_deform_bwd, py::arg("rotation"), py::arg("mask"), py::arg("res_xyz"), py::arg("res_rotation"),
          py::arg("grad_xyz"), py::arg("grad_rotation"), py::arg("want_xyz") = true, py::arg("want_rotation") = true,
          py::arg("want_res_xyz") = true, py::arg("want_res_rotation") = true, py::call_guard<py::gil_scoped_release>());
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
    m.def("adam_step_multi", &adam_step_multi, py::arg("params"), py::arg("grads"), py::arg("exp_avgs"), py::arg("exp_avg_sqs"), py::arg("lrs"),
          py::arg("bias_correction1"), py::arg("bias_correction2_sqrt"), py::arg("beta1"), py::arg("beta2"), py::arg("eps"),
          py::arg("steps") = std::vector<Tensor>(), py::arg("done_scratch") = py::none(), py::call_guard<py::gil_scoped_release>());
    m.def("adam_dev_scratch_words", []() { return (int64_t)igs_adam_step_multi_dev_scratch_words(); });
    m.def("l1_mean", &l1_mean, py::arg("a"), py::arg("b"), py::call_guard<py::gil_scoped_release>());
    m.def("ssim_mean", &ssim_mean, py::arg("a"), py::arg("b"), py::call_guard<py::gil_scoped_release>());
    m.def("abi_version", []() { return igs_rast_version(); });
}
