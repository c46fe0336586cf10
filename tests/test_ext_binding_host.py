"""The Python-visible surface of the compiled `_C` module (igs_amd/csrc_torch/igs_torch_ext.cpp) without a GPU: which names it exports,
and that its two backward functions -- generated from one parameter list -- name the same arguments in the same order."""
import re

PUBLIC = [
    "NotImplementedDtype", "RasterizerError", "ScratchSet", "abi_version", "adam_dev_scratch_words", "adam_step_multi",
    "anchors_bbox_select", "anchors_fps", "anchors_knn", "attn_bwd", "attn_fwd", "cond_ray_fwd", "count_gaussians", "distCUDA2",
    "forward_finish", "integrate_gaussians_to_points", "l1_mean", "mark_visible", "modln_bwd", "modln_fwd", "motion_deform_bwd",
    "motion_deform_fwd", "motion_interp_bwd", "motion_interp_fwd", "motion_interp_index", "motion_lift_bwd", "motion_lift_fwd",
    "nan_report_wait", "rasterize_gaussians", "rasterize_gaussians_backward", "rasterize_gaussians_backward_ex", "ssim_mean",
]
# the reference's 32 positional arguments (DGR/rasterize_points.cu:135-167), then this module's keyword-only extras
BACKWARD_POSITIONAL = [
    "background", "means3D", "radii", "colors", "scales", "rotations", "scale_modifier", "cov3D_precomp", "viewmatrix", "projmatrix",
    "tan_fovx", "tan_fovy", "kernel_size", "dL_dout_color", "dL_dout_coord", "dL_dout_mcoord", "dL_dout_depth", "dL_dout_mdepth",
    "dL_dout_alpha", "dL_dout_normal", "normalmap", "sh", "degree", "campos", "geomBuffer", "R", "binningBuffer", "imageBuffer", "alphas",
    "require_coord", "require_depth", "debug",
]
BACKWARD_EXTRAS = ["workspace", "out_means2D", "out_colors", "out_opacity", "out_means3D", "out_cov3D", "out_sh", "out_scales",
                   "out_rotations"]


def _ext():
    from igs_amd import _cabi
    return _cabi.ext()


def _signature(fn):
    """(positional names, keyword-only names with their defaults) from the first line of a pybind docstring."""
    line = fn.__doc__.splitlines()[0]
    m = re.match(r"%s\((.*)\) -> " % fn.__name__, line)
    assert m, line
    positional, _, kw_only = m.group(1).partition(", *, ")
    names = [a.split(": ")[0] for a in positional.split(", ")]
    return names, [(a.split(": ")[0], a.partition(" = ")[2]) for a in kw_only.split(", ")]


def test_public_names_of_the_compiled_module():
    E = _ext()
    assert sorted(n for n in dir(E) if not n.startswith("_")) == sorted(PUBLIC)
    classes = {n for n in PUBLIC if isinstance(getattr(E, n), type)}
    assert classes == {"NotImplementedDtype", "RasterizerError", "ScratchSet"}
    assert issubclass(E.RasterizerError, RuntimeError) and issubclass(E.NotImplementedDtype, NotImplementedError)
    for n in set(PUBLIC) - classes:
        assert callable(getattr(E, n)) and type(getattr(E, n)).__name__ == "builtin_function_or_method", n


def test_both_backward_functions_name_one_argument_list():
    E = _ext()
    pos, kw = _signature(E.rasterize_gaussians_backward)
    pos_ex, kw_ex = _signature(E.rasterize_gaussians_backward_ex)
    assert pos == BACKWARD_POSITIONAL and pos_ex == BACKWARD_POSITIONAL
    assert kw == [(n, "None") for n in BACKWARD_EXTRAS]
    assert kw_ex == kw + [("nan_report", "0"), ("clamp", "0.0")]
    # the annotations too, argument by argument: the text up to `nan_report` is the plain function's whole list
    args = E.rasterize_gaussians_backward.__doc__.splitlines()[0].split("(", 1)[1].rsplit(") -> ", 1)[0]
    args_ex = E.rasterize_gaussians_backward_ex.__doc__.splitlines()[0].split("(", 1)[1].rsplit(") -> ", 1)[0]
    assert args_ex.startswith(args + ", nan_report: ") and args_ex.count(", ") == args.count(", ") + 2
