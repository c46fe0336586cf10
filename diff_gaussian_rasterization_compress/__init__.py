"""Drop-in for the reference package `diff_gaussian_rasterization_compress`
(submodules/RaDe-GS/submodules/compress-diff-gaussian-rasterization/diff_gaussian_rasterization_compress/__init__.py),
backed by the MI355X-native HIP library.

RaDe-GS imports it next to the rade package (gaussian_renderer/__init__.py:15); LightGaussian pruning (compress.py, prune.py:prune_list)
calls it with `f_count=True` once per training view and reads `(gaussians_count, important_score, color, radii)`.  That count pass is
native (igs_rast_count_gaussians: vanilla preprocess, slab binning, a counting colour-only blend).  Two deliberate differences:
  * `gaussians_count[i]` is the exact number of pixels Gaussian i is blended into, and `important_score[i]` is
    `gaussians_count[i] * opacity[i]` rounded once -- the reference increments both with unsynchronised read-modify-writes from
    256 threads at once, so its values undercount by a run-dependent amount;
  * the vanilla training path (`f_count=False` and the backward) is not built and raises NotImplementedError: RaDe-GS trains and
    renders through diff_gaussian_rasterization_rade.
"""
from typing import NamedTuple

import torch
import torch.nn as nn

from . import _C


def cpu_deep_copy_tuple(input_tuple):
    return tuple(item.cpu().clone() if isinstance(item, torch.Tensor) else item for item in input_tuple)


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings):
    if raster_settings.f_count:
        return _RasterizeGaussians.forward_count(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                                                 raster_settings)
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings)


def _count_args(means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, rs):
    # the reference's argument order (rasterize_points.cu CountGaussiansCUDA)
    return (rs.bg, means3D, colors_precomp, opacities, scales, rotations, rs.scale_modifier, cov3Ds_precomp, rs.viewmatrix,
            rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width, sh, rs.sh_degree, rs.campos, rs.prefiltered,
            rs.debug, rs.f_count)


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings):
        if not raster_settings.f_count:
            raise NotImplementedError(_C.TRAINING_PATH_MESSAGE)
        # (f_count=True through apply: the reference returns the count pass's four outputs, none of them differentiable here)
        out = _RasterizeGaussians.forward_count(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                                                raster_settings)
        ctx.mark_non_differentiable(*out)
        return out

    @staticmethod
    def forward_count(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings):
        assert raster_settings.f_count
        args = _count_args(means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings)
        if raster_settings.debug:
            cpu_args = cpu_deep_copy_tuple(args)      # Copy them before they can be corrupted
            try:
                gaussians_count, important_score, num_rendered, color, radii, geomBuffer, binningBuffer, imgBuffer = _C.count_gaussians(*args)
            except Exception as ex:
                torch.save(cpu_args, "snapshot_fw.dump")
                print("\nAn error occured in forward. Please forward snapshot_fw.dump for debugging.")
                raise ex
        else:
            gaussians_count, important_score, num_rendered, color, radii, geomBuffer, binningBuffer, imgBuffer = _C.count_gaussians(*args)
        return gaussians_count, important_score, color, radii

    @staticmethod
    def backward(ctx, *grads):
        raise NotImplementedError(_C.TRAINING_PATH_MESSAGE)


class GaussianRasterizationSettings(NamedTuple):
    """Field order is API (the reference's __init__.py, class GaussianRasterizationSettings)."""
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool
    f_count: bool


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions):
        # Mark visible points (based on frustum culling for camera) with a boolean
        with torch.no_grad():
            raster_settings = self.raster_settings
            visible = _C.mark_visible(positions, raster_settings.viewmatrix, raster_settings.projmatrix)
        return visible

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None):
        raster_settings = self.raster_settings
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception('Please provide excatly one of either SHs or precomputed colors!')
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')
        if shs is None:
            shs = torch.Tensor([])
        if colors_precomp is None:
            colors_precomp = torch.Tensor([])
        if scales is None:
            scales = torch.Tensor([])
        if rotations is None:
            rotations = torch.Tensor([])
        if cov3D_precomp is None:
            cov3D_precomp = torch.Tensor([])
        return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, raster_settings)

    # the reference's second entry point (same checks, same call)
    forward_count = forward
