"""The functions of the compress package's pybind module, from the compiled module igs_amd/_C.*.so
(igs_amd/csrc_torch/igs_torch_ext.cpp: torch glue over the C ABI of libigs_rast.so).

`count_gaussians` (CountGaussiansCUDA) and `mark_visible` are native.  The vanilla training path -- `rasterize_gaussians` /
`rasterize_gaussians_backward` of vanilla 3DGS -- is not built: RaDe-GS trains and renders through diff_gaussian_rasterization_rade."""
from igs_amd._cabi import ext as _ext

_m = _ext()
count_gaussians = _m.count_gaussians
mark_visible = _m.mark_visible

TRAINING_PATH_MESSAGE = ("the vanilla 3DGS forward / backward of diff_gaussian_rasterization_compress is not implemented on this backend "
                         "(only the count pass, f_count=True, is): train and render with diff_gaussian_rasterization_rade")


def rasterize_gaussians(*args, **kwargs):
    raise NotImplementedError(TRAINING_PATH_MESSAGE)


def rasterize_gaussians_backward(*args, **kwargs):
    raise NotImplementedError(TRAINING_PATH_MESSAGE)
