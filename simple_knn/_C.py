"""The functions of simple-knn's pybind module, from the compiled module igs_amd/_C.*.so (igs_amd/csrc_torch/igs_torch_ext.cpp:
torch glue over igs_knn_mean_dist2 of libigs_rast.so)."""
from igs_amd._cabi import ext as _ext

distCUDA2 = _ext().distCUDA2
