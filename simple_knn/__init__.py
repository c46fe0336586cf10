"""Drop-in for the `simple-knn` package of 3DGS (the "Follow 3DGS to install simple-knn" step of RaDe-GS's README), backed by the
MI355X-native HIP library.

RaDe-GS (scene/gaussian_model.py:20) and IGS's refine-time model (igs/models/gaussian_model.py:19) import
`from simple_knn._C import distCUDA2`; create_from_pcd uses it for the initial scales.  distCUDA2(points [N, 3] float32 on a GPU)
returns, for every point, the mean of its three smallest squared distances to the other points (include/igs_rast.h:
igs_knn_mean_dist2 has the full contract, N <= 3 and non-finite points included).
"""
from . import _C  # noqa: F401
