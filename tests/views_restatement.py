"""The multi-view backward restated from the single-view oracle (helper of tests/test_views_host.py and tests/test_gpu_views.py; no test).

`rasterize_views` promises the SUM over the views of what V single-view backward passes give, each view's gradients clamped first in the
clamp variant.  `oracle_views` forms exactly that from `certificate.oracle_all` per view, in float64 and in float32, so that
`certificate.certify` can hold the summed HIP gradients to the bar of a single view.

The tolerance needs no new derivation: an element's allowance in `certify` is 5 x |oracle32 - f64| (read from g32 and g64) + 5 x shift.
For a sum, |sum_v a_v - sum_v b_v| <= sum_v |a_v - b_v|, and clamping is 1-Lipschitz, |clamp(a) - clamp(b)| <= |a - b|, so the views'
shifts add up to a shift of the clamped sum, and the clamped float32 sum's distance from the clamped float64 sum is what `certify`
measures anyway.  means2D is per view: it is left out of the sum (an empty entry, which `certify` passes over) and
certified view by view against `ob["views"][v]`.
"""
import numpy as np

import certificate as cert

CLAMPED = ("means3D", "sh", "opacity", "scales", "rotations")      # what the clamp package clamps (means2D, colours, cov3D are not)


def clamp_view(name, g, clamp):
    """One view's tensor as the clamp variant hands it to the sum."""
    return np.clip(g, -clamp, clamp) if (clamp > 0 and name in CLAMPED) else g


def sum_views(obs, clamp=0.0):
    """The `ob` of the sum from the per-view results of `certificate.oracle_all` (shared between tests: the oracle runs once per view)."""
    ob = {"views": obs, "g64": {}, "g32": {}, "shift": {}, "nr": [o["nr"] for o in obs]}
    for n in cert.GNAMES:
        if n == "means2D":
            ob["g64"][n] = ob["g32"][n] = np.zeros((0,))      # (size 0: `certify` passes it over)
            continue
        ob["g64"][n] = sum(clamp_view(n, np.asarray(o["g64"][n], np.float64), clamp) for o in obs)
        # (float32 views are added in float64: the sum's own rounding, at most V - 1 half-ulps, is far inside the plain 1e-3 bar)
        ob["g32"][n] = sum(clamp_view(n, np.asarray(o["g32"][n], np.float64), clamp) for o in obs)
        if obs[0]["g32"][n].size:
            ob["shift"][n] = sum(o["shift"][n] for o in obs)
    return ob


def oracle_views(a, cams, bg, grads_per_view, clamp=0.0, **kw):
    """`ob` for `certificate.certify` of the gradients summed over `cams` (`grads_per_view[v]`: view v's seven upstream image gradients).
    g64 / g32: sum over the views, each view clamped to +-clamp first where the clamp package clamps; shift: the sum of the views' shifts.
    Also returns the per-view oracle results under "views" (their means2D is what the per-view dL_dmeans2D is certified against)."""
    return sum_views([cert.oracle_all(a, cam, bg, g, **kw) for cam, g in zip(cams, grads_per_view)], clamp)


def certify_views(gout, ob, label, **kw):
    """`certify` of the seven summed tensors (gout in GNAMES order; entry 0, means2D, is [V, P, 3] or None and is certified per view)."""
    m2d = gout[0]
    stats = cert.certify([None] + list(gout[1:]), ob, label, **kw)
    if m2d is not None:
        for v, o in enumerate(ob["views"]):
            only = {"g32": {n: (o["g32"][n] if n == "means2D" else np.zeros((0,))) for n in cert.GNAMES}, "g64": o["g64"], "shift": o["shift"]}
            cert.certify([m2d[v]] + [None] * 7, only, "%s means2D of view %d" % (label, v), **kw)
    return stats
