"""Restatement of the densify-and-prune decision (include/igs_rast.h: igs_densify_plan; igs_amd/densify.py: plan, which restates
igs/models/gaussian_model.py:586-663) in float64 numpy with explicit normals -- the oracle of tests/test_gpu_densify_native.py, tied
to the pinned PyTorch plan by tests/test_densify_native_host.py.

The gradient statistic g = grad_accum / denom is a float32 quotient by definition (it is what the top-k orders, and two float32
quotients may be equal where the float64 ones are not); everything after it is float64.

with_margin() moves the inputs away from the four thresholds so that float32 rounding of exp / sigmoid cannot flip a class, and
classes_agree() is the assertion that float64 and float32 then classify identically."""
import numpy as np

MARGIN = 1e-4          # smallest relative distance of a value to its threshold after with_margin()


def _f64(a):
    return np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, dtype=np.float64)


def _f32(a):
    return np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, dtype=np.float32)


def gradient(grad_accum, denom):
    """g as float32: NaN (0/0) and negative values count as 0, +inf stays."""
    with np.errstate(divide="ignore", invalid="ignore"):
        g = _f32(grad_accum).reshape(-1) / _f32(denom).reshape(-1)
    g[np.isnan(g) | (g < 0)] = 0.0
    return g


def rotation_matrix(q):
    """densify.build_rotation: q / |q| (no epsilon), (w, x, y, z)."""
    q = q / np.sqrt((q * q).sum(axis=1, keepdims=True))
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                  2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                  2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], axis=1)
    return R.reshape(-1, 3, 3)


def select(g, grad_threshold, max_num_add, control_max):
    """Candidates after the max-points bound; ties at the cut go to the lowest index."""
    cand = g.astype(np.float64) >= grad_threshold
    if control_max and int(cand.sum()) > max_num_add:
        keep = np.zeros_like(cand)
        if max_num_add > 0:
            order = np.argsort(-g.astype(np.float64), kind="stable")          # descending g, ascending index among equals
            keep[order[:max_num_add]] = True
        cand = keep
    return cand


def restate(xyz, rotation, opacity_logit, log_scale, grad_accum, denom, normals, grad_threshold, min_opacity, split_scale_limit,
            world_scale_limit, max_num_add, control_max, candidates=None):
    """The dict of densify.plan / plan_native (numpy; ovr_xyz and ovr_scale in float64) plus, for the children's error bound,
    `child_R` [2 n_split, 3, 3], `child_v` [2 n_split, 3] = z * exp(log_scale) and `child_src` [2 n_split], the children's sources.
    `candidates` (bool [P]) replaces select(): for comparisons with torch.topk where the cut falls among equal gradients and the
    choice among them is torch's."""
    xyz, rotation, log_scale = _f64(xyz), _f64(rotation), _f64(log_scale)
    opa = 1.0 / (1.0 + np.exp(-_f64(opacity_logit).reshape(-1)))
    P = xyz.shape[0]
    g = gradient(grad_accum, denom)
    cand = select(g, grad_threshold, int(max_num_add), control_max) if candidates is None else np.asarray(candidates, dtype=bool)
    s = np.exp(log_scale)
    smax = s.max(axis=1) if P else np.zeros(0)
    big = smax > split_scale_limit
    idx_clone, idx_split = np.nonzero(cand & ~big)[0], np.nonzero(cand & big)[0]
    n_c, n_s = idx_clone.size, idx_split.size
    z = _f64(normals)[idx_split] if normals is not None else np.zeros((n_s, 2, 3))
    R = rotation_matrix(rotation[idx_split])
    v = np.concatenate([z[:, 0] * s[idx_split], z[:, 1] * s[idx_split]])                  # child c of source j: row c * n_s + j
    R2 = np.concatenate([R, R])
    ovr_xyz = np.einsum("nij,nj->ni", R2, v) + np.concatenate([xyz[idx_split]] * 2)
    ovr_scale = np.log(np.concatenate([s[idx_split]] * 2) / 1.6)
    src = np.concatenate([np.arange(P), idx_clone, idx_split, idx_split])
    fresh = np.concatenate([np.zeros(P, dtype=np.int64), np.ones(n_c + 2 * n_s, dtype=np.int64)])
    ovr = np.concatenate([np.full(P + n_c, -1, dtype=np.int64), np.arange(2 * n_s)])
    keep = np.concatenate([~(cand & big), np.ones(n_c + 2 * n_s, dtype=bool)])
    prune = opa[src] < min_opacity
    if world_scale_limit > 0:
        own = smax[src]
        own[P + n_c:] = np.exp(ovr_scale).max(axis=1) if n_s else 0.0
        prune |= own > world_scale_limit
    keep &= ~prune
    return dict(src=src[keep].astype(np.int32), fresh=fresh[keep].astype(np.int32), ovr=ovr[keep].astype(np.int32), ovr_xyz=ovr_xyz,
                ovr_scale=ovr_scale, n_clone=int(n_c), n_split=int(n_s), n_pruned=int((~keep).sum()) - int(n_s), child_R=R2, child_v=v,
                child_src=np.concatenate([idx_split, idx_split]))


def restate_cfg(t, state, cfg, normals, candidates=None):
    """restate() with the arguments densify.plan_native derives from a DensifyConfig; t: dict of xyz / rotation / opacity / scaling."""
    P = t["xyz"].shape[0]
    return restate(t["xyz"], t["rotation"], t["opacity"], t["scaling"], state.grad_accum, state.denom, normals, cfg.grad_threshold,
                   cfg.min_opacity, cfg.percent_dense * cfg.extent, 0.1 * cfg.extent if cfg.max_screen_size else 0.0, cfg.max_num - P,
                   cfg.control_max, candidates)


def _close(value, threshold):
    with np.errstate(invalid="ignore"):
        return np.abs(value / threshold - 1.0) < MARGIN


def with_margin(t, grad_accum, denom, cfg):
    """Copies of the inputs (torch float32 CPU tensors) in which every value closer than MARGIN (relative) to its threshold is moved
    away: g by scaling grad_accum, the largest scale (and the child's, 1 / 1.6 of it) by scaling the Gaussian, sigmoid(opacity) by
    shifting the logit."""
    import torch
    t = {k: v.clone() for k, v in t.items()}
    grad_accum = grad_accum.clone()
    split, world = cfg.percent_dense * cfg.extent, 0.1 * cfg.extent
    for _ in range(8):
        g = gradient(grad_accum, denom).astype(np.float64)
        smax = np.exp(_f64(t["scaling"])).max(axis=1)
        opa = 1.0 / (1.0 + np.exp(-_f64(t["opacity"]).reshape(-1)))
        bad_g = _close(g, cfg.grad_threshold)
        bad_s = _close(smax, split) | _close(smax, world) | _close(smax / 1.6, world)
        bad_o = _close(opa, cfg.min_opacity)
        if not (bad_g.any() or bad_s.any() or bad_o.any()):
            return t, grad_accum
        grad_accum[torch.from_numpy(bad_g)] *= 1.001
        t["scaling"][torch.from_numpy(bad_s)] += 0.001
        t["opacity"][torch.from_numpy(bad_o)] += 0.01
    raise AssertionError("with_margin did not converge")


def classes_agree(t, grad_accum, denom, cfg):
    """True when the float64 formulation and the float32 one of densify.plan put every Gaussian on the same side of the four
    thresholds (the tests assert this on the CPU before they compare decisions for equality)."""
    import torch
    split, world = cfg.percent_dense * cfg.extent, 0.1 * cfg.extent
    g = gradient(grad_accum, denom)
    s64 = np.exp(_f64(t["scaling"]))
    opa64 = 1.0 / (1.0 + np.exp(-_f64(t["opacity"]).reshape(-1)))
    c64 = [g.astype(np.float64) >= cfg.grad_threshold, s64.max(axis=1) > split, opa64 < cfg.min_opacity, s64.max(axis=1) > world,
           np.exp(np.log(s64 / 1.6)).max(axis=1) > world]
    g32 = torch.from_numpy(g)
    s32 = torch.exp(t["scaling"].float())
    c32 = [g32 >= cfg.grad_threshold, s32.max(dim=1).values > split, torch.sigmoid(t["opacity"].float().view(-1)) < cfg.min_opacity,
           s32.max(dim=1).values > world, torch.exp(torch.log(s32 / 1.6)).max(dim=1).values > world]
    return all(np.array_equal(a, b.numpy()) for a, b in zip(c64, c32))
