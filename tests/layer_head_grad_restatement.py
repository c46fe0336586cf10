"""Float64 restatement of what igs_amd/csrc/proj_bwd.hip computes (the backward of the fused projections of tests/layer_head_restatement.py,
written out with the roll), the transposed pack as that kernel reads it, restated without the library's packer, the scratch size, and the
C ABI's refusals as a list that the host test and the GPU test share."""
import torch

import layer_head_restatement as LH
import layer_tail_restatement as LR

D = LH.D
MAX_SLICES = 64                                                     # IGS_TOKEN_PROJ_BWD_MAX_SLICES
MIN_SLICE_ROWS = 512
DW_BYTES = D * D * 4


# ---------------------------------------------------------------- the computation
def rolled_back(g, r):
    """g_j[t] for every t: row (t + r) mod T of output j's gradient."""
    T = g.shape[0]
    return g[(torch.arange(T, device=g.device) + r) % max(T, 1)]


def project_grad_restate(x, weights, grads, rot=None):
    """(d x [T, 128], [d W_j [128, 128] or None]) in the dtype of x (pass float64).  grads: n entries [T, 128], the gradient of each
    output as the forward wrote it, or None for an output without one."""
    dx = torch.zeros_like(x)
    dws = []
    for j, (W, g) in enumerate(zip(weights, grads)):
        if g is None:
            dws.append(None)
            continue
        gj = rolled_back(g, 0 if rot is None else rot[j])
        dx = dx + gj @ W                                            # W_j^T g_j[t], row by row
        dws.append(gj.t() @ x)                                      # sum_t g_j[t] (x) x[t]
    return dx, dws


def slice_plan(T):
    """(rows of a slice, slices, slices the scratch has room for)."""
    least = -(-T // MIN_SLICE_ROWS)
    rows = MIN_SLICE_ROWS
    if least > MAX_SLICES:
        rows = -(-(-(-T // MAX_SLICES)) // 128) * 128
    return rows, -(-T // rows), min(least, MAX_SLICES)


def scratch_bytes(T, n):
    return slice_plan(T)[2] * n * DW_BYTES


# ---------------------------------------------------------------- the allowance
FLOOR = {torch.float32: 1e-5, torch.float16: 2e-3}                  # as tests/test_gpu_layer_head.py


def rel(got, ref):
    return ((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def four_times(label, fused, cmp_, ref, cdt):
    """The project's four-times rule on max |err| / max |ref|: `fused` may be at most 4 x as far from the float64 `ref` as the comparator
    `cmp_` is, with the floor of the compute dtype.  Prints both errors."""
    assert not torch.isnan(fused).any(), (label, "an element was not written")
    e_f, e_c = rel(fused, ref), rel(cmp_, ref)
    allowed = max(4 * e_c, FLOOR[cdt])
    print("%s: max |err| / max |ref| against float64: comparator %.3e, fused %.3e (allowed %.3e)" % (label, e_c, e_f, allowed))
    assert e_f <= allowed, (label, e_f, e_c)


def linear_autograd(x, weights, grads, rot, cdt, dx_dtype):
    """The comparator: F.linear under autograd on the same inputs in the compute dtype `cdt`, outputs rolled as the forward writes them;
    (d x rounded to dx_dtype, [d W_j as float32 or None])."""
    import torch.nn.functional as F
    xc = x.detach().to(cdt).clone().requires_grad_(True)            # (leaves of their own: nothing accumulates into the caller's tensors)
    ws = [w.detach().to(cdt).clone().requires_grad_(True) for w in weights]
    outs = [torch.roll(F.linear(xc, w), 0 if rot is None else rot[j], 0) for j, w in enumerate(ws)]
    used = [(o, g.to(cdt)) for o, g in zip(outs, grads) if g is not None]
    if used:
        torch.autograd.backward([o for o, _ in used], [g for _, g in used])
    dx = torch.zeros_like(xc) if xc.grad is None else xc.grad
    return dx.to(dx_dtype), [None if g is None else w.grad.float() for w, g in zip(ws, grads)]


# ---------------------------------------------------------------- the transposed pack, element by element
def pack_transposed(weights):
    """Matrix j is W_j^T: element e of lane (r, h) of tile (ot, kt) is W_j^T[32 ot + r][32 kt + (e & 3) + 8 (e >> 2) + 4 h], i.e.
    W_j[32 kt + (e & 3) + 8 (e >> 2) + 4 h][32 ot + r]; float32 tiles keep a lane's elements in chunks of 4 (chunk q of lane l at
    (q 64 + l) 4), float16 tiles in chunks of 8 (chunk s of lane l at (s 64 + l) 8); tile 4 ot + kt."""
    half = weights[0].dtype == torch.float16
    E = 8 if half else 4
    out = weights[0].new_zeros(len(weights) * LH.MATRIX)
    ot, kt, h, r, e = torch.meshgrid(torch.arange(4), torch.arange(4), torch.arange(2), torch.arange(32), torch.arange(16), indexing="ij")
    pos = (4 * ot + kt) * LR.TILE + ((e // E) * 64 + 32 * h + r) * E + e % E
    row, col = 32 * kt + (e & 3) + 8 * (e >> 2) + 4 * h, 32 * ot + r
    for j, W in enumerate(weights):
        out[j * LH.MATRIX + pos.reshape(-1)] = W.to(weights[0].dtype)[row.reshape(-1), col.reshape(-1)]
    return out


# ---------------------------------------------------------------- the C ABI's refusals
ORDER = ("T", "n", "cdt", "x", "xdt", "xstr", "g", "gdt", "gstr", "rot", "wt", "scr", "sbytes", "dx", "dxdt", "dxstr", "dW")


def good_call(X, G, WT, SCR, DX, DW):
    """T = 5, n = 3: G and DW are the addresses of output 0's operand, the others follow at 0x100000 each."""
    step = 0x100000
    return dict(T=5, n=3, cdt=0, x=X, xdt=0, xstr=128, g=(G, G + step, G + 2 * step), gdt=0, gstr=(128, 128, 128), rot=(0, 0, 0), wt=WT, scr=SCR,
                sbytes=1 << 30, dx=DX, dxdt=0, dxstr=128, dW=(DW, DW + step, DW + 2 * step))


def refusals(X, G, WT, SCR, DX, DW):
    """[(what differs from good_call, a word of the reason)]: each case differs from a call that would pass in the one thing its reason
    names.  The addresses: spans that do not meet, 0x100000 apart for the three g and the three dW, with room for a few bytes more."""
    big, step = (1 << 31) + 4, 0x100000
    g, dW = (G, G + step, G + 2 * step), (DW, DW + step, DW + 2 * step)
    need = scratch_bytes(5, 3)
    swap = lambda t, i, v: tuple(v if k == i else a for k, a in enumerate(t))
    return ([(dict([(k, v)]), "dtype") for k in ("cdt", "xdt", "gdt", "dxdt") for v in (-1, 2)]
            + [(dict(n=v), "n out of range") for v in (0, -1, LH.MAX_OUT + 1)]
            + [(dict(T=-1), "T out of range"), (dict(T=LH.MAX_ROWS + 1), "T out of range")]
            + [(dict([(k, v)]), "row stride") for k in ("xstr", "dxstr") for v in (127, 0, -128, big)]
            + [(dict(gstr=swap((128,) * 3, i, v)), "row stride") for i, v in ((0, 127), (1, 0), (2, -128), (1, big))]
            + [(dict(rot=r), "rot") for r in ((0, 0, 5), (-1, 0, 0), (0, 1 << 40, 0))] + [(dict(T=1, rot=(0, 1, 0)), "rot")]
            + [(dict(x=None), "NULL"), (dict(wt=None), "NULL"), (dict(scr=None), "NULL"), (dict(gstr=None), "NULL")]
            + [(dict(x=X + 2), "aligned to its element size"), (dict(xdt=1, x=X + 1), "aligned to its element size"),
               (dict(dx=DX + 2), "aligned to its element size"), (dict(dxdt=1, dx=DX + 1), "aligned to its element size"),
               (dict(g=swap(g, 1, g[1] + 2)), "aligned to its element size"), (dict(gdt=1, g=swap(g, 2, g[2] + 1)), "aligned to its element size")]
            + [(dict(wt=WT + 4), "16 bytes"), (dict(wt=WT + 8), "16 bytes"), (dict(cdt=1, wt=WT + 2), "16 bytes"), (dict(scr=SCR + 8), "16 bytes"),
               (dict(dW=swap(dW, 0, DW + 4)), "16 bytes"), (dict(dW=swap(dW, 2, dW[2] + 8)), "16 bytes")]
            + [(dict(sbytes=need - 1), "scratch is smaller"), (dict(sbytes=0), "scratch is smaller"), (dict(T=513, sbytes=need), "scratch is smaller")]
            # an output over an input or another output: the same base, an input's last element, rows between rows at wider strides
            + [(dict(dx=X), "dx overlaps"), (dict(dx=g[1] + (4 * 128 + 127) * 4), "dx overlaps"),
               (dict(xstr=1024, dx=X + 128 * 4, dxstr=1024), "dx overlaps"), (dict(dx=WT + 3 * LH.MATRIX * 4 - 16), "dx overlaps"),
               (dict(dW=swap(dW, 1, X)), "overlaps"), (dict(dW=swap(dW, 0, g[2] + 16)), "overlaps"), (dict(dW=swap(dW, 2, DX + 16)), "overlaps"),
               (dict(dW=swap(dW, 1, DW + 64)), "overlaps"), (dict(dW=(DW, DW, None)), "overlaps"),
               (dict(scr=X + 16), "overlaps"), (dict(scr=DX), "overlaps"), (dict(scr=dW[1] - need + 16), "overlaps"), (dict(scr=WT), "overlaps")])


def call_abi(lib, stream, k):
    import ctypes
    arr = lambda t, ty: None if t is None else (ty * len(t))(*t)
    return lib.igs_token_proj_bwd(stream, k["T"], k["n"], k["cdt"], k["x"], k["xdt"], k["xstr"], arr(k["g"], ctypes.c_void_p), k["gdt"],
                                  arr(k["gstr"], ctypes.c_longlong), arr(k["rot"], ctypes.c_longlong), k["wt"], k["scr"], k["sbytes"], k["dx"],
                                  k["dxdt"], k["dxstr"], arr(k["dW"], ctypes.c_void_p))
