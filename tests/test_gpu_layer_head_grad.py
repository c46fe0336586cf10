"""The backward of the fused q / k / v projections (igs_amd/csrc/proj_bwd.hip through the C ABI and through igs_amd.tokens) against the
float64 restatement of tests/layer_head_grad_restatement.py on the same float32 / float16 inputs, and the two binders with training=True.

Every element of d x and of each d W_j is compared.  The allowance is the project's four-times rule on max |err| / max |ref|: the comparator
is F.linear under autograd on the same inputs in the same compute dtype (its d x rounded to the written dtype), and the native result may be
at most 4 x as far from float64 as that comparator is, with the floors of test_gpu_layer_head.py (1e-5 in float32, 2e-3 in float16).  For the
binders the comparator is the same stand-in transformer bound with use_native_layer_tails alone.  Both errors are printed for every case.

The C ABI cases run on PyTorch's current stream so that the test chooses where the operands lie (the Rows scheme of test_gpu_layer_head.py):
rows at strides above the minimum, bases one element off the 16-byte grid, mixed x / g / d x dtypes, outputs pre-filled with NaN inside
allocations that hold a sentinel everywhere else, the scratch included, which is checked afterwards.

The binder tests set the routing constants they depend on, so that they pin the kernels' paths whatever the measurements of DESIGN.md
section 28 decide.

Recorded on one MI355X ("The backward"), max |err| / max |ref| against float64, native beside the comparator: float32
compute d x 3.2e-7 to 9.8e-7 beside 2.4e-7 to 5.2e-7 (4.4e-4 on both sides where d x is written as float16), d W up to 1.4e-6 beside up to
6.2e-6; float16 compute d x 2.0e-4 to 5.1e-4 beside 3.7e-4 to 1.0e-3, d W up to 6.1e-4 beside 2.4e-4 to 8.2e-4 (the native d W is never
rounded to half); through .backward() 3.5e-7 to 7.2e-7 beside 2.8e-7 to 5.8e-7 in float32 and 3.1e-4 to 6.1e-4 beside 3.8e-4 to 6.3e-4 under
autocast; the bound stand-in transformers, per gradient tensor, up to 2.8e-6 beside up to 3.3e-6 in float32 and up to 6.3e-3 beside up to
6.4e-3 under float16 autocast."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import layer_head_grad_restatement as GR
import layer_head_restatement as LH
import token_ops_restatement as TR
import window_attention_restatement as WR
from test_gpu_layer_head import Counter, Rows, SENTINEL, _attention, _bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F16 = torch.float32, torch.float16
CODE = {F32: 0, F16: 1}
E_INVALID = -1


def _lib():
    from igs_amd import _cabi
    return _cabi.lib()


def _ok(rc):
    from igs_amd import _cabi
    assert rc == 0, _cabi.last_error()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Heads:
    """n weights as the C ABI takes them: float64 and float32 copies and the transposed pack per compute dtype on the GPU."""

    def __init__(self, n, seed=0):
        self.n = n
        self.w32 = [w.to(DEV) for w in LH.make_weights(n, seed, F32)]
        self.w64 = [w.double() for w in self.w32]
        self.packs_t = {dt: GR.pack_transposed([w.cpu().to(dt) for w in self.w32]).contiguous().to(DEV) for dt in (F32, F16)}

    def run(self, cdt, x, gs, rot, dx, dws, scratch=None):
        """x: Rows; gs: n Rows or None; dx: Rows or None; dws: n Rows or None, or None for a NULL array.  Returns the scratch's Rows."""
        T, n = x.v.shape[0], self.n
        if scratch is None and dws is not None:
            scratch = Rows(1, max(GR.scratch_bytes(T, n) // 4, 4), F32)
        gdt = next((g.v.dtype for g in gs if g is not None), F32)
        gp = (ctypes.c_void_p * n)(*[None if g is None else g.v.data_ptr() for g in gs])
        gst = (ctypes.c_longlong * n)(*[128 if g is None else g.stride for g in gs])
        r = None if rot is None else (ctypes.c_longlong * n)(*rot)
        wp = None if dws is None else (ctypes.c_void_p * n)(*[None if d is None else d.v.data_ptr() for d in dws])
        _ok(_lib().igs_token_proj_bwd(_stream(), T, n, CODE[cdt], x.v.data_ptr(), CODE[x.v.dtype], x.stride, gp, CODE[gdt], gst, r,
                                      self.packs_t[cdt].data_ptr(), None if scratch is None else scratch.v.data_ptr(),
                                      0 if scratch is None else scratch.v.numel() * 4, None if dx is None else dx.v.data_ptr(),
                                      CODE[F32 if dx is None else dx.v.dtype], 128 if dx is None else dx.stride, wp))
        return scratch

    def dense(self, cdt, x, grads, rot=None, want_dw=True):
        """(d x, [d W_j]) for contiguous float32 tensors."""
        T = x.shape[0]
        rx, gs = Rows(T, 128, F32, src=x), [None if g is None else Rows(T, 128, F32, src=g) for g in grads]
        dx, dws = Rows(T, 128, F32), [Rows(128, 128, F32) for _ in range(self.n)] if want_dw else None
        scratch = self.run(cdt, rx, gs, rot, dx, dws)
        for r in [rx, dx] + [g for g in gs if g is not None] + (dws or []) + ([scratch] if scratch is not None else []):
            r.check("dense")
        return dx.v.clone(), None if dws is None else [d.v.clone() for d in dws]


_HEADS = {}


@pytest.fixture(scope="module", autouse=True)
def _leave_no_cached_blocks():
    """As in test_gpu_layer_head.py: this file returns what it allocated."""
    yield
    _HEADS.clear()
    _REFS.clear()
    if torch.cuda.is_available():
        import gc
        gc.collect()
        torch.cuda.empty_cache()


def _heads(n):
    if n not in _HEADS:
        _HEADS[n] = Heads(n, seed=n)
    return _HEADS[n]


def _rot_for(T, n, turn=0):
    """Offsets from {0, 1, T / 2, T - 1}, a different one for neighbouring outputs."""
    return [(0, 1 % T, T // 2, T - 1)[(j + turn) % 4] for j in range(n)]


def _grads64(T, n, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(T, 128, dtype=torch.float64, generator=g).to(DEV) for _ in range(n)]


# (x dtype, g dtype, d x dtype, extra stride of x / g / d x, offset from the 16-byte grid)
VARIANTS = [(F32, F32, F32, (0, 0, 0), 0), (F32, F32, F32, (4, 8, 12), 0), (F32, F32, F32, (3, 5, 1), 1), (F16, F16, F16, (0, 0, 0), 0),
            (F32, F16, F32, (128, 4, 0), 0), (F16, F16, F16, (2, 6, 0), 1), (F16, F32, F16, (8, 8, 8), 0), (F32, F16, F16, (0, 256, 4), 0)]


def _abi_case(heads, cdt, T, variant, seed, turn=0, none=(), want_dx=True, want_dw=True):
    """One call with every operand in a sentinel allocation, compared element by element.  none: the outputs without a gradient;
    want_dw: True, None (a NULL array) or the set of j that are wanted."""
    xdt, gdt, ddt, extra, offset = variant
    n = heads.n
    x64 = LH.project_inputs(T, seed, DEV)
    g64 = _grads64(T, n, seed + 1)
    x = Rows(T, 128, xdt, 128 + extra[0], offset, x64.to(xdt))
    gs = [None if j in none else Rows(T, 128, gdt, 128 + extra[1] + 4 * j, offset, g64[j].to(gdt)) for j in range(n)]
    dx = Rows(T, 128, ddt, 128 + extra[2], offset) if want_dx else None
    wanted = set(range(n)) if want_dw is True else set(want_dw or ())
    dws = None if want_dw is None else [Rows(128, 128, F32) if j in wanted else None for j in range(n)]
    rot = _rot_for(T, n, turn)
    label = "T %d n %d compute %s x %s g %s dx %s stride +%s offset %d rot %s none %s" % (
        T, n, str(cdt)[6:], str(xdt)[6:], str(gdt)[6:], str(ddt)[6:], extra, offset, rot, none)
    scratch = heads.run(cdt, x, gs, rot, dx, dws)
    for r in [x, dx, scratch] + gs + (dws or []):
        if r is not None:
            r.check(label)
    assert torch.equal(x.v.double(), x64.to(xdt).double()), (label, "x was written")
    grads = [None if g is None else g.v.contiguous() for g in gs]
    for j, g in enumerate(gs):
        assert g is None or torch.equal(g.v.double(), g64[j].to(gdt).double()), (label, "a gradient was written")
    ref_dx, ref_dw = GR.project_grad_restate(x.v.double(), heads.w64, [None if g is None else g.double() for g in grads], rot)
    cmp_dx, cmp_dw = GR.linear_autograd(x.v.contiguous(), heads.w32, grads, rot, cdt, ddt)
    if want_dx:
        if len(none) == n:
            assert not dx.v.any(), (label, "d x with no gradient at all is zero")
        else:
            GR.four_times(label + ": d x", dx.v, cmp_dx, ref_dx, cdt)
    for j in sorted(wanted):
        if j in none:
            assert dws[j].v.dtype == F32 and not dws[j].v.any(), (label, j, "d W_j of an output without a gradient is zero")
        else:
            GR.four_times(label + ": d W_%d" % j, dws[j].v, cmp_dw[j], ref_dw[j], cdt)


# ---------------------------------------------------------------- 1. through the C ABI against float64
# a trip of the d x kernel is 128 rows, a wave's share 32; a slice of the weight-gradient kernel 512 rows, up to 64 of them, longer above
CAP_ROWS = GR.MIN_SLICE_ROWS * GR.MAX_SLICES
SIZES = (1, 31, 33, 127, 128, 129, 288, GR.MIN_SLICE_ROWS - 1, GR.MIN_SLICE_ROWS + 1, CAP_ROWS + 1)


@pytest.mark.parametrize("cdt", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_every_element_against_float64_at_the_wave_trip_and_slice_boundaries(n, cdt):
    assert GR.slice_plan(CAP_ROWS + 1)[0] > GR.MIN_SLICE_ROWS and GR.slice_plan(GR.MIN_SLICE_ROWS + 1)[1] == 2
    heads = _heads(n)
    for i, T in enumerate(SIZES):
        _abi_case(heads, cdt, T, VARIANTS[(i + n) % len(VARIANTS)], seed=7 * T + n, turn=i)


@pytest.mark.parametrize("cdt", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("n", [2, 5])
def test_operand_layouts_null_gradients_null_dx_and_a_null_dw_array(n, cdt):
    heads = _heads(n)
    for v, variant in enumerate(VARIANTS):                                                       # every layout just past a wave's share and a trip
        _abi_case(heads, cdt, (33, 129)[v % 2], variant, seed=11 * v + n, turn=v)
    _abi_case(heads, cdt, 129, VARIANTS[2], seed=1, turn=1, none=(1,))                           # a NULL g[j]: skipped by d x, its d W_j zeros
    _abi_case(heads, cdt, 129, VARIANTS[4], seed=2, turn=2, none=(0,), want_dw={1})              # ... and not wanted at all
    _abi_case(heads, cdt, 129, VARIANTS[1], seed=3, turn=3, none=tuple(range(n)))                # no gradient at all: zeros
    _abi_case(heads, cdt, 130, VARIANTS[5], seed=4, turn=0, want_dx=False)                       # NULL d x
    _abi_case(heads, cdt, 130, VARIANTS[6], seed=5, turn=1, want_dw=None)                        # a NULL d W array: no scratch either
    _abi_case(heads, cdt, 130, VARIANTS[3], seed=6, turn=2, want_dw={n - 1})                     # one d W_j alone


def test_t_zero_zero_fills_the_wanted_weight_gradients_and_writes_no_dx():
    heads = _heads(3)
    x, dx = Rows(0, 128, F32), Rows(0, 128, F32)
    dws = [Rows(128, 128, F32), None, Rows(128, 128, F32)]
    heads.run(F32, x, [None] * 3, None, dx, dws, scratch=None)
    torch.cuda.synchronize()
    for r in (x, dx, dws[0], dws[2]):
        r.check("T = 0")
    assert not dws[0].v.any() and not dws[2].v.any()


@pytest.mark.parametrize("cdt", [F32, F16], ids=["f32", "f16"])
def test_a_workgroup_takes_a_second_trip_of_dx(cdt):
    """The forward's launch rule: min(trips, compute units x (float16 ? 2 : 1)) workgroups, so one row more than a full grid of trips sends
    workgroup 0 round its loop again.  No float64 reference at this size: rows from both ends and the middle must have the bits they have
    in a small call (a row's d x depends on that row's gradients and the weights only)."""
    n = 3
    heads = _heads(n)
    groups = torch.cuda.get_device_properties(0).multi_processor_count * (2 if cdt == F16 else 1)
    T = groups * LH.TRIP_ROWS + 1
    gen = torch.Generator(DEV).manual_seed(3)
    x = torch.zeros(1, 128, device=DEV).expand(T, 128)
    gs = [torch.randn(T, 128, device=DEV, generator=gen) for _ in range(n)]
    rot = _rot_for(T, n, 1)
    rx, rg, dx = Rows(T, 128, F32, src=x), [Rows(T, 128, F32, src=g) for g in gs], Rows(T, 128, F32, 132)
    heads.run(cdt, rx, rg, rot, dx, None)
    dx.check("second trip")
    assert not torch.isnan(dx.v).any(), "an element was not written"
    pick = torch.cat([torch.arange(0, 200), torch.arange(T // 2 - 70, T // 2 + 70), torch.arange(T - 200, T)]).to(DEV)
    small, _ = heads.dense(cdt, x[pick].contiguous(), [g[(pick + rot[j]) % T].contiguous() for j, g in enumerate(gs)], want_dw=False)
    assert torch.equal(_bits(dx.v[pick]), _bits(small)), "rows of the large call differ from the small call's"


# ---------------------------------------------------------------- 2. bits
@pytest.mark.parametrize("cdt", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("n", [2, 5])
def test_two_runs_agree_and_a_row_has_the_same_bits_alone_and_elsewhere(n, cdt):
    heads = _heads(n)
    T = 600                                                                                      # two slices
    x = LH.project_inputs(T, 11, DEV).to(F32)
    gs = [g.to(F32) for g in _grads64(T, n, 12)]
    rot = _rot_for(T, n, 2)
    dx, dws = heads.dense(cdt, x, gs, rot)
    dx2, dws2 = heads.dense(cdt, x, gs, rot)
    assert torch.equal(_bits(dx), _bits(dx2)) and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(dws, dws2)), "two runs of the same call differ"
    other_x = LH.project_inputs(50, 13, DEV).to(F32)
    other_g = [g.to(F32) for g in _grads64(50, n, 14)]
    for i in (0, 31, 37, 127, 128, 511, 512, 599):
        mine = [g[(i + rot[j]) % T] for j, g in enumerate(gs)]
        alone, _ = heads.dense(cdt, x[i: i + 1], [m[None].contiguous() for m in mine], want_dw=False)
        assert torch.equal(_bits(alone[0]), _bits(dx[i])), (i, "alone")
        moved = [g.clone() for g in other_g]
        for m, g in zip(mine, moved):
            g[13] = m
        there, _ = heads.dense(cdt, other_x, moved, want_dw=False)
        assert torch.equal(_bits(there[13]), _bits(dx[i])), (i, "at another position, beside another x")


@pytest.mark.parametrize("cdt", [F32, F16], ids=["f32", "f16"])
def test_a_nan_stays_in_its_row_of_dx_and_reaches_the_weight_gradient(cdt):
    n, T, bad = 3, 140, 77
    heads = _heads(n)
    x = LH.project_inputs(T, 5, DEV).to(F32)
    gs = [g.to(F32) for g in _grads64(T, n, 6)]
    rot = _rot_for(T, n, 1)
    clean_dx, clean_dw = heads.dense(cdt, x, gs, rot)
    # in g_1: the row of x it belongs to is bad - rot[1]
    dirty = [g.clone() for g in gs]
    dirty[1][bad, 19] = float("nan")
    dx, dws = heads.dense(cdt, x, dirty, rot)
    hit = torch.zeros(T, dtype=torch.bool, device=DEV)
    hit[(bad - rot[1]) % T] = True
    assert torch.isnan(dx[hit]).all() and torch.equal(_bits(dx[~hit]), _bits(clean_dx[~hit])), "a NaN in g_1 left its row of d x"
    assert torch.isnan(dws[1][19]).all() and not torch.isnan(dws[1][:19]).any() and not torch.isnan(dws[1][20:]).any()
    assert torch.equal(_bits(dws[0]), _bits(clean_dw[0])) and torch.equal(_bits(dws[2]), _bits(clean_dw[2]))
    # in x: d x does not read x; every d W_j has the NaN in x's column
    xd = x.clone()
    xd[bad, 19] = float("nan")
    dx, dws = heads.dense(cdt, xd, gs, rot)
    assert torch.equal(_bits(dx), _bits(clean_dx)), "a NaN in x reached d x"
    for j in range(n):
        assert torch.isnan(dws[j][:, 19]).all(), j
        keep = torch.ones(128, dtype=torch.bool, device=DEV)
        keep[19] = False
        assert torch.equal(_bits(dws[j][:, keep]), _bits(clean_dw[j][:, keep])), j


# ---------------------------------------------------------------- 3. refused calls
def test_a_refused_call_launches_nothing():
    """The host test's list with device memory behind the addresses: every case is refused, and afterwards the outputs still hold their
    fill and the inputs their values."""
    from igs_amd import _cabi
    step = 0x100000
    x = Rows(5, 128, F32, src=LH.project_inputs(5, 1, DEV).to(F32))
    g = torch.full((3 * step // 4 + 1024,), 0.5, device=DEV)
    dw = torch.full((3 * step // 4 + 1024,), SENTINEL, device=DEV)
    dx = Rows(5, 1024, F32)
    dx.v.fill_(SENTINEL)
    scr = torch.full((GR.scratch_bytes(513, 3) // 4,), SENTINEL, device=DEV)
    wt = _heads(3).packs_t[F32]
    kept = [t.clone() for t in (x.big, g, wt)]
    base = (x.v.data_ptr(), g.data_ptr(), wt.data_ptr(), scr.data_ptr(), dx.v.data_ptr(), dw.data_ptr())
    for kw, word in GR.refusals(*base):
        assert GR.call_abi(_cabi.lib(), _stream(), dict(GR.good_call(*base), **kw)) == E_INVALID, kw
        assert word in _cabi.last_error(), (kw, _cabi.last_error())
    torch.cuda.synchronize()
    assert (dx.big == SENTINEL).all() and (dw == SENTINEL).all() and (scr == SENTINEL).all()
    assert all(torch.equal(a, b) for a, b in zip(kept, (x.big, g, wt)))


# ---------------------------------------------------------------- 4. the Python layer
def _python_case(half, rot, use, stream=None):
    """project_tokens_autograd through .backward() beside F.linear under autograd and float64.  use: per output how often it enters the
    loss (0: unused)."""
    from igs_amd import tokens as TK
    n, T = len(use), 2 * 65
    x64 = LH.project_inputs(T, 31, DEV).view(2, 65, 128)
    w32 = [w.to(DEV) for w in LH.make_weights(n, 8, F32)]
    g64 = [g.view(2, 65, 128) for g in _grads64(T, n, 32)]
    cdt = F16 if half else F32

    def loss(outs):
        return sum(k * (o.double() * g).sum() for o, g, k in zip(outs, g64, use) if k)

    x = x64.float().requires_grad_(True)
    ws = [w.clone().requires_grad_(True) for w in w32]
    with torch.autocast("cuda", dtype=F16, enabled=half):
        if stream is None:
            outs = TK.project_tokens_autograd(x, ws, rot=rot)
            loss(outs).backward()
        else:
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                outs = TK.project_tokens_autograd(x, ws, rot=rot)
                loss(outs).backward()
            torch.cuda.current_stream().wait_stream(stream)
    assert len(outs) == n and all(o.shape == x.shape and o.dtype == cdt for o in outs)
    assert len({o.untyped_storage().data_ptr() for o in outs}) == 1 and all(o.stride(-2) == 128 * n for o in outs), "not slices of one buffer"
    xc = x64.float().requires_grad_(True)
    wc = [w.clone().requires_grad_(True) for w in w32]
    with torch.autocast("cuda", dtype=F16, enabled=half):
        couts = [torch.roll(F.linear(xc, w).view(T, 128), 0 if rot is None else rot[j], 0).view(x.shape) for j, w in enumerate(wc)]
        loss(couts).backward()
    grads = [None if not k else k * g.view(T, 128) for g, k in zip(g64, use)]
    ref_dx, ref_dw = GR.project_grad_restate(x64.view(T, 128), [w.double() for w in w32], grads, rot)
    label = "python half %s rot %s use %s" % (half, rot, use)
    for j, (o, c) in enumerate(zip(outs, couts)):
        GR.four_times(label + ": out %d" % j, o.detach().float(), c.detach().float(),
                      LH.project_restate(x64.view(T, 128), [w.double() for w in w32], rot)[:, 128 * j: 128 * (j + 1)].view(x.shape), cdt)
    assert x.grad.dtype == F32 and x.grad.shape == x.shape
    GR.four_times(label + ": d x", x.grad.view(T, 128), xc.grad.view(T, 128), ref_dx, cdt)
    for j, k in enumerate(use):
        if k:
            assert ws[j].grad.dtype == F32
            GR.four_times(label + ": d W_%d" % j, ws[j].grad, wc[j].grad, ref_dw[j], cdt)
        else:
            assert ws[j].grad is None or not ws[j].grad.any(), (label, j, "an unused output's weight has a gradient")


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16-autocast"])
def test_autograd_with_an_unused_output_and_one_used_twice(half):
    _python_case(half, (0, 1, 65, 129), (1, 0, 2, 1))
    _python_case(half, None, (1,))


def test_autograd_on_a_side_stream():
    _python_case(False, (0, 65), (1, 1), stream=torch.cuda.Stream())


def test_a_frozen_input_gets_no_dx_launch_and_frozen_weights_no_weight_gradients(monkeypatch):
    from igs_amd import _cabi
    from igs_amd import tokens as TK
    proj = _cabi.ext()._proj
    calls = Counter(proj.token_proj_bwd, lambda x, grads, pack_t, rot, want_dx, want_dw, *a: (want_dx, list(want_dw), [g is not None for g in grads]))
    monkeypatch.setattr(proj, "token_proj_bwd", calls)
    x = LH.project_inputs(70, 3, DEV).float()
    ws = [w.to(DEV).requires_grad_(j != 1) for j, w in enumerate(LH.make_weights(3, 2, F32))]
    q, k, v = TK.project_tokens_autograd(x, ws)
    (q.sum() + v.sum()).backward()
    assert calls.seen == [(False, [True, False, True], [True, False, True])], calls.seen
    assert ws[1].grad is None and ws[0].grad is not None
    # an expanded gradient (stride 0) is copied once and read
    assert torch.allclose(ws[0].grad, x.sum(0)[None].expand(128, 128), rtol=1e-4, atol=1e-4)


# ---------------------------------------------------------------- 5. the binders on stand-in transformers, training
H = W = 4
SPLITS = 2                                                           # 2 x 2-token windows: the smallest a shifted call allows; block 1 is shifted


@pytest.fixture
def routed(monkeypatch):
    """The routing constants the binder tests pin: every launch fused, forward and backward, the fused tail whatever the fill."""
    from igs_amd import tokens as TK
    monkeypatch.setattr(TK, "LAYER_HEAD_FUSED", {F32: True, F16: True})
    monkeypatch.setattr(TK, "LAYER_HEAD_MIN_OUTPUTS", {F32: 1, F16: 1})
    monkeypatch.setattr(TK, "LAYER_HEAD_BWD_NATIVE", {F32: True, F16: True})
    monkeypatch.setattr(TK, "LAYER_HEAD_BWD_MIN_OUTPUTS", {F32: 1, F16: 1})
    monkeypatch.setattr(TK, "LAYER_TAIL_FFN_MIN_FILL", {F32: 0.0, F16: 0.0})
    return TK


def _train(model, bidirectional, half, dtype=F32):
    """[out, d feature0, d feature1, every parameter's gradient] of one training step's forward and backward."""
    f0, f1 = (t.to(dtype).requires_grad_(True) for t in LH.feature_inputs(1, H, W, 3, DEV))
    with torch.autocast("cuda", dtype=F16, enabled=half):
        out = model(f0, f1, attn_type="swin", attn_num_splits=SPLITS)
    out = torch.cat(list(out), 0) if bidirectional else out
    out.backward(torch.cos(torch.arange(out.numel(), device=DEV, dtype=F32)).view(out.shape).to(out.dtype))
    return [out.detach(), f0.grad, f1.grad] + [p.grad for p in model.parameters()]


_REFS = {}


def _reference(monkeypatch, bidirectional):
    """The unbound stand-in in float64 with the restated attention, computed once per case and left unchanged."""
    if bidirectional not in _REFS:
        _attention(monkeypatch, False)
        _REFS[bidirectional] = _train(LH.make_transformer(bidirectional).double().to(DEV), bidirectional, False, torch.float64)
    return _REFS[bidirectional]


def _count(monkeypatch):
    from igs_amd import _cabi
    proj = _cabi.ext()._proj
    fwd = Counter(proj.token_proj_fwd, lambda x, pack, n, *a, **k: n)
    bwd = Counter(proj.token_proj_bwd, lambda x, grads, *a, **k: len(grads))
    monkeypatch.setattr(proj, "token_proj_fwd", fwd)
    monkeypatch.setattr(proj, "token_proj_bwd", bwd)
    return fwd, bwd


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16-autocast"])
@pytest.mark.parametrize("bidirectional", [True, False], ids=["two-way", "one-way"])
def test_bound_transformer_trains_against_float64_with_pinned_launches(routed, monkeypatch, bidirectional, half):
    TK = routed
    ref = _reference(monkeypatch, bidirectional)
    _attention(monkeypatch, True)
    today, mine = (LH.make_transformer(bidirectional).to(DEV) for _ in range(2))
    assert TK.use_native_layer_tails(today) == 4 and TK.use_native_feature_transformer(mine, bidirectional, training=True) == 4
    cmp_ = _train(today, bidirectional, half)
    fwd, bwd = _count(monkeypatch)
    got = _train(mine, bidirectional, half)
    # a two-way block: five projections of its input, then the cross layer's q; a one-way block: q, k, v of its input, k, v of feature1, q
    want = ([5, 1] if bidirectional else [3, 2, 1]) * 2
    assert fwd.seen == want, fwd.seen
    assert sorted(bwd.seen) == sorted(want), bwd.seen
    names = ["out", "d feature0", "d feature1"] + ["d " + k for k, _ in mine.named_parameters()]
    cdt = F16 if half else F32
    for name, g, c, r in zip(names, got, cmp_, ref):
        assert g is not None and g.shape == r.shape and g.dtype == c.dtype, name
        GR.four_times("%s %s %s" % ("two-way" if bidirectional else "one-way", str(cdt)[6:], name), g, c, r, cdt)


@pytest.mark.parametrize("bidirectional", [True, False], ids=["two-way", "one-way"])
def test_with_the_constants_off_a_training_call_is_bit_identical_to_todays(routed, monkeypatch, bidirectional):
    TK = routed
    monkeypatch.setattr(TK, "LAYER_HEAD_BWD_NATIVE", {F32: False, F16: False})
    monkeypatch.setattr(TK, "LAYER_TAIL_BWD_NATIVE", {F32: False, F16: False})                   # (so that training=True and the default route the tails alike)
    _attention(monkeypatch, True)
    today, mine = (LH.make_transformer(bidirectional).to(DEV) for _ in range(2))
    TK.use_native_layer_tails(today, training=True)
    TK.use_native_feature_transformer(mine, bidirectional, training=True)
    fwd, bwd = _count(monkeypatch)
    a, b = _train(today, bidirectional, False), _train(mine, bidirectional, False)
    assert fwd.seen == [] and bwd.seen == [], "a call that needs a gradient reached the fused projections"
    for i, (t, m) in enumerate(zip(a, b)):
        assert torch.equal(_bits(m), _bits(t)), (i, "differs from the forward of use_native_layer_tails")
    # the default binding (training=False) ignores LAYER_HEAD_BWD_NATIVE
    monkeypatch.setattr(TK, "LAYER_HEAD_BWD_NATIVE", {F32: True, F16: True})
    TK.use_native_feature_transformer(mine, bidirectional)
    c = _train(mine, bidirectional, False)
    assert fwd.seen == [] and bwd.seen == []
    assert all(torch.equal(_bits(m), _bits(t)) for t, m in zip(a[:3], c[:3]))


def test_a_frozen_feature1_gets_no_dx_launch_in_the_one_way_transformer(routed, monkeypatch):
    from igs_amd import _cabi
    TK = routed
    _attention(monkeypatch, True)
    model = LH.make_transformer(False).to(DEV)
    TK.use_native_feature_transformer(model, False, training=True)
    proj = _cabi.ext()._proj
    calls = Counter(proj.token_proj_bwd, lambda x, grads, pack_t, rot, want_dx, *a: (len(grads), want_dx))
    monkeypatch.setattr(proj, "token_proj_bwd", calls)
    f0, f1 = LH.feature_inputs(1, H, W, 3, DEV)
    model(f0.requires_grad_(True), f1, attn_type="swin", attn_num_splits=SPLITS).sum().backward()
    assert sorted(calls.seen) == sorted([(3, True), (2, False), (1, True)] * 2), calls.seen
