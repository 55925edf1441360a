"""Edge gates on bf16 feature rows (MI355X): the six mgcn_gate_*_bf16 entries
and everything mgcn.ops / mgcn.models route to them.

The yardstick of every case is the fp32 op -- held to the reference's fp64
fixtures by the other edge-gate tests -- run in the same process on
``Hx.float()`` / ``dY.float()``.  The contract is bitwise: fp32 outputs (gates,
dl, dc, da, dw, argmax, the gradients of the gate vectors, t and bias) are
``torch.equal``; bf16 outputs (Y, dHx) have the bit patterns of the fp32 result
rounded once (``.cpu().to(torch.bfloat16)``, compared as ``int16``).  No
tolerance anywhere.

Graphs: edge_gate_ref.ladder_graph (a row of every in- and out-degree
0 .. 130, isolated rows, parallel edges) for the wave kernels, and a hub
ladder (one row of every degree around the heavy and the giant thresholds, in
both views) for the workgroup path."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from edge_gate_ref import MODEL_ARGS, ladder_graph, small_graph

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
HUB_DEGREES = (127, 128, 129, 191, 192, 193, 511, 512, 513, 1000, 2100)
POOL = 128
WAVE_BF16 = {"gate_fwd_bf16", "gate_bwd_dst_bf16", "gate_bwd_src_bf16"}
HEAVY_BF16 = {"gate_fwd_heavy_bf16", "gate_bwd_dst_heavy_bf16", "gate_bwd_src_heavy_bf16"}
# launches that read or write fp32 feature rows
FP32_ROW_LAUNCHES = {"att_scores", "gate_fwd", "gate_bwd_dst", "gate_bwd_src", "gate_fwd_heavy",
                     "gate_bwd_dst_heavy", "gate_bwd_src_heavy"}


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def same_bits(got, want32):
    """got (bf16, device) against the fp32 path's result rounded once."""
    assert got.dtype == BF16 and want32.dtype == torch.float32
    return torch.equal(bits(got), bits(want32.detach().cpu().to(BF16)))


@functools.lru_cache(maxsize=None)
def ladder():
    from mgcn.graph import plan_for
    ei, N = ladder_graph()
    eig = ei.cuda()
    return eig, N, plan_for(eig, N)


@functools.lru_cache(maxsize=None)
def hub_ladder():
    """test_gpu_edge_gate_heavy.py's hub ladder: 128 pool nodes with 400 random
    edges among themselves, one node of every in-degree and one of every
    out-degree in HUB_DEGREES (other endpoints drawn with replacement from the
    pool: parallel edges occur), 3 isolated nodes, shuffled COO order."""
    from mgcn.graph import plan_for
    rng = np.random.default_rng(71)
    nd = len(HUB_DEGREES)
    N = POOL + 2 * nd + 3
    parts = [rng.integers(0, POOL, (2, 400))]
    for i, d in enumerate(HUB_DEGREES):
        parts.append(np.stack([rng.integers(0, POOL, d), np.full(d, POOL + i)]))
        parts.append(np.stack([np.full(d, POOL + nd + i), rng.integers(0, POOL, d)]))
    ei = np.concatenate(parts, axis=1)
    ei = ei[:, rng.permutation(ei.shape[1])]
    ind, outd = np.bincount(ei[1], minlength=N), np.bincount(ei[0], minlength=N)
    assert tuple(ind[POOL:POOL + nd]) == HUB_DEGREES
    assert tuple(outd[POOL + nd:POOL + 2 * nd]) == HUB_DEGREES
    eig = torch.from_numpy(ei.astype(np.int64)).cuda()
    plan = plan_for(eig, N)
    for view in (plan.fwd, plan.bwd):  # 129 .. 2100 heavy, 513 / 1000 / 2100 giant
        assert view.order is not None and (view.n_heavy, view.n_giant) == (9, 3)
    return eig, N, plan


@contextlib.contextmanager
def route(on, names):
    """The heavy-row switch set to ``on``, every launch's timer name recorded."""
    from mgcn import _call, ops
    before = ops.gate_heavy_rows()
    ops.set_gate_heavy_rows(on)
    _call.set_kernel_timer(lambda name, start, rows=None, edges=None:
                           names.append(name) if start else None)
    try:
        yield
    finally:
        _call.set_kernel_timer(None)
        ops.set_gate_heavy_rows(before)


def gate_names(names):
    return {n for n in names if n.startswith("gate_")}


def layer_inputs(graph, dn, gate, epi, C, seed):
    """bf16-representable Hx, dY; fp32 gate vectors, t, bias and dG."""
    _, N, plan = graph
    E = plan.nnz
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    x = {"Hx": rnd(N, C).to(BF16).cuda(), "dY": rnd(N, C).to(BF16).cuda(), "dG": rnd(E).cuda()}
    if gate in ("proj", "proj_edge"):
        x["w_src"], x["w_dst"] = (rnd(C) * 0.3).cuda(), (rnd(C) * 0.3).cuda()
    if gate == "proj":
        x["t"] = rnd(1).cuda()
    elif gate in ("proj_edge", "free"):
        x["t"] = rnd(E).cuda()
    if epi:
        x["bias"] = (rnd(C) * 0.5).cuda()
    return x, plan.norm(dn)


def layer(graph, aggr, dn, gate, epi, C, dg_in, seed, rows):
    """One gate_aggregate forward + backward with ``rows`` (fp32: on the
    upcast Hx and dY); every tensor it produces, by name."""
    from mgcn.ops import gate_aggregate
    x, norm = layer_inputs(graph, dn, gate, epi, C, seed)
    plan = graph[2]
    leaves = {k: x[k].detach().clone().requires_grad_(True)
              for k in ("w_src", "w_dst", "t", "bias") if k in x}
    leaves["Hx"] = x["Hx"].to(rows).requires_grad_(True)
    Y, g = gate_aggregate(leaves["Hx"], plan, norm, aggr, leaves.get("w_src"),
                          leaves.get("w_dst"), leaves.get("t"), leaves.get("bias"), relu=epi)
    assert Y.dtype == rows and g.dtype == torch.float32
    if dg_in:
        torch.autograd.backward([Y, g], [x["dY"].to(rows), x["dG"]])
    else:
        Y.backward(x["dY"].to(rows))
    out = {"Y": Y.detach(), "g_coo": g.detach()}
    for k, v in leaves.items():
        assert v.grad is not None, k
        out["d_" + k] = v.grad
    torch.cuda.synchronize()
    return out


def assert_rounded_fp32(got, r32, tag):
    """bf16 outputs: the fp32 ones rounded once; fp32 outputs: equal."""
    assert got.keys() == r32.keys()
    for k, v in got.items():
        assert not torch.isnan(v.float()).any(), f"{tag}: {k} has NaN"
        if k in ("Y", "d_Hx"):
            assert r32[k].dtype == torch.float32
            assert same_bits(v, r32[k]), f"{tag}: {k} is not the rounded fp32 result"
        else:
            assert v.dtype == torch.float32, f"{tag}: {k} is {v.dtype}"
            assert torch.equal(v, r32[k]), f"{tag}: {k} differs from the fp32 path"


# ------------------------------------------------------ 1. layer bits, wave path
# (aggr, norm, gate, bias + ReLU, C, a gradient into g_coo): every width of
# test_gpu_edge_gate_shapes.WIDTHS (each FPL instantiation, both sides of each
# 64-lane boundary) under sum or mean and under max; the gate's terms on / off
# (proj: a, c and a scalar t; proj_edge: a, c and t [E]; free: t [E] alone);
# per-slot weights ('sm'), the row post-scale ('rw') and neither; the mean's
# cnt with and without the rank-one terms; the epilogue on / off.
WAVE_CASES = [
    ("add", "sm", "proj", True, 32, False),
    ("mean", None, "proj", False, 32, False),
    ("max", None, "proj", True, 32, True),
    ("add", "rw", "proj_edge", True, 33, False),
    ("max", "sm", "proj", True, 33, False),
    ("mean", "sm", "free", True, 33, True),
    ("add", "sm", "free", False, 7, False),
    ("mean", "rw", "proj_edge", False, 7, True),
    ("max", "rw", "free", False, 1, False),
    ("mean", None, "free", True, 1, False),
    ("add", None, "proj", True, 64, False),
    ("mean", "rw", "proj", True, 64, True),
    ("max", "sm", "proj_edge", False, 64, False),
    ("add", "sm", "proj", True, 65, False),
    ("max", None, "proj", False, 65, True),
    ("mean", "sm", "proj_edge", True, 129, False),
    ("max", "rw", "proj", True, 129, False),
    ("add", None, "proj", False, 257, True),
    ("max", None, "proj_edge", True, 257, False),
    ("add", "rw", "proj", False, 513, False),
    ("mean", "sm", "proj", True, 513, False),
    ("max", "sm", "proj", True, 513, True),
    ("mean", "sm", "proj", True, 1024, False),
    ("add", None, "proj_edge", True, 1024, True),
    ("max", "rw", "proj", False, 1024, False),
]


@pytest.mark.parametrize("case", WAVE_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_layer_bits_wave_path(cuda, case):
    """gate_aggregate forward + backward on the degree ladder, one wave per
    row for every row: bf16 rows against the fp32 op on the upcast rows."""
    seed = 100 + WAVE_CASES.index(case)
    names = []
    with route(False, names):
        got = layer(ladder(), *case, seed=seed, rows=BF16)
    assert gate_names(names) == WAVE_BF16 and not set(names) & FP32_ROW_LAUNCHES, names
    with route(False, []):
        r32 = layer(ladder(), *case, seed=seed, rows=torch.float32)
    assert_rounded_fp32(got, r32, "wave")
    if case[2] != "free":
        assert got["g_coo"].unique().numel() > 100
    _, N, plan = ladder()
    no_in = (plan.in_cnt == 1) & (plan.fwd.rowptr[1:] == plan.fwd.rowptr[:-1])
    if not case[3]:
        assert not bits(got["Y"][no_in]).any(), "Y of a row without in-edges"


# ------------------------------------------------------------- 2. heavy rows
# the three reductions at the issue's widths (C = 32: 8-byte gathers in the
# heavy-row body; 33 and 129: single elements, one and two feature chunks) and
# C = 34 (4-byte gathers); heavy rows in the fwd view (forward, adjoint by
# destination) and in the bwd view (adjoint by source) of the hub ladder
HEAVY_CASES = [
    ("add", "sm", "proj", True, 32, False),
    ("mean", None, "proj", True, 32, True),
    ("max", None, "proj", True, 32, False),
    ("add", "rw", "proj_edge", False, 33, True),
    ("mean", "sm", "proj", True, 33, False),
    ("max", "sm", "free", False, 33, False),
    ("add", None, "proj", True, 129, False),
    ("mean", "rw", "proj_edge", True, 129, False),
    ("max", "rw", "proj", True, 129, True),
    ("mean", "sm", "proj", False, 34, False),
    ("add", "rw", "free", True, 34, False),
]


@pytest.mark.parametrize("case", HEAVY_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_heavy_rows_bits_and_timer_names(cuda, case):
    """With the heavy-row switch on, the bits equal those with it off and the
    rounded fp32 path; the timer names are the ``_heavy_bf16`` ones when on
    and the plain ``_bf16`` ones when off."""
    seed = 200 + HEAVY_CASES.index(case)
    runs = {}
    for on in (True, False):
        names = []
        with route(on, names):
            runs[on] = layer(hub_ladder(), *case, seed=seed, rows=BF16)
        assert gate_names(names) == (HEAVY_BF16 if on else WAVE_BF16), names
        assert not set(names) & FP32_ROW_LAUNCHES, names
    for k, v in runs[True].items():
        off = runs[False][k]
        assert v.dtype == off.dtype
        if v.dtype == BF16:
            v, off = bits(v), bits(off)
        assert torch.equal(v, off), f"{k}: the heavy route changed bits"
    with route(True, []):
        r32 = layer(hub_ladder(), *case, seed=seed, rows=torch.float32)
    assert_rounded_fp32(runs[True], r32, "heavy")


# ------------------------------------------------------------------ 3. C ABI
PAD = 67  # guard elements on either side of a flat array
R0 = 77   # the row ranges [0, R0) and [R0, N) of the entries without a schedule


class Bufs:
    """Outputs in sentinel-filled buffers whose untouched part is checked."""

    def __init__(self, cuda):
        self.cuda = cuda
        self.all = []  # (buffer, mask of the guard elements, sentinel)

    def banded(self, n, dtype=torch.float32):
        fill = -7 if dtype == torch.int32 else float("nan")
        buf = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=self.cuda)
        m = torch.ones(n + 2 * PAD, dtype=torch.bool, device=self.cuda)
        m[PAD:PAD + n] = False
        self.all.append((buf, m, fill))
        return buf[PAD:PAD + n]

    def window(self, N, C, ld, off, dtype, src=None):
        """[N, C] at column ``off`` of rows 1 .. N of a NaN-filled [N + 2, ld]."""
        buf = torch.full((N + 2, ld), float("nan"), dtype=dtype, device=self.cuda)
        m = torch.ones(N + 2, ld, dtype=torch.bool, device=self.cuda)
        m[1:N + 1, off:off + C] = False
        self.all.append((buf, m, float("nan")))
        win = buf[1:N + 1, off:off + C]
        if src is not None:
            win.copy_(src)
        return win

    def intact(self):
        for buf, m, fill in self.all:
            v = buf[m]
            if not bool((torch.isnan(v) if fill != fill else v == fill).all()):
                return False
        return True


@functools.lru_cache(maxsize=None)
def abi_inputs(C):
    _, N, plan = hub_ladder()
    nnz = plan.nnz
    gen = torch.Generator().manual_seed(8)
    rnd = lambda *s: torch.randn(*s, generator=gen).cuda()  # noqa: E731
    return dict(a=rnd(N) * 0.3, c=rnd(N) * 0.3, t=rnd(nnz), w=rnd(nnz).abs() + 0.5,
                wt=rnd(nnz).abs() + 0.5, bias=rnd(C), wsd=rnd(2 * C), rs=rnd(N), dgi=rnd(nnz),
                Hx=rnd(N, C).to(BF16), dY=rnd(N, C).to(BF16))


def abi_run(cuda, reduce, C, rows, mode, full):
    """The three launches through ctypes.  rows fp32: the reference entries on
    the upcast Hx and on dY.float() (mean: pre-divided by the row counts);
    rows bf16, mode 'range': the entries without a schedule over two row
    ranges, 'sched': the _sched entries; both on windows with padded leading
    dimensions at an odd element offset and with guard bands.  ``full``: every
    nullable argument present, else absent.  Returns (outputs, Bufs)."""
    import mgcn
    from mgcn import _lib as L
    from mgcn.ops import max_mask
    lib = mgcn.load()
    _, N, plan = hub_ladder()
    fwd, bwd, nnz = plan.fwd, plan.bwd, plan.nnz
    slot, st = plan.slot_map(), L.stream_of(cuda)
    x = abi_inputs(C)
    opt = (lambda k: x[k]) if full else (lambda k: None)
    bf = rows == BF16
    B = Bufs(cuda)
    mean = reduce == 1
    if bf:
        hx = B.window(N, C, C + 3, 3, BF16, x["Hx"])       # odd offset, odd row pitch
        dy = B.window(N, C, C + 7, 5, BF16, x["dY"])
        Y, dHx = B.window(N, C, C + 7, 1, BF16), B.window(N, C, C + 4, 2, BF16)
        assert hx.data_ptr() % 4 == 2 and dHx.data_ptr() % 4 == 2
        cnt = plan.in_cnt if mean else None
    else:
        hx = x["Hx"].float()
        dy = x["dY"].float() / plan.in_cnt[:, None] if mean else x["dY"].float()
        Y = torch.full((N, C), float("nan"), device=cuda)
        dHx = torch.full((N, C), float("nan"), device=cuda)
    g, dl, coef_f, coef_b = (B.banded(nnz) for _ in range(4))
    dw = B.banded(nnz) if full else None
    dc, da = (B.banded(N), B.banded(N)) if full else (None, None)
    am = B.banded(N * C, torch.int32).view(N, C)
    sfx = ("_sched" if mode == "sched" else "") + ("_bf16" if bf else "")
    ranges = [(0, N)] if mode == "sched" or not bf else [(0, R0), (R0, N)]

    def tail(view, coef):
        if mode != "sched":
            return ()
        t = (L.ptr(view.order), view.n_heavy, view.n_giant)
        return t if coef is None else t + (L.ptr(coef),)

    def adv(t, r0):  # a row-indexed array advanced to the range
        return None if t is None else L.ptr(t[r0:])

    for r0, r1 in ranges:
        rc = getattr(lib, "mgcn_gate_fwd" + sfx)(
            r1 - r0, nnz, C, adv(fwd.rowptr, r0), L.ptr(fwd.col), L.ptr(fwd.eid), L.ptr(opt("a")),
            adv(opt("c"), r0), L.ptr(opt("t")), 0, L.ptr(opt("w")), L.ptr(hx), hx.stride(0),
            reduce, L.ptr(opt("bias")), int(full), adv(Y, r0), Y.stride(0), L.ptr(g),
            adv(am, r0), *tail(fwd, coef_f), st)
        assert rc == 0, lib.mgcn_last_error()
    win = max_mask(plan, am.clone()) if reduce == 2 else None
    for r0, r1 in ranges:
        rc = getattr(lib, "mgcn_gate_bwd_dst" + sfx)(
            r1 - r0, nnz, C, adv(fwd.rowptr, r0), L.ptr(fwd.col), L.ptr(hx), hx.stride(0),
            adv(dy, r0), dy.stride(0), L.ptr(opt("w")), L.ptr(g), L.ptr(win), L.ptr(opt("dgi")),
            L.ptr(dl), adv(dc, r0), L.ptr(dw), *((adv(cnt, r0),) if bf else ()),
            *tail(fwd, None), st)
        assert rc == 0, lib.mgcn_last_error()
    for r0, r1 in ranges:
        rc = getattr(lib, "mgcn_gate_bwd_src" + sfx)(
            r1 - r0, nnz, C, adv(bwd.rowptr, r0), L.ptr(bwd.col), L.ptr(slot), L.ptr(dy),
            dy.stride(0), L.ptr(opt("wt")), adv(opt("rs"), r0), L.ptr(g), L.ptr(dl), L.ptr(win),
            L.ptr(opt("wsd")), adv(dc, r0), adv(da, r0), adv(dHx, r0), dHx.stride(0),
            *((L.ptr(cnt),) if bf else ()), *tail(bwd, coef_b), st)
        assert rc == 0, lib.mgcn_last_error()
    torch.cuda.synchronize()
    out = {"Y": Y, "g": g, "dl": dl, "dHx": dHx}
    if full:
        out.update(dw=dw, dc=dc, da=da)
    if reduce == 2:
        out["argmax"] = am
    return {k: v.clone() for k, v in out.items()}, B


@pytest.mark.parametrize("full", [True, False], ids=["all-args", "nullable-absent"])
@pytest.mark.parametrize("reduce", [0, 1, 2], ids=["sum", "mean", "max"])
def test_c_abi_entries(cuda, reduce, full):
    """Each of the six entries through ctypes against the fp32 entries: padded
    leading dimensions, an odd element offset, row ranges (rowptr + r0) for
    the entries without a schedule, the schedule for the others, ``cnt``
    against pre-divided fp32 rows, every guard element intact."""
    C = 37
    ref, _ = abi_run(cuda, reduce, C, torch.float32, "plain", full)
    for k, v in ref.items():
        assert not (torch.isnan(v).any() if v.is_floating_point() else (v == -7).any()), k
    for mode in ("range", "sched"):
        got, B = abi_run(cuda, reduce, C, BF16, mode, full)
        assert got.keys() == ref.keys()
        for k, v in got.items():
            if k in ("Y", "dHx"):
                assert same_bits(v, ref[k]), f"{mode}: {k}"
            else:
                assert torch.equal(v, ref[k]), f"{mode}: {k}"
        assert B.intact(), f"{mode}: a guard element was written"


def test_c_abi_no_op_and_einval_leave_outputs_untouched(cuda):
    """n_rows == 0 is a successful no-op; an out-of-range C and n_giant >
    n_heavy return MGCN_EINVAL; no output element is written either way."""
    import mgcn
    from mgcn import _lib as L
    lib = mgcn.load()
    _, N, plan = hub_ladder()
    fwd, bwd, nnz = plan.fwd, plan.bwd, plan.nnz
    C = 8
    st = L.stream_of(cuda)
    x = abi_inputs(C)
    slot = plan.slot_map()
    nan32 = lambda *s: torch.full(s, float("nan"), device=cuda)  # noqa: E731
    Y, dHx = nan32(N, C).to(BF16), nan32(N, C).to(BF16)
    g, dl, dc, da, dw, coef = nan32(nnz), nan32(nnz), nan32(N), nan32(N), nan32(nnz), nan32(nnz)
    am = torch.full((N, C), -7, dtype=torch.int32, device=cuda)

    def calls(n, C_, n_heavy, n_giant, sched_only=False):
        """Return codes of the six entries (``sched_only``: of the three with
        a schedule); every array has the size a launch would need."""
        f = (n, nnz, C_, L.ptr(fwd.rowptr), L.ptr(fwd.col), L.ptr(fwd.eid), L.ptr(x["a"]),
             L.ptr(x["c"]), L.ptr(x["t"]), 0, L.ptr(x["w"]), L.ptr(x["Hx"]), C, 2,
             L.ptr(x["bias"]), 1, L.ptr(Y), C, L.ptr(g), L.ptr(am))
        d = (n, nnz, C_, L.ptr(fwd.rowptr), L.ptr(fwd.col), L.ptr(x["Hx"]), C, L.ptr(x["dY"]), C,
             L.ptr(x["w"]), L.ptr(x["t"]), None, L.ptr(x["dgi"]), L.ptr(dl), L.ptr(dc), L.ptr(dw),
             L.ptr(plan.in_cnt))
        s = (n, nnz, C_, L.ptr(bwd.rowptr), L.ptr(bwd.col), L.ptr(slot), L.ptr(x["dY"]), C,
             L.ptr(x["wt"]), L.ptr(x["rs"]), L.ptr(x["w"]), L.ptr(x["t"]), None, L.ptr(x["wsd"]),
             L.ptr(x["c"]), L.ptr(da), L.ptr(dHx), C, L.ptr(plan.in_cnt))
        sf = (L.ptr(fwd.order), n_heavy, n_giant)
        sb = (L.ptr(bwd.order), n_heavy, n_giant)
        rcs = [] if sched_only else [lib.mgcn_gate_fwd_bf16(*f, st),
                                     lib.mgcn_gate_bwd_dst_bf16(*d, st),
                                     lib.mgcn_gate_bwd_src_bf16(*s, st)]
        return rcs + [lib.mgcn_gate_fwd_sched_bf16(*f, *sf, L.ptr(coef), st),
                      lib.mgcn_gate_bwd_dst_sched_bf16(*d, *sf, st),
                      lib.mgcn_gate_bwd_src_sched_bf16(*s, *sb, L.ptr(coef), st)]

    assert calls(0, C, 0, 0) == [0] * 6           # n_rows == 0: a no-op
    assert calls(N, 1025, 9, 3) == [1] * 6        # MGCN_EINVAL: C out of range
    assert calls(N, 0, 9, 3) == [1] * 6
    assert calls(N, C, 3, 9, sched_only=True) == [1] * 3  # MGCN_EINVAL: n_giant > n_heavy
    assert b"n_giant <= n_heavy" in lib.mgcn_last_error()
    torch.cuda.synchronize()
    for t in (Y, dHx, g, dl, dc, da, dw, coef):
        assert bool(torch.isnan(t.float()).all())
    assert bool((am == -7).all())


# ---------------------------------------------------------------- 4. routing
def _routed(cuda, rows, wgrad=False, epi=True, aggr="max"):
    from mgcn.graph import plan_for
    from mgcn.ops import gate_aggregate
    ei, N = small_graph(9, 70, 400)
    ei = ei.to(cuda)
    plan = plan_for(ei, N)
    gen = torch.Generator().manual_seed(2)
    hx = torch.randn(N, 32, generator=gen).to(rows).to(cuda).requires_grad_(True)
    ws, wd, b = (torch.randn(32, generator=gen).to(cuda).requires_grad_(True) for _ in range(3))
    ew = None
    if wgrad:
        ew = (torch.rand(plan.nnz, generator=gen) + 0.5).to(cuda).requires_grad_(True)
    norm = plan.norm("sm", edge_weight=ew)
    assert norm.grad is wgrad
    names = []
    with route(True, names):
        y, _ = gate_aggregate(hx, plan, norm, aggr, ws, wd, None, b if epi else None, relu=epi)
        y.float().sum().backward()
    torch.cuda.synchronize()
    assert y.dtype == rows and hx.grad.dtype == rows
    return names


def test_routing_by_row_dtype(cuda):
    """fp32 rows record exactly the fp32 route's timer names; bf16 rows only
    ``_bf16`` row launches (the column sums of a bias gradient and the gate
    vectors' mgcn_gemm_tn run on fp32 temporaries); a norm with ``grad`` keeps
    the fp32 launches for bf16 rows; float16 raises TypeError."""
    from mgcn.graph import plan_for
    from mgcn.ops import gate_aggregate
    assert _routed(cuda, torch.float32) == ["att_scores", "gate_fwd", "relu_bwd_colsum",
                                           "gate_bwd_dst", "gate_bwd_src", "gemm_tn"]
    assert _routed(cuda, BF16) == ["att_scores_bf16", "gate_fwd_bf16", "relu_bwd_colsum_bf16",
                                  "relu_bwd_colsum", "gate_bwd_dst_bf16", "gate_bwd_src_bf16",
                                  "gemm_tn"]
    assert _routed(cuda, BF16, epi=False, aggr="mean") == [
        "att_scores_bf16", "gate_fwd_bf16", "gate_bwd_dst_bf16", "gate_bwd_src_bf16", "gemm_tn"]
    names = _routed(cuda, BF16, wgrad=True, aggr="add")
    assert gate_names(names) == {"gate_fwd", "gate_bwd_dst", "gate_bwd_src"}
    assert "att_scores" in names and not [n for n in names if n.endswith("_bf16")]
    ei, N = small_graph(9, 70, 400)
    plan = plan_for(ei.to(cuda), N)
    for dt in (torch.float16, torch.float64):
        with pytest.raises(TypeError, match="float32 or bfloat16"):
            gate_aggregate(torch.zeros(N, 8, device=cuda, dtype=dt), plan, plan.norm(None))


# ---------------------------------------------------------------- 5. modules
def _node_model(cuda, aggr):
    """A gated 32 -> 32 node model whose parameters are bf16-representable and
    whose weight_node is the identity: x @ W is x exactly in either dtype, so
    the layer's output and input gradient are bitwise comparable."""
    from mgcn.models import NodeModelGatedAdditive
    torch.manual_seed(5)
    nm = NodeModelGatedAdditive(32, 32, deg_norm="sm", edge_gate="proj", aggr=aggr, bias=True)
    with torch.no_grad():
        nm.weight_node.copy_(torch.eye(32))
        nm.bias.uniform_(-0.5, 0.5)
        for p in nm.edge_gate.parameters():
            p.uniform_(-0.5, 0.5)
        for p in nm.parameters():
            p.copy_(p.to(BF16).float())
    return nm.to(cuda)


@pytest.mark.parametrize("aggr", ["add", "mean", "max"])
@pytest.mark.parametrize("converted", [False, True], ids=["fp32-masters", "converted"])
def test_node_model_on_bf16_input(cuda, converted, aggr):
    """NodeModelGatedAdditive on bf16 input, with fp32 master parameters and
    after ``.to(torch.bfloat16)``: bf16 output, gradients in the parameters'
    dtype, output and input gradient the fp32 layer's rounded once."""
    ei, N, _ = ladder()
    gen = torch.Generator().manual_seed(6)
    x = torch.randn(N, 32, generator=gen).to(BF16).to(cuda)
    dY = torch.randn(N, 32, generator=gen).to(BF16).to(cuda)
    ref = _node_model(cuda, aggr)
    x32 = x.float().requires_grad_(True)
    store32 = []
    y32 = ref.forward_fused(x32, ei, relu=True, gate_store=store32)
    y32.backward(dY.float())
    nm = _node_model(cuda, aggr)
    if converted:
        nm = nm.to(BF16)
    want = BF16 if converted else torch.float32
    assert all(p.dtype == want for p in nm.parameters())
    xb = x.clone().requires_grad_(True)
    store, names = [], []
    with route(True, names):
        y = nm.forward_fused(xb, ei, relu=True, gate_store=store)
        y.backward(dY)
    torch.cuda.synchronize()
    assert y.dtype == BF16 and xb.grad.dtype == BF16
    assert gate_names(names) <= WAVE_BF16 | HEAVY_BF16 and not set(names) & FP32_ROW_LAUNCHES
    assert same_bits(y, y32), "y"
    assert same_bits(xb.grad, x32.grad), "dx"
    assert store[0].dtype == torch.float32 and not store[0].requires_grad
    assert torch.equal(store[0], store32[0])
    for (k, p), (_, p32) in zip(nm.named_parameters(), ref.named_parameters()):
        assert p.grad is not None and p.grad.dtype == want, k
        assert torch.isfinite(p.grad.float()).all(), k
        if k != "weight_node":  # (its gradient is a bf16 GEMM under bf16 rows)
            if converted:
                assert torch.equal(bits(p.grad), bits(p32.grad.to(BF16))), k
            else:
                assert torch.equal(p.grad, p32.grad), k


@pytest.mark.parametrize("converted", [False, True], ids=["fp32-masters", "converted"])
def test_gated_model_trains_on_bf16_input(cuda, converted):
    """The 6-layer gated GCNModel of the botnet runs on bf16 input: one
    training step runs and stays finite (layers compound roundings: no bit
    claim)."""
    from mgcn.models import GCNModel
    ei, N, _ = ladder()
    torch.manual_seed(3)
    m = GCNModel(**MODEL_ARGS).to(cuda)
    if converted:
        m = m.to(BF16)
    want = BF16 if converted else torch.float32
    opt = torch.optim.SGD(m.parameters(), lr=0.01)
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(N, 1, generator=gen).to(BF16).to(cuda)
    target = torch.randint(0, 2, (N,), generator=gen).to(cuda)
    names = []
    with route(True, names):
        out = m(x, ei)
        assert out.dtype == BF16 and out.shape == (N, 2)
        loss = torch.nn.functional.cross_entropy(out.float(), target)
        loss.backward()
    assert gate_names(names) <= WAVE_BF16 | HEAVY_BF16 and len(gate_names(names)) >= 3
    assert not set(names) & FP32_ROW_LAUNCHES, names
    for k, p in m.named_parameters():
        assert p.grad is not None and p.grad.dtype == want, k
        assert torch.isfinite(p.grad.float()).all(), k
    opt.step()
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and all(torch.isfinite(p.float()).all() for p in m.parameters())
