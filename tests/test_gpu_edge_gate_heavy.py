"""The heavy-row route of the edge gates on the MI355X (mgcn_gate_*_sched,
csrc/edge_gate_heavy.hip): every tensor a gated layer produces has, with the
route on, the bits the wave-per-row kernels give it (``torch.equal``: no
tolerance), on a graph with one row of every degree around the heavy (128) and
the giant (512) thresholds in both views; plus the restatement's bound (a
route wrong in the same way on and off), the C ABI with leading dimensions
and guard bands, a gated GCNModel, and a graph without heavy rows."""
import contextlib

import numpy as np
import pytest
import torch

from edge_gate_ref import (PARAM_KEYS, check, make_node_model, params_of, ref_run, small_graph)

pytestmark = pytest.mark.gpu

DEGREES = (127, 128, 129, 191, 192, 193, 511, 512, 513, 1000, 2100)
POOL = 128
HEAVY_NAMES = {"gate_fwd_heavy", "gate_bwd_dst_heavy", "gate_bwd_src_heavy"}
WAVE_NAMES = {"gate_fwd", "gate_bwd_dst", "gate_bwd_src"}
_HUB = {}


def hub_ladder(cuda):
    """(edge_index on the GPU, N, plan): 128 pool nodes with 400 random edges
    among themselves, one node of every in-degree and one of every out-degree
    in DEGREES (the other endpoints drawn with replacement from the pool:
    parallel edges occur), 3 isolated nodes, shuffled COO order."""
    if "g" not in _HUB:
        from mgcn.graph import plan_for
        rng = np.random.default_rng(71)
        nd = len(DEGREES)
        N = POOL + 2 * nd + 3
        parts = [rng.integers(0, POOL, (2, 400))]
        for i, d in enumerate(DEGREES):
            parts.append(np.stack([rng.integers(0, POOL, d), np.full(d, POOL + i)]))
            parts.append(np.stack([np.full(d, POOL + nd + i), rng.integers(0, POOL, d)]))
        ei = np.concatenate(parts, axis=1)
        ei = ei[:, rng.permutation(ei.shape[1])]
        ind, outd = np.bincount(ei[1], minlength=N), np.bincount(ei[0], minlength=N)
        assert tuple(ind[POOL:POOL + nd]) == DEGREES and not outd[POOL:POOL + nd].any()
        assert tuple(outd[POOL + nd:POOL + 2 * nd]) == DEGREES and not ind[POOL + nd:N].any()
        assert ind[:POOL].max() < 128 and outd[:POOL].max() < 128
        assert not ind[N - 3:].any() and not outd[N - 3:].any()
        pairs = ei[0] * N + ei[1]
        assert len(np.unique(pairs)) < pairs.size  # parallel edges: ties under max
        eig = torch.from_numpy(ei.astype(np.int64)).to(cuda)
        plan = plan_for(eig, N)
        for view in (plan.fwd, plan.bwd):  # 129 .. 2100 heavy, 513 / 1000 / 2100 giant
            assert view.order is not None and (view.n_heavy, view.n_giant) == (9, 3)
        _HUB["g"] = (eig, N, plan)
    return _HUB["g"]


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


def layer(cuda, aggr, dn, gate, epi, C, dg_in=False, wgrad=False, seed=0):
    """One gate_aggregate forward + backward on the hub ladder; every tensor it
    produces, by name."""
    from mgcn.ops import gate_aggregate
    ei, N, plan = hub_ladder(cuda)
    E = plan.nnz
    gen = torch.Generator().manual_seed(1000 + seed)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(cuda)  # noqa: E731
    leaves = {"Hx": rnd(N, C).requires_grad_(True)}
    if gate in ("proj", "proj_edge"):
        leaves["w_src"] = (rnd(C) * 0.3).requires_grad_(True)
        leaves["w_dst"] = (rnd(C) * 0.3).requires_grad_(True)
    if gate == "proj":
        leaves["t"] = rnd(1).requires_grad_(True)
    elif gate in ("proj_edge", "free"):
        leaves["t"] = rnd(E).requires_grad_(True)
    if epi:
        leaves["bias"] = rnd(C).requires_grad_(True)
    ew = deg = None
    if dn == "sm+ew":
        ew = (torch.rand(E, generator=gen) + 0.5).to(cuda)
        if wgrad:
            leaves["edge_weight"] = ew.requires_grad_(True)
    elif wgrad:
        assert dn == "rw"
        deg = (plan.bwd.rowptr[1:] - plan.bwd.rowptr[:-1]).float() + 1.0
        leaves["deg"] = deg.requires_grad_(True)
    norm = plan.norm("sm" if dn == "sm+ew" else dn, deg=deg, edge_weight=ew)
    assert norm.grad is wgrad
    dY, dG = rnd(N, C), rnd(E)
    Y, g = gate_aggregate(leaves["Hx"], plan, norm, aggr, leaves.get("w_src"),
                          leaves.get("w_dst"), leaves.get("t"), leaves.get("bias"), relu=epi)
    loss = (Y * dY).sum()
    if dg_in:
        loss = loss + (g * dG).sum()
    loss.backward()
    out = {"Y": Y.detach(), "g_coo": g.detach()}
    for k, v in leaves.items():
        assert v.grad is not None, k
        out["d_" + k] = v.grad
    torch.cuda.synchronize()
    return out


# (aggr, norm, gate, bias + ReLU, C[, dg_in, wgrad]): the product of the
# issue's grid pruned to the combinations that reach distinct code --
#   forward: sum / mean epilogue / max x (a, c) on / off x t scalar / [E] / none
#            x w on / off x bias + ReLU on / off;
#   the heavy-row body's vector width 4 / 2 / 1 (C = 32 / 130 / 1, 3, 33, 257),
#   one and several feature chunks (C <= 128, C = 130: a 2-wide second chunk,
#   C = 257: three chunks), one and two fold waves (C <= 64, C > 64);
#   adjoints: every count of lane registers of the chunk kernel (1, 2, 4, 8, 16:
#   C <= 64, 96, 130, 257, 520), max's winner words (one: C <= 32, two: 33,
#   several: 130, 257, 520), a partly filled lane register (C = 1, 3, 33, 130,
#   257, 520), dw, dg_in, da / dc on / off, per-slot weights in the bwd view
#   ('sm', edge weights) and the 'rw' row post-scale.
CASES = [
    ("add", "sm", "proj", True, 32),
    ("mean", None, "proj", False, 32),
    ("max", None, "proj", True, 32),
    ("add", "rw", "proj_edge", True, 33),
    ("add", "sm+ew", "free", False, 3),
    ("max", "sm", "proj", True, 33),
    ("max", "rw", "free", False, 1),
    ("max", "sm+ew", "none", False, 130),
    ("add", None, "none", False, 1),
    ("mean", "sm+ew", "proj_edge", True, 130),
    ("add", "sm", "proj", False, 257),
    ("max", None, "proj_edge", True, 257),
    ("mean", "rw", "proj", False, 3),
    ("add", None, "proj", True, 130),
    ("mean", "rw", "proj", True, 96),                    # two lane registers (65 .. 128)
    ("max", "sm", "proj", True, 520),                    # sixteen (513 .. 1024), five chunks
    ("add", "sm", "proj", False, 32, True, False),      # a gradient arriving on g_coo
    ("max", None, "proj", False, 33, True, False),
    ("add", "sm+ew", "proj", False, 32, False, True),   # dw: edge_weight.requires_grad
    ("add", "rw", "proj", True, 33, False, True),       # dw: deg.requires_grad
    ("max", "sm+ew", "proj", False, 32, True, True),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_layer_bits_equal_the_wave_path(cuda, case):
    """gate_aggregate forward + backward with the route on and off: every
    tensor ``torch.equal``; the three heavy launches ran in the first run and
    none in the second.  Max (parallel edges tie: the later slot must win on
    both paths) is compared with the wave path only."""
    runs = {}
    for on in (True, False):
        names = []
        with route(on, names):
            runs[on] = layer(cuda, *case, seed=CASES.index(case))
        assert gate_names(names) == (HEAVY_NAMES if on else WAVE_NAMES), names
    assert runs[True].keys() == runs[False].keys()
    for k, v in runs[True].items():
        assert not torch.isnan(v).any(), k
        assert torch.equal(v, runs[False][k]), f"{k}: the heavy route changed bits"
    if case[2] != "none":  # (all gates 0.5 otherwise)
        assert runs[True]["g_coo"].unique().numel() > 100


@pytest.mark.parametrize("aggr,dn", [("add", "sm"), ("mean", None)])
def test_against_the_restatement(cuda, aggr, dn):
    """The gated node model on the hub ladder, route on, against the
    plain-torch restatement in fp32 and fp64 under the edge-gate tests' bound
    (tests/edge_gate_ref.py): catches a route wrong in the same way on and
    off."""
    ei, N, _ = hub_ladder(cuda)
    spec = ("proj", dn, aggr, True, False, False, None, "")
    fin, C = 8, 32
    torch.manual_seed(5)
    nm = make_node_model(spec, num_edges=ei.size(1), fin=fin, fout=C)
    with torch.no_grad():
        nm.bias.uniform_(-0.5, 0.5)
        for p in nm.edge_gate.parameters():
            p.uniform_(-0.5, 0.5)
    gen = torch.Generator().manual_seed(6)
    x, dY = torch.randn(N, fin, generator=gen), torch.randn(N, C, generator=gen)
    P = params_of({k: v.detach() for k, v in nm.state_dict().items()})
    eic = ei.cpu()
    r32, r64 = (ref_run(x, P, eic, dY, "proj", dn, aggr, dt, relu=True)
                for dt in (torch.float32, torch.float64))
    nm = nm.to(cuda)
    xg = x.to(cuda).requires_grad_(True)
    store, names = [], []
    with route(True, names):
        y = nm.forward_fused(xg, ei, relu=True, gate_store=store)
        y.backward(dY.to(cuda))
    assert gate_names(names) == HEAVY_NAMES
    tag = f"hub/{dn}/{aggr}"
    check(tag + ".y", y, r32["y"], r64["y"])
    check(tag + ".gate", store[0].view(-1, 1), r32["gate"], r64["gate"])
    check(tag + ".dx", xg.grad, r32["dx"], r64["dx"])
    params = dict(nm.named_parameters())
    for k, v in PARAM_KEYS.items():
        if v in params:
            check(f"{tag}.g_{k}", params[v].grad, r32["g_" + k], r64["g_" + k])


PAD = 67  # guard elements on either side of a flat array


@pytest.mark.parametrize("reduce", [0, 1, 2])
def test_c_abi_schedule_windows_and_guard_bands(cuda, reduce):
    """The _sched entries with order = NULL give the bits of the entries
    without a schedule; with the schedule, Hx / Y / dY / dHx as column windows
    (ld = C + 3 / C + 7) of NaN-filled buffers and NaN (-7) bands around g, dl,
    dw, dc, da, argmax and the coef scratch, they give those bits again and
    every guard element is intact."""
    import mgcn
    from mgcn import _lib as L
    from mgcn.ops import max_mask
    lib = mgcn.load()
    C = 37
    _, N, plan = hub_ladder(cuda)
    fwd, bwd, nnz = plan.fwd, plan.bwd, plan.nnz
    slot = plan.slot_map()
    st = L.stream_of(cuda)
    gen = torch.Generator().manual_seed(8)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(cuda)  # noqa: E731
    a, c, t = rnd(N) * 0.3, rnd(N) * 0.3, rnd(nnz)
    w, wt = rnd(nnz).abs() + 0.5, rnd(nnz).abs() + 0.5
    bias, wsd, rs, dgi = rnd(C), rnd(2 * C), rnd(N), rnd(nnz)
    Hx, dY = rnd(N, C), rnd(N, C)
    bufs = []  # (buffer, mask of the guard elements, sentinel)

    def banded(n, dtype=torch.float32):
        fill = float("nan") if dtype == torch.float32 else -7
        buf = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=cuda)
        m = torch.ones(n + 2 * PAD, dtype=torch.bool, device=cuda)
        m[PAD:PAD + n] = False
        bufs.append((buf, m, fill))
        return buf[PAD:PAD + n]

    def window(ld, src=None):
        buf = torch.full((N + 2, ld), float("nan"), device=cuda)
        m = torch.ones_like(buf, dtype=torch.bool)
        m[1:N + 1, 2:2 + C] = False
        bufs.append((buf, m, float("nan")))
        win = buf[1:N + 1, 2:2 + C]
        if src is not None:
            win.copy_(src)
        return win

    def guards_ok():
        for buf, m, fill in bufs:
            v = buf[m]
            if not bool((torch.isnan(v) if fill != fill else v == fill).all()):
                return False
        return True

    def run(mode):
        """mode 'old': the entries without a schedule; 'null': _sched with
        order = NULL; 'sched': the schedule, windows and bands."""
        hard = mode == "sched"
        flat = banded if hard else (lambda n, dtype=torch.float32: torch.full(
            (n,), float("nan") if dtype == torch.float32 else -7, dtype=dtype, device=cuda))
        hx = window(C + 3, Hx) if hard else Hx
        dy = window(C + 7, dY) if hard else dY
        Y = window(C + 7) if hard else torch.full((N, C), float("nan"), device=cuda)
        dHx = window(C + 3) if hard else torch.full((N, C), float("nan"), device=cuda)
        g, dl, dw, coef_f, coef_b = (flat(nnz) for _ in range(5))
        dc, da = flat(N), flat(N)
        am = flat(N * C, torch.int32)

        def sched(view, coef):
            if mode == "old":
                return ()
            order = L.ptr(view.order) if hard else None
            tail = (order, view.n_heavy, view.n_giant)
            return tail if coef is None else tail + (L.ptr(coef),)
        sfx = "" if mode == "old" else "_sched"
        rc = getattr(lib, "mgcn_gate_fwd" + sfx)(
            N, nnz, C, L.ptr(fwd.rowptr), L.ptr(fwd.col), L.ptr(fwd.eid), L.ptr(a), L.ptr(c),
            L.ptr(t), 0, L.ptr(w), L.ptr(hx), hx.stride(0), reduce, L.ptr(bias), 1, L.ptr(Y),
            Y.stride(0), L.ptr(g), L.ptr(am), *sched(fwd, coef_f), st)
        assert rc == 0, lib.mgcn_last_error()
        win = max_mask(plan, am.view(N, C).clone()) if reduce == 2 else None
        rc = getattr(lib, "mgcn_gate_bwd_dst" + sfx)(
            N, nnz, C, L.ptr(fwd.rowptr), L.ptr(fwd.col), L.ptr(hx), hx.stride(0), L.ptr(dy),
            dy.stride(0), L.ptr(w), L.ptr(g), L.ptr(win), L.ptr(dgi), L.ptr(dl), L.ptr(dc),
            L.ptr(dw), *sched(fwd, None), st)
        assert rc == 0, lib.mgcn_last_error()
        rc = getattr(lib, "mgcn_gate_bwd_src" + sfx)(
            N, nnz, C, L.ptr(bwd.rowptr), L.ptr(bwd.col), L.ptr(slot), L.ptr(dy), dy.stride(0),
            L.ptr(wt), L.ptr(rs), L.ptr(g), L.ptr(dl), L.ptr(win), L.ptr(wsd), L.ptr(dc),
            L.ptr(da), L.ptr(dHx), dHx.stride(0), *sched(bwd, coef_b), st)
        assert rc == 0, lib.mgcn_last_error()
        torch.cuda.synchronize()
        out = {"Y": Y, "g": g, "dl": dl, "dw": dw, "dc": dc, "da": da, "dHx": dHx}
        if reduce == 2:
            out["argmax"] = am
        return {k: v.clone() for k, v in out.items()}

    old = run("old")
    for k, v in old.items():
        assert not (torch.isnan(v).any() if v.is_floating_point() else (v == -7).any()), k
    for mode in ("null", "sched"):
        got = run(mode)
        for k, v in old.items():
            assert torch.equal(got[k], v), f"{mode}: {k}"
    assert len(bufs) == 12 and guards_ok()


def _model_run(cuda, on):
    from mgcn.models import GCNModel
    ei, N, _ = hub_ladder(cuda)
    torch.manual_seed(3)
    m = GCNModel(1, [32] * 3, 2, residual_hop=1, final_type='proj', deg_norm=None,
                 edge_gate='proj', bias=False).to(cuda)
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(N, 1, generator=gen).to(cuda)
    dOut = torch.randn(N, 2, generator=gen).to(cuda)
    names = []
    torch.manual_seed(11)  # the model's dropout (0.5, training mode) draws the same masks
    with route(on, names):
        out = m(x, ei)
        out.backward(dOut)
    torch.cuda.synchronize()
    res = {"out": out.detach()}
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        res[k] = p.grad
    return res, gate_names(names)


def test_gated_model_bits(cuda):
    """A 3-layer gated GCNModel (the botnet run's shape of model) on the hub
    ladder: output and every parameter gradient ``torch.equal`` with the route
    on and off, and between two runs with it on."""
    on, n_on = _model_run(cuda, True)
    off, n_off = _model_run(cuda, False)
    again, _ = _model_run(cuda, True)
    assert n_on == HEAVY_NAMES and n_off == WAVE_NAMES
    assert len(on) >= 8 and on.keys() == off.keys()
    for k, v in on.items():
        assert torch.isfinite(v).all(), k
        assert torch.equal(v, off[k]), f"{k}: on != off"
        assert torch.equal(v, again[k]), f"{k}: two runs differ"


def test_no_heavy_rows_no_heavy_launch(cuda):
    """On a graph whose largest degree is below 128 the route, switched on,
    launches none of the heavy names."""
    from mgcn.graph import plan_for
    from mgcn.ops import gate_aggregate
    ei, N = small_graph(9, 70, 400)
    ei = ei.to(cuda)
    plan = plan_for(ei, N)
    assert plan.fwd.n_heavy == 0 and plan.bwd.n_heavy == 0
    gen = torch.Generator().manual_seed(2)
    hx = torch.randn(N, 32, generator=gen).to(cuda).requires_grad_(True)
    ws, wd = (torch.randn(32, generator=gen).to(cuda) for _ in range(2))
    names = []
    with route(True, names):
        y, _ = gate_aggregate(hx, plan, plan.norm(None), "add", ws, wd)
        y.sum().backward()
    assert gate_names(names) == WAVE_NAMES
