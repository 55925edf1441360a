"""The gate kernels' branch structure on the MI355X: every width
instantiation, rows of every degree around the 64-slot chunk, more rows than
one grid trip, every nullable argument, and leading dimensions through the C
ABI.  All cases against the plain-torch restatement (tests/edge_gate_ref.py)
run in fp32 and fp64 on the CPU, under the bound

    max|t_gpu - t64| <= max(4 * max|t32 - t64|, 1e-5 * max|t64|)
"""
import numpy as np
import pytest
import torch

from edge_gate_ref import (PARAM_KEYS, check, ladder_graph, make_node_model, max_gap,
                           max_hub_graph, params_of, ref_run, small_graph)

pytestmark = pytest.mark.gpu

FIN = 8
GRID_ROWS = 4096 * 4  # att_grid: at most 4096 workgroups of 4 waves, one row per wave


def _model(spec, C, E, seed):
    torch.manual_seed(seed)
    nm = make_node_model(spec, num_edges=E, fin=FIN, fout=C)
    with torch.no_grad():
        if nm.bias is not None:
            nm.bias.uniform_(-0.5, 0.5)
        for p in nm.edge_gate.parameters():
            p.uniform_(-0.5, 0.5)
    return nm


def _run(cuda, spec, C, ei, N, seed=0, relu=False):
    """One layer, forward and backward, on the GPU and in the restatement."""
    gate, dn, aggr, bias, use_ew, _deg, edim, _ = spec
    E = ei.size(1)
    gen = torch.Generator().manual_seed(seed + 1)
    for trial in range(64):  # max: a draw whose fp64 winners win by a margin
        nm = _model(spec, C, E, seed + 1000 * trial)
        x = torch.randn(N, FIN, generator=gen)
        dY = torch.randn(N, C, generator=gen)
        ea = torch.randn(E, edim, generator=gen) if edim else None
        ew = torch.rand(E, generator=gen) + 0.5 if use_ew else None
        P = params_of({k: v.detach() for k, v in nm.state_dict().items()})
        r64 = ref_run(x, P, ei, dY, gate, dn, aggr, torch.float64, edge_attr=ea, edge_weight=ew,
                      relu=relu)
        if aggr != "max" or max_gap(r64["msg"], ei[1], N) > 1e-4:
            break
    else:
        raise AssertionError("no draw passes the max gap condition")
    r32 = ref_run(x, P, ei, dY, gate, dn, aggr, torch.float32, edge_attr=ea, edge_weight=ew,
                  relu=relu)
    nm = nm.to(cuda)
    xg = x.to(cuda).requires_grad_(True)
    store = []
    y = nm.forward_fused(xg, ei.to(cuda), None if ea is None else ea.to(cuda), None,
                         None if ew is None else ew.to(cuda), relu=relu, gate_store=store)
    y.backward(dY.to(cuda))
    tag = f"{gate}/{dn}/{aggr}/C{C}"
    check(tag + ".y", y, r32["y"], r64["y"])
    check(tag + ".gate", store[0].view(-1, 1), r32["gate"], r64["gate"])
    check(tag + ".dx", xg.grad, r32["dx"], r64["dx"])
    sd_keys = dict(nm.named_parameters())
    for k, v in PARAM_KEYS.items():
        if v in sd_keys:
            check(f"{tag}.g_{k}", sd_keys[v].grad, r32["g_" + k], r64["g_" + k])
    return y.detach()


WIDTHS = [1, 7, 32, 33, 64, 65, 129, 257, 513, 1024]


@pytest.mark.parametrize("C", WIDTHS)
def test_every_width_sum_and_max(cuda, C):
    """C = 1 .. 1024: every lanes-hold-f = l + 64 i instantiation (FPL 1, 2, 4,
    8, 16) with partly filled last registers, for the sum and the max kernels
    (max on a graph without parallel edges)."""
    ei, N = small_graph(3, 90, 500)
    _run(cuda, ("proj", "sm", "add", True, False, False, None, ""), C, ei, N, seed=C)
    # few rows with two or more in-edges: at C = 1024 a draw must still keep
    # every (node, feature) winner 1e-4 max|m| ahead
    ei, N = small_graph(4, 24, 22)
    _run(cuda, ("proj", "rw", "max", True, False, False, None, ""), C, ei, N, seed=C)


@pytest.mark.parametrize("dn,use_ew", [("sm", False), ("sm", True), ("rw", False), ("rw", True),
                                       (None, False)])
@pytest.mark.parametrize("C", [3, 33])
def test_max_on_long_rows_under_every_norm(cuda, dn, use_ew, C):
    """Max with rows of in-degree 71 and 141 and out-degree 70 and 140 (the
    winner carried across 64-slot chunks, winner bits of long rows read
    through the slot map; C = 33: two winner words per slot) under
    'sm' and 'rw' with and without edge weights and under None: per-slot
    weights in both views ('sm', edge weights) and the 'rw' row post-scale.
    Every draw passes the gap condition (_run)."""
    ei, N = max_hub_graph()
    _run(cuda, ("proj", dn, "max", True, use_ew, False, None, ""), C, ei, N, seed=17 + C)


@pytest.mark.parametrize("aggr,dn", [("add", "sm"), ("mean", None), ("add", "rw")])
def test_degree_ladder(cuda, aggr, dn):
    """A row of every in-degree and out-degree 0 .. 130 (one below, at and one
    above the 64-slot chunk, twice); rows without in-edges give exactly 0."""
    ei, N = ladder_graph()
    y = _run(cuda, ("proj", dn, aggr, False, False, False, None, ""), 33, ei, N, seed=7)
    empty = torch.from_numpy(np.bincount(ei[1].numpy(), minlength=N) == 0)
    assert empty.sum() >= 132
    assert torch.count_nonzero(y[empty.to(cuda)]) == 0


def test_more_rows_than_two_grid_trips(cuda):
    """N = two full grid trips of the launch cap plus 37, with two hubs (in-
    and out-degree 200) and empty rows in the last trip."""
    N = 2 * GRID_ROWS + 37
    rng = np.random.default_rng(41)
    last = 2 * GRID_ROWS
    parts = [rng.integers(0, last + 20, (2, 70000)),
             np.stack([rng.integers(0, N - 10, 200), np.full(200, last + 25)]),
             np.stack([np.full(200, last + 26), rng.integers(0, N - 10, 200)])]
    ei = np.concatenate(parts, axis=1)
    ei = torch.from_numpy(ei[:, rng.permutation(ei.shape[1])].astype(np.int64))
    ind = np.bincount(ei[1].numpy(), minlength=N)
    assert ind[last + 25] >= 200 and not ind[N - 10:].any()
    y = _run(cuda, ("proj", None, "add", False, False, False, None, ""), 8, ei, N, seed=2)
    assert torch.count_nonzero(y[N - 10:]) == 0


NULLABLE = [  # a / c, t and w of mgcn_gate_fwd, each absent and present
    ("free", None, "add", False, False, False, None, ""),    # a, c null; t [nnz]; w null
    ("free", "sm", "mean", True, True, False, None, ""),     # a, c null; t [nnz]; w given
    ("proj", None, "max", True, False, False, None, ""),     # t one element; w null
    ("proj", "sm", "add", True, True, False, None, ""),      # t one element; w given
    ("proj", "rw", "add", True, False, False, 3, ""),        # t [nnz] (edge features)
    ("proj", None, "mean", False, False, False, 3, ""),
]


@pytest.mark.parametrize("spec", NULLABLE, ids=lambda s: "-".join(str(v) for v in s[:7]))
@pytest.mark.parametrize("relu", [False, True])
def test_nullable_arguments(cuda, spec, relu):
    ei, N = small_graph(9, 70, 400)
    _run(cuda, spec, 32, ei, N, seed=11, relu=relu)


def test_scores_without_a_logit_term(cuda):
    """a and c given, t null (gate_aggregate without a bias)."""
    from mgcn.graph import plan_for
    from mgcn.ops import gate_aggregate
    ei, N = small_graph(9, 70, 400)
    gen = torch.Generator().manual_seed(3)
    hx = torch.randn(N, 33, generator=gen)
    ws, wd = (torch.rand(1, 33, generator=gen) - 0.5 for _ in range(2))
    dY = torch.randn(N, 33, generator=gen)
    P = {"weight_node": torch.eye(33), "linsrc": ws, "lintgt": wd}
    r32, r64 = (ref_run(hx, P, ei, dY, "proj", None, "add", dt)
                for dt in (torch.float32, torch.float64))
    h = hx.to(cuda).requires_grad_(True)
    a, b = ws.to(cuda).requires_grad_(True), wd.to(cuda).requires_grad_(True)
    plan = plan_for(ei.to(cuda), N)
    y, g = gate_aggregate(h, plan, plan.norm(None), "add", a, b)
    y.backward(dY.to(cuda))
    check("not.y", y, r32["y"], r64["y"])
    check("not.gate", g.view(-1, 1), r32["gate"], r64["gate"])
    check("not.dx", h.grad, r32["dx"], r64["dx"])
    check("not.g_linsrc", a.grad, r32["g_linsrc"], r64["g_linsrc"])
    check("not.g_lintgt", b.grad, r32["g_lintgt"], r64["g_lintgt"])


@pytest.mark.parametrize("reduce", [0, 2])
def test_leading_dimensions_and_row_range_through_the_c_abi(cuda, reduce):
    """Hx, Y, dY and dHx as column windows with ld = C + 3 / 5 / 5 / 7 inside
    NaN-filled buffers: the results equal the packed call's bit for bit and the
    guard bands stay untouched; each of the three kernels over two row ranges
    equals the call over all rows."""
    import mgcn
    from mgcn import _lib as L
    from mgcn.graph import plan_for
    from mgcn.ops import max_mask
    lib = mgcn.load()
    C = 37
    ei, N = small_graph(13, 80, 450)
    plan = plan_for(ei.to(cuda), N)
    fwd, bwd, nnz = plan.fwd, plan.bwd, plan.nnz
    st = L.stream_of(cuda)
    gen = torch.Generator().manual_seed(8)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(cuda)  # noqa: E731
    a, c, t, w, wt = rnd(N), rnd(N), rnd(nnz), rnd(nnz).abs() + 0.5, rnd(nnz).abs() + 0.5
    bias, wsd, dc_in = rnd(C), rnd(2 * C), rnd(N)

    def window(rows, ld, src=None):
        buf = torch.full((rows + 2, ld), float("nan"), device=cuda)
        win = buf[1:rows + 1, 2:2 + C]
        if src is not None:
            win.copy_(src)
        return buf, win

    def guard_ok(buf, rows):
        m = torch.ones_like(buf, dtype=torch.bool)
        m[1:rows + 1, 2:2 + C] = False
        return bool(torch.isnan(buf[m]).all())

    def forward(Hx, Y, r0=0, r1=N, g=None, am=None):
        g = torch.full((nnz,), float("nan"), device=cuda) if g is None else g
        am = torch.full((N, C), -7, dtype=torch.int32, device=cuda) if am is None else am
        rp = fwd.rowptr[r0:]
        rc = lib.mgcn_gate_fwd(r1 - r0, nnz, C, L.ptr(rp), L.ptr(fwd.col), L.ptr(fwd.eid), L.ptr(a),
                               L.ptr(c[r0:]), L.ptr(t), 0, L.ptr(w), L.ptr(Hx), Hx.stride(0), reduce,
                               L.ptr(bias), 1, L.ptr(Y[r0:]), Y.stride(0), L.ptr(g),
                               L.ptr(am[r0:]), st)
        assert rc == 0, lib.mgcn_last_error()
        return g, am

    Hx = rnd(N, C)
    Y0 = torch.empty(N, C, device=cuda)
    g0, am0 = forward(Hx, Y0)
    hbuf, hwin = window(N, C + 3, Hx)
    ybuf, ywin = window(N, C + 5)
    g1, am1 = forward(hwin, ywin)
    assert torch.equal(ywin, Y0) and torch.equal(g1, g0) and torch.equal(am1, am0)
    assert guard_ok(ybuf, N) and not torch.isnan(g0).any()
    # two row ranges
    Y2 = torch.full((N, C), float("nan"), device=cuda)
    g2, am2 = forward(Hx, Y2, 0, 31)
    forward(Hx, Y2, 31, N, g2, am2)
    assert torch.equal(Y2, Y0) and torch.equal(g2, g0) and torch.equal(am2, am0)

    win = max_mask(plan, am0) if reduce == 2 else None
    dY = rnd(N, C)

    def backward(Hx, dY, dHx, ranges=((0, N),)):
        """Both adjoint kernels, each over the given row ranges: the row-indexed
        arrays (bwd_dst: dY, dc; bwd_src: row_scale, dc, da, dHx) advanced to
        the range's first row, the slot- and column-indexed ones as they are."""
        dl = torch.full((nnz,), float("nan"), device=cuda)
        dw = torch.full((nnz,), float("nan"), device=cuda)
        dc = torch.full((N,), float("nan"), device=cuda)
        da = torch.full((N,), float("nan"), device=cuda)
        for r0, r1 in ranges:
            rc = lib.mgcn_gate_bwd_dst(r1 - r0, nnz, C, L.ptr(fwd.rowptr[r0:]), L.ptr(fwd.col),
                                       L.ptr(Hx), Hx.stride(0), L.ptr(dY[r0:]), dY.stride(0),
                                       L.ptr(w), L.ptr(g0), L.ptr(win), L.ptr(t), L.ptr(dl),
                                       L.ptr(dc[r0:]), L.ptr(dw), st)
            assert rc == 0, lib.mgcn_last_error()
        for r0, r1 in ranges:
            rc = lib.mgcn_gate_bwd_src(r1 - r0, nnz, C, L.ptr(bwd.rowptr[r0:]), L.ptr(bwd.col),
                                       L.ptr(plan.slot_map()), L.ptr(dY), dY.stride(0), L.ptr(wt),
                                       L.ptr(dc_in[r0:]), L.ptr(g0), L.ptr(dl), L.ptr(win),
                                       L.ptr(wsd), L.ptr(dc[r0:]), L.ptr(da[r0:]),
                                       L.ptr(dHx[r0:]), dHx.stride(0), st)
            assert rc == 0, lib.mgcn_last_error()
        return dl, dw, dc, da

    dH0 = torch.empty(N, C, device=cuda)
    out0 = backward(Hx, dY, dH0)
    dybuf, dywin = window(N, C + 5, dY)
    dhbuf, dhwin = window(N, C + 7)
    out1 = backward(hwin, dywin, dhwin)
    assert torch.equal(dhwin, dH0) and guard_ok(dhbuf, N) and guard_ok(hbuf, N)
    for p, q in zip(out0, out1):
        assert torch.equal(p, q) and not torch.isnan(p).any()
    assert not torch.isnan(dH0).any()
    # two row ranges per adjoint kernel
    dH2 = torch.full((N, C), float("nan"), device=cuda)
    out2 = backward(Hx, dY, dH2, ranges=((0, 31), (31, N)))
    assert torch.equal(dH2, dH0)
    for p, q in zip(out0, out2):
        assert torch.equal(p, q)
