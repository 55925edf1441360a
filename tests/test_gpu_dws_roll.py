"""The rolling gather of the warp-specialised F = 128 adjoint (fused_dws.hip,
spmm_xw_bwd_ws_kernel, mgcn_set_option "xw_ws_roll"): 0 issues a row quad's
gathers in batches, 2 (the default) refills a slot as soon as it is folded and
hands the last slots of a quad to the wave's next quad.  (1, the refill within
a quad alone, was measured, lost and is removed: DESIGN section 4.)  The forms
differ in WHEN a load is issued, never in what is folded or in which order, so
every output -- dX, dW, the bias column sums and, with dy_colsum_out, dY's own
column sums -- is compared bit for bit between them, through ops.spmm_xw_bwd
and through the C ABI on row-range views between guard bands.

Shapes (a gather wave walks quads of 4 consecutive rows, 8 quads to a 32-row
chunk, chunks dealt to one workgroup per CU; a quad's rounds are
ceil(max degree / U), U = 5, within 32-slot metadata windows):
  * the degree ladder 0 .. 66 (crosses U, 2 U, the window and two windows), as
    it is, permuted into chosen quads, and tiled so that every wave carries
    every such quad into a next one;
  * 1 .. 130 rows: fewer quads than gather waves, partial quads and chunks;
  * 256 * 32 * 3 + 17 rows: three chunks and more per workgroup, so each ring
    buffer is used again and the carry crosses chunk boundaries;
  * the three epilogues, dW alone, a hub row of 700, the max adjoint (which
    keeps the batch form).
"""
import numpy as np
import pytest
import torch

from attention_ref import ladder_graph
from test_gpu_fused_ws import BAND, F, _graph, _guarded, _intact, _plan, _t  # noqa: F401

pytestmark = pytest.mark.gpu

ROLLS = (0, 2)
DEFAULT_ROLL = 2


@pytest.fixture
def roll():
    from mgcn import _lib as L
    yield lambda v: L.set_option("xw_ws_roll", v)
    L.set_option("xw_ws_roll", DEFAULT_ROLL)


def _same(a, b, what):
    assert len(a) == len(b)
    for i, (u, v) in enumerate(zip(a, b)):
        assert (u is None) == (v is None), (what, i)
        if u is not None:
            assert torch.equal(u, v), (what, i)


def _all_rolls(roll, call, what):
    """call() under every xw_ws_roll value; asserts the same bits; returns roll 0's."""
    out = {}
    for r in ROLLS:
        roll(r)
        out[r] = call()
    for r in ROLLS[1:]:
        _same(out[r], out[0], (what, r))
    return out[0]


def _inputs(cuda, N, seed):
    g = torch.Generator(device=cuda).manual_seed(seed)
    dY = torch.randn(N, F, device=cuda, generator=g)
    X = torch.randn(N, F, device=cuda, generator=g)
    lower = torch.randn(N, F, device=cuda, generator=g)
    W = torch.randn(F, F, device=cuda, generator=g) * 0.1
    return dY, X, lower, W


def _with_hcs(ops, plan, norm, dY, X, W, **kw):
    """(dW, dX, colsum, dY's column sums) of the HCS launch."""
    hc = torch.full((F,), float("nan"), device=dY.device)
    return ops.spmm_xw_bwd(plan.bwd, norm.w_bwd, norm.row_scale_bwd, dY, X, W, dy_colsum_out=hc,
                           **kw) + (hc,)


# ------------------------------------------------------------ degree ladder

def _ladder(kind):
    """(ei [2, E] numpy, N).  The adjoint's row v gathers over v's out-edges:
    nodes 67 + v have out-degree v (v = 0 .. 66), nodes 0 .. 66 none."""
    ei, N = ladder_graph()
    ei = ei.numpy()
    if kind == "as_is":
        return ei, N
    # rows in a new order: quad 0 = degrees (0, 0, 0, 0), quad 1 = (0, 33, 0, 5),
    # quad 2 = (66, 1, 0, 32), quads 3 .. 5 empty, ..., the last quad empty
    head = [0, 1, 2, 3, 4, 67 + 33, 5, 67 + 5, 67 + 66, 67 + 1, 6, 67 + 32] + list(range(7, 19))
    tail = [19, 20, 21, 22]
    rest = [v for v in range(N) if v not in set(head) | set(tail)]
    order = np.array(head + rest + tail)
    assert len(order) == N and len(set(order.tolist())) == N
    new_id = np.empty(N, np.int64)
    new_id[order] = np.arange(N)
    ei = new_id[ei]
    outd = np.bincount(ei[0], minlength=N)
    assert list(outd[:24]) == [0, 0, 0, 0, 0, 33, 0, 5, 66, 1, 0, 32] + [0] * 12
    assert not outd[N - 4:].any()
    if kind == "permuted":
        return ei, N
    # tiled: 130 disjoint copies = 26000 rows, more than three chunks for each
    # of up to 256 workgroups, so the carry meets every quad above
    K = 130
    ei = np.concatenate([ei + k * N for k in range(K)], axis=1)
    return ei, K * N


@pytest.mark.parametrize("kind", ["as_is", "permuted", "tiled"])
def test_degree_ladder(cuda, oracle, roll, kind):
    """Rows of every degree 0 .. 66, empty quads in runs and at the end: the
    same bits for xw_ws_roll 0 / 2, plain and with dY's column sums; the
    permuted ladder's dX at W = I is the oracle's adjoint, bit for bit."""
    from mgcn import ops
    ei, N = _ladder(kind)
    plan, norm = _plan(cuda, ei, N, "sm")
    dY, X, lower, W = _inputs(cuda, N, 101)
    rm = ops.make_relu_mask(lower)
    _all_rolls(roll, lambda: ops.spmm_xw_bwd(plan.bwd, norm.w_bwd, norm.row_scale_bwd, dY, X, W,
                                             relu_mask=rm), kind)
    _all_rolls(roll, lambda: _with_hcs(ops, plan, norm, dY, X, W, relu_mask=rm), kind + " hcs")
    if kind == "permuted":
        eye = torch.eye(F, device=cuda)
        _, dX, _ = _all_rolls(roll, lambda: ops.spmm_xw_bwd(plan.bwd, norm.w_bwd,
                                                            norm.row_scale_bwd, dY, X, eye,
                                                            relu_mask=rm), "eye")
        _, wb, rs = oracle.edge_factors(ei, N, "sm")
        dH, _ = oracle.aggr_bwd(ei, dY.cpu().numpy(), wb, rs, "add")
        ref = np.where(lower.cpu().numpy() > 0, np.asarray(dH, np.float32), 0).astype(np.float32)
        np.testing.assert_array_equal(dX.cpu().numpy(), ref)


# ------------------------------------------------------ quad and chunk edges

EDGE_ROWS = [1, 3, 4, 5, 28, 31, 32, 33, 130]


@pytest.mark.parametrize("n_rows", EDGE_ROWS)
def test_quad_and_chunk_edges_whole_view(cuda, roll, n_rows):
    """Whole graphs of 1 .. 130 rows (fewer quads than the 8 gather waves, a
    partial last quad, a partial last chunk): the same bits for every roll."""
    from mgcn import ops
    rng = np.random.default_rng(300 + n_rows)
    s = rng.integers(0, n_rows, 7 * n_rows)
    d = rng.integers(0, n_rows, 7 * n_rows)
    ei = np.stack([s, d]).astype(np.int64)  # (no self-loops: empty rows stay)
    plan, norm = _plan(cuda, ei, n_rows, "sm")
    dY, X, lower, W = _inputs(cuda, n_rows, 7 + n_rows)
    rm = ops.make_relu_mask(lower)
    _all_rolls(roll, lambda: ops.spmm_xw_bwd(plan.bwd, norm.w_bwd, norm.row_scale_bwd, dY, X, W,
                                             relu_mask=rm, row_div=plan.in_cnt), n_rows)
    _all_rolls(roll, lambda: _with_hcs(ops, plan, norm, dY, X, W, relu_mask=rm), (n_rows, "hcs"))


def test_quad_and_chunk_edges_row_ranges_c_abi(cuda, roll):
    """mgcn_spmm_xw_bwd itself on row-range views of 1 .. 130 rows that start
    at rows 5 and 211, every output between guard bands: the bands intact and
    dX / dW / the column sums the same bits for every roll."""
    from mgcn import _lib as L
    from mgcn import ops
    N = 600
    rng = np.random.default_rng(19)
    ei = _graph(rng, N, 5000)
    plan, norm = _plan(cuda, ei, N, "sm")
    lib = L.load()
    dY, X, lower, W = _inputs(cuda, N, 6)
    rm = ops.make_relu_mask(lower)
    for a in (5, 211):
        for n in EDGE_ROWS:
            v = plan.bwd.rows(a, a + n)
            wsb = int(lib.mgcn_spmm_xw_bwd_workspace_bytes(n, F, F))
            got = {}
            for r in ROLLS:
                roll(r)
                bx, dX = _guarded((n, F), cuda)
                bc, cs = _guarded((F,), cuda)
                bw, dW = _guarded((F, F), cuda)
                bws, ws = _guarded((max(wsb // 4, 1),), cuda)
                with L.device_guard(cuda):
                    rc = lib.mgcn_spmm_xw_bwd(
                        n, v.n_cols, F, F, L.ptr(v.rowptr), L.ptr(v.col), L.ptr(norm.w_bwd), None,
                        L.ptr(dY), F, L.ptr(X[a:]), F, L.ptr(W), F, L.ptr(dW), F, 0, L.ptr(dX), F,
                        L.ptr(rm[a:]), None, L.ptr(cs), None, None, L.ptr(ws), wsb,
                        L.stream_of(cuda))
                L.check(rc, "mgcn_spmm_xw_bwd")
                for b in (bx, bc, bw, bws):
                    assert _intact(b), (a, n, r)
                got[r] = (dW.clone(), dX.clone(), cs.clone())
            for r in ROLLS[1:]:
                _same(got[r], got[0], (a, n, r))


# ----------------------------------------------------------- ring generations

def test_ring_generations_repeatable(cuda, roll):
    """256 * 32 * 3 + 17 rows, about 10 edges each: every workgroup runs at
    least three chunks, so both ring buffers are used again and a wave's
    carried slots cross chunk boundaries.  Five launches per roll value, all
    ten with the same bits (and the HCS launch among the rolls)."""
    from mgcn import ops
    N = 256 * 32 * 3 + 17
    rng = np.random.default_rng(77)
    ei = _graph(rng, N, 9 * N)
    plan, norm = _plan(cuda, ei, N, "sm")
    dY, X, lower, W = _inputs(cuda, N, 78)
    rm = ops.make_relu_mask(lower)
    first = None
    for r in ROLLS:
        roll(r)
        for rep in range(5):
            out = ops.spmm_xw_bwd(plan.bwd, norm.w_bwd, norm.row_scale_bwd, dY, X, W, relu_mask=rm)
            if first is None:
                first = out
            else:
                _same(out, first, (r, rep))
    hc = _all_rolls(roll, lambda: _with_hcs(ops, plan, norm, dY, X, W, relu_mask=rm), "hcs")
    _same(hc[:3], first, "hcs vs plain")


# ------------------------------------------------------------------ epilogues

@pytest.mark.parametrize("N,E,hub", [(4097, 40000, 0), (3000, 20000, 700)])
@pytest.mark.parametrize("deg_norm,epi", [("sm", "relu"), ("rw", "relu_div"), (None, "store")])
def test_epilogues(cuda, roll, N, E, hub, deg_norm, epi):
    """sm + relu, rw + relu_div (mean) and none + store, on a plain graph and
    on one with a hub row of 700; with dX and as dW alone: the same bits for
    every roll.  sm + relu without the hub also against mgcn_spmm_bwd +
    mgcn_gemm_bwd: dX bit for bit, dW within the fp64 |.|-bound of X^T dH."""
    from mgcn import _lib as L
    from mgcn import ops
    rng = np.random.default_rng(7 * N + E + len(epi))
    ei = _graph(rng, N, E, hub)
    plan, norm = _plan(cuda, ei, N, deg_norm)
    dY, X, lower, W = _inputs(cuda, N, N + 29)
    rm = ops.make_relu_mask(lower) if epi != "store" else None
    rd = plan.in_cnt if epi == "relu_div" else None
    dW, dX, cs = _all_rolls(roll, lambda: ops.spmm_xw_bwd(plan.bwd, norm.w_bwd,
                                                          norm.row_scale_bwd, dY, X, W,
                                                          relu_mask=rm, row_div=rd), epi)
    only = _all_rolls(roll, lambda: ops.spmm_xw_bwd(plan.bwd, norm.w_bwd, norm.row_scale_bwd, dY,
                                                    X, W, want_dx=False), epi + " dW alone")
    assert only[1] is None and torch.equal(only[0], dW)
    if epi == "relu" and not hub:
        dH = ops.spmm_bwd(plan.bwd, norm.w_bwd, norm.row_scale_bwd, dY, L.REDUCE_SUM)
        _, dXa, csa = ops.gemm_bwd(X, dH, W, relu_mask=rm)
        assert torch.equal(dX, dXa)
        ref = X.double().t() @ dH.double()
        bound = X.double().abs().t() @ dH.double().abs()
        assert ((dW.double() - ref).abs() <= 1e-5 * bound + 1e-6).all()
        torch.testing.assert_close(cs, csa, rtol=1e-4, atol=1e-3)


# --------------------------------------------------------------- max untouched

def test_max_adjoint_keeps_batch_form(cuda, roll):
    """The max adjoint on DWS (win_mask + slot_map) does not take the rolling
    gather: xw_ws_roll 2 and 0 give the same bits."""
    from mgcn import _lib as L
    from mgcn import ops
    N, E = 4097, 40000
    rng = np.random.default_rng(55)
    ei = _graph(rng, N, E)
    plan, norm = _plan(cuda, ei, N, None)
    dY, X, lower, W = _inputs(cuda, N, 56)
    H = torch.randn(N, F, device=cuda, generator=torch.Generator(device=cuda).manual_seed(57))
    _, win = ops.spmm_fwd(plan.fwd, norm.w_fwd, H, L.REDUCE_MAX, mask_plan=plan)
    sm = plan.slot_map()
    rm = ops.make_relu_mask(lower)
    out = {}
    for r in (0, 2):
        roll(r)
        out[r] = ops.spmm_xw_bwd(plan.bwd, norm.w_bwd, norm.row_scale_bwd, dY, X, W, relu_mask=rm,
                                 win_mask=win, slot_map=sm)
    _same(out[2], out[0], "max")


def test_removed_value_is_refused(cuda, roll):
    """xw_ws_roll takes 0 and 2; 1 (measured slower than 2, removed) and 3 are errors."""
    from mgcn import _lib as L
    for v in (1, 3, -1):
        with pytest.raises(L.MgcnError):
            L.set_option("xw_ws_roll", v)
    roll(0)
    roll(2)
