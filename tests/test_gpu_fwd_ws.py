"""The warp-specialised 128-wide fused forward (fused_fwd_ws.hip,
spmm_xw_fwd_ws_kernel; mgcn_set_option "xw_fwd_ws" 1) against the two-phase
kernel ("xw_fwd_ws" 0) through mgcn_spmm_xw_fwd itself: the forms differ in
which wave does what and when a load is issued, never in what is folded or
multiplied or in which order, so Y, Z and the ReLU mask words are compared BIT
FOR BIT (as int32 words), every output between guard bands; at W = I, Y is the
C oracle's aggregate bit for bit (NodeModelAdditive's gather -> * norm ->
scatter_add, src/gcn_meta/models/gcn_base_models.py:223-237).

Two graphs, each built once:
  * LADDER: row i has in-degree (0, 1, 4, 5, 6, 10, 11, 31, 32, 33, 70)[i % 11]
    -- below / at / above the 5 slots in flight, two and more rounds, the
    32-slot metadata window and the second and third metadata batch, an empty
    row between full ones; the rows of a lockstep pair (i, i + 2) never have
    equal degrees (the period is odd).  One workgroup per CU takes chunk
    b + i grid, so with G = the CU count its row-range views give a workgroup
      1, 31, 32, 33 rows            0 or 1 chunks (every other workgroup none)
      G 32 + 17                     1 and 2 chunks, a partial last chunk
      G 32 R, G 32 (R + 1) + 17     R and R + 1 / R + 2 chunks for every ring
                                    depth R the kernel can be built with (3, 4,
                                    5: the views of 3 .. 7 rounds), so each
                                    ring buffer is used again
    Views start at row 0 and at row 5, so n_cols != n_rows, and X lives in a
    table of leading dimension 160.
  * TAIL: 16 G 32 + 15 rows of degree ~3: 8 static rounds, then 8 rounds and
    a ragged chunk claimed by ticket (2 x xw_dyn_rounds = 16, less what keeps
    8 rounds static); launched 5 times, the same bits every time.  (Views of
    8 rounds or less, all of LADDER's, run every chunk static; the full-size
    stack tests claim the whole 16.)
Epilogues on every view: sum + bias + ReLU + mask + Z, mean alone (no bias,
no ReLU, no mask, no Z), sum + bias + ReLU + Z without the mask, mean + bias +
ReLU + mask.
"""
import functools

import numpy as np
import pytest
import torch

from test_gpu_fused_ws import _guarded, _intact, _t

pytestmark = pytest.mark.gpu

F = 128
R = 32  # rows per chunk
LDX = 160
LADDER = (0, 1, 4, 5, 6, 10, 11, 31, 32, 33, 70)
DEFAULT_WS = 1
# (reduce, bias, relu, mask, Z)
EPILOGUES = [("add", True, True, True, True), ("mean", False, False, False, False),
             ("add", True, True, False, True), ("mean", True, True, True, False)]


def _grid():
    """Workgroups of the warp-specialised forward: one per CU."""
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture
def fwd_ws():
    from mgcn import _lib as L
    yield lambda v: L.set_option("xw_fwd_ws", v)
    L.set_option("xw_fwd_ws", DEFAULT_WS)


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=2)
def _case(kind):
    """Graph, plan, inputs and the oracle's aggregate of one kind: built once, never written."""
    from mgcn.graph import plan_for
    from oracle import oracle
    dev = torch.device("cuda:0")
    g = _grid()
    if kind == "ladder":
        N = g * R * 7 + 17
        deg = np.array(LADDER)[np.arange(N) % len(LADDER)]
        assert (deg[:-2] != deg[2:]).all()  # lockstep pairs: unequal degrees
        rng = np.random.default_rng(11)
        d = np.repeat(np.arange(N), deg)
        s = rng.integers(0, N, d.size)
        ldx = LDX
    else:
        N = 16 * g * R + 15
        rng = np.random.default_rng(12)
        s = np.concatenate([rng.integers(0, N, 2 * N), np.arange(N)])
        d = np.concatenate([rng.integers(0, N, 2 * N), np.arange(N)])
        ldx = F
    ei = np.stack([s, d]).astype(np.int64)
    plan = plan_for(_t(ei, dev), N)
    gen = torch.Generator(device=dev).manual_seed(N)
    table = torch.randn(N, ldx, device=dev, generator=gen)
    wf, _, _ = oracle.edge_factors(ei, N, "sm")
    z_ref, _ = oracle.aggr_fwd(ei, table[:, :F].cpu().numpy(), wf, "add")
    return dict(N=N, ei=ei, plan=plan, norm=plan.norm("sm"), table=table, ldx=ldx,
                W=torch.randn(F, F, device=dev, generator=gen) * 0.1,
                b=torch.rand(F, device=dev, generator=gen) - 0.5,
                z_ref=np.asarray(z_ref, np.float32))


def _call(c, a, n, W, reduce, bias, relu, mask, want_z, what):
    """mgcn_spmm_xw_fwd on rows [a, a + n) of the case's forward view; returns
    the int32 words of (Y, Z or None, mask or None); the guard bands intact."""
    from mgcn import _lib as L
    lib = L.load()
    dev = W.device
    v = c["plan"].fwd.rows(a, a + n)
    wsb = int(lib.mgcn_spmm_xw_fwd_workspace_bytes(F, F))
    by, Y = _guarded((n, F), dev)
    bz, Z = _guarded((n, F), dev)
    bm, M = _guarded((n, 4), dev, torch.int32)
    bw, ws = _guarded((max(wsb // 4, 1),), dev)
    with L.device_guard(dev):
        rc = lib.mgcn_spmm_xw_fwd(
            n, v.n_cols, F, F, L.ptr(v.rowptr), L.ptr(v.col), L.ptr(c["norm"].w_fwd),
            L.ptr(c["table"]), c["ldx"], L.ptr(W), F, L.ptr(c["b"]) if bias else None, L.ptr(Y), F,
            L.REDUCE_CODES[reduce], int(relu), L.ptr(M) if mask else None,
            L.ptr(Z) if want_z else None, F if want_z else 0, L.ptr(ws), wsb, L.stream_of(dev))
    L.check(rc, "mgcn_spmm_xw_fwd")
    for band in (by, bz, bm, bw):
        assert _intact(band), what
    return (_bits(Y).clone(), _bits(Z).clone() if want_z else None, M.clone() if mask else None)


def _same(got, ref, what):
    for i, (u, v) in enumerate(zip(got, ref)):
        assert (u is None) == (v is None), (what, i)
        if u is not None:
            assert torch.equal(u, v), (what, i)


def _views():
    g = _grid()
    out = [(0, 1), (5, 1), (0, 31), (0, 32), (5, 33), (0, g * R + 17)]
    out += [(0, g * R * r) for r in (3, 4, 5)]
    out += [(5, g * R * 6 + 12), (0, g * R * 7 + 17)]
    return out


@pytest.mark.parametrize("vi", range(11))
def test_ladder_views_bitwise(cuda, fwd_ws, vi):
    """Every epilogue on one row-range view of the ladder graph: Y, Z and the
    mask words of "xw_fwd_ws" 1 are the two-phase kernel's bits; the sum's Z
    (and at W = I, without bias and ReLU, Y) is the oracle's aggregate."""
    c = _case("ladder")
    a, n = _views()[vi]
    assert a + n <= c["N"]
    for epi in EPILOGUES:
        out = {}
        for form in (1, 0):
            fwd_ws(form)
            out[form] = _call(c, a, n, c["W"], *epi, (vi, epi, form))
        _same(out[1], out[0], (vi, epi))
        if epi[0] == "add" and epi[4]:
            np.testing.assert_array_equal(out[1][1].view(torch.float32).cpu().numpy(),
                                          c["z_ref"][a:a + n])
    fwd_ws(1)
    eye = torch.eye(F, device=cuda)
    Y, _, _ = _call(c, a, n, eye, "add", False, False, False, False, (vi, "eye"))
    np.testing.assert_array_equal(Y.view(torch.float32).cpu().numpy(), c["z_ref"][a:a + n])


def test_ticketed_tail_repeatable(cuda, fwd_ws):
    """16 rounds + 15 rows: the last 8 rounds are claimed by ticket.  Five
    launches of "xw_fwd_ws" 1, each the two-phase kernel's bits; at W = I the
    oracle's aggregate."""
    c = _case("tail")
    N = c["N"]
    assert N // R // _grid() >= 16
    epi = ("add", True, True, True, True)
    fwd_ws(0)
    base = _call(c, 0, N, c["W"], *epi, "two-phase")
    fwd_ws(1)
    for rep in range(5):
        _same(_call(c, 0, N, c["W"], *epi, rep), base, rep)
    eye = torch.eye(F, device=cuda)
    Y, Z, _ = _call(c, 0, N, eye, "mean", False, False, False, True, "eye")
    cnt = np.maximum(np.bincount(c["ei"][1], minlength=N), 1).astype(np.float32)
    np.testing.assert_array_equal(Z.view(torch.float32).cpu().numpy(), c["z_ref"])
    np.testing.assert_array_equal(Y.view(torch.float32).cpu().numpy(),
                                  (c["z_ref"] / cnt[:, None]).astype(np.float32))


def test_option_values(cuda, fwd_ws):
    """xw_fwd_ws takes 0 and 1."""
    from mgcn import _lib as L
    for v in (-1, 2):
        with pytest.raises(L.MgcnError):
            L.set_option("xw_fwd_ws", v)
    fwd_ws(0)
    fwd_ws(1)
