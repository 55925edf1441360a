"""The dynamic claim of the 128-wide forward's last rounds (fused_fwd.hip,
spmm_xw_fwd_kernel DYN; mgcn_set_option "xw_dyn_rounds", default 8): which
workgroup runs a chunk of the tail is decided on the device, what it computes
is not.

Reference: NodeModelAdditive's forward, x @ weight_node then gather -> * norm
-> scatter_add + bias (src/gcn_meta/models/gcn_base_models.py:199-243),
through the C oracle at W = I as the other fused-forward tests.  Bars:
  * Y, Z and the ReLU mask words are per-row results: BIT FOR BIT the static
    assignment's ("xw_dyn_rounds" 0) on every one of 5 repeated launches, and
    the oracle's at W = I;
  * without the workspace the entry assigns statically: same bits;
  * bench.build_stack's 3-layer step with the default against the static
    assignment: y and every gradient bit for bit (the adjoint kernels are the
    same ones, on the same bits).
Shapes (the kernel launches 2 workgroups per CU = 512; the claim needs 8
static rounds before the claimed ones): 9 rounds + a 15-row chunk with 1
claimed round (the smallest launch that takes the path, a ragged pool), 16
rounds exactly (where the default of 8 rounds starts to apply, pool = whole
rounds), one chunk less (static), 17 rounds + 3 chunks, and 12 rounds + 1 row
with 4 claimed; degrees ~7, half 1 / half 40, and a run of 3000 empty rows in
the claimed tail.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F = 128
R = 32  # rows per chunk


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.detach().cpu().numpy()


def _grid():
    """Workgroups of the forward: 2 per CU."""
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count


def _edges(kind, N):
    rng = np.random.default_rng(N + len(kind))
    loops = np.arange(N)
    if kind == "skew":  # odd rows: 39 in-edges + the loop; even rows: the loop alone
        d = np.repeat(np.arange(1, N, 2), 39)
        s = rng.integers(0, N, d.size)
    else:
        s = rng.integers(0, N, 6 * N)
        d = rng.integers(0, N, 6 * N)
    s, d = np.concatenate([s, loops]), np.concatenate([d, loops])
    if kind == "gap":  # 3000 consecutive rows without a slot, inside the claimed tail
        keep = (d < N - 5000) | (d >= N - 2000)
        s, d = s[keep], d[keep]
    return np.stack([s, d]).astype(np.int64)


@pytest.fixture
def dyn_rounds():
    from mgcn import _lib as L
    yield lambda v: L.set_option("xw_dyn_rounds", v)
    L.set_option("xw_dyn_rounds", 8)  # the default


@functools.lru_cache(maxsize=2)
def _case(kind, N):
    """Graph, plan and inputs of one (kind, N): built once, never written."""
    from mgcn.graph import plan_for
    dev = torch.device("cuda:0")
    ei = _edges(kind, N)
    plan = plan_for(_t(ei, dev), N)
    g = torch.Generator(device=dev).manual_seed(N)
    return dict(ei=ei, plan=plan, norm=plan.norm("sm"),
                X=torch.randn(N, F, device=dev, generator=g),
                W=torch.randn(F, F, device=dev, generator=g) * 0.1,
                b=torch.rand(F, device=dev, generator=g) - 0.5)


def _fwd(c, reduce, W):
    from mgcn import ops
    view = c["plan"].fwd
    rm = torch.zeros(view.n_rows, 4, dtype=torch.int32, device=W.device)
    Y, Z = ops.spmm_xw_fwd(view, c["norm"].w_fwd, c["X"], W, reduce, c["b"], True, relu_mask=rm,
                           want_z=True)
    return Y, Z, rm


def _sizes():
    g = _grid()
    return {"9r+15rows/1": (9 * g * R + 15, 1), "16r/8": (16 * g * R, 8),
            "16r-1chunk/8": (16 * g * R - R, 8), "17r+3chunks/8": ((17 * g + 3) * R, 8),
            "12r+1row/4": (12 * g * R + 1, 4)}


@pytest.mark.parametrize("kind,aggr", [("rand", "add"), ("skew", "mean"), ("gap", "add")])
@pytest.mark.parametrize("shape", ["9r+15rows/1", "16r/8", "16r-1chunk/8", "17r+3chunks/8",
                                   "12r+1row/4"])
def test_forward_dynamic_claim_bitwise(cuda, oracle, dyn_rounds, shape, kind, aggr):
    """5 launches with the tail claimed: Y, Z and the mask words bit for bit
    the static assignment's, at W = I and at a random W; at W = I bit for bit
    the oracle's layer."""
    from mgcn import _lib as L
    N, rounds = _sizes()[shape]
    c = _case(kind, N)
    reduce = L.REDUCE_CODES[aggr]
    eye = torch.eye(F, device=cuda)
    for W in (eye, c["W"]):
        dyn_rounds(0)
        base = _fwd(c, reduce, W)
        dyn_rounds(rounds)
        for _ in range(5):
            for a, b in zip(_fwd(c, reduce, W), base):
                assert torch.equal(a, b)
    wf, _, _ = oracle.edge_factors(c["ei"], N, "sm")
    y_ref, _ = oracle.aggr_fwd(c["ei"], _np(c["X"]), wf, aggr, _np(c["b"]), True)
    z_ref, _ = oracle.aggr_fwd(c["ei"], _np(c["X"]), wf, "add")
    Y, Z, _ = _fwd(c, reduce, eye)
    np.testing.assert_array_equal(_np(Y), y_ref)
    np.testing.assert_array_equal(_np(Z), z_ref)


def test_forward_without_workspace_is_static(cuda, dyn_rounds):
    """mgcn_spmm_xw_fwd with a NULL or short workspace (callers from before
    the claim existed): the static assignment, same bits; the option's range."""
    from mgcn import _lib as L
    from mgcn import ops
    lib = L.load()
    N = _sizes()["9r+15rows/1"][0]
    c = _case("rand", N)
    dyn_rounds(1)
    Y0 = ops.spmm_xw_fwd(c["plan"].fwd, c["norm"].w_fwd, c["X"], c["W"], L.REDUCE_SUM, c["b"])
    need = int(lib.mgcn_spmm_xw_fwd_workspace_bytes(F, F))
    assert need >= 4 + 8 * _grid()
    v = c["plan"].fwd
    for ws_bytes in (0, need - 1):
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=cuda)
        Y = torch.empty(N, F, device=cuda)
        with L.device_guard(cuda):
            rc = lib.mgcn_spmm_xw_fwd(N, v.n_cols, F, F, L.ptr(v.rowptr), L.ptr(v.col),
                                      L.ptr(c["norm"].w_fwd), L.ptr(c["X"]), F, L.ptr(c["W"]), F,
                                      L.ptr(c["b"]), L.ptr(Y), F, L.REDUCE_SUM, 0, None, None, 0,
                                      L.ptr(ws) if ws_bytes else None, ws_bytes,
                                      L.stream_of(cuda))
        L.check(rc, "mgcn_spmm_xw_fwd")
        assert torch.equal(Y, Y0)
    for bad in (-1, 65):
        with pytest.raises(L.MgcnError):
            L.set_option("xw_dyn_rounds", bad)


def test_stack_step_default_vs_static(cuda, dyn_rounds):
    """bench.build_stack's 3-layer step where the default claims the forward's
    tail (16 rounds + 15 rows): y and all six gradients bit for bit the static
    assignment's."""
    from bench import build_stack, make_inputs
    N = 16 * _grid() * R + 15
    ei = torch.from_numpy(_edges("rand", N))
    X, Ws, bs, dY = make_inputs(N, F, 3)
    out = {}
    for key, rounds in (("default", 8), ("static", 0)):
        dyn_rounds(rounds)
        step, params = build_stack(cuda, ei, X, Ws, bs, dY)
        y = step()
        out[key] = [y.detach().clone()] + [p.grad.clone() for p in params]
    assert len(out["default"]) == 7
    for a, b in zip(out["default"], out["static"]):
        assert torch.equal(a, b)
