"""bf16 feature rows on the GPU: mgcn_spmm_fwd_bf16 / mgcn_spmm_bwd_bf16 /
mgcn_relu_bwd_colsum_bf16 and everything mgcn.ops routes to them.

The reference of every op-level case is the existing fp32 path -- which the
other GPU tests pin bit for bit to the oracle -- run in the same process on
``H.float()`` / ``dZ.float()`` and rounded with ``.cpu().to(torch.bfloat16)``;
outputs are compared as bit patterns (``.view(torch.int16)``), no tolerance.
Inputs are standard-normal values rounded to bf16, so no fp32 result falls
below bf16's range and the ReLU masks of the two paths coincide.

Graph (a): tests/timer_names_cases.py's (N = 70, 300 random edges + loops:
three 32-row chunks, the last partial).  Graph (b): N = 1000, 3000 random
edges with duplicates among the first 980 nodes (20 isolated), plus nodes of
in-degree 300 and 700 and of out-degree 300 and 700: heavy (> 128 edges) and
giant (> 512) rows in both views."""
import functools

import numpy as np
import pytest
import torch

import timer_names_cases as tc

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
NB, ISOLATED = 1000, 20


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def same_bits(got, want32):
    """got (bf16, device) against the fp32 path's result rounded once."""
    assert got.dtype == BF16
    return torch.equal(bits(got), bits(want32.detach().cpu().to(BF16)))


@functools.lru_cache(maxsize=None)
def graph_np(which):
    if which == "a":
        return tc.edge_index(), tc.N
    rng = np.random.default_rng(11)
    live = NB - ISOLATED
    s, d = [rng.integers(0, live, 3000)], [rng.integers(0, live, 3000)]
    for node, deg, incoming in ((3, 300, True), (5, 700, True), (7, 300, False), (9, 700, False)):
        other = rng.integers(0, live, deg)
        hub = np.full(deg, node)
        s.append(other if incoming else hub)
        d.append(hub if incoming else other)
    return np.stack([np.concatenate(s), np.concatenate(d)]).astype(np.int64), NB


@functools.lru_cache(maxsize=None)
def graph(which):
    from mgcn.graph import plan_for
    ei, n = graph_np(which)
    ei = torch.from_numpy(ei).cuda()
    return ei, n, plan_for(ei, n)


@functools.lru_cache(maxsize=None)
def norm_of(which, norm_name):
    ei, n, plan = graph(which)
    if norm_name == "ew":  # edge weights under the symmetric norm
        g = torch.Generator().manual_seed(5)
        ew = (torch.rand(ei.size(1), generator=g) + 0.5).cuda()
        return plan.norm("sm", edge_weight=ew)
    return plan.norm(norm_name)


def rand_bf16(seed, *shape):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(BF16).cuda()


REDUCES = ("add", "mean", "max")
NORMS = (None, "sm", "rw", "ew")
WIDTHS = (8, 24, 128, 136, 512)
GRID = [(w, r, nm, epi, F) for w in "ab" for r in REDUCES for nm in NORMS for epi in (False, True)
        for F in WIDTHS]


def grid_id(c):
    return "{}-{}-{}-{}-F{}".format(c[0], c[1], c[2], "epi" if c[3] else "plain", c[4])


@functools.lru_cache(maxsize=None)
def inputs(which, epi, F):
    _, n, _ = graph(which)
    H = rand_bf16(100 + F, n, F)
    dZ = rand_bf16(200 + F, n, F)
    bias = rand_bf16(300 + F, F).float() * 0.5 if epi else None  # fp32 bias
    return H, dZ, bias


def test_graph_b_has_heavy_and_giant_rows_in_both_views(cuda):
    _, _, plan = graph("b")
    for view in (plan.fwd, plan.bwd):
        assert view.order is not None and view.n_heavy >= 2 and view.n_giant >= 1
    deg = plan.fwd.rowptr[1:] - plan.fwd.rowptr[:-1]
    assert int((deg == 0).sum()) >= ISOLATED


@pytest.mark.parametrize("case", GRID, ids=grid_id)
def test_forward_bits(cuda, case):
    """Y, and for max the winner bits (the mask aggregate_plan keeps) and the
    argmax (what scatter_ keeps), against the fp32 kernels on the upcast rows."""
    from mgcn import _lib as L
    from mgcn import ops
    which, aggr, norm_name, epi, F = case
    _, n, plan = graph(which)
    norm = norm_of(which, norm_name)
    H, _, bias = inputs(which, epi, F)
    reduce = L.REDUCE_CODES[aggr]
    Y32, m32 = ops.spmm_fwd(plan.fwd, norm.w_fwd, H.float(), reduce, bias, epi, mask_plan=plan)
    Y, m = ops.spmm_fwd_bf16(plan.fwd, norm.w_fwd, H, reduce, bias, epi, mask_plan=plan)
    assert same_bits(Y, Y32)
    if aggr == "max":
        assert m.dtype == torch.int32 and torch.equal(m.cpu(), m32.cpu())
        Y32b, a32 = ops.spmm_fwd(plan.fwd, norm.w_fwd, H.float(), reduce, bias, epi)
        Yb, a = ops.spmm_fwd_bf16(plan.fwd, norm.w_fwd, H, reduce, bias, epi)
        assert torch.equal(a.cpu(), a32.cpu()) and same_bits(Yb, Y32b)
    else:
        assert m is None
    if aggr != "add" and not epi:  # empty rows: 0 for max and for mean
        deg = (plan.fwd.rowptr[1:] - plan.fwd.rowptr[:-1]).cpu()
        assert torch.count_nonzero(Y.cpu().float()[deg == 0]) == 0
    # the public entry point takes the same launch
    assert same_bits(ops.aggregate_plan(H, plan, norm, aggr, bias, epi), Y32)


def run_backward(fn, x, dZ, params):
    x = x.detach().clone().requires_grad_(True)
    ps = [p.detach().clone().requires_grad_(True) if p is not None else None for p in params]
    fn(x, *ps).backward(dZ)
    return x.grad, [p.grad if p is not None else None for p in ps]


@pytest.mark.parametrize("case", GRID, ids=grid_id)
def test_adjoint_bits_db_bound_and_determinism(cuda, case):
    from mgcn import ops
    which, aggr, norm_name, epi, F = case
    _, n, plan = graph(which)
    norm = norm_of(which, norm_name)
    H, dZ, bias = inputs(which, epi, F)

    def f(h, b):
        return ops.aggregate_plan(h, plan, norm, aggr, b, epi)

    dH32, _ = run_backward(f, H.float(), dZ.float(), [bias])
    dH, (db,) = run_backward(f, H, dZ, [bias])
    assert same_bits(dH, dH32)
    dH2, (db2,) = run_backward(f, H, dZ, [bias])
    assert torch.equal(bits(dH), bits(dH2))
    if epi:
        assert db.dtype == torch.float32 and torch.equal(db, db2)
        # fp32 summation of n_rows terms, any order:
        # |db - db64| <= n_rows 2^-24 sum_i |dY[i, f]|
        Y = f(H, bias).detach()
        dY64 = torch.where(Y > 0, dZ.double(), torch.zeros((), dtype=torch.float64, device=cuda))
        err = (db.double() - dY64.sum(0)).abs()
        bound = n * 2.0 ** -24 * dY64.abs().sum(0)
        assert bool((err <= bound).all()), f"db: worst err/bound {(err / bound).max().item():.3f}"


@pytest.mark.parametrize("aggr", REDUCES)
@pytest.mark.parametrize("which", "ab")
def test_scatter_bits(cuda, which, aggr):
    """scatter_ on an explicit [E, F] bf16 src: forward, and the adjoint
    through the saved argmax / the counts."""
    from mgcn import ops
    ei, n, _ = graph(which)
    E, F = ei.size(1), 24
    src, dZ = rand_bf16(41, E, F), rand_bf16(42, n, F)
    index = ei[1].contiguous()

    def f(s):
        return ops.scatter_(aggr, s, index, n)

    y32 = f(src.float())
    assert same_bits(f(src), y32)
    g32, _ = run_backward(f, src.float(), dZ.float(), [])
    g, _ = run_backward(f, src, dZ, [])
    assert same_bits(g, g32)


@pytest.mark.parametrize("aggr", REDUCES)
def test_layouts_aligned_view_in_place_misaligned_copied(cuda, aggr):
    from mgcn import ops
    _, n, plan = graph("a")
    norm = norm_of("a", "sm")
    F = 128
    wide = rand_bf16(7, n, F + 32)
    for off, copies in ((16, 0), (4, 1)):
        H = wide[:, off:off + F]
        assert (H.data_ptr() % 16 == 0) == (copies == 0) and H.stride(0) == F + 32
        before = ops.ROW_COPIES["H"]
        y = ops.aggregate_plan(H, plan, norm, aggr)
        assert ops.ROW_COPIES["H"] - before == copies
        assert same_bits(y, ops.aggregate_plan(H.float(), plan, norm, aggr))


@pytest.mark.parametrize("aggr", REDUCES)
def test_fallback_f7_and_1d_scatter(cuda, aggr):
    """Shapes the kernels do not take: upcast -> fp32 path -> round; no bf16 launch."""
    from mgcn import ops
    ei, n, plan = graph("a")
    norm = norm_of("a", "sm")
    names = []
    ops.set_kernel_timer(lambda name, start, rows=None, edges=None: names.append(name))
    try:
        H, dZ = rand_bf16(1, n, 7), rand_bf16(2, n, 7)
        bias = rand_bf16(3, 7).float()

        def f(h, b):
            return ops.aggregate_plan(h, plan, norm, aggr, b, True)

        assert same_bits(f(H, bias), f(H.float(), bias))
        dH32, _ = run_backward(f, H.float(), dZ.float(), [bias])
        dH, (db,) = run_backward(f, H, dZ, [bias])
        assert same_bits(dH, dH32) and db.dtype == torch.float32
        src, index = rand_bf16(4, ei.size(1)), ei[1].contiguous()
        y = ops.scatter_(aggr, src, index, n)
        assert y.dim() == 1 and same_bits(y, ops.scatter_(aggr, src.float(), index, n))
    finally:
        ops.set_kernel_timer(None)
    assert names and not [nm for nm in names if nm.endswith("_bf16")]


@pytest.mark.parametrize("aggr", REDUCES)
def test_fallback_differentiable_edge_weight(cuda, aggr):
    from mgcn import ops
    ei, n, plan = graph("a")
    F = 24
    H, dZ = rand_bf16(1, n, F), rand_bf16(2, n, F)
    g = torch.Generator().manual_seed(9)
    ew0 = (torch.rand(ei.size(1), generator=g) + 0.5).cuda()

    def run(h, dz):
        ew = ew0.clone().requires_grad_(True)
        h = h.clone().requires_grad_(True)
        norm = plan.norm("sm", edge_weight=ew)
        assert norm.grad
        y = ops.aggregate_plan(h, plan, norm, aggr)
        y.backward(dz)
        return y, h.grad, ew.grad

    y32, dh32, dw32 = run(H.float(), dZ.float())
    y, dh, dw = run(H, dZ)
    assert same_bits(y, y32) and same_bits(dh, dh32)
    assert dw.dtype == torch.float32 and torch.equal(dw, dw32)


# ------------------------------------------------------------ layers, modules
def dense_norm(plan, norm, n):
    """(A, |A|) in fp64 from the fwd view's slots: A[row, col] += w."""
    v = plan.fwd
    deg = v.rowptr[1:] - v.rowptr[:-1]
    rows = torch.repeat_interleave(torch.arange(n, device=deg.device), deg)
    cols = v.col.long()
    w = (norm.w_fwd if norm.w_fwd is not None else torch.ones(cols.numel(), device=deg.device))
    w = w.detach().double()
    A = torch.zeros(n, n, dtype=torch.float64, device=deg.device)
    return (A.index_put((rows, cols), w, accumulate=True),
            A.index_put((rows, cols), w.abs(), accumulate=True))


def bf16_valued_(module):
    """Round every parameter to a bf16 value in place (kept fp32): the fp32
    master weights and their bf16 casts are then the same numbers."""
    g = torch.Generator().manual_seed(21)
    with torch.no_grad():
        for p in module.parameters():
            if p.dim() == 1:  # biases start at zero
                p.copy_(torch.randn(p.shape, generator=g) * 0.5)
            p.copy_(p.to(BF16).float())
    return module


def check_layer(y, x, W, b, A, Aabs, relu=False):
    """|y - y64| <= 3 2^-9 (|A| |H64| + |b|), H64 = X64 W64 and y64 in fp64
    from the bf16-valued operands: one rounding of h and one of y, each 2^-9
    relative, give 2^-9 (2 |A||H| + |b|) to first order; the 3 covers the
    second-order terms and the fp32 accumulation.  ReLU is 1-Lipschitz.

    Measured on the seeded modules below (torch.manual_seed(0), chosen before
    any run): worst err / bound 0.89 (gcn_layer), 0.85 (NodeModelAdditive),
    0.58 (GCNConv), the same with fp32 master weights and after
    .to(torch.bfloat16).  The bound is not a worst-case one: one bf16 rounding
    is up to 2^-8 relative, not 2^-9, so a row with a single dominant edge can
    reach 4/3 of it; an unseeded NodeModelAdditive initialisation measured
    1.005 once."""
    assert y.dtype == BF16
    H64 = x.double() @ W.detach().double()
    b64 = b.detach().double() if b is not None else torch.zeros((), dtype=torch.float64,
                                                                 device=x.device)
    y64 = A @ H64 + b64
    if relu:
        y64 = y64.clamp_min(0)
    bound = 3 * 2.0 ** -9 * (Aabs @ H64.abs() + b64.abs())
    err = (y.double() - y64).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"layer: worst err/bound {worst:.3f}")
    assert bool((err <= bound).all()), f"worst err/bound {worst:.3f}"


def layer_cases():
    from mgcn import ops, pyg
    from mgcn.graph import plan_for
    from mgcn.models import NodeModelAdditive
    ei, n, plan = graph("a")
    torch.manual_seed(0)  # the modules' own initialisation draws from the global generator

    def gcn_layer_case():
        lin = bf16_valued_(torch.nn.Linear(128, 128)).cuda()  # holder of W [in, out] and b
        norm = plan.norm("sm")
        return (lin, lambda x: ops.gcn_layer(x, lin.weight, plan, norm, "add", lin.bias, True),
                lin.weight, lin.bias, plan, norm, 128, True)

    def additive_case():
        nm = bf16_valued_(NodeModelAdditive(128, 128)).cuda()
        return nm, lambda x: nm(x, ei), nm.weight_node, nm.bias, plan, plan.norm("sm"), 128, False

    def gcnconv_case():
        conv = bf16_valued_(pyg.GCNConv(24, 8)).cuda()
        ei2, ew2 = pyg._with_loops(ei, torch.ones(ei.size(1), device=ei.device), n, 1)
        plan2 = plan_for(ei2, n)
        return (conv, lambda x: conv(x, ei), conv.weight, conv.bias, plan2,
                plan2.norm("sm", edge_weight=ew2), 24, False)

    return {"gcn_layer": gcn_layer_case, "NodeModelAdditive": additive_case,
            "GCNConv": gcnconv_case}


@pytest.mark.parametrize("converted", (False, True), ids=("fp32_master", "to_bf16"))
@pytest.mark.parametrize("name", ("gcn_layer", "NodeModelAdditive", "GCNConv"))
def test_layer_on_bf16_input(cuda, name, converted):
    _, n, _ = graph("a")
    module, fwd, W, b, plan, norm, f_in, relu = layer_cases()[name]()
    W64, b64 = W.detach().clone(), b.detach().clone()
    if converted:
        module.to(BF16)
    pdt = BF16 if converted else torch.float32
    A, Aabs = dense_norm(plan, norm, n)
    x = rand_bf16(31, n, f_in).requires_grad_(True)
    y = fwd(x)
    check_layer(y, x.detach(), W64, b64, A, Aabs, relu)
    y.backward(rand_bf16(32, *y.shape))
    assert x.grad.dtype == BF16 and bool(torch.isfinite(x.grad.float()).all())
    for p in module.parameters():
        assert p.dtype == pdt and p.grad is not None and p.grad.dtype == pdt
        assert bool(torch.isfinite(p.grad.float()).all())
        assert float(p.grad.float().abs().sum()) > 0


def record_names(fn):
    from mgcn import ops
    names = []
    ops.set_kernel_timer(lambda name, start, rows=None, edges=None: names.append(name))
    try:
        fn()
    finally:
        ops.set_kernel_timer(None)
    return names


def stack_and_model():
    from mgcn.models import GCNLayer, GCNModel, GCNStack
    torch.manual_seed(3)
    stack = GCNStack([GCNLayer(128, 128), GCNLayer(128, 128),
                      GCNLayer(128, 128, non_linear="none")]).cuda()
    model = GCNModel(32, [32, 32, 32], 4, residual_hop=1, dropout=0, final_type="proj").cuda()
    return stack, model


def fused(names):
    return [nm for nm in names if nm.startswith("spmm_xw_") or nm.startswith("residual_")]


def run_stack_and_model(dtype):
    ei, n, _ = graph("a")
    stack, model = stack_and_model()
    out = {}
    for key, mod, f_in in (("stack", stack, 128), ("model", model, 32)):
        x = rand_bf16(51, n, f_in).to(dtype).requires_grad_(True)

        def step():
            y = mod(x, ei)
            assert y.dtype == dtype
            y.backward(rand_bf16(52, *y.shape).to(dtype))

        out[key] = record_names(step)
        assert x.grad.dtype == dtype and bool(torch.isfinite(x.grad.float()).all())
        for p in mod.parameters():
            assert p.grad is not None and p.grad.dtype == torch.float32
            assert bool(torch.isfinite(p.grad).all())
    return out


def test_stack_and_model_go_layer_by_layer_on_bf16(cuda):
    names = run_stack_and_model(BF16)
    for key in ("stack", "model"):
        assert not fused(names[key]), names[key]
        assert "spmm_fwd_bf16" in names[key] and "spmm_bwd_bf16" in names[key]
        assert "relu_bwd_colsum_bf16" in names[key]  # the ReLU folded into the bf16 epilogue


def test_fp32_calls_record_no_bf16_launch(cuda):
    """The same calls with fp32 input: the launches they took before (the
    fused layer kernels among them), no *_bf16 one."""
    from mgcn import ops
    names = run_stack_and_model(torch.float32)
    assert fused(names["stack"]) and fused(names["model"])
    _, n, plan = graph("b")
    norm = norm_of("b", "sm")
    H, dZ, bias = inputs("b", True, 128)

    def op_level():
        for aggr in REDUCES:
            run_backward(lambda h, b: ops.aggregate_plan(h, plan, norm, aggr, b, True),
                         H.float(), dZ.float(), [bias])
        ei = graph("b")[0]
        ops.scatter_("max", rand_bf16(1, ei.size(1), 24).float(), ei[1].contiguous(), n)

    names = names["stack"] + names["model"] + record_names(op_level)
    assert "spmm_fwd" in names and "spmm_bwd" in names
    assert not [nm for nm in names if nm.endswith("_bf16")]
