"""The fused bf16 layer kernel (csrc/fused_bf16.hip, mgcn_spmm_xw_bf16) and the
opt-in route ``ops.gcn_layer`` takes to it (``ops.set_bf16_fused_layers``).

References: the project's pinned bf16 aggregation kernels (``spmm_fwd_bf16`` /
``spmm_bwd_bf16`` / ``relu_bwd_colsum_bf16``, tests/test_gpu_bf16.py) and fp64
arithmetic on their results; the kernel under test is never a reference.

Graph (c): tests/timer_names_cases.py's (N = 70: three 32-row chunks, the last
partial) plus a node with 40 extra in-edges and one with 40 extra out-edges
(rows of more than two 16-edge metadata windows, the last one ragged) and 5
appended isolated nodes, N = 75.  Graph (d): N = 5, one partial chunk.  Graph
(e): N = 20,011, 100,000 random edges plus loops -- 626 chunks, more than the
2 x 256 persistent workgroups, so workgroups take a second chunk and write a
staged tile out beside its gathers.

The bound of the general-W cases, elementwise, with y64 in fp64 from the bf16
operands:
    |y - y64| <= 2^-8 |y64| + (1 + 2^-8) 130 2^-23 (|Zref| @ |Wb| + |b|)
-- bf16's unit roundoff on the one store, and 128 fp32 additions plus the bias,
in any order, at one unit in the last place each (every product is exact);
ReLU is 1-Lipschitz."""
import functools

import numpy as np
import pytest
import torch

import timer_names_cases as tc

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
F = 128
NC, ND, NE = tc.N + 5, 5, 20011
NORMS = (None, "sm", "rw", "ew")
AGGRS = ("add", "mean")


def bits(t):
    assert t.dtype == BF16
    return t.detach().cpu().contiguous().view(torch.int16)


def rand_bf16(seed, *shape):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(BF16).cuda()


@functools.lru_cache(maxsize=None)
def graph_np(which):
    if which == "c":
        rng = np.random.default_rng(23)
        base = tc.edge_index()
        others_in, others_out = rng.integers(0, tc.N, 40), rng.integers(0, tc.N, 40)
        s = np.concatenate([base[0], others_in, np.full(40, 11)])
        d = np.concatenate([base[1], np.full(40, 4), others_out])
        return np.stack([s, d]).astype(np.int64), NC
    if which == "d":
        rng = np.random.default_rng(29)
        s, d = rng.integers(0, ND, 12), rng.integers(0, ND, 12)
        loops = np.arange(ND)
        return np.stack([np.concatenate([s, loops]), np.concatenate([d, loops])]).astype(np.int64), ND
    rng = np.random.default_rng(31)
    s, d = rng.integers(0, NE, 100000), rng.integers(0, NE, 100000)
    loops = np.arange(NE)
    return np.stack([np.concatenate([s, loops]), np.concatenate([d, loops])]).astype(np.int64), NE


@functools.lru_cache(maxsize=None)
def graph(which):
    from mgcn.graph import plan_for
    ei, n = graph_np(which)
    ei = torch.from_numpy(ei).cuda()
    return ei, n, plan_for(ei, n)


@functools.lru_cache(maxsize=None)
def norm_of(which, norm_name):
    ei, n, plan = graph(which)
    if norm_name == "ew":  # seeded edge weights under the symmetric norm
        g = torch.Generator().manual_seed(5)
        ew = (torch.rand(ei.size(1), generator=g) + 0.5).cuda()
        return plan.norm("sm", edge_weight=ew)
    return plan.norm(norm_name)


@functools.lru_cache(maxsize=None)
def inputs(which):
    """(X, dY, Wb, bias): standard-normal values rounded to bf16; the bias
    fp32 with bf16 values."""
    _, n, _ = graph(which)
    return (rand_bf16(101, n, F), rand_bf16(102, n, F), rand_bf16(103, F, F),
            rand_bf16(104, F).float())


@functools.lru_cache(maxsize=None)
def z_ref(which, norm_name, aggr):
    """The pinned forward kernel's bf16 aggregate of X (computed once)."""
    from mgcn import _lib as L
    from mgcn import ops
    _, _, plan = graph(which)
    X = inputs(which)[0]
    return ops.spmm_fwd_bf16(plan.fwd, norm_of(which, norm_name).w_fwd, X, L.REDUCE_CODES[aggr])[0]


@functools.lru_cache(maxsize=None)
def dh_ref(which, norm_name, aggr):
    """The pinned adjoint kernel's bf16 aggregate of dY (computed once)."""
    from mgcn import _lib as L
    from mgcn import ops
    _, _, plan = graph(which)
    norm = norm_of(which, norm_name)
    dY = inputs(which)[1]
    return ops.spmm_bwd_bf16(plan.bwd, norm.w_bwd, norm.row_scale_bwd, dY, L.REDUCE_CODES[aggr],
                             cnt=plan.in_cnt if aggr == "mean" else None)


def adjoint(which, norm_name, aggr, dY, B):
    from mgcn import ops
    _, _, plan = graph(which)
    norm = norm_of(which, norm_name)
    return ops.spmm_xw_bwd_bf16(plan.bwd, norm.w_bwd, norm.row_scale_bwd, dY, B,
                                cnt=plan.in_cnt if aggr == "mean" else None)


def eye():
    return torch.eye(F, dtype=BF16, device="cuda")


def check_bound(what, y, zref, Wb, bias=None, relu=False):
    """The module docstring's bound; zref @ Wb in fp64 is the reference."""
    assert y.dtype == BF16
    z64, w64 = zref.double(), Wb.double()
    b64 = bias.double() if bias is not None else torch.zeros((), dtype=torch.float64,
                                                             device=y.device)
    y64 = z64 @ w64 + b64
    if relu:
        y64 = y64.clamp_min(0)
    bound = 2.0 ** -8 * y64.abs() + (1 + 2.0 ** -8) * 130 * 2.0 ** -23 * (z64.abs() @ w64.abs()
                                                                          + b64.abs())
    err = (y.double() - y64).abs()
    ok = err <= bound
    worst = (err / bound.clamp_min(1e-300))[bound > 0].max().item() if bool((bound > 0).any()) else 0.0
    print(f"{what}: worst err/bound {worst:.3f}")
    assert bool(ok.all()), f"{what}: worst err/bound {worst:.3f}"


def record_names(fn):
    """The timer names of the launches fn() makes, one per launch."""
    from mgcn import ops
    names = []
    ops.set_kernel_timer(lambda name, start, rows=None, edges=None: start and names.append(name))
    try:
        fn()
    finally:
        ops.set_kernel_timer(None)
    return names


def _switched(value):
    from mgcn import ops
    before = ops._BF16_FUSED
    ops.set_bf16_fused_layers(value)
    try:
        yield
    finally:
        ops.set_bf16_fused_layers(before)


@pytest.fixture
def switch_on():
    yield from _switched(True)


@pytest.fixture
def switch_off():
    yield from _switched(False)


def xw_names(names):
    return [nm for nm in names if nm.startswith("spmm_xw_") and nm.endswith("_bf16")]


# ------------------------------------------------------------------ the graphs
def test_graphs_have_the_shapes_the_cases_need(cuda):
    _, n, plan = graph("c")
    assert n == 75
    for view in (plan.fwd, plan.bwd):
        deg = view.rowptr[1:] - view.rowptr[:-1]
        assert view.n_heavy == 0 and int(deg.max()) >= 33 and int((deg == 0).sum()) >= 5
    _, n, plan = graph("d")
    assert n == 5 and plan.fwd.n_heavy == plan.bwd.n_heavy == 0
    _, n, plan = graph("e")
    assert (n + 31) // 32 == 626 and plan.fwd.n_heavy == plan.bwd.n_heavy == 0


# ---------------------------------------------------------------- 1. the Z bits
@pytest.mark.parametrize("aggr", AGGRS)
@pytest.mark.parametrize("norm_name", NORMS, ids=str)
@pytest.mark.parametrize("which", "cde")
def test_z_bits_forward_and_adjoint(cuda, which, norm_name, aggr):
    from mgcn import _lib as L
    from mgcn import ops
    _, _, plan = graph(which)
    norm = norm_of(which, norm_name)
    X, dY, Wb, _ = inputs(which)
    _, Z = ops.spmm_xw_fwd_bf16(plan.fwd, norm.w_fwd, X, Wb, L.REDUCE_CODES[aggr], want_z=True)
    assert torch.equal(bits(Z), bits(z_ref(which, norm_name, aggr)))
    # adjoint with B = I: the rounded aggregate itself (row_scale under 'rw', cnt under mean)
    dX = adjoint(which, norm_name, aggr, dY, eye())
    assert torch.equal(bits(dX), bits(dh_ref(which, norm_name, aggr)))


# ------------------------------------------------------------ 2. exact products
@pytest.mark.parametrize("aggr", AGGRS)
@pytest.mark.parametrize("which", "cde")
def test_identity_w_returns_z(cuda, which, aggr):
    from mgcn import _lib as L
    from mgcn import ops
    _, _, plan = graph(which)
    Y = ops.spmm_xw_fwd_bf16(plan.fwd, norm_of(which, "sm").w_fwd, inputs(which)[0], eye(),
                             L.REDUCE_CODES[aggr])
    assert torch.equal(bits(Y), bits(z_ref(which, "sm", aggr)))


@pytest.mark.parametrize("transpose", (False, True), ids=("B", "Bt"))
@pytest.mark.parametrize("which", "cde")
def test_signed_scaled_permutation_is_exact(cuda, which, transpose):
    """W = a signed permutation of the columns scaled by powers of two: every
    output is one exact product plus the bias, so the bits are those of torch's
    fp32 arithmetic on the pinned Z -- row, column and k-block placement with
    no tolerance, for both settings of the transpose flag."""
    from mgcn import _lib as L
    from mgcn import ops
    _, _, plan = graph(which)
    g = torch.Generator().manual_seed(61)
    perm = torch.randperm(F, generator=g)
    s = (2.0 ** torch.randint(-3, 4, (F,), generator=g).float()) * \
        (1 - 2 * torch.randint(0, 2, (F,), generator=g).float())
    W = torch.zeros(F, F)
    W[perm, torch.arange(F)] = s  # Y[:, n] = Z[:, perm[n]] * s[n]
    W = W.to(BF16).cuda()
    X, _, _, bias = inputs(which)
    zref = z_ref(which, "sm", "add")
    want = torch.relu(zref.float()[:, perm.cuda()] * s.cuda() + bias).to(BF16)
    B = W.t().contiguous() if transpose else W
    Y, _ = ops.spmm_xw_bf16(plan.fwd, norm_of(which, "sm").w_fwd, None, None, X, B, transpose,
                            bias, True, L.REDUCE_SUM, False)
    assert torch.equal(bits(Y), bits(want))


# ------------------------------------------------- 3. general W against fp64
@pytest.mark.parametrize("norm_name,aggr", (("sm", "add"), ("ew", "mean")))
@pytest.mark.parametrize("which", "cde")
def test_forward_general_w_within_the_derived_bound(cuda, which, norm_name, aggr):
    from mgcn import _lib as L
    from mgcn import ops
    _, _, plan = graph(which)
    X, _, Wb, bias = inputs(which)
    Y = ops.spmm_xw_fwd_bf16(plan.fwd, norm_of(which, norm_name).w_fwd, X, Wb,
                             L.REDUCE_CODES[aggr], bias, True)
    check_bound(f"fwd {which} {norm_name} {aggr}", Y, z_ref(which, norm_name, aggr), Wb, bias, True)


@pytest.mark.parametrize("norm_name,aggr", (("sm", "add"), ("rw", "add"), ("ew", "mean")))
@pytest.mark.parametrize("which", "ce")
def test_adjoint_general_w_within_the_derived_bound(cuda, which, norm_name, aggr):
    _, dY, Wb, _ = inputs(which)
    dX = adjoint(which, norm_name, aggr, dY, Wb)
    check_bound(f"adjoint {which} {norm_name} {aggr}", dX, dh_ref(which, norm_name, aggr),
                Wb.t())


# --------------------------------------------------------------- 4. layouts
def test_layouts_aligned_view_in_place_misaligned_copied(cuda):
    from mgcn import _lib as L
    from mgcn import ops
    _, n, plan = graph("c")
    w = norm_of("c", "sm").w_fwd
    X, _, Wb, bias = inputs("c")
    want = ops.spmm_xw_fwd_bf16(plan.fwd, w, X, Wb, L.REDUCE_SUM, bias, True)
    wide = torch.zeros(n, F + 8, dtype=BF16, device="cuda")
    for off, copies in ((0, 0), (8, 0), (3, 1)):  # 0 / 16 / 6 bytes into a 272-byte row
        view = wide[:, off:off + F]
        view.copy_(X)
        assert view.stride(0) == 136 and (view.data_ptr() % 16 == 0) == (copies == 0)
        before = ops.ROW_COPIES["X"]
        got = ops.spmm_xw_fwd_bf16(plan.fwd, w, view, Wb, L.REDUCE_SUM, bias, True)
        assert ops.ROW_COPIES["X"] - before == copies
        assert torch.equal(bits(got), bits(want))


# --------------------------------------------------------------- 5. autograd
@pytest.mark.parametrize("relu", (False, True), ids=("plain", "relu"))
@pytest.mark.parametrize("aggr", AGGRS)
def test_autograd_through_gcn_layer(cuda, switch_on, aggr, relu):
    from mgcn import _lib as L
    from mgcn import ops
    _, n, plan = graph("c")
    norm = norm_of("c", "sm")
    reduce = L.REDUCE_CODES[aggr]
    cnt = plan.in_cnt if aggr == "mean" else None
    X, dZ, Wb, bias = inputs("c")
    x = X.clone().requires_grad_(True)
    W = Wb.float().requires_grad_(True)  # fp32 masters with bf16 values
    b = bias.clone().requires_grad_(True)
    out = {}

    def step():
        out["y"] = ops.gcn_layer(x, W, plan, norm, aggr, b, relu)
        out["y"].backward(dZ)

    names = record_names(step)
    assert names == ["spmm_xw_fwd_z_bf16", "relu_bwd_colsum_bf16", "spmm_xw_bwd_bf16"]
    y = out["y"].detach()
    check_bound(f"layer {aggr}", y, z_ref("c", "sm", aggr), Wb, bias, relu)

    dY = torch.where(y > 0, dZ, torch.zeros_like(dZ)) if relu else dZ
    direct = ops.spmm_xw_bwd_bf16(plan.bwd, norm.w_bwd, norm.row_scale_bwd, dY, Wb, cnt=cnt)
    assert x.grad.dtype == BF16 and torch.equal(bits(x.grad), bits(direct))
    dh = ops.spmm_bwd_bf16(plan.bwd, norm.w_bwd, norm.row_scale_bwd, dY, reduce, cnt=cnt)
    check_bound(f"layer dx {aggr}", direct, dh, Wb.t())

    _, Z = ops.spmm_xw_fwd_bf16(plan.fwd, norm.w_fwd, X, Wb, reduce, want_z=True)
    assert W.grad.dtype == torch.float32
    dW64 = Z.double().t() @ dY.double()
    bound = 2.0 ** -8 * dW64.abs() + (n + 2) * 2.0 ** -23 * (Z.double().abs().t() @ dY.double().abs())
    err = (W.grad.double() - dW64).abs()
    print(f"dW {aggr}: worst err/bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert bool((err <= bound).all())

    _, db = ops.relu_bwd_colsum_bf16(dZ, y, relu, True)
    assert b.grad.dtype == torch.float32 and torch.equal(b.grad, db)

    with torch.no_grad():
        names = record_names(lambda: ops.gcn_layer(x, W, plan, norm, aggr, b, relu))
    assert names == ["spmm_xw_fwd_bf16"]


# ---------------------------------------------------------------- 6. routing
def layer_names(plan, norm, x, W, b, aggr="add"):
    from mgcn import ops

    def step():
        xx = x.detach().clone().requires_grad_(True)
        ww = W.detach().clone().requires_grad_(True)
        y = ops.gcn_layer(xx, ww, plan, norm, aggr, b, True)
        y.backward(torch.ones_like(y))

    return record_names(step)


def test_routes_the_fused_kernel_does_not_take(cuda, switch_on):
    import test_gpu_bf16 as tb
    ei, n, plan = graph("c")
    norm = norm_of("c", "sm")
    X, _, Wb, bias = inputs("c")
    W = Wb.float()
    # 24 -> 8
    names = layer_names(plan, norm, rand_bf16(1, n, 24), rand_bf16(2, 24, 8).float(), None)
    assert "spmm_fwd_bf16" in names and not xw_names(names)
    # max does not commute with W
    names = layer_names(plan, norm, X, W, bias, "max")
    assert "spmm_fwd_bf16" in names and not xw_names(names)
    # heavy rows (graph (b) of tests/test_gpu_bf16.py)
    _, nb, plan_b = tb.graph("b")
    assert plan_b.fwd.n_heavy > 0
    names = layer_names(plan_b, plan_b.norm("sm"), rand_bf16(3, nb, F), W, bias)
    assert "spmm_fwd_bf16" in names and not xw_names(names)
    # a differentiable edge weight keeps today's path
    g = torch.Generator().manual_seed(9)
    ew = (torch.rand(ei.size(1), generator=g) + 0.5).cuda().requires_grad_(True)
    gnorm = plan.norm("sm", edge_weight=ew)
    assert gnorm.grad
    names = layer_names(plan, gnorm, X, W, bias)
    assert names and not xw_names(names)
    assert ew.grad is not None
    # fp32 input: the fp32 fused kernels
    names = layer_names(plan, norm, X.float(), W, bias)
    assert [nm for nm in names if nm.startswith("spmm_xw_fwd")]
    assert not [nm for nm in names if nm.endswith("_bf16")]


def test_switch_off_keeps_todays_launches(cuda, switch_off):
    _, _, plan = graph("c")
    X, _, Wb, bias = inputs("c")
    names = layer_names(plan, norm_of("c", "sm"), X, Wb.float(), bias)
    assert "spmm_fwd_bf16" in names and "spmm_bwd_bf16" in names
    assert not [nm for nm in names if nm.startswith("spmm_xw_")]


def test_stack_of_three_layers_takes_the_fused_route(cuda, switch_on):
    from mgcn.models import GCNLayer, GCNStack
    ei, n, _ = graph("c")
    torch.manual_seed(3)
    stack = GCNStack([GCNLayer(F, F), GCNLayer(F, F), GCNLayer(F, F, non_linear="none")]).cuda()
    x = rand_bf16(51, n, F).requires_grad_(True)

    def step():
        y = stack(x, ei)
        assert y.dtype == BF16
        y.backward(rand_bf16(52, n, F))

    names = record_names(step)
    assert len([nm for nm in names if nm.startswith("spmm_xw_fwd") and nm.endswith("_bf16")]) == 3
    assert names.count("spmm_xw_bwd_bf16") == 3
    assert x.grad.dtype == BF16 and bool(torch.isfinite(x.grad.float()).all())
    for p in stack.parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32
        assert bool(torch.isfinite(p.grad).all())


# -------------------------------------------- 7. determinism, argument checks
def test_two_launches_give_equal_bits(cuda):
    from mgcn import _lib as L
    from mgcn import ops
    _, _, plan = graph("e")
    X, dY, Wb, bias = inputs("e")
    w = norm_of("e", "sm").w_fwd
    a = ops.spmm_xw_fwd_bf16(plan.fwd, w, X, Wb, L.REDUCE_SUM, bias, True)
    b = ops.spmm_xw_fwd_bf16(plan.fwd, w, X, Wb, L.REDUCE_SUM, bias, True)
    assert torch.equal(bits(a), bits(b))
    a, b = adjoint("e", "sm", "add", dY, Wb), adjoint("e", "sm", "add", dY, Wb)
    assert torch.equal(bits(a), bits(b))


def test_supported_probe_and_argument_checks(cuda):
    import mgcn
    from mgcn import _lib as L
    from mgcn import ops
    lib = mgcn.load()
    for fi in (64, 128, 256):
        for fo in (64, 128, 256):
            for reduce in (L.REDUCE_SUM, L.REDUCE_MEAN, L.REDUCE_MAX):
                want = fi == fo == 128 and reduce != L.REDUCE_MAX
                assert bool(lib.mgcn_spmm_xw_bf16_supported(fi, fo, reduce)) == want
    _, n, plan = graph("d")
    v = plan.fwd
    assert ops.spmm_xw_bf16_supported(v, 128, 128, L.REDUCE_SUM)
    assert ops.spmm_xw_bf16_supported(v, 128, 128, L.REDUCE_MEAN, ld=136)
    assert not ops.spmm_xw_bf16_supported(v, 128, 128, L.REDUCE_SUM, ld=132)
    assert not ops.spmm_xw_bf16_supported(v, 64, 64, L.REDUCE_SUM)
    X = torch.zeros(n, 136, dtype=BF16, device="cuda")
    Y = torch.zeros(n, 136, dtype=BF16, device="cuda")
    Wb = inputs("d")[2]
    cnt = plan.in_cnt

    def call(n_rows=n, f=128, ldx=136, reduce=L.REDUCE_SUM, cnt=None):
        return lib.mgcn_spmm_xw_bf16(n_rows, f, f, L.ptr(v.rowptr), L.ptr(v.col), None, None,
                                     L.ptr(cnt), L.ptr(X), ldx, L.ptr(Wb), 128, 0, None, 0,
                                     L.ptr(Y), 136, None, 0, reduce, L.stream_of(X.device))

    assert call(f=64) == L.EINVAL and b"unsupported" in lib.mgcn_last_error()
    assert call(ldx=132) == L.EINVAL and b"16-byte aligned" in lib.mgcn_last_error()
    assert call(reduce=L.REDUCE_MEAN, cnt=cnt) == L.EINVAL and b"cnt" in lib.mgcn_last_error()
    assert call(n_rows=0) == L.OK
    assert call() == L.OK
    torch.cuda.synchronize()
