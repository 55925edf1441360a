"""GPU tests of the fused multi-kernel layer (csrc/multi_kernel.hip,
mgcn/ops_multi.py, GCNMultiKernel's route).

Against the reference (fixtures mk_*.npz) and, for the route and ReLU cases,
the restatement of multi_kernel_ref, every tensor within

    max|t_gpu - t64| <= max(4 * max|t32 - t64|, 1e-5 * max|t64|)

The two entry points are compared bit for bit (torch.equal) with K
mgcn_spmm_fwd / mgcn_spmm_bwd calls on the column-block views, combined by
torch in kernel order.  The combine mean divides by a device tensor: torch
turns a division by a Python scalar into a multiplication by its reciprocal
on the device, which is not the true division the entries do.
"""
import pytest
import torch

from conftest import load_golden
from multi_kernel_ref import (DEGREES, FIXTURES, ISOLATED, MODEL_ARGS, MODEL_FIXTURE, check,
                              degree_graphs, fixture_inputs, fixture_tensors, make_module,
                              random_graph, ref_run, zero_graph)
from residual_ref import BAND, SENT, Guarded  # noqa: F401  (the sentinel-guarded buffer)

pytestmark = pytest.mark.gpu


class Launches:
    """Names of the libmgcn launches made inside the block (the kernel timer hook)."""

    def __enter__(self):
        from mgcn import ops
        self.names = []
        ops.set_kernel_timer(lambda name, start, rows=None, edges=None:
                             self.names.append(name) if start else None)
        return self

    def __exit__(self, *exc):
        from mgcn import ops
        ops.set_kernel_timer(None)

    def count(self, prefix):
        return sum(n.startswith(prefix) for n in self.names)

    def fused(self, n=1):
        """n multi-kernel launches per direction and no per-kernel aggregation."""
        return (self.count("multi_spmm_fwd") == n and self.count("multi_spmm_bwd") == n
                and self.count("spmm_") == 0)

    def looped(self, K):
        return (self.count("multi_") == 0 and
                self.count("spmm_fwd") + self.count("spmm_xw_fwd") == K)


def _dev(ts, cuda):
    return None if ts is None else [None if t is None else t.to(cuda) for t in ts]


def _run_module(mod, x, eis, degs, ews, dY, relu=False):
    mod.zero_grad()
    xx = x.detach().clone().requires_grad_(True)
    y = mod.forward_fused(xx, eis, None, degs, ews, relu=relu)
    y.backward(dY)
    out = {"y": y.detach(), "dx": xx.grad}
    out.update({"g_" + k: p.grad for k, p in mod.named_parameters() if p.grad is not None})
    return out


# ------------------------------------------------------------------ fixtures
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_fixture(cuda, name):
    """The reference's y, dx and every parameter gradient within the bound on
    the fused route (one launch per direction); a second run is bitwise equal;
    the rows without an edge in any kernel hold the combined biases exactly."""
    spec = FIXTURES[name]
    z, sd = fixture_tensors(load_golden(name))
    eis, degs, ews = fixture_inputs(z, spec)
    mod = make_module(spec)
    mod.load_state_dict(sd, strict=True)
    mod = mod.to(cuda)
    args = (z["x"].to(cuda), _dev(eis, cuda), _dev(degs, cuda), _dev(ews, cuda), z["dY"].to(cuda))
    with Launches() as rec:
        got = _run_module(mod, *args)
    assert rec.fused(), rec.names
    for k, v in got.items():
        check(f"{name}.{k}", v, z[k + "32"], z[k + "64"])
    assert {k for k in z if k.endswith("64")} == {k + "64" for k in got}
    again = _run_module(mod, *args)
    for k, v in got.items():
        assert torch.equal(v, again[k]), k
    bs = [sd.get(f"node_models.{k}.bias") for k in range(spec["K"]) if eis[k] is not None]
    C = got["y"].size(1) // (len(bs) if spec["combine"] == "cat" else 1)
    bs = [torch.zeros(C) if b is None else b for b in bs]
    if spec["combine"] == "cat":
        want = torch.cat(bs)
    else:
        want = bs[0]
        for b in bs[1:]:
            want = want + b
        if spec["combine"] == "mean":
            want = want / torch.tensor(float(len(bs)))
    assert torch.equal(got["y"][-ISOLATED:].cpu(), want.expand(ISOLATED, -1))


def test_model_fixture(cuda):
    """The reference's GCNModel with two kernels per layer: every layer takes
    the fused route with its ReLU folded."""
    from mgcn.models import GCNModel
    z, sd = fixture_tensors(load_golden(MODEL_FIXTURE))
    args = dict(MODEL_ARGS)
    m = GCNModel(args.pop("in_channels"), args.pop("enc_sizes"), args.pop("num_classes"), **args)
    m.load_state_dict(sd, strict=True)
    m = m.to(cuda)
    eis = [z["edge_index0"].to(cuda), z["edge_index1"].to(cuda)]
    x = z["x"].to(cuda).requires_grad_(True)
    with Launches() as rec:
        y = m(x, eis)
        y.backward(z["dY"].to(cuda))
    assert rec.fused(3), rec.names
    check("mk_model.y", y, z["y32"], z["y64"])
    check("mk_model.dx", x.grad, z["dx32"], z["dx64"])
    for k, p in m.named_parameters():
        check(f"mk_model.g_{k}", p.grad, z[f"g_{k}32"], z[f"g_{k}64"])


# ---------------------------------------------------------------- ABI parity
_PLANS = {}
METHODS = ("sm", None, "rw")


def _plans(cuda, n, zero=False):
    """(plans, norms) of degree_graphs(8, n): normalisations cycle sm / none /
    rw (per-slot weights, ones, the adjoint's row scale); ``zero``: the second
    set has no edges."""
    key = (n, zero)
    if key not in _PLANS:
        from mgcn.graph import build_plan
        eis = degree_graphs(8, n)
        if zero:
            eis[1] = zero_graph()
        plans = [build_plan(ei.to(cuda), n) for ei in eis]
        for p in plans:
            assert p.fwd.n_heavy == 0 and p.bwd.n_heavy == 0
        ind = torch.stack([p.fwd.rowptr[1:] - p.fwd.rowptr[:-1] for p in plans]).cpu()
        for k in (0, 2, 3):  # the ladder rows of set k are empty in set k + 1
            assert ind[k, 8 * (k % 4):8 * (k % 4) + 8].tolist() == list(DEGREES)
            assert not ind[(k + 1) % 8, 8 * (k % 4):8 * (k % 4) + 8].any()
        _PLANS[key] = (plans, [p.norm(METHODS[k % 3]) for k, p in enumerate(plans)])
    return _PLANS[key]


def _strided(rows, cols, pad, cuda, gen=None):
    """[rows, cols] float32 with row stride cols + pad."""
    buf = torch.empty(rows, cols + pad, device=cuda)
    if gen is not None:
        buf.copy_(torch.randn(rows, cols + pad, generator=gen))
    return buf[:, :cols]


@pytest.mark.parametrize("n", [67, 300])
@pytest.mark.parametrize("C,pad", [(8, 0), (30, 2), (33, 0), (128, 4), (130, 0), (160, 0)])
def test_entries_equal_the_single_kernel_calls(cuda, C, pad, n):
    """mgcn_multi_spmm_fwd / _bwd against K mgcn_spmm_fwd / _bwd calls on the
    column-block views, torch adds in kernel order and a true division:
    torch.equal.  K in 2, 3, 8; combine add / mean / cat; reduce sum / mean;
    ReLU on and off; C at vector widths 4 (8, 128, 160), 2 (30, 130) and 1
    (33), lane groups of 4 to 64 lanes and two chunks (130); rows of 0, 1, 31,
    32, 33, 64, 65 and 128 slots in one kernel that are empty in another; a
    kernel without edges (K = 3); leading dimensions beyond K C (pad)."""
    from mgcn import _lib as L, ops
    gen = torch.Generator().manual_seed(1000 * C + n)
    for K in (2, 3, 8):
        plans, norms = _plans(cuda, n, zero=(K == 3))
        plans, norms = plans[:K], norms[:K]
        H = _strided(n, K * C, pad, cuda, gen)
        biases = [torch.randn(C, generator=gen).to(cuda) if k % 2 == 0 else None for k in range(K)]
        Kt = torch.tensor(float(K), device=cuda)
        for combine in ("add", "mean", "cat"):
            cc = L.COMBINE_CODES[combine]
            wide = K * C if combine == "cat" else C
            dY = _strided(n, wide, pad, cuda, gen)
            for reduce in (L.REDUCE_SUM, L.REDUCE_MEAN):
                for relu in (False, True):
                    tag = f"K={K} {combine} reduce={reduce} relu={relu}"
                    got = ops.multi_spmm_fwd(plans, norms, H, reduce, cc, biases, relu,
                                             out=_strided(n, wide, pad, cuda))
                    parts = [ops.spmm_fwd(p.fwd, nm.w_fwd, H[:, k * C:(k + 1) * C], reduce, b,
                                          relu and combine == "cat")[0]
                             for k, (p, nm, b) in enumerate(zip(plans, norms, biases))]
                    if combine == "cat":
                        want = torch.cat(parts, dim=1)
                    else:
                        want = parts[0]
                        for part in parts[1:]:
                            want = want + part
                        if combine == "mean":
                            want = want / Kt
                        if relu:
                            want = torch.relu(want)
                    assert torch.equal(got, want), "fwd " + tag
                # adjoint
                got = ops.multi_spmm_bwd(plans, norms, dY, reduce, cc,
                                         out=_strided(n, K * C, pad, cuda))
                g = dY / Kt if combine == "mean" else dY
                want = torch.empty(n, K * C, device=cuda)
                for k, (p, nm) in enumerate(zip(plans, norms)):
                    gk = g[:, k * C:(k + 1) * C] if combine == "cat" else g
                    ops.spmm_bwd(p.bwd, nm.w_bwd, nm.row_scale_bwd, gk, reduce, cnt=p.in_cnt,
                                 out=want[:, k * C:(k + 1) * C])
                assert torch.equal(got, want), f"bwd K={K} {combine} reduce={reduce}"


# --------------------------------------------------------------------- route
def _layer_case(cuda, eis, n, K=2, fin=16, fout=32, seed=0):
    from mgcn.models import GCNLayer
    torch.manual_seed(seed)
    layer = GCNLayer(fin, fout, deg_norm='sm', num_kernel=K, non_linear='relu')
    with torch.no_grad():
        for nm in layer.gcn.node_models:
            nm.bias.uniform_(-0.5, 0.5)
    x, dY = torch.randn(n, fin), torch.randn(n, fout)
    Ws = [nm.weight_node.detach().clone() for nm in layer.gcn.node_models]
    bs = [nm.bias.detach().clone() for nm in layer.gcn.node_models]
    refs = [ref_run(x, Ws, bs, eis, dY, 'sm', 'add', 'add', dt, relu=True)
            for dt in (torch.float32, torch.float64)]
    return layer.to(cuda), x.to(cuda), dY.to(cuda), [ei.to(cuda) for ei in eis], refs


def _run_layer(layer, x, eis, dY):
    layer.zero_grad()
    xx = x.detach().clone().requires_grad_(True)
    with Launches() as rec:
        y = layer(xx, eis)
        y.backward(dY)
    nms = layer.gcn.node_models
    return rec, {"y": y.detach(), "dx": xx.grad, "g_W": [nm.weight_node.grad for nm in nms],
                 "g_b": [nm.bias.grad for nm in nms]}


def _check_layer(tag, got, refs):
    r32, r64 = refs
    for k in ("y", "dx"):
        check(f"{tag}.{k}", got[k], r32[k], r64[k])
    for k in ("g_W", "g_b"):
        for i, g in enumerate(got[k]):
            check(f"{tag}.{k}{i}", g, r32[k][i], r64[k][i])


def test_route_switch(cuda):
    """A K = 2 GCNLayer with ReLU: with the switch on exactly one
    mgcn_multi_spmm_fwd and one mgcn_multi_spmm_bwd and no mgcn_spmm_* launch;
    with it off the loop over the kernels; both within the bound."""
    from mgcn import ops
    n = 300
    eis = [random_graph(s, n, 2000, isolated=2) for s in (11, 12)]
    layer, x, dY, deis, refs = _layer_case(cuda, eis, n)
    rec, on = _run_layer(layer, x, deis, dY)
    assert rec.fused(), rec.names
    ops.set_fused_multi_kernel(False)
    try:
        rec, off = _run_layer(layer, x, deis, dY)
    finally:
        ops.set_fused_multi_kernel(True)
    assert rec.looped(2) and rec.count("spmm_bwd") + rec.count("spmm_xw_bwd") == 2, rec.names
    _check_layer("on", on, refs)
    _check_layer("off", off, refs)


def test_heavy_rows_take_the_loop(cuda):
    """One row of degree 200 (a heavy row of the first kernel's fwd view): the
    loop runs with the switch on."""
    from mgcn.graph import plan_for
    n = 300
    hub = torch.stack([torch.arange(40, 240), torch.full((200,), 7)])
    eis = [torch.cat([random_graph(21, n, 1500), hub], dim=1), random_graph(22, n, 1500)]
    layer, x, dY, deis, refs = _layer_case(cuda, eis, n, seed=1)
    assert plan_for(deis[0], n).fwd.n_heavy == 1
    rec, got = _run_layer(layer, x, deis, dY)
    assert rec.looped(2), rec.names
    _check_layer("hub", got, refs)


def test_fused_layer_shapes_take_the_loop(cuda):
    """128 -> 128: every kernel's layer runs on the fused aggregate-then-transform
    kernel, which measured faster than the GEMM + one gather launch; the loop
    runs with the switch on, and the fused route when those kernels are off."""
    from mgcn import ops
    n = 300
    eis = [random_graph(s, n, 2000, isolated=2) for s in (41, 42)]
    layer, x, dY, deis, refs = _layer_case(cuda, eis, n, fin=128, fout=128, seed=2)
    rec, got = _run_layer(layer, x, deis, dY)
    assert rec.count("multi_") == 0 and rec.count("spmm_xw_fwd") == 2, rec.names
    _check_layer("xw", got, refs)
    ops.set_fused_layers(False)
    try:
        rec, got = _run_layer(layer, x, deis, dY)
    finally:
        ops.set_fused_layers(True)
    assert rec.fused(), rec.names
    _check_layer("multi128", got, refs)


# --------------------------------------------------------------- ReLU folded
@pytest.mark.parametrize("combine", ["add", "mean", "cat"])
def test_relu_folded_equals_relu_after(cuda, combine):
    """forward_fused(relu=True) on the fused route against torch.relu of its
    relu=False output: y and every gradient bit for bit, with zeros and
    positives both present."""
    from mgcn.models import GCNMultiKernel
    n, K = 300, 3
    torch.manual_seed(5)
    mod = GCNMultiKernel(16, 32, None, deg_norm='rw', aggr='mean', bias=True, num_kernel=K,
                         kernel_combine=combine).to(cuda)
    with torch.no_grad():
        for nm in mod.node_models:
            nm.bias.uniform_(-0.5, 0.5)
    eis = [random_graph(30 + k, n, 1800, isolated=1).to(cuda) for k in range(K)]
    x = torch.randn(n, 16, device=cuda)
    dY = torch.randn(n, 32 * (K if combine == "cat" else 1), device=cuda)
    with Launches() as rec:
        folded = _run_module(mod, x, eis, None, None, dY, relu=True)
    assert rec.fused(), rec.names
    mod.zero_grad()
    xx = x.detach().clone().requires_grad_(True)
    y = torch.relu(mod.forward_fused(xx, eis, relu=False))
    y.backward(dY)
    assert bool((y == 0).any()) and bool((y > 0).any())
    assert torch.equal(folded["y"], y)
    assert torch.equal(folded["dx"], xx.grad)
    for k, p in mod.named_parameters():
        assert torch.equal(folded["g_" + k], p.grad), k


# -------------------------------------------------------------------- EINVAL
def test_entries_reject_bad_arguments(cuda):
    from mgcn import _lib as L
    from mgcn.ops_multi import _views
    lib = L.load()
    n, C = 67, 8
    plans, norms = _plans(cuda, n)
    H = torch.zeros(n, 9 * C, device=cuda)
    Y = torch.zeros(n, 9 * C, device=cuda)
    st = L.stream_of(cuda)

    def both(rows, K, v):
        return [lib.mgcn_multi_spmm_fwd(rows, K, C, v, L.ptr(H), 9 * C, L.ptr(Y), 9 * C, 0, 0, 0,
                                        st),
                lib.mgcn_multi_spmm_bwd(rows, K, C, v, L.ptr(Y), 9 * C, L.ptr(H), 9 * C, 0, 0, st)]
    v = _views(plans, norms, False, [None] * 8)
    assert both(n, 0, v) == [L.EINVAL] * 2
    assert both(n, 9, v) == [L.EINVAL] * 2
    assert both(n - 1, 2, v) == [L.EINVAL] * 2  # the views have n rows
    v.n_rows[1] = n - 1
    assert both(n, 2, v) == [L.EINVAL] * 2
    assert b"view 1 has 66 rows" in lib.mgcn_last_error()
    torch.cuda.synchronize()
    assert not H.any() and not Y.any()  # nothing was launched


# --------------------------------------------------------------- guard bands
# (Guarded, SENT, BAND: residual_ref.py, shared with test_gpu_residual_shapes.py)
@pytest.mark.parametrize("n", [67, 300])
@pytest.mark.parametrize("C", [8, 30, 33, 128, 130])
def test_guard_bands_stay_untouched(cuda, C, n):
    """Y and dH_all between sentinel bands, for every combine: the bands are
    untouched and every element between them is written."""
    from mgcn import _lib as L, ops
    K = 3
    plans, norms = _plans(cuda, n)
    plans, norms = plans[:K], norms[:K]
    gen = torch.Generator().manual_seed(C)
    H = torch.randn(n, K * C, generator=gen).to(cuda)
    for combine in ("add", "cat"):
        cc = L.COMBINE_CODES[combine]
        wide = K * C if combine == "cat" else C
        Y = Guarded(n, wide, cuda)
        ops.multi_spmm_fwd(plans, norms, H, L.REDUCE_MEAN, cc, [None] * K, True, out=Y.t)
        dH = Guarded(n, K * C, cuda)
        ops.multi_spmm_bwd(plans, norms, torch.randn(n, wide, generator=gen).to(cuda),
                           L.REDUCE_MEAN, cc, out=dH.t)
        torch.cuda.synchronize()
        assert Y.intact() and dH.intact(), combine
        for g in (Y, dH):
            assert not bool((g.t.view(torch.int32) == SENT).any()), combine
