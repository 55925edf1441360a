"""NodeModelGatedAdditive / gate_aggregate on the fused HIP gate kernels
(MI355X), against the reference's own runs (golden fixtures gate_*.npz,
tests/golden/make_golden_edge_gate.py).

Every comparison uses one tolerance, per compared tensor t (edge_gate_ref.py):

    max|t_gpu - t64| <= max(4 * max|t32 - t64|, 1e-5 * max|t64|)
"""
import numpy as np
import pytest
import torch

from conftest import load_golden
from edge_gate_ref import (FIXTURES, MODEL_ARGS, MODEL_FIXTURE, check, fixture_tensors,
                           make_node_model, params_of, ref_run)

pytestmark = pytest.mark.gpu


def _gpu_run(nm, z, cuda, relu=False):
    x = z["x"].to(cuda).requires_grad_(True)
    kw = {k: z[k].to(cuda) for k in ("edge_attr", "edge_weight", "deg") if k in z}
    nm.zero_grad()
    store = []
    ei = z["edge_index"].to(cuda)
    if relu:
        y = nm.forward_fused(x, ei, kw.get("edge_attr"), kw.get("deg"), kw.get("edge_weight"),
                             relu=True, gate_store=store)
    else:
        y = nm(x, ei, gate_store=store, **kw)
    y.backward(z["dY"].to(cuda))
    out = {"y": y.detach(), "gate": store[0].view(-1, 1), "dx": x.grad}
    for k, p in nm.named_parameters():
        out["g_" + k] = p.grad
    return out


def _load(name, cuda):
    z, sd = fixture_tensors(load_golden(name))
    nm = make_node_model(name, num_edges=z["edge_index"].size(1))
    nm.load_state_dict(sd, strict=True)
    return z, nm.to(cuda)


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_fixture(cuda, name):
    """y, the gates (COO order), dx and every parameter gradient against the
    reference's own fp64 run; two runs bitwise equal; on the hub graph (20
    nodes without any edge; the random graphs carry a self-loop on every node)
    rows without in-edges give exactly the bias."""
    z, nm = _load(name, cuda)
    got = _gpu_run(nm, z, cuda)
    keys = ["y", "gate", "dx"] + ["g_" + k for k, _ in nm.named_parameters()]
    for k in keys:
        check(f"{name}.{k}", got[k], z[k + "32"], z[k + "64"])
    again = _gpu_run(nm, z, cuda)
    for k in keys:
        assert torch.equal(got[k], again[k]), k
    if name.endswith("hub"):
        N = z["x"].size(0)
        empty = torch.from_numpy(np.bincount(z["edge_index"][1].numpy(), minlength=N) == 0)
        assert empty.sum() >= 20
        rows = got["y"][empty.to(cuda)]
        assert torch.equal(rows, nm.bias.detach().expand_as(rows))


def test_model_debru(cuda):
    """The run_debru_32_eg.sh model at 6 layers end to end: output, input
    gradient and every parameter gradient against the reference model's own
    fp64 run; the fused residual route declines it.  (The generator keeps a
    draw of this fixture only if the reference's own fp32 run stays inside the
    bound under 8 other edge orders: make_golden_edge_gate.py.)"""
    from mgcn.models import GCNModel, NodeModelGatedAdditive
    z, sd = fixture_tensors(load_golden(MODEL_FIXTURE))
    args = dict(MODEL_ARGS)
    m = GCNModel(args.pop("in_channels"), args.pop("enc_sizes"), args.pop("num_classes"), **args)
    m.load_state_dict(sd, strict=True)
    m = m.to(cuda)
    assert all(isinstance(l.gcn.node_models[0], NodeModelGatedAdditive) for l in m.gcn_net)
    x = z["x"].to(cuda).requires_grad_(True)
    ei = z["edge_index"].to(cuda)
    assert not m._residual_fusable(x, ei, None)
    store = []
    y = m(x, ei, gate_store=store)
    y.backward(z["dY"].to(cuda))
    assert [tuple(g.shape) for g in store] == [(ei.size(1),)] * 6  # one [E] per layer
    check("model.y", y, z["y32"], z["y64"])
    check("model.dx", x.grad, z["dx32"], z["dx64"])
    for k, p in m.named_parameters():
        check("model.g_" + k, p.grad, z["g_" + k + "32"], z["g_" + k + "64"])


@pytest.mark.parametrize("name,which", [("gate_proj_sm_add_ew", "edge_weight"),
                                        ("gate_proj_rw_add_deg", "deg"),
                                        ("gate_proj_sm_mean_bias", "deg")])
def test_norm_input_gradients(cuda, name, which):
    """Gradients with respect to edge_weight / deg (through the differentiable
    norm and the kernel's per-slot weight gradient) against the restatement's
    fp32 and fp64 runs."""
    z, nm = _load(name, cuda)
    gate, dn, aggr = FIXTURES[name][:3]
    N = z["x"].size(0)
    ew = z.get("edge_weight")
    deg = z.get("deg")
    if which == "deg" and deg is None:
        deg = torch.from_numpy(np.bincount(z["edge_index"][0].numpy(), minlength=N)
                               .astype(np.float32)) + 0.25
    P = params_of({k: v.detach().cpu() for k, v in nm.state_dict().items()})
    r32, r64 = (ref_run(z["x"], P, z["edge_index"], z["dY"], gate, dn, aggr, dt, edge_weight=ew,
                        deg=deg) for dt in (torch.float32, torch.float64))
    x = z["x"].to(cuda).requires_grad_(True)
    t = (ew if which == "edge_weight" else deg).to(cuda).requires_grad_(True)
    kw = {"edge_weight": t} if which == "edge_weight" else {"deg": t}
    nm.zero_grad()
    y = nm(x, z["edge_index"].to(cuda), **kw)
    y.backward(z["dY"].to(cuda))
    check(f"{name}.y", y, r32["y"], r64["y"])
    check(f"{name}.dx", x.grad, r32["dx"], r64["dx"])
    check(f"{name}.g_{which}", t.grad, r32["g_" + which], r64["g_" + which])
    check(f"{name}.g_linsrc", nm.edge_gate.linsrc.weight.grad, r32["g_linsrc"], r64["g_linsrc"])


@pytest.mark.parametrize("name", ["gate_proj_none_add_bias", "gate_proj_none_max",
                                  "gate_proj_sm_mean_bias"])
def test_relu_fused_equals_unfused(cuda, name):
    """The ReLU epilogue of the kernel against torch.relu on the unfused
    layer's output: forward and every gradient bit for bit."""
    z, nm = _load(name, cuda)
    fused = _gpu_run(nm, z, cuda, relu=True)
    x = z["x"].to(cuda).requires_grad_(True)
    nm.zero_grad()
    y = torch.relu(nm(x, z["edge_index"].to(cuda)))
    y.backward(z["dY"].to(cuda))
    assert (y == 0).any() and (y > 0).any()
    assert torch.equal(fused["y"], y.detach())
    assert torch.equal(fused["dx"], x.grad)
    for k, p in nm.named_parameters():
        assert torch.equal(fused["g_" + k], p.grad), k


def test_layer_routes_relu_through_the_epilogue(cuda):
    """GCNLayer(edge_gate='proj', non_linear='relu') equals relu(node model)."""
    from mgcn.models import GCNLayer
    z, nm = _load("gate_proj_none_add_bias", cuda)
    layer = GCNLayer(16, 32, deg_norm=None, edge_gate='proj', aggr='add', bias=True).to(cuda)
    layer.gcn.node_models[0].load_state_dict(nm.state_dict(), strict=True)
    ei = z["edge_index"].to(cuda)
    assert layer.gcn.can_fuse_relu(ei)
    x = z["x"].to(cuda)
    store, direct = [], []
    assert torch.equal(layer(x, ei, gate_store=store), torch.relu(nm(x, ei, gate_store=direct)))
    assert len(store) == 1 and torch.equal(store[0], direct[0])


def test_bf16_input_is_the_rounded_fp32_result(cuda):
    """A bfloat16 Hx runs on the upcast rows and Y is rounded once."""
    from mgcn.graph import plan_for
    from mgcn.ops import gate_aggregate
    z, nm = _load("gate_proj_sm_add", cuda)
    ei = z["edge_index"].to(cuda)
    plan = plan_for(ei, z["x"].size(0))
    norm = plan.norm("sm")
    hx = (z["x"].to(cuda) @ nm.weight_node.detach()).to(torch.bfloat16)
    eg = nm.edge_gate
    args = (plan, norm, "add", eg.linsrc.weight.detach(), eg.lintgt.weight.detach(),
            eg.bias.detach())
    yb, gb = gate_aggregate(hx, *args)
    yf, gf = gate_aggregate(hx.float(), *args)
    assert yb.dtype == torch.bfloat16 and gb.dtype == torch.float32
    assert torch.equal(yb, yf.to(torch.bfloat16)) and torch.equal(gb, gf)


def test_gradient_arriving_on_the_gates(cuda):
    """g_coo is a differentiable output: a gradient sent into it joins the
    gate's own (the route of the edge-feature message term)."""
    from mgcn.graph import plan_for
    from mgcn.ops import gate_aggregate, linear
    name = "gate_proj_sm_add"
    z, nm = _load(name, cuda)
    gate, dn, aggr = FIXTURES[name][:3]
    E = z["edge_index"].size(1)
    dg = torch.randn(E, 1, generator=torch.Generator().manual_seed(5))
    P = params_of({k: v.detach().cpu() for k, v in nm.state_dict().items()})
    r32, r64 = (ref_run(z["x"], P, z["edge_index"], z["dY"], gate, dn, aggr, dt, dg=dg)
                for dt in (torch.float32, torch.float64))
    x = z["x"].to(cuda).requires_grad_(True)
    nm.zero_grad()
    plan = plan_for(z["edge_index"].to(cuda), x.size(0))
    eg = nm.edge_gate
    y, g = gate_aggregate(linear(x, nm.weight_node), plan, plan.norm(dn), aggr, eg.linsrc.weight,
                          eg.lintgt.weight, eg.bias, nm.bias)
    ((y * z["dY"].to(cuda)).sum() + (g * dg.view(-1).to(cuda)).sum()).backward()
    check("dg.dx", x.grad, r32["dx"], r64["dx"])
    check("dg.g_linsrc", eg.linsrc.weight.grad, r32["g_linsrc"], r64["g_linsrc"])
    check("dg.g_lintgt", eg.lintgt.weight.grad, r32["g_lintgt"], r64["g_lintgt"])
    check("dg.g_gbias", eg.bias.grad, r32["g_gbias"], r64["g_gbias"])
    check("dg.g_weight_node", nm.weight_node.grad, r32["g_weight_node"], r64["g_weight_node"])


def test_standalone_gate_modules(cuda):
    """EdgeGateProj.forward on projected rows returns the fixture's gates as
    [E, 1] in COO order; EdgeGateFree the sigmoid of its parameter."""
    z, nm = _load("gate_proj_sm_add_ea", cuda)
    hx = z["x"].to(cuda) @ nm.weight_node.detach()
    g = nm.edge_gate(hx, z["edge_index"].to(cuda), edge_attr=z["edge_attr"].to(cuda))
    assert g.shape == (z["edge_index"].size(1), 1)
    check("standalone.gate", g, z["gate32"], z["gate64"])
    z, nm = _load("gate_free_sm_add", cuda)
    check("standalone.free", nm.edge_gate(), z["gate32"], z["gate64"])


def test_shape_limits_and_cpu_raise(cuda):
    import mgcn
    from mgcn.graph import plan_for
    from mgcn.ops import gate_aggregate
    ei = torch.tensor([[0, 1, 2], [1, 2, 0]], device=cuda)
    plan = plan_for(ei, 3)
    with pytest.raises(mgcn.MgcnError, match="C <= 1024"):
        gate_aggregate(torch.zeros(3, 1025, device=cuda), plan, plan.norm(None))
    with pytest.raises(mgcn.MgcnError, match="HIP device"):
        gate_aggregate(torch.zeros(3, 8), plan, plan.norm(None))
    with pytest.raises(ValueError, match="come together"):
        gate_aggregate(torch.zeros(3, 8, device=cuda), plan, plan.norm(None),
                       w_src=torch.zeros(8, device=cuda))
