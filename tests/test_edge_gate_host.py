"""CPU-only checks of the edge-gate feature's host layer (no GPU compute): the
GPU tests' torch restatement against the reference's fp64 fixtures, the module
surface against the reference's state_dicts, the routing of gated layers and
argument validation before any launch."""
import pytest
import torch

from conftest import golden_names, load_golden
from edge_gate_ref import (FIXTURES, MODEL_ARGS, MODEL_FIXTURE, fixture_tensors,
                           make_node_model, params_of, ref_run)


def test_every_fixture_is_present():
    assert set(golden_names("gate_")) == set(FIXTURES) | {MODEL_FIXTURE}


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_restatement_agrees_with_reference_fixture(name):
    """edge_gate_ref.gate_layer_ref, the yardstick of the random GPU cases, in
    fp64 on a fixture's own inputs against the reference's fp64 results:
    max|r64 - t64| <= 1e-12 max|t64| for y, the gates, dx and every parameter
    gradient."""
    gate, dn, aggr = FIXTURES[name][:3]
    z, sd = fixture_tensors(load_golden(name))
    r64 = ref_run(z["x"], params_of(sd), z["edge_index"], z["dY"], gate, dn, aggr, torch.float64,
                  edge_attr=z.get("edge_attr"), edge_weight=z.get("edge_weight"),
                  deg=z.get("deg"))
    from edge_gate_ref import PARAM_KEYS
    pairs = [("y", "y"), ("gate", "gate"), ("dx", "dx")]
    pairs += [("g_" + k, "g_" + v) for k, v in PARAM_KEYS.items() if v in sd]
    for rk, fk in pairs:
        t64 = z[fk + "64"]
        assert r64[rk].dtype == torch.float64 and r64[rk].shape == t64.shape, rk
        err = (r64[rk] - t64).abs().max().item()
        scale = t64.abs().max().item()
        print(f"{name}.{rk}: restatement err {err:.3e}  max|t64| {scale:.3e}")
        assert err <= 1e-12 * scale, f"{name}.{rk}: {err:.3e} > 1e-12 * {scale:.3e}"


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_state_dict_matches_the_reference(name):
    """Keys (in order) and shapes equal the reference's; a strict load."""
    z, sd = fixture_tensors(load_golden(name))
    nm = make_node_model(name, num_edges=z["edge_index"].size(1))
    own = nm.state_dict()
    assert list(own) == list(sd)
    assert all(own[k].shape == sd[k].shape for k in sd)
    nm.load_state_dict(sd, strict=True)


def test_reference_model_state_dict_loads_strictly():
    from mgcn.models import EdgeGateProj, GCNModel, NodeModelGatedAdditive
    z, sd = fixture_tensors(load_golden(MODEL_FIXTURE))
    args = dict(MODEL_ARGS)
    m = GCNModel(args.pop("in_channels"), args.pop("enc_sizes"), args.pop("num_classes"), **args)
    assert list(m.state_dict()) == list(sd)
    assert "gcn_net.0.gcn.node_models.0.edge_gate.linsrc.weight" in sd
    m.load_state_dict(sd, strict=True)
    for layer in m.gcn_net:
        nm = layer.gcn.node_models[0]
        assert isinstance(nm, NodeModelGatedAdditive) and isinstance(nm.edge_gate, EdgeGateProj)
        assert nm.edge_gate.linsrc.weight.shape == (1, 32) and nm.edge_gate.bias.shape == (1,)


def test_routing_builds_the_gated_class():
    from mgcn.models import (EdgeGateFree, EdgeGateProj, GCNLayer, GCNMultiKernel,
                             NodeModelAdditive, NodeModelGatedAdditive)
    mk = GCNMultiKernel(6, 8, None, deg_norm='sm', edge_gate='proj', num_kernel=2)
    assert all(type(nm) is NodeModelGatedAdditive for nm in mk.node_models)
    assert isinstance(mk.node_models[0].edge_gate, EdgeGateProj)
    assert mk.node_models[0].edge_gate.in_channels == 8  # the gate reads the projected rows
    layer = GCNLayer(6, 8, edge_gate='free', num_edges=11)
    nm = layer.gcn.node_models[0]
    assert type(nm) is NodeModelGatedAdditive and isinstance(nm.edge_gate, EdgeGateFree)
    assert nm.edge_gate.edge_gates.shape == (11, 1)
    assert torch.equal(nm.edge_gate.edge_gates, torch.ones(11, 1))  # the reference's init
    assert layer.gcn.can_fuse_relu(torch.tensor([[0, 1], [1, 0]]))  # the kernel has the epilogue
    plain = GCNLayer(6, 8)
    assert type(plain.gcn.node_models[0]) is NodeModelAdditive
    assert plain.gcn.node_models[0].edge_gate is None
    with pytest.raises(NotImplementedError, match="NodeModelGatedAdditive"):
        NodeModelAdditive(3, 5, edge_gate="proj")  # the plain class keeps raising
    with pytest.raises(AssertionError):
        NodeModelGatedAdditive(3, 5, edge_gate="free")  # num_edges missing, as in the reference
    nm = NodeModelGatedAdditive(3, 5, in_edgedim=2, edge_gate="proj")
    assert list(nm.state_dict()) == ["weight_node", "weight_edge", "bias", "edge_gate.bias",
                                     "edge_gate.linsrc.weight", "edge_gate.lintgt.weight",
                                     "edge_gate.linedge.weight"]


def test_fused_routes_decline_gated_layers():
    from mgcn.dist import ShardedGCNStack
    from mgcn.models import GCNLayer, GCNModel, GCNStack
    x = torch.zeros(4, 32)
    gated = GCNStack([GCNLayer(32, 32, edge_gate='proj'), GCNLayer(32, 32, edge_gate='proj')])
    plain = GCNStack([GCNLayer(32, 32), GCNLayer(32, 32)])
    mixed = GCNStack([GCNLayer(32, 32), GCNLayer(32, 32, edge_gate='proj')])
    assert plain._fusable(x) is not None
    assert gated._fusable(x) is None and mixed._fusable(x) is None
    ei = torch.tensor([[0, 1], [1, 0]])
    with pytest.raises(NotImplementedError, match="gated"):
        ShardedGCNStack(gated, ei, 4)

    class _Cuda:  # _residual_fusable asks only for the device type and dtype
        device = torch.device("cuda")
        dtype = torch.float32
    for eg, want in ((None, True), ('proj', False)):
        m = GCNModel(32, [32, 32], 2, residual_hop=1, dropout=0, edge_gate=eg)
        assert m._residual_fusable(_Cuda, ei, None) is want


def test_argument_errors_before_any_launch():
    import mgcn
    from mgcn.models import NodeModelAdditive, NodeModelGatedAdditive
    x = torch.randn(5, 4)
    ei = torch.tensor([[0, 1, 2], [1, 2, 3]])
    with pytest.raises(mgcn.MgcnError, match="HIP device"):
        NodeModelGatedAdditive(4, 6, edge_gate="proj")(x, ei)
    with pytest.raises(mgcn.MgcnError, match="HIP device"):
        NodeModelGatedAdditive(4, 6, edge_gate="proj").edge_gate(torch.randn(5, 6), ei)
    # EdgeGateFree holds one gate per edge of a fixed graph
    with pytest.raises(ValueError, match="holds 7 gates, the graph has 3 edges"):
        NodeModelGatedAdditive(4, 6, edge_gate="free", num_edges=7)(x, ei)
    # max is not linear in the message: no edge-feature message term, gated or not
    ea = torch.randn(3, 2)
    for nm in (NodeModelGatedAdditive(4, 6, in_edgedim=2, edge_gate="proj", aggr="max"),
               NodeModelAdditive(4, 6, in_edgedim=2, aggr="max")):
        with pytest.raises(NotImplementedError, match="aggr='max' with an edge_attr message"):
            nm(x, ei, edge_attr=ea)
    with pytest.raises(ValueError, match=r"edge_attr must be \[3, 2\]"):
        NodeModelAdditive(4, 6, in_edgedim=2)(x, ei, edge_attr=torch.randn(4, 2))


def test_gate_entries_validate_before_any_launch():
    import mgcn
    lib = mgcn.load()

    def calls(n, nnz, C, reduce=0):
        return [lib.mgcn_gate_fwd(n, nnz, C, None, None, None, None, None, None, 0, None, None, C,
                                  reduce, None, 0, None, C, None, None, None),
                lib.mgcn_gate_bwd_dst(n, nnz, C, None, None, None, C, None, C, None, None, None,
                                      None, None, None, None, None),
                lib.mgcn_gate_bwd_src(n, nnz, C, None, None, None, None, C, None, None, None, None,
                                      None, None, None, None, None, C, None)]
    assert calls(0, 0, 32) == [0, 0, 0]          # zero rows: a successful no-op
    assert calls(0, 0, 1024) == [0, 0, 0]
    assert calls(0, 0, 1025) == [1, 1, 1]
    assert b"C <= 1024" in lib.mgcn_last_error()
    assert calls(0, 0, 0) == [1, 1, 1]
    assert calls(-1, 0, 8) == [1, 1, 1]
    assert calls(0, 1 << 31, 8) == [1, 1, 1]
    assert b"nnz < 2^31" in lib.mgcn_last_error()
    assert calls(4, 0, 8) == [1, 1, 1]           # rows with null arrays
    assert calls(0, 0, 8, reduce=3)[0] == 1
    assert lib.mgcn_abi_version() == 22          # the additions are backward compatible
