"""CPU-only checks of the multi-kernel feature's host layer (no GPU compute):
the GPU tests' torch restatement against the reference's fp64 fixtures, the
module surface against the reference's state_dicts, the routing predicate and
argument validation before any launch."""
import types

import pytest
import torch

from conftest import golden_names, load_golden
from multi_kernel_ref import (FIXTURES, MODEL_ARGS, MODEL_FIXTURE, fixture_inputs,
                              fixture_tensors, make_module, ref_run)


def test_every_fixture_is_present():
    assert set(golden_names("mk_")) == set(FIXTURES) | {MODEL_FIXTURE}


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_restatement_agrees_with_reference_fixture(name):
    """multi_kernel_ref.multi_layer_ref, the yardstick of the random GPU cases,
    in fp64 on a fixture's own inputs against the reference's fp64 results:
    max|r64 - t64| <= 1e-12 max|t64| for y, dx and every parameter gradient."""
    spec = FIXTURES[name]
    z, sd = fixture_tensors(load_golden(name))
    eis, degs, ews = fixture_inputs(z, spec)
    K = spec["K"]
    Ws = [sd[f"node_models.{k}.weight_node"] for k in range(K)]
    bs = [sd.get(f"node_models.{k}.bias") for k in range(K)]
    r64 = ref_run(z["x"], Ws, bs, eis, z["dY"], spec["deg_norm"], spec["aggr"], spec["combine"],
                  torch.float64, degs, ews)
    pairs = [("y", r64["y"]), ("dx", r64["dx"])]
    for k in range(K):
        if eis[k] is None:
            assert f"g_node_models.{k}.weight_node64" not in z  # a skipped kernel gets none
            continue
        pairs.append((f"g_node_models.{k}.weight_node", r64["g_W"][k]))
        if spec["bias"]:
            pairs.append((f"g_node_models.{k}.bias", r64["g_b"][k]))
    for fk, got in pairs:
        t64 = z[fk + "64"]
        assert got.dtype == torch.float64 and got.shape == t64.shape, fk
        err = (got - t64).abs().max().item()
        scale = t64.abs().max().item()
        print(f"{name}.{fk}: restatement err {err:.3e}  max|t64| {scale:.3e}")
        assert err <= 1e-12 * scale, f"{name}.{fk}: {err:.3e} > 1e-12 * {scale:.3e}"


def test_isolated_rows_hold_the_bias_sum():
    """The fixtures' last three nodes have no edge in any kernel: the
    reference's rows there are the combined biases (the GPU test asks the
    engine for exactly that)."""
    z, sd = fixture_tensors(load_golden("mk_add_k2_sm_add_bias"))
    want = sd["node_models.0.bias"] + sd["node_models.1.bias"]
    assert torch.equal(z["y32"][-3:], want.expand(3, -1))


@pytest.mark.parametrize("name", ["mk_add_k3_sm_mean_bias", "mk_add_k3_sm_add_skip",
                                  "mk_cat_k3_none_mean"])
def test_state_dict_of_three_kernels_loads_from_the_reference(name):
    """Keys (in order) and shapes equal the reference's; a strict load."""
    _, sd = fixture_tensors(load_golden(name))
    mod = make_module(FIXTURES[name])
    own = mod.state_dict()
    assert list(own) == list(sd) and len(mod.node_models) == 3
    assert all(own[k].shape == sd[k].shape for k in sd)
    mod.load_state_dict(sd, strict=True)


def test_reference_model_state_dict_loads_strictly():
    from mgcn.models import GCNModel
    _, sd = fixture_tensors(load_golden(MODEL_FIXTURE))
    args = dict(MODEL_ARGS)
    m = GCNModel(args.pop("in_channels"), args.pop("enc_sizes"), args.pop("num_classes"), **args)
    assert list(m.state_dict()) == list(sd)
    assert "gcn_net.2.gcn.node_models.1.weight_node" in sd
    m.load_state_dict(sd, strict=True)


def test_multi_aggregate_is_exported():
    import mgcn
    from mgcn import ops, ops_multi
    assert mgcn.multi_aggregate is ops.multi_aggregate is ops_multi.multi_aggregate
    assert "multi_aggregate" in mgcn.__all__
    for name in ("multi_kernel_fusable", "multi_kernel_reason", "multi_spmm_fwd",
                 "multi_spmm_bwd", "_MultiAggregate"):
        assert getattr(ops, name) is getattr(ops_multi, name)
    # the switch and its setter live in mgcn.ops itself (tests/test_ops_call.py)
    assert ops.set_fused_multi_kernel.__module__ == "mgcn.ops" and ops._FUSE_MULTI is True
    with pytest.raises(mgcn.MgcnError, match="HIP device"):
        mgcn.multi_aggregate(torch.zeros(4, 8), [], [])


class _OnDevice:
    """What the predicate reads of a device tensor (nothing touches a device)."""
    is_cuda = True
    dtype = torch.float32

    def __init__(self, n=10, f=4, dtype=torch.float32):
        self.n, self.f, self.dtype = n, f, dtype

    def dim(self):
        return 2

    def size(self, i):
        return (self.n, self.f)[i]

    def stride(self, i):
        return (self.f, 1)[i]


def _plan(n=10, heavy_fwd=0, heavy_bwd=0):
    return types.SimpleNamespace(num_nodes=n, nnz=5,
                                 fwd=types.SimpleNamespace(n_heavy=heavy_fwd, n_cols=n),
                                 bwd=types.SimpleNamespace(n_heavy=heavy_bwd, n_cols=n))


def _norm(grad=False):
    return types.SimpleNamespace(grad=grad)


def test_fusable_accepts_the_plain_case_and_declines_each_excluded_one():
    from mgcn import ops
    from mgcn.ops import multi_kernel_fusable as ok, multi_kernel_reason as why
    x = _OnDevice()
    two = ([_plan(), _plan()], [_norm(), _norm()])
    assert ok(x, *two) and ok(x, *two, aggr="mean")
    assert ok(x, [_plan()] * 8, [_norm()] * 8)
    assert not ok(x, [_plan()], [_norm()])                       # K = 1
    assert "1 kernels" in why(x, 1)
    assert not ok(x, [_plan()] * 9, [_norm()] * 9)               # K = 9
    assert "9 kernels" in why(x, 9)
    assert not ok(x, *two, aggr="max") and "max" in why(x, 2, "max")
    assert not ok(x, *two, plain=False) and "gated or attention" in why(x, 2, plain=False)
    assert not ok(x, *two, edge_attr=True) and "edge_attr" in why(x, 2, edge_attr=True)
    bf = _OnDevice(dtype=torch.bfloat16)
    assert not ok(bf, *two) and "bfloat16" in why(bf, 2)
    assert not ok(torch.zeros(10, 4), *two) and "not on the device" in why(torch.zeros(10, 4), 2)
    assert not ok(x, [_plan(), _plan()], [_norm(), _norm(grad=True)])     # differentiable norm
    assert not ok(x, [_plan(), _plan(heavy_fwd=1)], two[1])               # heavy rows, forward
    assert not ok(x, [_plan(heavy_bwd=2), _plan()], two[1])               # and backward
    assert not ok(x, [_plan(), _plan(n=11)], two[1])                      # another node set
    ops.set_fused_multi_kernel(False)
    try:
        assert not ok(x, *two)
    finally:
        ops.set_fused_multi_kernel(True)
    assert ok(x, *two)
    # shapes whose per-kernel layers run on the fused layer kernels keep the loop
    # (measured faster there), unless those kernels are switched off
    wide = _OnDevice(f=128)
    assert ok(wide, *two, out_channels=32) and ok(x, *two, out_channels=128)
    assert not ok(wide, *two, out_channels=128)
    assert not ok(_OnDevice(f=256), *two, aggr="mean", out_channels=256)
    ops.set_fused_layers(False)
    try:
        assert ok(wide, *two, out_channels=128)
    finally:
        ops.set_fused_layers(True)


def test_modules_decline_gated_attention_max_and_edge_attr():
    from mgcn.models import GCNLayer, GCNMultiKernel
    x = torch.zeros(6, 4)  # on the CPU: a module the route could take stops at the device
    ei = torch.tensor([[0, 1, 2], [1, 2, 3]])
    ea = torch.zeros(3, 2)

    def why(mod, eis, eas=None):
        return mod._multi_reason(x, eis, eas or [None] * len(eis))
    plain = GCNMultiKernel(4, 8, None, deg_norm='sm', num_kernel=2)
    assert why(plain, [ei, ei]) == "x is not on the device"
    assert "1 kernels" in why(plain, [ei, None])
    assert "gated or attention" in why(GCNMultiKernel(4, 8, None, edge_gate='proj', num_kernel=2),
                                       [ei, ei])
    assert "gated or attention" in why(GCNMultiKernel(4, 8, None, nodemodel='attention',
                                                      num_kernel=2), [ei, ei])
    assert "max" in why(GCNMultiKernel(4, 8, None, aggr='max', num_kernel=2), [ei, ei])
    assert "edge_attr" in why(GCNMultiKernel(4, 8, 2, num_kernel=2), [ei, ei], [ea, None])
    assert "bfloat16" in plain._multi_reason(x.bfloat16(), [ei, ei], [None, None])
    assert "9 kernels" in why(GCNMultiKernel(4, 8, None, num_kernel=9), [ei] * 9)
    # the layer folds its ReLU exactly for the modules the route may take
    for kwargs, want in ((dict(num_kernel=2), True), (dict(num_kernel=3, aggr='mean'), True),
                         (dict(num_kernel=2, aggr='max'), False),
                         (dict(num_kernel=2, edge_gate='proj'), False),
                         (dict(num_kernel=2, nodemodel='attention'), False),
                         (dict(num_kernel=9), False)):
        layer = GCNLayer(4, 8, **kwargs)
        assert layer.gcn.can_fuse_relu([ei] * kwargs["num_kernel"]) is want, kwargs
    two = GCNLayer(4, 8, num_kernel=2)
    assert two.gcn.can_fuse_relu([ei, None]) is False
    assert GCNLayer(4, 8).gcn.can_fuse_relu(ei) is True  # a single kernel: as before


def test_entries_validate_before_any_launch():
    import mgcn
    from mgcn import _lib as L
    lib = mgcn.load()
    assert {"mgcn_multi_spmm_fwd", "mgcn_multi_spmm_bwd"} <= set(L.SIGNATURES)

    def calls(n, K, C, rows=None, reduce=0, combine=0, ld=None):
        v = L.MultiViewsC()
        for k in range(L.MULTI_MAX_K):
            v.n_rows[k] = n if rows is None else rows[k]
        ld = K * C if ld is None else ld
        return [lib.mgcn_multi_spmm_fwd(n, K, C, v, None, ld, None, ld, reduce, combine, 0, None),
                lib.mgcn_multi_spmm_bwd(n, K, C, v, None, ld, None, ld, reduce, combine, None)]
    assert calls(0, 2, 32) == [0, 0]             # zero rows: a successful no-op
    assert calls(0, 8, 33, combine=2) == [0, 0]
    assert calls(0, 0, 32) == [1, 1]
    assert b"K = 0 outside [1, 8]" in lib.mgcn_last_error()
    assert calls(0, 9, 32) == [1, 1]
    assert calls(0, 2, 0) == [1, 1]
    assert calls(-1, 2, 8) == [1, 1]
    assert calls(0, 2, 8, reduce=2) == [1, 1]    # max
    assert calls(0, 2, 8, combine=3) == [1, 1]
    assert calls(5, 2, 8, rows=[5, 4] + [0] * 6) == [1, 1]
    assert b"view 1 has 4 rows, the call 5" in lib.mgcn_last_error()
    assert calls(4, 2, 8) == [1, 1]              # rows with null arrays
    assert lib.mgcn_abi_version() == 22          # the additions are backward compatible
