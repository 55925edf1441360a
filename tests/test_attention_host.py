"""CPU-only checks of the attention node model's host layer and C ABI boundary
(no GPU compute): module surface against the reference's, argument validation
before any launch; the GPU tests' torch restatement against the reference's
fp64 fixtures."""
import pytest
import torch

from attention_ref import FIXTURES, ref_run
from conftest import load_golden


def test_state_dict_keys_and_shapes_per_combine_mode():
    from mgcn.models import NodeModelAttention
    for combine, w_cols, c1 in (("cat", 12, 4), ("add", 36, 12), ("mean", 36, 12)):
        nm = NodeModelAttention(5, 12, nheads=3, att_combine=combine, bias=True)
        sd = nm.state_dict()
        assert list(sd) == ["weight", "att_weight", "bias"]
        assert sd["weight"].shape == (5, w_cols)
        assert sd["att_weight"].shape == (1, 3, 2 * c1)
        assert sd["bias"].shape == (12,)
        assert torch.count_nonzero(sd["bias"]) == 0  # zeros init
        assert nm.out_channels_1head == c1
    nm = NodeModelAttention(5, 12, nheads=3)
    assert list(nm.state_dict()) == ["weight", "att_weight"] and nm.bias is None
    assert repr(nm).startswith("NodeModelAttention (in_channels: 5, out_channels: 12, "
                               "in_edgedim: None, nheads: 3, att_activation: ")
    assert "att_dropout: 0, att_combine: cat, att_dir: in | number of parameters: 84" in repr(nm)


def test_reference_citation_state_dict_loads_strictly():
    """The reference's own GCNModel(nodemodel='attention') state_dict (golden
    fixture att_model_citation) loads with strict=True."""
    from mgcn.models import GCNModel, NodeModelAttention
    z = load_golden("att_model_citation")
    sd = {k[2:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("p_")}
    m = GCNModel(24, [32, 32, 7], 7, nheads=[2, 2, 1], residual_hop=1, nodemodel='attention',
                 bias=False, dropout=0, att_act='lrelu', att_dir='in', final_type='none')
    m.load_state_dict(sd, strict=True)
    nms = [layer.gcn.node_models[0] for layer in m.gcn_net]
    assert all(isinstance(nm, NodeModelAttention) for nm in nms)
    assert [nm.nheads for nm in nms] == [2, 2, 1]
    assert nms[2].att_weight.shape == (1, 1, 14)


def test_constructor_assertions():
    from mgcn.models import NodeModelAttention
    with pytest.raises(AssertionError):
        NodeModelAttention(4, 8, att_act="elu")
    with pytest.raises(AssertionError):
        NodeModelAttention(4, 8, att_dir="both")
    with pytest.raises(AssertionError):
        NodeModelAttention(4, 8, att_combine="max")
    with pytest.raises(AssertionError, match="divisible by nheads"):
        NodeModelAttention(4, 8, nheads=3)
    NodeModelAttention(4, 8, nheads=3, att_combine="add")  # not 'cat': any head count


def test_layer_and_multi_kernel_registration():
    from mgcn.models import GCNLayer, GCNMultiKernel, NodeModelAdditive, NodeModelAttention
    layer = GCNLayer(6, 8, nodemodel='attention', nheads=2)
    nm = layer.gcn.node_models[0]
    assert isinstance(nm, NodeModelAttention) and nm.nheads == 2
    assert nm.att_weight.shape == (1, 2, 8)
    ei = torch.tensor([[0, 1], [1, 0]])
    assert not layer.gcn.can_fuse_relu(ei)
    add = GCNLayer(6, 8, nheads=2)  # additive: nheads dropped, as before
    assert isinstance(add.gcn.node_models[0], NodeModelAdditive)
    assert add.gcn.can_fuse_relu(ei)
    with pytest.raises(NotImplementedError):
        GCNLayer(6, 8, nodemodel='hardattention')
    with pytest.raises(NotImplementedError):
        GCNMultiKernel(6, 8, nodemodel='hardattention')


def test_cpu_input_raises():
    import mgcn
    from mgcn.models import GCNLayer, NodeModelAttention
    x = torch.randn(5, 4)
    ei = torch.tensor([[0, 1, 2], [1, 2, 3]])
    with pytest.raises(mgcn.MgcnError, match="HIP device"):
        NodeModelAttention(4, 6, nheads=2)(x, ei)
    with pytest.raises(mgcn.MgcnError, match="HIP device"):
        GCNLayer(4, 6, nodemodel='attention', nheads=2)(x, ei)


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_restatement_agrees_with_reference_fixture(name):
    """The torch restatement (attention_ref.att_ref), the yardstick of every
    random GPU case, run in fp64 on a fixture's own x / parameters / edges /
    dY against the reference's fp64 results: max|r64 - t64| <= 1e-12 max|t64|.
    Measured 3.9e-16 .. 6.9e-16 relative; 1e-12 leaves room for another BLAS's
    summation order and is five orders below the fp32 error (2.4e-7 .. 3.8e-7)
    that the GPU bound rests on."""
    fin, fout, H, combine, adir, act, bias = FIXTURES[name]
    z = {k: torch.from_numpy(v) for k, v in load_golden(name).items()}
    assert z["p_weight"].shape[0] == fin and z["dY"].shape[1] == fout
    r64 = ref_run(z["x"], z["p_weight"], z["p_att_weight"], z["p_bias"] if bias else None,
                  z["edge_index"], z["dY"], H, combine, adir, act, torch.float64)
    for k in ("y", "alpha", "dx", "dW", "datt") + (("db",) if bias else ()):
        t64 = z[k + "64"]
        assert r64[k].dtype == torch.float64 and r64[k].shape == t64.shape, k
        err = (r64[k] - t64).abs().max().item()
        scale = t64.abs().max().item()
        print(f"{name}.{k}: restatement err {err:.3e}  max|t64| {scale:.3e}")
        assert err <= 1e-12 * scale, f"{name}.{k}: {err:.3e} > 1e-12 * {scale:.3e}"


def _calls(lib, n, nnz, H, C):
    ld = H * C
    return {
        "scores": lib.mgcn_att_scores(n, H, C, None, ld, None, None, None, None),
        "fwd": lib.mgcn_att_fwd(n, nnz, H, C, None, None, None, None, 0, None, None, None, ld,
                                None, ld, None, None),
        "softmax": lib.mgcn_edge_softmax(n, nnz, H, None, None, None, None, 0, None, None),
        "bwd_dst": lib.mgcn_att_bwd_dst(n, nnz, H, C, None, None, None, ld, None, ld, None, None,
                                        None, None, 0, 1, None, None, None),
        "bwd_src": lib.mgcn_att_bwd_src(n, nnz, H, C, None, None, None, None, ld, None, None,
                                        None, None, None, 0, 0, None, None, None, None, ld, None),
        "dst_fold": lib.mgcn_att_dst_fold(n, nnz, H, C, None, None, None, None, None, ld, None),
    }


def test_c_entries_validate_before_any_launch():
    import mgcn
    lib = mgcn.load()
    # zero rows with null pointers: a successful no-op
    assert set(_calls(lib, 0, 0, 2, 8).values()) == {0}
    # negative sizes
    assert set(_calls(lib, -1, 0, 2, 8).values()) == {1}
    bad = _calls(lib, 0, -1, 2, 8)
    assert all(bad[k] == 1 for k in bad if k != "scores")
    # H = 0, H = 17
    assert set(_calls(lib, 0, 0, 0, 8).values()) == {1}
    assert set(_calls(lib, 0, 0, 17, 8).values()) == {1}
    assert b"1 <= H <= 16" in lib.mgcn_last_error()
    # H C = 1025 (the softmax alone has no C)
    bad = _calls(lib, 0, 0, 1, 1025)
    assert all(bad[k] == 1 for k in bad if k != "softmax")
    assert all(v == 0 for k, v in _calls(lib, 0, 0, 1, 1024).items())
    assert all(v == 0 for k, v in _calls(lib, 0, 0, 16, 64).items())
    bad = _calls(lib, 0, 0, 16, 65)
    assert all(bad[k] == 1 for k in bad if k != "softmax")
    # C = 0, nnz H >= 2^31
    bad = _calls(lib, 0, 0, 2, 0)
    assert all(bad[k] == 1 for k in bad if k != "softmax")
    bad = _calls(lib, 0, 1 << 28, 8, 4)
    assert all(bad[k] == 1 for k in bad if k != "scores")
    assert b"nnz H < 2^31" in lib.mgcn_last_error()
    # rows with null arrays, bad activation code
    assert set(_calls(lib, 4, 0, 2, 8).values()) - {0} == {1}
    assert lib.mgcn_att_fwd(0, 0, 2, 8, None, None, None, None, 3, None, None, None, 16, None, 16,
                            None, None) == 1
    assert b"bad act" in lib.mgcn_last_error()
    assert lib.mgcn_abi_version() == 22  # the additions are backward compatible
