"""Hard attention / VotePool without a GPU: the plain-torch restatement
(tests/hard_attention_ref.py) against the reference's own fp64 runs
(tests/golden/hatt_*.npz, vote_*.npz: 1e-12 relative on continuous tensors,
exact on the one-hot alpha, edge_index, nodes and slices), the modules'
construction surface, and the three reference defects that are not mirrored.
"""
import pytest
import torch

import hard_attention_ref as R


def rel(name, got, want, tol=1e-12):
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    if want.numel():
        err = (got - want).abs().max().item()
        assert err <= tol * max(want.abs().max().item(), 1e-300), f"{name}: {err:.3e}"


def params64(fx):
    return {k[2:]: v.double() for k, v in fx.items() if k.startswith("p_")}


# ------------------------------------------------- restatement vs fixtures
@pytest.mark.parametrize("name", list(R.TRAIN) + list(R.EVAL))
def test_restatement_node_model(name):
    training = name in R.TRAIN
    if training:
        fin, fout, H, combine, adir, act, bias, T = R.TRAIN[name]
    else:
        fin, fout, H, combine, adir, act, sample = R.EVAL[name]
        bias, T = False, 0.1
    fx = R.fixture(name)
    p = {k: v.clone().requires_grad_(True) for k, v in params64(fx).items()}
    x = fx["x"].double().requires_grad_(True)
    noise = R.noises(fx)
    assert len(noise) == (1 if training or sample else 0)
    y, alpha = R.hatt_ref(x, p["weight"], p["att_weight"], p.get("bias"), fx["edge_index"], H,
                          combine, adir, act, T, training, noise[0] if noise else None)
    y.backward(fx["dY"].double())
    rel("y", y.detach(), fx["y64"])
    rel("dx", x.grad, fx["dx64"])
    rel("dW", p["weight"].grad, fx["dW64"])
    if training:
        rel("alpha", alpha.detach(), fx["alpha64"])
        rel("datt", p["att_weight"].grad, fx["datt64"])
        if bias:
            rel("db", p["bias"].grad, fx["db64"])
    else:
        assert torch.equal(alpha, fx["alpha64"])
        assert torch.equal(fx["alpha32"].double(), fx["alpha64"])
        assert p["att_weight"].grad is None


def test_ties_fixture_is_decided_by_the_rule_alone():
    """att_weight = 0: every logit is exactly 0, the last edge of a group in
    COO order wins; duplicates exist and the quirk fires."""
    fx = R.fixture("hatt_eval_ties")
    ei, a = fx["edge_index"], fx["alpha64"]
    assert not fx["p_att_weight"].any()
    E, N = ei.size(1), fx["x"].size(0)
    assert torch.unique(ei, dim=1).size(1) < E
    last = torch.full((N,), -1, dtype=torch.long).scatter_reduce(0, ei[1], torch.arange(E), "amax")
    assert (last < 0).any()
    want = torch.zeros(E, 2, dtype=torch.float64)
    want[last[last >= 0]] = 1
    want[E - 1] = 1
    assert torch.equal(a, want)


@pytest.mark.parametrize("name", list(R.VOTE_LAYER))
def test_restatement_vote_layer(name):
    training, kw = R.VOTE_LAYER[name]
    fx = R.fixture(name)
    p = {k: v.clone().requires_grad_(True) for k, v in params64(fx).items()}
    x = fx["x"].double().requires_grad_(True)
    noise = R.noises(fx)
    xo, eo, nodes, sl, alpha = R.vote_layer_ref(p, x, fx["edge_index"], fx["slices_in"].tolist(),
                                                training, noise[0] if noise else None, **kw)
    rows = nodes if kw.get("relabel") else slice(None)
    xo.backward(fx["dY"].double()[rows])
    assert torch.equal(eo, fx["edge_out"]) and torch.equal(nodes, fx["nodes"])
    if kw.get("relabel"):
        # the reference's slices (end - kept) are recorded but wrong; the kept counts:
        assert sl == [0] + [int((nodes < e).sum()) for e in fx["slices_in"].tolist()[1:]]
        assert sl[-1] == nodes.numel() == xo.size(0)
    else:
        assert sl == fx["slices_out"].tolist()
    rel("y", xo.detach(), fx["y64"])
    rel("dx", x.grad, fx["dx64"])
    rel("dW", p["weight"].grad, fx["dW64"])
    if training:
        rel("alpha", alpha.detach(), fx["alpha64"])
        rel("datt", p["att_weight"].grad, fx["datt64"])
    else:
        assert torch.equal(alpha, fx["alpha64"])


@pytest.mark.parametrize("name", ["vote_model_eval", "vote_model_train"])
def test_restatement_vote_model(name):
    training = name.endswith("train")
    fx = R.fixture(name)
    p = {k: v.clone().requires_grad_(True) for k, v in params64(fx).items()}
    x = fx["x"].double().requires_grad_(True)
    remaining = []
    kw = {k: v for k, v in R.VOTE_MODEL_KW.items() if k not in ("nheads", "residual")}
    y = R.vote_model_ref(p, x, fx["edge_index"], [0, x.size(0)], training, R.noises(fx),
                         remaining=remaining, **kw)
    y.backward(fx["dY"].double())
    for i, nodes in enumerate(remaining):
        assert torch.equal(nodes, fx["remaining_%d" % i])
    rel("y", y.detach(), fx["y64"])
    rel("dx", x.grad, fx["dx64"])
    for k, v in p.items():
        if "g_" + k + "64" in fx:
            # self_attention.bias: a softmax is shift invariant, the true gradient is 0
            tol = 1e-12 if k != "out_net.self_attention.bias" else float("inf")
            rel("g_" + k, v.grad, fx["g_" + k + "64"], tol)
        else:
            assert v.grad is None, k  # eval: att_weight receives no gradient


# -------------------------------------------------------- module surface
def test_node_model_surface():
    from mgcn.models import NodeModelHardAttention
    import mgcn.models as M
    for name, cfg in list(R.TRAIN.items()) + list(R.EVAL.items()):
        fin, fout, H, combine, adir, act = cfg[:6]
        bias = cfg[6] if name in R.TRAIN else False
        nm = NodeModelHardAttention(fin, fout, nheads=H, att_act=act, att_combine=combine,
                                    att_dir=adir, bias=bias)
        fx = R.fixture(name)
        want = {k[2:]: tuple(v.shape) for k, v in fx.items() if k.startswith("p_")}
        assert {k: tuple(v.shape) for k, v in nm.state_dict().items()} == want
    nm = NodeModelHardAttention(8, 16, nheads=4, att_act="lrelu", bias=True, temperature=0.3)
    assert repr(nm) == ("NodeModelHardAttention (in_channels: 8, out_channels: 16, in_edgedim: "
                        "None, nheads: 4, att_activation: LeakyReLU(negative_slope=0.2),"
                        "att_dropout: 0, att_combine: cat, att_dir: in, temperature: 0.3 | "
                        "number of parameters: 176)")
    assert nm.temperature == 0.3 and nm.sample is False
    assert "NodeModelHardAttention" in M.__all__
    assert NodeModelHardAttention not in M.GCNMultiKernel.nodemodel_dict.values()
    g = M.gumbel_samples(torch.empty(50, 3))
    assert g.shape == (50, 3) and g.dtype == torch.float32 and torch.isfinite(g).all()


def test_votepool_surface():
    from mgcn import votepool as V
    for name, (_, kw) in R.VOTE_LAYER.items():
        layer = V.VotePoolLayer(12, 8, **kw)
        fx = R.fixture(name)
        want = {k[2:]: tuple(v.shape) for k, v in fx.items() if k.startswith("p_")}
        assert {k: tuple(v.shape) for k, v in layer.state_dict().items()} == want
    m = V.VotePoolModel(12, [16, 16], 3, **R.VOTE_MODEL_KW)
    fx = R.fixture("vote_model_eval")
    want = {k[2:]: tuple(v.shape) for k, v in fx.items() if k.startswith("p_")}
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
    layer = V.VotePoolLayer(12, 8, nheads=2, att_act="relu", p_keep=0.3, relabel=True)
    assert repr(layer) == ("VotePoolLayer (in_channels: 12, out_channels: 8, nheads: 2, "
                           "att_activation: ReLU(),att_dropout: 0, att_combine: cat, att_dir: out, "
                           "temperature: 0.1, sample: False, pruning_p: 0.3, pruning_relabel: True "
                           "| number of parameters: 112)")
    with pytest.raises(NotImplementedError, match="max"):
        V.VotePoolLayer(12, 8, aggr="max")
    with pytest.raises(NotImplementedError, match="max"):
        V.VotePoolModel(12, [8], 3, aggr="max")
    for fn in ("gumbel_samples", "subgraph", "get_edge_select", "prune", "VotePoolLayer",
               "SATOutLayer", "VotePoolModel"):
        assert hasattr(V, fn)


def test_cpu_tensors_raise():
    import mgcn
    from mgcn import votepool as V
    from mgcn.models import NodeModelHardAttention
    x = torch.randn(6, 12)
    ei = torch.tensor([[0, 1, 2, 3], [1, 2, 3, 0]])
    with pytest.raises(mgcn.MgcnError):
        NodeModelHardAttention(12, 8, nheads=2)(x, ei)
    with pytest.raises(mgcn.MgcnError):
        V.VotePoolLayer(12, 8, nheads=2)(x, ei, [0, 6])
    with pytest.raises(mgcn.MgcnError):
        V.VotePoolModel(12, [8], 3, nheads=2)(x, ei, [0, 6])


# ------------------------------------------------ defects that are not mirrored
def test_prune_relabel_slices_are_kept_counts():
    """Graphs [0, 4) and [4, 9); edges select nodes 1, 3 (graph 0) and 4, 7, 8
    (graph 1): the reference returns [0, 4 - 2, 9 - 5] = [0, 2, 4]; the kept
    counts below each boundary are [0, 2, 5]."""
    from mgcn.votepool import prune
    x = torch.arange(18.0).view(9, 2)
    ei = torch.tensor([[0, 1, 3, 5, 7, 8, 2], [1, 3, 1, 4, 8, 7, 0]])
    sel = torch.tensor([True, True, True, True, True, True, False])
    xo, eo, nodes, sl = prune(x.clone(), ei, sel, relabel=True, batch_slices_x=[0, 4, 9])
    assert nodes.tolist() == [1, 3, 4, 7, 8]
    assert sl == [0, 2, 5]
    assert torch.equal(xo, x[nodes])
    # induced subgraph on the kept nodes, renumbered in id order
    assert eo.tolist() == [[0, 1, 3, 4], [1, 0, 4, 3]]
    xo, eo, nodes, sl = prune(x.clone(), ei, sel, relabel=False, batch_slices_x=[0, 4, 9])
    assert sl == [0, 4, 9] and eo.tolist() == [[1, 3, 7, 8], [3, 1, 8, 7]]
    assert torch.equal(xo[nodes], x[nodes]) and torch.count_nonzero(xo[[0, 2, 5, 6]]) == 0


def test_sat_out_multi_graph_equals_single_graph():
    """The padded multi-graph formula (pad and zero rows masked, a graph with
    no row left -> proj(0)) equals the single-graph formula graph by graph."""
    g = torch.Generator().manual_seed(0)
    C, K = 6, 3
    p = {"out_net.self_attention.weight": torch.randn(1, C, generator=g, dtype=torch.float64),
         "out_net.self_attention.bias": torch.randn(1, generator=g, dtype=torch.float64),
         "out_net.proj.weight": torch.randn(K, C, generator=g, dtype=torch.float64),
         "out_net.proj.bias": torch.randn(K, generator=g, dtype=torch.float64)}
    x = torch.rand(12, C, generator=g, dtype=torch.float64)
    x[[1, 4, 5]] = 0          # pruned rows
    x[7:9] = 0                # graph [7, 9): nothing left
    slices = [0, 4, 7, 9, 12]
    multi = R.sat_out_padded_ref(p, x, slices)
    single = torch.cat([R.sat_out_ref(p, x[i:j], [0, j - i])
                        for i, j in zip(slices, slices[1:])])
    assert torch.isfinite(multi).all()
    rel("multi vs single", multi, single)
    rel("empty graph", multi[2], p["out_net.proj.bias"])


def test_get_edge_select_mask_follows_alpha_device():
    """The training-mode mask is created on alpha's device (the reference made
    it on the CPU): a CPU alpha must fail in the engine's argmax, not in an
    index_put across devices -- the error names the device."""
    import mgcn
    from mgcn.votepool import get_edge_select
    with pytest.raises(mgcn.MgcnError, match="HIP device"):
        get_edge_select(torch.zeros(3, 1), torch.tensor([[0, 1], [1, 2]]), torch.rand(2, 2))
    sel = get_edge_select(torch.zeros(3, 1), torch.tensor([[0, 1], [1, 2]]),
                          torch.tensor([[0.0, 1.0], [0.0, 0.0]]), training=False)
    assert sel.tolist() == [True, False]
