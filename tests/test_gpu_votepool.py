"""mgcn.votepool on the GPU (MI355X): VotePoolLayer and VotePoolModel against
the reference's own runs (tests/golden/vote_*.npz, Gumbel noise replayed in
call order), batching, and relabelling.

Continuous tensors use attention_ref.check,

    max|t_gpu - t64| <= max(4 * max|t32 - t64|, 1e-5 * max|t64|)

with t32 / t64 the reference's fp32 / fp64 runs (fixtures) or the restatement
hard_attention_ref on the CPU; the one-hot alpha, the pruned edge_index, nodes
and slices must be equal.
"""
import numpy as np
import pytest
import torch

import hard_attention_ref as R
from attention_ref import check

pytestmark = pytest.mark.gpu


def load_into(mod, fx, cuda):
    mod.load_state_dict({k[2:]: v for k, v in fx.items() if k.startswith("p_")})
    return mod.to(cuda)


@pytest.mark.parametrize("name", list(R.VOTE_LAYER))
def test_fixture_layer(cuda, name):
    from mgcn import votepool as V
    training, kw = R.VOTE_LAYER[name]
    fx = R.fixture(name)
    layer = load_into(V.VotePoolLayer(12, 8, **kw), fx, cuda).train(training)
    x = fx["x"].to(cuda).requires_grad_(True)
    store = []
    with R.replay_noise(V, R.noises(fx), cuda):
        xo, eo, nodes, sl = layer(x, fx["edge_index"].to(cuda), fx["slices_in"].tolist(),
                                  attn_store=store)
    rows = nodes if kw.get("relabel") else slice(None)
    xo.backward(fx["dY"].to(cuda)[rows])
    assert eo.device.type == "cuda" and torch.equal(eo.cpu(), fx["edge_out"])
    assert torch.equal(nodes.cpu(), fx["nodes"])
    if kw.get("relabel"):
        # not the reference's (end - kept): the kept counts below each boundary
        assert sl == [0] + [int((fx["nodes"] < e).sum()) for e in fx["slices_in"].tolist()[1:]]
    else:
        assert sl == fx["slices_out"].tolist()
    check(f"{name}.y", xo, fx["y32"], fx["y64"])
    check(f"{name}.dx", x.grad, fx["dx32"], fx["dx64"])
    check(f"{name}.dW", layer.weight.grad, fx["dW32"], fx["dW64"])
    if training:
        check(f"{name}.alpha", store[0], fx["alpha32"], fx["alpha64"])
        check(f"{name}.datt", layer.att_weight.grad, fx["datt32"], fx["datt64"])
    else:
        assert torch.equal(store[0].cpu().double(), fx["alpha64"])
        assert layer.att_weight.grad is None


@pytest.mark.parametrize("name", ["vote_model_eval", "vote_model_train"])
def test_fixture_model(cuda, name):
    from mgcn import votepool as V
    training = name.endswith("train")
    fx = R.fixture(name)
    m = load_into(V.VotePoolModel(12, [16, 16], 3, **R.VOTE_MODEL_KW), fx, cuda).train(training)
    x = fx["x"].to(cuda).requires_grad_(True)
    remaining = []
    with R.replay_noise(V, R.noises(fx), cuda):
        y = m(x, fx["edge_index"].to(cuda), [0, x.size(0)], remaining_nodes=remaining)
    y.backward(fx["dY"].to(cuda))
    for i, nodes in enumerate(remaining):
        assert torch.equal(nodes.cpu(), fx["remaining_%d" % i])
    check(f"{name}.y", y, fx["y32"], fx["y64"])
    check(f"{name}.dx", x.grad, fx["dx32"], fx["dx64"])
    for k, v in m.named_parameters():
        if k == "out_net.self_attention.bias":
            # a softmax is shift invariant: the true gradient is 0 and t32 / t64 are
            # both rounding residue.  It is the sum of the score gradients whose
            # x-weighted sum is self_attention.weight's gradient, so it is held to
            # the project's dense-product bound, 1e-5, on that gradient's scale.
            scale = fx["g_out_net.self_attention.weight64"].abs().max().item()
            assert v.grad.abs().max().item() <= 1e-5 * scale
        elif "g_" + k + "64" in fx:
            check(f"{name}.g_{k}", v.grad, fx["g_" + k + "32"], fx["g_" + k + "64"])
        else:
            assert v.grad is None, k  # eval: att_weight receives no gradient


# ------------------------------------------------------ batching, relabel
def two_graphs(seed=5, sizes=(30, 40), E_per=200):
    """Two deduplicated random graphs without self-loops; nodes 0..2 of each
    have no out-edge (an empty argmax group in eval, so the reference's quirk
    marks the last edge of whatever edge list a layer sees).  That edge
    differs between a batch and its single graphs, so each graph's list ends
    with c -> a, a -> b on three extra nodes whose only out-edges these are:
    a -> b is then the winner of a's group on every head anyway, a (voted by
    c) and b (voted by a) are kept, and the pruned list ends with a -> b
    again: the quirk fires in every layer and changes nothing."""
    rng = np.random.default_rng(seed)
    parts = []
    for n in sizes:
        e = rng.integers(0, n - 3, (2, E_per))
        e = np.unique(e[:, (e[0] != e[1]) & (e[0] >= 3)], axis=1)
        e = e[:, rng.permutation(e.shape[1])]
        parts.append(np.concatenate([e, [[n - 3, n - 2], [n - 2, n - 1]]], axis=1))
    return [torch.from_numpy(p.astype(np.int64)) for p in parts], list(sizes)


def model_and_params(cuda, **kw):
    from mgcn import votepool as V
    torch.manual_seed(11)
    base = dict(R.VOTE_MODEL_KW)
    base.update(kw)
    m = V.VotePoolModel(12, [16, 16], 3, **base).to(cuda)
    p = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    return m, p


def test_model_batch_equals_single_graphs(cuda):
    """A batch of two graphs gives, row by row, the output of the two
    single-graph runs (multi-graph read-out = single-graph read-out), to the
    bound of the restatement's single-graph runs; the kept nodes agree."""
    eis, sizes = two_graphs()
    m, p = model_and_params(cuda)
    m.eval()
    g = torch.Generator().manual_seed(2)
    xs = [torch.randn(n, 12, generator=g) for n in sizes]
    ei_b = torch.cat([eis[0], eis[1] + sizes[0]], dim=1)
    rem_b = []
    with torch.no_grad():
        yb = m(torch.cat(xs).to(cuda), ei_b.to(cuda), [0, sizes[0], sum(sizes)],
               remaining_nodes=rem_b)
    assert yb.shape == (2, 3)
    off = 0
    for i, (x, ei, n) in enumerate(zip(xs, eis, sizes)):
        rem = []
        with torch.no_grad():
            y1 = m(x.to(cuda), ei.to(cuda), [0, n], remaining_nodes=rem)
        r32 = R.vote_model_ref(p, x, ei, [0, n], False, [], **{
            k: v for k, v in R.VOTE_MODEL_KW.items() if k not in ("nheads", "residual")})
        p64 = {k: v.double() for k, v in p.items()}
        rem64 = []
        r64 = R.vote_model_ref(p64, x.double(), ei, [0, n], False, [], remaining=rem64, **{
            k: v for k, v in R.VOTE_MODEL_KW.items() if k not in ("nheads", "residual")})
        for lay in range(2):
            in_graph = rem_b[lay][(rem_b[lay] >= off) & (rem_b[lay] < off + n)] - off
            assert torch.equal(in_graph, rem[lay])
            assert torch.equal(rem[lay].cpu(), rem64[lay])
        check(f"single{i}.y", y1, r32, r64)
        check(f"batch{i}.y", yb[i:i + 1], r32, r64)
        off += n


def test_sat_out_layer_graph_with_no_row_left(cuda):
    """SATOutLayer on a batch in which one graph has only zero rows (all of it
    pruned) and the others have some: the module's padded branch equals the
    single-graph formula graph by graph, the emptied graph gives proj(0) = the
    projection's bias, and gradients stay finite."""
    from mgcn.votepool import SATOutLayer
    torch.manual_seed(21)
    C, K = 6, 3
    layer = SATOutLayer(C, K).to(cuda)
    p = {"out_net." + k: v.detach().cpu() for k, v in layer.state_dict().items()}
    g = torch.Generator().manual_seed(0)
    x = torch.rand(12, C, generator=g)
    x[[1, 4, 5]] = 0
    x[7:9] = 0                # graph [7, 9): nothing left
    slices = [0, 4, 7, 9, 12]
    xg = x.to(cuda).requires_grad_(True)
    out = layer(xg, slices)
    out.sum().backward()
    assert out.shape == (4, K)
    assert torch.isfinite(xg.grad).all()
    assert all(torch.isfinite(q.grad).all() for q in layer.parameters())
    r32 = R.sat_out_ref(p, x, slices)
    r64 = R.sat_out_ref({k: v.double() for k, v in p.items()}, x.double(), slices)
    check("sat_out.batch", out, r32, r64)
    assert torch.equal(out[2].detach().cpu(), p["out_net.proj.bias"])
    assert torch.count_nonzero(xg.grad[7:9]) == 0
    # a single all-zero graph through the single-graph branch: proj(0) as well
    one = layer(torch.zeros(3, C, device=cuda), [0, 3])
    assert torch.equal(one[0].detach().cpu(), p["out_net.proj.bias"])


@pytest.mark.parametrize("training", [False, True])
def test_relabel_equals_no_relabel(cuda, training):
    """relabel=True drops the rows that relabel=False zeroes: the layer's
    kept rows and the model's output agree (same parameters, same noise)."""
    from mgcn import votepool as V
    eis, sizes = two_graphs(seed=6)
    ei = torch.cat([eis[0], eis[1] + sizes[0]], dim=1).to(cuda)
    slices = [0, sizes[0], sum(sizes)]
    g = torch.Generator().manual_seed(3)
    x = torch.randn(sum(sizes), 12, generator=g).to(cuda)
    m0, p = model_and_params(cuda, relabel=False)
    m1, _ = model_and_params(cuda, relabel=True)
    m1.load_state_dict(m0.state_dict())
    m0.train(training), m1.train(training)
    # layer 0 sees the same graph in both models, so one noise record serves both
    E = ei.size(1)
    noise0 = -torch.log(-torch.log(torch.rand(E, 2, generator=g) + 1e-20) + 1e-20)
    l0, l1 = m0.gpool_net[0], m1.gpool_net[0]
    with R.replay_noise(V, [noise0] if training else [], cuda):
        xa, ea, na, sa = l0(x, ei, slices)
    with R.replay_noise(V, [noise0] if training else [], cuda):
        xb, eb, nb, sb = l1(x, ei, slices)
    assert torch.equal(na, nb)
    assert torch.equal(xa[na], xb) and xb.size(0) == nb.numel() == sb[-1]
    keep = torch.zeros(sum(sizes), dtype=torch.bool, device=cuda)
    keep[na] = True
    assert torch.count_nonzero(xa[~keep]) == 0
    assert sa == slices and sb == [0] + [int((nb < e).sum()) for e in slices[1:]]
    # the relabelled edges are the kept edges under the kept nodes' ranks
    rank = torch.cumsum(keep, 0) - 1
    assert torch.equal(eb, rank[ea])
    if training:
        return  # deeper layers would need noise aligned across different edge lists
    with torch.no_grad():
        y0 = m0(x, ei, slices)
        y1 = m1(x, ei, slices)
    p64 = {k: v.double() for k, v in p.items()}
    kw = {k: v for k, v in R.VOTE_MODEL_KW.items() if k not in ("nheads", "residual", "relabel")}
    r32 = R.vote_model_ref(p, x.cpu(), ei.cpu(), slices, False, [], relabel=False, **kw)
    r64 = R.vote_model_ref(p64, x.cpu().double(), ei.cpu(), slices, False, [], relabel=False, **kw)
    r64r = R.vote_model_ref(p64, x.cpu().double(), ei.cpu(), slices, False, [], relabel=True, **kw)
    assert (r64 - r64r).abs().max().item() <= 1e-12 * r64.abs().max().item()
    check("relabel.y0", y0, r32, r64)
    check("relabel.y1", y1, r32, r64)
