"""Shared reference side of the hard-attention / VotePool tests (a plain
helper module, not collected): a plain-torch restatement of
graph_hard_attention.py's NodeModelHardAttention.forward and of
gpool_hard_attention.py's VotePoolLayer / SATOutLayer / VotePoolModel
forwards, with the Gumbel noise as an argument, at the dtype of ``x``; the
fixture loader; and the noise replay used by the module tests.

tests/test_votepool_host.py holds the restatement to the reference's own fp64
fixtures (tests/golden/make_golden_hard_attention.py) at 1e-12 relative, and
exactly on every discrete output.  Where the reference has a defect that the
project does not mirror (votepool.py's docstring lists the three), the
restatement states the project's behaviour; none of the fixtures reaches one
of them except the relabel=True slices, which are not compared.
"""
import contextlib
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# name -> (in, out, nheads, combine, dir, act, bias, T)  (make_golden_hard_attention.py TRAIN)
TRAIN = {
    "hatt_train_h1_in_none_t1": (16, 8, 1, "cat", "in", "none", False, 1.0),
    "hatt_train_h4_in_lrelu_bias_t01": (8, 16, 4, "cat", "in", "lrelu", True, 0.1),
    "hatt_train_h3_mean_out_relu_t05": (16, 5, 3, "mean", "out", "relu", False, 0.5),
    "hatt_train_hub_out_t05": (8, 8, 2, "cat", "out", "lrelu", False, 0.5),
}
# name -> (in, out, nheads, combine, dir, act, sample)
EVAL = {
    "hatt_eval_h4_in_lrelu": (8, 16, 4, "cat", "in", "lrelu", False),
    "hatt_eval_h3_add_out_relu_sample": (16, 5, 3, "add", "out", "relu", True),
    "hatt_eval_ties": (8, 8, 2, "cat", "in", "none", False),
}
# name -> (training, layer kwargs); 12 -> 8 channels, slices [0, 40, 90]
VOTE_LAYER = {
    "vote_layer_train_h2_t05": (True, dict(nheads=2, att_act="lrelu", temperature=0.5)),
    "vote_layer_train_pkeep": (True, dict(nheads=2, att_act="lrelu", temperature=0.1,
                                          p_keep=0.3)),
    "vote_layer_train_mean": (True, dict(nheads=2, att_act="lrelu", temperature=0.5,
                                         aggr="mean")),
    "vote_layer_eval_h2": (False, dict(nheads=2, att_act="lrelu")),
    "vote_layer_eval_relabel": (False, dict(nheads=2, att_act="lrelu", relabel=True)),
}
VOTE_MODEL_KW = dict(residual=True, nheads=[2, 2], att_act="lrelu", temperature=0.5,
                     relabel=False)

_FIX = {}


def fixture(name):
    """The arrays of tests/golden/<name>.npz as torch tensors (loaded once)."""
    if name not in _FIX:
        with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
            _FIX[name] = {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}
    return _FIX[name]


def noises(fx):
    return [fx[k] for k in sorted((k for k in fx if k.startswith("noise_")),
                                  key=lambda k: int(k.split("_")[1]))]


@contextlib.contextmanager
def replay_noise(module, recorded, device):
    """Replace ``module.gumbel_samples`` by a replay of ``recorded`` (COO
    order), in call order; checks the calling contract and that every record
    was consumed."""
    calls = []
    orig = module.gumbel_samples

    def replay(base):
        assert base.dtype == torch.float32 and base.dim() == 2
        n = recorded[len(calls)]
        assert tuple(base.shape) == tuple(n.shape), (base.shape, n.shape)
        calls.append(1)
        return n.to(device=base.device, dtype=base.dtype)

    module.gumbel_samples = replay
    try:
        yield calls
    finally:
        module.gumbel_samples = orig
    assert len(calls) == len(recorded), (len(calls), len(recorded))


# --------------------------------------------------------------- the scan
def scan_argmax(l, idx, N):
    """torch_scatter 1.x's CPU scatter_max(l, idx, fill_value=-1e16) argmax for
    l [E, H]: sequential in edge order with ``l >= best`` from -1e16, so the
    last of equal maxima wins, a value below -1e16 or a NaN never does, an
    empty group has -1.  Vectorised: the largest edge id among the entries
    that equal the group maximum of the admissible entries."""
    E, H = l.shape
    ok = l >= -1e16  # False for NaN
    ix = idx.view(-1, 1).expand(-1, H)
    lv = torch.where(ok, l, torch.full_like(l, -1e16))
    m = torch.full((N, H), -1e16, dtype=l.dtype).scatter_reduce(0, ix, lv, "amax")
    eid = torch.arange(E).view(-1, 1).expand(-1, H)
    cand = torch.where(ok & (lv == m[idx]), eid, torch.full_like(eid, -1))
    return torch.full((N, H), -1, dtype=torch.long).scatter_reduce(0, ix, cand, "amax")


def one_hot(argmax, E):
    """graph_hard_attention.py:118-123, literally: argmax -1 marks flat index
    E h - 1 of the transposed array."""
    H = argmax.size(1)
    flat = torch.zeros(H * E)
    if E:
        flat[(argmax + E * torch.arange(H)).view(-1)] = 1.0
    return flat.reshape(H, E).t()


_ACT = {"none": lambda t: t, "lrelu": lambda t: torch.nn.functional.leaky_relu(t, 0.2),
        "relu": torch.relu}


def hatt_ref(x, W, att, bias, ei, H, combine, adir, act, T, training, noise=None, mask=None,
             aggr="add", alpha_eval=None):
    """NodeModelHardAttention.forward / the message passing of VotePoolLayer
    in plain torch; returns (y, alpha [E, H]).  ``alpha_eval`` replaces the
    eval branch's own one-hot (to follow a selection made elsewhere)."""
    N = x.size(0)
    src, dst = ei[0], ei[1]
    hp = (x @ W).view(N, H, -1)
    xj, xi = hp[src], hp[dst]
    e = _ACT[act]((torch.cat([xj, xi], dim=-1) * att).sum(dim=-1))
    idx = src if adir == "out" else dst
    if training:
        l = (e + (0 if noise is None else noise.to(x.dtype))) / T
        ix = idx.view(-1, 1).expand(-1, H)
        m = torch.full((N, H), -1e16, dtype=x.dtype).scatter_reduce(0, ix, l.detach(), "amax")
        p = (l - m[idx]).exp()
        s = torch.zeros(N, H, dtype=x.dtype).index_add(0, idx, p)
        alpha = p / (s[idx] + 1e-16)
        if mask is not None:
            alpha = alpha * mask.to(x.dtype)
    else:
        l = e.detach() if noise is None else e.detach() + noise.to(x.dtype)
        alpha = one_hot(scan_argmax(l, idx, N), ei.size(1)) if alpha_eval is None else alpha_eval
        alpha = alpha.to(x.dtype)
    y = torch.zeros_like(hp).index_add(0, dst, xj * alpha.unsqueeze(-1))
    if aggr == "mean":
        cnt = torch.bincount(dst, minlength=N).clamp(min=1).to(x.dtype)
        y = y / cnt.view(-1, 1, 1)
    if combine == "cat":
        y = y.reshape(N, -1)
    elif combine == "add":
        y = y.sum(dim=1)
    else:
        y = y.mean(dim=1)
    if bias is not None:
        y = y + bias
    return y, alpha


# ---------------------------------------------------------------- VotePool
def edge_select_ref(N, ei, alpha, training, p_keep):
    if not training:
        return alpha.sum(dim=1) > 0
    argmax = scan_argmax(alpha, ei[0], N)
    if p_keep is None:
        sel = torch.zeros(alpha.size(0), dtype=torch.bool)
        sel[argmax.view(-1)] = True  # -1: the last edge
        return sel
    H = alpha.size(1)
    out = torch.full((N, H), -1e16, dtype=alpha.dtype).scatter_reduce(
        0, ei[0].view(-1, 1).expand(-1, H), alpha, "amax")
    node_keep = (out < p_keep).sum(dim=1) > 0
    return ((alpha >= p_keep).sum(dim=1) > 0) | node_keep[ei[0]]


def prune_ref(x, ei, sel, relabel, slices):
    nodes = ei[1, sel].unique()
    n_mask = torch.zeros(x.size(0), dtype=torch.bool)
    n_mask[nodes] = True
    ei = ei[:, n_mask[ei[0]] & n_mask[ei[1]]]
    if relabel:
        n_idx = torch.zeros(x.size(0), dtype=torch.long)
        n_idx[nodes] = torch.arange(nodes.size(0))
        return x[nodes], n_idx[ei], nodes, [0] + [int((nodes < e).sum()) for e in slices[1:]]
    return x * n_mask.view(-1, 1).to(x.dtype), ei, nodes, slices


def vote_layer_ref(p, x, ei, slices, training, noise, nheads=1, att_act="none",
                   att_combine="cat", aggr="add", temperature=0.1, p_keep=None, relabel=False):
    """VotePoolLayer.forward; ``p`` holds weight / att_weight (/ bias) at the
    dtype of x.  Returns (x, edge_index, nodes, slices, alpha)."""
    y, alpha = hatt_ref(x, p["weight"], p["att_weight"], p.get("bias"), ei, nheads, att_combine,
                        "out", att_act, temperature, training, noise, aggr=aggr)
    sel = edge_select_ref(x.size(0), ei, alpha.detach(), training, p_keep)
    return prune_ref(y, ei, sel, relabel, slices) + (alpha,)


def sat_out_ref(p, x, slices, prefix="out_net."):
    """SATOutLayer.forward: per graph, softmax self-attention over the rows
    whose sum exceeds 1e-20, then the projection; no row: proj(0)."""
    wa, ba = p[prefix + "self_attention.weight"], p[prefix + "self_attention.bias"]
    wp, bp = p[prefix + "proj.weight"], p[prefix + "proj.bias"]
    outs = []
    for i, j in zip(slices, slices[1:]):
        g = x[i:j]
        g = g[g.sum(dim=1) > 1e-20]
        w = torch.softmax(g @ wa.t() + ba, dim=0)
        outs.append((g * w).sum(dim=0, keepdim=True) @ wp.t() + bp)
    return torch.cat(outs, dim=0)


def sat_out_padded_ref(p, x, slices, prefix="out_net."):
    """The multi-graph formula as votepool.SATOutLayer states it (padding,
    -inf on padded and zero rows, an all-masked graph softened to zeros)."""
    wa, ba = p[prefix + "self_attention.weight"], p[prefix + "self_attention.bias"]
    wp, bp = p[prefix + "proj.weight"], p[prefix + "proj.bias"]
    xb = torch.nn.utils.rnn.pad_sequence([x[i:j] for i, j in zip(slices, slices[1:])],
                                         batch_first=True)
    valid = xb.sum(dim=-1) > 1e-20
    sc = (xb @ wa.t() + ba).masked_fill(~valid.unsqueeze(2), float("-inf"))
    sc = sc.masked_fill(~valid.any(dim=1).view(-1, 1, 1), 0.0)
    w = torch.softmax(sc, dim=1) * valid.unsqueeze(2)
    return (xb * w).sum(dim=1) @ wp.t() + bp


def vote_model_ref(p, x, ei, slices, training, noise_list, enc=(16, 16), remaining=None,
                   nheads=(2, 2), residual=True, **kw):
    """VotePoolModel.forward (non_linear relu, dropout 0)."""
    relabel = kw.get("relabel", False)
    for n in range(len(enc)):
        lp = {k.split(".", 2)[2]: v for k, v in p.items() if k.startswith("gpool_net.%d." % n)}
        noise = noise_list[n] if (training or kw.get("sample")) else None
        xo, ei, nodes, slices, _ = vote_layer_ref(lp, x, ei, slices, training, noise,
                                                  nheads=nheads[n], **kw)
        if residual:
            xr = x @ p["residual_net.%d.weight" % n].t() + p["residual_net.%d.bias" % n]
            if relabel:
                xr = xr[nodes]
            else:
                keep = torch.zeros(xr.size(0), 1, dtype=xr.dtype)
                keep[nodes] = 1
                xr = xr * keep
            x = torch.relu(xo + xr)
        else:
            x = torch.relu(xo)
        if remaining is not None:
            remaining.append(nodes)
    return sat_out_ref(p, x, slices)
