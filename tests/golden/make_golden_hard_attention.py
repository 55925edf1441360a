"""Generate the hard-attention fixtures tests/golden/hatt_*.npz and
vote_*.npz from the REFERENCE.

    python tests/golden/make_golden_hard_attention.py

Runs the reference's own NodeModelHardAttention
(src/gcn_meta/models/graph_hard_attention.py) and VotePoolLayer /
VotePoolModel (gpool_hard_attention.py) on the CPU under the stubs of
make_golden.py plus one more, ``torch_geometric.utils.num_nodes
.maybe_num_nodes`` (PyG 1.3: ``index.max() + 1`` when num_nodes is None).
Every case runs twice on the same parameters and the same Gumbel noise (the
module's ``gumbel_samples`` is wrapped: the fp32 run records, the fp64 run
replays): once as is (fp32) and once with ``.double()``.  The fp64 run is the
truth the tests compare against, the fp32 run measures the reference's own
rounding error, which sets the tolerance of the attention suite:

    max|t_gpu - t64| <= max(4 * max|t32 - t64|, 1e-5 * max|t64|)

Discrete outputs (a one-hot alpha, the pruned edge_index, nodes, slices) must
be decidable, or a test of them would test rounding.  For every case the
script asserts that the fp32 and fp64 runs agree on them exactly, and that
 * every eval argmax has an fp64 top-2 gap of at least 1e-4 max|logit| (with
   the noise where sampled; hatt_eval_ties, whose logits are all exactly 0,
   is decided by the tie rule alone and is the one eval graph with duplicate
   edges); for vote_model_eval that holds for both layers, each on its own
   input and pruned edge list, and the fp32 and fp64 one-hots of both agree,
 * every training-mode selection of VotePoolLayer has a top-2 gap of alpha64
   of at least 1e-4 and, with p_keep, no alpha64 and no group maximum within
   1e-4 of p_keep.
Seeds are walked from a fixed start until that holds; the seed is recorded.

The fixtures hold arrays only: edge_index, x, dY, the noise (noise_<call>),
the parameters (p_*) and the results with the suffixes 32 and 64.  The script
prints max|t32 - t64| / max|t64| of every continuous tensor (the table in
DESIGN.md).
"""
from __future__ import annotations

import copy
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import REF_SRC, _install_stubs, _t, make_graph, save  # noqa: E402
from make_golden_attention import hub_graph, report  # noqa: E402

GAP = 1e-4
SEED0 = 20260301

# name -> (in, out, nheads, combine, dir, act, bias, T, graph, N, E)
TRAIN = {
    "hatt_train_h1_in_none_t1": (16, 8, 1, "cat", "in", "none", False, 1.0, "rand", 300, 2000),
    "hatt_train_h4_in_lrelu_bias_t01": (8, 16, 4, "cat", "in", "lrelu", True, 0.1, "rand", 200,
                                        1200),
    "hatt_train_h3_mean_out_relu_t05": (16, 5, 3, "mean", "out", "relu", False, 0.5, "rand", 300,
                                        1500),
    "hatt_train_hub_out_t05": (8, 8, 2, "cat", "out", "lrelu", False, 0.5, "hub", 320, 1500),
}
# name -> (in, out, nheads, combine, dir, act, sample, graph, N, E)
EVAL = {
    "hatt_eval_h4_in_lrelu": (8, 16, 4, "cat", "in", "lrelu", False, "noin", 120, 700),
    "hatt_eval_h3_add_out_relu_sample": (16, 5, 3, "add", "out", "relu", True, "allout", 120, 700),
    "hatt_eval_ties": (8, 8, 2, "cat", "in", "none", False, "dup", 60, 400),
}


class Noise:
    """Wraps a reference module's gumbel_samples: records the fp32 noise of
    every call, or replays the record (cast to the dtype asked for)."""

    def __init__(self, module):
        self.module, self.orig = module, module.gumbel_samples
        self.rec, self.pos, self.replay = [], 0, False
        module.gumbel_samples = self

    def __call__(self, base):
        if not self.replay:
            assert base.dtype == torch.float32
            self.rec.append(self.orig(base))
            return self.rec[-1]
        n = self.rec[self.pos]
        self.pos += 1
        assert n.shape == base.shape
        return n.to(base)

    def start_replay(self):
        self.replay, self.pos = True, 0

    def close(self):
        self.module.gumbel_samples = self.orig


def dedup(ei):
    _, first = np.unique(ei[0] * (ei.max() + 1) + ei[1], return_index=True)
    return ei[:, np.sort(first)]


def eval_graph(kind, rng, N, E):
    if kind == "dup":  # duplicates, a few nodes without in-edges
        return make_graph(rng, N, E, self_loops=False, isolated=4)
    ei = dedup(make_graph(rng, N, E, self_loops=False, isolated=0))
    if kind == "noin":  # nodes 0..9 receive nothing: the quirk fires
        return ei[:, ei[1] >= 10]
    loops = np.arange(N)  # every node has an out-edge: no quirk
    ei = ei[:, ei[0] != ei[1]]
    return np.concatenate([ei, np.stack([loops, loops])], axis=1)


def top2_gap(val, idx, N):
    """Smallest difference between the largest and the second largest value
    of a group, over all (group, column) with at least two entries."""
    val = np.asarray(val, dtype=np.float64)
    gap = np.inf
    for g in range(N):
        v = val[idx == g]
        if v.shape[0] >= 2:
            s = np.sort(v, axis=0)
            gap = min(gap, float((s[-1] - s[-2]).min()))
    return gap


def logits64(mod, x, ei, noise):
    """The fp64 pre-softmax scores act(z) (+ noise) of a reference module."""
    with torch.no_grad():
        hp = torch.mm(x.double(), mod.weight).view(-1, mod.nheads, mod.out_channels_1head)
        z = (torch.cat([hp[ei[0]], hp[ei[1]]], dim=-1) * mod.att_weight).sum(dim=-1)
        a = mod.att_act(z)
        return (a if noise is None else a + noise.double()).numpy()


def train_case(gh, name, seed):
    fin, fout, H, combine, adir, act, bias, T, graph, N, E = TRAIN[name]
    rng = np.random.default_rng(seed)
    ei = hub_graph(rng, N, E) if graph == "hub" else make_graph(rng, N, E, isolated=3)
    torch.manual_seed(seed)
    nm = gh.NodeModelHardAttention(fin, fout, nheads=H, att_act=act, att_dropout=0,
                                   att_combine=combine, att_dir=adir, bias=bias, temperature=T)
    if bias:
        nm.bias.data.uniform_(-0.5, 0.5)
    x = torch.randn(N, fin)
    dY = torch.randn(N, fout)
    rec = {"edge_index": ei, "x": x, "dY": dY, "seed": np.int64(seed)}
    for pk, pv in nm.state_dict().items():
        rec["p_" + pk] = pv.clone()
    noise = Noise(gh)
    for tag, mod, dt in (("32", nm, torch.float32), ("64", copy.deepcopy(nm).double(),
                                                     torch.float64)):
        if tag == "64":
            noise.start_replay()
        mod.train()
        xx = x.detach().clone().to(dt).requires_grad_(True)
        store = []
        y = mod(xx, _t(ei), attn_store=store)
        y.backward(dY.to(dt))
        rec["y" + tag], rec["alpha" + tag] = y.detach(), store[0].detach()
        rec["dx" + tag], rec["dW" + tag] = xx.grad, mod.weight.grad
        rec["datt" + tag] = mod.att_weight.grad
        if bias:
            rec["db" + tag] = mod.bias.grad
    noise.close()
    rec["noise_0"] = noise.rec[0]
    return rec


def eval_case(gh, name, seed):
    fin, fout, H, combine, adir, act, sample, graph, N, E = EVAL[name]
    rng = np.random.default_rng(seed)
    ei = eval_graph(graph, rng, N, E)
    torch.manual_seed(seed)
    nm = gh.NodeModelHardAttention(fin, fout, nheads=H, att_act=act, att_combine=combine,
                                   att_dir=adir, sample=sample)
    if graph == "dup":
        nm.att_weight.data.zero_()
    x = torch.randn(N, fin)
    dY = torch.randn(N, fout)
    rec = {"edge_index": ei, "x": x, "dY": dY, "seed": np.int64(seed)}
    for pk, pv in nm.state_dict().items():
        rec["p_" + pk] = pv.clone()
    noise = Noise(gh)
    for tag, mod, dt in (("32", nm, torch.float32), ("64", copy.deepcopy(nm).double(),
                                                     torch.float64)):
        if tag == "64":
            noise.start_replay()
        mod.eval()
        xx = x.detach().clone().to(dt).requires_grad_(True)
        store = []
        y = mod(xx, _t(ei), attn_store=store)
        y.backward(dY.to(dt))
        assert mod.att_weight.grad is None
        rec["y" + tag], rec["alpha" + tag] = y.detach(), store[0].detach()
        rec["dx" + tag], rec["dW" + tag] = xx.grad, mod.weight.grad
    noise.close()
    if sample:
        rec["noise_0"] = noise.rec[0]
    if not np.array_equal(rec["alpha32"].numpy(), rec["alpha64"].numpy()):
        return None
    if graph != "dup":
        lg = logits64(copy.deepcopy(nm).double(), x, _t(ei), noise.rec[0] if sample else None)
        if top2_gap(lg, ei[0] if adir == "out" else ei[1], N) < GAP * np.abs(lg).max():
            return None
    else:
        assert not logits64(copy.deepcopy(nm).double(), x, _t(ei), None).any()
    idx = ei[0] if adir == "out" else ei[1]
    empty = np.bincount(idx, minlength=N).min() == 0
    assert empty == (graph != "allout")
    return rec


# ------------------------------------------------------------------ VotePool
# name -> (training, layer kwargs)
VOTE_LAYER = {
    "vote_layer_train_h2_t05": (True, dict(nheads=2, att_act="lrelu", temperature=0.5)),
    "vote_layer_train_pkeep": (True, dict(nheads=2, att_act="lrelu", temperature=0.1,
                                          p_keep=0.3)),
    "vote_layer_train_mean": (True, dict(nheads=2, att_act="lrelu", temperature=0.5,
                                         aggr="mean")),
    "vote_layer_eval_h2": (False, dict(nheads=2, att_act="lrelu")),
    "vote_layer_eval_relabel": (False, dict(nheads=2, att_act="lrelu", relabel=True)),
}
VOTE_N = (40, 50)  # the layer cases: a batch of two graphs
VOTE_F = (12, 8)   # in, out


def vote_graph(rng, sizes, E_per):
    """Block-diagonal, deduplicated, no self-loops; the first 3 nodes of every
    graph have no out-edge (their group is empty: the quirk fires in eval)."""
    parts, off = [], 0
    for n in sizes:
        e = dedup(make_graph(rng, n, E_per, self_loops=False))
        e = e[:, (e[0] != e[1]) & (e[0] >= 3)]
        parts.append(e + off)
        off += n
    ei = np.concatenate(parts, axis=1)
    return ei[:, rng.permutation(ei.shape[1])].astype(np.int64)


def slices_of(sizes):
    return [0] + list(np.cumsum(sizes))


def vote_select_ok(alpha64, ei, N, p_keep):
    a = np.asarray(alpha64, dtype=np.float64)
    if top2_gap(a, ei[0], N) < GAP:
        return False
    if p_keep is not None:
        if np.abs(a - p_keep).min() < GAP:
            return False
        mx = np.full((N, a.shape[1]), -1e16)
        np.maximum.at(mx, ei[0], a)
        if np.abs(mx - p_keep).min() < GAP:
            return False
    return True


def vote_layer_case(gp, name, seed):
    training, kw = VOTE_LAYER[name]
    rng = np.random.default_rng(seed)
    ei = vote_graph(rng, VOTE_N, 260)
    N = sum(VOTE_N)
    torch.manual_seed(seed)
    layer = gp.VotePoolLayer(VOTE_F[0], VOTE_F[1], **kw)
    x = torch.randn(N, VOTE_F[0])
    dY = torch.randn(N, VOTE_F[1])
    rec = {"edge_index": ei, "x": x, "dY": dY, "seed": np.int64(seed),
           "slices_in": np.asarray(slices_of(VOTE_N), dtype=np.int64)}
    for pk, pv in layer.state_dict().items():
        rec["p_" + pk] = pv.clone()
    noise = Noise(gp)
    for tag, mod, dt in (("32", layer, torch.float32), ("64", copy.deepcopy(layer).double(),
                                                        torch.float64)):
        if tag == "64":
            noise.start_replay()
        mod.train(training)
        xx = x.detach().clone().to(dt).requires_grad_(True)
        store = []
        xo, eo, nodes, sl = mod(xx, _t(ei), slices_of(VOTE_N), attn_store=store)
        rows = nodes if kw.get("relabel") else slice(None)
        xo.backward(dY.to(dt)[rows])
        rec["y" + tag], rec["alpha" + tag] = xo.detach(), store[0].detach()
        rec["dx" + tag], rec["dW" + tag] = xx.grad, mod.weight.grad
        if training:
            rec["datt" + tag] = mod.att_weight.grad
        rec["edge_out" + tag], rec["nodes" + tag] = eo, nodes
        rec["slices_out" + tag] = np.asarray(sl, dtype=np.int64)
    noise.close()
    if noise.rec:
        rec["noise_0"] = noise.rec[0]
    for k in ("edge_out", "nodes", "slices_out"):
        if not np.array_equal(np.asarray(rec[k + "32"]), np.asarray(rec[k + "64"])):
            return None
        rec[k] = rec.pop(k + "64")
        del rec[k + "32"]
    if training:
        if not vote_select_ok(rec["alpha64"], ei, N, kw.get("p_keep")):
            return None
    else:
        if not np.array_equal(rec["alpha32"].numpy(), rec["alpha64"].numpy()):
            return None
        lg = logits64(copy.deepcopy(layer).double(), x, _t(ei), None)
        if top2_gap(lg, ei[0], N) < GAP * np.abs(lg).max():
            return None
    return rec


def vote_model_case(gp, name, seed):
    training = name.endswith("train")
    rng = np.random.default_rng(seed)
    N = 60
    ei = vote_graph(rng, (N,), 420)
    torch.manual_seed(seed)
    m = gp.VotePoolModel(12, [16, 16], 3, residual=True, nheads=[2, 2], att_act="lrelu",
                         temperature=0.5, relabel=False)
    x = torch.randn(N, 12)
    dY = torch.randn(1, 3)
    rec = {"edge_index": ei, "x": x, "dY": dY, "seed": np.int64(seed)}
    for pk, pv in m.state_dict().items():
        rec["p_" + pk] = pv.clone()
    noise = Noise(gp)
    orig_select, orig_forward = gp.get_edge_select, gp.VotePoolLayer.forward
    alphas, inputs = {"32": [], "64": []}, {"32": [], "64": []}
    run = ["32"]

    def spy(x_, edge_index, alpha, training=True, p_keep=None):
        alphas[run[0]].append((alpha.detach().clone(), edge_index.clone(), x_.size(0)))
        return orig_select(x_, edge_index, alpha, training=training, p_keep=p_keep)

    def spy_forward(self, x_, edge_index, batch_slices_x, attn_store=None):
        inputs[run[0]].append((self, x_.detach().clone(), edge_index.clone()))
        return orig_forward(self, x_, edge_index, batch_slices_x, attn_store=attn_store)

    gp.get_edge_select, gp.VotePoolLayer.forward = spy, spy_forward
    for tag, mod, dt in (("32", m, torch.float32), ("64", copy.deepcopy(m).double(),
                                                    torch.float64)):
        run[0] = tag
        if tag == "64":
            noise.start_replay()
        mod.train(training)
        xx = x.detach().clone().to(dt).requires_grad_(True)
        remaining = []
        y = mod(xx, _t(ei), [0, N], remaining_nodes=remaining)
        y.backward(dY.to(dt))
        rec["y" + tag], rec["dx" + tag] = y.detach(), xx.grad
        for pk, pv in mod.named_parameters():
            if pv.grad is not None:
                rec["g_" + pk + tag] = pv.grad
        for i, nodes in enumerate(remaining):
            rec["remaining_%d_%s" % (i, tag)] = nodes
    gp.get_edge_select, gp.VotePoolLayer.forward = orig_select, orig_forward
    noise.close()
    for i, n in enumerate(noise.rec):
        rec["noise_%d" % i] = n
    for i in range(2):
        a, b = rec.pop("remaining_%d_32" % i), rec.pop("remaining_%d_64" % i)
        if not np.array_equal(a.numpy(), b.numpy()):
            return None
        rec["remaining_%d" % i] = b
    if training:
        for alpha, e, n in alphas["64"]:  # the fp64 run's selections
            if e.size(1) and not vote_select_ok(alpha.numpy(), e.numpy(), n, None):
                return None
        return rec
    # eval: every layer's one-hot agrees between fp32 and fp64, and every layer's
    # fp64 argmax (over the layer's own input and pruned edge list) is decided
    for (a32, _, _), (a64, _, _) in zip(alphas["32"], alphas["64"]):
        if not np.array_equal(a32.numpy(), a64.numpy()):
            return None
    for layer, xin, e in inputs["64"]:
        if not e.size(1):
            return None
        lg = logits64(layer, xin, e, None)
        if top2_gap(lg, e[0].numpy(), xin.size(0)) < GAP * np.abs(lg).max():
            return None
    if len(rec["remaining_1"]) < 2:
        return None
    return rec


def walk(fn, mod, name):
    for seed in range(SEED0, SEED0 + 200):
        rec = fn(mod, name, seed)
        if rec is not None:
            save(name, **rec)
            report("%s (seed +%d)" % (name, seed - SEED0),
                   {k: v for k, v in rec.items() if not k.startswith(("edge_", "nodes", "slices",
                                                                      "remaining", "seed"))})
            return
    raise SystemExit("no decidable seed for " + name)


def main():
    _install_stubs()
    nn_mod = types.ModuleType("torch_geometric.utils.num_nodes")
    nn_mod.maybe_num_nodes = lambda index, num_nodes=None: (
        int(index.max()) + 1 if num_nodes is None else num_nodes)
    sys.modules["torch_geometric.utils.num_nodes"] = nn_mod
    sys.path.insert(0, REF_SRC)
    from gcn_meta.models import gpool_hard_attention, graph_hard_attention
    for name in TRAIN:
        walk(train_case, graph_hard_attention, name)
    for name in EVAL:
        walk(eval_case, graph_hard_attention, name)
    for name in VOTE_LAYER:
        walk(vote_layer_case, gpool_hard_attention, name)
    for name in ("vote_model_eval", "vote_model_train"):
        walk(vote_model_case, gpool_hard_attention, name)


if __name__ == "__main__":
    main()
