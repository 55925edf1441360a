"""Generate the attention fixtures tests/golden/att_*.npz from the REFERENCE.

    python tests/golden/make_golden_attention.py

Runs the reference's own NodeModelAttention
(src/gcn_meta/models/graph_attention.py) and, for ``att_model_citation``, its
GCNModel on the CPU under the stubs of make_golden.py (torch_scatter 1.x
restatement, PyG glorot / zeros / scatter_), twice: once as is (fp32) and once
with ``.double()`` on the same parameters.  The fp64 run is the truth the GPU
tests compare against; the fp32 run measures the reference's own rounding
error, which sets the tolerance:

    max|t_gpu - t64| <= max(4 * max|t32 - t64|, 1e-5 * max|t64|)

The fixtures hold arrays only: edge_index, x, the parameters (p_*), dY, and
y / alpha / dx / dW / datt / db (the model case: y, dx and g_<parameter>) with
the suffixes 32 and 64.  The script prints max|t32 - t64| / max|t64| of every
recorded tensor (the table in DESIGN.md).
"""
from __future__ import annotations

import copy
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import REF_SRC, _install_stubs, _t, make_graph, save  # noqa: E402

# name -> (in, out, nheads, combine, dir, act, bias, graph, N, random edges);
# sizes chosen so that every file stays under 200 KB
CASES = {
    "att_h1_cat_in_none": (16, 8, 1, "cat", "in", "none", False, "rand", 300, 2150),
    "att_h4_cat_in_lrelu_bias": (8, 16, 4, "cat", "in", "lrelu", True, "rand", 200, 1500),
    "att_h1_c7_in_lrelu": (32, 7, 1, "cat", "in", "lrelu", False, "rand", 200, 2150),
    "att_h3_mean_out_relu": (16, 5, 3, "mean", "out", "relu", False, "rand", 300, 2150),
    "att_h2_add_in_lrelu": (16, 8, 2, "add", "in", "lrelu", False, "rand", 300, 2150),
    "att_hub_in": (8, 8, 2, "cat", "in", "lrelu", False, "hub", 320, 1900),
    "att_hub_out": (8, 8, 2, "cat", "out", "lrelu", False, "hub", 320, 1900),
}


def hub_graph(rng, N=320, E=1900, isolated=20):
    """One node with in-degree 300 (node 0), one with out-degree 300 (node 1),
    `isolated` nodes without any edge, duplicate edges, no self-loops."""
    ei = make_graph(rng, N, E, self_loops=False, isolated=isolated)
    ei = ei[:, ei[0] != ei[1]]
    ei = ei[:, (ei[1] != 0) & (ei[0] != 1)]
    active = N - isolated
    into0 = np.concatenate([np.arange(2, active), [2]])        # 298 + a duplicate (+ 1 -> 0 below)
    from1 = np.concatenate([[0], np.arange(2, active), [5]])   # 299 + a duplicate
    hub = np.concatenate([np.stack([into0, np.zeros_like(into0)]),
                          np.stack([np.ones_like(from1), from1])], axis=1)
    ei = np.concatenate([ei, hub], axis=1)
    ei = ei[:, rng.permutation(ei.shape[1])]
    assert (ei[1] == 0).sum() == 300 and (ei[0] == 1).sum() == 300
    assert (ei[0] != ei[1]).all() and ei.max() < active
    return ei.astype(np.int64)


def report(name, rec):
    parts = []
    for k in sorted(rec):
        if k.endswith("64") and k[:-2] + "32" in rec:
            t64 = np.asarray(rec[k], dtype=np.float64)
            t32 = np.asarray(rec[k[:-2] + "32"], dtype=np.float64)
            parts.append("%s %.1e" % (k[:-2], np.abs(t32 - t64).max() / max(np.abs(t64).max(),
                                                                           1e-300)))
    print("%-26s %s" % (name, "  ".join(parts)))


def layer_case(ga, name, rng):
    fin, fout, H, combine, adir, act, bias, graph, N, E = CASES[name]
    if graph == "hub":
        ei = hub_graph(rng, N, E)
    else:
        ei = make_graph(rng, N, E, self_loops=True, isolated=3)
    torch.manual_seed(int(rng.integers(1 << 30)))
    nm = ga.NodeModelAttention(fin, fout, nheads=H, att_act=act, att_dropout=0,
                               att_combine=combine, att_dir=adir, bias=bias)
    if bias:
        nm.bias.data.uniform_(-0.5, 0.5)
    x = torch.randn(N, fin)
    dY = torch.randn(N, fout)
    rec = {"edge_index": ei, "x": x, "dY": dY}
    for pk, pv in nm.state_dict().items():
        rec["p_" + pk] = pv.clone()
    for tag, mod, dt in (("32", nm, torch.float32), ("64", copy.deepcopy(nm).double(),
                                                     torch.float64)):
        xx = x.detach().clone().to(dt).requires_grad_(True)
        store = []
        y = mod(xx, _t(ei), attn_store=store)
        y.backward(dY.to(dt))
        rec["y" + tag] = y.detach()
        rec["alpha" + tag] = store[0].detach()
        rec["dx" + tag] = xx.grad
        rec["dW" + tag] = mod.weight.grad
        rec["datt" + tag] = mod.att_weight.grad
        if bias:
            rec["db" + tag] = mod.bias.grad
    save(name, **rec)
    report(name, rec)


def model_case(gm, rng):
    N = 200
    ei = make_graph(rng, N, 1500, self_loops=True, isolated=2)
    torch.manual_seed(int(rng.integers(1 << 30)))
    m = gm.GCNModel(24, [32, 32, 7], 7, nheads=[2, 2, 1], residual_hop=1, nodemodel='attention',
                    bias=False, dropout=0, att_act='lrelu', att_dir='in', final_type='none')
    x = torch.randn(N, 24)
    dY = torch.randn(N, 7)
    rec = {"edge_index": ei, "x": x, "dY": dY}
    for pk, pv in m.state_dict().items():
        rec["p_" + pk] = pv.clone()
    for tag, mod, dt in (("32", m, torch.float32), ("64", copy.deepcopy(m).double(),
                                                    torch.float64)):
        xx = x.detach().clone().to(dt).requires_grad_(True)
        y = mod(xx, _t(ei))
        y.backward(dY.to(dt))
        rec["y" + tag] = y.detach()
        rec["dx" + tag] = xx.grad
        for pk, pv in mod.named_parameters():
            rec["g_" + pk + tag] = pv.grad
    save("att_model_citation", **rec)
    report("att_model_citation", rec)


def main():
    _install_stubs()
    sys.path.insert(0, REF_SRC)
    from gcn_meta.models import gcn_model, graph_attention
    rng = np.random.default_rng(20260119)
    for name in CASES:
        layer_case(graph_attention, name, rng)
    model_case(gcn_model, rng)


if __name__ == "__main__":
    main()
