"""Shared reference side of the multi-kernel tests (a plain helper module, not
collected): the tolerance, the fixture table and a plain-torch restatement of
the reference's GCNMultiKernel over plain NodeModelAdditive kernels
(gcn_multi_kernel.py:76-114 on gcn_base_models.py:199-243).

Every comparison uses the attention tests' tolerance, per compared tensor t:

    max|t_gpu - t64| <= max(4 * max|t32 - t64|, 1e-5 * max|t64|)

t32 / t64 are the reference's own fp32 and fp64 results (golden fixtures
mk_*.npz, tests/golden/make_golden_multi_kernel.py) or, for the random cases,
the restatement below run in fp32 and fp64 on the CPU.

``kernel_combine`` 'mean' and 'cat' follow mgcn.models (and the reference's
intent): the sum over the kernels with edges divided by their number, and
``torch.cat`` along the channels; the reference itself raises for both when
K > 1 (``if xo == 0`` on a tensor, gcn_multi_kernel.py:100, 103).
"""
import numpy as np
import torch

from attention_ref import check  # noqa: F401  (the shared bound)
from edge_gate_ref import gate_layer_ref

FIN, FOUT, N, E = 16, 32, 300, 1815

# name -> dict(K, deg_norm, aggr, combine, bias, and the optional keys
#   lists: kernel 0 takes an edge_weight, kernel 1 a deg (both passed as K-lists)
#   empty: kernel 1 has 20 further nodes without an in-edge
#   skip:  index of a kernel whose edge_index is None
#   fout:  output channels per kernel (cat: 16 and 8, so that y stays within [300, 32]))
FIXTURES = {
    "mk_add_k2_sm_add_bias": dict(K=2, deg_norm="sm", aggr="add", combine="add", bias=True),
    "mk_add_k3_sm_mean_bias": dict(K=3, deg_norm="sm", aggr="mean", combine="add", bias=True),
    "mk_add_k2_rw_add": dict(K=2, deg_norm="rw", aggr="add", combine="add", bias=False),
    "mk_add_k3_rw_mean_bias": dict(K=3, deg_norm="rw", aggr="mean", combine="add", bias=True),
    "mk_add_k3_none_add": dict(K=3, deg_norm=None, aggr="add", combine="add", bias=False),
    "mk_add_k2_none_mean_bias": dict(K=2, deg_norm=None, aggr="mean", combine="add", bias=True),
    "mk_add_k2_sm_add_lists": dict(K=2, deg_norm="sm", aggr="add", combine="add", bias=True,
                                   lists=True),
    "mk_add_k2_sm_add_empty": dict(K=2, deg_norm="sm", aggr="add", combine="add", bias=True,
                                   empty=True),
    "mk_add_k3_sm_add_skip": dict(K=3, deg_norm="sm", aggr="add", combine="add", bias=True,
                                  skip=1),
    "mk_mean_k2_sm_add_bias": dict(K=2, deg_norm="sm", aggr="add", combine="mean", bias=True),
    "mk_mean_k3_rw_mean": dict(K=3, deg_norm="rw", aggr="mean", combine="mean", bias=False),
    "mk_cat_k2_sm_add_bias": dict(K=2, deg_norm="sm", aggr="add", combine="cat", bias=True,
                                  fout=16),
    "mk_cat_k3_none_mean": dict(K=3, deg_norm=None, aggr="mean", combine="cat", bias=False,
                                fout=8),
}
MODEL_FIXTURE = "mk_model"
MODEL_ARGS = dict(in_channels=FIN, enc_sizes=[32] * 3, num_classes=2, non_linear='relu',
                  non_linear_layer_wise='relu', residual_hop=1, dropout=0,
                  final_layer_config=None, final_type='proj', pred_on='node', nodemodel='additive',
                  deg_norm='sm', edge_gate=None, aggr='add', bias=True, num_kernel=2)
ISOLATED = 3  # the last nodes of every fixture graph have no edge in any kernel


# ------------------------------------------------------ torch restatement
def multi_layer_ref(x, Ws, bs, eis, deg_norm, aggr, combine, degs=None, ews=None, relu=False):
    """gcn_multi_kernel.py:93-112 in plain torch (the dtype of x): kernels
    whose edge_index is None are skipped, 'mean' divides by the number left."""
    K = len(eis)
    degs = degs or [None] * K
    ews = ews or [None] * K
    outs = []
    for W, b, ei, deg, ew in zip(Ws, bs, eis, degs, ews):
        if ei is None:
            continue
        outs.append(gate_layer_ref(x, {"weight_node": W, "bias": b}, ei, None, deg_norm, aggr,
                                   edge_weight=ew if deg_norm is not None else None, deg=deg)[0])
    if combine == "cat":
        y = torch.cat(outs, dim=1)
    else:
        y = outs[0]
        for o in outs[1:]:
            y = y + o
        if combine == "mean":
            y = y / len(outs)
    return torch.relu(y) if relu else y


def ref_run(x, Ws, bs, eis, dY, deg_norm, aggr, combine, dtype, degs=None, ews=None, relu=False):
    """Forward and backward of the restatement in ``dtype``: y, dx, g_W (list),
    g_b (list, None where there is no bias or the kernel is skipped)."""
    def leaf(t):
        return None if t is None else t.detach().clone().to(dtype).requires_grad_(True)

    def plain(t):
        return None if t is None else t.detach().to(dtype)
    xx = leaf(x)
    WW, bb = [leaf(W) for W in Ws], [leaf(b) for b in bs]
    y = multi_layer_ref(xx, WW, bb, eis, deg_norm, aggr, combine,
                        None if degs is None else [plain(d) for d in degs],
                        None if ews is None else [plain(w) for w in ews], relu)
    (y * dY.to(dtype)).sum().backward()
    return {"y": y.detach(), "dx": xx.grad, "g_W": [w.grad for w in WW],
            "g_b": [None if b is None else b.grad for b in bb]}


# ------------------------------------------------------------ module glue
def fixture_tensors(z):
    z = {k: torch.from_numpy(np.asarray(v)) for k, v in z.items()}
    sd = {k[2:]: v for k, v in z.items() if k.startswith("p_")}
    return z, sd


def fixture_inputs(z, spec):
    """(eis, degs, ews) of a layer fixture as K-lists (None entries kept)."""
    K = spec["K"]
    eis = [z.get(f"edge_index{k}") for k in range(K)]
    degs = [z.get(f"deg{k}") for k in range(K)]
    ews = [z.get(f"edge_weight{k}") for k in range(K)]
    return (eis, degs if any(d is not None for d in degs) else None,
            ews if any(w is not None for w in ews) else None)


def make_module(spec, fin=FIN):
    from mgcn.models import GCNMultiKernel
    return GCNMultiKernel(fin, spec.get("fout", FOUT), None, deg_norm=spec["deg_norm"],
                          aggr=spec["aggr"], bias=spec["bias"], num_kernel=spec["K"],
                          kernel_combine=spec["combine"])


# ----------------------------------------------------------------- graphs
def random_graph(seed, n, e, isolated=0):
    """Random directed multigraph on the first n - isolated nodes, COO order."""
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.integers(0, n - isolated, (2, e)).astype(np.int64))


DEGREES = (0, 1, 31, 32, 33, 64, 65, 128)


def degree_graphs(K, n, seed=0):
    """K edge sets over n >= 67 nodes for the kernels' row paths.  In set k,
    node 8 (k % 4) + j has in-degree and out-degree DEGREES[j]: rows of 0, 1,
    31, 32, 33 (around one 32-slot window), 64, 65 and 128 slots (the longest
    row that is not a heavy one).  The other nodes below 32 have no edge in
    set k, so a ladder row of one set is empty in every set that puts its
    ladder elsewhere.  The other endpoints are drawn with replacement from
    nodes 32 .. n - 3 (duplicates occur), which also carry 3 n random edges
    among themselves; the last two nodes have no edge in any set.  Shuffled
    COO order."""
    out = []
    for k in range(K):
        rng = np.random.default_rng([seed, k])
        base = 8 * (k % 4)
        lo, hi = 32, n - 2
        parts = [rng.integers(lo, hi, (2, 3 * n))]
        for j, d in enumerate(DEGREES):
            v = base + j
            parts.append(np.stack([rng.integers(lo, hi, d), np.full(d, v)]))  # in-degree d
            parts.append(np.stack([np.full(d, v), rng.integers(lo, hi, d)]))  # out-degree d
        ei = np.concatenate(parts, axis=1)
        ei = ei[:, rng.permutation(ei.shape[1])]
        ind, outd = np.bincount(ei[1], minlength=n), np.bincount(ei[0], minlength=n)
        assert list(ind[base:base + 8]) == list(DEGREES) == list(outd[base:base + 8])
        others = [v for v in range(32) if not base <= v < base + 8]
        assert not ind[others].any() and not outd[others].any()
        out.append(torch.from_numpy(ei.astype(np.int64)))
    return out


def zero_graph():
    """An edge set without edges."""
    return torch.zeros(2, 0, dtype=torch.int64)
