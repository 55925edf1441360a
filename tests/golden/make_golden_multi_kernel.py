"""Generate the multi-kernel fixtures tests/golden/mk_*.npz from the REFERENCE.

    python tests/golden/make_golden_multi_kernel.py

Runs the reference on the CPU under the stubs of make_golden.py, twice: once
as is (fp32) and once with ``.double()`` on the same parameters.  The fp64 run
is the truth the GPU tests compare against; the fp32 run measures the
reference's own rounding error, which sets the tolerance:

    max|t_gpu - t64| <= max(4 * max|t32 - t64|, 1e-5 * max|t64|)

``mk_add_*`` run the reference's own GCNMultiKernel (gcn_multi_kernel.py:
76-114, kernel_combine='add') and ``mk_model`` its GCNModel with two kernels
per layer.  ``mk_mean_*`` and ``mk_cat_*`` run the reference's
NodeModelAdditive once per kernel (the node_models of a reference
GCNMultiKernel, so the state_dict keys are the module's) and combine the K
results here, sum / count and ``torch.cat``: the reference's own forward
raises for these two when K > 1 (``if xo == 0`` / ``xo != 0`` on a tensor,
gcn_multi_kernel.py:100, 103), and this is the combination its code intends
and mgcn.models implements.

The fixtures hold arrays only: edge_index<k> (absent: that kernel's edge_index
is None), x, dY, where used edge_weight<k> / deg<k>, the parameters
(p_<state_dict key>), and y / dx / g_<parameter> with the suffixes 32 and 64.
The last three nodes have no edge in any kernel (their rows are the sum of the
biases).  N = 300, about 2,150 edges per kernel, 16 -> 32 channels; the cat
cases 16 -> 16 (K = 2) and 16 -> 8 (K = 3) per kernel, which keeps y within
[300, 32] and every file under 300 KB.  Biases are drawn from U(-0.5, 0.5).
The script prints max|t32 - t64| / max|t64| of every recorded tensor.
"""
from __future__ import annotations

import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import REF_SRC, _install_stubs, _t, make_graph, save  # noqa: E402
from make_golden_attention import report  # noqa: E402
from multi_kernel_ref import (E, FIN, FIXTURES, FOUT, ISOLATED, MODEL_ARGS, MODEL_FIXTURE,  # noqa: E402
                              N)

MAX_BYTES = 300 * 1024


def _graphs(rng, K, empty=False, skip=None):
    eis = []
    for k in range(K):
        if k == skip:
            eis.append(None)
            continue
        ei = make_graph(rng, N, E, self_loops=False, isolated=ISOLATED)
        if empty and k == 1:  # 20 further nodes without an in-edge
            ei = ei[:, ei[1] < N - ISOLATED - 20]
        # self-loops on the nodes that have edges (data_procs/loop.py:13-17)
        loops = np.arange(N - ISOLATED - (20 if empty and k == 1 else 0))
        eis.append(np.concatenate([ei, np.stack([loops, loops])], axis=1).astype(np.int64))
    return eis


def _randomise_biases(mod):
    with torch.no_grad():
        for name, p in mod.named_parameters():
            if name.endswith("bias"):
                p.uniform_(-0.5, 0.5)


def _forward(mod, spec, xx, eis, degs, ews, dt):
    def cast(ts):
        return None if ts is None else [None if t is None else t.to(dt) for t in ts]
    tei = [None if ei is None else _t(ei) for ei in eis]
    degs, ews = cast(degs), cast(ews)
    if spec["combine"] == "add":
        return mod(xx, tei, None, degs, ews)
    outs = []
    for k, (nm, ei) in enumerate(zip(mod.node_models, tei)):
        if ei is not None:
            outs.append(nm(xx, ei, None, None if degs is None else degs[k],
                           None if ews is None else ews[k]))
    if spec["combine"] == "cat":
        return torch.cat(outs, dim=1)
    return sum(outs[1:], outs[0]) / len(outs)


def layer_case(gmk, name, rng):
    spec = FIXTURES[name]
    K, fout = spec["K"], spec.get("fout", FOUT)
    eis = _graphs(rng, K, spec.get("empty", False), spec.get("skip"))
    torch.manual_seed(int(rng.integers(1 << 30)))
    mod = gmk.GCNMultiKernel(FIN, fout, None, deg_norm=spec["deg_norm"], aggr=spec["aggr"],
                             bias=spec["bias"], num_kernel=K, kernel_combine=spec["combine"])
    _randomise_biases(mod)
    x = torch.randn(N, FIN)
    dY = torch.randn(N, fout * (sum(ei is not None for ei in eis)
                                if spec["combine"] == "cat" else 1))
    degs = ews = None
    if spec.get("lists"):
        ews = [torch.rand(eis[0].shape[1]) * 1.9 + 0.1] + [None] * (K - 1)
        degs = [None, torch.rand(N) * 4.0 + 0.5] + [None] * (K - 2)
    rec = {"x": x, "dY": dY}
    for k in range(K):
        rec[f"edge_index{k}"] = eis[k]
        rec[f"edge_weight{k}"] = None if ews is None else ews[k]
        rec[f"deg{k}"] = None if degs is None else degs[k]
    for pk, pv in mod.state_dict().items():
        rec["p_" + pk] = pv.clone()
    for tag, m, dt in (("32", mod, torch.float32), ("64", copy.deepcopy(mod).double(),
                                                    torch.float64)):
        xx = x.detach().clone().to(dt).requires_grad_(True)
        y = _forward(m, spec, xx, eis, degs, ews, dt)
        y.backward(dY.to(dt))
        rec["y" + tag] = y.detach()
        rec["dx" + tag] = xx.grad
        for pk, pv in m.named_parameters():
            if pv.grad is not None:  # a skipped kernel's parameters get none
                rec["g_" + pk + tag] = pv.grad
    path = save(name, **rec)
    assert os.path.getsize(path) < MAX_BYTES, (name, os.path.getsize(path))
    report(name, rec)


def model_case(gm, rng):
    eis = _graphs(rng, 2)
    torch.manual_seed(int(rng.integers(1 << 30)))
    args = dict(MODEL_ARGS)
    m = gm.GCNModel(args.pop("in_channels"), args.pop("enc_sizes"), args.pop("num_classes"), **args)
    _randomise_biases(m)
    x = torch.randn(N, FIN)
    dY = torch.randn(N, 2)
    rec = {"x": x, "dY": dY, "edge_index0": eis[0], "edge_index1": eis[1]}
    for pk, pv in m.state_dict().items():
        rec["p_" + pk] = pv.clone()
    for tag, mod, dt in (("32", m, torch.float32), ("64", copy.deepcopy(m).double(),
                                                    torch.float64)):
        xx = x.detach().clone().to(dt).requires_grad_(True)
        y = mod(xx, [_t(ei) for ei in eis])
        y.backward(dY.to(dt))
        rec["y" + tag] = y.detach()
        rec["dx" + tag] = xx.grad
        for pk, pv in mod.named_parameters():
            rec["g_" + pk + tag] = pv.grad
    path = save(MODEL_FIXTURE, **rec)
    assert os.path.getsize(path) < MAX_BYTES, os.path.getsize(path)
    report(MODEL_FIXTURE, rec)


def main():
    _install_stubs()
    sys.path.insert(0, REF_SRC)
    from gcn_meta.models import gcn_model, gcn_multi_kernel
    # one generator per case (seeded by its position), so that a subset named on
    # the command line reproduces the same files
    names = list(FIXTURES) + [MODEL_FIXTURE]
    for idx, name in enumerate(names):
        if sys.argv[1:] and name not in sys.argv[1:]:
            continue
        rng = np.random.default_rng([20261021, idx])
        if name == MODEL_FIXTURE:
            model_case(gcn_model, rng)
        else:
            layer_case(gcn_multi_kernel, name, rng)


if __name__ == "__main__":
    main()
