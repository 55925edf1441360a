"""Generate the edge-gate fixtures tests/golden/gate_*.npz from the REFERENCE.

    python tests/golden/make_golden_edge_gate.py

Runs the reference's own NodeModelAdditive with ``edge_gate`` 'proj' / 'free'
(src/gcn_meta/models/gcn_base_models.py:199-243, 322-396) and, for
``gate_model_debru``, its GCNModel as src/run/run_debru_32_eg.sh builds it (6
layers) on the CPU under the stubs of make_golden.py, twice: once as is (fp32)
and once with ``.double()`` on the same parameters.  The fp64 run is the truth
the GPU tests compare against; the fp32 run measures the reference's own
rounding error, which sets the tolerance:

    max|t_gpu - t64| <= max(4 * max|t32 - t64|, 1e-5 * max|t64|)

The fixtures hold arrays only: edge_index, x, dY, where used edge_attr /
edge_weight / deg, the parameters (p_<state_dict key>), and y / gate / dx /
g_<parameter> with the suffixes 32 and 64.  The script prints
max|t32 - t64| / max|t64| of every recorded tensor (the table in DESIGN.md).

Max cases run on a graph without parallel edges and must pass a gap condition:
in fp64 the two largest messages of every (node, feature) differ by more than
1e-4 max|m|; a case that fails takes another seed.  A winner that flips between
fp32 and fp64 would put a discontinuity into the bound.

The model case must pass a conditioning check of the same kind.  With
deg_norm None, sum aggregation and in_channels = 1 its first-layer gradients
are sums with heavy cancellation, and the reference's own fp32 error on them
moves by more than ten times with the order of the edges alone (the order its
scatter_add walks).  One fp32 run is then no measure of the fp32 error, and
the bound built on it fails the reference itself.  So the reference's fp32 run
is repeated on PERMS permutations of the edge list, and a draw is kept only if
every one of those runs is inside the bound built from the recorded t32 / t64
for every recorded tensor; a draw that fails takes another seed.  The check
uses the reference alone.
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
from make_golden_attention import hub_graph, report  # noqa: E402
from edge_gate_ref import (FIXTURES, MODEL_ARGS, MODEL_FIXTURE, gate_layer_ref, max_gap,  # noqa: E402
                           params_of)

FIN, FOUT, N, E = 16, 32, 300, 2150
GAP = 1e-4
# y / dx / gate alone, in fp32 and fp64 at N = 300 and 16 -> 32 channels, are 202 KB of
# incompressible mantissas; with the inputs a file comes to about 270 KB
MAX_BYTES = 300 * 1024


def _graph(rng, kind, aggr):
    if kind == "hub":
        return hub_graph(rng)
    ei = make_graph(rng, N, E, self_loops=True, isolated=3)
    if aggr == "max":  # parallel edges carry equal messages: an exact tie
        _, first = np.unique(ei[0] * N + ei[1], return_index=True)
        ei = ei[:, np.sort(first)]
    return ei


def layer_case(gbm, name, rng):
    gate, dn, aggr, bias, use_ew, use_deg, edim, kind = FIXTURES[name]
    while True:
        ei = _graph(rng, kind, aggr)
        n, nnz = (320 if kind == "hub" else N), ei.shape[1]
        torch.manual_seed(int(rng.integers(1 << 30)))
        nm = gbm.NodeModelAdditive(FIN, FOUT, in_edgedim=edim, deg_norm=dn, edge_gate=gate,
                                   aggr=aggr, bias=bias, num_edges=nnz)
        with torch.no_grad():  # the inits (gates near 1/2, zero biases) test little
            if bias:
                nm.bias.uniform_(-0.5, 0.5)
            if gate == "proj":
                nm.edge_gate.linsrc.weight.uniform_(-0.5, 0.5)
                nm.edge_gate.lintgt.weight.uniform_(-0.5, 0.5)
                nm.edge_gate.bias.uniform_(-0.5, 0.5)
                if edim is not None:
                    nm.edge_gate.linedge.weight.uniform_(-0.5, 0.5)
            else:
                nm.edge_gate.edge_gates.uniform_(-2.0, 2.0)
        x = torch.randn(n, FIN)
        dY = torch.randn(n, FOUT)
        ea = torch.randn(nnz, edim) if edim is not None else None
        ew = torch.rand(nnz) * 1.9 + 0.1 if use_ew else None
        deg = torch.rand(n) * 4.0 + 0.5 if use_deg else None
        if aggr == "max":
            # screen the draw with the fp64 restatement (vectorised) before the
            # reference's sequential scatter_max runs; the reference's own
            # messages are checked again below
            P64 = {k: v.double() for k, v in params_of(nm.state_dict()).items()}
            msg = gate_layer_ref(x.double(), P64, _t(ei), gate, dn, aggr,
                                 edge_weight=None if ew is None else ew.double(),
                                 deg=None if deg is None else deg.double())[2]
            if not max_gap(msg, _t(ei)[1], n) > GAP:
                continue
        rec = {"edge_index": ei, "x": x, "dY": dY, "edge_attr": ea, "edge_weight": ew, "deg": deg}
        for pk, pv in nm.state_dict().items():
            rec["p_" + pk] = pv.clone()
        msgs = {}
        for tag, mod, dt in (("32", nm, torch.float32), ("64", copy.deepcopy(nm).double(),
                                                         torch.float64)):
            xx = x.detach().clone().to(dt).requires_grad_(True)
            gates = []
            hook = mod.edge_gate.register_forward_hook(lambda m, i, o: gates.append(o.detach()))
            orig = gbm.scatter_

            def spy(name_, src, index, dim_size=None, _tag=tag):
                msgs[_tag] = src.detach()
                return orig(name_, src, index, dim_size=dim_size)
            gbm.scatter_ = spy
            try:
                y = mod(xx, _t(ei), edge_attr=None if ea is None else ea.to(dt),
                        deg=None if deg is None else deg.to(dt),
                        edge_weight=None if ew is None else ew.to(dt))
            finally:
                gbm.scatter_ = orig
                hook.remove()
            y.backward(dY.to(dt))
            rec["y" + tag] = y.detach()
            rec["gate" + tag] = gates[0]
            rec["dx" + tag] = xx.grad
            for pk, pv in mod.named_parameters():
                rec["g_" + pk + tag] = pv.grad
        if aggr == "max":
            gap = max_gap(msgs["64"], _t(ei)[1], n)
            if not gap > GAP:
                print("%-26s gap %.1e: another seed" % (name, gap))
                continue
        break
    path = save(name, **rec)
    assert os.path.getsize(path) < MAX_BYTES, (name, os.path.getsize(path))
    report(name, rec)


PERMS = 8


def _model_run(mod, x, ei, dY, dt):
    mod.zero_grad()
    xx = x.detach().clone().to(dt).requires_grad_(True)
    y = mod(xx, _t(ei))
    y.backward(dY.to(dt))
    out = {"y": y.detach(), "dx": xx.grad}
    for pk, pv in mod.named_parameters():
        out["g_" + pk] = pv.grad.clone()
    return out


def model_case(gm, rng):
    while True:
        rec = _model_draw(gm, rng)
        m, ei = rec.pop("_model"), rec["edge_index"]
        worst = 0.0
        for _ in range(PERMS):
            run = _model_run(m, rec["x"], ei[:, rng.permutation(ei.shape[1])], rec["dY"],
                             torch.float32)
            for k, v in run.items():
                t64 = rec[k + "64"].double()
                e32 = (rec[k + "32"].double() - t64).abs().max().item()
                bound = max(4 * e32, 1e-5 * t64.abs().max().item())
                worst = max(worst, (v.double() - t64).abs().max().item() / bound)
        print("%-26s worst fp32 err / bound over %d edge orders: %.2f" % (MODEL_FIXTURE, PERMS,
                                                                         worst))
        if worst <= 1.0:
            break
    path = save(MODEL_FIXTURE, **rec)
    assert os.path.getsize(path) < MAX_BYTES, os.path.getsize(path)
    report(MODEL_FIXTURE, rec)


def _model_draw(gm, rng):
    ei = make_graph(rng, N, E, self_loops=True, isolated=3)
    torch.manual_seed(int(rng.integers(1 << 30)))
    args = dict(MODEL_ARGS)
    m = gm.GCNModel(args.pop("in_channels"), args.pop("enc_sizes"), args.pop("num_classes"), **args)
    with torch.no_grad():
        for layer in m.gcn_net:
            eg = layer.gcn.node_models[0].edge_gate
            eg.linsrc.weight.uniform_(-0.5, 0.5)
            eg.lintgt.weight.uniform_(-0.5, 0.5)
            eg.bias.uniform_(-0.5, 0.5)
    x = torch.randn(N, 1)
    dY = torch.randn(N, 2)
    rec = {"edge_index": ei, "x": x, "dY": dY}
    for pk, pv in m.state_dict().items():
        rec["p_" + pk] = pv.clone()
    for tag, mod, dt in (("32", m, torch.float32), ("64", copy.deepcopy(m).double(),
                                                    torch.float64)):
        for k, v in _model_run(mod, x, ei, dY, dt).items():
            rec[k + tag] = v
    rec["_model"] = m
    return rec


def main():
    _install_stubs()
    sys.path.insert(0, REF_SRC)
    from gcn_meta.models import gcn_base_models, gcn_model
    # one generator per case (seeded by its position), so that a subset named on
    # the command line reproduces the same files
    names = list(FIXTURES) + [MODEL_FIXTURE]
    for idx, name in enumerate(names):
        if sys.argv[1:] and name not in sys.argv[1:]:
            continue
        rng = np.random.default_rng([20261020, idx])
        if name == MODEL_FIXTURE:
            model_case(gcn_model, rng)
        else:
            layer_case(gcn_base_models, name, rng)


if __name__ == "__main__":
    main()
