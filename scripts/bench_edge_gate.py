"""A/B of the fused edge-gate kernels against the gate composed from the ops
that existed before them.

    python scripts/bench_edge_gate.py [--window 1.0] [--out profiles/edge_gate_heavy/ab.json]

One gated layer after its ``x @ W``, forward plus backward (gradients to Hx,
the two gate vectors and the gate bias), on two shapes:

* the config-3 botnet graph at C = 32, deg_norm None, 'proj' (the workload's)
* the config-2 graph at C = 128, 'sm', 'proj'

Protocol of scripts/bench_spmm_bf16.py: four arms alternate in blocks within
one process after a warm-up, each with at least ``--window`` seconds of timed
launches --

  A   the two scores as one ``linear`` (Hx @ [w_src | w_dst]), torch gathers of
      them per edge, sigmoid, times the norm, fed as differentiable per-slot
      weights to ``_AggregateW`` (mgcn_spmm_fwd / mgcn_spmm_bwd /
      mgcn_edge_weight_grad)
  A2  the same again: its distance from A is the run's own spread
  B_off  ``gate_aggregate`` (mgcn_att_scores, mgcn_gate_fwd, mgcn_gate_bwd_dst,
         mgcn_gate_bwd_src, mgcn_gemm_tn) with the heavy-row route switched
         off (``ops.set_gate_heavy_rows(False)``): one wave per row, every row
  B_on   the same with the route on (the default): the heavy rows of the
         three gate launches by workgroups (mgcn_gate_*_sched)

Algorithmic bytes of arm B's launches, from the shapes (w: 4 more per edge
and gathering launch when the norm has weights):
    scores   4 N C + 8 N
    fwd      8 (N + 1) + nnz (4 col + 4 C row + 4 a + 4 g) + 4 N C + 4 N
    bwd_dst  8 (N + 1) + nnz (4 col + 4 C row + 4 g + 4 dl) + 4 N C + 4 N
    bwd_src  8 (N + 1) + nnz (4 col + 4 slot + 4 C row + 4 g + 4 dl) + 4 N C + 12 N
    gemm_tn  4 N C + 8 N
The JSON holds the times, these bytes, B_on's TB/s, the ratios B_on / B_off and
B_on / A and the A/A2 spread; ``on_faster_than_spread`` says whether B_on beats
B_off by more than that spread, ``on_within_spread`` whether the two are
inside it (a graph without heavy rows: the same launches), and
``faster_than_spread`` whether B_on beats A by more than it.  ``launch_ms``
holds the median HIP-event time of each gate launch with the route on and off.
Then, without a threshold, ms per step of the 12-layer gated GCNModel of
src/run/run_debru_32_eg.sh on the config-3 graph, route on and off, next to
the ungated model.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "meta-gcn_amd"), os.path.join(ROOT, "scripts")]

import torch  # noqa: E402

import mgcn  # noqa: E402,F401
from mgcn import _lib as L  # noqa: E402
from mgcn import ops  # noqa: E402
from mgcn.graph import NormPlan, plan_for  # noqa: E402
from bench import HBM_PEAK_GBS, make_botnet_graph, make_er_graph  # noqa: E402
from bench_spmm_bf16 import alternate  # noqa: E402


def fused_bytes(N, nnz, C, weighted):
    w = 4 * nnz if weighted else 0
    scores = 4 * N * C + 8 * N
    fwd = 8 * (N + 1) + nnz * (4 + 4 * C + 4 + 4) + w + 4 * N * C + 4 * N
    dst = 8 * (N + 1) + nnz * (4 + 4 * C + 4 + 4) + w + 4 * N * C + 4 * N
    src = 8 * (N + 1) + nnz * (4 + 4 + 4 * C + 4 + 4) + w + 4 * N * C + 12 * N
    return scores + fwd + dst + src + scores


def layer_ab(ei, N, C, deg_norm, window_s, dev):
    plan = plan_for(ei, N)
    norm = plan.norm(deg_norm)
    nnz = plan.nnz
    g = torch.Generator().manual_seed(1)
    Hx = torch.randn(N, C, generator=g).to(dev).requires_grad_(True)
    wsd = ((torch.rand(C, 2, generator=g) - 0.5) * 0.2).to(dev).requires_grad_(True)
    beta = torch.zeros(1, device=dev, requires_grad=True)
    dY = torch.randn(N, C, generator=g).to(dev)
    leaves = (Hx, wsd, beta)
    src, dst = plan.coo()
    feid, beid = plan.fwd.eid.long(), plan.bwd.eid.long()
    n_coo = None
    if norm.w_fwd is not None:
        n_coo = torch.empty_like(norm.w_fwd)
        n_coo[feid] = norm.w_fwd

    def step_a():
        for t in leaves:
            t.grad = None
        s = ops.linear(Hx, wsd)
        gate = torch.sigmoid(s[src, 0] + s[dst, 1] + beta)
        w = gate * n_coo if n_coo is not None else gate
        wf = w[feid]
        na = NormPlan(norm.method, wf, w.detach()[beid], None, None, None, grad=True)
        y = ops._AggregateW.apply(Hx, wf, None, plan, na, L.REDUCE_SUM, False)
        y.backward(dY)

    def step_b(heavy):
        ops.set_gate_heavy_rows(heavy)
        for t in leaves:
            t.grad = None
        y, _ = ops.gate_aggregate(Hx, plan, norm, "add", wsd[:, 0], wsd[:, 1], beta)
        y.backward(dY)
        ops.set_gate_heavy_rows(True)

    def step_off():
        step_b(False)

    def step_on():
        step_b(True)

    step_a()
    ga = [t.grad.clone() for t in leaves]
    step_off()
    goff = [t.grad.clone() for t in leaves]
    step_on()
    agree = [float((t.grad - a).abs().max() / a.abs().max().clamp(min=1e-30))
             for t, a in zip(leaves, ga)]
    same_bits = all(torch.equal(t.grad, a) for t, a in zip(leaves, goff))
    r = alternate({"A_composed": step_a, "A2_composed": step_a, "B_off": step_off,
                   "B_on": step_on}, window_s)
    A, A2, Boff, B = (r[k]["median_ms"] for k in ("A_composed", "A2_composed", "B_off", "B_on"))
    by = fused_bytes(N, nnz, C, norm.w_fwd is not None)
    for k in ("B_off", "B_on"):
        r[k]["bytes"] = by
        r[k]["tb_per_s"] = by / r[k]["median_ms"] / 1e9
        r[k]["share_of_hbm_peak"] = r[k]["tb_per_s"] * 1e3 / HBM_PEAK_GBS
    r["ratio_B_over_A"] = B / A
    r["ratio_on_over_off"] = B / Boff
    r["spread_A_A2"] = abs(A - A2) / A
    r["faster_than_spread"] = bool((A - B) / A > r["spread_A_A2"])
    r["on_faster_than_spread"] = bool((Boff - B) / Boff > r["spread_A_A2"])
    r["on_within_spread"] = bool(abs(Boff - B) / Boff <= r["spread_A_A2"])
    r["grad_rel_diff_B_vs_A"] = dict(zip(("Hx", "wsd", "beta"), agree))
    r["on_off_same_bits"] = same_bits
    r["launch_ms"] = {"on": launch_ms(step_on), "off": launch_ms(step_off)}
    r.update({"n_nodes": N, "nnz": nnz, "C": C, "deg_norm": deg_norm,
              "n_heavy": [plan.fwd.n_heavy, plan.bwd.n_heavy]})
    return r


def launch_ms(step, steps=20):
    """Median HIP-event ms of every ``gate_*`` launch of ``step`` (the kernel
    timer hook of mgcn._call)."""
    evs, open_ = {}, {}

    def timer(name, start, rows=None, edges=None):
        if not name.startswith("gate_"):
            return
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        if start:
            open_[name] = e
        else:
            evs.setdefault(name, []).append((open_.pop(name), e))
    ops.set_kernel_timer(timer)
    try:
        for _ in range(steps):
            step()
    finally:
        ops.set_kernel_timer(None)
    torch.cuda.synchronize()
    out = {}
    for name, pairs in evs.items():
        ms = sorted(a.elapsed_time(b) for a, b in pairs)
        out[name] = ms[len(ms) // 2]
    return out


def model_ms(ei, N, edge_gate, dev, steps=10, warmup=3, heavy=True):
    from mgcn.models import GCNModel
    ops.set_gate_heavy_rows(heavy)
    torch.manual_seed(0)
    m = GCNModel(1, [32] * 12, 2, residual_hop=1, dropout=0, final_type='proj', deg_norm=None,
                 edge_gate=edge_gate, aggr='add', bias=False).to(dev)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(N, 1, generator=g).to(dev)
    dY = (torch.randn(N, 2, generator=g) * 1e-3).to(dev)

    def step():
        m.zero_grad(set_to_none=True)
        m(x, ei).backward(dY)
    for _ in range(warmup):
        step()
    evs = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        evs.append((a, b))
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in evs)
    ops.set_gate_heavy_rows(True)
    return ms[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0, help="seconds of timed launches per arm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edge_gate_heavy",
                                                  "ab.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "hbm_peak_tb_per_s": HBM_PEAK_GBS / 1e3}
    ei3, N3, _ = make_botnet_graph()
    ei3 = ei3.to(dev)
    res["config3_botnet_C32_none"] = layer_ab(ei3, N3, 32, None, args.window, dev)
    res["model12_config3_ms_per_step"] = {
        "gated_proj": model_ms(ei3, N3, "proj", dev),
        "gated_proj_heavy_off": model_ms(ei3, N3, "proj", dev, heavy=False),
        "ungated": model_ms(ei3, N3, None, dev)}
    del ei3
    ei2, N2 = make_er_graph()
    ei2 = ei2.to(dev)
    res["config2_C128_sm"] = layer_ab(ei2, N2, 128, "sm", args.window, dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    for k in ("config3_botnet_C32_none", "config2_C128_sm"):
        r = res[k]
        print(json.dumps({"run": k, "A_ms": r["A_composed"]["median_ms"],
                          "A2_ms": r["A2_composed"]["median_ms"],
                          "B_off_ms": r["B_off"]["median_ms"], "B_on_ms": r["B_on"]["median_ms"],
                          "on_over_off": r["ratio_on_over_off"], "B_over_A": r["ratio_B_over_A"],
                          "spread": r["spread_A_A2"], "B_tb_per_s": r["B_on"]["tb_per_s"],
                          "on_faster_than_spread": r["on_faster_than_spread"],
                          "on_within_spread": r["on_within_spread"],
                          "faster_than_spread": r["faster_than_spread"],
                          "same_bits": r["on_off_same_bits"], "launch_ms": r["launch_ms"]}),
              flush=True)
    print(json.dumps({"run": "model12_config3", **res["model12_config3_ms_per_step"]}))


if __name__ == "__main__":
    main()
