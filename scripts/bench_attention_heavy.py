"""A/B of the heavy-row route of the attention launches (mgcn_(h)att_*_sched)
against one wave per row, and against the commit before the route.

    python scripts/bench_attention_heavy.py [--window 1.0] [--parent parent.json]
                                            [--out profiles/attention_heavy/ab.json]

One attention layer after its ``x @ W``, forward plus backward (gradients to
Hp and the attention vector), soft (``attention_aggregate``) and hard training
(``hard_attention_aggregate(training=True)``, noise given, T = 0.5), att_dir
'in' and 'out', lrelu:

* the config-3 botnet graph at H = 4, C = 8 (hub rows of several thousand
  edges in either view)
* the config-2 graph at H = 8, C = 16, soft 'in' (no heavy row: the route's
  launches are the wave kernels')

Protocol of scripts/bench_spmm_bf16.py: the arms alternate in blocks within one
process after a warm-up, each with at least ``--window`` seconds of timed
launches -- ``off`` (the route switched off: one wave per row, every row),
``off2`` (the same again: its distance from ``off`` is the run's own spread)
and ``on`` (the default).  On a tree without the switch (the parent commit)
there is one arm, timed twice (``off``, ``off2``), and the file says
``"switch": false``; ``--parent`` merges such a file, written in the same
session on the same device, into the output as the yardstick:
``on_vs_parent`` = on / parent and ``default_on_justified`` = on beats the
parent by more than the larger of the two runs' spreads (soft 'in': the rule
for the default), ``off_vs_parent`` the cross-check that off is the parent.

``launch_ms`` holds the median HIP-event time of every attention launch of a
step (timer names ``att_*`` / ``hatt_*`` / ``edge_softmax``), route on and off;
with the route on a launch is its whole ``_sched`` entry, the serial S-chain
pass of the adjoints included.  Then ms per step of the 6-layer
``GCNModel(nodemodel='attention')`` of src/run/run_botnet_soft.sh (32 wide,
one head, 'out', lrelu, residual_hop 1, final proj) on the config-3 graph.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "meta-gcn_amd"), os.path.join(ROOT, "scripts")]

import torch  # noqa: E402

import mgcn  # noqa: E402,F401
from mgcn import ops  # noqa: E402
from mgcn.graph import plan_for  # noqa: E402
from bench import make_botnet_graph, make_er_graph  # noqa: E402
from bench_spmm_bf16 import alternate  # noqa: E402

HAS_SWITCH = hasattr(ops, "set_attention_heavy_rows")


def set_route(on):
    if HAS_SWITCH:
        ops.set_attention_heavy_rows(on)


def launch_ms(step, steps=20):
    """Median HIP-event ms of every attention launch of ``step`` (the kernel
    timer hook of mgcn._call)."""
    evs, open_ = {}, {}

    def timer(name, start, rows=None, edges=None):
        if not (name.startswith(("att_", "hatt_")) or name.endswith("edge_softmax")):
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


def layer_ab(plan, N, H, C, kind, adir, window_s, dev):
    nnz = plan.nnz
    g = torch.Generator().manual_seed(1)
    Hp = torch.randn(N, H * C, generator=g).to(dev).requires_grad_(True)
    att = (torch.randn(1, H, 2 * C, generator=g) * 0.3).to(dev).requires_grad_(True)
    dY = torch.randn(N, H * C, generator=g).to(dev)
    noise = None
    if kind == "hard":
        u = torch.rand(nnz, H, generator=g).clamp(1e-6, 1 - 1e-6)
        noise = (-torch.log(-torch.log(u))).to(dev)

    def step(on):
        set_route(on)
        Hp.grad = att.grad = None
        if kind == "soft":
            y, _ = ops.attention_aggregate(Hp, att, plan, H, "lrelu", adir)
        else:
            y, _ = ops.hard_attention_aggregate(Hp, att, plan, H, "lrelu", adir, 0.5,
                                                training=True, noise=noise)
        y.backward(dY)
        set_route(True)

    def step_off():
        step(False)

    def step_on():
        step(True)

    arms = {"off": step_off, "off2": step_off}
    same_bits = None
    if HAS_SWITCH:
        arms["on"] = step_on
        step_off()
        goff = [Hp.grad.clone(), att.grad.clone()]
        step_on()
        same_bits = torch.equal(Hp.grad, goff[0]) and torch.equal(att.grad, goff[1])
    r = alternate(arms, window_s)
    off, off2 = r["off"]["median_ms"], r["off2"]["median_ms"]
    r["spread_off_off2"] = abs(off - off2) / off
    r["launch_ms"] = {"off": launch_ms(step_off)}
    if HAS_SWITCH:
        on = r["on"]["median_ms"]
        r["ratio_on_over_off"] = on / off
        r["on_faster_than_spread"] = bool((off - on) / off > r["spread_off_off2"])
        r["on_within_spread"] = bool(abs(off - on) / off <= r["spread_off_off2"])
        r["on_off_same_bits"] = same_bits
        r["launch_ms"]["on"] = launch_ms(step_on)
    r.update({"n_nodes": N, "nnz": nnz, "H": H, "C": C, "kind": kind, "att_dir": adir,
              "n_heavy": [plan.fwd.n_heavy, plan.bwd.n_heavy],
              "max_degree": [int((v.rowptr[1:] - v.rowptr[:-1]).max())
                             for v in (plan.fwd, plan.bwd)]})
    return r


def model_ms(ei, N, dev, on, steps=10, warmup=3):
    from mgcn.models import GCNModel
    set_route(on)
    torch.manual_seed(0)
    m = GCNModel(1, [32] * 6, 2, residual_hop=1, dropout=0.0, final_type='proj',
                 nodemodel='attention', nheads=1, att_act='lrelu', att_dropout=0.0,
                 att_dir='out', bias=False).to(dev)
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
    set_route(True)
    return ms[len(ms) // 2]


def merge_parent(res, parent):
    """The parent commit's file (one arm, same session) as the yardstick."""
    res["parent_device"] = parent.get("device")
    for k, r in res.items():
        p = parent.get(k)
        if not isinstance(r, dict) or not isinstance(p, dict) or "launch_ms" not in r:
            continue
        pm = p["off"]["median_ms"]
        spread = max(r["spread_off_off2"], p["spread_off_off2"])
        r["parent_ms"] = pm
        r["parent_spread"] = p["spread_off_off2"]
        r["parent_launch_ms"] = p["launch_ms"]["off"]
        r["off_vs_parent"] = r["off"]["median_ms"] / pm
        r["off_is_parent_within_spread"] = bool(abs(r["off"]["median_ms"] - pm) / pm <= spread)
        if "on" in r:
            on = r["on"]["median_ms"]
            r["on_vs_parent"] = on / pm
            r["on_beats_parent_by_more_than_spread"] = bool((pm - on) / pm > spread)
            r["on_is_parent_within_spread"] = bool(abs(on - pm) / pm <= spread)
    if "model6_config3_ms_per_step" in parent:
        res["model6_config3_ms_per_step"]["parent"] = parent["model6_config3_ms_per_step"]["off"]
    key = "config3_botnet_H4_C8_soft_in"
    if "on_beats_parent_by_more_than_spread" in res.get(key, {}):
        res["default_on_justified"] = res[key]["on_beats_parent_by_more_than_spread"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0, help="seconds of timed launches per arm")
    ap.add_argument("--parent", default=None, help="this script's output on the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_heavy",
                                                  "ab.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "switch": HAS_SWITCH}
    ei3, N3, _ = make_botnet_graph()
    ei3 = ei3.to(dev)
    plan3 = plan_for(ei3, N3)
    runs = []
    for kind in ("soft", "hard"):
        for adir in ("in", "out"):
            k = f"config3_botnet_H4_C8_{kind}_{adir}"
            res[k] = layer_ab(plan3, N3, 4, 8, kind, adir, args.window, dev)
            runs.append(k)
    res["model6_config3_ms_per_step"] = {"off": model_ms(ei3, N3, dev, False)}
    if HAS_SWITCH:
        res["model6_config3_ms_per_step"]["on"] = model_ms(ei3, N3, dev, True)
    del ei3, plan3
    ei2, N2 = make_er_graph()
    ei2 = ei2.to(dev)
    k = "config2_H8_C16_soft_in"
    res[k] = layer_ab(plan_for(ei2, N2), N2, 8, 16, "soft", "in", args.window, dev)
    runs.append(k)
    if args.parent:
        with open(args.parent) as f:
            merge_parent(res, json.load(f))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    for k in runs:
        r = res[k]
        print(json.dumps({"run": k, "off_ms": r["off"]["median_ms"],
                          "off2_ms": r["off2"]["median_ms"],
                          "on_ms": r.get("on", {}).get("median_ms"),
                          "parent_ms": r.get("parent_ms"), "spread": r["spread_off_off2"],
                          "on_vs_parent": r.get("on_vs_parent"),
                          "off_vs_parent": r.get("off_vs_parent"),
                          "same_bits": r.get("on_off_same_bits"), "n_heavy": r["n_heavy"],
                          "launch_ms": r["launch_ms"]}), flush=True)
    print(json.dumps({"run": "model6_config3", **res["model6_config3_ms_per_step"],
                      "default_on_justified": res.get("default_on_justified")}))


if __name__ == "__main__":
    main()
