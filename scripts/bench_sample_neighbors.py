"""A/B of neighbour sampling on the device against the torch composition.

    python scripts/bench_sample_neighbors.py [--window 1.0] [--out profiles/sample_neighbors/ab.json]

Graphs: bench.py's config-2 generator (1M nodes, 11M slots) and the config-3
botnet-shaped graph; fan-outs k = 5, 10, 25.  Within one process the arms of a
case alternate in blocks after a warm-up until each has at least ``--window``
seconds of timed calls; an arm that runs twice (A / A') gives the run's spread.

  mask      the ``mgcn_sample_rows`` launch alone (``mgcn.sample_keep``), with
            the view's row schedule (S, S' again) and without it (N: natural
            order, the long rows found by a walk).  HIP events around blocks of
            16 calls; ``gbs`` is the algorithmic bytes 8 (N + 1) + nnz (4 + 4 +
            1) (rowptr, col, eid, the keep byte) over the median, ``of_8tbs``
            that over 8 TB/s.
  sample    mask + derive.  A / A': what a user of a tree without the entry
            writes -- ``torch.rand(E)`` keys, a sort by (dst, key), ranks from
            the row pointers, ``rank < k``, ``select_edges``; B:
            ``mgcn.sample_neighbors``.  Host clock, every call ends in a device
            synchronise (the edge-count wait of select_edges is part of both).
            The baseline ranks self loops like any edge; B keeps them on top
            (the default ``keep_loops``).
  mean      ``aggregate_plan(h, plan, plan.norm(None), 'mean')`` forward +
            backward at F = 128 on the full plan (A / A') and the sampled one (B).
  sage      a training step of two ``mgcn.pyg.SAGEConv(128, 128)`` on the full
            edge list (A / A') and the sampled one (B), plans cached.

``not_slower_than_spread``: (B - A) / A <= |A - A'| / A on the medians.
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "meta-gcn_amd")]

import torch  # noqa: E402

import mgcn  # noqa: E402
from mgcn import graph as G  # noqa: E402
from mgcn.ops import aggregate_plan  # noqa: E402
from bench import make_er_graph  # noqa: E402

FANOUTS = (5, 10, 25)


def host_block(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3  # ms per call


def event_block(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def alternate(arms, window_s, block, n):
    """arms: [(name, fn)].  Blocks of n calls, the arms taking turns, until every
    arm has at least window_s of timed calls; per-call ms."""
    for _, fn in arms:  # warm-up
        block(fn, n)
    est = [block(fn, n) * n / 1e3 for _, fn in arms]
    rounds = max(5, math.ceil(1.1 * window_s / max(min(est), 1e-6)))
    ms = {name: [] for name, _ in arms}
    for _ in range(rounds):
        for name, fn in arms:
            ms[name].append(block(fn, n))
    out = {}
    for name, v in ms.items():
        v = sorted(v)
        out[name] = {"median_ms": v[len(v) // 2], "mean_ms": sum(v) / len(v), "min_ms": v[0],
                     "calls": n * len(v), "window_s": sum(v) * n / 1e3}
    return out


def verdict(r, a, a2, b):
    A, A2, B = r[a]["median_ms"], r[a2]["median_ms"], r[b]["median_ms"]
    r["spread"] = abs(A - A2) / A
    r["ratio_B_over_A"] = B / A
    r["not_slower_than_spread"] = bool((B - A) / A <= r["spread"])
    return r


def run_mask(plan, k, window_s):
    def arm(on):
        def fn():
            mgcn.set_sample_heavy_rows(on)
            mgcn.sample_keep(plan, k, seed=1, offset=2)
        return fn
    r = alternate([("N_no_schedule", arm(False)), ("S_schedule", arm(True)),
                   ("S2_schedule", arm(True))], window_s, event_block, 16)
    mgcn.set_sample_heavy_rows(True)
    r["bytes"] = 8 * (plan.num_nodes + 1) + plan.nnz * 9
    for name in ("N_no_schedule", "S_schedule"):
        gbs = r["bytes"] / (r[name]["median_ms"] * 1e-3) / 1e9
        r[name]["gbs"], r[name]["of_8tbs"] = gbs, gbs / 8000.0
    # the switch stays on if the scheduled route (B) is not slower than none (A)
    A, B, B2 = (r[n]["median_ms"] for n in ("N_no_schedule", "S_schedule", "S2_schedule"))
    r["spread"] = abs(B - B2) / B
    r["ratio_S_over_N"] = B / A
    r["schedule_not_slower_than_spread"] = bool((B - A) / A <= r["spread"])
    r["kept"] = int(mgcn.sample_keep(plan, k, seed=1, offset=2).sum())
    return r


def torch_sample(plan, dst, k):
    E = plan.nnz
    key = torch.rand(E, device=plan.device)
    o = torch.argsort(key)
    o = o[torch.argsort(dst[o], stable=True)]  # by (dst, key)
    rank = torch.arange(E, device=plan.device) - plan.fwd.rowptr[dst[o]]
    keep = torch.empty(E, dtype=torch.bool, device=plan.device)
    keep[o] = rank < k
    return plan.select_edges(keep), keep


def run_sample(plan, dst, k, window_s):
    base = lambda: torch_sample(plan, dst, k)  # noqa: E731
    new = lambda: mgcn.sample_neighbors(plan, k, seed=1, offset=2)  # noqa: E731
    r = alternate([("A_torch", base), ("A2_torch", base), ("B_device", new)], window_s,
                  host_block, 4)
    r["edges_kept_torch"], r["edges_kept_device"] = base()[0].nnz, new()[0].nnz
    return verdict(r, "A_torch", "A2_torch", "B_device")


def run_mean(full, child, window_s, F=128):
    dev = full.device
    g = torch.Generator().manual_seed(0)
    h = torch.randn(full.num_nodes, F, generator=g).to(dev).requires_grad_(True)
    dy = torch.randn(full.num_nodes, F, generator=g).to(dev)

    def arm(plan):
        norm = plan.norm(None)

        def fn():
            h.grad = None
            aggregate_plan(h, plan, norm, 'mean').backward(dy)
        return fn
    r = alternate([("A_full", arm(full)), ("A2_full", arm(full)), ("B_sampled", arm(child))],
                  window_s, host_block, 4)
    return verdict(r, "A_full", "A2_full", "B_sampled")


def run_sage(ei, ei_child, N, window_s, F=128):
    from mgcn.pyg import SAGEConv
    dev = ei.device
    torch.manual_seed(0)
    c1, c2 = SAGEConv(F, F).to(dev), SAGEConv(F, F).to(dev)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(N, F, generator=g).to(dev)
    dy = torch.randn(N, F, generator=g).to(dev)

    def arm(e):
        def fn():
            for m in (c1, c2):
                m.zero_grad(set_to_none=True)
            c2(c1(x, e).relu(), e).backward(dy)
        return fn
    r = alternate([("A_full", arm(ei)), ("A2_full", arm(ei)), ("B_sampled", arm(ei_child))],
                  window_s, host_block, 4)
    return verdict(r, "A_full", "A2_full", "B_sampled")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0, help="seconds of timed calls per arm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_neighbors", "ab.json"))
    ap.add_argument("--small", action="store_true", help="tiny graphs (a rehearsal of the script)")
    ap.add_argument("--skip-steps", action="store_true", help="no downstream arms")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    from mgcn.botnet import make_botnet_graph
    if args.small:
        er, er_n = make_er_graph(20_000, 100_000)
        bot, bot_n, _ = make_botnet_graph(5_000, 12_000, 600, 500, 2_000)
    else:
        er, er_n = make_er_graph()
        bot, bot_n, _ = make_botnet_graph()
    res = {"device": torch.cuda.get_device_name(0), "window_s": args.window, "graphs": {}}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    for name, ei, N in (("config2", er.to(dev), er_n), ("botnet", bot.to(dev), bot_n)):
        plan = G.build_plan(ei, N)
        deg = plan.fwd.rowptr[1:] - plan.fwd.rowptr[:-1]
        out = res["graphs"][name] = {
            "nodes": N, "edges": plan.nnz, "max_in_degree": int(deg.max()),
            "n_heavy": plan.fwd.n_heavy, "scheduled": plan.fwd.order is not None,
            "mask": {}, "sample": {}, "mean": {}, "sage": {}}
        for k in FANOUTS:
            r = out["mask"][k] = run_mask(plan, k, args.window)
            print(json.dumps({"case": f"{name}/mask/k{k}", "N_ms": r["N_no_schedule"]["median_ms"],
                              "S_ms": r["S_schedule"]["median_ms"],
                              "S2_ms": r["S2_schedule"]["median_ms"],
                              "S_gbs": r["S_schedule"]["gbs"], "of_8tbs": r["S_schedule"]["of_8tbs"],
                              "kept": r["kept"], "schedule_not_slower_than_spread":
                              r["schedule_not_slower_than_spread"]}), flush=True)
            write()
        for k in FANOUTS:
            r = out["sample"][k] = run_sample(plan, ei[1], k, args.window)
            print(json.dumps({"case": f"{name}/sample/k{k}", "A_ms": r["A_torch"]["median_ms"],
                              "A2_ms": r["A2_torch"]["median_ms"],
                              "B_ms": r["B_device"]["median_ms"], "B_over_A": r["ratio_B_over_A"],
                              "spread": r["spread"]}), flush=True)
            write()
        if args.skip_steps:
            continue
        for k in FANOUTS:
            child, keep = mgcn.sample_neighbors(plan, k, seed=1, offset=2)
            for kind, r in (("mean", run_mean(plan, child, args.window)),
                            ("sage", run_sage(ei, ei[:, keep], N, args.window))):
                out[kind][k] = r
                print(json.dumps({"case": f"{name}/{kind}/k{k}", "A_ms": r["A_full"]["median_ms"],
                                  "A2_ms": r["A2_full"]["median_ms"],
                                  "B_ms": r["B_sampled"]["median_ms"],
                                  "B_over_A": r["ratio_B_over_A"], "spread": r["spread"],
                                  "edges_kept": child.nnz}), flush=True)
                write()
            G.clear_cache()
    write()


if __name__ == "__main__":
    main()
