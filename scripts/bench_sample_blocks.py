"""A/B of the mini-batch block builder against the per-hop composition.

    python scripts/bench_sample_blocks.py [--window 1.0] [--out profiles/sample_blocks/ab.json]

Graphs: bench.py's config-2 generator (1M nodes, 11M slots) and the config-3
botnet-shaped graph; ``fanouts = [10, 10]``; 1024 and 16,384 seeds drawn once
under a fixed generator.  Within one process the arms of a case alternate in
blocks after a warm-up until each has at least ``--window`` seconds of timed
calls; an arm that runs twice (A / A') gives the run's spread.  Host clock,
every call ends in a device synchronise.

  build     A / A': the composition of API that needs no block builder -- per
            hop ``plan.sample_neighbors(k, rows=mask)``, a scatter of the
            sampled sources into a node mask, ``child.induced(nodes,
            relabel=True)`` --, every pass over the parent's edge-sized arrays;
            B: ``mgcn.sample_blocks``.  The same seeds, fan-outs, seed and
            offset: the same edges per hop (A relabels ascending, B
            destinations first).
  sage      a training step of two ``mgcn.pyg.SAGEConv(128, 128)``: A / A' on
            the full graph's sampled edge list (``sample_neighbors(10)``, the
            step scripts/bench_sample_neighbors.py times as its arm B), B on
            two prebuilt blocks, C ``sample_blocks`` + the step on fresh blocks.

``not_slower_than_spread``: (B - A) / A <= |A - A'| / A on the medians;
``faster_than_spread``: (A - B) / A > |A - A'| / A.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "meta-gcn_amd"), os.path.join(ROOT, "scripts")]

import torch  # noqa: E402

import mgcn  # noqa: E402
from mgcn import graph as G  # noqa: E402
from bench import make_er_graph  # noqa: E402
from bench_sample_neighbors import alternate, host_block, verdict  # noqa: E402

FANOUTS = [10, 10]
SEED_COUNTS = (1024, 16384)
SEED, OFFSET = 1, 2


def compose(plan, seeds, fanouts):
    """The per-hop composition: [(relabelled plan, its node ids ascending)]."""
    n = plan.num_nodes
    rows = torch.zeros(n, dtype=torch.bool, device=plan.device)
    rows[seeds] = True
    out = [None] * len(fanouts)
    for l in range(len(fanouts) - 1, -1, -1):
        child, _ = plan.sample_neighbors(fanouts[l], seed=SEED, offset=OFFSET + l, rows=rows)
        nodes = rows.clone()
        nodes[child.fwd.col.long()] = True  # the sampled sources
        out[l] = (child.induced(nodes, relabel=True), nodes)
        rows = nodes
    return out


def run_build(plan, seeds, window_s):
    base = lambda: compose(plan, seeds, FANOUTS)  # noqa: E731
    new = lambda: mgcn.sample_blocks(plan, seeds, FANOUTS, seed=SEED, offset=OFFSET)  # noqa: E731
    r = alternate([("A_compose", base), ("A2_compose", base), ("B_blocks", new)], window_s,
                  host_block, 4)
    a, b = base(), new()
    r["edges"] = [blk.plan.nnz for blk in b]
    r["nodes"] = [blk.n_src for blk in b]
    r["same_edge_counts"] = [p.nnz for p, _ in a] == r["edges"]
    r["same_node_counts"] = [p.num_nodes for p, _ in a] == r["nodes"]
    r = verdict(r, "A_compose", "A2_compose", "B_blocks")
    r["faster_than_spread"] = bool(1.0 - r["ratio_B_over_A"] > r["spread"])
    return r


def run_sage(plan, ei, seeds, window_s, F=128):
    from mgcn.pyg import SAGEConv
    dev = plan.device
    n = plan.num_nodes
    torch.manual_seed(0)
    c1, c2 = SAGEConv(F, F).to(dev), SAGEConv(F, F).to(dev)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(n, F, generator=g).to(dev)
    dy = torch.randn(n, F, generator=g).to(dev)
    child, keep = mgcn.sample_neighbors(plan, FANOUTS[0], seed=SEED, offset=OFFSET)
    ei_child = ei[:, keep]
    mgcn.adopt_plan(ei_child, n, child)
    blocks = mgcn.sample_blocks(plan, seeds, FANOUTS, seed=SEED, offset=OFFSET)
    dy_seeds = dy[seeds]

    def zero():
        for m in (c1, c2):
            m.zero_grad(set_to_none=True)

    def full():
        zero()
        c2(c1(x, ei_child).relu(), ei_child).backward(dy)

    def on_blocks(bl):
        zero()
        h = c1(x[bl[0].src_ids], bl[0].edge_index)[:bl[0].n_dst].relu()
        c2(h, bl[1].edge_index)[:bl[1].n_dst].backward(dy_seeds)

    def fresh():
        on_blocks(mgcn.sample_blocks(plan, seeds, FANOUTS, seed=SEED, offset=OFFSET))

    r = alternate([("A_full_sampled", full), ("A2_full_sampled", full),
                   ("B_blocks", lambda: on_blocks(blocks)), ("C_sample_and_step", fresh)],
                  window_s, host_block, 4)
    r["ratio_C_over_A"] = r["C_sample_and_step"]["median_ms"] / r["A_full_sampled"]["median_ms"]
    r = verdict(r, "A_full_sampled", "A2_full_sampled", "B_blocks")
    r["faster_than_spread"] = bool(1.0 - r["ratio_B_over_A"] > r["spread"])
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0, help="seconds of timed calls per arm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_blocks", "ab.json"))
    ap.add_argument("--small", action="store_true", help="tiny graphs (a rehearsal of the script)")
    ap.add_argument("--skip-steps", action="store_true", help="no training-step arms")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    from mgcn.botnet import make_botnet_graph
    if args.small:
        er, er_n = make_er_graph(20_000, 100_000)
        bot, bot_n, _ = make_botnet_graph(5_000, 12_000, 600, 500, 2_000)
    else:
        er, er_n = make_er_graph()
        bot, bot_n, _ = make_botnet_graph()
    res = {"device": torch.cuda.get_device_name(0), "window_s": args.window, "fanouts": FANOUTS,
           "graphs": {}}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    for name, ei, N in (("config2", er.to(dev), er_n), ("botnet", bot.to(dev), bot_n)):
        plan = G.build_plan(ei, N)
        out = res["graphs"][name] = {"nodes": N, "edges": plan.nnz, "n_heavy": plan.fwd.n_heavy,
                                     "build": {}, "sage": {}}
        perm = torch.randperm(N, generator=torch.Generator().manual_seed(0))
        for n_seeds in SEED_COUNTS:
            seeds = perm[:min(n_seeds, N)].to(dev)
            r = out["build"][n_seeds] = run_build(plan, seeds, args.window)
            print(json.dumps({"case": f"{name}/build/{n_seeds}",
                              "A_ms": r["A_compose"]["median_ms"],
                              "A2_ms": r["A2_compose"]["median_ms"],
                              "B_ms": r["B_blocks"]["median_ms"], "B_over_A": r["ratio_B_over_A"],
                              "spread": r["spread"], "edges": r["edges"], "nodes": r["nodes"],
                              "same_counts": r["same_edge_counts"] and r["same_node_counts"]}),
                  flush=True)
            write()
            if args.skip_steps:
                continue
            r = out["sage"][n_seeds] = run_sage(plan, ei, seeds, args.window)
            print(json.dumps({"case": f"{name}/sage/{n_seeds}",
                              "A_ms": r["A_full_sampled"]["median_ms"],
                              "A2_ms": r["A2_full_sampled"]["median_ms"],
                              "B_ms": r["B_blocks"]["median_ms"],
                              "C_ms": r["C_sample_and_step"]["median_ms"],
                              "B_over_A": r["ratio_B_over_A"], "C_over_A": r["ratio_C_over_A"],
                              "spread": r["spread"]}), flush=True)
            write()
            G.clear_cache()
    write()


if __name__ == "__main__":
    main()
