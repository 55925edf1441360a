"""A/B of deriving the plan of an edge subset against rebuilding it.

    python scripts/bench_derived_plan.py [--window 1.0] [--out profiles/derived_plan/ab.json]

Per shape three arms alternate in blocks within one process after a warm-up,
until each has at least ``--window`` seconds of timed calls:

  A   build_plan(edge_index[:, keep], N)      what a tree without derived plans does
  A'  the same again                          the run's own spread
  B   parent.select_edges(keep)               libmgcn mgcn_edge_rank + mgcn_csr_derive

and, for the relabelled node filter (TopK / SAG pooling, VotePool relabel):

  A   build_plan(filter_adj(edge_index, None, perm, N)[0], len(perm))
  B   parent.induced(perm, relabel=True)

Every call is timed with the host clock and ends in a device synchronise: the
host waits inside the calls (the out-of-range check of each mgcn_csr_build,
the read-backs of the row schedule, the edge count) are part of what is
compared.  ``keep`` and ``perm`` are fixed per shape; the parent plan is built
before the clock starts (a cache hit in the modules).

Shapes: bench.py's config-2 generator (1M nodes, 11M slots) at keep 0.8 and
0.5, the config-3 botnet-shaped graph, a batch of 128 graphs of the
MUTAG-shaped synthetic set; ``induced`` at ratio 0.5 on the first and third.

Bytes B must move at the least, from the shapes (E parent edges, E' kept, N
nodes; int32 slots, int64 row pointers):

  edge_rank    keep read in two passes 2 E, eid_new written 4 E
  per view     count pass: eid 4 E, eid_new gathered 4 E, new ids stored 4 E
               emit pass:  new ids 4 E, prefixes 4 E, col 4 E, outputs 8 E'
               row pointers: 8 (N + 1) read, 4 (N + 1) gathered, 8 (N + 1) written
  (the row schedule of both views, shared with the rebuild, is not counted)

``bytes_over_time_gbs`` is those bytes over the whole call's time -- a
whole-call rate, host waits and the row schedule included, not a kernel's.

Module steps with ``mgcn.graph.set_derived_plans`` on and off, alternating in
the same way: one training step of a 2-layer VotePoolModel on the
botnet-shaped graph (the wiring of ``votepool.prune``), one of GraphConv ->
TopKPooling(0.5) -> GraphConv on the MUTAG-shaped batch (the wiring of
``pool._select``; both reuse the edge mask the torch code computed, which
``induced`` has to form itself), and one training step of the config-2 GCNStack with
DropEdge at p = 0.2 (``drop_edges`` + ``adopt_plan`` against boolean indexing
+ ``plan_for``; the child is re-normalised either way).

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

import mgcn  # noqa: E402,F401
from mgcn import graph as G  # noqa: E402
from mgcn.pool import filter_adj  # noqa: E402
from bench import make_er_graph, make_inputs, make_stack  # noqa: E402

BLOCK = 4  # calls per timed block


def derive_bytes(N, E, E_out):
    view = E * (4 + 4 + 4) + E * (4 + 4 + 4) + 8 * E_out + 20 * (N + 1)
    return 2 * E + 4 * E + 2 * view


def timed_block(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(BLOCK):
        fn()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / BLOCK * 1e3  # ms per call


def alternate(arms, window_s):
    """arms: [(name, fn)].  Blocks of BLOCK calls, the arms taking turns, until
    every arm has at least window_s of timed calls; per-call ms."""
    for _, fn in arms:  # warm-up
        timed_block(fn)
    est = [timed_block(fn) * BLOCK / 1e3 for _, fn in arms]
    rounds = max(5, math.ceil(1.1 * window_s / min(est)))
    ms = {name: [] for name, _ in arms}
    for _ in range(rounds):
        for name, fn in arms:
            ms[name].append(timed_block(fn))
    out = {}
    for name, v in ms.items():
        v = sorted(v)
        out[name] = {"median_ms": v[len(v) // 2], "mean_ms": sum(v) / len(v), "min_ms": v[0],
                     "calls": BLOCK * len(v), "window_s": sum(v) * BLOCK / 1e3}
    return out


def verdict(r, a="A", a2="A2", b="B"):
    A, A2, B = r[a]["median_ms"], r[a2]["median_ms"], r[b]["median_ms"]
    r["spread_A_A2"] = abs(A - A2) / A
    r["ratio_B_over_A"] = B / A
    r["not_slower_than_spread"] = bool((B - A) / A <= r["spread_A_A2"])
    return r


def same_plan(a, b):
    ok = a.num_nodes == b.num_nodes and a.nnz == b.nnz and torch.equal(a.in_cnt, b.in_cnt)
    for va, vb in ((a.fwd, b.fwd), (a.bwd, b.bwd)):
        ok = ok and all(torch.equal(getattr(va, f), getattr(vb, f)) for f in ("rowptr", "col", "eid"))
        ok = ok and (va.n_heavy, va.n_giant) == (vb.n_heavy, vb.n_giant)
        ok = ok and ((va.order is None and vb.order is None) or
                     (va.order is not None and vb.order is not None and
                      torch.equal(va.order, vb.order)))
    return bool(ok)


def run_select(ei, N, p_keep, window_s):
    parent = G.build_plan(ei, N)
    g = torch.Generator(device=ei.device).manual_seed(0)
    keep = torch.rand(ei.size(1), device=ei.device, generator=g) < p_keep
    rebuild = lambda: G.build_plan(ei[:, keep], N)
    derive = lambda: parent.select_edges(keep)
    equal = same_plan(derive(), rebuild())
    r = alternate([("A", rebuild), ("A2", rebuild), ("B", derive)], window_s)
    E_out = int(keep.sum())
    r.update({"nodes": N, "edges": int(ei.size(1)), "edges_kept": E_out, "equal_to_rebuild": equal,
              "bytes_B": derive_bytes(N, int(ei.size(1)), E_out)})
    r["bytes_over_time_gbs"] = r["bytes_B"] / (r["B"]["median_ms"] * 1e-3) / 1e9
    return verdict(r)


def run_induced(ei, N, ratio, window_s):
    parent = G.build_plan(ei, N)
    g = torch.Generator(device=ei.device).manual_seed(1)
    perm = torch.randperm(N, device=ei.device, generator=g)[:int(ratio * N)]
    n_out = int(perm.numel())
    rebuild = lambda: G.build_plan(filter_adj(ei, None, perm, N)[0], n_out)
    derive = lambda: parent.induced(perm, relabel=True)
    equal = same_plan(derive(), rebuild())
    r = alternate([("A", rebuild), ("A2", rebuild), ("B", derive)], window_s)
    r.update({"nodes": N, "edges": int(ei.size(1)), "nodes_kept": n_out,
              "edges_kept": derive().nnz, "equal_to_rebuild": equal})
    return verdict(r)


def run_switch(step, window_s):
    def arm(on):
        def fn():
            G.set_derived_plans(on)
            step(on)
        return fn
    r = alternate([("A_rebuild", arm(False)), ("A2_rebuild", arm(False)), ("B_derived", arm(True))],
                  window_s)
    G.set_derived_plans(True)
    return verdict(r, "A_rebuild", "A2_rebuild", "B_derived")


def votepool_step(ei, N, dev):
    from mgcn.votepool import VotePoolModel
    torch.manual_seed(0)
    model = VotePoolModel(8, [32, 32], 2, residual=True, nheads=[2, 2], att_act="lrelu",
                          temperature=0.5, relabel=False).to(dev).train()
    x = torch.randn(N, 8, generator=torch.Generator().manual_seed(1)).to(dev)

    def step(on):
        model.zero_grad(set_to_none=True)
        model(x, ei, [0, N]).square().sum().backward()
    return step


def dropedge_step(ei, N, dev, p=0.2):
    X, Ws, bs, dY = make_inputs(N, 128, 3)
    stack = make_stack(dev, Ws, bs)
    params = list(stack.parameters())
    Xd, dYd = X.to(dev), dY.to(dev)
    parent = G.plan_for(ei, N)

    def step(on):
        for q in params:
            q.grad = None
        if on:
            child, keep = G.drop_edges(parent, p)
            ei_t = ei[:, keep]
            G.adopt_plan(ei_t, N, child)
        else:
            ei_t = ei[:, torch.rand(ei.size(1), device=dev) >= p]
        stack(Xd, ei_t).backward(dYd)
    return step


def topk_step(ei, N, batch, dev):
    from mgcn.pool import TopKPooling
    from mgcn.pyg import GraphConv
    torch.manual_seed(0)
    conv0, pool, conv = GraphConv(16, 32).to(dev), TopKPooling(32, ratio=0.5).to(dev), \
        GraphConv(32, 32).to(dev)
    x = torch.randn(N, 16, generator=torch.Generator().manual_seed(1)).to(dev)

    def step(on):
        for m in (conv0, pool, conv):
            m.zero_grad(set_to_none=True)
        h = conv0(x, ei).relu()
        h, ei2, _, _, _, _ = pool(h, ei, batch=batch)
        conv(h, ei2).square().sum().backward()
    return step


def mutag_batch(n_graphs=128):
    from mgcn.kernel.data import Batch, synthetic_tu
    ds = synthetic_tu()
    b = Batch.from_data_list([ds[j] for j in range(n_graphs)])
    return b.edge_index, b.num_nodes, b.batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0, help="seconds of timed calls per arm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "derived_plan", "ab.json"))
    ap.add_argument("--small", action="store_true", help="tiny graphs (a rehearsal of the script)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.small:
        er, er_n = make_er_graph(20_000, 100_000)
        from mgcn.botnet import make_botnet_graph
        bot, bot_n, _ = make_botnet_graph(5_000, 12_000, 600, 500, 2_000)
    else:
        er, er_n = make_er_graph()
        from mgcn.botnet import make_botnet_graph
        bot, bot_n, _ = make_botnet_graph()
    mu, mu_n, mu_b = mutag_batch()
    er, bot, mu, mu_b = er.to(dev), bot.to(dev), mu.to(dev), mu_b.to(dev)
    res = {"device": torch.cuda.get_device_name(0), "window_s": args.window, "select_edges": {},
           "induced": {}, "steps": {}}

    def show(kind, name, r):
        res[kind][name] = r
        a, a2, b = [k for k in r if isinstance(r[k], dict) and "median_ms" in r[k]]
        print(json.dumps({"case": f"{kind}/{name}", "A_ms": r[a]["median_ms"],
                          "A2_ms": r[a2]["median_ms"], "B_ms": r[b]["median_ms"],
                          "B_over_A": r["ratio_B_over_A"], "spread": r["spread_A_A2"],
                          "not_slower_than_spread": r["not_slower_than_spread"],
                          "equal_to_rebuild": r.get("equal_to_rebuild"),
                          "gbs": r.get("bytes_over_time_gbs")}), flush=True)

    show("select_edges", "config2_keep0.8", run_select(er, er_n, 0.8, args.window))
    show("select_edges", "config2_keep0.5", run_select(er, er_n, 0.5, args.window))
    show("select_edges", "botnet_keep0.8", run_select(bot, bot_n, 0.8, args.window))
    show("select_edges", "mutag_batch_keep0.8", run_select(mu, mu_n, 0.8, args.window))
    show("induced", "config2_ratio0.5", run_induced(er, er_n, 0.5, args.window))
    show("induced", "botnet_ratio0.5", run_induced(bot, bot_n, 0.5, args.window))
    show("induced", "mutag_batch_ratio0.5", run_induced(mu, mu_n, 0.5, args.window))
    G.clear_cache()
    show("steps", "votepool_botnet", run_switch(votepool_step(bot, bot_n, dev), args.window))
    G.clear_cache()
    show("steps", "topk_mutag_batch", run_switch(topk_step(mu, mu_n, mu_b, dev), args.window))
    G.clear_cache()
    show("steps", "dropedge_config2_p0.2", run_switch(dropedge_step(er, er_n, dev), args.window))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
