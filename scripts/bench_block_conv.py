"""A/B of the convs on mini-batch blocks: ``conv(h, block)`` against
``conv(h, block.edge_index)[:n_dst]``.

    python scripts/bench_block_conv.py [--window 1.0] [--out profiles/block_conv/ab.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o bc -- \\
        python scripts/bench_block_conv.py --trace-steps 50
    python scripts/bench_block_conv.py --kernel-stats DIR/.../bc_kernel_stats.csv   (folds it in)

Graphs: bench.py's config-2 generator (1M nodes, 11M slots) and the config-3
botnet-shaped graph; ``fanouts = [10, 10]``; 1024 and 16,384 seeds drawn once
under a fixed generator; the step is forward + backward of two
``mgcn.pyg.SAGEConv(128, 128)`` with a ReLU between.  Within one process the
arms of a case alternate in blocks after a warm-up until each has at least
``--window`` seconds of timed calls.  Host clock, every call ends in a device
synchronise.

  A / A'  the step on prebuilt blocks through ``block.edge_index`` (the shipped
          route: the loop-augmented list and its plan are cached after the
          first call); run twice, their difference is the run's spread
  B       the same step through ``conv(h, block)``
  C       ``sample_blocks`` + the step through ``edge_index`` (fresh blocks: the
          list is edited and its plan built every step)
  D       ``sample_blocks`` + the step through ``conv(h, block)``

Per case the JSON also holds, per layer, the block's shape, whether it took
the block launches or the fallback (heavy rows), and the algorithmic bytes of
its two launches: ``8 (n_dst + 1) + nnz (4 + 4 [w] + 4 F) + 4 F n_dst`` plus
``4 F n_dst`` for the appended loops' rows forward, the same with the rows of
the bwd view (``n_src``) and the loop rows of the destinations for the adjoint.
``--trace-steps`` runs arm B of config 2 at 16,384 seeds alone (for a kernel
trace); ``--kernel-stats`` folds a rocprofv3 kernel_stats.csv of such a run
into the JSON as ``kernels`` (mean time per launch and share of 8 TB/s).
Without one, ``kernels`` says "not measured".
"""
import argparse
import csv
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "meta-gcn_amd"), os.path.join(ROOT, "scripts")]

import torch  # noqa: E402

import mgcn  # noqa: E402
from mgcn import graph as G  # noqa: E402
from mgcn.ops import block_conv_supported  # noqa: E402
from bench import make_er_graph  # noqa: E402
from bench_sample_neighbors import alternate, host_block  # noqa: E402

FANOUTS = [10, 10]
SEED_COUNTS = (1024, 16384)
SEED, OFFSET = 1, 2
F = 128
HBM_BYTES_PER_S = 8e12


def launch_bytes(b, weighted=False):
    """Algorithmic bytes of block_fwd / block_bwd on ``b`` under 'append'."""
    per_slot = 4 + (4 if weighted else 0) + 4 * F
    loops = 4 * F * b.n_dst
    return {"block_fwd": 8 * (b.n_dst + 1) + b.plan.nnz * per_slot + 4 * F * b.n_dst + loops,
            "block_bwd": 8 * (b.n_src + 1) + b.plan.nnz * (per_slot + 4) + 4 * F * b.n_src + loops}


def describe(blocks, x):
    out = []
    for b in blocks:
        took = block_conv_supported(b, x, None)
        out.append({"n_dst": b.n_dst, "n_src": b.n_src, "nnz": b.plan.nnz,
                    "heavy_rows": [b.plan.fwd.n_heavy, b.plan.bwd.n_heavy],
                    "route": "block" if took else "fallback", "bytes": launch_bytes(b)})
    return out


class Step:
    def __init__(self, plan, seeds):
        from mgcn.pyg import SAGEConv
        dev = plan.device
        self.plan, self.seeds = plan, seeds
        torch.manual_seed(0)
        self.c1, self.c2 = SAGEConv(F, F).to(dev), SAGEConv(F, F).to(dev)
        g = torch.Generator().manual_seed(0)
        self.x = torch.randn(plan.num_nodes, F, generator=g).to(dev)
        self.dy = torch.randn(plan.num_nodes, F, generator=g).to(dev)[seeds]
        self.blocks = self.sample()

    def sample(self):
        return mgcn.sample_blocks(self.plan, self.seeds, FANOUTS, seed=SEED, offset=OFFSET)

    def run(self, bl, through_blocks):
        for m in (self.c1, self.c2):
            m.zero_grad(set_to_none=True)
        h = self.x[bl[0].src_ids]
        if through_blocks:
            self.c2(self.c1(h, bl[0]).relu(), bl[1]).backward(self.dy)
        else:
            h = self.c1(h, bl[0].edge_index)[:bl[0].n_dst].relu()
            self.c2(h, bl[1].edge_index)[:bl[1].n_dst].backward(self.dy)


def run_case(plan, seeds, window_s):
    s = Step(plan, seeds)
    arms = [("A_edge_index", lambda: s.run(s.blocks, False)),
            ("A2_edge_index", lambda: s.run(s.blocks, False)),
            ("B_block", lambda: s.run(s.blocks, True)),
            ("C_fresh_edge_index", lambda: s.run(s.sample(), False)),
            ("D_fresh_block", lambda: s.run(s.sample(), True))]
    r = alternate(arms, window_s, host_block, 4)
    A, A2, B, C, D = (r[name]["median_ms"] for name, _ in arms)
    r["spread"] = abs(A - A2) / A
    r["ratio_B_over_A"] = B / A
    r["ratio_D_over_C"] = D / C
    # a difference inside the A / A' spread is level
    for key, ratio in (("B_vs_A", B / A), ("D_vs_C", D / C)):
        r[key] = "level" if abs(ratio - 1.0) <= r["spread"] else \
            ("faster" if ratio < 1.0 else "slower")
    r["layers"] = describe(s.blocks, s.x)
    return r


def fold_kernel_stats(res, path, steps):
    """rocprofv3's kernel_stats.csv of a ``--trace-steps`` run -> res['kernels']."""
    layers = res["graphs"]["config2"]["cases"][str(SEED_COUNTS[-1])]["layers"]
    # the input layer's rows need no gradient: its adjoint is never launched
    per_step = {"block_fwd": sum(l["bytes"]["block_fwd"] for l in layers),
                "block_bwd": layers[-1]["bytes"]["block_bwd"]}
    out = {}
    for row in csv.DictReader(open(path)):
        name = row["Name"]
        if "block_spmm_kernel" not in name:
            continue
        # the last template argument is the mode: 0 forward, 1 / 2 the adjoints
        m = re.search(r"block_spmm_kernel<[^>]*?(\d+)\s*>", name) or \
            re.search(r"block_spmm_kernelILi\d+ELi\d+ELi\d+ELi(\d+)E", name)
        if m is None:
            continue
        key = "block_fwd" if m.group(1) == "0" else "block_bwd"
        e = out.setdefault(key, {"launches": 0, "total_ns": 0.0, "names": []})
        e["launches"] += int(row["Calls"])
        e["total_ns"] += float(row["TotalDurationNs"])
        e["names"].append(name[:120])
    for key, e in out.items():
        e["mean_us"] = e["total_ns"] / max(e["launches"], 1) / 1e3
        e["bytes_per_step"] = per_step[key]
        e["of_8tbs"] = per_step[key] * steps / (e["total_ns"] * 1e-9) / HBM_BYTES_PER_S
    res["kernels"] = {"case": f"config2, {SEED_COUNTS[-1]} seeds, arm B", "steps": steps, **out} \
        if out else "not measured"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0, help="seconds of timed calls per arm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "block_conv", "ab.json"))
    ap.add_argument("--small", action="store_true", help="tiny graphs (a rehearsal of the script)")
    ap.add_argument("--trace-steps", type=int, default=0,
                    help="run only arm B of config 2 at the larger seed count, this many steps")
    ap.add_argument("--kernel-stats", default=None,
                    help="fold a rocprofv3 kernel_stats.csv of a --trace-steps run into --out")
    ap.add_argument("--kernel-stats-steps", type=int, default=50)
    args = ap.parse_args()
    if args.kernel_stats:
        with open(args.out) as f:
            res = json.load(f)
        fold_kernel_stats(res, args.kernel_stats, args.kernel_stats_steps + 2)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps({"kernels": res["kernels"]}))
        return
    dev = torch.device("cuda:0")
    from mgcn.botnet import make_botnet_graph
    if args.small:
        er, er_n = make_er_graph(20_000, 100_000)
        bot, bot_n, _ = make_botnet_graph(5_000, 12_000, 600, 500, 2_000)
    else:
        er, er_n = make_er_graph()
        bot, bot_n, _ = (None, 0, None) if args.trace_steps else make_botnet_graph()
    if args.trace_steps:
        plan = G.build_plan(er.to(dev), er_n)
        perm = torch.randperm(er_n, generator=torch.Generator().manual_seed(0))
        s = Step(plan, perm[:min(SEED_COUNTS[-1], er_n)].to(dev))
        for _ in range(args.trace_steps + 2):  # (two warm-up steps are traced too)
            s.run(s.blocks, True)
        torch.cuda.synchronize()
        return
    res = {"device": torch.cuda.get_device_name(0), "window_s": args.window, "fanouts": FANOUTS,
           "F": F, "small": bool(args.small), "graphs": {}, "kernels": "not measured"}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    for name, ei, N in (("config2", er.to(dev), er_n), ("botnet", bot.to(dev), bot_n)):
        plan = G.build_plan(ei, N)
        out = res["graphs"][name] = {"nodes": N, "edges": plan.nnz, "n_heavy": plan.fwd.n_heavy,
                                     "cases": {}}
        perm = torch.randperm(N, generator=torch.Generator().manual_seed(0))
        for n_seeds in SEED_COUNTS:
            seeds = perm[:min(n_seeds, N)].to(dev)
            r = out["cases"][str(n_seeds)] = run_case(plan, seeds, args.window)
            print(json.dumps({"case": f"{name}/{n_seeds}",
                              "A_ms": r["A_edge_index"]["median_ms"],
                              "A2_ms": r["A2_edge_index"]["median_ms"],
                              "B_ms": r["B_block"]["median_ms"],
                              "C_ms": r["C_fresh_edge_index"]["median_ms"],
                              "D_ms": r["D_fresh_block"]["median_ms"],
                              "B_over_A": r["ratio_B_over_A"], "D_over_C": r["ratio_D_over_C"],
                              "spread": r["spread"], "B_vs_A": r["B_vs_A"], "D_vs_C": r["D_vs_C"],
                              "routes": [l["route"] for l in r["layers"]]}), flush=True)
            write()
            G.clear_cache()
    write()


if __name__ == "__main__":
    main()
