"""A/B of the fused multi-kernel route against the loop over the kernels.

    python scripts/bench_multi_kernel.py [--window 1.0] [--shapes 2x32,2x128,3x32,3x128]
                                         [--force] [--out profiles/multi_kernel/ab.json]

Graphs: bench.py's config-2 generator (N = 1M, 11M slots), K independent edge
sets (seeds 0 .. K - 1), deg_norm = 'sm'.  One
``GCNLayer(C, C, num_kernel=K, non_linear='relu')`` forward + backward per
step, x with gradient, timed with device events.  Three arms alternate in
blocks within one process after a warm-up -- A (switch off: the loop), A'
(off again: the run's own spread) and B (switch on: one launch per direction)
-- with enough blocks that every arm's timed window is at least ``--window``
seconds.  On a tree without the switch only the loop arm runs (the same script
on the parent commit).  At a shape the routing predicate declines
(``multi_kernel_fusable``: 128 -> 128, where the loop runs the fused layer
kernels) arm B runs the loop too and ``B_route`` says so; ``--force`` lifts
that exclusion for the run, which is how the numbers behind it were taken.

Algorithmic bytes of one step, from the shapes (S_k = 8 (N + 1) + nnz_k
(8 + 4 C), the rows one aggregation of kernel k gathers with its metadata;
R = 4 N C, one pass over an [N, C] table):

  fused   forward   GEMM x [W_0 | ..]: R + K R (+ weights);  launch: sum S_k + R
          backward  ReLU / bias pass 3 R;  launch: sum S_k + K R;
                    dense backward (dW_all, dx): 2 (K R + R)
  loop    forward   per kernel GEMM 2 R + aggregation S_k + R (the 128 -> 128
                    fused layer kernel: S_k + R, no GEMM);  K - 1 adds 3 R each;
                    ReLU 2 R
          backward  ReLU 3 R;  per kernel bias sums R, adjoint S_k + R, dense
                    backward 4 R (fused layer kernel: S_k + 2 R);  K - 1 dx adds
                    3 R each

The JSON holds the times, these bytes, the B / A ratio and the A / A' spread;
``not_slower_than_spread`` says whether B is within that spread of A or
faster.  The exit status is nonzero when B is slower at any shape.
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "meta-gcn_amd")]

import torch  # noqa: E402

import mgcn  # noqa: E402,F401
from mgcn import ops  # noqa: E402
from mgcn.graph import plan_for  # noqa: E402
from mgcn.models import GCNLayer  # noqa: E402
from bench import make_er_graph  # noqa: E402

BLOCK = 4  # steps per timed block
HAS_SWITCH = hasattr(ops, "set_fused_multi_kernel")


def step_bytes(N, nnzs, C, xw_layers):
    """(fused, loop) algorithmic bytes of one forward + backward (module docstring)."""
    K = len(nnzs)
    R = 4 * N * C
    S = sum(8 * (N + 1) + nnz * (8 + 4 * C) for nnz in nnzs)
    W = 4 * C * C
    fused_f = (R + K * R + K * W) + (S + R)
    fused_b = 3 * R + (S + K * R) + 2 * (K * R + R) + 2 * K * W
    if xw_layers:
        loop_f = S + K * (R + W)
        loop_b = K * R + S + K * (2 * R + 2 * W)
    else:
        loop_f = K * (2 * R + W) + S + K * R
        loop_b = K * R + S + K * R + K * (4 * R + 2 * W)
    loop_f += (K - 1) * 3 * R + 2 * R
    loop_b += 3 * R + (K - 1) * 3 * R
    return {"fused_fwd": fused_f, "fused_bwd": fused_b, "loop_fwd": loop_f, "loop_bwd": loop_b}


def block_events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(BLOCK):
        fn()
    b.record()
    return a, b


def alternate(arms, window_s):
    """arms: [(name, fn)].  Blocks of BLOCK steps, the arms taking turns, until
    every arm has at least window_s of timed steps; per-step ms."""
    for _, fn in arms:  # warm-up
        for _ in range(BLOCK):
            fn()
    torch.cuda.synchronize()
    est = []
    for _, fn in arms:
        a, b = block_events(fn)
        torch.cuda.synchronize()
        est.append(a.elapsed_time(b) / 1e3)
    rounds = max(5, math.ceil(1.1 * window_s / min(est)))  # 10 % over the estimate
    evs = {name: [] for name, _ in arms}
    for _ in range(rounds):
        for name, fn in arms:
            evs[name].append(block_events(fn))
    torch.cuda.synchronize()
    out = {}
    for name, pairs in evs.items():
        ms = sorted(a.elapsed_time(b) / BLOCK for a, b in pairs)
        out[name] = {"median_ms": ms[len(ms) // 2], "mean_ms": sum(ms) / len(ms), "min_ms": ms[0],
                     "steps": BLOCK * len(ms), "window_s": sum(ms) * BLOCK / 1e3}
    return out


def run_shape(K, C, eis, N, window_s, dev):
    torch.manual_seed(0)
    layer = GCNLayer(C, C, deg_norm='sm', num_kernel=K, non_linear='relu').to(dev)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(N, C, generator=g).to(dev).requires_grad_(True)
    dY = torch.randn(N, C, generator=g).to(dev)
    eis = eis[:K]
    plans = [plan_for(ei, N) for ei in eis]

    def step(fused):
        def fn():
            if HAS_SWITCH:
                ops.set_fused_multi_kernel(fused)
            x.grad = None
            layer.zero_grad(set_to_none=True)
            layer(x, eis).backward(dY)
        return fn

    names = []
    ops.set_kernel_timer(lambda name, start, rows=None, edges=None:
                         names.append(name) if start else None)
    launches = {}
    for arm, fused in (("A_loop", False), ("B_fused", True)):
        if fused and not HAS_SWITCH:
            continue
        del names[:]
        step(fused)()
        launches[arm] = sorted(set(names))
    ops.set_kernel_timer(None)
    if HAS_SWITCH:
        arms = [("A_loop", step(False)), ("A2_loop", step(False)), ("B_fused", step(True))]
    else:
        arms = [("A_loop", step(False)), ("A2_loop", step(False))]
    r = alternate(arms, window_s)
    if HAS_SWITCH:
        ops.set_fused_multi_kernel(True)
    xw = any(n.startswith("spmm_xw") for n in launches["A_loop"])
    r["bytes"] = step_bytes(N, [p.nnz for p in plans], C, xw)
    r["launches"] = launches
    if HAS_SWITCH:
        r["B_route"] = ("fused" if any(n.startswith("multi_spmm") for n in launches["B_fused"])
                        else "loop")
    A, A2 = r["A_loop"]["median_ms"], r["A2_loop"]["median_ms"]
    r["spread_A_A2"] = abs(A - A2) / A
    if HAS_SWITCH:
        B = r["B_fused"]["median_ms"]
        r["ratio_B_over_A"] = B / A
        r["byte_ratio_fused_over_loop"] = ((r["bytes"]["fused_fwd"] + r["bytes"]["fused_bwd"]) /
                                           (r["bytes"]["loop_fwd"] + r["bytes"]["loop_bwd"]))
        r["not_slower_than_spread"] = bool((B - A) / A <= r["spread_A_A2"])
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0, help="seconds of timed steps per arm")
    ap.add_argument("--shapes", default="2x32,2x128,3x32,3x128", help="KxC, comma separated")
    ap.add_argument("--force", action="store_true",
                    help="take the fused route at the shapes the predicate excludes as well")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_kernel", "ab.json"))
    args = ap.parse_args()
    if args.force:
        from mgcn import models
        fusable = models.multi_kernel_fusable
        models.multi_kernel_fusable = lambda *a, out_channels=None, **kw: fusable(*a, **kw)
    dev = torch.device("cuda:0")
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    N = None
    eis = []
    for seed in range(max(K for K, _ in shapes)):
        ei, N = make_er_graph(seed=seed)
        eis.append(ei.to(dev))
    res = {"device": torch.cuda.get_device_name(0), "n_nodes": N, "deg_norm": "sm",
           "has_fused_route": HAS_SWITCH, "forced": bool(args.force), "shapes": {}}
    for K, C in shapes:
        r = run_shape(K, C, eis, N, args.window, dev)
        res["shapes"][f"K{K}_C{C}"] = r
        line = {"K": K, "C": C, "A_ms": r["A_loop"]["median_ms"], "A2_ms": r["A2_loop"]["median_ms"],
                "spread": r["spread_A_A2"]}
        if HAS_SWITCH:
            line.update({"B_ms": r["B_fused"]["median_ms"], "B_over_A": r["ratio_B_over_A"],
                         "bytes_B_over_A": r["byte_ratio_fused_over_loop"], "B_route": r["B_route"],
                         "not_slower_than_spread": r["not_slower_than_spread"]})
        print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    if HAS_SWITCH and not all(r["not_slower_than_spread"] for r in res["shapes"].values()):
        sys.exit("the fused route is slower than the loop by more than the A/A' spread")


if __name__ == "__main__":
    main()
