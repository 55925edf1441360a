"""A/B of the bf16 and fp32 aggregation kernels on the config-2 graph.

    python scripts/bench_spmm_bf16.py [--window 1.0] [--out profiles/bf16/spmm_ab.json]

Graph: bench.py's config-2 generator and seeds (N = 1M, 11M slots, F = 128,
deg_norm = 'sm').  Timed with device events: the sum forward and the sum
adjoint, three arms alternating in blocks within one process after a warm-up
-- A (fp32), A' (fp32 again: the run's own spread) and B (bf16) -- with enough
blocks that every arm's timed window is at least ``--window`` seconds.  Then
one mean run, one max run and one run on the config-3 botnet graph at F = 32
(heavy rows) per dtype.

Algorithmic bytes per launch, from the shapes:
    fp32  8 (N + 1) + nnz (8 + 4 F) + 4 N F
    bf16  8 (N + 1) + nnz (8 + 2 F) + 2 N F
(max adds the winner words, 4 ceil(F / 32) bytes per edge.)  The JSON holds
the times, these bytes, the achieved TB/s, the B/A ratio and the A/A' spread;
``faster_than_spread`` says whether B beats A by more than that spread.
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
from mgcn import _lib as L  # noqa: E402
from mgcn import ops  # noqa: E402
from mgcn.graph import plan_for  # noqa: E402
from bench import HBM_PEAK_GBS, make_botnet_graph, make_er_graph  # noqa: E402

BLOCK = 10  # launches per timed block


def bytes_fp32(n, nnz, F, extra_per_edge=0):
    return 8 * (n + 1) + nnz * (8 + 4 * F + extra_per_edge) + 4 * n * F


def bytes_bf16(n, nnz, F, extra_per_edge=0):
    return 8 * (n + 1) + nnz * (8 + 2 * F + extra_per_edge) + 2 * n * F


def block_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(BLOCK):
        fn()
    b.record()
    return a, b


def alternate(arms, window_s):
    """arms: {name: fn}.  Blocks of BLOCK launches, the arms taking turns,
    until every arm has at least window_s of timed launches; per-launch ms."""
    for fn in arms.values():  # warm-up
        for _ in range(BLOCK):
            fn()
    torch.cuda.synchronize()
    est = {}
    for name, fn in arms.items():
        a, b = block_ms(fn)
        torch.cuda.synchronize()
        est[name] = a.elapsed_time(b) / 1e3
    rounds = max(5, math.ceil(1.1 * window_s / min(est.values())))  # 10 % over the estimate
    evs = {name: [] for name in arms}
    for _ in range(rounds):
        for name, fn in arms.items():
            evs[name].append(block_ms(fn))
    torch.cuda.synchronize()
    out = {}
    for name, pairs in evs.items():
        ms = sorted(a.elapsed_time(b) / BLOCK for a, b in pairs)
        out[name] = {"median_ms": ms[len(ms) // 2], "mean_ms": sum(ms) / len(ms), "min_ms": ms[0],
                     "launches": BLOCK * len(ms), "window_s": sum(ms) * BLOCK / 1e3}
    return out


def ab(fn32, fnb, b32, bb, window_s):
    r = alternate({"A_fp32": fn32, "A2_fp32": fn32, "B_bf16": fnb}, window_s)
    A, A2, B = (r[k]["median_ms"] for k in ("A_fp32", "A2_fp32", "B_bf16"))
    r["A_fp32"]["bytes"] = r["A2_fp32"]["bytes"] = b32
    r["B_bf16"]["bytes"] = bb
    for k, by in (("A_fp32", b32), ("A2_fp32", b32), ("B_bf16", bb)):
        r[k]["tb_per_s"] = by / r[k]["median_ms"] / 1e9
        r[k]["share_of_hbm_peak"] = r[k]["tb_per_s"] * 1e3 / HBM_PEAK_GBS
    r["byte_ratio"] = bb / b32
    r["ratio_B_over_A"] = B / A
    r["spread_A_A2"] = abs(A - A2) / A
    r["faster_than_spread"] = bool((A - B) / A > r["spread_A_A2"])
    return r


def one(fn32, fnb, b32, bb, reps=20):
    out = {}
    for name, fn, by in (("fp32", fn32, b32), ("bf16", fnb, bb)):
        for _ in range(3):
            fn()
        evs = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            evs.append((a, b))
        torch.cuda.synchronize()
        ms = sorted(a.elapsed_time(b) for a, b in evs)
        out[name] = {"median_ms": ms[len(ms) // 2], "bytes": by,
                     "tb_per_s": by / ms[len(ms) // 2] / 1e9}
    out["ratio_bf16_over_fp32"] = out["bf16"]["median_ms"] / out["fp32"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0, help="seconds of timed launches per arm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf16", "spmm_ab.json"))
    ap.add_argument("--once", action="store_true",
                    help="one bf16 fwd + bwd launch on the config-2 graph (for a kernel trace)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    SUM, MEAN, MAX = L.REDUCE_SUM, L.REDUCE_MEAN, L.REDUCE_MAX

    ei, N = make_er_graph()
    ei = ei.to(dev)
    F = 128
    plan = plan_for(ei, N)
    norm = plan.norm("sm")
    nnz = plan.nnz
    g = torch.Generator().manual_seed(1)
    H = torch.randn(N, F, generator=g).to(dev)
    Hb = H.to(torch.bfloat16)
    fw, bw, rs = norm.w_fwd, norm.w_bwd, norm.row_scale_bwd
    if args.once:
        ops.spmm_fwd_bf16(plan.fwd, fw, Hb, SUM)
        ops.spmm_bwd_bf16(plan.bwd, bw, rs, Hb, SUM)
        torch.cuda.synchronize()
        return
    res = {"device": torch.cuda.get_device_name(0), "hbm_peak_tb_per_s": HBM_PEAK_GBS / 1e3,
           "config2": {"n_nodes": N, "nnz": nnz, "F": F, "deg_norm": "sm"}}
    b32, bb = bytes_fp32(N, nnz, F), bytes_bf16(N, nnz, F)
    res["config2"]["sum_fwd"] = ab(lambda: ops.spmm_fwd(plan.fwd, fw, H, SUM),
                                   lambda: ops.spmm_fwd_bf16(plan.fwd, fw, Hb, SUM), b32, bb,
                                   args.window)
    res["config2"]["sum_bwd"] = ab(lambda: ops.spmm_bwd(plan.bwd, bw, rs, H, SUM),
                                   lambda: ops.spmm_bwd_bf16(plan.bwd, bw, rs, Hb, SUM), b32, bb,
                                   args.window)
    cnt = plan.in_cnt
    res["config2"]["mean_fwd"] = one(lambda: ops.spmm_fwd(plan.fwd, fw, H, MEAN),
                                     lambda: ops.spmm_fwd_bf16(plan.fwd, fw, Hb, MEAN), b32, bb)
    res["config2"]["mean_bwd"] = one(
        lambda: ops.spmm_bwd(plan.bwd, bw, rs, H, MEAN, cnt=cnt),
        lambda: ops.spmm_bwd_bf16(plan.bwd, bw, rs, Hb, MEAN, cnt=cnt), b32 + 4 * nnz, bb + 4 * nnz)
    wb = 4 * ((F + 31) // 32)  # winner words per edge
    _, win = ops.spmm_fwd(plan.fwd, fw, H, MAX, mask_plan=plan)
    sm = plan.slot_map()
    m32, mb = bytes_fp32(N, nnz, F, wb), bytes_bf16(N, nnz, F, wb)
    res["config2"]["max_fwd"] = one(
        lambda: ops.spmm_fwd(plan.fwd, fw, H, MAX, mask_plan=plan),
        lambda: ops.spmm_fwd_bf16(plan.fwd, fw, Hb, MAX, mask_plan=plan), m32, mb)
    res["config2"]["max_bwd"] = one(
        lambda: ops.spmm_bwd(plan.bwd, bw, rs, H, MAX, win_mask=win, slot_map=sm),
        lambda: ops.spmm_bwd_bf16(plan.bwd, bw, rs, Hb, MAX, win_mask=win, slot_map=sm),
        m32 + 4 * nnz, mb + 4 * nnz)
    del H, Hb, win, plan, norm, ei

    # config 3: the botnet graph (heavy and giant rows), F = 32
    ei3, N3, _ = make_botnet_graph()
    ei3 = ei3.to(dev)
    F3 = 32
    plan3 = plan_for(ei3, N3)
    norm3 = plan3.norm("sm")
    H3 = torch.randn(N3, F3, generator=g).to(dev)
    H3b = H3.to(torch.bfloat16)
    c32, cb = bytes_fp32(N3, plan3.nnz, F3), bytes_bf16(N3, plan3.nnz, F3)
    res["config3_botnet"] = {
        "n_nodes": N3, "nnz": plan3.nnz, "F": F3,
        "n_heavy": [plan3.fwd.n_heavy, plan3.bwd.n_heavy],
        "n_giant": [plan3.fwd.n_giant, plan3.bwd.n_giant],
        "sum_fwd": one(lambda: ops.spmm_fwd(plan3.fwd, norm3.w_fwd, H3, SUM),
                       lambda: ops.spmm_fwd_bf16(plan3.fwd, norm3.w_fwd, H3b, SUM), c32, cb),
        "sum_bwd": one(
            lambda: ops.spmm_bwd(plan3.bwd, norm3.w_bwd, norm3.row_scale_bwd, H3, SUM),
            lambda: ops.spmm_bwd_bf16(plan3.bwd, norm3.w_bwd, norm3.row_scale_bwd, H3b, SUM),
            c32, cb)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    c2 = res["config2"]
    for k in ("sum_fwd", "sum_bwd"):
        print(json.dumps({"run": k, "A_ms": c2[k]["A_fp32"]["median_ms"],
                          "A2_ms": c2[k]["A2_fp32"]["median_ms"],
                          "B_ms": c2[k]["B_bf16"]["median_ms"], "B_over_A": c2[k]["ratio_B_over_A"],
                          "spread": c2[k]["spread_A_A2"], "B_tb_per_s": c2[k]["B_bf16"]["tb_per_s"],
                          "faster_than_spread": c2[k]["faster_than_spread"]}), flush=True)
    for k in ("mean_fwd", "mean_bwd", "max_fwd", "max_bwd"):
        print(json.dumps({"run": k, **{d: c2[k][d]["median_ms"] for d in ("fp32", "bf16")}}))
    for k in ("sum_fwd", "sum_bwd"):
        print(json.dumps({"run": "botnet_" + k, **{d: res["config3_botnet"][k][d]["median_ms"]
                                                    for d in ("fp32", "bf16")}}))
    if not (c2["sum_fwd"]["faster_than_spread"] and c2["sum_bwd"]["faster_than_spread"]):
        sys.exit("bf16 is not faster than fp32 by more than the A/A' spread")


if __name__ == "__main__":
    main()
