"""A/B of attention over bf16 and fp32 feature rows.

    python scripts/bench_attention_bf16.py [--window 1.0] [--out profiles/attention_bf16/ab.json]

One step is ``attention_aggregate`` forward + backward after ``Hp`` is formed
(scores, softmax + gather, the two adjoint launches, the attention vector's
gradient); the x W GEMM around it is not part of the step.

Graph 1 is the DESIGN "Attention" shape: bench.py's config-2 generator (N = 1M,
10M edges + 1M loops), H = 8, C = 16, 'in', LeakyReLU(0.2).  Three arms
alternate in blocks within one process after a warm-up -- A (fp32), A' (fp32
again: the run's own spread) and B (bf16) -- with enough blocks that every
arm's timed window is at least ``--window`` seconds.  Then, per dtype, a pass
with the kernel-timer hook installed gives the median HIP-event time of every
libmgcn launch of a step.  Graph 2 is the config-3 botnet graph (hub rows, no
heavy-row path in the attention kernels) at H = 4, C = 8, one run per dtype.

Algorithmic bytes per launch come from the shapes (``launch_bytes``: rows at 4
or 2 bytes an element, everything per edge and per (node, head) at 4).  The
JSON holds the times, the bytes, the achieved TB/s, the bf16 / fp32 time and
byte ratios and the A / A' spread; ``faster_than_spread`` says whether B beats
A by more than that spread.  A record: no target is set and the exit status
does not depend on the outcome.
"""
import argparse
import json
import math
import os
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "meta-gcn_amd")]

import torch  # noqa: E402

import mgcn  # noqa: E402,F401
from mgcn import ops  # noqa: E402
from mgcn.graph import plan_for  # noqa: E402
from bench import HBM_PEAK_GBS, make_botnet_graph, make_er_graph  # noqa: E402

BLOCK = 3  # steps per timed block


def launch_bytes(N, nnz, H, C, row_bytes):
    """Bytes every launch of a step has to move ('in'), each operand counted
    once per launch that needs it; ``row_bytes`` per feature-row element."""
    HC = H * C
    rp = 8 * (N + 1)
    rows = row_bytes * N * HC
    sfx = "_bf16" if row_bytes == 2 else ""
    out = {
        "att_scores" + sfx: rows + 4 * (2 * HC + 2 * N * H),
        "att_fwd" + sfx: rp + nnz * (4 + row_bytes * HC + 8 * H) + rows + 4 * N * H,
        "att_bwd_dst" + sfx: rp + nnz * (4 + row_bytes * HC + 12 * H) + rows + 8 * N * H,
        "att_bwd_src" + sfx: rp + nnz * (8 + row_bytes * HC + 8 * H) + rows + 8 * N * H,
        "gemm_tn": 4 * (N * 2 * H + N * HC + 2 * H * HC),  # da, on fp32 rows
    }
    if row_bytes == 2:
        out["upcast_for_gemm_tn"] = 2 * N * HC + 4 * N * HC  # Hp.float(): a torch op
    return out


class EventTimer:
    """mgcn.ops kernel-timer hook: one HIP event pair per libmgcn launch."""

    def __init__(self):
        self.pairs = defaultdict(list)
        self.open = None

    def __call__(self, name, start, rows=None, edges=None):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        if start:
            self.open = ev
        else:
            self.pairs[name].append((self.open, ev))

    def medians(self, steps):
        out = {}
        for name, ps in self.pairs.items():
            per_step = len(ps) // steps
            ms = [sum(a.elapsed_time(b) for a, b in ps[s * per_step:(s + 1) * per_step])
                  for s in range(steps)]
            out[name] = sorted(ms)[len(ms) // 2]
        return out


def make_step(plan, H, Hp, att, dY):
    Hp = Hp.detach().requires_grad_(True)
    att = att.detach().clone().requires_grad_(True)

    def step():
        Hp.grad = att.grad = None
        y, _ = ops.attention_aggregate(Hp, att, plan, H, "lrelu", "in")
        y.backward(dY)
        return y
    return step


def block_events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(BLOCK):
        fn()
    b.record()
    return a, b


def alternate(arms, window_s):
    """arms: {name: fn}.  Blocks of BLOCK steps, the arms taking turns, until
    every arm has at least window_s of timed steps; per-step ms."""
    for fn in arms.values():  # warm-up
        for _ in range(BLOCK):
            fn()
    torch.cuda.synchronize()
    est = {}
    for name, fn in arms.items():
        a, b = block_events(fn)
        torch.cuda.synchronize()
        est[name] = a.elapsed_time(b) / 1e3
    rounds = max(5, math.ceil(1.1 * window_s / min(est.values())))  # 10 % over the estimate
    evs = {name: [] for name in arms}
    for _ in range(rounds):
        for name, fn in arms.items():
            evs[name].append(block_events(fn))
    torch.cuda.synchronize()
    out = {}
    for name, pairs in evs.items():
        ms = sorted(a.elapsed_time(b) / BLOCK for a, b in pairs)
        out[name] = {"median_ms": ms[len(ms) // 2], "mean_ms": sum(ms) / len(ms), "min_ms": ms[0],
                     "max_ms": ms[-1], "steps": BLOCK * len(ms),
                     "window_s": sum(ms) * BLOCK / 1e3}
    return out


def per_launch(step, nbytes, steps=10):
    """Median per-step HIP-event time of every libmgcn launch of ``step``."""
    timer = EventTimer()
    step()
    torch.cuda.synchronize()
    ops.set_kernel_timer(timer)
    try:
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
    finally:
        ops.set_kernel_timer(None)
    out = {}
    for name, ms in timer.medians(steps).items():
        out[name] = {"ms": ms}
        if name in nbytes:
            out[name].update(bytes=nbytes[name], tb_per_s=nbytes[name] / ms / 1e9)
    return out


def few(step, reps=10):
    for _ in range(2):
        step()
    evs = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        evs.append((a, b))
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in evs)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}


def rows_for(N, H, C, seed, dev):
    g = torch.Generator().manual_seed(seed)
    Hp = torch.randn(N, H * C, generator=g).to(torch.bfloat16).to(dev)  # the same values in both
    dY = torch.randn(N, H * C, generator=g).to(torch.bfloat16).to(dev)
    att = (torch.randn(1, H, 2 * C, generator=g) * 0.5).to(dev)
    return Hp, dY, att


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0, help="seconds of timed steps per arm")
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--pairs", type=int, default=5_000_000)
    ap.add_argument("--out",
                    default=os.path.join(ROOT, "profiles", "attention_bf16", "ab.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_attention_bf16.py needs a HIP device")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "hbm_peak_tb_per_s": HBM_PEAK_GBS / 1e3}

    # graph 1: the DESIGN "Attention" shape
    ei, N = make_er_graph(args.nodes, args.pairs)
    plan = plan_for(ei.to(dev), N)
    nnz = plan.nnz
    H, C = 8, 16
    Hp, dY, att = rows_for(N, H, C, 1, dev)
    s32 = make_step(plan, H, Hp.float(), att, dY.float())
    sbf = make_step(plan, H, Hp, att, dY)
    y32, ybf = s32().detach(), sbf().detach()
    same = bool(torch.equal(ybf.view(torch.int16), y32.to(torch.bfloat16).view(torch.int16)))
    b32, bbf = launch_bytes(N, nnz, H, C, 4), launch_bytes(N, nnz, H, C, 2)
    t32, tbf = sum(b32.values()), sum(bbf.values())
    r = alternate({"A_fp32": s32, "A2_fp32": s32, "B_bf16": sbf}, args.window)
    A, A2, B = (r[k]["median_ms"] for k in ("A_fp32", "A2_fp32", "B_bf16"))
    for k, by in (("A_fp32", t32), ("A2_fp32", t32), ("B_bf16", tbf)):
        r[k]["bytes"] = by
        r[k]["tb_per_s"] = by / r[k]["median_ms"] / 1e9
        r[k]["share_of_hbm_peak"] = r[k]["tb_per_s"] * 1e3 / HBM_PEAK_GBS
    r["byte_ratio"] = tbf / t32
    r["ratio_B_over_A"] = B / A
    r["spread_A_A2"] = abs(A - A2) / A
    r["faster_than_spread"] = bool((A - B) / A > r["spread_A_A2"])
    r["Y_bits_equal_rounded_fp32"] = same
    r["per_launch_fp32"] = per_launch(s32, b32)
    r["per_launch_bf16"] = per_launch(sbf, bbf)
    res["attention_shape"] = {"n_nodes": N, "nnz": nnz, "H": H, "C": C, "att_dir": "in",
                              "act": "lrelu", **r}
    del s32, sbf, Hp, dY, y32, ybf, plan, ei

    # graph 2: the botnet graph (hub rows walked by one wave each), H C = 32
    ei3, N3, _ = make_botnet_graph()
    plan3 = plan_for(ei3.to(dev), N3)
    H3, C3 = 4, 8
    Hp3, dY3, att3 = rows_for(N3, H3, C3, 2, dev)
    f32 = few(make_step(plan3, H3, Hp3.float(), att3, dY3.float()))
    f32b = few(make_step(plan3, H3, Hp3.float(), att3, dY3.float()))
    fbf = few(make_step(plan3, H3, Hp3, att3, dY3))
    c32 = sum(launch_bytes(N3, plan3.nnz, H3, C3, 4).values())
    cbf = sum(launch_bytes(N3, plan3.nnz, H3, C3, 2).values())
    spread3 = abs(f32["median_ms"] - f32b["median_ms"]) / f32["median_ms"]
    res["botnet"] = {"n_nodes": N3, "nnz": plan3.nnz, "H": H3, "C": C3,
                     "fp32": f32, "fp32_again": f32b, "bf16": fbf, "byte_ratio": cbf / c32,
                     "ratio_bf16_over_fp32": fbf["median_ms"] / f32["median_ms"],
                     "spread_fp32": spread3,
                     "faster_than_spread": bool(
                         (f32["median_ms"] - fbf["median_ms"]) / f32["median_ms"] > spread3)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    a = res["attention_shape"]
    print(json.dumps({"run": "attention_shape", "A_ms": A, "A2_ms": A2, "B_ms": B,
                      "B_over_A": a["ratio_B_over_A"], "byte_ratio": a["byte_ratio"],
                      "spread": a["spread_A_A2"], "faster_than_spread": a["faster_than_spread"],
                      "Y_bits_equal_rounded_fp32": same}), flush=True)
    for k in ("per_launch_fp32", "per_launch_bf16"):
        print(json.dumps({"run": k, **{n: round(v["ms"], 4) for n, v in a[k].items()}}))
    b = res["botnet"]
    print(json.dumps({"run": "botnet", "fp32_ms": b["fp32"]["median_ms"],
                      "fp32_again_ms": b["fp32_again"]["median_ms"],
                      "bf16_ms": b["bf16"]["median_ms"], "byte_ratio": b["byte_ratio"],
                      "bf16_over_fp32": b["ratio_bf16_over_fp32"],
                      "faster_than_spread": b["faster_than_spread"]}))


if __name__ == "__main__":
    main()
