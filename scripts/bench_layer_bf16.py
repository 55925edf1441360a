"""A/B of a bf16 GCN layer with and without the fused bf16 kernel, config-2 graph.

    python scripts/bench_layer_bf16.py [--window 1.0] [--out profiles/bf16_fused/ab.json]

Graph: bench.py's config-2 generator and seeds (N = 1M, 11M slots, F = 128,
deg_norm = 'sm').  Timed with device events, three arms alternating in blocks
within one process after a warm-up -- A (today's bf16 layer: the vendor GEMM,
then the bf16 aggregation; the switch off), A' (the same again: the run's own
spread) and B (mgcn_spmm_xw_bf16; the switch on) -- with enough blocks that
every arm's timed window is at least ``--window`` seconds.  Medians per call.

Runs: the forward without Z (inference), the forward as training runs it (B
also writes Z), the adjoint to dx, and a full forward + backward step of a
3-layer GCNStack (parameter gradients; bf16 activations, fp32 masters).  The
fp32 fused layer (mgcn_spmm_xw_fwd / _bwd) is timed beside them, one arm.

Algorithmic bytes, from the shapes (M = 8 (N + 1) + 8 nnz of metadata):
    A forward   GEMM 2NF + 2NF, aggregation M + 2F nnz + 2NF
    B forward   M + 2F nnz + 2NF   (+ 2NF with Z)
    A adjoint   aggregation M + 2F nnz + 2NF, GEMM 2NF + 2NF
    B adjoint   M + 2F nnz + 2NF
    fp32 fused  8 (N + 1) + nnz (8 + 4F) + 4NF
(the 32 KB of W are left out).  ``faster_than_spread`` says whether B beats A
by more than the A/A' spread."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "meta-gcn_amd")]

import torch  # noqa: E402

import mgcn  # noqa: E402,F401
from mgcn import _lib as L  # noqa: E402
from mgcn import ops  # noqa: E402
from mgcn.graph import plan_for  # noqa: E402
from mgcn.models import GCNLayer, GCNStack  # noqa: E402
from bench import HBM_PEAK_GBS, make_er_graph  # noqa: E402
from bench_spmm_bf16 import alternate  # noqa: E402

BF16 = torch.bfloat16


def ab(fn_a, fn_b, bytes_a, bytes_b, window_s):
    r = alternate({"A": fn_a, "A2": fn_a, "B": fn_b}, window_s)
    A, A2, B = (r[k]["median_ms"] for k in ("A", "A2", "B"))
    for k, by in (("A", bytes_a), ("A2", bytes_a), ("B", bytes_b)):
        if by:
            r[k]["bytes"] = by
            r[k]["tb_per_s"] = by / r[k]["median_ms"] / 1e9
            r[k]["share_of_hbm_peak"] = r[k]["tb_per_s"] * 1e3 / HBM_PEAK_GBS
    if bytes_a and bytes_b:
        r["byte_ratio"] = bytes_b / bytes_a
    r["ratio_B_over_A"] = B / A
    r["spread_A_A2"] = abs(A - A2) / A
    r["faster_than_spread"] = bool((A - B) / A > r["spread_A_A2"])
    return r


def one(fn, nbytes, window_s):
    r = alternate({"fp32": fn}, window_s)["fp32"]
    r["bytes"] = nbytes
    r["tb_per_s"] = nbytes / r["median_ms"] / 1e9
    return r


def with_switch(value, fn):
    def run():
        ops.set_bf16_fused_layers(value)
        try:
            return fn()
        finally:
            ops.set_bf16_fused_layers(False)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0, help="seconds of timed calls per arm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf16_fused", "ab.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    SUM = L.REDUCE_SUM

    ei, N = make_er_graph()
    ei = ei.to(dev)
    F = 128
    plan = plan_for(ei, N)
    norm = plan.norm("sm")
    nnz = plan.nnz
    assert plan.fwd.n_heavy == 0 and plan.bwd.n_heavy == 0
    g = torch.Generator().manual_seed(1)
    x32 = torch.randn(N, F, generator=g).to(dev)
    dy32 = torch.randn(N, F, generator=g).to(dev)
    W32 = (torch.randn(F, F, generator=g) * 0.09).to(dev)
    b32 = (torch.randn(F, generator=g) * 0.1).to(dev)
    x, dy, W = x32.to(BF16), dy32.to(BF16), W32.to(BF16)
    fw, bw, rs = norm.w_fwd, norm.w_bwd, norm.row_scale_bwd

    meta = 8 * (N + 1) + 8 * nnz
    agg = meta + 2 * F * nnz + 2 * N * F
    gemm = 4 * N * F
    fp32 = 8 * (N + 1) + nnz * (8 + 4 * F) + 4 * N * F
    res = {"device": torch.cuda.get_device_name(0), "hbm_peak_tb_per_s": HBM_PEAK_GBS / 1e3,
           "config2": {"n_nodes": N, "nnz": nnz, "F": F, "deg_norm": "sm"},
           "bytes": {"A_fwd": agg + gemm, "B_fwd": agg, "B_fwd_z": agg + 2 * N * F,
                     "A_bwd": agg + gemm, "B_bwd": agg, "fp32_fused": fp32}}

    def a_fwd():
        return ops.spmm_fwd_bf16(plan.fwd, fw, torch.matmul(x, W), SUM, b32, True)[0]

    def a_bwd():
        return torch.matmul(ops.spmm_bwd_bf16(plan.bwd, bw, rs, dy, SUM), W.t())

    with torch.no_grad():
        res["fwd"] = ab(a_fwd, lambda: ops.spmm_xw_fwd_bf16(plan.fwd, fw, x, W, SUM, b32, True),
                        agg + gemm, agg, args.window)
        res["fwd_z"] = ab(a_fwd, lambda: ops.spmm_xw_fwd_bf16(plan.fwd, fw, x, W, SUM, b32, True,
                                                              want_z=True),
                          agg + gemm, agg + 2 * N * F, args.window)
        res["bwd_dx"] = ab(a_bwd, lambda: ops.spmm_xw_bwd_bf16(plan.bwd, bw, rs, dy, W),
                           agg + gemm, agg, args.window)
        res["fp32_fused_fwd"] = one(
            lambda: ops.spmm_xw_fwd(plan.fwd, fw, x32, W32, SUM, b32, True), fp32, args.window)
        res["fp32_fused_bwd_dx"] = one(
            lambda: ops.spmm_xw_bwd(plan.bwd, bw, rs, dy32, None, W32), fp32, args.window)

    # a 3-layer stack, forward + backward (parameter gradients)
    torch.manual_seed(0)
    stack = GCNStack([GCNLayer(F, F), GCNLayer(F, F), GCNLayer(F, F, non_linear="none")]).to(dev)

    def step(inp, dout):
        def run():
            for p in stack.parameters():
                p.grad = None
            stack(inp, ei).backward(dout)
        return run

    names = []
    ops.set_kernel_timer(lambda name, start, rows=None, edges=None: start and names.append(name))
    with_switch(True, step(x, dy))()
    ops.set_kernel_timer(None)
    res["stack3_step_B_launches"] = names
    res["stack3_step"] = ab(with_switch(False, step(x, dy)), with_switch(True, step(x, dy)), 0, 0,
                            args.window)
    res["stack3_step_fp32_fused"] = alternate({"fp32": step(x32, dy32)}, args.window)["fp32"]

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    for k in ("fwd", "fwd_z", "bwd_dx", "stack3_step"):
        r = res[k]
        print(json.dumps({"run": k, "A_ms": r["A"]["median_ms"], "A2_ms": r["A2"]["median_ms"],
                          "B_ms": r["B"]["median_ms"], "B_over_A": r["ratio_B_over_A"],
                          "byte_ratio": r.get("byte_ratio"), "spread": r["spread_A_A2"],
                          "faster_than_spread": r["faster_than_spread"]}), flush=True)
    for k in ("fp32_fused_fwd", "fp32_fused_bwd_dx", "stack3_step_fp32_fused"):
        print(json.dumps({"run": k, "ms": res[k]["median_ms"]}), flush=True)


if __name__ == "__main__":
    main()
