"""A/B of the edge gates over bf16 and fp32 feature rows.

    python scripts/bench_edge_gate_bf16.py [--window 1.0] [--out profiles/edge_gate_bf16/ab.json]

One step is ``gate_aggregate`` forward + backward after ``Hx`` is formed
(scores, gate + gather, the two adjoint launches, the gate vectors' gradient;
'proj' gate with a scalar bias, bias + ReLU in the epilogue); the x W GEMM
around it is not part of the step.

Shapes: the config-3 botnet graph at C = 32 without a norm (heavy rows on: the
gated botnet runs), and bench.py's config-2 generator under 'sm' at C = 32 and
C = 128.  Per shape three arms alternate in blocks within one process after a
warm-up -- A (fp32), A2 (fp32 again: the run's own spread) and B (bf16) -- with
enough blocks that every arm's timed window is at least ``--window`` seconds.
Then, per dtype, a pass with the kernel-timer hook installed gives the median
HIP-event time of every libmgcn launch of a step.

Algorithmic bytes per launch come from the shapes (``launch_bytes``: rows at 4
or 2 bytes an element, everything per edge and per node at 4).  The JSON holds
the times, the bytes, the achieved TB/s, the bf16 / fp32 time and byte ratios
and the A / A2 spread; ``faster_than_spread`` says whether B beats A by more
than that spread.  Then ms per step of the 12-layer gated GCNModel of
src/run/run_debru_32_eg.sh on the config-3 graph: fp32, bf16 input with fp32
master parameters, and the model after ``.to(torch.bfloat16)``.  A record: no
target is set and the exit status does not depend on the outcome.
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
from bench import HBM_PEAK_GBS, make_botnet_graph, make_er_graph  # noqa: E402
from bench_attention_bf16 import alternate, per_launch  # noqa: E402

BF16 = torch.bfloat16


def launch_bytes(N, nnz, C, weighted, row_bytes, heavy):
    """Bytes every launch of a step has to move, each operand counted once per
    launch that needs it; ``row_bytes`` per feature-row element."""
    rp = 8 * (N + 1)
    rows = row_bytes * N * C
    w = 4 * nnz if weighted else 0
    sfx = ("_heavy" if heavy else "") + ("_bf16" if row_bytes == 2 else "")
    bf = "_bf16" if row_bytes == 2 else ""
    out = {
        "att_scores" + bf: rows + 8 * N,
        "gate_fwd" + sfx: rp + nnz * (4 + row_bytes * C + 4 + 4) + w + rows + 4 * N,
        "relu_bwd_colsum" + bf: 3 * rows,
        "gate_bwd_dst" + sfx: rp + nnz * (4 + row_bytes * C + 4 + 4) + w + rows + 4 * N,
        "gate_bwd_src" + sfx: rp + nnz * (4 + 4 + row_bytes * C + 4 + 4) + w + rows + 12 * N,
        "gemm_tn": 4 * N * C + 8 * N,  # [da | dc]^T Hx on fp32 rows
    }
    if row_bytes == 2:
        out["upcasts_for_gemm_tn_and_db"] = 2 * (2 * N * C + 4 * N * C)  # torch ops
        out["relu_bwd_colsum"] = 4 * N * C  # db from the masked rows upcast
    return out


def make_step(plan, norm, x, rows):
    Hx = x["Hx"].to(rows).requires_grad_(True)
    leaves = [x[k].detach().clone().requires_grad_(True) for k in ("w_src", "w_dst", "t", "bias")]
    dY = x["dY"].to(rows)

    def step():
        Hx.grad = None
        for v in leaves:
            v.grad = None
        y, _ = ops.gate_aggregate(Hx, plan, norm, "add", leaves[0], leaves[1], leaves[2],
                                  leaves[3], relu=True)
        y.backward(dY)
        return y
    return step


def layer_ab(ei, N, C, deg_norm, window_s, dev):
    plan = plan_for(ei, N)
    norm = plan.norm(deg_norm)
    nnz = plan.nnz
    g = torch.Generator().manual_seed(C)
    x = {"Hx": torch.randn(N, C, generator=g).to(BF16).to(dev),  # the same values in both
         "dY": torch.randn(N, C, generator=g).to(BF16).to(dev),
         "w_src": (torch.randn(C, generator=g) * 0.3).to(dev),
         "w_dst": (torch.randn(C, generator=g) * 0.3).to(dev),
         "t": torch.randn(1, generator=g).to(dev), "bias": (torch.randn(C, generator=g) * 0.5).to(dev)}
    s32, sbf = make_step(plan, norm, x, torch.float32), make_step(plan, norm, x, BF16)
    y32, ybf = s32().detach(), sbf().detach()
    same = bool(torch.equal(ybf.view(torch.int16), y32.to(BF16).view(torch.int16)))
    heavy = ops.gate_heavy_rows() and plan.fwd.n_heavy > 0
    b32 = launch_bytes(N, nnz, C, deg_norm is not None, 4, heavy)
    bbf = launch_bytes(N, nnz, C, deg_norm is not None, 2, heavy)
    t32, tbf = sum(b32.values()), sum(bbf.values())
    r = alternate({"A_fp32": s32, "A2_fp32": s32, "B_bf16": sbf}, window_s)
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
    return {"n_nodes": N, "nnz": nnz, "C": C, "deg_norm": deg_norm, "heavy_rows": bool(heavy),
            "n_heavy_fwd": plan.fwd.n_heavy, "n_heavy_bwd": plan.bwd.n_heavy, **r}


def model_ms(ei, N, dev, rows, convert, steps=10, warmup=3):
    from mgcn.models import GCNModel
    torch.manual_seed(0)
    m = GCNModel(1, [32] * 12, 2, residual_hop=1, dropout=0, final_type='proj', deg_norm=None,
                 edge_gate='proj', aggr='add', bias=False).to(dev)
    if convert:
        m = m.to(BF16)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(N, 1, generator=g).to(rows).to(dev)
    dY = (torch.randn(N, 2, generator=g) * 1e-3).to(rows).to(dev)

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
    return ms[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0, help="seconds of timed steps per arm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edge_gate_bf16", "ab.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_edge_gate_bf16.py needs a HIP device")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "hbm_peak_tb_per_s": HBM_PEAK_GBS / 1e3}
    ei3, N3, _ = make_botnet_graph()
    ei3 = ei3.to(dev)
    res["config3_botnet_C32_none"] = layer_ab(ei3, N3, 32, None, args.window, dev)
    res["model12_config3_ms_per_step"] = {
        "fp32": model_ms(ei3, N3, dev, torch.float32, False),
        "fp32_again": model_ms(ei3, N3, dev, torch.float32, False),
        "bf16_input_fp32_masters": model_ms(ei3, N3, dev, BF16, False),
        "bf16_converted": model_ms(ei3, N3, dev, BF16, True)}
    del ei3
    ei2, N2 = make_er_graph()
    ei2 = ei2.to(dev)
    for C in (32, 128):
        res[f"config2_C{C}_sm"] = layer_ab(ei2, N2, C, "sm", args.window, dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    for k in ("config3_botnet_C32_none", "config2_C32_sm", "config2_C128_sm"):
        a = res[k]
        print(json.dumps({"run": k, "A_ms": a["A_fp32"]["median_ms"],
                          "A2_ms": a["A2_fp32"]["median_ms"], "B_ms": a["B_bf16"]["median_ms"],
                          "B_over_A": a["ratio_B_over_A"], "byte_ratio": a["byte_ratio"],
                          "spread": a["spread_A_A2"],
                          "faster_than_spread": a["faster_than_spread"],
                          "Y_bits_equal_rounded_fp32": a["Y_bits_equal_rounded_fp32"]}),
              flush=True)
        for p in ("per_launch_fp32", "per_launch_bf16"):
            print(json.dumps({"run": f"{k}.{p}",
                              **{n: round(v["ms"], 4) for n, v in a[p].items()}}))
    print(json.dumps({"run": "model12_config3", **res["model12_config3_ms_per_step"]}))


if __name__ == "__main__":
    main()
