"""Where the persistent F = 128 kernels spend their last microseconds: when
every workgroup of the config-2 forward (spmm_xw_fwd_kernel) and dW + dX
adjoint (spmm_xw_bwd_ws_kernel) starts and ends.

Needs the experiment build (`make -C meta-gcn_amd/csrc exp`, loaded through
MGCN_LIB), whose two kernels stamp wall_clock64() (100 MHz) per workgroup.
Writes <out>/tail_before.json (every chunk assigned statically, chunk c to
workgroup c mod grid: mgcn_set_option "xw_dyn_rounds" 0) and tail_after.json
(the default: the forward's last rounds claimed from a counter; the adjoint
is static in both): per kernel and sample the kernel's span, the distribution
of exit times, the share of the span after the median workgroup's exit, and
the correlation of exit time with the workgroup's slot count and its XCD
(blockIdx.x % 8).

    python scripts/prof_tail.py [--samples 5] [--out profiles/balance]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "meta-gcn_amd")]
os.environ.setdefault("MGCN_LIB", os.path.join(ROOT, "meta-gcn_amd", "mgcn", "libmgcn_exp.so"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench import make_er_graph  # noqa: E402
from mgcn import _lib as L  # noqa: E402
from mgcn import ops  # noqa: E402
from mgcn.graph import plan_for  # noqa: E402

TICK_US = 0.01  # wall_clock64: 100 MHz
F, R = 128, 32


def wg_slots(rowptr, n_rows, grid):
    """Slots and chunks of every workgroup under the static assignment."""
    nch = (n_rows + R - 1) // R
    edge = rowptr[np.minimum(np.arange(nch + 1, dtype=np.int64) * R, n_rows)]
    g = min(grid, nch)
    slots = np.bincount(np.arange(nch) % g, weights=np.diff(edge), minlength=g)
    chunks = np.bincount(np.arange(nch) % g, minlength=g)
    return slots, chunks


def summarize(t, slots, chunks, static):
    g = len(slots)
    entry, exit_, n_my = (t[:g, k].astype(np.int64) for k in range(3))
    assert (entry > 0).all() and (exit_ >= entry).all(), "a workgroup left no stamps"
    assert n_my.sum() == chunks.sum(), "chunks run != chunks of the view"
    assert (n_my == chunks).all() == static, "the kernel ran another chunk assignment"
    t0 = entry.min()
    ex = (exit_ - t0) * TICK_US
    span = float(ex.max())
    xcd = np.arange(g) % 8
    q = np.percentile(ex, [0, 10, 50, 90, 99, 100])
    return {
        "workgroups": g,
        "span_us": span,
        "entry_spread_us": float((entry.max() - t0) * TICK_US),
        "exit_us": dict(zip(["min", "p10", "median", "p90", "p99", "max"], q.round(2).tolist())),
        "tail_after_median_share": float((span - q[2]) / span),
        "tail_after_p10_share": float((span - q[1]) / span),
        "slots": {"mean": float(slots.mean()), "max_over_mean": float(slots.max() / slots.mean())},
        "chunks_run": {"min": int(n_my.min()), "max": int(n_my.max())},
        "corr_exit_chunks_run": float(np.corrcoef(ex, n_my)[0, 1]) if n_my.std() > 0 else None,
        "corr_exit_slots": float(np.corrcoef(ex, slots)[0, 1]) if slots.std() > 0 else None,
        "xcd_mean_exit_us": [float(ex[xcd == x].mean()) for x in range(8)],
        "corr_exit_xcd_mean": float(np.corrcoef(ex, np.array(
            [ex[xcd == x].mean() for x in range(8)])[xcd])[0, 1]),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "balance"))
    args = ap.parse_args()
    lib = L.load()
    tail = lib.mgcn_debug_xw_tail
    tail.argtypes = [ctypes.c_void_p]
    dev = torch.device("cuda:0")
    ei, n = make_er_graph()
    plan = plan_for(ei.to(dev), n)
    norm = plan.norm("sm")
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.randn(n, F, device=dev, generator=g)
    W = torch.randn(F, F, device=dev, generator=g) * 0.1
    b = torch.zeros(F, device=dev)
    dY = torch.randn(n, F, device=dev, generator=g)
    rm = ops.make_relu_mask(torch.randn(n, F, device=dev, generator=g))
    mask_out = torch.empty(n, 4, dtype=torch.int32, device=dev)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    grids = {"fwd": 2 * cus, "dws": cus}  # workgroups per CU: 2 and 1
    views = {"fwd": plan.fwd, "dws": plan.bwd}

    def launch(kernel):
        if kernel == "fwd":
            ops.spmm_xw_fwd(plan.fwd, norm.w_fwd, X, W, L.REDUCE_SUM, b, True, relu_mask=mask_out)
        else:
            ops.spmm_xw_bwd(plan.bwd, norm.w_bwd, norm.row_scale_bwd, dY, X, W, relu_mask=rm)

    os.makedirs(args.out, exist_ok=True)
    for fname, rounds in (("tail_before.json", 0), ("tail_after.json", 8)):
        L.set_option("xw_dyn_rounds", rounds)
        doc = {"assignment": f"forward: last {rounds} rounds claimed" if rounds else "static",
               "graph": {"n": n, "nnz": plan.fwd.nnz}, "tick_us": TICK_US}
        for kernel, idx in (("fwd", 0), ("dws", 1)):
            view, grid = views[kernel], grids[kernel]
            slots, chunks = wg_slots(view.rowptr.cpu().numpy(), view.n_rows, grid)
            for _ in range(2):
                launch(kernel)
            samples = []
            for _ in range(args.samples):
                L.check(tail(None), "mgcn_debug_xw_tail")  # clear
                launch(kernel)
                buf = np.zeros((2, 1024, 4), dtype=np.uint64)
                L.check(tail(buf.ctypes.data), "mgcn_debug_xw_tail")
                samples.append(summarize(buf[idx], slots, chunks,
                                         static=kernel == "dws" or rounds == 0))
            shares = [s["tail_after_median_share"] for s in samples]
            doc[kernel] = {"samples": samples,
                           "tail_after_median_share_median": float(np.median(shares)),
                           "span_us_median": float(np.median([s["span_us"] for s in samples]))}
            print(json.dumps({"assignment": doc["assignment"], "kernel": kernel,
                              "span_us": doc[kernel]["span_us_median"],
                              "tail_after_median_share": doc[kernel]["tail_after_median_share_median"],
                              "corr_exit_slots": samples[-1]["corr_exit_slots"],
                              "slots_max_over_mean": samples[-1]["slots"]["max_over_mean"]}),
                  flush=True)
        with open(os.path.join(args.out, fname), "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
