"""Benchmark of one NodeModelAttention layer, forward + backward (a record, not
a gate): the fused HIP attention kernels against the same step composed from
torch index_select / scatter ops on the same device.

    python scripts/bench_attention.py [--steps 20] [--warmup 3] [--out profiles/attention/bench.json]

Shape: N = 1M nodes, E = 10M random directed edges + 1M self-loops, F_in = 128,
H = 8 heads of C = 16 channels, att_dir 'in', LeakyReLU(0.2).  Prints one JSON
line: median ms/step of both, the median HIP-event time of every libmgcn
launch of a step, and the algorithmic bytes of the step (computed from the
shapes below) over its time, against 8 TB/s.
"""
import argparse
import json
import os
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "meta-gcn_amd")]
import torch  # noqa: E402

from bench import make_er_graph  # noqa: E402

HBM_PEAK = 8.0e12


def algorithmic_bytes(N, nnz, fin, H, C):
    """Bytes every launch of a step has to move (fp32 values, int32 columns,
    int64 row pointers), each operand counted once per launch that needs it."""
    HC = H * C
    rp = 8 * (N + 1)
    return {
        "gemm_nn": 4 * (N * fin + fin * HC + N * HC),                     # Hp = x W
        "att_scores": 4 * (N * HC + 2 * H * C + 2 * N * H),
        "att_fwd": rp + nnz * (4 + 4 * HC + 4 * H + 4 * H) + 4 * N * HC + 4 * N * H,
        "att_bwd_dst": rp + nnz * (4 + 4 * HC + 3 * 4 * H) + 4 * N * HC + 2 * 4 * N * H,
        "att_bwd_src": rp + nnz * (8 + 4 * HC + 2 * 4 * H) + 4 * N * HC + 2 * 4 * N * H,
        "gemm_tn": 4 * (N * 2 * H + N * HC + 2 * H * HC),                 # da
        "gemm_bwd": 4 * (2 * N * HC + 2 * N * fin + 2 * fin * HC),        # dW, dx
    }


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


def median_step(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
           for _ in range(steps)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in evs)
    return ms[len(ms) // 2], ms[0], ms[-1]


def torch_layer(x, W, att, src, dst, N, H, C):
    """The reference's forward (graph_attention.py:64-100) in torch ops."""
    hp = (x @ W).view(N, H, C)
    xj, xi = hp.index_select(0, src), hp.index_select(0, dst)
    e = torch.nn.functional.leaky_relu((torch.cat([xj, xi], dim=-1) * att).sum(-1), 0.2)
    ix = dst.view(-1, 1).expand(-1, H)
    m = torch.full((N, H), -1e16, device=x.device).scatter_reduce(0, ix, e.detach(), "amax")
    p = (e - m.index_select(0, dst)).exp()
    s = torch.zeros(N, H, device=x.device).scatter_add(0, ix, p)
    alpha = p / (s.index_select(0, dst) + 1e-16)
    msg = xj * alpha.unsqueeze(-1)
    y = torch.zeros(N, H, C, device=x.device).scatter_add(
        0, dst.view(-1, 1, 1).expand(-1, H, C), msg)
    return y.view(N, H * C)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--pairs", type=int, default=5_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention", "bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_attention.py needs a HIP device")
    from mgcn import ops
    from mgcn.models import NodeModelAttention
    dev = torch.device("cuda:0")
    fin, H, C = 128, 8, 16
    ei, N = make_er_graph(args.nodes, args.pairs)
    ei = ei.to(dev)
    nnz = int(ei.size(1))
    torch.manual_seed(0)
    nm = NodeModelAttention(fin, H * C, nheads=H, att_act='lrelu', att_dir='in').to(dev)
    x = torch.randn(N, fin, device=dev).requires_grad_(True)
    dY = torch.randn(N, H * C, device=dev)

    def step():
        x.grad = None
        nm.zero_grad(set_to_none=True)
        nm(x, ei).backward(dY)

    ms, lo, hi = median_step(step, args.warmup, args.steps)
    y_fused = nm(x, ei).detach()
    timer = EventTimer()
    ops.set_kernel_timer(timer)
    for _ in range(args.steps):
        step()
    ops.set_kernel_timer(None)
    torch.cuda.synchronize()
    kernels = timer.medians(args.steps)

    src, dst = ei[0].contiguous(), ei[1].contiguous()

    def torch_step():
        x.grad = None
        nm.zero_grad(set_to_none=True)
        torch_layer(x, nm.weight, nm.att_weight, src, dst, N, H, C).backward(dY)

    t_ms, t_lo, t_hi = median_step(torch_step, 1, max(5, args.steps // 4))
    with torch.no_grad():
        y_torch = torch_layer(x, nm.weight, nm.att_weight, src, dst, N, H, C)
    diff = (y_fused - y_torch).abs().max().item() / y_torch.abs().max().item()

    by = algorithmic_bytes(N, nnz, fin, H, C)
    total = sum(by.values())
    out = {
        "shape": {"nodes": N, "edges": nnz, "F_in": fin, "heads": H, "channels": C,
                  "att_dir": "in", "att_act": "lrelu"},
        "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": ms, "ms_min": lo, "ms_max": hi,
        "kernel_ms": kernels, "kernel_ms_sum": sum(kernels.values()),
        "algorithmic_bytes": by, "algorithmic_bytes_total": total,
        "achieved_TBps": total / (ms * 1e-3) / 1e12,
        "share_of_8TBps": total / (ms * 1e-3) / HBM_PEAK,
        "kernel_TBps": {k: by[k] / (v * 1e-3) / 1e12 for k, v in kernels.items() if k in by},
        "torch_ms_per_step": t_ms, "torch_ms_min": t_lo, "torch_ms_max": t_hi,
        "speedup_over_torch": t_ms / ms,
        "max_rel_diff_vs_torch": diff,
    }
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
