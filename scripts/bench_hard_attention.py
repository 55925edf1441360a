"""Benchmark of one NodeModelHardAttention layer (a record, not a gate), at
the shape of scripts/bench_attention.py:

    python scripts/bench_hard_attention.py [--steps 20] [--warmup 3]
                                           [--out profiles/hard_attention/bench.json]

N = 1M nodes, E = 10M random directed edges + 1M self-loops, F_in = 128, H = 8
heads of C = 16 channels, att_dir 'in', LeakyReLU(0.2), T = 0.1.  Prints one
JSON line and writes it to --out:

 (a) training: median ms/step (forward + backward) of NodeModelHardAttention
     beside the soft NodeModelAttention step, same graph, same box, and the
     median HIP-event time of every libmgcn launch of the hard step.  The
     Gumbel noise is drawn once outside the timed region and replayed (the
     module draws it with torch ops; a fused generator is out of scope).
 (b) eval: the median ms of the forward, and of its gather alone through
     mgcn_hatt_gather (loads the rows of the slots with a non-zero
     coefficient) beside the same one-hot alpha through mgcn_att_fwd's
     aggregate-only mode (loads every neighbour's row), with a bitwise
     comparison of the two results.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "meta-gcn_amd"), os.path.join(ROOT, "scripts")]
import torch  # noqa: E402

from bench import make_er_graph  # noqa: E402
from bench_attention import EventTimer, median_step  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--pairs", type=int, default=5_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hard_attention",
                                                  "bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_hard_attention.py needs a HIP device")
    import mgcn
    import mgcn.models as M
    from mgcn import _lib as L
    from mgcn import ops
    from mgcn.graph import plan_for
    dev = torch.device("cuda:0")
    fin, H, C, T = 128, 8, 16, 0.1
    HC = H * C
    ei, N = make_er_graph(args.nodes, args.pairs)
    ei = ei.to(dev)
    nnz = int(ei.size(1))
    torch.manual_seed(0)
    hard = M.NodeModelHardAttention(fin, HC, nheads=H, att_act='lrelu', att_dir='in',
                                    temperature=T).to(dev)
    soft = M.NodeModelAttention(fin, HC, nheads=H, att_act='lrelu', att_dir='in').to(dev)
    soft.load_state_dict(hard.state_dict())
    x = torch.randn(N, fin, device=dev).requires_grad_(True)
    dY = torch.randn(N, HC, device=dev)
    noise = M.gumbel_samples(torch.empty(nnz, H, device=dev))
    draw = M.gumbel_samples
    M.gumbel_samples = lambda base: noise

    def step(nm):
        def run():
            x.grad = None
            nm.zero_grad(set_to_none=True)
            nm(x, ei).backward(dY)
        return run

    hard.train(), soft.train()
    h_ms, h_lo, h_hi = median_step(step(hard), args.warmup, args.steps)
    s_ms, s_lo, s_hi = median_step(step(soft), args.warmup, args.steps)
    timer = EventTimer()
    ops.set_kernel_timer(timer)
    for _ in range(args.steps):
        step(hard)()
    ops.set_kernel_timer(None)
    torch.cuda.synchronize()
    train_kernels = timer.medians(args.steps)

    # (b) eval
    hard.eval()
    store = []

    def eval_fwd():
        with torch.no_grad():
            hard(x, ei, attn_store=store)
        del store[1:]

    e_ms, e_lo, e_hi = median_step(eval_fwd, args.warmup, args.steps)
    timer = EventTimer()
    ops.set_kernel_timer(timer)
    for _ in range(args.steps):
        eval_fwd()
    ops.set_kernel_timer(None)
    torch.cuda.synchronize()
    eval_kernels = timer.medians(args.steps)

    lib = mgcn.load()
    plan = plan_for(ei, N)
    fwd = plan.fwd
    alpha = store[0][fwd.eid.long()].contiguous()  # the one-hot, fwd slot order
    with torch.no_grad():
        Hp = ops.linear(x.detach(), hard.weight.detach())
    Y_skip = torch.empty(N, HC, device=dev)
    Y_dense = torch.empty(N, HC, device=dev)
    st = L.stream_of(dev)

    def gather():
        L.check(lib.mgcn_hatt_gather(N, nnz, H, C, L.ptr(fwd.rowptr), L.ptr(fwd.col), L.ptr(alpha),
                                     L.ptr(Hp), HC, L.ptr(Y_skip), HC, st), "mgcn_hatt_gather")

    def dense():
        L.check(lib.mgcn_att_fwd(N, nnz, H, C, L.ptr(fwd.rowptr), L.ptr(fwd.col), None, None, 0,
                                 L.ptr(alpha), None, L.ptr(Hp), HC, L.ptr(Y_dense), HC, None, st),
                "mgcn_att_fwd")

    g_ms, g_lo, g_hi = median_step(gather, args.warmup, args.steps)
    d_ms, d_lo, d_hi = median_step(dense, args.warmup, args.steps)
    M.gumbel_samples = draw
    selected = int((alpha != 0).any(dim=1).sum().item())

    out = {
        "shape": {"nodes": N, "edges": nnz, "F_in": fin, "heads": H, "channels": C,
                  "att_dir": "in", "att_act": "lrelu", "temperature": T},
        "steps": args.steps, "warmup": args.warmup,
        "train": {
            "hard_ms_per_step": h_ms, "hard_ms_min": h_lo, "hard_ms_max": h_hi,
            "soft_ms_per_step": s_ms, "soft_ms_min": s_lo, "soft_ms_max": s_hi,
            "hard_over_soft": h_ms / s_ms,
            "kernel_ms": train_kernels, "kernel_ms_sum": sum(train_kernels.values()),
        },
        "eval": {
            "forward_ms": e_ms, "forward_ms_min": e_lo, "forward_ms_max": e_hi,
            "kernel_ms": eval_kernels,
            "hatt_gather_ms": g_ms, "hatt_gather_ms_min": g_lo, "hatt_gather_ms_max": g_hi,
            "att_fwd_aggregate_only_ms": d_ms, "att_fwd_aggregate_only_ms_min": d_lo,
            "att_fwd_aggregate_only_ms_max": d_hi,
            "dense_over_gather": d_ms / g_ms,
            "slots_with_a_winner": selected, "share_of_slots": selected / nnz,
            "bitwise_equal": bool(torch.equal(Y_skip, Y_dense)),
        },
    }
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
