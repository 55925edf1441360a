"""A/B of the attention modules' ``edge_rng``: the Gumbel noise and the dropout
mask drawn by torch (as shipped: the noise on the CPU) against the seeded
on-device generator (mgcn_edge_noise).  A record, not a gate.

    python scripts/bench_edge_noise.py [--window 1.0] [--out profiles/edge_noise/ab.json]

The training step (forward + backward) of one node model, the draw inside the
timed region in every arm:

* ``NodeModelHardAttention`` (lrelu, 'in', T = 0.1, no dropout)
    a   edge_rng='torch' as shipped: ``gumbel_samples`` draws E H floats on the
        CPU, copies them to the device, six elementwise passes, and the op
        permutes the result to slot order
    b   the same with ``gumbel_samples`` drawing on the device (torch.rand on
        the GPU): what is left is the passes and the permutation
    b2  b again: its distance from b is the run's own spread
    c   edge_rng='device': one mgcn_edge_noise launch in slot order
* ``NodeModelAttention`` (lrelu, 'in', att_dropout = 0.5)
    a   edge_rng='torch' as shipped: F.dropout(ones [E, H]) on the device and
        the op's permutation (this arm has no CPU draw, so it is arm b as well)
    a2  a again (the spread)
    c   edge_rng='device'

on the attention shape of DESIGN.md section 4 (N = 1M, E = 11M, F_in = 128,
H = 8, C = 16) and on the config-3 botnet graph at F_in = 32, H = 4, C = 8.
Protocol of scripts/bench_spmm_bf16.py: the arms alternate in blocks within
one process after a warm-up, each with at least ``--window`` seconds of timed
steps; ``spread`` is the distance of the repeated arm from its first run.
``launch_ms_c`` / ``launch_ms_b`` hold the median HIP-event time of every
libmgcn launch of arm c's step and of the torch arm on the device (b; soft: a);
``edge_noise`` gives that launch's algorithmic bytes
(4 nnz of eid read + 4 nnz H written) over its time, as a share of 8 TB/s.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "meta-gcn_amd"), os.path.join(ROOT, "scripts")]

import torch  # noqa: E402

import mgcn  # noqa: E402,F401
import mgcn.models as M  # noqa: E402
from mgcn import ops  # noqa: E402
from mgcn.graph import plan_for  # noqa: E402
from bench import make_botnet_graph, make_er_graph  # noqa: E402
from bench_spmm_bf16 import alternate  # noqa: E402

HBM_PEAK_TBS = 8.0
SHIPPED_DRAW = M.gumbel_samples


def device_draw(base):
    """``gumbel_samples`` with the uniform draw on ``base``'s device."""
    noise = torch.rand(base.size(), dtype=base.dtype, device=base.device)
    eps = 1e-20
    noise.add_(eps).log_().neg_()
    noise.add_(eps).log_().neg_()
    return noise


def launch_ms(step, steps=20):
    """Median HIP-event ms of every libmgcn launch of ``step``, by timer name
    (a name launched several times a step: the median of the step's sum)."""
    evs, open_ = [], {}

    def timer(name, start, rows=None, edges=None):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        if start:
            open_[name] = e
        else:
            evs[-1].setdefault(name, []).append((open_.pop(name), e))
    ops.set_kernel_timer(timer)
    try:
        for _ in range(steps):
            evs.append({})
            step()
    finally:
        ops.set_kernel_timer(None)
    torch.cuda.synchronize()
    out = {}
    for name in evs[0]:
        ms = sorted(sum(a.elapsed_time(b) for a, b in s.get(name, [])) for s in evs)
        out[name] = ms[len(ms) // 2]
    return out


def module_ab(kind, ei, N, fin, H, C, window_s, dev):
    nnz = int(ei.size(1))
    plan_for(ei, N)  # the plan is built (and cached) outside every arm
    torch.manual_seed(0)
    if kind == "hard":
        kw = dict(nheads=H, att_act='lrelu', att_dir='in', temperature=0.1)
        cls = M.NodeModelHardAttention
    else:
        kw = dict(nheads=H, att_act='lrelu', att_dir='in', att_dropout=0.5)
        cls = M.NodeModelAttention
    shipped = cls(fin, H * C, **kw).to(dev).train()
    fused = cls(fin, H * C, edge_rng='device', **kw).to(dev).train()
    fused.load_state_dict(shipped.state_dict())
    g = torch.Generator().manual_seed(1)
    x = torch.randn(N, fin, generator=g).to(dev).requires_grad_(True)
    dY = torch.randn(N, H * C, generator=g).to(dev)

    def step(nm, draw):
        def run():
            M.gumbel_samples = draw
            x.grad = None
            nm.zero_grad(set_to_none=True)
            nm(x, ei).backward(dY)
            M.gumbel_samples = SHIPPED_DRAW
        return run

    c = step(fused, SHIPPED_DRAW)
    if kind == "hard":
        arms = {"a_torch_cpu_draw": step(shipped, SHIPPED_DRAW),
                "b_torch_device_draw": step(shipped, device_draw),
                "b2_torch_device_draw": step(shipped, device_draw), "c_device": c}
        base, again = "b_torch_device_draw", "b2_torch_device_draw"
    else:
        arms = {"a_torch": step(shipped, SHIPPED_DRAW), "a2_torch": step(shipped, SHIPPED_DRAW),
                "c_device": c}
        base, again = "a_torch", "a2_torch"
    r = alternate(arms, window_s)
    ms = {k: r[k]["median_ms"] for k in arms}
    r["spread"] = abs(ms[base] - ms[again]) / ms[base]
    r["spread_of"] = [base, again]
    first = next(iter(arms))
    r["ratio_c_over_a"] = ms["c_device"] / ms[first]
    r["ratio_c_over_b"] = ms["c_device"] / ms[base]
    r["c_faster_than_b_beyond_spread"] = bool((ms[base] - ms["c_device"]) / ms[base] > r["spread"])
    r["launch_ms_c"] = launch_ms(c)
    r["launch_ms_b"] = launch_ms(arms[base])
    t = r["launch_ms_c"]["edge_noise"]
    by = 4 * nnz + 4 * nnz * H
    r["edge_noise"] = {"kind": "gumbel" if kind == "hard" else "dropout", "launch_ms": t,
                       "algorithmic_bytes": by, "tb_per_s": by / t / 1e9,
                       "share_of_8_tb_per_s": by / t / 1e9 / HBM_PEAK_TBS}
    r.update({"module": cls.__name__, "n_nodes": N, "nnz": nnz, "F_in": fin, "H": H, "C": C})
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0, help="seconds of timed steps per arm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edge_noise", "ab.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_edge_noise.py needs a HIP device")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "window_s": args.window}

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    for name, make, fin, H, C in (("config3_botnet_H4_C8", lambda: make_botnet_graph()[:2], 32, 4, 8),
                                  ("attention_shape_H8_C16", make_er_graph, 128, 8, 16)):
        ei, N = make()
        ei = ei.to(dev)
        for kind in ("hard", "soft"):
            k = f"{name}_{kind}"
            res[k] = module_ab(kind, ei, N, fin, H, C, args.window, dev)
            r = res[k]
            print(json.dumps({"run": k, **{a: v["median_ms"] for a, v in r.items()
                                           if isinstance(v, dict) and "median_ms" in v},
                              "spread": r["spread"], "c_over_a": r["ratio_c_over_a"],
                              "c_over_b": r["ratio_c_over_b"],
                              "c_faster_than_b_beyond_spread": r["c_faster_than_b_beyond_spread"],
                              "edge_noise": r["edge_noise"]}), flush=True)
            flush()
        del ei
        mgcn.clear_cache()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
