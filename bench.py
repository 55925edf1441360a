#!/usr/bin/env python
"""Headline benchmark: edges/sec of GCN forward+backward on the 10M-edge
synthetic graph, F = 128 (BASELINE.json `metric`, config 2).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps and prints the result line
(`value`, `ms_per_step`, ...).  `--dump-outputs DIR` then writes what the last
timed step computed (:func:`dump_outputs`).  `--full` adds everything that
takes runs of its own: the instrumented per-kernel pass (`kernels`,
`kernel_templates`, `roofline`), the CPU baseline (`cpu_baseline`) and, at
N > 1 in `--mode auto`, the second parallelisation (`replicas`).

Workload: Erdos-Renyi, N = 1,000,000 nodes,
5,000,000 random (s, d) pairs drawn with torch.Generator seed 0 (s first,
then d), symmetrised to E = 10,000,000 directed edges (duplicates and rare
self-pairs kept), N self-loops appended (data_procs/loop.py:13-17) ->
nnz = 11,000,000.  X ~ N(0,1) seed 1; W glorot seed 2; b ~ U(-0.1, 0.1)
seed 3; upstream gradient dY ~ N(0,1) seed 4.  Three GCN layers
128 -> 128 -> 128 -> 128 (NodeModelAdditive deg_norm='sm', aggr='add',
bias) with ReLU between layers.  One step = forward of all layers +
backward to every weight and bias (no optimizer step, as the metric defines).

    edges/s = E * L / t_step          (E = 10M graph edges, loops not counted)

N > 1 GPUs (torch.distributed.run, one rank per GPU, RCCL): `value` is the
edges/s of ONE config-2 graph sharded by destination-node range over the N
ranks (mgcn.dist: the north star's partitioning, chunked RCCL all-gathers of
the layer activations and upstream gradients over xGMI overlapped with the
fused layer kernels; `scaling` "strong").  With `--full` the same run also
times data-parallel replicas (every rank its own config-2 graph, one bucketed
gradient all-reduce per step) and reports them under `replicas` (`scaling`
"weak").  `--mode shard|replica` measures one of them as `value`.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, "meta-gcn_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md, chip-level parameters)
METRIC = "edges/sec GCN fwd+bwd, 10M-edge synth graph F=128, at 1/2/4/8 MI355X"


# ------------------------------------------------------------ workload
def make_er_graph(n_nodes: int = 1_000_000, n_pairs: int = 5_000_000, seed: int = 0):
    """Config-2 graph on the CPU: ([2, 2*n_pairs + n_nodes] int64, n_nodes)."""
    g = torch.Generator().manual_seed(seed)
    s = torch.randint(0, n_nodes, (n_pairs,), generator=g)
    d = torch.randint(0, n_nodes, (n_pairs,), generator=g)
    loops = torch.arange(n_nodes)
    src = torch.cat([s, d, loops])
    dst = torch.cat([d, s, loops])
    return torch.stack([src, dst]), n_nodes


def make_botnet_graph(*args, **kw):
    """Config-3 graph generator (mgcn.botnet.make_botnet_graph)."""
    from mgcn.botnet import make_botnet_graph as make
    return make(*args, **kw)


def batch_graphs(graphs):
    """PyG-style Batch collation of [(edge_index, n)]: offsets node ids."""
    eis, off = [], 0
    for ei, n in graphs:
        eis.append(ei + off)
        off += n
    return torch.cat(eis, 1), off


def make_inputs(n_nodes: int, feat: int, layers: int):
    gx = torch.Generator().manual_seed(1)
    X = torch.randn(n_nodes, feat, generator=gx)
    gw = torch.Generator().manual_seed(2)
    gb = torch.Generator().manual_seed(3)
    Ws, bs = [], []
    for _ in range(layers):
        a = (6.0 / (feat + feat)) ** 0.5
        Ws.append(torch.rand(feat, feat, generator=gw) * (2 * a) - a)
        bs.append(torch.rand(feat, generator=gb) * 0.2 - 0.1)
    gy = torch.Generator().manual_seed(4)
    dY = torch.randn(n_nodes, feat, generator=gy)
    return X, Ws, bs, dY


def spmm_bytes(n_rows: int, nnz: int, F: int) -> int:
    """Algorithmic HBM bytes of one SpMM launch (SURVEY.md §8(d) B_spmm):
    rowptr 8(N+1) + per slot (4 col + 4 weight + 4F gathered row) + 4NF out."""
    return 8 * (n_rows + 1) + nnz * (8 + 4 * F) + 4 * n_rows * F


def pmc_traffic(kernel: str, args, world: int):
    """HBM bytes per launch of `kernel` from the committed rocprofv3 PMC summary
    (profiles/<round>/pmc_fused.json or pmc_spmm.json: FETCH_SIZE and
    WRITE_SIZE in separate passes, FETCH_SIZE corrected by the factors
    calibrated on known-size launches, scripts/pmc_summary.py).  PMC needs its own profiler run, so bench.py reports the
    committed measurement of this exact kernel/config, or None."""
    if world != 1 or (args.nodes, args.pairs, args.feat) != (1_000_000, 5_000_000, 128):
        return None, None
    pdir = os.path.join(ROOT, "profiles")
    if not os.path.isdir(pdir):
        return None, None
    # the newest round's summary that holds this kernel (pmc_fused.json: the
    # fused layer kernels; pmc_spmm.json: the unfused SpMMs)
    for rnd in sorted(os.listdir(pdir), reverse=True):
        for fname in ("pmc_fused.json", "pmc_spmm.json"):
            path = os.path.join(pdir, rnd, fname)
            if not os.path.exists(path):
                continue
            with open(path) as f:
                k = json.load(f)["kernels"].get(kernel)
            if k:
                return k["traffic_bytes"], os.path.relpath(path, ROOT)
    return None, None


# ------------------------------------------------------------ CPU baseline
def cpu_baseline(ei_cpu, X, W, b, n_edges: int, reps: int = 3):
    """The reference's op sequence on the host cores: oracle.torch_layer_reference
    (matmul -> index_select -> mul(norm) -> scatter_add -> + b, autograd), one
    middle layer (input requires grad) fwd+bwd, 1 warm-up + median of `reps`."""
    from oracle import oracle as orc
    threads = len(os.sched_getaffinity(0))
    env = os.environ.get("OMP_NUM_THREADS")
    if env and env.isdigit():
        threads = min(threads, int(env))
    prev = torch.get_num_threads()
    torch.set_num_threads(threads)
    try:
        x = X.clone().requires_grad_(True)
        Wc = W.clone().requires_grad_(True)
        bc = b.clone().requires_grad_(True)
        dY = torch.randn(X.shape[0], W.shape[1], generator=torch.Generator().manual_seed(4))
        times = []
        for i in range(reps + 1):
            t0 = time.perf_counter()
            out = orc.torch_layer_reference(x, ei_cpu, Wc, bc, deg_norm="sm", aggr="add")
            out.backward(dY)
            t1 = time.perf_counter()
            x.grad = Wc.grad = bc.grad = None
            del out
            if i > 0:
                times.append(t1 - t0)
        t = statistics.median(times)
    finally:
        torch.set_num_threads(prev)
    return {"value": n_edges / t, "unit": "edges/s", "cores": threads, "kind": "port",
            "sample": f"1 GCN layer fwd+bwd of config 2 (N=1M, E=10M+1M loops, F=128) in torch "
                      f"CPU ops (oracle.torch_layer_reference), 1 warm-up + median of {reps}; "
                      f"edge-layers/s (a 3-layer step = 3x this layer's time)",
            "layer_s": t}


# ------------------------------------------------------------ kernel timers
class KernelTimer:
    """HIP events around every libmgcn launch, recorded on the launch stream
    (mgcn.ops launches on torch's current stream), with each launch's row and
    edge counts for its algorithmic bytes."""

    def __init__(self):
        self.events = {}

    def __call__(self, name, start: bool, rows=None, edges=None):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        if start:
            self.events.setdefault(name, []).append([ev, None, rows, edges])
        else:
            self.events[name][-1][1] = ev

    def summary(self):
        out = {}
        for name, recs in self.events.items():
            ms = [a.elapsed_time(b) for a, b, _, _ in recs]
            out[name] = {"launches": len(ms), "avg_ms": sum(ms) / len(ms), "total_ms": sum(ms),
                         "sizes": [(r, e) for _, _, r, e in recs]}
        return out


def launch_bytes(name: str, rows: int, edges: int, F: int):
    """(algorithmic HBM bytes, flops) of one libmgcn launch:
    the SpMM's B_spmm for every gathering kernel, plus the fused kernels'
    extra streams (Z written, X read, ReLU mask words); the dense dW / dX
    passes read and write whole [rows, F] tensors."""
    if name.startswith("spmm_xw"):
        b = spmm_bytes(rows, edges, F)
        fl = 2.0 * rows * F * F
        if name.endswith("_pk"):
            # gathered from a packed table in place (mgcn.dist, round 6): per
            # slot the row's F / 4-B header instead of its 4F B, plus its
            # nonzero words at the nominal half density of a ReLU'd table
            b -= edges * 4 * F
            b += edges * (F / 4 + 2 * F)
            name = name[:-3]
        if name == "spmm_xw_bwd":
            b += 4 * rows * F     # X rows read beside the gathered dY
            fl *= 2
        elif name == "spmm_xw_fwd_z":
            b += 4 * rows * F     # the aggregate Z written beside Y
        elif name == "spmm_xw_bwd_dx":
            b += 16 * rows        # the lower layer's ReLU mask words
        return b, fl
    if name.startswith("spmm"):
        return spmm_bytes(rows, edges, F), 0.0
    if name.startswith("residual_layer"):
        # residual.hip (F = 32 whatever the bench width): the SpMM bytes plus
        # the row's own X and its Z / dX out, and the two ReLU mask words
        Fr = 32
        return (8 * (rows + 1) + edges * (8 + 4 * Fr) + 8 * rows * Fr + 8 * rows,
                4.0 * rows * Fr * Fr)
    if name.startswith("pack_rows") or name == "unpack_rows":
        # zero-skipping exchange (mgcn.dist): a dense [rows, F] side plus the
        # packed side at the ~half density of a ReLU'd table (F / 4 B of
        # header pairs -- mask and position words -- + ~2F B of values per row)
        dense = 4 * F
        if name == "pack_rows_count":  # rows read; mask words + count written
            return rows * (dense + 4 + F / 8), 0.0
        if name == "pack_rows_values":  # rows read; position words + values written
            return rows * (dense + F / 8 + 2 * F), 0.0
        return rows * (dense + F / 4 + 2 * F), 0.0
    if name == "input_layer_fwd":  # a, x read; Z written (the 1-wide SpMM is its own launch)
        return 8 * rows + 4 * F * rows, 0.0
    if name == "input_layer_bwd":  # dZ, Z, a, x read
        return 8 * F * rows + 8 * rows, 0.0
    if name.startswith("residual_stack"):
        return None, None  # one launch runs a whole run of layers: no per-launch count
    if name == "gemm_bwd":        # dW and dX: X, dH read, dX + mask
        return (12 * F + 16) * rows, 4.0 * rows * F * F
    if name == "gemm_bwd_dw":     # dW alone: X (or Z), dH read
        return 8 * F * rows, 2.0 * rows * F * F
    if name == "gemm_bwd_dw_cs":  # dW alone + the column sums of a third [rows, F] stream
        return 12 * F * rows, 2.0 * rows * F * F
    if name == "relu_bwd_colsum":  # dZ read (+ Z read and dY written under ReLU): lower bound
        return 4 * F * rows, 0.0
    return 8 * F * rows, 2.0 * rows * F * F  # F x F transforms: read + write [rows, F]


# The HIP kernel template behind each timed launch name: one template can
# serve several launch forms (the forward with and without Z), and rocprofv3
# reports per template, so the roofline's dominant kernel is picked per
# template (launch-weighted over its forms).
TEMPLATES = {"spmm_xw_fwd": "spmm_xw_fwd_kernel", "spmm_xw_fwd_z": "spmm_xw_fwd_kernel",
             "spmm_xw_bwd": "spmm_xw_bwd_ws_kernel", "spmm_xw_bwd_dw": "spmm_xw_bwd_ws_kernel",
             "spmm_xw_bwd_dx": "spmm_xw_bwd_kernel",
             "spmm_xw_fwd_pk": "spmm_xw_wide_ws_kernel", "spmm_xw_fwd_z_pk": "spmm_xw_wide_ws_kernel",
             "spmm_xw_bwd_dx_pk": "spmm_xw_wide_ws_kernel",
             "gemm_bwd_dw_cs": "gemm_bwd_kernel", "gemm_bwd_dw": "gemm_bwd_kernel",
             "gemm_bwd": "gemm_bwd_kernel"}


def by_template(kern):
    """{template: {launches, total_ms, avg_ms, bytes (per launch), gbs, forms}}
    from the per-launch-name kernel table."""
    out = {}
    for name, k in kern.items():
        t = TEMPLATES.get(name, name)
        o = out.setdefault(t, {"launches": 0, "total_ms": 0.0, "bytes_total": 0.0, "forms": []})
        o["launches"] += k["launches"]
        o["total_ms"] += k["total_ms"]
        o["forms"].append(name)
        if k.get("bytes") is None or o["bytes_total"] is None:
            o["bytes_total"] = None
        else:
            o["bytes_total"] += k["bytes"] * k["launches"]
    for o in out.values():
        o["avg_ms"] = o["total_ms"] / o["launches"]
        b = o.pop("bytes_total")
        o["bytes"] = None if b is None else b / o["launches"]
        o["gbs"] = None if b is None else b / (o["total_ms"] * 1e-3) / 1e9
    return out


# ------------------------------------------------------------ main
def make_stack(dev, Ws, bs):
    """The config-2 model: GCNStack of GCNLayers (NodeModelAdditive 'sm' /
    'add' + bias, ReLU between layers) holding the given weights."""
    from mgcn.models import GCNLayer, GCNStack
    L = len(Ws)
    F = Ws[0].shape[0]
    layers = []
    for i in range(L):
        layer = GCNLayer(F, F, deg_norm='sm', aggr='add', bias=True,
                         non_linear='relu' if i < L - 1 else 'none').to(dev)
        nm = layer.gcn.node_models[0]
        with torch.no_grad():
            nm.weight_node.copy_(Ws[i])
            nm.bias.copy_(bs[i])
        layers.append(layer)
    return GCNStack(layers)


def build_stack(dev, ei_cpu, X, Ws, bs, dY):
    """Single-GPU config-2 model (:func:`make_stack`, the fused libmgcn path)
    on one graph; returns (step, params).  The step is fwd + bwd to every
    weight and bias against the fixed upstream gradient dY, and returns the
    top layer's output."""
    stack = make_stack(dev, Ws, bs)
    params = list(stack.parameters())
    ei = ei_cpu.to(dev)
    Xd = X.to(dev)
    dYd = dY.to(dev)

    def step():
        for p in params:
            p.grad = None
        y = stack(Xd, ei)
        y.backward(dYd)
        return y
    return step, params


def timed(run_step, steps, warmup, world, dev, timer=None, after=None):
    """Graph prep + first step (untimed, reported), W warm-up steps, then
    exactly K steps bracketed by barrier + device sync; max over ranks.
    ``after`` (--dump-outputs) is called once the clock has stopped, with what
    the last timed step returned, before anything else runs.
    The headline loop runs uninstrumented; with ``timer`` a separate pass of
    min(K, 10) steps afterwards records HIP events around every libmgcn
    launch (per-kernel averages; not part of the headline time)."""
    from mgcn import ops

    def barrier():
        if world > 1:
            import torch.distributed as dist
            dist.barrier()

    torch.cuda.synchronize()
    barrier()
    t0 = time.perf_counter()
    run_step()
    torch.cuda.synchronize()
    prep_ms = (time.perf_counter() - t0) * 1e3
    for _ in range(warmup):
        run_step()
    torch.cuda.synchronize()
    barrier()
    last = None
    t0 = time.perf_counter()
    for _ in range(steps - 1):
        run_step()
    if steps > 0:
        last = run_step()  # the last step's result is kept for --dump-outputs
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    barrier()
    elapsed = t1 - t0
    if after is not None:
        after(last)
    del last
    if timer is not None:  # instrumented pass, outside the timed region
        ops.set_kernel_timer(timer)
        for _ in range(min(steps, 10)):
            run_step()
        torch.cuda.synchronize()
        ops.set_kernel_timer(None)
        barrier()
    if world > 1:
        import torch.distributed as dist
        t = torch.tensor([elapsed, prep_ms], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed, prep_ms = float(t[0]), float(t[1])
    return elapsed, prep_ms


DUMP_BUDGET = 64 << 20   # bytes, all files of one --dump-outputs together
DUMP_SEED = 5            # row sample of an output over half the budget


def dump_outputs(path: str, y, grads) -> dict:
    """Write what the last timed step handed its caller as ``path/<name>.npy``
    (float32): ``y``, the top layer's output [rows, F] (None where the step
    returns nothing, as the sharded step does), and ``grads``, {name: the
    gradient the step left on a weight or bias}.  An output over half of
    DUMP_BUDGET is written as a fixed sample of its rows (ascending row ids
    of torch.randperm(rows) under torch.Generator seed DUMP_SEED), so two
    builds run with the same arguments write the same rows.  Returns
    {name: shape written}."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    out = {}
    if y is not None:
        y = y.detach()
        row_bytes = 4 * y[0].numel()
        keep = (DUMP_BUDGET // 2) // row_bytes
        if y.shape[0] > keep:
            g = torch.Generator().manual_seed(DUMP_SEED)
            rows = torch.randperm(y.shape[0], generator=g)[:keep].sort().values
            y = y[rows.to(y.device)]
        out["y"] = y
    for name, gr in grads.items():
        out["grad_" + name] = gr.detach()
    shapes, total = {}, 0
    for name, t in out.items():
        a = np.ascontiguousarray(t.to(torch.float32).cpu().numpy())
        total += a.nbytes
        assert total <= DUMP_BUDGET, "dump_outputs: over DUMP_BUDGET"
        np.save(os.path.join(path, name + ".npy"), a)
        shapes[name] = list(a.shape)
    return shapes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--pairs", type=int, default=5_000_000)
    ap.add_argument("--feat", type=int, default=128)
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline figure does not need: the instrumented "
                         "per-kernel pass (kernels, kernel_templates, roofline), the CPU "
                         "baseline and, at N > 1 in --mode auto, the replica measurement")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write the last step's output (a seeded row "
                         "sample) and every weight / bias gradient as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--no-kernel-timers", action="store_true",
                    help="--full without the instrumented per-kernel pass")
    ap.add_argument("--dense-exchange", action="store_true",
                    help="N > 1 sharded: send every exchanged table dense (no zero-skipping)")
    ap.add_argument("--packed-exchange", action="store_true",
                    help="N > 1 sharded: pack the ReLU'd tables at every N (default: up to 4 "
                         "ranks, mgcn.dist.set_pack_exchange('auto'))")
    ap.add_argument("--mode", choices=["auto", "replica", "shard"], default="auto",
                    help="N > 1: 'auto' measures the dst-range sharded graph (value, strong "
                         "scaling) and, with --full, data-parallel replicas (the 'replicas' "
                         "field, weak scaling); 'shard' / 'replica' measure one of them as value")
    ap.add_argument("--chunks", type=int, default=4,
                    help="N > 1 sharded path: row chunks per layer output (all-gathers "
                         "pipelined behind the compute)")
    ap.add_argument("--opt", action="append", default=[], metavar="NAME=VALUE",
                    help="mgcn_set_option before the run (A/B experiments; repeatable)")
    ap.add_argument("--dist-backend", default="nccl", help=argparse.SUPPRESS)  # gloo: tests
    ap.add_argument("--one-device", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("--gpus N > 1 must be launched with torch.distributed.run "
                             "(one process per GPU)")
    dev_index = 0 if args.one_device else local_rank
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    if world > 1:
        import torch.distributed as dist
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(args.dist_backend)

    import mgcn  # noqa: F401
    for kv in args.opt:
        k, v = kv.split("=")
        mgcn.set_option(k, int(v))

    F, L = args.feat, args.layers
    n_edges = 2 * args.pairs          # graph edges, self-loops not counted
    X, Ws, bs, dY = make_inputs(args.nodes, F, L)
    timer = KernelTimer() if args.full and not args.no_kernel_timers else None
    mode = args.mode if world > 1 else "replica"
    if mode == "auto":
        mode = "shard"
    do_shard = world > 1 and (args.mode in ("auto", "shard"))
    do_replica = world == 1 or args.mode == "replica" or (args.mode == "auto" and args.full)
    sharded = replicas = None
    dumped = None
    N = args.nodes
    ei_cpu = None
    if do_shard:
        from mgcn import dist as mdist
        from mgcn.dist import ShardedGCN
        mdist.set_pack_exchange(False if args.dense_exchange else
                                True if args.packed_exchange else "auto")
        ei_cpu, N = make_er_graph(args.nodes, args.pairs)
        model = ShardedGCN(ei_cpu, N, Ws, bs, device=dev, chunks=args.chunks)
        nnz = ei_cpu.shape[1]
        mdist.STATS.update(dense_words=0, sent_words=0)

        def dump_sharded(_):
            # the sharded step returns nothing: its caller receives the
            # all-reduced gradients
            nonlocal dumped
            grads = {f"W{i}": w.grad for i, w in enumerate(model.W)}
            grads.update({f"b{i}": b.grad for i, b in enumerate(model.b)})
            dumped = dump_outputs(args.dump_outputs, None, grads)
        dump = args.dump_outputs and mode == "shard" and rank == 0
        t_sh, prep_sh = timed(model.step_fn(X, dY), args.steps, args.warmup, world, dev,
                              timer if mode == "shard" else None,
                              dump_sharded if dump else None)
        st = dict(mdist.STATS)
        sharded = {"value": n_edges * L / (t_sh / args.steps), "unit": "edges/s",
                   "ms_per_step": t_sh / args.steps * 1e3, "scaling": "strong",
                   "parallelism": f"dst-range x{world}",
                   "path": ("fused layer kernels, chunked RCCL all-gathers (x%d per layer and "
                            "direction) overlapped with compute" % model.shard.chunks
                            if model.fused else "per-layer GEMM + SpMM, RCCL all-gathers"),
                   "workload": "config 2 (one 10M-edge graph) sharded by destination range",
                   "graph_prep_plus_first_step_ms": prep_sh,
                   "rows_per_rank": model.shard.rows,
                   # ReLU'd tables sent packed (zero-skipping): words sent / dense words
                   "packed_exchange_ratio": (st["sent_words"] / st["dense_words"]
                                             if st["dense_words"] else None)}
        del model
        torch.cuda.empty_cache()
    if do_replica:
        from mgcn.dist import allreduce_grads
        # data-parallel replicas: rank r trains its own config-2 graph (seed r)
        # with the shared weights; one bucketed gradient all-reduce per step
        ei_r, N = make_er_graph(args.nodes, args.pairs, seed=rank)
        if ei_cpu is None:
            ei_cpu = ei_r
        nnz = ei_r.shape[1]
        step, params = build_stack(dev, ei_r, X, Ws, bs, dY)

        def run_step():
            y = step()
            allreduce_grads(params)
            return y

        def dump_stack(y):
            # make_stack's parameters: W0, b0, W1, b1, ...
            nonlocal dumped
            grads = {f"{'Wb'[i % 2]}{i // 2}": p.grad for i, p in enumerate(params)}
            dumped = dump_outputs(args.dump_outputs, y, grads)
        dump = args.dump_outputs and mode == "replica" and rank == 0
        t_r, prep_r = timed(run_step, args.steps, args.warmup, world, dev,
                            timer if mode == "replica" else None,
                            dump_stack if dump else None)
        replicas = {"value": world * n_edges * L / (t_r / args.steps), "unit": "edges/s",
                    "ms_per_step": t_r / args.steps * 1e3, "scaling": "weak",
                    "parallelism": f"dp{world}" if world > 1 else "single",
                    "workload": ("config2: Erdos-Renyi N=1M, E=10M (+1M self-loops), F=128, "
                                 "3-layer GCN (sm, add, bias, ReLU) fwd+bwd" + (
                                     "; one graph per GPU (seed = rank), gradient all-reduce"
                                     if world > 1 else "")),
                    "graph_prep_plus_first_step_ms": prep_r}
    head = sharded if mode == "shard" else replicas
    value, ms_per_step = head["value"], head["ms_per_step"]
    result = {
        "metric": METRIC, "value": value, "unit": "edges/s", "n_gpus": world,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_per_step,
        "higher_is_better": True, "scaling": head["scaling"],
        "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "arithmetic": ("aggregation fp32 (bitwise = reference); dense x@W / dW / dX products as "
                       "bf16x6 (exact 3-term bf16 split of each fp32 operand, 6 MFMA products, "
                       "fp32 accumulate; error at fp32 level, tests/test_gpu_parity.py); "
                       "forward fused as (A x) W in one launch per layer, keeping Z = A x where the "
                       "backward reads it (the bottom layer); "
                       "backward: the top and middle layers' adjoints gather dY and form "
                       "dW = X^T (A^T dY) and dX in one launch (mgcn_spmm_xw_bwd, the "
                       "warp-specialised kernel); the bottom layer keeps Z = A x from its "
                       "forward and forms dW = Z^T dY in one dense pass that also streams the "
                       "top layer's dY for the top bias gradient (mgcn_gemm_bwd_dw_cs), no gather "
                       "(tests/test_gpu_fused.py, tests/test_gpu_headline.py)"),
        "config": {"workload": head["workload"], "nodes": N, "edges": n_edges, "nnz": nnz,
                   "feat": F, "layers": L, "global_batch": world if mode == "replica" else 1,
                   "parallelism": head["parallelism"]},
        "graph_prep_plus_first_step_ms": head["graph_prep_plus_first_step_ms"],
    }
    if dumped is not None:
        result["dumped_outputs"] = dumped
    if world > 1:
        if mode == "shard" and replicas is not None:
            result["replicas"] = replicas
        if mode == "replica" and sharded is not None:
            result["sharded"] = sharded
    if timer is not None:
        ks = timer.summary()
        kern = {}
        for name, s_ in ks.items():
            bytes_ = flops = 0.0
            for r, e in s_.pop("sizes"):
                b, fl = launch_bytes(name, r or 0, e or 0, F)
                if b is None:
                    bytes_ = flops = None
                    break
                bytes_ += b
                flops += fl
            t = s_["total_ms"] * 1e-3
            if bytes_ is None:
                kern[name] = dict(s_, bytes=None, gbs=None, flop=None, tflops=None)
                continue
            kern[name] = dict(s_, bytes=bytes_ / s_["launches"], gbs=bytes_ / t / 1e9,
                              flop=flops / s_["launches"], tflops=flops / t / 1e12)
        tmpl = by_template(kern)
        dom = max((t for t in tmpl if t.startswith("spmm")), key=lambda t: tmpl[t]["total_ms"])
        a = tmpl[dom]["gbs"]
        result["kernels"] = kern
        result["kernel_templates"] = tmpl
        result["kernels_note"] = ("HIP events on the launch stream around every libmgcn launch, in a "
                                  "separate instrumented pass of min(K, 10) steps after the timed "
                                  "loop (per rank: rank 0's); bytes = algorithmic bytes per launch "
                                  "(bench.launch_bytes), gbs = their sum over the summed launch "
                                  "times; heavy-row launches on the side stream are not included "
                                  "(config 2 has none)")
        # PMC traffic per launch of the template: its forms' committed
        # measurements, weighted by their launches in this step
        traffic, src, tot = 0.0, None, 0
        for form in tmpl[dom]["forms"]:
            t_, s_ = pmc_traffic(form, args, world)
            if t_ is None:
                traffic = None
                break
            traffic += t_ * kern[form]["launches"]
            tot += kern[form]["launches"]
            src = s_
        if traffic is not None and tot:
            traffic /= tot
        result["roofline"] = {"bound": "hbm", "kernel": dom, "forms": tmpl[dom]["forms"],
                              "achieved": a, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                              "frac": a / HBM_PEAK_GBS, "traffic": traffic,
                              "traffic_source": src,
                              "note": "achieved = the template's algorithmic bytes per launch "
                                      "(bench.launch_bytes, launch-weighted over its forms) / its "
                                      "average HIP-event launch time; the dominant template by "
                                      "GPU time, as rocprofv3 --stats reports kernels"}
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        result["cpu_baseline"] = cpu_baseline(ei_cpu, X, Ws[1], bs[1], n_edges)
    if rank == 0:
        print(json.dumps(result), flush=True)
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
