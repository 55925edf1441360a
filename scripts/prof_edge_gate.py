"""One gated layer after its ``x @ W`` (config-3 botnet graph, C = 32, deg_norm
None, 'proj'), forward + backward, 25 times with the heavy-row route on: the
program of a kernel trace, in a run of its own --

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o gate -- \
        python scripts/prof_edge_gate.py

(`profiles/edge_gate_heavy/kernel_trace.txt`: calls, average us, total ms and
name of the busiest kernels of that run's ``gate_kernel_stats.csv``)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "meta-gcn_amd"), os.path.join(ROOT, "scripts")]
import torch  # noqa: E402

import mgcn  # noqa: E402,F401
from mgcn import ops  # noqa: E402
from mgcn.graph import plan_for  # noqa: E402
from bench import make_botnet_graph  # noqa: E402

dev = torch.device("cuda:0")
ei, N, _ = make_botnet_graph()
ei = ei.to(dev)
plan = plan_for(ei, N)
norm = plan.norm(None)
g = torch.Generator().manual_seed(1)
C = 32
Hx = torch.randn(N, C, generator=g).to(dev).requires_grad_(True)
wsd = ((torch.rand(C, 2, generator=g) - 0.5) * 0.2).to(dev).requires_grad_(True)
beta = torch.zeros(1, device=dev, requires_grad=True)
dY = torch.randn(N, C, generator=g).to(dev)
for _ in range(25):
    for t in (Hx, wsd, beta):
        t.grad = None
    y, _ = ops.gate_aggregate(Hx, plan, norm, "add", wsd[:, 0], wsd[:, 1], beta)
    y.backward(dY)
torch.cuda.synchronize()
print("done", plan.fwd.n_heavy, plan.fwd.n_giant, plan.bwd.n_heavy, plan.bwd.n_giant)
