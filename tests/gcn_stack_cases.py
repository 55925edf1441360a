"""The case table behind tests/golden/gcn_stack_launches.json: small GCN stacks
that between them take every forward form and backward route of
``mgcn.ops._GCNStack``, and the helpers that run one (on a device, recording
its libmgcn launches) or plan one (on the host, from stub views).

The golden file holds, per case, the launch names of one forward + backward
(recorded from the commit before the routing moved into ``_plan_stack``; a
later change of a route on purpose re-records them) and the planner's routes
for the same case; per graph, the heavy-row counts of both views.
"""
import contextlib
import dataclasses
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "gcn_stack_launches.json")
N, E, HUB = 600, 6000, 300  # HUB > graph.HEAVY_THRESHOLD: one heavy row in one view
GRAPHS = ("light", "heavy_adjoint", "heavy_forward")
SWITCHES = {"_FUSE_XW": True, "_Z_MIDDLE": False, "_TOP_FULL": True, "_TOP_HCS": False,
            "_TOP_CS_DEFER": True, "_MAX_FULL": True}
RRN = ("relu", "relu", "none")


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    acts: tuple = RRN
    aggr: str = "add"
    F: int = 128
    bias: bool = True
    x_grad: bool = True
    frozen: tuple = ()       # layers whose weight wants no gradient
    graph: str = "light"
    switch: tuple = ()       # (name, value): the one switch off its default

    @property
    def default_switches(self):
        return not self.switch

    @property
    def all_grads(self):
        return self.x_grad and not self.frozen


def _cases():
    c = [
        # depth and activation patterns
        Case("d1_none", ("none",)),
        Case("d1_relu", ("relu",)),
        Case("d1_none_nox", ("none",), x_grad=False),
        Case("d2_relu_none", ("relu", "none")),
        Case("d2_relu_relu", ("relu", "relu")),
        Case("d3_add"),
        Case("d3_none_relu_none", ("none", "relu", "none")),
        Case("d3_all_relu", ("relu", "relu", "relu")),
        # aggregation
        Case("d3_mean", aggr="mean"),
        Case("d3_max", aggr="max"),
        Case("d1_max", ("none",), aggr="max"),
        Case("d3_all_relu_mean", ("relu", "relu", "relu"), aggr="mean"),
        Case("d3_none_relu_none_max", ("none", "relu", "none"), aggr="max"),
        # bias, x without gradient
        Case("d3_add_nobias", bias=False),
        Case("d3_mean_nobias", aggr="mean", bias=False),
        Case("d3_add_nox", x_grad=False),
        Case("d3_mean_nox", aggr="mean", x_grad=False),
        Case("d3_max_nox", aggr="max", x_grad=False),
        # frozen weights
        Case("d3_add_frozen_bottom", frozen=(0,)),
        Case("d3_add_frozen_bottom_nox", frozen=(0,), x_grad=False),
        Case("d3_add_frozen_middle", frozen=(1,)),
        Case("d3_add_frozen_all", frozen=(0, 1, 2)),
        Case("d3_max_frozen_middle", aggr="max", frozen=(1,)),
        Case("d3_none_relu_none_frozen_middle", ("none", "relu", "none"), frozen=(1,)),
        # heavy rows in one view
        Case("d3_add_heavy_adjoint", graph="heavy_adjoint"),
        Case("d3_mean_heavy_adjoint", aggr="mean", graph="heavy_adjoint"),
        Case("d3_max_heavy_adjoint", aggr="max", graph="heavy_adjoint"),
        Case("d3_add_heavy_adjoint_nox", graph="heavy_adjoint", x_grad=False),
        Case("d3_add_heavy_forward", graph="heavy_forward"),
        Case("d3_max_heavy_forward", aggr="max", graph="heavy_forward"),
        # widths
        Case("d3_add_256", F=256),
        Case("d3_mean_256", aggr="mean", F=256),
        Case("d3_add_256_frozen_middle", F=256, frozen=(1,)),
        Case("d3_max_256", aggr="max", F=256),
        Case("d3_add_64", F=64),
        Case("d3_add_64_nox", F=64, x_grad=False),
    ]
    # each switch off its default, alone
    for name, default in SWITCHES.items():
        tag = name.strip("_").lower() + ("0" if default else "1")
        for aggr in ("add", "mean") + (("max",) if name == "_MAX_FULL" else ()):
            c.append(Case(f"d3_{aggr}_{tag}", aggr=aggr, switch=(name, not default)))
    assert len({x.name for x in c}) == len(c)
    return c


CASES = _cases()


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


@contextlib.contextmanager
def switches(ops, case):
    """``ops``' six route switches at their defaults, but for the case's one."""
    saved = {k: getattr(ops, k) for k in SWITCHES}
    try:
        for k, v in {**SWITCHES, **dict([case.switch] if case.switch else [])}.items():
            setattr(ops, k, v)
        yield
    finally:
        for k, v in saved.items():
            setattr(ops, k, v)


def edge_index(kind):
    """[2, nnz] int64 (src, dst): E random edges and the self loops; HUB more
    out-edges of node 1 (a heavy row of the adjoint's view) or in-edges of
    node 0 (of the forward's)."""
    rng = np.random.default_rng(GRAPHS.index(kind))
    s, d = rng.integers(0, N, E), rng.integers(0, N, E)
    if kind == "heavy_adjoint":
        s = np.concatenate([s, np.ones(HUB, np.int64)])
        d = np.concatenate([d, rng.integers(0, N, HUB)])
    elif kind == "heavy_forward":
        s = np.concatenate([s, rng.integers(0, N, HUB)])
        d = np.concatenate([d, np.zeros(HUB, np.int64)])
    loops = np.arange(N)
    return np.stack([np.concatenate([s, loops]), np.concatenate([d, loops])]).astype(np.int64)


def tensors(case, dev):
    """(x, Ws, bs, dZ) of a case: seeded, leaves on ``dev`` with the case's
    requires_grad pattern."""
    g = torch.Generator().manual_seed(len(case.acts) * 1000 + case.F)
    F = case.F
    x = torch.randn(N, F, generator=g).to(dev).requires_grad_(case.x_grad)
    Ws, bs = [], []
    for i in range(len(case.acts)):
        Ws.append((torch.randn(F, F, generator=g) * F ** -0.5).to(dev)
                  .requires_grad_(i not in case.frozen))
        bs.append((torch.randn(F, generator=g) * 0.1).to(dev).requires_grad_(True)
                  if case.bias else None)
    return x, Ws, bs, torch.randn(N, F, generator=g).to(dev)


def run_case(case, ops, plan, norm, dev):
    """One forward + backward of the case through ``ops.gcn_stack``:
    (launch names in order, {name: tensor} of y and every gradient)."""
    x, Ws, bs, dZ = tensors(case, dev)
    names = []
    with switches(ops, case):
        ops.set_kernel_timer(lambda name, start, *a: names.append(name) if start else None)
        try:
            y = ops.gcn_stack(x, plan, norm, Ws, bs, [a == "relu" for a in case.acts], case.aggr)
            y.backward(dZ)
        finally:
            ops.set_kernel_timer(None)
    out = {"y": y.detach(), "dx": x.grad}
    for i, (W, b) in enumerate(zip(Ws, bs)):
        out[f"dW{i}"] = W.grad
        out[f"db{i}"] = None if b is None else b.grad
    return names, {k: v for k, v in out.items() if v is not None}


def stub_views(n_heavy_fwd, n_heavy_bwd):
    """Host-only CSRViews with what the planner reads: n_rows, n_cols, n_heavy."""
    from mgcn.graph import CSRView
    i64, i32 = torch.empty(0, dtype=torch.int64), torch.empty(0, dtype=torch.int32)
    return tuple(CSRView(rowptr=i64, col=i32, eid=i32, n_rows=N, n_cols=N, n_heavy=h)
                 for h in (n_heavy_fwd, n_heavy_bwd))


def plan_case(case, ops, fwd, bwd):
    """``ops._plan_stack`` of the case (x contiguous) under its switches."""
    from mgcn import _lib as L
    n = len(case.acts)
    with switches(ops, case):
        return ops._plan_stack([(case.F, case.F)] * n, tuple(a == "relu" for a in case.acts),
                               [case.bias] * n, [i not in case.frozen for i in range(n)],
                               case.x_grad, L.REDUCE_CODES[case.aggr], fwd, bwd, case.F)


def routes(stack_plan):
    """A stack plan as the golden file stores it."""
    layers = []
    for lp in stack_plan.layers:
        d = dataclasses.asdict(lp)
        d["bwd"] = lp.bwd.value
        layers.append(d)
    return {"top_bias": stack_plan.top_bias.value, "layers": layers}


def record(path=GOLDEN):
    """Re-record the golden file from this tree, on a device (after a route
    changed on purpose): ``python tests/gcn_stack_cases.py``."""
    import mgcn
    from mgcn import ops
    from mgcn.graph import plan_for
    dev = torch.device("cuda:0")
    mgcn.load()
    gold = {"graphs": {}, "cases": {}}
    plans = {}
    for kind in GRAPHS:
        plan = plan_for(torch.from_numpy(edge_index(kind)).to(dev), N)
        plans[kind] = (plan, plan.norm("sm"))
        gold["graphs"][kind] = {"n_heavy_fwd": plan.fwd.n_heavy, "n_heavy_bwd": plan.bwd.n_heavy}
    for case in CASES:
        plan, norm = plans[case.graph]
        gold["cases"][case.name] = {
            "launches": run_case(case, ops, plan, norm, dev)[0],
            "routes": routes(plan_case(case, ops, plan.fwd, plan.bwd))}
    with open(path, "w") as f:
        json.dump(gold, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(GOLDEN)), os.pardir,
                                    "meta-gcn_amd"))
    record()
