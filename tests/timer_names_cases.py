"""One pass over every timed libmgcn launch family through mgcn.ops' public
API, at the smallest shapes that still take each path, with a recording kernel
timer: the driver of tests/test_gpu_timer_names.py and of the golden file
tests/golden/ops_timer_names.json (recorded with this driver on the commit
before mgcn/ops.py was split).

The graph: N = 70 nodes, 300 random edges and the self loops -- three 32-row
chunks, the last one partial."""
import json
import os

import numpy as np
import torch

N, E = 70, 300
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ops_timer_names.json")


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def edge_index():
    rng = np.random.default_rng(7)
    s, d = rng.integers(0, N, E), rng.integers(0, N, E)
    loops = np.arange(N)
    return np.stack([np.concatenate([s, loops]), np.concatenate([d, loops])]).astype(np.int64)


def _t(g, dev, *shape, scale=1.0, grad=True):
    return (torch.randn(*shape, generator=g) * scale).to(dev).requires_grad_(grad)


def _residual(ops, plan, norm, g, dev, f_in, f):
    x = _t(g, dev, N, f_in)
    ps = [_t(g, dev, f_in, f, scale=0.3), _t(g, dev, f, scale=0.1), _t(g, dev, f, f_in, scale=0.3),
          _t(g, dev, f, scale=0.1)]
    return ops.residual_gcn_layer(x, plan, norm, "add", True, True, *ps), [x] + ps


def _gcn_layer(aggr):
    def run(ops, plan, norm, g, dev):
        x, W, b = _t(g, dev, N, 128), _t(g, dev, 128, 128, scale=0.09), _t(g, dev, 128, scale=0.1)
        return ops.gcn_layer(x, W, plan, norm, aggr, b, True), [x, W, b]
    return run


def _attention(att_dir):
    def run(ops, plan, norm, g, dev):
        Hp, att = _t(g, dev, N, 8), _t(g, dev, 1, 2, 8)
        return ops.attention_aggregate(Hp, att, plan, 2, "lrelu", att_dir)[0], [Hp, att]
    return run


def _hard_attention(training):
    def run(ops, plan, norm, g, dev):
        Hp, att = _t(g, dev, N, 8), _t(g, dev, 1, 2, 8)
        noise = torch.randn(plan.nnz, 2, generator=g).to(dev)
        y = ops.hard_attention_aggregate(Hp, att, plan, 2, "lrelu", "in", 0.5, training=training,
                                         noise=noise)[0]
        return y, [Hp, att] if training else [Hp]
    return run


def _linear_bias(ops, plan, norm, g, dev):
    x, W, b = _t(g, dev, N, 48), _t(g, dev, 24, 48, scale=0.2), _t(g, dev, 24, scale=0.1)
    return ops.linear_bias(x, W, b), [x, W, b]


def _bmm(ops, plan, norm, g, dev):
    a, b = _t(g, dev, 3, N, 20), _t(g, dev, 20, 12)
    return ops.bmm(a, b), [a, b]


def _scatter(ops, plan, norm, g, dev):
    src = _t(g, dev, E, 16)
    index = torch.randint(0, N, (E,), generator=g).to(dev)
    return ops.scatter_("mean", src, index, N), [src]


def _segment_mean(ops, plan, norm, g, dev):
    x = _t(g, dev, N, 16)
    ptr = torch.tensor([0, 9, 9, 41, N], dtype=torch.int64, device=dev)
    return ops.segment_mean(x, ptr), [x]


CASES = {
    "gcn_layer_sum_f128": _gcn_layer("add"),
    "gcn_layer_max_f128": _gcn_layer("max"),
    "residual_f32_fused": lambda ops, plan, norm, g, dev: _residual(ops, plan, norm, g, dev, 32, 32),
    "residual_f48_two_launch": lambda ops, plan, norm, g, dev: _residual(ops, plan, norm, g, dev,
                                                                         48, 48),
    "input_layer_in1": lambda ops, plan, norm, g, dev: _residual(ops, plan, norm, g, dev, 1, 32),
    "attention_in": _attention("in"),
    "attention_out": _attention("out"),
    "hard_attention_train": _hard_attention(True),
    "hard_attention_eval": _hard_attention(False),
    "linear_bias": _linear_bias,
    "bmm": _bmm,
    "scatter_mean": _scatter,
    "segment_mean": _segment_mean,
}


def run_all(ops, dev):
    """{case: (events, tensors)}: ``events`` every call of the kernel timer
    during the case's forward + backward, as [name, start, rows, edges] (a stop
    carries None, None); ``tensors`` the output and every input gradient."""
    from mgcn.graph import plan_for
    ei = torch.from_numpy(edge_index()).to(dev)
    plan = plan_for(ei, N)
    norm = plan.norm("sm")
    out = {}
    for i, (name, case) in enumerate(CASES.items()):
        g = torch.Generator().manual_seed(100 + i)
        events = []
        ops.set_kernel_timer(lambda name, start, rows=None, edges=None:
                             events.append([name, bool(start), rows, edges]))
        try:
            y, leaves = case(ops, plan, norm, g, dev)
            y.backward(torch.randn(y.shape, generator=g).to(dev))
        finally:
            ops.set_kernel_timer(None)
        out[name] = (events, [y.detach()] + [t.grad for t in leaves])
    return out


def launches(events):
    """The start calls of ``events`` as the golden file stores them."""
    return [[n, rows, edges] for n, start, rows, edges in events if start]
