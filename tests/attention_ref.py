"""Shared reference side of the attention tests (a plain helper module, not
collected): the tolerance, the torch restatement of the reference's attention
node model, and the graphs the cases run on.

Every comparison uses one tolerance, per compared tensor t:

    max|t_gpu - t64| <= max(4 * max|t32 - t64|, 1e-5 * max|t64|)

t32 / t64 are the reference's own fp32 and fp64 results (golden fixtures
att_*.npz, tests/golden/make_golden_attention.py) or, for the random cases, the
torch restatement below run in fp32 and fp64 on the CPU.  The factor 4 allows
for a summation order other than the reference's (same fp32 rounding class);
1e-5 is the project's dense-product bound (tests/test_gpu_headline.py).
"""
import numpy as np
import torch

# name -> (in, out, nheads, combine, dir, act, bias)   (make_golden_attention.py CASES)
FIXTURES = {
    "att_h1_cat_in_none": (16, 8, 1, "cat", "in", "none", False),
    "att_h4_cat_in_lrelu_bias": (8, 16, 4, "cat", "in", "lrelu", True),
    "att_h1_c7_in_lrelu": (32, 7, 1, "cat", "in", "lrelu", False),
    "att_h3_mean_out_relu": (16, 5, 3, "mean", "out", "relu", False),
    "att_h2_add_in_lrelu": (16, 8, 2, "add", "in", "lrelu", False),
    "att_hub_in": (8, 8, 2, "cat", "in", "lrelu", False),
    "att_hub_out": (8, 8, 2, "cat", "out", "lrelu", False),
}


def check(name, got, t32, t64):
    got = torch.as_tensor(got).detach().double().cpu()
    t32 = torch.as_tensor(t32).detach().double().cpu()
    t64 = torch.as_tensor(t64).detach().double().cpu()
    assert got.shape == t64.shape, (name, got.shape, t64.shape)
    if t64.numel() == 0:
        return
    assert torch.isfinite(got).all(), name
    err = (got - t64).abs().max().item()
    e32 = (t32 - t64).abs().max().item()
    bound = max(4 * e32, 1e-5 * t64.abs().max().item())
    print(f"{name}: err {err:.3e}  ref32 err {e32:.3e}  bound {bound:.3e}")
    assert err <= bound, f"{name}: {err:.3e} > {bound:.3e}"


# ------------------------------------------------------ torch restatement
def att_ref(x, W, att, bias, ei, H, combine, adir, act, mask=None):
    """graph_attention.py:60-117 + common.py:69-92 in plain torch (the dtype of
    x); returns (y, alpha', hp)."""
    N = x.size(0)
    src, dst = ei[0], ei[1]
    hp = (x @ W).view(N, H, -1)
    xj, xi = hp[src], hp[dst]
    z = (torch.cat([xj, xi], dim=-1) * att).sum(dim=-1)
    e = {"none": lambda t: t, "lrelu": lambda t: torch.nn.functional.leaky_relu(t, 0.2),
         "relu": torch.relu}[act](z)
    idx = src if adir == "out" else dst
    ix = idx.view(-1, 1).expand(-1, H)
    m = torch.full((N, H), -1e16, dtype=x.dtype).scatter_reduce(0, ix, e.detach(), "amax")
    p = (e - m[idx]).exp()
    s = torch.zeros(N, H, dtype=x.dtype).index_add(0, idx, p)
    alpha = p / (s[idx] + 1e-16)
    if mask is not None:
        alpha = alpha * mask.to(x.dtype)
    y = torch.zeros_like(hp).index_add(0, dst, xj * alpha.unsqueeze(-1))
    if combine == "cat":
        y = y.reshape(N, -1)
    elif combine == "add":
        y = y.sum(dim=1)
    else:
        y = y.mean(dim=1)
    if bias is not None:
        y = y + bias
    return y, alpha, hp


def ref_run(x, W, att, bias, ei, dY, H, combine, adir, act, dtype):
    x, W, att = (t.detach().clone().to(dtype).requires_grad_(True) for t in (x, W, att))
    b = None if bias is None else bias.detach().clone().to(dtype).requires_grad_(True)
    y, alpha, _ = att_ref(x, W, att, b, ei, H, combine, adir, act)
    y.backward(dY.to(dtype))
    return {"y": y.detach(), "alpha": alpha.detach(), "dx": x.grad, "dW": W.grad,
            "datt": att.grad, "db": None if b is None else b.grad}


def gpu_run(nm, x, ei, dY):
    x = x.detach().requires_grad_(True)
    nm.zero_grad()
    store = []
    y = nm(x, ei, attn_store=store)
    y.backward(dY)
    return {"y": y.detach(), "alpha": store[0], "dx": x.grad, "dW": nm.weight.grad,
            "datt": nm.att_weight.grad, "db": None if nm.bias is None else nm.bias.grad}


def make_node_model(cuda, fin, fout, H, combine, adir, act, bias, dropout=0.0):
    from mgcn.models import NodeModelAttention
    nm = NodeModelAttention(fin, fout, nheads=H, att_act=act, att_dropout=dropout,
                            att_combine=combine, att_dir=adir, bias=bias)
    if bias:
        nm.bias.data.uniform_(-0.5, 0.5)
    return nm.to(cuda)


# ----------------------------------------------------------------- graphs
_GRAPH = {}


def degree_graph():
    """N = 257 (no tile multiple); on the in side and on the out side a row of
    every degree in {0, 1, 63, 64, 65, 300} (node 0: no edge at all; nodes
    1-5: in-degree 1 / 63 / 64 / 65 / 300 and out-degree 0; nodes 6-10: the
    same out-degrees and in-degree 0), duplicates, shuffled COO order."""
    if not _GRAPH:
        rng = np.random.default_rng(11)
        N = 257
        parts = [rng.integers(11, N, (2, 1500))]
        for node, deg in zip(range(1, 6), (1, 63, 64, 65, 300)):
            parts.append(np.stack([rng.integers(11, N, deg), np.full(deg, node)]))
        for node, deg in zip(range(6, 11), (1, 63, 64, 65, 300)):
            parts.append(np.stack([np.full(deg, node), rng.integers(11, N, deg)]))
        ei = np.concatenate(parts, axis=1)
        ei = ei[:, rng.permutation(ei.shape[1])]
        ind = np.bincount(ei[1], minlength=N)
        outd = np.bincount(ei[0], minlength=N)
        assert list(ind[:11]) == [0, 1, 63, 64, 65, 300, 0, 0, 0, 0, 0]
        assert list(outd[:11]) == [0, 0, 0, 0, 0, 0, 1, 63, 64, 65, 300]
        _GRAPH["ei"] = torch.from_numpy(ei.astype(np.int64))
        _GRAPH["N"] = N
    return _GRAPH["ei"], _GRAPH["N"]


_LADDER = {}


def ladder_graph():
    """N = 200, a row of every degree 0..66 on either side: node v in 0..66 has
    in-degree exactly v and out-degree 0, node 67 + v has out-degree exactly v
    and in-degree 0.  The other endpoints are drawn with replacement from nodes
    134..199 (duplicates occur), which also carry 400 random edges among
    themselves; shuffled COO order.  For every head count H the flat chunk
    size G = 64 // H has a row of degree G - 1, G and G + 1 (for G <= 32 of
    2 G and 2 G + 1 as well)."""
    if not _LADDER:
        rng = np.random.default_rng(23)
        N = 200
        parts = [rng.integers(134, N, (2, 400))]
        for v in range(67):
            parts.append(np.stack([rng.integers(134, N, v), np.full(v, v)]))
            parts.append(np.stack([np.full(v, 67 + v), rng.integers(134, N, v)]))
        ei = np.concatenate(parts, axis=1)
        ei = ei[:, rng.permutation(ei.shape[1])]
        ind = np.bincount(ei[1], minlength=N)
        outd = np.bincount(ei[0], minlength=N)
        assert list(ind[:67]) == list(range(67)) and not outd[:67].any()
        assert list(outd[67:134]) == list(range(67)) and not ind[67:134].any()
        _LADDER["ei"] = torch.from_numpy(ei.astype(np.int64))
        _LADDER["N"] = N
    return _LADDER["ei"], _LADDER["N"]
