"""NodeModelAttention on the fused HIP attention kernels (MI355X).

Every comparison uses one tolerance, per compared tensor t:

    max|t_gpu - t64| <= max(4 * max|t32 - t64|, 1e-5 * max|t64|)

t32 / t64 are the reference's own fp32 and fp64 results (golden fixtures
att_*.npz, tests/golden/make_golden_attention.py) or, for the random cases, the
torch restatement (tests/attention_ref.py) run in fp32 and fp64 on the CPU.
The factor 4 allows for a summation order other than the reference's (same
fp32 rounding class); 1e-5 is the project's dense-product bound
(tests/test_gpu_headline.py).
"""
import pytest
import torch

from attention_ref import (FIXTURES, att_ref, check, degree_graph, gpu_run,
                           make_node_model, ref_run)
from conftest import load_golden

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------- fixtures
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_fixture(cuda, name):
    """y, alpha (from attn_store, COO order), dx, dW, datt, db against the
    reference's own fp64 run."""
    fin, fout, H, combine, adir, act, bias = FIXTURES[name]
    z = load_golden(name)
    nm = make_node_model(cuda, fin, fout, H, combine, adir, act, bias)
    sd = {k[2:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("p_")}
    nm.load_state_dict(sd, strict=True)
    ei = torch.from_numpy(z["edge_index"]).to(cuda)
    got = gpu_run(nm, torch.from_numpy(z["x"]).to(cuda), ei, torch.from_numpy(z["dY"]).to(cuda))
    assert got["alpha"].shape == (ei.size(1), H) and not got["alpha"].requires_grad
    for k in ("y", "alpha", "dx", "dW", "datt") + (("db",) if bias else ()):
        check(f"{name}.{k}", got[k], z[k + "32"], z[k + "64"])


def test_model_citation(cuda):
    """The citation GCNModel (3 attention layers, heads 2 / 2 / 1, residual
    hop 1): output, input gradient and every parameter gradient against the
    reference model's own fp64 run."""
    from mgcn.models import GCNModel
    z = load_golden("att_model_citation")
    m = GCNModel(24, [32, 32, 7], 7, nheads=[2, 2, 1], residual_hop=1, nodemodel='attention',
                 bias=False, dropout=0, att_act='lrelu', att_dir='in', final_type='none')
    m.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("p_")},
                      strict=True)
    m = m.to(cuda)
    x = torch.from_numpy(z["x"]).to(cuda).requires_grad_(True)
    ei = torch.from_numpy(z["edge_index"]).to(cuda)
    store = []
    y = m(x, ei, attn_store=store)
    y.backward(torch.from_numpy(z["dY"]).to(cuda))
    assert [tuple(a.shape) for a in store] == [(ei.size(1), h) for h in (2, 2, 1)]
    check("model.y", y, z["y32"], z["y64"])
    check("model.dx", x.grad, z["dx32"], z["dx64"])
    for k, p in m.named_parameters():
        check("model.g_" + k, p.grad, z["g_" + k + "32"], z["g_" + k + "64"])


# ------------------------------------------------------------ random cases
RANDOM = [  # (H, C, combine, dir, act, bias)
    (1, 1, "cat", "in", "none", False),
    (1, 7, "cat", "out", "lrelu", True),
    (2, 16, "cat", "in", "lrelu", False),
    (3, 5, "mean", "out", "relu", True),
    (8, 16, "cat", "in", "relu", False),
    (4, 130, "add", "out", "none", False),
    (16, 64, "cat", "in", "lrelu", False),
]


@pytest.mark.parametrize("H,C,combine,adir,act,bias", RANDOM)
def test_random_against_restatement(cuda, H, C, combine, adir, act, bias):
    ei, N = degree_graph()
    fin = 12
    fout = H * C if combine == "cat" else C
    g = torch.Generator().manual_seed(100 * H + C)
    nm = make_node_model(cuda, fin, fout, H, combine, adir, act, bias)
    wide = torch.randn(N, fin + 5, generator=g)
    x = wide[:, 3:3 + fin]  # a strided slice of a wider tensor
    dY = torch.randn(N, fout, generator=g)
    W, att = nm.weight.detach().cpu(), nm.att_weight.detach().cpu()
    b = None if nm.bias is None else nm.bias.detach().cpu()
    r32 = ref_run(x, W, att, b, ei, dY, H, combine, adir, act, torch.float32)
    r64 = ref_run(x, W, att, b, ei, dY, H, combine, adir, act, torch.float64)
    xg = wide.to(cuda)[:, 3:3 + fin]
    assert not xg.is_contiguous()
    got = gpu_run(nm, xg, ei.to(cuda), dY.to(cuda))
    for k in ("y", "alpha", "dx", "dW", "datt") + (("db",) if bias else ()):
        check(f"H{H}C{C}{adir}{act}.{k}", got[k], r32[k], r64[k])


@pytest.mark.parametrize("adir", ["in", "out"])
def test_large_logits(cuda, adir):
    """att_weight scaled until |z| reaches ~100: no inf / nan, every group's
    alpha sums to 1, alpha within the tolerance."""
    ei, N = degree_graph()
    H, C, fin = 2, 8, 12
    g = torch.Generator().manual_seed(5)
    nm = make_node_model(cuda, fin, H * C, H, "cat", adir, "lrelu", False)
    x = torch.randn(N, fin, generator=g)
    W, att = nm.weight.detach().cpu(), nm.att_weight.detach().cpu()
    hp = (x @ W).view(N, H, C)
    z = (torch.cat([hp[ei[0]], hp[ei[1]]], dim=-1) * att).sum(-1)
    att = att * (100.0 / z.abs().max())
    nm.att_weight.data.copy_(att)
    dY = torch.randn(N, H * C, generator=g)
    r32 = ref_run(x, W, att, None, ei, dY, H, "cat", adir, "lrelu", torch.float32)
    r64 = ref_run(x, W, att, None, ei, dY, H, "cat", adir, "lrelu", torch.float64)
    got = gpu_run(nm, x.to(cuda), ei.to(cuda), dY.to(cuda))
    for k in ("y", "alpha", "dx", "dW", "datt"):
        assert torch.isfinite(got[k]).all(), k
    idx = ei[0] if adir == "out" else ei[1]
    sums = torch.zeros(N, H, dtype=torch.float64).index_add(0, idx, got["alpha"].double().cpu())
    has = torch.bincount(idx, minlength=N) > 0
    dev = (sums[has] - 1).abs().max().item()
    print(f"large logits {adir}: max |sum alpha - 1| = {dev:.3e}")
    assert dev <= 1e-5
    assert torch.count_nonzero(sums[~has]) == 0
    check(f"large.{adir}.alpha", got["alpha"], r32["alpha"], r64["alpha"])
    check(f"large.{adir}.y", got["y"], r32["y"], r64["y"])


@pytest.mark.parametrize("adir,H,C", [("in", 3, 5), ("out", 4, 16)])
def test_bitwise_repeatable(cuda, adir, H, C):
    ei, N = degree_graph()
    g = torch.Generator().manual_seed(9)
    nm = make_node_model(cuda, 12, H * C, H, "cat", adir, "lrelu", True)
    x = torch.randn(N, 12, generator=g).to(cuda)
    dY = torch.randn(N, H * C, generator=g).to(cuda)
    eig = ei.to(cuda)
    a = {k: v.clone() for k, v in gpu_run(nm, x, eig, dY).items()}
    b = gpu_run(nm, x, eig, dY)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("adir", ["in", "out"])
def test_dropout(cuda, adir):
    """Training mode, p = 0.5, E * H ~ 1e4: the zeroed share of the stored
    alpha' is within 8 sigma of 1/2, survivors are 2 alpha of an eval pass, y
    is the aggregate of the stored alpha'; eval with p = 0.6 is bitwise p = 0."""
    ei, N = degree_graph()
    H, C, fin = 4, 8, 12
    E = ei.size(1)
    assert 9000 <= E * H <= 11000
    g = torch.Generator().manual_seed(21)
    nm = make_node_model(cuda, fin, H * C, H, "cat", adir, "lrelu", False, dropout=0.5)
    x = torch.randn(N, fin, generator=g)
    xg, eig = x.to(cuda), ei.to(cuda)
    W, att = nm.weight.detach().cpu(), nm.att_weight.detach().cpu()
    nm.eval()
    ev = []
    y_eval = nm(xg, eig, attn_store=ev)
    nm.train()
    torch.manual_seed(1234)
    tr = []
    y_tr = nm(xg, eig, attn_store=tr)
    a_tr = tr[0].cpu()
    zero = a_tr == 0
    share = zero.double().mean().item()
    print(f"dropout {adir}: zeroed share {share:.4f}")
    assert 0.46 <= share <= 0.54
    refs = {}
    for dt in (torch.float32, torch.float64):
        _, alpha, hp = att_ref(x.to(dt), W.to(dt), att.to(dt), None, ei, H, "cat", adir, "lrelu")
        y = torch.zeros_like(hp).index_add(0, ei[1], hp[ei[0]] * a_tr.to(dt).unsqueeze(-1))
        refs[dt] = (2 * alpha, y.reshape(N, -1))
    keep = ~zero
    check(f"dropout.{adir}.survivors", a_tr[keep], refs[torch.float32][0][keep],
          refs[torch.float64][0][keep])
    check(f"dropout.{adir}.y", y_tr, refs[torch.float32][1], refs[torch.float64][1])
    # the gradient flows through the masked coefficients without inf / nan
    nm.zero_grad()
    torch.manual_seed(1234)
    y2 = nm(xg, eig)
    assert torch.equal(y2, y_tr)  # same seed, same mask
    y2.sum().backward()
    assert torch.isfinite(nm.weight.grad).all() and torch.isfinite(nm.att_weight.grad).all()
    # eval: dropout is the identity
    nm.eval()
    nm.att_dropout.p = 0.6
    st = []
    y06 = nm(xg, eig, attn_store=st)
    assert torch.equal(y06, y_eval) and torch.equal(st[0], ev[0])


@pytest.mark.parametrize("adir", ["in", "out"])
def test_dropout_gradient(cuda, adir):
    """Backward under a given edge mask (ops.attention_aggregate) against
    autograd of the restatement with the same mask."""
    from mgcn.graph import plan_for
    from mgcn.ops import attention_aggregate, linear
    ei, N = degree_graph()
    H, C, fin = 2, 6, 12
    g = torch.Generator().manual_seed(33)
    x = torch.randn(N, fin, generator=g)
    W = torch.randn(fin, H * C, generator=g) * 0.3
    att = torch.randn(1, H, 2 * C, generator=g) * 0.5
    dY = torch.randn(N, H * C, generator=g)
    mask = (torch.rand(ei.size(1), H, generator=g) < 0.5).float() * 2
    res = {}
    for dt in (torch.float32, torch.float64):
        xs, Ws, As = (t.clone().to(dt).requires_grad_(True) for t in (x, W, att))
        y, alpha, _ = att_ref(xs, Ws, As, None, ei, H, "cat", adir, "lrelu", mask=mask)
        y.backward(dY.to(dt))
        res[dt] = {"y": y.detach(), "alpha": alpha.detach(), "dx": xs.grad, "dW": Ws.grad,
                   "datt": As.grad}
    xs, Ws, As = (t.to(cuda).requires_grad_(True) for t in (x, W, att))
    eig = ei.to(cuda)
    y, alpha = attention_aggregate(linear(xs, Ws), As, plan_for(eig, N), H, "lrelu", adir,
                                   edge_mask=mask.to(cuda))
    y.backward(dY.to(cuda))
    got = {"y": y, "alpha": alpha, "dx": xs.grad, "dW": Ws.grad, "datt": As.grad}
    for k in got:
        check(f"mask.{adir}.{k}", got[k], res[torch.float32][k], res[torch.float64][k])


@pytest.mark.parametrize("adir", ["in", "out"])
def test_empty_graph(cuda, adir):
    """E = 0: the output is the bias (or zeros), gradients are zero."""
    ei = torch.zeros(2, 0, dtype=torch.int64, device=cuda)
    x = torch.randn(9, 4).to(cuda).requires_grad_(True)
    for bias in (True, False):
        nm = make_node_model(cuda, 4, 6, 2, "cat", adir, "lrelu", bias)
        store = []
        y = nm(x, ei, attn_store=store)
        want = nm.bias.detach().expand(9, 6) if bias else torch.zeros(9, 6, device=cuda)
        assert torch.equal(y, want)
        assert store[0].shape == (0, 2)
        y.sum().backward()
        assert torch.count_nonzero(nm.weight.grad) == 0
        assert torch.count_nonzero(nm.att_weight.grad) == 0


def test_multi_kernel_shares_one_attn_store(cuda):
    """GCNMultiKernel(num_kernel=2, kernel_combine='add') over two edge sets:
    the sum of the two node models' outputs; one attn_store gets two entries."""
    from mgcn.models import GCNMultiKernel
    ei, N = degree_graph()
    g = torch.Generator().manual_seed(3)
    ei2 = torch.randint(0, N, (2, 900), generator=g)
    mk = GCNMultiKernel(12, 8, None, num_kernel=2, nodemodel='attention', kernel_combine='add',
                        nheads=2, att_act='lrelu').to(cuda)
    x = torch.randn(N, 12, generator=g).to(cuda)
    e1, e2 = ei.to(cuda), ei2.to(cuda)
    store = []
    y = mk(x, [e1, e2], attn_store=store)
    assert [tuple(a.shape) for a in store] == [(ei.size(1), 2), (900, 2)]
    y1 = mk.node_models[0](x, e1)
    y2 = mk.node_models[1](x, e2)
    assert torch.equal(y, y1 + y2)
