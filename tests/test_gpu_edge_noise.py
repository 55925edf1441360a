"""The seeded edge-noise generator on the MI355X (mgcn_edge_noise,
csrc/edge_noise.hip) against its numpy restatement (tests/philox_ref.py):
the bits of u, order independence over a plan's views, the Gumbel transform
against fp64, the dropout mask, statistics that a wrong counter layout fails,
and the opt-in through the attention ops, modules and models."""
import math

import numpy as np
import pytest
import torch

import philox_ref as pr

pytestmark = pytest.mark.gpu

SEED, OFFSET = 0xfedcba9876543210 >> 1, 2 ** 32 + 5  # both high words live
BAND = 64
SENTINEL = -7.0
# (nnz, H): one item, H % 4 in {1, 3, 0}, several groups of four heads, more
# than one block; the last two exceed the kernel's grid cap (2048 blocks of
# 256 items), so its grid-stride loop wraps, in the float4 and the scalar form
SHAPES = [(1, 1), (70, 5), (257, 3), (4099, 4), (1000, 16), (524288 + 4099, 4), (524288 + 70, 1)]
DEGREES = (0, 1, 64, 129, 300)
_CACHE = {}


def raw_fill(cuda, kind, nnz, H, eid=None, p=0.0, seed=SEED, offset=OFFSET, shift=0):
    """mgcn_edge_noise called directly on a buffer with a sentinel band behind
    (and ``shift`` floats in front of) out; returns (out [nnz, H], bands)."""
    import mgcn
    from mgcn import _lib as L
    lib = mgcn.load()
    buf = torch.full((shift + nnz * H + BAND,), SENTINEL, dtype=torch.float32, device=cuda)
    out = buf[shift:shift + nnz * H]
    rc = lib.mgcn_edge_noise(kind, seed, offset, nnz, H, L.ptr(eid), p, L.ptr(out),
                             L.stream_of(cuda))
    L.check(rc, "mgcn_edge_noise")
    return out.view(nnz, H).cpu().numpy(), torch.cat([buf[:shift], buf[shift + nnz * H:]]).cpu()


@pytest.mark.parametrize("perm", [False, True], ids=["coo", "perm"])
@pytest.mark.parametrize("nnz,H", SHAPES)
def test_uniform_bits(cuda, nnz, H, perm):
    from mgcn import _lib as L
    eid = None
    if perm:
        eid = np.random.default_rng(nnz + H).permutation(nnz).astype(np.int32)
    got, band = raw_fill(cuda, L.NOISE_UNIFORM, nnz, H,
                         None if eid is None else torch.from_numpy(eid).to(cuda))
    want = pr.uniform(SEED, OFFSET, nnz, H, eid)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert (band == SENTINEL).all()


def test_uniform_bits_unaligned_out(cuda):
    """H % 4 == 0 with out off the 16-byte grid: the scalar stores."""
    from mgcn import _lib as L
    got, band = raw_fill(cuda, L.NOISE_UNIFORM, 257, 4, shift=1)
    assert np.array_equal(got, pr.uniform(SEED, OFFSET, 257, 4))
    assert band.numel() == BAND + 1 and (band == SENTINEL).all()


def test_seed_and_offset_words_all_matter(cuda):
    from mgcn import _lib as L
    base, _ = raw_fill(cuda, L.NOISE_UNIFORM, 70, 5)
    for seed, offset in ((SEED ^ 1, OFFSET), (SEED ^ (1 << 40), OFFSET), (SEED, OFFSET ^ 1),
                         (SEED, OFFSET ^ (1 << 40))):
        got, _ = raw_fill(cuda, L.NOISE_UNIFORM, 70, 5, seed=seed, offset=offset)
        assert np.array_equal(got, pr.uniform(seed, offset, 70, 5))
        assert not np.array_equal(got, base)


def ladder(cuda):
    """(edge_index on the GPU, N, plan): 64 pool nodes with 300 random edges
    among themselves; one node of every in-degree in DEGREES and one of every
    out-degree (other endpoints drawn from 300 more nodes, so no further heavy
    row arises); shuffled COO order.  129 and 300 are heavy rows in both views."""
    if "g" not in _CACHE:
        from mgcn.graph import plan_for
        rng = np.random.default_rng(17)
        POOL, FAR, ND = 64, 300, len(DEGREES)
        N = POOL + FAR + 2 * ND
        parts = [rng.integers(0, POOL, (2, 300))]
        for i, d in enumerate(DEGREES):
            far = POOL + rng.permutation(FAR)[:d]
            parts.append(np.stack([far, np.full(d, POOL + FAR + i)]))
            parts.append(np.stack([np.full(d, POOL + FAR + ND + i), far]))
        ei = np.concatenate(parts, axis=1)
        ei = ei[:, rng.permutation(ei.shape[1])]
        ind, outd = np.bincount(ei[1], minlength=N), np.bincount(ei[0], minlength=N)
        assert tuple(ind[POOL + FAR:POOL + FAR + ND]) == DEGREES
        assert tuple(outd[POOL + FAR + ND:]) == DEGREES
        eig = torch.from_numpy(ei.astype(np.int64)).to(cuda)
        plan = plan_for(eig, N)
        for view in (plan.fwd, plan.bwd):
            assert view.order is not None and view.n_heavy == 2
        _CACHE["g"] = (eig, N, plan)
    return _CACHE["g"]


KINDS = [("uniform", None), ("gumbel", None), ("dropout", 0.5)]


@pytest.mark.parametrize("kind,p", KINDS)
@pytest.mark.parametrize("H", [3, 4])
def test_order_independence(cuda, kind, p, H):
    from mgcn import ops
    _, _, plan = ladder(cuda)
    coo = ops.edge_noise(plan, H, kind, seed=SEED, offset=OFFSET, p=p, order='coo')
    assert coo.shape == (plan.nnz, H) and coo.dtype == torch.float32 and coo.is_cuda
    for order, view in (('fwd', plan.fwd), ('bwd', plan.bwd)):
        got = ops.edge_noise(plan, H, kind, seed=SEED, offset=OFFSET, p=p, order=order)
        assert torch.equal(got, coo[view.eid.long()]), order
    if kind == "uniform":
        assert np.array_equal(coo.cpu().numpy(), pr.uniform(SEED, OFFSET, plan.nnz, H))


def test_edge_noise_argument_errors(cuda):
    import mgcn
    from mgcn import ops
    _, _, plan = ladder(cuda)
    with pytest.raises(ValueError, match="kind"):
        ops.edge_noise(plan, 2, "normal", seed=1, offset=2)
    with pytest.raises(ValueError, match="order"):
        ops.edge_noise(plan, 2, "gumbel", seed=1, offset=2, order='slot')
    with pytest.raises(ValueError, match="needs p"):
        ops.edge_noise(plan, 2, "dropout", seed=1, offset=2)
    with pytest.raises(ValueError, match="takes none"):
        ops.edge_noise(plan, 2, "gumbel", seed=1, offset=2, p=0.5)
    with pytest.raises(ValueError, match="seed"):
        ops.edge_noise(plan, 2, "gumbel", seed=-1, offset=2)
    with pytest.raises(mgcn.MgcnError, match="unsupported shape"):
        ops.edge_noise(plan, 17, "gumbel", seed=1, offset=2)
    with pytest.raises(mgcn.MgcnError, match="outside"):
        ops.edge_noise(plan, 2, "dropout", seed=1, offset=2, p=1.5)


def test_gumbel_against_fp64(cuda):
    """The device's fp32 Gumbel transform against the fp64 formula on the
    exact u: max|d - t64| <= max(4 max|t32 - t64|, 1e-5 max|t64|), t32 numpy's
    fp32 evaluation (the project's rule for an fp32 result)."""
    from mgcn import _lib as L
    worst = 0.0
    for nnz, H in ((4099, 4), (20000, 3), (1000, 16)):
        got, band = raw_fill(cuda, L.NOISE_GUMBEL, nnz, H)
        u = pr.uniform(SEED, OFFSET, nnz, H)
        t32, t64 = pr.gumbel32(u), pr.gumbel64(u)
        assert np.isfinite(got).all() and (band == SENTINEL).all()
        err = np.abs(got.astype(np.float64) - t64).max()
        e32 = np.abs(t32.astype(np.float64) - t64).max()
        bound = max(4 * e32, 1e-5 * np.abs(t64).max())
        print(f"gumbel ({nnz}, {H}): device err {err:.3e}  numpy fp32 err {e32:.3e}  "
              f"bound {bound:.3e}  range {got.min():.3f} .. {got.max():.3f}")
        assert err <= bound
        worst = max(worst, err)
    print(f"gumbel: max device err {worst:.3e}")


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5, 0.9, 1.0])
def test_dropout_mask(cuda, p):
    from mgcn import _lib as L
    for nnz, H in ((4099, 4), (257, 3)):
        got, band = raw_fill(cuda, L.NOISE_DROPOUT, nnz, H, p=p)
        u = pr.uniform(SEED, OFFSET, nnz, H)
        keep = pr.dropout_keep(u, p)
        assert np.array_equal(got != 0, keep)
        assert (got[~keep] == 0).all()
        if p < 1.0:
            assert (got[keep] == pr.dropout_scale(p)).all()
        assert np.array_equal(got, pr.dropout32(u, p))
        assert (band == SENTINEL).all()
        if p == 0.0:
            assert (got == 1.0).all()
        if p == 1.0:
            assert (got == 0.0).all()


def test_statistics(cuda):
    """Moments and correlations no wrong counter layout passes (a repeated or
    stuck counter word correlates heads or edges), each within 4 sigma."""
    from mgcn import _lib as L
    seed, nnz, H = 20260301, 20000, 3
    n = nnz * H

    def within(name, value, expect, sigma):
        z = (value - expect) / sigma
        print(f"{name}: {value:.6f}  expect {expect:.6f}  {z:+.2f} sigma")
        assert abs(z) <= 4.0, name

    u, _ = raw_fill(cuda, L.NOISE_UNIFORM, nnz, H, seed=seed, offset=0)
    assert np.array_equal(u, pr.uniform(seed, 0, nnz, H))
    u = u.astype(np.float64)
    within("mean of u", u.mean(), 0.5, math.sqrt(1 / 12 / n))
    g, _ = raw_fill(cuda, L.NOISE_GUMBEL, nnz, H, seed=seed, offset=0)
    g = g.astype(np.float64)
    v = math.pi ** 2 / 6
    within("Gumbel mean", g.mean(), 0.5772157, math.sqrt(v / n))
    within("Gumbel variance", g.var(), v, math.sqrt(4.4) * v / math.sqrt(n))
    for p in (0.1, 0.5, 0.9):
        m, _ = raw_fill(cuda, L.NOISE_DROPOUT, nnz, H, p=p, seed=seed, offset=0)
        within(f"keep fraction at p = {p}", (m != 0).mean(), 1 - p, math.sqrt(p * (1 - p) / n))
    cap = 4 / math.sqrt(nnz)
    heads = np.corrcoef(u[:, 0], u[:, 1])[0, 1]
    lag = np.corrcoef(u[:-1, 0], u[1:, 0])[0, 1]
    print(f"corr(u[:, 0], u[:, 1]) {heads:+.4f}  lag-1 of u[:, 0] {lag:+.4f}  cap {cap:.4f}")
    assert abs(heads) <= cap and abs(lag) <= cap


# ------------------------------------------------------------------- ops
def _op_inputs(cuda, H, C, dtype, seed):
    _, N, plan = ladder(cuda)
    gen = torch.Generator().manual_seed(900 + seed)
    Hp = torch.randn(N, H * C, generator=gen).to(cuda).to(dtype)
    att = (torch.randn(1, H, 2 * C, generator=gen) * 0.5).to(cuda)
    dY = torch.randn(N, H * C, generator=gen).to(cuda).to(dtype)
    return plan, Hp, att, dY


def _run(fn, Hp, att, dY, want_datt=True):
    Hp = Hp.clone().requires_grad_(True)
    att = att.clone().requires_grad_(True)
    Y, alpha = fn(Hp, att)
    Y.backward(dY)
    out = [Y.detach(), alpha, Hp.grad]
    if want_datt:
        out.append(att.grad)
    else:
        assert att.grad is None
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("H", [3, 4])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("adir", ["in", "out"])
def test_hard_attention_descriptors_equal_coo_tensors(cuda, adir, training, H, dtype):
    """Descriptors realised in slot order against the same values handed over
    as COO tensors (today's path: permuted by the op), heavy-row routing on."""
    from mgcn import ops
    assert ops.attention_heavy_rows()
    plan, Hp, att, dY = _op_inputs(cuda, H, 4, dtype, H)
    s, o, s2, o2 = 11, 2 ** 40 + 3, 2 ** 62 + 1, 7
    noise = ops.edge_noise(plan, H, "gumbel", seed=s, offset=o, order='coo')
    mask = ops.edge_noise(plan, H, "dropout", seed=s2, offset=o2, p=0.5, order='coo')
    assert 0.3 < (mask == 0).float().mean().item() < 0.7

    def with_tensors(Hp, att):
        return ops.hard_attention_aggregate(Hp, att, plan, H, 'lrelu', adir, 0.5,
                                            training=training, noise=noise, edge_mask=mask)

    def with_descriptors(Hp, att):
        return ops.hard_attention_aggregate(Hp, att, plan, H, 'lrelu', adir, 0.5,
                                            training=training, noise=ops.DeviceGumbel(s, o),
                                            edge_mask=ops.DeviceDropout(0.5, s2, o2))
    a = _run(with_tensors, Hp, att, dY, want_datt=training)
    b = _run(with_descriptors, Hp, att, dY, want_datt=training)
    for name, x, y in zip(("Y", "alpha_coo", "dHp", "datt"), a, b):
        assert x.dtype == y.dtype and torch.equal(x, y), name
    assert a[0].dtype == dtype and torch.isfinite(a[0].float()).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("H", [3, 4])
@pytest.mark.parametrize("adir", ["in", "out"])
def test_attention_descriptor_equals_coo_tensor(cuda, adir, H, dtype):
    from mgcn import ops
    plan, Hp, att, dY = _op_inputs(cuda, H, 4, dtype, 10 + H)
    s2, o2 = 2 ** 62 + 1, 7
    mask = ops.edge_noise(plan, H, "dropout", seed=s2, offset=o2, p=0.5, order='coo')
    a = _run(lambda Hp, att: ops.attention_aggregate(Hp, att, plan, H, 'lrelu', adir,
                                                     edge_mask=mask), Hp, att, dY)
    b = _run(lambda Hp, att: ops.attention_aggregate(
        Hp, att, plan, H, 'lrelu', adir, edge_mask=ops.DeviceDropout(0.5, s2, o2)), Hp, att, dY)
    for name, x, y in zip(("Y", "alpha_coo", "dHp", "datt"), a, b):
        assert x.dtype == y.dtype and torch.equal(x, y), name
    # the mask reached alpha: a dropped edge has alpha' == 0
    assert (a[1][mask == 0] == 0).all() and (a[1] != 0).any()


# --------------------------------------------------------------- modules
class _Names:
    """A kernel timer that records the names of the launches it brackets."""

    def __init__(self):
        self.names = []

    def __call__(self, name, start, rows=None, edges=None):
        if start:
            self.names.append(name)

    def __enter__(self):
        from mgcn import ops
        ops.set_kernel_timer(self)
        return self

    def __exit__(self, *exc):
        from mgcn import ops
        ops.set_kernel_timer(None)
        return False


def _small_graph(cuda, n=40, E=220, seed=3):
    rng = np.random.default_rng(seed)
    e = rng.integers(0, n, (2, E))
    e = np.unique(e[:, e[0] != e[1]], axis=1)
    e = e[:, rng.permutation(e.shape[1])]
    x = torch.from_numpy(rng.standard_normal((n, 6)).astype(np.float32)).to(cuda)
    return x, torch.from_numpy(e.astype(np.int64)).to(cuda), n


def _no_host_draws(monkeypatch):
    """The torch path's draws raise: the module globals the reference's noise
    goes through, torch.rand under them, and F.dropout of the [E, H] ones."""
    import mgcn.models as M
    import mgcn.votepool as V

    def raises(*a, **k):
        raise AssertionError("edge_rng='device' drew on the host")
    monkeypatch.setattr(M, "gumbel_samples", raises)
    monkeypatch.setattr(V, "gumbel_samples", raises)
    monkeypatch.setattr(torch, "rand", raises)
    monkeypatch.setattr(torch.nn.functional, "dropout", raises)


def _module_cases(cuda):
    from mgcn.models import NodeModelAttention, NodeModelHardAttention
    from mgcn.votepool import VotePoolLayer
    x, ei, n = _small_graph(cuda)

    def node(cls, **kw):
        def make(edge_rng):
            torch.manual_seed(5)
            extra = {} if edge_rng is None else {"edge_rng": edge_rng}
            m = cls(6, 8, nheads=2, att_act='lrelu', att_dropout=0.5, **kw, **extra).to(cuda)
            return m, (lambda: m(x, ei))
        return make

    def vote(edge_rng):
        torch.manual_seed(5)
        extra = {} if edge_rng is None else {"edge_rng": edge_rng}
        m = VotePoolLayer(6, 8, nheads=2, att_act='lrelu', att_dropout=0.5, temperature=0.5,
                          **extra).to(cuda)
        return m, (lambda: m(x, ei, [0, n])[0])
    # (factory, edge_noise launches of one training forward)
    return {"attention": (node(NodeModelAttention), 1),
            "hard": (node(NodeModelHardAttention, temperature=0.5), 2),
            "vote": (vote, 2)}


@pytest.mark.parametrize("which", ["attention", "hard", "vote"])
def test_modules_train_on_device_noise(cuda, monkeypatch, which):
    make, launches = _module_cases(cuda)[which]
    # the default keeps today's path: host draws, no edge_noise launch
    m, fwd = make(None)
    assert m.edge_rng == 'torch'
    with _Names() as t:
        fwd().sum().backward()
    assert "edge_noise" not in t.names and t.names
    _no_host_draws(monkeypatch)
    with pytest.raises(AssertionError, match="drew on the host"):
        make('torch')[1]()
    m, fwd = make('device')
    m.train()
    with _Names() as t:
        y = fwd()
        y.sum().backward()
    assert t.names.count("edge_noise") == launches
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    assert torch.isfinite(y).all() and y.abs().sum() > 0
    # torch.manual_seed replays the forward; successive forwards differ
    torch.manual_seed(77)
    y1, y2 = fwd().detach(), fwd().detach()
    torch.manual_seed(77)
    y3 = fwd().detach()
    assert torch.equal(y1, y3) and not torch.equal(y1, y2)
    # eval: no dropout mask; noise only under sample=True
    m.eval()
    with _Names() as t, torch.no_grad():
        fwd()
    assert "edge_noise" not in t.names
    if which != "attention":
        m.sample = True
        with _Names() as t, torch.no_grad():
            fwd()
        assert t.names.count("edge_noise") == 1


def test_models_train_on_device_noise(cuda, monkeypatch):
    from mgcn.models import GCNModel
    from mgcn.votepool import VotePoolModel
    import mgcn.models as M
    import mgcn.votepool as V

    def raises(*a, **k):
        raise AssertionError("edge_rng='device' drew on the host")
    monkeypatch.setattr(M, "gumbel_samples", raises)
    monkeypatch.setattr(V, "gumbel_samples", raises)
    x, ei, n = _small_graph(cuda)
    torch.manual_seed(9)
    gcn = GCNModel(6, [8, 8], 3, nodemodel='attention', nheads=2, att_dropout=0.5,
                   residual_hop=1, final_type='proj', edge_rng='device').to(cuda).train()
    vote = VotePoolModel(6, [8, 8], 3, nheads=2, att_dropout=0.5, temperature=0.5,
                         edge_rng='device').to(cuda).train()
    for name, m, fwd, launches in (("gcn", gcn, lambda: gcn(x, ei), 2),
                                   ("vote", vote, lambda: vote(x, ei, [0, n]), 4)):
        with _Names() as t:
            y = fwd()
            y.sum().backward()
        assert t.names.count("edge_noise") == launches, name
        assert torch.isfinite(y).all(), name
        for k, p in m.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), (name, k)
