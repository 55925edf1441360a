"""Attention and hard attention on bf16 feature rows (MI355X): the
mgcn_*_bf16 attention entries and everything mgcn.ops / mgcn.models route to
them.

The reference of every case is the fp32 path -- held to the reference
implementation's fp64 fixtures by the other attention tests -- run in the same
process on ``Hp.float()`` / ``dY.float()``.  The contract is bitwise: fp32
outputs (alpha, datt) are ``torch.equal``, bf16 outputs (Y, dHp) have the bit
patterns of the fp32 result rounded once (``.cpu().to(torch.bfloat16)``,
compared as ``int16``).  No tolerance anywhere.

Graph: attention_ref.ladder_graph (N = 200; a row of every in- and out-degree
0 .. 66, so G - 1, G, G + 1 of the flat chunk G = 64 // H for every H) plus a
node of in-degree 230 and one of out-degree 230 among nodes 134 .. 199, which
leaves the ladder's degrees alone."""
import functools

import numpy as np
import pytest
import torch

from attention_ref import ladder_graph

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
HUB_IN, HUB_OUT, HUB_DEG = 190, 191, 230

# FPL 1 / 1 / 2 / 2 / 4 / 8 / 16 / 16; pow2 and non-pow2 C; odd widths 65, 129,
# 257, 513; H C = 1024
WIDTHS = [(3, 4), (8, 8), (5, 13), (2, 64), (3, 43), (1, 257), (16, 64), (1, 513)]
ACTS = ("none", "lrelu", "relu")
FP32_ROW_LAUNCHES = {"att_scores", "att_fwd", "att_bwd_dst", "att_bwd_src", "att_dst_fold",
                     "hatt_fwd", "hatt_bwd_dst", "hatt_bwd_src", "hatt_gather"}


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def same_bits(got, want32):
    """got (bf16, device) against the fp32 path's result rounded once."""
    assert got.dtype == BF16 and want32.dtype == torch.float32
    return torch.equal(bits(got), bits(want32.detach().cpu().to(BF16)))


@functools.lru_cache(maxsize=None)
def graph():
    from mgcn.graph import plan_for
    ei, N = ladder_graph()
    rng = np.random.default_rng(5)
    other = torch.from_numpy(rng.integers(134, N, (2, HUB_DEG)))
    hub_in = torch.stack([other[0], torch.full((HUB_DEG,), HUB_IN)])
    hub_out = torch.stack([torch.full((HUB_DEG,), HUB_OUT), other[1]])
    ei = torch.cat([ei, hub_in, hub_out], dim=1)
    ei = ei[:, torch.from_numpy(rng.permutation(ei.size(1)))].contiguous()
    ind = torch.bincount(ei[1], minlength=N)
    outd = torch.bincount(ei[0], minlength=N)
    assert ind[:67].tolist() == list(range(67)) and outd[67:134].tolist() == list(range(67))
    assert int(ind[HUB_IN]) > 200 and int(outd[HUB_OUT]) > 200
    eig = ei.cuda()
    return eig, N, plan_for(eig, N), (ind == 0).cuda()


def inputs(H, C, seed):
    """bf16 Hp and dY, the fp32 attention vector, a keep-half dropout mask and
    Gumbel-like noise, all on the device."""
    ei, N, _, _ = graph()
    E = ei.size(1)
    g = torch.Generator().manual_seed(seed)
    Hp = torch.randn(N, H * C, generator=g).to(BF16).cuda()
    dY = torch.randn(N, H * C, generator=g).to(BF16).cuda()
    att = (torch.randn(1, H, 2 * C, generator=g) * 0.5).cuda()
    mask = ((torch.rand(E, H, generator=g) < 0.5).float() * 2).cuda()
    u = torch.rand(E, H, generator=g).clamp_(1e-6, 1 - 1e-6)
    noise = (-(-u.log()).log()).cuda()
    return Hp, dY, att, mask, noise


def run(op, Hp, dY, att, need_att=True):
    """One forward + backward of ``op(Hp_leaf, att_leaf)`` -> (Y, alpha_coo)."""
    Hp = Hp.detach().clone().requires_grad_(True)
    att = att.detach().clone().requires_grad_(need_att)
    y, alpha = op(Hp, att)
    assert not alpha.requires_grad and alpha.dtype == torch.float32
    y.backward(dY)
    return {"y": y.detach(), "alpha": alpha, "dHp": Hp.grad, "datt": att.grad}


def check_against_fp32(op, Hp, dY, att, tag, datt=True):
    """The bf16 run against the fp32 op on the upcast rows, and against itself."""
    _, _, _, no_in = graph()
    r32 = run(op, Hp.float(), dY.float(), att, need_att=datt)
    got = run(op, Hp, dY, att, need_att=datt)
    again = run(op, Hp, dY, att, need_att=datt)
    assert r32["y"].dtype == torch.float32 and r32["dHp"].dtype == torch.float32
    assert same_bits(got["y"], r32["y"]), f"{tag}: Y"
    assert torch.equal(got["alpha"], r32["alpha"]), f"{tag}: alpha"
    assert same_bits(got["dHp"], r32["dHp"]), f"{tag}: dHp"
    if datt:
        assert got["datt"].dtype == torch.float32
        assert torch.equal(got["datt"], r32["datt"]), f"{tag}: datt"
    for k in ("y", "alpha", "dHp") + (("datt",) if datt else ()):
        assert torch.equal(got[k], again[k]), f"{tag}: {k} differs between two runs"
    assert not bits(got["y"][no_in]).any(), f"{tag}: Y of a row without in-edges"
    return got, r32


# ------------------------------------------------------------ soft attention
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "mask"])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("adir", ["in", "out"])
@pytest.mark.parametrize("H,C", WIDTHS)
def test_soft_attention_bits(cuda, H, C, adir, act, masked):
    from mgcn.ops import attention_aggregate
    _, _, plan, _ = graph()
    Hp, dY, att, mask, _ = inputs(H, C, 1000 * H + C)

    def op(h, a):
        return attention_aggregate(h, a, plan, H, act, adir, edge_mask=mask if masked else None)

    check_against_fp32(op, Hp, dY, att, f"soft.H{H}C{C}.{adir}.{act}")


# ------------------------------------------------------------ hard attention
@pytest.mark.parametrize("T", [0.1, 1.0])
@pytest.mark.parametrize("adir", ["in", "out"])
@pytest.mark.parametrize("H,C", WIDTHS)
def test_hard_attention_training_bits(cuda, H, C, adir, T):
    """Gumbel-softmax with replayed noise, under a mask."""
    from mgcn.ops import hard_attention_aggregate
    _, _, plan, _ = graph()
    Hp, dY, att, mask, noise = inputs(H, C, 2000 * H + C)

    def op(h, a):
        return hard_attention_aggregate(h, a, plan, H, "lrelu", adir, T, training=True,
                                        noise=noise, edge_mask=mask)

    check_against_fp32(op, Hp, dY, att, f"hard.H{H}C{C}.{adir}.T{T}")


@pytest.mark.parametrize("sample", [False, True], ids=["argmax", "sample"])
@pytest.mark.parametrize("adir", ["in", "out"])
@pytest.mark.parametrize("H,C", WIDTHS)
def test_hard_attention_eval_bits(cuda, H, C, adir, sample):
    """Eval: the one-hot is exact and equal to the fp32 path's, Y and dHp are
    its rounded rows, and att_weight gets no gradient."""
    from mgcn.ops import hard_attention_aggregate
    _, _, plan, _ = graph()
    Hp, dY, att, _, noise = inputs(H, C, 3000 * H + C)

    def op(h, a):
        return hard_attention_aggregate(h, a, plan, H, "lrelu", adir, training=False,
                                        noise=noise if sample else None)

    got, _ = check_against_fp32(op, Hp, dY, att, f"eval.H{H}C{C}.{adir}", datt=False)
    assert bool(((got["alpha"] == 0) | (got["alpha"] == 1)).all())
    got = run(op, Hp, dY, att, need_att=True)
    assert got["datt"] is None


# ------------------------------------------------------------------ layouts
SENTINEL = 12345.0
OFF, PAD = 1, 3  # an odd element offset, ld = H C + 3


def window(src, N, HC, dev):
    """A [N, HC] column window at element offset OFF of a sentinel-filled bf16
    [N, HC + PAD] buffer; ``src`` is copied into the window."""
    buf = torch.full((N, HC + PAD), SENTINEL, dtype=BF16, device=dev)
    win = buf[:, OFF:OFF + HC]
    assert win.stride(0) == HC + PAD and (win.data_ptr() - buf.data_ptr()) == 2 * OFF
    if src is not None:
        win.copy_(src)
    return buf, win


def padding_intact(buf, HC):
    cols = torch.ones(HC + PAD, dtype=torch.bool)
    cols[OFF:OFF + HC] = False
    return bool((buf[:, cols.to(buf.device)] == SENTINEL).all())


def replay_bf16(plan, Hp, att, mask, dY, H, C, act, adir):
    """ops._AttentionAggregate's bf16 launch sequence through the C ABI with
    Hp / Y / dY / dHp as windows.  ``mask`` is in fwd slot order."""
    import mgcn
    from mgcn import _lib as L
    lib = mgcn.load()
    dev = Hp.device
    N, nnz, HC = plan.num_nodes, plan.nnz, H * C
    fwd, bwd, slot = plan.fwd, plan.bwd, plan.slot_map()
    st = L.stream_of(dev)
    ptr = L.ptr
    (bHp, wHp), (bY, wY), (bdY, wdY), (bdHp, wdHp) = (
        window(src, N, HC, dev) for src in (Hp, None, dY, None))
    ld = HC + PAD

    def f32(*shape):
        return torch.empty(*shape, dtype=torch.float32, device=dev)
    s_src, s_dst, alpha = f32(N, H), f32(N, H), f32(nnz, H)
    L.check(lib.mgcn_att_scores_bf16(N, H, C, ptr(wHp), ld, ptr(att), ptr(s_src), ptr(s_dst), st),
            "mgcn_att_scores_bf16")
    inn = adir == "in"
    if inn:
        L.check(lib.mgcn_att_fwd_bf16(N, nnz, H, C, ptr(fwd.rowptr), ptr(fwd.col), ptr(s_dst),
                                      ptr(s_src), act, None, ptr(mask), ptr(wHp), ld, ptr(wY),
                                      ld, ptr(alpha), st), "mgcn_att_fwd_bf16")
    else:
        a_bwd = f32(nnz, H)
        L.check(lib.mgcn_edge_softmax(N, nnz, H, ptr(bwd.rowptr), ptr(bwd.col), ptr(s_src),
                                      ptr(s_dst), act, ptr(a_bwd), st), "mgcn_edge_softmax")
        alpha[slot[:nnz].long()] = a_bwd
        L.check(lib.mgcn_att_fwd_bf16(N, nnz, H, C, ptr(fwd.rowptr), ptr(fwd.col), None, None,
                                      act, ptr(alpha), ptr(mask), ptr(wHp), ld, ptr(wY), ld,
                                      None, st), "mgcn_att_fwd_bf16")
    dz, ds_src, ds_dst = f32(nnz, H), f32(N, H), f32(N, H)
    park = None if inn else f32(N, HC)
    L.check(lib.mgcn_att_bwd_dst_bf16(N, nnz, H, C, ptr(fwd.rowptr), ptr(fwd.col), ptr(wHp), ld,
                                      ptr(wdY), ld, ptr(alpha), ptr(mask), ptr(s_dst),
                                      ptr(s_src), act, int(inn), ptr(dz), ptr(ds_dst), st),
            "mgcn_att_bwd_dst_bf16")
    L.check(lib.mgcn_att_bwd_src_bf16(N, nnz, H, C, ptr(bwd.rowptr), ptr(bwd.col), ptr(slot),
                                      ptr(wdY), ld, ptr(alpha), ptr(mask), ptr(dz), ptr(s_src),
                                      ptr(s_dst), act, int(not inn), ptr(att),
                                      ptr(ds_dst) if inn else None, ptr(ds_src), ptr(wdHp), ld,
                                      ptr(park), st), "mgcn_att_bwd_src_bf16")
    if not inn:
        # the parked launch leaves dHp alone: the window still holds the sentinel
        assert bool((bdHp == SENTINEL).all())
        L.check(lib.mgcn_att_dst_fold_bf16(N, nnz, H, C, ptr(fwd.rowptr), ptr(dz), ptr(att),
                                           ptr(ds_dst), ptr(park), ptr(wdHp), ld, st),
                "mgcn_att_dst_fold_bf16")
    torch.cuda.synchronize(dev)
    return {"Y": wY, "alpha": alpha, "dHp": wdHp, "buffers": (bHp, bY, bdY, bdHp)}


@pytest.mark.parametrize("adir", ["in", "out"])
@pytest.mark.parametrize("H,C", [(5, 13), (3, 43), (2, 64)])
def test_windows_at_odd_offsets(cuda, H, C, adir):
    """Hp / dY as column windows at an odd element offset with ld = H C + 3
    through the public op, and all four row arrays as such windows through the
    C ABI: the bits of the compact call, every padding element untouched."""
    from mgcn import _lib as L
    from mgcn.ops import attention_aggregate
    ei, N, plan, _ = graph()
    HC = H * C
    Hp, dY, att, mask, _ = inputs(H, C, 4000 * H + C)

    def op(h, a):
        return attention_aggregate(h, a, plan, H, "lrelu", adir, edge_mask=mask)

    flat = run(op, Hp, dY, att)
    bHp, wHp = window(Hp, N, HC, cuda)
    bdY, wdY = window(dY, N, HC, cuda)
    leaf = wHp.detach().requires_grad_(True)  # a view of the buffer: consumed in place
    assert leaf.data_ptr() == wHp.data_ptr() and leaf.stride(0) == HC + PAD
    a = att.clone().requires_grad_(True)
    y, alpha = op(leaf, a)
    y.backward(wdY)
    for name, t, want in (("Y", y, flat["y"]), ("alpha", alpha, flat["alpha"]),
                          ("dHp", leaf.grad, flat["dHp"]), ("datt", a.grad, flat["datt"])):
        assert torch.equal(t.detach(), want), name
    assert padding_intact(bHp, HC) and padding_intact(bdY, HC)

    mask_slot = mask[plan.fwd.eid.long()].contiguous()
    att2 = att.reshape(H, 2 * C).contiguous()
    wide = replay_bf16(plan, Hp, att2, mask_slot, dY, H, C, L.ATT_ACT_CODES["lrelu"], adir)
    assert torch.equal(bits(wide["Y"]), bits(flat["y"]))
    assert torch.equal(bits(wide["dHp"]), bits(flat["dHp"]))
    coo = torch.empty_like(flat["alpha"])
    coo[plan.fwd.eid.long()] = wide["alpha"] * mask_slot
    assert torch.equal(coo, flat["alpha"])
    for buf, name in zip(wide["buffers"], ("Hp", "Y", "dY", "dHp")):
        assert padding_intact(buf, HC), f"{name}: a padding element was written"


def test_hard_gather_window(cuda):
    """mgcn_hatt_gather_bf16 with windowed Hp and Y: the bits of
    mgcn_att_fwd_bf16 in its aggregate-only mode on compact rows."""
    import mgcn
    from mgcn import _lib as L
    lib = mgcn.load()
    _, N, plan, _ = graph()
    H, C = 5, 13
    HC, nnz, fwd = H * C, plan.nnz, plan.fwd
    Hp, _, _, _, _ = inputs(H, C, 77)
    g = torch.Generator().manual_seed(8)
    alpha = (torch.rand(nnz, H, generator=g) * (torch.rand(nnz, H, generator=g) < 0.3)).cuda()
    st = L.stream_of(cuda)
    dense = torch.empty(N, HC, dtype=BF16, device=cuda)
    L.check(lib.mgcn_att_fwd_bf16(N, nnz, H, C, L.ptr(fwd.rowptr), L.ptr(fwd.col), None, None, 0,
                                  L.ptr(alpha), None, L.ptr(Hp), HC, L.ptr(dense), HC, None, st),
            "mgcn_att_fwd_bf16")
    bHp, wHp = window(Hp, N, HC, cuda)
    bY, wY = window(None, N, HC, cuda)
    L.check(lib.mgcn_hatt_gather_bf16(N, nnz, H, C, L.ptr(fwd.rowptr), L.ptr(fwd.col),
                                      L.ptr(alpha), L.ptr(wHp), HC + PAD, L.ptr(wY), HC + PAD,
                                      st), "mgcn_hatt_gather_bf16")
    torch.cuda.synchronize(cuda)
    assert torch.equal(bits(wY), bits(dense))
    assert padding_intact(bHp, HC) and padding_intact(bY, HC)


# ------------------------------------------------------------------ modules
@pytest.mark.parametrize("converted", [False, True], ids=["fp32-masters", "to-bf16"])
@pytest.mark.parametrize("combine", ["cat", "add", "mean"])
@pytest.mark.parametrize("hard", [False, True], ids=["soft", "hard"])
def test_node_model_on_bf16_input(cuda, hard, combine, converted):
    """The module's output is bf16 and is the head combine and the bias
    accumulated in fp32 from the op's bf16 Y, rounded once; parameter
    gradients have the parameters' dtype."""
    from mgcn.models import NodeModelAttention, NodeModelHardAttention
    from mgcn.ops import attention_aggregate, hard_attention_aggregate, linear
    ei, N, plan, _ = graph()
    H, fin, fout = 3, 10, 12
    torch.manual_seed(11)
    cls = NodeModelHardAttention if hard else NodeModelAttention
    nm = cls(fin, fout, nheads=H, att_act="lrelu", att_combine=combine, bias=True).cuda()
    with torch.no_grad():
        nm.bias.copy_(torch.randn(fout))
    nm.eval()  # hard: argmax, no noise drawn; soft: no dropout
    if converted:
        nm = nm.to(BF16)
    pdt = BF16 if converted else torch.float32
    g = torch.Generator().manual_seed(12)
    x = torch.randn(N, fin, generator=g).to(BF16).cuda().requires_grad_(True)
    y = nm(x, ei)
    assert y.dtype == BF16 and y.shape == (N, fout)
    with torch.no_grad():
        hp = linear(x, nm.weight)
        assert hp.dtype == BF16
        if hard:
            yo, _ = hard_attention_aggregate(hp, nm.att_weight, plan, H, "lrelu", "in",
                                             nm.temperature, training=False)
        else:
            yo, _ = attention_aggregate(hp, nm.att_weight, plan, H, "lrelu", "in")
        assert yo.dtype == BF16
        f = yo.float()
        if combine == "add":
            f = f.view(N, H, -1).sum(dim=1)
        elif combine == "mean":
            f = f.view(N, H, -1).mean(dim=1)
        want = (f + nm.bias.float()).to(BF16)
    assert torch.equal(bits(y), bits(want))
    y.backward(torch.randn(N, fout, generator=g).to(BF16).cuda())
    assert x.grad.dtype == BF16 and bool(torch.isfinite(x.grad.float()).all())
    for name, p in nm.named_parameters():
        assert p.dtype == pdt, name
        if hard and name == "att_weight":
            assert p.grad is None  # eval: nothing flows to the attention vector
            continue
        assert p.grad is not None and p.grad.dtype == pdt, name
        assert bool(torch.isfinite(p.grad.float()).all()) and float(p.grad.float().abs().sum()) > 0


@pytest.mark.parametrize("converted", [False, True], ids=["fp32-masters", "to-bf16"])
def test_citation_model_runs_on_bf16_input(cuda, converted):
    """The citation configuration, three attention layers, forward and backward
    on bf16 input, layer by layer."""
    from mgcn.models import GCNModel
    ei, N, _, _ = graph()
    torch.manual_seed(21)
    model = GCNModel(24, [32, 32, 7], 7, nodemodel="attention", nheads=[2, 2, 1], dropout=0.0,
                     att_act="lrelu", att_dropout=0.0).cuda()
    if converted:
        model = model.to(BF16)
    pdt = BF16 if converted else torch.float32
    g = torch.Generator().manual_seed(22)
    x = torch.randn(N, 24, generator=g).to(BF16).cuda().requires_grad_(True)
    y = model(x, ei)
    assert y.dtype == BF16 and y.shape == (N, 7) and bool(torch.isfinite(y.float()).all())
    y.backward(torch.randn(N, 7, generator=g).to(BF16).cuda())
    assert x.grad.dtype == BF16 and bool(torch.isfinite(x.grad.float()).all())
    params = dict(model.named_parameters())
    assert sum(k.endswith("att_weight") for k in params) == 3
    for name, p in params.items():
        assert p.grad is not None and p.grad.dtype == p.dtype == pdt, name
        assert bool(torch.isfinite(p.grad.float()).all()), name


# ------------------------------------------------------------------ routing
def record_names(fn):
    from mgcn import ops
    names = []
    ops.set_kernel_timer(lambda name, start, rows=None, edges=None: names.append(name))
    try:
        fn()
    finally:
        ops.set_kernel_timer(None)
    return set(names)


@pytest.mark.parametrize("adir", ["in", "out"])
def test_routing_by_row_dtype(cuda, adir):
    """An fp32 call records no ``_bf16`` launch; a bf16 call records no fp32
    launch that touches a feature row, and every bf16 sibling it should."""
    from mgcn.ops import attention_aggregate, hard_attention_aggregate
    _, _, plan, _ = graph()
    H, C = 3, 4
    Hp, dY, att, mask, noise = inputs(H, C, 5)

    def soft(h, a):
        return attention_aggregate(h, a, plan, H, "lrelu", adir, edge_mask=mask)

    def train(h, a):
        return hard_attention_aggregate(h, a, plan, H, "lrelu", adir, 0.5, training=True,
                                        noise=noise)

    def evalu(h, a):
        return hard_attention_aggregate(h, a, plan, H, "lrelu", adir, training=False)

    fold = set() if adir == "in" else {"att_dst_fold"}
    expect = {
        soft: {"att_scores", "att_fwd", "att_bwd_dst", "att_bwd_src"} | fold,
        train: {"att_scores", "hatt_fwd", "hatt_bwd_dst", "hatt_bwd_src"} | fold,
        evalu: {"att_scores", "hatt_gather", "att_bwd_src"},
    }
    for op, rows in expect.items():
        n32 = record_names(lambda: run(op, Hp.float(), dY.float(), att, need_att=op is not evalu))
        assert rows <= n32 and not [n for n in n32 if n.endswith("_bf16")]
        nbf = record_names(lambda: run(op, Hp, dY, att, need_att=op is not evalu))
        assert not nbf & FP32_ROW_LAUNCHES, nbf & FP32_ROW_LAUNCHES
        assert {n + "_bf16" for n in rows} <= nbf
        # the launches that see fp32 scores alone are shared
        assert {n for n in n32 if n.endswith(("edge_softmax", "hatt_select"))} == \
            {n for n in nbf if n.endswith(("edge_softmax", "hatt_select"))}
