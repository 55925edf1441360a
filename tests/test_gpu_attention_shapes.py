"""The attention kernels (csrc/attention.hip) along their own branch structure
(MI355X): every FPL instantiation, every head count 1..16 with a row on each
edge of the flat chunk, rows past the launch's first grid-stride trip, leading
dimensions above H C at the C ABI, the activation's derivative at z = 0, and
the values that are exact.

Every comparison with a reference uses attention_ref.check,

    max|t_gpu - t64| <= max(4 * max|t32 - t64|, 1e-5 * max|t64|)

with t32 / t64 the torch restatement (attention_ref.att_ref) run on the CPU in
fp32 and fp64; comparisons of one kernel run with another are bitwise
(torch.equal).
"""
import numpy as np
import pytest
import torch

from attention_ref import (att_ref, check, degree_graph, gpu_run, ladder_graph, make_node_model,
                           ref_run)

pytestmark = pytest.mark.gpu

KEYS = ("y", "alpha", "dx", "dW", "datt")


def node_model_case(cuda, tag, ei, N, fin, H, C, adir, act, bias, seed):
    """One NodeModelAttention ('cat') forward + backward against the
    restatement: y, alpha (attn_store), dx, dW, datt, db."""
    torch.manual_seed(seed)
    nm = make_node_model(cuda, fin, H * C, H, "cat", adir, act, bias)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, fin, generator=g)
    dY = torch.randn(N, H * C, generator=g)
    W, att = nm.weight.detach().cpu(), nm.att_weight.detach().cpu()
    b = None if nm.bias is None else nm.bias.detach().cpu()
    r32 = ref_run(x, W, att, b, ei, dY, H, "cat", adir, act, torch.float32)
    r64 = ref_run(x, W, att, b, ei, dY, H, "cat", adir, act, torch.float64)
    got = gpu_run(nm, x.to(cuda), ei.to(cuda), dY.to(cuda))
    assert got["alpha"].shape == (ei.size(1), H)
    for k in KEYS + (("db",) if bias else ()):
        check(f"{tag}.{k}", got[k], r32[k], r64[k])
    return nm, x, got, r32, r64


def op_ref(x, W, att, ei, dY, H, adir, act, mask, dtype):
    """Autograd of the restatement under an edge mask."""
    xs, Ws, As = (t.detach().clone().to(dtype).requires_grad_(True) for t in (x, W, att))
    y, alpha, _ = att_ref(xs, Ws, As, None, ei, H, "cat", adir, act, mask=mask)
    y.backward(dY.to(dtype))
    return {"y": y.detach(), "alpha": alpha.detach(), "dx": xs.grad, "dW": Ws.grad,
            "datt": As.grad}


def op_run(cuda, x, W, att, ei, N, dY, H, adir, act, mask, need=("x", "W", "att")):
    """ops.linear + ops.attention_aggregate forward + backward; ``need`` names
    the leaves that require a gradient."""
    from mgcn.graph import plan_for
    from mgcn.ops import attention_aggregate, linear
    xs, Ws, As = (t.detach().to(cuda).requires_grad_(n in need)
                  for t, n in ((x, "x"), (W, "W"), (att, "att")))
    y, alpha = attention_aggregate(linear(xs, Ws), As, plan_for(ei.to(cuda), N), H, act, adir,
                                   edge_mask=None if mask is None else mask.to(cuda))
    assert not alpha.requires_grad
    y.backward(dY.to(cuda))
    return {"y": y.detach(), "alpha": alpha, "dx": xs.grad, "dW": Ws.grad, "datt": As.grad}


# ---------------------------------------------------------- a. dispatch sweep
# ATT_DISPATCH picks FPL = 1 / 2 / 4 / 8 / 16 from ceil(H C / 64)
SWEEP = [
    # FPL 1: hpi = 1; pow2 C with non-pow2 H; nothing pow2
    (1, 64), (3, 16), (7, 9),
    # FPL 2: width 65; head 2 alone in register 1; pow2 C > 64 takes the generic branch
    (5, 13), (3, 32), (1, 128),
    # FPL 4: widths 129 / 256 / 256 / 192; 4 heads per register
    (3, 43), (4, 64), (16, 16), (12, 16),
    # FPL 8: widths 257 / 512 / 512 / 352
    (1, 257), (8, 64), (16, 32), (11, 32),
    # FPL 16: width 513; pow2 C = 512; 900
    (1, 513), (2, 512), (9, 100),
]
SWEEP_FPL = [1] * 3 + [2] * 3 + [4] * 4 + [8] * 4 + [16] * 3
SWEEP_CASES = [(H, C, adir, ("none", "lrelu", "relu")[i % 3], i % 2 == 0)
               for i, (H, C) in enumerate(SWEEP) for adir in ("in", "out")]


def test_sweep_reaches_every_instantiation():
    def fpl(hc):
        return next(f for f in (1, 2, 4, 8, 16) if (hc + 63) // 64 <= f)
    assert [fpl(H * C) for H, C in SWEEP] == SWEEP_FPL


@pytest.mark.parametrize("H,C,adir,act,bias", SWEEP_CASES)
def test_dispatch_sweep(cuda, H, C, adir, act, bias):
    ei, N = degree_graph()
    node_model_case(cuda, f"sweep.H{H}C{C}{adir}{act}", ei, N, 12, H, C, adir, act, bias,
                    seed=1000 * H + C)


# ------------------------------------- b. head counts on a degree ladder
def zero_group_mask(ei, H, adir, node, keep, scale, g):
    """Bernoulli(keep) * scale over [E, H], every entry of ``node``'s softmax
    group forced to 0."""
    idx = ei[0] if adir == "out" else ei[1]
    mask = (torch.rand(ei.size(1), H, generator=g) < keep).float() * scale
    mask[idx == node] = 0
    return mask, idx == node


@pytest.mark.parametrize("adir", ["in", "out"])
@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("H", range(1, 17))
def test_head_count_ladder(cuda, H, C, adir):
    """The flat layout has G = 64 // H slots per chunk and 64 - G H idle
    lanes; the ladder has a row of degree G - 1, G, G + 1 for every H.  Odd H:
    also under an edge mask (keep 1/4, scale 4) through the op, with the whole
    group of the ladder row of degree G + 1 masked out."""
    ei, N = ladder_graph()
    fin = 6
    tag = f"ladder.H{H}C{C}{adir}"
    nm = node_model_case(cuda, tag, ei, N, fin, H, C, adir, "lrelu", False,
                         seed=100 * H + C)[0]
    if H % 2 == 0:
        return
    G = 64 // H
    node = G + 1 if adir == "in" else 67 + G + 1
    g = torch.Generator().manual_seed(7 * H + C)
    mask, group = zero_group_mask(ei, H, adir, node, 0.25, 4.0, g)
    assert int(group.sum()) == G + 1
    x = torch.randn(N, fin, generator=g)
    dY = torch.randn(N, H * C, generator=g)
    W, att = nm.weight.detach().cpu(), nm.att_weight.detach().cpu()
    r32 = op_ref(x, W, att, ei, dY, H, adir, "lrelu", mask, torch.float32)
    r64 = op_ref(x, W, att, ei, dY, H, adir, "lrelu", mask, torch.float64)
    got = op_run(cuda, x, W, att, ei, N, dY, H, adir, "lrelu", mask)
    for k in KEYS:
        check(f"{tag}.mask.{k}", got[k], r32[k], r64[k])


# ------------------------------------------------------ c. grid-stride trips
# att_grid's cap (4096 workgroups) x kAttWaves (4 waves, one row each): the
# rows one launch covers in its first grid-stride trip
GRID_WAVES = 4096 * 4
_STRIDE = {}


def stride_graph():
    """N = 2 * GRID_WAVES + 37 (some waves take a third row), E = 3 N uniform
    random edges, and two hubs with 200 more in-edges and 200 more out-edges
    each, one on the second trip and one on the third."""
    if not _STRIDE:
        rng = np.random.default_rng(1)
        N = 2 * GRID_WAVES + 37
        parts = [rng.integers(0, N, (2, 3 * N))]
        for hub in (GRID_WAVES + 5001, N - 3):
            parts.append(np.stack([rng.integers(0, N, 200), np.full(200, hub)]))
            parts.append(np.stack([np.full(200, hub), rng.integers(0, N, 200)]))
        ei = np.concatenate(parts, axis=1)
        ei = ei[:, rng.permutation(ei.shape[1])]
        _STRIDE["ei"] = torch.from_numpy(ei.astype(np.int64))
        _STRIDE["N"] = N
    return _STRIDE["ei"], _STRIDE["N"]


def logits64(x, W, att, ei, H):
    """z [E, H] of the restatement in fp64."""
    hp = (x.double() @ W.double()).view(x.size(0), H, -1)
    return (torch.cat([hp[ei[0]], hp[ei[1]]], dim=-1) * att.double()).sum(-1)


@pytest.mark.parametrize("H,C,adir,act", [(2, 8, "in", "lrelu"), (3, 5, "out", "relu"),
                                          (16, 4, "in", "none")])
def test_grid_stride_trips(cuda, H, C, adir, act):
    """Rows >= GRID_WAVES are a wave's second and third row: per-row state
    (m, denom, acc, S, part) must not carry over.  Y of a row without in-edges
    is exactly 0 (no bias).

    With 1e5 edges some |z| comes within fp32 rounding (~1e-7) of 0, where an
    activation with a kink has two derivatives: the fp32 restatement then
    takes the other side than fp64 and its error, which sets the bound, jumps
    from 3e-6 to 7e-3 (seen with H = 16, 1.6e6 logits, min|z| = 1.3e-8).  So
    H = 16 runs without activation and the other two assert min|z| > 1e-6."""
    ei, N = stride_graph()
    ind = torch.bincount(ei[1], minlength=N)
    outd = torch.bincount(ei[0], minlength=N)
    G = 64 // H
    for lo in (GRID_WAVES, 2 * GRID_WAVES):  # the second and the third trip
        assert ind[lo:].max() > G and outd[lo:].max() > G
    late_zero_in = int((ind[GRID_WAVES:] == 0).sum())
    print(f"stride graph: {late_zero_in} rows >= {GRID_WAVES} without in-edges, "
          f"{int((outd[GRID_WAVES:] == 0).sum())} without out-edges")
    assert late_zero_in > 0 and (outd[GRID_WAVES:] == 0).any()
    nm, x, got, _, _ = node_model_case(cuda, f"stride.H{H}C{C}{adir}", ei, N, 6, H, C, adir, act,
                                       False, seed=50 * H + C)
    if act != "none":
        z64 = logits64(x, nm.weight.detach().cpu(), nm.att_weight.detach().cpu(), ei, H)
        assert z64.abs().min().item() > 1e-6
    assert torch.count_nonzero(got["y"][(ind == 0).to(cuda)]) == 0


# -------------------------------------- d. leading dimensions at the C ABI
SENTINEL = 12345.0


def window(src, N, HC, pad, dev):
    """A [N, HC] column window (from column pad // 2) of a [N, HC + pad] buffer
    filled with the sentinel; ``src`` is copied into the window."""
    buf = torch.full((N, HC + pad), SENTINEL, dtype=torch.float32, device=dev)
    win = buf[:, pad // 2:pad // 2 + HC]
    if src is not None:
        win.copy_(src)
    return buf, win


def padding_intact(buf, HC, pad):
    cols = torch.ones(HC + pad, dtype=torch.bool)
    cols[pad // 2:pad // 2 + HC] = False
    return bool((buf[:, cols.to(buf.device)] == SENTINEL).all())


def replay(plan, Hp, att, mask, dY, H, C, act, adir, pads):
    """The launch sequence of ops._AttentionAggregate (forward and backward)
    through the C ABI, with Hp / Y / dY / dHp as column windows of buffers
    ``pads`` columns wider than H C.  ``mask`` is in fwd slot order."""
    import mgcn
    from mgcn import _lib as L
    lib = mgcn.load()
    dev = Hp.device
    N, nnz, HC = plan.num_nodes, plan.nnz, H * C
    fwd, bwd, slot = plan.fwd, plan.bwd, plan.slot_map()
    st = L.stream_of(dev)
    ptr = L.ptr
    (bHp, wHp), (bY, wY), (bdY, wdY), (bdHp, wdHp) = (
        window(src, N, HC, pad, dev) for src, pad in zip((Hp, None, dY, None), pads))
    ldh, ldy, lddy, lddh = (w.stride(0) for w in (wHp, wY, wdY, wdHp))
    assert (ldh, ldy, lddy, lddh) == tuple(HC + p for p in pads)

    def f32(*shape):
        return torch.empty(*shape, dtype=torch.float32, device=dev)
    s_src, s_dst, alpha = f32(N, H), f32(N, H), f32(nnz, H)
    L.check(lib.mgcn_att_scores(N, H, C, ptr(wHp), ldh, ptr(att), ptr(s_src), ptr(s_dst), st),
            "mgcn_att_scores")
    inn = adir == "in"
    if inn:
        L.check(lib.mgcn_att_fwd(N, nnz, H, C, ptr(fwd.rowptr), ptr(fwd.col), ptr(s_dst),
                                 ptr(s_src), act, None, ptr(mask), ptr(wHp), ldh, ptr(wY), ldy,
                                 ptr(alpha), st), "mgcn_att_fwd")
    else:
        a_bwd = f32(nnz, H)
        L.check(lib.mgcn_edge_softmax(N, nnz, H, ptr(bwd.rowptr), ptr(bwd.col), ptr(s_src),
                                      ptr(s_dst), act, ptr(a_bwd), st), "mgcn_edge_softmax")
        alpha[slot[:nnz].long()] = a_bwd
        L.check(lib.mgcn_att_fwd(N, nnz, H, C, ptr(fwd.rowptr), ptr(fwd.col), None, None, act,
                                 ptr(alpha), ptr(mask), ptr(wHp), ldh, ptr(wY), ldy, None, st),
                "mgcn_att_fwd")
    dz, ds_src, ds_dst = f32(nnz, H), f32(N, H), f32(N, H)
    L.check(lib.mgcn_att_bwd_dst(N, nnz, H, C, ptr(fwd.rowptr), ptr(fwd.col), ptr(wHp), ldh,
                                 ptr(wdY), lddy, ptr(alpha), ptr(mask), ptr(s_dst), ptr(s_src),
                                 act, int(inn), ptr(dz), ptr(ds_dst), st), "mgcn_att_bwd_dst")
    L.check(lib.mgcn_att_bwd_src(N, nnz, H, C, ptr(bwd.rowptr), ptr(bwd.col), ptr(slot), ptr(wdY),
                                 lddy, ptr(alpha), ptr(mask), ptr(dz), ptr(s_src), ptr(s_dst),
                                 act, int(not inn), ptr(att), ptr(ds_dst) if inn else None,
                                 ptr(ds_src), ptr(wdHp), lddh, st), "mgcn_att_bwd_src")
    if not inn:
        L.check(lib.mgcn_att_dst_fold(N, nnz, H, C, ptr(fwd.rowptr), ptr(dz), ptr(att),
                                      ptr(ds_dst), ptr(wdHp), lddh, st), "mgcn_att_dst_fold")
    torch.cuda.synchronize(dev)
    return {"Y": wY, "alpha": alpha, "ds_src": ds_src, "ds_dst": ds_dst, "dHp": wdHp,
            "buffers": (bHp, bY, bdY, bdHp)}


def ld_inputs(cuda, H, C, N, E, seed):
    g = torch.Generator().manual_seed(seed)
    Hp = torch.randn(N, H * C, generator=g).to(cuda)
    att = (torch.randn(1, H, 2 * C, generator=g) * 0.5).to(cuda)
    dY = torch.randn(N, H * C, generator=g).to(cuda)
    mask = ((torch.rand(E, H, generator=g) < 0.5).float() * 2).to(cuda)
    return Hp, att, dY, mask


@pytest.mark.parametrize("adir", ["in", "out"])
@pytest.mark.parametrize("H,C", [(3, 5), (4, 64)])
def test_leading_dimensions_c_abi(cuda, H, C, adir):
    """ldh, ldy, lddy, lddh = H C + 3, + 5, + 7, + 11 (no two agree): the same
    kernels in the same order, so Y, alpha, ds_src, ds_dst and dHp are the
    bits of the compact run, and no padding column is touched."""
    from mgcn import _lib as L
    from mgcn.graph import plan_for
    from mgcn.ops import attention_aggregate, gemm_tn
    ei, N = degree_graph()
    HC = H * C
    eig = ei.to(cuda)
    plan = plan_for(eig, N)
    Hp, att, dY, mask = ld_inputs(cuda, H, C, N, ei.size(1), 40 + H)
    Hp.requires_grad_(True)
    att.requires_grad_(True)
    y, alpha_coo = attention_aggregate(Hp, att, plan, H, "lrelu", adir, edge_mask=mask)
    y.backward(dY)
    eid = plan.fwd.eid.long()
    mask_slot = mask[eid].contiguous()
    att2 = att.detach().reshape(H, 2 * C).contiguous()
    act = L.ATT_ACT_CODES["lrelu"]
    pads = (3, 5, 7, 11)
    flat = replay(plan, Hp.detach(), att2, mask_slot, dY, H, C, act, adir, (0, 0, 0, 0))
    wide = replay(plan, Hp.detach(), att2, mask_slot, dY, H, C, act, adir, pads)
    for k in ("Y", "alpha", "ds_src", "ds_dst", "dHp"):
        assert torch.equal(wide[k], flat[k]), k
    for buf, pad, name in zip(wide["buffers"], pads, ("Hp", "Y", "dY", "dHp")):
        assert padding_intact(buf, HC, pad), f"{name}: a padding column was written"
    # ... and of the public op's compact run (datt is its gemm over ds_src | ds_dst)
    assert torch.equal(wide["Y"], y.detach())
    coo = torch.empty_like(alpha_coo)
    coo[eid] = wide["alpha"] * mask_slot
    assert torch.equal(coo, alpha_coo)
    assert torch.equal(wide["dHp"], Hp.grad)
    full = gemm_tn(torch.cat([wide["ds_src"], wide["ds_dst"]], dim=1), Hp.detach())
    full = full.view(2, H, H, C)
    hh = torch.arange(H, device=cuda)
    datt = torch.cat([full[0, hh, hh], full[1, hh, hh]], dim=1)
    assert torch.equal(datt, att.grad.reshape(H, 2 * C))


@pytest.mark.parametrize("adir", ["in", "out"])
def test_leading_dimensions_public_op(cuda, adir):
    """Hp as a column window of a wider tensor and a row-strided upstream
    gradient pass through the op without a copy (ops._contig_f32): bitwise the
    compact result."""
    from mgcn.graph import plan_for
    from mgcn.ops import attention_aggregate
    ei, N = degree_graph()
    H, C = 3, 5
    HC = H * C
    plan = plan_for(ei.to(cuda), N)
    Hp, att, dY, mask = ld_inputs(cuda, H, C, N, ei.size(1), 77)

    def run(hp_leaf, hp, consumer):
        a = att.clone().requires_grad_(True)
        seen = []
        y, alpha = attention_aggregate(hp, a, plan, H, "lrelu", adir, edge_mask=mask)
        y.register_hook(lambda gr: seen.append(gr.stride()))
        consumer(y)
        return y.detach(), alpha, hp_leaf.grad, a.grad, seen[0]

    hp0 = Hp.clone().requires_grad_(True)
    y0, a0, dhp0, datt0, s0 = run(hp0, hp0, lambda y: y.backward(dY))
    assert s0 == (HC, 1)

    y_wide_buffer = torch.full((N, HC + 6), SENTINEL, device=cuda)
    y_wide_buffer[:, :HC] = dY
    consumers = {
        "product": lambda y: (y_wide_buffer[:, :HC] * y).sum().backward(),
        "strided": lambda y: y.backward(y_wide_buffer[:, :HC]),
    }
    for name, consumer in consumers.items():
        wide = torch.full((N, HC + 5), SENTINEL, device=cuda)
        wide[:, 2:2 + HC] = Hp
        wide.requires_grad_(True)
        hp = wide[:, 2:2 + HC]
        assert hp.stride() == (HC + 5, 1)
        y1, a1, dwide, datt1, s1 = run(wide, hp, consumer)
        if name == "strided":
            assert s1 == (HC + 6, 1)  # the op did receive a row-strided dY
        assert torch.equal(y1, y0) and torch.equal(a1, a0), name
        assert torch.equal(dwide[:, 2:2 + HC], dhp0), name
        assert torch.count_nonzero(dwide[:, :2]) == 0 and torch.count_nonzero(dwide[:, 2 + HC:]) == 0
        assert torch.equal(datt1, datt0), name


# ------------------------------------------- e. activation kink, z = 0 exactly
_KINK = {}


def kink_graph():
    """N = 96, nodes 0..23 'zero' (their x rows are 0), the rest live: 500
    edges among live nodes, 120 zero -> zero, 150 live -> zero, 150 zero ->
    live, shuffled."""
    if not _KINK:
        rng = np.random.default_rng(5)

        def part(src, dst, n):
            return np.stack([rng.integers(*src, n), rng.integers(*dst, n)])
        zero, live = (0, 24), (24, 96)
        ei = np.concatenate([part(live, live, 500), part(zero, zero, 120), part(live, zero, 150),
                             part(zero, live, 150)], axis=1)
        ei = ei[:, rng.permutation(ei.shape[1])]
        _KINK["ei"] = torch.from_numpy(ei.astype(np.int64))
    return _KINK["ei"], 96


@pytest.mark.parametrize("adir", ["in", "out"])
@pytest.mark.parametrize("act", ["relu", "lrelu"])
def test_activation_kink(cuda, act, adir):
    """att_act_grad takes the negative side at z == 0, as torch's relu /
    leaky_relu backward.  Head 0's source half of the attention vector is 0,
    so z of head 0 is exactly 0 on each of the 270 edges into a zero node; the
    other side would move dx and datt by 1e4 times the bound."""
    ei, N = kink_graph()
    H, C, fin = 3, 5, 7
    torch.manual_seed(17)
    nm = make_node_model(cuda, fin, H * C, H, "cat", adir, act, False)
    nm.att_weight.data[0, 0, :C] = 0
    g = torch.Generator().manual_seed(18)
    x = torch.randn(N, fin, generator=g)
    x[:24] = 0
    dY = torch.randn(N, H * C, generator=g)
    W, att = nm.weight.detach().cpu(), nm.att_weight.detach().cpu()
    z64 = logits64(x, W, att, ei, H)
    assert int((z64[:, 0] == 0).sum()) >= 200
    assert int((z64[:, 1:] == 0).sum()) == 120 * (H - 1)  # zero -> zero: every head
    r32 = ref_run(x, W, att, None, ei, dY, H, "cat", adir, act, torch.float32)
    r64 = ref_run(x, W, att, None, ei, dY, H, "cat", adir, act, torch.float64)
    got = gpu_run(nm, x.to(cuda), ei.to(cuda), dY.to(cuda))
    for k in KEYS:
        check(f"kink.{act}.{adir}.{k}", got[k], r32[k], r64[k])


# ------------------------------------------------------------ f. exact values
@pytest.mark.parametrize("adir", ["in", "out"])
@pytest.mark.parametrize("H", [3, 8])
def test_exact_single_member_and_bias(cuda, H, adir):
    """alpha of a one-member softmax group is exp(0) / (1 + 1e-16) = 1.0 in
    fp32, bit for bit (the fp32 restatement gives exactly 1 too); Y of a row
    without in-edges is the bias, bit for bit."""
    ei, N = ladder_graph()
    C = 4
    nm, _, got, r32, _ = node_model_case(cuda, f"exact.H{H}{adir}", ei, N, 6, H, C, adir,
                                         "lrelu", True, seed=900 + H)
    idx = ei[0] if adir == "out" else ei[1]
    single = torch.bincount(idx, minlength=N)[idx] == 1
    assert single.any()
    one = torch.ones(int(single.sum()), H)
    assert torch.equal(r32["alpha"][single], one)
    assert torch.equal(got["alpha"].cpu()[single], one)
    no_in = torch.bincount(ei[1], minlength=N) == 0
    assert int(no_in.sum()) >= 68
    rows = got["y"][no_in.to(cuda)]
    assert torch.equal(rows, nm.bias.detach().expand_as(rows))


def ladder_op_inputs(H, C, adir, seed):
    ei, N = ladder_graph()
    g = torch.Generator().manual_seed(seed)
    fin = 6
    x = torch.randn(N, fin, generator=g)
    W = torch.randn(fin, H * C, generator=g) * 0.3
    att = torch.randn(1, H, 2 * C, generator=g) * 0.5
    dY = torch.randn(N, H * C, generator=g)
    node = 40 if adir == "in" else 67 + 40
    mask, group = zero_group_mask(ei, H, adir, node, 0.25, 4.0, g)
    assert int(group.sum()) == 40
    return ei, N, x, W, att, dY, mask, group


@pytest.mark.parametrize("adir", ["in", "out"])
def test_exact_zero_mask_group_and_grad_subsets(cuda, adir):
    """The alpha' rows of a fully masked group are bitwise 0.  The op run with
    only x, or only the parameters, requiring a gradient gives the bits of the
    run with both for what it computes, and None for what it does not."""
    H, C = 5, 4
    ei, N, x, W, att, dY, mask, group = ladder_op_inputs(H, C, adir, 61)
    both = op_run(cuda, x, W, att, ei, N, dY, H, adir, "lrelu", mask)
    assert torch.count_nonzero(both["alpha"][group.to(cuda)]) == 0
    assert torch.count_nonzero(both["alpha"]) > 0
    only_x = op_run(cuda, x, W, att, ei, N, dY, H, adir, "lrelu", mask, need=("x",))
    only_p = op_run(cuda, x, W, att, ei, N, dY, H, adir, "lrelu", mask, need=("W", "att"))
    for k in ("y", "alpha"):
        assert torch.equal(only_x[k], both[k]) and torch.equal(only_p[k], both[k]), k
    assert torch.equal(only_x["dx"], both["dx"])
    assert only_x["dW"] is None and only_x["datt"] is None
    assert only_p["dx"] is None
    assert torch.equal(only_p["dW"], both["dW"]) and torch.equal(only_p["datt"], both["datt"])


@pytest.mark.parametrize("adir", ["in", "out"])
def test_exact_argument_forms(cuda, adir):
    """Hp as [N, H, C] and att_weight as [H, 2C] give the bits of the 2-D /
    [1, H, 2C] forms, forward and backward."""
    from mgcn.graph import plan_for
    from mgcn.ops import attention_aggregate
    H, C = 6, 3
    ei, N, x, W, att, dY, mask, _ = ladder_op_inputs(H, C, adir, 62)
    plan = plan_for(ei.to(cuda), N)
    Hp = (x @ W).to(cuda)
    out = []
    for hp_shape, att_shape in (((N, H * C), (1, H, 2 * C)), ((N, H, C), (H, 2 * C))):
        hp = Hp.reshape(hp_shape).clone().requires_grad_(True)
        a = att.to(cuda).reshape(att_shape).clone().requires_grad_(True)
        y, alpha = attention_aggregate(hp, a, plan, H, "lrelu", adir, edge_mask=mask.to(cuda))
        y.backward(dY.to(cuda))
        assert y.shape == (N, H * C) and alpha.shape == (ei.size(1), H)
        assert hp.grad.shape == hp_shape and a.grad.shape == att_shape
        out.append((y.detach(), alpha, hp.grad.reshape(N, -1), a.grad.reshape(H, -1)))
    for t0, t1 in zip(*out):
        assert torch.equal(t0, t1)
