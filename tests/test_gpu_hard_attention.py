"""Hard attention on the GPU (MI355X): NodeModelHardAttention and
ops.hard_attention_aggregate against the reference's own runs
(tests/golden/hatt_*.npz, Gumbel noise replayed), bitwise anchors against the
soft-attention kernels, the kernels' branch structure, and the argmax's edge
cases.

Every continuous tensor compared with a reference uses attention_ref.check,

    max|t_gpu - t64| <= max(4 * max|t32 - t64|, 1e-5 * max|t64|)

with t32 / t64 the reference's fp32 / fp64 runs (fixtures) or the torch
restatement hard_attention_ref.hatt_ref on the CPU (random shapes).  Discrete
tensors (the one-hot alpha, winner) must be equal; comparisons of one kernel
run with another are bitwise (torch.equal).
"""
import numpy as np
import pytest
import torch

from attention_ref import check, degree_graph, ladder_graph
from hard_attention_ref import EVAL, TRAIN, fixture, hatt_ref, noises, one_hot, replay_noise, \
    scan_argmax

pytestmark = pytest.mark.gpu


def make_nm(cuda, fin, fout, H, combine, adir, act, bias, T=0.1, sample=False, dropout=0.0):
    from mgcn.models import NodeModelHardAttention
    nm = NodeModelHardAttention(fin, fout, nheads=H, att_act=act, att_dropout=dropout,
                                att_combine=combine, att_dir=adir, bias=bias, temperature=T,
                                sample=sample)
    return nm.to(cuda)


def run_nm(nm, x, ei, dY, noise):
    import mgcn.models as M
    x = x.detach().requires_grad_(True)
    nm.zero_grad()
    for p in nm.parameters():
        p.grad = None
    store = []
    with replay_noise(M, noise, x.device):
        y = nm(x, ei, attn_store=store)
    y.backward(dY)
    assert not store[0].requires_grad
    return {"y": y.detach(), "alpha": store[0], "dx": x.grad, "dW": nm.weight.grad,
            "datt": nm.att_weight.grad, "db": None if nm.bias is None else nm.bias.grad}


def load_into(nm, fx, cuda):
    nm.load_state_dict({k[2:]: v for k, v in fx.items() if k.startswith("p_")})
    return nm.to(cuda)


# ------------------------------------------------------------------ fixtures
@pytest.mark.parametrize("name", list(TRAIN))
def test_fixture_train(cuda, name):
    fin, fout, H, combine, adir, act, bias, T = TRAIN[name]
    fx = fixture(name)
    nm = load_into(make_nm(cuda, fin, fout, H, combine, adir, act, bias, T), fx, cuda).train()
    got = run_nm(nm, fx["x"].to(cuda), fx["edge_index"].to(cuda), fx["dY"].to(cuda), noises(fx))
    for k in ("y", "alpha", "dx", "dW", "datt") + (("db",) if bias else ()):
        check(f"{name}.{k}", got[k], fx[k + "32"], fx[k + "64"])


@pytest.mark.parametrize("name", list(EVAL))
def test_fixture_eval(cuda, name):
    fin, fout, H, combine, adir, act, sample = EVAL[name]
    fx = fixture(name)
    nm = load_into(make_nm(cuda, fin, fout, H, combine, adir, act, False, sample=sample), fx,
                   cuda).eval()
    got = run_nm(nm, fx["x"].to(cuda), fx["edge_index"].to(cuda), fx["dY"].to(cuda), noises(fx))
    assert torch.equal(got["alpha"].cpu().double(), fx["alpha64"])
    assert got["datt"] is None
    for k in ("y", "dx", "dW"):
        check(f"{name}.{k}", got[k], fx[k + "32"], fx[k + "64"])


# ------------------------------------------------------- op-level machinery
def rand_inputs(N, E, fin, H, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, fin, generator=g)
    W = torch.randn(fin, H * C, generator=g) * 0.3
    att = torch.randn(1, H, 2 * C, generator=g) * 0.5
    dY = torch.randn(N, H * C, generator=g)
    u = torch.rand(E, H, generator=g)
    noise = -torch.log(-torch.log(u + 1e-20) + 1e-20)
    return x, W, att, dY, noise


def op_run(cuda, x, W, att, ei, N, dY, H, adir, act, T, training, noise, mask=None):
    from mgcn.graph import plan_for
    from mgcn.ops import hard_attention_aggregate, linear
    xs, Ws, As = (t.detach().to(cuda).requires_grad_(True) for t in (x, W, att))
    y, alpha = hard_attention_aggregate(
        linear(xs, Ws), As, plan_for(ei.to(cuda), N), H, act, adir, T, training=training,
        noise=None if noise is None else noise.to(cuda),
        edge_mask=None if mask is None else mask.to(cuda))
    assert not alpha.requires_grad
    y.backward(dY.to(cuda))
    return {"y": y.detach(), "alpha": alpha, "dx": xs.grad, "dW": Ws.grad, "datt": As.grad}


def op_ref(x, W, att, ei, dY, H, adir, act, T, training, noise, dtype, mask=None,
           alpha_eval=None):
    xs, Ws, As = (t.detach().clone().to(dtype).requires_grad_(True) for t in (x, W, att))
    y, alpha = hatt_ref(xs, Ws, As, None, ei, H, "cat", adir, act, T, training, noise, mask,
                        alpha_eval=alpha_eval)
    y.backward(dY.to(dtype))
    return {"y": y.detach(), "alpha": alpha.detach(), "dx": xs.grad, "dW": Ws.grad,
            "datt": As.grad}


def near_argmax(alpha, x, W, att, ei, N, H, adir, act, noise):
    """A selection made on fp32 logits: every (group, head) with an edge has
    exactly one entry (plus the quirk edge when some group is empty), and the
    fp64 logit of the selected edge is within the fp32 rounding of the group's
    fp64 maximum.  The rounding: Hp is a fin-term fp32 dot product, z a 2 C
    term one over it, then the activation and the noise add, so
    (fin + 2 C + 8) 2^-23 times the largest sum of magnitudes bounds it."""
    E = ei.size(1)
    C = W.size(1) // H
    xd, Wd, ad = x.double(), W.double(), att.double()
    hp = (xd @ Wd).view(N, H, -1)
    z = (torch.cat([hp[ei[0]], hp[ei[1]]], dim=-1) * ad).sum(-1)
    l = {"none": z, "lrelu": torch.nn.functional.leaky_relu(z, 0.2), "relu": torch.relu(z)}[act]
    l = l + noise.double()
    hpm = (xd.abs() @ Wd.abs()).view(N, H, -1)
    mag = (torch.cat([hpm[ei[0]], hpm[ei[1]]], dim=-1) * ad.abs()).sum(-1) + noise.double().abs()
    tol = (x.size(1) + 2 * C + 8) * 2.0 ** -23 * float(mag.max())
    idx = ei[0] if adir == "out" else ei[1]
    ix = idx.view(-1, 1).expand(-1, H)
    m = torch.full((N, H), -1e16, dtype=torch.float64).scatter_reduce(0, ix, l, "amax")
    alpha = alpha.double().cpu()
    assert set(alpha.unique().tolist()) <= {0.0, 1.0}
    has_empty = bool((torch.bincount(idx, minlength=N) == 0).any())
    picked = alpha.clone()
    if has_empty:
        assert (alpha[E - 1] == 1).all()
        picked[E - 1] = 0
    count = torch.zeros(N, H, dtype=torch.float64).index_add(0, idx, picked)
    nonempty = (torch.bincount(idx, minlength=N) > 0).view(-1, 1).expand(-1, H)
    last = torch.zeros(N, H, dtype=torch.bool)
    if has_empty:
        last[idx[E - 1]] = True  # the quirk edge may also be its own group's winner
    assert ((count == 1) | (last & (count == 0)) | ~nonempty).all()
    assert (count[~nonempty] == 0).all()
    worst = ((m[idx] - l) * picked).max().item()
    print(f"near-argmax: worst deficit {worst:.3e}  tolerance {tol:.3e}")
    assert worst <= tol


def both_modes(cuda, tag, ei, N, fin, H, C, adir, act, seed, T=0.5):
    """Training: y, alpha, dx, dW, datt to the bound.  Sampled eval: the
    selection is a valid one and picks a maximum up to fp32 rounding of the
    logits (near_argmax; mgcn_hatt_select's exact rule is pinned on exact
    logits by the select tests below), and y, dx, dW follow that selection to
    the bound; att_weight receives no gradient."""
    x, W, att, dY, noise = rand_inputs(N, ei.size(1), fin, H, C, seed)
    r32 = op_ref(x, W, att, ei, dY, H, adir, act, T, True, noise, torch.float32)
    r64 = op_ref(x, W, att, ei, dY, H, adir, act, T, True, noise, torch.float64)
    got = op_run(cuda, x, W, att, ei, N, dY, H, adir, act, T, True, noise)
    for k in ("y", "alpha", "dx", "dW", "datt"):
        check(f"{tag}.train.{k}", got[k], r32[k], r64[k])
    got = op_run(cuda, x, W, att, ei, N, dY, H, adir, act, T, False, noise)
    assert got["datt"] is None
    sel = got["alpha"].cpu()
    near_argmax(sel, x, W, att, ei, N, H, adir, act, noise)
    r32 = op_ref(x, W, att, ei, dY, H, adir, act, T, False, noise, torch.float32, alpha_eval=sel)
    r64 = op_ref(x, W, att, ei, dY, H, adir, act, T, False, noise, torch.float64, alpha_eval=sel)
    for k in ("y", "dx", "dW"):
        check(f"{tag}.eval.{k}", got[k], r32[k], r64[k])


# ------------------------------------------------------------- branch sweep
@pytest.mark.parametrize("adir", ["in", "out"])
@pytest.mark.parametrize("H,C", [(1, 7), (3, 33), (4, 64), (8, 64), (16, 64)])
def test_fpl_instantiations(cuda, H, C, adir):
    """One (H, C) per FPL = 1 / 2 / 4 / 8 / 16 of ATT_DISPATCH, on the graph
    with rows of degree 0 / 1 / 63 / 64 / 65 / 300 on either side."""
    assert [f for f in (1, 2, 4, 8, 16) if (H * C + 63) // 64 <= f][0] == \
        {7: 1, 99: 2, 256: 4, 512: 8, 1024: 16}[H * C]
    ei, N = degree_graph()
    both_modes(cuda, f"fpl.H{H}C{C}{adir}", ei, N, 12, H, C, adir, "lrelu", 300 + H)


@pytest.mark.parametrize("adir", ["in", "out"])
@pytest.mark.parametrize("H", [3, 5, 7, 16])
def test_head_counts_ladder(cuda, H, adir):
    """H that does not divide 64 (idle lanes, the lane-group combine) and
    H = 16 on the ladder: rows of every degree 0..66 cover G - 1, G, G + 1 for
    G = 64 // H."""
    ei, N = ladder_graph()
    both_modes(cuda, f"ladder.H{H}{adir}", ei, N, 6, H, 4, adir, "relu", 400 + H)


_STRIDE = {}


def stride_graph():
    """N = 2 * 16384 + 37: att_grid's cap (4096 workgroups of 4 waves) covers
    16384 rows per trip, so some waves take a third row; 3 N random edges."""
    if not _STRIDE:
        rng = np.random.default_rng(3)
        N = 2 * 16384 + 37
        ei = rng.integers(0, N, (2, 3 * N))
        _STRIDE["ei"], _STRIDE["N"] = torch.from_numpy(ei.astype(np.int64)), N
    return _STRIDE["ei"], _STRIDE["N"]


def test_grid_stride(cuda):
    """Per-row state (max, denominator, winner, accumulators) must not carry
    over to a wave's second and third row.  No activation: with 1e5 logits a
    kink within fp32 rounding of some z would set the bound, not the code
    (tests/test_gpu_attention_shapes.py::test_grid_stride_trips)."""
    ei, N = stride_graph()
    both_modes(cuda, "stride", ei, N, 6, 2, 4, "in", "none", 77)


# ------------------------------------------------------------ bitwise anchors
@pytest.mark.parametrize("adir", ["in", "out"])
@pytest.mark.parametrize("null_noise", [True, False])
def test_t1_zero_noise_is_soft_attention(cuda, adir, null_noise):
    """T = 1 and no noise: e + 0 and e / 1 are exact, so y, alpha, dHp and
    datt are the bits of attention_aggregate (also under a dropout mask)."""
    from mgcn.graph import plan_for
    from mgcn.ops import attention_aggregate, hard_attention_aggregate
    ei, N = degree_graph()
    H, C = 3, 5
    x, W, att, dY, _ = rand_inputs(N, ei.size(1), 6, H, C, 5)
    plan = plan_for(ei.to(cuda), N)
    g = torch.Generator().manual_seed(9)
    mask = ((torch.rand(ei.size(1), H, generator=g) < 0.5).float() * 2).to(cuda)
    noise = None if null_noise else torch.zeros(ei.size(1), H, device=cuda)
    out = []
    for hard in (False, True):
        hp = (x @ W).to(cuda).requires_grad_(True)
        a = att.to(cuda).requires_grad_(True)
        if hard:
            y, alpha = hard_attention_aggregate(hp, a, plan, H, "lrelu", adir, 1.0, training=True,
                                                noise=noise, edge_mask=mask)
        else:
            y, alpha = attention_aggregate(hp, a, plan, H, "lrelu", adir, edge_mask=mask)
        y.backward(dY.to(cuda))
        out.append((y.detach(), alpha, hp.grad, a.grad))
    for name, s, h in zip(("y", "alpha", "dHp", "datt"), *out):
        assert torch.equal(s, h), name


def c_gather(plan, alpha_slot, Hp, H, C, dense, pads=(0, 0)):
    """mgcn_hatt_gather, or mgcn_att_fwd in its aggregate-only mode, through
    the C ABI; Hp / Y as windows of sentinel-filled buffers."""
    import mgcn
    from mgcn import _lib as L
    from test_gpu_attention_shapes import window
    lib = mgcn.load()
    N, nnz, HC = plan.num_nodes, plan.nnz, H * C
    fwd = plan.fwd
    (bHp, wHp), (bY, wY) = (window(s, N, HC, p, Hp.device) for s, p in zip((Hp, None), pads))
    st = L.stream_of(Hp.device)
    if dense:
        L.check(lib.mgcn_att_fwd(N, nnz, H, C, L.ptr(fwd.rowptr), L.ptr(fwd.col), None, None, 0,
                                 L.ptr(alpha_slot), None, L.ptr(wHp), wHp.stride(0), L.ptr(wY),
                                 wY.stride(0), None, st), "mgcn_att_fwd")
    else:
        L.check(lib.mgcn_hatt_gather(N, nnz, H, C, L.ptr(fwd.rowptr), L.ptr(fwd.col),
                                     L.ptr(alpha_slot), L.ptr(wHp), wHp.stride(0), L.ptr(wY),
                                     wY.stride(0), st), "mgcn_hatt_gather")
    torch.cuda.synchronize(Hp.device)
    return wY, (bHp, bY)


@pytest.mark.parametrize("H,C", [(1, 7), (3, 33), (4, 64), (8, 64), (16, 64), (5, 4)])
def test_gather_is_dense_aggregate_bitwise(cuda, H, C):
    """mgcn_hatt_gather == mgcn_att_fwd(alpha_in) bit for bit, on a one-hot
    alpha (one winner per row and head) and on a random alpha with 70 % zeros
    (whole slots zero, and slots zero on some heads only); two runs agree; a
    leading dimension of H C + 3 gives the same bits and leaves the padding."""
    from mgcn.graph import plan_for
    from test_gpu_attention_shapes import padding_intact
    ei, N = degree_graph()
    E = ei.size(1)
    plan = plan_for(ei.to(cuda), N)
    g = torch.Generator().manual_seed(10 * H + C)
    Hp = torch.randn(N, H * C, generator=g).to(cuda)
    hot = one_hot(scan_argmax(torch.randn(E, H, generator=g), ei[1], N), E)
    sparse = torch.randn(E, H, generator=g) * (torch.rand(E, H, generator=g) < 0.3)
    sparse[torch.rand(E, generator=g) < 0.5] = 0
    for name, a in (("one-hot", hot), ("sparse", sparse)):
        a_slot = a.to(cuda)[plan.fwd.eid.long()].contiguous()
        dense, _ = c_gather(plan, a_slot, Hp, H, C, True)
        skip, _ = c_gather(plan, a_slot, Hp, H, C, False)
        again, _ = c_gather(plan, a_slot, Hp, H, C, False)
        wide, bufs = c_gather(plan, a_slot, Hp, H, C, False, pads=(3, 3))
        assert torch.count_nonzero(dense) > 0
        assert torch.equal(skip, dense), name
        assert torch.equal(again, skip) and torch.equal(wide, skip), name
        assert padding_intact(bufs[0], H * C, 3) and padding_intact(bufs[1], H * C, 3)


def c_train(plan, Hp, att, noise_slot, dY, H, C, act, adir, T, pads):
    """The launch sequence of ops._HardAttentionTrain through the C ABI with
    Hp / Y / dY / dHp as windows of wider buffers."""
    import mgcn
    from mgcn import _lib as L
    from test_gpu_attention_shapes import window
    lib, ptr = mgcn.load(), L.ptr
    dev = Hp.device
    N, nnz, HC = plan.num_nodes, plan.nnz, H * C
    fwd, bwd, slot = plan.fwd, plan.bwd, plan.slot_map()
    st = L.stream_of(dev)
    (bHp, wHp), (bY, wY), (bdY, wdY), (bdHp, wdHp) = (
        window(s, N, HC, p, dev) for s, p in zip((Hp, None, dY, None), pads))
    ldh, ldy, lddy, lddh = (w.stride(0) for w in (wHp, wY, wdY, wdHp))

    def f32(*shape):
        return torch.empty(*shape, dtype=torch.float32, device=dev)
    s_src, s_dst, alpha = f32(N, H), f32(N, H), f32(nnz, H)
    L.check(lib.mgcn_att_scores(N, H, C, ptr(wHp), ldh, ptr(att), ptr(s_src), ptr(s_dst), st),
            "mgcn_att_scores")
    inn = adir == "in"
    if inn:
        L.check(lib.mgcn_hatt_fwd(N, nnz, H, C, ptr(fwd.rowptr), ptr(fwd.col), ptr(s_dst),
                                  ptr(s_src), act, ptr(noise_slot), T, None, None, ptr(wHp), ldh,
                                  ptr(wY), ldy, ptr(alpha), st), "mgcn_hatt_fwd")
    else:
        a_bwd = f32(nnz, H)
        L.check(lib.mgcn_hatt_edge_softmax(N, nnz, H, ptr(bwd.rowptr), ptr(bwd.col), ptr(s_src),
                                           ptr(s_dst), act, ptr(noise_slot), T, ptr(a_bwd), st),
                "mgcn_hatt_edge_softmax")
        alpha[slot[:nnz].long()] = a_bwd
        L.check(lib.mgcn_hatt_fwd(N, nnz, H, C, ptr(fwd.rowptr), ptr(fwd.col), None, None, act,
                                  None, T, ptr(alpha), None, ptr(wHp), ldh, ptr(wY), ldy, None,
                                  st), "mgcn_hatt_fwd")
    dz, ds_src, ds_dst = f32(nnz, H), f32(N, H), f32(N, H)
    L.check(lib.mgcn_hatt_bwd_dst(N, nnz, H, C, ptr(fwd.rowptr), ptr(fwd.col), ptr(wHp), ldh,
                                  ptr(wdY), lddy, ptr(alpha), None, ptr(s_dst), ptr(s_src), act,
                                  int(inn), T, ptr(dz), ptr(ds_dst), st), "mgcn_hatt_bwd_dst")
    L.check(lib.mgcn_hatt_bwd_src(N, nnz, H, C, ptr(bwd.rowptr), ptr(bwd.col), ptr(slot),
                                  ptr(wdY), lddy, ptr(alpha), None, ptr(dz), ptr(s_src),
                                  ptr(s_dst), act, int(not inn), T, ptr(att),
                                  ptr(ds_dst) if inn else None, ptr(ds_src), ptr(wdHp), lddh, st),
            "mgcn_hatt_bwd_src")
    if not inn:
        L.check(lib.mgcn_att_dst_fold(N, nnz, H, C, ptr(fwd.rowptr), ptr(dz), ptr(att),
                                      ptr(ds_dst), ptr(wdHp), lddh, st), "mgcn_att_dst_fold")
    torch.cuda.synchronize(dev)
    return {"Y": wY, "alpha": alpha, "dHp": wdHp, "buffers": (bHp, bY, bdY, bdHp)}


@pytest.mark.parametrize("adir", ["in", "out"])
def test_leading_dimensions_c_abi(cuda, adir):
    """Hp / Y / dY / dHp with ld = H C + 3 inside sentinel-filled buffers: the
    bits of the compact call and of the public op, sentinels untouched."""
    from mgcn import _lib as L
    from mgcn.graph import plan_for
    from mgcn.ops import hard_attention_aggregate
    from test_gpu_attention_shapes import padding_intact
    ei, N = degree_graph()
    H, C, T = 3, 5, 0.5
    x, W, att, dY, noise = rand_inputs(N, ei.size(1), 6, H, C, 21)
    plan = plan_for(ei.to(cuda), N)
    Hp = (x @ W).to(cuda).requires_grad_(True)
    a = att.to(cuda).requires_grad_(True)
    y, alpha_coo = hard_attention_aggregate(Hp, a, plan, H, "lrelu", adir, T, training=True,
                                            noise=noise.to(cuda))
    y.backward(dY.to(cuda))
    walked = plan.fwd if adir == "in" else plan.bwd
    n_slot = noise.to(cuda)[walked.eid.long()].contiguous()
    att2 = a.detach().reshape(H, 2 * C).contiguous()
    act = L.ATT_ACT_CODES["lrelu"]
    flat = c_train(plan, Hp.detach(), att2, n_slot, dY.to(cuda), H, C, act, adir, T, (0,) * 4)
    wide = c_train(plan, Hp.detach(), att2, n_slot, dY.to(cuda), H, C, act, adir, T, (3,) * 4)
    for k in ("Y", "alpha", "dHp"):
        assert torch.equal(wide[k], flat[k]), k
    for buf, name in zip(wide["buffers"], ("Hp", "Y", "dY", "dHp")):
        assert padding_intact(buf, H * C, 3), f"{name}: a padding column was written"
    assert torch.equal(wide["Y"], y.detach()) and torch.equal(wide["dHp"], Hp.grad)
    coo = torch.empty_like(alpha_coo)
    coo[plan.fwd.eid.long()] = wide["alpha"]
    assert torch.equal(coo, alpha_coo)


@pytest.mark.parametrize("training", [True, False])
def test_two_runs_bitwise(cuda, training):
    ei, N = degree_graph()
    H, C = 5, 4
    x, W, att, dY, noise = rand_inputs(N, ei.size(1), 6, H, C, 31)
    a, b = (op_run(cuda, x, W, att, ei, N, dY, H, "out", "lrelu", 0.1, training, noise)
            for _ in range(2))
    for k in a:
        assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), k


# ---------------------------------------------------------- select edge cases
def c_select(cuda, ei, N, s_row, s_col, act, noise, H, by="dst"):
    """mgcn_hatt_select through the C ABI over the fwd (groups = destinations)
    or bwd view; returns (alpha in COO order, winner as COO edge ids)."""
    import mgcn
    from mgcn import _lib as L
    from mgcn.graph import plan_for
    lib = mgcn.load()
    plan = plan_for(ei.to(cuda), N)
    view = plan.fwd if by == "dst" else plan.bwd
    eid = view.eid.long()
    nnz = plan.nnz
    alpha = torch.full((nnz, H), 7.0, dtype=torch.float32, device=cuda)
    winner = torch.full((N, H), -7, dtype=torch.int32, device=cuda)
    n_slot = None if noise is None else noise.to(cuda)[eid].contiguous()
    L.check(lib.mgcn_hatt_select(N, nnz, H, L.ptr(view.rowptr), L.ptr(view.col),
                                 L.ptr(s_row.to(cuda).contiguous()),
                                 L.ptr(s_col.to(cuda).contiguous()), L.ATT_ACT_CODES[act],
                                 L.ptr(n_slot), L.ptr(alpha), L.ptr(winner),
                                 L.stream_of(torch.device(cuda))), "mgcn_hatt_select")
    torch.cuda.synchronize()
    coo = torch.empty_like(alpha)
    coo[eid] = alpha
    w = winner.long().cpu()
    w_coo = torch.where(w >= 0, eid.cpu()[w.clamp(min=0)], w)
    return coo.cpu(), w_coo


def check_select(cuda, ei, N, s_row, s_col, noise, H, by="dst"):
    """winner and the one-hot agree with each other and with the `>=` scan."""
    alpha, w = c_select(cuda, ei, N, s_row, s_col, "none", noise, H, by)
    idx = ei[1] if by == "dst" else ei[0]
    oth = ei[0] if by == "dst" else ei[1]
    l = s_row[idx] + s_col[oth] + (0 if noise is None else noise)
    want = scan_argmax(l, idx, N)
    assert torch.equal(w, want)
    hot = torch.zeros(ei.size(1), H)
    for h in range(H):
        hot[want[:, h][want[:, h] >= 0], h] = 1.0
    assert torch.equal(alpha, hot)
    return alpha, w


@pytest.mark.parametrize("by", ["dst", "src"])
@pytest.mark.parametrize("H", [1, 3, 4, 16])
def test_select_consistent_with_scan(cuda, H, by):
    """Random scores on the ladder graph (rows of every degree 0..66): one
    winner per non-empty (row, head), -1 and no entry for an empty row, a row
    of one slot has alpha bitwise 1."""
    ei, N = ladder_graph()
    g = torch.Generator().manual_seed(50 + H)
    s_row, s_col = torch.randn(N, H, generator=g), torch.randn(N, H, generator=g)
    noise = torch.randn(ei.size(1), H, generator=g)
    alpha, w = check_select(cuda, ei, N, s_row, s_col, noise, H, by)
    idx = ei[1] if by == "dst" else ei[0]
    deg = torch.bincount(idx, minlength=N)
    assert (w[deg == 0] == -1).all() and (w[deg > 0] >= 0).all()
    assert torch.equal(alpha[deg[idx] == 1], torch.ones(int((deg[idx] == 1).sum()), H))


def test_select_ties_last_slot_wins(cuda):
    """All-equal scores (every logit exactly 0), duplicate edges, and a
    three-way tie spread over two chunks of a degree-70 row with H = 4 (chunks
    of 16 slots): the last slot in COO order wins in each."""
    H = 4
    N = 80
    src = torch.arange(1, 71)
    ei = torch.stack([torch.cat([src, torch.tensor([5, 5, 9])]),
                      torch.cat([torch.zeros(70, dtype=torch.long), torch.tensor([1, 1, 1])])])
    zero = torch.zeros(N, H)
    alpha, w = check_select(cuda, ei, N, zero, zero, None, H)
    assert (w[0] == 69).all() and (w[1] == 72).all()
    # node 0: scores 1 on slots 3, 20 and 40 (chunks 0, 1, 2), head 2 only; 0 elsewhere
    noise = torch.zeros(73, H)
    noise[[3, 20, 40], 2] = 1.0
    alpha, w = check_select(cuda, ei, N, zero, zero, noise, H)
    assert w[0].tolist() == [69, 69, 40, 69]
    # duplicates 5 -> 1 (edges 70, 71) tie above 9 -> 1: the later duplicate
    noise = torch.zeros(73, H)
    noise[[70, 71]] = 2.0
    alpha, w = check_select(cuda, ei, N, zero, zero, noise, H)
    assert (w[1] == 71).all()


def test_select_below_fill_and_nan_never_win(cuda):
    """A logit below -1e16 or a NaN never wins; a row of nothing else has no
    winner and an all-zero alpha."""
    H, N = 2, 6
    ei = torch.tensor([[1, 2, 3, 4, 5, 1], [0, 0, 0, 3, 3, 4]])
    zero = torch.zeros(N, H)
    noise = torch.zeros(6, H)
    noise[0] = -3e16
    noise[1, 0] = float("nan")
    noise[1, 1] = -1e16          # exactly the start value: `>=` takes it ...
    noise[2, 1] = -2e16          # ... and a later smaller one does not replace it
    noise[2, 0] = -5.0
    noise[3] = -2e16
    noise[4] = float("nan")
    alpha, w = check_select(cuda, ei, N, zero, zero, noise, H)
    assert w[0].tolist() == [2, 1] and w[3].tolist() == [-1, -1] and w[4].tolist() == [5, 5]
    assert torch.count_nonzero(alpha[[0, 3, 4]]) == 0


@pytest.mark.parametrize("adir", ["in", "out"])
def test_quirk_both_ways(cuda, adir):
    """One empty group marks COO edge E - 1 on every head (and its message
    reaches Y); no empty group marks nothing beyond the winners."""
    H, C, N = 3, 4, 12
    g = torch.Generator().manual_seed(3)
    ring = torch.stack([torch.arange(N), (torch.arange(N) + 1) % N])
    extra = torch.stack([torch.randint(0, N, (30,), generator=g),
                         torch.randint(0, N, (30,), generator=g)])
    full = torch.cat([extra, ring], dim=1)            # every node has an in- and an out-edge
    holed = full[:, (full[0] != 4) & (full[1] != 4)]  # node 4: no edge at all
    x, W, att, dY, _ = rand_inputs(N, 1, 6, H, C, 8)
    for ei, empty in ((full, False), (holed, True)):
        E = ei.size(1)
        noise = torch.randn(E, H, generator=g)
        got = op_run(cuda, x, W, att, ei, N, dY, H, adir, "lrelu", 0.1, False, noise)
        ref = op_ref(x, W, att, ei, dY, H, adir, "lrelu", 0.1, False, noise, torch.float64)
        alpha = got["alpha"].cpu()
        assert torch.equal(alpha.double(), ref["alpha"])
        idx = ei[0] if adir == "out" else ei[1]
        groups = int((torch.bincount(idx, minlength=N) > 0).sum())
        if empty:
            assert (alpha[E - 1] == 1).all()
            assert groups * H <= int(alpha.sum()) <= groups * H + H
        else:
            assert int(alpha.sum()) == N * H
        r32 = op_ref(x, W, att, ei, dY, H, adir, "lrelu", 0.1, False, noise, torch.float32)
        check(f"quirk.{adir}.{empty}.y", got["y"], r32["y"], ref["y"])
        if adir == "in":
            assert torch.count_nonzero(got["y"][(torch.bincount(ei[1], minlength=N) == 0)
                                                .to(cuda)]) == 0


def test_c_abi_refuses_bad_arguments(cuda):
    """Every new entry returns MGCN_EINVAL, before a launch, for H = 17,
    H C > 1024, a leading dimension below H C and (where it takes one) a
    temperature <= 0; outputs keep their sentinel."""
    import mgcn
    from mgcn import _lib as L
    from mgcn.graph import plan_for
    lib, ptr = mgcn.load(), L.ptr
    ei, N = ladder_graph()
    plan = plan_for(ei.to(cuda), N)
    nnz, fwd, bwd, slot = plan.nnz, plan.fwd, plan.bwd, plan.slot_map()
    st = L.stream_of(cuda)

    def buf(*shape):
        return torch.full(shape, 7.0, dtype=torch.float32, device=cuda)
    # sized for the largest shape asked for below, so that even a launch would stay in bounds
    Hp, Y, dY, dHp = buf(N, 1100), buf(N, 1100), buf(N, 1100), buf(N, 1100)
    s1, s2, ds1, ds2 = buf(N, 17), buf(N, 17), buf(N, 17), buf(N, 17)
    alpha, dz, att = buf(nnz, 17), buf(nnz, 17), buf(17, 2200)
    winner = torch.full((N, 17), -7, dtype=torch.int32, device=cuda)

    def fwd_(H, C, T, ld):
        return lib.mgcn_hatt_fwd(N, nnz, H, C, ptr(fwd.rowptr), ptr(fwd.col), ptr(s1), ptr(s2), 0,
                                 None, T, None, None, ptr(Hp), ld, ptr(Y), ld, ptr(alpha), st)

    def softmax_(H, C, T, ld):
        return lib.mgcn_hatt_edge_softmax(N, nnz, H, ptr(bwd.rowptr), ptr(bwd.col), ptr(s1),
                                          ptr(s2), 0, None, T, ptr(alpha), st)

    def bwd_dst_(H, C, T, ld):
        return lib.mgcn_hatt_bwd_dst(N, nnz, H, C, ptr(fwd.rowptr), ptr(fwd.col), ptr(Hp), ld,
                                     ptr(dY), ld, ptr(alpha), None, ptr(s1), ptr(s2), 0, 1, T,
                                     ptr(dz), ptr(ds1), st)

    def bwd_src_(H, C, T, ld):
        return lib.mgcn_hatt_bwd_src(N, nnz, H, C, ptr(bwd.rowptr), ptr(bwd.col), ptr(slot),
                                     ptr(dY), ld, ptr(alpha), None, ptr(dz), ptr(s1), ptr(s2), 0,
                                     1, T, ptr(att), None, ptr(ds2), ptr(dHp), ld, st)

    def select_(H, C, T, ld):
        return lib.mgcn_hatt_select(N, nnz, H, ptr(fwd.rowptr), ptr(fwd.col), ptr(s1), ptr(s2), 0,
                                    None, ptr(alpha), ptr(winner), st)

    def gather_(H, C, T, ld):
        return lib.mgcn_hatt_gather(N, nnz, H, C, ptr(fwd.rowptr), ptr(fwd.col), ptr(alpha),
                                    ptr(Hp), ld, ptr(Y), ld, st)

    with_c = (fwd_, bwd_dst_, bwd_src_, gather_)
    with_t = (fwd_, softmax_, bwd_dst_, bwd_src_)
    for fn in with_c + (softmax_, select_):
        assert fn(17, 2, 1.0, 34) == L.EINVAL, fn.__name__           # H > 16
        assert fn(0, 2, 1.0, 34) == L.EINVAL, fn.__name__            # H < 1
    for fn in with_c:
        assert fn(2, 513, 1.0, 1026) == L.EINVAL, fn.__name__        # H C = 1026
        assert fn(4, 8, 1.0, 31) == L.EINVAL, fn.__name__            # ld < H C
    for fn in with_t:
        assert fn(4, 8, 0.0, 32) == L.EINVAL, fn.__name__
        assert fn(4, 8, -0.5, 32) == L.EINVAL, fn.__name__
    assert b"temperature" in lib.mgcn_last_error()
    torch.cuda.synchronize()
    for t in (Y, dHp, alpha, dz, ds1, ds2):
        assert bool((t == 7.0).all())
    assert bool((winner == -7).all())
    # n_rows == 0 is a successful no-op
    assert lib.mgcn_hatt_select(0, 0, 4, None, None, None, None, 0, None, None, None, st) == L.OK
    assert lib.mgcn_hatt_gather(0, 0, 4, 8, None, None, None, None, 32, None, 32, st) == L.OK


def test_empty_graph_and_bad_shapes(cuda):
    """E == 0: nothing happens (Y = 0, alpha [0, H]); H = 17 is refused by the
    op before a launch; CPU tensors raise."""
    import mgcn
    from mgcn.graph import plan_for
    from mgcn.ops import hard_attention_aggregate
    N, H, C = 5, 2, 3
    ei = torch.zeros(2, 0, dtype=torch.long, device=cuda)
    plan = plan_for(ei, N)
    Hp = torch.randn(N, H * C, device=cuda)
    att = torch.randn(1, H, 2 * C, device=cuda)
    for training in (True, False):
        y, alpha = hard_attention_aggregate(Hp, att, plan, H, "none", "out", 0.1,
                                            training=training)
        assert torch.count_nonzero(y) == 0 and alpha.shape == (0, H)
    with pytest.raises(mgcn.MgcnError):
        hard_attention_aggregate(torch.randn(N, 17 * 2, device=cuda),
                                 torch.randn(1, 17, 4, device=cuda), plan, 17, training=False)
    with pytest.raises(mgcn.MgcnError):
        hard_attention_aggregate(Hp.cpu(), att.cpu(), plan, H, training=False)


# -------------------------------------------------------------------- dropout
@pytest.mark.parametrize("adir", ["in", "out"])
def test_dropout_training(cuda, adir):
    """Under a fixed torch seed the module draws mask = dropout(ones) [E, H]:
    attn_store holds alpha * mask and the gradients follow the mask (the
    restatement run with the same mask)."""
    import mgcn.models as M
    ei, N = degree_graph()
    H, C, fin, p = 3, 4, 6, 0.4
    E = ei.size(1)
    x, _, _, dY, noise = rand_inputs(N, E, fin, H, C, 91)
    torch.manual_seed(4)
    nm = make_nm(cuda, fin, H * C, H, "cat", adir, "lrelu", False, T=0.5, dropout=p).train()
    torch.manual_seed(1234)
    mask = torch.nn.functional.dropout(torch.ones(E, H, device=cuda), p=p, training=True).cpu()
    assert 0 < int((mask == 0).sum()) < E * H
    torch.manual_seed(1234)
    got = run_nm(nm, x.to(cuda), ei.to(cuda), dY.to(cuda), [noise])
    assert torch.equal(got["alpha"].cpu() == 0, mask == 0)
    W, att = nm.weight.detach().cpu(), nm.att_weight.detach().cpu()
    r32 = op_ref(x, W, att, ei, dY, H, adir, "lrelu", 0.5, True, noise, torch.float32, mask)
    r64 = op_ref(x, W, att, ei, dY, H, adir, "lrelu", 0.5, True, noise, torch.float64, mask)
    for k in ("y", "alpha", "dx", "dW", "datt"):
        check(f"dropout.{adir}.{k}", got[k], r32[k], r64[k])
    nm.eval()  # no dropout, no noise call without sample
    store = []
    with replay_noise(M, [], cuda):
        nm(x.to(cuda), ei.to(cuda), attn_store=store)
    assert set(store[0].unique().tolist()) <= {0.0, 1.0}
