"""The residual layer, its stack and the input layer at the ABI
(mgcn_residual_layer_fwd / _bwd, mgcn_residual_stack_fwd / _bwd,
mgcn_input_layer_fwd / _bwd; csrc/residual.hip, the ResEpi epilogue of the
heavy-row kernels) against the fp64 restatements of residual_ref.py, on graphs
whose rows sit on every boundary of the kernels:

  a  the degree ladder, N = 700: heavy and giant rows in both views, degrees at
     the gather's round boundaries and at the heavy / giant thresholds
  b  the ladder cut at degree 128: a schedule without heavy rows
  c  the ladder cut at degree 300: heavy rows, no giant ones
  d  uniform random, N = 1 .. 130: no schedule (order NULL), N around a tile
     of 16 rows and a workgroup of 64
  e  every row heavy, N = 40: a light launch without rows
  f  no edges, N = 65
  g  N = 4200 with residual_blocks = 64: the light launch's waves loop

Every tensor is held to fp64_ref.within(err, bound, TOL) with TOL = 1e-5 per
layer passed (d layers: d TOL of the propagated bound); mask bits to the sign
of the fp64 pre-activations wherever that is not within TOL of the bound of
zero (at most AMBIGUOUS_CAP of a case's bits, asserted; the host tests check
the same inputs).  The worst err / limit per tensor is in every assertion
message and printed when the module ends.
"""
import contextlib
from types import SimpleNamespace

import pytest
import torch

import residual_ref as R
from fp64_ref import within

pytestmark = pytest.mark.gpu

F = R.F
TOL = R.TOL
DEFAULTS = {"residual_blocks": 8192, "residual_fused_mask": 1, "gemm_tn_staged": 1,
            "heavy_side_stream": 1}
WORST = {}
SHARES = {}
_CASES = {}
_EDGES = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst err / limit per tensor:", {k: round(v, 4) for k, v in sorted(WORST.items())})
    print("worst ambiguous share per test:", {k: f"{v:.2e}" for k, v in sorted(SHARES.items())})


@contextlib.contextmanager
def option(name, value):
    from mgcn import _lib as L
    try:
        L.set_option(name, value)
        yield
    finally:
        L.set_option(name, DEFAULTS[name])


def graph_options(gname):
    """Graph g is the one whose light launch must loop."""
    return option("residual_blocks", 64) if gname == "g" else contextlib.nullcontext()


def case(cuda, gname, ni):
    """The graph plan, normalisation and fp64 operator of (graph, NORMS[ni]),
    built once; the schedule each graph is there for is asserted here."""
    from mgcn import _lib as L
    from mgcn.graph import plan_for
    key = (gname, ni)
    if key in _CASES:
        return _CASES[key]
    N, build = R.GRAPHS[gname]
    if gname not in _EDGES:
        ei = build()
        _EDGES[gname] = (ei, torch.from_numpy(ei).to(cuda))
    ei, eit = _EDGES[gname]
    deg_norm, aggr = R.NORMS[ni]
    plan = plan_for(eit, N)
    c = SimpleNamespace(N=N, ei=ei, eit=eit, plan=plan, norm=plan.norm(deg_norm), aggr=aggr,
                        mean=aggr == "mean", reduce=L.REDUCE_CODES[aggr],
                        A=R.make_A(ei, N, deg_norm, aggr, cuda))
    c.row_div = plan.in_cnt if c.mean else None
    din, dout = R.degrees_of(ei, N)
    c.din = torch.from_numpy(din).to(cuda)
    fv, bv = plan.fwd, plan.bwd
    if gname == "a":
        L_ = len(R.DEFAULT_LADDER)
        for v, first in ((fv, 0), (bv, L_)):
            assert v.n_heavy > 0 and v.n_giant > 0
            heavy = set(v.order[:v.n_heavy].tolist())
            giant = set(v.order[:v.n_giant].tolist())
            at = {d: first + i for i, d in enumerate(R.DEFAULT_LADDER)}
            assert at[129] in heavy and at[128] not in heavy
            assert at[513] in giant and at[512] not in giant and at[512] in heavy
    elif gname == "b":
        for v in (fv, bv):
            assert v.order is not None and v.n_heavy == 0
    elif gname == "c":
        for v in (fv, bv):
            assert v.n_heavy > 0 and v.n_giant == 0
    elif gname.startswith("d") or gname == "g":
        for v in (fv, bv):
            assert v.order is None
        if gname == "g":  # more 64-row groups than workgroups: the waves loop
            assert N - fv.n_heavy > 4 * 16 * 64 and -(-N // 64) > 64
    elif gname == "e":
        assert fv.n_heavy == N and bv.n_heavy == N
    elif gname == "f":
        assert plan.nnz == 0
    _CASES[key] = c
    return c


def hold(name, got, ref, bound, tol, tag):
    ok, worst = within(got.double() - ref, bound, tol)
    WORST[name] = max(WORST.get(name, 0.0), worst)
    assert ok, f"{name} {tag}: worst err / limit {worst:.3f}"
    return worst


def check_forward(test, Z, masks, z1p, zp, b1, bd, relu2, tol, tag, name="Z"):
    """Z and the two mask words of one layer against its fp64 pre-activations."""
    assert R.all_written(Z) and R.all_written(masks), tag
    hold(name, Z, zp.clamp_min(0) if relu2 else zp, bd, tol, tag)
    bits = R.words_bits(masks)
    for w, (pre, bound) in enumerate(((z1p, b1), (zp, bd))):
        amb = R.ambiguous(pre, bound)
        share = float(amb.double().mean()) if amb.numel() else 0.0
        SHARES[test] = max(SHARES.get(test, 0.0), share)
        assert share <= R.AMBIGUOUS_CAP, f"{tag} word {w}: ambiguous share {share:.2e}"
        bad = (bits[:, w] != (pre > 0)) & ~amb
        assert not bool(bad.any()), f"{tag} word {w}: {int(bad.sum())} wrong mask bits"
        assert not bool(bits[:, w][bound == 0].any()), f"{tag} word {w}: bit set where the bound is 0"
    if relu2:
        assert torch.equal(bits[:, 1], Z > 0), f"{tag}: word 1 is not the kernel's own Z > 0"


def new_masks(n, dev):
    return torch.full((n, 2), R.SENT, dtype=torch.int32, device=dev)


def run_layer_fwd(c, xs, W, b, Wr, br, relu1, relu2, **kw):
    from mgcn import _lib as L
    Zv, Zbuf = R.strided(c.N, F, 40, xs.device)
    masks = new_masks(c.N, xs.device)
    rc = R.layer_fwd(c.plan.fwd, c.norm.w_fwd, xs, W, b, Wr, br, c.reduce, relu1, relu2, Zv, masks,
                     **kw)
    assert rc == L.OK, R.last_error()
    assert R.untouched(Zbuf[:, F:]), "the padding of Z's rows was written"
    return Zv, masks


# ---------------------------------------------------------------- 1. forward
@pytest.mark.parametrize("ni", range(len(R.NORMS)))
@pytest.mark.parametrize("gname", sorted(R.GRAPHS))
def test_layer_forward_against_fp64(cuda, gname, ni):
    """Z (strided, ld = 40) within the bound, every mask bit outside the
    ambiguous ones, every word written: all ReLU and bias combinations."""
    c = case(cuda, gname, ni)
    x, _, W, b, Wr, br = R.layer_inputs(c.N, R.case_seed(gname, ni), cuda)
    xs, _ = R.strided(c.N, F, 40, cuda, x)
    with graph_options(gname):
        for kind in R.BIASES:
            bb, bbr = R.pick_bias(kind, b, br)
            for relu1, relu2 in R.RELUS:
                tag = f"{gname} {R.NORMS[ni]} {kind} relu {relu1, relu2}"
                Z, masks = run_layer_fwd(c, xs, W, bb, Wr, bbr, relu1, relu2)
                z1p, zp, b1, bd = R.layer_fwd64(x, c.A, W, bb, Wr, bbr, c.mean, relu1, relu2,
                                                pre=True)
                check_forward("forward", Z, masks, z1p, zp, b1, bd, relu2, TOL, tag)


# ------------------------------------------------------- 2. schedule or not
@pytest.mark.parametrize("ni", range(len(R.NORMS)))
def test_rows_do_not_depend_on_the_schedule(cuda, ni):
    """Graph a with the plan's schedule and with order = NULL (every row on
    the light path, in natural order): the light rows bit for bit, the heavy
    ones within the bound."""
    c = case(cuda, "a", ni)
    x, _, W, b, Wr, br = R.layer_inputs(c.N, R.case_seed("a", ni), cuda)
    xs, _ = R.strided(c.N, F, 40, cuda, x)
    light = c.din <= 128
    assert int((~light).sum()) == c.plan.fwd.n_heavy > 0
    for relu1, relu2 in R.RELUS:
        tag = f"{R.NORMS[ni]} relu {relu1, relu2}"
        Zs, ms = run_layer_fwd(c, xs, W, b, Wr, br, relu1, relu2)
        Zn, mn = run_layer_fwd(c, xs, W, b, Wr, br, relu1, relu2, order=None)
        assert torch.equal(Zs[light], Zn[light]) and torch.equal(ms[light], mn[light]), tag
        z1p, zp, b1, bd = R.layer_fwd64(x, c.A, W, b, Wr, br, c.mean, relu1, relu2, pre=True)
        zr = zp.clamp_min(0) if relu2 else zp
        for Z, how in ((Zs, "scheduled"), (Zn, "natural")):
            hold("Z heavy rows", Z[~light], zr[~light], bd[~light], TOL, f"{tag} {how}")
        check_forward("schedule", Zn, mn, z1p, zp, b1, bd, relu2, TOL, tag + " natural")


# --------------------------------------------------------------- 3. backward
def run_layer_bwd(c, dZs, masks, relu1, relu2, W, Wr, ld=40, lddh=72):
    from mgcn import _lib as L
    dev = dZs.device
    dX, dXbuf = R.strided(c.N, F, ld, dev)
    DH, DHbuf = R.strided(c.N, 2 * F, lddh, dev)
    colsums = torch.full((2 * F,), R.SENT, dtype=torch.int32, device=dev).view(torch.float32)
    ws = torch.empty(R.ws_bytes("residual_layer_bwd", c.N), dtype=torch.uint8, device=dev)
    v = c.plan.bwd
    rc = R.layer_bwd(v, c.norm.w_bwd, c.norm.row_scale_bwd, c.row_div, dZs, masks, relu1, relu2, W,
                     Wr, dX, DH, colsums, ws)
    assert rc == L.OK, R.last_error()
    assert R.untouched(dXbuf[:, F:]) and R.untouched(DHbuf[:, 2 * F:]), "row padding was written"
    assert R.all_written(dX) and R.all_written(DH) and R.all_written(colsums)
    return dX, DH, colsums


@pytest.mark.parametrize("ni", range(len(R.NORMS)))
@pytest.mark.parametrize("gname", sorted(R.GRAPHS))
def test_layer_backward_against_fp64(cuda, gname, ni):
    """mgcn_residual_layer_bwd with the reference's masks: dS exact, dH the
    adjoint SpMM's bits, dX / colsums / dW / dWr within the bound."""
    from mgcn import _lib as L
    from mgcn import ops
    c = case(cuda, gname, ni)
    x, dZ, W, b, Wr, br = R.layer_inputs(c.N, R.case_seed(gname, ni), cuda)
    dZs, _ = R.strided(c.N, F, 40, cuda, dZ)
    v = c.plan.bwd
    with graph_options(gname):
        for relu1, relu2 in R.RELUS:
            tag = f"{gname} {R.NORMS[ni]} relu {relu1, relu2}"
            z1p, zp, _, _ = R.layer_fwd64(x, c.A, W, b, Wr, br, c.mean, relu1, relu2, pre=True)
            m1, m2 = z1p > 0, zp > 0
            dX, DH, colsums = run_layer_bwd(c, dZs, R.masks_words(m1, m2), relu1, relu2, W, Wr)
            ref, bd = R.layer_bwd64(dZ, m1, m2, c.A, W, Wr, x, c.mean, relu1, relu2)
            zero = torch.zeros((), device=cuda)
            dS = torch.where(m2, dZ, zero) if relu2 else dZ
            dA = torch.where(m1, dS, zero) if relu1 else dS
            if c.mean:
                dA = dA / c.plan.in_cnt[:, None]
            assert torch.equal(DH[:, F:], dS), f"dS {tag}"
            dH = ops.spmm_bwd(v, c.norm.w_bwd, c.norm.row_scale_bwd, dA.contiguous(), L.REDUCE_SUM)
            assert torch.equal(DH[:, :F], dH), f"dH is not the adjoint SpMM's {tag}"
            hold("dH", DH[:, :F], ref.dH, bd.dH, TOL, tag)
            hold("dX", dX, ref.dX, bd.dX, TOL, tag)
            hold("db", colsums[:F], ref.db, bd.db, TOL, tag)
            hold("dbr", colsums[F:], ref.dbr, bd.dbr, TOL, tag)
            dW, dWr = ops.gemm_tn_split(x, DH, F)
            g = x.double().t() @ DH.double()
            gb = x.double().abs().t() @ DH.double().abs()
            hold("dW (of DH)", dW, g[:, :F], gb[:, :F], TOL, tag)
            hold("dWr (of DH)", dWr, g[:, F:].t(), gb[:, F:].t(), TOL, tag)
            hold("dW", dW, ref.dW, bd.dW, TOL, tag)
            hold("dWr", dWr, ref.dWr, bd.dWr, TOL, tag)


# ------------------------------------------------------------------ 4. stack
def run_stack_fwd(c, x0s, params, r1, r2, Z=None, masks=None):
    from mgcn import _lib as L
    nl, dev = len(params), x0s.device
    if Z is None:
        Z = torch.full((nl, c.N, F), R.SENT, dtype=torch.int32, device=dev).view(torch.float32)
        masks = torch.full((nl, c.N, 2), R.SENT, dtype=torch.int32, device=dev)
    Ws, bs, Wrs, brs = zip(*params)
    rc = R.stack_fwd(c.plan.fwd, c.norm.w_fwd, x0s, Ws, bs, Wrs, brs, c.reduce, r1, r2, Z, masks)
    assert rc == L.OK, R.last_error()
    return Z, masks


def run_stack_bwd(c, dZs, x0s, Z, masks, params, r1, r2, with_dx0=True, out=None):
    """-> dX0 (or None), G [nl, 2, F, F] = dW[l] | dWr[l], sums [nl, 2 F]."""
    from mgcn import _lib as L
    nl, dev = len(params), dZs.device
    sent = lambda *s: torch.full(s, R.SENT, dtype=torch.int32, device=dev).view(torch.float32)  # noqa: E731
    if out is None:
        dX0, G, sums = sent(c.N, F) if with_dx0 else None, sent(nl, 2, F, F), sent(nl, 2 * F)
        ws = torch.empty(R.ws_bytes("residual_stack_bwd", c.N), dtype=torch.uint8, device=dev)
    else:
        dX0, G, sums, ws = out
    Ws, _, Wrs, _ = zip(*params)
    v = c.plan.bwd
    rc = R.stack_bwd(v, c.norm.w_bwd, c.norm.row_scale_bwd, c.row_div, dZs, x0s, Z, masks, r1, r2,
                     Ws, Wrs, dX0, [G[l, 0] for l in range(nl)], [G[l, 1] for l in range(nl)],
                     sums, ws)
    assert rc == L.OK, R.last_error()
    assert R.all_written(G) and R.all_written(sums) and (dX0 is None or R.all_written(dX0))
    return dX0, G, sums


def stack_reference(c, x0, dZ, params, r1, r2):
    """The fp64 stack, and what mgcn_residual_stack_bwd is fed from it: its Z
    rounded to fp32 and its mask words."""
    fwd = R.stack_fwd64(x0, c.A, params, c.mean, r1, r2)
    bwd = R.stack_bwd64(dZ, x0, fwd, c.A, params, c.mean, r1, r2)
    Zin = torch.stack([f.z.float() for f in fwd]).contiguous()
    min_ = torch.stack([R.masks_words(f.z1p > 0, f.zp > 0) for f in fwd]).contiguous()
    return fwd, bwd, Zin, min_


def check_stack_bwd(bwd, dX0, G, sums, tag, skip=()):
    nl = len(bwd)
    if dX0 is not None:
        hold("stack dX0", dX0, bwd[0][0].dX, bwd[0][1].dX, nl * TOL, tag)
    for l, (v, bd) in enumerate(bwd):
        d = nl - l
        hold("stack dW", G[l, 0], v.dW, bd.dW, d * TOL, f"{tag} layer {l}")
        hold("stack dWr", G[l, 1], v.dWr, bd.dWr, d * TOL, f"{tag} layer {l}")
        hold("stack db", sums[l, :F], v.db, bd.db, d * TOL, f"{tag} layer {l}")
        hold("stack dbr", sums[l, F:], v.dbr, bd.dbr, d * TOL, f"{tag} layer {l}")


@pytest.mark.parametrize("ni", range(len(R.NORMS)))
@pytest.mark.parametrize("nl", R.STACK_DEPTHS)
@pytest.mark.parametrize("gname", R.STACK_GRAPHS)
def test_stack_against_fp64(cuda, gname, nl, ni):
    """Depths 1, 2, 3 and 5 with mixed per-layer flags, strided X0 and dZ,
    dX0 given and NULL: every layer's Z and masks, dX0 and every dW, dWr and
    bias sum against the fp64 stack within the propagated bound, and dX0, dW,
    dWr bit for bit (the sums to fp32 rounding) the layer-by-layer entries."""
    from mgcn import ops
    c = case(cuda, gname, ni)
    x0, dZ, params, r1, r2 = R.stack_inputs(c.N, nl, R.case_seed(gname, ni, nl), cuda, c.A)
    x0s, _ = R.strided(c.N, F, 40, cuda, x0)
    dZs, _ = R.strided(c.N, F, 36, cuda, dZ)
    tag = f"{gname} {R.NORMS[ni]} depth {nl}"
    fwd, bwd, Zin, min_ = stack_reference(c, x0, dZ, params, r1, r2)
    Z, masks = run_stack_fwd(c, x0s, params, r1, r2)
    for l, f in enumerate(fwd):
        check_forward("stack", Z[l], masks[l], f.z1p, f.zp, f.bound1, f.bound, r2[l],
                      (l + 1) * TOL, f"{tag} layer {l}", name="stack Z")
    # layer by layer, top down, through mgcn_residual_layer_bwd
    g, lay = dZs, [None] * nl
    for l in range(nl - 1, -1, -1):
        W, _, Wr, _ = params[l]
        dX, DH, cs = run_layer_bwd(c, g, min_[l], r1[l], r2[l], W, Wr, ld=F, lddh=2 * F)
        lay[l] = (*ops.gemm_tn_split(x0s if l == 0 else Zin[l - 1], DH, F), cs)
        g = dX
    for with_dx0 in (True, False):
        dX0, G, sums = run_stack_bwd(c, dZs, x0s, Zin, min_, params, r1, r2, with_dx0)
        t = f"{tag} dX0 {'given' if with_dx0 else 'NULL'}"
        check_stack_bwd(bwd, dX0, G, sums, t)
        assert dX0 is None or torch.equal(dX0, g), f"dX0 differs from layer by layer, {t}"
        for l, (dW, dWr, cs) in enumerate(lay):
            assert torch.equal(G[l, 0], dW) and torch.equal(G[l, 1], dWr), f"{t} layer {l}"
            torch.testing.assert_close(sums[l], cs, rtol=1e-5,
                                       atol=1e-6 * max(1.0, cs.abs().max().item()))


# ---------------------------------------------------------------- 5. options
@pytest.mark.parametrize("ni", range(len(R.NORMS)))
@pytest.mark.parametrize("name,value,gname", [
    ("residual_fused_mask", 0, "a"), ("gemm_tn_staged", 0, "a"), ("residual_blocks", 64, "a"),
    ("heavy_side_stream", 0, "a"), ("residual_blocks", 64, "g")])
def test_options_keep_the_results(cuda, name, value, gname, ni):
    """A depth-3 stack under each switch: within the fp64 bound, and bit for
    bit the default run wherever the switch leaves the summation order alone.
    residual_fused_mask = 0 computes the same dS / dA in residual_mask_bwd_kernel
    (only the bias sums' partials change); residual_blocks only deals the
    tiles to other workgroups (again the fused sums' partials); gemm_tn_staged
    = 0 folds dW / dWr in gemm_tn_small_kernel's order; heavy_side_stream = 0
    only serialises the giant rows."""
    nl = 3
    c = case(cuda, gname, ni)
    x0, dZ, params, r1, r2 = R.stack_inputs(c.N, nl, R.case_seed(gname, ni, nl), cuda, c.A)
    x0s, _ = R.strided(c.N, F, 40, cuda, x0)
    dZs, _ = R.strided(c.N, F, 36, cuda, dZ)
    tag = f"{name} = {value} on {gname} {R.NORMS[ni]}"
    fwd, bwd, Zin, min_ = stack_reference(c, x0, dZ, params, r1, r2)
    Z0, masks0 = run_stack_fwd(c, x0s, params, r1, r2)
    dX0_0, G0, sums0 = run_stack_bwd(c, dZs, x0s, Zin, min_, params, r1, r2)
    with option(name, value):
        Z, masks = run_stack_fwd(c, x0s, params, r1, r2)
        dX0, G, sums = run_stack_bwd(c, dZs, x0s, Zin, min_, params, r1, r2)
    for l, f in enumerate(fwd):
        check_forward("options", Z[l], masks[l], f.z1p, f.zp, f.bound1, f.bound, r2[l],
                      (l + 1) * TOL, f"{tag} layer {l}", name="stack Z")
    check_stack_bwd(bwd, dX0, G, sums, tag)
    assert torch.equal(Z, Z0) and torch.equal(masks, masks0), tag
    assert torch.equal(dX0, dX0_0), tag
    if name != "gemm_tn_staged":
        assert torch.equal(G, G0), tag
    if name == "heavy_side_stream":
        assert torch.equal(sums, sums0), tag


# ------------------------------------------------------------ 6. guard bands
@pytest.mark.parametrize("ni", range(len(R.NORMS)))
@pytest.mark.parametrize("gname", ["a", "d1", "d17", "d65"])
def test_guard_bands_stay_untouched(cuda, gname, ni):
    """Every output and both workspaces (exactly *_workspace_bytes long)
    between sentinel bands, for the layer, a depth-3 stack and the input
    layer: the bands stay, every output word is written."""
    from mgcn import _lib as L
    from mgcn import ops
    c = case(cuda, gname, ni)
    N, nl = c.N, 3
    G_ = lambda rows, cols: R.Guarded(rows, cols, cuda)  # noqa: E731

    def ws_of(entry):
        nbytes = R.ws_bytes(entry, N)
        assert nbytes % 4 == 0
        g = G_(1, max(nbytes // 4, 1))
        return g, g.t.view(-1).view(torch.uint8)[:nbytes]

    x, dZ, W, b, Wr, br = R.layer_inputs(N, R.case_seed(gname, ni), cuda)
    Z, masks, dX, DH, cs = G_(N, F), G_(N, 2), G_(N, F), G_(N, 2 * F), G_(1, 2 * F)
    wsg, ws = ws_of("residual_layer_bwd")
    mw = masks.t.view(torch.int32)
    fv, bv = c.plan.fwd, c.plan.bwd
    assert R.layer_fwd(fv, c.norm.w_fwd, x, W, b, Wr, br, c.reduce, 1, 1, Z.t, mw) == L.OK
    assert R.layer_bwd(bv, c.norm.w_bwd, c.norm.row_scale_bwd, c.row_div, dZ, mw, 1, 1, W, Wr,
                       dX.t, DH.t, cs.t.view(-1), ws) == L.OK
    guards = {"Z": Z, "masks": masks, "dX": dX, "DH": DH, "colsums": cs, "layer workspace": wsg}

    x0, dZ0, params, r1, r2 = R.stack_inputs(N, nl, R.case_seed(gname, ni, nl), cuda, c.A)
    sZ, sm, sdX, sG, ssum = G_(nl * N, F), G_(nl * N, 2), G_(N, F), G_(nl * 2 * F, F), G_(nl, 2 * F)
    swsg, sws = ws_of("residual_stack_bwd")
    Zt, mt = sZ.t.view(nl, N, F), sm.t.view(torch.int32).view(nl, N, 2)
    run_stack_fwd(c, x0, params, r1, r2, Z=Zt, masks=mt)
    run_stack_bwd(c, dZ0, x0, Zt, mt, params, r1, r2,
                  out=(sdX.t, sG.t.view(nl, 2, F, F), ssum.t, sws))
    guards.update({"stack Z": sZ, "stack masks": sm, "dX0": sdX, "G": sG, "sums": ssum,
                   "stack workspace": swsg})

    xi, dZi, Wi, bi, Wri, bri = R.layer_inputs(N, R.case_seed(gname, ni, 7), cuda, f_in=1)
    a, _ = ops.spmm_fwd(fv, c.norm.w_fwd, xi, c.reduce)
    iZ, grads, da, dxr = G_(N, F), G_(1, 4 * F), G_(1, N), G_(1, N)
    iwsg, iws = ws_of("input_layer_bwd")
    assert R.input_layer_fwd(a.view(-1), xi.view(-1), Wi, bi, Wri, bri, 1, 1, iZ.t) == L.OK
    assert R.input_layer_bwd(dZi, iZ.t, a.view(-1), xi.view(-1), Wi, bi, Wri, 1, 1, c.row_div,
                             da.t.view(-1), dxr.t.view(-1), grads.t.view(-1), iws) == L.OK
    guards.update({"input Z": iZ, "grads": grads, "da": da, "dxr": dxr, "input workspace": iwsg})
    torch.cuda.synchronize()
    for name, g in guards.items():
        assert g.intact(), f"{name}: a guard band was written ({gname}, N = {N})"
        if "workspace" not in name:
            assert R.all_written(g.t), f"{name}: not every word was written"


# ------------------------------------------------------------- 7. rejections
def test_bad_arguments_are_rejected(cuda):
    """Each bad argument returns MGCN_EINVAL (a workspace one byte short: the
    ABI's own code for that, MGCN_EWORKSPACE) with a message, before any
    launch: no output word changes.  n_rows = 0 succeeds and zeroes the sums."""
    from mgcn import _lib as L
    c = case(cuda, "a", 0)
    N, nl = c.N, 2
    fv, bv = c.plan.fwd, c.plan.bwd
    x, dZ, W, b, Wr, br = R.layer_inputs(N, 5, cuda)
    sent = lambda *s: torch.full(s, R.SENT, dtype=torch.int32, device=cuda)  # noqa: E731
    Z, masks, dX, DH, cs = (sent(N, F).view(torch.float32), sent(N + 1, 2),
                            sent(N, F).view(torch.float32), sent(N, 2 * F).view(torch.float32),
                            sent(2 * F).view(torch.float32))
    sZ, smasks = sent(nl, N, F).view(torch.float32), sent(nl * N + 1, 2)
    dX0, G, sums = (sent(N, F).view(torch.float32), sent(nl, 2, F, F).view(torch.float32),
                    sent(nl, 2 * F).view(torch.float32))
    good_masks = torch.zeros(nl * N + 1, 2, dtype=torch.int32, device=cuda)
    ws = torch.empty(R.ws_bytes("residual_layer_bwd", N), dtype=torch.uint8, device=cuda)
    sws = torch.empty(R.ws_bytes("residual_stack_bwd", N), dtype=torch.uint8, device=cuda)
    outs = (Z, masks, dX, DH, cs, sZ, smasks, dX0, G, sums)
    Ws, bs, Wrs, brs = [W] * nl, [b] * nl, [Wr] * nl, [br] * nl
    lf = dict(view=fv, w=c.norm.w_fwd, X=x, W=W, b=b, Wr=Wr, br=br, reduce=c.reduce, relu1=1,
              relu2=1, Z=Z, masks=masks)
    sf = dict(view=fv, w=c.norm.w_fwd, X0=x, Ws=Ws, bs=bs, Wrs=Wrs, brs=brs, reduce=c.reduce,
              relu1s=[1] * nl, relu2s=[1] * nl, Z=sZ, masks=smasks)
    lb = dict(view_t=bv, w_t=c.norm.w_bwd, row_scale=c.norm.row_scale_bwd, row_div=c.row_div,
              dZ=dZ, masks=good_masks, relu1=1, relu2=1, W=W, Wr=Wr, dX=dX, DH=DH, colsums=cs, ws=ws)
    sb = dict(view_t=bv, w_t=c.norm.w_bwd, row_scale=c.norm.row_scale_bwd, row_div=c.row_div,
              dZ=dZ, X0=x, Z=torch.zeros(nl, N, F, device=cuda), masks=good_masks,
              relu1s=[1] * nl, relu2s=[1] * nl, Ws=Ws, Wrs=Wrs, dX0=dX0,
              dWs=[G[l, 0] for l in range(nl)], dWrs=[G[l, 1] for l in range(nl)], sums=sums,
              ws=sws)
    off4 = lambda t: int(t.data_ptr()) + 4  # noqa: E731
    sched = [("n_giant > n_heavy", dict(n_heavy=1, n_giant=2)),
             ("n_heavy > n_rows", dict(n_heavy=N + 1, n_giant=0))]
    cases = [
        (R.layer_fwd, lf, [("F = 16", dict(F=16)), ("reduce = max", dict(reduce=L.REDUCE_MAX)),
                           ("ldx = 34", dict(ldx=34)), ("X + 4 bytes", dict(X=off4(x), ldx=F)),
                           ("Z aliases X", dict(Z=x)), *sched, ("null masks", dict(masks=None)),
                           ("masks + 4 bytes", dict(masks=off4(masks)))]),
        (R.stack_fwd, sf, [("F = 16", dict(F=16)), ("reduce = max", dict(reduce=L.REDUCE_MAX)),
                           ("ldx = 34", dict(ldx=34)), ("X0 + 4 bytes", dict(X0=off4(x), ldx=F)),
                           ("Z aliases X0", dict(Z=x)), *sched, ("null masks", dict(masks=None)),
                           ("masks + 4 bytes", dict(masks=off4(smasks)))]),
        (R.layer_bwd, lb, [("F = 16", dict(F=16)), ("lddz = 34", dict(lddz=34)),
                           ("dZ + 4 bytes", dict(dZ=off4(dZ), lddz=F)), *sched,
                           ("workspace one byte short", dict(ws_bytes=ws.numel() - 1)),
                           ("null masks", dict(masks=None)),
                           ("masks + 4 bytes", dict(masks=off4(good_masks)))]),
        (R.stack_bwd, sb, [("F = 16", dict(F=16)), ("ldx = 34", dict(ldx=34)),
                           ("dZ + 4 bytes", dict(dZ=off4(dZ), lddz=F)), *sched,
                           ("workspace one byte short", dict(ws_bytes=sws.numel() - 1)),
                           ("null masks", dict(masks=None)),
                           ("masks + 4 bytes", dict(masks=off4(good_masks)))]),
    ]
    for fn, base, bad in cases:
        for what, over in bad:
            rc = fn(**{**base, **over})
            want = L.EWORKSPACE if "workspace" in what else L.EINVAL
            assert rc == want, f"{fn.__name__}: {what} returned {rc}"
            assert R.last_error(), f"{fn.__name__}: {what} left no message"
    torch.cuda.synchronize()
    for t in outs:
        assert R.untouched(t), "a rejected call wrote an output"
    # no rows: success, nothing but the sums is touched, and those are zero
    for fn, base in ((R.layer_fwd, lf), (R.stack_fwd, sf), (R.layer_bwd, lb), (R.stack_bwd, sb)):
        assert fn(**{**base, "n_rows": 0}) == L.OK, fn.__name__
    torch.cuda.synchronize()
    for t in (Z, masks, dX, DH, sZ, smasks, dX0):
        assert R.untouched(t)
    assert not bool(cs.any()) and not bool(G.any()) and not bool(sums.any())
    assert R.all_written(cs) and R.all_written(G) and R.all_written(sums)


# ------------------------------------------------------------ 8. input layer
@pytest.mark.parametrize("need_x", [False, True])
@pytest.mark.parametrize("ni", range(len(R.NORMS)))
@pytest.mark.parametrize("gname", R.INPUT_GRAPHS)
def test_input_layer_against_fp64(cuda, gname, ni, need_x):
    """ops._InputLayer (in_channels = 1): Z, dW, db, dWr, dbr and dx against
    the fp64 restatement.  Where a pre-activation is ambiguous the backward
    reference takes the kernel's decision: relu2's from its saved Z, relu1's
    from the forward's arithmetic on its own aggregate (a W + b, each rounded,
    which the backward kernel recomputes bit for bit)."""
    from mgcn import ops
    c = case(cuda, gname, ni)
    x, dZ, W, b, Wr, br = R.layer_inputs(c.N, R.case_seed(gname, ni, 7), cuda, f_in=1)
    a32, _ = ops.spmm_fwd(c.plan.fwd, c.norm.w_fwd, x, c.reduce)
    for kind in R.BIASES:
        bb, bbr = R.pick_bias(kind, b, br)
        for relu1, relu2 in R.RELUS:
            tag = f"{gname} {R.NORMS[ni]} {kind} relu {relu1, relu2} need_x {need_x}"
            xi = x.clone().requires_grad_(need_x)
            ps = [None if p is None else p.clone().requires_grad_(True) for p in (W, bb, Wr, bbr)]
            Z = ops._InputLayer.apply(xi, c.plan, c.norm, c.reduce, relu1, relu2, *ps)
            Z.backward(dZ)
            Z = Z.detach()
            z1p, zp, b1, bd = R.layer_fwd64(x, c.A, W, bb, Wr, bbr, c.mean, relu1, relu2, pre=True)
            hold("input Z", Z, zp.clamp_min(0) if relu2 else zp, bd, TOL, tag)
            amb1, amb2 = R.ambiguous(z1p, b1), R.ambiguous(zp, bd)
            for amb in (amb1, amb2):
                share = float(amb.double().mean())
                SHARES["input layer"] = max(SHARES.get("input layer", 0.0), share)
                assert share <= R.AMBIGUOUS_CAP, f"{tag}: ambiguous share {share:.2e}"
            z1k = a32 * W if bb is None else a32 * W + bb
            m1 = torch.where(amb1, z1k > 0, z1p > 0)
            m2 = torch.where(amb2, Z > 0, zp > 0)
            ref, rb = R.layer_bwd64(dZ, m1, m2, c.A, W, Wr, x, c.mean, relu1, relu2)
            hold("input dW", ps[0].grad, ref.dW, rb.dW, TOL, tag)
            hold("input dWr", ps[2].grad, ref.dWr, rb.dWr, TOL, tag)
            if bb is not None:
                hold("input db", ps[1].grad, ref.db, rb.db, TOL, tag)
            if bbr is not None:
                hold("input dbr", ps[3].grad, ref.dbr, rb.dbr, TOL, tag)
            if need_x:
                hold("input dx", xi.grad, ref.dX, rb.dX, TOL, tag)
            else:
                assert xi.grad is None
