"""Host checks of tests/residual_ref.py, the reference side of
test_gpu_residual_shapes.py (no GPU):

  * the adjoint restatements equal torch.autograd of the forward ones in fp64;
  * the margin is real: the same restatements evaluated in plain fp32 on the
    CPU stay within a quarter of the bound the GPU tests hold the kernels to;
  * the inputs of every GPU case leave at most AMBIGUOUS_CAP of the ReLU
    decisions to fp32 rounding;
  * the graphs have the degrees they promise and the mask words round-trip.
"""
import numpy as np
import pytest
import torch

import residual_ref as R
from fp64_ref import within

CPU = torch.device("cpu")
F = R.F


def _rel(a, b, bound):
    """max |a - b| / bound over the elements with a nonzero bound (0 where
    the bound is 0 the values must agree exactly)."""
    err = (a - b).abs()
    assert bool((err[bound == 0] == 0).all())
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if bool(nz.any()) else 0.0


@pytest.fixture(scope="module")
def small():
    N = 60
    ei = R.ladder_graph(N, 9, (0, 1, 3, 5, 9, 17), 200)
    return N, ei


@pytest.mark.parametrize("ni", range(len(R.NORMS)))
@pytest.mark.parametrize("relu1,relu2", R.RELUS)
def test_layer_bwd64_is_autograd_of_layer_fwd64(small, ni, relu1, relu2):
    N, ei = small
    deg_norm, aggr = R.NORMS[ni]
    A = R.make_A(ei, N, deg_norm, aggr, CPU)
    x, dZ, W, b, Wr, br = [t.double().requires_grad_(True) for t in R.layer_inputs(N, 3 + ni, CPU)]
    z1p, zp, _, _ = R.layer_fwd64(x, A, W, b, Wr, br, aggr == "mean", relu1, relu2, pre=True)
    _, z, _, _ = R.layer_fwd64(x, A, W, b, Wr, br, aggr == "mean", relu1, relu2)
    z.backward(dZ.detach())
    v, bd = R.layer_bwd64(dZ.detach(), z1p.detach() > 0, zp.detach() > 0, A, W.detach(),
                          Wr.detach(), x.detach(), aggr == "mean", relu1, relu2)
    for name, ref in (("dX", x.grad), ("dW", W.grad), ("dWr", Wr.grad), ("db", b.grad),
                      ("dbr", br.grad)):
        r = _rel(getattr(v, name), ref, getattr(bd, name))
        assert r <= 1e-12, (name, r)


@pytest.mark.parametrize("ni", range(len(R.NORMS)))
@pytest.mark.parametrize("nl", R.STACK_DEPTHS)
def test_stack_bwd64_is_autograd_of_stack_fwd64(small, ni, nl):
    N, ei = small
    deg_norm, aggr = R.NORMS[ni]
    mean = aggr == "mean"
    A = R.make_A(ei, N, deg_norm, aggr, CPU)
    x0, dZ, params, r1, r2 = R.stack_inputs(N, nl, 5 + ni, CPU, A)
    x0 = x0.double().requires_grad_(True)
    params = [tuple(None if p is None else p.double().requires_grad_(True) for p in q)
              for q in params]
    fwd = R.stack_fwd64(x0, A, params, mean, r1, r2)
    fwd[-1].z.backward(dZ.double())
    det = [tuple(None if p is None else p.detach() for p in q) for q in params]
    fd = [R.Fwd(*[t.detach() for t in f]) for f in fwd]
    out = R.stack_bwd64(dZ.double(), x0.detach(), fd, A, det, mean, r1, r2)
    assert _rel(out[0][0].dX, x0.grad, out[0][1].dX) <= 1e-12
    for l, (W, b, Wr, br) in enumerate(params):
        v, bd = out[l]
        pairs = [("dW", W.grad), ("dWr", Wr.grad)]
        if b is not None:
            pairs.append(("db", b.grad))
        if br is not None:
            pairs.append(("dbr", br.grad))
        for name, ref in pairs:
            r = _rel(getattr(v, name), ref, getattr(bd, name))
            assert r <= 1e-12, (l, name, r)


@pytest.fixture(scope="module")
def ladder():
    N, build = R.GRAPHS["a"]
    return N, build()


@pytest.mark.parametrize("ni", range(len(R.NORMS)))
def test_fp32_restatement_of_the_layer_uses_a_quarter_of_the_bound(ladder, ni):
    """Every tensor of the layer, fp32 on the CPU against fp64, on the ladder
    graph at N = 700: worst err / (TOL bound + atol) <= 0.25."""
    N, ei = ladder
    deg_norm, aggr = R.NORMS[ni]
    mean = aggr == "mean"
    A, A32 = R.make_A(ei, N, deg_norm, aggr, CPU), R.make_A(ei, N, deg_norm, aggr, CPU, R.A32)
    x, dZ, W, b, Wr, br = R.layer_inputs(N, R.case_seed("a", ni), CPU)
    worst = {}
    for relu1, relu2 in R.RELUS:
        z1p, zp, _, _ = R.layer_fwd64(x, A, W, b, Wr, br, mean, relu1, relu2, pre=True)
        _, z, _, bound = R.layer_fwd64(x, A, W, b, Wr, br, mean, relu1, relu2)
        _, z32, _, _ = R.layer_fwd64(x, A32, W, b, Wr, br, mean, relu1, relu2)
        assert z32.dtype == torch.float32
        worst["Z"] = max(worst.get("Z", 0.0), within(z32.double() - z, bound, R.TOL)[1])
        m1, m2 = z1p > 0, zp > 0
        v, bd = R.layer_bwd64(dZ, m1, m2, A, W, Wr, x, mean, relu1, relu2)
        v32, _ = R.layer_bwd64(dZ, m1, m2, A32, W, Wr, x, mean, relu1, relu2)
        for name in R.Bwd._fields:
            r = within(getattr(v32, name).double() - getattr(v, name), getattr(bd, name), R.TOL)[1]
            worst[name] = max(worst.get(name, 0.0), r)
    print("fp32 / limit, layer,", R.NORMS[ni], {k: round(v, 4) for k, v in worst.items()})
    assert max(worst.values()) <= 0.25, worst


@pytest.mark.parametrize("ni", range(len(R.NORMS)))
def test_fp32_restatement_of_the_stack_uses_a_quarter_of_the_bound(ladder, ni):
    """The same for a stack of depth 5 with the propagated bounds: Z[l] at
    (l + 1) TOL, dX0 at nl TOL, dW[l] / dWr[l] / sums[l] at (nl - l) TOL."""
    N, ei = ladder
    nl = 5
    deg_norm, aggr = R.NORMS[ni]
    mean = aggr == "mean"
    A, A32 = R.make_A(ei, N, deg_norm, aggr, CPU), R.make_A(ei, N, deg_norm, aggr, CPU, R.A32)
    x0, dZ, params, r1, r2 = R.stack_inputs(N, nl, R.case_seed("a", ni, nl), CPU, A)
    fwd = R.stack_fwd64(x0, A, params, mean, r1, r2)
    fwd32 = R.stack_fwd64(x0, A32, params, mean, r1, r2)
    worst = {}
    for l in range(nl):
        worst[f"Z{l}"] = within(fwd32[l].z.double() - fwd[l].z, fwd[l].bound, (l + 1) * R.TOL)[1]
    masks = [(f.z1p > 0, f.zp > 0) for f in fwd]
    out = R.stack_bwd64(dZ, x0, fwd, A, params, mean, r1, r2)
    out32 = R.stack_bwd64(dZ, x0, fwd, A32, params, mean, r1, r2, masks=masks)
    worst["dX0"] = within(out32[0][0].dX.double() - out[0][0].dX, out[0][1].dX, nl * R.TOL)[1]
    for l in range(nl):
        for name in ("dW", "dWr", "db", "dbr"):
            worst[f"{name}{l}"] = within(getattr(out32[l][0], name).double() -
                                         getattr(out[l][0], name), getattr(out[l][1], name),
                                         (nl - l) * R.TOL)[1]
    print("fp32 / limit, stack,", R.NORMS[ni], {k: round(v, 4) for k, v in worst.items()})
    assert max(worst.values()) <= 0.25, worst


def _share(zp, bound):
    return float(R.ambiguous(zp, bound).double().mean()) if zp.numel() else 0.0


@pytest.mark.parametrize("gname", sorted(R.GRAPHS))
def test_ambiguous_share_of_the_layer_cases(gname):
    """The share of pre-activations within TOL bound of zero, for the inputs
    of every layer case of the GPU tests (forward, backward, options, guards)."""
    N, build = R.GRAPHS[gname]
    ei = build()
    worst = 0.0
    for ni, (deg_norm, aggr) in enumerate(R.NORMS):
        A = R.make_A(ei, N, deg_norm, aggr, CPU)
        x, _, W, b, Wr, br = R.layer_inputs(N, R.case_seed(gname, ni), CPU)
        for kind in R.BIASES:
            bb, bbr = R.pick_bias(kind, b, br)
            for relu1, relu2 in R.RELUS:
                z1p, zp, b1, bd = R.layer_fwd64(x, A, W, bb, Wr, bbr, aggr == "mean", relu1,
                                                relu2, pre=True)
                worst = max(worst, _share(z1p, b1), _share(zp, bd))
    print("ambiguous share, layer,", gname, worst)
    assert worst <= R.AMBIGUOUS_CAP, worst


@pytest.mark.parametrize("gname", R.STACK_GRAPHS + ("g",))
def test_ambiguous_share_of_the_stack_cases(gname):
    N, build = R.GRAPHS[gname]
    ei = build()
    worst = 0.0
    for ni, (deg_norm, aggr) in enumerate(R.NORMS):
        A = R.make_A(ei, N, deg_norm, aggr, CPU)
        for nl in R.STACK_DEPTHS:
            x0, _, params, r1, r2 = R.stack_inputs(N, nl, R.case_seed(gname, ni, nl), CPU, A)
            for f in R.stack_fwd64(x0, A, params, aggr == "mean", r1, r2):
                worst = max(worst, _share(f.z1p, f.bound1), _share(f.zp, f.bound))
    print("ambiguous share, stack,", gname, worst)
    assert worst <= R.AMBIGUOUS_CAP, worst


@pytest.mark.parametrize("gname", R.INPUT_GRAPHS)
def test_ambiguous_share_of_the_input_layer_cases(gname):
    N, build = R.GRAPHS[gname]
    ei = build()
    worst = 0.0
    for ni, (deg_norm, aggr) in enumerate(R.NORMS):
        A = R.make_A(ei, N, deg_norm, aggr, CPU)
        x, _, W, b, Wr, br = R.layer_inputs(N, R.case_seed(gname, ni, 7), CPU, f_in=1)
        for kind in R.BIASES:
            bb, bbr = R.pick_bias(kind, b, br)
            for relu1, relu2 in R.RELUS:
                z1p, zp, b1, bd = R.layer_fwd64(x, A, W, bb, Wr, bbr, aggr == "mean", relu1,
                                                relu2, pre=True)
                worst = max(worst, _share(z1p, b1), _share(zp, bd))
    print("ambiguous share, input layer,", gname, worst)
    assert worst <= R.AMBIGUOUS_CAP, worst


def test_ladder_graph_degrees():
    N, build = R.GRAPHS["a"]
    ei = build()
    L = len(R.DEFAULT_LADDER)
    din, dout = R.degrees_of(ei, N)
    assert tuple(din[:L]) == R.DEFAULT_LADDER and tuple(dout[L:2 * L]) == R.DEFAULT_LADDER
    assert ei.min() >= 0 and ei.max() < N
    # no ladder row is touched by another edge: its in-edges come from, and
    # every other edge ends, beyond the two blocks
    assert (ei[1][ei[1] < L].size == sum(R.DEFAULT_LADDER)) and not ((ei[1] >= L) & (ei[1] < 2 * L)).any()
    assert (dout[:L] == 1).all()
    N, build = R.GRAPHS["e"]
    din, dout = R.degrees_of(build(), N)
    assert (din == 130).all() and (dout == 130).all()
    assert max(R.LADDER_128) == 128 and max(R.LADDER_300) == 300
    for n in R.UNIFORM_N:
        ei = R.GRAPHS[f"d{n}"][1]()
        assert ei.shape == (2, 4 * n) and ei.max() < n
    assert R.GRAPHS["f"][1]().shape == (2, 0)


def test_masks_words_roundtrip():
    g = torch.Generator().manual_seed(0)
    m1 = torch.rand(50, 32, generator=g) < 0.5
    m2 = torch.rand(50, 32, generator=g) < 0.5
    m1[0], m2[0] = True, False
    m1[1, :] = False
    m1[1, 31] = True  # the sign bit alone
    w = R.masks_words(m1, m2)
    assert w.dtype == torch.int32 and tuple(w.shape) == (50, 2)
    assert int(w[0, 0]) == -1 and int(w[0, 1]) == 0 and int(w[1, 0]) == -2 ** 31
    bits = R.words_bits(w)
    assert torch.equal(bits[:, 0], m1) and torch.equal(bits[:, 1], m2)
    ref = np.array([sum(int(m1[5, c]) << c for c in range(32))], dtype=np.uint32).view(np.int32)
    assert int(w[5, 0]) == int(ref[0])
