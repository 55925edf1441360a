"""Reference side of the residual layer / stack tests (csrc/residual.hip, the
ResEpi epilogue of the heavy-row kernels, mgcn_input_layer_*): graphs whose
rows sit on every boundary of the kernels, fp64 restatements of the layer, the
stack and their adjoints with |.|-bounds (the convention of fp64_ref.py), the
kernel's ReLU mask words, thin ctypes callers of the six entry points that
leave every pointer, leading dimension and schedule argument to the test, and
the sentinel-guarded buffer.  Imports without a GPU.

The layer (gcn_model.py:89-105 with residual_hop = 1), W [in][out], Wr [out][in]:

    Z1 = relu1((A X) W + b)     R = X Wr^T + br     Z = relu2(Z1 + R)

and its adjoint, with the ReLU decisions m1 = [Z1 > 0], m2 = [Z > 0] given:

    dS = relu2 ? dZ . m2 : dZ        dA = relu1 ? dS . m1 : dS
    dH = A^T dA                      dX = dH W^T + dS Wr
    dW = X^T dH   dWr = dS^T X       db = colsum dA   dbr = colsum dS

(A^T of a mean aggregation divides dA by the in-degree first; db sums the
undivided dA, as the kernels do.)  A bound is the same expression with every
operand replaced by its absolute value and the ReLUs dropped.
"""
import ctypes
from collections import namedtuple

import numpy as np
import torch

from fp64_ref import A64

F = 32
DEFAULT_LADDER = (0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 127, 128, 129, 130, 300, 512,
                  513, 700)


# ------------------------------------------------------------------ graphs
def ladder_graph(N, seed, degrees=DEFAULT_LADDER, extra_edges=None):
    """int64 [2, E] edge list (numpy), shuffled.  With L = len(degrees):

    * row i < L gets exactly degrees[i] in-edges, from random sources >= 2 L
      (multi-edges happen), and one out-edge to a node >= 2 L, so that no
      normalisation gives its in-edges a zero weight;
    * row L + i gets exactly degrees[i] out-edges, to random nodes >= 2 L:
      the backward view has the same ladder;
    * ``extra_edges`` (default 4 N) random edges among the nodes >= 2 L.

    degrees = (): a uniform random graph."""
    rng = np.random.default_rng(seed)
    L = len(degrees)
    if N <= 2 * L and L:
        raise ValueError(f"ladder_graph: N = {N} leaves no node beyond the two ladder blocks")
    if extra_edges is None:
        extra_edges = 4 * N
    lo = 2 * L
    s, d = [], []
    for i, k in enumerate(degrees):
        s += [rng.integers(lo, N, k), np.full(k, L + i)]
        d += [np.full(k, i), rng.integers(lo, N, k)]
    if L:
        s.append(np.arange(L))
        d.append(rng.integers(lo, N, L))
    s.append(rng.integers(lo, N, extra_edges))
    d.append(rng.integers(lo, N, extra_edges))
    ei = np.stack([np.concatenate(s), np.concatenate(d)]).astype(np.int64)
    return np.ascontiguousarray(ei[:, rng.permutation(ei.shape[1])])


def all_heavy_graph(N, degree, seed=0):
    """Every row with exactly ``degree`` in-edges and ``degree`` out-edges
    (a circulant with wrap-around multi-edges), shuffled."""
    rng = np.random.default_rng(seed)
    dst = np.repeat(np.arange(N), degree)
    src = (dst + np.tile(np.arange(1, degree + 1), N)) % N
    ei = np.stack([src, dst]).astype(np.int64)
    return np.ascontiguousarray(ei[:, rng.permutation(ei.shape[1])])


def empty_graph():
    return np.zeros((2, 0), np.int64)


def degrees_of(ei, N):
    """(in-degree, out-degree) int64 [N] of an edge list."""
    return np.bincount(ei[1], minlength=N), np.bincount(ei[0], minlength=N)


class A32(A64):
    """A64's aggregation evaluated in float32 throughout (edge-order
    ``index_add_``): what plain fp32 arithmetic makes of the restatements."""
    dtype = torch.float32

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.w = self.w.float()
        if self.inv_cnt is not None:
            self.cnt = (1.0 / self.inv_cnt).float()

    def apply(self, H, transpose=False, absolute=False):
        H = H.float()
        if transpose and self.inv_cnt is not None:
            H = H / self.cnt[:, None]
        w = self.w.abs() if absolute else self.w
        fr, to = (self.dst, self.src) if transpose else (self.src, self.dst)
        out = torch.zeros(self.N, H.size(1), dtype=torch.float32, device=H.device)
        out.index_add_(0, to, H[fr] * w[:, None])
        if not transpose and self.inv_cnt is not None:
            out = out / self.cnt[:, None]
        return out


def make_A(ei, N, deg_norm, aggr, dev, cls=A64):
    """The aggregation operator of (edge list, normalisation, add / mean) with
    the C oracle's per-edge weights."""
    from oracle import oracle as orc
    wf, _, _ = orc.edge_factors(ei, N, deg_norm)
    return cls(torch.from_numpy(ei), wf, N, dev, mean=aggr == "mean")


# ------------------------------------------------------------- restatements
def _dt(A):
    return getattr(A, "dtype", torch.float64)


def _c(t, dt):
    return None if t is None else t.to(dt)


def layer_fwd64(x, A, W, b, Wr, br, mean, relu1, relu2, x_bound=None, pre=False):
    """-> z1, z, bound1, bound.  ``pre``: the two pre-activations instead (the
    values the mask bits and the ambiguity test are about).  ``x_bound``: a
    bound of |x| in place of |x| (the stack: the previous layer's bound)."""
    assert bool(mean) == (A.inv_cnt is not None)
    dt = _dt(A)
    x, W, b, Wr, br = (_c(t, dt) for t in (x, W, b, Wr, br))
    xb = x.abs() if x_bound is None else x_bound.to(dt)
    z1 = A.apply(x) @ W
    bound1 = A.apply(xb, absolute=True) @ W.abs()
    if b is not None:
        z1, bound1 = z1 + b, bound1 + b.abs()
    r = x @ Wr.t()
    rb = xb @ Wr.abs().t()
    if br is not None:
        r, rb = r + br, rb + br.abs()
    z = (z1.clamp_min(0) if relu1 else z1) + r
    bound = bound1 + rb
    if pre:
        return z1, z, bound1, bound
    return (z1.clamp_min(0) if relu1 else z1), (z.clamp_min(0) if relu2 else z), bound1, bound


Bwd = namedtuple("Bwd", "dS dA dH dX dW dWr db dbr")


def layer_bwd64(dZ, m1, m2, A, W, Wr, x, mean, relu1, relu2, dZ_bound=None):
    """-> (values, bounds), two ``Bwd`` tuples.  ``dZ_bound``: a bound of |dZ|
    in place of |dZ| (the stack: the bound of the layer above's dX)."""
    assert bool(mean) == (A.inv_cnt is not None)
    dt = _dt(A)
    dZ, W, Wr, x = (_c(t, dt) for t in (dZ, W, Wr, x))
    g = dZ.abs() if dZ_bound is None else dZ_bound.to(dt)
    dS = dZ * m2.to(dt) if relu2 else dZ
    dA = dS * m1.to(dt) if relu1 else dS
    dH = A.apply(dA, transpose=True)
    bH = A.apply(g, transpose=True, absolute=True)
    xa = x.abs()
    vals = Bwd(dS, dA, dH, dH @ W.t() + dS @ Wr, x.t() @ dH, dS.t() @ x, dA.sum(0), dS.sum(0))
    bounds = Bwd(g, g, bH, bH @ W.abs().t() + g @ Wr.abs(), xa.t() @ bH, g.t() @ xa, g.sum(0),
                 g.sum(0))
    return vals, bounds


Fwd = namedtuple("Fwd", "z1p zp z bound1 bound")


def stack_fwd64(x0, A, params, mean, relu1s, relu2s):
    """-> one ``Fwd`` per layer (pre-activations, output, bounds); params =
    [(W, b, Wr, br), ...].  Layer l's input bound is layer l-1's bound."""
    out, x, xb = [], x0, None
    for (W, b, Wr, br), r1, r2 in zip(params, relu1s, relu2s):
        z1p, zp, b1, bd = layer_fwd64(x, A, W, b, Wr, br, mean, r1, r2, x_bound=xb, pre=True)
        z = zp.clamp_min(0) if r2 else zp
        out.append(Fwd(z1p, zp, z, b1, bd))
        x, xb = z, bd
    return out


def stack_bwd64(dZ, x0, fwd, A, params, mean, relu1s, relu2s, masks=None):
    """-> [(values, bounds)] per layer, from the outputs ``fwd`` of
    :func:`stack_fwd64`; ``masks`` [(m1, m2)] replaces the decisions taken from
    ``fwd``.  The bound of layer l-1's dZ is the bound of layer l's dX."""
    nl = len(params)
    out = [None] * nl
    g, gb = dZ, None
    for l in range(nl - 1, -1, -1):
        W, _, Wr, _ = params[l]
        m1, m2 = masks[l] if masks is not None else (fwd[l].z1p > 0, fwd[l].zp > 0)
        x = x0 if l == 0 else fwd[l - 1].z
        out[l] = layer_bwd64(g, m1, m2, A, W, Wr, x, mean, relu1s[l], relu2s[l], dZ_bound=gb)
        g, gb = out[l][0].dX, out[l][1].dX
    return out


def ambiguous(zp, bound, tol=1e-5):
    """Pre-activations whose sign fp32 rounding may decide either way: within
    ``tol`` of the bound of zero.  An exact zero of the reference is none (a
    row that aggregates rows the ReLU has emptied, without a bias): its bit
    is held to 0 like any other."""
    return (bound > 0) & (zp != 0) & (zp.abs() <= tol * bound)


# ------------------------------------------------------------------- masks
def masks_words(m1, m2):
    """int32 [N, 2] in the kernel's format: bit c of word 0 <=> m1[:, c], of
    word 1 <=> m2[:, c] (m1, m2 bool [N, 32])."""
    sh = torch.arange(32, device=m1.device, dtype=torch.int64)
    w = torch.stack([(m.to(torch.int64) << sh).sum(1) for m in (m1, m2)], dim=1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def words_bits(words):
    """The inverse: bool [N, 2, 32] of int32 [N, 2]."""
    sh = torch.arange(32, device=words.device, dtype=torch.int64)
    return ((words.to(torch.int64)[..., None] >> sh) & 1).bool()


# -------------------------------------------------------- sentinel buffers
SENT = 0x7FBADBAD  # a NaN bit pattern no kernel writes
BAND = 4096


class Guarded:
    """A [rows, cols] float32 tensor between two bands of sentinel words."""

    def __init__(self, rows, cols, dev):
        self.base = torch.full((BAND + rows * cols + BAND,), SENT, dtype=torch.int32, device=dev)
        self.t = self.base[BAND:BAND + rows * cols].view(torch.float32).view(rows, cols)

    def intact(self):
        b = self.base
        return bool((b[:BAND] == SENT).all()) and bool((b[b.numel() - BAND:] == SENT).all())


def strided(rows, cols, ld, dev, src=None):
    """(view [rows, cols], buffer [rows, ld]): rows ``ld`` floats apart in a
    buffer of sentinel words, the view filled from ``src`` if given."""
    buf = torch.full((max(rows, 1), ld), SENT, dtype=torch.int32, device=dev).view(torch.float32)
    v = buf[:rows, :cols]
    if src is not None:
        v.copy_(src)
    return v, buf


def untouched(t):
    """Every word of ``t`` still the sentinel."""
    return bool((t.view(torch.int32) == SENT).all())


def all_written(t):
    return not bool((t.view(torch.int32) == SENT).any())


# --------------------------------------------------------- ctypes callers
PLAN = object()  # order / n_heavy / n_giant: the view's own schedule


def _p(t):
    if t is None:
        return None
    if isinstance(t, int):
        return ctypes.c_void_p(t)
    return ctypes.c_void_p(t.data_ptr())


def _ld(t, ld):
    return int(ld) if ld is not None else int(t.stride(0))


def _sched(view, order, n_heavy, n_giant):
    if order is PLAN:
        order = view.order
    return (_p(order), view.n_heavy if n_heavy is None else n_heavy,
            view.n_giant if n_giant is None else n_giant)


def _ptrs(ts):
    arr = (ctypes.c_void_p * max(len(ts), 1))(*[None if t is None else t.data_ptr() for t in ts])
    return arr


def _ints(vals):
    return (ctypes.c_int32 * max(len(vals), 1))(*[int(bool(v)) for v in vals])


def _lib_dev(*ts):
    from mgcn import _lib as L
    dev = next(t.device for t in ts if isinstance(t, torch.Tensor))
    return L.load(), L.stream_of(dev)


def last_error():
    from mgcn import _lib as L
    return L.load().mgcn_last_error().decode(errors="replace")


def layer_fwd(view, w, X, W, b, Wr, br, reduce, relu1, relu2, Z, masks, order=PLAN, n_heavy=None,
              n_giant=None, n_rows=None, F=F, ldx=None, ldz=None, ldw=None, ldwr=None):
    """mgcn_residual_layer_fwd -> its return code.  Tensors, ints (raw
    addresses) or None for pointers; ld* default to the tensors' strides."""
    lib, s = _lib_dev(view.rowptr)
    o, nh, ng = _sched(view, order, n_heavy, n_giant)
    return lib.mgcn_residual_layer_fwd(
        view.n_rows if n_rows is None else n_rows, F, _p(view.rowptr), _p(view.col), _p(view.eid),
        _p(w), _p(X), _ld(X, ldx), _p(W), _ld(W, ldw), _p(b), _p(Wr), _ld(Wr, ldwr), _p(br),
        int(reduce), int(relu1), int(relu2), _p(Z), _ld(Z, ldz), _p(masks), o, nh, ng, s)


def layer_bwd(view_t, w_t, row_scale, row_div, dZ, masks, relu1, relu2, W, Wr, dX, DH, colsums,
              ws, ws_bytes=None, order=PLAN, n_heavy=None, n_giant=None, n_rows=None, F=F,
              lddz=None, lddx=None, lddh=None):
    """mgcn_residual_layer_bwd -> its return code."""
    lib, s = _lib_dev(view_t.rowptr)
    o, nh, ng = _sched(view_t, order, n_heavy, n_giant)
    return lib.mgcn_residual_layer_bwd(
        view_t.n_rows if n_rows is None else n_rows, F, _p(view_t.rowptr), _p(view_t.col),
        _p(view_t.eid), _p(w_t), _p(row_scale), _p(row_div), _p(dZ), _ld(dZ, lddz), _p(masks),
        int(relu1), int(relu2), _p(W), W.stride(0), _p(Wr), Wr.stride(0), _p(dX), _ld(dX, lddx),
        _p(DH), _ld(DH, lddh), _p(colsums), o, nh, ng, _p(ws),
        int(ws.numel() * ws.element_size()) if ws_bytes is None else ws_bytes, s)


def stack_fwd(view, w, X0, Ws, bs, Wrs, brs, reduce, relu1s, relu2s, Z, masks, order=PLAN,
              n_heavy=None, n_giant=None, n_rows=None, F=F, ldx=None):
    """mgcn_residual_stack_fwd -> its return code (Z [nl, n, F], masks [nl, n, 2])."""
    lib, s = _lib_dev(view.rowptr)
    o, nh, ng = _sched(view, order, n_heavy, n_giant)
    keep = [_ptrs(Ws), _ptrs(bs), _ptrs(Wrs), _ptrs(brs), _ints(relu1s), _ints(relu2s)]
    pw, pb, pwr, pbr, r1, r2 = (ctypes.cast(a, ctypes.c_void_p) for a in keep)
    return lib.mgcn_residual_stack_fwd(
        view.n_rows if n_rows is None else n_rows, F, len(Ws), _p(view.rowptr), _p(view.col),
        _p(view.eid), _p(w), _p(X0), _ld(X0, ldx), pw, pb, pwr, pbr, int(reduce), r1, r2, _p(Z),
        _p(masks), o, nh, ng, s)


def stack_bwd(view_t, w_t, row_scale, row_div, dZ, X0, Z, masks, relu1s, relu2s, Ws, Wrs, dX0,
              dWs, dWrs, sums, ws, ws_bytes=None, order=PLAN, n_heavy=None, n_giant=None,
              n_rows=None, F=F, lddz=None, ldx=None):
    """mgcn_residual_stack_bwd -> its return code (dWs / dWrs: one [F, F]
    tensor per layer, sums [nl, 2 F])."""
    lib, s = _lib_dev(view_t.rowptr)
    o, nh, ng = _sched(view_t, order, n_heavy, n_giant)
    keep = [_ptrs(Ws), _ptrs(Wrs), _ptrs(dWs), _ptrs(dWrs), _ints(relu1s), _ints(relu2s)]
    pw, pwr, pdw, pdwr, r1, r2 = (ctypes.cast(a, ctypes.c_void_p) for a in keep)
    return lib.mgcn_residual_stack_bwd(
        view_t.n_rows if n_rows is None else n_rows, F, len(Ws), _p(view_t.rowptr), _p(view_t.col),
        _p(view_t.eid), _p(w_t), _p(row_scale), _p(row_div), _p(dZ), _ld(dZ, lddz), _p(X0),
        _ld(X0, ldx), _p(Z), _p(masks), r1, r2, pw, pwr, _p(dX0), pdw, pdwr, _p(sums), o, nh, ng,
        _p(ws), int(ws.numel() * ws.element_size()) if ws_bytes is None else ws_bytes, s)


def input_layer_fwd(a, x, W, b, Wr, br, relu1, relu2, Z, ldz=None, F=F):
    """mgcn_input_layer_fwd -> its return code (a = A x and x are [n])."""
    lib, s = _lib_dev(a)
    return lib.mgcn_input_layer_fwd(a.numel(), F, _p(a), _p(x), _p(W), _p(b), _p(Wr), _p(br),
                                    int(relu1), int(relu2), _p(Z), _ld(Z, ldz), s)


def input_layer_bwd(dZ, Z, a, x, W, b, Wr, relu1, relu2, row_div, da, dxr, grads, ws,
                    ws_bytes=None, lddz=None, ldz=None, F=F):
    """mgcn_input_layer_bwd -> its return code (grads [4 F]: dW | db | dWr | dbr)."""
    lib, s = _lib_dev(a)
    return lib.mgcn_input_layer_bwd(
        a.numel(), F, _p(dZ), _ld(dZ, lddz), _p(Z), _ld(Z, ldz), _p(a), _p(x), _p(W), _p(b),
        _p(Wr), int(relu1), int(relu2), _p(row_div), _p(da), _p(dxr), _p(grads), _p(ws),
        int(ws.numel() * ws.element_size()) if ws_bytes is None else ws_bytes, s)


def ws_bytes(name, n, F=F):
    """``mgcn_<name>_workspace_bytes(n, F)``."""
    from mgcn import _lib as L
    return int(getattr(L.load(), f"mgcn_{name}_workspace_bytes")(n, F))


# ------------------------------------------------------------------- cases
# The graphs of tests/test_gpu_residual_shapes.py (and of the host checks of
# the same cases): name -> (N, edge list builder).
LADDER_128 = tuple(d for d in DEFAULT_LADDER if d <= 128)
LADDER_300 = tuple(d for d in DEFAULT_LADDER if d <= 300)
UNIFORM_N = (1, 15, 16, 17, 63, 64, 65, 130)
GRAPHS = {
    "a": (700, lambda: ladder_graph(700, 1)),
    "b": (300, lambda: ladder_graph(300, 2, LADDER_128)),
    "c": (500, lambda: ladder_graph(500, 3, LADDER_300)),
    "e": (40, lambda: all_heavy_graph(40, 130, 6)),
    "f": (65, empty_graph),
    "g": (4200, lambda: ladder_graph(4200, 5, (), 3 * 4200)),
}
for _n in UNIFORM_N:
    GRAPHS[f"d{_n}"] = (_n, (lambda n: lambda: ladder_graph(n, 40 + n, (), 4 * n))(_n))
STACK_GRAPHS = ("a", "b", "d65", "e", "f")
STACK_DEPTHS = (1, 2, 3, 5)
INPUT_GRAPHS = ("a", "d17", "d65", "f")
TOL = 1e-5        # per layer, of the |.|-bound (fp64_ref.within)
AMBIGUOUS_CAP = 1e-3
NORMS = (("sm", "add"), ("rw", "mean"), (None, "mean"))
RELUS = ((True, True), (True, False), (False, True))
BIASES = ("both", "none", "rbias")
BIAS_U = (0.3, 0.4)  # bias = -(0.3 + 0.4 rand) x column median, see stack_inputs
SCALE = 0.3  # of the weights and biases (randn); inputs are randn


def case_seed(gname, ni, extra=0):
    """The input seed of (graph, NORMS[ni]): the host checks of a case's inputs
    (ambiguous share, fp32 margin) and the GPU test draw the same tensors."""
    return 1000 * extra + 10 * sorted(GRAPHS).index(gname) + ni + 1


def layer_inputs(N, seed, dev, f_in=F):
    """x [N, f_in], dZ [N, F], W [f_in, F], b, Wr [F, f_in], br: float32 on ``dev``,
    drawn on the CPU (the same values with and without a GPU)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    t = [r(N, f_in), r(N, F), r(f_in, F) * SCALE, r(F) * SCALE, r(F, f_in) * SCALE, r(F) * SCALE]
    return [v.to(dev) for v in t]


def pick_bias(kind, b, br):
    return {"both": (b, br), "none": (None, None), "rbias": (None, br)}[kind]


# per depth: relu1 / relu2 of every layer and which layers go without bias / rbias
STACK_FLAGS = {
    1: ((True,), (False,), (), ()),
    2: ((True, True), (False, True), (0,), (1,)),
    3: ((True, False, True), (True, True, False), (2,), (0,)),
    5: ((True, False, True, True, True), (True, True, False, True, False), (3,), (1,)),
}


def stack_inputs(N, nl, seed, dev, A):
    """x0, dZ and [(W, b, Wr, br)] of a stack of depth ``nl`` with the flags of
    STACK_FLAGS -> x0, dZ, params, relu1s, relu2s.

    The |.|-bound of a stack drops every ReLU and every cancellation, layer
    after layer: with weights of random sign it outgrows the values about
    tenfold per layer, and by the fifth layer TOL times the bound covers a
    fifth of the pre-activations (measured), far above AMBIGUOUS_CAP.  So the
    stack cases keep the cancellation in the biases alone: x0, W and Wr are
    non-negative (|randn|, the weights scaled by SCALE), and every bias is
    minus the column medians of the term it joins (evaluated in fp64 with
    ``A``), times a random factor in [0.3, 0.7] -- a fifth to a third of the
    ReLU decisions of a layer fall on the zero side, row by row, and bound
    and value stay within a factor the cap can take (biases at the medians
    themselves: 4e-3 of the fifth layer ambiguous).  dZ is randn."""
    r1, r2, no_b, no_br = STACK_FLAGS[nl]
    mean = A.inv_cnt is not None
    adev = A.src.device
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    u = lambda: BIAS_U[0] + BIAS_U[1] * torch.rand(F, generator=g).double()  # noqa: E731
    x0, dZ = r(N, F).abs(), r(N, F)
    params = []
    x = x0.double().to(adev)
    for l in range(nl):
        W, Wr = r(F, F).abs() * SCALE, r(F, F).abs() * SCALE
        ub, ubr = u().to(adev), u().to(adev)
        b = br = None
        if l not in no_b:
            h, _, _, _ = layer_fwd64(x, A, W.to(adev), None, Wr.to(adev), None, mean, False, False,
                                     pre=True)
            b = (-h.median(0).values * ub).float()
        if l not in no_br:
            _, z, _, _ = layer_fwd64(x, A, W.to(adev), b, Wr.to(adev), None, mean, r1[l], False,
                                     pre=True)
            br = (-z.median(0).values * ubr).float()
        _, x, _, _ = layer_fwd64(x, A, W.to(adev), b, Wr.to(adev), br, mean, r1[l], r2[l])
        params.append((W.to(dev), None if b is None else b.to(dev), Wr.to(dev),
                       None if br is None else br.to(dev)))
    return x0.to(dev), dZ.to(dev), params, r1, r2
