"""Block convs on the GPU: ``mgcn.block_aggregate`` (mgcn_block_spmm_fwd /
_bwd) against the shipped path on the edited edge list -- bit for bit, forward
and adjoint --, against the CPU oracle, and the PyG convs on a ``Block``."""
import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 1500
TOP = 140            # rows 0 .. TOP have in-degree = their id
LONG = TOP + 1       # one row of 1000 slots
TWO_LOOPS = 60       # two self loops, at slots 5 and 40 of its row
ONLY_LOOP = 1        # its one edge is its loop
DUP = 50             # slots 3 and 7 of its row are the same edge
SEED, OFFSET = 5, 11
F_ALL = [1, 8, 32, 64, 128, 130, 256]  # G = 4, 4, 8, 16, 32, 64 (two chunks, the last partial), 64


def degree_ladder(n):
    """COO list [2, E] (int64): rows 0 .. 140 with in-degree = id, row 141 with
    1000 slots, every later node with 4; all in one random COO order.  Sources
    are drawn past the ladder, so a ladder node is a source only through its
    planted loops: in the first slot of rows = 2 mod 6, a middle slot of rows =
    3 mod 6 (the long row among them), the last slot of rows = 4 mod 6; node 60
    carries two loops, node 1 only its loop, row 50 one edge twice; every
    fourth node past the ladder has a loop (last in COO order)."""
    rng = np.random.default_rng(0)
    deg = np.concatenate([np.arange(TOP + 1), [1000], np.full(n - LONG - 1, 4)])
    dst = np.repeat(np.arange(n), deg)
    dst = dst[rng.permutation(dst.size)]
    src = rng.integers(LONG + 1, n, dst.size)
    clash = src == dst
    src[clash] = LONG + 1 + (src[clash] - LONG) % (n - LONG - 1)  # the only loops are planted
    for row in range(1, LONG + 1):
        slots = np.flatnonzero(dst == row)
        if row % 6 == 2:
            src[slots[0]] = row
        elif row % 6 == 3:
            src[slots[slots.size // 2]] = row
        elif row % 6 == 4:
            src[slots[-1]] = row
    slots = np.flatnonzero(dst == TWO_LOOPS)
    src[slots[5]] = src[slots[40]] = TWO_LOOPS
    src[np.flatnonzero(dst == ONLY_LOOP)[0]] = ONLY_LOOP
    slots = np.flatnonzero(dst == DUP)
    src[slots[7]] = src[slots[3]]
    rest = np.arange(LONG + 1, n)
    rest = rest[rest % 4 == 0]
    return np.stack([np.concatenate([src, rest]), np.concatenate([dst, rest])]).astype(np.int64)


class Ladder:
    def __init__(self, dev):
        import mgcn
        from mgcn.graph import build_plan
        self.dev = dev
        self.ei_np = degree_ladder(N)
        self.ei = torch.from_numpy(self.ei_np).to(dev)
        self.plan = build_plan(self.ei, N)
        indeg = np.bincount(self.ei_np[1], minlength=N)
        assert [int(indeg[r]) for r in (0, 127, 128, 129, LONG)] == [0, 127, 128, 129, 1000]
        assert int(indeg.max()) == 1000
        rng = np.random.default_rng(1)
        every = torch.from_numpy(rng.permutation(N)).to(dev)
        mixed = np.concatenate([rng.permutation(np.arange(1, 129))[:28], [TWO_LOOPS, ONLY_LOOP],
                                rng.permutation(np.arange(LONG + 1, N))[:10]])
        mixed = torch.from_numpy(rng.permutation(np.unique(mixed))).to(dev)

        def draw(seeds, fanouts):
            return mgcn.sample_blocks(self.plan, seeds, fanouts, seed=SEED, offset=OFFSET)
        (self.full,) = draw(every, [2000])       # every ladder length, n_dst == n_src
        self.hop0, self.hop1 = draw(mixed, [5, 3])  # the common case, n_src > n_dst
        (self.single,) = draw(torch.tensor([TWO_LOOPS], device=dev), [2000])  # n_dst == 1
        assert self.full.n_dst == self.full.n_src == N and self.full.plan.fwd.n_heavy > 0
        assert self.single.n_dst == 1 < self.single.n_src
        for b in (self.hop0, self.hop1):
            assert b.n_src > b.n_dst and b.plan.fwd.n_heavy == 0 == b.plan.bwd.n_heavy
        self.blocks = {"full": self.full, "hop0": self.hop0, "hop1": self.hop1,
                       "single": self.single}
        self._edited = {}

    def local(self, b, node):
        """The local id of parent node ``node`` in block ``b``."""
        (pos,) = torch.nonzero(b.src_ids == node, as_tuple=True)
        assert pos.numel() == 1
        return int(pos)

    def weights(self, b):
        gen = torch.Generator().manual_seed(b.plan.nnz)
        return (torch.rand(b.plan.nnz, generator=gen) * 1.9 + 0.1).to(self.dev)

    def edited(self, name, loops, weighted, fill):
        """(plan, norm) of the shipped path: the block's edge list edited in
        torch, its plan built; made once per case and kept."""
        from mgcn import pyg
        from mgcn.graph import plan_for
        key = (name, loops, weighted, fill)
        if key not in self._edited:
            b = self.blocks[name]
            ew = self.weights(b) if weighted else None
            ei = b.edge_index
            if loops == "drop":
                ei, ew = pyg.remove_self_loops(ei, ew)
            elif loops == "append":
                ei, ew = pyg.add_remaining_self_loops(ei, ew, fill, b.n_src)
            ei = ei.contiguous()
            plan = plan_for(ei, b.n_src)
            self._edited[key] = (ei, plan, plan.norm(None, edge_weight=ew))
        return self._edited[key][1:]


@pytest.fixture(scope="module")
def ladder(cuda):
    import mgcn
    g = Ladder(cuda)
    yield g
    mgcn.clear_cache()


# (loops, weighted, fill): fill only matters where a loop is appended with weights
CASES = [("keep", False, 1.0), ("keep", True, 1.0), ("drop", False, 1.0), ("drop", True, 1.0),
         ("append", False, 1.0), ("append", True, 1.0), ("append", True, 2.0)]


def _features(g, b, F, layout="plain"):
    gen = torch.Generator().manual_seed(100 + F)
    if layout == "ld":  # ldx = F + 1: rows no vector load can take
        return torch.randn(b.n_src, F + 1, generator=gen).to(g.dev)[:, :F]
    if layout == "offset":  # the base pointer 4 bytes past an aligned one
        return torch.randn(b.n_src * F + 1, generator=gen).to(g.dev)[1:].view(b.n_src, F)
    return torch.randn(b.n_src, F, generator=gen).to(g.dev)


def _both(g, name, xb, loops, weighted, fill, aggr):
    """(block_aggregate, the shipped path's rows) for one case."""
    import mgcn
    from mgcn.ops import aggregate_plan
    b = g.blocks[name]
    plan, norm = g.edited(name, loops, weighted, fill)
    got = mgcn.block_aggregate(xb, b, aggr, loops, g.weights(b) if weighted else None, fill)
    return got, aggregate_plan(xb, plan, norm, aggr)[:b.n_dst]


# ------------------------------------------ 1. forward bits, the shipped path
@pytest.mark.parametrize("F,layout", [(F, "plain") for F in F_ALL] +
                         [(32, "ld"), (130, "ld"), (128, "offset"), (8, "offset")])
def test_forward_bits_against_the_shipped_path(ladder, F, layout):
    g = ladder
    for name, b in g.blocks.items():
        xb = _features(g, b, F, layout)
        if layout == "ld":
            assert xb.stride(0) == F + 1
        if layout == "offset":
            assert xb.data_ptr() % 8 == 4
        for loops, weighted, fill in CASES:
            for aggr in ("add", "mean"):
                got, want = _both(g, name, xb, loops, weighted, fill, aggr)
                case = (name, loops, weighted, fill, aggr)
                assert got.shape == (b.n_dst, F) and got.is_contiguous(), case
                assert torch.equal(got, want), case
                assert bool(got.abs().sum() > 0), case


# ------------------------------------------------- 2. forward, the CPU oracle
@pytest.mark.parametrize("weighted", [False, True])
def test_forward_against_the_oracle(ladder, oracle, weighted):
    import mgcn
    g = ladder
    for b in (g.hop0, g.hop1):
        xb = _features(g, b, 32)
        ew = g.weights(b) if weighted else None
        ei2, ew2 = oracle.add_remaining_self_loops(
            b.edge_index.cpu().numpy(), None if ew is None else ew.cpu().numpy(), 1.0, b.n_src)
        want, _ = oracle.aggr_fwd(ei2, xb.cpu().numpy(), ew2, "mean")
        got = mgcn.block_aggregate(xb, b, "mean", "append", ew, 1.0)
        np.testing.assert_array_equal(got.cpu().numpy(), want[:b.n_dst])
        assert bool(got.abs().sum() > 0)


# ------------------------------------------------------------ 3. adjoint bits
@pytest.mark.parametrize("F", [32, 130])
def test_adjoint_bits_against_the_shipped_path(ladder, F):
    g = ladder
    for name, b in g.blocks.items():
        x0 = _features(g, b, F)
        dY = torch.randn(b.n_dst, F, generator=torch.Generator().manual_seed(F)).to(g.dev)
        for loops, weighted, fill in CASES:
            for aggr in ("add", "mean"):
                xa = x0.clone().requires_grad_(True)
                xr = x0.clone().requires_grad_(True)
                got, _ = _both(g, name, xa, loops, weighted, fill, aggr)
                _, want = _both(g, name, xr, loops, weighted, fill, aggr)
                got.backward(dY)
                want.backward(dY)  # the slice feeds zeros to the rows >= n_dst
                case = (name, loops, weighted, fill, aggr)
                assert xa.grad.shape == (b.n_src, F), case
                assert torch.equal(xa.grad, xr.grad), case  # +-0 compare equal: intended
                assert bool(xa.grad.abs().sum() > 0), case


# --------------------------------- 4. a dropped loop is not read into the sum
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("aggr", ["add", "mean"])
def test_a_dropped_loop_never_reaches_the_sum(ladder, aggr, weighted):
    """inf in the rows of destinations that are sources only through their own
    loops (first, middle, last slot; two loops; the loop alone; the long row)."""
    import mgcn
    g, b = ladder, ladder.full
    nodes = [2, 3, 4, 128, 129, TWO_LOOPS, ONLY_LOOP, LONG]
    ei = g.ei_np
    for v in nodes:
        assert ((ei[0] == v) & (ei[1] == v)).any() and not ((ei[0] == v) & (ei[1] != v)).any()
    rows = sorted(g.local(b, v) for v in nodes)
    x = _features(g, b, 8).clone()
    x[rows] = float("inf")
    ew = g.weights(b) if weighted else None
    dY = torch.randn(b.n_dst, 8, generator=torch.Generator().manual_seed(9)).to(g.dev)
    xd = x.clone().requires_grad_(True)
    y = mgcn.block_aggregate(xd, b, aggr, "drop", ew)
    y.backward(dY)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(xd.grad).all())
    assert bool(y.abs().sum() > 0) and bool(xd.grad.abs().sum() > 0)
    ya = mgcn.block_aggregate(x, b, aggr, "append", ew)
    bad = (~torch.isfinite(ya)).any(dim=1)
    assert torch.nonzero(bad).view(-1).tolist() == rows
    assert bool((~torch.isfinite(ya[rows])).all())


# ---------------------------------------------------------- 5. last loop wins
@pytest.mark.parametrize("name", ["single", "full", "hop1"])
def test_the_later_of_two_loops_gives_the_appended_weight(ladder, name):
    import mgcn
    from mgcn import pyg
    g, b = ladder, ladder.blocks[name]
    i = g.local(b, TWO_LOOPS)
    assert i < b.n_dst
    ew = g.weights(b)
    ei = b.edge_index
    (at,) = torch.nonzero((ei[0] == i) & (ei[1] == i), as_tuple=True)
    assert at.numel() == 2 and float(ew[at[0]]) != float(ew[at[1]])
    w_last = ew[at[1]]  # the later one in COO order
    ei2, ew2 = pyg.add_remaining_self_loops(ei, ew, 7.0, b.n_src)
    n_kept = int((ei[0] != ei[1]).sum())
    assert torch.equal(ew2[n_kept + i], w_last)
    # forward: only the node's own row is non-zero, so its sum is the loop term
    x = torch.zeros(b.n_src, 8, device=g.dev)
    x[i] = 1.0
    x.requires_grad_(True)
    y = mgcn.block_aggregate(x, b, "add", "append", ew, 7.0)
    assert torch.equal(y[i], w_last.expand(8))
    # adjoint: only its dY row is non-zero, and it is its own source only by the loop
    dY = torch.zeros(b.n_dst, 8, device=g.dev)
    dY[i] = 1.0
    y.backward(dY)
    assert torch.equal(x.grad[i], w_last.expand(8))


# ------------------------------------------------------------------- 6. convs
@contextlib.contextmanager
def launches():
    """The timer names of the libmgcn launches inside the block."""
    from mgcn.ops import set_kernel_timer
    names = []

    def hook(name, start, rows=None, edges=None):
        if start:
            names.append(name)
    set_kernel_timer(hook)
    try:
        yield names
    finally:
        set_kernel_timer(None)


def _conv(kind, F, dev):
    from mgcn.pyg import GINConv, GraphConv, SAGEConv
    eye = torch.eye(F, device=dev)
    if kind == "sage":
        conv = SAGEConv(F, F).to(dev)
        conv.weight.data.copy_(eye)
    elif kind == "sage_concat":
        conv = SAGEConv(F, F, concat=True).to(dev)
        conv.weight.data.copy_(torch.cat([eye, eye]))
    elif kind == "gin":
        conv = GINConv(torch.nn.Identity(), eps=0.25, train_eps=True).to(dev)
    else:
        conv = GraphConv(F, F, aggr=kind[len("graph_"):]).to(dev)
        conv.weight.data.copy_(eye)
        conv.lin.weight.data.zero_()
        conv.lin.bias.data.zero_()
    return conv


@pytest.mark.parametrize("kind", ["sage", "sage_concat", "gin", "graph_add", "graph_mean"])
@pytest.mark.parametrize("name", ["hop0", "hop1", "full"])
def test_convs_on_a_block_give_the_edge_index_bits(ladder, kind, name):
    g, b = ladder, ladder.blocks[name]
    F = 32
    torch.manual_seed(3)
    conv = _conv(kind, F, g.dev)
    h0 = _features(g, b, F)
    dY = torch.randn(b.n_dst, F, generator=torch.Generator().manual_seed(4)).to(g.dev)
    ew = g.weights(b) if kind in ("sage", "graph_add") else None
    args = () if kind == "gin" or ew is None else (ew,)
    ha = h0.clone().requires_grad_(True)
    with launches() as names:
        ya = conv(ha, b, *args)
        ya.backward(dY)
    took_block = "block_fwd" in names
    assert took_block == ("block_bwd" in names) == (name != "full")
    if took_block:
        assert "spmm_fwd" not in names and "spmm_bwd" not in names
    hr = h0.clone().requires_grad_(True)
    yr = conv(hr, b.edge_index, *args)[:b.n_dst]
    yr.backward(dY)
    assert ya.shape == (b.n_dst, F)
    assert torch.equal(ya, yr) and torch.equal(ha.grad, hr.grad)
    assert bool(ya.abs().sum() > 0) and bool(ha.grad.abs().sum() > 0)


@pytest.mark.parametrize("use_ew", [False, True])
def test_sageconv_weight_gradients_on_a_block(ladder, use_ew):
    """Random W: dW against the fp64 product agg^T dY inside the bound
    tests/test_gpu_conv_parity.py::test_sageconv_vs_oracle uses for it."""
    import mgcn
    from mgcn.pyg import SAGEConv
    g, b = ladder, ladder.hop0
    F_in, F_out = 32, 48
    torch.manual_seed(5)
    conv = SAGEConv(F_in, F_out).to(g.dev)
    h = _features(g, b, F_in)
    ew = g.weights(b) if use_ew else None
    dY = torch.randn(b.n_dst, F_out, generator=torch.Generator().manual_seed(6)).to(g.dev)
    with launches() as names:
        conv(h, b, ew).backward(dY)
    assert "block_fwd" in names
    agg = mgcn.block_aggregate(h, b, "mean", "append", ew, 1.0).cpu().numpy().astype(np.float64)
    dZ = dY.cpu().numpy().astype(np.float64)
    err = np.abs(conv.weight.grad.cpu().numpy() - agg.T @ dZ)
    bound = 4e-5 * (np.abs(agg).T @ np.abs(dZ)) + 1e-6
    print("dW max error %.3e, smallest slack %.3e" % (err.max(), (bound - err).min()))
    assert (err <= bound).all()
    np.testing.assert_allclose(conv.bias.grad.cpu().numpy(), dZ.sum(0), rtol=1e-4, atol=1e-3)


def test_gcnconv_and_graphconv_max_take_the_fallback(ladder):
    from mgcn.pyg import GCNConv, GraphConv
    g, b = ladder, ladder.hop1
    h = _features(g, b, 32)
    torch.manual_seed(8)
    for conv in (GCNConv(32, 16).to(g.dev), GraphConv(32, 16, aggr="max").to(g.dev)):
        with launches() as names:
            y = conv(h, b)
        assert "block_fwd" not in names
        assert y.shape == (b.n_dst, 16) and torch.equal(y, conv(h, b.edge_index)[:b.n_dst])
        assert bool(y.abs().sum() > 0)


# ----------------------------------------------------------- 7. no plan built
def _two_layer_step(g, x, convs, blocks, through_blocks):
    h = x[blocks[0].src_ids]
    for l, (conv, b) in enumerate(zip(convs, blocks)):
        h = conv(h, b) if through_blocks else conv(h, b.edge_index)[:b.n_dst]
        h = torch.relu(h) if l == 0 else h
    h.square().mean().backward()
    return h


def test_a_step_on_fresh_blocks_builds_no_plan(ladder, monkeypatch):
    import mgcn
    from mgcn import graph, pyg
    g = ladder
    counts = {"plans": 0, "loops": 0}
    build_plan, add_loops = graph.build_plan, pyg.add_remaining_self_loops

    def counted_build(*a, **k):
        counts["plans"] += 1
        return build_plan(*a, **k)

    def counted_loops(*a, **k):
        counts["loops"] += 1
        return add_loops(*a, **k)
    monkeypatch.setattr(graph, "build_plan", counted_build)
    monkeypatch.setattr(pyg, "add_remaining_self_loops", counted_loops)
    torch.manual_seed(12)
    convs = [pyg.SAGEConv(16, 16).to(g.dev), pyg.SAGEConv(16, 16).to(g.dev)]
    x = torch.randn(N, 16, generator=torch.Generator().manual_seed(13)).to(g.dev)
    seeds = g.hop1.src_ids[:g.hop1.n_dst]
    blocks = mgcn.sample_blocks(g.plan, seeds, [5, 5], seed=SEED, offset=OFFSET + 7)
    _two_layer_step(g, x, convs, blocks, True)
    assert counts == {"plans": 0, "loops": 0}
    blocks = mgcn.sample_blocks(g.plan, seeds, [5, 5], seed=SEED, offset=OFFSET + 9)
    _two_layer_step(g, x, convs, blocks, False)
    assert counts == {"plans": 2, "loops": 2}


# ------------------------------------------------------------------ 8. switch
def test_the_switch_sends_blocks_through_the_fallback(ladder):
    import mgcn
    g, b = ladder, ladder.hop0
    conv = _conv("sage", 32, g.dev)
    h = _features(g, b, 32)
    with launches() as names:
        on = conv(h, b)
    assert "block_fwd" in names and mgcn.block_convs()
    try:
        mgcn.set_block_convs(False)
        with launches() as names:
            off = conv(h, b)
        assert "block_fwd" not in names and "spmm_fwd" in names
    finally:
        mgcn.set_block_convs(True)
    assert torch.equal(on, off) and bool(on.abs().sum() > 0)


# ------------------------------------------------------- 9. two-hop training
def test_sage_minibatch_step_on_blocks_trains_and_replays(ladder):
    import mgcn
    from mgcn.pyg import SAGEConv
    g = ladder
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(N, 16, generator=gen).to(g.dev)
    target = torch.randn(N, 16, generator=gen).to(g.dev)
    seeds = g.hop1.src_ids[:g.hop1.n_dst]

    def step(through_blocks=True):
        torch.manual_seed(7)
        convs = [SAGEConv(16, 16).to(g.dev), SAGEConv(16, 16).to(g.dev)]
        blocks = mgcn.sample_blocks(g.plan, seeds, [5, 5])  # seed=None: torch's generator
        h = x[blocks[0].src_ids]
        first = None
        for l, (conv, b) in enumerate(zip(convs, blocks)):
            h = conv(h, b) if through_blocks else conv(h, b.edge_index)[:b.n_dst]
            first = h.detach().clone() if l == 0 else first
            h = torch.relu(h) if l == 0 else h
        loss = ((h - target[seeds]) ** 2).mean()
        loss.backward()
        grads = [p.grad.clone() for conv in convs for p in conv.parameters()]
        assert grads and all(bool(torch.isfinite(gr).all()) for gr in grads)
        assert all(bool(gr.abs().sum() > 0) for gr in grads)
        return loss.detach(), grads, first

    with launches() as names:
        l1, g1, h1 = step()
    # (the input layer's rows need no gradient: one adjoint launch, the top layer's)
    assert names.count("block_fwd") == 2 and names.count("block_bwd") == 1
    assert "spmm_fwd" not in names and "spmm_bwd" not in names
    l2, g2, _ = step()
    assert torch.equal(l1, l2) and all(torch.equal(a, b) for a, b in zip(g1, g2))
    _, _, h_ref = step(through_blocks=False)
    assert torch.equal(h1, h_ref)  # layer 1 at F = 16: the same aggregate, the same GEMM
    mgcn.clear_cache()
