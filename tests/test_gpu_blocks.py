"""Mini-batch blocks on the device (mgcn_block_count / _fill / _relabel,
mgcn.sample_blocks / block_batches).

The contract is the definition restated in tests/block_ref.py on top of
tests/sample_ref.py: every comparison is ``torch.equal`` -- integers, or
floats summed in the same order, no tolerance anywhere.  The graph is a degree
ladder: in-degrees 0 .. 140 (the lane groups' 128-slot limit at 127 / 128 /
129), rows of 7168 and 7169 slots (the LDS capacity of the workgroup route)
and one of 40,000 slots whose COO ids 0 .. 39999 hold the key tie that
seed 1, offset 0 has at ids 24791 and 30978."""
import numpy as np
import pytest
import torch

import block_ref as br
import sample_ref as sr

pytestmark = pytest.mark.gpu

N = 3000
LADDER = list(range(0, 141)) + [7168, 7169]  # row i has in-degree LADDER[i]
HUB = len(LADDER)                             # 40,000 slots, COO ids 0 .. 39999
HEAVY = list(range(129, 141)) + [141, 142, HUB]
SEED, OFFSET = 1, 0
TIE_A, TIE_B, TIE_RANK = 24791, 30978, 13430  # equal keys; 13430 smaller keys in the row


# ------------------------------------------------------------------ helpers
def assert_plans_equal(a, b):
    assert a.num_nodes == b.num_nodes and a.nnz == b.nnz
    assert a.in_cnt.dtype == b.in_cnt.dtype and torch.equal(a.in_cnt, b.in_cnt)
    for name in ("fwd", "bwd"):
        va, vb = getattr(a, name), getattr(b, name)
        for f in ("rowptr", "col", "eid"):
            ta, tb = getattr(va, f), getattr(vb, f)
            assert ta.dtype == tb.dtype and ta.shape == tb.shape, (name, f)
            assert torch.equal(ta, tb), (name, f)
        for f in ("n_rows", "n_cols", "n_heavy", "n_giant", "heavy_thr"):
            assert getattr(va, f) == getattr(vb, f), (name, f)
        assert (va.order is None) == (vb.order is None), name
        if va.order is not None:
            assert va.order.dtype == vb.order.dtype and torch.equal(va.order, vb.order), name


def ladder_edges(n):
    """The hub's edges first (COO ids 0 .. 39999), then the ladder rows' in a
    random COO order; sources random with repeats; a self loop in the first
    slot of every even ladder row and on every even node past the ladder; one
    duplicated edge."""
    rng = np.random.default_rng(0)
    dst = np.repeat(np.arange(len(LADDER)), LADDER)
    dst = np.concatenate([np.full(40000, HUB), dst[rng.permutation(dst.size)]])
    src = rng.integers(0, n, dst.size)
    src[src == dst] = n - 1  # the only loops are the planted ones
    for row in range(2, len(LADDER) + 1, 2):  # the hub is even too
        src[np.flatnonzero(dst == row)[0]] = row
    slots = np.flatnonzero(dst == 50)
    src[slots[7]] = src[slots[3]]  # the same edge twice
    rest = np.arange(len(LADDER) + 1, n)
    rest = rest[rest % 2 == 0]
    return np.stack([np.concatenate([src, rest]), np.concatenate([dst, rest])]).astype(np.int64)


class Graph:
    def __init__(self, n, dev):
        from mgcn.graph import build_plan
        self.ei_np, self.n, self.dev = ladder_edges(n), n, dev
        self.ei = torch.from_numpy(self.ei_np).to(dev)
        self.plan = build_plan(self.ei, n)
        deg = np.bincount(self.ei_np[1], minlength=n)
        assert [int(deg[r]) for r in (127, 128, 129, 141, 142, HUB)] == [127, 128, 129, 7168, 7169,
                                                                          40000]
        rng = np.random.default_rng(1)
        light = rng.permutation(np.concatenate([  # 30 ladder rows, 10 rows past the ladder
            rng.permutation(129)[:30], rng.permutation(np.arange(HUB + 1, n))[:10]]))
        mixed = np.empty(2 * len(HEAVY), dtype=np.int64)
        mixed[0::2], mixed[1::2] = HEAVY, light[:len(HEAVY)]
        self.seeds = {
            "heavy_first": np.concatenate([HEAVY, light]),
            "heavy_last": np.concatenate([light, HEAVY[::-1]]),
            "interleaved": np.concatenate([light[len(HEAVY):], mixed]),
            "single": np.array([HUB]),
            "all": rng.permutation(n),
        }

    def ref(self, seeds, fanouts, keep_loops=True, seed=SEED, offset=OFFSET):
        return br.blocks(self.ei_np[0], self.ei_np[1], self.n, seeds, fanouts, seed, offset,
                         keep_loops)

    def got(self, seeds, fanouts, keep_loops=True, seed=SEED, offset=OFFSET, **kw):
        import mgcn
        if isinstance(seeds, np.ndarray):
            seeds = torch.from_numpy(seeds).to(self.dev)
        return mgcn.sample_blocks(self.plan, seeds, fanouts, seed=seed, offset=offset,
                                  keep_loops=keep_loops, **kw)

    def mask(self, ids):
        m = torch.zeros(self.n, dtype=torch.bool, device=self.dev)
        m[ids] = True
        return m


def check_fields(blocks, ref):
    assert len(blocks) == len(ref)
    for l, (b, (ids, n_dst, ei, peid)) in enumerate(zip(blocks, ref)):
        assert (b.n_dst, b.n_src) == (n_dst, ids.size), l
        assert b.plan.num_nodes == b.n_src and b.plan.nnz == peid.size, l
        for got, want in ((b.src_ids, ids), (b.edge_index, ei), (b.parent_eid, peid)):
            assert got.dtype == torch.int64 and got.device.type == "cuda", l
            assert got.shape == want.shape and torch.equal(got.cpu(), torch.from_numpy(want)), l


def blocks_equal(a, b):
    return len(a) == len(b) and all(
        (x.n_dst, x.n_src) == (y.n_dst, y.n_src) and torch.equal(x.src_ids, y.src_ids)
        and torch.equal(x.edge_index, y.edge_index) and torch.equal(x.parent_eid, y.parent_eid)
        for x, y in zip(a, b))


@pytest.fixture(scope="module")
def ladder(cuda):
    """n = 3000: mean degree 21, lane groups of 32."""
    g = Graph(N, cuda)
    assert 16 < g.plan.nnz // N <= 48
    return g


# ------------------------------------------- 1. fields equal the restatement
@pytest.mark.parametrize("keep_loops", [True, False])
@pytest.mark.parametrize("fanouts", [[5], [0], [127], [129], [1000], [5, 3], [16, 5, 2]])
def test_fields_equal_the_restatement(ladder, fanouts, keep_loops):
    g = ladder
    for name, seeds in g.seeds.items():
        blocks = g.got(seeds, fanouts, keep_loops)
        check_fields(blocks, g.ref(seeds, fanouts, keep_loops))
        top = blocks[-1]
        assert torch.equal(top.src_ids[:top.n_dst].cpu(), torch.from_numpy(seeds)), name
        for lo, hi in zip(blocks[:-1], blocks[1:]):
            assert torch.equal(lo.src_ids[:lo.n_dst], hi.src_ids), name


def test_seed_forms(ladder):
    """int32 ids, a bool mask (its ids ascending), the method, validate=False."""
    g = ladder
    seeds = g.seeds["interleaved"]
    ref = g.ref(seeds, [5, 3])
    check_fields(g.got(torch.from_numpy(seeds).to(g.dev, torch.int32), [5, 3]), ref)
    check_fields(g.got(seeds, [5, 3], validate=False), ref)
    check_fields(g.plan.sample_blocks(torch.from_numpy(seeds).to(g.dev), [5, 3], seed=SEED,
                                      offset=OFFSET), ref)
    check_fields(g.got(g.mask(torch.from_numpy(seeds).to(g.dev)), [5, 3]),
                 g.ref(np.sort(seeds), [5, 3]))


@pytest.mark.parametrize("n,lanes", [(1200, 64), (5000, 16), (9000, 8)])
def test_lane_group_widths(cuda, n, lanes):
    """The same ladder among n nodes: the parent's mean degree picks the width."""
    g = Graph(n, cuda)
    mean = g.plan.nnz // n
    assert {64: mean > 48, 16: 8 < mean <= 16, 8: mean <= 8}[lanes]
    seeds = g.seeds["interleaved"]
    for fanouts, keep_loops in (([5], True), ([127], False), ([16, 5], True)):
        check_fields(g.got(seeds, fanouts, keep_loops), g.ref(seeds, fanouts, keep_loops))


# --------------------------------------------- 2. tie to the shipped kernel
@pytest.mark.parametrize("fanouts", [[5, 3], [TIE_RANK + 1], [TIE_RANK + 2], [129, 1000]])
def test_edges_are_the_shipped_masks(ladder, fanouts):
    import mgcn
    g = ladder
    tie = fanouts[0] in (TIE_RANK + 1, TIE_RANK + 2)
    keep_loops = not tie  # the recorded rank counts all 40,000 ids as candidates
    blocks = g.got(g.seeds["heavy_last"], fanouts, keep_loops)
    for l, b in enumerate(blocks):
        D = b.src_ids[:b.n_dst]
        keep = mgcn.sample_keep(g.plan, fanouts[l], seed=SEED, offset=OFFSET + l,
                                keep_loops=keep_loops, rows=g.mask(D))
        assert torch.equal(b.parent_eid.sort().values, keep.nonzero().view(-1)), l
    if tie:
        k = sr.keys(SEED, OFFSET, 40000)
        assert k[TIE_A] == k[TIE_B] and int((k < k[TIE_A]).sum()) == TIE_RANK
        kept = set(blocks[0].parent_eid.tolist())
        assert TIE_A in kept and (TIE_B in kept) == (fanouts[0] == TIE_RANK + 2)


# ----------------------------------------------- 3. the plan is the rebuild
@pytest.mark.parametrize("name,fanouts,keep_loops", [
    ("heavy_first", [1000], True), ("interleaved", [5, 3], True), ("all", [16, 5], False),
    ("heavy_last", [0], False), ("heavy_last", [0], True), ("single", [129], True)])
def test_plan_is_the_rebuild(ladder, name, fanouts, keep_loops):
    from mgcn.graph import build_plan
    g = ladder
    for b in g.got(g.seeds[name], fanouts, keep_loops):
        assert_plans_equal(b.plan, build_plan(b.edge_index.clone(), b.n_src))
        assert b.plan.norms == {}
        rows = b.plan.fwd.rowptr
        assert bool((rows[b.n_dst:] == b.plan.nnz).all())  # the rows past the destinations: empty


# ------------------------- 4. forward bit-equality with the full sampled graph
def _children(g, blocks, fanouts, keep_loops=True):
    """The full-graph sampled child of every hop, from the shipped API."""
    out = []
    for l, b in enumerate(blocks):
        child, _ = g.plan.sample_neighbors(fanouts[l], seed=SEED, offset=OFFSET + l,
                                           keep_loops=keep_loops,
                                           rows=g.mask(b.src_ids[:b.n_dst]))
        out.append(child)
    return out


@pytest.mark.parametrize("name,fanout", [("interleaved", 5), ("heavy_first", 16), ("all", 10)])
def test_forward_bits_one_hop(ladder, name, fanout):
    from mgcn.ops import aggregate_plan
    g = ladder
    x = torch.randn(g.n, 32, generator=torch.Generator().manual_seed(3)).to(g.dev)
    deg_full = (g.plan.bwd.rowptr[1:] - g.plan.bwd.rowptr[:-1]).to(torch.float32)
    (b,) = g.got(g.seeds[name], [fanout])
    (child,) = _children(g, [b], [fanout])
    D = b.src_ids[:b.n_dst]
    xb = x[b.src_ids]
    y = aggregate_plan(xb, b.plan, b.plan.norm(None), 'mean')[:b.n_dst]
    assert torch.equal(y, aggregate_plan(x, child, child.norm(None), 'mean')[D])
    assert bool(y.abs().sum() > 0)
    y = aggregate_plan(xb, b.plan, b.plan.norm('sm', deg=deg_full[b.src_ids]), 'add')[:b.n_dst]
    assert torch.equal(y, aggregate_plan(x, child, child.norm('sm', deg=deg_full), 'add')[D])
    assert bool(y.abs().sum() > 0)


def test_forward_bits_two_hops(ladder):
    from mgcn.ops import aggregate_plan
    g = ladder
    fanouts = [6, 4]
    x = torch.randn(g.n, 32, generator=torch.Generator().manual_seed(4)).to(g.dev)
    blocks = g.got(g.seeds["interleaved"], fanouts)
    children = _children(g, blocks, fanouts)
    h, y = x[blocks[0].src_ids], x
    for b, child in zip(blocks, children):
        h = aggregate_plan(h, b.plan, b.plan.norm(None), 'mean')[:b.n_dst]
        y = aggregate_plan(y, child, child.norm(None), 'mean')
    seeds = blocks[1].src_ids[:blocks[1].n_dst]
    assert torch.equal(h, y[seeds]) and bool(h.abs().sum() > 0)


# ------------------------------------------ 5. backward with exact arithmetic
@pytest.mark.parametrize("name,fanout", [("interleaved", 5), ("heavy_first", 1000)])
def test_backward_on_integers(ladder, name, fanout):
    """x and dY hold integers in [-4, 4] and every partial sum stays below
    2^24, so no summation order can change a bit."""
    from mgcn.ops import aggregate_plan
    g = ladder
    gen = torch.Generator().manual_seed(5)
    x = torch.randint(-4, 5, (g.n, 8), generator=gen).float().to(g.dev)
    (b,) = g.got(g.seeds[name], [fanout])
    (child,) = _children(g, [b], [fanout])
    D = b.src_ids[:b.n_dst]
    dY = torch.randint(-4, 5, (b.n_dst, 8), generator=gen).float().to(g.dev)
    xf = x.clone().requires_grad_(True)
    (dY * aggregate_plan(xf, child, child.norm(None), 'add')[D]).sum().backward()
    xb = x[b.src_ids].clone().requires_grad_(True)
    (dY * aggregate_plan(xb, b.plan, b.plan.norm(None), 'add')[:b.n_dst]).sum().backward()
    assert torch.equal(xb.grad, xf.grad[b.src_ids]) and bool(xb.grad.abs().sum() > 0)
    outside = torch.ones(g.n, dtype=torch.bool, device=g.dev)
    outside[b.src_ids] = False
    assert not bool(xf.grad[outside].any())


# ------------------------------------------------- 6. route independence
def _edges_by_destination(b):
    """(global destination, parent COO id) of every block edge, sorted."""
    pairs = torch.stack([b.src_ids[b.edge_index[1]], b.parent_eid], dim=1)
    return pairs[torch.argsort(pairs[:, 1])]  # a parent edge has one destination


@pytest.mark.parametrize("fanouts", [[5], [129], [5, 3]])
def test_seed_order_does_not_change_a_row(ladder, fanouts):
    from mgcn.ops import aggregate_plan
    g = ladder
    seeds = g.seeds["heavy_first"]
    x = torch.randn(g.n, 32, generator=torch.Generator().manual_seed(6)).to(g.dev)
    base = g.got(seeds, fanouts)
    top = base[-1]
    y_base = aggregate_plan(x[top.src_ids], top.plan, top.plan.norm(None), 'mean')[:top.n_dst]
    for perm in (np.arange(seeds.size)[::-1].copy(),
                 np.random.default_rng(8).permutation(seeds.size)):
        other = g.got(seeds[perm], fanouts)
        for a, b in zip(base, other):
            assert torch.equal(_edges_by_destination(a), _edges_by_destination(b))
            assert torch.equal(a.src_ids.sort().values, b.src_ids.sort().values)
        o = other[-1]
        y = aggregate_plan(x[o.src_ids], o.plan, o.plan.norm(None), 'mean')[:o.n_dst]
        assert torch.equal(y, y_base[torch.from_numpy(perm).to(g.dev)])


# ---------------------------------------------------------------- 7. replay
def test_replay_and_seed_words(ladder):
    import mgcn
    g = ladder
    seeds = torch.from_numpy(g.seeds["interleaved"]).to(g.dev)
    s, o = 0x0123456789abcdef, 0xfedcba9876543210
    base = g.got(seeds, [5, 3], seed=s, offset=o)
    assert blocks_equal(base, g.got(seeds, [5, 3], seed=s, offset=o))
    for s2, o2 in ((s ^ 1, o), (s ^ (1 << 32), o), (s, o ^ 1), (s, o ^ (1 << 32))):
        other = g.got(seeds, [5, 3], seed=s2, offset=o2)
        assert not torch.equal(other[1].parent_eid, base[1].parent_eid), (hex(s2), hex(o2))
    torch.manual_seed(21)
    first = mgcn.sample_blocks(g.plan, seeds, [5, 3])
    second = mgcn.sample_blocks(g.plan, seeds, [5, 3])
    assert not blocks_equal(first, second)  # successive draws differ
    torch.manual_seed(21)
    assert blocks_equal(first, mgcn.sample_blocks(g.plan, seeds, [5, 3]))
    assert blocks_equal(second, mgcn.sample_blocks(g.plan, seeds, [5, 3]))


# --------------------------------------------------------------- 8. modules
def test_sage_minibatch_step_trains_and_replays(ladder):
    import mgcn
    from mgcn.graph import plan_for
    from mgcn.pyg import SAGEConv
    g = ladder
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(g.n, 16, generator=gen).to(g.dev)
    target = torch.randn(g.n, 16, generator=gen).to(g.dev)
    seeds = torch.from_numpy(g.seeds["interleaved"]).to(g.dev)

    def step():
        torch.manual_seed(7)
        convs = [SAGEConv(16, 16).to(g.dev), SAGEConv(16, 16).to(g.dev)]
        blocks = mgcn.sample_blocks(g.plan, seeds, [5, 5])  # seed=None: torch's generator
        h = x[blocks[0].src_ids]
        for l, (conv, b) in enumerate(zip(convs, blocks)):
            assert plan_for(b.edge_index, b.n_src) is b.plan
            h = conv(h, b.edge_index)[:b.n_dst]
            h = torch.relu(h) if l == 0 else h
        loss = ((h - target[seeds]) ** 2).mean()
        loss.backward()
        grads = [p.grad.clone() for conv in convs for p in conv.parameters()]
        assert grads and all(bool(torch.isfinite(gr).all()) for gr in grads)
        assert all(bool(gr.abs().sum() > 0) for gr in grads)
        return loss.detach(), grads

    l1, g1 = step()
    l2, g2 = step()
    assert torch.equal(l1, l2) and all(torch.equal(a, b) for a, b in zip(g1, g2))
    mgcn.clear_cache()


def test_block_batches_cover_every_id_once(ladder):
    import mgcn
    g = ladder
    ids = torch.arange(100, 400, device=g.dev)
    gen = torch.Generator().manual_seed(3)
    batches = list(mgcn.block_batches(g.plan, ids, 64, [4, 2], generator=gen))
    assert len(batches) == 5 and all(len(blocks) == 2 for blocks in batches)
    tops = [blocks[1].src_ids[:blocks[1].n_dst] for blocks in batches]
    assert [int(t.numel()) for t in tops] == [64, 64, 64, 64, 44]
    seen = torch.cat(tops)
    assert not torch.equal(seen, ids) and torch.equal(seen.sort().values, ids)  # shuffled
    plain = list(mgcn.block_batches(g.plan, ids, 128, [3], shuffle=False))
    assert torch.equal(torch.cat([bl[0].src_ids[:bl[0].n_dst] for bl in plain]), ids)
    # the generator replays the epoch
    again = list(mgcn.block_batches(g.plan, ids, 64, [4, 2],
                                    generator=torch.Generator().manual_seed(3)))
    assert all(blocks_equal(a, b) for a, b in zip(batches, again))


# ------------------------------------------------------------ 9. validation
def test_validation(ladder):
    import mgcn
    g = ladder
    dev = g.dev
    for bad in ([5, 9, 5], [0, g.n], [3, -1], [2 ** 40, 4]):
        with pytest.raises(ValueError, match="seed id"):
            mgcn.sample_blocks(g.plan, torch.tensor(bad, device=dev), [5, 3], seed=1)
    with pytest.raises(mgcn.MgcnError, match="HIP device only"):
        mgcn.sample_blocks(g.plan, torch.tensor([1, 2]), [5], seed=1)
    for empty in (torch.zeros(0, dtype=torch.int64, device=dev),
                  torch.zeros(g.n, dtype=torch.bool, device=dev)):
        blocks = mgcn.sample_blocks(g.plan, empty, [5, 3], seed=1)
        assert len(blocks) == 2
        for b in blocks:
            assert b.n_src == 0 and b.n_dst == 0 and b.plan.nnz == 0 and b.plan.num_nodes == 0
            assert b.src_ids.shape == (0,) and b.edge_index.shape == (2, 0)
            assert b.parent_eid.shape == (0,) and b.src_ids.device.type == "cuda"
    # a parent without edges: every block is its destinations alone
    from mgcn.graph import build_plan
    bare = build_plan(torch.zeros(2, 0, dtype=torch.int64, device=dev), 9)
    seeds = torch.tensor([4, 0, 7], device=dev)
    for b in mgcn.sample_blocks(bare, seeds, [3, 3], seed=1):
        assert (b.n_dst, b.n_src, b.plan.nnz) == (3, 3, 0) and torch.equal(b.src_ids, seeds)
