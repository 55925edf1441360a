"""Neighbour sampling on the device (mgcn_sample_rows, mgcn.sample_keep /
sample_neighbors / sample_layers).

The contract is the definition restated in tests/sample_ref.py: every
comparison is ``torch.equal`` of the mask against it -- integers only, no
tolerance anywhere.  Shapes cross the lane-group widths of the light kernel
(8 / 16 / 32 / 64 lanes by mean degree), its 128-slot limit, the schedule's
128 / 129 heavy and 512 / 513 giant thresholds, the 7168-slot LDS capacity of
the heavy kernel (7168 / 7169, and the 40,000-edge row), and the launches'
grid caps."""
import dataclasses

import numpy as np
import pytest
import torch

import sample_ref as sr

pytestmark = pytest.mark.gpu

LADDER = list(range(0, 131)) + [200, 512, 513, 1025, 40000]
FANOUTS = [0, 1, 2, 5, 16, 64, 127, 128, 129, 1000, 50000]
# (row, slot): start / middle / end; rows 129 .. 135 are heavy, 133 .. 135 giant
LOOPS = ((1, "s"), (7, "s"), (8, "m"), (9, "e"), (40, "s"), (40, "e"), (128, "m"), (129, "s"),
         (130, "e"), (131, "m"), (133, "s"), (133, "e"), (135, "m"))
SEED, OFFSET = 0x0123456789abcdef, 0xfedcba9876543210


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


def ladder_edges(n, seed=0):
    """Destination row i has in-degree LADDER[i] (rows past the ladder: none),
    sources random with repeats; the COO order is a random permutation, so slot
    order differs from id order; self loops at the start, the middle and the
    end of some rows' slots (a row's slots are in COO id order), two in one row."""
    rng = np.random.default_rng(seed)
    dst = np.repeat(np.arange(len(LADDER)), LADDER)
    dst = dst[rng.permutation(dst.size)]
    src = rng.integers(0, n, dst.size)
    src[src == dst] = n - 1  # the only loops are the planted ones
    for row, where in LOOPS:
        slots = np.flatnonzero(dst == row)
        src[slots[{"s": 0, "m": slots.size // 2, "e": -1}[where]]] = row
    return np.stack([src, dst]).astype(np.int64)


class Graph:
    def __init__(self, ei, n, dev):
        from mgcn.graph import build_plan
        self.ei_np, self.n = ei, n
        self.ei = torch.from_numpy(ei).to(dev)
        self.plan = build_plan(self.ei, n)
        self.rows_np = np.random.default_rng(5).random(n) < 0.5
        self.rows = torch.from_numpy(self.rows_np).to(dev)

    def ref(self, fanout, seed=SEED, offset=OFFSET, keep_loops=True, masked=False):
        return sr.sample_keep(self.ei_np[0], self.ei_np[1], self.n, fanout, seed, offset,
                              keep_loops, self.rows_np if masked else None)

    def got(self, fanout, seed=SEED, offset=OFFSET, keep_loops=True, masked=False, plan=None):
        import mgcn
        return mgcn.sample_keep(plan or self.plan, fanout, seed=seed, offset=offset,
                                keep_loops=keep_loops, rows=self.rows if masked else None)


def same(mask, ref):
    assert mask.dtype == torch.bool and mask.shape == ref.shape
    return torch.equal(mask.cpu(), torch.from_numpy(ref))


@pytest.fixture(scope="module")
def ladder(cuda):
    """n = 4000: mean degree 12, lane groups of 16."""
    g = Graph(ladder_edges(4000), 4000, cuda)
    v = g.plan.fwd
    assert v.order is not None and v.n_heavy == 7 and v.n_giant == 3
    return g


# ------------------------------------------------------------ 1. the ladder
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("keep_loops", [True, False])
@pytest.mark.parametrize("fanout", FANOUTS)
def test_degree_ladder(ladder, fanout, keep_loops, masked):
    g = ladder
    mask = g.got(fanout, keep_loops=keep_loops, masked=masked)
    assert same(mask, g.ref(fanout, keep_loops=keep_loops, masked=masked))
    src, dst = g.ei[0], g.ei[1]
    counted = mask & (src != dst) if keep_loops else mask
    per_row = torch.bincount(dst[counted], minlength=g.n)
    assert int(per_row.max()) <= fanout
    if keep_loops and not masked:
        assert bool(mask[src == dst].all()) and int((src == dst).sum()) == len(LOOPS)


@pytest.mark.parametrize("n,lanes", [(200, 64), (1500, 32), (7000, 8)])
def test_lane_group_widths(cuda, n, lanes):
    """The same ladder among n nodes: the mean degree picks the group width."""
    g = Graph(ladder_edges(n, seed=n), n, cuda)
    mean = g.plan.nnz // n
    assert {64: mean > 48, 32: 16 < mean <= 48, 8: mean <= 8}[lanes]
    for fanout in (1, 5, 64, 127):
        for keep_loops in (True, False):
            assert same(g.got(fanout, keep_loops=keep_loops),
                        g.ref(fanout, keep_loops=keep_loops)), (fanout, keep_loops)
    assert same(g.got(3, masked=True), g.ref(3, masked=True))


def test_more_rows_than_one_launch_holds(cuda):
    """300,000 rows in groups of 8 lanes (more than 8192 workgroups x 32 rows),
    8,200 of them heavy (more than the 8192 workgroups of the heavy launch)."""
    rng = np.random.default_rng(3)
    n, n_heavy = 300_000, 8200
    dst = np.concatenate([np.repeat(rng.permutation(n)[:n_heavy], 129), rng.integers(0, n, 400_000)])
    src = rng.integers(0, n, dst.size)
    perm = rng.permutation(dst.size)
    g = Graph(np.stack([src[perm], dst[perm]]).astype(np.int64), n, cuda)
    assert g.plan.fwd.n_heavy >= n_heavy and g.plan.nnz // n <= 8
    assert same(g.got(3), g.ref(3))
    ref = g.ref(100, keep_loops=False, masked=True)
    assert same(g.got(100, keep_loops=False, masked=True), ref)
    flat = dataclasses.replace(g.plan, fwd=dataclasses.replace(g.plan.fwd, order=None, n_heavy=0,
                                                               n_giant=0))
    assert same(g.got(100, keep_loops=False, masked=True, plan=flat), ref)


def test_lds_capacity_boundary(cuda):
    """Rows of 7168 and 7169 slots: the last row whose keys the heavy kernel
    holds in LDS and the first that recomputes them in every pass."""
    rng = np.random.default_rng(9)
    n = 300
    dst = np.repeat([3, 200], [7168, 7169])
    dst = dst[rng.permutation(dst.size)]
    src = rng.integers(0, n, dst.size)
    g = Graph(np.stack([src, dst]).astype(np.int64), n, cuda)
    assert g.plan.fwd.n_heavy == 2
    for fanout, keep_loops in ((1, True), (700, False), (7167, True), (7168, False)):
        assert same(g.got(fanout, keep_loops=keep_loops),
                    g.ref(fanout, keep_loops=keep_loops)), (fanout, keep_loops)


# --------------------------------------------------------------- 2. the tie
def test_key_tie_is_broken_by_the_coo_id(cuda):
    import mgcn
    from mgcn.graph import build_plan
    nnz, a, b = 40000, 24791, 30978
    k = sr.keys(1, 0, nnz)
    assert k[a] == k[b] == 0x55e32f24 and int((k < k[a]).sum()) == 13430
    src = 1 + np.arange(nnz) % 100
    dst = np.zeros(nnz, dtype=np.int64)
    plan = build_plan(torch.from_numpy(np.stack([src, dst])).to(cuda), 101)
    m1 = mgcn.sample_keep(plan, 13431, seed=1, offset=0)
    assert bool(m1[a]) and not bool(m1[b]) and int(m1.sum()) == 13431
    assert same(m1, sr.sample_keep(src, dst, 101, 13431, 1, 0))
    m2 = mgcn.sample_keep(plan, 13432, seed=1, offset=0)
    assert bool(m2[a]) and bool(m2[b]) and int(m2.sum()) == 13432
    assert same(m2, sr.sample_keep(src, dst, 101, 13432, 1, 0))


# ------------------------------------------------- 3. route independence
def _raw(plan, fanout, keep_loops, rows, order, n_heavy):
    from mgcn import _lib as L
    lib = L.load()
    v = plan.fwd
    keep = torch.full((plan.nnz,), 7, dtype=torch.uint8, device=plan.device)
    rc = lib.mgcn_sample_rows(v.n_rows, plan.nnz, L.ptr(v.rowptr), L.ptr(v.col), L.ptr(v.eid),
                              L.ptr(order), n_heavy, L.ptr(rows), fanout, int(keep_loops), SEED,
                              OFFSET, L.ptr(keep), None, 0, L.stream_of(plan.device))
    L.check(rc, "mgcn_sample_rows")
    assert int(keep.max()) <= 1  # every byte written, 0 or 1
    return keep.bool()


@pytest.mark.parametrize("fanout", [1, 5, 127, 129, 1000])
def test_route_independence(ladder, fanout):
    import mgcn
    g = ladder
    for keep_loops in (True, False):
        ref = g.ref(fanout, keep_loops=keep_loops, masked=True)
        assert same(g.got(fanout, keep_loops=keep_loops, masked=True), ref)
        mgcn.set_sample_heavy_rows(False)
        try:
            assert not mgcn.ops.sample_heavy_rows()
            assert same(g.got(fanout, keep_loops=keep_loops, masked=True), ref)
        finally:
            mgcn.set_sample_heavy_rows(True)
        flat = dataclasses.replace(g.plan, fwd=dataclasses.replace(
            g.plan.fwd, order=None, n_heavy=0, n_giant=0))
        assert same(g.got(fanout, keep_loops=keep_loops, masked=True, plan=flat), ref)
        v = g.plan.fwd
        assert same(_raw(g.plan, fanout, keep_loops, g.rows, None, 0), ref)
        assert same(_raw(g.plan, fanout, keep_loops, g.rows, v.order, v.n_heavy), ref)
        # a schedule that marks more rows heavy: the workgroups take short rows too
        assert same(_raw(g.plan, fanout, keep_loops, g.rows, v.order, v.n_heavy + 40), ref)
        # col is not read without keep_loops
        if not keep_loops:
            from mgcn import _lib as L
            keep = torch.empty(g.plan.nnz, dtype=torch.uint8, device=g.plan.device)
            rc = L.load().mgcn_sample_rows(v.n_rows, g.plan.nnz, L.ptr(v.rowptr), None,
                                           L.ptr(v.eid), None, 0, L.ptr(g.rows), fanout, 0, SEED,
                                           OFFSET, L.ptr(keep), None, 0,
                                           L.stream_of(g.plan.device))
            assert rc == L.OK and same(keep.bool(), ref)


# ------------------------------------------------------------ 4. seed words
def test_every_seed_word_matters_and_replays(ladder):
    g = ladder
    base = g.got(5)
    assert same(base, g.ref(5)) and torch.equal(base, g.got(5))
    for seed, offset in ((SEED ^ 1, OFFSET), (SEED ^ (1 << 32), OFFSET), (SEED, OFFSET ^ 1),
                         (SEED, OFFSET ^ (1 << 32)), (2 ** 64 - 1, 2 ** 64 - 1), (0, 0)):
        m = g.got(5, seed=seed, offset=offset)
        assert not torch.equal(m, base), (hex(seed), hex(offset))
        assert same(m, g.ref(5, seed=seed, offset=offset)), (hex(seed), hex(offset))
    # the mask is the noise entry's uniform, ranked
    import mgcn
    u = mgcn.edge_noise(g.plan, 1, 'uniform', seed=SEED >> 1, offset=OFFSET >> 1)[:, 0].cpu()
    k = sr.keys(SEED >> 1, OFFSET >> 1, g.plan.nnz)
    assert torch.equal(u, torch.from_numpy((k >> np.uint32(8)).astype(np.float32)
                                           * np.float32(2.0 ** -24)))


# ------------------------------------------------------------ 5. child plan
@pytest.mark.parametrize("fanout,masked", [(5, False), (16, True), (0, False)])
def test_child_plan_is_the_rebuild(ladder, fanout, masked):
    import mgcn
    from mgcn.graph import build_plan, clear_cache, plan_for
    g = ladder
    rows = g.rows if masked else None
    child, keep = mgcn.sample_neighbors(g.plan, fanout, seed=SEED, offset=OFFSET, rows=rows)
    assert same(keep, g.ref(fanout, masked=masked))
    ei = g.ei[:, keep]
    assert_plans_equal(child, build_plan(ei, g.n))
    assert child.norms == {} and child is not g.plan
    via_method, keep2 = g.plan.sample_neighbors(fanout, seed=SEED, offset=OFFSET, rows=rows)
    assert torch.equal(keep, keep2)
    assert_plans_equal(via_method, child)
    clear_cache()
    mgcn.adopt_plan(ei, g.n, child)
    assert plan_for(ei, g.n) is child
    clear_cache()


def test_a_cap_that_caps_nothing_returns_the_parent(ladder):
    import mgcn
    g = ladder
    same_plan, keep = mgcn.sample_neighbors(g.plan, g.plan.nnz, seed=1)
    assert same_plan is g.plan and bool(keep.all()) and keep.dtype == torch.bool
    assert keep.device == g.plan.device and keep.shape == (g.plan.nnz,)
    # with a row mask the cap is not the whole story: derived
    child, keep = mgcn.sample_neighbors(g.plan, g.plan.nnz, seed=1, rows=g.rows)
    assert child is not g.plan and same(keep, g.ref(g.plan.nnz, masked=True))


# ------------------------------------------------------------ 6. end to end
def test_aggregate_on_the_sampled_plan_is_the_rebuilds(ladder):
    import mgcn
    from mgcn.graph import build_plan
    from mgcn.ops import aggregate_plan
    g = ladder
    child, keep = mgcn.sample_neighbors(g.plan, 5, seed=SEED, offset=OFFSET)
    rebuilt = build_plan(g.ei[:, keep], g.n)
    gen = torch.Generator().manual_seed(1)
    h0 = torch.randn(g.n, 32, generator=gen).to(g.plan.device)
    dy = torch.randn(g.n, 32, generator=gen).to(g.plan.device)
    outs = []
    for plan in (child, rebuilt):
        h = h0.clone().requires_grad_(True)
        y = aggregate_plan(h, plan, plan.norm(None), 'mean')
        y.backward(dy)
        outs.append((y.detach(), h.grad))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert bool(outs[0][0].abs().sum() > 0)


def test_sage_step_on_the_sampled_edges_trains_and_replays(ladder):
    import mgcn
    from mgcn.pyg import SAGEConv
    g = ladder
    dev = g.plan.device
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(g.n, 16, generator=gen).to(dev)
    target = torch.randn(g.n, 8, generator=gen).to(dev)

    def step():
        torch.manual_seed(7)
        conv = SAGEConv(16, 8).to(dev)
        child, keep = mgcn.sample_neighbors(g.plan, 10)  # seed=None: torch's generator
        ei = g.ei[:, keep]
        mgcn.adopt_plan(ei, g.n, child)
        loss = ((conv(x, ei) - target) ** 2).mean()
        loss.backward()
        grads = [p.grad.clone() for p in conv.parameters()]
        assert grads and all(bool(torch.isfinite(gr).all()) for gr in grads)
        assert any(bool(gr.abs().sum() > 0) for gr in grads)
        return keep, loss.detach(), grads

    k1, l1, g1 = step()
    k2, l2, g2 = step()
    assert torch.equal(k1, k2) and torch.equal(l1, l2)
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))
    assert int(k1.sum()) < g.plan.nnz
    mgcn.clear_cache()


# --------------------------------------------------------- 7. sample_layers
def test_sample_layers(ladder):
    import mgcn
    from mgcn.graph import build_plan
    g = ladder
    o = 2 ** 32 - 2  # the offsets cross a 32-bit word
    layers = mgcn.sample_layers(g.plan, [25, 10, 5], seed=SEED, offset=o, rows=g.rows)
    assert len(layers) == 3
    for l, (fanout, (child, keep)) in enumerate(zip([25, 10, 5], layers)):
        assert same(keep, g.ref(fanout, offset=o + l, masked=True)), l
        assert child.nnz == int(keep.sum())
    assert_plans_equal(layers[2][0], build_plan(g.ei[:, layers[2][1]], g.n))


# ---------------------------------------------------------- 8. empty inputs
def test_empty_inputs(cuda):
    import mgcn
    from mgcn.graph import build_plan
    empty = build_plan(torch.zeros(2, 0, dtype=torch.int64, device=cuda), 5)
    keep = mgcn.sample_keep(empty, 3, seed=1)
    assert keep.shape == (0,) and keep.dtype == torch.bool and keep.device.type == "cuda"
    child, keep = mgcn.sample_neighbors(empty, 3, seed=1, rows=torch.ones(5, dtype=torch.bool,
                                                                         device=cuda))
    assert child.nnz == 0 and keep.shape == (0,)
    loops = torch.arange(6, device=cuda).repeat(2, 1)
    loops = torch.cat([loops, loops[:, :2]], dim=1)  # nodes 0 and 1 have two loops
    plan = build_plan(loops, 7)
    assert bool(mgcn.sample_keep(plan, 0, seed=1).all())  # loops are kept on top
    m = mgcn.sample_keep(plan, 1, seed=1, keep_loops=False)
    assert same(m, sr.sample_keep(loops[0].cpu().numpy(), loops[1].cpu().numpy(), 7, 1, 1, 0,
                                  False))
    assert int(m.sum()) == 6
    assert not bool(mgcn.sample_keep(plan, 0, seed=1, keep_loops=False).any())
    child, keep = mgcn.sample_neighbors(plan, 0, seed=1)
    assert_plans_equal(child, build_plan(loops[:, keep], 7))
