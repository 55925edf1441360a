"""Derived graph plans on the device (GraphPlan.select_edges / induced /
reversed, drop_edges, the pooling modules' wiring).

The contract: a derived plan equals ``build_plan`` of the child edge list --
the list today's torch code makes (``edge_index[:, keep]``,
``votepool.subgraph``, ``pool.filter_adj``) -- field for field.  The reference
of every comparison is that rebuild, never the derive path.

T = 2048 is the tile of derive.hip's scan (kTile: 256 threads x 8 items); a
tile launch has at most 1024 workgroups (kMaxGrid), so 1025 tiles make one
workgroup take a second tile."""
import numpy as np
import pytest
import torch

import timer_names_cases as TN

pytestmark = pytest.mark.gpu

T = 2048
MAX_GRID = 1024


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


def base_edges():
    """The 70-node / 370-edge graph of the timer-name cases (self loops
    included), its first 12 edges repeated, shifted by one id into 72 nodes:
    node 0 and node 71 have no edge (empty first and last rows in both views)."""
    ei = TN.edge_index()
    ei = np.concatenate([ei, ei[:, :12]], axis=1) + 1
    return torch.from_numpy(ei), TN.N + 2


@pytest.fixture(scope="module")
def base(cuda):
    from mgcn.graph import build_plan
    ei, n = base_edges()
    ei = ei.to(cuda)
    return ei, n, build_plan(ei, n)


def random_edges(rng, n, e):
    return torch.from_numpy(rng.integers(0, n, (2, e)).astype(np.int64))


# ------------------------------------------------------------ keep patterns
def _keep_patterns(ei):
    e = ei.size(1)
    dst, src = ei[1], ei[0]
    row = int(torch.bincount(dst).argmax())  # a row with several edges
    slots = (dst == row).nonzero().view(-1)  # its fwd slots, in COO order
    out = {"all": torch.ones(e, dtype=torch.bool), "none": torch.zeros(e, dtype=torch.bool)}
    out["one"] = torch.zeros(e, dtype=torch.bool)
    out["one"][123] = True
    for name, k in (("first_slot_of_a_row", slots[0]), ("last_slot_of_a_row", slots[-1])):
        out[name] = torch.ones(e, dtype=torch.bool)
        out[name][k] = False
    out["every_other"] = torch.arange(e) % 2 == 0
    gone = torch.zeros(int(ei.max()) + 2, dtype=torch.bool)
    gone[[1, 2, 17, 40, 70]] = True
    out["rows_emptied"] = ~(gone[dst] | gone[src])  # every edge at those nodes, both views
    out["bernoulli"] = torch.rand(e, generator=torch.Generator().manual_seed(3)) < 0.5
    return out


@pytest.mark.parametrize("pattern", ["all", "none", "one", "first_slot_of_a_row",
                                     "last_slot_of_a_row", "every_other", "rows_emptied",
                                     "bernoulli"])
def test_select_edges_keep_patterns(base, pattern):
    from mgcn.graph import build_plan
    ei, n, plan = base
    keep = _keep_patterns(ei.cpu())[pattern].to(ei.device)
    child = plan.select_edges(keep)
    assert_plans_equal(child, build_plan(ei[:, keep], n))
    assert child.norms == {} and child._slot_map is None
    if pattern == "all":
        assert_plans_equal(child, plan)
        assert child is not plan and child.fwd.col.data_ptr() != plan.fwd.col.data_ptr()
    if pattern == "none":
        assert child.nnz == 0 and child.fwd.col.shape == (0,)
    assert torch.equal(child.edge_index(), ei[:, keep])


@pytest.mark.parametrize("nnz_in", [T - 1, T, T + 1, 3 * T + 37, (MAX_GRID + 1) * T + 3])
def test_scan_boundaries(cuda, nnz_in):
    """Tile edges of the scan: one short tile, one full tile, one item into
    the second, several tiles (the tile-offset hand-off), and more tiles than
    workgroups (the grid-stride loop)."""
    from mgcn.graph import build_plan
    n = 300 if nnz_in < 10 * T else 20000
    rng = np.random.default_rng(nnz_in)
    ei = random_edges(rng, n, nnz_in).to(cuda)
    keep = (torch.rand(nnz_in, generator=torch.Generator().manual_seed(nnz_in)) < 0.5).to(cuda)
    keep[-1] = True  # the last item of the last tile is live
    plan = build_plan(ei, n)
    assert_plans_equal(plan.select_edges(keep), build_plan(ei[:, keep], n))
    perm = torch.from_numpy(rng.permutation(n)[:n // 2 + 1]).to(cuda)
    from mgcn.pool import filter_adj
    child_ei, _ = filter_adj(ei, None, perm, n)
    assert_plans_equal(plan.induced(perm, relabel=True), build_plan(child_ei, perm.numel()))


# ---------------------------------------------------- row-schedule thresholds
@pytest.fixture(scope="module")
def star(cuda):
    """A hub (node 0) with 600 in-edges and 600 out-edges, plus 400 noise edges
    among the other 699 nodes."""
    from mgcn.graph import build_plan
    rng = np.random.default_rng(11)
    n = 700
    others = rng.integers(1, n, 600)
    into, out_of = np.stack([others, np.zeros(600, np.int64)]), np.stack([np.zeros(600, np.int64),
                                                                          rng.integers(1, n, 600)])
    noise = rng.integers(1, n, (2, 400))
    ei = np.concatenate([into, out_of, noise], axis=1).astype(np.int64)
    ei = torch.from_numpy(ei[:, rng.permutation(ei.shape[1])]).to(cuda)
    return ei, n, build_plan(ei, n)


@pytest.mark.parametrize("hub_edges", [520, 511, 130, 128, 100])
def test_row_schedule_thresholds(star, hub_edges):
    """The hub crosses the giant (512) and the heavy (128) threshold on the
    way down; n_giant, n_heavy and order (None below the thresholds unless the
    degrees stay skewed) must be the rebuild's in both views."""
    from mgcn.graph import build_plan
    ei, n, plan = star
    assert plan.fwd.n_heavy == 1 and plan.bwd.n_heavy == 1 and plan.fwd.n_giant == 1
    keep = torch.ones(ei.size(1), dtype=torch.bool, device=ei.device)
    for end in (0, 1):  # out-edges of the hub, in-edges of the hub
        hub = (ei[end] == 0).nonzero().view(-1)
        keep[hub[hub_edges:]] = False
    child, ref = plan.select_edges(keep), build_plan(ei[:, keep], n)
    assert_plans_equal(child, ref)
    assert int(child.fwd.rowptr[1]) == hub_edges
    assert child.fwd.n_heavy == (1 if hub_edges > 128 else 0)
    assert child.fwd.n_giant == ref.fwd.n_giant and child.bwd.n_giant == ref.bwd.n_giant


def test_schedule_falls_back_to_natural_order(cuda):
    """A hub whose edges all go: the child is near-uniform, order is None."""
    from mgcn.graph import build_plan
    rng = np.random.default_rng(5)
    n = 400
    hub = np.stack([rng.integers(1, n, 300), np.zeros(300, np.int64)])
    ring = np.stack([np.arange(n), (np.arange(n) + 1) % n])
    ei = torch.from_numpy(np.concatenate([hub, ring, ring[::-1]], axis=1).astype(np.int64)).to(cuda)
    plan = build_plan(ei, n)
    assert plan.fwd.order is not None
    keep = torch.ones(ei.size(1), dtype=torch.bool, device=cuda)
    keep[:300] = False
    child = plan.select_edges(keep)
    assert child.fwd.order is None and child.bwd.order is None
    assert_plans_equal(child, build_plan(ei[:, keep], n))


# ------------------------------------------------------------- node filters
def _node_sets(n):
    g = torch.Generator().manual_seed(9)
    half = torch.randperm(n, generator=g)[:n // 2]
    return {
        "random_half": half,  # an id list in no particular order
        "all_descending": torch.arange(n - 1, -1, -1),
        "one_node": torch.tensor([5]),
        "no_edges": torch.tensor([n - 1, 0]),  # the two isolated nodes
        "empty": torch.zeros(0, dtype=torch.int64),
    }


@pytest.mark.parametrize("relabel", [False, True])
@pytest.mark.parametrize("form", ["ids", "mask"])
@pytest.mark.parametrize("which", ["random_half", "all_descending", "one_node", "no_edges",
                                   "empty"])
def test_induced(base, which, form, relabel):
    from mgcn.graph import build_plan
    from mgcn.votepool import subgraph
    ei, n, plan = base
    ids = _node_sets(n)[which].to(ei.device)
    if form == "mask":
        nodes = torch.zeros(n, dtype=torch.bool, device=ei.device)
        nodes[ids] = True
        n_child = int(nodes.sum()) if relabel else n
    else:
        nodes, n_child = ids, (ids.numel() if relabel else n)
    child_ei, _ = subgraph(nodes, ei, relabel_nodes=relabel, num_nodes=n)
    child = plan.induced(nodes, relabel=relabel)
    assert_plans_equal(child, build_plan(child_ei, n_child))
    assert torch.equal(child.edge_index(), child_ei)
    if which == "all_descending":
        assert child.nnz == plan.nnz  # a pure permutation of the nodes
    if which in ("no_edges", "empty"):
        assert child.nnz == 0
    if form == "ids" and ids.numel():
        assert_plans_equal(plan.induced(nodes, relabel=relabel, validate=False), child)


def test_induced_rejects_bad_ids_on_the_device(base):
    ei, n, plan = base
    for ids, what in (([3, n], "out of range"), ([-1], "out of range"), ([4, 9, 4], "repeated")):
        for relabel in (False, True):
            with pytest.raises(ValueError, match=what):
                plan.induced(torch.tensor(ids, device=ei.device), relabel=relabel)
    with pytest.raises(ValueError):
        plan.select_edges(torch.ones(plan.nnz + 1, dtype=torch.bool, device=ei.device))


def test_induced_topk_perm_over_a_batch(cuda):
    """filter_adj with the perm TopK pooling makes over a batch of 3 graphs:
    per graph the best half, in descending score order."""
    from mgcn.graph import build_plan
    from mgcn.pool import filter_adj, topk
    rng = np.random.default_rng(21)
    sizes, parts, off = [23, 40, 9], [], 0
    for s in sizes:
        parts.append(random_edges(rng, s, 4 * s) + off)
        off += s
    ei = torch.cat(parts, dim=1).to(cuda)
    batch = torch.repeat_interleave(torch.arange(3), torch.tensor(sizes)).to(cuda)
    score = torch.randn(off, generator=torch.Generator().manual_seed(1)).to(cuda)
    perm = topk(score, 0.5, batch)
    child_ei, _ = filter_adj(ei, None, perm, off)
    child = build_plan(ei, off).induced(perm, relabel=True)
    assert child.num_nodes == perm.numel() == 12 + 20 + 5
    assert_plans_equal(child, build_plan(child_ei, perm.numel()))


def test_chain_of_three_derives(base):
    from mgcn.graph import build_plan
    from mgcn.pool import filter_adj
    ei, n, plan = base
    g = torch.Generator().manual_seed(17)
    k1 = (torch.rand(ei.size(1), generator=g) < 0.8).to(ei.device)
    e1 = ei[:, k1]
    perm = torch.randperm(n, generator=g)[:50].to(ei.device)
    e2, _ = filter_adj(e1, None, perm, n)
    k3 = (torch.rand(e2.size(1), generator=g) < 0.6).to(ei.device)
    e3 = e2[:, k3]
    child = plan.select_edges(k1).induced(perm, relabel=True).select_edges(k3)
    assert_plans_equal(child, build_plan(e3, 50))
    assert torch.equal(child.edge_index(), e3)


def test_reversed(base):
    from mgcn.graph import build_plan
    ei, n, plan = base
    assert_plans_equal(plan.reversed(), build_plan(ei.flip(0), n))
    assert torch.equal(plan.reversed().edge_index(), ei.flip(0))


# --------------------------------------------------------------- downstream
@pytest.fixture(scope="module")
def derived_and_rebuilt(base):
    from mgcn.graph import build_plan
    ei, n, plan = base
    keep = (torch.rand(ei.size(1), generator=torch.Generator().manual_seed(4)) < 0.7).to(ei.device)
    return plan.select_edges(keep), build_plan(ei[:, keep], n), n


@pytest.mark.parametrize("aggr", ["add", "mean", "max"])
def test_aggregate_on_a_derived_plan(derived_and_rebuilt, aggr):
    from mgcn.ops import aggregate_plan
    child, ref, n = derived_and_rebuilt
    g = torch.Generator().manual_seed(8)
    x0, gy = torch.randn(n, 8, generator=g), torch.randn(n, 8, generator=g)
    res = []
    for plan in (child, ref):
        x = x0.to(plan.device).requires_grad_(True)
        y = aggregate_plan(x, plan, plan.norm("sm"), aggr)
        y.backward(gy.to(plan.device))
        res.append((y.detach(), x.grad))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_attention_on_a_derived_plan(derived_and_rebuilt):
    """att_dir 'out' reads slot_map(), built lazily on the child."""
    from mgcn.ops import attention_aggregate
    child, ref, n = derived_and_rebuilt
    g = torch.Generator().manual_seed(6)
    h0, a0, gy = torch.randn(n, 8, generator=g), torch.randn(1, 2, 8, generator=g), \
        torch.randn(n, 8, generator=g)
    res = []
    for plan in (child, ref):
        hp = h0.to(plan.device).requires_grad_(True)
        att = a0.to(plan.device).requires_grad_(True)
        y, alpha = attention_aggregate(hp, att, plan, 2, "lrelu", "out")
        y.backward(gy.to(plan.device))
        res.append((y.detach(), alpha.detach(), hp.grad, att.grad))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert torch.equal(child.slot_map(), ref.slot_map())


# ------------------------------------------------------------------ modules
class _CountBuilds:
    def __enter__(self):
        from mgcn import graph as G
        self.G, self.orig, self.calls = G, G.build_plan, 0

        def counted(edge_index, num_nodes):
            self.calls += 1
            return self.orig(edge_index, num_nodes)
        G.build_plan = counted
        return self

    def __exit__(self, *exc):
        self.G.build_plan = self.orig


def _run_with(derived, fn):
    from mgcn import graph as G
    G.clear_cache()
    G.set_derived_plans(derived)
    try:
        with _CountBuilds() as c:
            out = fn()
        return out, c.calls
    finally:
        G.set_derived_plans(True)
        G.clear_cache()


@pytest.mark.parametrize("relabel", [False, True])
def test_votepool_model_derived_equals_rebuilt(cuda, relabel):
    from mgcn import votepool as V
    rng = np.random.default_rng(31)
    sizes = [30, 22]
    ei = torch.cat([random_edges(rng, sizes[0], 150), random_edges(rng, sizes[1], 90) + sizes[0]],
                   dim=1).to(cuda)
    torch.manual_seed(13)
    model = V.VotePoolModel(12, [16, 16], 3, residual=True, nheads=[2, 2], att_act="lrelu",
                            temperature=0.5, relabel=relabel).to(cuda).train()
    x0 = torch.randn(sum(sizes), 12, generator=torch.Generator().manual_seed(2)).to(cuda)
    seen = []
    layer_forward = V.VotePoolLayer.forward

    def run():
        torch.manual_seed(77)  # the Gumbel noise of both runs
        model.zero_grad()
        x = x0.clone().requires_grad_(True)
        eis = []

        def spy(self, x_, edge_index, slices, attn_store=None):
            res = layer_forward(self, x_, edge_index, slices, attn_store=attn_store)
            eis.append(res[1])
            return res
        V.VotePoolLayer.forward = spy
        try:
            y = model(x, ei, [0, sizes[0], sum(sizes)])
        finally:
            V.VotePoolLayer.forward = layer_forward
        y.square().sum().backward()
        seen.append(eis)
        return [y.detach(), x.grad] + eis + [p.grad.clone() for p in model.parameters()
                                              if p.grad is not None]

    on, builds_on = _run_with(True, run)
    off, builds_off = _run_with(False, run)
    assert len(on) == len(off) and len(seen[0]) == 2
    for a, b in zip(on, off):
        assert a.shape == b.shape and torch.equal(a, b)
    # one build per forward (the input graph), not one per layer
    assert builds_on == 1 and builds_off == 2


def test_topk_then_graphconv_derived_equals_rebuilt(cuda):
    from mgcn.graph import plan_for
    from mgcn.pool import TopKPooling
    from mgcn.pyg import GraphConv
    rng = np.random.default_rng(41)
    sizes, parts, off = [19, 33, 12], [], 0
    for s in sizes:
        parts.append(random_edges(rng, s, 5 * s) + off)
        off += s
    ei = torch.cat(parts, dim=1).to(cuda)
    batch = torch.repeat_interleave(torch.arange(3), torch.tensor(sizes)).to(cuda)
    torch.manual_seed(3)
    conv0, pool, conv = GraphConv(10, 16).to(cuda), TopKPooling(16, ratio=0.5).to(cuda), \
        GraphConv(16, 8).to(cuda)
    mods = (conv0, pool, conv)
    x0 = torch.randn(off, 10, generator=torch.Generator().manual_seed(5)).to(cuda)

    def run():
        for m in mods:
            m.zero_grad()
        x = x0.clone().requires_grad_(True)
        h = conv0(x, ei).relu()  # plans the input graph, as the pooling nets do
        h, ei2, _, b2, perm, score = pool(h, ei, batch=batch)
        y = conv(h, ei2)
        assert plan_for(ei2, h.size(0)).nnz == ei2.size(1)
        y.square().sum().backward()
        return [y.detach(), x.grad, ei2, perm, score.detach()] + \
            [p.grad.clone() for m in mods for p in m.parameters()]

    on, builds_on = _run_with(True, run)
    off_, builds_off = _run_with(False, run)
    for a, b in zip(on, off_):
        assert a.shape == b.shape and torch.equal(a, b)
    assert builds_on == 1 and builds_off == 2


def test_adopted_plan_is_the_next_layers_cache_hit(base):
    from mgcn import graph as G
    from mgcn.votepool import prune
    ei, n, _ = base
    G.clear_cache()
    try:
        parent = G.plan_for(ei, n)
        x = torch.ones(n, 4, device=ei.device)
        sel = torch.arange(ei.size(1), device=ei.device) % 3 == 0
        for relabel in (False, True):
            xo, eo, nodes, _ = prune(x.clone(), ei, sel, relabel=relabel, batch_slices_x=[0, n])
            with _CountBuilds() as c:
                child = G.plan_for(eo, xo.size(0))
            assert c.calls == 0 and child is not parent
            assert_plans_equal(child, G.build_plan(eo, xo.size(0)))
    finally:
        G.clear_cache()


# --------------------------------------------------------------- drop_edges
def test_drop_edges(base):
    import mgcn
    ei, n, plan = base
    gen = torch.Generator(device=ei.device)
    child, keep = mgcn.drop_edges(plan, 0.3, generator=gen.manual_seed(5))
    child2, keep2 = mgcn.drop_edges(plan, 0.3, generator=gen.manual_seed(5))
    assert keep.dtype == torch.bool and keep.shape == (plan.nnz,) and torch.equal(keep, keep2)
    assert 0 < int(keep.sum()) < plan.nnz
    assert_plans_equal(child, child2)
    assert_plans_equal(child, plan.select_edges(keep))
    assert_plans_equal(child, mgcn.build_plan(ei[:, keep], n))
    same, all_kept = mgcn.drop_edges(plan, 0.0)
    assert same is plan and bool(all_kept.all()) and all_kept.shape == (plan.nnz,)
    none, k0 = mgcn.drop_edges(plan, 1.0)
    assert none.nnz == 0 and not bool(k0.any())
