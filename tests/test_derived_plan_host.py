"""Derived graph plans, the part that needs no GPU: the new C entries are
exported and declared, their argument checks answer before any launch, the
Python methods reject CPU tensors and bad node ids on the host, reversed()
swaps the views, and adopt_plan / plan_for share one cache."""
import ctypes
import gc
from types import SimpleNamespace

import pytest
import torch

import mgcn
from mgcn import _lib as L
from mgcn import graph as G
from mgcn.graph import CSRView, GraphPlan

NEW = ("mgcn_edge_rank_workspace_bytes", "mgcn_edge_rank", "mgcn_csr_derive_workspace_bytes",
       "mgcn_csr_derive")


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _cpu_plan():
    """4 nodes, edges 0->1, 2->1, 1->3, 3->3 as a hand-built CPU GraphPlan."""
    ei = torch.tensor([[0, 2, 1, 3], [1, 1, 3, 3]])
    i32 = torch.int32
    fwd = CSRView(rowptr=torch.tensor([0, 0, 2, 2, 4]), col=torch.tensor([0, 2, 1, 3], dtype=i32),
                  eid=torch.tensor([0, 1, 2, 3], dtype=i32), n_rows=4, n_cols=4, n_heavy=0)
    bwd = CSRView(rowptr=torch.tensor([0, 1, 2, 3, 4]), col=torch.tensor([1, 3, 1, 3], dtype=i32),
                  eid=torch.tensor([0, 2, 1, 3], dtype=i32), n_rows=4, n_cols=4, n_heavy=0)
    in_cnt = torch.tensor([1.0, 2.0, 1.0, 2.0])
    return GraphPlan(4, 4, torch.device("cpu"), fwd, bwd, in_cnt), ei


def test_symbols_exported_and_declared(lib):
    for name in NEW:
        assert name in L.SIGNATURES
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert lib.mgcn_abi_version() == 22 == L.ABI_VERSION
    for name in ("adopt_plan", "drop_edges", "set_derived_plans", "GraphPlan"):
        assert name in mgcn.__all__ and hasattr(mgcn, name)
    for name in ("select_edges", "induced", "reversed", "edge_index"):
        assert callable(getattr(GraphPlan, name))


def test_workspace_sizes_grow_with_the_graph(lib):
    small = lib.mgcn_csr_derive_workspace_bytes(10, 10, 100)
    assert small > 0 and lib.mgcn_csr_derive_workspace_bytes(10, 10, 100000) > small
    assert lib.mgcn_edge_rank_workspace_bytes(100000) > lib.mgcn_edge_rank_workspace_bytes(1) > 0


def test_csr_derive_argument_errors(lib):
    """Checked before any launch: the pointers are never dereferenced."""
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    args = lambda rowptr_out, ws, ws_bytes: (3, 3, 5, p, p, p, None, 3, None, p, 2, rowptr_out,
                                             p, p, ws, ws_bytes, None)
    need = lib.mgcn_csr_derive_workspace_bytes(3, 3, 5)
    assert lib.mgcn_csr_derive(*args(None, p, need)) == L.EINVAL
    assert b"rowptr_out is null" in lib.mgcn_last_error()
    # (the identity form needs the first parts of `need` only: a clearly short one)
    assert lib.mgcn_csr_derive(*args(p, p, 64)) == L.EWORKSPACE
    assert b"workspace 64 bytes" in lib.mgcn_last_error()
    permuted = (3, 3, 5, p, p, p, p, 3, None, p, 2, p, p, p, p, need - 1, None)
    assert lib.mgcn_csr_derive(*permuted) == L.EWORKSPACE
    assert lib.mgcn_csr_derive(*args(p, None, 0)) == L.EWORKSPACE
    # identity rows with another row count, more edges out than in, null inputs
    bad_rows = (3, 3, 5, p, p, p, None, 2, None, p, 2, p, p, p, p, need, None)
    assert lib.mgcn_csr_derive(*bad_rows) == L.EINVAL and b"identity" in lib.mgcn_last_error()
    too_many = (3, 3, 5, p, p, p, None, 3, None, p, 6, p, p, p, p, need, None)
    assert lib.mgcn_csr_derive(*too_many) == L.EINVAL and b"nnz_out" in lib.mgcn_last_error()
    null_in = (3, 3, 5, p, None, p, None, 3, None, p, 2, p, p, p, p, need, None)
    assert lib.mgcn_csr_derive(*null_in) == L.EINVAL and b"null array" in lib.mgcn_last_error()


def test_edge_rank_argument_errors(lib):
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    need = lib.mgcn_edge_rank_workspace_bytes(5)
    no_maps = (None,) * 6
    assert lib.mgcn_edge_rank(5, p, *no_maps, p, None, p, need, None) == L.EINVAL
    assert b"total is null" in lib.mgcn_last_error()
    assert lib.mgcn_edge_rank(5, None, *no_maps, p, p, p, need, None) == L.EINVAL
    assert b"neither" in lib.mgcn_last_error()
    assert lib.mgcn_edge_rank(5, p, None, None, p, p, p, p, p, p, p, need, None) == L.EINVAL
    assert b"needs a view" in lib.mgcn_last_error()
    assert lib.mgcn_edge_rank(5, p, *no_maps, p, p, p, need - 1, None) == L.EWORKSPACE
    assert b"workspace" in lib.mgcn_last_error()


def test_cpu_tensors_raise():
    plan, _ = _cpu_plan()
    with pytest.raises(L.MgcnError, match="HIP device"):
        plan.select_edges(torch.ones(4, dtype=torch.bool))
    with pytest.raises(L.MgcnError, match="HIP device"):
        plan.induced(torch.tensor([True, True, False, True]))
    with pytest.raises(L.MgcnError, match="HIP device"):
        plan.induced(torch.tensor([0, 1, 3]), relabel=True)
    with pytest.raises(L.MgcnError, match="HIP device"):
        G.drop_edges(plan, 0.5)


def test_keep_mask_shape_and_dtype():
    plan, _ = _cpu_plan()
    with pytest.raises(ValueError, match="bool"):
        plan.select_edges(torch.ones(4))
    with pytest.raises(ValueError, match="bool"):
        plan.select_edges(torch.ones(3, dtype=torch.bool))
    with pytest.raises(ValueError):
        plan.induced(torch.ones(5, dtype=torch.bool))
    with pytest.raises(ValueError):
        G.drop_edges(plan, 1.5)


@pytest.mark.parametrize("relabel", [False, True])
@pytest.mark.parametrize("ids, what", [([0, 4], "out of range"), ([-1, 2], "out of range"),
                                       ([1, 2, 1], "repeated")])
def test_induced_rejects_bad_ids(ids, what, relabel):
    plan, _ = _cpu_plan()
    with pytest.raises(ValueError, match=what):
        plan.induced(torch.tensor(ids), relabel=relabel)
    with pytest.raises(ValueError, match=what):
        plan.induced(ids, relabel=relabel)


def test_reversed_swaps_the_views():
    plan, ei = _cpu_plan()
    plan.fwd.n_heavy, plan.bwd.n_giant = 3, 2  # schedule fields travel with their view
    r = plan.reversed()
    assert r.num_nodes == 4 and r.nnz == 4 and r.device == plan.device
    for a, b in ((r.fwd, plan.bwd), (r.bwd, plan.fwd)):
        assert a is not b
        assert a.rowptr is b.rowptr and a.col is b.col and a.eid is b.eid
        assert (a.n_rows, a.n_cols, a.n_heavy, a.n_giant, a.heavy_thr, a.order) == \
            (b.n_rows, b.n_cols, b.n_heavy, b.n_giant, b.heavy_thr, b.order)
    # in-degrees of the flipped graph = out-degrees of this one, clamped at 1
    assert torch.equal(r.in_cnt, torch.tensor([1.0, 1.0, 1.0, 1.0]))
    assert r.norms == {} and r._slot_map is None
    assert torch.equal(r.edge_index(), ei.flip(0)) and torch.equal(plan.edge_index(), ei)
    back = r.reversed()
    assert back.fwd.rowptr is plan.fwd.rowptr and torch.equal(back.in_cnt, plan.in_cnt)


def _fake(n, e):
    return SimpleNamespace(num_nodes=n, nnz=e)


def test_adopt_plan_and_plan_for_share_the_cache():
    G.clear_cache()
    ei = torch.tensor([[0, 1, 2], [1, 2, 0]])
    fake = _fake(3, 3)
    assert G.cached_plan(ei, 3) is None
    assert G.adopt_plan(ei, 3, fake) is fake
    assert G.plan_for(ei, 3) is fake and G.cached_plan(ei, 3) is fake
    assert G.cached_plan(ei, 4) is None  # num_nodes is part of the key
    other = _fake(3, 3)
    G.adopt_plan(ei, 3, other)  # re-adopting replaces
    assert G.plan_for(ei, 3) is other
    ei.add_(0)  # an in-place write bumps the version: the entry no longer matches
    assert G.cached_plan(ei, 3) is None
    with pytest.raises(ValueError, match="nodes"):
        G.adopt_plan(ei, 3, _fake(4, 3))
    with pytest.raises(ValueError, match="edges"):
        G.adopt_plan(ei, 3, _fake(3, 2))
    with pytest.raises(ValueError):
        G.adopt_plan(ei[0], 3, fake)
    G.clear_cache()


def test_adopted_entries_die_with_their_tensor_and_are_evicted():
    G.clear_cache()
    ei = torch.tensor([[0, 1], [1, 0]])
    G.adopt_plan(ei, 2, _fake(2, 2))
    key = G.cache_key(ei, 2)
    assert key in G._CACHE
    del ei
    gc.collect()
    assert G._CACHE[key][0]() is None  # only a weak reference was held
    keep = [torch.zeros(2, k + 1, dtype=torch.int64) for k in range(G._CACHE_SIZE + 3)]
    plans = [_fake(9, k + 1) for k in range(len(keep))]
    for t, p in zip(keep, plans):
        G.adopt_plan(t, 9, p)
    assert len(G._CACHE) == G._CACHE_SIZE
    assert G.cached_plan(keep[0], 9) is None and G.cached_plan(keep[2], 9) is None
    assert G.cached_plan(keep[3], 9) is plans[3] and G.plan_for(keep[-1], 9) is plans[-1]
    G.clear_cache()


def test_switch_and_adopt_derived_without_a_parent():
    assert G.derived_plans_enabled() is True
    G.set_derived_plans(False)
    try:
        assert G.derived_plans_enabled() is False
    finally:
        G.set_derived_plans(True)
    # CPU tensors / no cached parent: nothing is derived, nothing is cached
    G.clear_cache()
    ei = torch.tensor([[0, 1], [1, 0]])
    G.adopt_derived(ei, 2, torch.tensor([False, False]), ei[:, :0], 1, torch.tensor([0]))
    assert len(G._CACHE) == 0
