"""CPU-only checks of mini-batch blocks' host side (no GPU compute): the numpy
restatement of the definition (block_ref) against a brute-force loop and for
its structural properties, the C entries' argument answers, and the Python
errors that come before any device call."""
import ctypes

import numpy as np
import pytest
import torch

import block_ref as br
import sample_ref as sr

SEED, OFFSET = 0x0123456789abcdef, 2 ** 32 - 1  # offset + l crosses a 32-bit word


def small_graph():
    """60 nodes, 700 random edges with repeats, loops on every third node."""
    rng = np.random.default_rng(11)
    n = 60
    src, dst = rng.integers(0, n, 700), rng.integers(0, n, 700)
    loops = np.arange(0, n, 3)
    src = np.concatenate([src, loops, loops[:5]])  # five nodes carry two loops
    dst = np.concatenate([dst, loops, loops[:5]])
    perm = rng.permutation(src.size)
    return src[perm], dst[perm], n


def brute_force(src, dst, n, seeds, fanouts, seed, offset, keep_loops):
    """The definition, row by row and edge by edge."""
    D = [int(s) for s in seeds]
    out = [None] * len(fanouts)
    for l in range(len(fanouts) - 1, -1, -1):
        key = sr.keys(seed, offset + l, src.size)
        edges = []  # (parent COO id, position of dst in D)
        for i, d in enumerate(D):
            row = [e for e in range(src.size) if dst[e] == d]
            loops = [e for e in row if keep_loops and src[e] == d]
            cand = sorted((e for e in row if e not in loops), key=lambda e: (int(key[e]), e))
            edges += [(e, i) for e in sorted(loops + cand[:fanouts[l]])]
        others = sorted({int(src[e]) for e, _ in edges} - set(D))
        F = D + others
        local = {v: i for i, v in enumerate(F)}
        ei = np.array([[local[int(src[e])] for e, _ in edges], [i for _, i in edges]],
                      dtype=np.int64).reshape(2, -1)
        out[l] = (np.array(F, dtype=np.int64), len(D), ei,
                  np.array([e for e, _ in edges], dtype=np.int64))
        D = F
    return out


def same_blocks(a, b):
    assert len(a) == len(b)
    for (ids_a, nd_a, ei_a, pe_a), (ids_b, nd_b, ei_b, pe_b) in zip(a, b):
        assert nd_a == nd_b
        np.testing.assert_array_equal(ids_a, ids_b)
        np.testing.assert_array_equal(ei_a, ei_b)
        np.testing.assert_array_equal(pe_a, pe_b)


@pytest.mark.parametrize("keep_loops", [True, False])
@pytest.mark.parametrize("fanouts", [[3], [0], [100], [4, 2], [5, 3, 2]])
def test_restatement_against_brute_force(fanouts, keep_loops):
    src, dst, n = small_graph()
    seeds = np.array([41, 3, 0, 59, 17, 30])
    got = br.blocks(src, dst, n, seeds, fanouts, SEED, OFFSET, keep_loops)
    same_blocks(got, brute_force(src, dst, n, seeds, fanouts, SEED, OFFSET, keep_loops))


def test_prefix_properties_and_local_ids():
    src, dst, n = small_graph()
    seeds = np.array([7, 2, 33, 50])
    blocks = br.blocks(src, dst, n, seeds, [6, 4, 2], SEED, OFFSET)
    np.testing.assert_array_equal(blocks[2][0][:blocks[2][1]], seeds)
    for lo, hi in zip(blocks[:-1], blocks[1:]):
        np.testing.assert_array_equal(lo[0][:lo[1]], hi[0])  # a layer's outputs: the next's inputs
    for ids, n_dst, ei, peid in blocks:
        assert len(set(ids.tolist())) == ids.size
        assert np.all(np.diff(ids[n_dst:]) > 0)  # the new sources ascend
        assert ei.shape == (2, peid.size) and np.all(ei[1] < n_dst) and np.all(ei[0] < ids.size)
        np.testing.assert_array_equal(ids[ei[0]], src[peid])
        np.testing.assert_array_equal(ids[ei[1]], dst[peid])
        # ordered by (destination's position, parent COO id): a row sums in the parent's order
        order = np.lexsort((peid, ei[1]))
        np.testing.assert_array_equal(order, np.arange(peid.size))
        assert set(ids[n_dst:].tolist()) == set(src[peid].tolist()) - set(ids[:n_dst].tolist())


def test_keep_loops_keeps_loops_on_top_of_the_cap():
    src, dst, n = small_graph()
    seeds = np.arange(0, n, 3)  # every seed has a loop, the first five have two
    (ids, n_dst, ei, peid), = br.blocks(src, dst, n, seeds, [2], SEED, OFFSET, keep_loops=True)
    loop = ei[0] == ei[1]
    per_row = np.bincount(ei[1][~loop], minlength=n_dst)
    assert per_row.max() == 2
    assert int(loop.sum()) == int(((src == dst) & np.isin(dst, seeds)).sum()) >= seeds.size + 5
    (_, _, ei_free, _), = br.blocks(src, dst, n, seeds, [2], SEED, OFFSET, keep_loops=False)
    assert np.bincount(ei_free[1], minlength=n_dst).max() == 2  # loops count like any edge


def test_fanout_zero_and_empty_seeds_give_empty_blocks():
    src, dst, n = small_graph()
    seeds = np.array([v for v in range(n) if not ((src == v) & (dst == v)).any()][:4])
    for ids, n_dst, ei, peid in br.blocks(src, dst, n, seeds, [0, 0], SEED, OFFSET):
        np.testing.assert_array_equal(ids, seeds)
        assert n_dst == 4 and ei.shape == (2, 0) and peid.size == 0
    for ids, n_dst, ei, peid in br.blocks(src, dst, n, np.zeros(0, dtype=np.int64), [3, 3], SEED,
                                          OFFSET):
        assert ids.size == 0 and n_dst == 0 and ei.shape == (2, 0) and peid.size == 0


def test_hop_l_is_drawn_under_offset_plus_l():
    src, dst, n = small_graph()
    seeds = np.array([9, 8, 20, 44, 45])
    two = br.blocks(src, dst, n, seeds, [3, 3], SEED, OFFSET)
    (top,) = br.blocks(src, dst, n, seeds, [3], SEED, OFFSET + 1)
    same_blocks([two[1]], [top])
    (inner,) = br.blocks(src, dst, n, two[1][0], [3], SEED, OFFSET)
    same_blocks([two[0]], [inner])
    (same_offset,) = br.blocks(src, dst, n, seeds, [3], SEED, OFFSET)
    assert not np.array_equal(same_offset[3], top[3])


# --------------------------------------------------------------- the C entries
def test_entries_answer_without_a_device():
    """MGCN_EINVAL from the argument checks alone, before any HIP call."""
    import mgcn
    from mgcn import _lib as L
    lib = mgcn.load()
    assert lib.mgcn_block_workspace_bytes(1000, 10) > 0
    assert (lib.mgcn_block_workspace_bytes(10 ** 6, 10 ** 4) <
            lib.mgcn_block_workspace_bytes(10 ** 6, 10 ** 5))
    buf = torch.zeros(64, dtype=torch.int64)
    P = ctypes.c_void_p(buf.data_ptr())

    def count(n=3, nnz=4, rowptr=P, col=P, dst=P, n_dst=2, fanout=2, keep_loops=1, node_map=P,
              rowptr_out=P, meta=P, ws=P, ws_bytes=1 << 20):
        return lib.mgcn_block_count(n, nnz, rowptr, col, dst, n_dst, fanout, keep_loops, node_map,
                                    rowptr_out, meta, ws, ws_bytes, None)

    def fill(n=3, nnz=4, rowptr=P, col=P, eid=P, dst=P, n_dst=2, fanout=2, rowptr_out=P,
             nnz_out=2, n_heavy=0, node_map=P, src_out=P, eid_out=P, dst_out=P, meta=P, ws=P,
             ws_bytes=1 << 20):
        return lib.mgcn_block_fill(n, nnz, rowptr, col, eid, dst, n_dst, fanout, 1, 1, 2,
                                   rowptr_out, nnz_out, n_heavy, node_map, src_out, eid_out,
                                   dst_out, meta, ws, ws_bytes, None)

    def relabel(n=3, dst=P, n_dst=2, n_src=3, nnz_out=2, src_out=P, node_map=P, src_ids=P,
                col_out=P, coo_src=P, ws=P, ws_bytes=1 << 20):
        return lib.mgcn_block_relabel(n, dst, n_dst, n_src, nnz_out, src_out, node_map, src_ids,
                                      col_out, coo_src, ws, ws_bytes, None)

    bad = [count(n=-1), count(nnz=-1), count(n_dst=-1), count(nnz=2 ** 31), count(fanout=-1),
           count(dst=None), count(rowptr=None), count(col=None), count(node_map=None),
           count(rowptr_out=None), count(meta=None),
           fill(n=-1), fill(nnz=2 ** 31), fill(fanout=-1), fill(nnz_out=-1), fill(nnz_out=5),
           fill(n_heavy=3), fill(n_heavy=-1), fill(eid=None), fill(src_out=None),
           fill(dst_out=None), fill(meta=None),
           relabel(n_dst=-1), relabel(n_src=1), relabel(n_src=4), relabel(src_ids=None),
           relabel(col_out=None), relabel(n_src=3, nnz_out=0)]
    assert bad == [L.EINVAL] * len(bad)
    assert b"mgcn_block_relabel" in lib.mgcn_last_error()
    assert count(ws=None) == L.EWORKSPACE and fill(ws_bytes=8) == L.EWORKSPACE
    assert (buf == 0).all()


def test_signatures_and_exports():
    import mgcn
    from mgcn import _lib as L
    for name in ("mgcn_block_workspace_bytes", "mgcn_block_count", "mgcn_block_fill",
                 "mgcn_block_relabel"):
        assert name in L.SIGNATURES
    assert mgcn.load().mgcn_abi_version() == 22 == L.ABI_VERSION
    for name in ("Block", "sample_blocks", "block_batches"):
        assert getattr(mgcn, name) is getattr(mgcn.ops, name) is getattr(mgcn.ops_block, name)
        assert name in mgcn.__all__
    assert callable(mgcn.GraphPlan.sample_blocks)


# ------------------------------------------------------------ Python errors
def _cpu_plan(n=3, nnz=4):
    """A plan-shaped object on the CPU: enough for the argument checks."""
    from mgcn.graph import CSRView, GraphPlan
    rowptr = torch.tensor([0, 2, 3, 4][:n + 1], dtype=torch.int64)
    z = torch.zeros(nnz, dtype=torch.int32)
    view = CSRView(rowptr=rowptr, col=z, eid=torch.arange(nnz, dtype=torch.int32), n_rows=n,
                   n_cols=n)
    return GraphPlan(num_nodes=n, nnz=nnz, device=torch.device("cpu"), fwd=view, bwd=view,
                     in_cnt=torch.ones(n))


def test_python_errors_come_before_any_device_call(monkeypatch):
    import mgcn

    def no_device(*a, **k):
        raise AssertionError("an argument error touched the device")
    monkeypatch.setattr(torch.cuda, "_lazy_init", no_device)
    monkeypatch.setattr(torch.cuda, "synchronize", no_device)
    plan = _cpu_plan()
    seeds = torch.tensor([0, 2])
    for call in (lambda *a, **k: mgcn.sample_blocks(plan, *a, **k), plan.sample_blocks):
        for bad in ([2, -1], [1.5], ["3"], [None], [True]):
            with pytest.raises(ValueError, match="fanout"):
                call(seeds, bad, seed=1)
        for kw in ({"seed": -1}, {"seed": 2 ** 64}, {"seed": 1, "offset": -1},
                   {"seed": 1, "offset": 2 ** 64}, {"seed": 1.5},
                   {"seed": 1, "offset": 2 ** 64 - 1}):  # offset + 1 for the second layer
            with pytest.raises(ValueError, match="seed|offset"):
                call(seeds, [2, 2], **kw)
        for bad in (torch.tensor([0.0, 1.0]), torch.tensor([[0, 1]]), torch.tensor(1),
                    torch.tensor([0, 1], dtype=torch.int16), [0, 1],
                    torch.ones(4, dtype=torch.bool), torch.ones(3, 1, dtype=torch.bool)):
            with pytest.raises(ValueError, match="seeds"):
                call(bad, [2], seed=1)
        # CPU tensors: the engine is GPU-only
        with pytest.raises(mgcn.MgcnError, match="HIP device only"):
            call(seeds, [2], seed=1)
        with pytest.raises(mgcn.MgcnError, match="HIP device only"):
            call(torch.ones(3, dtype=torch.bool), [2], seed=1)
        with pytest.raises(mgcn.MgcnError, match="HIP device only"):
            call(seeds.to(torch.int32), [2, 2])  # seed=None: a host draw, then the device check
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="batch_size"):
            next(mgcn.block_batches(plan, seeds, bad, [2]))
    with pytest.raises(ValueError, match="ids"):
        next(mgcn.block_batches(plan, torch.tensor([0.5]), 2, [2]))
