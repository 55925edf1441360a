"""CPU-only checks of neighbour sampling's host side (no GPU compute): the
numpy restatement of the definition (sample_ref) against the tested generator
and for uniformity, the C entry's argument answers, the Python errors and the
seed draws."""
import ctypes

import numpy as np
import pytest
import torch

import philox_ref as pr
import sample_ref as sr


def test_key_is_the_noise_entrys_word():
    """key(e) >> 8 is the 24 bits of mgcn_edge_noise's uniform for head 0."""
    seed, offset = 0xfedcba9876543210, 2 ** 32 + 5
    k = sr.keys(seed, offset, 1000)
    assert k.dtype == np.uint32 and k.shape == (1000,)
    u = pr.uniform(seed, offset, 1000, 1)[:, 0]
    np.testing.assert_array_equal((k >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24),
                                  u)
    # all 32 bits are used: the low byte is not constant
    assert len(set((k & np.uint32(0xff)).tolist())) > 200


def test_restatement_on_a_hand_case():
    """Two rows; row 1 has a loop (edge 2).  The kept set is the smallest keys."""
    src = np.array([0, 2, 1, 3, 4, 0, 2])
    dst = np.array([1, 1, 1, 1, 1, 0, 0])
    k = sr.keys(7, 3, 7)
    for fanout in range(0, 6):
        keep = sr.sample_keep(src, dst, 5, fanout, 7, 3, keep_loops=True)
        assert keep[2]  # the loop 1 -> 1, on top of the fan-out
        cand = np.array([0, 1, 3, 4])
        want = cand[np.lexsort((cand, k[cand]))][:fanout]
        assert sorted(np.flatnonzero(keep[[0, 1, 3, 4]]).tolist()) == sorted(
            np.searchsorted(cand, want).tolist())
        # row 0: edge 5 is the loop 0 -> 0, edge 6 the one candidate
        assert keep[5] and keep[6] == (fanout >= 1)
        free = sr.sample_keep(src, dst, 5, fanout, 7, 3, keep_loops=False)
        assert free[dst == 1].sum() == min(fanout, 5) and free[dst == 0].sum() == min(fanout, 2)
    rows = np.array([True, False, True, True, True])
    keep = sr.sample_keep(src, dst, 5, 2, 7, 3, keep_loops=True, rows=rows)
    assert not keep[dst == 1].any() and keep[dst == 0].all()


def test_definition_is_uniform():
    """One row of 40 candidates, fanout 5, 4000 offsets: every edge is kept
    with probability 1 / 8; the counts' scaled chi-square statistic stays below
    the 0.999 quantile of chi-square with 39 degrees of freedom (72.1)."""
    n_edges, fanout, draws = 40, 5, 4000
    src = np.arange(1, n_edges + 1)
    dst = np.zeros(n_edges, dtype=np.int64)
    counts = np.zeros(n_edges, dtype=np.int64)
    for offset in range(draws):
        keep = sr.sample_keep(src, dst, n_edges + 1, fanout, 0x1234567, offset)
        assert keep.sum() == fanout
        counts += keep
    exp = draws * fanout / n_edges
    var = draws * (1 / 8) * (7 / 8)
    stat = (39 / 40) * float(((counts - exp) ** 2 / var).sum())
    print(f"statistic {stat:.2f}, counts {counts.min()} .. {counts.max()}")
    assert exp == 500 and stat < 72.1


def test_entry_answers_without_a_device():
    """mgcn_sample_rows answers from its argument checks alone, before any HIP
    call: 0 where there is nothing to do, MGCN_EINVAL for every unsupported
    argument, with the keep buffer left as it was."""
    import mgcn
    from mgcn import _lib as L
    lib = mgcn.load()
    assert lib.mgcn_sample_rows_workspace_bytes(1000, 5000) == 0
    rowptr = torch.zeros(4, dtype=torch.int64)
    idx = torch.zeros(4, dtype=torch.int32)
    keep = torch.full((8,), 7, dtype=torch.uint8)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def call(n_rows=3, nnz=4, rowptr=P(rowptr), col=P(idx), eid=P(idx), order=None, n_heavy=0,
             fanout=2, keep_loops=1, keep=P(keep)):
        return lib.mgcn_sample_rows(n_rows, nnz, rowptr, col, eid, order, n_heavy, None, fanout,
                                    keep_loops, 1, 2, keep, None, 0, None)

    assert call(nnz=0) == L.OK and call(n_rows=0, nnz=0, keep=None) == L.OK
    assert call(nnz=0, rowptr=None, col=None, eid=None, keep=None) == L.OK
    assert call(n_rows=0) == L.OK  # no row: nothing is launched
    bad = [call(n_rows=-1), call(nnz=-1), call(nnz=2 ** 31), call(fanout=-1), call(keep=None),
           call(rowptr=None), call(eid=None), call(col=None, keep_loops=1),
           call(order=None, n_heavy=1), call(order=P(idx), n_heavy=-1),
           call(order=P(idx), n_heavy=4)]
    assert bad == [L.EINVAL] * len(bad)
    assert (keep == 7).all()
    assert b"mgcn_sample_rows" in lib.mgcn_last_error()


def test_signatures_and_abi():
    import mgcn
    from mgcn import _lib as L
    assert "mgcn_sample_rows" in L.SIGNATURES
    assert "mgcn_sample_rows_workspace_bytes" in L.SIGNATURES
    assert mgcn.load().mgcn_abi_version() == 22 == L.ABI_VERSION
    for name in ("sample_keep", "sample_neighbors", "sample_layers", "set_sample_heavy_rows"):
        assert getattr(mgcn, name) is getattr(mgcn.ops, name)
        assert name in mgcn.__all__


def _cpu_plan(n=3, nnz=4):
    """A plan-shaped object on the CPU: enough for the argument checks."""
    from mgcn.graph import CSRView, GraphPlan
    rowptr = torch.tensor([0, 2, 3, 4][:n + 1], dtype=torch.int64)
    z = torch.zeros(nnz, dtype=torch.int32)
    view = CSRView(rowptr=rowptr, col=z, eid=torch.arange(nnz, dtype=torch.int32), n_rows=n,
                   n_cols=n)
    return GraphPlan(num_nodes=n, nnz=nnz, device=torch.device("cpu"), fwd=view, bwd=view,
                     in_cnt=torch.ones(n))


def test_python_errors():
    import mgcn
    plan = _cpu_plan()
    for fn in (mgcn.sample_keep, mgcn.sample_neighbors, plan.sample_neighbors):
        call = (lambda *a, **k: fn(*a, **k)) if fn == plan.sample_neighbors else (
            lambda *a, **k: fn(plan, *a, **k))
        for bad in (-1, 1.5, "3", None, True):
            with pytest.raises(ValueError, match="fanout"):
                call(bad, seed=1)
        for kw in ({"seed": -1}, {"seed": 2 ** 64}, {"seed": 1, "offset": -1},
                   {"seed": 1, "offset": 2 ** 64}, {"seed": 1.5}):
            with pytest.raises(ValueError, match="seed|offset"):
                call(2, **kw)
        for rows in (torch.ones(4, dtype=torch.bool), torch.ones(3, dtype=torch.uint8),
                     torch.ones(3, 1, dtype=torch.bool), [True, False, True]):
            with pytest.raises(ValueError, match="rows"):
                call(2, seed=1, rows=rows)
        # a CPU tensor, a CPU plan: the engine is GPU-only
        with pytest.raises(mgcn.MgcnError, match="HIP device only"):
            call(2, seed=1, rows=torch.ones(3, dtype=torch.bool))
        with pytest.raises(mgcn.MgcnError, match="HIP device only"):
            call(2, seed=1)
    with pytest.raises(ValueError, match="fanout"):
        mgcn.sample_layers(plan, [2, -1], seed=1)
    with pytest.raises(ValueError, match="offset"):
        mgcn.sample_layers(plan, [2, 2], seed=1, offset=2 ** 64 - 1)
    # the largest words pass the checks (and then meet the device check)
    with pytest.raises(mgcn.MgcnError, match="HIP device only"):
        mgcn.sample_keep(plan, 2, seed=2 ** 64 - 1, offset=2 ** 64 - 1)


def test_seed_none_draws_once_per_mask_on_the_host(monkeypatch):
    import mgcn
    from mgcn import ops_sample
    from mgcn.graph import GraphPlan

    def no_device(*a, **k):
        raise AssertionError("the seed draw touched the device")
    monkeypatch.setattr(torch.cuda, "_lazy_init", no_device)
    monkeypatch.setattr(torch.cuda, "synchronize", no_device)
    draws, calls = [], []
    real_draw = ops_sample.draw_edge_seed

    def counting_draw(*a, **k):
        draws.append(real_draw(*a, **k))
        return draws[-1]

    def fake_keep(plan, fanout, *, seed, offset, keep_loops, rows):
        calls.append((fanout, seed, offset))
        return torch.ones(plan.nnz, dtype=torch.bool)
    monkeypatch.setattr(ops_sample, "draw_edge_seed", counting_draw)
    monkeypatch.setattr(ops_sample, "sample_keep", fake_keep)
    monkeypatch.setattr(GraphPlan, "select_edges", lambda self, keep: "child")
    plan = _cpu_plan()

    torch.manual_seed(99)
    assert mgcn.sample_neighbors(plan, 2)[0] == "child"
    assert len(draws) == 1 and calls == [(2, *draws[0])]
    plan.sample_neighbors(1)
    assert len(draws) == 2 and calls[1] == (1, *draws[1]) and draws[0] != draws[1]
    # fanout >= nnz: the parent itself, and still one draw (the stream of pairs
    # does not depend on the fan-out)
    out, keep = mgcn.sample_neighbors(plan, plan.nnz)
    assert out is plan and keep.all() and len(draws) == 3 and len(calls) == 2
    layers = mgcn.sample_layers(plan, [3, 2, 1])
    assert len(layers) == 3 and len(draws) == 6
    assert calls[2:] == [(3, *draws[3]), (2, *draws[4]), (1, *draws[5])]
    first = list(draws)
    # torch.manual_seed replays the pairs
    torch.manual_seed(99)
    del draws[:], calls[:]
    mgcn.sample_neighbors(plan, 2), plan.sample_neighbors(1), mgcn.sample_neighbors(plan, 4)
    mgcn.sample_layers(plan, [3, 2, 1])
    assert draws == first
    # an explicit seed draws nothing; layer l uses offset + l
    del draws[:], calls[:]
    mgcn.sample_neighbors(plan, 2, seed=5, offset=9)
    mgcn.sample_layers(plan, [3, 2, 1], seed=2 ** 64 - 1, offset=40)
    assert draws == []
    assert calls == [(2, 5, 9), (3, 2 ** 64 - 1, 40), (2, 2 ** 64 - 1, 41), (1, 2 ** 64 - 1, 42)]
