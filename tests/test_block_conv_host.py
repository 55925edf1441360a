"""CPU-only checks of the block convs' host side (no GPU compute): the two C
entries' argument answers, the signatures and exports, the Python errors that
come before any device call, and the MGCN_BLOCK_CONV switch."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from conftest import PKG_DIR


def test_entries_answer_without_a_device():
    """MGCN_EINVAL from the argument checks alone, before any HIP call."""
    import mgcn
    from mgcn import _lib as L
    lib = mgcn.load()
    buf = torch.zeros(64, dtype=torch.int64)
    P = ctypes.c_void_p(buf.data_ptr())

    def fwd(n_dst=2, n_src=3, F=4, rowptr=P, col=P, w=None, fill=1.0, loops=0, X=P, ldx=4, Y=P,
            ldy=4, reduce=L.REDUCE_SUM, cnt=None):
        return lib.mgcn_block_spmm_fwd(n_dst, n_src, F, rowptr, col, w, fill, loops, X, ldx, Y,
                                       ldy, reduce, cnt, None)

    def bwd(n_src=3, n_dst=2, F=4, rowptr_t=P, col_t=P, eid_t=P, w=None, fill=1.0, loops=0, dY=P,
            lddy=4, dX=P, lddx=4, reduce=L.REDUCE_SUM, cnt=None):
        return lib.mgcn_block_spmm_bwd(n_src, n_dst, F, rowptr_t, col_t, eid_t, w, fill, loops,
                                       dY, lddy, dX, lddx, reduce, cnt, None)

    bad = [fwd(reduce=L.REDUCE_MAX), fwd(reduce=7), fwd(loops=3), fwd(loops=-1), fwd(F=0),
           fwd(F=-4), fwd(n_dst=4), fwd(n_dst=-1), fwd(n_src=-1, n_dst=-1), fwd(n_src=2 ** 31),
           fwd(rowptr=None), fwd(X=None), fwd(Y=None), fwd(ldx=3), fwd(ldy=3)]
    assert bad == [L.EINVAL] * len(bad)
    assert b"mgcn_block_spmm_fwd" in lib.mgcn_last_error()
    bad = [bwd(reduce=L.REDUCE_MAX), bwd(loops=3), bwd(loops=-2), bwd(F=0), bwd(n_dst=4),
           bwd(n_dst=-1), bwd(n_src=-1, n_dst=-1), bwd(rowptr_t=None), bwd(dY=None),
           bwd(dX=None), bwd(lddy=3), bwd(lddx=3), bwd(reduce=L.REDUCE_MEAN),
           bwd(reduce=L.REDUCE_MEAN, loops=2), bwd(w=P, eid_t=None)]
    assert bad == [L.EINVAL] * len(bad)
    assert b"mgcn_block_spmm_bwd" in lib.mgcn_last_error()
    # nothing to do: no launch, no pointer read
    assert fwd(n_dst=0, n_src=0, rowptr=None, X=None, Y=None) == L.OK
    assert bwd(n_src=0, n_dst=0, rowptr_t=None, dY=None, dX=None) == L.OK
    assert (buf == 0).all()


def test_signatures_and_exports():
    import mgcn
    from mgcn import _lib as L
    for name in ("mgcn_block_spmm_fwd", "mgcn_block_spmm_bwd"):
        assert name in L.SIGNATURES
    assert len(L.SIGNATURES["mgcn_block_spmm_fwd"][1]) == 15
    assert len(L.SIGNATURES["mgcn_block_spmm_bwd"][1]) == 16
    assert mgcn.load().mgcn_abi_version() == 22 == L.ABI_VERSION
    for name in ("block_aggregate", "set_block_convs", "block_convs"):
        assert getattr(mgcn, name) is getattr(mgcn.ops, name) is getattr(mgcn.ops_block_conv, name)
        assert name in mgcn.__all__
    assert mgcn.ops.block_conv_supported is mgcn.ops_block_conv.block_conv_supported
    assert mgcn.ops_block_conv.LOOPS_CODES == {"keep": 0, "drop": 1, "append": 2}


def _cpu_block(n_dst=2, n_src=3, nnz=4):
    """A block-shaped object on the CPU: enough for the argument checks."""
    from mgcn.graph import CSRView, GraphPlan
    from mgcn.ops_block import Block
    rowptr = torch.tensor([0, 2, 4, 4], dtype=torch.int64)
    z = torch.zeros(nnz, dtype=torch.int32)
    view = CSRView(rowptr=rowptr, col=z, eid=torch.arange(nnz, dtype=torch.int32), n_rows=n_src,
                   n_cols=n_src)
    plan = GraphPlan(num_nodes=n_src, nnz=nnz, device=torch.device("cpu"), fwd=view, bwd=view,
                     in_cnt=torch.ones(n_src))
    return Block(plan=plan, n_dst=n_dst, n_src=n_src, src_ids=torch.arange(n_src),
                 parent_eid=torch.arange(nnz), _coo=torch.zeros(2, nnz, dtype=torch.int64))


def test_python_errors_come_before_any_device_call(monkeypatch):
    import mgcn

    def no_device(*a, **k):
        raise AssertionError("an argument error touched the device")
    monkeypatch.setattr(torch.cuda, "_lazy_init", no_device)
    monkeypatch.setattr(torch.cuda, "synchronize", no_device)
    b = _cpu_block()
    x = torch.zeros(3, 4)
    w = torch.ones(4)
    with pytest.raises(ValueError, match="aggr"):
        mgcn.block_aggregate(x, b, "max")
    with pytest.raises(ValueError, match="aggr"):
        mgcn.block_aggregate(x, b, "median")
    with pytest.raises(ValueError, match="loops"):
        mgcn.block_aggregate(x, b, "add", "remove")
    with pytest.raises(ValueError, match="gradient"):
        mgcn.block_aggregate(x, b, "add", "keep", w.clone().requires_grad_(True))
    for bad_x in (torch.zeros(4, 4), torch.zeros(2, 4), torch.zeros(3), torch.zeros(3, 4, 1),
                  torch.zeros(3, 0)):
        with pytest.raises(ValueError):
            mgcn.block_aggregate(bad_x, b)
    for bad_w in (torch.ones(3), torch.ones(4, 1), torch.ones(4, dtype=torch.float64)):
        with pytest.raises(ValueError, match="edge_weight"):
            mgcn.block_aggregate(x, b, "mean", "append", bad_w)
    with pytest.raises(ValueError, match="Block"):
        mgcn.block_aggregate(x, b.plan)
    for bad_x in (x.double(), x.half(), x.to(torch.bfloat16), x.long()):
        with pytest.raises(TypeError, match="float32"):
            mgcn.block_aggregate(bad_x, b)
    for kw in ({}, {"aggr": "mean", "loops": "append", "edge_weight": w}):
        with pytest.raises(mgcn.MgcnError, match="HIP device only"):
            mgcn.block_aggregate(x, b, **kw)


def test_predicate_reads_the_switch_the_dtype_and_the_heavy_rows():
    import mgcn
    from mgcn.ops import block_conv_supported
    b = _cpu_block()
    x = torch.zeros(3, 4)
    w = torch.ones(4)
    assert mgcn.block_convs() is True
    assert block_conv_supported(b, x, None) and block_conv_supported(b, x, w)
    assert not block_conv_supported(b, x.to(torch.bfloat16), None)
    assert not block_conv_supported(b, x[0], None)
    assert not block_conv_supported(b, x, w.clone().requires_grad_(True))
    for view in (b.plan.fwd, b.plan.bwd):
        view.n_heavy = 1
        assert not block_conv_supported(b, x, None)
        view.n_heavy = 0
    try:
        mgcn.set_block_convs(False)
        assert mgcn.block_convs() is False and not block_conv_supported(b, x, None)
    finally:
        mgcn.set_block_convs(True)
    assert block_conv_supported(b, x, None)


def test_switch_is_on_by_default_and_read_from_the_environment():
    env = {k: v for k, v in os.environ.items() if k != "MGCN_BLOCK_CONV"}
    code = "import mgcn; print(int(mgcn.block_convs()))"
    for extra, want in (({}, "1"), ({"MGCN_BLOCK_CONV": "1"}, "1"), ({"MGCN_BLOCK_CONV": "0"}, "0")):
        r = subprocess.run([sys.executable, "-c", code], cwd=PKG_DIR, env={**env, **extra},
                           capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip() == want, r.stderr
