"""CPU-only checks of the bf16 aggregation's C ABI boundary and dtype dispatch
(no GPU compute): the four new symbols, their validation before any launch,
the shape probe, and what aggregate() does with CPU and float16 tensors."""
import pytest
import torch


def _fwd(lib, n, F, reduce=0, H=None, Y=None, rowptr=None, ld=None):
    ld = F if ld is None else ld
    return lib.mgcn_spmm_fwd_bf16(n, F, rowptr, None, None, None, H, ld, Y, ld, reduce, None, 0,
                                  None, None, None, 0, 0, None)


def _bwd(lib, n, F, reduce=0, dY=None, dH=None, rowptr=None, ld=None):
    ld = F if ld is None else ld
    return lib.mgcn_spmm_bwd_bf16(n, F, rowptr, None, None, None, None, dY, ld, dH, ld, reduce,
                                  None, None, None, None, None, 0, 0, None)


def _colsum(lib, n, F, relu=0):
    return lib.mgcn_relu_bwd_colsum_bf16(n, F, None, None, relu, None, None, None, 0, None)


def test_symbols_load_and_abi_stays_22():
    import mgcn
    from mgcn import _lib as L
    lib = mgcn.load()
    for name in ("mgcn_spmm_fwd_bf16", "mgcn_spmm_bwd_bf16", "mgcn_relu_bwd_colsum_bf16",
                 "mgcn_spmm_bf16_supported"):
        assert name in L.SIGNATURES
        assert getattr(lib, name) is not None
    assert lib.mgcn_abi_version() == 22  # the additions are backward compatible


def test_supported_probe():
    import mgcn
    lib = mgcn.load()
    assert lib.mgcn_spmm_bf16_supported(128, 128, 128) == 1
    assert lib.mgcn_spmm_bf16_supported(12, 12, 12) == 0
    assert lib.mgcn_spmm_bf16_supported(128, 132, 128) == 0
    assert lib.mgcn_spmm_bf16_supported(128, 128, 132) == 0
    assert lib.mgcn_spmm_bf16_supported(8, 8, 8) == 1
    assert lib.mgcn_spmm_bf16_supported(128, 160, 136) == 1  # aligned, ld > F
    assert lib.mgcn_spmm_bf16_supported(128, 120, 128) == 0  # ld < F
    assert lib.mgcn_spmm_bf16_supported(0, 0, 0) == 0


def test_c_entries_validate_before_any_launch():
    import mgcn
    lib = mgcn.load()
    # zero-sized work with null pointers: a successful no-op
    assert _fwd(lib, 0, 128) == 0 and _bwd(lib, 0, 128) == 0
    assert _fwd(lib, 5, 0) == 0 and _bwd(lib, 5, 0) == 0
    assert _colsum(lib, 0, 0) == 0 and _colsum(lib, 5, 0) == 0
    # negative sizes
    for rc in (_fwd(lib, -1, 128), _fwd(lib, 4, -8), _bwd(lib, -1, 128), _bwd(lib, 4, -8),
               _colsum(lib, -1, 8), _colsum(lib, 4, -8)):
        assert rc == 1
    assert b"negative size" in lib.mgcn_last_error()
    # bad reduce, also with nothing to do
    assert _fwd(lib, 0, 128, reduce=3) == 1
    assert b"bad reduce" in lib.mgcn_last_error()
    assert _bwd(lib, 0, 128, reduce=-1) == 1
    assert b"bad reduce" in lib.mgcn_last_error()
    # an F the kernels do not take, also with nothing to do
    assert _fwd(lib, 0, 12) == 1
    assert b"F % 8 == 0" in lib.mgcn_last_error()
    assert _bwd(lib, 4, 12) == 1
    assert b"F % 8 == 0" in lib.mgcn_last_error()
    # work to do and null arrays
    assert _fwd(lib, 4, 128) == 1
    assert b"null array" in lib.mgcn_last_error()
    assert _bwd(lib, 4, 128) == 1
    assert b"null array" in lib.mgcn_last_error()
    assert _colsum(lib, 4, 8) == 1
    assert b"dZ is null" in lib.mgcn_last_error()


def test_misaligned_rows_rejected_before_any_launch():
    """Host buffers stand in for device pointers: every check below fails
    before a launch, so nothing dereferences them."""
    import ctypes

    import mgcn
    lib = mgcn.load()
    buf = (ctypes.c_uint16 * 4096)()
    rp = (ctypes.c_int64 * 8)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    p, rowptr = ctypes.c_void_p(base), ctypes.cast(rp, ctypes.c_void_p)
    odd = ctypes.c_void_p(base + 8)
    assert _fwd(lib, 4, 128, H=odd, Y=p, rowptr=rowptr) == 1
    assert b"16-byte aligned" in lib.mgcn_last_error()
    assert _bwd(lib, 4, 128, dY=p, dH=odd, rowptr=rowptr) == 1
    assert b"16-byte aligned" in lib.mgcn_last_error()
    assert _fwd(lib, 4, 128, H=p, Y=p, rowptr=rowptr, ld=132) == 1
    assert b"16-byte aligned" in lib.mgcn_last_error()
    assert _fwd(lib, 4, 128, H=p, Y=p, rowptr=rowptr, ld=120) == 1
    assert b"leading dimension" in lib.mgcn_last_error()
    # max without argmax or win_mask; mean adjoint without cnt
    assert _fwd(lib, 4, 128, reduce=2, H=p, Y=p, rowptr=rowptr) == 1
    assert b"MAX needs" in lib.mgcn_last_error()
    assert _bwd(lib, 4, 128, reduce=1, dY=p, dH=p, rowptr=rowptr) == 1
    assert b"MEAN needs cnt" in lib.mgcn_last_error()


def test_dispatch_by_dtype_on_cpu_tensors():
    import mgcn
    from mgcn import ops
    ei = torch.tensor([[0, 1, 2], [1, 2, 3]])
    x = torch.randn(5, 8)
    with pytest.raises(mgcn.MgcnError, match="HIP device"):
        ops.aggregate(x.to(torch.bfloat16), ei)
    with pytest.raises(TypeError, match="float32 or bfloat16"):
        ops.aggregate(x.to(torch.float16), ei)
    with pytest.raises(TypeError, match="float32 or bfloat16"):
        ops.scatter_("add", x.to(torch.float16), torch.tensor([0, 1, 1, 2, 0]), 3)
    with pytest.raises(mgcn.MgcnError, match="HIP device"):
        ops.scatter_("add", x.to(torch.bfloat16), torch.tensor([0, 1, 1, 2, 0]), 3)


def test_ops_reexports_the_bf16_names():
    from mgcn import ops, ops_bf16
    for name in ("spmm_fwd_bf16", "spmm_bwd_bf16", "relu_bwd_colsum_bf16", "spmm_bf16_supported",
                 "_AggregateBf16", "_SegmentReduceBf16", "ROW_COPIES"):
        assert getattr(ops, name) is getattr(ops_bf16, name)
    assert ops.spmm_bf16_supported(128) and not ops.spmm_bf16_supported(12)
    assert not ops.spmm_bf16_supported(128, 132, 128)
