"""CPU-only checks of the fused bf16 layer's C ABI boundary and switch (no GPU
compute): the two new symbols, the shape probe, the validation that precedes
any launch, and the default of ``ops.set_bf16_fused_layers``."""
import ctypes
import os
import subprocess
import sys

from conftest import PKG_DIR

SUM, MEAN, MAX = 0, 1, 2


def _call(lib, n_rows=4, f=128, rowptr=None, X=None, ldx=128, B=None, ldb=128, Y=None, ldy=128,
          Z=None, ldz=128, reduce=SUM, cnt=None):
    return lib.mgcn_spmm_xw_bf16(n_rows, f, f, rowptr, None, None, None, cnt, X, ldx, B, ldb, 0,
                                 None, 0, Y, ldy, Z, ldz, reduce, None)


def test_symbols_load_and_abi_stays_22():
    import mgcn
    from mgcn import _lib as L
    lib = mgcn.load()
    for name in ("mgcn_spmm_xw_bf16", "mgcn_spmm_xw_bf16_supported"):
        assert name in L.SIGNATURES and getattr(lib, name) is not None
    assert lib.mgcn_abi_version() == 22  # a backward-compatible addition


def test_supported_probe():
    import mgcn
    lib = mgcn.load()
    for fi in (0, 64, 128, 136, 256):
        for fo in (64, 128, 256):
            for reduce in (SUM, MEAN, MAX, 7):
                want = fi == fo == 128 and reduce in (SUM, MEAN)
                assert bool(lib.mgcn_spmm_xw_bf16_supported(fi, fo, reduce)) == want


def test_entry_validates_before_any_launch():
    """Host buffers stand in for device pointers: every failing check comes
    before a launch, so nothing dereferences them."""
    import mgcn
    lib = mgcn.load()
    buf = (ctypes.c_uint16 * 8192)()
    rp = (ctypes.c_int64 * 8)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    p, odd = ctypes.c_void_p(base), ctypes.c_void_p(base + 8)
    rowptr = ctypes.cast(rp, ctypes.c_void_p)
    # nothing to do: success, also with null arrays
    assert _call(lib, n_rows=0) == 0
    assert _call(lib, n_rows=-1) == 1 and b"negative size" in lib.mgcn_last_error()
    # shapes and reduces the kernel does not take, also with nothing to do
    assert _call(lib, n_rows=0, f=64) == 1 and b"unsupported" in lib.mgcn_last_error()
    assert _call(lib, reduce=MAX) == 1 and b"unsupported" in lib.mgcn_last_error()
    # the adjoint's per-edge division goes with a sum
    assert _call(lib, rowptr=rowptr, X=p, B=p, Y=p, reduce=MEAN, cnt=p) == 1
    assert b"cnt" in lib.mgcn_last_error()
    # work to do and null arrays
    assert _call(lib) == 1 and b"null array" in lib.mgcn_last_error()
    # leading dimensions and alignment, of every row operand
    ok = dict(rowptr=rowptr, X=p, B=p, Y=p)
    assert _call(lib, **ok, ldx=120) == 1 and b"leading dimension" in lib.mgcn_last_error()
    for bad in (dict(ldx=132), dict(ldy=132), dict(ldb=132), dict(Z=p, ldz=132), dict(X=odd),
                dict(Y=odd), dict(B=odd), dict(Z=odd)):
        assert _call(lib, **{**ok, **bad}) == 1, bad
        assert b"16-byte aligned" in lib.mgcn_last_error()


def test_switch_is_off_by_default_and_set_by_the_environment():
    env = {k: v for k, v in os.environ.items() if k != "MGCN_BF16_FUSED"}
    code = "from mgcn import ops; print(int(ops._BF16_FUSED))"
    for extra, want in (({}, "0"), ({"MGCN_BF16_FUSED": "0"}, "0"), ({"MGCN_BF16_FUSED": "1"}, "1")):
        r = subprocess.run([sys.executable, "-c", code], cwd=PKG_DIR, env={**env, **extra},
                           capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip() == want, r.stderr


def test_setter_and_reexports():
    from mgcn import ops, ops_bf16
    for name in ("spmm_xw_bf16", "spmm_xw_fwd_bf16", "spmm_xw_bwd_bf16", "spmm_xw_bf16_supported",
                 "_LayerXWBf16"):
        assert getattr(ops, name) is getattr(ops_bf16, name)
    assert ops.set_bf16_fused_layers.__module__ == "mgcn.ops"
    before = ops._BF16_FUSED
    try:
        ops.set_bf16_fused_layers(True)
        assert ops._BF16_FUSED is True
        ops.set_bf16_fused_layers(False)
        assert ops._BF16_FUSED is False
    finally:
        ops.set_bf16_fused_layers(before)
