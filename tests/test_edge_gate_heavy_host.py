"""CPU-only checks of the heavy-row route of the edge gates: the three
mgcn_gate_*_sched entries exist with declared signatures, keep the ABI
version, validate every argument before any launch, and the host switch
round-trips."""
import ctypes
import os

import pytest

SCHED = ("mgcn_gate_fwd_sched", "mgcn_gate_bwd_dst_sched", "mgcn_gate_bwd_src_sched")


@pytest.fixture(scope="module")
def lib():
    import mgcn
    return mgcn.load()


def test_entries_exist_and_are_declared(lib):
    from mgcn import _lib as L
    for name in SCHED:
        assert name in L.SIGNATURES, name
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int
        # the entry without a schedule + order, n_heavy, n_giant [, coef]
        extra = 3 if name == "mgcn_gate_bwd_dst_sched" else 4
        assert len(fn.argtypes) == len(L.SIGNATURES[name[:-len("_sched")]][1]) + extra
    assert lib.mgcn_abi_version() == 22  # the additions are backward compatible


# Pointers that are never dereferenced: every call below fails (or is a no-op)
# before a launch.
P = ctypes.c_void_p(0x1000)


def _fwd(lib, n=4, nnz=6, C=8, rowptr=P, Hx=P, Y=P, ldh=None, ldy=None, order=P, n_heavy=1,
         n_giant=0, coef=P):
    ldh = C if ldh is None else ldh
    ldy = C if ldy is None else ldy
    return lib.mgcn_gate_fwd_sched(n, nnz, C, rowptr, P, P, P, P, P, 0, P, Hx, ldh, 0, P, 0, Y,
                                   ldy, P, None, order, n_heavy, n_giant, coef, None)


def _dst(lib, n=4, nnz=6, C=8, rowptr=P, Hx=P, dY=P, ldh=None, lddy=None, order=P, n_heavy=1,
         n_giant=0):
    ldh = C if ldh is None else ldh
    lddy = C if lddy is None else lddy
    return lib.mgcn_gate_bwd_dst_sched(n, nnz, C, rowptr, P, Hx, ldh, dY, lddy, P, P, None, None,
                                       P, P, None, order, n_heavy, n_giant, None)


def _src(lib, n=4, nnz=6, C=8, rowptr=P, dY=P, dHx=P, lddy=None, lddh=None, order=P, n_heavy=1,
         n_giant=0, coef=P):
    lddy = C if lddy is None else lddy
    lddh = C if lddh is None else lddh
    return lib.mgcn_gate_bwd_src_sched(n, nnz, C, rowptr, P, P, dY, lddy, P, None, P, P, None, P,
                                       P, P, dHx, lddh, order, n_heavy, n_giant, coef, None)


def _einval(lib, rc, text):
    from mgcn import _lib as L
    assert rc == L.EINVAL, rc
    assert text in lib.mgcn_last_error(), lib.mgcn_last_error()


@pytest.mark.parametrize("call,name", list(zip((_fwd, _dst, _src), SCHED)), ids=SCHED)
def test_sched_entries_validate_before_any_launch(lib, call, name):
    tag = name.encode() + b":"
    _einval(lib, call(lib, rowptr=None), tag + b" null array")
    for C in (0, 1025):
        _einval(lib, call(lib, C=C), b"C <= 1024")
    _einval(lib, call(lib, n=-1), b"negative size")
    _einval(lib, call(lib, nnz=1 << 31), b"nnz < 2^31")
    _einval(lib, call(lib, n_heavy=2, n_giant=3), b"n_giant <= n_heavy <= n_rows")
    _einval(lib, call(lib, n=4, n_heavy=5), b"n_giant <= n_heavy <= n_rows")
    _einval(lib, call(lib, n_heavy=1, n_giant=-1), b"n_giant <= n_heavy <= n_rows")
    assert lib.mgcn_last_error().startswith(tag)
    # zero rows: a successful no-op, with and without a schedule
    assert call(lib, n=0, nnz=0, n_heavy=0) == 0
    assert call(lib, n=0, nnz=0, order=None, n_heavy=7, n_giant=9) == 0  # counts not read


def test_leading_dimensions_and_scratch(lib):
    for rc in (_fwd(lib, ldh=7), _fwd(lib, ldy=7), _dst(lib, ldh=7), _dst(lib, lddy=7),
               _src(lib, lddy=7), _src(lib, lddh=7)):
        _einval(lib, rc, b"leading dimension too small")
    # a schedule without its scratch (the adjoint by destination needs none)
    _einval(lib, _fwd(lib, coef=None), b"coef scratch")
    _einval(lib, _src(lib, coef=None), b"coef scratch")
    # other null arrays of each entry
    _einval(lib, _fwd(lib, Hx=None), b"null array")
    _einval(lib, _fwd(lib, Y=None), b"null array")
    _einval(lib, _dst(lib, dY=None), b"null array")
    _einval(lib, _src(lib, dHx=None), b"null array")


def test_switch_round_trips():
    from mgcn import ops, ops_gate
    assert callable(ops.set_gate_heavy_rows)
    before = ops.gate_heavy_rows()
    try:
        for v in (False, True, False):
            ops.set_gate_heavy_rows(v)
            assert ops.gate_heavy_rows() is v and ops_gate._GATE_HEAVY is v
    finally:
        ops.set_gate_heavy_rows(before)
    assert before is (os.environ.get("MGCN_GATE_HEAVY", "1") != "0")  # default on
