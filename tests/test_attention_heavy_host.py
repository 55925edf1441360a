"""CPU-only checks of the heavy-row route of the attention launches: the eight
mgcn_(h)att_*_sched entries are declared in include/mgcn.h and in
_lib.SIGNATURES as their siblings without a schedule plus (order, n_heavy,
n_giant[, coef]), keep the ABI version, validate the schedule before any
launch, and the host switch round-trips with its env default."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# entry -> takes the coef scratch
SCHED = {
    "mgcn_att_fwd_sched": True, "mgcn_edge_softmax_sched": False,
    "mgcn_att_bwd_dst_sched": False, "mgcn_att_bwd_src_sched": True,
    "mgcn_hatt_fwd_sched": True, "mgcn_hatt_edge_softmax_sched": False,
    "mgcn_hatt_bwd_dst_sched": False, "mgcn_hatt_bwd_src_sched": True,
}


@pytest.fixture(scope="module")
def lib():
    import mgcn
    return mgcn.load()


def test_entries_are_declared_in_the_header():
    text = open(os.path.join(ROOT, "include", "mgcn.h")).read()
    for name, coef in SCHED.items():
        m = re.search(r"\bint " + name + r"\(([^;]*?)\);", text, re.S)
        assert m, f"{name} is not declared in include/mgcn.h"
        args = [a.strip() for a in m.group(1).split(",")]
        tail = ["const int32_t *order", "int64_t n_heavy", "int64_t n_giant"]
        tail += ["float *coef"] if coef else []
        tail += ["void *stream"]
        assert [" ".join(a.split()) for a in args[-len(tail):]] == tail, (name, args)
        # the arguments before the schedule are the sibling's
        m0 = re.search(r"\bint " + name[:-len("_sched")] + r"\(([^;]*?)\);", text, re.S)
        args0 = [" ".join(a.split()) for a in m0.group(1).split(",")]
        assert [" ".join(a.split()) for a in args[:-len(tail)]] == args0[:-1], name
    assert "#define MGCN_ABI_VERSION 22" in text  # backward-compatible additions


def test_signature_rows(lib):
    from mgcn import _lib as L
    _i64, _vp = ctypes.c_int64, ctypes.c_void_p
    for name, coef in SCHED.items():
        assert name in L.SIGNATURES, name
        res, args = L.SIGNATURES[name]
        res0, args0 = L.SIGNATURES[name[:-len("_sched")]]
        assert res is res0 is ctypes.c_int
        extra = [_vp, _i64, _i64] + ([_vp] if coef else [])
        assert args == args0[:-1] + extra + [args0[-1]], name
        fn = getattr(lib, name)  # the symbol exists in libmgcn.so
        assert fn.argtypes == args
    assert lib.mgcn_abi_version() == 22


# Pointers that are never dereferenced: every call below fails (or is a no-op)
# before a launch.
P = ctypes.c_void_p(0x1000)


def _call(lib, name, n=4, nnz=6, order=P, n_heavy=1, n_giant=0, coef=P):
    hard = name.startswith("mgcn_hatt")
    T = (0.5,) if hard else ()
    sched = (order, n_heavy, n_giant) + ((coef,) if SCHED[name] else ())
    H, C = 2, 4
    if name.endswith("_fwd_sched"):
        args = (n, nnz, H, C, P, P, P, P, 1) + ((P,) + T if hard else ()) + \
               (None, None, P, H * C, P, H * C, P)
    elif name.endswith("edge_softmax_sched"):
        args = (n, nnz, H, P, P, P, P, 1) + ((P,) + T if hard else ()) + (P,)
    elif name.endswith("bwd_dst_sched"):
        args = (n, nnz, H, C, P, P, P, H * C, P, H * C, P, None, P, P, 1, 1) + T + (P, P)
    else:
        args = (n, nnz, H, C, P, P, P, P, H * C, P, None, P, P, P, 1, 0) + T + \
               (P, P, P, P, H * C)
    return getattr(lib, name)(*args, *sched, None)


@pytest.mark.parametrize("name", list(SCHED))
def test_schedule_is_validated_before_any_launch(lib, name):
    from mgcn import _lib as L
    bad = b"n_giant <= n_heavy <= n_rows"
    for kw in (dict(n_heavy=2, n_giant=3), dict(n=4, n_heavy=5), dict(n_heavy=1, n_giant=-1)):
        assert _call(lib, name, **kw) == L.EINVAL
        err = lib.mgcn_last_error()
        assert bad in err and err.startswith(name.encode() + b":"), err
    if SCHED[name]:
        assert _call(lib, name, coef=None) == L.EINVAL
        assert b"coef scratch" in lib.mgcn_last_error()
    # zero rows: a successful no-op, with and without a schedule
    assert _call(lib, name, n=0, nnz=0, n_heavy=0) == 0
    assert _call(lib, name, n=0, nnz=0, order=None, n_heavy=7, n_giant=9) == 0  # counts not read


def test_switch_round_trips():
    from mgcn import ops, ops_attention
    before = ops.attention_heavy_rows()
    try:
        for v in (False, True, False):
            ops.set_attention_heavy_rows(v)
            assert ops.attention_heavy_rows() is v and ops_attention._ATT_HEAVY is v
    finally:
        ops.set_attention_heavy_rows(before)
    assert before is (os.environ.get("MGCN_ATT_HEAVY", "1") != "0")  # default on


@pytest.mark.parametrize("value,expect", [(None, True), ("0", False), ("1", True)])
def test_env_default_is_read_at_import(value, expect):
    env = {k: v for k, v in os.environ.items() if k != "MGCN_ATT_HEAVY"}
    if value is not None:
        env["MGCN_ATT_HEAVY"] = value
    env["PYTHONPATH"] = os.pathsep.join(p for p in sys.path if p)
    out = subprocess.run([sys.executable, "-c",
                          "from mgcn import ops; print(ops.attention_heavy_rows())"],
                         env=env, capture_output=True, text=True, check=True)
    assert out.stdout.strip() == str(expect)
