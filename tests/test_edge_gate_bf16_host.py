"""CPU-only checks of the edge gates on bf16 rows: the six mgcn_gate_*_bf16
entries against the header, the library and the ctypes table, their argument
validation before any launch, and the device error of gate_aggregate (no GPU
compute)."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "mgcn.h")

# name -> arguments it takes beyond its fp32 sibling's (cnt on the adjoints)
BF16_ENTRIES = {
    "mgcn_gate_fwd_bf16": 0, "mgcn_gate_bwd_dst_bf16": 1, "mgcn_gate_bwd_src_bf16": 1,
    "mgcn_gate_fwd_sched_bf16": 0, "mgcn_gate_bwd_dst_sched_bf16": 1,
    "mgcn_gate_bwd_src_sched_bf16": 1,
}


def _declared_arg_counts():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2).count(",") + 1
            for m in re.finditer(r"\b(mgcn_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src)}


def test_bf16_entries_are_declared_exported_and_bound():
    from mgcn import _lib
    declared = _declared_arg_counts()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, extra in BF16_ENTRIES.items():
        assert name in declared, f"include/mgcn.h does not declare {name}"
        assert hasattr(lib, name), f"libmgcn.so does not export {name}"
        assert name in _lib.SIGNATURES, f"_lib.SIGNATURES has no {name}"
        n_args = len(_lib.SIGNATURES[name][1])
        assert n_args == declared[name], f"{name}: {n_args} bound, {declared[name]} declared"
        assert n_args == len(_lib.SIGNATURES[name[:-5]][1]) + extra, name
        assert declared[name[:-5]] == len(_lib.SIGNATURES[name[:-5]][1]), name[:-5]


def test_abi_stays_22():
    import mgcn
    assert mgcn.load().mgcn_abi_version() == mgcn._lib.ABI_VERSION == 22


def _calls(lib, n, nnz, C, n_heavy=0, n_giant=0, order=None):
    """Every entry with null arrays: only the host checks can answer."""
    fwd = (n, nnz, C, None, None, None, None, None, None, 0, None, None, C, 0, None, 0, None, C,
           None, None)
    dst = (n, nnz, C, None, None, None, C, None, C, None, None, None, None, None, None, None, None)
    src = (n, nnz, C, None, None, None, None, C, None, None, None, None, None, None, None, None,
           None, C, None)
    return {
        "fwd": lib.mgcn_gate_fwd_bf16(*fwd, None),
        "dst": lib.mgcn_gate_bwd_dst_bf16(*dst, None),
        "src": lib.mgcn_gate_bwd_src_bf16(*src, None),
        "fwd_sched": lib.mgcn_gate_fwd_sched_bf16(*fwd, order, n_heavy, n_giant, None, None),
        "dst_sched": lib.mgcn_gate_bwd_dst_sched_bf16(*dst, order, n_heavy, n_giant, None),
        "src_sched": lib.mgcn_gate_bwd_src_sched_bf16(*src, order, n_heavy, n_giant, None, None),
    }


def test_bf16_entries_validate_before_any_launch():
    """The limits of the fp32 entries, checked on the host: no launch happens
    with a bad shape, a bad schedule or a null array."""
    import mgcn
    lib = mgcn.load()
    assert set(_calls(lib, 0, 0, 8).values()) == {0}  # zero rows: a no-op
    assert set(_calls(lib, 0, 0, 1).values()) == {0}
    assert set(_calls(lib, 0, 0, 1024).values()) == {0}
    assert set(_calls(lib, -1, 0, 8).values()) == {1}
    assert set(_calls(lib, 0, 0, 0).values()) == {1}
    assert set(_calls(lib, 0, 0, 1025).values()) == {1}
    assert b"_bf16: need 1 <= C <= 1024" in lib.mgcn_last_error()
    assert set(_calls(lib, 0, 1 << 31, 8).values()) == {1}
    assert b"nnz < 2^31" in lib.mgcn_last_error()
    assert set(_calls(lib, 4, 0, 8).values()) == {1}  # rows with null arrays
    assert b"_bf16: null" in lib.mgcn_last_error()
    order = ctypes.c_void_p(ctypes.addressof((ctypes.c_int32 * 4)()))
    bad = _calls(lib, 0, 0, 8, n_heavy=0, n_giant=1, order=order)  # n_giant > n_heavy
    assert {k: v for k, v in bad.items() if k.endswith("sched")} == {
        "fwd_sched": 1, "dst_sched": 1, "src_sched": 1}
    assert b"n_giant <= n_heavy" in lib.mgcn_last_error()
    # cnt is the mean's, win_mask max's: both at once is refused
    one = ctypes.c_void_p(ctypes.addressof((ctypes.c_float * 4)()))
    assert lib.mgcn_gate_bwd_dst_bf16(0, 0, 8, None, None, None, 8, None, 8, None, None, one, None,
                                      None, None, None, one, None) == 1
    assert b"exclude each other" in lib.mgcn_last_error()
    assert lib.mgcn_gate_bwd_src_bf16(0, 0, 8, None, None, None, None, 8, None, None, None, None,
                                      one, None, None, None, None, 8, one, None) == 1
    assert b"exclude each other" in lib.mgcn_last_error()


def _plan_stub(n):
    """gate_aggregate checks the device before it touches the plan."""
    class View:
        rowptr = torch.zeros(n + 1, dtype=torch.int64)

    class Plan:
        fwd = View()
        num_nodes = n
        nnz = 0
    return Plan()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cpu_tensors_raise(dtype):
    import mgcn
    from mgcn.ops import gate_aggregate
    hx = torch.randn(5, 8).to(dtype)
    w = torch.randn(8)
    with pytest.raises(mgcn.MgcnError, match="HIP device"):
        gate_aggregate(hx, _plan_stub(5), None, "add", w, w)
    with pytest.raises(mgcn.MgcnError, match="HIP device"):
        gate_aggregate(hx, _plan_stub(5), None, "mean", w.to(torch.bfloat16),
                       w.to(torch.bfloat16), bias=w)


def test_cpu_bf16_module_raises():
    import mgcn
    from mgcn.models import NodeModelGatedAdditive
    x = torch.randn(5, 4).to(torch.bfloat16)
    ei = torch.tensor([[0, 1, 2], [1, 2, 3]])
    with pytest.raises(mgcn.MgcnError, match="HIP device"):
        NodeModelGatedAdditive(4, 6, edge_gate="proj")(x, ei)
    with pytest.raises(mgcn.MgcnError, match="HIP device"):
        NodeModelGatedAdditive(4, 6, edge_gate="proj").to(torch.bfloat16)(x, ei)
