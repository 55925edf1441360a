"""CPU-only checks of the bf16 attention rows: the new C entries against the
header, the library and the ctypes table, their argument validation, and the
dtype / device errors of the two ops (no GPU compute)."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "mgcn.h")

BF16_ENTRIES = (
    "mgcn_att_scores_bf16", "mgcn_att_fwd_bf16", "mgcn_att_bwd_dst_bf16", "mgcn_att_bwd_src_bf16",
    "mgcn_att_dst_fold_bf16", "mgcn_hatt_fwd_bf16", "mgcn_hatt_bwd_dst_bf16",
    "mgcn_hatt_bwd_src_bf16", "mgcn_hatt_gather_bf16",
)
# fp32 scores alone: no bf16 sibling
SCORE_ONLY = ("mgcn_edge_softmax", "mgcn_hatt_edge_softmax", "mgcn_hatt_select")


def test_bf16_entries_are_declared_exported_and_bound():
    from mgcn import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(mgcn_[a-z0-9_]+)\s*\(", src))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in BF16_ENTRIES:
        assert name in declared, f"include/mgcn.h does not declare {name}"
        assert hasattr(lib, name), f"libmgcn.so does not export {name}"
        assert name in _lib.SIGNATURES, f"_lib.SIGNATURES has no {name}"
        # the sibling takes the fp32 entry's arguments; the two bwd_src entries
        # and the fold take the fp32 hand-off row as one more pointer
        extra = 1 if name.endswith(("bwd_src_bf16", "dst_fold_bf16")) else 0
        assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[name[:-5]][1]) + extra, name
    for name in SCORE_ONLY:
        assert name + "_bf16" not in declared and not hasattr(lib, name + "_bf16")


def test_abi_stays_22():
    import mgcn
    assert mgcn.load().mgcn_abi_version() == mgcn._lib.ABI_VERSION == 22


def _calls(lib, n, nnz, H, C):
    ld = H * C
    return {
        "scores": lib.mgcn_att_scores_bf16(n, H, C, None, ld, None, None, None, None),
        "fwd": lib.mgcn_att_fwd_bf16(n, nnz, H, C, None, None, None, None, 0, None, None, None,
                                     ld, None, ld, None, None),
        "bwd_dst": lib.mgcn_att_bwd_dst_bf16(n, nnz, H, C, None, None, None, ld, None, ld, None,
                                             None, None, None, 0, 1, None, None, None),
        "bwd_src": lib.mgcn_att_bwd_src_bf16(n, nnz, H, C, None, None, None, None, ld, None, None,
                                             None, None, None, 0, 0, None, None, None, None, ld,
                                             None, None),
        "dst_fold": lib.mgcn_att_dst_fold_bf16(n, nnz, H, C, None, None, None, None, None, None,
                                               ld, None),
        "hfwd": lib.mgcn_hatt_fwd_bf16(n, nnz, H, C, None, None, None, None, 0, None, 1.0, None,
                                       None, None, ld, None, ld, None, None),
        "hbwd_dst": lib.mgcn_hatt_bwd_dst_bf16(n, nnz, H, C, None, None, None, ld, None, ld, None,
                                               None, None, None, 0, 1, 1.0, None, None, None),
        "hbwd_src": lib.mgcn_hatt_bwd_src_bf16(n, nnz, H, C, None, None, None, None, ld, None,
                                               None, None, None, None, 0, 0, 1.0, None, None,
                                               None, None, ld, None, None),
        "gather": lib.mgcn_hatt_gather_bf16(n, nnz, H, C, None, None, None, None, ld, None, ld,
                                            None),
    }


def test_bf16_entries_validate_before_any_launch():
    """The limits of the fp32 entries, checked on the host: no launch happens
    with a bad shape or a null array."""
    import mgcn
    lib = mgcn.load()
    assert set(_calls(lib, 0, 0, 2, 8).values()) == {0}  # zero rows: a no-op
    assert set(_calls(lib, -1, 0, 2, 8).values()) == {1}
    assert set(_calls(lib, 0, 0, 0, 8).values()) == {1}
    assert set(_calls(lib, 0, 0, 17, 8).values()) == {1}
    assert b"1 <= H <= 16" in lib.mgcn_last_error()
    assert set(_calls(lib, 0, 0, 1, 1025).values()) == {1}
    assert set(_calls(lib, 0, 0, 16, 65).values()) == {1}
    assert set(_calls(lib, 0, 0, 1, 1024).values()) == {0}
    assert set(_calls(lib, 0, 0, 16, 64).values()) == {0}
    assert set(_calls(lib, 0, 0, 2, 0).values()) == {1}
    bad = _calls(lib, 0, 1 << 28, 8, 4)
    assert all(bad[k] == 1 for k in bad if k != "scores")
    assert set(_calls(lib, 4, 0, 2, 8).values()) == {1}  # rows with null arrays
    assert b"_bf16: null" in lib.mgcn_last_error()
    assert lib.mgcn_hatt_fwd_bf16(0, 0, 2, 8, None, None, None, None, 0, None, 0.0, None, None,
                                  None, 16, None, 16, None, None) == 1
    assert b"temperature" in lib.mgcn_last_error()


def _plan_stub(n):
    """attention_aggregate checks dtype and device before it touches the plan."""
    class View:
        rowptr = torch.zeros(n + 1, dtype=torch.int64)
    class Plan:
        fwd = View()
        num_nodes = n
        nnz = 0
    return Plan()


@pytest.mark.parametrize("hard", [False, True])
def test_dtype_and_device_errors(hard):
    import mgcn
    from mgcn.ops import attention_aggregate, hard_attention_aggregate
    att = torch.randn(1, 2, 8)

    def call(Hp):
        if hard:
            return hard_attention_aggregate(Hp, att, _plan_stub(5), 2, training=True)
        return attention_aggregate(Hp, att, _plan_stub(5), 2)

    with pytest.raises(mgcn.MgcnError, match="HIP device"):
        call(torch.randn(5, 8).to(torch.bfloat16))
    with pytest.raises(mgcn.MgcnError, match="HIP device"):
        call(torch.randn(5, 8))
    with pytest.raises(TypeError, match="float32 or bfloat16"):
        call(torch.randn(5, 8).to(torch.float16))
    with pytest.raises(TypeError, match="float32 or bfloat16"):
        call(torch.randn(5, 8).to(torch.float64))


def test_cpu_bf16_module_raises():
    import mgcn
    from mgcn.models import NodeModelAttention, NodeModelHardAttention
    x = torch.randn(5, 4).to(torch.bfloat16)
    ei = torch.tensor([[0, 1, 2], [1, 2, 3]])
    for cls in (NodeModelAttention, NodeModelHardAttention):
        with pytest.raises(mgcn.MgcnError, match="HIP device"):
            cls(4, 6, nheads=2)(x, ei)
        with pytest.raises(mgcn.MgcnError, match="HIP device"):
            cls(4, 6, nheads=2).to(torch.bfloat16)(x, ei)


def test_head_combine_accumulates_in_fp32_and_rounds_once():
    """models._combine_heads on bf16 rows: fp32 sum / mean over heads plus the
    bias (fp32 or bf16), one rounding; fp32 rows take the reference's ops."""
    from mgcn.models import _combine_heads
    g = torch.Generator().manual_seed(3)
    y = torch.randn(9, 3 * 5, generator=g).to(torch.bfloat16)
    b = torch.randn(5, generator=g)
    for combine in ("add", "mean"):
        f = y.float().view(-1, 3, 5)
        red = f.sum(dim=1) if combine == "add" else f.mean(dim=1)
        for bias in (None, b, b.to(torch.bfloat16)):
            want = red if bias is None else red + bias.float()
            got = _combine_heads(y, 3, 5, combine, bias)
            assert got.dtype == torch.bfloat16
            assert torch.equal(got.view(torch.int16), want.to(torch.bfloat16).view(torch.int16))
    assert _combine_heads(y, 3, 5, "cat", None) is y
    bc = torch.randn(15, generator=g)
    got = _combine_heads(y, 3, 5, "cat", bc)
    assert torch.equal(got.view(torch.int16),
                       (y.float() + bc).to(torch.bfloat16).view(torch.int16))
    y32 = y.float()
    assert torch.equal(_combine_heads(y32, 3, 5, "add", b), y32.view(-1, 3, 5).sum(dim=1) + b)
    assert _combine_heads(y32, 3, 5, "cat", None) is y32
