"""Host checks (no GPU) of the one launch path of mgcn.ops (mgcn._call) and of
the module surface mgcn.ops keeps over the modules split out of it."""
import inspect
import subprocess
import sys

import pytest
import torch

from conftest import PKG_DIR
from mgcn import _call, _lib as L, ops

DEV = torch.device("cuda")  # index None: the guard is a no-op, nothing touches a device


@pytest.fixture
def events():
    ev = []
    ops.set_kernel_timer(lambda *a: ev.append(("timer",) + a))
    yield ev
    ops.set_kernel_timer(None)


def _fake(ev, rc):
    def fn(*args):
        ev.append(("call",) + args)
        return rc
    return fn


def test_launch_brackets_the_call(events):
    _call.launch("spmm_fwd", "mgcn_spmm_fwd", DEV, 70, 370, _fake(events, L.OK), 1, "two")
    assert events == [("timer", "spmm_fwd", True, 70, 370), ("call", 1, "two"),
                      ("timer", "spmm_fwd", False)]


@pytest.mark.parametrize("rc,exc", [(L.EINVAL, L.MgcnError), (L.EWORKSPACE, L.MgcnError),
                                    (L.EINDEX, IndexError)])
def test_failed_call_records_the_stop_then_raises(events, monkeypatch, rc, exc):
    class _Lib:  # L.check asks the library for the message of a failed call
        @staticmethod
        def mgcn_last_error():
            return b"bad argument"
    monkeypatch.setattr(L, "load", lambda path=None: _Lib)
    with pytest.raises(exc, match="mgcn_gemm_tn_split.*bad argument"):
        _call.launch("gemm_tn", "mgcn_gemm_tn_split", DEV, 5, None, _fake(events, rc))
    assert events == [("timer", "gemm_tn", True, 5, None), ("call",), ("timer", "gemm_tn", False)]


def test_untimed_launches_never_call_the_timer(events):
    _call.launch(None, "mgcn_relu_mask", DEV, 5, None, _fake(events, L.OK), 7)
    assert events == [("call", 7)]
    ops.set_kernel_timer(None)
    ev = []
    _call.launch("spmm_fwd", "mgcn_spmm_fwd", DEV, 5, 9, _fake(ev, L.OK), 7)
    assert ev == [("call", 7)]


def test_timer_hook_is_shared_with_ops():
    t = lambda *a: None  # noqa: E731
    ops.set_kernel_timer(t)
    try:
        assert _call._TIMER is t and ops._TIMER is t
    finally:
        ops.set_kernel_timer(None)
    assert _call._TIMER is None and ops._TIMER is None


# Every name mgcn/ops.py defined at module level (functions, classes, constants
# and switches) before it was split, but the two private helpers that the
# split retired by design: _att_call (the attention launches take
# _call.launch like every other) and _spmm_xw_bwd_packed (spmm_xw_bwd's packed
# form, now inside spmm_xw_bwd with one launch tail).
OPS_NAMES = """
_TIMER _FUSE_XW _Z_MIDDLE _TOP_FULL _TOP_HCS _TOP_CS_DEFER _MAX_FULL set_fused_layers
set_z_middle set_kernel_timer _contig_f32 spmm_fwd XW_MAX_TABLE_BYTES spmm_xw_supported
xw_full_supported mask_words layer_fusable spmm_xw_fwd spmm_xw_bwd spmm_bwd
relu_bwd_colsum gemm_tn gemm_tn_split gemm_nn_supported gemm_nn_epi_supported make_relu_mask
gemm_nn gemm_bwd_supported gemm_bwd dw_pass_supported dw_pass_cs dw_pass SMALL_K gemm_small_k
VENDOR_GEMMS mm_route _mm _mm_t _gemm_batched _bstr _Bmm bmm _Linear _LinearBias linear_bias
linear max_mask _Aggregate aggregate edge_weight_grad _AggregateW aggregate_plan _LayerXW
gcn_layer _Bwd _TopBias _LayerPlan _StackPlan _plan_stack _GCNStack gcn_stack residual_act
residual_act_bwd _ResidualGCNLayer _aligned_rows residual_layer_supported _ResidualLayerFused
_ptr_array _int_array _param_f32 _ResidualStack residual_stack input_layer_supported _InputLayer
residual_gcn_layer _AttentionAggregate attention_aggregate _HardAttentionTrain
_HardAttentionEval hard_attention_aggregate _SegmentReduce scatter_ segment_mean _SegmentMean
pack_rows_count pack_rows_values PackedTable packed_row_bits packed_cols PACK_ROWS_WIDTHS
pack_rows unpack_rows
""".split()

SWITCHES = ("_FUSE_XW", "_Z_MIDDLE", "_TOP_FULL", "_TOP_HCS", "_TOP_CS_DEFER", "_MAX_FULL")


def test_ops_keeps_every_name():
    assert len(OPS_NAMES) == 92 and len(set(OPS_NAMES)) == 92
    missing = [n for n in OPS_NAMES if not hasattr(ops, n)]
    assert missing == []


def test_switches_and_their_setters_live_in_ops_itself():
    """tests and scripts set the switches with setattr(ops, ...): the code
    that reads them (_plan_stack, gcn_layer, the *_supported probes) must look
    them up in mgcn.ops' own globals."""
    assert ops.set_fused_layers.__module__ == "mgcn.ops"
    assert ops.set_z_middle.__module__ == "mgcn.ops"
    src = inspect.getsource(ops)
    for name in SWITCHES:
        assert name in vars(ops)
        assert f"\n{name} = os.environ.get(" in src
    for reader in (ops._plan_stack, ops.gcn_layer, ops.residual_layer_supported,
                   ops.input_layer_supported):
        assert reader.__module__ == "mgcn.ops" and reader.__globals__ is vars(ops)


@pytest.mark.parametrize("module", ["_call", "ops_gemm", "ops_attention", "ops_pack", "ops"])
def test_each_module_imports_alone(module):
    """A fresh interpreter imports the module first: an import cycle between
    the layers would fail here."""
    r = subprocess.run([sys.executable, "-c", f"import mgcn.{module}"], cwd=PKG_DIR,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
