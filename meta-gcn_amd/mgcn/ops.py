"""Autograd-aware aggregation ops on top of libmgcn.

``aggregate`` is the fused replacement for the reference's message-passing
core (src/gcn_meta/models/gcn_base_models.py:209-241 + common.py:37-66):

    x_j = index_select(H, 0, src) * norm      # [E, F] materialised
    y   = torch_scatter.scatter_{add,mean,max}(x_j, dst, dim_size=N)
    y[y == -1e38] = 0                          # max only
    y   = y + bias ; y = relu(y)               # layer epilogue

Here it is one HIP kernel per direction (libmgcn ``mgcn_spmm_fwd`` /
``mgcn_spmm_bwd``); the [E, F] tensor never exists.  Gradients follow the
reference's autograd graph operation for operation (gather of dY, multiply by
norm, index_add over sources in edge order; mean divides dY by the count;
max routes through the saved argmax), so the adjoint is bit-identical too.
"""
from __future__ import annotations

import enum
import os
from dataclasses import dataclass

import torch

from . import _call
from . import _lib as L
from ._call import _aligned_rows, _contig_f32, launch, set_kernel_timer, workspace  # noqa: F401
from .graph import CSRView, GraphPlan, NormPlan, plan_for
# The layers below this module (the launch path): every name they
# define stays importable from here.
from .ops_gemm import (SMALL_K, VENDOR_GEMMS, _Bmm, _bstr, _gemm_batched,  # noqa: F401
                       _Linear, _LinearBias, _mm, _mm_t, bmm, dw_pass, dw_pass_cs,
                       dw_pass_supported, gemm_bwd, gemm_bwd_supported, gemm_nn,
                       gemm_nn_epi_supported, gemm_nn_supported, gemm_small_k, gemm_tn,
                       gemm_tn_split, linear, linear_bias, make_relu_mask, mm_route,
                       relu_bwd_colsum)
from .ops_attention import (_AttentionAggregate, _HardAttentionEval,  # noqa: F401
                            _HardAttentionTrain, attention_aggregate,
                            attention_heavy_rows, hard_attention_aggregate,
                            set_attention_heavy_rows)
from .ops_noise import (NOISE_KINDS, DeviceDropout, DeviceGumbel, draw_edge_seed,  # noqa: F401
                        edge_noise)
from .ops_sample import (sample_heavy_rows, sample_keep, sample_layers,  # noqa: F401
                         sample_neighbors, set_sample_heavy_rows)
from .ops_block import Block, block_batches, sample_blocks  # noqa: F401
from .ops_block_conv import (LOOPS_CODES, _BlockAggregate, block_aggregate,  # noqa: F401
                             block_conv_supported, block_convs, block_spmm_bwd, block_spmm_fwd,
                             set_block_convs)
from .ops_gate import (_GateAggregate, _GateAggregateBf16, gate_aggregate,  # noqa: F401
                       gate_heavy_rows, set_gate_heavy_rows)
from .ops_multi import (_MultiAggregate, multi_aggregate, multi_kernel_fusable,  # noqa: F401
                        multi_kernel_reason, multi_spmm_bwd, multi_spmm_fwd)
from .ops_bf16 import (ROW_COPIES, _AggregateBf16, _LayerXWBf16, _SegmentReduceBf16,  # noqa: F401
                       relu_bwd_colsum_bf16, spmm_bf16_supported, spmm_bwd_bf16, spmm_fwd_bf16,
                       spmm_xw_bf16, spmm_xw_bf16_supported, spmm_xw_bwd_bf16,
                       spmm_xw_fwd_bf16)
from .ops_pack import (PACK_ROWS_WIDTHS, PackedTable, _SegmentMean, pack_rows,  # noqa: F401
                       pack_rows_count, pack_rows_values, packed_cols, packed_row_bits,
                       segment_mean, unpack_rows)


def __getattr__(name):
    if name == "_TIMER":  # the hook's home is _call
        return _call._TIMER
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


# fused aggregate-then-transform forward for 128 -> 128 sum / mean layers
# (mgcn_spmm_xw_fwd); MGCN_FUSE_XW=0 selects the GEMM + SpMM launches
_FUSE_XW = os.environ.get("MGCN_FUSE_XW", "1") != "0"

# fused bf16 layer (mgcn_spmm_xw_bf16: one launch per direction for a bf16
# 128 -> 128 sum / mean layer).  Opt-in, MGCN_BF16_FUSED=1: it rounds the
# aggregate Z = A x to bf16 where the two-launch route rounds h = x W, so a
# layer's bits (and its error bound) change with the switch
_BF16_FUSED = os.environ.get("MGCN_BF16_FUSED", "0") != "0"

# one launch per direction for a multi-kernel layer (mgcn_multi_spmm_fwd /
# _bwd, :func:`multi_kernel_fusable`); MGCN_FUSE_MULTI=0 keeps the loop over
# the kernels
_FUSE_MULTI = os.environ.get("MGCN_FUSE_MULTI", "1") != "0"


# The route switches of a GCN stack: :func:`_plan_stack` reads them, once per
# forward, and says what each one selects.
_Z_MIDDLE = os.environ.get("MGCN_Z_MIDDLE", "0") != "0"
_TOP_FULL = os.environ.get("MGCN_TOP_FULL", "1") != "0"
_TOP_HCS = os.environ.get("MGCN_TOP_HCS", "0") != "0"
_TOP_CS_DEFER = os.environ.get("MGCN_TOP_CS_DEFER", "1") != "0"
_MAX_FULL = os.environ.get("MGCN_MAX_FULL", "1") != "0"


def set_fused_layers(enabled: bool) -> None:
    """Use (True, the default) or bypass the fused aggregate+transform layer
    kernels (mgcn_spmm_xw_fwd / _bwd) where they apply."""
    global _FUSE_XW
    _FUSE_XW = bool(enabled)


def set_bf16_fused_layers(enabled: bool) -> None:
    """Send (True) a bf16 128 -> 128 sum / mean layer of :func:`gcn_layer`
    through the fused bf16 kernel (mgcn_spmm_xw_bf16), or keep (False, the
    default; env MGCN_BF16_FUSED=1 turns it on) the vendor GEMM followed by
    the bf16 aggregation."""
    global _BF16_FUSED
    _BF16_FUSED = bool(enabled)


def set_fused_multi_kernel(enabled: bool) -> None:
    """Use (True, the default) or bypass the fused multi-kernel route of
    :class:`mgcn.models.GCNMultiKernel` (:func:`multi_kernel_fusable`)."""
    global _FUSE_MULTI
    _FUSE_MULTI = bool(enabled)


def set_z_middle(enabled: bool) -> None:
    """Send the middle layers of a fused stack through the Z^T dY + dX-only
    backward too (True; env MGCN_Z_MIDDLE=1) or keep them on the one dW + dX
    gather kernel (False, the default)."""
    global _Z_MIDDLE
    _Z_MIDDLE = bool(enabled)


def spmm_fwd(view: CSRView, w: torch.Tensor | None, H: torch.Tensor, reduce: int,
             bias: torch.Tensor | None = None, relu: bool = False,
             out: torch.Tensor | None = None, mask_plan: GraphPlan | None = None,
             relu_mask: torch.Tensor | None = None):
    """Y[view.n_rows, F] = epi(reduce_k H[col_k] * w_k); returns (Y, argmax).

    Max with ``mask_plan`` (the plan ``view`` belongs to): instead of argmax
    the kernel writes every edge's winner bits at its slot (int32
    [nnz, ceil(F/32)] bit patterns), returned in argmax's place.
    ``relu_mask`` (int32 [n_rows, 4], with relu and F <= 128) receives the
    Y > 0 bits the dX GEMM's fused ReLU backward reads (:func:`gemm_nn`)."""
    lib = L.load()
    H = _contig_f32(H, "H")
    dev = L.require_device(H, view.rowptr, w, bias)
    if H.size(0) != view.n_cols:
        raise ValueError(f"H has {H.size(0)} rows, graph has {view.n_cols} source nodes")
    F = H.size(1)
    Y = out if out is not None else torch.empty(view.n_rows, F, dtype=torch.float32, device=dev)
    argmax = mask = None
    if reduce == L.REDUCE_MAX:
        if mask_plan is not None:
            mask = torch.empty(max(mask_plan.nnz, 1), (F + 31) // 32, dtype=torch.int32,
                               device=dev)
        else:
            argmax = torch.empty(view.n_rows, F, dtype=torch.int32, device=dev)
    if bias is not None:
        bias = bias.detach().to(torch.float32).contiguous()
        if bias.numel() != F:
            raise ValueError(f"bias has {bias.numel()} entries, expected {F}")
    launch("spmm_fwd", "mgcn_spmm_fwd", dev, view.n_rows, view.edges, lib.mgcn_spmm_fwd,
           view.n_rows, F, L.ptr(view.rowptr), L.ptr(view.col), L.ptr(view.eid), L.ptr(w),
           L.ptr(H), H.stride(0), L.ptr(Y), Y.stride(0), reduce, L.ptr(bias), int(bool(relu)),
           L.ptr(argmax), L.ptr(mask), L.ptr(relu_mask), L.ptr(view.order), view.n_heavy,
           view.n_giant, L.stream_of(dev))
    return Y, (mask if mask is not None else argmax)


# The fused kernels address the gathered table (X forward, dY backward) with
# 32-bit byte offsets: mgcn_spmm_xw_fwd / _bwd reject a table of more than
# 4 GiB - 16 bytes (fused.hip, the n_cols * ld * 4 checks), i.e. more than
# 8,388,607 rows at F = 128.  Larger graphs take the two-launch path, whose
# SpMM indexes with 64-bit offsets.
XW_MAX_TABLE_BYTES = 0xfffffff0


def spmm_xw_supported(view: CSRView, F_in: int, F_out: int, reduce: int,
                      ld: int | None = None) -> bool:
    """True when :func:`spmm_xw_fwd` (``view`` the fwd view, gathering [n_cols,
    F_in] rows of leading dimension ``ld``) or :func:`spmm_xw_bwd` (``view``
    the bwd view, gathering dY, F_in / F_out swapped) takes this layer:
    128 -> 128 or 256 -> 256, sum or mean, no heavy rows (skewed graphs keep
    the GEMM + heavy-row SpMM path); at 128 a gathered table within the
    kernels' 32-bit offsets (:data:`XW_MAX_TABLE_BYTES`; the 256-wide kernels
    give every gathered row a 64-bit base).  At 256 the backward is the
    dX-only form (:func:`xw_full_supported`)."""
    ld = int(F_in) if ld is None else max(int(ld), int(F_in))
    small = int(F_in) <= 128
    return (view.n_heavy == 0 and view.n_cols > 0 and
            (not small or view.n_cols * ld * 4 <= XW_MAX_TABLE_BYTES) and
            bool(L.load().mgcn_spmm_xw_supported(int(F_in), int(F_out), int(reduce))))


def xw_full_supported(F_in: int, F_out: int) -> bool:
    """mgcn_spmm_xw_bwd's dW-accumulating form (and its max adjoint): 128 x 128."""
    return bool(L.load().mgcn_spmm_xw_bwd_full_supported(int(F_in), int(F_out)))


def mask_words(F: int) -> int:
    """int32 ReLU mask words per row: 4 per 128 features (bit b of word
    4 (f >> 7) + v <-> feature f = 128 (f >> 7) + 4 b + v)."""
    return 4 * ((int(F) + 127) // 128)


def layer_fusable(plan: GraphPlan, x: torch.Tensor, W: torch.Tensor, reduce: int) -> bool:
    """Both directions of a layer on ``plan`` fit the fused kernels: the
    forward gathers x over the fwd view, the backward dY over the bwd view."""
    return (x.dim() == 2 and x.dtype == torch.float32 and W.dtype == torch.float32 and
            x.is_cuda and x.size(0) == plan.fwd.n_cols == plan.fwd.n_rows and
            spmm_xw_supported(plan.fwd, W.size(0), W.size(1), reduce, x.stride(0)) and
            spmm_xw_supported(plan.bwd, W.size(1), W.size(0), L.REDUCE_SUM))


def layer_fusable_bf16(plan: GraphPlan, x: torch.Tensor, W: torch.Tensor, reduce: int) -> bool:
    """Both directions of a bf16 layer on ``plan`` fit the fused bf16 kernel
    (:func:`spmm_xw_bf16_supported`: 128 -> 128, sum / mean, no heavy rows in
    either view)."""
    return (x.dim() == 2 and x.dtype == torch.bfloat16 and W.dtype == torch.bfloat16 and
            W.dim() == 2 and x.is_cuda and
            x.size(0) == plan.fwd.n_cols == plan.fwd.n_rows and x.size(1) == W.size(0) and
            spmm_xw_bf16_supported(plan.fwd, W.size(0), W.size(1), reduce) and
            spmm_xw_bf16_supported(plan.bwd, W.size(1), W.size(0), L.REDUCE_SUM))


def spmm_xw_fwd(view: CSRView, w: torch.Tensor | None, X: torch.Tensor, W: torch.Tensor,
                reduce: int, bias: torch.Tensor | None = None, relu: bool = False,
                relu_mask: torch.Tensor | None = None, want_z: bool = False,
                out: torch.Tensor | None = None, z_out: torch.Tensor | None = None):
    """Y = epi((reduce_k X[col_k] * w_k) @ W + bias) in one launch
    (``mgcn_spmm_xw_fwd``): the layer's GEMM fused behind its aggregation, so
    X @ W is never written.  Sum / mean only (they commute with W).  With
    ``want_z`` returns (Y, Z): Z = the aggregated rows before W (for mean
    before the division), from which the backward forms dW = Z^T dY.
    ``out`` / ``z_out``: [n_rows, F] row-major buffers (16-byte aligned rows)
    to write Y / Z into instead of new tensors.  ``X`` may be a
    :class:`PackedTable` (128- or 256-wide layers; the view's columns then
    are packed positions): the rows are gathered from the packed exchange buffers in
    place (``mgcn_spmm_xw_fwd_packed``), bit for bit the dense table's result."""
    lib = L.load()
    packed = isinstance(X, PackedTable)
    if not packed:
        X = _aligned_rows(X, "X")
    W = W.detach()
    dev = L.require_device(X.words if packed else X, W, view.rowptr, w, bias, relu_mask)
    F_in, F_out = W.shape
    if packed:
        if X.F != F_in:
            raise ValueError(f"spmm_xw_fwd: packed table of F = {X.F}, W is [{F_in}, {F_out}]")
    elif X.size(0) != view.n_cols:
        raise ValueError(f"X has {X.size(0)} rows, graph has {view.n_cols} source nodes")
    elif X.size(1) != F_in:
        raise ValueError(f"spmm_xw_fwd: X is [{X.size(0)}, {X.size(1)}], W is [{F_in}, {F_out}]")
    if W.dtype != torch.float32 or W.stride(1) != 1:
        W = W.to(torch.float32).contiguous()
    if bias is not None:
        bias = bias.detach().to(torch.float32).contiguous()
        if bias.numel() != F_out:
            raise ValueError(f"bias has {bias.numel()} entries, expected {F_out}")
    if relu_mask is not None:
        # the kernel writes n_rows x 16 B of mask words through this pointer
        if not relu:
            raise ValueError("spmm_xw_fwd: relu_mask needs relu")
        mw = mask_words(F_out)
        if (relu_mask.shape != (view.n_rows, mw) or relu_mask.dtype != torch.int32 or
                not relu_mask.is_contiguous() or relu_mask.data_ptr() % 16):
            raise ValueError(f"spmm_xw_fwd: relu_mask must be a contiguous, 16-byte aligned "
                             f"int32 [{view.n_rows}, {mw}] tensor")
    Y = out if out is not None else torch.empty(view.n_rows, F_out, dtype=torch.float32,
                                                device=dev)
    Z = None
    if want_z:
        Z = z_out if z_out is not None else torch.empty(view.n_rows, F_in, dtype=torch.float32,
                                                        device=dev)
    for name, t, f in (("out", Y, F_out), ("z_out", Z, F_in)):
        if t is not None and (t.dtype != torch.float32 or t.dim() != 2 or t.size(0) != view.n_rows
                              or t.size(1) != f or t.stride(1) != 1 or t.stride(0) % 4
                              or t.data_ptr() % 16):
            raise ValueError(f"spmm_xw_fwd: {name} must be float32 [{view.n_rows}, {f}] with "
                             f"16-byte aligned rows")
    ws, ws_bytes = workspace(lib.mgcn_spmm_xw_fwd_workspace_bytes(F_in, F_out), dev, or_null=True)
    tname = ("spmm_xw_fwd_z" if want_z else "spmm_xw_fwd") + ("_pk" if packed else "")
    # after the table (the dense one with its row count), both entries take the same arguments
    tail = (L.ptr(W), W.stride(0), L.ptr(bias), L.ptr(Y), Y.stride(0), reduce, int(bool(relu)),
            L.ptr(relu_mask), L.ptr(Z), Z.stride(0) if Z is not None else 0, L.ptr(ws), ws_bytes,
            L.stream_of(dev))
    if packed:
        pk = X.c_struct()
        launch(tname, "mgcn_spmm_xw_fwd_packed", dev, view.n_rows, view.edges,
               lib.mgcn_spmm_xw_fwd_packed, view.n_rows, F_in, F_out, L.ptr(view.rowptr),
               L.ptr(view.col), L.ptr(w), L.byref(pk), *tail)
    else:
        launch(tname, "mgcn_spmm_xw_fwd", dev, view.n_rows, view.edges, lib.mgcn_spmm_xw_fwd,
               view.n_rows, view.n_cols, F_in, F_out, L.ptr(view.rowptr), L.ptr(view.col),
               L.ptr(w), L.ptr(X), X.stride(0), *tail)
    return (Y, Z) if want_z else Y


def spmm_xw_bwd(view_t: CSRView, w_t: torch.Tensor | None, row_scale: torch.Tensor | None,
                dY: torch.Tensor, X: torch.Tensor, W: torch.Tensor, want_dx: bool = True,
                relu_mask: torch.Tensor | None = None, row_div: torch.Tensor | None = None,
                win_mask: torch.Tensor | None = None, slot_map: torch.Tensor | None = None,
                dx_out: torch.Tensor | None = None, colsum_acc: torch.Tensor | None = None,
                dy_colsum_out: torch.Tensor | None = None):
    """Both adjoints of a 128 -> 128 layer from one pass (``mgcn_spmm_xw_bwd``):
    dH = A^T dY [* row_scale] stays on chip, and dW = X^T dH, dX = dH W^T
    (with the lower layer's ReLU mask / row divisor / bias column sums, as
    :func:`gemm_bwd`) are formed from it.  Max: ``win_mask`` (the forward's
    winner bits, :func:`spmm_fwd` with ``mask_plan``) and the plan's
    ``slot_map`` route dY as :func:`spmm_bwd` does.  ``dy_colsum_out`` (a
    float32 [F_out] tensor; the dW + dX form of a whole square graph, no max)
    receives the column sums of dY itself -- the layer's own bias gradient --
    from the same launch (``mgcn_spmm_xw_bwd_hcs``).  Returns
    (dW, dX or None, colsum or None).  ``dY`` may be a :class:`PackedTable`
    (128- or 256-wide, dX-only form X = None; ``mgcn_spmm_xw_bwd_packed``)."""
    lib = L.load()
    packed = isinstance(dY, PackedTable)
    dx_only = X is None  # dW formed by the caller (Z^T dY, :func:`gemm_bwd`)
    if packed:
        if not dx_only or not want_dx or win_mask is not None or dy_colsum_out is not None:
            raise ValueError("spmm_xw_bwd: a packed dY takes the dX-only form (X = None, no max)")
    else:
        dY = _aligned_rows(dY, "dY")
        if not dx_only:
            X = _aligned_rows(X, "X")
    W = W.detach()
    # (the warp-specialised adjoint copies W into LDS with 16-byte loads)
    if W.dtype != torch.float32 or W.stride(1) != 1 or W.stride(0) % 4 or W.data_ptr() % 16:
        W = W.to(torch.float32).contiguous()
    dev = L.require_device(dY.words if packed else dY, X, W, view_t.rowptr, w_t, row_scale,
                           relu_mask, row_div)
    F_in, F_out = W.shape
    M = view_t.n_rows if dx_only else X.size(0)
    if packed:
        if dY.F != F_out:
            raise ValueError(f"spmm_xw_bwd: packed dY of F = {dY.F}, W is [{F_in}, {F_out}]")
    else:
        if dx_only and (not want_dx or win_mask is not None):
            raise ValueError("spmm_xw_bwd: X=None (dX only) needs want_dx and no win_mask")
        if (not dx_only and X.size(1) != F_in) or M != view_t.n_rows or \
                dY.size(0) != view_t.n_cols or dY.size(1) != F_out:
            raise ValueError(f"spmm_xw_bwd: X {None if dx_only else tuple(X.shape)}, dY "
                             f"{tuple(dY.shape)} do not fit the "
                             f"graph ({view_t.n_rows} sources, {view_t.n_cols} destinations)")
        if (win_mask is None) != (slot_map is None):
            raise ValueError("spmm_xw_bwd: win_mask and slot_map go together (max adjoint)")
        if win_mask is not None and (win_mask.dtype != torch.int32 or win_mask.dim() != 2
                                     or win_mask.size(1) != (F_out + 31) // 32):
            raise ValueError("spmm_xw_bwd: win_mask must be int32 [nnz, ceil(F/32)]")
    dW = None if dx_only else torch.empty(F_in, F_out, dtype=torch.float32, device=dev)
    dX = None
    if want_dx:
        dX = dx_out if dx_out is not None else torch.empty(M, F_in, dtype=torch.float32,
                                                           device=dev)
        ok = (dX.dtype == torch.float32 and dX.dim() == 2 and tuple(dX.shape) == (M, F_in) and
              dX.stride(1) == 1)
        if packed and (not ok or dX.stride(0) % 4 or dX.data_ptr() % 16):
            raise ValueError(f"spmm_xw_bwd: dx_out must be float32 [{M}, {F_in}], 16-byte rows")
        if not packed and (not ok or dX.stride(0) < F_in):
            raise ValueError(f"spmm_xw_bwd: dx_out must be float32 [{M}, {F_in}], row-major")
    colsum = None
    if relu_mask is not None:
        if not want_dx:
            raise ValueError("spmm_xw_bwd: relu_mask needs want_dx")
        mw = mask_words(F_in)
        if relu_mask.shape != (M, mw) or relu_mask.dtype != torch.int32:
            raise ValueError(f"spmm_xw_bwd: relu_mask must be int32 [{M}, {mw}]")
        relu_mask = relu_mask.contiguous()
        if colsum_acc is not None:
            if not dx_only or colsum_acc.dtype != torch.float32 or \
                    tuple(colsum_acc.shape) != (F_in,) or not colsum_acc.is_contiguous():
                raise ValueError(f"spmm_xw_bwd: colsum_acc must be a contiguous float32 [{F_in}] "
                                 f"tensor (dX-only form)")
            L.require_device(colsum_acc)
            colsum = colsum_acc
        else:
            colsum = torch.empty(F_in, dtype=torch.float32, device=dev)
    elif colsum_acc is not None:
        raise ValueError("spmm_xw_bwd: colsum_acc needs relu_mask")
    acc_flag = 1 if colsum_acc is not None else 0
    if dy_colsum_out is not None:
        if (dx_only or not want_dx or win_mask is not None or view_t.n_rows != view_t.n_cols or
                dy_colsum_out.dtype != torch.float32 or
                tuple(dy_colsum_out.shape) != (F_out,) or not dy_colsum_out.is_contiguous()):
            raise ValueError("spmm_xw_bwd: dy_colsum_out needs the dW + dX form of a square "
                             f"graph (no max) and a contiguous float32 [{F_out}] tensor")
        L.require_device(dy_colsum_out)
    ws, ws_bytes = workspace(lib.mgcn_spmm_xw_bwd_workspace_bytes(M, F_in, F_out), dev)
    graph = (L.ptr(view_t.rowptr), L.ptr(view_t.col), L.ptr(w_t), L.ptr(row_scale))
    epi = (L.ptr(relu_mask), L.ptr(row_div), L.ptr(colsum))
    if packed:
        tname, sym = "spmm_xw_bwd_dx_pk", "mgcn_spmm_xw_bwd_packed"
        pk = dY.c_struct()
        args = (M, F_in, F_out, *graph, L.byref(pk), L.ptr(W), W.stride(0), L.ptr(dX),
                dX.stride(0), *epi, acc_flag)
    elif dy_colsum_out is not None:
        tname, sym = "spmm_xw_bwd", "mgcn_spmm_xw_bwd_hcs"
        args = (M, view_t.n_cols, *graph, L.ptr(dY), dY.stride(0), L.ptr(X), X.stride(0),
                L.ptr(W), W.stride(0), L.ptr(dW), dW.stride(0), 0, L.ptr(dX), dX.stride(0), *epi,
                L.ptr(dy_colsum_out))
    else:
        tname = "spmm_xw_bwd_dx" if dx_only else "spmm_xw_bwd" if want_dx else "spmm_xw_bwd_dw"
        sym = "mgcn_spmm_xw_bwd"
        args = (M, view_t.n_cols, F_in, F_out, *graph, L.ptr(dY), dY.stride(0), L.ptr(X),
                0 if dx_only else X.stride(0), L.ptr(W), W.stride(0), L.ptr(dW),
                0 if dx_only else dW.stride(0), acc_flag, L.ptr(dX),
                dX.stride(0) if dX is not None else 0, *epi, L.ptr(win_mask), L.ptr(slot_map))
    launch(tname, sym, dev, view_t.n_rows, view_t.edges, getattr(lib, sym), *args, L.ptr(ws),
           ws_bytes, L.stream_of(dev))
    return dW, dX, colsum


def spmm_bwd(view_t: CSRView, w_t: torch.Tensor | None, row_scale: torch.Tensor | None,
             dY: torch.Tensor, reduce: int, cnt: torch.Tensor | None = None,
             argmax: torch.Tensor | None = None, out: torch.Tensor | None = None,
             accumulate: bool = False, win_mask: torch.Tensor | None = None,
             slot_map: torch.Tensor | None = None) -> torch.Tensor:
    """dH[view_t.n_rows, F] = sum_k g(dY[col_k]) * w_k  [* row_scale]."""
    lib = L.load()
    dY = _contig_f32(dY, "dY")
    dev = L.require_device(dY, view_t.rowptr, w_t, row_scale)
    F = dY.size(1)
    dH = out if out is not None else torch.empty(view_t.n_rows, F, dtype=torch.float32,
                                                 device=dev)
    launch("spmm_bwd", "mgcn_spmm_bwd", dev, view_t.n_rows, view_t.edges, lib.mgcn_spmm_bwd,
           view_t.n_rows, F, L.ptr(view_t.rowptr), L.ptr(view_t.col), L.ptr(view_t.eid),
           L.ptr(w_t), L.ptr(row_scale), L.ptr(dY), dY.stride(0), L.ptr(dH), dH.stride(0), reduce,
           L.ptr(cnt), L.ptr(argmax), L.ptr(win_mask), L.ptr(slot_map), int(bool(accumulate)),
           L.ptr(view_t.order), view_t.n_heavy, view_t.n_giant, L.stream_of(dev))
    return dH


def max_mask(plan: GraphPlan, argmax: torch.Tensor) -> torch.Tensor:
    """Winner bits of every edge at its fwd slot (mgcn_max_mask): int32
    [nnz, ceil(F/32)] (bit patterns), replacing argmax in the backward."""
    lib = L.load()
    F = argmax.size(1)
    W = (F + 31) // 32
    dev = argmax.device
    mask = torch.empty(max(plan.nnz, 1), W, dtype=torch.int32, device=dev)
    launch(None, "mgcn_max_mask", dev, None, None, lib.mgcn_max_mask,
           plan.fwd.n_rows, F, L.ptr(plan.fwd.rowptr), L.ptr(plan.fwd.eid), L.ptr(argmax),
           L.ptr(mask), L.stream_of(dev))
    return mask


class _Aggregate(torch.autograd.Function):
    """y = epi(A_norm (x) H) with bias and ReLU fused; see module docstring.
    Max saves the per-edge winner bits (max_mask), not the argmax rows."""

    @staticmethod
    def forward(ctx, H, bias, plan: GraphPlan, norm: NormPlan, reduce: int, relu: bool):
        Y, mask = spmm_fwd(plan.fwd, norm.w_fwd, H, reduce, bias, relu, mask_plan=plan)
        ctx.plan, ctx.norm, ctx.reduce, ctx.relu = plan, norm, reduce, relu
        ctx.has_bias = bias is not None
        ctx.save_for_backward(Y if relu else None, mask)  # max: winner bits per edge
        return Y

    @staticmethod
    def backward(ctx, dZ):
        Y, mask = ctx.saved_tensors
        plan, norm = ctx.plan, ctx.norm
        need_h = ctx.needs_input_grad[0]
        need_b = ctx.has_bias and ctx.needs_input_grad[1]
        mean = ctx.reduce == L.REDUCE_MEAN
        # mean: dY rows divided by their count once here (bitwise the same as
        # dividing every gathered copy), so the adjoint is a plain sum
        dY, db = relu_bwd_colsum(dZ, Y, ctx.relu, need_b,
                                 row_div=plan.in_cnt if (mean and need_h) else None)
        dH = None
        if need_h:
            dH = spmm_bwd(plan.bwd, norm.w_bwd, norm.row_scale_bwd, dY,
                          L.REDUCE_SUM if mean else ctx.reduce, win_mask=mask,
                          slot_map=plan.slot_map() if mask is not None else None)
        return dH, db, None, None, None, None


def _feature_dtype(t: torch.Tensor, name: str) -> bool:
    """True for a bfloat16 feature tensor (the bf16 kernels of
    :mod:`mgcn.ops_bf16`), False for float32; any other dtype raises."""
    if t.dtype == torch.float32:
        return False
    if t.dtype == torch.bfloat16:
        return True
    raise TypeError(f"{name} must be float32 or bfloat16, got {t.dtype}")


def aggregate(H: torch.Tensor, edge_index: torch.Tensor, aggr: str = "add",
              deg_norm: str | None = None, deg: torch.Tensor | None = None,
              edge_weight: torch.Tensor | None = None, bias: torch.Tensor | None = None,
              relu: bool = False, num_nodes: int | None = None) -> torch.Tensor:
    """Fused gather -> scale -> reduce -> (+bias) -> (ReLU) over ``edge_index``.

    Semantics of NodeModelAdditive.forward after its matmul
    (gcn_base_models.py:209-241): messages flow ``edge_index[0] -> [1]``;
    ``deg_norm`` in {None, 'sm', 'rw'} as degnorm_const; ``aggr`` in
    {'add', 'mean', 'max'} as common.scatter_.
    """
    if aggr not in L.REDUCE_CODES:
        raise ValueError(f"aggr must be one of add/mean/max, got {aggr!r}")
    if deg_norm not in L.NORM_CODES:
        raise ValueError(f"deg_norm must be None, 'sm' or 'rw', got {deg_norm!r}")
    _feature_dtype(H, "H")
    n = H.size(0) if num_nodes is None else int(num_nodes)
    plan = plan_for(edge_index, n)
    norm = plan.norm(deg_norm, deg=deg, edge_weight=edge_weight)
    return aggregate_plan(H, plan, norm, aggr, bias, relu)


def edge_weight_grad(view: CSRView, H: torch.Tensor, dY: torch.Tensor,
                     win_mask: torch.Tensor | None = None) -> torch.Tensor:
    """dw[k] = sum_f dY[row(k), f] * H[col[k], f] for every slot k of the fwd
    view (``mgcn_edge_weight_grad``; max: the features slot k won), in slot
    order: the gradient of the aggregation with respect to its per-slot edge
    weights (the reference's ``x_j * norm.view(-1, 1)`` adjoint,
    gcn_base_models.py:217-224)."""
    lib = L.load()
    H = _contig_f32(H, "H")
    dY = _contig_f32(dY, "dY")
    dev = L.require_device(H, dY, view.rowptr)
    F = H.size(1)
    if dY.size(1) != F or H.size(0) != view.n_cols or dY.size(0) != view.n_rows:
        raise ValueError(f"edge_weight_grad: H {tuple(H.shape)}, dY {tuple(dY.shape)} do not fit "
                         f"the view ({view.n_rows} rows, {view.n_cols} columns)")
    dw = torch.empty(view.nnz, dtype=torch.float32, device=dev)
    launch(None, "mgcn_edge_weight_grad", dev, None, None, lib.mgcn_edge_weight_grad,
           view.n_rows, F, L.ptr(view.rowptr), L.ptr(view.col), L.ptr(H), H.stride(0), L.ptr(dY),
           dY.stride(0), L.ptr(win_mask), L.ptr(dw), L.stream_of(dev))
    return dw


class _AggregateW(torch.autograd.Function):
    """:class:`_Aggregate` with the fwd per-slot weights as an autograd input
    (a :class:`NormPlan` built with ``grad``): the backward also returns their
    gradient, from which autograd reaches edge_weight / deg through the
    differentiable degnorm_const of graph._grad_norm."""

    @staticmethod
    def forward(ctx, H, w_fwd, bias, plan: GraphPlan, norm: NormPlan, reduce: int, relu: bool):
        Y, mask = spmm_fwd(plan.fwd, w_fwd.detach(), H, reduce, bias, relu, mask_plan=plan)
        ctx.plan, ctx.norm, ctx.reduce, ctx.relu = plan, norm, reduce, relu
        ctx.has_bias = bias is not None
        ctx.save_for_backward(H, Y if relu else None, mask)
        return Y

    @staticmethod
    def backward(ctx, dZ):
        H, Y, mask = ctx.saved_tensors
        plan, norm = ctx.plan, ctx.norm
        need_h = ctx.needs_input_grad[0]
        need_w = ctx.needs_input_grad[1]
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        mean = ctx.reduce == L.REDUCE_MEAN
        # mean: dY divided by the counts once, for the adjoint gather and for
        # the weights' gradient alike (scatter_mean's backward, common.py:59)
        dY, db = relu_bwd_colsum(dZ, Y, ctx.relu, need_b,
                                 row_div=plan.in_cnt if (mean and (need_h or need_w)) else None)
        dH = dw = None
        if need_h:
            dH = spmm_bwd(plan.bwd, norm.w_bwd, norm.row_scale_bwd, dY,
                          L.REDUCE_SUM if mean else ctx.reduce, win_mask=mask,
                          slot_map=plan.slot_map() if mask is not None else None)
        if need_w:
            dw = edge_weight_grad(plan.fwd, H, dY, win_mask=mask)
        return dH, dw, db, None, None, None, None


def aggregate_plan(H: torch.Tensor, plan: GraphPlan, norm: NormPlan, aggr: str = "add",
                   bias: torch.Tensor | None = None, relu: bool = False) -> torch.Tensor:
    """:func:`aggregate` on an already-built plan (no cache lookup).  A
    bfloat16 ``H`` takes the bf16 kernels (:class:`_AggregateBf16`: bf16 in
    and out, fp32 weights, bias and accumulators); a shape they do not take
    (F % 8 != 0) or a differentiable norm goes through the fp32 path on the
    upcast rows and is rounded once -- the same bits by the kernels' contract."""
    if _feature_dtype(H, "H"):
        if H.dim() == 2 and spmm_bf16_supported(H.size(1)) and not norm.grad:
            return _AggregateBf16.apply(H, bias, plan, norm, L.REDUCE_CODES[aggr], bool(relu))
        return aggregate_plan(H.float(), plan, norm, aggr, bias, relu).to(torch.bfloat16)
    if norm.grad:
        return _AggregateW.apply(H, norm.w_fwd, bias, plan, norm, L.REDUCE_CODES[aggr],
                                 bool(relu))
    return _Aggregate.apply(H, bias, plan, norm, L.REDUCE_CODES[aggr], bool(relu))


class _LayerXW(torch.autograd.Function):
    """One GCN layer  y = epi((A_norm x) W + b)  on the fused kernels: the
    forward is one mgcn_spmm_xw_fwd launch, the backward one relu_bwd_colsum
    (this layer's ReLU / bias gradient; mean's division) and one
    mgcn_spmm_xw_bwd (dW and dx from on-chip dH).  Same gradients as
    linear() + aggregate_plan() up to the association of the forward sums."""

    @staticmethod
    def forward(ctx, x, W, bias, plan: GraphPlan, norm: NormPlan, reduce: int, relu: bool):
        # Z = the aggregate before W: dW = Z^T dY needs no second gather
        want_z = bool(ctx.needs_input_grad[1]) and dw_pass_supported(W.size(0), W.size(1))
        Y = spmm_xw_fwd(plan.fwd, norm.w_fwd, x, W, reduce, bias, relu, want_z=want_z)
        Y, Z = Y if want_z else (Y, None)
        ctx.plan, ctx.norm, ctx.reduce, ctx.relu = plan, norm, reduce, relu
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x, W, Y if relu else None, Z)
        return Y

    @staticmethod
    def backward(ctx, dZ):
        x, W, Y, Z = ctx.saved_tensors
        plan, norm = ctx.plan, ctx.norm
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        mean = ctx.reduce == L.REDUCE_MEAN
        if Z is None:
            dY, db = relu_bwd_colsum(dZ.contiguous(), Y, ctx.relu, need_b,
                                     row_div=plan.in_cnt if mean else None)
            if not xw_full_supported(W.size(0), W.size(1)):  # 256: W needs no grad here
                dx = None
                if ctx.needs_input_grad[0]:
                    dx = spmm_xw_bwd(plan.bwd, norm.w_bwd, norm.row_scale_bwd, dY, None, W)[1]
                return dx, None, db, None, None, None, None
            dW, dx, _ = spmm_xw_bwd(plan.bwd, norm.w_bwd, norm.row_scale_bwd, dY, x, W,
                                    want_dx=ctx.needs_input_grad[0])
            return dx, dW, db, None, None, None, None
        # reassociated: dW = Z^T dY (mean: undivided Z, dY / count) on the
        # dense dW pass, the gather only for dx
        hcs = need_b and not ctx.relu and not mean  # db from the dW pass
        if hcs:
            dY, db = dZ.contiguous(), None
        else:
            dY, db = relu_bwd_colsum(dZ.contiguous(), Y, ctx.relu, need_b,
                                     row_div=plan.in_cnt if mean else None)
        dW, cs = dw_pass(Z, dY, W, dh_colsum=hcs)
        if hcs:
            db = cs
        dx = None
        if ctx.needs_input_grad[0]:
            dx = spmm_xw_bwd(plan.bwd, norm.w_bwd, norm.row_scale_bwd, dY, None, W)[1]
        return dx, dW, db, None, None, None, None


def gcn_layer(x: torch.Tensor, W: torch.Tensor, plan: GraphPlan, norm: NormPlan,
              aggr: str = "add", bias: torch.Tensor | None = None,
              relu: bool = False, aggregate_first: bool = False) -> torch.Tensor:
    """``aggregate_plan(x @ W, plan, norm, aggr, bias, relu)`` -- the
    reference's ``x @ weight_node`` then gather / scale / scatter (+ bias,
    ReLU) (gcn_base_models.py:201-241) -- as one fused launch per direction
    where the kernels apply (128 -> 128, sum / mean, no heavy rows in either
    view, gathered tables within 4 GiB); otherwise the GEMM and the
    aggregation run as separate launches, in the order the caller's
    reference uses: ``aggregate_first`` (PyG SAGEConv: mean_j x_j, then
    @ W + b) or x @ W first (the default).  A bfloat16 ``x`` takes the two
    launches unless :func:`set_bf16_fused_layers` is on and
    :func:`layer_fusable_bf16` holds: then one mgcn_spmm_xw_bf16 launch per
    direction (:class:`_LayerXWBf16`)."""
    reduce = L.REDUCE_CODES[aggr]
    if x.dtype == torch.bfloat16 and W.dtype != x.dtype:
        # fp32 master weights under bf16 activations: the cast is an autograd
        # node, so W receives an fp32 gradient; the bias stays fp32 into the
        # aggregation's epilogue
        W = W.to(x.dtype)
    if _FUSE_XW and not norm.grad and layer_fusable(plan, x, W, reduce):
        return _LayerXW.apply(x, W, bias, plan, norm, reduce, bool(relu))
    if _BF16_FUSED and not norm.grad and layer_fusable_bf16(plan, x, W, reduce):
        return _LayerXWBf16.apply(x, W, bias, plan, norm, reduce, bool(relu))
    if aggregate_first:
        out = linear(aggregate_plan(x, plan, norm, aggr), W)
        if bias is not None:
            out = out + bias.to(out.dtype)
        return torch.relu(out) if relu else out
    return aggregate_plan(linear(x, W), plan, norm, aggr, bias, relu)


class _Bwd(enum.Enum):
    """The backward route of one layer of a GCN stack (:func:`_plan_stack`)."""
    NONE = "none"                # frozen weight at the bottom, x without gradient
    DX_ONLY = "dx_only"          # frozen weight: the dX-only adjoint
    Z_FORM = "z_form"            # dense dW = Z^T dY pass + the dX-only adjoint
    FULL = "full"                # the one-pass dW + dX adjoint
    FULL_DW = "full_dw"          # its dW-only form (bottom layer, x without gradient)
    GEMM_BWD = "gemm_bwd"        # spmm_bwd, then dW + dX from one gemm_bwd
    GEMM_BWD_DW = "gemm_bwd_dw"  # spmm_bwd, then gemm_bwd's dW-only form
    GENERIC = "generic"          # spmm_bwd, then gemm_tn and a dX product


class _TopBias(enum.Enum):
    """Where a GCN stack's top-layer bias gradient (dZ's column sums) comes from."""
    COLSUM_PASS = "colsum_pass"      # relu_bwd_colsum over dZ (also the top ReLU / mean)
    TOP_DW_PASS = "top_dw_pass"      # the top layer's own Z^T dY pass
    ADJOINT = "adjoint"              # the top layer's dW + dX adjoint launch
    BOTTOM_DW_PASS = "bottom_dw_pass"  # the bottom layer's Z^T dY pass (dw_pass_cs)


@dataclass(frozen=True)
class _LayerPlan:
    fused_fwd: bool    # spmm_xw_fwd; otherwise the GEMM, then spmm_fwd
    write_mask: bool   # the forward writes the ReLU mask the layer above reads
    keep_z: bool       # the forward keeps the aggregate Z = A h (bwd is Z_FORM)
    winner_bits: bool  # max on spmm_fwd: the adjoint routes dY through the winners
    bwd: _Bwd
    epilogue: bool     # the lower layer's ReLU / bias gradient / mean divisor ride in this dX
    want_dw: bool
    want_dx: bool      # every layer but the bottom one; there: x needs a gradient


@dataclass(frozen=True)
class _StackPlan:
    layers: tuple
    top_bias: _TopBias


def _plan_stack(shapes, relus, has_bias, need_w, need_x: bool, reduce: int, fwd: CSRView,
                bwd: CSRView, ld_x: int) -> _StackPlan:
    """Every launch decision of a :class:`_GCNStack`, taken once, before its
    forward: ``shapes`` the layers' (F_in, F_out), ``need_w`` which weights
    want a gradient, ``ld_x`` the leading dimension of the stack's input.  Of
    the views only n_rows, n_cols and n_heavy are read, no tensor data: the
    plan is a function of these arguments, the module switches and libmgcn's
    ``*_supported`` probes.

    Forward.  A layer the fused kernel takes (128 -> 128 or 256 -> 256, sum /
    mean, no heavy rows: :func:`spmm_xw_supported`; ``MGCN_FUSE_XW=0`` turns
    every fused kernel off) aggregates then multiplies in one launch, (A h) W,
    and h W is never written; any other runs the GEMM, then the SpMM (max does
    not commute with W), which for max leaves each edge's winner bits.  A ReLU
    layer writes its mask (16 B per row and 128 features) iff the layer above
    reads it in its dX epilogue: mgcn_gemm_nn's fused ReLU backward (N <= 128)
    or, for the 8-word masks that only a 256-wide fused forward writes, the
    dX-only adjoint.

    Backward, top layer first; each layer takes the first route that applies.
      * NONE / DX_ONLY: a frozen weight wants no dW -- nothing at the bottom of
        a stack whose x wants no gradient, otherwise the dX-only adjoint where
        it applies (no max; the lower layer's mask kept, or the bottom layer).
        A frozen weight it does not take falls through to the routes below
        and its dW is dropped.
      * Z_FORM: the forward kept Z = A h (mean: the undivided sum, dY arrives
        divided by the counts), dW = Z^T dY is one dense pass and the gather
        runs only for dX, so the bottom layer runs no gather at all.  For the
        bottom layer, or one above a kept mask, whose weight wants a gradient
        and whose adjoint the fused kernel takes; but not for a middle layer
        (Z write + dW pass + dX-only gather cost 1.18 ms there against 1.15
        for the one kernel; ``MGCN_Z_MIDDLE=1`` sends them through Z too) nor,
        by default, for a 128-wide top layer without ReLU on a square graph:
        with the adjoint at 0.99 ms it is cheaper on FULL than Z's write, the
        dX-only adjoint and the dense pass (``MGCN_TOP_FULL=0``: Z_FORM).
        256-wide layers have no FULL form and always take Z.
      * FULL: adjoint SpMM, dW and dX with the lower layer's epilogue in one
        pass, dH never leaves the chip; 128 x 128 above a kept mask.  Max
        routes dY through the forward's winner bits in the same launch (the
        warp-specialised kernel; ``MGCN_MAX_FULL=0``: spmm_bwd + gemm_bwd).
        FULL_DW is its dW-only form at a bottom layer whose x wants no gradient.
      * GEMM_BWD / GEMM_BWD_DW / GENERIC: spmm_bwd writes dH; then one
        gemm_bwd for dW and dX (128 x 128 above a kept mask), its dW-only form
        (bottom, x without gradient), or gemm_tn for dW and, for dX,
        gemm_nn with the mask epilogue / a plain product and relu_bwd_colsum.

    The top layer's bias gradient is the column sums of dZ.  Without a top
    ReLU or mean they come free from the top layer's own Z^T dY pass
    (TOP_DW_PASS); with the top layer on FULL from the bottom layer's Z^T dY
    pass, which streams dZ beside its own operands (BOTTOM_DW_PASS,
    mgcn_gemm_bwd_dw_cs: 0.245 vs 0.224 ms for the plain pass, config 2
    4.89-4.90 vs 4.95-4.96 ms/step; ``MGCN_TOP_CS_DEFER=0`` turns it off) or,
    ``MGCN_TOP_HCS=1``, from the FULL launch itself (ADJOINT,
    mgcn_spmm_xw_bwd_hcs: its dY row reads and their registers cost that
    launch ~0.25 ms, 5.16-5.19).  Otherwise a relu_bwd_colsum pass over dZ
    (COLSUM_PASS, 0.095 ms), which also applies the top ReLU and mean's
    division."""
    fuse, z_middle, top_full, top_hcs, cs_defer, max_full = (
        _FUSE_XW, _Z_MIDDLE, _TOP_FULL, _TOP_HCS, _TOP_CS_DEFER, _MAX_FULL)
    top = len(shapes) - 1
    mean = reduce == L.REDUCE_MEAN
    square = bwd.n_rows == bwd.n_cols

    def adjoint_ok(l):  # the fused adjoint gathers layer l's dY over the bwd view
        return spmm_xw_supported(bwd, shapes[l][1], shapes[l][0], L.REDUCE_SUM)

    layers = []
    for l, (f_in, f_out) in enumerate(shapes):
        xw = bool(fuse and spmm_xw_supported(fwd, f_in, f_out, reduce, ld_x if l == 0 else None))
        mask = bool(relus[l] and l < top and (
            gemm_nn_epi_supported(shapes[l + 1][1], shapes[l + 1][0]) or
            (xw and f_out > 128 and adjoint_ok(l + 1))))
        epilogue = l > 0 and layers[l - 1].write_mask
        winners = reduce == L.REDUCE_MAX and not xw
        want_dw, want_dx = bool(need_w[l]), l > 0 or bool(need_x)
        full_ok = fuse and xw_full_supported(f_in, f_out) and adjoint_ok(l)
        middle = 0 < l < top and relus[l - 1]
        on_full = (top_full and l == top and epilogue and not relus[l] and
                   reduce in (L.REDUCE_SUM, L.REDUCE_MEAN) and square and
                   xw_full_supported(f_in, f_out))
        keep_z = bool(xw and want_dw and (l == 0 or epilogue) and not on_full and
                      (z_middle or not middle or not xw_full_supported(f_in, f_out)) and
                      dw_pass_supported(f_in, f_out) and adjoint_ok(l))
        if not want_dw and not want_dx:
            route = _Bwd.NONE
        elif not want_dw and not winners and (l == 0 or epilogue) and fuse and adjoint_ok(l):
            route = _Bwd.DX_ONLY
        elif keep_z:
            route = _Bwd.Z_FORM
        elif full_ok and epilogue and (not winners or max_full):
            route = _Bwd.FULL
        elif full_ok and not want_dx:
            route = _Bwd.FULL_DW
        elif epilogue and gemm_bwd_supported(f_in, f_out):
            route = _Bwd.GEMM_BWD
        elif not want_dx and gemm_bwd_supported(f_in, f_out):
            route = _Bwd.GEMM_BWD_DW
        else:
            route = _Bwd.GENERIC
        layers.append(_LayerPlan(xw, mask, keep_z, winners, route, epilogue, want_dw, want_dx))

    plain_top = not relus[top] and not mean  # dY = dZ as it is
    if plain_top and layers[top].keep_z:
        top_bias = _TopBias.TOP_DW_PASS
    elif (plain_top and top_full and top_hcs and layers[top].bwd is _Bwd.FULL and
          not layers[top].winner_bits and has_bias[top] and square):
        top_bias = _TopBias.ADJOINT
    elif (plain_top and cs_defer and top > 0 and has_bias[top] and layers[0].keep_z and
          gemm_bwd_supported(*shapes[0]) and shapes[top][1] == 128):
        top_bias = _TopBias.BOTTOM_DW_PASS
    else:
        top_bias = _TopBias.COLSUM_PASS
    return _StackPlan(tuple(layers), top_bias)


class _GCNStack(torch.autograd.Function):
    """A chain of GCN layers  Z_l = act_l(A_norm (Z_{l-1} W_l) + b_l)  as one
    autograd node, so the backward can fuse across layer boundaries: the ReLU
    mask and bias gradient of layer l-1 are computed in the epilogue of layer
    l's dX, instead of a separate pass.  :func:`_plan_stack` chooses every
    launch of both directions before the forward runs; the forward executes
    its half and leaves the plan on ``ctx`` for the backward.  Same math and
    the same per-edge summation order as the layer-by-layer modules."""

    @staticmethod
    def forward(ctx, x, plan, norm, reduce, relus, *params):
        Ws, bs = params[0::2], params[1::2]
        n = len(Ws)
        has_bias = [b is not None for b in bs]
        route = _plan_stack([tuple(W.shape) for W in Ws], relus, has_bias,
                            [ctx.needs_input_grad[5 + 2 * i] for i in range(n)],
                            ctx.needs_input_grad[0], reduce, plan.fwd, plan.bwd, x.stride(0))
        h = x
        inputs, outs, args, rmasks, zs = [], [], [], [], []
        for W, b, relu, lp in zip(Ws, bs, relus, route.layers):
            inputs.append(h)
            z = am = rm = None
            if lp.write_mask:
                rm = torch.empty(plan.fwd.n_rows, mask_words(W.size(1)), dtype=torch.int32,
                                 device=h.device)
            if lp.fused_fwd:
                h = spmm_xw_fwd(plan.fwd, norm.w_fwd, h, W, reduce, b, relu, relu_mask=rm,
                                want_z=lp.keep_z)
                if lp.keep_z:
                    h, z = h
            else:
                h, am = spmm_fwd(plan.fwd, norm.w_fwd, _mm(h, W), reduce, b, relu, mask_plan=plan,
                                 relu_mask=rm)
            outs.append(h)
            args.append(am)  # max: winner bits per edge (adjoint slot order)
            rmasks.append(rm)
            zs.append(z)
        ctx.plan, ctx.norm, ctx.reduce, ctx.relus = plan, norm, reduce, relus
        ctx.n_layers, ctx.has_bias, ctx.route = n, has_bias, route
        ctx.save_for_backward(*inputs, *outs, *[a if a is not None else torch.empty(0)
                                                for a in args], *Ws,
                              *[m if m is not None else torch.empty(0) for m in rmasks],
                              *[z if z is not None else torch.empty(0) for z in zs])
        return h

    @staticmethod
    def backward(ctx, dZ):
        n = ctx.n_layers
        saved = ctx.saved_tensors
        inputs, outs = saved[:n], saved[n:2 * n]
        args, Ws, rmasks = saved[2 * n:3 * n], saved[3 * n:4 * n], saved[4 * n:5 * n]
        zs = saved[5 * n:6 * n]
        plan, norm, reduce, relus = ctx.plan, ctx.norm, ctx.reduce, ctx.relus
        has_bias, top_bias = ctx.has_bias, ctx.route.top_bias
        view, w_t, scale = plan.bwd, norm.w_bwd, norm.row_scale_bwd
        gW = [None] * n
        gb = [None] * n
        top = n - 1
        # mean: every layer's dY is produced divided by the row counts (fused
        # into relu_bwd_colsum / the dX epilogue); the adjoint is a sum
        mean = reduce == L.REDUCE_MEAN
        rd = plan.in_cnt if mean else None
        adj = L.REDUCE_SUM if mean else reduce
        dZ = dZ.contiguous()
        if top_bias is _TopBias.COLSUM_PASS:
            dY, gb[top] = relu_bwd_colsum(dZ, outs[top], relus[top], has_bias[top], row_div=rd)
        else:
            dY = dZ  # its column sums come from a later launch, no separate read of dZ

        def lower_bias(l, db):
            gb[l - 1] = db if has_bias[l - 1] else None

        def gather_dx(l, dY, lp):
            """Layer l's dX-only adjoint: the lower layer's dY (through its ReLU
            mask and mean divisor, with its bias gradient), or the stack's dx."""
            if lp.epilogue:
                _, dY, db = spmm_xw_bwd(view, w_t, scale, dY, None, Ws[l], relu_mask=rmasks[l - 1],
                                        row_div=rd)
                lower_bias(l, db)
                return dY
            if lp.want_dx:
                return spmm_xw_bwd(view, w_t, scale, dY, None, Ws[l])[1]
            return None

        # dY: the gradient of layer l's output on entry, of its input on exit
        for l in range(top, -1, -1):
            lp, W = ctx.route.layers[l], Ws[l]
            if lp.bwd is _Bwd.NONE:
                dY = None
                continue
            am = args[l] if lp.winner_bits else None
            sm = plan.slot_map() if lp.winner_bits else None
            if lp.bwd is _Bwd.DX_ONLY:
                dY = gather_dx(l, dY, lp)
            elif lp.bwd is _Bwd.Z_FORM:
                if l == 0 and top_bias is _TopBias.BOTTOM_DW_PASS:
                    gW[l], gb[top] = dw_pass_cs(zs[l], dY, dZ)
                else:
                    hcs = l == top and top_bias is _TopBias.TOP_DW_PASS and has_bias[top]
                    gW[l], cs = dw_pass(zs[l], dY, W, dh_colsum=hcs)
                    if hcs:
                        gb[top] = cs
                dY = gather_dx(l, dY, lp)
            elif lp.bwd is _Bwd.FULL:
                hcs = None
                if l == top and top_bias is _TopBias.ADJOINT:
                    hcs = gb[top] = torch.empty(W.size(1), dtype=torch.float32, device=dY.device)
                gW[l], dY, db = spmm_xw_bwd(view, w_t, scale, dY, inputs[l], W,
                                            relu_mask=rmasks[l - 1], row_div=rd, win_mask=am,
                                            slot_map=sm, dy_colsum_out=hcs)
                lower_bias(l, db)
            elif lp.bwd is _Bwd.FULL_DW:
                gW[l] = spmm_xw_bwd(view, w_t, scale, dY, inputs[l], W, want_dx=False,
                                    win_mask=am, slot_map=sm)[0]
                dY = None
            else:
                dH = spmm_bwd(view, w_t, scale, dY, adj, win_mask=am, slot_map=sm)
                dY = None
                if lp.bwd is _Bwd.GEMM_BWD:
                    gW[l], dY, db = gemm_bwd(inputs[l], dH, W, relu_mask=rmasks[l - 1], row_div=rd)
                    lower_bias(l, db)
                elif lp.bwd is _Bwd.GEMM_BWD_DW:
                    gW[l] = gemm_bwd(inputs[l], dH, W, want_dx=False)[0]
                else:
                    if lp.want_dw:
                        gW[l] = gemm_tn(inputs[l], dH)
                    if lp.epilogue:
                        dY, db = gemm_nn(dH, W, transpose_w=True, relu_mask=rmasks[l - 1],
                                         row_div=rd)
                        lower_bias(l, db)
                    elif l > 0:
                        dY, gb[l - 1] = relu_bwd_colsum(_mm_t(dH, W), outs[l - 1], relus[l - 1],
                                                        has_bias[l - 1], row_div=rd)
                    elif lp.want_dx:
                        dY = _mm_t(dH, W)
        grads = []
        for w, b in zip(gW, gb):
            grads += [w, b]
        return (dY, None, None, None, None, *grads)


def gcn_stack(x: torch.Tensor, plan: GraphPlan, norm: NormPlan, Ws, bs, relus,
              aggr: str = "add") -> torch.Tensor:
    """Run len(Ws) fused GCN layers (see :class:`_GCNStack`)."""
    if norm.grad:  # weights with autograd history: layer by layer (_AggregateW)
        for W, b, r in zip(Ws, bs, relus):
            x = aggregate_plan(linear(x, W), plan, norm, aggr, b, bool(r))
        return x
    params = []
    for W, b in zip(Ws, bs):
        params += [W, b]
    return _GCNStack.apply(x, plan, norm, L.REDUCE_CODES[aggr], tuple(bool(r) for r in relus),
                           *params)


# ------------------------------------------------------- residual GCN layer
def residual_act(Z1: torch.Tensor, R: torch.Tensor, rbias: torch.Tensor | None,
                 relu: bool) -> torch.Tensor:
    """Z = act(Z1 + (R + rbias)) (``mgcn_residual_act``)."""
    lib = L.load()
    dev = L.require_device(Z1, R, rbias)
    n, F = Z1.shape
    Z = torch.empty(n, F, dtype=torch.float32, device=dev)
    rb = rbias.detach().contiguous() if rbias is not None else None
    launch(None, "mgcn_residual_act", dev, None, None, lib.mgcn_residual_act,
           n, F, L.ptr(Z1), Z1.stride(0), L.ptr(R), R.stride(0), L.ptr(rb), int(bool(relu)),
           L.ptr(Z), Z.stride(0), L.stream_of(dev))
    return Z


def residual_act_bwd(dZ, Z, relu, Z1, relu1, dA, dS, row_div=None, want_sums=True):
    """dS / dA / their column sums (``mgcn_residual_act_bwd``); returns the
    [2F] sums (dA | dS) or None."""
    lib = L.load()
    dev = L.require_device(dZ, dA)
    n, F = dZ.shape
    sums = torch.empty(2 * F, dtype=torch.float32, device=dev) if want_sums else None
    ws, ws_bytes = (workspace(lib.mgcn_residual_act_bwd_workspace_bytes(n, F), dev)
                    if want_sums else (None, 0))
    launch(None, "mgcn_residual_act_bwd", dev, None, None, lib.mgcn_residual_act_bwd,
           n, F, L.ptr(dZ), dZ.stride(0), L.ptr(Z), Z.stride(0) if Z is not None else F,
           int(bool(relu)), L.ptr(Z1), Z1.stride(0) if Z1 is not None else F, int(bool(relu1)),
           L.ptr(row_div), L.ptr(dA), dA.stride(0), L.ptr(dS),
           dS.stride(0) if dS is not None else F, L.ptr(sums), L.ptr(ws), ws_bytes,
           L.stream_of(dev))
    return sums


class _ResidualGCNLayer(torch.autograd.Function):
    """One GCNModel layer with its residual Linear (gcn_model.py:92-105,
    residual_hop = 1) as a single autograd node:

        [H | R] = x @ [W | Wr^T]                 one GEMM, x read once
        Z1 = relu1(A_norm H + b)                 SpMM, bias/ReLU epilogue
        Z  = relu2(Z1 + (R + br))                mgcn_residual_act

    backward: mgcn_residual_act_bwd gives dA (into the adjoint SpMM), dS and
    both bias gradients in one pass; the adjoint SpMM writes dH beside dS,
    so dx = [dH | dS] @ [W | Wr^T]^T and [dW | dWr^T] = x^T [dH | dS] are one
    GEMM each.  Forward values are the layer-by-layer path's bit for bit;
    gradients agree within fp32 GEMM tolerance (different summation order)."""

    @staticmethod
    def forward(ctx, x, plan, norm, reduce, relu1, relu2, W, b, Wr, br):
        F_out = W.size(1)
        Wc = torch.cat([W.detach(), Wr.detach().t()], dim=1)
        HR = _mm(x, Wc)
        Z1, mask = spmm_fwd(plan.fwd, norm.w_fwd, HR[:, :F_out], reduce, b, relu1, mask_plan=plan)
        Z = residual_act(Z1, HR[:, F_out:], br, relu2)
        ctx.plan, ctx.norm, ctx.reduce, ctx.relu1, ctx.relu2 = plan, norm, reduce, relu1, relu2
        ctx.has_b, ctx.has_br = b is not None, br is not None
        ctx.save_for_backward(x, Z1, Z, Wc, mask)
        return Z

    @staticmethod
    def backward(ctx, dZ):
        x, Z1, Z, Wc, mask = ctx.saved_tensors
        plan, norm = ctx.plan, ctx.norm
        n, F_out = Z.shape
        dZ = dZ.contiguous()
        mean = ctx.reduce == L.REDUCE_MEAN
        DH = torch.empty(n, 2 * F_out, dtype=torch.float32, device=dZ.device)
        dA = torch.empty(n, F_out, dtype=torch.float32, device=dZ.device)
        sums = residual_act_bwd(dZ, Z, ctx.relu2, Z1, ctx.relu1, dA, DH[:, F_out:],
                                row_div=plan.in_cnt if mean else None)
        spmm_bwd(plan.bwd, norm.w_bwd, norm.row_scale_bwd, dA,
                 L.REDUCE_SUM if mean else ctx.reduce, out=DH[:, :F_out], win_mask=mask,
                 slot_map=plan.slot_map() if mask is not None else None)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = _mm_t(DH, Wc)
        # [dW | dWr^T] = x^T [dH | dS] in one pass, dWr written transposed
        dW, dWr = gemm_tn_split(x, DH, F_out)
        db = sums[:F_out] if ctx.has_b else None
        dbr = sums[F_out:] if ctx.has_br else None
        return (dx, None, None, None, None, None, dW, db, dWr, dbr)


def residual_layer_supported(plan: GraphPlan, x: torch.Tensor, W: torch.Tensor, Wr: torch.Tensor,
                             reduce: int) -> bool:
    """True when :class:`_ResidualLayerFused` takes this layer: 32 -> 32 with a
    32 -> 32 residual Linear, sum or mean, fp32, on a square graph plan."""
    return (_FUSE_XW and x.dim() == 2 and x.dtype == torch.float32 and x.is_cuda and
            W.dtype == torch.float32 and Wr.dtype == torch.float32 and
            tuple(W.shape) == (x.size(1), x.size(1)) and tuple(Wr.shape) == tuple(W.shape) and
            x.size(0) == plan.fwd.n_rows == plan.fwd.n_cols and
            bool(L.load().mgcn_residual_layer_supported(x.size(1), W.size(1), int(reduce))))


class _ResidualLayerFused(torch.autograd.Function):
    """One GCNModel layer with its residual Linear (gcn_model.py:89-105,
    residual_hop = 1), F = 32, on libmgcn's fused residual-layer kernels
    (residual.hip): the forward is one pass over the rows (aggregation of x,
    both 32 x 32 products, bias, ReLU, join, ReLU; ReLU masks kept instead of
    the activations), the backward one mask pass + one pass that gathers the
    adjoint and forms dX = dH W^T + dS Wr, then [dW | dWr^T] = x^T [dH | dS]
    as one GEMM.  (A x) W instead of A (x W): the same layer to fp32
    rounding; the adjoint dH is the SpMM's bit for bit."""

    @staticmethod
    def forward(ctx, x, plan, norm, reduce, relu1, relu2, W, b, Wr, br):
        lib = L.load()
        x = _aligned_rows(x)
        dev = L.require_device(x, W, Wr, b, br)
        n, F = x.shape
        Wd = W.detach().to(torch.float32).contiguous()
        Wrd = Wr.detach().to(torch.float32).contiguous()
        bd = None if b is None else b.detach().to(torch.float32).contiguous()
        brd = None if br is None else br.detach().to(torch.float32).contiguous()
        Z = torch.empty(n, F, dtype=torch.float32, device=dev)
        masks = torch.empty(n, 2, dtype=torch.int32, device=dev)
        v = plan.fwd
        launch("residual_layer_fwd", "mgcn_residual_layer_fwd", dev, v.n_rows, v.edges,
               lib.mgcn_residual_layer_fwd,
               n, F, L.ptr(v.rowptr), L.ptr(v.col), L.ptr(v.eid), L.ptr(norm.w_fwd), L.ptr(x),
               x.stride(0), L.ptr(Wd), F, L.ptr(bd), L.ptr(Wrd), F, L.ptr(brd), int(reduce),
               int(bool(relu1)), int(bool(relu2)), L.ptr(Z), F, L.ptr(masks), L.ptr(v.order),
               v.n_heavy, v.n_giant, L.stream_of(dev))
        ctx.plan, ctx.norm, ctx.reduce, ctx.relu1, ctx.relu2 = plan, norm, reduce, relu1, relu2
        ctx.has_b, ctx.has_br = b is not None, br is not None
        ctx.save_for_backward(x, Wd, Wrd, masks)
        return Z

    @staticmethod
    def backward(ctx, dZ):
        lib = L.load()
        x, Wd, Wrd, masks = ctx.saved_tensors
        plan, norm = ctx.plan, ctx.norm
        dZ = _aligned_rows(dZ)
        dev = dZ.device
        n, F = x.shape
        dX = torch.empty(n, F, dtype=torch.float32, device=dev)
        DH = torch.empty(n, 2 * F, dtype=torch.float32, device=dev)
        sums = torch.empty(2 * F, dtype=torch.float32, device=dev)
        ws, ws_bytes = workspace(lib.mgcn_residual_layer_bwd_workspace_bytes(n, F), dev)
        v = plan.bwd
        rd = plan.in_cnt if ctx.reduce == L.REDUCE_MEAN else None
        launch("residual_layer_bwd", "mgcn_residual_layer_bwd", dev, v.n_rows, v.edges,
               lib.mgcn_residual_layer_bwd,
               n, F, L.ptr(v.rowptr), L.ptr(v.col), L.ptr(v.eid), L.ptr(norm.w_bwd),
               L.ptr(norm.row_scale_bwd), L.ptr(rd), L.ptr(dZ), dZ.stride(0), L.ptr(masks),
               int(bool(ctx.relu1)), int(bool(ctx.relu2)), L.ptr(Wd), F, L.ptr(Wrd), F, L.ptr(dX),
               F, L.ptr(DH), 2 * F, L.ptr(sums), L.ptr(v.order), v.n_heavy, v.n_giant, L.ptr(ws),
               ws_bytes, L.stream_of(dev))
        # [dW | dWr^T] = x^T [dH | dS] in one pass, dWr written transposed
        dW, dWr = gemm_tn_split(x, DH, F)
        db = sums[:F] if ctx.has_b else None
        dbr = sums[F:] if ctx.has_br else None
        dx = dX if ctx.needs_input_grad[0] else None
        return (dx, None, None, None, None, None, dW, db, dWr, dbr)


def _ptr_array(ts):
    """Host array of device pointers (NULL for None) for the stack entry points."""
    import ctypes
    arr = (ctypes.c_void_p * max(len(ts), 1))(*[None if t is None else t.data_ptr() for t in ts])
    return ctypes.cast(arr, ctypes.c_void_p), arr


def _int_array(vals):
    import ctypes
    arr = (ctypes.c_int32 * max(len(vals), 1))(*[int(bool(v)) for v in vals])
    return ctypes.cast(arr, ctypes.c_void_p), arr


def _param_f32(t):
    if t is None:
        return None
    t = t.detach()
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.to(torch.float32).contiguous()


class _ResidualStack(torch.autograd.Function):
    """Consecutive 32 -> 32 GCNModel layers with their residual Linears
    (:class:`_ResidualLayerFused` each) as ONE autograd node and one host call
    per direction (``mgcn_residual_stack_fwd`` / ``_bwd``): bitwise the
    layer-by-layer fused path, without ~40 us of Python and ctypes work per
    layer and direction (the 12-layer config-3 step was bound by host issue).
    params = (W, b, Wr, br) per layer."""

    @staticmethod
    def forward(ctx, x0, plan, norm, reduce, relu1s, relu2s, *params):
        lib = L.load()
        nl = len(relu1s)
        x0 = _aligned_rows(x0)
        dev = x0.device
        n, F = x0.shape
        Ws = [_param_f32(p) for p in params[0::4]]
        bs = [_param_f32(p) for p in params[1::4]]
        Wrs = [_param_f32(p) for p in params[2::4]]
        brs = [_param_f32(p) for p in params[3::4]]
        Z = torch.empty(nl, n, F, dtype=torch.float32, device=dev)
        masks = torch.empty(nl, n, 2, dtype=torch.int32, device=dev)
        pw, aw = _ptr_array(Ws)
        pb, ab = _ptr_array(bs)
        pwr, awr = _ptr_array(Wrs)
        pbr, abr = _ptr_array(brs)
        pr1, ar1 = _int_array(relu1s)
        pr2, ar2 = _int_array(relu2s)
        v = plan.fwd
        launch("residual_stack_fwd", "mgcn_residual_stack_fwd", dev, v.n_rows, v.edges,
               lib.mgcn_residual_stack_fwd,
               n, F, nl, L.ptr(v.rowptr), L.ptr(v.col), L.ptr(v.eid), L.ptr(norm.w_fwd), L.ptr(x0),
               x0.stride(0), pw, pb, pwr, pbr, int(reduce), pr1, pr2, L.ptr(Z), L.ptr(masks),
               L.ptr(v.order), v.n_heavy, v.n_giant, L.stream_of(dev))
        ctx.plan, ctx.norm, ctx.reduce = plan, norm, reduce
        ctx.relu1s, ctx.relu2s = relu1s, relu2s
        ctx.has_b = [b is not None for b in bs]
        ctx.has_br = [b is not None for b in brs]
        ctx.save_for_backward(x0, Z, masks, *Ws, *Wrs)
        return Z[nl - 1]

    @staticmethod
    def backward(ctx, dZ):
        lib = L.load()
        nl = len(ctx.relu1s)
        saved = ctx.saved_tensors
        x0, Z, masks = saved[:3]
        Ws, Wrs = saved[3:3 + nl], saved[3 + nl:3 + 2 * nl]
        plan, norm = ctx.plan, ctx.norm
        dZ = _aligned_rows(dZ)
        dev = dZ.device
        n, F = x0.shape
        G = torch.empty(nl, 2, F, F, dtype=torch.float32, device=dev)  # dW[l] | dWr[l]
        sums = torch.empty(nl, 2 * F, dtype=torch.float32, device=dev)
        dX0 = torch.empty(n, F, dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] \
            else None
        ws, ws_bytes = workspace(lib.mgcn_residual_stack_bwd_workspace_bytes(n, F), dev)
        pw, aw = _ptr_array(Ws)
        pwr, awr = _ptr_array(Wrs)
        pdw, adw = _ptr_array([G[l, 0] for l in range(nl)])
        pdwr, adwr = _ptr_array([G[l, 1] for l in range(nl)])
        pr1, ar1 = _int_array(ctx.relu1s)
        pr2, ar2 = _int_array(ctx.relu2s)
        v = plan.bwd
        rd = plan.in_cnt if ctx.reduce == L.REDUCE_MEAN else None
        launch("residual_stack_bwd", "mgcn_residual_stack_bwd", dev, v.n_rows, v.edges,
               lib.mgcn_residual_stack_bwd,
               n, F, nl, L.ptr(v.rowptr), L.ptr(v.col), L.ptr(v.eid), L.ptr(norm.w_bwd),
               L.ptr(norm.row_scale_bwd), L.ptr(rd), L.ptr(dZ), dZ.stride(0), L.ptr(x0),
               x0.stride(0), L.ptr(Z), L.ptr(masks), pr1, pr2, pw, pwr, L.ptr(dX0), pdw, pdwr,
               L.ptr(sums), L.ptr(v.order), v.n_heavy, v.n_giant, L.ptr(ws), ws_bytes,
               L.stream_of(dev))
        grads = []
        for l in range(nl):
            grads += [G[l, 0], sums[l, :F] if ctx.has_b[l] else None, G[l, 1],
                      sums[l, F:] if ctx.has_br[l] else None]
        return (dX0, None, None, None, None, None, *grads)


def residual_stack(x, plan: GraphPlan, norm: NormPlan, aggr: str, relu1s, relu2s, params):
    """Layers of :class:`_ResidualStack`; params = [(W, b, Wr, br), ...]."""
    flat = []
    for p in params:
        flat += list(p)
    return _ResidualStack.apply(x, plan, norm, L.REDUCE_CODES[aggr],
                                tuple(bool(r) for r in relu1s), tuple(bool(r) for r in relu2s),
                                *flat)


def input_layer_supported(plan: GraphPlan, x: torch.Tensor, W: torch.Tensor, Wr: torch.Tensor,
                          reduce: int) -> bool:
    """True when :class:`_InputLayer` takes this layer: in_channels = 1 with a
    1 -> F residual Linear, sum or mean, fp32, on a square graph plan."""
    return (_FUSE_XW and x.dim() == 2 and x.size(1) == 1 and x.dtype == torch.float32 and
            x.is_cuda and W.dtype == torch.float32 and Wr.dtype == torch.float32 and
            W.dim() == 2 and W.size(0) == 1 and tuple(Wr.shape) == (W.size(1), 1) and
            reduce in (L.REDUCE_SUM, L.REDUCE_MEAN) and
            x.size(0) == plan.fwd.n_rows == plan.fwd.n_cols and
            bool(L.load().mgcn_input_layer_supported(1, W.size(1))))


class _InputLayer(torch.autograd.Function):
    """GCNModel's input layer with its residual Linear when in_channels = 1
    (config 3's botnet node feature; gcn_model.py:89-105, residual_hop = 1),
    associated as (A x) W: a = A x is a 1-wide aggregation (mgcn_spmm_fwd,
    4 gathered bytes per edge instead of 4 F) and everything after it is
    elementwise (mgcn_input_layer_fwd):

        Z = relu2( relu1(a W + b) + (x Wr^T + br) )

    backward: one pass over dZ (mgcn_input_layer_bwd) gives dW, db, dWr, dbr
    as fixed-order column sums -- no adjoint gather at all unless x itself
    needs a gradient (then dx = A^T (dA W^T) + dS Wr, a 1-wide adjoint SpMM).
    The reference's A (x W) to fp32 rounding (a different association)."""

    @staticmethod
    def forward(ctx, x, plan, norm, reduce, relu1, relu2, W, b, Wr, br):
        lib = L.load()
        dev = L.require_device(x, W, b, Wr, br)
        x = x.contiguous()
        n, F = x.size(0), W.size(1)
        a, _ = spmm_fwd(plan.fwd, norm.w_fwd, x, reduce)
        Wd, Wrd = W.detach().contiguous(), Wr.detach().contiguous()
        bd = b.detach().contiguous() if b is not None else None
        brd = br.detach().contiguous() if br is not None else None
        Z = torch.empty(n, F, dtype=torch.float32, device=dev)
        launch("input_layer_fwd", "mgcn_input_layer_fwd", dev, n, None, lib.mgcn_input_layer_fwd,
               n, F, L.ptr(a), L.ptr(x), L.ptr(Wd), L.ptr(bd), L.ptr(Wrd), L.ptr(brd), int(relu1),
               int(relu2), L.ptr(Z), Z.stride(0), L.stream_of(dev))
        ctx.plan, ctx.norm, ctx.reduce, ctx.relu1, ctx.relu2 = plan, norm, reduce, relu1, relu2
        ctx.has_b, ctx.has_br = b is not None, br is not None
        ctx.save_for_backward(x, a, Z, Wd, bd if bd is not None else torch.empty(0), Wrd)
        return Z

    @staticmethod
    def backward(ctx, dZ):
        lib = L.load()
        x, a, Z, W, b, Wr = ctx.saved_tensors
        plan, norm = ctx.plan, ctx.norm
        n, F = Z.shape
        dev = Z.device
        dZ = _aligned_rows(dZ)
        need_x = bool(ctx.needs_input_grad[0])
        da = torch.empty(n, dtype=torch.float32, device=dev) if need_x else None
        dxr = torch.empty(n, dtype=torch.float32, device=dev) if need_x else None
        grads = torch.empty(4 * F, dtype=torch.float32, device=dev)
        mean = ctx.reduce == L.REDUCE_MEAN
        ws, ws_bytes = workspace(lib.mgcn_input_layer_bwd_workspace_bytes(n, F), dev)
        launch("input_layer_bwd", "mgcn_input_layer_bwd", dev, n, None, lib.mgcn_input_layer_bwd,
               n, F, L.ptr(dZ), dZ.stride(0), L.ptr(Z), Z.stride(0), L.ptr(a), L.ptr(x), L.ptr(W),
               L.ptr(b if b.numel() else None), L.ptr(Wr), int(ctx.relu1), int(ctx.relu2),
               L.ptr(plan.in_cnt if (mean and need_x) else None), L.ptr(da), L.ptr(dxr),
               L.ptr(grads), L.ptr(ws), ws_bytes, L.stream_of(dev))
        dx = None
        if need_x:
            dx = spmm_bwd(plan.bwd, norm.w_bwd, norm.row_scale_bwd, da.view(n, 1), L.REDUCE_SUM)
            dx.add_(dxr.view(n, 1))
        dW = grads[:F].view(1, F)
        db = grads[F:2 * F] if ctx.has_b else None
        dWr = grads[2 * F:3 * F].view(F, 1)
        dbr = grads[3 * F:] if ctx.has_br else None
        return (dx, None, None, None, None, None, dW, db, dWr, dbr)


def residual_gcn_layer(x, plan: GraphPlan, norm: NormPlan, aggr: str, relu1: bool, relu2: bool,
                       W, b, Wr, br):
    """One GCNModel layer + residual join: :class:`_ResidualLayerFused` where
    it applies (32 -> 32, sum / mean), :class:`_InputLayer` for an
    in_channels = 1 input layer, else :class:`_ResidualGCNLayer`."""
    reduce = L.REDUCE_CODES[aggr]
    if input_layer_supported(plan, x, W, Wr, reduce):
        return _InputLayer.apply(x, plan, norm, reduce, bool(relu1), bool(relu2), W, b, Wr, br)
    if residual_layer_supported(plan, x, W, Wr, reduce):
        return _ResidualLayerFused.apply(x, plan, norm, reduce, bool(relu1), bool(relu2), W, b,
                                         Wr, br)
    return _ResidualGCNLayer.apply(x, plan, norm, reduce, bool(relu1), bool(relu2), W, b, Wr, br)


# ---------------------------------------------------------------- scatter_
class _SegmentReduce(torch.autograd.Function):
    """torch_scatter 1.x scatter_{add,mean,max}(src, index, 0, None, dim_size)
    on an explicit [E, F] ``src`` (common.py:37-66), as a SpMM whose k-th slot
    gathers src row eid_k; the adjoint gathers dY[index[e]] back per edge."""

    @staticmethod
    def forward(ctx, src, index, dim_size: int, reduce: int):
        dev = L.require_device(src, index)
        E = src.size(0)
        from .graph import build_view
        ids = torch.arange(E, dtype=torch.int64, device=dev)
        view = build_view(index, ids, dim_size, E)
        Y, argmax = spmm_fwd(view, None, src, reduce)
        # adjoint view: one slot per edge e, pointing at row index[e]
        view_t = CSRView(rowptr=torch.arange(E + 1, dtype=torch.int64, device=dev),
                         col=index.to(torch.int32).contiguous(),
                         eid=ids.to(torch.int32), n_rows=E, n_cols=dim_size)
        cnt = (view.rowptr[1:] - view.rowptr[:-1]).clamp_(min=1).to(torch.float32)
        ctx.view_t, ctx.reduce, ctx.cnt = view_t, reduce, cnt
        ctx.save_for_backward(argmax)
        return Y

    @staticmethod
    def backward(ctx, dY):
        (argmax,) = ctx.saved_tensors
        d_src = spmm_bwd(ctx.view_t, None, None, dY, ctx.reduce,
                         cnt=ctx.cnt if ctx.reduce == L.REDUCE_MEAN else None, argmax=argmax)
        return d_src, None, None, None


def scatter_(name: str, src: torch.Tensor, index: torch.Tensor, dim_size: int | None = None,
             out: torch.Tensor | None = None) -> torch.Tensor:
    """Drop-in for src/gcn_meta/models/common.py:37-66 ``scatter_``.

    'max' fills empty rows with -1e38 and then replaces exact fill values by 0
    (:57, :63-64); 'mean' divides by ``max(count, 1)``.  ``out`` is accepted
    for signature compatibility; like the reference's only caller (which
    passes none) it must be None.
    """
    assert name in ["add", "mean", "max"]
    if out is not None:
        raise NotImplementedError("scatter_(out=...) is not supported; the reference never uses it")
    if dim_size is None:
        dim_size = int(index.max().item()) + 1 if index.numel() else 0
    if _feature_dtype(src, "src"):
        if src.dim() == 2 and spmm_bf16_supported(src.size(1)):
            return _SegmentReduceBf16.apply(src, index, int(dim_size), L.REDUCE_CODES[name])
        # 1-D src, F % 8 != 0: the fp32 path on the upcast rows, rounded once
        return scatter_(name, src.float(), index, dim_size).to(torch.bfloat16)
    squeeze = src.dim() == 1
    x = src.unsqueeze(1) if squeeze else src
    y = _SegmentReduce.apply(x, index, int(dim_size), L.REDUCE_CODES[name])
    return y.squeeze(1) if squeeze else y
