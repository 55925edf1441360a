"""bf16 feature rows through the aggregation kernels (libmgcn
``mgcn_spmm_fwd_bf16`` / ``mgcn_spmm_bwd_bf16`` / ``mgcn_relu_bwd_colsum_bf16``):
the wrappers and the autograd functions :mod:`mgcn.ops` dispatches a
``torch.bfloat16`` input to.  Sits on :mod:`mgcn._call`; :mod:`mgcn.ops`
re-exports every name.

Contract (the bf16 rows): each bf16 element is widened to fp32
(exact), the row is formed exactly as the fp32 kernels form it -- fp32 edge
weights, bias, counts and accumulators, the same order and roundings -- and
rounded once, to nearest even, at the store.  The result is bit for bit the
fp32 path on the upcast input, rounded to bf16; so every case the kernels do
not take (``F % 8 != 0``, a differentiable norm, a 1-D ``scatter_``) goes
through upcast -> fp32 path -> round in :mod:`mgcn.ops` and gives the same
bits.

The fused bf16 layer (``mgcn_spmm_xw_bf16``, :class:`_LayerXWBf16`) lives here
too: the same aggregate, rounded to bf16 once and multiplied by a 128 x 128
bf16 matrix on one MFMA term in the same launch.  :func:`mgcn.ops.gcn_layer`
takes it only behind :func:`mgcn.ops.set_bf16_fused_layers`."""
from __future__ import annotations

from collections import Counter

import torch

from . import _lib as L
from ._call import launch, workspace
from .graph import CSRView, GraphPlan, NormPlan

BF16 = torch.bfloat16

# rows the wrappers had to copy to give the kernels 16-byte aligned rows, by
# argument name (an aligned view with ld > F is consumed in place)
ROW_COPIES: "Counter[str]" = Counter()


def spmm_bf16_supported(F: int, ld_in: int | None = None, ld_out: int | None = None) -> bool:
    """The bf16 kernels take this row shape: F % 8 == 0 and leading dimensions
    that keep rows 16-byte aligned (``mgcn_spmm_bf16_supported``)."""
    F = int(F)
    return bool(L.load().mgcn_spmm_bf16_supported(F, F if ld_in is None else int(ld_in),
                                                  F if ld_out is None else int(ld_out)))


def _rows_bf16(t: torch.Tensor, name: str) -> torch.Tensor:
    """A bf16 [N, F] tensor with unit column stride and 16-byte aligned rows:
    ``t`` itself where it already is (any ld >= F with ld % 8 == 0), else a
    contiguous copy (counted in :data:`ROW_COPIES`)."""
    if t.dtype != BF16:
        raise TypeError(f"{name} must be bfloat16, got {t.dtype}")
    if t.dim() != 2:
        raise ValueError(f"{name} must be 2-D [N, F], got {tuple(t.shape)}")
    if t.stride(1) != 1 or t.stride(0) < t.size(1) or t.stride(0) % 8 or t.data_ptr() % 16:
        ROW_COPIES[name] += 1
        t = t.contiguous()
        if t.data_ptr() % 16:  # a contiguous view at an odd storage offset
            t = t.clone()
    return t


def _bias_f32(bias, F: int):
    if bias is None:
        return None
    bias = bias.detach().to(torch.float32).contiguous()
    if bias.numel() != F:
        raise ValueError(f"bias has {bias.numel()} entries, expected {F}")
    return bias


def spmm_fwd_bf16(view: CSRView, w: torch.Tensor | None, H: torch.Tensor, reduce: int,
                  bias: torch.Tensor | None = None, relu: bool = False,
                  mask_plan: GraphPlan | None = None):
    """:func:`mgcn.ops.spmm_fwd` over bf16 rows: Y (bf16) = round(epi(reduce_k
    float(H[col_k]) * w_k)); returns (Y, argmax) -- for max with ``mask_plan``
    the winner bits in argmax's place.  F % 8 == 0."""
    lib = L.load()
    H = _rows_bf16(H, "H")
    dev = L.require_device(H, view.rowptr, w, bias)
    if H.size(0) != view.n_cols:
        raise ValueError(f"H has {H.size(0)} rows, graph has {view.n_cols} source nodes")
    F = H.size(1)
    Y = torch.empty(view.n_rows, F, dtype=BF16, device=dev)
    argmax = mask = None
    if reduce == L.REDUCE_MAX:
        if mask_plan is not None:
            mask = torch.empty(max(mask_plan.nnz, 1), (F + 31) // 32, dtype=torch.int32,
                               device=dev)
        else:
            argmax = torch.empty(view.n_rows, F, dtype=torch.int32, device=dev)
    bias = _bias_f32(bias, F)
    launch("spmm_fwd_bf16", "mgcn_spmm_fwd_bf16", dev, view.n_rows, view.edges,
           lib.mgcn_spmm_fwd_bf16,
           view.n_rows, F, L.ptr(view.rowptr), L.ptr(view.col), L.ptr(view.eid), L.ptr(w),
           L.ptr(H), H.stride(0), L.ptr(Y), Y.stride(0), reduce, L.ptr(bias), int(bool(relu)),
           L.ptr(argmax), L.ptr(mask), L.ptr(view.order), view.n_heavy, view.n_giant,
           L.stream_of(dev))
    return Y, (mask if mask is not None else argmax)


def spmm_bwd_bf16(view_t: CSRView, w_t: torch.Tensor | None, row_scale: torch.Tensor | None,
                  dY: torch.Tensor, reduce: int, cnt: torch.Tensor | None = None,
                  argmax: torch.Tensor | None = None, win_mask: torch.Tensor | None = None,
                  slot_map: torch.Tensor | None = None) -> torch.Tensor:
    """:func:`mgcn.ops.spmm_bwd` over bf16 rows: dH (bf16) = round(sum_k
    g(float(dY[col_k])) * w_k [* row_scale]).  Mean takes the undivided dY and
    ``cnt``: the kernel divides every gathered row in fp32."""
    lib = L.load()
    dY = _rows_bf16(dY, "dY")
    dev = L.require_device(dY, view_t.rowptr, w_t, row_scale, cnt)
    F = dY.size(1)
    dH = torch.empty(view_t.n_rows, F, dtype=BF16, device=dev)
    launch("spmm_bwd_bf16", "mgcn_spmm_bwd_bf16", dev, view_t.n_rows, view_t.edges,
           lib.mgcn_spmm_bwd_bf16,
           view_t.n_rows, F, L.ptr(view_t.rowptr), L.ptr(view_t.col), L.ptr(view_t.eid),
           L.ptr(w_t), L.ptr(row_scale), L.ptr(dY), dY.stride(0), L.ptr(dH), dH.stride(0), reduce,
           L.ptr(cnt), L.ptr(argmax), L.ptr(win_mask), L.ptr(slot_map), L.ptr(view_t.order),
           view_t.n_heavy, view_t.n_giant, L.stream_of(dev))
    return dH


def relu_bwd_colsum_bf16(dZ: torch.Tensor, Z: torch.Tensor | None, relu: bool, want_db: bool):
    """(dY, db): dY = Z > 0 ? dZ : 0 in bf16 (exact; dZ itself when not relu),
    db = sum_i dY[i] accumulated in fp32 in a fixed order.  No row divisor:
    the mean's division lives in :func:`spmm_bwd_bf16`."""
    lib = L.load()
    if dZ.dtype != BF16:
        raise TypeError(f"dZ must be bfloat16, got {dZ.dtype}")
    dZ = dZ.contiguous()
    dev = L.require_device(dZ, Z)
    n, F = dZ.shape
    dY = torch.empty_like(dZ) if relu else dZ
    db = torch.empty(F, dtype=torch.float32, device=dev) if want_db else None
    if not relu and not want_db:
        return dY, None
    ws, ws_bytes = workspace(lib.mgcn_colsum_workspace_bytes(n, F), dev) if want_db else (None, 0)
    launch("relu_bwd_colsum_bf16", "mgcn_relu_bwd_colsum_bf16", dev, n, None,
           lib.mgcn_relu_bwd_colsum_bf16,
           n, F, L.ptr(dZ), L.ptr(Z.contiguous() if relu else None), int(bool(relu)),
           L.ptr(dY if relu else None), L.ptr(db), L.ptr(ws), ws_bytes, L.stream_of(dev))
    return dY, db


class _AggregateBf16(torch.autograd.Function):
    """:class:`mgcn.ops._Aggregate` over bf16 rows: bf16 H, fp32 norm weights,
    fp32 bias in the epilogue; saves the bf16 Y (ReLU) and the winner bits
    (max).  Backward: relu_bwd_colsum_bf16, then spmm_bwd_bf16 (mean: cnt =
    plan.in_cnt, divided inside the kernel); dH in bf16, db summed in fp32."""

    @staticmethod
    def forward(ctx, H, bias, plan: GraphPlan, norm: NormPlan, reduce: int, relu: bool):
        Y, mask = spmm_fwd_bf16(plan.fwd, norm.w_fwd, H, reduce, bias, relu, mask_plan=plan)
        ctx.plan, ctx.norm, ctx.reduce, ctx.relu = plan, norm, reduce, relu
        ctx.bias_dtype = bias.dtype if bias is not None else None
        ctx.save_for_backward(Y if relu else None, mask)  # max: winner bits per edge
        return Y

    @staticmethod
    def backward(ctx, dZ):
        Y, mask = ctx.saved_tensors
        plan, norm = ctx.plan, ctx.norm
        need_h = ctx.needs_input_grad[0]
        need_b = ctx.bias_dtype is not None and ctx.needs_input_grad[1]
        mean = ctx.reduce == L.REDUCE_MEAN
        dY, db = relu_bwd_colsum_bf16(dZ.to(BF16), Y, ctx.relu, need_b)
        dH = None
        if need_h:
            dH = spmm_bwd_bf16(plan.bwd, norm.w_bwd, norm.row_scale_bwd, dY, ctx.reduce,
                               cnt=plan.in_cnt if mean else None, win_mask=mask,
                               slot_map=plan.slot_map() if mask is not None else None)
        if db is not None and db.dtype != ctx.bias_dtype:
            db = db.to(ctx.bias_dtype)  # a bf16 bias parameter: its gradient rounded once
        return dH, db, None, None, None, None


def spmm_xw_bf16_supported(view: CSRView, F_in: int, F_out: int, reduce: int,
                           ld: int | None = None) -> bool:
    """True when :func:`spmm_xw_fwd_bf16` (``view`` the fwd view) or
    :func:`spmm_xw_bwd_bf16` (``view`` the bwd view, F_in / F_out swapped)
    takes this layer: 128 -> 128, sum or mean, no heavy rows, and -- when
    given -- a leading dimension ``ld`` of the gathered rows that keeps them
    16-byte aligned in place."""
    if ld is not None and (int(ld) < int(F_in) or int(ld) % 8):
        return False
    return (view.n_heavy == 0 and view.n_cols > 0 and
            bool(L.load().mgcn_spmm_xw_bf16_supported(int(F_in), int(F_out), int(reduce))))


def spmm_xw_bf16(view: CSRView, w, row_scale, cnt, X: torch.Tensor, W: torch.Tensor,
                 transpose: bool, bias, relu: bool, reduce: int, want_z: bool,
                 tname: str | None = "spmm_xw_bf16"):
    """``mgcn_spmm_xw_bf16`` as it stands, both directions: (Y, Zb or None) with
    Y = round(epi(Zb @ (W^T if transpose else W) + bias)); the launch is
    timed under ``tname``.  :func:`spmm_xw_fwd_bf16` and
    :func:`spmm_xw_bwd_bf16` are the two uses a layer makes of it."""
    lib = L.load()
    X = _rows_bf16(X, "X" if not transpose else "dY")
    W = _rows_bf16(W, "W")
    dev = L.require_device(X, W, view.rowptr, w, row_scale, cnt, bias)
    if X.size(0) != view.n_cols:
        raise ValueError(f"gathered table has {X.size(0)} rows, the view has {view.n_cols} columns")
    if X.size(1) != 128 or tuple(W.shape) != (128, 128) or view.n_heavy:
        raise ValueError("the fused bf16 layer kernel takes 128 -> 128 layers on views without "
                         f"heavy rows: X {tuple(X.shape)}, W {tuple(W.shape)}, "
                         f"n_heavy = {view.n_heavy}")
    Y = torch.empty(view.n_rows, 128, dtype=BF16, device=dev)
    Z = torch.empty(view.n_rows, 128, dtype=BF16, device=dev) if want_z else None
    bias = _bias_f32(bias, 128)
    launch(tname, "mgcn_spmm_xw_bf16", dev, view.n_rows, view.edges, lib.mgcn_spmm_xw_bf16,
           view.n_rows, 128, 128, L.ptr(view.rowptr), L.ptr(view.col), L.ptr(w),
           L.ptr(row_scale), L.ptr(cnt), L.ptr(X), X.stride(0), L.ptr(W), W.stride(0),
           int(bool(transpose)), L.ptr(bias), int(bool(relu)), L.ptr(Y), Y.stride(0), L.ptr(Z),
           128, reduce, L.stream_of(dev))
    return Y, Z


def spmm_xw_fwd_bf16(view: CSRView, w: torch.Tensor | None, X: torch.Tensor, W: torch.Tensor,
                     reduce: int, bias: torch.Tensor | None = None, relu: bool = False,
                     want_z: bool = False):
    """Y (bf16) = round(epi(Zb @ W + bias)), Zb = :func:`spmm_fwd_bf16`'s rows
    bit for bit (for mean the divided rows), in one launch
    (``mgcn_spmm_xw_bf16``): bf16 ``X`` [n_cols, 128] and ``W`` [128, 128],
    fp32 weights and bias, one bf16 MFMA term with fp32 accumulators.  With
    ``want_z`` returns (Y, Zb)."""
    if reduce not in (L.REDUCE_SUM, L.REDUCE_MEAN):
        raise ValueError("spmm_xw_fwd_bf16: sum or mean only (max does not commute with W)")
    Y, Z = spmm_xw_bf16(view, w, None, None, X, W, False, bias, relu, reduce, want_z,
                        tname="spmm_xw_fwd_z_bf16" if want_z else "spmm_xw_fwd_bf16")
    return (Y, Z) if want_z else Y


def spmm_xw_bwd_bf16(view_t: CSRView, w_t: torch.Tensor | None, row_scale: torch.Tensor | None,
                     dY: torch.Tensor, W: torch.Tensor, cnt: torch.Tensor | None = None):
    """dX (bf16) = round(dHb @ W^T), dHb = :func:`spmm_bwd_bf16`'s rows bit
    for bit (sum, or mean when ``cnt`` is given: every gathered dY row divided
    by cnt inside the kernel), in one launch (``mgcn_spmm_xw_bf16`` with the
    transpose flag)."""
    return spmm_xw_bf16(view_t, w_t, row_scale, cnt, dY, W, True, None, False, L.REDUCE_SUM, False,
                        tname="spmm_xw_bwd_bf16")[0]


class _LayerXWBf16(torch.autograd.Function):
    """One bf16 GCN layer  y = epi((A_norm x) W + b)  on the fused bf16 kernel:
    the forward is one launch (Z = the rounded aggregate kept only when W
    wants a gradient); the backward runs relu_bwd_colsum_bf16 (dY, fp32 db),
    dW = Z^T dY on the vendor bf16 GEMM and one spmm_xw_bwd_bf16 for dx."""

    @staticmethod
    def forward(ctx, x, W, bias, plan: GraphPlan, norm: NormPlan, reduce: int, relu: bool):
        want_z = bool(ctx.needs_input_grad[1])
        out = spmm_xw_fwd_bf16(plan.fwd, norm.w_fwd, x, W, reduce, bias, relu, want_z=want_z)
        Y, Z = out if want_z else (out, None)
        ctx.plan, ctx.norm, ctx.reduce, ctx.relu = plan, norm, reduce, relu
        ctx.bias_dtype = bias.dtype if bias is not None else None
        ctx.save_for_backward(W, Y if relu else None, Z)
        return Y

    @staticmethod
    def backward(ctx, dZ):
        W, Y, Z = ctx.saved_tensors
        plan, norm = ctx.plan, ctx.norm
        need_b = ctx.bias_dtype is not None and ctx.needs_input_grad[2]
        mean = ctx.reduce == L.REDUCE_MEAN
        dY, db = relu_bwd_colsum_bf16(dZ.to(BF16), Y, ctx.relu, need_b)
        dW = dx = None
        if Z is not None:
            from .ops_gemm import VENDOR_GEMMS
            VENDOR_GEMMS[("matmul", (Z.size(1), Z.size(0)), tuple(dY.shape), str(BF16))] += 1
            dW = torch.matmul(Z.t(), dY)  # mean: Z is the divided row, dY undivided
        if ctx.needs_input_grad[0]:
            dx = spmm_xw_bwd_bf16(plan.bwd, norm.w_bwd, norm.row_scale_bwd, dY, W,
                                  cnt=plan.in_cnt if mean else None)
        if db is not None and db.dtype != ctx.bias_dtype:
            db = db.to(ctx.bias_dtype)
        return dx, dW, db, None, None, None, None


class _SegmentReduceBf16(torch.autograd.Function):
    """:class:`mgcn.ops._SegmentReduce` over a bf16 [E, F] ``src`` (F % 8 == 0)."""

    @staticmethod
    def forward(ctx, src, index, dim_size: int, reduce: int):
        dev = L.require_device(src, index)
        E = src.size(0)
        from .graph import build_view
        ids = torch.arange(E, dtype=torch.int64, device=dev)
        view = build_view(index, ids, dim_size, E)
        Y, argmax = spmm_fwd_bf16(view, None, src, reduce)
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
        d_src = spmm_bwd_bf16(ctx.view_t, None, None, dY.to(BF16), ctx.reduce,
                              cnt=ctx.cnt if ctx.reduce == L.REDUCE_MEAN else None, argmax=argmax)
        return d_src, None, None, None
