"""Aggregation on a mini-batch block: rectangular launches over the block's
own plan with PyG's self-loop rules folded in (``mgcn_block_spmm_fwd`` /
``mgcn_block_spmm_bwd``, include/mgcn.h), so a convolution on a fresh block
edits no edge list and builds no plan.  Depends on :mod:`mgcn._call` and
:mod:`mgcn.ops_block`; :mod:`mgcn.ops` re-exports every name.

``block_aggregate(x, block, aggr, loops)`` is, bit for bit, the first
``n_dst`` rows of ``aggregate_plan`` on the plan of

    loops='keep'    block.edge_index
    loops='drop'    pyg.remove_self_loops(block.edge_index)
    loops='append'  pyg.add_remaining_self_loops(block.edge_index, w, fill, n_src)

and its gradient is that path's gradient (up to the sign of a zero)."""
from __future__ import annotations

import os

import torch

from . import _lib as L
from ._call import _contig_f32, launch
from .ops_block import Block

LOOPS_CODES = {"keep": 0, "drop": 1, "append": 2}  # include/mgcn.h MGCN_LOOPS_*

# convs on a Block take the block launches (:func:`block_conv_supported`);
# MGCN_BLOCK_CONV=0 keeps conv(x, block.edge_index)[:n_dst] everywhere
_BLOCK_CONV = os.environ.get("MGCN_BLOCK_CONV", "1") != "0"


def set_block_convs(enabled: bool) -> None:
    """Send (True, the default) the convs of :mod:`mgcn.pyg` on a
    :class:`Block` through :func:`block_aggregate` where
    :func:`block_conv_supported` holds, or (False; env MGCN_BLOCK_CONV=0) keep
    them all on ``conv(x, block.edge_index)[:block.n_dst]``."""
    global _BLOCK_CONV
    _BLOCK_CONV = bool(enabled)


def block_convs() -> bool:
    """The switch :func:`set_block_convs` sets."""
    return _BLOCK_CONV


def block_conv_supported(block: Block, x: torch.Tensor, edge_weight=None) -> bool:
    """True when a conv on ``block`` takes the block launches: the switch is on,
    ``x`` is a 2-D float32 tensor, ``edge_weight`` (float32) needs no gradient, and
    neither view of ``block.plan`` has heavy rows (the block kernels walk a row
    with one lane group; rows above 128 slots keep the workgroup path of the
    shipped route)."""
    return (_BLOCK_CONV and isinstance(x, torch.Tensor) and x.dtype == torch.float32 and
            x.dim() == 2 and
            (edge_weight is None or
             (edge_weight.dtype == torch.float32 and not edge_weight.requires_grad)) and
            block.plan.fwd.n_heavy == 0 and block.plan.bwd.n_heavy == 0)


def block_spmm_fwd(block: Block, w, x: torch.Tensor, reduce: int, loops: int, fill: float):
    """(Y [n_dst, F], cnt [n_dst]) of ``mgcn_block_spmm_fwd`` on ``block``."""
    lib = L.load()
    view = block.plan.fwd
    dev = L.require_device(x, view.rowptr, w)
    F = x.size(1)
    Y = torch.empty(block.n_dst, F, dtype=torch.float32, device=dev)
    cnt = torch.empty(block.n_dst, dtype=torch.float32, device=dev)
    launch("block_fwd", "mgcn_block_spmm_fwd", dev, block.n_dst, view.edges,
           lib.mgcn_block_spmm_fwd, block.n_dst, block.n_src, F, L.ptr(view.rowptr),
           L.ptr(view.col), L.ptr(w), float(fill), loops, L.ptr(x), x.stride(0), L.ptr(Y),
           Y.stride(0), reduce, L.ptr(cnt), L.stream_of(dev))
    return Y, cnt


def block_spmm_bwd(block: Block, w, dY: torch.Tensor, reduce: int, loops: int, fill: float,
                   cnt) -> torch.Tensor:
    """dX [n_src, F] of ``mgcn_block_spmm_bwd`` on ``block``."""
    lib = L.load()
    view = block.plan.bwd
    dY = _contig_f32(dY, "dY")
    dev = L.require_device(dY, view.rowptr, w, cnt)
    F = dY.size(1)
    dX = torch.empty(block.n_src, F, dtype=torch.float32, device=dev)
    launch("block_bwd", "mgcn_block_spmm_bwd", dev, block.n_src, view.edges,
           lib.mgcn_block_spmm_bwd, block.n_src, block.n_dst, F, L.ptr(view.rowptr),
           L.ptr(view.col), L.ptr(view.eid), L.ptr(w), float(fill), loops, L.ptr(dY),
           dY.stride(0), L.ptr(dX), dX.stride(0), reduce, L.ptr(cnt), L.stream_of(dev))
    return dX


class _BlockAggregate(torch.autograd.Function):
    """One node over the two block launches; the forward's counts feed the
    mean's adjoint."""

    @staticmethod
    def forward(ctx, x, w, block: Block, reduce: int, loops: int, fill: float):
        Y, cnt = block_spmm_fwd(block, w, x, reduce, loops, fill)
        ctx.block, ctx.reduce, ctx.loops, ctx.fill = block, reduce, loops, fill
        ctx.save_for_backward(w, cnt)
        return Y

    @staticmethod
    def backward(ctx, dY):
        w, cnt = ctx.saved_tensors
        dX = None
        if ctx.needs_input_grad[0]:
            dX = block_spmm_bwd(ctx.block, w, dY, ctx.reduce, ctx.loops, ctx.fill,
                                cnt if ctx.reduce == L.REDUCE_MEAN else None)
        return dX, None, None, None, None, None


def block_aggregate(x: torch.Tensor, block: Block, aggr: str = "add", loops: str = "keep",
                    edge_weight: torch.Tensor | None = None, fill: float = 1.0) -> torch.Tensor:
    """The aggregate of ``block``'s ``n_dst`` destinations over ``x`` (float32
    [n_src, F] on the block's device): [n_dst, F].  ``aggr`` 'add' or 'mean';
    ``loops`` 'keep', 'drop' (in-row self loops do not count) or 'append'
    (dropped, then one loop per destination last, PyG 1.3's
    add_remaining_self_loops: its weight is the row's last loop's, else
    ``fill``); ``edge_weight`` float32 [nnz_b] in the block's COO order
    (``w_parent[block.parent_eid]``), no gradient.  Always the block kernels,
    whatever the row lengths.  An empty block gives an empty tensor."""
    if not isinstance(block, Block):
        raise ValueError(f"block must be a mgcn.Block, got {type(block).__name__}")
    if aggr == "max" or aggr not in L.REDUCE_CODES:
        raise ValueError(f"block_aggregate: aggr must be 'add' or 'mean', got {aggr!r}")
    if loops not in LOOPS_CODES:
        raise ValueError(f"block_aggregate: loops must be 'keep', 'drop' or 'append', "
                         f"got {loops!r}")
    x = _contig_f32(x, "x")
    if x.size(0) != block.n_src:
        raise ValueError(f"x has {x.size(0)} rows, the block has {block.n_src} source nodes")
    if x.size(1) < 1:
        raise ValueError("x must have at least one feature column")
    w = None
    if edge_weight is not None:
        if edge_weight.requires_grad:
            raise ValueError("block_aggregate: edge_weight with a gradient is not supported "
                             "(the convs fall back for it)")
        if edge_weight.dtype != torch.float32 or edge_weight.dim() != 1 or \
                edge_weight.numel() != block.plan.nnz:
            raise ValueError(f"edge_weight must be float32 [{block.plan.nnz}], got "
                             f"{edge_weight.dtype} {tuple(edge_weight.shape)}")
        w = edge_weight.contiguous()
    L.require_device(x, block.plan.fwd.rowptr, w)
    if block.n_dst == 0:
        return x[:0]
    return _BlockAggregate.apply(x, w, block, L.REDUCE_CODES[aggr], LOOPS_CODES[loops],
                                 float(fill))


__all__ = ["LOOPS_CODES", "block_aggregate", "block_conv_supported", "block_convs",
           "block_spmm_bwd", "block_spmm_fwd", "set_block_convs"]
