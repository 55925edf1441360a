"""Multi-kernel aggregation: K edge sets over one node set on libmgcn's
multi-kernel launches (csrc/multi_kernel.hip), one per direction.  Sits on
:mod:`mgcn.ops_gemm` (the ReLU / bias adjoint is ``relu_bwd_colsum``);
:mod:`mgcn.ops` re-exports every name and holds the route's switch."""
from __future__ import annotations

import torch

from . import _lib as L
from ._call import _contig_f32, launch
from .ops_gemm import relu_bwd_colsum


def _views(plans, norms, bwd: bool, biases=None, mean: bool = False) -> L.MultiViewsC:
    """The K pointer sets of one direction (include/mgcn.h mgcn_multi_views).
    The caller keeps every tensor alive until the launch is enqueued."""
    v = L.MultiViewsC()
    for k, (plan, norm) in enumerate(zip(plans, norms)):
        view = plan.bwd if bwd else plan.fwd
        w = norm.w_bwd if bwd else norm.w_fwd
        v.n_rows[k] = view.n_rows
        v.rowptr[k] = view.rowptr.data_ptr()
        v.col[k] = view.col.data_ptr()
        v.w[k] = None if w is None else w.data_ptr()
        if bwd:
            v.cnt[k] = plan.in_cnt.data_ptr() if mean else None
            rs = norm.row_scale_bwd
            v.row_scale[k] = None if rs is None else rs.data_ptr()
        elif biases[k] is not None:
            v.bias[k] = biases[k].data_ptr()
    return v


def _edges(plans, bwd: bool) -> int:
    return sum((p.bwd if bwd else p.fwd).edges for p in plans)


def multi_spmm_fwd(plans, norms, H_all: torch.Tensor, reduce: int, combine: int, biases,
                   relu: bool = False, out: torch.Tensor | None = None) -> torch.Tensor:
    """Y = combine_k epi_k(A_k H_all[:, k C:(k + 1) C]) in one launch
    (``mgcn_multi_spmm_fwd``): Y is [N, C], or [N, K C] under cat."""
    lib = L.load()
    K = len(plans)
    H_all = _contig_f32(H_all, "H_all")
    N = H_all.size(0)
    C = H_all.size(1) // max(K, 1)
    biases = [None if b is None else b.detach().to(torch.float32).contiguous() for b in biases]
    dev = L.require_device(H_all, *[p.fwd.rowptr for p in plans], *[n.w_fwd for n in norms],
                           *biases)
    Y = out if out is not None else torch.empty(
        N, K * C if combine == L.COMBINE_CODES["cat"] else C, dtype=torch.float32, device=dev)
    v = _views(plans, norms, False, biases)
    launch("multi_spmm_fwd", "mgcn_multi_spmm_fwd", dev, N, _edges(plans, False),
           lib.mgcn_multi_spmm_fwd, N, K, C, v, L.ptr(H_all), H_all.stride(0), L.ptr(Y),
           Y.stride(0), reduce, combine, int(bool(relu)), L.stream_of(dev))
    return Y


def multi_spmm_bwd(plans, norms, dY: torch.Tensor, reduce: int, combine: int,
                   out: torch.Tensor | None = None) -> torch.Tensor:
    """dH_all [N, K C]: block k = A_k^T g_k(dY) [* row_scale_k] in one launch
    (``mgcn_multi_spmm_bwd``); dY is [N, C], or [N, K C] under cat."""
    lib = L.load()
    K = len(plans)
    dY = _contig_f32(dY, "dY")
    N = dY.size(0)
    C = dY.size(1) // K if combine == L.COMBINE_CODES["cat"] else dY.size(1)
    mean = reduce == L.REDUCE_MEAN
    dev = L.require_device(dY, *[p.bwd.rowptr for p in plans], *[n.w_bwd for n in norms],
                           *[n.row_scale_bwd for n in norms])
    dH = out if out is not None else torch.empty(N, K * C, dtype=torch.float32, device=dev)
    v = _views(plans, norms, True, mean=mean)
    launch("multi_spmm_bwd", "mgcn_multi_spmm_bwd", dev, N, _edges(plans, True),
           lib.mgcn_multi_spmm_bwd, N, K, C, v, L.ptr(dY), dY.stride(0), L.ptr(dH), dH.stride(0),
           reduce, combine, L.stream_of(dev))
    return dH


class _MultiAggregate(torch.autograd.Function):
    """The message passing of K plain NodeModelAdditive kernels after their
    shared ``x @ [W_0 | .. | W_{K-1}]`` and the kernel combine
    (gcn_multi_kernel.py:93-112), ``H_all, *biases -> Y``.

    Forward: one mgcn_multi_spmm_fwd.  Saved: Y under ReLU.  Backward: one
    relu_bwd_colsum over dZ (the ReLU mask and the column sums every bias
    gradient comes from), then one mgcn_multi_spmm_bwd."""

    @staticmethod
    def forward(ctx, H_all, plans, norms, reduce: int, combine: int, relu: bool, *biases):
        Y = multi_spmm_fwd(plans, norms, H_all, reduce, combine, biases, relu)
        ctx.plans, ctx.norms, ctx.reduce, ctx.combine, ctx.relu = plans, norms, reduce, combine, relu
        ctx.has_bias = [b is not None for b in biases]
        ctx.save_for_backward(Y if relu else None)
        return Y

    @staticmethod
    def backward(ctx, dZ):
        Y, = ctx.saved_tensors
        K = len(ctx.plans)
        need_b = any(h and g for h, g in zip(ctx.has_bias, ctx.needs_input_grad[6:]))
        dY, cs = relu_bwd_colsum(_contig_f32(dZ, "dY"), Y, ctx.relu, need_b)
        dH = None
        if ctx.needs_input_grad[0]:
            dH = multi_spmm_bwd(ctx.plans, ctx.norms, dY, ctx.reduce, ctx.combine)
        db = [None] * K
        if need_b:
            if ctx.combine == L.COMBINE_CODES["cat"]:
                C = cs.numel() // K
                parts = [cs[k * C:(k + 1) * C] for k in range(K)]
            else:
                if ctx.combine == L.COMBINE_CODES["mean"]:
                    cs = cs / K
                parts = [cs] + [cs.clone() for _ in range(K - 1)]  # one tensor per parameter
            db = [p if h else None for p, h in zip(parts, ctx.has_bias)]
        return (dH, None, None, None, None, None, *db)


def multi_kernel_reason(x: torch.Tensor, n_kernels: int, aggr: str = "add", plain: bool = True,
                        edge_attr: bool = False) -> str | None:
    """Why a multi-kernel layer cannot take the fused route, from what is known
    before any plan is built (None: nothing so far): the number of kernels
    with edges, the node models (``plain``: every one a NodeModelAdditive
    without gate), the aggregation, edge features and the input rows."""
    if not 2 <= n_kernels <= L.MULTI_MAX_K:
        return f"{n_kernels} kernels with edges (the fused route takes 2 to {L.MULTI_MAX_K})"
    if not plain:
        return "a gated or attention node model"
    if aggr not in ("add", "mean"):
        return f"aggr={aggr!r} (add and mean only)"
    if edge_attr:
        return "edge_attr message terms"
    if x.dim() != 2 or x.dtype != torch.float32:
        return f"x is {x.dtype}, {x.dim()}-D (float32 [N, F] only)"
    if not x.is_cuda:
        return "x is not on the device"
    return None


def multi_kernel_fusable(x: torch.Tensor, plans, norms, aggr: str = "add", plain: bool = True,
                         edge_attr: bool = False, out_channels: int | None = None) -> bool:
    """True when ``multi_aggregate(linear(x, cat(W_k)), plans, norms, ...)`` is
    the layer's route: :func:`multi_kernel_reason` finds nothing, no norm
    carries autograd history, every plan spans x's rows, no view of any plan
    has heavy rows (the launches walk rows in natural order, one lane group
    each) and the switch (:func:`mgcn.ops.set_fused_multi_kernel`) is on.

    With ``out_channels`` (the width C of every kernel) the shapes whose
    per-kernel layers run on the fused aggregate-then-transform kernels
    (:func:`mgcn.ops.layer_fusable`: 128 -> 128 and 256 -> 256) are declined:
    there the loop never writes x W_k at all, and measured faster than this
    route's GEMM + gather (profiles/multi_kernel/ab.json)."""
    from . import ops  # the switches live beside set_fused_layers
    if not ops._FUSE_MULTI:
        return False
    if len(plans) != len(norms) or multi_kernel_reason(x, len(plans), aggr, plain, edge_attr):
        return False
    if not (all(not n.grad for n in norms) and all(
            p.num_nodes == x.size(0) and p.nnz < 2 ** 31 and p.fwd.n_heavy == 0
            and p.bwd.n_heavy == 0 for p in plans)):
        return False
    if out_channels is not None and ops._FUSE_XW:
        f_in, reduce = x.size(1), L.REDUCE_CODES[aggr]
        if all(ops.spmm_xw_supported(p.fwd, f_in, out_channels, reduce, x.stride(0)) and
               ops.spmm_xw_supported(p.bwd, out_channels, f_in, L.REDUCE_SUM) for p in plans):
            return False
    return True


def multi_aggregate(H_all: torch.Tensor, plans, norms, biases=None, aggr: str = "add",
                    combine: str = "add", relu: bool = False) -> torch.Tensor:
    """The K kernels of a multi-kernel layer after their projections, fused:

        Y = combine_k ( reduce_{e in A_k -> i} n_e H_all[j, k C:(k + 1) C] + bias_k )

    ``H_all`` [N, K C] float32 holds the K projected row blocks side by side
    (``linear(x, torch.cat(Ws, 1))``), ``plans`` / ``norms`` the K graph plans
    over the same N nodes with their normalisations, ``biases`` K entries
    ([C] or None; None: no biases), ``aggr`` add / mean, ``combine`` add /
    mean (sum / K) / cat ([N, K C]), ReLU in the epilogue.  Differentiable in
    H_all and the biases; equal, bit for bit, to K :func:`aggregate_plan`
    calls on the column blocks combined left to right.  2 <= K <= 8; plans
    with heavy rows are the caller's to route elsewhere
    (:func:`multi_kernel_fusable`).  CPU tensors raise: no CPU path."""
    plans, norms = list(plans), list(norms)
    K = len(plans)
    biases = [None] * K if biases is None else list(biases)
    L.require_device(H_all, *[p.fwd.rowptr for p in plans], *biases)
    if not (1 <= K <= L.MULTI_MAX_K) or len(norms) != K or len(biases) != K:
        raise ValueError(f"multi_aggregate: {K} plans, {len(norms)} norms, {len(biases)} biases "
                         f"(1 to {L.MULTI_MAX_K} of each)")
    if aggr not in ("add", "sum", "mean"):
        raise ValueError(f"multi_aggregate: aggr must be add or mean, got {aggr!r}")
    if combine not in L.COMBINE_CODES:
        raise ValueError(f"multi_aggregate: combine must be add, mean or cat, got {combine!r}")
    H_all = _contig_f32(H_all, "H_all")
    N, KC = H_all.shape
    if KC % K or KC == 0:
        raise ValueError(f"multi_aggregate: H_all has {KC} columns for {K} kernels")
    C = KC // K
    for p in plans:
        if p.num_nodes != N:
            raise ValueError(f"H_all has {N} rows, a graph has {p.num_nodes} nodes")
    if any(n.grad for n in norms):
        raise ValueError("multi_aggregate: differentiable edge weights / degrees are not "
                         "supported (use aggregate_plan per kernel)")
    for b in biases:
        if b is not None and b.numel() != C:
            raise ValueError(f"bias has {b.numel()} entries, expected {C}")
    return _MultiAggregate.apply(H_all, tuple(plans), tuple(norms), L.REDUCE_CODES[aggr],
                                 L.COMBINE_CODES[combine], bool(relu), *biases)
