"""Edge-gated aggregation over a graph plan on libmgcn's gate kernels
(csrc/edge_gate.hip).  Sits on :mod:`mgcn.ops_gemm` (the score vectors'
gradients are one ``gemm_tn``, the ReLU / bias / mean adjoint is
``relu_bwd_colsum``); :mod:`mgcn.ops` re-exports every name.

Feature rows are fp32 or bf16 (``Hx.dtype``).  A bf16 ``Hx`` takes the
``mgcn_gate_*_bf16`` sibling of every gate launch (timer names end in
``_bf16``): Hx, Y, dY and dHx are bf16, scores, gates and every gradient of a
parameter fp32.  Contract ("Edge gates", "bf16 rows"): every
fp32 output has the bits of the fp32 path on ``Hx.float()`` / ``dY.float()``,
every bf16 output those bits rounded once."""
from __future__ import annotations

import os

import torch

from . import _lib as L
from ._call import _contig_f32, launch
from .graph import GraphPlan, NormPlan
from .ops_bf16 import relu_bwd_colsum_bf16
from .ops_gemm import gemm_tn, relu_bwd_colsum

BF16 = torch.bfloat16


# heavy rows (degree > 128, graph.schedule_rows) of a gated layer by workgroups
# (the mgcn_gate_*_sched entries, bit-identical to the wave-per-row launches);
# MGCN_GATE_HEAVY=0 keeps the wave-per-row launches for every row
_GATE_HEAVY = os.environ.get("MGCN_GATE_HEAVY", "1") != "0"


def set_gate_heavy_rows(enabled: bool) -> None:
    """Send (True, the default) the heavy rows of a gated layer's three
    launches through the workgroup path (mgcn_gate_fwd_sched / _bwd_dst_sched /
    _bwd_src_sched) or keep (False; env MGCN_GATE_HEAVY=0) one wave per row
    for every row.  Results are bitwise the same either way."""
    global _GATE_HEAVY
    _GATE_HEAVY = bool(enabled)


def gate_heavy_rows() -> bool:
    """The switch :func:`set_gate_heavy_rows` sets."""
    return _GATE_HEAVY


def _heavy(view) -> bool:
    return _GATE_HEAVY and view.order is not None and view.n_heavy > 0


def _max_mask(plan: GraphPlan, argmax: torch.Tensor) -> torch.Tensor:
    """Winner bits of every edge at its fwd slot (mgcn_max_mask), as
    :func:`mgcn.ops.max_mask`."""
    lib = L.load()
    F = argmax.size(1)
    dev = argmax.device
    mask = torch.empty(max(plan.nnz, 1), (F + 31) // 32, dtype=torch.int32, device=dev)
    launch(None, "mgcn_max_mask", dev, None, None, lib.mgcn_max_mask,
           plan.fwd.n_rows, F, L.ptr(plan.fwd.rowptr), L.ptr(plan.fwd.eid), L.ptr(argmax),
           L.ptr(mask), L.stream_of(dev))
    return mask


class _GateAggregate(torch.autograd.Function):
    """The message passing of a gated NodeModelAdditive after its ``x @ W``
    (gcn_base_models.py:209-241 with the gate of :322-396) on libmgcn's gate
    kernels.

    Forward: mgcn_att_scores (H = 1, the two gate vectors concatenated) when
    the gate projects node rows, then one mgcn_gate_fwd launch (logit, sigmoid,
    weighted gather, reduce, bias, ReLU); max: mgcn_max_mask on its argmax.
    Saved: Hx, the gate (fwd slot order), the gate vectors, Y under ReLU, the
    winner bits under max.  Backward: relu_bwd_colsum, mgcn_gate_bwd_dst,
    mgcn_gate_bwd_src, and [da | dc]^T Hx as one mgcn_gemm_tn.

    A view with heavy rows sends its launches through the ``_sched`` entries
    (:func:`set_gate_heavy_rows`; timer names ``gate_*_heavy``): same bits.

    ``t`` is [E] in COO order or one element; ``w_fwd`` is ``norm.w_fwd`` as an
    autograd input when the norm carries history (else None).  Returns
    ``(Y, g_coo)``, both differentiable."""

    @staticmethod
    def forward(ctx, Hx, wsd, t, bias, w_fwd, plan: GraphPlan, norm: NormPlan, reduce: int,
                relu: bool):
        lib = L.load()
        dev = Hx.device
        N, C = Hx.shape
        nnz = plan.nnz
        st = L.stream_of(dev)
        fwd = plan.fwd
        eid = plan.fwd_eid64() if nnz else None
        a = c = None
        if wsd is not None:
            wsd = wsd.detach().contiguous()
            a = torch.empty(N, dtype=torch.float32, device=dev)
            c = torch.empty(N, dtype=torch.float32, device=dev)
            launch("att_scores", "mgcn_att_scores", dev, N, None, lib.mgcn_att_scores,
                   N, 1, C, L.ptr(Hx), Hx.stride(0), L.ptr(wsd), L.ptr(a), L.ptr(c), st)
        t_bcast = t is not None and t.numel() == 1
        ts = None
        if t is not None:
            ts = t.detach().reshape(-1)
            if not t_bcast:
                ts = ts[eid] if nnz else ts
            ts = ts.contiguous()
        w = norm.w_fwd
        w = None if w is None else w.detach().contiguous()
        b = None if bias is None else bias.detach().to(torch.float32).contiguous()
        Y = torch.empty(N, C, dtype=torch.float32, device=dev)
        g = torch.empty(nnz, dtype=torch.float32, device=dev)
        is_max = reduce == L.REDUCE_MAX
        argmax = torch.empty(N, C, dtype=torch.int32, device=dev) if is_max else None
        args = (N, nnz, C, L.ptr(fwd.rowptr), L.ptr(fwd.col), L.ptr(fwd.eid), L.ptr(a), L.ptr(c),
                L.ptr(ts), int(t_bcast), L.ptr(w), L.ptr(Hx), Hx.stride(0), reduce, L.ptr(b),
                int(bool(relu)), L.ptr(Y), C, L.ptr(g), L.ptr(argmax))
        if _heavy(fwd):
            coef = torch.empty(nnz, dtype=torch.float32, device=dev)
            launch("gate_fwd_heavy", "mgcn_gate_fwd_sched", dev, N, fwd.edges,
                   lib.mgcn_gate_fwd_sched, *args, L.ptr(fwd.order), fwd.n_heavy, fwd.n_giant,
                   L.ptr(coef), st)
        else:
            launch("gate_fwd", "mgcn_gate_fwd", dev, N, fwd.edges, lib.mgcn_gate_fwd, *args, st)
        mask = _max_mask(plan, argmax) if is_max else None
        g_coo = torch.empty_like(g)
        if nnz:
            g_coo[eid] = g
        ctx.plan, ctx.norm, ctx.reduce, ctx.relu = plan, norm, reduce, relu
        ctx.t_shape, ctx.t_bcast = None if t is None else tuple(t.shape), t_bcast
        ctx.has_bias = bias is not None
        ctx.set_materialize_grads(False)  # an unused output sends None, not zeros
        ctx.save_for_backward(Hx, wsd, g, Y if relu else None, mask)
        return Y, g_coo

    @staticmethod
    def backward(ctx, dZ, dg_coo):
        Hx, wsd, g, Y, mask = ctx.saved_tensors
        plan, norm = ctx.plan, ctx.norm
        lib = L.load()
        dev = Hx.device
        N, C = Hx.shape
        nnz = plan.nnz
        st = L.stream_of(dev)
        fwd, bwd = plan.fwd, plan.bwd
        eid = plan.fwd_eid64() if nnz else None
        need_b = ctx.has_bias and ctx.needs_input_grad[3]
        need_w = ctx.needs_input_grad[4]
        mean = ctx.reduce == L.REDUCE_MEAN
        if dZ is None:  # only the gates were used
            dZ = torch.zeros(N, C, dtype=torch.float32, device=dev)
        # mean: dY rows divided by their count once, as _Aggregate does
        dY, db = relu_bwd_colsum(_contig_f32(dZ, "dY"), Y, ctx.relu, need_b,
                                 row_div=plan.in_cnt if mean else None)
        dg_in = None
        if dg_coo is not None and nnz:
            dg_in = dg_coo.to(torch.float32)[eid].contiguous()
        proj = wsd is not None
        w = norm.w_fwd
        w = None if w is None else w.detach().contiguous()
        dl = torch.empty(nnz, dtype=torch.float32, device=dev)
        dc = torch.empty(N, dtype=torch.float32, device=dev) if proj else None
        da = torch.empty(N, dtype=torch.float32, device=dev) if proj else None
        dw = torch.empty(nnz, dtype=torch.float32, device=dev) if need_w else None
        dHx = torch.empty(N, C, dtype=torch.float32, device=dev)
        args = (N, nnz, C, L.ptr(fwd.rowptr), L.ptr(fwd.col), L.ptr(Hx), Hx.stride(0), L.ptr(dY),
                dY.stride(0), L.ptr(w), L.ptr(g), L.ptr(mask), L.ptr(dg_in), L.ptr(dl), L.ptr(dc),
                L.ptr(dw))
        if _heavy(fwd):
            launch("gate_bwd_dst_heavy", "mgcn_gate_bwd_dst_sched", dev, N, fwd.edges,
                   lib.mgcn_gate_bwd_dst_sched, *args, L.ptr(fwd.order), fwd.n_heavy,
                   fwd.n_giant, st)
        else:
            launch("gate_bwd_dst", "mgcn_gate_bwd_dst", dev, N, fwd.edges,
                   lib.mgcn_gate_bwd_dst, *args, st)
        slot = plan.slot_map() if nnz else None
        args = (N, nnz, C, L.ptr(bwd.rowptr), L.ptr(bwd.col), L.ptr(slot), L.ptr(dY),
                dY.stride(0), L.ptr(norm.w_bwd), L.ptr(norm.row_scale_bwd), L.ptr(g), L.ptr(dl),
                L.ptr(mask), L.ptr(wsd), L.ptr(dc), L.ptr(da), L.ptr(dHx), C)
        if _heavy(bwd):
            coef = torch.empty(nnz, dtype=torch.float32, device=dev)
            launch("gate_bwd_src_heavy", "mgcn_gate_bwd_src_sched", dev, N, bwd.edges,
                   lib.mgcn_gate_bwd_src_sched, *args, L.ptr(bwd.order), bwd.n_heavy,
                   bwd.n_giant, L.ptr(coef), st)
        else:
            launch("gate_bwd_src", "mgcn_gate_bwd_src", dev, N, bwd.edges,
                   lib.mgcn_gate_bwd_src, *args, st)
        dwsd = None
        if proj and ctx.needs_input_grad[1]:
            dwsd = gemm_tn(torch.stack([da, dc], dim=1), Hx).reshape(-1)  # [w_src | w_dst]
        dt = None
        if ctx.t_shape is not None and ctx.needs_input_grad[2]:
            if ctx.t_bcast:
                dt = dl.sum().reshape(ctx.t_shape)
            else:
                dt = torch.empty_like(dl)
                if nnz:
                    dt[eid] = dl
                dt = dt.reshape(ctx.t_shape)
        return dHx, dwsd, dt, db, dw, None, None, None, None


class _GateAggregateBf16(torch.autograd.Function):
    """:class:`_GateAggregate` over bf16 rows (the ``mgcn_gate_*_bf16``
    entries; timer names ``gate_*_bf16`` / ``gate_*_heavy_bf16``): Hx, Y, dY
    and dHx are bf16, everything per node and per edge (scores, gates, dl, dc,
    da, bias, the gate vectors) stays fp32.

    Forward: mgcn_att_scores_bf16 (H = 1), one mgcn_gate_fwd[_sched]_bf16
    launch, mgcn_max_mask under max.  Saved: the bf16 Hx, the gate, the gate
    vectors, the bf16 Y under ReLU (its sign is the fp32 Y's, as
    ``_AggregateBf16`` takes it), the winner bits under max.  Backward:
    relu_bwd_colsum_bf16 masks dY (exact), then the two bf16 adjoint launches;
    mean hands them ``plan.in_cnt`` and they divide every loaded dY element in
    fp32, so no divided bf16 row exists.  The gradients of the gate vectors
    and of the bias are taken from fp32 temporaries (Hx upcast for
    mgcn_gemm_tn, the masked dY upcast for the column sums of
    mgcn_relu_bwd_colsum), so they have the fp32 route's bits.

    ``norm`` carries no autograd history here (:func:`gate_aggregate` sends a
    differentiable norm through the upcast route)."""

    @staticmethod
    def forward(ctx, Hx, wsd, t, bias, plan: GraphPlan, norm: NormPlan, reduce: int, relu: bool):
        lib = L.load()
        dev = Hx.device
        N, C = Hx.shape
        nnz = plan.nnz
        st = L.stream_of(dev)
        fwd = plan.fwd
        eid = plan.fwd_eid64() if nnz else None
        a = c = None
        if wsd is not None:
            wsd = wsd.detach().contiguous()
            a = torch.empty(N, dtype=torch.float32, device=dev)
            c = torch.empty(N, dtype=torch.float32, device=dev)
            launch("att_scores_bf16", "mgcn_att_scores_bf16", dev, N, None,
                   lib.mgcn_att_scores_bf16, N, 1, C, L.ptr(Hx), Hx.stride(0), L.ptr(wsd),
                   L.ptr(a), L.ptr(c), st)
        t_bcast = t is not None and t.numel() == 1
        ts = None
        if t is not None:
            ts = t.detach().reshape(-1)
            if not t_bcast:
                ts = ts[eid] if nnz else ts
            ts = ts.contiguous()
        w = norm.w_fwd
        w = None if w is None else w.detach().contiguous()
        b = None if bias is None else bias.detach().contiguous()
        Y = torch.empty(N, C, dtype=BF16, device=dev)
        g = torch.empty(nnz, dtype=torch.float32, device=dev)
        is_max = reduce == L.REDUCE_MAX
        argmax = torch.empty(N, C, dtype=torch.int32, device=dev) if is_max else None
        args = (N, nnz, C, L.ptr(fwd.rowptr), L.ptr(fwd.col), L.ptr(fwd.eid), L.ptr(a), L.ptr(c),
                L.ptr(ts), int(t_bcast), L.ptr(w), L.ptr(Hx), Hx.stride(0), reduce, L.ptr(b),
                int(bool(relu)), L.ptr(Y), C, L.ptr(g), L.ptr(argmax))
        if _heavy(fwd):
            coef = torch.empty(nnz, dtype=torch.float32, device=dev)
            launch("gate_fwd_heavy_bf16", "mgcn_gate_fwd_sched_bf16", dev, N, fwd.edges,
                   lib.mgcn_gate_fwd_sched_bf16, *args, L.ptr(fwd.order), fwd.n_heavy,
                   fwd.n_giant, L.ptr(coef), st)
        else:
            launch("gate_fwd_bf16", "mgcn_gate_fwd_bf16", dev, N, fwd.edges,
                   lib.mgcn_gate_fwd_bf16, *args, st)
        mask = _max_mask(plan, argmax) if is_max else None
        g_coo = torch.empty_like(g)
        if nnz:
            g_coo[eid] = g
        ctx.plan, ctx.norm, ctx.reduce, ctx.relu = plan, norm, reduce, relu
        ctx.t_shape, ctx.t_bcast = None if t is None else tuple(t.shape), t_bcast
        ctx.has_bias = bias is not None
        ctx.set_materialize_grads(False)  # an unused output sends None, not zeros
        ctx.save_for_backward(Hx, wsd, g, Y if relu else None, mask)
        return Y, g_coo

    @staticmethod
    def backward(ctx, dZ, dg_coo):
        Hx, wsd, g, Y, mask = ctx.saved_tensors
        plan, norm = ctx.plan, ctx.norm
        lib = L.load()
        dev = Hx.device
        N, C = Hx.shape
        nnz = plan.nnz
        st = L.stream_of(dev)
        fwd, bwd = plan.fwd, plan.bwd
        eid = plan.fwd_eid64() if nnz else None
        need_b = ctx.has_bias and ctx.needs_input_grad[3]
        cnt = plan.in_cnt if ctx.reduce == L.REDUCE_MEAN else None
        if dZ is None:  # only the gates were used
            dZ = torch.zeros(N, C, dtype=BF16, device=dev)
        dY, _ = relu_bwd_colsum_bf16(dZ.to(BF16), Y, ctx.relu, False)
        # the bf16 column-sum kernel splits the rows among its threads by F / 8,
        # the fp32 one by F / 4: db in the fp32 route's order, from the masked
        # rows upcast (exact)
        db = relu_bwd_colsum(dY.float(), None, False, True)[1] if need_b else None
        dg_in = None
        if dg_coo is not None and nnz:
            dg_in = dg_coo.to(torch.float32)[eid].contiguous()
        proj = wsd is not None
        w = norm.w_fwd
        w = None if w is None else w.detach().contiguous()
        dl = torch.empty(nnz, dtype=torch.float32, device=dev)
        dc = torch.empty(N, dtype=torch.float32, device=dev) if proj else None
        da = torch.empty(N, dtype=torch.float32, device=dev) if proj else None
        dHx = torch.empty(N, C, dtype=BF16, device=dev)
        args = (N, nnz, C, L.ptr(fwd.rowptr), L.ptr(fwd.col), L.ptr(Hx), Hx.stride(0), L.ptr(dY),
                dY.stride(0), L.ptr(w), L.ptr(g), L.ptr(mask), L.ptr(dg_in), L.ptr(dl), L.ptr(dc),
                None, L.ptr(cnt))
        if _heavy(fwd):
            launch("gate_bwd_dst_heavy_bf16", "mgcn_gate_bwd_dst_sched_bf16", dev, N, fwd.edges,
                   lib.mgcn_gate_bwd_dst_sched_bf16, *args, L.ptr(fwd.order), fwd.n_heavy,
                   fwd.n_giant, st)
        else:
            launch("gate_bwd_dst_bf16", "mgcn_gate_bwd_dst_bf16", dev, N, fwd.edges,
                   lib.mgcn_gate_bwd_dst_bf16, *args, st)
        slot = plan.slot_map() if nnz else None
        args = (N, nnz, C, L.ptr(bwd.rowptr), L.ptr(bwd.col), L.ptr(slot), L.ptr(dY),
                dY.stride(0), L.ptr(norm.w_bwd), L.ptr(norm.row_scale_bwd), L.ptr(g), L.ptr(dl),
                L.ptr(mask), L.ptr(wsd), L.ptr(dc), L.ptr(da), L.ptr(dHx), C, L.ptr(cnt))
        if _heavy(bwd):
            coef = torch.empty(nnz, dtype=torch.float32, device=dev)
            launch("gate_bwd_src_heavy_bf16", "mgcn_gate_bwd_src_sched_bf16", dev, N, bwd.edges,
                   lib.mgcn_gate_bwd_src_sched_bf16, *args, L.ptr(bwd.order), bwd.n_heavy,
                   bwd.n_giant, L.ptr(coef), st)
        else:
            launch("gate_bwd_src_bf16", "mgcn_gate_bwd_src_bf16", dev, N, bwd.edges,
                   lib.mgcn_gate_bwd_src_bf16, *args, st)
        dwsd = None
        if proj and ctx.needs_input_grad[1]:
            # [w_src | w_dst]: Hx upcast (an fp32 temporary), the fp32 route's bits
            dwsd = gemm_tn(torch.stack([da, dc], dim=1), Hx.float()).reshape(-1)
        dt = None
        if ctx.t_shape is not None and ctx.needs_input_grad[2]:
            if ctx.t_bcast:
                dt = dl.sum().reshape(ctx.t_shape)
            else:
                dt = torch.empty_like(dl)
                if nnz:
                    dt[eid] = dl
                dt = dt.reshape(ctx.t_shape)
        return dHx, dwsd, dt, db, None, None, None, None


def _rows_f32_or_bf16(Hx: torch.Tensor) -> torch.Tensor:
    """fp32 or bf16 [N, C] rows with unit column stride (any leading dimension
    >= C; the bf16 wave kernels read and write single elements, so any offset)."""
    if Hx.dtype == torch.float32:
        return _contig_f32(Hx, "Hx")
    if Hx.dim() != 2:
        raise ValueError(f"Hx must be 2-D [N, F], got {tuple(Hx.shape)}")
    if Hx.stride(1) != 1 or Hx.stride(0) < Hx.size(1):
        Hx = Hx.contiguous()
    return Hx


def gate_aggregate(Hx: torch.Tensor, plan: GraphPlan, norm: NormPlan, aggr: str = "add",
                   w_src: torch.Tensor | None = None, w_dst: torch.Tensor | None = None,
                   t: torch.Tensor | None = None, bias: torch.Tensor | None = None,
                   relu: bool = False):
    """Gated aggregation (gcn_base_models.py:209-241 with the edge gates of
    :322-396), fused: for edge k: j -> i

        g_k = sigmoid(Hx[j] . w_src + Hx[i] . w_dst + t_k)
        Y[i] = epi(reduce_{k -> i} g_k n_k Hx[j])

    ``Hx`` [N, C] are the projected rows, ``w_src`` / ``w_dst`` ([C] or [1, C],
    both or neither) the gate's two vectors, ``t`` a per-edge logit term [E] /
    [E, 1] in COO order or one element added to every edge (None: none),
    ``n_k`` the weights of ``norm`` (they do not enter the gate), ``aggr`` in
    add / mean / max, bias and ReLU in the kernel's epilogue.

    Returns ``(Y, g_coo)``: Y [N, C] and the gates [E] in COO order.  Both are
    differentiable: in Hx, w_src, w_dst, t, bias and (a norm built with
    ``grad``) the norm's weights; a gradient arriving on ``g_coo`` joins the
    gate's own.

    ``Hx`` is float32 or bfloat16 (any other dtype: ``TypeError``).  float32
    rows take the fp32 launches.  bfloat16 rows stay bf16 through the
    ``mgcn_gate_*_bf16`` kernels (timer names end in ``_bf16``): Y and the
    gradient of Hx are bf16, the saved Hx stays bf16, g_coo and every
    per-node / per-edge quantity stay fp32.  The result is not approximate:
    g_coo and the gradients of w_src, w_dst, t and bias have the bits of the
    fp32 route on ``Hx.float()`` / ``dY.float()``, Y and the gradient of Hx
    those bits rounded once to nearest even.  A norm built with ``grad`` keeps
    the literal route for bf16 rows (upcast, fp32 launches, round), with the
    same bits.  ``w_src``, ``w_dst``, ``t`` and ``bias`` may be float32 or
    bfloat16 with either row dtype; they are cast to fp32 through autograd, so
    a gradient arrives in its parameter's dtype.  CPU tensors raise: no CPU
    path."""
    L.require_device(Hx, plan.fwd.rowptr, w_src, w_dst, t, bias)
    if aggr not in L.REDUCE_CODES:
        raise ValueError(f"aggr must be one of add/mean/max, got {aggr!r}")
    if Hx.dtype not in (torch.float32, BF16):
        raise TypeError(f"Hx must be float32 or bfloat16, got {Hx.dtype}")
    if Hx.dtype == BF16 and norm.grad:
        # dw is wanted: the fp32 launches on the upcast rows, as ops_bf16 does
        # for the plain aggregation
        Y, g = gate_aggregate(Hx.float(), plan, norm, aggr, w_src, w_dst, t, bias, relu)
        return Y.to(BF16), g
    Hx = _rows_f32_or_bf16(Hx)
    N, C = Hx.shape
    if N != plan.num_nodes:
        raise ValueError(f"Hx has {N} rows, graph has {plan.num_nodes} nodes")
    if not (1 <= C <= 1024 and plan.nnz < 2 ** 31):
        raise L.MgcnError(f"gate_aggregate: unsupported shape (C = {C}, nnz = {plan.nnz}): "
                          "need 1 <= C <= 1024, nnz < 2^31")
    if (w_src is None) != (w_dst is None):
        raise ValueError("gate_aggregate: w_src and w_dst come together")
    wsd = None
    if w_src is not None:
        for name, v in (("w_src", w_src), ("w_dst", w_dst)):
            if v.dtype not in (torch.float32, BF16) or v.numel() != C:
                raise ValueError(f"{name} must be float32 or bfloat16 with {C} entries, got "
                                 f"{v.dtype} {tuple(v.shape)}")
        # (a bf16 vector -- a module after .to(torch.bfloat16) -- is cast through
        # autograd: its gradient comes back in its own dtype)
        wsd = torch.cat([w_src.reshape(-1).to(torch.float32), w_dst.reshape(-1).to(torch.float32)])
    if t is not None:
        if t.numel() not in (1, plan.nnz):
            raise ValueError(f"t must have 1 or {plan.nnz} entries, got {tuple(t.shape)}")
        t = t.to(torch.float32)
    if bias is not None:
        if bias.numel() != C:
            raise ValueError(f"bias has {bias.numel()} entries, expected {C}")
        bias = bias.to(torch.float32)
    if Hx.dtype == BF16:
        return _GateAggregateBf16.apply(Hx, wsd, t, bias, plan, norm, L.REDUCE_CODES[aggr],
                                        bool(relu))
    return _GateAggregate.apply(Hx, wsd, t, bias, norm.w_fwd if norm.grad else None, plan, norm,
                                L.REDUCE_CODES[aggr], bool(relu))
