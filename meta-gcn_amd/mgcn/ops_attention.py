"""Soft and hard multi-head attention over a graph plan on libmgcn's
attention kernels.  Sits on :mod:`mgcn.ops_gemm` (the attention vector's
gradient is one ``gemm_tn``); :mod:`mgcn.ops` re-exports every name.

Feature rows are fp32 or bf16 (``Hp.dtype``).  A bf16 ``Hp`` takes the
``mgcn_*_bf16`` sibling of every launch that reads or writes a feature row
(timer names end in ``_bf16``): Hp, Y, dY and dHp are bf16, while the scores,
alpha, the mask, the noise, dz, ds and the attention vector stay fp32.
Contract ("bf16 attention rows"): every fp32 output has the bits of
the fp32 path on ``Hp.float()`` / ``dY.float()``, every bf16 output those bits
rounded once to nearest even.

Heavy rows ("Attention", "Heavy rows"): an fp32 launch over a
view whose row schedule has heavy rows (degree > 128) goes through the
``mgcn_*_sched`` sibling of its entry, which sends those rows to workgroups
and changes no bit (:func:`set_attention_heavy_rows`; timer names are
unchanged).  bf16 rows, ``att_dst_fold`` and the eval forward keep one wave
per row."""
from __future__ import annotations

import os

import torch

from . import _lib as L
from ._call import _contig_f32, launch
from .graph import GraphPlan
from .ops_gemm import gemm_tn
from .ops_noise import DeviceDropout, DeviceGumbel, edge_noise

BF16 = torch.bfloat16


# heavy rows (degree > 128, graph.schedule_rows) of the fp32 attention launches
# by workgroups (the mgcn_(h)att_*_sched entries, bit-identical to the
# wave-per-row launches); MGCN_ATT_HEAVY=0 keeps one wave per row for every row
_ATT_HEAVY = os.environ.get("MGCN_ATT_HEAVY", "1") != "0"


def set_attention_heavy_rows(enabled: bool) -> None:
    """Send (True, the default) the heavy rows of the fp32 attention launches
    (soft and hard: fwd, edge_softmax, bwd_dst, bwd_src) through the workgroup
    path of the ``mgcn_*_sched`` entries, or keep (False; env
    MGCN_ATT_HEAVY=0) one wave per row for every row.  Results are bitwise the
    same either way."""
    global _ATT_HEAVY
    _ATT_HEAVY = bool(enabled)


def attention_heavy_rows() -> bool:
    """The switch :func:`set_attention_heavy_rows` sets."""
    return _ATT_HEAVY


def _require_row_dtype(t: torch.Tensor, name: str) -> None:
    if t.dtype not in (torch.float32, BF16):
        raise TypeError(f"{name} must be float32 or bfloat16, got {t.dtype}")


def _rows(t: torch.Tensor, name: str) -> torch.Tensor:
    """fp32 or bf16 [N, F] rows with unit column stride (any leading dimension
    >= F, any offset: the bf16 kernels read and write single elements)."""
    _require_row_dtype(t, name)
    if t.dtype != BF16:
        return _contig_f32(t, name)
    if t.dim() != 2:
        raise ValueError(f"{name} must be 2-D [N, F], got {tuple(t.shape)}")
    if t.stride(1) != 1 or t.stride(0) < t.size(1):
        t = t.contiguous()
    return t


def _grad_rows(dY: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """The incoming gradient in the row dtype of the forward."""
    if dtype != BF16:
        return _contig_f32(dY, "dY")
    return _rows(dY.to(BF16), "dY")


def _row_launch(lib, name: str, bf16: bool, dev, rows, edges, *args) -> None:
    """One launch that touches feature rows: ``mgcn_<name>``, or for bf16 rows
    its ``mgcn_<name>_bf16`` sibling, timed under the name without ``mgcn_``."""
    if bf16:
        name += "_bf16"
    launch(name, "mgcn_" + name, dev, rows, edges, getattr(lib, "mgcn_" + name), *args)


def _view_launch(lib, name: str, bf16: bool, dev, rows, view, nnz: int, H: int, scratch: bool,
                 *args, bf16_rows: bool = False) -> None:
    """A launch of entry ``name`` that walks ``view`` (args up to the stream,
    which comes last): for fp32 rows over a view with heavy rows, with the
    switch on, its ``mgcn_<name>_sched`` sibling with the view's schedule (and
    a coef scratch [nnz, H] from torch's allocator where the entry takes one),
    under the same timer name; else :func:`_row_launch`.  ``bf16_rows``: a
    launch that touches no feature row (no ``_bf16`` sibling) of an op on bf16
    rows, which keeps the wave launches throughout."""
    if bf16 or bf16_rows or not (_ATT_HEAVY and view.order is not None and view.n_heavy > 0):
        _row_launch(lib, name, bf16, dev, rows, view.edges, *args)
        return
    sched = (L.ptr(view.order), view.n_heavy, view.n_giant)
    if scratch:
        coef = torch.empty(nnz, H, dtype=torch.float32, device=dev)
        sched += (L.ptr(coef),)
    sym = "mgcn_" + name + "_sched"
    launch(name, sym, dev, rows, view.edges, getattr(lib, sym), *args[:-1], *sched, args[-1])


def _att_f32(att_weight: torch.Tensor, H: int, C: int) -> torch.Tensor:
    """The attention vector as fp32 [H, 2C]; a bf16 one (a module after
    ``.to(torch.bfloat16)``) is cast through autograd, so its gradient comes
    back in its own dtype."""
    if att_weight.dtype not in (torch.float32, BF16) or att_weight.numel() != 2 * H * C:
        raise ValueError(f"att_weight must be float32 or bfloat16 [1, {H}, {2 * C}], got "
                         f"{att_weight.dtype} {tuple(att_weight.shape)}")
    return att_weight.reshape(H, 2 * C).to(torch.float32)


def _datt(ds_src, ds_dst, Hp, H: int, C: int):
    """da = [ds_src | ds_dst]^T Hp on mgcn_gemm_tn, of which head h's own C
    columns are its rows; bf16 rows are upcast first (an fp32 temporary), so
    the result is the fp32 path's bit for bit."""
    full = gemm_tn(torch.cat([ds_src, ds_dst], dim=1), Hp.float() if Hp.dtype == BF16 else Hp)
    full = full.view(2, H, H, C)  # [src | dst, head of ds, head of Hp, c]
    hh = torch.arange(H, device=Hp.device)
    return torch.cat([full[0, hh, hh], full[1, hh, hh]], dim=1)  # [H, 2C]


def _train_forward(ctx, Hp, att, mask, noise, T, plan: GraphPlan, H: int, act: int, att_dir: str):
    """The forward of :class:`_AttentionAggregate` (``noise`` and ``T`` None:
    the mgcn_att_* entries) and of :class:`_HardAttentionTrain` (the
    mgcn_hatt_* entries, which take ``noise, T`` after ``act``)."""
    hard = T is not None
    fwd_name, softmax_name = ("hatt_fwd", "hatt_edge_softmax") if hard else ("att_fwd",
                                                                             "edge_softmax")
    noise_T = (L.ptr(noise), T) if hard else ()
    lib = L.load()
    dev = Hp.device
    N, HC = Hp.shape
    C = HC // H
    nnz = plan.nnz
    st = L.stream_of(dev)
    bf = Hp.dtype == BF16
    att = att.detach().contiguous()
    s_src = torch.empty(N, H, dtype=torch.float32, device=dev)
    s_dst = torch.empty(N, H, dtype=torch.float32, device=dev)
    Y = torch.empty(N, HC, dtype=Hp.dtype, device=dev)
    alpha = torch.empty(nnz, H, dtype=torch.float32, device=dev)
    fwd, bwd = plan.fwd, plan.bwd
    _row_launch(lib, "att_scores", bf, dev, N, None,
                N, H, C, L.ptr(Hp), Hp.stride(0), L.ptr(att), L.ptr(s_src), L.ptr(s_dst), st)
    if att_dir == 'in' or nnz == 0:
        _view_launch(lib, fwd_name, bf, dev, N, fwd, nnz, H, True,
                     N, nnz, H, C, L.ptr(fwd.rowptr), L.ptr(fwd.col), L.ptr(s_dst),
                     L.ptr(s_src), act, *noise_T, None, L.ptr(mask), L.ptr(Hp), Hp.stride(0),
                     L.ptr(Y), HC, L.ptr(alpha), st)
    else:
        a_bwd = torch.empty(nnz, H, dtype=torch.float32, device=dev)
        _view_launch(lib, softmax_name, False, dev, N, bwd, nnz, H, False,
                     N, nnz, H, L.ptr(bwd.rowptr), L.ptr(bwd.col), L.ptr(s_src),
                     L.ptr(s_dst), act, *noise_T, L.ptr(a_bwd), st, bf16_rows=bf)
        alpha[plan.slot_map()[:nnz].long()] = a_bwd
        _view_launch(lib, fwd_name, bf, dev, N, fwd, nnz, H, True,
                     N, nnz, H, C, L.ptr(fwd.rowptr), L.ptr(fwd.col), None, None, act,
                     *((None, T) if hard else ()), L.ptr(alpha), L.ptr(mask), L.ptr(Hp),
                     Hp.stride(0), L.ptr(Y), HC, None, st)
    ctx.plan, ctx.H, ctx.act, ctx.att_dir, ctx.T = plan, H, act, att_dir, T
    ctx.save_for_backward(Hp, att, alpha, mask, s_src, s_dst)
    ctx.mark_non_differentiable(alpha)
    return Y, alpha


def _train_backward(ctx, dY):
    """``(dHp, datt)`` of either training function (``ctx.T`` None: soft):
    mgcn_(h)att_bwd_dst, mgcn_(h)att_bwd_src and, for 'out', mgcn_att_dst_fold.
    bf16 rows under 'out' hand the unrounded fp32 row from bwd_src to the fold
    through a scratch [N, H C], so dHp is rounded once."""
    Hp, att, alpha, mask, s_src, s_dst = ctx.saved_tensors
    plan, H, act, T = ctx.plan, ctx.H, ctx.act, ctx.T
    pre, temp = ("att_", ()) if T is None else ("hatt_", (T,))
    lib = L.load()
    dev = Hp.device
    N, HC = Hp.shape
    C = HC // H
    nnz = plan.nnz
    st = L.stream_of(dev)
    bf = Hp.dtype == BF16
    dY = _grad_rows(dY, Hp.dtype)
    fwd, bwd = plan.fwd, plan.bwd
    dz = torch.empty(nnz, H, dtype=torch.float32, device=dev)
    ds_src = torch.empty(N, H, dtype=torch.float32, device=dev)
    ds_dst = torch.empty(N, H, dtype=torch.float32, device=dev)
    inn = ctx.att_dir == 'in'
    _view_launch(lib, pre + "bwd_dst", bf, dev, N, fwd, nnz, H, False,
                 N, nnz, H, C, L.ptr(fwd.rowptr), L.ptr(fwd.col), L.ptr(Hp), Hp.stride(0),
                 L.ptr(dY), dY.stride(0), L.ptr(alpha), L.ptr(mask), L.ptr(s_dst),
                 L.ptr(s_src), act, int(inn), *temp, L.ptr(dz), L.ptr(ds_dst), st)
    slot = plan.slot_map() if nnz else None
    dHp = torch.empty(N, HC, dtype=dY.dtype, device=dev)
    park = torch.empty(N, HC, dtype=torch.float32, device=dev) if bf and not inn else None
    _view_launch(lib, pre + "bwd_src", bf, dev, N, bwd, nnz, H, True,
                 N, nnz, H, C, L.ptr(bwd.rowptr), L.ptr(bwd.col), L.ptr(slot), L.ptr(dY),
                 dY.stride(0), L.ptr(alpha), L.ptr(mask), L.ptr(dz), L.ptr(s_src), L.ptr(s_dst),
                 act, int(not inn), *temp, L.ptr(att), L.ptr(ds_dst) if inn else None,
                 L.ptr(ds_src), L.ptr(dHp), HC, *((L.ptr(park),) if bf else ()), st)
    if not inn:
        _row_launch(lib, "att_dst_fold", bf, dev, N, fwd.edges,
                    N, nnz, H, C, L.ptr(fwd.rowptr), L.ptr(dz), L.ptr(att), L.ptr(ds_dst),
                    *((L.ptr(park),) if bf else ()), L.ptr(dHp), HC, st)
    datt = _datt(ds_src, ds_dst, Hp, H, C) if ctx.needs_input_grad[1] else None
    return dHp, datt


class _AttentionAggregate(torch.autograd.Function):
    """The message passing of NodeModelAttention after its ``x @ W``
    (graph_attention.py:66-100) on libmgcn's attention kernels.

    Forward: mgcn_att_scores, then for 'in' one mgcn_att_fwd launch (logits,
    softmax by destination, weighted gather); for 'out' mgcn_edge_softmax over
    the source-grouped view, alpha carried to fwd slot order, mgcn_att_fwd in
    its aggregate-only mode.  Saved: Hp, alpha (fwd slot order, before the
    dropout mask), the slot-order mask, s_src / s_dst.  Backward:
    mgcn_att_bwd_dst, mgcn_att_bwd_src (+ mgcn_att_dst_fold for 'out'), and the
    attention vector's gradient as one mgcn_gemm_tn ([ds_src | ds_dst]^T Hp,
    of which head h's own C columns are its rows of da).  bf16 ``Hp``: the
    ``_bf16`` sibling of every launch but mgcn_edge_softmax; Y, the saved Hp
    and dHp are bf16."""

    @staticmethod
    def forward(ctx, Hp, att, mask, plan: GraphPlan, H: int, act: int, att_dir: str):
        return _train_forward(ctx, Hp, att, mask, None, None, plan, H, act, att_dir)

    @staticmethod
    def backward(ctx, dY, _dalpha):
        return (*_train_backward(ctx, dY), None, None, None, None, None)


def _check_args(who: str, Hp, att_weight, plan: GraphPlan, nheads: int, act: str, att_dir: str,
                *others):
    """The argument checks :func:`attention_aggregate` and
    :func:`hard_attention_aggregate` (``who``) share; ``others``: further
    tensors that must live on Hp's device.  Returns the rows [N, H C], the
    fp32 attention vector [H, 2C] and H."""
    _require_row_dtype(Hp, "Hp")
    L.require_device(Hp, att_weight, plan.fwd.rowptr,
                     *(t for t in others if not isinstance(t, (DeviceGumbel, DeviceDropout))))
    if act not in L.ATT_ACT_CODES:
        raise ValueError(f"act must be one of none/lrelu/relu, got {act!r}")
    if att_dir not in ('in', 'out'):
        raise ValueError(f"att_dir must be 'in' or 'out', got {att_dir!r}")
    H = int(nheads)
    Hp2 = _rows(Hp.reshape(Hp.size(0), -1), "Hp")
    if Hp2.size(0) != plan.num_nodes:
        raise ValueError(f"Hp has {Hp2.size(0)} rows, graph has {plan.num_nodes} nodes")
    HC = Hp2.size(1)
    if H < 1 or HC % H:
        raise ValueError(f"Hp width {HC} is not a multiple of nheads = {H}")
    C = HC // H
    att2 = _att_f32(att_weight, H, C)
    if not (1 <= H <= 16 and HC <= 1024 and plan.nnz * H < 2 ** 31):
        raise L.MgcnError(f"{who}: unsupported shape (H = {H}, C = {C}, nnz = "
                          f"{plan.nnz}): need 1 <= H <= 16, H C <= 1024, nnz H < 2^31")
    return Hp2, att2, H


def _slot_mask(edge_mask, plan: GraphPlan, H: int):
    """``edge_mask`` [E, H] (COO order; None stays None) as fp32 in fwd slot
    order; a :class:`DeviceDropout` is generated in that order."""
    if edge_mask is None:
        return None
    if isinstance(edge_mask, DeviceDropout):
        return edge_noise(plan, H, L.NOISE_DROPOUT, seed=edge_mask.seed, offset=edge_mask.offset,
                          p=edge_mask.p, order='fwd')
    if tuple(edge_mask.shape) != (plan.nnz, H):
        raise ValueError(f"edge_mask must be [{plan.nnz}, {H}] in COO order, got "
                         f"{tuple(edge_mask.shape)}")
    return edge_mask.detach().to(torch.float32)[plan.fwd.eid.long()].contiguous()


def _alpha_coo(alpha, mask, plan: GraphPlan):
    """alpha' = alpha * mask, detached, carried from fwd slot order to COO order."""
    alpha = alpha.detach()
    alpha_coo = torch.empty_like(alpha)
    if plan.nnz:
        alpha_coo[plan.fwd.eid.long()] = alpha * mask if mask is not None else alpha
    return alpha_coo


def attention_aggregate(Hp: torch.Tensor, att_weight: torch.Tensor, plan: GraphPlan, nheads: int,
                        act: str = 'none', att_dir: str = 'in',
                        edge_mask: torch.Tensor | DeviceDropout | None = None):
    """Multi-head soft attention over each node's neighbourhood
    (graph_attention.py:66-100 + the softmax of common.py:69-92), fused:

    ``Hp`` [N, H * C] (or [N, H, C]) are the transformed features, ``att_weight``
    [1, H, 2C] (or [H, 2C]) the attention vector, ``act`` in none / lrelu /
    relu, ``att_dir`` 'in' (softmax over the edges into a node) or 'out' (over
    the edges out of it).  ``edge_mask`` [E, H], in COO edge order, multiplies
    the attention coefficients (the dropout mask with its 1 / (1 - p) scale);
    a :class:`mgcn.ops.DeviceDropout` instead of a tensor has that mask made
    by one ``mgcn_edge_noise`` launch, directly in the order the kernels read.

    Returns ``(Y, alpha_coo)``: Y [N, H * C] = sum over in-edges of alpha' *
    Hp[src], and alpha' = alpha * mask as [E, H] in COO order, detached.
    Differentiable in Hp and att_weight.  CPU tensors raise: no CPU path.

    ``Hp`` is float32 or bfloat16 (any other dtype: ``TypeError``).  For a
    bfloat16 ``Hp`` the feature rows stay bf16 through every kernel and Y and
    the gradient of Hp are bf16; alpha stays fp32.  ``att_weight`` may be
    float32 or bfloat16 with either (its gradient has its dtype)."""
    Hp2, att2, H = _check_args("attention_aggregate", Hp, att_weight, plan, nheads, act, att_dir,
                               edge_mask)
    mask = _slot_mask(edge_mask, plan, H)
    Y, alpha = _AttentionAggregate.apply(Hp2, att2, mask, plan, H, L.ATT_ACT_CODES[act], att_dir)
    return Y, _alpha_coo(alpha, mask, plan)


# ---------------------------------------------------------- hard attention
class _HardAttentionTrain(torch.autograd.Function):
    """The training branch of NodeModelHardAttention / VotePoolLayer after
    ``x @ W`` (graph_hard_attention.py:82-103): soft attention whose logit is
    (act(z) + noise) / T, on the mgcn_hatt_* instantiations of the attention
    kernels.  Launches, saved tensors and the backward are those of
    :class:`_AttentionAggregate` (the noise is not saved: act' needs z alone);
    ``noise`` is in the slot order of the view the softmax walks."""

    @staticmethod
    def forward(ctx, Hp, att, mask, noise, plan: GraphPlan, H: int, act: int, att_dir: str,
                T: float):
        return _train_forward(ctx, Hp, att, mask, noise, T, plan, H, act, att_dir)

    @staticmethod
    def backward(ctx, dY, _dalpha):
        return (*_train_backward(ctx, dY), None, None, None, None, None, None, None)


class _HardAttentionEval(torch.autograd.Function):
    """The eval branch (graph_hard_attention.py:105-139): per-(group, head)
    argmax, the reference's one-hot including its last-edge quirk, and the
    gather that reads one row per winner.

    Forward: mgcn_att_scores, mgcn_hatt_select over the view whose rows are the
    softmax groups ('out': the bwd view, the one-hot carried to fwd slot order
    through the slot map), the quirk on the one-hot, mgcn_hatt_gather.  Saved:
    the one-hot (fwd slot order) and the attention vector (only as the
    finite multiplier of a zero ds).  Backward: dHp[j] = sum_k alpha_k dY[i]
    through mgcn_att_bwd_src with a zero dz; nothing flows to att_weight."""

    @staticmethod
    def forward(ctx, Hp, att, noise, plan: GraphPlan, H: int, act: int, att_dir: str):
        lib = L.load()
        dev = Hp.device
        N, HC = Hp.shape
        C = HC // H
        nnz = plan.nnz
        st = L.stream_of(dev)
        bf = Hp.dtype == BF16
        att = att.detach().contiguous()
        s_src = torch.empty(N, H, dtype=torch.float32, device=dev)
        s_dst = torch.empty(N, H, dtype=torch.float32, device=dev)
        Y = torch.empty(N, HC, dtype=Hp.dtype, device=dev)
        alpha = torch.empty(nnz, H, dtype=torch.float32, device=dev)
        winner = torch.empty(N, H, dtype=torch.int32, device=dev)
        fwd, bwd = plan.fwd, plan.bwd
        _row_launch(lib, "att_scores", bf, dev, N, None,
                    N, H, C, L.ptr(Hp), Hp.stride(0), L.ptr(att), L.ptr(s_src), L.ptr(s_dst), st)
        if att_dir == 'in':
            launch("hatt_select", "mgcn_hatt_select", dev, N, fwd.edges, lib.mgcn_hatt_select,
                   N, nnz, H, L.ptr(fwd.rowptr), L.ptr(fwd.col), L.ptr(s_dst), L.ptr(s_src), act,
                   L.ptr(noise), L.ptr(alpha), L.ptr(winner), st)
        else:
            a_bwd = torch.empty(nnz, H, dtype=torch.float32, device=dev)
            launch("hatt_select", "mgcn_hatt_select", dev, N, bwd.edges, lib.mgcn_hatt_select,
                   N, nnz, H, L.ptr(bwd.rowptr), L.ptr(bwd.col), L.ptr(s_src), L.ptr(s_dst), act,
                   L.ptr(noise), L.ptr(a_bwd), L.ptr(winner), st)
            if nnz:
                alpha[plan.slot_map()[:nnz].long()] = a_bwd
        if nnz:
            # graph_hard_attention.py:118-123: an argmax of -1 (a group without a
            # winner) indexes the transposed flat one-hot at E h - 1, which is COO
            # edge E - 1 of head h - 1 (head 0: of the last head)
            mark = (winner < 0).any(dim=0).roll(-1).to(torch.float32)
            last = plan.last_edge_slot()  # cached on the plan: no scan, no host sync
            alpha[last] = torch.maximum(alpha[last], mark)
        _row_launch(lib, "hatt_gather", bf, dev, N, fwd.edges,
                    N, nnz, H, C, L.ptr(fwd.rowptr), L.ptr(fwd.col), L.ptr(alpha), L.ptr(Hp),
                    Hp.stride(0), L.ptr(Y), HC, st)
        ctx.plan, ctx.H, ctx.row_dtype = plan, H, Hp.dtype
        ctx.save_for_backward(alpha, att)
        ctx.mark_non_differentiable(alpha)
        return Y, alpha

    @staticmethod
    def backward(ctx, dY, _dalpha):
        alpha, att = ctx.saved_tensors
        plan, H = ctx.plan, ctx.H
        lib = L.load()
        dev = alpha.device
        N, nnz = plan.num_nodes, plan.nnz
        bf = ctx.row_dtype == BF16
        dY = _grad_rows(dY, ctx.row_dtype)
        HC = dY.size(1)
        bwd = plan.bwd
        slot = plan.slot_map() if nnz else None
        dz = torch.zeros(nnz, H, dtype=torch.float32, device=dev)
        ds_src = torch.empty(N, H, dtype=torch.float32, device=dev)
        dHp = torch.empty(N, HC, dtype=dY.dtype, device=dev)
        _view_launch(lib, "att_bwd_src", bf, dev, N, bwd, nnz, H, True,
                     N, nnz, H, HC // H, L.ptr(bwd.rowptr), L.ptr(bwd.col), L.ptr(slot), L.ptr(dY),
                     dY.stride(0), L.ptr(alpha), None, L.ptr(dz), None, None, 0, 0, L.ptr(att),
                     None, L.ptr(ds_src), L.ptr(dHp), HC, *((None,) if bf else ()),
                     L.stream_of(dev))
        return dHp, None, None, None, None, None, None


def hard_attention_aggregate(Hp: torch.Tensor, att_weight: torch.Tensor, plan: GraphPlan,
                             nheads: int, act: str = 'none', att_dir: str = 'in',
                             temperature: float = 0.1, *, training: bool,
                             noise: torch.Tensor | DeviceGumbel | None = None,
                             edge_mask: torch.Tensor | DeviceDropout | None = None):
    """Multi-head hard attention over each node's neighbourhood
    (graph_hard_attention.py:82-139), fused.  Arguments as for
    :func:`attention_aggregate`, plus:

    ``training=True``: Gumbel-softmax.  The logit of an edge is
    ``(act(z) + noise) / temperature``; ``noise`` [E, H] in COO edge order
    (None: zeros).  Differentiable in Hp and att_weight.

    ``training=False``: every (group, head) keeps the one edge with the largest
    ``act(z) + noise`` (``noise`` None: the plain argmax; given: the reference's
    ``sample=True``), ties going to the last edge in COO order.  If any group
    has no winner, COO edge E - 1 is selected too (on every head when the group
    is empty), as the reference's flat indexing with argmax = -1 does.
    Differentiable in Hp only; ``att_weight`` receives no gradient and
    ``edge_mask`` is not used (the reference drops out in training alone).

    ``noise`` may be a :class:`mgcn.ops.DeviceGumbel` and ``edge_mask`` a
    :class:`mgcn.ops.DeviceDropout` instead of tensors: each is then made by
    one ``mgcn_edge_noise`` launch in the slot order its kernel reads (the
    walked view for the noise, fwd for the mask), with the values
    :func:`mgcn.ops.edge_noise` gives in COO order under the same seed and
    offset, and no COO tensor or permutation in between.

    Returns ``(Y, alpha_coo)``: Y [N, H * C] and the coefficients that weighted
    the messages, [E, H] in COO order, detached.  ``Hp`` float32 or bfloat16 as
    for :func:`attention_aggregate`."""
    Hp2, att2, H = _check_args("hard_attention_aggregate", Hp, att_weight, plan, nheads, act,
                               att_dir, edge_mask, noise)
    T = float(temperature)
    if training and not T > 0:
        raise ValueError(f"temperature must be positive, got {temperature!r}")
    # the view whose rows are the softmax / argmax groups
    walked = plan.fwd if att_dir == 'in' or (training and plan.nnz == 0) else plan.bwd
    if isinstance(noise, DeviceGumbel):
        noise = edge_noise(plan, H, L.NOISE_GUMBEL, seed=noise.seed, offset=noise.offset,
                           order='fwd' if walked is plan.fwd else 'bwd')
    elif noise is not None:
        if tuple(noise.shape) != (plan.nnz, H):
            raise ValueError(f"noise must be [{plan.nnz}, {H}] in COO order, got "
                             f"{tuple(noise.shape)}")
        noise = noise.detach().to(torch.float32)[walked.eid.long()].contiguous()
    mask = None
    if training:
        mask = _slot_mask(edge_mask, plan, H)
        Y, alpha = _HardAttentionTrain.apply(Hp2, att2, mask, noise, plan, H,
                                             L.ATT_ACT_CODES[act], att_dir, T)
    else:
        Y, alpha = _HardAttentionEval.apply(Hp2, att2.detach(), noise, plan, H,
                                            L.ATT_ACT_CODES[act], att_dir)
    return Y, _alpha_coo(alpha, mask, plan)
