"""Neighbour sampling: a fan-out cap on every destination row, drawn on the
device from libmgcn's counter-based generator (``mgcn_sample_rows``,
include/mgcn.h), and the child plans derived from the masks.  Depends on
:mod:`mgcn._call`, :mod:`mgcn.graph` and :mod:`mgcn.ops_noise`; :mod:`mgcn.ops`
re-exports every name.

``keep[e]`` is a pure function of (graph, fanout, keep_loops, rows, seed,
offset): among the candidates of a destination row -- every edge, or with
``keep_loops`` every edge but the self loops, which are kept and not counted --
the ``fanout`` of smallest ``(key(e), e)`` stay, ``key(e)`` being the 32-bit
word whose top 24 bits are ``edge_noise(plan, 1, 'uniform', seed=, offset=)[e,
0]``.  Integers only, so the mask does not depend on slot order or on the
route a row takes."""
from __future__ import annotations

import operator
import os

import torch

from . import _lib as L
from ._call import launch, workspace
from .graph import GraphPlan, _same_device
from .ops_noise import draw_edge_seed

# one workgroup per heavy row of the fwd view's schedule (order[0, n_heavy));
# MGCN_SAMPLE_HEAVY=0 hands the entry no schedule: natural row order and a
# walk that finds the long rows.  The mask is the same either way.
_SAMPLE_HEAVY = os.environ.get("MGCN_SAMPLE_HEAVY", "1") != "0"
_LIGHT_MAX = 128  # slots of a lane-group row (sample.hip kLight)
_FANOUT_MAX = 2 ** 31 - 1  # a plan has fewer edges than that: a larger cap caps nothing


def set_sample_heavy_rows(enabled: bool) -> None:
    """Route the scheduled heavy rows of :func:`sample_keep` through the
    workgroup launch over the view's schedule (True, the default) or (False;
    env MGCN_SAMPLE_HEAVY=0) pass no schedule.  Results are bytewise the same."""
    global _SAMPLE_HEAVY
    _SAMPLE_HEAVY = bool(enabled)


def sample_heavy_rows() -> bool:
    """The switch :func:`set_sample_heavy_rows` sets."""
    return _SAMPLE_HEAVY


def _u64(v, name: str) -> int:
    try:
        v = operator.index(v)
    except TypeError:
        raise ValueError(f"{name} must be an integer in [0, 2^64), got {v!r}") from None
    if not 0 <= v < 2 ** 64:
        raise ValueError(f"{name} must be an integer in [0, 2^64), got {v}")
    return v


def _fanout(fanout) -> int:
    if isinstance(fanout, bool):
        raise ValueError(f"fanout must be a non-negative integer, got {fanout!r}")
    try:
        k = operator.index(fanout)
    except TypeError:
        raise ValueError(f"fanout must be a non-negative integer, got {fanout!r}") from None
    if k < 0:
        raise ValueError(f"fanout must be a non-negative integer, got {k}")
    return k


def _row_mask(plan: GraphPlan, rows):
    if rows is None:
        return None
    if not isinstance(rows, torch.Tensor) or rows.dtype != torch.bool or rows.dim() != 1 \
            or rows.numel() != plan.num_nodes:
        what = (f"{rows.dtype} {tuple(rows.shape)}" if isinstance(rows, torch.Tensor)
                else type(rows).__name__)
        raise ValueError(f"rows must be a bool [{plan.num_nodes}] mask, got {what}")
    _same_device(plan, rows)
    return rows.contiguous()


def sample_keep(plan: GraphPlan, fanout: int, *, seed: int, offset: int = 0,
                keep_loops: bool = True, rows: torch.Tensor | None = None) -> torch.Tensor:
    """The bool [nnz] keep mask (COO order) of a fan-out cap: one
    ``mgcn_sample_rows`` call on the plan's device.  ``rows``: a bool
    [num_nodes] mask of the destination rows that receive anything (the seed
    nodes of a mini-batch); the other rows keep nothing, loops included."""
    k = _fanout(fanout)
    seed, offset = _u64(seed, "seed"), _u64(offset, "offset")
    mask = _row_mask(plan, rows)
    view = plan.fwd
    dev = L.require_device(view.rowptr)
    if dev != plan.device:
        raise L.MgcnError(f"tensor on {dev}, graph is on {plan.device}")
    nnz = plan.nnz
    keep = torch.empty(nnz, dtype=torch.bool, device=dev)
    if nnz == 0:
        return keep
    # the lane groups hold rows of at most 128 slots: a schedule cut higher is not passed
    sched = _SAMPLE_HEAVY and view.order is not None and view.heavy_thr <= _LIGHT_MAX
    order, n_heavy = (view.order, view.n_heavy) if sched else (None, 0)
    lib = L.load()
    ws, ws_bytes = workspace(lib.mgcn_sample_rows_workspace_bytes(view.n_rows, nnz), dev,
                             or_null=True)
    launch("sample_rows_heavy" if n_heavy else "sample_rows", "mgcn_sample_rows", dev,
           view.n_rows, nnz, lib.mgcn_sample_rows, view.n_rows, nnz, L.ptr(view.rowptr),
           L.ptr(view.col), L.ptr(view.eid), L.ptr(order), n_heavy, L.ptr(mask),
           min(k, _FANOUT_MAX), int(bool(keep_loops)), seed, offset, L.ptr(keep), L.ptr(ws),
           ws_bytes, L.stream_of(dev))
    return keep


def sample_neighbors(plan: GraphPlan, fanout: int, *, seed: int | None = None, offset: int = 0,
                     keep_loops: bool = True, rows: torch.Tensor | None = None):
    """GraphSAGE's fan-out cap: every destination keeps at most ``fanout`` of
    its in-neighbours, a uniform sample without replacement (self loops kept on
    top with ``keep_loops``).  Returns ``(child_plan, keep)``: ``keep`` the bool
    [nnz] mask in COO order (:func:`sample_keep`), the child
    ``plan.select_edges(keep)`` -- one host wait, for the edge count.

    ``seed=None`` draws ``(seed, offset)`` with :func:`draw_edge_seed` (one draw
    per call, on the host: ``torch.manual_seed`` replays it); ``offset`` is read
    together with an explicit ``seed`` alone.  ``fanout >= plan.nnz`` with no
    ``rows`` caps nothing: the parent itself comes back, with a mask of ones."""
    k = _fanout(fanout)
    if seed is None:
        seed, offset = draw_edge_seed()
    seed, offset = _u64(seed, "seed"), _u64(offset, "offset")
    mask = _row_mask(plan, rows)
    if mask is None and k >= plan.nnz:
        return plan, torch.ones(plan.nnz, dtype=torch.bool, device=plan.device)
    keep = sample_keep(plan, k, seed=seed, offset=offset, keep_loops=keep_loops, rows=mask)
    return plan.select_edges(keep), keep


def sample_layers(plan: GraphPlan, fanouts, *, seed: int | None = None, offset: int = 0,
                  rows: torch.Tensor | None = None, keep_loops: bool = True) -> list:
    """One ``(plan, keep)`` per entry of ``fanouts``, each sampled from the
    parent (independent per-layer neighbourhoods): layer ``l`` under
    ``(seed, offset + l)``, or with ``seed=None`` under its own
    :func:`draw_edge_seed` pair."""
    ks = [_fanout(f) for f in fanouts]
    if seed is not None:
        seed, offset = _u64(seed, "seed"), _u64(offset, "offset")
        _u64(offset + max(len(ks) - 1, 0), "offset + layer")
    return [sample_neighbors(plan, k, seed=seed, offset=offset + l if seed is not None else 0,
                             keep_loops=keep_loops, rows=rows)
            for l, k in enumerate(ks)]


__all__ = ["sample_keep", "sample_neighbors", "sample_layers", "set_sample_heavy_rows",
           "sample_heavy_rows"]
