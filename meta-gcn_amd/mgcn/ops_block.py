"""Mini-batch blocks: the sampled multi-hop frontier of a list of seed nodes,
one small square plan per layer, built on the device in time proportional to
the frontier (``mgcn_block_count`` / ``mgcn_block_fill`` / ``mgcn_block_relabel``,
include/mgcn.h).  Depends on :mod:`mgcn._call`, :mod:`mgcn.graph`,
:mod:`mgcn.ops_noise` and :mod:`mgcn.ops_sample`; :mod:`mgcn.ops` re-exports
every name.

Frontiers grow from the seeds outwards: ``F_L = seeds``; for ``l = L-1 .. 0``
the destinations ``D = F_{l+1}`` keep the edges of
``sample_keep(parent, fanouts[l], seed=, offset=offset + l, rows=mask(D))``,
ordered by (position of the destination in ``D``, parent COO id), and
``F_l`` is ``D`` followed by the other sources in ascending id.  A node's local
id is its position in ``F_l``, so one layer's output rows are the next
layer's input rows::

    h = x[blocks[0].src_ids]
    for l, conv in enumerate(convs):
        h = conv(h, blocks[l])  # or conv(h, blocks[l].edge_index)[:blocks[l].n_dst]

(:mod:`mgcn.ops_block_conv` has what a conv does with a block).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import torch

from . import _lib as L
from ._call import launch, workspace
from .graph import CSRView, GraphPlan, _same_device, adopt_plan, build_view, schedule_rows
from .ops_noise import draw_edge_seed
from .ops_sample import _FANOUT_MAX, _fanout, _u64


@dataclass
class Block:
    """One layer of a mini-batch: ``plan`` is square over ``n_src`` nodes, its
    rows ``>= n_dst`` empty; local id ``i`` is parent node ``src_ids[i]`` and
    the first ``n_dst`` of them are the layer's destinations; block edge ``p``
    is parent COO edge ``parent_eid[p]``."""
    plan: GraphPlan
    n_dst: int
    n_src: int
    src_ids: torch.Tensor      # int64 [n_src]
    parent_eid: torch.Tensor   # int64 [nnz_b]
    _coo: torch.Tensor = field(repr=False, default=None)  # int64 [2, nnz_b], local ids
    _adopted: bool = field(repr=False, default=False)

    @property
    def edge_index(self) -> torch.Tensor:
        """int64 [2, nnz_b] in local ids, held by the block; ``plan_for`` of it
        (with ``n_src`` nodes) is ``plan`` while the block is alive."""
        if not self._adopted:
            adopt_plan(self._coo, self.n_src, self.plan)
            self._adopted = True
        return self._coo


def _seed_list(plan: GraphPlan, seeds) -> tuple[torch.Tensor, bool]:
    """The int32 destination list of the outermost hop and whether its ids need
    the device's range / repeat checks (a mask's ids need none)."""
    n = plan.num_nodes
    if not isinstance(seeds, torch.Tensor):
        raise ValueError(f"seeds must be a 1-d int64 / int32 tensor of node ids or a bool "
                         f"[{n}] mask, got {type(seeds).__name__}")
    if seeds.dtype == torch.bool:
        if seeds.dim() != 1 or seeds.numel() != n:
            raise ValueError(f"seeds: a bool mask must have shape ({n},), got "
                             f"{tuple(seeds.shape)}")
        _same_device(plan, seeds)
        return seeds.nonzero().view(-1).to(torch.int32), False
    if seeds.dtype not in (torch.int64, torch.int32) or seeds.dim() != 1:
        raise ValueError(f"seeds must be a 1-d int64 / int32 tensor of node ids or a bool "
                         f"[{n}] mask, got {seeds.dtype} {tuple(seeds.shape)}")
    _same_device(plan, seeds)
    # an id outside int32 stays outside [0, n) for the device's check
    return seeds.clamp(-1, n).to(torch.int32).contiguous(), True


def _empty_block(plan: GraphPlan) -> Block:
    dev = plan.device

    def view():
        return CSRView(rowptr=torch.zeros(1, dtype=torch.int64, device=dev),
                       col=torch.empty(0, dtype=torch.int32, device=dev),
                       eid=torch.empty(0, dtype=torch.int32, device=dev), n_rows=0, n_cols=0)
    empty = GraphPlan(num_nodes=0, nnz=0, device=dev, fwd=view(), bwd=view(),
                      in_cnt=torch.empty(0, dtype=torch.float32, device=dev))
    return Block(plan=empty, n_dst=0, n_src=0,
                 src_ids=torch.empty(0, dtype=torch.int64, device=dev),
                 parent_eid=torch.empty(0, dtype=torch.int64, device=dev),
                 _coo=torch.empty(2, 0, dtype=torch.int64, device=dev))


def _hop(plan: GraphPlan, dst: torch.Tensor, k: int, seed: int, offset: int, keep_loops: bool,
         validate: bool) -> Block:
    """One block: the destinations ``dst`` (int32, on the plan's device) under
    the cap ``k``.  Two host waits of its own, for (edge count, long rows, id
    checks) and for the node count."""
    n_dst = int(dst.numel())
    if n_dst == 0:
        return _empty_block(plan)
    lib = L.load()
    view = plan.fwd
    dev = L.require_device(view.rowptr)
    n, nnz = plan.num_nodes, plan.nnz
    stream = L.stream_of(dev)
    ws, ws_bytes = workspace(lib.mgcn_block_workspace_bytes(n, n_dst), dev)
    node_map = torch.empty(n, dtype=torch.int32, device=dev)
    rowptr = torch.empty(n_dst + 1, dtype=torch.int64, device=dev)
    meta = torch.empty(5, dtype=torch.int64, device=dev)
    graph = (n, nnz, L.ptr(view.rowptr), L.ptr(view.col))
    launch("block_count", "mgcn_block_count", dev, n_dst, 0, lib.mgcn_block_count, *graph,
           L.ptr(dst), n_dst, k, int(keep_loops), L.ptr(node_map), L.ptr(rowptr), L.ptr(meta),
           L.ptr(ws), ws_bytes, stream)
    nnz_b, n_heavy, out_of_range, repeated, _ = meta.tolist()  # host wait 1
    if validate and out_of_range:
        raise ValueError(f"sample_blocks: seed id out of range (expected 0 <= id < {n})")
    if (validate and repeated) or not 0 <= nnz_b <= nnz:
        raise ValueError("sample_blocks: repeated seed id")
    src_g = torch.empty(nnz_b, dtype=torch.int32, device=dev)
    peid = torch.empty(nnz_b, dtype=torch.int32, device=dev)
    coo = torch.empty(2, nnz_b, dtype=torch.int64, device=dev)
    launch("block_fill_heavy" if n_heavy else "block_fill", "mgcn_block_fill", dev, n_dst, nnz_b,
           lib.mgcn_block_fill, *graph, L.ptr(view.eid), L.ptr(dst), n_dst, k, int(keep_loops),
           seed, offset, L.ptr(rowptr), nnz_b, n_heavy, L.ptr(node_map), L.ptr(src_g),
           L.ptr(peid), L.ptr(coo[1]), L.ptr(meta), L.ptr(ws), ws_bytes, stream)
    n_src = n_dst + int(meta[4])  # host wait 2
    src_ids = torch.empty(n_src, dtype=torch.int64, device=dev)
    col = torch.empty(nnz_b, dtype=torch.int32, device=dev)
    launch("block_relabel", "mgcn_block_relabel", dev, n_src, nnz_b, lib.mgcn_block_relabel, n,
           L.ptr(dst), n_dst, n_src, nnz_b, L.ptr(src_g), L.ptr(node_map), L.ptr(src_ids),
           L.ptr(col), L.ptr(coo[0]), L.ptr(ws), ws_bytes, stream)
    # the fwd view needs no sort: the edges are in slot order, and the rows
    # past the destinations repeat the last row pointer
    fwd = CSRView(rowptr=torch.cat([rowptr, rowptr[-1:].expand(n_src - n_dst)]), col=col,
                  eid=torch.arange(nnz_b, dtype=torch.int32, device=dev), n_rows=n_src,
                  n_cols=n_src)
    fwd = schedule_rows(fwd)
    bwd = build_view(coo[0], coo[1], n_src, n_src)
    in_cnt = (fwd.rowptr[1:] - fwd.rowptr[:-1]).clamp_(min=1).to(torch.float32)
    block_plan = GraphPlan(num_nodes=n_src, nnz=nnz_b, device=dev, fwd=fwd, bwd=bwd,
                           in_cnt=in_cnt)
    return Block(plan=block_plan, n_dst=n_dst, n_src=n_src, src_ids=src_ids,
                 parent_eid=peid.long(), _coo=coo)


def sample_blocks(plan: GraphPlan, seeds: torch.Tensor, fanouts, *, seed: int | None = None,
                  offset: int = 0, keep_loops: bool = True, validate: bool = True) -> list:
    """The mini-batch blocks of ``seeds`` (distinct node ids in any order, int64
    or int32 on the plan's device, or a bool [num_nodes] mask: its ids
    ascending): one :class:`Block` per entry of ``fanouts``, ``blocks[0]`` the
    input layer.  Layer ``l`` is drawn under ``(seed, offset + l)`` with
    :func:`mgcn.ops_sample.sample_keep`'s definition; ``seed=None`` draws one
    :func:`draw_edge_seed` pair per call.  Ids out of range or repeated raise
    ValueError (``validate=False``: the caller vouches for them).  Each hop
    costs time proportional to its frontier plus a few passes over node-sized
    arrays, never one over the parent's edges."""
    ks = [min(_fanout(f), _FANOUT_MAX) for f in fanouts]
    if seed is None:
        seed, offset = draw_edge_seed()
    seed, offset = _u64(seed, "seed"), _u64(offset, "offset")
    _u64(offset + max(len(ks) - 1, 0), "offset + layer")
    dst, check = _seed_list(plan, seeds)
    blocks: list = [None] * len(ks)
    for l in range(len(ks) - 1, -1, -1):
        blocks[l] = _hop(plan, dst, ks[l], seed, offset + l, bool(keep_loops),
                         validate and check)
        dst, check = blocks[l].src_ids.to(torch.int32), False
    return blocks


def block_batches(plan: GraphPlan, ids: torch.Tensor, batch_size: int, fanouts, *,
                  shuffle: bool = True, generator: torch.Generator | None = None,
                  keep_loops: bool = True):
    """One epoch of mini-batches over ``ids`` (a 1-d tensor of distinct node
    ids on the plan's device): yields ``sample_blocks(plan, batch, fanouts)``
    for consecutive ``batch_size`` slices of ``ids``, permuted first with
    ``shuffle`` (a host permutation from ``generator``, default torch's global
    one).  Every batch draws its own seed pair from the same generator."""
    if isinstance(batch_size, bool) or not isinstance(batch_size, int) or batch_size < 1:
        raise ValueError(f"batch_size must be a positive integer, got {batch_size!r}")
    if not isinstance(ids, torch.Tensor) or ids.dim() != 1 or \
            ids.dtype not in (torch.int64, torch.int32):
        raise ValueError("ids must be a 1-d int64 / int32 tensor of node ids")
    if shuffle:
        perm = torch.randperm(int(ids.numel()), generator=generator, device="cpu")
        ids = ids[perm.to(ids.device)]
    for a in range(0, int(ids.numel()), batch_size):
        seed, offset = draw_edge_seed(generator)
        yield sample_blocks(plan, ids[a:a + batch_size], fanouts, seed=seed, offset=offset,
                            keep_loops=keep_loops)


__all__ = ["Block", "sample_blocks", "block_batches"]
