"""Seeded per-edge random tensors made on the device: the Gumbel noise of hard
attention / VotePool and the attention dropout mask, from libmgcn's
counter-based generator (``mgcn_edge_noise``, include/mgcn.h).  Depends on
:mod:`mgcn._call` and :mod:`mgcn.graph`; :mod:`mgcn.ops` re-exports every name.

A value is a pure function of (kind, seed, offset, COO edge id, head, p), so
the fill of a view's slot order is the COO fill carried to that order bit for
bit: the attention ops realise a :class:`DeviceGumbel` / :class:`DeviceDropout`
with one launch, directly in the order their kernels read, and make neither a
COO tensor nor a permutation."""
from __future__ import annotations

from dataclasses import dataclass

import torch

from . import _lib as L
from ._call import launch
from .graph import GraphPlan

NOISE_KINDS = {"uniform": L.NOISE_UNIFORM, "gumbel": L.NOISE_GUMBEL, "dropout": L.NOISE_DROPOUT}
_SEED_MAX = 2 ** 63 - 1


def _u63(v, name: str) -> int:
    v = int(v)
    if not 0 <= v <= _SEED_MAX:
        raise ValueError(f"{name} must be an integer in [0, 2^63), got {v}")
    return v


@dataclass(frozen=True)
class DeviceGumbel:
    """Gumbel(0, 1) noise [E, H] to be generated on the device under
    ``(seed, offset)``: the ``noise`` of :func:`mgcn.ops.hard_attention_aggregate`."""
    seed: int
    offset: int

    def __post_init__(self):
        _u63(self.seed, "seed"), _u63(self.offset, "offset")


@dataclass(frozen=True)
class DeviceDropout:
    """A dropout mask [E, H] (0 with probability ``p``, else 1 / (1 - p)) to be
    generated on the device under ``(seed, offset)``: the ``edge_mask`` of
    :func:`mgcn.ops.attention_aggregate` / ``hard_attention_aggregate``."""
    p: float
    seed: int
    offset: int

    def __post_init__(self):
        if not 0.0 <= float(self.p) <= 1.0:  # (NaN fails both comparisons)
            raise ValueError(f"dropout probability has to be between 0 and 1, got {self.p}")
        _u63(self.seed, "seed"), _u63(self.offset, "offset")


def draw_edge_seed(generator: torch.Generator | None = None) -> tuple[int, int]:
    """``(seed, offset)`` for one device tensor: two integers in [0, 2^63) read
    from torch's CPU generator (default: the global one), so
    ``torch.manual_seed(s)`` replays the stream of pairs and successive draws
    differ.  Two words on the host: no device is touched or waited for."""
    seed, offset = torch.randint(0, _SEED_MAX, (2,), dtype=torch.int64, device="cpu",
                                 generator=generator).tolist()
    return seed, offset


def edge_noise(plan: GraphPlan, nheads: int, kind, *, seed: int, offset: int,
               p: float | None = None, order: str = 'coo') -> torch.Tensor:
    """The fp32 [nnz, H] device tensor of ``kind`` ('uniform', 'gumbel' or
    'dropout', or the ``mgcn._lib.NOISE_*`` code) under ``(seed, offset)``, one
    ``mgcn_edge_noise`` launch on the plan's device.  ``order``: 'coo' (row e is
    COO edge e), 'fwd' or 'bwd' (row k is slot k of ``plan.fwd`` / ``plan.bwd``,
    i.e. the 'coo' tensor indexed by that view's ``eid``, bit for bit).  ``p``
    is the dropout probability ('dropout' alone, where it is required)."""
    code = NOISE_KINDS.get(kind, kind) if isinstance(kind, str) else kind
    if code not in NOISE_KINDS.values() or isinstance(code, bool):
        raise ValueError(f"kind must be one of uniform/gumbel/dropout, got {kind!r}")
    if order not in ('coo', 'fwd', 'bwd'):
        raise ValueError(f"order must be 'coo', 'fwd' or 'bwd', got {order!r}")
    if code == L.NOISE_DROPOUT:
        if p is None:
            raise ValueError("kind 'dropout' needs p")
    elif p is not None:
        raise ValueError(f"p is the dropout probability; kind {kind!r} takes none")
    seed, offset = _u63(seed, "seed"), _u63(offset, "offset")
    dev = L.require_device(plan.fwd.rowptr)
    H, nnz = int(nheads), plan.nnz
    eid = None if order == 'coo' else (plan.fwd if order == 'fwd' else plan.bwd).eid
    if not (1 <= H <= 16 and nnz * H < 2 ** 31):
        raise L.MgcnError(f"edge_noise: unsupported shape (H = {H}, nnz = {nnz}): need "
                          "1 <= H <= 16, nnz H < 2^31")
    out = torch.empty(nnz, H, dtype=torch.float32, device=dev)
    lib = L.load()
    launch("edge_noise", "mgcn_edge_noise", dev, nnz, None if eid is None else nnz,
           lib.mgcn_edge_noise, code, seed, offset, nnz, H, L.ptr(eid),
           0.0 if p is None else float(p), L.ptr(out), L.stream_of(dev))
    return out


__all__ = ["NOISE_KINDS", "DeviceGumbel", "DeviceDropout", "draw_edge_seed", "edge_noise"]
