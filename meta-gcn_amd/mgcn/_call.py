"""The one path every libmgcn launch of :mod:`mgcn.ops` and its ``ops_*``
modules takes: the kernel-timer hook, :func:`launch`, the workspace buffer
and the fp32 input normalisers.  Depends on :mod:`mgcn._lib` alone."""
from __future__ import annotations

import torch

from . import _lib as L

# optional callable(name, start: bool, rows=None, edges=None) called right
# before / after each libmgcn launch on its stream (bench.py's HIP-event timer);
# the start call carries the launch's row and edge counts for byte accounting
_TIMER = None


def set_kernel_timer(timer) -> None:
    """Install (or clear with None) a hook called right before and after each
    libmgcn launch, on the launch stream -- used to time kernels with events."""
    global _TIMER
    _TIMER = timer


def launch(tname, sym: str, dev: torch.device, rows, edges, fn, *args) -> None:
    """``fn(*args)``, one libmgcn entry point, on ``dev``: inside the device
    guard, bracketed by the kernel timer's start ``(tname, True, rows, edges)``
    and stop ``(tname, False)`` when a timer is installed and ``tname`` is not
    None (an untimed launch), then :func:`mgcn._lib.check` under the C symbol
    ``sym``.  The stop is recorded before a failed call raises."""
    timer = _TIMER if tname is not None else None
    with L.device_guard(dev):
        if timer is not None:
            timer(tname, True, rows, edges)
        rc = fn(*args)
        if timer is not None:
            timer(tname, False)
    L.check(rc, sym)


def workspace(nbytes, dev: torch.device, or_null: bool = False):
    """(buffer, byte count) for a ``*_workspace_bytes`` answer: a uint8 tensor
    of at least one byte, or None for an empty workspace with ``or_null`` (the
    entry points that take NULL for it)."""
    nbytes = int(nbytes)
    if or_null and not nbytes:
        return None, 0
    return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev), nbytes


def _contig_f32(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32 (the reference computes in fp32), got {t.dtype}")
    if t.dim() != 2:
        raise ValueError(f"{name} must be 2-D [N, F], got {tuple(t.shape)}")
    if t.stride(1) != 1 or t.stride(0) < t.size(1):
        t = t.contiguous()
    return t


def _aligned_rows(t: torch.Tensor, name: str = "x") -> torch.Tensor:
    """:func:`_contig_f32` with 16-byte aligned rows (the kernels' float4 accesses)."""
    t = _contig_f32(t, name)
    if t.stride(0) % 4 or t.data_ptr() % 16:
        t = t.contiguous()
    return t
