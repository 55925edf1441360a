"""Segment means and the packed (zero-skipping) exchange tables on libmgcn.
Sits on :mod:`mgcn._call`; :mod:`mgcn.ops` re-exports every name."""
from __future__ import annotations

from dataclasses import dataclass

import torch

from . import _lib as L
from ._call import _contig_f32, launch, workspace


def segment_mean(x: torch.Tensor, ptr: torch.Tensor) -> torch.Tensor:
    """Mean of contiguous row segments [ptr[g], ptr[g+1]) (global_mean_pool)."""
    return _SegmentMean.apply(x, ptr)


class _SegmentMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ptr):
        lib = L.load()
        x = _contig_f32(x, "x")
        ptr = ptr.to(torch.int64).contiguous()
        dev = L.require_device(x, ptr)
        G = ptr.numel() - 1
        out = torch.empty(G, x.size(1), dtype=torch.float32, device=dev)
        launch(None, "mgcn_segment_mean", dev, None, None, lib.mgcn_segment_mean,
               G, x.size(1), L.ptr(ptr), L.ptr(x), x.stride(0), L.ptr(out), out.stride(0),
               L.stream_of(dev))
        ctx.save_for_backward(ptr)
        ctx.n = x.size(0)
        return out

    @staticmethod
    def backward(ctx, dout):
        (ptr,) = ctx.saved_tensors
        counts = (ptr[1:] - ptr[:-1])
        seg = torch.repeat_interleave(torch.arange(counts.numel(), device=ptr.device), counts,
                                      output_size=ctx.n)
        scale = counts.clamp(min=1).to(dout.dtype)
        return (dout / scale.unsqueeze(1))[seg], None


# ------------------------------------------------- packed table exchange
def pack_rows_count(rows: torch.Tensor, hdr: torch.Tensor, counts: torch.Tensor) -> None:
    """hdr[i, 2 w] = mask word w of rows[i] (its not-+0.0 bits), counts[i] =
    their number (``mgcn_pack_rows_count``; mgcn.dist's packed exchange).
    ``hdr`` is the [n, 2 F/32] int32 header of the packed chunk."""
    lib = L.load()
    rows = _contig_f32(rows, "rows")
    n, F = rows.shape
    dev = L.require_device(rows, hdr, counts)
    if hdr.shape != (n, 2 * (F // 32)) or hdr.dtype != torch.int32 or not hdr.is_contiguous() \
            or counts.shape != (n,) or counts.dtype != torch.int32:
        raise ValueError("pack_rows_count: hdr int32 [n, 2 F/32] contiguous, counts int32 [n]")
    launch("pack_rows_count", "mgcn_pack_rows_count", dev, n, None, lib.mgcn_pack_rows_count,
           n, F, L.ptr(rows), rows.stride(0), L.ptr(hdr), L.ptr(counts), L.stream_of(dev))


def pack_rows_values(rows: torch.Tensor, offs: torch.Tensor, hdr: torch.Tensor,
                     vals: torch.Tensor) -> None:
    """vals[offs[i] ...] = the not-+0.0 words of rows[i] in order, and the
    header's value positions hdr[i, 2 w + 1] (``mgcn_pack_rows_values``)."""
    lib = L.load()
    rows = _contig_f32(rows, "rows")
    n, F = rows.shape
    dev = L.require_device(rows, offs, hdr, vals)
    if offs.shape != (n,) or offs.dtype != torch.int32 or vals.dtype != torch.int32 or \
            hdr.shape != (n, 2 * (F // 32)) or hdr.dtype != torch.int32 or not hdr.is_contiguous():
        raise ValueError("pack_rows_values: offs int32 [n], hdr int32 [n, 2 F/32], vals int32")
    launch("pack_rows_values", "mgcn_pack_rows_values", dev, n, None, lib.mgcn_pack_rows_values,
           n, F, L.ptr(rows), rows.stride(0), L.ptr(offs), L.ptr(hdr), L.ptr(vals),
           L.stream_of(dev))


@dataclass
class PackedTable:
    """An exchange table as the zero-skipping exchange delivered it
    (``mgcn_packed_table``): C x P packed segments of ``seg_rows`` rows each
    (pack.hip's layout), segment s at word ``seg_off[s]`` of buffer
    ``bufs[seg_buf[s]]`` (one receive buffer per row chunk, or one for all).
    The fused 128- and 256-wide layer kernels gather from it in place
    (:func:`spmm_xw_fwd` / :func:`spmm_xw_bwd` with a PackedTable for X / dY,
    over a view whose columns are packed positions (s << row_bits) | i:
    :func:`packed_cols`).  At F = 128 every segment must lie within 2 GiB of
    the lowest buffer (the kernels read the table through one range: in
    practice, one buffer)."""
    bufs: list               # int32 tensors holding the segments (kept alive here)
    seg_buf: list            # segment s -> index into bufs
    seg_off: list            # segment s -> word offset in that buffer
    seg_rows: int
    row_bits: int
    F: int

    @property
    def n_seg(self) -> int:
        return len(self.seg_off)

    @property
    def words(self) -> torch.Tensor:
        return self.bufs[0]

    def c_struct(self):
        """The C descriptor: every segment's offset counted from the lowest
        buffer address (one device address space)."""
        if self.n_seg > 64:
            raise ValueError(f"PackedTable: {self.n_seg} segments (at most 64)")
        ptrs = [b.data_ptr() for b in self.bufs]
        anchor = min(ptrs)
        if any((p - anchor) % 4 for p in ptrs):
            raise ValueError("PackedTable: buffers must be 4-byte aligned")
        rel = [(p - anchor) // 4 for p in ptrs]
        t = L.PackedTableC()
        t.words = anchor
        t.n_words = max(r + b.numel() for r, b in zip(rel, self.bufs))
        t.n_seg = self.n_seg
        t.seg_rows = int(self.seg_rows)
        t.row_bits = int(self.row_bits)
        t.F = int(self.F)
        for s_, (bi, off) in enumerate(zip(self.seg_buf, self.seg_off)):
            t.seg_base[s_] = rel[bi] + int(off)
        return t


def packed_row_bits(seg_rows: int) -> int:
    return max(int(seg_rows - 1).bit_length(), 0)


def packed_cols(col: torch.Tensor, seg_rows: int, row_bits: int) -> torch.Tensor:
    """Table positions t (row t % seg_rows of segment t // seg_rows) ->
    packed positions (s << row_bits) | i, int32."""
    t = col.to(torch.int64)
    s_ = torch.div(t, seg_rows, rounding_mode="floor")
    return ((s_ << row_bits) | (t - s_ * seg_rows)).to(torch.int32)


PACK_ROWS_WIDTHS = (32, 64, 128, 256)  # mgcn_pack_rows: one 256-word segment per row


def pack_rows(rows: torch.Tensor, hdr: torch.Tensor, vals: torch.Tensor,
              total: torch.Tensor) -> None:
    """The packed chunk in one pass (``mgcn_pack_rows``): hdr as
    pack_rows_count + pack_rows_values write it, vals, and total[0] = the
    number of values (device int64) -- no counts, no scan."""
    lib = L.load()
    rows = _contig_f32(rows, "rows")
    n, F = rows.shape
    dev = L.require_device(rows, hdr, vals, total)
    if F not in PACK_ROWS_WIDTHS or hdr.shape != (n, 2 * (F // 32)) or hdr.dtype != torch.int32 \
            or not hdr.is_contiguous() or vals.dtype != torch.int32 or total.dtype != torch.int64 \
            or total.numel() < 1:
        raise ValueError("pack_rows: F in (32, 64, 128, 256), hdr int32 [n, 2 F/32] contiguous, "
                         "vals int32, total int64")
    ws, ws_bytes = workspace(lib.mgcn_pack_rows_workspace_bytes(n, F), dev, or_null=True)
    launch("pack_rows", "mgcn_pack_rows", dev, n, None, lib.mgcn_pack_rows,
           n, F, L.ptr(rows), rows.stride(0), L.ptr(hdr), L.ptr(vals), L.ptr(total), L.ptr(ws),
           ws_bytes, L.stream_of(dev))


def unpack_rows(buf: torch.Tensor, n_seg: int, n: int, seg_words: int, out: torch.Tensor) -> None:
    """out[p n + i] = row i of packed segment p of ``buf`` (``mgcn_unpack_rows``)."""
    lib = L.load()
    dev = L.require_device(buf, out)
    F = out.size(1)
    if buf.dtype != torch.int32 or not buf.is_contiguous() or buf.numel() < n_seg * seg_words or \
            out.dtype != torch.float32 or out.size(0) < n_seg * n or out.stride(1) != 1:
        raise ValueError("unpack_rows: buf int32 [n_seg * seg_words], out float32 [n_seg * n, F]")
    launch("unpack_rows", "mgcn_unpack_rows", dev, n_seg * n, None, lib.mgcn_unpack_rows,
           n_seg, n, F, L.ptr(buf), seg_words, L.ptr(out), out.stride(0), L.stream_of(dev))
