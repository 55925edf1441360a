"""Dense products and the Linear layers on libmgcn's GEMM kernels, with the
column-sum / ReLU-mask passes their backwards use.  Sits on :mod:`mgcn._call`;
:mod:`mgcn.ops` re-exports every name."""
from __future__ import annotations

from collections import Counter

import torch

from . import _lib as L
from ._call import _aligned_rows, _contig_f32, launch, workspace


def relu_bwd_colsum(dZ: torch.Tensor, Z: torch.Tensor | None, relu: bool, want_db: bool,
                    row_div: torch.Tensor | None = None):
    """(dY, db): dY = Z > 0 ? dZ : 0 (dZ itself when not relu), divided by
    ``row_div`` per row when given (mean aggregation); db = sum_i of the
    undivided dY."""
    lib = L.load()
    dZ = dZ.contiguous()
    dev = L.require_device(dZ, Z, row_div)
    n, F = dZ.shape
    write = relu or row_div is not None
    dY = torch.empty_like(dZ) if write else dZ
    db = torch.empty(F, dtype=torch.float32, device=dev) if want_db else None
    if not write and not want_db:
        return dY, None
    ws, ws_bytes = workspace(lib.mgcn_colsum_workspace_bytes(n, F), dev) if want_db else (None, 0)
    launch("relu_bwd_colsum", "mgcn_relu_bwd_colsum", dev, n, None, lib.mgcn_relu_bwd_colsum,
           n, F, L.ptr(dZ), L.ptr(Z.contiguous() if relu else None), int(bool(relu)),
           L.ptr(row_div), L.ptr(dY if write else None), L.ptr(db), L.ptr(ws), ws_bytes,
           L.stream_of(dev))
    return dY, db


def gemm_tn(A: torch.Tensor, B: torch.Tensor, out: torch.Tensor | None = None,
            accumulate: bool = False) -> torch.Tensor:
    """C = A^T B on fp32 MFMA with split-K (libmgcn ``mgcn_gemm_tn``)."""
    lib = L.load()
    A = _contig_f32(A, "A")
    B = _contig_f32(B, "B")
    dev = L.require_device(A, B)
    K, M = A.shape
    if B.size(0) != K:
        raise ValueError(f"gemm_tn: A has {K} rows, B has {B.size(0)}")
    N = B.size(1)
    C = out if out is not None else torch.empty(M, N, dtype=torch.float32, device=dev)
    ws, ws_bytes = workspace(lib.mgcn_gemm_tn_workspace_bytes(K, M, N), dev)
    launch("gemm_tn", "mgcn_gemm_tn", dev, K, None, lib.mgcn_gemm_tn,
           K, M, N, L.ptr(A), A.stride(0), L.ptr(B), B.stride(0), L.ptr(C), C.stride(0),
           int(bool(accumulate)), L.ptr(ws), ws_bytes, L.stream_of(dev))
    return C


def gemm_tn_split(A: torch.Tensor, B: torch.Tensor, n1: int):
    """(C1, C2t) with A^T B = [C1 | C2t^T]: columns [0, n1) as C1 [M, n1],
    the rest transposed as C2t [N - n1, M], both contiguous, from one
    ``mgcn_gemm_tn_split`` pass (two parameter gradients in their own
    layouts, no copies)."""
    lib = L.load()
    A = _contig_f32(A, "A")
    B = _contig_f32(B, "B")
    dev = L.require_device(A, B)
    K, M = A.shape
    N = B.size(1)
    if B.size(0) != K or not 0 <= n1 <= N:
        raise ValueError(f"gemm_tn_split: A {tuple(A.shape)}, B {tuple(B.shape)}, n1 {n1}")
    C1 = torch.empty(M, n1, dtype=torch.float32, device=dev)
    C2 = torch.empty(N - n1, M, dtype=torch.float32, device=dev)
    ws, ws_bytes = workspace(lib.mgcn_gemm_tn_workspace_bytes(K, M, N), dev)
    launch("gemm_tn", "mgcn_gemm_tn_split", dev, K, None, lib.mgcn_gemm_tn_split,
           K, M, N, n1, L.ptr(A), A.stride(0), L.ptr(B), B.stride(0), L.ptr(C1), max(n1, 1),
           L.ptr(C2), max(M, 1), 0, L.ptr(ws), ws_bytes, L.stream_of(dev))
    return C1, C2


def gemm_nn_supported(K: int, N: int) -> bool:
    return bool(L.load().mgcn_gemm_nn_supported(int(K), int(N)))


def gemm_nn_epi_supported(K: int, N: int) -> bool:
    """The fused ReLU-mask / bias-gradient epilogue of mgcn_gemm_nn (the tuned
    kernel, N <= 128)."""
    return bool(L.load().mgcn_gemm_nn_epi_supported(int(K), int(N)))


def make_relu_mask(Z: torch.Tensor) -> torch.Tensor:
    """int32 [rows, 4]: bit b of word v set iff Z[i, 4 b + v] > 0 (F <= 128;
    ``mgcn_relu_mask``)."""
    lib = L.load()
    Z = _contig_f32(Z, "Z")
    dev = L.require_device(Z)
    n, F = Z.shape
    m = torch.empty(n, 4, dtype=torch.int32, device=dev)
    launch(None, "mgcn_relu_mask", dev, None, None, lib.mgcn_relu_mask,
           n, F, L.ptr(Z), Z.stride(0), L.ptr(m), L.stream_of(dev))
    return m


def gemm_nn(A: torch.Tensor, W: torch.Tensor, transpose_w: bool = False,
            Z: torch.Tensor | None = None, row_div: torch.Tensor | None = None,
            relu_mask: torch.Tensor | None = None):
    """C = A @ W (or A @ W^T) on libmgcn's tall-skinny MFMA kernel
    (``mgcn_gemm_nn``).  With ``relu_mask`` (from :func:`spmm_fwd` or
    :func:`make_relu_mask`) or ``Z``: C = Z > 0 ? A @ W^T : 0 and the column sums
    of C are returned too (fused ReLU backward + bias gradient).  Returns
    (C, colsum or None)."""
    lib = L.load()
    A = _aligned_rows(A, "A")
    W = W.detach()
    dev = L.require_device(A, W, Z, relu_mask)
    if relu_mask is None and Z is not None:
        relu_mask = make_relu_mask(Z)
    M, K = A.shape
    if transpose_w:
        N, Kw = W.shape
        sbk, sbn = W.stride(1), W.stride(0)
    else:
        Kw, N = W.shape
        sbk, sbn = W.stride(0), W.stride(1)
    if Kw != K:
        raise ValueError(f"gemm_nn: A is [{M}, {K}], W gives K = {Kw}")
    C = torch.empty(M, N, dtype=torch.float32, device=dev)
    colsum = ws = None
    ws_bytes = 0
    if relu_mask is not None:
        if relu_mask.shape != (M, 4) or relu_mask.dtype != torch.int32:
            raise ValueError(f"gemm_nn: relu_mask must be int32 [{M}, 4]")
        relu_mask = relu_mask.contiguous()
        colsum = torch.empty(N, dtype=torch.float32, device=dev)
        ws, ws_bytes = workspace(lib.mgcn_gemm_nn_workspace_bytes(M, N), dev)
    launch("gemm_nn", "mgcn_gemm_nn", dev, M, None, lib.mgcn_gemm_nn,
           M, K, N, L.ptr(A), A.stride(0), L.ptr(W), sbk, sbn, L.ptr(C), C.stride(0),
           L.ptr(relu_mask), L.ptr(row_div), L.ptr(colsum), L.ptr(ws), ws_bytes,
           L.stream_of(dev))
    return C, colsum


def gemm_bwd_supported(F_in: int, F_out: int) -> bool:
    return bool(L.load().mgcn_gemm_bwd_supported(int(F_in), int(F_out)))


def gemm_bwd(x: torch.Tensor, dH: torch.Tensor, W: torch.Tensor, want_dx: bool = True,
             relu_mask: torch.Tensor | None = None, row_div: torch.Tensor | None = None,
             dW_out: torch.Tensor | None = None, accumulate: bool = False,
             dh_colsum: bool = False):
    """Both adjoints of H = x @ W in one pass (``mgcn_gemm_bwd``, F_in = F_out
    = 128): dW = x^T dH and dX = dH W^T -- with ``relu_mask`` the lower
    layer's ReLU backward and bias-gradient column sums fused as in
    :func:`gemm_nn`.  ``dh_colsum`` (dW only): colsum = the column sums of dH
    (a bias gradient) from the same pass.  Returns (dW, dX or None, colsum or
    None)."""
    lib = L.load()
    x = _aligned_rows(x, "x")
    dH = _aligned_rows(dH, "dH")
    W = W.detach().contiguous()
    dev = L.require_device(x, dH, W, relu_mask, row_div)
    M, F_in = x.shape
    F_out = dH.size(1)
    if dH.size(0) != M or tuple(W.shape) != (F_in, F_out):
        raise ValueError(f"gemm_bwd: x {tuple(x.shape)}, dH {tuple(dH.shape)}, W {tuple(W.shape)}")
    dW = dW_out if dW_out is not None else torch.empty(F_in, F_out, dtype=torch.float32,
                                                       device=dev)
    dX = torch.empty(M, F_in, dtype=torch.float32, device=dev) if want_dx else None
    colsum = None
    if dh_colsum:
        if want_dx or relu_mask is not None:
            raise ValueError("gemm_bwd: dh_colsum is the dW-only form's")
        colsum = torch.empty(F_out, dtype=torch.float32, device=dev)
    if relu_mask is not None:
        if not want_dx:
            raise ValueError("gemm_bwd: relu_mask needs want_dx")
        if relu_mask.shape != (M, 4) or relu_mask.dtype != torch.int32:
            raise ValueError(f"gemm_bwd: relu_mask must be int32 [{M}, 4]")
        relu_mask = relu_mask.contiguous()
        colsum = torch.empty(F_in, dtype=torch.float32, device=dev)
    ws, ws_bytes = workspace(lib.mgcn_gemm_bwd_workspace_bytes(M, F_in, F_out), dev)
    launch("gemm_bwd" if want_dx else "gemm_bwd_dw", "mgcn_gemm_bwd", dev, M, None,
           lib.mgcn_gemm_bwd,
           M, F_in, F_out, L.ptr(x), x.stride(0), L.ptr(dH), dH.stride(0), L.ptr(W), W.stride(0),
           L.ptr(dW), dW.stride(0), int(bool(accumulate)), L.ptr(dX),
           dX.stride(0) if dX is not None else F_in, L.ptr(relu_mask), L.ptr(row_div),
           L.ptr(colsum), L.ptr(ws), ws_bytes, L.stream_of(dev))
    return dW, dX, colsum


def dw_pass_supported(F_in: int, F_out: int) -> bool:
    """The dense dW = Z^T dY pass of the reassociated backward: mgcn_gemm_bwd
    (dW-only) at 128 x 128, mgcn_gemm_tn (bf16x6, 128 x 128 output tiles)
    for other multiples of 128 (256 x 256: config 5)."""
    return gemm_bwd_supported(F_in, F_out) or (int(F_in) % 128 == 0 and int(F_out) % 128 == 0)


def dw_pass_cs(Z: torch.Tensor, dY: torch.Tensor, S: torch.Tensor):
    """(dW = Z^T dY, the column sums of S) in one pass (``mgcn_gemm_bwd_dw_cs``,
    128 x 128): S [M, 128] is streamed beside Z and dY -- a stack's top-layer
    bias gradient folded into its bottom layer's dW pass."""
    lib = L.load()
    Z = _contig_f32(Z, "Z")
    dY = _contig_f32(dY, "dY")
    S = _contig_f32(S, "S")
    for name, t in (("Z", Z), ("dY", dY), ("S", S)):
        if t.dim() != 2 or t.size(1) != 128 or t.stride(0) % 4 or t.data_ptr() % 16:
            raise ValueError(f"dw_pass_cs: {name} must be a [M, 128] float32 with 16-byte rows")
    M = Z.size(0)
    if dY.size(0) != M or S.size(0) != M:
        raise ValueError(f"dw_pass_cs: Z, dY, S rows {M}, {dY.size(0)}, {S.size(0)}")
    dev = L.require_device(Z, dY, S)
    dW = torch.empty(128, 128, dtype=torch.float32, device=dev)
    scs = torch.empty(128, dtype=torch.float32, device=dev)
    ws, ws_bytes = workspace(lib.mgcn_gemm_bwd_dw_cs_workspace_bytes(M), dev)
    launch("gemm_bwd_dw_cs", "mgcn_gemm_bwd_dw_cs", dev, M, None, lib.mgcn_gemm_bwd_dw_cs,
           M, L.ptr(Z), Z.stride(0), L.ptr(dY), dY.stride(0), L.ptr(dW), dW.stride(0), 0, None,
           L.ptr(S), S.stride(0), L.ptr(scs), L.ptr(ws), ws_bytes, L.stream_of(dev))
    return dW, scs


def dw_pass(Z: torch.Tensor, dY: torch.Tensor, W: torch.Tensor, dh_colsum: bool = False):
    """(dW = Z^T dY, the column sums of dY or None) -- :func:`dw_pass_supported`."""
    if gemm_bwd_supported(W.size(0), W.size(1)):
        dW, _, cs = gemm_bwd(Z, dY, W, want_dx=False, dh_colsum=dh_colsum)
        return dW, cs
    dW = gemm_tn(Z, dY)
    cs = relu_bwd_colsum(dY, None, False, True)[1] if dh_colsum else None
    return dW, cs


SMALL_K = 8  # mgcn_gemm_small_k: K <= 8, N <= 128


def gemm_small_k(A: torch.Tensor, W: torch.Tensor, transpose_w: bool = False) -> torch.Tensor:
    """A @ W (or A @ W^T) for a contraction of at most SMALL_K features
    (``mgcn_gemm_small_k``: k-ordered fma, HBM-bound)."""
    lib = L.load()
    A = _contig_f32(A, "A")
    W = W.detach().to(torch.float32)
    dev = L.require_device(A, W)
    K = A.size(1)
    N = W.size(0) if transpose_w else W.size(1)
    if (W.size(1) if transpose_w else W.size(0)) != K:
        raise ValueError(f"gemm_small_k: A {tuple(A.shape)}, W {tuple(W.shape)}")
    sbk, sbn = (W.stride(1), W.stride(0)) if transpose_w else (W.stride(0), W.stride(1))
    C = torch.empty(A.size(0), N, dtype=torch.float32, device=dev)
    launch(None, "mgcn_gemm_small_k", dev, None, None, lib.mgcn_gemm_small_k,
           A.size(0), K, N, L.ptr(A), A.stride(0), L.ptr(W), sbk, sbn, L.ptr(C), C.stride(0),
           L.stream_of(dev))
    return C


# Dense products that left libmgcn for torch.matmul (hipBLASLt), by shape:
# only non-2-D or non-fp32 operands do (every 2-D fp32 shape has a libmgcn
# kernel since ABI v15).  tests/test_host.py holds configs 2-4 to zero.
VENDOR_GEMMS: "Counter[tuple]" = Counter()


def mm_route(K: int, N: int, dim: int = 2, dtype=torch.float32) -> str:
    """Which kernel takes C[M, N] = A[M, K] B[K, N]: 'nn' (mgcn_gemm_nn: the
    tuned kernel for K in {32, 64, 128, 256}, the generic tiled one for the
    rest), 'small_k' (mgcn_gemm_small_k: K <= SMALL_K, N <= 128, k-ordered
    fma) or 'vendor' (torch.matmul: non-2-D / non-fp32 operands only)."""
    if dim != 2 or dtype != torch.float32 or K < 1 or N < 1:
        return "vendor"
    if K <= SMALL_K and N <= 128:
        return "small_k"
    return "nn"


def _mm(x: torch.Tensor, W: torch.Tensor) -> torch.Tensor:
    """x @ W on libmgcn (:func:`mm_route`)."""
    route = mm_route(W.size(0), W.size(1), x.dim(), x.dtype if W.dtype == torch.float32 else None)
    if route == "nn":
        return gemm_nn(x, W)[0]
    if route == "small_k":
        return gemm_small_k(x, W)
    VENDOR_GEMMS[("mm", tuple(x.shape), tuple(W.shape), str(x.dtype))] += 1
    return torch.matmul(x, W.detach())


def _mm_t(dH: torch.Tensor, W: torch.Tensor) -> torch.Tensor:
    """dH @ W^T on libmgcn (:func:`mm_route`)."""
    route = mm_route(W.size(1), W.size(0), dH.dim(),
                     dH.dtype if W.dtype == torch.float32 else None)
    if route == "nn":
        return gemm_nn(dH, W, transpose_w=True)[0]
    if route == "small_k":
        return gemm_small_k(dH, W, transpose_w=True)
    VENDOR_GEMMS[("mm_t", tuple(dH.shape), tuple(W.shape), str(dH.dtype))] += 1
    return torch.matmul(dH, W.detach().t())


def _gemm_batched(A: torch.Tensor, B: torch.Tensor, C: torch.Tensor,
                  a_str, b_str, c_str, M: int, N: int, K: int, batch: int,
                  accumulate: bool = False) -> None:
    """C (+)= A B per batch through explicit (batch, row, col) element strides
    (``mgcn_gemm_batched``)."""
    lib = L.load()
    dev = L.require_device(A, B, C)
    launch(None, "mgcn_gemm_batched", dev, None, None, lib.mgcn_gemm_batched,
           batch, M, N, K, L.ptr(A), *a_str, L.ptr(B), *b_str, L.ptr(C), *c_str,
           1 if accumulate else 0, L.stream_of(dev))


def _bstr(t: torch.Tensor):
    """(batch, row, col) strides of a 3-D tensor or a broadcast 2-D one."""
    return (t.stride(0), t.stride(1), t.stride(2)) if t.dim() == 3 else (0, t.stride(0), t.stride(1))


class _Bmm(torch.autograd.Function):
    """a [B, M, K] @ b ([B, K, N] or a broadcast [K, N]) on mgcn_gemm_batched,
    with its adjoints dA = dC b^T, db = a^T dC (summed over the batch for a
    broadcast b) through transposed strides -- no copies."""

    @staticmethod
    def forward(ctx, a, b):
        Bn, M, K = a.shape
        N = b.shape[-1]
        out = torch.empty(Bn, M, N, dtype=torch.float32, device=a.device)
        _gemm_batched(a, b, out, _bstr(a), _bstr(b), _bstr(out), M, N, K, Bn)
        ctx.save_for_backward(a, b)
        return out

    @staticmethod
    def backward(ctx, dC):
        a, b = ctx.saved_tensors
        dC = dC.to(torch.float32)  # any strides: the kernel addresses them
        Bn, M, K = a.shape
        N = b.shape[-1]
        da = db = None
        if ctx.needs_input_grad[0]:
            da = torch.empty_like(a, memory_format=torch.contiguous_format)
            sb = _bstr(b)
            _gemm_batched(dC, b, da, _bstr(dC), (sb[0], sb[2], sb[1]), _bstr(da), M, K, N, Bn)
        if ctx.needs_input_grad[1]:
            sa = _bstr(a)
            if b.dim() == 3:
                db = torch.empty(Bn, K, N, dtype=torch.float32, device=a.device)
                _gemm_batched(a, dC, db, (sa[0], sa[2], sa[1]), _bstr(dC), _bstr(db), K, N, M, Bn)
            else:  # broadcast weight: one product over the flattened batch rows
                a2 = a.reshape(Bn * M, K)
                d2 = dC.reshape(Bn * M, N)
                db = torch.empty(K, N, dtype=torch.float32, device=a.device)
                _gemm_batched(a2, d2, db, (0, a2.stride(1), a2.stride(0)), (0, d2.stride(0),
                              d2.stride(1)), (0, db.stride(0), db.stride(1)), K, N, Bn * M, 1)
        return da, db


def bmm(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Batched dense product of DiffPool's dense operators (PyG 1.3
    DenseSAGEConv / dense_diff_pool; reference kernel/diff_pool.py:13-14, 68,
    76): a [B, M, K] @ b [B, K, N] (or a [K, N] weight broadcast over the
    batch) on libmgcn's MFMA kernel, differentiable in both operands."""
    if a.dtype != torch.float32 or b.dtype != torch.float32:
        raise TypeError(f"bmm: float32 operands (the reference computes in fp32), got "
                        f"{a.dtype} @ {b.dtype}")
    if a.dim() != 3 or b.dim() not in (2, 3) or a.size(2) != b.size(-2) or \
            (b.dim() == 3 and b.size(0) != a.size(0)):
        raise ValueError(f"bmm: shapes {tuple(a.shape)} @ {tuple(b.shape)}")
    L.require_device(a, b)
    return _Bmm.apply(a, b)


class _Linear(torch.autograd.Function):
    """H = x @ W (gcn_base_models.py:201) with all three products on libmgcn's
    MFMA kernels: forward on mgcn_gemm_nn (tall-skinny); backward dW = x^T dH
    (a K = num_nodes reduction) and dX = dH W^T together in one pass of
    mgcn_gemm_bwd at F = 128, else mgcn_gemm_tn (split-K) + mgcn_gemm_nn."""

    @staticmethod
    def forward(ctx, x, W):
        ctx.save_for_backward(x, W)
        return _mm(x, W)

    @staticmethod
    def backward(ctx, dH):
        x, W = ctx.saved_tensors
        dx = dW = None
        dH = dH.contiguous()
        if ctx.needs_input_grad[1] and gemm_bwd_supported(W.size(0), W.size(1)):
            dW, dx, _ = gemm_bwd(x, dH, W, want_dx=bool(ctx.needs_input_grad[0]))
            return dx, dW
        if ctx.needs_input_grad[0]:
            dx = _mm_t(dH, W)
        if ctx.needs_input_grad[1]:
            dW = gemm_tn(x, dH)
        return dx, dW


class _LinearBias(torch.autograd.Function):
    """torch.nn.functional.linear(x, W, b) = x W^T + b with W [out, in] on the
    libmgcn GEMMs (dW = dy^T x is the K = num_nodes reduction that hipBLASLt
    runs at ~18 TFLOP/s: GCNModel's residual and final Linear layers,
    gcn_model.py:64-73)."""

    @staticmethod
    def forward(ctx, x, W, b):
        ctx.save_for_backward(x, W)
        ctx.has_b = b is not None
        y = _mm_t(x, W)
        return y.add_(b.detach()) if b is not None else y

    @staticmethod
    def backward(ctx, dy):
        x, W = ctx.saved_tensors
        dy = dy.contiguous()
        dx = dW = db = None
        if ctx.needs_input_grad[0]:
            dx = _mm(dy, W)
        if ctx.needs_input_grad[1]:
            dW = gemm_tn(dy, x)
        if ctx.has_b and ctx.needs_input_grad[2]:
            db = relu_bwd_colsum(dy, None, False, True)[1]
        return dx, dW, db


def linear_bias(x: torch.Tensor, W: torch.Tensor, b: torch.Tensor | None) -> torch.Tensor:
    """F.linear on libmgcn for 2-D fp32 inputs (other ranks / dtypes: torch's
    F.linear on the same HIP device).  CPU tensors raise: no CPU path."""
    L.require_device(x, W, b)
    if x.dtype == torch.bfloat16:
        # bf16 activations: weight and bias cast through autograd (fp32
        # master parameters receive fp32 gradients), product on the vendor GEMM
        W = W.to(x.dtype)
        b = b.to(x.dtype) if b is not None else None
    if x.dim() != 2 or x.dtype != torch.float32:
        VENDOR_GEMMS[("linear", tuple(x.shape), tuple(W.shape), str(x.dtype))] += 1
        return torch.nn.functional.linear(x, W, b)
    return _LinearBias.apply(x, W, b)


def linear(x: torch.Tensor, W: torch.Tensor) -> torch.Tensor:
    """``torch.matmul(x, W)`` with the libmgcn weight-gradient kernel.  CPU
    tensors raise: no CPU path."""
    L.require_device(x, W)
    if x.dtype == torch.bfloat16 and W.dtype != x.dtype:
        W = W.to(x.dtype)  # fp32 master weight: cast through autograd
    if x.dim() != 2 or x.dtype != torch.float32 or W.dtype != torch.float32:
        VENDOR_GEMMS[("matmul", tuple(x.shape), tuple(W.shape), str(x.dtype))] += 1
        return torch.matmul(x, W)
    return _Linear.apply(x, W)
