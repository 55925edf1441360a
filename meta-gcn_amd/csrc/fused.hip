// The fused GCN layer's C entry points at F = 128 and 256, dense and packed:
// argument checks, the kernels' argument structs and the routing between the
// kernels.  Host code only -- the 128-wide kernels live in fused_fwd.hip,
// fused_bwd.hip, fused_dws.hip and fused_fwd_ws.hip (xw128.h: the design and
// what they share), the 256-wide ones in fused_wide.hip.

#include "xw128.h"

using namespace mgcn;

extern "C" int mgcn_spmm_xw_supported(int32_t F_in, int32_t F_out, int reduce) {
  return F_in == F_out && (F_in == kXwF || F_in == 256) && gemm_precision_is_x6() &&
         (reduce == MGCN_REDUCE_SUM || reduce == MGCN_REDUCE_MEAN);
}

extern "C" int mgcn_spmm_xw_bwd_full_supported(int32_t F_in, int32_t F_out) {
  // the dW-accumulating backward and the max adjoint: 128 x 128 only (at
  // 256 the dW accumulators do not fit beside the gather: Z^T dY instead)
  return F_in == kXwF && F_out == kXwF && gemm_precision_is_x6();
}

extern "C" size_t mgcn_spmm_xw_fwd_workspace_bytes(int32_t F_in, int32_t F_out) {
  if (F_in == kXwF && F_out == kXwF) return xw_dyn_workspace_bytes();
  return F_in == 256 && F_out == 256 ? xw_wide_workspace_bytes(false) : 0;
}

// Host code the layer entry points share, dense and packed.  `who` is the
// entry's name, as in check_packed: every message keeps its prefix.
namespace {
inline bool aligned16(const void *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// the last argument checks of a forward; wide: the 256-wide kernels (no bias
// requirement, no ldz bound: 64-bit row bases)
int check_fwd_outputs(const char *who, bool wide, int32_t F_in, const float *bias,
                      const uint32_t *relu_mask, const float *Z, int64_t ldz) {
  MGCN_REQUIRE(wide || bias == nullptr || reinterpret_cast<uintptr_t>(bias) % 4 == 0,
               "%s: bias not 4-byte aligned", who);
  MGCN_REQUIRE(relu_mask == nullptr || aligned16(relu_mask), "%s: relu_mask not 16-byte aligned",
               who);
  MGCN_REQUIRE(Z == nullptr || (ldz >= F_in && ldz % 4 == 0 && aligned16(Z) &&
                                (wide || (uint64_t)kXwRows * (uint64_t)ldz * 4u < (1ull << 31))),
               "%s: Z must have 16-byte aligned rows (ldz >= F_in)", who);
  return MGCN_OK;
}

// the 128-wide forward's arguments but its table (X, ldx, n_cols, or fill_pk128)
XwArgs xw_args(int64_t n_rows, const int64_t *rowptr, const int32_t *col, const float *w,
               const float *W, int64_t ldw, const float *bias, float *Y, int64_t ldy, int reduce,
               int relu, uint32_t *relu_mask, float *Z, int64_t ldz) {
  XwArgs a{};
  a.n_rows = n_rows;
  a.rowptr = rowptr;
  a.col = col;
  a.w = w;
  a.W = W;
  a.ldw = ldw;
  a.bias = bias;
  a.Y = Y;
  a.ldy = ldy;
  a.relu_mask = relu_mask;
  a.Z = Z;
  a.ldz = ldz;
  a.mean = reduce == MGCN_REDUCE_MEAN;
  a.relu = relu != 0;
  return a;
}

inline int epi_of(const uint32_t *relu_mask, const float *row_div) {
  return relu_mask == nullptr ? EPI_STORE : row_div != nullptr ? EPI_RELU_DIV : EPI_RELU;
}

// the last argument checks of an adjoint: W / dX (wide: the 256-wide
// kernels), the mask and the workspace
int check_bwd_outputs(const char *who, bool wide, int64_t n_rows, int32_t F_in, int32_t F_out,
                      const float *W, int64_t ldw, const float *dX, int64_t lddx,
                      const uint32_t *relu_mask, const void *workspace, size_t workspace_bytes) {
  if (wide)
    MGCN_REQUIRE(W != nullptr && ldw >= F_out && lddx >= F_in && lddx % 4 == 0 && aligned16(dX) &&
                     (uint64_t)16 * (uint64_t)lddx * 4u < (1ull << 31),
                 "%s: bad W/dX (16-byte aligned dX rows)", who);
  else  // the warp-specialised adjoint copies W into LDS with 16-byte loads
    MGCN_REQUIRE(W == nullptr || (ldw % 4 == 0 && aligned16(W)),
                 "%s: W must have 16-byte aligned rows", who);
  MGCN_REQUIRE(relu_mask == nullptr || aligned16(relu_mask), "%s: relu_mask not 16-byte aligned",
               who);
  return require_workspace(who, workspace, workspace_bytes,
                           mgcn_spmm_xw_bwd_workspace_bytes(n_rows, F_in, F_out));
}

// the 128-wide adjoint's arguments but its table (dY, lddy, n_cols, or
// fill_pk128), X and the max adjoint's maps; the workspace split into the dW
// and column-sum partials
XbArgs xb_args(int64_t n_rows, const int64_t *rowptr_t, const int32_t *col_t, const float *w_t,
               const float *row_scale, const float *W, int64_t ldw, float *dX, int64_t lddx,
               const uint32_t *relu_mask, const float *row_div, void *workspace) {
  XbArgs a{};
  a.n_rows = n_rows;
  a.rowptr = rowptr_t;
  a.col = col_t;
  a.w = w_t;
  a.row_scale = row_scale;
  a.W = W;
  a.ldw = ldw;
  a.dX = dX;
  a.lddx = lddx;
  a.relu_mask = relu_mask;
  a.row_div = row_div;
  a.dw_partial = static_cast<float *>(workspace);
  a.colsum_partial = reinterpret_cast<float *>(static_cast<char *>(workspace) +
                                               align_up((size_t)xw_grid() * kXwF * kXwF * 4, 256));
  return a;
}
}  // namespace

extern "C" int mgcn_spmm_xw_fwd(int64_t n_rows, int64_t n_cols, int32_t F_in, int32_t F_out,
                                const int64_t *rowptr, const int32_t *col, const float *w,
                                const float *X, int64_t ldx, const float *W, int64_t ldw,
                                const float *bias, float *Y, int64_t ldy, int reduce, int relu,
                                uint32_t *relu_mask, float *Z, int64_t ldz, void *workspace,
                                size_t workspace_bytes, void *stream) {
  clear_error();
  if (int rc = take_device_error()) return rc;  // a previous launch failed on the device
  MGCN_REQUIRE(n_rows >= 0, "mgcn_spmm_xw_fwd: negative size");
  MGCN_REQUIRE(mgcn_spmm_xw_supported(F_in, F_out, reduce),
               "mgcn_spmm_xw_fwd: unsupported F_in=%d F_out=%d reduce=%d (needs 128 x 128 or "
               "256 x 256, sum/mean, bf16x6)",
               F_in, F_out, reduce);
  MGCN_REQUIRE(relu_mask == nullptr || relu, "mgcn_spmm_xw_fwd: relu_mask needs relu");
  if (n_rows == 0) return MGCN_OK;
  MGCN_REQUIRE(rowptr && X && W && Y, "mgcn_spmm_xw_fwd: null array");
  MGCN_REQUIRE(ldx >= F_in && ldx % 4 == 0 && reinterpret_cast<uintptr_t>(X) % 16 == 0,
               "mgcn_spmm_xw_fwd: X must have 16-byte aligned rows");
  MGCN_REQUIRE(ldw >= F_out && ldy >= F_out, "mgcn_spmm_xw_fwd: leading dimension too small");
  if (F_in == 256) {
    // the wide kernels address every gathered row through a 64-bit base:
    // no table-size limit; 32-bit offsets only within a 16-row chunk
    MGCN_REQUIRE(n_cols > 0 && (uint64_t)16 * (uint64_t)(ldy > ldz ? ldy : ldz) * 4u < (1ull << 31),
                 "mgcn_spmm_xw_fwd: leading dimension too large");
    if (int rc = check_fwd_outputs("mgcn_spmm_xw_fwd", true, F_in, bias, relu_mask, Z, ldz))
      return rc;
    MGCN_REQUIRE(ldy % 4 == 0 && aligned16(Y),
                 "mgcn_spmm_xw_fwd: Y must have 16-byte aligned rows at F = 256");
    if (int rc = require_workspace("mgcn_spmm_xw_fwd", workspace, workspace_bytes,
                                   mgcn_spmm_xw_fwd_workspace_bytes(F_in, F_out)))
      return rc;
    return xw_wide_fwd(n_rows, rowptr, col, w, X, ldx, W, ldw, bias, Y, ldy,
                       reduce == MGCN_REDUCE_MEAN, relu != 0, relu_mask, Z, ldz, workspace,
                       as_stream(stream));
  }
  MGCN_REQUIRE(n_cols > 0 && (uint64_t)n_cols * (uint64_t)ldx * 4u <= 0xfffffff0ull,
               "mgcn_spmm_xw_fwd: X must hold 1 .. 4 GiB - 1 bytes (32-bit gather offsets)");
  MGCN_REQUIRE((uint64_t)kXwRows * (uint64_t)ldy * 4u < (1ull << 31),
               "mgcn_spmm_xw_fwd: ldy too large");
  if (int rc = check_fwd_outputs("mgcn_spmm_xw_fwd", false, F_in, bias, relu_mask, Z, ldz))
    return rc;
  XwArgs a = xw_args(n_rows, rowptr, col, w, W, ldw, bias, Y, ldy, reduce, relu, relu_mask, Z, ldz);
  a.X = X;
  a.ldx = ldx;
  a.n_cols = n_cols;
  hipStream_t s = as_stream(stream);
  // (without the workspace -- callers from before it existed -- every chunk is static)
  int rc = MGCN_OK;
  if (launch_xw_ws(&a, workspace, workspace_bytes, s, &rc)) return rc;
  if (launch_xw_dyn(&a, workspace, workspace_bytes, s, &rc)) return rc;
  return launch_xw_fwd(&a, false, s);
}

extern "C" size_t mgcn_spmm_xw_bwd_workspace_bytes(int64_t n_rows, int32_t F_in, int32_t F_out) {
  (void)n_rows;
  if (F_in == 256 && F_out == 256) return xw_wide_workspace_bytes(true);
  const size_t g = (size_t)xw_grid();
  return align_up(g * kXwF * kXwF * 4, 256) + align_up(g * kXwF * 4, 256);
}

namespace {
// mgcn_spmm_xw_bwd and (dy_colsum != NULL) mgcn_spmm_xw_bwd_hcs
int xw_bwd_impl(int64_t n_rows, int64_t n_cols, int32_t F_in, int32_t F_out,
                const int64_t *rowptr_t, const int32_t *col_t, const float *w_t,
                const float *row_scale, const float *dY, int64_t lddy, const float *X,
                int64_t ldx, const float *W, int64_t ldw, float *dW, int64_t lddw, int accumulate,
                float *dX, int64_t lddx, const uint32_t *relu_mask, const float *row_div,
                float *colsum, const uint32_t *win_mask, const int32_t *slot_map,
                float *dy_colsum, void *workspace, size_t workspace_bytes, void *stream) {
  if (int rc = take_device_error()) return rc;  // a previous launch failed on the device
  MGCN_REQUIRE(n_rows >= 0, "mgcn_spmm_xw_bwd: negative size");
  MGCN_REQUIRE((win_mask == nullptr) == (slot_map == nullptr),
               "mgcn_spmm_xw_bwd: win_mask and slot_map go together (max adjoint)");
  MGCN_REQUIRE(mgcn_spmm_xw_supported(F_in, F_out, MGCN_REDUCE_SUM),
               "mgcn_spmm_xw_bwd: unsupported F_in=%d F_out=%d (needs 128 x 128 or 256 x 256, "
               "bf16x6)", F_in, F_out);
  // X == NULL and dW == NULL: dX only (dW formed by the caller from Z^T dY)
  const bool dx_only = X == nullptr && dW == nullptr;
  MGCN_REQUIRE(dx_only || mgcn_spmm_xw_bwd_full_supported(F_in, F_out),
               "mgcn_spmm_xw_bwd: at F=%d only the dX-only form (X = dW = NULL)", F_in);
  MGCN_REQUIRE(dx_only || (X != nullptr && dW != nullptr && lddw >= F_out),
               "mgcn_spmm_xw_bwd: bad dW (X and dW are given together, or both NULL for dX only)");
  MGCN_REQUIRE(row_div == nullptr || relu_mask != nullptr,
               "mgcn_spmm_xw_bwd: row_div needs relu_mask");
  hipStream_t s = as_stream(stream);
  if (n_rows == 0) {  // an empty row range (a sharded chunk): no dX rows to write
    if (dy_colsum) MGCN_HIP_TRY(hipMemsetAsync(dy_colsum, 0, sizeof(float) * F_out, s));
    if (!accumulate && dW != nullptr)
      for (int32_t r = 0; r < F_in; ++r)
        MGCN_HIP_TRY(hipMemsetAsync(dW + r * lddw, 0, sizeof(float) * F_out, s));
    if (colsum && !(dx_only && accumulate))
      MGCN_HIP_TRY(hipMemsetAsync(colsum, 0, sizeof(float) * F_in, s));
    return MGCN_OK;
  }
  MGCN_REQUIRE(!dx_only || (dX != nullptr && win_mask == nullptr),
               "mgcn_spmm_xw_bwd: the dX-only form needs dX and takes no win_mask");
  const int epi = epi_of(relu_mask, row_div);
  MGCN_REQUIRE(epi == EPI_STORE || (dX != nullptr && colsum != nullptr),
               "mgcn_spmm_xw_bwd: relu_mask needs dX and colsum");
  MGCN_REQUIRE(rowptr_t && dY, "mgcn_spmm_xw_bwd: null array");
  MGCN_REQUIRE(lddy >= F_out && lddy % 4 == 0 && reinterpret_cast<uintptr_t>(dY) % 16 == 0,
               "mgcn_spmm_xw_bwd: dY must have 16-byte aligned rows");
  if (F_in == 256) {
    MGCN_REQUIRE(dX != nullptr && win_mask == nullptr, "mgcn_spmm_xw_bwd: the dX-only form needs dX");
    if (int rc = check_bwd_outputs("mgcn_spmm_xw_bwd", true, n_rows, F_in, F_out, W, ldw, dX, lddx,
                                   relu_mask, workspace, workspace_bytes))
      return rc;
    return xw_wide_bwd_dx(n_rows, rowptr_t, col_t, w_t, row_scale, dY, lddy, W, ldw, dX, lddx,
                          relu_mask, row_div, colsum, accumulate, workspace, s);
  }
  MGCN_REQUIRE(dx_only || (ldx >= F_in && ldx % 4 == 0 && reinterpret_cast<uintptr_t>(X) % 16 == 0),
               "mgcn_spmm_xw_bwd: X must have 16-byte aligned rows");
  if (dx_only) ldx = 0;
  MGCN_REQUIRE(n_cols > 0 && (uint64_t)n_cols * (uint64_t)lddy * 4u <= 0xfffffff0ull,
               "mgcn_spmm_xw_bwd: dY must hold 1 .. 4 GiB - 1 bytes (32-bit gather offsets)");
  MGCN_REQUIRE((uint64_t)kXwRows * (uint64_t)(ldx > lddx ? ldx : lddx) * 4u < (1ull << 31),
               "mgcn_spmm_xw_bwd: leading dimension too large");
  MGCN_REQUIRE(dX == nullptr || (W != nullptr && ldw >= F_out && lddx >= F_in),
               "mgcn_spmm_xw_bwd: bad W/dX");
  if (int rc = check_bwd_outputs("mgcn_spmm_xw_bwd", false, n_rows, F_in, F_out, W, ldw, dX, lddx,
                                 relu_mask, workspace, workspace_bytes))
    return rc;
  const int64_t n_chunks = (n_rows + kXwRows - 1) / kXwRows;
  int grid = xw_grid();
  if (grid > n_chunks) grid = (int)n_chunks;
  XbArgs a = xb_args(n_rows, rowptr_t, col_t, w_t, row_scale, W, ldw, dX, lddx, relu_mask, row_div,
                     workspace);
  a.dY = dY;
  a.lddy = lddy;
  a.n_cols = n_cols;
  a.X = X;
  a.ldx = ldx;
  a.win_mask = win_mask;
  a.slot_map = slot_map;
  int rc;
  if (dx_only) {
    rc = launch_xb_bwd(&a, epi, grid, true, false, s);
    if (rc || epi == EPI_STORE) return rc;
    // dX only: accumulate != 0 adds the column sums into colsum (row chunks
    // of one adjoint fold their bias gradient on the device)
    return launch_fold(a.colsum_partial, grid, kXwF, kXwF, colsum, kXwF, accumulate, s);
  }
  float *hcs_partial = nullptr;
  // (the max adjoint's dW-only form stays two-phase: 1.10 vs 1.22 ms at config 4)
  if ((g_opt.xw_ws_full || dy_colsum) &&
      (win_mask == nullptr || (g_opt.xw_ws_max && dX != nullptr))) {
    // the warp-specialised dW + dX (or dW-only) form (one workgroup per CU; DWS)
    grid = device_cus() < n_chunks ? device_cus() : (int)n_chunks;
    // dY's column sums: [grid][128] partials past the grid's dW slabs (the
    // dW partial area holds xw_grid() = 2 x CUs slabs, this grid <= CUs)
    if (dy_colsum) hcs_partial = a.dw_partial + (size_t)grid * kXwF * kXwF;
    rc = launch_dws(&a, epi, grid, hcs_partial, s);
  } else {
    rc = launch_xb_bwd(&a, epi, grid, false, false, s);
  }
  if (rc) return rc;
  rc = launch_split_reduce(a.dw_partial, grid, (int64_t)kXwF * kXwF, kXwF, dW, lddw, accumulate, s);
  if (rc == MGCN_OK && hcs_partial) rc = launch_colsum_fold(hcs_partial, grid, kXwF, dy_colsum, s);
  if (rc || epi == EPI_STORE) return rc;
  return launch_colsum_fold(a.colsum_partial, grid, kXwF, colsum, s);
}
}  // namespace

extern "C" int mgcn_spmm_xw_bwd(int64_t n_rows, int64_t n_cols, int32_t F_in, int32_t F_out,
                                const int64_t *rowptr_t, const int32_t *col_t, const float *w_t,
                                const float *row_scale, const float *dY, int64_t lddy,
                                const float *X, int64_t ldx, const float *W, int64_t ldw,
                                float *dW, int64_t lddw, int accumulate, float *dX, int64_t lddx,
                                const uint32_t *relu_mask, const float *row_div, float *colsum,
                                const uint32_t *win_mask, const int32_t *slot_map,
                                void *workspace, size_t workspace_bytes, void *stream) {
  clear_error();
  return xw_bwd_impl(n_rows, n_cols, F_in, F_out, rowptr_t, col_t, w_t, row_scale, dY, lddy, X,
                     ldx, W, ldw, dW, lddw, accumulate, dX, lddx, relu_mask, row_div, colsum,
                     win_mask, slot_map, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int mgcn_spmm_xw_bwd_hcs(int64_t n_rows, int64_t n_cols, const int64_t *rowptr_t,
                                    const int32_t *col_t, const float *w_t,
                                    const float *row_scale, const float *dY, int64_t lddy,
                                    const float *X, int64_t ldx, const float *W, int64_t ldw,
                                    float *dW, int64_t lddw, int accumulate, float *dX,
                                    int64_t lddx, const uint32_t *relu_mask,
                                    const float *row_div, float *colsum, float *dy_colsum,
                                    void *workspace, size_t workspace_bytes, void *stream) {
  clear_error();
  MGCN_REQUIRE(n_rows == n_cols, "mgcn_spmm_xw_bwd_hcs: needs n_rows == n_cols (%lld, %lld): "
               "every dY row a row of the view", (long long)n_rows, (long long)n_cols);
  MGCN_REQUIRE(X != nullptr && dW != nullptr && dX != nullptr && dy_colsum != nullptr,
               "mgcn_spmm_xw_bwd_hcs: X, dW, dX and dy_colsum are required");
  return xw_bwd_impl(n_rows, n_cols, kXwF, kXwF, rowptr_t, col_t, w_t, row_scale, dY, lddy, X,
                     ldx, W, ldw, dW, lddw, accumulate, dX, lddx, relu_mask, row_div, colsum,
                     nullptr, nullptr, dy_colsum, workspace, workspace_bytes, stream);
}

#if MGCN_EXPERIMENT
// [2][1024][4] ticks (XTAIL_*, xw128.h: the forward's, then DWS's) to `host`,
// then cleared for the next launch
extern "C" int mgcn_debug_xw_tail(unsigned long long *host) {
  MGCN_HIP_TRY(hipDeviceSynchronize());
  if (int rc = xw_fwd_tail_take(host)) return rc;
  return dws_tail_take(host != nullptr ? host + kTailMaxWg * 4 : nullptr);
}
#endif

// ---------------------------------------------------------------- packed tables
namespace {
int check_packed(const mgcn_packed_table *t, int32_t F, const char *who) {
  MGCN_REQUIRE(t != nullptr && t->words != nullptr, "%s: null packed table", who);
  MGCN_REQUIRE(t->F == F, "%s: packed table of F = %d for a layer of F = %d", who, t->F, F);
  MGCN_REQUIRE(t->n_seg >= 1 && t->n_seg <= 64, "%s: n_seg %d outside 1 .. 64", who, t->n_seg);
  MGCN_REQUIRE(t->row_bits >= 0 && t->row_bits + 6 <= 31 && t->seg_rows >= 1 &&
                   (int64_t)t->seg_rows <= ((int64_t)1 << t->row_bits),
               "%s: seg_rows %d does not fit row_bits %d", who, t->seg_rows, t->row_bits);
  // in-segment byte offsets stay below 2 GiB (the header plus a dense-size
  // value area): the kernels' buffer ranges are capped there
  MGCN_REQUIRE((uint64_t)t->seg_rows * (2 * (F / 32) + F) * 4u + 16u < (1ull << 31),
               "%s: seg_rows %d too large for the 2-GiB in-segment offsets", who, t->seg_rows);
  MGCN_REQUIRE(t->n_words >= 0, "%s: negative n_words", who);
  if (F == kXwF) {
    // F = 128: one buffer resource over the whole table (32-bit offsets)
    MGCN_REQUIRE((uint64_t)t->n_words * 4u <= 0x7ffffff0ull,
                 "%s: an F = 128 packed table spans at most 2 GiB - 16 B (got %lld words)", who,
                 (long long)t->n_words);
    for (int s = 0; s < t->n_seg; ++s)
      MGCN_REQUIRE(t->seg_base[s] >= 0 && t->seg_base[s] <= t->n_words,
                   "%s: segment %d at word %lld outside the table's %lld words", who, s,
                   (long long)t->seg_base[s], (long long)t->n_words);
  }
  return MGCN_OK;
}

// the F = 128 kernels' view of a checked packed table
template <class Args>
void fill_pk128(Args &a, const mgcn_packed_table *t) {
  a.pk = t->words;
  a.pk_bytes = (uint32_t)(t->n_words * 4);
  a.pk_rbits = (uint32_t)t->row_bits;
  a.pk_head = (uint32_t)t->seg_rows * 8u;
  for (int s = 0; s < 64; ++s) a.pk_base[s] = s < t->n_seg ? (uint32_t)t->seg_base[s] : 0u;
}
}  // namespace

extern "C" int mgcn_spmm_xw_fwd_packed(int64_t n_rows, int32_t F_in, int32_t F_out,
                                       const int64_t *rowptr, const int32_t *col, const float *w,
                                       const mgcn_packed_table *X, const float *W, int64_t ldw,
                                       const float *bias, float *Y, int64_t ldy, int reduce,
                                       int relu, uint32_t *relu_mask, float *Z, int64_t ldz,
                                       void *workspace, size_t workspace_bytes, void *stream) {
  clear_error();
  if (int rc = take_device_error()) return rc;  // a previous launch failed on the device
  MGCN_REQUIRE(n_rows >= 0, "mgcn_spmm_xw_fwd_packed: negative size");
  MGCN_REQUIRE(mgcn_spmm_xw_supported(F_in, F_out, reduce),
               "mgcn_spmm_xw_fwd_packed: 128 x 128 or 256 x 256, sum / mean, bf16x6 only");
  MGCN_REQUIRE(relu_mask == nullptr || relu, "mgcn_spmm_xw_fwd_packed: relu_mask needs relu");
  if (n_rows == 0) return MGCN_OK;
  if (int rc = check_packed(X, F_in, "mgcn_spmm_xw_fwd_packed")) return rc;
  MGCN_REQUIRE(rowptr && W && Y, "mgcn_spmm_xw_fwd_packed: null array");
  if (F_in == kXwF) {
    MGCN_REQUIRE(ldw >= F_out && ldy >= F_out && (uint64_t)kXwRows * (uint64_t)ldy * 4u < (1ull << 31),
                 "mgcn_spmm_xw_fwd_packed: bad ldw / ldy");
    if (int rc = check_fwd_outputs("mgcn_spmm_xw_fwd_packed", false, F_in, bias, relu_mask, Z, ldz))
      return rc;
    XwArgs a = xw_args(n_rows, rowptr, col, w, W, ldw, bias, Y, ldy, reduce, relu, relu_mask, Z,
                       ldz);
    fill_pk128(a, X);
    return launch_xw_fwd(&a, true, as_stream(stream));
  }
  MGCN_REQUIRE(ldw >= F_out && ldy >= F_out && ldy % 4 == 0 &&
                   reinterpret_cast<uintptr_t>(Y) % 16 == 0 &&
                   (uint64_t)16 * (uint64_t)(ldy > ldz ? ldy : ldz) * 4u < (1ull << 31),
               "mgcn_spmm_xw_fwd_packed: Y must have 16-byte aligned rows");
  if (int rc = check_fwd_outputs("mgcn_spmm_xw_fwd_packed", true, F_in, bias, relu_mask, Z, ldz))
    return rc;
  if (int rc = require_workspace("mgcn_spmm_xw_fwd_packed", workspace, workspace_bytes,
                                 mgcn_spmm_xw_fwd_workspace_bytes(F_in, F_out)))
    return rc;
  return xw_wide_fwd(n_rows, rowptr, col, w, nullptr, 0, W, ldw, bias, Y, ldy,
                     reduce == MGCN_REDUCE_MEAN, relu != 0, relu_mask, Z, ldz, workspace,
                     as_stream(stream), X);
}

extern "C" int mgcn_spmm_xw_bwd_packed(int64_t n_rows, int32_t F_in, int32_t F_out,
                                       const int64_t *rowptr_t, const int32_t *col_t,
                                       const float *w_t, const float *row_scale,
                                       const mgcn_packed_table *dY, const float *W, int64_t ldw,
                                       float *dX, int64_t lddx, const uint32_t *relu_mask,
                                       const float *row_div, float *colsum, int accumulate,
                                       void *workspace, size_t workspace_bytes, void *stream) {
  clear_error();
  if (int rc = take_device_error()) return rc;  // a previous launch failed on the device
  MGCN_REQUIRE(n_rows >= 0, "mgcn_spmm_xw_bwd_packed: negative size");
  MGCN_REQUIRE(mgcn_spmm_xw_supported(F_in, F_out, MGCN_REDUCE_SUM),
               "mgcn_spmm_xw_bwd_packed: 128 x 128 or 256 x 256, bf16x6 only");
  MGCN_REQUIRE(row_div == nullptr || relu_mask != nullptr,
               "mgcn_spmm_xw_bwd_packed: row_div needs relu_mask");
  MGCN_REQUIRE(relu_mask == nullptr || colsum != nullptr,
               "mgcn_spmm_xw_bwd_packed: relu_mask needs colsum");
  hipStream_t s = as_stream(stream);
  if (n_rows == 0) {  // an empty row range: no dX rows to write
    if (colsum && !accumulate) MGCN_HIP_TRY(hipMemsetAsync(colsum, 0, sizeof(float) * F_in, s));
    return MGCN_OK;
  }
  if (int rc = check_packed(dY, F_out, "mgcn_spmm_xw_bwd_packed")) return rc;
  MGCN_REQUIRE(rowptr_t && W && dX, "mgcn_spmm_xw_bwd_packed: null array");
  if (F_in == kXwF) {
    MGCN_REQUIRE(ldw >= F_out && lddx >= F_in && (uint64_t)kXwRows * (uint64_t)lddx * 4u < (1ull << 31),
                 "mgcn_spmm_xw_bwd_packed: bad W/dX");
    if (int rc = check_bwd_outputs("mgcn_spmm_xw_bwd_packed", false, n_rows, F_in, F_out, W, ldw,
                                   dX, lddx, relu_mask, workspace, workspace_bytes))
      return rc;
    const int epi = epi_of(relu_mask, row_div);
    const int64_t n_chunks = (n_rows + kXwRows - 1) / kXwRows;
    int grid = xw_grid();
    if (grid > n_chunks) grid = (int)n_chunks;
    XbArgs a = xb_args(n_rows, rowptr_t, col_t, w_t, row_scale, W, ldw, dX, lddx, relu_mask,
                       row_div, workspace);
    fill_pk128(a, dY);
    const int rc = launch_xb_bwd(&a, epi, grid, true, true, s);
    if (rc || epi == EPI_STORE) return rc;
    return launch_fold(a.colsum_partial, grid, kXwF, kXwF, colsum, kXwF, accumulate, s);
  }
  if (int rc = check_bwd_outputs("mgcn_spmm_xw_bwd_packed", true, n_rows, F_in, F_out, W, ldw, dX,
                                 lddx, relu_mask, workspace, workspace_bytes))
    return rc;
  return xw_wide_bwd_dx(n_rows, rowptr_t, col_t, w_t, row_scale, nullptr, 0, W, ldw, dX, lddx,
                        relu_mask, row_div, colsum, accumulate, workspace, s, dY);
}
