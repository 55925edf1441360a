/*
 * mgcn.h -- C ABI of libmgcn.so, the MI355X (gfx950) engine behind the GCN
 * neighbourhood aggregation  Y = reduce_{e: dst_e = i} w_e * H[src_e]  and its
 * adjoint  dH = A^T dY.
 *
 * Plain C: pointers, sizes and a `void *stream` (a hipStream_t; NULL = the
 * default stream).  No torch types.  Every buffer is BORROWED: the library
 * never allocates or frees device memory; scratch space is passed in by the
 * caller (see the *_workspace_bytes queries).  Every call returns 0 on
 * success or an MGCN_E* code; mgcn_last_error() (thread-local) says why.
 *
 * Each entry point names the reference interface it replaces
 * (paths relative to jzhou316/meta-gcn @ 2025-08-24):
 *
 *  - torch_scatter.scatter_{add,mean,max}(src, index, 0, out, dim_size, fill)
 *      called at src/gcn_meta/models/common.py:56-59 on the gathered-and-scaled
 *      edge tensor built at src/gcn_meta/models/gcn_base_models.py:209-224.
 *      The reference materialises x_j = x[src] * norm  ([E, F]) and then
 *      scatters it; mgcn_spmm_fwd fuses gather, scale, reduce, the
 *      `out[out == fill] = 0` fix-up (common.py:63-64), the bias add
 *      (gcn_base_models.py:240-241) and the layer ReLU
 *      (gcn_model.py:196, kernel/gcn.py:26-28) and never materialises [E, F].
 *  - the autograd adjoints of those ops (index_select -> index_add_,
 *      mul -> mul, scatter -> gather / argmax routing): mgcn_spmm_bwd.
 *  - NodeModelBase.degnorm_const (src/gcn_meta/models/gcn_base_models.py:65-146):
 *      mgcn_degree_norm + mgcn_edge_norm.
 *  - the per-forward graph bookkeeping of PyG (edge_index kept as COO and
 *      re-scattered every call): mgcn_csr_build, run once per static graph.
 */
#ifndef MGCN_H
#define MGCN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MGCN_ABI_VERSION 22

/* return codes */
#define MGCN_OK 0
#define MGCN_EINVAL 1   /* bad argument (shape, alignment, null pointer)      */
#define MGCN_EINDEX 2   /* an edge index is outside [0, n)                    */
#define MGCN_EHIP 3     /* a HIP runtime call or kernel launch failed          */
#define MGCN_EWORKSPACE 4 /* caller-provided workspace is too small            */
#define MGCN_EDEVICE 5  /* a kernel reported a failure from the device: the
                           outputs of that launch are invalid (see
                           mgcn_check_device)                                 */

/* reductions (common.py:54 `name in ['add', 'mean', 'max']`) */
#define MGCN_REDUCE_SUM 0
#define MGCN_REDUCE_MEAN 1
#define MGCN_REDUCE_MAX 2

/* degree normalisation methods (gcn_base_models.py:45 deg_norm) */
#define MGCN_NORM_NONE 0
#define MGCN_NORM_SM 1 /* symmetric:  deg^-1/2[src] * w * deg^-1/2[dst]  */
#define MGCN_NORM_RW 2 /* random walk: deg^-1[src] * w                    */

/* fill value of the 'max' reduction (common.py:57) */
#define MGCN_MAX_FILL (-1e38f)

int mgcn_abi_version(void);
const char *mgcn_last_error(void);

/* Device-side failures (ABI 21).  The warp-specialised kernels (the 128-wide
 * adjoint behind mgcn_spmm_xw_bwd, the 256-wide layer kernels behind
 * mgcn_spmm_xw_fwd / _bwd) hand chunks between their waves through LDS
 * counters with bounded spins; a spin that runs past its bound makes every
 * wave leave, and the kernel then stores a code into a host-mapped error
 * word instead of finishing silently.  That word is reported as MGCN_EDEVICE
 * (+ mgcn_last_error naming the kernel) by the next mgcn_spmm_xw_* call, or
 * here: sync != 0 synchronises `stream` first, so every launch issued on it
 * before this call is covered.  Reading the word clears it.  No reference
 * counterpart (torch_scatter reports nothing from the device either). */
int mgcn_check_device(void *stream, int sync);

/* Tuning knobs (ABI 21: only knobs that keep every result within its tested
 * bound -- bit for bit, except gemm_precision).  Process-wide settings meant
 * to be set once at start-up (MGCN_OPTIONS="name=value,..." does that from
 * the environment), not per call; the defaults are the measured-fastest
 * forms.  Switches that change results (timing experiments: wide_dbg,
 * xw_ws_dbg) and the warp-specialised spin bound (ws_spin_limit) exist only
 * in the experiment build libmgcn_exp.so (make -C meta-gcn_amd/csrc exp);
 * this library rejects them (MGCN_EINVAL).
 *   "spmm_vec"    : cap the floats per lane of the SpMM gathers (1, 2, 4)
 *   "spmm_unroll" : gathers in flight per lane group (4, 8 or 16)
 *   "heavy_side_stream": 1 (default) runs the heavy-row launch on a side
 *                   stream concurrently with the lane-group launch; 0 serial
 *   "heavy_side_fence": 1 = system-scope events on that side stream
 *   "heavy_lds_kb": LDS per giant-row workgroup, 16..160 (default 160)
 *   "heavy_block" : threads per giant-row workgroup, 256/512/1024 (1024)
 *   "heavy_mid_lds_kb": LDS per (non-giant) heavy-row workgroup (default 40)
 *   "heavy_mid_q1": 1 (default) = one edge quad in flight per producer in the
 *                   non-giant heavy-row workgroups when a row is <= 32 floats
 *                   wide (fewer registers, more workgroups per CU); 0 = four
 *   "heavy_giant_thr" : degree above which a heavy row is giant, read by
 *                   mgcn_row_schedule (default 512)
 *   "residual_blocks": workgroup cap of the fused residual layer's launches
 *                   (default 8192; the backward's is also capped at 4096)
 *   "residual_fused_mask": 1 (default) the residual stack's lower-layer mask
 *                   pass fused into its launches
 *   "gemm_tn_variant": LDS-staged dW kernel chunk depth (M, N multiples of
 *                   128): 0 = 64 rows (default), 1 = 32, 2 = 16
 *   "gemm_tn_staged": 1 (default) the staged small-C kernel at M = 32
 *   "gemm_precision": product arithmetic of mgcn_gemm_nn / mgcn_gemm_tn:
 *                   1 = bf16x6 (default; fp32 operands split exactly into
 *                   three bf16 terms, six products on bf16 MFMA, fp32
 *                   accumulate -- fp32-level error), 0 = f32
 *                   MFMA (v_mfma_f32_32x32x2_f32)
 *   "spmm_xw_unroll": gathers in flight per row of the fused 128-wide layer
 *                   forward, 4 / 5 (default) / 6 / 8 (the two-phase adjoints:
 *                   8, else 4); every value folds in edge order (same bits)
 *   "xw_dyn_rounds": the last rounds of the 128-wide forward's chunks whose
 *                   workgroup is decided on the device (claimed from a
 *                   counter in the call's workspace, so that the workgroups
 *                   end together), 0 .. 64, default 8; 0 = every chunk goes
 *                   to workgroup c mod grid.  Per-row results: same bits.
 *                   (The warp-specialised forward, at half the grid, claims
 *                   twice as many rounds: the same chunks.)
 *   "xw_fwd_ws"   : 1 (default) = mgcn_spmm_xw_fwd at F = 128 on the
 *                   warp-specialised kernel where a workspace is given (one
 *                   workgroup per CU: 8 gather waves with the rolling gather,
 *                   8 MFMA waves, a ring of chunk images in LDS), 0 = the
 *                   two-phase kernel.  Same sums and products in the same
 *                   order: Y, Z and the mask words keep their bits.  (The
 *                   packed forward and calls without a workspace or with
 *                   "spmm_xw_unroll" off its default are always two-phase.)
 *   "xw_ws_full"  : 1 (default) = mgcn_spmm_xw_bwd's dW (+ dX) form on the
 *                   warp-specialised kernel (DWS), 0 = the two-phase kernel
 *   "xw_ws_max"   : 1 (default) = the max adjoint with dX on DWS as well
 *   "xw_ws_full_unroll": DWS gathers in flight per row, 4 / 5 (default) / 6
 *   "xw_ws_roll"  : how the sum / mean DWS gather waves issue those gathers:
 *                   0 = in batches (issue all, wait, fold), 2 (default) = a
 *                   slot takes its next load as soon as it is folded, and the
 *                   last slots of a row quad take the next quad's first.  Same
 *                   folds in the same order: same bits.  (The max adjoint
 *                   always gathers in batches.)
 *   "wide_ws"     : the 256-wide layer kernels: bit 0 the forward, bit 1 the
 *                   adjoint on the warp-specialised form (default 3), else
 *                   the 16-row two-phase form
 *   "wide_pair"   : the two-phase 256-wide form gathers a wave's two rows
 *                   together (bit 0 forward, bit 1 adjoint; default 3)
 *   "wide_mfma"   : MFMA waves of the warp-specialised 256-wide kernels, 4 / 8
 *                   (default)
 * (Measured-slower forms removed in round 6 live as patches under exp/.) */
int mgcn_set_option(const char *name, int value);

/* ------------------------------------------------------------------ graph */

/* Bytes of scratch mgcn_csr_build needs for `nnz` edges over `n` rows. */
size_t mgcn_csr_workspace_bytes(int64_t nnz, int64_t n);

/*
 * Build a CSR view of a COO edge list, grouping edges by `key` (pass
 * edge_index[1] = dst for the forward view, edge_index[0] = src for the
 * transposed view used by the backward pass).  Within a row the edges keep
 * their original (COO) order -- the order in which the reference's CPU
 * scatter_add / index_add_ accumulate -- so sums are reproduced bit for bit.
 *
 *   key[nnz], other[nnz] : int64 device arrays (rows of edge_index)
 *   rowptr[n + 1]        : int64 out
 *   col[nnz]             : int32 out, other[e] of each edge, row-grouped
 *   eid[nnz]             : int32 out, original edge id e of each CSR slot
 * Indices are validated: any key or other outside [0, n_key) / [0, n_other)
 * returns MGCN_EINDEX (this call synchronises `stream` once to check).
 * Replaces: COO edge_index consumed by index_select/scatter at
 * gcn_base_models.py:211-237 on every forward.
 */
int mgcn_csr_build(const int64_t *key, const int64_t *other, int64_t nnz,
                   int64_t n_key, int64_t n_other, int64_t *rowptr,
                   int32_t *col, int32_t *eid, void *workspace,
                   size_t workspace_bytes, void *stream);

/*
 * Node degrees and their inverse powers (gcn_base_models.py:117-135).
 *   deg_in      : optional precomputed degrees [n] (the `deg` argument);
 *                 when NULL the degree is the sum of edge weights (or the
 *                 edge count) over the rows of the given CSR, which must be
 *                 grouped by SOURCE node (gcn_base_models.py:124-126 sums
 *                 over edge_index[0]); the sum runs in edge order.
 *   edge_weight : optional [nnz] weights in COO order (indexed through eid).
 *   method      : MGCN_NORM_SM -> dinv = 1/sqrt(deg), MGCN_NORM_RW -> 1/deg;
 *                 +inf results become 0 (gcn_base_models.py:135).
 *   deg_out     : [n] degree actually used (may alias deg_in)
 *   dinv_out    : [n]
 */
int mgcn_degree_norm(int64_t n, const int64_t *rowptr_src, const int32_t *eid_src,
                     const float *deg_in, const float *edge_weight, int method,
                     float *deg_out, float *dinv_out, void *stream);

/*
 * Per-slot edge weights of a CSR view (gcn_base_models.py:137-142), stored in
 * the CSR's own slot order so the SpMM streams them:
 *   SM, no edge_weight : dinv[src] * dinv[dst]
 *   SM, edge_weight    : (dinv[src] * ew) * dinv[dst]
 *   RW, no edge_weight : dinv[src]   (the reference scales x rows before the
 *                                     gather, :217-220; same products)
 *   RW, edge_weight    : dinv[src] * ew
 *   NONE, edge_weight  : ew          (PyG GraphConv/SAGEConv message weights)
 * rows_are_dst = 1 for the forward (dst-grouped) view, 0 for the transposed.
 */
int mgcn_edge_norm(int64_t n_rows, int64_t nnz, const int64_t *rowptr, const int32_t *col,
                   const int32_t *eid, int rows_are_dst, const float *dinv,
                   const float *edge_weight, int method, float *w_out,
                   void *stream);

/* ------------------------------------------------------------ aggregation */

/*
 * Forward aggregation over a dst-grouped CSR (rows = destinations):
 *   acc_i = reduce_{k in row i, in edge order} ( H[col_k, :] * w_k )
 *   SUM : acc_i                   MEAN : acc_i / max(deg_i, 1)
 *   MAX : max with fill -1e38, ties -> later edge; fill entries -> 0;
 *         argmax[i, f] = eid of the winning edge, -1 where the output was fill
 *   then  y = acc (+ bias[f]) ; if relu: y = y < 0 ? 0 : y
 * w may be NULL (unweighted).  H rows have stride ldh floats, Y rows ldy.
 * argmax: int32 [n_rows, F] (stride F) for MAX, ignored otherwise; and/or
 * win_mask (see mgcn_max_mask): MAX also writes every edge's winner bits at
 * its slot (argmax may then be NULL).
 * relu_mask (nullable; needs relu and F <= 128): uint32 [n_rows][4], bit b
 * of word v set iff y[i, 4 b + v] > 0 -- the ReLU mask mgcn_gemm_nn's dX
 * epilogue reads (16 B per row instead of the 4F-byte Z row).
 * No floating-point contraction: products and sums are rounded separately,
 * in edge order, exactly as the reference's mul + scatter_add sequence.
 */
int mgcn_spmm_fwd(int64_t n_rows, int32_t F, const int64_t *rowptr,
                  const int32_t *col, const int32_t *eid, const float *w,
                  const float *H, int64_t ldh, float *Y, int64_t ldy,
                  int reduce, const float *bias, int relu, int32_t *argmax,
                  uint32_t *win_mask, uint32_t *relu_mask, const int32_t *order,
                  int64_t n_heavy, int64_t n_giant, void *stream);

/* The ReLU mask of rows Z (layout as mgcn_spmm_fwd's relu_mask; F <= 128),
 * for callers whose Z was not produced by mgcn_spmm_fwd. */
int mgcn_relu_mask(int64_t n_rows, int32_t F, const float *Z, int64_t ldz,
                   uint32_t *relu_mask, void *stream);

/*
 * Adjoint aggregation over the transposed (src-grouped) CSR:
 *   dH_s = sum_{k in row s, in edge order} ( g_k * w_k ) [* row_scale_s]
 *   g_k  = dY[col_k, :]                         (SUM)
 *        = dY[col_k, :] / cnt[col_k]            (MEAN; cnt = max(in-deg, 1))
 *        = argmax[col_k, f] == eid_k ? dY : 0   (MAX; or bit f of the edge's
 *                       win_mask word, found through slot_map = mgcn_slot_map)
 * row_scale (nullable) is the RW post-scale dinv[src] (gcn_base_models.py:218).
 * If accumulate != 0 the result is added to dH (dH += ...), else stored.
 */
int mgcn_spmm_bwd(int64_t n_rows, int32_t F, const int64_t *rowptr_t,
                  const int32_t *col_t, const int32_t *eid_t, const float *w_t,
                  const float *row_scale, const float *dY, int64_t lddy,
                  float *dH, int64_t lddh, int reduce, const float *cnt,
                  const int32_t *argmax, const uint32_t *win_mask,
                  const int32_t *slot_map, int accumulate,
                  const int32_t *order, int64_t n_heavy, int64_t n_giant, void *stream);

/*
 * bf16 feature rows (additions to ABI 22, backward compatible).  H / Y (dY /
 * dH) hold bf16 bit patterns, leading dimensions are counted in elements;
 * edge weights, bias, row_scale and cnt stay fp32.  Contract: every element
 * is widened to fp32 (exact), the row is formed exactly as mgcn_spmm_fwd /
 * mgcn_spmm_bwd form it (same order, same roundings, fp32 accumulators), and
 * the fp32 result is rounded once, to nearest even, at the store -- the
 * output is bit for bit bf16(mgcn_spmm_fwd(float(H))); argmax and win_mask
 * are the fp32 entry point's.  The adjoint's MEAN divides every gathered dY
 * row by cnt in fp32 inside the kernel (pass the undivided dY).
 * Shapes: F % 8 == 0 and 16-byte aligned rows (pointers % 16 == 0, leading
 * dimensions % 8 == 0), as mgcn_spmm_bf16_supported reports; anything else is
 * MGCN_EINVAL.  (order, n_heavy, n_giant) as above: every row, however long,
 * is folded in edge order.
 */
int mgcn_spmm_bf16_supported(int32_t F, int64_t ld_in, int64_t ld_out);
int mgcn_spmm_fwd_bf16(int64_t n_rows, int32_t F, const int64_t *rowptr,
                       const int32_t *col, const int32_t *eid, const float *w,
                       const uint16_t *H, int64_t ldh, uint16_t *Y, int64_t ldy,
                       int reduce, const float *bias, int relu, int32_t *argmax,
                       uint32_t *win_mask, const int32_t *order, int64_t n_heavy,
                       int64_t n_giant, void *stream);
int mgcn_spmm_bwd_bf16(int64_t n_rows, int32_t F, const int64_t *rowptr_t,
                       const int32_t *col_t, const int32_t *eid_t, const float *w_t,
                       const float *row_scale, const uint16_t *dY, int64_t lddy,
                       uint16_t *dH, int64_t lddh, int reduce, const float *cnt,
                       const int32_t *argmax, const uint32_t *win_mask,
                       const int32_t *slot_map, const int32_t *order, int64_t n_heavy,
                       int64_t n_giant, void *stream);
/*
 * dY = Z > 0 ? dZ : 0 over contiguous bf16 [n_rows, F] (exact; written only
 * when relu != 0 and dY != NULL) and db[f] = sum_i dY[i, f] in fp32, in a
 * fixed order (when db != NULL; workspace of mgcn_colsum_workspace_bytes).
 */
int mgcn_relu_bwd_colsum_bf16(int64_t n_rows, int32_t F, const uint16_t *dZ,
                              const uint16_t *Z, int relu, uint16_t *dY, float *db,
                              void *workspace, size_t workspace_bytes, void *stream);

/*
 * Fused bf16 layer (addition to ABI 22, backward compatible): the aggregation
 * of bf16 rows and a 128 x 128 bf16 product in one launch, for both
 * directions of a layer.
 *   Zf = reduce_k float(X[col_k]) * w_k [/ cnt[col_k]] [/ max(count, 1)] [* row_scale[row]]
 *   Zb = bf16(Zf)                       (round to nearest even, once)
 *   Y  = bf16(epi(float(Zb) @ float(B or B^T) + bias)),  epi = optional ReLU
 * Zf is formed exactly as mgcn_spmm_fwd_bf16 / mgcn_spmm_bwd_bf16 form it, so
 * Zb has their bits; the product is one bf16 MFMA term accumulated in fp32
 * (every product exact) and Y is rounded once.  Deterministic.
 * Forward: the fwd view, w = w_fwd, B = W, reduce = SUM or MEAN (division by
 * max(count, 1)), bias / relu, Z (optional, [n_rows, 128]) receives Zb.
 * Adjoint (dX): the bwd view, w = w_bwd, row_scale, reduce = SUM, and for a
 * mean layer cnt (every gathered row divided by cnt[col], as
 * mgcn_spmm_bwd_bf16's MEAN), B = W with transpose_b = 1.
 * w, row_scale, cnt, bias and Z are NULL where unused.  Shapes: F_in = F_out
 * = 128 (mgcn_spmm_xw_bf16_supported), every leading dimension >= 128 and
 * % 8 == 0, X / B / Y / Z 16-byte aligned; cnt together with reduce != SUM,
 * or anything else, is MGCN_EINVAL.  Every row is folded by one 16-lane
 * group: meant for views without heavy rows.
 */
int mgcn_spmm_xw_bf16_supported(int32_t F_in, int32_t F_out, int reduce);
int mgcn_spmm_xw_bf16(int64_t n_rows, int32_t F_in, int32_t F_out, const int64_t *rowptr,
                      const int32_t *col, const float *w, const float *row_scale,
                      const float *cnt, const uint16_t *X, int64_t ldx, const uint16_t *B,
                      int64_t ldb, int transpose_b, const float *bias, int relu, uint16_t *Y,
                      int64_t ldy, uint16_t *Z, int64_t ldz, int reduce, void *stream);

/*
 * Row schedule (degree skew: the botnet graphs reach degree ~6k, config 3).
 * mgcn_row_schedule writes every row id into order[n_rows], by degree,
 * heaviest first (stable: equal degrees keep ascending ids), and returns
 * n_heavy = #rows with degree > heavy_thr and n_giant = #those with degree >
 * the "heavy_giant_thr" option; it synchronises `stream`.  Passed to
 * mgcn_spmm_fwd/bwd as (order, n_heavy, n_giant): each heavy row gets a whole
 * workgroup that gathers a batch of its edges in parallel and folds them per
 * feature in edge order (same bits) -- giant rows a 1024-thread workgroup with
 * the whole LDS of a CU on a side stream, the others a 256-thread one -- and
 * the lane-group kernel takes order[n_heavy, n_rows) longest first, so the
 * rows of one wave have similar degrees.  order = NULL: natural row order,
 * no heavy path (n_heavy, n_giant ignored).
 */
size_t mgcn_row_schedule_workspace_bytes(int64_t n_rows);
int mgcn_row_schedule(int64_t n_rows, const int64_t *rowptr, int64_t heavy_thr, int32_t *order,
                      int64_t *n_heavy_out, int64_t *n_giant_out, void *workspace,
                      size_t workspace_bytes, void *stream);

/*
 * Max aggregation adjoint without the per-edge argmax gather (config 4 max).
 * mgcn_max_mask: from the forward's argmax [n_rows, F], for every fwd row d
 * and edge slot k of it, bit f of win_mask[k * ceil(F/32) + f/32] =
 * (argmax[d, f] == eid[k]) -- the edges each output feature came from (16 B
 * per edge at F = 128); mgcn_spmm_fwd writes the same bits itself when given
 * win_mask.  mgcn_slot_map: slot_map[j] = the fwd slot of the edge in bwd
 * slot j (eid / eid_t of the two views; workspace
 * mgcn_slot_map_workspace_bytes).  mgcn_spmm_bwd(MAX, win_mask, slot_map)
 * then reads one word per edge, issued with the dY gather instead of after a
 * 4F-byte argmax row.  Same routing as argmax (torch_scatter 1.x scatter_max
 * backward), same bits.
 */
size_t mgcn_slot_map_workspace_bytes(int64_t nnz);
int mgcn_slot_map(int64_t nnz, const int32_t *eid, const int32_t *eid_t, int32_t *slot_map,
                  void *workspace, size_t workspace_bytes, void *stream);
int mgcn_max_mask(int64_t n_rows, int32_t F, const int64_t *rowptr, const int32_t *eid,
                  const int32_t *argmax, uint32_t *win_mask, void *stream);

/* ------------------------------------------------------------------ dense */

/* Bytes of scratch mgcn_gemm_tn needs. */
size_t mgcn_gemm_tn_workspace_bytes(int64_t K, int32_t M, int32_t N);

/*
 * C[M, N] = A^T B (accumulate != 0: C += A^T B) for row-major A [K, M] (row
 * stride lda) and B [K, N] (ldb), fp32 on MFMA (gemm_precision), K split over
 * the chip with a deterministic fixed-order reduction of the partials.
 * Replaces autograd's weight gradient of `torch.matmul(x, self.weight_node)`
 * (gcn_base_models.py:201): dW = x^T dH with K = number of nodes.
 */
int mgcn_gemm_tn(int64_t K, int32_t M, int32_t N, const float *A, int64_t lda,
                 const float *B, int64_t ldb, float *C, int64_t ldc, int accumulate,
                 void *workspace, size_t workspace_bytes, void *stream);

/*
 * mgcn_gemm_tn with the product's columns split over two outputs: columns
 * [0, N1) of A^T B go to C1 [M, N1] (row stride ldc1), columns [N1, N) go
 * TRANSPOSED to C2t [N - N1, M] (row stride ldc2t).  Workspace as
 * mgcn_gemm_tn(K, M, N).  Replaces the two weight gradients of a GCNModel
 * layer and its residual Linear (gcn_model.py:94-105: weight_node [F_in,
 * F_out] and the Linear's weight [F_out, F_in]) from ONE pass over x and
 * [dH | dS], each written in its parameter's own layout.
 */
int mgcn_gemm_tn_split(int64_t K, int32_t M, int32_t N, int32_t N1, const float *A, int64_t lda,
                       const float *B, int64_t ldb, float *C1, int64_t ldc1, float *C2t,
                       int64_t ldc2t, int accumulate, void *workspace, size_t workspace_bytes,
                       void *stream);

/*
 * C[M, N] = A[M, K] . B[K, N] for 1 <= K <= 8, N <= 128, B addressed as B[k * sbk +
 * n * sbn] (W or W^T): the products accumulated in k order on fma.  Replaces
 * `torch.matmul` where the contraction is a handful of features (a 1 -> F
 * input layer, gcn_model.py:64-66; the F -> 2 projection's input gradient).
 */
int mgcn_gemm_small_k(int64_t M, int32_t K, int32_t N, const float *A, int64_t lda,
                      const float *B, int64_t sbk, int64_t sbn, float *C, int64_t ldc,
                      void *stream);

/* 1 if mgcn_gemm_nn handles this (K, N): every K, N >= 1 (ABI v15). */
int mgcn_gemm_nn_supported(int32_t K, int32_t N);
/* 1 if (K, N) takes the tuned tall-skinny kernel (K in {32, 64, 128, 256},
 * any N; A rows must also be 16-byte aligned): else the generic tiled one. */
int mgcn_gemm_nn_fast(int32_t K, int32_t N);
/* 1 if the fused ReLU-mask epilogue (relu_mask != NULL) is available for
 * (K, N): the tuned kernel with N <= 128. */
int mgcn_gemm_nn_epi_supported(int32_t K, int32_t N);
/* Bytes of scratch mgcn_gemm_nn needs for its fused column sums. */
size_t mgcn_gemm_nn_workspace_bytes(int64_t M, int32_t N);

/*
 * C[M, N] = A[M, K] . B[K, N] on MFMA (gemm_precision: bf16x6 or f32); A
 * row-major (lda), B addressed as B[k * sbk + n * sbn] (so W or W^T).
 * K in {32, 64, 128, 256} with 16-byte aligned A rows: the tuned
 * tall-skinny kernel (B^T split once per workgroup into LDS, A streamed;
 * N wider than 128 (64 at K = 256) as XCD-local column groups); any other
 * shape: a generic 64 x 64-tiled kernel.  Replaces `torch.matmul(x,
 * self.weight_node)` (gcn_base_models.py:201), its input gradient
 * dX = dH W^T, and the Linear layers of the module surface.  If relu_mask
 * != NULL (mgcn_spmm_fwd / mgcn_relu_mask layout, the previous layer's
 * output Z > 0) the ReLU backward and bias gradient are fused into the
 * epilogue:
 *   C = Z > 0 ? A.B : 0,  colsum[n] = sum_m C[m, n]  (deterministic)
 * (gcn_model.py:196 + gcn_base_models.py:240-241 adjoints); with row_div
 * (mean aggregation, = max(in-degree, 1)) C is stored divided by it, the
 * column sums stay undivided (mgcn_gemm_nn_epi_supported shapes only).
 */
int mgcn_gemm_nn(int64_t M, int32_t K, int32_t N, const float *A, int64_t lda,
                 const float *B, int64_t sbk, int64_t sbn, float *C, int64_t ldc,
                 const uint32_t *relu_mask, const float *row_div, float *colsum,
                 void *workspace, size_t workspace_bytes, void *stream);

/* 1 if mgcn_gemm_bwd handles (F_in, F_out): 128 x 128 under bf16x6 precision. */
int mgcn_gemm_bwd_supported(int32_t F_in, int32_t F_out);
/* Bytes of scratch mgcn_gemm_bwd needs (split-K partials + column sums). */
size_t mgcn_gemm_bwd_workspace_bytes(int64_t M, int32_t F_in, int32_t F_out);

/*
 * Both dense adjoints of H = X W (gcn_base_models.py:201) from one pass over
 * X [M, F_in] (ldx) and dH [M, F_out] (lddh), W [F_in, F_out] row-major (ldw):
 *   dW  = X^T dH          (accumulate != 0: dW += X^T dH; deterministic split-K)
 *   dX  = dH W^T          (skipped when dX == NULL)
 * With relu_mask (mgcn_spmm_fwd layout; the lower layer's output > 0) the
 * ReLU backward and that layer's bias gradient are fused as in mgcn_gemm_nn:
 *   dX = mask ? dH W^T : 0 (stored / row_div[m] when row_div != NULL),
 *   colsum[n] = sum_m dX[m, n] (undivided).
 * With dX == NULL and colsum != NULL: colsum[n] = sum_m dH[m, n] (F_out
 * entries; the bias gradient when dH is a layer output's gradient).
 * Replaces autograd's two matmul adjoints of `torch.matmul(x, self.weight_node)`
 * plus the threshold_backward/sum of gcn_model.py:196 and
 * gcn_base_models.py:240-241 (mgcn_gemm_tn + mgcn_gemm_nn in one launch).
 */
int mgcn_gemm_bwd(int64_t M, int32_t F_in, int32_t F_out, const float *X, int64_t ldx,
                  const float *dH, int64_t lddh, const float *W, int64_t ldw,
                  float *dW, int64_t lddw, int accumulate, float *dX, int64_t lddx,
                  const uint32_t *relu_mask, const float *row_div, float *colsum,
                  void *workspace, size_t workspace_bytes, void *stream);

/* Bytes of scratch mgcn_gemm_bwd_dw_cs needs (ABI v20). */
size_t mgcn_gemm_bwd_dw_cs_workspace_bytes(int64_t M);

/*
 * mgcn_gemm_bwd's dW-only form at 128 x 128 (ABI v20) that also returns
 *   s_colsum[128] = sum over the M rows of S   (S [M, 128], lds, 16-byte rows)
 * streamed in the same pass: dW (+)= X^T dH, colsum (nullable) = dH's column
 * sums as mgcn_gemm_bwd.  A GCN stack folds its TOP layer's bias gradient
 * (the column sums of the upstream gradient, gcn_base_models.py:240) into the
 * BOTTOM layer's dW = Z^T dY pass this way, instead of a separate pass over
 * the upstream gradient.  Deterministic (fixed-order folds).
 */
int mgcn_gemm_bwd_dw_cs(int64_t M, const float *X, int64_t ldx, const float *dH, int64_t lddh,
                        float *dW, int64_t lddw, int accumulate, float *colsum, const float *S,
                        int64_t lds, float *s_colsum, void *workspace, size_t workspace_bytes,
                        void *stream);

/* ------------------------------------------------- fused layer forward */

/* 1 if mgcn_spmm_xw_fwd / _bwd handle (F_in, F_out, reduce): 128 x 128 or
 * 256 x 256 (ABI v15), sum or mean, under bf16x6 precision.  At 256 the
 * backward is the dX-only form. */
int mgcn_spmm_xw_supported(int32_t F_in, int32_t F_out, int reduce);
/* 1 if mgcn_spmm_xw_bwd's dW-accumulating form and its max adjoint apply
 * (128 x 128 only). */
int mgcn_spmm_xw_bwd_full_supported(int32_t F_in, int32_t F_out);
/* Bytes of scratch mgcn_spmm_xw_fwd takes: at 128 the chunk counter and the
 * workgroups' mailbox words of the dynamic claim ("xw_dyn_rounds"; optional
 * there: without it every chunk is assigned statically), the split W image
 * at 256. */
size_t mgcn_spmm_xw_fwd_workspace_bytes(int32_t F_in, int32_t F_out);

/*
 * One GCN layer forward in one launch, aggregating before transforming:
 *   Y[i] = epi( (reduce_{k in row i} X[col_k] * w_k) . W + bias )
 * over the fwd CSR view (rowptr/col as mgcn_spmm_fwd; w nullable), X
 * [n_cols, F_in] (ldx, 16-byte aligned rows; under 4 GiB at F = 128, any
 * size at F = 256, whose kernel gives every gathered row a 64-bit base), W
 * [F_in, F_out] row-major (ldw),
 * reduce SUM or MEAN (divides the aggregated row by max(in-degree, 1)), epi =
 * optional ReLU, relu_mask (nullable, needs relu) in mgcn_spmm_fwd's layout.
 * Equals mgcn_gemm_nn (X W) followed by mgcn_spmm_fwd up to the association
 * of the sums (A (X W) = (A X) W for a linear aggregator): the reference's
 * `x @ weight_node` then gather / scale / scatter_add
 * (gcn_base_models.py:201, 223-241; PyG GCNConv x @ W then propagate) without
 * materialising X W.  Rows with heavy degree are handled, but slowly (one
 * lane group per row): callers route skewed graphs to the two-launch path.
 * Z (nullable, [n_rows, F_in], ldz, 16-byte aligned rows) receives the
 * aggregated rows before W -- for MEAN before the division -- so the
 * backward can form dW = Z^T dY' (dY' = dY pre-divided by the counts for
 * MEAN) with mgcn_gemm_bwd instead of a second gather over the graph
 * (the adjoint of `x @ weight_node`, gcn_base_models.py:201, reassociated).
 * At F = 256 (fused_wide.hip) W is split once per call into a fragment
 * image in `workspace` (mgcn_spmm_xw_fwd_workspace_bytes; at 128 the
 * workspace may be NULL: it only holds the dynamic claim's counter, and
 * without it the call runs the two-phase kernel, "xw_fwd_ws"; a hand-off of
 * the warp-specialised kernel that gives up is reported as MGCN_EDEVICE by
 * the next call), Y
 * needs 16-byte aligned rows, and relu_mask holds 8 words per row (feature f
 * at word 4 (f >> 7) + (f & 3), bit (f & 127) >> 2).
 */
int mgcn_spmm_xw_fwd(int64_t n_rows, int64_t n_cols, int32_t F_in, int32_t F_out, const int64_t *rowptr,
                     const int32_t *col, const float *w, const float *X, int64_t ldx,
                     const float *W, int64_t ldw, const float *bias, float *Y, int64_t ldy,
                     int reduce, int relu, uint32_t *relu_mask, float *Z, int64_t ldz,
                     void *workspace, size_t workspace_bytes, void *stream);

/* Bytes of scratch mgcn_spmm_xw_bwd needs (split-K partials + column sums;
 * at 256: the split W^T image + column-sum partials). */
size_t mgcn_spmm_xw_bwd_workspace_bytes(int64_t n_rows, int32_t F_in, int32_t F_out);

/*
 * One GCN layer backward in one launch (F_in = F_out = 128; sum / mean
 * aggregation, whose adjoint is a plain sum once dY is pre-divided):
 *   dH  = reduce_{k in row s} dY[col_k] * w_k  [* row_scale[s]]   (bwd view:
 *         rows = source nodes; = mgcn_spmm_bwd's dH, bit for bit)
 *   dW  = X^T dH   (accumulate != 0: dW += ...; deterministic split-K)
 *   dX  = dH W^T   with relu_mask / row_div / colsum as mgcn_gemm_bwd
 *         (skipped when dX == NULL)
 * dH is never written: it goes from the gather into LDS and through both
 * MFMA products.  Replaces mgcn_spmm_bwd + mgcn_gemm_bwd (the adjoints of
 * gcn_base_models.py:201-241: autograd's index_add of the gathered dY and
 * the two matmul adjoints, plus the ReLU / bias gradient of the layer below,
 * gcn_model.py:196).  dY rows [n_cols, 128] (lddy, 16-byte aligned, under
 * 4 GiB), X [n_rows, 128] (ldx, 16-byte aligned), W [128, 128] row-major.
 * Max (win_mask + slot_map, both or neither): the adjoint of
 * mgcn_spmm_fwd(MAX) -- each edge's dY row counts only at the features whose
 * winner it was (its bits in win_mask at its fwd slot slot_map[k], as
 * mgcn_spmm_bwd(MAX, win_mask, slot_map)); dH bit for bit that function's.
 * dX only: X == NULL and dW == NULL (dX required, no win_mask) -- the
 * gather, dX = dH W^T and its epilogue, nothing else; dX bit for bit the
 * full form's.  Pair with mgcn_spmm_xw_fwd's Z and mgcn_gemm_bwd (dW-only).
 * In the dX-only form `accumulate` != 0 ADDS the column sums into colsum
 * (colsum += ...; ABI v17), so the row chunks of one adjoint fold their bias
 * gradient on the device, in chunk order.
 * F = 256: the dX-only form only (dY any size: 64-bit row bases; relu_mask
 * in the 8-word layout of mgcn_spmm_xw_fwd at 256; dX 16-byte aligned rows).
 */
int mgcn_spmm_xw_bwd(int64_t n_rows, int64_t n_cols, int32_t F_in, int32_t F_out,
                     const int64_t *rowptr_t, const int32_t *col_t, const float *w_t,
                     const float *row_scale, const float *dY, int64_t lddy, const float *X,
                     int64_t ldx, const float *W, int64_t ldw, float *dW, int64_t lddw,
                     int accumulate, float *dX, int64_t lddx, const uint32_t *relu_mask,
                     const float *row_div, float *colsum, const uint32_t *win_mask,
                     const int32_t *slot_map, void *workspace, size_t workspace_bytes,
                     void *stream);

/*
 * The top layer's adjoint (ABI v19; F = 128, bf16x6): mgcn_spmm_xw_bwd's
 * dW + dX form (X, dW and dX required; no max) that also returns
 *   dy_colsum[128] = sum over the rows of dY   (the layer's own bias gradient,
 *                    autograd of `+ self.bias`, gcn_base_models.py:240)
 * from the launch that already streams dY -- each workgroup sums the dY rows
 * of its own row chunks beside the gathers -- so the top layer of a stack
 * needs neither a separate pass over dY nor the forward's Z and the dense
 * Z^T dY pass.  Needs n_rows == n_cols (every dY row is a row of the view:
 * a whole, square graph).  Runs the warp-specialised kernel (one workgroup
 * per CU); dX bit for bit mgcn_spmm_xw_bwd's; dW and the column sums folded
 * in a fixed order (deterministic).  Scratch: mgcn_spmm_xw_bwd_workspace_bytes.
 */
int mgcn_spmm_xw_bwd_hcs(int64_t n_rows, int64_t n_cols, const int64_t *rowptr_t,
                         const int32_t *col_t, const float *w_t, const float *row_scale,
                         const float *dY, int64_t lddy, const float *X, int64_t ldx,
                         const float *W, int64_t ldw, float *dW, int64_t lddw, int accumulate,
                         float *dX, int64_t lddx, const uint32_t *relu_mask, const float *row_div,
                         float *colsum, float *dy_colsum, void *workspace, size_t workspace_bytes,
                         void *stream);

/* ---------------------------------------------------- edge weight adjoint */

/*
 * Gradient of the per-edge message weights (the SDDMM of the aggregation's
 * adjoint): over the fwd view (rowptr / col: rows = destinations, col =
 * sources), for every slot k of row d
 *   dw[k] = sum_f dY[d, f] * H[col[k], f]   (MAX: only the features f whose
 *           winner slot k is, bit f of win_mask[k * ceil(F/32) + f/32])
 * in fwd slot order; dY as the SpMM adjoint receives it (mean: divided by the
 * in-degree).  This is what autograd of the reference's
 * `index_select(x, 0, src) * norm.view(-1, 1)` gives the norm
 * (gcn_base_models.py:217-224), from which degnorm_const's edge_weight / deg
 * gradients follow (gcn_base_models.py:102-140; chained by the host).
 * Deterministic; fp32 products, a fixed butterfly sum over features (the
 * reference's CPU sum order differs: equal to fp32 rounding, not bitwise).
 * 1 <= F <= 1024; H rows stride ldh, dY rows lddy.
 */
int mgcn_edge_weight_grad(int64_t n_rows, int32_t F, const int64_t *rowptr, const int32_t *col,
                          const float *H, int64_t ldh, const float *dY, int64_t lddy,
                          const uint32_t *win_mask, float *dw, void *stream);

/* ------------------------------------------------------- pooling support */

/*
 * Batched dense product (ABI v18), DiffPool's dense operators (PyG 1.3
 * DenseSAGEConv adj @ x @ weight and dense_diff_pool's S^T X, S^T A S, S S^T,
 * reference kernel/diff_pool.py:13-14, 68, 76):
 *   C[b][m][n] (+)= sum_k A[b][m][k] B[b][k][n]      (accumulate != 0: +=)
 * every operand addressed through (batch, row, column) element strides, so
 * transposed views need no copies; fp32 products and accumulation on MFMA.
 * batch <= 65535.
 */
int mgcn_gemm_batched(int64_t batch, int32_t M, int32_t N, int32_t K, const float *A, int64_t sab,
                      int64_t sam, int64_t sak, const float *B, int64_t sbb, int64_t sbk,
                      int64_t sbn, float *C, int64_t scb, int64_t scm, int64_t scn,
                      int accumulate, void *stream);

/* Bytes of scratch mgcn_edge_merge_greedy needs. */
size_t mgcn_edge_merge_workspace_bytes(int64_t n_nodes, int64_t n_edges);

/*
 * EdgePooling's edge contraction (PyG 1.3 EdgePooling.__merge_edges__, the
 * pool of reference kernel/edge_pool.py:19,42): walking the edges in `order`
 * (edge ids by descending score), an edge whose endpoints are both unmatched
 * is taken; taken edges become clusters 0..n_chosen-1 in walk order, the
 * unmatched nodes the clusters after them in ascending node order.  Built on
 * the device as the equivalent locally-dominant matching (same result bit for
 * bit).  src / dst: the two rows of edge_index (int64, E each); order: a
 * permutation of 0..E-1.  Outputs (device): cluster[N], chosen[0..n_chosen)
 * (edge ids, walk order; E entries of room), counts = {n_chosen, n_clusters}.
 * N, E < 2^31 - 1.
 */
int mgcn_edge_merge_greedy(int64_t n_nodes, int64_t n_edges, const int64_t *src, const int64_t *dst,
                           const int64_t *order, void *workspace, size_t workspace_bytes,
                           int64_t *cluster, int64_t *chosen, int64_t *counts, void *stream);

/* ----------------------------------------------------------- elementwise */

/* Bytes of scratch mgcn_relu_bwd_colsum needs. */
size_t mgcn_colsum_workspace_bytes(int64_t n_rows, int32_t F);

/*
 * ReLU backward + bias gradient in one pass over [n_rows, F]:
 *   dY = Z > 0 ? dZ : 0   (written only when relu != 0 or row_div != NULL,
 *                          and dY != NULL; divided by row_div[i] when given:
 *                          the mean aggregation's 1/count, applied once per
 *                          row instead of once per edge in the adjoint)
 *   db[f] = sum_i dY[i, f] (undivided; when db != NULL; deterministic)
 * Replaces autograd's threshold_backward + sum for `x + bias` then ReLU
 * (gcn_base_models.py:240-241, gcn_model.py:196).
 */
int mgcn_relu_bwd_colsum(int64_t n_rows, int32_t F, const float *dZ,
                         const float *Z, int relu, const float *row_div, float *dY,
                         float *db, void *workspace, size_t workspace_bytes,
                         void *stream);

/*
 * GCNModel's residual join (gcn_model.py:99-105, residual_hop = 1):
 *   Z = act(Z1 + (R + rbias))      act = ReLU if relu != 0 (layers before the
 * last, :103) else identity (:105); R = the residual Linear's x Wr^T (its
 * bias rbias may be NULL).  Replaces `xo + xr` and `self.non_linear(...)`.
 */
int mgcn_residual_act(int64_t n_rows, int32_t F, const float *Z1, int64_t ldz1,
                      const float *R, int64_t ldr, const float *rbias, int relu,
                      float *Z, int64_t ldz, void *stream);

/* Bytes of scratch mgcn_residual_act_bwd needs for its column sums. */
size_t mgcn_residual_act_bwd_workspace_bytes(int64_t n_rows, int32_t F);

/*
 * Adjoint of the residual join and of the layer's own ReLU in one pass:
 *   dS = relu ? (Z > 0 ? dZ : 0) : dZ          (written when dS != NULL)
 *   dA = relu1 ? (Z1 > 0 ? dS : 0) : dS        (stored / row_div[i] if given)
 *   colsums[0:F] = sum_i dA (undivided), colsums[F:2F] = sum_i dS
 * (deterministic; colsums may be NULL).  dA feeds the adjoint SpMM, dS the
 * residual Linear's gradients, the sums the two bias gradients.
 */
int mgcn_residual_act_bwd(int64_t n_rows, int32_t F, const float *dZ, int64_t lddz,
                          const float *Z, int64_t ldz, int relu, const float *Z1,
                          int64_t ldz1, int relu1, const float *row_div, float *dA,
                          int64_t ldda, float *dS, int64_t ldds, float *colsums,
                          void *workspace, size_t workspace_bytes, void *stream);

/*
 * GCNModel's INPUT layer with its residual Linear when in_channels = 1 (the
 * botnet node feature; GCNLayer(1, F) + residuals[0] + the join,
 * gcn_model.py:89-105 with residual_hop = 1) associated as (A x) W (ABI
 * v17): with a = A x (mgcn_spmm_fwd at F = 1; for MEAN already divided)
 *   Z[i][j] = relu2( relu1(a[i] W[j] + b[j]) + (x[i] Wr[j] + br[j]) )
 * W = weight_node [1][F], Wr = the Linear weight [F][1] (contiguous: F
 * floats each), b / br nullable; Z [n_rows][F] (ldz, 16-byte aligned rows).
 * The reference's A (x W) to fp32 rounding, without an F-wide gather.
 * Supported: F_in = 1, F / 4 a power of two, 4 <= F <= 256.
 */
int mgcn_input_layer_supported(int32_t F_in, int32_t F);
int mgcn_input_layer_fwd(int64_t n_rows, int32_t F, const float *a, const float *x,
                         const float *W, const float *b, const float *Wr, const float *br,
                         int relu1, int relu2, float *Z, int64_t ldz, void *stream);
/* Bytes of scratch mgcn_input_layer_bwd needs (block partials of 4 F sums). */
size_t mgcn_input_layer_bwd_workspace_bytes(int64_t n_rows, int32_t F);
/*
 * Its adjoint in one pass over dZ (and Z when relu2): dS = relu2' dZ, dA =
 * relu1' dS (relu1's decision recomputed bit for bit), and
 *   grads[0:F] = dW = sum_i a[i] dA[i]    grads[F:2F]  = db  = sum_i dA[i]
 *   grads[2F:3F] = dWr = sum_i x[i] dS[i] grads[3F:4F] = dbr = sum_i dS[i]
 * (deterministic fixed-order sums).  da / dxr (nullable, together): da[i] =
 * sum_j dA[i][j] W[j] [/ row_div[i]] -- the input of the 1-wide adjoint
 * SpMM (dx = A^T da + dxr) -- and dxr[i] = sum_j dS[i][j] Wr[j].
 */
int mgcn_input_layer_bwd(int64_t n_rows, int32_t F, const float *dZ, int64_t lddz,
                         const float *Z, int64_t ldz, const float *a, const float *x,
                         const float *W, const float *b, const float *Wr, int relu1, int relu2,
                         const float *row_div, float *da, float *dxr, float *grads,
                         void *workspace, size_t workspace_bytes, void *stream);

/*
 * One GCNModel layer with its residual Linear, F = 32 (the botnet stack of
 * config 3: GCNLayer + residuals[n] + the join, gcn_model.py:89-105 with
 * residual_hop = 1; NodeModelAdditive.forward gcn_base_models.py:199-243):
 *   Z1 = relu1((A X) W + bias),  Z = relu2(Z1 + (X Wr^T + rbias))
 * in one pass over the rows (fwd view: rows = destinations; order / n_heavy /
 * n_giant its row schedule, as mgcn_spmm_fwd).  W is [F][F] (H = X W), Wr
 * the Linear weight [out][in]; bias / rbias may be NULL; reduce SUM or MEAN.
 * masks[2 i] / masks[2 i + 1]: bit c <=> Z1[i][c] > 0 / Z[i][c] > 0
 * (the activations the backward needs).  Z must not alias X.  Replaces the
 * reference's x @ W, gather / scale / scatter_add, + b, ReLU, the residual
 * Linear, `xo + xr` and the join's ReLU.
 */
int mgcn_residual_layer_supported(int32_t F_in, int32_t F_out, int reduce);
int mgcn_residual_layer_fwd(int64_t n_rows, int32_t F, const int64_t *rowptr,
                            const int32_t *col, const int32_t *eid, const float *w,
                            const float *X, int64_t ldx, const float *W, int64_t ldw,
                            const float *bias, const float *Wr, int64_t ldwr,
                            const float *rbias, int reduce, int relu1, int relu2,
                            float *Z, int64_t ldz, uint32_t *masks, const int32_t *order,
                            int64_t n_heavy, int64_t n_giant, void *stream);

/* Bytes of scratch mgcn_residual_layer_bwd needs (dA rows + column sums). */
size_t mgcn_residual_layer_bwd_workspace_bytes(int64_t n_rows, int32_t F);

/*
 * Its adjoint (bwd view: rows = sources; row_scale the 'rw' post-scale,
 * row_div the in-degree divisor for MEAN, both nullable):
 *   dS = relu2' dZ,  dA = relu1' dS [/ row_div]        (from masks)
 *   DH[:, 0:F] = dH = A^T dA,  DH[:, F:2F] = dS         (lddh >= 2F)
 *   dX = dH W^T + dS Wr
 *   colsums[0:F] = sum_i dA (undivided: the bias gradient), [F:2F] = sum_i dS
 * [dW | dWr^T] = X^T DH is then one mgcn_gemm_tn_split.  dH is bit for bit
 * mgcn_spmm_bwd's of dA.  masks is read as 8-byte pairs: 8-byte aligned, like
 * the forward's (else MGCN_EINVAL).
 */
int mgcn_residual_layer_bwd(int64_t n_rows, int32_t F, const int64_t *rowptr_t,
                            const int32_t *col_t, const int32_t *eid_t, const float *w_t,
                            const float *row_scale, const float *row_div, const float *dZ,
                            int64_t lddz, const uint32_t *masks, int relu1, int relu2,
                            const float *W, int64_t ldw, const float *Wr, int64_t ldwr,
                            float *dX, int64_t lddx, float *DH, int64_t lddh, float *colsums,
                            const int32_t *order, int64_t n_heavy, int64_t n_giant,
                            void *workspace, size_t workspace_bytes, void *stream);

/*
 * A stack of n_layers such layers in one call (GCNModel's 32 -> 32 layers):
 * layer l reads X0 (l = 0) or Z[l - 1] and writes Z[l] = Z + l n_rows F and
 * masks + 2 l n_rows; W / bias / Wr / rbias / relu1 / relu2 are host arrays
 * with one entry per layer (device pointers; bias / rbias arrays or entries
 * may be NULL).  The backward runs the layers top-down: dZ the top layer's
 * upstream gradient, dW[l] ([F][F]) and dWr[l] ([F][F], the Linear layout)
 * written per layer, sums + 2 F l = (bias | rbias gradient) of layer l, dX0
 * (nullable) the gradient of X0.  Bitwise the layer-by-layer calls.  Both
 * check (order, n_heavy, n_giant), the 8-byte alignment of masks and the
 * 16-byte alignment of X0 / dZ / dX0 rows before any launch (MGCN_EINVAL).
 */
int mgcn_residual_stack_fwd(int64_t n_rows, int32_t F, int32_t n_layers, const int64_t *rowptr,
                            const int32_t *col, const int32_t *eid, const float *w,
                            const float *X0, int64_t ldx, const float *const *W,
                            const float *const *bias, const float *const *Wr,
                            const float *const *rbias, int reduce, const int32_t *relu1,
                            const int32_t *relu2, float *Z, uint32_t *masks,
                            const int32_t *order, int64_t n_heavy, int64_t n_giant, void *stream);
size_t mgcn_residual_stack_bwd_workspace_bytes(int64_t n_rows, int32_t F);
int mgcn_residual_stack_bwd(int64_t n_rows, int32_t F, int32_t n_layers, const int64_t *rowptr_t,
                            const int32_t *col_t, const int32_t *eid_t, const float *w_t,
                            const float *row_scale, const float *row_div, const float *dZ,
                            int64_t lddz, const float *X0, int64_t ldx, const float *Z,
                            const uint32_t *masks, const int32_t *relu1, const int32_t *relu2,
                            const float *const *W, const float *const *Wr, float *dX0,
                            float *const *dW, float *const *dWr, float *sums,
                            const int32_t *order, int64_t n_heavy, int64_t n_giant,
                            void *workspace, size_t workspace_bytes, void *stream);

/*
 * Segment mean over contiguous node ranges (PyG global_mean_pool on a
 * collated Batch, kernel/gcn.py:29; GCNModel pred_on='graph',
 * gcn_model.py:112-123):  out[g, :] = sum_{i in [ptr[g], ptr[g+1])} x[i, :]
 *                                     / max(ptr[g+1] - ptr[g], 1)
 * summed in node order.
 */
int mgcn_segment_mean(int64_t n_seg, int32_t F, const int64_t *ptr,
                      const float *x, int64_t ldx, float *out, int64_t ldo,
                      void *stream);

/*
 * Zero-skipping row packing for the sharded path's table exchange
 * (mgcn.dist: the all-gathered tables between layers are ReLU outputs or
 * ReLU-masked gradients, about half +0.0 words; the reference is
 * single-device, so this replaces nothing of it -- it shrinks the exchange of
 * SURVEY.md §8(e)'s destination-range sharding).  A chunk of n rows of F
 * floats (F % 32 == 0, W = F / 32) travels as one int32 buffer (ABI 21)
 *   [hdr: n x W pairs (mask_w, pos_w)][vals: the rows' words that are not +0.0]
 * bit b of mask_w of a row <=> word 32 w + b is not +0.0 (bit-pattern test:
 * -0.0 / NaN travel as values); pos_w = index in vals of the row's first
 * value at or after word 32 w (offs[i] + the popcounts of mask_0 .. w-1).
 * mgcn_pack_rows_count writes the masks (hdr[2 (i W + w)]) and per-row
 * counts; the caller forms offs (exclusive prefix sum of counts);
 * mgcn_pack_rows_values writes vals and the positions (hdr[2 (i W + w) + 1]).
 * mgcn_unpack_rows expands n_seg such segments (segment p at buf + p
 * seg_words) into rows p n + i of T, bit for bit the packed rows; the fused
 * 256-wide layer kernels also gather straight from them
 * (mgcn_spmm_xw_fwd_packed / _bwd_packed).
 */
int mgcn_pack_rows_count(int64_t n, int32_t F, const float *X, int64_t ldx, uint32_t *hdr,
                         int32_t *counts, void *stream);
int mgcn_pack_rows_values(int64_t n, int32_t F, const float *X, int64_t ldx,
                          const int32_t *offs, uint32_t *hdr, uint32_t *vals, void *stream);
int mgcn_unpack_rows(int64_t n_seg, int64_t n, int32_t F, const uint32_t *buf, int64_t seg_words,
                     float *T, int64_t ldt, void *stream);

/*
 * The same packed chunk in ONE pass (ABI 22; F in {32, 64, 128, 256}): hdr
 * (masks and positions), vals and *total (device int64: the number of
 * values) from a single read of the rows -- a workgroup holds its tile of
 * rows in registers and takes its offset from its predecessors' published
 * counts (decoupled look-back), so neither the count pass's read nor the
 * host-side scan of the counts is needed.  Bit for bit the two-pass output.
 * workspace: mgcn_pack_rows_workspace_bytes(n, F) bytes, 16-byte aligned
 * (cleared by the call on `stream`).  A look-back that waits past the spin
 * bound reports MGCN_EDEVICE (see mgcn_check_device).
 */
size_t mgcn_pack_rows_workspace_bytes(int64_t n, int32_t F);
int mgcn_pack_rows(int64_t n, int32_t F, const float *X, int64_t ldx, uint32_t *hdr,
                   uint32_t *vals, int64_t *total, void *workspace, size_t workspace_bytes,
                   void *stream);

/*
 * A packed exchange table gathered in place (ABI 21; the fused 128- and
 * 256-wide layer kernels).  The zero-skipping exchange delivers a table of C row
 * chunks x P ranks as C * P packed segments of `seg_rows` rows each (the
 * layout above, segment s = c P + k at words + seg_base[s]); instead of
 * expanding them into a dense [C P seg_rows, F] table (mgcn_unpack_rows: a
 * write of the whole table and its re-read by the next layer), the gather
 * reads each needed row from its segment: one 8-B header pair per lane, then
 * the lane's nonzero words -- the bytes of the packed row only.  The view's
 * column indices address packed rows as col = (s << row_bits) | i (row i of
 * segment s; mgcn.dist builds these once per shard).  Results are bit for bit
 * those of the dense table (every +0.0 the packing skipped is folded as 0.0).
 * F = 128: the kernels read the whole table through ONE 32-bit range (the two
 * rows a wave gathers at once are addressed per lane), so every seg_base lies
 * in 0 .. n_words and n_words * 4 <= 2 GiB - 16 B (one receive buffer;
 * MGCN_EINVAL otherwise).  F = 256 (a wave per row, its address in SGPRs):
 * segments anywhere in one device's address space.
 */
typedef struct mgcn_packed_table {
  const uint32_t *words;   /* device: base the segment offsets count from */
  int64_t n_words;         /* words readable at `words` (loads past it read 0) */
  int32_t n_seg;           /* C * P segments, 1 .. 64 */
  int32_t seg_rows;        /* rows per segment (the chunk rows) */
  int32_t row_bits;        /* col = (s << row_bits) | i; seg_rows <= 2^row_bits */
  int32_t F;               /* row width (128 or 256) */
  int64_t seg_base[64];    /* word offset of segment s from `words` (host values,
                              passed to the kernels by value; the segments may
                              live in separate allocations of one device) */
} mgcn_packed_table;

/* mgcn_spmm_xw_fwd (F_in = F_out = 128 or 256, sum / mean) gathering X from a
 * packed table: Y = epi((A X) W + b) (+ Z = A X, + ReLU mask words) -- bit for
 * bit mgcn_spmm_xw_fwd on the unpacked table.  Scratch:
 * mgcn_spmm_xw_fwd_workspace_bytes(F, F). */
int mgcn_spmm_xw_fwd_packed(int64_t n_rows, int32_t F_in, int32_t F_out, const int64_t *rowptr,
                            const int32_t *col, const float *w, const mgcn_packed_table *X,
                            const float *W, int64_t ldw, const float *bias, float *Y,
                            int64_t ldy, int reduce, int relu, uint32_t *relu_mask, float *Z,
                            int64_t ldz, void *workspace, size_t workspace_bytes, void *stream);

/* mgcn_spmm_xw_bwd's dX-only form (F = 128 or 256) gathering dY from a packed
 * table: dX = relu'(lower) ((A^T dY [* row_scale]) W^T) [/ row_div], colsum
 * (+)= sum_rows dX -- bit for bit the dense-table call.  Scratch:
 * mgcn_spmm_xw_bwd_workspace_bytes(n_rows, F, F). */
int mgcn_spmm_xw_bwd_packed(int64_t n_rows, int32_t F_in, int32_t F_out, const int64_t *rowptr_t,
                            const int32_t *col_t, const float *w_t, const float *row_scale,
                            const mgcn_packed_table *dY, const float *W, int64_t ldw, float *dX,
                            int64_t lddx, const uint32_t *relu_mask, const float *row_div,
                            float *colsum, int accumulate, void *workspace,
                            size_t workspace_bytes, void *stream);

/* ------------------------------------------------- attention node model */

/*
 * Multi-head soft attention over a node's neighbourhood: the message passing
 * of NodeModelAttention (src/gcn_meta/models/graph_attention.py:60-117) with
 * the sparse softmax of src/gcn_meta/models/common.py:69-92, and its adjoint.
 * These entry points were added under ABI 22 without changing any existing
 * one (a backward-compatible addition: MGCN_ABI_VERSION stays 22).
 *
 * Hp = X W is [N, H C] (head h in columns [h C, h C + C), row stride ldh) and
 * a is the attention vector [H, 2C], contiguous (att_weight [1, H, 2C]).  For
 * edge k (j -> i):  z_k[h] = s_src[j,h] + s_dst[i,h],  e = act(z),
 *   alpha_k = exp(e_k - m) / (sum_group exp(e - m) + 1e-16),
 *   m = max(-1e16, max_group e),
 * the group being the row of the CSR view the call walks.  Per-edge arrays
 * (alpha, mask, dz) are [nnz, H] contiguous.  Supported: 1 <= H <= 16, C >= 1,
 * H C <= 1024, nnz H < 2^31, any leading dimension >= H C; anything else
 * returns MGCN_EINVAL before a launch.  n_rows == 0 is a successful no-op.
 * No atomics; rows keep COO order and every sum has a fixed order, so results
 * are bitwise repeatable (equal to the reference to fp32 rounding: its CPU
 * summation order differs).
 */
#define MGCN_ATT_ACT_NONE 0
#define MGCN_ATT_ACT_LRELU 1 /* LeakyReLU(0.2), common.py:27 */
#define MGCN_ATT_ACT_RELU 2

/* s_src[n,h] = sum_c Hp[n,h,c] a[h,c],  s_dst[n,h] = sum_c Hp[n,h,c] a[h,C+c]
 * ([n, H] contiguous); products summed per lane in column order, then a
 * fixed butterfly. */
int mgcn_att_scores(int64_t n, int32_t H, int32_t C, const float *Hp, int64_t ldh,
                    const float *a, float *s_src, float *s_dst, void *stream);

/*
 * The forward over a view whose rows are destinations (rowptr / col of the
 * fwd view; col = sources), in one launch:
 *   alpha_in == NULL:  z = s_row[row] + s_col[col]  (s_row = s_dst, s_col =
 *     s_src), the softmax over the row, alpha written in slot order;
 *   alpha_in != NULL:  alpha = alpha_in (att_dir = 'out': softmax taken over
 *     the source-grouped view by mgcn_edge_softmax and carried to fwd slot
 *     order); s_row / s_col / alpha are not used.
 *   Y[row,h,:] = sum_k alpha_k[h] mask_k[h] Hp[col_k,h,:]   (mask NULL: ones),
 * summed in slot (COO) order.  The stored alpha is the one before the mask.
 */
int mgcn_att_fwd(int64_t n_rows, int64_t nnz, int32_t H, int32_t C, const int64_t *rowptr,
                 const int32_t *col, const float *s_row, const float *s_col, int act,
                 const float *alpha_in, const float *mask, const float *Hp, int64_t ldh,
                 float *Y, int64_t ldy, float *alpha, void *stream);

/* The same logits and softmax over any view (groups = rows), no gather:
 * alpha in the view's slot order (the same device code as mgcn_att_fwd). */
int mgcn_edge_softmax(int64_t n_rows, int64_t nnz, int32_t H, const int64_t *rowptr,
                      const int32_t *col, const float *s_row, const float *s_col, int act,
                      float *alpha, void *stream);

/*
 * Adjoint by destination row (fwd view), from dY [N, H C]:
 *   dalpha_k[h] = mask_k[h] sum_c dY[row,h,c] Hp[col_k,h,c]   (per-head SDDMM)
 *   softmax == 0: dz := dalpha                                 (att_dir 'out')
 *   softmax != 0: dz_k = alpha_k (dalpha_k - sum_row alpha dalpha) act'(z_k),
 *                 ds_row[row,h] = sum_k dz_k[h]  (= ds_dst)    (att_dir 'in')
 * dz in fwd slot order.
 */
int mgcn_att_bwd_dst(int64_t n_rows, int64_t nnz, int32_t H, int32_t C, const int64_t *rowptr,
                     const int32_t *col, const float *Hp, int64_t ldh, const float *dY,
                     int64_t lddy, const float *alpha, const float *mask, const float *s_row,
                     const float *s_col, int act, int softmax, float *dz, float *ds_row,
                     void *stream);

/*
 * Adjoint by source row (the bwd view rowptr_t / col_t, col_t = destinations;
 * slot_map = mgcn_slot_map: the fwd slot of every bwd slot; alpha, mask and dz
 * are in fwd slot order):
 *   softmax != 0 (att_dir 'out'): dz (holding dalpha) is replaced in place by
 *     alpha (dalpha - sum_row alpha dalpha) act'(z), z = s_row[row] + s_col[col]
 *     (s_row = s_src, s_col = s_dst);
 *   ds_src[row,h] = sum_k dz_k[h]
 *   dHp[row,h,:] = sum_k alpha_k mask_k dY[col_k,h,:] + ds_src[row,h] a[h,:C]
 *                  (+ ds_dst[row,h] a[h,C:] when ds_dst != NULL: 'in', where
 *                  mgcn_att_bwd_dst has produced it; 'out': mgcn_att_dst_fold)
 */
int mgcn_att_bwd_src(int64_t n_rows, int64_t nnz, int32_t H, int32_t C, const int64_t *rowptr_t,
                     const int32_t *col_t, const int32_t *slot_map, const float *dY,
                     int64_t lddy, const float *alpha, const float *mask, float *dz,
                     const float *s_row, const float *s_col, int act, int softmax,
                     const float *a, const float *ds_dst, float *ds_src, float *dHp,
                     int64_t lddh, void *stream);

/* att_dir 'out', after mgcn_att_bwd_src: over the fwd view,
 * ds_dst[row,h] = sum_k dz_k[h]  and  dHp[row,h,:] += ds_dst[row,h] a[h,C:]. */
int mgcn_att_dst_fold(int64_t n_rows, int64_t nnz, int32_t H, int32_t C, const int64_t *rowptr,
                      const float *dz, const float *a, float *ds_dst, float *dHp, int64_t lddh,
                      void *stream);

/* -------------------------------------------- hard attention node model */

/*
 * Gumbel-softmax / argmax hard attention: the message passing of
 * NodeModelHardAttention (src/gcn_meta/models/graph_hard_attention.py:70-136)
 * and of VotePoolLayer (gpool_hard_attention.py:214-275).  Added under ABI 22
 * as the attention entries were (backward-compatible: the version stays 22);
 * the mgcn_att_* entries are unchanged and share their device code with these
 * through template parameters.  Shapes, limits, error behaviour and the
 * determinism guarantees are those of the attention entries above.
 *
 * Training: the logit of slot k is  l_k = (act(z_k) + noise_k) / T  (an fp32
 * add, then an fp32 divide), the softmax over the row is the one above with l
 * in the place of e.  noise is [nnz, H] in the slot order of the view the
 * call walks, NULL = zeros.  temperature must be > 0 (else MGCN_EINVAL).  With
 * noise == NULL and T == 1 every entry returns the bits of its mgcn_att_*
 * counterpart.
 */
int mgcn_hatt_fwd(int64_t n_rows, int64_t nnz, int32_t H, int32_t C, const int64_t *rowptr,
                  const int32_t *col, const float *s_row, const float *s_col, int act,
                  const float *noise, float temperature, const float *alpha_in,
                  const float *mask, const float *Hp, int64_t ldh, float *Y, int64_t ldy,
                  float *alpha, void *stream);

int mgcn_hatt_edge_softmax(int64_t n_rows, int64_t nnz, int32_t H, const int64_t *rowptr,
                           const int32_t *col, const float *s_row, const float *s_col, int act,
                           const float *noise, float temperature, float *alpha, void *stream);

/* mgcn_att_bwd_dst / mgcn_att_bwd_src with the 1 / T of the logit:
 *   dz_k = alpha_k (dalpha_k - sum_row alpha dalpha) / T  act'(z_k).
 * act' depends on z alone, so the noise is not an argument.  ds, the dHp
 * terms, mgcn_att_dst_fold for 'out' and da are as for soft attention. */
int mgcn_hatt_bwd_dst(int64_t n_rows, int64_t nnz, int32_t H, int32_t C, const int64_t *rowptr,
                      const int32_t *col, const float *Hp, int64_t ldh, const float *dY,
                      int64_t lddy, const float *alpha, const float *mask, const float *s_row,
                      const float *s_col, int act, int softmax, float temperature, float *dz,
                      float *ds_row, void *stream);

int mgcn_hatt_bwd_src(int64_t n_rows, int64_t nnz, int32_t H, int32_t C, const int64_t *rowptr_t,
                      const int32_t *col_t, const int32_t *slot_map, const float *dY,
                      int64_t lddy, const float *alpha, const float *mask, float *dz,
                      const float *s_row, const float *s_col, int act, int softmax,
                      float temperature, const float *a, const float *ds_dst, float *ds_src,
                      float *dHp, int64_t lddh, void *stream);

/*
 * Eval: the winner of every (row, head) of any view (groups = rows) among
 * l_k = act(z_k) + noise_k  (z = s_row[row] + s_col[col]; noise NULL = none;
 * no temperature).  The tie rule is torch_scatter 1.x's CPU scan: start from
 * -1e16f, `l >= best` replaces the winner, so the last slot in slot (COO)
 * order among equal maxima wins; a value below -1e16f or a NaN never wins; an
 * empty row has no winner.  alpha [nnz, H] in the view's slot order receives
 * the one-hot (every entry is written, 1.0f or 0.0f), winner [n_rows, H] the
 * winning slot or -1.
 */
int mgcn_hatt_select(int64_t n_rows, int64_t nnz, int32_t H, const int64_t *rowptr,
                     const int32_t *col, const float *s_row, const float *s_col, int act,
                     const float *noise, float *alpha, int32_t *winner, void *stream);

/*
 * Y[row,h,:] = sum_k alpha_k[h] Hp[col_k,h,:] over the fwd view, alpha [nnz, H]
 * in fwd slot order, terms added in slot order.  The feature row of a slot
 * whose H coefficients are all zero is not loaded (a wave-uniform test).  For
 * finite Hp the result is bit for bit mgcn_att_fwd(alpha_in = alpha, mask =
 * NULL).  Non-finite Hp is outside the contract: a skipped 0 * inf stays 0
 * where the reference's dense product would give NaN.
 */
int mgcn_hatt_gather(int64_t n_rows, int64_t nnz, int32_t H, int32_t C, const int64_t *rowptr,
                     const int32_t *col, const float *alpha, const float *Hp, int64_t ldh,
                     float *Y, int64_t ldy, void *stream);

/* ---------------------------- attention and hard attention on bf16 rows */

/*
 * The _bf16 sibling of every attention / hard-attention entry that reads or
 * writes a feature row.  Added under ABI 22 without changing any existing
 * entry (backward-compatible: MGCN_ABI_VERSION stays 22).  mgcn_edge_softmax,
 * mgcn_hatt_edge_softmax and mgcn_hatt_select touch fp32 scores alone and
 * serve both row types.
 *
 * bf16 (bit patterns as uint16_t; leading dimensions counted in elements):
 * Hp, Y, dY, dHp.  fp32 as in the entries above: s_src / s_dst, alpha, mask,
 * noise, dz, ds_src / ds_dst and the attention vector a.
 *
 * Contract (that of mgcn_spmm_fwd_bf16): a loaded bf16 element is widened to
 * fp32 exactly; every value is then formed by the operations of the fp32
 * entry in the same order; each bf16 output element is rounded once, to
 * nearest even, at its store.  So every fp32 output (scores, alpha, dz, ds)
 * has the bits of the fp32 entry called on the upcast rows, and every bf16
 * output the bits of the fp32 entry's output rounded to bf16.
 *
 * Shapes, limits, error behaviour and determinism are those of the fp32
 * entries: 1 <= H <= 16, C >= 1, H C <= 1024, any leading dimension >= H C
 * and any element offset (rows need no alignment beyond the 2 bytes of an
 * element: every row access is a 2-byte load or store).
 *
 * att_dir 'out': mgcn_att_bwd_src stores dHp and mgcn_att_dst_fold adds a
 * term to it, which would round a bf16 row twice.  With dHp_f32 != NULL
 * ([n_rows, H C] fp32, contiguous, caller-provided) mgcn_att_bwd_src_bf16 /
 * mgcn_hatt_bwd_src_bf16 park the unrounded row there and do not touch dHp
 * (which may then be NULL); mgcn_att_dst_fold_bf16 reads it, adds its term in
 * fp32 and stores the row to dHp, rounded once.  With dHp_f32 == NULL ('in',
 * and the eval branch of hard attention) the row is rounded and stored to dHp
 * by mgcn_att_bwd_src_bf16 itself.
 */
int mgcn_att_scores_bf16(int64_t n, int32_t H, int32_t C, const uint16_t *Hp, int64_t ldh,
                         const float *a, float *s_src, float *s_dst, void *stream);

int mgcn_att_fwd_bf16(int64_t n_rows, int64_t nnz, int32_t H, int32_t C, const int64_t *rowptr,
                      const int32_t *col, const float *s_row, const float *s_col, int act,
                      const float *alpha_in, const float *mask, const uint16_t *Hp, int64_t ldh,
                      uint16_t *Y, int64_t ldy, float *alpha, void *stream);

int mgcn_att_bwd_dst_bf16(int64_t n_rows, int64_t nnz, int32_t H, int32_t C,
                          const int64_t *rowptr, const int32_t *col, const uint16_t *Hp,
                          int64_t ldh, const uint16_t *dY, int64_t lddy, const float *alpha,
                          const float *mask, const float *s_row, const float *s_col, int act,
                          int softmax, float *dz, float *ds_row, void *stream);

int mgcn_att_bwd_src_bf16(int64_t n_rows, int64_t nnz, int32_t H, int32_t C,
                          const int64_t *rowptr_t, const int32_t *col_t, const int32_t *slot_map,
                          const uint16_t *dY, int64_t lddy, const float *alpha, const float *mask,
                          float *dz, const float *s_row, const float *s_col, int act, int softmax,
                          const float *a, const float *ds_dst, float *ds_src, uint16_t *dHp,
                          int64_t lddh, float *dHp_f32, void *stream);

/* dHp[row,h,:] = round(dHp_f32[row,h,:] + ds_dst[row,h] a[h,C:]) */
int mgcn_att_dst_fold_bf16(int64_t n_rows, int64_t nnz, int32_t H, int32_t C,
                           const int64_t *rowptr, const float *dz, const float *a, float *ds_dst,
                           const float *dHp_f32, uint16_t *dHp, int64_t lddh, void *stream);

int mgcn_hatt_fwd_bf16(int64_t n_rows, int64_t nnz, int32_t H, int32_t C, const int64_t *rowptr,
                       const int32_t *col, const float *s_row, const float *s_col, int act,
                       const float *noise, float temperature, const float *alpha_in,
                       const float *mask, const uint16_t *Hp, int64_t ldh, uint16_t *Y,
                       int64_t ldy, float *alpha, void *stream);

int mgcn_hatt_bwd_dst_bf16(int64_t n_rows, int64_t nnz, int32_t H, int32_t C,
                           const int64_t *rowptr, const int32_t *col, const uint16_t *Hp,
                           int64_t ldh, const uint16_t *dY, int64_t lddy, const float *alpha,
                           const float *mask, const float *s_row, const float *s_col, int act,
                           int softmax, float temperature, float *dz, float *ds_row,
                           void *stream);

int mgcn_hatt_bwd_src_bf16(int64_t n_rows, int64_t nnz, int32_t H, int32_t C,
                           const int64_t *rowptr_t, const int32_t *col_t, const int32_t *slot_map,
                           const uint16_t *dY, int64_t lddy, const float *alpha,
                           const float *mask, float *dz, const float *s_row, const float *s_col,
                           int act, int softmax, float temperature, const float *a,
                           const float *ds_dst, float *ds_src, uint16_t *dHp, int64_t lddh,
                           float *dHp_f32, void *stream);

int mgcn_hatt_gather_bf16(int64_t n_rows, int64_t nnz, int32_t H, int32_t C,
                          const int64_t *rowptr, const int32_t *col, const float *alpha,
                          const uint16_t *Hp, int64_t ldh, uint16_t *Y, int64_t ldy,
                          void *stream);

/* ------------------------------------------------ edge-gated node model */

/*
 * Edge-gated message passing: NodeModelAdditive with an EdgeGateProj /
 * EdgeGateFree gate (src/gcn_meta/models/gcn_base_models.py:229-232, 322-396)
 * after its x @ weight_node, and the adjoint.  Added under ABI 22 as the
 * attention entries were (backward-compatible: the version stays 22).
 *
 * Hx = X W is [N, C] (row stride ldh).  For edge k (j -> i):
 *   l_k = a[j] + c[i] + t_k,   g_k = sigmoid(l_k) = 1 / (1 + exp(-l_k)),
 *   m_k = g_k w_k Hx[j],       Y[i] = reduce_{k -> i} m_k  (+ bias, ReLU).
 * a = Hx w_src and c = Hx w_dst are per-node scores (mgcn_att_scores with
 * H = 1 and a = [w_src | w_dst]); t is a per-slot term [nnz] in fwd slot
 * order (edge features, free gates) or, with t_bcast != 0, one element read
 * from the device and added to every slot (a scalar bias: no host sync);
 * a, c and t are each NULL for an absent term (a and c together).  w are the
 * per-slot message weights (NULL: ones); they do not enter the gate.
 * Per-edge arrays (g, dl, dw, t, w, dg_in) are [nnz] in fwd slot order.
 * Supported: 1 <= C <= 1024, nnz < 2^31, any leading dimension >= C; anything
 * else returns MGCN_EINVAL before a launch.  n_rows == 0 is a successful
 * no-op.  rowptr entries are absolute slot indices, so a row range [r0, r1) is
 * the call with rowptr + r0, n_rows = r1 - r0 and the row-indexed arrays
 * advanced by the caller (mgcn_gate_fwd: c, Y, argmax; mgcn_gate_bwd_dst: dY,
 * dc; mgcn_gate_bwd_src: row_scale, dc, da, dHx); column- and slot-indexed
 * arrays are passed as they are.  No atomics; slots keep
 * COO order and every sum has a fixed order: results are bitwise repeatable.
 */

/*
 * Forward over the fwd view (rows = destinations, col = sources):
 * g written in slot order, Y[row] = epi(reduce_k g_k w_k Hx[col_k]) with
 * reduce MGCN_REDUCE_SUM / MEAN (divided by max(degree, 1)) / MAX (`>=` in
 * slot order: the later slot wins ties; an empty row gives 0), then + bias
 * (NULL: none) and ReLU (relu != 0).  MAX writes argmax [n_rows, C]
 * (contiguous): the winning edge's id eid[slot], -1 for an empty row -- the
 * input of mgcn_max_mask; eid and argmax are not read otherwise.
 */
int mgcn_gate_fwd(int64_t n_rows, int64_t nnz, int32_t C, const int64_t *rowptr,
                  const int32_t *col, const int32_t *eid, const float *a, const float *c,
                  const float *t, int t_bcast, const float *w, const float *Hx, int64_t ldh,
                  int reduce, const float *bias, int relu, float *Y, int64_t ldy, float *g,
                  int32_t *argmax, void *stream);

/*
 * Adjoint by destination row (fwd view), from dY [N, C] (ReLU / bias already
 * taken back; mean: already divided by the row's count):
 *   s_k  = sum_f dY[row,f] Hx[col_k,f]     (win_mask != NULL, max: over the
 *          features whose winner bit of slot k is set)
 *   dw_k = g_k s_k                          (dw NULL: not wanted)
 *   dg_k = w_k s_k (+ dg_in[k]),   dl_k = dg_k g_k (1 - g_k)
 *   dc[row] = sum_k dl_k                    (dc NULL: not wanted)
 */
int mgcn_gate_bwd_dst(int64_t n_rows, int64_t nnz, int32_t C, const int64_t *rowptr,
                      const int32_t *col, const float *Hx, int64_t ldh, const float *dY,
                      int64_t lddy, const float *w, const float *g, const uint32_t *win_mask,
                      const float *dg_in, float *dl, float *dc, float *dw, void *stream);

/*
 * Adjoint by source row (the bwd view rowptr_t / col_t, col_t = destinations;
 * slot_map = mgcn_slot_map; g, dl and win_mask are in fwd slot order, w_t in
 * bwd slot order):
 *   da[row] = sum_k dl_k                                  (da NULL: not wanted)
 *   dHx[row] = (sum_k g_k w_t_k dY[col_k]) [* row_scale[row]]
 *              + da[row] w_sd[0:C] + dc[row] w_sd[C:2C]
 * (max: dY restricted to the slot's winner bits; the rank-one terms only for
 * da / dc given, w_sd = [w_src | w_dst] contiguous).
 */
int mgcn_gate_bwd_src(int64_t n_rows, int64_t nnz, int32_t C, const int64_t *rowptr_t,
                      const int32_t *col_t, const int32_t *slot_map, const float *dY,
                      int64_t lddy, const float *w_t, const float *row_scale, const float *g,
                      const float *dl, const uint32_t *win_mask, const float *w_sd,
                      const float *dc, float *da, float *dHx, int64_t lddh, void *stream);

/*
 * The three gate launches with the row schedule of the view they walk
 * (mgcn_row_schedule: order, n_heavy, n_giant; the fwd view's for
 * mgcn_gate_fwd_sched / mgcn_gate_bwd_dst_sched, the bwd view's for
 * mgcn_gate_bwd_src_sched).  Backward-compatible additions: MGCN_ABI_VERSION
 * stays 22.  The rows order[0, n_heavy) -- a hub of several thousand edges
 * would hold one wave for the whole launch -- go to workgroups: forward and
 * adjoint by source one workgroup per row (the SpMM's heavy-row body over a
 * per-slot coefficient g w; the first n_giant rows by the larger workgroup),
 * adjoint by destination one wave per 64-slot chunk of the row, then one wave
 * per row for dc.  The rows order[n_heavy, n_rows) stay on the wave-per-row
 * kernels.  Every output element has the bits the entry without a schedule
 * gives it; no atomics.  All launches are on `stream`.
 *
 * coef is the caller's scratch of nnz floats (g w of every slot of a heavy
 * row, in the slot order of the view walked; its contents after the call are
 * unspecified); required whenever order is given and nnz > 0.  The adjoint
 * by destination needs none.  order == NULL: exactly the entry without a
 * schedule (n_heavy, n_giant and coef are not read).  With order given,
 * 0 <= n_giant <= n_heavy <= n_rows, else MGCN_EINVAL; like every other
 * argument error, before any launch.  order holds each row of [0, n_rows)
 * once; a row range of a view cannot carry a schedule.
 */
int mgcn_gate_fwd_sched(int64_t n_rows, int64_t nnz, int32_t C, const int64_t *rowptr,
                        const int32_t *col, const int32_t *eid, const float *a, const float *c,
                        const float *t, int t_bcast, const float *w, const float *Hx,
                        int64_t ldh, int reduce, const float *bias, int relu, float *Y,
                        int64_t ldy, float *g, int32_t *argmax, const int32_t *order,
                        int64_t n_heavy, int64_t n_giant, float *coef, void *stream);

int mgcn_gate_bwd_dst_sched(int64_t n_rows, int64_t nnz, int32_t C, const int64_t *rowptr,
                            const int32_t *col, const float *Hx, int64_t ldh, const float *dY,
                            int64_t lddy, const float *w, const float *g,
                            const uint32_t *win_mask, const float *dg_in, float *dl, float *dc,
                            float *dw, const int32_t *order, int64_t n_heavy, int64_t n_giant,
                            void *stream);

int mgcn_gate_bwd_src_sched(int64_t n_rows, int64_t nnz, int32_t C, const int64_t *rowptr_t,
                            const int32_t *col_t, const int32_t *slot_map, const float *dY,
                            int64_t lddy, const float *w_t, const float *row_scale,
                            const float *g, const float *dl, const uint32_t *win_mask,
                            const float *w_sd, const float *dc, float *da, float *dHx,
                            int64_t lddh, const int32_t *order, int64_t n_heavy,
                            int64_t n_giant, float *coef, void *stream);

/*
 * The six gate entries on bf16 feature rows.  Added under ABI 22 as the
 * attention _bf16 siblings were, without changing any existing entry
 * (backward-compatible: MGCN_ABI_VERSION stays 22).
 *
 * bf16 (bit patterns as uint16_t; leading dimensions counted in elements):
 * Hx, Y, dY, dHx.  fp32 as in the entries above: a, c, t, w / w_t, row_scale,
 * g, dl, dc, da, dw, dg_in, bias, w_sd and the coef scratch.  argmax, win_mask
 * and slot_map are unchanged.
 *
 * Contract (that of mgcn_spmm_fwd_bf16 and of the attention siblings): a
 * loaded bf16 element is widened to fp32 exactly; every value is then formed
 * by the operations of the fp32 entry in the same order; each bf16 output
 * element is rounded once, to nearest even, at its store.  So g, dl, dc, da,
 * dw and argmax have the bits of the fp32 entry called on the upcast rows, and
 * Y and dHx the bits of the fp32 entry's output rounded to bf16.  dHx includes
 * the two rank-one terms da w_sd[0:C] + dc w_sd[C:2C]: they are added in fp32
 * before the single rounding, in the kernel that forms the row (wave kernel
 * and heavy-row workgroup alike).
 *
 * Arguments, their order, the nullable ones, the row-range use, the limits
 * (1 <= C <= 1024, nnz < 2^31, any leading dimension >= C), MGCN_EINVAL before
 * any launch, n_rows == 0 as a no-op, the absence of atomics and the fixed
 * summation orders are those of the fp32 entries.  Rows need no alignment
 * beyond the 2 bytes of an element (the wave kernels access single elements;
 * the heavy-row workgroups pick 8-, 4- or 2-byte gathers from the alignment of
 * the pointers and leading dimensions, per launch).
 *
 * Mean: the fp32 route divides the dY rows by their count once and hands the
 * divided fp32 rows to both adjoint entries; a bf16 dY cannot carry the
 * quotient without a second rounding.  The four adjoint entries therefore take
 * one more argument after the fp32 entry's arrays, cnt (nullable; fp32, indexed
 * by destination node, each >= 1; as mgcn_spmm_bwd_bf16 takes it): with cnt
 * given every loaded dY element is widened and divided by its destination's
 * count (IEEE division, round to nearest) before any other use --
 * mgcn_gate_bwd_dst_bf16 by cnt[row] (the row-range caller advances cnt with
 * dY), mgcn_gate_bwd_src_bf16 by cnt[col_k] of the gathered column -- so the
 * value entering every later operation is bit for bit the fp32 route's.  cnt
 * belongs to mean and win_mask to max: giving both is MGCN_EINVAL.
 *
 * The _sched_bf16 entries send order[0, n_heavy) through the workgroup path
 * with bf16 rows and the remaining rows through the wave kernels, with the
 * bits of the _bf16 entries without a schedule; coef stays fp32 [nnz].
 */
int mgcn_gate_fwd_bf16(int64_t n_rows, int64_t nnz, int32_t C, const int64_t *rowptr,
                       const int32_t *col, const int32_t *eid, const float *a, const float *c,
                       const float *t, int t_bcast, const float *w, const uint16_t *Hx,
                       int64_t ldh, int reduce, const float *bias, int relu, uint16_t *Y,
                       int64_t ldy, float *g, int32_t *argmax, void *stream);

int mgcn_gate_bwd_dst_bf16(int64_t n_rows, int64_t nnz, int32_t C, const int64_t *rowptr,
                           const int32_t *col, const uint16_t *Hx, int64_t ldh,
                           const uint16_t *dY, int64_t lddy, const float *w, const float *g,
                           const uint32_t *win_mask, const float *dg_in, float *dl, float *dc,
                           float *dw, const float *cnt, void *stream);

int mgcn_gate_bwd_src_bf16(int64_t n_rows, int64_t nnz, int32_t C, const int64_t *rowptr_t,
                           const int32_t *col_t, const int32_t *slot_map, const uint16_t *dY,
                           int64_t lddy, const float *w_t, const float *row_scale,
                           const float *g, const float *dl, const uint32_t *win_mask,
                           const float *w_sd, const float *dc, float *da, uint16_t *dHx,
                           int64_t lddh, const float *cnt, void *stream);

int mgcn_gate_fwd_sched_bf16(int64_t n_rows, int64_t nnz, int32_t C, const int64_t *rowptr,
                             const int32_t *col, const int32_t *eid, const float *a,
                             const float *c, const float *t, int t_bcast, const float *w,
                             const uint16_t *Hx, int64_t ldh, int reduce, const float *bias,
                             int relu, uint16_t *Y, int64_t ldy, float *g, int32_t *argmax,
                             const int32_t *order, int64_t n_heavy, int64_t n_giant, float *coef,
                             void *stream);

int mgcn_gate_bwd_dst_sched_bf16(int64_t n_rows, int64_t nnz, int32_t C, const int64_t *rowptr,
                                 const int32_t *col, const uint16_t *Hx, int64_t ldh,
                                 const uint16_t *dY, int64_t lddy, const float *w,
                                 const float *g, const uint32_t *win_mask, const float *dg_in,
                                 float *dl, float *dc, float *dw, const float *cnt,
                                 const int32_t *order, int64_t n_heavy, int64_t n_giant,
                                 void *stream);

int mgcn_gate_bwd_src_sched_bf16(int64_t n_rows, int64_t nnz, int32_t C,
                                 const int64_t *rowptr_t, const int32_t *col_t,
                                 const int32_t *slot_map, const uint16_t *dY, int64_t lddy,
                                 const float *w_t, const float *row_scale, const float *g,
                                 const float *dl, const uint32_t *win_mask, const float *w_sd,
                                 const float *dc, float *da, uint16_t *dHx, int64_t lddh,
                                 const float *cnt, const int32_t *order, int64_t n_heavy,
                                 int64_t n_giant, float *coef, void *stream);

/* ---------------------------------------- attention launches, heavy rows */

/*
 * The fp32 attention launches, soft and hard, with the row schedule of the
 * view they walk (mgcn_row_schedule: order, n_heavy, n_giant; the fwd view's
 * for the _fwd_sched and _bwd_dst_sched entries, the bwd view's for the
 * _edge_softmax_sched and _bwd_src_sched ones).  Backward-compatible
 * additions: MGCN_ABI_VERSION stays 22.  Each entry has the arguments of the
 * entry without a schedule, with (order, n_heavy, n_giant[, coef]) before the
 * stream.
 *
 * The rows order[0, n_heavy) -- a hub of several thousand edges would hold
 * one wave for the whole launch -- go to workgroups (the first n_giant of
 * them to the larger workgroup); the rows order[n_heavy, n_rows) stay on the
 * wave-per-row kernels.  Every output element (Y, alpha, dz, ds_row, ds_src,
 * dHp) has exactly the bits the entry without a schedule gives it: what a
 * (slot, head) contributes is formed by any thread, what a row sums is
 * summed in the wave kernel's order (its per-lane chains over the slots
 * c G + kl, its serial S chains, one chain per feature in slot order for the
 * gathers).  No atomics, no hand-off between workgroups; every launch is on
 * `stream`; the library allocates nothing.
 *
 *   _fwd_sched           one workgroup per heavy row: row max, sum exp,
 *                        alpha, coef = alpha mask, the weighted gather
 *                        (alpha_in given: coef and the gather only)
 *   _edge_softmax_sched  the same without the gather
 *   _bwd_dst_sched       the row's slots spread over waves (per-slot dots,
 *                        dz = mask dalpha'), then under softmax one
 *                        workgroup per row (S, the edge phase, ds_row)
 *   _bwd_src_sched       one workgroup per heavy row of the bwd view: coef,
 *                        S, under softmax the adjoint in place and ds_src,
 *                        the gather, the two rank-one terms
 *
 * coef is the caller's scratch of nnz H floats (alpha mask of every (slot,
 * head) of a heavy row, in the slot order of the view walked; its contents
 * after the call are unspecified); required whenever order is given and
 * nnz > 0.  The edge softmax and the adjoint by destination need none and do
 * not take it.  order == NULL: exactly the entry without a schedule
 * (n_heavy, n_giant and coef are not read).  With order given,
 * 0 <= n_giant <= n_heavy <= n_rows, else MGCN_EINVAL; like every other
 * argument error, before any launch.  order holds each row of [0, n_rows)
 * once.
 *
 * Kept on one wave per row: the _bf16 entries, mgcn_att_dst_fold,
 * mgcn_hatt_select / mgcn_hatt_gather, mgcn_att_scores (per node).
 */
int mgcn_att_fwd_sched(int64_t n_rows, int64_t nnz, int32_t H, int32_t C, const int64_t *rowptr,
                       const int32_t *col, const float *s_row, const float *s_col, int act,
                       const float *alpha_in, const float *mask, const float *Hp, int64_t ldh,
                       float *Y, int64_t ldy, float *alpha, const int32_t *order,
                       int64_t n_heavy, int64_t n_giant, float *coef, void *stream);

int mgcn_edge_softmax_sched(int64_t n_rows, int64_t nnz, int32_t H, const int64_t *rowptr,
                            const int32_t *col, const float *s_row, const float *s_col, int act,
                            float *alpha, const int32_t *order, int64_t n_heavy,
                            int64_t n_giant, void *stream);

int mgcn_att_bwd_dst_sched(int64_t n_rows, int64_t nnz, int32_t H, int32_t C,
                           const int64_t *rowptr, const int32_t *col, const float *Hp,
                           int64_t ldh, const float *dY, int64_t lddy, const float *alpha,
                           const float *mask, const float *s_row, const float *s_col, int act,
                           int softmax, float *dz, float *ds_row, const int32_t *order,
                           int64_t n_heavy, int64_t n_giant, void *stream);

int mgcn_att_bwd_src_sched(int64_t n_rows, int64_t nnz, int32_t H, int32_t C,
                           const int64_t *rowptr_t, const int32_t *col_t,
                           const int32_t *slot_map, const float *dY, int64_t lddy,
                           const float *alpha, const float *mask, float *dz, const float *s_row,
                           const float *s_col, int act, int softmax, const float *a,
                           const float *ds_dst, float *ds_src, float *dHp, int64_t lddh,
                           const int32_t *order, int64_t n_heavy, int64_t n_giant, float *coef,
                           void *stream);

int mgcn_hatt_fwd_sched(int64_t n_rows, int64_t nnz, int32_t H, int32_t C, const int64_t *rowptr,
                        const int32_t *col, const float *s_row, const float *s_col, int act,
                        const float *noise, float temperature, const float *alpha_in,
                        const float *mask, const float *Hp, int64_t ldh, float *Y, int64_t ldy,
                        float *alpha, const int32_t *order, int64_t n_heavy, int64_t n_giant,
                        float *coef, void *stream);

int mgcn_hatt_edge_softmax_sched(int64_t n_rows, int64_t nnz, int32_t H, const int64_t *rowptr,
                                 const int32_t *col, const float *s_row, const float *s_col,
                                 int act, const float *noise, float temperature, float *alpha,
                                 const int32_t *order, int64_t n_heavy, int64_t n_giant,
                                 void *stream);

int mgcn_hatt_bwd_dst_sched(int64_t n_rows, int64_t nnz, int32_t H, int32_t C,
                            const int64_t *rowptr, const int32_t *col, const float *Hp,
                            int64_t ldh, const float *dY, int64_t lddy, const float *alpha,
                            const float *mask, const float *s_row, const float *s_col, int act,
                            int softmax, float temperature, float *dz, float *ds_row,
                            const int32_t *order, int64_t n_heavy, int64_t n_giant, void *stream);

int mgcn_hatt_bwd_src_sched(int64_t n_rows, int64_t nnz, int32_t H, int32_t C,
                            const int64_t *rowptr_t, const int32_t *col_t,
                            const int32_t *slot_map, const float *dY, int64_t lddy,
                            const float *alpha, const float *mask, float *dz, const float *s_row,
                            const float *s_col, int act, int softmax, float temperature,
                            const float *a, const float *ds_dst, float *ds_src, float *dHp,
                            int64_t lddh, const int32_t *order, int64_t n_heavy, int64_t n_giant,
                            float *coef, void *stream);

/* --------------------------------------------------- multi-kernel layers */

/*
 * GCNMultiKernel's additive layer (src/gcn_meta/models/gcn_multi_kernel.py:
 * 76-114): K edge sets ("kernels") over one node set, each with its own
 * weight_node, normalisation and bias, combined by add, mean (sum / K) or
 * cat.  Added under ABI 22 as the attention and gate entries were
 * (backward-compatible: the version stays 22).
 *
 * All K views are square over the same N nodes (n_rows == n_cols == N).
 * H_all = x [W_0 | .. | W_{K-1}] is [N, K C] fp32 with row stride ldh; kernel
 * k gathers its column block [k C, (k + 1) C).  The per-kernel arrays travel
 * as one struct of pointer sets passed by value; entries k >= K are not read.
 *
 * Supported: 1 <= K <= MGCN_MULTI_MAX_K, reduce SUM / MEAN, any C >= 1 (the
 * vector width, 4 / 2 / 1 floats, is the widest that C, both leading
 * dimensions and both base addresses allow: block k starts k C floats into a
 * row), any leading dimension that holds the row; n_rows == 0 is a successful
 * no-op.  Anything else -- K outside the range, a view whose n_rows differs
 * from the call's, reduce MAX, a short leading dimension, a NULL array --
 * returns MGCN_EINVAL before a launch.  Rows are walked in natural order and
 * there is no heavy-row path: the caller routes graphs with heavy rows to the
 * per-kernel entries.  No atomics; slots keep COO order, kernels are combined
 * in index order, every product, sum and division is rounded on its own:
 * results are bitwise repeatable and equal the K single-kernel calls below.
 */
#define MGCN_MULTI_MAX_K 8
#define MGCN_COMBINE_ADD 0
#define MGCN_COMBINE_MEAN 1
#define MGCN_COMBINE_CAT 2

typedef struct mgcn_multi_views {
  int64_t n_rows[MGCN_MULTI_MAX_K];          /* rows of view k: must equal the call's n_rows */
  const int64_t *rowptr[MGCN_MULTI_MAX_K];   /* [n_rows + 1] */
  const int32_t *col[MGCN_MULTI_MAX_K];      /* [nnz_k] (may be NULL when nnz_k == 0) */
  const float *w[MGCN_MULTI_MAX_K];          /* [nnz_k] per-slot weights, NULL: ones */
  const float *bias[MGCN_MULTI_MAX_K];       /* forward: [C], NULL: none */
  const float *cnt[MGCN_MULTI_MAX_K];        /* adjoint, MEAN: max(in-degree_k, 1) [N] */
  const float *row_scale[MGCN_MULTI_MAX_K];  /* adjoint: [n_rows] post-scale, NULL: none */
} mgcn_multi_views;

/*
 * Forward over the K fwd views (rows = destinations).  For row i, feature f:
 *   for k = 0 .. K-1, in kernel order:
 *     s = 0; for the slots of view k's row i, in slot order:
 *       s = s + H_all[col, k C + f] * w_k[slot]
 *     reduce MEAN:  s = s / max(deg_k(i), 1)
 *     bias_k != NULL:  s = s + bias_k[f]
 *     combine ADD / MEAN:  y = (k == 0) ? s : y + s
 *     combine CAT:         Y[i, k C + f] = relu ? max(s, 0) : s
 *   combine MEAN:  y = y / (float)K
 *   ADD / MEAN:  Y[i, f] = relu ? max(y, 0) : y
 * i.e. mgcn_spmm_fwd per kernel on the column-block views, then the
 * reference's left-to-right `xo +=`, bit for bit.  A row that is empty in view
 * k contributes 0 + bias_k.  Y is [n_rows, C] (CAT: [n_rows, K C]), row
 * stride ldy.
 */
int mgcn_multi_spmm_fwd(int64_t n_rows, int32_t K, int32_t C, mgcn_multi_views views,
                        const float *H_all, int64_t ldh, float *Y, int64_t ldy, int reduce,
                        int combine, int relu, void *stream);

/*
 * Adjoint over the K bwd views (rows = sources, col = destinations, w in bwd
 * slot order).  For source row s, kernel k, feature f:
 *   acc = 0; for the slots of view k's row s, in slot order:
 *     g = dY[col, (CAT ? k C : 0) + f]
 *     combine MEAN:  g = g / (float)K
 *     reduce MEAN:   g = g / cnt_k[col]
 *     acc = acc + g * w_k[slot]
 *   dH_all[s, k C + f] = acc [* row_scale_k[s]]
 * i.e. K mgcn_spmm_bwd calls (SUM, or MEAN with cnt) on dY / comb_div (true
 * divisions) into the column blocks of dH_all [n_rows, K C], row stride lddh.
 * dY has the ReLU and bias already taken back.
 */
int mgcn_multi_spmm_bwd(int64_t n_rows, int32_t K, int32_t C, mgcn_multi_views views_t,
                        const float *dY, int64_t lddy, float *dH_all, int64_t lddh, int reduce,
                        int combine, void *stream);

/*
 * Derived plans: a CSR view of an edge subset of a graph that already has one
 * (derive.hip), without a sort, an index check or a host wait.  The child keeps
 * the parent's row grouping and the COO order inside each row, so its view is
 * a stable stream compaction of the parent's: flags, an exclusive prefix sum,
 * a scatter.  The result is what mgcn_csr_build gives for the filtered (and
 * relabelled) edge list.
 *
 * mgcn_edge_rank: eid_new[e] = rank of COO edge e among the surviving edges,
 * -1 where it is dropped; *total (a device word) = their number.  An edge
 * survives iff keep[e] != 0 (keep NULL: every edge) and, where node maps are
 * given, both endpoints map to >= 0.  An endpoint's map comes with the slots
 * (col, eid) of the view whose COLUMNS are that endpoint: map_a[col_a[k]] is
 * tested for edge eid_a[k] (the fwd view holds the sources, the bwd view the
 * destinations).  Either map may be NULL (no filter on that endpoint, its
 * view is not read).
 */
size_t mgcn_edge_rank_workspace_bytes(int64_t nnz);
int mgcn_edge_rank(int64_t nnz, const uint8_t *keep, const int32_t *col_a, const int32_t *eid_a,
                   const int32_t *map_a, const int32_t *col_b, const int32_t *eid_b,
                   const int32_t *map_b, int32_t *eid_new, int64_t *total, void *workspace,
                   size_t workspace_bytes, void *stream);

/*
 * mgcn_csr_derive: parent slot k of parent row p is kept iff
 * eid_new[eid[k]] >= 0.  Output rows r = 0 .. n_rows_out - 1 are the parent
 * rows row_src[r] (every kept slot must lie in one of them, each parent row
 * at most once); inside a row the kept slots keep the parent's order.
 * col_out = col_map[col[k]], eid_out = eid_new[eid[k]],
 * rowptr_out[n_rows_out] = nnz_out.  The parent's arrays are trusted (they
 * come from mgcn_csr_build); stores past nnz_out entries are suppressed.
 * nnz_in == 0 or nnz_out == 0: rowptr_out is zeroed, nothing else runs.
 */
size_t mgcn_csr_derive_workspace_bytes(int64_t n_rows_in, int64_t n_rows_out, int64_t nnz_in);
int mgcn_csr_derive(
    int64_t n_rows_in, int64_t n_cols_in, int64_t nnz_in,
    const int64_t *rowptr, const int32_t *col, const int32_t *eid, /* one view of the parent */
    const int32_t *row_src, /* [n_rows_out] parent row of each output row; NULL: identity */
    int64_t n_rows_out,
    const int32_t *col_map, /* [n_cols_in] new id of a parent column, -1: dropped; NULL: identity */
    const int32_t *eid_new, /* [nnz_in] new COO id of each parent COO edge, -1: dropped */
    int64_t nnz_out,        /* number of eid_new entries >= 0 */
    int64_t *rowptr_out, int32_t *col_out, int32_t *eid_out,
    void *workspace, size_t workspace_bytes, void *stream);

/*
 * Seeded per-edge random fills (edge_noise.hip): the Gumbel noise of hard
 * attention / VotePool and the attention dropout mask, written on the device
 * directly in the slot order of a view.  A backward-compatible addition:
 * MGCN_ABI_VERSION stays 22.
 *
 * out is [nnz, H], contiguous fp32.  Slot k belongs to COO edge e = eid[k]
 * (eid NULL: e = k, COO order), and out[k, h] depends on (kind, seed, offset,
 * e, h, p) alone: the fill of a view is the COO fill carried to its slots.
 *
 * u comes from Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl
 * constants 0x9E3779B9 / 0xBB67AE85) under the key (seed & 0xffffffff,
 * seed >> 32) and the counter (e, h / 4, offset & 0xffffffff, offset >> 32):
 * output word h % 4 serves head h, u = float(word >> 8) * 2^-24 (exact, so
 * 0 <= u <= 1 - 2^-24).
 *   UNIFORM  u
 *   GUMBEL   -logf(-logf(u + 1e-20f) + 1e-20f), the reference's fp32 operations
 *            in its order (graph_hard_attention.py:12-20); finite for every u
 *   DROPOUT  u >= p ? 1.0f / (1.0f - p) : 0.0f (one fp32 division): p == 0
 *            gives 1 everywhere, p == 1 gives 0 everywhere
 * p is read by DROPOUT alone.
 *
 * MGCN_EINVAL before any launch, out untouched: an unknown kind, nnz < 0,
 * H outside 1 .. 16, nnz * H >= 2^31, DROPOUT with p outside [0, 1] or NaN,
 * out NULL with nnz > 0.  nnz == 0 succeeds and launches nothing.  eid values
 * are not checked (they are a plan's own, from mgcn_csr_build).
 */
#define MGCN_NOISE_UNIFORM 0
#define MGCN_NOISE_GUMBEL 1
#define MGCN_NOISE_DROPOUT 2
int mgcn_edge_noise(int kind, uint64_t seed, uint64_t offset, int64_t nnz, int32_t H,
                    const int32_t *eid, float p, float *out, void *stream);

/*
 * Neighbour sampling (sample.hip): the COO keep mask that caps every
 * destination row at `fanout` neighbours drawn without replacement, for
 * mgcn_edge_rank / mgcn_csr_derive to turn into a child plan.  A
 * backward-compatible addition: MGCN_ABI_VERSION stays 22.
 *
 * The view is the fwd one (rows = destinations, col = sources, eid = COO ids).
 *   key(e)      output word 0, all 32 bits, of the Philox4x32-10 call that
 *               mgcn_edge_noise makes for head 0: key (seed & 0xffffffff,
 *               seed >> 32), counter (e, 0, offset & 0xffffffff, offset >> 32);
 *               key(e) >> 8 is UNIFORM's u of that edge times 2^24
 *   candidates  keep_loops != 0: an edge with col == row is no candidate, it
 *               is kept and does not count against the fan-out; keep_loops
 *               == 0: loops are candidates like any other edge
 *   selection   the candidates of a row ordered by (key(e), e) ascending, a
 *               strict total order; the first min(fanout, #candidates) are
 *               kept (fanout == 0: no candidate)
 *   row_mask    [n_rows] bytes or NULL: a row with row_mask[row] == 0 keeps
 *               nothing, loops included
 * keep [nnz] is in COO order and every entry is written, 0 or 1.  It is a
 * function of the arguments above alone -- integers only: not of the slot
 * order, of the route a row takes, of the launch shape or of the device.
 *
 * order / n_heavy: the view's row schedule (mgcn_row_schedule).  Rows
 * order[0, n_heavy) go one to a workgroup (a radix select of the fanout-th
 * smallest (key << 32) | e, any row length); rows order[n_heavy, n_rows) must
 * have at most 128 slots, the schedule's default threshold, and go to lane
 * groups.  order NULL (n_heavy 0): natural row order, and the rows above 128
 * slots are found by a walk over the row pointers: the same mask, slower.
 *
 * No workspace is needed (mgcn_sample_rows_workspace_bytes is 0 and workspace
 * may be NULL), nothing is allocated, the launches go to `stream`.
 * MGCN_EINVAL before any launch, keep untouched: n_rows < 0, nnz < 0, nnz >=
 * 2^31, fanout < 0, n_heavy outside [0, n_rows], order NULL with n_heavy > 0,
 * and with nnz > 0: keep, rowptr or eid NULL, col NULL with keep_loops.
 * nnz == 0 or n_rows == 0 succeeds and launches nothing.  rowptr, eid and
 * order are a plan's own (mgcn_csr_build) and are not validated; a store
 * whose COO id is outside [0, nnz) is suppressed.
 */
size_t mgcn_sample_rows_workspace_bytes(int64_t n_rows, int64_t nnz);
int mgcn_sample_rows(int64_t n_rows, int64_t nnz, const int64_t *rowptr, const int32_t *col,
                     const int32_t *eid, const int32_t *order, int64_t n_heavy,
                     const uint8_t *row_mask, int32_t fanout, int keep_loops, uint64_t seed,
                     uint64_t offset, uint8_t *keep, void *workspace, size_t workspace_bytes,
                     void *stream);

/*
 * Mini-batch blocks (block.hip): one hop of a sampled multi-hop frontier,
 * built in time proportional to the frontier -- no pass reads or writes an
 * array sized by the parent's nnz (node-sized ones: yes).  Backward-compatible
 * additions: MGCN_ABI_VERSION stays 22.
 *
 * dst [n_dst] int32 is the hop's destination list D (distinct parent node
 * ids, any order); the parent is given by its fwd view (rows = destinations,
 * col = sources, eid = COO ids), n_nodes rows and nnz slots.  The block's
 * edges are the slots mgcn_sample_rows keeps under (fanout, keep_loops, seed,
 * offset) with D as its row mask -- the same definition, byte for byte --,
 * ordered by (position of the row in D, slot order inside the row); a block
 * edge's id is its position.  Its nodes: D in list order (local ids 0 ..
 * n_dst - 1), then the other sources, ascending (n_dst .. n_src - 1).
 *
 * Three calls per hop on one stream with the same workspace
 * (mgcn_block_workspace_bytes(n_nodes, n_dst) bytes: it carries state from
 * one call to the next), the caller reading two device words in between to
 * size the outputs:
 *
 * mgcn_block_count   node_map [n_nodes]: D[i] -> i, every other node -1;
 *   rowptr_out [n_dst + 1]: the block's fwd row pointers; meta [5] int64 on
 *   the device: meta[0] = nnz_out (the block's edges), meta[1] = n_heavy (rows
 *   of D above 128 slots), meta[2] != 0: an id of D outside [0, n_nodes),
 *   meta[3] != 0: an id listed twice (the block of such a list is not
 *   defined; every store stays inside the arrays), meta[4] = 0.
 * mgcn_block_fill    nnz_out and n_heavy as read from meta.  src_out /
 *   eid_out [nnz_out] int32: the parent id of every block edge's source and
 *   its parent COO id; dst_out [nnz_out] int64: its destination's local id.
 *   meta[4] = the number of sources outside D.  Rows of D above 128 slots go
 *   one to a workgroup wherever they stand in the list; neither that nor the
 *   lane-group width changes a byte.
 * mgcn_block_relabel n_src = n_dst + meta[4].  node_map gains the new
 *   sources' local ids; src_ids [n_src] int64: the parent id of every local
 *   id; col_out [nnz_out] int32 and coo_src [nnz_out] int64: every block
 *   edge's source in local ids.  (coo_src, dst_out) is the block's COO list:
 *   its fwd view is (rowptr_out extended by its last entry to n_src + 1 rows,
 *   col_out, eid = 0 .. nnz_out - 1), its bwd view mgcn_csr_build of the list.
 *
 * Nothing is allocated and no call waits for the device.  MGCN_EINVAL before
 * any launch: a negative size, nnz, n_nodes or n_dst >= 2^31, fanout < 0,
 * nnz_out outside [0, nnz], n_heavy outside [0, n_dst], n_src outside [n_dst,
 * n_nodes], a NULL array that the sizes say is read or written;
 * MGCN_EWORKSPACE for a short workspace.  n_dst == 0, fanout == 0 and nnz ==
 * 0 succeed and describe empty blocks.  The parent's arrays are a plan's own
 * and are not validated.
 */
size_t mgcn_block_workspace_bytes(int64_t n_nodes, int64_t n_dst);
int mgcn_block_count(int64_t n_nodes, int64_t nnz, const int64_t *rowptr, const int32_t *col,
                     const int32_t *dst, int64_t n_dst, int32_t fanout, int keep_loops,
                     int32_t *node_map, int64_t *rowptr_out, int64_t *meta, void *workspace,
                     size_t workspace_bytes, void *stream);
int mgcn_block_fill(int64_t n_nodes, int64_t nnz, const int64_t *rowptr, const int32_t *col,
                    const int32_t *eid, const int32_t *dst, int64_t n_dst, int32_t fanout,
                    int keep_loops, uint64_t seed, uint64_t offset, const int64_t *rowptr_out,
                    int64_t nnz_out, int64_t n_heavy, const int32_t *node_map, int32_t *src_out,
                    int32_t *eid_out, int64_t *dst_out, int64_t *meta, void *workspace,
                    size_t workspace_bytes, void *stream);
int mgcn_block_relabel(int64_t n_nodes, const int32_t *dst, int64_t n_dst, int64_t n_src,
                       int64_t nnz_out, const int32_t *src_out, int32_t *node_map,
                       int64_t *src_ids, int32_t *col_out, int64_t *coo_src, void *workspace,
                       size_t workspace_bytes, void *stream);

/*
 * Aggregation on a mini-batch block (block_conv.hip): rectangular launches
 * over the block's own views, PyG's self-loop rules folded in, so no edge
 * list is edited and no plan is built.  Backward-compatible additions:
 * MGCN_ABI_VERSION stays 22.
 *
 * The block has n_dst destinations (local ids 0 .. n_dst - 1) among n_src
 * nodes, n_dst <= n_src.  `loops` says what a slot whose two ends are the same
 * node (an in-row self loop) does:
 *   MGCN_LOOPS_KEEP    it counts like any slot;
 *   MGCN_LOOPS_DROP    it adds nothing and its source row never reaches the
 *                      sum (PyG's remove_self_loops);
 *   MGCN_LOOPS_APPEND  dropped likewise, then one term X[i] * w_loop closes
 *                      row i (PyG 1.3's add_remaining_self_loops: w_loop = 1
 *                      without weights, else the weight of the row's last loop
 *                      slot, or `fill` where the row has none).
 *
 * mgcn_block_spmm_fwd  Y [n_dst, F] from X [n_src, F]: row i folded in slot
 *   order (= COO order) with separately rounded products and sums, as
 *   mgcn_spmm_fwd folds it; rowptr [n_dst + 1] is the head of the block's fwd
 *   row pointers, w (nullable) [nnz] in slot order.  MEAN divides by max(c, 1),
 *   c = the slots that counted (+ 1 under APPEND), written to cnt [n_dst]
 *   (nullable) as a float.  A row without counted slots gives 0 (KEEP / DROP)
 *   or X[i] * w_loop (APPEND).
 * mgcn_block_spmm_bwd  dX [n_src, F] from dY [n_dst, F] over the block's bwd
 *   view (rows = sources): per slot k the term g * w[eid_t[k]], g = dY[col_k]
 *   (MEAN: dY[col_k] / cnt[col_k], the forward's cnt), loop slots as above;
 *   under APPEND rows s < n_dst end with g(dY[s]) * w_loop.
 *
 * Any F >= 1 and leading dimensions >= F; rows of any length (a long row is
 * walked by its lane group).  No atomics, no workspace, nothing allocated.
 * MGCN_EINVAL before any HIP call: a negative size, n_dst > n_src, n_src >=
 * 2^31, F < 1, a leading dimension < F, reduce other than SUM / MEAN, a bad
 * `loops`, a NULL array that is read or written (col / col_t / eid_t may be
 * NULL for a block without edges), MEAN in the adjoint without cnt.
 */
enum { MGCN_LOOPS_KEEP = 0, MGCN_LOOPS_DROP = 1, MGCN_LOOPS_APPEND = 2 };
int mgcn_block_spmm_fwd(int64_t n_dst, int64_t n_src, int32_t F, const int64_t *rowptr,
                        const int32_t *col, const float *w, float fill, int loops, const float *X,
                        int64_t ldx, float *Y, int64_t ldy, int reduce, float *cnt, void *stream);
int mgcn_block_spmm_bwd(int64_t n_src, int64_t n_dst, int32_t F, const int64_t *rowptr_t,
                        const int32_t *col_t, const int32_t *eid_t, const float *w, float fill,
                        int loops, const float *dY, int64_t lddy, float *dX, int64_t lddx,
                        int reduce, const float *cnt, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MGCN_H */
