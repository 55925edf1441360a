// Internal helpers shared by the libmgcn translation units (not installed).
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "mgcn.h"

namespace mgcn {

void set_error(const char *fmt, ...);
void clear_error();

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

// Experiment builds (make exp -> libmgcn_exp.so, -DMGCN_EXPERIMENT=1) accept
// the timing-only switches that change results (wide_dbg, xw_ws_dbg) and a
// settable hand-off spin bound (ws_spin_limit); the product library compiles
// those switches out and rejects their names.
#ifndef MGCN_EXPERIMENT
#define MGCN_EXPERIMENT 0
#endif
constexpr int kDbgMask = MGCN_EXPERIMENT ? ~0 : 0;  // (a.dbg & kDbgMask): constant 0 in the product
constexpr int kSpinLimitDefault = 1 << 25;          // ~1 s of s_sleep(1) polls per hand-off

// Every mgcn_set_option knob: one field per option, named as the option, at
// its default.  options.hip holds the table of names and accepted values and
// is the only writer; include/mgcn.h says what each knob does.
struct Options {
  int spmm_vec = 0;  // cap of the floats per lane of the SpMM gathers (0: none)
  int spmm_unroll = 8;
  int spmm_unroll_set = 0;    // spmm_unroll given explicitly: every mode takes it
  int heavy_side_stream = 1;  // heavy-row launch on a side stream (concurrent)
  int heavy_side_fence = 0;   // 1 = system-scope events on that side stream
  // LDS per heavy workgroup (two product buffers + the metadata ring).  The
  // per-batch cost is about one gather round trip, so long rows want big
  // batches: a giant row's workgroup takes the whole 160 KB of a CU; the other
  // heavy rows (a few hundred edges) take little, so several share a CU.
  int heavy_lds_kb = 160;      // giant rows
  int heavy_mid_lds_kb = 40;   // other heavy rows
  int heavy_mid_q1 = 1;        // narrow rows: one edge quad in flight
  int heavy_block = 1024;      // threads per giant-row workgroup
  int heavy_giant_thr = 512;   // degree above which a heavy row is giant
  int residual_blocks = 8192;  // residual.hip: workgroups per light-row launch (grid-stride beyond)
  int residual_fused_mask = 1; // residual.hip: the stack's fused lower-layer mask pass
  // LDS-staged dW variants (gemm.hip; measured at K = 1M, M = N = 128: 0.321 /
  // 0.335 / 0.337 ms): 0 = BK 64, one workgroup per CU; 1 = BK 32, two; 2 =
  // BK 16, three
  int gemm_tn_variant = 0;
  int gemm_tn_staged = 1;  // M = 32, N = 32 / 64: gemm_tn_staged_kernel (0: gemm_tn_small_kernel)
  int gemm_precision = 1;  // gemm.hip: PREC_F32 0 / PREC_BF16X6 1 (gemm_precision_is_x6())
  int spmm_xw_unroll = 5;  // forward gathers in flight per row (5: config 2 5.06 -> 5.005 ms/step; 6 spills)
  // the forward's last rounds claimed from a counter (spmm_xw_fwd_kernel DYN;
  // 0: every chunk static)
  int xw_dyn_rounds = 8;
  // 1 = the 128-wide dense forward on spmm_xw_fwd_ws_kernel (default unroll,
  // a workspace given), 0 = two-phase
  int xw_fwd_ws = 1;
  int xw_ws_full = 1;  // the warp-specialised dW + dX adjoint (DWS)
  int xw_ws_max = 1;   // ... and its max adjoint (DWS + win_mask)
  int xw_ws_full_unroll = 5;  // DWS gathers in flight per row (5: 0.984-0.991 vs 1.000-1.012 ms at 4)
  // the sum / mean DWS gather waves' load schedule -- 0 batches, 2 a slot
  // refilled as it is folded, within a quad and into the next (config 2:
  // 4.72-4.73 vs 4.82-4.84 ms/step; 1, the refill within a quad alone, gained a
  // third of that and is removed: DESIGN section 4)
  int xw_ws_roll = 2;
  // fused_wide.hip: both rows of a wave's pair gathered together or one after
  // the other -- bit 0 the forward, bit 1 the adjoint (default 3: both paired)
  int wide_pair = 3;
  int wide_ws = 3;    // the 256-wide warp-specialised kernels -- bit 0 the forward, bit 1 the adjoint
  int wide_mfma = 8;  // MFMA waves of those kernels (4 or 8)
  // ---- experiment builds only (the product library rejects the names) ----
  int ws_spin_limit = kSpinLimitDefault;  // the warp-specialised kernels' hand-off bound (abort-path tests)
  // timing experiments on the 256-wide warp-specialised kernels (results are
  // WRONG when set): bit 0 the MFMA waves skip their W loads, bit 1 they skip
  // the products, bit 2 the gather waves skip the gathers; bits 3 / 4:
  // s_setprio 2 on the gather / MFMA waves (results stay exact)
  int wide_dbg = 0;
  // timing experiments on DWS (dW / dX WRONG when set): bit 0 skip the dW
  // products, bit 2 skip the X loads, bit 3 skip the W^T reads
  int xw_ws_dbg = 0;
  // packed-table forms: slots in flight per row (experiment builds sweep them;
  // config 2's shape, profiles/r06/packed_unroll_sweep.json: forward 1.20 / 1.27
  // / 1.39 / 1.41 ms at U = 3 / 4 / 5 / 6 -- the extra registers spill more as U
  // grows --, adjoint 1.07 / 1.05 / 1.08 ms at 2 / 3 / 4)
  int xw_pk_unroll = 3;
  int xw_pk_bwd_unroll = 3;
};
extern Options g_opt;

// Device-side failure reporting (round 6): the host-mapped error word
// (graph.hip).  A kernel that cannot finish its work correctly stores a code
// there; take_device_error() turns a stored code into MGCN_EDEVICE + the
// message (and clears it).  The launchers of such kernels call it first, so a
// failed launch fails the next call at the latest; mgcn_check_device() reads
// it after a stream sync.
constexpr unsigned kDevErrDws = 1;   // spmm_xw_bwd_ws_kernel: hand-off spin bound exceeded
constexpr unsigned kDevErrWide = 2;  // spmm_xw_wide_ws_kernel: hand-off spin bound exceeded
constexpr unsigned kDevErrPack = 3;  // pack_rows_kernel: look-back spin bound exceeded
constexpr unsigned kDevErrFwdWs = 4; // spmm_xw_fwd_ws_kernel: hand-off spin bound exceeded
unsigned *device_error_word();       // device pointer (nullptr + set_error on failure)
int take_device_error();

// lane 0 of the calling wave stores `code` into the error word (a vector
// store to host-coherent memory at system scope)
__device__ inline void report_device_error(unsigned *err, unsigned code) {
  if (err != nullptr && (threadIdx.x & 63) == 0)
    __hip_atomic_store(err, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// One gathered edge folded into a lane's four features: acc += x * w, product
// and sum rounded separately (the SpMM's arithmetic, bit for bit)
__device__ __forceinline__ void fold4(float (&acc)[4], const float4 &x, float w) {
  acc[0] = __fadd_rn(acc[0], __fmul_rn(x.x, w));
  acc[1] = __fadd_rn(acc[1], __fmul_rn(x.y, w));
  acc[2] = __fadd_rn(acc[2], __fmul_rn(x.z, w));
  acc[3] = __fadd_rn(acc[3], __fmul_rn(x.w, w));
}

// Check the last launch on this thread; record the HIP error string on failure.
inline int check_launch(const char *what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return MGCN_EHIP;
  }
  return MGCN_OK;
}

#define MGCN_HIP_TRY(call)                                                    \
  do {                                                                        \
    hipError_t _e = (call);                                                   \
    if (_e != hipSuccess) {                                                   \
      ::mgcn::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), \
                        __FILE__, __LINE__);                                  \
      return MGCN_EHIP;                                                       \
    }                                                                         \
  } while (0)

#define MGCN_REQUIRE(cond, ...)       \
  do {                                \
    if (!(cond)) {                    \
      ::mgcn::set_error(__VA_ARGS__); \
      return MGCN_EINVAL;             \
    }                                 \
  } while (0)

// Let `kernel` take up to max_bytes of dynamic LDS on the current device.  The
// attribute is per device: attr_set (a static of the calling launcher, so one
// per kernel instantiation) holds one bit per device id; racing threads at
// worst both set it.
inline int allow_lds(const void *kernel, std::atomic<uint64_t> &attr_set, int max_bytes) {
  int dev = 0;
  MGCN_HIP_TRY(hipGetDevice(&dev));
  const uint64_t bit = uint64_t(1) << (dev & 63);
  if (!(attr_set.load(std::memory_order_acquire) & bit)) {
    MGCN_HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     max_bytes));
    attr_set.fetch_or(bit, std::memory_order_release);
  }
  return MGCN_OK;
}

// MGCN_EWORKSPACE ("<who>: workspace <given> < <need>") unless `workspace` holds `need` bytes
inline int require_workspace(const char *who, const void *workspace, size_t bytes, size_t need) {
  if (workspace != nullptr && bytes >= need) return MGCN_OK;
  set_error("%s: workspace %zu < %zu", who, bytes, need);
  return MGCN_EWORKSPACE;
}

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Grid sizing for grid-stride loops over memory-bound work: enough blocks to
// fill 256 CUs several times over, capped (cdna_hip_programming.md G11).
inline unsigned grid_for(int64_t work_items, int block) {
  int64_t g = (work_items + block - 1) / block;
  if (g < 1) g = 1;
  if (g > 8192) g = 8192;
  return static_cast<unsigned>(g);
}

// CUs of the current device (256 where the query fails), for grids sized per
// CU.  Asked on every call: the current device changes between calls.
inline int device_cus() {
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    cus = 256;
  return cus;
}

int gemm_precision_is_x6();  // 1 under bf16x6 (the fused kernels need it)
// deterministic folds of per-workgroup partials (gemm.hip)
// deterministic fold of split partials: C[e] (+)= sum_sp partial[sp * MN + e]
int launch_fold(const float *partial, int64_t splits, int64_t MN, int N, float *C, int64_t ldc,
                int accumulate, hipStream_t s);
int launch_fold_split(const float *partial, int64_t splits, int64_t MN, int N, float *C,
                      int64_t ldc, int N1, float *C2, int64_t ldc2, int accumulate, hipStream_t s);
int launch_split_reduce(const float *partial, int splits, int64_t MN, int N, float *C,
                        int64_t ldc, int accumulate, hipStream_t s);
int launch_colsum_fold(const float *partial, int64_t nparts, int N, float *out, hipStream_t s);
// A fold of split partials (launch_fold_split's job: C[e] = sum_sp
// partial[sp * MN + e], columns [N1, N) of the [MN / N, N] result to C2
// transposed) run by `blocks` extra 256-thread workgroups of a launch that
// has other work; a workgroup b < blocks calls side_fold_block(f, b, red).
struct SideFold {
  const float *partial;
  int64_t parts, MN;
  int N, N1, log_eb, blocks;
  float *C, *C2;
  int64_t ldc, ldc2;
};
SideFold make_side_fold(const float *partial, int64_t parts, int64_t MN, int N, float *C,
                        int64_t ldc, int N1, float *C2, int64_t ldc2);
int launch_side_fold(const SideFold &f, hipStream_t s);  // on its own (nothing to ride in)

// the same fixed order as fold_partials_kernel (strided partial sums of EB
// elements per workgroup, then a tree over the 256 / EB groups); red: 256
// floats of LDS; every thread of the workgroup calls it
__device__ inline void side_fold_block(const SideFold &f, int b, float *red) {
  const int EB = 1 << f.log_eb, T = 256 >> f.log_eb;
  const int el = threadIdx.x & (EB - 1), g = threadIdx.x >> f.log_eb;
  const int64_t e = (int64_t)b * EB + el;
  float acc = 0.0f;
  if (e < f.MN) {
#pragma unroll 4
    for (int64_t sp = g; sp < f.parts; sp += T) acc = __fadd_rn(acc, f.partial[sp * f.MN + e]);
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int h = T >> 1; h >= 1; h >>= 1) {
    if (g < h) red[threadIdx.x] = __fadd_rn(red[threadIdx.x], red[threadIdx.x + h * EB]);
    __syncthreads();
  }
  if (g == 0 && e < f.MN) {
    const int64_t row = e / f.N, col = e % f.N;
    float *dst = col < f.N1 ? f.C + row * f.ldc + col : f.C2 + (col - f.N1) * f.ldc2 + row;
    *dst = red[el];
  }
}

// The staged small-C GEMM C = A^T B as a job for other launches (tn_staged.h:
// tn_staged_block over `blocks` workgroups into the split partials at
// `partial`, folded afterwards with make_side_fold(partial, blocks, M N, ...)).
struct TnJob {
  const float *A;
  int64_t lda;
  const float *B;
  int64_t ldb;
  int64_t K, kps;
  float *partial;
  int blocks;
};
bool tn_staged_plan(int64_t K, int32_t M, int32_t N, const float *A, int64_t lda, const float *B,
                    int64_t ldb, void *workspace, size_t workspace_bytes, TnJob *job);

// mgcn_gemm_tn_split (accumulate = 0) with `side` folded by extra workgroups
// of the same launch; where the staged kernel takes the shape and `defer` is
// given, its own split-K fold is left to the caller (*defer, to ride in a
// later launch: launch_side_fold if none does), else folded here
int gemm_tn_split_fold(int64_t K, int32_t M, int32_t N, int32_t N1, const float *A, int64_t lda,
                       const float *B, int64_t ldb, float *C1, int64_t ldc1, float *C2t,
                       int64_t ldc2t, void *workspace, size_t workspace_bytes,
                       const SideFold &side, hipStream_t s, SideFold *defer = nullptr);
// The residual layer's forward transform (residual.hip, F = 32) applied by
// the heavy-row kernels to their rows' aggregates: Z = relu2(relu1(agg W + b)
// + x Wr^T + br) and the rows' two mask words.  W == NULL: plain aggregate.
struct ResEpi {
  const float *W, *Wr, *b, *br;
  int64_t ldw, ldwr;
  const float *X;  // the rows' own inputs
  int64_t ldx;
  uint32_t *masks;
  int relu1, relu2;
};
// heavy rows of a view alone (spmm.hip), for the fused layer kernels of residual.hip
int heavy_rows(int bwd, int64_t n_rows, int32_t F, const int64_t *rowptr, const int32_t *col,
               const int32_t *eid, const float *w, const float *X, int64_t ldx, float *Y,
               int64_t ldy, const float *row_scale, int mean, const int32_t *order,
               int64_t n_heavy, int64_t n_giant, hipStream_t stream, bool *side_used,
               const ResEpi *rs = nullptr);
int heavy_rows_join(hipStream_t stream);
// fused layer kernels at F = 256 (fused_wide.hip)
size_t xw_wide_workspace_bytes(bool bwd);
int xw_wide_fwd(int64_t n_rows, const int64_t *rowptr, const int32_t *col, const float *w,
                const float *X, int64_t ldx, const float *W, int64_t ldw, const float *bias,
                float *Y, int64_t ldy, int mean, int relu, uint32_t *relu_mask, float *Z,
                int64_t ldz, void *workspace, hipStream_t s,
                const mgcn_packed_table *pk = nullptr);
int xw_wide_bwd_dx(int64_t n_rows, const int64_t *rowptr_t, const int32_t *col_t,
                   const float *w_t, const float *row_scale, const float *dY, int64_t lddy,
                   const float *W, int64_t ldw, float *dX, int64_t lddx,
                   const uint32_t *relu_mask, const float *row_div, float *colsum,
                   int accumulate, void *workspace, hipStream_t s,
                   const mgcn_packed_table *pk = nullptr);

}  // namespace mgcn
