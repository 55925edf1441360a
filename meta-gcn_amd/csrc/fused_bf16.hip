// Fused bf16 GCN layer on gfx950: the aggregation of bf16 feature rows and the
// layer's 128 x 128 product in one launch, for both directions of a layer
// (mgcn_spmm_xw_bf16).
//
//   Zf = reduce_k float(X[col_k]) * w_k [/ cnt[col_k]]  [/ count] [* row_scale]   (fp32)
//   Zb = bf16(Zf)                                         (round to nearest even, once)
//   Y  = bf16(epi(fp32acc(float(Zb) @ float(B)) + bias)),  epi = optional ReLU
//
// Forward of a layer: the fwd view, w = w_fwd, B = W, bias and ReLU in the
// epilogue, Z (optional output) = Zb -- for mean the divided row.  Adjoint
// (dX only): the bwd view, w = w_bwd, row_scale, cnt for mean (every gathered
// row divided inside the gather), B = W with the transpose flag.
//
// Arithmetic contract:
//   1. Zf is formed exactly as spmm_bf16.hip forms it (edge order within a
//      row, products and sums rounded separately, no contraction), so Zb is
//      bit for bit mgcn_spmm_fwd_bf16's output in the forward and
//      mgcn_spmm_bwd_bf16's in the adjoint.
//   2. The product is ONE bf16 MFMA term (v_mfma_f32_16x16x32_bf16) with an
//      fp32 accumulator, not the bf16x6 split: both operands are bf16 numbers
//      already, so every product is exact in fp32.
//   3. One rounding at the store of Y; no atomics, a fixed chunk -> workgroup
//      map: deterministic from run to run.
//
// Work split (fused_fwd.hip's plain chunk kernel): persistent 512-thread
// workgroups, two per CU; chunk c (rows 32 c .. 32 c + 31) goes to workgroup
// c % grid.
//   Phase A (gather, spmm_bf16_kernel at G = 16): row 4 wave + grp of the
//     chunk is owned by the 16-lane group grp of wave `wave` -- 16 lanes x
//     16 B read a whole 256-B row, U = 8 gathers in flight per group, 64-bit
//     row addresses.  The rounded row goes into the chunk's Zb image in LDS
//     (x6.h's swizzled row-major layout, a single term) and, when asked for,
//     to Z as a whole row.
//   Phase B (MFMA): wave w owns output columns 16 w .. 16 w + 15.  The
//     operands are swapped (B's fragment in the A slot, the Zb rows in the B
//     slot), so that a lane's four accumulators are four CONSECUTIVE columns
//     of one row: they are rounded and staged as one 8-byte LDS write.
//   The staged bf16 tile is written out as whole 256-B rows (16 B per lane,
//   one row-chunk per thread) after the next chunk's barrier, beside its
//   gathers.
// B is staged once per workgroup into LDS as Bt[n][k] -- a straight 16-B copy
// under the transpose flag, an element transposition otherwise -- and each
// wave then keeps its four fragments (16 VGPRs) for the whole kernel.
//
// LDS: Bt 32 KB + 2 x 8 KB Zb images + 2 x 8 KB staging tiles = 64 KB (the
// images and tiles double-buffered, so one barrier per chunk orders
// everything): two workgroups per CU.
//
// Roofline: HBM-bound.  Bytes per launch
//     8 (n_rows + 1) + nnz (4 col + 4 w + 2 F) + 2 n_rows F  (+ 2 n_rows F with Z)
// against the unfused pair's extra 4 N F (the GEMM reads x and writes h).

#include "mgcn_internal.h"
#include "x6.h"

namespace mgcn {
namespace {

using namespace x6;

constexpr int kF = 128;
constexpr int kRows = 32;            // rows per chunk
constexpr int kWaves = 8;
constexpr int kThreads = 64 * kWaves;
constexpr int kPerCU = 2;            // resident workgroups per CU the grid is sized for
constexpr int kG = 16;               // lanes per gathered row (8 bf16 = 16 B each)
constexpr int kU = 8;                // gathers in flight per row
constexpr int kTile = kRows * 256;   // a [32][128] bf16 image: 8 KB
constexpr int kBtOff = 0;            // Bt[n][k], 128 rows of 256 B
constexpr int kImgOff = kF * 256;
constexpr int kStageOff = kImgOff + 2 * kTile;
constexpr int kLds = kStageOff + 2 * kTile;
static_assert(kPerCU * kLds <= 160 * 1024, "two workgroups per CU");

struct Args {
  int64_t n_rows;
  const int64_t *rowptr;
  const int32_t *col;
  const float *w;          // per-slot weights, nullable
  const float *row_scale;  // per-row factor, nullable
  const float *cnt;        // per gathered row divisor (CNT kernels)
  const uint16_t *X;       // gathered rows [n_cols][128] bf16
  int64_t ldx;
  const uint16_t *B;       // [128][128] bf16, row-major
  int64_t ldb;
  int transpose_b;         // Y = Zb B^T
  const float *bias;       // nullable, fp32
  uint16_t *Y;
  int64_t ldy;
  uint16_t *Z;             // nullable: Zb
  int64_t ldz;
  int mean;                // divide the row by max(count, 1)
  int relu;
};

// 8 bf16 -> 8 floats (exact): element 2 i in the low half of word i
__device__ __forceinline__ void widen8(const u32x4 p, float (&r)[8]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x2 t = widen_bf16x2(p[i]);
    r[2 * i] = t.x;
    r[2 * i + 1] = t.y;
  }
}
__device__ __forceinline__ uint32_t round2(float lo, float hi) {  // v_cvt_pk_bf16_f32, RNE
  const f32x2 t = {lo, hi};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(t, bf16x2));
}

// One row per 16-lane group, four rows per wave, exactly spmm_bf16_kernel's
// loop at G = 16, U = 8 (FWD_SUM / BWD_SUM; CNT: BWD_MEAN's per-edge
// division): metadata lane-parallel 16 edges at a time, broadcast inside the
// group; U gathers issued before any is folded; the fold in ascending edge
// order, products and sums rounded separately.
template <bool CNT>
__device__ __forceinline__ void gather_row16(const Args &a, int64_t beg, int64_t deg, int gl,
                                             int gbase, float (&acc)[8]) {
  const uint16_t *__restrict__ X = a.X;
  const bool has_w = a.w != nullptr;
  int64_t maxdeg = deg;  // over the wave's four rows: wave-uniform loop bounds
#pragma unroll
  for (int off = kG; off < 64; off <<= 1) {
    const int64_t o = __shfl_xor(maxdeg, off, 64);
    maxdeg = o > maxdeg ? o : maxdeg;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.0f;
  const int f0 = 8 * gl;
  for (int64_t e0 = 0; e0 < maxdeg; e0 += kG) {
    const int64_t my = e0 + gl;
    int mc = 0;
    float mw = 1.0f, mcnt = 1.0f;
    if (my < deg) {
      mc = a.col[beg + my];
      if (has_w) mw = a.w[beg + my];
      if constexpr (CNT) mcnt = a.cnt[mc];
    }
    const int64_t rem = deg - e0;
    const int nb = rem <= 0 ? 0 : (rem < kG ? (int)rem : kG);  // this group
    const int64_t remw = maxdeg - e0;
    const int nbmax = remw < kG ? (int)remw : kG;              // wave-uniform
    for (int k0 = 0; k0 < nbmax; k0 += kU) {
      u32x4 xb[kU];
      float wk[kU], cntk[kU];
      bool ok[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int k = k0 + u;
        const int kk = k & (kG - 1);
        const int ck = __shfl(mc, gbase + kk, 64);
        wk[u] = __int_as_float(__shfl(__float_as_int(mw), gbase + kk, 64));
        cntk[u] = 1.0f;
        if constexpr (CNT) cntk[u] = __int_as_float(__shfl(__float_as_int(mcnt), gbase + kk, 64));
        ok[u] = k < nb;
        if (ok[u]) xb[u] = *reinterpret_cast<const u32x4 *>(X + (int64_t)ck * a.ldx + f0);
      }
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        if (ok[u]) {
          float xv[8];
          widen8(xb[u], xv);
          if constexpr (CNT) {
#pragma unroll
            for (int j = 0; j < 8; ++j) xv[j] = __fdiv_rn(xv[j], cntk[u]);
          }
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[j] = __fadd_rn(acc[j], __fmul_rn(xv[j], wk[u]));
        }
      }
    }
  }
}

template <bool CNT>
__global__ __launch_bounds__(kThreads, 2 * kPerCU) void spmm_xw_bf16_kernel(const Args a) {
  __shared__ __attribute__((aligned(16))) char lds[kLds];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int gl = lane & (kG - 1), grp = lane / kG, gbase = grp * kG;
  const int l16 = lane & 15, g4 = lane >> 4;
  const int64_t n_chunks = (a.n_rows + kRows - 1) / kRows;

  // ---- B -> Bt[n][k] in LDS (x6.h's image layout over 128 rows), once -----
  if (a.transpose_b) {
    // Bt[n][k] = B[n][k]: 128 rows x 16 chunks of 16 B, four per thread
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int q = tid + kThreads * i;
      const int n = q >> 4, ch = q & 15;
      const u32x4 v = *reinterpret_cast<const u32x4 *>(a.B + (int64_t)n * a.ldb + 8 * ch);
      *reinterpret_cast<u32x4 *>(lds + kBtOff + img_off(n, ch)) = v;
    }
  } else {
    // Bt[n][k] = B[k][n]: a thread reads 8 consecutive n of one k, writes 8 elements
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int q = tid + kThreads * i;
      const int k = q >> 4, nc = q & 15;
      const u32x4 v = *reinterpret_cast<const u32x4 *>(a.B + (int64_t)k * a.ldb + 8 * nc);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int n = 8 * nc + j;
        const uint16_t e = (uint16_t)(v[j >> 1] >> (16 * (j & 1)));
        *reinterpret_cast<uint16_t *>(lds + kBtOff + img_off(n, k >> 3) + 2 * (k & 7)) = e;
      }
    }
  }
  __syncthreads();
  // this wave's fragments: lane (g4, l16) holds k = 32 ks + 8 g4 + j of column n = 16 wave + l16
  bf16x8 wb[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks)
    wb[ks] = *reinterpret_cast<const bf16x8 *>(lds + kBtOff + img_off(16 * wave + l16, 4 * ks + g4));
  // the lane's output columns in phase B: 16 wave + 4 g4 + r
  float bcol[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (a.bias != nullptr) {
#pragma unroll
    for (int r = 0; r < 4; ++r) bcol[r] = a.bias[16 * wave + 4 * g4 + r];
  }

  // staged rows of chunk c -> Y: thread tid writes 16-B chunk tid & 15 of row tid >> 4
  auto flush = [&](int64_t c, const char *stage) {
    const int lr = tid >> 4, ch = tid & 15;
    const int64_t row = c * kRows + lr;
    const u32x4 v = *reinterpret_cast<const u32x4 *>(stage + img_off(lr, ch));
    if (row < a.n_rows) *reinterpret_cast<u32x4 *>(a.Y + row * a.ldy + 8 * ch) = v;
  };

  const int lr = 4 * wave + grp;  // this group's row of every chunk
  const int64_t step = (int64_t)gridDim.x * kRows;
  int64_t row_n = (int64_t)blockIdx.x * kRows + lr;
  bool ok_n = row_n < a.n_rows;
  int64_t beg_n = ok_n ? a.rowptr[row_n] : 0, end_n = ok_n ? a.rowptr[row_n + 1] : 0;
  int it = 0;
  for (int64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x, ++it) {
    char *img = lds + kImgOff + (it & 1) * kTile;
    char *stage = lds + kStageOff + (it & 1) * kTile;

    // ---- Phase A: aggregate the chunk's rows into the Zb image -------------
    const int64_t row = row_n;
    const bool row_ok = ok_n;
    const int64_t beg = beg_n, deg = end_n - beg_n;
    row_n += step;  // the next chunk's row pointers, under this chunk's gathers
    ok_n = row_n < a.n_rows;
    beg_n = ok_n ? a.rowptr[row_n] : 0;
    end_n = ok_n ? a.rowptr[row_n + 1] : 0;
    float acc[8];
    gather_row16<CNT>(a, beg, deg, gl, gbase, acc);
    if (a.mean) {
      const float c = (float)(deg > 1 ? deg : 1);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = __fdiv_rn(acc[j], c);
    }
    if (a.row_scale != nullptr && row_ok) {
      const float s = a.row_scale[row];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = __fmul_rn(acc[j], s);
    }
    u32x4 zb;  // the one rounding of Z (rows past the end: zeros)
#pragma unroll
    for (int i = 0; i < 4; ++i) zb[i] = round2(acc[2 * i], acc[2 * i + 1]);
    *reinterpret_cast<u32x4 *>(img + img_off(lr, gl)) = zb;
    if (a.Z != nullptr && row_ok) *reinterpret_cast<u32x4 *>(a.Z + row * a.ldz + 8 * gl) = zb;

    __syncthreads();
    // the previous chunk's output rows (staged before this barrier) go out
    if (it > 0) flush(chunk - gridDim.x, lds + kStageOff + ((it + 1) & 1) * kTile);

    // ---- Phase B: Y^T tile = Bt-fragment x Zb rows -> staging tile ---------
    // operands swapped: acc2[t][r] = Y[16 t + l16][16 wave + 4 g4 + r]
    f32x4_t acc2[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc2[t][r] = 0.0f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const bf16x8 z =
            *reinterpret_cast<const bf16x8 *>(img + img_off(16 * t + l16, 4 * ks + g4));
        acc2[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb[ks], z, acc2[t], 0, 0, 0);
      }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        v[r] = acc2[t][r];
        if (a.bias != nullptr) v[r] = __fadd_rn(v[r], bcol[r]);
        if (a.relu) v[r] = (v[r] < 0.0f) ? 0.0f : v[r];
      }
      // the one rounding of Y; 8 B at columns 16 wave + 4 g4 of row 16 t + l16
      const u32x2 p = {round2(v[0], v[1]), round2(v[2], v[3])};
      *reinterpret_cast<u32x2 *>(stage + img_off(16 * t + l16, 2 * wave + (g4 >> 1)) +
                                 8 * (g4 & 1)) = p;
    }
  }
  if (it > 0) {
    __syncthreads();
    flush((int64_t)blockIdx.x + (int64_t)(it - 1) * gridDim.x,
          lds + kStageOff + ((it + 1) & 1) * kTile);
  }
}

int grid_size(int64_t n_chunks) {
  const int64_t g = (int64_t)kPerCU * device_cus();
  return (int)(g < n_chunks ? g : n_chunks);
}

inline bool rows16(const void *p, int64_t ld) {
  return ld >= kF && ld % 8 == 0 && reinterpret_cast<uintptr_t>(p) % 16 == 0;
}

}  // namespace
}  // namespace mgcn

using namespace mgcn;

extern "C" int mgcn_spmm_xw_bf16_supported(int32_t F_in, int32_t F_out, int reduce) {
  return (F_in == kF && F_out == kF && (reduce == MGCN_REDUCE_SUM || reduce == MGCN_REDUCE_MEAN))
             ? 1 : 0;
}

extern "C" int mgcn_spmm_xw_bf16(int64_t n_rows, int32_t F_in, int32_t F_out,
                                 const int64_t *rowptr, const int32_t *col, const float *w,
                                 const float *row_scale, const float *cnt, const uint16_t *X,
                                 int64_t ldx, const uint16_t *B, int64_t ldb, int transpose_b,
                                 const float *bias, int relu, uint16_t *Y, int64_t ldy,
                                 uint16_t *Z, int64_t ldz, int reduce, void *stream) {
  clear_error();
  MGCN_REQUIRE(n_rows >= 0, "mgcn_spmm_xw_bf16: negative size");
  MGCN_REQUIRE(mgcn_spmm_xw_bf16_supported(F_in, F_out, reduce),
               "mgcn_spmm_xw_bf16: unsupported F_in=%d F_out=%d reduce=%d (needs 128 x 128, "
               "sum/mean)",
               F_in, F_out, reduce);
  MGCN_REQUIRE(cnt == nullptr || reduce == MGCN_REDUCE_SUM,
               "mgcn_spmm_xw_bf16: cnt (the adjoint's per-edge division) goes with reduce = sum");
  if (n_rows == 0) return MGCN_OK;
  MGCN_REQUIRE(rowptr && X && B && Y, "mgcn_spmm_xw_bf16: null array");  // col may be NULL when nnz == 0
  MGCN_REQUIRE(ldx >= kF && ldy >= kF && ldb >= kF && (Z == nullptr || ldz >= kF),
               "mgcn_spmm_xw_bf16: leading dimension < 128");
  MGCN_REQUIRE(rows16(X, ldx) && rows16(Y, ldy) && rows16(B, ldb) && (Z == nullptr || rows16(Z, ldz)),
               "mgcn_spmm_xw_bf16: rows must be 16-byte aligned (pointer %% 16 == 0, ld %% 8 == 0)");
  MGCN_REQUIRE(bias == nullptr || reinterpret_cast<uintptr_t>(bias) % 4 == 0,
               "mgcn_spmm_xw_bf16: bias not 4-byte aligned");
  Args a{};
  a.n_rows = n_rows;
  a.rowptr = rowptr;
  a.col = col;
  a.w = w;
  a.row_scale = row_scale;
  a.cnt = cnt;
  a.X = X;
  a.ldx = ldx;
  a.B = B;
  a.ldb = ldb;
  a.transpose_b = transpose_b != 0;
  a.bias = bias;
  a.Y = Y;
  a.ldy = ldy;
  a.Z = Z;
  a.ldz = ldz;
  a.mean = reduce == MGCN_REDUCE_MEAN;
  a.relu = relu != 0;
  const int64_t n_chunks = (n_rows + kRows - 1) / kRows;
  const dim3 grid((unsigned)grid_size(n_chunks));
  hipStream_t s = as_stream(stream);
  if (cnt != nullptr)
    hipLaunchKernelGGL(spmm_xw_bf16_kernel<true>, grid, dim3(kThreads), 0, s, a);
  else
    hipLaunchKernelGGL(spmm_xw_bf16_kernel<false>, grid, dim3(kThreads), 0, s, a);
  return check_launch("spmm_xw_bf16_kernel");
}
