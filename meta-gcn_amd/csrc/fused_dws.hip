// The warp-specialised fused adjoint at F = 128 (DWS), spmm_xw_bwd_ws_kernel,
// with its launch ladder (xw128.h: the design, the shared gather primitives
// and chunk helpers; ws_handoff.h: the LDS counter hand-off).

#include "ws_handoff.h"
#include "xw128.h"

namespace mgcn {
namespace {

#if MGCN_EXPERIMENT
__device__ unsigned long long g_tail[kTailMaxWg][4];  // XTAIL_* (xw128.h), kernel 1
#endif

// ===================== warp-specialised adjoint (round 5) =====================
//
// DWS: the layer's whole adjoint re-cut by role as fused_wide.hip's F = 256
// kernels (dW = X^T dH and dX = relu'(lower) (dH W^T) [/ row_div], dH =
// A^T dY [* rs] never leaving the chip):
//
// One 1024-thread workgroup per CU: 8 GATHER waves aggregate dH rows (two
// 32-lane groups per wave, gather_row_meta's edge order: bit for bit the
// SpMM's adjoint), write them as bf16 term images into a ring of two chunk
// buffers and load the chunk's own X rows (fp32) beside them under the
// gathers; 8 MFMA waves form the chunk's dX (W^T as the A operand from an LDS
// copy of W: a lane's fragment is 4 consecutive columns of one row, one 16-B
// store; the same six products in the same order as the two-phase kernel, so
// dX is bit for bit its result), apply the epilogue, and fold their two 32x32
// tiles of X^T dH straight from the ring -- one 128 x 128 partial per
// workgroup over a one-workgroup-per-CU split-K grid, folded in workgroup
// order.  Hand-offs: LDS counters as in fused_wide.hip (bounded spins, abort
// word, reported through the device error word).  (The dX-only form of this
// kernel and DWL -- the lower layer's dW fused into the dX-only adjoint --
// measured slower than the two-phase kernel / the separate dW pass, round 5,
// and are removed.)
constexpr int kBsDws = 2, kBsDwsH = 3, kBsDwsM = 4;  // spmm_xw_bwd_ws_kernel MODE
#ifndef MGCN_DS_MASK_RING
#define MGCN_DS_MASK_RING 1  // DWS: ReLU mask words / divisors through the ring (0: MFMA waves load them)
#endif
// Layout: a ring of two (dH term images + X fp32 rows) chunk buffers and
// W in fp32 (rows padded to 528 B: the 16 rows of a W^T fragment read and the
// two row halves of an X^T fragment read fall on distinct banks); the MFMA
// waves split W^T and X^T fragments as they read them
constexpr int kDsXLd = kXwF + 4;                    // floats per padded row
constexpr int kDsXOff = kBsImgSet;                  // X rows within a ring buffer
constexpr int kDsMaskOff = kDsXOff + kXwRows * kDsXLd * 4;  // [32][4] mask words
constexpr int kDsDivOff = kDsMaskOff + kXwRows * 16;         // [32] row divisors
constexpr int kDsRingBuf = kDsDivOff + kXwRows * 4;
constexpr int kDsWOff = 2 * kDsRingBuf;
constexpr int kDsCtrOff = kDsWOff + kXwF * kDsXLd * 4;
constexpr int kDsLds = kDsCtrOff + 64;
static_assert(kDsLds <= 160 * 1024, "one DWS workgroup per CU");
static_assert(16 * kXwF * 4 <= kDsWOff, "column-sum fold fits in the ring");

// the two-phase kernel's six products (dH_l W_h, dH_h W_l, dH_m W_m, dH_m W_h,
// dH_h W_m, dH_h W_h) with W^T as the A operand
__device__ __forceinline__ f32x4_t mfma16_x6_at(const bf16x8 (&w)[3], const bf16x8 &xh,
                                               const bf16x8 &xm, const bf16x8 &xl, f32x4_t c) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[0], xl, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[2], xh, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[1], xm, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[0], xm, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[1], xh, c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[0], xh, c, 0, 0, 0);
}

struct XbsArgs {
  XbArgs b;             // rowptr .. colsum_partial; X, dw_partial: [grid][128][128]
  float *hcs_partial;   // DWS (nullable): [grid][128] column sums of dY's own rows
  int dbg;              // xw_ws_dbg (experiment builds only; masked by kDbgMask)
  uint32_t spin;        // hand-off spin bound ("ws_spin_limit")
  unsigned *err;        // device error word: kDevErrDws when a hand-off gave up
};

template <int U, int EPI, int MODE, int ROLL>
__global__ __launch_bounds__(kBsThreads) void spmm_xw_bwd_ws_kernel(const XbsArgs A) {
  constexpr bool HCS = MODE == kBsDwsH;  // DWS + dY's column sums (hcs_partial)
  constexpr bool MAXM = MODE == kBsDwsM;  // DWS on the max adjoint (win_mask + slot_map)
  static_assert(ROLL == 0 || (ROLL == 2 && !MAXM), "the max adjoint keeps the batch gather");
  constexpr bool MRING = MGCN_DS_MASK_RING;
  constexpr int kRing = kDsRingBuf;
  // The max adjoint keeps the timing switches' runtime branches in the
  // product too (A.dbg is 0 there: the product rejects xw_ws_dbg, bs_prepare
  // passes dbg = 0): compiled out, their block boundaries went with them
  // and this kernel ran 1.55 vs 1.34 ms at config 4 (round 6, A/B on one box;
  // sched_barrier fences at the same places did not restore it).  The sum
  // adjoint measured the same either way and compiles them out.
  constexpr int kDbgMask = MAXM ? ~0 : mgcn::kDbgMask;
  const XbArgs &a = A.b;
  __shared__ __attribute__((aligned(16))) char lds[kDsLds];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int gl = lane & 31, grp = lane >> 5;
  const int l16 = lane & 15, g4 = lane >> 4;
  int *ctr = reinterpret_cast<int *>(lds + kDsCtrOff);
  int *filled = ctr, *mdone = ctr + 2, *freed = ctr + 4, *abort_word = ctr + 8;
  if (tid < 16) ctr[tid] = 0;
  // W (64 KB) into LDS once: four float4 per thread
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int e = tid + kBsThreads * j;  // float4 e: row e >> 5, columns 4 (e & 31) ..
    const float4 v = *reinterpret_cast<const float4 *>(a.W + (int64_t)(e >> 5) * a.ldw + 4 * (e & 31));
    *reinterpret_cast<float4 *>(lds + kDsWOff + 4 * ((e >> 5) * kDsXLd + 4 * (e & 31))) = v;
  }
  __syncthreads();

  const int64_t n_chunks = (a.n_rows + kXwRows - 1) / kXwRows;
  const int64_t n_my = my_chunks(n_chunks);
  auto chunk_of = [&](int64_t i) { return (int64_t)blockIdx.x + i * gridDim.x; };
  XTAIL_ENTRY(1);
  auto rows_in = [&](int64_t c) -> uint32_t {
    const int64_t r = a.n_rows - c * kXwRows;
    return (uint32_t)(r <= 0 ? 0 : r >= kXwRows ? kXwRows : r);
  };

  float cs[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // MFMA waves: column sums of their 4 columns
  float hc[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // gather waves (hcs_partial): dY column sums
  f32x16 accw[2];                          // MFMA waves: two 32 x 32 dW tiles
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int r = 0; r < 16; ++r) accw[s][r] = 0.0f;

  if (wave < kBsNG) {
    // ------------------------------- gather waves ---------------------------
    // the wave's k-th quad is q = wave + 8 k: chunk q >> 3, rows
    // 4 (q & 7) + grp and 4 (q & 7) + 2 + grp for lane group grp
    const int64_t n_quads = 8 * n_my;
    auto row_of = [&](int64_t k, int second) -> int64_t {
      const int64_t q = wave + kBsNG * k;
      return chunk_of(q >> 3) * kXwRows + 4 * (q & 7) + 2 * second + grp;
    };
    const auto rdy = buf_rsrc(a.dY, (uint32_t)(a.n_cols * a.lddy * 4));
    const uint32_t ldy_b = (uint32_t)a.lddy * 4u;
    RowMeta cur[2] = {}, nxt[2] = {};
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      meta_rowptr(a.rowptr, row_of(0, j), row_of(0, j) < a.n_rows && wave < n_quads, cur[j]);
      if constexpr (MAXM)
        meta_first_m(a.col, a.w, a.slot_map, gl, cur[j]);
      else
        meta_first(a.col, a.w, gl, cur[j]);
      meta_rowptr(a.rowptr, row_of(1, j), row_of(1, j) < a.n_rows && wave + kBsNG < n_quads,
                  nxt[j]);
    }
    // ROLL 2: the quad's first U slots per row are in flight on entry (here:
    // the first quad's; then issued under the previous quad's last round)
    RollWin<U> win;
    if constexpr (ROLL == 2) roll_first<U>(rdy, ldy_b, cur[0], cur[1], gl, grp, win);
    int64_t k = 0;
    for (int64_t q = wave; q < n_quads; q += kBsNG, ++k) {
      RowMeta nn[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if constexpr (MAXM)
          meta_first_m(a.col, a.w, a.slot_map, gl, nxt[j]);
        else
          meta_first(a.col, a.w, gl, nxt[j]);
        const int64_t r2 = row_of(k + 2, j);
        if constexpr (ROLL == 2)
          meta_rowptr_raw(a.rowptr, r2, r2 < a.n_rows && q + 2 * kBsNG < n_quads, nn[j]);
        else
          meta_rowptr(a.rowptr, r2, r2 < a.n_rows && q + 2 * kBsNG < n_quads, nn[j]);
      }
      const int64_t i = q >> 3;
      const int64_t c = chunk_of(i);
      const int64_t r0 = c * kXwRows;
      const int lr0 = 4 * (int)(q & 7) + grp;
      u32x4 zv[2] = {};
      if (!(A.dbg & kDbgMask & 4)) {  // the rows' X, under the gathers (streamed once)
        const auto rz = buf_rsrc(a.X + r0 * a.ldx, rows_in(c) * (uint32_t)a.ldx * 4u);
#pragma unroll
        for (int j = 0; j < 2; ++j)
          zv[j] = __builtin_amdgcn_raw_buffer_load_b128(
              rz, 4 * (int)((lr0 + 2 * j) * a.ldx + 4 * gl), 0, MGCN_NT_AUX);
      }
      // DWS + hcs_partial (n_cols == n_rows): the rows' own dY rows, whose
      // column sums are the layer's bias gradient -- every dY row once, rows
      // q then q + 2 of every quad: a fixed order
      // DWS: the rows' ReLU mask words (lanes 0-3) and divisor (lane 4) ride
      // through the ring to the MFMA waves' epilogue (no registers held there)
      uint32_t mv[2] = {0u, 0u};
      if constexpr (MRING && EPI != EPI_STORE) {
        const auto rm = buf_rsrc(a.relu_mask + r0 * 4, rows_in(c) * 16u);
#pragma unroll
        for (int j = 0; j < 2; ++j)
          if (gl < 4) mv[j] = __builtin_amdgcn_raw_buffer_load_b32(rm, 4 * ((lr0 + 2 * j) * 4 + gl), 0, 0);
        if constexpr (EPI == EPI_RELU_DIV) {
          const auto rd = buf_rsrc(a.row_div + r0, rows_in(c) * 4u);
#pragma unroll
          for (int j = 0; j < 2; ++j)
            if (gl == 4) mv[j] = __builtin_amdgcn_raw_buffer_load_b32(rd, 4 * (lr0 + 2 * j), 0, 0);
        }
      }
      u32x4 yv[2] = {};
      if constexpr (HCS) {
        const auto ry = buf_rsrc(a.dY + r0 * a.lddy, rows_in(c) * (uint32_t)a.lddy * 4u);
#pragma unroll
        for (int j = 0; j < 2; ++j)
          yv[j] = __builtin_amdgcn_raw_buffer_load_b128(
              ry, 4 * (int)((lr0 + 2 * j) * a.lddy + 4 * gl), 0, 0);
      }
      float rsc[2] = {1.0f, 1.0f};  // ROLL 2: row_scale ('rw'), loaded ahead of the next quad's slots
      float acc[2][4];
      if constexpr (ROLL == 0)
        gather_row2_meta<U, MAXM>(rdy, ldy_b, a.col, a.w, cur[0], cur[1], gl, grp, acc[0], acc[1],
                                  a.win_mask, a.slot_map);
      else
        gather_row2_roll<U>(rdy, ldy_b, a.rowptr, a.col, a.w, r0 + lr0, r0 + lr0 + 2, cur[0], cur[1],
                            nxt[0], nxt[1], q + kBsNG < n_quads, gl, grp, acc[0], acc[1], win,
                            a.row_scale, a.n_rows, rsc);
      if constexpr (HCS) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const float4 y = __builtin_bit_cast(float4, yv[j]);
          hc[0] = __fadd_rn(hc[0], y.x);
          hc[1] = __fadd_rn(hc[1], y.y);
          hc[2] = __fadd_rn(hc[2], y.z);
          hc[3] = __fadd_rn(hc[3], y.w);
        }
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int64_t row = r0 + lr0 + 2 * j;
        if (a.row_scale != nullptr && row < a.n_rows) {
          const float sc = ROLL == 2 ? rsc[j] : a.row_scale[row];
#pragma unroll
          for (int t = 0; t < 4; ++t) acc[j][t] = __fmul_rn(acc[j][t], sc);
        }
      }
      const int b = (int)(i & 1);
      const int gen = (int)(i >> 1);
      if (!lds_wait_ge(freed + b, gen, abort_word, A.spin)) break;
      char *buf = lds + b * kRing;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        store_row_terms(buf, lr0 + 2 * j, gl, acc[j]);
        // the X rows as they are (split by the MFMA waves)
        *reinterpret_cast<u32x4 *>(buf + kDsXOff + 4 * ((lr0 + 2 * j) * kDsXLd + 4 * gl)) = zv[j];
        if constexpr (MRING && EPI != EPI_STORE) {
          if (gl < 4)
            *reinterpret_cast<uint32_t *>(buf + kDsMaskOff + 4 * ((lr0 + 2 * j) * 4 + gl)) = mv[j];
          if (EPI == EPI_RELU_DIV && gl == 4)
            *reinterpret_cast<uint32_t *>(buf + kDsDivOff + 4 * (lr0 + 2 * j)) = mv[j];
        }
      }
      lds_signal(filled + b, 4, lane);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        cur[j] = nxt[j];
        nxt[j] = nn[j];
        if constexpr (ROLL == 2) meta_deg(nxt[j]);
      }
    }
  } else {
    // -------------------------------- MFMA waves ----------------------------
    const int m = wave - kBsNG;  // dX columns 16 m .. 16 m + 15
    // dW tiles (gemm_bwd's mapping): rows 32 ti, columns 32 (tj0 + s)
    const int ti = m >> 1, tj0 = 2 * (m & 1);
    auto read8 = [&](const char *base, const int (&o)[2]) {
      const v4i16 x0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16_t *)(base + o[0]));
      const v4i16 x1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16_t *)(base + o[1]));
      const short y[8] = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
      return __builtin_bit_cast(bf16x8, y);
    };
    const int bit = 4 * m + g4;  // mask bit of this lane's columns (word r: column 16 m + 4 g4 + r)
    for (int64_t i = 0; i < n_my; ++i) {
      // the lane-derived LDS offsets, recomputed per chunk from an opaque copy
      // of the lane id: hoisted out of the loop they were spilled, and every
      // scratch reload waited behind s_waitcnt vmcnt(0) -- i.e. for the
      // previous chunk's dX stores too
      int lane_o = lane;
      asm volatile("" : "+v"(lane_o));
      const int l16 = lane_o & 15, g4 = lane_o >> 4, h = lane_o >> 5;
      int offb[2][2];
      {
        const int q = (lane_o >> 2) & 3, p4 = lane_o & 3;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
          for (int r = 0; r < 2; ++r)
            offb[s2][r] = img_off(8 * h + q + 4 * r, 4 * (tj0 + s2) + 2 * (g4 & 1) + (p4 >> 1)) +
                          8 * (p4 & 1);
      }
      const int b = (int)(i & 1);
      const int gen = (int)(i >> 1);
      const int64_t c = chunk_of(i);
      const int64_t r0 = c * kXwRows;
      const uint32_t rv = rows_in(c);
      u32x4 mk[2] = {};
      float dv[2] = {1.0f, 1.0f};
      if constexpr (EPI != EPI_STORE && !MRING) {
        const auto rm = buf_rsrc(a.relu_mask + r0 * 4, rv * 16u);
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
          mk[rt] = __builtin_amdgcn_raw_buffer_load_b128(rm, 16 * (16 * rt + l16), 0, 0);
        if constexpr (EPI == EPI_RELU_DIV) {
          const auto rd = buf_rsrc(a.row_div + r0, rv * 4u);
#pragma unroll
          for (int rt = 0; rt < 2; ++rt)
            dv[rt] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rd, 4 * (16 * rt + l16), 0, 0));
        }
      }
      if (!lds_wait_ge(filled + b, kXwRows * (gen + 1), abort_word, A.spin)) break;
      uint32_t mbits[2] = {0u, 0u};  // MRING: this lane's 4 mask bits per row tile
      if constexpr (EPI != EPI_STORE && MRING) {  // from the ring (the gather waves loaded them)
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) {
          const u32x4 w4 = *reinterpret_cast<const u32x4 *>(lds + b * kRing + kDsMaskOff + 16 * (16 * rt + l16));
#pragma unroll
          for (int r = 0; r < 4; ++r) mbits[rt] |= ((w4[r] >> bit) & 1u) << r;
          if constexpr (EPI == EPI_RELU_DIV)
            dv[rt] = *reinterpret_cast<const float *>(lds + b * kRing + kDsDivOff + 4 * (16 * rt + l16));
        }
      }
      if constexpr (EPI == EPI_RELU_DIV) {
        // rows past the end read divisor 0: make it 1, so their zero rows stay
        // 0 (not 0 / 0) in the dX images dWl reads
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
          if ((uint32_t)(16 * rt + l16) >= rv) dv[rt] = 1.0f;
      }
      const char *buf = lds + b * kRing;
      {
        // (first: nothing but the dW accumulators is live across it)
        // dW += X^T dH: X^T fragments (lane: column 32 ti + lc of rows
        // 16 ks + 8 h + j) read from the fp32 rows and split here, dH^T
        // fragments from the term images
          if (!(A.dbg & kDbgMask & 1)) {
          const float *xr = reinterpret_cast<const float *>(buf + kDsXOff) + 32 * ti + (lane_o & 31);
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            float xv[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) xv[j] = xr[(16 * ks + 8 * h + j) * kDsXLd];
            bf16x8 fa[3];
            split3_bf16(xv, fa[0], fa[1], fa[2]);
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
              bf16x8 fb[3];
#pragma unroll
              for (int t = 0; t < 3; ++t) fb[t] = read8(buf + ks * 16 * 256 + t * kXwImg, offb[s2]);
              accw[s2] = mfma_x6(fa[0], fa[1], fa[2], fb[0], fb[1], fb[2], accw[s2]);
            }
          }
        }
        }
      const auto rx = buf_rsrc(a.dX + r0 * a.lddx, rv * (uint32_t)a.lddx * 4u);
      f32x4_t acc2[2];
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc2[rt][r] = 0.0f;
      // W^T fragment rows from the LDS copy
      const float *wq = reinterpret_cast<const float *>(lds + kDsWOff) + (16 * m + l16) * kDsXLd + 8 * g4;
      float4 wn0{}, wn1{};
      if (!(A.dbg & kDbgMask & 8)) {  // dbg 8: no W^T loads (timing only: dX wrong)
        wn0 = *reinterpret_cast<const float4 *>(wq);
        wn1 = *reinterpret_cast<const float4 *>(wq + 4);
      }
      // dX == NULL: dW alone (the same partials as with dX)
      if (a.dX != nullptr) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        bf16x8 wk[3];
        {
          const float v8[8] = {wn0.x, wn0.y, wn0.z, wn0.w, wn1.x, wn1.y, wn1.z, wn1.w};
              if (ks + 1 < 4 && !(A.dbg & kDbgMask & 8)) {
            wn0 = *reinterpret_cast<const float4 *>(wq + 32 * (ks + 1));
            wn1 = *reinterpret_cast<const float4 *>(wq + 32 * (ks + 1) + 4);
          }
              split3_bf16(v8, wk[0], wk[1], wk[2]);
        }
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) {
          const int off = img_off(16 * rt + l16, 4 * ks + g4);
          const bf16x8 xh = *reinterpret_cast<const bf16x8 *>(buf + off);
          const bf16x8 xm = *reinterpret_cast<const bf16x8 *>(buf + kXwImg + off);
          const bf16x8 xl = *reinterpret_cast<const bf16x8 *>(buf + 2 * kXwImg + off);
          acc2[rt] = mfma16_x6_at(wk, xh, xm, xl, acc2[rt]);
        }
      }
#pragma unroll
      for (int rt = 0; rt < 2; ++rt) {
        const int row = 16 * rt + l16;
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          v[r] = acc2[rt][r];
          if constexpr (EPI != EPI_STORE) {
            const uint32_t on = MRING ? (mbits[rt] >> r) & 1u : (mk[rt][r] >> bit) & 1u;
            v[r] = on ? v[r] : 0.0f;
            cs[r] = __fadd_rn(cs[r], v[r]);  // rows past the end: zero mask words
            if constexpr (EPI == EPI_RELU_DIV) v[r] = __fdiv_rn(v[r], dv[rt]);
          }
        }
        __builtin_amdgcn_raw_buffer_store_b128(
            __builtin_bit_cast(u32x4, make_float4(v[0], v[1], v[2], v[3])), rx,
            4 * (int)(row * a.lddx + 16 * m + 4 * g4), 0, MGCN_NT_OUT);
      }
      }
      const int old = lds_signal(mdone + b, 1, lane);
      if (old == kBsNM * gen + kBsNM - 1) lds_signal(freed + b, 1, lane);
    }
  }
  __syncthreads();
  // a hand-off gave up: this launch's dX / dW are incomplete -- say so (the
  // host turns the word into MGCN_EDEVICE) instead of returning them silently
  if (wave == 0 && lds_load(abort_word) != 0) report_device_error(A.err, kDevErrDws);
  if (wave >= kBsNG) {
    const int m = wave - kBsNG;
    {
      const int h = lane >> 5, lc = lane & 31;
      const int ti = m >> 1, tj0 = 2 * (m & 1);
      float *slab = a.dw_partial + (int64_t)blockIdx.x * kXwF * kXwF;
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = 32 * ti + (r & 3) + 8 * (r >> 2) + 4 * h;
          slab[row * kXwF + 32 * (tj0 + s2) + lc] = accw[s2][r];
        }
    }
    if constexpr (EPI != EPI_STORE) {
      float *red = reinterpret_cast<float *>(lds);  // [16 row lanes][128]
      *reinterpret_cast<float4 *>(red + l16 * kXwF + 16 * m + 4 * g4) =
          make_float4(cs[0], cs[1], cs[2], cs[3]);
    }
  }
  if constexpr (HCS) {  // (past the dX column sums' [16][128] in LDS)
    float *red2 = reinterpret_cast<float *>(lds) + 16 * kXwF;
    if (wave < kBsNG)
      *reinterpret_cast<float4 *>(red2 + (2 * wave + grp) * kXwF + 4 * gl) =
          make_float4(hc[0], hc[1], hc[2], hc[3]);
  }
  if (EPI != EPI_STORE || HCS) {
    __syncthreads();
    if constexpr (EPI != EPI_STORE) {
      if (tid < kXwF) {
        const float *red = reinterpret_cast<const float *>(lds);
        float s = 0.0f;
#pragma unroll
        for (int l = 0; l < 16; ++l) s = __fadd_rn(s, red[l * kXwF + tid]);
        a.colsum_partial[(int64_t)blockIdx.x * kXwF + tid] = s;
      }
    }
    if (HCS && tid >= kXwF && tid < 2 * kXwF) {
      const int f = tid - kXwF;
      const float *red2 = reinterpret_cast<const float *>(lds) + 16 * kXwF;
      float s = 0.0f;
#pragma unroll
      for (int l = 0; l < 16; ++l) s = __fadd_rn(s, red2[l * kXwF + f]);
      A.hcs_partial[(int64_t)blockIdx.x * kXwF + f] = s;
    }
  }
  XTAIL_EXIT(1, n_my);
}

template <int U, int MODE, int ROLL>
int launch_bs_ur(const XbsArgs &a, int epi, int grid, hipStream_t s) {
  if (epi == EPI_RELU_DIV)
    hipLaunchKernelGGL((spmm_xw_bwd_ws_kernel<U, EPI_RELU_DIV, MODE, ROLL>), dim3(grid),
                       dim3(kBsThreads), 0, s, a);
  else if (epi == EPI_RELU)
    hipLaunchKernelGGL((spmm_xw_bwd_ws_kernel<U, EPI_RELU, MODE, ROLL>), dim3(grid),
                       dim3(kBsThreads), 0, s, a);
  else
    hipLaunchKernelGGL((spmm_xw_bwd_ws_kernel<U, EPI_STORE, MODE, ROLL>), dim3(grid),
                       dim3(kBsThreads), 0, s, a);
  return check_launch("spmm_xw_bwd_ws_kernel");
}

template <int U, int MODE>
int launch_bs_u(const XbsArgs &a, int epi, int grid, hipStream_t s) {
  if constexpr (MODE == kBsDwsM) {
    return launch_bs_ur<U, MODE, 0>(a, epi, grid, s);
  } else {
    return g_opt.xw_ws_roll == 0 ? launch_bs_ur<U, MODE, 0>(a, epi, grid, s)
                          : launch_bs_ur<U, MODE, 2>(a, epi, grid, s);
  }
}

template <int MODE>
int launch_bs(const XbsArgs &a, int epi, int grid, hipStream_t s) {
  if constexpr (MODE == kBsDwsM) {  // the winner words take registers: 3 slots per row
    return launch_bs_u<3, MODE>(a, epi, grid, s);
  } else {
    return g_opt.xw_ws_full_unroll == 4 ? launch_bs_u<4, MODE>(a, epi, grid, s)
         : g_opt.xw_ws_full_unroll == 5 ? launch_bs_u<5, MODE>(a, epi, grid, s)
                                 : launch_bs_u<6, MODE>(a, epi, grid, s);
  }
}

// the warp-specialised launch's failure plumbing: spin bound, error word
int bs_prepare(XbsArgs &sa) {
  sa.dbg = MGCN_EXPERIMENT ? g_opt.xw_ws_dbg : 0;  // (always 0 in the product)
  sa.spin = (uint32_t)g_opt.ws_spin_limit;
  sa.err = device_error_word();
  return sa.err == nullptr ? MGCN_EHIP : MGCN_OK;
}

}  // namespace

int launch_dws(const void *xb, int epi, int grid, float *hcs_partial, hipStream_t s) {
  XbsArgs sa{};
  sa.b = *static_cast<const XbArgs *>(xb);
  if (int rc = bs_prepare(sa)) return rc;
  sa.hcs_partial = hcs_partial;
  return hcs_partial             ? launch_bs<kBsDwsH>(sa, epi, grid, s)
         : sa.b.win_mask != nullptr ? launch_bs<kBsDwsM>(sa, epi, grid, s)
                                    : launch_bs<kBsDws>(sa, epi, grid, s);
}

#if MGCN_EXPERIMENT
int dws_tail_take(unsigned long long *host) { return tail_take(HIP_SYMBOL(g_tail), host); }
#endif

}  // namespace mgcn
