// The two-phase fused adjoint at F = 128, spmm_xw_bwd_kernel, with its launch
// ladder and the phase-profile build's stamps (xw128.h: the design, the
// shared gather primitives and chunk helpers).

#include "xw128.h"

namespace mgcn {
namespace {

typedef __attribute__((address_space(3))) void lds_void_t;

// ---------------------------------------------------------------------------
// Backward.  LDS: X images, dH images (single-buffered: two barriers per
// chunk), the chunk's mask / divisor words, the dX staging tile.  dX: wave w
// owns columns 16 w .. +15; its W^T fragments are re-read from L2 (W is
// 64 KB) and split per chunk -- held for the whole kernel they would take 48
// VGPRs beside the gather's and dW's (the dX-only form, DW = false, holds
// them: it has no dW accumulators).
constexpr int kXbHOff = 3 * kXwImg;
constexpr int kXbMaskOff = 6 * kXwImg;                 // [32][4] mask words
constexpr int kXbDivOff = kXbMaskOff + kXwRows * 16;   // [32] row divisors
constexpr int kXbStageOff = kXbDivOff + kXwRows * 4;
constexpr int kXbColsumOff = kXbStageOff + kXwStage;     // [512 threads][4] column sums
constexpr int kXbLds = kXbColsumOff + kXwThreads * 16;
static_assert(2 * kXbLds <= 160 * 1024, "two backward workgroups per CU");

#ifdef MGCN_XW_PROFILE
// phase timestamps of workgroup 0, waves 0 and 7 (scripts/prof_fused.py):
// [wave][chunk iteration][stamp]
__device__ unsigned long long g_xprof[2][64][6];
#define XPROF(it, k)                                                                      \
  if (blockIdx.x == 0 && (wave == 0 || wave == 7) && (it) < 64 && lane == 0)              \
    g_xprof[wave == 7][it][k] = __builtin_readcyclecounter();
#else
#define XPROF(it, k)
#endif

// DW = false: dX only (X == NULL) -- the caller forms dW = Z^T dY from the
// forward's aggregate (mgcn_gemm_bwd, dW-only), so the chunk's X rows, their
// images and the dW MFMAs drop out.
template <int U, bool DX, int EPI, bool MAXM, bool DW = true, bool PK = false>
__global__ __launch_bounds__(kXwThreads, 2 * kXwPerCU) void spmm_xw_bwd_kernel(const XbArgs a) {
  static_assert(!PK || (!DW && !MAXM), "the packed gather serves the dX-only adjoint");
  __shared__ __attribute__((aligned(16))) char lds[kXbLds];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int gl = lane & 31, grp = lane >> 5;
  const int h = lane >> 5, lc = lane & 31;
  const int l16 = lane & 15, g4 = lane >> 4;
  const int64_t n_chunks = (a.n_rows + kXwRows - 1) / kXwRows;
  const auto rdy = buf_rsrc(PK ? nullptr : a.dY, PK ? 0u : (uint32_t)(a.n_cols * a.lddy * 4));
  const uint32_t ldy_b = (uint32_t)a.lddy * 4u;
  Pk128 pk{};
  u32x2 hh[PK ? U : 1];
  if constexpr (PK) {
    pk.r = buf_rsrc(a.pk, a.pk_bytes);
    pk.rbits = a.pk_rbits;
    pk.head = a.pk_head;
    pk.base = a.pk_base[lane];
  }
  float *stage = reinterpret_cast<float *>(lds + kXbStageOff);
  const float *wp = a.W + (int64_t)(16 * wave + l16) * a.ldw + 8 * g4;  // B[k][n] = W[n][k]

  // dW fragment offsets (gemm_bwd mapping): lane = 16 g + 4 q + p reads
  // row 8 h + q (+ 4) of chunk (col0 >> 3) + 2 (g & 1) + (p >> 1), half p & 1
  const int q = (lane >> 2) & 3, p4 = lane & 3;
  auto frag_off = [&](int col0, int second) {
    return img_off(8 * h + q + 4 * second, (col0 >> 3) + 2 * (g4 & 1) + (p4 >> 1)) + 8 * (p4 & 1);
  };
  const int ti = wave >> 1, tj0 = 2 * (wave & 1);
  int offa[2], offb[2][2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    offa[r] = frag_off(32 * ti, r);
    offb[0][r] = kXbHOff + frag_off(32 * tj0, r);
    offb[1][r] = kXbHOff + frag_off(32 * (tj0 + 1), r);
  }
  auto read8 = [&](const char *base, const int (&o)[2]) {
    const v4i16 x0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16_t *)(base + o[0]));
    const v4i16 x1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16_t *)(base + o[1]));
    const short y[8] = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
    return __builtin_bit_cast(bf16x8, y);
  };

  f32x16 accw[2];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int r = 0; r < 16; ++r) accw[s][r] = 0.0f;
  const int ncol = 16 * wave + l16;  // dX column of this lane
  const int xoff = 4 * (int)((tid >> 5) * a.ldx + 4 * (tid & 31));
  // dX only: no dW accumulators, so this wave's W^T fragments are split once
  // and held (48 VGPRs) instead of re-read from L2 every chunk
  bf16x8 wt[DW ? 1 : 4][3];
  if constexpr (!DW) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const float4 w0 = *reinterpret_cast<const float4 *>(wp + 32 * ks);
      const float4 w1 = *reinterpret_cast<const float4 *>(wp + 32 * ks + 4);
      const float v[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
      split3_bf16(v, wt[ks][0], wt[ks][1], wt[ks][2]);
    }
  }

  // staged dX rows of chunk `c` -> dX (16 B per lane, whole rows)
  // The ReLU mask, the bias column sums and mean's division are applied here,
  // on whole staged rows, rather than in the MFMA epilogue (whose registers
  // are the kernel's peak): thread (q, lc) owns features 4 lc .. 4 lc + 3 of
  // rows q and 16 + q; feature 4 lc + j is bit lc of the row's mask word j.
  // column sums of this thread's features, kept in LDS (registers are the
  // kernel's limit)
  float *cs = reinterpret_cast<float *>(lds + kXbColsumOff) + 4 * tid;
  if constexpr (DX && EPI != EPI_STORE)
    *reinterpret_cast<float4 *>(cs) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  auto flush = [&](int64_t c) {
    const int64_t r0 = c * kXwRows;
    const int64_t left = a.n_rows - r0;
    const uint32_t rows_in = (uint32_t)(left >= kXwRows ? kXwRows : left);
    const auto rx = buf_rsrc(a.dX + r0 * a.lddx, rows_in * (uint32_t)a.lddx * 4u);
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int lr = 16 * m + (tid >> 5);
      const float *srow = stage + lr * kXwStageLd;
      float v[4];
      *reinterpret_cast<float4 *>(v) = *reinterpret_cast<const float4 *>(srow + 4 * lc);
      if constexpr (EPI != EPI_STORE) {
        const u32x4 mw = *reinterpret_cast<const u32x4 *>(srow + kXwF);
        // rows past the end were staged from zero dH rows with zero mask words
        float c[4];
        *reinterpret_cast<float4 *>(c) = *reinterpret_cast<const float4 *>(cs);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[j] = ((mw[j] >> lc) & 1u) ? v[j] : 0.0f;
          c[j] = __fadd_rn(c[j], v[j]);
        }
        *reinterpret_cast<float4 *>(cs) = *reinterpret_cast<const float4 *>(c);
        if constexpr (EPI == EPI_RELU_DIV) {
          const float d = srow[kXwF + 4];
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = __fdiv_rn(v[j], d);
        }
      }
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, *reinterpret_cast<float4 *>(v)),
                                             rx, 4 * (int)(lr * a.lddx + 4 * lc), 0, MGCN_NT_OUT);
    }
  };

  // dX only: the row metadata runs one row ahead as in the forward
  // (gather_row_meta: row k + 1's first edge slots and row k + 2's pointers
  // load under row k's gathers)
  const int64_t n_my = my_chunks(n_chunks);
  const RowSeq seq{(int64_t)blockIdx.x * kXwRows + 2 * wave + grp, (int64_t)gridDim.x * kXwRows,
                   a.n_rows};
  RowMeta cur{}, nxt{};
  if constexpr (!DW && !MAXM) {
    meta_rowptr(a.rowptr, seq.row(0), seq.row(0) < a.n_rows, cur);
    if constexpr (PK) {
      meta_first_pk(pk, a.col, a.w, gl, cur);
      pk128_headers<U>(pk, cur.mc, grp, 0, cur.deg < 32 ? cur.deg : 32, 8u * (uint32_t)(gl >> 3), hh);
    } else {
      meta_first(a.col, a.w, gl, cur);
    }
    meta_rowptr(a.rowptr, seq.row(1), seq.row(1) < a.n_rows, nxt);
  }
  int it = 0;
  for (int64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x, ++it) {
    const int64_t r0 = chunk * kXwRows;
    const int64_t left = a.n_rows - r0;
    const uint32_t rows_in = (uint32_t)(left >= kXwRows ? kXwRows : left);
    XPROF(it, 0);
    if constexpr (DX) {
      if (it > 0) flush(chunk - gridDim.x);
    }
    // the chunk's X rows (q and 16 + q, float4 tid & 31), issued first so
    // they land under the gathers
    u32x4 xa{}, xb{};
    if constexpr (DW) {
      const auto rxx = buf_rsrc(a.X + r0 * a.ldx, rows_in * (uint32_t)a.ldx * 4u);
      xa = __builtin_amdgcn_raw_buffer_load_b128(rxx, xoff, 0, MGCN_NT_AUX);
      xb = __builtin_amdgcn_raw_buffer_load_b128(rxx, xoff + 64 * (int)a.ldx, 0, MGCN_NT_AUX);
    }
    // the chunk's mask / divisor words straight into LDS (LDS-DMA: no registers
    // held across the gathers); rows past the end read row r0 and are never used
    if constexpr (DX && EPI != EPI_STORE) {
      if (wave == 0 && h == 0) {
        const int64_t mr = r0 + ((uint32_t)lc < rows_in ? lc : 0);
        __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(a.relu_mask + mr * 4),
                                         (lds_void_t *)(lds + kXbMaskOff), 16, 0, 0);
        if constexpr (EPI == EPI_RELU_DIV)
          __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(a.row_div + mr),
                                           (lds_void_t *)(lds + kXbDivOff), 4, 0, 0);
      }
    }

    // ---- Phase A: dH rows of the chunk -> bf16 images; X rows -> images --
#pragma unroll 1
    for (int p = 0; p < 2; ++p) {
      const int lr = 16 * p + 2 * wave + grp;
      const int64_t row = r0 + lr;
      const bool row_ok = row < a.n_rows;
      int deg;
      float acc[4];
      if constexpr (!DW && !MAXM) {
        const int64_t k = 2 * it + p;
        if constexpr (PK)
          meta_first_pk(pk, a.col, a.w, gl, nxt);
        else
          meta_first(a.col, a.w, gl, nxt);
        RowMeta nn;
        const int64_t rk2 = seq.row(k + 2);
        meta_rowptr(a.rowptr, rk2, rk2 < a.n_rows && k + 2 < 2 * n_my, nn);
        if constexpr (PK)
          gather_row_meta_pk<U>(pk, a.col, a.w, cur, nxt, gl, grp, acc, hh);
        else
          gather_row_meta<U>(rdy, ldy_b, a.col, a.w, cur, gl, grp, acc);
        cur = nxt;
        nxt = nn;
      } else {
        gather_row<U, MAXM>(rdy, ldy_b, a.rowptr, a.col, a.w, row, row_ok, gl, grp, acc, deg,
                            a.win_mask, a.slot_map);
      }
      if (a.row_scale != nullptr && row_ok) {
        const float sc = a.row_scale[row];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = __fmul_rn(acc[j], sc);
      }
      store_row_terms(lds + kXbHOff, lr, gl, acc);
    }
    XPROF(it, 1);
    if constexpr (DW) {
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const float4 v = __builtin_bit_cast(float4, m == 0 ? xa : xb);
        const float f[4] = {v.x, v.y, v.z, v.w};
        store_row_terms(lds, 16 * m + (tid >> 5), lc, f);
      }
    }
    // the mask / divisor LDS-DMA (older than this wave's gathers) has landed
    if constexpr (DX && EPI != EPI_STORE)
      if (wave == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // this wave's W^T fragments (B[k][n] = W[n][k], 32 floats per lane): issued
    // before the barrier, so the L2 round trip (thousands of cycles while the
    // other workgroup's gathers load the memory system) is hidden by the
    // barrier wait and the dW MFMAs
    float4 wr[4][2];
    if constexpr (DX && DW) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int j = 0; j < 2; ++j) wr[ks][j] = *reinterpret_cast<const float4 *>(wp + 32 * ks + 4 * j);
    }
    __syncthreads();
    XPROF(it, 2);

    // ---- Phase B1: dW += X^T dH (two 16-row k-steps) ---------------------
#pragma unroll
    for (int ks = 0; ks < (DW ? 2 : 0); ++ks) {
      const char *kb = lds + ks * 16 * 256;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        bf16x8 fa[3], fb[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) {
          fa[t] = read8(kb + t * kXwImg, offa);
          fb[t] = read8(kb + t * kXwImg, offb[s]);
        }
        accw[s] = mfma_x6(fa[0], fa[1], fa[2], fb[0], fb[1], fb[2], accw[s]);
      }
    }
    XPROF(it, 3);
    // ---- Phase B2: dX = relu'(lower) (dH W^T) [/ row_div] -> staging ------
    if constexpr (DX) {
      f32x4_t acc2[2];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc2[t][r] = 0.0f;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        if constexpr (DW) {
          bf16x8 wb[3];
          const float v[8] = {wr[ks][0].x, wr[ks][0].y, wr[ks][0].z, wr[ks][0].w,
                              wr[ks][1].x, wr[ks][1].y, wr[ks][1].z, wr[ks][1].w};
          split3_bf16(v, wb[0], wb[1], wb[2]);
          mfma_rows(lds + kXbHOff, wb, ks, l16, g4, acc2);
        } else {
          mfma_rows(lds + kXbHOff, wt[ks], ks, l16, g4, acc2);
        }
      }
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) stage[(16 * t + 4 * g4 + r) * kXwStageLd + ncol] = acc2[t][r];
      if constexpr (EPI != EPI_STORE) {
        // the chunk's mask words (and divisors) travel with the staged rows
        if (wave == 0 && h == 0) {
          *reinterpret_cast<u32x4 *>(stage + lc * kXwStageLd + kXwF) =
              *reinterpret_cast<const u32x4 *>(lds + kXbMaskOff + 16 * lc);
          if constexpr (EPI == EPI_RELU_DIV)
            stage[lc * kXwStageLd + kXwF + 4] = *reinterpret_cast<const float *>(lds + kXbDivOff + 4 * lc);
        }
      }
    }
    XPROF(it, 4);
    __syncthreads();
    XPROF(it, 5);
  }
  if constexpr (DX) {
    if (it > 0) flush(blockIdx.x + (int64_t)(it - 1) * gridDim.x);  // staged before the last barrier
  }

  // dW partial slab of this workgroup; C map: col = lc, row = (r & 3) + 8 (r >> 2) + 4 h
  float *slab = a.dw_partial + (int64_t)blockIdx.x * kXwF * kXwF;
#pragma unroll
  for (int s = 0; s < (DW ? 2 : 0); ++s)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = 32 * ti + (r & 3) + 8 * (r >> 2) + 4 * h;
      slab[row * kXwF + 32 * (tj0 + s) + lc] = accw[s][r];
    }
  if constexpr (DX && EPI != EPI_STORE) {
    // fold the 16 row slots of each column in fixed order: thread (q, lc)
    // holds features 4 lc .. 4 lc + 3 at cs slot 32 q + lc
    __syncthreads();
    const float *red = reinterpret_cast<const float *>(lds + kXbColsumOff);
    if (tid < kXwF) {
      float c = 0.0f;
#pragma unroll
      for (int q = 0; q < 16; ++q) c = __fadd_rn(c, red[4 * (32 * q + (tid >> 2)) + (tid & 3)]);
      a.colsum_partial[(int64_t)blockIdx.x * kXwF + tid] = c;
    }
  }
}

template <int U, bool DX, int EPI, bool MAXM, bool DW = true, bool PK = false>
int launch_xb(const XbArgs &a, int grid, hipStream_t s) {
  hipLaunchKernelGGL((spmm_xw_bwd_kernel<U, DX, EPI, MAXM, DW, PK>), dim3((unsigned)grid),
                     dim3(kXwThreads), 0, s, a);
  return check_launch("spmm_xw_bwd_kernel");
}

// dX only (no X, no dW), sum adjoint
template <int U, bool PK = false>
int launch_xb_dx(const XbArgs &a, int epi, int grid, hipStream_t s) {
  if (epi == EPI_RELU_DIV) return launch_xb<U, true, EPI_RELU_DIV, false, false, PK>(a, grid, s);
  if (epi == EPI_RELU) return launch_xb<U, true, EPI_RELU, false, false, PK>(a, grid, s);
  return launch_xb<U, true, EPI_STORE, false, false, PK>(a, grid, s);
}

template <int U, bool MAXM>
int launch_xb_m(const XbArgs &a, int epi, int grid, hipStream_t s) {
  if (a.dX == nullptr) return launch_xb<U, false, EPI_STORE, MAXM>(a, grid, s);
  if (epi == EPI_RELU_DIV) return launch_xb<U, true, EPI_RELU_DIV, MAXM>(a, grid, s);
  if (epi == EPI_RELU) return launch_xb<U, true, EPI_RELU, MAXM>(a, grid, s);
  return launch_xb<U, true, EPI_STORE, MAXM>(a, grid, s);
}

template <int U>
int launch_xb_u(const XbArgs &a, int epi, int grid, hipStream_t s) {
  return a.win_mask != nullptr ? launch_xb_m<U, true>(a, epi, grid, s)
                               : launch_xb_m<U, false>(a, epi, grid, s);
}

}  // namespace

int launch_xb_bwd(const void *xb, int epi, int grid, bool dx_only, bool packed, hipStream_t s) {
  const XbArgs &a = *static_cast<const XbArgs *>(xb);
  if (packed) {
    constexpr bool X = MGCN_EXPERIMENT;  // (the product build instantiates U = 3 only)
    if (X && g_opt.xw_pk_bwd_unroll == 2) return launch_xb_dx<X ? 2 : 3, true>(a, epi, grid, s);
    if (X && g_opt.xw_pk_bwd_unroll == 4) return launch_xb_dx<X ? 4 : 3, true>(a, epi, grid, s);
    return launch_xb_dx<3, true>(a, epi, grid, s);
  }
  if (dx_only)
    return g_opt.spmm_xw_unroll == 8 ? launch_xb_dx<8>(a, epi, grid, s)
                                     : launch_xb_dx<4>(a, epi, grid, s);
  return g_opt.spmm_xw_unroll == 8 ? launch_xb_u<8>(a, epi, grid, s)
                                   : launch_xb_u<4>(a, epi, grid, s);
}

}  // namespace mgcn

#ifdef MGCN_XW_PROFILE
extern "C" int mgcn_debug_xw_prof(unsigned long long *host) {
  using namespace mgcn;
  MGCN_HIP_TRY(hipDeviceSynchronize());
  MGCN_HIP_TRY(hipMemcpyFromSymbol(host, HIP_SYMBOL(g_xprof), sizeof(g_xprof)));
  return MGCN_OK;
}
#endif
