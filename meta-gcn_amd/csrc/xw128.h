// Fused GCN layer kernels on gfx950: the aggregation and the layer's dense
// product in one pass, forward and backward (F_in = F_out = 128, sum / mean).
// What the four kernels share (internal, device + host): the constants, the
// argument structs, the gather primitives, the chunk helpers and each file's
// launch functions.  The kernels: fused_fwd.hip, fused_bwd.hip (two-phase),
// fused_dws.hip, fused_fwd_ws.hip (warp-specialised); the C entry points and
// the routing between the kernels: fused.hip.
//
// Forward:   Y = epi( (A_norm X) W + b ),   epi = optional ReLU (+ row mask)
// Backward:  dH = A_norm^T dY [* row_scale];  dW = X^T dH;
//            dX = relu'(lower) (dH W^T) [/ row_div],  colsum = sum_rows dX
//
// The reference computes a layer as  x @ W  then  gather -> * norm ->
// scatter_add  (src/gcn_meta/models/gcn_base_models.py:201, 223-237; PyG
// GCNConv: x @ W then propagate), and autograd runs the adjoints in reverse.
// Unfused here that is two launches per direction: mgcn_gemm_nn (reads X,
// writes H = X W) + mgcn_spmm_fwd (gathers H), and mgcn_spmm_bwd (writes dH)
// + mgcn_gemm_bwd (reads X and dH, writes dX).  For a linear aggregator
// A (X W) = (A X) W, so the forward gathers X itself and multiplies the
// aggregated rows of a 32-row chunk by W on MFMA in the same workgroup, and
// the backward multiplies the chunk's dH rows by W^T and X^T before they
// ever leave the workgroup.  H and dH never exist: per layer at config 2 this
// removes 1 GB of HBM traffic in each direction and a launch.  Max does not
// commute with W and keeps the two-launch path.
//
// Numerics: aggregated rows are summed exactly as the SpMM sums (edge order,
// separately rounded products and adds: mgcn_spmm_fwd / _bwd bit for bit);
// the dense products are the bf16x6 MFMA arithmetic of gemm.hip.  The
// forward's association differs from the reference's (A (X W) vs (A X) W),
// so the layer output matches within fp32 tolerance, not bitwise -- except
// for W = I, where every bf16x6 product is exact.  The backward's dX is
// mgcn_gemm_bwd's bit for bit (same dH, same products and order); dW and
// the column sums fold the same products over a different split-K grid.
//
// Chunk layout (both directions): persistent 512-thread workgroups (8
// waves), two per CU; chunk c (rows 32 c .. 32 c + 31) goes to workgroup
// c % grid.
//   Phase A (gather): row 16 p + 2 wave + grp of the chunk is owned by the
//     32-lane group grp of wave `wave` in pass p; lane gl holds features
//     4 gl .. 4 gl + 3 of every gathered 512-B row, U gathers in flight per
//     group, folded in edge order; the finished row is split into the
//     chunk's bf16 hi / mid / lo images (x6.h layout).
//   Phase B (MFMA): wave w owns output columns 16 w .. 16 w + 15 of the
//     chunk (v_mfma_f32_16x16x32_bf16); the backward's dW tiles are
//     gemm_bwd's (32x32x16 on transposed image reads).  Results go to an
//     fp32 staging tile in LDS.
//   The staged tile is written out as whole 512-B rows (16 B per lane) at
//   the start of the next chunk, beside its gathers: 4-byte column stores
//   straight from the MFMA layout cost 0.19 ms per 512 MB (store issue).
// The full adjoint (DWS) and the dense forward (spmm_xw_fwd_ws_kernel) run
// the same chunks cut by role instead: one 1024-thread workgroup per CU, 8
// gather waves that never wait for a barrier, 8 MFMA waves, an LDS ring.
//
// Roofline: HBM-bound like the SpMM, with the GEMMs' bytes removed:
//   forward  8 (N + 1) + nnz (4 col + 4 w + 4 F) + 4 N F (+ 16 N mask)
//   backward the same + 4 N F (X) (+ 16 N mask)
// and 2 N F^2 (forward) / 4 N F^2 (backward) x 6 bf16 MFMA flops under it.

#pragma once

#include "mgcn_internal.h"
#include "x6.h"

// cache policy of the streamed (read-once / written-once) rows -- Z written
// by the forward, the own X rows of the backward: 2 = nt (config 2: 5.16 ->
// 5.11-5.12 ms/step, A/B on one box: the fwd-with-Z launch 0.933 -> 0.917 ms,
// the full backward 1.14 -> 1.13 ms)
#ifndef MGCN_NT_AUX
#define MGCN_NT_AUX 2
#endif
// and for the layer outputs (Y forward, dX backward), although they are the
// next kernel's gathered table: the config-2 tables are twice the 256-MB
// Infinity Cache, and allocating the written lines there costs more than it
// saves the next gather (5.14 -> 5.07-5.08 ms/step, three A/B pairs on one
// box: forward 0.864 -> 0.852 ms, dX-only 0.883 -> 0.868, full 1.134 -> 1.119)
#ifndef MGCN_NT_OUT
#define MGCN_NT_OUT 2
#endif

namespace mgcn {
namespace {

using namespace x6;

constexpr int kXwF = 128;
constexpr int kXwRows = 32;
constexpr int kXwWaves = 8;
constexpr int kXwThreads = 64 * kXwWaves;
constexpr int kXwImg = kXwRows * 256;          // one bf16 term image of a chunk
constexpr int kXwStageLd = kXwF + 8;           // backward staging row: 128 values, the row's
                                               // 4 ReLU mask words, its divisor, padding
constexpr int kXwStage = kXwRows * kXwStageLd * 4;
constexpr int kXfStage = kXwRows * kXwF * 4;   // forward staging tile (unpadded: 2 fit)
constexpr int kXwPerCU = 2;  // resident workgroups per CU the grid is sized for

constexpr int EPI_STORE = 0, EPI_RELU = 1, EPI_RELU_DIV = 2;

// Aggregate one row in the 32-lane group `grp` of the wave (both groups of a
// wave call this together): acc = sum_k X[col_k] * w_k in edge order,
// products and sums rounded separately -- the SpMM's arithmetic, bit for bit.
// Lane gl holds features 4 gl .. 4 gl + 3; edge metadata is loaded 32 edges
// at a time lane-parallel and broadcast by ds_bpermute; U gathers of whole
// 512-B rows are in flight per group before any is folded.
// MAXM (the max adjoint): each edge's dY row counts only at the features
// whose forward winner it was -- the edge's winner word (found through
// slot_map, the fwd slot of each bwd slot; word gl / 8 of its 16-B record,
// bits 4 (gl % 8) + j) is loaded beside the row and selects in the fold.
template <int U, bool MAXM = false>
__device__ __forceinline__ void gather_row(const __amdgpu_buffer_rsrc_t rx, uint32_t ldx_b,
                                           const int64_t *__restrict__ rowptr,
                                           const int32_t *__restrict__ col,
                                           const float *__restrict__ w, int64_t row, bool row_ok,
                                           int gl, int grp, float (&acc)[4], int &deg_out,
                                           const uint32_t *__restrict__ win = nullptr,
                                           const int32_t *__restrict__ slot_map = nullptr) {
  const bool has_w = w != nullptr;
  const int64_t beg = row_ok ? rowptr[row] : 0;
  // a row's degree fits 32 bits; the edge slots are addressed from beg
  const int deg = row_ok ? (int)(rowptr[row + 1] - beg) : 0;
  const int odeg = __shfl_xor(deg, 32, 64);
  const int maxdeg = deg > odeg ? deg : odeg;
  const int32_t *__restrict__ colr = col + beg;
  const float *__restrict__ wr = has_w ? w + beg : nullptr;
  acc[0] = acc[1] = acc[2] = acc[3] = 0.0f;
  for (int e0 = 0; e0 < maxdeg; e0 += 32) {
    const int my = e0 + gl;
    int mc = 0, ms = 0;
    float mw = 1.0f;
    if (my < deg) {
      mc = colr[my];
      if (has_w) mw = wr[my];
      if constexpr (MAXM) ms = slot_map[beg + my];
    }
    const int rem = deg - e0;
    const int nb = rem <= 0 ? 0 : (rem < 32 ? rem : 32);
    const int remw = maxdeg - e0;
    const int nbmax = remw < 32 ? remw : 32;  // wave-uniform
    for (int k0 = 0; k0 < nbmax; k0 += U) {
      float4 xv[U];
      float wk[U];
      bool ok[U];
      uint32_t wbits[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int k = k0 + u;
        const int ck = __shfl(mc, 32 * grp + (k & 31), 64);
        wk[u] = __shfl(mw, 32 * grp + (k & 31), 64);
        ok[u] = k < nb;
        // past-the-row edges get an offset beyond the buffer: no access, zeros
        const uint32_t off = ok[u] ? (uint32_t)ck * ldx_b + 16u * gl : 0xfffffff0u;
        xv[u] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rx, off, 0, 0));
        if constexpr (MAXM) {
          // loaded unconditionally (masked edges read word 0, never used)
          const int sk = __shfl(ms, 32 * grp + (k & 31), 64);
          wbits[u] = win[ok[u] ? (int64_t)sk * 4 + (gl >> 3) : 0];
        }
      }
      // fold in strictly ascending edge order (as the SpMM, bit for bit)
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (ok[u]) {
          if constexpr (MAXM) {
            const uint32_t bits = wbits[u] >> (4 * (gl & 7));
            xv[u].x = (bits & 1u) ? xv[u].x : 0.0f;
            xv[u].y = (bits & 2u) ? xv[u].y : 0.0f;
            xv[u].z = (bits & 4u) ? xv[u].z : 0.0f;
            xv[u].w = (bits & 8u) ? xv[u].w : 0.0f;
          }
          fold4(acc, xv[u], wk[u]);
        }
      }
    }
  }
  deg_out = deg;
}

// Broadcast of lane 32 grp + k (k wave-uniform) to its 32-lane group
// (ds_bpermute; the two-v_readlane form measured slower, exp/ in git history)
__device__ __forceinline__ int bcast_g(int v, int grp, int k) {
  return __shfl(v, 32 * grp + k, 64);
}
__device__ __forceinline__ float bcast_g(float v, int grp, int k) {
  return __int_as_float(bcast_g(__float_as_int(v), grp, k));
}

// Pipelined form for a wave that walks a known sequence of rows: the row
// pointer pair of row k + 2 and the first 32 edge slots (col, w) of row k + 1
// are loaded while row k's feature rows are gathered, so a row costs one
// gather round trip instead of three dependent ones (rowptr -> col -> row).
struct RowMeta {
  int64_t beg;
  int32_t deg;  // a row's degree fits 32 bits (the slots are addressed from beg)
  int mc;
  float mw;
  int ms;  // max adjoint (meta_first_m): fwd slot of the lane's edge
  int mv;  // packed table (meta_first_pk): word offset of the lane's edge's segment values
};

__device__ __forceinline__ void meta_rowptr(const int64_t *__restrict__ rowptr, int64_t row,
                                            bool ok, RowMeta &m) {
  m.beg = ok ? rowptr[row] : 0;
  m.deg = ok ? (int32_t)(rowptr[row + 1] - m.beg) : 0;
}

// meta_rowptr in two parts, for a wave that has gathers in flight when it
// loads the pointers: the subtraction waits for the pair, so it is left to
// meta_deg, behind those gathers' folds (until then deg holds the low word of
// the row's end: a degree fits 32 bits, so the low words' difference is it)
__device__ __forceinline__ void meta_rowptr_raw(const int64_t *__restrict__ rowptr, int64_t row,
                                                bool ok, RowMeta &m) {
  m.beg = ok ? rowptr[row] : 0;
  // (the low word alone: the pair's unused high word would be a register
  // that waits for the load before it can be used again)
  m.deg = ok ? *reinterpret_cast<const int32_t *>(rowptr + row + 1) : 0;
}
__device__ __forceinline__ void meta_deg(RowMeta &m) {
  m.deg = (int32_t)((uint32_t)m.deg - (uint32_t)(uint64_t)m.beg);
}

__device__ __forceinline__ void meta_first(const int32_t *__restrict__ col,
                                           const float *__restrict__ w, int gl, RowMeta &m) {
  m.mc = 0;
  m.mw = 1.0f;
  if (gl < m.deg) {
    m.mc = col[m.beg + gl];
    if (w != nullptr) m.mw = w[m.beg + gl];
  }
}

// meta_first plus the lane's edge's fwd slot (the max adjoint's slot_map)
__device__ __forceinline__ void meta_first_m(const int32_t *__restrict__ col,
                                             const float *__restrict__ w,
                                             const int32_t *__restrict__ slot_map, int gl,
                                             RowMeta &m) {
  meta_first(col, w, gl, m);
  m.ms = gl < m.deg ? slot_map[m.beg + gl] : 0;
}

template <int U>
__device__ __forceinline__ void gather_row_meta(const __amdgpu_buffer_rsrc_t rx, uint32_t ldx_b,
                                                const int32_t *__restrict__ col,
                                                const float *__restrict__ w, const RowMeta &m,
                                                int gl, int grp, float (&acc)[4]) {
  const int64_t beg = m.beg, deg = m.deg;
  const int64_t odeg = __shfl_xor(deg, 32, 64);
  const int64_t maxdeg = deg > odeg ? deg : odeg;
  acc[0] = acc[1] = acc[2] = acc[3] = 0.0f;
  int mc = m.mc;
  float mw = m.mw;
  for (int64_t e0 = 0; e0 < maxdeg; e0 += 32) {
    if (e0 > 0) {  // rows longer than one metadata batch load the rest in place
      const int64_t my = e0 + gl;
      mc = 0;
      mw = 1.0f;
      if (my < deg) {
        mc = col[beg + my];
        if (w != nullptr) mw = w[beg + my];
      }
    }
    const int64_t rem = deg - e0;
    const int nb = rem <= 0 ? 0 : (rem < 32 ? (int)rem : 32);
    const int64_t remw = maxdeg - e0;
    const int nbmax = remw < 32 ? (int)remw : 32;  // wave-uniform
    for (int k0 = 0; k0 < nbmax; k0 += U) {
      float4 xv[U];
      float wk[U];
      bool ok[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int k = k0 + u;
        const int ck = bcast_g(mc, grp, k & 31);
        wk[u] = bcast_g(mw, grp, k & 31);
        ok[u] = k < nb;
        const uint32_t off = ok[u] ? (uint32_t)ck * ldx_b + 16u * gl : 0xfffffff0u;
        xv[u] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rx, off, 0, 0));
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (ok[u]) {
          fold4(acc, xv[u], wk[u]);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// In-place gather from a PACKED table at F = 128 (round 6; pack.hip's layout;
// fused_wide.hip's wide_gather2_pk is the 256-wide form).  The two lane groups
// of a wave walk different rows, so a row's address is per lane: the table is
// read through ONE buffer resource (every segment at a word offset below
// 2^29, the mgcn_spmm_xw_*_packed check), and the metadata loads turn a
// slot's packed col (s << rbits) | i into the word offsets of its row header
// (base[s] + 8 i) and of its segment's values (base[s] + head) -- base[]
// lane-resident, one ds_bpermute per 32 slots, not per slot.  Lane gl reads
// the header pair w = gl / 8 (8 B), then 16 B of values at pos_w +
// popc(mask_w below bit 4 (gl % 8)), expanded by pk_expand: the dense row's
// bits, so the fold is gather_row_meta's, bit for bit.  The headers of batch
// k + 1 (after a row's last batch: the next row's first) load under batch k's
// values, so a row costs the dense gather's round trips.
struct Pk128 {
  __amdgpu_buffer_rsrc_t r;  // the whole table
  uint32_t rbits, head;      // col = (s << rbits) | i; head = seg_rows * 8 words
  uint32_t base;             // lane-resident: base[lane], word offset of segment `lane`
};

// packed col -> (header word offset, value-area word offset); all lanes
// active (ds_bpermute), masked slots carry col 0
__device__ __forceinline__ void pk128_meta(const Pk128 &pk, int c, int &mh, int &mv) {
  const uint32_t s = (uint32_t)c >> pk.rbits;
  const uint32_t i = (uint32_t)c & ((1u << pk.rbits) - 1u);
  const uint32_t b = (uint32_t)__shfl((int)pk.base, (int)(s & 63u), 64);
  mh = (int)(b + 8u * i);
  mv = (int)(b + pk.head);
}

__device__ __forceinline__ void meta_first_pk(const Pk128 &pk, const int32_t *__restrict__ col,
                                              const float *__restrict__ w, int gl, RowMeta &m) {
  meta_first(col, w, gl, m);
  pk128_meta(pk, m.mc, m.mc, m.mv);
}

// the header pairs of slots k0 .. k0 + U - 1 of the group's row (slots past
// n: the "no load" offset, the pair reads 0 and its values are never read)
template <int U>
__device__ __forceinline__ void pk128_headers(const Pk128 &pk, int mh, int grp, int k0, int n,
                                              uint32_t hoff, u32x2 (&h)[U]) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int k = k0 + u;
    const uint32_t hk = (uint32_t)bcast_g(mh, grp, k & 31);
    h[u] = __builtin_amdgcn_raw_buffer_load_b64(pk.r, k < n ? 4u * hk + hoff : 0xfffffff0u, 0, 0);
  }
}

// gather_row_meta from a packed table: hh holds, on entry, the header pairs
// of the row's first U slots and, on return, those of row nx's
template <int U>
__device__ __forceinline__ void gather_row_meta_pk(const Pk128 &pk, const int32_t *__restrict__ col,
                                                   const float *__restrict__ w, const RowMeta &m,
                                                   const RowMeta &nx, int gl, int grp,
                                                   float (&acc)[4], u32x2 (&hh)[U]) {
  const int64_t beg = m.beg, deg = m.deg;
  const int64_t odeg = __shfl_xor(deg, 32, 64);
  const int64_t maxdeg = deg > odeg ? deg : odeg;
  // (two empty rows still run one all-masked batch: the next rows' headers
  // are issued from the one call site below)
  const int64_t maxdeg1 = maxdeg > 0 ? maxdeg : 1;
  acc[0] = acc[1] = acc[2] = acc[3] = 0.0f;
  int mh = m.mc, mv = m.mv;
  float mw = m.mw;
  const uint32_t hoff = 8u * (uint32_t)(gl >> 3);
  const uint32_t sh = 4u * (uint32_t)(gl & 7);  // the lane's nibble in mask_w
  const uint32_t below = (1u << sh) - 1u;
  const int nn = nx.deg < 32 ? nx.deg : 32;
  for (int64_t e0 = 0; e0 < maxdeg1; e0 += 32) {
    const int64_t rem = deg - e0;
    const int nb = rem <= 0 ? 0 : (rem < 32 ? (int)rem : 32);
    const int64_t remw = maxdeg1 - e0;
    const int nbmax = remw < 32 ? (int)remw : 32;  // wave-uniform
    if (e0 > 0) {  // rows longer than one metadata batch load the rest in place
      const int64_t my = e0 + gl;
      int c = 0;
      mw = 1.0f;
      if (my < deg) {
        c = col[beg + my];
        if (w != nullptr) mw = w[beg + my];
      }
      pk128_meta(pk, c, mh, mv);
      pk128_headers<U>(pk, mh, grp, 0, nb, hoff, hh);
    }
    const bool last_window = e0 + 32 >= maxdeg1;
    for (int k0 = 0; k0 < nbmax; k0 += U) {
      u32x4 v[U];
      uint32_t nib[U];
      float wk[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int k = k0 + u;
        wk[u] = bcast_g(mw, grp, k & 31);
        const uint32_t vk = (uint32_t)bcast_g(mv, grp, k & 31);
        nib[u] = (hh[u][0] >> sh) & 0xfu;
        const uint32_t q = hh[u][1] + (uint32_t)__builtin_popcount(hh[u][0] & below);
        // a lane with no nonzero word moves no bytes (offset past the range)
        v[u] = __builtin_amdgcn_raw_buffer_load_b128(pk.r, nib[u] ? 4u * (vk + q) : 0xfffffff0u, 0, 0);
      }
      // the next headers, under these values: this window's next batch, or
      // (the last batch of the last window) row nx's first -- one call site
      const bool more = k0 + U < nbmax;
      if (more || last_window)
        pk128_headers<U>(pk, more ? mh : nx.mc, grp, more ? k0 + U : 0, more ? nb : nn, hoff, hh);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k0 + u < nb) {  // strictly ascending edge order (gather_row_meta)
          const float4 x = pk_expand(nib[u], v[u]);
          fold4(acc, x, wk[u]);
        }
      }
    }
  }
}

// Two rows per lane group at once (the warp-specialised adjoint's gather
// waves): U slots of EACH row in flight per round, so a wave keeps four rows'
// gathers in flight; each row folded in its own edge order, products and
// sums rounded separately (gather_row_meta bit for bit).
template <int U, bool MAXM = false>
__device__ __forceinline__ void gather_row2_meta(const __amdgpu_buffer_rsrc_t rx, uint32_t ldx_b,
                                                 const int32_t *__restrict__ col,
                                                 const float *__restrict__ w, const RowMeta &ma,
                                                 const RowMeta &mb, int gl, int grp,
                                                 float (&aa)[4], float (&ab)[4],
                                                 const uint32_t *__restrict__ win = nullptr,
                                                 const int32_t *__restrict__ slot_map = nullptr) {
#pragma unroll
  for (int j = 0; j < 4; ++j) aa[j] = ab[j] = 0.0f;
  const int64_t da = ma.deg, db = mb.deg;
  int64_t dm = da > db ? da : db;
  const int64_t odm = __shfl_xor(dm, 32, 64);
  dm = dm > odm ? dm : odm;  // wave-uniform loop bound
  int mca = ma.mc, mcb = mb.mc;
  float mwa = ma.mw, mwb = mb.mw;
  int msa = 0, msb = 0;
  if constexpr (MAXM) {
    msa = ma.ms;
    msb = mb.ms;
  }
  for (int64_t e0 = 0; e0 < dm; e0 += 32) {
    if (e0 > 0) {  // rows longer than one metadata batch load the rest in place
      const int64_t my = e0 + gl;
      mca = mcb = 0;
      mwa = mwb = 1.0f;
      if (my < da) {
        mca = col[ma.beg + my];
        if (w != nullptr) mwa = w[ma.beg + my];
        if constexpr (MAXM) msa = slot_map[ma.beg + my];
      }
      if (my < db) {
        mcb = col[mb.beg + my];
        if (w != nullptr) mwb = w[mb.beg + my];
        if constexpr (MAXM) msb = slot_map[mb.beg + my];
      }
    }
    const int64_t ra = da - e0, rb = db - e0;
    const int na = ra <= 0 ? 0 : (ra < 32 ? (int)ra : 32);
    const int nb = rb <= 0 ? 0 : (rb < 32 ? (int)rb : 32);
    const int64_t remw = dm - e0;
    const int nbmax = remw < 32 ? (int)remw : 32;  // wave-uniform
    for (int k0 = 0; k0 < nbmax; k0 += U) {
      float4 xa[U], xb[U];
      float wa[U], wb[U];
      uint32_t ba[U], bb[U];  // MAXM: the edges' winner words (word gl / 8 of the record)
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int k = k0 + u;
        const int ca = bcast_g(mca, grp, k & 31);
        const int cb = bcast_g(mcb, grp, k & 31);
        wa[u] = bcast_g(mwa, grp, k & 31);
        wb[u] = bcast_g(mwb, grp, k & 31);
        const uint32_t oa = k < na ? (uint32_t)ca * ldx_b + 16u * gl : 0xfffffff0u;
        const uint32_t ob = k < nb ? (uint32_t)cb * ldx_b + 16u * gl : 0xfffffff0u;
        xa[u] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rx, oa, 0, 0));
        xb[u] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rx, ob, 0, 0));
        if constexpr (MAXM) {
          // loaded unconditionally (masked edges read word 0, never used)
          const int sa = bcast_g(msa, grp, k & 31);
          const int sb = bcast_g(msb, grp, k & 31);
          ba[u] = win[k < na ? (int64_t)sa * 4 + (gl >> 3) : 0];
          bb[u] = win[k < nb ? (int64_t)sb * 4 + (gl >> 3) : 0];
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if constexpr (MAXM) {  // each edge's dY counts only where it won (gather_row's select)
          const uint32_t qa = ba[u] >> (4 * (gl & 7)), qb = bb[u] >> (4 * (gl & 7));
          xa[u].x = (qa & 1u) ? xa[u].x : 0.0f;
          xa[u].y = (qa & 2u) ? xa[u].y : 0.0f;
          xa[u].z = (qa & 4u) ? xa[u].z : 0.0f;
          xa[u].w = (qa & 8u) ? xa[u].w : 0.0f;
          xb[u].x = (qb & 1u) ? xb[u].x : 0.0f;
          xb[u].y = (qb & 2u) ? xb[u].y : 0.0f;
          xb[u].z = (qb & 4u) ? xb[u].z : 0.0f;
          xb[u].w = (qb & 8u) ? xb[u].w : 0.0f;
        }
        if (k0 + u < na) {
          fold4(aa, xa[u], wa[u]);
        }
        if (k0 + u < nb) {
          fold4(ab, xb[u], wb[u]);
        }
      }
    }
  }
}

// Rolling form of gather_row2_meta (sum / mean; "xw_ws_roll" 2): the same
// slots folded in the same order, but a slot's registers take their next load
// the moment the slot has been folded, and a quad's last round takes the
// first slots of the wave's NEXT quad -- so a wave stands with nothing in
// flight neither between two batches nor under the quad's epilogue (term
// split, `freed` wait, ring stores, signal).
template <int U>
struct RollWin {  // U slots of each of the group's two rows: the rows' 16 B and the edge weights
  float4 xa[U], xb[U];
  float wa[U], wb[U];
};

// register u <- slot k of the rows whose lane-resident (col, w) words are
// (mca, mwa) / (mcb, mwb); slots at or past na / nb: no access
template <int U>
__device__ __forceinline__ void roll_issue(const __amdgpu_buffer_rsrc_t rx, uint32_t ldx_b, int mca,
                                           int mcb, float mwa, float mwb, int na, int nb, int k,
                                           int u, int gl, int grp, RollWin<U> &s) {
  const int ca = bcast_g(mca, grp, k & 31);
  const int cb = bcast_g(mcb, grp, k & 31);
  s.wa[u] = bcast_g(mwa, grp, k & 31);
  s.wb[u] = bcast_g(mwb, grp, k & 31);
  const uint32_t oa = k < na ? (uint32_t)ca * ldx_b + 16u * gl : 0xfffffff0u;
  const uint32_t ob = k < nb ? (uint32_t)cb * ldx_b + 16u * gl : 0xfffffff0u;
  s.xa[u] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rx, oa, 0, 0));
  s.xb[u] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rx, ob, 0, 0));
  // (the loads in slot order, each behind its slot's fold: the folds wait on
  // counted vmcnt, oldest first)
  __builtin_amdgcn_sched_barrier(0);
}

// One round: fold the U slots in flight (row a, then row b, ascending) and
// refill each register at once with slot kn + u of the rows (mc*, mw*).
// The folds carry no mask: a slot past its row's end was loaded with the "no
// access" offset and reads +0, its weight is the 1.0 of a lane without an
// edge, and a sum that started at +0 is never -0, so adding that +0 leaves
// its bits as they are -- the batch form's skipped slot.
template <int U>
__device__ __forceinline__ void roll_round(const __amdgpu_buffer_rsrc_t rx, uint32_t ldx_b, int gl,
                                           int grp, float (&aa)[4], float (&ab)[4], RollWin<U> &s,
                                           int mca, int mcb, float mwa, float mwb, int nna,
                                           int nnb, int kn) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    fold4(aa, s.xa[u], s.wa[u]);
    fold4(ab, s.xb[u], s.wb[u]);
    // the slot's fold ahead of its refill: left free, the folds sink below
    // the round's refills, which then need U more slots of registers (spills)
    asm volatile("" : "+v"(aa[0]), "+v"(aa[1]), "+v"(aa[2]), "+v"(aa[3]), "+v"(ab[0]),
                      "+v"(ab[1]), "+v"(ab[2]), "+v"(ab[3]));
    roll_issue<U>(rx, ldx_b, mca, mcb, mwa, mwb, nna, nnb, kn + u, u, gl, grp, s);
  }
}

// the first U slots of rows ma / mb (their first 32 (col, w) words lane-resident)
template <int U>
__device__ __forceinline__ void roll_first(const __amdgpu_buffer_rsrc_t rx, uint32_t ldx_b,
                                           const RowMeta &ma, const RowMeta &mb, int gl, int grp,
                                           RollWin<U> &s) {
  const int na = ma.deg < 32 ? ma.deg : 32, nb = mb.deg < 32 ? mb.deg : 32;
#pragma unroll
  for (int u = 0; u < U; ++u)
    roll_issue<U>(rx, ldx_b, ma.mc, mb.mc, ma.mw, mb.mw, na, nb, u, u, gl, grp, s);
}

// On entry s holds slots 0 .. U - 1 of rows ma / mb in flight, and on return
// those of rows xa / xb (the wave's next quad; `carry` false, the last quad:
// every slot the "no access" offset, nothing is read).  Two empty rows still
// run one all-masked round, so the carry has one call site.  The rounds that
// refill from the window and the window's last round are separate code, so
// the last one's wait for xa / xb's words stands in a straight line behind
// the loop.  (That wait is counted from the shortest path, a quad of one
// round: vmcnt(2), most of the round in flight.  Two copies of the last round
// -- one behind a refill round, with the full count -- cost 75 spilled
// registers.)  row_a / row_b: the rows (a row longer than one window reads its
// rowptr again: the rows' beg is not held for it); rsc: the rows' row_scale
// ('rw'), loaded ahead of the next quad's slots -- loaded behind them, its
// wait would be theirs too.
template <int U>
__device__ __forceinline__ void gather_row2_roll(const __amdgpu_buffer_rsrc_t rx, uint32_t ldx_b,
                                                 const int64_t *__restrict__ rowptr,
                                                 const int32_t *__restrict__ col,
                                                 const float *__restrict__ w, int64_t row_a,
                                                 int64_t row_b, const RowMeta &ma,
                                                 const RowMeta &mb, const RowMeta &xa,
                                                 const RowMeta &xb, bool carry, int gl, int grp,
                                                 float (&aa)[4], float (&ab)[4], RollWin<U> &s,
                                                 const float *__restrict__ row_scale,
                                                 int64_t n_rows, float (&rsc)[2]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) aa[j] = ab[j] = 0.0f;
  const int32_t da = ma.deg, db = mb.deg;
  int32_t dm = da > db ? da : db;
  const int32_t odm = __shfl_xor(dm, 32, 64);
  // wave-uniform loop bound, in a scalar register: the loops below are then
  // scalar branches, not exec-masked ones with their copies of the window
  dm = __builtin_amdgcn_readfirstlane(dm > odm ? dm : odm);
  if (dm < 1) dm = 1;
  int mca = ma.mc, mcb = mb.mc;
  float mwa = ma.mw, mwb = mb.mw;
  int32_t e0 = 0;
  do {
    const int32_t ra = da - e0, rb = db - e0;
    const int na = ra <= 0 ? 0 : (ra < 32 ? ra : 32);
    const int nb = rb <= 0 ? 0 : (rb < 32 ? rb : 32);
    const int32_t remw = dm - e0;
    const int nbmax = remw < 32 ? remw : 32;  // wave-uniform
    if (e0 > 0) {  // rows longer than one metadata batch load the rest in place
      const int32_t my = e0 + gl;
      mca = mcb = 0;
      mwa = mwb = 1.0f;
      if (my < da) {
        const int64_t beg = rowptr[row_a];
        mca = col[beg + my];
        if (w != nullptr) mwa = w[beg + my];
      }
      if (my < db) {
        const int64_t beg = rowptr[row_b];
        mcb = col[beg + my];
        if (w != nullptr) mwb = w[beg + my];
      }
      // the window's first U slots (the previous window drained at its end).
      // In this block, behind its loads: the wait for the words is then not
      // carried, as a maybe, into the rounds, where it would be vmcnt(0).
#pragma unroll
      for (int u = 0; u < U; ++u) roll_issue<U>(rx, ldx_b, mca, mcb, mwa, mwb, na, nb, u, u, gl, grp, s);
    }
    e0 += 32;
    for (int k0 = U; k0 < nbmax; k0 += U)  // (slots past a row's end: no access)
      roll_round<U>(rx, ldx_b, gl, grp, aa, ab, s, mca, mcb, mwa, mwb, na, nb, k0);
    // the window's last round: the next quad's first slots (nothing at a window boundary)
    const bool to_next = carry && e0 >= dm;
    const int nxa = !to_next ? 0 : xa.deg < 32 ? xa.deg : 32;
    const int nxb = !to_next ? 0 : xb.deg < 32 ? xb.deg : 32;
    if (row_scale != nullptr && e0 >= dm) {
      if (row_a < n_rows) rsc[0] = row_scale[row_a];
      if (row_b < n_rows) rsc[1] = row_scale[row_b];
    }
    roll_round<U>(rx, ldx_b, gl, grp, aa, ab, s, xa.mc, xb.mc, xa.mw, xb.mw, nxa, nxb, 0);
  } while (e0 < dm);
}

// The row sequence of one lane group in the chunk loop: row k is slot
// 16 (k & 1) + 2 wave + grp of the workgroup's chunk k >> 1 (chunks
// blockIdx.x + i gridDim.x).  Used by the forward (-2.5 %) and the dX-only
// backward (-0.5 %); the dW + dX backward has no registers to spare for the
// extra state (its spills cost more).
struct RowSeq {
  int64_t base;  // blockIdx.x * 32 + 2 wave + grp
  int64_t step;  // gridDim.x * 32
  int64_t n_rows;
  __device__ __forceinline__ int64_t row(int64_t k) const { return base + (k >> 1) * step + 16 * (k & 1); }
};

// chunks of this workgroup in a grid-stride chunk loop
__device__ __forceinline__ int64_t my_chunks(int64_t n_chunks) {
  return blockIdx.x < n_chunks ? (n_chunks - 1 - blockIdx.x) / gridDim.x + 1 : 0;
}

#if MGCN_EXPERIMENT
// Experiment builds: when every workgroup of the forward (0) and of the
// warp-specialised adjoint (1) starts and ends (scripts/prof_tail.py: the
// tail a kernel spends waiting for its last workgroups) -- [kernel][workgroup]
// {entry, exit (the latest wave's), chunks}, wall_clock64() ticks; read and
// cleared by mgcn_debug_xw_tail.  Device globals are per file: each of the two
// kernels' files defines its own g_tail[kTailMaxWg][4] (row k of the host
// layout) and hands it out through tail_take.
constexpr int kTailMaxWg = 1024;
#define XTAIL_ENTRY(k)                                           \
  if (threadIdx.x == 0 && blockIdx.x < kTailMaxWg) g_tail[blockIdx.x][0] = wall_clock64();
#define XTAIL_EXIT(k, chunks)                                                      \
  if ((threadIdx.x & 63) == 0 && blockIdx.x < kTailMaxWg) {                        \
    atomicMax(&g_tail[blockIdx.x][1], (unsigned long long)wall_clock64());         \
    if (threadIdx.x == 0) g_tail[blockIdx.x][2] = (unsigned long long)(chunks);    \
  }
// a file's [kTailMaxWg][4] ticks to `host` (nullable), then cleared for the next launch
inline int tail_take(const void *symbol, unsigned long long *host) {
  constexpr size_t bytes = sizeof(unsigned long long) * kTailMaxWg * 4;
  if (host != nullptr) MGCN_HIP_TRY(hipMemcpyFromSymbol(host, symbol, bytes));
  static const unsigned long long zero[kTailMaxWg][4] = {};
  MGCN_HIP_TRY(hipMemcpyToSymbol(symbol, zero, bytes));
  return MGCN_OK;
}
#else
#define XTAIL_ENTRY(k)
#define XTAIL_EXIT(k, chunks)
#endif

// One row's four features -> its three bf16 term images (lane gl of the group)
__device__ __forceinline__ void store_row_terms(char *img_base, int lr, int gl, const float (&v)[4]) {
  uint32_t hi[2], mid[2], lo[2];
  split3_pair(f32x2{v[0], v[1]}, hi[0], mid[0], lo[0]);
  split3_pair(f32x2{v[2], v[3]}, hi[1], mid[1], lo[1]);
  char *img = img_base + img_off(lr, gl >> 1) + 8 * (gl & 1);
  *reinterpret_cast<uint2 *>(img) = make_uint2(hi[0], hi[1]);
  *reinterpret_cast<uint2 *>(img + kXwImg) = make_uint2(mid[0], mid[1]);
  *reinterpret_cast<uint2 *>(img + 2 * kXwImg) = make_uint2(lo[0], lo[1]);
}

// 16x16x32 products of the chunk's 32 rows (A image at `img`) with this
// wave's 16 columns of B (fragments in registers): acc[t] = rows 16 t + 4 g4 + r
__device__ __forceinline__ void mfma_rows(const char *img, const bf16x8 (&b)[3], int ks, int l16,
                                          int g4, f32x4_t (&acc)[2]) {
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int off = img_off(16 * t + l16, 4 * ks + g4);
    const bf16x8 ah = *reinterpret_cast<const bf16x8 *>(img + off);
    const bf16x8 am = *reinterpret_cast<const bf16x8 *>(img + kXwImg + off);
    const bf16x8 al = *reinterpret_cast<const bf16x8 *>(img + 2 * kXwImg + off);
    acc[t] = mfma16_x6(ah, am, al, b[0], b[1], b[2], acc[t]);
  }
}

struct XwArgs {
  int64_t n_rows;
  const int64_t *rowptr;
  const int32_t *col;
  const float *w;     // per-slot weights, nullable
  const float *X;     // gathered rows [n_cols][128]
  int64_t ldx;
  int64_t n_cols;
  const float *W;     // [128][128], Y = Z W
  int64_t ldw;
  const float *bias;  // nullable
  float *Y;
  int64_t ldy;
  uint32_t *relu_mask;  // nullable; [n_rows][4], bit b of word v <=> Y[row][4 b + v] > 0
  float *Z;             // nullable; the aggregated rows before W (and before mean's division)
  int64_t ldz;
  int mean;
  int relu;
  // DYN kernel (launch_xw_dyn): the chunks from dyn_first on are claimed from
  // claim[0] (zeroed before the launch); mail: [grid][2] words
  int32_t dyn_first;
  uint32_t *claim;
  int32_t *mail;
  // packed table (PK kernels; mgcn_spmm_xw_fwd_packed): X unused
  const uint32_t *pk;
  uint32_t pk_bytes, pk_rbits, pk_head;
  uint32_t pk_base[64];
};

struct XbArgs {
  int64_t n_rows;  // source nodes: rows of the bwd view, of X and of dX
  const int64_t *rowptr;
  const int32_t *col;
  const float *w;
  const float *row_scale;  // nullable ('rw')
  const float *dY;         // gathered rows [n_cols][128]
  int64_t lddy;
  int64_t n_cols;
  const float *X;  // layer input [n_rows][128]
  int64_t ldx;
  const float *W;  // [128][128], H = X W
  int64_t ldw;
  float *dX;  // nullable
  int64_t lddx;
  const uint32_t *relu_mask;  // lower layer's output > 0 (mgcn_spmm_fwd layout)
  const float *row_div;
  float *dw_partial;      // [grid][128][128]
  float *colsum_partial;  // [grid][128]
  const uint32_t *win_mask;  // max adjoint: winner bits per fwd slot ([nnz][4])
  const int32_t *slot_map;   // max adjoint: fwd slot of every bwd slot
  // packed dY (dX-only PK kernel; mgcn_spmm_xw_bwd_packed): dY unused
  const uint32_t *pk;
  uint32_t pk_bytes, pk_rbits, pk_head;
  uint32_t pk_base[64];
};

// the two warp-specialised kernels (fused_dws.hip, fused_fwd_ws.hip): 8 gather
// and 8 MFMA waves, ring buffers of a chunk's three bf16 term images
constexpr int kBsImgSet = 3 * kXwImg;          // dH's three term images: 24 KB
constexpr int kBsNG = 8, kBsNM = 8;
constexpr int kBsThreads = 64 * (kBsNG + kBsNM);

inline int xw_grid() { return kXwPerCU * device_cus(); }  // the two-phase kernels' grid

}  // namespace

// Each kernel file's launch functions, called by fused.hip.  XwArgs / XbArgs
// are part of the kernels' mangled names and so stay in the unnamed
// namespace: they have no linkage, and a function that names them cannot be
// called from another file.  `xw` / `xb` point to the caller's XwArgs / XbArgs.

// fused_fwd.hip: the two-phase forward at "spmm_xw_unroll" (packed: the
// packed-table forward at "xw_pk_unroll")
int launch_xw_fwd(const void *xw, bool packed, hipStream_t s);
size_t xw_dyn_workspace_bytes();
// The dynamic-claim forward where it applies: the default unroll, a
// workspace, and static rounds left (>= 8, the kernel needs 3) before the
// claimed ones; returns false (nothing launched) otherwise.
bool launch_xw_dyn(const void *xw, void *workspace, size_t workspace_bytes, hipStream_t s, int *rc);
// fused_fwd_ws.hip: the warp-specialised forward where it applies; returns
// false (nothing launched) otherwise
bool launch_xw_ws(const void *xw, void *workspace, size_t workspace_bytes, hipStream_t s, int *rc);
// fused_bwd.hip: the two-phase adjoint, dW (+ dX) or (dx_only) dX alone from
// a dense or packed dY
int launch_xb_bwd(const void *xb, int epi, int grid, bool dx_only, bool packed, hipStream_t s);
// fused_dws.hip: the warp-specialised adjoint (hcs_partial: nullable)
int launch_dws(const void *xb, int epi, int grid, float *hcs_partial, hipStream_t s);
#if MGCN_EXPERIMENT
int xw_fwd_tail_take(unsigned long long *host);  // fused_fwd.hip: [kTailMaxWg][4]
int dws_tail_take(unsigned long long *host);     // fused_dws.hip
#endif

}  // namespace mgcn
