// Argument blocks and device helpers shared by the gate launches: the
// wave-per-row kernels (edge_gate.hip) and the workgroup path of heavy rows
// (edge_gate_heavy.hip).  Internal header.
//
// Feature rows (Hx, Y, dY, dHx) have the element type R of the argument
// struct: float, or bf16 bit patterns as uint16_t (the mgcn_gate_*_bf16
// entries), read and written through attention.h's row_ld / row_st: a bf16
// element is widened exactly at its load, every value is formed by the fp32
// kernel's operations in its order, and a bf16 output element is rounded once,
// to nearest even, at its store.  With R = float the kernels are the fp32 ones
// instruction for instruction.  a, c, t, w, g, dl, dc, da, dw, bias, w_sd and
// coef are fp32 with either R.
#pragma once

#include "mgcn_internal.h"

namespace mgcn {

// Row schedule of a view (mgcn_row_schedule): order[0, n_heavy) are the heavy
// rows, the first n_giant of them giant; order[n_heavy, n_rows) the rows the
// wave kernels keep.  order == NULL: every row on the wave kernels.
struct GateSched {
  const int32_t *order;
  int64_t n_heavy, n_giant;
  float *coef;  // caller's scratch [nnz]: g w per slot of the view walked
};

template <class R>
struct GateFwdArgsT {
  using Row = R;
  int64_t n_rows;
  int C, reduce, relu, t_bcast;
  const int64_t *rowptr;
  const int32_t *col, *eid;
  const float *a, *c, *t, *w;
  const R *Hx;
  int64_t ldh;
  const float *bias;
  R *Y;
  int64_t ldy;
  float *g;
  int32_t *argmax;
  GateSched s;
};
using GateFwdArgs = GateFwdArgsT<float>;
using GateFwdArgsBf16 = GateFwdArgsT<uint16_t>;

// kCnt: the struct carries `cnt` (mean over bf16 rows: a bf16 dY cannot hold
// the divided row without a second rounding, so every loaded dY element is
// divided by its destination's count in fp32, as mgcn_spmm_bwd_bf16 does)
template <class R>
struct GateBwdDstArgsT {
  using Row = R;
  int64_t n_rows;
  int C;
  const int64_t *rowptr;
  const int32_t *col;
  const R *Hx;
  int64_t ldh;
  const R *dY;
  int64_t lddy;
  const float *w, *g, *dg_in;
  const uint32_t *win;
  float *dl, *dc, *dw;
  GateSched s;
  static constexpr bool kCnt = false;
};
using GateBwdDstArgs = GateBwdDstArgsT<float>;
struct GateBwdDstArgsBf16 : GateBwdDstArgsT<uint16_t> {
  const float *cnt;  // nullable, by destination node: the row's own count
  static constexpr bool kCnt = true;
};

template <class R>
struct GateBwdSrcArgsT {
  using Row = R;
  int64_t n_rows;
  int C;
  const int64_t *rowptr;
  const int32_t *col, *slot;
  const R *dY;
  int64_t lddy;
  const float *w_t, *row_scale, *g, *dl;
  const uint32_t *win;
  const float *wsd, *dc;
  float *da;
  R *dHx;
  int64_t lddh;
  GateSched s;
  static constexpr bool kCnt = false;
};
using GateBwdSrcArgs = GateBwdSrcArgsT<float>;
struct GateBwdSrcArgsBf16 : GateBwdSrcArgsT<uint16_t> {
  const float *cnt;  // nullable, by destination node: the gathered column's count
  static constexpr bool kCnt = true;
};

__device__ inline float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = __fadd_rn(v, __shfl_xor(v, off, 64));
  return v;
}

__device__ inline float gate_sigmoid(float l) {
  return __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-l)));
}

// bit f of a slot's winner words (mgcn_max_mask layout: [nnz, ceil(C / 32)])
__device__ inline bool won(const uint32_t *win, int64_t slot, int W, int f) {
  return (win[slot * W + (f >> 5)] >> (f & 31)) & 1u;
}

// The heavy rows of each launch (edge_gate_heavy.hip), on `stream`; a.s.order
// set and a.s.n_heavy > 0.  Every output element has the bits the wave kernel
// gives it.
int gate_fwd_heavy(const GateFwdArgs &a, hipStream_t stream);
int gate_bwd_dst_heavy(const GateBwdDstArgs &a, hipStream_t stream);
int gate_bwd_src_heavy(const GateBwdSrcArgs &a, hipStream_t stream);
int gate_fwd_heavy(const GateFwdArgsBf16 &a, hipStream_t stream);
int gate_bwd_dst_heavy(const GateBwdDstArgsBf16 &a, hipStream_t stream);
int gate_bwd_src_heavy(const GateBwdSrcArgsBf16 &a, hipStream_t stream);

}  // namespace mgcn
