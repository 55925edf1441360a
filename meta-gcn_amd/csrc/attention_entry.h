// Host side of the attention entries that walk a view: one checked body per
// operation -- forward / edge softmax, adjoint by destination, adjoint by
// source -- for soft and hard attention, fp32 and bf16 rows, with and without
// a row schedule.  An entry fills its argument struct (attention.h) and calls
// fwd / bwd_dst / bwd_src; a _sched entry (attention_heavy.hip) calls the
// operation's check with its schedule, launches the heavy rows itself, and
// hands the schedule's rest to the wave launch over SchedArgsT<A>.
//
// Templates, not functions of one translation unit: the argument structs live
// in an anonymous namespace, so each including file instantiates the kernels
// of its own entries, as it always did.
#pragma once

#include "attention.h"

namespace mgcn {
namespace {

// The schedule of a _sched entry: rows order[0, n_giant) and
// order[n_giant, n_heavy) by workgroups, order[n_heavy, n_rows) by waves;
// coef: the [nnz, H] scratch of the entries that gather.
struct HeavyRows {
  const int32_t *order;
  int64_t n_heavy, n_giant;
  float *coef;
};

// What a check returns besides MGCN_OK (launch) and MGCN_EINVAL: nothing to
// do, the entry returns MGCN_OK.
constexpr int kAttNoop = -1;
#define ATT_CHECKED(check)                                         \
  do {                                                             \
    if (int rc_ = (check)) return rc_ == kAttNoop ? MGCN_OK : rc_; \
  } while (0)

// shape, act, temperature (hard), the schedule if any -- in that order, and
// all before the n_rows == 0 return
template <class A>
int check_head(const char *fn, const A &k, int64_t nnz, const HeavyRows *s) {
  clear_error();
  ATT_REQUIRE_SHAPE(fn, k.n_rows, nnz, k.H, k.C);
  ATT_ACT_OK(fn, k.act);
  if constexpr (A::kHard)
    MGCN_REQUIRE(k.temperature > 0.0f, "%s: need temperature > 0 (got %g)", fn,
                 (double)k.temperature);
  if (s != nullptr)
    MGCN_REQUIRE(0 <= s->n_giant && s->n_giant <= s->n_heavy && s->n_heavy <= k.n_rows,
                 "%s: need 0 <= n_giant <= n_heavy <= n_rows", fn);
  return k.n_rows == 0 ? kAttNoop : MGCN_OK;
}

// rows the wave kernel walks: all of them, or the schedule's rest
template <class W>
int64_t wave_rows(const W &w) {
  if constexpr (W::kSched)
    return w.n_rows - w.n_heavy;
  else
    return w.n_rows;
}

// ----------------------------------------------------------------- forward
// A: FwdArgsT<R> or HardFwdArgsT<R>.  GATHER: Y rows as well; else alpha only
// (the edge softmax, C = 1).
template <bool GATHER, class A>
int fwd_check(const char *fn, const A &k, int64_t nnz, const HeavyRows *s = nullptr) {
  if (int rc = check_head(fn, k, nnz, s)) return rc;
  if constexpr (GATHER) {
    MGCN_REQUIRE(k.rowptr && k.Hp && k.Y, "%s: null array", fn);
    MGCN_REQUIRE(nnz == 0 || k.col, "%s: null col", fn);
    MGCN_REQUIRE(k.alpha_in != nullptr || (k.s_row && k.s_col && (k.alpha || nnz == 0)),
                 "%s: need alpha_in, or s_row / s_col / alpha", fn);
    MGCN_REQUIRE(k.ldh >= (int64_t)k.H * k.C && k.ldy >= (int64_t)k.H * k.C,
                 "%s: leading dimension too small", fn);
    if (s) MGCN_REQUIRE(nnz == 0 || s->coef, "%s: a schedule needs the coef scratch [nnz, H]", fn);
  } else {
    if (nnz == 0) return kAttNoop;
    MGCN_REQUIRE(k.rowptr && k.col && k.s_row && k.s_col && k.alpha, "%s: null array", fn);
  }
  return MGCN_OK;
}

// W: A, or SchedArgsT<A>
template <bool GATHER, class W>
int fwd_waves(const W &w, const char *label, hipStream_t st) {
  const int64_t n_work = wave_rows(w);
  if (n_work == 0) return MGCN_OK;
  if constexpr (GATHER) {
#define CALL(FPL)                                                                  \
  hipLaunchKernelGGL((att_fwd_kernel<FPL, true, W>), dim3(att_grid(n_work)),      \
                     dim3(kAttThreads), 0, st, w)
    ATT_DISPATCH(w.H * w.C, CALL);
#undef CALL
  } else {
    hipLaunchKernelGGL((att_fwd_kernel<1, false, W>), dim3(att_grid(n_work)), dim3(kAttThreads), 0,
                       st, w);
  }
  return check_launch(label);
}

template <bool GATHER, class A>
int fwd(const char *fn, const A &k, int64_t nnz, const char *label, void *stream) {
  ATT_CHECKED((fwd_check<GATHER>(fn, k, nnz)));
  return fwd_waves<GATHER>(k, label, as_stream(stream));
}

// ------------------------------------------------- adjoint, by destination
// A: BwdDstArgsT<R> or HardBwdDstArgsT<R>
template <class A>
int bwd_dst_check(const char *fn, const A &k, int64_t nnz, const HeavyRows *s = nullptr) {
  if (int rc = check_head(fn, k, nnz, s)) return rc;
  MGCN_REQUIRE(k.rowptr && k.Hp && k.dY, "%s: null array", fn);
  MGCN_REQUIRE(nnz == 0 || (k.col && k.dz), "%s: null col / dz", fn);
  MGCN_REQUIRE(!k.softmax || (k.ds_row && k.s_row && k.s_col && (k.alpha || nnz == 0)),
               "%s: the softmax adjoint needs alpha, s_row, s_col, ds_row", fn);
  MGCN_REQUIRE(k.ldh >= (int64_t)k.H * k.C && k.lddy >= (int64_t)k.H * k.C,
               "%s: leading dimension too small", fn);
  return MGCN_OK;
}

template <class W>
int bwd_dst_waves(const W &w, const char *label, hipStream_t st) {
  const int64_t n_work = wave_rows(w);
  if (n_work == 0) return MGCN_OK;
#define CALL(FPL)                                                                             \
  hipLaunchKernelGGL((att_bwd_dst_kernel<FPL, W>), dim3(att_grid(n_work)), dim3(kAttThreads), \
                     0, st, w)
  ATT_DISPATCH(w.H * w.C, CALL);
#undef CALL
  return check_launch(label);
}

template <class A>
int bwd_dst(const char *fn, const A &k, int64_t nnz, const char *label, void *stream) {
  ATT_CHECKED(bwd_dst_check(fn, k, nnz));
  return bwd_dst_waves(k, label, as_stream(stream));
}

// ------------------------------------------------------ adjoint, by source
// A: BwdSrcArgs, BwdSrcArgsBf16 or HardBwdSrcArgsT of either.  A parked row
// (kPark, dHp_f32 given) needs no dHp.
template <class A>
int bwd_src_check(const char *fn, const A &k, int64_t nnz, const HeavyRows *s = nullptr) {
  if (int rc = check_head(fn, k, nnz, s)) return rc;
  MGCN_REQUIRE(k.rowptr && k.dY && k.a && k.ds_src, "%s: null array", fn);
  MGCN_REQUIRE(nnz == 0 || (k.col && k.slot && k.alpha && k.dz),
               "%s: null col / slot_map / alpha / dz", fn);
  MGCN_REQUIRE(!k.softmax || (k.s_row && k.s_col), "%s: the softmax adjoint needs s_row, s_col",
               fn);
  bool parked = false;
  if constexpr (A::kPark) parked = k.dHp_f32 != nullptr;
  MGCN_REQUIRE(parked || k.dHp, "%s: null dHp", fn);
  MGCN_REQUIRE(k.lddy >= (int64_t)k.H * k.C && (parked || k.lddh >= (int64_t)k.H * k.C),
               "%s: leading dimension too small", fn);
  if (s) MGCN_REQUIRE(nnz == 0 || s->coef, "%s: a schedule needs the coef scratch [nnz, H]", fn);
  return MGCN_OK;
}

template <class W>
int bwd_src_waves(const W &w, const char *label, hipStream_t st) {
  const int64_t n_work = wave_rows(w);
  if (n_work == 0) return MGCN_OK;
#define CALL(FPL)                                                                             \
  hipLaunchKernelGGL((att_bwd_src_kernel<FPL, W>), dim3(att_grid(n_work)), dim3(kAttThreads), \
                     0, st, w)
  ATT_DISPATCH(w.H * w.C, CALL);
#undef CALL
  return check_launch(label);
}

template <class A>
int bwd_src(const char *fn, const A &k, int64_t nnz, const char *label, void *stream) {
  ATT_CHECKED(bwd_src_check(fn, k, nnz));
  return bwd_src_waves(k, label, as_stream(stream));
}

}  // namespace
}  // namespace mgcn
