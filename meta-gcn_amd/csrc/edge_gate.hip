// Edge-gated message passing (gfx950): NodeModelAdditive with an EdgeGateProj /
// EdgeGateFree gate (src/gcn_meta/models/gcn_base_models.py:229-232, 322-396)
// after its x @ weight_node, and the adjoint.
//
// With Hx = X W [N, C] and edge k: j -> i,
//   l_k = a[j] + c[i] + t_k      a = Hx w_src, c = Hx w_dst (mgcn_att_scores, H = 1)
//   g_k = sigmoid(l_k)           t: per-slot term (edge features, free gates) or one scalar
//   Y[i] = reduce_{k -> i} g_k w_k Hx[j]  (+ bias, ReLU)      reduce: sum / mean / max
// The reference materialises x_j, x_i, the gate [E, 1] and the gated messages
// [E, C]; here the logit needs two N-length score vectors, so the per-edge
// state is the gate g [nnz] and, going back, its logit gradient dl [nnz].
//
// Work split: that of the attention kernels (attention.h) with one head.  Four
// waves per workgroup, one wave per CSR row, grid-stride over rows, a row of
// any degree walked in chunks of 64 slots.  Edge phase: lane u stands for slot
// k0 + u, so g / w / t / dl are read and written coalesced.  Feature phase:
// lane l holds features f = l + 64 i (i < FPL); the coefficient of a slot
// comes from the lane that formed it (ds_bpermute).  No LDS, no barrier, no
// atomics; slots keep COO order and every sum has a fixed order (per-slot dot
// products: the lane's own products in i order, then the xor butterfly), so
// results are bitwise repeatable.  With a row schedule (the mgcn_gate_*_sched
// entries) the rows over 128 edges go to workgroups instead
// (edge_gate_heavy.hip), with the same bits; these kernels then walk the
// schedule's remaining rows.
//
// Roofline (forward): 8 (N + 1) rowptr + nnz (4 col + 4 C row + 4 a + 4 g
// [+ 4 w] [+ 4 t]) + 4 N C (Y) + 4 N (c) bytes.
//
// The kernels are templated on their argument struct (edge_gate.h): with bf16
// rows (the mgcn_gate_*_bf16 entries) Hx / Y / dY / dHx elements take 2 bytes,
// are widened exactly at the load and rounded once at the store, and every
// operation between is the fp32 kernel's.  The lane layout is the same (lane l
// <-> features l + 64 i: the per-slot dot product of the adjoint by
// destination sums in a lane-dependent order).  Mean: the two bf16 adjoint
// kernels divide each loaded dY element by its destination's count (cnt)
// where the fp32 route reads rows divided beforehand.

#include "attention.h"
#include "edge_gate.h"

namespace mgcn {
namespace {

// ----------------------------------------------------------------- forward
// SCHED: the rows order[n_heavy, n_rows) of the schedule (the heavy rows are
// edge_gate_heavy.hip's); else rows 0 .. n_rows
template <int FPL, bool MAX, bool SCHED = false, class A = GateFwdArgs>
__global__ __launch_bounds__(kAttThreads) void gate_fwd_kernel(A a) {
  constexpr int U = gather_unroll<FPL>();
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = blockIdx.x * (int64_t)kAttWaves + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kAttWaves;
  const int C = a.C;
  const float tb = (a.t != nullptr && a.t_bcast) ? a.t[0] : 0.0f;
  const int64_t n_work = SCHED ? a.n_rows - a.s.n_heavy : a.n_rows;
  for (int64_t ri = wave0; ri < n_work; ri += nwaves) {
    const int64_t row = SCHED ? (int64_t)a.s.order[a.s.n_heavy + ri] : ri;
    const int64_t beg = a.rowptr[row], end = a.rowptr[row + 1];
    const float cr = a.c != nullptr ? a.c[row] : 0.0f;
    float acc[FPL];
    int32_t arg[FPL];  // max: the winning slot
#pragma unroll
    for (int i = 0; i < FPL; ++i) {
      acc[i] = MAX ? MGCN_MAX_FILL : 0.0f;
      arg[i] = -1;
    }
    for (int64_t k0 = beg; k0 < end; k0 += 64) {
      const int64_t k = k0 + lane;
      float coef = 0.0f;  // g w of this lane's slot
      if (k < end) {
        float l = cr;
        if (a.a != nullptr) l = __fadd_rn(a.a[a.col[k]], l);
        if (a.t != nullptr) l = __fadd_rn(l, a.t_bcast ? tb : a.t[k]);
        const float g = gate_sigmoid(l);
        a.g[k] = g;
        coef = a.w != nullptr ? __fmul_rn(g, a.w[k]) : g;
      }
      const int ns = (int)(end - k0 < 64 ? end - k0 : 64);
      for (int kk = 0; kk < ns; kk += U) {
        float hp[U][FPL];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const bool on = kk + u < ns;
          const int64_t c = on ? __builtin_amdgcn_readfirstlane(a.col[k0 + kk + u]) : 0;
#pragma unroll
          for (int i = 0; i < FPL; ++i) {
            const int f = lane + 64 * i;
            hp[u][i] = row_ld(on && f < C, a.Hx, c * a.ldh + f);
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (kk + u < ns) {
            const float w = __shfl(coef, kk + u, 64);
#pragma unroll
            for (int i = 0; i < FPL; ++i) {
              const float p = __fmul_rn(w, hp[u][i]);
              if constexpr (MAX) {
                if (p >= acc[i]) {  // torch_scatter 1.x CPU: `>=`, the later edge wins ties
                  acc[i] = p;
                  arg[i] = (int32_t)(k0 + kk + u);
                }
              } else {
                acc[i] = __fadd_rn(acc[i], p);
              }
            }
          }
        }
      }
    }
    const float cnt = (float)(end - beg > 1 ? end - beg : 1);
#pragma unroll
    for (int i = 0; i < FPL; ++i) {
      const int f = lane + 64 * i;
      if (f < C) {
        float y = acc[i];
        if constexpr (MAX) {
          if (y == MGCN_MAX_FILL) {  // common.py:63-64: an empty row gives 0
            y = 0.0f;
            arg[i] = -1;
          }
          a.argmax[row * C + f] = arg[i] >= 0 ? a.eid[arg[i]] : -1;
        } else {
          if (a.reduce == MGCN_REDUCE_MEAN) y = __fdiv_rn(y, cnt);
        }
        if (a.bias != nullptr) y = __fadd_rn(y, a.bias[f]);
        if (a.relu) y = y < 0.0f ? 0.0f : y;
        row_st(a.Y + row * a.ldy + f, y);
      }
    }
  }
}

// ------------------------------------------------- adjoint, by destination
template <int FPL, bool MAX, bool SCHED = false, class A = GateBwdDstArgs>
__global__ __launch_bounds__(kAttThreads) void gate_bwd_dst_kernel(A a) {
  constexpr int U = gather_unroll<FPL>();
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = blockIdx.x * (int64_t)kAttWaves + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kAttWaves;
  const int C = a.C, W = (a.C + 31) >> 5;
  const int64_t n_work = SCHED ? a.n_rows - a.s.n_heavy : a.n_rows;
  for (int64_t ri = wave0; ri < n_work; ri += nwaves) {
    const int64_t row = SCHED ? (int64_t)a.s.order[a.s.n_heavy + ri] : ri;
    float dy[FPL];
#pragma unroll
    for (int i = 0; i < FPL; ++i) {
      const int f = lane + 64 * i;
      dy[i] = row_ld(f < C, a.dY, row * a.lddy + f);
    }
    if constexpr (A::kCnt) {  // mean over bf16 rows: the fp32 path's divided row
      if (a.cnt != nullptr) {
        const float cn = a.cnt[row];
#pragma unroll
        for (int i = 0; i < FPL; ++i) dy[i] = __fdiv_rn(dy[i], cn);
      }
    }
    const int64_t beg = a.rowptr[row], end = a.rowptr[row + 1];
    float part = 0.0f;  // this lane's share of sum_row dl
    for (int64_t k0 = beg; k0 < end; k0 += 64) {
      const int ns = (int)(end - k0 < 64 ? end - k0 : 64);
      float dot = 0.0f;  // lane u: sum_f dY[row, f] Hx[col, f] of slot k0 + u
      for (int kk = 0; kk < ns; kk += U) {
        float hp[U][FPL];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const bool on = kk + u < ns;
          const int64_t c = on ? __builtin_amdgcn_readfirstlane(a.col[k0 + kk + u]) : 0;
#pragma unroll
          for (int i = 0; i < FPL; ++i) {
            const int f = lane + 64 * i;
            bool ld = on && f < C;
            if constexpr (MAX) ld = ld && won(a.win, k0 + kk + u, W, f);
            hp[u][i] = row_ld(ld, a.Hx, c * a.ldh + f);
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (kk + u < ns) {
            float p = 0.0f;
#pragma unroll
            for (int i = 0; i < FPL; ++i) p = __fadd_rn(p, __fmul_rn(dy[i], hp[u][i]));
            p = wave_sum(p);
            if (lane == kk + u) dot = p;
          }
        }
      }
      const int64_t k = k0 + lane;
      if (k < end) {
        const float g = a.g[k];
        if (a.dw != nullptr) a.dw[k] = __fmul_rn(dot, g);
        float dg = a.w != nullptr ? __fmul_rn(dot, a.w[k]) : dot;
        if (a.dg_in != nullptr) dg = __fadd_rn(dg, a.dg_in[k]);
        const float v = __fmul_rn(dg, __fmul_rn(g, __fsub_rn(1.0f, g)));
        a.dl[k] = v;
        part = __fadd_rn(part, v);
      }
    }
    if (a.dc != nullptr) {
      const float tot = wave_sum(part);
      if (lane == 0) a.dc[row] = tot;
    }
  }
}

// ------------------------------------------------------ adjoint, by source
// MEAN (bf16 rows with cnt; never with MAX): every gathered dY element divided
// by its column's count.  A template parameter, not a test of a.cnt: a branch
// between the gathers of a batch keeps the compiler from issuing the batch's
// column loads together (the sum at C = 32 on the config-2 graph: 1.56 ms with
// the test, 1.15 ms without; DESIGN.md §4, "Edge gates", "bf16 rows").
template <int FPL, bool MAX, bool SCHED = false, class A = GateBwdSrcArgs, bool MEAN = false>
__global__ __launch_bounds__(kAttThreads) void gate_bwd_src_kernel(A a) {
  constexpr int U = gather_unroll<FPL>();
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = blockIdx.x * (int64_t)kAttWaves + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kAttWaves;
  const int C = a.C, W = (a.C + 31) >> 5;
  const int64_t n_work = SCHED ? a.n_rows - a.s.n_heavy : a.n_rows;
  for (int64_t ri = wave0; ri < n_work; ri += nwaves) {
    const int64_t row = SCHED ? (int64_t)a.s.order[a.s.n_heavy + ri] : ri;
    const int64_t beg = a.rowptr[row], end = a.rowptr[row + 1];
    float acc[FPL];
#pragma unroll
    for (int i = 0; i < FPL; ++i) acc[i] = 0.0f;
    float part = 0.0f;  // this lane's share of sum_row dl
    for (int64_t k0 = beg; k0 < end; k0 += 64) {
      const int64_t k = k0 + lane;
      int32_t fs = 0;     // the fwd slot of this lane's slot
      float coef = 0.0f;  // its g w
      if (k < end) {
        fs = a.slot[k];
        const float g = a.g[fs];
        coef = a.w_t != nullptr ? __fmul_rn(g, a.w_t[k]) : g;
        if (a.da != nullptr) part = __fadd_rn(part, a.dl[fs]);
      }
      const int ns = (int)(end - k0 < 64 ? end - k0 : 64);
      for (int kk = 0; kk < ns; kk += U) {
        float dy[U][FPL];
        [[maybe_unused]] float cn[U];  // MEAN: the gathered columns' counts
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const bool on = kk + u < ns;
          const int64_t c = on ? __builtin_amdgcn_readfirstlane(a.col[k0 + kk + u]) : 0;
          int64_t fsu = 0;
          if constexpr (MAX) fsu = on ? __shfl(fs, kk + u, 64) : 0;
#pragma unroll
          for (int i = 0; i < FPL; ++i) {
            const int f = lane + 64 * i;
            bool ld = on && f < C;
            if constexpr (MAX) ld = ld && won(a.win, fsu, W, f);
            dy[u][i] = row_ld(ld, a.dY, c * a.lddy + f);
          }
          if constexpr (MEAN) cn[u] = a.cnt[c];  // (!on: c = 0, a valid column)
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (kk + u < ns) {
            const float w = __shfl(coef, kk + u, 64);
            if constexpr (MEAN) {  // the fp32 route's divided row, formed where it is used
#pragma unroll
              for (int i = 0; i < FPL; ++i) dy[u][i] = __fdiv_rn(dy[u][i], cn[u]);
            }
#pragma unroll
            for (int i = 0; i < FPL; ++i) acc[i] = __fadd_rn(acc[i], __fmul_rn(w, dy[u][i]));
          }
        }
      }
    }
    float dav = 0.0f;
    if (a.da != nullptr) {
      dav = wave_sum(part);
      if (lane == 0) a.da[row] = dav;
    }
    const float dcv = a.dc != nullptr ? a.dc[row] : 0.0f;
    const float rs = a.row_scale != nullptr ? a.row_scale[row] : 1.0f;
#pragma unroll
    for (int i = 0; i < FPL; ++i) {
      const int f = lane + 64 * i;
      if (f < C) {
        float v = acc[i];
        if (a.row_scale != nullptr) v = __fmul_rn(v, rs);
        if (a.wsd != nullptr) {
          if (a.da != nullptr) v = __fadd_rn(v, __fmul_rn(dav, a.wsd[f]));
          if (a.dc != nullptr) v = __fadd_rn(v, __fmul_rn(dcv, a.wsd[C + f]));
        }
        row_st(a.dHx + row * a.lddh + f, v);
      }
    }
  }
}

}  // namespace
}  // namespace mgcn

using namespace mgcn;

#define GATE_REQUIRE_SHAPE(fn, n_rows, nnz, C)                                                 \
  do {                                                                                         \
    MGCN_REQUIRE((n_rows) >= 0 && (nnz) >= 0, "%s: negative size", fn);                        \
    MGCN_REQUIRE((C) >= 1 && (C) <= 1024, "%s: need 1 <= C <= 1024 (C = %d)", fn, (int)(C));   \
    MGCN_REQUIRE((int64_t)(nnz) < ((int64_t)1 << 31), "%s: need nnz < 2^31", fn);              \
  } while (0)

// the schedule of a _sched entry (order == NULL: none, the counts are not read)
#define GATE_REQUIRE_SCHED(fn, s, n_rows)                                                      \
  MGCN_REQUIRE((s).order == nullptr ||                                                         \
                   (0 <= (s).n_giant && (s).n_giant <= (s).n_heavy && (s).n_heavy <= (n_rows)), \
               "%s: need 0 <= n_giant <= n_heavy <= n_rows", fn)

// one wave kernel (argument struct A: fp32 or bf16 rows) over rows 0 .. n_rows
// (sched false) or over the schedule's rows past the heavy ones
#define GATE_LAUNCH(KERNEL, FPL, A, is_max, sched, n_work, st, k)                              \
  do {                                                                                         \
    const dim3 grid_(att_grid(n_work)), block_(kAttThreads);                                   \
    if ((is_max) && (sched))                                                                   \
      hipLaunchKernelGGL((KERNEL<FPL, true, true, A>), grid_, block_, 0, st, k);               \
    else if (is_max)                                                                           \
      hipLaunchKernelGGL((KERNEL<FPL, true, false, A>), grid_, block_, 0, st, k);              \
    else if (sched)                                                                            \
      hipLaunchKernelGGL((KERNEL<FPL, false, true, A>), grid_, block_, 0, st, k);              \
    else                                                                                       \
      hipLaunchKernelGGL((KERNEL<FPL, false, false, A>), grid_, block_, 0, st, k);             \
  } while (0)

// The body of mgcn_gate_fwd (s.order == NULL: its launch, nothing else) and of
// mgcn_gate_fwd_sched: the heavy rows by workgroups, then the wave kernel over
// the rest.  R: the row type of the entry (float, or uint16_t for _bf16).
template <class R>
static int gate_fwd_run(const char *fn, int64_t n_rows, int64_t nnz, int32_t C,
                        const int64_t *rowptr, const int32_t *col, const int32_t *eid,
                        const float *a, const float *c, const float *t, int t_bcast,
                        const float *w, const R *Hx, int64_t ldh, int reduce, const float *bias,
                        int relu, R *Y, int64_t ldy, float *g, int32_t *argmax, GateSched s,
                        void *stream) {
  using A = GateFwdArgsT<R>;
  clear_error();
  GATE_REQUIRE_SHAPE(fn, n_rows, nnz, C);
  MGCN_REQUIRE(reduce == MGCN_REDUCE_SUM || reduce == MGCN_REDUCE_MEAN ||
                   reduce == MGCN_REDUCE_MAX, "%s: bad reduce %d", fn, reduce);
  GATE_REQUIRE_SCHED(fn, s, n_rows);
  if (n_rows == 0) return MGCN_OK;
  MGCN_REQUIRE(rowptr && Hx && Y, "%s: null array", fn);
  MGCN_REQUIRE(nnz == 0 || (col && g), "%s: null col / g", fn);
  MGCN_REQUIRE(reduce != MGCN_REDUCE_MAX || (argmax && (eid || nnz == 0)),
               "%s: MAX needs argmax and eid", fn);
  MGCN_REQUIRE(ldh >= C && ldy >= C, "%s: leading dimension too small", fn);
  MGCN_REQUIRE(s.order == nullptr || nnz == 0 || s.coef,
               "%s: a schedule needs the coef scratch [nnz]", fn);
  const bool sched = s.order != nullptr;
  if (!sched) s = GateSched{};
  A k{n_rows, C, reduce, relu ? 1 : 0, t_bcast ? 1 : 0, rowptr, col, eid, a, c, t, w,
      Hx, ldh, bias, Y, ldy, g, argmax, s};
  hipStream_t st = as_stream(stream);
  if (s.n_heavy > 0)
    if (int rc = gate_fwd_heavy(k, st)) return rc;
  const int64_t n_work = n_rows - s.n_heavy;
  if (n_work == 0) return MGCN_OK;
  const bool is_max = reduce == MGCN_REDUCE_MAX;
#define CALL(FPL) GATE_LAUNCH(gate_fwd_kernel, FPL, A, is_max, sched, n_work, st, k)
  ATT_DISPATCH(C, CALL);
#undef CALL
  return check_launch("gate_fwd_kernel");
}

extern "C" int mgcn_gate_fwd(int64_t n_rows, int64_t nnz, int32_t C, const int64_t *rowptr,
                             const int32_t *col, const int32_t *eid, const float *a,
                             const float *c, const float *t, int t_bcast, const float *w,
                             const float *Hx, int64_t ldh, int reduce, const float *bias,
                             int relu, float *Y, int64_t ldy, float *g, int32_t *argmax,
                             void *stream) {
  return gate_fwd_run("mgcn_gate_fwd", n_rows, nnz, C, rowptr, col, eid, a, c, t, t_bcast, w, Hx,
                      ldh, reduce, bias, relu, Y, ldy, g, argmax, GateSched{}, stream);
}

extern "C" int mgcn_gate_fwd_sched(int64_t n_rows, int64_t nnz, int32_t C, const int64_t *rowptr,
                                   const int32_t *col, const int32_t *eid, const float *a,
                                   const float *c, const float *t, int t_bcast, const float *w,
                                   const float *Hx, int64_t ldh, int reduce, const float *bias,
                                   int relu, float *Y, int64_t ldy, float *g, int32_t *argmax,
                                   const int32_t *order, int64_t n_heavy, int64_t n_giant,
                                   float *coef, void *stream) {
  return gate_fwd_run("mgcn_gate_fwd_sched", n_rows, nnz, C, rowptr, col, eid, a, c, t, t_bcast,
                      w, Hx, ldh, reduce, bias, relu, Y, ldy, g, argmax,
                      GateSched{order, n_heavy, n_giant, coef}, stream);
}

extern "C" int mgcn_gate_fwd_bf16(int64_t n_rows, int64_t nnz, int32_t C, const int64_t *rowptr,
                                  const int32_t *col, const int32_t *eid, const float *a,
                                  const float *c, const float *t, int t_bcast, const float *w,
                                  const uint16_t *Hx, int64_t ldh, int reduce, const float *bias,
                                  int relu, uint16_t *Y, int64_t ldy, float *g, int32_t *argmax,
                                  void *stream) {
  return gate_fwd_run("mgcn_gate_fwd_bf16", n_rows, nnz, C, rowptr, col, eid, a, c, t, t_bcast,
                      w, Hx, ldh, reduce, bias, relu, Y, ldy, g, argmax, GateSched{}, stream);
}

extern "C" int mgcn_gate_fwd_sched_bf16(int64_t n_rows, int64_t nnz, int32_t C,
                                        const int64_t *rowptr, const int32_t *col,
                                        const int32_t *eid, const float *a, const float *c,
                                        const float *t, int t_bcast, const float *w,
                                        const uint16_t *Hx, int64_t ldh, int reduce,
                                        const float *bias, int relu, uint16_t *Y, int64_t ldy,
                                        float *g, int32_t *argmax, const int32_t *order,
                                        int64_t n_heavy, int64_t n_giant, float *coef,
                                        void *stream) {
  return gate_fwd_run("mgcn_gate_fwd_sched_bf16", n_rows, nnz, C, rowptr, col, eid, a, c, t,
                      t_bcast, w, Hx, ldh, reduce, bias, relu, Y, ldy, g, argmax,
                      GateSched{order, n_heavy, n_giant, coef}, stream);
}

// A: GateBwdDstArgs, or GateBwdDstArgsBf16 (which alone reads cnt)
template <class A>
static int gate_bwd_dst_run(const char *fn, int64_t n_rows, int64_t nnz, int32_t C,
                            const int64_t *rowptr, const int32_t *col,
                            const typename A::Row *Hx, int64_t ldh, const typename A::Row *dY,
                            int64_t lddy, const float *w, const float *g,
                            const uint32_t *win_mask, const float *dg_in, float *dl, float *dc,
                            float *dw, const float *cnt, GateSched s, void *stream) {
  clear_error();
  GATE_REQUIRE_SHAPE(fn, n_rows, nnz, C);
  GATE_REQUIRE_SCHED(fn, s, n_rows);
  MGCN_REQUIRE(cnt == nullptr || win_mask == nullptr,
               "%s: cnt (mean) and win_mask (max) exclude each other", fn);
  if (n_rows == 0) return MGCN_OK;
  MGCN_REQUIRE(rowptr && Hx && dY, "%s: null array", fn);
  MGCN_REQUIRE(nnz == 0 || (col && g && dl), "%s: null col / g / dl", fn);
  MGCN_REQUIRE(ldh >= C && lddy >= C, "%s: leading dimension too small", fn);
  const bool sched = s.order != nullptr;
  if (!sched) s = GateSched{};
  A k{};
  static_cast<GateBwdDstArgsT<typename A::Row> &>(k) = {n_rows, C,  rowptr, col,      Hx, ldh,
                                                        dY,     lddy, w,    g,        dg_in,
                                                        win_mask, dl, dc,   dw,       s};
  if constexpr (A::kCnt) k.cnt = cnt;
  hipStream_t st = as_stream(stream);
  if (s.n_heavy > 0)
    if (int rc = gate_bwd_dst_heavy(k, st)) return rc;
  const int64_t n_work = n_rows - s.n_heavy;
  if (n_work == 0) return MGCN_OK;
  const bool is_max = win_mask != nullptr;
#define CALL(FPL) GATE_LAUNCH(gate_bwd_dst_kernel, FPL, A, is_max, sched, n_work, st, k)
  ATT_DISPATCH(C, CALL);
#undef CALL
  return check_launch("gate_bwd_dst_kernel");
}

extern "C" int mgcn_gate_bwd_dst(int64_t n_rows, int64_t nnz, int32_t C, const int64_t *rowptr,
                                 const int32_t *col, const float *Hx, int64_t ldh,
                                 const float *dY, int64_t lddy, const float *w, const float *g,
                                 const uint32_t *win_mask, const float *dg_in, float *dl,
                                 float *dc, float *dw, void *stream) {
  return gate_bwd_dst_run<GateBwdDstArgs>("mgcn_gate_bwd_dst", n_rows, nnz, C, rowptr, col, Hx,
                                          ldh, dY, lddy, w, g, win_mask, dg_in, dl, dc, dw,
                                          nullptr, GateSched{}, stream);
}

extern "C" int mgcn_gate_bwd_dst_sched(int64_t n_rows, int64_t nnz, int32_t C,
                                       const int64_t *rowptr, const int32_t *col, const float *Hx,
                                       int64_t ldh, const float *dY, int64_t lddy, const float *w,
                                       const float *g, const uint32_t *win_mask,
                                       const float *dg_in, float *dl, float *dc, float *dw,
                                       const int32_t *order, int64_t n_heavy, int64_t n_giant,
                                       void *stream) {
  return gate_bwd_dst_run<GateBwdDstArgs>("mgcn_gate_bwd_dst_sched", n_rows, nnz, C, rowptr, col,
                                          Hx, ldh, dY, lddy, w, g, win_mask, dg_in, dl, dc, dw,
                                          nullptr, GateSched{order, n_heavy, n_giant, nullptr},
                                          stream);
}

extern "C" int mgcn_gate_bwd_dst_bf16(int64_t n_rows, int64_t nnz, int32_t C,
                                      const int64_t *rowptr, const int32_t *col,
                                      const uint16_t *Hx, int64_t ldh, const uint16_t *dY,
                                      int64_t lddy, const float *w, const float *g,
                                      const uint32_t *win_mask, const float *dg_in, float *dl,
                                      float *dc, float *dw, const float *cnt, void *stream) {
  return gate_bwd_dst_run<GateBwdDstArgsBf16>("mgcn_gate_bwd_dst_bf16", n_rows, nnz, C, rowptr,
                                              col, Hx, ldh, dY, lddy, w, g, win_mask, dg_in, dl,
                                              dc, dw, cnt, GateSched{}, stream);
}

extern "C" int mgcn_gate_bwd_dst_sched_bf16(int64_t n_rows, int64_t nnz, int32_t C,
                                            const int64_t *rowptr, const int32_t *col,
                                            const uint16_t *Hx, int64_t ldh, const uint16_t *dY,
                                            int64_t lddy, const float *w, const float *g,
                                            const uint32_t *win_mask, const float *dg_in,
                                            float *dl, float *dc, float *dw, const float *cnt,
                                            const int32_t *order, int64_t n_heavy,
                                            int64_t n_giant, void *stream) {
  return gate_bwd_dst_run<GateBwdDstArgsBf16>(
      "mgcn_gate_bwd_dst_sched_bf16", n_rows, nnz, C, rowptr, col, Hx, ldh, dY, lddy, w, g,
      win_mask, dg_in, dl, dc, dw, cnt, GateSched{order, n_heavy, n_giant, nullptr}, stream);
}

// A: GateBwdSrcArgs, or GateBwdSrcArgsBf16 (which alone reads cnt)
template <class A>
static int gate_bwd_src_run(const char *fn, int64_t n_rows, int64_t nnz, int32_t C,
                            const int64_t *rowptr_t, const int32_t *col_t,
                            const int32_t *slot_map, const typename A::Row *dY, int64_t lddy,
                            const float *w_t, const float *row_scale, const float *g,
                            const float *dl, const uint32_t *win_mask, const float *w_sd,
                            const float *dc, float *da, typename A::Row *dHx, int64_t lddh,
                            const float *cnt, GateSched s, void *stream) {
  clear_error();
  GATE_REQUIRE_SHAPE(fn, n_rows, nnz, C);
  GATE_REQUIRE_SCHED(fn, s, n_rows);
  MGCN_REQUIRE(cnt == nullptr || win_mask == nullptr,
               "%s: cnt (mean) and win_mask (max) exclude each other", fn);
  if (n_rows == 0) return MGCN_OK;
  MGCN_REQUIRE(rowptr_t && dY && dHx, "%s: null array", fn);
  MGCN_REQUIRE(nnz == 0 || (col_t && slot_map && g), "%s: null col / slot_map / g", fn);
  MGCN_REQUIRE(da == nullptr || nnz == 0 || dl, "%s: da needs dl", fn);
  MGCN_REQUIRE((da == nullptr && dc == nullptr) || w_sd, "%s: the rank-one terms need w_sd", fn);
  MGCN_REQUIRE(lddy >= C && lddh >= C, "%s: leading dimension too small", fn);
  MGCN_REQUIRE(s.order == nullptr || nnz == 0 || s.coef,
               "%s: a schedule needs the coef scratch [nnz]", fn);
  const bool sched = s.order != nullptr;
  if (!sched) s = GateSched{};
  A k{};
  static_cast<GateBwdSrcArgsT<typename A::Row> &>(k) = {n_rows, C,   rowptr_t,  col_t, slot_map,
                                                        dY,     lddy, w_t,      row_scale, g,
                                                        dl,     win_mask, w_sd, dc,    da,
                                                        dHx,    lddh, s};
  if constexpr (A::kCnt) k.cnt = cnt;
  hipStream_t st = as_stream(stream);
  if (s.n_heavy > 0)
    if (int rc = gate_bwd_src_heavy(k, st)) return rc;
  const int64_t n_work = n_rows - s.n_heavy;
  if (n_work == 0) return MGCN_OK;
  if constexpr (A::kCnt) {
    if (cnt != nullptr) {  // mean: the dividing instantiation
#define CALL(FPL)                                                                              \
  do {                                                                                         \
    const dim3 grid_(att_grid(n_work)), block_(kAttThreads);                                   \
    if (sched)                                                                                 \
      hipLaunchKernelGGL((gate_bwd_src_kernel<FPL, false, true, A, true>), grid_, block_, 0,   \
                         st, k);                                                               \
    else                                                                                       \
      hipLaunchKernelGGL((gate_bwd_src_kernel<FPL, false, false, A, true>), grid_, block_, 0,  \
                         st, k);                                                               \
  } while (0)
      ATT_DISPATCH(C, CALL);
#undef CALL
      return check_launch("gate_bwd_src_kernel");
    }
  }
  const bool is_max = win_mask != nullptr;
#define CALL(FPL) GATE_LAUNCH(gate_bwd_src_kernel, FPL, A, is_max, sched, n_work, st, k)
  ATT_DISPATCH(C, CALL);
#undef CALL
  return check_launch("gate_bwd_src_kernel");
}

extern "C" int mgcn_gate_bwd_src(int64_t n_rows, int64_t nnz, int32_t C, const int64_t *rowptr_t,
                                 const int32_t *col_t, const int32_t *slot_map, const float *dY,
                                 int64_t lddy, const float *w_t, const float *row_scale,
                                 const float *g, const float *dl, const uint32_t *win_mask,
                                 const float *w_sd, const float *dc, float *da, float *dHx,
                                 int64_t lddh, void *stream) {
  return gate_bwd_src_run<GateBwdSrcArgs>("mgcn_gate_bwd_src", n_rows, nnz, C, rowptr_t, col_t,
                                          slot_map, dY, lddy, w_t, row_scale, g, dl, win_mask,
                                          w_sd, dc, da, dHx, lddh, nullptr, GateSched{}, stream);
}

extern "C" int mgcn_gate_bwd_src_sched(int64_t n_rows, int64_t nnz, int32_t C,
                                       const int64_t *rowptr_t, const int32_t *col_t,
                                       const int32_t *slot_map, const float *dY, int64_t lddy,
                                       const float *w_t, const float *row_scale, const float *g,
                                       const float *dl, const uint32_t *win_mask,
                                       const float *w_sd, const float *dc, float *da, float *dHx,
                                       int64_t lddh, const int32_t *order, int64_t n_heavy,
                                       int64_t n_giant, float *coef, void *stream) {
  return gate_bwd_src_run<GateBwdSrcArgs>("mgcn_gate_bwd_src_sched", n_rows, nnz, C, rowptr_t,
                                          col_t, slot_map, dY, lddy, w_t, row_scale, g, dl,
                                          win_mask, w_sd, dc, da, dHx, lddh, nullptr,
                                          GateSched{order, n_heavy, n_giant, coef}, stream);
}

extern "C" int mgcn_gate_bwd_src_bf16(int64_t n_rows, int64_t nnz, int32_t C,
                                      const int64_t *rowptr_t, const int32_t *col_t,
                                      const int32_t *slot_map, const uint16_t *dY, int64_t lddy,
                                      const float *w_t, const float *row_scale, const float *g,
                                      const float *dl, const uint32_t *win_mask,
                                      const float *w_sd, const float *dc, float *da,
                                      uint16_t *dHx, int64_t lddh, const float *cnt,
                                      void *stream) {
  return gate_bwd_src_run<GateBwdSrcArgsBf16>("mgcn_gate_bwd_src_bf16", n_rows, nnz, C, rowptr_t,
                                              col_t, slot_map, dY, lddy, w_t, row_scale, g, dl,
                                              win_mask, w_sd, dc, da, dHx, lddh, cnt, GateSched{},
                                              stream);
}

extern "C" int mgcn_gate_bwd_src_sched_bf16(int64_t n_rows, int64_t nnz, int32_t C,
                                            const int64_t *rowptr_t, const int32_t *col_t,
                                            const int32_t *slot_map, const uint16_t *dY,
                                            int64_t lddy, const float *w_t,
                                            const float *row_scale, const float *g,
                                            const float *dl, const uint32_t *win_mask,
                                            const float *w_sd, const float *dc, float *da,
                                            uint16_t *dHx, int64_t lddh, const float *cnt,
                                            const int32_t *order, int64_t n_heavy,
                                            int64_t n_giant, float *coef, void *stream) {
  return gate_bwd_src_run<GateBwdSrcArgsBf16>(
      "mgcn_gate_bwd_src_sched_bf16", n_rows, nnz, C, rowptr_t, col_t, slot_map, dY, lddy, w_t,
      row_scale, g, dl, win_mask, w_sd, dc, da, dHx, lddh, cnt,
      GateSched{order, n_heavy, n_giant, coef}, stream);
}
