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
// results are bitwise repeatable.
//
// Roofline (forward): 8 (N + 1) rowptr + nnz (4 col + 4 C row + 4 a + 4 g
// [+ 4 w] [+ 4 t]) + 4 N C (Y) + 4 N (c) bytes.

#include "attention.h"

namespace mgcn {
namespace {

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

// ----------------------------------------------------------------- forward
struct GateFwdArgs {
  int64_t n_rows;
  int C, reduce, relu, t_bcast;
  const int64_t *rowptr;
  const int32_t *col, *eid;
  const float *a, *c, *t, *w, *Hx;
  int64_t ldh;
  const float *bias;
  float *Y;
  int64_t ldy;
  float *g;
  int32_t *argmax;
};

template <int FPL, bool MAX>
__global__ __launch_bounds__(kAttThreads) void gate_fwd_kernel(GateFwdArgs a) {
  constexpr int U = gather_unroll<FPL>();
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = blockIdx.x * (int64_t)kAttWaves + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kAttWaves;
  const int C = a.C;
  const float tb = (a.t != nullptr && a.t_bcast) ? a.t[0] : 0.0f;
  for (int64_t row = wave0; row < a.n_rows; row += nwaves) {
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
            hp[u][i] = (on && f < C) ? a.Hx[c * a.ldh + f] : 0.0f;
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
        a.Y[row * a.ldy + f] = y;
      }
    }
  }
}

// ------------------------------------------------- adjoint, by destination
struct GateBwdDstArgs {
  int64_t n_rows;
  int C;
  const int64_t *rowptr;
  const int32_t *col;
  const float *Hx;
  int64_t ldh;
  const float *dY;
  int64_t lddy;
  const float *w, *g, *dg_in;
  const uint32_t *win;
  float *dl, *dc, *dw;
};

template <int FPL, bool MAX>
__global__ __launch_bounds__(kAttThreads) void gate_bwd_dst_kernel(GateBwdDstArgs a) {
  constexpr int U = gather_unroll<FPL>();
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = blockIdx.x * (int64_t)kAttWaves + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kAttWaves;
  const int C = a.C, W = (a.C + 31) >> 5;
  for (int64_t row = wave0; row < a.n_rows; row += nwaves) {
    float dy[FPL];
#pragma unroll
    for (int i = 0; i < FPL; ++i) {
      const int f = lane + 64 * i;
      dy[i] = f < C ? a.dY[row * a.lddy + f] : 0.0f;
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
            hp[u][i] = ld ? a.Hx[c * a.ldh + f] : 0.0f;
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
struct GateBwdSrcArgs {
  int64_t n_rows;
  int C;
  const int64_t *rowptr;
  const int32_t *col, *slot;
  const float *dY;
  int64_t lddy;
  const float *w_t, *row_scale, *g, *dl;
  const uint32_t *win;
  const float *wsd, *dc;
  float *da, *dHx;
  int64_t lddh;
};

template <int FPL, bool MAX>
__global__ __launch_bounds__(kAttThreads) void gate_bwd_src_kernel(GateBwdSrcArgs a) {
  constexpr int U = gather_unroll<FPL>();
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = blockIdx.x * (int64_t)kAttWaves + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kAttWaves;
  const int C = a.C, W = (a.C + 31) >> 5;
  for (int64_t row = wave0; row < a.n_rows; row += nwaves) {
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
            dy[u][i] = ld ? a.dY[c * a.lddy + f] : 0.0f;
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (kk + u < ns) {
            const float w = __shfl(coef, kk + u, 64);
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
        a.dHx[row * a.lddh + f] = v;
      }
    }
  }
}

}  // namespace
}  // namespace mgcn

using namespace mgcn;

#define GATE_REQUIRE_SHAPE(fn, n_rows, nnz, C)                                          \
  do {                                                                                  \
    MGCN_REQUIRE((n_rows) >= 0 && (nnz) >= 0, fn ": negative size");                    \
    MGCN_REQUIRE((C) >= 1 && (C) <= 1024, fn ": need 1 <= C <= 1024 (C = %d)", (int)(C)); \
    MGCN_REQUIRE((int64_t)(nnz) < ((int64_t)1 << 31), fn ": need nnz < 2^31");           \
  } while (0)

extern "C" int mgcn_gate_fwd(int64_t n_rows, int64_t nnz, int32_t C, const int64_t *rowptr,
                             const int32_t *col, const int32_t *eid, const float *a,
                             const float *c, const float *t, int t_bcast, const float *w,
                             const float *Hx, int64_t ldh, int reduce, const float *bias,
                             int relu, float *Y, int64_t ldy, float *g, int32_t *argmax,
                             void *stream) {
  clear_error();
  GATE_REQUIRE_SHAPE("mgcn_gate_fwd", n_rows, nnz, C);
  MGCN_REQUIRE(reduce == MGCN_REDUCE_SUM || reduce == MGCN_REDUCE_MEAN ||
                   reduce == MGCN_REDUCE_MAX, "mgcn_gate_fwd: bad reduce %d", reduce);
  if (n_rows == 0) return MGCN_OK;
  MGCN_REQUIRE(rowptr && Hx && Y, "mgcn_gate_fwd: null array");
  MGCN_REQUIRE(nnz == 0 || (col && g), "mgcn_gate_fwd: null col / g");
  MGCN_REQUIRE(reduce != MGCN_REDUCE_MAX || (argmax && (eid || nnz == 0)),
               "mgcn_gate_fwd: MAX needs argmax and eid");
  MGCN_REQUIRE(ldh >= C && ldy >= C, "mgcn_gate_fwd: leading dimension too small");
  GateFwdArgs k{n_rows, C, reduce, relu ? 1 : 0, t_bcast ? 1 : 0, rowptr, col, eid, a, c, t, w,
                Hx, ldh, bias, Y, ldy, g, argmax};
  hipStream_t s = as_stream(stream);
#define CALL(FPL)                                                                             \
  do {                                                                                        \
    if (reduce == MGCN_REDUCE_MAX)                                                            \
      hipLaunchKernelGGL((gate_fwd_kernel<FPL, true>), dim3(att_grid(n_rows)),                \
                         dim3(kAttThreads), 0, s, k);                                         \
    else                                                                                      \
      hipLaunchKernelGGL((gate_fwd_kernel<FPL, false>), dim3(att_grid(n_rows)),               \
                         dim3(kAttThreads), 0, s, k);                                         \
  } while (0)
  ATT_DISPATCH(C, CALL);
#undef CALL
  return check_launch("gate_fwd_kernel");
}

extern "C" int mgcn_gate_bwd_dst(int64_t n_rows, int64_t nnz, int32_t C, const int64_t *rowptr,
                                 const int32_t *col, const float *Hx, int64_t ldh,
                                 const float *dY, int64_t lddy, const float *w, const float *g,
                                 const uint32_t *win_mask, const float *dg_in, float *dl,
                                 float *dc, float *dw, void *stream) {
  clear_error();
  GATE_REQUIRE_SHAPE("mgcn_gate_bwd_dst", n_rows, nnz, C);
  if (n_rows == 0) return MGCN_OK;
  MGCN_REQUIRE(rowptr && Hx && dY, "mgcn_gate_bwd_dst: null array");
  MGCN_REQUIRE(nnz == 0 || (col && g && dl), "mgcn_gate_bwd_dst: null col / g / dl");
  MGCN_REQUIRE(ldh >= C && lddy >= C, "mgcn_gate_bwd_dst: leading dimension too small");
  GateBwdDstArgs k{n_rows, C, rowptr, col, Hx, ldh, dY, lddy, w, g, dg_in, win_mask, dl, dc, dw};
  hipStream_t s = as_stream(stream);
#define CALL(FPL)                                                                             \
  do {                                                                                        \
    if (win_mask != nullptr)                                                                  \
      hipLaunchKernelGGL((gate_bwd_dst_kernel<FPL, true>), dim3(att_grid(n_rows)),            \
                         dim3(kAttThreads), 0, s, k);                                         \
    else                                                                                      \
      hipLaunchKernelGGL((gate_bwd_dst_kernel<FPL, false>), dim3(att_grid(n_rows)),           \
                         dim3(kAttThreads), 0, s, k);                                         \
  } while (0)
  ATT_DISPATCH(C, CALL);
#undef CALL
  return check_launch("gate_bwd_dst_kernel");
}

extern "C" int mgcn_gate_bwd_src(int64_t n_rows, int64_t nnz, int32_t C, const int64_t *rowptr_t,
                                 const int32_t *col_t, const int32_t *slot_map, const float *dY,
                                 int64_t lddy, const float *w_t, const float *row_scale,
                                 const float *g, const float *dl, const uint32_t *win_mask,
                                 const float *w_sd, const float *dc, float *da, float *dHx,
                                 int64_t lddh, void *stream) {
  clear_error();
  GATE_REQUIRE_SHAPE("mgcn_gate_bwd_src", n_rows, nnz, C);
  if (n_rows == 0) return MGCN_OK;
  MGCN_REQUIRE(rowptr_t && dY && dHx, "mgcn_gate_bwd_src: null array");
  MGCN_REQUIRE(nnz == 0 || (col_t && slot_map && g), "mgcn_gate_bwd_src: null col / slot_map / g");
  MGCN_REQUIRE(da == nullptr || nnz == 0 || dl, "mgcn_gate_bwd_src: da needs dl");
  MGCN_REQUIRE((da == nullptr && dc == nullptr) || w_sd,
               "mgcn_gate_bwd_src: the rank-one terms need w_sd");
  MGCN_REQUIRE(lddy >= C && lddh >= C, "mgcn_gate_bwd_src: leading dimension too small");
  GateBwdSrcArgs k{n_rows, C, rowptr_t, col_t, slot_map, dY, lddy, w_t, row_scale, g, dl,
                   win_mask, w_sd, dc, da, dHx, lddh};
  hipStream_t s = as_stream(stream);
#define CALL(FPL)                                                                             \
  do {                                                                                        \
    if (win_mask != nullptr)                                                                  \
      hipLaunchKernelGGL((gate_bwd_src_kernel<FPL, true>), dim3(att_grid(n_rows)),            \
                         dim3(kAttThreads), 0, s, k);                                         \
    else                                                                                      \
      hipLaunchKernelGGL((gate_bwd_src_kernel<FPL, false>), dim3(att_grid(n_rows)),           \
                         dim3(kAttThreads), 0, s, k);                                         \
  } while (0)
  ATT_DISPATCH(C, CALL);
#undef CALL
  return check_launch("gate_bwd_src_kernel");
}
