// Multi-kernel GCN aggregation on gfx950 (MI355X): K edge sets ("kernels",
// src/gcn_meta/models/gcn_multi_kernel.py:76-114) over one node set, one
// launch per direction.
//
// The layer computes  combine_k epi_k( A_k (x W_k) )  with a weight_node, a
// degree normalisation and a bias per kernel.  With H_all = x [W_0 | .. |
// W_{K-1}] ([N, K C], one GEMM) the forward gathers column block k of H_all
// over view k and combines the K results per destination row; the adjoint
// gathers dY over the K transposed views into the column blocks of dH_all.
//
// Work split: spmm.hip's lane groups.  A group of G lanes owns one output row
// for all K kernels: it walks view 0's slots, then view 1's, ..., each in slot
// (COO) order with U gathered rows in flight, and keeps the combined row in
// registers, so the K partial results are never written.  Edge metadata (col,
// w, cnt) is loaded lane-parallel, G slots per instruction, and broadcast in
// the group; the row pointers of all K views are loaded lane-parallel too
// (lane k of the group holds view k's) one row ahead of the gathers.  Rows in
// natural order, no heavy-row path (the host routes graphs with heavy rows to
// the per-kernel launches), no LDS, no atomics.  Products and sums are rounded
// separately, divisions are true divisions: per kernel the arithmetic is that
// of spmm_kernel, so the results equal K mgcn_spmm_fwd / mgcn_spmm_bwd calls
// on the column-block views, combined left to right, bit for bit.
//
// Roofline: HBM-bound.  Algorithmic bytes, forward:
//     sum_k [8 (N + 1) + nnz_k (4 col + 4 w + 4 C)] + 4 N C   (cat: 4 N K C)
// against the K launches' sum_k [...] + 4 N C (3 K - 2): the K results
// written, and read and written again by the K - 1 adds.

#include "heavy.h"
#include "mgcn_internal.h"

namespace mgcn {
namespace {

constexpr int kWaves = 4;  // waves per 256-thread block
constexpr int kBlock = 64 * kWaves;

struct MultiArgs {
  int64_t n_rows;
  int32_t C, K, n_chunks;
  int32_t mean, relu, cat;  // reduce MEAN; fwd ReLU; combine CAT
  float comb_div;           // combine MEAN: K, else 1
  mgcn_multi_views v;
  const float *X;  // gathered rows (H_all forward, dY adjoint)
  int64_t ldx;
  float *Y;  // output rows (Y forward, dH_all adjoint)
  int64_t ldy;
};

// Broadcast lane `k` of this lane's group (groups of G lanes).  G == 64: the
// group is the wave and k is wave-uniform -> v_readlane.
template <int G>
__device__ __forceinline__ int bcast_i(int v, int group_base, int k) {
  if constexpr (G == 64) {
    return __builtin_amdgcn_readlane(v, k);
  } else {
    return __shfl(v, group_base + k, 64);
  }
}
template <int G>
__device__ __forceinline__ float bcast_f(float v, int group_base, int k) {
  return __int_as_float(bcast_i<G>(__float_as_int(v), group_base, k));
}
template <int G>
__device__ __forceinline__ int64_t bcast_l(int64_t v, int group_base, int k) {
  const uint32_t lo = (uint32_t)bcast_i<G>((int)(uint32_t)v, group_base, k);
  const uint32_t hi = (uint32_t)bcast_i<G>((int)(uint32_t)((uint64_t)v >> 32), group_base, k);
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// max over the wave of a per-group value (groups of G lanes; all lanes active)
template <int G>
__device__ __forceinline__ int64_t wave_max_over_groups(int64_t v) {
#pragma unroll
  for (int off = G; off < 64; off <<= 1) {
    const int64_t o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}

// MODE: the forward; the adjoint as a plain sum; the adjoint with its
// divisions (combine mean: by K, reduce mean: by the gathered row's count) --
// apart, so that the plain sum carries neither the count's broadcast nor a
// branch per gathered row
enum MultiMode : int { M_FWD = 0, M_BWD = 1, M_BWD_DIV = 2 };

template <int VEC, int G, int U, int MODE>
__global__ __launch_bounds__(kBlock) void multi_spmm_kernel(const MultiArgs a) {
  constexpr bool FWD = MODE == M_FWD;
  constexpr bool DIV = MODE == M_BWD_DIV;
  constexpr int RPW = 64 / G;  // rows per wave
  // row-pointer slots per lane: view k sits in lane k % G, slot k / G
  constexpr int NS = (MGCN_MULTI_MAX_K + G - 1) / G;
  const int lane = threadIdx.x & 63;
  const int gl = lane & (G - 1);
  const int grp = lane / G;
  const int gbase = grp * G;
  const int wave_in_block = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t n_row_groups = (a.n_rows + RPW - 1) / RPW;
  const int64_t wave_stride = (int64_t)gridDim.x * kWaves;
  const float *__restrict__ X = a.X;

  // first slot and degree of the group's row in every view, one row ahead of
  // the gathers (a row then costs col -> rows round trips, not rowptr -> col
  // -> rows, K times)
  auto load_ptrs = [&](int64_t wv, int64_t (&b)[NS], int64_t (&d)[NS]) {
    const int64_t row = wv * RPW + grp;
    const bool ok = wv < n_row_groups && row < a.n_rows;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int k = gl + s * G;
      b[s] = 0;
      d[s] = 0;
      if (ok && k < a.K) {
        const int64_t *__restrict__ rp = a.v.rowptr[k];
        b[s] = rp[row];
        d[s] = rp[row + 1] - b[s];
      }
    }
  };

  const int64_t wv0 = (int64_t)blockIdx.x * kWaves + wave_in_block;
  int64_t beg_n[NS], deg_n[NS];
  load_ptrs(wv0, beg_n, deg_n);
  for (int64_t wv = wv0; wv < n_row_groups; wv += wave_stride) {
    int64_t beg_c[NS], deg_c[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      beg_c[s] = beg_n[s];
      deg_c[s] = deg_n[s];
    }
    load_ptrs(wv + wave_stride, beg_n, deg_n);
    const int64_t row = wv * RPW + grp;
    const bool row_ok = row < a.n_rows;

    for (int c = 0; c < a.n_chunks; ++c) {
      const int f0 = (c * G + gl) * VEC;
      const bool f_ok = f0 < a.C;
      F32v<VEC> y;  // forward, combine add / mean: the kernels' results so far
#pragma unroll
      for (int j = 0; j < VEC; ++j) y.v[j] = 0.0f;

      for (int k = 0; k < a.K; ++k) {  // wave-uniform
        int64_t beg, deg;
        if constexpr (NS == 1) {
          beg = bcast_l<G>(beg_c[0], gbase, k);
          deg = bcast_l<G>(deg_c[0], gbase, k);
        } else {
          const bool hi = k >= G;
          beg = bcast_l<G>(hi ? beg_c[1] : beg_c[0], gbase, k & (G - 1));
          deg = bcast_l<G>(hi ? deg_c[1] : deg_c[0], gbase, k & (G - 1));
        }
        const int64_t maxdeg = (RPW > 1) ? wave_max_over_groups<G>(deg) : deg;
        const int32_t *__restrict__ colk = a.v.col[k];
        const float *__restrict__ wk_all = a.v.w[k];
        const float *__restrict__ cntk_all = a.v.cnt[k];
        const bool has_w = wk_all != nullptr;
        const bool by_cnt = DIV && a.mean;
        // column block of view k in the gathered table (adjoint: of dY under cat)
        const int64_t xoff = (FWD || a.cat) ? (int64_t)k * a.C + f0 : (int64_t)f0;
        F32v<VEC> acc;
#pragma unroll
        for (int j = 0; j < VEC; ++j) acc.v[j] = 0.0f;

        for (int64_t e0 = 0; e0 < maxdeg; e0 += G) {
          // lane-parallel metadata for the next (up to) G slots of this row
          const int64_t my = e0 + gl;
          int mc = 0;
          float mw = 1.0f, mcnt = 1.0f;
          if (my < deg) {
            mc = colk[beg + my];
            if (has_w) mw = wk_all[beg + my];
            if constexpr (DIV) {
              if (by_cnt) mcnt = cntk_all[mc];
            }
          }
          const int64_t rem = deg - e0;
          const int nb = rem <= 0 ? 0 : (rem < G ? (int)rem : G);  // this group
          const int64_t remw = maxdeg - e0;
          const int nbmax = remw < G ? (int)remw : G;              // wave-uniform

          for (int k0 = 0; k0 < nbmax; k0 += U) {
            F32v<VEC> xv[U];
            float wk[U], ck[U];
            bool ok[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
              const int e = k0 + u;
              const int ee = e & (G - 1);
              const int cu = bcast_i<G>(mc, gbase, ee);
              wk[u] = bcast_f<G>(mw, gbase, ee);
              ck[u] = 1.0f;
              if constexpr (DIV) ck[u] = bcast_f<G>(mcnt, gbase, ee);
              ok[u] = (e < nb) && f_ok;
              if (ok[u]) {
                xv[u] = load_f<VEC>(X + (int64_t)cu * a.ldx + xoff);
              } else {
#pragma unroll
                for (int j = 0; j < VEC; ++j) xv[u].v[j] = 0.0f;
              }
            }
            // fold in strictly ascending slot order
#pragma unroll
            for (int u = 0; u < U; ++u) {
              if (ok[u]) {
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                  float g = xv[u].v[j];
                  if constexpr (DIV) {  // x / 1 is x: an absent divisor is 1
                    g = __fdiv_rn(g, a.comb_div);
                    g = __fdiv_rn(g, ck[u]);
                  }
                  acc.v[j] = __fadd_rn(acc.v[j], __fmul_rn(g, wk[u]));
                }
              }
            }
          }
        }

        if constexpr (FWD) {
          // kernel k's epilogue (mgcn_spmm_fwd's), then the combine
          const float *__restrict__ bk = a.v.bias[k];
          const float cnt = (float)(deg > 1 ? deg : 1);
#pragma unroll
          for (int j = 0; j < VEC; ++j) {
            float s = acc.v[j];
            if (a.mean) s = __fdiv_rn(s, cnt);
            if (bk != nullptr && f_ok) s = __fadd_rn(s, bk[f0 + j]);
            if (a.cat) {
              acc.v[j] = (a.relu && s < 0.0f) ? 0.0f : s;
            } else {
              y.v[j] = (k == 0) ? s : __fadd_rn(y.v[j], s);
            }
          }
          if (a.cat && row_ok && f_ok) {
            float *dst = a.Y + row * a.ldy + (int64_t)k * a.C + f0;
            if constexpr (MGCN_NT_EXTRA != 0 && G >= 32) store_f_nt<VEC>(dst, acc);
            else store_f<VEC>(dst, acc);
          }
        } else {
          if (row_ok && f_ok) {
            const float *__restrict__ rs = a.v.row_scale[k];
            if (rs != nullptr) {
              const float s = rs[row];
#pragma unroll
              for (int j = 0; j < VEC; ++j) acc.v[j] = __fmul_rn(acc.v[j], s);
            }
            float *dst = a.Y + row * a.ldy + (int64_t)k * a.C + f0;
            if constexpr (MGCN_NT_EXTRA != 0 && G >= 32) store_f_nt<VEC>(dst, acc);
            else store_f<VEC>(dst, acc);
          }
        }
      }

      if constexpr (FWD) {
        if (!a.cat && row_ok && f_ok) {
#pragma unroll
          for (int j = 0; j < VEC; ++j) {
            float v = y.v[j];
            if (a.comb_div != 1.0f) v = __fdiv_rn(v, a.comb_div);
            y.v[j] = (a.relu && v < 0.0f) ? 0.0f : v;
          }
          float *dst = a.Y + row * a.ldy + f0;
          if constexpr (MGCN_NT_EXTRA != 0 && G >= 32) store_f_nt<VEC>(dst, y);
          else store_f<VEC>(dst, y);
        }
      }
    }
  }
}

template <int VEC, int G, int U, int MODE>
int launch_one(const MultiArgs &a, hipStream_t stream) {
  constexpr int RPW = 64 / G;
  const int64_t waves = (a.n_rows + RPW - 1) / RPW;
  int64_t blocks = (waves + kWaves - 1) / kWaves;
  if (blocks > (int64_t(1) << 20)) blocks = int64_t(1) << 20;  // grid-stride beyond
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL((multi_spmm_kernel<VEC, G, U, MODE>), dim3((unsigned)blocks), dim3(kBlock), 0,
                     stream, a);
  return check_launch("multi_spmm_kernel");
}

// the lane group of spmm.hip's launch_g: the narrowest that covers a row
template <int VEC, int MODE>
int launch_g(MultiArgs a, hipStream_t stream) {
  const int lanes = (a.C + VEC - 1) / VEC;
  a.n_chunks = (lanes + 63) / 64;
  if (lanes > 32) return launch_one<VEC, 64, 8, MODE>(a, stream);
  if (lanes > 16) return launch_one<VEC, 32, 8, MODE>(a, stream);
  if (lanes > 8) return launch_one<VEC, 16, 8, MODE>(a, stream);
  if (lanes > 4) return launch_one<VEC, 8, 8, MODE>(a, stream);
  return launch_one<VEC, 4, 4, MODE>(a, stream);
}

template <int MODE>
int launch_v(const MultiArgs &a, int vec, hipStream_t stream) {
  if (vec == 4) return launch_g<4, MODE>(a, stream);
  if (vec == 2) return launch_g<2, MODE>(a, stream);
  return launch_g<1, MODE>(a, stream);
}

// Widest vector every accessed block allows: column block k starts k C floats
// into a row, so C must be a multiple of it as well as both leading dimensions
// and both base addresses.
int multi_vec(int32_t C, const void *p0, int64_t ld0, const void *p1, int64_t ld1) {
  auto ok = [&](int v) {
    return C % v == 0 && ld0 % v == 0 && ld1 % v == 0 &&
           reinterpret_cast<uintptr_t>(p0) % (4 * v) == 0 &&
           reinterpret_cast<uintptr_t>(p1) % (4 * v) == 0;
  };
  return ok(4) ? 4 : ok(2) ? 2 : 1;
}

// the checks both entry points share; *noop: nothing to launch
int check_common(const char *who, int64_t n_rows, int32_t K, int32_t C,
                 const mgcn_multi_views &v, int reduce, int combine, bool *noop) {
  *noop = false;
  MGCN_REQUIRE(K >= 1 && K <= MGCN_MULTI_MAX_K, "%s: K = %d outside [1, %d]", who, K,
               MGCN_MULTI_MAX_K);
  MGCN_REQUIRE(n_rows >= 0 && C >= 1, "%s: need n_rows >= 0 and C >= 1", who);
  MGCN_REQUIRE((int64_t)K * C <= INT32_MAX, "%s: K C too large", who);
  MGCN_REQUIRE(reduce == MGCN_REDUCE_SUM || reduce == MGCN_REDUCE_MEAN,
               "%s: reduce must be SUM or MEAN, got %d", who, reduce);
  MGCN_REQUIRE(combine == MGCN_COMBINE_ADD || combine == MGCN_COMBINE_MEAN ||
                   combine == MGCN_COMBINE_CAT,
               "%s: bad combine %d", who, combine);
  for (int k = 0; k < K; ++k)
    MGCN_REQUIRE(v.n_rows[k] == n_rows, "%s: view %d has %lld rows, the call %lld", who, k,
                 (long long)v.n_rows[k], (long long)n_rows);
  if (n_rows == 0) {
    *noop = true;
    return MGCN_OK;
  }
  for (int k = 0; k < K; ++k)  // col may be NULL when the view has no edges
    MGCN_REQUIRE(v.rowptr[k] != nullptr, "%s: view %d: null rowptr", who, k);
  return MGCN_OK;
}

}  // namespace
}  // namespace mgcn

using namespace mgcn;

extern "C" int mgcn_multi_spmm_fwd(int64_t n_rows, int32_t K, int32_t C, mgcn_multi_views views,
                                   const float *H_all, int64_t ldh, float *Y, int64_t ldy,
                                   int reduce, int combine, int relu, void *stream) {
  clear_error();
  bool noop = false;
  if (int rc = check_common("mgcn_multi_spmm_fwd", n_rows, K, C, views, reduce, combine, &noop))
    return rc;
  if (noop) return MGCN_OK;
  const bool cat = combine == MGCN_COMBINE_CAT;
  MGCN_REQUIRE(H_all && Y, "mgcn_multi_spmm_fwd: null array");
  MGCN_REQUIRE(ldh >= (int64_t)K * C && ldy >= (cat ? (int64_t)K * C : (int64_t)C),
               "mgcn_multi_spmm_fwd: leading dimension too small");
  MultiArgs a{};
  a.n_rows = n_rows;
  a.C = C;
  a.K = K;
  a.mean = reduce == MGCN_REDUCE_MEAN;
  a.relu = relu != 0;
  a.cat = cat;
  a.comb_div = combine == MGCN_COMBINE_MEAN ? (float)K : 1.0f;
  a.v = views;
  for (int k = 0; k < MGCN_MULTI_MAX_K; ++k) {
    a.v.cnt[k] = nullptr;  // adjoint arrays: not read by the forward
    a.v.row_scale[k] = nullptr;
    if (k < K)
      MGCN_REQUIRE(reinterpret_cast<uintptr_t>(views.bias[k]) % 4 == 0,
                   "mgcn_multi_spmm_fwd: bias not 4-byte aligned");
  }
  a.X = H_all;
  a.ldx = ldh;
  a.Y = Y;
  a.ldy = ldy;
  return launch_v<M_FWD>(a, multi_vec(C, H_all, ldh, Y, ldy), as_stream(stream));
}

extern "C" int mgcn_multi_spmm_bwd(int64_t n_rows, int32_t K, int32_t C, mgcn_multi_views views_t,
                                   const float *dY, int64_t lddy, float *dH_all, int64_t lddh,
                                   int reduce, int combine, void *stream) {
  clear_error();
  bool noop = false;
  if (int rc = check_common("mgcn_multi_spmm_bwd", n_rows, K, C, views_t, reduce, combine, &noop))
    return rc;
  if (noop) return MGCN_OK;
  const bool cat = combine == MGCN_COMBINE_CAT;
  MGCN_REQUIRE(dY && dH_all, "mgcn_multi_spmm_bwd: null array");
  MGCN_REQUIRE(lddh >= (int64_t)K * C && lddy >= (cat ? (int64_t)K * C : (int64_t)C),
               "mgcn_multi_spmm_bwd: leading dimension too small");
  if (reduce == MGCN_REDUCE_MEAN)
    for (int k = 0; k < K; ++k)
      MGCN_REQUIRE(views_t.cnt[k] != nullptr, "mgcn_multi_spmm_bwd: MEAN needs cnt (view %d)", k);
  MultiArgs a{};
  a.n_rows = n_rows;
  a.C = C;
  a.K = K;
  a.mean = reduce == MGCN_REDUCE_MEAN;
  a.cat = cat;
  a.comb_div = combine == MGCN_COMBINE_MEAN ? (float)K : 1.0f;
  a.v = views_t;
  a.X = dY;
  a.ldx = lddy;
  a.Y = dH_all;
  a.ldy = lddh;
  const int vec = multi_vec(C, dY, lddy, dH_all, lddh);
  if (a.mean || a.comb_div != 1.0f) return launch_v<M_BWD_DIV>(a, vec, as_stream(stream));
  return launch_v<M_BWD>(a, vec, as_stream(stream));
}
