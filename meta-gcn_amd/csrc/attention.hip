// Multi-head soft attention over a node's neighbourhood (gfx950): the message
// passing of NodeModelAttention (src/gcn_meta/models/graph_attention.py:60-117
// with the sparse softmax of common.py:69-92) and its adjoint.
//
// With Hp = X W viewed as [N, H, C] and the attention vector a [H, 2C]:
//   s_src[n,h] = sum_c Hp[n,h,c] a[h,c]      s_dst[n,h] = sum_c Hp[n,h,c] a[h,C+c]
//   z_k = s_src[j,h] + s_dst[i,h]   e_k = act(z_k)            (edge k: j -> i)
//   alpha_k = exp(e_k - m) / (sum_group exp(e - m) + 1e-16),  m = max(-1e16, max_group e)
//   Y[i,h,:] = sum_{k -> i} alpha_k mask_k Hp[j,h,:]
// The reference materialises x_j, x_i and their concatenation ([E, H, 2C]) to
// form z; z only needs the two per-node scores, so the [E, ...] tensors never
// exist here: the per-edge state is alpha [nnz, H] (and dz in the backward).
//
// Work split (all kernels: 4 waves per workgroup, one wave per CSR row,
// grid-stride over rows, a row of any degree walked in chunks):
//  * feature phase: lane l holds features f = l + 64 i (i < FPL) of the row's
//    H C wide vector, so every gathered row is read coalesced; the head of a
//    feature is f / C (any C).  Per-head dot products sum the lane's own
//    products of that head in i order and then take a fixed xor-butterfly
//    (C a power of two <= 64: one segmented butterfly for all heads).
//  * edge phase ("flat"): lane t of a chunk stands for (slot k0 + t / H, head
//    t % H) -- 64 / H slots per chunk -- which is exactly the [nnz, H] layout
//    of alpha / mask / dz, so those are read and written coalesced.  Group
//    sums: every lane sums its own entries chunk after chunk, then the lanes
//    of one head are combined in a fixed order (butterfly over the strides
//    >= H when H divides 64, else lane group after lane group).
//  * the weighted gather takes alpha' of (slot, head of f) from the lane that
//    holds it (ds_bpermute): no LDS, no barrier, no atomics.
// Rows keep COO order and every sum has a fixed order: results are bitwise
// repeatable.  The summation order is not the reference's (a CPU scatter_add
// over [E, H]), so results match it to fp32 rounding, not bit for bit.
//
// Roofline (forward, 'in'): 8 (N + 1) rowptr + nnz (4 col + 4 H C row + 4 H
// s_src + 4 H alpha) + 4 N H C (Y) + 4 N H (s_dst) bytes.

#include "mgcn_internal.h"

namespace mgcn {
namespace {

constexpr int kAttWaves = 4;
constexpr int kAttThreads = 64 * kAttWaves;

__device__ inline float att_act(float z, int act) {
  if (act == MGCN_ATT_ACT_LRELU) return z > 0.0f ? z : __fmul_rn(z, 0.2f);
  if (act == MGCN_ATT_ACT_RELU) return z > 0.0f ? z : 0.0f;
  return z;
}

// d act / dz as torch's leaky_relu / relu backward take it (z == 0: the
// negative side)
__device__ inline float att_act_grad(float z, int act) {
  if (act == MGCN_ATT_ACT_LRELU) return z > 0.0f ? 1.0f : 0.2f;
  if (act == MGCN_ATT_ACT_RELU) return z > 0.0f ? 1.0f : 0.0f;
  return 1.0f;
}

// Flat layout: the total over the lanes of one head (lane % H), left in every
// lane of that head.  Lanes >= (64 / H) H pass 0.
__device__ inline float head_sum(float v, int H, int h) {
  if ((H & (H - 1)) == 0) {
    for (int off = 32; off >= H; off >>= 1) v = __fadd_rn(v, __shfl_xor(v, off, 64));
    return v;
  }
  float acc = 0.0f;
  for (int g = 0; g < 64 / H; ++g) acc = __fadd_rn(acc, __shfl(v, g * H + h, 64));
  return acc;
}

__device__ inline float head_max(float v, int H, int h) {
  if ((H & (H - 1)) == 0) {
    for (int off = 32; off >= H; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
  }
  float acc = v;
  for (int g = 0; g < 64 / H; ++g) acc = fmaxf(acc, __shfl(v, g * H + h, 64));
  return acc;
}

// Feature layout: lane hh (< H) receives sum_{f of head hh} prod[f]; every
// lane calls it.  Own products in i order, then the xor-butterfly, head after
// head.  C a power of two <= 64: the heads are aligned segments of C lanes
// (head of (lane, i) = lane / C + i 64 / C), so one segmented butterfly per i
// sums all of them at once and lane hh fetches its head's total.
template <int FPL>
__device__ inline float head_dots(const float (&prod)[FPL], const int (&hf)[FPL], int H, int C,
                                  int lane) {
  float mine = 0.0f;
  if ((C & (C - 1)) == 0 && C <= 64) {
    const int hpi = 64 / C;
#pragma unroll
    for (int i = 0; i < FPL; ++i) {
      float p = prod[i];
      for (int off = C >> 1; off >= 1; off >>= 1) p = __fadd_rn(p, __shfl_xor(p, off, 64));
      const float v = __shfl(p, (lane % hpi) * C, 64);
      if (lane / hpi == i) mine = v;
    }
    return mine;
  }
  for (int hh = 0; hh < H; ++hh) {
    float p = 0.0f;
#pragma unroll
    for (int i = 0; i < FPL; ++i) p = __fadd_rn(p, hf[i] == hh ? prod[i] : 0.0f);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) p = __fadd_rn(p, __shfl_xor(p, off, 64));
    if (lane == hh) mine = p;
  }
  return mine;
}

template <int FPL>
__device__ inline void feature_heads(int (&hf)[FPL], int lane, int HC, int C) {
#pragma unroll
  for (int i = 0; i < FPL; ++i) {
    const int f = lane + 64 * i;
    hf[i] = f < HC ? f / C : 0;
  }
}

template <int FPL>
constexpr int gather_unroll() {
  return FPL <= 4 ? 4 : 2;
}

// ------------------------------------------------------------------ scores
struct ScoreArgs {
  int64_t n;
  int H, C;
  const float *Hp;
  int64_t ldh;
  const float *a;
  float *s_src, *s_dst;
};

template <int FPL>
__global__ __launch_bounds__(kAttThreads) void att_scores_kernel(ScoreArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = blockIdx.x * (int64_t)kAttWaves + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kAttWaves;
  const int H = a.H, HC = a.H * a.C;
  int hf[FPL];
  feature_heads<FPL>(hf, lane, HC, a.C);
  float as[FPL], ad[FPL];
#pragma unroll
  for (int i = 0; i < FPL; ++i) {
    const int f = lane + 64 * i;
    const int c = f - hf[i] * a.C;
    as[i] = f < HC ? a.a[(int64_t)hf[i] * 2 * a.C + c] : 0.0f;
    ad[i] = f < HC ? a.a[(int64_t)hf[i] * 2 * a.C + a.C + c] : 0.0f;
  }
  for (int64_t row = wave0; row < a.n; row += nwaves) {
    float ps[FPL], pd[FPL];
#pragma unroll
    for (int i = 0; i < FPL; ++i) {
      const int f = lane + 64 * i;
      const float x = f < HC ? a.Hp[row * a.ldh + f] : 0.0f;
      ps[i] = __fmul_rn(x, as[i]);
      pd[i] = __fmul_rn(x, ad[i]);
    }
    const float ss = head_dots<FPL>(ps, hf, H, a.C, lane);
    const float sd = head_dots<FPL>(pd, hf, H, a.C, lane);
    if (lane < H) {
      a.s_src[row * H + lane] = ss;
      a.s_dst[row * H + lane] = sd;
    }
  }
}

// ----------------------------------------------- softmax + weighted gather
struct FwdArgs {
  int64_t n_rows;
  int H, C, act;
  const int64_t *rowptr;
  const int32_t *col;
  const float *s_row, *s_col, *alpha_in, *mask, *Hp;
  int64_t ldh;
  float *Y;
  int64_t ldy;
  float *alpha;
};

// GATHER: Y rows as well (mgcn_att_fwd); else alpha only (mgcn_edge_softmax)
template <int FPL, bool GATHER>
__global__ __launch_bounds__(kAttThreads) void att_fwd_kernel(FwdArgs a) {
  constexpr int U = gather_unroll<FPL>();
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = blockIdx.x * (int64_t)kAttWaves + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kAttWaves;
  const int H = a.H, G = 64 / a.H, HC = a.H * a.C;
  const int h = lane % H, kl = lane / H;
  const bool live = lane < G * H;
  int hf[FPL];
  feature_heads<FPL>(hf, lane, HC, GATHER ? a.C : 1);
  for (int64_t row = wave0; row < a.n_rows; row += nwaves) {
    const int64_t beg = a.rowptr[row], end = a.rowptr[row + 1];
    float m = -1e16f, denom = 1.0f, sr = 0.0f;
    if (a.alpha_in == nullptr) {
      sr = a.s_row[row * H + h];
      for (int64_t k0 = beg; k0 < end; k0 += G) {
        const int64_t k = k0 + kl;
        if (live && k < end)
          m = fmaxf(m, att_act(__fadd_rn(sr, a.s_col[(int64_t)a.col[k] * H + h]), a.act));
      }
      m = head_max(m, H, h);
      float sum = 0.0f;
      for (int64_t k0 = beg; k0 < end; k0 += G) {
        const int64_t k = k0 + kl;
        if (live && k < end) {
          const float e = att_act(__fadd_rn(sr, a.s_col[(int64_t)a.col[k] * H + h]), a.act);
          sum = __fadd_rn(sum, expf(__fsub_rn(e, m)));
        }
      }
      denom = __fadd_rn(head_sum(sum, H, h), 1e-16f);
    }
    float acc[FPL];
#pragma unroll
    for (int i = 0; i < FPL; ++i) acc[i] = 0.0f;
    for (int64_t k0 = beg; k0 < end; k0 += G) {
      const int64_t k = k0 + kl;
      float al = 0.0f;  // alpha' of this lane's (slot, head)
      if (live && k < end) {
        const int64_t idx = k * H + h;
        if (a.alpha_in != nullptr) {
          al = a.alpha_in[idx];
        } else {
          const float e = att_act(__fadd_rn(sr, a.s_col[(int64_t)a.col[k] * H + h]), a.act);
          al = __fdiv_rn(expf(__fsub_rn(e, m)), denom);
          a.alpha[idx] = al;
        }
        if (a.mask != nullptr) al = __fmul_rn(al, a.mask[idx]);
      }
      if (GATHER) {
        const int ns = (int)(end - k0 < G ? end - k0 : G);
        for (int kk = 0; kk < ns; kk += U) {
          float hp[U][FPL];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const bool on = kk + u < ns;
            const int64_t c = on ? __builtin_amdgcn_readfirstlane(a.col[k0 + kk + u]) : 0;
#pragma unroll
            for (int i = 0; i < FPL; ++i) {
              const int f = lane + 64 * i;
              hp[u][i] = (on && f < HC) ? a.Hp[c * a.ldh + f] : 0.0f;
            }
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {
            if (kk + u < ns) {
#pragma unroll
              for (int i = 0; i < FPL; ++i) {
                const float w = __shfl(al, (kk + u) * H + hf[i], 64);
                acc[i] = __fadd_rn(acc[i], __fmul_rn(w, hp[u][i]));
              }
            }
          }
        }
      }
    }
    if (GATHER) {
#pragma unroll
      for (int i = 0; i < FPL; ++i) {
        const int f = lane + 64 * i;
        if (f < HC) a.Y[row * a.ldy + f] = acc[i];
      }
    }
  }
}

// ------------------------------------------------- adjoint, by destination
struct BwdDstArgs {
  int64_t n_rows;
  int H, C, act, softmax;
  const int64_t *rowptr;
  const int32_t *col;
  const float *Hp;
  int64_t ldh;
  const float *dY;
  int64_t lddy;
  const float *alpha, *mask, *s_row, *s_col;
  float *dz, *ds_row;
};

template <int FPL>
__global__ __launch_bounds__(kAttThreads) void att_bwd_dst_kernel(BwdDstArgs a) {
  constexpr int U = gather_unroll<FPL>();
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = blockIdx.x * (int64_t)kAttWaves + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kAttWaves;
  const int H = a.H, G = 64 / a.H, HC = a.H * a.C;
  const int h = lane % H, kl = lane / H;
  const bool live = lane < G * H;
  int hf[FPL];
  feature_heads<FPL>(hf, lane, HC, a.C);
  for (int64_t row = wave0; row < a.n_rows; row += nwaves) {
    float dy[FPL];
#pragma unroll
    for (int i = 0; i < FPL; ++i) {
      const int f = lane + 64 * i;
      dy[i] = f < HC ? a.dY[row * a.lddy + f] : 0.0f;
    }
    const int64_t beg = a.rowptr[row], end = a.rowptr[row + 1];
    float S = 0.0f;  // lane hh < H: sum_k alpha dalpha of head hh
    for (int64_t k0 = beg; k0 < end; k0 += U) {
      float hp[U][FPL], ml[U], al[U];  // ml / al: lane hh < H, the slot's mask / alpha of head hh
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool on = k0 + u < end;
        const int64_t c = on ? __builtin_amdgcn_readfirstlane(a.col[k0 + u]) : 0;
#pragma unroll
        for (int i = 0; i < FPL; ++i) {
          const int f = lane + 64 * i;
          hp[u][i] = (on && f < HC) ? a.Hp[c * a.ldh + f] : 0.0f;
        }
        const bool mine_on = on && lane < H;
        ml[u] = (mine_on && a.mask != nullptr) ? a.mask[(k0 + u) * H + lane] : 1.0f;
        al[u] = (mine_on && a.softmax) ? a.alpha[(k0 + u) * H + lane] : 0.0f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k0 + u < end) {
#pragma unroll
          for (int i = 0; i < FPL; ++i) hp[u][i] = __fmul_rn(dy[i], hp[u][i]);
          const float mine = head_dots<FPL>(hp[u], hf, H, a.C, lane);
          if (lane < H) {
            const float d = a.mask != nullptr ? __fmul_rn(mine, ml[u]) : mine;
            a.dz[(k0 + u) * H + lane] = d;
            if (a.softmax) S = __fadd_rn(S, __fmul_rn(al[u], d));
          }
        }
      }
    }
    if (a.softmax) {
      // the dalpha entries above are re-read by other lanes of this wave
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      const float Sh = __shfl(S, h, 64);
      const float sr = a.s_row[row * H + h];
      float part = 0.0f;
      for (int64_t k0 = beg; k0 < end; k0 += G) {
        const int64_t k = k0 + kl;
        if (live && k < end) {
          const int64_t idx = k * H + h;
          const float z = __fadd_rn(sr, a.s_col[(int64_t)a.col[k] * H + h]);
          const float de = __fmul_rn(a.alpha[idx], __fsub_rn(a.dz[idx], Sh));
          const float v = __fmul_rn(de, att_act_grad(z, a.act));
          a.dz[idx] = v;
          part = __fadd_rn(part, v);
        }
      }
      const float tot = head_sum(part, H, h);
      if (lane < H) a.ds_row[row * H + lane] = tot;
    }
  }
}

// ------------------------------------------------------ adjoint, by source
struct BwdSrcArgs {
  int64_t n_rows;
  int H, C, act, softmax;
  const int64_t *rowptr;
  const int32_t *col, *slot;
  const float *dY;
  int64_t lddy;
  const float *alpha, *mask;
  float *dz;
  const float *s_row, *s_col, *a, *ds_dst;
  float *ds_src, *dHp;
  int64_t lddh;
};

template <int FPL>
__global__ __launch_bounds__(kAttThreads) void att_bwd_src_kernel(BwdSrcArgs a) {
  constexpr int U = gather_unroll<FPL>();
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = blockIdx.x * (int64_t)kAttWaves + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kAttWaves;
  const int H = a.H, G = 64 / a.H, HC = a.H * a.C;
  const int h = lane % H, kl = lane / H;
  const bool live = lane < G * H;
  int hf[FPL];
  feature_heads<FPL>(hf, lane, HC, a.C);
  for (int64_t row = wave0; row < a.n_rows; row += nwaves) {
    const int64_t beg = a.rowptr[row], end = a.rowptr[row + 1];
    float acc[FPL];
#pragma unroll
    for (int i = 0; i < FPL; ++i) acc[i] = 0.0f;
    // lane hh < H: softmax ? sum_k alpha dalpha : sum_k dz (= ds_src) of head hh
    float S = 0.0f;
    for (int64_t k0 = beg; k0 < end; k0 += U) {
      float dy[U][FPL], w[U][FPL], dzl[U], all[U];  // dzl / all: lane hh < H, the slot's dz / alpha
      int64_t fs[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool on = k0 + u < end;
        const int64_t c = on ? __builtin_amdgcn_readfirstlane(a.col[k0 + u]) : 0;
        fs[u] = on ? __builtin_amdgcn_readfirstlane(a.slot[k0 + u]) : 0;
#pragma unroll
        for (int i = 0; i < FPL; ++i) {
          const int f = lane + 64 * i;
          const bool ld = on && f < HC;
          dy[u][i] = ld ? a.dY[c * a.lddy + f] : 0.0f;
          w[u][i] = ld ? a.alpha[fs[u] * H + hf[i]] : 0.0f;
          if (a.mask != nullptr) w[u][i] = ld ? __fmul_rn(w[u][i], a.mask[fs[u] * H + hf[i]]) : 0.0f;
        }
        const bool mine_on = on && lane < H;
        dzl[u] = mine_on ? a.dz[fs[u] * H + lane] : 0.0f;
        all[u] = (mine_on && a.softmax) ? a.alpha[fs[u] * H + lane] : 0.0f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k0 + u < end) {
#pragma unroll
          for (int i = 0; i < FPL; ++i) acc[i] = __fadd_rn(acc[i], __fmul_rn(w[u][i], dy[u][i]));
          if (lane < H) S = __fadd_rn(S, a.softmax ? __fmul_rn(all[u], dzl[u]) : dzl[u]);
        }
      }
    }
    float dsv = S;  // lane hh < H: ds_src[row, hh]
    if (a.softmax) {
      const float Sh = __shfl(S, h, 64);
      const float sr = a.s_row[row * H + h];
      float part = 0.0f;
      for (int64_t k0 = beg; k0 < end; k0 += G) {
        const int64_t k = k0 + kl;
        if (live && k < end) {
          const int64_t idx = (int64_t)a.slot[k] * H + h;
          const float z = __fadd_rn(sr, a.s_col[(int64_t)a.col[k] * H + h]);
          const float de = __fmul_rn(a.alpha[idx], __fsub_rn(a.dz[idx], Sh));
          const float v = __fmul_rn(de, att_act_grad(z, a.act));
          a.dz[idx] = v;
          part = __fadd_rn(part, v);
        }
      }
      dsv = head_sum(part, H, h);
    }
    if (lane < H) a.ds_src[row * H + lane] = dsv;
#pragma unroll
    for (int i = 0; i < FPL; ++i) {
      const int f = lane + 64 * i;
      const int hh = hf[i], c = f - hf[i] * a.C;
      const float ds = __shfl(dsv, hh, 64);
      if (f < HC) {
        float v = __fadd_rn(acc[i], __fmul_rn(ds, a.a[(int64_t)hh * 2 * a.C + c]));
        if (a.ds_dst != nullptr)
          v = __fadd_rn(v, __fmul_rn(a.ds_dst[row * H + hh], a.a[(int64_t)hh * 2 * a.C + a.C + c]));
        a.dHp[row * a.lddh + f] = v;
      }
    }
  }
}

// ------------------------------- 'out': ds_dst and its term of dHp, by row
__global__ __launch_bounds__(kAttThreads) void att_dst_fold_kernel(
    int64_t n_rows, int H, int C, const int64_t *__restrict__ rowptr, const float *__restrict__ dz,
    const float *__restrict__ av, float *__restrict__ ds_dst, float *__restrict__ dHp,
    int64_t lddh) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = blockIdx.x * (int64_t)kAttWaves + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kAttWaves;
  const int G = 64 / H, HC = H * C;
  const int h = lane % H, kl = lane / H;
  const bool live = lane < G * H;
  for (int64_t row = wave0; row < n_rows; row += nwaves) {
    const int64_t beg = rowptr[row], end = rowptr[row + 1];
    float part = 0.0f;
    for (int64_t k0 = beg; k0 < end; k0 += G) {
      const int64_t k = k0 + kl;
      if (live && k < end) part = __fadd_rn(part, dz[k * H + h]);
    }
    const float tot = head_sum(part, H, h);
    if (lane < H) ds_dst[row * H + lane] = tot;
    for (int f0 = 0; f0 < HC; f0 += 64) {
      const int f = f0 + lane;
      const int hh = f < HC ? f / C : 0, c = f - hh * C;
      const float ds = __shfl(tot, hh, 64);
      if (f < HC) {
        float *p = dHp + row * lddh + f;
        *p = __fadd_rn(*p, __fmul_rn(ds, av[(int64_t)hh * 2 * C + C + c]));
      }
    }
  }
}

unsigned att_grid(int64_t n_rows) {
  int64_t blocks = (n_rows + kAttWaves - 1) / kAttWaves;
  if (blocks > 4096) blocks = 4096;
  return (unsigned)blocks;
}

#define ATT_DISPATCH(HC, CALL)          \
  do {                                  \
    const int fpl_ = ((HC) + 63) / 64;  \
    if (fpl_ <= 1) CALL(1);             \
    else if (fpl_ <= 2) CALL(2);        \
    else if (fpl_ <= 4) CALL(4);        \
    else if (fpl_ <= 8) CALL(8);        \
    else CALL(16);                      \
  } while (0)

}  // namespace
}  // namespace mgcn

using namespace mgcn;

// the supported range, checked on the host before any launch
#define ATT_REQUIRE_SHAPE(fn, n_rows, nnz, H, C)                                              \
  do {                                                                                        \
    MGCN_REQUIRE((n_rows) >= 0 && (nnz) >= 0, fn ": negative size");                          \
    MGCN_REQUIRE((H) >= 1 && (H) <= 16, fn ": need 1 <= H <= 16 (H = %d)", (int)(H));          \
    MGCN_REQUIRE((C) >= 1 && (int64_t)(H) * (C) <= 1024,                                      \
                 fn ": need C >= 1 and H C <= 1024 (H = %d, C = %d)", (int)(H), (int)(C));     \
    MGCN_REQUIRE((int64_t)(nnz) * (H) < ((int64_t)1 << 31), fn ": need nnz H < 2^31");         \
  } while (0)

#define ATT_ACT_OK(fn, act) \
  MGCN_REQUIRE((act) >= MGCN_ATT_ACT_NONE && (act) <= MGCN_ATT_ACT_RELU, fn ": bad act %d", act)

extern "C" int mgcn_att_scores(int64_t n, int32_t H, int32_t C, const float *Hp, int64_t ldh,
                               const float *a, float *s_src, float *s_dst, void *stream) {
  clear_error();
  ATT_REQUIRE_SHAPE("mgcn_att_scores", n, 0, H, C);
  if (n == 0) return MGCN_OK;
  MGCN_REQUIRE(Hp && a && s_src && s_dst, "mgcn_att_scores: null array");
  MGCN_REQUIRE(ldh >= (int64_t)H * C, "mgcn_att_scores: leading dimension too small");
  ScoreArgs k{n, H, C, Hp, ldh, a, s_src, s_dst};
  hipStream_t s = as_stream(stream);
#define CALL(FPL) \
  hipLaunchKernelGGL((att_scores_kernel<FPL>), dim3(att_grid(n)), dim3(kAttThreads), 0, s, k)
  ATT_DISPATCH(H * C, CALL);
#undef CALL
  return check_launch("att_scores_kernel");
}

extern "C" int mgcn_att_fwd(int64_t n_rows, int64_t nnz, int32_t H, int32_t C,
                            const int64_t *rowptr, const int32_t *col, const float *s_row,
                            const float *s_col, int act, const float *alpha_in,
                            const float *mask, const float *Hp, int64_t ldh, float *Y,
                            int64_t ldy, float *alpha, void *stream) {
  clear_error();
  ATT_REQUIRE_SHAPE("mgcn_att_fwd", n_rows, nnz, H, C);
  ATT_ACT_OK("mgcn_att_fwd", act);
  if (n_rows == 0) return MGCN_OK;
  MGCN_REQUIRE(rowptr && Hp && Y, "mgcn_att_fwd: null array");
  MGCN_REQUIRE(nnz == 0 || col, "mgcn_att_fwd: null col");
  MGCN_REQUIRE(alpha_in != nullptr || (s_row && s_col && (alpha || nnz == 0)),
               "mgcn_att_fwd: need alpha_in, or s_row / s_col / alpha");
  MGCN_REQUIRE(ldh >= (int64_t)H * C && ldy >= (int64_t)H * C,
               "mgcn_att_fwd: leading dimension too small");
  FwdArgs k{n_rows, H, C, act, rowptr, col, s_row, s_col, alpha_in, mask, Hp, ldh, Y, ldy, alpha};
  hipStream_t s = as_stream(stream);
#define CALL(FPL)                                                                          \
  hipLaunchKernelGGL((att_fwd_kernel<FPL, true>), dim3(att_grid(n_rows)), dim3(kAttThreads), \
                     0, s, k)
  ATT_DISPATCH(H * C, CALL);
#undef CALL
  return check_launch("att_fwd_kernel");
}

extern "C" int mgcn_edge_softmax(int64_t n_rows, int64_t nnz, int32_t H, const int64_t *rowptr,
                                 const int32_t *col, const float *s_row, const float *s_col,
                                 int act, float *alpha, void *stream) {
  clear_error();
  ATT_REQUIRE_SHAPE("mgcn_edge_softmax", n_rows, nnz, H, 1);
  ATT_ACT_OK("mgcn_edge_softmax", act);
  if (n_rows == 0 || nnz == 0) return MGCN_OK;
  MGCN_REQUIRE(rowptr && col && s_row && s_col && alpha, "mgcn_edge_softmax: null array");
  FwdArgs k{n_rows, H, 1, act, rowptr, col, s_row, s_col, nullptr, nullptr, nullptr, 0,
            nullptr, 0, alpha};
  hipLaunchKernelGGL((att_fwd_kernel<1, false>), dim3(att_grid(n_rows)), dim3(kAttThreads), 0,
                     as_stream(stream), k);
  return check_launch("att_fwd_kernel (softmax)");
}

extern "C" int mgcn_att_bwd_dst(int64_t n_rows, int64_t nnz, int32_t H, int32_t C,
                                const int64_t *rowptr, const int32_t *col, const float *Hp,
                                int64_t ldh, const float *dY, int64_t lddy, const float *alpha,
                                const float *mask, const float *s_row, const float *s_col,
                                int act, int softmax, float *dz, float *ds_row, void *stream) {
  clear_error();
  ATT_REQUIRE_SHAPE("mgcn_att_bwd_dst", n_rows, nnz, H, C);
  ATT_ACT_OK("mgcn_att_bwd_dst", act);
  if (n_rows == 0) return MGCN_OK;
  MGCN_REQUIRE(rowptr && Hp && dY, "mgcn_att_bwd_dst: null array");
  MGCN_REQUIRE(nnz == 0 || (col && dz), "mgcn_att_bwd_dst: null col / dz");
  MGCN_REQUIRE(!softmax || (ds_row && s_row && s_col && (alpha || nnz == 0)),
               "mgcn_att_bwd_dst: the softmax adjoint needs alpha, s_row, s_col, ds_row");
  MGCN_REQUIRE(ldh >= (int64_t)H * C && lddy >= (int64_t)H * C,
               "mgcn_att_bwd_dst: leading dimension too small");
  BwdDstArgs k{n_rows, H, C, act, softmax ? 1 : 0, rowptr, col, Hp, ldh, dY, lddy,
               alpha, mask, s_row, s_col, dz, ds_row};
  hipStream_t s = as_stream(stream);
#define CALL(FPL)                                                                            \
  hipLaunchKernelGGL((att_bwd_dst_kernel<FPL>), dim3(att_grid(n_rows)), dim3(kAttThreads), 0, \
                     s, k)
  ATT_DISPATCH(H * C, CALL);
#undef CALL
  return check_launch("att_bwd_dst_kernel");
}

extern "C" int mgcn_att_bwd_src(int64_t n_rows, int64_t nnz, int32_t H, int32_t C,
                                const int64_t *rowptr_t, const int32_t *col_t,
                                const int32_t *slot_map, const float *dY, int64_t lddy,
                                const float *alpha, const float *mask, float *dz,
                                const float *s_row, const float *s_col, int act, int softmax,
                                const float *a, const float *ds_dst, float *ds_src, float *dHp,
                                int64_t lddh, void *stream) {
  clear_error();
  ATT_REQUIRE_SHAPE("mgcn_att_bwd_src", n_rows, nnz, H, C);
  ATT_ACT_OK("mgcn_att_bwd_src", act);
  if (n_rows == 0) return MGCN_OK;
  MGCN_REQUIRE(rowptr_t && dY && a && ds_src && dHp, "mgcn_att_bwd_src: null array");
  MGCN_REQUIRE(nnz == 0 || (col_t && slot_map && alpha && dz),
               "mgcn_att_bwd_src: null col / slot_map / alpha / dz");
  MGCN_REQUIRE(!softmax || (s_row && s_col),
               "mgcn_att_bwd_src: the softmax adjoint needs s_row, s_col");
  MGCN_REQUIRE(lddy >= (int64_t)H * C && lddh >= (int64_t)H * C,
               "mgcn_att_bwd_src: leading dimension too small");
  BwdSrcArgs k{n_rows, H, C, act, softmax ? 1 : 0, rowptr_t, col_t, slot_map, dY, lddy,
               alpha, mask, dz, s_row, s_col, a, ds_dst, ds_src, dHp, lddh};
  hipStream_t s = as_stream(stream);
#define CALL(FPL)                                                                            \
  hipLaunchKernelGGL((att_bwd_src_kernel<FPL>), dim3(att_grid(n_rows)), dim3(kAttThreads), 0, \
                     s, k)
  ATT_DISPATCH(H * C, CALL);
#undef CALL
  return check_launch("att_bwd_src_kernel");
}

extern "C" int mgcn_att_dst_fold(int64_t n_rows, int64_t nnz, int32_t H, int32_t C,
                                 const int64_t *rowptr, const float *dz, const float *a,
                                 float *ds_dst, float *dHp, int64_t lddh, void *stream) {
  clear_error();
  ATT_REQUIRE_SHAPE("mgcn_att_dst_fold", n_rows, nnz, H, C);
  if (n_rows == 0) return MGCN_OK;
  MGCN_REQUIRE(rowptr && a && ds_dst && dHp, "mgcn_att_dst_fold: null array");
  MGCN_REQUIRE(nnz == 0 || dz, "mgcn_att_dst_fold: null dz");
  MGCN_REQUIRE(lddh >= (int64_t)H * C, "mgcn_att_dst_fold: leading dimension too small");
  hipLaunchKernelGGL(att_dst_fold_kernel, dim3(att_grid(n_rows)), dim3(kAttThreads), 0,
                     as_stream(stream), n_rows, (int)H, (int)C, rowptr, dz, a, ds_dst, dHp, lddh);
  return check_launch("att_dst_fold_kernel");
}
