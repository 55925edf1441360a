// Device code shared by attention.hip (soft attention) and
// hard_attention.hip (Gumbel-softmax / argmax hard attention): the lane-layout
// helpers, the softmax + gather kernel and the two adjoint kernels, templated
// on their argument struct.  The hard structs add noise / temperature; with
// the soft structs every `if constexpr (A::kHard)` branch drops out and the
// kernels are the soft ones, source path for source path.  The work split is
// described at the top of attention.hip.
//
// Feature rows (Hp, Y, dY, dHp) have the element type R of the argument
// struct: float, or bf16 bit patterns as uint16_t (the mgcn_*_bf16 entries).
// A bf16 element is widened to fp32 exactly at its load (row_ld), every value
// is then formed by the fp32 kernel's operations in its order, and a bf16
// output element is rounded once, to nearest even, at its store (row_st): the
// fp32 outputs (scores, alpha, dz, ds) have the bits of the fp32 entry on the
// upcast rows, the bf16 outputs those bits rounded.  With R = float row_ld /
// row_st are the load / store the fp32 kernels always had.  Scores, alpha,
// mask, noise, dz, ds and the attention vector are fp32 with either R.
#pragma once

#include "mgcn_internal.h"

namespace mgcn {
namespace {

constexpr int kAttWaves = 4;
constexpr int kAttThreads = 64 * kAttWaves;

// Element i of a row array as fp32, 0 when !on.  fp32: the predicated load
// the kernels always had.  bf16: the same predicated load of 2 bytes, then
// the exact widening (bits << 16).  The value of the !on side is a zero the
// compiler cannot see through (an empty asm on a register): with a literal 0
// it moves the shift into the predicated block, where the shift waits for its
// own load, and the loads of a gather batch no longer overlap.
__device__ inline float row_ld(bool on, const float *rows, int64_t i) {
  return on ? rows[i] : 0.0f;
}
__device__ inline float row_ld(bool on, const uint16_t *rows, int64_t i) {
  uint32_t zero = 0;
  asm("" : "+s"(zero));
  const uint32_t r = on ? (uint32_t)rows[i] : zero;
  return __uint_as_float(r << 16);
}
__device__ inline void row_st(float *p, float v) { *p = v; }
__device__ inline void row_st(uint16_t *p, float v) {  // v_cvt_pk_bf16_f32: RNE
  *p = __builtin_bit_cast(uint16_t, static_cast<__bf16>(v));
}

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

// ----------------------------------------------- softmax + weighted gather
template <class R>
struct FwdArgsT {
  using Row = R;
  int64_t n_rows;
  int H, C, act;
  const int64_t *rowptr;
  const int32_t *col;
  const float *s_row, *s_col, *alpha_in, *mask;
  const R *Hp;
  int64_t ldh;
  R *Y;
  int64_t ldy;
  float *alpha;
  static constexpr bool kHard = false;
  static constexpr bool kSched = false;
};
using FwdArgs = FwdArgsT<float>;

// Hard attention (graph_hard_attention.py:96-110): Gumbel noise and a
// temperature inside the logit, l = (act(z) + noise) / T; noise is [nnz, H]
// in the slot order of the view walked, NULL = zeros.
template <class R>
struct HardFwdArgsT : FwdArgsT<R> {
  const float *noise;
  float temperature;
  static constexpr bool kHard = true;
};
using HardFwdArgs = HardFwdArgsT<float>;

// Any argument struct B of the three kernels below with a row schedule
// (mgcn_row_schedule): the kernel walks the rows order[n_heavy, n_rows) in
// that order instead of [0, n_rows); the heavy rows order[0, n_heavy) are
// attention_heavy.hip's.  Without it (kSched false) the kernels are the code
// they always were.
template <class B>
struct SchedArgsT : B {
  const int32_t *order;
  int64_t n_heavy;
  static constexpr bool kSched = true;
};

// The logit of (slot, head) idx from its pre-activation z.
template <bool HARD>
__device__ inline float att_logit(float z, int act, const float *noise, float T, int64_t idx) {
  const float e = att_act(z, act);
  if constexpr (HARD)
    return __fdiv_rn(__fadd_rn(e, noise != nullptr ? noise[idx] : 0.0f), T);
  else
    return e;
}

// The softmax adjoint de through the 1 / T of the logit (autograd walks
// (act(z) + g) / T backwards: the divide first, then act').
template <bool HARD>
__device__ inline float att_dlogit(float de, float T) {
  if constexpr (HARD)
    return __fdiv_rn(de, T);
  else
    return de;
}

// GATHER: Y rows as well (mgcn_att_fwd); else alpha only (mgcn_edge_softmax)
template <int FPL, bool GATHER, class A = FwdArgs>
__global__ __launch_bounds__(kAttThreads) void att_fwd_kernel(A a) {
  constexpr int U = gather_unroll<FPL>();
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = blockIdx.x * (int64_t)kAttWaves + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kAttWaves;
  const int H = a.H, G = 64 / a.H, HC = a.H * a.C;
  const int h = lane % H, kl = lane / H;
  const bool live = lane < G * H;
  int hf[FPL];
  feature_heads<FPL>(hf, lane, HC, GATHER ? a.C : 1);
  const float *noise = nullptr;
  float T = 1.0f;
  if constexpr (A::kHard) {
    noise = a.noise;
    T = a.temperature;
  }
  int64_t n_work = a.n_rows;
  if constexpr (A::kSched) n_work -= a.n_heavy;
  for (int64_t ri = wave0; ri < n_work; ri += nwaves) {
    int64_t row = ri;
    if constexpr (A::kSched) row = a.order[a.n_heavy + ri];
    const int64_t beg = a.rowptr[row], end = a.rowptr[row + 1];
    float m = -1e16f, denom = 1.0f, sr = 0.0f;
    if (a.alpha_in == nullptr) {
      sr = a.s_row[row * H + h];
      for (int64_t k0 = beg; k0 < end; k0 += G) {
        const int64_t k = k0 + kl;
        if (live && k < end)
          m = fmaxf(m, att_logit<A::kHard>(__fadd_rn(sr, a.s_col[(int64_t)a.col[k] * H + h]),
                                           a.act, noise, T, k * H + h));
      }
      m = head_max(m, H, h);
      float sum = 0.0f;
      for (int64_t k0 = beg; k0 < end; k0 += G) {
        const int64_t k = k0 + kl;
        if (live && k < end) {
          const float e = att_logit<A::kHard>(
              __fadd_rn(sr, a.s_col[(int64_t)a.col[k] * H + h]), a.act, noise, T, k * H + h);
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
          const float e = att_logit<A::kHard>(
              __fadd_rn(sr, a.s_col[(int64_t)a.col[k] * H + h]), a.act, noise, T, idx);
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
              hp[u][i] = row_ld(on && f < HC, a.Hp, c * a.ldh + f);
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
        if (f < HC) row_st(a.Y + row * a.ldy + f, acc[i]);
      }
    }
  }
}

// ------------------------------------------------- adjoint, by destination
template <class R>
struct BwdDstArgsT {
  using Row = R;
  int64_t n_rows;
  int H, C, act, softmax;
  const int64_t *rowptr;
  const int32_t *col;
  const R *Hp;
  int64_t ldh;
  const R *dY;
  int64_t lddy;
  const float *alpha, *mask, *s_row, *s_col;
  float *dz, *ds_row;
  static constexpr bool kHard = false;
  static constexpr bool kSched = false;
};
using BwdDstArgs = BwdDstArgsT<float>;

template <class R>
struct HardBwdDstArgsT : BwdDstArgsT<R> {
  float temperature;
  static constexpr bool kHard = true;
};
using HardBwdDstArgs = HardBwdDstArgsT<float>;

template <int FPL, class A = BwdDstArgs>
__global__ __launch_bounds__(kAttThreads) void att_bwd_dst_kernel(A a) {
  constexpr int U = gather_unroll<FPL>();
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = blockIdx.x * (int64_t)kAttWaves + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kAttWaves;
  const int H = a.H, G = 64 / a.H, HC = a.H * a.C;
  const int h = lane % H, kl = lane / H;
  const bool live = lane < G * H;
  int hf[FPL];
  feature_heads<FPL>(hf, lane, HC, a.C);
  float T = 1.0f;
  if constexpr (A::kHard) T = a.temperature;
  int64_t n_work = a.n_rows;
  if constexpr (A::kSched) n_work -= a.n_heavy;
  for (int64_t ri = wave0; ri < n_work; ri += nwaves) {
    int64_t row = ri;
    if constexpr (A::kSched) row = a.order[a.n_heavy + ri];
    float dy[FPL];
#pragma unroll
    for (int i = 0; i < FPL; ++i) {
      const int f = lane + 64 * i;
      dy[i] = row_ld(f < HC, a.dY, row * a.lddy + f);
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
          hp[u][i] = row_ld(on && f < HC, a.Hp, c * a.ldh + f);
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
          const float v = __fmul_rn(att_dlogit<A::kHard>(de, T), att_act_grad(z, a.act));
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
template <class R>
struct BwdSrcArgsT {
  using Row = R;
  int64_t n_rows;
  int H, C, act, softmax;
  const int64_t *rowptr;
  const int32_t *col, *slot;
  const R *dY;
  int64_t lddy;
  const float *alpha, *mask;
  float *dz;
  const float *s_row, *s_col, *a, *ds_dst;
  float *ds_src;
  R *dHp;
  int64_t lddh;
  static constexpr bool kHard = false;
  static constexpr bool kPark = false;
  static constexpr bool kSched = false;
};
using BwdSrcArgs = BwdSrcArgsT<float>;

// bf16 rows, att_dir 'out': mgcn_att_dst_fold adds a term to dHp after this
// kernel, and a bf16 row must be rounded once.  With dHp_f32 given
// ([n_rows, H C] fp32, compact) the unrounded row is parked there and dHp is
// left to the fold, which adds its term in fp32 and rounds at its store.
struct BwdSrcArgsBf16 : BwdSrcArgsT<uint16_t> {
  float *dHp_f32;
  static constexpr bool kPark = true;
};

template <class B>
struct HardBwdSrcArgsT : B {
  float temperature;
  static constexpr bool kHard = true;
};
using HardBwdSrcArgs = HardBwdSrcArgsT<BwdSrcArgs>;

template <int FPL, class A = BwdSrcArgs>
__global__ __launch_bounds__(kAttThreads) void att_bwd_src_kernel(A a) {
  constexpr int U = gather_unroll<FPL>();
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = blockIdx.x * (int64_t)kAttWaves + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kAttWaves;
  const int H = a.H, G = 64 / a.H, HC = a.H * a.C;
  const int h = lane % H, kl = lane / H;
  const bool live = lane < G * H;
  int hf[FPL];
  feature_heads<FPL>(hf, lane, HC, a.C);
  float T = 1.0f;
  if constexpr (A::kHard) T = a.temperature;
  int64_t n_work = a.n_rows;
  if constexpr (A::kSched) n_work -= a.n_heavy;
  for (int64_t ri = wave0; ri < n_work; ri += nwaves) {
    int64_t row = ri;
    if constexpr (A::kSched) row = a.order[a.n_heavy + ri];
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
          dy[u][i] = row_ld(ld, a.dY, c * a.lddy + f);
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
          const float v = __fmul_rn(att_dlogit<A::kHard>(de, T), att_act_grad(z, a.act));
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
        bool parked = false;
        if constexpr (A::kPark) {
          parked = a.dHp_f32 != nullptr;
          if (parked) a.dHp_f32[row * HC + f] = v;
        }
        if (!parked) row_st(a.dHp + row * a.lddh + f, v);
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

// the supported range, checked on the host before any launch
// (fn: the C entry's name, a const char *: the fp32 and the bf16 entry share
// one templated body)
#define ATT_REQUIRE_SHAPE(fn, n_rows, nnz, H, C)                                               \
  do {                                                                                         \
    MGCN_REQUIRE((n_rows) >= 0 && (nnz) >= 0, "%s: negative size", fn);                        \
    MGCN_REQUIRE((H) >= 1 && (H) <= 16, "%s: need 1 <= H <= 16 (H = %d)", fn, (int)(H));        \
    MGCN_REQUIRE((C) >= 1 && (int64_t)(H) * (C) <= 1024,                                       \
                 "%s: need C >= 1 and H C <= 1024 (H = %d, C = %d)", fn, (int)(H), (int)(C));   \
    MGCN_REQUIRE((int64_t)(nnz) * (H) < ((int64_t)1 << 31), "%s: need nnz H < 2^31", fn);       \
  } while (0)

#define ATT_ACT_OK(fn, act) \
  MGCN_REQUIRE((act) >= MGCN_ATT_ACT_NONE && (act) <= MGCN_ATT_ACT_RELU, "%s: bad act %d", fn, act)
