// Heavy rows of the fp32 attention launches, soft and hard (gfx950): the rows
// order[0, n_heavy) of a view's schedule (mgcn_row_schedule: degree > 128; the
// botnet graphs reach ~6.5k), which the wave-per-row kernels of attention.h
// walk by one wave each.  The mgcn_(h)att_*_sched entries send them to
// workgroups and the rows order[n_heavy, n_rows) to the wave kernels (the
// kernels of attention.h over a SchedArgsT argument struct).  Every output
// element keeps the bits the entry without a schedule gives it:
//
//  * what a (slot, head) contributes -- the logit, exp(e - m), alpha,
//    alpha mask, the per-slot head dots, de, v -- depends on the slot alone,
//    so any thread may form it; the row max is exact in any order;
//  * what a row sums is summed as the wave kernel's chains.  All threads of
//    the workgroup form a batch of terms in [slot, head] order into LDS
//    (staged()), barrier, and wave 0 alone runs the chains over the batch:
//    the "flat" sums (sum exp, ds) as lane (kl, h) adding the terms of slots
//    c G + kl, c = 0, 1, ..., then head_sum; the serial sums (S of the two
//    adjoints) as lane hh < H adding the row's terms of head hh one by one;
//  * the weighted gathers are one chain per feature in slot order:
//    producer waves form the products coef[slot, head of f] X[col, f] of a
//    batch of slots into one of two LDS buffers while the fold waves add the
//    other buffer's, one thread per feature (heavy_gather(); heavy.h's body
//    takes one coefficient per slot, attention needs one per slot and head).
//
// Forward / edge softmax: one workgroup per row (three staged passes -- max,
// sum exp, then alpha and coef = alpha mask in place -- and the gather).
// Adjoint by destination: the row's slots spread over the waves of several
// workgroups (the wave kernel's per-slot SDDMM, dz = mask dalpha' stored),
// then, under softmax, one workgroup per row: the S chain, the edge phase in
// place, ds_row.  Adjoint by source: one workgroup per row of the bwd view
// (coef and the S terms in one staged pass, for 'out' the softmax adjoint in
// place and ds_src, then the gather whose last step adds the two rank-one
// terms).  The first n_giant rows take 1024 threads and the large LDS budget,
// the others 256 threads and the small one, as the SpMM's and the gates'
// heavy launches.  Barriers only: no atomics, no hand-off between workgroups;
// separate launches are ordered by the stream.

#include "attention_entry.h"

namespace mgcn {
namespace {

constexpr int kStage = 4096;  // floats of LDS a staged() batch may take
constexpr int kStaticLds = 256;  // bytes kept out of the LDS budget for the kernels' static arrays

// A row's n = deg H terms, term(i) for i = (slot - beg) H + h, formed by all
// HB threads batch after batch into stage[]; wave 0 consumes each batch with
// use(stage, nb).  `chunk` (<= kStage) is a multiple of G H, so a batch starts
// on a chunk boundary of the flat layout and on a slot.  Ends on a barrier.
template <int HB, class Term, class Use>
__device__ __forceinline__ void staged(int n, int chunk, float *stage, Term term, Use use) {
  for (int i0 = 0; i0 < n; i0 += chunk) {
    const int nb = n - i0 < chunk ? n - i0 : chunk;
    for (int i = threadIdx.x; i < nb; i += HB) stage[i] = term(i0 + i);
    __syncthreads();
    if (threadIdx.x < 64) use(stage, nb);
    __syncthreads();
  }
}

// wave 0, flat layout: lane < GH adds stage[lane], stage[lane + GH], ... to acc
__device__ __forceinline__ void flat_add(float &acc, const float *stage, int nb, int GH, int lane) {
  constexpr int kB = 8;
  if (lane >= GH) return;
  int j = lane;
  for (; j + (kB - 1) * GH < nb; j += kB * GH) {
    float r[kB];
#pragma unroll
    for (int u = 0; u < kB; ++u) r[u] = stage[j + u * GH];
#pragma unroll
    for (int u = 0; u < kB; ++u) acc = __fadd_rn(acc, r[u]);
  }
  for (; j < nb; j += GH) acc = __fadd_rn(acc, stage[j]);
}

__device__ __forceinline__ void flat_max(float &acc, const float *stage, int nb, int GH, int lane) {
  if (lane >= GH) return;
  for (int j = lane; j < nb; j += GH) acc = fmaxf(acc, stage[j]);
}

// wave 0, serial: lane hh < H adds stage[hh], stage[H + hh], ... to acc
__device__ __forceinline__ void serial_add(float &acc, const float *stage, int nb, int H, int lane) {
  constexpr int kB = 8;
  if (lane >= H) return;
  int j = lane;
  for (; j + (kB - 1) * H < nb; j += kB * H) {
    float r[kB];
#pragma unroll
    for (int u = 0; u < kB; ++u) r[u] = stage[j + u * H];
#pragma unroll
    for (int u = 0; u < kB; ++u) acc = __fadd_rn(acc, r[u]);
  }
  for (; j < nb; j += H) acc = __fadd_rn(acc, stage[j]);
}

// out[f] = epi(f, sum_k coef[(beg + k) H + f / C] X[col[beg + k], f]), the sum
// one __fadd_rn chain per feature over k = 0 .. deg - 1 from 0: the wave
// kernels' acc.  Feature chunks of FC (<= 128); threads [0, 64 ceil(fc / 64))
// fold, the others produce; smem holds 2 FC (BE + 1) floats (the odd row
// stride keeps the producers' stores and the fold reads off shared banks).
// coef must be visible to the workgroup (a barrier after its stores).  Ends on
// a barrier.
struct NoEpi {
  __device__ __forceinline__ float operator()(int, float v) const { return v; }
};
template <int HB, class Epi = NoEpi>
__device__ __forceinline__ void heavy_gather(const int32_t *__restrict__ col, int64_t beg, int deg,
                                             const float *coef, int H, int C, const float *X,
                                             int64_t ldx, float *out, int FC, int BE,
                                             float *__restrict__ smem, Epi epi = Epi{}) {
  constexpr int kU = 4;  // gathers in flight per producer thread
  const int HC = H * C, BEp = BE + 1;
  const int t = threadIdx.x;
  const int nbatch = (deg + BE - 1) / BE;
  for (int f0 = 0; f0 < HC; f0 += FC) {
    const int fc = HC - f0 < FC ? HC - f0 : FC;
    const int fold = 64 * ((fc + 63) / 64);
    const int np = HB - fold, pt = t - fold;
    const int qe = np / fc, qf = np - qe * fc;  // a step of np pairs in (slot, feature)
    auto produce = [&](int b) {
      float *P = smem + (b & 1) * FC * BEp;
      const int64_t k0 = beg + (int64_t)b * BE;
      const int nb = deg - b * BE < BE ? deg - b * BE : BE;
      int e = pt / fc, f = pt - e * fc;  // pair pt, pt + np, ...: slot e, feature f0 + f
      while (e < nb) {
        float x[kU], w[kU];
        int off[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const bool on = e < nb;
          off[u] = on ? f * BEp + e : -1;
          const int64_t k = k0 + e;
          const int64_t c = on ? col[k] : 0;
          x[u] = on ? X[c * ldx + f0 + f] : 0.0f;
          w[u] = on ? coef[k * H + (f0 + f) / C] : 0.0f;
          e += qe;
          f += qf;
          if (f >= fc) {
            f -= fc;
            ++e;
          }
        }
#pragma unroll
        for (int u = 0; u < kU; ++u)
          if (off[u] >= 0) P[off[u]] = __fmul_rn(w[u], x[u]);
      }
    };
    float acc = 0.0f;
    if (pt >= 0 && nbatch > 0) produce(0);
    __syncthreads();
    for (int bi = 0; bi < nbatch; ++bi) {
      if (pt < 0) {
        if (t < fc) {
          constexpr int kB = 8;
          const float *pr = smem + (bi & 1) * FC * BEp + t * BEp;
          const int nb = deg - bi * BE < BE ? deg - bi * BE : BE;
          int e = 0;
          for (; e + kB <= nb; e += kB) {
            float r[kB];
#pragma unroll
            for (int u = 0; u < kB; ++u) r[u] = pr[e + u];
#pragma unroll
            for (int u = 0; u < kB; ++u) acc = __fadd_rn(acc, r[u]);
          }
          for (; e < nb; ++e) acc = __fadd_rn(acc, pr[e]);
        }
      } else if (bi + 1 < nbatch) {
        produce(bi + 1);
      }
      __syncthreads();
    }
    if (t < fc) out[f0 + t] = epi(f0 + t, acc);
  }
}

// ----------------------------------------------------------------- forward
// GATHER: Y rows as well; else alpha only (the edge softmax).
template <int HB, bool GATHER, class A>
__global__ __launch_bounds__(HB) void att_fwd_heavy_kernel(A a, const int32_t *rows, float *coef,
                                                           int FC, int BE) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ float shead[16];
  const int t = threadIdx.x, lane = t & 63;
  const int H = a.H, G = 64 / a.H, GH = G * H;
  const int h = lane % H;
  const int64_t row = rows[blockIdx.x];
  const int64_t beg = a.rowptr[row], end = a.rowptr[row + 1];
  const int deg = (int)(end - beg), n = deg * H;
  const int chunk = kStage / GH * GH;
  const int64_t base = beg * H;
  if (a.alpha_in == nullptr) {
    const float *noise = nullptr;
    float T = 1.0f;
    if constexpr (A::kHard) {
      noise = a.noise;
      T = a.temperature;
    }
    auto logit = [&](int i) {
      const int k = i / H, hh = i - k * H;
      const float z = __fadd_rn(a.s_row[row * H + hh], a.s_col[(int64_t)a.col[beg + k] * H + hh]);
      return att_logit<A::kHard>(z, a.act, noise, T, base + i);
    };
    float m = -1e16f;
    staged<HB>(n, chunk, smem, logit,
               [&](const float *st, int nb) { flat_max(m, st, nb, GH, lane); });
    if (t < 64) {
      m = head_max(m, H, h);
      if (lane < H) shead[lane] = m;
    }
    __syncthreads();
    float sum = 0.0f;
    staged<HB>(n, chunk, smem,
               [&](int i) {
                 const float p = expf(__fsub_rn(logit(i), shead[i % H]));
                 a.alpha[base + i] = p;  // parked: divided below
                 return p;
               },
               [&](const float *st, int nb) { flat_add(sum, st, nb, GH, lane); });
    if (t < 64) {
      const float denom = __fadd_rn(head_sum(sum, H, h), 1e-16f);
      if (lane < H) shead[lane] = denom;
    }
    __syncthreads();
    for (int i = t; i < n; i += HB) {
      const float al = __fdiv_rn(a.alpha[base + i], shead[i % H]);
      a.alpha[base + i] = al;
      if (GATHER) coef[base + i] = a.mask != nullptr ? __fmul_rn(al, a.mask[base + i]) : al;
    }
  } else if (GATHER) {
    for (int i = t; i < n; i += HB) {
      const float al = a.alpha_in[base + i];
      coef[base + i] = a.mask != nullptr ? __fmul_rn(al, a.mask[base + i]) : al;
    }
  }
  if (GATHER) {
    __syncthreads();  // the row's coef
    heavy_gather<HB>(a.col, beg, deg, coef, H, a.C, a.Hp, a.ldh, a.Y + row * a.ldy, FC, BE, smem);
  }
}

// ------------------------------------------------- adjoint, by destination
// The per-slot part of att_bwd_dst_kernel for heavy row rows[blockIdx.x]: its
// groups of U slots by the waves along blockIdx.y.
template <int FPL, class A>
__global__ __launch_bounds__(kAttThreads) void att_bwd_dst_slots_kernel(A a, const int32_t *rows) {
  constexpr int U = gather_unroll<FPL>();
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = blockIdx.y * (int64_t)kAttWaves + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.y * kAttWaves;
  const int H = a.H, HC = a.H * a.C;
  const int64_t row = rows[blockIdx.x];
  const int64_t beg = a.rowptr[row], end = a.rowptr[row + 1];
  const int64_t n_groups = (end - beg + U - 1) / U;
  if (wave0 >= n_groups) return;
  int hf[FPL];
  feature_heads<FPL>(hf, lane, HC, a.C);
  float dy[FPL];
#pragma unroll
  for (int i = 0; i < FPL; ++i) {
    const int f = lane + 64 * i;
    dy[i] = row_ld(f < HC, a.dY, row * a.lddy + f);
  }
  for (int64_t g = wave0; g < n_groups; g += nwaves) {
    const int64_t k0 = beg + g * U;
    float hp[U][FPL], ml[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool on = k0 + u < end;
      const int64_t c = on ? __builtin_amdgcn_readfirstlane(a.col[k0 + u]) : 0;
#pragma unroll
      for (int i = 0; i < FPL; ++i) {
        const int f = lane + 64 * i;
        hp[u][i] = row_ld(on && f < HC, a.Hp, c * a.ldh + f);
      }
      ml[u] = (on && lane < H && a.mask != nullptr) ? a.mask[(k0 + u) * H + lane] : 1.0f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (k0 + u < end) {
#pragma unroll
        for (int i = 0; i < FPL; ++i) hp[u][i] = __fmul_rn(dy[i], hp[u][i]);
        const float mine = head_dots<FPL>(hp[u], hf, H, a.C, lane);
        if (lane < H)
          a.dz[(k0 + u) * H + lane] = a.mask != nullptr ? __fmul_rn(mine, ml[u]) : mine;
      }
    }
  }
}

// The softmax adjoint of heavy row rows[blockIdx.x] over the dz the slots
// kernel stored: S, the edge phase in place, ds_row.
template <class A>
__global__ __launch_bounds__(kAttThreads) void att_bwd_dst_row_kernel(A a, const int32_t *rows) {
  __shared__ float stage[kStage];
  __shared__ float shead[16];
  const int t = threadIdx.x, lane = t & 63;
  const int H = a.H, G = 64 / a.H, GH = G * H;
  const int h = lane % H;
  const int64_t row = rows[blockIdx.x];
  const int64_t beg = a.rowptr[row], end = a.rowptr[row + 1];
  const int deg = (int)(end - beg), n = deg * H;
  const int chunk = kStage / GH * GH;
  const int64_t base = beg * H;
  float T = 1.0f;
  if constexpr (A::kHard) T = a.temperature;
  float S = 0.0f;
  staged<kAttThreads>(n, chunk, stage,
                      [&](int i) { return __fmul_rn(a.alpha[base + i], a.dz[base + i]); },
                      [&](const float *st, int nb) { serial_add(S, st, nb, H, lane); });
  if (t < H) shead[t] = S;
  __syncthreads();
  float part = 0.0f;
  staged<kAttThreads>(n, chunk, stage,
                      [&](int i) {
                        const int k = i / H, hh = i - k * H;
                        const float z = __fadd_rn(a.s_row[row * H + hh],
                                                  a.s_col[(int64_t)a.col[beg + k] * H + hh]);
                        const float de =
                            __fmul_rn(a.alpha[base + i], __fsub_rn(a.dz[base + i], shead[hh]));
                        const float v =
                            __fmul_rn(att_dlogit<A::kHard>(de, T), att_act_grad(z, a.act));
                        a.dz[base + i] = v;
                        return v;
                      },
                      [&](const float *st, int nb) { flat_add(part, st, nb, GH, lane); });
  if (t < 64) {
    const float tot = head_sum(part, H, h);
    if (lane < H) a.ds_row[row * H + lane] = tot;
  }
}

// ------------------------------------------------------ adjoint, by source
// the wave kernel's epilogue on element f of the row: + ds_src a[:, :C], then
// + ds_dst a[:, C:]
struct BwdSrcEpi {
  const float *av, *ds /* LDS: ds_src of this row */, *ds_dst /* of this row, or NULL */;
  int C;
  __device__ __forceinline__ float operator()(int f, float v) const {
    const int hh = f / C, c = f - hh * C;
    v = __fadd_rn(v, __fmul_rn(ds[hh], av[(int64_t)hh * 2 * C + c]));
    if (ds_dst != nullptr) v = __fadd_rn(v, __fmul_rn(ds_dst[hh], av[(int64_t)hh * 2 * C + C + c]));
    return v;
  }
};

template <int HB, class A>
__global__ __launch_bounds__(HB) void att_bwd_src_heavy_kernel(A a, const int32_t *rows,
                                                               float *coef, int FC, int BE) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ float shead[16], sds[16];
  const int t = threadIdx.x, lane = t & 63;
  const int H = a.H, G = 64 / a.H, GH = G * H;
  const int h = lane % H;
  const int64_t row = rows[blockIdx.x];
  const int64_t beg = a.rowptr[row], end = a.rowptr[row + 1];
  const int deg = (int)(end - beg), n = deg * H;
  const int chunk = kStage / GH * GH;
  const int64_t base = beg * H;
  float T = 1.0f;
  if constexpr (A::kHard) T = a.temperature;
  float S = 0.0f;  // lane hh < H of wave 0: sum alpha dalpha, or sum dz = ds_src
  staged<HB>(n, chunk, smem,
             [&](int i) {
               const int k = i / H, hh = i - k * H;
               const int64_t idx = (int64_t)a.slot[beg + k] * H + hh;
               const float al = a.alpha[idx];
               coef[base + i] = a.mask != nullptr ? __fmul_rn(al, a.mask[idx]) : al;
               const float dzl = a.dz[idx];
               return a.softmax ? __fmul_rn(al, dzl) : dzl;
             },
             [&](const float *st, int nb) { serial_add(S, st, nb, H, lane); });
  if (a.softmax) {
    if (t < H) shead[t] = S;
    __syncthreads();
    float part = 0.0f;
    staged<HB>(n, chunk, smem,
               [&](int i) {
                 const int k = i / H, hh = i - k * H;
                 const int64_t idx = (int64_t)a.slot[beg + k] * H + hh;
                 const float z = __fadd_rn(a.s_row[row * H + hh],
                                           a.s_col[(int64_t)a.col[beg + k] * H + hh]);
                 const float de = __fmul_rn(a.alpha[idx], __fsub_rn(a.dz[idx], shead[hh]));
                 const float v = __fmul_rn(att_dlogit<A::kHard>(de, T), att_act_grad(z, a.act));
                 a.dz[idx] = v;
                 return v;
               },
               [&](const float *st, int nb) { flat_add(part, st, nb, GH, lane); });
    if (t < 64) S = head_sum(part, H, h);
  }
  if (t < H) {
    sds[t] = S;
    a.ds_src[row * H + t] = S;
  }
  __syncthreads();  // the row's coef (staged() ends on a barrier) and sds
  const BwdSrcEpi epi{a.a, sds, a.ds_dst != nullptr ? a.ds_dst + row * H : nullptr, a.C};
  heavy_gather<HB>(a.col, beg, deg, coef, H, a.C, a.dY, a.lddy, a.dHp + row * a.lddh, FC, BE, smem,
                   epi);
}

// ------------------------------------------------------------------- host
// the gather's launch shape: feature chunk FC, slot batch BE and the dynamic
// LDS (at least a staged() batch) out of `budget` bytes
struct GatherShape {
  int FC, BE;
  size_t lds;
};
GatherShape gather_shape(int HC, int budget) {
  budget -= kStaticLds;
  const int FC = HC < 128 ? HC : 128;
  int BE = budget / 4 / (2 * FC) - 1;
  if (BE > 1024) BE = 1024;
  BE &= ~1;  // BE + 1 odd
  if (BE < 2) BE = 2;
  size_t lds = sizeof(float) * (size_t)2 * FC * (BE + 1);
  if (lds < sizeof(float) * kStage) lds = sizeof(float) * kStage;
  return {FC, BE, lds};
}

constexpr int kMaxLds = 160 * 1024 - kStaticLds;  // dynamic LDS a heavy kernel may be given

template <int HB, bool GATHER, class A>
int launch_fwd_rows(const A &a, const int32_t *rows, int64_t n, float *coef, int budget,
                    hipStream_t st) {
  if (n <= 0) return MGCN_OK;
  const GatherShape g = gather_shape(GATHER ? a.H * a.C : 1, budget);
  static std::atomic<uint64_t> attr_set{0};
  if (int rc = allow_lds(reinterpret_cast<const void *>(&att_fwd_heavy_kernel<HB, GATHER, A>),
                         attr_set, kMaxLds))
    return rc;
  hipLaunchKernelGGL((att_fwd_heavy_kernel<HB, GATHER, A>), dim3((unsigned)n), dim3(HB), g.lds, st,
                     a, rows, coef, g.FC, g.BE);
  return check_launch("att_fwd_heavy_kernel");
}

template <int HB, class A>
int launch_src_rows(const A &a, const int32_t *rows, int64_t n, float *coef, int budget,
                    hipStream_t st) {
  if (n <= 0) return MGCN_OK;
  const GatherShape g = gather_shape(a.H * a.C, budget);
  static std::atomic<uint64_t> attr_set{0};
  if (int rc = allow_lds(reinterpret_cast<const void *>(&att_bwd_src_heavy_kernel<HB, A>),
                         attr_set, kMaxLds))
    return rc;
  hipLaunchKernelGGL((att_bwd_src_heavy_kernel<HB, A>), dim3((unsigned)n), dim3(HB), g.lds, st, a,
                     rows, coef, g.FC, g.BE);
  return check_launch("att_bwd_src_heavy_kernel");
}

// The _sched bodies.  A: the argument struct of the entry without a schedule,
// checked as that entry checks it (attention_entry.h) plus the schedule.
// Heavy rows by workgroups, then the wave kernel over the schedule's rest.
template <bool GATHER, class A>
int fwd_sched(const char *fn, const A &k, int64_t nnz, const HeavyRows &s, void *stream) {
  ATT_CHECKED((fwd_check<GATHER>(fn, k, nnz, &s)));
  hipStream_t st = as_stream(stream);
  if (int rc = launch_fwd_rows<1024, GATHER>(k, s.order, s.n_giant, s.coef,
                                             g_opt.heavy_lds_kb * 1024, st))
    return rc;
  if (int rc = launch_fwd_rows<256, GATHER>(k, s.order + s.n_giant, s.n_heavy - s.n_giant, s.coef,
                                            g_opt.heavy_mid_lds_kb * 1024, st))
    return rc;
  return fwd_waves<GATHER>(SchedArgsT<A>{k, s.order, s.n_heavy}, "att_fwd_kernel (schedule)", st);
}

template <class A>
int bwd_dst_sched(const char *fn, const A &k, int64_t nnz, const HeavyRows &s, void *stream) {
  ATT_CHECKED(bwd_dst_check(fn, k, nnz, &s));
  hipStream_t st = as_stream(stream);
  // waves along y per row: a giant row's slot groups a few per wave, the
  // other heavy rows' (129 .. giant_thr slots) a handful
  auto slots = [&](const int32_t *rows, int64_t n, unsigned blocks_y) {
    if (n <= 0) return;
    const dim3 grid((unsigned)n, blocks_y), block(kAttThreads);
#define CALL(FPL) hipLaunchKernelGGL((att_bwd_dst_slots_kernel<FPL, A>), grid, block, 0, st, k, rows)
    ATT_DISPATCH(k.H * k.C, CALL);
#undef CALL
  };
  slots(s.order, s.n_giant, 32);
  slots(s.order + s.n_giant, s.n_heavy - s.n_giant, 2);
  if (int rc = check_launch("att_bwd_dst_slots_kernel")) return rc;
  if (k.softmax && s.n_heavy > 0) {
    hipLaunchKernelGGL((att_bwd_dst_row_kernel<A>), dim3((unsigned)s.n_heavy), dim3(kAttThreads),
                       0, st, k, s.order);
    if (int rc = check_launch("att_bwd_dst_row_kernel")) return rc;
  }
  return bwd_dst_waves(SchedArgsT<A>{k, s.order, s.n_heavy}, "att_bwd_dst_kernel (schedule)", st);
}

template <class A>
int bwd_src_sched(const char *fn, const A &k, int64_t nnz, const HeavyRows &s, void *stream) {
  ATT_CHECKED(bwd_src_check(fn, k, nnz, &s));
  hipStream_t st = as_stream(stream);
  if (int rc = launch_src_rows<1024>(k, s.order, s.n_giant, s.coef, g_opt.heavy_lds_kb * 1024, st))
    return rc;
  if (int rc = launch_src_rows<256>(k, s.order + s.n_giant, s.n_heavy - s.n_giant, s.coef,
                                    g_opt.heavy_mid_lds_kb * 1024, st))
    return rc;
  return bwd_src_waves(SchedArgsT<A>{k, s.order, s.n_heavy}, "att_bwd_src_kernel (schedule)", st);
}

}  // namespace
}  // namespace mgcn

using namespace mgcn;

extern "C" int mgcn_att_fwd_sched(int64_t n_rows, int64_t nnz, int32_t H, int32_t C,
                                  const int64_t *rowptr, const int32_t *col, const float *s_row,
                                  const float *s_col, int act, const float *alpha_in,
                                  const float *mask, const float *Hp, int64_t ldh, float *Y,
                                  int64_t ldy, float *alpha, const int32_t *order,
                                  int64_t n_heavy, int64_t n_giant, float *coef, void *stream) {
  if (order == nullptr)
    return mgcn_att_fwd(n_rows, nnz, H, C, rowptr, col, s_row, s_col, act, alpha_in, mask, Hp, ldh,
                        Y, ldy, alpha, stream);
  FwdArgs k{n_rows, H, C, act, rowptr, col, s_row, s_col, alpha_in, mask, Hp, ldh, Y, ldy, alpha};
  return fwd_sched<true>("mgcn_att_fwd_sched", k, nnz, HeavyRows{order, n_heavy, n_giant, coef},
                         stream);
}

extern "C" int mgcn_edge_softmax_sched(int64_t n_rows, int64_t nnz, int32_t H,
                                       const int64_t *rowptr, const int32_t *col,
                                       const float *s_row, const float *s_col, int act,
                                       float *alpha, const int32_t *order, int64_t n_heavy,
                                       int64_t n_giant, void *stream) {
  if (order == nullptr)
    return mgcn_edge_softmax(n_rows, nnz, H, rowptr, col, s_row, s_col, act, alpha, stream);
  FwdArgs k{n_rows, H, 1, act, rowptr, col, s_row, s_col, nullptr, nullptr, nullptr, 0,
            nullptr, 0, alpha};
  return fwd_sched<false>("mgcn_edge_softmax_sched", k, nnz,
                          HeavyRows{order, n_heavy, n_giant, nullptr}, stream);
}

extern "C" int mgcn_att_bwd_dst_sched(int64_t n_rows, int64_t nnz, int32_t H, int32_t C,
                                      const int64_t *rowptr, const int32_t *col, const float *Hp,
                                      int64_t ldh, const float *dY, int64_t lddy,
                                      const float *alpha, const float *mask, const float *s_row,
                                      const float *s_col, int act, int softmax, float *dz,
                                      float *ds_row, const int32_t *order, int64_t n_heavy,
                                      int64_t n_giant, void *stream) {
  if (order == nullptr)
    return mgcn_att_bwd_dst(n_rows, nnz, H, C, rowptr, col, Hp, ldh, dY, lddy, alpha, mask, s_row,
                            s_col, act, softmax, dz, ds_row, stream);
  BwdDstArgs k{n_rows, H, C, act, softmax ? 1 : 0, rowptr, col, Hp, ldh, dY, lddy,
               alpha, mask, s_row, s_col, dz, ds_row};
  return bwd_dst_sched("mgcn_att_bwd_dst_sched", k, nnz,
                       HeavyRows{order, n_heavy, n_giant, nullptr}, stream);
}

extern "C" int mgcn_att_bwd_src_sched(int64_t n_rows, int64_t nnz, int32_t H, int32_t C,
                                      const int64_t *rowptr_t, const int32_t *col_t,
                                      const int32_t *slot_map, const float *dY, int64_t lddy,
                                      const float *alpha, const float *mask, float *dz,
                                      const float *s_row, const float *s_col, int act,
                                      int softmax, const float *a, const float *ds_dst,
                                      float *ds_src, float *dHp, int64_t lddh,
                                      const int32_t *order, int64_t n_heavy, int64_t n_giant,
                                      float *coef, void *stream) {
  if (order == nullptr)
    return mgcn_att_bwd_src(n_rows, nnz, H, C, rowptr_t, col_t, slot_map, dY, lddy, alpha, mask,
                            dz, s_row, s_col, act, softmax, a, ds_dst, ds_src, dHp, lddh, stream);
  BwdSrcArgs k{n_rows, H, C, act, softmax ? 1 : 0, rowptr_t, col_t, slot_map, dY, lddy,
               alpha, mask, dz, s_row, s_col, a, ds_dst, ds_src, dHp, lddh};
  return bwd_src_sched("mgcn_att_bwd_src_sched", k, nnz,
                       HeavyRows{order, n_heavy, n_giant, coef}, stream);
}

// ----------------------------------------------------------- hard attention
extern "C" int mgcn_hatt_fwd_sched(int64_t n_rows, int64_t nnz, int32_t H, int32_t C,
                                   const int64_t *rowptr, const int32_t *col, const float *s_row,
                                   const float *s_col, int act, const float *noise,
                                   float temperature, const float *alpha_in, const float *mask,
                                   const float *Hp, int64_t ldh, float *Y, int64_t ldy,
                                   float *alpha, const int32_t *order, int64_t n_heavy,
                                   int64_t n_giant, float *coef, void *stream) {
  if (order == nullptr)
    return mgcn_hatt_fwd(n_rows, nnz, H, C, rowptr, col, s_row, s_col, act, noise, temperature,
                         alpha_in, mask, Hp, ldh, Y, ldy, alpha, stream);
  HardFwdArgs k{{n_rows, H, C, act, rowptr, col, s_row, s_col, alpha_in, mask, Hp, ldh, Y, ldy,
                 alpha},
                noise, temperature};
  return fwd_sched<true>("mgcn_hatt_fwd_sched", k, nnz, HeavyRows{order, n_heavy, n_giant, coef},
                         stream);
}

extern "C" int mgcn_hatt_edge_softmax_sched(int64_t n_rows, int64_t nnz, int32_t H,
                                            const int64_t *rowptr, const int32_t *col,
                                            const float *s_row, const float *s_col, int act,
                                            const float *noise, float temperature, float *alpha,
                                            const int32_t *order, int64_t n_heavy,
                                            int64_t n_giant, void *stream) {
  if (order == nullptr)
    return mgcn_hatt_edge_softmax(n_rows, nnz, H, rowptr, col, s_row, s_col, act, noise,
                                  temperature, alpha, stream);
  HardFwdArgs k{{n_rows, H, 1, act, rowptr, col, s_row, s_col, nullptr, nullptr, nullptr, 0,
                 nullptr, 0, alpha},
                noise, temperature};
  return fwd_sched<false>("mgcn_hatt_edge_softmax_sched", k, nnz,
                          HeavyRows{order, n_heavy, n_giant, nullptr}, stream);
}

extern "C" int mgcn_hatt_bwd_dst_sched(int64_t n_rows, int64_t nnz, int32_t H, int32_t C,
                                       const int64_t *rowptr, const int32_t *col, const float *Hp,
                                       int64_t ldh, const float *dY, int64_t lddy,
                                       const float *alpha, const float *mask, const float *s_row,
                                       const float *s_col, int act, int softmax,
                                       float temperature, float *dz, float *ds_row,
                                       const int32_t *order, int64_t n_heavy, int64_t n_giant,
                                       void *stream) {
  if (order == nullptr)
    return mgcn_hatt_bwd_dst(n_rows, nnz, H, C, rowptr, col, Hp, ldh, dY, lddy, alpha, mask, s_row,
                             s_col, act, softmax, temperature, dz, ds_row, stream);
  HardBwdDstArgs k{{n_rows, H, C, act, softmax ? 1 : 0, rowptr, col, Hp, ldh, dY, lddy,
                    alpha, mask, s_row, s_col, dz, ds_row},
                   temperature};
  return bwd_dst_sched("mgcn_hatt_bwd_dst_sched", k, nnz,
                       HeavyRows{order, n_heavy, n_giant, nullptr}, stream);
}

extern "C" int mgcn_hatt_bwd_src_sched(int64_t n_rows, int64_t nnz, int32_t H, int32_t C,
                                       const int64_t *rowptr_t, const int32_t *col_t,
                                       const int32_t *slot_map, const float *dY, int64_t lddy,
                                       const float *alpha, const float *mask, float *dz,
                                       const float *s_row, const float *s_col, int act,
                                       int softmax, float temperature, const float *a,
                                       const float *ds_dst, float *ds_src, float *dHp,
                                       int64_t lddh, const int32_t *order, int64_t n_heavy,
                                       int64_t n_giant, float *coef, void *stream) {
  if (order == nullptr)
    return mgcn_hatt_bwd_src(n_rows, nnz, H, C, rowptr_t, col_t, slot_map, dY, lddy, alpha, mask,
                             dz, s_row, s_col, act, softmax, temperature, a, ds_dst, ds_src, dHp,
                             lddh, stream);
  HardBwdSrcArgs k{{n_rows, H, C, act, softmax ? 1 : 0, rowptr_t, col_t, slot_map, dY, lddy,
                    alpha, mask, dz, s_row, s_col, a, ds_dst, ds_src, dHp, lddh},
                   temperature};
  return bwd_src_sched("mgcn_hatt_bwd_src_sched", k, nnz,
                       HeavyRows{order, n_heavy, n_giant, coef}, stream);
}
