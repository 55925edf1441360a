// Heavy rows of the edge-gate launches (gfx950): the rows order[0, n_heavy) of
// a view's schedule (mgcn_row_schedule: degree > 128; the botnet graphs reach
// ~6k), which the wave-per-row kernels of edge_gate.hip would walk 64 slots at
// a time by one wave each.  Every output element keeps the bits the wave
// kernel gives it: what a slot contributes depends on the slot alone, so any
// thread may form it; what a row sums is summed in the wave kernel's order.
//
// Forward, one workgroup per row: all threads form the row's gates (g written
// as always) and coefficients coef = g w into the caller's scratch, barrier,
// then the SpMM's heavy-row body (heavy.h) with w := coef: producer waves
// gather batches of the row's edges into LDS, the fold waves run one chain per
// feature in slot order (`__fadd_rn`, or `>=` with the later slot winning),
// and its epilogue is the gate kernel's (mean division, bias, ReLU; argmax as
// eid[slot]).  A product is __fmul_rn(Hx, coef) there and __fmul_rn(coef, Hx)
// in the wave kernel: the same bits.
//
// Adjoint by destination: the per-slot results (dot, dw, dg, dl) depend on the
// slot's 64-slot chunk only, so the chunks of a heavy row go to separate waves
// of several workgroups, each chunk processed as the wave kernel processes it.
// dc[row] is then summed by one wave per row that re-reads the row's dl in the
// wave kernel's order (lane u adds dl[k0 + u] chunk after chunk, then the
// butterfly): a second launch, ordered behind the first by the stream.
//
// Adjoint by source, one workgroup per row: coef = g[slot_map[k]] w_t[k] into
// the scratch, barrier, the heavy-row body (BWD_SUM, or BWD_MAXM under max:
// dY replaced by 0 where the fwd slot did not win) writes dHx[row] =
// chain [* row_scale]; wave 0 sums da[row] in the wave kernel's order, and
// each fold thread adds da w_sd[f], then dc w_sd[C + f], to the element it
// wrote.
//
// Barriers only: no atomics, no hand-off between workgroups.
//
// bf16 rows (the mgcn_gate_*_sched_bf16 entries; argument structs with Row =
// uint16_t): the heavy-row body gathers and stores through load_x / store_y
// with T = uint16_t -- its LDS holds fp32 products and metadata words with
// either T, so heavy_shape is unchanged -- and the chunk kernel through
// row_ld.  A bf16 dHx element must be rounded once, so the by-source kernel
// cannot add the rank-one terms to a stored row: wave 0 sums da before the
// body and the terms are the body's last fp32 step (GateSrcEpi).  Mean: the
// body's BWD_MEAN divides each gathered dY element by cnt[col] before its
// product, the chunk kernel divides its dY row by cnt[row].

#include <atomic>

#include "attention.h"
#include "edge_gate.h"
#include "heavy.h"

namespace mgcn {
namespace {

// Edge quads in flight per producer thread of the heavy-row body (0: its own
// choice).  The 1024-thread workgroups (128 VGPRs per thread) take one: with
// the body's two, the float4 forward sum kernel spilled 4 VGPRs to scratch.
template <int HB>
constexpr int kQuads = HB >= 1024 ? 1 : 0;

// ----------------------------------------------------------------- forward
template <int VEC, int MODE, int HB, class A = GateFwdArgs>
__global__ __launch_bounds__(HB) void gate_fwd_heavy_kernel(const SpmmArgs s, const A a, int FC,
                                                            int BE) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int64_t row = s.heavy_rows[blockIdx.x];
  const int64_t beg = a.rowptr[row], end = a.rowptr[row + 1];
  const float tb = (a.t != nullptr && a.t_bcast) ? a.t[0] : 0.0f;
  const float cr = a.c != nullptr ? a.c[row] : 0.0f;
  for (int64_t k = beg + threadIdx.x; k < end; k += HB) {
    float l = cr;
    if (a.a != nullptr) l = __fadd_rn(a.a[a.col[k]], l);
    if (a.t != nullptr) l = __fadd_rn(l, a.t_bcast ? tb : a.t[k]);
    const float g = gate_sigmoid(l);
    a.g[k] = g;
    a.s.coef[k] = a.w != nullptr ? __fmul_rn(g, a.w[k]) : g;
  }
  __syncthreads();  // the row's coef: written above, read below as s.w
  heavy_row_block<VEC, MODE, HB, kQuads<HB>, typename A::Row>(s, FC, BE, blockIdx.x, smem);
}

// ------------------------------------------------- adjoint, by destination
// Chunk c of heavy row order[blockIdx.x] by wave c (grid-stride over the
// row's chunks along blockIdx.y): gate_bwd_dst_kernel's chunk body.
template <int FPL, bool MAX, class A = GateBwdDstArgs>
__global__ __launch_bounds__(kAttThreads) void gate_bwd_dst_chunk_kernel(A a,
                                                                         const int32_t *rows) {
  constexpr int U = gather_unroll<FPL>();
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = blockIdx.y * (int64_t)kAttWaves + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.y * kAttWaves;
  const int C = a.C, W = (a.C + 31) >> 5;
  const int64_t row = rows[blockIdx.x];
  const int64_t beg = a.rowptr[row], end = a.rowptr[row + 1];
  const int64_t n_chunks = (end - beg + 63) >> 6;
  if (wave0 >= n_chunks) return;
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
  for (int64_t ch = wave0; ch < n_chunks; ch += nwaves) {
    const int64_t k0 = beg + 64 * ch;
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
      a.dl[k] = __fmul_rn(dg, __fmul_rn(g, __fsub_rn(1.0f, g)));
    }
  }
}

// dc of the heavy rows, one wave per row: the wave kernel's sum of the row's
// dl (lane u adds dl[k0 + u] chunk after chunk, then the butterfly), re-read
// from memory.
template <class A = GateBwdDstArgs>
__global__ __launch_bounds__(kAttThreads) void gate_dc_heavy_kernel(A a) {
  const int lane = threadIdx.x & 63;
  const int64_t i = blockIdx.x * (int64_t)kAttWaves + (threadIdx.x >> 6);
  if (i >= a.s.n_heavy) return;
  const int64_t row = a.s.order[i];
  const int64_t beg = a.rowptr[row], end = a.rowptr[row + 1];
  float part = 0.0f;
  for (int64_t k0 = beg; k0 < end; k0 += 64) {
    const int64_t k = k0 + lane;
    if (k < end) part = __fadd_rn(part, a.dl[k]);
  }
  const float tot = wave_sum(part);
  if (lane == 0) a.dc[row] = tot;
}

// ------------------------------------------------------ adjoint, by source
// the rank-one terms of dHx[row, f] as the heavy-row body's last fp32 step
// (bf16 rows): the wave kernel's two adds, in its order
struct GateSrcEpi {
  const float *wsd;
  int C;
  float dav, dcv;
  bool has_da, has_dc;
  __device__ __forceinline__ float operator()(int f, float v) const {
    if (wsd != nullptr) {
      if (has_da) v = __fadd_rn(v, __fmul_rn(dav, wsd[f]));
      if (has_dc) v = __fadd_rn(v, __fmul_rn(dcv, wsd[C + f]));
    }
    return v;
  }
};

template <int VEC, int MODE, int HB, class A = GateBwdSrcArgs>
__global__ __launch_bounds__(HB) void gate_bwd_src_heavy_kernel(const SpmmArgs s, const A a,
                                                                int FC, int BE) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int t = threadIdx.x;
  const int64_t row = s.heavy_rows[blockIdx.x];
  const int64_t beg = a.rowptr[row], end = a.rowptr[row + 1];
  for (int64_t k = beg + t; k < end; k += HB) {
    const float g = a.g[a.slot[k]];
    a.s.coef[k] = a.w_t != nullptr ? __fmul_rn(g, a.w_t[k]) : g;
  }
  if constexpr (sizeof(typename A::Row) != sizeof(float)) {
    // bf16 rows: da first (wave 0, the wave kernel's order), handed to every
    // thread through smem[0] -- read before the body's first barrier, written
    // by the body only after it -- then the body rounds chain [* row_scale]
    // + da w_sd[f] + dc w_sd[C + f] once at its store
    if (a.da != nullptr && t < 64) {
      float part = 0.0f;
      for (int64_t k0 = beg; k0 < end; k0 += 64) {
        const int64_t k = k0 + t;
        if (k < end) part = __fadd_rn(part, a.dl[a.slot[k]]);
      }
      const float tot = wave_sum(part);
      if (t == 0) {
        a.da[row] = tot;
        smem[0] = tot;
      }
    }
    __syncthreads();  // the row's coef and da
    const GateSrcEpi epi{a.wsd, a.C, a.da != nullptr ? smem[0] : 0.0f,
                         a.dc != nullptr ? a.dc[row] : 0.0f, a.da != nullptr, a.dc != nullptr};
    heavy_row_block<VEC, MODE, HB, kQuads<HB>, typename A::Row>(s, FC, BE, blockIdx.x, smem, epi);
  } else {
    __syncthreads();  // the row's coef: written above, read below as s.w
    // dHx[row, f] = chain [* row_scale]; ends on a barrier
    heavy_row_block<VEC, MODE, HB, kQuads<HB>>(s, FC, BE, blockIdx.x, smem);
    if (a.da == nullptr && a.dc == nullptr) return;
    float dav = 0.0f;
    if (a.da != nullptr) {
      if (t < 64) {
        float part = 0.0f;  // lane t's share of sum_row dl, in the wave kernel's order
        for (int64_t k0 = beg; k0 < end; k0 += 64) {
          const int64_t k = k0 + t;
          if (k < end) part = __fadd_rn(part, a.dl[a.slot[k]]);
        }
        const float tot = wave_sum(part);
        if (t == 0) {
          a.da[row] = tot;
          smem[0] = tot;
        }
      }
      __syncthreads();
      dav = smem[0];
    }
    const float dcv = a.dc != nullptr ? a.dc[row] : 0.0f;
    const int C = a.C;
    // thread t < fc stored feature f0 + t of every chunk (heavy_row_block)
    for (int f0 = 0; f0 < C; f0 += FC) {
      const int fc = C - f0 < FC ? C - f0 : FC;
      if (t < fc) {
        const int f = f0 + t;
        float v = a.dHx[row * a.lddh + f];
        if (a.da != nullptr) v = __fadd_rn(v, __fmul_rn(dav, a.wsd[f]));
        if (a.dc != nullptr) v = __fadd_rn(v, __fmul_rn(dcv, a.wsd[C + f]));
        a.dHx[row * a.lddh + f] = v;
      }
    }
  }
}

// ------------------------------------------------------------------- host
// widest vector the gathered and the written rows both allow (spmm.hip)
// (esz: bytes per row element -- 4, or 2 for bf16 rows)
int gate_vec(int32_t F, const void *p0, int64_t ld0, const void *p1, int64_t ld1, int esz) {
  auto ok = [&](int v) {
    return F % v == 0 && ld0 % v == 0 && ld1 % v == 0 &&
           reinterpret_cast<uintptr_t>(p0) % (esz * v) == 0 &&
           reinterpret_cast<uintptr_t>(p1) % (esz * v) == 0;
  };
  return ok(4) ? 4 : ok(2) ? 2 : 1;
}

template <int VEC, int MODE, int HB, class A>
int launch_rows(SpmmArgs s, const A &a, const int32_t *rows, int64_t n, int lds_budget,
                hipStream_t stream) {
  if (n <= 0) return MGCN_OK;
  s.heavy_rows = rows;
  const HeavyShape h = heavy_shape(s.F, VEC, HB, lds_budget);
  static std::atomic<uint64_t> attr_set{0};
  if constexpr (MODE == FWD_SUM || MODE == FWD_MAX) {
    if (int rc = allow_lds(
            reinterpret_cast<const void *>(&gate_fwd_heavy_kernel<VEC, MODE, HB, A>), attr_set,
            160 * 1024))
      return rc;
    hipLaunchKernelGGL((gate_fwd_heavy_kernel<VEC, MODE, HB, A>), dim3((unsigned)n), dim3(HB),
                       h.lds, stream, s, a, h.FC, h.BE);
    return check_launch("gate_fwd_heavy_kernel");
  } else {
    if (int rc = allow_lds(
            reinterpret_cast<const void *>(&gate_bwd_src_heavy_kernel<VEC, MODE, HB, A>),
            attr_set, 160 * 1024))
      return rc;
    hipLaunchKernelGGL((gate_bwd_src_heavy_kernel<VEC, MODE, HB, A>), dim3((unsigned)n),
                       dim3(HB), h.lds, stream, s, a, h.FC, h.BE);
    return check_launch("gate_bwd_src_heavy_kernel");
  }
}

// giant rows by 1024-thread workgroups with the large LDS budget, the other
// heavy rows by 256-thread ones, as the SpMM's heavy launches
template <int VEC, int MODE, class A>
int launch_heavy(const SpmmArgs &s, const A &a, hipStream_t stream) {
  const GateSched &g = a.s;
  if (int rc = launch_rows<VEC, MODE, 1024>(s, a, g.order, g.n_giant, g_opt.heavy_lds_kb * 1024,
                                            stream))
    return rc;
  return launch_rows<VEC, MODE, 256>(s, a, g.order + g.n_giant, g.n_heavy - g.n_giant,
                                     g_opt.heavy_mid_lds_kb * 1024, stream);
}

template <int MODE, class A>
int launch_heavy_v(const SpmmArgs &s, const A &a, hipStream_t stream) {
  const int vec = gate_vec(s.F, s.X, s.ldx, s.Y, s.ldy, (int)sizeof(typename A::Row));
  if (vec == 4) return launch_heavy<4, MODE>(s, a, stream);
  if (vec == 2) return launch_heavy<2, MODE>(s, a, stream);
  return launch_heavy<1, MODE>(s, a, stream);
}

// (the SpMM block holds X and Y as float pointers; bf16 rows travel behind
// them and the body casts back to its T)
template <class R>
const float *as_f(const R *p) {
  return reinterpret_cast<const float *>(p);
}
template <class R>
float *as_f(R *p) {
  return reinterpret_cast<float *>(p);
}

template <class A>
int fwd_heavy(const A &a, hipStream_t stream) {
  SpmmArgs s{};
  s.n_rows = a.n_rows;
  s.F = a.C;
  s.n_chunks = 1;
  s.rowptr = a.rowptr;
  s.col = a.col;
  s.eid = a.eid;
  s.w = a.s.coef;
  s.X = as_f(a.Hx);
  s.ldx = a.ldh;
  s.Y = as_f(a.Y);
  s.ldy = a.ldy;
  s.bias = a.bias;
  s.argmax_out = a.argmax;
  s.mean = a.reduce == MGCN_REDUCE_MEAN;
  s.relu = a.relu;
  if (a.reduce == MGCN_REDUCE_MAX) return launch_heavy_v<FWD_MAX>(s, a, stream);
  return launch_heavy_v<FWD_SUM>(s, a, stream);
}

template <class A>
int bwd_dst_heavy(const A &a, hipStream_t stream) {
  // waves along y per row: a giant row's chunks one or two per wave, the
  // other heavy rows' (129 .. giant_thr slots) a few
  auto chunks = [&](const int32_t *rows, int64_t n, unsigned blocks_y) {
    if (n <= 0) return;
    const dim3 grid((unsigned)n, blocks_y), block(kAttThreads);
#define CALL(FPL)                                                                             \
  do {                                                                                        \
    if (a.win != nullptr)                                                                     \
      hipLaunchKernelGGL((gate_bwd_dst_chunk_kernel<FPL, true, A>), grid, block, 0, stream,   \
                         a, rows);                                                            \
    else                                                                                      \
      hipLaunchKernelGGL((gate_bwd_dst_chunk_kernel<FPL, false, A>), grid, block, 0, stream,  \
                         a, rows);                                                            \
  } while (0)
    ATT_DISPATCH(a.C, CALL);
#undef CALL
  };
  chunks(a.s.order, a.s.n_giant, 16);
  chunks(a.s.order + a.s.n_giant, a.s.n_heavy - a.s.n_giant, 2);
  if (int rc = check_launch("gate_bwd_dst_chunk_kernel")) return rc;
  if (a.dc == nullptr) return MGCN_OK;
  const unsigned blocks = (unsigned)((a.s.n_heavy + kAttWaves - 1) / kAttWaves);
  hipLaunchKernelGGL(gate_dc_heavy_kernel<A>, dim3(blocks), dim3(kAttThreads), 0, stream, a);
  return check_launch("gate_dc_heavy_kernel");
}

template <class A>
int bwd_src_heavy(const A &a, hipStream_t stream) {
  SpmmArgs s{};
  s.n_rows = a.n_rows;
  s.F = a.C;
  s.n_chunks = 1;
  s.rowptr = a.rowptr;
  s.col = a.col;
  s.w = a.s.coef;
  s.X = as_f(a.dY);
  s.ldx = a.lddy;
  s.Y = as_f(a.dHx);
  s.ldy = a.lddh;
  s.row_scale = a.row_scale;
  s.win_mask = a.win;
  s.slot_map = a.slot;
  if (a.win != nullptr) return launch_heavy_v<BWD_MAXM>(s, a, stream);
  if constexpr (A::kCnt) {
    if (a.cnt != nullptr) {  // mean: every gathered element divided by cnt[col]
      s.cnt = a.cnt;
      return launch_heavy_v<BWD_MEAN>(s, a, stream);
    }
  }
  return launch_heavy_v<BWD_SUM>(s, a, stream);
}

}  // namespace

int gate_fwd_heavy(const GateFwdArgs &a, hipStream_t stream) { return fwd_heavy(a, stream); }
int gate_fwd_heavy(const GateFwdArgsBf16 &a, hipStream_t stream) { return fwd_heavy(a, stream); }
int gate_bwd_dst_heavy(const GateBwdDstArgs &a, hipStream_t stream) {
  return bwd_dst_heavy(a, stream);
}
int gate_bwd_dst_heavy(const GateBwdDstArgsBf16 &a, hipStream_t stream) {
  return bwd_dst_heavy(a, stream);
}
int gate_bwd_src_heavy(const GateBwdSrcArgs &a, hipStream_t stream) {
  return bwd_src_heavy(a, stream);
}
int gate_bwd_src_heavy(const GateBwdSrcArgsBf16 &a, hipStream_t stream) {
  return bwd_src_heavy(a, stream);
}

}  // namespace mgcn
