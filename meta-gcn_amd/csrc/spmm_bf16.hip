// bf16 feature rows through the CSR row-block SpMM (gfx950): mgcn_spmm_fwd_bf16,
// mgcn_spmm_bwd_bf16 and mgcn_relu_bwd_colsum_bf16.
//
// Arithmetic contract: every bf16 element of H (dY in the adjoint) is widened
// to fp32 (exact), then the row is formed exactly as spmm.hip's spmm_kernel
// forms it -- products and sums rounded separately, in COO edge order within
// a row, fp32 edge weights, fp32 mean division, the max fill / tie / fill -> 0
// rules, fp32 bias and ReLU, row_scale and the adjoint's per-edge division by
// cnt -- and the fp32 result is rounded once, to nearest even, at the store.
// The outputs are therefore bit for bit  bf16(mgcn_spmm_fwd(float(H)))  and
// bf16(mgcn_spmm_bwd(float(dY))); argmax and the winner bits are the fp32
// path's as they stand.
//
// Roofline: HBM-bound.  Algorithmic bytes per launch
//     8 (n_rows + 1) + nnz * (4 col + 4 w + 2 F) + 2 n_rows F
// i.e. 0.51 of the fp32 launch at F = 128 and 11 edges per row.
//
// Layout of a wave: a lane holds 8 consecutive bf16 (one 16-byte load), so
// G = F / 8 lanes read a whole row in one coalesced instruction (F = 128: 16
// lanes, 256 B, four rows per wave).  Edge metadata is loaded lane-parallel,
// G edges per instruction, and broadcast inside the group; U gathers are
// issued back to back before any is consumed; the eight accumulators per lane
// are fp32 registers.  Shapes taken: F % 8 == 0, 16-byte aligned rows
// (mgcn_spmm_bf16_supported); the Python layer routes every other shape
// through  float -> fp32 kernel -> bf16,  which gives the same bits.
//
// Heavy and giant rows (order, n_heavy, n_giant as mgcn_spmm_fwd takes them)
// run heavy.h's workgroup-per-row pipeline, instantiated over bf16 storage:
// 4 bf16 (8 B) per producer thread, the products and the edge-order fold in
// fp32 as they are.  Both heavy launches go on the caller's stream, ahead of
// the lane-group kernel (no side stream here).

#include "heavy.h"
#include "mgcn_internal.h"
#include "x6.h"

namespace mgcn {
namespace {

using x6::bf16x2;
using x6::f32x2;
using x6::u32x4;
using x6::widen_bf16x2;

constexpr int kWaves = 4;  // waves per 256-thread block
constexpr int kBlock = 64 * kWaves;
constexpr int kVec = 8;    // bf16 per lane: one 16-byte access

// The kernels take heavy.h's SpmmArgs as the fp32 ones do; X and Y carry the
// bf16 rows behind its float pointers (ldx / ldy count elements), relu_mask,
// accumulate and rs stay unset.

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
__device__ __forceinline__ int64_t wave_max_over_groups(int64_t v) {
#pragma unroll
  for (int off = G; off < 64; off <<= 1) {
    const int64_t o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}

// 8 bf16 <-> 8 floats: element 2 i in the low half of word i
__device__ __forceinline__ F32v<kVec> widen8(const u32x4 p) {
  F32v<kVec> r;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x2 t = widen_bf16x2(p[i]);
    r.v[2 * i] = t.x;
    r.v[2 * i + 1] = t.y;
  }
  return r;
}
__device__ __forceinline__ u32x4 round8(const F32v<kVec> &r) {  // v_cvt_pk_bf16_f32, RNE
  u32x4 p;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x2 t = {r.v[2 * i], r.v[2 * i + 1]};
    p[i] = __builtin_bit_cast(uint32_t, __builtin_convertvector(t, bf16x2));
  }
  return p;
}
__device__ __forceinline__ u32x4 load_bf8(const uint16_t *p) {
  return *reinterpret_cast<const u32x4 *>(p);
}
__device__ __forceinline__ I32v<kVec> load_i8(const int32_t *p) {
  const I32v<4> a = load_i<4>(p), b = load_i<4>(p + 4);
  I32v<kVec> r;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    r.v[j] = a.v[j];
    r.v[4 + j] = b.v[j];
  }
  return r;
}

// spmm.hip's spmm_kernel over bf16 rows: the same loop structure, metadata
// run-ahead and fold order; a lane's piece of a row is 8 features.
template <int G, int U, int MODE>
__global__ __launch_bounds__(kBlock) void spmm_bf16_kernel(const SpmmArgs a) {
  constexpr int VEC = kVec;
  constexpr int RPW = 64 / G;  // rows per wave
  constexpr bool kFwd = (MODE == FWD_SUM || MODE == FWD_MAX);
  constexpr bool kNeedEid = (MODE == BWD_MAX);
  const int lane = threadIdx.x & 63;
  const int gl = lane & (G - 1);
  const int grp = lane / G;
  const int gbase = grp * G;
  const int wave_in_block = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t n_work = a.order != nullptr ? a.n_rows - a.n_heavy : a.n_rows;
  const int32_t *__restrict__ order = a.order != nullptr ? a.order + a.n_heavy : nullptr;
  const int64_t n_row_groups = (n_work + RPW - 1) / RPW;
  const int64_t wave_stride = (int64_t)gridDim.x * kWaves;
  const uint16_t *__restrict__ X = reinterpret_cast<const uint16_t *>(a.X);
  const bool has_w = a.w != nullptr;

  auto row_of = [&](int64_t wv, bool &ok) -> int64_t {
    const int64_t item = wv * RPW + grp;
    ok = wv < n_row_groups && item < n_work;
    return !ok ? 0 : order != nullptr ? (int64_t)order[item] : item;
  };
  const int64_t wv0 = (int64_t)blockIdx.x * kWaves + wave_in_block;
  bool ok_n, ok_nn;
  int64_t row_n = row_of(wv0, ok_n);
  int64_t beg_n = ok_n ? a.rowptr[row_n] : 0, end_n = ok_n ? a.rowptr[row_n + 1] : 0;
  int64_t row_nn = row_of(wv0 + wave_stride, ok_nn);
  for (int64_t wv = wv0; wv < n_row_groups; wv += wave_stride) {
    const bool row_ok = ok_n;
    const int64_t row = row_n;
    const int64_t beg = beg_n;
    const int64_t deg = end_n - beg_n;
    row_n = row_nn;
    ok_n = ok_nn;
    beg_n = ok_n ? a.rowptr[row_n] : 0;
    end_n = ok_n ? a.rowptr[row_n + 1] : 0;
    row_nn = row_of(wv + 2 * wave_stride, ok_nn);
    const int64_t maxdeg = (RPW > 1) ? wave_max_over_groups<G>(deg) : deg;

    for (int c = 0; c < a.n_chunks; ++c) {
      const int f0 = (c * G + gl) * VEC;
      const bool f_ok = f0 < a.F;  // F % 8 == 0: a lane's 8 features are all in or all out
      F32v<VEC> acc;
      I32v<VEC> arg;
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        acc.v[j] = (MODE == FWD_MAX) ? MGCN_MAX_FILL : 0.0f;
        arg.v[j] = -1;
      }

      for (int64_t e0 = 0; e0 < maxdeg; e0 += G) {
        // lane-parallel metadata for the next (up to) G edges of this row
        const int64_t my = e0 + gl;
        int mc = 0, me = 0;
        float mw = 1.0f, mcnt = 1.0f;
        if (my < deg) {
          mc = a.col[beg + my];
          if (has_w) mw = a.w[beg + my];
          if constexpr (kNeedEid) me = a.eid[beg + my];
          if constexpr (MODE == BWD_MAXM) me = a.slot_map[beg + my];  // fwd slot of this edge
          if constexpr (MODE == BWD_MEAN) mcnt = a.cnt[mc];
        }
        const int64_t rem = deg - e0;
        const int nb = rem <= 0 ? 0 : (rem < G ? (int)rem : G);  // this group
        const int64_t remw = maxdeg - e0;
        const int nbmax = remw < G ? (int)remw : G;              // wave-uniform

        for (int k0 = 0; k0 < nbmax; k0 += U) {
          u32x4 xb[U];  // the gathered rows as they arrive, 8 bf16 per lane
          float wk[U], cntk[U];
          int ek[U];
          bool ok[U];
          uint32_t wbits[U];  // BWD_MAXM: the edge's winner word
          I32v<VEC> am[U];    // BWD_MAX: the gathered row's argmax
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int k = k0 + u;
            const int kk = k & (G - 1);
            const int ck = bcast_i<G>(mc, gbase, kk);
            wk[u] = bcast_f<G>(mw, gbase, kk);
            ek[u] = (MODE == FWD_MAX) ? (int)(e0 + k)
                    : (kNeedEid || MODE == BWD_MAXM) ? bcast_i<G>(me, gbase, kk) : 0;
            cntk[u] = 1.0f;
            if constexpr (MODE == BWD_MEAN) cntk[u] = bcast_f<G>(mcnt, gbase, kk);
            ok[u] = (k < nb) && f_ok;
            const uint16_t *src = X + (int64_t)ck * a.ldx + f0;
            if constexpr (MODE == BWD_MAXM) {
              // dY row and the edge's winner bits (at its fwd slot) are loaded
              // unconditionally (masked edges read row 0 / word 0, never
              // used), as spmm_kernel does: no select between the loads
              const int64_t W = (a.F + 31) >> 5;
              wbits[u] = a.win_mask[ok[u] ? (int64_t)ek[u] * W + (f0 >> 5) : 0];
              xb[u] = load_bf8(ok[u] ? src : X);
            } else if (ok[u]) {
              xb[u] = load_bf8(src);
              if constexpr (MODE == BWD_MAX) am[u] = load_i8(a.argmax_in + (int64_t)ck * a.F + f0);
            }
          }
          // fold in strictly ascending edge order
#pragma unroll
          for (int u = 0; u < U; ++u) {
            if (ok[u]) {
              F32v<VEC> xv = widen8(xb[u]);
              if constexpr (MODE == BWD_MAXM) {
                const uint32_t bits = wbits[u] >> (f0 & 31);
#pragma unroll
                for (int j = 0; j < VEC; ++j) xv.v[j] = ((bits >> j) & 1u) ? xv.v[j] : 0.0f;
              }
              if constexpr (MODE == BWD_MAX) {
#pragma unroll
                for (int j = 0; j < VEC; ++j) xv.v[j] = (am[u].v[j] == ek[u]) ? xv.v[j] : 0.0f;
              }
              if constexpr (MODE == BWD_MEAN) {
#pragma unroll
                for (int j = 0; j < VEC; ++j) xv.v[j] = __fdiv_rn(xv.v[j], cntk[u]);
              }
#pragma unroll
              for (int j = 0; j < VEC; ++j) {
                const float p = __fmul_rn(xv.v[j], wk[u]);
                if constexpr (MODE == FWD_MAX) {
                  if (p >= acc.v[j]) {  // `>=`: the later edge wins ties
                    acc.v[j] = p;
                    arg.v[j] = ek[u];
                  }
                } else {
                  acc.v[j] = __fadd_rn(acc.v[j], p);
                }
              }
            }
          }
        }
      }

      if constexpr (MODE == FWD_MAX) {
        if (a.win_mask_out != nullptr) {
          // winner bits of every edge of this row, at its own (fwd) slot: a
          // pass over the row's edge positions; each 32-bit word is OR-ed over
          // its 4 lanes (all lanes of the group take part; a lane past F
          // holds no winner and contributes 0)
          int32_t winner[VEC];  // position of the winning edge in the row, -1: none
#pragma unroll
          for (int j = 0; j < VEC; ++j) winner[j] = (acc.v[j] == MGCN_MAX_FILL) ? -1 : arg.v[j];
          const int64_t W = (a.F + 31) >> 5;
          constexpr int LW = 32 / VEC;  // lanes per word (G >= 4)
          for (int64_t e0 = 0; e0 < maxdeg; e0 += G) {
            const int64_t rem = deg - e0;
            const int nb = rem <= 0 ? 0 : (rem < G ? (int)rem : G);
            const int64_t remw = maxdeg - e0;
            const int nbmax = remw < G ? (int)remw : G;  // wave-uniform
            for (int k = 0; k < nbmax; ++k) {
              const int32_t ek = (int32_t)(e0 + k);
              uint32_t v = 0;
#pragma unroll
              for (int j = 0; j < VEC; ++j) v |= (winner[j] == ek ? 1u : 0u) << j;
              v <<= (f0 & 31);
#pragma unroll
              for (int off = 1; off < LW; off <<= 1) v |= __shfl_xor(v, off, 64);
              if (k < nb && f_ok && (f0 & 31) == 0)
                a.win_mask_out[(beg + e0 + k) * W + (f0 >> 5)] = v;
            }
          }
        }
      }
      if (!(row_ok && f_ok)) continue;
      uint16_t *dst = reinterpret_cast<uint16_t *>(a.Y) + row * a.ldy + f0;
      if constexpr (kFwd) {
        const float inv_cnt = (float)(deg > 1 ? deg : 1);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          float y = acc.v[j];
          if constexpr (MODE == FWD_MAX) {
            if (y == MGCN_MAX_FILL) {
              y = 0.0f;
              arg.v[j] = -1;
            }
          } else {
            if (a.mean) y = __fdiv_rn(y, inv_cnt);
          }
          if (a.bias != nullptr) y = __fadd_rn(y, a.bias[f0 + j]);
          if (a.relu) y = (y < 0.0f) ? 0.0f : y;
          acc.v[j] = y;
        }
        if constexpr (MODE == FWD_MAX) {
          if (a.argmax_out != nullptr) {
            // winner positions -> edge ids (torch_scatter's argmax)
            I32v<4> lo, hi;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              lo.v[j] = arg.v[j] >= 0 ? a.eid[beg + arg.v[j]] : -1;
              hi.v[j] = arg.v[4 + j] >= 0 ? a.eid[beg + arg.v[4 + j]] : -1;
            }
            store_i<4>(a.argmax_out + row * a.F + f0, lo);
            store_i<4>(a.argmax_out + row * a.F + f0 + 4, hi);
          }
        }
      } else {
        if (a.row_scale != nullptr) {
          const float s = a.row_scale[row];
#pragma unroll
          for (int j = 0; j < VEC; ++j) acc.v[j] = __fmul_rn(acc.v[j], s);
        }
      }
      // the one rounding of the contract
      *reinterpret_cast<u32x4 *>(dst) = round8(acc);
    }
  }
}

template <int G, int U, int MODE>
int launch_one(const SpmmArgs &a, hipStream_t stream) {
  constexpr int RPW = 64 / G;
  const int64_t light = a.order != nullptr ? a.n_rows - a.n_heavy : a.n_rows;
  if (light <= 0) return MGCN_OK;
  const int64_t waves = (light + RPW - 1) / RPW;
  int64_t blocks = (waves + kWaves - 1) / kWaves;
  if (blocks > (int64_t(1) << 20)) blocks = int64_t(1) << 20;  // grid-stride beyond
  hipLaunchKernelGGL((spmm_bf16_kernel<G, U, MODE>), dim3((unsigned)blocks), dim3(kBlock), 0,
                     stream, a);
  return check_launch("spmm_bf16_kernel");
}

// ---------------------------------------------------------------- heavy rows
// heavy.h's heavy_row_block over bf16 storage (VEC = 4: 8 bytes per producer
// thread and row piece); workgroup shapes and LDS budgets as spmm.hip's
// defaults: 1024 threads and a CU's 160 KB for a giant row, 256 threads and
// 40 KB for the other heavy rows (one edge quad in flight at F <= 32).
constexpr int kHeavyVec = 4;
constexpr int kGiantLds = 160 * 1024;
constexpr int kMidLds = 40 * 1024;

template <int MODE, int HB, int Q>
__global__ __launch_bounds__(HB) void spmm_bf16_heavy_kernel(const SpmmArgs a, int FC, int BE) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  heavy_row_block<kHeavyVec, MODE, HB, Q, uint16_t>(a, FC, BE, blockIdx.x, smem);
}

template <int MODE, int HB, int Q>
int launch_heavy_q(const SpmmArgs &a, int64_t n, const HeavyShape &h, hipStream_t stream) {
  static std::atomic<uint64_t> attr_set{0};  // per instantiation
  if (int rc = allow_lds(reinterpret_cast<const void *>(&spmm_bf16_heavy_kernel<MODE, HB, Q>),
                         attr_set, kGiantLds))
    return rc;
  hipLaunchKernelGGL((spmm_bf16_heavy_kernel<MODE, HB, Q>), dim3((unsigned)n), dim3(HB), h.lds,
                     stream, a, h.FC, h.BE);
  return check_launch("spmm_bf16_heavy_kernel");
}

template <int MODE, int HB>
int launch_heavy_hb(SpmmArgs a, const int32_t *rows, int64_t n, int lds_budget,
                    hipStream_t stream) {
  if (n <= 0) return MGCN_OK;
  a.heavy_rows = rows;
  const HeavyShape h = heavy_shape(a.F, kHeavyVec, HB, lds_budget);  // F % 8 == 0: FC = min(F, 128)
  if constexpr (HB == 256)
    if (h.FC <= 32) return launch_heavy_q<MODE, HB, 1>(a, n, h, stream);
  return launch_heavy_q<MODE, HB, 0>(a, n, h, stream);
}

template <int MODE>
int launch_mode(SpmmArgs a, hipStream_t stream) {
  if (a.order == nullptr) a.n_heavy = a.n_giant = 0;
  // giant rows, then the other heavy rows, then the lane-group kernel
  if (int rc = launch_heavy_hb<MODE, 1024>(a, a.order, a.n_giant, kGiantLds, stream)) return rc;
  if (int rc = launch_heavy_hb<MODE, 256>(a, a.order + a.n_giant, a.n_heavy - a.n_giant, kMidLds,
                                          stream))
    return rc;
  const int lanes = a.F / kVec;
  a.n_chunks = (lanes + 63) / 64;
  if (a.n_chunks < 1) a.n_chunks = 1;
  if (lanes > 32) return launch_one<64, 8, MODE>(a, stream);
  if (lanes > 16) return launch_one<32, 8, MODE>(a, stream);
  if (lanes > 8) return launch_one<16, 8, MODE>(a, stream);
  if (lanes > 4) return launch_one<8, 8, MODE>(a, stream);
  return launch_one<4, 4, MODE>(a, stream);
}

// --------------------------------------------------- relu backward + colsum
constexpr int kMaxPartialBlocks = 1024;  // as elementwise.hip: mgcn_colsum_workspace_bytes' count

int colsum_blocks(int64_t n) {
  int64_t b = (n + 63) / 64;
  if (b > kMaxPartialBlocks) b = kMaxPartialBlocks;
  if (b < 1) b = 1;
  return (int)b;
}

template <int VEC>
__device__ __forceinline__ void load_bf(const uint16_t *p, float (&v)[VEC]) {
  if constexpr (VEC == 8) {
    const F32v<8> t = widen8(load_bf8(p));
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = t.v[j];
  } else {
    v[0] = __uint_as_float((uint32_t)p[0] << 16);
  }
}

// elementwise.hip's relu_bwd_colsum_kernel over bf16 rows: block b owns rows
// b, b + gridDim.x, ...; T threads cover a row, VEC columns each; the column
// sums are fp32, block partials in ascending row order folded in block order.
// dY = Z > 0 ? dZ : 0 copies bf16 bits (exact); written only with relu.
template <int VEC>
__global__ __launch_bounds__(kBlock) void relu_bwd_colsum_bf16_kernel(
    int64_t n, int F, const uint16_t *__restrict__ dZ, const uint16_t *__restrict__ Z, int relu,
    uint16_t *__restrict__ dY, float *__restrict__ partial /*[gridDim.x][F]*/, int T) {
  __shared__ float red[kBlock * VEC];
  const int R = kBlock / T;  // row slots per block iteration
  const int t_col = threadIdx.x % T;
  const int t_row = threadIdx.x / T;
  for (int c0 = 0; c0 < F; c0 += T * VEC) {
    const int f0 = c0 + t_col * VEC;
    const bool f_ok = (t_row < R) && (f0 < F);
    float acc[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[j] = 0.0f;
    if (f_ok) {
      constexpr int kUR = 4;  // rows per step, loads issued before any is used
      const int64_t stride = (int64_t)gridDim.x * R;
      for (int64_t r0 = (int64_t)blockIdx.x * R + t_row; r0 < n; r0 += kUR * stride) {
        float g[kUR][VEC], z[kUR][VEC];
#pragma unroll
        for (int u = 0; u < kUR; ++u) {
          const int64_t r = r0 + u * stride;
          const int64_t off = (r < n ? r : 0) * F + f0;
          load_bf<VEC>(dZ + off, g[u]);
          if (relu) load_bf<VEC>(Z + off, z[u]);
        }
#pragma unroll
        for (int u = 0; u < kUR; ++u) {
          const int64_t r = r0 + u * stride;
          if (r >= n) break;
          if (relu) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) g[u][j] = (z[u][j] > 0.0f) ? g[u][j] : 0.0f;
            if (dY != nullptr) {
              if constexpr (VEC == 8) {
                F32v<8> o;
#pragma unroll
                for (int j = 0; j < 8; ++j) o.v[j] = g[u][j];
                // bf16 values (or +0): the conversion back is exact
                *reinterpret_cast<u32x4 *>(dY + r * F + f0) = round8(o);
              } else {
                dY[r * F + f0] = (uint16_t)(__float_as_uint(g[u][0]) >> 16);
              }
            }
          }
#pragma unroll
          for (int j = 0; j < VEC; ++j) acc[j] = __fadd_rn(acc[j], g[u][j]);
        }
      }
    }
    if (partial == nullptr) continue;
    // fold the R row slots of this block (fixed order)
#pragma unroll
    for (int j = 0; j < VEC; ++j) red[threadIdx.x * VEC + j] = acc[j];
    __syncthreads();
    if (t_row == 0 && f0 < F) {
      float s[VEC];
#pragma unroll
      for (int j = 0; j < VEC; ++j) s[j] = red[t_col * VEC + j];
      for (int rr = 1; rr < R; ++rr)
#pragma unroll
        for (int j = 0; j < VEC; ++j) s[j] = __fadd_rn(s[j], red[(rr * T + t_col) * VEC + j]);
#pragma unroll
      for (int j = 0; j < VEC; ++j) partial[(int64_t)blockIdx.x * F + f0 + j] = s[j];
    }
    __syncthreads();
  }
}

bool rows_ok(int32_t F, const void *p0, int64_t ld0, const void *p1, int64_t ld1) {
  return mgcn_spmm_bf16_supported(F, ld0, ld1) && reinterpret_cast<uintptr_t>(p0) % 16 == 0 &&
         reinterpret_cast<uintptr_t>(p1) % 16 == 0;
}

}  // namespace

}  // namespace mgcn

using namespace mgcn;

extern "C" int mgcn_spmm_bf16_supported(int32_t F, int64_t ld_in, int64_t ld_out) {
  return (F > 0 && F % 8 == 0 && ld_in >= F && ld_out >= F && ld_in % 8 == 0 && ld_out % 8 == 0)
             ? 1 : 0;
}

extern "C" int mgcn_spmm_fwd_bf16(int64_t n_rows, int32_t F, const int64_t *rowptr,
                                  const int32_t *col, const int32_t *eid, const float *w,
                                  const uint16_t *H, int64_t ldh, uint16_t *Y, int64_t ldy,
                                  int reduce, const float *bias, int relu, int32_t *argmax,
                                  uint32_t *win_mask, const int32_t *order, int64_t n_heavy,
                                  int64_t n_giant, void *stream) {
  clear_error();
  MGCN_REQUIRE(n_rows >= 0 && F >= 0, "mgcn_spmm_fwd_bf16: negative size");
  MGCN_REQUIRE(reduce == MGCN_REDUCE_SUM || reduce == MGCN_REDUCE_MEAN || reduce == MGCN_REDUCE_MAX,
               "mgcn_spmm_fwd_bf16: bad reduce %d", reduce);
  MGCN_REQUIRE(F % 8 == 0, "mgcn_spmm_fwd_bf16: F = %d, the bf16 kernels need F %% 8 == 0", F);
  if (n_rows == 0 || F == 0) return MGCN_OK;
  MGCN_REQUIRE(rowptr && H && Y, "mgcn_spmm_fwd_bf16: null array");  // col may be NULL when nnz == 0
  MGCN_REQUIRE(ldh >= F && ldy >= F, "mgcn_spmm_fwd_bf16: leading dimension < F");
  MGCN_REQUIRE(rows_ok(F, H, ldh, Y, ldy),
               "mgcn_spmm_fwd_bf16: rows must be 16-byte aligned (pointer %% 16 == 0, ld %% 8 == 0)");
  MGCN_REQUIRE(reduce != MGCN_REDUCE_MAX || argmax != nullptr || win_mask != nullptr,
               "mgcn_spmm_fwd_bf16: MAX needs argmax and/or win_mask (+ eid)");
  MGCN_REQUIRE(reduce != MGCN_REDUCE_MAX || eid != nullptr, "mgcn_spmm_fwd_bf16: MAX needs eid");
  MGCN_REQUIRE(reduce != MGCN_REDUCE_MAX || reinterpret_cast<uintptr_t>(argmax) % 16 == 0,
               "mgcn_spmm_fwd_bf16: argmax not 16-byte aligned");
  MGCN_REQUIRE(bias == nullptr || reinterpret_cast<uintptr_t>(bias) % 4 == 0,
               "mgcn_spmm_fwd_bf16: bias not 4-byte aligned");
  MGCN_REQUIRE(order == nullptr || (0 <= n_giant && n_giant <= n_heavy && n_heavy <= n_rows),
               "spmm: need 0 <= n_giant <= n_heavy <= n_rows");
  SpmmArgs a{};
  a.n_rows = n_rows;
  a.F = F;
  a.rowptr = rowptr;
  a.col = col;
  a.eid = eid;
  a.w = w;
  a.X = reinterpret_cast<const float *>(H);  // bf16 rows behind SpmmArgs' pointers
  a.ldx = ldh;
  a.Y = reinterpret_cast<float *>(Y);
  a.ldy = ldy;
  a.bias = bias;
  a.argmax_out = reduce == MGCN_REDUCE_MAX ? argmax : nullptr;
  a.win_mask_out = reduce == MGCN_REDUCE_MAX ? win_mask : nullptr;
  a.order = order;
  a.n_heavy = n_heavy;
  a.n_giant = n_giant;
  a.mean = reduce == MGCN_REDUCE_MEAN;
  a.relu = relu != 0;
  hipStream_t s = as_stream(stream);
  if (reduce == MGCN_REDUCE_MAX) return launch_mode<FWD_MAX>(a, s);
  return launch_mode<FWD_SUM>(a, s);
}

extern "C" int mgcn_spmm_bwd_bf16(int64_t n_rows, int32_t F, const int64_t *rowptr_t,
                                  const int32_t *col_t, const int32_t *eid_t, const float *w_t,
                                  const float *row_scale, const uint16_t *dY, int64_t lddy,
                                  uint16_t *dH, int64_t lddh, int reduce, const float *cnt,
                                  const int32_t *argmax, const uint32_t *win_mask,
                                  const int32_t *slot_map, const int32_t *order, int64_t n_heavy,
                                  int64_t n_giant, void *stream) {
  clear_error();
  MGCN_REQUIRE(n_rows >= 0 && F >= 0, "mgcn_spmm_bwd_bf16: negative size");
  MGCN_REQUIRE(reduce == MGCN_REDUCE_SUM || reduce == MGCN_REDUCE_MEAN || reduce == MGCN_REDUCE_MAX,
               "mgcn_spmm_bwd_bf16: bad reduce %d", reduce);
  MGCN_REQUIRE(F % 8 == 0, "mgcn_spmm_bwd_bf16: F = %d, the bf16 kernels need F %% 8 == 0", F);
  if (n_rows == 0 || F == 0) return MGCN_OK;
  MGCN_REQUIRE(rowptr_t && dY && dH, "mgcn_spmm_bwd_bf16: null array");  // col may be NULL when nnz == 0
  MGCN_REQUIRE(lddy >= F && lddh >= F, "mgcn_spmm_bwd_bf16: leading dimension < F");
  MGCN_REQUIRE(rows_ok(F, dY, lddy, dH, lddh),
               "mgcn_spmm_bwd_bf16: rows must be 16-byte aligned (pointer %% 16 == 0, ld %% 8 == 0)");
  MGCN_REQUIRE(reduce != MGCN_REDUCE_MEAN || cnt != nullptr, "mgcn_spmm_bwd_bf16: MEAN needs cnt");
  MGCN_REQUIRE(reduce != MGCN_REDUCE_MAX || argmax != nullptr || win_mask != nullptr,
               "mgcn_spmm_bwd_bf16: MAX needs argmax (+ eid) or win_mask (+ slot_map)");
  MGCN_REQUIRE(win_mask == nullptr || slot_map != nullptr || reduce != MGCN_REDUCE_MAX,
               "mgcn_spmm_bwd_bf16: win_mask needs slot_map");
  const bool by_mask = reduce == MGCN_REDUCE_MAX && win_mask != nullptr;
  MGCN_REQUIRE(reduce != MGCN_REDUCE_MAX || by_mask ||
                   (eid_t != nullptr && reinterpret_cast<uintptr_t>(argmax) % 16 == 0),
               "mgcn_spmm_bwd_bf16: argmax needs eid and a 16-byte aligned pointer");
  MGCN_REQUIRE(order == nullptr || (0 <= n_giant && n_giant <= n_heavy && n_heavy <= n_rows),
               "spmm: need 0 <= n_giant <= n_heavy <= n_rows");
  SpmmArgs a{};
  a.n_rows = n_rows;
  a.F = F;
  a.rowptr = rowptr_t;
  a.col = col_t;
  a.eid = eid_t;
  a.w = w_t;
  a.X = reinterpret_cast<const float *>(dY);
  a.ldx = lddy;
  a.Y = reinterpret_cast<float *>(dH);
  a.ldy = lddh;
  a.row_scale = row_scale;
  a.cnt = cnt;
  a.argmax_in = argmax;
  a.win_mask = by_mask ? win_mask : nullptr;
  a.slot_map = slot_map;
  a.order = order;
  a.n_heavy = n_heavy;
  a.n_giant = n_giant;
  hipStream_t s = as_stream(stream);
  if (reduce == MGCN_REDUCE_MAX)
    return by_mask ? launch_mode<BWD_MAXM>(a, s) : launch_mode<BWD_MAX>(a, s);
  if (reduce == MGCN_REDUCE_MEAN) return launch_mode<BWD_MEAN>(a, s);
  return launch_mode<BWD_SUM>(a, s);
}

extern "C" int mgcn_relu_bwd_colsum_bf16(int64_t n_rows, int32_t F, const uint16_t *dZ,
                                         const uint16_t *Z, int relu, uint16_t *dY, float *db,
                                         void *workspace, size_t workspace_bytes, void *stream) {
  clear_error();
  MGCN_REQUIRE(n_rows >= 0 && F >= 0, "mgcn_relu_bwd_colsum_bf16: negative size");
  hipStream_t s = as_stream(stream);
  if (F == 0) return MGCN_OK;
  if (n_rows == 0) {
    if (db) MGCN_HIP_TRY(hipMemsetAsync(db, 0, sizeof(float) * F, s));
    return MGCN_OK;
  }
  MGCN_REQUIRE(dZ != nullptr, "mgcn_relu_bwd_colsum_bf16: dZ is null");
  MGCN_REQUIRE(!relu || Z != nullptr, "mgcn_relu_bwd_colsum_bf16: relu needs Z");
  const int nblk = colsum_blocks(n_rows);
  float *partial = nullptr;
  if (db != nullptr) {
    const size_t need = mgcn_colsum_workspace_bytes(n_rows, F);
    if (int rc = require_workspace("mgcn_relu_bwd_colsum_bf16", workspace, workspace_bytes, need))
      return rc;
    partial = static_cast<float *>(workspace);
  }
  const bool v8 = (F % 8 == 0) && ((uintptr_t)dZ % 16 == 0) && (!relu || (uintptr_t)Z % 16 == 0) &&
                  (dY == nullptr || (uintptr_t)dY % 16 == 0);
  if (v8) {
    int T = 1;
    while (T < F / 8 && T < kBlock) T <<= 1;
    hipLaunchKernelGGL(relu_bwd_colsum_bf16_kernel<8>, dim3(nblk), dim3(kBlock), 0, s, n_rows, F,
                       dZ, Z, relu, dY, partial, T);
  } else {
    int T = 1;
    while (T < F && T < kBlock) T <<= 1;
    hipLaunchKernelGGL(relu_bwd_colsum_bf16_kernel<1>, dim3(nblk), dim3(kBlock), 0, s, n_rows, F,
                       dZ, Z, relu, dY, partial, T);
  }
  if (int rc = check_launch("relu_bwd_colsum_bf16_kernel")) return rc;
  if (db != nullptr) return launch_colsum_fold(partial, nblk, F, db, s);
  return MGCN_OK;
}
