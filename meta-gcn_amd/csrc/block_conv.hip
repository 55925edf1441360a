// Aggregation on a mini-batch block (gfx950): rectangular launches over the
// block's own views with PyG's self-loop rules folded in.
//
// A block (block.hip) has n_dst destinations among n_src nodes; its plan is
// square over n_src with the rows >= n_dst empty.  A convolution on it wants
//     y_i = reduce_{k in row i, counted} X[col_k, :] * w_k  [+ X[i, :] * w_loop]
// for i < n_dst only, under one of three loop rules (include/mgcn.h): KEEP,
// DROP (remove_self_loops) or APPEND (add_remaining_self_loops: the in-row
// loops dropped, one loop term last).  The shipped path edits the edge list in
// torch, builds a plan of the edited list (two sorts and their host waits) and
// aggregates all n_src rows; here the forward launches n_dst rows over the
// block's fwd view and the adjoint n_src rows over its bwd view, and a loop
// slot is recognised where it stands (col == row).
//
// Bits: the order of operations of spmm.hip's FWD_SUM / BWD_SUM / BWD_MEAN --
// slot order = COO order, __fmul_rn then __fadd_rn, mean's __fdiv_rn in the
// forward's epilogue and on the gathered dY in the adjoint -- so a row equals
// the same row of mgcn_spmm_fwd / _bwd on the edited list.  The fold is
// branch-free: a slot that does not count contributes the product -0.0f, and
// x + (-0.0f) == x bit for bit for every x (+0.0f, the accumulator's start,
// included), so it is the row without that slot.  The slot's gather is
// predicated off (its registers hold zeros) and the select discards whatever
// 0 * w would give, so an inf or NaN in a dropped loop's source row or weight
// never reaches the sum.
//
// Layout: spmm_kernel's.  64 lanes = 64 / G row groups of G lanes, a group
// covers G * VEC consecutive features per chunk; (col, w, cnt) are loaded
// lane-parallel, G slots per instruction, and broadcast inside the group; U
// gathers are issued before the ordered fold; the row pointers of the next
// task are loaded while the current one is gathered.  The loop slots of a
// metadata batch are found with one ballot: their number from a popcount, the
// last one's weight (w_loop) from the highest set lane.  The row's own X / dY
// row -- APPEND's last term -- is loaded before the walk, so its latency hides
// behind it.  Rows of any length are walked by their lane group; there is no
// workgroup path here (ops_block_conv.block_conv_supported keeps blocks with
// rows above 128 slots on the shipped path).  No atomics, no workspace.

#include "heavy.h"
#include "mgcn_internal.h"

namespace mgcn {
namespace {

constexpr int kWaves = 4;  // waves per 256-thread block
constexpr int kBlock = 64 * kWaves;

enum BlockMode : int { BK_FWD = 0, BK_BWD_SUM = 1, BK_BWD_MEAN = 2 };

struct BlockArgs {
  int64_t n_rows;  // rows of this launch: n_dst forward, n_src adjoint
  int64_t n_dst;
  int32_t F;
  int32_t n_chunks;
  const int64_t *rowptr;
  const int32_t *col;
  const int32_t *eid;  // adjoint: the COO id of every slot (w's index)
  const float *w;      // nullable
  float fill;
  int loops;
  const float *X;  // gathered operand (X forward, dY adjoint)
  int64_t ldx;
  float *Y;
  int64_t ldy;
  int mean;          // forward: divide by max(c, 1)
  float *cnt_out;    // forward, nullable
  const float *cnt;  // adjoint MEAN
};

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

template <int VEC, int G, int U, int MODE>
__global__ __launch_bounds__(kBlock) void block_spmm_kernel(const BlockArgs a) {
  constexpr int RPW = 64 / G;  // rows per wave
  constexpr bool kBwd = MODE != BK_FWD;
  const int lane = threadIdx.x & 63;
  const int gl = lane & (G - 1);
  const int grp = lane / G;
  const int gbase = grp * G;
  const int wave_in_block = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t n_row_groups = (a.n_rows + RPW - 1) / RPW;
  const int64_t wave_stride = (int64_t)gridDim.x * kWaves;
  const float *__restrict__ X = a.X;
  const bool has_w = a.w != nullptr;
  const bool cut = a.loops != MGCN_LOOPS_KEEP;  // in-row loops do not count
  const bool append = a.loops == MGCN_LOOPS_APPEND;

  // the row pointers of the next task are loaded while this one is gathered
  auto row_of = [&](int64_t wv, bool &ok) -> int64_t {
    const int64_t item = wv * RPW + grp;
    ok = wv < n_row_groups && item < a.n_rows;
    return ok ? item : 0;
  };
  const int64_t wv0 = (int64_t)blockIdx.x * kWaves + wave_in_block;
  bool ok_n;
  int64_t row_n = row_of(wv0, ok_n);
  int64_t beg_n = ok_n ? a.rowptr[row_n] : 0, end_n = ok_n ? a.rowptr[row_n + 1] : 0;
  for (int64_t wv = wv0; wv < n_row_groups; wv += wave_stride) {
    const bool row_ok = ok_n;
    const int64_t row = row_n;
    const int64_t beg = beg_n;
    const int64_t deg = end_n - beg_n;
    row_n = row_of(wv + wave_stride, ok_n);
    beg_n = ok_n ? a.rowptr[row_n] : 0;
    end_n = ok_n ? a.rowptr[row_n + 1] : 0;
    const int64_t maxdeg = (RPW > 1) ? wave_max_over_groups<G>(deg) : deg;
    // APPEND's last term belongs to the destinations: every forward row, the
    // adjoint's rows below n_dst
    const bool has_self = append && row_ok && (!kBwd || row < a.n_dst);

    for (int c = 0; c < a.n_chunks; ++c) {
      const int f0 = (c * G + gl) * VEC;
      const bool f_ok = f0 < a.F;
      F32v<VEC> acc, self;
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        acc.v[j] = 0.0f;
        self.v[j] = 0.0f;
      }
      float self_cnt = 1.0f;
      if (has_self && f_ok) {
        self = load_f<VEC>(X + row * a.ldx + f0);
        if constexpr (MODE == BK_BWD_MEAN) self_cnt = a.cnt[row];
      }
      int n_cut = 0;                          // loop slots of this row
      float w_loop = has_w ? a.fill : 1.0f;   // the weight of APPEND's last term

      for (int64_t e0 = 0; e0 < maxdeg; e0 += G) {
        // lane-parallel metadata for the next (up to) G slots of this row
        const int64_t my = e0 + gl;
        int mc = -1;
        float mw = 1.0f, mcnt = 1.0f;
        bool mloop = false;
        if (my < deg) {
          mc = a.col[beg + my];
          mloop = cut && mc == (int32_t)row;
          if (has_w) mw = kBwd ? a.w[a.eid[beg + my]] : a.w[beg + my];
          if constexpr (MODE == BK_BWD_MEAN) {
            if (!mloop) mcnt = a.cnt[mc];  // (a dropped loop's count may be 0)
          }
        }
        if (cut) {
          const uint64_t wave_bits = __ballot(mloop);
          if (wave_bits != 0) {  // wave-uniform
            const uint64_t bits = (G == 64) ? wave_bits : (wave_bits >> gbase) & ((1ull << (G & 63)) - 1);
            const int last = bits != 0 ? 63 - __clzll((long long)bits) : 0;
            const float wl = __shfl(mw, gbase + last, 64);
            if (bits != 0) {
              w_loop = wl;  // the last loop slot so far: COO order, so the last one wins
              n_cut += __popcll(bits);
            }
            if (mloop) mc = -1;  // not gathered, not folded
          }
        }
        const int64_t remw = maxdeg - e0;
        const int nbmax = remw < G ? (int)remw : G;  // wave-uniform

        for (int k0 = 0; k0 < nbmax; k0 += U) {
          F32v<VEC> xv[U];
          float wk[U];
          bool ok[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int kk = (k0 + u) & (G - 1);
            const int ck = bcast_i<G>(mc, gbase, kk);  // -1: past the row's end, or a cut loop
            wk[u] = bcast_f<G>(mw, gbase, kk);
            float cntk = 1.0f;
            if constexpr (MODE == BK_BWD_MEAN) cntk = bcast_f<G>(mcnt, gbase, kk);
            ok[u] = (k0 + u < nbmax) && ck >= 0 && f_ok;
            if (ok[u]) {
              xv[u] = load_f<VEC>(X + (int64_t)ck * a.ldx + f0);
            } else {
#pragma unroll
              for (int j = 0; j < VEC; ++j) xv[u].v[j] = 0.0f;
            }
            if constexpr (MODE == BK_BWD_MEAN) {
#pragma unroll
              for (int j = 0; j < VEC; ++j) xv[u].v[j] = __fdiv_rn(xv[u].v[j], cntk);
            }
          }
          // fold in strictly ascending slot order; -0.0f stands in for "nothing"
#pragma unroll
          for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
              const float p = ok[u] ? __fmul_rn(xv[u].v[j], wk[u]) : -0.0f;
              acc.v[j] = __fadd_rn(acc.v[j], p);
            }
          }
        }
      }

      const int64_t counted = deg - n_cut + (append ? 1 : 0);
      if constexpr (!kBwd) {
        if (a.cnt_out != nullptr && row_ok && c == 0 && gl == 0) a.cnt_out[row] = (float)counted;
      }
      if (!(row_ok && f_ok)) continue;
      if (has_self) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          float g = self.v[j];
          if constexpr (MODE == BK_BWD_MEAN) g = __fdiv_rn(g, self_cnt);
          acc.v[j] = __fadd_rn(acc.v[j], __fmul_rn(g, w_loop));
        }
      }
      if constexpr (!kBwd) {
        if (a.mean) {
          const float div = (float)(counted > 1 ? counted : 1);
#pragma unroll
          for (int j = 0; j < VEC; ++j) acc.v[j] = __fdiv_rn(acc.v[j], div);
        }
      }
      store_f<VEC>(a.Y + row * a.ldy + f0, acc);
    }
  }
}

int pick_vec(int32_t F, const void *p0, int64_t ld0, const void *p1, int64_t ld1) {
  auto ok = [&](int v) {
    if (F % v) return false;
    if (ld0 % v || ld1 % v) return false;
    if (reinterpret_cast<uintptr_t>(p0) % (4 * v)) return false;
    if (reinterpret_cast<uintptr_t>(p1) % (4 * v)) return false;
    return true;
  };
  int v = ok(4) ? 4 : ok(2) ? 2 : 1;
  if (g_opt.spmm_vec != 0 && g_opt.spmm_vec < v) v = g_opt.spmm_vec;
  return v;
}

template <int VEC, int G, int U, int MODE>
int launch_one(const BlockArgs &a, hipStream_t stream) {
  constexpr int RPW = 64 / G;
  const int64_t waves = (a.n_rows + RPW - 1) / RPW;
  int64_t blocks = (waves + kWaves - 1) / kWaves;
  if (blocks > (int64_t(1) << 20)) blocks = int64_t(1) << 20;  // grid-stride beyond
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL((block_spmm_kernel<VEC, G, U, MODE>), dim3((unsigned)blocks), dim3(kBlock), 0,
                     stream, a);
  return check_launch("block_spmm_kernel");
}

template <int VEC, int MODE>
int launch_g(BlockArgs a, hipStream_t stream) {
  const int lanes = (a.F + VEC - 1) / VEC;
  a.n_chunks = (a.F + 64 * VEC - 1) / (64 * VEC);
  if (lanes > 32) return launch_one<VEC, 64, 8, MODE>(a, stream);
  if (lanes > 16) return launch_one<VEC, 32, 8, MODE>(a, stream);
  if (lanes > 8) return launch_one<VEC, 16, 8, MODE>(a, stream);
  if (lanes > 4) return launch_one<VEC, 8, 8, MODE>(a, stream);
  return launch_one<VEC, 4, 4, MODE>(a, stream);
}

template <int MODE>
int launch_mode(const BlockArgs &a, int vec, hipStream_t stream) {
  return vec == 4   ? launch_g<4, MODE>(a, stream)
         : vec == 2 ? launch_g<2, MODE>(a, stream)
                    : launch_g<1, MODE>(a, stream);
}

// the checks the two entries share
int check_shape(const char *who, int64_t n_dst, int64_t n_src, int32_t F, int loops, int reduce) {
  MGCN_REQUIRE(n_dst >= 0 && n_src >= 0, "%s: negative size", who);
  MGCN_REQUIRE(n_dst <= n_src, "%s: n_dst %lld > n_src %lld", who, (long long)n_dst,
               (long long)n_src);
  MGCN_REQUIRE(n_src < (int64_t(1) << 31), "%s: n_src must be < 2^31 (int32 ids)", who);
  MGCN_REQUIRE(F >= 1, "%s: F must be >= 1, got %d", who, F);
  MGCN_REQUIRE(reduce == MGCN_REDUCE_SUM || reduce == MGCN_REDUCE_MEAN,
               "%s: reduce must be SUM or MEAN, got %d", who, reduce);
  MGCN_REQUIRE(loops == MGCN_LOOPS_KEEP || loops == MGCN_LOOPS_DROP || loops == MGCN_LOOPS_APPEND,
               "%s: bad loops code %d", who, loops);
  return MGCN_OK;
}

}  // namespace
}  // namespace mgcn

using namespace mgcn;

extern "C" int mgcn_block_spmm_fwd(int64_t n_dst, int64_t n_src, int32_t F, const int64_t *rowptr,
                                   const int32_t *col, const float *w, float fill, int loops,
                                   const float *X, int64_t ldx, float *Y, int64_t ldy, int reduce,
                                   float *cnt, void *stream) {
  clear_error();
  if (int rc = check_shape("mgcn_block_spmm_fwd", n_dst, n_src, F, loops, reduce)) return rc;
  MGCN_REQUIRE(ldx >= F && ldy >= F, "mgcn_block_spmm_fwd: leading dimension < F");
  if (n_dst == 0) return MGCN_OK;
  MGCN_REQUIRE(rowptr && X && Y, "mgcn_block_spmm_fwd: rowptr / X / Y is NULL");
  BlockArgs a{};
  a.n_rows = n_dst;
  a.n_dst = n_dst;
  a.F = F;
  a.rowptr = rowptr;
  a.col = col;
  a.w = w;
  a.fill = fill;
  a.loops = loops;
  a.X = X;
  a.ldx = ldx;
  a.Y = Y;
  a.ldy = ldy;
  a.mean = reduce == MGCN_REDUCE_MEAN;
  a.cnt_out = cnt;
  return launch_mode<BK_FWD>(a, pick_vec(F, X, ldx, Y, ldy), as_stream(stream));
}

extern "C" int mgcn_block_spmm_bwd(int64_t n_src, int64_t n_dst, int32_t F,
                                   const int64_t *rowptr_t, const int32_t *col_t,
                                   const int32_t *eid_t, const float *w, float fill, int loops,
                                   const float *dY, int64_t lddy, float *dX, int64_t lddx,
                                   int reduce, const float *cnt, void *stream) {
  clear_error();
  if (int rc = check_shape("mgcn_block_spmm_bwd", n_dst, n_src, F, loops, reduce)) return rc;
  MGCN_REQUIRE(lddy >= F && lddx >= F, "mgcn_block_spmm_bwd: leading dimension < F");
  MGCN_REQUIRE(reduce != MGCN_REDUCE_MEAN || cnt != nullptr || n_dst == 0,
               "mgcn_block_spmm_bwd: MEAN needs cnt (the forward's)");
  if (n_src == 0) return MGCN_OK;
  MGCN_REQUIRE(rowptr_t && dX, "mgcn_block_spmm_bwd: rowptr_t / dX is NULL");
  MGCN_REQUIRE(dY != nullptr || n_dst == 0, "mgcn_block_spmm_bwd: dY is NULL");
  MGCN_REQUIRE(w == nullptr || eid_t != nullptr, "mgcn_block_spmm_bwd: w needs eid_t (its index)");
  BlockArgs a{};
  a.n_rows = n_src;
  a.n_dst = n_dst;
  a.F = F;
  a.rowptr = rowptr_t;
  a.col = col_t;
  a.eid = eid_t;
  a.w = w;
  a.fill = fill;
  a.loops = loops;
  a.X = dY;
  a.ldx = lddy;
  a.Y = dX;
  a.ldy = lddx;
  a.cnt = cnt;
  const int vec = pick_vec(F, dY, lddy, dX, lddx);
  hipStream_t s = as_stream(stream);
  if (reduce == MGCN_REDUCE_MEAN && n_dst > 0) return launch_mode<BK_BWD_MEAN>(a, vec, s);
  return launch_mode<BK_BWD_SUM>(a, vec, s);
}
