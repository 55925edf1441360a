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
// grid-stride over rows, a row of any degree walked in chunks; the _sched
// entries of attention_heavy.hip take the rows of more than 128 edges of the
// fp32 launches to workgroups instead, with the same bits):
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
//
// The lane-layout helpers, the softmax + gather kernel and the two adjoint
// kernels live in attention.h, shared with hard_attention.hip; the scores and
// fold kernels and the soft C entries are here.  The entries that walk a view
// (fwd, edge_softmax, bwd_dst, bwd_src) fill an argument struct and call the
// operation's checked body in attention_entry.h.
//
// Every entry that reads or writes a feature row has a _bf16 sibling over
// bf16 rows (the contract at the top of attention.h); the two share one
// kernel source, instantiated per row type.

#include "attention_entry.h"

namespace mgcn {
namespace {

// ------------------------------------------------------------------ scores
template <class R>
struct ScoreArgsT {
  int64_t n;
  int H, C;
  const R *Hp;
  int64_t ldh;
  const float *a;
  float *s_src, *s_dst;
};

template <int FPL, class R = float>
__global__ __launch_bounds__(kAttThreads) void att_scores_kernel(ScoreArgsT<R> a) {
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
      const float x = row_ld(f < HC, a.Hp, row * a.ldh + f);
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

// ------------------------------- 'out': ds_dst and its term of dHp, by row
// The row written is  prev[row] + ds_dst a[:, C:]:  fp32 rows add to dHp in
// place (prev = dHp); bf16 rows take the unrounded fp32 row mgcn_att_bwd_src
// parked (prev [n_rows, H C], compact) and round once at the store.
template <class R>
__device__ inline void att_dst_fold_rows(int64_t n_rows, int H, int C, const int64_t *rowptr,
                                         const float *dz, const float *av, float *ds_dst,
                                         const float *prev, int64_t ldp, R *dHp, int64_t lddh) {
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
      if (f < HC)
        row_st(dHp + row * lddh + f,
               __fadd_rn(prev[row * ldp + f], __fmul_rn(ds, av[(int64_t)hh * 2 * C + C + c])));
    }
  }
}

__global__ __launch_bounds__(kAttThreads) void att_dst_fold_kernel(
    int64_t n_rows, int H, int C, const int64_t *__restrict__ rowptr, const float *__restrict__ dz,
    const float *__restrict__ av, float *__restrict__ ds_dst, float *dHp, int64_t lddh) {
  att_dst_fold_rows<float>(n_rows, H, C, rowptr, dz, av, ds_dst, dHp, lddh, dHp, lddh);
}

__global__ __launch_bounds__(kAttThreads) void att_dst_fold_bf16_kernel(
    int64_t n_rows, int H, int C, const int64_t *__restrict__ rowptr, const float *__restrict__ dz,
    const float *__restrict__ av, float *__restrict__ ds_dst, const float *__restrict__ dHp_f32,
    uint16_t *__restrict__ dHp, int64_t lddh) {
  att_dst_fold_rows<uint16_t>(n_rows, H, C, rowptr, dz, av, ds_dst, dHp_f32, (int64_t)H * C, dHp,
                              lddh);
}

// ------------------------------------------- entry body, per row type R
template <class R>
int att_scores(const char *fn, int64_t n, int32_t H, int32_t C, const R *Hp, int64_t ldh,
               const float *a, float *s_src, float *s_dst, void *stream) {
  clear_error();
  ATT_REQUIRE_SHAPE(fn, n, 0, H, C);
  if (n == 0) return MGCN_OK;
  MGCN_REQUIRE(Hp && a && s_src && s_dst, "%s: null array", fn);
  MGCN_REQUIRE(ldh >= (int64_t)H * C, "%s: leading dimension too small", fn);
  ScoreArgsT<R> k{n, H, C, Hp, ldh, a, s_src, s_dst};
  hipStream_t s = as_stream(stream);
#define CALL(FPL) \
  hipLaunchKernelGGL((att_scores_kernel<FPL, R>), dim3(att_grid(n)), dim3(kAttThreads), 0, s, k)
  ATT_DISPATCH(H * C, CALL);
#undef CALL
  return check_launch("att_scores_kernel");
}

}  // namespace
}  // namespace mgcn

using namespace mgcn;

extern "C" int mgcn_att_scores(int64_t n, int32_t H, int32_t C, const float *Hp, int64_t ldh,
                               const float *a, float *s_src, float *s_dst, void *stream) {
  return att_scores<float>("mgcn_att_scores", n, H, C, Hp, ldh, a, s_src, s_dst, stream);
}

extern "C" int mgcn_att_scores_bf16(int64_t n, int32_t H, int32_t C, const uint16_t *Hp,
                                    int64_t ldh, const float *a, float *s_src, float *s_dst,
                                    void *stream) {
  return att_scores<uint16_t>("mgcn_att_scores_bf16", n, H, C, Hp, ldh, a, s_src, s_dst, stream);
}

extern "C" int mgcn_att_fwd(int64_t n_rows, int64_t nnz, int32_t H, int32_t C,
                            const int64_t *rowptr, const int32_t *col, const float *s_row,
                            const float *s_col, int act, const float *alpha_in,
                            const float *mask, const float *Hp, int64_t ldh, float *Y,
                            int64_t ldy, float *alpha, void *stream) {
  FwdArgs k{n_rows, H, C, act, rowptr, col, s_row, s_col, alpha_in, mask, Hp, ldh, Y, ldy, alpha};
  return fwd<true>("mgcn_att_fwd", k, nnz, "att_fwd_kernel", stream);
}

extern "C" int mgcn_att_fwd_bf16(int64_t n_rows, int64_t nnz, int32_t H, int32_t C,
                                 const int64_t *rowptr, const int32_t *col, const float *s_row,
                                 const float *s_col, int act, const float *alpha_in,
                                 const float *mask, const uint16_t *Hp, int64_t ldh, uint16_t *Y,
                                 int64_t ldy, float *alpha, void *stream) {
  FwdArgsT<uint16_t> k{n_rows, H, C, act, rowptr, col, s_row, s_col, alpha_in, mask, Hp, ldh, Y,
                       ldy, alpha};
  return fwd<true>("mgcn_att_fwd_bf16", k, nnz, "att_fwd_kernel", stream);
}

extern "C" int mgcn_edge_softmax(int64_t n_rows, int64_t nnz, int32_t H, const int64_t *rowptr,
                                 const int32_t *col, const float *s_row, const float *s_col,
                                 int act, float *alpha, void *stream) {
  FwdArgs k{n_rows, H, 1, act, rowptr, col, s_row, s_col, nullptr, nullptr, nullptr, 0,
            nullptr, 0, alpha};
  return fwd<false>("mgcn_edge_softmax", k, nnz, "att_fwd_kernel (softmax)", stream);
}

extern "C" int mgcn_att_bwd_dst(int64_t n_rows, int64_t nnz, int32_t H, int32_t C,
                                const int64_t *rowptr, const int32_t *col, const float *Hp,
                                int64_t ldh, const float *dY, int64_t lddy, const float *alpha,
                                const float *mask, const float *s_row, const float *s_col,
                                int act, int softmax, float *dz, float *ds_row, void *stream) {
  BwdDstArgs k{n_rows, H, C, act, softmax ? 1 : 0, rowptr, col, Hp, ldh, dY, lddy,
               alpha, mask, s_row, s_col, dz, ds_row};
  return bwd_dst("mgcn_att_bwd_dst", k, nnz, "att_bwd_dst_kernel", stream);
}

extern "C" int mgcn_att_bwd_dst_bf16(int64_t n_rows, int64_t nnz, int32_t H, int32_t C,
                                     const int64_t *rowptr, const int32_t *col,
                                     const uint16_t *Hp, int64_t ldh, const uint16_t *dY,
                                     int64_t lddy, const float *alpha, const float *mask,
                                     const float *s_row, const float *s_col, int act, int softmax,
                                     float *dz, float *ds_row, void *stream) {
  BwdDstArgsT<uint16_t> k{n_rows, H, C, act, softmax ? 1 : 0, rowptr, col, Hp, ldh, dY, lddy,
                          alpha, mask, s_row, s_col, dz, ds_row};
  return bwd_dst("mgcn_att_bwd_dst_bf16", k, nnz, "att_bwd_dst_kernel", stream);
}

extern "C" int mgcn_att_bwd_src(int64_t n_rows, int64_t nnz, int32_t H, int32_t C,
                                const int64_t *rowptr_t, const int32_t *col_t,
                                const int32_t *slot_map, const float *dY, int64_t lddy,
                                const float *alpha, const float *mask, float *dz,
                                const float *s_row, const float *s_col, int act, int softmax,
                                const float *a, const float *ds_dst, float *ds_src, float *dHp,
                                int64_t lddh, void *stream) {
  BwdSrcArgs k{n_rows, H, C, act, softmax ? 1 : 0, rowptr_t, col_t, slot_map, dY, lddy,
               alpha, mask, dz, s_row, s_col, a, ds_dst, ds_src, dHp, lddh};
  return bwd_src("mgcn_att_bwd_src", k, nnz, "att_bwd_src_kernel", stream);
}

extern "C" int mgcn_att_bwd_src_bf16(int64_t n_rows, int64_t nnz, int32_t H, int32_t C,
                                     const int64_t *rowptr_t, const int32_t *col_t,
                                     const int32_t *slot_map, const uint16_t *dY, int64_t lddy,
                                     const float *alpha, const float *mask, float *dz,
                                     const float *s_row, const float *s_col, int act, int softmax,
                                     const float *a, const float *ds_dst, float *ds_src,
                                     uint16_t *dHp, int64_t lddh, float *dHp_f32, void *stream) {
  BwdSrcArgsBf16 k{{n_rows, H, C, act, softmax ? 1 : 0, rowptr_t, col_t, slot_map, dY, lddy,
                    alpha, mask, dz, s_row, s_col, a, ds_dst, ds_src, dHp, lddh},
                   dHp_f32};
  return bwd_src("mgcn_att_bwd_src_bf16", k, nnz, "att_bwd_src_kernel", stream);
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

extern "C" int mgcn_att_dst_fold_bf16(int64_t n_rows, int64_t nnz, int32_t H, int32_t C,
                                      const int64_t *rowptr, const float *dz, const float *a,
                                      float *ds_dst, const float *dHp_f32, uint16_t *dHp,
                                      int64_t lddh, void *stream) {
  clear_error();
  ATT_REQUIRE_SHAPE("mgcn_att_dst_fold_bf16", n_rows, nnz, H, C);
  if (n_rows == 0) return MGCN_OK;
  MGCN_REQUIRE(rowptr && a && ds_dst && dHp_f32 && dHp, "mgcn_att_dst_fold_bf16: null array");
  MGCN_REQUIRE(nnz == 0 || dz, "mgcn_att_dst_fold_bf16: null dz");
  MGCN_REQUIRE(lddh >= (int64_t)H * C, "mgcn_att_dst_fold_bf16: leading dimension too small");
  hipLaunchKernelGGL(att_dst_fold_bf16_kernel, dim3(att_grid(n_rows)), dim3(kAttThreads), 0,
                     as_stream(stream), n_rows, (int)H, (int)C, rowptr, dz, a, ds_dst, dHp_f32,
                     dHp, lddh);
  return check_launch("att_dst_fold_bf16_kernel");
}
