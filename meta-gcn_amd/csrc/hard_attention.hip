// Hard attention over a node's neighbourhood (gfx950): the message passing of
// NodeModelHardAttention (src/gcn_meta/models/graph_hard_attention.py:70-136)
// and VotePoolLayer (gpool_hard_attention.py:214-275).
//
// Training is soft attention with Gumbel noise and a temperature inside the
// logit, l = (act(z) + g) / T: the kernels of attention.h instantiated with
// the hard argument structs (the soft instantiations live in attention.hip,
// a translation unit this file does not touch).  Eval replaces the softmax by
// a per-(row, head) argmax under torch_scatter's tie rule
// (hatt_select_kernel) and the gather by one that loads only the rows of the
// slots with a non-zero coefficient (hatt_gather_kernel): with a one-hot
// alpha that is at most H rows per node instead of the whole neighbourhood.
// Same work split as attention.hip: 4 waves per workgroup, one wave per CSR
// row, grid-stride over rows, no LDS, no atomics, every sum in a fixed order.

#include "attention.h"

namespace mgcn {
namespace {

// -------------------------------------------------- hard attention, eval
// Flat layout: the (value, slot) pair of a head's lanes that wins under
// "greater value, else later slot", left in every lane of that head (power of
// two H) or in the lanes that read it (any H).  Slots are distinct except for
// the "none yet" pair (-1e16f, -1), which loses to any slot of equal value.
__device__ inline void head_argmax(float &v, int &s, int H, int h) {
  if ((H & (H - 1)) == 0) {
    for (int off = 32; off >= H; off >>= 1) {
      const float ov = __shfl_xor(v, off, 64);
      const int os = __shfl_xor(s, off, 64);
      if (ov > v || (ov == v && os > s)) { v = ov; s = os; }
    }
    return;
  }
  float bv = -1e16f;
  int bs = -1;
  for (int g = 0; g < 64 / H; ++g) {
    const float ov = __shfl(v, g * H + h, 64);
    const int os = __shfl(s, g * H + h, 64);
    if (ov > bv || (ov == bv && os > bs)) { bv = ov; bs = os; }
  }
  v = bv;
  s = bs;
}

// One wave per row of any view: every lane scans its own (slot, head) entries
// chunk after chunk with torch_scatter's `>=` rule (the later slot of equal
// values wins), head_argmax combines the lanes of a head under the same rule,
// and a second walk writes the one-hot.
__global__ __launch_bounds__(kAttThreads) void hatt_select_kernel(
    int64_t n_rows, int H, int act, const int64_t *__restrict__ rowptr,
    const int32_t *__restrict__ col, const float *__restrict__ s_row,
    const float *__restrict__ s_col, const float *__restrict__ noise, float *__restrict__ alpha,
    int32_t *__restrict__ winner) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = blockIdx.x * (int64_t)kAttWaves + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kAttWaves;
  const int G = 64 / H;
  const int h = lane % H, kl = lane / H;
  const bool live = lane < G * H;
  for (int64_t row = wave0; row < n_rows; row += nwaves) {
    const int64_t beg = rowptr[row], end = rowptr[row + 1];
    const float sr = s_row[row * H + h];
    float best = -1e16f;
    int slot = -1;
    for (int64_t k0 = beg; k0 < end; k0 += G) {
      const int64_t k = k0 + kl;
      if (live && k < end) {
        float l = att_act(__fadd_rn(sr, s_col[(int64_t)col[k] * H + h]), act);
        if (noise != nullptr) l = __fadd_rn(l, noise[k * H + h]);
        if (l >= best) { best = l; slot = (int)k; }
      }
    }
    head_argmax(best, slot, H, h);
    for (int64_t k0 = beg; k0 < end; k0 += G) {
      const int64_t k = k0 + kl;
      if (live && k < end) alpha[k * H + h] = (int)k == slot ? 1.0f : 0.0f;
    }
    if (lane < H) winner[row * H + lane] = slot;
  }
}

struct GatherArgs {
  int64_t n_rows;
  int H, C;
  const int64_t *rowptr;
  const int32_t *col;
  const float *alpha, *Hp;
  int64_t ldh;
  float *Y;
  int64_t ldy;
};

// att_fwd_kernel's aggregate-only walk, loading only the feature rows of the
// slots with a non-zero coefficient on some head: a ballot over the edge-phase
// lanes gives the chunk's non-zero (slot, head) bits, and the wave pops the
// slots that own one, in slot order, U at a time.  A skipped term would add
// +-0 to an accumulator that starts at +0 and so can never be -0: the bits
// are those of the dense walk.
template <int FPL>
__global__ __launch_bounds__(kAttThreads) void hatt_gather_kernel(GatherArgs a) {
  constexpr int U = gather_unroll<FPL>();
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = blockIdx.x * (int64_t)kAttWaves + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kAttWaves;
  const int H = a.H, G = 64 / a.H, HC = a.H * a.C;
  const int h = lane % H, kl = lane / H;
  const bool live = lane < G * H;
  const uint64_t head_bits = ((uint64_t)1 << H) - 1;
  int hf[FPL];
  feature_heads<FPL>(hf, lane, HC, a.C);
  for (int64_t row = wave0; row < a.n_rows; row += nwaves) {
    const int64_t beg = a.rowptr[row], end = a.rowptr[row + 1];
    float acc[FPL];
#pragma unroll
    for (int i = 0; i < FPL; ++i) acc[i] = 0.0f;
    for (int64_t k0 = beg; k0 < end; k0 += G) {
      const int64_t k = k0 + kl;
      float al = 0.0f;
      if (live && k < end) al = a.alpha[k * H + h];
      uint64_t nz = __ballot(al != 0.0f);
      while (nz != 0) {
        int ks[U];  // the chunk slots of this round, -1: none left
        float hp[U][FPL];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          ks[u] = -1;
          if (nz != 0) {
            ks[u] = __builtin_ctzll(nz) / H;
            nz &= ~(head_bits << (ks[u] * H));
          }
          const bool on = ks[u] >= 0;
          const int64_t c = on ? __builtin_amdgcn_readfirstlane(a.col[k0 + ks[u]]) : 0;
#pragma unroll
          for (int i = 0; i < FPL; ++i) {
            const int f = lane + 64 * i;
            hp[u][i] = (on && f < HC) ? a.Hp[c * a.ldh + f] : 0.0f;
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (ks[u] >= 0) {
#pragma unroll
            for (int i = 0; i < FPL; ++i) {
              const float w = __shfl(al, ks[u] * H + hf[i], 64);
              acc[i] = __fadd_rn(acc[i], __fmul_rn(w, hp[u][i]));
            }
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < FPL; ++i) {
      const int f = lane + 64 * i;
      if (f < HC) a.Y[row * a.ldy + f] = acc[i];
    }
  }
}

}  // namespace
}  // namespace mgcn

using namespace mgcn;

#define HATT_TEMPERATURE_OK(fn, T) \
  MGCN_REQUIRE((T) > 0.0f, fn ": need temperature > 0 (got %g)", (double)(T))

extern "C" int mgcn_hatt_fwd(int64_t n_rows, int64_t nnz, int32_t H, int32_t C,
                             const int64_t *rowptr, const int32_t *col, const float *s_row,
                             const float *s_col, int act, const float *noise, float temperature,
                             const float *alpha_in, const float *mask, const float *Hp,
                             int64_t ldh, float *Y, int64_t ldy, float *alpha, void *stream) {
  clear_error();
  ATT_REQUIRE_SHAPE("mgcn_hatt_fwd", n_rows, nnz, H, C);
  ATT_ACT_OK("mgcn_hatt_fwd", act);
  HATT_TEMPERATURE_OK("mgcn_hatt_fwd", temperature);
  if (n_rows == 0) return MGCN_OK;
  MGCN_REQUIRE(rowptr && Hp && Y, "mgcn_hatt_fwd: null array");
  MGCN_REQUIRE(nnz == 0 || col, "mgcn_hatt_fwd: null col");
  MGCN_REQUIRE(alpha_in != nullptr || (s_row && s_col && (alpha || nnz == 0)),
               "mgcn_hatt_fwd: need alpha_in, or s_row / s_col / alpha");
  MGCN_REQUIRE(ldh >= (int64_t)H * C && ldy >= (int64_t)H * C,
               "mgcn_hatt_fwd: leading dimension too small");
  HardFwdArgs k{{n_rows, H, C, act, rowptr, col, s_row, s_col, alpha_in, mask, Hp, ldh, Y, ldy,
                 alpha},
                noise, temperature};
  hipStream_t s = as_stream(stream);
#define CALL(FPL)                                                                \
  hipLaunchKernelGGL((att_fwd_kernel<FPL, true, HardFwdArgs>), dim3(att_grid(n_rows)), \
                     dim3(kAttThreads), 0, s, k)
  ATT_DISPATCH(H * C, CALL);
#undef CALL
  return check_launch("att_fwd_kernel (hard)");
}

extern "C" int mgcn_hatt_edge_softmax(int64_t n_rows, int64_t nnz, int32_t H,
                                      const int64_t *rowptr, const int32_t *col,
                                      const float *s_row, const float *s_col, int act,
                                      const float *noise, float temperature, float *alpha,
                                      void *stream) {
  clear_error();
  ATT_REQUIRE_SHAPE("mgcn_hatt_edge_softmax", n_rows, nnz, H, 1);
  ATT_ACT_OK("mgcn_hatt_edge_softmax", act);
  HATT_TEMPERATURE_OK("mgcn_hatt_edge_softmax", temperature);
  if (n_rows == 0 || nnz == 0) return MGCN_OK;
  MGCN_REQUIRE(rowptr && col && s_row && s_col && alpha, "mgcn_hatt_edge_softmax: null array");
  HardFwdArgs k{{n_rows, H, 1, act, rowptr, col, s_row, s_col, nullptr, nullptr, nullptr, 0,
                 nullptr, 0, alpha},
                noise, temperature};
  hipLaunchKernelGGL((att_fwd_kernel<1, false, HardFwdArgs>), dim3(att_grid(n_rows)),
                     dim3(kAttThreads), 0, as_stream(stream), k);
  return check_launch("att_fwd_kernel (hard softmax)");
}

extern "C" int mgcn_hatt_bwd_dst(int64_t n_rows, int64_t nnz, int32_t H, int32_t C,
                                 const int64_t *rowptr, const int32_t *col, const float *Hp,
                                 int64_t ldh, const float *dY, int64_t lddy, const float *alpha,
                                 const float *mask, const float *s_row, const float *s_col,
                                 int act, int softmax, float temperature, float *dz,
                                 float *ds_row, void *stream) {
  clear_error();
  ATT_REQUIRE_SHAPE("mgcn_hatt_bwd_dst", n_rows, nnz, H, C);
  ATT_ACT_OK("mgcn_hatt_bwd_dst", act);
  HATT_TEMPERATURE_OK("mgcn_hatt_bwd_dst", temperature);
  if (n_rows == 0) return MGCN_OK;
  MGCN_REQUIRE(rowptr && Hp && dY, "mgcn_hatt_bwd_dst: null array");
  MGCN_REQUIRE(nnz == 0 || (col && dz), "mgcn_hatt_bwd_dst: null col / dz");
  MGCN_REQUIRE(!softmax || (ds_row && s_row && s_col && (alpha || nnz == 0)),
               "mgcn_hatt_bwd_dst: the softmax adjoint needs alpha, s_row, s_col, ds_row");
  MGCN_REQUIRE(ldh >= (int64_t)H * C && lddy >= (int64_t)H * C,
               "mgcn_hatt_bwd_dst: leading dimension too small");
  HardBwdDstArgs k{{n_rows, H, C, act, softmax ? 1 : 0, rowptr, col, Hp, ldh, dY, lddy, alpha,
                    mask, s_row, s_col, dz, ds_row},
                   temperature};
  hipStream_t s = as_stream(stream);
#define CALL(FPL)                                                                    \
  hipLaunchKernelGGL((att_bwd_dst_kernel<FPL, HardBwdDstArgs>), dim3(att_grid(n_rows)), \
                     dim3(kAttThreads), 0, s, k)
  ATT_DISPATCH(H * C, CALL);
#undef CALL
  return check_launch("att_bwd_dst_kernel (hard)");
}

extern "C" int mgcn_hatt_bwd_src(int64_t n_rows, int64_t nnz, int32_t H, int32_t C,
                                 const int64_t *rowptr_t, const int32_t *col_t,
                                 const int32_t *slot_map, const float *dY, int64_t lddy,
                                 const float *alpha, const float *mask, float *dz,
                                 const float *s_row, const float *s_col, int act, int softmax,
                                 float temperature, const float *a, const float *ds_dst,
                                 float *ds_src, float *dHp, int64_t lddh, void *stream) {
  clear_error();
  ATT_REQUIRE_SHAPE("mgcn_hatt_bwd_src", n_rows, nnz, H, C);
  ATT_ACT_OK("mgcn_hatt_bwd_src", act);
  HATT_TEMPERATURE_OK("mgcn_hatt_bwd_src", temperature);
  if (n_rows == 0) return MGCN_OK;
  MGCN_REQUIRE(rowptr_t && dY && a && ds_src && dHp, "mgcn_hatt_bwd_src: null array");
  MGCN_REQUIRE(nnz == 0 || (col_t && slot_map && alpha && dz),
               "mgcn_hatt_bwd_src: null col / slot_map / alpha / dz");
  MGCN_REQUIRE(!softmax || (s_row && s_col),
               "mgcn_hatt_bwd_src: the softmax adjoint needs s_row, s_col");
  MGCN_REQUIRE(lddy >= (int64_t)H * C && lddh >= (int64_t)H * C,
               "mgcn_hatt_bwd_src: leading dimension too small");
  HardBwdSrcArgs k{{n_rows, H, C, act, softmax ? 1 : 0, rowptr_t, col_t, slot_map, dY, lddy,
                    alpha, mask, dz, s_row, s_col, a, ds_dst, ds_src, dHp, lddh},
                   temperature};
  hipStream_t s = as_stream(stream);
#define CALL(FPL)                                                                    \
  hipLaunchKernelGGL((att_bwd_src_kernel<FPL, HardBwdSrcArgs>), dim3(att_grid(n_rows)), \
                     dim3(kAttThreads), 0, s, k)
  ATT_DISPATCH(H * C, CALL);
#undef CALL
  return check_launch("att_bwd_src_kernel (hard)");
}

extern "C" int mgcn_hatt_select(int64_t n_rows, int64_t nnz, int32_t H, const int64_t *rowptr,
                                const int32_t *col, const float *s_row, const float *s_col,
                                int act, const float *noise, float *alpha, int32_t *winner,
                                void *stream) {
  clear_error();
  ATT_REQUIRE_SHAPE("mgcn_hatt_select", n_rows, nnz, H, 1);
  ATT_ACT_OK("mgcn_hatt_select", act);
  if (n_rows == 0) return MGCN_OK;
  MGCN_REQUIRE(rowptr && s_row && winner, "mgcn_hatt_select: null array");
  MGCN_REQUIRE(nnz == 0 || (col && s_col && alpha), "mgcn_hatt_select: null col / s_col / alpha");
  hipLaunchKernelGGL(hatt_select_kernel, dim3(att_grid(n_rows)), dim3(kAttThreads), 0,
                     as_stream(stream), n_rows, (int)H, act, rowptr, col, s_row, s_col, noise,
                     alpha, winner);
  return check_launch("hatt_select_kernel");
}

extern "C" int mgcn_hatt_gather(int64_t n_rows, int64_t nnz, int32_t H, int32_t C,
                                const int64_t *rowptr, const int32_t *col, const float *alpha,
                                const float *Hp, int64_t ldh, float *Y, int64_t ldy,
                                void *stream) {
  clear_error();
  ATT_REQUIRE_SHAPE("mgcn_hatt_gather", n_rows, nnz, H, C);
  if (n_rows == 0) return MGCN_OK;
  MGCN_REQUIRE(rowptr && Hp && Y, "mgcn_hatt_gather: null array");
  MGCN_REQUIRE(nnz == 0 || (col && alpha), "mgcn_hatt_gather: null col / alpha");
  MGCN_REQUIRE(ldh >= (int64_t)H * C && ldy >= (int64_t)H * C,
               "mgcn_hatt_gather: leading dimension too small");
  GatherArgs k{n_rows, H, C, rowptr, col, alpha, Hp, ldh, Y, ldy};
  hipStream_t s = as_stream(stream);
#define CALL(FPL) \
  hipLaunchKernelGGL((hatt_gather_kernel<FPL>), dim3(att_grid(n_rows)), dim3(kAttThreads), 0, s, k)
  ATT_DISPATCH(H * C, CALL);
#undef CALL
  return check_launch("hatt_gather_kernel");
}
