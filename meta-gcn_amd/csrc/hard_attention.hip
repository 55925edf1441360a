// Hard attention over a node's neighbourhood (gfx950): the message passing of
// NodeModelHardAttention (src/gcn_meta/models/graph_hard_attention.py:70-136)
// and VotePoolLayer (gpool_hard_attention.py:214-275).
//
// Training is soft attention with Gumbel noise and a temperature inside the
// logit, l = (act(z) + g) / T: the kernels of attention.h instantiated with
// the hard argument structs through the checked bodies of attention_entry.h
// (the soft instantiations live in attention.hip, a translation unit this
// file does not touch).  Eval replaces the softmax by
// a per-(row, head) argmax under torch_scatter's tie rule
// (hatt_select_kernel) and the gather by one that loads only the rows of the
// slots with a non-zero coefficient (hatt_gather_kernel): with a one-hot
// alpha that is at most H rows per node instead of the whole neighbourhood.
// Same work split as attention.hip: 4 waves per workgroup, one wave per CSR
// row, grid-stride over rows, no LDS, no atomics, every sum in a fixed order.
// The entries that touch a feature row have _bf16 siblings (the row type R of
// attention.h); select and the edge softmax see fp32 scores alone.

#include "attention_entry.h"

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

template <class R>
struct GatherArgsT {
  int64_t n_rows;
  int H, C;
  const int64_t *rowptr;
  const int32_t *col;
  const float *alpha;
  const R *Hp;
  int64_t ldh;
  R *Y;
  int64_t ldy;
};

// att_fwd_kernel's aggregate-only walk, loading only the feature rows of the
// slots with a non-zero coefficient on some head: a ballot over the edge-phase
// lanes gives the chunk's non-zero (slot, head) bits, and the wave pops the
// slots that own one, in slot order, U at a time.  A skipped term would add
// +-0 to an accumulator that starts at +0 and so can never be -0: the bits
// are those of the dense walk.
template <int FPL, class R = float>
__global__ __launch_bounds__(kAttThreads) void hatt_gather_kernel(GatherArgsT<R> a) {
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
            hp[u][i] = row_ld(on && f < HC, a.Hp, c * a.ldh + f);
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
      if (f < HC) row_st(a.Y + row * a.ldy + f, acc[i]);
    }
  }
}

// ------------------------------------------- entry body, per row type R
template <class R>
int hatt_gather(const char *fn, int64_t n_rows, int64_t nnz, int32_t H, int32_t C,
                const int64_t *rowptr, const int32_t *col, const float *alpha, const R *Hp,
                int64_t ldh, R *Y, int64_t ldy, void *stream) {
  clear_error();
  ATT_REQUIRE_SHAPE(fn, n_rows, nnz, H, C);
  if (n_rows == 0) return MGCN_OK;
  MGCN_REQUIRE(rowptr && Hp && Y, "%s: null array", fn);
  MGCN_REQUIRE(nnz == 0 || (col && alpha), "%s: null col / alpha", fn);
  MGCN_REQUIRE(ldh >= (int64_t)H * C && ldy >= (int64_t)H * C,
               "%s: leading dimension too small", fn);
  GatherArgsT<R> k{n_rows, H, C, rowptr, col, alpha, Hp, ldh, Y, ldy};
  hipStream_t s = as_stream(stream);
#define CALL(FPL)                                                                              \
  hipLaunchKernelGGL((hatt_gather_kernel<FPL, R>), dim3(att_grid(n_rows)), dim3(kAttThreads), 0, \
                     s, k)
  ATT_DISPATCH(H * C, CALL);
#undef CALL
  return check_launch("hatt_gather_kernel");
}

}  // namespace
}  // namespace mgcn

using namespace mgcn;

extern "C" int mgcn_hatt_fwd(int64_t n_rows, int64_t nnz, int32_t H, int32_t C,
                             const int64_t *rowptr, const int32_t *col, const float *s_row,
                             const float *s_col, int act, const float *noise, float temperature,
                             const float *alpha_in, const float *mask, const float *Hp,
                             int64_t ldh, float *Y, int64_t ldy, float *alpha, void *stream) {
  HardFwdArgs k{{n_rows, H, C, act, rowptr, col, s_row, s_col, alpha_in, mask, Hp, ldh, Y, ldy,
                 alpha},
                noise, temperature};
  return fwd<true>("mgcn_hatt_fwd", k, nnz, "att_fwd_kernel (hard)", stream);
}

extern "C" int mgcn_hatt_fwd_bf16(int64_t n_rows, int64_t nnz, int32_t H, int32_t C,
                                  const int64_t *rowptr, const int32_t *col, const float *s_row,
                                  const float *s_col, int act, const float *noise,
                                  float temperature, const float *alpha_in, const float *mask,
                                  const uint16_t *Hp, int64_t ldh, uint16_t *Y, int64_t ldy,
                                  float *alpha, void *stream) {
  HardFwdArgsT<uint16_t> k{{n_rows, H, C, act, rowptr, col, s_row, s_col, alpha_in, mask, Hp, ldh,
                            Y, ldy, alpha},
                           noise, temperature};
  return fwd<true>("mgcn_hatt_fwd_bf16", k, nnz, "att_fwd_kernel (hard)", stream);
}

extern "C" int mgcn_hatt_edge_softmax(int64_t n_rows, int64_t nnz, int32_t H,
                                      const int64_t *rowptr, const int32_t *col,
                                      const float *s_row, const float *s_col, int act,
                                      const float *noise, float temperature, float *alpha,
                                      void *stream) {
  HardFwdArgs k{{n_rows, H, 1, act, rowptr, col, s_row, s_col, nullptr, nullptr, nullptr, 0,
                 nullptr, 0, alpha},
                noise, temperature};
  return fwd<false>("mgcn_hatt_edge_softmax", k, nnz, "att_fwd_kernel (hard softmax)", stream);
}

extern "C" int mgcn_hatt_bwd_dst(int64_t n_rows, int64_t nnz, int32_t H, int32_t C,
                                 const int64_t *rowptr, const int32_t *col, const float *Hp,
                                 int64_t ldh, const float *dY, int64_t lddy, const float *alpha,
                                 const float *mask, const float *s_row, const float *s_col,
                                 int act, int softmax, float temperature, float *dz,
                                 float *ds_row, void *stream) {
  HardBwdDstArgs k{{n_rows, H, C, act, softmax ? 1 : 0, rowptr, col, Hp, ldh, dY, lddy,
                    alpha, mask, s_row, s_col, dz, ds_row},
                   temperature};
  return bwd_dst("mgcn_hatt_bwd_dst", k, nnz, "att_bwd_dst_kernel (hard)", stream);
}

extern "C" int mgcn_hatt_bwd_dst_bf16(int64_t n_rows, int64_t nnz, int32_t H, int32_t C,
                                      const int64_t *rowptr, const int32_t *col,
                                      const uint16_t *Hp, int64_t ldh, const uint16_t *dY,
                                      int64_t lddy, const float *alpha, const float *mask,
                                      const float *s_row, const float *s_col, int act,
                                      int softmax, float temperature, float *dz, float *ds_row,
                                      void *stream) {
  HardBwdDstArgsT<uint16_t> k{{n_rows, H, C, act, softmax ? 1 : 0, rowptr, col, Hp, ldh, dY, lddy,
                               alpha, mask, s_row, s_col, dz, ds_row},
                              temperature};
  return bwd_dst("mgcn_hatt_bwd_dst_bf16", k, nnz, "att_bwd_dst_kernel (hard)", stream);
}

extern "C" int mgcn_hatt_bwd_src(int64_t n_rows, int64_t nnz, int32_t H, int32_t C,
                                 const int64_t *rowptr_t, const int32_t *col_t,
                                 const int32_t *slot_map, const float *dY, int64_t lddy,
                                 const float *alpha, const float *mask, float *dz,
                                 const float *s_row, const float *s_col, int act, int softmax,
                                 float temperature, const float *a, const float *ds_dst,
                                 float *ds_src, float *dHp, int64_t lddh, void *stream) {
  HardBwdSrcArgs k{{n_rows, H, C, act, softmax ? 1 : 0, rowptr_t, col_t, slot_map, dY, lddy,
                    alpha, mask, dz, s_row, s_col, a, ds_dst, ds_src, dHp, lddh},
                   temperature};
  return bwd_src("mgcn_hatt_bwd_src", k, nnz, "att_bwd_src_kernel (hard)", stream);
}

extern "C" int mgcn_hatt_bwd_src_bf16(int64_t n_rows, int64_t nnz, int32_t H, int32_t C,
                                      const int64_t *rowptr_t, const int32_t *col_t,
                                      const int32_t *slot_map, const uint16_t *dY, int64_t lddy,
                                      const float *alpha, const float *mask, float *dz,
                                      const float *s_row, const float *s_col, int act,
                                      int softmax, float temperature, const float *a,
                                      const float *ds_dst, float *ds_src, uint16_t *dHp,
                                      int64_t lddh, float *dHp_f32, void *stream) {
  HardBwdSrcArgsT<BwdSrcArgsBf16> k{{{n_rows, H, C, act, softmax ? 1 : 0, rowptr_t, col_t,
                                      slot_map, dY, lddy, alpha, mask, dz, s_row, s_col, a,
                                      ds_dst, ds_src, dHp, lddh},
                                     dHp_f32},
                                    temperature};
  return bwd_src("mgcn_hatt_bwd_src_bf16", k, nnz, "att_bwd_src_kernel (hard)", stream);
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
  return hatt_gather<float>("mgcn_hatt_gather", n_rows, nnz, H, C, rowptr, col, alpha, Hp, ldh, Y,
                            ldy, stream);
}

extern "C" int mgcn_hatt_gather_bf16(int64_t n_rows, int64_t nnz, int32_t H, int32_t C,
                                     const int64_t *rowptr, const int32_t *col,
                                     const float *alpha, const uint16_t *Hp, int64_t ldh,
                                     uint16_t *Y, int64_t ldy, void *stream) {
  return hatt_gather<uint16_t>("mgcn_hatt_gather_bf16", n_rows, nnz, H, C, rowptr, col, alpha, Hp,
                               ldh, Y, ldy, stream);
}
