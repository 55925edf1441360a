// Seeded per-edge random fills for the attention ops (gfx950).
//
//  * mgcn_edge_noise: out[k, h] for slot k of a view (or COO edge k) and head h,
//    a pure function of (kind, seed, offset, COO edge id e = eid[k], h, p):
//    Philox4x32-10 under key = seed and counter (e, h / 4, offset lo, offset hi),
//    output word h % 4, u = (word >> 8) * 2^-24.  UNIFORM stores u, GUMBEL
//    -log(-log(u + 1e-20) + 1e-20) in the reference's fp32 order
//    (graph_hard_attention.py:12-20), DROPOUT u >= p ? 1 / (1 - p) : 0.
//    The value does not depend on the slot, so a view's fill is the COO fill
//    carried to that view's slot order, bit for bit, with no permutation pass.
//
// One work item is (slot, group of four heads): one Philox call, up to four
// values.  With H % 4 == 0 item i stores floats [4 i, 4 i + 4): one 16-byte
// store per lane, consecutive across the wave.  Algorithmic bytes: 4 nnz (eid)
// read + 4 nnz H written.  Ten rounds of two 32 x 32 -> 64 multiplies and two
// logs per value make the Gumbel fill VALU work rather than a pure store
// stream; no LDS, no atomics, a capped grid with a grid-stride loop.

#include "mgcn_internal.h"
#include "philox.h"

namespace mgcn {
namespace {

constexpr int kBlock = 256;
constexpr int kMaxBlocks = 2048;  // grid-stride beyond (cdna_hip_programming.md G11)

template <int KIND>
__device__ __forceinline__ float transform(uint32_t word, float p, float keep_scale) {
  const float u = (float)(word >> 8) * 0x1p-24f;  // exact: 24 bits
  if constexpr (KIND == MGCN_NOISE_GUMBEL) {
    const float a = -logf(__fadd_rn(u, 1e-20f));
    return -logf(__fadd_rn(a, 1e-20f));
  } else if constexpr (KIND == MGCN_NOISE_DROPOUT) {
    return u >= p ? keep_scale : 0.0f;
  } else {
    return u;
  }
}

// V4: H % 4 == 0 and out 16-byte aligned (every item a whole float4)
template <int KIND, bool V4>
__global__ __launch_bounds__(kBlock) void edge_noise_kernel(
    int64_t nnz, int H, int Q /* ceil(H / 4) */, const int32_t *__restrict__ eid, uint32_t key0,
    uint32_t key1, uint32_t off0, uint32_t off1, float p, float keep_scale,
    float *__restrict__ out) {
  const int64_t total = nnz * Q;  // < 2^31 (nnz H < 2^31)
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * kBlock) {
    const uint32_t k = (uint32_t)i / (uint32_t)Q;
    const uint32_t q = (uint32_t)i - k * (uint32_t)Q;
    const uint32_t e = eid != nullptr ? (uint32_t)eid[k] : k;
    uint32_t c[4] = {e, q, off0, off1};
    philox4x32_10(c, key0, key1);
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = transform<KIND>(c[j], p, keep_scale);
    if constexpr (V4) {
      *reinterpret_cast<float4 *>(out + i * 4) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      float *o = out + (int64_t)k * H + q * 4;
      const int left = H - (int)q * 4;  // >= 1
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < left) o[j] = v[j];
    }
  }
}

template <int KIND>
int launch_kind(int64_t nnz, int H, const int32_t *eid, uint64_t seed, uint64_t offset, float p,
                float keep_scale, float *out, hipStream_t s) {
  const int Q = (H + 3) / 4;
  const bool v4 = H % 4 == 0 && (uintptr_t)out % 16 == 0;
  int64_t g = (nnz * Q + kBlock - 1) / kBlock;
  if (g > kMaxBlocks) g = kMaxBlocks;
  const uint32_t key0 = (uint32_t)seed, key1 = (uint32_t)(seed >> 32);
  const uint32_t off0 = (uint32_t)offset, off1 = (uint32_t)(offset >> 32);
  if (v4)
    hipLaunchKernelGGL((edge_noise_kernel<KIND, true>), dim3((unsigned)g), dim3(kBlock), 0, s, nnz,
                       H, Q, eid, key0, key1, off0, off1, p, keep_scale, out);
  else
    hipLaunchKernelGGL((edge_noise_kernel<KIND, false>), dim3((unsigned)g), dim3(kBlock), 0, s,
                       nnz, H, Q, eid, key0, key1, off0, off1, p, keep_scale, out);
  return check_launch("edge_noise_kernel");
}

}  // namespace
}  // namespace mgcn

using namespace mgcn;

extern "C" int mgcn_edge_noise(int kind, uint64_t seed, uint64_t offset, int64_t nnz, int32_t H,
                               const int32_t *eid, float p, float *out, void *stream) {
  clear_error();
  MGCN_REQUIRE(kind == MGCN_NOISE_UNIFORM || kind == MGCN_NOISE_GUMBEL ||
                   kind == MGCN_NOISE_DROPOUT,
               "mgcn_edge_noise: unknown kind %d", kind);
  MGCN_REQUIRE(nnz >= 0, "mgcn_edge_noise: negative nnz");
  MGCN_REQUIRE(H >= 1 && H <= 16 && nnz * (int64_t)H < ((int64_t)1 << 31),
               "mgcn_edge_noise: unsupported shape (H = %d, nnz = %lld): need 1 <= H <= 16, "
               "nnz H < 2^31", H, (long long)nnz);
  // (a NaN p fails both comparisons)
  MGCN_REQUIRE(kind != MGCN_NOISE_DROPOUT || (p >= 0.0f && p <= 1.0f),
               "mgcn_edge_noise: dropout p = %g outside [0, 1]", (double)p);
  if (nnz == 0) return MGCN_OK;
  MGCN_REQUIRE(out != nullptr, "mgcn_edge_noise: out is NULL");
  hipStream_t s = as_stream(stream);
  switch (kind) {
    case MGCN_NOISE_GUMBEL:
      return launch_kind<MGCN_NOISE_GUMBEL>(nnz, H, eid, seed, offset, 0.0f, 0.0f, out, s);
    case MGCN_NOISE_DROPOUT: {
      // one fp32 division; p == 1: the scale is inf and never selected (u < 1)
      const float keep_scale = 1.0f / (1.0f - p);
      return launch_kind<MGCN_NOISE_DROPOUT>(nnz, H, eid, seed, offset, p, keep_scale, out, s);
    }
    default:
      return launch_kind<MGCN_NOISE_UNIFORM>(nnz, H, eid, seed, offset, 0.0f, 0.0f, out, s);
  }
}
