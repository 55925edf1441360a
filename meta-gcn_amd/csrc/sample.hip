// Seeded fan-out-capped neighbour sampling (gfx950): a COO keep mask that
// keeps, in every destination row, the `fanout` candidates of smallest
// (key, COO id), key(e) = word 0 of mgcn_edge_noise's Philox call for head 0.
//
//  * mgcn_sample_rows: keep[e] for every COO edge e of the fwd view (rows =
//    destinations, col = sources), a pure function of (graph, fanout,
//    keep_loops, row_mask, seed, offset): integers only, so neither the slot
//    order, the route of a row nor the launch shape can change a byte.
//
// Two kernels, every row in exactly one of them (the selection they run is
// sample_select.h's light_row / heavy_pick, which block.hip runs too):
//   sample_light_kernel<G>  rows of at most kLight = 128 slots, one lane group
//       of G lanes per row (G from the mean degree).  A row whose candidates
//       fit the fan-out stores its ones without a Philox call.  Otherwise the
//       group forms the 64-bit composites (key << 32) | e in an LDS tile and
//       every slot counts the composites below its own: kept iff rank < fanout.
//   sample_heavy_kernel     one workgroup per longer row: an 8-pass
//       most-significant-byte radix select of the fanout-th smallest composite
//       on an LDS histogram (LDS atomics on the bins), then one pass stores
//       composite <= threshold.  Rows of up to kCap slots hold their keys in
//       LDS; longer ones recompute them in every pass (no upper limit).
//       With a row schedule the workgroups take order[0, n_heavy); without
//       one (SCAN) they walk the row pointers and take what the light kernel
//       leaves: correct, and slower.
// Every COO edge has one slot, so every keep byte has one writer: plain vector
// stores, no global atomics, no workspace.  Algorithmic bytes: 8 (n_rows + 1)
// + nnz (4 + 4 + 1) (rowptr, col, eid, the keep byte).

#include "mgcn_internal.h"
#include "sample_select.h"

namespace mgcn {
namespace {

using namespace sampling;  // the selection itself: sample_select.h

struct SampleArgs : SelectArgs {
  const int32_t *order;
  int64_t n_heavy;
  const uint8_t *row_mask;
  uint8_t *keep;
};

__device__ __forceinline__ void put(const SampleArgs &a, int32_t e, bool v) {
  if ((uint64_t)(uint32_t)e < (uint64_t)a.nnz) a.keep[e] = v ? 1 : 0;
}

template <int G>
__global__ __launch_bounds__(kBlock) void sample_light_kernel(SampleArgs a) {
  constexpr int GPB = kBlock / G;  // rows of a workgroup per round
  __shared__ uint64_t s_tile[GPB * kTileStride];
  const int g = threadIdx.x / G, lg = threadIdx.x % G;
  uint64_t *tile = s_tile + g * kTileStride;
  const int64_t first = a.order != nullptr ? a.n_heavy : 0;
  const int64_t n_items = a.n_rows - first;
  for (int64_t base = (int64_t)blockIdx.x * GPB; base < n_items;
       base += (int64_t)gridDim.x * GPB) {
    const int64_t i = base + g;
    int64_t r = 0, s0 = 0;
    int d = 0;
    if (i < n_items) {
      r = a.order != nullptr ? (int64_t)a.order[first + i] : i;
      if (r >= 0 && r < a.n_rows) {
        s0 = a.rowptr[r];
        const int64_t len = a.rowptr[r + 1] - s0;
        d = (len > 0 && len <= kLight) ? (int)len : 0;  // a longer row: sample_heavy_kernel
      }
    }
    const bool masked = d > 0 && a.row_mask != nullptr && a.row_mask[r] == 0;
    light_row<G>(a, r, s0, d, masked, tile, lg,
                 [&](int, int32_t e, bool kept) { put(a, e, kept); });
  }
}

// One row by the whole workgroup; every branch that returns is uniform.
__device__ void heavy_row(const SampleArgs &a, int64_t r, HeavyLds &s) {
  const int64_t s0 = a.rowptr[r];
  const int64_t d = a.rowptr[r + 1] - s0;
  if (d <= 0) return;
  const bool masked = a.row_mask != nullptr && a.row_mask[r] == 0;
  const HeavyPick p = heavy_pick(a, r, s0, d, masked, s);
  for (int64_t j = threadIdx.x; j < d; j += kBlock) {
    int32_t e;
    const bool kept = heavy_kept(a, p, s, r, s0, j, e);
    put(a, e, kept);
  }
}

template <bool SCAN>
__global__ __launch_bounds__(kBlock) void sample_heavy_kernel(SampleArgs a) {
  __shared__ HeavyLds s;
  if constexpr (!SCAN) {
    for (int64_t i = blockIdx.x; i < a.n_heavy; i += gridDim.x) {
      const int64_t r = a.order[i];
      if (r >= 0 && r < a.n_rows) heavy_row(a, r, s);
      __syncthreads();  // the next row rewrites the LDS
    }
  } else {
    for (int64_t base = (int64_t)blockIdx.x * kBlock; base < a.n_rows;
         base += (int64_t)gridDim.x * kBlock) {
      const int64_t r = base + threadIdx.x;
      const int heavy = (r < a.n_rows && a.rowptr[r + 1] - a.rowptr[r] > kLight) ? 1 : 0;
      s.flag[threadIdx.x] = (uint8_t)heavy;
      if (__syncthreads_or(heavy)) {
        for (int t = 0; t < kBlock; ++t) {
          if (s.flag[t]) {
            heavy_row(a, base + t, s);
            __syncthreads();
          }
        }
      }
      __syncthreads();  // the flags are rewritten next round
    }
  }
}

template <int G>
int launch_light(const SampleArgs &a, int64_t n_items, hipStream_t s) {
  constexpr int GPB = kBlock / G;
  int64_t g = (n_items + GPB - 1) / GPB;
  if (g > kMaxGrid) g = kMaxGrid;
  hipLaunchKernelGGL(sample_light_kernel<G>, dim3((unsigned)g), dim3(kBlock), 0, s, a);
  return check_launch("mgcn_sample_rows (light rows)");
}

}  // namespace
}  // namespace mgcn

using namespace mgcn;

extern "C" size_t mgcn_sample_rows_workspace_bytes(int64_t /*n_rows*/, int64_t /*nnz*/) {
  return 0;  // heavy rows past the LDS capacity recompute their keys
}

extern "C" int mgcn_sample_rows(int64_t n_rows, int64_t nnz, const int64_t *rowptr,
                                const int32_t *col, const int32_t *eid, const int32_t *order,
                                int64_t n_heavy, const uint8_t *row_mask, int32_t fanout,
                                int keep_loops, uint64_t seed, uint64_t offset, uint8_t *keep,
                                void *workspace, size_t workspace_bytes, void *stream) {
  clear_error();
  MGCN_REQUIRE(n_rows >= 0 && nnz >= 0, "mgcn_sample_rows: negative size");
  MGCN_REQUIRE(nnz < (int64_t(1) << 31), "mgcn_sample_rows: nnz must be < 2^31 (int32 eid)");
  MGCN_REQUIRE(fanout >= 0, "mgcn_sample_rows: negative fanout %d", fanout);
  MGCN_REQUIRE(n_heavy >= 0 && n_heavy <= n_rows,
               "mgcn_sample_rows: n_heavy %lld outside [0, n_rows]", (long long)n_heavy);
  MGCN_REQUIRE(order != nullptr || n_heavy == 0,
               "mgcn_sample_rows: n_heavy %lld without a row order", (long long)n_heavy);
  MGCN_REQUIRE(order == nullptr || n_rows < (int64_t(1) << 31),
               "mgcn_sample_rows: a row order needs n_rows < 2^31 (int32 ids)");
  const size_t need = mgcn_sample_rows_workspace_bytes(n_rows, nnz);
  MGCN_REQUIRE(need == 0 || (workspace != nullptr && workspace_bytes >= need),
               "mgcn_sample_rows: workspace %zu < %zu", workspace_bytes, need);
  if (nnz > 0) {
    MGCN_REQUIRE(keep != nullptr, "mgcn_sample_rows: keep is NULL");
    MGCN_REQUIRE(rowptr != nullptr && eid != nullptr, "mgcn_sample_rows: rowptr / eid is NULL");
    MGCN_REQUIRE(col != nullptr || !keep_loops,
                 "mgcn_sample_rows: keep_loops needs col (the sources)");
  }
  if (nnz == 0 || n_rows == 0) return MGCN_OK;
  hipStream_t s = as_stream(stream);
  const SampleArgs a{select_args(n_rows, nnz, rowptr, col, eid, fanout, keep_loops, seed, offset),
                     order, order != nullptr ? n_heavy : 0, row_mask, keep};
  // heavy rows first: the longest work starts earliest
  if (order != nullptr) {
    if (n_heavy > 0) {
      const unsigned g = (unsigned)(n_heavy < kMaxGrid ? n_heavy : kMaxGrid);
      hipLaunchKernelGGL(sample_heavy_kernel<false>, dim3(g), dim3(kBlock), 0, s, a);
      if (int rc = check_launch("mgcn_sample_rows (heavy rows)")) return rc;
    }
  } else {
    hipLaunchKernelGGL(sample_heavy_kernel<true>, dim3(grid_for(n_rows, kBlock)), dim3(kBlock), 0,
                       s, a);
    if (int rc = check_launch("mgcn_sample_rows (row walk)")) return rc;
  }
  const int64_t n_items = n_rows - a.n_heavy;
  if (n_items == 0) return MGCN_OK;
  const int64_t mean = nnz / n_rows;  // lanes per row from the mean degree
  if (mean <= 8) return launch_light<8>(a, n_items, s);
  if (mean <= 16) return launch_light<16>(a, n_items, s);
  if (mean <= 48) return launch_light<32>(a, n_items, s);
  return launch_light<64>(a, n_items, s);
}
