// Seeded fan-out-capped neighbour sampling (gfx950): a COO keep mask that
// keeps, in every destination row, the `fanout` candidates of smallest
// (key, COO id), key(e) = word 0 of mgcn_edge_noise's Philox call for head 0.
//
//  * mgcn_sample_rows: keep[e] for every COO edge e of the fwd view (rows =
//    destinations, col = sources), a pure function of (graph, fanout,
//    keep_loops, row_mask, seed, offset): integers only, so neither the slot
//    order, the route of a row nor the launch shape can change a byte.
//
// Two kernels, every row in exactly one of them:
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
#include "philox.h"

namespace mgcn {
namespace {

constexpr int kBlock = 256;
constexpr int kLight = 128;              // slots of a light row (the row schedule's heavy threshold)
constexpr int kTileStride = kLight + 1;  // u64 entries: the groups' tiles start two banks apart
constexpr int kCap = 7168;               // slots of a heavy row whose keys stay in LDS (56 KB)
constexpr unsigned kMaxGrid = 8192;      // grid-stride beyond (cdna_hip_programming.md G11)
constexpr uint64_t kNotCand = ~uint64_t(0);  // no composite: e < 2^31
static_assert(kBlock == 256, "one thread per bin of the radix histogram");

struct SampleArgs {
  int64_t n_rows, nnz;
  const int64_t *rowptr;
  const int32_t *col, *eid, *order;
  int64_t n_heavy;
  const uint8_t *row_mask;
  uint32_t fanout;
  int keep_loops;
  uint32_t key0, key1, off0, off1;
  uint8_t *keep;
};

// word 0 of mgcn_edge_noise's call for head 0 of COO edge e
__device__ __forceinline__ uint32_t edge_key(const SampleArgs &a, uint32_t e) {
  uint32_t c[4] = {e, 0u, a.off0, a.off1};
  philox4x32_10(c, a.key0, a.key1);
  return c[0];
}

__device__ __forceinline__ void put(const SampleArgs &a, int32_t e, bool v) {
  if ((uint64_t)(uint32_t)e < (uint64_t)a.nnz) a.keep[e] = v ? 1 : 0;
}

// What a row that needs no selection stores in slot k: nothing of a masked
// row, everything where the candidates fit, else (fanout == 0) the loops.
__device__ __forceinline__ bool fill_value(const SampleArgs &a, bool masked, bool all, int64_t r,
                                           int64_t k) {
  if (masked) return false;
  if (all) return true;
  return a.keep_loops && a.col[k] == (int32_t)r;
}

// A group's tile is written and read by lanes of one wave alone, whose LDS
// operations complete in order: no workgroup barrier, only the compiler's.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
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
    // the lane's first slot (the only one of a row of at most G) rides in
    // registers: its eid and col loads go out together
    const bool has0 = lg < d;
    int32_t e0 = 0;
    bool cand0 = false;
    if (has0) {
      e0 = a.eid[s0 + lg];
      cand0 = !a.keep_loops || a.col[s0 + lg] != (int32_t)r;
    }
    int cand = d;
    if (a.keep_loops) {
      int c = cand0 ? 1 : 0;
      for (int j = lg + G; j < d; j += G) c += a.col[s0 + j] != (int32_t)r ? 1 : 0;
#pragma unroll
      for (int off = G / 2; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
      cand = c;
    }
    const bool select = !masked && a.fanout > 0 && (uint32_t)cand > a.fanout;
    uint64_t mine0 = kNotCand;
    if (select) {
      if (has0) {
        if (cand0) mine0 = ((uint64_t)edge_key(a, (uint32_t)e0) << 32) | (uint32_t)e0;
        tile[lg] = mine0;
      }
      for (int j = lg + G; j < d; j += G) {
        const int32_t e = a.eid[s0 + j];
        const bool is_cand = !a.keep_loops || a.col[s0 + j] != (int32_t)r;
        tile[j] = is_cand ? ((uint64_t)edge_key(a, (uint32_t)e) << 32) | (uint32_t)e : kNotCand;
      }
    }
    wave_sync();
    if (select) {
      auto rank_put = [&](uint64_t mine, int32_t e) {
        bool kept = true;
        if (mine != kNotCand) {
          uint32_t rank = 0;
          for (int t = 0; t < d; ++t) rank += tile[t] < mine ? 1u : 0u;
          kept = rank < a.fanout;
        }
        put(a, e, kept);
      };
      if (has0) rank_put(mine0, e0);
      for (int j = lg + G; j < d; j += G) rank_put(tile[j], a.eid[s0 + j]);
    } else if (d > 0) {
      const bool all = (uint32_t)cand <= a.fanout;
      if (has0) put(a, e0, masked ? false : all ? true : (a.keep_loops && !cand0));
      for (int j = lg + G; j < d; j += G)
        put(a, a.eid[s0 + j], fill_value(a, masked, all, r, s0 + j));
    }
    wave_sync();  // the tiles are rewritten next round
  }
}

struct HeavyLds {
  uint32_t key[kCap];
  uint32_t e[kCap];  // bit 31: not a candidate (a kept loop)
  uint32_t hist[256];
  uint32_t wave[kBlock / 64];
  uint32_t bin, excl;
  uint8_t flag[kBlock];
};

// inclusive prefix sum of v over the workgroup's threads; *total: the sum
__device__ inline uint32_t block_scan_incl(uint32_t v, uint32_t *s_wave, uint32_t *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t t = __shfl_up(inc, off, 64);
    if (lane >= off) inc += t;
  }
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  uint32_t base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < kBlock / 64; ++w) {
    const uint32_t t = s_wave[w];
    base += w < wave ? t : 0u;
    tot += t;
  }
  __syncthreads();
  *total = tot;
  return base + inc;
}

// One row by the whole workgroup; every branch that returns is uniform.
__device__ void heavy_row(const SampleArgs &a, int64_t r, HeavyLds &s) {
  const int tid = threadIdx.x;
  const int64_t s0 = a.rowptr[r];
  const int64_t d = a.rowptr[r + 1] - s0;
  if (d <= 0) return;
  const bool masked = a.row_mask != nullptr && a.row_mask[r] == 0;
  uint32_t cand = (uint32_t)d;
  if (!masked && a.keep_loops) {
    uint32_t c = 0;
    for (int64_t j = tid; j < d; j += kBlock) c += a.col[s0 + j] != (int32_t)r ? 1u : 0u;
    block_scan_incl(c, s.wave, &cand);
  }
  if (masked || cand <= a.fanout || a.fanout == 0) {
    const bool all = cand <= a.fanout;
    for (int64_t j = tid; j < d; j += kBlock)
      put(a, a.eid[s0 + j], fill_value(a, masked, all, r, s0 + j));
    return;
  }
  const bool cached = d <= kCap;
  if (cached) {
    for (int64_t j = tid; j < d; j += kBlock) {
      const int32_t e = a.eid[s0 + j];
      const bool is_cand = !a.keep_loops || a.col[s0 + j] != (int32_t)r;
      s.key[j] = is_cand ? edge_key(a, (uint32_t)e) : 0u;
      s.e[j] = (uint32_t)e | (is_cand ? 0u : 0x80000000u);
    }
  }
  // slot j: its COO id, its composite, whether it is a candidate
  auto load = [&](int64_t j, int32_t &e, uint64_t &comp) -> bool {
    if (cached) {
      const uint32_t w = s.e[j];
      e = (int32_t)(w & 0x7fffffffu);
      comp = ((uint64_t)s.key[j] << 32) | (w & 0x7fffffffu);
      return (w >> 31) == 0;
    }
    e = a.eid[s0 + j];
    if (a.keep_loops && a.col[s0 + j] == (int32_t)r) {
      comp = 0;
      return false;
    }
    comp = ((uint64_t)edge_key(a, (uint32_t)e) << 32) | (uint32_t)e;
    return true;
  };
  // the k-th smallest composite (k = fanout < cand), a byte per pass from the top
  uint64_t prefix = 0;
  uint32_t k = a.fanout;
  for (int pass = 7; pass >= 0; --pass) {
    const int shift = pass * 8;
    s.hist[tid] = 0;
    __syncthreads();  // (first pass: the cached keys are in place too)
    for (int64_t j = tid; j < d; j += kBlock) {
      int32_t e;
      uint64_t comp;
      if (load(j, e, comp) && (pass == 7 || (comp >> (shift + 8)) == prefix))
        atomicAdd(&s.hist[(uint32_t)(comp >> shift) & 255u], 1u);
    }
    __syncthreads();
    const uint32_t v = s.hist[tid];
    uint32_t tot;
    const uint32_t inc = block_scan_incl(v, s.wave, &tot);
    if (inc - v < k && k <= inc) {  // one bin: 1 <= k <= tot
      s.bin = (uint32_t)tid;
      s.excl = inc - v;
    }
    __syncthreads();
    prefix = (prefix << 8) | s.bin;
    k -= s.excl;
  }
  for (int64_t j = tid; j < d; j += kBlock) {
    int32_t e;
    uint64_t comp;
    const bool is_cand = load(j, e, comp);
    put(a, e, !is_cand || comp <= prefix);
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
  const SampleArgs a{n_rows, nnz, rowptr, col, eid, order, order != nullptr ? n_heavy : 0,
                     row_mask, (uint32_t)fanout, keep_loops ? 1 : 0, (uint32_t)seed,
                     (uint32_t)(seed >> 32), (uint32_t)offset, (uint32_t)(offset >> 32), keep};
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
