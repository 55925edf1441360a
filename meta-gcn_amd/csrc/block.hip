// Mini-batch blocks (gfx950): one hop of a sampled multi-hop frontier, built
// in time proportional to the frontier.  D = the hop's destination list; the
// block holds, for every row of D in list order, the slots of the parent's fwd
// view that mgcn_sample_rows would keep under (fanout, keep_loops, seed,
// offset) with D as its row mask, compacted in the parent's slot order, and
// the nodes relabelled "destinations first": D in its order, then the other
// sources ascending.
//
// Three entries per hop, a host read between them (the two sizes the caller
// allocates by); no pass touches an array sized by the parent's nnz:
//   mgcn_block_count    node_map[D[i]] = i (the range and repeat checks ride in
//       it), the kept count of every row -- loops + min(fanout, candidates),
//       known without a Philox call: lane groups of 8 count the loops of rows
//       up to 128 slots, a workgroup those of a longer one --, the list of the
//       longer rows (a tile scan over D) and the block's row pointers (another)
//   mgcn_block_fill     the selection of sample_select.h, the longer rows one
//       to a workgroup wherever they stand in D; a kept slot's place is its
//       row pointer plus the kept slots before it in the row (counted in LDS),
//       so neither the launch shape nor the group width can move a byte.  A
//       byte flag per parent node marks the sources; a tile scan over the
//       nodes counts the flagged ones outside D
//   mgcn_block_relabel  that scan's emit pass: local ids and src_ids, then
//       the block's columns and its COO list in local ids
// Several lanes may store the same flag value; every other word has one
// writer.  Plain vector stores, no global atomics, nothing allocated.

#include "mgcn_internal.h"
#include "sample_select.h"
#include "tile_scan.h"

namespace mgcn {
namespace {

namespace sp = sampling;
using tiles::tiles_of;

constexpr int kBlock = 256;
constexpr int kCountG = 8;  // lanes per row of block_count_kernel
constexpr int kMaxHeavyGrid = 1024;
// the meta words (int64, on the device)
constexpr int kMetaNnz = 0, kMetaHeavy = 1, kMetaRange = 2, kMetaRepeat = 3, kMetaNew = 4;

struct BlockScratch {
  size_t cnt, heavy, tile_d, nflag, tile_n, total;
};

BlockScratch block_scratch(int64_t n_nodes, int64_t n_dst) {
  BlockScratch b{};
  auto words = [](int64_t n) { return align_up(static_cast<size_t>(n > 0 ? n : 1) * 4, 256); };
  size_t o = 0;
  b.cnt = o, o += words(n_dst);
  b.heavy = o, o += words(n_dst);
  b.tile_d = o, o += words(tiles_of(n_dst) + 1);
  b.nflag = o, o += align_up(static_cast<size_t>(n_nodes > 0 ? n_nodes : 1), 256);
  b.tile_n = o, o += words(tiles_of(n_nodes) + 1);
  b.total = o;
  return b;
}

__device__ __forceinline__ int32_t kept_count(uint32_t fanout, int64_t deg, int64_t loops) {
  const int64_t cand = deg - loops;
  return (int32_t)(loops + (cand < (int64_t)fanout ? cand : (int64_t)fanout));
}

__global__ __launch_bounds__(kBlock) void block_mark_kernel(int64_t n_nodes,
                                                            const int32_t *__restrict__ dst,
                                                            int64_t n_dst,
                                                            int32_t *__restrict__ node_map,
                                                            int64_t *__restrict__ meta) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_dst;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t v = dst[i];
    if (v < 0 || v >= n_nodes)
      meta[kMetaRange] = 1;
    else
      node_map[v] = (int32_t)i;  // a repeated id: one of its places wins, the other sees it
  }
}

// cnt[i] of every row of D; a row above kLight slots whose loops count waits
// for block_heavy_count_kernel holds 0 until then
__global__ __launch_bounds__(kBlock) void block_count_kernel(
    int64_t n_nodes, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
    const int32_t *__restrict__ dst, int64_t n_dst, uint32_t fanout, int keep_loops,
    const int32_t *__restrict__ node_map, int32_t *__restrict__ cnt, int64_t *__restrict__ meta) {
  constexpr int GPB = kBlock / kCountG;
  const int g = threadIdx.x / kCountG, lg = threadIdx.x % kCountG;
  for (int64_t base = (int64_t)blockIdx.x * GPB; base < n_dst; base += (int64_t)gridDim.x * GPB) {
    const int64_t i = base + g;
    int64_t v = -1, s0 = 0, deg = 0;
    if (i < n_dst) v = dst[i];
    const bool ok = v >= 0 && v < n_nodes;
    if (ok) {
      s0 = rowptr[v];
      deg = rowptr[v + 1] - s0;
      if (lg == 0 && node_map[v] != (int32_t)i) meta[kMetaRepeat] = 1;
    }
    const bool light = deg <= sp::kLight;
    int loops = 0;
    if (keep_loops && light)
      for (int64_t j = lg; j < deg; j += kCountG) loops += col[s0 + j] == (int32_t)v ? 1 : 0;
#pragma unroll
    for (int off = kCountG / 2; off >= 1; off >>= 1) loops += __shfl_xor(loops, off, 64);
    if (i < n_dst && lg == 0)
      cnt[i] = !ok ? 0 : (light || !keep_loops) ? kept_count(fanout, deg, loops) : 0;
  }
}

// Positions of D whose row is longer than kLight, in list order.
struct HeavyOp {
  int64_t n_nodes;
  const int64_t *rowptr;
  const int32_t *dst;
  int32_t *heavy;
  __device__ int32_t first(int64_t i) const {
    const int64_t v = dst[i];
    return (v >= 0 && v < n_nodes && rowptr[v + 1] - rowptr[v] > sp::kLight) ? 1 : 0;
  }
  __device__ int32_t again(int64_t i) const { return first(i); }
  __device__ static int value(int32_t raw) { return raw; }
  __device__ void emit(int64_t i, int64_t p, int32_t raw) const {
    if (raw != 0) heavy[p] = (int32_t)i;
  }
};

// one workgroup per longer row: its loops, then its kept count
__global__ __launch_bounds__(kBlock) void block_heavy_count_kernel(
    const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
    const int32_t *__restrict__ dst, int64_t n_dst, uint32_t fanout,
    const int32_t *__restrict__ heavy, const int64_t *__restrict__ meta,
    int32_t *__restrict__ cnt) {
  __shared__ uint32_t s_wave[kBlock / 64];
  int64_t n_heavy = meta[kMetaHeavy];
  if (n_heavy > n_dst) n_heavy = n_dst;
  for (int64_t h = blockIdx.x; h < n_heavy; h += gridDim.x) {
    const int64_t i = heavy[h];
    const int64_t v = dst[i];
    const int64_t s0 = rowptr[v], deg = rowptr[v + 1] - s0;
    uint32_t c = 0, loops = 0;
    for (int64_t j = threadIdx.x; j < deg; j += kBlock) c += col[s0 + j] == (int32_t)v ? 1u : 0u;
    sp::block_scan_incl(c, s_wave, &loops);
    if (threadIdx.x == 0) cnt[i] = kept_count(fanout, deg, loops);
  }
}

// rowptr_out[i] = kept slots of the rows before i
struct CountOp {
  const int32_t *cnt;
  int64_t *rowptr_out;
  __device__ int32_t first(int64_t i) const { return cnt[i]; }
  __device__ int32_t again(int64_t i) const { return cnt[i]; }
  __device__ static int value(int32_t raw) { return raw; }
  __device__ void emit(int64_t i, int64_t p, int32_t) const { rowptr_out[i] = p; }
};

struct FillArgs : sp::SelectArgs {
  const int32_t *dst;
  int64_t n_dst;
  const int64_t *rowptr_out;
  int64_t nnz_out;
  const int32_t *heavy;
  int64_t n_heavy;
  int32_t *src_out, *eid_out;
  int64_t *dst_out;
  uint8_t *nflag;
};

// block edge p: source c (a parent id), parent COO id e, destination D[i]
__device__ __forceinline__ void store_edge(const FillArgs &a, int64_t p, int32_t c, int32_t e,
                                           int64_t i) {
  if (p < 0 || p >= a.nnz_out) return;
  a.src_out[p] = c;
  a.eid_out[p] = e;
  a.dst_out[p] = i;
  if ((uint64_t)(uint32_t)c < (uint64_t)a.n_rows) a.nflag[c] = 1;
}

template <int G>
__global__ __launch_bounds__(kBlock) void block_fill_light_kernel(FillArgs a) {
  constexpr int GPB = kBlock / G;
  __shared__ uint64_t s_tile[GPB * sp::kTileStride];
  __shared__ uint8_t s_kept[GPB * sp::kLight];
  const int g = threadIdx.x / G, lg = threadIdx.x % G;
  uint64_t *tile = s_tile + g * sp::kTileStride;
  uint8_t *kept_of = s_kept + g * sp::kLight;
  for (int64_t base = (int64_t)blockIdx.x * GPB; base < a.n_dst;
       base += (int64_t)gridDim.x * GPB) {
    const int64_t i = base + g;
    int64_t r = 0, s0 = 0;
    int d = 0;
    if (i < a.n_dst) {
      r = a.dst[i];
      if (r >= 0 && r < a.n_rows) {
        s0 = a.rowptr[r];
        const int64_t len = a.rowptr[r + 1] - s0;
        d = (len > 0 && len <= sp::kLight) ? (int)len : 0;  // a longer row: block_fill_heavy_kernel
      }
    }
    sp::light_row<G>(a, r, s0, d, false, tile, lg,
                     [&](int j, int32_t, bool kept) { kept_of[j] = kept ? 1 : 0; });
    if (d > 0) {
      const int64_t out0 = a.rowptr_out[i];
      for (int j = lg; j < d; j += G) {
        if (kept_of[j] == 0) continue;
        int before = 0;
        for (int t = 0; t < j; ++t) before += kept_of[t];
        store_edge(a, out0 + before, a.col[s0 + j], a.eid[s0 + j], i);
      }
    }
    sp::wave_sync();  // the verdicts are rewritten next round
  }
}

__global__ __launch_bounds__(kBlock) void block_fill_heavy_kernel(FillArgs a) {
  __shared__ sp::HeavyLds s;
  for (int64_t h = blockIdx.x; h < a.n_heavy; h += gridDim.x) {
    const int64_t i = a.heavy[h];
    const int64_t r = (i >= 0 && i < a.n_dst) ? (int64_t)a.dst[i] : -1;
    if (r >= 0 && r < a.n_rows) {  // uniform
      const int64_t s0 = a.rowptr[r];
      const int64_t d = a.rowptr[r + 1] - s0;
      if (d > 0) {
        const sp::HeavyPick p = sp::heavy_pick(a, r, s0, d, false, s);
        int64_t run = a.rowptr_out[i];
        for (int64_t base = 0; base < d; base += kBlock) {
          const int64_t j = base + threadIdx.x;
          int32_t e = 0;
          const bool kept = j < d && sp::heavy_kept(a, p, s, r, s0, j, e);
          uint32_t tot;
          const uint32_t inc = sp::block_scan_incl(kept ? 1u : 0u, s.wave, &tot);
          if (kept) store_edge(a, run + inc - 1, a.col[s0 + j], e, i);
          run += tot;
        }
      }
    }
    __syncthreads();  // the next row rewrites the LDS
  }
}

// Parent nodes: raw = a flagged source outside D (kept in nflag between the
// passes); the emit pass gives it the local id n_dst + its rank.
struct NewOp {
  uint8_t *nflag;
  int32_t *node_map;
  int64_t *src_ids;
  int64_t n_dst, n_src;
  __device__ int32_t first(int64_t v) const {
    const int32_t f = (nflag[v] != 0 && node_map[v] < 0) ? 1 : 0;
    nflag[v] = (uint8_t)f;
    return f;
  }
  __device__ int32_t again(int64_t v) const { return nflag[v]; }
  __device__ static int value(int32_t raw) { return raw; }
  __device__ void emit(int64_t v, int64_t p, int32_t raw) const {
    const int64_t l = n_dst + p;
    if (raw != 0 && l < n_src) {
      node_map[v] = (int32_t)l;
      src_ids[l] = v;
    }
  }
};

__global__ __launch_bounds__(kBlock) void block_ids_kernel(const int32_t *__restrict__ dst,
                                                           int64_t n_dst, int64_t n_src,
                                                           int64_t *__restrict__ src_ids) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_dst && i < n_src;
       i += (int64_t)gridDim.x * blockDim.x)
    src_ids[i] = dst[i];
}

__global__ __launch_bounds__(kBlock) void block_cols_kernel(int64_t n_nodes, int64_t nnz_out,
                                                            const int32_t *__restrict__ src_out,
                                                            const int32_t *__restrict__ node_map,
                                                            int32_t *__restrict__ col_out,
                                                            int64_t *__restrict__ coo_src) {
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < nnz_out;
       p += (int64_t)gridDim.x * blockDim.x) {
    const int32_t c = src_out[p];
    const int32_t l = (uint64_t)(uint32_t)c < (uint64_t)n_nodes ? node_map[c] : -1;
    col_out[p] = l;
    coo_src[p] = l;
  }
}

template <int G>
int launch_fill_light(const FillArgs &a, hipStream_t s) {
  constexpr int GPB = kBlock / G;
  int64_t g = (a.n_dst + GPB - 1) / GPB;
  if (g > sp::kMaxGrid) g = sp::kMaxGrid;
  hipLaunchKernelGGL(block_fill_light_kernel<G>, dim3((unsigned)g), dim3(kBlock), 0, s, a);
  return check_launch("mgcn_block_fill (light rows)");
}

// the size checks the three entries share
int check_sizes(const char *who, int64_t n_nodes, int64_t nnz, int64_t n_dst) {
  MGCN_REQUIRE(n_nodes >= 0 && nnz >= 0 && n_dst >= 0, "%s: negative size", who);
  MGCN_REQUIRE(nnz < (int64_t(1) << 31), "%s: nnz must be < 2^31 (int32 eid)", who);
  MGCN_REQUIRE(n_nodes < (int64_t(1) << 31), "%s: n_nodes must be < 2^31 (int32 ids)", who);
  MGCN_REQUIRE(n_dst < (int64_t(1) << 31), "%s: n_dst must be < 2^31 (int32 ids)", who);
  return MGCN_OK;
}

}  // namespace
}  // namespace mgcn

using namespace mgcn;

extern "C" size_t mgcn_block_workspace_bytes(int64_t n_nodes, int64_t n_dst) {
  return block_scratch(n_nodes, n_dst).total;
}

extern "C" int mgcn_block_count(int64_t n_nodes, int64_t nnz, const int64_t *rowptr,
                                const int32_t *col, const int32_t *dst, int64_t n_dst,
                                int32_t fanout, int keep_loops, int32_t *node_map,
                                int64_t *rowptr_out, int64_t *meta, void *workspace,
                                size_t workspace_bytes, void *stream) {
  clear_error();
  if (int rc = check_sizes("mgcn_block_count", n_nodes, nnz, n_dst)) return rc;
  MGCN_REQUIRE(fanout >= 0, "mgcn_block_count: negative fanout %d", fanout);
  MGCN_REQUIRE(rowptr_out != nullptr && meta != nullptr,
               "mgcn_block_count: rowptr_out / meta is NULL");
  MGCN_REQUIRE(node_map != nullptr || n_nodes == 0, "mgcn_block_count: node_map is NULL");
  if (n_dst > 0) {
    MGCN_REQUIRE(dst != nullptr && rowptr != nullptr, "mgcn_block_count: dst / rowptr is NULL");
    MGCN_REQUIRE(nnz == 0 || col != nullptr || !keep_loops,
                 "mgcn_block_count: keep_loops needs col (the sources)");
  }
  const BlockScratch b = block_scratch(n_nodes, n_dst);
  if (int rc = require_workspace("mgcn_block_count", workspace, workspace_bytes, b.total))
    return rc;
  hipStream_t s = as_stream(stream);
  MGCN_HIP_TRY(hipMemsetAsync(meta, 0, sizeof(int64_t) * 5, s));
  if (n_nodes > 0) MGCN_HIP_TRY(hipMemsetAsync(node_map, 0xff, sizeof(int32_t) * n_nodes, s));
  if (n_dst == 0) {
    MGCN_HIP_TRY(hipMemsetAsync(rowptr_out, 0, sizeof(int64_t), s));
    return MGCN_OK;
  }
  char *ws = static_cast<char *>(workspace);
  int32_t *cnt = reinterpret_cast<int32_t *>(ws + b.cnt);
  int32_t *heavy = reinterpret_cast<int32_t *>(ws + b.heavy);
  int32_t *tile_d = reinterpret_cast<int32_t *>(ws + b.tile_d);
  hipLaunchKernelGGL(block_mark_kernel, dim3(grid_for(n_dst, kBlock)), dim3(kBlock), 0, s, n_nodes,
                     dst, n_dst, node_map, meta);
  if (int rc = check_launch("mgcn_block_count (mark)")) return rc;
  hipLaunchKernelGGL(block_count_kernel, dim3(grid_for(n_dst, kBlock / kCountG)), dim3(kBlock), 0,
                     s, n_nodes, rowptr, col, dst, n_dst, (uint32_t)fanout, keep_loops ? 1 : 0,
                     node_map, cnt, meta);
  if (int rc = check_launch("mgcn_block_count (counts)")) return rc;
  const HeavyOp hop{n_nodes, rowptr, dst, heavy};
  if (int rc = tiles::tile_scan(n_dst, hop, tile_d, meta + kMetaHeavy, s,
                                "mgcn_block_count (longer rows)"))
    return rc;
  if (keep_loops && nnz > sp::kLight) {
    int64_t g = nnz / (sp::kLight + 1);  // no more rows than that are longer
    if (g > n_dst) g = n_dst;
    if (g > kMaxHeavyGrid) g = kMaxHeavyGrid;
    hipLaunchKernelGGL(block_heavy_count_kernel, dim3((unsigned)g), dim3(kBlock), 0, s, rowptr,
                       col, dst, n_dst, (uint32_t)fanout, heavy, meta, cnt);
    if (int rc = check_launch("mgcn_block_count (longer rows' loops)")) return rc;
  }
  const CountOp cop{cnt, rowptr_out};
  if (int rc = tiles::tile_scan(n_dst, cop, tile_d, rowptr_out + n_dst, s,
                                "mgcn_block_count (row pointers)"))
    return rc;
  MGCN_HIP_TRY(hipMemcpyAsync(meta + kMetaNnz, rowptr_out + n_dst, sizeof(int64_t),
                              hipMemcpyDeviceToDevice, s));
  return MGCN_OK;
}

extern "C" int mgcn_block_fill(int64_t n_nodes, int64_t nnz, const int64_t *rowptr,
                               const int32_t *col, const int32_t *eid, const int32_t *dst,
                               int64_t n_dst, int32_t fanout, int keep_loops, uint64_t seed,
                               uint64_t offset, const int64_t *rowptr_out, int64_t nnz_out,
                               int64_t n_heavy, const int32_t *node_map, int32_t *src_out,
                               int32_t *eid_out, int64_t *dst_out, int64_t *meta, void *workspace,
                               size_t workspace_bytes, void *stream) {
  clear_error();
  if (int rc = check_sizes("mgcn_block_fill", n_nodes, nnz, n_dst)) return rc;
  MGCN_REQUIRE(fanout >= 0, "mgcn_block_fill: negative fanout %d", fanout);
  MGCN_REQUIRE(nnz_out >= 0 && nnz_out <= nnz, "mgcn_block_fill: nnz_out %lld outside [0, nnz]",
               (long long)nnz_out);
  MGCN_REQUIRE(n_heavy >= 0 && n_heavy <= n_dst, "mgcn_block_fill: n_heavy %lld outside [0, n_dst]",
               (long long)n_heavy);
  MGCN_REQUIRE(meta != nullptr, "mgcn_block_fill: meta is NULL");
  if (nnz_out > 0) {
    MGCN_REQUIRE(rowptr && col && eid && dst && rowptr_out && node_map,
                 "mgcn_block_fill: a graph or list array is NULL");
    MGCN_REQUIRE(src_out && eid_out && dst_out, "mgcn_block_fill: an output array is NULL");
  }
  const BlockScratch b = block_scratch(n_nodes, n_dst);
  if (int rc = require_workspace("mgcn_block_fill", workspace, workspace_bytes, b.total)) return rc;
  hipStream_t s = as_stream(stream);
  if (nnz_out == 0) {
    MGCN_HIP_TRY(hipMemsetAsync(meta + kMetaNew, 0, sizeof(int64_t), s));
    return MGCN_OK;
  }
  char *ws = static_cast<char *>(workspace);
  uint8_t *nflag = reinterpret_cast<uint8_t *>(ws + b.nflag);
  int32_t *tile_n = reinterpret_cast<int32_t *>(ws + b.tile_n);
  MGCN_HIP_TRY(hipMemsetAsync(nflag, 0, static_cast<size_t>(n_nodes), s));
  const FillArgs a{sp::select_args(n_nodes, nnz, rowptr, col, eid, fanout, keep_loops, seed,
                                   offset),
                   dst, n_dst, rowptr_out, nnz_out,
                   reinterpret_cast<const int32_t *>(ws + b.heavy), n_heavy, src_out, eid_out,
                   dst_out, nflag};
  // the longer rows first: the longest work starts earliest
  if (n_heavy > 0) {
    const unsigned g = (unsigned)(n_heavy < sp::kMaxGrid ? n_heavy : sp::kMaxGrid);
    hipLaunchKernelGGL(block_fill_heavy_kernel, dim3(g), dim3(kBlock), 0, s, a);
    if (int rc = check_launch("mgcn_block_fill (longer rows)")) return rc;
  }
  if (n_heavy < n_dst) {
    const int64_t mean = nnz / n_nodes;  // lanes per row from the parent's mean degree
    int rc;
    if (mean <= 8)
      rc = launch_fill_light<8>(a, s);
    else if (mean <= 16)
      rc = launch_fill_light<16>(a, s);
    else if (mean <= 48)
      rc = launch_fill_light<32>(a, s);
    else
      rc = launch_fill_light<64>(a, s);
    if (rc) return rc;
  }
  const NewOp nop{nflag, const_cast<int32_t *>(node_map), nullptr, n_dst, n_dst};
  return tiles::tile_scan_sums(n_nodes, nop, tile_n, meta + kMetaNew, s,
                               "mgcn_block_fill (new nodes)");
}

extern "C" int mgcn_block_relabel(int64_t n_nodes, const int32_t *dst, int64_t n_dst,
                                  int64_t n_src, int64_t nnz_out, const int32_t *src_out,
                                  int32_t *node_map, int64_t *src_ids, int32_t *col_out,
                                  int64_t *coo_src, void *workspace, size_t workspace_bytes,
                                  void *stream) {
  clear_error();
  if (int rc = check_sizes("mgcn_block_relabel", n_nodes, nnz_out, n_dst)) return rc;
  MGCN_REQUIRE(n_src >= n_dst && n_src <= n_nodes,
               "mgcn_block_relabel: n_src %lld outside [n_dst, n_nodes]", (long long)n_src);
  MGCN_REQUIRE(n_src == n_dst || nnz_out > 0, "mgcn_block_relabel: new nodes without an edge");
  if (n_src > 0)
    MGCN_REQUIRE(src_ids != nullptr && (dst != nullptr || n_dst == 0),
                 "mgcn_block_relabel: src_ids / dst is NULL");
  if (nnz_out > 0)
    MGCN_REQUIRE(src_out && node_map && col_out && coo_src, "mgcn_block_relabel: NULL array");
  const BlockScratch b = block_scratch(n_nodes, n_dst);
  if (int rc = require_workspace("mgcn_block_relabel", workspace, workspace_bytes, b.total))
    return rc;
  hipStream_t s = as_stream(stream);
  if (n_dst > 0) {
    hipLaunchKernelGGL(block_ids_kernel, dim3(grid_for(n_dst, kBlock)), dim3(kBlock), 0, s, dst,
                       n_dst, n_src, src_ids);
    if (int rc = check_launch("mgcn_block_relabel (destinations)")) return rc;
  }
  if (nnz_out == 0) return MGCN_OK;
  char *ws = static_cast<char *>(workspace);
  const NewOp nop{reinterpret_cast<uint8_t *>(ws + b.nflag), node_map, src_ids, n_dst, n_src};
  if (int rc = tiles::tile_scan_emit(n_nodes, nop, reinterpret_cast<int32_t *>(ws + b.tile_n), s,
                                     "mgcn_block_relabel (new nodes)"))
    return rc;
  hipLaunchKernelGGL(block_cols_kernel, dim3(grid_for(nnz_out, kBlock)), dim3(kBlock), 0, s,
                     n_nodes, nnz_out, src_out, node_map, col_out, coo_src);
  return check_launch("mgcn_block_relabel (columns)");
}
