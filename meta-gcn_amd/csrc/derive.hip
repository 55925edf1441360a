// Derived graph plans (gfx950): a CSR view of an edge subset of a graph that
// already has one, without sorting.
//
// The child of a planned graph (an edge subset, an induced subgraph, a
// relabelled induced subgraph) keeps the parent's row grouping and the COO
// order inside each row, so each of its CSR views is a STABLE STREAM
// COMPACTION of the parent's view: flag every parent slot (kept / dropped),
// take the exclusive prefix sum of the flags, scatter the kept slots to their
// prefix.  The prefix read at a row's first slot is that row's new row
// pointer.  mgcn_csr_build's radix sort, its index validation and its host
// wait are not needed: the parent was validated.
//
// The scan is tile_scan.h's three-launch reduce-then-scan over tiles of 2048
// items (count, one workgroup of offsets, emit with the operation's stores):
// integer sums in a fixed order, plain vector stores, no atomics, no
// inter-workgroup hand-off inside a launch and no host wait: deterministic.
// Everything is slot-parallel -- a hub row of thousands of edges is spread
// over its slots like any other (a slot's row, where it is needed, comes from
// a binary search on the row pointers, as in edge_norm_kernel).

#include "mgcn_internal.h"
#include "tile_scan.h"

namespace mgcn {
namespace {

using namespace tiles;  // the scan itself: tile_scan.h

// Slots of a parent view: raw = the slot's new COO edge id (-1: dropped),
// kept in `mapped` between the passes (one gather, not two); the emit pass
// overwrites it with the slot's prefix (rowptr_at_kernel reads those).
struct SlotOp {
  const int32_t *col, *eid, *col_map, *eid_new;
  int32_t *mapped;  // [nnz_in]: new edge id, then the slot's prefix
  int32_t *col_out, *eid_out;
  int64_t cap;  // entries of col_out / eid_out
  __device__ int32_t first(int64_t k) const {
    const int32_t ne = eid_new[eid[k]];
    mapped[k] = ne;
    return ne;
  }
  __device__ int32_t again(int64_t k) const { return mapped[k]; }
  __device__ static int value(int32_t raw) { return raw >= 0 ? 1 : 0; }
  __device__ void emit(int64_t k, int64_t p, int32_t raw) const {
    mapped[k] = static_cast<int32_t>(p);
    if (raw >= 0 && p < cap) {
      const int32_t c = col[k];
      col_out[p] = col_map != nullptr ? col_map[c] : c;
      eid_out[p] = raw;
    }
  }
};

// Output rows of a permuted view: raw = kept slots of the row's parent row.
struct RowOp {
  const int32_t *row_src, *rp;  // rp [n_rows_in + 1]: compacted row pointers of the parent rows
  int64_t n_rows_in;
  int64_t *rowptr_out;
  __device__ int32_t first(int64_t r) const {
    const int64_t p = row_src[r];
    return (p >= 0 && p < n_rows_in) ? rp[p + 1] - rp[p] : 0;
  }
  __device__ int32_t again(int64_t r) const { return first(r); }
  __device__ static int value(int32_t raw) { return raw; }
  __device__ void emit(int64_t r, int64_t p, int32_t) const { rowptr_out[r] = p; }
};

// COO edges: raw = the edge's keep flag; eid_new = rank among the kept, or -1.
struct RankOp {
  const uint8_t *flag;
  int32_t *eid_new;
  __device__ int32_t first(int64_t e) const { return flag[e] != 0 ? 1 : 0; }
  __device__ int32_t again(int64_t e) const { return first(e); }
  __device__ static int value(int32_t raw) { return raw; }
  __device__ void emit(int64_t e, int64_t p, int32_t raw) const {
    eid_new[e] = raw != 0 ? static_cast<int32_t>(p) : -1;
  }
};

// out[r] = the prefix at slot rowptr[r] (the total at nnz_in), r in [0, n_rows]
template <class T>
__global__ __launch_bounds__(kBlock) void rowptr_at_kernel(int64_t n_rows, int64_t nnz_in,
                                                           const int64_t *__restrict__ rowptr,
                                                           const int32_t *__restrict__ prefix,
                                                           const int32_t *__restrict__ total,
                                                           T *__restrict__ out) {
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r <= n_rows;
       r += (int64_t)gridDim.x * blockDim.x) {
    const int64_t k = rowptr[r];
    out[r] = static_cast<T>(k >= nnz_in ? *total : prefix[k < 0 ? 0 : k]);
  }
}

// One thread per output slot: its row by binary search on rowptr_out, its
// source the same offset into the parent row's compacted segment.
__global__ __launch_bounds__(kBlock) void segment_copy_kernel(
    int64_t n_rows_out, int64_t n_rows_in, int64_t nnz_out, int64_t nnz_in,
    const int64_t *__restrict__ rowptr_out, const int32_t *__restrict__ row_src,
    const int32_t *__restrict__ rp, const int32_t *__restrict__ col_tmp,
    const int32_t *__restrict__ eid_tmp, int32_t *__restrict__ col_out,
    int32_t *__restrict__ eid_out) {
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < nnz_out;
       j += (int64_t)gridDim.x * blockDim.x) {
    int64_t lo = 0, hi = n_rows_out;  // rowptr_out[lo] <= j < rowptr_out[lo + 1]
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (rowptr_out[mid] <= j)
        lo = mid;
      else
        hi = mid;
    }
    const int64_t p = row_src[lo];
    if (p < 0 || p >= n_rows_in) continue;
    const int64_t s = rp[p] + (j - rowptr_out[lo]);
    if (s < 0 || s >= nnz_in) continue;
    col_out[j] = col_tmp[s];
    eid_out[j] = eid_tmp[s];
  }
}

// flag[e] of every COO edge from the slots of one view: kept, and the slot's
// column mapped.  One thread per slot, no row needed: the other endpoint is the
// column of the edge's slot in the other view, taken by a second launch with
// `narrow` set, which only clears flags (every edge has one slot per view, so
// each byte has one writer per launch).
__global__ __launch_bounds__(kBlock) void edge_flag_kernel(
    int64_t nnz, const int32_t *__restrict__ col, const int32_t *__restrict__ eid,
    const uint8_t *__restrict__ keep, const int32_t *__restrict__ map, int narrow,
    uint8_t *__restrict__ flag) {
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < nnz;
       k += (int64_t)gridDim.x * blockDim.x) {
    const int32_t e = eid[k];
    const bool in = map[col[k]] >= 0;
    if (narrow) {
      if (!in) flag[e] = 0;
    } else {
      flag[e] = (in && (keep == nullptr || keep[e] != 0)) ? 1 : 0;
    }
  }
}

struct DeriveScratch {
  size_t mapped, tile_a, rp, col_tmp, eid_tmp, tile_b, total;
};

DeriveScratch derive_scratch(int64_t n_rows_in, int64_t n_rows_out, int64_t nnz_in,
                             bool permuted) {
  DeriveScratch d{};
  auto words = [](int64_t n) { return align_up(static_cast<size_t>(n > 0 ? n : 1) * 4, 256); };
  size_t o = 0;
  d.mapped = o, o += words(nnz_in);
  d.tile_a = o, o += words(tiles_of(nnz_in) + 1);
  if (permuted) {
    d.rp = o, o += words(n_rows_in + 1);
    d.col_tmp = o, o += words(nnz_in);
    d.eid_tmp = o, o += words(nnz_in);
    d.tile_b = o, o += words(tiles_of(n_rows_out) + 1);
  }
  d.total = o;
  return d;
}

}  // namespace
}  // namespace mgcn

using namespace mgcn;

extern "C" size_t mgcn_csr_derive_workspace_bytes(int64_t n_rows_in, int64_t n_rows_out,
                                                  int64_t nnz_in) {
  // sized for a permuted row_src (the identity form needs the first two parts)
  return derive_scratch(n_rows_in, n_rows_out, nnz_in, true).total;
}

extern "C" int mgcn_csr_derive(int64_t n_rows_in, int64_t n_cols_in, int64_t nnz_in,
                               const int64_t *rowptr, const int32_t *col, const int32_t *eid,
                               const int32_t *row_src, int64_t n_rows_out,
                               const int32_t *col_map, const int32_t *eid_new, int64_t nnz_out,
                               int64_t *rowptr_out, int32_t *col_out, int32_t *eid_out,
                               void *workspace, size_t workspace_bytes, void *stream_) {
  clear_error();
  hipStream_t stream = as_stream(stream_);
  MGCN_REQUIRE(n_rows_in >= 0 && n_cols_in >= 0 && nnz_in >= 0 && n_rows_out >= 0 && nnz_out >= 0,
               "mgcn_csr_derive: negative size");
  MGCN_REQUIRE(nnz_in < (int64_t(1) << 31) && n_rows_in < (int64_t(1) << 31) &&
                   n_rows_out < (int64_t(1) << 31) && n_cols_in < (int64_t(1) << 31),
               "mgcn_csr_derive: sizes must be < 2^31 (int32 col/eid)");
  MGCN_REQUIRE(nnz_out <= nnz_in, "mgcn_csr_derive: nnz_out %lld > nnz_in %lld",
               (long long)nnz_out, (long long)nnz_in);
  MGCN_REQUIRE(row_src != nullptr || n_rows_out == n_rows_in,
               "mgcn_csr_derive: identity row_src needs n_rows_out == n_rows_in");
  MGCN_REQUIRE(rowptr_out != nullptr, "mgcn_csr_derive: rowptr_out is null");
  if (nnz_in == 0 || nnz_out == 0) {
    MGCN_HIP_TRY(hipMemsetAsync(rowptr_out, 0, sizeof(int64_t) * (n_rows_out + 1), stream));
    return MGCN_OK;
  }
  MGCN_REQUIRE(rowptr && col && eid && eid_new && col_out && eid_out,
               "mgcn_csr_derive: null array");
  const bool permuted = row_src != nullptr;
  const DeriveScratch d = derive_scratch(n_rows_in, n_rows_out, nnz_in, permuted);
  if (workspace == nullptr || workspace_bytes < d.total) {
    set_error("mgcn_csr_derive: workspace %zu bytes < required %zu", workspace_bytes, d.total);
    return MGCN_EWORKSPACE;
  }
  char *ws = static_cast<char *>(workspace);
  int32_t *mapped = reinterpret_cast<int32_t *>(ws + d.mapped);
  int32_t *tile_a = reinterpret_cast<int32_t *>(ws + d.tile_a);
  const int64_t n_tiles = tiles_of(nnz_in);

  if (!permuted) {
    // one flat compaction over the slots; rowptr_out[r] = the prefix at rowptr[r]
    const SlotOp op{col, eid, col_map, eid_new, mapped, col_out, eid_out, nnz_out};
    if (int rc = tile_scan(nnz_in, op, tile_a, nullptr, stream, "mgcn_csr_derive (slots)"))
      return rc;
    hipLaunchKernelGGL(rowptr_at_kernel<int64_t>, dim3(grid_for(n_rows_in + 1, kBlock)),
                       dim3(kBlock), 0, stream, n_rows_in, nnz_in, rowptr, mapped,
                       tile_a + n_tiles, rowptr_out);
    return check_launch("mgcn_csr_derive (rowptr)");
  }

  // permuted rows: compact in parent order into the workspace, scan the kept
  // counts of the output rows' parent rows, copy the segments
  int32_t *rp = reinterpret_cast<int32_t *>(ws + d.rp);
  int32_t *col_tmp = reinterpret_cast<int32_t *>(ws + d.col_tmp);
  int32_t *eid_tmp = reinterpret_cast<int32_t *>(ws + d.eid_tmp);
  int32_t *tile_b = reinterpret_cast<int32_t *>(ws + d.tile_b);
  const SlotOp op{col, eid, col_map, eid_new, mapped, col_tmp, eid_tmp, nnz_in};
  if (int rc = tile_scan(nnz_in, op, tile_a, nullptr, stream, "mgcn_csr_derive (slots)")) return rc;
  hipLaunchKernelGGL(rowptr_at_kernel<int32_t>, dim3(grid_for(n_rows_in + 1, kBlock)), dim3(kBlock),
                     0, stream, n_rows_in, nnz_in, rowptr, mapped, tile_a + n_tiles, rp);
  if (int rc = check_launch("mgcn_csr_derive (rowptr)")) return rc;
  if (n_rows_out == 0) {
    MGCN_HIP_TRY(hipMemsetAsync(rowptr_out, 0, sizeof(int64_t), stream));
    return MGCN_OK;
  }
  const RowOp rop{row_src, rp, n_rows_in, rowptr_out};
  if (int rc = tile_scan(n_rows_out, rop, tile_b, rowptr_out + n_rows_out, stream,
                         "mgcn_csr_derive (rows)"))
    return rc;
  hipLaunchKernelGGL(segment_copy_kernel, dim3(grid_for(nnz_out, kBlock)), dim3(kBlock), 0, stream,
                     n_rows_out, n_rows_in, nnz_out, nnz_in, rowptr_out, row_src, rp, col_tmp,
                     eid_tmp, col_out, eid_out);
  return check_launch("mgcn_csr_derive (segments)");
}

extern "C" size_t mgcn_edge_rank_workspace_bytes(int64_t nnz) {
  return align_up(static_cast<size_t>(nnz > 0 ? nnz : 1), 256) +
         align_up(static_cast<size_t>(tiles_of(nnz) + 1) * 4, 256);
}

extern "C" int mgcn_edge_rank(int64_t nnz, const uint8_t *keep, const int32_t *col_a,
                              const int32_t *eid_a, const int32_t *map_a, const int32_t *col_b,
                              const int32_t *eid_b, const int32_t *map_b, int32_t *eid_new,
                              int64_t *total, void *workspace, size_t workspace_bytes,
                              void *stream_) {
  clear_error();
  hipStream_t stream = as_stream(stream_);
  MGCN_REQUIRE(nnz >= 0, "mgcn_edge_rank: negative size");
  MGCN_REQUIRE(nnz < (int64_t(1) << 31), "mgcn_edge_rank: nnz must be < 2^31");
  MGCN_REQUIRE(total != nullptr, "mgcn_edge_rank: total is null");
  if (nnz == 0) {
    MGCN_HIP_TRY(hipMemsetAsync(total, 0, sizeof(int64_t), stream));
    return MGCN_OK;
  }
  const bool mapped = map_a != nullptr || map_b != nullptr;
  MGCN_REQUIRE(eid_new != nullptr, "mgcn_edge_rank: eid_new is null");
  MGCN_REQUIRE(keep != nullptr || mapped, "mgcn_edge_rank: neither a keep mask nor a node map");
  MGCN_REQUIRE((map_a == nullptr || (col_a && eid_a)) && (map_b == nullptr || (col_b && eid_b)),
               "mgcn_edge_rank: a node map needs a view of the graph (col, eid)");
  if (int rc = require_workspace("mgcn_edge_rank", workspace, workspace_bytes,
                                 mgcn_edge_rank_workspace_bytes(nnz)))
    return rc;
  char *ws = static_cast<char *>(workspace);
  uint8_t *flag = reinterpret_cast<uint8_t *>(ws);
  int32_t *tile = reinterpret_cast<int32_t *>(ws + align_up(static_cast<size_t>(nnz), 256));
  if (mapped) {
    const bool both = map_a != nullptr && map_b != nullptr;
    const bool a_first = map_a != nullptr;
    hipLaunchKernelGGL(edge_flag_kernel, dim3(grid_for(nnz, kBlock)), dim3(kBlock), 0, stream, nnz,
                       a_first ? col_a : col_b, a_first ? eid_a : eid_b, keep,
                       a_first ? map_a : map_b, 0, flag);
    if (int rc = check_launch("mgcn_edge_rank (flags)")) return rc;
    if (both) {
      hipLaunchKernelGGL(edge_flag_kernel, dim3(grid_for(nnz, kBlock)), dim3(kBlock), 0, stream,
                         nnz, col_b, eid_b, keep, map_b, 1, flag);
      if (int rc = check_launch("mgcn_edge_rank (flags, other endpoint)")) return rc;
    }
  }
  const RankOp op{mapped ? flag : keep, eid_new};
  return tile_scan(nnz, op, tile, total, stream, "mgcn_edge_rank");
}
