// The tile scan (gfx950): an exclusive prefix sum over n items with the
// operation's stores riding in it, shared by derive.hip (stream compaction of
// a parent's views) and block.hip (frontier lists and relabelling).
//
// A three-launch reduce-then-scan over tiles of kTile = 2048 items (256
// threads x 8 items, item i of lane l of a wave at i * 64 + l of the wave's
// 512: every load and store of a wave-instruction is 256 contiguous bytes):
//   tile_count_kernel   per-tile sums (grid-stride over the tiles)
//   tile_scan_kernel    one workgroup: exclusive offsets of the tiles
//   tile_emit_kernel    per tile: the items' exclusive prefixes, and the
//                       operation's stores
// Integer sums in a fixed order, plain vector stores, no atomics, no
// inter-workgroup hand-off inside a launch and no host wait: deterministic.
#pragma once

#include "mgcn_internal.h"

namespace mgcn {
namespace tiles {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kItems = 8;
constexpr int kTile = kBlock * kItems;  // 2048 items per tile
constexpr int kMaxGrid = 1024;          // workgroups of a tile launch (grid-stride beyond)
constexpr int kScanBlock = 1024;        // tile_scan_kernel's one workgroup

inline int64_t tiles_of(int64_t n) { return (n + kTile - 1) / kTile; }
inline unsigned tile_grid(int64_t n_tiles) {
  return static_cast<unsigned>(n_tiles < 1 ? 1 : n_tiles > kMaxGrid ? kMaxGrid : n_tiles);
}

__device__ inline int wave_sum(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// inclusive prefix sum over the wave's 64 lanes
__device__ inline int wave_scan_incl(int v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_up(v, off, 64);
    if (lane >= off) v += t;
  }
  return v;
}

// An operation of the tile scan:
//   first(k)        the item's raw word in the count pass (may store)
//   again(k)        the same word in the emit pass
//   value(raw)      what the item adds to the sum (>= 0)
//   emit(k, p, raw) the item's exclusive prefix p

template <class Op>
__global__ __launch_bounds__(kBlock) void tile_count_kernel(int64_t n, int64_t n_tiles, Op op,
                                                            int32_t *__restrict__ tile_sum) {
  __shared__ int s_wave[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t k0 = tile * kTile + (int64_t)wave * (64 * kItems) + lane;
    int s = 0;
#pragma unroll
    for (int i = 0; i < kItems; ++i) {
      const int64_t k = k0 + (int64_t)i * 64;
      if (k < n) s += Op::value(op.first(k));
    }
    s = wave_sum(s);
    if (lane == 0) s_wave[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      int t = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) t += s_wave[w];
      tile_sum[tile] = t;
    }
    __syncthreads();
  }
}

// tile[j] <- sum of tile[0 .. j), tile[n_tiles] <- the total (also to *total).
// One workgroup; a thread owns a run of consecutive tiles.
static __global__ __launch_bounds__(kScanBlock) void tile_scan_kernel(int64_t n_tiles,
                                                               int32_t *__restrict__ tile,
                                                               int64_t *__restrict__ total) {
  __shared__ int s_wave[kScanBlock / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t chunk = (n_tiles + kScanBlock - 1) / kScanBlock;
  const int64_t a = threadIdx.x * chunk;
  const int64_t b = a + chunk < n_tiles ? a + chunk : n_tiles;
  int s = 0;
  for (int64_t j = a; j < b; ++j) s += tile[j];
  const int inc = wave_scan_incl(s, lane);
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < kScanBlock / 64; ++w) {
    const int t = s_wave[w];
    base += w < wave ? t : 0;
    tot += t;
  }
  int run = base + inc - s;
  for (int64_t j = a; j < b; ++j) {
    const int v = tile[j];
    tile[j] = run;
    run += v;
  }
  if (threadIdx.x == 0) {
    tile[n_tiles] = tot;
    if (total != nullptr) *total = tot;
  }
}

template <class Op>
__global__ __launch_bounds__(kBlock) void tile_emit_kernel(int64_t n, int64_t n_tiles, Op op,
                                                           const int32_t *__restrict__ tile_off) {
  __shared__ int s_wave[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t k0 = tile * kTile + (int64_t)wave * (64 * kItems) + lane;
    int32_t raw[kItems];
    int s = 0;
#pragma unroll
    for (int i = 0; i < kItems; ++i) {
      const int64_t k = k0 + (int64_t)i * 64;
      raw[i] = k < n ? op.again(k) : 0;
      s += k < n ? Op::value(raw[i]) : 0;
    }
    s = wave_sum(s);
    if (lane == 0) s_wave[wave] = s;
    __syncthreads();
    int64_t run = tile_off[tile];
#pragma unroll
    for (int w = 0; w < kWaves; ++w) run += w < wave ? s_wave[w] : 0;
#pragma unroll
    for (int i = 0; i < kItems; ++i) {
      const int64_t k = k0 + (int64_t)i * 64;
      const int v = k < n ? Op::value(raw[i]) : 0;
      const int inc = wave_scan_incl(v, lane);
      if (k < n) op.emit(k, run + inc - v, raw[i]);
      run += __shfl(inc, 63, 64);
    }
    __syncthreads();
  }
}

// count + offsets: tile[0 .. n_tiles] and *total (a device word, may be NULL)
template <class Op>
int tile_scan_sums(int64_t n, const Op &op, int32_t *tile, int64_t *total, hipStream_t s,
                   const char *who) {
  const int64_t n_tiles = tiles_of(n);
  hipLaunchKernelGGL(tile_count_kernel<Op>, dim3(tile_grid(n_tiles)), dim3(kBlock), 0, s, n,
                     n_tiles, op, tile);
  if (int rc = check_launch(who)) return rc;
  hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(kScanBlock), 0, s, n_tiles, tile, total);
  return check_launch(who);
}

// the emit pass over what tile_scan_sums left in `tile`
template <class Op>
int tile_scan_emit(int64_t n, const Op &op, const int32_t *tile, hipStream_t s, const char *who) {
  const int64_t n_tiles = tiles_of(n);
  hipLaunchKernelGGL(tile_emit_kernel<Op>, dim3(tile_grid(n_tiles)), dim3(kBlock), 0, s, n,
                     n_tiles, op, tile);
  return check_launch(who);
}

template <class Op>
int tile_scan(int64_t n, const Op &op, int32_t *tile, int64_t *total, hipStream_t s,
              const char *who) {
  if (int rc = tile_scan_sums(n, op, tile, total, s, who)) return rc;
  return tile_scan_emit(n, op, tile, s, who);
}

}  // namespace tiles
}  // namespace mgcn
