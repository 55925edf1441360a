// The row selection of neighbour sampling (gfx950), shared by sample.hip (the
// COO keep mask) and block.hip (compacted mini-batch blocks): which slots of
// one destination row of a fwd view stay under a fan-out cap -- the `fanout`
// candidates of smallest (key, COO id), key(e) = word 0 of mgcn_edge_noise's
// Philox call for head 0.  Integers only; what a caller does with a slot's
// verdict is its own business.
//
//   light_row<G>   a row of at most kLight = 128 slots by one lane group of G
//       lanes.  A row whose candidates fit the fan-out decides without a
//       Philox call.  Otherwise the group forms the 64-bit composites
//       (key << 32) | e in an LDS tile and every slot counts the composites
//       below its own: kept iff rank < fanout.
//   heavy_pick / heavy_kept   a longer row by a whole workgroup: an 8-pass
//       most-significant-byte radix select of the fanout-th smallest composite
//       on an LDS histogram (LDS atomics on the bins); a slot is kept iff its
//       composite <= that threshold.  Rows of up to kCap slots hold their keys
//       in LDS; longer ones recompute them in every pass (no upper limit).
#pragma once

#include "mgcn_internal.h"
#include "philox.h"

namespace mgcn {
namespace sampling {

constexpr int kBlock = 256;
constexpr int kLight = 128;              // slots of a light row (the schedule's heavy threshold)
constexpr int kTileStride = kLight + 1;  // u64 entries: the groups' tiles start two banks apart
constexpr int kCap = 7168;               // slots of a heavy row whose keys stay in LDS (56 KB)
constexpr unsigned kMaxGrid = 8192;      // grid-stride beyond (cdna_hip_programming.md G11)
constexpr uint64_t kNotCand = ~uint64_t(0);  // no composite: e < 2^31
static_assert(kBlock == 256, "one thread per bin of the radix histogram");

// What the selection reads: the fwd view, the cap and the Philox words.
struct SelectArgs {
  int64_t n_rows, nnz;
  const int64_t *rowptr;
  const int32_t *col, *eid;
  uint32_t fanout;
  int keep_loops;
  uint32_t key0, key1, off0, off1;
};

inline SelectArgs select_args(int64_t n_rows, int64_t nnz, const int64_t *rowptr,
                              const int32_t *col, const int32_t *eid, int32_t fanout,
                              int keep_loops, uint64_t seed, uint64_t offset) {
  return SelectArgs{n_rows, nnz, rowptr, col, eid, (uint32_t)fanout, keep_loops ? 1 : 0,
                    (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)offset,
                    (uint32_t)(offset >> 32)};
}

// word 0 of mgcn_edge_noise's call for head 0 of COO edge e
__device__ __forceinline__ uint32_t edge_key(const SelectArgs &a, uint32_t e) {
  uint32_t c[4] = {e, 0u, a.off0, a.off1};
  philox4x32_10(c, a.key0, a.key1);
  return c[0];
}

// What a row that needs no selection decides for slot k: nothing of a masked
// row, everything where the candidates fit, else (fanout == 0) the loops.
__device__ __forceinline__ bool fill_value(const SelectArgs &a, bool masked, bool all, int64_t r,
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

// Row r = slots [s0, s0 + d) with d <= kLight (d == 0: no row) by the group's
// G lanes, lane lg of it; `tile`: the group's kTileStride u64 of LDS.  Every
// lane of the wave calls it (the wave syncs inside, once more at the end: the
// tile may be rewritten, and LDS that `put` wrote may be read, right after).
// put(j, e, kept) runs once per slot j (COO id e) on the lane that owns it.
template <int G, class Put>
__device__ __forceinline__ void light_row(const SelectArgs &a, int64_t r, int64_t s0, int d,
                                          bool masked, uint64_t *tile, int lg, Put &&put) {
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
    auto rank_put = [&](int j, uint64_t mine, int32_t e) {
      bool kept = true;
      if (mine != kNotCand) {
        uint32_t rank = 0;
        for (int t = 0; t < d; ++t) rank += tile[t] < mine ? 1u : 0u;
        kept = rank < a.fanout;
      }
      put(j, e, kept);
    };
    if (has0) rank_put(lg, mine0, e0);
    for (int j = lg + G; j < d; j += G) rank_put(j, tile[j], a.eid[s0 + j]);
  } else if (d > 0) {
    const bool all = (uint32_t)cand <= a.fanout;
    if (has0) put(lg, e0, masked ? false : all ? true : (a.keep_loops && !cand0));
    for (int j = lg + G; j < d; j += G)
      put(j, a.eid[s0 + j], fill_value(a, masked, all, r, s0 + j));
  }
  wave_sync();
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

// A heavy row's verdict, the same in every thread of the workgroup.
struct HeavyPick {
  bool masked, all;  // read where !select: fill_value's arguments
  bool select;       // a slot is kept iff it is no candidate or its composite <= thr
  bool cached;       // the composites sit in HeavyLds
  uint64_t thr;
};

// slot j of a row under selection: its COO id, its composite, whether it is a candidate
__device__ __forceinline__ bool heavy_load(const SelectArgs &a, const HeavyLds &s, bool cached,
                                           int64_t r, int64_t s0, int64_t j, int32_t &e,
                                           uint64_t &comp) {
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
}

// Row r = slots [s0, s0 + d), d > 0, by the whole workgroup (every thread
// calls it; the branches are uniform).  The LDS it fills is read by
// heavy_kept: a barrier before the next row's call.
__device__ inline HeavyPick heavy_pick(const SelectArgs &a, int64_t r, int64_t s0, int64_t d,
                                       bool masked, HeavyLds &s) {
  const int tid = threadIdx.x;
  HeavyPick p{masked, false, false, false, 0};
  uint32_t cand = (uint32_t)d;
  if (!masked && a.keep_loops) {
    uint32_t c = 0;
    for (int64_t j = tid; j < d; j += kBlock) c += a.col[s0 + j] != (int32_t)r ? 1u : 0u;
    block_scan_incl(c, s.wave, &cand);
  }
  if (masked || cand <= a.fanout || a.fanout == 0) {
    p.all = cand <= a.fanout;
    return p;
  }
  p.select = true;
  p.cached = d <= kCap;
  if (p.cached) {
    for (int64_t j = tid; j < d; j += kBlock) {
      const int32_t e = a.eid[s0 + j];
      const bool is_cand = !a.keep_loops || a.col[s0 + j] != (int32_t)r;
      s.key[j] = is_cand ? edge_key(a, (uint32_t)e) : 0u;
      s.e[j] = (uint32_t)e | (is_cand ? 0u : 0x80000000u);
    }
  }
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
      if (heavy_load(a, s, p.cached, r, s0, j, e, comp) &&
          (pass == 7 || (comp >> (shift + 8)) == prefix))
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
  p.thr = prefix;
  return p;
}

// whether slot j of the row heavy_pick judged is kept; e: its COO id
__device__ __forceinline__ bool heavy_kept(const SelectArgs &a, const HeavyPick &p,
                                           const HeavyLds &s, int64_t r, int64_t s0, int64_t j,
                                           int32_t &e) {
  if (!p.select) {
    e = a.eid[s0 + j];
    return fill_value(a, p.masked, p.all, r, s0 + j);
  }
  uint64_t comp;
  const bool is_cand = heavy_load(a, s, p.cached, r, s0, j, e, comp);
  return !is_cand || comp <= p.thr;
}

}  // namespace sampling
}  // namespace mgcn
