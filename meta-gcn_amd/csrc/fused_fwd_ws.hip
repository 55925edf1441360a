// The warp-specialised fused forward at F = 128, spmm_xw_fwd_ws_kernel, with
// its launch (xw128.h: the design, the shared gather primitives and chunk
// helpers; ws_handoff.h: the LDS counter hand-off).

#include "ws_handoff.h"
#include "xw128.h"

namespace mgcn {
namespace {

// ===================== warp-specialised forward ================================
//
// spmm_xw_fwd_kernel re-cut by role like DWS: one 1024-thread workgroup per
// CU.  8 GATHER waves aggregate the chunk's rows with the rolling gather (a
// wave's quad of a chunk: rows 4 wave + grp and 4 wave + 2 + grp per lane
// group; gather_row_meta's edge order, products and sums rounded separately:
// the SpMM bit for bit), carry their slots from a quad's last round into the
// quad of the workgroup's next chunk, store Z straight from registers, apply
// mean's division and write the three bf16 term images into a ring of
// MGCN_XF_RING chunk buffers.  They hold no W and never stop for a barrier or
// an MFMA phase.  8 MFMA waves hold the W fragments of their 16 output columns
// (wb[4][3], as the two-phase kernel), take the chunks in ring order, run the
// same six products in the same order, add bias / ReLU, stage the tile and
// write whole 512-B rows and the mask words by the two-phase kernel's ballots:
// Y, Z and the mask keep their bits.
//
// Chunk index i of a workgroup: chunk b + i grid for i < n_stat, then (the
// claimed tail, as the two-phase DYN kernel's) dyn_first + a ticket.  Gather
// wave 0 draws the ticket of index k + kXfsLead at the start of its quad k and
// posts it in LDS (tslot / tpub) at the quad's end; a gather wave needs index
// k + 2 at the start of its quad k (the rowptr prefetch), so it may run two
// quads ahead of wave 0 before it waits.  The chunk id of a ring slot travels
// with it (cid); id -1, posted by gather wave 0 alone, ends the MFMA waves.
// Hand-offs (monotonic LDS counters; bounded spins, abort word, device error
// word as DWS):
//   filled[b]  += 4 per gather wave and quad; MFMA waves wait 32 (gen + 1)
//   mdone[b]   += 1 per MFMA wave; the 8th of a generation bumps freed[b]
//   freed[b]   gather waves wait >= gen before they overwrite slot b
//   staged     += 1 per MFMA wave and chunk; chunk i - 1 is flushed once it
//              stands at 8 i -- which also says every wave has read chunk
//              i - 2's tile (it did so before it staged i - 1), the tile chunk
//              i is staged into
#ifndef MGCN_XF_RING
#define MGCN_XF_RING 4  // ring depth (profiles/fwd_ws/ring_sweep.json)
#endif
constexpr int kXfsRing = MGCN_XF_RING;
constexpr int kXfsLead = 4;  // ticket drawn this many chunk indices ahead
constexpr int kXfsStageOff = kXfsRing * kBsImgSet;
constexpr int kXfsCtrOff = kXfsStageOff + 2 * kXfStage;
constexpr int kXfsLds = kXfsCtrOff + 256;
static_assert(kXfsRing >= 2 && kXfsRing <= 8, "ring counters: 8 words each");
static_assert(kXfsLds <= 160 * 1024, "one forward workgroup per CU");

struct XfsArgs {
  XwArgs a;       // dyn_first < 0: every chunk static (claim unused)
  uint32_t spin;  // hand-off spin bound ("ws_spin_limit")
  unsigned *err;  // device error word: kDevErrFwdWs when a hand-off gave up
};

template <int U>
__global__ __launch_bounds__(kBsThreads) void spmm_xw_fwd_ws_kernel(const XfsArgs A) {
  const XwArgs &a = A.a;
  __shared__ __attribute__((aligned(16))) char lds[kXfsLds];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int gl = lane & 31, grp = lane >> 5;
  int *ctr = reinterpret_cast<int *>(lds + kXfsCtrOff);
  int *filled = ctr, *mdone = ctr + 8, *freed = ctr + 16, *cid = ctr + 24, *tslot = ctr + 32;
  int *staged = ctr + 48, *tpub = ctr + 49, *abort_word = ctr + 50;
  if (tid < 64) ctr[tid] = 0;
  __syncthreads();

  const int64_t n_chunks = (a.n_rows + kXwRows - 1) / kXwRows;
  const bool dyn = a.dyn_first >= 0;
  auto rows_in = [&](int c) -> uint32_t {
    const int64_t r = a.n_rows - (int64_t)c * kXwRows;
    return (uint32_t)(r >= kXwRows ? kXwRows : r);
  };

  if (wave < kBsNG) {
    // ------------------------------- gather waves ---------------------------
    const int n_stat = (int)my_chunks(dyn ? (int64_t)a.dyn_first : n_chunks);
    auto stat_chunk = [&](int i) -> int {
      return i < n_stat ? (int)(blockIdx.x + i * gridDim.x) : -1;
    };
    auto row_of = [&](int c, int second) -> int64_t {
      return (int64_t)c * kXwRows + 4 * wave + 2 * second + grp;
    };
    const auto rx = buf_rsrc(a.X, (uint32_t)(a.n_cols * a.ldx * 4));
    const uint32_t ldx_b = (uint32_t)a.ldx * 4u;
    // chunk indices k, k + 1 (static: the host leaves >= kXfsLead static rounds
    // before a claimed tail)
    int c0 = stat_chunk(0), c1 = stat_chunk(1);
    RowMeta cur[2] = {}, nxt[2] = {};
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      meta_rowptr(a.rowptr, row_of(c0, j), c0 >= 0 && row_of(c0, j) < a.n_rows, cur[j]);
      meta_first(a.col, a.w, gl, cur[j]);
      meta_rowptr(a.rowptr, row_of(c1, j), c1 >= 0 && row_of(c1, j) < a.n_rows, nxt[j]);
    }
    RollWin<U> win;
    roll_first<U>(rx, ldx_b, cur[0], cur[1], gl, grp, win);
    int k = 0, b = 0, gen = 0;
    while (c0 >= 0) {
      // the ticket of chunk index k + kXfsLead: its round trip under the gathers
      uint32_t ticket = 0;
      const bool draw = dyn && wave == 0 && k + kXfsLead >= n_stat;
      if (draw && lane == 0)
        ticket = __hip_atomic_fetch_add(a.claim, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      int c2 = stat_chunk(k + 2);
      if (dyn && k + 2 >= n_stat) {
        if (!lds_wait_ge(tpub, k + 3, abort_word, A.spin)) break;
        c2 = lds_load(tslot + ((k + 2) & 15));
      }
      RowMeta nn[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        meta_first(a.col, a.w, gl, nxt[j]);
        const int64_t r2 = row_of(c2, j);
        meta_rowptr_raw(a.rowptr, r2, c2 >= 0 && r2 < a.n_rows, nn[j]);
      }
      const int64_t r0 = (int64_t)c0 * kXwRows;
      const int lr0 = 4 * wave + grp;
      float rsc[2] = {1.0f, 1.0f};
      float acc[2][4];
      gather_row2_roll<U>(rx, ldx_b, a.rowptr, a.col, a.w, r0 + lr0, r0 + lr0 + 2, cur[0], cur[1],
                          nxt[0], nxt[1], c1 >= 0, gl, grp, acc[0], acc[1], win, nullptr, a.n_rows,
                          rsc);
      if (a.Z != nullptr) {
        // the aggregate the backward's dW = Z^T dY reads (rows past the end
        // fall outside the chunk's buffer range)
        const auto rz = buf_rsrc(a.Z + r0 * a.ldz, rows_in(c0) * (uint32_t)a.ldz * 4u);
#pragma unroll
        for (int j = 0; j < 2; ++j)
          __builtin_amdgcn_raw_buffer_store_b128(
              __builtin_bit_cast(u32x4, make_float4(acc[j][0], acc[j][1], acc[j][2], acc[j][3])),
              rz, 4 * (int)((lr0 + 2 * j) * a.ldz + 4 * gl), 0, MGCN_NT_AUX);
      }
      if (a.mean) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const float c = (float)(cur[j].deg > 1 ? cur[j].deg : 1);
#pragma unroll
          for (int t = 0; t < 4; ++t) acc[j][t] = __fdiv_rn(acc[j][t], c);
        }
      }
      if (!lds_wait_ge(freed + b, gen, abort_word, A.spin)) break;
      char *buf = lds + b * kBsImgSet;
#pragma unroll
      for (int j = 0; j < 2; ++j) store_row_terms(buf, lr0 + 2 * j, gl, acc[j]);
      if (wave == 0 && lane == 0)
        __hip_atomic_store(cid + b, c0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      lds_signal(filled + b, 4, lane);
      if (draw) {  // post chunk index k + kXfsLead, then say so
        const uint32_t c = (uint32_t)a.dyn_first + (uint32_t)__builtin_amdgcn_readfirstlane(ticket);
        if (lane == 0) {
          __hip_atomic_store(tslot + ((k + kXfsLead) & 15), c < (uint32_t)n_chunks ? (int)c : -1,
                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          __hip_atomic_store(tpub, k + kXfsLead + 1, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        cur[j] = nxt[j];
        nxt[j] = nn[j];
        meta_deg(nxt[j]);
      }
      c0 = c1;
      c1 = c2;
      ++k;
      if (++b == kXfsRing) {
        b = 0;
        ++gen;
      }
    }
    // no more chunks: gather wave 0 says so in the next ring slot
    if (wave == 0 && lds_wait_ge(freed + b, gen, abort_word, A.spin)) {
      if (lane == 0)
        __hip_atomic_store(cid + b, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      lds_signal(filled + b, kXwRows, lane);
    }
  } else {
    // -------------------------------- MFMA waves ----------------------------
    const int m = wave - kBsNG;  // output columns 16 m .. 16 m + 15
    const int mt = tid - 64 * kBsNG;
    const int l16 = lane & 15, g4 = lane >> 4;
    const bool has_b = a.bias != nullptr;
    // W fragments (spmm_xw_fwd_kernel's): lane (g4, l16) holds k = 32 ks +
    // 8 g4 + j of column n = 16 m + l16
    const int ncol = 16 * m + l16;
    bf16x8 wb[4][3];
    {
      const float *wp = a.W + (int64_t)(8 * g4) * a.ldw + ncol;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = wp[(int64_t)(32 * ks + j) * a.ldw];
        split3_bf16(v, wb[ks][0], wb[ks][1], wb[ks][2]);
      }
    }
    const float bcol = has_b ? a.bias[ncol] : 0.0f;
    // staged rows of chunk c -> Y (thread: rows mt >> 5 and 16 + (mt >> 5),
    // float4 gl) and the rows' ReLU mask words (spmm_xw_fwd_kernel's flush)
    auto flush = [&](int c, const float *stage) {
      const int64_t r0 = (int64_t)c * kXwRows;
      const uint32_t rin = rows_in(c);
      const auto ry = buf_rsrc(a.Y + r0 * a.ldy, rin * (uint32_t)a.ldy * 4u);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int lr = 16 * h + (mt >> 5);
        const float4 v = *reinterpret_cast<const float4 *>(stage + lr * kXwF + 4 * gl);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), ry,
                                               4 * (int)(lr * a.ldy + 4 * gl), 0, MGCN_NT_OUT);
        if (a.relu_mask != nullptr) {
          const uint32_t m0 = (uint32_t)(__ballot(v.x > 0.0f) >> (32 * grp));
          const uint32_t m1 = (uint32_t)(__ballot(v.y > 0.0f) >> (32 * grp));
          const uint32_t m2 = (uint32_t)(__ballot(v.z > 0.0f) >> (32 * grp));
          const uint32_t m3 = (uint32_t)(__ballot(v.w > 0.0f) >> (32 * grp));
          if (gl == 0 && (uint32_t)lr < rin)
            *reinterpret_cast<uint4 *>(a.relu_mask + (r0 + lr) * 4) = make_uint4(m0, m1, m2, m3);
        }
      }
    };
    int b = 0, gen = 0, prev = -1;
    for (int i = 0;; ++i) {
      // chunk i - 1's rows go out once all eight waves have staged them
      if (i > 0) {
        if (!lds_wait_ge(staged, kBsNM * i, abort_word, A.spin)) break;
        flush(prev, reinterpret_cast<const float *>(lds + kXfsStageOff + ((i - 1) & 1) * kXfStage));
      }
      if (!lds_wait_ge(filled + b, kXwRows * (gen + 1), abort_word, A.spin)) break;
      const int c = lds_load(cid + b);
      if (c < 0) break;
      const char *buf = lds + b * kBsImgSet;
      f32x4_t acc2[2];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc2[t][r] = 0.0f;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) mfma_rows(buf, wb[ks], ks, l16, g4, acc2);
      const int old = lds_signal(mdone + b, 1, lane);
      if (old == kBsNM * gen + kBsNM - 1) lds_signal(freed + b, 1, lane);
      float *stage = reinterpret_cast<float *>(lds + kXfsStageOff + (i & 1) * kXfStage);
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = acc2[t][r];
          if (has_b) v = __fadd_rn(v, bcol);
          if (a.relu) v = (v < 0.0f) ? 0.0f : v;
          stage[(16 * t + 4 * g4 + r) * kXwF + ncol] = v;
        }
      lds_signal(staged, 1, lane);
      prev = c;
      if (++b == kXfsRing) {
        b = 0;
        ++gen;
      }
    }
  }
  __syncthreads();
  // a hand-off gave up: this launch's Y / Z are incomplete -- say so
  if (wave == 0 && lds_load(abort_word) != 0) report_device_error(A.err, kDevErrFwdWs);
}

}  // namespace

// The last 2 xw_dyn_rounds rounds are claimed (this
// grid is half the two-phase kernel's: the same chunks), fewer where that
// leaves less than 8 static rounds before them (launch_xw_dyn's margin; the
// kernel needs kXfsLead); a view of 8 rounds or less runs every chunk static.
bool launch_xw_ws(const void *xw, void *workspace, size_t workspace_bytes, hipStream_t s, int *rc) {
  const XwArgs &a0 = *static_cast<const XwArgs *>(xw);
  const int64_t n_chunks = (a0.n_rows + kXwRows - 1) / kXwRows;
  if (g_opt.xw_fwd_ws == 0 || g_opt.spmm_xw_unroll != 5 || workspace == nullptr ||
      reinterpret_cast<uintptr_t>(workspace) % 4 != 0 ||
      workspace_bytes < xw_dyn_workspace_bytes() || n_chunks >= (int64_t(1) << 30))
    return false;
  XfsArgs A{};
  A.a = a0;
  A.spin = (uint32_t)g_opt.ws_spin_limit;
  A.err = device_error_word();
  if (A.err == nullptr) {
    *rc = MGCN_EHIP;
    return true;
  }
  const int64_t grid = device_cus();  // one workgroup per CU
  const int64_t rounds = n_chunks / grid;
  int64_t tail = 2 * (int64_t)g_opt.xw_dyn_rounds;
  if (tail > rounds - 8) tail = rounds - 8;
  static_assert(kXfsLead <= 8, "static rounds before the claimed tail");
  A.a.dyn_first = -1;
  if (tail > 0) {
    A.a.dyn_first = (int32_t)((rounds - tail) * grid);
    A.a.claim = static_cast<uint32_t *>(workspace);
    if (hipMemsetAsync(A.a.claim, 0, sizeof(uint32_t), s) != hipSuccess) {
      *rc = check_launch("hipMemsetAsync");
      return true;
    }
  }
  hipLaunchKernelGGL((spmm_xw_fwd_ws_kernel<5>), dim3((unsigned)grid), dim3(kBsThreads), 0, s, A);
  *rc = check_launch("spmm_xw_fwd_ws_kernel");
  return true;
}

}  // namespace mgcn
