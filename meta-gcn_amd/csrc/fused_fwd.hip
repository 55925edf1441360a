// The two-phase fused forward at F = 128, spmm_xw_fwd_kernel, with its static,
// packed-table and dynamic-claim launches (xw128.h: the design, the shared
// gather primitives and chunk helpers).

#include "xw128.h"

namespace mgcn {
namespace {

#if MGCN_EXPERIMENT
__device__ unsigned long long g_tail[kTailMaxWg][4];  // XTAIL_* (xw128.h), kernel 0
#endif

// ---------------------------------------------------------------------------
// Forward.  LDS: two image sets and two fp32 staging tiles, double-buffered
// so that one barrier per chunk orders everything: chunk c's images are
// written before barrier c and read after it; its output rows are staged
// after barrier c and written out after barrier c + 1.  80 KB: two per CU.
constexpr int kXfBuf = 3 * kXwImg;
constexpr int kXfStageOff = 2 * kXfBuf;
constexpr int kXfLds = kXfStageOff + 2 * kXfStage;
static_assert(2 * kXfLds <= 160 * 1024, "two forward workgroups per CU");

// DYN: the last rounds' chunks are claimed from a global counter instead of
// falling to workgroup c mod grid.  The workgroups of a launch do not run at
// one speed (their exit times spread over ~10 % of the kernel, uncorrelated
// with their slot counts: profiles/balance/tail_before.json), and the kernel
// ends with the slowest; with the tail claimed, the fast ones take more of it.
// Every chunk's rows are computed as before, whoever runs it: Y, Z and the
// mask words keep their bits.  Chunks b + i grid (i < n_my, the rounds before
// dyn_first) are static; chunk index i >= n_my of a workgroup is dyn_first +
// a ticket.
// The next chunk is always known, so that the metadata prefetch two rows
// ahead keeps its target: wave 0 draws a ticket at the end of phase A of
// iteration j, posts it (a global mailbox word of the workgroup; LDS is full)
// at the end of phase B, and every wave reads it after the barrier of
// iteration j + 1 -- chunk index j + 3.
template <int U, bool PK = false, bool DYN = false>
__global__ __launch_bounds__(kXwThreads, 2 * kXwPerCU) void spmm_xw_fwd_kernel(const XwArgs a) {
  static_assert(!(DYN && PK), "the dynamic claim serves the dense forward");
  __shared__ __attribute__((aligned(16))) char lds[kXfLds];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int gl = lane & 31, grp = lane >> 5;
  const int l16 = lane & 15, g4 = lane >> 4;
  const int64_t n_chunks = (a.n_rows + kXwRows - 1) / kXwRows;
  const bool has_b = a.bias != nullptr;
  // gathers through one buffer resource over X: 32-bit offsets, 1 VGPR each
  const auto rx = buf_rsrc(PK ? nullptr : a.X, PK ? 0u : (uint32_t)(a.n_cols * a.ldx * 4));
  const uint32_t ldx_b = (uint32_t)a.ldx * 4u;
  Pk128 pk{};
  u32x2 hh[PK ? U : 1];
  if constexpr (PK) {
    pk.r = buf_rsrc(a.pk, a.pk_bytes);
    pk.rbits = a.pk_rbits;
    pk.head = a.pk_head;
    pk.base = a.pk_base[lane];
  }

  // W fragments of this wave's 16 output columns: B[k][n] = W[k][n], lane
  // (g4, l16) holds k = 32 ks + 8 g4 + j of column n = 16 wave + l16
  const int ncol = 16 * wave + l16;
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

  // staged rows of chunk `c` -> Y (thread: rows tid >> 5 and 16 + (tid >> 5),
  // float4 gl), and the ReLU mask words of each row from four ballots
  auto flush = [&](int64_t c, const float *stage) {
    const int64_t r0 = c * kXwRows;
    const int64_t left = a.n_rows - r0;
    const uint32_t rows_in = (uint32_t)(left >= kXwRows ? kXwRows : left);
    const auto ry = buf_rsrc(a.Y + r0 * a.ldy, rows_in * (uint32_t)a.ldy * 4u);
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int lr = 16 * m + (tid >> 5);
      const float4 v = *reinterpret_cast<const float4 *>(stage + lr * kXwF + 4 * gl);
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), ry,
                                             4 * (int)(lr * a.ldy + 4 * gl), 0, MGCN_NT_OUT);
      if (a.relu_mask != nullptr) {
        // word j of the row: bit gl <=> feature 4 gl + j > 0 (the SpMM's layout)
        const uint32_t m0 = (uint32_t)(__ballot(v.x > 0.0f) >> (32 * grp));
        const uint32_t m1 = (uint32_t)(__ballot(v.y > 0.0f) >> (32 * grp));
        const uint32_t m2 = (uint32_t)(__ballot(v.z > 0.0f) >> (32 * grp));
        const uint32_t m3 = (uint32_t)(__ballot(v.w > 0.0f) >> (32 * grp));
        if (gl == 0 && (uint32_t)lr < rows_in)
          *reinterpret_cast<uint4 *>(a.relu_mask + (r0 + lr) * 4) = make_uint4(m0, m1, m2, m3);
      }
    }
  };

  // static chunks of this workgroup: all of its round robin, or (DYN) the
  // rounds before dyn_first (a multiple of the grid, >= 3 rounds)
  const int64_t n_my = my_chunks(DYN ? a.dyn_first : n_chunks);
  const RowSeq seq{(int64_t)blockIdx.x * kXwRows + 2 * wave + grp, (int64_t)gridDim.x * kXwRows,
                   a.n_rows};
  XTAIL_ENTRY(0);
  // DYN: chunk index it + 1 of this workgroup (-1: none; 32-bit: scalar
  // registers are short), uniform
  auto stat_chunk = [&](int i) -> int {
    return i < (int)n_my ? (int)(blockIdx.x + i * gridDim.x) : -1;
  };
  int c1 = stat_chunk(1);
  // row 16 p + 2 wave + grp of chunk c
  auto dyn_row = [&](int c, int p) { return (int64_t)c * kXwRows + 16 * p + 2 * wave + grp; };
  RowMeta cur, nxt;
  meta_rowptr(a.rowptr, seq.row(0), seq.row(0) < a.n_rows, cur);
  if constexpr (PK) {
    meta_first_pk(pk, a.col, a.w, gl, cur);
    pk128_headers<U>(pk, cur.mc, grp, 0, cur.deg < 32 ? cur.deg : 32, 8u * (uint32_t)(gl >> 3), hh);
  } else {
    meta_first(a.col, a.w, gl, cur);
  }
  meta_rowptr(a.rowptr, seq.row(1), seq.row(1) < a.n_rows, nxt);
  int it = 0;
  int prev = -1;  // DYN: the chunk whose rows are staged
  for (int64_t chunk = blockIdx.x; DYN ? chunk >= 0 : chunk < n_chunks; ++it) {
    char *buf = lds + (it & 1) * kXfBuf;
    float *stage = reinterpret_cast<float *>(lds + kXfStageOff + (it & 1) * kXfStage);

    // ---- Phase A: aggregate the chunk's rows into the bf16 images --------
#pragma unroll 1
    for (int p = 0; p < 2; ++p) {
      const int lr = 16 * p + 2 * wave + grp;
      const int64_t k = 2 * it + p;
      if constexpr (PK)
        meta_first_pk(pk, a.col, a.w, gl, nxt);
      else
        meta_first(a.col, a.w, gl, nxt);
      RowMeta nn;
      const int64_t r2 = DYN ? dyn_row(c1, p) : seq.row(k + 2);
      meta_rowptr(a.rowptr, r2, r2 < a.n_rows && (DYN ? c1 >= 0 : k + 2 < 2 * n_my), nn);
      float acc[4];
      if constexpr (PK)
        gather_row_meta_pk<U>(pk, a.col, a.w, cur, nxt, gl, grp, acc, hh);
      else
        gather_row_meta<U>(rx, ldx_b, a.col, a.w, cur, gl, grp, acc);
      if (a.Z != nullptr) {
        // the aggregate the backward's dW = Z^T dY reads (whole 512-B rows;
        // rows past the end fall outside the chunk's buffer range)
        const int64_t r0 = chunk * kXwRows;
        const int64_t left = a.n_rows - r0;
        const uint32_t rows_in = (uint32_t)(left >= kXwRows ? kXwRows : left);
        const auto rz = buf_rsrc(a.Z + r0 * a.ldz, rows_in * (uint32_t)a.ldz * 4u);
        __builtin_amdgcn_raw_buffer_store_b128(
            __builtin_bit_cast(u32x4, make_float4(acc[0], acc[1], acc[2], acc[3])), rz,
            4 * (int)(lr * a.ldz + 4 * gl), 0, MGCN_NT_AUX);
      }
      if (a.mean) {
        const float c = (float)(cur.deg > 1 ? cur.deg : 1);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = __fdiv_rn(acc[j], c);
      }
      store_row_terms(buf, lr, gl, acc);
      cur = nxt;
      nxt = nn;
    }
    // DYN: a ticket for chunk index it + 3 (past the static rounds), drawn
    // here so that its round trip runs under the barrier and phase B
    uint32_t ticket = 0;
    const bool draw = DYN && wave == 0 && it + 3 >= (int)n_my;
    if constexpr (DYN)
      if (draw && lane == 0)
        ticket = __hip_atomic_fetch_add(a.claim, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    // the previous chunk's output rows (staged before this barrier) go out
    if (it > 0)
      flush(DYN ? prev : chunk - gridDim.x,
            reinterpret_cast<const float *>(lds + kXfStageOff + ((it + 1) & 1) * kXfStage));
    // DYN: the ticket posted in iteration it - 1 (before this barrier)
    int posted = 0;
    const bool take = DYN && it + 2 >= (int)n_my && it > 0;
    if constexpr (DYN)
      if (take)
        posted = __hip_atomic_load(a.mail + 2 * blockIdx.x + ((it + 1) & 1), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_WORKGROUP);

    // ---- Phase B: Y = Z W (+ b), ReLU -> staging tile ----------------------
    f32x4_t acc2[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc2[t][r] = 0.0f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) mfma_rows(buf, wb[ks], ks, l16, g4, acc2);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = acc2[t][r];
        if (has_b) v = __fadd_rn(v, bcol);
        if (a.relu) v = (v < 0.0f) ? 0.0f : v;
        stage[(16 * t + 4 * g4 + r) * kXwF + ncol] = v;
      }
    if constexpr (DYN) {
      if (draw && lane == 0)
        __hip_atomic_store(a.mail + 2 * blockIdx.x + (it & 1), (int)ticket, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_WORKGROUP);
      // chunk index it + 2: static, or dyn_first + the ticket while chunks last
      int c2 = stat_chunk(it + 2);
      if (take) {
        const uint32_t c = (uint32_t)a.dyn_first + (uint32_t)__builtin_amdgcn_readfirstlane(posted);
        c2 = c < (uint32_t)n_chunks ? (int)c : -1;
      }
      prev = (int)chunk;
      chunk = c1;
      c1 = c2;
    } else {
      chunk += gridDim.x;
    }
  }
  if (it > 0) {
    __syncthreads();
    flush(DYN ? prev : blockIdx.x + (int64_t)(it - 1) * gridDim.x,
          reinterpret_cast<const float *>(lds + kXfStageOff + ((it + 1) & 1) * kXfStage));
  }
  XTAIL_EXIT(0, it);
}

template <int U, bool PK = false>
int launch_xw(const XwArgs &a, hipStream_t s) {
  const int64_t n_chunks = (a.n_rows + kXwRows - 1) / kXwRows;
  int64_t grid = xw_grid();
  if (grid > n_chunks) grid = n_chunks;
  hipLaunchKernelGGL((spmm_xw_fwd_kernel<U, PK>), dim3((unsigned)grid), dim3(kXwThreads), 0, s, a);
  return check_launch("spmm_xw_fwd_kernel");
}

constexpr size_t kXwDynMailOff = 256;  // workspace: the counter, then [grid][2] mailbox words

}  // namespace

int launch_xw_fwd(const void *xw, bool packed, hipStream_t s) {
  const XwArgs &a = *static_cast<const XwArgs *>(xw);
  if (packed) {
    // (the product build instantiates U = 3 only)
    constexpr bool X = MGCN_EXPERIMENT;
    if (X && g_opt.xw_pk_unroll == 4) return launch_xw<X ? 4 : 3, true>(a, s);
    if (X && g_opt.xw_pk_unroll == 5) return launch_xw<X ? 5 : 3, true>(a, s);
    if (X && g_opt.xw_pk_unroll == 6) return launch_xw<X ? 6 : 3, true>(a, s);
    return launch_xw<3, true>(a, s);
  }
  return g_opt.spmm_xw_unroll == 4 ? launch_xw<4>(a, s)
       : g_opt.spmm_xw_unroll == 5 ? launch_xw<5>(a, s)
       : g_opt.spmm_xw_unroll == 6 ? launch_xw<6>(a, s)
                                   : launch_xw<8>(a, s);
}

size_t xw_dyn_workspace_bytes() { return kXwDynMailOff + align_up((size_t)xw_grid() * 8, 256); }

bool launch_xw_dyn(const void *xw, void *workspace, size_t workspace_bytes, hipStream_t s, int *rc) {
  XwArgs a = *static_cast<const XwArgs *>(xw);
  const int64_t n_chunks = (a.n_rows + kXwRows - 1) / kXwRows;
  const int64_t grid = xw_grid();
  const int64_t rounds = n_chunks / grid;
  if (g_opt.xw_dyn_rounds <= 0 || g_opt.spmm_xw_unroll != 5 || workspace == nullptr ||
      reinterpret_cast<uintptr_t>(workspace) % 4 != 0 ||
      workspace_bytes < xw_dyn_workspace_bytes() || rounds < g_opt.xw_dyn_rounds + 8 ||
      n_chunks >= (int64_t(1) << 30))
    return false;
  a.dyn_first = (int32_t)((rounds - g_opt.xw_dyn_rounds) * grid);
  a.claim = static_cast<uint32_t *>(workspace);
  a.mail = reinterpret_cast<int32_t *>(static_cast<char *>(workspace) + kXwDynMailOff);
  if (hipMemsetAsync(a.claim, 0, sizeof(uint32_t), s) != hipSuccess) {
    *rc = check_launch("hipMemsetAsync");
    return true;
  }
  hipLaunchKernelGGL((spmm_xw_fwd_kernel<5, false, true>), dim3((unsigned)grid), dim3(kXwThreads),
                     0, s, a);
  *rc = check_launch("spmm_xw_fwd_kernel");
  return true;
}

#if MGCN_EXPERIMENT
int xw_fwd_tail_take(unsigned long long *host) { return tail_take(HIP_SYMBOL(g_tail), host); }
#endif

}  // namespace mgcn
