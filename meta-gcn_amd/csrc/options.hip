// mgcn_set_option: one table of every knob (the fields and their defaults:
// struct Options, mgcn_internal.h; what each does: include/mgcn.h).

#include <climits>
#include <cstring>
#include <string>

#include "mgcn_internal.h"

namespace mgcn {

Options g_opt;

namespace {

// accepted values: lo .. hi (n == 0), or one of of[0 .. n)
struct Rule {
  int lo, hi, n;
  int of[4];
};
constexpr Rule range(int lo, int hi) { return Rule{lo, hi, 0, {}}; }
template <class... T>
constexpr Rule one_of(T... v) {
  return Rule{0, 0, (int)sizeof...(v), {v...}};
}
constexpr Rule kFlag = range(0, 1), kAny = range(INT_MIN, INT_MAX);

struct Row {
  const char *name;
  int Options::*field;
  Rule rule;
  bool experiment_only;  // the product library rejects the name (mgcn_internal.h: MGCN_EXPERIMENT)
  int Options::*mark;    // set to 1 beside the value ("the option was given"), or none
};

constexpr Row kRows[] = {
    {"spmm_vec", &Options::spmm_vec, one_of(0, 1, 2, 4), false, nullptr},
    {"spmm_unroll", &Options::spmm_unroll, one_of(4, 6, 8, 16), false, &Options::spmm_unroll_set},
    {"heavy_side_stream", &Options::heavy_side_stream, kFlag, false, nullptr},
    {"heavy_side_fence", &Options::heavy_side_fence, kFlag, false, nullptr},
    {"heavy_lds_kb", &Options::heavy_lds_kb, range(16, 160), false, nullptr},
    {"heavy_block", &Options::heavy_block, one_of(256, 512, 1024), false, nullptr},
    {"heavy_mid_lds_kb", &Options::heavy_mid_lds_kb, range(16, 160), false, nullptr},
    {"heavy_mid_q1", &Options::heavy_mid_q1, kFlag, false, nullptr},
    {"heavy_giant_thr", &Options::heavy_giant_thr, range(0, INT_MAX), false, nullptr},
    {"residual_blocks", &Options::residual_blocks, range(64, 65536), false, nullptr},
    {"residual_fused_mask", &Options::residual_fused_mask, kFlag, false, nullptr},
    {"gemm_tn_variant", &Options::gemm_tn_variant, range(0, 2), false, nullptr},
    {"gemm_tn_staged", &Options::gemm_tn_staged, kFlag, false, nullptr},
    {"gemm_precision", &Options::gemm_precision, kFlag, false, nullptr},  // 0 f32, 1 bf16x6
    // 5 / 6: the forward only (the two-phase adjoints: 8, else 4)
    {"spmm_xw_unroll", &Options::spmm_xw_unroll, one_of(4, 5, 6, 8), false, nullptr},
    {"xw_dyn_rounds", &Options::xw_dyn_rounds, range(0, 64), false, nullptr},  // 0: no dynamic claim
    {"xw_fwd_ws", &Options::xw_fwd_ws, kFlag, false, nullptr},
    {"xw_ws_full", &Options::xw_ws_full, kFlag, false, nullptr},
    {"xw_ws_max", &Options::xw_ws_max, kFlag, false, nullptr},
    {"xw_ws_full_unroll", &Options::xw_ws_full_unroll, one_of(4, 5, 6), false, nullptr},
    {"xw_ws_roll", &Options::xw_ws_roll, one_of(0, 2), false, nullptr},
    {"wide_ws", &Options::wide_ws, range(0, 3), false, nullptr},
    {"wide_pair", &Options::wide_pair, range(0, 3), false, nullptr},
    {"wide_mfma", &Options::wide_mfma, one_of(4, 8), false, nullptr},
    // experiment builds: the hand-off bound (abort-path tests), the timing
    // experiments (results WRONG when set) and the packed forms' unroll sweep
    {"ws_spin_limit", &Options::ws_spin_limit, range(1, INT_MAX), true, nullptr},
    {"wide_dbg", &Options::wide_dbg, kAny, true, nullptr},
    {"xw_ws_dbg", &Options::xw_ws_dbg, kAny, true, nullptr},
    {"xw_pk_unroll", &Options::xw_pk_unroll, one_of(3, 4, 5, 6), true, nullptr},
    {"xw_pk_bwd_unroll", &Options::xw_pk_bwd_unroll, one_of(2, 3, 4), true, nullptr},
};

bool accepts(const Rule &r, int value) {
  if (r.n == 0) return value >= r.lo && value <= r.hi;
  for (int i = 0; i < r.n; ++i)
    if (r.of[i] == value) return true;
  return false;
}

// "<name> must be ..." from the rule
void set_rule_error(const Row &row, int value) {
  const Rule &r = row.rule;
  if (r.n == 0) {
    set_error("%s must be in %d .. %d (got %d)", row.name, r.lo, r.hi, value);
    return;
  }
  std::string list;
  for (int i = 0; i < r.n; ++i) list += (i ? ", " : "") + std::to_string(r.of[i]);
  set_error("%s must be one of %s (got %d)", row.name, list.c_str(), value);
}

}  // namespace
}  // namespace mgcn

using namespace mgcn;

extern "C" int mgcn_set_option(const char *name, int value) {
  clear_error();
  MGCN_REQUIRE(name != nullptr, "mgcn_set_option: null name");
  for (const Row &row : kRows) {
    if (std::strcmp(row.name, name) != 0) continue;
    MGCN_REQUIRE(MGCN_EXPERIMENT || !row.experiment_only,
                 "%s: experiment builds only (make exp -> libmgcn_exp.so)", name);
    if (!accepts(row.rule, value)) {
      set_rule_error(row, value);
      return MGCN_EINVAL;
    }
    g_opt.*row.field = value;
    if (row.mark != nullptr) g_opt.*row.mark = 1;
    return MGCN_OK;
  }
  set_error("mgcn_set_option: unknown option '%s'", name);
  return MGCN_EINVAL;
}
