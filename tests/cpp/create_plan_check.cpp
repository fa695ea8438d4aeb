// Host-only check of the resolver behind povar_create (povar_amd/csrc/create_plan.hpp): a table of (flags, e0_mode, robust_norm,
// n_cams, n_obs, CU count, environment) against EVERY field of the CreatePlan, or against the refusal's code and text.  The
// expected values are written down from povar_create's statement order before the resolver existed and from INTEGRATION.md
// section 6, never taken from the resolver: a row states what differs from the defaults of its problem.  No HIP runtime call.
// tests/test_gpu_create_plan.py holds the same expectations to povar_layout_info on a device.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "../../povar_amd/csrc/create_plan.hpp"

using namespace povar;

using Env = std::vector<std::pair<const char*, const char*>>;
static const Env* g_env = nullptr;
static const char* lookup(const char* name) {
  for (const auto& kv : *g_env)
    if (!std::strcmp(kv.first, name)) return kv.second;
  return nullptr;
}

static CkShape shape(int slot_bytes, int li_mul, int max_slots, bool need_uv, int acc_bytes, bool cold_q, int wide_slots) {
  CkShape s;
  s.slot_bytes = slot_bytes; s.li_mul = li_mul; s.max_slots = max_slots; s.need_uv = need_uv; s.acc_bytes = acc_bytes; s.cold_q = cold_q;
  s.wide_slots = wide_slots;
  return s;
}
static const CkShape STEP1_COLD_Q = shape(48, 3, INT_MAX, true, 104, true, 0), STEP1_RECORDS = shape(48, 3, INT_MAX, true, 104, false, 0),
                     STEP1_DET = shape(50, 3, INT_MAX, true, 106, false, 0), STEP2 = shape(64, 1, 1536, false, 104, false, 2048),
                     STEP2_DET = shape(66, 1, 1536, false, 106, false, 0);

// The problem every row starts from: 100 cameras, 70 000 observations, a device of 256 CUs, POVAR_E0_IMPLICIT_LDSACC, no robust
// norm, no flag, an empty environment -- and what povar_create makes of it.
static CreatePlan base_plan() {
  CreatePlan p;
  p.timing = false;
  p.device_cus = 256; p.cu_first = 0; p.cu_last = -1; p.cu_limit = 0;
  p.deterministic = false; p.det_ck = false; p.e0_mode = POVAR_E0_IMPLICIT_LDSACC;
  p.fp32_terms = false; p.use_graph = true; p.no_err_memo = false; p.graph_with_comm = false; p.fuse_binv = true;
  p.use_lpl = true; p.lpl_forced = false; p.k1_qr = true; p.use_lpl_prepare = true;
  p.ck_variant = 0; p.ckh_variant = 0; p.ck_auto = true; p.want_ck = true;
  p.cut.nw = 16; p.cut.ng = 1; p.cut.hmax = 16; p.cut.place = true; p.cut.pack = true; p.cut.shape1 = STEP1_COLD_Q; p.cut.shape2 = STEP2;
  p.ckh_early = false;
  p.place_mode = 1; p.place_forced = false; p.q_rows = -1;
  p.res_mode = -1; p.res_spin_limit = 262144u; p.res_max_obs = 400000; p.res_obs_per_wg = 256; p.res_wgs = 256;  // ceil(70000 / 256) = 274 > 256 CUs
  p.e0_wgs = 256; p.n_hot_acc = 100; p.ck_max_cams = 65535; p.long_separate = false;
  return p;
}

struct Row {
  const char* name;
  uint32_t flags;
  Env env;
  std::function<void(CreatePlan&)> expect;  // what differs from base_plan()
  int rc = 0;
  const char* message = "";
  int e0_mode = POVAR_E0_IMPLICIT_LDSACC, robust = POVAR_NORM_NONE, n_cams = 100;
  int64_t n_obs = 70000;
  int cus = 256;
};

static int n_bad = 0;
#define FIELD(f)                                                                                                      \
  if (!(got.f == want.f)) { std::printf("FAILED %s: %s = %lld, expected %lld\n", name, #f, (long long)got.f, (long long)want.f); ++n_bad; }
static void compare_shape(const char* name, const char* which, const CkShape& got, const CkShape& want) {
  if (got.slot_bytes != want.slot_bytes || got.li_mul != want.li_mul || got.max_slots != want.max_slots || got.need_uv != want.need_uv ||
      got.acc_bytes != want.acc_bytes || got.cold_q != want.cold_q || got.wide_slots != want.wide_slots) {
    std::printf("FAILED %s: %s = {%d, %d, %d, %d, %d, %d, %d}, expected {%d, %d, %d, %d, %d, %d, %d}\n", name, which, got.slot_bytes, got.li_mul,
                got.max_slots, got.need_uv, got.acc_bytes, got.cold_q, got.wide_slots, want.slot_bytes, want.li_mul, want.max_slots, want.need_uv,
                want.acc_bytes, want.cold_q, want.wide_slots);
    ++n_bad;
  }
}
static void compare(const char* name, const CreatePlan& got, const CreatePlan& want) {
  FIELD(timing) FIELD(device_cus) FIELD(cu_first) FIELD(cu_last) FIELD(cu_limit) FIELD(deterministic) FIELD(det_ck) FIELD(e0_mode)
  FIELD(fp32_terms) FIELD(use_graph) FIELD(no_err_memo) FIELD(graph_with_comm) FIELD(fuse_binv) FIELD(use_lpl) FIELD(lpl_forced) FIELD(k1_qr)
  FIELD(use_lpl_prepare) FIELD(ck_variant) FIELD(ckh_variant) FIELD(ck_auto) FIELD(want_ck) FIELD(cut.nw) FIELD(cut.ng) FIELD(cut.hmax)
  FIELD(cut.place) FIELD(cut.pack) FIELD(ckh_early) FIELD(place_mode) FIELD(place_forced) FIELD(q_rows) FIELD(res_mode) FIELD(res_spin_limit)
  FIELD(res_max_obs) FIELD(res_obs_per_wg) FIELD(res_wgs) FIELD(e0_wgs) FIELD(n_hot_acc) FIELD(ck_max_cams) FIELD(long_separate)
  compare_shape(name, "cut.shape1", got.cut.shape1, want.cut.shape1);
  compare_shape(name, "cut.shape2", got.cut.shape2, want.cut.shape2);
}
// (a field added to CreatePlan must be added to compare(): the struct's size is pinned so that it cannot be forgotten)
static_assert(sizeof(CreatePlan) == 184, "CreatePlan changed: compare() in this file must list every field");

// the deterministic context whatever else is asked: gather mode, nothing timed, e0_lpl's variant numbers, no resident series, no placement
static void det(CreatePlan& p) {
  p.deterministic = true; p.det_ck = true; p.e0_mode = POVAR_E0_IMPLICIT; p.ck_auto = false; p.ck_variant = p.ckh_variant = 0; p.res_mode = 0;
  p.place_mode = 0; p.cut.shape1 = STEP1_DET; p.cut.shape2 = STEP2_DET;
}
static void forced_variant(CreatePlan& p, int variant, int nw, int ng) {
  p.ck_auto = false; p.ck_variant = variant; p.ckh_variant = variant > 0; p.cut.nw = nw; p.cut.ng = ng;
}
static void fp32(CreatePlan& p) { p.fp32_terms = true; p.ck_variant = 1; p.res_mode = 0; p.place_mode = 1; }

#define REFUSED "POVAR_FLAG_FP32_TERMS cannot be combined with "
static const char* const REFUSED_DET = REFUSED "POVAR_FLAG_DETERMINISTIC: its adds land in arrival order";
static const char* const REFUSED_RES = REFUSED "POVAR_FLAG_SERIES_KERNEL(1): the resident series has no fp32 form";
static const char* const REFUSED_LPL = REFUSED "POVAR_FLAG_E0_KERNEL(0): the fp32 terms are a camera-chunk kernel";
static const char* const REFUSED_MODE = REFUSED "an E0 mode other than POVAR_E0_IMPLICIT_LDSACC";
static const char* const BAD_MASK = "POVAR_CU_MASK: expected <first>-<last> inside the device's CU range";

int main() {
  const uint32_t DET = POVAR_FLAG_DETERMINISTIC, F32 = POVAR_FLAG_FP32_TERMS;
  const auto same = [](CreatePlan&) {};
  std::vector<Row> rows;
  const auto row = [&](const char* name, uint32_t flags, Env env, std::function<void(CreatePlan&)> expect) -> Row& {
    rows.push_back(Row{name, flags, std::move(env), std::move(expect)});
    return rows.back();
  };
  const auto refused = [&](const char* name, uint32_t flags, Env env, const char* message) -> Row& {
    Row& r = row(name, flags, std::move(env), same);
    r.rc = -1; r.message = message;
    return r;
  };
  // ---- defaults by size
  row("defaults", 0, {}, same);
  row("65535 observations: lane per observation, no chunk layout", 0, {}, [](CreatePlan& p) { p.use_lpl = p.want_ck = false; }).n_obs = 65535;
  row("65536 observations: lane per landmark", 0, {}, same).n_obs = 65536;
  row("2^20 - 1 observations: rows placed in the call", 0, {}, same).n_obs = (1 << 20) - 1;
  row("2^20 observations: rows placed on a host thread", 0, {}, [](CreatePlan& p) { p.place_mode = 2; }).n_obs = 1 << 20;
  row("1000 observations: 8 resident workgroups at least", 0, {}, [](CreatePlan& p) { p.use_lpl = p.want_ck = false; p.res_wgs = 8; }).n_obs = 1000;
  row("30000 observations: a resident workgroup per 256", 0, {}, [](CreatePlan& p) { p.use_lpl = p.want_ck = false; p.res_wgs = 118; }).n_obs = 30000;
  row("more CUs than resident workgroups exist", 0, {}, [](CreatePlan& p) { p.device_cus = p.e0_wgs = 304; p.res_wgs = 256; }).cus = 304;
  row("the caller's E0 mode is kept", 0, {}, [](CreatePlan& p) { p.e0_mode = POVAR_E0_TILES; }).e0_mode = POVAR_E0_TILES;
  // ---- the environment overrides the flag, both directions
  row("deterministic: flag", DET, {}, det);
  row("deterministic: variable without the flag", 0, {{"POVAR_DETERMINISTIC", "1"}}, det);
  row("deterministic: variable 0 over the flag", DET, {{"POVAR_DETERMINISTIC", "0"}}, same);
  row("NO_GRAPH: flag", POVAR_FLAG_NO_GRAPH, {}, [](CreatePlan& p) { p.use_graph = false; });
  row("NO_GRAPH: variable 0 over the flag", POVAR_FLAG_NO_GRAPH, {{"POVAR_NO_GRAPH", "0"}}, same);
  row("NO_GRAPH: variable without the flag", 0, {{"POVAR_NO_GRAPH", "1"}}, [](CreatePlan& p) { p.use_graph = false; });
  row("E0 kernel: flag value k is variant k (3: 12 wavefronts)", POVAR_FLAG_E0_KERNEL(3), {}, [](CreatePlan& p) { forced_variant(p, 3, 12, 1); });
  row("E0 kernel: flag 0 is e0_lpl, cut as variant 1", POVAR_FLAG_E0_KERNEL(0), {}, [](CreatePlan& p) { forced_variant(p, 0, 16, 1); });
  row("E0 kernel: variable 0 over flag 3", POVAR_FLAG_E0_KERNEL(3), {{"POVAR_E0_CK", "0"}}, [](CreatePlan& p) { forced_variant(p, 0, 16, 1); });
  row("E0 kernel: variable 4 over flag 0 (8 wavefronts in 2 groups)", POVAR_FLAG_E0_KERNEL(0), {{"POVAR_E0_CK", "4"}},
      [](CreatePlan& p) { forced_variant(p, 4, 8, 2); });
  row("E0 kernel: variable 5 (two groups of 8)", 0, {{"POVAR_E0_CK", "5"}}, [](CreatePlan& p) { forced_variant(p, 5, 8, 2); });
  row("E0 kernel: variable 2", 0, {{"POVAR_E0_CK", "2"}}, [](CreatePlan& p) { forced_variant(p, 2, 16, 1); });
  row("E0 kernel: variable above the variants is clamped to 6", 0, {{"POVAR_E0_CK", "9"}}, [](CreatePlan& p) { forced_variant(p, 6, 8, 1); });
  row("E0 kernel: a negative variable over the flag is the timed choice", POVAR_FLAG_E0_KERNEL(2), {{"POVAR_E0_CK", "-1"}}, same);
  row("series kernel: flag 1", POVAR_FLAG_SERIES_KERNEL(1), {}, [](CreatePlan& p) { p.res_mode = 1; });
  row("series kernel: flag 0", POVAR_FLAG_SERIES_KERNEL(0), {}, [](CreatePlan& p) { p.res_mode = 0; });
  row("series kernel: variable 0 over flag 1", POVAR_FLAG_SERIES_KERNEL(1), {{"POVAR_RES", "0"}}, [](CreatePlan& p) { p.res_mode = 0; });
  row("series kernel: variable 1 over flag 0", POVAR_FLAG_SERIES_KERNEL(0), {{"POVAR_RES", "1"}}, [](CreatePlan& p) { p.res_mode = 1; });
  row("placement: flag 2", POVAR_FLAG_PLACEMENT(2), {}, [](CreatePlan& p) { p.place_mode = 2; p.place_forced = true; });
  row("placement: flag 3 is none", POVAR_FLAG_PLACEMENT(3), {}, [](CreatePlan& p) { p.place_mode = 0; p.place_forced = true; });
  row("placement: flag 1 on a large problem", POVAR_FLAG_PLACEMENT(1), {}, [](CreatePlan& p) { p.place_forced = true; }).n_obs = 1 << 20;
  row("placement: variable sync over flag 2", POVAR_FLAG_PLACEMENT(2), {{"POVAR_LPL_PLACE", "sync"}}, [](CreatePlan& p) { p.place_forced = true; });
  row("placement: variable async over flag 1", POVAR_FLAG_PLACEMENT(1), {{"POVAR_LPL_PLACE", "async"}},
      [](CreatePlan& p) { p.place_mode = 2; p.place_forced = true; });
  row("placement: variable none", 0, {{"POVAR_LPL_PLACE", "none"}}, [](CreatePlan& p) { p.place_mode = 0; p.place_forced = true; });
  row("placement: an unknown word keeps the mode, forced", 0, {{"POVAR_LPL_PLACE", "later"}}, [](CreatePlan& p) { p.place_forced = true; });
  row("placement: NOPLACE alone is none, not forced", 0, {{"POVAR_LPL_NOPLACE", "1"}}, [](CreatePlan& p) { p.place_mode = 0; });
  row("placement: NOPLACE over flag 2", POVAR_FLAG_PLACEMENT(2), {{"POVAR_LPL_NOPLACE", "1"}}, [](CreatePlan& p) { p.place_mode = 0; p.place_forced = true; });
  row("placement: NOPLACE loses to PLACE=sync", 0, {{"POVAR_LPL_NOPLACE", "1"}, {"POVAR_LPL_PLACE", "sync"}}, [](CreatePlan& p) { p.place_forced = true; });
  // ---- deterministic mode pins the E0 mode, the kernels and the placement
  row("deterministic: kernels pinned whatever variables and flags say", DET | POVAR_FLAG_E0_KERNEL(2) | POVAR_FLAG_SERIES_KERNEL(1),
      {{"POVAR_E0_CK", "3"}, {"POVAR_RES", "1"}}, det);
  row("deterministic: the gather mode whatever the caller's", DET, {}, det).e0_mode = POVAR_E0_TILES_LDSACC;
  row("deterministic: no host thread on a large problem", DET, {}, det).n_obs = 1 << 20;
  row("deterministic: forced sync is kept", DET, {{"POVAR_LPL_PLACE", "sync"}}, [](CreatePlan& p) { det(p); p.place_mode = 1; p.place_forced = true; });
  row("deterministic: placement flag 1 is kept", DET | POVAR_FLAG_PLACEMENT(1), {}, [](CreatePlan& p) { det(p); p.place_mode = 1; p.place_forced = true; });
  row("deterministic: forced async gives none", DET, {{"POVAR_LPL_PLACE", "async"}}, [](CreatePlan& p) { det(p); p.place_forced = true; });
  const auto det_gather = [](CreatePlan& p) { det(p); p.det_ck = false; p.cut.shape1 = STEP1_COLD_Q; p.cut.shape2 = STEP2; };
  row("deterministic: POVAR_DET_CK=0 clears det_ck", DET, {{"POVAR_DET_CK", "0"}}, det_gather);
  row("deterministic: the gather-terms flag clears det_ck", DET | POVAR_FLAG_DET_GATHER_TERMS, {}, det_gather);
  row("deterministic: POVAR_DET_CK=1 over the gather-terms flag", DET | POVAR_FLAG_DET_GATHER_TERMS, {{"POVAR_DET_CK", "1"}}, det);
  row("the gather-terms flag alone does nothing", POVAR_FLAG_DET_GATHER_TERMS, {{"POVAR_DET_CK", "1"}}, same);
  row("deterministic with HUBER: the det shape, not the plain one", DET, {}, det).robust = POVAR_NORM_HUBER;
  // ---- fp32 terms: four refusals in this order, then what an accepted context is forced to
  refused("fp32: deterministic first", F32 | DET, {{"POVAR_RES", "1"}, {"POVAR_E0_CK", "0"}}, REFUSED_DET).e0_mode = POVAR_E0_IMPLICIT;
  refused("fp32: deterministic by variable", F32, {{"POVAR_DETERMINISTIC", "1"}}, REFUSED_DET);
  refused("fp32: then the forced resident series", F32, {{"POVAR_RES", "1"}, {"POVAR_E0_CK", "0"}}, REFUSED_RES).e0_mode = POVAR_E0_IMPLICIT;
  refused("fp32: resident series by flag", F32 | POVAR_FLAG_SERIES_KERNEL(1), {}, REFUSED_RES);
  refused("fp32: then the forced e0_lpl", F32, {{"POVAR_E0_CK", "0"}}, REFUSED_LPL).e0_mode = POVAR_E0_IMPLICIT;
  refused("fp32: e0_lpl by flag", F32 | POVAR_FLAG_E0_KERNEL(0), {}, REFUSED_LPL);
  refused("fp32: then the E0 mode", F32, {}, REFUSED_MODE).e0_mode = POVAR_E0_IMPLICIT;
  refused("fp32: by variable, refused alike", 0, {{"POVAR_FP32_TERMS", "1"}}, REFUSED_MODE).e0_mode = POVAR_E0_TILES_LDSACC;
  row("fp32: variable 0 over the flag", F32, {{"POVAR_FP32_TERMS", "0"}}, same);
  row("fp32: accepted", F32, {}, fp32);
  row("fp32: the variables that lift a refusing flag", F32 | POVAR_FLAG_SERIES_KERNEL(1) | POVAR_FLAG_E0_KERNEL(0), {{"POVAR_RES", "0"}, {"POVAR_E0_CK", "3"}},
      [](CreatePlan& p) { fp32(p); p.ck_auto = false; p.ckh_variant = 1; });  // (e0_ck_f32 runs variant 1's layout whatever is forced)
  row("fp32: a small problem, POVAR_E0_V1=1 and no placement asked for", F32, {{"POVAR_E0_V1", "1"}, {"POVAR_PREPARE_V1", "1"}, {"POVAR_LPL_PLACE", "none"}},
      [](CreatePlan& p) { fp32(p); p.lpl_forced = true; p.place_forced = true; p.res_wgs = 118; }).n_obs = 30000;
  row("fp32: rows placed in the call on a large problem too", F32, {}, fp32).n_obs = 1 << 20;
  // ---- shapes of step 1's chunk layout
  row("HUBER: records for the cold chunks", 0, {}, [](CreatePlan& p) { p.cut.shape1 = STEP1_RECORDS; }).robust = POVAR_NORM_HUBER;
  row("CAUCHY keeps the cold view", 0, {}, same).robust = POVAR_NORM_CAUCHY;
  row("POVAR_CK_COLD_RECORDS: records", 0, {{"POVAR_CK_COLD_RECORDS", "1"}}, [](CreatePlan& p) { p.cut.shape1 = STEP1_RECORDS; });
  // ---- clamps
  row("POVAR_CK_HMAX below 1", 0, {{"POVAR_CK_HMAX", "0"}}, [](CreatePlan& p) { p.cut.hmax = 1; });
  row("POVAR_CK_HMAX above CK_HMAX", 0, {{"POVAR_CK_HMAX", "99"}}, [](CreatePlan& p) { p.cut.hmax = 16; });
  row("POVAR_CK_HMAX inside", 0, {{"POVAR_CK_HMAX", "5"}}, [](CreatePlan& p) { p.cut.hmax = 5; });
  row("POVAR_HOT_ACC below 1", 0, {{"POVAR_HOT_ACC", "0"}}, [](CreatePlan& p) { p.n_hot_acc = 1; });
  row("POVAR_HOT_ACC inside", 0, {{"POVAR_HOT_ACC", "50"}}, [](CreatePlan& p) { p.n_hot_acc = 50; });
  row("POVAR_HOT_ACC above HOT_ACC_MAX, then the cameras", 0, {{"POVAR_HOT_ACC", "9999"}}, same);
  row("POVAR_HOT_ACC above HOT_ACC_MAX, more cameras", 0, {{"POVAR_HOT_ACC", "9999"}}, [](CreatePlan& p) { p.n_hot_acc = 520; }).n_cams = 1000;
  row("HOT_ACC_MAX cameras at most by default", 0, {}, [](CreatePlan& p) { p.n_hot_acc = 520; }).n_cams = 1000;
  row("POVAR_E0_WGS below 1", 0, {{"POVAR_E0_WGS", "0"}}, [](CreatePlan& p) { p.e0_wgs = 1; });
  row("POVAR_E0_WGS may exceed the CUs", 0, {{"POVAR_E0_WGS", "1000"}}, [](CreatePlan& p) { p.e0_wgs = 1000; });
  row("POVAR_RES_OBS_PER_WG below 64", 0, {{"POVAR_RES_OBS_PER_WG", "10"}}, [](CreatePlan& p) { p.use_lpl = p.want_ck = false; p.res_obs_per_wg = 64; p.res_wgs = 16; }).n_obs = 1000;
  row("POVAR_RES_OBS_PER_WG inside", 0, {{"POVAR_RES_OBS_PER_WG", "1000"}}, [](CreatePlan& p) { p.res_obs_per_wg = 1000; p.res_wgs = 70; });
  row("POVAR_RES_WGS below 1", 0, {{"POVAR_RES_WGS", "0"}}, [](CreatePlan& p) { p.res_wgs = 1; });
  row("POVAR_RES_WGS above the CUs", 0, {{"POVAR_RES_WGS", "200"}}, [](CreatePlan& p) { p.device_cus = p.e0_wgs = 100; p.res_wgs = 100; }).cus = 100;
  row("POVAR_RES_WGS above RES_MAX_WG", 0, {{"POVAR_RES_WGS", "300"}}, [](CreatePlan& p) { p.device_cus = p.e0_wgs = 304; p.res_wgs = 256; }).cus = 304;
  row("POVAR_RES_WGS inside", 0, {{"POVAR_RES_WGS", "12"}}, [](CreatePlan& p) { p.res_wgs = 12; });
  row("POVAR_RES_SPIN below 1", 0, {{"POVAR_RES_SPIN", "0"}}, [](CreatePlan& p) { p.res_spin_limit = 1; });
  row("POVAR_RES_SPIN inside", 0, {{"POVAR_RES_SPIN", "77"}}, [](CreatePlan& p) { p.res_spin_limit = 77; });
  row("POVAR_RES_MAX_OBS", 0, {{"POVAR_RES_MAX_OBS", "1000"}}, [](CreatePlan& p) { p.res_max_obs = 1000; });
  row("POVAR_CK_MAX_CAMS below 0", 0, {{"POVAR_CK_MAX_CAMS", "-5"}}, [](CreatePlan& p) { p.ck_max_cams = 0; });
  row("POVAR_CK_MAX_CAMS inside", 0, {{"POVAR_CK_MAX_CAMS", "10"}}, [](CreatePlan& p) { p.ck_max_cams = 10; });
  // ---- the CU mask
  refused("CU mask: not a range", 0, {{"POVAR_CU_MASK", "half"}}, BAD_MASK);
  refused("CU mask: one number", 0, {{"POVAR_CU_MASK", "12"}}, BAD_MASK);
  refused("CU mask: last before first", 0, {{"POVAR_CU_MASK", "4-2"}}, BAD_MASK);
  refused("CU mask: negative first", 0, {{"POVAR_CU_MASK", "-1-3"}}, BAD_MASK);
  refused("CU mask: past the device's CUs", 0, {{"POVAR_CU_MASK", "0-256"}}, BAD_MASK);
  refused("CU mask: checked before the fp32 refusals", F32 | DET, {{"POVAR_CU_MASK", "0-256"}}, BAD_MASK);
  row("CU mask: the upper half", 0, {{"POVAR_CU_MASK", "128-255"}},
      [](CreatePlan& p) { p.cu_first = 128; p.cu_last = 255; p.cu_limit = 128; p.e0_wgs = 128; p.res_wgs = 128; });
  row("CU mask: one CU", 0, {{"POVAR_CU_MASK", "7-7"}}, [](CreatePlan& p) { p.cu_first = p.cu_last = 7; p.cu_limit = 1; p.e0_wgs = 1; p.res_wgs = 1; });
  row("CU mask: POVAR_E0_WGS and POVAR_RES_WGS against the range", 0, {{"POVAR_CU_MASK", "0-63"}, {"POVAR_E0_WGS", "100"}, {"POVAR_RES_WGS", "100"}},
      [](CreatePlan& p) { p.cu_last = 63; p.cu_limit = 64; p.e0_wgs = 100; p.res_wgs = 64; });
  // ---- the chunk layout is wanted with the lane-per-landmark kernels only
  row("POVAR_NO_CK", 0, {{"POVAR_NO_CK", "1"}}, [](CreatePlan& p) { p.want_ck = false; });
  row("POVAR_E0_V1=1: no lane per landmark, no chunk layout", 0, {{"POVAR_E0_V1", "1"}}, [](CreatePlan& p) { p.use_lpl = p.want_ck = false; p.lpl_forced = true; });
  row("POVAR_E0_V1=0 on a small problem: both", 0, {{"POVAR_E0_V1", "0"}}, [](CreatePlan& p) { p.lpl_forced = true; p.res_wgs = 118; }).n_obs = 30000;
  // ---- the plain switches
  row("POVAR_NO_ERR_MEMO", 0, {{"POVAR_NO_ERR_MEMO", "1"}}, [](CreatePlan& p) { p.no_err_memo = true; });
  row("POVAR_GRAPH_COMM", 0, {{"POVAR_GRAPH_COMM", "1"}}, [](CreatePlan& p) { p.graph_with_comm = true; });
  row("POVAR_NO_FUSE", 0, {{"POVAR_NO_FUSE", "1"}}, [](CreatePlan& p) { p.fuse_binv = false; });
  row("POVAR_NO_FUSE=0", 0, {{"POVAR_NO_FUSE", "0"}}, same);
  row("POVAR_K1_NORMAL_EQ", 0, {{"POVAR_K1_NORMAL_EQ", "1"}}, [](CreatePlan& p) { p.k1_qr = false; });
  row("POVAR_PREPARE_V1", 0, {{"POVAR_PREPARE_V1", "1"}}, [](CreatePlan& p) { p.use_lpl_prepare = false; });
  row("POVAR_CKH_EARLY", 0, {{"POVAR_CKH_EARLY", "1"}}, [](CreatePlan& p) { p.ckh_early = true; });
  row("POVAR_CK_NOPLACE", 0, {{"POVAR_CK_NOPLACE", "1"}}, [](CreatePlan& p) { p.cut.place = false; });
  row("POVAR_FLAG_NO_PACKED_ROWS", POVAR_FLAG_NO_PACKED_ROWS, {}, [](CreatePlan& p) { p.cut.pack = false; });
  row("POVAR_COLD_Q_ROWS=0", 0, {{"POVAR_COLD_Q_ROWS", "0"}}, [](CreatePlan& p) { p.q_rows = 0; });
  row("POVAR_COLD_Q_ROWS=1", 0, {{"POVAR_COLD_Q_ROWS", "1"}}, [](CreatePlan& p) { p.q_rows = 1; });
  row("POVAR_LONG_SEPARATE", 0, {{"POVAR_LONG_SEPARATE", "1"}}, [](CreatePlan& p) { p.long_separate = true; });
  row("POVAR_LAYOUT_TIMING", 0, {{"POVAR_LAYOUT_TIMING", "1"}}, [](CreatePlan& p) { p.timing = true; });

  for (const Row& r : rows) {
    g_env = &r.env;
    povar_options o{};
    o.flags = r.flags; o.e0_mode = r.e0_mode; o.robust_norm = r.robust;
    CreatePlan got;
    std::string err;
    const int rc = resolve_create_plan(got, o, r.n_cams, r.n_obs, r.cus, &err, lookup);
    if (rc != r.rc || err != r.message) {
      std::printf("FAILED %s: returned %d \"%s\", expected %d \"%s\"\n", r.name, rc, err.c_str(), r.rc, r.message);
      ++n_bad;
    }
    if (rc != 0 || r.rc != 0) continue;
    CreatePlan want = base_plan();
    r.expect(want);
    compare(r.name, got, want);
  }
  // without a lookup the process's environment is read, at every call
  {
    povar_options o{};
    o.e0_mode = POVAR_E0_IMPLICIT_LDSACC;
    CreatePlan got, want = base_plan();
    std::string err;
    setenv("POVAR_NO_FUSE", "1", 1);
    if (resolve_create_plan(got, o, 100, 70000, 256, &err) != 0) { std::printf("FAILED process environment: refused\n"); ++n_bad; }
    want.fuse_binv = false;
    compare("process environment: set", got, want);
    unsetenv("POVAR_NO_FUSE");
    if (resolve_create_plan(got, o, 100, 70000, 256, &err) != 0) { std::printf("FAILED process environment: refused\n"); ++n_bad; }
    compare("process environment: unset again", got, base_plan());
  }
  if (n_bad) return 1;
  std::printf("create_plan_check: ok (%zu rows)\n", rows.size());
  return 0;
}
