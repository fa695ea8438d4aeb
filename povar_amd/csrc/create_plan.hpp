// create_plan.hpp -- what a context is going to be, decided in ONE place before povar_create builds anything: povar_options.flags,
// the POVAR_* environment variables of povar_create and the problem's size resolve to a CreatePlan (resolve_create_plan), and the
// phases of povar_create only read it.  Host-only (no HIP runtime call, no context): tests/cpp/create_plan_check.cpp holds the
// precedence rules below to a table.  An environment variable that is set overrides its flag (diagnosis, the forced-mode suites);
// the environment is looked up at every call, never cached.  The knobs of the layout builders themselves (POVAR_LPL_*, POVAR_CK_NB,
// POVAR_CK_TILE_COST, POVAR_CKH_STRIDE, POVAR_CKH_ACC_CAP, POVAR_CK_COLD_Q_ALWAYS, POVAR_CK_PACK, POVAR_LAYOUT_THREADS) stay with them.
#pragma once
#include "../../include/povar_hip.h"
#include "ck_layout.hpp"
#include "res_layout.hpp"

#include <string>

namespace povar {

// e0_ck instantiations (CreatePlan::ck_variant): wavefronts per workgroup, rows a tile keeps in flight, double-buffered
// tile records, groups of wavefronts working on different batches (povar_kernels_ck.hpp)
#define POVAR_CK_VARIANTS(X) \
  X(1, 16, 2, false, 1) X(2, 16, 4, false, 1) X(3, 12, 2, true, 1) X(4, 16, 2, false, 2) X(5, 16, 4, false, 2) X(6, 8, 2, true, 1)
constexpr int CK_VARIANTS = 6;
struct CkVariant { int nw, sd; bool db; int ng; };
inline CkVariant ck_variant_info(int variant) {
  switch (variant) {
#define X(id, nw, sd, db, ng) case id: return CkVariant{nw, sd, db, ng};
    POVAR_CK_VARIANTS(X)
#undef X
    default: return CkVariant{16, 2, false, 1};
  }
}

// How the camera-chunk layouts are cut: for the instantiation that will run them (the tiles are scheduled over its wavefronts).
struct CkCut {
  int nw = 16, ng = 1;   // step 1: wavefronts of ONE group, groups (step 2 has one instantiation: 16 wavefronts, one group)
  int hmax = CK_HMAX;    // POVAR_CK_HMAX: most observations per chunk
  bool place = true;     // LDS bank placement of the chunk rows (ck_layout.hpp); POVAR_CK_NOPLACE
  bool pack = true;      // packed image points where they pack (POVAR_FLAG_NO_PACKED_ROWS; POVAR_CK_PACK=0 overrides inside build_ck)
  // step 1's layout: batches cut for the kernel that runs them; e0_ck leaves q of its cold observations in the parent's cold view
  // (not with the HUBER norm: e0_ck<..., ROBUST = true> has no cold loop -- povar_kernels_ck.hpp; not with POVAR_CK_COLD_RECORDS)
  CkShape shape1, shape2;
};

// The part of the plan a context keeps (povar_ctx derives from it): the switches the other units read after povar_create,
// some of which the setters of the C ABI change later (povar_set_e0_kernel, povar_set_series_kernel).
struct CtxSwitches {
  // POVAR_DETERMINISTIC=1: run-to-run BIT-reproducible results for a given device count (SURVEY 8(e) "fixed reduction order
  // inside a GPU"), whatever E0 mode the caller asked for, and no run-time timing decides a kernel:
  //   * linearisation, preparation and cost of both steps run in the gather mode (POVAR_E0_IMPLICIT: per-landmark wavefront
  //     scans, per-camera sums through the camera-major index -- no atomics anywhere);
  //   * the terms of the power series -- the hot path -- run e0_ck_det (step 1) / e0_ck_h_det (step 2)
  //     (povar_kernels_ck_det.hpp: the camera-chunk kernels with the landmark sums in 64-bit fixed point -- integer adds are
  //     associative -- and the accumulator adds in ticket order) + cam_cold_sum_binv[_h] (a fixed-order sum), on the landmark
  //     records and camera image the gather mode's kernels leave in lane order anyway.  POVAR_DET_CK=0: the gather form there
  //     too (3.7 x slower than the default mode on venice-1778, profiles/r05_experiments.txt; also what runs when a chunk
  //     layout does not fit);
  //   * the rows are never placed on a host thread (when they arrive would decide the bits of every later solve).
  // The default mode accumulates in LDS in arrival order and is reproducible to rounding (1e-15), like the reference's
  // mutex order.
  // deterministic: the E0 mode and the kernel choices are pinned; det_ck: ... and step 1's terms run e0_ck_det where the chunk
  // layout fits (else: the gather form)
  bool deterministic = false, det_ck = false;
  // POVAR_FLAG_FP32_TERMS (POVAR_FP32_TERMS=1|0): step 1's power-series terms in single precision (e0_ck_f32, povar_kernels_ck_f32.hpp).
  // The kernel is a camera-chunk kernel that adds in arrival order and runs per term: the switches that promise something else are
  // refused, not overridden.  It runs on the chunk layout of variant 1 whatever the size (use_lpl), on rows placed in the call.
  bool fp32_terms = false;
  bool use_graph = true, graph_with_comm = false;  // hipGraph of the m-term loop (POVAR_NO_GRAPH); also with a communicator (POVAR_GRAPH_COMM)
  bool no_err_memo = false;     // POVAR_NO_ERR_MEMO=1: evaluate every compute_error call (timing the kernel itself)
  bool fuse_binv = true;        // POVAR_NO_FUSE=1: keep cam_cold_sum and cam_binv_axpy separate
  // A problem that gives the 256 x 16 wavefronts of the lane-per-landmark kernels less than a row each is bound by the
  // launch of the 1024-thread workgroups: the lane-per-observation kernels of round 1 are faster there (ladybug-49,
  // 31 843 observations: 127 k against 106 k terms/s; trafalgar-257, 225 911: 64.9 k against 67.0 k).
  // use_lpl: from 65536 observations on; POVAR_E0_V1=1: keep e0_lm_cached<true> (lane per observation) for A/B runs
  // lpl_forced: POVAR_E0_V1 set: keep the choice (the peer-to-peer exchange otherwise turns use_lpl on)
  bool use_lpl = true, lpl_forced = false;
  bool use_lpl_prepare = true;  // POVAR_PREPARE_V1=1: keep lm_regular<OpPrepare> + cm_scatter
  bool k1_qr = true;            // POVAR_K1_NORMAL_EQ=1: the round-1 normal-equation kernels (A/B accuracy runs)
  // ck_variant: 0: e0_lpl; 1..CK_VARIANTS: e0_ck instantiation (POVAR_E0_CK=<variant>, povar_set_e0_kernel); ckh_variant: step 2:
  // 0: e0_lpl_h; 1: e0_ck_h
  int ck_variant = 0, ckh_variant = 0;
  bool ck_auto = true;          // the library picks e0_lpl or e0_ck by timing both on this problem (ck_autotune); false: forced
  // resident power series (res_layout.hpp): for contexts whose observations fit the lanes' registers.  -1: the library times
  // it against the per-term kernels once per context (res_autotune); 0: per-term kernels; 1: resident series whenever the
  // context allows (POVAR_RES=0|1)
  int res_mode = -1;
  unsigned res_spin_limit = 1u << 18;  // POVAR_RES_SPIN: polls a hand-over waits before the launch gives up
  int n_hot_acc = 0;            // cameras whose Jp^T s is accumulated in LDS (POVAR_HOT_ACC=<n> lowers it: tuning knob)
  int ck_max_cams = 65535;      // POVAR_CK_MAX_CAMS lowers the camera limit of the camera-chunk kernels (tests: the fall-back to e0_lpl)
};

// ... and what povar_create alone reads.
struct CreatePlan : CtxSwitches {
  bool timing = false;  // POVAR_LAYOUT_TIMING: the phases of povar_create with their wall times on stderr
  // POVAR_CU_MASK=<first>-<last>: the context's stream runs on that range of CUs only.  For several contexts that share ONE
  // device and wait for each other inside kernels (the peer-to-peer term exchange with two ranks on a one-GPU box): an
  // E0 workgroup takes a CU's whole register file, so the bounded spin of one rank's reduce kernel on every CU kept the
  // other rank's E0 kernel off the device until the spin timed out.  Disjoint CU ranges make the ranks two half devices.
  int device_cus = 0, cu_first = 0, cu_last = -1;
  int cu_limit = 0;  // CUs of the range (0: no mask, the whole device): "one workgroup per CU" then means per CU of the range
  int e0_mode = 0;  // the caller's, POVAR_E0_IMPLICIT on a deterministic context
  bool want_ck = false;  // build the camera-chunk layouts: with the lane-per-landmark kernels, unless POVAR_NO_CK
  CkCut cut;
  bool ckh_early = false;  // POVAR_CKH_EARLY: with placement 2, step 2's chunk layout from the natural rows inside the call too
  // LDS bank placement of the lane-per-landmark rows: 0 none, 1 in the call, 2 on a host thread (from 2^20 observations on).
  // Deterministic: never on a host thread -- WHEN the placed rows (and the chunk layout cut from them: another, equally fixed
  // summation order) arrive would depend on the host's timing, and with it the bits of every later solve.  None at all unless
  // asked for: the gather-mode kernels do not read these rows, e0_ck_det does not care about their order.
  int place_mode = 1;
  bool place_forced = false;
  int q_rows = -1;  // POVAR_COLD_Q_ROWS=0|1 (-1: by the cold share, povar_ctx::q_rows)
  // (measured, profiles/r05_res_term_times.txt: ahead of the per-term kernels up to a shard of 313 k observations, behind them
  // on one of 625 k, where the partial records -- 21.7 MB written and read per term -- are the term)
  int64_t res_max_obs = 400000;  // POVAR_RES_MAX_OBS: no resident-series layout beyond
  int res_obs_per_wg = 256;  // POVAR_RES_OBS_PER_WG (ladybug-49: 32 workgroups 8.7, 63: 7.5, 125: 7.3 us per term -- the phases of a term are the workgroup's size)
  int res_wgs = 0;           // workgroups of the resident series (POVAR_RES_WGS, at most the CUs and RES_MAX_WG)
  int e0_wgs = 1;            // one 1024-thread workgroup per CU for the LDS-cached E0 kernels (POVAR_E0_WGS: tuning knob)
  bool long_separate = false;  // POVAR_LONG_SEPARATE: keep the lm_long kernel (lane-per-observation kernels only)
};

using EnvLookup = const char* (*)(const char*);

// 0, or the negative code of povar_create with its message in *err.
inline int resolve_create_plan(CreatePlan& p, const povar_options& o, int n_cams, int64_t n_obs, int device_cus, std::string* err,
                               EnvLookup env = [](const char* k) -> const char* { return std::getenv(k); }) {
  p = CreatePlan();
  const uint32_t fl = o.flags;
  const auto field = [fl](uint32_t mask, int shift) { return (int)((fl & mask) >> shift); };
  const auto refuse = [err](const std::string& why) { *err = why; return -1; };
  const auto is1 = [env](const char* name, bool unset) { const char* e = env(name); return e ? e[0] == '1' : unset; };
  p.timing = env("POVAR_LAYOUT_TIMING") != nullptr;
  p.device_cus = device_cus;
  if (const char* g = env("POVAR_CU_MASK")) {
    if (std::sscanf(g, "%d-%d", &p.cu_first, &p.cu_last) != 2 || p.cu_first < 0 || p.cu_last < p.cu_first || p.cu_last >= device_cus)
      return refuse("POVAR_CU_MASK: expected <first>-<last> inside the device's CU range");
    p.cu_limit = p.cu_last - p.cu_first + 1;
  }
  const int cus = std::max(p.cu_limit > 0 ? p.cu_limit : device_cus, 1);
  p.deterministic = is1("POVAR_DETERMINISTIC", (fl & POVAR_FLAG_DETERMINISTIC) != 0);
  const char* det_ck_env = env("POVAR_DET_CK");
  p.det_ck = p.deterministic && !(det_ck_env ? det_ck_env[0] == '0' : (fl & POVAR_FLAG_DET_GATHER_TERMS) != 0);
  p.e0_mode = p.deterministic ? (int)POVAR_E0_IMPLICIT : o.e0_mode;
  // the forced kernels: -1 timed; E0 0 e0_lpl, 1.. an e0_ck instantiation; series 0 per-term kernels, 1 resident
  const char *ek = env("POVAR_E0_CK"), *rs = env("POVAR_RES");
  const int e0k = ek ? std::atoi(ek) : field(POVAR_FLAG_E0_KERNEL_MASK, POVAR_FLAG_E0_KERNEL_SHIFT) - 1;
  const int series = rs ? (rs[0] == '1' ? 1 : 0) : field(POVAR_FLAG_SERIES_KERNEL_MASK, POVAR_FLAG_SERIES_KERNEL_SHIFT) - 1;
  if (is1("POVAR_FP32_TERMS", (fl & POVAR_FLAG_FP32_TERMS) != 0)) {
    const char* why = p.deterministic ? "POVAR_FLAG_DETERMINISTIC: its adds land in arrival order"
                      : series == 1 ? "POVAR_FLAG_SERIES_KERNEL(1): the resident series has no fp32 form"
                      : e0k == 0 ? "POVAR_FLAG_E0_KERNEL(0): the fp32 terms are a camera-chunk kernel"
                      : o.e0_mode != POVAR_E0_IMPLICIT_LDSACC ? "an E0 mode other than POVAR_E0_IMPLICIT_LDSACC"
                      : nullptr;
    if (why) return refuse(std::string("POVAR_FLAG_FP32_TERMS cannot be combined with ") + why);
    p.fp32_terms = true;
  }
  p.use_graph = !is1("POVAR_NO_GRAPH", (fl & POVAR_FLAG_NO_GRAPH) != 0);
  p.no_err_memo = is1("POVAR_NO_ERR_MEMO", false); p.graph_with_comm = is1("POVAR_GRAPH_COMM", false); p.fuse_binv = !is1("POVAR_NO_FUSE", false);
  p.lpl_forced = env("POVAR_E0_V1") != nullptr;
  p.use_lpl = p.fp32_terms || (p.lpl_forced ? !is1("POVAR_E0_V1", false) : n_obs >= 65536);
  p.k1_qr = !is1("POVAR_K1_NORMAL_EQ", false); p.use_lpl_prepare = p.fp32_terms || !is1("POVAR_PREPARE_V1", false);
  p.ck_auto = !p.deterministic && e0k < 0;
  if (!p.ck_auto && !p.deterministic) {
    p.ck_variant = std::max(0, std::min(CK_VARIANTS, e0k));
    p.ckh_variant = p.ck_variant > 0 ? 1 : 0;  // (step 2 has one camera-chunk instantiation)
  }
  if (p.fp32_terms) p.ck_variant = 1;  // e0_ck_f32 runs the layout of variant 1 (16 wavefronts, one group)
  p.want_ck = p.use_lpl && env("POVAR_NO_CK") == nullptr;
  const CkVariant ckv = ck_variant_info(p.ck_variant > 0 ? p.ck_variant : 1);
  p.cut.nw = ckv.nw / ckv.ng; p.cut.ng = ckv.ng;
  if (const char* e = env("POVAR_CK_HMAX")) p.cut.hmax = std::min(CK_HMAX, std::max(1, std::atoi(e)));
  p.cut.place = env("POVAR_CK_NOPLACE") == nullptr; p.cut.pack = !(fl & POVAR_FLAG_NO_PACKED_ROWS);
  p.cut.shape1 = p.det_ck ? ck_shape_det()
                 : (env("POVAR_CK_COLD_RECORDS") || o.robust_norm == POVAR_NORM_HUBER) ? CkShape()
                 : ck_shape_step1();
  p.cut.shape2 = p.det_ck ? ck_shape_step2_det() : ck_shape_step2();
  p.ckh_early = env("POVAR_CKH_EARLY") != nullptr;
  p.place_mode = n_obs >= (1 << 20) ? 2 : 1;
  if (const int pf = field(POVAR_FLAG_PLACEMENT_MASK, POVAR_FLAG_PLACEMENT_SHIFT)) { p.place_mode = pf == 3 ? 0 : pf; p.place_forced = true; }
  if (env("POVAR_LPL_NOPLACE")) p.place_mode = 0;
  if (const char* e = env("POVAR_LPL_PLACE")) { p.place_mode = e[0] == 'n' ? 0 : e[0] == 's' ? 1 : e[0] == 'a' ? 2 : p.place_mode; p.place_forced = true; }
  if (p.deterministic) p.place_mode = p.place_mode == 1 && p.place_forced ? 1 : 0;
  if (p.fp32_terms) p.place_mode = 1;  // the rows placed in this call: every solve, from the first, runs the fp32 terms
  if (const char* e = env("POVAR_COLD_Q_ROWS")) p.q_rows = e[0] == '1';
  if (p.deterministic || p.fp32_terms) p.res_mode = 0;
  if (series >= 0 && !p.deterministic) p.res_mode = series;
  if (const char* e = env("POVAR_RES_SPIN")) p.res_spin_limit = (unsigned)std::max(1, std::atoi(e));
  if (const char* e = env("POVAR_RES_MAX_OBS")) p.res_max_obs = std::atoll(e);
  if (const char* e = env("POVAR_RES_OBS_PER_WG")) p.res_obs_per_wg = std::max(64, std::atoi(e));
  const int res_cus = std::min(cus, RES_MAX_WG);
  p.res_wgs = (int)std::min<int64_t>(res_cus, std::max<int64_t>(8, (n_obs + p.res_obs_per_wg - 1) / p.res_obs_per_wg));
  if (const char* e = env("POVAR_RES_WGS")) p.res_wgs = std::max(1, std::min(std::atoi(e), res_cus));
  p.e0_wgs = cus;
  if (const char* e = env("POVAR_E0_WGS")) p.e0_wgs = std::max(std::atoi(e), 1);
  const char* acc = env("POVAR_HOT_ACC");
  p.n_hot_acc = std::min(n_cams, acc ? std::max(1, std::min(HOT_ACC_MAX, std::atoi(acc))) : HOT_ACC_MAX);
  if (const char* e = env("POVAR_CK_MAX_CAMS")) p.ck_max_cams = std::max(0, std::atoi(e));
  p.long_separate = env("POVAR_LONG_SEPARATE") != nullptr;
  return 0;
}

}  // namespace povar
