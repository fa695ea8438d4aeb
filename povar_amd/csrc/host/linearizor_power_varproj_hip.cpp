// LinearizorPowerVarproj (solver/linearizor_power_varproj.cpp:21-308 + solver/linearizor_base.cpp:48-100)
// and LinearizorSC (solver/linearizor_sc.cpp:50-360; PCG / CHOLESKY / RIPCG) on top of the C ABI of
// include/povar_hip.h: the two reference classes differ in solve()/solve_joint() and in the Jl column
// scaling of step 1 only, so one class serves both.  The device context owns cameras and landmarks
// between calls; BalProblem forwards backup/restore/normalise through StateMirror.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <memory>
#include <cstring>
#include <cstdlib>

#include "../../../include/povar_hip.h"
#include "linearizor.hpp"
#include "shard_team.hpp"

namespace povar_host {

namespace {

#define IF_SET(P) if (P) P

void check(int rc, const char* what) {
  if (rc < 0) {  // hard failures abort like CHECK / LOG(FATAL) (linearizor_power_varproj.cpp:59-60)
    std::fprintf(stderr, "FATAL: %s failed (%d): %s\n", what, rc, povar_last_error());
    std::abort();
  }
}

// what a device context is built from: sizes, options, every (camera, u, v) in landmark order
std::string context_key(const BalProblem& p, const povar_options& o) {
  unsigned long long h = 1469598103934665603ull;
  auto mix = [&](unsigned long long v) { h = (h ^ v) * 1099511628211ull; };
  long n_obs = 0;
  for (const auto& lm : p.landmarks()) {
    mix(lm.obs.size());
    for (const auto& kv : lm.obs) {
      unsigned long long bu, bv;
      std::memcpy(&bu, &kv.second[0], 8);
      std::memcpy(&bv, &kv.second[1], 8);
      mix((unsigned long long)kv.first);
      mix(bu);
      mix(bv);
    }
    n_obs += (long)lm.obs.size();
  }
  char buf[256];
  std::snprintf(buf, sizeof buf, "%d/%d/%ld/%016llx/norm%d/%.17g/%.17g/dev%d/e0%d/f%x", p.num_cameras(), p.num_landmarks(), n_obs, h,
                o.robust_norm, o.huber_parameter, o.jacobi_scaling_eps, o.device, o.e0_mode, o.flags);
  return buf;
}

ResidualInfo to_ri(const povar_residual_info& r) {
  ResidualInfo o;
  o.all = {r.all_num_obs, r.all_error, r.all_residual_sum};
  o.valid = {r.valid_num_obs, r.valid_error, r.valid_residual_sum};
  o.is_numerically_valid = r.is_numerically_valid != 0;
  return o;
}

// One device context, or N landmark shards in one process (BASELINE configs 4 / 5; SURVEY 8(b): "one context per process
// drives all local GPUs").  Every virtual is "the same call on every shard, then rank 0's answer": cameras and every
// per-camera result are replicated (identical on all ranks after the library's exchange steps), landmarks live on the
// shard that owns them.
//   not sharded: one shard over all landmarks, the calls made on the caller's thread (a ShardTeam without a worker); the
//                context is parked in BalProblem::device_cache between step 1 and step 2.
//   sharded:     one ShardTeam worker per shard context (shard_team.hpp says why).  Exchange: RCCL (povar_comm_init) when
//                the shards sit on distinct devices; an in-process all-reduce through the library's host hook
//                (povar_comm_init_host) when they share one (RCCL refuses duplicate devices) or POVAR_HOST_COMM=1.
//                Serves the power-series solvers; no camera covariance; no context cache.
class LinearizorPowerVarprojHip : public Linearizor, public StateMirror {
 public:
  LinearizorPowerVarprojHip(BalProblem& bal_problem, const SolverOptions& options, SolverSummary* summary, bool homogeneous,
                            bool sharded)
      : options_(options), bal_problem_(bal_problem), summary_(summary), homogeneous_(homogeneous), sharded_(sharded),
        team_(options.gpus, sharded), shards_(team_.size()) {
    using ST = SolverOptions::SolverType;
    using ST2 = SolverOptions::SolverTypeRiemannian;
    const bool sc1 = options.solver_type_step_1 == ST::PCG || options.solver_type_step_1 == ST::CHOLESKY;
    const bool sc2 = options.solver_type_step_2 == ST2::RIPCG || options.solver_type_step_2 == ST2::RICHOLESKY;
    if (sharded && (sc1 || sc2)) {
      std::fprintf(stderr, "FATAL: --gpus > 1 serves the power-series solvers (POWER_VARPROJ, POWER_SCHUR_COMPLEMENT, RIPOBA)\n");
      std::abort();
    }
    sc_step1_ = !homogeneous && sc1;
    sc_step2_ = homogeneous && sc2;
    povar_options o{};
    o.robust_norm = (int)options.residual.robust_norm;
    o.huber_parameter = options.residual.huber_parameter;
    // get_effective_jacobi_scaling_epsilon, linearizor_base.cpp:94-100 (Sophus epsilonSqrt<double> = 1e-5)
    o.jacobi_scaling_eps = options.jacobi_scaling_epsilon > 0 ? options.jacobi_scaling_epsilon : 1e-5;
    o.device = options.device;  // (sharded: the first shard's; shard r sits r devices further on)
    o.e0_mode = options.e0_mode == "tiles" ? POVAR_E0_TILES
                : options.e0_mode == "implicit" ? POVAR_E0_IMPLICIT : POVAR_E0_IMPLICIT_LDSACC;
    o.flags = (options.deterministic ? POVAR_FLAG_DETERMINISTIC : 0u) | (options.fp32_terms ? POVAR_FLAG_FP32_TERMS : 0u);
    if (sharded) create_shards(o); else create_or_take_over(o);
    all([&](Shard& s, int r) {
      // LinearizorSC::linearize_pOSE does not scale the landmark Jacobian columns (linearizor_sc.cpp:163-191)
      check(povar_set_jl_col_scaling(s.ctx, sc_step1_ ? 0 : 1), "povar_set_jl_col_scaling");
      // IterationSummary timings come from the device (hipEvents on the library's stream, povar_timings), not from
      // host clocks around the calls; rank 0's (the ranks run the same calls side by side)
      if (r == 0) check(povar_timings_enable(s.ctx, 1), "povar_timings_enable");
      // --fixed-cameras: the same set on every shard context (an empty one clears what a context taken over from step 1 holds)
      check(povar_set_fixed_cameras(s.ctx, options.fixed_cameras.data(), (int32_t)options.fixed_cameras.size()), "povar_set_fixed_cameras");
      // --compact-fixed-cameras: likewise the layout of the dense matrix (0 again on a context taken over from step 1)
      check(povar_set_dense_compaction(s.ctx, options.dense_compaction ? 1 : 0), "povar_set_dense_compaction");
    });
    cov_gauge_ = options.fixed_cameras.empty() ? POVAR_COV_FREE_GAUGE : POVAR_COV_FIXED_GAUGE;
    push_state();
    bal_problem_.mirror = this;
  }
  ~LinearizorPowerVarprojHip() override {
    pull_state();
    bal_problem_.mirror = nullptr;
    if (sharded_) {
      all([&](Shard& s, int) { povar_destroy(s.ctx); });
    } else {
      bal_problem_.device_cache.ctx = std::move(holder_);  // destroyed with the problem, or taken over by the next linearizor
      bal_problem_.device_cache.key = cache_key_;
    }
  }

  bool holds_fixed_cameras() const override { return true; }
  void start_iteration(IterationSummary* it) override { it_summary_ = it; }
  void finish_iteration() override {}

  void initialize_varproj_lm_pOSE(double alpha, bool initialization_varproj) override {
    if (initialization_varproj) all([&](Shard& s, int) { check(povar_init_landmarks_pose(s.ctx, alpha), "povar_init_landmarks_pose"); });
  }
  void compute_error_pOSE(ResidualInfo& ri, bool) override { compute_error(false, ri); }
  void compute_error_homogeneous(ResidualInfo& ri, bool) override { compute_error(true, ri); }
  void linearize_pOSE(double alpha) override {
    linearize_all(false, alpha, "povar_linearize_pose");
    book_linearize();
  }
  void linearize_projective_space_homogeneous() override {
    linearize_all(true, 0.0, "povar_linearize_homogeneous");
    book_linearize();
  }
  // Gauge of all of them: the free gauge, or with --fixed-cameras the gauge those cameras fix (POVAR_COV_FIXED_GAUGE).
  // The three covariance calls are the library calls themselves: they run after the LM loop, when the iteration summary
  // start_iteration handed over is gone and the solver summary is finished -- no timing or evaluation count is booked.
  // Sharded, every shard linearises and calls (the assembly is all-reduced, every rank inverts the same matrix) and writes
  // the blocks of its own landmarks / the rows of its own observations at their place in file order.
  int camera_covariance(bool step2, double alpha, VecX& cov) override {
    if (sharded_) return -1;
    cov.assign(144 * (size_t)bal_problem_.num_cameras(), 0.0);
    linearize_all(step2, alpha, "povar_linearize (camera covariance)");
    return covariance_status("povar_camera_covariance", [&](Shard& s) {
      return step2 ? povar_camera_covariance_joint(s.ctx, 0.0, cov_gauge_, POVAR_COV_CAMERA_COORDS, cov.data())
                   : povar_camera_covariance_pose(s.ctx, 0.0, cov_gauge_, POVAR_COV_CAMERA_COORDS, cov.data());
    });
  }
  int landmark_covariance(bool step2, double alpha, VecX& lm_cov, VecX* cam_cov) override {
    if (cam_cov && sharded_) return -1;  // (the camera file is the single device's)
    const size_t stride = step2 ? 16 : 9;
    lm_cov.assign(stride * (size_t)bal_problem_.num_landmarks(), 0.0);
    if (cam_cov) cam_cov->assign(144 * (size_t)bal_problem_.num_cameras(), 0.0);
    linearize_all(step2, alpha, "povar_linearize (landmark covariance)");
    double* cam = cam_cov ? cam_cov->data() : nullptr;
    return covariance_status("povar_landmark_covariance", [&](Shard& s) {
      double* out = lm_cov.data() + stride * (size_t)s.lb;
      return step2 ? povar_landmark_covariance_joint(s.ctx, 0.0, cov_gauge_, POVAR_COV_LANDMARK_COORDS, nullptr, 0, out, cam)
                   : povar_landmark_covariance_pose(s.ctx, 0.0, cov_gauge_, POVAR_COV_LANDMARK_COORDS, nullptr, 0, out, cam);
    });
  }
  int observation_covariance(bool step2, double alpha, VecX& obs_cov) override {
    obs_cov.assign(4 * (size_t)bal_problem_.num_observations(), 0.0);
    linearize_all(step2, alpha, "povar_linearize (observation covariance)");
    return covariance_status("povar_observation_covariance", [&](Shard& s) {
      double* out = obs_cov.data() + 4 * (size_t)s.ob;
      return step2 ? povar_observation_covariance_joint(s.ctx, 0.0, cov_gauge_, nullptr, 0, out, s.on)
                   : povar_observation_covariance_pose(s.ctx, 0.0, cov_gauge_, nullptr, 0, out, s.on);
    });
  }
  int observation_hat(bool step2, double alpha, VecX& rows) override {
    const size_t stride = step2 ? 5 : 14;
    rows.assign(stride * (size_t)bal_problem_.num_observations(), 0.0);
    linearize_all(step2, alpha, "povar_linearize (observation diagnostics)");
    return covariance_status("povar_observation_hat", [&](Shard& s) {
      double* out = rows.data() + stride * (size_t)s.ob;
      return step2 ? povar_observation_hat_joint(s.ctx, 0.0, cov_gauge_, nullptr, 0, out, s.on)
                   : povar_observation_hat_pose(s.ctx, 0.0, cov_gauge_, nullptr, 0, out, s.on);
    });
  }
  int covariance_blocks(bool step2, double alpha, const std::vector<int32_t>& pairs, VecX& blocks) override {
    if (sharded_) return -1;  // (landmark ids are the shard's own)
    linearize_all(step2, alpha, "povar_linearize (covariance blocks)");
    return covariance_status("povar_covariance_blocks", [&](Shard& s) {
      const int32_t n = (int32_t)(pairs.size() / 4);
      return step2 ? povar_covariance_blocks_joint(s.ctx, 0.0, cov_gauge_, POVAR_COV_CAMERA_COORDS, pairs.data(), n, blocks.data(),
                                                   (int64_t)blocks.size())
                   : povar_covariance_blocks_pose(s.ctx, 0.0, cov_gauge_, POVAR_COV_CAMERA_COORDS, pairs.data(), n, blocks.data(),
                                                  (int64_t)blocks.size());
    });
  }
  VecX solve(const SolverOptions& so, double lambda, double) override {
    std::vector<Solved> out(shards_.size(), Solved{VecX(12 * (size_t)bal_problem_.num_cameras()), 0, 0});
    if (sc_step1_) {  // LinearizorSC::solve, linearizor_sc.cpp:85-160
      const bool chol = so.solver_type_step_1 == SolverOptions::SolverType::CHOLESKY;
      if (!chol) require_schur_jacobi();
      all([&](Shard& s, int k) {
        check(povar_solve_pose_sc(s.ctx, lambda, chol ? POVAR_SC_CHOLESKY : POVAR_SC_PCG, options_.min_linear_solver_iterations,
                                  options_.max_linear_solver_iterations, options_.eta, out[k].inc.data(), &out[k].iters, &out[k].term),
              "povar_solve_pose_sc");
      });
      return book_solve(out[0], true, chol);
    }
    const int st = power_solver_type(so);
    all([&](Shard& s, int k) {
      check(povar_prepare_pose(s.ctx, lambda, st), "povar_prepare_pose");
      check(povar_power_series_pose(s.ctx, options_.power_sc_iterations, options_.eta, options_.r_tolerance, &out[k].iters, &out[k].term),
            "povar_power_series_pose");
      check(povar_get_increment(s.ctx, out[k].inc.data()), "povar_get_increment");
    });
    return book_solve(out[0], false);
  }
  VecX solve_joint(double lambda, double) override {
    std::vector<Solved> out(shards_.size(), Solved{VecX(11 * (size_t)bal_problem_.num_cameras()), 0, 0});
    if (sc_step2_) {  // LinearizorSC::solve_joint, linearizor_sc.cpp:224-303; RICHOLESKY: the direct solve (not in the reference)
      const bool chol = options_.solver_type_step_2 == SolverOptions::SolverTypeRiemannian::RICHOLESKY;
      if (!chol) require_schur_jacobi();
      all([&](Shard& s, int k) {
        check(povar_solve_joint_sc_method(s.ctx, lambda, chol ? POVAR_SC_CHOLESKY : POVAR_SC_PCG, options_.min_linear_solver_iterations,
                                          options_.max_linear_solver_iterations, options_.eta, out[k].inc.data(), &out[k].iters,
                                          &out[k].term), "povar_solve_joint_sc_method");
      });
      return book_solve(out[0], true, chol);
    }
    all([&](Shard& s, int k) {
      check(povar_solve_joint(s.ctx, lambda, options_.power_sc_iterations, options_.eta, options_.r_tolerance, out[k].inc.data(),
                              &out[k].iters, &out[k].term), "povar_solve_joint");
    });
    return book_solve(out[0], false);
  }
  double apply(const SolverOptions& so, double alpha, VecX&& inc) override {
    const int st = power_solver_type(so);
    return apply_all([&](Shard& s, double* l_diff) { check(povar_apply_pose(s.ctx, st, alpha, inc.data(), l_diff), "povar_apply_pose"); });
  }
  double apply_joint(VecX&& inc) override {
    return apply_all([&](Shard& s, double* l_diff) { check(povar_apply_joint(s.ctx, inc.data(), l_diff), "povar_apply_joint"); });
  }

  // StateMirror
  void backup_pOSE() override { all([&](Shard& s, int) { check(povar_backup_pose(s.ctx), "povar_backup_pose"); }); }
  void restore_pOSE() override { all([&](Shard& s, int) { check(povar_restore_pose(s.ctx), "povar_restore_pose"); }); }
  void backup_joint() override { all([&](Shard& s, int) { check(povar_backup_joint(s.ctx), "povar_backup_joint"); }); }
  void restore_joint() override { all([&](Shard& s, int) { check(povar_restore_joint(s.ctx), "povar_restore_joint"); }); }
  void normalize_joint() override { all([&](Shard& s, int) { check(povar_normalize_joint(s.ctx), "povar_normalize_joint"); }); }
  void pull_state() override {
    const int nc = bal_problem_.num_cameras();
    const int w = homogeneous_ ? 4 : 3;
    std::vector<double> cams(12 * (size_t)nc);
    all([&](Shard& s, int k) {
      if (k == 0) check(povar_get_cameras(s.ctx, cams.data()), "povar_get_cameras");
      std::vector<double> lms((size_t)w * (s.le - s.lb));
      if (homogeneous_) check(povar_get_landmarks_homogeneous(s.ctx, lms.data()), "povar_get_landmarks_homogeneous");
      else check(povar_get_landmarks(s.ctx, lms.data()), "povar_get_landmarks");
      for (int l = s.lb; l < s.le; ++l)
        for (int q = 0; q < w; ++q) {
          const double v = lms[(size_t)w * (l - s.lb) + q];
          if (homogeneous_) bal_problem_.landmarks()[l].p_w_homogeneous[q] = v;
          else bal_problem_.landmarks()[l].p_w[q] = v;
        }
    });
    for (int c = 0; c < nc; ++c)
      for (int q = 0; q < 12; ++q) bal_problem_.cameras()[c].space_matrix[q] = cams[12 * (size_t)c + q];
  }

 private:
  struct Shard {
    povar_ctx* ctx = nullptr;
    int32_t lb = 0, le = 0;  // its landmarks [lb, le)
    int64_t ob = 0, on = 0;  // its observations in file order: the first one and their number
  };
  struct Solved {  // what one shard's solve leaves
    VecX inc;
    int32_t iters, term;
  };
  template <class F>
  void all(F&& f) {
    team_.run([&](int r) { f(shards_[r], r); });
  }

  // The reference builds a new linearizor for step 2 (its constructor only allocates: sc/linearization_varproj.hpp:
  // 44-60); the device context -- observation layout, camera sets, row placement under way -- depends on the
  // observations and these options only, so the one step 1 left behind is taken over.
  void create_or_take_over(const povar_options& o) {
    Shard& s = shards_[0];
    s.le = bal_problem_.num_landmarks();
    s.on = bal_problem_.num_observations();
    cache_key_ = context_key(bal_problem_, o);
    if (bal_problem_.device_cache.ctx && bal_problem_.device_cache.key == cache_key_) {
      holder_ = std::move(bal_problem_.device_cache.ctx);
      bal_problem_.device_cache = BalProblem::DeviceCache();
      s.ctx = static_cast<povar_ctx*>(holder_.get());
    } else {
      bal_problem_.device_cache = BalProblem::DeviceCache();  // a context for something else: release it first
      std::vector<int> lm_off, cam_idx;
      std::vector<double> obs;
      bal_problem_.flatten(lm_off, cam_idx, obs);
      check(povar_create(&s.ctx, bal_problem_.num_cameras(), bal_problem_.num_landmarks(), (int64_t)cam_idx.size(),
                         lm_off.data(), cam_idx.data(), obs.data(), &o), "povar_create");
      holder_ = std::shared_ptr<void>(s.ctx, [](void* c) { povar_destroy(static_cast<povar_ctx*>(c)); });
    }
  }
  // every worker builds the context of its contiguous landmark range and joins the communicator
  void create_shards(const povar_options& o) {
    const int world = team_.size();
    std::vector<int> lm_off, cam_idx;
    std::vector<double> obs;
    bal_problem_.flatten(lm_off, cam_idx, obs);
    const int n_lms = bal_problem_.num_landmarks();
    const int n_dev = std::max(povar_device_count(), 1);
    const bool distinct = world <= n_dev;
    const char* force_host = std::getenv("POVAR_HOST_COMM");
    const bool use_rccl = distinct && !(force_host && force_host[0] == '1');
    uint8_t uid[128] = {0};
    if (use_rccl) check(povar_comm_unique_id(uid), "povar_comm_unique_id");
    std::fprintf(stderr, "[bal] shard team of %d on %d device(s): exchange: %s\n", world, n_dev, use_rccl ? "RCCL" : "host all-reduce");
    all([&](Shard& s, int r) {
      check(povar_shard_range(n_lms, lm_off.data(), world, r, &s.lb, &s.le), "povar_shard_range");
      std::vector<int> off(lm_off.begin() + s.lb, lm_off.begin() + s.le + 1);
      const int ob = off.front();
      for (int& v : off) v -= ob;
      s.ob = ob;
      s.on = off.back();
      povar_options or_ = o;
      or_.device = (o.device + r) % n_dev;
      check(povar_create(&s.ctx, bal_problem_.num_cameras(), s.le - s.lb, (int64_t)off.back(), off.data(), cam_idx.data() + ob,
                         obs.data() + 2 * (size_t)ob, &or_), "povar_create");
      if (use_rccl) check(povar_comm_init(s.ctx, world, r, uid), "povar_comm_init");
      else check(povar_comm_init_host(s.ctx, world, r, &ShardTeam::allreduce_hook, &team_.hook_args[r]), "povar_comm_init_host");
    });
  }

  void compute_error(bool step2, ResidualInfo& ri) {
    std::vector<povar_residual_info> r(shards_.size());
    all([&](Shard& s, int k) {
      if (step2) check(povar_error_homogeneous(s.ctx, &r[k]), "povar_error_homogeneous");
      else check(povar_error_pose(s.ctx, options_.alpha, &r[k]), "povar_error_pose");
    });
    ri = to_ri(r[0]);  // (all-reduced inside the library: the same on every rank)
    IF_SET(it_summary_)->residual_evaluation_time_in_seconds += device_seconds(4);
    IF_SET(summary_)->num_residual_evaluations += 1;
  }
  // the step's linearisation on every shard; books nothing
  void linearize_all(bool step2, double alpha, const char* what) {
    std::atomic<int> failed{0};
    all([&](Shard& s, int) {
      const int rc = step2 ? povar_linearize_homogeneous(s.ctx) : povar_linearize_pose(s.ctx, alpha);
      check(rc, what);
      if (rc == POVAR_NUMERIC_FAILURE) failed.store(1);
    });
    if (failed.load()) {
      std::fprintf(stderr, "FATAL: did not expect numerical failure during linearization\n");
      std::abort();
    }
  }
  void book_linearize() {
    const double e = device_seconds(0);
    IF_SET(it_summary_)->jacobian_evaluation_time_in_seconds = e;
    IF_SET(it_summary_)->stage1_time_in_seconds = e;
    IF_SET(summary_)->num_jacobian_evaluations += 1;
  }
  // call(shard) on every shard: the library's status, non-zero if any shard's is
  template <class F>
  int covariance_status(const char* what, F&& call) {
    std::atomic<int> status{0};
    all([&](Shard& s, int) {
      const int rc = call(s);
      check(rc, what);
      if (rc != 0) status.store(rc);
    });
    return status.load();
  }
  static int power_solver_type(const SolverOptions& so) {
    return so.solver_type_step_1 == SolverOptions::SolverType::POWER_SCHUR_COMPLEMENT ? POVAR_POWER_SCHUR_COMPLEMENT : POVAR_POWER_VARPROJ;
  }
  // rank 0's increment, its solve booked into the summaries (sc: with the messages of the explicit-SC solvers)
  VecX book_solve(Solved& s, bool sc, bool direct = false) {
    IF_SET(it_summary_)->prepare_time_in_seconds = device_seconds(1);
    if (sc) fill_sc_summary(device_seconds(2), s.iters, s.term, direct);
    else fill_solver_summary(device_seconds(2), s.iters, s.term);
    return std::move(s.inc);
  }
  template <class F>
  double apply_all(F&& call) {
    std::vector<double> l_diff(shards_.size(), 0.0);
    all([&](Shard& s, int k) { call(s, &l_diff[k]); });
    IF_SET(it_summary_)->back_substitution_time_in_seconds = device_seconds(3);
    return l_diff[0];
  }
  // seconds of device time rank 0's entry points of `kind` have taken since the previous call of this helper
  // (0 linearize, 1 prepare, 2 solve, 3 apply, 4 other)
  double device_seconds(int kind) {
    povar_timings_info t;
    check(povar_timings(shards_[0].ctx, &t), "povar_timings");
    const double now[5] = {t.linearize_ms, t.prepare_ms, t.solve_ms, t.apply_ms, t.other_ms};
    const double d = (now[kind] - seen_[kind]) * 1e-3;
    seen_[kind] = now[kind];
    return d;
  }
  void push_state() {
    const int nc = bal_problem_.num_cameras();
    const int w = homogeneous_ ? 4 : 3;
    std::vector<double> cams(12 * (size_t)nc);
    for (int c = 0; c < nc; ++c)
      for (int q = 0; q < 12; ++q) cams[12 * (size_t)c + q] = bal_problem_.cameras()[c].space_matrix[q];
    all([&](Shard& s, int) {
      check(povar_set_cameras(s.ctx, cams.data()), "povar_set_cameras");
      std::vector<double> lms((size_t)w * (s.le - s.lb));
      for (int l = s.lb; l < s.le; ++l)
        for (int q = 0; q < w; ++q)
          lms[(size_t)w * (l - s.lb) + q] = homogeneous_ ? bal_problem_.landmarks()[l].p_w_homogeneous[q] : bal_problem_.landmarks()[l].p_w[q];
      if (homogeneous_) check(povar_set_landmarks_homogeneous(s.ctx, lms.data()), "povar_set_landmarks_homogeneous");
      else check(povar_set_landmarks(s.ctx, lms.data()), "povar_set_landmarks");
    });
  }
  void fill_solver_summary(double seconds, int iters, int term) {
    IF_SET(it_summary_)->solve_reduced_system_time_in_seconds = seconds;
    IF_SET(it_summary_)->linear_solver_iterations = iters;
    // messages of linearization_power_varproj.hpp:213-235
    IF_SET(it_summary_)->linear_solver_message =
        term == POVAR_LINEAR_SOLVER_SUCCESS ? "Iteration: " + std::to_string(iters) + " Convergence."
                                            : "Maximum number of iterations reached.";
    IF_SET(it_summary_)->linear_solver_type = "bal_power_sc";
    IF_SET(summary_)->num_linear_solves += 1;
  }

  void require_schur_jacobi() const {  // CHECK of linearizor_sc.cpp:126-128, 268-270
    if (options_.preconditioner_type != SolverOptions::PreconditionerType::SCHUR_JACOBI) {
      std::fprintf(stderr, "FATAL: preconditioner_type: not implemented\n");
      std::abort();
    }
  }
  void fill_sc_summary(double seconds, int iters, int term, bool direct) {
    IF_SET(it_summary_)->solve_reduced_system_time_in_seconds = seconds;
    IF_SET(it_summary_)->linear_solver_iterations = iters;
    // messages of conjugate_gradient.hpp:114-301 (without the numbers they embed); solve_direct_pOSE
    // leaves the message empty (linearization_sc.hpp:239)
    IF_SET(it_summary_)->linear_solver_message =
        direct ? ""
        : term == POVAR_LINEAR_SOLVER_SUCCESS ? "Iteration: " + std::to_string(iters) + " Convergence."
        : term == POVAR_LINEAR_SOLVER_FAILURE ? "Numerical failure."
                                              : "Maximum number of iterations reached.";
    IF_SET(it_summary_)->linear_solver_type = "bal_sc";
    IF_SET(summary_)->num_linear_solves += 1;
  }

  SolverOptions options_;
  bool sc_step1_ = false, sc_step2_ = false;
  int32_t cov_gauge_ = POVAR_COV_FREE_GAUGE;
  BalProblem& bal_problem_;
  SolverSummary* summary_ = nullptr;
  IterationSummary* it_summary_ = nullptr;
  bool homogeneous_;
  bool sharded_;
  ShardTeam team_;
  std::vector<Shard> shards_;
  std::shared_ptr<void> holder_;  // not sharded: owns the context; handed to BalProblem::device_cache by the destructor
  std::string cache_key_;
  double seen_[5] = {0, 0, 0, 0, 0};
};

LinearizorFactory g_factory = nullptr;

// a linearizor that would ignore --fixed-cameras is not handed out
std::unique_ptr<Linearizor> fixed_cameras_checked(std::unique_ptr<Linearizor> lin, const SolverOptions& o) {
  if (!o.fixed_cameras.empty() && !lin->holds_fixed_cameras()) {
    std::fprintf(stderr, "FATAL: --fixed-cameras: this linearizor does not implement fixed cameras\n");
    std::abort();
  }
  return lin;
}

std::unique_ptr<Linearizor> make(BalProblem& p, const SolverOptions& o, SolverSummary* s, bool hom) {
  if (g_factory) return fixed_cameras_checked(g_factory(p, o, s, hom), o);
  // POVAR_FORCE_MULTI=1: also `--gpus 1` runs sharded (a team of one: an RCCL communicator of one rank created on the
  // worker thread, the all-reduces of the one shard inside its captured term loop with POVAR_GRAPH_COMM=1) -- the branch
  // a one-GPU box can otherwise never execute (tests/test_gpu_bal_cli.py)
  const char* force_multi = std::getenv("POVAR_FORCE_MULTI");
  const bool sharded = o.gpus > 1 || (force_multi && force_multi[0] == '1');
  return std::make_unique<LinearizorPowerVarprojHip>(p, o, s, hom, sharded);
}

}  // namespace

void set_linearizor_factory(LinearizorFactory f) { g_factory = f; }

std::unique_ptr<Linearizor> Linearizor::create(BalProblem& p, const SolverOptions& o, SolverSummary* s) {
  return make(p, o, s, false);  // solver/linearizor.cpp:47-62: every SolverType has a device implementation
}

std::unique_ptr<Linearizor> Linearizor::create_homogeneous(BalProblem& p, const SolverOptions& o, SolverSummary* s) {
  return make(p, o, s, true);  // solver/linearizor.cpp:64-80
}

}  // namespace povar_host
