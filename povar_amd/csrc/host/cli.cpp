// Flat CLI parser reproducing the reference's flag names: "--" + nested prefix + member name with
// '_' -> '-' (cli/cli_options.cpp:61, 134), booleans as --x / --no-x (cli_options.cpp:85-91), enums
// from strings (cli_options.cpp:102-111).  Prefixes: dataset and solver members have none, the
// nested solver.residual and solver.log structs use "residual-" and "log-".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <string>

#include "solver_options.hpp"

namespace povar_host {

const char* to_string(SolverOptions::SolverType t) {
  switch (t) {
    case SolverOptions::SolverType::PCG: return "PCG";
    case SolverOptions::SolverType::POWER_SCHUR_COMPLEMENT: return "POWER_SCHUR_COMPLEMENT";
    case SolverOptions::SolverType::POWER_VARPROJ: return "POWER_VARPROJ";
    default: return "CHOLESKY";
  }
}
const char* to_string(SolverOptions::SolverTypeRiemannian t) {
  switch (t) {
    case SolverOptions::SolverTypeRiemannian::RIPOBA: return "RIPOBA";
    case SolverOptions::SolverTypeRiemannian::RIPCG: return "RIPCG";
    default: return "RICHOLESKY";
  }
}

namespace {
template <class E>
bool parse_enum(const std::string& v, const std::map<std::string, E>& m, E& out) {
  auto it = m.find(v);
  if (it == m.end()) return false;
  out = it->second;
  return true;
}
}  // namespace

bool parse_bal_app_arguments(int argc, char** argv, BalAppOptions& o) {
  using S = SolverOptions;
  std::map<std::string, std::function<bool(const std::string&)>> val;
  std::map<std::string, bool*> flag;
  auto dbl = [&](const char* n, double* p) { val[n] = [p](const std::string& v) { char* e; *p = std::strtod(v.c_str(), &e); return *e == 0; }; };
  auto integer = [&](const char* n, int* p) { val[n] = [p](const std::string& v) { char* e; *p = (int)std::strtol(v.c_str(), &e, 10); return *e == 0; }; };
  auto str = [&](const char* n, std::string* p) { val[n] = [p](const std::string& v) { *p = v; return true; }; };
  str("input", &o.dataset.input);
  integer("random-seed", &o.dataset.random_seed);
  flag["create-dataset"] = &o.dataset.create_dataset;
  flag["quiet"] = &o.dataset.quiet;
  val["solver-type-step-1"] = [&](const std::string& v) {
    return parse_enum<S::SolverType>(v, {{"PCG", S::SolverType::PCG}, {"POWER_SCHUR_COMPLEMENT", S::SolverType::POWER_SCHUR_COMPLEMENT},
                                         {"POWER_VARPROJ", S::SolverType::POWER_VARPROJ}, {"CHOLESKY", S::SolverType::CHOLESKY}}, o.solver.solver_type_step_1); };
  val["solver-type-step-2"] = [&](const std::string& v) {
    return parse_enum<S::SolverTypeRiemannian>(v, {{"RIPOBA", S::SolverTypeRiemannian::RIPOBA}, {"RIPCG", S::SolverTypeRiemannian::RIPCG},
                                                   {"RICHOLESKY", S::SolverTypeRiemannian::RICHOLESKY}}, o.solver.solver_type_step_2); };
  val["optimized-cost"] = [&](const std::string& v) {
    return parse_enum<S::OptimizedCost>(v, {{"ERROR", S::OptimizedCost::ERROR}, {"ERROR_VALID", S::OptimizedCost::ERROR_VALID},
                                            {"ERROR_VALID_AVG", S::OptimizedCost::ERROR_VALID_AVG}}, o.solver.optimized_cost); };
  val["preconditioner-type"] = [&](const std::string& v) {
    return parse_enum<S::PreconditionerType>(v, {{"JACOBI", S::PreconditionerType::JACOBI}, {"SCHUR_JACOBI", S::PreconditionerType::SCHUR_JACOBI}}, o.solver.preconditioner_type); };
  val["residual-robust-norm"] = [&](const std::string& v) {
    using R = BalResidualOptions::RobustNorm;
    return parse_enum<R>(v, {{"NONE", R::NONE}, {"HUBER", R::HUBER}, {"CAUCHY", R::CAUCHY}}, o.solver.residual.robust_norm); };
  dbl("residual-huber-parameter", &o.solver.residual.huber_parameter);
  str("log-log-path", &o.solver.log.log_path);
  flag["log-disable-all"] = &o.solver.log.disable_all;
  integer("verbosity-level", &o.solver.verbosity_level);
  flag["debug"] = &o.solver.debug;
  integer("num-threads", &o.solver.num_threads);
  dbl("alpha", &o.solver.alpha);
  integer("max-num-iterations-step-1", &o.solver.max_num_iterations_step_1);
  integer("max-num-iterations-step-2", &o.solver.max_num_iterations_step_2);
  dbl("min-relative-decrease", &o.solver.min_relative_decrease);
  dbl("initial-trust-region-radius", &o.solver.initial_trust_region_radius);
  dbl("min-trust-region-radius", &o.solver.min_trust_region_radius);
  dbl("max-trust-region-radius", &o.solver.max_trust_region_radius);
  integer("min-linear-solver-iterations", &o.solver.min_linear_solver_iterations);
  integer("max-linear-solver-iterations", &o.solver.max_linear_solver_iterations);
  dbl("eta", &o.solver.eta);
  dbl("r-tolerance", &o.solver.r_tolerance);
  flag["jacobi-scaling"] = &o.solver.jacobi_scaling;
  dbl("jacobi-scaling-epsilon", &o.solver.jacobi_scaling_epsilon);
  dbl("function-tolerance", &o.solver.function_tolerance);
  integer("power-sc-iterations", &o.solver.power_sc_iterations);
  dbl("initial-vee", &o.solver.initial_vee);
  dbl("vee-factor", &o.solver.vee_factor);
  str("e0-mode", &o.solver.e0_mode);
  flag["deterministic"] = &o.solver.deterministic;
  flag["fp32-terms"] = &o.solver.fp32_terms;
  flag["compact-fixed-cameras"] = &o.solver.dense_compaction;
  integer("device", &o.solver.device);
  integer("gpus", &o.solver.gpus);
  str("camera-covariance-path", &o.solver.camera_covariance_path);
  str("landmark-covariance-path", &o.solver.landmark_covariance_path);
  str("observation-covariance-path", &o.solver.observation_covariance_path);
  str("observation-diagnostics-path", &o.solver.observation_diagnostics_path);
  dbl("observation-diagnostics-tol", &o.solver.observation_diagnostics_tol);
  str("covariance-pairs-path", &o.solver.covariance_pairs_path);
  str("covariance-blocks-path", &o.solver.covariance_blocks_path);
  // LIST: comma-separated tokens, each an id or a range a-b (a <= b); the ids are checked against the camera count once the
  // problem is loaded (bal.cpp)
  val["fixed-cameras"] = [&](const std::string& v) {
    std::vector<int>& ids = o.solver.fixed_cameras;
    ids.clear();
    size_t at = 0;
    while (at <= v.size()) {
      const size_t comma = std::min(v.find(',', at), v.size());
      const std::string tok = v.substr(at, comma - at);
      at = comma + 1;
      if (tok.empty() || tok[0] < '0' || tok[0] > '9') return false;
      char* e;
      const long a = std::strtol(tok.c_str(), &e, 10);
      long b = a;
      if (*e == '-') {
        const char* rest = e + 1;
        if (*rest < '0' || *rest > '9') return false;
        b = std::strtol(rest, &e, 10);
      }
      if (*e != 0 || b < a || b > 0x7fffffffL || b - a > (1L << 24)) return false;
      for (long k = a; k <= b; ++k) ids.push_back((int)k);
    }
    return true;
  };

  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    if (a == "-h" || a == "--help") {
      std::printf("usage: bal --input FILE [--create-dataset] [options]\n  value options:");
      for (auto& kv : val) std::printf(" --%s", kv.first.c_str());
      std::printf("\n  boolean options (--x / --no-x):");
      for (auto& kv : flag) std::printf(" --%s", kv.first.c_str());
      std::printf("\n  --solver-type-step-1 PCG | POWER_SCHUR_COMPLEMENT | POWER_VARPROJ | CHOLESKY\n"
                  "  --solver-type-step-2 RIPOBA | RIPCG | RICHOLESKY\n"
                  "      RICHOLESKY is not a value of the reference: the direct solve of the joint system (dense Cholesky on the\n"
                  "      device), the limit RIPOBA and RIPCG approach\n"
                  "  --camera-covariance-path FILE\n"
                  "      not an option of the reference: at the final accepted state of the last step that ran, the free-gauge marginal\n"
                  "      covariance (inverse information) of every camera: n_cams, then 144 numbers (12 x 12, row-major) per camera\n"
                  "  --landmark-covariance-path FILE\n"
                  "      likewise for every landmark (gauge fixed on the cameras): n_lms, then 9 numbers (3 x 3, after step 1) or 16\n"
                  "      (4 x 4 homogeneous, after step 2) per landmark; with --camera-covariance-path one call serves both files\n"
                  "  --observation-covariance-path FILE\n"
                  "      likewise for every observation, independent of the gauge: n_obs, then one line per observation in file order:\n"
                  "      landmark camera h c_uu c_uv c_vv -- the leverage h (redundancy number: 4 - h after step 1, 2 - h after step 2)\n"
                  "      and the 2 x 2 covariance of the predicted image point\n"
                  "  --observation-diagnostics-path FILE [--observation-diagnostics-tol 1e-8]\n"
                  "      likewise the outlier diagnostics of every observation: n_obs, then one line per observation in file order:\n"
                  "      landmark camera t rank, then the d weighted residuals r and the upper triangle of the d x d hat block P (d = 4\n"
                  "      after step 1, 2 after step 2).  t = r^T (I - P)^+ r is the decrease of the linearised cost when the observation\n"
                  "      is deleted and everything re-estimated (exact at a converged state), rank the number of eigenvalues of I - P\n"
                  "      above the tolerance: the local redundancy (an observation of a two-view track has one null direction)\n"
                  "  --covariance-pairs-path IN --covariance-blocks-path OUT\n"
                  "      likewise the covariance block of every pair of parameter blocks listed in IN (the number of pairs, then one\n"
                  "      line `c|l id c|l id` per pair: c a camera, l a landmark), gauge fixed on the cameras: OUT gets the number of\n"
                  "      pairs, then one line `rows cols` and the rows x cols numbers per pair (a camera 12 coordinates, a landmark 3\n"
                  "      after step 1, 4 after step 2); one device only\n"
                  "  --fixed-cameras LIST\n"
                  "      not an option of the reference: hold these cameras constant in every solve of both steps (comma-separated ids\n"
                  "      and ranges a-b, in file order); the covariance outputs above are then those of the gauge the fixed cameras\n"
                  "      define (zero blocks on them) instead of the free gauge.  One fixed camera does not fix the gauge\n"
                  "  --compact-fixed-cameras\n"
                  "      with --fixed-cameras: CHOLESKY / RICHOLESKY and the covariance outputs build their dense matrix over the free\n"
                  "      cameras only (same results; memory and factorisation scale with the free cameras).  No effect without it\n");
      return false;
    }
    if (a.rfind("--", 0) != 0) {
      std::fprintf(stderr, "unexpected argument '%s'\n", a.c_str());
      return false;
    }
    a = a.substr(2);
    std::string v;
    bool has_v = false;
    const size_t eq = a.find('=');
    if (eq != std::string::npos) { v = a.substr(eq + 1); a = a.substr(0, eq); has_v = true; }
    if (flag.count(a)) { *flag[a] = true; continue; }
    if (a.rfind("no-", 0) == 0 && flag.count(a.substr(3))) { *flag[a.substr(3)] = false; continue; }
    auto it = val.find(a);
    if (it == val.end()) { std::fprintf(stderr, "unknown option '--%s'\n", a.c_str()); return false; }
    if (!has_v) {
      if (i + 1 >= argc) { std::fprintf(stderr, "option '--%s' needs a value\n", a.c_str()); return false; }
      v = argv[++i];
    }
    if (!it->second(v)) { std::fprintf(stderr, "invalid value '%s' for '--%s'\n", v.c_str(), a.c_str()); return false; }
  }
  if (o.dataset.input.empty()) { std::fprintf(stderr, "missing --input\n"); return false; }
  if (o.solver.gpus > 1 && !o.solver.camera_covariance_path.empty()) {
    std::fprintf(stderr, "--gpus > 1 does not serve --camera-covariance-path (the dense factor is inverted on one device)\n");
    return false;
  }
  if (o.solver.covariance_pairs_path.empty() != o.solver.covariance_blocks_path.empty()) {
    std::fprintf(stderr, "--covariance-pairs-path and --covariance-blocks-path go together\n");
    return false;
  }
  if (o.solver.gpus > 1 && !o.solver.covariance_pairs_path.empty()) {
    std::fprintf(stderr, "--gpus > 1 does not serve --covariance-pairs-path (landmark ids would be those of a shard)\n");
    return false;
  }
  return true;
}

}  // namespace povar_host
