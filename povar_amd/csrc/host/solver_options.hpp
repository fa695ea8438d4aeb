// Option structs of the drop-in surface: same names and defaults as the reference
// (bal/solver_options.hpp:95-305, bal/bal_residual_options.hpp:53-62, bal/bal_dataset_options.hpp:49-94,
// bal/ba_log_options.hpp:46-56).  The reference's reflection/clipp/TOML option framework is out of
// scope; a flat parser reproduces the flag names (cli.cpp).
#pragma once
#include <string>
#include <vector>

namespace povar_host {

struct BalResidualOptions {
  enum class RobustNorm { NONE, HUBER, CAUCHY };
  RobustNorm robust_norm = RobustNorm::NONE;
  double huber_parameter = 1.0;
};

struct BaLogOptions {
  std::string log_path = "ba_log.json";
  bool disable_all = false;
};

struct SolverOptions {
  enum class SolverType { PCG, POWER_SCHUR_COMPLEMENT, POWER_VARPROJ, CHOLESKY };
  // RICHOLESKY: dense Cholesky of the joint reduced system on the device (povar_solve_joint_sc_method); not a reference value
  enum class SolverTypeRiemannian { RIPOBA, RIPCG, RICHOLESKY };
  enum class OptimizedCost { ERROR, ERROR_VALID, ERROR_VALID_AVG };
  enum class PreconditionerType { JACOBI, SCHUR_JACOBI };

  SolverType solver_type_step_1 = SolverType::POWER_VARPROJ;
  SolverTypeRiemannian solver_type_step_2 = SolverTypeRiemannian::RIPOBA;
  int verbosity_level = 2;
  bool debug = false;
  int num_threads = 0;
  BalResidualOptions residual;
  double alpha = 0.01;
  BaLogOptions log;
  OptimizedCost optimized_cost = OptimizedCost::ERROR;
  int max_num_iterations_step_1 = 50;
  int max_num_iterations_step_2 = 50;
  double min_relative_decrease = 0.0;
  double initial_trust_region_radius = 1e4;
  double min_trust_region_radius = 1e-32;
  double max_trust_region_radius = 1e16;
  int min_linear_solver_iterations = 0;    // bal/solver_options.hpp:196-200
  int max_linear_solver_iterations = 500;  // bal/solver_options.hpp:201-203
  double eta = 1e-2;
  double r_tolerance = -1.0;
  bool jacobi_scaling = true;
  double jacobi_scaling_epsilon = 0.0;
  PreconditionerType preconditioner_type = PreconditionerType::SCHUR_JACOBI;
  double function_tolerance = 1e-6;
  int power_sc_iterations = 10;
  double initial_vee = 2.0;
  double vee_factor = 2.0;
  // MI355X build: which E0 operator form the device uses (not a reference option)
  std::string e0_mode = "ldsacc";  // "ldsacc" (fastest), "implicit" (bit-reproducible), "tiles" (stored tiles)
  // bit-reproducible results run to run (povar_options.flags: POVAR_FLAG_DETERMINISTIC; 1.26 x the default term on venice-1778)
  bool deterministic = false;
  // step 1's power-series terms in single precision (povar_options.flags: POVAR_FLAG_FP32_TERMS; contract in include/povar_hip.h)
  bool fp32_terms = false;
  int device = 0;
  // landmark shards = device contexts of ONE process (BASELINE configs 4 / 5: "landmarks sharded across 8 x MI355X"):
  // shard r runs on device (device + r) mod device count; one exchange step per power-series term (RCCL, or an in-process
  // all-reduce when shards share a device)
  int gpus = 1;
  // not in the reference: after the last step that ran, at its final accepted state, linearise and write the free-gauge
  // marginal covariance of every camera in camera coordinates (povar_camera_covariance_pose / _joint): n_cams on the first
  // line, then 144 numbers (12 x 12 row-major, %.17g) per camera.  Empty: nothing is written.  One device only.
  std::string camera_covariance_path;
  // likewise the free-gauge marginal covariance of every landmark in landmark coordinates (povar_landmark_covariance_pose /
  // _joint): n_lms on the first line, then 9 (after step 1: 3 x 3) or 16 (after step 2: 4 x 4) numbers per landmark in file
  // order.  With camera_covariance_path one library call serves both files.  Served with --gpus N too: every shard writes its
  // own landmarks.
  std::string landmark_covariance_path;
  // leverage and predicted-point covariance of every observation (povar_observation_covariance_pose / _joint, free gauge):
  // n_obs on the first line, then one line per observation in file order: landmark camera h c_uu c_uv c_vv (%.17g).  A call
  // of its own, independent of the two paths above; served with --gpus N too: every shard writes its own observations.
  std::string observation_covariance_path;
  // residual, hat block and deletion statistic of every observation (povar_observation_hat_pose / _joint, free gauge): n_obs on
  // the first line, then one line per observation in file order: landmark camera t rank, then the raw row of the call (the d
  // weighted residuals and the upper triangle of the d x d block P_ii by rows, %.17g; d = 4 after step 1, 2 after step 2).
  // t = r^T (I - P_ii)^+ r and rank = rank(I - P_ii) come from the host's own eigen-decomposition of I - P_ii, eigenvalues above
  // observation_diagnostics_tol kept.  A call of its own, independent of the paths above; served with --gpus N as the
  // observation path is.
  std::string observation_diagnostics_path;
  double observation_diagnostics_tol = 1e-8;
  // covariance blocks of parameter pairs (povar_covariance_blocks_pose / _joint, free gauge, parameter coordinates).
  // covariance_pairs_path is read: the number of pairs, then one line `c|l id c|l id` per pair (c: a camera, l: a landmark, ids
  // in file order).  covariance_blocks_path is written: the number of pairs, then one line per pair: rows cols and the rows x cols
  // numbers row-major (%.17g); a camera has 12 coordinates, a landmark 3 (after step 1) or 4 (after step 2).  Both or neither;
  // one device only.
  std::string covariance_pairs_path, covariance_blocks_path;
  // not in the reference (Ceres: SetParameterBlockConstant): cameras held constant in every solve of both steps, ids in file
  // order (--fixed-cameras LIST: comma-separated ids and a-b ranges; povar_set_fixed_cameras on every shard context).  With
  // the set non-empty the covariance outputs above are those of POVAR_COV_FIXED_GAUGE -- [S_ff(0)]^-1, zero on the fixed
  // cameras -- and their files say so.  One fixed camera does not fix the gauge (include/povar_hip.h).
  std::vector<int> fixed_cameras;
  // --compact-fixed-cameras: the dense matrix of CHOLESKY / RICHOLESKY and the covariance outputs spans the free cameras only
  // (povar_set_dense_compaction(1) on every shard context): memory and factorisation follow the window, the outputs are the
  // same.  No effect without --fixed-cameras.
  bool dense_compaction = false;

  // solver_options.cpp:41-51
  bool use_projection_validity_check() const { return optimized_cost != OptimizedCost::ERROR; }
};

struct BalDatasetOptions {
  std::string input;
  bool create_dataset = false;
  int random_seed = 38401;
  bool quiet = false;
};

struct BalAppOptions {
  BalDatasetOptions dataset;
  SolverOptions solver;
};

// returns false (after printing a message) on a parse error or --help
bool parse_bal_app_arguments(int argc, char** argv, BalAppOptions& options);
const char* to_string(SolverOptions::SolverType t);
const char* to_string(SolverOptions::SolverTypeRiemannian t);

}  // namespace povar_host
