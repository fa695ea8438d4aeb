/*
 * povar_hip.h -- C ABI of the MI355X (gfx950) implementation of PoVar's power-series
 * Schur-complement inner solve.
 *
 * The reference (tum-vision/povar, C++17, CPU only) has no C ABI.  Its operator boundary for
 * this path is the abstract class Linearizor<Scalar> (src/rootba_povar/solver/linearizor.hpp:48-82)
 * as implemented by LinearizorPowerVarproj (solver/linearizor_power_varproj.cpp:21-308) on top
 * of LinearizationPowerVarproj (sc/linearization_power_varproj.hpp:28-469), and -- for the explicit
 * Schur-complement solver types PCG / CHOLESKY / RIPCG -- by LinearizorSC (solver/linearizor_sc.cpp:50-360)
 * on top of LinearizationSC (sc/linearization_sc.hpp).  Each entry point below names the reference
 * interface it replaces.  A reference-side binding (a Linearizor
 * subclass forwarding to these calls) is shown in INTEGRATION.md.
 *
 * Conventions: plain pointers and sizes, caller-allocated HOST buffers, fp64 values, int32
 * indices, row-major 3x4 camera matrices flattened to 12 (bal_problem.hpp:147-157).  Every
 * function returns an int status: 0 = ok, POVAR_NUMERIC_FAILURE (1) = non-finite values where
 * the reference would flag numerical failure, < 0 = HIP / RCCL / argument error (text via
 * povar_last_error()).  No exceptions cross the ABI.  A context is single-threaded, like the
 * reference Linearizor (not re-entrant: linearizor_base.hpp:80-86).
 */
#ifndef POVAR_HIP_H
#define POVAR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct povar_ctx povar_ctx;

#define POVAR_OK 0
#define POVAR_NUMERIC_FAILURE 1

/* BalResidualOptions::RobustNorm  (bal/bal_residual_options.hpp:45-49) */
enum { POVAR_NORM_NONE = 0, POVAR_NORM_HUBER = 1, POVAR_NORM_CAUCHY = 2 };
/* SolverOptions::SolverType values served by this path (bal/solver_options.hpp:60-66;
 * factory solver/linearizor.cpp:51-56) */
enum { POVAR_POWER_VARPROJ = 0, POVAR_POWER_SCHUR_COMPLEMENT = 1 };
/* LinearizationPowerVarproj::Summary::TerminationType (sc/linearization_power_varproj.hpp:52-56) */
enum { POVAR_LINEAR_SOLVER_NO_CONVERGENCE = 0, POVAR_LINEAR_SOLVER_SUCCESS = 1,
       POVAR_LINEAR_SOLVER_FAILURE = 2 };
/* how E0*x is evaluated: 0 = implicit (tiles recomputed from cameras/landmarks/observations,
 * deterministic two-pass scatter), 1 = stored tiles (the reference's [Jp|Jl] blocks kept in HBM
 * and streamed once per term, same deterministic scatter), 2 = implicit with the Jp^T s contributions
 * of the ~590 most observed cameras accumulated in LDS (fp64 LDS atomics: fastest, summation order
 * and therefore the last bits not reproducible run to run -- like the reference's mutex order),
 * 3 = stored tiles with the same LDS accumulation (Jp^T s taken from the stored Jp).  Step 2 has the
 * implicit forms only: modes 1 and 3 run its deterministic implicit path. */
enum { POVAR_E0_IMPLICIT = 0, POVAR_E0_TILES = 1, POVAR_E0_IMPLICIT_LDSACC = 2, POVAR_E0_TILES_LDSACC = 3 };

/* LandmarkBlockSC::Options (sc/landmark_block.hpp:61-75) + device selection */
typedef struct {
  int32_t robust_norm;       /* POVAR_NORM_* */
  double huber_parameter;    /* bal_residual_options.hpp:61-62 */
  double jacobi_scaling_eps; /* effective epsilon, linearizor_base.cpp:94-100 (1e-5 if option is 0) */
  int32_t device;            /* HIP device ordinal */
  int32_t e0_mode;           /* POVAR_E0_* */
  uint32_t flags;            /* POVAR_FLAG_* behaviour switches, 0 = the library's defaults (below) */
} povar_options;

/* povar_options.flags -- the behaviour switches of a context.  The reference passes every such switch through SolverOptions
 * (bal/solver_options.hpp:95-305); this is that struct's place for the MI355X build's own.  The POVAR_* environment variables
 * named beside them stay as OVERRIDES for diagnosis (a variable that is set wins over the flag). */
enum {
  /* run-to-run BIT-reproducible results for a given device count (fixed reduction order inside a GPU): the gather
   * mode for linearisation / preparation / cost, the fixed-point, ticket-ordered camera-chunk kernels for the terms (1.26 x the
   * default term on venice-1778), the ordered assembly of the dense reduced camera matrix (povar_set_sc_assembly: CHOLESKY,
   * RICHOLESKY and the covariance calls are covered like PCG / RIPCG and the power series), no row placement on a host thread,
   * no timing decides a kernel.  [POVAR_DETERMINISTIC=1] */
  POVAR_FLAG_DETERMINISTIC = 1u << 0,
  /* with POVAR_FLAG_DETERMINISTIC: the terms in the gather form too (3.7 x the default term).  [POVAR_DET_CK=0] */
  POVAR_FLAG_DET_GATHER_TERMS = 1u << 1,
  /* launch the term loop kernel by kernel instead of replaying a captured hipGraph.  [POVAR_NO_GRAPH=1] */
  POVAR_FLAG_NO_GRAPH = 1u << 2,
  /* bits 4..7: per-term E0 kernel, as povar_set_e0_kernel: POVAR_FLAG_E0_KERNEL(k), k = -1 (field 0: the library times the
   * kernels once per layout and keeps the faster), 0 = e0_lpl / e0_lpl_h, 1..6 = a camera-chunk instantiation.  [POVAR_E0_CK=k] */
  POVAR_FLAG_E0_KERNEL_SHIFT = 4, POVAR_FLAG_E0_KERNEL_MASK = 0xFu << 4,
  /* bits 8..9: the m-term loop, as povar_set_series_kernel: POVAR_FLAG_SERIES_KERNEL(m), m = -1 (field 0: timed), 0 = per-term
   * kernels, 1 = the resident launch wherever the context allows it; one switch for the series of both steps (solve_pOSE and
   * solve_joint).  [POVAR_RES=m] */
  POVAR_FLAG_SERIES_KERNEL_SHIFT = 8, POVAR_FLAG_SERIES_KERNEL_MASK = 0x3u << 8,
  /* bits 12..13: LDS bank placement of the lane-per-landmark rows: POVAR_FLAG_PLACEMENT(p), p = 0 (by size: inside povar_create
   * under 2^20 observations, on a host thread from there on), 1 = inside povar_create, 2 = on a host thread, 3 = none.
   * [POVAR_LPL_PLACE=sync|async|none] */
  POVAR_FLAG_PLACEMENT_SHIFT = 12, POVAR_FLAG_PLACEMENT_MASK = 0x3u << 12,
  /* keep the 16-byte image points in the camera-chunk rows even where they pack (six-decimal observations).  [POVAR_CK_PACK=0] */
  POVAR_FLAG_NO_PACKED_ROWS = 1u << 16,
  /* step 1's power-series terms (solve_pOSE under POVAR_POWER_VARPROJ and POVAR_POWER_SCHUR_COMPLEMENT, povar_power_series_step,
   * povar_right_mul_e0_pose) in single precision: the camera-chunk kernel e0_ck_f32 on a chunk layout povar_create always builds
   * for such a context, rows placed inside the call (as POVAR_FLAG_PLACEMENT(1)).  Numerical contract:
   *   fp32: the per-observation arithmetic of E0; the landmark records (h~ and G = S Hll^-1 S, rounded from fp64 by
   *         ck32_records) and slot values (h~, u = Jl^T Jp x, g = G u; u sums in LDS with ds_add_f32); the scalars sb^2, sa^2
   *         and the Huber threshold; the camera records a chunk gathers (Z = sigma_c x_c, P3 and, for HUBER, the translation); the image
   *         points -- packed rows as (float)k * 1e-6f, rows that do not pack stored as float2; HUBER weights recomputed per
   *         observation in fp32 (CAUCHY's are 1); a chunk's own sum (<= 16 observations of one camera);
   *   fp64: every sum across chunks of a camera (the segmented wavefront sum, the LDS accumulators, the partial records, the
   *         cold view, the per-camera sums), B^-1 -- stored and applied in fp64 --, the running sum x and the z handed from one
   *         term to the next (converted to fp32 where a chunk gathers it), the exchange of a sharded context.
   * Everything else -- linearisation, b, back substitution, cost, step 2, the explicit-SC solvers -- is the fp64 path.  Not
   * bit-reproducible: the LDS adds land in arrival order, as in the default mode.  povar_create fails with
   * POVAR_FLAG_DETERMINISTIC, POVAR_FLAG_SERIES_KERNEL(1), POVAR_FLAG_E0_KERNEL(0) or an e0_mode other than
   * POVAR_E0_IMPLICIT_LDSACC, and where the chunk layout cannot be built; povar_set_e0_kernel(ctx, 0),
   * povar_set_series_kernel(ctx, 1) and povar_set_e0_mode to another mode fail on such a context.  [POVAR_FP32_TERMS=1|0] */
  POVAR_FLAG_FP32_TERMS = 1u << 17
};
#define POVAR_FLAG_E0_KERNEL(k) ((((uint32_t)((k) + 1)) & 0xFu) << POVAR_FLAG_E0_KERNEL_SHIFT)
#define POVAR_FLAG_SERIES_KERNEL(m) ((((uint32_t)((m) + 1)) & 0x3u) << POVAR_FLAG_SERIES_KERNEL_SHIFT)
#define POVAR_FLAG_PLACEMENT(p) ((((uint32_t)(p)) & 0x3u) << POVAR_FLAG_PLACEMENT_SHIFT)

/* ResidualInfo (bal/residual_info.hpp:59-92) */
typedef struct {
  int64_t all_num_obs;
  double all_error;
  double all_residual_sum;
  int64_t valid_num_obs;
  double valid_error;
  double valid_residual_sum;
  int32_t is_numerically_valid;
} povar_residual_info;

/* per-kernel-class device time measured with HIP events on the context's stream */
typedef struct {
  double e0_ms;      /* sum over launches of the E0 (SpMV) kernels of one term; a dense call (CHOLESKY, RICHOLESKY, covariance)
                        adds one interval: the launches that assemble its matrix */
  int64_t e0_launches;
  double binv_ms;    /* B^-1 / AXPY kernel */
  int64_t binv_launches;
  double comm_ms;    /* RCCL all-reduce */
  int64_t comm_launches;
} povar_profile_info;

const char* povar_last_error(void);
/* number of visible HIP devices (0 without a GPU; < 0 on a runtime error) */
int povar_device_count(void);
/* compute units of a device (hipDeviceProp_t::multiProcessorCount; < 0 on a runtime error).  A launcher that puts several
 * ranks on ONE device gives each a range of them (environment POVAR_CU_MASK=<first>-<last>, read by povar_create). */
int povar_device_cu_count(int32_t device);

/* LinearizorPowerVarproj ctor (linearizor_power_varproj.cpp:21-38) + LinearizationVarProj ctor /
 * allocate_landmark (linearization_varproj.hpp:42-61, landmark_block.hpp:101-133).
 * lm_offsets[n_lms+1] CSR over observations, cam_idx ascending inside a landmark (std::map
 * order, bal_problem.hpp:226), obs = (u, v) with v already negated (bal_problem.cpp:240).
 * With povar_comm_init() the arrays describe this rank's landmark shard only. */
int povar_create(povar_ctx** out, int32_t n_cams, int32_t n_lms, int64_t n_obs,
                 const int32_t* lm_offsets, const int32_t* cam_idx, const double* obs,
                 const povar_options* options);
void povar_destroy(povar_ctx* ctx);

/* BalProblem state shared with the caller (linearizor_base.hpp:80; bal_problem.hpp:290-294) */
int povar_set_cameras(povar_ctx* ctx, const double* cams /*12 n_cams*/);
int povar_get_cameras(povar_ctx* ctx, double* cams);
int povar_set_landmarks(povar_ctx* ctx, const double* lms /*3 n_lms*/);
int povar_get_landmarks(povar_ctx* ctx, double* lms);
/* BalProblem::backup_pOSE / restore_pOSE (bal_problem.cpp:670-677, 701-708) */
int povar_backup_pose(povar_ctx* ctx);
int povar_restore_pose(povar_ctx* ctx);

/* Linearizor::initialize_varproj_lm_pOSE (linearizor_base.cpp:60-67; helper.cpp:76-114) */
int povar_init_landmarks_pose(povar_ctx* ctx, double alpha);
/* Linearizor::compute_error_pOSE (linearizor_base.cpp:69-77; helper.cpp:117-154) */
int povar_error_pose(povar_ctx* ctx, double alpha, povar_residual_info* out);
/* Linearizor::linearize_pOSE (linearizor_power_varproj.cpp:45-76) */
int povar_linearize_pose(povar_ctx* ctx, double alpha);
/* Linearizor::solve (linearizor_power_varproj.cpp:178-243): scale_Jp_cols on a new
 * linearisation point, prepare_Hb_pOSE[_poBA], solve_pOSE.  inc[12 n_cams] in scaled
 * coordinates; *num_iterations / *termination as Summary (linearization_power_varproj.hpp:51-61).
 * q_tolerance = SolverOptions::eta, r_tolerance = SolverOptions::r_tolerance. */
int povar_solve_pose(povar_ctx* ctx, double lambda, int32_t solver_type, int32_t power_sc_iterations,
                     double q_tolerance, double r_tolerance, double* inc, int32_t* num_iterations,
                     int32_t* termination);
/* Linearizor::apply (linearizor_power_varproj.cpp:246-273): camera update + back substitution;
 * *l_diff = model cost change. */
int povar_apply_pose(povar_ctx* ctx, int32_t solver_type, double alpha, const double* inc,
                     double* l_diff);

/* ---- the two halves of povar_solve_pose, separately (bench / parity tests) ---- */
/* LinearizationPowerVarproj::prepare_Hb_pOSE / _poBA (linearization_power_varproj.hpp:124-188) */
int povar_prepare_pose(povar_ctx* ctx, double lambda, int32_t solver_type);
/* LinearizationPowerVarproj::solve_pOSE (linearization_power_varproj.hpp:191-237); asynchronous
 * when both tolerances are <= 0 (result stays on the device; see povar_get_increment). */
int povar_power_series_pose(povar_ctx* ctx, int32_t power_sc_iterations, double q_tolerance,
                            double r_tolerance, int32_t* num_iterations, int32_t* termination);
int povar_get_increment(povar_ctx* ctx, double* inc /*12 n_cams*/);
/* term-by-term access: begin = accum = tmp = B^-1(-b) (hpp:196-200), step = one pass of the loop
 * body (hpp:202-203); get_term copies the current term. */
int povar_power_series_begin(povar_ctx* ctx);
int povar_power_series_step(povar_ctx* ctx);
int povar_get_term(povar_ctx* ctx, double* term /*12 n_cams*/);
/* LinearizationPowerVarproj::right_mul_e0_pOSE (linearization_power_varproj.hpp:364-406) */
int povar_right_mul_e0_pose(povar_ctx* ctx, const double* x, double* y);
int povar_set_e0_mode(povar_ctx* ctx, int32_t e0_mode);
int povar_synchronize(povar_ctx* ctx);

/* ---- step 2: projective refinement on the Riemannian manifold (RIPOBA) ---- */
/* BalProblem::Landmark::p_w_homogeneous (bal_problem.hpp:225), 4 n_lms; shares storage with p_w */
int povar_set_landmarks_homogeneous(povar_ctx* ctx, const double* lms_h);
int povar_get_landmarks_homogeneous(povar_ctx* ctx, double* lms_h);
/* BalProblem::backup_joint / restore_joint (bal_problem.cpp:658-665, 691-698) */
int povar_backup_joint(povar_ctx* ctx);
int povar_restore_joint(povar_ctx* ctx);
/* Linearizor::compute_error_homogeneous (linearizor_base.cpp:79-87; helper.cpp:157-196) */
int povar_error_homogeneous(povar_ctx* ctx, povar_residual_info* out);
/* Linearizor::linearize_projective_space_homogeneous (linearizor_power_varproj.cpp:80-110) */
int povar_linearize_homogeneous(povar_ctx* ctx);
/* LinearizationPowerVarproj::prepare_Hb_joint (linearization_power_varproj.hpp:74-122) incl. the
 * scale_Jp_cols_joint + linearize_nullspace of a new linearisation point (cpp:129-133) */
int povar_prepare_joint(povar_ctx* ctx, double lambda);
/* Linearizor::solve_joint (linearizor_power_varproj.cpp:114-175); inc[11 n_cams] in tangent
 * coordinates of the Householder bases N_c (see povar_get_buffer POVAR_BUF_NC_HOUSEHOLDER) */
int povar_solve_joint(povar_ctx* ctx, double lambda, int32_t power_sc_iterations, double q_tolerance,
                      double r_tolerance, double* inc, int32_t* num_iterations, int32_t* termination);
/* Linearizor::apply_joint (linearizor_power_varproj.cpp:277-308) */
int povar_apply_joint(povar_ctx* ctx, const double* inc, double* l_diff);
/* the renormalisation the outer loop performs after apply_joint (bal_bundle_adjustment.cpp:700-705) */
int povar_normalize_joint(povar_ctx* ctx);
/* povar_power_series_pose / _begin / _step / povar_get_term / povar_get_increment act on the system
 * prepared last (povar_prepare_pose: 12 n_cams vectors, povar_prepare_joint: 11 n_cams vectors) */

/* ---- constant cameras (Ceres: SetParameterBlockConstant; the reference has no counterpart).  A context carries a set F of
 * fixed cameras, whole cameras only, empty by default.  With F non-empty every solve -- the power series of both steps in every
 * kernel family, PCG / RIPCG, CHOLESKY / RICHOLESKY -- returns the increment of the system restricted to the free cameras,
 * S_ff x_f = -b_f, with the entries of the cameras in F exactly +0.0 or -0.0.  S, b and the landmark elimination are unchanged:
 * fixed cameras still observe and enter Hpp, E0, the cost, the back substitution and l_diff as constants.  povar_apply_pose /
 * povar_apply_joint with such an increment leave the 12 numbers of a fixed camera bitwise unchanged (but for the sign of an
 * entry that is -0.0, which adding +0.0 turns into +0.0); povar_normalize_joint
 * still rescales every camera to unit norm, fixed ones included (the same projective camera).  With F empty every call is bit
 * for bit what it is without this call.
 *   cam_ids: n_ids global camera ids, duplicates allowed; n_ids = 0 or a null pointer clears the set.  An id out of range is an
 * argument error that leaves the set as it was.  The set takes effect at the next call that prepares a system (povar_prepare_*,
 * povar_solve_*, a covariance call); a system prepared earlier is what it was.  The linearisation stays.  On a sharded context
 * every rank passes the same set.
 *   What the inspection buffers show on F: POVAR_BUF_B_INV[_JOINT] and POVAR_BUF_SC_PRECOND zero blocks; POVAR_BUF_SC_BLOCKDIAG
 * is unchanged; POVAR_BUF_SC_FACTOR identity rows and columns with y = x = 0. */
int povar_set_fixed_cameras(povar_ctx* ctx, const int32_t* cam_ids, int32_t n_ids);
/* the number of fixed cameras (the set as the last povar_set_fixed_cameras left it); flags: n_cams entries 0 / 1, or null */
int povar_fixed_cameras(povar_ctx* ctx, int32_t* flags /* n_cams or NULL */);

/* ---- compacted dense system (opt-in).  The dense matrix of every dense call -- CHOLESKY / RICHOLESKY and the camera, landmark,
 * observation, hat and pair covariance calls of both steps -- spans
 *   mode 0 (default): all cameras, the fixed ones as identity rows: n = dim n_cams rows, camera c at row dim c (today's layout);
 *   mode 1:           the free cameras only, in ascending camera id: A = S_ff (or S_ff(lambda)), n = dim (n_cams - |F|) rows.
 * The mode takes effect, like the fixed set, at the next call that prepares a system.  An unknown mode is an argument error.  On
 * a sharded context every rank passes the same mode.  PCG / RIPCG and the power series do not read it.
 *   Solves in mode 1: the increment keeps the fixed-camera contract -- the entries on F are exactly +0.0, the free entries solve
 * S_ff x_f = -b_f from the compact factor; num_iterations, termination and the not-positive-definite rule are unchanged.
 *   Covariance in mode 1: the outputs are those of the fixed-set rules, [S_ff(0)]^-1 or [S_ff(lambda)]^-1 zero-padded on F,
 * computed from the compact W and C (a block with a camera of F is exactly zero); the rules of gauge, coords and lambda are
 * unchanged; the pivot rule is applied to all rows of the compact matrix.
 *   Inspection buffers in mode 1: POVAR_BUF_SC_FACTOR, POVAR_BUF_COV_FACTOR, _INVERSE and _PANEL have N = the n of
 * povar_dense_layout rounded up to 64, with the padding rows as documented there; no identity rows stand for fixed cameras: a
 * camera is found through cam_row.  POVAR_BUF_COV_GAUGE (free gauge: F is empty), POVAR_BUF_SC_BLOCKDIAG and _PRECOND are as in
 * mode 0.
 *   F empty in mode 1: every call is bit for bit what it is in mode 0, and the map is dim c.
 *   Every camera fixed in mode 1 (n = 0): no matrix is allocated and no factorisation is launched.  A solve returns all +0.0
 * with status 0 and POVAR_LINEAR_SOLVER_SUCCESS; a covariance call returns the status mode 0 returns for the same request, camera
 * blocks exactly zero and the landmark, observation, hat and pair outputs of mode 0 (the same kernels on the same nonzero
 * operands); POVAR_BUF_SC_FACTOR and POVAR_BUF_COV_* are argument errors afterwards.
 *   Memory: the dense matrix, the padded solution, the covariance panel, the kept factor of povar_set_cov_inspect and the
 * all-reduce of a sharded context are sized by n; the out-of-memory message names the rows asked for. */
int povar_set_dense_compaction(povar_ctx* ctx, int32_t mode);
int povar_dense_compaction(povar_ctx* ctx);            /* the mode as last set; < 0 on error */
/* Layout of the dense matrix the last dense call built: returns its row count n (0: none yet, or no camera in it; < 0 on error).
 * cam_row: NULL, or n_cams entries: first row of camera c in that matrix, -1 for a camera that is not in it. */
int povar_dense_layout(povar_ctx* ctx, int32_t* cam_row /* n_cams or NULL */);

/* ---- explicit-Schur-complement solvers: LinearizorSC (solver/linearizor_sc.cpp), selected by
 * --solver-type-step-1 PCG | CHOLESKY and --solver-type-step-2 RIPCG (solver/linearizor.cpp:51-53,
 * 67-72), and --solver-type-step-2 RICHOLESKY (not in the reference).  The reduced camera system S x = b, S = (Hpp + lambda I) - E0, is solved without landmark
 * damping in step 1 (linearizor_sc.cpp:85-160) and with it in step 2 (:224-303); linearisation,
 * error evaluation and apply are the calls above (povar_apply_pose with POVAR_POWER_VARPROJ ==
 * LinearizorSC::apply, linearizor_sc.cpp:65-83). ---- */
enum { POVAR_SC_PCG = 0, POVAR_SC_CHOLESKY = 1 };
/* LinearizorPowerVarproj::linearize_pOSE scales the Jl columns (linearizor_power_varproj.cpp:62-64 ->
 * landmark_block.hpp:284-295), LinearizorSC::linearize_pOSE does not (linearizor_sc.cpp:163-191); the
 * stored Jl enters l_diff of apply (landmark_block.hpp:703-704).  enable = 1 (default) / 0 takes effect
 * at the next povar_linearize_pose.  Step 2 scales in both linearizors. */
int povar_set_jl_col_scaling(povar_ctx* ctx, int32_t enable);
/* LinearizorSC::solve (linearizor_sc.cpp:85-160).  POVAR_SC_PCG: ConjugateGradientsSolver::solve
 * (cg/conjugate_gradient.hpp:112-290) as driven by LinearizorBase::pcg (linearizor_base.cpp:104-125:
 * min/max_linear_solver_iterations, q_tolerance = eta, r_tolerance = -1, result negated) with the
 * SCHUR_JACOBI preconditioner (cg/preconditioner.hpp:66-135); S is applied matrix-free with the
 * per-term E0 kernels.  POVAR_SC_CHOLESKY: solve_direct_pOSE (sc/linearization_sc.hpp:236-245), dense
 * Cholesky of S on the device (needs 8 * (12 n_cams)^2 bytes of HBM; num_iterations = 0).
 * termination = POVAR_LINEAR_SOLVER_*. */
int povar_solve_pose_sc(povar_ctx* ctx, double lambda, int32_t method, int32_t min_iterations,
                        int32_t max_iterations, double eta, double* inc, int32_t* num_iterations,
                        int32_t* termination);
/* LinearizorSC::solve_joint (linearizor_sc.cpp:224-303): PCG (conjugate_gradient.hpp:292-470) on the
 * 11 n_cams tangent system */
int povar_solve_joint_sc(povar_ctx* ctx, double lambda, int32_t min_iterations, int32_t max_iterations,
                         double eta, double* inc, int32_t* num_iterations, int32_t* termination);
/* The same with the solver named, as povar_solve_pose_sc (povar_solve_joint_sc forwards with POVAR_SC_PCG).
 * POVAR_SC_CHOLESKY: direct solve of the joint system -- the dense S = (N_c^T sigma Hpp sigma N_c + lambda I) -
 * N_c^T sigma E0 sigma N_c of the 11 n_cams tangent coordinates is assembled on the device (landmark damping
 * included, as povar_prepare_joint leaves it) and factored by the kernels of CHOLESKY (needs 8 * (11 n_cams)^2 bytes
 * of HBM; num_iterations = 0; min / max_iterations and eta are not read).  The reference has no direct step-2
 * solver: this is `bal --solver-type-step-2 RICHOLESKY`, the limit RIPOBA and RIPCG approach.  The default assembly
 * adds with fp64 atomics, so it is not bit-reproducible (as step 1's); the ordered assembly is (povar_set_sc_assembly; what a
 * POVAR_FLAG_DETERMINISTIC context runs), and everything after the assembly is fixed-order in both.  A system that is not positive definite gives a
 * non-finite increment and POVAR_NUMERIC_FAILURE; an unknown method is an argument error. */
int povar_solve_joint_sc_method(povar_ctx* ctx, double lambda, int32_t method, int32_t min_iterations,
                                int32_t max_iterations, double eta, double* inc /*11 n_cams*/,
                                int32_t* num_iterations, int32_t* termination);
/* right_mul_e0_joint (sc/linearization_power_varproj.hpp:408-453) in tangent coordinates:
 * y = N_c^T sigma E0 sigma N_c x on the joint system prepared last (povar_prepare_joint, or any step-2 solve), with the
 * per-term E0 kernels the series and RIPCG use; x, y: 11 n_cams.  An error when the system prepared last is step 1's. */
int povar_right_mul_e0_joint(povar_ctx* ctx, const double* x, double* y);

/* ---- marginal covariance of the cameras.  The reference has no counterpart (it reports no uncertainty; Ceres answers the
 * same question with ceres::Covariance).  Both calls return, per camera, the diagonal block of the inverse of the reduced
 * camera system of their step, computed from the dense factor of CHOLESKY / RICHOLESKY (S = R^T R on the device, W = R^-1 in
 * place on the fp64 matrix cores, block_c = sum_k W[J_c, k] W[J_c, k]^T; needs the memory of those solvers plus a 64-column
 * panel).  The blocks are the inverse INFORMATION of the linearised problem in the library's residual units: the caller
 * multiplies by their own noise variance.
 *   gauge  POVAR_COV_FREE_GAUGE: lambda must be 0.  The blocks of the pseudo-inverse S(0)^+ of the undamped system, i.e. the
 *          free-gauge, minimum-norm covariance, as (S0 + Q Q^T)^-1 - Q Q^T with Q an orthonormal basis of the gauge null space
 *          of S0, built on the host in closed form from the linearisation point: step 1 the 12-dimensional affine gauge
 *          X -> A X that keeps the last homogeneous coordinate (per camera vec(-P_c G) / sigma_c, G = e_i e_j^T, i < 3),
 *          step 2 the 15-dimensional projective gauge (G = e_i e_j^T, (i, j) != (3, 3), the camera's own scale absorbed,
 *          projected on the tangent space N_c).  A system that is singular beyond its gauge is reported: after the
 *          factorisation of A = S0 + Q Q^T the smallest pivot R_kk^2 is compared with sqrt(u) max_k A_kk, u = 2^-53.
 *          POVAR_COV_DAMPED: lambda > 0.  The blocks of S(lambda)^-1 for exactly the matrix CHOLESKY / RICHOLESKY assemble at
 *          that lambda (step 1 without landmark damping, step 2 with it, as povar_prepare_joint leaves it); positive
 *          definiteness by CHOLESKY's own rule.
 *   coords POVAR_COV_SOLVER_COORDS: the solver's Jacobi-scaled coordinates, dim x dim row-major with dim = 12 (pose) or 11
 *          (joint: tangent coordinates of N_c), at stride 144 per camera -- the layout of POVAR_BUF_SC_BLOCKDIAG; the rest of
 *          the 144 is zero.  POVAR_COV_CAMERA_COORDS: always 12 x 12, the block T carried through the map that
 *          povar_apply_pose / povar_apply_joint apply to an increment: D T D with D = diag(sigma_c) (pose), D N_c T N_c^T D
 *          (joint; rank 11: the direction of P_c itself is not a degree of freedom).
 * Every block is symmetric bit for bit.  cov: 144 n_cams doubles.
 * Precondition: the step's linearisation is in force (povar_linearize_pose / povar_linearize_homogeneous); otherwise, for
 * an unknown enum value and for a lambda the mode does not take, an argument error (< 0).  The call prepares the system itself
 * (as povar_solve_pose_sc / povar_solve_joint_sc_method do): the system prepared before, the inspection buffers of the
 * explicit-SC solvers and the increment buffer are overwritten.  Not positive definite, or singular (free gauge): every entry of
 * cov is NaN and the call returns POVAR_NUMERIC_FAILURE.  Not enough device memory: the error of CHOLESKY / RICHOLESKY.
 * On a sharded context every rank calls; the assembly is all-reduced and every rank inverts the same matrix.
 *   With fixed cameras (povar_set_fixed_cameras, set F) every covariance call -- camera, landmark, observation, hat and pair,
 * both steps, both coords -- returns C with zero rows and columns on F:
 *          POVAR_COV_FIXED_GAUGE: lambda must be 0 and F non-empty (both violations are argument errors).  The blocks of
 *          [S_ff(0)]^-1, the covariance in the gauge the fixed cameras define, zero-padded on F.  No gauge basis is built
 *          (POVAR_BUF_COV_GAUGE is an argument error afterwards, as after POVAR_COV_DAMPED).  Singularity beyond what F fixes is
 *          reported by the pivot rule above, applied to the rows of the free cameras: NaN and POVAR_NUMERIC_FAILURE.  ONE fixed
 *          camera is not enough: it leaves a 4-dimensional null space in step 2 at a generic state, and in step 1 at an affine
 *          state (third camera row (0, 0, 0, 1), as the pOSE start state has it).  Two or more fix the gauge in both steps.
 *          POVAR_COV_DAMPED with F non-empty: the blocks of [S_ff(lambda)]^-1, zero-padded.
 *          POVAR_COV_FREE_GAUGE with F non-empty is an argument error.
 * A landmark's block contracts its free cameras only; a pair block with a fixed camera on either side is zero. ---- */
enum { POVAR_COV_FREE_GAUGE = 0, POVAR_COV_DAMPED = 1, POVAR_COV_FIXED_GAUGE = 2 };
enum { POVAR_COV_CAMERA_COORDS = 0, POVAR_COV_SOLVER_COORDS = 1 };
/* after povar_linearize_pose: the 12 n_cams system of step 1 */
int povar_camera_covariance_pose(povar_ctx* ctx, double lambda, int32_t gauge, int32_t coords, double* cov /*144 n_cams*/);
/* after povar_linearize_homogeneous: the 11 n_cams tangent system of step 2 */
int povar_camera_covariance_joint(povar_ctx* ctx, double lambda, int32_t gauge, int32_t coords, double* cov /*144 n_cams*/);

/* ---- marginal covariance of the landmarks: the other half of the question (ceres::Covariance serves both).  With
 * H = [[Hpp + lambda I, Hpl], [Hlp, Hll + lambda_l I]] in the solver's Jacobi-scaled coordinates (lambda_l = 0 in step 1, the
 * system CHOLESKY assembles; lambda_l = lambda in step 2, as povar_prepare_joint leaves the tangent Hll^-1), C the camera
 * covariance the calls above take blocks of and F_l = Hpl[:, l] Hll_l^-1, the block of landmark l is
 *       Sigma_l = Hll_l^-1 + F_l^T C F_l.
 * From the same factor: W = R^-1 as above, then C = W W^T off the diagonal too (a third n^3 / 3 pass on the fp64 matrix
 * cores, in place: no further n^2 buffer) and one workgroup per requested landmark that contracts the blocks C[c_i, c_j] of
 * its camera pairs.  Given C a block is reproducible: the contraction uses no atomics (the default assembly
 * of S does; with the ordered assembly -- povar_set_sc_assembly, POVAR_FLAG_DETERMINISTIC -- C and the blocks are bit-reproducible).
 *   gauge  POVAR_COV_DAMPED: C = S(lambda)^-1 and Sigma_l is exactly the (l, l) block of H^-1.
 *          POVAR_COV_FREE_GAUGE (lambda = 0): C = S(0)^+.  This is the covariance with the gauge fixed on the cameras: minimum
 *          norm over the camera parameters, i.e. under the constraint Q^T x_cameras = 0 -- the gauge the camera call fixes,
 *          so the two calls describe one consistent joint covariance.  It is NOT the landmark block of the pseudo-inverse
 *          of the full H (minimum norm over cameras and landmarks together), which differs from it at order one.
 *          Same lambda rules, pivot rule and errors as the camera calls.
 *   coords POVAR_COV_SOLVER_COORDS: the 3 x 3 block in the scaled coordinates (step 2: the tangent coordinates of N_l) in
 *          the first 9 numbers of the landmark's stride, the rest zero.  POVAR_COV_LANDMARK_COORDS: the block carried through
 *          the map back-substitution applies to a landmark increment: pose: D Sigma D, D = diag(s_l) the Jl column scale
 *          (ones with povar_set_jl_col_scaling(0)), 3 x 3; joint: the 4 x 4 D4 N_l Sigma N_l^T D4 with N_l the reflector
 *          basis of X_l (rank 3, null vector X_l / s_l).
 *   lm_ids indices into the context's own landmarks (on a sharded context: of the rank's shard), n_ids of them, duplicates
 *          allowed, an id out of range is an argument error; NULL: every landmark of the context in order (n_ids ignored).
 *   lm_cov row-major blocks at stride 9 (pose) or 16 (joint) per requested landmark, symmetric bit for bit.
 *   cam_cov NULL, or 144 n_cams doubles: the camera blocks of the same call in the same coords, as the camera calls return
 *          them (one factorisation and one inversion serve both); n_ids = 0 with cam_cov given is allowed.
 * Preconditions, side effects (POVAR_BUF_SC_FACTOR is an argument error afterwards), the sharded rule and the failure modes
 * are those of the camera calls; on POVAR_NUMERIC_FAILURE every entry of lm_cov and cam_cov is NaN. ---- */
enum { POVAR_COV_LANDMARK_COORDS = 0 }; /* = POVAR_COV_CAMERA_COORDS: the parameter's own coordinates */
/* after povar_linearize_pose: 3 x 3 per landmark, row-major at stride 9 */
int povar_landmark_covariance_pose(povar_ctx* ctx, double lambda, int32_t gauge, int32_t coords,
                                   const int32_t* lm_ids /* NULL = all landmarks of the context */, int32_t n_ids,
                                   double* lm_cov, double* cam_cov /* 144 n_cams or NULL */);
/* after povar_linearize_homogeneous: stride 16 per landmark */
int povar_landmark_covariance_joint(povar_ctx* ctx, double lambda, int32_t gauge, int32_t coords,
                                    const int32_t* lm_ids /* NULL = all landmarks of the context */, int32_t n_ids,
                                    double* lm_cov, double* cam_cov /* 144 n_cams or NULL */);

/* ---- per-observation leverage and covariance of the predicted image point: the block of the hat matrix J H^+ J^T of every
 * observation of the requested landmarks, J = [Jp Jl] the weighted Jacobian of the step (d = 4 residual rows per observation in
 * step 1, d = 2 in step 2).  With y = P_c X_l the projected homogeneous point, Syy_i the 3 x 3 covariance of y that the joint
 * covariance of camera c_i and landmark l implies (the camera-landmark cross terms included, which neither call above
 * exposes), each observation gets one row of 4 doubles
 *       (h, c_uu, c_uv, c_vv):   h = tr(J_i H^+ J_i^T), the leverage in the weighted residual metric the step minimises
 *                                (d - h is the redundancy number of the observation; 0 <= h <= d);
 *                                [[c_uu, c_uv], [c_uv, c_vv]] the covariance of the predicted image point (y0 / y2, y1 / y2),
 *                                unweighted (step 2: h = w_i (c_uu + c_vv) with w_i the robust weight).
 * These values do not depend on the gauge, on the Jacobi scaling or on povar_set_jl_col_scaling: there is no coords argument
 * and no caveat about where the gauge is fixed.  In the free gauge, over all observations of an unsharded context,
 *       sum_i h_i = rank J = DIM n_cams + 3 n_lms - nq     (DIM = 12, nq = 12 in step 1; DIM = 11, nq = 15 in step 2).
 * From the same factor as the landmark calls: C = W W^T, Sigma_l (without the gauge correction, which cancels in J C J^T) and
 * one more workgroup per landmark; given C a row is reproducible (no atomics; with the ordered assembly, as above, bit for bit).
 *   gauge, lambda   the camera calls' rules.  POVAR_COV_DAMPED: h = tr(J_i H(lambda)^-1 J_i^T).
 *   lm_ids, n_ids   as the landmark calls'.
 *   obs_cov, n_rows 4 n_rows doubles.  The rows are the observations of the requested landmarks in the caller's CSR order:
 *                   NULL: every observation of the context in order; a list: the tracks concatenated in list order, duplicates
 *                   allowed.  n_rows must be the number of rows the request produces, else an argument error.  On a sharded
 *                   context each rank returns its shard's observations.
 * Preconditions, the pivot rule, side effects (on the dense matrix, POVAR_BUF_SC_FACTOR and POVAR_BUF_COV_*), the sharded rule
 * and the memory errors are those of the landmark calls.  On POVAR_NUMERIC_FAILURE every entry is NaN.  The status judges the
 * factorisation only: an observation with y2 == 0 (a point in the camera's principal plane) gets non-finite c_* by IEEE
 * rules with status 0, and its h is unaffected in step 1 (step 2's linearisation already reports such a point). ---- */
/* after povar_linearize_pose */
int povar_observation_covariance_pose(povar_ctx* ctx, double lambda, int32_t gauge,
                                      const int32_t* lm_ids /* NULL = all landmarks of the context */, int32_t n_ids,
                                      double* obs_cov /* 4 n_rows */, int64_t n_rows);
/* after povar_linearize_homogeneous */
int povar_observation_covariance_joint(povar_ctx* ctx, double lambda, int32_t gauge,
                                       const int32_t* lm_ids /* NULL = all landmarks of the context */, int32_t n_ids,
                                       double* obs_cov /* 4 n_rows */, int64_t n_rows);

/* ---- per-observation residuals and hat blocks: what an outlier test (data snooping) of single observations needs.  For every
 * observation of the requested landmarks the weighted residual r_i (d numbers: the r the step minimises, sqrt(w_i) included)
 * and the whole d x d block P_ii = J_i H^+ J_i^T of the hat matrix whose trace is the h of the calls above.  One row each:
 *       pose  (d = 4), stride 14:  r0 r1 r2 r3,  P00 P01 P02 P03 P11 P12 P13 P22 P23 P33
 *       joint (d = 2), stride  5:  r0 r1,        P00 P01 P11
 * (the upper triangle by rows; the block is symmetric).  The rows come in the order of the calls above.  Like h, the blocks do
 * not depend on the gauge, on the Jacobi scaling or on povar_set_jl_col_scaling.
 * The deletion statistic of observation i is a d x d computation on its row:
 *       t_i = r_i^T (I_d - P_ii)^+ r_i.
 * Where J^T r = 0 (a stationary point: a converged state) t_i is exactly the decrease of the linearised cost |r + J delta|^2 when
 * observation i is removed and all cameras and landmarks are re-estimated; elsewhere it is that decrease only up to the
 * gradient's part.  The rank of I_d - P_ii is the local redundancy of the observation: every observation of a two-view track has
 * exactly one null direction (its eigenvalue is rounding noise, the others are of the order 1e-3 and above on ordinary
 * problems), r_i has no component along it, and the pseudo-inverse leaves it out.  The library returns r and P; the rank
 * decision is a tolerance on a d x d matrix and is the caller's (capi.deletion_statistics, bal --observation-diagnostics-path).
 * POVAR_COV_DAMPED: P = J H(lambda)^-1 J^T and the statistic belongs to the damped problem.  Where the damping reaches every
 * parameter (step 2: cameras and landmarks) I - P_ii is nonsingular; step 1 damps the cameras only (lambda_l = 0), and there
 * the null direction of a two-view observation, which lives in its undamped landmark, stays null.
 * From the same walk as the calls above (one body, another row).  Arguments, the gauge / lambda rules, lm_ids and n_rows,
 * preconditions, side effects, the sharded rule, the memory errors and the NaN rule on POVAR_NUMERIC_FAILURE are exactly those of
 * povar_observation_covariance_*.  The status judges the factorisation only: y2 == 0 in step 2 leaves the row non-finite by
 * IEEE rules with status 0. ---- */
/* after povar_linearize_pose */
int povar_observation_hat_pose(povar_ctx* ctx, double lambda, int32_t gauge,
                               const int32_t* lm_ids /* NULL = all landmarks of the context */, int32_t n_ids,
                               double* rows /* 14 n_rows */, int64_t n_rows);
/* after povar_linearize_homogeneous */
int povar_observation_hat_joint(povar_ctx* ctx, double lambda, int32_t gauge,
                                const int32_t* lm_ids /* NULL = all landmarks of the context */, int32_t n_ids,
                                double* rows /* 5 n_rows */, int64_t n_rows);

/* ---- covariance blocks of parameter pairs: the cross-covariances the calls above do not return (ceres::Covariance takes a
 * list of parameter-block pairs for the same reason): what the uncertainty of a relative pose, a baseline, the distance of two
 * points or a point in another camera's frame is made of.  In the setting of the landmark calls, with W_i = E_i Hll_l^-1
 * (E_i the block of Hpl of observation i of landmark l), the block of a pair is
 *       camera a, camera b        C[a, b]
 *       camera c, landmark l      -sum_{j in obs(l)} C[c, c_j] W_j                                     (dim x 3)
 *       landmark l, landmark m    delta_lm Hll_l^-1 + sum_{i in obs(l), j in obs(m)} W_i^T C[c_i, c_j] W_j
 * and a (landmark, camera) pair gets the transpose of the (camera, landmark) block.
 *   gauge  POVAR_COV_DAMPED: C = S(lambda)^-1; the blocks are exactly those of H(lambda)^-1.
 *          POVAR_COV_FREE_GAUGE (lambda = 0): C = S(0)^+; the blocks of the covariance with the gauge fixed on the cameras, the
 *          one the camera and the landmark calls take their diagonal blocks of (the top-left part of [[H0, Cg], [Cg^T, 0]]^-1,
 *          Cg = [Q; 0]).  Same lambda rules, pivot rule and errors as the camera calls.
 *   coords POVAR_COV_SOLVER_COORDS: a camera has 12 (pose) or 11 (joint) coordinates, a landmark 3.  POVAR_COV_CAMERA_COORDS
 *          (= POVAR_COV_LANDMARK_COORDS, the parameters' own coordinates): a camera 12, a landmark 3 (pose) or 4 (joint); the
 *          block is M_a T M_b^T with the maps of the calls above (camera: D or D N_c; landmark: diag(s_l) or D4 N_l).
 *   pairs  4 n_pairs numbers, (kind_a, id_a, kind_b, id_b) per pair, kind POVAR_COV_BLOCK_CAMERA or POVAR_COV_BLOCK_LANDMARK.
 *          Camera ids are global; landmark ids index the context's own landmarks (on a sharded context: the rank's shard, as
 *          lm_ids of the landmark calls -- a pair of landmarks of two different shards is therefore not served).  Any pair is
 *          valid: a == b, a camera with a landmark it does not observe, duplicates.  An unknown kind or an id out of range
 *          is an argument error.
 *   blocks, n_out   the blocks one after the other in request order, each rows(a) x cols(b) row-major without padding.  n_out
 *          must be the number of doubles the request produces, else an argument error.
 * From the same factor as the landmark calls (C = W W^T off the diagonal too), then one workgroup per pair; no atomics and every
 * sum in a fixed order: given C a block is reproducible (with the ordered assembly, as above, bit for bit across calls).  Every
 * pair is evaluated in one canonical order: the block of (b, a) is the bitwise transpose of the block of (a, b), a block with
 * a == b is symmetric bit for bit, duplicates are the same bits.
 * Preconditions, the sharded rule (every rank calls) and the memory errors are those of the landmark calls.  Side effects: with
 * n_pairs > 0 those of a landmark call with n_ids > 0 (POVAR_BUF_COV_INVERSE, _PANEL and _GAUGE hand out W, C and Q;
 * POVAR_BUF_SC_FACTOR is an argument error afterwards); n_pairs = 0 returns 0 and leaves W alone, as a camera call does.  On
 * POVAR_NUMERIC_FAILURE every entry of blocks is NaN. ---- */
enum { POVAR_COV_BLOCK_CAMERA = 0, POVAR_COV_BLOCK_LANDMARK = 1 };
/* after povar_linearize_pose: the 12 n_cams system of step 1 */
int povar_covariance_blocks_pose(povar_ctx* ctx, double lambda, int32_t gauge, int32_t coords,
                                 const int32_t* pairs /* 4 n_pairs */, int32_t n_pairs, double* blocks /* n_out */, int64_t n_out);
/* after povar_linearize_homogeneous: the 11 n_cams tangent system of step 2 */
int povar_covariance_blocks_joint(povar_ctx* ctx, double lambda, int32_t gauge, int32_t coords,
                                  const int32_t* pairs /* 4 n_pairs */, int32_t n_pairs, double* blocks /* n_out */, int64_t n_out);

/* ---- inspection of internal state in the reference's layouts (parity tests) ---- */
enum {
  POVAR_BUF_DIAG2 = 0,     /* get_Jp_diag2_pOSE, 12 n_cams (linearization_varproj.hpp:183-222) */
  POVAR_BUF_POSE_SCALING,  /* pose_jacobian_scaling_pOSE_, 12 n_cams (linearizor_power_varproj.cpp:68-70) */
  POVAR_BUF_JL_COL_SCALE,  /* Jl_col_scale_pOSE, 3 n_lms (landmark_block.hpp:289-292) */
  POVAR_BUF_HLL_INV,       /* hll_inv_pOSE_, 9 n_lms (linearization_power_varproj.hpp:469) */
  POVAR_BUF_B,             /* b_p, 12 n_cams */
  POVAR_BUF_B_INV,         /* b_inv_pOSE_, 144 n_cams */
  POVAR_BUF_STORAGE,       /* storage_pOSE_ of every landmark, [4 n_obs][16] (landmark_block.hpp:726) */
  POVAR_BUF_JL_COL_SCALE_H, /* Jl_col_scale_homogeneous, 4 n_lms (landmark_block.hpp:303-306) */
  POVAR_BUF_B_JOINT,       /* b_p of prepare_Hb_joint, 11 n_cams */
  POVAR_BUF_B_INV_JOINT,   /* b_inv_joint_, 121 n_cams */
  POVAR_BUF_NC_HOUSEHOLDER, /* per camera (w[12], beta): N_c = (I - beta w w^T)[:, 1:], 13 n_cams */
  POVAR_BUF_SC_PRECOND,    /* Schur-Jacobi inv_blocks of the last povar_solve_*_sc (preconditioner.hpp:80-107),
                              144 n_cams (step 1) or 121 n_cams (step 2) */
  POVAR_BUF_SC_BLOCKDIAG,  /* B_c = Hpp_c + lambda I of the last povar_solve_*_sc, same sizes */
  POVAR_BUF_SC_FACTOR,     /* the factored augmented matrix of the last successful CHOLESKY / RICHOLESKY solve and its two
                              triangular solves: N x (N + 2) doubles row-major, N = dim n_cams rounded up to 64 (dim = 12
                              for step 1, 11 for step 2).  Row i: M[i, 0:N] (row i of the upper factor R in the columns
                              j >= i, S = R^T R; the columns j < i are unspecified), then y_i (R^T y = -b: column N of the
                              augmented matrix after the factorisation) and x_i (R x = y; the increment is x[0:dim n_cams]).
                              Rows and columns past dim n_cams are the padding: identity in R, 0 in y and x.
                              With povar_set_dense_compaction(1) read n = the row count of povar_dense_layout for dim n_cams,
                              here and in the three POVAR_BUF_COV_* below that are sized by N: x[0:n] is the increment of the
                              free cameras in the order of cam_row.
                              Precondition: the last call that wrote the dense matrix was a CHOLESKY / RICHOLESKY solve
                              that found it positive definite; any other state (no direct solve yet, a failed
                              factorisation, a povar_*_covariance_* call since, which inverts R in place) is an argument
                              error.  PCG / RIPCG and the power series leave the factor alone.  On a sharded context every
                              rank holds the all-reduced matrix. */
  POVAR_BUF_COV_FACTOR,    /* the four POVAR_BUF_COV_* hand out what the last povar_*_covariance_* call left on the device.
                              Precondition of all four: the last call that wrote the dense matrix was a covariance call
                              that returned 0; any other state (no such call yet, POVAR_NUMERIC_FAILURE, a CHOLESKY /
                              RICHOLESKY solve since) is an argument error.  N = dim n_cams rounded up to 64, n = dim n_cams.
                              COV_FACTOR: N x N row-major, the augmented matrix's first N columns after the factorisation: the
                              upper factor R (A = R^T R, A = S(lambda) or S0 + Q Q^T) the inversion started from, in the
                              columns j >= i; the columns j < i are unspecified; rows and columns past n are the identity's.
                              It is a copy made before W overwrites R, only while povar_set_cov_inspect is on: an argument
                              error when the switch was off during that call. */
  POVAR_BUF_COV_INVERSE,   /* N x N row-major, the dense matrix after the call.  The upper block triangle of 64 x 64 blocks
                              holds W = R^-1 (upper triangular: zero below the diagonal inside the diagonal blocks, the
                              identity on the padding).  After a landmark call with n_ids > 0 the strictly lower 64 x 64 blocks
                              hold C = W W^T; after a camera call they are unspecified. */
  POVAR_BUF_COV_PANEL,     /* N x 64 row-major: rows 64 I .. 64 I + 63 are the diagonal block I of C = W W^T.  Valid after a
                              landmark call with n_ids > 0 only; an argument error after a camera call. */
  POVAR_BUF_COV_GAUGE      /* n x nq row-major (nq = 12 pose, 15 joint): the orthonormal gauge basis Q of the last covariance
                              call, in the solver's coordinates.  An argument error when that call was POVAR_COV_DAMPED. */
};
/* enable = 1: every later povar_*_covariance_* call keeps a device copy of its factor R for POVAR_BUF_COV_FACTOR (8 N^2 bytes
 * more, counted in povar_device_bytes; not enough memory: the error of CHOLESKY / RICHOLESKY).  0 (default): no allocation,
 * no copy.  For tests that hold the stages of the covariance path to their own rounding-error bounds. */
int povar_set_cov_inspect(povar_ctx* ctx, int32_t enable);
int povar_get_buffer(povar_ctx* ctx, int32_t which, double* out, int64_t n);

/* ---- measurement ---- */
int povar_profile_enable(povar_ctx* ctx, int32_t enable);
int povar_profile_get(povar_ctx* ctx, povar_profile_info* out);
/* bytes of device memory held by the context */
int64_t povar_device_bytes(povar_ctx* ctx);
/* Byte floor of ONE application of E0 (right_mul_e0_pOSE, linearization_power_varproj.hpp:364-406) in the
 * context's current E0 mode: what the landmark-major kernel and the per-camera kernel must stream by design
 * (each array once).  bench.py prices the HIP-event time of those kernels against it (roofline.achieved). */
int povar_e0_model_bytes(povar_ctx* ctx, int64_t* lm_kernel_bytes, int64_t* cam_kernel_bytes);
/* Device-side stage timings (hipEvent pairs on the context's stream around the entry points), the source of the
 * IterationSummary timing fields of solver/solver_summary.hpp:186-212 that LinearizorPowerVarproj fills from host
 * timers (linearizor_power_varproj.cpp:61-72, 194-233, 257-258).  Accumulated since povar_timings_enable(ctx, 1). */
typedef struct {
  double linearize_ms;  /* linearize_pOSE / linearize_projective_space_homogeneous: stage1_time */
  int64_t linearize_calls;
  double prepare_ms;    /* prepare_Hb_*: prepare_time (+ scale_pose_jacobian, landmark_damping) */
  int64_t prepare_calls;
  double solve_ms;      /* solve_pOSE / solve_joint (power series) or PCG / CHOLESKY: solve_reduced_system_time */
  int64_t solve_calls;
  double apply_ms;      /* apply / apply_joint: back_substitution_time + update_cameras_time */
  int64_t apply_calls;
  double other_ms;      /* cost evaluations, landmark initialisation */
  int64_t other_calls;
} povar_timings_info;
int povar_timings_enable(povar_ctx* ctx, int32_t enable);
int povar_timings(povar_ctx* ctx, povar_timings_info* out);
/* what the layout of the per-term E0 kernel decided for this problem (measurement / DESIGN.md tables) */
typedef struct {
  int32_t grid;         /* E0 workgroups */
  int32_t lds_slots;    /* camera slots (record + accumulators) of the fullest workgroup */
  int32_t n_global;     /* cameras resident in every workgroup */
  int32_t n_tail;       /* cameras resident in one row and one column of the workgroup grid */
  int64_t n_tiles, n_rows;  /* 64-lane tiles and observation rows of the row stream */
  int64_t n_cold;       /* observations whose camera is not LDS-resident in their workgroup */
  int64_t n_obs;
  int64_t lane_per_landmark; /* 1: the term loop runs e0_lpl / e0_lpl_h on this layout; 0: the lane-per-observation
                                kernels (problems under 65 536 observations, POVAR_E0_V1=1) */
  double create_ms;     /* host wall time of povar_create: layout construction + uploads (the reference's counterpart,
                           allocating the landmark blocks, sc/linearization_varproj.hpp:44-60, is part of its
                           preprocessor_time_in_seconds too, bal_bundle_adjustment.cpp:260-286) */
  int32_t strategy;     /* landmark -> workgroup assignment the layout chose: 0 rank-based camera grid (graphs without
                           locality), 1 contiguous landmark ranges with per-workgroup camera sets (the file's landmark
                           order carries the locality, as for the reference: bal/bal_problem.cpp:183-303) */
  int32_t hubs;         /* camera slots per workgroup with four accumulator replicas */
  int32_t placement;    /* LDS bank placement of the rows: 0 natural order (none), 1 placed inside povar_create,
                           2 being placed on a host thread (the kernels run on the natural order meanwhile),
                           3 placed rows swapped in */
  double placement_ms;  /* host wall time of the background placement (0 until it has finished) */
  int32_t e0_kernel;    /* per-term E0 kernel of step 1: 0 e0_lpl (lane = landmark, cameras in LDS), 1..6: the e0_ck
                           instantiation in use (lane = camera chunk, landmarks in LDS; povar_set_e0_kernel); with
                           POVAR_DETERMINISTIC=1: 7 = e0_ck_det (the bit-reproducible camera-chunk kernel), 0 = the gather form */
  int32_t ck_ready;     /* 1: the camera-chunk layout of the rows in use exists (with the rows placed on a host thread
                           it arrives together with them) */
  int32_t ck_batches, ck_slots;  /* landmark batches per workgroup, landmark slots per batch */
  int32_t ck_tiles_max; /* most chunk tiles of one (workgroup, batch) */
  int32_t ck_part_rec;  /* partial records of the camera-chunk kernel (workgroup slots + chunks of cameras without one) */
  int64_t ck_rows, ck_chunks, ck_cold_chunks;
  double ck_build_ms;   /* host time of the derivation from the lane-per-landmark layout */
  int32_t e0_auto;      /* 0: the E0 kernel was forced (POVAR_E0_CK, povar_set_e0_kernel); 1: the library will time e0_lpl and e0_ck
                           on this problem at the next power series; 2: it has (e0_kernel is its choice) */
  float tune_lpl_us, tune_ck_us;  /* what that timing saw: microseconds per term pair (the E0 kernel + the per-camera kernel behind it), the faster of two rounds */
  /* step 2 (solve_joint): the same pair of kernels for the homogeneous operator, on a layout instance of its own
   * (64 instead of 48 bytes of LDS per landmark slot: more batches, shorter chunks) */
  int32_t e0_kernel_h;  /* 0: e0_lpl_h, 1: e0_ck_h; with POVAR_DETERMINISTIC=1: 2 = e0_ck_h_det, 0 = the gather form */
  int32_t ckh_ready, ckh_batches, ckh_slots;
  int64_t ckh_chunks, ckh_cold_chunks;
  int32_t e0_auto_h;    /* as e0_auto: 0 forced, 1 to be timed at the next step-2 power series, 2 timed */
  float tune_lpl_h_us, tune_ck_h_us;
  /* resident power series (series_res, povar_kernels_res.hpp: res_series with ResPose): the whole loop of solve_pOSE
   * (sc/linearization_power_varproj.hpp:191-237) in one launch, observation rows in registers, landmarks and B^-1 in LDS */
  int32_t res_ready;    /* 1: the layout exists (the context's observations fit the lanes of one workgroup per CU) */
  int32_t res_active;   /* 1: the next step-1 power series of this context runs as the resident kernel */
  int32_t res_auto;     /* 0 forced (POVAR_RES, povar_set_series_kernel), 1 to be timed at the next series, 2 timed */
  int32_t res_wgs, res_waves, res_rows, res_rounds;  /* workgroups, wavefronts per workgroup, rows per chunk, chunks per lane */
  int32_t res_records;  /* partial records = (workgroup, camera) pairs */
  int32_t res_max_cams, res_max_lms, res_max_chunks, res_max_oq;  /* of the fullest workgroup: cameras, landmarks, chunks,
                           partial records it reads as the owner of cameras */
  int32_t res_order;    /* landmark order the workgroup ranges were cut from: 0 natural (file) order, 1 by rarest camera */
  int32_t res_lds_bytes;
  double res_build_ms;
  float tune_terms_us, tune_res_us;  /* what the timing saw, microseconds per term: per-term kernels, resident series */
  int32_t res_failed;   /* 1: a resident series gave up (its workgroups were not all on the device together); the
                           context repeated that series with the per-term kernels and stays on them */
  int32_t ck_packed;    /* 1: the rows of the camera-chunk layout keep the image points packed (two int32 of micro-units,
                           8 instead of 16 bytes per observation and walk): every observation of the problem is a six-decimal
                           number -- what the reference's files hold, bal/bal_problem.cpp:373-375 -- and comes back bit for bit */
  int32_t ck_cold_q;    /* 1: chunks of cameras without an accumulator slot leave q of each observation (32 bytes) in the cold
                           camera-major view instead of a 96-byte partial record per chunk (layouts with at most 8 % cold observations) */
  int32_t ckh_stride;   /* step 2's camera-chunk layout: landmark slots the LDS arrays of e0_ck_h are cut for -- 1536, or 2048 where
                           that saves a landmark batch (then with ckh_accumulators < lds_slots: the workgroup keeps the accumulator
                           slots of its most observed cameras, the other cameras' chunks write records of their own) */
  int32_t ckh_accumulators;      /* accumulator slots per workgroup at most */
  int64_t ckh_capped_obs;        /* observations of cameras that have a slot in the lane-per-landmark layout but none here */
  /* resident power series of step 2 (series_res_h, povar_kernels_res.hpp: one body with series_res): the loop of
   * solve_joint (:240-287) in one launch.  The res_* fields above stay step 1's.  (fp32_terms stays the struct's last
   * field; these stand in front of it.) */
  int32_t res_ready_h;  /* 1: step 2 has an instance (its own, or step 1's: res_shared_h) and an instantiation for its shape */
  int32_t res_active_h; /* 1: the next povar_solve_joint of this context runs its series as the resident kernel */
  int32_t res_auto_h;   /* as res_auto, for step 2: 0 forced, 1 to be timed at the next step-2 series, 2 timed */
  int32_t res_shared_h; /* 1: step 1's cut fits the LDS under the step-2 formula: the two instances share every array but uv */
  int32_t res_wgs_h, res_waves_h, res_rows_h, res_rounds_h;
  int32_t res_lds_bytes_h;
  double res_build_h_ms;  /* host time of the step-2 instance (the check of step 1's cut, or the second build and upload) */
  float tune_terms_h_us, tune_res_h_us;  /* step 2, microseconds per term: per-term kernels, resident series */
  int32_t fp32_terms;   /* 1: the last step-1 power series (povar_power_series_pose / _step) ran its terms in fp32
                           (POVAR_FLAG_FP32_TERMS: e0_ck_f32) */
} povar_layout_info;
int povar_get_layout_info(povar_ctx* ctx, povar_layout_info* out);
/* The reference's constructor is a trivial allocation (sc/linearization_varproj.hpp:44-60); this library's builds the
 * lane-per-landmark row stream, and the LDS bank placement of its rows is two thirds of that time while it only buys
 * 10 % of the term rate.  From 2^20 observations on (POVAR_LPL_PLACE=sync|async|none overrides) povar_create therefore
 * returns on the natural row order and a host thread places the rows; they are swapped in by the first
 * povar_linearize_* call that finds them ready.  povar_layout_finalize(ctx, 1) waits for the thread and swaps at
 * once (benchmarks; a linearisation taken before is dropped: linearise again), (ctx, 0) swaps only if ready.
 * Returns 1 if the placed rows are in use after the call, 0 if not (yet), < 0 on error. */
int povar_layout_finalize(povar_ctx* ctx, int32_t wait);
/* Per-term E0 kernels (step 1 replaces right_mul_e0_pOSE, sc/linearization_power_varproj.hpp:364-406; step 2
 * right_mul_e0_joint, :408-453; either way): 0 = e0_lpl / e0_lpl_h; > 0 = the camera-chunk kernels: for step 2 e0_ck_h
 * (povar_kernels_ck_joint.hpp), for step 1 one of the e0_ck instantiations (povar_kernels_ck.hpp; table POVAR_CK_VARIANTS in povar_ctx.hpp: wavefronts per
 * workgroup, register-resident tiles, rows in flight).  Environment: POVAR_E0_CK=<n> sets the initial choice, which also
 * decides how the camera-chunk layout is cut (chunk cap, wavefronts the tiles are scheduled over).  kernel = -1 (the
 * default when nothing is forced): the library times both kernels of a step once per layout on the prepared problem and
 * keeps the faster one (povar_layout_info.e0_auto[_h], tune_*_us). */
int povar_set_e0_kernel(povar_ctx* ctx, int32_t kernel);
/* The m-term loop of solve_pOSE (sc/linearization_power_varproj.hpp:191-237) and of solve_joint (:240-287; povar_solve_joint
 * runs series_res_h, with a layout instance, a timing and a choice of its own) as per-term kernels inside a hipGraph
 * (mode 0) or as ONE resident launch that keeps the term-invariant operands on the chip (mode 1; contexts of up to 400 000
 * observations -- POVAR_RES_MAX_OBS -- in the LDS-accumulating E0 mode, without peers: a context with a communicator of more
 * than one rank or with the peer-to-peer exchange runs the per-term kernels);
 * -1 (default): the library times both once per context and step on the caller's prepared system and keeps the faster one
 * (povar_layout_info.res_auto[_h], tune_terms[_h]_us, tune_res[_h]_us).  The switch covers both steps; a series of either
 * step that gives up (res_failed) leaves both on the per-term kernels.  Environment: POVAR_RES=0|1. */
int povar_set_series_kernel(povar_ctx* ctx, int32_t mode);
/* Assembly of the dense reduced camera matrix that CHOLESKY, RICHOLESKY and the covariance calls factor (one switch: they share
 * the assembly).  mode 1: fp64 atomics, a workgroup per landmark (sc_dense_offdiag[_h]; the last bits depend on the arrival
 * order); mode 2: the ordered kernel (sc_dense_ordered, povar_kernels_sc.hpp): the same terms, no floating-point atomic, added
 * in an order that is a function of the context's layout alone -- with it a direct solve and a covariance are bit-reproducible
 * run to run (sharded: for a given device count and an all-reduce that sums in a fixed order, as the host hook does);
 * mode -1 (default): the library's choice, ordered on a POVAR_FLAG_DETERMINISTIC context and atomics otherwise.  On a
 * deterministic context the choice is pinned: the call returns 0 and changes nothing.  An unknown mode is an argument error. */
int povar_set_sc_assembly(povar_ctx* ctx, int32_t mode);
/* the assembly the context's last dense call ran: 0 = none yet, 1 = atomics, 2 = ordered (PCG / RIPCG and the power series
 * assemble nothing and leave the value alone); < 0 on error */
int povar_sc_assembly(povar_ctx* ctx);
/* Diagnostic builds only (tools/variants/build_variant.sh ck_stamps -- a patched copy of the sources --, tools/ck_stamps.py):
 * in-kernel s_memtime stamps of e0_ck's phases, [workgroups][16 wavefronts][40]; the first call arms the collection.  The
 * shipped library executes no stamp and returns an error. */
int povar_debug_ck_stamps(povar_ctx* ctx, uint64_t* out, int64_t n);

/* ---- multi-GPU: landmarks sharded over ranks, one RCCL all-reduce per exchange step ---- */
/* host-only: contiguous landmark range of `rank`, balanced by observation count */
int povar_shard_range(int32_t n_lms, const int32_t* lm_offsets, int32_t world, int32_t rank,
                      int32_t* lm_begin, int32_t* lm_end);
int povar_comm_unique_id(uint8_t id[128]);
int povar_comm_init(povar_ctx* ctx, int32_t world, int32_t rank, const uint8_t id[128]);
/* ranks of the attached communicator (ncclCommCount; the world size of a host hook), 0 = none, < 0 on error */
int povar_comm_ranks(povar_ctx* ctx);
/* Peer-to-peer exchange of the per-term E0 partials, on top of a communicator attached with
 * povar_comm_init / povar_comm_init_host (which keeps serving the once-per-solve exchanges): instead of one
 * all-reduce of 12 n_cams doubles per power-series term, every rank's per-camera kernel pushes its partial sums
 * into every peer's exchange buffer (stores over xGMI) and the B^-1 kernel of every rank waits for the world's slabs
 * of its camera and sums them in rank order -- two kernels and no library call per term, deterministic for a world.
 * Every rank calls povar_p2p_export(ctx, world, handle) (allocates its buffer, returns a 64-byte hipIpcMemHandle),
 * the launcher gathers the handles, every rank calls povar_p2p_attach(ctx, world, rank, handles[world][64]). */
int povar_p2p_export(povar_ctx* ctx, int32_t world, uint8_t handle[64]);
int povar_p2p_attach(povar_ctx* ctx, int32_t world, int32_t rank, const uint8_t* handles);
/* switch the per-term exchange between the attached peer-to-peer kernels (on != 0) and the communicator's
 * all-reduce (0): a launcher validates the first against the second before it trusts it (bench.py does) */
int povar_p2p_enable(povar_ctx* ctx, int32_t on);
/* same exchange steps through a caller-supplied host all-reduce (sum, in place) instead of RCCL:
 * lets an MPI/gloo launcher or an in-process test stand in for the communicator */
typedef void (*povar_allreduce_fn)(double* buf, int64_t n, void* user);
int povar_comm_init_host(povar_ctx* ctx, int32_t world, int32_t rank, povar_allreduce_fn fn, void* user);

#ifdef __cplusplus
}
#endif
#endif
