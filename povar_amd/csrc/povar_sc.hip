// povar_sc.hip -- explicit-Schur-complement solvers (LinearizorSC: PCG, CHOLESKY, RIPCG).
#include "povar_ctx.hpp"
#include "povar_kernels_cov.hpp"

// ------------------------------------------------------------------------------------------
// explicit-Schur-complement solvers (LinearizorSC: PCG, CHOLESKY, RIPCG)
// ------------------------------------------------------------------------------------------

int ensure_sc(povar_ctx* c) {
  if (c->sc_s.p) return 0;
  const size_t nc = c->n_cams;
  HIP_TRY(c->sc_dm_part.alloc(60 * (size_t)std::max(c->n_items, 1), &c->bytes));
  HIP_TRY(c->sc_dm.alloc(60 * nc, &c->bytes));
  HIP_TRY(c->sc_bmat.alloc(144 * nc, &c->bytes));
  HIP_TRY(c->sc_minv.alloc(144 * nc, &c->bytes));
  HIP_TRY(c->sc_x.alloc(12 * nc, &c->bytes));
  HIP_TRY(c->sc_r.alloc(12 * nc, &c->bytes));
  HIP_TRY(c->sc_p.alloc(12 * nc, &c->bytes));
  HIP_TRY(c->sc_q.alloc(12 * nc, &c->bytes));
  HIP_TRY(c->sc_zv.alloc(12 * nc, &c->bytes));
  HIP_TRY(c->sc_part.alloc(4 * (size_t)c->n_cam_blocks, &c->bytes));
  HIP_TRY(c->sc_s.alloc(PS_COUNT, &c->bytes));
  c->sc = ScP{c->sc_dm_part.p, c->sc_dm.p, c->sc_bmat.p, c->sc_minv.p, c->sc_x.p, c->sc_r.p, c->sc_p.p,
              c->sc_q.p,       c->sc_zv.p, c->sc_part.p, c->sc_s.p,    c->ncw.p};
  return 0;
}

// after povar_prepare_pose / povar_prepare_joint: B_c (matrix) and the Schur-Jacobi preconditioner
// S_cc^-1 (linearizor_sc.cpp:129-135, 271-274)
template <bool HOM>
int build_schur_jacobi(povar_ctx* c, double lambda) {
  hipLaunchKernelGGL((cm_gram_sc<HOM>), dim3(grid_for(std::max(c->n_items, 1), 4)), dim3(256), 0, c->stream, c->d,
                     c->sc.dm_part);
  hipLaunchKernelGGL(cam_sum_parts60, dim3(c->n_cams), dim3(1024), 0, c->stream, c->d, (const double*)c->sc.dm_part,
                     c->sc.dm);
  if (int rc = allreduce(c, c->sc.dm, 60 * (size_t)c->n_cams)) return rc;
  const dim3 g(grid_for(c->n_cams, K8_SC_THREADS)), b(K8_SC_THREADS);
  hipLaunchKernelGGL((cam_build_sc<HOM>), g, b, 0, c->stream, c->d, lambda, c->sc.ncw, (const double*)nullptr,
                     (double*)nullptr, c->sc.bmat, (const uint8_t*)c->fixed_mask.p);
  hipLaunchKernelGGL((cam_build_sc<HOM>), g, b, 0, c->stream, c->d, lambda, c->sc.ncw, (const double*)c->sc.dm,
                     c->sc.minv, (double*)nullptr, (const uint8_t*)c->fixed_mask.p);
  HIP_TRY(hipGetLastError());
  return 0;
}

// E0 * (vector last written by emit_z) into the dense ambient y
int e0_dense(povar_ctx* c) {
  // (POVAR_FLAG_FP32_TERMS covers the power-series terms only: the explicit-SC solvers stay in fp64)
  const TermPlan p = term_plan(c, c->joint ? 2 : 1, TermUse::dense);
  if (int rc = launch_e0(c, p)) return rc;
  if (p.cam == CamStep::scatter)
    hipLaunchKernelGGL(cam_sum_items, dim3(grid_for(c->n_cams, 4)), dim3(256), 0, c->stream, c->d, c->d.y, 1);
  return 0;
}

namespace {
// which assembly the next dense call runs (povar_set_sc_assembly): the ordered kernel where the caller asked for it and, unasked, on
// a deterministic context (whose setter changes nothing)
bool sc_assembly_ordered(const povar_ctx* c) { return c->sc_assembly == 2 || (c->sc_assembly < 0 && c->deterministic); }

}  // namespace

int no_memory(int dim, int rows, const char* what, size_t bytes) {
  return fail(-1, std::string(dim == 11 ? "RICHOLESKY" : "CHOLESKY") + ": not enough device memory for the " + what + " of " +
                      std::to_string(rows) + " rows (" + std::to_string(bytes >> 20) + " MiB)");
}

// The system as the direct and PCG solvers prepare it (an argument error without the step's linearisation): B_c and the
// Schur-Jacobi preconditioner on top of povar_prepare_pose (LinearizorSC::solve, linearizor_sc.cpp:85-160: no landmark damping
// on this path) or povar_prepare_joint (solve_joint, linearizor_sc.cpp:224-303; landmark damping is part of the prepared system)
int prepare_sc(povar_ctx* c, int dim, double lambda) {
  if (int rc = dim == 12 ? povar_prepare_pose(c, lambda, POVAR_POWER_VARPROJ) : povar_prepare_joint(c, lambda)) return rc;
  // cm_gram_sc reads the per-slot sqrt(w) and the landmark-order records: after a lane-per-landmark linearisation /
  // prepare they are rebuilt here (missing until round 3: RIPCG with a robust norm took stale weights on every problem
  // large enough for the lane-per-landmark kernels -- the parity tests' "lane-per-landmark" halves were not running
  // those kernels, tests/conftest.py)
  ensure_legacy(c);
  if (int rc = ensure_sc(c)) return rc;
  return with_step(dim, [&](auto step) { return build_schur_jacobi<decltype(step)::HOM>(c, lambda); });
}

// First half, shared with the covariance calls (povar_cov.hip): assembly of the augmented matrix and its factorisation, R left in
// sc_dense.  Q (device, n x nq row-major; null for the solvers) is the free-gauge term: A = S + Q Q^T, added on rank 0 before
// the all-reduce; `stat` (device, 2 doubles; null for the solvers) then receives max_k A_kk and min_k R_kk^2.
// The matrix spans the cameras of the step's map (povar_ctx::cam_row, povar_set_dense_compaction): all of them, the fixed ones
// turned into identity rows after the all-reduce, or the free ones alone.  No camera in it (n = 0): nothing is allocated or
// launched.
int chol_factor(povar_ctx* c, int dim, const double* Q, int nq, double* stat) {
  c->sc_factor_dim = c->sc_factor_n = 0;  // (run_cholesky sets it again once the factorisation has succeeded)
  c->cov.invalidate();  // (a covariance call sets it again once it has returned its blocks)
  const DenseDims g = dense_dims(dim, c->cam_row_n / dim);
  const int n = g.n, N = g.N;
  const int64_t ld = g.ld;
  const size_t count = g.count;
  c->layout_n = n;  // (povar_dense_layout: this call's matrix)
  c->layout_rows = c->cam_row_host;
  if (n > 0)
    if (const hipError_t e = grow_buffer(c, c->sc_dense, count, (size_t)1 << 30)) {
      if (e == hipErrorOutOfMemory) return no_memory(dim, n, "dense reduced camera matrix", count * sizeof(double));
      HIP_TRY(e);
    }
  if (!c->sc_info.p) {
    HIP_TRY(c->sc_info.alloc(1, &c->bytes));
    std::vector<int> s0(c->n_lms), cnt(c->n_lms);
    for (int l = 0; l < c->n_lms; ++l) {
      cnt[l] = c->lm_off[l + 1] - c->lm_off[l];
      s0[l] = cnt[l] > 0 ? c->slot_of_obs[c->lm_off[l]] : 0;
    }
    if (int rc = upload(c->sc_lm_slot0, s0, c)) return rc;
    if (int rc = upload(c->sc_lm_cnt, cnt, c)) return rc;
  }
  if (n == 0) return 0;
  const int* rows = c->cam_row.p;
  const int some_out = n < dim * c->n_cams ? 1 : 0;  // a camera is not in the matrix: sc_dense_offdiag[_h] may skip whole landmarks
  double* M = c->sc_dense.p;
  HIP_TRY(hipMemsetAsync(M, 0, count * sizeof(double), c->stream));
  HIP_TRY(hipMemsetAsync(c->sc_info.p, 0, sizeof(int), c->stream));
  // replicated parts (B_c, -b, padding identity) once over the ranks; the landmark part is sharded
  const bool ordered = sc_assembly_ordered(c);
  c->sc_assembly_last = ordered ? 2 : 1;
  prof_mark(c, 0);  // (povar_profile_info.e0_ms of a dense call: the assembly's launches)
  if (c->rank == 0) {
    with_step(dim, [&](auto step) {
      constexpr int DIM = decltype(step)::DIM;
      if (ordered)  // (B_c is sc_dense_ordered's last addition: the right-hand side alone)
        hipLaunchKernelGGL((sc_dense_diag<DIM, false>), dim3(c->n_cams), dim3(256), 0, c->stream, c->d, (const double*)c->sc.bmat, rows, M, ld, N);
      else
        hipLaunchKernelGGL(sc_dense_diag<DIM>, dim3(c->n_cams), dim3(256), 0, c->stream, c->d, (const double*)c->sc.bmat, rows, M, ld, N);
    });
    if (N > n) hipLaunchKernelGGL(chol_pad, dim3(1), dim3(64), 0, c->stream, M, ld, n, N);
    if (Q) hipLaunchKernelGGL(cov_add_qqt, dim3(N / CH_NB, N / CH_NB), dim3(256), 0, c->stream, M, ld, n, Q, nq);
  }
  if (ordered) {
    // (after cov_add_qqt in stream order: an entry is Q Q^T, then the workgroup's sum; every rank's cameras: rank 0 has B_c to add
    // where no landmark is)
    const unsigned n_tiles = (unsigned)((c->n_cams + SCO_T - 1) / SCO_T);
    with_step(dim, [&](auto step) {
      hipLaunchKernelGGL(sc_dense_ordered<decltype(step)>, dim3((unsigned)c->n_cams * n_tiles), dim3(SCO_WALK), 0, c->stream, c->d,
                         (const double*)c->sc.ncw, c->rank == 0 ? (const double*)c->sc.bmat : (const double*)nullptr, rows, M, ld);
    });
  } else if (c->n_lms > 0) {
    if (dim == 11)
      hipLaunchKernelGGL(sc_dense_offdiag_h, dim3(c->n_lms), dim3(256), 0, c->stream, c->d, c->sc.ncw, (const int*)c->sc_lm_slot0.p,
                         (const int*)c->sc_lm_cnt.p, rows, some_out, M, ld);
    else
      hipLaunchKernelGGL(sc_dense_offdiag, dim3(c->n_lms), dim3(256), 0, c->stream, c->d, (const int*)c->sc_lm_slot0.p,
                         (const int*)c->sc_lm_cnt.p, rows, some_out, M, ld);
  }
  prof_mark(c, -1);
  HIP_TRY(hipGetLastError());
  if (int rc = allreduce(c, M, count)) return rc;
  // fixed cameras: identity rows and columns, right-hand side 0 -- whichever assembly ran, on every rank alike.  The compacted
  // matrix holds no such row: nothing to fix, and the pivot scan skips nothing
  const uint8_t* fixed = c->compaction ? nullptr : c->fixed_mask.p;
  if (fixed && c->n_fixed > 0) hipLaunchKernelGGL(sc_fix_cameras, dim3(c->n_cams), dim3(256), 0, c->stream, M, ld, N, dim, fixed);
  if (stat) hipLaunchKernelGGL(cov_diag_scan, dim3(1), dim3(256), 0, c->stream, (const double*)M, ld, n, 0, stat, fixed, dim);
  for (int K0 = 0; K0 < N; K0 += CH_OB) {
    const int kdepth = std::min(CH_OB, N - K0), R0 = K0 + kdepth;
    for (int k0 = K0; k0 < R0; k0 += CH_NB) {
      const int k1 = k0 + CH_NB;
      hipLaunchKernelGGL(chol_diag, dim3(1), dim3(64), 0, c->stream, M, ld, k0, c->sc_info.p);
      hipLaunchKernelGGL(chol_trsm, dim3(grid_for((int64_t)N + 1 - k1, 128)), dim3(128), 0, c->stream, M, ld, k0);
      if (k1 < R0)  // the block's own remaining rows, all columns to their right (through the rhs tile)
        hipLaunchKernelGGL(chol_syrk, dim3((unsigned)((N + CH_NB - k1) / CH_NB), (unsigned)((R0 - k1) / CH_NB)), dim3(256),
                           0, c->stream, M, ld, k0);
    }
    if (R0 < N)
      hipLaunchKernelGGL(chol_syrk_outer, dim3((unsigned)((N - R0) / CH_T + 1), (unsigned)((N - R0 + CH_T - 1) / CH_T)),
                         dim3(256), 0, c->stream, M, ld, K0, kdepth);
  }
  if (stat) hipLaunchKernelGGL(cov_diag_scan, dim3(1), dim3(256), 0, c->stream, (const double*)M, ld, n, 1, stat, fixed, dim);
  HIP_TRY(hipGetLastError());
  return 0;
}

// solve_direct_pOSE (linearization_sc.hpp:236-245): accum = LLT(S).solve(-b) with the dense S,
// factored by the kernels of povar_kernels_chol.hpp.  dim = 12: step 1's system; dim = 11: the joint tangent system of
// step 2 (RICHOLESKY; not in the reference).  A context that solves both keeps one dense buffer, sized for the larger.
int run_cholesky(povar_ctx* c, int dim, int32_t* num_iterations, int32_t* termination) {
  if (int rc = chol_factor(c, dim, nullptr, 0, nullptr)) return rc;
  const DenseDims g = dense_dims(dim, c->cam_row_n / dim);
  const int n = g.n, N = g.N;
  const int64_t ld = g.ld;
  const size_t n_inc = (size_t)dim * (size_t)c->n_cams;
  if (num_iterations) *num_iterations = 0;  // LinearizationSC::Summary default (linearization_sc.hpp:71-81)
  if (termination) *termination = POVAR_LINEAR_SOLVER_SUCCESS;
  if (n == 0) {  // every camera fixed: the increment is +0.0, no factor is in place
    HIP_TRY(hipMemsetAsync(c->accum.p, 0, n_inc * sizeof(double), c->stream));
    return 0;
  }
  double* M = c->sc_dense.p;
  HIP_TRY(grow_buffer(c, c->sc_xpad, (size_t)N));
  double* x = c->sc_xpad.p;  // N entries, the first n are the solution
  hipLaunchKernelGGL(chol_copy_rhs, dim3(grid_for(N, 256)), dim3(256), 0, c->stream, (const double*)M, ld, N, x);
  for (int k0 = N - CH_NB; k0 >= 0; k0 -= CH_NB) {
    hipLaunchKernelGGL(chol_back_solve, dim3(1), dim3(64), 0, c->stream, (const double*)M, ld, k0, x);
    if (k0 > 0)
      hipLaunchKernelGGL(chol_back_update, dim3(grid_for(k0, 4)), dim3(256), 0, c->stream, (const double*)M, ld, k0, x);
  }
  HIP_TRY(hipGetLastError());
  int info = 0;
  HIP_TRY(hipMemcpyAsync(&info, c->sc_info.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (info != 0) {
    // S not positive definite: Eigen's SimplicialLLT would hand back garbage; report a non-finite step
    std::vector<double> nanv(n_inc, std::nan(""));
    HIP_TRY(hipMemcpyAsync(c->accum.p, nanv.data(), n_inc * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  } else {
    // x by rows of the matrix -> the increment by camera id; +0.0 for a camera that is not in the matrix
    hipLaunchKernelGGL(chol_scatter_x, dim3(grid_for((int64_t)n_inc, 256)), dim3(256), 0, c->stream, (const double*)x, (const int*)c->cam_row.p,
                       dim, c->n_cams, c->accum.p);
    HIP_TRY(hipGetLastError());
    c->sc_factor_dim = dim;
    c->sc_factor_n = n;
  }
  return 0;
}

template <int DIM, bool HOM>
int run_pcg(povar_ctx* c, int32_t min_it, int32_t max_it, double eta, int32_t* num_iterations, int32_t* termination) {
  const dim3 g(c->n_cam_blocks), b(K9_CAMS * 64);
  const int residual_reset_period = 10;  // ConjugateGradientsSolver::Options, conjugate_gradient.hpp:87
  const double r_tol = -1.0;             // linearizor_base.cpp:113
  HIP_TRY(hipMemsetAsync(c->flags.p + 1, 0, sizeof(int) * 3, c->stream));
  hipLaunchKernelGGL((pcg_init<DIM>), g, b, 0, c->stream, c->d, c->sc);
  hipLaunchKernelGGL(pcg_check, dim3(1), dim3(64), 0, c->stream, c->d, c->sc, c->n_cam_blocks, 0, min_it, max_it, eta, r_tol);
  int f[4] = {0, 0, 0, 0};
  if (int rc = read_flags(c, f)) return rc;
  // The termination tests run on the device (pcg_alpha / pcg_check set flags[1]; every kernel of a later
  // iteration then returns at once), so the host only polls the flag word every few iterations: the
  // launch pipeline stays full and at most kPoll - 1 empty iterations are enqueued past the end.
  constexpr int kPoll = 4;
  for (int it = 1; !f[1]; ++it) {
    hipLaunchKernelGGL((pcg_dir<DIM, HOM>), g, b, 0, c->stream, c->d, c->sc, it == 1 ? 1 : 0);
    if (int rc = e0_dense(c)) return rc;
    hipLaunchKernelGGL((pcg_apply<DIM, HOM>), g, b, 0, c->stream, c->d, c->sc);
    hipLaunchKernelGGL(pcg_alpha, dim3(1), dim3(64), 0, c->stream, c->d, c->sc, c->n_cam_blocks, it);
    if (it % residual_reset_period == 0) {
      hipLaunchKernelGGL((pcg_update<DIM, HOM>), g, b, 0, c->stream, c->d, c->sc, 1);
      if (int rc = e0_dense(c)) return rc;
      hipLaunchKernelGGL((pcg_residual<DIM, HOM>), g, b, 0, c->stream, c->d, c->sc);
    } else {
      hipLaunchKernelGGL((pcg_update<DIM, HOM>), g, b, 0, c->stream, c->d, c->sc, 0);
    }
    hipLaunchKernelGGL(pcg_check, dim3(1), dim3(64), 0, c->stream, c->d, c->sc, c->n_cam_blocks, it, min_it, max_it, eta, r_tol);
    HIP_TRY(hipGetLastError());
    // with a host exchange hook every all-reduce already synchronises; poll each iteration there
    if (it % kPoll == 0 || it >= max_it || c->host_fn)
      if (int rc = read_flags(c, f)) return rc;
  }
  hipLaunchKernelGGL(pcg_finish, dim3(grid_for((int64_t)DIM * c->n_cams, 256)), dim3(256), 0, c->stream,
                     (const double*)c->sc.x, c->accum.p, DIM * c->n_cams);
  HIP_TRY(hipGetLastError());
  if (num_iterations) *num_iterations = f[2];
  if (termination) *termination = f[3];
  return 0;
}

// LinearizorSC::solve / solve_joint behind povar_solve_pose_sc and povar_solve_joint_sc_method: PCG / RIPCG or the direct solve
// of the step's reduced camera system, the increment to the host, POVAR_NUMERIC_FAILURE when it is not finite
// (bal_bundle_adjustment.cpp:362)
static int solve_sc(povar_ctx* c, int dim, const char* who, double lambda, int32_t method, int32_t min_iterations,
                    int32_t max_iterations, double eta, double* inc, int32_t* num_iterations, int32_t* termination) {
  if (method != POVAR_SC_PCG && method != POVAR_SC_CHOLESKY) return fail(-1, std::string(who) + ": unknown method");
  if (int rc = prepare_sc(c, dim, lambda)) return rc;
  {
    TimeScope ts(c, 2);
    const int rc = method == POVAR_SC_CHOLESKY ? run_cholesky(c, dim, num_iterations, termination) : with_step(dim, [&](auto step) {
      typedef decltype(step) S;
      return run_pcg<S::DIM, S::HOM>(c, min_iterations, max_iterations, eta, num_iterations, termination);
    });
    if (rc) return rc;
  }
  if (int rc = povar_get_increment(c, inc)) return rc;
  for (size_t i = 0; i < (size_t)dim * (size_t)c->n_cams; ++i)
    if (!std::isfinite(inc[i])) return POVAR_NUMERIC_FAILURE;
  return 0;
}

extern "C" {

int povar_set_fixed_cameras(povar_ctx* c, const int32_t* cam_ids, int32_t n_ids) {
  if (int rc = check_ctx(c)) return rc;
  if (n_ids < 0) return fail(-1, "povar_set_fixed_cameras: negative n_ids");
  std::vector<uint8_t> next((size_t)c->n_cams, 0);
  for (int i = 0; cam_ids && i < n_ids; ++i) {
    if (cam_ids[i] < 0 || cam_ids[i] >= c->n_cams) return fail(-1, "povar_set_fixed_cameras: camera id out of range");
    next[(size_t)cam_ids[i]] = 1;
  }
  if (next != c->fixed_next) c->fixed_dirty = true;  // (the next preparation uploads it: povar_lm.hip, lm_prepare)
  c->fixed_next.swap(next);
  return 0;
}

int povar_fixed_cameras(povar_ctx* c, int32_t* flags) {
  if (int rc = check_ctx(c)) return rc;
  int count = 0;
  for (int k = 0; k < c->n_cams; ++k) {
    count += c->fixed_next[(size_t)k];
    if (flags) flags[k] = c->fixed_next[(size_t)k];
  }
  return count;
}

int povar_set_dense_compaction(povar_ctx* c, int32_t mode) {
  if (int rc = check_ctx(c)) return rc;
  if (mode != 0 && mode != 1) return fail(-1, "povar_set_dense_compaction: unknown mode");
  c->compaction_next = mode;  // (the next preparation rebuilds the map: povar_lm.hip, lm_prepare)
  return 0;
}

int povar_dense_compaction(povar_ctx* c) {
  if (int rc = check_ctx(c)) return rc;
  return c->compaction_next;
}

int povar_dense_layout(povar_ctx* c, int32_t* cam_row) {
  if (int rc = check_ctx(c)) return rc;
  for (int k = 0; cam_row && k < c->n_cams; ++k) cam_row[k] = c->layout_rows.empty() ? -1 : c->layout_rows[(size_t)k];
  return c->layout_n;
}

int povar_set_sc_assembly(povar_ctx* c, int32_t mode) {
  if (int rc = check_ctx(c)) return rc;
  if (mode != -1 && mode != 1 && mode != 2) return fail(-1, "unknown dense assembly");
  if (c->deterministic) return 0;  // pinned (POVAR_DETERMINISTIC)
  c->sc_assembly = mode;
  return 0;
}

int povar_sc_assembly(povar_ctx* c) {
  if (int rc = check_ctx(c)) return rc;
  return c->sc_assembly_last;
}

int povar_set_jl_col_scaling(povar_ctx* c, int32_t enable) {
  if (int rc = check_ctx(c)) return rc;
  c->d.scale_jl = enable ? 1 : 0;
  return 0;
}

int povar_solve_pose_sc(povar_ctx* c, double lambda, int32_t method, int32_t min_iterations, int32_t max_iterations,
                        double eta, double* inc, int32_t* num_iterations, int32_t* termination) {
  return solve_sc(c, 12, "povar_solve_pose_sc", lambda, method, min_iterations, max_iterations, eta, inc, num_iterations, termination);
}

int povar_solve_joint_sc_method(povar_ctx* c, double lambda, int32_t method, int32_t min_iterations, int32_t max_iterations,
                                double eta, double* inc, int32_t* num_iterations, int32_t* termination) {
  return solve_sc(c, 11, "povar_solve_joint_sc_method", lambda, method, min_iterations, max_iterations, eta, inc, num_iterations,
                  termination);
}

int povar_solve_joint_sc(povar_ctx* c, double lambda, int32_t min_iterations, int32_t max_iterations, double eta,
                         double* inc, int32_t* num_iterations, int32_t* termination) {
  return povar_solve_joint_sc_method(c, lambda, POVAR_SC_PCG, min_iterations, max_iterations, eta, inc, num_iterations, termination);
}

int povar_right_mul_e0_joint(povar_ctx* c, const double* x, double* y) {
  if (int rc = check_ctx(c)) return rc;
  if (!x || !y) return fail(-1, "null argument");
  if (!c->joint || c->prep_id == 0) return fail(-1, "povar_right_mul_e0_joint: the system prepared last is not the joint one (povar_prepare_joint)");
  if (int rc = res_verify(c)) return rc;
  const size_t n = 11 * (size_t)c->n_cams;
  // tmp11 = x, z = sigma (N_c x), dense y = sigma E0 z, out = N_c^T y: the operator RIPCG applies (schur_times) without B
  if (int rc = write_cam_vector(c, c->tmp.p, x, n)) return rc;
  HIP_TRY(hipMemsetAsync(c->flags.p + 1, 0, sizeof(int) * 3, c->stream));
  hipLaunchKernelGGL(sc_emit_z_h, dim3(c->n_cam_blocks), dim3(K9_CAMS * 64), 0, c->stream, c->d, (const double*)c->ncw.p,
                     (const double*)c->tmp.p);
  const TermPlan p = term_plan(c, 2, TermUse::right_mul);
  if (int rc = launch_e0(c, p)) return rc;
  if (p.cam == CamStep::scatter)
    hipLaunchKernelGGL(cam_sum_items, dim3(grid_for(c->n_cams, 4)), dim3(256), 0, c->stream, c->d, c->d.y, 1);
  hipLaunchKernelGGL(sc_project_y_h, dim3(grid_for(c->n_cams, 256)), dim3(256), 0, c->stream, c->d, (const double*)c->ncw.p, c->tmp.p);
  HIP_TRY(hipMemsetAsync(c->y.p, 0, sizeof(double) * 12 * (size_t)c->n_cams, c->stream));
  HIP_TRY(hipGetLastError());
  return read_cam_vector(c, y, c->tmp.p, n);
}

}  // extern "C"
