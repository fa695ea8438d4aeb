// povar_sc.hip -- explicit-Schur-complement solvers (LinearizorSC: PCG, CHOLESKY, RIPCG).
#include <optional>

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
// The run-time block dimension (12: step 1, 11: step 2) to the step type of the dense kernels: fn(ScdPose()) or fn(ScdJoint()),
// so every launch templated on the step is written once
template <class F>
auto with_step(int dim, F fn) {
  return dim == 12 ? fn(ScdPose()) : fn(ScdJoint());
}

// A device buffer the context keeps (counted in povar_device_bytes), grown to `count` elements once the stream has drained.
// `headroom` > 0: the device must have that many bytes free beside the new buffer, else hipErrorOutOfMemory without trying.
// On an error the buffer is empty.
template <typename T>
hipError_t grow_buffer(povar_ctx* c, DevBuf<T>& buf, size_t count, size_t headroom = 0) {
  if (buf.p && buf.n >= count) return hipSuccess;
  if (buf.p) {
    if (hipError_t e = hipStreamSynchronize(c->stream)) return e;
    c->bytes -= buf.n * sizeof(T);
    buf.release();
  }
  size_t free_b = 0, total_b = 0;
  if (headroom > 0) {
    if (hipError_t e = hipMemGetInfo(&free_b, &total_b)) return e;
    if (count * sizeof(T) + headroom > free_b) return hipErrorOutOfMemory;
  }
  const hipError_t e = buf.alloc(count, &c->bytes);
  if (e != hipSuccess) (void)hipGetLastError();
  return e;
}

// which assembly the next dense call runs (povar_set_sc_assembly): the ordered kernel where the caller asked for it and, unasked, on
// a deterministic context (whose setter changes nothing)
bool sc_assembly_ordered(const povar_ctx* c) { return c->sc_assembly == 2 || (c->sc_assembly < 0 && c->deterministic); }

int no_memory(int dim, int n_cams, const char* what, size_t bytes) {
  return fail(-1, std::string(dim == 11 ? "RICHOLESKY" : "CHOLESKY") + ": not enough device memory for the " + what + " of " +
                      std::to_string(dim * n_cams) + " rows (" + std::to_string(bytes >> 20) + " MiB)");
}
}  // namespace

// The system as the direct and PCG solvers prepare it (an argument error without the step's linearisation): B_c and the
// Schur-Jacobi preconditioner on top of povar_prepare_pose (LinearizorSC::solve, linearizor_sc.cpp:85-160: no landmark damping
// on this path) or povar_prepare_joint (solve_joint, linearizor_sc.cpp:224-303; landmark damping is part of the prepared system)
static int prepare_sc(povar_ctx* c, int dim, double lambda) {
  if (int rc = dim == 12 ? povar_prepare_pose(c, lambda, POVAR_POWER_VARPROJ) : povar_prepare_joint(c, lambda)) return rc;
  // cm_gram_sc reads the per-slot sqrt(w) and the landmark-order records: after a lane-per-landmark linearisation /
  // prepare they are rebuilt here (missing until round 3: RIPCG with a robust norm took stale weights on every problem
  // large enough for the lane-per-landmark kernels -- the parity tests' "lane-per-landmark" halves were not running
  // those kernels, tests/conftest.py)
  ensure_legacy(c);
  if (int rc = ensure_sc(c)) return rc;
  return with_step(dim, [&](auto step) { return build_schur_jacobi<decltype(step)::HOM>(c, lambda); });
}

// First half, shared with the covariance calls below: assembly of the augmented matrix and its factorisation, R left in
// sc_dense.  Q (device, n x nq row-major; null for the solvers) is the free-gauge term: A = S + Q Q^T, added on rank 0 before
// the all-reduce; `stat` (device, 2 doubles; null for the solvers) then receives max_k A_kk and min_k R_kk^2.
static int chol_factor(povar_ctx* c, int dim, const double* Q, int nq, double* stat) {
  c->sc_factor_dim = c->sc_factor_n = 0;  // (run_cholesky sets it again once the factorisation has succeeded)
  c->sc_cov_kind = c->sc_cov_n = 0;  // (a covariance call sets it again once it has returned its blocks)
  const DenseDims g = dense_dims(dim, c->n_cams);
  const int n = g.n, N = g.N;
  const int64_t ld = g.ld;
  const size_t count = g.count;
  if (const hipError_t e = grow_buffer(c, c->sc_dense, count, (size_t)1 << 30)) {
    if (e == hipErrorOutOfMemory) return no_memory(dim, c->n_cams, "dense reduced camera matrix", count * sizeof(double));
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
        hipLaunchKernelGGL((sc_dense_diag<DIM, false>), dim3(c->n_cams), dim3(256), 0, c->stream, c->d, (const double*)c->sc.bmat, M, ld, N);
      else
        hipLaunchKernelGGL(sc_dense_diag<DIM>, dim3(c->n_cams), dim3(256), 0, c->stream, c->d, (const double*)c->sc.bmat, M, ld, N);
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
                         (const double*)c->sc.ncw, c->rank == 0 ? (const double*)c->sc.bmat : (const double*)nullptr, M, ld);
    });
  } else if (c->n_lms > 0) {
    if (dim == 11)
      hipLaunchKernelGGL(sc_dense_offdiag_h, dim3(c->n_lms), dim3(256), 0, c->stream, c->d, c->sc.ncw, (const int*)c->sc_lm_slot0.p,
                         (const int*)c->sc_lm_cnt.p, M, ld);
    else
      hipLaunchKernelGGL(sc_dense_offdiag, dim3(c->n_lms), dim3(256), 0, c->stream, c->d, (const int*)c->sc_lm_slot0.p,
                         (const int*)c->sc_lm_cnt.p, M, ld);
  }
  prof_mark(c, -1);
  HIP_TRY(hipGetLastError());
  if (int rc = allreduce(c, M, count)) return rc;
  const uint8_t* fixed = c->fixed_mask.p;
  // fixed cameras: identity rows and columns, right-hand side 0 -- whichever assembly ran, on every rank alike
  if (c->n_fixed > 0) hipLaunchKernelGGL(sc_fix_cameras, dim3(c->n_cams), dim3(256), 0, c->stream, M, ld, N, dim, fixed);
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
  const DenseDims g = dense_dims(dim, c->n_cams);
  const int n = g.n, N = g.N;
  const int64_t ld = g.ld;
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
    std::vector<double> nanv((size_t)n, std::nan(""));
    HIP_TRY(hipMemcpyAsync(c->accum.p, nanv.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  } else {
    HIP_TRY(hipMemcpyAsync(c->accum.p, x, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    c->sc_factor_dim = dim;
    c->sc_factor_n = n;
  }
  if (num_iterations) *num_iterations = 0;  // LinearizationSC::Summary default (linearization_sc.hpp:71-81)
  if (termination) *termination = POVAR_LINEAR_SOLVER_SUCCESS;
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

// ------------------------------------------------------------------------------------------
// marginal covariance of cameras and landmarks (povar_camera_covariance_* / povar_landmark_covariance_*; not in the reference)
// ------------------------------------------------------------------------------------------
namespace {
// a scratch buffer of the covariance calls, grown to `count` doubles and kept (counted in povar_device_bytes); no memory:
// the error of CHOLESKY / RICHOLESKY
template <typename T>
int cov_buffer(povar_ctx* c, DevBuf<T>& buf, size_t count, int dim) {
  const hipError_t e = grow_buffer(c, buf, count);
  if (e == hipErrorOutOfMemory) return no_memory(dim, c->n_cams, "covariance scratch", count * sizeof(T));
  HIP_TRY(e);
  return 0;
}

// Orthonormal basis Q (n x nq, row-major) of the gauge null space of the undamped reduced system, in the solver's
// Jacobi-scaled coordinates, from the linearisation point P_c, sigma_c and the reflectors (w, beta):
//   step 1 (dim 12, nq 12): the affine gauge X -> A X that keeps the last homogeneous coordinate: generators
//           G = e_i e_j^T, i < 3:  v_c = vec(-P_c G) / sigma_c;
//   step 2 (dim 11, nq 15): the projective gauge, generators (i, j) != (3, 3), the per-camera scale absorbed: with
//           g = vec(-P_c G), h0 = the reflector's first column, a = -(h0 . g / sigma_c) / (h0 . P_c / sigma_c):
//           x_c = N_c^T ((g + a P_c) / sigma_c).
// Orthonormalised by twice-applied modified Gram-Schmidt in fp64.  false: the columns are numerically dependent.
bool gauge_basis(int n_cams, int dim, const std::vector<double>& P, const std::vector<double>& sg, const std::vector<double>& ncw,
                 std::vector<double>& Q, int& nq) {
  nq = dim == 12 ? 12 : 15;
  const size_t n = (size_t)dim * n_cams;
  std::vector<std::vector<double>> V(nq, std::vector<double>(n));
  for (int col = 0; col < nq; ++col) {
    const int gi = col / 4, gj = col % 4;  // G = e_gi e_gj^T; step 1 stops at gi = 2, step 2 at (3, 2)
    for (int c = 0; c < n_cams; ++c) {
      const double* p = P.data() + 12 * (size_t)c;
      const double* s = sg.data() + 12 * (size_t)c;
      double g[12];
      for (int r = 0; r < 3; ++r)
        for (int j = 0; j < 4; ++j) g[4 * r + j] = j == gj ? -p[4 * r + gi] : 0.0;
      if (dim == 12) {
        for (int k = 0; k < 12; ++k) V[col][12 * (size_t)c + k] = g[k] / s[k];
        continue;
      }
      const double* w = ncw.data() + 13 * (size_t)c;
      const double beta = w[12];
      double hg = 0, hp = 0;
      for (int k = 0; k < 12; ++k) {
        const double h0 = (k == 0 ? 1.0 : 0.0) - beta * w[k] * w[0];
        hg += h0 * (g[k] / s[k]);
        hp += h0 * (p[k] / s[k]);
      }
      const double a = -hg / hp;
      double y[12], wy = 0;
      for (int k = 0; k < 12; ++k) {
        y[k] = (g[k] + a * p[k]) / s[k];
        wy += w[k] * y[k];
      }
      for (int j = 0; j < 11; ++j) V[col][11 * (size_t)c + j] = y[j + 1] - beta * w[j + 1] * wy;
    }
  }
  auto dot = [&](const std::vector<double>& x, const std::vector<double>& y) {
    double s = 0;
    for (size_t i = 0; i < n; ++i) s += x[i] * y[i];
    return s;
  };
  for (int k = 0; k < nq; ++k) {
    const double norm0 = std::sqrt(dot(V[k], V[k]));
    for (int pass = 0; pass < 2; ++pass)
      for (int j = 0; j < k; ++j) {
        const double t = dot(V[j], V[k]);
        for (size_t i = 0; i < n; ++i) V[k][i] -= t * V[j][i];
      }
    const double norm = std::sqrt(dot(V[k], V[k]));
    if (!(norm > 1e-8 * norm0) || !std::isfinite(norm)) return false;
    for (size_t i = 0; i < n; ++i) V[k][i] /= norm;
  }
  Q.assign(n * nq, 0.0);
  for (int k = 0; k < nq; ++k)
    for (size_t i = 0; i < n; ++i) Q[i * nq + k] = V[k][i];
  return true;
}
}  // namespace

// What the covariance calls share: the argument checks, the prepared system, the gauge basis, the factorisation of
// CHOLESKY / RICHOLESKY (A = S(lambda), or S0 + Q Q^T in the free gauge), the pivot rule and W = R^-1 in place.
struct CovInverse : DenseDims {
  const double* q = nullptr;  // device: the gauge basis (free gauge), n x nq row-major
  int nq = 0;
};
// 0: W is in the upper block triangle of sc_dense, the scratch panel is allocated and free;  POVAR_NUMERIC_FAILURE: not
// positive definite, or singular beyond the gauge (the caller fills its outputs with NaN);  < 0: an error.  `ts` is the call's
// one solve-stage timing: it opens here, once the system is prepared, and closes when the caller is done.
static int cov_inverse(povar_ctx* c, int dim, const char* who, bool have_out, double lambda, int32_t gauge, int32_t coords,
                       CovInverse& f, std::optional<TimeScope>& ts) {
  if (int rc = check_ctx(c)) return rc;
  if (!have_out) return fail(-1, std::string(who) + ": null argument");
  if (gauge != POVAR_COV_FREE_GAUGE && gauge != POVAR_COV_DAMPED && gauge != POVAR_COV_FIXED_GAUGE)
    return fail(-1, std::string(who) + ": unknown gauge");
  if (coords != POVAR_COV_CAMERA_COORDS && coords != POVAR_COV_SOLVER_COORDS) return fail(-1, std::string(who) + ": unknown coords");
  if (gauge == POVAR_COV_FREE_GAUGE && lambda != 0.0) return fail(-1, std::string(who) + ": POVAR_COV_FREE_GAUGE takes lambda = 0");
  if (gauge == POVAR_COV_DAMPED && !(lambda > 0.0)) return fail(-1, std::string(who) + ": POVAR_COV_DAMPED takes lambda > 0");
  // (the set as the caller left it: the preparation below is the one that installs it)
  const bool any_fixed = std::find(c->fixed_next.begin(), c->fixed_next.end(), (uint8_t)1) != c->fixed_next.end();
  if (gauge == POVAR_COV_FIXED_GAUGE && lambda != 0.0) return fail(-1, std::string(who) + ": POVAR_COV_FIXED_GAUGE takes lambda = 0");
  if (gauge == POVAR_COV_FIXED_GAUGE && !any_fixed)
    return fail(-1, std::string(who) + ": POVAR_COV_FIXED_GAUGE needs fixed cameras (povar_set_fixed_cameras)");
  if (gauge == POVAR_COV_FREE_GAUGE && any_fixed)
    return fail(-1, std::string(who) + ": POVAR_COV_FREE_GAUGE with fixed cameras: the gauge they fix is POVAR_COV_FIXED_GAUGE");
  if (int rc = prepare_sc(c, dim, lambda)) return rc;
  const size_t nc = c->n_cams;
  static_cast<DenseDims&>(f) = dense_dims(dim, c->n_cams);
  ts.emplace(c, 2);
  c->sc_cov_kind = 0;  // (from here on Q, the dense matrix and the panel are rewritten: POVAR_BUF_COV_* wait for cov_done)
  const bool free_gauge = gauge == POVAR_COV_FREE_GAUGE;
  if (free_gauge) {
    std::vector<double> P(12 * nc), sg(12 * nc), ncw(13 * nc), Q;
    HIP_TRY(hipMemcpyAsync(P.data(), c->cams_lin4.p, 12 * nc * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(sg.data(), c->sigma.p, 12 * nc * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (dim == 11) HIP_TRY(hipMemcpyAsync(ncw.data(), c->ncw.p, 13 * nc * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (!gauge_basis(c->n_cams, dim, P, sg, ncw, Q, f.nq)) return POVAR_NUMERIC_FAILURE;
    if (int rc = cov_buffer(c, c->sc_cov_q, Q.size(), dim)) return rc;
    if (int rc = cov_buffer(c, c->sc_cov_stat, 2, dim)) return rc;
    HIP_TRY(hipMemcpyAsync(c->sc_cov_q.p, Q.data(), Q.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // (Q is pageable host memory that goes out of scope)
    f.q = c->sc_cov_q.p;
  }
  // (the pivot scan belongs to the undamped gauges: the damped mode judges by chol_diag's info alone)
  const bool scan = free_gauge || gauge == POVAR_COV_FIXED_GAUGE;
  if (scan && !free_gauge)
    if (int rc = cov_buffer(c, c->sc_cov_stat, 2, dim)) return rc;
  if (int rc = chol_factor(c, dim, f.q, f.nq, scan ? c->sc_cov_stat.p : nullptr)) return rc;
  c->sc_factor_dim = c->sc_factor_n = 0;  // (R becomes R^-1 below: not the factor POVAR_BUF_SC_FACTOR hands out)
  int info = 0;
  double st[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(&info, c->sc_info.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (scan) HIP_TRY(hipMemcpyAsync(st, c->sc_cov_stat.p, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (info != 0) return POVAR_NUMERIC_FAILURE;  // not positive definite: CHOLESKY's own rule
  if (scan) {
    // (fixed gauge: the same rule on S_ff(0), whose fixed cameras must have taken the whole gauge)
    // a gauge-only system keeps pivots of the order of its smallest eigenvalue; further degeneracy leaves rounding
    // noise of the order u max A_kk: the threshold sqrt(u) max A_kk sits in the gap
    const double thr = std::sqrt(std::ldexp(1.0, -53)) * st[0];
    if (!(st[1] >= thr)) return POVAR_NUMERIC_FAILURE;
  }
  double* M = c->sc_dense.p;
  const int64_t ld = f.ld;
  if (int rc = cov_buffer(c, c->sc_cov_panel, (size_t)f.N * CH_NB, dim)) return rc;
  double* panel = c->sc_cov_panel.p;
  c->sc_cov_kept = false;
  if (c->cov_inspect) {  // povar_set_cov_inspect: keep the R the inversion starts from (POVAR_BUF_COV_FACTOR)
    if (int rc = cov_buffer(c, c->sc_cov_r, (size_t)f.N * f.N, dim)) return rc;
    HIP_TRY(hipMemcpy2DAsync(c->sc_cov_r.p, (size_t)f.N * sizeof(double), M, (size_t)ld * sizeof(double), (size_t)f.N * sizeof(double),
                             (size_t)f.N, hipMemcpyDeviceToDevice, c->stream));
    c->sc_cov_kept = true;
  }
  // W = R^-1 in place, block column by block column (povar_kernels_cov.hpp)
  for (int j = 0; j < f.N / CH_NB; ++j) {
    const int64_t k0 = (int64_t)j * CH_NB;
    hipLaunchKernelGGL(cov_diag_inv, dim3(1), dim3(64), 0, c->stream, M, ld, (int)k0);
    if (j == 0) continue;
    hipLaunchKernelGGL(cov_trmm, dim3(j), dim3(256), 0, c->stream, (const double*)(M + k0), ld, (const double*)(M + k0 * ld + k0), ld,
                       panel, (int64_t)CH_NB, 0, 1, 1.0);
    hipLaunchKernelGGL(cov_trmm, dim3(j), dim3(256), 0, c->stream, (const double*)M, ld, (const double*)panel, (int64_t)CH_NB,
                       M + k0, ld, 1, j, -1.0);
  }
  // fixed cameras: W_kk = 0 on their rows, so C and everything taken from it is zero there
  if (c->n_fixed > 0)
    hipLaunchKernelGGL(cov_fix_cameras, dim3(grid_for(f.n, 256)), dim3(256), 0, c->stream, M, ld, f.n, dim, (const uint8_t*)c->fixed_mask.p);
  HIP_TRY(hipGetLastError());
  return 0;
}

// Diagonal blocks of W W^T, less Q_J Q_J^T in the free gauge, in `coords`, into the host's cov (144 n_cams).  Reads the
// upper block triangle of sc_dense only.  POVAR_NUMERIC_FAILURE: a block is not finite.
static int cov_camera_blocks(povar_ctx* c, int dim, const CovInverse& f, int32_t coords, double* cov) {
  const size_t out_count = 144 * (size_t)c->n_cams;
  if (int rc = cov_buffer(c, c->sc_cov_blocks, out_count, dim)) return rc;
  const double* M = c->sc_dense.p;
  double* blocks = c->sc_cov_blocks.p;
  HIP_TRY(hipMemsetAsync(blocks, 0, out_count * sizeof(double), c->stream));
  with_step(dim, [&](auto step) {
    constexpr int DIM = decltype(step)::DIM;
    hipLaunchKernelGGL(cov_gram<DIM>, dim3(c->n_cams), dim3(256), 0, c->stream, M, f.ld, f.n, blocks);
    hipLaunchKernelGGL(cov_finish<DIM>, dim3(c->n_cams), dim3(256), 0, c->stream, blocks, f.q, f.nq,
                       (const double*)c->sigma.p, (const double*)c->ncw.p, coords);
  });
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(cov, blocks, out_count * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < out_count; ++i)
    if (!std::isfinite(cov[i])) return POVAR_NUMERIC_FAILURE;
  return 0;
}

// a covariance call has returned 0: what POVAR_BUF_COV_* may hand out (kind 1: a camera call, 2: a landmark call)
static void cov_done(povar_ctx* c, const CovInverse& f, int kind) {
  c->sc_cov_kind = kind;
  c->sc_cov_n = f.n;
  c->sc_cov_nq = f.nq;
}

// Diagonal blocks of S(lambda)^-1 (POVAR_COV_DAMPED) or of the pseudo-inverse S(0)^+ = (S0 + Q Q^T)^-1 - Q Q^T
// (POVAR_COV_FREE_GAUGE), through the factorisation of CHOLESKY / RICHOLESKY: A = R^T R, W = R^-1 in place, blocks of W W^T.
static int camera_covariance(povar_ctx* c, int dim, double lambda, int32_t gauge, int32_t coords, double* cov) {
  const char* who = dim == 12 ? "povar_camera_covariance_pose" : "povar_camera_covariance_joint";
  CovInverse f{};
  std::optional<TimeScope> ts;
  int rc = cov_inverse(c, dim, who, cov != nullptr, lambda, gauge, coords, f, ts);
  if (rc == 0) rc = cov_camera_blocks(c, dim, f, coords, cov);
  if (rc == POVAR_NUMERIC_FAILURE) std::fill(cov, cov + 144 * (size_t)c->n_cams, std::nan(""));
  if (rc == 0) cov_done(c, f, 1);
  return rc;
}

// C = W W^T off the diagonal too (cov_lauum), then the blocks of the n_out requested landmarks into sc_cov_lm (lm_cov)
static void cov_lm_launch(povar_ctx* c, int dim, const CovInverse& f, const int* ids, int n_out, const double* q, int nq, int32_t coords) {
  double* M = c->sc_dense.p;
  const int nb = f.N / CH_NB;
  hipLaunchKernelGGL(cov_lauum, dim3((unsigned)(nb * (nb + 1) / 2)), dim3(256), 0, c->stream, M, f.ld, c->sc_cov_panel.p, nb);
  with_step(dim, [&](auto step) {
    hipLaunchKernelGGL(lm_cov<decltype(step)>, dim3(n_out), dim3(256), 0, c->stream, c->d, (const double*)c->ncw.p,
                       (const int*)c->sc_lm_slot0.p, (const int*)c->sc_lm_cnt.p, ids, (const double*)M, f.ld,
                       (const double*)c->sc_cov_panel.p, q, nq, coords, c->sc_cov_lm.p);
  });
}

static int lm_stride(int dim) {
  return with_step(dim, [](auto step) { return decltype(step)::LM_STRIDE; });
}

// A request of the landmark and observation calls: which landmarks (lm_ids null: all of them), where the results go, and what
// the two calls do alike on both sides of cov_inverse
struct CovRequest {
  const char* who = "";
  const int32_t* lm_ids = nullptr;
  int n_out = 0;
  std::vector<int> row0;     // observation call: the first row of every requested landmark, and the number of rows
  int64_t rows = 0;
  double* out = nullptr;     // the call's outputs (cam: the landmark call's camera blocks, on request): NaN on a numeric failure
  double* cam = nullptr;
  size_t count = 0, cam_count = 0;
  const int* ids = nullptr;  // device copy of lm_ids

  // n_out and the id check; with_rows: row0 and rows in the same walk
  int check(povar_ctx* c, const int32_t* lm_ids_, int32_t n_ids, bool with_rows) {
    if (int rc = check_ctx(c)) return rc;
    lm_ids = lm_ids_;
    n_out = lm_ids ? n_ids : c->n_lms;
    if (n_out < 0) return fail(-1, std::string(who) + ": negative n_ids");
    if (with_rows) row0.resize((size_t)n_out);
    for (int i = 0; (lm_ids || with_rows) && i < n_out; ++i) {
      const int l = lm_ids ? lm_ids[i] : i;
      if (l < 0 || l >= c->n_lms) return fail(-1, std::string(who) + ": landmark id out of range");
      if (!with_rows) continue;
      if (rows > INT32_MAX) return fail(-1, std::string(who) + ": more than 2^31 rows requested");
      row0[i] = (int)rows;
      rows += c->lm_off[l + 1] - c->lm_off[l];
    }
    return 0;
  }
  int all_nan() const {
    std::fill(out, out + count, std::nan(""));
    if (cam) std::fill(cam, cam + cam_count, std::nan(""));
    return POVAR_NUMERIC_FAILURE;
  }
  // After cov_inverse (and the camera blocks).  true: the call ends here with rc -- an error, a numeric failure (NaN), or
  // nothing requested: W alone is in place (kind 1; cov_lauum does not run)
  bool over(povar_ctx* c, const CovInverse& f, bool empty, int& rc) const {
    if (rc == POVAR_NUMERIC_FAILURE) rc = all_nan();
    else if (rc == 0 && empty) cov_done(c, f, 1);
    return rc != 0 || empty;
  }
  // (lm_ids is the caller's memory: the call synchronises the stream before it returns)
  int upload_ids(povar_ctx* c, int dim) {
    if (!lm_ids) return 0;
    if (int rc = cov_buffer(c, c->sc_cov_ids, (size_t)n_out, dim)) return rc;
    HIP_TRY(hipMemcpyAsync(c->sc_cov_ids.p, lm_ids, (size_t)n_out * sizeof(int), hipMemcpyHostToDevice, c->stream));
    ids = c->sc_cov_ids.p;
    return 0;
  }
};

// Landmark blocks Sigma_l = Hll^-1 + F_l^T C F_l of the requested landmarks (and, on request, the camera blocks of the
// same C): the camera call's W, then C = W W^T off the diagonal too (cov_lauum) and the per-landmark contraction (lm_cov).
static int landmark_covariance(povar_ctx* c, int dim, double lambda, int32_t gauge, int32_t coords, const int32_t* lm_ids,
                               int32_t n_ids, double* lm_cov_out, double* cam_cov) {
  CovRequest q;
  q.who = dim == 12 ? "povar_landmark_covariance_pose" : "povar_landmark_covariance_joint";
  if (int rc = q.check(c, lm_ids, n_ids, false)) return rc;
  q.out = lm_cov_out;
  q.count = (size_t)lm_stride(dim) * (size_t)q.n_out;
  q.cam = cam_cov;
  q.cam_count = 144 * (size_t)c->n_cams;
  CovInverse f{};
  std::optional<TimeScope> ts;
  int rc = cov_inverse(c, dim, q.who, lm_cov_out != nullptr || q.n_out == 0, lambda, gauge, coords, f, ts);
  if (rc == 0 && cam_cov) rc = cov_camera_blocks(c, dim, f, coords, cam_cov);
  if (q.over(c, f, q.n_out == 0, rc)) return rc;
  if (int rc2 = cov_buffer(c, c->sc_cov_lm, q.count, dim)) return rc2;
  if (int rc2 = q.upload_ids(c, dim)) return rc2;
  cov_lm_launch(c, dim, f, q.ids, q.n_out, f.q, f.nq, coords);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(lm_cov_out, c->sc_cov_lm.p, q.count * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < q.count; ++i)
    if (!std::isfinite(lm_cov_out[i])) return q.all_nan();
  cov_done(c, f, 2);
  return 0;
}

// Per-observation rows of the requested landmarks' observations: the landmark call's C, Sigma_l without the gauge correction
// (lm_cov with nq = 0 in solver coordinates, into sc_cov_lm) and the per-landmark walk obs_rows, which reads no Q: the gauge part
// of C cancels in J C J^T only if no term carries the correction.  The two calls differ in the row alone:
//   hat = false  povar_observation_covariance_*: (h, c_uu, c_uv, c_vv), obs_cov, stride 4
//   hat = true   povar_observation_hat_*: r_i and the upper triangle of P_ii, obs_hat, stride 14 (step 1) or 5 (step 2)
static int observation_rows(povar_ctx* c, int dim, bool hat, double lambda, int32_t gauge, const int32_t* lm_ids, int32_t n_ids,
                            double* rows_out, int64_t n_rows) {
  CovRequest q;
  q.who = hat ? (dim == 12 ? "povar_observation_hat_pose" : "povar_observation_hat_joint")
              : (dim == 12 ? "povar_observation_covariance_pose" : "povar_observation_covariance_joint");
  if (int rc = q.check(c, lm_ids, n_ids, true)) return rc;
  if (n_rows != q.rows)
    return fail(-1, std::string(q.who) + ": n_rows is " + std::to_string(n_rows) + ", the request produces " + std::to_string(q.rows));
  const size_t stride = !hat ? 4 : with_step(dim, [](auto step) { return (size_t)ObsHatRow<decltype(step)>::STRIDE; });
  q.out = rows_out;
  q.count = stride * (size_t)q.rows;
  CovInverse f{};
  std::optional<TimeScope> ts;
  int rc = cov_inverse(c, dim, q.who, rows_out != nullptr || q.rows == 0, lambda, gauge, POVAR_COV_SOLVER_COORDS, f, ts);
  if (q.over(c, f, q.rows == 0, rc)) return rc;
  const size_t sig_count = (size_t)lm_stride(dim) * (size_t)q.n_out;
  if (int rc2 = cov_buffer(c, c->sc_cov_lm, sig_count, dim)) return rc2;
  if (int rc2 = cov_buffer(c, c->sc_cov_row0, (size_t)q.n_out, dim)) return rc2;
  if (int rc2 = cov_buffer(c, c->sc_cov_obs, q.count, dim)) return rc2;
  if (int rc2 = q.upload_ids(c, dim)) return rc2;
  HIP_TRY(hipMemcpyAsync(c->sc_cov_row0.p, q.row0.data(), (size_t)q.n_out * sizeof(int), hipMemcpyHostToDevice, c->stream));
  // (rows of a landmark without observations do not exist; every other entry is written)
  cov_lm_launch(c, dim, f, q.ids, q.n_out, nullptr, 0, POVAR_COV_SOLVER_COORDS);
  with_step(dim, [&](auto step) {
    typedef decltype(step) S;
    const auto rows_kernel = hat ? obs_hat<S> : obs_cov<S>;
    hipLaunchKernelGGL(rows_kernel, dim3(q.n_out), dim3(256), 0, c->stream, c->d, (const double*)c->ncw.p,
                       (const int*)c->sc_lm_slot0.p, (const int*)c->sc_lm_cnt.p, q.ids, (const int*)c->sc_cov_row0.p,
                       (const double*)c->sc_dense.p, f.ld, (const double*)c->sc_cov_panel.p, (const double*)c->sc_cov_lm.p,
                       c->sc_cov_obs.p);
  });
  HIP_TRY(hipGetLastError());
  std::vector<double> sig(hat ? sig_count : 0);
  if (hat) HIP_TRY(hipMemcpyAsync(sig.data(), c->sc_cov_lm.p, sig_count * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(rows_out, c->sc_cov_obs.p, q.count * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));  // (also: row0 is host memory that goes out of scope)
  // The status judges the factorisation: a leverage that is not finite means C is not; c_* may be non-finite at y2 = 0.  Every
  // entry of a step-2 hat row divides by y2, so there Sigma_l answers, which sums every K_ij of the track the rows are made of.
  for (size_t i = 0; !hat && i < q.count; i += 4)
    if (!std::isfinite(rows_out[i])) return q.all_nan();
  for (size_t i = 0; i < sig.size(); ++i)
    if (!std::isfinite(sig[i])) return q.all_nan();
  cov_done(c, f, 2);
  return 0;
}

// Covariance blocks of parameter pairs: the landmark call's C, then one workgroup per pair in three launches (pair_cc, pair_cl,
// pair_ll of povar_kernels_cov.hpp).  The request is checked and split into three lists before anything runs; every pair goes to
// its kernel in the canonical order with a flag for the transposed store, its block to its place in request order.
static int covariance_blocks(povar_ctx* c, int dim, double lambda, int32_t gauge, int32_t coords, const int32_t* pairs, int32_t n_pairs,
                             double* blocks, int64_t n_out) {
  const std::string who = dim == 12 ? "povar_covariance_blocks_pose" : "povar_covariance_blocks_joint";
  if (int rc = check_ctx(c)) return rc;
  if (n_pairs < 0) return fail(-1, who + ": negative n_pairs");
  if (n_pairs > 0 && !pairs) return fail(-1, who + ": null argument");
  if (coords != POVAR_COV_CAMERA_COORDS && coords != POVAR_COV_SOLVER_COORDS) return fail(-1, who + ": unknown coords");
  const int side[2] = {coords == POVAR_COV_SOLVER_COORDS ? dim : 12, (coords == POVAR_COV_SOLVER_COORDS || dim == 12) ? 3 : 4};
  struct List {
    std::vector<int> items;
    std::vector<long long> off;
    void add(int a, int b, bool tr, long long o) {
      items.insert(items.end(), {a, b, tr ? 1 : 0, 0});
      off.push_back(o);
    }
    int size() const { return (int)off.size(); }
  } list[3];  // camera-camera, camera-landmark, landmark-landmark
  long long total = 0;
  for (int p = 0; p < n_pairs; ++p) {
    const int ka = pairs[4 * (size_t)p], a = pairs[4 * (size_t)p + 1], kb = pairs[4 * (size_t)p + 2], b = pairs[4 * (size_t)p + 3];
    for (int s = 0; s < 2; ++s) {
      const int kind = s ? kb : ka, id = s ? b : a;
      if (kind != POVAR_COV_BLOCK_CAMERA && kind != POVAR_COV_BLOCK_LANDMARK) return fail(-1, who + ": unknown kind");
      if (id < 0 || id >= (kind == POVAR_COV_BLOCK_CAMERA ? c->n_cams : c->n_lms))
        return fail(-1, who + (kind == POVAR_COV_BLOCK_CAMERA ? ": camera id out of range" : ": landmark id out of range"));
    }
    if (ka == POVAR_COV_BLOCK_CAMERA && kb == POVAR_COV_BLOCK_CAMERA) list[0].add(std::max(a, b), std::min(a, b), a < b, total);
    else if (ka == POVAR_COV_BLOCK_LANDMARK && kb == POVAR_COV_BLOCK_LANDMARK) list[2].add(std::min(a, b), std::max(a, b), a > b, total);
    else if (ka == POVAR_COV_BLOCK_CAMERA) list[1].add(a, b, false, total);
    else list[1].add(b, a, true, total);
    total += (long long)side[ka] * side[kb];
  }
  if (n_out != total)
    return fail(-1, who + ": n_out is " + std::to_string(n_out) + ", the request produces " + std::to_string(total));
  CovInverse f{};
  std::optional<TimeScope> ts;
  int rc = cov_inverse(c, dim, who.c_str(), blocks != nullptr || total == 0, lambda, gauge, coords, f, ts);
  if (rc == POVAR_NUMERIC_FAILURE) std::fill(blocks, blocks + total, std::nan(""));
  if (rc == 0 && n_pairs == 0) cov_done(c, f, 1);  // nothing requested: W alone is in place (cov_lauum does not run)
  if (rc != 0 || n_pairs == 0) return rc;
  if (int rc2 = cov_buffer(c, c->sc_cov_pair_out, (size_t)total, dim)) return rc2;
  if (int rc2 = cov_buffer(c, c->sc_cov_pair_items, 4 * (size_t)n_pairs, dim)) return rc2;
  if (int rc2 = cov_buffer(c, c->sc_cov_pair_off, (size_t)n_pairs, dim)) return rc2;
  size_t first[3], at = 0;
  for (int k = 0; k < 3; ++k) {
    first[k] = at;
    if (list[k].size() == 0) continue;
    HIP_TRY(hipMemcpyAsync(c->sc_cov_pair_items.p + 4 * at, list[k].items.data(), list[k].items.size() * sizeof(int),
                           hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->sc_cov_pair_off.p + at, list[k].off.data(), list[k].off.size() * sizeof(long long), hipMemcpyHostToDevice,
                           c->stream));
    at += (size_t)list[k].size();
  }
  const double* M = c->sc_dense.p;
  const double* panel = c->sc_cov_panel.p;
  const int nb = f.N / CH_NB;
  hipLaunchKernelGGL(cov_lauum, dim3((unsigned)(nb * (nb + 1) / 2)), dim3(256), 0, c->stream, c->sc_dense.p, f.ld, c->sc_cov_panel.p, nb);
  with_step(dim, [&](auto step) {
    typedef decltype(step) S;
    auto items = [&](int k) { return reinterpret_cast<const int4*>(c->sc_cov_pair_items.p) + first[k]; };
    auto off = [&](int k) { return (const long long*)c->sc_cov_pair_off.p + first[k]; };
    if (list[0].size())
      hipLaunchKernelGGL(pair_cc<S>, dim3(list[0].size()), dim3(192), 0, c->stream, items(0), off(0), M, f.ld, panel, f.q, f.nq,
                         (const double*)c->sigma.p, (const double*)c->ncw.p, coords, c->sc_cov_pair_out.p);
    if (list[1].size())
      hipLaunchKernelGGL(pair_cl<S>, dim3(list[1].size()), dim3(256), 0, c->stream, c->d, (const double*)c->ncw.p,
                         (const int*)c->sc_lm_slot0.p, (const int*)c->sc_lm_cnt.p, items(1), off(1), M, f.ld, panel, f.q, f.nq, coords,
                         c->sc_cov_pair_out.p);
    if (list[2].size())
      hipLaunchKernelGGL(pair_ll<S>, dim3(list[2].size()), dim3(256), 0, c->stream, c->d, (const double*)c->ncw.p,
                         (const int*)c->sc_lm_slot0.p, (const int*)c->sc_lm_cnt.p, items(2), off(2), M, f.ld, panel, f.q, f.nq, coords,
                         c->sc_cov_pair_out.p);
  });
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(blocks, c->sc_cov_pair_out.p, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));  // (also: the lists are host memory that goes out of scope)
  for (long long i = 0; i < total; ++i)
    if (!std::isfinite(blocks[i])) {
      std::fill(blocks, blocks + total, std::nan(""));
      return POVAR_NUMERIC_FAILURE;
    }
  cov_done(c, f, 2);
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

int povar_camera_covariance_pose(povar_ctx* c, double lambda, int32_t gauge, int32_t coords, double* cov) {
  return camera_covariance(c, 12, lambda, gauge, coords, cov);
}

int povar_camera_covariance_joint(povar_ctx* c, double lambda, int32_t gauge, int32_t coords, double* cov) {
  return camera_covariance(c, 11, lambda, gauge, coords, cov);
}

int povar_landmark_covariance_pose(povar_ctx* c, double lambda, int32_t gauge, int32_t coords, const int32_t* lm_ids, int32_t n_ids,
                                   double* lm_cov, double* cam_cov) {
  return landmark_covariance(c, 12, lambda, gauge, coords, lm_ids, n_ids, lm_cov, cam_cov);
}

int povar_landmark_covariance_joint(povar_ctx* c, double lambda, int32_t gauge, int32_t coords, const int32_t* lm_ids, int32_t n_ids,
                                    double* lm_cov, double* cam_cov) {
  return landmark_covariance(c, 11, lambda, gauge, coords, lm_ids, n_ids, lm_cov, cam_cov);
}

int povar_observation_covariance_pose(povar_ctx* c, double lambda, int32_t gauge, const int32_t* lm_ids, int32_t n_ids, double* obs_cov,
                                      int64_t n_rows) {
  return observation_rows(c, 12, false, lambda, gauge, lm_ids, n_ids, obs_cov, n_rows);
}

int povar_observation_covariance_joint(povar_ctx* c, double lambda, int32_t gauge, const int32_t* lm_ids, int32_t n_ids, double* obs_cov,
                                       int64_t n_rows) {
  return observation_rows(c, 11, false, lambda, gauge, lm_ids, n_ids, obs_cov, n_rows);
}

int povar_observation_hat_pose(povar_ctx* c, double lambda, int32_t gauge, const int32_t* lm_ids, int32_t n_ids, double* rows,
                               int64_t n_rows) {
  return observation_rows(c, 12, true, lambda, gauge, lm_ids, n_ids, rows, n_rows);
}

int povar_observation_hat_joint(povar_ctx* c, double lambda, int32_t gauge, const int32_t* lm_ids, int32_t n_ids, double* rows,
                                int64_t n_rows) {
  return observation_rows(c, 11, true, lambda, gauge, lm_ids, n_ids, rows, n_rows);
}

int povar_covariance_blocks_pose(povar_ctx* c, double lambda, int32_t gauge, int32_t coords, const int32_t* pairs, int32_t n_pairs,
                                 double* blocks, int64_t n_out) {
  return covariance_blocks(c, 12, lambda, gauge, coords, pairs, n_pairs, blocks, n_out);
}

int povar_covariance_blocks_joint(povar_ctx* c, double lambda, int32_t gauge, int32_t coords, const int32_t* pairs, int32_t n_pairs,
                                  double* blocks, int64_t n_out) {
  return covariance_blocks(c, 11, lambda, gauge, coords, pairs, n_pairs, blocks, n_out);
}

int povar_set_cov_inspect(povar_ctx* c, int32_t enable) {
  if (int rc = check_ctx(c)) return rc;
  c->cov_inspect = enable ? 1 : 0;
  return 0;
}

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
