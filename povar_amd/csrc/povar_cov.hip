// povar_cov.hip -- marginal covariance of cameras, landmarks, observations and parameter pairs from CHOLESKY's factor
// (povar_camera_covariance_* / povar_landmark_covariance_* / povar_observation_covariance_* / povar_observation_hat_* /
// povar_covariance_blocks_*; not in the reference).  What a call decides without the device is in cov_plan.hpp.
#include <optional>

#include "povar_ctx.hpp"
#include "povar_kernels_cov.hpp"

namespace {
// a scratch buffer of the covariance calls, grown to `count` doubles and kept (counted in povar_device_bytes); no memory:
// the error of CHOLESKY / RICHOLESKY
template <typename T>
int cov_buffer(povar_ctx* c, DevBuf<T>& buf, size_t count, int dim) {
  const hipError_t e = grow_buffer(c, buf, count);
  if (e == hipErrorOutOfMemory) return no_memory(dim, c->cam_row_n, "covariance scratch", count * sizeof(T));
  HIP_TRY(e);
  return 0;
}

bool all_finite(const double* p, size_t count, size_t stride = 1) {
  for (size_t i = 0; i < count; i += stride)
    if (!std::isfinite(p[i])) return false;
  return true;
}

int lm_stride(int dim) {
  return with_step(dim, [](auto step) { return decltype(step)::LM_STRIDE; });
}
}  // namespace

// What the covariance calls share: the prepared system, the gauge basis, the factorisation of CHOLESKY / RICHOLESKY
// (A = S(lambda), or S0 + Q Q^T in the free gauge), the pivot rule and W = R^-1 in place.
struct CovInverse : DenseDims {
  const double* q = nullptr;  // device: the gauge basis (free gauge), n x nq row-major
  int nq = 0;
};
// 0: W is in the upper block triangle of sc_dense, the scratch panel is allocated and free;  POVAR_NUMERIC_FAILURE: not
// positive definite, or singular beyond the gauge (the caller fills its outputs with NaN);  < 0: an error.  `ts` is the call's
// one solve-stage timing: it opens here, once the system is prepared, and closes when the caller is done.
static int cov_inverse(povar_ctx* c, int dim, double lambda, int32_t gauge, CovInverse& f, std::optional<TimeScope>& ts) {
  if (int rc = prepare_sc(c, dim, lambda)) return rc;
  const size_t nc = c->n_cams;
  static_cast<DenseDims&>(f) = dense_dims(dim, c->cam_row_n / dim);  // (the cameras of the step's map: povar_set_dense_compaction)
  ts.emplace(c, 2);
  c->cov.invalidate();  // (from here on Q, the dense matrix and the panel are rewritten: POVAR_BUF_COV_* wait for CovState::done)
  const bool free_gauge = gauge == POVAR_COV_FREE_GAUGE;
  if (free_gauge) {
    std::vector<double> P(12 * nc), sg(12 * nc), ncw(13 * nc), Q;
    HIP_TRY(hipMemcpyAsync(P.data(), c->cams_lin4.p, 12 * nc * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(sg.data(), c->sigma.p, 12 * nc * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (dim == 11) HIP_TRY(hipMemcpyAsync(ncw.data(), c->ncw.p, 13 * nc * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (!gauge_basis(c->n_cams, dim, P, sg, ncw, Q, f.nq)) return POVAR_NUMERIC_FAILURE;
    if (int rc = cov_buffer(c, c->cov.q, Q.size(), dim)) return rc;
    if (int rc = cov_buffer(c, c->cov.stat, 2, dim)) return rc;
    HIP_TRY(hipMemcpyAsync(c->cov.q.p, Q.data(), Q.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // (Q is pageable host memory that goes out of scope)
    f.q = c->cov.q.p;
  }
  // (the pivot scan belongs to the undamped gauges: the damped mode judges by chol_diag's info alone)
  const bool scan = free_gauge || gauge == POVAR_COV_FIXED_GAUGE;
  if (scan && !free_gauge)
    if (int rc = cov_buffer(c, c->cov.stat, 2, dim)) return rc;
  if (int rc = chol_factor(c, dim, f.q, f.nq, scan ? c->cov.stat.p : nullptr)) return rc;
  c->sc_factor_dim = c->sc_factor_n = 0;  // (R becomes R^-1 below: not the factor POVAR_BUF_SC_FACTOR hands out)
  // every camera fixed in the compacted layout: no matrix, and the answer of the full layout -- whose scan skips every row and
  // whose pivot rule then passes -- is C = 0: the readers of C take exact zeros from the map alone
  if (f.n == 0) return 0;
  int info = 0;
  double st[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(&info, c->sc_info.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (scan) HIP_TRY(hipMemcpyAsync(st, c->cov.stat.p, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (info != 0) return POVAR_NUMERIC_FAILURE;  // not positive definite: CHOLESKY's own rule
  if (scan && !cov_pivots_ok(st[0], st[1])) return POVAR_NUMERIC_FAILURE;
  double* M = c->sc_dense.p;
  const int64_t ld = f.ld;
  if (int rc = cov_buffer(c, c->cov.panel, (size_t)f.N * CH_NB, dim)) return rc;
  double* panel = c->cov.panel.p;
  if (c->cov.inspect) {  // povar_set_cov_inspect: keep the R the inversion starts from (POVAR_BUF_COV_FACTOR)
    if (int rc = cov_buffer(c, c->cov.r, (size_t)f.N * f.N, dim)) return rc;
    HIP_TRY(hipMemcpy2DAsync(c->cov.r.p, (size_t)f.N * sizeof(double), M, (size_t)ld * sizeof(double), (size_t)f.N * sizeof(double),
                             (size_t)f.N, hipMemcpyDeviceToDevice, c->stream));
    c->cov.kept = true;
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
  // fixed cameras: W_kk = 0 on their rows, so C and everything taken from it is zero there (the compacted matrix has no such
  // row: the readers of C take the zeros from the map)
  if (c->n_fixed > 0 && !c->compaction)
    hipLaunchKernelGGL(cov_fix_cameras, dim3(grid_for(f.n, 256)), dim3(256), 0, c->stream, M, ld, f.n, dim, (const uint8_t*)c->fixed_mask.p);
  HIP_TRY(hipGetLastError());
  return 0;
}

// Diagonal blocks of W W^T, less Q_J Q_J^T in the free gauge, in `coords`, into the host's cov (144 n_cams).  Reads the
// upper block triangle of sc_dense only.  POVAR_NUMERIC_FAILURE: a block is not finite.
static int cov_camera_blocks(povar_ctx* c, int dim, const CovInverse& f, int32_t coords, double* cov) {
  const size_t out_count = 144 * (size_t)c->n_cams;
  if (int rc = cov_buffer(c, c->cov.blocks, out_count, dim)) return rc;
  const double* M = c->sc_dense.p;
  double* blocks = c->cov.blocks.p;
  HIP_TRY(hipMemsetAsync(blocks, 0, out_count * sizeof(double), c->stream));
  with_step(dim, [&](auto step) {
    constexpr int DIM = decltype(step)::DIM;
    hipLaunchKernelGGL(cov_gram<DIM>, dim3(c->n_cams), dim3(256), 0, c->stream, M, f.ld, f.n, (const int*)c->cam_row.p, blocks);
    hipLaunchKernelGGL(cov_finish<DIM>, dim3(c->n_cams), dim3(256), 0, c->stream, blocks, f.q, f.nq,
                       (const double*)c->sigma.p, (const double*)c->ncw.p, coords);
  });
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(cov, blocks, out_count * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return all_finite(cov, out_count) ? 0 : POVAR_NUMERIC_FAILURE;
}

// One covariance call, once its request is checked.  The families differ in the description alone:
struct CovCall {
  const char* who;
  struct { double* p; size_t count; } out[2];  // the outputs: NaN on a numeric failure (the first is required unless it is empty)
  bool empty;    // nothing beyond W and the camera blocks is requested: W alone is in place (kind 1; cov_lauum does not run)
  double* cam;   // the camera blocks first, into here (null: not wanted)
};
// The mode rules, W (cov_inverse), the camera blocks, then -- unless the request is empty -- C = W W^T off the diagonal too
// (cov_lauum) and the family's own part: stage(f) grows its buffers, uploads and enqueues its kernels and the copy-back (an error:
// its return value), judge() is the host's finite rule on what came back.
template <class Stage, class Judge>
static int cov_call(povar_ctx* c, int dim, const CovCall& q, double lambda, int32_t gauge, int32_t coords, Stage stage, Judge judge) {
  if (!q.out[0].p && q.out[0].count > 0) return fail(-1, std::string(q.who) + ": null argument");
  // (the set as the caller left it: the preparation below is the one that installs it)
  const bool any_fixed = std::find(c->fixed_next.begin(), c->fixed_next.end(), (uint8_t)1) != c->fixed_next.end();
  std::string err;
  if (!cov_check_mode(q.who, gauge, coords, lambda, any_fixed, &err)) return fail(-1, err);
  const auto all_nan = [&] {
    for (const auto& o : q.out)
      if (o.p) std::fill(o.p, o.p + o.count, std::nan(""));
    return POVAR_NUMERIC_FAILURE;
  };
  CovInverse f{};
  std::optional<TimeScope> ts;
  int rc = cov_inverse(c, dim, lambda, gauge, f, ts);
  if (rc == 0 && q.cam) rc = cov_camera_blocks(c, dim, f, coords, q.cam);
  if (rc != 0) return rc == POVAR_NUMERIC_FAILURE ? all_nan() : rc;
  if (!q.empty) {
    const int nb = f.N / CH_NB;
    if (nb > 0)
      hipLaunchKernelGGL(cov_lauum, dim3((unsigned)(nb * (nb + 1) / 2)), dim3(256), 0, c->stream, c->sc_dense.p, f.ld, c->cov.panel.p, nb);
    if (int rc2 = stage(f)) return rc2;
    HIP_TRY(hipStreamSynchronize(c->stream));  // (also: the request's lists are host memory that goes out of scope)
    if (!judge()) return all_nan();
  }
  if (f.n > 0) c->cov.done(q.empty ? 1 : 2, f.n, f.nq);  // (no matrix: nothing for POVAR_BUF_COV_* to hand out)
  return 0;
}

// Diagonal blocks of S(lambda)^-1 (POVAR_COV_DAMPED) or of the pseudo-inverse S(0)^+ = (S0 + Q Q^T)^-1 - Q Q^T
// (POVAR_COV_FREE_GAUGE), through the factorisation of CHOLESKY / RICHOLESKY: A = R^T R, W = R^-1 in place, blocks of W W^T.
static int camera_covariance(povar_ctx* c, int dim, double lambda, int32_t gauge, int32_t coords, double* cov) {
  if (int rc = check_ctx(c)) return rc;
  const CovCall q{dim == 12 ? "povar_camera_covariance_pose" : "povar_camera_covariance_joint", {{cov, 144 * (size_t)c->n_cams}, {}}, true, cov};
  return cov_call(c, dim, q, lambda, gauge, coords, [](const CovInverse&) { return 0; }, [] { return true; });
}

// the blocks of the n_out requested landmarks (ids null: all of them) into cov.lm (lm_cov), from C
static void cov_lm_launch(povar_ctx* c, int dim, const CovInverse& f, const int* ids, int n_out, const double* q, int nq, int32_t coords) {
  with_step(dim, [&](auto step) {
    hipLaunchKernelGGL(lm_cov<decltype(step)>, dim3(n_out), dim3(256), 0, c->stream, c->d, (const double*)c->ncw.p,
                       (const int*)c->sc_lm_slot0.p, (const int*)c->sc_lm_cnt.p, ids, (const double*)c->sc_dense.p, f.ld,
                       (const double*)c->cov.panel.p, (const int*)c->cam_row.p, q, nq, coords, c->cov.lm.p);
  });
}

// the device copy of lm_ids (null: all landmarks) into ids (lm_ids is the caller's memory: the call synchronises the stream before
// it returns)
static int cov_upload_ids(povar_ctx* c, int dim, const int32_t* lm_ids, int n_out, const int*& ids) {
  ids = nullptr;
  if (!lm_ids) return 0;
  if (int rc = cov_buffer(c, c->cov.ids, (size_t)n_out, dim)) return rc;
  HIP_TRY(hipMemcpyAsync(c->cov.ids.p, lm_ids, (size_t)n_out * sizeof(int), hipMemcpyHostToDevice, c->stream));
  ids = c->cov.ids.p;
  return 0;
}

// Landmark blocks Sigma_l = Hll^-1 + F_l^T C F_l of the requested landmarks (and, on request, the camera blocks of the
// same C): the camera call's W, then C and the per-landmark contraction (lm_cov).
static int landmark_covariance(povar_ctx* c, int dim, double lambda, int32_t gauge, int32_t coords, const int32_t* lm_ids,
                               int32_t n_ids, double* lm_cov_out, double* cam_cov) {
  if (int rc = check_ctx(c)) return rc;
  const char* who = dim == 12 ? "povar_landmark_covariance_pose" : "povar_landmark_covariance_joint";
  CovLmRequest r;
  std::string err;
  if (!cov_lm_request(c->n_lms, c->lm_off.data(), lm_ids, n_ids, false, r, &err)) return fail(-1, std::string(who) + ": " + err);
  const size_t count = (size_t)lm_stride(dim) * (size_t)r.n_out;
  const CovCall q{who, {{lm_cov_out, count}, {cam_cov, 144 * (size_t)c->n_cams}}, r.n_out == 0, cam_cov};
  const auto stage = [&](const CovInverse& f) {
    const int* ids;
    if (int rc = cov_buffer(c, c->cov.lm, count, dim)) return rc;
    if (int rc = cov_upload_ids(c, dim, lm_ids, r.n_out, ids)) return rc;
    cov_lm_launch(c, dim, f, ids, r.n_out, f.q, f.nq, coords);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(lm_cov_out, c->cov.lm.p, count * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return 0;
  };
  return cov_call(c, dim, q, lambda, gauge, coords, stage, [&] { return all_finite(lm_cov_out, count); });
}

// Per-observation rows of the requested landmarks' observations: the landmark call's C, Sigma_l without the gauge correction
// (lm_cov with nq = 0 in solver coordinates, into cov.lm) and the per-landmark walk obs_rows, which reads no Q: the gauge part
// of C cancels in J C J^T only if no term carries the correction.  The two calls differ in the row alone:
//   hat = false  povar_observation_covariance_*: (h, c_uu, c_uv, c_vv), obs_cov, stride 4
//   hat = true   povar_observation_hat_*: r_i and the upper triangle of P_ii, obs_hat, stride 14 (step 1) or 5 (step 2)
static int observation_rows(povar_ctx* c, int dim, bool hat, double lambda, int32_t gauge, const int32_t* lm_ids, int32_t n_ids,
                            double* rows_out, int64_t n_rows) {
  if (int rc = check_ctx(c)) return rc;
  const std::string who = hat ? (dim == 12 ? "povar_observation_hat_pose" : "povar_observation_hat_joint")
                              : (dim == 12 ? "povar_observation_covariance_pose" : "povar_observation_covariance_joint");
  CovLmRequest r;
  std::string err;
  if (!cov_lm_request(c->n_lms, c->lm_off.data(), lm_ids, n_ids, true, r, &err)) return fail(-1, who + ": " + err);
  if (n_rows != r.rows) return fail(-1, who + ": n_rows is " + std::to_string(n_rows) + ", the request produces " + std::to_string(r.rows));
  const size_t stride = !hat ? 4 : with_step(dim, [](auto step) { return (size_t)ObsHatRow<decltype(step)>::STRIDE; });
  const size_t count = stride * (size_t)r.rows, sig_count = (size_t)lm_stride(dim) * (size_t)r.n_out;
  const CovCall q{who.c_str(), {{rows_out, count}, {}}, r.rows == 0, nullptr};
  std::vector<double> sig(hat ? sig_count : 0);
  const auto stage = [&](const CovInverse& f) {
    const int* ids;
    if (int rc = cov_buffer(c, c->cov.lm, sig_count, dim)) return rc;
    if (int rc = cov_buffer(c, c->cov.row0, (size_t)r.n_out, dim)) return rc;
    if (int rc = cov_buffer(c, c->cov.obs, count, dim)) return rc;
    if (int rc = cov_upload_ids(c, dim, lm_ids, r.n_out, ids)) return rc;
    HIP_TRY(hipMemcpyAsync(c->cov.row0.p, r.row0.data(), (size_t)r.n_out * sizeof(int), hipMemcpyHostToDevice, c->stream));
    // (rows of a landmark without observations do not exist; every other entry is written)
    cov_lm_launch(c, dim, f, ids, r.n_out, nullptr, 0, POVAR_COV_SOLVER_COORDS);
    with_step(dim, [&](auto step) {
      typedef decltype(step) S;
      const auto rows_kernel = hat ? obs_hat<S> : obs_cov<S>;
      hipLaunchKernelGGL(rows_kernel, dim3(r.n_out), dim3(256), 0, c->stream, c->d, (const double*)c->ncw.p,
                         (const int*)c->sc_lm_slot0.p, (const int*)c->sc_lm_cnt.p, ids, (const int*)c->cov.row0.p,
                         (const double*)c->sc_dense.p, f.ld, (const double*)c->cov.panel.p, (const int*)c->cam_row.p,
                         (const double*)c->cov.lm.p, c->cov.obs.p);
    });
    HIP_TRY(hipGetLastError());
    if (hat) HIP_TRY(hipMemcpyAsync(sig.data(), c->cov.lm.p, sig_count * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(rows_out, c->cov.obs.p, count * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return 0;
  };
  // The status judges the factorisation: a leverage that is not finite means C is not; c_* may be non-finite at y2 = 0.  Every
  // entry of a step-2 hat row divides by y2, so there Sigma_l answers, which sums every K_ij of the track the rows are made of.
  const auto judge = [&] { return hat ? all_finite(sig.data(), sig.size()) : all_finite(rows_out, count, 4); };
  return cov_call(c, dim, q, lambda, gauge, POVAR_COV_SOLVER_COORDS, stage, judge);
}

// Covariance blocks of parameter pairs: the landmark call's C, then one workgroup per pair in three launches (pair_cc, pair_cl,
// pair_ll of povar_kernels_cov.hpp) on the three lists of the request (cov_plan.hpp: cov_pair_request).
static int covariance_blocks(povar_ctx* c, int dim, double lambda, int32_t gauge, int32_t coords, const int32_t* pairs, int32_t n_pairs,
                             double* blocks, int64_t n_out) {
  if (int rc = check_ctx(c)) return rc;
  const std::string who = dim == 12 ? "povar_covariance_blocks_pose" : "povar_covariance_blocks_joint";
  CovPairRequest r;
  std::string err;
  if (!cov_pair_request(dim, coords, c->n_cams, c->n_lms, pairs, n_pairs, r, &err)) return fail(-1, who + ": " + err);
  if (n_out != r.total) return fail(-1, who + ": n_out is " + std::to_string(n_out) + ", the request produces " + std::to_string(r.total));
  const size_t total = (size_t)r.total;
  const CovCall q{who.c_str(), {{blocks, total}, {}}, n_pairs == 0, nullptr};
  const auto stage = [&](const CovInverse& f) {
    if (int rc = cov_buffer(c, c->cov.pair_out, total, dim)) return rc;
    if (int rc = cov_buffer(c, c->cov.pair_items, 4 * (size_t)n_pairs, dim)) return rc;
    if (int rc = cov_buffer(c, c->cov.pair_off, (size_t)n_pairs, dim)) return rc;
    size_t first[3], at = 0;
    for (int k = 0; k < 3; ++k) {
      const auto& l = r.list[k];
      first[k] = at;
      if (l.size() == 0) continue;
      HIP_TRY(hipMemcpyAsync(c->cov.pair_items.p + 4 * at, l.items.data(), l.items.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
      HIP_TRY(hipMemcpyAsync(c->cov.pair_off.p + at, l.off.data(), l.off.size() * sizeof(long long), hipMemcpyHostToDevice, c->stream));
      at += (size_t)l.size();
    }
    const double* M = c->sc_dense.p;
    const double* panel = c->cov.panel.p;
    const int* rows = c->cam_row.p;
    with_step(dim, [&](auto step) {
      typedef decltype(step) S;
      auto items = [&](int k) { return reinterpret_cast<const int4*>(c->cov.pair_items.p) + first[k]; };
      auto off = [&](int k) { return (const long long*)c->cov.pair_off.p + first[k]; };
      if (r.list[0].size())
        hipLaunchKernelGGL(pair_cc<S>, dim3(r.list[0].size()), dim3(192), 0, c->stream, items(0), off(0), M, f.ld, panel, rows, f.q, f.nq,
                           (const double*)c->sigma.p, (const double*)c->ncw.p, coords, c->cov.pair_out.p);
      if (r.list[1].size())
        hipLaunchKernelGGL(pair_cl<S>, dim3(r.list[1].size()), dim3(256), 0, c->stream, c->d, (const double*)c->ncw.p,
                           (const int*)c->sc_lm_slot0.p, (const int*)c->sc_lm_cnt.p, items(1), off(1), M, f.ld, panel, rows, f.q, f.nq, coords,
                           c->cov.pair_out.p);
      if (r.list[2].size())
        hipLaunchKernelGGL(pair_ll<S>, dim3(r.list[2].size()), dim3(256), 0, c->stream, c->d, (const double*)c->ncw.p,
                           (const int*)c->sc_lm_slot0.p, (const int*)c->sc_lm_cnt.p, items(2), off(2), M, f.ld, panel, rows, f.q, f.nq, coords,
                           c->cov.pair_out.p);
    });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(blocks, c->cov.pair_out.p, total * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return 0;
  };
  return cov_call(c, dim, q, lambda, gauge, coords, stage, [&] { return all_finite(blocks, total); });
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
  c->cov.inspect = enable ? 1 : 0;
  return 0;
}

}  // extern "C"
