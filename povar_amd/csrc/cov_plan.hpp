// cov_plan.hpp -- what a covariance call (povar_cov.hip) decides before it touches the device: the argument rules of gauge, lambda,
// coords and the fixed set, the landmark request (ids to rows), the pair request (pairs to three canonical lists), the gauge basis
// of the free gauge and the pivot rule -- and the layout of the dense matrix they share with CHOLESKY / RICHOLESKY (cam_row_map;
// tests/cpp/cam_row_map_check.cpp).  Host-only plain C++17 (no HIP, no context): tests/cpp/cov_plan_check.cpp holds every rule
// to a table on the CPU.  The request functions return false with the message in *err, without the caller's name in front.
#pragma once
#include "../../include/povar_hip.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

namespace povar {

// The rules of (gauge, coords, lambda) and the fixed set (any_fixed: the set as the caller left it), in the order the caller sees
// them; after "null argument", before anything is prepared.  false: *err is the whole message.
inline bool cov_check_mode(const char* who, int32_t gauge, int32_t coords, double lambda, bool any_fixed, std::string* err) {
  const auto no = [&](const char* what) {
    *err = std::string(who) + what;
    return false;
  };
  if (gauge != POVAR_COV_FREE_GAUGE && gauge != POVAR_COV_DAMPED && gauge != POVAR_COV_FIXED_GAUGE) return no(": unknown gauge");
  if (coords != POVAR_COV_CAMERA_COORDS && coords != POVAR_COV_SOLVER_COORDS) return no(": unknown coords");
  if (gauge == POVAR_COV_FREE_GAUGE && lambda != 0.0) return no(": POVAR_COV_FREE_GAUGE takes lambda = 0");
  if (gauge == POVAR_COV_DAMPED && !(lambda > 0.0)) return no(": POVAR_COV_DAMPED takes lambda > 0");
  if (gauge == POVAR_COV_FIXED_GAUGE && lambda != 0.0) return no(": POVAR_COV_FIXED_GAUGE takes lambda = 0");
  if (gauge == POVAR_COV_FIXED_GAUGE && !any_fixed) return no(": POVAR_COV_FIXED_GAUGE needs fixed cameras (povar_set_fixed_cameras)");
  if (gauge == POVAR_COV_FREE_GAUGE && any_fixed)
    return no(": POVAR_COV_FREE_GAUGE with fixed cameras: the gauge they fix is POVAR_COV_FIXED_GAUGE");
  return true;
}

// Layout of the dense matrix of CHOLESKY / RICHOLESKY and the covariance calls (povar_set_dense_compaction): rows[c] is the first
// of the dim rows of camera c, -1 for a camera that is not in the matrix; the return value is the row count n.
//   mode 0: every camera at dim c, fixed ones included (they become identity rows), n = dim n_cams;
//   mode 1: the free cameras (fixed[c] == 0) alone, in ascending camera id, n = dim (n_cams - |F|).  No fixed camera: mode 0's map.
inline int cam_row_map(const uint8_t* fixed, int n_cams, int dim, int mode, std::vector<int32_t>& rows) {
  rows.assign((size_t)std::max(n_cams, 0), -1);
  int n = 0;
  for (int c = 0; c < n_cams; ++c) {
    if (mode == 1 && fixed[c]) continue;
    rows[(size_t)c] = n;
    n += dim;
  }
  return n;
}

// A request of the landmark and observation calls: which landmarks (lm_ids null: all of them)
struct CovLmRequest {
  int n_out = 0;
  std::vector<int> row0;  // observation calls: the first row of every requested landmark, and the number of rows
  int64_t rows = 0;
};
// n_out and the id check; with_rows: row0 and rows in the same walk (row0 is an int: a landmark that would start past 2^31 is refused)
inline bool cov_lm_request(int n_lms, const int* lm_off, const int32_t* lm_ids, int32_t n_ids, bool with_rows, CovLmRequest& r,
                           std::string* err) {
  r = CovLmRequest();
  r.n_out = lm_ids ? n_ids : n_lms;
  if (r.n_out < 0) return *err = "negative n_ids", false;
  if (with_rows) r.row0.resize((size_t)r.n_out);
  for (int i = 0; (lm_ids || with_rows) && i < r.n_out; ++i) {
    const int l = lm_ids ? lm_ids[i] : i;
    if (l < 0 || l >= n_lms) return *err = "landmark id out of range", false;
    if (!with_rows) continue;
    if (r.rows > INT32_MAX) return *err = "more than 2^31 rows requested", false;
    r.row0[i] = (int)r.rows;
    r.rows += (int64_t)lm_off[l + 1] - lm_off[l];
  }
  return true;
}

// A request of the pair calls, checked in full and split into three lists before anything runs: every pair goes to its kernel
// in the canonical order with a flag for the transposed store, its block to its place (off) in request order.
struct CovPairRequest {
  struct List {
    std::vector<int> items;  // (a, b, transposed, -) per pair
    std::vector<long long> off;
    void add(int a, int b, bool tr, long long o) {
      items.insert(items.end(), {a, b, tr ? 1 : 0, 0});
      off.push_back(o);
    }
    int size() const { return (int)off.size(); }
  } list[3];  // camera-camera, camera-landmark, landmark-landmark
  long long total = 0;
};
inline bool cov_pair_request(int dim, int32_t coords, int n_cams, int n_lms, const int32_t* pairs, int32_t n_pairs, CovPairRequest& r,
                             std::string* err) {
  r = CovPairRequest();
  if (n_pairs < 0) return *err = "negative n_pairs", false;
  if (n_pairs > 0 && !pairs) return *err = "null argument", false;
  if (coords != POVAR_COV_CAMERA_COORDS && coords != POVAR_COV_SOLVER_COORDS) return *err = "unknown coords", false;
  const int side[2] = {coords == POVAR_COV_SOLVER_COORDS ? dim : 12, (coords == POVAR_COV_SOLVER_COORDS || dim == 12) ? 3 : 4};
  for (int p = 0; p < n_pairs; ++p) {
    const int ka = pairs[4 * (size_t)p], a = pairs[4 * (size_t)p + 1], kb = pairs[4 * (size_t)p + 2], b = pairs[4 * (size_t)p + 3];
    for (int s = 0; s < 2; ++s) {
      const int kind = s ? kb : ka, id = s ? b : a;
      if (kind != POVAR_COV_BLOCK_CAMERA && kind != POVAR_COV_BLOCK_LANDMARK) return *err = "unknown kind", false;
      if (id < 0 || id >= (kind == POVAR_COV_BLOCK_CAMERA ? n_cams : n_lms))
        return *err = kind == POVAR_COV_BLOCK_CAMERA ? "camera id out of range" : "landmark id out of range", false;
    }
    if (ka == POVAR_COV_BLOCK_CAMERA && kb == POVAR_COV_BLOCK_CAMERA) r.list[0].add(std::max(a, b), std::min(a, b), a < b, r.total);
    else if (ka == POVAR_COV_BLOCK_LANDMARK && kb == POVAR_COV_BLOCK_LANDMARK) r.list[2].add(std::min(a, b), std::max(a, b), a > b, r.total);
    else if (ka == POVAR_COV_BLOCK_CAMERA) r.list[1].add(a, b, false, r.total);
    else r.list[1].add(b, a, true, r.total);
    r.total += (long long)side[ka] * side[kb];
  }
  return true;
}

// Orthonormal basis Q (n x nq, row-major) of the gauge null space of the undamped reduced system, in the solver's
// Jacobi-scaled coordinates, from the linearisation point P_c, sigma_c and the reflectors (w, beta):
//   step 1 (dim 12, nq 12): the affine gauge X -> A X that keeps the last homogeneous coordinate: generators
//           G = e_i e_j^T, i < 3:  v_c = vec(-P_c G) / sigma_c;
//   step 2 (dim 11, nq 15): the projective gauge, generators (i, j) != (3, 3), the per-camera scale absorbed: with
//           g = vec(-P_c G), h0 = the reflector's first column, a = -(h0 . g / sigma_c) / (h0 . P_c / sigma_c):
//           x_c = N_c^T ((g + a P_c) / sigma_c).
// Orthonormalised by twice-applied modified Gram-Schmidt in fp64.  false: the columns are numerically dependent.
inline bool gauge_basis(int n_cams, int dim, const std::vector<double>& P, const std::vector<double>& sg, const std::vector<double>& ncw,
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

// The pivot rule of the undamped gauges on (max_k A_kk, min_k R_kk^2) (fixed gauge: on S_ff(0), whose fixed cameras must have taken
// the whole gauge): a gauge-only system keeps pivots of the order of its smallest eigenvalue; further degeneracy leaves rounding
// noise of the order u max A_kk: the threshold sqrt(u) max A_kk sits in the gap
inline bool cov_pivots_ok(double max_akk, double min_rkk2) {
  const double thr = std::sqrt(std::ldexp(1.0, -53)) * max_akk;
  return min_rkk2 >= thr;
}

}  // namespace povar
