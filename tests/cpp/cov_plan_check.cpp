// Host-only check of what a covariance call decides before it touches the device (povar_amd/csrc/cov_plan.hpp): the mode rules, the
// landmark request, the pair request and the gauge basis.  Plain C++: no HIP, no library, no device.  The expected values are
// written down here from the statement of the calls in include/povar_hip.h and DESIGN.md, never taken from the functions under
// test.  Without arguments: checks A to C, "cov_plan_check: ok" and exit status 0, or every mismatch and 1.
//   cov_plan_check gauge FILE   FILE: dim n_cams, then P [12 n_cams], sigma [12 n_cams], (w, beta) [13 n_cams] (step 1: unread).
//                               Prints "dependent", or "nq <nq>" and the n rows of Q (tests/test_host_cov_plan.py, check D).
#include <climits>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../povar_amd/csrc/cov_plan.hpp"

using namespace povar;

static int g_bad = 0;
static void expect(bool ok, const std::string& what) {
  if (ok) return;
  std::printf("MISMATCH %s\n", what.c_str());
  ++g_bad;
}

// ---- A: (gauge, coords, lambda, fixed set) -> the first rule that fails.  include/povar_hip.h: FREE_GAUGE: lambda must be 0, and
// with fixed cameras an argument error; DAMPED: lambda > 0, any fixed set; FIXED_GAUGE: lambda must be 0 and F non-empty.  Where two
// rules fail: the two enums first (gauge, then coords), then the gauge's own lambda rule, then its rule on the fixed set.
static void check_mode() {
  const char* FREE_L = "W: POVAR_COV_FREE_GAUGE takes lambda = 0";
  const char* FREE_F = "W: POVAR_COV_FREE_GAUGE with fixed cameras: the gauge they fix is POVAR_COV_FIXED_GAUGE";
  const char* DAMP_L = "W: POVAR_COV_DAMPED takes lambda > 0";
  const char* FIX_L = "W: POVAR_COV_FIXED_GAUGE takes lambda = 0";
  const char* FIX_F = "W: POVAR_COV_FIXED_GAUGE needs fixed cameras (povar_set_fixed_cameras)";
  const double lambdas[3] = {0.0, 1e-3, -1.0};
  // [gauge 0..2][lambda 0, 1e-3, -1][no camera fixed, some fixed], for a known coords
  const char* table[3][3][2] = {
      {{"ok", FREE_F}, {FREE_L, FREE_L}, {FREE_L, FREE_L}},
      {{DAMP_L, DAMP_L}, {"ok", "ok"}, {DAMP_L, DAMP_L}},
      {{FIX_F, "ok"}, {FIX_L, FIX_L}, {FIX_L, FIX_L}},
  };
  int cases = 0;
  for (int gauge = -1; gauge <= 3; ++gauge)
    for (int coords = -1; coords <= 2; ++coords)
      for (int li = 0; li < 3; ++li)
        for (int fx = 0; fx < 2; ++fx, ++cases) {
          const char* want = gauge < 0 || gauge > 2 ? "W: unknown gauge" : coords < 0 || coords > 1 ? "W: unknown coords" : table[gauge][li][fx];
          std::string err = "ok";
          const bool ok = cov_check_mode("W", gauge, coords, lambdas[li], fx != 0, &err);
          expect(ok == !std::strcmp(want, "ok") && err == want, "mode gauge " + std::to_string(gauge) + " coords " + std::to_string(coords) +
                                                                    " lambda " + std::to_string(lambdas[li]) + " fixed " + std::to_string(fx) +
                                                                    ": got '" + err + "', want '" + want + "'");
        }
  expect(cases == 120, "mode: 120 cases");
  std::string err;  // (a NaN lambda is no lambda of any gauge)
  expect(!cov_check_mode("W", POVAR_COV_DAMPED, POVAR_COV_SOLVER_COORDS, std::nan(""), false, &err) && err == DAMP_L, "mode: DAMPED, NaN");
}

// ---- B: the landmark request on five landmarks with 3, 0, 4, 1, 4 observations
static void lm_case(const char* name, int n_lms, const std::vector<int>& lm_off, const int32_t* ids, int32_t n_ids, bool with_rows,
                    const char* want_err, int want_n_out, const std::vector<int>& want_row0, int64_t want_rows) {
  CovLmRequest r;
  std::string err = "ok";
  const bool ok = cov_lm_request(n_lms, lm_off.data(), ids, n_ids, with_rows, r, &err);
  if (want_err) return expect(!ok && err == want_err, std::string("lm ") + name + ": got '" + err + "', want '" + want_err + "'");
  expect(ok && r.n_out == want_n_out && r.row0 == want_row0 && r.rows == want_rows,
         std::string("lm ") + name + ": '" + err + "' n_out " + std::to_string(r.n_out) + " rows " + std::to_string((long long)r.rows));
}
static void check_lm_request() {
  const std::vector<int> off = {0, 3, 3, 7, 8, 12};
  const int32_t none[1] = {0}, a[3] = {4, 0, 0}, two[1] = {2}, empty_track[1] = {1}, around[3] = {1, 2, 1}, neg[1] = {-1}, past[1] = {5}, mixed[2] = {1, 5};
  lm_case("all, rows", 5, off, nullptr, 0, true, nullptr, 5, {0, 3, 3, 7, 8}, 12);
  lm_case("all, rows, n_ids unread", 5, off, nullptr, -7, true, nullptr, 5, {0, 3, 3, 7, 8}, 12);
  lm_case("all, no rows", 5, off, nullptr, 0, false, nullptr, 5, {}, 0);
  lm_case("[], rows", 5, off, none, 0, true, nullptr, 0, {}, 0);
  lm_case("[], no rows", 5, off, none, 0, false, nullptr, 0, {}, 0);
  lm_case("[4, 0, 0], rows", 5, off, a, 3, true, nullptr, 3, {0, 4, 7}, 10);
  lm_case("[4, 0, 0], no rows", 5, off, a, 3, false, nullptr, 3, {}, 0);
  lm_case("[2] alone, rows", 5, off, two, 1, true, nullptr, 1, {0}, 4);
  lm_case("[1] (no observation), rows", 5, off, empty_track, 1, true, nullptr, 1, {0}, 0);
  lm_case("[1, 2, 1], rows", 5, off, around, 3, true, nullptr, 3, {0, 0, 4}, 4);
  for (int with_rows = 0; with_rows < 2; ++with_rows) {
    lm_case("[-1]", 5, off, neg, 1, with_rows != 0, "landmark id out of range", 0, {}, 0);
    lm_case("[5]", 5, off, past, 1, with_rows != 0, "landmark id out of range", 0, {}, 0);
    lm_case("[1, 5]", 5, off, mixed, 2, with_rows != 0, "landmark id out of range", 0, {}, 0);
    lm_case("n_ids -1", 5, off, a, -1, with_rows != 0, "negative n_ids", 0, {}, 0);
  }
  // the cap: row0 is an int, so a landmark may not START past 2^31 - 1.  One landmark of 2^31 rows (two offsets, no allocation):
  // alone it is row 0 of a request of 2^31 rows; asked for twice, the second would start at 2^31
  const std::vector<int> huge = {-1, INT32_MAX};
  const int32_t once[1] = {0}, twice[2] = {0, 0};
  lm_case("2^31 rows, once", 1, huge, once, 1, true, nullptr, 1, {0}, (int64_t)1 << 31);
  lm_case("2^31 rows, twice", 1, huge, twice, 2, true, "more than 2^31 rows requested", 0, {}, 0);
  lm_case("2^31 rows, twice, no rows", 1, huge, twice, 2, false, nullptr, 2, {}, 0);
  const std::vector<int> big = {0, INT32_MAX};  // 2^31 - 1 rows: the second still starts inside, a third does not
  const int32_t thrice[3] = {0, 0, 0};
  lm_case("2^31 - 1 rows, twice", 1, big, twice, 2, true, nullptr, 2, {0, INT32_MAX}, 2 * (int64_t)INT32_MAX);
  lm_case("2^31 - 1 rows, thrice", 1, big, thrice, 3, true, "more than 2^31 rows requested", 0, {}, 0);
}

// ---- C: the pair request on 4 cameras and 5 landmarks.  A camera has 12 (pose) or 11 (joint) solver coordinates and 12 of its
// own; a landmark 3 solver coordinates and 3 (pose) or 4 (joint) of its own (include/povar_hip.h).  Canonical order: camera-camera
// (larger, smaller), landmark-landmark (smaller, larger), camera-landmark (camera, landmark); tr: the request had the other order.
static void check_pair_request() {
  const int C = POVAR_COV_BLOCK_CAMERA, L = POVAR_COV_BLOCK_LANDMARK;
  const int32_t req[8 * 4] = {C, 1, C, 3,  C, 3, C, 1,  C, 2, C, 2,  L, 0, L, 4,  L, 4, L, 0,  L, 2, L, 2,  C, 0, L, 3,  L, 1, C, 2};
  struct Want {
    int dim, coords;
    long long off[8], total;  // where the eight blocks start, in request order
  } const want[4] = {
      {12, POVAR_COV_SOLVER_COORDS, {0, 144, 288, 432, 441, 450, 459, 495}, 531},  // camera 12, landmark 3
      {12, POVAR_COV_CAMERA_COORDS, {0, 144, 288, 432, 441, 450, 459, 495}, 531},  // camera 12, landmark 3
      {11, POVAR_COV_SOLVER_COORDS, {0, 121, 242, 363, 372, 381, 390, 423}, 456},  // camera 11, landmark 3
      {11, POVAR_COV_CAMERA_COORDS, {0, 144, 288, 432, 448, 464, 480, 528}, 576},  // camera 12, landmark 4
  };
  for (const Want& w : want) {
    const std::string name = "pairs dim " + std::to_string(w.dim) + " coords " + std::to_string(w.coords);
    CovPairRequest r;
    std::string err = "ok";
    expect(cov_pair_request(w.dim, w.coords, 4, 5, req, 8, r, &err), name + ": " + err);
    // camera-camera: pairs 0, 1, 2;  camera-landmark: pairs 6, 7;  landmark-landmark: pairs 3, 4, 5
    expect(r.list[0].items == std::vector<int>{3, 1, 1, 0, 3, 1, 0, 0, 2, 2, 0, 0}, name + ": camera-camera items");
    expect(r.list[0].off == std::vector<long long>{w.off[0], w.off[1], w.off[2]}, name + ": camera-camera offsets");
    expect(r.list[1].items == std::vector<int>{0, 3, 0, 0, 2, 1, 1, 0}, name + ": camera-landmark items");
    expect(r.list[1].off == std::vector<long long>{w.off[6], w.off[7]}, name + ": camera-landmark offsets");
    expect(r.list[2].items == std::vector<int>{0, 4, 0, 0, 0, 4, 1, 0, 2, 2, 0, 0}, name + ": landmark-landmark items");
    expect(r.list[2].off == std::vector<long long>{w.off[3], w.off[4], w.off[5]}, name + ": landmark-landmark offsets");
    expect(r.list[0].size() == 3 && r.list[1].size() == 2 && r.list[2].size() == 3, name + ": list sizes");
    expect(r.total == w.total, name + ": total " + std::to_string(r.total));
  }
  const auto refused = [&](const char* name, int32_t coords, const int32_t* pairs, int32_t n_pairs, const char* want_err) {
    for (int dim = 11; dim <= 12; ++dim) {
      CovPairRequest r;
      std::string err = "ok";
      const bool ok = cov_pair_request(dim, coords, 4, 5, pairs, n_pairs, r, &err);
      expect(!ok && err == want_err, std::string("pairs ") + name + ": got '" + err + "', want '" + want_err + "'");
    }
  };
  const int32_t kind_a[4] = {2, 0, C, 0}, kind_b[4] = {L, 0, -1, 0}, cam_hi[4] = {C, 4, L, 0}, cam_lo[4] = {L, 0, C, -1}, lm_hi[4] = {L, 5, C, 0},
                lm_lo[4] = {C, 0, L, -1}, a_first[4] = {C, 9, 7, 0}, later[8] = {C, 0, C, 1, L, 0, L, 5};
  refused("negative n_pairs", POVAR_COV_SOLVER_COORDS, req, -1, "negative n_pairs");
  refused("null pairs", POVAR_COV_SOLVER_COORDS, nullptr, 1, "null argument");
  refused("coords 2", 2, req, 8, "unknown coords");
  refused("coords -1 before the kinds", -1, kind_a, 1, "unknown coords");
  refused("negative n_pairs before null and coords", 2, nullptr, -1, "negative n_pairs");
  refused("kind 2 in a", POVAR_COV_SOLVER_COORDS, kind_a, 1, "unknown kind");
  refused("kind -1 in b", POVAR_COV_CAMERA_COORDS, kind_b, 1, "unknown kind");
  refused("camera 4 of 4", POVAR_COV_SOLVER_COORDS, cam_hi, 1, "camera id out of range");
  refused("camera -1", POVAR_COV_SOLVER_COORDS, cam_lo, 1, "camera id out of range");
  refused("landmark 5 of 5", POVAR_COV_SOLVER_COORDS, lm_hi, 1, "landmark id out of range");
  refused("landmark -1", POVAR_COV_SOLVER_COORDS, lm_lo, 1, "landmark id out of range");
  refused("a's id before b's kind", POVAR_COV_SOLVER_COORDS, a_first, 1, "camera id out of range");
  refused("the second pair", POVAR_COV_SOLVER_COORDS, later, 2, "landmark id out of range");
  for (int dim = 11; dim <= 12; ++dim) {  // nothing requested: no list to read
    CovPairRequest r;
    std::string err = "ok";
    expect(cov_pair_request(dim, POVAR_COV_CAMERA_COORDS, 4, 5, nullptr, 0, r, &err) && r.total == 0 && r.list[0].size() == 0 &&
               r.list[1].size() == 0 && r.list[2].size() == 0, "pairs: empty request: " + err);
  }
}

// the pivot rule: accept iff min R_kk^2 >= sqrt(2^-53) max A_kk, and nothing that is not a number
static void check_pivots() {
  const double root_u = 1.0536712127723509e-08;  // sqrt(2^-53)
  expect(cov_pivots_ok(1.0, 1.001 * root_u) && !cov_pivots_ok(1.0, 0.999 * root_u) && cov_pivots_ok(4.0, 4.004 * root_u) &&
             !cov_pivots_ok(4.0, 3.9 * root_u) && !cov_pivots_ok(1.0, std::nan("")) && !cov_pivots_ok(std::nan(""), 1.0) &&
             !cov_pivots_ok(1.0, -1.0), "pivot rule");
}

static int gauge_from_file(const char* path) {
  std::FILE* f = std::fopen(path, "r");
  int dim = 0, n_cams = 0;
  if (!f || std::fscanf(f, "%d %d", &dim, &n_cams) != 2 || (dim != 11 && dim != 12) || n_cams < 1) return std::printf("bad file\n"), 2;
  std::vector<double> P(12 * (size_t)n_cams), sg(12 * (size_t)n_cams), ncw(13 * (size_t)n_cams), Q;
  for (std::vector<double>* v : {&P, &sg, &ncw})
    for (double& x : *v)
      if (std::fscanf(f, "%lf", &x) != 1) return std::printf("bad file\n"), 2;
  std::fclose(f);
  int nq = 0;
  if (!gauge_basis(n_cams, dim, P, sg, ncw, Q, nq)) return std::printf("dependent\n"), 0;
  std::printf("nq %d\n", nq);
  for (size_t i = 0; i < (size_t)dim * n_cams; ++i) {
    for (int k = 0; k < nq; ++k) std::printf("%.17g ", Q[i * nq + k]);
    std::printf("\n");
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && !std::strcmp(argv[1], "gauge")) return gauge_from_file(argv[2]);
  check_mode();
  check_lm_request();
  check_pair_request();
  check_pivots();
  if (g_bad) return std::printf("cov_plan_check: %d mismatches\n", g_bad), 1;
  std::printf("cov_plan_check: ok\n");
  return 0;
}
