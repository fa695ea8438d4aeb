// cam_row_map_check.cpp -- the host-only builder of the dense matrix's layout (cov_plan.hpp: cam_row_map; povar_set_dense_compaction)
// held to its contract on the CPU: mode 0 gives dim c for every camera; mode 1 gives ascending rows in steps of dim over exactly
// the free cameras and -1 elsewhere; the row count; empty F, full F, one camera; both dims.  Stand-alone: compiled and run by
// tests/test_dense_compaction_cpu.py with the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../povar_amd/csrc/cov_plan.hpp"

namespace {
int failures = 0;
void expect(bool ok, const char* what, int a = 0, int b = 0) {
  if (ok) return;
  ++failures;
  std::fprintf(stderr, "FAIL: %s (%d, %d)\n", what, a, b);
}

// the contract, written out independently of the builder
void check(const std::vector<uint8_t>& fixed, int dim, int mode) {
  const int n_cams = (int)fixed.size();
  std::vector<int32_t> rows(3, 77);  // (a stale vector of another size: the builder resizes and overwrites)
  const int n = povar::cam_row_map(fixed.data(), n_cams, dim, mode, rows);
  expect((int)rows.size() == n_cams, "size of the map", (int)rows.size(), n_cams);
  int n_free = 0, next = 0;
  for (int c = 0; c < n_cams; ++c) {
    const bool in = mode == 0 || !fixed[(size_t)c];
    if (mode == 0) expect(rows[(size_t)c] == dim * c, "mode 0: camera c at dim c", c, rows[(size_t)c]);
    if (in) {
      expect(rows[(size_t)c] == next, "ascending rows in steps of dim", c, rows[(size_t)c]);
      next += dim;
      ++n_free;
    } else {
      expect(rows[(size_t)c] == -1, "-1 for a camera that is not in the matrix", c, rows[(size_t)c]);
    }
  }
  expect(n == dim * n_free, "row count", n, dim * n_free);
}
}  // namespace

int main() {
  for (const int dim : {12, 11})
    for (const int mode : {0, 1}) {
      check({}, dim, mode);                        // no camera at all
      check({0}, dim, mode);                       // n_cams = 1, free
      check({1}, dim, mode);                       // n_cams = 1, fixed
      check({0, 0, 0, 0, 0, 0}, dim, mode);        // empty F
      check({1, 1, 1, 1, 1, 1}, dim, mode);        // full F
      check({0, 1, 0, 0, 1, 0}, dim, mode);        // the set of `small`
      check({1, 0, 0, 0, 0, 1}, dim, mode);        // first and last
      check({0, 0, 0, 1, 1, 1}, dim, mode);        // a suffix
      std::vector<uint8_t> window(40, 1);          // a window: all but five
      for (const int c : {7, 8, 30, 33, 34}) window[(size_t)c] = 0;
      check(window, dim, mode);
    }
  // the values of two cases spelled out
  std::vector<int32_t> rows;
  const uint8_t f6[6] = {0, 1, 0, 0, 1, 0};
  expect(povar::cam_row_map(f6, 6, 12, 1, rows) == 48, "small, step 1: 48 rows");
  expect(rows == std::vector<int32_t>({0, -1, 12, 24, -1, 36}), "small, step 1: the map");
  expect(povar::cam_row_map(f6, 6, 11, 1, rows) == 44, "small, step 2: 44 rows");
  expect(rows == std::vector<int32_t>({0, -1, 11, 22, -1, 33}), "small, step 2: the map");
  expect(povar::cam_row_map(f6, 6, 11, 0, rows) == 66, "small, step 2, mode 0: 66 rows");
  expect(rows == std::vector<int32_t>({0, 11, 22, 33, 44, 55}), "small, step 2, mode 0: the map");
  const uint8_t all[2] = {1, 1};
  expect(povar::cam_row_map(all, 2, 12, 1, rows) == 0 && rows == std::vector<int32_t>({-1, -1}), "every camera fixed: n = 0");
  if (failures) return 1;
  std::printf("cam_row_map: ok\n");
  return 0;
}
