// The `bal` executable of the drop-in surface (src/app/bal.cpp:44-103): parse -> load ->
// bundle_adjust_manual -> log.
#include <cstdio>
#include <vector>

#include "linearizor.hpp"

int main(int argc, char** argv) {
  using namespace povar_host;
  BalAppOptions options;
  if (!parse_bal_app_arguments(argc, argv, options)) return 1;
  // src/app/bal.cpp:83-99: load (+ dataset summary, timing) -> solve -> postprocess -> log
  BalPipelineSummary summary;
  BalProblem bal_problem = load_normalized_bal_problem(options.dataset, &summary.dataset, &summary.timing);
  if (!options.solver.fixed_cameras.empty()) {  // --fixed-cameras: the ids against the problem, before any device work
    std::vector<char> seen((size_t)bal_problem.num_cameras(), 0);
    int k = 0;
    for (const int id : options.solver.fixed_cameras) {
      if (id >= bal_problem.num_cameras()) {
        std::fprintf(stderr, "--fixed-cameras: camera %d out of range (the problem has %d cameras)\n", id, bal_problem.num_cameras());
        return 1;
      }
      k += !seen[(size_t)id];
      seen[(size_t)id] = 1;
    }
    std::printf("fixed cameras: %d of %d\n", k, bal_problem.num_cameras());
    if (options.solver.dense_compaction)  // --compact-fixed-cameras (no effect, and no line, without the set)
      std::printf("dense system: compacted to the %d free cameras\n", bal_problem.num_cameras() - k);
    std::fflush(stdout);
  }
  bundle_adjust_manual(bal_problem, options.solver, &summary.solver, &summary.timing);
  save_ba_log_json(summary, options.solver);
  return 0;
}
