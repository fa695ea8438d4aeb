// Host-only checker of ShardTeam (host/shard_team.hpp), the threading under the sharded linearizor: who runs fn, how
// often, and what allreduce leaves.  Prints one line per failed check; exit status 0 when all pass.
#include <atomic>
#include <cstdio>
#include <cstring>
#include <set>

#include "../../povar_amd/csrc/host/shard_team.hpp"

using povar_host::ShardTeam;

namespace {

int g_failed = 0;
#define EXPECT(cond, ...)                \
  do {                                   \
    if (!(cond)) {                       \
      ++g_failed;                        \
      std::fprintf(stderr, "FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
      std::fprintf(stderr, __VA_ARGS__); \
      std::fprintf(stderr, "\n");        \
    }                                    \
  } while (0)

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// a team of one without a worker: fn(0), once, on the calling thread
void check_inline_team() {
  ShardTeam team(1, false);
  EXPECT(team.size() == 1, "size %d", team.size());
  int calls = 0, rank = -1;
  std::thread::id where;
  for (int i = 0; i < 200; ++i)
    team.run([&](int r) {
      ++calls;
      rank = r;
      where = std::this_thread::get_id();
    });
  EXPECT(calls == 200 && rank == 0, "calls %d rank %d", calls, rank);
  EXPECT(where == std::this_thread::get_id(), "fn ran on another thread");
}

// n workers: fn once per rank per run, on n distinct threads that are not the caller's and stay the same from run to run
void check_threaded_team(int n) {
  ShardTeam team(n);
  EXPECT(team.size() == n, "size %d of %d", team.size(), n);
  std::vector<std::thread::id> first(n);
  for (int i = 0; i < 200; ++i) {
    std::vector<int> calls(n, 0);  // (each rank writes its own slot; run() returning orders them before the reads)
    std::vector<std::thread::id> where(n);
    std::atomic<int> total{0};
    team.run([&](int r) {
      ++calls[r];
      where[r] = std::this_thread::get_id();
      total.fetch_add(1);
    });
    EXPECT(total.load() == n, "run %d: %d calls for %d ranks", i, total.load(), n);
    for (int r = 0; r < n; ++r) EXPECT(calls[r] == 1, "run %d: rank %d called %d times", i, r, calls[r]);
    std::set<std::thread::id> distinct(where.begin(), where.end());
    EXPECT((int)distinct.size() == n, "run %d: %zu distinct threads for %d ranks", i, distinct.size(), n);
    EXPECT(distinct.count(std::this_thread::get_id()) == 0, "run %d: fn ran on the caller's thread", i);
    if (i == 0) first = where;
    EXPECT(where == first, "run %d: a rank changed its thread", i);
  }
}

// per-rank values whose sum depends on the order: every rank must be left with the left-to-right sum over ranks, bit for bit;
// two buffer lengths back to back, several rounds (the slabs are reused)
void check_allreduce(int n) {
  ShardTeam team(n);
  const double big[3] = {1e16, 1.0, -1e16};  // ((1e16 + 1) - 1e16) = 0 in this order, 1 in the order 0, 2, 1
  auto value = [&](int r, int64_t i, int round) { return big[r % 3] * (double)(i % 5 + 1) + 0.1 * (double)(round + r * i); };
  for (int round = 0; round < 20; ++round)
    for (int64_t len : {int64_t(7), int64_t(1000), int64_t(1)}) {
      std::vector<std::vector<double>> buf(n, std::vector<double>((size_t)len));
      for (int r = 0; r < n; ++r)
        for (int64_t i = 0; i < len; ++i) buf[r][(size_t)i] = value(r, i, round);
      team.run([&](int r) { ShardTeam::allreduce_hook(buf[r].data(), len, &team.hook_args[r]); });
      for (int64_t i = 0; i < len; ++i) {
        double want = 0;
        for (int r = 0; r < n; ++r) want += value(r, i, round);
        for (int r = 0; r < n; ++r)
          EXPECT(same_bits(buf[r][(size_t)i], want), "%d ranks, round %d, length %ld: rank %d element %ld is %.17g, not %.17g", n, round,
                 (long)len, r, (long)i, buf[r][(size_t)i], want);
      }
    }
  // the textbook case itself: 1e16, 1, -1e16 over three ranks gives 0 on every rank (any other order gives 1)
  if (n == 3) {
    double v[3] = {1e16, 1.0, -1e16};
    team.run([&](int r) { ShardTeam::allreduce_hook(&v[r], 1, &team.hook_args[r]); });
    for (int r = 0; r < 3; ++r) EXPECT(same_bits(v[r], (1e16 + 1.0) + -1e16), "rank %d has %.17g", r, v[r]);
    EXPECT(!same_bits((1e16 + 1.0) + -1e16, (1e16 + -1e16) + 1.0), "the order does not matter for these values");
  }
}

}  // namespace

int main() {
  check_inline_team();
  check_threaded_team(1);  // (what a forced one-rank shard team is)
  check_threaded_team(2);
  check_threaded_team(3);
  check_allreduce(2);
  check_allreduce(3);
  if (g_failed) {
    std::fprintf(stderr, "%d check(s) failed\n", g_failed);
    return 1;
  }
  std::printf("shard_team_check: ok\n");
  return 0;
}
