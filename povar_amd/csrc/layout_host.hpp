// layout_host.hpp -- what the host-side layout builders share that a plain C++ compiler can read without the HIP headers:
// the wavefront width, the host thread pool, and -- outside hipcc -- stand-ins for the two vector types the layouts carry.
// res_layout.hpp needs nothing else, so its stand-alone checker (tests/cpp/res_layout_h_check.cpp) builds with g++ alone.
#pragma once

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#else
struct int2 { int x, y; };
struct double2 { double x, y; };
inline int2 make_int2(int x, int y) { return int2{x, y}; }
inline double2 make_double2(double x, double y) { return double2{x, y}; }
#ifndef __host__
#define __host__
#define __device__
#endif
#endif

namespace povar {

constexpr int WAVE = 64;

// CPUs this process may actually use: the hardware threads, cut by the cgroup CPU quota when there is one (a container
// that sees 256 hardware threads under a 16-CPU quota gets slower, not faster, beyond 16 busy threads)
inline int lpl_effective_cpus() {
  int n = (int)std::max(1u, std::thread::hardware_concurrency());
  if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {  // cgroup v2: "<quota|max> <period>"
    char q[32] = {0};
    long period = 0;
    if (std::fscanf(f, "%31s %ld", q, &period) == 2 && q[0] != 'm' && period > 0)
      n = std::min<long>(n, std::max<long>(1, (std::atol(q) + period - 1) / period));
    std::fclose(f);
  } else if (FILE* g = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {  // cgroup v1
    long quota = -1, period = 0;
    if (std::fscanf(g, "%ld", &quota) != 1) quota = -1;
    std::fclose(g);
    if (FILE* h = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
      if (std::fscanf(h, "%ld", &period) != 1) period = 0;
      std::fclose(h);
    }
    if (quota > 0 && period > 0) n = std::min<long>(n, std::max<long>(1, (quota + period - 1) / period));
  }
  return n;
}

// fn(item) for item in [0, n_items) on up to n_threads host threads (items taken on demand; the caller's thread works too)
// (cancel: when it turns true the remaining items are dropped -- a build whose result nobody waits for any more)
template <class F>
inline void lpl_parallel(int n_items, int n_threads, F&& fn, const std::atomic<bool>* cancel = nullptr) {
  std::atomic<int> next{0};
  auto work = [&]() {
    for (;;) {
      const int i = next.fetch_add(1);
      if (i >= n_items || (cancel && cancel->load(std::memory_order_relaxed))) break;
      fn(i);
    }
  };
  std::vector<std::thread> pool;
  for (int t = 1; t < std::min(n_threads, n_items); ++t) pool.emplace_back(work);
  work();
  for (auto& th : pool) th.join();
}

}  // namespace povar
