// One host thread per shard context.  The library's sharded entry points are collectives -- every rank must be inside
// the same call at the same time -- while the reference's caller is ONE thread (solver/linearizor.hpp:65-81): run() hands
// the same call to every worker and waits.  A team of one may do without a worker: run() is then a plain call.
// Plain C++17, no device header: tests/cpp/shard_team_check.cpp compiles it alone.
#pragma once
#include <condition_variable>
#include <cstdint>
#include <functional>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

namespace povar_host {

class ShardTeam {
 public:
  // threads == false (a team of one only): no worker, no lock -- run(fn) is fn(0) on the caller's thread
  explicit ShardTeam(int n, bool threads = true) : n_(threads ? n : 1), slab_(n_) {
    for (int r = 0; r < n_; ++r) hook_args.emplace_back(this, r);
    for (int r = 0; threads && r < n_; ++r) workers_.emplace_back([this, r] { loop(r); });
  }
  ShardTeam(const ShardTeam&) = delete;
  ShardTeam& operator=(const ShardTeam&) = delete;
  ~ShardTeam() {
    if (workers_.empty()) return;
    {
      std::lock_guard<std::mutex> lk(mu_);
      quit_ = true;
      ++gen_;
    }
    cv_.notify_all();
    for (auto& t : workers_) t.join();
  }
  int size() const { return n_; }
  // fn(rank) on every shard's thread, concurrently; returns when all are done
  void run(const std::function<void(int)>& fn) {
    if (workers_.empty()) {
      fn(0);
      return;
    }
    {
      std::lock_guard<std::mutex> lk(mu_);
      fn_ = &fn;
      pending_ = n_;
      ++gen_;
    }
    cv_.notify_all();
    std::unique_lock<std::mutex> lk(mu_);
    done_cv_.wait(lk, [this] { return pending_ == 0; });
    fn_ = nullptr;
  }
  // in-process all-reduce (sum, in place, fixed rank order on every rank): the host hook of povar_comm_init_host, with
  // &hook_args[rank] as its user pointer; every rank calls it from its own worker
  static void allreduce_hook(double* buf, int64_t n, void* user) {
    auto* a = static_cast<std::pair<ShardTeam*, int>*>(user);
    a->first->allreduce(a->second, buf, n);
  }
  std::vector<std::pair<ShardTeam*, int>> hook_args;  // one per rank, filled by the constructor

 private:
  void loop(int r) {
    long seen = 0;
    for (;;) {
      const std::function<void(int)>* fn = nullptr;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return gen_ != seen; });
        seen = gen_;
        if (quit_) return;
        fn = fn_;
      }
      (*fn)(r);
      {
        std::lock_guard<std::mutex> lk(mu_);
        --pending_;
      }
      done_cv_.notify_all();
    }
  }
  void barrier() {
    std::unique_lock<std::mutex> lk(bar_mu_);
    const long g = bar_gen_;
    if (++bar_count_ == n_) {
      bar_count_ = 0;
      ++bar_gen_;
      bar_cv_.notify_all();
    } else {
      bar_cv_.wait(lk, [&] { return bar_gen_ != g; });
    }
  }
  void allreduce(int rank, double* buf, int64_t n) {
    slab_[rank].assign(buf, buf + n);
    barrier();
    for (int64_t i = 0; i < n; ++i) {
      double s = 0;
      for (int r = 0; r < n_; ++r) s += slab_[r][i];
      buf[i] = s;
    }
    barrier();
  }
  int n_;
  std::vector<std::thread> workers_;
  std::mutex mu_, bar_mu_;
  std::condition_variable cv_, done_cv_, bar_cv_;
  const std::function<void(int)>* fn_ = nullptr;
  int pending_ = 0, bar_count_ = 0;
  long gen_ = 0, bar_gen_ = 0;
  bool quit_ = false;
  std::vector<std::vector<double>> slab_;
};

}  // namespace povar_host
