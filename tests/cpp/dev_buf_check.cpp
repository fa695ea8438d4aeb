// Host-only checker of DevBuf<T> (dev_buf.hpp), the self-freeing device allocation behind every buffer of a context: what
// is freed when, what alloc counts, what a failed allocation leaves.  hipMalloc / hipFree are this file's own (a table of live
// blocks, a failure on demand): no HIP runtime is linked.  Prints one line per failed check; exit status 0 when all pass.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>

#include "../../povar_amd/csrc/dev_buf.hpp"

namespace {
std::set<void*> g_live;  // blocks handed out and not yet freed
int g_mallocs = 0, g_frees = 0, g_bad_frees = 0;
int g_fail_at = 0;       // the k-th hipMalloc from now fails (0: none)
}  // namespace

extern "C" hipError_t hipMalloc(void** ptr, size_t size) {
  if (g_fail_at > 0 && --g_fail_at == 0) return hipErrorOutOfMemory;  // (*ptr untouched, as the runtime leaves it)
  ++g_mallocs;
  *ptr = std::malloc(size ? size : 1);
  g_live.insert(*ptr);
  return hipSuccess;
}

extern "C" hipError_t hipFree(void* ptr) {
  ++g_frees;
  if (!ptr) return hipSuccess;
  if (!g_live.erase(ptr)) {  // a second free of the same block, or of one that was never handed out
    ++g_bad_frees;
    return hipErrorInvalidValue;
  }
  std::free(ptr);
  return hipSuccess;
}

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

void must(hipError_t e) { EXPECT(e == hipSuccess, "an allocation of the set-up failed (%d)", (int)e); }
int live() { return (int)g_live.size(); }
// every case ends with nothing live and no block freed twice
void expect_clean(const char* what) { EXPECT(live() == 0 && g_bad_frees == 0, "%s: live %d, bad frees %d", what, live(), g_bad_frees); }

void check_scope_and_release() {
  size_t total = 0;
  {
    DevBuf<double> a;
    EXPECT(a.p == nullptr && a.n == 0, "a fresh buffer owns something");
    EXPECT(a.alloc(10, &total) == hipSuccess && a.p && a.n == 10, "alloc(10): n %zu", a.n);
    EXPECT(total == 10 * sizeof(double) && live() == 1, "total %zu live %d", total, live());
  }
  EXPECT(live() == 0, "scope exit left %d blocks", live());
  DevBuf<int> b;
  EXPECT(b.alloc(3, nullptr) == hipSuccess && live() == 1, "alloc without a counter");
  b.release();
  EXPECT(b.p == nullptr && b.n == 0 && live() == 0, "release: n %zu live %d", b.n, live());
  b.release();
  EXPECT(b.p == nullptr && b.n == 0, "second release: n %zu", b.n);
  expect_clean("scope / release");
}

void check_alloc() {
  size_t total = 0;
  DevBuf<float> a;
  const int mallocs0 = g_mallocs;
  EXPECT(a.alloc(0, &total) == hipSuccess && a.p == nullptr && a.n == 0 && total == 0, "alloc(0): n %zu total %zu", a.n, total);
  EXPECT(g_mallocs == mallocs0 && live() == 0, "alloc(0) called hipMalloc");
  EXPECT(a.alloc(8, &total) == hipSuccess && total == 8 * sizeof(float), "total %zu", total);
  total = 0;
  // on a buffer that owns a block: the old one is freed, only the new one is counted (counting down is the caller's business)
  const int frees0 = g_frees;
  EXPECT(a.alloc(20, &total) == hipSuccess && a.n == 20 && live() == 1, "re-alloc: n %zu live %d", a.n, live());
  EXPECT(total == 20 * sizeof(float) && g_frees == frees0 + 1, "re-alloc counted %zu, freed %d", total, g_frees - frees0);
  // alloc(0) on an owning buffer frees it
  EXPECT(a.alloc(0, &total) == hipSuccess && a.p == nullptr && a.n == 0 && live() == 0, "alloc(0) kept the block");
  // a failed allocation: empty buffer, counter untouched -- on an empty buffer and on one that owned a block
  total = 0;
  g_fail_at = 1;
  EXPECT(a.alloc(5, &total) == hipErrorOutOfMemory && a.p == nullptr && a.n == 0 && total == 0, "failed alloc: n %zu total %zu", a.n, total);
  EXPECT(a.alloc(5, &total) == hipSuccess && total == 5 * sizeof(float), "alloc after a failure");
  total = 0;
  g_fail_at = 1;
  EXPECT(a.alloc(7, &total) == hipErrorOutOfMemory && a.p == nullptr && a.n == 0 && total == 0 && live() == 0,
         "failed re-alloc: n %zu total %zu live %d", a.n, total, live());
  // the k-th call fails, the ones before it succeed
  DevBuf<float> b, c2;
  g_fail_at = 2;
  EXPECT(b.alloc(1, &total) == hipSuccess && c2.alloc(1, &total) == hipErrorOutOfMemory && live() == 1 && total == sizeof(float), "second of two");
  b.release();
  expect_clean("alloc");
}

void check_move() {
  size_t total = 0;
  DevBuf<int> a;
  must(a.alloc(4, &total));
  int* pa = a.p;
  DevBuf<int> b(std::move(a));
  EXPECT(a.p == nullptr && a.n == 0 && b.p == pa && b.n == 4 && live() == 1, "move construction");
  DevBuf<int> c2;
  must(c2.alloc(6, &total));
  int* pc = c2.p;
  const int frees0 = g_frees;
  c2 = std::move(b);  // frees what c2 held
  EXPECT(b.p == nullptr && b.n == 0 && c2.p == pa && c2.n == 4, "move assignment");
  EXPECT(live() == 1 && !g_live.count(pc) && g_frees == frees0 + 1, "move assignment: live %d frees %d", live(), g_frees - frees0);
  DevBuf<int>& self = c2;
  c2 = std::move(self);
  EXPECT(c2.p == pa && c2.n == 4 && live() == 1, "self move assignment lost the block");
  c2 = DevBuf<int>();  // an empty one assigned: freed
  EXPECT(c2.p == nullptr && c2.n == 0 && live() == 0, "assigning an empty buffer");
  expect_clean("move");
}

// the shape of povar_ctx::CkDev: a base of buffers, counts beside it, release() that assigns an empty base
struct Bufs {
  DevBuf<double> uv;
  DevBuf<int> src, tile;
};
struct Dev : Bufs {
  int nb = 0;
  double build_ms = 0;
  bool ready = false;
  void release() {
    static_cast<Bufs&>(*this) = Bufs();
    ready = false;
  }
};

void check_swap_and_structs() {
  size_t total = 0;
  {
    DevBuf<int> a, b;
    must(a.alloc(2, &total));
    must(b.alloc(3, &total));
    int *pa = a.p, *pb = b.p;
    std::swap(a, b);
    EXPECT(a.p == pb && a.n == 3 && b.p == pa && b.n == 2, "swap of two buffers");
    EXPECT(live() == 2 && g_live.count(pa) && g_live.count(pb), "swap freed a block (live %d)", live());
    DevBuf<int> e;
    std::swap(a, e);  // with an empty one
    EXPECT(a.p == nullptr && a.n == 0 && e.p == pb && live() == 2, "swap with an empty buffer");
  }
  EXPECT(live() == 0, "swapped buffers left %d blocks", live());
  {
    Dev x, y;
    must(x.uv.alloc(5, &total)); must(x.src.alloc(6, &total)); x.nb = 7; x.build_ms = 1.5; x.ready = true;
    must(y.uv.alloc(8, &total)); must(y.tile.alloc(9, &total)); y.nb = 11; y.build_ms = 2.5;
    double* xu = x.uv.p;
    int* yt = y.tile.p;
    std::swap(x, y);
    EXPECT(live() == 4, "swap of two structs freed a block (live %d)", live());
    EXPECT(y.uv.p == xu && y.uv.n == 5 && y.src.n == 6 && y.tile.p == nullptr && y.nb == 7 && y.build_ms == 1.5 && y.ready, "struct swap: y");
    EXPECT(x.tile.p == yt && x.uv.n == 8 && x.src.p == nullptr && x.nb == 11 && x.build_ms == 2.5 && !x.ready, "struct swap: x");
    y.release();  // every buffer freed, the counts kept
    EXPECT(live() == 2 && y.uv.p == nullptr && y.uv.n == 0 && y.src.p == nullptr && y.tile.p == nullptr, "release left buffers (live %d)", live());
    EXPECT(y.nb == 7 && y.build_ms == 1.5 && !y.ready, "release touched the counts: nb %d", y.nb);
    y.release();
    EXPECT(live() == 2, "second release");
    Dev z(std::move(x));  // a struct of buffers moves as a whole
    EXPECT(live() == 2 && x.uv.p == nullptr && x.tile.p == nullptr && z.tile.p == yt && z.nb == 11, "struct move construction");
  }
  expect_clean("swap / structs");
}

}  // namespace

int main() {
  check_scope_and_release();
  check_alloc();
  check_move();
  check_swap_and_structs();
  expect_clean("exit");
  if (g_failed) {
    std::fprintf(stderr, "dev_buf_check: %d checks failed\n", g_failed);
    return 1;
  }
  std::printf("dev_buf_check: ok\n");
  return 0;
}
