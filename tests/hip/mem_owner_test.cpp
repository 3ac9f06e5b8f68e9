// Host test of csrc/ewarp_mem.h (Buf, Arena, the reallocation hook): this
// file supplies mem_alloc / mem_free itself, on malloc / free, counts the live
// blocks and can fail the n-th allocation.  No HIP, no GPU.  Build and run
// under the sanitizers (make mem-test, tests/test_mem_owner_host.py):
//   g++ -std=c++17 -fsanitize=address,undefined -o build/mem_owner_test tests/hip/mem_owner_test.cpp
#include "../../enterprise_warp_amd/csrc/ewarp_mem.h"

#include <cstdio>
#include <cstdlib>
#include <set>

using namespace ewh_mem;

namespace {
std::set<void*> g_live;
int g_allocs = 0, g_frees = 0, g_bad_frees = 0;
int g_fail_at = 0;          // fail the g_fail_at-th allocation from now (0: none)
int g_checks = 0, g_failed = 0;

void check(bool ok, const char* what, int line) {
  ++g_checks;
  if (!ok) {
    ++g_failed;
    std::printf("FAILED line %d: %s\n", line, what);
  }
}
#define CHECK(x) check((x), #x, __LINE__)

void reset_counts() { g_allocs = g_frees = 0; }
}  // namespace

int ewh_mem::mem_alloc(MemKind, void** p, size_t bytes) {
  *p = nullptr;
  if (g_fail_at > 0 && --g_fail_at == 0) return -3;
  *p = std::malloc(bytes);
  if (!*p) return -3;
  g_live.insert(*p);
  ++g_allocs;
  return 0;
}

void ewh_mem::mem_free(MemKind, void* p) {
  if (g_live.erase(p) != 1) {       // a block freed twice, or never handed out
    ++g_bad_frees;
    return;
  }
  ++g_frees;
  std::free(p);
}

int main() {
  int fired = 0;
  const Hook hook{[](void* n) { ++*(int*)n; }, &fired};

  {  // reserve within the cap allocates nothing; the hook stays quiet
    Buf<double> b;
    CHECK(b.p == nullptr && b.cap == 0);
    CHECK(b.reserve(10, hook) == 0 && b.p && b.cap == 10);
    CHECK(g_allocs == 1 && g_frees == 0 && fired == 1);
    double* p0 = b.p;
    b.p[9] = 1.0;                   // the last element is ours (ASan)
    CHECK(b.reserve(10, hook) == 0 && b.reserve(3, hook) == 0 && b.reserve(0, hook) == 0);
    CHECK(b.p == p0 && b.cap == 10 && g_allocs == 1 && g_frees == 0 && fired == 1);
    // growth frees exactly one block and allocates one; the hook fires
    CHECK(b.reserve(11, hook) == 0 && b.cap == 11);
    CHECK(g_allocs == 2 && g_frees == 1 && g_live.size() == 1 && fired == 2);
    b.p[10] = 2.0;
    // a failed reserve leaves the buffer empty, the old block freed once
    g_fail_at = 1;
    CHECK(b.reserve(100, hook) != 0);
    CHECK(b.p == nullptr && b.cap == 0 && g_allocs == 2 && g_frees == 2 && g_live.empty() && fired == 3);
    // ... and the next reserve allocates again
    CHECK(b.reserve(4, hook) == 0 && b.cap == 4 && g_live.size() == 1);
    // release is idempotent
    b.release();
    b.release();
    CHECK(b.p == nullptr && b.cap == 0 && g_live.empty() && g_frees == 3 && g_bad_frees == 0);
    // an empty request on an empty buffer is a no-op; a first one gets a block
    CHECK(b.reserve(0, hook) == 0 && b.p == nullptr && g_live.empty());
  }

  {  // an Arena frees everything once: on release, and not again on destruction
    reset_counts();
    fired = 0;
    {
      Arena a(hook);
      double* x;
      int* y;
      char* z;
      CHECK(a.alloc(&x, 5) == 0 && a.alloc(&y, 0) == 0 && a.alloc(&z, 7) == 0);
      CHECK(x && y && z && g_live.size() == 3 && fired == 3);
      x[4] = 1.0;
      y[0] = 1;
      g_fail_at = 1;
      double* w = x;
      CHECK(a.alloc(&w, 9) != 0 && w == nullptr && g_live.size() == 3);
      a.release();
      CHECK(g_live.empty() && g_frees == 3);
      CHECK(a.alloc(&x, 2) == 0 && g_live.size() == 1);
    }                                // ~Arena: the one block left
    CHECK(g_live.empty() && g_frees == 4 && g_allocs == 4 && g_bad_frees == 0);
  }

  {  // a group of three, the second allocation failing: all empty after the
     // group's release, nothing live (the chunk scratches of DevCtx)
    reset_counts();
    struct Group {
      Buf<double> a, b;
      Buf<int> c;
      int chunk = 0;
      void release() {
        a.release();
        b.release();
        c.release();
        chunk = 0;
      }
      int reserve(size_t n) {
        release();
        int rc;
        if ((rc = a.reserve(n)) || (rc = b.reserve(2 * n)) || (rc = c.reserve(n))) {
          release();
          return rc;
        }
        chunk = (int)n;
        return 0;
      }
    } g;
    CHECK(g.reserve(8) == 0 && g.chunk == 8 && g_live.size() == 3);
    g_fail_at = 2;
    CHECK(g.reserve(16) != 0);
    CHECK(!g.a.p && !g.b.p && !g.c.p && g.a.cap == 0 && g.b.cap == 0 && g.c.cap == 0 && g.chunk == 0);
    CHECK(g_live.empty() && g_allocs == 4 && g_frees == 4 && g_bad_frees == 0);
    CHECK(g.reserve(16) == 0 && g.chunk == 16 && g_live.size() == 3);   // the next call sizes it again
    g.release();
    g.release();
    CHECK(g_live.empty() && g_bad_frees == 0);
  }

  std::printf("mem_owner_test: %d checks, %d failed\n", g_checks, g_failed);
  return g_failed == 0 && g_live.empty() && g_bad_frees == 0 ? 0 : 1;
}
