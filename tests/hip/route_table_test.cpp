// Host check of the factorisation route (csrc/ewarp_route.h): including the
// header runs its static_asserts -- the route table of the product modes and
// the equality with the routing code it replaced -- under the host compiler.
// The program prints the table and compares each cell, at run time, with the
// table written out below (one letter per width).  Built by `make route-test`
// (g++, no HIP), run by tests/test_route_host.py.
#include <cstdio>

#include "../../enterprise_warp_amd/csrc/ewarp_route.h"

using namespace ewh_dev;

static const char* name(Route r) {
  switch (r) {
    case Route::Register: return "register";
    case Route::Big: return "big";
    case Route::Lds: return "lds";
    case Route::Wide: return "wide";
    case Route::DdVerify: return "dd-verify";
    case Route::DdAll: return "dd-all";
    default: return "unsupported";
  }
}

static char letter(Route r) { return "RGLWVAU"[(int)r]; }   // the enum's order

// the routes at 1, 9, 10, 16, 17, 64 and 65 blocks: fixed run, sampled chunk, common process
struct Expect { int mode; const char *fixed, *sampled, *common; };
static const Expect EXPECT[] = {
    {0, "RRVVVVU", "RRGGVVU", "RRGGWWU"},  {1, "LLLLWWU", "LLLLWWU", "LLLLWWU"},
    {2, "RRVVVVU", "RRGGVVU", "RRGGWWU"},  {7, "RRVVVVU", "RRGGVVU", "RRGGWWU"},
    {27, "WWWWWWU", "WWWWWWU", "WWWWWWU"}, {29, "AAAAAAA", "RRGGAAA", "RRGGWWU"},
};

int main() {
  const int widths[] = {1, 9, 10, 16, 17, 64, 65};
  int rows = 0, failed = 0;
  std::printf("mode nb  fixed-run (refine)     sampled (refine)       common process\n");
  for (const Expect& e : EXPECT) {
    const KernelPlan p = plan_for(e.mode, false);
    for (int i = 0; i < 7; ++i) {
      const int nb = widths[i];
      const Route fx = route_for(p, false, false, nb, true), sm = route_for(p, false, false, nb, false),
                  cm = route_for(p, true, false, nb, true);
      // (no launch of an unsupported width gets as far as the refine pass)
      const bool rfx = fx != Route::Unsupported && refine_after(Source::FixedRun, nb, false, p, false, false);
      const bool rsm = sm != Route::Unsupported && refine_after(Source::Varying, nb, false, p, false, false);
      const bool ok = letter(fx) == e.fixed[i] && letter(sm) == e.sampled[i] && letter(cm) == e.common[i] &&
                      route_for(p, false, true, nb, true) == cm;
      failed += !ok;
      std::printf("%4d %2d  %-12s %-9s %-12s %-9s %s%s\n", e.mode, nb, name(fx), rfx ? "refine" : "-", name(sm),
                  rsm ? "refine" : "-", name(cm), ok ? "" : "   <-- not the expected route");
      ++rows;
    }
  }
  std::printf("%d rows, %d failed\n", rows, failed);
  return failed ? 1 : 0;
}
