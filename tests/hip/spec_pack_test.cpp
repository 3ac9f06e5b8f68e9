// Host check of what the fixed-form spectrum prologue of chol_mfma_kernel reads
// (csrc/ewarp_spec.h): which jobs get compact power-law records (pl_pack), the
// packing and the 16-byte pieces at the offsets the kernel loads, the padding
// that contributes an exact +0.0, and the 32-bit unit decode against u / B and
// u % B.  Built by `make spec-test` (g++, no HIP), run by
// tests/test_spec_pack_host.py.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../enterprise_warp_amd/csrc/ewarp_spec.h"

using namespace ewh_dev;

// the fields of the device entry (ewarp_dev.h DSpec) that pl_pack reads
struct Spec {
  int kind, col;
  int i0, i1, i2, pad_;
  double v0, v1, v2;
  double a, lnf, lnfyr, f;
};

static int failed = 0, checks = 0;
#define CHECK(c)                                                    \
  do {                                                              \
    ++checks;                                                       \
    if (!(c)) {                                                     \
      ++failed;                                                     \
      std::printf("FAILED line %d: %s\n", __LINE__, #c);            \
    }                                                               \
  } while (0)

static Spec powerlaw(int col, int i0, double v0, int i1, double v1, double k) {
  return Spec{1, col, i0, i1, -1, 0, v0, v1, 0.0, -3.0 - k, -17.0 + k, -17.3, 1e-8};
}

// one column per record, record u with ne[u] entries
static void job(const std::vector<std::vector<Spec>>& recs, std::vector<int>& ptr, std::vector<Spec>& ent,
                std::vector<int>& ulist) {
  ptr.assign(1, 0);
  ent.clear();
  ulist.clear();
  for (size_t u = 0; u < recs.size(); ++u) {
    for (const Spec& s : recs[u]) ent.push_back(s);
    ptr.push_back((int)ent.size());
    ulist.push_back((int)u);
  }
}

// the record as the kernel sees it: 16-byte piece k of entry e = doubles 2 (3 e + k), 2 (3 e + k) + 1
struct Piece { double x, y; };
static Piece piece(const PlRec& r, int e, int k) {
  Piece p;
  std::memcpy(&p, reinterpret_cast<const char*>(&r) + 16 * pl_piece(e, k), 16);
  return p;
}
static void ints(double x, int& lo, int& hi) {
  int v[2];
  std::memcpy(v, &x, 8);
  lo = v[0];
  hi = v[1];
}

// the kernel's evaluation of one entry on the host (the association of spec_phi_body's power law)
static double eval(const PlRec& r, int e, const double* th) {
  const Piece h = piece(r, e, 0), m = piece(r, e, 1), l = piece(r, e, 2);
  int i0, i1;
  ints(h.x, i0, i1);
  const double t0 = th[i0 > 0 ? i0 : 0], t1 = th[i1 > 0 ? i1 : 0];
  const double lgA = i0 >= 0 ? t0 : h.y, gam = i1 >= 0 ? t1 : m.x;
  return std::exp(m.y + 2.0 * 2.302585092994045684 * lgA + (gam - 3.0) * l.y - gam * l.x);
}

static void test_pack() {
  std::vector<int> ptr, ulist;
  std::vector<Spec> ent;
  std::vector<PlRec> out;
  int nem = -1;
  const double th[4] = {-14.2, 4.33, -13.1, 2.5};

  // ne = 1, 2, 3 in one job; sampled and constant parameters in either slot
  const Spec s_ss = powerlaw(0, 0, 0.0, 1, 0.0, 0.1), s_cs = powerlaw(1, -1, -15.5, 3, 0.0, 0.2),
             s_sc = powerlaw(2, 2, 0.0, -1, 4.3333, 0.3), s_cc = powerlaw(2, -7, -16.0, -2, 3.1, 0.4);
  job({{s_ss}, {s_cs, s_sc}, {s_ss, s_sc, s_cc}}, ptr, ent, ulist);
  CHECK(pl_pack(ptr, ent, ulist, 4, out, &nem));
  CHECK(nem == 3 && out.size() == 64);
  CHECK(out[0].ne == 1 && out[1].ne == 2 && out[2].ne == 3 && out[3].ne == 0 && out[63].ne == 0);
  {
    int i0, i1;
    const PlRec& r = out[1];               // {constant lgA, sampled gamma}, {sampled lgA, constant gamma}
    ints(piece(r, 0, 0).x, i0, i1);
    CHECK(i0 == -1 && i1 == 3 && piece(r, 0, 0).y == -15.5);
    CHECK(piece(r, 0, 1).y == s_cs.a && piece(r, 0, 2).x == s_cs.lnf && piece(r, 0, 2).y == s_cs.lnfyr);
    ints(piece(r, 1, 0).x, i0, i1);
    CHECK(i0 == 2 && i1 == -1 && piece(r, 1, 1).x == 4.3333);
    CHECK(piece(r, 1, 1).y == s_sc.a && piece(r, 1, 2).x == s_sc.lnf && piece(r, 1, 2).y == s_sc.lnfyr);
    ints(piece(out[2], 2, 0).x, i0, i1);   // any negative index: the constant
    CHECK(i0 == -1 && i1 == -1 && piece(out[2], 2, 0).y == -16.0 && piece(out[2], 2, 1).x == 3.1);
    // the value, against the entries evaluated one by one
    auto one = [&](const Spec& s) {
      const double lgA = s.i0 >= 0 ? th[s.i0] : s.v0, gam = s.i1 >= 0 ? th[s.i1] : s.v1;
      return std::exp(s.a + 2.0 * 2.302585092994045684 * lgA + (gam - 3.0) * s.lnfyr - gam * s.lnf);
    };
    double want = 0.0, got = 0.0;
    for (const Spec& s : {s_ss, s_sc, s_cc}) want += one(s);
    for (int e = 0; e < PL_NE; ++e) got += eval(out[2], e, th);
    CHECK(want == got && want > 0.0);
    // the unused entries of a shorter record, and a pad record: exactly +0.0
    for (int e = 1; e < PL_NE; ++e) CHECK(eval(out[0], e, th) == 0.0 && !std::signbit(eval(out[0], e, th)));
    for (int e = 0; e < PL_NE; ++e) CHECK(eval(out[40], e, th) == 0.0 && !std::signbit(eval(out[40], e, th)));
    double ph = 0.0;
    for (int e = 0; e < PL_NE; ++e) ph += eval(out[0], e, th);
    CHECK(ph == 0.0 + one(s_ss));
    // ... with a NaN or an inf in theta[0], the row entry the clamped index reads
    const double bad[2][4] = {{NAN, 4.33, -13.1, 2.5}, {INFINITY, 4.33, -13.1, 2.5}};
    for (const auto& tb : bad)
      for (int e = 0; e < PL_NE; ++e) CHECK(eval(out[40], e, tb) == 0.0 && eval(out[1], 0, tb) == eval(out[1], 0, th));
  }

  // more entries than a record holds
  job({{s_ss, s_cs, s_sc, s_cc}}, ptr, ent, ulist);
  CHECK(!pl_pack(ptr, ent, ulist, 4, out, &nem));
  CHECK(nem == 0 && out.empty());            // a refused job leaves nothing half-built
  job({{s_ss, s_cs}, {s_ss, s_cs, s_sc, s_cc}}, ptr, ent, ulist);
  CHECK(!pl_pack(ptr, ent, ulist, 4, out, &nem) && nem == 0 && out.empty());
  // a turnover, a free-spectrum, a constant entry beside power laws
  for (int kind : {2, 3, 4}) {
    Spec o = s_ss;
    o.kind = kind;
    job({{s_ss}, {s_cs, o}}, ptr, ent, ulist);
    CHECK(!pl_pack(ptr, ent, ulist, 4, out, &nem));
    job({{o}}, ptr, ent, ulist);
    CHECK(!pl_pack(ptr, ent, ulist, 4, out, &nem));
  }
  // no theta row to load from; an index past the row
  job({{s_cc}}, ptr, ent, ulist);
  CHECK(!pl_pack(ptr, ent, ulist, 0, out, &nem));
  CHECK(pl_pack(ptr, ent, ulist, 1, out, &nem) && nem == 1);
  job({{s_cs}}, ptr, ent, ulist);
  CHECK(!pl_pack(ptr, ent, ulist, 3, out, &nem));
  // whole waves of records: 64 -> 64, 65 -> 128; no spectrum at all -> one wave of pads
  for (int nu : {0, 1, 64, 65, 128, 143}) {
    std::vector<std::vector<Spec>> recs((size_t)nu, std::vector<Spec>{s_ss});
    job(recs, ptr, ent, ulist);
    CHECK(pl_pack(ptr, ent, ulist, 4, out, &nem));
    CHECK(out.size() == (size_t)(nu == 0 ? 64 : (nu + 63) / 64 * 64) && out.size() % 64 == 0 && (int)out.size() >= nu);
    CHECK(nem == (nu ? 1 : 0));
  }
  // a column without entries between the representatives (ulist names columns, not positions)
  ptr = {0, 1, 1, 2};
  ent = {s_ss, s_sc};
  ulist = {0, 2};
  CHECK(pl_pack(ptr, ent, ulist, 4, out, &nem));
  int i0, i1;
  ints(piece(out[1], 0, 0).x, i0, i1);
  CHECK(out[1].ne == 1 && i0 == 2 && i1 == -1);
}

static void test_decode() {
  // every unit of the launch, against the 64-bit division
  struct Case { long long u0, n; int B; };
  const Case cases[] = {{0, 5000, 1},       {12345, 70000, 1},      {0, 184320, 4096},  {4096 * 7 + 1234, 100000, 4096},
                        {100, 100000, 7},   {33, 50000, 48},        {5, 4000, 3},       {31, 2000, 32},
                        {999999, 3000, 1000}, {(1ll << 31) + 77, 100000, 24}, {123456789012ll, 66000, 4099}};
  for (const Case& c : cases) {
    const UnitDec d = unit_dec_make(c.u0, c.B);
    long long bad = 0;
    for (long long v = 0; v < c.n; ++v) {
      int p, b;
      unit_decode(d, (uint32_t)v, (uint32_t)c.B, p, b);
      if (p != (int)((c.u0 + v) / c.B) || b != (int)((c.u0 + v) % c.B)) ++bad;
    }
    std::printf("decode u0 %lld n %lld B %d: %lld wrong\n", c.u0, c.n, c.B, bad);
    CHECK(bad == 0);
  }
  // the ends of the range: a launch of 2^31 units, the largest batch
  for (int B : {1, 2, 3, 7, 4096, 65537, 0x7fffffff}) {
    for (long long u0 : {0ll, (long long)B - 1, 5ll * B + B / 2}) {
      const UnitDec d = unit_dec_make(u0, B);
      long long bad = 0;
      for (long long v : {0ll, 1ll, (long long)B - 1, (long long)B, (1ll << 31) - 2, (1ll << 31) - 1})
        for (long long w = v > 2000 ? v - 2000 : 0; w <= v; ++w) {
          int p, b;
          if ((u0 + w) / B > 0x7fffffff) continue;   // (a pulsar index is an int)
          unit_decode(d, (uint32_t)w, (uint32_t)B, p, b);
          if (p != (int)((u0 + w) / B) || b != (int)((u0 + w) % B)) ++bad;
        }
      CHECK(bad == 0);
    }
  }
}

int main() {
  test_pack();
  test_decode();
  std::printf("%d checks, %d failed\n", checks, failed);
  return failed ? 1 : 0;
}
