// ewarp_spec.h — what the fixed-form spectrum prologue of chol_mfma_kernel
// reads: the compact power-law records of a fixed-white-noise job (PlRec, the
// rule for which jobs have them, their packing) and the 32-bit unit decode
// (UnitDec).  Both are decided on the host, once; the kernel only loads and
// evaluates.  No HIP dependency (tests/hip/spec_pack_test.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <limits>
#include <vector>

#if defined(__HIPCC__)
#define EWH_SPEC_HD __host__ __device__
#else
#define EWH_SPEC_HD
#endif

namespace ewh_dev {

constexpr int PL_KIND_POWERLAW = 1;   // EWH_SPEC_POWERLAW (include/ewarp_hip.h)
constexpr int PL_NE = 3;              // entries per record (URec::NE)
constexpr int PL_LANES = 64;          // records are dealt one per lane: the array is padded to whole waves

// One power-law entry: phi_e = exp(a + 2 ln10 lgA + (gam - 3) lnfyr - gam lnf)
// with lgA = i0 >= 0 ? theta[i0] : v0 and gam = i1 >= 0 ? theta[i1] : v1 (i0,
// i1: positions in the sample's theta row itself).  Three 16-byte pieces.
struct PlEntry {
  int32_t i0, i1;
  double v0;
  double v1, a;
  double lnf, lnfyr;
};

// One distinct spectrum: phi = 0.0 + phi_0 + phi_1 + phi_2.  An unused entry
// is {-1, -1, 0, 0, -inf, 0, 0}: exp(-inf + 0 + (0 - 3) 0 - 0 0) = +0.0, and
// x + 0.0 == x for every x >= 0, inf and NaN -- so a launch evaluates the
// entries up to the largest ne of its jobs (CholJob::pl_ne) on every lane,
// without a per-lane branch.  Ten 16-byte pieces.
struct PlRec {
  PlEntry e[PL_NE];
  int32_t ne, pad_[3];
};

static_assert(sizeof(PlEntry) == 48 && sizeof(PlRec) == 160 && alignof(PlRec) == 8, "compact record: 10 x 16 bytes");
static_assert(offsetof(PlEntry, i0) == 0 && offsetof(PlEntry, i1) == 4 && offsetof(PlEntry, v0) == 8 &&
                  offsetof(PlEntry, v1) == 16 && offsetof(PlEntry, a) == 24 && offsetof(PlEntry, lnf) == 32 &&
                  offsetof(PlEntry, lnfyr) == 40,
              "entry: {i0, i1, v0} {v1, a} {lnf, lnfyr}");
static_assert(offsetof(PlRec, e) == 0 && offsetof(PlRec, ne) == 144, "record: three entries, then ne");
// the kernel's view of a record: piece k of entry e at 16-byte index 3 e + k
constexpr int PL_PIECES = 10;
constexpr int pl_piece(int e, int k) { return 3 * e + k; }
static_assert(pl_piece(PL_NE - 1, 2) == PL_PIECES - 2 && PL_PIECES * 16 == (int)sizeof(PlRec), "pieces cover the record");

inline PlEntry pl_pad_entry() {
  return PlEntry{-1, -1, 0.0, 0.0, -std::numeric_limits<double>::infinity(), 0.0, 0.0};
}
inline PlRec pl_pad_rec() {
  PlRec r{};
  for (int e = 0; e < PL_NE; ++e) r.e[e] = pl_pad_entry();
  r.ne = 0;
  return r;
}

// Records in the array of a job with nu distinct spectra: whole waves, at
// least one, so lane l of trip t always has record 64 t + l to load.
constexpr size_t pl_padded(size_t nu) { return nu == 0 ? PL_LANES : (nu + PL_LANES - 1) / PL_LANES * PL_LANES; }

// The compact records of a job from its CSR spectra (ptr over columns, ent the
// entries with positions in the theta row: fields kind, i0, i1, v0, v1, a,
// lnf, lnfyr) and the list of the columns that represent its distinct spectra.
// A job qualifies -- returns true, out filled and padded, *ne_max the largest
// entry count -- when every entry of every record is a power law, no record
// has more than PL_NE entries, and the theta row has at least one parameter
// (the kernel loads theta[max(i, 0)] before it selects the constant).
template <class Spec>
bool pl_pack(const std::vector<int>& ptr, const std::vector<Spec>& ent, const std::vector<int>& ulist, int n_param,
             std::vector<PlRec>& out, int* ne_max) {
  out.clear();
  *ne_max = 0;
  if (n_param < 1) return false;
  auto fail = [&] {   // (nothing half-built is left behind)
    out.clear();
    *ne_max = 0;
    return false;
  };
  out.assign(pl_padded(ulist.size()), pl_pad_rec());
  for (size_t u = 0; u < ulist.size(); ++u) {
    const int a = ulist[u];
    const int ne = ptr[a + 1] - ptr[a];
    if (ne > PL_NE) return fail();
    for (int e = 0; e < ne; ++e) {
      const Spec& s = ent[ptr[a] + e];
      if (s.kind != PL_KIND_POWERLAW || s.i0 >= n_param || s.i1 >= n_param) return fail();
      out[u].e[e] = PlEntry{s.i0 < 0 ? -1 : s.i0, s.i1 < 0 ? -1 : s.i1, s.v0, s.v1, s.a, s.lnf, s.lnfyr};
    }
    out[u].ne = ne;
    if (ne > *ne_max) *ne_max = ne;
  }
  return true;
}

// ---- unit decode ------------------------------------------------------------
// Unit u = u0 + v of a launch (v < n <= 2^31 its workgroup's place) is pulsar
// p = u / B, sample b = u % B.  With p0 = u0 / B and r0 = u0 % B formed on the
// host, t = r0 + v < 2^32 and p = p0 + t / B, b = t % B -- and t / B by one
// 32-bit multiply-high and one correction: with M = min(floor(2^32 / B),
// 2^32 - 1), q' = (t M) >> 32 is t / B or one less (2^32 / B - M <= 1, so
// t / B - t M / 2^32 <= t / 2^32 < 1).
struct UnitDec {
  int32_t p0 = 0;
  uint32_t r0 = 0, magic = 0;
};

inline UnitDec unit_dec_make(long long u0, int B) {
  UnitDec d;
  d.p0 = (int32_t)(u0 / B);
  d.r0 = (uint32_t)(u0 % B);
  const uint64_t m = (uint64_t(1) << 32) / (uint32_t)B;
  d.magic = m > 0xffffffffull ? 0xffffffffu : (uint32_t)m;
  return d;
}

EWH_SPEC_HD inline void unit_decode(const UnitDec& d, uint32_t v, uint32_t B, int& p, int& b) {
  const uint32_t t = d.r0 + v;
  uint32_t q = (uint32_t)(((uint64_t)t * d.magic) >> 32);
  uint32_t r = t - q * B;
  if (r >= B) {
    q += 1;
    r -= B;
  }
  p = d.p0 + (int)q;
  b = (int)r;
}

}  // namespace ewh_dev
