// ewarp_dev.h — shared device primitives, job structs, and the register LDL^T
// factorisation that chol_small, chol_small_pl, chol_partial, chol_lat,
// chol_big and chol_wide build on.  Every translation unit of libewarp_hip.so
// includes it (through ewarp_launch.h, the units' launchers); what only one
// unit instantiates lives in that unit (contract.hip, chol_big.hip).
// The register factorisation (Split .. panel_ldl_row, chol_mfma_kernel and its
// spectrum prologues) stays in this file, not behind an #include of its own:
// the benchmark hashes this file and chol_small.hip as the headline kernel's source
// and reports its measured traffic (profiles/pmc_chol.json) only while the hash matches.
// The width constants and the factorisation route: ewarp_route.h (no HIP
// dependency).  See ewarp_hip.hip for the formulation.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "ewarp_hip.h"
#include "ewarp_route.h"
#include "ewarp_spec.h"

namespace ewh_dev {

// thread-local error message of the C ABI (defined in ewarp_hip.hip)
int set_err(int code, const std::string& msg);

#define EWH_HIP(expr)                                                          \
  do {                                                                         \
    hipError_t e_ = (expr);                                                    \
    if (e_ != hipSuccess)                                                      \
      return ::ewh_dev::set_err(EWH_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

// Device-side invariant checks of the debug build (`make debug`: -DEWH_DEBUG,
// build/libewarp_hip_debug.so; SURVEY.md §5's sanitizer row for device code).
// A violated check prints its site, block and thread, then traps -- a bounded
// failure with a location instead of a hang or a silent out-of-bounds access.
// Sites: every work-grab / spin loop carries an iteration bound (and the
// grab a full exec mask), and LDS / scratch / operand indices are checked
// against their allocations in chol_dd, chol_wide and contract_xr.  The
// product and dev builds compile the checks away.
#ifdef EWH_DEBUG
#define EWH_DCHECK(cond, what)                                                                           \
  do {                                                                                                   \
    if (!(cond)) {                                                                                       \
      printf("EWH_DCHECK failed: %s (%s:%d) block %d,%d thread %d\n", what, __FILE__, __LINE__,          \
             (int)blockIdx.x, (int)blockIdx.y, (int)threadIdx.x);                                        \
      __builtin_trap();                                                                                  \
    }                                                                                                    \
  } while (0)
#else
#define EWH_DCHECK(cond, what) \
  do {                         \
  } while (0)
#endif

constexpr int default_waves(int nb) { return nb <= 8 ? 2 : 1; }
typedef double v4d __attribute__((ext_vector_type(4)));
// global-address-space view of a device pointer: loads through it are
// global_load (vmcnt only), not flat_load, whose lgkmcnt share makes every
// ds_bpermute wait (s_waitcnt lgkmcnt(0)) for all matrix loads in flight
typedef const __attribute__((address_space(1))) double* gdptr;

// ----------------------------------------------------------------------------
// device helpers
// ----------------------------------------------------------------------------
// compile-time loop: f(std::integral_constant<int, I>) for I in [B, E)
template <int B, int E, typename F>
__host__ __device__ __forceinline__ void static_for(F&& f) {
  if constexpr (B < E) {
    f(std::integral_constant<int, B>{});
    static_for<B + 1, E>(f);
  }
}

__device__ __forceinline__ double pref_val(const ewh_pref& r, const double* th) {
  return r.idx >= 0 ? th[r.idx] : r.cval;
}

// Device form of one spectral entry (built from ewh_spec_entry at create).
// phi is evaluated as one exp of a sum of logs:
//   POWERLAW  A^2/(12 pi^2) fyr^(g-3) f^-g df = exp(a + 2 ln10 lgA + (g-3) ln fyr - g ln f)
//   TURNOVER  A^2/(12 pi^2) fyr^-3 ((f+fc)/fyr)^-g df
//             = exp(a + 2 ln10 lgA - 3 ln fyr - g (ln(f+fc) - ln fyr)),  fc = 10^fc if fc < 0
//   FREESPEC  10^(2 rho) = exp(2 ln10 rho)
//   CONST     v0
// with a = ln(df / (12 pi^2)); the same quantities as [ent] utils.powerlaw,
// the reference's powerlaw_bpl (enterprise_models.py:553-563) and
// [ent] gp_priors.free_spectrum, re-associated (relative error ~1e-14).
struct DSpec {
  int kind, col;
  int i0, i1, i2, pad_;
  double v0, v1, v2;     // constant values of the three parameters
  double a, lnf, lnfyr, f;
};

__device__ __forceinline__ double dpar(int idx, double cval, const double* th) {
  return idx >= 0 ? th[idx] : cval;
}

constexpr double LN10 = 2.302585092994045684;

// spec_phi_body: the arithmetic; spec_phi: an out-of-line copy for the schur and
// LDS-Cholesky kernels (ROCm 7.2 clang crashes in the CGSCC inliner when one
// inlined copy serves both); the register-resident kernels inline the body
// (a call there reserves a scratch frame the unrolled factorisation then
// spills into).
// (the power law's one expression: spec_phi_body and the fixed-form prologue
// of chol_mfma_kernel evaluate it with the same association, bit for bit)
__device__ __forceinline__ double powerlaw_phi(double a, double lgA, double gam, double lnfyr, double lnf) {
  return exp(a + 2.0 * LN10 * lgA + (gam - 3.0) * lnfyr - gam * lnf);
}

template <int DUMMY = 0>
__device__ __forceinline__ double spec_phi_body(const DSpec& s, const double* th) {
  switch (s.kind) {
    case EWH_SPEC_POWERLAW: {
      const double lgA = dpar(s.i0, s.v0, th), gam = dpar(s.i1, s.v1, th);
      return powerlaw_phi(s.a, lgA, gam, s.lnfyr, s.lnf);
    }
    case EWH_SPEC_TURNOVER: {
      const double lgA = dpar(s.i0, s.v0, th), gam = dpar(s.i1, s.v1, th);
      double fc = dpar(s.i2, s.v2, th);
      if (fc < 0) fc = exp(LN10 * fc);
      return exp(s.a + 2.0 * LN10 * lgA - 3.0 * s.lnfyr - gam * (log(s.f + fc) - s.lnfyr));
    }
    case EWH_SPEC_FREESPEC:
      return exp(2.0 * LN10 * dpar(s.i0, s.v0, th));
    case EWH_SPEC_CONST:
      return s.v0;
    default:
      return __builtin_nan("");
  }
}

static __device__ __noinline__ double spec_phi(const DSpec& s, const double* th) { return spec_phi_body(s, th); }

// phi of column a: the CSR sum of its entries, from 0.0 in entry order (host twin:
// ewarp_cpu.cpp).  col_phi calls spec_phi; col_phi<true> inlines the body (as above).
template <bool BODY = false>
__device__ __forceinline__ double col_phi(const int* col_ptr, const DSpec* spec, int a, const double* th) {
  double ph = 0.0;
  for (int e = col_ptr[a]; e < col_ptr[a + 1]; ++e) ph += BODY ? spec_phi_body(spec[e], th) : spec_phi(spec[e], th);
  return ph;
}

// running log-determinant without a log per term: product of frexp mantissas
// (each in [0.5, 1): >= 2^-1000 after 1000 terms, no underflow) + exponent sum.
struct LogAcc {
  double mant = 1.0;
  int ex = 0;
  __device__ __forceinline__ void add(double x) {
    mant *= __builtin_amdgcn_frexp_mant(x);   // <= 1000 terms: no renormalisation needed
    ex += __builtin_amdgcn_frexp_exp(x);
  }
  // the product of two accumulators (o of a few terms: no underflow)
  __device__ __forceinline__ void merge(const LogAcc& o) {
    mant *= o.mant;
    ex += o.ex;
  }
  __device__ __forceinline__ double value() const { return log(mant) + ex * 0.69314718055994530942; }
};

__device__ __forceinline__ double readlane_d(double x, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(x), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(x), lane);
  return __hiloint2double(hi, lo);
}

// 1/sqrt(a): hardware estimate + two Newton steps (~1 ulp).
__device__ __forceinline__ double rsqrt_nr(double a) {
  double y = __builtin_amdgcn_rsq(a);
  const double h = 0.5 * a;
  double t = fma(-h * y, y, 0.5);
  y = fma(y, t, y);
  t = fma(-h * y, y, 0.5);
  return fma(y, t, y);
}

// XCD-aware unit order: the dispatcher deals workgroup b to XCD b % 8, so
// XCD x gets the contiguous unit range [x q, (x+1) q) (q = n / 8; the n % 8
// tail maps to itself).  Units are pulsar-major, so each pulsar's reduced
// matrix is fetched into ~one XCD's L2 instead of all eight.
__device__ __forceinline__ long long xcd_unit(unsigned b, unsigned n) {
  const unsigned q = n >> 3;
  return b < (q << 3) ? (long long)(b & 7) * q + (b >> 3) : (long long)b;
}

// 1/a: hardware estimate + two Newton steps (~1 ulp).
__device__ __forceinline__ double rcp_nr(double a) {
  double y = __builtin_amdgcn_rcp(a);
  double e = fma(-a, y, 1.0);
  y = fma(y, e, y);
  e = fma(-a, y, 1.0);
  return fma(y, e, y);
}

// x / a with one cubic correction: y = rcp(a) (|e| = |1 - a y| < 2^-24),
// x / a = x y (1 + e + e^2) + O(e^3).  t = x y forms beside e, so the chain
// after the estimate is e -> s -> result (3 ops; x * rcp_nr(a) is 5) and the
// whole quotient is 5 fp64 VALU ops instead of 6.  ~1 ulp.
__device__ __forceinline__ double div_fast(double x, double a) {
  const double y = __builtin_amdgcn_rcp(a);
  const double e = fma(-a, y, 1.0);
  const double t = x * y;
  const double s = fma(e, e, e);
  return fma(t, s, t);
}

// 1/sqrt(a) with one cubic correction: e = 1 - a y^2,
// a^-1/2 = y (1 + e/2 + 3e^2/8) + O(e^3).  6 fp64 VALU ops (rsqrt_nr is 8).
__device__ __forceinline__ double rsqrt_fast(double a) {
  const double y = __builtin_amdgcn_rsq(a);
  const double e = fma(-(a * y), y, 1.0);
  const double s = e * fma(0.375, e, 0.5);
  return fma(y, s, y);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// 256-thread block sum; `scratch` holds >= 4 doubles.
static __device__ double block_sum256(double v, double* scratch) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) scratch[w] = v;
  __syncthreads();
  double t = scratch[0] + scratch[1] + scratch[2] + scratch[3];
  __syncthreads();
  return t;
}

// ----------------------------------------------------------------------------
// double-double helpers (Knuth TwoSum, TwoProd by fma; Dekker / Bailey
// normalisation): value = hi + lo with |lo| <= ulp(hi) / 2.
// Every error-free transformation is compiled with floating-point
// contraction off (`#pragma clang fp contract(off)`, round 6): hipcc's device
// default (-ffp-contract=fast) fused `s = hi + x * y` into one fma while the
// TwoSum error term still used the separately rounded product, which left
// every "double-double" kernel (gram_dd, schur, chol_dd) only about fp64-
// accurate -- the ~15x strict floor of the device's double-double twin
// against the CPU double-double reference on C3 prior draws, and indefinite
// C4 refinements (ISA: v_fma_f64 in place of v_add_f64)
// ----------------------------------------------------------------------------
struct dd {
  double hi, lo;
};
__device__ __forceinline__ dd dd_two_sum(double a, double b) {
#pragma clang fp contract(off)
  const double s = a + b, bp = s - a;
  return {s, (a - (s - bp)) + (b - bp)};
}
__device__ __forceinline__ dd dd_fast(double a, double b) {   // |a| >= |b|
#pragma clang fp contract(off)
  const double s = a + b;
  return {s, b - (s - a)};
}
__device__ __forceinline__ dd dd_add(dd x, dd y) {
#pragma clang fp contract(off)
  const dd s = dd_two_sum(x.hi, y.hi);
  return dd_fast(s.hi, s.lo + x.lo + y.lo);
}
// x + y with both parts TwoSum-ed (the accurate double-double sum: a
// relative error of ~2^-106 of |x + y| even under cancellation, which the
// sloppy dd_add above does not bound)
__device__ __forceinline__ dd dd_add_ieee(dd x, dd y) {
#pragma clang fp contract(off)
  dd s = dd_two_sum(x.hi, y.hi);
  const dd t = dd_two_sum(x.lo, y.lo);
  s = dd_fast(s.hi, s.lo + t.hi);
  return dd_fast(s.hi, s.lo + t.lo);
}
__device__ __forceinline__ dd dd_mul(dd x, dd y) {
#pragma clang fp contract(off)
  const double p = x.hi * y.hi;
  return dd_fast(p, fma(x.hi, y.hi, -p) + (x.hi * y.lo + x.lo * y.hi));
}
__device__ __forceinline__ dd dd_div(dd x, dd y) {          // one Newton correction of x.hi / y.hi
#pragma clang fp contract(off)
  const double q = x.hi / y.hi;
  const dd r = dd_add(x, dd_mul({-q, 0.0}, y));
  return dd_fast(q, r.hi / y.hi);
}
__device__ __forceinline__ dd dd_sqrt(dd x) {
#pragma clang fp contract(off)
  const double r = sqrt(x.hi);
  const dd e = dd_add(x, dd_mul({-r, 0.0}, {r, 0.0}));
  return dd_fast(r, e.hi / (2.0 * r));
}

// ----------------------------------------------------------------------------
// per-pulsar device tables
// ----------------------------------------------------------------------------
struct PsrDev {
  int n_toa, m, ld, nb;      // varying layout: T_aug is n_toa x ld, r at ld-1
  int n_epoch;
  const double* T;           // n_toa x ld row-major
  const double* sig2;        // toaerr^2
  const int* efac_slot;
  const int* equad_slot;
  const ewh_pref* slots;
  const int* ep_start;
  const int* ep_stop;
  const int* ep_slot;
  int n_bgroup;              // theta-dependent chromatic basis groups (0: none)
  const int* col_bgroup;     // ld entries, -1 = fixed column
  const double* ln_chrom;    // n_toa: ln(1400 / nu)
  const ewh_pref* bgroup;    // n_bgroup: chromatic index per group
  const int* toa_ep;         // n_toa + CT_ROWS (ewarp_launch.h): 2 e + (last TOA of e), -1 = no epoch (pad rows -1)
};

// One factorisation job: (pulsar, sample) -> matrix + diagonal update.
struct CholJob {
  const double* mats;        // matrix of sample b at mats + (b - b_off) * mstride
  long long mstride;         // 0: one matrix shared by every sample
  int ld;                    // leading dimension (= 16 * NB)
  int mreal;                 // columns with a phi entry (0..mreal-1); r at ld-1
  const int* col_ptr;        // CSR of spectral entries over mreal columns
  const DSpec* spec;
  const double* K;           // additive constant, K[(b - b_off) * kstride]
  int kstride;
  int fail;                  // 1: lead block not positive definite -> -inf
  // fixed white noise: columns sharing one spectrum (the sin / cos pair of a
  // frequency) -- rep[a] = the first column with the same entries, ulist =
  // the nu representatives; the prologue then forms each spectrum once
  const int* rep = nullptr;
  const int* ulist = nullptr;
  int nu = 0;
  // the same, staged for the register kernels' prologue: one record per
  // distinct spectrum with its entries inline (URec), and per column the
  // record it takes (urep, -1 = no entry); theta is read from LDS.  One
  // global-load level instead of four (ulist -> col_ptr -> spec -> theta).
  // NULL: the CSR path (a spectrum with more than URec::NE entries)
  const struct URec* urec = nullptr;
  const int* urep = nullptr;
  // the theta entries the records reference, staged alone (their DSpec
  // indices are positions in this list); 0: the whole theta row is staged
  int ntidx = 0;
  int tidx[16] = {};
  // the low part of a double-double matrix (chol_dd_kernel; same stride as
  // mats), or NULL
  const double* mats_lo = nullptr;
  // the reversed verify pass's input fl(hi + 2 lo), formed once where the
  // matrix is shared by every sample (mstride 0: the fixed-WN cache), or NULL
  // (the pass then forms it from mats and mats_lo at every load)
  const double* mats_rev = nullptr;
  // the operand images of a shared matrix of at most MFMA_NB_MAX blocks
  // (mstride 0: the fixed-WN cache; img_index below): its upper-triangle
  // blocks in chol_mfma_kernel's register layout, in the stored order (img)
  // and, for a frame with a dead slice (front_dead >= 1), in the front-pad
  // order of the job's own pad count (img_front); NULL: read mats
  const double* img = nullptr;
  const double* img_front = nullptr;
  // the staged records again in the fixed form of the product kernel's
  // prologue (ewarp_spec.h PlRec: power laws only, theta positions in the
  // sample's own row, padded to whole waves), pl_ne the most entries any of
  // them has; NULL: the job does not qualify (pl_pack) -- the launch then
  // takes the interpreted prologue
  const PlRec* pl = nullptr;
  int pl_ne = 0;
};

// Units [u0, u0 + n) (u = pulsar * B + sample) of one factorisation launch, as
// the host launchers pass them on (unpacked at the kernel launch): sample b in
// slot b - b_off of its job, ldth doubles of theta per sample, terms to units[u]
struct UnitSpan {
  const CholJob* jobs; int B; long long u0, n; int b_off;
  const double* theta; int ldth; double* units; hipStream_t st;
};

// one distinct spectrum of a fixed-WN job: phi = sum of its ne entries
struct URec {
  static constexpr int NE = 3;
  DSpec e[NE];
  int ne, pad_[3];
};
static_assert(PL_NE == URec::NE, "a compact record (ewarp_spec.h) holds what a staged record holds");
constexpr int STAGE_THETA_MAX = 512;   // theta row staged in LDS up to this many parameters
constexpr int TIDX_MAX = 16;           // CholJob::tidx

// ----------------------------------------------------------------------------
// batched factorisation, MFMA register-blocked: one wave (64 lanes) per unit.
// The upper triangle of the LD x LD matrix (LD = 16 NB) is held as 16x16
// blocks in the v_mfma_f64_16x16x4_f64 C/D layout (lane l, reg r <-> row
// (l>>4) + 4r, col l&15).  A = U^T U (upper, as LAPACK dpotrf 'U' behind
// scipy cho_factor) by a blocked LDL^T: per block row bb the 16x16 diagonal
// block is eliminated (panel), the rest of the block row becomes
// V = L^-1 A_bj = E^T A_bj by four MFMAs per block (E = L^-T, built by the
// panel's column operations), the rows are scaled to U = D^-1/2 V, and the
// trailing blocks take A_ij -= U_bi^T U_bj by four MFMAs each with no data
// movement -- register s of a C/D-layout block IS the MFMA A / B operand of
// k-slice s.
//
// Three phases keep at most 26 blocks live for NB = 8 (36 in a plain
// right-looking order): (1) factor block rows 0..H-1 (H = NB/2) with the
// trailing update restricted to those rows; (2) load the trailing A22
// triangle and apply the H panel rows to it; (3) factor A22.  Same
// arithmetic, re-ordered (left-looking at the 2x2 block level).
// ----------------------------------------------------------------------------
template <int NB, bool FULL = false>
struct Split {
  // FULL (dev A/B, one wave per SIMD): the whole triangle resident, plain
  // right-looking order (phases 2 and 3 empty)
  static constexpr int H = FULL ? NB : NB == 8 ? 3 : NB / 2;
  static constexpr int M = NB - H;                    // A22 block order
  static constexpr int n1 = H * NB - H * (H - 1) / 2; // blocks (i < H, j >= i)
  static constexpr int n2 = M * (M + 1) / 2;          // blocks (H <= i <= j)
  static constexpr int i1(int i, int j) { return i * NB - (i * (i - 1)) / 2 + (j - i); }
  static constexpr int i2(int i, int j) { return (i - H) * M - ((i - H) * (i - H - 1)) / 2 + (j - i); }
};

// A -= U_i^T U_j : four f64 MFMAs.  For the f64 MFMAs of gfx940+ the last
// (blgp) field is the neg modifier (bit 0 negates A: `neg:[1,0,0]`), so no
// v_xor per negated operand.  S0: the first k-slice to issue (the slices
// before it are rows of zeros: the dead slices of block row 0, below).
template <int S0 = 0>
__device__ __forceinline__ void syrk_update(v4d& C, const v4d& Ui, const v4d& Uj) {
#pragma unroll
  for (int sk = S0; sk < 4; ++sk) C = __builtin_amdgcn_mfma_f64_16x16x4f64(Ui[sk], Uj[sk], C, 0, 0, 1);
}

// ----------------------------------------------------------------------------
// Working order of the register kernels without kept blocks (chol_mfma_kernel
// KEEP == 0, chol_lat_kernel): pads in front.  The stored reduced matrix is
// [mreal real columns | s pads | r] in a frame of LD = 16 NB (s = LD - 1 -
// mreal; a pad is an identity row and column).  At the end of the frame the
// pads are waste in the M / N dimension of every MFMA of the last block
// column; the kernels factor [s pads | real columns | r] instead, where the
// pads are waste in the K dimension of block row 0: its first DEAD = s / 4
// k-slices are rows of zeros, and an MFMA over such a slice is not issued.
// Only the loads know: front_src maps a working index to the stored one (a
// leading pad to one of the stored pads, whose 0 / 1 it reads: every address
// lies in the frame), and phi^-1 is staged in working order.  A symmetric
// permutation: the same lnL up to the order of the pivots.
// ----------------------------------------------------------------------------
constexpr int FRONT_PAD_MAX = 15;      // pads the map moves (a frame of minimal NB has no more)
__host__ __device__ constexpr int front_pads(int ld, int mreal) {
  const int s = ld - 1 - mreal;
  return s < 0 ? 0 : s > FRONT_PAD_MAX ? FRONT_PAD_MAX : s;   // (further pads stay behind the real columns)
}
__host__ __device__ constexpr int front_src(int w, int s, int ld) {
  return w < s ? ld - 1 - s + w : w == ld - 1 ? w : w - s;   // (the last s stored pads; r; the columns before them)
}
// the dead slices of a frame (host: the instantiation of a launch is the
// smallest over its jobs; any DEAD <= s / 4 gives the same values)
constexpr int front_dead(int ld, int mreal) { return front_pads(ld, mreal) / 4; }
// The instantiation both register kernels (and chol_wide_kernel's forward
// pass) take for a launch whose jobs share `dead` dead slices: 1..3, the
// front-pad order with that DEAD; -1, the stored order -- where there is no
// slice to drop (under 4 pads: the code is what it was before the front-pad
// order existed), and at six blocks with one, whose instantiation does not
// fit 256 VGPRs and is not built.  One rule for every launcher, so the
// kernels of one handle always work in the same order.
constexpr int front_inst(int nb, int dead) {
  return dead <= 0 || (nb == 6 && dead == 1) ? -1 : dead > 3 ? 3 : dead;
}
// The instantiations with the fixed-form spectrum prologue (PL) that are
// built: inst as front_inst returns it.  <6, DEAD 2, IMG, PL> and <8, stored
// order, IMG, PL> spill at two waves per SIMD as chol_small_pl.hip compiles
// them (12 / 16 bytes of scratch per lane; profiles/r16/
// resources_chol_small.txt) and are not: such a launch keeps the interpreted
// prologue.  (The figure is the translation unit's, not the kernel's alone:
// <6, DEAD 2, IMG, PL> instantiated by itself in a unit comes out at 252
// VGPRs without scratch; beside the unit's other instantiations it does not.)
constexpr bool pl_built(int nb, int inst, bool img) {
  return !(img && ((nb == 6 && inst == 2) || (nb == 8 && inst == -1)));
}
// For every mreal of a frame of nb blocks: front_src maps the working
// positions [s, LD) onto the stored real columns and r one to one and in
// order, and every leading pad onto a stored pad of its own, never onto a
// real column or r -- a permutation of the frame (checked at compile time
// where the register kernels are built: chol_small.hip)
constexpr bool front_map_ok(int nb) {
  const int ld = 16 * nb;
  for (int mreal = 0; mreal < ld; ++mreal) {
    const int s = front_pads(ld, mreal);
    int next = 0;                          // the stored index the next real position must take
    for (int w = 0; w < ld; ++w) {
      const int a = front_src(w, s, ld);
      if (w < s) {
        if (a != ld - 1 - s + w || a < mreal || a >= ld - 1) return false;
      } else if (w == ld - 1) {
        if (a != ld - 1 || next != ld - 1 - s) return false;
      } else {
        if (a != next++ || a >= ld - 1) return false;
      }
    }
    // a frame of minimal NB (mreal >= LD - 16): every real column is reached
    if (mreal >= ld - 16 && ld - 1 - s != mreal) return false;
  }
  return true;
}

// Element (16 BI + q + 4 R, 16 BJ + c) of the working order from the stored
// matrix A.  The stored index of a real entry is the working one minus s, so
// every lane's address is one per-lane base plus a compile-time offset, as in
// the stored order; only block row / column 0 (pads) and NB - 1 (r stays at
// LD - 1) select.
// Af = A - (s LD + s), the base moved back by s rows and s columns (formed
// once per unit, front_base; s in 0..15 is uniform): the element is then
// Af[K + lane part], K a compile-time offset and the lane part q LD + c that
// of the stored order -- a scalar base and a small non-negative lane offset.
template <int NB, typename Ptr>
__device__ __forceinline__ Ptr front_base(Ptr A, int s) { return A - (s * (16 * NB) + s); }
// the lane part of element (16 bi + q + 4 r, 16 bj + c) of a frame of nb blocks
__host__ __device__ constexpr unsigned front_lane(int nb, int bi, int bj, int r, int q, int c, int s) {
  const int ld = 16 * nb;
  unsigned lp = (unsigned)(q * ld + c);
  if (bi == nb - 1 && r == 3) lp += q == 3 ? (unsigned)(s * ld) : 0u;   // the r row
  if (bj == nb - 1) lp += c == 15 ? (unsigned)s : 0u;                   // the r column
  // a leading pad reads its stored pad (front_src: LD - 1 - s + w, which is
  // LD - 1 + w from the moved base), an identity row and column: an address
  // select, in range, and no select on the value
  if (bi == 0) lp += q + 4 * r < s ? (unsigned)((ld - 1) * ld) : 0u;
  if (bj == 0) lp += c < s ? (unsigned)(ld - 1) : 0u;
  return lp;
}
// the offset from the moved base that is a compile-time constant
constexpr int front_const(int nb, int bi, int bj, int r) { return (16 * bi + 4 * r) * 16 * nb + 16 * bj; }
// The address the kernels form is the one front_src names: for every pad
// count, lane and register of the blocks at the frame's edges and one inside
// (the only cases the arithmetic tells apart), Af[K + lane part] is
// A[front_src(row) LD + front_src(col)] (compile time: chol_small.hip)
constexpr bool front_elem_ok(int nb) {
  const int ld = 16 * nb;
  for (int s = 0; s <= FRONT_PAD_MAX; ++s)
    for (int bi = 0; bi < nb; ++bi) {
      if (bi > 1 && bi < nb - 2) continue;
      for (int bj = bi; bj < nb; ++bj) {
        if (bj > 1 && bj < nb - 2) continue;
        for (int r = 0; r < 4; ++r)
          for (int q = 0; q < 4; ++q)
            for (int c = 0; c < 16; ++c) {
              const int row = 16 * bi + q + 4 * r, col = 16 * bj + c;
              const long long got = (long long)front_const(nb, bi, bj, r) - (s * ld + s) + front_lane(nb, bi, bj, r, q, c, s);
              if (got != (long long)front_src(row, s, ld) * ld + front_src(col, s, ld)) return false;
            }
      }
    }
  return true;
}
template <int NB, int DEAD, int BI, int BJ, int R, typename Ptr>
__device__ __forceinline__ double front_elem(Ptr Af, int q, int c, int s) {
  static_assert(DEAD >= 0 && DEAD <= 3, "front-pad order: 0..3 dead slices");
  static_assert(BJ >= BI, "front-pad order: upper-triangle blocks");
  if constexpr (BI == 0 && R < DEAD) {
    return (BJ == 0 && q + 4 * R == c) ? 1.0 : 0.0;    // a dead slice: pads only, no load
  } else {
    const Ptr Ak = Af + front_const(NB, BI, BJ, R);
    return Ak[front_lane(NB, BI, BJ, R, q, c, s)];
  }
}

// ----------------------------------------------------------------------------
// Operand image of a matrix that every sample shares (fixed white noise: the
// cached S_p; CholJob::img, img_front).  The layout change from the row-major
// stored matrix to chol_mfma_kernel's registers -- and the front-pad
// permutation -- is the same for every sample and every call, so it is done
// once where the matrix is formed (white.hip operand_image_kernel): the
// NB (NB + 1) / 2 upper-triangle blocks in row-major block order (the order the
// kernel consumes them), each block as [half h][lane][2 doubles], half h
// holding registers 2 h and 2 h + 1 of lane (q, c) = elements
// (16 bi + q + 4 r, 16 bj + c).  A half is contiguous across the lanes: the
// kernel reads a block as two 16-byte loads per lane, each a coalesced 1 KiB,
// at compile-time offsets from one per-lane base.  The pads are the stored
// identity rows and columns; no select on a value.
// ----------------------------------------------------------------------------
struct ImgPos {
  int bi, bj, r, lane;
};
constexpr int img_block(int nb, int bi, int bj) { return bi * nb - bi * (bi - 1) / 2 + (bj - bi); }
constexpr long long img_doubles(int nb) { return 256LL * (nb * (nb + 1) / 2); }
// (nb, bi, bj, r, lane) -> offset in the image: what the loads use ...
__host__ __device__ constexpr long long img_index(int nb, int bi, int bj, int r, int lane) {
  return 256LL * (bi * nb - bi * (bi - 1) / 2 + (bj - bi)) + 128 * (r >> 1) + 2 * lane + (r & 1);
}
// ... and its inverse: what the builder uses (one thread per image position)
__host__ __device__ constexpr ImgPos img_at(int nb, long long k) {
  int t = (int)(k / 256), bi = 0;
  while (t >= nb - bi) t -= nb - bi++;
  const int w = (int)(k % 256);
  return ImgPos{bi, bi + t, 2 * (w >> 7) + (w & 1), (w >> 1) & 63};
}
// the stored element an image position holds, in the working order with s
// leading pads (s = 0: the stored order)
__host__ __device__ constexpr long long img_src(int nb, ImgPos e, int s) {
  const int ld = 16 * nb;
  return (long long)front_src(16 * e.bi + (e.lane >> 4) + 4 * e.r, s, ld) * ld + front_src(16 * e.bj + (e.lane & 15), s, ld);
}
// The map is a bijection onto [0, img_doubles) -- every (block, register,
// lane) in image order takes the next offset, and img_at inverts it -- and for
// every pad count the element the builder stores at an offset is the one
// front_src names for that register and lane, which is the plain element in
// the stored order and the address front_elem forms in the front-pad order
// (compile time: chol_small.hip)
constexpr bool img_map_ok(int nb) {
  const int ld = 16 * nb;
  for (int s = 0; s <= FRONT_PAD_MAX; ++s) {
    long long k = 0;
    for (int bi = 0; bi < nb; ++bi)
      for (int bj = bi; bj < nb; ++bj) {
        if (img_block(nb, bi, bj) != (int)(k / 256)) return false;
        for (int h = 0; h < 2; ++h)
          for (int lane = 0; lane < 64; ++lane)
            for (int e = 0; e < 2; ++e) {
              const int r = 2 * h + e, q = lane >> 4, c = lane & 15;
              const long long idx = img_index(nb, bi, bj, r, lane);
              if (idx != k++) return false;
              const ImgPos p = img_at(nb, idx);
              if (p.bi != bi || p.bj != bj || p.r != r || p.lane != lane) return false;
              const int row = 16 * bi + q + 4 * r, col = 16 * bj + c;
              const long long src = img_src(nb, p, s);
              if (src != (long long)front_src(row, s, ld) * ld + front_src(col, s, ld)) return false;
              if (s == 0 && src != (long long)row * ld + col) return false;
              if (src != (long long)front_const(nb, bi, bj, r) - (s * ld + s) + front_lane(nb, bi, bj, r, q, c, s))
                return false;
            }
      }
    if (k != img_doubles(nb)) return false;
  }
  return true;
}

// lane (q, c) <- lane (q, K) of its 16-lane row (DPP row_newbcast, gfx90a+):
// one v_mov_b64_dpp (64-bit DPP takes row_newbcast; with bound_ctrl there is
// no `old` operand to materialise).
template <int K>
__device__ __forceinline__ double row_newbcast(double x) {
  const long v = __builtin_amdgcn_mov_dpp(__builtin_bit_cast(long, x), 0x150 + K, 0xf, 0xf, true);
  return __builtin_bit_cast(double, v);
}

// One pivot k = 4 KR + KQ of the panel as fused DP-ALU DPP multiply-adds,
// each ONE v_fmac_f64_dpp whose src0 is read from lane k of its 16-lane row
// (row_newbcast: column k of the lane's row):
//  * row update A[q+4r][c] += A[q+4r][k] * nw of register KR in the 16-lane
//    rows q > KQ (row_mask) and, with FULLROWS (the one-level panel of round
//    2, dev A/B only), of every register r > KR;
//  * with DOE the column operation E[q+4r][c] += E[q+4r][k] * nwm on the
//    registers r <= KR (nwm is 0 in the lanes c <= k).
// Hazards the compiler cannot see inside the asm: (1) a DPP source must be
// written >= 2 wait states before it is read -- one statement per pivot, and
// the next pivot's statement needs nw, whose chain (readlane of this
// statement's output, rcp, 3 fma) lies in between; the first pivot of a
// sub-panel (NOP) follows the compiler's E initialisation or the sub-panel
// MFMA's copy-out, hence its s_nop; (2) E is an MFMA operand (V = E^T A)
// right after the last column operation (k = 14): a trailing s_nop covers
// VALU-write -> MFMA-read.  Only live registers (A, E) are written, so no
// in-flight MFMA reads them as a dead source.
template <int K, int KR, int KQ, bool DOE, bool NOP, bool FULLROWS>
__device__ __forceinline__ void pivot_fused(v4d& A, v4d& E, double nw, double nwm) {
  double a0 = A[0], a1 = A[1], a2 = A[2], a3 = A[3];
  double e0 = E[0], e1 = E[1], e2 = E[2], e3 = E[3];
  constexpr int RM = (0xf << (KQ + 1)) & 0xf;   // rows q > KQ of register KR
  asm(".if %[nop]\n s_nop 1\n .endif\n"
      ".if %[fr]\n"
      " .if %[kr] < 1\n v_fmac_f64_dpp %[a1], %[a1], %[nw] row_newbcast:%[k] row_mask:0xf bank_mask:0xf\n .endif\n"
      " .if %[kr] < 2\n v_fmac_f64_dpp %[a2], %[a2], %[nw] row_newbcast:%[k] row_mask:0xf bank_mask:0xf\n .endif\n"
      " .if %[kr] < 3\n v_fmac_f64_dpp %[a3], %[a3], %[nw] row_newbcast:%[k] row_mask:0xf bank_mask:0xf\n .endif\n"
      ".endif\n"
      ".if %[rm] != 0\n"
      " .if %[kr] == 0\n v_fmac_f64_dpp %[a0], %[a0], %[nw] row_newbcast:%[k] row_mask:%[rm] bank_mask:0xf\n .endif\n"
      " .if %[kr] == 1\n v_fmac_f64_dpp %[a1], %[a1], %[nw] row_newbcast:%[k] row_mask:%[rm] bank_mask:0xf\n .endif\n"
      " .if %[kr] == 2\n v_fmac_f64_dpp %[a2], %[a2], %[nw] row_newbcast:%[k] row_mask:%[rm] bank_mask:0xf\n .endif\n"
      " .if %[kr] == 3\n v_fmac_f64_dpp %[a3], %[a3], %[nw] row_newbcast:%[k] row_mask:%[rm] bank_mask:0xf\n .endif\n"
      ".endif\n"
      ".if %[doe]\n"
      " v_fmac_f64_dpp %[e0], %[e0], %[nwm] row_newbcast:%[k] row_mask:0xf bank_mask:0xf\n"
      " .if %[kr] >= 1\n v_fmac_f64_dpp %[e1], %[e1], %[nwm] row_newbcast:%[k] row_mask:0xf bank_mask:0xf\n .endif\n"
      " .if %[kr] >= 2\n v_fmac_f64_dpp %[e2], %[e2], %[nwm] row_newbcast:%[k] row_mask:0xf bank_mask:0xf\n .endif\n"
      " .if %[kr] >= 3\n v_fmac_f64_dpp %[e3], %[e3], %[nwm] row_newbcast:%[k] row_mask:0xf bank_mask:0xf\n .endif\n"
      " .if %[k] == 14\n s_nop 7\n s_nop 7\n .endif\n"
      ".endif\n"
      : [a0] "+v"(a0), [a1] "+v"(a1), [a2] "+v"(a2), [a3] "+v"(a3), [e0] "+v"(e0), [e1] "+v"(e1), [e2] "+v"(e2),
        [e3] "+v"(e3)
      : [nw] "v"(nw), [nwm] "v"(nwm), [k] "i"(K), [kr] "i"(KR), [rm] "i"(RM), [doe] "i"(DOE ? 1 : 0),
        [nop] "i"(NOP ? 1 : 0), [fr] "i"(FULLROWS ? 1 : 0));
  A[0] = a0; A[1] = a1; A[2] = a2; A[3] = a3;
  E[0] = e0; E[1] = e1; E[2] = e2; E[3] = e3;
}

// upper-triangle blocks (i, j), r0 <= i < r1, i <= j < NB, enumerated row by
// row: count, and block t -> (i, j)
constexpr int tri_count(int nb, int r0, int r1) {
  int n = 0;
  for (int i = r0; i < r1; ++i) n += nb - i;
  return n;
}
constexpr int tri_row(int nb, int r0, int t) {
  int i = r0;
  while (t >= nb - i) { t -= nb - i; ++i; }
  return i;
}
constexpr int tri_col(int nb, int r0, int t) {
  int i = r0;
  while (t >= nb - i) { t -= nb - i; ++i; }
  return i + t;
}

// Hooks of the panel: the dense diagonal-tile kernel of the correlated
// factorisation exports E = L^-T of each 16-row sub-block (before V = E^T A)
// and each register's row scale D^-1/2.
struct NoHook {
  __device__ __forceinline__ void on_e(const v4d&) const {}
  __device__ __forceinline__ void on_scale(int, double) const {}
};


// PANEL_2L on the diagonal block D of block row BB (of NB): its 16 pivots in
// four sub-panels of 4 rows (register s of the C/D layout).  Inside a
// sub-panel the pivots update only register s (rows q > kq) and E; after it,
// the sub-panel's rows are scaled to U_s = D_s^-1/2 V_s and the rows below
// take D -= U_s^T U_s by ONE MFMA.  Leaves E = L^-T (column operations) and
// the row scales rsr[r] = D^-1/2 of register r; accumulates log d_k (lane
// c == 0 of each row) and d_k > 0.  RL: the last column of block row NB-1 is
// the residual (not pivoted); klim: pivots >= klim of that block row are pads
// (identity rows and columns: pivot 1, every multiplier 0) and are skipped.
// Rr[j] += Rr[j] (lane k of its row) * nw for the rows j in (KQ, 4): the
// replicated copies of the sub-panel's rows, updated exactly as pivot_fused
// updates their originals in register kr (bit-identical copies).  The
// leading s_nop covers a DPP read of a VGPR the previous pivot wrote.
template <int K, int KQ>
__device__ __forceinline__ void repl_rows_update(double (&Rr)[4], double nw) {
  double r1 = Rr[1], r2 = Rr[2], r3 = Rr[3];
  asm(" s_nop 1\n"
      ".if %[kq] < 1\n v_fmac_f64_dpp %[r1], %[r1], %[nw] row_newbcast:%[k] row_mask:0xf bank_mask:0xf\n .endif\n"
      ".if %[kq] < 2\n v_fmac_f64_dpp %[r2], %[r2], %[nw] row_newbcast:%[k] row_mask:0xf bank_mask:0xf\n .endif\n"
      ".if %[kq] < 3\n v_fmac_f64_dpp %[r3], %[r3], %[nw] row_newbcast:%[k] row_mask:0xf bank_mask:0xf\n .endif\n"
      : [r1] "+v"(r1), [r2] "+v"(r2), [r3] "+v"(r3)
      : [nw] "v"(nw), [k] "i"(K), [kq] "i"(KQ));
  Rr[1] = r1; Rr[2] = r2; Rr[3] = r3;
}

// REPL (the latency kernel): the four rows of each sub-panel are broadcast to
// every 16-lane row once, when the sub-panel starts (4 ds_bpermute pairs in
// flight together), and kept up to date by repl_rows_update, so no pivot
// waits on a ds_bpermute round trip: 6 more DPP multiply-adds per sub-panel
// for a shorter dependent chain.  Same values bit for bit.
// The pivot d = A[k][k] is read by two v_readlane_b32 from the register
// itself, in parallel with the ds_bpermute that broadcasts row k.  (Round 3
// A/B, profiles/r03e/chol_ab.log: taking d from the broadcast row by one
// v_mov_b64_dpp -- one instruction less per pivot -- put the bpermute's
// latency in front of the reciprocal: 3.70 vs 3.65 ms per launch; masking
// only the high dword of the E multiplier -- one v_cndmask_b32 less -- 3.70
// ms.  Neither is kept.)
// __shfl(x, 16 KQ + c) with the lane address formed at the use: an empty asm
// keeps the compiler from carrying the address of one KQ across the whole
// kernel (in the headline kernel's last block row it did, and spilled it:
// VERDICT r03 item 2)
template <int KQ>
__device__ __forceinline__ double shfl_row_fresh(double x, int c) {
  int a = c << 2;
  asm volatile("" : "+v"(a));
  const int lo = __builtin_amdgcn_ds_bpermute(a + 64 * KQ, __double2loint(x));
  const int hi = __builtin_amdgcn_ds_bpermute(a + 64 * KQ, __double2hiint(x));
  return __hiloint2double(hi, lo);
}

// The four rows of a sub-panel register x (row j = lanes 16 j .. 16 j + 15)
// broadcast to every 16-lane row by gfx950's lane-swap instructions:
// v_permlane32_swap of x with a copy gives rows (0, 1, 0, 1) and (2, 3, 2, 3),
// v_permlane16_swap of each with a copy the four broadcasts -- 6 swaps on the
// VALU instead of 8 ds_bpermute round trips through the LDS crossbar.  Same
// values bit for bit.  (In the batched kernel, issue-bound, the extra copies
// and replica updates cost more than the crossbar: 3.65 -> 3.76 ms, DESIGN.md
// §4a; the latency kernel waits on the round trip instead.)
__device__ __forceinline__ void bcast_rows4(double x, double (&R)[4]) {
  const int lo = __double2loint(x), hi = __double2hiint(x);
  const auto l32 = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
  const auto h32 = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
  const auto l01 = __builtin_amdgcn_permlane16_swap(l32[0], l32[0], false, false);
  const auto h01 = __builtin_amdgcn_permlane16_swap(h32[0], h32[0], false, false);
  const auto l23 = __builtin_amdgcn_permlane16_swap(l32[1], l32[1], false, false);
  const auto h23 = __builtin_amdgcn_permlane16_swap(h32[1], h32[1], false, false);
  R[0] = __hiloint2double(h01[0], l01[0]);
  R[1] = __hiloint2double(h01[1], l01[1]);
  R[2] = __hiloint2double(h23[0], l23[0]);
  R[3] = __hiloint2double(h23[1], l23[1]);
}

// REPL: 0 = each pivot row broadcast by ds_bpermute when it is needed (the
// batched kernels); 1 = the sub-panel's four rows replicated up front by
// ds_bpermute; 2 = replicated by the lane swaps of bcast_rows4
// DEAD >= 0: the front-pad working order (front_src).  The last block row
// then holds 15 real columns and r (no pad pivots, klim unused), and the pads
// lead block row 0: its first DEAD sub-panels are pads for every job of the
// launch and have no code at all -- neither pivots, scale nor MFMA -- and in
// sub-panel DEAD the pivots k < kfirst are skipped (wave-uniform, as klim).
// Any pivot of that sub-panel may then be the first one executed after the
// compiler's E initialisation, so each carries the leading s_nop.  A job with
// more pads than the launch's 4 DEAD + 3 pivots the rest as what they are,
// identity rows (pivot 1, every multiplier 0): each skip is a branch whose
// join copies the block's registers, which costs more than it saves.
// DEAD < 0: the stored order (pads behind the real columns, klim).
// BLKLD (the register kernels without kept blocks, in either order): the
// block's four log d terms are multiplied up on their own and merged into ldet
// once, so chol_lat_kernel -- whose diagonal blocks are factored by different
// waves -- folds the same per-block products in the same order and returns
// the same log-determinant bit for bit.  A leading pad's pivot (1) is never
// added, so the value does not depend on DEAD either.
template <int NB, int BB, bool RL, int REPL = 0, int DEAD = -1, bool BLKLD = (DEAD >= 0)>
__device__ __forceinline__ void diag_factor_2l(v4d& D, v4d& E, double (&rsr)[4], int q, int c, LogAcc& ldet,
                                               bool& ok, int klim, int kfirst = 0) {
  constexpr bool LASTR = RL && BB == NB - 1;          // block row holding the residual
  constexpr bool FRONT = DEAD >= 0;
  constexpr bool LEADR = FRONT && BB == 0;            // block row holding the leading pads
  constexpr bool KLIM = LASTR && !FRONT;              // block row holding trailing pads
  LogAcc lb;
  static_for<0, 4>([&](auto R) {
    constexpr int r = decltype(R)::value;
    E[r] = (q + 4 * r == c) ? 1.0 : 0.0;
    rsr[r] = 1.0;
  });
  // (Folding the row scales into E's columns instead -- E D^-1/2, one gather,
  // four multiplies -- was tried in round 3: the wide chol_big_kernel and the
  // one-wave NB = 9 kernel then faulted with an illegal address on the GPU;
  // not kept.)
  static_for<0, 4>([&](auto KR) {
    constexpr int kr = decltype(KR)::value;
    constexpr int nk = (LASTR && kr == 3) ? 3 : 4;   // the r column is not pivoted
    if constexpr (!(LEADR && kr < DEAD)) {           // (a dead sub-panel: pads only)
    double Rr[4];
    if constexpr (REPL == 1) {
      static_for<0, 4>([&](auto J) { Rr[decltype(J)::value] = __shfl(D[kr], 16 * decltype(J)::value + c); });
    } else if constexpr (REPL == 2) {
      bcast_rows4(D[kr], Rr);
    }
    static_for<0, nk>([&](auto KQc) {
      constexpr int kq = decltype(KQc)::value;
      constexpr int k = 4 * kr + kq;
      if constexpr (KLIM) {
        if (k >= klim) return;                         // wave-uniform: pad pivots
      }
      if constexpr (LEADR && kr == DEAD) {
        if (k < kfirst) return;                        // wave-uniform: leading pad pivots
      }
      constexpr bool doe = !LASTR && k < 15;
      const double xk = REPL ? Rr[kq] : LASTR ? shfl_row_fresh<kq>(D[kr], c) : __shfl(D[kr], 16 * kq + c);  // A[k][c]
      const double d = REPL ? readlane_d(Rr[kq], k) : readlane_d(D[kr], 16 * kq + k);
      const double nw = div_fast(-xk, d);
      const double nwm = (doe && c > k) ? nw : 0.0;
      pivot_fused<k, kr, kq, doe, kq == 0 || (LEADR && kr == DEAD), false>(D, E, nw, nwm);
      if constexpr (REPL && kq < 3) repl_rows_update<k, kq>(Rr, nw);
    });
    // sub-panel kr done: lane (q, c) takes the pivot of row 4 kr + q (lane
    // (q, 4 kr + q)): log-det, positivity, row scale; U_s = D_s^-1/2 V_s and
    // the rows below take D -= U_s^T U_s (one MFMA, in place: registers
    // <= kr are not read again)
    auto sub = [&]() {
      const double dg = __shfl(D[kr], 17 * q + 4 * kr);
      const double dv = (LASTR && kr == 3 && q == 3) ? 1.0 : dg;   // (the r row)
      ok = ok && (dv > 0.0);
      if (c == 0 && !(LEADR && 4 * kr + q < kfirst)) {   // (not a leading pad's 1)
        if constexpr (BLKLD) lb.add(dv); else ldet.add(dv);
      }
      if constexpr (!(LASTR && kr == 3)) {
        const double rs = rsqrt_fast(dv);
        rsr[kr] = rs;
        if constexpr (kr < 3) {
          const double u = D[kr] * rs;
          D = __builtin_amdgcn_mfma_f64_16x16x4f64(u, u, D, 0, 0, 1);
        }
      }
    };
    if constexpr (KLIM) {
      if (4 * kr < klim) sub();                      // (a sub-panel of pads: pivots 1, no update)
    } else {
      sub();
    }
    }
  });
  if constexpr (BLKLD) ldet.merge(lb);
}

// The rest of a block row after its diagonal block: V = E^T A (4 MFMAs)
// (row_v_2l), rows scaled to U = D^-1/2 V (row r of register r times rsr[r]).
// S0: the first k-slice to issue (block row 0 of the front-pad order: rows
// 0 .. 4 S0 - 1 of A are pads, zero outside the diagonal block).
template <int S0 = 0>
__device__ __forceinline__ void row_v_2l(const v4d& E, v4d& A) {
  v4d acc = {0.0, 0.0, 0.0, 0.0};
  static_for<S0, 4>([&](auto S) {
    constexpr int s = decltype(S)::value;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(E[s], A[s], acc, 0, 0, 0);
  });
  A = acc;
}

// The LDL^T panel of block row BB over the blocks blk(j), j = BB..NB-1 (C/D
// layout, upper triangle; the diagonal block is held in full): eliminates
// the diagonal block pivot by pivot (row k broadcast to every 16-lane row by
// ds_bpermute, pivot by readlane, quotient by div_fast), builds E = L^-T by
// column operations, turns the rest of the row into V = E^T A (4 MFMAs per
// block) and scales it to U = D^-1/2 V.  Accumulates log d_k (packed: one
// lane per row) and d_k > 0.
// RL: the last column of block row NB-1 is the residual (not pivoted), as in
// the per-pulsar factorisations; false for a plain SPD block (the dense
// cross-pulsar factorisation's diagonal tiles).
// PANEL_2L (the default): diag_factor_2l + row_v_2l + the row scales.  PANEL_1L (dev A/B
// only: the round-2 default): every pivot updates every register r >= kr by
// VALU.  The update A[i][c] -= A[i][k] (A[k][c] / d) rounds differently from
// its mirror A[c][i] -= A[c][k] (A[k][i] / d), so the lower triangle drifts
// from the upper one and, on ill-conditioned draws, the Schur complements
// drift with it (tests/golden: c1_turnover sample 0 at 4e3x the strict bound
// vs 22x for PANEL_2L and 79x for enterprise's LAPACK order).
// PACK (PANEL_1L): the row scales D^-1/2 of all 16 rows by one gather + one
// rsqrt per lane (lane (q, c) takes d of row q + 4 (c/4)); else one per
// register (the phase-1 form of chol_mfma_kernel<8>, where the packed
// temporaries spill).
// klim: pivots >= klim of the last block row are pads and are skipped.
constexpr int PANEL_1L = 11;
constexpr int PANEL_2L = 25;

// DEAD >= 0 (PANEL_2L): the front-pad working order with DEAD dead slices in
// block row 0, whose pivots k < kfirst are pads (diag_factor_2l); klim unused.
template <int NB, int ALG, bool RL, bool PACK, int DEAD = -1, bool BLKLD = (DEAD >= 0), typename BBt, typename Blk,
          typename Hook = NoHook>
__device__ __forceinline__ void panel_ldl_row(BBt BBc, Blk&& blk, int q, int c, LogAcc& ldet, bool& ok,
                                              const Hook& hook = Hook{}, int klim = 16, int kfirst = 0) {
  constexpr int bb = decltype(BBc)::value;
  static_assert(ALG == PANEL_1L || ALG == PANEL_2L, "unknown panel form");
  static_assert(DEAD < 0 || ALG == PANEL_2L, "the front-pad order exists for the two-level panel");
  constexpr bool LASTR = RL && bb == NB - 1;          // block row holding the residual
  if constexpr (ALG == PANEL_2L) {
    v4d E;
    double rsr[4];
    diag_factor_2l<NB, bb, RL, 0, DEAD, BLKLD>(blk(BBc), E, rsr, q, c, ldet, ok, klim, kfirst);
    if constexpr (!LASTR) {
      hook.on_e(E);
      static_for<bb + 1, NB>([&](auto JJ) { row_v_2l<(bb == 0 && DEAD > 0) ? DEAD : 0>(E, blk(JJ)); });
      static_for<0, 4>([&](auto R) {
        constexpr int r = decltype(R)::value;
        hook.on_scale(r, rsr[r]);
        static_for<bb + 1, NB>([&](auto JJ) { blk(JJ)[r] *= rsr[r]; });
      });
    }
    return;
  } else {
  v4d E;
  static_for<0, 4>([&](auto R) {
    constexpr int r = decltype(R)::value;
    E[r] = (q + 4 * r == c) ? 1.0 : 0.0;
  });
  static_for<0, 4>([&](auto KR) {
    constexpr int kr = decltype(KR)::value;
    constexpr int nk = (LASTR && kr == 3) ? 3 : 4;   // the r column is not pivoted
    static_for<0, nk>([&](auto KQc) {
      constexpr int kq = decltype(KQc)::value;
      constexpr int k = 4 * kr + kq;
      if constexpr (LASTR) {
        if (k >= klim) return;                         // wave-uniform: pad pivots
      }
      constexpr bool doe = !LASTR && k < 15;
      const double xk = __shfl(blk(BBc)[kr], 16 * kq + c);    // A[k][c]
      const double d = readlane_d(blk(BBc)[kr], 16 * kq + k);
      const double nw = div_fast(-xk, d);
      const double nwm = (doe && c > k) ? nw : 0.0;
      pivot_fused<k, kr, kq, doe, k == 0, true>(blk(BBc), E, nw, nwm);
    });
  });
  if constexpr (!LASTR) hook.on_e(E);
  static_for<bb + 1, NB>([&](auto JJ) {
    v4d acc = {0.0, 0.0, 0.0, 0.0};
    static_for<0, 4>([&](auto S) {
      constexpr int s = decltype(S)::value;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(E[s], blk(JJ)[s], acc, 0, 0, 0);
    });
    blk(JJ) = acc;
  });
  // rows of the block row -> U = d^-1/2 V (the diagonal block itself is not
  // needed after its panel; the last block row has nothing to scale)
  if constexpr (PACK) {
    // d of row q + 4r read from the diagonal (lane 17q + 4r); lane (q, c)
    // takes d of row q + 4 (c/4) -- held in register c/4 of lane
    // (q, q + 4 (c/4)), whose own c/4 is the same -- so one gather, one rsqrt
    // and one log-det term (lanes c % 4 == 0) cover all 16 rows; register r
    // then takes its rows' scale from lane (q, 4r) by DPP
    const int cr = c >> 2;
    const double own = cr == 0 ? blk(BBc)[0] : cr == 1 ? blk(BBc)[1] : cr == 2 ? blk(BBc)[2] : blk(BBc)[3];
    double dv = __shfl(own, 17 * q + 4 * cr);
    if constexpr (LASTR) dv = (q == 3 && cr == 3) ? 1.0 : dv;
    ok = ok && (dv > 0.0);
    if ((c & 3) == 0) ldet.add(dv);
    if constexpr (!LASTR) {
      const double rsp = rsqrt_nr(dv);
      static_for<0, 4>([&](auto R) {
        constexpr int r = decltype(R)::value;
        const double rs = row_newbcast<4 * r>(rsp);
        hook.on_scale(r, rs);
        static_for<bb + 1, NB>([&](auto JJ) { blk(JJ)[r] *= rs; });
      });
    }
  } else {
    static_for<0, 4>([&](auto R) {
      constexpr int r = decltype(R)::value;
      const bool rrow = LASTR && r == 3 && q == 3;
      const double dg = __shfl(blk(BBc)[r], 17 * q + 4 * r);
      const double dv = rrow ? 1.0 : dg;
      ok = ok && (dv > 0.0);
      if (c == 0) ldet.add(dv);
      if constexpr (!LASTR) {
        const double rs = rsqrt_nr(dv);
        hook.on_scale(r, rs);
        static_for<bb + 1, NB>([&](auto JJ) { blk(JJ)[r] *= rs; });
      }
    });
  }
  }
}

// KEEP > 0 (correlated common process): only block rows 0..NB-KEEP-1 (the
// pulsar's own columns) are factored; the trailing KEEP x KEEP blocks (the
// common columns + r: their Schur complement S^G, d', rho) are written to
// keep_out[(p * keep_bs + (b - keep_b0))] as a dense (16 KEEP)^2 square
// (pulsar-major: a device's pulsar range is one contiguous slice, the unit an
// all-gather moves), and
// the unit term is the local part K - 1/2 log|Sigma_LL| - 1/2 log|phi_L|.
#ifdef EWH_DEV
// STAMP (dev diagnostics): s_memtime stamps at the phase boundaries of the
// units with blockIdx < STAMP_UNITS (ewh_dev_stamps)
constexpr int STAMP_UNITS = 4096, STAMP_N = 24;
static __device__ long long g_stamps[STAMP_UNITS * STAMP_N];
#endif

// W: waves per SIMD the register budget is cut for (2 -> 256 VGPRs: the NB = 8
// three-phase kernel fits, so two units share each SIMD and one's MFMAs
// overlap the other's VALU / LDS latency).  Block row 0 is loaded before the
// spectra are formed (its latency overlaps the prologue); with fixed white
// noise each distinct spectrum is formed once (the sin / cos columns of a
// frequency share one: J.rep / J.ulist) and shared through LDS; the last
// panel's pad pivots are skipped.
// DEAD >= 0 (KEEP == 0, PANEL_2L): the front-pad working order (front_src) with
// DEAD dead k-slices in block row 0 -- every job of the launch has at least
// 4 DEAD pads; DEAD < 0: the stored order (launches without a dead slice,
// front_inst; the kept-block form; the dev A/B variants 17 and 26).
// IMG (KEEP == 0): the matrix is read from the job's operand image (img_index:
// img_front in the front-pad order, img in the stored order) -- two 16-byte
// loads per block at compile-time offsets from one per-lane base, the dead
// slices' registers with them; every job of the launch carries that image.
// The same values reach the same registers as from J.mats.
// PL (KEEP == 0, PANEL_2L): the fixed-form spectrum prologue -- every job of the
// launch carries compact power-law records (CholJob::pl, ewarp_spec.h).  Each
// lane loads one record in 16-byte pieces and gathers its theta entries from
// the sample's row in global memory, all issued beside block row 0 and ahead
// of the first wait; the entries are evaluated straight-line up to the
// launch's largest count (wave-uniform; padded entries add an exact +0.0), and
// the unit is decoded in 32-bit scalar arithmetic from ud (unit_decode; u0 is
// not read).  Same expression, exp, order of sums, division and LogAcc order
// as the interpreted prologue below: the same bits.
template <int NB, int W, int ALG = PANEL_2L, bool STAMP = false, int KEEP = 0, bool FULL = false, int DEAD = -1,
          bool IMG = false, bool PL = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(W, W)))
void chol_mfma_kernel(const CholJob* __restrict__ jobs, int B, long long u0, int b_off,
                      const double* __restrict__ theta, int ldth, double* __restrict__ out_units,
                      double* __restrict__ keep_out, int keep_b0, int keep_bs, UnitDec ud) {
#ifdef EWH_DEV
  long long stp[STAMP_N];
#define EWH_STAMP(I)                                            \
  if constexpr (STAMP) {                                        \
    __builtin_amdgcn_sched_barrier(0);                          \
    stp[(I)] = (long long)__builtin_amdgcn_s_memtime();         \
    __builtin_amdgcn_sched_barrier(0);                          \
  }
#else
  static_assert(!STAMP, "phase stamps exist only in the dev library");
#define EWH_STAMP(I)
#endif
  EWH_STAMP(0)
  constexpr int LD = 16 * NB;
  using S = Split<NB, FULL>;
  constexpr int H = S::H;
  static_assert(!FULL || KEEP == 0, "the FULL form has no kept blocks");
  static_assert(FULL || NB - KEEP >= H, "kept blocks must lie in the phase-3 triangle");
  __shared__ double phinv[LD];
  __shared__ double phs[LD];
  const int lane = threadIdx.x;
  const int q = lane >> 4, c = lane & 15;
  static_assert(!PL || (KEEP == 0 && ALG == PANEL_2L && !FULL), "fixed-form prologue: the product form without kept blocks");
  int p, b;
  if constexpr (PL) {
    unit_decode(ud, (uint32_t)xcd_unit(blockIdx.x, gridDim.x), (uint32_t)B, p, b);
  } else {
    const long long u = u0 + xcd_unit(blockIdx.x, gridDim.x);
    p = (int)(u / B);
    b = (int)(u % B);
  }
  const CholJob J = jobs[p];
  [[maybe_unused]] const gdptr A = (gdptr)(J.mats + (long long)(b - b_off) * J.mstride);
  const double* th = theta + (long long)b * ldth;
  constexpr bool FRONT = DEAD >= 0;
  static_assert(!FRONT || (KEEP == 0 && ALG == PANEL_2L), "front-pad order: the full two-level factorisation");
  static_assert(!IMG || (KEEP == 0 && ALG == PANEL_2L && !FULL), "operand image: the product form without kept blocks");
  // the image as 16-byte pairs, from this lane's pair on: block t, half h at I[128 t + 64 h]
  typedef double v2d __attribute__((ext_vector_type(2)));
  typedef const __attribute__((address_space(1))) v2d* gv2ptr;
  [[maybe_unused]] const gv2ptr I = IMG ? (gv2ptr)(FRONT ? J.img_front : J.img) + lane : nullptr;
  EWH_DCHECK(!IMG || (I != nullptr && J.mstride == 0), "chol_mfma: the job carries the launch's operand image");
  [[maybe_unused]] auto image_block = [&](auto BI, auto BJ, v4d& v) {
    constexpr long long o = img_index(NB, decltype(BI)::value, decltype(BJ)::value, 0, 0) / 2;
    static_assert(img_index(NB, decltype(BI)::value, decltype(BJ)::value, 2, 0) / 2 == o + 64, "image halves 1 KiB apart");
    const v2d lo = I[o], hi = I[o + 64];
    v[0] = lo.x;
    v[1] = lo.y;
    v[2] = hi.x;
    v[3] = hi.y;
  };
  // the log-determinant by per-block products, as chol_lat_kernel folds it
  // (diag_factor_2l BLKLD): the product kernels and their stamped twin
  constexpr bool BLKLD = KEEP == 0 && ALG == PANEL_2L && !FULL;
  // leading pads of the working order (0: the stored order)
  // (clamped after the readfirstlane: the compiler sees 0 <= s <= 15)
  const int s = FRONT ? front_pads(LD, __builtin_amdgcn_readfirstlane(J.mreal)) : 0;
  EWH_DCHECK(!FRONT || s >= 4 * DEAD, "chol_mfma: the job has the launch's dead slices");
  [[maybe_unused]] const gdptr Af = front_base<NB>(A, s);

  // fixed-form prologue, loads: this lane's record of every trip (nine 16-byte
  // pieces at compile-time offsets from one base; a trip past the job's
  // records is skipped, wave-uniformly) and its columns' record indices --
  // issued ahead of block row 0, so the wait for them leaves the matrix loads
  // in flight
  constexpr int CT = (LD + 63) / 64;        // column trips
  constexpr int RT = (LD - 1 + 63) / 64;    // record trips: nu <= mreal <= LD - 1
  [[maybe_unused]] v2d rc[RT][PL_PIECES - 1] = {};
  [[maybe_unused]] int urp[CT];
  [[maybe_unused]] const int pl_nu = PL ? __builtin_amdgcn_readfirstlane(J.nu) : 0;
  [[maybe_unused]] const int pl_ne = PL ? __builtin_amdgcn_readfirstlane(J.pl_ne) : 0;
  if constexpr (PL) {
    EWH_DCHECK(J.pl != nullptr && J.urep != nullptr && pl_ne <= PL_NE && pl_nu <= 64 * RT,
               "chol_mfma: the job carries the launch's compact records");
    const gv2ptr R = (gv2ptr)J.pl + lane * PL_PIECES;
    static_for<0, RT>([&](auto T) {
      constexpr int t = decltype(T)::value;
      if (t == 0 || 64 * t < pl_nu)
        static_for<0, PL_PIECES - 1>([&](auto K) { rc[t][decltype(K)::value] = R[64 * t * PL_PIECES + decltype(K)::value]; });
    });
    // (phi^-1 is staged in working order: position 64 i + lane takes stored
    // column 64 i + lane - s; the leading pads and r carry none)
    static_for<0, CT>([&](auto I) {
      constexpr int i = decltype(I)::value;
      const int a = 64 * i + lane - s;
      urp[i] = (a >= 0 && a < J.mreal) ? J.urep[a] : -1;
    });
  }

  v4d pre[NB];
  static_for<0, NB>([&](auto BJ) {
    if constexpr (IMG) {
      image_block(std::integral_constant<int, 0>{}, BJ, pre[decltype(BJ)::value]);
    } else {
      static_for<0, 4>([&](auto R) {
        constexpr int r = decltype(R)::value;
        if constexpr (FRONT) {
          pre[decltype(BJ)::value][r] = front_elem<NB, DEAD, 0, decltype(BJ)::value, r>(Af, q, c, s);
        } else {
          pre[decltype(BJ)::value][r] = A[(long long)(q + 4 * r) * LD + 16 * decltype(BJ)::value + c];
        }
      });
    }
  });
  // log|phi| is summed into the per-lane log-det accumulator (one log() at
  // the end of the kernel)
  LogAcc ldet;
  if constexpr (PL) {
    // fixed form: every entry a power law.  The theta gathers of a trip are
    // issued together (index clamped to 0 where the constant applies: the row
    // has a parameter, pl_pack), then the entries are evaluated up to the
    // launch's largest count and summed from 0.0 in entry order
    __shared__ double phq[64 * RT];
    const gdptr thg = (gdptr)th;
    static_for<0, RT>([&](auto T) {
      constexpr int t = decltype(T)::value;
      if (t == 0 || 64 * t < pl_nu) {
        // (the gathers of all three entries, unguarded: one wait for the lot;
        // a padded entry reads theta[0] and selects its constant)
        double lgA[PL_NE], gam[PL_NE];
        static_for<0, PL_NE>([&](auto E) {
          constexpr int e = decltype(E)::value;
          const v2d h = rc[t][pl_piece(e, 0)];
          const int i0 = __double2loint(h.x), i1 = __double2hiint(h.x);
          const double t0 = thg[max(i0, 0)], t1 = thg[max(i1, 0)];
          lgA[e] = i0 >= 0 ? t0 : h.y;
          gam[e] = i1 >= 0 ? t1 : rc[t][pl_piece(e, 1)].x;
        });
        double ph = 0.0;
        static_for<0, PL_NE>([&](auto E) {
          constexpr int e = decltype(E)::value;
          if (e == 0 || e < pl_ne)
            ph += powerlaw_phi(rc[t][pl_piece(e, 1)].y, lgA[e], gam[e], rc[t][pl_piece(e, 2)].y, rc[t][pl_piece(e, 2)].x);
        });
        phq[64 * t + lane] = ph;
      }
    });
    __syncthreads();
    static_for<0, CT>([&](auto I) {
      constexpr int i = decltype(I)::value;
      const int a = 64 * i + lane;
      if (a < LD) {
        double pi = 0.0;
        if (urp[i] >= 0) {
          const double ph = phq[urp[i]];
          pi = 1.0 / ph;
          ldet.add(ph);
        }
        phinv[a] = pi;
      }
    });
  } else if (J.urec != nullptr && (J.ntidx > 0 || ldth <= STAGE_THETA_MAX)) {
    // staged: the theta entries the spectra read (or the whole row) -> LDS,
    // each distinct spectrum's record by its lane, every column's record
    // index -- all loads issued together
    __shared__ double ths[STAGE_THETA_MAX];
    // (phi^-1 is staged in working order: position 64 i + lane takes stored
    // column 64 i + lane - s; the leading pads and r carry none)
    int ur[(LD + 63) / 64];
    static_for<0, (LD + 63) / 64>([&](auto I) {
      constexpr int i = decltype(I)::value;
      const int a = 64 * i + lane - s;
      ur[i] = (a >= 0 && a < J.mreal) ? J.urep[a] : -1;
    });
    if (J.ntidx > 0) {
      if (lane < J.ntidx) ths[lane] = th[jobs[p].tidx[lane]];
    } else {
      for (int i = lane; i < ldth; i += 64) ths[i] = th[i];
    }
    __syncthreads();
    for (int u = lane; u < J.nu; u += 64) {
      const URec& R = J.urec[u];
      double ph = 0.0;
      for (int e = 0; e < R.ne; ++e) ph += spec_phi_body(R.e[e], ths);
      phs[u] = ph;
    }
    __syncthreads();
    static_for<0, (LD + 63) / 64>([&](auto I) {
      constexpr int i = decltype(I)::value;
      const int a = 64 * i + lane;
      if (a < LD) {
        double pi = 0.0;
        if (ur[i] >= 0) {
          const double ph = phs[ur[i]];
          pi = 1.0 / ph;
          ldet.add(ph);
        }
        phinv[a] = pi;
      }
    });
  } else {
    const bool dedup = J.rep != nullptr;
    if (dedup) {
      for (int i = lane; i < J.nu; i += 64) {
        const int a = J.ulist[i];
        phs[a] = col_phi<true>(J.col_ptr, J.spec, a, th);
      }
      __syncthreads();
    }
    for (int wa = lane; wa < LD; wa += 64) {
      const int a = wa - s;                                   // (working position wa: stored column a)
      double pi = 0.0;
      if (a >= 0 && a < J.mreal && J.col_ptr[a] < J.col_ptr[a + 1]) {   // (pads carry no entry)
        const double ph = dedup ? phs[J.rep[a]] : col_phi<true>(J.col_ptr, J.spec, a, th);
        pi = 1.0 / ph;
        ldet.add(ph);
      }
      phinv[wa] = pi;
    }
  }
  __syncthreads();
  EWH_STAMP(1)

  auto load_block = [&](auto BI, auto BJ, v4d& v) {
    constexpr int bi = decltype(BI)::value, bj = decltype(BJ)::value;
    if constexpr (IMG) {
      image_block(BI, BJ, v);
    } else {
      static_for<0, 4>([&](auto R) {
        constexpr int r = decltype(R)::value;
        if constexpr (FRONT) {
          v[r] = front_elem<NB, DEAD, bi, bj, r>(Af, q, c, s);
        } else {
          v[r] = A[(long long)(16 * bi + q + 4 * r) * LD + 16 * bj + c];
        }
      });
    }
    if constexpr (bi == bj) {
      const double pd = phinv[16 * bi + c];
      static_for<0, 4>([&](auto R) {
        constexpr int r = decltype(R)::value;
        v[r] += (q + 4 * r == c) ? pd : 0.0;
      });
    }
  };

  bool ok = true;
  constexpr bool SKIPPAD = KEEP == 0 && !FRONT;      // (front-pad order: the pads lead block row 0, s of them)
  const int klast = SKIPPAD ? __builtin_amdgcn_readfirstlane(J.mreal - 16 * (NB - 1)) : 16;
  constexpr int D0 = FRONT ? DEAD : 0;               // slices of block row 0 that are not issued
  // phase 1 (NB = 8): per-register row scales (the packed form's temporaries spill there)
  constexpr bool PACK1 = NB != 8;

  // ---- phase 1: block rows 0..H-1 ----
  v4d U1[S::n1 > 0 ? S::n1 : 1];
  static_for<0, H>([&](auto BI) {
    constexpr int bi = decltype(BI)::value;
    static_for<bi, NB>([&](auto BJ) {
      constexpr int bj = decltype(BJ)::value;
      if constexpr (bi == 0) {
        U1[S::i1(0, bj)] = pre[bj];
        if constexpr (bj == 0) {
          const double pd = phinv[c];
          static_for<0, 4>([&](auto R) {
            constexpr int r = decltype(R)::value;
            U1[S::i1(0, 0)][r] += (q + 4 * r == c) ? pd : 0.0;
          });
        }
      } else {
        load_block(BI, BJ, U1[S::i1(bi, bj)]);
      }
    });
  });
  static_for<0, H>([&](auto BBc) {
    constexpr int bb = decltype(BBc)::value;
    panel_ldl_row<NB, ALG, KEEP == 0, PACK1, DEAD, BLKLD>(
        BBc, [&](auto JJ) -> v4d& { return U1[S::i1(bb, decltype(JJ)::value)]; }, q, c, ldet, ok, NoHook{}, klast, s);
    EWH_STAMP(2 + 2 * bb)
    static_for<bb + 1, H>([&](auto II) {
      constexpr int i = decltype(II)::value;
      static_for<i, NB>([&](auto JJ) {
        constexpr int j = decltype(JJ)::value;
        syrk_update<bb == 0 ? D0 : 0>(U1[S::i1(i, j)], U1[S::i1(bb, i)], U1[S::i1(bb, j)]);
      });
    });
    EWH_STAMP(3 + 2 * bb)
  });
  // ---- phase 2: A22 -= U12^T U12 ----
  // block by block in row order: U1 column i is dead once row i of A22 is done
  v4d U2[S::n2 > 0 ? S::n2 : 1];
  static_for<H, NB>([&](auto II) {
    constexpr int i = decltype(II)::value;
    static_for<i, NB>([&](auto JJ) {
      constexpr int j = decltype(JJ)::value;
      load_block(II, JJ, U2[S::i2(i, j)]);
      static_for<0, H>([&](auto BBc) {
        constexpr int bb = decltype(BBc)::value;
        syrk_update<bb == 0 ? D0 : 0>(U2[S::i2(i, j)], U1[S::i1(bb, i)], U1[S::i1(bb, j)]);
      });
    });
  });
  EWH_STAMP(2 + 2 * H)
  // ---- phase 3: factor A22 (up to the kept blocks) ----
  static_for<H, NB - KEEP>([&](auto BBc) {
    constexpr int bb = decltype(BBc)::value;
    panel_ldl_row<NB, ALG, KEEP == 0, true, DEAD, BLKLD>(
        BBc, [&](auto JJ) -> v4d& { return U2[S::i2(bb, decltype(JJ)::value)]; }, q, c, ldet, ok, NoHook{}, klast, s);
    EWH_STAMP(3 + 2 * bb)
    static_for<bb + 1, NB>([&](auto II) {
      constexpr int i = decltype(II)::value;
      static_for<i, NB>([&](auto JJ) {
        constexpr int j = decltype(JJ)::value;
        syrk_update(U2[S::i2(i, j)], U2[S::i2(bb, i)], U2[S::i2(bb, j)]);
      });
    });
    EWH_STAMP(4 + 2 * bb)
  });
  double qv = 0.0;
  if constexpr (FULL) {
    qv = readlane_d(U1[S::i1(NB - 1, NB - 1)][3], 63);
  } else if constexpr (KEEP == 0) {
    qv = readlane_d(U2[S::i2(NB - 1, NB - 1)][3], 63);
  } else {
    constexpr int KD = 16 * KEEP;
    double* ko = keep_out + ((long long)p * keep_bs + (b - keep_b0)) * (KD * KD);
    // (debug build: the unit's kept square is one of its pulsar's keep_bs
    // slots; rows and columns below are 16 (i - (NB - KEEP)) + 0..15 < KD)
    EWH_DCHECK(keep_out != nullptr && b - keep_b0 >= 0 && b - keep_b0 < keep_bs,
               "chol_mfma: kept block inside its pulsar's slice");
    int qo = q, co = c;                     // (store addresses formed here, not hoisted: they spilled)
    asm volatile("" : "+v"(qo), "+v"(co));
    static_for<NB - KEEP, NB>([&](auto II) {
      constexpr int i = decltype(II)::value;
      static_for<i, NB>([&](auto JJ) {
        constexpr int j = decltype(JJ)::value;
        static_for<0, 4>([&](auto RR) {
          constexpr int r = decltype(RR)::value;
          const int row = 16 * (i - (NB - KEEP)) + qo + 4 * r, col = 16 * (j - (NB - KEEP)) + co;
          const double v = U2[S::i2(i, j)][r];
          if (i != j || row <= col) {
            ko[row * KD + col] = v;
            ko[col * KD + row] = v;
          }
        });
      });
    });
  }
  const double ldet_v = wave_sum(ldet.value());    // per-lane partial log-dets (pivots and phi)
  const bool ok_all = __all(ok);
  if (lane == 0) {
    double lnl = J.K[(long long)(b - b_off) * J.kstride] - 0.5 * qv - 0.5 * ldet_v;
    if (!ok_all || J.fail) lnl = -INFINITY;
    out_units[(long long)p * B + b] = lnl;
  }
#ifdef EWH_DEV
  if constexpr (STAMP) {
    EWH_STAMP(3 + 2 * NB)
    if (lane == 0 && blockIdx.x < STAMP_UNITS) {
      long long* o = g_stamps + (long long)blockIdx.x * STAMP_N;
      for (int i = 0; i < 4 + 2 * NB && i < STAMP_N - 2; ++i) o[i] = stp[i];
      o[STAMP_N - 2] = __builtin_amdgcn_s_getreg(4 | (31 << 11));    // HW_ID (wave, SIMD, CU, SE)
      o[STAMP_N - 1] = __builtin_amdgcn_s_getreg(20 | (31 << 11));   // XCC_ID
    }
  }
#endif
#undef EWH_STAMP
}

}  // namespace ewh_dev
