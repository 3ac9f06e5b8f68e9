// ewarp_route.h — which kernel family factors a launch of per-pulsar units:
// arithmetic on the width in 16-column blocks, the source of the matrices and
// the plan's flags.  route_for() is the definition; ewarp_hip.hip switches on
// its value; the static_asserts below pin the table.  No HIP dependency.
#pragma once
#include "ewarp_plan.h"

namespace ewh_dev {

// widest basis, in blocks, of chol_mfma_kernel, chol_big_kernel and chol_wide_kernel / chol_dd_kernel
constexpr int MFMA_NB_MAX = 9;
constexpr int BIG_NB_MAX = 16;
constexpr int WIDE_NB_MAX = 64;
constexpr int WIDE_LD_MAX = 16 * WIDE_NB_MAX;
constexpr int CONTRACT2_NB_MAX = 13;   // widest basis of the pipelined contraction (contract2_kernel)
constexpr int LAT_NB_MAX = 8;          // ... of the latency kernel (chol_lat_kernel)

// The register partial kernel exists for kept sizes 1..PARTIAL_KEEP_MAX (up to
// 63 kept columns: 31 common frequencies + r) where the kept blocks lie in its
// phase-3 triangle (Split<NB>::H) and the kernel holds its blocks without
// spilling: <7, 3> and <7, 4> spill at two waves per SIMD (32 / 16 bytes of
// scratch per lane) and are not built.  Every other
// (nb, keep) is chol_wide_kernel's.
constexpr int PARTIAL_KEEP_MAX = 4;
constexpr bool partial_in_registers(int nb, int keep) {
  return nb <= MFMA_NB_MAX && keep >= 1 && keep <= PARTIAL_KEEP_MAX && nb - keep >= (nb == 8 ? 3 : nb / 2) &&
         !(nb == 7 && keep >= 3);
}

enum class Route {
  Register,     // chol_mfma_kernel<NB>
  Big,          // chol_big_kernel<NB>
  Lds,          // chol_lds_kernel
  Wide,         // chol_wide_kernel, fp64
  DdVerify,     // forward and reversed chol_wide_kernel, chol_dd_kernel where they disagree (VERIFY_FRAC)
  DdAll,        // chol_dd_kernel on every unit
  Unsupported,  // wider than WIDE_NB_MAX blocks
};
enum class PartialRoute { Register, Wide };   // chol_mfma_kernel<NB, KEEP> / chol_wide_kernel with keep > 0

enum class Source {   // where a launch's matrices come from
  FixedRun,     // a run of pulsars of one reduced width, the cached S (fixed white noise)
  FixedDelay,   // a chunk of samples of a delay pulsar of a fixed-white-noise handle: full width, per sample
  Varying,      // a chunk of samples of one pulsar, varying white noise: full width, per sample
};

// the widths the double-double factorisation covers: past 9 blocks where the
// matrix is the cached (double-double) S, past 16 anywhere; all_dd: every cached S
constexpr bool dd_path(const KernelPlan& plan, bool corr, bool osmode, int nb, bool fixed) {
  if (corr || osmode || plan.all_wide || plan.lds_only) return false;
  if (plan.all_dd && fixed) return true;
  return nb > BIG_NB_MAX || (fixed && nb > MFMA_NB_MAX);
}

// The route of a full factorisation of nb blocks; fixed: Source::FixedRun.
//
//   blocks   | default plan (modes 0, 2, 7)    | lds_only | all_wide | all_dd (29)
//            | fixed      sampled, corr, os    | (1)      | (27)     | fixed    sampled
//   1..9     | Register   Register             | Lds      | Wide     | DdAll    Register
//   10..16   | DdVerify   Big                  | Lds      | Wide     | DdAll    Big
//   17..64   | DdVerify   DdVerify (*)         | Wide     | Wide     | DdAll    DdAll
//   65..     | Unsupported                     | Unsupp.  | Unsupp.  | DdAll    DdAll
//
// (*) with a common process (corr, osmode) no route is double-double, in any
// mode: the fp64 columns of the plan apply, Wide past 16 blocks.  (The all_dd
// launcher has no width check of its own.)
constexpr Route route_for(const KernelPlan& plan, bool corr, bool osmode, int nb, bool fixed) {
  if (dd_path(plan, corr, osmode, nb, fixed))
    return plan.all_dd ? Route::DdAll : nb > WIDE_NB_MAX ? Route::Unsupported : Route::DdVerify;
  if (plan.all_wide || nb > BIG_NB_MAX) return nb > WIDE_NB_MAX ? Route::Unsupported : Route::Wide;
  if (plan.lds_only) return Route::Lds;
  return nb > MFMA_NB_MAX ? Route::Big : Route::Register;
}

constexpr PartialRoute partial_route_for(const KernelPlan& plan, int nb, int keep) {
  return partial_in_registers(nb, keep) && !plan.all_wide ? PartialRoute::Register : PartialRoute::Wide;
}

// Whether the refine pass follows the launch (refine_failed).  Never with a
// common process or in the cross-check modes 1 / 27; else by source:
//   FixedRun    unless the route was double-double already
//   FixedDelay  up to 16 blocks (the slots' G_lo holds the per-sample column)
//   Varying     without backend groups -- past 16 blocks too: the verify
//               route reads the compensated, not error-free, G_hi + G_lo of
//               the wide contraction, the refine pass the error-free Gram
// The three conditions coincide for some plans, not by construction.  (Not
// tied to the route: true for an Unsupported one too, whose launch has
// returned its error before this is asked.)
constexpr bool refine_after(Source src, int nb, bool bgroups, const KernelPlan& plan, bool corr, bool osmode) {
  if (corr || osmode || !plan.refine) return false;
  switch (src) {
    case Source::FixedRun: return !dd_path(plan, corr, osmode, nb, true);
    case Source::FixedDelay: return nb <= BIG_NB_MAX;
    default: return !bgroups;
  }
}

// all_dd: the refine pass of a varying-white-noise chunk on an fp64 route lists
// every unit, not only the -inf ones: the double-double twin of that route
// (a FixedDelay chunk was judged by the rule of the cached S: the -inf units only)
constexpr bool refine_lists_all(Source src, int nb, const KernelPlan& plan) {
  return plan.all_dd && src == Source::Varying && nb <= BIG_NB_MAX;
}

// ---- the table, pinned ------------------------------------------------------
namespace route_check {

constexpr Route R = Route::Register, G = Route::Big, L = Route::Lds, W = Route::Wide, V = Route::DdVerify,
                A = Route::DdAll, U = Route::Unsupported;

// route_for at 1, 9, 10, 16, 17, 64 and 65 blocks, in the product and the dev library
constexpr bool row(int mode, bool fixed, Route r1, Route r9, Route r10, Route r16, Route r17, Route r64, Route r65) {
  for (int dev = 0; dev < 2; ++dev) {
    const KernelPlan p = plan_for(mode, dev == 1);
    if (route_for(p, false, false, 1, fixed) != r1 || route_for(p, false, false, 9, fixed) != r9 ||
        route_for(p, false, false, 10, fixed) != r10 || route_for(p, false, false, 16, fixed) != r16 ||
        route_for(p, false, false, 17, fixed) != r17 || route_for(p, false, false, 64, fixed) != r64 ||
        route_for(p, false, false, 65, fixed) != r65)
      return false;
  }
  return true;
}
static_assert(row(0, true, R, R, V, V, V, V, U) && row(0, false, R, R, G, G, V, V, U), "route table, mode 0");
static_assert(row(2, true, R, R, V, V, V, V, U) && row(2, false, R, R, G, G, V, V, U), "route table, mode 2");
static_assert(row(7, true, R, R, V, V, V, V, U) && row(7, false, R, R, G, G, V, V, U), "route table, mode 7");
static_assert(row(1, true, L, L, L, L, W, W, U) && row(1, false, L, L, L, L, W, W, U), "route table, mode 1");
static_assert(row(27, true, W, W, W, W, W, W, U) && row(27, false, W, W, W, W, W, W, U), "route table, mode 27");
static_assert(row(29, true, A, A, A, A, A, A, A) && row(29, false, R, R, G, G, A, A, A), "route table, mode 29");

// The routing code this header replaced, transcribed: dispatch_chol's chain of
// tests (with launch_chol_small's refusal of mode 1 and launch_wide's width
// check), the three refine conditions of ctx_units' three loops and
// refine_failed's `all`.  Every mode, both libraries, 1..65 blocks.
constexpr Route old_route(const KernelPlan& p, bool corr, bool osmode, int nb, bool fixed) {
  const bool dd = !(corr || osmode || p.all_wide || p.lds_only) &&
                  ((p.all_dd && fixed) || nb > 16 || (fixed && nb > 9));
  if (dd && p.all_dd) return A;
  if (dd) return nb > 64 ? U : V;
  if (p.all_wide || nb > 16) return nb > 64 ? U : W;
  const bool regs = !p.lds_only;
  if (regs && nb > 9 && nb <= 16) return G;
  if (regs && nb <= 9) return R;
  return L;
}
constexpr bool same_as_old(int mode_lo, int mode_hi) {
  for (int mode = mode_lo; mode <= mode_hi; ++mode)
    for (int dev = 0; dev < 2; ++dev) {
      const KernelPlan p = plan_for(mode, dev == 1);
      for (int common = 0; common < 3; ++common) {      // none, corr, osmode
        const bool corr = common == 1, osmode = common == 2;
        const bool refine_on = !corr && !osmode && p.refine;
        for (int nb = 1; nb <= 65; ++nb) {
          const bool dd_fixed = !(corr || osmode || p.all_wide || p.lds_only) &&
                                ((p.all_dd && true) || nb > 16 || (true && nb > 9));
          const bool dd_sampled = !(corr || osmode || p.all_wide || p.lds_only) &&
                                  ((p.all_dd && false) || nb > 16 || (false && nb > 9));
          if (route_for(p, corr, osmode, nb, true) != old_route(p, corr, osmode, nb, true) ||
              route_for(p, corr, osmode, nb, false) != old_route(p, corr, osmode, nb, false))
            return false;
          for (int bg = 0; bg < 2; ++bg) {
            if (refine_after(Source::FixedRun, nb, bg == 1, p, corr, osmode) != (!dd_fixed && refine_on) ||
                refine_after(Source::FixedDelay, nb, bg == 1, p, corr, osmode) != (nb <= 16 && refine_on) ||
                refine_after(Source::Varying, nb, bg == 1, p, corr, osmode) != (bg == 0 && refine_on))
              return false;
          }
          // (refine_failed took `fixed` from psr == NULL: true for both fixed sources)
          if (refine_on && (refine_lists_all(Source::FixedRun, nb, p) != (p.all_dd && !dd_fixed) ||
                            refine_lists_all(Source::FixedDelay, nb, p) != (p.all_dd && !dd_fixed) ||
                            refine_lists_all(Source::Varying, nb, p) != (p.all_dd && !dd_sampled)))
            return false;
          // a common process is never double-double
          if (common != 0 && (route_for(p, corr, osmode, nb, true) == V || route_for(p, corr, osmode, nb, true) == A ||
                              route_for(p, corr, osmode, nb, false) == V || route_for(p, corr, osmode, nb, false) == A))
            return false;
        }
      }
    }
  return true;
}
static_assert(same_as_old(0, 9), "routes and refine conditions as before, modes 0..9");
static_assert(same_as_old(10, 19), "routes and refine conditions as before, modes 10..19");
static_assert(same_as_old(20, 29), "routes and refine conditions as before, modes 20..29");
static_assert(same_as_old(30, KERNEL_MODE_MAX), "routes and refine conditions as before, modes 30..");

constexpr bool no_refine(int mode) {
  for (int nb = 1; nb <= 65; ++nb)
    for (int src = 0; src < 3; ++src)
      if (refine_after((Source)src, nb, false, plan_for(mode, false), false, false)) return false;
  return true;
}
static_assert(no_refine(1) && no_refine(27), "the cross-check modes compare the fp64 kernels as such");

constexpr bool partial_as_old() {
  for (int mode = 0; mode <= KERNEL_MODE_MAX; ++mode)
    for (int nb = 1; nb <= 17; ++nb)
      for (int keep = 0; keep <= 5; ++keep) {
        const KernelPlan p = plan_for(mode, true);
        if ((partial_route_for(p, nb, keep) == PartialRoute::Register) !=
            (partial_in_registers(nb, keep) && !p.all_wide))
          return false;
      }
  return true;
}
static_assert(partial_as_old(), "the partial route: registers where the kernel exists, unless all_wide");

}  // namespace route_check
}  // namespace ewh_dev
