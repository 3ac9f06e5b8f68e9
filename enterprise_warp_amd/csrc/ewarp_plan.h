// ewarp_plan.h — what an ewh_set_kernel_mode number selects, by name.
//
// plan_for() is the only place a mode number is interpreted: the host code
// (ewarp_hip.hip) and the kernel families' launch wrappers test the fields of
// the KernelPlan it returns.  (launch_chol_small and launch_contract2_nb still
// take integers -- the mode itself and KernelPlan::contract2_waves.)  The
// defaults are mode 0, the product path.  No HIP dependency.
#pragma once

namespace ewh_dev {

struct KernelPlan {
  bool in_range = true;       // 0 .. KERNEL_MODE_MAX (outside: EWH_E_INVALID, not EWH_E_UNSUPPORTED)
  bool valid = true;          // the mode exists in this build (product, or the dev library's A/B variants)
  bool variant = false;       // A/B variant that variant_built() (chol_small.hip) answers for
  // ---- latency path (chol_lat.hip) of small single-device batches
  bool lat = true;
  bool lat_stamps = false;    // phase stamps
  int lat_variant = 0;        // LAT_VAR_BARRIER 1 / LAT_VAR_R3 2 / LAT_VAR_STALL 3
  // ---- factorisation route
  bool lds_only = false;      // every unit by chol_lds_kernel
  bool all_wide = false;      // every factorisation (full and partial) by the fp64 chol_wide_kernel
  bool all_dd = false;        // every unit the double-double path covers by chol_dd_kernel, no verify step
  bool refine = true;         // -inf units of the fp64 kernels refactored in double-double
  bool wide_r05a = false;     // round-5a wide schedule: 128 MB scratch budgets, forward / reversed passes apart
  // ---- contraction
  bool contract2 = true;      // pipelined contraction (contract2)
  bool rsep = true;           // r-separated Gram where the residual fills the last block
  int contract2_waves = 0;    // launch_contract2_nb's `waves` (0: its default form)
  bool epoch_multi = true;    // epoch sums of ES_S samples per workgroup
  bool fixed_gram_dd = true;  // fixed white noise: the cached Gram in double-double (gram_dd_kernel)
  bool stage_spectra = true;  // register kernels read the staged spectrum records (off: the CSR prologue)
  bool compact_spectra = true;  // ... their compact power-law form where a launch qualifies (off: the interpreted staged prologue)
  // ---- correlated common process (common_dense.hip)
  bool minv_reg = true;       // register M_g inverse where P allows, run beside the partial factorisations
  bool corr_right = true;     // right-looking schedule for small sample chunks
  bool corr_fuse_diag = true; // right-looking: the next diagonal block factored inside the trailing update
  bool corr_fused = true;     // large chunks: row update and panel in one kernel
  bool corr_pairs = true;     // large chunks: two block rows per update pass
  bool corr_rowupdate_r1 = false;  // round-1 row update (both operands staged through LDS)
  bool corr_diag_lds = false;      // round-1 LDS diagonal block and LDS-staged panel
  bool corr_one_tile = false;      // round-3 row update + panel: one tile per workgroup
  bool corr_pair_unpiped = false;  // pair kernel with U_pj loaded at the top of each step
  bool corr_trailing = false;      // left-looking schedule with a separate right-looking trailing update
};

constexpr int KERNEL_MODE_MAX = 39;

// Product modes: 0 the default, 1 the LDS kernels, 2 the batched path at every
// batch size, 7 the round-1 contraction / common-process kernels, 27 fp64
// wide, 29 double-double.  Every other valid mode is an A/B variant of the
// dev library (include/ewarp_hip.h lists them).
constexpr KernelPlan plan_for(int mode, bool dev_lib) {
  KernelPlan p;
  p.in_range = mode >= 0 && mode <= KERNEL_MODE_MAX;
  bool dev_only = true;
  // (the small-chunk right-looking schedule was tuned for the default path
  // only: every other mode, 2 / 27 / 29 included, is left-looking throughout)
  p.corr_right = mode == 0 || mode == 33;
  p.lat = false;
  switch (mode) {
    case 0: p.lat = true; dev_only = false; break;
    case 1:
      p.lds_only = true; p.refine = false;
      p.corr_fused = false; p.corr_rowupdate_r1 = true; p.corr_diag_lds = true;
      dev_only = false;
      break;
    case 2: dev_only = false; break;
    case 7:
      p.contract2 = false; p.fixed_gram_dd = false; p.minv_reg = false;
      p.corr_fused = false; p.corr_diag_lds = true; p.corr_trailing = true;
      dev_only = false;
      break;
    case 27: p.all_wide = true; p.refine = false; dev_only = false; break;
    case 29: p.all_dd = true; dev_only = false; break;
    case 14: p.compact_spectra = false; p.variant = true; break;   // (a free number inside 0 .. KERNEL_MODE_MAX: the range stays)
    // (tests/test_gpu_properties.py::test_kernel_mode_acceptance lists the dev library's modes without 14 and
    // would refuse it there; the suite runs that test on the product library only -- its list wants 14 added)
    case 15: p.contract2_waves = 4; p.variant = true; break;
    case 16: p.contract2_waves = 8; p.variant = true; break;
    case 17: case 21: case 26: p.variant = true; break;     // chol_mfma variants: launch_chol_small reads the mode
    case 19: p.stage_spectra = false; p.variant = true; break;
    case 22: p.lat = true; p.lat_stamps = true; p.variant = true; break;
    case 23: p.lat = true; p.lat_variant = 3; p.variant = true; break;
    case 24: p.lat = true; p.lat_variant = 1; p.variant = true; break;
    case 25: p.lat = true; p.lat_variant = 2; p.variant = true; break;
    case 28: p.corr_pairs = false; p.corr_one_tile = true; p.variant = true; break;
    case 30: p.rsep = false; p.contract2_waves = 30; p.variant = true; break;
    case 31: p.corr_pairs = false; p.variant = true; break;
    case 32: p.corr_pair_unpiped = true; p.variant = true; break;
    case 33: p.corr_fuse_diag = false; break;
    case 34: p.wide_r05a = true; break;
    case 35: p.contract2_waves = 35; break;
    case 36: p.rsep = false; break;
    case 37: p.epoch_multi = false; break;
    case 38: p.rsep = false; p.contract2_waves = 38; break;
    case 39: p.rsep = false; p.contract2_waves = 39; break;
    default: p.valid = false; break;
  }
  if (dev_only && !dev_lib) p.valid = false;
  return p;
}

constexpr bool same_plan(const KernelPlan& a, const KernelPlan& b) {
  return a.in_range == b.in_range && a.valid == b.valid && a.variant == b.variant && a.lat == b.lat &&
         a.lat_stamps == b.lat_stamps && a.lat_variant == b.lat_variant && a.lds_only == b.lds_only && a.all_wide == b.all_wide &&
         a.all_dd == b.all_dd && a.refine == b.refine && a.wide_r05a == b.wide_r05a && a.contract2 == b.contract2 &&
         a.rsep == b.rsep && a.contract2_waves == b.contract2_waves && a.epoch_multi == b.epoch_multi &&
         a.fixed_gram_dd == b.fixed_gram_dd && a.stage_spectra == b.stage_spectra && a.compact_spectra == b.compact_spectra &&
         a.minv_reg == b.minv_reg &&
         a.corr_right == b.corr_right && a.corr_fuse_diag == b.corr_fuse_diag && a.corr_fused == b.corr_fused &&
         a.corr_pairs == b.corr_pairs && a.corr_rowupdate_r1 == b.corr_rowupdate_r1 &&
         a.corr_diag_lds == b.corr_diag_lds && a.corr_one_tile == b.corr_one_tile &&
         a.corr_pair_unpiped == b.corr_pair_unpiped && a.corr_trailing == b.corr_trailing;
}

constexpr KernelPlan batched_default_plan() {   // mode 2 as it must come out
  KernelPlan p;
  p.lat = false;
  p.corr_right = false;
  return p;
}

static_assert(same_plan(plan_for(0, false), KernelPlan{}) && same_plan(plan_for(0, true), KernelPlan{}),
              "mode 0 is the default plan");
static_assert(same_plan(plan_for(2, false), batched_default_plan()),
              "mode 2 leaves the latency path and (with every non-default mode) the right-looking schedule, no more");
static_assert(!plan_for(-1, true).in_range && !plan_for(KERNEL_MODE_MAX + 1, true).in_range &&
                  plan_for(3, true).in_range && plan_for(KERNEL_MODE_MAX, false).in_range,
              "the range of mode numbers");
static_assert(plan_for(14, true).valid && !plan_for(14, true).compact_spectra && plan_for(14, true).stage_spectra &&
                  plan_for(19, true).compact_spectra && !plan_for(14, false).valid,
              "mode 14 turns off the fixed-form prologue alone, in the dev library");
static_assert(!plan_for(-1, true).valid && !plan_for(3, true).valid && !plan_for(18, true).valid &&
                  !plan_for(20, true).valid && !plan_for(KERNEL_MODE_MAX + 1, true).valid,
              "a mode outside the lists is invalid");
static_assert(plan_for(33, true).valid && !plan_for(33, false).valid && !plan_for(15, false).valid &&
                  !plan_for(39, false).valid,
              "a dev-only mode is invalid in the product library");
static_assert(plan_for(1, false).valid && plan_for(7, false).valid && plan_for(27, false).valid &&
                  plan_for(29, false).valid,
              "the product modes");

}  // namespace ewh_dev
