// chol_small.hip — register-resident factorisation chol_mfma_kernel<NB <= 9>
// and (dev library only, -DEWH_DEV) its A/B variants (see ewarp_dev.h,
// ewh_set_kernel_mode).
#include "ewarp_dev.h"

namespace ewh_dev {
namespace {

// the front-pad map of the product kernels (ewarp_dev.h front_src), every
// (NB, mreal)
static_assert(front_map_ok(1) && front_map_ok(2) && front_map_ok(3) && front_map_ok(4) && front_map_ok(5) &&
                  front_map_ok(6) && front_map_ok(7) && front_map_ok(8) && front_map_ok(9),
              "front-pad map: a permutation of the frame, real columns and r in order, pads onto stored pads");
static_assert(MFMA_NB_MAX == 9, "front_map_ok covers every register-kernel width");
// ... and the addresses front_elem forms are the ones that map names
static_assert(front_elem_ok(1) && front_elem_ok(2) && front_elem_ok(3) && front_elem_ok(4) && front_elem_ok(5) &&
                  front_elem_ok(6) && front_elem_ok(7) && front_elem_ok(8) && front_elem_ok(9),
              "front_elem: base + constant + lane part == front_src(row) LD + front_src(col)");
// ... and the operand image (ewarp_dev.h img_index) holds, for every width and
// pad count, each of those elements once, at the offset the loads read
static_assert(img_map_ok(1) && img_map_ok(2) && img_map_ok(3), "operand image map, 1..3 blocks");
static_assert(img_map_ok(4) && img_map_ok(5), "operand image map, 4 and 5 blocks");
static_assert(img_map_ok(6), "operand image map, 6 blocks");
static_assert(img_map_ok(7), "operand image map, 7 blocks");
static_assert(img_map_ok(8), "operand image map, 8 blocks");
static_assert(img_map_ok(9), "operand image map, 9 blocks");

// DEAD: dead k-slices of block row 0 in the front-pad order (0..3), or -1:
// the stored order; IMG: the jobs' operand images instead of their matrices
template <int NB, int ALG = PANEL_2L, bool STAMP = false, int W = default_waves(NB), bool FULL = false, int DEAD = -1,
          bool IMG = false>
void launch_chol_mfma(const UnitSpan& s) {
  hipLaunchKernelGGL(HIP_KERNEL_NAME(chol_mfma_kernel<NB, W, ALG, STAMP, 0, FULL, DEAD, IMG>), dim3((unsigned)s.n),
                     dim3(64), 0, s.st, s.jobs, s.B, s.u0, s.b_off, s.theta, s.ldth, s.units, nullptr, 0, 0);
}

// the product kernel of width NB for a launch whose jobs share `dead` dead
// slices: the instantiation front_inst picks (ewarp_dev.h; the same rule as
// chol_lat_kernel's launcher) -- the stored order where no slice can be dropped
template <int NB, bool STAMP = false, bool IMG = false>
void launch_chol_front(int dead, const UnitSpan& s) {
  constexpr int W = default_waves(NB);
  switch (front_inst(NB, dead)) {
    case 3: launch_chol_mfma<NB, PANEL_2L, STAMP, W, false, 3, IMG>(s); break;
    case 2: launch_chol_mfma<NB, PANEL_2L, STAMP, W, false, 2, IMG>(s); break;
    // (<6, DEAD 1> does not fit 256 VGPRs -- 44 bytes of scratch per lane --
    // and is not built; front_inst never picks it)
    case 1: launch_chol_mfma<NB, PANEL_2L, STAMP, W, false, NB == 6 ? -1 : 1, IMG>(s); break;
    default: launch_chol_mfma<NB, PANEL_2L, STAMP, W, false, -1, IMG>(s); break;
  }
}

// ... from the jobs' operand images where every job of the launch has one
template <int NB, bool STAMP = false>
void launch_chol_product(int dead, bool img, const UnitSpan& s) {
  if (img)
    launch_chol_front<NB, STAMP, true>(dead, s);
  else
    launch_chol_front<NB, STAMP, false>(dead, s);
}

}  // namespace

#ifdef EWH_DEV
// (23: the latency kernel with every wait forced to run out, LAT_VAR_STALL;
// 24, 25: latency-kernel variants, chol_lat.hip LAT_VAR_BARRIER / LAT_VAR_R3;
// 26: one wave per SIMD, whole triangle resident, plain right-looking order;
// 28: the C5 row update + panel with one tile per workgroup, one block row
// per pass (round 3); 30: the TwoSum contraction up to 10 blocks;
// 31: the C5 row update one block row per pass, two tiles per workgroup;
// 32: the C5 pair kernel with each U_pj slab loaded at the top of its step)
bool variant_built(int mode) {
  return mode == 15 || mode == 16 || mode == 17 || mode == 19 || mode == 21 || mode == 22 || mode == 23 ||
         mode == 24 || mode == 25 || mode == 26 || mode == 28 || mode == 30 || mode == 31 || mode == 32;
}
// phase stamps of kernel mode 21 (g_stamps: STAMP_UNITS x STAMP_N)
extern "C" int ewh_dev_stamps(long long* out, long long n) {
  if (n > (long long)STAMP_UNITS * STAMP_N) n = (long long)STAMP_UNITS * STAMP_N;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), (size_t)n * sizeof(long long)) == hipSuccess ? 0 : -1;
}
#else
bool variant_built(int) { return false; }
#endif

int launch_chol_small(int mode, int nb, int dead, bool img, const UnitSpan& s) {
#ifdef EWH_DEV
  // A/B variants (NB = 8, the C3 reduced width)
  if (nb == 8) {
    switch (mode) {
      case 17: launch_chol_mfma<8, PANEL_1L>(s); return 0;  // round-2 one-level panel
      case 21: launch_chol_product<8, true>(dead, img, s); return 0;  // the product kernel + phase stamps
      case 26: launch_chol_mfma<8, PANEL_2L, false, 1, true>(s); return 0;  // W = 1, FULL
      default: break;
    }
  }
#endif
  // default: the two-level LDL^T panel (ewarp_dev.h PANEL_2L); in the front-pad
  // order with the dead slices every job of the launch has, where it has any,
  // and from the operand images where every job has the one of that order
  switch (nb) {
    case 1: launch_chol_product<1>(dead, img, s); return 0;
    case 2: launch_chol_product<2>(dead, img, s); return 0;
    case 3: launch_chol_product<3>(dead, img, s); return 0;
    case 4: launch_chol_product<4>(dead, img, s); return 0;
    case 5: launch_chol_product<5>(dead, img, s); return 0;
    case 6: launch_chol_product<6>(dead, img, s); return 0;
    case 7: launch_chol_product<7>(dead, img, s); return 0;
    case 8: launch_chol_product<8>(dead, img, s); return 0;
    case 9: launch_chol_product<9>(dead, img, s); return 0;
    default: return set_err(EWH_E_UNSUPPORTED, "no register kernel past 9 blocks");
  }
}

}  // namespace ewh_dev
