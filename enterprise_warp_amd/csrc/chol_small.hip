// chol_small.hip — register-resident factorisation chol_mfma_kernel<NB <= 9>
// and (dev library only, -DEWH_DEV) its A/B variants (see ewarp_dev.h,
// ewh_set_kernel_mode).
#include "ewarp_chol_small.h"

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

// ... from the jobs' compact power-law records (the fixed-form prologue,
// chol_small_pl.hip) where every job of the launch has them
template <int NB, bool STAMP = false>
void launch_chol_product(int dead, bool img, bool pl, const UnitSpan& s) {
  if (pl)
    launch_chol_small_pl(NB, dead, img, STAMP, s);
  else
    launch_chol_images<NB, STAMP, false>(dead, img, s);
}

}  // namespace

#ifdef EWH_DEV
// (23: the latency kernel with every wait forced to run out, LAT_VAR_STALL;
// 24, 25: latency-kernel variants, chol_lat.hip LAT_VAR_BARRIER / LAT_VAR_R3;
// 26: one wave per SIMD, whole triangle resident, plain right-looking order;
// 28: the C5 row update + panel with one tile per workgroup, one block row
// per pass (round 3); 30: the TwoSum contraction up to 10 blocks;
// 31: the C5 row update one block row per pass, two tiles per workgroup;
// 32: the C5 pair kernel with each U_pj slab loaded at the top of its step;
// 14: the product kernel with the interpreted staged prologue where the
// launch would take the fixed-form one)
bool variant_built(int mode) {
  return mode == 15 || mode == 16 || mode == 17 || mode == 19 || mode == 21 || mode == 22 || mode == 23 ||
         mode == 24 || mode == 25 || mode == 26 || mode == 28 || mode == 30 || mode == 31 || mode == 32 || mode == 14;
}
// phase stamps of kernel mode 21 (g_stamps: STAMP_UNITS x STAMP_N).  g_stamps
// is one array per translation unit: the fixed-form twin's stamps lie in
// chol_small_pl.hip's copy (dev_stamps_pl), and the last mode-21 launch says
// which of the two to read
int dev_stamps_pl(long long* out, long long n);
static bool g_stamps_in_pl = false;
extern "C" int ewh_dev_stamps(long long* out, long long n) {
  if (n > (long long)STAMP_UNITS * STAMP_N) n = (long long)STAMP_UNITS * STAMP_N;
  if (g_stamps_in_pl) return dev_stamps_pl(out, n);
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), (size_t)n * sizeof(long long)) == hipSuccess ? 0 : -1;
}
#else
bool variant_built(int) { return false; }
#endif

int launch_chol_small(int mode, int nb, int dead, bool img, bool pl, const UnitSpan& s) {
#ifdef EWH_DEV
  // A/B variants (NB = 8, the C3 reduced width)
  if (nb == 8) {
    switch (mode) {
      case 17: launch_chol_mfma<8, PANEL_1L>(s); return 0;  // round-2 one-level panel
      case 21:                                                         // the product kernel + phase stamps
        g_stamps_in_pl = pl;
        launch_chol_product<8, true>(dead, img, pl, s);
        return 0;
      case 26: launch_chol_mfma<8, PANEL_2L, false, 1, true>(s); return 0;  // W = 1, FULL
      default: break;
    }
  }
#endif
  // default: the two-level LDL^T panel (ewarp_dev.h PANEL_2L); in the front-pad
  // order with the dead slices every job of the launch has, where it has any,
  // and from the operand images where every job has the one of that order
  switch (nb) {
    case 1: launch_chol_product<1>(dead, img, pl, s); return 0;
    case 2: launch_chol_product<2>(dead, img, pl, s); return 0;
    case 3: launch_chol_product<3>(dead, img, pl, s); return 0;
    case 4: launch_chol_product<4>(dead, img, pl, s); return 0;
    case 5: launch_chol_product<5>(dead, img, pl, s); return 0;
    case 6: launch_chol_product<6>(dead, img, pl, s); return 0;
    case 7: launch_chol_product<7>(dead, img, pl, s); return 0;
    case 8: launch_chol_product<8>(dead, img, pl, s); return 0;
    case 9: launch_chol_product<9>(dead, img, pl, s); return 0;
    default: return set_err(EWH_E_UNSUPPORTED, "no register kernel past 9 blocks");
  }
}

}  // namespace ewh_dev
