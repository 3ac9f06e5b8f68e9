// ewarp_chol_small.h — the launch templates of the product register kernel
// chol_mfma_kernel<NB <= 9>, shared by the two translation units that
// instantiate it: chol_small.hip (the interpreted spectrum prologue, and the
// dev library's A/B variants) and chol_small_pl.hip (the fixed-form prologue,
// PL) -- two units so that `make -j` compiles the two halves side by side.
#pragma once
#include "ewarp_launch.h"

namespace ewh_dev {
namespace {

// DEAD: dead k-slices of block row 0 in the front-pad order (0..3), or -1:
// the stored order; IMG: the jobs' operand images instead of their matrices;
// PL: the jobs' compact power-law records, the fixed-form prologue
template <int NB, int ALG = PANEL_2L, bool STAMP = false, int W = default_waves(NB), bool FULL = false, int DEAD = -1,
          bool IMG = false, bool PL = false>
void launch_chol_mfma(const UnitSpan& s) {
  // (an instantiation that is not built, pl_built: the interpreted prologue --
  // launch_register does not ask for it)
  constexpr bool PLB = PL && pl_built(NB, DEAD, IMG);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(chol_mfma_kernel<NB, W, ALG, STAMP, 0, FULL, DEAD, IMG, PLB>), dim3((unsigned)s.n),
                     dim3(64), 0, s.st, s.jobs, s.B, s.u0, s.b_off, s.theta, s.ldth, s.units, nullptr, 0, 0,
                     PLB ? unit_dec_make(s.u0, s.B) : UnitDec{});
}

// the product kernel of width NB for a launch whose jobs share `dead` dead
// slices: the instantiation front_inst picks (ewarp_dev.h; the same rule as
// chol_lat_kernel's launcher) -- the stored order where no slice can be dropped
template <int NB, bool STAMP = false, bool IMG = false, bool PL = false>
void launch_chol_front(int dead, const UnitSpan& s) {
  constexpr int W = default_waves(NB);
  switch (front_inst(NB, dead)) {
    case 3: launch_chol_mfma<NB, PANEL_2L, STAMP, W, false, 3, IMG, PL>(s); break;
    case 2: launch_chol_mfma<NB, PANEL_2L, STAMP, W, false, 2, IMG, PL>(s); break;
    // (<6, DEAD 1> does not fit 256 VGPRs -- 44 bytes of scratch per lane --
    // and is not built; front_inst never picks it)
    case 1: launch_chol_mfma<NB, PANEL_2L, STAMP, W, false, NB == 6 ? -1 : 1, IMG, PL>(s); break;
    default: launch_chol_mfma<NB, PANEL_2L, STAMP, W, false, -1, IMG, PL>(s); break;
  }
}

// ... from the jobs' operand images where every job of the launch has one
template <int NB, bool STAMP = false, bool PL = false>
void launch_chol_images(int dead, bool img, const UnitSpan& s) {
  if (img)
    launch_chol_front<NB, STAMP, true, PL>(dead, s);
  else
    launch_chol_front<NB, STAMP, false, PL>(dead, s);
}

}  // namespace
}  // namespace ewh_dev
