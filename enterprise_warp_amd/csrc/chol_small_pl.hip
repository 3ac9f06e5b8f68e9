// chol_small_pl.hip — chol_mfma_kernel<NB <= 9, ..., PL>: the product register
// kernel with the fixed-form spectrum prologue (ewarp_dev.h; ewarp_spec.h), for
// launches whose jobs all carry compact power-law records.  A translation
// unit of its own beside chol_small.hip (ewarp_chol_small.h).
#include "ewarp_chol_small.h"

namespace ewh_dev {

#ifdef EWH_DEV
// the stamps of this unit's kernels (ewh_dev_stamps, chol_small.hip)
int dev_stamps_pl(long long* out, long long n) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), (size_t)n * sizeof(long long)) == hipSuccess ? 0 : -1;
}
#endif

// stamp: the dev library's phase-stamped twin (kernel mode 21, eight blocks)
void launch_chol_small_pl(int nb, int dead, bool img, [[maybe_unused]] bool stamp, const UnitSpan& s) {
#ifdef EWH_DEV
  if (stamp && nb == 8) return launch_chol_images<8, true, true>(dead, img, s);
#endif
  switch (nb) {
    case 1: return launch_chol_images<1, false, true>(dead, img, s);
    case 2: return launch_chol_images<2, false, true>(dead, img, s);
    case 3: return launch_chol_images<3, false, true>(dead, img, s);
    case 4: return launch_chol_images<4, false, true>(dead, img, s);
    case 5: return launch_chol_images<5, false, true>(dead, img, s);
    case 6: return launch_chol_images<6, false, true>(dead, img, s);
    case 7: return launch_chol_images<7, false, true>(dead, img, s);
    case 8: return launch_chol_images<8, false, true>(dead, img, s);
    case 9: return launch_chol_images<9, false, true>(dead, img, s);
    default: return;   // (launch_chol_small has refused the width)
  }
}

}  // namespace ewh_dev
