// chol_partial.hip — chol_mfma_kernel<..., KEEP>: per-pulsar partial
// factorisation for the correlated common process (see ewarp_hip.hip), kept
// sizes 1..4 (up to 31 common frequencies + r) at the widths
// partial_in_registers (ewarp_route.h) names.
#include "ewarp_launch.h"

namespace ewh_dev {
namespace {

template <int NB, int KEEP>
int launch_partial(const UnitSpan& s, double* keep_out, int keep_bs) {
  if constexpr (partial_in_registers(NB, KEEP) && NB - KEEP >= Split<NB>::H) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(chol_mfma_kernel<NB, default_waves(NB), PANEL_2L, false, KEEP>),
                       dim3((unsigned)s.n), dim3(64), 0, s.st, s.jobs, s.B, s.u0, s.b_off, s.theta, s.ldth, s.units,
                       keep_out, 0, keep_bs, UnitDec{});
    return 0;
  } else {
    return set_err(EWH_E_UNSUPPORTED, "common: reduced basis too narrow for the kept common block");
  }
}

}  // namespace

int launch_partial_nb(int nb, int keep, const UnitSpan& s, double* keep_out, int keep_bs) {
  // (every keep names its own instantiation: a keep without one is refused,
  // never factored by a kernel built for another kept size)
  if (!partial_in_registers(nb, keep))
    return set_err(EWH_E_UNSUPPORTED, "common: no register kernel for this reduced width and kept size");
#define EWH_PARTK(NBV, KV) \
  case KV: return launch_partial<NBV, KV>(s, keep_out, keep_bs);
#define EWH_PART(NBV)   \
  case NBV:             \
    switch (keep) {     \
      EWH_PARTK(NBV, 1) \
      EWH_PARTK(NBV, 2) \
      EWH_PARTK(NBV, 3) \
      EWH_PARTK(NBV, 4) \
    }                   \
    break;
  switch (nb) {
    EWH_PART(2)
    EWH_PART(3)
    EWH_PART(4)
    EWH_PART(5)
    EWH_PART(6)
    EWH_PART(7)
    EWH_PART(8)
    EWH_PART(9)
    default: break;
  }
#undef EWH_PART
#undef EWH_PARTK
  return set_err(EWH_E_UNSUPPORTED, "common: unsupported reduced width");
}


}  // namespace ewh_dev
