// chol_big.hip — left-looking wide-basis factorisation chol_big_kernel<NB 10..16>.
#include "ewarp_dev.h"

namespace ewh_dev {
namespace {

template <int NB>
void launch_chol_big(const UnitSpan& s, double* scr, long long cap) {
  for (long long o = 0; o < s.n; o += cap)   // one scratch slot per workgroup of a launch
    hipLaunchKernelGGL(HIP_KERNEL_NAME(chol_big_kernel<NB>), dim3((unsigned)std::min(cap, s.n - o)), dim3(64), 0, s.st,
                       s.jobs, s.B, s.u0 + o, s.b_off, s.theta, s.ldth, s.units, scr);
}

}  // namespace

int launch_chol_big_nb(int nb, const UnitSpan& s, double* scr, long long cap) {
  switch (nb) {
    case 10: launch_chol_big<10>(s, scr, cap); return 0;
    case 11: launch_chol_big<11>(s, scr, cap); return 0;
    case 12: launch_chol_big<12>(s, scr, cap); return 0;
    case 13: launch_chol_big<13>(s, scr, cap); return 0;
    case 14: launch_chol_big<14>(s, scr, cap); return 0;
    case 15: launch_chol_big<15>(s, scr, cap); return 0;
    case 16: launch_chol_big<16>(s, scr, cap); return 0;
    default: return set_err(EWH_E_UNSUPPORTED, "basis too wide (> 255 reduced columns)");
  }
}

}  // namespace ewh_dev
