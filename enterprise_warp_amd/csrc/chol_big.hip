// chol_big.hip — left-looking wide-basis factorisation chol_big_kernel<NB 10..16>.
#include "ewarp_launch.h"

namespace ewh_dev {

// ----------------------------------------------------------------------------
// batched factorisation for wide bases (NB > 9, e.g. C4's 193-wide Sigma):
// one wave per unit, LEFT-looking over block rows.  Block row i (<= NB
// blocks, C/D layout) is loaded into registers, takes the updates
// A_ij -= U_pi^T U_pj of every finished row p < i (4 MFMAs per block, the U
// blocks streamed back from a per-wave scratch in the same lane layout,
// double-buffered), is factored by the LDL^T panel and written to scratch.
// Same arithmetic as chol_mfma_kernel (right-looking), re-ordered.
// ----------------------------------------------------------------------------
template <int NB>
__device__ __forceinline__ long long big_blk(int p, int j) {   // packed upper block index
  return (long long)p * NB - (long long)p * (p - 1) / 2 + (j - p);
}

template <int NB>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1)))
void chol_big_kernel(const CholJob* __restrict__ jobs, int B, long long u0, int b_off,
                     const double* __restrict__ theta, int ldth, double* __restrict__ out_units,
                     double* __restrict__ scratch) {
  constexpr int LD = 16 * NB;
  __shared__ double phinv[LD];
  const int lane = threadIdx.x;
  const int q = lane >> 4, c = lane & 15;
  const long long u = u0 + xcd_unit(blockIdx.x, gridDim.x);
  const int p = (int)(u / B), b = (int)(u % B);
  const CholJob J = jobs[p];
  const gdptr A = (gdptr)(J.mats + (long long)(b - b_off) * J.mstride);
  const double* th = theta + (long long)b * ldth;
  typedef __attribute__((address_space(1))) v4d gv4d;   // global_load / store (see gdptr)
  __attribute__((address_space(1))) double* scr =
      (__attribute__((address_space(1))) double*)(scratch + (long long)blockIdx.x * (NB * (NB + 1) / 2) * 256 + lane * 4);

  LogAcc lphi;
  for (int a = lane; a < LD; a += 64) {
    double pi = 0.0;
    if (a < J.mreal && J.col_ptr[a] < J.col_ptr[a + 1]) {   // (pads carry no entry)
      const double ph = col_phi<true>(J.col_ptr, J.spec, a, th);
      pi = 1.0 / ph;
      lphi.add(ph);
    }
    phinv[a] = pi;
  }
  const double lphi_sum = wave_sum(lphi.value());
  __syncthreads();

  LogAcc ldet;
  bool ok = true;
  double qv = 0.0;
  const int klast = __builtin_amdgcn_readfirstlane(J.mreal - 16 * (NB - 1));   // the last row's pad pivots are skipped
  static_for<0, NB>([&](auto I) {
    constexpr int i = decltype(I)::value;
    constexpr int W = NB - i;                       // blocks in row i
    v4d R[W];
    static_for<0, W>([&](auto JJ) {
      constexpr int j = i + decltype(JJ)::value;
      static_for<0, 4>([&](auto RR) {
        constexpr int r = decltype(RR)::value;
        R[j - i][r] = A[(long long)(16 * i + q + 4 * r) * LD + 16 * j + c];
      });
      if constexpr (j == i) {
        const double pd = phinv[16 * i + c];
        static_for<0, 4>([&](auto RR) {
          constexpr int r = decltype(RR)::value;
          R[0][r] += (q + 4 * r == c) ? pd : 0.0;
        });
      }
    });
    if constexpr (i > 0) {
      // U blocks (p, i..NB-1) of earlier rows: Ui once, then each Uj in turn
      // (the compiler issues the row's loads ahead of its MFMAs)
#pragma unroll 1
      for (int pp = 0; pp < i; ++pp) {
        const v4d Ui = *(const gv4d*)(scr + big_blk<NB>(pp, i) * 256);
        static_for<0, W>([&](auto JJ) {
          constexpr int jj = decltype(JJ)::value;
          const v4d Uj = *(const gv4d*)(scr + big_blk<NB>(pp, i + jj) * 256);
          syrk_update(R[jj], Ui, Uj);
        });
      }
    }
    panel_ldl_row<NB, PANEL_2L, true, true>(I, [&](auto JJ) -> v4d& { return R[decltype(JJ)::value - i]; }, q, c,
                                            ldet, ok, NoHook{}, klast);
    if constexpr (i < NB - 1) {
      static_for<0, W>([&](auto JJ) {
        constexpr int j = i + decltype(JJ)::value;
        *(gv4d*)(scr + big_blk<NB>(i, j) * 256) = R[j - i];
      });
    } else {
      qv = readlane_d(R[0][3], 63);
    }
  });
  const double ldet_v = wave_sum(ldet.value());
  const bool ok_all = __all(ok);
  if (lane == 0) {
    double lnl = J.K[(long long)(b - b_off) * J.kstride] - 0.5 * qv - 0.5 * ldet_v - 0.5 * lphi_sum;
    if (!ok_all || J.fail) lnl = -INFINITY;
    out_units[(long long)p * B + b] = lnl;
  }
}

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
