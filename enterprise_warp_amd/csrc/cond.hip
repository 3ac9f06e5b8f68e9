// cond.hip — the per-pulsar conditional Gaussian process (ABI 10: ewh_cond_gp).
//
// Input: the chunk's G slots (ld x ld per sample, r in the last row and
// column), filled by the route the likelihood uses (run_white / run_delay, or
// the broadcast of the cached full-width Gram).  Per (pulsar, sample) unit,
// all fp64, in the DEVICE basis T A (DESIGN.md §2, §Conditional GP):
//   cond_solve_kernel    Sigma = G + diag(1/phi) = L L^T in place on the slot
//                        (lower triangle): left-looking in 16-column panels,
//                        the update of a panel from the finished ones on
//                        v_mfma_f64_16x16x4_f64, the 16x16 diagonal block in
//                        LDS by VALU, the rows below it by forward
//                        substitution with that block; then y = L^-1 d and
//                        x = L^-T (y + z).  Pad columns are identity.
//   cond_pack_kernel     the back-map to the caller's basis, a_user = a_dev +
//                        c_r - C_F b (ProjCoef), the coefficient rows, and
//                        the ld x (samples x groups) matrix V of the
//                        realisations: y_g = T_aug v_g
//   cond_process_kernel  Y = V^T T_aug^T on the fp64 MFMA: i runs over the
//                        (sample, group) outputs and j over TOAs, so each
//                        (q, r) of a lane group stores 16 consecutive TOAs; a
//                        workgroup stages its 16-TOA tile of T_aug in LDS
//                        once and reuses it for every output of the chunk
//   cond_process_valu_kernel  the same for a theta-dependent basis (the
//                        chromatic factor differs per sample: VALU)
// A unit whose pivot fails (status 1) or whose delay parameters are not
// finite (status 2) gets NaN coefficients and realisations, nothing else.
// Launch wrappers: ewarp_launch.h.
#include "ewarp_launch.h"

namespace ewh_dev {

namespace {

constexpr int CS_THREADS = 256;
constexpr int CS_LDT = 17;            // LDS row stride of the 16 x 16 diagonal block

// the diagonal block A[16 kb ..][16 kb ..] (lower) -> LDS
__device__ __forceinline__ void load_diag(const double* __restrict__ A, int ld, int kb, double* Ls) {
  const int i = threadIdx.x >> 4, j = threadIdx.x & 15;
  if (threadIdx.x < 256) Ls[i * CS_LDT + j] = j <= i ? A[(long long)(16 * kb + i) * ld + 16 * kb + j] : 0.0;
}

}  // namespace

// grid: (nsamp); 256 threads.  G: the chunk's slots (destroyed: L is left in
// the lower triangle); x: ld entries per unit (pads zero); z: m entries per
// unit or NULL; Kb: the slots' -1/2 log|N| (-inf: a non-finite delay parameter)
__global__ __launch_bounds__(CS_THREADS) void cond_solve_kernel(double* __restrict__ G, int ld, int m,
                                                                 const int* __restrict__ col_ptr,
                                                                 const DSpec* __restrict__ spec,
                                                                 const double* __restrict__ theta, int ldth,
                                                                 const double* __restrict__ Kb, int has_delay,
                                                                 const double* __restrict__ z, int nsamp,
                                                                 double* __restrict__ x, int* __restrict__ status) {
  __shared__ double d[WIDE_LD_MAX];
  __shared__ double Ls[16 * CS_LDT];
  __shared__ int s_fail;
  const int bl = blockIdx.x, tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63, q = lane >> 4, c = lane & 15;
  const int nbf = (m + 15) / 16, n = 16 * nbf;
  EWH_DCHECK(bl < nsamp && ld % 16 == 0 && m >= 1 && m < ld && n <= ld && ld <= WIDE_LD_MAX, "cond_solve shape");
  double* A = G + (long long)bl * ld * ld;
  double* xo = x + (long long)bl * ld;
  const double* th = theta + (long long)bl * ldth;
  const double qnan = __builtin_nan("");
  if (has_delay && Kb[bl] == -INFINITY) {
    for (int j = tid; j < ld; j += CS_THREADS) xo[j] = j < m ? qnan : 0.0;
    if (tid == 0) status[bl] = 2;
    return;
  }
  if (tid == 0) s_fail = 0;
  for (int j = tid; j < n; j += CS_THREADS) d[j] = j < m ? A[(long long)(ld - 1) * ld + j] : 0.0;
  __syncthreads();
  // pads as identity, then diag += 1 / phi
  for (int j = m + wave; j < n; j += 4) {
    for (int cc = lane; cc <= j; cc += 64) A[(long long)j * ld + cc] = cc == j ? 1.0 : 0.0;
    for (int i = j + 1 + lane; i < n; i += 64) A[(long long)i * ld + j] = 0.0;
  }
  for (int a = tid; a < m; a += CS_THREADS) {
    double ph = 0.0;   // (col_phi written out: the helper swaps an add's operands here, profiles/r17/same_device_code.txt)
    for (int e = col_ptr[a]; e < col_ptr[a + 1]; ++e) ph += spec_phi(spec[e], th);
    A[(long long)a * ld + a] += 1.0 / ph;
  }
  __syncthreads();
  for (int kb = 0; kb < nbf; ++kb) {
    // panel kb -= L[.][0 .. 16 kb) L[kb][0 .. 16 kb)^T, one 16 x 16 tile per wave and pass
    if (kb > 0) {
      for (int ib = kb + wave; ib < nbf; ib += 4) {
        EWH_DCHECK(ib >= kb && 16 * ib + 15 < n && 16 * kb + 15 < n, "cond_solve trailing tile");
        const double* ar = A + (long long)(16 * ib + c) * ld + q;
        const double* br = A + (long long)(16 * kb + c) * ld + q;
        v4d acc = {0.0, 0.0, 0.0, 0.0};
        for (int j0 = 0; j0 < 16 * kb; j0 += 4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[j0], br[j0], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          double* dst = A + (long long)(16 * ib + q + 4 * r) * ld + 16 * kb + c;
          *dst -= acc[r];
        }
      }
      __syncthreads();
    }
    // the diagonal block in LDS
    load_diag(A, ld, kb, Ls);
    __syncthreads();
    for (int kk = 0; kk < 16; ++kk) {
      if (tid == 0) {
        const double p = Ls[kk * CS_LDT + kk];
        if (!(p > 0.0) || !isfinite(p)) s_fail = 1;
        else Ls[kk * CS_LDT + kk] = sqrt(p);
      }
      __syncthreads();
      if (s_fail) break;
      if (tid < 16 && tid > kk) Ls[tid * CS_LDT + kk] /= Ls[kk * CS_LDT + kk];
      __syncthreads();
      {
        const int i = tid >> 4, j = tid & 15;
        if (j > kk && j <= i) Ls[i * CS_LDT + j] = fma(-Ls[i * CS_LDT + kk], Ls[j * CS_LDT + kk], Ls[i * CS_LDT + j]);
      }
      __syncthreads();
    }
    if (s_fail) break;
    {
      const int i = tid >> 4, j = tid & 15;
      if (j <= i) A[(long long)(16 * kb + i) * ld + 16 * kb + j] = Ls[i * CS_LDT + j];
    }
    // the rows below: X L_kk^T = A, one row per thread
    for (int row = 16 * (kb + 1) + tid; row < n; row += CS_THREADS) {
      EWH_DCHECK(row < n && 16 * kb + 15 < n, "cond_solve panel row");
      double* ap = A + (long long)row * ld + 16 * kb;
      double v[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] = ap[j];
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        double s = v[j];
#pragma unroll
        for (int p = 0; p < j; ++p) s = fma(-v[p], Ls[j * CS_LDT + p], s);
        v[j] = s / Ls[j * CS_LDT + j];
      }
#pragma unroll
      for (int j = 0; j < 16; ++j) ap[j] = v[j];
    }
    __syncthreads();
  }
  if (s_fail) {
    for (int j = tid; j < ld; j += CS_THREADS) xo[j] = j < m ? qnan : 0.0;
    if (tid == 0) status[bl] = 1;
    return;
  }
  // y = L^-1 d
  for (int kb = 0; kb < nbf; ++kb) {
    load_diag(A, ld, kb, Ls);
    __syncthreads();
    if (tid == 0) {
      for (int j = 0; j < 16; ++j) {
        double s = d[16 * kb + j];
        for (int p = 0; p < j; ++p) s = fma(-Ls[j * CS_LDT + p], d[16 * kb + p], s);
        d[16 * kb + j] = s / Ls[j * CS_LDT + j];
      }
    }
    __syncthreads();
    for (int row = 16 * (kb + 1) + tid; row < n; row += CS_THREADS) {
      const double* ap = A + (long long)row * ld + 16 * kb;
      double s = d[row];
#pragma unroll
      for (int p = 0; p < 16; ++p) s = fma(-ap[p], d[16 * kb + p], s);
      d[row] = s;
    }
    __syncthreads();
  }
  if (z)
    for (int j = tid; j < m; j += CS_THREADS) d[j] += z[(long long)bl * m + j];
  __syncthreads();
  // x = L^-T (y + z)
  for (int kb = nbf - 1; kb >= 0; --kb) {
    load_diag(A, ld, kb, Ls);
    __syncthreads();
    if (tid == 0) {
      for (int j = 15; j >= 0; --j) {
        double s = d[16 * kb + j];
        for (int p = j + 1; p < 16; ++p) s = fma(-Ls[p * CS_LDT + j], d[16 * kb + p], s);
        d[16 * kb + j] = s / Ls[j * CS_LDT + j];
      }
    }
    __syncthreads();
    for (int col = tid; col < 16 * kb; col += CS_THREADS) {
      double s = d[col];
#pragma unroll
      for (int p = 0; p < 16; ++p) s = fma(-A[(long long)(16 * kb + p) * ld + col], d[16 * kb + p], s);
      d[col] = s;
    }
    __syncthreads();
  }
  for (int j = tid; j < ld; j += CS_THREADS) xo[j] = j < m ? d[j] : 0.0;
  if (tid == 0) {
    EWH_DCHECK(bl >= 0 && bl < nsamp, "cond_solve status slot");
    status[bl] = 0;
  }
}

// grid: (nsamp); 256 threads.  x: the device-basis coefficients (ld per unit);
// C: nl x (nproj + 1) row-major, pcols: the nproj projected columns (the last
// column of C is the residual's, c_r); grp: the group of each of the m columns
// or NULL; coef: m per unit (caller's basis) or NULL; V: ld x ldv, column
// bl * n_group + g (zeroed by the caller)
__global__ __launch_bounds__(256) void cond_pack_kernel(const double* __restrict__ x, int ld, int m, int nl, int nproj,
                                                        const int* __restrict__ pcols, const double* __restrict__ C,
                                                        const int* __restrict__ status, const int* __restrict__ grp,
                                                        int n_group, int nsamp, double* __restrict__ coef,
                                                        double* __restrict__ V, int ldv) {
  const int bl = blockIdx.x, tid = threadIdx.x;
  const double* xs = x + (long long)bl * ld;
  const bool bad = status[bl] != 0;
  const double qnan = __builtin_nan("");
  const int nc = nproj + 1;
  EWH_DCHECK(bl < nsamp && (n_group == 0 || (bl + 1) * n_group <= ldv) && nl <= m && m < ld, "cond_pack V columns");
  for (int j = tid; j < m; j += 256) {
    double au = xs[j];
    if (j < nl && !bad) {
      // a_user = a_dev + c_r - C_F b
      double s = C[(long long)j * nc + nproj];
      for (int k = 0; k < nproj; ++k) s = fma(-C[(long long)j * nc + k], xs[pcols[k]], s);
      au += s;
    }
    if (bad) au = qnan;
    if (coef) coef[(long long)bl * m + j] = au;
    for (int g = 0; g < n_group; ++g) {
      double v = grp[j] == g ? au : 0.0;
      if (j < nl && !bad)
        for (int k = 0; k < nproj; ++k)
          if (grp[pcols[k]] == g) v = fma(C[(long long)j * nc + k], xs[pcols[k]], v);
      if (bad) v = qnan;
      EWH_DCHECK(j < ld && bl * n_group + g < ldv, "cond_pack V index");
      V[(long long)j * ldv + bl * n_group + g] = v;
    }
  }
}

// Y[o][t] = sum_k V[k][o] T_aug[t][k], k < m.  grid: (ceil(n_toa / 16)); 4
// waves; dynamic LDS: K4 x 16 doubles, K4 = m rounded up to 4 (the tile of
// T_aug, k-major).  lane l = (q = l >> 4, c = l & 15) holds A[i = c][k = q] =
// V[k0 + q][16 ot + c] and B[k = q][j = c] = T_aug[t0 + c][k0 + q]; D: TOA c,
// output q + 4 r.  nout = samples x groups of the chunk, ldv >= nout padded to 16.
__global__ __launch_bounds__(256) void cond_process_kernel(const double* __restrict__ T, int n_toa, int ld, int m,
                                                           const double* __restrict__ V, int ldv, int nout,
                                                           double* __restrict__ Y) {
  extern __shared__ __attribute__((aligned(16))) double Ts[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, q = lane >> 4, c = lane & 15;
  const int t0 = 16 * blockIdx.x, K4 = 4 * ((m + 3) / 4);
  EWH_DCHECK(K4 <= ld && t0 < n_toa && 16 * ((nout + 15) / 16) <= ldv, "cond_process tile against ld / ldv");
  for (int idx = tid; idx < 16 * K4; idx += 256) {
    const int tt = idx / K4, k = idx - tt * K4;
    const int t = t0 + tt;
    Ts[k * 16 + tt] = (t < n_toa && k < m) ? T[(long long)t * ld + k] : 0.0;
  }
  __syncthreads();
  const int ntile = (nout + 15) / 16;
  for (int ot = wave; ot < ntile; ot += 4) {
    const double* vp = V + (long long)q * ldv + 16 * ot + c;
    v4d acc = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < K4; k0 += 4)
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(vp[(long long)k0 * ldv], Ts[(k0 + q) * 16 + c], acc, 0, 0, 0);
    const int t = t0 + c;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int o = 16 * ot + q + 4 * r;
      if (o < nout && t < n_toa) {
        EWH_DCHECK(o >= 0 && t >= 0, "cond_process Y index");
        Y[(long long)o * n_toa + t] = acc[r];
      }
    }
  }
}

// theta-dependent basis: column j of sample bl is T_aug[t][j] fac_g(j)[t].
// grid: (ceil(n_toa / 256), nout); fac: wn_weights' chromatic factors of the chunk
__global__ __launch_bounds__(256) void cond_process_valu_kernel(PsrDev P, const double* __restrict__ fac,
                                                                const double* __restrict__ V, int ldv, int n_group,
                                                                int nout, double* __restrict__ Y) {
  const int t = blockIdx.x * 256 + threadIdx.x, o = blockIdx.y;
  if (t >= P.n_toa) return;
  EWH_DCHECK(o < nout && o < ldv && n_group > 0, "cond_process_valu output");
  const int bl = o / n_group;
  const double* row = P.T + (long long)t * P.ld;
  double s = 0.0;
  for (int j = 0; j < P.m; ++j) {
    const int g = P.col_bgroup[j];
    double v = row[j];
    if (g >= 0) v *= fac[((long long)bl * P.n_bgroup + g) * P.n_toa + t];
    s = fma(v, V[(long long)j * ldv + o], s);
  }
  Y[(long long)o * P.n_toa + t] = s;
}

int launch_cond_solve(double* G, int ld, int m, const int* col_ptr, const DSpec* spec, const double* theta, int ldth,
                      const double* Kb, bool has_delay, const double* z, int nsamp, double* x, int* status,
                      hipStream_t st) {
  if (nsamp <= 0) return 0;
  if (ld > WIDE_LD_MAX || m < 1 || m >= ld) return set_err(EWH_E_UNSUPPORTED, "conditional GP: basis wider than 1023 columns");
  hipLaunchKernelGGL(cond_solve_kernel, dim3((unsigned)nsamp), dim3(CS_THREADS), 0, st, G, ld, m, col_ptr, spec, theta,
                     ldth, Kb, has_delay ? 1 : 0, z, nsamp, x, status);
  EWH_HIP(hipGetLastError());
  return 0;
}

int launch_cond_pack(const double* x, int ld, int m, int nl, int nproj, const int* pcols, const double* C,
                     const int* status, const int* grp, int n_group, int nsamp, double* coef, double* V, int ldv,
                     hipStream_t st) {
  if (nsamp <= 0) return 0;
  hipLaunchKernelGGL(cond_pack_kernel, dim3((unsigned)nsamp), dim3(256), 0, st, x, ld, m, nl, nproj, pcols, C, status,
                     grp, n_group, nsamp, coef, V, ldv);
  EWH_HIP(hipGetLastError());
  return 0;
}

int launch_cond_process(const PsrDev& P, const double* fac, const double* V, int ldv, int n_group, int nout, double* Y,
                        hipStream_t st) {
  if (nout <= 0) return 0;
  if (P.n_bgroup > 0) {
    hipLaunchKernelGGL(cond_process_valu_kernel, dim3((unsigned)((P.n_toa + 255) / 256), (unsigned)nout), dim3(256), 0,
                       st, P, fac, V, ldv, n_group, nout, Y);
  } else {
    const size_t lds = (size_t)16 * (4 * ((P.m + 3) / 4)) * sizeof(double);
    if (lds > 48 * 1024)
      EWH_HIP(hipFuncSetAttribute((const void*)cond_process_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(cond_process_kernel, dim3((unsigned)((P.n_toa + 15) / 16)), dim3(256), lds, st, P.T, P.n_toa,
                       P.ld, P.m, V, ldv, nout, Y);
  }
  EWH_HIP(hipGetLastError());
  return 0;
}

}  // namespace ewh_dev
