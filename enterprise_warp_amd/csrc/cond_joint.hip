// cond_joint.hip — the conditional Gaussian process under a correlated (ORF)
// common process (ABI 11: ewh_cond_joint), the joint solve over all pulsars.
//
// Elimination order (include/ewarp_hip.h, DESIGN.md §Joint conditional GP):
// every pulsar's own block [lead | own], pulsar-major, then the common columns
// in (pulsar a, column g) order.  With L = [[L_A, 0], [W, L_c]], L_A block
// diagonal over the pulsars, all fp64, in the DEVICE basis T A:
//   cond_joint_partial_kernel   per (pulsar, sample) on the chunk's G slot:
//                        phi^-1 on the own columns, L_A,p by left-looking
//                        16-column panels (the panel update and the Schur
//                        update of the common block on
//                        v_mfma_f64_16x16x4_f64, the tile pattern of
//                        cond_solve_kernel), W_p = C_p^T L_A,p^-T below it,
//                        y_a,p = L_A,p^-1 d_a,p; S_p = G_cc,p - W_p W_p^T and
//                        e_p = d_c,p - W_p y_a,p go to a compact block, L_A, W
//                        and y_a (r row) stay in the slot
//   cond_joint_assemble_kernel  per sample the lower triangle of
//                        Sigma_c[(a,g),(b,h)] = d_ab S_a[g,h] + d_gh M_g^-1[a,b]
//                        (order N_c = P n_col, padded to 16 with identity) and
//                        the right-hand side e; a failed own block or a
//                        non-finite log|M_g| marks the sample
//   cond_joint_dense_kernel     one workgroup per sample: Sigma_c = L_c L_c^T by
//                        the same panels, y_c = L_c^-1 e, x_c = L_c^-T (y_c + z_c);
//                        the vector lives in LDS
//   cond_joint_back_kernel      per (pulsar, sample): x_a = L_A^-T (y_a + z_a -
//                        W^T x_c); x leaves in the ld layout cond_pack_kernel reads
// z is indexed by coefficient (the caller's [B, n_coef] array), whatever the
// coefficient's place in the elimination order.  Launch wrappers: ewarp_launch.h.
#include "ewarp_launch.h"

namespace ewh_dev {

namespace {

constexpr int CJ_THREADS = 256;
constexpr int CJ_LDT = 17;            // LDS row stride of the 16 x 16 diagonal block

// the diagonal block A[16 kb ..][16 kb ..] (lower) -> LDS
__device__ __forceinline__ void cj_load_diag(const double* __restrict__ A, long long ld, int kb, double* Ls) {
  const int i = threadIdx.x >> 4, j = threadIdx.x & 15;
  Ls[i * CJ_LDT + j] = j <= i ? A[(16LL * kb + i) * ld + 16 * kb + j] : 0.0;
}

// The leading npiv columns of the n x n matrix A (lower triangle, row stride
// ld, n a multiple of 16) are eliminated in place: L in columns [0, npiv), and
// the Schur complement in the lower triangle of rows / columns [npiv, n).
// Left-looking in 16-column panels; the last panel stops its pivot loop at
// npiv, and the MFMAs of the trailing tiles mask the k-lanes >= npiv (those
// slots hold Schur values, not L).  Returns false at a pivot <= 0 or not
// finite.  Ls: 16 x CJ_LDT doubles of LDS; s_fail: one int of LDS, zeroed and
// synchronised by the caller.
__device__ bool cj_eliminate(double* __restrict__ A, long long ld, int n, int npiv, double* Ls, int* s_fail) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, q = lane >> 4, c = lane & 15;
  const int nbf = n / 16, nbo = (npiv + 15) / 16;
  for (int kb = 0; kb < nbo; ++kb) {
    const int kmax = min(16, npiv - 16 * kb);
    // panel kb -= L[.][0 .. 16 kb) L[kb][0 .. 16 kb)^T, one 16 x 16 tile per wave and pass
    if (kb > 0) {
      for (int ib = kb + wave; ib < nbf; ib += 4) {
        EWH_DCHECK(ib >= kb && 16 * ib + 15 < n && 16 * kb + 15 < n, "cond_joint panel tile");
        const double* ar = A + (16LL * ib + c) * ld + q;
        const double* br = A + (16LL * kb + c) * ld + q;
        v4d acc = {0.0, 0.0, 0.0, 0.0};
        for (int j0 = 0; j0 < 16 * kb; j0 += 4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[j0], br[j0], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          double* dst = A + (16LL * ib + q + 4 * r) * ld + 16 * kb + c;
          *dst -= acc[r];
        }
      }
      __syncthreads();
    }
    // the diagonal block in LDS: pivots [0, kmax), right-looking (the entries
    // past kmax end as Schur values)
    cj_load_diag(A, ld, kb, Ls);
    __syncthreads();
    for (int kk = 0; kk < kmax; ++kk) {
      if (tid == 0) {
        const double p = Ls[kk * CJ_LDT + kk];
        if (!(p > 0.0) || !isfinite(p)) *s_fail = 1;
        else Ls[kk * CJ_LDT + kk] = sqrt(p);
      }
      __syncthreads();
      if (*s_fail) break;
      if (tid < 16 && tid > kk) Ls[tid * CJ_LDT + kk] /= Ls[kk * CJ_LDT + kk];
      __syncthreads();
      {
        const int i = tid >> 4, j = tid & 15;
        if (j > kk && j <= i) Ls[i * CJ_LDT + j] = fma(-Ls[i * CJ_LDT + kk], Ls[j * CJ_LDT + kk], Ls[i * CJ_LDT + j]);
      }
      __syncthreads();
    }
    if (*s_fail) return false;
    {
      const int i = tid >> 4, j = tid & 15;
      if (j <= i) A[(16LL * kb + i) * ld + 16 * kb + j] = Ls[i * CJ_LDT + j];
    }
    // the rows below, one per thread: X L_kk^T = A on the pivot columns, the
    // Schur update on the panel's columns past kmax
    for (int row = 16 * (kb + 1) + tid; row < n; row += CJ_THREADS) {
      EWH_DCHECK(row < n && 16 * kb + 15 < n, "cond_joint panel row");
      double* ap = A + (long long)row * ld + 16 * kb;
      double v[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] = ap[j];
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        double s = v[j];
#pragma unroll
        for (int p = 0; p < j; ++p)
          if (p < kmax) s = fma(-v[p], Ls[j * CJ_LDT + p], s);
        v[j] = j < kmax ? s / Ls[j * CJ_LDT + j] : s;
      }
#pragma unroll
      for (int j = 0; j < 16; ++j) ap[j] = v[j];
    }
    __syncthreads();
  }
  // trailing tiles (jb >= nbo) -= L[ib][0 .. npiv) L[jb][0 .. npiv)^T
  const int nt = nbf - nbo;
  if (nt > 0) {
    for (int t = wave; t < nt * (nt + 1) / 2; t += 4) {
      int ii = 0, rem = t;                   // t -> (ii >= jj), row-major over the lower triangle of tiles
      while (rem > ii) rem -= ++ii;
      const int ib = nbo + ii, jb = nbo + rem;
      EWH_DCHECK(jb >= nbo && ib >= jb && 16 * ib + 15 < n, "cond_joint Schur tile");
      const double* ar = A + (16LL * ib + c) * ld + q;
      const double* br = A + (16LL * jb + c) * ld + q;
      v4d acc = {0.0, 0.0, 0.0, 0.0};
      for (int j0 = 0; j0 < 16 * nbo; j0 += 4) {
        const bool live = j0 + q < npiv;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(live ? ar[j0] : 0.0, live ? br[j0] : 0.0, acc, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        double* dst = A + (16LL * ib + q + 4 * r) * ld + 16 * jb + c;
        *dst -= acc[r];
      }
    }
    __syncthreads();
  }
  return true;
}

// d[0 .. npiv) <- L^-1 d, d[npiv .. n) -= W d[0 .. npiv)  (d in LDS)
__device__ void cj_forward(const double* __restrict__ A, long long ld, int n, int npiv, double* d, double* Ls) {
  const int tid = threadIdx.x, nbo = (npiv + 15) / 16;
  for (int kb = 0; kb < nbo; ++kb) {
    const int kmax = min(16, npiv - 16 * kb);
    cj_load_diag(A, ld, kb, Ls);
    __syncthreads();
    if (tid == 0) {
      for (int j = 0; j < 16; ++j) {
        double s = d[16 * kb + j];
        for (int p = 0; p < j && p < kmax; ++p) s = fma(-Ls[j * CJ_LDT + p], d[16 * kb + p], s);
        d[16 * kb + j] = j < kmax ? s / Ls[j * CJ_LDT + j] : s;
      }
    }
    __syncthreads();
    for (int row = 16 * (kb + 1) + tid; row < n; row += CJ_THREADS) {
      const double* ap = A + (long long)row * ld + 16 * kb;
      double s = d[row];
      for (int p = 0; p < kmax; ++p) s = fma(-ap[p], d[16 * kb + p], s);
      d[row] = s;
    }
    __syncthreads();
  }
}

// d[0 .. npiv) <- L^-T d[0 .. npiv)  (d in LDS)
__device__ void cj_backward(const double* __restrict__ A, long long ld, int npiv, double* d, double* Ls) {
  const int tid = threadIdx.x, nbo = (npiv + 15) / 16;
  for (int kb = nbo - 1; kb >= 0; --kb) {
    const int kmax = min(16, npiv - 16 * kb);
    cj_load_diag(A, ld, kb, Ls);
    __syncthreads();
    if (tid == 0) {
      for (int j = kmax - 1; j >= 0; --j) {
        double s = d[16 * kb + j];
        for (int p = j + 1; p < kmax; ++p) s = fma(-Ls[p * CJ_LDT + j], d[16 * kb + p], s);
        d[16 * kb + j] = s / Ls[j * CJ_LDT + j];
      }
    }
    __syncthreads();
    for (int col = tid; col < 16 * kb; col += CJ_THREADS) {
      double s = d[col];
      for (int p = 0; p < kmax; ++p) s = fma(-A[(16LL * kb + p) * ld + col], d[16 * kb + p], s);
      d[col] = s;
    }
    __syncthreads();
  }
}

}  // namespace

// grid: (nsamp); 256 threads.  G: the chunk's slots (ld x ld, r in the last
// row); columns [0, mo) are the own block (phi^-1 from the CSR; with varying
// white noise mo = gstart_v and the inner pads carry phi = 1), [mo, mo + nc)
// the common block.  S: (nc + 1) x nc per unit -- S_p, both triangles, then the
// row e_p.  The slot keeps L_A and W, and y_a | e_p in its r row.  status: 0,
// or 1 at a failed pivot (S is then not written).
__global__ __launch_bounds__(CJ_THREADS) void cond_joint_partial_kernel(double* __restrict__ G, int ld, int mo, int nc,
                                                                        const int* __restrict__ col_ptr,
                                                                        const DSpec* __restrict__ spec,
                                                                        const double* __restrict__ theta, int ldth,
                                                                        int nsamp, double* __restrict__ S,
                                                                        int* __restrict__ status) {
  __shared__ double d[WIDE_LD_MAX];
  __shared__ double Ls[16 * CJ_LDT];
  __shared__ int s_fail;
  const int bl = blockIdx.x, tid = threadIdx.x;
  const int m = mo + nc, n = 16 * ((m + 15) / 16);
  EWH_DCHECK(bl < nsamp && ld % 16 == 0 && mo >= 1 && nc >= 1 && mo <= m && m < ld && n <= ld && ld <= WIDE_LD_MAX,
             "cond_joint_partial shape");
  double* A = G + (long long)bl * ld * ld;
  const double* th = theta + (long long)bl * ldth;
  if (tid == 0) s_fail = 0;
  for (int j = tid; j < n; j += CJ_THREADS) d[j] = j < m ? A[(long long)(ld - 1) * ld + j] : 0.0;
  // phi^-1 on the own columns only (the common columns' prior is M_g^-1)
  for (int a = tid; a < mo; a += CJ_THREADS) {
    double ph = 0.0;   // (col_phi written out: the helper swaps an add's operands here, profiles/r17/same_device_code.txt)
    for (int e = col_ptr[a]; e < col_ptr[a + 1]; ++e) ph += spec_phi(spec[e], th);
    A[(long long)a * ld + a] += 1.0 / ph;
  }
  __syncthreads();
  if (!cj_eliminate(A, ld, n, mo, Ls, &s_fail)) {
    if (tid == 0) status[bl] = 1;
    return;
  }
  cj_forward(A, ld, n, mo, d, Ls);
  double* So = S + (long long)bl * (nc + 1) * nc;
  for (int idx = tid; idx < nc * nc; idx += CJ_THREADS) {
    const int g = idx / nc, h = idx - g * nc;
    const int hi = max(g, h), lo = min(g, h);
    EWH_DCHECK(mo + hi < m && idx < (nc + 1) * nc, "cond_joint_partial S slot");
    So[idx] = A[(long long)(mo + hi) * ld + mo + lo];
  }
  for (int h = tid; h < nc; h += CJ_THREADS) So[nc * nc + h] = d[mo + h];
  for (int j = tid; j < m; j += CJ_THREADS) A[(long long)(ld - 1) * ld + j] = d[j];
  if (tid == 0) {
    EWH_DCHECK(bl >= 0 && bl < nsamp, "cond_joint_partial status slot");
    status[bl] = 0;
  }
}

// grid: (Npad, nsamp); 256 threads: row i of Sigma_c of sample bl (columns
// j <= i) and rhs[i].  S: pulsar a's block of sample bl at
// S[(a sstride + bl) (nc + 1) nc]; pstat: the own blocks' status,
// [a sstride + bl]; minv / mlog / rep: launch_minv's.  sfail[bl] = 1 where an
// own block failed or a log|M_g| is not finite (the rows are then not written).
__global__ __launch_bounds__(256) void cond_joint_assemble_kernel(const double* __restrict__ S, long long sstride, int P,
                                                                  int nc, int nsamp, const int* __restrict__ pstat,
                                                                  const double* __restrict__ minv,
                                                                  const double* __restrict__ mlog,
                                                                  const int* __restrict__ rep, int Npad,
                                                                  double* __restrict__ dense, double* __restrict__ rhs,
                                                                  int* __restrict__ sfail) {
  __shared__ int s_bad;
  const int i = blockIdx.x, bl = blockIdx.y, tid = threadIdx.x, N = P * nc;
  EWH_DCHECK(i < Npad && bl < nsamp && N <= Npad && Npad % 16 == 0, "cond_joint_assemble row");
  if (tid == 0) s_bad = 0;
  __syncthreads();
  for (int a = tid; a < P; a += 256)
    if (pstat[(long long)a * sstride + bl] != 0) s_bad = 1;
  for (int g = tid; g < nc; g += 256)
    if (!isfinite(mlog[(long long)bl * nc + rep[g]])) s_bad = 1;
  __syncthreads();
  if (i == 0 && tid == 0) sfail[bl] = s_bad;
  if (s_bad) return;
  double* row = dense + ((long long)bl * Npad + i) * Npad;
  if (i >= N) {
    for (int j = tid; j <= i; j += 256) row[j] = j == i ? 1.0 : 0.0;
    if (tid == 0) rhs[(long long)bl * Npad + i] = 0.0;
    return;
  }
  const int a = i / nc, g = i - a * nc;
  const double* Sa = S + ((long long)a * sstride + bl) * (nc + 1) * nc;
  const double* mg = minv + ((long long)bl * nc + rep[g]) * P * P + (long long)a * P;   // row a of M_g^-1
  for (int j = tid; j <= i; j += 256) {
    const int b = j / nc, h = j - b * nc;
    double v = 0.0;
    if (b == a) v = Sa[g * nc + h];
    if (h == g) v += mg[b];
    row[j] = v;
  }
  if (tid == 0) rhs[(long long)bl * Npad + i] = Sa[nc * nc + g];
}

// grid: (nsamp); 256 threads; dynamic LDS: Npad doubles (the vector).
// dense: Npad x Npad per sample (lower triangle; L_c is left there); z: the
// chunk's normals, n_coef per sample (NULL: the mean), the common columns of
// pulsar a at cstart[a]; xc: Npad per sample.  A failed pivot sets sfail[bl].
__global__ __launch_bounds__(CJ_THREADS) void cond_joint_dense_kernel(double* __restrict__ dense, int Npad, int P, int nc,
                                                                      const double* __restrict__ rhs,
                                                                      const double* __restrict__ z, long long n_coef,
                                                                      const int* __restrict__ cstart, int nsamp,
                                                                      int* __restrict__ sfail, double* __restrict__ xc) {
  extern __shared__ __attribute__((aligned(16))) double dv[];
  __shared__ double Ls[16 * CJ_LDT];
  __shared__ int s_fail;
  const int bl = blockIdx.x, tid = threadIdx.x, N = P * nc;
  EWH_DCHECK(bl < nsamp && Npad % 16 == 0 && N <= Npad, "cond_joint_dense shape");
  if (sfail[bl]) return;
  double* A = dense + (long long)bl * Npad * Npad;
  if (tid == 0) s_fail = 0;
  for (int j = tid; j < Npad; j += CJ_THREADS) dv[j] = rhs[(long long)bl * Npad + j];
  __syncthreads();
  if (!cj_eliminate(A, Npad, Npad, Npad, Ls, &s_fail)) {
    if (tid == 0) sfail[bl] = 1;
    return;
  }
  cj_forward(A, Npad, Npad, Npad, dv, Ls);
  if (z)
    for (int j = tid; j < N; j += CJ_THREADS) {
      const int a = j / nc, g = j - a * nc;
      EWH_DCHECK(cstart[a] + g < n_coef, "cond_joint_dense z index");
      dv[j] += z[(long long)bl * n_coef + cstart[a] + g];
    }
  __syncthreads();
  cj_backward(A, Npad, Npad, dv, Ls);
  for (int j = tid; j < Npad; j += CJ_THREADS) xc[(long long)bl * Npad + j] = dv[j];
}

// grid: (nsamp); 256 threads.  G: pulsar p's retained slots (L_A, W, y_a in the
// r row); xc: the sample's x_c (Npad per sample), this pulsar's at xc_off; z:
// the chunk's normals (n_coef per sample; this pulsar's columns from z_off, the
// first nlo of them the own block's; NULL: the mean).  x: ld per unit, [x_a |
// x_c,p | 0].  status: 0; 1 where this pulsar's own block failed; 3 where the
// sample failed elsewhere (x is then NaN on the m columns).
__global__ __launch_bounds__(CJ_THREADS) void cond_joint_back_kernel(const double* __restrict__ G, int ld, int mo, int nc,
                                                                     int nlo, const double* __restrict__ xc, int Npad,
                                                                     int xc_off, const double* __restrict__ z,
                                                                     long long n_coef, long long z_off,
                                                                     const int* __restrict__ pstat,
                                                                     const int* __restrict__ sfail, int nsamp,
                                                                     double* __restrict__ x, int* __restrict__ status) {
  __shared__ double d[WIDE_LD_MAX];
  __shared__ double Ls[16 * CJ_LDT];
  const int bl = blockIdx.x, tid = threadIdx.x, m = mo + nc;
  EWH_DCHECK(bl < nsamp && mo >= 1 && nlo <= mo && m < ld && ld <= WIDE_LD_MAX && xc_off + nc <= Npad,
             "cond_joint_back shape");
  const double* A = G + (long long)bl * ld * ld;
  double* xo = x + (long long)bl * ld;
  if (pstat[bl] != 0 || sfail[bl] != 0) {
    const double qnan = __builtin_nan("");
    for (int j = tid; j < ld; j += CJ_THREADS) xo[j] = j < m ? qnan : 0.0;
    if (tid == 0) status[bl] = pstat[bl] != 0 ? 1 : 3;
    return;
  }
  const double* xs = xc + (long long)bl * Npad + xc_off;
  for (int j = tid; j < 16 * ((mo + 15) / 16); j += CJ_THREADS) {
    double s = 0.0;
    if (j < mo) {
      s = A[(long long)(ld - 1) * ld + j];
      if (z && j < nlo) s += z[(long long)bl * n_coef + z_off + j];
      for (int g = 0; g < nc; ++g) s = fma(-A[(long long)(mo + g) * ld + j], xs[g], s);
    }
    d[j] = s;
  }
  __syncthreads();
  cj_backward(A, ld, mo, d, Ls);
  for (int j = tid; j < ld; j += CJ_THREADS) xo[j] = j < mo ? d[j] : j < m ? xs[j - mo] : 0.0;
  if (tid == 0) status[bl] = 0;
}

int launch_cond_joint_partial(double* G, int ld, int mo, int nc, const int* col_ptr, const DSpec* spec,
                              const double* theta, int ldth, int nsamp, double* S, int* status, hipStream_t st) {
  if (nsamp <= 0) return 0;
  if (mo < 1 || nc < 1) return set_err(EWH_E_INVALID, "joint conditional GP: an empty own or common block");
  if (ld > WIDE_LD_MAX || mo + nc >= ld)
    return set_err(EWH_E_UNSUPPORTED, "joint conditional GP: basis wider than 1023 columns");
  hipLaunchKernelGGL(cond_joint_partial_kernel, dim3((unsigned)nsamp), dim3(CJ_THREADS), 0, st, G, ld, mo, nc, col_ptr,
                     spec, theta, ldth, nsamp, S, status);
  EWH_HIP(hipGetLastError());
  return 0;
}

int cond_joint_npad(int P, int nc) { return 16 * ((P * nc + 15) / 16); }

int launch_cond_joint_dense(const double* S, long long sstride, int P, int nc, int nsamp, const int* pstat,
                            const double* minv, const double* mlog, const int* rep, double* dense, double* rhs,
                            const double* z, long long n_coef, const int* cstart, int* sfail, double* xc,
                            hipStream_t st) {
  if (nsamp <= 0) return 0;
  const long long N = (long long)P * nc;
  if (N > COND_JOINT_NC_MAX)
    return set_err(EWH_E_UNSUPPORTED, "joint conditional GP: Sigma_c of " + std::to_string(N) +
                                          " columns; the dense solve holds its vector in LDS, at most " +
                                          std::to_string(COND_JOINT_NC_MAX));
  const int Npad = cond_joint_npad(P, nc);
  hipLaunchKernelGGL(cond_joint_assemble_kernel, dim3((unsigned)Npad, (unsigned)nsamp), dim3(256), 0, st, S, sstride, P,
                     nc, nsamp, pstat, minv, mlog, rep, Npad, dense, rhs, sfail);
  EWH_HIP(hipGetLastError());
  const size_t lds = (size_t)Npad * sizeof(double);
  if (lds > 32 * 1024)
    EWH_HIP(hipFuncSetAttribute((const void*)cond_joint_dense_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(cond_joint_dense_kernel, dim3((unsigned)nsamp), dim3(CJ_THREADS), lds, st, dense, Npad, P, nc, rhs,
                     z, n_coef, cstart, nsamp, sfail, xc);
  EWH_HIP(hipGetLastError());
  return 0;
}

int launch_cond_joint_back(const double* G, int ld, int mo, int nc, int nlo, const double* xc, int Npad, int xc_off,
                           const double* z, long long n_coef, long long z_off, const int* pstat, const int* sfail,
                           int nsamp, double* x, int* status, hipStream_t st) {
  if (nsamp <= 0) return 0;
  hipLaunchKernelGGL(cond_joint_back_kernel, dim3((unsigned)nsamp), dim3(CJ_THREADS), 0, st, G, ld, mo, nc, nlo, xc,
                     Npad, xc_off, z, n_coef, z_off, pstat, sfail, nsamp, x, status);
  EWH_HIP(hipGetLastError());
  return 0;
}

}  // namespace ewh_dev
