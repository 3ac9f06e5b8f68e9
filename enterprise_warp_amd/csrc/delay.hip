// delay.hip — deterministic delay signals (ABI 8: ewh_pulsar_desc::delays).
//
// A delay pulsar's residual column differs per sample: r'_b = r - sum_k
// delta_k(theta_b), as enterprise forms r - delta before the likelihood.  Per
// chunk of samples the column of the unit's matrix that carries r is REPLACED
// (never corrected from cached values):
//   delay_resid_kernel   R[t][b] = r'_b[t] and Z[t][b] = w_b[t] r'_b[t], both
//                        TOA-major (n_toa x zld, zld = the chunk padded to 16
//                        samples) so the GEMM's two operands load coalesced
//   delay_ecorr_kernel   ECORR epochs (contiguous TOA slices), the Sherman-
//                        Morrison convention of wn_weights_kernel:
//                        z[t] = w[t] (r'[t] - beta_e sum_{s in e} w[s] r'[s])
//   delay_gemm_kernel    C = T_aug^T Z on v_mfma_f64_16x16x4_f64 (16 basis
//                        columns x 16 samples x 4 TOA rows per instruction),
//                        accumulated in 64-row groups whose partial sums are
//                        added by TwoSum (hi + lo); the corner r'^T z by VALU
//                        from the same tiles
//   delay_bgroup_kernel  the same column for a theta-dependent basis (the A
//                        operand then differs per sample: VALU)
//   delay_scatter_kernel the column (hi, lo) into the last row and column of
//                        the chunk's G (and G_lo) slots
//   gram_broadcast_kernel fixed white noise: the cached full-width Gram of a
//                        delay pulsar (hi, lo) and its -1/2 log|N| into the
//                        chunk's slots; T^T N^-1 T is not contracted again
// The per-unit factorisation kernels then run unmodified on those slots.
// Launch wrappers: ewarp_launch.h.
#include "ewarp_launch.h"

namespace ewh_dev {

namespace {

constexpr int DG_ROWS = 64;                       // TOA rows per accumulation group
constexpr double DAY_S = 86400.0;
constexpr double TWO_PI_FYR = 2.0 * M_PI * (1.0 / (365.25 * 86400.0));   // as numpy: (2 pi fyr) t

// s + e = a + b exactly (Knuth); compiled with contraction off
__device__ __forceinline__ void two_sum(double a, double b, double& s, double& e) {
#pragma clang fp contract(off)
  s = a + b;
  const double bp = s - a;
  e = (a - (s - bp)) + (b - bp);
}

}  // namespace

// grid: (ceil(n_toa / 64), ceil(zld / 64)); 256 threads = 64 samples x 4 TOA lanes
__global__ __launch_bounds__(256) void delay_resid_kernel(PsrDev P, DelayDev D, const double* __restrict__ theta,
                                                          int ldth, int b0, int nsamp,
                                                          const double* __restrict__ w, long long wstride,
                                                          double* __restrict__ R, double* __restrict__ Z, int zld,
                                                          double* __restrict__ Kb) {
  __shared__ double s_amp[DELAY_MAX][64], s_a[DELAY_MAX][64], s_b[DELAY_MAX][64];
  const int bx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int bl = blockIdx.y * 64 + bx;            // chunk-local sample
  const bool live = bl < nsamp;
  EWH_DCHECK(D.n_delay >= 1 && D.n_delay <= DELAY_MAX, "delay_resid entry count");
  if (ty == 0) {
    bool bad = false;
    for (int k = 0; k < D.n_delay; ++k) {
      double amp = 0.0, a = 0.0, b = 0.0;
      if (live) {
        const DDelay e = D.ent[k];
        const double* th = theta + (long long)(b0 + bl) * ldth;
        amp = exp(LN10 * dpar(e.i0, e.v0, th));
        if (e.kind == EWH_DELAY_EXP_DIP) {
          const double tau = exp(LN10 * dpar(e.i1, e.v1, th)) * DAY_S;
          const double sp = dpar(e.i3, e.v3, th);
          a = dpar(e.i2, e.v2, th) * DAY_S;
          b = -1.0 / tau;
          bad = bad || !(tau > 0.0) || !isfinite(tau) || !isfinite(a) || !isfinite(sp);
          amp *= sp > 0.0 ? 1.0 : (sp < 0.0 ? -1.0 : 0.0);     // np.sign
        } else {
          a = dpar(e.i1, e.v1, th);
          bad = bad || !isfinite(a);
        }
        bad = bad || !isfinite(amp);
      }
      s_amp[k][bx] = amp;
      s_a[k][bx] = a;
      s_b[k][bx] = b;
    }
    if (bad) {              // lnL = -inf for this sample alone: no delay, K = -inf
      for (int k = 0; k < D.n_delay; ++k) s_amp[k][bx] = s_a[k][bx] = s_b[k][bx] = 0.0;
      if (blockIdx.x == 0) Kb[bl] = -INFINITY;
    }
  }
  __syncthreads();
  if (bl >= zld) return;
  for (int i = ty; i < 64; i += 4) {
    const int t = blockIdx.x * 64 + i;
    if (t >= P.n_toa) break;
    double v = 0.0, wt = 0.0;
    if (live) {
      const double tt = D.toas[t], lnc = P.ln_chrom[t];
      double del = 0.0;
      for (int k = 0; k < D.n_delay; ++k) {
        const double amp = s_amp[k][bx], a = s_a[k][bx];
        const double chrom = exp(D.ent[k].idx * lnc);
        if (D.ent[k].kind == EWH_DELAY_EXP_DIP) {
          const double dt = tt - a;
          if (dt >= 0.0) del += amp * (dt > 0.0 ? exp(dt * s_b[k][bx]) : 1.0) * chrom;
        } else {
          del += amp * sin(TWO_PI_FYR * tt + a) * chrom;
        }
      }
      v = P.T[(long long)t * P.ld + P.ld - 1] - del;
      wt = w[(long long)bl * wstride + t];
    }
    EWH_DCHECK(t >= 0 && bl >= 0 && bl < zld, "delay_resid Z index");
    R[(long long)t * zld + bl] = v;
    Z[(long long)t * zld + bl] = wt * v;
  }
}

// grid: (n_epoch, ceil(zld / 64)); 64 threads, one per sample
__global__ __launch_bounds__(64) void delay_ecorr_kernel(PsrDev P, int nsamp, const double* __restrict__ w,
                                                         long long wstride, const double* __restrict__ beta,
                                                         long long bstride, const double* __restrict__ R,
                                                         double* __restrict__ Z, int zld) {
  const int e = blockIdx.x, bl = blockIdx.y * 64 + threadIdx.x;
  if (bl >= nsamp) return;
  const int t0 = P.ep_start[e], t1 = P.ep_stop[e];
  EWH_DCHECK(t0 >= 0 && t1 <= P.n_toa && bl < zld, "delay_ecorr epoch slice");
  const double* wr = w + (long long)bl * wstride;
  double s = 0.0;
  for (int t = t0; t < t1; ++t) s = fma(wr[t], R[(long long)t * zld + bl], s);
  const double bs = beta[(long long)bl * bstride + e] * s;
  for (int t = t0; t < t1; ++t) Z[(long long)t * zld + bl] = wr[t] * (R[(long long)t * zld + bl] - bs);
}

// C[j][b] = sum_t T_aug[t][j] Z[t][b].  grid: (ld / 16, zld / 16); 4 waves, wave
// v takes the 64-row groups v, v + 4, ...; lane l = (q = l >> 4, c = l & 15)
// holds A[i = c][k = q] = T_aug[t0 + q][16 jb + c], B[k = q][j = c] =
// Z[t0 + q][16 bg + c]; D: column (sample) c, row (basis column) q + 4 r.
// The waves' sums are folded in wave order (TwoSum), so the result does not
// depend on scheduling.  Row ld - 1 (stored r) is skipped; the block row that
// holds it also forms the corner r'^T z from R and Z.
__global__ __launch_bounds__(256) void delay_gemm_kernel(PsrDev P, int nsamp, const double* __restrict__ R,
                                                         const double* __restrict__ Z, int zld,
                                                         double* __restrict__ col_hi, double* __restrict__ col_lo) {
  __shared__ double red_hi[3][4][64], red_lo[3][4][64], c_hi[256], c_lo[256];
  const int jb = blockIdx.x, bg = blockIdx.y;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, q = lane >> 4, c = lane & 15;
  const int ld = P.ld, n = P.n_toa;
  const bool corner = jb == (int)gridDim.x - 1;
  EWH_DCHECK(16 * (int)gridDim.x == ld && 16 * (bg + 1) <= zld, "delay_gemm grid against ld / zld");
  const double* Tc = P.T + 16 * jb + c;
  const double* Zc = Z + 16 * bg + c;
  const double* Rc = R + 16 * bg + c;
  v4d thi = {0.0, 0.0, 0.0, 0.0}, tlo = {0.0, 0.0, 0.0, 0.0};
  double chi = 0.0, clo = 0.0;
  for (int t0 = wave * DG_ROWS; t0 < n; t0 += 4 * DG_ROWS) {
    double a[DG_ROWS / 4], b[DG_ROWS / 4];
#pragma unroll
    for (int kk = 0; kk < DG_ROWS / 4; ++kk) {
      const int t = t0 + 4 * kk + q;
      const bool ok = t < n;
      a[kk] = ok ? Tc[(long long)t * ld] : 0.0;
      b[kk] = ok ? Zc[(long long)t * zld] : 0.0;
    }
    if (corner) {
      double ca = 0.0;
#pragma unroll
      for (int kk = 0; kk < DG_ROWS / 4; ++kk) {
        const int t = t0 + 4 * kk + q;
        ca = fma(t < n ? Rc[(long long)t * zld] : 0.0, b[kk], ca);
      }
      double s, e;
      two_sum(chi, ca, s, e);
      chi = s;
      clo += e;
    }
    v4d acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < DG_ROWS / 4; ++kk) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kk], b[kk], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double s, e;
      two_sum(thi[r], acc[r], s, e);
      thi[r] = s;
      tlo[r] += e;
    }
  }
  if (wave > 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      red_hi[wave - 1][r][lane] = thi[r];
      red_lo[wave - 1][r][lane] = tlo[r];
    }
  }
  c_hi[threadIdx.x] = chi;
  c_lo[threadIdx.x] = clo;
  __syncthreads();
  if (wave != 0) return;
  const int bl = 16 * bg + c;
  for (int v = 0; v < 3; ++v) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double s, e;
      two_sum(thi[r], red_hi[v][r][lane], s, e);
      thi[r] = s;
      tlo[r] += e + red_lo[v][r][lane];
    }
  }
  if (bl < nsamp) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * jb + q + 4 * r;
      if (row == ld - 1) continue;
      const double v = thi[r] + tlo[r];
      EWH_DCHECK(row >= 0 && row < ld, "delay_gemm column row");
      col_hi[(long long)bl * ld + row] = v;
      col_lo[(long long)bl * ld + row] = (thi[r] - v) + tlo[r];
    }
    if (corner && q == 0) {       // the 16 partial corners of sample c: (wave, q) in order
      double hi = 0.0, lo = 0.0;
      for (int i = 0; i < 16; ++i) {
        const int src = (i >> 2) * 64 + (i & 3) * 16 + c;
        double s, e;
        two_sum(hi, c_hi[src], s, e);
        hi = s;
        lo += e + c_lo[src];
      }
      const double v = hi + lo;
      col_hi[(long long)bl * ld + ld - 1] = v;
      col_lo[(long long)bl * ld + ld - 1] = (hi - v) + lo;
    }
  }
}

// theta-dependent basis: column c of sample bl is T_aug[t][c] fac_g(c)[t];
// grid: (nsamp); thread c over the ld columns, the sums in 64-row groups
__global__ __launch_bounds__(256) void delay_bgroup_kernel(PsrDev P, const double* __restrict__ fac,
                                                           const double* __restrict__ R,
                                                           const double* __restrict__ Z, int zld,
                                                           double* __restrict__ col_hi, double* __restrict__ col_lo) {
  const int bl = blockIdx.x, ld = P.ld, n = P.n_toa;
  EWH_DCHECK(bl < zld, "delay_bgroup sample");
  for (int c = threadIdx.x; c < ld; c += 256) {
    const int g = P.n_bgroup ? P.col_bgroup[c] : -1;
    const double* fr = g >= 0 ? fac + ((long long)bl * P.n_bgroup + g) * n : nullptr;
    double tot = 0.0;
    for (int t0 = 0; t0 < n; t0 += DG_ROWS) {
      double a = 0.0;
      const int t1 = min(n, t0 + DG_ROWS);
      for (int t = t0; t < t1; ++t) {
        double x = c == ld - 1 ? R[(long long)t * zld + bl] : P.T[(long long)t * ld + c];
        if (g >= 0) x *= fr[t];
        a = fma(x, Z[(long long)t * zld + bl], a);
      }
      tot += a;
    }
    col_hi[(long long)bl * ld + c] = tot;
    col_lo[(long long)bl * ld + c] = 0.0;
  }
}

// grid: (nsamp)
__global__ __launch_bounds__(256) void delay_scatter_kernel(int ld, const double* __restrict__ col_hi,
                                                            const double* __restrict__ col_lo,
                                                            double* __restrict__ G, double* __restrict__ Glo) {
  const int bl = blockIdx.x;
  double* g = G + (long long)bl * ld * ld;
  double* gl = Glo ? Glo + (long long)bl * ld * ld : nullptr;
  for (int c = threadIdx.x; c < ld; c += 256) {
    const double v = col_hi[(long long)bl * ld + c], l = col_lo[(long long)bl * ld + c];
    g[(long long)c * ld + ld - 1] = v;
    g[(long long)(ld - 1) * ld + c] = v;
    if (gl) {
      gl[(long long)c * ld + ld - 1] = l;
      gl[(long long)(ld - 1) * ld + c] = l;
    }
  }
}

// grid: (blocks over n, nsamp)
__global__ __launch_bounds__(256) void gram_broadcast_kernel(const double* __restrict__ src_hi,
                                                             const double* __restrict__ src_lo, long long n,
                                                             double Kval, double* __restrict__ G,
                                                             double* __restrict__ Glo, double* __restrict__ Kb) {
  const int bl = blockIdx.y;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += 256LL * gridDim.x) {
    G[(long long)bl * n + i] = src_hi[i];
    Glo[(long long)bl * n + i] = src_lo[i];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) Kb[bl] = Kval;
}

int launch_delay_column(const PsrDev& P, const DelayDev& D, const double* theta, int ldth, int b0, int nsamp,
                        const double* w, long long wstride, const double* beta, long long bstride,
                        const double* fac, double* R, double* Z, double* col_hi, double* col_lo, double* Kb,
                        hipStream_t st) {
  if (nsamp <= 0) return 0;
  if (D.n_delay < 1 || D.n_delay > DELAY_MAX) return set_err(EWH_E_UNSUPPORTED, "more than 8 delay entries on a pulsar");
  const int zld = 16 * ((nsamp + 15) / 16);
  const unsigned tg = (unsigned)((P.n_toa + 63) / 64), sg = (unsigned)((zld + 63) / 64);
  hipLaunchKernelGGL(delay_resid_kernel, dim3(tg, sg), dim3(256), 0, st, P, D, theta, ldth, b0, nsamp, w, wstride, R,
                     Z, zld, Kb);
  if (P.n_epoch > 0)
    hipLaunchKernelGGL(delay_ecorr_kernel, dim3((unsigned)P.n_epoch, sg), dim3(64), 0, st, P, nsamp, w, wstride, beta,
                       bstride, R, Z, zld);
  if (P.n_bgroup > 0)
    hipLaunchKernelGGL(delay_bgroup_kernel, dim3((unsigned)nsamp), dim3(256), 0, st, P, fac, R, Z, zld, col_hi, col_lo);
  else
    hipLaunchKernelGGL(delay_gemm_kernel, dim3((unsigned)(P.ld / 16), (unsigned)(zld / 16)), dim3(256), 0, st, P, nsamp,
                       R, Z, zld, col_hi, col_lo);
  EWH_HIP(hipGetLastError());
  return 0;
}

void launch_delay_scatter(int ld, int nsamp, const double* col_hi, const double* col_lo, double* G, double* Glo,
                          hipStream_t st) {
  if (nsamp <= 0) return;
  hipLaunchKernelGGL(delay_scatter_kernel, dim3((unsigned)nsamp), dim3(256), 0, st, ld, col_hi, col_lo, G, Glo);
}

void launch_gram_broadcast(const double* src_hi, const double* src_lo, long long n, double Kval, int nsamp, double* G,
                           double* Glo, double* Kb, hipStream_t st) {
  if (nsamp <= 0) return;
  const unsigned gx = (unsigned)std::min<long long>(64, (n + 255) / 256);
  hipLaunchKernelGGL(gram_broadcast_kernel, dim3(gx, (unsigned)nsamp), dim3(256), 0, st, src_hi, src_lo, n, Kval, G,
                     Glo, Kb);
}

}  // namespace ewh_dev
