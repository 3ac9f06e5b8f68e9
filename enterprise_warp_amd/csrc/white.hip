// white.hip — white-noise preparation and the double-double setup:
// wn_weights (N^-1, ECORR Sherman-Morrison terms, -1/2 log|N|), the ECORR
// epoch sums, the double-double Grams (fixed white noise, and the units whose
// fp64 factorisation failed), the fixed-white-noise timing-model elimination
// (schur) and the reversed verify pass's input.  Launch wrappers:
// ewarp_launch.h.
#include "ewarp_launch.h"

namespace ewh_dev {

// ----------------------------------------------------------------------------
// white noise: w_t = 1/N_t, ECORR beta_e, -1/2 log|N|     ([ent] ShermanMorrison)
// grid: one 256-thread block per sample of the chunk
// ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void wn_weights_kernel(PsrDev P, const double* __restrict__ theta,
                                                         int ldth, int b0, double* __restrict__ w,
                                                         double* __restrict__ beta,
                                                         double* __restrict__ Kb, double* __restrict__ fac,
                                                         double* __restrict__ rho) {
  __shared__ double red[4];
  const int bl = blockIdx.x;
  const double* th = theta + (long long)(b0 + bl) * ldth;
  double* wr = w + (long long)bl * P.n_toa;
  // theta-dependent chromatic basis: fac[t][g] = (1400/nu_t)^idx_g
  for (int g = 0; g < P.n_bgroup; ++g) {
    const double idx = pref_val(P.bgroup[g], th);
    double* fr = fac + ((long long)bl * P.n_bgroup + g) * P.n_toa;
    for (int t = threadIdx.x; t < P.n_toa; t += 256) fr[t] = exp(idx * P.ln_chrom[t]);
  }
  double acc = 0.0;
  for (int t = threadIdx.x; t < P.n_toa; t += 256) {
    const double ef = pref_val(P.slots[P.efac_slot[t]], th);
    double D = ef * ef * P.sig2[t];                       // MeasurementNoise
    const int qs = P.equad_slot[t];
    if (qs >= 0) D += pow(10.0, 2.0 * pref_val(P.slots[qs], th));  // TNEquadNoise
    wr[t] = 1.0 / D;
    acc += log(D);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < P.n_epoch; e += 256) {   // EcorrKernelNoise
    double s = 0.0;
    for (int t = P.ep_start[e]; t < P.ep_stop[e]; ++t) s += wr[t];
    const double J = pow(10.0, 2.0 * pref_val(P.slots[P.ep_slot[e]], th));
    const double be = 1.0 / (s + 1.0 / J);
    beta[(long long)bl * P.n_epoch + e] = be;
    acc += log(J) - log(be);
  }
  acc = block_sum256(acc, red);
  if (threadIdx.x == 0) Kb[bl] = -0.5 * acc;
  if (rho) {
    // r^T W r (no ECORR: the r-separated contraction, contract2 RSEP): r is
    // T_aug's last column; per thread a strided partial sum, then the tree
    double q = 0.0;
    for (int t = threadIdx.x; t < P.n_toa; t += 256) {
      const double r = P.T[(long long)t * P.ld + P.ld - 1];
      q = fma(wr[t] * r, r, q);
    }
    q = block_sum256(q, red);
    if (threadIdx.x == 0) rho[bl] = q;
  }
}

// s[bl][e][:] = sum_{t in epoch e} w_t T_aug[t][:]
__global__ __launch_bounds__(256) void epoch_sums_kernel(PsrDev P, const double* __restrict__ w,
                                                         const double* __restrict__ fac,
                                                         double* __restrict__ s) {
  const int e = blockIdx.x, bl = blockIdx.y;
  const double* wr = w + (long long)bl * P.n_toa;
  double* out = s + ((long long)bl * P.n_epoch + e) * P.ld;
  const int t0 = P.ep_start[e], t1 = P.ep_stop[e];
  for (int c = threadIdx.x; c < P.ld; c += 256) {
    const int g = P.n_bgroup ? P.col_bgroup[c] : -1;
    const double* fr = g >= 0 ? fac + ((long long)bl * P.n_bgroup + g) * P.n_toa : nullptr;
    double a = 0.0;
    for (int t = t0; t < t1; ++t) {
      const double x = P.T[(long long)t * P.ld + c];
      a += wr[t] * (g >= 0 ? x * fr[t] : x);
    }
    out[c] = a;
  }
}

// The same for ES_S samples per workgroup (round 5, the varying-white-noise
// wide path: the per-(epoch, sample) kernel above re-read the epoch's T rows
// from L2 / MALL for every sample -- 1.0 ms per 256 samples at 384 columns x
// 10k TOAs, 8 % of the w372 batch): the epoch's rows of each column are read
// once into registers (ES_R at a time), the group's weights staged in LDS
// (epochs up to ES_RMAX TOAs; longer ones, and theta-dependent bases, keep
// the kernel above).  s[b][e][c] = sum_t w_bt T[t][c], the terms in TOA
// order by fma.
constexpr int ES_S = 32, ES_R = 16, ES_RMAX = 128;
__global__ __launch_bounds__(256) void epoch_sums_multi_kernel(PsrDev P, const double* __restrict__ w, int nsamp,
                                                               double* __restrict__ s) {
  __shared__ double ws[ES_S * ES_RMAX];
  const int e = blockIdx.x, s0 = blockIdx.y * ES_S;
  const int t0 = P.ep_start[e], nr = P.ep_stop[e] - t0;
  const int ns = min(ES_S, nsamp - s0);
  for (int i = threadIdx.x; i < ES_S * nr; i += 256) {
    const int sl = i / nr, r = i - sl * nr;
    ws[sl * ES_RMAX + r] = sl < ns ? w[(long long)(s0 + sl) * P.n_toa + t0 + r] : 0.0;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < P.ld; c += 256) {
    double acc[ES_S];
#pragma unroll
    for (int sl = 0; sl < ES_S; ++sl) acc[sl] = 0.0;
    for (int r0 = 0; r0 < nr; r0 += ES_R) {
      double tv[ES_R];
#pragma unroll
      for (int r = 0; r < ES_R; ++r) tv[r] = r0 + r < nr ? P.T[(long long)(t0 + r0 + r) * P.ld + c] : 0.0;
      const int rn = min(ES_R, nr - r0);
#pragma unroll
      for (int sl = 0; sl < ES_S; ++sl) {
        const double* wl = ws + sl * ES_RMAX + r0;
#pragma unroll
        for (int r = 0; r < ES_R; ++r)
          if (r < rn) acc[sl] = fma(wl[r], tv[r], acc[sl]);
      }
    }
#pragma unroll
    for (int sl = 0; sl < ES_S; ++sl)
      if (sl < ns) s[((long long)(s0 + sl) * P.n_epoch + e) * P.ld + c] = acc[sl];
  }
}

// ----------------------------------------------------------------------------
// The double-double Gram G = X^T W X - sum_e beta_e s_e s_e^T of one pulsar,
// X = T_aug = X_hi + X_lo: X_hi the projected basis the fp64 kernels read
// (P.T), X_lo its projection residual (PsrHost::d_Tlo, round 6: X_hi + X_lo =
// T - M C to double-double, create_ctx), so the Gram is that of the exactly
// projected basis -- an exact reparametrisation of enterprise's -- and the
// projection's fp64 rounding (a basis perturbation of O(eps |M C|), up to
// ~1e-14 of the projected column's own size) stays out.  Every w_t X_ta X_tb
// is summed in double-double (Dot2, Ogita-Rump-Oishi 2005: TwoProd by fma,
// TwoSum): w X_a,hi is itself split by TwoProd, so each hi x hi term is exact
// with only w_t = 1/N_t rounded once (a relative perturbation of N_t by <=
// 2^-53, benign: it keeps G a Gram); the cross terms w (X_a,hi X_b,lo +
// X_a,lo X_b,hi) are added to the low part in fp64.  The ECORR epoch sums
// s_e = sum over the epoch of w_t (X_hi + X_lo)_t are formed here in fp64
// (<= 16-32 TOAs).  Rounds 2-5 summed the Gram of the rounded projected basis:
// on ill-conditioned prior draws that left the device's double-double twin
// ~16x strict from the CPU double-double value on C3 and made C4 units
// indefinite (tests/test_gpu_parity.py::test_headline_matches_dd_at_scale,
// test_c4_bench_inf_sets_at_scale).  One workgroup per upper 16x16 block,
// thread (ty, tx) -> entry (16 bi + ty, 16 bj + tx); 32-row chunks staged in
// LDS.  Writes G_hi / G_lo of block (bi, bj) (both triangles).
__device__ __forceinline__ void gram_dd_block(const PsrDev& P, const double* __restrict__ Xlo,
                                              const double* __restrict__ w, const double* __restrict__ beta, int bi,
                                              int bj, double* __restrict__ G, double* __restrict__ Glo,
                                              double (*Ta)[17], double (*Tb)[17], double (*Ua)[17], double (*Ub)[17],
                                              double* wv) {
#pragma clang fp contract(off)
  const int LD = P.ld;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  dd acc = {0.0, 0.0};
  for (int pass = 0; pass < 2; ++pass) {     // TOA rows (w), then epoch rows (-beta)
    const int nrows = pass == 0 ? P.n_toa : P.n_epoch;
    for (int t0 = 0; t0 < nrows; t0 += 32) {
      for (int idx = threadIdx.x; idx < 1024; idx += 256) {
        const int r = idx >> 5, c = idx & 31, cc = c & 15;
        const int col = 16 * (c < 16 ? bi : bj) + cc;
        double v = 0.0, vl = 0.0;
        if (t0 + r < nrows) {
          if (pass == 0) {
            const long long o = (long long)(t0 + r) * LD + col;
            v = P.T[o];
            vl = Xlo ? Xlo[o] : 0.0;
          } else {
            // s_e[col] = sum over the epoch's rows of w_t X_t,col in
            // double-double (round 6; fp64 until then -- a relative rounding
            // of the rank-one ECORR term, i.e. of G itself)
            for (int t = P.ep_start[t0 + r]; t < P.ep_stop[t0 + r]; ++t) {
              const long long o = (long long)t * LD + col;
              const double p = w[t] * P.T[o];
              const double pe = fma(w[t], P.T[o], -p);
              const double sum = v + p, bp = sum - v;
              vl += ((v - (sum - bp)) + (p - bp)) + pe + (Xlo ? w[t] * Xlo[o] : 0.0);
              v = sum;
            }
          }
        }
        if (c < 16) {
          Ta[r][cc] = v;
          Ua[r][cc] = vl;
        } else {
          Tb[r][cc] = v;
          Ub[r][cc] = vl;
        }
      }
      if (threadIdx.x < 32)
        wv[threadIdx.x] = t0 + (int)threadIdx.x < nrows ? (pass == 0 ? w[t0 + threadIdx.x] : -beta[t0 + threadIdx.x])
                                                        : 0.0;
      __syncthreads();
      // the tile's 32 terms by Dot2 into a fresh (hi, lo), then added to the
      // running total in double-double (round 6: one Dot2 over all rows had an
      // error bound of gamma_n^2 sum |terms| -- ~5e-24 of it at 20k TOAs; now
      // gamma_32^2 per tile and 2^-106 per tile fold)
      double hi = 0.0, lo = 0.0;
      for (int r = 0; r < 32; ++r) {
        const double wa = wv[r], ta = Ta[r][ty], yv = Tb[r][tx];
        const double x = wa * ta;
        const double xe = fma(wa, ta, -x);          // TwoProd: w X_a = x + xe exactly
        const double pr = x * yv;
        const double pe = fma(x, yv, -pr);          // TwoProd: x X_b = pr + pe exactly
        const double sum = hi + pr;                 // TwoSum: hi + pr = sum + se exactly
        const double bp = sum - hi;
        const double se = (hi - (sum - bp)) + (pr - bp);
        hi = sum;
        // + the low parts' cross terms (X_lo, or the epoch sums' low parts)
        lo += se + fma(xe, yv, pe) + wa * fma(ta, Ub[r][tx], Ua[r][ty] * yv);
      }
      acc = dd_add_ieee(acc, dd_two_sum(hi, lo));
      __syncthreads();
    }
  }
  const int row = 16 * bi + ty, col = 16 * bj + tx;
  if (row > col) return;      // diagonal block: the upper entry's thread writes both (exactly symmetric)
  dd v = acc;
  // (the register kernels' front-pad order reads the pads' entries
  // themselves, ewarp_dev.h front_src: a pad must be an exact identity row and
  // column -- 1 here, zeros from T_aug's zero pad columns)
  if (row == col && row >= P.m && row < LD - 1) v = {1.0, 0.0};   // unit pads, as the contraction kernels
  G[(long long)row * LD + col] = v.hi;
  G[(long long)col * LD + row] = v.hi;
  Glo[(long long)row * LD + col] = v.lo;
  Glo[(long long)col * LD + row] = v.lo;
}

__device__ __forceinline__ void upper_block(int blk, int nb, int& bi, int& bj) {
  bi = 0;
  while (blk >= nb - bi) { blk -= nb - bi; ++bi; }
  bj = bi + blk;
}

// fixed white noise, one-off (ewh_create / ewh_set_fixed_white): the cached
// Gram for the double-double timing-model elimination (schur_kernel).  One
// fp64 MFMA accumulator over 20k TOAs had moved prior-draw lnL by up to 7e-2
// on C3 through the ill-conditioned elimination (round 2,
// tests/test_gpu_parity.py::test_c3_bench_workload_prior_draws).  (Chromatic
// `vary` bases never take this path: their basis is theta-dependent, so white
// noise is not cached.)
__global__ __launch_bounds__(256) void gram_dd_kernel(PsrDev P, const double* __restrict__ Xlo,
                                                      const double* __restrict__ w,
                                                      const double* __restrict__ beta, double* __restrict__ G,
                                                      double* __restrict__ Glo) {
  __shared__ double Ta[32][17], Tb[32][17], Ua[32][17], Ub[32][17], wv[32];
  int bi, bj;
  upper_block(blockIdx.x, P.nb, bi, bj);
  gram_dd_block(P, Xlo, w, beta, bi, bj, G, Glo, Ta, Tb, Ua, Ub, wv);
}

// Round 6: the same Gram for the varying-white-noise units whose fp64
// factorisation failed (a pivot <= 0: an -inf term), listed by the failure
// scan (verify_units_kernel on the unit terms alone).  The exact Sigma of a
// full-rank basis is positive definite, so such an -inf is a rounding failure
// of the fp64 Gram or factorisation; the unit is refactored by chol_dd_kernel
// on this G_hi + G_lo (tests/test_gpu_parity.py::
// test_c4_bench_inf_sets_at_scale).  Grid (upper blocks, list slots): slot y
// takes list entries y, y + gridDim.y, ...; unit u -> sample b = u % B, row
// j = b - b_off of the chunk's per-sample weights / beta and of G (stride
// ld^2).
__global__ __launch_bounds__(256) void gram_dd_units_kernel(PsrDev P, const double* __restrict__ Xlo,
                                                            const double* __restrict__ w,
                                                            const double* __restrict__ beta,
                                                            const int* __restrict__ list,
                                                            const int* __restrict__ count, int B, int b_off,
                                                            double* __restrict__ G, double* __restrict__ Glo) {
  __shared__ double Ta[32][17], Tb[32][17], Ua[32][17], Ub[32][17], wv[32];
  int bi, bj;
  upper_block(blockIdx.x, P.nb, bi, bj);
  const int cnt = *count;
  const long long LD2 = (long long)P.ld * P.ld;
  for (int y = blockIdx.y; y < cnt; y += gridDim.y) {
    const int jb = list[y] % B - b_off;
    gram_dd_block(P, Xlo, w + (long long)jb * P.n_toa, beta + (long long)jb * P.n_epoch, bi, bj, G + jb * LD2,
                  Glo + jb * LD2, Ta, Tb, Ua, Ub, wv);
  }
}

// ----------------------------------------------------------------------------
// fixed white noise: eliminate the leading constant-phi (timing-model) block
// of G = Ghi + Glo once, in double-double (Cholesky, row k scaled by
// 1/sqrt(pivot)); write the reduced matrix S (fx_ld x fx_ld, r last, rounded
// to fp64) and K.  The elimination cancels most of the low-frequency Fourier
// columns' Gram (they are close to the span of the spin-down columns), so it
// runs on the double-double Gram.  One 256-thread block per
// pulsar; Ghi / Glo are modified in place.
// ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void schur_kernel(double* Ghi, double* Glo, int ld, int m, int nlead,
                                                    const int* __restrict__ col_ptr,
                                                    const DSpec* __restrict__ spec,
                                                    double Kb, double* S, int fx_ld, int nloc, int gstart,
                                                    int ncommon, double* Kout, int* fail_out, double* Slo) {
#pragma clang fp contract(off)   // (double-double elimination: ewarp_dev.h)
  __shared__ double rh[256 * 4], rl[256 * 4];
  __shared__ double red[4];
  double lphi = 0.0;
  for (int a = threadIdx.x; a < nlead; a += 256) {
    double ph = 0.0;   // (col_phi written out: the helper swaps an add's operands here, profiles/r17/same_device_code.txt)
    for (int e = col_ptr[a]; e < col_ptr[a + 1]; ++e) ph += spec_phi(spec[e], nullptr);
    const dd v = dd_add({Ghi[(long long)a * ld + a], Glo[(long long)a * ld + a]}, {1.0 / ph, 0.0});
    Ghi[(long long)a * ld + a] = v.hi;
    Glo[(long long)a * ld + a] = v.lo;
    lphi += log(ph);
  }
  lphi = block_sum256(lphi, red);
  __syncthreads();
  double logdet = 0.0;
  int ok = 1;
  for (int k = 0; k < nlead; ++k) {
    const dd piv = {Ghi[(long long)k * ld + k], Glo[(long long)k * ld + k]};
    ok &= piv.hi > 0.0;
    const dd d = dd_sqrt(piv);
    logdet += log(d.hi) + d.lo / d.hi;
    __syncthreads();
    for (int j = k + 1 + threadIdx.x; j < ld; j += 256) {
      const dd x = dd_div({Ghi[(long long)k * ld + j], Glo[(long long)k * ld + j]}, d);
      rh[j] = x.hi;
      rl[j] = x.lo;
    }
    __syncthreads();
    for (int i = k + 1; i < ld; ++i) {
      const dd ri = {rh[i], rl[i]};
      for (int j = k + 1 + threadIdx.x; j < ld; j += 256) {
        const dd v = dd_add({Ghi[(long long)i * ld + j], Glo[(long long)i * ld + j]}, dd_mul({-ri.hi, -ri.lo}, {rh[j], rl[j]}));
        Ghi[(long long)i * ld + j] = v.hi;
        Glo[(long long)i * ld + j] = v.lo;
      }
    }
    __syncthreads();
  }
  // reduced index a -> G column: own columns a < nloc -> nlead + a; common
  // columns gstart <= a < gstart + ncommon -> nlead + nloc + (a - gstart);
  // a == fx_ld - 1 -> r (ld - 1); else an identity pad
  // (an exact one -- 1 on the diagonal, 0 elsewhere: the register kernels'
  // front-pad order reads these entries, ewarp_dev.h front_src)
  auto gmap = [&](int a) {
    if (a < nloc) return nlead + a;
    if (a >= gstart && a < gstart + ncommon) return nlead + nloc + (a - gstart);
    return a == fx_ld - 1 ? ld - 1 : -1;
  };
  for (int idx = threadIdx.x; idx < fx_ld * fx_ld; idx += 256) {
    const int a = idx / fx_ld, bcol = idx % fx_ld;
    const int ga = gmap(a);
    const int gb = gmap(bcol);
    dd v = {(a == bcol) ? 1.0 : 0.0, 0.0};
    if (ga >= 0 && gb >= 0) v = dd_two_sum(Ghi[(long long)ga * ld + gb], Glo[(long long)ga * ld + gb]);
    S[idx] = v.hi;
    if (Slo) Slo[idx] = v.lo;     // (the double-double factorisation's input, chol_dd_kernel)
  }
  if (threadIdx.x == 0) {
    *Kout = Kb - logdet - 0.5 * lphi;
    *fail_out = ok ? 0 : 1;
  }
}

// fl(hi + 2 lo) of a double-double matrix: the reversed verify pass's input
// (chol_wide_kernel forms the same value per load where it is not cached)
__global__ void rev_input_kernel(const double* __restrict__ hi, const double* __restrict__ lo, double* __restrict__ out,
                                 long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = hi[i] + 2.0 * lo[i];
}

// The operand images of a reduced matrix S of nb blocks (ewarp_dev.h
// img_index): one workgroup per upper-triangle block and image, one thread per
// image position.  blockIdx.y 0: the stored order; 1: the front-pad order with
// s leading pads (front NULL: the frame has no dead slice, no such image).
__global__ void operand_image_kernel(const double* __restrict__ S, int nb, int s, double* __restrict__ stored,
                                     double* __restrict__ front) {
  double* const out = blockIdx.y == 0 ? stored : front;
  if (out == nullptr) return;
  const long long k = 256LL * blockIdx.x + threadIdx.x;
  out[k] = S[img_src(nb, img_at(nb, k), blockIdx.y == 0 ? 0 : s)];
}

void launch_wn_weights(const PsrDev& P, const double* theta, int ldth, int b0, int nsamp, double* w, double* beta,
                       double* Kb, double* fac, double* rho, hipStream_t st) {
  hipLaunchKernelGGL(wn_weights_kernel, dim3(nsamp), dim3(256), 0, st, P, theta, ldth, b0, w, beta, Kb, fac, rho);
}

void launch_epoch_sums(const PsrDev& P, int n_epoch, int max_epoch, bool multi, const double* w, const double* fac,
                       double* s, int nsamp, hipStream_t st) {
  if (multi && P.n_bgroup == 0 && max_epoch <= ES_RMAX)
    hipLaunchKernelGGL(epoch_sums_multi_kernel, dim3(n_epoch, (nsamp + ES_S - 1) / ES_S), dim3(256), 0, st, P, w, nsamp,
                       s);
  else
    hipLaunchKernelGGL(epoch_sums_kernel, dim3(n_epoch, nsamp), dim3(256), 0, st, P, w, fac, s);
}

void launch_gram_dd(const PsrDev& P, int nb, const double* Xlo, const double* w, const double* beta, double* G,
                    double* Glo, hipStream_t st) {
  hipLaunchKernelGGL(gram_dd_kernel, dim3(nb * (nb + 1) / 2), dim3(256), 0, st, P, Xlo, w, beta, G, Glo);
}

void launch_gram_dd_units(const PsrDev& P, int nb, unsigned slots, const double* Xlo, const double* w,
                          const double* beta, const int* list, const int* count, int B, int b_off, double* G,
                          double* Glo, hipStream_t st) {
  hipLaunchKernelGGL(gram_dd_units_kernel, dim3(nb * (nb + 1) / 2, slots), dim3(256), 0, st, P, Xlo, w, beta, list,
                     count, B, b_off, G, Glo);
}

void launch_schur(double* Ghi, double* Glo, int ld, int m, int nlead, const int* col_ptr, const DSpec* spec, double Kb,
                  double* S, int fx_ld, int nloc, int gstart, int ncommon, double* Kout, int* fail_out, double* Slo,
                  hipStream_t st) {
  hipLaunchKernelGGL(schur_kernel, dim3(1), dim3(256), 0, st, Ghi, Glo, ld, m, nlead, col_ptr, spec, Kb, S, fx_ld, nloc,
                     gstart, ncommon, Kout, fail_out, Slo);
}

void launch_rev_input(const double* hi, const double* lo, double* out, long long n, hipStream_t st) {
  hipLaunchKernelGGL(rev_input_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, hi, lo, out, n);
}

void launch_operand_image(const double* S, int nb, int s, double* stored, double* front, hipStream_t st) {
  hipLaunchKernelGGL(operand_image_kernel, dim3(nb * (nb + 1) / 2, 2), dim3(256), 0, st, S, nb, s, stored, front);
}

}  // namespace ewh_dev
