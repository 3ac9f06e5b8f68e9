// common_dense.hip — the correlated common process across pulsars: the M_g
// inverses (common_minv*), the assembly of the dense Sigma_c from the pulsars'
// kept blocks, its blocked factorisation (dchol_*: 64-column block rows,
// left-looking for large sample chunks, right-looking for a few proposals)
// and the global term (common_final); and the optimal statistic (os_*).
// Launch wrappers with the schedules: ewarp_launch.h.
#include "ewarp_launch.h"

namespace ewh_dev {

// M_g^-1 and log|M_g| by in-place Gauss-Jordan (SPD: no pivoting needed).
// grid (n_c, Bc), 256 threads, dynamic LDS (P (P+1) + 3 P) doubles.
// grid.x runs over the distinct M_g (sin / cos columns of one frequency share
// it): slot blockIdx.x stands for common column uniq[blockIdx.x].
// TERMS: the term form (CommonTerms; EWH_COMMON_MAX_TERMS more doubles of
// LDS): the weights w_t = coef_t(theta) phi_t(g; theta) are evaluated once
// per workgroup, one thread per term, and element (i, j) is formed as
// sum_t w_t mat_t[i][j]; the elimination is the same.  A sampled ORF can make
// M_g indefinite: a pivot <= 0 marks the sample (mlog = NaN -> lnL = -inf).
template <bool TERMS>
__global__ __launch_bounds__(256) void common_minv_kernel(const CommonPsr* __restrict__ cps, int P,
                                                          const double* __restrict__ orf,
                                                          const DSpec* __restrict__ cspec, int nc,
                                                          const int* __restrict__ uniq,
                                                          const double* __restrict__ theta, int ldth, int b0,
                                                          double* __restrict__ minv, double* __restrict__ mlog,
                                                          CommonTerms ct) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int LDP = P + 1;
  double* M = sm;
  double* colk = sm + P * LDP;
  double* rowk = colk + P;
  double* own = rowk + P;
  const int slot = blockIdx.x, g = uniq[slot], bl = blockIdx.y;
  const double* th = theta + (long long)(b0 + bl) * ldth;
  double pc = 0.0;
  if constexpr (!TERMS) pc = spec_phi(cspec[g], th);
  for (int a = threadIdx.x; a < P; a += 256) {
    const CommonPsr c = cps[a];
    const double v = col_phi(c.colptr, c.spec, c.gstart + g, th);
    own[a] = v;
  }
  if constexpr (TERMS) {
    double* wt = own + P;
    EWH_DCHECK(ct.n_term >= 1 && ct.n_term <= EWH_COMMON_MAX_TERMS, "common_minv: term count");
    EWH_DCHECK((int)(wt - sm) + ct.n_term <= ct.lds_doubles, "common_minv: term weights inside the dynamic LDS");
    if ((int)threadIdx.x < ct.n_term)
      wt[threadIdx.x] = pref_val(ct.coef[threadIdx.x], th) * spec_phi(ct.spec[ct.set[threadIdx.x] * nc + g], th);
    __syncthreads();
    for (int idx = threadIdx.x; idx < P * P; idx += 256) {
      const int i = idx / P, j = idx - i * P;
      double v = 0.0;
      for (int t = 0; t < ct.n_term; ++t) v += wt[t] * ct.mat[(long long)t * P * P + idx];
      M[i * LDP + j] = v + (i == j ? own[i] : 0.0);
    }
  } else {
    __syncthreads();
    for (int idx = threadIdx.x; idx < P * P; idx += 256) {
      const int i = idx / P, j = idx - i * P;
      M[i * LDP + j] = orf[idx] * pc + (i == j ? own[i] : 0.0);
    }
  }
  __syncthreads();
  double lsum = 0.0;
  bool ok = true;
  for (int k = 0; k < P; ++k) {
    const double piv = M[k * LDP + k];
    ok = ok && (piv > 0.0);
    lsum += log(piv);
    const double pinv = 1.0 / piv;
    for (int i = threadIdx.x; i < P; i += 256) {
      colk[i] = M[i * LDP + k];
      rowk[i] = M[k * LDP + i] * pinv;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < P * P; idx += 256) {
      const int i = idx / P, j = idx - i * P;
      double v;
      if (i == k) v = (j == k) ? pinv : rowk[j];
      else if (j == k) v = -colk[i] * pinv;
      else v = M[i * LDP + j] - colk[i] * rowk[j];
      M[i * LDP + j] = v;
    }
    __syncthreads();
  }
  double* out = minv + ((long long)bl * nc + slot) * P * P;
  for (int idx = threadIdx.x; idx < P * P; idx += 256) {
    const int i = idx / P, j = idx - i * P;
    out[idx] = M[i * LDP + j];
  }
  if (threadIdx.x == 0) mlog[(long long)bl * nc + slot] = ok ? lsum : __builtin_nan("");
}

// The same inverse for P <= MINV_PMAX with M held in registers: 8 waves, wave
// w owns rows i = w + 8 r (r < MINV_PMAX / 8), lane l columns j = l + 64 cc
// (cc < 2).  Per pivot k the owners of column k and row k publish them to LDS
// (double buffered by pivot parity: one barrier per pivot) and every thread
// updates its elements in place.  The pivot loop is unrolled over the row
// register r (k = 8 r + w_k), so row k's register and column k's half are
// compile-time indices (the round-3 form, 4 waves with a runtime register
// select and 338 registers at one wave per SIMD, took 6.7 ms per C5 batch of
// 512; the same arithmetic in the same order: bit-identical).
constexpr int MINV_PMAX = 128;
// sample chunks up to this size factor Sigma_c right-looking (corr_finish):
// C5 right- vs left-looking per chunk, ms (profiles/r04g/xover_B*.log):
// B = 4 1.67 / 3.21, 8 2.62 / 3.53, 12 3.65 / 4.01, 16 4.72 / 4.59
constexpr int CORR_RIGHT_LOOKING_MAX = 12;

// TERMS: the term form, as in common_minv_kernel<true> (the weights in LDS, one
// thread per term; each thread accumulates its elements term by term, one
// term's loads in flight at a time).
template <bool TERMS>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void common_minv_reg_kernel(const CommonPsr* __restrict__ cps, int P,
                                                              const double* __restrict__ orf,
                                                              const DSpec* __restrict__ cspec, int nc,
                                                              const int* __restrict__ uniq,
                                                              const double* __restrict__ theta, int ldth, int b0,
                                                              double* __restrict__ minv, double* __restrict__ mlog,
                                                              CommonTerms ct) {
  constexpr int NW = 8, RW = MINV_PMAX / NW;     // waves; rows per wave
  __shared__ double own[MINV_PMAX];
  __shared__ double colk[2][MINV_PMAX], rowk[2][MINV_PMAX];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int slot = blockIdx.x, g = uniq[slot], bl = blockIdx.y;
  const double* th = theta + (long long)(b0 + bl) * ldth;
  double pc = 0.0;
  if constexpr (!TERMS) pc = spec_phi(cspec[g], th);
  for (int a = tid; a < P; a += 64 * NW) {
    const CommonPsr c = cps[a];
    const double v = col_phi(c.colptr, c.spec, c.gstart + g, th);
    own[a] = v;
  }
  double m[RW][2];
  if constexpr (TERMS) {
    __shared__ double wt[EWH_COMMON_MAX_TERMS];
    EWH_DCHECK(ct.n_term >= 1 && ct.n_term <= EWH_COMMON_MAX_TERMS, "common_minv_reg: term count fits the LDS weights");
    EWH_DCHECK(P <= MINV_PMAX, "common_minv_reg: P <= MINV_PMAX");
    if (tid < ct.n_term) wt[tid] = pref_val(ct.coef[tid], th) * spec_phi(ct.spec[ct.set[tid] * nc + g], th);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RW; ++r) m[r][0] = m[r][1] = 0.0;
    // every load in bounds: columns past P read column 0, rows past P (a
    // wave-uniform condition) read this wave's first row.  A matrix is under
    // 128 KB: the element is a uniform row base + the lane's 32-bit byte
    // offset, which passes through an empty asm per term (hoisted out of the
    // term loop, the thirty-two offsets spilled at four waves per SIMD).
    const int wu = __builtin_amdgcn_readfirstlane(w);
    const int wc = wu < P ? wu : 0;
    const unsigned o0 = 8u * (unsigned)(lane < P ? lane : 0), o1 = 8u * (unsigned)(lane + 64 < P ? lane + 64 : 0);
#pragma unroll 1
    for (int t = 0; t < ct.n_term; ++t) {
      const double wv = wt[t];
      const char* B = (const char*)(ct.mat + (long long)t * P * P + wc * P);
      unsigned a0 = o0, a1 = o1;
      asm volatile("" : "+v"(a0), "+v"(a1));
#pragma unroll
      for (int r = 0; r < RW; ++r) {
        const char* Br = B + ((wu + NW * r < P) ? 8 * (NW * r * P) : 0);
        m[r][0] += wv * *(const double*)(Br + a0);
        m[r][1] += wv * *(const double*)(Br + a1);
      }
    }
#pragma unroll
    for (int r = 0; r < RW; ++r) {
      const int i = w + NW * r;
#pragma unroll
      for (int cc = 0; cc < 2; ++cc) {
        const int j = lane + 64 * cc;
        m[r][cc] = (i < P && j < P) ? m[r][cc] + (i == j ? own[i] : 0.0) : 0.0;
      }
    }
  } else {
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RW; ++r) {
      const int i = w + NW * r;
#pragma unroll
      for (int cc = 0; cc < 2; ++cc) {
        const int j = lane + 64 * cc;
        m[r][cc] = (i < P && j < P) ? orf[i * P + j] * pc + (i == j ? own[i] : 0.0) : 0.0;
      }
    }
  }
  LogAcc lacc;
  bool ok = true;
  static_for<0, RW>([&](auto R) {
    constexpr int r = decltype(R)::value;
    constexpr int cc = (NW * r) >= 64 ? 1 : 0;     // column k = NW r + wk lies in half cc
#pragma unroll 1
    for (int wk = 0; wk < NW; ++wk) {
      const int k = NW * r + wk;
      if (k >= P) break;
      const int buf = k & 1;
      const bool colown = lane == (k & 63);
      if (colown) {                                  // column k: one lane per wave
#pragma unroll
        for (int r2 = 0; r2 < RW; ++r2) colk[buf][w + NW * r2] = m[r2][cc];
      }
      if (w == wk) {                                 // row k: this wave, register r
        rowk[buf][lane] = m[r][0];
        rowk[buf][lane + 64] = m[r][1];
      }
      __syncthreads();
      const double piv = rowk[buf][k];
      ok = ok && (piv > 0.0);
      lacc.add(piv);
      const double pinv = 1.0 / piv;
      const double rj0 = rowk[buf][lane] * pinv, rj1 = rowk[buf][lane + 64] * pinv;
      double ci[RW];                                 // (all reads first: one LDS wait)
#pragma unroll
      for (int r2 = 0; r2 < RW; ++r2) ci[r2] = colk[buf][w + NW * r2];
#pragma unroll
      for (int r2 = 0; r2 < RW; ++r2) {
        const double u0 = fma(-ci[r2], rj0, m[r2][0]), u1 = fma(-ci[r2], rj1, m[r2][1]);
        const double cv = -ci[r2] * pinv;            // column k: -M[i][k] / piv (a select, no branch)
        m[r2][0] = (cc == 0 && colown) ? cv : u0;
        m[r2][1] = (cc == 1 && colown) ? cv : u1;
      }
      if (w == wk) {                                 // row k: M[k][j] / piv, the pivot 1 / piv
        m[r][0] = rj0;
        m[r][1] = rj1;
        if (colown) m[r][cc] = pinv;
      }
    }
  });
  double* out = minv + ((long long)bl * nc + slot) * P * P;
  int o0 = w * P + lane;              // (formed here: addresses carried from the loads spill)
  asm volatile("" : "+v"(o0));
#pragma unroll
  for (int r = 0; r < RW; ++r) {
    const int i = w + NW * r;
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
      const int j = lane + 64 * cc;
      if (i < P && j < P) out[o0 + NW * r * P + 64 * cc] = m[r][cc];
    }
  }
  if (tid == 0) mlog[(long long)bl * nc + slot] = ok ? lacc.value() : __builtin_nan("");
}

// Dense Sigma_c (Np x Np, row-major) of sample bl, one row per wave (four
// per workgroup): rows/cols (a, g) -> a nc + g; r at Np - 1; pad rows/cols
// identity.  keep: pulsar-major kept blocks, Bk samples per pulsar; this chunk
// starts at sample b0 (pulsar a's block of sample bl at keep[(a Bk + b0 + bl)
// KD^2]).  Column j -> (pulsar, common column) by a float reciprocal (exact:
// (j + 1/2) / nc is at least 1/(2 nc) from an integer) instead of an integer
// division per element.
__device__ __forceinline__ int div_nc(int j, float rnc) { return (int)(((float)j + 0.5f) * rnc); }

__global__ __launch_bounds__(256) void common_assemble_kernel(const double* __restrict__ keep, int KD, int P, int nc,
                                                              long long Bk, int b0,
                                                              const double* __restrict__ minv,
                                                              const int* __restrict__ rep, int Np,
                                                              double* __restrict__ mats, double* __restrict__ cldet,
                                                              double* __restrict__ cq, int* __restrict__ cfail) {
  typedef double d2 __attribute__((ext_vector_type(2)));
  const int i = 4 * blockIdx.x + (threadIdx.x >> 6), lane = threadIdx.x & 63, bl = blockIdx.y;
  if (blockIdx.x == 0 && threadIdx.x == 0) {   // the factorisation's per-sample accumulators (no memset launches)
    cldet[bl] = 0.0;
    cq[bl] = 0.0;
    cfail[bl] = 0;
  }
  if (i >= Np) return;
  const int N = P * nc;
  const float rnc = 1.0f / (float)nc;
  const long long ps = Bk * KD * KD;                                // pulsar stride
  double* row = mats + ((long long)bl * Np + i) * Np;
  const double* kb = keep + (long long)(b0 + bl) * KD * KD;
  const double* mb = minv + (long long)bl * nc * P * P;
  // only the upper tiles (64-column tiles at or right of the diagonal tile)
  // are ever read by the factorisation: the rest of the row is not written.
  // Two columns per lane, one 16-byte store (Np and the tile starts are
  // multiples of 64: every pair is aligned and inside the row).
  const int j0 = (i / DCB) * DCB;
  if (i < N) {
    const int a = div_nc(i, rnc), g = i - a * nc;
    const double* ka = kb + (long long)a * ps + g * KD;            // row g of pulsar a's kept square
    const double* mg = mb + (long long)rep[g] * P * P + (long long)a * P;  // row a of M_g^-1
    auto val = [&](int j) {
      double v = 0.0;
      if (j < N) {
        const int bb = div_nc(j, rnc), h = j - bb * nc;
        if (bb == a) v = ka[h];
        if (h == g) v += mg[bb];
      } else if (j == Np - 1) {
        v = ka[KD - 1];
      }
      return v;
    };
    for (int j = j0 + 2 * lane; j < Np; j += 128) {
      const d2 v = {val(j), val(j + 1)};
      __builtin_nontemporal_store(v, (d2*)(row + j));
    }
  } else if (i == Np - 1) {
    for (int j = j0 + lane; j < Np; j += 64) {
      double v = 0.0;
      if (j < N) {
        const int bb = div_nc(j, rnc), h = j - bb * nc;
        v = kb[(long long)bb * ps + (KD - 1) * KD + h];
      } else if (j == Np - 1) {
        for (int a = 0; a < P; ++a) v += kb[(long long)a * ps + KD * KD - 1];
      }
      __builtin_nontemporal_store(v, row + j);
    }
  } else {
    for (int j = j0 + 2 * lane; j < Np; j += 128) {
      const d2 v = {(j == i) ? 1.0 : 0.0, (j + 1 == i) ? 1.0 : 0.0};
      __builtin_nontemporal_store(v, (d2*)(row + j));
    }
  }
}

// Diagonal 64 x 64 block k of every sample: Cholesky A_kk = L L^T in LDS,
// log-det accumulation, W = L^-1 (forward substitution, one column per
// thread) to wbuf.  The last pivot of the last block is r: stored as q.
__global__ __launch_bounds__(256) void dchol_diag_kernel(double* __restrict__ mats, int Np, int k,
                                                         double* __restrict__ wbuf, double* __restrict__ ldet,
                                                         double* __restrict__ qout, int* __restrict__ fail) {
  __shared__ double L[DCB][DCB + 1];
  __shared__ double Wl[DCB][DCB + 1];
  __shared__ double qlast;
  const int bl = blockIdx.x, t = threadIdx.x;
  const double* A = mats + (long long)bl * Np * Np + (long long)(DCB * k) * Np + DCB * k;
  for (int idx = t; idx < DCB * DCB; idx += 256) L[idx / DCB][idx % DCB] = A[(long long)(idx / DCB) * Np + idx % DCB];
  __syncthreads();
  const bool last = (k == Np / DCB - 1);
  const int npiv = last ? DCB - 1 : DCB;
  double lsum = 0.0;
  bool ok = true;
  for (int j = 0; j < npiv; ++j) {
    const double piv = L[j][j];
    ok = ok && (piv > 0.0);
    lsum += log(piv);
    const double rd = 1.0 / sqrt(piv);
    __syncthreads();
    for (int i = j + 1 + t; i < DCB; i += 256) L[i][j] *= rd;
    if (t == 0) L[j][j] = sqrt(piv);
    __syncthreads();
    for (int idx = t; idx < (DCB - j - 1) * (DCB - j - 1); idx += 256) {
      const int i = j + 1 + idx / (DCB - j - 1), l = j + 1 + idx % (DCB - j - 1);
      if (l <= i) L[i][l] -= L[i][j] * L[l][j];
    }
    __syncthreads();
  }
  if (last) {
    if (t == 0) {
      qlast = L[DCB - 1][DCB - 1];          // q = rho - d'^T Sigma^-1 d'
      L[DCB - 1][DCB - 1] = 1.0;            // W's r row is unused
    }
    __syncthreads();
  }
  // W = L^-1 by forward elimination on [L | I], all threads: step k scales row
  // k of W by 1/L_kk, then eliminates column k from the rows below
  for (int idx = t; idx < DCB * DCB; idx += 256) Wl[idx / DCB][idx % DCB] = (idx / DCB == idx % DCB) ? 1.0 : 0.0;
  __syncthreads();
  for (int k2 = 0; k2 < DCB; ++k2) {
    const double rk = 1.0 / L[k2][k2];
    if (t <= k2) Wl[k2][t] *= rk;
    __syncthreads();
    for (int idx = t; idx < (DCB - 1 - k2) * (k2 + 1); idx += 256) {
      const int i = k2 + 1 + idx / (k2 + 1), cc = idx % (k2 + 1);
      Wl[i][cc] -= L[i][k2] * Wl[k2][cc];
    }
    __syncthreads();
  }
  double* W = wbuf + (long long)bl * DCB * DCB;
  for (int idx = t; idx < DCB * DCB; idx += 256) W[idx] = Wl[idx / DCB][idx % DCB];
  if (t == 0) {
    ldet[bl] += lsum;
    if (!ok) fail[bl] = 1;
    if (last) qout[bl] = qlast;
  }
}

// ---- register-resident diagonal block + panel (the default) -------------
// wbuf per sample (DW doubles): slots of 256 doubles in the MFMA C/D lane
// layout (lane l holds 4 consecutive doubles: register r <-> row (l>>4) + 4r,
// column l&15) -- E_s = L_ss^-T of the 16-row sub-blocks s = 0..3 (slots
// 0-3), their row scales D_s^-1/2 (4-7), the scaled factor blocks U_st,
// s < t (8-13: 01 02 03 12 13 23).
constexpr int DW_SLOTS = 14;
__host__ __device__ constexpr int dw_u(int s, int t) { return 8 + (s == 0 ? t - 1 : s == 1 ? t + 1 : 5); }

struct DiagHook : NoHook {
  double* W;
  int bb;
  __device__ __forceinline__ void on_e(const v4d& E) const { *(v4d*)(W + bb * 256) = E; }
  __device__ __forceinline__ void on_scale(int r, double rs) const { W[(4 + bb) * 256 + r] = rs; }
};

// One wave per sample: the 64 x 64 diagonal block k of Sigma_c factored in
// registers by the blocked LDL^T panel of chol_mfma_kernel (NB = 4, no
// residual column except in the LAST block, whose last pivot is
// q_c = rho - d'^T Sigma_c^-1 d'); log-det and positivity accumulated; E_s,
// D_s^-1/2 and U_st written for dchol_panel_reg_kernel.
// (body shared with dchol_update_diag_kernel: one wave, sample bl)
template <bool LAST>
__device__ __forceinline__ void diag_reg_body(double* __restrict__ mats, int Np, int k, double* __restrict__ wbuf,
                                              double* __restrict__ ldet, double* __restrict__ qout,
                                              int* __restrict__ fail, int bl, int lane) {
  const int q = lane >> 4, c = lane & 15;
  const double* A = mats + (long long)bl * Np * Np + (long long)(DCB * k) * Np + DCB * k;
  double* W = wbuf + (long long)bl * DW_SLOTS * 256 + lane * 4;
  constexpr auto id = [](int i, int j) { return i * 4 - i * (i - 1) / 2 + (j - i); };
  v4d U[10];
  static_for<0, 4>([&](auto I) {
    constexpr int i = decltype(I)::value;
    static_for<i, 4>([&](auto J) {
      constexpr int j = decltype(J)::value;
      static_for<0, 4>([&](auto R) {
        constexpr int r = decltype(R)::value;
        U[id(i, j)][r] = A[(long long)(16 * i + q + 4 * r) * Np + 16 * j + c];
      });
    });
  });
  LogAcc ld;
  bool ok = true;
  static_for<0, 4>([&](auto BBc) {
    constexpr int bb = decltype(BBc)::value;
    DiagHook hk;
    hk.W = W;
    hk.bb = bb;
    panel_ldl_row<4, PANEL_2L, LAST, false>(BBc, [&](auto JJ) -> v4d& { return U[id(bb, decltype(JJ)::value)]; }, q,
                                            c, ld, ok, hk);
    static_for<bb + 1, 4>([&](auto II) {
      constexpr int i = decltype(II)::value;
      static_for<i, 4>([&](auto JJ) {
        constexpr int j = decltype(JJ)::value;
        syrk_update(U[id(i, j)], U[id(bb, i)], U[id(bb, j)]);
      });
    });
  });
  if constexpr (!LAST) {
    static_for<0, 4>([&](auto SS) {
      constexpr int s0 = decltype(SS)::value;
      static_for<s0 + 1, 4>([&](auto TT) {
        constexpr int t0 = decltype(TT)::value;
        *(v4d*)(W + dw_u(s0, t0) * 256) = U[id(s0, t0)];
      });
    });
  }
  const double ldv = wave_sum(ld.value());
  const bool ok_all = __all(ok);
  double qv = 0.0;
  if constexpr (LAST) qv = readlane_d(U[id(3, 3)][3], 63);
  if (lane == 0) {
    ldet[bl] += ldv;
    if (!ok_all) fail[bl] = 1;
    if (LAST) qout[bl] = qv;
  }
}

template <bool LAST>
__global__ __launch_bounds__(64) void dchol_diag_reg_kernel(double* __restrict__ mats, int Np, int k,
                                                            double* __restrict__ wbuf, double* __restrict__ ldet,
                                                            double* __restrict__ qout, int* __restrict__ fail) {
  diag_reg_body<LAST>(mats, Np, k, wbuf, ldet, qout, fail, blockIdx.x, threadIdx.x);
}

// U_kj = L_kk^-1 A_kj (scaled) for the tiles j > k: one wave per (16-column
// strip, tile, sample), the strip's four 16 x 16 blocks in registers, the
// block forward substitution by fp64 MFMA with the operands of wbuf.
__global__ __launch_bounds__(64) void dchol_panel_reg_kernel(double* __restrict__ mats, int Np, int k,
                                                             const double* __restrict__ wbuf) {
  const int strip = blockIdx.x & 3, jt = blockIdx.x >> 2, bl = blockIdx.y;
  const int lane = threadIdx.x, q = lane >> 4, c = lane & 15;
  const int j = k + 1 + jt;
  double* T = mats + (long long)bl * Np * Np + (long long)(DCB * k) * Np + DCB * j + 16 * strip;
  const double* W = wbuf + (long long)bl * DW_SLOTS * 256 + lane * 4;
  v4d a[4];
  static_for<0, 4>([&](auto SS) {
    constexpr int s0 = decltype(SS)::value;
    static_for<0, 4>([&](auto R) {
      constexpr int r = decltype(R)::value;
      a[s0][r] = T[(long long)(16 * s0 + q + 4 * r) * Np + c];
    });
  });
  static_for<0, 4>([&](auto SS) {
    constexpr int s0 = decltype(SS)::value;
    static_for<0, s0>([&](auto TT) {
      constexpr int t0 = decltype(TT)::value;
      syrk_update(a[s0], *(const v4d*)(W + dw_u(t0, s0) * 256), a[t0]);
    });
    const v4d E = *(const v4d*)(W + s0 * 256);
    const v4d rs = *(const v4d*)(W + (4 + s0) * 256);
    v4d acc = {0.0, 0.0, 0.0, 0.0};
    static_for<0, 4>([&](auto S2) {
      constexpr int sk = decltype(S2)::value;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(E[sk], a[s0][sk], acc, 0, 0, 0);
    });
    static_for<0, 4>([&](auto R) {
      constexpr int r = decltype(R)::value;
      a[s0][r] = acc[r] * rs[r];
    });
  });
  static_for<0, 4>([&](auto SS) {
    constexpr int s0 = decltype(SS)::value;
    static_for<0, 4>([&](auto R) {
      constexpr int r = decltype(R)::value;
      T[(long long)(16 * s0 + q + 4 * r) * Np + c] = a[s0][r];
    });
  });
}

// stage a 64 x 64 tile (row stride ld, 16-byte aligned rows) into LDS
// [64][64 + 1] with 256 threads: all eight 16-byte loads of a thread issued
// before its first LDS write (a rolled loop waited on each load in turn --
// 16 dependent global round trips per tile, most of the right-looking update
// kernel's time at B = 1)
typedef double v2d __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void stage64(double (*dst)[DCB + 1], const double* src, long long ld) {
  constexpr int NIT = DCB * DCB / 2 / 256;
  v2d v[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int p = threadIdx.x + 256 * it;
    v[it] = *(const v2d*)(src + (long long)(p >> 5) * ld + 2 * (p & 31));
  }
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int p = threadIdx.x + 256 * it;
    dst[p >> 5][2 * (p & 31)] = v[it][0];
    dst[p >> 5][2 * (p & 31) + 1] = v[it][1];
  }
}

// Panel: U_kj = W A_kj for the blocks j > k of every sample (in place).
// grid (nb - k - 1, Bc); 4 waves, wave w -> rows 16w..16w+15, 4 column blocks.
__global__ __launch_bounds__(256) void dchol_panel_kernel(double* __restrict__ mats, int Np, int k,
                                                          const double* __restrict__ wbuf) {
  __shared__ double Ws[DCB][DCB + 1];
  __shared__ double As[DCB][DCB + 1];
  const int j = k + 1 + blockIdx.x, bl = blockIdx.y;
  double* Akj = mats + (long long)bl * Np * Np + (long long)(DCB * k) * Np + DCB * j;
  stage64(Ws, wbuf + (long long)bl * DCB * DCB, DCB);
  stage64(As, Akj, Np);
  __syncthreads();
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, q = lane >> 4, c = lane & 15;
  v4d acc[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
  for (int ts = 0; ts < DCB / 4; ++ts) {
    const double a = Ws[16 * w + c][4 * ts + q];
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) acc[jb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, As[4 * ts + q][16 * jb + c], acc[jb], 0, 0, 0);
  }
#pragma unroll
  for (int jb = 0; jb < 4; ++jb)
#pragma unroll
    for (int r = 0; r < 4; ++r) Akj[(long long)(16 * w + q + 4 * r) * Np + 16 * jb + c] = acc[jb][r];
}

// Trailing update A_ij -= U_ki^T U_kj, k < i <= j, every sample.
// grid (T(k), Bc) with T(k) = m (m + 1) / 2, m = nb - k - 1.
__device__ __forceinline__ void update_tile_body(double* __restrict__ mats, int Np, int k) {
  __shared__ double Ui[DCB][DCB + 1];
  __shared__ double Uj[DCB][DCB + 1];
  const int nb = Np / DCB, m = nb - k - 1;
  int tix = blockIdx.x, ii = 0;
  while (tix >= m - ii) { tix -= m - ii; ++ii; }
  const int i = k + 1 + ii, j = i + tix;
  const int bl = blockIdx.y;
  double* base = mats + (long long)bl * Np * Np;
  stage64(Ui, base + (long long)(DCB * k) * Np + DCB * i, Np);
  stage64(Uj, base + (long long)(DCB * k) * Np + DCB * j, Np);
  double* Aij = base + (long long)(DCB * i) * Np + DCB * j;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, q = lane >> 4, c = lane & 15;
  v4d acc[4];
#pragma unroll
  for (int jb = 0; jb < 4; ++jb)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[jb][r] = Aij[(long long)(16 * w + q + 4 * r) * Np + 16 * jb + c];
  __syncthreads();
#pragma unroll
  for (int ts = 0; ts < DCB / 4; ++ts) {
    const double a = -Ui[4 * ts + q][16 * w + c];
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) acc[jb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Uj[4 * ts + q][16 * jb + c], acc[jb], 0, 0, 0);
  }
#pragma unroll
  for (int jb = 0; jb < 4; ++jb)
#pragma unroll
    for (int r = 0; r < 4; ++r) Aij[(long long)(16 * w + q + 4 * r) * Np + 16 * jb + c] = acc[jb][r];
}

__global__ __launch_bounds__(256) void dchol_update_kernel(double* __restrict__ mats, int Np, int k) {
  update_tile_body(mats, Np, k);
}

// The trailing update of step k with the diagonal block k + 1 factored in
// the same launch: workgroup 0 of each sample owns tile (k + 1, k + 1);
// after storing it, its first wave runs the diagonal factorisation of
// dchol_diag_reg_kernel on it (same values, same code: bit-identical) while
// the other workgroups are still updating their tiles -- one launch and one
// dependent gap fewer per block row of the one-proposal schedule.  Nothing
// else reads the block-(k + 1) operands in wbuf before the next panel.
template <bool LAST>
__global__ __launch_bounds__(256) void dchol_update_diag_kernel(double* __restrict__ mats, int Np, int k,
                                                                double* __restrict__ wbuf, double* __restrict__ ldet,
                                                                double* __restrict__ qout, int* __restrict__ fail) {
  update_tile_body(mats, Np, k);
  if (blockIdx.x != 0) return;
  __syncthreads();   // the tile's rows stored by every wave of the workgroup
  if (threadIdx.x < 64) diag_reg_body<LAST>(mats, Np, k + 1, wbuf, ldet, qout, fail, blockIdx.y, threadIdx.x);
}

// Row-oriented (left-looking) update, the default: before block row i is
// factored, A_ij -= sum_{p < i} U_pi^T U_pj for every j >= i.  One workgroup
// per (j, sample) keeps its 64 x 64 tile in registers across all p (K = 64 i),
// staging U_pi / U_pj through LDS with the next pair prefetched into
// registers: each tile is read and written once per factorisation instead of
// once per panel step (the right-looking dchol_update_kernel above).
__global__ __launch_bounds__(256) void dchol_rowupdate_kernel(double* __restrict__ mats, int Np, int i) {
  __shared__ double Ui[DCB][DCB + 1];
  __shared__ double Uj[DCB][DCB + 1];
  const int j = i + blockIdx.x, bl = blockIdx.y, t = threadIdx.x;
  double* base = mats + (long long)bl * Np * Np;
  double* Aij = base + (long long)(DCB * i) * Np + DCB * j;
  const int w = t >> 6, lane = t & 63, q = lane >> 4, c = lane & 15;
  v4d acc[4];
#pragma unroll
  for (int jb = 0; jb < 4; ++jb)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[jb][r] = Aij[(long long)(16 * w + q + 4 * r) * Np + 16 * jb + c];
  double pf[32];
  auto gload = [&](int p) {
    const double* rp = base + (long long)(DCB * p) * Np;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int idx = t + 256 * r, row = idx >> 6, col = idx & 63;
      pf[r] = rp[(long long)row * Np + DCB * i + col];
      pf[16 + r] = rp[(long long)row * Np + DCB * j + col];
    }
  };
  gload(0);
  for (int p = 0; p < i; ++p) {
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int idx = t + 256 * r, row = idx >> 6, col = idx & 63;
      Ui[row][col] = pf[r];
      Uj[row][col] = pf[16 + r];
    }
    __syncthreads();
    if (p + 1 < i) gload(p + 1);
#pragma unroll
    for (int ts = 0; ts < DCB / 4; ++ts) {
      const double a = -Ui[4 * ts + q][16 * w + c];
#pragma unroll
      for (int jb = 0; jb < 4; ++jb)
        acc[jb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Uj[4 * ts + q][16 * jb + c], acc[jb], 0, 0, 0);
    }
  }
#pragma unroll
  for (int jb = 0; jb < 4; ++jb)
#pragma unroll
    for (int r = 0; r < 4; ++r) Aij[(long long)(16 * w + q + 4 * r) * Np + 16 * jb + c] = acc[jb][r];
}

// The same row update with more waves per CU (the default): only U_pj is
// staged through LDS (one 64 x 64 tile, 33 KB: four workgroups fit a CU
// instead of two); each wave reads its A operand -- the 64 x 16 column slab
// of U_pi it multiplies, 16 doubles per lane -- straight from global memory
// into registers, prefetched one step ahead together with the U_pj tile; the
// minus sign is the MFMA neg modifier.  Same sums in the same order as
// dchol_rowupdate_kernel: bit-identical.  p0 > 0: only the rows p0 <= p < i
// (the rest already applied by dchol_rowpair_kernel).
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4)))
void dchol_rowupdate2_kernel(double* __restrict__ mats, int Np, int i, int p0) {
  __shared__ double Uj[DCB][DCB + 1];
  const int j = i + blockIdx.x, bl = blockIdx.y, t = threadIdx.x;
  const int w = t >> 6, lane = t & 63, q = lane >> 4, c = lane & 15;
  // accesses as the sample's uniform base + 32-bit byte offsets (see
  // dchol_rowpair_kernel)
  char* cb = (char*)(mats + (long long)bl * Np * Np);
  auto at = [&](unsigned off) -> double& { return *(double*)(cb + off); };
  const unsigned rowb = 8u * (unsigned)Np;
  const unsigned toff = (unsigned)(DCB * i + 16 * w + q) * rowb + 8u * (unsigned)(DCB * j + c);
  v4d acc[4];
#pragma unroll
  for (int jb = 0; jb < 4; ++jb)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[jb][r] = at(toff + (unsigned)(4 * r) * rowb + 8u * (unsigned)(16 * jb));
  // A slab of U_pi (column block 16w..16w+15, all 64 rows) in registers, U_pj
  // staged through LDS (prefetched one step ahead into registers)
  const unsigned aoff = (unsigned)q * rowb + 8u * (unsigned)(DCB * i + 16 * w + c);
  const unsigned boff = (unsigned)(t >> 6) * rowb + 8u * (unsigned)(DCB * j + (t & 63));
  double pb[16];
  auto bload = [&](int p) {
    unsigned o = boff + (unsigned)(DCB * p) * rowb;
    asm volatile("" : "+v"(o));
#pragma unroll
    for (int r = 0; r < 16; ++r) pb[r] = at(o + (unsigned)(4 * r) * rowb);
  };
  // the A slab of the next step is loaded into the registers of this one as
  // they die (a[0..7] after the MFMAs of ts = 7, a[8..15] after ts = 15), as
  // in dchol_rowpair_kernel<PIPE>; loads unconditional (the last step reloads
  // its own rows) so the waitcnt pass sees one path
  if (p0 < i) {
    double a[16];
    auto ahalf = [&](int p, int h) {
      unsigned o = aoff + (unsigned)(DCB * p) * rowb;
      asm volatile("" : "+v"(o));
#pragma unroll
      for (int ts = 8 * h; ts < 8 * h + 8; ++ts) a[ts] = at(o + (unsigned)(4 * ts) * rowb);
    };
    bload(p0);
    ahalf(p0, 0);
    ahalf(p0, 1);
    for (int p = p0; p < i; ++p) {
      const int pn = min(p + 1, i - 1);
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 16; ++r) Uj[(t >> 6) + 4 * r][t & 63] = pb[r];
      __syncthreads();
      bload(pn);
      static_for<0, 2>([&](auto H) {
        constexpr int h = decltype(H)::value;
#pragma unroll
        for (int ts = 8 * h; ts < 8 * h + 8; ++ts) {
#pragma unroll
          for (int jb = 0; jb < 4; ++jb)
            acc[jb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ts], Uj[4 * ts + q][16 * jb + c], acc[jb], 0, 0, 1);
        }
        asm volatile("" ::: "memory");
        ahalf(pn, h);
        asm volatile("" ::: "memory");
      });
    }
  }
  unsigned toff2 = toff;
  asm volatile("" : "+v"(toff2));
#pragma unroll
  for (int jb = 0; jb < 4; ++jb)
#pragma unroll
    for (int r = 0; r < 4; ++r) at(toff2 + (unsigned)(4 * r) * rowb + 8u * (unsigned)(16 * jb)) = acc[jb][r];
}

// Row update + panel in one pass for the tiles j > k of block row k (after
// dchol_diag_reg_kernel has factored tile (k, k)): wave w owns the 16-column
// strip w of tile (k, j) over all 64 rows, so after accumulating
// A_kj - sum_p U_pk^T U_pj it applies the block forward substitution of
// dchol_panel_reg_kernel to its own registers and writes U_kj once (no
// round trip of the updated tile through HBM, one launch less per block row).
// U_pk is staged through LDS (shared by the four waves), each wave's U_pj
// slab comes from global memory into registers.  Same sums, same order as
// dchol_rowupdate2_kernel + dchol_panel_reg_kernel: bit-identical.
// TPW = 2 (the default since round 4): two tiles (k, j), (k, j + 1) per
// 8-wave workgroup sharing one LDS copy of U_pk -- per p the workgroup reads
// 96 KB (U_pk + two U_pj) for two tiles instead of 64 KB for one; C5 at
// B = 512: 91.3 vs 95.8 ms per batch, bit-identical (scripts/c5_ab.py).
// TPW = 1: the round-3 form (dev kernel mode 28).  p0 > 0: only the rows
// p0 <= p < k (dchol_rowpair_kernel applied the others; p0 = k: the panel
// alone).
template <int TPW>
__global__ __launch_bounds__(256 * TPW) __attribute__((amdgpu_waves_per_eu(TPW == 1 ? 3 : 4, TPW == 1 ? 3 : 4)))
void dchol_rowpanel_kernel(double* __restrict__ mats, int Np, int k, int p0, const double* __restrict__ wbuf) {
  constexpr int NT = 256 * TPW, RW = 64 / (NT / 64);   // threads; U_pk rows staged per thread
  __shared__ double Uk[DCB][DCB + 1];
  const int t = threadIdx.x, wave = t >> 6, tile = wave >> 2, w = wave & 3;
  const int j = k + 1 + TPW * blockIdx.x + tile, bl = blockIdx.y;
  const bool live = j < Np / DCB;                  // (the last workgroup of an odd row: one tile)
  double* base = mats + (long long)bl * Np * Np;
  double* Akj = base + (long long)(DCB * k) * Np + DCB * (live ? j : k + 1);
  const int lane = t & 63, q = lane >> 4, c = lane & 15;
  v4d acc[4];
#pragma unroll
  for (int s0 = 0; s0 < 4; ++s0)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[s0][r] = live ? Akj[(long long)(16 * s0 + q + 4 * r) * Np + 16 * w + c] : 0.0;
  const double* bcol = base + DCB * (live ? j : k + 1) + 16 * w + c + (long long)q * Np;
  const double* acol = base + DCB * k + (t & 63) + (long long)(t >> 6) * Np;
  double pa[RW];
  auto aload = [&](int p) {
    const double* rp = acol + (long long)(DCB * p) * Np;
#pragma unroll
    for (int r = 0; r < RW; ++r) pa[r] = rp[(long long)((NT / 64) * r) * Np];
  };
  if (p0 < k) aload(p0);
  for (int p = p0; p < k; ++p) {
    double b[16];
    const double* bp = bcol + (long long)(DCB * p) * Np;
#pragma unroll
    for (int ts = 0; ts < 16; ++ts) b[ts] = bp[(long long)(4 * ts) * Np];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RW; ++r) Uk[(t >> 6) + (NT / 64) * r][t & 63] = pa[r];
    __syncthreads();
    // (measured round 4: forcing a true one-step-ahead prefetch here -- an
    // unconditional load pinned by an empty asm -- ran C5 at 89.9 instead of
    // 83.6 ms; as written the compiler issues it with the next step's loads)
    if (p + 1 < k) aload(p + 1);
#pragma unroll
    for (int ts = 0; ts < DCB / 4; ++ts) {
#pragma unroll
      for (int s0 = 0; s0 < 4; ++s0)
        acc[s0] = __builtin_amdgcn_mfma_f64_16x16x4f64(Uk[4 * ts + q][16 * s0 + c], b[ts], acc[s0], 0, 0, 1);
    }
  }
  if (!live) return;
  // the panel: U_kj = L_kk^-1 A_kj on this strip (dchol_panel_reg_kernel)
  const double* W = wbuf + (long long)bl * DW_SLOTS * 256 + lane * 4;
  static_for<0, 4>([&](auto SS) {
    constexpr int s0 = decltype(SS)::value;
    static_for<0, s0>([&](auto TT) {
      constexpr int t0 = decltype(TT)::value;
      syrk_update(acc[s0], *(const v4d*)(W + dw_u(t0, s0) * 256), acc[t0]);
    });
    const v4d E = *(const v4d*)(W + s0 * 256);
    const v4d rs = *(const v4d*)(W + (4 + s0) * 256);
    v4d v = {0.0, 0.0, 0.0, 0.0};
    static_for<0, 4>([&](auto S2) {
      constexpr int sk = decltype(S2)::value;
      v = __builtin_amdgcn_mfma_f64_16x16x4f64(E[sk], acc[s0][sk], v, 0, 0, 0);
    });
    static_for<0, 4>([&](auto R) {
      constexpr int r = decltype(R)::value;
      acc[s0][r] = v[r] * rs[r];
    });
  });
#pragma unroll
  for (int s0 = 0; s0 < 4; ++s0)
#pragma unroll
    for (int r = 0; r < 4; ++r) Akj[(long long)(16 * s0 + q + 4 * r) * Np + 16 * w + c] = acc[s0][r];
}

// The row update of two block rows at once -- a 128-row block row for the
// update, whose cost is streaming the finished rows U_pj from HBM: tiles
// (k, j) and (k + 1, j) for j > k take the updates of every row p < k, the
// U_pj tile streamed once for both (twice the MFMA work per HBM byte of
// dchol_rowpanel_kernel), U_pk and U_p,k+1 (adjacent; shared by every
// workgroup of the sample, from L2) staged through LDS.  8 waves per column
// tile j: wave w updates strip w & 3 (16 columns, all 64 rows) of tile
// (k + (w >> 2), j); the two waves of a strip read the same U_pj slab (the
// second read from L1 / L2).  Launched after dchol_diag_reg_kernel has
// factored tile (k, k): the row-k waves finish with the panel (U_kj written
// once, as dchol_rowpanel_kernel), the row-(k + 1) accumulators go back to
// HBM and row k + 1 takes its last update p = k in dchol_rowpanel_kernel
// (p0 = k) -- per tile the same MFMAs on the same operands in the same order
// as the one-row schedule, the accumulator stored and reloaded exactly in
// between: bit-identical (dev kernel mode 31 runs the one-row schedule).
// PIPE (the default): the next step's U_pj slab is loaded into the registers
// of the current one as they die -- b[0..7] after the MFMAs of ts = 7,
// b[8..15] after ts = 15 -- so no step starts on a cold load and no register
// is added (the loads pinned in place by empty asm statements).  C5 at
// B = 512: 80.7 vs 83.6 ms (!PIPE, the slab loaded at the top of its step:
// dev kernel mode 32), bit-identical.
// (Measured and dropped: one more workgroup per sample pre-updating the next
// pair's diagonal tile over p < k, which cut the diagonal-tile row update
// from 69 to 17 us per launch but lengthened the pair launches by more --
// m + 1 instead of m workgroups per sample, and late pairs have m ~ 1-3:
// 81.3 vs 79.7 ms per C5 batch.)
template <bool PIPE>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4)))
void dchol_rowpair_kernel(double* __restrict__ mats, int Np, int k, const double* __restrict__ wbuf) {
  __shared__ double Uk[2][DCB][DCB + 1];
  const int t = threadIdx.x, wave = t >> 6, rt = wave >> 2, w = wave & 3;
  const int j = k + 1 + blockIdx.x, bl = blockIdx.y;
  const int lane = t & 63, q = lane >> 4, c = lane & 15;
  // every access as the sample's (uniform) base + a 32-bit byte offset (a
  // sample's matrix is < 4 GB); the offsets pass through an empty asm where
  // the compiler would otherwise keep one register per load live across the
  // loop (which spills)
  char* cb = (char*)(mats + (long long)bl * Np * Np);
  auto at = [&](unsigned off) -> double& { return *(double*)(cb + off); };
  const unsigned rowb = 8u * (unsigned)Np;                       // bytes per row
  // this lane's element (q, c) of strip w of tile (k + rt, j)
  const unsigned toff = (unsigned)(DCB * (k + rt) + q) * rowb + 8u * (unsigned)(DCB * j + 16 * w + c);
  v4d acc[4];
#pragma unroll
  for (int s0 = 0; s0 < 4; ++s0)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[s0][r] = at(toff + (unsigned)(16 * s0 + 4 * r) * rowb);
  const unsigned boff = (unsigned)q * rowb + 8u * (unsigned)(DCB * j + 16 * w + c);
  // staging: thread t holds column (t & 127) of the 128-column pair, rows
  // (t >> 7) + 4 r
  const int scol = t & 127, srow = t >> 7, stile = scol >> 6, scc = scol & 63;
  const unsigned aoff = 8u * (unsigned)(DCB * k + scol) + (unsigned)srow * rowb;
  double pa[16];
  auto aload = [&](int p) {
    unsigned o = aoff + (unsigned)(DCB * p) * rowb;
    asm volatile("" : "+v"(o));
#pragma unroll
    for (int r = 0; r < 16; ++r) pa[r] = at(o + (unsigned)(4 * r) * rowb);
  };
  if constexpr (!PIPE) {
    if (k > 0) aload(0);
    for (int p = 0; p < k; ++p) {
      double b[16];
      unsigned o = boff + (unsigned)(DCB * p) * rowb;
      asm volatile("" : "+v"(o));
#pragma unroll
      for (int ts = 0; ts < 16; ++ts) b[ts] = at(o + (unsigned)(4 * ts) * rowb);
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 16; ++r) Uk[stile][srow + 4 * r][scc] = pa[r];
      __syncthreads();
      // (measured round 4: forcing a true one-step-ahead prefetch here -- an
      // unconditional load pinned by an empty asm -- ran C5 at 89.9 instead of
      // 83.6 ms; as written the compiler issues it with the next step's loads)
      if (p + 1 < k) aload(p + 1);
#pragma unroll
      for (int ts = 0; ts < DCB / 4; ++ts) {
#pragma unroll
        for (int s0 = 0; s0 < 4; ++s0)
          acc[s0] = __builtin_amdgcn_mfma_f64_16x16x4f64(Uk[rt][4 * ts + q][16 * s0 + c], b[ts], acc[s0], 0, 0, 1);
      }
    }
  } else if (k > 0) {
    double b[16];
    auto bhalf = [&](int p, int h) {           // b[8 h .. 8 h + 7] of step p
      unsigned o = boff + (unsigned)(DCB * p) * rowb;
      asm volatile("" : "+v"(o));
#pragma unroll
      for (int ts = 8 * h; ts < 8 * h + 8; ++ts) b[ts] = at(o + (unsigned)(4 * ts) * rowb);
    };
    aload(0);
    bhalf(0, 0);
    bhalf(0, 1);
    for (int p = 0; p < k; ++p) {
      const int pn = min(p + 1, k - 1);          // (unconditional loads: one waitcnt path)
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 16; ++r) Uk[stile][srow + 4 * r][scc] = pa[r];
      __syncthreads();
      aload(pn);
      static_for<0, 2>([&](auto H) {
        constexpr int h = decltype(H)::value;
#pragma unroll
        for (int ts = 8 * h; ts < 8 * h + 8; ++ts) {
#pragma unroll
          for (int s0 = 0; s0 < 4; ++s0)
            acc[s0] = __builtin_amdgcn_mfma_f64_16x16x4f64(Uk[rt][4 * ts + q][16 * s0 + c], b[ts], acc[s0], 0, 0, 1);
        }
        asm volatile("" ::: "memory");
        bhalf(pn, h);
        asm volatile("" ::: "memory");
      });
    }
  }
  if (rt == 0) {
    // row k is complete: its panel U_kj = L_kk^-1 A_kj on this strip, with the
    // operands dchol_diag_reg_kernel left in wbuf (as dchol_rowpanel_kernel)
    const double* W = wbuf + (long long)bl * DW_SLOTS * 256 + lane * 4;
    static_for<0, 4>([&](auto SS) {
      constexpr int s0 = decltype(SS)::value;
      static_for<0, s0>([&](auto TT) {
        constexpr int t0 = decltype(TT)::value;
        syrk_update(acc[s0], *(const v4d*)(W + dw_u(t0, s0) * 256), acc[t0]);
      });
      const v4d E = *(const v4d*)(W + s0 * 256);
      const v4d rs = *(const v4d*)(W + (4 + s0) * 256);
      v4d v = {0.0, 0.0, 0.0, 0.0};
      static_for<0, 4>([&](auto S2) {
        constexpr int sk = decltype(S2)::value;
        v = __builtin_amdgcn_mfma_f64_16x16x4f64(E[sk], acc[s0][sk], v, 0, 0, 0);
      });
      static_for<0, 4>([&](auto R) {
        constexpr int r = decltype(R)::value;
        acc[s0][r] = v[r] * rs[r];
      });
    });
  }
  unsigned toff2 = toff;
  asm volatile("" : "+v"(toff2));
#pragma unroll
  for (int s0 = 0; s0 < 4; ++s0)
#pragma unroll
    for (int r = 0; r < 4; ++r) at(toff2 + (unsigned)(16 * s0 + 4 * r) * rowb) = acc[s0][r];
}

// ----------------------------------------------------------------------------
// optimal statistic (EWH_COMMON_OPTSTAT handles; ewh_optstat)
// From pulsar a's kept block K (its common columns G after eliminating the
// rest, phi^-1 on every column): (Sigma^-1)_GG = K_GG^-1 and
// (Sigma^-1 d)_G = K_GG^-1 K_Gr, so with D = diag(phi^-1)_G
//   X = D K_GG^-1 K_Gr,  Z = D - D K_GG^-1 D
// (F^T P^-1 r and F^T P^-1 F by Woodbury: TNT = Sigma - Phi^-1).  Stored
// pre-scaled by phihat^1/2: x^ = phihat^1/2 X, W = phihat^1/2 Z phihat^1/2, so
// that per pair top = x^_a . x^_b and bot = tr(Z_a phihat Z_b phihat) = <W_a, W_b>.
// ----------------------------------------------------------------------------
__global__ __launch_bounds__(64) void os_xz_kernel(const double* __restrict__ keep, int KD, int P, int nc,
                                                   const CommonPsr* __restrict__ cps,
                                                   const double* __restrict__ theta, int ldth,
                                                   const double* __restrict__ phihat, double* __restrict__ xh,
                                                   double* __restrict__ wh) {
  __shared__ double M[32][33];
  __shared__ double colk[32], rowk[32], dv[32], kr[32], sq[32];
  const int a = blockIdx.x, bl = blockIdx.y, t = threadIdx.x;
  EWH_DCHECK(nc >= 1 && nc <= 31 && nc < KD, "os_xz: nc within the static LDS arrays");
  const double* K = keep + ((long long)a * gridDim.y + bl) * KD * KD;     // pulsar-major, B = gridDim.y
  const double* th = theta + (long long)bl * ldth;
  for (int idx = t; idx < nc * nc; idx += 64) M[idx / nc][idx % nc] = K[(idx / nc) * KD + idx % nc];
  if (t < nc) {
    kr[t] = K[t * KD + KD - 1];
    const CommonPsr c = cps[a];
    const double ph = col_phi(c.colptr, c.spec, c.gstart + t, th);
    dv[t] = 1.0 / ph;
    sq[t] = sqrt(phihat[(long long)bl * nc + t]);
  }
  __syncthreads();
  for (int k = 0; k < nc; ++k) {        // Gauss-Jordan inverse of K_GG (SPD)
    const double pinv = 1.0 / M[k][k];
    if (t < nc) {
      colk[t] = M[t][k];
      rowk[t] = M[k][t] * pinv;
    }
    __syncthreads();
    for (int idx = t; idx < nc * nc; idx += 64) {
      const int i = idx / nc, j = idx % nc;
      double v;
      if (i == k) v = (j == k) ? pinv : rowk[j];
      else if (j == k) v = -colk[i] * pinv;
      else v = M[i][j] - colk[i] * rowk[j];
      M[i][j] = v;
    }
    __syncthreads();
  }
  double* xo = xh + ((long long)bl * P + a) * nc;
  double* wo = wh + ((long long)bl * P + a) * nc * nc;
  if (t < nc) {
    double v = 0.0;
    for (int h = 0; h < nc; ++h) v += M[t][h] * kr[h];
    xo[t] = sq[t] * dv[t] * v;
  }
  for (int idx = t; idx < nc * nc; idx += 64) {
    const int g = idx / nc, h = idx % nc;
    const double z = (g == h ? dv[g] : 0.0) - dv[g] * M[g][h] * dv[h];
    wo[idx] = sq[g] * z * sq[h];
  }
}

// The same for nc up to EWH_OS_MAX_COMMON_COLS (63: 31 frequencies): K_GG in
// dynamic LDS with an odd row stride (the column read M[t][k] of a pivot step
// then walks the banks), four waves over the nc^2 entries of each Gauss-Jordan
// step (a 63^2 block is 16 passes of 256 threads instead of 62 of one wave).
// Per element the same operations in the same order as os_xz_kernel; that
// kernel stays the route for nc <= 31, so those results do not move.
constexpr int OS_WIDE_THREADS = 256;
__host__ __device__ inline int os_wide_ldm(int nc) { return nc | 1; }
__host__ __device__ inline size_t os_wide_lds_doubles(int nc) { return (size_t)nc * os_wide_ldm(nc) + 5 * (size_t)nc; }

__global__ __launch_bounds__(OS_WIDE_THREADS) void os_xz_wide_kernel(const double* __restrict__ keep, int KD, int P,
                                                                     int nc, const CommonPsr* __restrict__ cps,
                                                                     const double* __restrict__ theta, int ldth,
                                                                     const double* __restrict__ phihat,
                                                                     double* __restrict__ xh, double* __restrict__ wh,
                                                                     int lds_doubles) {
  extern __shared__ __attribute__((aligned(16))) double os_sm[];
  const int LDM = os_wide_ldm(nc);
  double* M = os_sm;
  double* colk = M + nc * LDM;
  double* rowk = colk + nc;
  double* dv = rowk + nc;
  double* kr = dv + nc;
  double* sq = kr + nc;
  const int a = blockIdx.x, bl = blockIdx.y, t = threadIdx.x;
  // (debug build: the matrix and its five side vectors fit the dynamic LDS
  // the launch asked for, the common columns and r fit the kept square)
  EWH_DCHECK(nc >= 1 && nc <= EWH_OS_MAX_COMMON_COLS && LDM >= nc, "os_xz_wide: nc within the OS cap");
  EWH_DCHECK((sq + nc) - os_sm <= lds_doubles, "os_xz_wide: LDS extents");
  EWH_DCHECK(nc < KD && a < P, "os_xz_wide: common columns inside the kept block");
  const double* K = keep + ((long long)a * gridDim.y + bl) * KD * KD;     // pulsar-major, B = gridDim.y
  const double* th = theta + (long long)bl * ldth;
  for (int idx = t; idx < nc * nc; idx += OS_WIDE_THREADS) {
    const int i = idx / nc, j = idx - i * nc;
    M[i * LDM + j] = K[i * KD + j];
  }
  if (t < nc) {
    kr[t] = K[t * KD + KD - 1];
    const CommonPsr c = cps[a];
    const double ph = col_phi(c.colptr, c.spec, c.gstart + t, th);
    dv[t] = 1.0 / ph;
    sq[t] = sqrt(phihat[(long long)bl * nc + t]);
  }
  __syncthreads();
  for (int k = 0; k < nc; ++k) {        // Gauss-Jordan inverse of K_GG (SPD)
    const double pinv = 1.0 / M[k * LDM + k];
    if (t < nc) {
      colk[t] = M[t * LDM + k];
      rowk[t] = M[k * LDM + t] * pinv;
    }
    __syncthreads();
    for (int idx = t; idx < nc * nc; idx += OS_WIDE_THREADS) {
      const int i = idx / nc, j = idx - i * nc;
      double v;
      if (i == k) v = (j == k) ? pinv : rowk[j];
      else if (j == k) v = -colk[i] * pinv;
      else v = M[i * LDM + j] - colk[i] * rowk[j];
      M[i * LDM + j] = v;
    }
    __syncthreads();
  }
  double* xo = xh + ((long long)bl * P + a) * nc;
  double* wo = wh + ((long long)bl * P + a) * nc * nc;
  if (t < nc) {
    double v = 0.0;
    for (int h = 0; h < nc; ++h) v += M[t * LDM + h] * kr[h];
    xo[t] = sq[t] * dv[t] * v;
  }
  for (int idx = t; idx < nc * nc; idx += OS_WIDE_THREADS) {
    const int g = idx / nc, h = idx - g * nc;
    const double z = (g == h ? dv[g] : 0.0) - dv[g] * M[g * LDM + h] * dv[h];
    wo[idx] = sq[g] * z * sq[h];
  }
}

// rho_ab, sig_ab for b > a: one wave per pair (lanes over the nc^2 entries).
__global__ __launch_bounds__(256) void os_pairs_kernel(const double* __restrict__ xh, const double* __restrict__ wh,
                                                       int P, int nc, double* __restrict__ rho,
                                                       double* __restrict__ sig) {
  const int a = blockIdx.x, bl = blockIdx.y, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const double* xa = xh + ((long long)bl * P + a) * nc;
  const double* wa = wh + ((long long)bl * P + a) * nc * nc;
  for (int b = a + 1 + w; b < P; b += 4) {
    const double* xb = xh + ((long long)bl * P + b) * nc;
    const double* wb = wh + ((long long)bl * P + b) * nc * nc;
    double top = 0.0, bot = 0.0;
    for (int g = lane; g < nc; g += 64) top += xa[g] * xb[g];
    for (int idx = lane; idx < nc * nc; idx += 64) bot += wa[idx] * wb[idx];
    top = wave_sum(top);
    bot = wave_sum(bot);
    if (lane == 0) {
      rho[((long long)bl * P + a) * P + b] = top / bot;
      sig[((long long)bl * P + a) * P + b] = 1.0 / sqrt(bot);
    }
  }
}

// OS = sum rho Gamma / sig^2 / sum Gamma^2 / sig^2 per draw (pairs in order).
__global__ void os_final_kernel(const double* __restrict__ rho, const double* __restrict__ sig,
                                const double* __restrict__ orf, int P, int B, double* __restrict__ os,
                                double* __restrict__ os_sig) {
  const int bl = blockIdx.x * blockDim.x + threadIdx.x;
  if (bl >= B) return;
  double num = 0.0, den = 0.0;
  for (int a = 0; a < P; ++a)
    for (int b = a + 1; b < P; ++b) {
      const double s = sig[((long long)bl * P + a) * P + b], r = rho[((long long)bl * P + a) * P + b];
      const double g = orf[a * P + b];
      num += r * g / (s * s);
      den += g * g / (s * s);
    }
  os[bl] = num / den;
  os_sig[bl] = 1.0 / sqrt(den);
}

// Global term of sample b: units[P * B + b] = -1/2 (log|Sigma_c| + q_c + sum_g log|M_g|).
__global__ void common_final_kernel(const double* __restrict__ ldet, const double* __restrict__ qv,
                                    const int* __restrict__ fail, const double* __restrict__ mlog,
                                    const int* __restrict__ rep, int nc, int Bc, int b0, int P, int B,
                                    double* __restrict__ units) {
  const int bl = blockIdx.x * blockDim.x + threadIdx.x;
  if (bl >= Bc) return;
  double ml = 0.0;
  for (int g = 0; g < nc; ++g) ml += mlog[(long long)bl * nc + rep[g]];
  double v = -0.5 * (ldet[bl] + qv[bl] + ml);
  if (fail[bl] || !(qv[bl] == qv[bl]) || !(ml == ml)) v = -INFINITY;
  units[(long long)P * B + b0 + bl] = v;
}

namespace {
size_t minv_lds_bytes(int P, bool terms) {
  return ((size_t)P * (P + 1) + 3 * P + (terms ? EWH_COMMON_MAX_TERMS : 0)) * sizeof(double);
}
}  // namespace

bool minv_in_registers(int P, const KernelPlan& plan) { return P <= MINV_PMAX && plan.minv_reg; }

hipError_t set_minv_attributes(int P) {
  const hipError_t e = hipFuncSetAttribute((const void*)common_minv_kernel<false>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)minv_lds_bytes(P, false));
  if (e != hipSuccess) return e;
  return hipFuncSetAttribute((const void*)common_minv_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)minv_lds_bytes(P, true));
}

// terms.n_term == 0: the legacy pair (orf, cspec) on the kernels as they were;
// else the term-form instantiations (orf / cspec unused)
void launch_minv(const CommonPsr* cps, int P, const double* orf, const DSpec* cspec, const CommonTerms& terms, int nc,
                 const int* uniq, int nuniq, const double* theta, int ldth, int b0, int nsamp, double* minv,
                 double* mlog, const KernelPlan& plan, hipStream_t st) {
  CommonTerms ct = terms;
  const bool general = ct.n_term > 0;
  const bool reg = minv_in_registers(P, plan);
  ct.lds_doubles = reg ? 0 : (int)(minv_lds_bytes(P, general) / sizeof(double));
  if (reg && general)
    hipLaunchKernelGGL(common_minv_reg_kernel<true>, dim3(nuniq, nsamp), dim3(512), 0, st, cps, P, orf, cspec, nc, uniq,
                       theta, ldth, b0, minv, mlog, ct);
  else if (reg)
    hipLaunchKernelGGL(common_minv_reg_kernel<false>, dim3(nuniq, nsamp), dim3(512), 0, st, cps, P, orf, cspec, nc,
                       uniq, theta, ldth, b0, minv, mlog, ct);
  else if (general)
    hipLaunchKernelGGL(common_minv_kernel<true>, dim3(nuniq, nsamp), dim3(256), minv_lds_bytes(P, true), st, cps, P,
                       orf, cspec, nc, uniq, theta, ldth, b0, minv, mlog, ct);
  else
    hipLaunchKernelGGL(common_minv_kernel<false>, dim3(nuniq, nsamp), dim3(256), minv_lds_bytes(P, false), st, cps, P,
                       orf, cspec, nc, uniq, theta, ldth, b0, minv, mlog, ct);
}

void launch_common_chunk(const double* keep, int KD, int P, int nc, int B, int b0, int nsamp, const double* minv,
                         const double* mlog, const int* rep, int Np, double* dense, double* wbuf, double* cldet,
                         double* cq, int* cfail, double* units, const KernelPlan& plan, hipStream_t st) {
  const int nb = nsamp, nbk = Np / DCB;
  hipLaunchKernelGGL(common_assemble_kernel, dim3((Np + 3) / 4, nb), dim3(256), 0, st, keep, KD, P, nc, (long long)B,
                     b0, minv, rep, Np, dense, cldet, cq, cfail);
  // one or a few proposals (PTMCMC): right-looking -- after each panel the
  // trailing tiles (i, j > k) are updated in parallel (m (m + 1) / 2 tiles
  // per launch, K = 64), instead of the left-looking row update whose
  // K = 64 k accumulation of one tile is a serial chain on one CU.  Tile
  // (i, j) takes the same K = 64 slabs in the same order into the same
  // accumulator (stored and reloaded in full between panels): bit-identical.
  const bool right = plan.corr_right && nb <= CORR_RIGHT_LOOKING_MAX;
  for (int k = 0; k < nbk; ++k) {
    const int m = nbk - k - 1;
    if (right) {
      // the diagonal block k + 1 is factored inside the update launch of
      // step k (dchol_update_diag_kernel) unless the plan launches it apart
      const bool fuse_diag = plan.corr_fuse_diag;
      if (k == 0 || !fuse_diag) {
        if (m == 0)
          hipLaunchKernelGGL(HIP_KERNEL_NAME(dchol_diag_reg_kernel<true>), dim3(nb), dim3(64), 0, st, dense, Np, k,
                             wbuf, cldet, cq, cfail);
        else
          hipLaunchKernelGGL(HIP_KERNEL_NAME(dchol_diag_reg_kernel<false>), dim3(nb), dim3(64), 0, st, dense, Np, k,
                             wbuf, cldet, cq, cfail);
      }
      if (m == 0) continue;
      hipLaunchKernelGGL(dchol_panel_reg_kernel, dim3(4 * m, nb), dim3(64), 0, st, dense, Np, k, wbuf);
      if (!fuse_diag)
        hipLaunchKernelGGL(dchol_update_kernel, dim3(m * (m + 1) / 2, nb), dim3(256), 0, st, dense, Np, k);
      else if (m == 1)   // block k + 1 is the last one (its pivot q_c)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(dchol_update_diag_kernel<true>), dim3(1, nb), dim3(256), 0, st, dense, Np,
                           k, wbuf, cldet, cq, cfail);
      else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(dchol_update_diag_kernel<false>), dim3(m * (m + 1) / 2, nb), dim3(256), 0,
                           st, dense, Np, k, wbuf, cldet, cq, cfail);
      continue;
    }
    // default for large sample chunks: row update + panel fused (the updated
    // tile never round-trips through HBM); small chunks keep the row update
    // of every tile in one launch, which shortens the dependent chain per
    // block row
    const bool fused = plan.corr_fused && nb >= 64;
    // two block rows per update pass (dchol_rowpair_kernel) for the large
    // chunks: at an even k with a row k + 1 following, the rows p < k of
    // both rows' tiles j > k first; row k + 1 then takes only p = k
    const bool pairs = fused && plan.corr_pairs;
    int p0 = 0;                                       // the first row p this block row still needs
    if (pairs && (k & 1)) p0 = k - 1;
    const bool pair_here = pairs && !(k & 1) && m > 0 && k > 0;
    if (plan.corr_rowupdate_r1 && k > 0)     // round-1 row update (both operands staged through LDS)
      hipLaunchKernelGGL(dchol_rowupdate_kernel, dim3(m + 1, nb), dim3(256), 0, st, dense, Np, k);
    else if (k > 0 && !plan.corr_trailing)   // the diagonal tile's row update only (fused), or the whole row
      hipLaunchKernelGGL(dchol_rowupdate2_kernel, dim3(fused ? 1 : m + 1, nb), dim3(256), 0, st, dense, Np, k, p0);

    if (plan.corr_diag_lds) {   // A/B: round-1 LDS diagonal block + LDS-staged panel
      hipLaunchKernelGGL(dchol_diag_kernel, dim3(nb), dim3(256), 0, st, dense, Np, k, wbuf, cldet, cq, cfail);
      if (m > 0) hipLaunchKernelGGL(dchol_panel_kernel, dim3(m, nb), dim3(256), 0, st, dense, Np, k, wbuf);
    } else {
      if (m > 0)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(dchol_diag_reg_kernel<false>), dim3(nb), dim3(64), 0, st, dense, Np, k,
                           wbuf, cldet, cq, cfail);
      else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(dchol_diag_reg_kernel<true>), dim3(nb), dim3(64), 0, st, dense, Np, k,
                           wbuf, cldet, cq, cfail);
      if (m > 0 && fused) {
        if (plan.corr_one_tile)   // (dev A/B: one tile per workgroup, one row per pass: the round-3 form)
          hipLaunchKernelGGL(HIP_KERNEL_NAME(dchol_rowpanel_kernel<1>), dim3(m, nb), dim3(256), 0, st, dense, Np, k, 0,
                             wbuf);
        else if (pair_here && plan.corr_pair_unpiped)   // (dev A/B: U_pj loaded at the top of each step)
          hipLaunchKernelGGL(HIP_KERNEL_NAME(dchol_rowpair_kernel<false>), dim3(m, nb), dim3(512), 0, st, dense, Np, k,
                             wbuf);
        else if (pair_here)         // rows k and k + 1 over p < k, row k's panel
          hipLaunchKernelGGL(HIP_KERNEL_NAME(dchol_rowpair_kernel<true>), dim3(m, nb), dim3(512), 0, st, dense, Np, k,
                             wbuf);
        else
          hipLaunchKernelGGL(HIP_KERNEL_NAME(dchol_rowpanel_kernel<2>), dim3((m + 1) / 2, nb), dim3(512), 0, st, dense,
                             Np, k, p0, wbuf);
      } else if (m > 0) {
        hipLaunchKernelGGL(dchol_panel_reg_kernel, dim3(4 * m, nb), dim3(64), 0, st, dense, Np, k, wbuf);
      }
    }
    if (m > 0 && plan.corr_trailing)   // A/B: right-looking trailing update
      hipLaunchKernelGGL(dchol_update_kernel, dim3(m * (m + 1) / 2, nb), dim3(256), 0, st, dense, Np, k);
  }
  hipLaunchKernelGGL(common_final_kernel, dim3((nb + 255) / 256), dim3(256), 0, st, cldet, cq, cfail, mlog, rep, nc,
                     nb, b0, P, B, units);
}

void launch_optstat(const double* keep, int KD, int P, int nc, const CommonPsr* cps, const double* theta, int ldth,
                    const double* phihat, double* xh, double* wh, int B, double* rho, double* sig, const double* orf,
                    double* os, double* os_sig, hipStream_t st) {
  if (nc <= 31) {
    hipLaunchKernelGGL(os_xz_kernel, dim3(P, B), dim3(64), 0, st, keep, KD, P, nc, cps, theta, ldth, phihat, xh, wh);
  } else {
    // (<= 33 KB at the cap of 63 columns: inside the default dynamic-LDS limit)
    const size_t nd = os_wide_lds_doubles(nc);
    hipLaunchKernelGGL(os_xz_wide_kernel, dim3(P, B), dim3(OS_WIDE_THREADS), nd * sizeof(double), st, keep, KD, P, nc,
                       cps, theta, ldth, phihat, xh, wh, (int)nd);
  }
  hipLaunchKernelGGL(os_pairs_kernel, dim3(P, B), dim3(256), 0, st, xh, wh, P, nc, rho, sig);
  hipLaunchKernelGGL(os_final_kernel, dim3((B + 255) / 256), dim3(256), 0, st, rho, sig, orf, P, B, os, os_sig);
}

}  // namespace ewh_dev
