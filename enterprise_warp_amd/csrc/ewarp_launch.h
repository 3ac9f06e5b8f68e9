// ewarp_launch.h — launch wrappers of the kernel families white.hip, delay.hip
// and common_dense.hip, called by the C ABI unit ewarp_hip.hip.  (The
// factorisation and contraction families are declared at the end of
// ewarp_dev.h.)  Arguments are device pointers, dimensions, the stream and,
// where a schedule is chosen, the KernelPlan of the context's kernel mode.
#pragma once

#include "ewarp_dev.h"
#include "ewarp_plan.h"

namespace ewh_dev {

// ---- white.hip: white-noise terms, epoch sums, double-double Grams, the
// fixed-white-noise timing-model elimination
// w, beta, -1/2 log|N| (Kb), chromatic factors (fac) and, rho != NULL, r^T W r
// of samples [b0, b0 + nsamp)
void launch_wn_weights(const PsrDev& P, const double* theta, int ldth, int b0, int nsamp, double* w, double* beta,
                       double* Kb, double* fac, double* rho, hipStream_t st);
// ECORR epoch sums of nsamp samples; multi: ES_S samples per workgroup where
// the basis is constant and no epoch is longer than ES_RMAX TOAs
void launch_epoch_sums(const PsrDev& P, int n_epoch, int max_epoch, bool multi, const double* w, const double* fac,
                       double* s, int nsamp, hipStream_t st);
void launch_gram_dd(const PsrDev& P, int nb, const double* Xlo, const double* w, const double* beta, double* G,
                    double* Glo, hipStream_t st);
// the same Gram for the listed units (slots list slots per upper block)
void launch_gram_dd_units(const PsrDev& P, int nb, unsigned slots, const double* Xlo, const double* w,
                          const double* beta, const int* list, const int* count, int B, int b_off, double* G,
                          double* Glo, hipStream_t st);
void launch_schur(double* Ghi, double* Glo, int ld, int m, int nlead, const int* col_ptr, const DSpec* spec, double Kb,
                  double* S, int fx_ld, int nloc, int gstart, int ncommon, double* Kout, int* fail_out, double* Slo,
                  hipStream_t st);
// out = fl(hi + 2 lo), n entries
void launch_rev_input(const double* hi, const double* lo, double* out, long long n, hipStream_t st);
// the operand images of S (nb <= MFMA_NB_MAX blocks, row-major, ld = 16 nb;
// img_doubles(nb) each): stored order, and (front != NULL) the front-pad
// order with s leading pads
void launch_operand_image(const double* S, int nb, int s, double* stored, double* front, hipStream_t st);

// ---- delay.hip: deterministic delay signals (the per-sample residual column)
constexpr int DELAY_MAX = 8;   // delay entries per pulsar
// device form of one ewh_delay_entry (i < 0: the constant v)
struct DDelay {
  int kind, i0, i1, i2, i3, pad_;
  double v0, v1, v2, v3, idx;
};
struct DelayDev {
  int n_delay;
  const DDelay* ent;      // n_delay
  const double* toas;     // n_toa, seconds
};
// The column [T_aug^T z; r'^T z] (hi, lo; ld entries per sample) of samples
// [b0, b0 + nsamp), z = N^-1 (r - sum_k delta_k): w / beta of sample i at
// w + i wstride / beta + i bstride (0: the fixed-white-noise values); R, Z:
// n_toa x 16 ceil(nsamp / 16) doubles of scratch each; Kb[i] = -inf where a
// delay parameter of sample i is not finite.  fac: wn_weights' chromatic
// factors (read when P.n_bgroup > 0)
int launch_delay_column(const PsrDev& P, const DelayDev& D, const double* theta, int ldth, int b0, int nsamp,
                        const double* w, long long wstride, const double* beta, long long bstride,
                        const double* fac, double* R, double* Z, double* col_hi, double* col_lo, double* Kb,
                        hipStream_t st);
// the columns into the last row and column of nsamp matrices G (and Glo, may be NULL)
void launch_delay_scatter(int ld, int nsamp, const double* col_hi, const double* col_lo, double* G, double* Glo,
                          hipStream_t st);
// one matrix (hi, lo; n entries) and Kval into nsamp slots of G, Glo and Kb
void launch_gram_broadcast(const double* src_hi, const double* src_lo, long long n, double Kval, int nsamp, double* G,
                           double* Glo, double* Kb, hipStream_t st);

// ---- cond.hip: the conditional Gaussian process (ABI 10, ewh_cond_gp)
// Sigma = G + diag(1/phi) = L L^T in place on nsamp slots (ld x ld, r last),
// x = L^-T (L^-1 d + z): ld entries per unit (device basis, pads zero, NaN
// where status != 0); z: m per unit or NULL; theta: the chunk's rows; Kb: the
// slots' -1/2 log|N| (has_delay: -inf marks a non-finite delay parameter)
int launch_cond_solve(double* G, int ld, int m, const int* col_ptr, const DSpec* spec, const double* theta, int ldth,
                      const double* Kb, bool has_delay, const double* z, int nsamp, double* x, int* status,
                      hipStream_t st);
// the back-map to the caller's basis (C: nl x (nproj + 1), pcols: the projected
// columns), coef (m per unit, may be NULL) and, n_group > 0, the realisation
// operand V (ld x ldv, zeroed by the caller; column bl * n_group + g)
int launch_cond_pack(const double* x, int ld, int m, int nl, int nproj, const int* pcols, const double* C,
                     const int* status, const int* grp, int n_group, int nsamp, double* coef, double* V, int ldv,
                     hipStream_t st);
// Y[o][t] = sum_k T_aug[t][k] V[k][o] for o < nout (n_toa per output); fac: the
// chunk's chromatic factors (read when P.n_bgroup > 0: the VALU kernel)
int launch_cond_process(const PsrDev& P, const double* fac, const double* V, int ldv, int n_group, int nout, double* Y,
                        hipStream_t st);

// ---- cond_joint.hip: the conditional GP under a correlated common process
// (ABI 11, ewh_cond_joint): the joint solve in the order [own blocks, pulsar-
// major | common columns, (pulsar, column)]
// most columns of Sigma_c (P x common columns): the dense solve keeps its
// vector in LDS (128 KiB of the 160 KiB at this bound)
constexpr int COND_JOINT_NC_MAX = 16384;
// the order of the padded Sigma_c: P nc rounded up to 16
int cond_joint_npad(int P, int nc);
// Stage 1 on nsamp slots (ld x ld, r last; own block [0, mo), common block
// [mo, mo + nc)): phi^-1 on the own columns, L_A and W in place, y_a | e in the
// r row; S: (nc + 1) x nc per unit (S_p, then the row e_p); status 0 / 1
int launch_cond_joint_partial(double* G, int ld, int mo, int nc, const int* col_ptr, const DSpec* spec,
                              const double* theta, int ldth, int nsamp, double* S, int* status, hipStream_t st);
// Stage 2 of nsamp samples: Sigma_c (cond_joint_npad(P, nc) squared doubles per
// sample in dense) from the S blocks (pulsar a's of sample bl at index
// a sstride + bl; pstat likewise) and launch_minv's minv / mlog / rep, then
// x_c = L_c^-T (L_c^-1 e + z_c) into xc (Npad per sample).  z: n_coef normals
// per sample or NULL, pulsar a's common columns from cstart[a].  sfail[bl]: the
// sample failed (an own block, M_g, or a pivot of Sigma_c)
int launch_cond_joint_dense(const double* S, long long sstride, int P, int nc, int nsamp, const int* pstat,
                            const double* minv, const double* mlog, const int* rep, double* dense, double* rhs,
                            const double* z, long long n_coef, const int* cstart, int* sfail, double* xc,
                            hipStream_t st);
// Stage 3 on one pulsar's retained slots: x = [L_A^-T (y_a + z_a - W^T x_c) |
// x_c,p | 0], ld per unit (cond_pack_kernel's input); nlo: the own columns that
// take a normal (from z_off); status 0, 1 (this own block failed) or 3
int launch_cond_joint_back(const double* G, int ld, int mo, int nc, int nlo, const double* xc, int Npad, int xc_off,
                           const double* z, long long n_coef, long long z_off, const int* pstat, const int* sfail,
                           int nsamp, double* x, int* status, hipStream_t st);

// ---- common_dense.hip: the correlated common process and the optimal statistic
// the M_g inverses run in registers (else: the LDS kernel, dynamic LDS set by
// set_minv_attributes)
bool minv_in_registers(int P, const KernelPlan& plan);
hipError_t set_minv_attributes(int P);
// M_g^-1 and log|M_g| of samples [b0, b0 + nsamp) for the nuniq distinct M_g
// (terms.n_term == 0: M_g = orf phi_c(g) + diag(own), the legacy kernels; else the
// term form, orf / cspec unused)
void launch_minv(const CommonPsr* cps, int P, const double* orf, const DSpec* cspec, const CommonTerms& terms, int nc,
                 const int* uniq, int nuniq, const double* theta, int ldth, int b0, int nsamp, double* minv,
                 double* mlog, const KernelPlan& plan, hipStream_t st);
// One sample chunk [b0, b0 + nsamp) of a batch of B: Sigma_c assembled from
// the kept blocks and minv, factored block row by block row in the schedule
// the plan and the chunk size select, the global term to units[P B + b].
void launch_common_chunk(const double* keep, int KD, int P, int nc, int B, int b0, int nsamp, const double* minv,
                         const double* mlog, const int* rep, int Np, double* dense, double* wbuf, double* cldet,
                         double* cq, int* cfail, double* units, const KernelPlan& plan, hipStream_t st);
// optimal statistic of B samples from the pulsars' kept blocks
void launch_optstat(const double* keep, int KD, int P, int nc, const CommonPsr* cps, const double* theta, int ldth,
                    const double* phihat, double* xh, double* wh, int B, double* rho, double* sig, const double* orf,
                    double* os, double* os_sig, hipStream_t st);

}  // namespace ewh_dev
