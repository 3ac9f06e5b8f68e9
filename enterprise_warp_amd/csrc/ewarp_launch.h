// ewarp_launch.h — launch wrappers of every kernel family, called by the C ABI
// units ewarp_hip.hip and ewarp_setup.hip, one heading per translation unit
// that defines them (each includes this header), with the constants and structs
// the host code shares with a family.  Arguments are device pointers,
// dimensions, the stream and, where a schedule is chosen, the KernelPlan of the
// kernel mode.  Launchers that return int: 0 on success, negative EWH_E* on error.
#pragma once

#include "ewarp_dev.h"
#include "ewarp_plan.h"

namespace ewh_dev {

// ---- contract.hip, contract_wide.hip: G = T_aug^T W T_aug - sum_e beta_e s_e s_e^T
constexpr int CT_ROWS = 32;   // TOA rows per contraction tile (8 MFMA k-steps); T_aug is padded by this many zero rows
// Glo: the low part of G (bases past 16 blocks only; may be NULL)
int launch_contract_nb(int nb, const PsrDev& P, const double* w, const double* beta, const double* s,
                       const double* fac, double* G, int nb_samples, hipStream_t st, double* Glo = nullptr);
// waves: 4 or 8 per sample (0 = the measured default for nb); nb: 1..CONTRACT2_NB_MAX
int launch_contract2_nb(int nb, int waves, const PsrDev& P, const double* w, const double* beta, double* s,
                        long long s_stride, double* G, int nb_samples, hipStream_t st, const double* rho = nullptr);
// dynamic-LDS attributes of the contraction kernels on the current device
int set_contract_attributes();
// the contraction of a basis past 16 blocks (contract_wide.hip)
int launch_contract_wide(int nb, const PsrDev& P, const double* w, const double* beta, const double* s,
                         const double* fac, double* G, int nb_samples, hipStream_t st, double* Glo);

// ---- chol_small.hip, chol_small_pl.hip, chol_partial.hip: chol_mfma_kernel
// mode: ewh_set_kernel_mode (the dev library's A/B variants of nb == 8); nb: 1..MFMA_NB_MAX
// dead: dead k-slices of block row 0 that every job of the launch has
// (front_dead of the widest mreal; 0 is always valid)
// img: every job of the launch carries the operand image of the order the
// launch takes (CholJob::img_front where front_inst(nb, dead) >= 1, else img)
// pl: every job of the launch carries compact power-law records (CholJob::pl):
// the fixed-form prologue (launch_chol_small_pl, chol_small_pl.hip: nb as
// checked by launch_chol_small; stamp: the dev library's mode-21 twin)
int launch_chol_small(int mode, int nb, int dead, bool img, bool pl, const UnitSpan& s);
void launch_chol_small_pl(int nb, int dead, bool img, bool stamp, const UnitSpan& s);
// true when kernel A/B mode `mode` (>= 3, not 7) is compiled into this library
// (dev library only: make dev, -DEWH_DEV)
bool variant_built(int mode);
// keep_out: pulsar-major kept blocks, keep_bs samples per pulsar (see chol_mfma_kernel KEEP);
// the (nb, keep) of partial_in_registers (ewarp_route.h)
int launch_partial_nb(int nb, int keep, const UnitSpan& s, double* keep_out, int keep_bs);

// ---- chol_big.hip: nb 10..BIG_NB_MAX; a scratch slot per workgroup, at most cap per launch
int launch_chol_big_nb(int nb, const UnitSpan& s, double* scr, long long cap);

// ---- chol_lat.hip: the latency form for small batches
// unit term of a latency-kernel unit whose dataflow wait ran out (a NaN
// payload no other path writes; ewh_lnl_batch returns EWH_E_HIP on it)
constexpr unsigned long long LAT_STALL_BITS = 0x7ff4dead057a1100ull;
// one 4-wave workgroup per unit of units [0, P B); theta and host_units may be host-mapped
// pinned memory; every unit term goes to units[p B + b] and host_units[p B + b].  Returns 1
// if nb has no latency kernel (nb > LAT_NB_MAX: the caller uses the batched path).
// dead: as launch_chol_small (the two kernels keep the same working order)
int launch_chol_lat(int nb, int dead, const CholJob* jobs, int B, int P, const double* theta, int ldth, double* units,
                    double* host_units, hipStream_t st, bool stamp = false, int var = 0);

// ---- chol_wide.hip: any width up to WIDE_NB_MAX blocks
// units [u0, u0 + n), slabs of at most cap workgroups, each with scr_per_wg doubles of scratch (wide_scratch_per_wg);
// keep > 0: the partial factorisation, kept blocks to keep_out as chol_mfma_kernel<KEEP> writes them
long long wide_scratch_per_wg(int nb, int keep);
// rev = 1 (keep == 0): the reversed column order (the verify step)
int launch_chol_wide(const UnitSpan& s, double* scr, long long scr_per_wg, long long cap, int keep, double* keep_out,
                     int keep_b0, int keep_bs, int rev = 0, double* units_rev = nullptr, bool pair = true);

// ---- chol_dd.hip: the double-double factorisation
// one 512-thread workgroup per unit, 2 ld^2 doubles of scratch each
// (dd_scratch_per_wg); ld = the jobs' width (one width per launch)
long long dd_scratch_per_wg(int ld);
int launch_chol_dd(const UnitSpan& s, double* scr, long long scr_per_wg, long long cap, int ld, bool r05a = false);
// dynamic-LDS limits of chol_dd_kernel on the current device
int set_dd_attributes();
// the verify-and-refine form: units a (forward fp64) vs b (reversed fp64) of
// [u0, u0 + n) -> list / count of the disagreeing ones (count zeroed by the
// caller; total, if not NULL: total[0] += the count, total[1] += n; all:
// every unit listed -- kernel mode 29's refine_failed), then
// chol_dd_kernel over the list (cap workgroups looping) into units; r05a: the
// round-5a panel solve (row-oriented; dev mode 34)
int launch_verify_units(const double* a, const double* b, long long u0, long long n, int* list, int* count,
                        unsigned long long* total, hipStream_t st, bool all = false);
// kernel mode 29 (every unit in double-double): total[0] and total[1] += n on
// the device, in stream order (so graph replays count, captures do not)
int launch_count_units(unsigned long long* total, long long n, hipStream_t st);
// (the units are the listed ones: the span's u0 and n are not read)
int launch_chol_dd_list(const UnitSpan& s, double* scr, long long scr_per_wg, long long cap, const int* list,
                        const int* count, int ld, bool r05a = false);

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
// (HD / monopole / dipole ORF; [ent] FourierBasisCommonGP,
// enterprise_models.py:390-415), fixed white noise.
// Per sample b (after the per-pulsar partial factorisations):
//   M_g = Gamma phi_c(g) + diag_a(phi_own(a, g))          (P x P, per common column g)
//   Sigma_c = blockdiag_a(S^G_a) + [M_g^-1]_(a,g),(b,g)    (P n_c square, + r row)
//   lnL_b = sum_a local_a - 1/2 (log|Sigma_c| + q_c + sum_g log|M_g|)
// Sigma_c is factored densely (blocked right-looking, 64-wide panels: diagonal
// block by LDS Cholesky + explicit inverse, panel and trailing update by fp64
// MFMA); its last pivot is q_c = rho - d'^T Sigma_c^-1 d'.
struct CommonPsr {
  const int* colptr;     // reduced-layout CSR of the pulsar's own spectral entries
  const DSpec* spec;
  int gstart;            // reduced index of common column 0
  int pad_;
};

// The term form of the cross-pulsar prior (ABI 9, ewh_common_term):
//   M_g = sum_t coef_t(theta) phi_t(g; theta) mat_t + diag_a(phi_own(a, g))
// n_term = 0: the legacy pair (Gamma, phi_c) of the kernels' orf / cspec
// arguments.  The terms' spectra are kept once per distinct content: term t
// reads entry g of set[t], at spec[set[t] nc + g].
struct CommonTerms {
  int n_term = 0;
  int lds_doubles = 0;                 // dynamic LDS of the launch (the LDS kernel; debug checks)
  const double* mat = nullptr;         // n_term matrices, P x P each
  const ewh_pref* coef = nullptr;      // n_term
  const DSpec* spec = nullptr;         // distinct spectrum sets, nc entries each
  const int* set = nullptr;            // n_term
};

constexpr int DCB = 64;            // dense panel width
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
