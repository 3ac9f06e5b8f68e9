// ewarp_hip.hip — MI355X (gfx950) PTA log-likelihood engine.
//
// Implements include/ewarp_hip.h.  The arithmetic restates the enterprise
// likelihood that enterprise_warp drives (signal_base.PTA built at
// enterprise_warp.py:502, called at bilby_warp.py:35):
//
//   lnL = sum_p [ -1/2 (r^T N^-1 r + log|N|)
//                 + 1/2 (d^T Sigma^-1 d - log|Sigma| - log|phi|) ],
//   Sigma = T^T N^-1 T + diag(1/phi),  d = T^T N^-1 r.
//
// Device formulation:
//  * The residual vector is appended to the basis as its LAST column
//    (T_aug = [T | pad | r]), so one contraction G = T_aug^T N^-1 T_aug gives
//    T^T N^-1 T, d and r^T N^-1 r together, and one Cholesky of
//    G + diag(1/phi, 0) gives, in its last pivot, q = r^T N^-1 r - d^T Sigma^-1 d.
//    lnL_p = -1/2 log|N| - 1/2 q - sum_j log U_jj - 1/2 sum_j log phi_j.
//  * White noise fixed: G and the elimination of the theta-independent
//    leading (timing-model, phi = 1e40) block are computed once at create; per
//    sample only the reduced (m - n_tm + 1)^2 factorisation runs.
//  * Kernels, one translation unit per family behind launch_* wrappers
//    (ewarp_launch.h): white.hip -- wn_weights (N, ECORR
//    Sherman-Morrison terms), epoch_sums, the double-double Grams, schur
//    (fixed-WN lead elimination); contract*.hip -- contract_mfma (fp64 MFMA
//    T^T N^-1 T with LDS-staged TOA tiles); chol_*.hip -- chol_mfma (one wave
//    per (pulsar, sample): 16x16 blocks register-resident in MFMA C/D layout,
//    panel rows by VALU + cross-lane shuffles, trailing update by
//    v_mfma_f64_16x16x4_f64) and its wider / double-double relatives;
//    delay.hip -- deterministic delays: a delay pulsar's per-sample residual
//    column (ABI 8); cond.hip -- the conditional GP (ABI 10: coefficients,
//    draws, realisations); cond_joint.hip -- the same under a correlated
//    common process (ABI 11); common_dense.hip -- the correlated common process and
//    the optimal statistic.  Here: the C ABI -- kernel routing, the batch
//    drivers, the multi-device handle and the ewh_* entries -- and the kernels
//    launched from several of its entry points: chol_lds (general fallback,
//    matrix in LDS), reduce_units (sum over pulsars in pulsar order),
//    expand_theta, fold_partials.  The contexts it runs on (ewarp_ctx.h) are
//    built in ewarp_setup.hip; all memory is owned through ewarp_mem.h, whose
//    two functions -- the only allocation and free calls -- are defined here.
//  * What an ewh_set_kernel_mode number selects is decided once, in
//    ewarp_plan.h (plan_for); the code below tests the plan's named fields.
#include "ewarp_ctx.h"

#include <atomic>
#include <chrono>
#include <map>
#include <mutex>

namespace ewh_dev {

thread_local std::string g_err;

int set_err(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

// ----------------------------------------------------------------------------
// batched Cholesky, general fallback: one 256-thread block per unit, the
// (compacted) matrix as a packed lower triangle in LDS.
// ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void chol_lds_kernel(const CholJob* __restrict__ jobs, int B,
                                                       long long u0, int b_off,
                                                       const double* __restrict__ theta, int ldth,
                                                       double* __restrict__ out_units) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  __shared__ double red[4];
  const long long u = u0 + blockIdx.x;
  const int p = (int)(u / B), b = (int)(u % B);
  const CholJob J = jobs[p];
  const int mr = J.mreal, ma = mr + 1, ld = J.ld;
  double* L = sm;                               // ma(ma+1)/2
  double* col = sm + (long long)ma * (ma + 1) / 2;
  const double* A = J.mats + (long long)(b - b_off) * J.mstride;
  const double* th = theta + (long long)b * ldth;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int i = wave; i < ma; i += 4) {
    const int gi = i < mr ? i : ld - 1;
    const int base = i * (i + 1) / 2;
    for (int j = lane; j <= i; j += 64) L[base + j] = A[(long long)gi * ld + (j < mr ? j : ld - 1)];
  }
  __syncthreads();
  LogAcc lphi;
  for (int a = threadIdx.x; a < mr; a += 256) {
    double ph = 0.0;   // (col_phi written out: the helper swaps an add's operands here, profiles/r17/same_device_code.txt)
    for (int e = J.col_ptr[a]; e < J.col_ptr[a + 1]; ++e) ph += spec_phi(J.spec[e], th);
    L[a * (a + 1) / 2 + a] += 1.0 / ph;
    lphi.add(ph);
  }
  const double lphi_sum = block_sum256(lphi.value(), red);
  __syncthreads();
  LogAcc ldet;                                  // sum of log pivots = 2 sum log U_jj
  bool ok = true;
  for (int k = 0; k < ma - 1; ++k) {
    const double piv = L[k * (k + 1) / 2 + k];
    ok = ok && (piv > 0.0);
    ldet.add(piv);
    const double rinv = rsqrt_nr(piv);
    for (int i = k + 1 + threadIdx.x; i < ma; i += 256) col[i] = L[i * (i + 1) / 2 + k] * rinv;
    __syncthreads();
    for (int i = k + 1 + wave; i < ma; i += 4) {
      const double ci = col[i];
      const int base = i * (i + 1) / 2;
      for (int j = k + 1 + lane; j <= i; j += 64) L[base + j] = fma(-ci, col[j], L[base + j]);
    }
    __syncthreads();
  }
  const double qv = L[(ma - 1) * ma / 2 + ma - 1];
  if (threadIdx.x == 0) {
    double lnl = J.K[(long long)(b - b_off) * J.kstride] - 0.5 * qv - 0.5 * ldet.value() - 0.5 * lphi_sum;
    if (!ok || J.fail) lnl = -INFINITY;
    out_units[(long long)p * B + b] = lnl;
  }
}

// out[b] = sum_p units[p * B + b], pulsars in order.
__global__ void reduce_units_kernel(const double* __restrict__ units, int P, int B, double* __restrict__ out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double s = 0.0;
  for (int p = 0; p < P; ++p) s += units[(long long)p * B + b];
  out[b] = s;
}

// Multi-context handle, theta staging: segment s of the table (5 ints: row_lo,
// row_hi, ncol, column-list offset, payload offset; the column lists follow
// the nseg records) scatters its packed rows x columns payload into the
// full-layout theta [B x np] of this device.  Columns and rows outside the
// segments are never read by the context's units (stage_theta_range sets them
// to NaN first).
__global__ __launch_bounds__(256) void expand_theta_kernel(const double* __restrict__ stage,
                                                           const int* __restrict__ seg, int nseg, int np,
                                                           double* __restrict__ theta) {
  const int* rec = seg + 5 * blockIdx.x;
  const int r0 = rec[0], nr = rec[1] - rec[0], nc = rec[2];
  const int* cols = seg + 5 * nseg + rec[3];
  const double* src = stage + rec[4];
  for (int idx = threadIdx.x; idx < nr * nc; idx += 256) {
    const int r = idx / nc, j = idx - r * nc;
    theta[(long long)(r0 + r) * np + cols[j]] = src[idx];
  }
}

// Multi-context handle: out[b] = sum_i part[i * B + b], the contexts' partial
// sums (each over its unit range, pulsars in order) in context order.
__global__ void fold_partials_kernel(const double* __restrict__ part, int nd, int B, double* __restrict__ out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double s = 0.0;
  for (int i = 0; i < nd; ++i) s += part[(long long)i * B + b];
  out[b] = s;
}

}  // namespace ewh_dev

using namespace ewh_host;

// ----------------------------------------------------------------------------
// ewarp_mem.h: the library's only allocation and free calls
// ----------------------------------------------------------------------------
int ewh_mem::mem_alloc(MemKind kind, void** p, size_t bytes) {
  *p = nullptr;
  if (kind != MemKind::Device) {
    // coherent: the latency kernel's stores to it are visible to a spinning
    // host thread before the launch completes (and its theta reads bypass L2)
    const unsigned flags = kind == MemKind::PinnedCoherent
                               ? hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent
                               : hipHostMallocPortable;
    const hipError_t e = hipHostMalloc(p, bytes, flags);
    if (e == hipSuccess) return 0;
    *p = nullptr;
    return set_err(EWH_E_NOMEM, std::string("hipHostMalloc: ") + hipGetErrorString(e));
  }
  const hipError_t e = hipMalloc(p, bytes);
  if (e == hipSuccess) return 0;
  *p = nullptr;
  // needed and available: the kept blocks of a correlated batch are
  // P x B x KD^2 doubles, the caller's lever is B
  size_t fr = 0, tot = 0;
  const bool known = hipMemGetInfo(&fr, &tot) == hipSuccess;
  (void)hipGetLastError();
  return set_err(EWH_E_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e) + ": needed " +
                                  std::to_string(bytes) + " bytes, " +
                                  (known ? std::to_string(fr) + " of " + std::to_string(tot) + " bytes free on the device"
                                         : std::string("free device memory unknown")));
}

void ewh_mem::mem_free(MemKind kind, void* p) {
  if (kind == MemKind::Device) (void)hipFree(p);
  else (void)hipHostFree(p);
}

int ewh_host::set_lds_attributes() {
  if (hipFuncSetAttribute((const void*)chol_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)(LDS_MAX - 64)) != hipSuccess)
    return set_err(EWH_E_HIP, "hipFuncSetAttribute(chol_lds_kernel) failed");
  return 0;
}

// ----------------------------------------------------------------------------
// host side: routing and the batch drivers (contexts are built in ewarp_setup.hip)
// ----------------------------------------------------------------------------
namespace {

// Scratch budgets of the wide / double-double factorisations: one slot per
// resident workgroup, up to 4 GB, capped at an
// eighth of the device memory free when first sized, so several handles on
// one device -- multi-context tests, one handle per sampler thread -- cannot
// take it all; at least 128 MB, which KernelPlan::wide_r05a (dev mode 34)
// keeps, with the separate forward / reversed launches (A/B)
long long scratch_budget(DevCtx* h) {
  if (h->plan.wide_r05a) return 1LL << 27;
  if (h->scr_budget == 0) {
    size_t fr = 0, tot = 0;
    (void)hipSetDevice(h->device);
    h->scr_budget = hipMemGetInfo(&fr, &tot) == hipSuccess
                        ? std::max<long long>(1LL << 27, std::min<long long>(1LL << 32, (long long)(fr / 8)))
                        : (1LL << 27);
  }
  return h->scr_budget;
}

// Workgroup slots of `per` doubles that a wide / double-double scratch holds
// once it is sized to the budget (0: allocation failed): chol_dd_kernel at
// most 1024, chol_wide_kernel at most 4096 (<= 4 GB)
long long scratch_slots(DevCtx* h, Buf<double>& scr, long long per, long long max_slots) {
  const long long want = std::min<long long>(max_slots, std::max<long long>(1, scratch_budget(h) / per)) * per;
  if (scr.reserve((size_t)want, h->hook)) return 0;
  return std::min<long long>(max_slots, std::min<long long>((long long)scr.cap, want) / per);
}

// rows of units x batch: the pulsars' terms + the common term row
size_t n_units(const DevCtx* h, int B) { return (size_t)(h->P + (h->corr ? 1 : 0)) * B; }

int launch_wide(DevCtx* h, int nb, int keep, const UnitSpan& s, double* keep_out, int rev = 0,
                double* units_rev = nullptr) {
  if (nb > WIDE_NB_MAX) return set_err(EWH_E_UNSUPPORTED, "basis wider than 1023 columns");
  const long long per = wide_scratch_per_wg(nb, keep);
  const long long cap = scratch_slots(h, h->d_widescr, per, 4096);
  if (cap <= 0 || (units_rev && cap < 2)) return EWH_E_NOMEM;
  return launch_chol_wide(s, h->d_widescr.p, per, cap, keep, keep_out, 0, s.B, rev, units_rev, !h->plan.wide_r05a);
}

// the double-double counters (zeroed when first allocated); list: and room for the batch's unit list
int ensure_dd_lists(DevCtx* h, const UnitSpan& s, bool list) {
  if (!h->d_ddstat) {
    if (const int rc = dalloc(h, &h->d_ddstat, 2)) return rc;
    EWH_HIP(hipMemsetAsync(h->d_ddstat, 0, 2 * sizeof(unsigned long long), s.st));
  }
  return list ? h->d_ddlist.reserve(n_units(h, s.B) + 1, h->hook) : 0;
}

// Route::DdAll and Route::DdVerify of a span of nb blocks
int launch_dd_path(DevCtx* h, int nb, const UnitSpan& s) {
  const long long per = dd_scratch_per_wg(16 * nb);
  const long long cap = scratch_slots(h, h->d_ddscr, per, 1024);
  if (cap <= 0) return EWH_E_NOMEM;
  int rc;
  if ((rc = ensure_dd_lists(h, s, false))) return rc;
  if (h->plan.all_dd) {
    if ((rc = launch_count_units(h->d_ddstat, s.n, s.st))) return rc;
    return launch_chol_dd(s, h->d_ddscr.p, per, cap, 16 * nb, h->plan.wide_r05a);
  }
  if ((rc = h->d_units2.reserve(n_units(h, s.B), h->hook)) || (rc = ensure_dd_lists(h, s, true))) return rc;
  // the forward and reversed fp64 passes: one launch (both in one grid) when
  // one pass alone would leave SIMD slots empty (chol_wide_kernel: two waves
  // per SIMD), else two; dev mode 34: always two
  const bool fuse = !h->plan.wide_r05a && 2 * s.n <= 8LL * h->n_cu;
  if (!fuse) {
    UnitSpan r = s;
    r.units = h->d_units2.p;
    if ((rc = launch_wide(h, nb, 0, s, nullptr, 0)) || (rc = launch_wide(h, nb, 0, r, nullptr, 1))) return rc;
  } else if ((rc = launch_wide(h, nb, 0, s, nullptr, 0, h->d_units2.p))) {
    return rc;
  }
  int *count = h->d_ddlist.p, *list = count + 1;
  EWH_HIP(hipMemsetAsync(count, 0, sizeof(int), s.st));
  if ((rc = launch_verify_units(s.units, h->d_units2.p, s.u0, s.n, list, count, h->d_ddstat, s.st))) return rc;
  return launch_chol_dd_list(s, h->d_ddscr.p, per, std::min<long long>(cap, s.n), list, count, 16 * nb,
                             h->plan.wide_r05a);
}

// One launch of for_segments: the source of its matrices, its pulsar (FixedRun:
// the run's first), the width in blocks, the widest mreal of its jobs, its units
struct Segment { Source src; int p0, nb, mreal; UnitSpan span; };

// The units [all.u0, all.u0 + all.n) as launches, in unit order: with fixed
// white noise one segment per run of consecutive pulsars of one reduced width
// (h->d_jobs_fixed; no delay pulsar in a run), else one per pulsar and chunk
// of at most h->var.chunk samples on the chunk scratch's full-width matrices
// (h->d_jobs_var).  body(segment) returns 0 or the error that ends the walk.
template <class F>
int for_segments(const DevCtx* h, const UnitSpan& all, F&& body) {
  const long long B = all.B, u_end = all.u0 + all.n;
  for (long long u = all.u0, end; u < u_end; u = end) {
    const int p0 = (int)(u / B);
    const PsrHost& ps = h->psr[p0];
    const bool run = h->white_fixed && ps.delay.n_delay == 0;
    Segment g{run ? Source::FixedRun : h->white_fixed ? Source::FixedDelay : Source::Varying, p0,
              run ? ps.fx_nb : ps.nb, run ? ps.fx_m : ps.m, all};
    int p1 = p0 + 1;
    for (; run && p1 * B < u_end && h->psr[p1].fx_nb == g.nb && h->psr[p1].delay.n_delay == 0; ++p1)
      g.mreal = std::max(g.mreal, h->psr[p1].fx_m);
    end = std::min(u_end, run ? p1 * B : std::min((p0 + 1) * B, u + h->var.chunk));
    g.span.jobs = run ? h->d_jobs_fixed : h->d_jobs_var;
    g.span.u0 = u;
    g.span.n = end - u;
    g.span.b_off = run ? 0 : (int)(u - p0 * B);
    if (const int rc = body(g)) return rc;
  }
  return 0;
}

// An -inf unit term from an fp64 factorisation is a rounding failure wherever
// the exact Sigma is positive definite (every full-rank basis), so the
// segment's units whose term is not finite are listed (verify_units_kernel on
// the terms alone) and refactored by chol_dd_kernel on a double-double matrix:
// the cached S_hi + S_lo, the slots' G_hi + G_lo with the per-sample column
// (the fixed sources), or G_hi + G_lo of those samples from
// gram_dd_units_kernel (Source::Varying: the chunk's weights in h->var).  The
// -inf that remains is the double-double factorisation's (or CholJob::fail).
// Four launches, empty lists exit at once.  When: refine_after (ewarp_route.h).
int refine_failed(DevCtx* h, const Segment& g) {
  const UnitSpan& s = g.span;
  const long long per = dd_scratch_per_wg(16 * g.nb);
  const long long cap = scratch_slots(h, h->d_ddscr, per, 1024);
  if (cap <= 0) return EWH_E_NOMEM;
  int rc;
  if ((rc = ensure_dd_lists(h, s, true))) return rc;
  int *count = h->d_ddlist.p, *list = count + 1;
  EWH_HIP(hipMemsetAsync(count, 0, sizeof(int), s.st));
  if ((rc = launch_verify_units(s.units, s.units, s.u0, s.n, list, count, h->d_ddstat, s.st,
                                refine_lists_all(g.src, g.nb, h->plan))))
    return rc;
  if (g.src == Source::Varying) {
    const PsrHost& ps = h->psr[g.p0];
    launch_gram_dd_units(ps.dev, ps.nb, (unsigned)std::min<long long>(s.n, 64), ps.d_Tlo, h->var.d_w.p, h->var.d_beta.p,
                         list, count, s.B, s.b_off, h->var.d_G.p, h->var.d_Glo.p, s.st);
    // (a delay pulsar: that Gram carries the stored r -- the chunk's per-
    // sample residual column goes back in, n = the chunk's samples)
    if (ps.delay.n_delay > 0)
      launch_delay_scatter(ps.ld, (int)s.n, h->var.d_dcol.p, h->var.d_dcollo.p, h->var.d_G.p, h->var.d_Glo.p, s.st);
    EWH_HIP(hipGetLastError());
  }
  return launch_chol_dd_list(s, h->d_ddscr.p, per, std::min<long long>(cap, s.n), list, count, 16 * g.nb, false);
}

// the partial factorisation (correlated common process) of a span of pulsars
// with nb blocks (partial_route_for)
int partial_units(DevCtx* h, int nb, const UnitSpan& s, double* keep_out) {
  if (partial_route_for(h->plan, nb, h->keep) == PartialRoute::Register)
    return launch_partial_nb(nb, h->keep, s, keep_out, s.B);
  return launch_wide(h, nb, h->keep, s, keep_out);
}

#ifdef EWH_DEV
// register-kernel launches since the library was loaded, by spectrum prologue
// (ewh_dev_prologue_launches): [0] interpreted, [1] fixed form
std::atomic<long long> g_prologue_launches[2] = {{0}, {0}};   // (handles may be driven from several host threads)
#endif

int launch_register(DevCtx* h, const Segment& g) {
  const UnitSpan& s = g.span;
  // mreal is the widest of the launch's jobs: the fewest leading pads, so
  // every job has these dead slices (the optimal statistic's jobs take
  // phi^-1 on every column of the frame: none)
  const int dead = h->osmode ? 0 : front_dead(16 * g.nb, g.mreal);
  // the operand images instead of the matrices (setup_fixed) where every
  // job of the launch has the image of the order the launch takes -- a
  // launch-wide rule like `dead`; the per-sample slots of d_jobs_var have none
  bool img = g.src == Source::FixedRun;
  for (long long p = s.u0 / s.B; img && p <= (s.u0 + s.n - 1) / s.B; ++p)
    img = (front_inst(g.nb, dead) >= 1 ? h->psr[p].d_imgf : h->psr[p].d_img) != nullptr;
  // the fixed-form spectrum prologue where every job of the launch has the
  // compact records (power laws only; setup: pl_pack) -- launch-wide again
  bool pl = g.src == Source::FixedRun && h->plan.compact_spectra && h->stage_spectra;
  for (long long p = s.u0 / s.B; pl && p <= (s.u0 + s.n - 1) / s.B; ++p) pl = h->psr[p].d_fx_pl != nullptr;
  pl = pl && pl_built(g.nb, front_inst(g.nb, dead), img);
#ifdef EWH_DEV
  g_prologue_launches[pl ? 1 : 0]++;
#endif
  return launch_chol_small(h->kernel_mode, g.nb, dead, img, pl, s);
}

int launch_lds(const UnitSpan& s, int mreal) {
  const size_t ma = (size_t)mreal + 1, lds = (ma * (ma + 1) / 2 + ma) * sizeof(double);   // packed triangle + one column
  if (lds > LDS_MAX - 64) return set_err(EWH_E_UNSUPPORTED, "reduced matrix too large for the LDS Cholesky kernel");
  // (the dynamic-LDS attribute of chol_lds_kernel is set per device in create_ctx)
  hipLaunchKernelGGL(chol_lds_kernel, dim3((unsigned)s.n), dim3(256), lds, s.st, s.jobs, s.B, s.u0, s.b_off, s.theta,
                     s.ldth, s.units);
  return 0;
}

// scratch of chol_big_kernel for NB: BIG_SLOTS workgroups x NB(NB+1)/2 blocks of 2 KiB
constexpr long long BIG_SLOTS = 2048;

// the full factorisation of a segment, by its route (route_for, ewarp_route.h)
int dispatch_chol(DevCtx* h, const Segment& g) {
  switch (route_for(h->plan, h->corr, h->osmode, g.nb, g.src == Source::FixedRun)) {
    case Route::Register: return launch_register(h, g);
    case Route::Big:
      if (const int rc = h->d_bigscr.reserve((size_t)BIG_SLOTS * (g.nb * (g.nb + 1) / 2) * 256, h->hook)) return rc;
      return launch_chol_big_nb(g.nb, g.span, h->d_bigscr.p, BIG_SLOTS);
    case Route::Lds: return launch_lds(g.span, g.mreal);
    case Route::Wide: return launch_wide(h, g.nb, 0, g.span, nullptr);
    case Route::DdVerify:
    case Route::DdAll: return launch_dd_path(h, g.nb, g.span);
    default: return set_err(EWH_E_UNSUPPORTED, "basis wider than 1023 columns");
  }
}

int reserve_units(DevCtx* h, int B) { return h->d_units.reserve(n_units(h, B), h->hook); }

// The varying-WN chunk scratch for a batch of B, and the jobs that point into
// it.  A failed allocation releases the whole group (chunk = 0): the next call
// sizes it again.
int reserve_var_scratch(DevCtx* h, int B) {
  if (h->white_fixed && h->n_delay_psr == 0 && !h->cond_all) return 0;
  DevCtx::VarChunk& v = h->var;
  // reuse while the chunk covers the batch or already sits at its cap (the
  // memory-derived limit, at most 1024): no free / re-malloc per call
  if (v.chunk > 0 && (v.chunk >= B || v.chunk >= h->chunk_cap)) return 0;
  v.release();
  size_t maxn = 1, maxe = 1, maxld = 16, maxfac = 1, maxdn = 0;
  for (auto& ps : h->psr) {
    // (fixed white noise: only the delay pulsars use the chunk scratch, until
    // the conditional GP -- which factors every pulsar's full-width matrix
    // there -- has been called)
    if (h->white_fixed && ps.delay.n_delay == 0 && !h->cond_all) continue;
    if (ps.delay.n_delay > 0) maxdn = std::max(maxdn, (size_t)ps.n_toa);
    maxn = std::max(maxn, (size_t)ps.n_toa);
    maxe = std::max(maxe, (size_t)ps.n_epoch);
    maxld = std::max(maxld, (size_t)ps.ld);
    maxfac = std::max(maxfac, (size_t)ps.n_toa * ps.dev.n_bgroup);
  }
  // chunk: keep G (ld^2) and s (E*ld) scratch under ~1.5 GB (8 GB for wide bases)
  // epoch-sum rows per sample: whole CT_ROWS tiles (+1) so the pipelined
  // contraction's last epoch tile reads zero-initialised pad rows
  const size_t sstride = ((maxe + CT_ROWS - 1) / CT_ROWS + 1) * CT_ROWS * maxld;
  const bool wide = maxld > 16 * BIG_NB_MAX;
  // G_lo for the double-double factorisation: of every unit past 16 blocks,
  // and (round 6) of the units whose fp64 factorisation fails (refine_failed)
  // (+ a delay pulsar's R, Z and residual column)
  const size_t per = (2 * maxld * maxld + sstride + maxn + maxe + maxfac + 1 + 2 * maxdn + 2 * maxld) * sizeof(double);
  // (bases past 16 blocks: 8 GB of the 288 GB HBM, so a batch of up to 1024
  // samples is one chunk -- one GEMM-form contraction over all of it and one
  // factorisation launch with 4 units per CU instead of 4 launches of 256
  // one-wave units)
  const size_t budget = (wide ? (size_t)8192 : (size_t)1536) * 1024 * 1024;
  size_t cap = std::min<size_t>(1024, std::max<size_t>(1, budget / per));
  // whole rounds of workgroups over the 256 CUs (a chunk of 853 samples of
  // C2 ran 2 rounds of 512 workgroups, the second two-thirds empty)
  if (cap > 256) cap -= cap % 256;
  h->chunk_cap = (int)cap;
  const size_t chunk = std::min<size_t>(cap, (size_t)std::max(B, 1));
  const size_t zld = 16 * ((chunk + 15) / 16);
  const Hook hk = h->hook;
  int rc;
  if ((rc = v.d_w.reserve(chunk * maxn, hk)) || (rc = v.d_beta.reserve(chunk * maxe, hk)) ||
      (rc = v.d_s.reserve(chunk * sstride, hk)) || (rc = v.d_G.reserve(chunk * maxld * maxld, hk)) ||
      (rc = v.d_Kb.reserve(chunk, hk)) || (rc = v.d_rho.reserve(chunk, hk)) ||
      (rc = v.d_fac.reserve(chunk * maxfac, hk)) || (rc = v.d_Glo.reserve(chunk * maxld * maxld, hk)) ||
      (maxdn > 0 && ((rc = v.d_dR.reserve(maxdn * zld, hk)) || (rc = v.d_dZ.reserve(maxdn * zld, hk)) ||
                     (rc = v.d_dcol.reserve(chunk * maxld, hk)) || (rc = v.d_dcollo.reserve(chunk * maxld, hk))))) {
    v.release();
    return rc;
  }
  EWH_HIP(hipMemset(v.d_s.p, 0, chunk * sstride * sizeof(double)));
  v.s_stride = (long long)sstride;
  v.chunk = (int)chunk;
  std::vector<CholJob> jobs(h->P);
  for (int p = 0; p < h->P; ++p) {
    const PsrHost& ps = h->psr[p];
    // (correlated: the columns before the common block take phi^-1; the
    // common block is assembled globally)
    const int mreal = h->corr ? ps.gstart_v : ps.m;
    jobs[p] = CholJob{h->var.d_G.p, (long long)ps.ld * ps.ld, ps.ld, mreal, ps.d_colptr, ps.d_spec, h->var.d_Kb.p, 1, 0};
    jobs[p].mats_lo = h->var.d_Glo.p;
  }
  EWH_HIP(hipMemcpy(h->d_jobs_var, jobs.data(), sizeof(CholJob) * h->P, hipMemcpyHostToDevice));
  return 0;
}

// white-noise terms of one pulsar for samples [b0, b0 + nb) into the chunk scratch
int run_white(DevCtx* h, int p, const double* theta, int ldth, int b0, int nb) {
  PsrHost& ps = h->psr[p];
  const bool c2 = ps.dev.n_bgroup == 0 && h->plan.contract2 && ps.nb <= CONTRACT2_NB_MAX;
  // the r-separated contraction (contract2 RSEP): when the residual alone
  // fills the last 16-column block (m <= 16 (NB - 1): C4's 192 columns + r
  // = 13 blocks), the MFMAs form only the NB - 1 block Gram; d = T^T W r by
  // VALU from the staged tiles, r^T W r in wn_weights_kernel.  No ECORR
  // (the epoch pass would need the same split).  KernelPlan::rsep: off (A/B)
  const bool rsep = c2 && ps.dev.n_epoch == 0 && ps.nb >= 2 && ps.dev.m <= 16 * (ps.nb - 1) && h->plan.rsep;
  launch_wn_weights(ps.dev, theta, ldth, b0, nb, h->var.d_w.p, h->var.d_beta.p, h->var.d_Kb.p, h->var.d_fac.p, rsep ? h->var.d_rho.p : nullptr,
                    h->stream);
  if (c2) {
    // (contract2_waves, dev library A/B: 4 / 8 waves per sample; 30: TwoSum
    // accumulation up to 10 blocks; 35: the run remainder on the first waves,
    // as in round 4-5a; 38 / 39: blocked accumulation up to 10 blocks, 4 / 8
    // waves)
    int rc = launch_contract2_nb(ps.nb, h->plan.contract2_waves, ps.dev, h->var.d_w.p, h->var.d_beta.p, h->var.d_s.p, h->var.s_stride,
                                 h->var.d_G.p, nb, h->stream, rsep ? h->var.d_rho.p : nullptr);
    if (rc) return rc;
    EWH_HIP(hipGetLastError());
    return 0;
  }
  // (KernelPlan::epoch_multi off: one sample per workgroup, as in round 5a)
  if (ps.n_epoch > 0)
    launch_epoch_sums(ps.dev, ps.n_epoch, ps.max_epoch, h->plan.epoch_multi, h->var.d_w.p, h->var.d_fac.p, h->var.d_s.p, nb, h->stream);
  int rc = launch_contract_nb(ps.nb, ps.dev, h->var.d_w.p, h->var.d_beta.p, h->var.d_s.p, h->var.d_fac.p, h->var.d_G.p, nb, h->stream,
                              ps.nb > BIG_NB_MAX ? h->var.d_Glo.p : nullptr);
  if (rc) return rc;
  EWH_HIP(hipGetLastError());
  return 0;
}

// A delay pulsar's samples [b0, b0 + nb): the per-sample residual column
// [T_aug^T z; r'^T z], z = N^-1 (r - sum delta), replaces the last row and
// column of the chunk's G slots (delay.hip).  Varying white noise: after
// run_white, from the chunk's w / beta.  Fixed white noise: the cached full-
// width Gram (hi, lo) and -1/2 log|N| are broadcast into the slots first, w /
// beta are the cached ones.  No allocation, no synchronisation (graph capture).
int run_delay(DevCtx* h, int p, const double* theta, int ldth, int b0, int nb) {
  PsrHost& ps = h->psr[p];
  const bool fx = h->white_fixed;
  if (fx)
    launch_gram_broadcast(ps.d_Gf, ps.d_Gflo, (long long)ps.ld * ps.ld, ps.fxKb, nb, h->var.d_G.p, h->var.d_Glo.p, h->var.d_Kb.p,
                          h->stream);
  const int rc = launch_delay_column(ps.dev, ps.delay, theta, ldth, b0, nb, fx ? ps.d_wf : h->var.d_w.p,
                                     fx ? 0 : ps.n_toa, fx ? ps.d_betaf : h->var.d_beta.p, fx ? 0 : ps.n_epoch, h->var.d_fac.p,
                                     h->var.d_dR.p, h->var.d_dZ.p, h->var.d_dcol.p, h->var.d_dcollo.p, h->var.d_Kb.p, h->stream);
  if (rc) return rc;
  // (G_lo where a factorisation reads it: the broadcast one, and the wide
  // contraction's past 16 blocks)
  launch_delay_scatter(ps.ld, nb, h->var.d_dcol.p, h->var.d_dcollo.p, h->var.d_G.p, fx || ps.nb > BIG_NB_MAX ? h->var.d_Glo.p : nullptr,
                       h->stream);
  EWH_HIP(hipGetLastError());
  return 0;
}

// per-chunk scratch of the dense cross-pulsar factorisation, sized to
// min(B, cap) on first use and grown (up to the cap) when a larger batch comes
// (a failed allocation releases the whole group, cchunk = 0)
int reserve_common_scratch(DevCtx* h, int B) {
  DevCtx::CorrChunk& c = h->cor;
  const int want = std::min(std::max(B, 1), h->cchunk_cap);
  if (c.cchunk >= want) return 0;
  c.release();
  const size_t Bc = want, P = h->P;
  const Hook hk = h->hook;
  int rc;
  if ((rc = c.d_minv.reserve(Bc * h->nc * P * P, hk)) || (rc = c.d_mlog.reserve(Bc * h->nc, hk)) ||
      (rc = c.d_dense.reserve(Bc * h->Np * h->Np, hk)) || (rc = c.d_wbuf.reserve(Bc * DCB * DCB, hk)) ||
      (rc = c.d_cldet.reserve(Bc, hk)) || (rc = c.d_cq.reserve(Bc, hk)) || (rc = c.d_cfail.reserve(Bc, hk))) {
    c.release();
    return rc;
  }
  c.cchunk = want;
  return 0;
}

int reserve_keep(DevCtx* h, int B) {
  const size_t KD = 16 * h->keep;
  return h->d_keep.reserve((size_t)B * h->P * KD * KD, h->hook);
}

// h->stream = st (run_white and run_delay launch there) until the scope ends
struct StreamScope {
  DevCtx* h;
  hipStream_t saved;
  StreamScope(DevCtx* h_, hipStream_t st) : h(h_), saved(h_->stream) { h->stream = st; }
  ~StreamScope() { h->stream = saved; }
};

// Step 1 of a correlated batch for pulsars [p_begin, p_end): the partial
// factorisations (own columns eliminated), writing each unit's local term to
// units[p B + b] and its kept common block to keep (pulsar-major, B samples
// per pulsar).
int corr_partial(DevCtx* h, const double* theta_dev, int B, int p_begin, int p_end, double* units, double* keep,
                 hipStream_t st) {
  // white noise varying: per pulsar and sample chunk the contraction
  // (run_white: N^-1, ECORR, G = T_aug^T N^-1 T_aug on h->stream) and the
  // partial factorisation of G + diag(phi^-1) with the timing model in
  if (!h->white_fixed)
    if (const int rc = reserve_var_scratch(h, B)) return rc;
  StreamScope on_st(h, st);   // (with fixed white noise too: nothing on that path reads h->stream)
  const UnitSpan all{nullptr, B, (long long)p_begin * B, (long long)(p_end - p_begin) * B, 0, theta_dev, h->n_param, units, st};
  return for_segments(h, all, [&](const Segment& g) {
    if (g.src == Source::Varying)
      if (const int rc = run_white(h, g.p0, theta_dev, h->n_param, g.span.b_off, (int)g.span.n)) return rc;
    return partial_units(h, g.nb, g.span, keep);
  });
}

// Step 2, once every pulsar's kept block is in `keep`: per sample chunk the
// M_g inverses, the dense Sigma_c assembly and factorisation; the global term
// of sample b goes to units[P B + b].
// the M_g inverses and log-determinants of samples [c0, c0 + nb)
void minv_chunk(DevCtx* h, const double* theta_dev, int c0, int nb, hipStream_t st) {
  launch_minv(h->d_cps, h->P, h->d_orf, h->d_cspec, h->cterms, h->nc, h->d_cuniq, h->nuniq, theta_dev, h->n_param, c0,
              nb, h->cor.d_minv.p, h->cor.d_mlog.p, h->plan, st);
}

// first_minv_done: the M_g inverses of the first chunk are already in
// d_minv (lnl_correlated ran them beside the partial factorisations)
int corr_finish(DevCtx* h, const double* theta_dev, int B, const double* keep, double* units, hipStream_t st,
                bool first_minv_done = false) {
  int rc;
  if ((rc = reserve_common_scratch(h, B))) return rc;
  for (int c0 = 0; c0 < B; c0 += h->cor.cchunk) {
    const int nb = std::min(h->cor.cchunk, B - c0);
    if (!(first_minv_done && c0 == 0)) minv_chunk(h, theta_dev, c0, nb, st);
    launch_common_chunk(keep, 16 * h->keep, h->P, h->nc, B, c0, nb, h->cor.d_minv.p, h->cor.d_mlog.p, h->d_crep, h->Np, h->cor.d_dense.p,
                        h->cor.d_wbuf.p, h->cor.d_cldet.p, h->cor.d_cq.p, h->cor.d_cfail.p, units, h->plan, st);
    EWH_HIP(hipGetLastError());
  }
  return 0;
}

// correlated batch on one device: step 1 for every pulsar, then step 2
int lnl_correlated(DevCtx* h, const double* theta_dev, int B, hipStream_t st) {
  int rc;
  if ((rc = reserve_keep(h, B)) || (rc = reserve_common_scratch(h, B))) return rc;
  // the first chunk's M_g inverses depend on theta only: they run on the
  // side stream while the partial factorisations run on st (forked after
  // whatever st produced theta with; joined before the assembly)
  // (large chunks only: for one proposal the fork / join costs more than the
  // overlap gains -- B = 1: 1.61 vs 1.49 ms)
  const bool overlap = minv_in_registers(h->P, h->plan) && B >= 64;
  if (overlap) {
    if (!h->side) {
      EWH_HIP(hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking));
      EWH_HIP(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
      EWH_HIP(hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming));
    }
    EWH_HIP(hipEventRecord(h->ev_fork, st));
    EWH_HIP(hipStreamWaitEvent(h->side, h->ev_fork, 0));
    minv_chunk(h, theta_dev, 0, std::min(h->cor.cchunk, B), h->side);
    EWH_HIP(hipEventRecord(h->ev_join, h->side));
  }
  if ((rc = corr_partial(h, theta_dev, B, 0, h->P, h->d_units.p, h->d_keep.p, st))) return rc;
  if (overlap) EWH_HIP(hipStreamWaitEvent(st, h->ev_join, 0));
  return corr_finish(h, theta_dev, B, h->d_keep.p, h->d_units.p, st, overlap);
}

// lnL terms of units [u_begin, u_end) (u = pulsar * B + sample) into h->d_units
// (rows outside the range zeroed); reduce: also out_dev[b] = sum over the rows.
int ctx_units(DevCtx* h, const double* theta_dev, int B, int64_t u_begin, int64_t u_end, double* out_dev,
              hipStream_t st, bool reduce) {
  const long long U = (long long)h->P * B;
  u_begin = std::max<int64_t>(0, u_begin);
  u_end = std::min<int64_t>(U, u_end);
  EWH_HIP(hipSetDevice(h->device));
  int rc;
  if ((rc = reserve_units(h, B))) return rc;
  const int rows = h->P + (h->corr ? 1 : 0);
  EWH_HIP(hipMemsetAsync(h->d_units.p, 0, sizeof(double) * (size_t)rows * B, st));
  StreamScope on_st(h, st);
  if (h->corr) {
    if (u_begin != 0 || u_end != U)
      return set_err(EWH_E_UNSUPPORTED, "correlated common process: pass the whole batch (shard samples, not units)");
    if ((rc = lnl_correlated(h, theta_dev, B, st))) return rc;
  } else {
    if ((rc = reserve_var_scratch(h, B))) return rc;
    const UnitSpan all{nullptr, B, u_begin, u_end - u_begin, 0, theta_dev, h->n_param, h->d_units.p, st};
    rc = for_segments(h, all, [&](const Segment& g) {
      // the segment's matrices where they are per sample: the contraction
      // (varying white noise), a delay pulsar's residual column
      const PsrHost& ps = h->psr[g.p0];
      const UnitSpan& s = g.span;
      int rc = 0;
      if (g.src == Source::Varying && (rc = run_white(h, g.p0, s.theta, s.ldth, s.b_off, (int)s.n))) return rc;
      if (g.src != Source::FixedRun && ps.delay.n_delay > 0 &&
          (rc = run_delay(h, g.p0, s.theta, s.ldth, s.b_off, (int)s.n)))
        return rc;
      if ((rc = dispatch_chol(h, g))) return rc;
      if (refine_after(g.src, g.nb, ps.dev.n_bgroup > 0, h->plan, h->corr, h->osmode)) rc = refine_failed(h, g);
      return rc;
    });
    if (rc) return rc;
  }
  if (reduce)
    hipLaunchKernelGGL(reduce_units_kernel, dim3((B + 255) / 256), dim3(256), 0, st, h->d_units.p, rows, B, out_dev);
  EWH_HIP(hipGetLastError());
  h->last_B = B;
  return 0;
}

// device theta / out buffers of one context, grown as needed
int reserve_io(DevCtx* h, int B) {
  const size_t nth = (size_t)B * std::max(1, h->n_param);
  const int rc = h->d_theta.reserve(nth + B, h->hook);
  h->d_out = rc ? nullptr : h->d_theta.p + nth;
  return rc;
}

// Cost-balanced contiguous unit ranges (the same rule as
// enterprise_warp_amd.sharding.unit_ranges).
std::vector<std::pair<long long, long long>> unit_ranges(const std::vector<double>& cost, int B, int world) {
  const int P = (int)cost.size();
  std::vector<std::pair<long long, long long>> out;
  if (world <= 1) {
    out.push_back({0, (long long)P * B});
    return out;
  }
  std::vector<double> cum(P + 1, 0.0);
  for (int p = 0; p < P; ++p) cum[p + 1] = cum[p] + cost[p] * B;
  std::vector<long long> bounds{0};
  for (int r = 1; r < world; ++r) {
    const double target = cum[P] * r / world;
    int p = (int)(std::upper_bound(cum.begin(), cum.end(), target) - cum.begin()) - 1;
    p = std::min(std::max(p, 0), P - 1);
    const double within = cost[p] > 0 ? (target - cum[p]) / cost[p] : 0.0;
    long long u = (long long)p * B + (long long)std::llround(within);
    u = std::min<long long>(std::max<long long>(u, bounds.back()), (long long)P * B);
    bounds.push_back(u);
  }
  bounds.push_back((long long)P * B);
  for (int i = 0; i < world; ++i) out.push_back({bounds[i], bounds[i + 1]});
  return out;
}

int ctx_optstat(DevCtx* h, const double* theta_host, int32_t B, const double* phihat_host, double* rho_host,
                double* sig_host, double* os_host, double* os_sig_host) {
  if (!h || !theta_host || !phihat_host || !os_host || !os_sig_host || B <= 0)
    return set_err(EWH_E_INVALID, "bad arguments");
  if (!h->osmode) return set_err(EWH_E_INVALID, "handle was not created with common->kind = EWH_COMMON_OPTSTAT");
  EWH_HIP(hipSetDevice(h->device));
  const int P = h->P, nc = h->nc, KD = 16 * h->keep, np = std::max(1, h->n_param);
  hipStream_t st = h->stream;
  int rc;
  double *th, *ph, *xh, *wh, *rho, *sig, *os;
  Arena tmp(h->hook);           // this call's buffers, freed on return
  if ((rc = tmp.alloc(&th, (size_t)B * np)) || (rc = tmp.alloc(&ph, (size_t)B * nc)) ||
      (rc = tmp.alloc(&xh, (size_t)B * P * nc)) || (rc = tmp.alloc(&wh, (size_t)B * P * nc * nc)) ||
      (rc = tmp.alloc(&rho, (size_t)B * P * P)) || (rc = tmp.alloc(&sig, (size_t)B * P * P)) ||
      (rc = tmp.alloc(&os, 2 * (size_t)B)))
    return rc;
  if (h->n_param > 0)
    EWH_HIP(hipMemcpyAsync(th, theta_host, sizeof(double) * (size_t)B * h->n_param, hipMemcpyHostToDevice, st));
  EWH_HIP(hipMemcpyAsync(ph, phihat_host, sizeof(double) * (size_t)B * nc, hipMemcpyHostToDevice, st));
  EWH_HIP(hipMemsetAsync(rho, 0, sizeof(double) * (size_t)B * P * P, st));
  EWH_HIP(hipMemsetAsync(sig, 0, sizeof(double) * (size_t)B * P * P, st));
  if ((rc = reserve_units(h, B)) || (rc = reserve_keep(h, B))) return rc;
  const long long U = (long long)P * B;
  // per-pulsar factorisations, common block kept
  const UnitSpan all{nullptr, B, 0, U, 0, th, h->n_param, h->d_units.p, st};
  if ((rc = for_segments(h, all, [&](const Segment& g) { return partial_units(h, g.nb, g.span, h->d_keep.p); })))
    return rc;
  launch_optstat(h->d_keep.p, KD, P, nc, h->d_cps, th, h->n_param, ph, xh, wh, B, rho, sig, h->d_orf, os, os + B, st);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && rho_host)
    e = hipMemcpyAsync(rho_host, rho, sizeof(double) * (size_t)B * P * P, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && sig_host)
    e = hipMemcpyAsync(sig_host, sig, sizeof(double) * (size_t)B * P * P, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(os_host, os, sizeof(double) * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(os_sig_host, os + B, sizeof(double) * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return set_err(EWH_E_HIP, std::string("ewh_optstat: ") + hipGetErrorString(e));
  return 0;
}

// The first conditional call on a context (ewh_cond_gp, ewh_cond_joint): from
// now on the chunk scratch covers every pulsar and a fixed-white-noise handle
// keeps every full-width Gram (the code create runs, again; S and K are
// recomputed to the same bits)
int ensure_cond_all(DevCtx* h) {
  if (h->cond_all) return 0;
  drop_graphs(h);
  EWH_HIP(hipStreamSynchronize(h->stream));
  h->cond_all = true;
  if (h->white_fixed) {
    h->var.release();
    if (const int rc = setup_fixed(h)) return rc;
  }
  return 0;
}

// The conditional GP of every pulsar for B samples (include/ewarp_hip.h,
// ewh_cond_gp) on one context, chunk by chunk: per chunk theta goes up once,
// then per pulsar the matrix route fills the chunk's G slots -- run_white (+
// run_delay) with varying white noise, the broadcast of the cached full-width
// Gram (run_delay for a delay pulsar) with fixed -- cond_solve factors and
// solves in place, cond_pack maps back to the caller's basis and cond_process
// forms the realisations; the results leave by strided copies into the
// caller's arrays.  Everything is on h->stream; each pulsar's step ends with a
// stream synchronisation (the staging buffers are reused).
int ctx_cond_gp(DevCtx* h, const double* theta_host, int B, const double* z_host, int n_group,
                const int32_t* col_group, double* coef_host, double* proc_host, int32_t* status_host,
                long long n_coef, long long n_toa_total) {
  EWH_HIP(hipSetDevice(h->device));
  int rc;
  if ((rc = ensure_cond_all(h)) || (rc = reserve_var_scratch(h, B))) return rc;
  const int chunk = h->var.chunk, np = std::max(1, h->n_param);
  size_t maxm = 1, maxld = 16, maxn = 1;
  for (const auto& ps : h->psr) {
    maxm = std::max(maxm, (size_t)ps.m);
    maxld = std::max(maxld, (size_t)ps.ld);
    maxn = std::max(maxn, (size_t)ps.n_toa);
  }
  const int cb = std::min(chunk, B);
  const size_t ldv_max = 16 * (((size_t)cb * std::max(1, n_group) + 15) / 16);
  DevCtx::CondChunk& c = h->cond;
  const Hook hk = h->hook;
  if ((rc = c.d_theta.reserve((size_t)cb * np, hk)) || (rc = c.d_z.reserve((size_t)cb * maxm, hk)) ||
      (rc = c.d_x.reserve((size_t)cb * maxld, hk)) || (rc = c.d_coef.reserve((size_t)cb * maxm, hk)) ||
      (rc = c.d_status.reserve((size_t)cb, hk)) || (rc = c.d_grp.reserve((size_t)std::max<long long>(1, n_coef), hk)) ||
      (n_group > 0 && ((rc = c.d_V.reserve(maxld * ldv_max, hk)) || (rc = c.d_Y.reserve(ldv_max * maxn, hk)))))
    return rc;
  hipStream_t st = h->stream;
  if (n_group > 0)
    EWH_HIP(hipMemcpyAsync(c.d_grp.p, col_group, sizeof(int) * (size_t)n_coef, hipMemcpyHostToDevice, st));
  for (int c0 = 0; c0 < B; c0 += chunk) {
    const int nb = std::min(chunk, B - c0);
    if (h->n_param > 0)
      EWH_HIP(hipMemcpyAsync(c.d_theta.p, theta_host + (size_t)c0 * h->n_param, sizeof(double) * (size_t)nb * h->n_param,
                             hipMemcpyHostToDevice, st));
    const int ldth = h->n_param;
    long long coff = 0, toff = 0;
    for (int p = 0; p < h->P; ++p) {
      PsrHost& ps = h->psr[p];
      const bool delay = ps.delay.n_delay > 0;
      if (!h->white_fixed) {
        if ((rc = run_white(h, p, c.d_theta.p, ldth, 0, nb))) return rc;
        if (delay && (rc = run_delay(h, p, c.d_theta.p, ldth, 0, nb))) return rc;
      } else if (delay) {
        if ((rc = run_delay(h, p, c.d_theta.p, ldth, 0, nb))) return rc;
      } else {
        launch_gram_broadcast(ps.d_Gf, ps.d_Gflo, (long long)ps.ld * ps.ld, ps.fxKb, nb, h->var.d_G.p, h->var.d_Glo.p,
                              h->var.d_Kb.p, st);
        EWH_HIP(hipGetLastError());
      }
      if (z_host)
        EWH_HIP(hipMemcpy2DAsync(c.d_z.p, sizeof(double) * ps.m, z_host + (size_t)c0 * n_coef + coff,
                                 sizeof(double) * (size_t)n_coef, sizeof(double) * ps.m, (size_t)nb,
                                 hipMemcpyHostToDevice, st));
      if ((rc = launch_cond_solve(h->var.d_G.p, ps.ld, ps.m, ps.d_colptr, ps.d_spec, c.d_theta.p, ldth, h->var.d_Kb.p,
                                  delay, z_host ? c.d_z.p : nullptr, nb, c.d_x.p, c.d_status.p, st)))
        return rc;
      const int nout = nb * n_group, ldv = 16 * ((nout + 15) / 16);
      if (n_group > 0) EWH_HIP(hipMemsetAsync(c.d_V.p, 0, sizeof(double) * (size_t)ps.ld * ldv, st));
      if ((rc = launch_cond_pack(c.d_x.p, ps.ld, ps.m, ps.has_proj ? ps.nlead : 0, ps.has_proj ? ps.nproj : 0,
                                 ps.d_projcols, ps.d_projC, c.d_status.p, n_group > 0 ? c.d_grp.p + coff : nullptr,
                                 n_group, nb, c.d_coef.p, c.d_V.p, ldv, st)))
        return rc;
      if (n_group > 0) {
        if ((rc = launch_cond_process(ps.dev, h->var.d_fac.p, c.d_V.p, ldv, n_group, nout, c.d_Y.p, st))) return rc;
        EWH_HIP(hipMemcpy2DAsync(proc_host + (size_t)c0 * n_group * n_toa_total + toff,
                                 sizeof(double) * (size_t)n_toa_total, c.d_Y.p, sizeof(double) * ps.n_toa,
                                 sizeof(double) * ps.n_toa, (size_t)nout, hipMemcpyDeviceToHost, st));
      }
      if (coef_host)
        EWH_HIP(hipMemcpy2DAsync(coef_host + (size_t)c0 * n_coef + coff, sizeof(double) * (size_t)n_coef, c.d_coef.p,
                                 sizeof(double) * ps.m, sizeof(double) * ps.m, (size_t)nb, hipMemcpyDeviceToHost, st));
      if (status_host)
        EWH_HIP(hipMemcpyAsync(status_host + (size_t)p * B + c0, c.d_status.p, sizeof(int) * (size_t)nb,
                               hipMemcpyDeviceToHost, st));
      EWH_HIP(hipStreamSynchronize(st));
      coff += ps.m;
      toff += ps.n_toa;
    }
  }
  return 0;
}

// bytes of retained factors (L_A, W: ld^2 per unit) one chunk may hold
constexpr size_t JOINT_RETAIN_BYTES = (size_t)4 << 30;

// The joint conditional GP of a correlated handle for B samples
// (include/ewarp_hip.h, ewh_cond_joint; cond_joint.hip) on one context.  The
// chunk is the smallest of the varying-WN chunk, the dense Sigma_c chunk, what
// JOINT_RETAIN_BYTES of retained factors allow, and the caller's max_chunk.
// Per chunk: theta (and z) go up once and the M_g inverses are formed; pass 1
// over the pulsars fills the chunk's G slots by the matrix route of
// ctx_cond_gp, runs the partial stage and copies the factored slots to the
// retained buffer; then Sigma_c is assembled and solved; pass 2 over the
// pulsars substitutes back, maps to the caller's basis (cond_pack), forms the
// realisations (cond_process) and copies out.  Everything is on h->stream;
// each pulsar's step of pass 2 ends with a stream synchronisation.  A failed
// allocation releases both scratch groups (joint, cond).
int ctx_cond_joint(DevCtx* h, const double* theta_host, int B, const double* z_host, int n_group,
                   const int32_t* col_group, double* coef_host, double* proc_host, int32_t* status_host, int max_chunk,
                   long long n_coef, long long n_toa_total) {
  EWH_HIP(hipSetDevice(h->device));
  const int P = h->P, nc = h->nc, np = std::max(1, h->n_param);
  if ((long long)P * nc > COND_JOINT_NC_MAX)
    return set_err(EWH_E_UNSUPPORTED, "ewh_cond_joint: Sigma_c of " + std::to_string((long long)P * nc) +
                                          " columns; the dense solve takes at most " + std::to_string(COND_JOINT_NC_MAX));
  int rc;
  if ((rc = ensure_cond_all(h))) return rc;
  const size_t Npad = (size_t)cond_joint_npad(P, nc);
  size_t maxm = 1, maxld = 16, maxn = 1, sumld2 = 0, summ = 0;
  for (const auto& ps : h->psr) {
    if (ps.delay.n_delay > 0) return set_err(EWH_E_UNSUPPORTED, "ewh_cond_joint: deterministic delays");
    maxm = std::max(maxm, (size_t)ps.m);
    maxld = std::max(maxld, (size_t)ps.ld);
    maxn = std::max(maxn, (size_t)ps.n_toa);
    sumld2 += (size_t)ps.ld * ps.ld;
    summ += (size_t)ps.m;
  }
  size_t want = std::min<size_t>((size_t)B, std::max<size_t>(1, JOINT_RETAIN_BYTES / (sizeof(double) * sumld2)));
  if (max_chunk > 0) want = std::min(want, (size_t)max_chunk);
  if ((rc = reserve_var_scratch(h, (int)want)) || (rc = reserve_common_scratch(h, (int)want))) return rc;
  const int chunk = (int)std::min({want, (size_t)h->var.chunk, (size_t)h->cor.cchunk});
  const size_t sblk = (size_t)(nc + 1) * nc;
  const size_t ldv_max = 16 * (((size_t)chunk * std::max(1, n_group) + 15) / 16);
  DevCtx::CondChunk& c = h->cond;
  DevCtx::JointChunk& jc = h->joint;
  const Hook hk = h->hook;
  if ((rc = jc.d_L.reserve((size_t)chunk * sumld2, hk)) || (rc = jc.d_S.reserve((size_t)P * chunk * sblk, hk)) ||
      (rc = jc.d_rhs.reserve((size_t)chunk * Npad, hk)) || (rc = jc.d_xc.reserve((size_t)chunk * Npad, hk)) ||
      (z_host && (rc = jc.d_z.reserve((size_t)chunk * n_coef, hk))) ||
      (rc = jc.d_pstat.reserve((size_t)P * chunk, hk)) || (rc = jc.d_sfail.reserve((size_t)chunk, hk)) ||
      (rc = jc.d_cstart.reserve((size_t)P, hk)) || (rc = jc.d_grp.reserve(summ, hk))) {
    jc.release();
    return rc;
  }
  if ((rc = c.d_theta.reserve((size_t)chunk * np, hk)) || (rc = c.d_x.reserve((size_t)chunk * maxld, hk)) ||
      (rc = c.d_coef.reserve((size_t)chunk * maxm, hk)) || (rc = c.d_status.reserve((size_t)chunk, hk)) ||
      (n_group > 0 && ((rc = c.d_V.reserve(maxld * ldv_max, hk)) || (rc = c.d_Y.reserve(ldv_max * maxn, hk))))) {
    c.release();
    jc.release();
    return rc;
  }
  // per pulsar: descriptor columns, own columns that take a normal, the own
  // block's width in the slot (varying white noise: up to the aligned common
  // block, inner pads included)
  std::vector<int> ncol(P), nlo(P), mo(P), cstart(P), grp(summ, -1);
  {
    long long coff = 0;
    size_t goff = 0;
    for (int p = 0; p < P; ++p) {
      const PsrHost& ps = h->psr[p];
      ncol[p] = ps.nlead + ps.fx_m;
      nlo[p] = ncol[p] - nc;
      mo[p] = h->white_fixed ? nlo[p] : ps.gstart_v;
      cstart[p] = (int)(coff + nlo[p]);
      if (nlo[p] < 1 || mo[p] + nc != ps.m) return set_err(EWH_E_UNSUPPORTED, "ewh_cond_joint: a pulsar whose every column is the common process's (no own block)");
      for (int j = 0; n_group > 0 && j < ncol[p]; ++j)
        grp[goff + (j < nlo[p] ? j : mo[p] + (j - nlo[p]))] = col_group[coff + j];
      coff += ncol[p];
      goff += (size_t)ps.m;
    }
  }
  EWH_HIP(hipMemcpy(jc.d_cstart.p, cstart.data(), sizeof(int) * (size_t)P, hipMemcpyHostToDevice));
  if (n_group > 0) EWH_HIP(hipMemcpy(jc.d_grp.p, grp.data(), sizeof(int) * summ, hipMemcpyHostToDevice));
  hipStream_t st = h->stream;
  const int ldth = h->n_param;
  for (int c0 = 0; c0 < B; c0 += chunk) {
    const int nb = std::min(chunk, B - c0);
    if (h->n_param > 0)
      EWH_HIP(hipMemcpyAsync(c.d_theta.p, theta_host + (size_t)c0 * h->n_param, sizeof(double) * (size_t)nb * h->n_param,
                             hipMemcpyHostToDevice, st));
    if (z_host)
      EWH_HIP(hipMemcpyAsync(jc.d_z.p, z_host + (size_t)c0 * n_coef, sizeof(double) * (size_t)nb * n_coef,
                             hipMemcpyHostToDevice, st));
    minv_chunk(h, c.d_theta.p, 0, nb, st);
    EWH_HIP(hipGetLastError());
    // pass 1: the own blocks
    size_t loff = 0;
    for (int p = 0; p < P; ++p) {
      PsrHost& ps = h->psr[p];
      const size_t ld2 = (size_t)ps.ld * ps.ld;
      if (!h->white_fixed) {
        if ((rc = run_white(h, p, c.d_theta.p, ldth, 0, nb))) return rc;
      } else {
        launch_gram_broadcast(ps.d_Gf, ps.d_Gflo, (long long)ld2, ps.fxKb, nb, h->var.d_G.p, h->var.d_Glo.p, h->var.d_Kb.p, st);
        EWH_HIP(hipGetLastError());
      }
      if ((rc = launch_cond_joint_partial(h->var.d_G.p, ps.ld, mo[p], nc, ps.d_colptr, ps.d_spec, c.d_theta.p, ldth, nb,
                                          jc.d_S.p + (size_t)p * chunk * sblk, jc.d_pstat.p + (size_t)p * chunk, st)))
        return rc;
      EWH_HIP(hipMemcpyAsync(jc.d_L.p + loff, h->var.d_G.p, sizeof(double) * (size_t)nb * ld2, hipMemcpyDeviceToDevice, st));
      loff += (size_t)chunk * ld2;
    }
    // Sigma_c
    if ((rc = launch_cond_joint_dense(jc.d_S.p, chunk, P, nc, nb, jc.d_pstat.p, h->cor.d_minv.p, h->cor.d_mlog.p, h->d_crep,
                                      h->cor.d_dense.p, jc.d_rhs.p, z_host ? jc.d_z.p : nullptr, n_coef, jc.d_cstart.p,
                                      jc.d_sfail.p, jc.d_xc.p, st)))
      return rc;
    // pass 2: back-substitution, the caller's basis, the realisations
    long long coff = 0, toff = 0;
    size_t goff = 0;
    loff = 0;
    for (int p = 0; p < P; ++p) {
      PsrHost& ps = h->psr[p];
      if ((rc = launch_cond_joint_back(jc.d_L.p + loff, ps.ld, mo[p], nc, nlo[p], jc.d_xc.p, (int)Npad, p * nc,
                                       z_host ? jc.d_z.p : nullptr, n_coef, coff, jc.d_pstat.p + (size_t)p * chunk,
                                       jc.d_sfail.p, nb, c.d_x.p, c.d_status.p, st)))
        return rc;
      const int nout = nb * n_group, ldv = 16 * ((nout + 15) / 16);
      if (n_group > 0) EWH_HIP(hipMemsetAsync(c.d_V.p, 0, sizeof(double) * (size_t)ps.ld * ldv, st));
      if ((rc = launch_cond_pack(c.d_x.p, ps.ld, ps.m, ps.has_proj ? ps.nlead : 0, ps.has_proj ? ps.nproj : 0,
                                 ps.d_projcols, ps.d_projC, c.d_status.p, n_group > 0 ? jc.d_grp.p + goff : nullptr,
                                 n_group, nb, c.d_coef.p, c.d_V.p, ldv, st)))
        return rc;
      if (n_group > 0) {
        // (a theta-dependent basis: this pulsar's chromatic factors of the chunk, again)
        if (ps.dev.n_bgroup > 0)
          launch_wn_weights(ps.dev, c.d_theta.p, ldth, 0, nb, h->var.d_w.p, h->var.d_beta.p, h->var.d_Kb.p, h->var.d_fac.p,
                            nullptr, st);
        if ((rc = launch_cond_process(ps.dev, h->var.d_fac.p, c.d_V.p, ldv, n_group, nout, c.d_Y.p, st))) return rc;
        EWH_HIP(hipMemcpy2DAsync(proc_host + (size_t)c0 * n_group * n_toa_total + toff,
                                 sizeof(double) * (size_t)n_toa_total, c.d_Y.p, sizeof(double) * ps.n_toa,
                                 sizeof(double) * ps.n_toa, (size_t)nout, hipMemcpyDeviceToHost, st));
      }
      if (coef_host) {
        // (descriptor order: the own columns, then the common block from its slot position)
        double* dst = coef_host + (size_t)c0 * n_coef + coff;
        EWH_HIP(hipMemcpy2DAsync(dst, sizeof(double) * (size_t)n_coef, c.d_coef.p, sizeof(double) * ps.m,
                                 sizeof(double) * nlo[p], (size_t)nb, hipMemcpyDeviceToHost, st));
        EWH_HIP(hipMemcpy2DAsync(dst + nlo[p], sizeof(double) * (size_t)n_coef, c.d_coef.p + mo[p], sizeof(double) * ps.m,
                                 sizeof(double) * nc, (size_t)nb, hipMemcpyDeviceToHost, st));
      }
      if (status_host)
        EWH_HIP(hipMemcpyAsync(status_host + (size_t)p * B + c0, c.d_status.p, sizeof(int) * (size_t)nb,
                               hipMemcpyDeviceToHost, st));
      EWH_HIP(hipStreamSynchronize(st));
      coff += ncol[p];
      toff += ps.n_toa;
      goff += (size_t)ps.m;
      loff += (size_t)chunk * (size_t)ps.ld * ps.ld;
    }
  }
  return 0;
}

double ctx_unit_cost(const DevCtx* h, int p) {
  const PsrHost& ps = h->psr[p];
  // (a delay pulsar with fixed white noise: the Gram broadcast, the column
  // GEMM over the TOAs and the full-width factorisation)
  if (h->white_fixed && ps.delay.n_delay > 0)
    return 2.0 * ps.ld * ps.ld + 2.0 * (double)ps.n_toa * ps.ld + (double)ps.ld * ps.ld * ps.ld / 3.0;
  if (h->white_fixed) return (double)ps.fx_ld * ps.fx_ld * ps.fx_ld / 3.0;
  return (double)ps.n_toa * ps.ld * ps.ld + (double)ps.ld * ps.ld * ps.ld / 3.0 +
         (ps.delay.n_delay > 0 ? 2.0 * (double)ps.n_toa * ps.ld : 0.0);
}

// Peer access is process-global state.  Handles share it by reference count:
// a direction (from, to) a handle enabled, or found enabled by another
// handle, is counted; the last handle to release it disables it.  A direction
// that was already on when no handle held it (the caller's own) is never
// counted, so never turned off here.
std::mutex g_peer_mu;
std::map<std::pair<int, int>, int> g_peer_refs;

bool peer_acquire(ewh_handle* H, int from, int to) {
  std::lock_guard<std::mutex> lk(g_peer_mu);
  if (hipSetDevice(from) != hipSuccess) return false;
  const hipError_t e = hipDeviceEnablePeerAccess(to, 0);
  (void)hipGetLastError();
  const auto key = std::make_pair(from, to);
  auto it = g_peer_refs.find(key);
  if (e == hipSuccess || (e == hipErrorPeerAccessAlreadyEnabled && it != g_peer_refs.end())) {
    ++g_peer_refs[key];
    H->peer_held.push_back(key);
    return true;
  }
  return e == hipErrorPeerAccessAlreadyEnabled;   // on outside any handle: usable, not ours
}

void peer_release_all(ewh_handle* H) {
  std::lock_guard<std::mutex> lk(g_peer_mu);
  for (const auto& key : H->peer_held) {
    auto it = g_peer_refs.find(key);
    if (it == g_peer_refs.end()) continue;
    if (--it->second == 0) {
      g_peer_refs.erase(it);
      if (hipSetDevice(key.first) == hipSuccess) (void)hipDeviceDisablePeerAccess(key.second);
      (void)hipGetLastError();
    }
  }
  H->peer_held.clear();
}

// enqueue one single-context batch on h->stream: H2D of theta from the pinned
// staging, the unit launches + reduction, D2H of lnL into the pinned staging
int enqueue_single(ewh_handle* H, DevCtx* h, int B) {
  const int np = H->n_param;
  int rc;
  if (np > 0)
    EWH_HIP(hipMemcpyAsync(h->d_theta.p, H->h_theta.p, sizeof(double) * (size_t)B * np, hipMemcpyHostToDevice,
                           h->stream));
  if ((rc = ctx_units(h, h->d_theta.p, B, 0, (long long)H->P * B, h->d_out, h->stream, true))) return rc;
  EWH_HIP(hipMemcpyAsync(H->h_out.p, h->d_out, sizeof(double) * B, hipMemcpyDeviceToHost, h->stream));
  return 0;
}

constexpr size_t GRAPH_CACHE = 8;

// Theta of one context's unit range [a, b) (u = pulsar * B + sample): per
// column, the sample rows its pulsars read (the union of their row ranges);
// columns with the same rows form one segment.  Packed into pinned memory,
// copied to the device and scattered into h->d_theta (full layout) on
// h->stream.  Returns the payload bytes (or a negative error code).
long long stage_theta_range(ewh_handle* H, DevCtx* h, const double* theta_host, int B, long long a, long long b) {
  const int np = H->n_param;
  if (b <= a || np <= 0) return 0;
  std::map<int, std::pair<int, int>> rows;                 // column -> [lo, hi)
  const int p0 = (int)(a / B), p1 = (int)((b - 1) / B);
  for (int p = p0; p <= p1; ++p) {
    const int lo = p == p0 ? (int)(a % B) : 0, hi = p == p1 ? (int)((b - 1) % B) + 1 : B;
    for (int c : H->psr_cols[p]) {
      auto it = rows.find(c);
      if (it == rows.end()) rows.emplace(c, std::make_pair(lo, hi));
      else it->second = {std::min(it->second.first, lo), std::max(it->second.second, hi)};
    }
  }
  std::map<std::pair<int, int>, std::vector<int>> segs;
  for (auto& kv : rows) segs[kv.second].push_back(kv.first);
  const int nseg = (int)segs.size();
  if (nseg == 0) return 0;
  size_t ncolsum = 0, payload = 0;
  for (auto& kv : segs) {
    ncolsum += kv.second.size();
    payload += (size_t)(kv.first.second - kv.first.first) * kv.second.size();
  }
  int rc;
  if ((rc = h->h_stage.reserve(payload)) || (rc = h->h_seg.reserve(5 * (size_t)nseg + ncolsum)) ||
      (rc = h->d_stage.reserve(payload, h->hook)) || (rc = h->d_seg.reserve(5 * (size_t)nseg + ncolsum, h->hook)))
    return rc;
  int si = 0, coloff = 0;
  size_t dataoff = 0;
  for (auto& kv : segs) {
    const int lo = kv.first.first, hi = kv.first.second, nc = (int)kv.second.size();
    int* rec = h->h_seg.p + 5 * si;
    rec[0] = lo; rec[1] = hi; rec[2] = nc; rec[3] = coloff; rec[4] = (int)dataoff;
    for (int j = 0; j < nc; ++j) h->h_seg.p[5 * nseg + coloff + j] = kv.second[j];
    for (int r = lo; r < hi; ++r) {
      const double* src = theta_host + (size_t)r * np;
      double* dst = h->h_stage.p + dataoff + (size_t)(r - lo) * nc;
      for (int j = 0; j < nc; ++j) dst[j] = src[kv.second[j]];
    }
    dataoff += (size_t)(hi - lo) * nc;
    coloff += nc;
    ++si;
  }
  EWH_HIP(hipMemcpyAsync(h->d_seg.p, h->h_seg.p, sizeof(int) * (5 * (size_t)nseg + ncolsum), hipMemcpyHostToDevice,
                         h->stream));
  EWH_HIP(hipMemcpyAsync(h->d_stage.p, h->h_stage.p, sizeof(double) * payload, hipMemcpyHostToDevice, h->stream));
  // every entry the segments do not cover reads as NaN (all bits set): a
  // column some kernel reads but psr_cols does not list gives a non-finite
  // phi -- a failed sample, not a stale value from an earlier batch
  EWH_HIP(hipMemsetAsync(h->d_theta.p, 0xFF, sizeof(double) * (size_t)B * np, h->stream));
  hipLaunchKernelGGL(expand_theta_kernel, dim3(nseg), dim3(256), 0, h->stream, h->d_stage.p, h->d_seg.p, nseg, np,
                     h->d_theta.p);
  EWH_HIP(hipGetLastError());
  return (long long)(payload * sizeof(double));
}

// Correlated common process, batch smaller than the device count (one
// PTMCMC proposal): the pulsars are split over the devices (the exchange step
// of SURVEY.md §8(e)) -- each device runs the partial factorisations of its
// pulsars, its kept common blocks and local terms are copied peer-to-peer into
// the first device's buffers (the all-gather), and the first device assembles
// and factors Sigma_c.  Per-pulsar results do not depend on the device, so the
// value equals the one-device result bit for bit.
int lnl_batch_corr_pulsars(ewh_handle* H, int B, double* out_host) {
  const int nd = (int)H->ctx.size(), P = H->P, np = H->n_param;
  DevCtx* h0 = H->ctx[0];
  const size_t kd2 = (size_t)(16 * h0->keep) * (16 * h0->keep);
  int rc;
  if ((rc = H->h_out.reserve((size_t)B, H->out_changed))) return rc;
  for (int i = 0; i < nd; ++i) {
    DevCtx* h = H->ctx[i];
    EWH_HIP(hipSetDevice(h->device));
    if ((rc = reserve_io(h, B)) || (rc = reserve_units(h, B)) || (rc = reserve_keep(h, B))) return rc;
  }
  EWH_HIP(hipSetDevice(h0->device));
  EWH_HIP(hipMemsetAsync(h0->d_units.p, 0, sizeof(double) * (size_t)(P + 1) * B, h0->stream));
  // theta on the first device always: corr_finish reads it there even when
  // the first context gets no pulsars (P < number of contexts)
  if (np > 0)
    EWH_HIP(hipMemcpyAsync(h0->d_theta.p, H->h_theta.p, sizeof(double) * (size_t)B * np, hipMemcpyHostToDevice,
                           h0->stream));
  H->h2d_bytes += (long long)sizeof(double) * B * np;
  EWH_HIP(hipStreamSynchronize(h0->stream));
  for (int i = 0; i < nd; ++i) {
    DevCtx* h = H->ctx[i];
    const int p0 = (int)((long long)P * i / nd), p1 = (int)((long long)P * (i + 1) / nd);
    if (p1 <= p0) continue;
    EWH_HIP(hipSetDevice(h->device));
    if (np > 0 && i > 0) {
      EWH_HIP(hipMemcpyAsync(h->d_theta.p, H->h_theta.p, sizeof(double) * (size_t)B * np, hipMemcpyHostToDevice,
                             h->stream));
      H->h2d_bytes += (long long)sizeof(double) * B * np;
    }
    if ((rc = corr_partial(h, h->d_theta.p, B, p0, p1, h->d_units.p, h->d_keep.p, h->stream))) return rc;
    if (i > 0) {   // gather: this device's pulsar slices into the first device
      EWH_HIP(hipMemcpyPeerAsync(h0->d_keep.p + (size_t)p0 * B * kd2, h0->device, h->d_keep.p + (size_t)p0 * B * kd2,
                                 h->device, sizeof(double) * (size_t)(p1 - p0) * B * kd2, h->stream));
      EWH_HIP(hipMemcpyPeerAsync(h0->d_units.p + (size_t)p0 * B, h0->device, h->d_units.p + (size_t)p0 * B, h->device,
                                 sizeof(double) * (size_t)(p1 - p0) * B, h->stream));
    }
  }
  for (int i = 1; i < nd; ++i) {
    EWH_HIP(hipSetDevice(H->ctx[i]->device));
    EWH_HIP(hipStreamSynchronize(H->ctx[i]->stream));
  }
  EWH_HIP(hipSetDevice(h0->device));
  if ((rc = corr_finish(h0, h0->d_theta.p, B, h0->d_keep.p, h0->d_units.p, h0->stream))) return rc;
  hipLaunchKernelGGL(reduce_units_kernel, dim3((B + 255) / 256), dim3(256), 0, h0->stream, h0->d_units.p, P + 1, B,
                     h0->d_out);
  EWH_HIP(hipGetLastError());
  EWH_HIP(hipMemcpyAsync(H->h_out.p, h0->d_out, sizeof(double) * B, hipMemcpyDeviceToHost, h0->stream));
  EWH_HIP(hipStreamSynchronize(h0->stream));
  std::memcpy(out_host, H->h_out.p, sizeof(double) * B);
  H->last_split.assign(1, {0, (long long)P * B});     // unit terms live on the first device
  H->last_B = B;
  h0->last_B = B;
  return 0;
}

// One device: replay the captured graph of this batch size when there is one;
// otherwise run the batch eagerly (that also sizes every scratch buffer) and
// capture the same sequence for the next call.
constexpr uint64_t LAT_SENTINEL = 0x7ff4dead0ebeef01ull;   // a NaN no kernel writes
// batches up to this size take the latency kernel (round 4, interleaved on
// C3: B = 12 / 16 / 24 at 57.9 / 57.5 / 80.0 us vs 64.2 / 65.8 / 83.3 us
// batched; B = 32 even, larger batched -- profiles/r04d/latency_sweep_bmax.log)
constexpr int LAT_B_MAX = 24;

int lnl_batch_single(ewh_handle* H, DevCtx* h, int B, double* out_host) {
  int rc;
  EWH_HIP(hipSetDevice(h->device));
  if ((rc = H->h_out.reserve((size_t)B, H->out_changed))) return rc;
  if (h->lat_nb > 0 && B <= LAT_B_MAX && h->plan.lat) {
    // latency path: one launch reads theta from the pinned staging and writes
    // the unit terms to pinned memory (chol_lat.hip); the host folds them
    if ((rc = reserve_units(h, B)) || (rc = H->h_out.reserve((size_t)h->P * B, H->out_changed))) return rc;
    // device addresses of the pinned staging (looked up again only after a reallocation)
    if (H->lat_th_host != H->h_theta.p) {
      EWH_HIP(hipHostGetDevicePointer((void**)&H->lat_th_dev, H->h_theta.p, 0));
      H->lat_th_host = H->h_theta.p;
    }
    if (H->lat_out_host != H->h_out.p) {
      EWH_HIP(hipHostGetDevicePointer((void**)&H->lat_out_dev, H->h_out.p, 0));
      H->lat_out_host = H->h_out.p;
    }
    double *th_dev = H->lat_th_dev, *out_dev = H->lat_out_dev;
    // every unit term lands in pinned memory; the host waits for them by
    // spinning on a sentinel (a NaN payload the kernel never writes: its
    // terms are finite or -inf) instead of a stream synchronisation, whose
    // wake-up is a sizeable share of a ~30 us call.  Every workgroup reads
    // theta before it writes its term, so the staging is free once all terms
    // are in; a launch error or a stall falls back to the stream (2 s)
    const size_t nu = (size_t)h->P * B;
    volatile uint64_t* hu = reinterpret_cast<volatile uint64_t*>(H->h_out.p);
    for (size_t i = 0; i < nu; ++i) hu[i] = LAT_SENTINEL;
    if ((rc = launch_chol_lat(h->lat_nb, h->lat_dead, h->d_jobs_fixed, B, h->P, th_dev, h->n_param, h->d_units.p, out_dev,
                              h->stream, h->plan.lat_stamps, h->plan.lat_variant)) < 0)
      return rc;
    if (rc == 0) {
      const auto t0 = std::chrono::steady_clock::now();
      size_t seen = 0;
      for (long spins = 0;; ++spins) {
        while (seen < nu && hu[seen] != LAT_SENTINEL) ++seen;
        if (seen == nu) break;
        if ((spins & 4095) == 4095) {
          const hipError_t q = hipStreamQuery(h->stream);
          if (q != hipSuccess && q != hipErrorNotReady)
            return set_err(EWH_E_HIP, std::string("chol_lat_kernel: ") + hipGetErrorString(q));
          if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) {
            EWH_HIP(hipStreamSynchronize(h->stream));
            for (seen = 0; seen < nu && hu[seen] != LAT_SENTINEL; ++seen) {
            }
            if (seen != nu) return set_err(EWH_E_HIP, "chol_lat_kernel: unit terms missing after the launch");
            break;
          }
        }
      }
      std::atomic_thread_fence(std::memory_order_acquire);
      // a unit whose dataflow wait ran out carries LAT_STALL_BITS: an error,
      // never a NaN lnL (the ABI promises finite values or -inf)
      for (size_t i = 0; i < nu; ++i)
        if (hu[i] == LAT_STALL_BITS) {
          (void)hipStreamSynchronize(h->stream);
          return set_err(EWH_E_HIP, "chol_lat_kernel: a dataflow wait of unit " + std::to_string(i) +
                                        " ran out (LAT_SPIN_MAX); no lnL was produced");
        }
      // lnL_b = sum over pulsars in pulsar order (reduce_units_kernel's fold)
      bool failed = false;
      for (int b = 0; b < B; ++b) {
        double s = 0.0;
        for (int p = 0; p < h->P; ++p) s += H->h_out.p[(size_t)p * B + b];
        out_host[b] = s;
        failed = failed || !std::isfinite(s);
      }
      // an fp64 pivot failure (-inf term) is refactored in double-double by
      // the batched path (refine_failed): take it for this call instead
      if (!failed) {
        H->last_split.assign(1, {0, (long long)H->P * B});
        H->last_B = B;
        h->last_B = B;
        return 0;
      }
      EWH_HIP(hipStreamSynchronize(h->stream));
    }
  }
  if ((rc = reserve_io(h, B))) return rc;
  DevCtx::Graph* hit = nullptr;
  for (auto& g : h->graphs)
    if (g.B == B && g.mode == h->kernel_mode && g.ht == H->h_theta.p && g.ho == H->h_out.p) hit = &g;
  if (hit) {
    hit->last_use = ++h->graph_clock;
    EWH_HIP(hipGraphLaunch(hit->exec, h->stream));
  } else {
    if ((rc = enqueue_single(H, h, B))) return rc;
  }
  EWH_HIP(hipStreamSynchronize(h->stream));
  std::memcpy(out_host, H->h_out.p, sizeof(double) * B);
  H->last_split.assign(1, {0, (long long)H->P * B});
  H->last_B = B;
  if (hit || h->corr) return 0;     // (correlated batches are long: launch overhead is immaterial)
  // capture for the next call of this size (buffers are sized now, so the
  // sequence makes no allocation or synchronous call)
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  if (hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) return 0;
  rc = enqueue_single(H, h, B);
  const hipError_t e = hipStreamEndCapture(h->stream, &graph);
  if (rc || e != hipSuccess || !graph) {
    if (graph) (void)hipGraphDestroy(graph);
    (void)hipGetLastError();
    return 0;                       // no graph: the eager path stays correct
  }
  const hipError_t ei = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (ei != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  if (h->graphs.size() >= GRAPH_CACHE) {
    auto lru = std::min_element(h->graphs.begin(), h->graphs.end(),
                                [](const DevCtx::Graph& a, const DevCtx::Graph& b) { return a.last_use < b.last_use; });
    (void)hipGraphExecDestroy(lru->exec);
    h->graphs.erase(lru);
  }
  h->graphs.push_back({B, h->kernel_mode, H->h_theta.p, H->h_out.p, exec, ++h->graph_clock});
  return 0;
}

}  // namespace

extern "C" {

int ewh_version(void) { return EWH_ABI_VERSION; }
int ewh_lat_b_max(void) { return LAT_B_MAX; }

const char* ewh_last_error(void) { return g_err.c_str(); }

int ewh_create(const ewh_pta_desc* d, const int32_t* device_ids, int32_t ndev, ewh_handle** out) {
  if (!out) return set_err(EWH_E_INVALID, "out is NULL");
  *out = nullptr;
  if (ndev < 0 || (ndev > 0 && !device_ids) || ndev > 64) return set_err(EWH_E_INVALID, "bad device list");
  int rc = validate(d);
  if (rc) return rc;
  int count = 0;
  EWH_HIP(hipGetDeviceCount(&count));
  std::vector<int> ids = ndev ? std::vector<int>(device_ids, device_ids + ndev) : std::vector<int>{0};
  for (int id : ids)
    if (id < 0 || id >= count) return set_err(EWH_E_INVALID, "device id " + std::to_string(id) + " out of range");
  ewh_handle* H = new ewh_handle();
  H->P = d->n_pulsar;
  H->n_param = d->n_param;
  H->psr_cols.resize(d->n_pulsar);
  for (int p = 0; p < d->n_pulsar; ++p) {
    const ewh_pulsar_desc& sd = d->pulsars[p];
    std::vector<int>& cols = H->psr_cols[p];
    auto add = [&](const ewh_pref& r) {
      if (r.idx >= 0) cols.push_back(r.idx);
    };
    for (int i = 0; i < sd.n_slot; ++i) add(sd.slots[i]);
    for (int e = 0; e < sd.n_spec; ++e) {
      add(sd.spec[e].p0);
      add(sd.spec[e].p1);
      add(sd.spec[e].p2);
    }
    for (int g = 0; g < sd.n_bgroup; ++g) add(sd.bgroup_idx[g]);
    for (int k = 0; k < sd.n_delay; ++k) {
      add(sd.delays[k].p0);
      add(sd.delays[k].p1);
      add(sd.delays[k].p2);
      add(sd.delays[k].p3);
    }
    if (d->common && d->common->spec)
      for (int g = 0; g < d->common->n_col; ++g) {
        add(d->common->spec[g].p0);
        add(d->common->spec[g].p1);
        add(d->common->spec[g].p2);
      }
    std::sort(cols.begin(), cols.end());
    cols.erase(std::unique(cols.begin(), cols.end()), cols.end());
  }
  std::vector<ProjCoef> proj(d->n_pulsar);
  for (int p = 0; p < d->n_pulsar; ++p) proj[p] = projection_coef(d->pulsars[p]);
  for (int id : ids) {
    DevCtx* c = nullptr;
    if ((rc = create_ctx(d, proj, id, &c))) {
      ewh_destroy(H);
      return rc;
    }
    H->ctx.push_back(c);
  }
  H->corr = H->ctx[0]->corr;
  // peer access between every context's device and the first one (both
  // directions: partial B-vectors and gathered kept blocks move device to
  // device); bit i of peer_mask records context i
  H->peer_mask = 1;
  for (size_t i = 1; i < ids.size(); ++i) {
    bool ok = ids[i] == ids[0];
    if (!ok) {
      int a = 0, b = 0;
      if (hipDeviceCanAccessPeer(&a, ids[i], ids[0]) == hipSuccess && hipDeviceCanAccessPeer(&b, ids[0], ids[i]) ==
                                                                             hipSuccess && a && b) {
        const bool a1 = peer_acquire(H, ids[i], ids[0]);
        const bool a2 = peer_acquire(H, ids[0], ids[i]);
        ok = a1 && a2;
      }
    }
    if (ok) H->peer_mask |= 1LL << i;
  }
  *out = H;
  return 0;
}

int ewh_transfer_stats(const ewh_handle* H, int64_t* h2d_bytes, int64_t* peer) {
  if (!H) return set_err(EWH_E_INVALID, "bad handle");
  if (h2d_bytes) *h2d_bytes = H->h2d_bytes;
  if (peer) *peer = H->peer_mask;
  return 0;
}

int ewh_refine_stats(ewh_handle* H, int64_t* checked, int64_t* refined) {
  if (!H) return set_err(EWH_E_INVALID, "bad handle");
  long long c = 0, r = 0;
  for (DevCtx* h : H->ctx) {
    EWH_HIP(hipSetDevice(h->device));
    // (the whole device: ewh_lnl_units_device runs the route on the caller's
    // stream, whose work must be counted before the reset)
    EWH_HIP(hipDeviceSynchronize());
    unsigned long long v[2] = {0, 0};
    if (h->d_ddstat) {
      EWH_HIP(hipMemcpy(v, h->d_ddstat, sizeof v, hipMemcpyDeviceToHost));
      EWH_HIP(hipMemset(h->d_ddstat, 0, sizeof v));
    }
    c += (long long)v[1];
    r += (long long)v[0];
  }
  if (checked) *checked = c;
  if (refined) *refined = r;
  return 0;
}

int ewh_num_devices(const ewh_handle* H) { return H ? (int)H->ctx.size() : 0; }

int ewh_set_fixed_white(ewh_handle* H, const double* values) {
  if (!H || !values) return set_err(EWH_E_INVALID, "bad arguments");
  for (DevCtx* h : H->ctx) {
    EWH_HIP(hipSetDevice(h->device));
    size_t off = 0;
    for (auto& ps : h->psr) {
      for (int i = 0; i < ps.n_slot; ++i)
        if (ps.slots[i].idx < 0) ps.slots[i].cval = values[off + i];
      off += ps.n_slot;
      if (ps.n_slot)
        EWH_HIP(hipMemcpyAsync(ps.d_slots, ps.slots.data(), sizeof(ewh_pref) * ps.n_slot, hipMemcpyHostToDevice,
                               h->stream));
    }
    EWH_HIP(hipStreamSynchronize(h->stream));
    drop_graphs(h);
    if (h->white_fixed) {
      int rc = setup_fixed(h);
      if (rc) return rc;
    }
  }
  return 0;
}

int ewh_set_kernel_mode(ewh_handle* H, int32_t mode) {
#ifdef EWH_DEV
  constexpr bool dev_lib = true;
#else
  constexpr bool dev_lib = false;
#endif
  const KernelPlan plan = plan_for(mode, dev_lib);
  if (!H || !plan.in_range) return set_err(EWH_E_INVALID, "bad handle / mode");
  if (!plan.valid || (plan.variant && !variant_built(mode)))
    return set_err(EWH_E_UNSUPPORTED, "kernel mode " + std::to_string(mode) +
                                          " is not built into this library (A/B variants: the dev library, make dev)");
  for (DevCtx* h : H->ctx) {
    h->kernel_mode = mode;
    h->plan = plan;
    (void)hipSetDevice(h->device);
    drop_graphs(h);
    const bool stage = plan.stage_spectra;
    // all_dd on a pulsar whose S_lo was not kept (register widths): set up again
    bool need_lo = false;
    if (h->white_fixed)
      for (const auto& ps : h->psr) need_lo = need_lo || (!ps.d_Slo && dd_path(plan, h->corr, h->osmode, ps.fx_nb, true));
    if (stage != h->stage_spectra || need_lo) {
      h->stage_spectra = stage;
      if (h->white_fixed) {
        const int rc = setup_fixed(h);
        if (rc) return rc;
      }
    }
  }
  return 0;
}

double ewh_unit_cost(const ewh_handle* H, int32_t p) {
  if (!H || p < 0 || p >= H->P) return 0.0;
  return ctx_unit_cost(H->ctx[0], p);
}

int ewh_lnl_units_device(ewh_handle* H, const double* theta_dev, int32_t B, int64_t u_begin, int64_t u_end,
                         double* out_dev, void* stream) {
  if (!H || !theta_dev || !out_dev || B <= 0) return set_err(EWH_E_INVALID, "bad arguments");
  DevCtx* h = H->ctx[0];
  if (h->osmode) return set_err(EWH_E_UNSUPPORTED, "an optimal-statistic handle evaluates ewh_optstat only");
  int rc = ctx_units(h, theta_dev, B, u_begin, u_end, out_dev, (hipStream_t)stream, true);
  if (rc) return rc;
  H->last_split.assign(1, {std::max<int64_t>(0, u_begin), std::min<int64_t>((long long)H->P * B, u_end)});
  H->last_B = B;
  return 0;
}

int ewh_lnl_batch(ewh_handle* H, const double* theta_host, int32_t B, double* out_host) {
  if (!H || !theta_host || !out_host || B <= 0) return set_err(EWH_E_INVALID, "bad arguments");
  if (H->ctx[0]->osmode) return set_err(EWH_E_UNSUPPORTED, "an optimal-statistic handle evaluates ewh_optstat only");
  const int nd = (int)H->ctx.size(), np = H->n_param;
  int rc;
  H->h2d_bytes = 0;
  if (nd == 1 || H->corr) {
    // (single context: the batch's theta rows, read by the latency kernel
    // straight from the pinned staging or copied once; correlated: each
    // context's sample slice, or every pulsar partition its copy)
    if ((rc = H->h_theta.reserve((size_t)B * std::max(1, np), H->th_changed))) return rc;
    if (np > 0) std::memcpy(H->h_theta.p, theta_host, sizeof(double) * (size_t)B * np);
  }
  if (nd == 1) {
    H->h2d_bytes = (long long)sizeof(double) * B * np;
    return lnl_batch_single(H, H->ctx[0], B, out_host);
  }
  if (H->corr && B < nd) return lnl_batch_corr_pulsars(H, B, out_host);
  std::vector<std::pair<long long, long long>> split;
  if (H->corr) {
    // samples: contiguous slices (the cross-pulsar factorisation needs every
    // pulsar of a sample on one device)
    for (int i = 0; i < nd; ++i) split.push_back({(long long)B * i / nd, (long long)B * (i + 1) / nd});
  } else {
    std::vector<double> cost(H->P);
    for (int p = 0; p < H->P; ++p) cost[p] = ctx_unit_cost(H->ctx[0], p);
    split = unit_ranges(cost, B, nd);
  }
  if ((rc = H->h_out.reserve((size_t)B, H->out_changed))) return rc;
  DevCtx* h0 = H->ctx[0];
  if (!H->corr) {
    // per-context partial sums are folded on the first device: a partial
    // B-vector per context there, one event per context
    EWH_HIP(hipSetDevice(h0->device));
    if ((rc = H->d_part.reserve((size_t)nd * B))) return rc;
    while ((int)H->ev.size() < nd) {
      const int i = (int)H->ev.size();
      EWH_HIP(hipSetDevice(H->ctx[i]->device));
      hipEvent_t e;
      EWH_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      H->ev.push_back(e);
    }
  }
  for (int i = 0; i < nd; ++i) {
    DevCtx* h = H->ctx[i];
    const long long a = split[i].first, b = split[i].second;
    EWH_HIP(hipSetDevice(h->device));
    if (H->corr) {
      if (b <= a) continue;
      const int Bd = (int)(b - a);
      if ((rc = reserve_io(h, Bd))) return rc;
      if (np > 0)
        EWH_HIP(hipMemcpyAsync(h->d_theta.p, H->h_theta.p + (size_t)a * np, sizeof(double) * (size_t)Bd * np,
                               hipMemcpyHostToDevice, h->stream));
      H->h2d_bytes += (long long)sizeof(double) * Bd * np;
      if ((rc = ctx_units(h, h->d_theta.p, Bd, 0, (long long)H->P * Bd, h->d_out, h->stream, true))) return rc;
      EWH_HIP(hipMemcpyAsync(H->h_out.p + a, h->d_out, sizeof(double) * Bd, hipMemcpyDeviceToHost, h->stream));
    } else {
      // every context evaluates its unit range and sums it over its pulsars
      // (rows outside the range are zero) into a B-vector, which goes to the
      // first device; only B doubles ever come back to the host
      if ((rc = reserve_io(h, B))) return rc;
      // only the theta entries this context's units read (the host packs
      // context i + 1's while context i's copy and launches run)
      const long long nbytes = stage_theta_range(H, h, theta_host, B, a, b);
      if (nbytes < 0) return (int)nbytes;
      H->h2d_bytes += nbytes;
      if ((rc = ctx_units(h, h->d_theta.p, B, a, b, h->d_out, h->stream, true))) return rc;
      EWH_HIP(hipMemcpyPeerAsync(H->d_part.p + (size_t)i * B, h0->device, h->d_out, h->device, sizeof(double) * B,
                                 h->stream));
      EWH_HIP(hipEventRecord(H->ev[i], h->stream));
    }
  }
  if (!H->corr) {
    EWH_HIP(hipSetDevice(h0->device));
    for (int i = 1; i < nd; ++i) EWH_HIP(hipStreamWaitEvent(h0->stream, H->ev[i], 0));
    hipLaunchKernelGGL(fold_partials_kernel, dim3((B + 255) / 256), dim3(256), 0, h0->stream, H->d_part.p, nd, B,
                       h0->d_out);
    EWH_HIP(hipGetLastError());
    EWH_HIP(hipMemcpyAsync(H->h_out.p, h0->d_out, sizeof(double) * B, hipMemcpyDeviceToHost, h0->stream));
    EWH_HIP(hipStreamSynchronize(h0->stream));
  } else {
    for (int i = 0; i < nd; ++i) {
      if (split[i].second <= split[i].first) continue;
      EWH_HIP(hipSetDevice(H->ctx[i]->device));
      EWH_HIP(hipStreamSynchronize(H->ctx[i]->stream));
    }
  }
  std::memcpy(out_host, H->h_out.p, sizeof(double) * B);
  H->last_split = split;
  H->last_B = B;
  return 0;
}

int ewh_contract_device(ewh_handle* H, const double* theta_dev, int32_t B, void* stream) {
  if (!H || !theta_dev || B <= 0) return set_err(EWH_E_INVALID, "bad arguments");
  DevCtx* h = H->ctx[0];
  if (h->white_fixed || h->corr || h->osmode)
    return set_err(EWH_E_UNSUPPORTED, "ewh_contract_device: white noise must vary (uncorrelated / CURN handle)");
  EWH_HIP(hipSetDevice(h->device));
  int rc;
  if ((rc = reserve_var_scratch(h, B))) return rc;
  hipStream_t saved = h->stream;
  h->stream = (hipStream_t)stream;
  for (int p = 0; p < h->P && !rc; ++p)
    for (int c0 = 0; c0 < B && !rc; c0 += h->var.chunk) rc = run_white(h, p, theta_dev, h->n_param, c0, std::min(h->var.chunk, B - c0));
  h->stream = saved;
  return rc;
}

int ewh_keep_dim(const ewh_handle* H) {
  if (!H || !H->corr) return 0;
  return 16 * H->ctx[0]->keep;
}

int ewh_corr_partial_device(ewh_handle* H, const double* theta_dev, int32_t B, int32_t p_begin, int32_t p_end,
                            double* keep_dev, double* local_dev, void* stream) {
  if (!H || !H->corr || !theta_dev || !keep_dev || !local_dev || B <= 0 || p_begin < 0 || p_end > H->P ||
      p_begin > p_end)
    return set_err(EWH_E_INVALID, "bad arguments (needs a correlated-common-process handle)");
  DevCtx* h = H->ctx[0];
  EWH_HIP(hipSetDevice(h->device));
  int rc = corr_partial(h, theta_dev, B, p_begin, p_end, local_dev, keep_dev, (hipStream_t)stream);
  if (rc) return rc;
  EWH_HIP(hipGetLastError());
  return 0;
}

int ewh_corr_finish_device(ewh_handle* H, const double* theta_dev, int32_t B, const double* keep_dev,
                           const double* local_dev, double* out_dev, void* stream) {
  if (!H || !H->corr || !theta_dev || !keep_dev || !local_dev || !out_dev || B <= 0)
    return set_err(EWH_E_INVALID, "bad arguments (needs a correlated-common-process handle)");
  DevCtx* h = H->ctx[0];
  hipStream_t st = (hipStream_t)stream;
  EWH_HIP(hipSetDevice(h->device));
  int rc;
  if ((rc = reserve_units(h, B))) return rc;
  EWH_HIP(hipMemcpyAsync(h->d_units.p, local_dev, sizeof(double) * (size_t)H->P * B, hipMemcpyDeviceToDevice, st));
  if ((rc = corr_finish(h, theta_dev, B, keep_dev, h->d_units.p, st))) return rc;
  hipLaunchKernelGGL(reduce_units_kernel, dim3((B + 255) / 256), dim3(256), 0, st, h->d_units.p, H->P + 1, B, out_dev);
  EWH_HIP(hipGetLastError());
  H->last_split.assign(1, {0, (long long)H->P * B});
  H->last_B = B;
  h->last_B = B;
  return 0;
}

int ewh_optstat(ewh_handle* H, const double* theta_host, int32_t B, const double* phihat_host, double* rho_host,
                double* sig_host, double* os_host, double* os_sig_host) {
  if (!H) return set_err(EWH_E_INVALID, "bad arguments");
  return ctx_optstat(H->ctx[0], theta_host, B, phihat_host, rho_host, sig_host, os_host, os_sig_host);
}

int ewh_cond_dims(const ewh_handle* H, int64_t* n_coef, int64_t* n_toa_total) {
  if (!H) return set_err(EWH_E_INVALID, "bad handle");
  int64_t nc = 0, nt = 0;
  for (const auto& ps : H->ctx[0]->psr) {
    nc += ps.m;
    nt += ps.n_toa;
  }
  if (n_coef) *n_coef = nc;
  if (n_toa_total) *n_toa_total = nt;
  return 0;
}

int ewh_cond_gp(ewh_handle* H, const double* theta_host, int32_t B, const double* z_host, int32_t n_group,
                const int32_t* col_group, double* coef_host, double* proc_host, int32_t* status_host) {
  if (!H || !theta_host || B <= 0 || n_group < 0 || (n_group > 0) != (col_group != nullptr) ||
      (n_group > 0) != (proc_host != nullptr))
    return set_err(EWH_E_INVALID, "bad arguments");
  DevCtx* h = H->ctx[0];
  if (h->corr || h->osmode)
    return set_err(EWH_E_UNSUPPORTED, "ewh_cond_gp: uncorrelated / CURN handles only (a correlated common process "
                                      "needs the dense Sigma_c solve; an optimal-statistic handle evaluates ewh_optstat)");
  int64_t n_coef = 0, n_toa = 0;
  ewh_cond_dims(H, &n_coef, &n_toa);
  for (int64_t j = 0; col_group && j < n_coef; ++j)
    if (col_group[j] < -1 || col_group[j] >= n_group) return set_err(EWH_E_INVALID, "col_group entry out of range");
  if ((long long)B * std::max(1, n_group) > (1LL << 30)) return set_err(EWH_E_INVALID, "B x n_group too large");
  return ctx_cond_gp(h, theta_host, B, z_host, n_group, col_group, coef_host, proc_host, status_host, n_coef, n_toa);
}

int ewh_cond_joint_dims(const ewh_handle* H, int64_t* n_coef, int64_t* n_toa_total) {
  if (!H) return set_err(EWH_E_INVALID, "bad handle");
  if (!H->ctx[0]->corr)
    return set_err(EWH_E_INVALID, "ewh_cond_joint_dims: the handle has no EWH_COMMON_CORRELATED descriptor "
                                  "(uncorrelated / CURN handles take ewh_cond_dims)");
  int64_t nc = 0, nt = 0;
  for (const auto& ps : H->ctx[0]->psr) {
    nc += ps.nlead + ps.fx_m;       // the descriptor's n_col (ps.m is the padded width with varying white noise)
    nt += ps.n_toa;
  }
  if (n_coef) *n_coef = nc;
  if (n_toa_total) *n_toa_total = nt;
  return 0;
}

int ewh_cond_joint(ewh_handle* H, const double* theta_host, int32_t B, const double* z_host, int32_t n_group,
                   const int32_t* col_group, double* coef_host, double* proc_host, int32_t* status_host,
                   int32_t max_chunk) {
  if (!H || !theta_host || B <= 0 || n_group < 0 || max_chunk < 0 || (n_group > 0) != (col_group != nullptr) ||
      (n_group > 0) != (proc_host != nullptr))
    return set_err(EWH_E_INVALID, "bad arguments");
  DevCtx* h = H->ctx[0];
  if (!h->corr)
    return set_err(EWH_E_INVALID, "ewh_cond_joint: the handle has no EWH_COMMON_CORRELATED descriptor (uncorrelated / "
                                  "CURN handles take ewh_cond_gp)");
  int64_t n_coef = 0, n_toa = 0;
  if (const int rc = ewh_cond_joint_dims(H, &n_coef, &n_toa)) return rc;
  for (int64_t j = 0; col_group && j < n_coef; ++j)
    if (col_group[j] < -1 || col_group[j] >= n_group) return set_err(EWH_E_INVALID, "col_group entry out of range");
  if ((long long)B * std::max(1, n_group) > (1LL << 30)) return set_err(EWH_E_INVALID, "B x n_group too large");
  return ctx_cond_joint(h, theta_host, B, z_host, n_group, col_group, coef_host, proc_host, status_host, max_chunk,
                        n_coef, n_toa);
}

int ewh_last_unit_terms(ewh_handle* H, double* out_host, int32_t B) {
  if (!H || !out_host || B != H->last_B || H->last_split.empty()) return set_err(EWH_E_INVALID, "no matching previous call");
  const int P = H->P, nd = (int)H->last_split.size();
  const bool by_samples = nd == 1 ? false : H->corr;
  std::memset(out_host, 0, sizeof(double) * (size_t)P * B);
  std::vector<double> tmp;
  for (int i = 0; i < nd; ++i) {
    DevCtx* h = H->ctx[i];
    const long long a = H->last_split[i].first, b = H->last_split[i].second;
    if (b <= a || !h->d_units.p) continue;
    EWH_HIP(hipSetDevice(h->device));
    EWH_HIP(hipStreamSynchronize(h->stream));
    EWH_HIP(hipDeviceSynchronize());
    if (nd == 1 && !H->corr) {
      EWH_HIP(hipMemcpy(out_host, h->d_units.p, sizeof(double) * (size_t)P * B, hipMemcpyDeviceToHost));
    } else if (by_samples || nd == 1) {
      const int Bd = nd == 1 ? B : (int)(b - a);
      const long long s0 = nd == 1 ? 0 : a;
      tmp.resize((size_t)P * Bd);
      EWH_HIP(hipMemcpy(tmp.data(), h->d_units.p, sizeof(double) * (size_t)P * Bd, hipMemcpyDeviceToHost));
      for (int p = 0; p < P; ++p)
        for (int k = 0; k < Bd; ++k) out_host[(size_t)p * B + s0 + k] = tmp[(size_t)p * Bd + k];
    } else {
      EWH_HIP(hipMemcpy(out_host + a, h->d_units.p + a, sizeof(double) * (size_t)(b - a), hipMemcpyDeviceToHost));
    }
  }
  return 0;
}

void ewh_destroy(ewh_handle* H) {
  if (!H) return;
  for (size_t i = 0; i < H->ev.size(); ++i) {
    (void)hipSetDevice(H->ctx[i]->device);
    (void)hipEventDestroy(H->ev[i]);
  }
  if (H->d_part.p) {
    (void)hipSetDevice(H->ctx[0]->device);
    H->d_part.release();
  }
  for (DevCtx* c : H->ctx) destroy_ctx(c);
  peer_release_all(H);
  H->h_theta.release();
  H->h_out.release();
  delete H;
}

#ifdef EWH_DEV
// ---- dev library only (make dev): intermediate quantities for diagnostics ----
// register-kernel launches so far with the interpreted (out[0]) and the
// fixed-form (out[1]) spectrum prologue, every handle of the process (a
// launch replayed from a captured graph counts once, at its capture)
int ewh_dev_prologue_launches(long long* out) {
  out[0] = g_prologue_launches[0].load();
  out[1] = g_prologue_launches[1].load();
  return 0;
}
// G = T_aug^T N^-1 T_aug of pulsar p for samples [0, B) (B <= the varying-WN
// chunk), row-major ld x ld per sample; returns ld (or a negative code).
int ewh_dev_gram(ewh_handle* H, int32_t p, const double* theta_host, int32_t B, double* G_out) {
  DevCtx* h = H->ctx[0];
  if (p < 0 || p >= h->P || B <= 0) return set_err(EWH_E_INVALID, "bad arguments");
  // (the chunk scratch of such a handle is sized for its delay pulsars alone)
  if (h->white_fixed && h->n_delay_psr > 0)
    return set_err(EWH_E_UNSUPPORTED, "ewh_dev_gram: fixed white noise with delay pulsars");
  int rc;
  EWH_HIP(hipSetDevice(h->device));
  const bool wf = h->white_fixed;
  h->white_fixed = false;
  rc = reserve_var_scratch(h, B);
  h->white_fixed = wf;
  if (rc) return rc;
  if (B > h->var.chunk) return set_err(EWH_E_INVALID, "B exceeds the varying-WN chunk");
  if ((rc = reserve_io(h, B))) return rc;
  if (h->n_param > 0)
    EWH_HIP(hipMemcpy(h->d_theta.p, theta_host, sizeof(double) * (size_t)B * h->n_param, hipMemcpyHostToDevice));
  if ((rc = run_white(h, p, h->d_theta.p, h->n_param, 0, B))) return rc;
  EWH_HIP(hipStreamSynchronize(h->stream));
  const int ld = h->psr[p].ld;
  EWH_HIP(hipMemcpy(G_out, h->var.d_G.p, sizeof(double) * (size_t)B * ld * ld, hipMemcpyDeviceToHost));
  return ld;
}

// the double-double G_hi / G_lo of gram_dd_units_kernel (the fp64-failure
// refinement, varying white noise) of pulsar p for samples [0, B); returns ld
int ewh_dev_gram_dd(ewh_handle* H, int32_t p, const double* theta_host, int32_t B, double* G_out, double* Glo_out) {
  DevCtx* h = H->ctx[0];
  if (p < 0 || p >= h->P || B <= 0 || h->white_fixed) return set_err(EWH_E_INVALID, "bad arguments");
  int rc;
  EWH_HIP(hipSetDevice(h->device));
  if ((rc = reserve_var_scratch(h, B))) return rc;
  if (B > h->var.chunk) return set_err(EWH_E_INVALID, "B exceeds the varying-WN chunk");
  if ((rc = reserve_io(h, B)) || (rc = reserve_units(h, B))) return rc;
  EWH_HIP(hipMemcpy(h->d_theta.p, theta_host, sizeof(double) * (size_t)B * h->n_param, hipMemcpyHostToDevice));
  if ((rc = run_white(h, p, h->d_theta.p, h->n_param, 0, B))) return rc;
  std::vector<int> lst(B + 1);
  lst[0] = B;
  for (int b = 0; b < B; ++b) lst[b + 1] = p * B + b;
  const size_t U = (size_t)(h->P + 1) * B;
  if ((rc = h->d_ddlist.reserve(U + 1, h->hook))) return rc;
  EWH_HIP(hipMemcpy(h->d_ddlist.p, lst.data(), sizeof(int) * (B + 1), hipMemcpyHostToDevice));
  const PsrHost& ps = h->psr[p];
  launch_gram_dd_units(ps.dev, ps.nb, (unsigned)std::min(B, 64), ps.d_Tlo, h->var.d_w.p, h->var.d_beta.p, h->d_ddlist.p + 1,
                       h->d_ddlist.p, B, 0, h->var.d_G.p, h->var.d_Glo.p, h->stream);
  EWH_HIP(hipStreamSynchronize(h->stream));
  const int ld = ps.ld;
  EWH_HIP(hipMemcpy(G_out, h->var.d_G.p, sizeof(double) * (size_t)B * ld * ld, hipMemcpyDeviceToHost));
  EWH_HIP(hipMemcpy(Glo_out, h->var.d_Glo.p, sizeof(double) * (size_t)B * ld * ld, hipMemcpyDeviceToHost));
  return ld;
}

// the cached reduced matrix S_p (fx_ld x fx_ld) and K_p of a fixed-WN handle; returns fx_ld
int ewh_dev_reduced(ewh_handle* H, int32_t p, double* S_out, double* K_out) {
  DevCtx* h = H->ctx[0];
  if (!h->white_fixed || p < 0 || p >= h->P) return set_err(EWH_E_INVALID, "bad arguments");
  EWH_HIP(hipSetDevice(h->device));
  EWH_HIP(hipDeviceSynchronize());
  const int n = h->psr[p].fx_ld;
  EWH_HIP(hipMemcpy(S_out, h->psr[p].d_S, sizeof(double) * (size_t)n * n, hipMemcpyDeviceToHost));
  EWH_HIP(hipMemcpy(K_out, h->d_fxK + p, sizeof(double), hipMemcpyDeviceToHost));
  return n;
}

// the operand images of S_p (ewarp_dev.h img_index; 256 nb (nb + 1) / 2 doubles
// each): the stored order into img_out and, where the job has one, the
// front-pad order into front_out (*has_front says so); returns the block
// count nb, or 0 where the pulsar has no image (more than MFMA_NB_MAX blocks)
int ewh_dev_images(ewh_handle* H, int32_t p, double* img_out, double* front_out, int32_t* has_front) {
  DevCtx* h = H->ctx[0];
  if (!h->white_fixed || p < 0 || p >= h->P) return set_err(EWH_E_INVALID, "bad arguments");
  EWH_HIP(hipSetDevice(h->device));
  EWH_HIP(hipDeviceSynchronize());
  const PsrHost& ps = h->psr[p];
  *has_front = ps.d_imgf != nullptr;
  if (!ps.d_img) return 0;
  const size_t bytes = sizeof(double) * (size_t)img_doubles(ps.fx_nb);
  EWH_HIP(hipMemcpy(img_out, ps.d_img, bytes, hipMemcpyDeviceToHost));
  if (ps.d_imgf) EWH_HIP(hipMemcpy(front_out, ps.d_imgf, bytes, hipMemcpyDeviceToHost));
  return ps.fx_nb;
}
#endif

}  // extern "C"
