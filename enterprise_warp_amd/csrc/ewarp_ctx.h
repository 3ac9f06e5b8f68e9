// ewarp_ctx.h — host-side state of the C ABI, shared by its two host units:
// ewarp_setup.hip builds and destroys a context (descriptor validation, CSR
// builders, the timing-model projection, the fixed-white-noise cache, the
// common-process tables), ewarp_hip.hip routes batches through it.  All
// memory is owned through ewarp_mem.h.
#pragma once

#include "ewarp_launch.h"
#include "ewarp_mem.h"

#include <utility>

namespace ewh_host {

using namespace ewh_dev;
using namespace ewh_mem;

constexpr size_t LDS_MAX = 160 * 1024;

struct PsrHost {
  int n_toa = 0, m = 0, nlead = 0, ld = 0, nb = 0, n_epoch = 0;
  int max_epoch = 0;               // TOAs of the longest ECORR epoch
  int fx_m = 0, fx_ld = 0, fx_nb = 0;
  int ncommon = 0, nloc = 0, gstart = 0;   // correlated layout of the reduced matrix
  // correlated common process with varying white noise: T_aug is laid out
  // [lead | own | pad to 16 | common | pad | r] -- common column g at
  // gstart_v + g, so the partial factorisation keeps whole blocks; the pads
  // inside take phi = 1 (CONST entries); mreal_v = gstart_v columns take phi^-1
  int gstart_v = 0;
  PsrDev dev{};
  int* d_colptr = nullptr;        // varying CSR (m+1)
  DSpec* d_spec = nullptr;
  int* d_fx_colptr = nullptr;     // fixed CSR (fx_m+1), entries re-indexed
  DSpec* d_fx_spec = nullptr;
  int* d_fx_rep = nullptr;        // fixed columns -> first column with the same spectrum
  int* d_fx_ulist = nullptr;      // the distinct-spectrum columns
  int fx_nu = 0;
  URec* d_fx_urec = nullptr;      // the distinct spectra with their entries inline (NULL: > URec::NE entries)
  std::vector<int> fx_tidx;       // theta entries the records read (their indices point here); empty: the whole row
  int* d_fx_urep = nullptr;       // fixed columns -> distinct-spectrum record (-1: no entry)
  // the records again in the product kernel's fixed form (ewarp_spec.h PlRec,
  // built at create with the records above; NULL: not every entry a power
  // law, pl_pack) and the most entries one of them has
  PlRec* d_fx_pl = nullptr;
  int fx_pl_ne = 0;
  double* d_S = nullptr;          // fx_ld^2
  double* d_Slo = nullptr;        // fx_ld^2, the low part of S (dd_path pulsars only)
  double* d_Srev = nullptr;       // fx_ld^2, fl(S + 2 S_lo): the reversed verify pass's input (with d_Slo)
  // the operand images of S for chol_mfma_kernel (fx_nb <= MFMA_NB_MAX;
  // img_doubles(fx_nb) each, ewarp_dev.h img_index): the stored order, and
  // the front-pad order where the frame has a dead slice (else NULL)
  double* d_img = nullptr;
  double* d_imgf = nullptr;
  // the projection residual X_lo of T_aug (round 6; the layout of dev.T,
  // zero outside the projected columns): dev.T + d_Tlo = T - M C to double-
  // double, read by the double-double Grams (gram_dd_block).  NULL for
  // pulsars with a theta-dependent basis (n_bgroup > 0) or the correlated
  // varying-WN layout
  double* d_Tlo = nullptr;
  bool has_theta_white = false;
  int n_slot = 0;
  ewh_pref* d_slots = nullptr;    // device copy of the white-noise slot table (PsrDev::slots)
  std::vector<ewh_pref> slots;    // host copy (ewh_set_fixed_white updates the constants)
  // deterministic delays (delay.hip): n_delay > 0 puts the pulsar's residual
  // column on the per-sample route.  Fixed white noise keeps for it what
  // setup_fixed forms before the timing-model elimination: the full-width
  // Gram (hi, lo; ld^2), w, beta and -1/2 log|N|
  DelayDev delay{};
  double *d_Gf = nullptr, *d_Gflo = nullptr, *d_wf = nullptr, *d_betaf = nullptr;
  double fxKb = 0.0;
  // the timing-model projection (ProjCoef) on the device, for the conditional
  // GP's back-map to the caller's basis (cond.hip): C is nlead x (nproj + 1)
  // row-major, its last column the residual's; projcols the nproj columns
  int nproj = 0;
  bool has_proj = false;          // false: no projection was applied (C is all zero)
  double* d_projC = nullptr;
  int* d_projcols = nullptr;
};

struct DevCtx {
  int device = 0;
  int n_cu = 256;              // compute units (hipDeviceAttributeMultiprocessorCount)
  int P = 0, n_param = 0;
  bool white_fixed = false;
  int kernel_mode = 0;         // as set: the graph-cache key, and launch_chol_small's variant selector
  KernelPlan plan{};           // plan_for(kernel_mode): what the code below tests
  bool stage_spectra = true;   // the KernelPlan::stage_spectra that the fixed jobs (setup_fixed) were built with
  hipStream_t stream = nullptr;
  std::vector<PsrHost> psr;
  // every device (re)allocation of the context drops the captured graphs
  // (create_ctx: drop_graphs on this context); `mem` holds what create and
  // setup upload -- tables, T_aug, the fixed-WN cache -- until destroy_ctx
  Hook hook;
  Arena mem;
  CholJob* d_jobs_fixed = nullptr;
  double* d_images = nullptr;    // the pulsars' operand images, one block (setup_fixed; PsrHost::d_img, d_imgf)
  CholJob* d_jobs_var = nullptr;
  double* d_fxK = nullptr;
  int* d_fxfail = nullptr;
  // per-call scratch
  Buf<double> d_units;
  Buf<double> d_theta;           // theta, and the outputs behind it:
  double* d_out = nullptr;       // d_theta.p + B max(1, n_param) (reserve_io)
  // varying-WN chunk scratch (reserve_var_scratch): sized for `chunk` samples
  struct VarChunk {
    Buf<double> d_w, d_beta, d_s, d_G, d_Kb, d_fac;
    Buf<double> d_rho;           // r^T W r per sample (the r-separated contraction)
    Buf<double> d_Glo;           // bases past 16 blocks: the low part of G (contract_wide_kernel)
    // delay pulsars (delay.hip): R = r', Z = N^-1 r' (TOA-major, chunk padded to
    // 16 samples) and the residual column (hi, lo; ld per sample).  A fixed-
    // white-noise handle with delay pulsars owns the chunk scratch too (those
    // pulsars' units are factored from d_G)
    Buf<double> d_dR, d_dZ, d_dcol, d_dcollo;
    long long s_stride = 0;      // doubles per sample in d_s (epoch rows padded to whole tiles)
    int chunk = 0;
    void release() {
      for (auto* b : {&d_w, &d_beta, &d_s, &d_G, &d_Kb, &d_fac, &d_rho, &d_Glo, &d_dR, &d_dZ, &d_dcol, &d_dcollo})
        b->release();
      chunk = 0;
    }
  } var;
  Buf<double> d_bigscr;          // chol_big_kernel: per-workgroup U blocks, BIG_SLOTS workgroups
  long long scr_budget = 0;      // bytes for each of the wide / dd scratches (scratch_budget)
  Buf<double> d_widescr;         // chol_wide_kernel: per-workgroup U blocks
  Buf<double> d_ddscr;           // chol_dd_kernel: per-workgroup hi / lo matrices
  Buf<double> d_units2;          // the verify step's reversed-order unit terms
  Buf<int> d_ddlist;             // the verify step's flagged units, [0] = count, list from [1]
  // ewh_refine_stats since the last query: 64-bit device counters [0] units
  // chol_dd_kernel refactored, [1] units that took the double-double route --
  // counted in stream order by the verify kernel (or, kernel mode 29, by
  // count_units_kernel), so graph replays count and captures do not
  unsigned long long* d_ddstat = nullptr;
  int n_delay_psr = 0;
  // conditional GP (ewh_cond_gp; set on its first call): the chunk scratch
  // covers every pulsar, and a fixed-white-noise handle keeps every pulsar's
  // full-width Gram, w and beta (setup_fixed), not the delay pulsars' alone
  bool cond_all = false;
  struct CondChunk {
    Buf<double> d_theta, d_z, d_x, d_coef, d_V, d_Y;
    Buf<int> d_status, d_grp;
    void release() {
      for (auto* b : {&d_theta, &d_z, &d_x, &d_coef, &d_V, &d_Y}) b->release();
      d_status.release();
      d_grp.release();
    }
  } cond;
  // joint conditional GP (ewh_cond_joint, cond_joint.hip), beside `cond`: the
  // chunk's retained factored slots (chunk x sum_p ld_p^2), the compact S
  // blocks, Sigma_c's right-hand side and solution, the chunk's normals, the
  // own blocks' status (P x chunk) and the per-sample failure flag; the
  // pulsars' common-column offsets into a row of z, and the column groups in
  // the device layout (sum_p m).  A failed allocation releases the group
  struct JointChunk {
    Buf<double> d_L, d_S, d_rhs, d_xc, d_z;
    Buf<int> d_pstat, d_sfail, d_cstart, d_grp;
    void release() {
      for (auto* b : {&d_L, &d_S, &d_rhs, &d_xc, &d_z}) b->release();
      for (auto* b : {&d_pstat, &d_sfail, &d_cstart, &d_grp}) b->release();
    }
  } joint;
  int chunk_cap = 0;        // largest chunk the ~1.5 GB scratch budget allows
  int last_B = 0;
  // correlated common process (fixed white noise)
  bool corr = false;
  int nc = 0, keep = 0, Np = 0;
  double* d_orf = nullptr;
  DSpec* d_cspec = nullptr;
  int* d_cuniq = nullptr;     // distinct M_g: representative common column per slot
  int* d_crep = nullptr;      // common column -> slot
  int nuniq = 0;
  CommonPsr* d_cps = nullptr;
  // the term form (ABI 9): matrices, coefficients, distinct spectrum sets
  double* d_tmat = nullptr;
  ewh_pref* d_tcoef = nullptr;
  DSpec* d_tspec = nullptr;
  int* d_tset = nullptr;
  CommonTerms cterms;         // n_term = 0: the legacy pair d_orf / d_cspec
  Buf<double> d_keep;         // the pulsars' kept common blocks (reserve_keep)
  // per-chunk scratch of the dense cross-pulsar factorisation
  // (reserve_common_scratch): sized for `cchunk` samples
  struct CorrChunk {
    Buf<double> d_minv, d_mlog, d_dense, d_wbuf, d_cldet, d_cq;
    Buf<int> d_cfail;
    int cchunk = 0;
    void release() {
      for (auto* b : {&d_minv, &d_mlog, &d_dense, &d_wbuf, &d_cldet, &d_cq}) b->release();
      d_cfail.release();
      cchunk = 0;
    }
  } cor;
  int cchunk_cap = 0;        // samples the dense Sigma_c budget allows per chunk
  int n_param_desc = 0;
  bool osmode = false;        // EWH_COMMON_OPTSTAT handle (ewh_optstat only)
  // captured ewh_lnl_batch sequences (H2D, launches, D2H) per batch size:
  // a sampler's single-theta calls replay one graph instead of ~5 API calls
  struct Graph {
    int B, mode;
    const void *ht, *ho;
    hipGraphExec_t exec;
    long long last_use;
  };
  std::vector<Graph> graphs;
  long long graph_clock = 0;
  // latency path of small single-device batches (chol_lat.hip): every pulsar
  // has the same reduced block count lat_nb <= LAT_NB_MAX (0: not eligible)
  int lat_nb = 0;
  // the dead k-slices of block row 0 every pulsar's frame has (ewarp_dev.h front_dead)
  int lat_dead = 0;
  // correlated process: a second stream on which the M_g inverses of the
  // first sample chunk run beside the per-pulsar partial factorisations
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  // multi-context batches: the theta entries this context's units read,
  // packed in pinned host memory (h_stage), copied to d_stage and scattered
  // into d_theta by expand_theta_kernel along the segment table d_seg
  Buf<double> h_stage{nullptr, 0, MemKind::PinnedPortable};
  Buf<int> h_seg{nullptr, 0, MemKind::PinnedPortable};
  Buf<double> d_stage;
  Buf<int> d_seg;
};

// captured graphs hold device pointers: any (re)allocation invalidates them
inline void drop_graphs(DevCtx* h) {
  for (auto& g : h->graphs) (void)hipGraphExecDestroy(g.exec);
  h->graphs.clear();
}

// a persistent block of the context (freed by destroy_ctx)
template <typename T>
int dalloc(DevCtx* h, T** p, size_t count) {
  return h->mem.alloc(p, count);
}

template <typename T>
int dupload(DevCtx* h, T** p, const T* src, size_t count) {
  int rc = dalloc(h, p, count);
  if (rc) return rc;
  if (count) EWH_HIP(hipMemcpy(*p, src, count * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}

// the timing-model projection of one pulsar's basis (ewarp_setup.hip, projection_coef)
struct ProjCoef {
  int nl = 0;
  std::vector<int> cols;     // projected basis columns (the residual is cols.size()-th)
  std::vector<double> C;     // nl x (cols.size() + 1), row-major
};

// ---- ewarp_setup.hip
int validate(const ewh_pta_desc* d);
ProjCoef projection_coef(const ewh_pulsar_desc& s);
int create_ctx(const ewh_pta_desc* d, const std::vector<ProjCoef>& proj, int device, DevCtx** out);
void destroy_ctx(DevCtx* h);
int setup_fixed(DevCtx* h);
// ---- ewarp_hip.hip: the dynamic-LDS attribute of chol_lds_kernel on the current device
int set_lds_attributes();

}  // namespace ewh_host

// The handle: one DevCtx per device of the node (a full replica of the PTA in
// each device's HBM -- C3 is 0.5 GB of bases against 288 GB), plus pinned
// host staging shared by all of them.
struct ewh_handle {
  std::vector<ewh_host::DevCtx*> ctx;
  int P = 0, n_param = 0;
  bool corr = false;
  // pinned host staging: theta rows, and the outputs / unit terms
  ewh_mem::Buf<double> h_theta{nullptr, 0, ewh_mem::MemKind::PinnedCoherent};
  ewh_mem::Buf<double> h_out{nullptr, 0, ewh_mem::MemKind::PinnedCoherent};
  // last ewh_lnl_batch split: per context, unit range (uncorrelated) or
  // sample range (correlated)
  std::vector<std::pair<long long, long long>> last_split;
  int last_B = 0;
  // multi-context fold on the first context's device: per-context partial
  // B-vectors (peer-copied in), and one event per context
  ewh_mem::Buf<double> d_part;
  std::vector<hipEvent_t> ev;
  // latency path: device addresses of h_theta / h_out (for the host pointers
  // recorded; a reallocation clears the record -- a new buffer may reuse the
  // address -- through these hooks)
  const double *lat_th_host = nullptr, *lat_out_host = nullptr;
  double *lat_th_dev = nullptr, *lat_out_dev = nullptr;
  static void forget(void* rec) { *(const double**)rec = nullptr; }
  ewh_mem::Hook th_changed{forget, &lat_th_host}, out_changed{forget, &lat_out_host};
  // theta columns each pulsar's units read (white-noise slots, spectra,
  // chromatic index groups; a correlated process's common spectra)
  std::vector<std::vector<int>> psr_cols;
  // ewh_transfer_stats: theta bytes host -> device of the last batch, and the
  // contexts with peer access to the first one
  long long h2d_bytes = 0;
  long long peer_mask = 1;
  // peer-access directions (from, to) this handle holds a reference on
  // (peer_acquire); released in ewh_destroy
  std::vector<std::pair<int, int>> peer_held;
};
