// ewarp_setup.hip — building and destroying one device's context of the C ABI
// (ewarp_ctx.h): descriptor validation, the CSR builders of the spectral
// entries, the timing-model projection, create_ctx (every table and T_aug on
// the device), setup_fixed (the fixed-white-noise cache: Gram, timing-model
// elimination), setup_common (the correlated common process's tables) and
// destroy_ctx.  Host code only: the kernels it launches are behind the
// launch_* wrappers of ewarp_launch.h.
#include "ewarp_ctx.h"
#include "ewarp_desc.h"

#include <map>

using namespace ewh_host;

namespace {

int nb_for(int cols_with_r) { return (cols_with_r + 15) / 16; }

bool pref_uses_theta(const ewh_pref& r) { return r.idx >= 0; }

DSpec to_dspec(const ewh_spec_entry& e, int col) {
  DSpec d{};
  d.kind = e.kind;
  d.col = col;
  d.i0 = e.p0.idx; d.i1 = e.p1.idx; d.i2 = e.p2.idx;
  d.v0 = e.p0.cval; d.v1 = e.p1.cval; d.v2 = e.p2.cval;
  d.f = e.f;
  d.lnf = e.f > 0 ? std::log(e.f) : 0.0;
  d.lnfyr = e.fyr > 0 ? std::log(e.fyr) : 0.0;
  d.a = e.df > 0 ? std::log(e.df / (12.0 * M_PI * M_PI)) : 0.0;
  return d;
}

// CSR over columns [c0, c1) re-indexed to start at 0 (caller's entry order kept per column).
void build_csr(const ewh_pulsar_desc& s, int c0, int c1, std::vector<int>& ptr, std::vector<DSpec>& ent) {
  const int n = c1 - c0;
  ptr.assign(n + 1, 0);
  for (int e = 0; e < s.n_spec; ++e)
    if (s.spec[e].col >= c0 && s.spec[e].col < c1) ptr[s.spec[e].col - c0 + 1]++;
  for (int j = 0; j < n; ++j) ptr[j + 1] += ptr[j];
  ent.assign(ptr[n], DSpec{});
  std::vector<int> fill(ptr.begin(), ptr.end() - 1);
  for (int e = 0; e < s.n_spec; ++e) {
    const int cc = s.spec[e].col;
    if (cc >= c0 && cc < c1) ent[fill[cc - c0]++] = to_dspec(s.spec[e], cc - c0);
  }
}

// CSR over T_aug positions for the correlated varying-white-noise layout:
// basis column c at pos(c), and a CONST phi = 1 entry on each internal pad
// position [pad0, pad1) (an identity row / column: pivot 1, log phi 0)
void build_csr_mapped(const ewh_pulsar_desc& s, const std::vector<int>& pos, int ncols, int pad0, int pad1,
                      std::vector<int>& ptr, std::vector<DSpec>& ent) {
  ptr.assign(ncols + 1, 0);
  for (int e = 0; e < s.n_spec; ++e) ptr[pos[s.spec[e].col] + 1]++;
  for (int a = pad0; a < pad1; ++a) ptr[a + 1]++;
  for (int j = 0; j < ncols; ++j) ptr[j + 1] += ptr[j];
  ent.assign(ptr[ncols], DSpec{});
  std::vector<int> fill(ptr.begin(), ptr.end() - 1);
  for (int e = 0; e < s.n_spec; ++e) {
    const int a = pos[s.spec[e].col];
    ent[fill[a]++] = to_dspec(s.spec[e], a);
  }
  for (int a = pad0; a < pad1; ++a) {
    ewh_spec_entry one{};
    one.kind = EWH_SPEC_CONST;
    one.col = a;
    one.p0 = ewh_pref{-1, 0, 1.0};
    one.p1 = ewh_pref{-1, 0, 0.0};
    one.p2 = ewh_pref{-1, 0, 0.0};
    ent[fill[a]++] = to_dspec(one, a);
  }
}

// CSR over the fixed (reduced) layout's fx_ld positions: basis column c >=
// nlead lands at c - nlead (own) or gstart + (c - nlead - nloc) (common).
void build_csr_fixed(const ewh_pulsar_desc& s, int nlead, int nloc, int gstart, int fx_ld, std::vector<int>& ptr,
                     std::vector<DSpec>& ent) {
  auto pos = [&](int c) { return c - nlead < nloc ? c - nlead : gstart + (c - nlead - nloc); };
  ptr.assign(fx_ld + 1, 0);
  for (int e = 0; e < s.n_spec; ++e)
    if (s.spec[e].col >= nlead) ptr[pos(s.spec[e].col) + 1]++;
  for (int j = 0; j < fx_ld; ++j) ptr[j + 1] += ptr[j];
  ent.assign(ptr[fx_ld], DSpec{});
  std::vector<int> fill(ptr.begin(), ptr.end() - 1);
  for (int e = 0; e < s.n_spec; ++e) {
    const int cc = s.spec[e].col;
    if (cc >= nlead) ent[fill[pos(cc)]++] = to_dspec(s.spec[e], pos(cc));
  }
}

// columns of a CSR whose spectral entries equal (all fields but `col`, bit
// for bit, same order) those of an earlier column: rep[a] = that column (a
// itself when first or without entries); ulist = the first columns with
// entries.  The sin / cos columns of one frequency share a spectrum.
void build_spec_rep(const std::vector<int>& ptr, const std::vector<DSpec>& ent, std::vector<int>& rep,
                    std::vector<int>& ulist) {
  const int ncol = (int)ptr.size() - 1;
  rep.assign(ncol, 0);
  ulist.clear();
  std::map<std::string, int> first;
  for (int a = 0; a < ncol; ++a) {
    rep[a] = a;
    if (ptr[a] == ptr[a + 1]) continue;
    std::string key;
    for (int e = ptr[a]; e < ptr[a + 1]; ++e) {
      DSpec d = ent[e];
      const int f[5] = {d.kind, d.i0, d.i1, d.i2, 0};
      const double v[7] = {d.v0, d.v1, d.v2, d.a, d.lnf, d.lnfyr, d.f};
      key.append((const char*)f, sizeof f);
      key.append((const char*)v, sizeof v);
    }
    auto it = first.find(key);
    if (it == first.end()) {
      first.emplace(key, a);
      ulist.push_back(a);
    } else {
      rep[a] = it->second;
    }
  }
}

// X' = X - M C on T_aug (row-major, leading dimension ld, residual at ld-1),
// formed in double-double (round 6): TwoProd of each M_ta C_ak (by fma) and
// TwoSum into (s, e), so s + e = X - M C to ~2^-106; T_aug takes the rounded
// value fl(s + e) and, when lo is given, lo takes the residual (s + e) -
// fl(s + e), the part of the exact projection that the fp64 T_aug drops
// (rounds 2-5: one fma chain, its rounding -- up to eps |M C|, cancellation
// included -- entered every Gram)
void apply_projection(const ProjCoef& pc, int n_toa, int ld, std::vector<double>& Ta, std::vector<double>* lo) {
#pragma clang fp contract(off)
  const int nl = pc.nl, nc = (int)pc.cols.size() + 1;
  if (nl == 0) return;
  for (int t = 0; t < n_toa; ++t) {
    double* row = &Ta[(size_t)t * ld];
    for (int k = 0; k < nc; ++k) {
      const int col = k < nc - 1 ? pc.cols[k] : ld - 1;
      double hs = row[col], es = 0.0;
      for (int a = 0; a < nl; ++a) {
        const double p = -row[a] * pc.C[(size_t)a * nc + k];
        const double pe = std::fma(-row[a], pc.C[(size_t)a * nc + k], -p);   // -M C = p + pe exactly
        const double sum = hs + p, bp = sum - hs;
        es += ((hs - (sum - bp)) + (p - bp)) + pe;                           // TwoSum error + product error
        hs = sum;
      }
      const double v = hs + es;
      row[col] = v;
      if (lo) (*lo)[(size_t)t * ld + col] = (hs - v) + es;                   // (hs - v exact: v ~ hs)
    }
  }
}

int setup_common(DevCtx* h, const ewh_pta_desc* d) {
  const ewh_common_desc& c = *d->common;
  const int P = h->P;
  h->corr = true;
  h->nc = c.n_col;
  h->keep = (c.n_col + 1 + 15) / 16;
  for (auto& ps : h->psr) {
    const int nbk = h->white_fixed ? ps.fx_nb : ps.nb;
    const int gs = h->white_fixed ? ps.gstart : ps.gstart_v;
    if (nbk - gs / 16 != h->keep) return set_err(EWH_E_INVALID, "common: inconsistent reduced layout");
    if (nbk > WIDE_NB_MAX) return set_err(EWH_E_UNSUPPORTED, "common: basis wider than 1023 columns");
  }
  int rc;
  // per pulsar: the CSR whose positions gstart.. hold the common columns'
  // own entries (fixed white noise: the reduced layout; varying: T_aug's)
  auto common_psr = [&](int p) {
    const PsrHost& ps = h->psr[p];
    return h->white_fixed ? CommonPsr{ps.d_fx_colptr, ps.d_fx_spec, ps.gstart, 0}
                          : CommonPsr{ps.d_colptr, ps.d_spec, ps.gstart_v, 0};
  };
  if (h->osmode) {               // optimal statistic: the CURN likelihood layout + the ORF only
    h->corr = false;
    if ((rc = dupload(h, &h->d_orf, c.orf, (size_t)P * P))) return rc;
    std::vector<CommonPsr> cps(P);
    for (int p = 0; p < P; ++p) cps[p] = common_psr(p);
    return dupload(h, &h->d_cps, cps.data(), cps.size());
  }
  auto same_ent = [](const ewh_spec_entry& x, const ewh_spec_entry& y) {
    auto pr = [](const ewh_pref& a, const ewh_pref& b) { return a.idx == b.idx && a.cval == b.cval; };
    return x.kind == y.kind && pr(x.p0, y.p0) && pr(x.p1, y.p1) && pr(x.p2, y.p2) && x.f == y.f && x.df == y.df &&
           x.fyr == y.fyr;
  };
  // The spectrum sets M_g is built from, once per distinct content: the
  // legacy pair has one; in the term form the terms of one process (a sampled
  // ORF's identity and bin terms) share theirs.  One term with the constant
  // coefficient 1 is the legacy pair and takes the legacy kernels.
  const bool legacy = c.n_term == 0 || (c.n_term == 1 && c.terms[0].coef.idx < 0 && c.terms[0].coef.cval == 1.0);
  std::vector<const ewh_spec_entry*> sets;
  if (legacy) {
    sets.push_back(c.n_term ? c.terms[0].spec : c.spec);
    if ((rc = dupload(h, &h->d_orf, c.n_term ? c.terms[0].mat : c.orf, (size_t)P * P))) return rc;
    std::vector<DSpec> cs(c.n_col);
    for (int g = 0; g < c.n_col; ++g) cs[g] = to_dspec(sets[0][g], g);
    if ((rc = dupload(h, &h->d_cspec, cs.data(), cs.size()))) return rc;
  } else {
    std::vector<int> set(c.n_term);
    std::vector<double> mats((size_t)c.n_term * P * P);
    std::vector<ewh_pref> coef(c.n_term);
    for (int t = 0; t < c.n_term; ++t) {
      int found = -1;
      for (size_t u = 0; u < sets.size() && found < 0; ++u) {
        bool eq = true;
        for (int g = 0; g < c.n_col && eq; ++g) eq = same_ent(c.terms[t].spec[g], sets[u][g]);
        if (eq) found = (int)u;
      }
      if (found < 0) {
        found = (int)sets.size();
        sets.push_back(c.terms[t].spec);
      }
      set[t] = found;
      coef[t] = c.terms[t].coef;
      std::copy(c.terms[t].mat, c.terms[t].mat + (size_t)P * P, mats.begin() + (size_t)t * P * P);
    }
    std::vector<DSpec> ts(sets.size() * (size_t)c.n_col);
    for (size_t u = 0; u < sets.size(); ++u)
      for (int g = 0; g < c.n_col; ++g) ts[u * c.n_col + g] = to_dspec(sets[u][g], g);
    if ((rc = dupload(h, &h->d_tmat, mats.data(), mats.size())) ||
        (rc = dupload(h, &h->d_tcoef, coef.data(), coef.size())) ||
        (rc = dupload(h, &h->d_tspec, ts.data(), ts.size())) || (rc = dupload(h, &h->d_tset, set.data(), set.size())))
      return rc;
    h->cterms.n_term = c.n_term;
    h->cterms.mat = h->d_tmat;
    h->cterms.coef = h->d_tcoef;
    h->cterms.spec = h->d_tspec;
    h->cterms.set = h->d_tset;
  }
  // columns whose M_g is identical (the sin / cos pair of a frequency: the
  // same entry in every spectrum set, same own spectra in every pulsar) share
  // one inverse
  auto own_entries = [&](int p, int g) {
    const ewh_pulsar_desc& sd = d->pulsars[p];
    const int col = sd.n_col - sd.n_common + g;
    std::vector<ewh_spec_entry> v;
    for (int e = 0; e < sd.n_spec; ++e)
      if (sd.spec[e].col == col) v.push_back(sd.spec[e]);
    return v;
  };
  std::vector<int> uniq, rep(c.n_col);
  for (int g = 0; g < c.n_col; ++g) {
    int found = -1;
    for (size_t u = 0; u < uniq.size() && found < 0; ++u) {
      const int g2 = uniq[u];
      bool eq = true;
      for (size_t q = 0; q < sets.size() && eq; ++q) eq = same_ent(sets[q][g], sets[q][g2]);
      for (int p = 0; p < P && eq; ++p) {
        const auto a = own_entries(p, g), b = own_entries(p, g2);
        eq = a.size() == b.size();
        for (size_t k = 0; k < a.size() && eq; ++k) eq = same_ent(a[k], b[k]);
      }
      if (eq) found = (int)u;
    }
    if (found < 0) {
      found = (int)uniq.size();
      uniq.push_back(g);
    }
    rep[g] = found;
  }
  h->nuniq = (int)uniq.size();
  if ((rc = dupload(h, &h->d_cuniq, uniq.data(), uniq.size()))) return rc;
  if ((rc = dupload(h, &h->d_crep, rep.data(), rep.size()))) return rc;
  std::vector<CommonPsr> cps(P);
  for (int p = 0; p < P; ++p) cps[p] = common_psr(p);
  if ((rc = dupload(h, &h->d_cps, cps.data(), cps.size()))) return rc;
  h->Np = DCB * ((P * h->nc + 1 + DCB - 1) / DCB);
  // the dense kernels address a sample's Sigma_c by 32-bit byte offsets
  // (dchol_rowpair_kernel, dchol_rowupdate2_kernel): < 4 GB per sample
  if ((double)h->Np * h->Np * 8.0 >= 4294967296.0)
    return set_err(EWH_E_UNSUPPORTED, "correlated common process: Sigma_c of " + std::to_string(h->Np) +
                                          " columns exceeds 4 GB per sample (P x common columns <= 23168)");
  const double per = (double)h->Np * h->Np * 8.0;
  h->cchunk_cap = (int)std::max(1.0, std::min(1024.0, 40.0e9 / per));   // <= 40 GB of dense Sigma_c per chunk
  h->cor.cchunk = 0;              // the chunk scratch is allocated on first use, sized to the batch
  EWH_HIP(set_minv_attributes(P));
  return 0;
}

}  // namespace

namespace ewh_host {

int validate(const ewh_pta_desc* d) {
  std::string msg;
  const int rc = ewh_desc::desc_check(d, msg);
  return rc ? set_err(rc, msg) : 0;
}

// Fixed white noise: G = T_aug^T N^-1 T_aug of every pulsar at the constant
// white-noise values, then the timing-model elimination (schur_kernel) into
// the cached reduced matrix S_p and constant K_p.  Called by create and again
// by ewh_set_fixed_white (new constants, same layout: buffers are reused).
int setup_fixed(DevCtx* h) {
  int rc;
  size_t maxn = 1, maxe = 1, maxld = 16;
  for (auto& ps : h->psr) {
    maxn = std::max(maxn, (size_t)ps.n_toa);
    maxe = std::max(maxe, (size_t)ps.n_epoch);
    maxld = std::max(maxld, (size_t)ps.ld);
  }
  Arena tmp;                    // this step's scratch, freed on return
  double *w, *beta, *s, *G, *Glo, *Kb, *dummy_theta;
  if ((rc = tmp.alloc(&w, maxn)) || (rc = tmp.alloc(&beta, maxe)) || (rc = tmp.alloc(&s, maxe * maxld)) ||
      (rc = tmp.alloc(&G, maxld * maxld)) || (rc = tmp.alloc(&Glo, maxld * maxld)) || (rc = tmp.alloc(&Kb, 1)) ||
      (rc = tmp.alloc(&dummy_theta, (size_t)std::max(1, h->n_param))))
    return rc;
  // theta is never read (every white-noise slot is constant)
  EWH_HIP(hipMemsetAsync(dummy_theta, 0, sizeof(double) * std::max(1, h->n_param), h->stream));
  if (!h->d_fxK && (rc = dalloc(h, &h->d_fxK, h->P))) return rc;
  if (!h->d_fxfail && (rc = dalloc(h, &h->d_fxfail, h->P))) return rc;
  // mreal: columns that take phi^-1 in the factorisation -- the own columns
  // (correlated: the common block is assembled globally), or every column
  // with entries (optimal statistic: the CURN Sigma of each pulsar)
  auto mreal_of = [&](const PsrHost& ps) { return h->osmode ? ps.fx_ld - 1 : ps.nloc; };
  if (!h->d_images) {
    // the operand images of every pulsar the register kernel takes, in one
    // block ahead of the matrices (so the cached S_p lie as close together as
    // without them: the latency path reads all of them in one launch): the
    // stored order, and the front-pad order where the frame has a dead slice
    size_t tot = 0;
    for (const auto& ps : h->psr)
      if (ps.fx_nb <= MFMA_NB_MAX)
        tot += (size_t)img_doubles(ps.fx_nb) * (front_dead(ps.fx_ld, mreal_of(ps)) >= 1 ? 2 : 1);
    if ((rc = dalloc(h, &h->d_images, tot))) return rc;
    double* at = h->d_images;
    for (auto& ps : h->psr) {
      if (ps.fx_nb > MFMA_NB_MAX) continue;
      ps.d_img = at;
      at += img_doubles(ps.fx_nb);
      if (front_dead(ps.fx_ld, mreal_of(ps)) >= 1) {
        ps.d_imgf = at;
        at += img_doubles(ps.fx_nb);
      }
    }
  }
  std::vector<CholJob> jobs(h->P);
  std::vector<int> fails(h->P, 0);
  for (int p = 0; p < h->P; ++p) {
    PsrHost& ps = h->psr[p];
    launch_wn_weights(ps.dev, dummy_theta, 0, 0, 1, w, beta, Kb, nullptr, nullptr, h->stream);
    if (ps.n_epoch > 0) launch_epoch_sums(ps.dev, ps.n_epoch, ps.max_epoch, false, w, nullptr, s, 1, h->stream);
    if (ps.dev.n_bgroup == 0 && h->plan.fixed_gram_dd) {
      // (the exactly projected basis: T_aug + its projection residual d_Tlo;
      // the epoch sums formed inside from both)
      launch_gram_dd(ps.dev, ps.nb, ps.d_Tlo, w, beta, G, Glo, h->stream);
      EWH_HIP(hipGetLastError());
    } else {
      EWH_HIP(hipMemsetAsync(Glo, 0, sizeof(double) * (size_t)ps.ld * ps.ld, h->stream));
      if ((rc = launch_contract_nb(ps.nb, ps.dev, w, beta, s, nullptr, G, 1, h->stream))) return rc;
    }
    if (ps.delay.n_delay > 0 || h->cond_all) {
      // a delay pulsar keeps the full-width Gram (before the elimination
      // below), w and beta: per sample only its residual column is formed
      // (run_delay), T^T N^-1 T is broadcast from here; after the first
      // ewh_cond_gp every pulsar does (the conditional GP factors the
      // full-width matrix)
      const size_t g2 = (size_t)ps.ld * ps.ld;
      if ((!ps.d_Gf && (rc = dalloc(h, &ps.d_Gf, g2))) || (!ps.d_Gflo && (rc = dalloc(h, &ps.d_Gflo, g2))) ||
          (!ps.d_wf && (rc = dalloc(h, &ps.d_wf, (size_t)ps.n_toa))) ||
          (!ps.d_betaf && (rc = dalloc(h, &ps.d_betaf, (size_t)ps.n_epoch))))
        return rc;
      EWH_HIP(hipMemcpyAsync(ps.d_Gf, G, sizeof(double) * g2, hipMemcpyDeviceToDevice, h->stream));
      EWH_HIP(hipMemcpyAsync(ps.d_Gflo, Glo, sizeof(double) * g2, hipMemcpyDeviceToDevice, h->stream));
      EWH_HIP(hipMemcpyAsync(ps.d_wf, w, sizeof(double) * ps.n_toa, hipMemcpyDeviceToDevice, h->stream));
      if (ps.n_epoch > 0)
        EWH_HIP(hipMemcpyAsync(ps.d_betaf, beta, sizeof(double) * ps.n_epoch, hipMemcpyDeviceToDevice, h->stream));
    }
    double Kb_h = 0.0;
    EWH_HIP(hipMemcpyAsync(&Kb_h, Kb, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    EWH_HIP(hipStreamSynchronize(h->stream));
    ps.fxKb = Kb_h;
    if (!ps.d_S && (rc = dalloc(h, &ps.d_S, (size_t)ps.fx_ld * ps.fx_ld))) return rc;
    // the low part of S for the double-double factorisation: bases past the
    // register kernels (dd_path), and (round 6) every unit whose fp64
    // factorisation fails (refine_failed)
    if (!ps.d_Slo && (rc = dalloc(h, &ps.d_Slo, (size_t)ps.fx_ld * ps.fx_ld))) return rc;
    if (ps.d_Slo && !ps.d_Srev && (rc = dalloc(h, &ps.d_Srev, (size_t)ps.fx_ld * ps.fx_ld))) return rc;
    launch_schur(G, Glo, ps.ld, ps.m, ps.nlead, ps.d_colptr, ps.d_spec, Kb_h, ps.d_S, ps.fx_ld, ps.nloc, ps.gstart,
                 ps.ncommon, h->d_fxK + p, h->d_fxfail + p, ps.d_Slo, h->stream);
    EWH_HIP(hipGetLastError());
    const int mreal = mreal_of(ps);
    jobs[p] = CholJob{ps.d_S, 0, ps.fx_ld, mreal, ps.d_fx_colptr, ps.d_fx_spec, h->d_fxK + p, 0, 0,
                      ps.d_fx_rep, ps.d_fx_ulist, ps.fx_nu, h->stage_spectra ? ps.d_fx_urec : nullptr, ps.d_fx_urep};
    jobs[p].mats_lo = ps.d_Slo;
    if (ps.d_Slo) {          // the reversed verify pass's input, once (chol_wide.hip)
      launch_rev_input(ps.d_S, ps.d_Slo, ps.d_Srev, (long long)ps.fx_ld * ps.fx_ld, h->stream);
      EWH_HIP(hipGetLastError());
      jobs[p].mats_rev = ps.d_Srev;
    }
    if (ps.d_img) {
      // the register kernel's operand images of the new S, once (ewarp_dev.h
      // img_index): the stored order, and the front-pad order of this job's
      // own pad count where it has one -- the launch picks (dispatch_chol)
      launch_operand_image(ps.d_S, ps.fx_nb, front_pads(ps.fx_ld, mreal), ps.d_img, ps.d_imgf, h->stream);
      EWH_HIP(hipGetLastError());
      jobs[p].img = ps.d_img;
      jobs[p].img_front = ps.d_imgf;
    }
    if (jobs[p].urec != nullptr) {
      jobs[p].ntidx = (int)ps.fx_tidx.size();
      for (int i = 0; i < jobs[p].ntidx; ++i) jobs[p].tidx[i] = ps.fx_tidx[i];
      // (the launch picks the prologue: launch_register)
      jobs[p].pl = ps.d_fx_pl;
      jobs[p].pl_ne = ps.fx_pl_ne;
    }
  }
  EWH_HIP(hipMemcpyAsync(fails.data(), h->d_fxfail, sizeof(int) * h->P, hipMemcpyDeviceToHost, h->stream));
  EWH_HIP(hipStreamSynchronize(h->stream));
  for (int p = 0; p < h->P; ++p) jobs[p].fail = fails[p];
  EWH_HIP(hipMemcpy(h->d_jobs_fixed, jobs.data(), sizeof(CholJob) * h->P, hipMemcpyHostToDevice));
  return 0;
}

void destroy_ctx(DevCtx* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  drop_graphs(h);
  h->h_stage.release();
  h->h_seg.release();
  if (h->side) (void)hipStreamSynchronize(h->side);
  for (auto* b : {&h->d_units, &h->d_theta, &h->d_bigscr, &h->d_widescr, &h->d_ddscr, &h->d_units2, &h->d_keep,
                  &h->d_stage})
    b->release();
  h->d_ddlist.release();
  h->d_seg.release();
  h->var.release();
  h->cond.release();
  h->joint.release();
  h->cor.release();
  h->mem.release();
  if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
  if (h->ev_join) (void)hipEventDestroy(h->ev_join);
  if (h->side) (void)hipStreamDestroy(h->side);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

// Timing-model projection of one pulsar's basis.  Every
// basis column that does not depend on theta, and the residual, loses its
// least-squares component along the leading constant-phi (timing-model)
// columns M under the weights 1/sigma^2:
//   X' = X - M C,   C = (M^T W0 M)^-1 M^T W0 X.
// With phi_M = 1e40 this is an exact reparametrisation of the same
// likelihood: the timing-model coefficients absorb M C b (prior ~ flat), so
// lnL, log|Sigma| and the quadratic form change by O(|C|^2 / phi_M) ~ 1e-36
// relative, and log|phi| is untouched (the map is unit triangular).  What it
// removes is the cancellation: the low-frequency Fourier columns lie close
// to the span of the spin-down / astrometric columns, so in the original
// basis the timing-model elimination subtracts two nearly equal Gram blocks
// (~1e14 each) and fp64 rounding of the Gram -- or an asymmetric panel --
// was amplified into the prior-draw lnL (tests/golden, c2_small: 7e5x the
// strict bound).  C needs no special accuracy: any C is an exact
// reparametrisation; only X' = X - M C is rounded (once, by fma), a
// perturbation of X of O(eps |X|) -- the size of X's own representation.
// Computed once per handle (ProjCoef), applied when T_aug is built.
ProjCoef projection_coef(const ewh_pulsar_desc& s) {
  ProjCoef pc;
  const int nl = s.n_lead_const, n = s.n_toa;
  if (nl <= 0 || nl >= s.n_col + 1) return pc;
  for (int j = nl; j < s.n_col; ++j)
    if (s.n_bgroup == 0 || s.col_bgroup[j] < 0) pc.cols.push_back(j);
  const int nc = (int)pc.cols.size() + 1;
  std::vector<double> G0((size_t)nl * nl, 0.0), Bm((size_t)nl * nc, 0.0), x(nc);
  for (int t = 0; t < n; ++t) {
    const double* row = s.basis + (size_t)t * s.n_col;
    const double w0 = 1.0 / (s.toaerr[t] * s.toaerr[t]);
    for (int k = 0; k < nc - 1; ++k) x[k] = row[pc.cols[k]];
    x[nc - 1] = s.resid[t];
    for (int a = 0; a < nl; ++a) {
      const double wa = w0 * row[a];
      if (wa == 0.0) continue;
      for (int b = 0; b < nl; ++b) G0[(size_t)a * nl + b] += wa * row[b];
      double* br = &Bm[(size_t)a * nc];
      for (int k = 0; k < nc; ++k) br[k] += wa * x[k];
    }
  }
  // Cholesky of G0; a column of M with (numerically) no weight of its own --
  // e.g. a zero-norm design-matrix column -- is left out of the projection
  double dmax = 0.0;
  for (int a = 0; a < nl; ++a) dmax = std::max(dmax, G0[(size_t)a * nl + a]);
  std::vector<double> L((size_t)nl * nl, 0.0);
  std::vector<char> use(nl, 0);
  for (int k = 0; k < nl; ++k) {
    double v = G0[(size_t)k * nl + k];
    for (int j = 0; j < k; ++j) v -= L[(size_t)k * nl + j] * L[(size_t)k * nl + j];
    if (!(v > 1e-12 * dmax)) continue;
    use[k] = 1;
    const double lkk = std::sqrt(v);
    L[(size_t)k * nl + k] = lkk;
    for (int i = k + 1; i < nl; ++i) {
      double u = G0[(size_t)i * nl + k];
      for (int j = 0; j < k; ++j) u -= L[(size_t)i * nl + j] * L[(size_t)k * nl + j];
      L[(size_t)i * nl + k] = u / lkk;
    }
  }
  // C = G0^-1 Bm over the used columns (forward, then back substitution)
  pc.nl = nl;
  pc.C.assign((size_t)nl * nc, 0.0);
  for (int k = 0; k < nc; ++k) {
    std::vector<double> y(nl, 0.0);
    for (int i = 0; i < nl; ++i) {
      if (!use[i]) continue;
      double v = Bm[(size_t)i * nc + k];
      for (int j = 0; j < i; ++j) v -= L[(size_t)i * nl + j] * y[j];
      y[i] = v / L[(size_t)i * nl + i];
    }
    for (int i = nl - 1; i >= 0; --i) {
      if (!use[i]) continue;
      double v = y[i];
      for (int j = i + 1; j < nl; ++j) v -= L[(size_t)j * nl + i] * pc.C[(size_t)j * nc + k];
      pc.C[(size_t)i * nc + k] = v / L[(size_t)i * nl + i];
    }
  }
  return pc;
}

// One device's copy of the PTA (every table, the fixed-WN cache, scratch).
int create_ctx(const ewh_pta_desc* d, const std::vector<ProjCoef>& proj, int device, DevCtx** out) {
  *out = nullptr;
  int rc;
  EWH_HIP(hipSetDevice(device));
  DevCtx* h = new DevCtx();
  h->hook = h->mem.changed = Hook{[](void* c) { drop_graphs((DevCtx*)c); }, h};
  h->device = device;
  h->P = d->n_pulsar;
  h->n_param = d->n_param;
  h->psr.resize(h->P);
  auto bail = [&](int code) {
    destroy_ctx(h);
    return code;
  };
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess)
    return bail(set_err(EWH_E_HIP, "hipStreamCreate failed"));
  if (hipDeviceGetAttribute(&h->n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || h->n_cu <= 0)
    h->n_cu = 256;
  // per device (the attributes are properties of the kernels on the current device)
  if ((rc = set_lds_attributes()) || (rc = set_contract_attributes()) || (rc = set_dd_attributes())) return bail(rc);
  bool any_theta_white = false;
  for (int p = 0; p < h->P; ++p) {
    const ewh_pulsar_desc& s = d->pulsars[p];
    for (int i = 0; i < s.n_slot; ++i) any_theta_white |= pref_uses_theta(s.slots[i]);
    any_theta_white |= s.n_bgroup > 0;
  }
  // a correlated common process with white noise varying (or a theta-dependent
  // basis): per sample, the contraction of a T_aug laid out with the common
  // columns in whole blocks, then the partial factorisation (corr_partial)
  const bool corr_var = d->common && d->common->kind == EWH_COMMON_CORRELATED &&
                        !((d->white_fixed != 0) && !any_theta_white);
  for (int p = 0; p < h->P; ++p) {
    const ewh_pulsar_desc& s = d->pulsars[p];
    PsrHost& ps = h->psr[p];
    ps.n_toa = s.n_toa;
    ps.m = s.n_col;
    ps.nlead = s.n_lead_const;
    // T_aug position of basis column j (identity, or the corr_var layout)
    std::vector<int> vpos(s.n_col);
    for (int j = 0; j < s.n_col; ++j) vpos[j] = j;
    int pad0 = 0, pad1 = 0;
    if (corr_var) {
      const int nlo = s.n_col - s.n_common;
      ps.gstart_v = 16 * ((nlo + 15) / 16);
      for (int j = nlo; j < s.n_col; ++j) vpos[j] = ps.gstart_v + (j - nlo);
      pad0 = nlo;
      pad1 = ps.gstart_v;
      ps.m = ps.gstart_v + s.n_common;
    }
    ps.nb = nb_for(ps.m + 1);
    ps.ld = 16 * ps.nb;
    ps.n_epoch = s.n_epoch;
    ps.max_epoch = 0;
    for (int e = 0; e < s.n_epoch; ++e) ps.max_epoch = std::max(ps.max_epoch, s.epoch_stop[e] - s.epoch_start[e]);
    ps.fx_m = s.n_col - s.n_lead_const;
    ps.ncommon = d->common ? s.n_common : 0;
    ps.nloc = ps.fx_m - ps.ncommon;
    if (ps.ncommon > 0) {          // [own | pad to 16 | common | pad | r]
      ps.gstart = 16 * ((ps.nloc + 15) / 16);
      ps.fx_nb = nb_for(ps.gstart + ps.ncommon + 1);
    } else {                       // [own | pad | r]
      ps.gstart = ps.nloc;
      ps.fx_nb = nb_for(ps.fx_m + 1);
    }
    ps.fx_ld = 16 * ps.fx_nb;
    for (int i = 0; i < s.n_slot; ++i) ps.has_theta_white |= pref_uses_theta(s.slots[i]);
    // T_aug: [basis | 0-pad | r], row-major n x ld
    // (+CT_ROWS zero rows: the pipelined contraction copies whole tiles)
    std::vector<double> Ta((size_t)(s.n_toa + CT_ROWS) * ps.ld, 0.0), sig2(s.n_toa);
    for (int t = 0; t < s.n_toa; ++t) {
      for (int j = 0; j < s.n_col; ++j) Ta[(size_t)t * ps.ld + j] = s.basis[(size_t)t * s.n_col + j];
      Ta[(size_t)t * ps.ld + ps.ld - 1] = s.resid[t];
      sig2[t] = s.toaerr[t] * s.toaerr[t];
    }
    // the projection residual for the double-double Grams (PsrHost::d_Tlo)
    const bool want_lo = !corr_var && s.n_bgroup == 0 && proj[p].nl > 0;
    std::vector<double> Tlo(want_lo ? Ta.size() : 0, 0.0);
    apply_projection(proj[p], s.n_toa, ps.ld, Ta, want_lo ? &Tlo : nullptr);
    if (want_lo && (rc = dupload(h, &ps.d_Tlo, Tlo.data(), Tlo.size()))) return bail(rc);
    // the projection's coefficients, kept for the conditional GP's back-map
    ps.has_proj = proj[p].nl > 0;
    ps.nproj = (int)proj[p].cols.size();
    if (ps.has_proj && !d->common) {
      if ((rc = dupload(h, &ps.d_projC, proj[p].C.data(), proj[p].C.size()))) return bail(rc);
      if ((rc = dupload(h, &ps.d_projcols, proj[p].cols.data(), proj[p].cols.size()))) return bail(rc);
    } else if (ps.has_proj && d->common->kind == EWH_COMMON_CORRELATED) {
      // (the joint conditional GP, cond_joint.hip: the projected columns at their T_aug positions)
      std::vector<int> pcols(proj[p].cols);
      for (int& j : pcols) j = vpos[j];
      if ((rc = dupload(h, &ps.d_projC, proj[p].C.data(), proj[p].C.size()))) return bail(rc);
      if ((rc = dupload(h, &ps.d_projcols, pcols.data(), pcols.size()))) return bail(rc);
    }
    if (corr_var) {       // common columns to their block-aligned positions (from the top: pos >= j)
      for (int t = 0; t < s.n_toa; ++t) {
        double* row = &Ta[(size_t)t * ps.ld];
        for (int j = s.n_col - 1; j >= pad0; --j) {
          const double v = row[j];
          row[j] = 0.0;
          row[vpos[j]] = v;
        }
      }
    }
    double* dT;
    double* dsig2;
    int *d_ef, *d_eq, *d_es, *d_ee, *d_eslot;
    ps.n_slot = s.n_slot;
    ps.slots.assign(s.slots, s.slots + s.n_slot);
    if ((rc = dupload(h, &dT, Ta.data(), Ta.size()))) return bail(rc);
    if ((rc = dupload(h, &dsig2, sig2.data(), sig2.size()))) return bail(rc);
    if ((rc = dupload(h, &d_ef, s.efac_slot, (size_t)s.n_toa))) return bail(rc);
    if ((rc = dupload(h, &d_eq, s.equad_slot, (size_t)s.n_toa))) return bail(rc);
    if ((rc = dupload(h, &ps.d_slots, s.slots, (size_t)s.n_slot))) return bail(rc);
    if ((rc = dupload(h, &d_es, s.epoch_start, (size_t)s.n_epoch))) return bail(rc);
    if ((rc = dupload(h, &d_ee, s.epoch_stop, (size_t)s.n_epoch))) return bail(rc);
    if ((rc = dupload(h, &d_eslot, s.epoch_slot, (size_t)s.n_epoch))) return bail(rc);
    std::vector<int> toa_ep((size_t)s.n_toa + CT_ROWS, -1);
    for (int e = 0; e < s.n_epoch; ++e)
      for (int t = s.epoch_start[e]; t < s.epoch_stop[e]; ++t) toa_ep[t] = 2 * e + (t == s.epoch_stop[e] - 1);
    int* d_tep;
    if ((rc = dupload(h, &d_tep, toa_ep.data(), toa_ep.size()))) return bail(rc);
    int* d_cbg = nullptr;
    double* d_lnc = nullptr;
    ewh_pref* d_bg = nullptr;
    if (s.n_bgroup > 0) {
      std::vector<int> cbg(ps.ld, -1);
      for (int j = 0; j < s.n_col; ++j) cbg[vpos[j]] = s.col_bgroup[j];
      if ((rc = dupload(h, &d_cbg, cbg.data(), cbg.size()))) return bail(rc);
      if ((rc = dupload(h, &d_bg, s.bgroup_idx, (size_t)s.n_bgroup))) return bail(rc);
    }
    if ((s.n_bgroup > 0 || s.n_delay > 0) && (rc = dupload(h, &d_lnc, s.ln_chrom, (size_t)s.n_toa))) return bail(rc);
    if (s.n_delay > 0) {
      static_assert(DELAY_MAX == 8, "ewarp_desc.h refuses more than 8 delay entries");
      std::vector<DDelay> de(s.n_delay);
      for (int k = 0; k < s.n_delay; ++k) {
        const ewh_delay_entry& e = s.delays[k];
        de[k] = DDelay{e.kind, e.p0.idx, e.p1.idx, e.p2.idx, e.p3.idx, 0,
                       e.p0.cval, e.p1.cval, e.p2.cval, e.p3.cval, e.idx};
      }
      DDelay* d_de;
      double* d_toas;
      if ((rc = dupload(h, &d_de, de.data(), de.size()))) return bail(rc);
      if ((rc = dupload(h, &d_toas, s.toas, (size_t)s.n_toa))) return bail(rc);
      ps.delay = DelayDev{s.n_delay, d_de, d_toas};
      h->n_delay_psr++;
    }
    ps.dev = PsrDev{s.n_toa, ps.m, ps.ld, ps.nb, s.n_epoch, dT, dsig2, d_ef, d_eq, ps.d_slots, d_es, d_ee, d_eslot,
                    s.n_bgroup, d_cbg, d_lnc, d_bg, d_tep};
    std::vector<int> ptr;
    std::vector<DSpec> ent;
    if (corr_var) build_csr_mapped(s, vpos, ps.m, pad0, pad1, ptr, ent);
    else build_csr(s, 0, s.n_col, ptr, ent);
    if ((rc = dupload(h, &ps.d_colptr, ptr.data(), ptr.size()))) return bail(rc);
    if ((rc = dupload(h, &ps.d_spec, ent.data(), ent.size()))) return bail(rc);
    build_csr_fixed(s, ps.nlead, ps.nloc, ps.gstart, ps.fx_ld, ptr, ent);
    if ((rc = dupload(h, &ps.d_fx_colptr, ptr.data(), ptr.size()))) return bail(rc);
    if ((rc = dupload(h, &ps.d_fx_spec, ent.data(), ent.size()))) return bail(rc);
    {
      std::vector<int> rep, ulist;
      build_spec_rep(ptr, ent, rep, ulist);
      ps.fx_nu = (int)ulist.size();
      // staged records: ulist order; urep[a] = record of column a's spectrum
      std::vector<int> urep(rep.size(), -1), uidx(rep.size(), -1);
      for (size_t u = 0; u < ulist.size(); ++u) uidx[ulist[u]] = (int)u;
      bool fits = true;
      // the fixed form of the same records, from the entries as they index
      // the theta row (before the records below are re-indexed to tidx)
      std::vector<PlRec> plrec;
      const bool compact = pl_pack(ptr, ent, ulist, h->n_param, plrec, &ps.fx_pl_ne);
      std::vector<URec> urec(std::max<size_t>(1, ulist.size()));
      for (size_t u = 0; u < ulist.size(); ++u) {
        const int a = ulist[u];
        const int ne = ptr[a + 1] - ptr[a];
        if (ne > URec::NE) fits = false;
        urec[u] = URec{};
        urec[u].ne = std::min(ne, URec::NE);
        for (int e = 0; e < urec[u].ne; ++e) urec[u].e[e] = ent[ptr[a] + e];
      }
      // the theta entries the records read: staged alone when there are at
      // most TIDX_MAX of them (the records then index that list)
      std::vector<int> tl;
      for (size_t u = 0; u < ulist.size(); ++u)
        for (int e = 0; e < urec[u].ne; ++e)
          for (int idx : {urec[u].e[e].i0, urec[u].e[e].i1, urec[u].e[e].i2})
            if (idx >= 0 && std::find(tl.begin(), tl.end(), idx) == tl.end()) tl.push_back(idx);
      std::sort(tl.begin(), tl.end());
      ps.fx_tidx.clear();
      if (fits && (int)tl.size() <= TIDX_MAX) {
        ps.fx_tidx = tl;
        auto pos = [&](int idx) { return idx < 0 ? idx : (int)(std::lower_bound(tl.begin(), tl.end(), idx) - tl.begin()); };
        for (size_t u = 0; u < ulist.size(); ++u)
          for (int e = 0; e < urec[u].ne; ++e) {
            urec[u].e[e].i0 = pos(urec[u].e[e].i0);
            urec[u].e[e].i1 = pos(urec[u].e[e].i1);
            urec[u].e[e].i2 = pos(urec[u].e[e].i2);
          }
      }
      for (size_t a = 0; a < rep.size(); ++a)
        if (ptr[a] < ptr[a + 1]) urep[a] = uidx[rep[a]];
      if (fits) {
        if ((rc = dupload(h, &ps.d_fx_urec, urec.data(), urec.size()))) return bail(rc);
        if ((rc = dupload(h, &ps.d_fx_urep, urep.data(), urep.size()))) return bail(rc);
        if (compact && (rc = dupload(h, &ps.d_fx_pl, plrec.data(), plrec.size()))) return bail(rc);
      }
      if (ulist.empty()) ulist.push_back(0);
      if ((rc = dupload(h, &ps.d_fx_rep, rep.data(), rep.size()))) return bail(rc);
      if ((rc = dupload(h, &ps.d_fx_ulist, ulist.data(), ulist.size()))) return bail(rc);
    }
  }
  h->white_fixed = (d->white_fixed != 0) && !any_theta_white;
  if ((rc = dalloc(h, &h->d_jobs_fixed, h->P))) return bail(rc);
  if ((rc = dalloc(h, &h->d_jobs_var, h->P))) return bail(rc);
  h->osmode = d->common && d->common->kind == EWH_COMMON_OPTSTAT;
  if (h->osmode && !h->white_fixed)
    return bail(set_err(EWH_E_UNSUPPORTED, "optimal statistic: white noise must be fixed (TNT cached)"));
  if (h->white_fixed && (rc = setup_fixed(h))) return bail(rc);
  if (d->common && (rc = setup_common(h, d))) return bail(rc);
  if (h->white_fixed && !h->corr && !h->osmode) {
    int nb = h->psr[0].fx_nb;
    for (const auto& ps : h->psr)
      if (ps.fx_nb != nb) nb = 0;
    // (a delay pulsar's residual column differs per sample: the latency
    // kernel reads the cached S -- such a handle runs the batched route at
    // every batch size)
    if (nb >= 1 && nb <= LAT_NB_MAX && h->n_delay_psr == 0) {
      h->lat_nb = nb;
      // (the jobs' mreal is nloc = fx_m here: no common block, not the optimal statistic)
      h->lat_dead = 3;
      for (const auto& ps : h->psr) h->lat_dead = std::min(h->lat_dead, front_dead(ps.fx_ld, ps.fx_m));
    }
  }
  *out = h;
  return 0;
}

}  // namespace ewh_host
