// contract.hip — the fp64 MFMA contraction kernels up to 16 blocks (contract_mfma_kernel, contract2_kernel
// and its compile-time block schedule) and their launchers; bases past 16 blocks: contract_wide.hip.
#include "ewarp_launch.h"

namespace ewh_dev {

constexpr int CT_GROUP = 2;   // contract2: tiles per accumulation group (a power of two)
constexpr int CT_SINGLE = 0, CT_BLOCKED = 1, CT_TWOSUM = 2;   // contract2 accumulation forms

// ----------------------------------------------------------------------------
// fp64 MFMA contraction G = T_aug^T W T_aug - sum_e beta_e s_e s_e^T
// One 256-thread workgroup (4 waves) per sample; the NB(NB+1)/2 upper 16x16
// output blocks are dealt round-robin to the waves; 32-row TOA tiles are
// staged in LDS and shared by the four waves.
// ----------------------------------------------------------------------------
template <int NB>
__global__ __launch_bounds__(256) void contract_mfma_kernel(PsrDev P, const double* __restrict__ w,
                                                            const double* __restrict__ beta,
                                                            const double* __restrict__ s,
                                                            const double* __restrict__ fac,
                                                            double* __restrict__ G) {
  constexpr int LD = 16 * NB;
  constexpr int NBLK = NB * (NB + 1) / 2;
  constexpr int SLOTS = (NBLK + 3) / 4;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* tile = smem;                     // CT_ROWS x LD
  double* wt = smem + CT_ROWS * LD;        // CT_ROWS weights
  const int bl = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, q = lane >> 4, c = lane & 15;

  int bi[SLOTS], bj[SLOTS];
  bool valid[SLOTS];
#pragma unroll
  for (int sl = 0; sl < SLOTS; ++sl) {
    int blk = wave + 4 * sl;
    valid[sl] = blk < NBLK;
    int i = 0;
    while (blk >= NB - i && i < NB - 1) { blk -= NB - i; ++i; }
    bi[sl] = i;
    bj[sl] = i + blk;
  }
  v4d acc[SLOTS];
#pragma unroll
  for (int sl = 0; sl < SLOTS; ++sl) acc[sl] = v4d{0.0, 0.0, 0.0, 0.0};

  // pass 0: TOA rows (weights w), pass 1: epoch rows (weights -beta)
  for (int pass = 0; pass < 2; ++pass) {
    const int nrows = pass == 0 ? P.n_toa : P.n_epoch;
    const double* src = pass == 0 ? P.T : s + (long long)bl * P.n_epoch * LD;
    const double* wsrc = pass == 0 ? w + (long long)bl * P.n_toa : beta + (long long)bl * P.n_epoch;
    const double wsign = pass == 0 ? 1.0 : -1.0;
    for (int t0 = 0; t0 < nrows; t0 += CT_ROWS) {
      const int rows = min(CT_ROWS, nrows - t0);
      if (pass == 0 && P.n_bgroup) {   // theta-dependent chromatic columns: scale per TOA
        for (int idx = threadIdx.x; idx < CT_ROWS * LD; idx += 256) {
          const int r = idx / LD, cc = idx - r * LD;
          double v = idx < rows * LD ? src[(long long)t0 * LD + idx] : 0.0;
          const int g = P.col_bgroup[cc];
          if (g >= 0 && r < rows) v *= fac[((long long)bl * P.n_bgroup + g) * P.n_toa + t0 + r];
          tile[idx] = v;
        }
      } else {
        for (int idx = threadIdx.x; idx < CT_ROWS * LD; idx += 256)
          tile[idx] = idx < rows * LD ? src[(long long)t0 * LD + idx] : 0.0;
      }
      if (threadIdx.x < CT_ROWS) wt[threadIdx.x] = threadIdx.x < rows ? wsign * wsrc[t0 + threadIdx.x] : 0.0;
      __syncthreads();
#pragma unroll
      for (int kk = 0; kk < CT_ROWS / 4; ++kk) {
        const int row = 4 * kk + q;
        const double wr = wt[row];
        const double* trow = tile + row * LD + c;
#pragma unroll
        for (int sl = 0; sl < SLOTS; ++sl) {
          if (valid[sl]) {
            const double a = wr * trow[16 * bi[sl]];
            const double b = trow[16 * bj[sl]];
            acc[sl] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[sl], 0, 0, 0);
          }
        }
      }
      __syncthreads();
    }
  }
  // epilogue: C/D layout lane -> (row q + 4r, col c); mirror to the lower half,
  // unit diagonal on pad columns (m .. LD-2) so they factor as identity.
  // (An exact identity -- T_aug's pad columns are zero, so every other entry
  // of a pad row and column is 0: the register kernels' front-pad order reads
  // these entries, ewarp_dev.h front_src.)
  double* out = G + (long long)bl * LD * LD;
#pragma unroll
  for (int sl = 0; sl < SLOTS; ++sl) {
    if (!valid[sl]) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * bi[sl] + q + 4 * r, col = 16 * bj[sl] + c;
      double v = acc[sl][r];
      if (row == col && row >= P.m && row < LD - 1) v = 1.0;
      out[(long long)row * LD + col] = v;
      out[(long long)col * LD + row] = v;
    }
  }
}

// ----------------------------------------------------------------------------
// fp64 MFMA contraction, pipelined (default for pulsars without theta-dependent
// basis columns).  One 256-thread workgroup (4 waves) per sample:
//   G = T_aug^T W T_aug - sum_e beta_e s_e s_e^T,  s_e = sum_{t in e} w_t T_aug[t].
//  * TOA tiles of CT_ROWS rows are copied global -> LDS by global_load_lds
//    (16 B per lane, 1 KiB per wave-instruction; T_aug is contiguous and padded
//    by CT_ROWS zero rows) into two buffers: tile i+1 streams in while the
//    MFMAs run on tile i.
//  * Wave WAVE owns the upper blocks blk = WAVE + 4 sl (compile-time, so the
//    operand set is known): per k-step it reads T[row][16 j + c] once per block
//    column j it touches and forms w_row * T[row][16 i + c] once per block row i.
//  * ECORR: the epoch sums s_e are accumulated from the same LDS tile (thread
//    = column; epochs are contiguous TOA runs that may straddle tiles) and
//    written to a per-sample scratch; a second pass runs them through the same
//    MFMA loop with weights -beta_e.  No second read of T from HBM.
// ----------------------------------------------------------------------------
typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) void gbl_void_t;

// Contraction block ownership (contract2_body).  The upper blocks are put in
// a tiled order -- tiles of th x tw blocks, row-major over the tiles and
// within one -- and wave v of WS takes a contiguous run of that order (the
// first NBLK % WS waves one block more).  (th, tw) is picked at compile time
// to minimise the per-k-step work of the busiest wave: one LDS read per block
// column it touches and one multiply by the row weight per block row it
// owns.  Round 4 dealt the blocks round-robin (blk = v + WS sl): C4's 13
// blocks over 8 waves then read 13 columns and scaled 10 rows per k-step
// (23 instructions beside 12 MFMAs, and 52 operand registers, which spilled
// the blocked accumulator); tiled runs: 12 (C2's 9 blocks: 15 -> 8).
struct CtOrd {
  int ij[136];                        // i * 64 + j of the pos-th block (NB <= 16)
};
constexpr CtOrd ct_order(int nb, int th, int tw) {
  CtOrd o{};
  int n = 0;
  for (int I = 0; I < nb; I += th)
    for (int J = (I / tw) * tw; J < nb; J += tw)
      for (int i = I; i < I + th && i < nb; ++i)
        for (int j = J; j < J + tw && j < nb; ++j)
          if (j >= i) o.ij[n++] = i * 64 + j;
  return o;
}
// Runs: wave v of ws takes nblk / ws blocks, and the nblk % ws remainder goes
// one each to the LAST waves (LATE, round 5): waves 0 .. ceil(LD / 64) - 1
// also carry the ECORR epoch sums (threads tid < LD) and wave 0 the per-tile
// weight staging, so they take the shorter runs (round 4: the first waves
// took the extra blocks -- C2's 45 blocks put 6 MFMA blocks AND the epoch
// sums on waves 0-2; dev mode 35 keeps that order for the A/B).  Used where
// the accumulator is TwoSum-compensated, round 6; single until then (contract2_late: NB <= 9)
constexpr int ct_run_start(int nblk, int ws, int v, bool late = true) {
  const int b = nblk / ws, x = nblk % ws;
  return late ? v * b + (v > ws - x ? v - (ws - x) : 0) : v * b + (v < x ? v : x);
}
constexpr int ct_run_len(int nblk, int ws, int v, bool late = true) {
  const int b = nblk / ws, x = nblk % ws;
  return b + ((late ? v >= ws - x : v < x) ? 1 : 0);
}
constexpr int ct_cost(int nb, int ws, int th, int tw, bool late = true) {
  const CtOrd o = ct_order(nb, th, tw);
  const int nblk = nb * (nb + 1) / 2;
  int worst = 0;
  for (int v = 0; v < ws; ++v) {
    bool col[16] = {}, row[16] = {};
    const int s0 = ct_run_start(nblk, ws, v, late), n = ct_run_len(nblk, ws, v, late);
    for (int s = s0; s < s0 + n; ++s) {
      row[o.ij[s] >> 6] = col[o.ij[s] >> 6] = col[o.ij[s] & 63] = true;
    }
    int c = 0;
    for (int k = 0; k < nb; ++k) c += (col[k] ? 1 : 0) + (row[k] ? 1 : 0);
    worst = c > worst ? c : worst;
  }
  return worst;
}
constexpr int ct_shape(int nb, int ws, bool late = true) {   // th * 64 + tw
  int best = 1 << 30, shape = 64 + nb;
  for (int th = 1; th <= 6; ++th)
    for (int tw = 1; tw <= nb; ++tw) {
      const int c = ct_cost(nb, ws, th, tw, late);
      if (c < best) {
        best = c;
        shape = th * 64 + tw;
      }
    }
  return shape;
}
// the (i * 64 + j) of slot sl of wave v under shape SH
constexpr int ct_blk(int nb, int ws, int sh, int v, int sl, bool late = true) {
  return ct_order(nb, sh >> 6, sh & 63).ij[ct_run_start(nb * (nb + 1) / 2, ws, v, late) + sl];
}
// does wave v touch block index j as a block row (A operand) / at all?
constexpr bool ct_uses_row(int nb, int ws, int sh, int v, int j, bool late = true) {
  for (int sl = 0; sl < ct_run_len(nb * (nb + 1) / 2, ws, v, late); ++sl)
    if ((ct_blk(nb, ws, sh, v, sl, late) >> 6) == j) return true;
  return false;
}
constexpr bool ct_uses(int nb, int ws, int sh, int v, int j, bool late = true) {
  for (int sl = 0; sl < ct_run_len(nb * (nb + 1) / 2, ws, v, late); ++sl) {
    const int b = ct_blk(nb, ws, sh, v, sl, late);
    if ((b >> 6) == j || (b & 63) == j) return true;
  }
  return false;
}

// WAVE / W: the physical wave and waves per workgroup (tile copies, the
// per-tile weights); VW / WS: the virtual wave that picks the output blocks
// (blocks VW + WS sl) and the virtual waves per sample -- WS = W SPLIT when a
// sample's blocks are split over SPLIT workgroups (contract2_kernel).
// RSEP (round 5; the caller guarantees no ECORR and m <= 16 (NB - 1)): the
// last block column holds only r and pad columns, so the MFMAs form the Gram
// of the first NG = NB - 1 blocks only (C4: 78 instead of 91 blocks, -14 %),
// and d = T^T W r is summed by VALU from the staged tile -- one FMA per
// (row, column) on the last DW waves (column tid - 64 (W - DW)), blocked like
// the Gram; r^T W r comes from wn_weights_kernel (rho).  The epilogue writes
// block column NB - 1 itself: d, zeros, the pads' unit diagonal and rho.
template <int NB, int WAVE, int W, int VW = WAVE, int WS = W, int COMP = CT_BLOCKED, bool LATE = true,
          bool RSEP = false>
__device__ __forceinline__ void contract2_body(const PsrDev& P, const double* __restrict__ wrow,
                                               const double* __restrict__ brow, double* __restrict__ srow,
                                               double* __restrict__ Gout, const double* __restrict__ rho = nullptr) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  constexpr int LD = 16 * NB;
  constexpr int NG = RSEP ? NB - 1 : NB;             // blocks the MFMAs form
  constexpr int NBLK = NG * (NG + 1) / 2;
  constexpr int SH = ct_shape(NG, WS, LATE);          // block ownership: tiled runs (ct_order)
  constexpr int SLOTS = ct_run_len(NBLK, WS, VW, LATE);
  constexpr int DW = RSEP ? (16 * NG + 63) / 64 : 0;  // the d waves (the last DW of W)
  constexpr bool DWAVE = RSEP && WAVE >= W - DW;
  static_assert(!RSEP || (DW <= W && WS == W), "r-separated contraction: one workgroup per sample");
  constexpr int TILE = CT_ROWS * LD;                 // doubles per tile
  constexpr int CHUNKS = TILE * 8 / 1024;            // 1-KiB glds pieces per tile (4 NB), dealt round-robin to the W waves
  static_assert(CHUNKS * 1024 == TILE * 8, "tile must split into pieces of 1 KiB");
  // LDS: [2][TILE] tiles | [2][CT_ROWS] weights | [2][CT_ROWS] epoch-sum
  // weights | [2][CT_ROWS] int flush epoch ids | [2] int flush masks
  const int tid = threadIdx.x, lane = tid & 63, q = lane >> 4, c = lane & 15;
  double* const wbase = smem + 2 * TILE;
  double* const ewbase = wbase + 2 * CT_ROWS;
  int* const ebase = (int*)(ewbase + 2 * CT_ROWS);
  int* const fmbase = ebase + 2 * CT_ROWS;

  // blocked accumulation: each group of CT_GROUP tiles
  // (CT_GROUP x 32 TOA rows) is summed by the MFMAs into a fresh accumulator
  // acc, which is then added into the running sum hi (CT_BLOCKED), or into hi
  // + lo by TwoSum (CT_TWOSUM, dev A/B); G = hi (+ lo) at the end.  A single
  // fp64 accumulator over all rows (CT_SINGLE) lost up to ~30x the strict
  // bound of lnL on ill-conditioned prior draws through the timing-model /
  // red-noise near-degeneracy (tests/golden c4_small sample 0: 4.0 vs
  // enterprise's 2.3 strict); per group the error grows only over CT_GROUP x
  // 32 rows, and the sum of the groups over n / 64 terms (restated on the
  // host, c4_small prior draws in strict units: single -2.1 / -27 / -8.6,
  // blocked -1.1 / -4.3 / -0.2, TwoSum -0.9 / 1.2 / 0.3 on samples 0 / 1 / 5,
  // against enterprise's -2.3 / -195 / -41).
  v4d acc[SLOTS > 0 ? SLOTS : 1], hi[SLOTS > 0 ? SLOTS : 1], lo[SLOTS > 0 ? SLOTS : 1];
#pragma unroll
  for (int sl = 0; sl < SLOTS; ++sl) {
    acc[sl] = v4d{0.0, 0.0, 0.0, 0.0};
    hi[sl] = v4d{0.0, 0.0, 0.0, 0.0};
    lo[sl] = v4d{0.0, 0.0, 0.0, 0.0};
  }
  // RSEP: d of column dc (the d waves), blocked like the Gram
  const int dc = DWAVE ? min(tid - 64 * (W - DW), 16 * NG - 1) : 0;
  double dacc = 0.0, dhi = 0.0, dlo = 0.0;
  auto flush = [&]() {
    if constexpr (COMP == CT_SINGLE) return;
    if constexpr (DWAVE) {
      if constexpr (COMP == CT_TWOSUM) {        // (d compensated like the Gram)
        const double sum = dhi + dacc, bp = sum - dhi;
        dlo += (dhi - (sum - bp)) + (dacc - bp);
        dhi = sum;
      } else {
        dhi += dacc;
      }
      dacc = 0.0;
    }
    static_for<0, SLOTS>([&](auto SL) {
      constexpr int sl = decltype(SL)::value;
      static_for<0, 4>([&](auto R) {
        constexpr int r = decltype(R)::value;
        if constexpr (COMP == CT_TWOSUM) {
          const double a = hi[sl][r], b = acc[sl][r];
          const double sum = a + b, bp = sum - a;
          lo[sl][r] += (a - (sum - bp)) + (b - bp);
          hi[sl][r] = sum;
        } else {
          hi[sl][r] += acc[sl][r];
        }
        acc[sl][r] = 0.0;
      });
    });
  };

  const bool ecorr = !RSEP && P.n_epoch > 0;       // (RSEP: none, by the caller's choice)
  double eacc = 0.0;                                 // running s_e of column `tid`
  // pass 0: TOA rows (weights w); pass 1: epoch rows (weights -beta)
  for (int pass = 0; pass < (ecorr ? 2 : 1); ++pass) {
    const bool epochs = pass == 0 && ecorr;
    const int nrows = pass == 0 ? P.n_toa : P.n_epoch;
    const double* src = pass == 0 ? P.T : srow;
    const double* wsrc = pass == 0 ? wrow : brow;
    const double wsign = pass == 0 ? 1.0 : -1.0;
    const int ntile = (nrows + CT_ROWS - 1) / CT_ROWS;
    auto issue = [&](int it) {
      const char* g = (const char*)(src + (long long)it * TILE) + lane * 16;
      char* l = (char*)(smem + (it & 1) * TILE);
#pragma unroll
      for (int k = WAVE; k < CHUNKS; k += W)
        __builtin_amdgcn_global_load_lds((gbl_void_t*)(g + k * 1024), (lds_void_t*)(l + k * 1024), 16, 0, 0);
    };
    // the tile's weights and epoch flags: wave 0 only (a compile-time branch,
    // no exec mask), loaded unconditionally from a clamped index and BEFORE
    // the tile's global_load_lds, so the wait for them is a counted vmcnt at
    // their use (the LDS store at the end of the iteration), never a
    // vmcnt(0) that would also wait for the next tile's DMA
    double wraw = 0.0, rraw = 0.0;
    int ev = -1;
    auto small = [&](int it) {
      if constexpr (WAVE == 0) {
        const int t = it * CT_ROWS + (lane & (CT_ROWS - 1));
        wraw = wsrc[min(t, nrows - 1)];
        ev = pass == 0 ? P.toa_ep[t] : -1;
        if constexpr (RSEP) rraw = P.T[(long long)min(t, nrows - 1) * LD + LD - 1];
      }
    };
    // staged per tile by wave 0: the Gram weights; the epoch-sum weights
    // (w on rows inside an epoch, 0 elsewhere); the mask of rows that close
    // an epoch and, in mask order, the epochs they close.  The epoch-sum loop
    // then runs on registers and one scalar mask: no per-row LDS round trip.
    auto stage = [&](int buf, int it) {
      if constexpr (WAVE == 0) {
        const int t = it * CT_ROWS + lane;
        const double w = (lane < CT_ROWS && t < nrows) ? wsign * wraw : 0.0;
        const bool fl = lane < CT_ROWS && ev >= 0 && (ev & 1);
        const unsigned long long fmask = __ballot(fl);
        if (lane < CT_ROWS) {
          wbase[buf * CT_ROWS + lane] = w;
          // (RSEP, no ECORR: the epoch-sum weights' slot carries w r, d's row weights)
          ewbase[buf * CT_ROWS + lane] = RSEP ? w * rraw : ev >= 0 ? w : 0.0;
        }
        if (fl) ebase[buf * CT_ROWS + __builtin_amdgcn_mbcnt_lo((unsigned)fmask, 0u)] = ev >> 1;
        if (lane == 0) fmbase[buf] = (int)(unsigned)fmask;
      }
    };
    small(0);
    issue(0);
    stage(0, 0);
    __syncthreads();
    for (int it = 0; it < ntile; ++it) {
      const int cur = it & 1;
      if (it + 1 < ntile) {
        small(it + 1);
        issue(it + 1);
      }
      const double* tile = smem + cur * TILE;
      const double* wt = wbase + cur * CT_ROWS;
#pragma unroll
      for (int kk = 0; kk < CT_ROWS / 4; ++kk) {
        const int row = 4 * kk + q;
        const double wr = wt[row];
        const double* trow = tile + row * LD + c;
        double tv[NG], av[NG];
        static_for<0, NG>([&](auto J) {
          constexpr int j = decltype(J)::value;
          if constexpr (ct_uses(NG, WS, SH, VW, j, LATE)) tv[j] = trow[16 * j];
          if constexpr (ct_uses_row(NG, WS, SH, VW, j, LATE)) av[j] = wr * tv[j];
        });
        static_for<0, SLOTS>([&](auto SL) {
          constexpr int blk = ct_blk(NG, WS, SH, VW, decltype(SL)::value, LATE);
          constexpr int bi = blk >> 6, bj = blk & 63;
          acc[decltype(SL)::value] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[bi], tv[bj], acc[decltype(SL)::value], 0, 0, 0);
        });
      }
      if (epochs && tid < LD) {                      // epoch sums of column tid
        // rows outside an epoch carry weight 0 (T is finite: fma(0, t, s) = s
        // exactly), so the running sum is a plain FMA chain over the tile,
        // its operands read 8 rows per LDS round trip; a row that closes an
        // epoch (bit of the wave-uniform mask) stores the sum and resets it.
        // (Interleaving the chain with the k-steps' MFMAs measured no faster
        // on C2 and 5 % slower on C4: more live registers.)
        const double* tcol = tile + tid;
        const double* ew = ewbase + cur * CT_ROWS;
        const int* fe = ebase + cur * CT_ROWS;
        const unsigned fm = (unsigned)__builtin_amdgcn_readfirstlane(fmbase[cur]);
        int nf = 0;
        // (4 rows per trip beside the blocked accumulator's second register
        // set, which leaves no room for 8)
        constexpr int ER = COMP != CT_SINGLE ? 4 : 8;
#pragma unroll
        for (int r0 = 0; r0 < CT_ROWS; r0 += ER) {
          double tc[ER], wc[ER];
#pragma unroll
          for (int i = 0; i < ER; ++i) {
            tc[i] = tcol[(r0 + i) * LD];
            wc[i] = ew[r0 + i];
          }
#pragma unroll
          for (int i = 0; i < ER; ++i) {
            eacc = fma(wc[i], tc[i], eacc);
            if ((fm >> (r0 + i)) & 1u) {
              const int e = __builtin_amdgcn_readfirstlane(fe[nf]);
              srow[(long long)e * LD + tid] = eacc;
              eacc = 0.0;
              ++nf;
            }
          }
        }
      }
      if constexpr (DWAVE) {                         // d of column dc: this tile's rows
        const double* ewr = ewbase + cur * CT_ROWS;
        constexpr int DR = COMP != CT_SINGLE ? 4 : 8;     // rows per LDS trip (registers, as the epoch sums)
#pragma unroll
        for (int r0 = 0; r0 < CT_ROWS; r0 += DR) {
          double tc[DR], wc[DR];
#pragma unroll
          for (int i = 0; i < DR; ++i) {
            tc[i] = tile[(r0 + i) * LD + dc];
            wc[i] = ewr[r0 + i];
          }
#pragma unroll
          for (int i = 0; i < DR; ++i) dacc = fma(wc[i], tc[i], dacc);
        }
      }
      if ((it & (CT_GROUP - 1)) == CT_GROUP - 1 || it + 1 == ntile) flush();
      if (it + 1 < ntile) stage(cur ^ 1, it + 1);
      __syncthreads();                               // drains the glds of tile it+1 (vmcnt(0))
    }
    if (pass == 0 && ecorr && tid < LD) {
      // pad rows [n_epoch, whole tiles) of the epoch pass: zero, so a value a
      // previous pulsar / sample left in the shared scratch never meets the
      // zero weight of the pad rows (0 * inf = NaN)
      const int epad = ((P.n_epoch + CT_ROWS - 1) / CT_ROWS) * CT_ROWS;
      for (int e = P.n_epoch; e < epad; ++e) srow[(long long)e * LD + tid] = 0.0;
    }
    if (pass == 0 && ecorr) __threadfence_block();   // s_e rows visible to the epoch pass
    __syncthreads();
  }
  // epilogue: C/D layout lane -> (row q + 4r, col c); mirror to the lower half,
  // unit diagonal on pad columns (m .. LD-2) so they factor as identity.
  // (An exact identity -- T_aug's pad columns are zero, so every other entry
  // of a pad row and column is 0: the register kernels' front-pad order reads
  // these entries, ewarp_dev.h front_src.)
  if constexpr (DWAVE) {
    // block column NB - 1: d in column LD - 1, zeros in the pad columns
    // [16 NG, LD - 1) (their rows too); the d wave of column 0 also writes
    // the last diagonal block: unit diagonal on the pads, rho at the corner
    const int a = tid - 64 * (W - DW);
    if (a < 16 * NG) {
      const double d = COMP == CT_SINGLE ? dacc : COMP == CT_TWOSUM ? dhi + dlo : dhi;
      Gout[(long long)a * LD + LD - 1] = d;
      Gout[(long long)(LD - 1) * LD + a] = d;
#pragma unroll
      for (int pc = 16 * NG; pc < LD - 1; ++pc) {
        Gout[(long long)a * LD + pc] = 0.0;
        Gout[(long long)pc * LD + a] = 0.0;
      }
    }
    if (WAVE == W - DW) {
#pragma unroll
      for (int e = lane; e < 256; e += 64) {
        const int row = 16 * NG + (e >> 4), col = 16 * NG + (e & 15);
        Gout[(long long)row * LD + col] = row == LD - 1 && col == LD - 1 ? rho[blockIdx.x] : row == col ? 1.0 : 0.0;
      }
    }
  }
  static_for<0, SLOTS>([&](auto SL) {
    constexpr int blk = ct_blk(NG, WS, SH, VW, decltype(SL)::value, LATE);
    constexpr int bi = blk >> 6, bj = blk & 63;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * bi + q + 4 * r, col = 16 * bj + c;
      constexpr int sl = decltype(SL)::value;
      double v = COMP == CT_TWOSUM ? hi[sl][r] + lo[sl][r] : COMP == CT_BLOCKED ? hi[sl][r] : acc[sl][r];
      if (row == col && row >= P.m && row < LD - 1) v = 1.0;
      Gout[(long long)row * LD + col] = v;
      Gout[(long long)col * LD + row] = v;
    }
  });
}

// W = 4 or 8 waves per workgroup (8: half the accumulators per wave, so the
// narrow NB = 9 kernel fits 4 waves per SIMD and the wide NB = 13 one 2).
template <int NB, int W, int COMP = CT_BLOCKED, bool LATE = true, bool RSEP = false>
__global__ __launch_bounds__(64 * W) void contract2_kernel(PsrDev P, const double* __restrict__ w,
                                                           const double* __restrict__ beta, double* __restrict__ s,
                                                           long long s_stride, double* __restrict__ G,
                                                           const double* __restrict__ rho) {
  const int bl = blockIdx.x;
  const double* wrow = w + (long long)bl * P.n_toa;
  const double* brow = beta + (long long)bl * P.n_epoch;
  double* srow = s + (long long)bl * s_stride;
  double* Gout = G + (long long)bl * 16 * NB * 16 * NB;
  const int wv = threadIdx.x >> 6;
  static_for<0, W>([&](auto WV) {
    constexpr int wave = decltype(WV)::value;
    if (wv == wave) contract2_body<NB, wave, W, wave, W, COMP, LATE, RSEP>(P, wrow, brow, srow, Gout, rho);
  });
}
// the accumulation per width: blocked from 10 blocks on (C4's 13: the same
// registers as the single accumulator plus one set -- 2 waves per SIMD as
// before); below, the single accumulator meets the per-sample accuracy bound
// (c2_small, the C2 bench draws) and the extra set would halve C2's occupancy
// (4 -> 2 waves per SIMD).  (Round 4 first used TwoSum at 10+ blocks: three
// accumulator sets, so 11+ blocks had to split a sample over two workgroups;
// C4 5.44 k evals/s, vs 6.51 k with one accumulator.)  Dev kernel mode 30:
// TwoSum at every width up to 10 blocks (A/B).
// Round 6: TwoSum groups up to 10 blocks (C2's 9), blocked from 11 on.  The
// single accumulator C2 had kept since round 4 left 36 of its 4096 bench prior
// draws less accurate than enterprise's own fp64 order (at most 15x) against
// the double-double twin; TwoSum: none (worst 0.59), for 17.6 -> 20.8 ms per
// batch (scripts/c2_accum_ab.py, profiles/r06i).  Past 10 blocks the third
// accumulator set does not fit one workgroup per sample (round 4: C4 split
// over two workgroups, -16 %)
constexpr int contract2_comp(int nb) { return nb >= 11 ? CT_BLOCKED : CT_TWOSUM; }

namespace {

template <int NB>
void launch_contract(const PsrDev& P, const double* w, const double* beta, const double* s, const double* fac,
                     double* G, int nb_samples, hipStream_t st) {
  const size_t lds = (size_t)(CT_ROWS * 16 * NB + CT_ROWS) * sizeof(double);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(contract_mfma_kernel<NB>), dim3(nb_samples), dim3(256), lds, st, P, w, beta, s,
                     fac, G);
}

int dispatch_contract(int nb, const PsrDev& P, const double* w, const double* beta, const double* s,
                      const double* fac, double* G, int nb_samples, hipStream_t st, double* Glo) {
  if (nb > 16) return launch_contract_wide(nb, P, w, beta, s, fac, G, nb_samples, st, Glo);   // (contract_wide.hip)
  switch (nb) {
    case 1: launch_contract<1>(P, w, beta, s, fac, G, nb_samples, st); break;
    case 2: launch_contract<2>(P, w, beta, s, fac, G, nb_samples, st); break;
    case 3: launch_contract<3>(P, w, beta, s, fac, G, nb_samples, st); break;
    case 4: launch_contract<4>(P, w, beta, s, fac, G, nb_samples, st); break;
    case 5: launch_contract<5>(P, w, beta, s, fac, G, nb_samples, st); break;
    case 6: launch_contract<6>(P, w, beta, s, fac, G, nb_samples, st); break;
    case 7: launch_contract<7>(P, w, beta, s, fac, G, nb_samples, st); break;
    case 8: launch_contract<8>(P, w, beta, s, fac, G, nb_samples, st); break;
    case 9: launch_contract<9>(P, w, beta, s, fac, G, nb_samples, st); break;
    case 10: launch_contract<10>(P, w, beta, s, fac, G, nb_samples, st); break;
    case 11: launch_contract<11>(P, w, beta, s, fac, G, nb_samples, st); break;
    case 12: launch_contract<12>(P, w, beta, s, fac, G, nb_samples, st); break;
    case 13: launch_contract<13>(P, w, beta, s, fac, G, nb_samples, st); break;
    case 14: launch_contract<14>(P, w, beta, s, fac, G, nb_samples, st); break;
    case 15: launch_contract<15>(P, w, beta, s, fac, G, nb_samples, st); break;
    case 16: launch_contract<16>(P, w, beta, s, fac, G, nb_samples, st); break;
    default: return set_err(EWH_E_UNSUPPORTED, "basis too wide for the contraction kernel (> 255 columns)");
  }
  return 0;
}

constexpr size_t contract2_lds(int nb) { return (size_t)(2 * CT_ROWS * 16 * nb + 6 * CT_ROWS) * sizeof(double); }

// waves per sample: 4, or 8 where measured faster (fewer accumulators per
// wave: more waves per SIMD to hide the k-steps' LDS latency)
constexpr int contract2_default_waves(int nb) { return nb >= 9 || contract2_comp(nb) == CT_TWOSUM ? 8 : 4; }
// the run remainder on the last waves (ct_run_start) where the accumulator is
// single (NB <= 9: C2's ECORR model); the blocked NB >= 10 kernel keeps the
// round-4 order -- with the remainder moved its spill grew 12 -> 28 B/lane
constexpr bool contract2_late(int nb) { return nb <= 9; }

template <int NB>
int launch_contract2(int waves, const PsrDev& P, const double* w, const double* beta, double* s, long long s_stride,
                     double* G, int nb_samples, hipStream_t st, const double* rho) {
  // (the dynamic-LDS attribute is set per device by set_contract_attributes)
  constexpr int CP = contract2_comp(NB);
#ifdef EWH_DEV
  if constexpr (NB <= 10) {
    if (waves == 30) {   // (dev A/B: TwoSum accumulation)
      hipLaunchKernelGGL(HIP_KERNEL_NAME(contract2_kernel<NB, 8, CT_TWOSUM>), dim3(nb_samples), dim3(512),
                         contract2_lds(NB), st, P, w, beta, s, s_stride, G, nullptr);
      return 0;
    }
    if (waves == 38 || waves == 39) {   // (dev A/B: blocked accumulation, 4 / 8 waves)
      if (waves == 39)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(contract2_kernel<NB, 8, CT_BLOCKED, contract2_late(NB)>), dim3(nb_samples),
                           dim3(512), contract2_lds(NB), st, P, w, beta, s, s_stride, G, nullptr);
      else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(contract2_kernel<NB, 4, CT_BLOCKED, contract2_late(NB)>), dim3(nb_samples),
                           dim3(256), contract2_lds(NB), st, P, w, beta, s, s_stride, G, nullptr);
      return 0;
    }
  }
  if (waves == 35) {     // (dev A/B: the extra blocks on the first waves, round 4-5a)
    if (contract2_default_waves(NB) == 8)
      hipLaunchKernelGGL(HIP_KERNEL_NAME(contract2_kernel<NB, 8, CP, false>), dim3(nb_samples), dim3(512),
                         contract2_lds(NB), st, P, w, beta, s, s_stride, G, nullptr);
    else
      hipLaunchKernelGGL(HIP_KERNEL_NAME(contract2_kernel<NB, 4, CP, false>), dim3(nb_samples), dim3(256),
                         contract2_lds(NB), st, P, w, beta, s, s_stride, G, nullptr);
    return 0;
  }
#endif
  if (waves == 0 || waves == 30) waves = contract2_default_waves(NB);
  constexpr bool LT = contract2_late(NB);
  if constexpr (NB >= 2) {
    if (rho) {   // the r-separated contraction (run_white decides; no ECORR, m <= 16 (NB - 1))
      if (waves == 8)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(contract2_kernel<NB, 8, CP, LT, true>), dim3(nb_samples), dim3(512),
                           contract2_lds(NB), st, P, w, beta, s, s_stride, G, rho);
      else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(contract2_kernel<NB, 4, CP, LT, true>), dim3(nb_samples), dim3(256),
                           contract2_lds(NB), st, P, w, beta, s, s_stride, G, rho);
      return 0;
    }
  }
  if (waves == 8)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(contract2_kernel<NB, 8, CP, LT>), dim3(nb_samples), dim3(512),
                       contract2_lds(NB), st, P, w, beta, s, s_stride, G, nullptr);
  else
    hipLaunchKernelGGL(HIP_KERNEL_NAME(contract2_kernel<NB, 4, CP, LT>), dim3(nb_samples), dim3(256),
                       contract2_lds(NB), st, P, w, beta, s, s_stride, G, nullptr);
  return 0;
}

int dispatch_contract2(int nb, int waves, const PsrDev& P, const double* w, const double* beta, double* s,
                       long long s_stride, double* G, int nb_samples, hipStream_t st, const double* rho) {
  int rc = 1;
  static_for<1, CONTRACT2_NB_MAX + 1>([&](auto N) {
    if (nb == decltype(N)::value)
      rc = launch_contract2<decltype(N)::value>(waves, P, w, beta, s, s_stride, G, nb_samples, st, rho);
  });
  if (rc == 1) return set_err(EWH_E_UNSUPPORTED, "basis too wide for the pipelined contraction (> 207 columns)");
  return rc;
}

template <int NB>
int set_attr2() {
  constexpr int CP = contract2_comp(NB);
  constexpr bool LT = contract2_late(NB);
  EWH_HIP(hipFuncSetAttribute((const void*)contract2_kernel<NB, 4, CP, LT>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)contract2_lds(NB)));
  EWH_HIP(hipFuncSetAttribute((const void*)contract2_kernel<NB, 8, CP, LT>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)contract2_lds(NB)));
  if constexpr (NB >= 2) {
    EWH_HIP(hipFuncSetAttribute((const void*)contract2_kernel<NB, 4, CP, LT, true>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)contract2_lds(NB)));
    EWH_HIP(hipFuncSetAttribute((const void*)contract2_kernel<NB, 8, CP, LT, true>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)contract2_lds(NB)));
  }
#ifdef EWH_DEV
  if constexpr (NB <= 10) {
    EWH_HIP(hipFuncSetAttribute((const void*)contract2_kernel<NB, 8, CT_TWOSUM>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)contract2_lds(NB)));
    EWH_HIP(hipFuncSetAttribute((const void*)contract2_kernel<NB, 4, CT_BLOCKED, contract2_late(NB)>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)contract2_lds(NB)));
    EWH_HIP(hipFuncSetAttribute((const void*)contract2_kernel<NB, 8, CT_BLOCKED, contract2_late(NB)>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)contract2_lds(NB)));
  }
  EWH_HIP(hipFuncSetAttribute((const void*)contract2_kernel<NB, 4, CP, false>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)contract2_lds(NB)));
  EWH_HIP(hipFuncSetAttribute((const void*)contract2_kernel<NB, 8, CP, false>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)contract2_lds(NB)));
#endif
  return 0;
}

template <int NB>
int set_attr1() {
  const size_t lds = (size_t)(CT_ROWS * 16 * NB + CT_ROWS) * sizeof(double);
  EWH_HIP(hipFuncSetAttribute((const void*)contract_mfma_kernel<NB>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds));
  return 0;
}

}  // namespace

// dynamic-LDS limits of every contraction instantiation on the current device
int set_contract_attributes() {
  int rc = 0;
  static_for<1, CONTRACT2_NB_MAX + 1>([&](auto N) {
    if (!rc) rc = set_attr2<decltype(N)::value>();
  });
  static_for<1, 17>([&](auto N) {
    if (!rc) rc = set_attr1<decltype(N)::value>();
  });
  return rc;
}

int launch_contract_nb(int nb, const PsrDev& P, const double* w, const double* beta, const double* s,
                       const double* fac, double* G, int nb_samples, hipStream_t st, double* Glo) {
  return dispatch_contract(nb, P, w, beta, s, fac, G, nb_samples, st, Glo);
}

int launch_contract2_nb(int nb, int waves, const PsrDev& P, const double* w, const double* beta, double* s,
                        long long s_stride, double* G, int nb_samples, hipStream_t st, const double* rho) {
  return dispatch_contract2(nb, waves, P, w, beta, s, s_stride, G, nb_samples, st, rho);
}

}  // namespace ewh_dev
