// RELL bootstrap support of placements (resampling of estimated log-likelihoods): per query the site log-likelihoods
// of its competing placements are resampled with replacement `replicates` times; the support of a placement is the
// fraction of replicates it wins.  The per-site values come from k_score_at<S, true> (score_at.hip).
//
// The resampling is specified exactly (include/epa_dev.h, epa_dev_rell_support), so that a result can be reproduced
// anywhere:
//   generator  Philox4x32-10 with the Random123 constants (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl increments
//              0x9E3779B9 / 0xBB67AE85), key = (seed low word, seed high word)
//   draws      replicate r of a query with stream id t and span n_q makes n_q draws; draw d uses output word d % 4 of
//              counter (d / 4, r, t low word, t high word); the drawn site is j = (word * n_q) >> 32
//   score      starts at 0.0 and adds, for d = 0 .. n_q - 1 in this order, the entry's site value at the drawn j:
//              plain fp64 adds, no centring, no reassociation
//   winner     the largest score; ties go to the smaller branch id, then to the smaller entry index
//
// Host side (rell_run): the entries are grouped by query with a stable radix sort of their indices, so a group
// keeps the caller's entry order; the groups are worked off in batches of whole queries whose site rows fit a fixed
// scratch budget (one query alone may exceed it: its rows are then allocated as they are).
//
// k_rell: one 256-thread workgroup per query, thread = replicate (in rounds of 256).  The entries are taken in tiles
// of TE = 4: the tile's [site][4] matrix is staged in LDS (32 bytes per site: a draw reads its four values with two
// ds_read_b128), every thread regenerates the same draws for every tile -- the point of a counter-based generator --
// and carries its running best (score, branch, position) across the tiles.  A window longer than LDS_SITES does not
// fit the LDS tile; its draws gather from the rows in HBM / L2 instead.  Wins are counted with LDS atomics for up to
// WINS_LDS entries per query, beyond that with global atomics.
//
// k_rell_tests (epa_dev_rell_tests): the same replicates also give the expected likelihood weight and the SH p-value of
// every entry.  Same shape as k_rell; the new part is that a replicate needs all of its query's scores twice.  A query
// of up to RES_TILES tiles (eight entries) keeps its scores in registers; a longer one sweeps its tiles twice and
// regenerates the draws: sweep 1 carries the running winner, the running maximum m with the sum Z = sum exp(s - m) rescaled whenever m
// moves, and max c; sweep 2 forms the weights exp(s - m) / Z and the comparisons t >= T.  The weights of the 256
// replicate lanes are added by epa_wave::wave_sum and the four wave partials in wave order, the rounds in round order,
// all by one thread per entry: a fixed order, no floating-point atomics.  The observed sums L and the thresholds T come
// from two small kernels in front (k_rell_observed, k_rell_threshold), once per entry.
//
// k_rell_ms / k_rell_au_fit (epa_dev_rell_au): the AU test's p-value from multiscale replicates.  k_rell_ms is k_rell with
// a loop over the scales around the rounds: scale s draws n'_s = round(n_q * scale_s) times from the same n_q sites, with
// (s + 1) << 20 above the replicate in the counter's second word, so every scale is a stream of its own.  A query of one
// tile is staged once for all scales and rounds.  The counters are [scale][entry]: in LDS while n_scales * E fit
// MS_WINS_LDS (the 4 KiB k_rell spends on its counters: the same three workgroups per CU), else global integer atomics.
// k_rell_au_fit: one thread per entry fits the signed distance d and the curvature c to its ten proportions and writes
// p_au = normcdf(c - d), or the plain proportion where fewer than three scales are usable.
//
// k_rell_pair_scale / k_rell_kh_thresholds / k_rell_kh (epa_dev_rell_kh): the KH, the weighted KH and the weighted SH
// test from the replicates of k_rell.  The first statistics here that need every PAIR of a query's entries: the scale
// w_kk' = 1 / sd(s_k' - s_k) comes from the two site rows (one thread per pair, sequential sums), the opponents and
// thresholds from w and the observed sums, once per entry; k_rell_kh then holds a replicate's centred scores of ALL
// entries -- in registers up to eight entries, beyond that in a scratch column of its own -- and compares every entry
// with every other.  Integer atomics only.  A batch is worked off in ranges of queries whose [K][K] matrices fit 64 MiB.
#include "epa_dev_internal.hpp"
#include "wave_util.hpp"


#include <algorithm>
#include <vector>

namespace {

constexpr int RELL_THREADS = 256;
constexpr int TE = 4;                    // entries per tile
constexpr uint32_t LDS_SITES = 1536;     // 1536 sites x 4 entries x 8 B = 48 KiB
constexpr uint32_t WINS_LDS = 1024;      // entries per query whose wins are counted in LDS
constexpr uint32_t MS_SCALES = 16;       // k_rell_ms: the most scales of a call
constexpr uint32_t MS_WINS_LDS = 1024;   // k_rell_ms: scales x entries per query counted in LDS: 48 + 4 KiB as k_rell, three workgroups per CU
constexpr int RES_TILES = 2;             // k_rell_tests: tiles of a query whose scores stay in registers between the sweeps
constexpr uint32_t ACC_LDS = 256;       // k_rell_tests: entries per query whose three accumulators live in LDS
constexpr int KH_RES = 2 * TE;           // k_rell_kh: entries of a query whose centred scores stay in registers, w in LDS
constexpr uint32_t KH_MAX_ENTRIES = 1024;   // epa_dev_rell_kh: entries per query; the [K][K] scales of one query: 8 MiB
constexpr uint32_t KH_CNT_LDS = 256;     // k_rell_kh: entries per query whose three counters live in LDS
constexpr uint32_t KH_NONE = 0xffffffffu;   // no opponent: every pair of the entry is skipped
constexpr size_t KH_W_BUDGET = (size_t)64 << 20;       // bytes of scale matrices per launch (a range of whole queries)
constexpr size_t KH_SPILL_BUDGET = (size_t)256 << 20;  // bytes of spilled scores of all workgroups of a launch
constexpr size_t ROWS_BUDGET = (size_t)128 << 20;   // bytes of site rows per batch

struct RellGroup {
  uint32_t q, start, count;   // query, first sorted position, entries
};

struct RellArgs {
  const RellGroup* groups;
  uint32_t n_groups;
  const uint32_t* order;      // sorted position -> entry
  const epa_pair* pairs;
  const uint32_t* span;
  const uint64_t* stream_id;  // null: the query's index
  const double* rows;         // [batch positions][pitch], row = position - pos0
  uint32_t pos0, pitch;
  uint32_t R, k0, k1;
  uint32_t* wins;             // [n] by sorted position
};

struct RellTestsArgs {
  RellArgs r;
  const double* L;            // [n] by sorted position: observed lnL (k_rell_observed)
  const double* T;            // [n]: the query's largest L minus the entry's (k_rell_threshold)
  double* elw;                // [n]: sum of the weights over the replicates
  uint32_t* sh;               // [n]: replicates with t >= T
};

struct RellMsScales {
  uint32_t n;                 // scales in use
  uint32_t pm[MS_SCALES];     // replicate length per mille of the span
};

struct RellMsArgs {
  RellArgs r;                 // r.wins: [scale][n] by sorted position
  RellMsScales sc;
  uint32_t n;                 // entries of the call: the pitch of the counters
};

struct RellKhArgs {
  RellArgs r;                 // r.groups: the queries of this launch (a range of a batch); r.wins is not used
  uint32_t lo, hi;            // the launch serves the queries of lo .. hi entries
  const double* L;            // [n] by sorted position: observed lnL (k_rell_observed)
  double* W;                  // the scale matrices of the launch's queries, [K][K] each (k_rell_pair_scale); < 0: skipped
  const uint64_t* woff;       // [queries of the launch]: where the query's matrix begins in W
  uint32_t* best;             // [queries of the launch]: b, the entry with the largest L (k_rell_kh_thresholds)
  uint32_t* opp;              // [n]: k*, the entry's opponent in the weighted KH test, or KH_NONE
  double *D, *Dw, *Tw;        // [n]: L_b - L_k; L_k* - L_k; T_k
  uint32_t* cnt;              // [3][n]: replicates counted by KH, weighted KH, weighted SH
  uint32_t n;                 // entries of the call: the pitch of the counters
  double* spill;              // [workgroups][spill_pitch]: the centred scores of a query beyond KH_RES, [entry][thread]
  uint32_t spill_pitch;
};

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t out[4]) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__global__ void __launch_bounds__(256) k_rell_keys(const epa_pair* __restrict__ pairs, uint32_t n,
                                                   uint32_t* __restrict__ keys, uint32_t* __restrict__ idx) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  keys[i] = pairs[i].seq_id;
  idx[i] = i;
}

// first and one-past-last sorted position of every query that has entries (bounds [2][Q], zeroed before)
__global__ void __launch_bounds__(256) k_rell_bounds(const uint32_t* __restrict__ sorted, uint32_t n, uint32_t Q,
                                                     uint32_t* __restrict__ bounds) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t q = sorted[i];
  if (q >= Q) return;
  if (i == 0 || sorted[i - 1] != q) bounds[q] = i;
  if (i + 1 == n || sorted[i + 1] != q) bounds[Q + q] = i + 1;
}

__global__ void __launch_bounds__(256) k_rell_support(const uint32_t* __restrict__ wins, const uint32_t* __restrict__ order,
                                                      uint32_t n, double R, double* __restrict__ support) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) support[order[i]] = (double)wins[i] / R;
}

// ---- what k_rell and k_rell_tests share: one tile of entries staged, scored in a replicate, and entered for the winner

// the tile's [site][TE] matrix (entries from te on: 0.0); the caller puts a barrier in front and behind
__device__ __forceinline__ void rell_stage_tile(double* mat, const double* __restrict__ rows, uint32_t pitch, uint32_t e0,
                                                uint32_t te, uint32_t nq, uint32_t tid) {
  for (uint32_t i = tid; i < nq * TE; i += RELL_THREADS) {
    const uint32_t k = i / nq, j = i - k * nq;   // consecutive threads read consecutive sites of one row
    mat[j * TE + k] = k < te ? rows[(size_t)(e0 + k) * pitch + j] : 0.0;
  }
}

// sc[k]: the score of entry e0 + k over nd draws from the nq sites, counter word 1 = c1 (the replicate r; k_rell_ms puts
// the scale above it), stream (tlo, thi), key (k0, k1).  k_rell and k_rell_tests draw nd = nq times
__device__ __forceinline__ void rell_tile_scores(const double* mat, const double* __restrict__ rows, uint32_t pitch,
                                                 uint32_t e0, uint32_t te, uint32_t nq, uint32_t nd, bool in_lds, uint32_t c1,
                                                 uint32_t tlo, uint32_t thi, uint32_t k0, uint32_t k1, double sc[TE]) {
#pragma unroll
  for (int k = 0; k < TE; ++k) sc[k] = 0.0;
  for (uint32_t d = 0; d < nd; d += 4) {
    uint32_t w[4];
    philox4x32_10(d >> 2, c1, tlo, thi, k0, k1, w);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (d + u < nd) {
        const uint32_t j = __umulhi(w[u], nq);
        if (in_lds) {
#pragma unroll
          for (int k = 0; k < TE; ++k) sc[k] += mat[j * TE + k];   // padded entries add 0.0 to unused scores
        } else {
#pragma unroll
          for (int k = 0; k < TE; ++k)
            if ((uint32_t)k < te) sc[k] += rows[(size_t)(e0 + k) * pitch + j];
        }
      }
    }
  }
}

// the running winner: the largest score, ties to the smaller branch id, then to the smaller entry index
__device__ __forceinline__ void rell_tile_winner(const double sc[TE], bool first_tile, uint32_t e0, uint32_t te,
                                                 const epa_pair* __restrict__ pairs, const uint32_t* __restrict__ ord,
                                                 double& best_sc, uint32_t& best_br, uint32_t& best_k) {
#pragma unroll
  for (int k = 0; k < TE; ++k) {
    if ((uint32_t)k < te) {
      const uint32_t br = pairs[ord[e0 + k]].branch_id;
      // positions of a group ascend with the entry index (stable sort): an equal branch keeps the earlier entry
      if ((first_tile && k == 0) || sc[k] > best_sc || (sc[k] == best_sc && br < best_br)) {
        best_sc = sc[k];
        best_br = br;
        best_k = e0 + k;
      }
    }
  }
}

__global__ void __launch_bounds__(RELL_THREADS) k_rell(const RellArgs a) {
  __shared__ __attribute__((aligned(16))) double mat[LDS_SITES * TE];   // [site][TE]
  __shared__ uint32_t wins_l[WINS_LDS];
  const uint32_t tid = threadIdx.x;
  for (uint32_t g = blockIdx.x; g < a.n_groups; g += gridDim.x) {
    const RellGroup grp = a.groups[g];
    const uint32_t E = grp.count, nq = a.span[grp.q];
    const uint64_t t = a.stream_id ? a.stream_id[grp.q] : (uint64_t)grp.q;
    const uint32_t tlo = (uint32_t)t, thi = (uint32_t)(t >> 32);
    const double* __restrict__ rows = a.rows + (size_t)(grp.start - a.pos0) * a.pitch;
    const uint32_t* __restrict__ ord = a.order + grp.start;
    const bool in_lds = nq <= LDS_SITES, wins_lds = E <= WINS_LDS;   // workgroup-uniform
    const uint32_t ntiles = (E + TE - 1) / TE;
    __syncthreads();   // the previous query's tile and counters are no longer read
    if (wins_lds)
      for (uint32_t i = tid; i < E; i += RELL_THREADS) wins_l[i] = 0;
    __syncthreads();
    for (uint32_t rbase = 0; rbase < a.R; rbase += RELL_THREADS) {
      const uint32_t r = rbase + tid;
      const bool active = r < a.R;
      double best_sc = 0.0;
      uint32_t best_br = 0, best_k = 0;
      for (uint32_t tile = 0; tile < ntiles; ++tile) {
        const uint32_t e0 = tile * TE, te = min((uint32_t)TE, E - e0);
        // a query of one tile keeps it for all rounds of replicates; more tiles are staged again every round
        if (in_lds && (ntiles > 1 || rbase == 0)) {
          __syncthreads();
          rell_stage_tile(mat, rows, a.pitch, e0, te, nq, tid);
          __syncthreads();
        }
        if (!active) continue;
        double sc[TE];
        rell_tile_scores(mat, rows, a.pitch, e0, te, nq, nq, in_lds, r, tlo, thi, a.k0, a.k1, sc);
        rell_tile_winner(sc, tile == 0, e0, te, a.pairs, ord, best_sc, best_br, best_k);
      }
      if (active) {
        if (wins_lds) atomicAdd(&wins_l[best_k], 1u);
        else atomicAdd(&a.wins[grp.start + best_k], 1u);
      }
    }
    __syncthreads();
    if (wins_lds)
      for (uint32_t i = tid; i < E; i += RELL_THREADS) a.wins[grp.start + i] = wins_l[i];
  }
}

// draws per replicate at scale pm (per mille) of a query of nq sites: round(nq * pm / 1000), at least 1; 0 for no sites
__device__ __forceinline__ uint32_t rell_ms_draws(uint32_t nq, uint32_t pm) {
  if (nq == 0) return 0;
  const uint64_t nd = ((uint64_t)nq * pm + 500u) / 1000u;
  return nd ? (uint32_t)nd : 1u;
}

// The multiscale replicates of epa_dev_rell_au: k_rell once per scale s with nd = rell_ms_draws(nq, pm[s]) draws from the
// same nq sites and (s + 1) << 20 above the replicate in the counter's second word.  A query of one tile is staged once for
// all scales and rounds; the counters are [scale][entry], in LDS while a query's n_scales * E fit MS_WINS_LDS
__global__ void __launch_bounds__(RELL_THREADS) k_rell_ms(const RellMsArgs ma) {
  __shared__ __attribute__((aligned(16))) double mat[LDS_SITES * TE];   // [site][TE]
  __shared__ uint32_t wins_l[MS_WINS_LDS];                              // [scale][E]
  const RellArgs& a = ma.r;
  const uint32_t tid = threadIdx.x, S = ma.sc.n;
  for (uint32_t g = blockIdx.x; g < a.n_groups; g += gridDim.x) {
    const RellGroup grp = a.groups[g];
    const uint32_t E = grp.count, nq = a.span[grp.q];
    const uint64_t t = a.stream_id ? a.stream_id[grp.q] : (uint64_t)grp.q;
    const uint32_t tlo = (uint32_t)t, thi = (uint32_t)(t >> 32);
    const double* __restrict__ rows = a.rows + (size_t)(grp.start - a.pos0) * a.pitch;
    const uint32_t* __restrict__ ord = a.order + grp.start;
    const bool in_lds = nq <= LDS_SITES, wins_lds = (uint64_t)S * E <= MS_WINS_LDS;   // workgroup-uniform
    const uint32_t ntiles = (E + TE - 1) / TE;
    __syncthreads();   // the previous query's tile and counters are no longer read
    if (wins_lds)
      for (uint32_t i = tid; i < S * E; i += RELL_THREADS) wins_l[i] = 0;
    if (in_lds && ntiles == 1) rell_stage_tile(mat, rows, a.pitch, 0, E, nq, tid);
    __syncthreads();
    for (uint32_t s = 0; s < S; ++s) {
      const uint32_t nd = rell_ms_draws(nq, ma.sc.pm[s]), c1 = (s + 1) << 20;
      for (uint32_t rbase = 0; rbase < a.R; rbase += RELL_THREADS) {
        const uint32_t r = rbase + tid;
        const bool active = r < a.R;
        double best_sc = 0.0;
        uint32_t best_br = 0, best_k = 0;
        for (uint32_t tile = 0; tile < ntiles; ++tile) {
          const uint32_t e0 = tile * TE, te = min((uint32_t)TE, E - e0);
          if (in_lds && ntiles > 1) {   // as k_rell: more tiles are staged again for every round of replicates
            __syncthreads();
            rell_stage_tile(mat, rows, a.pitch, e0, te, nq, tid);
            __syncthreads();
          }
          if (!active) continue;
          double sc[TE];
          rell_tile_scores(mat, rows, a.pitch, e0, te, nq, nd, in_lds, c1 | r, tlo, thi, a.k0, a.k1, sc);
          rell_tile_winner(sc, tile == 0, e0, te, a.pairs, ord, best_sc, best_br, best_k);
        }
        if (active) {
          if (wins_lds) atomicAdd(&wins_l[s * E + best_k], 1u);
          else atomicAdd(&a.wins[(size_t)s * ma.n + grp.start + best_k], 1u);
        }
      }
    }
    __syncthreads();
    if (wins_lds)
      for (uint32_t i = tid; i < S * E; i += RELL_THREADS) {
        const uint32_t s = i / E;
        a.wins[(size_t)s * ma.n + grp.start + (i - s * E)] = wins_l[i];
      }
  }
}

// The AU p-value of every entry from its win counts (include/epa_dev.h, epa_dev_rell_au): one thread per sorted position.
// Weighted least squares of z_s = -normcdfinv(p_s) on (sqrt(r_s), 1 / sqrt(r_s)) over the usable scales, the five sums in
// scale order; fewer than three usable scales, or one draw count among them: the count of the scale nearest 1000
__global__ void __launch_bounds__(256) k_rell_au_fit(const uint32_t* __restrict__ wins, const uint32_t* __restrict__ order,
                                                     const epa_pair* __restrict__ pairs, const uint32_t* __restrict__ span,
                                                     const RellMsScales sc, uint32_t n, uint32_t R, double* __restrict__ p_au,
                                                     uint32_t* __restrict__ counts, double* __restrict__ fit) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t e = order[i], nq = span[pairs[e].seq_id], S = sc.n;
  const double Rd = (double)R;
  uint32_t usable = 0, nd0 = 0, s_star = 0, off_star = 0xffffffffu;
  bool distinct = false;
  for (uint32_t s = 0; s < S; ++s) {
    const uint32_t c = wins[(size_t)s * n + i], pm = sc.pm[s], off = pm > 1000u ? pm - 1000u : 1000u - pm;
    if (counts) counts[(size_t)s * n + e] = c;
    if (off < off_star) { off_star = off; s_star = s; }
    if (c > 0 && c < R) {
      const uint32_t nd = rell_ms_draws(nq, pm);
      if (usable == 0) nd0 = nd;
      else if (nd != nd0) distinct = true;
      ++usable;
    }
  }
  double p = (double)wins[(size_t)s_star * n + i] / Rd, d = NAN, c = NAN;
  if (usable >= 3 && distinct) {
    double Saa = 0.0, Sab = 0.0, Sbb = 0.0, Saz = 0.0, Sbz = 0.0;
    for (uint32_t s = 0; s < S; ++s) {
      const uint32_t cs = wins[(size_t)s * n + i];
      if (cs == 0 || cs >= R) continue;
      const double ps = (double)cs / Rd, rs = (double)rell_ms_draws(nq, sc.pm[s]) / (double)nq;
      const double z = -normcdfinv(ps), as = sqrt(rs), bs = 1.0 / as;
      const double phi = 0.3989422804014327 * exp(-0.5 * z * z);   // 1 / sqrt(2 pi)
      const double w = phi * phi / (ps * (1.0 - ps));
      Saa += w * as * as;
      Sab += w * as * bs;
      Sbb += w * bs * bs;
      Saz += w * as * z;
      Sbz += w * bs * z;
    }
    const double det = Saa * Sbb - Sab * Sab;
    d = (Saz * Sbb - Sbz * Sab) / det;
    c = (Sbz * Saa - Saz * Sab) / det;
    p = normcdf(c - d);
  }
  if (p_au) p_au[e] = p;
  if (fit) { fit[2 * (size_t)e] = d; fit[2 * (size_t)e + 1] = c; }
}

// L[pos]: the site row of sorted position pos summed from site 0 on, one thread per row of the batch
__global__ void __launch_bounds__(256) k_rell_observed(const double* __restrict__ rows, uint32_t pitch, uint32_t pos0,
                                                       uint32_t npos, const uint32_t* __restrict__ order,
                                                       const epa_pair* __restrict__ pairs, const uint32_t* __restrict__ span,
                                                       double* __restrict__ L) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= npos) return;
  const uint32_t nq = span[pairs[order[pos0 + i]].seq_id];
  const double* __restrict__ row = rows + (size_t)i * pitch;
  double s = 0.0;
  for (uint32_t j = 0; j < nq; ++j) s += row[j];
  L[pos0 + i] = s;
}

// T[pos] = (the largest L of the query) - L[pos], one thread per query of the batch
__global__ void __launch_bounds__(256) k_rell_threshold(const RellGroup* __restrict__ groups, uint32_t n_groups,
                                                        const double* __restrict__ L, double* __restrict__ T) {
  const uint32_t g = blockIdx.x * 256 + threadIdx.x;
  if (g >= n_groups) return;
  const RellGroup grp = groups[g];
  double mx = L[grp.start];
  for (uint32_t k = 1; k < grp.count; ++k) mx = fmax(mx, L[grp.start + k]);
  for (uint32_t k = 0; k < grp.count; ++k) T[grp.start + k] = mx - L[grp.start + k];
}

__global__ void __launch_bounds__(RELL_THREADS) k_rell_tests(const RellTestsArgs ta) {
  __shared__ __attribute__((aligned(16))) double mat[LDS_SITES * TE];   // [site][TE]
  __shared__ double part[2][RELL_THREADS / 64][TE];                      // [tile parity][wave][entry]: the waves' weight sums
  __shared__ double elw_l[ACC_LDS];
  __shared__ uint32_t wins_l[ACC_LDS], sh_l[ACC_LDS];
  const RellArgs& a = ta.r;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint32_t flip = 0;
  for (uint32_t g = blockIdx.x; g < a.n_groups; g += gridDim.x) {
    const RellGroup grp = a.groups[g];
    const uint32_t E = grp.count, nq = a.span[grp.q];
    const uint64_t t = a.stream_id ? a.stream_id[grp.q] : (uint64_t)grp.q;
    const uint32_t tlo = (uint32_t)t, thi = (uint32_t)(t >> 32);
    const double* __restrict__ rows = a.rows + (size_t)(grp.start - a.pos0) * a.pitch;
    const uint32_t* __restrict__ ord = a.order + grp.start;
    const double* __restrict__ L = ta.L + grp.start;
    const double* __restrict__ T = ta.T + grp.start;
    const bool in_lds = nq <= LDS_SITES, acc_lds = E <= ACC_LDS;   // workgroup-uniform
    const uint32_t ntiles = (E + TE - 1) / TE;
    const bool resident = ntiles <= (uint32_t)RES_TILES;   // the query's scores stay in registers: no second sweep of draws
    __syncthreads();   // the previous query's tile and accumulators are no longer read
    if (acc_lds)
      for (uint32_t i = tid; i < E; i += RELL_THREADS) { wins_l[i] = 0; sh_l[i] = 0; elw_l[i] = 0.0; }
    __syncthreads();
    for (uint32_t rbase = 0; rbase < a.R; rbase += RELL_THREADS) {
      const uint32_t r = rbase + tid;
      const bool active = r < a.R;
      double sc[TE] = {0.0, 0.0, 0.0, 0.0};
      double keep[RES_TILES][TE] = {};   // indexed by unrolled loops only: registers
      // ---- sweep 1: the winner, m = max s with Z = sum exp(s - m), max c
      double best_sc = 0.0, m = -INFINITY, Z = 0.0, cmax = -INFINITY;
      uint32_t best_br = 0, best_k = 0;
      for (uint32_t tile = 0; tile < ntiles; ++tile) {
        const uint32_t e0 = tile * TE, te = min((uint32_t)TE, E - e0);
        if (in_lds && (ntiles > 1 || rbase == 0)) {   // as k_rell: a query of one tile keeps it for all rounds
          __syncthreads();
          rell_stage_tile(mat, rows, a.pitch, e0, te, nq, tid);
          __syncthreads();
        }
        if (!active) continue;
        rell_tile_scores(mat, rows, a.pitch, e0, te, nq, nq, in_lds, r, tlo, thi, a.k0, a.k1, sc);
        if (resident) {
#pragma unroll
          for (int u = 0; u < RES_TILES; ++u)
            if (tile == (uint32_t)u) {
#pragma unroll
              for (int k = 0; k < TE; ++k) keep[u][k] = sc[k];
            }
        }
        rell_tile_winner(sc, tile == 0, e0, te, a.pairs, ord, best_sc, best_br, best_k);
        double tm = sc[0];
#pragma unroll
        for (int k = 1; k < TE; ++k)
          if ((uint32_t)k < te) tm = fmax(tm, sc[k]);
        if (tm > m) {   // the sum so far refers to the old maximum (first tile: Z = 0 stays 0)
          Z *= exp(m - tm);
          m = tm;
        }
#pragma unroll
        for (int k = 0; k < TE; ++k) {
          if ((uint32_t)k < te) {
            Z += exp(sc[k] - m);
            const double c = sc[k] - L[e0 + k];
            cmax = c > cmax ? c : cmax;
          }
        }
      }
      if (active) {
        if (acc_lds) atomicAdd(&wins_l[best_k], 1u);
        else atomicAdd(&a.wins[grp.start + best_k], 1u);
      }
      // ---- sweep 2: weights and comparisons, every lane of every wave takes part in the sums
      for (uint32_t tile = 0; tile < ntiles; ++tile) {
        const uint32_t e0 = tile * TE, te = min((uint32_t)TE, E - e0);
        if (!resident) {
          if (in_lds) {
            __syncthreads();
            rell_stage_tile(mat, rows, a.pitch, e0, te, nq, tid);
            __syncthreads();
          }
          if (active) rell_tile_scores(mat, rows, a.pitch, e0, te, nq, nq, in_lds, r, tlo, thi, a.k0, a.k1, sc);
        } else {
#pragma unroll
          for (int u = 0; u < RES_TILES; ++u)
            if (tile == (uint32_t)u) {
#pragma unroll
              for (int k = 0; k < TE; ++k) sc[k] = keep[u][k];
            }
        }
        double w[TE];
        uint32_t hits[TE];
#pragma unroll
        for (int k = 0; k < TE; ++k) {
          const bool on = active && (uint32_t)k < te;
          bool hit = false;
          w[k] = 0.0;
          if (on) {
            w[k] = exp(sc[k] - m) / Z;
            const double c = sc[k] - L[e0 + k];
            const double tk = cmax - c;
            hit = tk >= T[e0 + k];
          }
          hits[k] = (uint32_t)__popcll(__ballot(hit));
        }
        epa_wave::wave_sum2(w[0], w[1], w[0], w[1]);
        epa_wave::wave_sum2(w[2], w[3], w[2], w[3]);
        if (lane == 0) {
#pragma unroll
          for (int k = 0; k < TE; ++k) {
            part[flip][wave][k] = w[k];
            if (hits[k]) {
              if (acc_lds) atomicAdd(&sh_l[e0 + k], hits[k]);
              else atomicAdd(&ta.sh[grp.start + e0 + k], hits[k]);
            }
          }
        }
        __syncthreads();
        if (tid < te) {   // one thread per entry: the waves in order, then onto the rounds before
          const double s = ((part[flip][0][tid] + part[flip][1][tid]) + part[flip][2][tid]) + part[flip][3][tid];
          if (acc_lds) elw_l[e0 + tid] += s;
          else ta.elw[grp.start + e0 + tid] += s;
        }
        flip ^= 1u;   // the next tile's partials go to the other half: one barrier per tile is enough
      }
    }
    __syncthreads();
    if (acc_lds)
      for (uint32_t i = tid; i < E; i += RELL_THREADS) {
        a.wins[grp.start + i] = wins_l[i];
        ta.sh[grp.start + i] = sh_l[i];
        ta.elw[grp.start + i] = elw_l[i];
      }
  }
}

__global__ void __launch_bounds__(256) k_rell_tests_out(const uint32_t* __restrict__ wins, const uint32_t* __restrict__ sh,
                                                        const double* __restrict__ elw_sum, const uint32_t* __restrict__ order,
                                                        uint32_t n, double R, double* __restrict__ support,
                                                        double* __restrict__ elw, double* __restrict__ p_sh) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t e = order[i];
  if (support) support[e] = (double)wins[i] / R;
  if (elw) elw[e] = elw_sum[i] / R;
  if (p_sh) p_sh[e] = (double)sh[i] / R;
}

// ---- epa_dev_rell_kh: the KH, the weighted KH and the weighted SH test (include/epa_dev.h)

// The scale w_kk' = 1 / sd(s_k' - s_k) of every ordered pair of entries of the launch's queries of lo .. hi entries: one
// thread per pair, the two sums over the sites sequential in site order.  blockIdx.y splits the pairs of a large query
// over several workgroups.  A skipped pair (the diagonal, q == 0, w not finite) is stored as -1.0
__global__ void __launch_bounds__(64) k_rell_pair_scale(const RellKhArgs ka) {
#pragma clang fp contract(off)   // q adds the ROUNDED product: every step is one fp64 operation
  const RellArgs& a = ka.r;
  for (uint32_t g = blockIdx.x; g < a.n_groups; g += gridDim.x) {
    const RellGroup grp = a.groups[g];
    const uint32_t E = grp.count;
    if (E < ka.lo || E > ka.hi) continue;
    const uint32_t nq = a.span[grp.q];
    const double nqd = (double)nq;
    const double* __restrict__ rows = a.rows + (size_t)(grp.start - a.pos0) * a.pitch;
    double* __restrict__ W = ka.W + ka.woff[g];
    for (uint32_t i = blockIdx.y * 64 + threadIdx.x; i < E * E; i += gridDim.y * 64) {   // E <= 1024: E * E fits
      const uint32_t k = i / E, kp = i - k * E;
      double w = -1.0;
      if (k != kp) {
        const double* __restrict__ xk = rows + (size_t)k * a.pitch;
        const double* __restrict__ xp = rows + (size_t)kp * a.pitch;
        double sum = 0.0;
        for (uint32_t j = 0; j < nq; ++j) sum += xp[j] - xk[j];
        const double m = sum / nqd;
        double q = 0.0;
        for (uint32_t j = 0; j < nq; ++j) {
          const double dev = (xp[j] - xk[j]) - m;
          const double sq = dev * dev;
          q += sq;
        }
        const double inv = 1.0 / sqrt(q);
        if (q != 0.0 && isfinite(inv)) w = inv;   // span 0 (m is NaN, q stays 0.0), span 1 and equal rows: q == 0
      }
      W[i] = w;
    }
  }
}

// Per query: b, the entry with the largest L; per entry k: L_b - L_k, the opponent k* = argmax (L_k' - L_k) w_kk' over the
// pairs not skipped with L_k* - L_k, and T_k, that maximum.  Ties as the winner's: the smaller branch id, then the
// smaller entry index.  b and its copies get no opponent: the weighted tests give them 1.0 as KH does.  One 64-thread workgroup per query, the entries dealt to its threads
__global__ void __launch_bounds__(64) k_rell_kh_thresholds(const RellKhArgs ka) {
#pragma clang fp contract(off)
  const RellArgs& a = ka.r;
  for (uint32_t g = blockIdx.x; g < a.n_groups; g += gridDim.x) {
    const RellGroup grp = a.groups[g];
    const uint32_t E = grp.count;
    const double* __restrict__ L = ka.L + grp.start;
    const uint32_t* __restrict__ ord = a.order + grp.start;
    const double* __restrict__ W = ka.W + ka.woff[g];
    uint32_t b = 0, b_br = a.pairs[ord[0]].branch_id;
    double Lb = L[0];
    for (uint32_t k = 1; k < E; ++k) {
      const double Lk = L[k];
      const uint32_t br = a.pairs[ord[k]].branch_id;
      if (Lk > Lb || (Lk == Lb && br < b_br)) { b = k; b_br = br; Lb = Lk; }
    }
    if (threadIdx.x == 0) ka.best[g] = b;
    for (uint32_t k = threadIdx.x; k < E; k += 64) {
      const double Lk = L[k];
      uint32_t ks = KH_NONE, ks_br = 0;
      double T = 0.0;
      // the best entry, and a copy of it (its pair with b skipped, the same L), is never rejected: no opponent
      const bool top = k == b || (Lb - Lk == 0.0 && !(W[(size_t)b * E + k] >= 0.0));
      for (uint32_t kp = 0; kp < E && !top; ++kp) {
        const double w = W[(size_t)k * E + kp];
        if (!(w >= 0.0)) continue;
        const double val = (L[kp] - Lk) * w;
        const uint32_t br = a.pairs[ord[kp]].branch_id;
        if (ks == KH_NONE || val > T || (val == T && br < ks_br)) { ks = kp; ks_br = br; T = val; }
      }
      const uint32_t pos = grp.start + k;
      ka.D[pos] = Lb - Lk;
      ka.opp[pos] = ks;
      ka.Dw[pos] = ks != KH_NONE ? L[ks] - Lk : 0.0;
      ka.Tw[pos] = T;
    }
  }
}

// the replicates of one wave in which entry `k` of the query is counted by the three tests, added to its counters
__device__ __forceinline__ void rell_kh_count(bool kh, bool wkh, bool wsh, uint32_t lane, uint32_t* c0, uint32_t* c1, uint32_t* c2) {
  const uint32_t n0 = (uint32_t)__popcll(__ballot(kh)), n1 = (uint32_t)__popcll(__ballot(wkh)), n2 = (uint32_t)__popcll(__ballot(wsh));
  if (lane == 0) {
    if (n0) atomicAdd(c0, n0);
    if (n1) atomicAdd(c1, n1);
    if (n2) atomicAdd(c2, n2);
  }
}

// The three counts of epa_dev_rell_kh: the shape of k_rell_tests -- one workgroup per query, thread = replicate, tiles of
// TE entries staged in LDS, the draws regenerated per tile -- and then every entry's centred score against all others.
// SPILL false serves the queries of up to KH_RES entries: the centred scores stay in registers, w and the thresholds in
// LDS.  SPILL true serves the larger ones: a thread writes its centred scores to its own column of the workgroup's row
// of ka.spill ([entry][thread]: a wave's 64 columns are 512 contiguous bytes) and sweeps them in blocks of KH_RES entries
// k against all k', w read from L2 at wave-uniform addresses (w[k'][k .. k + 8): contiguous, w is symmetric).  Integer
// atomics only, in LDS for up to KH_CNT_LDS entries
template <bool SPILL>
__global__ void __launch_bounds__(RELL_THREADS) k_rell_kh(const RellKhArgs ka) {
#pragma clang fp contract(off)
  constexpr uint32_t NC = SPILL ? KH_CNT_LDS : (uint32_t)KH_RES;
  __shared__ __attribute__((aligned(16))) double mat[LDS_SITES * TE];   // [site][TE]
  __shared__ uint32_t cnt_l[3][NC];
  __shared__ double w_l[KH_RES * KH_RES], L_l[KH_RES], D_l[KH_RES], Dw_l[KH_RES], Tw_l[KH_RES];   // SPILL false only
  __shared__ uint32_t opp_l[KH_RES];
  const RellArgs& a = ka.r;
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  for (uint32_t g = blockIdx.x; g < a.n_groups; g += gridDim.x) {
    const RellGroup grp = a.groups[g];
    const uint32_t E = grp.count;
    if (E < ka.lo || E > ka.hi) continue;   // workgroup-uniform, as everything below that guards a barrier
    uint32_t* __restrict__ cnt0 = ka.cnt + grp.start;
    uint32_t* __restrict__ cnt1 = ka.cnt + (size_t)ka.n + grp.start;
    uint32_t* __restrict__ cnt2 = ka.cnt + 2 * (size_t)ka.n + grp.start;
    if (E == 1) {   // nothing to compare with: 1, 1, 1
      if (tid == 0) { cnt0[0] = a.R; cnt1[0] = a.R; cnt2[0] = a.R; }
      continue;
    }
    const uint32_t nq = a.span[grp.q];
    const uint64_t t = a.stream_id ? a.stream_id[grp.q] : (uint64_t)grp.q;
    const uint32_t tlo = (uint32_t)t, thi = (uint32_t)(t >> 32);
    const double* __restrict__ rows = a.rows + (size_t)(grp.start - a.pos0) * a.pitch;
    const double* __restrict__ L = ka.L + grp.start;
    const double* __restrict__ D = ka.D + grp.start;
    const double* __restrict__ Dw = ka.Dw + grp.start;
    const double* __restrict__ Tw = ka.Tw + grp.start;
    const uint32_t* __restrict__ opp = ka.opp + grp.start;
    const double* __restrict__ W = ka.W + ka.woff[g];
    const uint32_t b = ka.best[g];
    const bool in_lds = nq <= LDS_SITES, cnt_lds = E <= NC;
    const uint32_t ntiles = (E + TE - 1) / TE;
    double* __restrict__ col = SPILL ? ka.spill + (size_t)blockIdx.x * ka.spill_pitch + tid : nullptr;   // col[k * 256]
    __syncthreads();   // the previous query's tile, tables and counters are no longer read
    if (cnt_lds)
      for (uint32_t i = tid; i < E; i += RELL_THREADS) { cnt_l[0][i] = 0; cnt_l[1][i] = 0; cnt_l[2][i] = 0; }
    if (!SPILL) {
      if (tid < (uint32_t)KH_RES) {
        const bool on = tid < E;
        L_l[tid] = on ? L[tid] : 0.0;
        D_l[tid] = on ? D[tid] : 0.0;
        Dw_l[tid] = on ? Dw[tid] : 0.0;
        Tw_l[tid] = on ? Tw[tid] : 0.0;
        opp_l[tid] = on ? opp[tid] : KH_NONE;
      }
      if (tid < (uint32_t)(KH_RES * KH_RES)) {
        const uint32_t k = tid / KH_RES, kp = tid % KH_RES;
        w_l[tid] = k < E && kp < E ? W[k * E + kp] : -1.0;
      }
    }
    __syncthreads();
    for (uint32_t rbase = 0; rbase < a.R; rbase += RELL_THREADS) {
      const uint32_t r = rbase + tid;
      const bool active = r < a.R;
      double c[KH_RES] = {};   // SPILL false: indexed by unrolled loops only: registers
      // ---- the centred scores c_k = s_k - L_k of the replicate
      for (uint32_t tile = 0; tile < ntiles; ++tile) {
        const uint32_t e0 = tile * TE, te = min((uint32_t)TE, E - e0);
        if (in_lds && (ntiles > 1 || rbase == 0)) {   // as k_rell: a query of one tile keeps it for all rounds
          __syncthreads();
          rell_stage_tile(mat, rows, a.pitch, e0, te, nq, tid);
          __syncthreads();
        }
        if (!active) continue;
        double sc[TE];
        rell_tile_scores(mat, rows, a.pitch, e0, te, nq, nq, in_lds, r, tlo, thi, a.k0, a.k1, sc);
        if (SPILL) {
#pragma unroll
          for (int k = 0; k < TE; ++k)
            if ((uint32_t)k < te) col[(size_t)(e0 + k) * RELL_THREADS] = sc[k] - L[e0 + k];
        } else {
#pragma unroll
          for (int u = 0; u < KH_RES / TE; ++u)
            if (tile == (uint32_t)u) {
#pragma unroll
              for (int k = 0; k < TE; ++k) c[u * TE + k] = sc[k] - L_l[u * TE + k];
            }
        }
      }
      // ---- every entry against the others; every lane of every wave takes part in the ballots
      if (!SPILL) {
#pragma unroll
        for (int k = 0; k < KH_RES; ++k) {
          if ((uint32_t)k < E) {
            const uint32_t ks = opp_l[k];
            double tk = -INFINITY, d_kh = 0.0, d_wkh = 0.0;
#pragma unroll
            for (int kp = 0; kp < KH_RES; ++kp) {
              if ((uint32_t)kp < E) {
                const double diff = c[kp] - c[k];
                const double w = w_l[k * KH_RES + kp];
                if (w >= 0.0) {
                  const double v = diff * w;
                  tk = v > tk ? v : tk;
                }
                if ((uint32_t)kp == b) d_kh = diff;
                if ((uint32_t)kp == ks) d_wkh = diff;
              }
            }
            const bool none = ks == KH_NONE;
            rell_kh_count(active && d_kh >= D_l[k], active && (none || d_wkh >= Dw_l[k]), active && (none || tk >= Tw_l[k]), lane,
                          &cnt_l[0][k], &cnt_l[1][k], &cnt_l[2][k]);
          }
        }
      } else {
        const double cb = active ? col[(size_t)b * RELL_THREADS] : 0.0;
        for (uint32_t k0 = 0; k0 < E; k0 += KH_RES) {
          const uint32_t nk = min((uint32_t)KH_RES, E - k0);
          double tk[KH_RES];
#pragma unroll
          for (int u = 0; u < KH_RES; ++u) {
            c[u] = active && (uint32_t)u < nk ? col[(size_t)(k0 + u) * RELL_THREADS] : 0.0;
            tk[u] = -INFINITY;
          }
          if (active)
            for (uint32_t kp = 0; kp < E; ++kp) {
              const double cp = col[(size_t)kp * RELL_THREADS];
              const double* __restrict__ wr = W + (size_t)kp * E + k0;   // w[kp][k0 + u] = w[k0 + u][kp]
#pragma unroll
              for (int u = 0; u < KH_RES; ++u) {
                if ((uint32_t)u < nk) {
                  const double w = wr[u];
                  if (w >= 0.0) {
                    const double v = (cp - c[u]) * w;
                    tk[u] = v > tk[u] ? v : tk[u];
                  }
                }
              }
            }
#pragma unroll
          for (int u = 0; u < KH_RES; ++u) {
            if ((uint32_t)u < nk) {
              const uint32_t k = k0 + u, ks = opp[k];
              const bool none = ks == KH_NONE;
              const double d_wkh = active && !none ? col[(size_t)ks * RELL_THREADS] - c[u] : 0.0;
              rell_kh_count(active && cb - c[u] >= D[k], active && (none || d_wkh >= Dw[k]), active && (none || tk[u] >= Tw[k]), lane,
                            cnt_lds ? &cnt_l[0][k] : cnt0 + k, cnt_lds ? &cnt_l[1][k] : cnt1 + k, cnt_lds ? &cnt_l[2][k] : cnt2 + k);
            }
          }
        }
      }
    }
    __syncthreads();
    if (cnt_lds)
      for (uint32_t i = tid; i < E; i += RELL_THREADS) { cnt0[i] = cnt_l[0][i]; cnt1[i] = cnt_l[1][i]; cnt2[i] = cnt_l[2][i]; }
  }
}

__global__ void __launch_bounds__(256) k_rell_kh_out(const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ order,
                                                     uint32_t n, double R, double* __restrict__ p_kh,
                                                     double* __restrict__ p_wkh, double* __restrict__ p_wsh) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t e = order[i];
  if (p_kh) p_kh[e] = (double)cnt[i] / R;
  if (p_wkh) p_wkh[e] = (double)cnt[(size_t)n + i] / R;
  if (p_wsh) p_wsh[e] = (double)cnt[2 * (size_t)n + i] / R;
}

// What the RELL calls share (rell_run): the entries grouped by query, the groups dealt into batches of whole
// queries, the site rows' scratch, the win counters cleared.  `who` names the entry point in error texts
struct RellBatch {
  size_t g0, g1;      // groups [g0, g1)
  uint64_t rows;      // sorted positions of the batch
  uint32_t pitch;     // its longest window
};

struct RellPlan {
  std::vector<RellGroup> groups;
  std::vector<RellBatch> batches;
  RellGroup* d_groups = nullptr;
  uint32_t *d_order = nullptr, *d_wins = nullptr;
  double* d_rows = nullptr;
};

int rell_plan(epa_ctx* ctx, const char* who, const epa_pair* d_pairs, uint32_t n, const uint32_t* h_span, uint32_t Q,
              RellPlan& plan) {
  std::vector<RellGroup>& groups = plan.groups;
  std::vector<RellBatch>& batches = plan.batches;
  // ---- group by query: stable sort of the entry indices by seq_id
  EntryGroups eg;
  int grc = launch_group_entries(ctx, d_pairs, n, Q, 1, &eg);
  if (grc) return grc;
  const uint32_t* d_bounds = eg.bounds;
  uint32_t *d_order = eg.order, *d_wins = eg.extra;
  EPA_HIP(ctx, hipMemsetAsync(d_wins, 0, sizeof(uint32_t) * (size_t)n, ctx->stream));
  std::vector<uint32_t> bounds(2 * (size_t)Q);
  EPA_HIP(ctx, hipMemcpyAsync(bounds.data(), d_bounds, sizeof(uint32_t) * 2 * (size_t)Q, hipMemcpyDeviceToHost, ctx->stream));
  EPA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  uint64_t covered = 0;
  for (uint32_t q = 0; q < Q; ++q)
    if (bounds[Q + q] > bounds[q]) {
      groups.push_back(RellGroup{q, bounds[q], bounds[Q + q] - bounds[q]});
      covered += groups.back().count;
    }
  if (covered != n) return epa_fail(ctx, EPA_ERR_INVALID_ARG, std::string(who) + ": a sequence id is out of range");
  RellGroup* d_groups = (RellGroup*)epa_scratch(ctx, SLOT_RELL_GROUPS, sizeof(RellGroup) * groups.size());
  if (!d_groups) return epa_fail(ctx, EPA_ERR_HIP, "hipMalloc(rell groups)");
  EPA_HIP(ctx, hipMemcpyAsync(d_groups, groups.data(), sizeof(RellGroup) * groups.size(), hipMemcpyHostToDevice, ctx->stream));

  // ---- batches of whole queries: rows [positions][pitch], pitch = the batch's longest window
  size_t rows_bytes = 0;
  for (size_t g0 = 0; g0 < groups.size();) {
    RellBatch b{g0, g0, 0, 1};
    while (b.g1 < groups.size()) {
      const uint32_t p = std::max(b.pitch, h_span[groups[b.g1].q]);
      if (b.g1 > g0 && (b.rows + groups[b.g1].count) * (uint64_t)p * sizeof(double) > ROWS_BUDGET) break;
      b.rows += groups[b.g1].count;
      b.pitch = p;
      ++b.g1;
    }
    rows_bytes = std::max(rows_bytes, (size_t)b.rows * b.pitch * sizeof(double));
    batches.push_back(b);
    g0 = b.g1;
  }
  plan.d_rows = (double*)epa_scratch(ctx, SLOT_RELL_ROWS, rows_bytes);
  if (!plan.d_rows) return epa_fail(ctx, EPA_ERR_HIP, "hipMalloc(rell site rows)");
  plan.d_groups = d_groups;
  plan.d_order = d_order;
  plan.d_wins = d_wins;
  return EPA_OK;
}

// what does not change from batch to batch
RellArgs rell_args(const RellPlan& plan, const EntryStage& e, const RellDraws& dr) {
  RellArgs a{};
  a.order = plan.d_order;
  a.pairs = e.d_pairs;
  a.span = e.d_span;
  a.stream_id = dr.d_stream_id;
  a.rows = plan.d_rows;
  a.R = dr.replicates;
  a.k0 = (uint32_t)dr.seed;
  a.k1 = (uint32_t)(dr.seed >> 32);
  a.wins = plan.d_wins;
  return a;
}

// the batch's site rows computed and its part of the arguments set
int rell_batch_rows(epa_ctx* ctx, const RellPlan& plan, const RellBatch& b, const EntryStage& e, RellArgs& a) {
  const uint32_t pos0 = plan.groups[b.g0].start;
  int rc = launch_site_lnl(ctx, e, plan.d_order + pos0, b.rows, b.pitch, plan.d_rows, SITES_PLAIN);
  if (rc) return rc;
  a.groups = plan.d_groups + b.g0;
  a.n_groups = (uint32_t)(b.g1 - b.g0);
  a.pos0 = pos0;
  a.pitch = b.pitch;
  return EPA_OK;
}

// One RELL call, timed as `timer`.  The variant supplies prepare(plan, a) -> status: its own scratch cleared, a.wins
// redirected if it counts elsewhere, whatever of the plan it refuses; batch(plan, b, a, grid): its kernels on a batch whose site rows are ready, `grid` the workgroups of
// the kernel that runs one query each; finish(plan, grid): the kernel that writes the outputs, one thread per entry
template <class Prepare, class Batch, class Finish>
int rell_run(epa_ctx* ctx, const char* who, int timer, const EntryStage& e, const RellDraws& dr, Prepare prepare, Batch batch,
             Finish finish) {
  const uint32_t n = (uint32_t)e.n;   // the caller checked e.n < 2^32
  epa_timer_start(ctx, epa_t(ctx, timer));
  RellPlan plan;
  int rc = rell_plan(ctx, who, e.d_pairs, n, e.h_span, e.Q, plan);
  if (rc) return rc;
  RellArgs a = rell_args(plan, e, dr);
  rc = prepare(plan, a);
  if (rc) return rc;
  for (const RellBatch& b : plan.batches) {
    rc = rell_batch_rows(ctx, plan, b, e, a);
    if (rc) return rc;
    batch(plan, b, a, dim3((uint32_t)std::min<uint64_t>(a.n_groups, (uint64_t)ctx->n_cu * 8)));
    EPA_HIP(ctx, hipGetLastError());
  }
  finish(plan, dim3((n + 255) / 256));
  epa_timer_stop(ctx, epa_t(ctx, timer));
  EPA_HIP(ctx, hipGetLastError());
  return EPA_OK;
}

}  // namespace

int launch_group_entries(epa_ctx* ctx, const epa_pair* d_pairs, uint32_t n, uint32_t Q, uint32_t extra_arrays, EntryGroups* g) {
  const dim3 ngrid((n + 255) / 256);
  int bits = 1;
  while (bits < 32 && ((uint64_t)1 << bits) < (uint64_t)Q) ++bits;
  size_t temp_bytes = 0;
  (void)rocprim::radix_sort_pairs<epa_radix_cfg>(nullptr, temp_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                                 (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)n, 0, bits, ctx->stream);
  const size_t nb = (sizeof(uint32_t) * (size_t)n + 255) & ~(size_t)255;
  char* base = (char*)epa_scratch(ctx, SLOT_RELL_SORT, (4 + (size_t)extra_arrays) * nb + temp_bytes);
  uint32_t* d_bounds = (uint32_t*)epa_scratch(ctx, SLOT_RELL_BOUNDS, sizeof(uint32_t) * 2 * (size_t)Q);
  if (!base || !d_bounds) return epa_fail(ctx, EPA_ERR_HIP, "hipMalloc(entry grouping)");
  uint32_t *d_keys = (uint32_t*)base, *d_idx = (uint32_t*)(base + nb), *d_sorted = (uint32_t*)(base + 2 * nb);
  uint32_t* d_order = (uint32_t*)(base + 3 * nb);
  void* temp = base + (4 + (size_t)extra_arrays) * nb;
  hipLaunchKernelGGL(k_rell_keys, ngrid, dim3(256), 0, ctx->stream, d_pairs, n, d_keys, d_idx);
  EPA_HIP(ctx, rocprim::radix_sort_pairs<epa_radix_cfg>(temp, temp_bytes, d_keys, d_sorted, d_idx, d_order, (size_t)n, 0, bits,
                                                        ctx->stream));
  EPA_HIP(ctx, hipMemsetAsync(d_bounds, 0, sizeof(uint32_t) * 2 * (size_t)Q, ctx->stream));
  hipLaunchKernelGGL(k_rell_bounds, ngrid, dim3(256), 0, ctx->stream, d_sorted, n, Q, d_bounds);
  EPA_HIP(ctx, hipGetLastError());
  *g = EntryGroups{d_sorted, d_order, d_bounds, extra_arrays ? (uint32_t*)(base + 4 * nb) : nullptr};
  return EPA_OK;
}

int launch_rell(epa_ctx* ctx, const EntryStage& e, const RellDraws& dr, double* d_support) {
  return rell_run(
      ctx, "rell_support", epa_ctx::T_RELL, e, dr, [](const RellPlan&, RellArgs&) -> int { return EPA_OK; },
      [&](const RellPlan&, const RellBatch&, const RellArgs& a, dim3 grid) {
        hipLaunchKernelGGL(k_rell, grid, dim3(RELL_THREADS), 0, ctx->stream, a);
      },
      [&](const RellPlan& plan, dim3 grid) {
        hipLaunchKernelGGL(k_rell_support, grid, dim3(256), 0, ctx->stream, plan.d_wins, plan.d_order, (uint32_t)e.n,
                           (double)dr.replicates, d_support);
      });
}

int launch_rell_tests(epa_ctx* ctx, const EntryStage& e, const RellDraws& dr, double* d_support, double* d_elw, double* d_p_sh) {
  const uint32_t n = (uint32_t)e.n;
  double *d_L = nullptr, *d_T = nullptr;
  RellTestsArgs ta{};
  return rell_run(
      ctx, "rell_tests", epa_ctx::T_RELL_TESTS, e, dr,
      [&](const RellPlan&, RellArgs&) -> int {
        // [L n | T n | weight sums n | SH counts n]; the two accumulators are cleared per call, L and T written in full
        const size_t db = (sizeof(double) * (size_t)n + 255) & ~(size_t)255;
        char* base = (char*)epa_scratch(ctx, SLOT_RELL_TESTS, 3 * db + sizeof(uint32_t) * (size_t)n);
        if (!base) return epa_fail(ctx, EPA_ERR_HIP, "hipMalloc(rell_tests accumulators)");
        ta.L = d_L = (double*)base;
        ta.T = d_T = (double*)(base + db);
        ta.elw = (double*)(base + 2 * db);
        ta.sh = (uint32_t*)(base + 3 * db);
        EPA_HIP(ctx, hipMemsetAsync(ta.elw, 0, db + sizeof(uint32_t) * (size_t)n, ctx->stream));
        return EPA_OK;
      },
      [&](const RellPlan& plan, const RellBatch& b, const RellArgs& a, dim3 grid) {
        const uint32_t npos = (uint32_t)b.rows;
        ta.r = a;
        hipLaunchKernelGGL(k_rell_observed, dim3((npos + 255) / 256), dim3(256), 0, ctx->stream, plan.d_rows, b.pitch, a.pos0,
                           npos, plan.d_order, e.d_pairs, e.d_span, d_L);
        hipLaunchKernelGGL(k_rell_threshold, dim3((a.n_groups + 255) / 256), dim3(256), 0, ctx->stream, a.groups, a.n_groups, d_L, d_T);
        hipLaunchKernelGGL(k_rell_tests, grid, dim3(RELL_THREADS), 0, ctx->stream, ta);
      },
      [&](const RellPlan& plan, dim3 grid) {
        hipLaunchKernelGGL(k_rell_tests_out, grid, dim3(256), 0, ctx->stream, plan.d_wins, ta.sh, ta.elw, plan.d_order, n,
                           (double)dr.replicates, d_support, d_elw, d_p_sh);
      });
}

int launch_rell_au(epa_ctx* ctx, const EntryStage& e, const RellDraws& dr, const uint32_t* h_scale_pm, uint32_t n_scales,
                   double* d_p_au, uint32_t* d_counts, double* d_fit) {
  const uint32_t n = (uint32_t)e.n;   // the caller checked n_scales <= MS_SCALES
  const size_t cbytes = sizeof(uint32_t) * (size_t)n_scales * n;
  uint32_t* d_ms = nullptr;
  RellMsArgs ma{};
  ma.sc.n = n_scales;
  for (uint32_t s = 0; s < n_scales; ++s) ma.sc.pm[s] = h_scale_pm[s];
  ma.n = n;
  return rell_run(
      ctx, "rell_au", epa_ctx::T_RELL_AU, e, dr,
      [&](const RellPlan&, RellArgs& a) -> int {   // the win counters [scale][n] by sorted position, cleared per call
        a.wins = d_ms = (uint32_t*)epa_scratch(ctx, SLOT_RELL_AU, cbytes);
        if (!d_ms) return epa_fail(ctx, EPA_ERR_HIP, "hipMalloc(rell_au counters)");
        EPA_HIP(ctx, hipMemsetAsync(d_ms, 0, cbytes, ctx->stream));
        return EPA_OK;
      },
      [&](const RellPlan&, const RellBatch&, const RellArgs& a, dim3 grid) {
        ma.r = a;
        hipLaunchKernelGGL(k_rell_ms, grid, dim3(RELL_THREADS), 0, ctx->stream, ma);
      },
      [&](const RellPlan& plan, dim3 grid) {
        hipLaunchKernelGGL(k_rell_au_fit, grid, dim3(256), 0, ctx->stream, d_ms, plan.d_order, e.d_pairs, e.d_span, ma.sc, n,
                           dr.replicates, d_p_au, d_counts, d_fit);
      });
}

int launch_rell_kh(epa_ctx* ctx, const EntryStage& e, const RellDraws& dr, double* d_p_kh, double* d_p_wkh, double* d_p_wsh) {
  const uint32_t n = (uint32_t)e.n;
  // a batch's queries are worked off in ranges whose scale matrices fit KH_W_BUDGET (one query's always do)
  struct Range {
    size_t g0, g1;                    // groups [g0, g1)
    uint32_t small, large, widest;    // queries of up to KH_RES entries, of more, and the most entries among those
  };
  std::vector<Range> ranges;
  std::vector<uint64_t> woff;         // per group: where its matrix begins in the range's W
  size_t next_range = 0;
  uint32_t spill_grid = 0;
  const uint64_t* d_woff = nullptr;
  uint32_t* d_best = nullptr;
  RellKhArgs ka{};
  return rell_run(
      ctx, "rell_kh", epa_ctx::T_RELL_KH, e, dr,
      [&](const RellPlan& plan, RellArgs&) -> int {
        const size_t G = plan.groups.size();
        woff.resize(G);
        size_t w_most = 0, large_most = 0;
        uint32_t widest = 0;
        for (const RellBatch& b : plan.batches)
          for (size_t g = b.g0; g < b.g1;) {
            Range r{g, g, 0, 0, 0};
            size_t w = 0;
            while (r.g1 < b.g1) {
              const uint32_t K = plan.groups[r.g1].count;
              if (K > KH_MAX_ENTRIES)
                return epa_fail(ctx, EPA_ERR_INVALID_ARG, "rell_kh: query " + std::to_string(plan.groups[r.g1].q) + " has " +
                                                              std::to_string(K) + " entries; at most " +
                                                              std::to_string(KH_MAX_ENTRIES) + " per query in this call");
              if (r.g1 > g && (w + (size_t)K * K) * sizeof(double) > KH_W_BUDGET) break;
              woff[r.g1] = w;
              w += (size_t)K * K;
              if (K > (uint32_t)KH_RES) { ++r.large; r.widest = std::max(r.widest, K); }
              else ++r.small;
              ++r.g1;
            }
            w_most = std::max(w_most, w);
            large_most = std::max(large_most, (size_t)r.large);
            widest = std::max(widest, r.widest);
            ranges.push_back(r);
            g = r.g1;
          }
        // the workgroups of the spilling launch: what KH_SPILL_BUDGET holds of rows of `widest` entries x 256 threads
        const size_t spill_row = sizeof(double) * (size_t)widest * RELL_THREADS;
        if (widest)
          spill_grid = (uint32_t)std::min<size_t>(std::min<size_t>(large_most, (size_t)ctx->n_cu * 8),
                                                  std::max<size_t>(1, KH_SPILL_BUDGET / spill_row));
        // [L n | D n | Dw n | Tw n | opp n | counters 3 n | woff G | best G | W | spill]; the counters are cleared per call,
        // everything else is written before it is read
        auto al = [](size_t bytes) { return (bytes + 255) & ~(size_t)255; };
        const size_t db = al(sizeof(double) * (size_t)n), ub = al(sizeof(uint32_t) * (size_t)n);
        const size_t cb = al(3 * sizeof(uint32_t) * (size_t)n), wo = al(sizeof(uint64_t) * G), bb = al(sizeof(uint32_t) * G);
        const size_t wb = al(sizeof(double) * w_most);
        char* base = (char*)epa_scratch(ctx, SLOT_RELL_KH, 4 * db + ub + cb + wo + bb + wb + spill_row * spill_grid);
        if (!base) return epa_fail(ctx, EPA_ERR_HIP, "hipMalloc(rell_kh scratch)");
        ka.L = (double*)base;
        ka.D = (double*)(base + db);
        ka.Dw = (double*)(base + 2 * db);
        ka.Tw = (double*)(base + 3 * db);
        ka.opp = (uint32_t*)(base + 4 * db);
        ka.cnt = (uint32_t*)(base + 4 * db + ub);
        d_woff = (const uint64_t*)(base + 4 * db + ub + cb);
        d_best = (uint32_t*)(base + 4 * db + ub + cb + wo);
        ka.W = (double*)(base + 4 * db + ub + cb + wo + bb);
        ka.spill = (double*)(base + 4 * db + ub + cb + wo + bb + wb);
        ka.spill_pitch = widest * RELL_THREADS;
        ka.n = n;
        EPA_HIP(ctx, hipMemsetAsync(ka.cnt, 0, 3 * sizeof(uint32_t) * (size_t)n, ctx->stream));
        EPA_HIP(ctx, hipMemcpyAsync((void*)d_woff, woff.data(), sizeof(uint64_t) * G, hipMemcpyHostToDevice, ctx->stream));
        return EPA_OK;
      },
      [&](const RellPlan& plan, const RellBatch& b, const RellArgs& a, dim3) {
        const uint32_t npos = (uint32_t)b.rows;
        hipLaunchKernelGGL(k_rell_observed, dim3((npos + 255) / 256), dim3(256), 0, ctx->stream, plan.d_rows, b.pitch, a.pos0,
                           npos, plan.d_order, e.d_pairs, e.d_span, (double*)ka.L);
        for (; next_range < ranges.size() && ranges[next_range].g1 <= b.g1; ++next_range) {
          const Range& r = ranges[next_range];
          ka.r = a;
          ka.r.groups = plan.d_groups + r.g0;
          ka.r.n_groups = (uint32_t)(r.g1 - r.g0);
          ka.woff = d_woff + r.g0;
          ka.best = d_best + r.g0;
          const uint32_t per_query = (uint32_t)std::min<uint64_t>(ka.r.n_groups, (uint64_t)ctx->n_cu * 32);   // one wave each
          if (r.small) {
            ka.lo = 1;
            ka.hi = KH_RES;
            hipLaunchKernelGGL(k_rell_pair_scale, dim3(per_query), dim3(64), 0, ctx->stream, ka);
          }
          if (r.large) {
            ka.lo = KH_RES + 1;
            ka.hi = KH_MAX_ENTRIES;
            const uint32_t slices = std::min<uint32_t>(64, (r.widest * r.widest + 63) / 64);
            hipLaunchKernelGGL(k_rell_pair_scale, dim3(per_query, slices), dim3(64), 0, ctx->stream, ka);
          }
          hipLaunchKernelGGL(k_rell_kh_thresholds, dim3(per_query), dim3(64), 0, ctx->stream, ka);
          if (r.small) {
            ka.lo = 1;
            ka.hi = KH_RES;
            hipLaunchKernelGGL(k_rell_kh<false>, dim3((uint32_t)std::min<uint64_t>(ka.r.n_groups, (uint64_t)ctx->n_cu * 8)),
                               dim3(RELL_THREADS), 0, ctx->stream, ka);
          }
          if (r.large) {
            ka.lo = KH_RES + 1;
            ka.hi = KH_MAX_ENTRIES;
            hipLaunchKernelGGL(k_rell_kh<true>, dim3(std::min(r.large, spill_grid)), dim3(RELL_THREADS), 0, ctx->stream, ka);
          }
        }
      },
      [&](const RellPlan& plan, dim3 grid) {
        hipLaunchKernelGGL(k_rell_kh_out, grid, dim3(256), 0, ctx->stream, ka.cnt, plan.d_order, n, (double)dr.replicates, d_p_kh,
                           d_p_wkh, d_p_wsh);
      });
}
