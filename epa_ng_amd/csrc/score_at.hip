// Log-likelihood of given placements at GIVEN branch lengths: no optimiser runs.
//
// Mapping to the reference: Tiny_Tree::place with opt_branches == false (src/tree/Tiny_Tree.cpp:186-204) after the
// three branch lengths were set -- pll_update_prob_matrices on the three edges, pll_update_partials of the inner node
// toward the query, pll_compute_edge_loglikelihood on the pendant edge, over the sites of the query's window.  It is
// the quantity score() of k_thorough_generic (thorough_generic.hip) forms between its Newton rounds, as a kernel of
// its own: no sumtable is kept, so there is no HBM slab and nothing is read but refT, scSum, cinv, blen and the model
// -- the kernel serves the resident and the blocked lookup layout alike and every shape a context can have (4 / 20
// states, 1 .. EPA_MAX_CATS categories with padded ones at weight 0, +I, both scaler modes after k_align_rates,
// verbatim eigenvalues).
// The SITES instantiation (epa_dev_site_lnl, the site rows of epa_dev_rell_support) stores the per-site terms of that
// lnL instead of their sum.
//
// One wavefront per entry, lane = site of the window (runtime loop over 64-site chunks), a persistent grid over the
// entries.  Per entry the wave keeps exp(lam_x r_k t) for the distal, the proximal and (times w_k) the pendant length
// in LDS; operand rows come from refT component-major, 64 consecutive sites of one component = one 512-byte segment.
#include "epa_dev_internal.hpp"
#include "wave_util.hpp"

#include <algorithm>

namespace {

using namespace epa_wave;

struct ScArgs {
  const ModelDev* m;
  const double* refT;      // [2B][c*s][W]
  const uint32_t* scSum;   // [B][W] proximal + distal scaler counts
  const double* cinv;      // +I: [W] p * pi_inv per site, or null
  double inv_w0;
  const double* blen;
  const epa_pair* pairs;
  const double* pendant;
  const double* distal;
  const double* proximal;  // null: blen[b] - distal
  const uint8_t* codes;
  uint32_t cstride, crel;
  const double* qe;        // PROFILE instantiations: eigen-space query rows [Q][qstride][S] in place of codes
  uint32_t qstride;
  const uint32_t* win_begin;
  const uint32_t* win_span;
  double* lnl;
  uint64_t n;
  uint32_t W;
  // SITES instantiation only: row i of `rows` ([n][pitch]) takes entry order[i] (null: entry i)
  const uint32_t* order;
  double* rows;
  uint32_t pitch;
  uint32_t pad;            // 1: the columns from the span up to the pitch are written as 0.0
};

constexpr double LN2 = 0.6931471805599453094;
// 32 x 2^-53: an entry of a back-transformed CLV below this fraction of its terms' magnitude sum is rounding residue
constexpr double NOISE_CUT = 0x1p-48;

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// SITES: instead of the entry's lnL the kernel stores what it is the sum of -- per lane log(l0) - 256 count ln 2, one
// coalesced 512-byte store per 64-site chunk -- into row i of a.rows; the lnL instantiation is the code it was.
// PROFILE: the query's eigen-space vector of a site is read from a.qe (a per-site likelihood row brought to the
// eigenbasis by k_profile_eigen, profile.hip) instead of the table entry of the site's column code; nothing else differs.
template <int S, bool SITES, bool PROFILE = false>
__global__ void __launch_bounds__(64) k_score_at(const ScArgs a) {
  __shared__ __attribute__((aligned(16))) double U[S * S];
  __shared__ __attribute__((aligned(16))) double UiT[S * S];   // [i][x] = U^-1[x][i]
  __shared__ __attribute__((aligned(16))) double tab[3][EPA_MAX_CATS * S];
  const int lane = threadIdx.x;
  const ModelDev* __restrict__ m = a.m;
  const int c = m->c, cs = c * S;
  for (int i = lane; i < S * S; i += 64) { U[i] = m->U[i]; UiT[(i % S) * S + i / S] = m->Ui[i]; }
  __syncthreads();
  const size_t cW = a.W;
  constexpr int UNROLL_I = S == 4 ? 4 : 1;

  for (uint64_t row = blockIdx.x; row < a.n; row += gridDim.x) {
    uint64_t e = row;
    if constexpr (SITES) { if (a.order) e = a.order[row]; }
    const epa_pair pr = a.pairs[e];
    const uint32_t b = pr.branch_id, q = pr.seq_id;
    const uint32_t begin = a.win_begin[q], n = a.win_span[q];
    const uint32_t nch = (n + 63) / 64;
    const double* Xt = a.refT + (size_t)(2 * b) * cs * cW + begin;       // proximal side
    const double* Dt = a.refT + (size_t)(2 * b + 1) * cs * cW + begin;   // distal side
    const uint32_t* scp = a.scSum + (size_t)b * cW + begin;
    const uint8_t* qc = nullptr;
    const double* qrow = nullptr;
    if constexpr (PROFILE) qrow = a.qe + (size_t)q * a.qstride * S;
    else qc = a.codes + (size_t)q * a.cstride + (a.crel ? 0u : begin);
    const double tp = a.pendant[e], td = a.distal[e];
    const double tx = a.proximal ? a.proximal[e] : a.blen[b] - td;

    // wave-uniform tables of this entry: exp(lr td), exp(lr tx), w_k exp(lr tp).  The wave runs entry after entry:
    // the first barrier keeps these writes behind the previous entry's reads, the second the reads below behind them.
    wave_sync();
    for (int i = lane; i < cs; i += 64) {
      const int k = i / S, x = i - k * S;
      const double lr = m->lam[x] * m->rate[k];
      tab[0][i] = exp(lr * td);
      tab[1][i] = exp(lr * tx);
      tab[2][i] = m->w[k] * exp(lr * tp);
    }
    wave_sync();

    double mant = 1.0;
    int ex = 0;
    for (uint32_t ch = 0; ch < nch; ++ch) {
      const uint32_t site = ch * 64 + lane;
      const bool valid = site < n;
      const uint32_t s = valid ? site : 0;
      const double* qv;
      if constexpr (PROFILE) qv = qrow + (size_t)s * S;
      else qv = m->qt + (size_t)qc[s] * S;
      double l0 = 0.0;
      bool all_small = true;
      for (int k = 0; k < c; ++k) {
        // inner CLV toward the query: I_i = (U (e_d o D_k))_i (U (e_x o X_k))_i
        double av[S], bv[S], acc[S];
#pragma unroll
        for (int x = 0; x < S; ++x) {
          av[x] = Dt[(size_t)(k * S + x) * cW + s] * tab[0][k * S + x];
          bv[x] = Xt[(size_t)(k * S + x) * cW + s] * tab[1][k * S + x];
          acc[x] = 0.0;
        }
        // row i of U and of (U^-1)^T per step: with 20 states the loop stays rolled, so the 2 x 400 matrix entries are
        // read from LDS where they are used instead of being hoisted into (and spilled from) registers
        double mx = 0.0;
#pragma unroll UNROLL_I
        for (int i = 0; i < S; ++i) {
          const double* Ur = U + i * S;
          double p = Ur[0] * av[0], r = Ur[0] * bv[0];
          double pb = fabs(p), rb = fabs(r);   // sum of the terms' magnitudes: the scale of the sums' rounding error
#pragma unroll
          for (int x = 1; x < S; ++x) {
            p = fma(Ur[x], av[x], p);
            r = fma(Ur[x], bv[x], r);
            pb = fma(fabs(Ur[x]), fabs(av[x]), pb);
            rb = fma(fabs(Ur[x]), fabs(bv[x]), rb);
          }
          // A state-space entry that does not exceed its own rounding-error bound is zero: libpll keeps CLVs in state
          // space, where a state a tip excludes is exactly 0 at branch length 0 (P(0) is the identity matrix), whereas
          // U (e o U^-1 clv) leaves a residue of a few ulp of the terms there -- which a tiny pendant length divides by
          // wherever the query shows such a state.  NOISE_CUT bounds the rounding of an S-term sum of rounded operands
          // and of U U^-1 = I itself (32 unit roundoffs of the magnitude sum).
          if (fabs(p) <= NOISE_CUT * pb) p = 0.0;
          if (fabs(r) <= NOISE_CUT * rb) r = 0.0;
          const double Ii = p * r;
          mx = fmax(mx, Ii);
          const double* Vr = UiT + i * S;
#pragma unroll
          for (int x = 0; x < S; ++x) acc[x] = fma(Vr[x], Ii, acc[x]);   // (U^-1 I)_x, summed over i in order
        }
        all_small = all_small && mx < 0x1p-256;   // pll_update_partials: every entry below 2^-256
        // edge lnL on the pendant edge: sum_x (U^-1 I)_x q_x w_k exp(lr tp)
        double l = 0.0;
#pragma unroll
        for (int x = 0; x < S; ++x) l = fma(acc[x] * qv[x], tab[2][k * S + x], l);
        l0 += l;
      }
      // per-site scaling: all c * s entries below the threshold -> * 2^256, count + 1
      uint32_t count = scp[s];
      if (all_small) { l0 *= 0x1p+256; ++count; }
      if (a.cinv)   // +I: p * pi_inv enters L_0 only, unscaled (thorough_generic.hip)
        l0 = fma(a.cinv[begin + s] * a.inv_w0, tab[2][0], l0);
      if constexpr (SITES) {
        if (valid) a.rows[row * a.pitch + site] = log(l0) - (double)(256 * (int)count) * LN2;
        continue;
      }
      if (!valid) { l0 = 1.0; count = 0; }
      mant *= __builtin_amdgcn_frexp_mant(l0);
      ex += __builtin_amdgcn_frexp_exp(l0) - 256 * (int)count;
      ex += __builtin_amdgcn_frexp_exp(mant);
      mant = __builtin_amdgcn_frexp_mant(mant);
    }
    if constexpr (SITES) {
      if (a.pad)
        for (uint32_t j = n + lane; j < a.pitch; j += 64) a.rows[row * a.pitch + j] = 0.0;
    } else {
      const double lnl = wave_sum(log(mant) + (double)ex * LN2);
      if (lane == 0) a.lnl[e] = lnl;
    }
  }
}

}  // namespace

static void fill_args(epa_ctx* ctx, ScArgs& a, const EntryStage& e, uint64_t n) {
  a.m = ctx->dmodel;
  a.refT = ctx->refT;
  a.scSum = ctx->scSum;
  a.cinv = ctx->cinv;
  a.inv_w0 = ctx->inv_w0;
  a.blen = ctx->blen;
  a.pairs = e.d_pairs;
  a.pendant = e.d_pen;
  a.distal = e.d_dis;
  a.proximal = e.d_prx;
  a.codes = e.d_codes;
  a.qe = e.d_qe;
  a.qstride = e.qe_stride;
  a.crel = ctx->code_stride ? 1u : 0u;
  a.cstride = a.crel ? ctx->code_stride : ctx->W;
  a.win_begin = e.d_begin;
  a.win_span = e.d_span;
  a.lnl = nullptr;
  a.n = n;
  a.W = ctx->W;
  a.order = nullptr;
  a.rows = nullptr;
  a.pitch = 0;
  a.pad = 0;
}

int launch_score_at(epa_ctx* ctx, const EntryStage& e, double* d_lnl) {
  ScArgs a;
  fill_args(ctx, a, e, e.n);
  a.lnl = d_lnl;
  // persistent grid: neither n nor a branch id reaches a grid dimension
  const uint32_t grid = (uint32_t)std::min<uint64_t>(e.n, (uint64_t)ctx->n_cu * 8);
  epa_timer_start(ctx, epa_t(ctx, epa_ctx::T_SCORE));
  if (a.qe) {   // profile queries
    if (ctx->s == 4) hipLaunchKernelGGL((k_score_at<4, false, true>), dim3(grid), dim3(64), 0, ctx->stream, a);
    else hipLaunchKernelGGL((k_score_at<20, false, true>), dim3(grid), dim3(64), 0, ctx->stream, a);
  } else if (ctx->s == 4) hipLaunchKernelGGL((k_score_at<4, false>), dim3(grid), dim3(64), 0, ctx->stream, a);
  else hipLaunchKernelGGL((k_score_at<20, false>), dim3(grid), dim3(64), 0, ctx->stream, a);
  epa_timer_stop(ctx, epa_t(ctx, epa_ctx::T_SCORE));
  EPA_HIP(ctx, hipGetLastError());
  return EPA_OK;
}

int launch_site_lnl(epa_ctx* ctx, const EntryStage& e, const uint32_t* d_order, uint64_t n_rows, uint32_t pitch,
                    double* d_rows, unsigned flags) {
  ScArgs a;
  fill_args(ctx, a, e, n_rows);
  a.order = d_order;
  a.rows = d_rows;
  a.pitch = pitch;
  a.pad = flags & SITES_PAD ? 1u : 0u;
  const bool timed = flags & SITES_TIMED;
  const uint32_t grid = (uint32_t)std::min<uint64_t>(n_rows, (uint64_t)ctx->n_cu * 8);
  if (timed) epa_timer_start(ctx, epa_t(ctx, epa_ctx::T_SITES));
  if (a.qe) {   // profile queries
    if (ctx->s == 4) hipLaunchKernelGGL((k_score_at<4, true, true>), dim3(grid), dim3(64), 0, ctx->stream, a);
    else hipLaunchKernelGGL((k_score_at<20, true, true>), dim3(grid), dim3(64), 0, ctx->stream, a);
  } else if (ctx->s == 4) hipLaunchKernelGGL((k_score_at<4, true>), dim3(grid), dim3(64), 0, ctx->stream, a);
  else hipLaunchKernelGGL((k_score_at<20, true>), dim3(grid), dim3(64), 0, ctx->stream, a);
  if (timed) epa_timer_stop(ctx, epa_t(ctx, epa_ctx::T_SITES));
  EPA_HIP(ctx, hipGetLastError());
  return EPA_OK;
}
