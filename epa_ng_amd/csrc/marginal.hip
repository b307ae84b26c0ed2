// Marginal likelihood of "read q sits somewhere on edge b": the lnL of k_score_at (score_at.hip) on a whole
// (distal x pendant) grid per entry, folded with the caller's log weights into one log-sum-exp (include/epa_dev.h,
// epa_dev_marginal_like, states the rule).  No reference counterpart: EPA-ng has no such mode (pplacer's -p is the
// motivation, not a parity target).
//
// Outer shape of k_score_at: one wavefront per entry, lane = site of the window (runtime loop over 64-site chunks), a
// persistent grid, nothing read but refT, scSum, cinv, blen and the model -- the same bits in the resident and the
// blocked lookup layout, every shape a context can have.
//
// What it saves against Kx * Kp score evaluations: everything up to g_x = (U^-1 I)_x q_x -- two S x S products with
// their magnitude sums, the noise cut, the all_small decision, the back-transform -- depends on the distal node only
// and is formed ONCE per (distal node, chunk, category); only the contraction of g against w_k exp(lam_x r_k p_j)
// runs per pendant node, against the LDS table tabP of a tile of TJ = 16 pendant nodes, into per-lane l0[j] /
// mant[j] / ex[j] accumulators (one wave_sum per (distal node, j) at the end of the node).  Inside a site the operand
// order is k_score_at's: the same fma chains, the same NOISE_CUT test, tabP[j][0] (score_at's tab[2][0]) for +I; a grid
// value differs from score_at at the same point by nothing but the order of the final sum over the lanes.
// When Kp exceeds the tile, the inner vector g is RECOMPUTED per tile (distal node outer, tile inner: the grid values
// come out in the order the log-sum-exp adds them) and tabP is rebuilt per (distal node, tile); with Kp <= 16 (the
// default rule is 8 x 16) tabP is built once per entry.  Rows of the last tile beyond Kp are zero and their
// accumulators are never read.
//
// LDS: U and UiT static (2 S^2 doubles), the tables dynamic: (2 + TJ) c S doubles -- 2.25 KiB at 4 states x 4
// categories, 11.25 KiB at 20 x 4, 45 KiB (51.25 KiB with the static part) at 20 x EPA_MAX_CATS, inside the 64 KiB of a
// workgroup (TJ <= 21 there).  Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): k_marginal<4> 250 VGPRs,
// 2 waves per SIMD; k_marginal<20> 256 VGPRs + 68 AGPRs (spill space in the register file), 1 wave per SIMD; no scratch
// in either.
//
// Expectation before the first run, from k_score_at's flop count at 4 states: ~100 flops per (site, category) before
// the pendant contraction and 4 FMAs for it, so a distal node with 16 pendant nodes should cost about a tenth of 16
// score evaluations, less what the per-(site, j) frexp / scaling work (not amortised) eats.
// MEASURED on MI355X (profiles/marginal_rate.py, HIP-event medians of 5 warm rounds, 20 000 entries, the default 8 x 16
// rule) against 128 score_at launches over the same entries at the same nodes: cfg2 shape (4 states x 4 categories,
// 150-site reads) 3.33 ms against 43.7 ms = 13.1 x; 20 states x 4 categories (100-site reads) 21.8 ms against 173.6 ms =
// 8.0 x.
#include "epa_dev_internal.hpp"
#include "wave_util.hpp"

#include <algorithm>

namespace {

using namespace epa_wave;

struct MgArgs {
  const ModelDev* m;
  const double* refT;      // [2B][c*s][W]
  const uint32_t* scSum;   // [B][W] proximal + distal scaler counts
  const double* cinv;      // +I: [W] p * pi_inv per site, or null
  double inv_w0;
  const double* blen;
  const epa_pair* pairs;
  const double* x_frac;    // [Kx] distal nodes as fractions of the branch
  const double* x_logw;    // [Kx]
  const double* p_len;     // [Kp] pendant nodes
  const double* p_logw;    // [Kp]
  uint32_t Kx, Kp;
  const uint8_t* codes;
  uint32_t cstride, crel;
  const uint32_t* win_begin;
  const uint32_t* win_span;
  double* marginal;        // [n]
  double* grid;            // [n][Kx][Kp], or null
  double* vbuf;            // [gridDim.x][Kx][Kp]: the v_ij of the entry a wave is working on
  uint64_t n;
  uint32_t W;
};

constexpr double LN2 = 0.6931471805599453094;
constexpr double NOISE_CUT = 0x1p-48;   // score_at.hip
constexpr int TJ = 16;                  // pendant nodes per tile

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int S>
__global__ void __launch_bounds__(64) k_marginal(const MgArgs a) {
  __shared__ __attribute__((aligned(16))) double U[S * S];
  __shared__ __attribute__((aligned(16))) double UiT[S * S];   // [i][x] = U^-1[x][i]
  extern __shared__ __attribute__((aligned(16))) double dyn[];  // tab0 [cs] | tab1 [cs] | tabP [TJ][cs]
  const int lane = threadIdx.x;
  const ModelDev* __restrict__ m = a.m;
  const int c = m->c, cs = c * S;
  double* tab0 = dyn;
  double* tab1 = dyn + cs;
  double* tabP = dyn + 2 * cs;
  for (int i = lane; i < S * S; i += 64) { U[i] = m->U[i]; UiT[(i % S) * S + i / S] = m->Ui[i]; }
  __syncthreads();
  const size_t cW = a.W;
  constexpr int UNROLL_I = S == 4 ? 4 : 1;
  const uint32_t Kx = a.Kx, Kp = a.Kp, T = Kx * Kp;
  const uint32_t ntile = (Kp + TJ - 1) / TJ;
  double* vb = a.vbuf + (size_t)blockIdx.x * T;

  for (uint64_t e = blockIdx.x; e < a.n; e += gridDim.x) {
    const epa_pair pr = a.pairs[e];
    const uint32_t b = pr.branch_id, q = pr.seq_id;
    const uint32_t begin = a.win_begin[q], n = a.win_span[q];
    const uint32_t nch = (n + 63) / 64;
    const double* Xt = a.refT + (size_t)(2 * b) * cs * cW + begin;       // proximal side
    const double* Dt = a.refT + (size_t)(2 * b + 1) * cs * cW + begin;   // distal side
    const uint32_t* scp = a.scSum + (size_t)b * cW + begin;
    const uint8_t* qc = a.codes + (size_t)q * a.cstride + (a.crel ? 0u : begin);
    const double len = a.blen[b];

    for (uint32_t ix = 0; ix < Kx; ++ix) {
      const double td = a.x_frac[ix] * len;
      const double tx = len - td;
      const double xlw = a.x_logw[ix];
      for (uint32_t tile = 0; tile < ntile; ++tile) {
        const uint32_t j0 = tile * TJ;
        const uint32_t nt = Kp - j0 < (uint32_t)TJ ? Kp - j0 : (uint32_t)TJ;
        // wave-uniform tables: exp(lr td), exp(lr tx) per distal node, w_k exp(lr p_j) per pendant tile.  The first
        // barrier keeps these writes behind the reads of the previous node / tile / entry, the second the reads below
        // behind them.
        wave_sync();
        if (tile == 0)
          for (int i = lane; i < cs; i += 64) {
            const int k = i / S, x = i - k * S;
            const double lr = m->lam[x] * m->rate[k];
            tab0[i] = exp(lr * td);
            tab1[i] = exp(lr * tx);
          }
        if (ntile > 1 || ix == 0)
          for (int i = lane; i < TJ * cs; i += 64) {
            const int jj = i / cs, r = i - jj * cs;
            const int k = r / S, x = r - k * S;
            double v = 0.0;
            if ((uint32_t)jj < nt) v = m->w[k] * exp(m->lam[x] * m->rate[k] * a.p_len[j0 + jj]);
            tabP[i] = v;
          }
        wave_sync();

        double mant[TJ];
        int ex[TJ];
#pragma unroll
        for (int jj = 0; jj < TJ; ++jj) { mant[jj] = 1.0; ex[jj] = 0; }
        for (uint32_t ch = 0; ch < nch; ++ch) {
          const uint32_t site = ch * 64 + lane;
          const bool valid = site < n;
          const uint32_t s = valid ? site : 0;
          const double* qv = m->qt + (size_t)qc[s] * S;
          double l0[TJ];
#pragma unroll
          for (int jj = 0; jj < TJ; ++jj) l0[jj] = 0.0;
          bool all_small = true;
          for (int k = 0; k < c; ++k) {
            // inner CLV toward the query: I_i = (U (e_d o D_k))_i (U (e_x o X_k))_i   (k_score_at, operand for operand)
            double av[S], bv[S], acc[S];
#pragma unroll
            for (int x = 0; x < S; ++x) {
              av[x] = Dt[(size_t)(k * S + x) * cW + s] * tab0[k * S + x];
              bv[x] = Xt[(size_t)(k * S + x) * cW + s] * tab1[k * S + x];
              acc[x] = 0.0;
            }
            double mx = 0.0;
#pragma unroll UNROLL_I
            for (int i = 0; i < S; ++i) {
              const double* Ur = U + i * S;
              double p = Ur[0] * av[0], r = Ur[0] * bv[0];
              double pb = fabs(p), rb = fabs(r);
#pragma unroll
              for (int x = 1; x < S; ++x) {
                p = fma(Ur[x], av[x], p);
                r = fma(Ur[x], bv[x], r);
                pb = fma(fabs(Ur[x]), fabs(av[x]), pb);
                rb = fma(fabs(Ur[x]), fabs(bv[x]), rb);
              }
              // the noise cut of k_score_at: an entry below the rounding-error bound of its own sum is zero
              if (fabs(p) <= NOISE_CUT * pb) p = 0.0;
              if (fabs(r) <= NOISE_CUT * rb) r = 0.0;
              const double Ii = p * r;
              mx = fmax(mx, Ii);
              const double* Vr = UiT + i * S;
#pragma unroll
              for (int x = 0; x < S; ++x) acc[x] = fma(Vr[x], Ii, acc[x]);
            }
            all_small = all_small && mx < 0x1p-256;
            // g_x = (U^-1 I)_x q_x once; per pendant node only the contraction against w_k exp(lr p_j)
#pragma unroll
            for (int x = 0; x < S; ++x) acc[x] *= qv[x];
            const double* tp = tabP + k * S;
#pragma unroll
            for (int jj = 0; jj < TJ; ++jj) {
              double l = 0.0;
#pragma unroll
              for (int x = 0; x < S; ++x) l = fma(acc[x], tp[jj * cs + x], l);
              l0[jj] += l;
            }
          }
          uint32_t count = scp[s];
          if (all_small) ++count;   // per-site scaling: all c * s entries below the threshold -> * 2^256, count + 1
          const bool inv = a.cinv != nullptr;
          const double ci = inv ? a.cinv[begin + s] * a.inv_w0 : 0.0;
          const int dex = 256 * (int)count;
#pragma unroll
          for (int jj = 0; jj < TJ; ++jj) {
            double l = l0[jj];
            if (all_small) l *= 0x1p+256;
            if (inv) l = fma(ci, tabP[jj * cs], l);   // +I: p * pi_inv enters L_0 only, unscaled
            int d = dex;
            if (!valid) { l = 1.0; d = 0; }
            mant[jj] *= __builtin_amdgcn_frexp_mant(l);
            ex[jj] += __builtin_amdgcn_frexp_exp(l) - d;
            ex[jj] += __builtin_amdgcn_frexp_exp(mant[jj]);
            mant[jj] = __builtin_amdgcn_frexp_mant(mant[jj]);
          }
        }
#pragma unroll
        for (int jj = 0; jj < TJ; ++jj) {
          if ((uint32_t)jj < nt) {   // wave-uniform
            const double g = wave_sum(log(mant[jj]) + (double)ex[jj] * LN2);
            if (lane == 0) {
              const size_t at = (size_t)ix * Kp + j0 + jj;
              vb[at] = (xlw + a.p_logw[j0 + jj]) + g;
              if (a.grid) a.grid[e * T + at] = g;
            }
          }
        }
      }
    }

    // M = m + log(sum exp(v - m)): m the exact maximum, the sum in the order i ascending, then j ascending
    wave_sync();   // lane 0's stores to vb before every lane's loads
    double vmax = -__builtin_inf();
    for (uint32_t t = lane; t < T; t += 64) vmax = fmax(vmax, vb[t]);
    vmax = wave_max_d(vmax);
    double sum = 0.0;
    for (uint32_t t0 = 0; t0 < T; t0 += 64) {
      const uint32_t t = t0 + lane;
      const double term = t < T ? exp(vb[t] - vmax) : 0.0;
      const uint32_t cnt = T - t0 < 64u ? T - t0 : 64u;
      for (uint32_t l = 0; l < cnt; ++l) sum += readlane_d(term, (int)l);   // wave-uniform, one add per term
    }
    if (lane == 0) a.marginal[e] = vmax + log(sum);
  }
}

}  // namespace

int launch_marginal(epa_ctx* ctx, const EntryStage& e, const double* d_rule, uint32_t Kx, uint32_t Kp, double* d_marginal,
                    double* d_grid) {
  MgArgs a;
  a.m = ctx->dmodel;
  a.refT = ctx->refT;
  a.scSum = ctx->scSum;
  a.cinv = ctx->cinv;
  a.inv_w0 = ctx->inv_w0;
  a.blen = ctx->blen;
  a.pairs = e.d_pairs;
  a.x_frac = d_rule;
  a.x_logw = d_rule + Kx;
  a.p_len = d_rule + 2 * (size_t)Kx;
  a.p_logw = d_rule + 2 * (size_t)Kx + Kp;
  a.Kx = Kx;
  a.Kp = Kp;
  a.codes = e.d_codes;
  a.crel = ctx->code_stride ? 1u : 0u;
  a.cstride = a.crel ? ctx->code_stride : ctx->W;
  a.win_begin = e.d_begin;
  a.win_span = e.d_span;
  a.marginal = d_marginal;
  a.grid = d_grid;
  a.n = e.n;
  a.W = ctx->W;
  // persistent grid: neither n nor a branch id reaches a grid dimension
  const uint32_t grid = (uint32_t)std::min<uint64_t>(e.n, (uint64_t)ctx->n_cu * 8);
  a.vbuf = (double*)epa_scratch(ctx, SLOT_MG_WAVES, sizeof(double) * (size_t)grid * Kx * Kp);
  if (!a.vbuf) return epa_fail(ctx, EPA_ERR_HIP, "hipMalloc(marginal_like grid values)");
  const size_t lds = sizeof(double) * (size_t)(2 + TJ) * ctx->hmodel.c * ctx->s;
  epa_timer_start(ctx, epa_t(ctx, epa_ctx::T_MARGINAL));
  if (ctx->s == 4) hipLaunchKernelGGL((k_marginal<4>), dim3(grid), dim3(64), lds, ctx->stream, a);
  else hipLaunchKernelGGL((k_marginal<20>), dim3(grid), dim3(64), lds, ctx->stream, a);
  epa_timer_stop(ctx, epa_t(ctx, epa_ctx::T_MARGINAL));
  EPA_HIP(ctx, hipGetLastError());
  return EPA_OK;
}
