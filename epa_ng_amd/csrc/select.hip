// Candidate selection on device: which branches of its preplacement row every query hands to the thorough kernels.
//
// k_select (the three selection rules) works on the table in HBM: one wave per query, the row lives in registers
// (k_select_wg / k_select_stream: larger trees; k_select_seg: the dynamic rule from the segment maxima the
// preplacement fast paths leave behind, preplace.hip); a selected (query, branch) is one bit of a [B][Q] bitmap + a
// per-branch counter, the candidate list in Work's branch-major order is one scan over the counters and one pass
// over the bitmap (k_emit_pairs).  Bitmaps over 64 MB: per-query staging rows, an exclusive scan of the counts,
// compaction and a stable radix sort on the branch bits.  The host reads back one block of RB_WORDS words (EpaReadback,
// epa_dev_internal.hpp): candidate total, status words, class histogram, the preplacement's window validation.
#include "epa_dev_internal.hpp"
#include "wave_util.hpp"

#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <cmath>

namespace {

using epa_wave::seg_key;
using epa_wave::seg_val;

// ---------------------------------------------------------------------------------------------
// k_select: dynamic heuristic on device (apply_heuristic -> dynamic_heuristic,
// src/core/heuristics.hpp:40-68; compute_and_set_lwr src/set_manipulators.cpp:43-69;
// until_accumulated_reached :90-114).  One wave per query, the row of B log-likelihoods in
// registers (NR values per lane); the largest remaining LWR is extracted until the running sum
// reaches `threshold` (the crossing element is included; a threshold <= 0 selects none, as the
// reference's top-up to min - 1 = 0 does).  Ties: lowest branch id first (the reference's std::sort
// is unstable; the host rules use the same order).  Selections go to stage[q][0..cap).
// ---------------------------------------------------------------------------------------------

// Stop rule of the per-query extraction loop (descending lnL == descending LWR, ties by branch id):
//   0 dynamic   until the accumulated LWR reaches thr, the crossing element included
//               (until_accumulated_reached, src/set_manipulators.cpp:90-114)
//   1 fixed     the ceil(x * B) best (until_top_percent, :82-88); limit precomputed by the host
//   2 baseball  every branch within 3.0 lnL of the best ("strike box"), plus min(40 - hits, 6)
//               more -- 6 when more than 40 were hit: the reference's unsigned wrap-around
//               (src/core/heuristics.hpp:70-117; quirk D7: clamped at B)
// Where a selected (query, branch) goes.  Bitmap form (the usual one): bit q of row b of a
// [B][ceil(Q / 32)] bitmap plus a per-branch counter -- the candidate list in the reference's Work
// order (branch-major, queries ascending: src/core/Work.hpp:21-113) is then one scan over the B
// counters and one pass over the bitmap (k_emit_pairs), no per-query staging rows, no compaction, no
// device sort.  Staging form (bitmap over 64 MB): key (branch << 32 | query) in stage[q][0..cap).
struct SelOut {
  unsigned long long* stage;
  uint32_t cap;
  uint32_t* bitmap;
  uint32_t* bcount;
  uint32_t wpr;     // bitmap words per branch row
  __device__ __forceinline__ void put(uint32_t q, uint32_t bi, uint32_t taken, uint32_t* status) const {
    if (bitmap) {
      atomicOr(&bitmap[(size_t)bi * wpr + (q >> 5)], 1u << (q & 31u));
      atomicAdd(&bcount[bi], 1u);
    } else if (taken < cap) {
      stage[(size_t)q * cap + taken] = ((unsigned long long)bi << 32) | q;
    } else {
      atomicMax(&status[SEL_OVERFLOW], taken + 1);  // staging row too short: caller retries wider
    }
  }
  __device__ __forceinline__ uint32_t count(uint32_t taken) const { return bitmap ? taken : min(taken, cap); }
};

struct SelRule {
  int mode;
  double thr;
  uint32_t limit;
  double sum = 0.0;
  uint32_t hits = 0;
  bool striking = true;
  const double* e2t = nullptr;   // LDS table of exp_tab (wave_util.hpp), or null: library exp
  __device__ __forceinline__ SelRule(int m, double t, uint32_t l, const double* tab = nullptr) : mode(m), thr(t), limit(l), e2t(tab) {}
  // exp(x), x <= 0; far below the underflow threshold either way once x < -800
  __device__ __forceinline__ double ex(double x) const {
    if (!e2t) return exp(x);
    return x == 0.0 ? 1.0 : epa_wave::exp_tab(fmax(x, -800.0), e2t);   // exp_tab(0) == 1 as well: the branch only saves the work
  }
  __device__ __forceinline__ bool more(uint32_t taken, uint32_t B) const {
    if (mode == 0) return taken < B && sum < thr;
    if (mode == 1) return taken < limit;
    return taken < B && (striking || taken < limit);
  }
  // the next best value: take it?  (wave / workgroup uniform)
  __device__ __forceinline__ bool accept(double best, double mx, double tot, uint32_t taken) {
    if (mode == 0) { sum += ex(best - mx) / tot; return true; }
    if (mode == 1) return true;
    if (striking) {
      if (!(best < mx - 3.0)) { ++hits; return true; }
      striking = false;
      // std::min(max_pitches - hits, max_strikes) in size_t arithmetic (heuristics.hpp:107): with
      // more than 40 hits the difference wraps around and 6 more are added, with exactly 40 none
      limit = hits + (hits > 40u ? 6u : min(40u - hits, 6u));
    }
    return taken < limit;
  }
};

template <int NR>
__global__ void __launch_bounds__(256) k_select(const double* __restrict__ lnl, uint32_t Q, uint32_t B, uint32_t pitch,
                                                double threshold, int mode, uint32_t limit, SelOut so,
                                                uint32_t* __restrict__ counts,
                                                uint32_t* __restrict__ status) {
  const uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (q >= Q) return;
  const double* src = lnl + (size_t)q * pitch;
  double v[NR];
  double mx = -INFINITY;
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const uint32_t i = r * 64 + lane;
    v[r] = i < B ? src[i] : -INFINITY;
    mx = fmax(mx, v[r]);
  }
  // wave reductions on the DPP ladder (no LDS round trips: the extraction loop below was 18
  // ds_bpermute per candidate), results wave-uniform
  mx = epa_wave::wave_max_d(mx);
  // (the table-driven exp_tab instead of the library exp: 0.283 -> 0.296 ms, the kernel is not bound by them)
  SelRule rule(mode, threshold, limit);
  double tot = 0.0;
#pragma unroll
  for (int r = 0; r < NR; ++r) tot += exp(v[r] - mx);  // exp(-inf) == 0 for the padding
  tot = epa_wave::wave_sum(tot);
  uint32_t taken = 0;
  while (rule.more(taken, B)) {
    double lbest = -INFINITY;
    uint32_t lbi = 0xffffffffu;
#pragma unroll
    for (int r = 0; r < NR; ++r)
      if (v[r] > lbest) { lbest = v[r]; lbi = r * 64 + lane; }
    // the largest value, ties by the lowest branch id
    const double best = epa_wave::wave_max_d(lbest);
    const uint32_t bi = epa_wave::wave_min_u((lbest == best && lbest > -INFINITY) ? lbi : 0xffffffffu);
    if (bi == 0xffffffffu) break;
    if (!rule.accept(best, mx, tot, taken)) break;
#pragma unroll
    for (int r = 0; r < NR; ++r)
      if ((uint32_t)(r * 64 + lane) == bi) v[r] = -INFINITY;
    if (lane == 0) so.put(q, bi, taken, status);
    ++taken;
  }
  if (lane == 0) counts[q] = so.count(taken);
}

// The dynamic rule from the per-segment maxima the preplacement left behind (epa_wave::seg_key): wave per query,
// lane = 64-branch segment.  With tot >= 1 (the maximum itself) a candidate has lnL >= mx + log((1 - thr) / B)
// -- everything below sums to less than 1 - thr -- and a term below mx - (log B + 38) is less than 2^-54 / B of
// tot: all B of them together cannot move its double.  So only the segments whose maximum lies inside those
// bands are read: 1.5 of 16 on average at cfg2 (tests/...) -- 0.13 GB instead of the 0.82 GB row
// read per 100k-read chunk.  The candidate segments are held in registers (2 -- the usual case -- or up to NRN);
// more (or a row without published maxima: its query went through another preplacement kernel) are streamed per
// extraction.
// Round 5 (the kernel was bound by its own vector instructions: 820 per query, 82 M per 100k reads = the 147 us it
// took, profiles/r5_pmc_summary.txt): the two band widths come from the host (two library logs per wave), the
// exponentials are exp_tab (16 instructions instead of ~45; exp_tab(0) = 1 exactly and the first candidate -- the
// row maximum -- skips it), rows with at most two candidate segments run a two-register extraction loop, a wave
// walks several queries (grid-stride, the next query's maxima requested ahead), and the span-class histogram of
// the candidate counts (k_class_hist: 1563 atomics on one word, 20 us) is summed per workgroup in LDS.
template <int N>
__device__ __forceinline__ uint32_t seg_extract(const double* __restrict__ src, uint32_t lane, uint32_t B,
                                                unsigned long long mask_x, double mx, double tot, SelRule& rule,
                                                const SelOut& so, uint32_t q, uint32_t* __restrict__ status) {
  double v[N];
  uint32_t base[N];
  unsigned long long mm = mask_x;
#pragma unroll
  for (int r = 0; r < N; ++r) {
    if (mm) {
      const uint32_t s = (uint32_t)__builtin_ctzll(mm);
      mm &= mm - 1;
      base[r] = s * 64;
      const uint32_t i = s * 64 + lane;
      v[r] = i < B ? src[i] : -INFINITY;
    } else {
      base[r] = 0;
      v[r] = -INFINITY;
    }
  }
  uint32_t taken = 0, cand = 0;
  while (rule.more(taken, B)) {
    double lbest = -INFINITY;
    uint32_t lbi = 0xffffffffu;
#pragma unroll
    for (int r = 0; r < N; ++r)   // segments ascend with r: the first maximum has the lowest branch id
      if (v[r] > lbest) { lbest = v[r]; lbi = base[r] + lane; }
    const double best = epa_wave::wave_max_d(lbest);
    const uint32_t bi = epa_wave::wave_min_u((lbest == best && lbest > -INFINITY) ? lbi : 0xffffffffu);
    if (bi == 0xffffffffu) break;
    if (!rule.accept(best, mx, tot, taken)) break;
#pragma unroll
    for (int r = 0; r < N; ++r)
      if (base[r] + lane == bi) v[r] = -INFINITY;
    // candidate k waits in lane k: the atomics of a query leave together, one instruction per kind, after its loop
    // (one pair of them per candidate from lane 0 sat between the next query's loads and their wait)
    if (taken < 64u) { if (lane == taken) cand = bi; }
    else if (lane == 0) so.put(q, bi, taken, status);
    ++taken;
  }
  if (lane < min(taken, 64u)) so.put(q, cand, lane, status);
  return taken;
}

template <int NRN>
__global__ void __launch_bounds__(256) k_select_seg(const double* __restrict__ lnl, const unsigned long long* __restrict__ segmax,
                                                    uint32_t segp, uint32_t Q, uint32_t B, uint32_t pitch, double threshold,
                                                    double band_x, double band_t,
                                                    SelOut so, uint32_t* __restrict__ counts, uint32_t* __restrict__ status,
                                                    const uint32_t* __restrict__ win_span, int states,
                                                    uint32_t* __restrict__ hist) {
  __shared__ double s_e2t[64];
  __shared__ uint32_t s_hist[EPA_N_CLS];
  if (threadIdx.x < 64) s_e2t[threadIdx.x] = exp2((double)threadIdx.x * 0.015625);
  if (threadIdx.x < EPA_N_CLS) s_hist[threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t nseg = (B + 63) >> 6;   // <= 64
  const uint32_t stride = gridDim.x * 4;
  uint32_t q = blockIdx.x * 4 + wv;
  unsigned long long key_next = (q < Q && lane < nseg) ? segmax[(size_t)q * segp + lane] : ~0ull;
  for (; q < Q; q += stride) {
    const unsigned long long key = key_next;
    {
      const uint32_t qn = q + stride;
      key_next = (qn < Q && lane < nseg) ? segmax[(size_t)qn * segp + lane] : ~0ull;
    }
    const double* src = lnl + (size_t)q * pitch;
    auto value = [&](uint32_t s) -> double {   // this lane's element of segment s (-inf past the row)
      const uint32_t i = s * 64 + lane;
      return i < B ? src[i] : -INFINITY;
    };
    double m = -INFINITY;
    if (__ballot(key == 0ull) == 0ull) {
      if (lane < nseg) m = seg_val(key);
    } else {   // no maxima for this row: build them from the row itself
      for (uint32_t s = 0; s < nseg; ++s) {
        const double xm = epa_wave::wave_max_d(value(s));
        if (lane == s) m = xm;
      }
    }
    const double mx = epa_wave::wave_max_d(m);
    const unsigned long long mask_t = __ballot(m >= mx - band_t), mask_x = __ballot(m >= mx - band_x);
    double tot = 0.0;
    for (unsigned long long mm = mask_t; mm; mm &= mm - 1)
      tot += epa_wave::exp_tab(fmax(value((uint32_t)__builtin_ctzll(mm)) - mx, -800.0), s_e2t);
    tot = epa_wave::wave_sum(tot);
    SelRule rule(0, threshold, 0u, s_e2t);
    uint32_t taken = 0;
    const int ncs = __popcll(mask_x);
    if (ncs <= 2) {
      taken = seg_extract<2>(src, lane, B, mask_x, mx, tot, rule, so, q, status);
    } else if (ncs <= NRN) {
      taken = seg_extract<NRN>(src, lane, B, mask_x, mx, tot, rule, so, q, status);
    } else {
      // many candidate segments: every extraction streams them again and takes the next element in
      // (lnL descending, branch ascending) order after the previous one
      double pbest = INFINITY;
      uint32_t pbi = 0, cand = 0;
      while (rule.more(taken, B)) {
        double lbest = -INFINITY;
        uint32_t lbi = 0xffffffffu;
        for (unsigned long long mm = mask_x; mm; mm &= mm - 1) {
          const uint32_t s = (uint32_t)__builtin_ctzll(mm), i = s * 64 + lane;
          const double x = value(s);
          const bool after = x < pbest || (x == pbest && i > pbi);
          if (after && x > lbest) { lbest = x; lbi = i; }
        }
        const double best = epa_wave::wave_max_d(lbest);
        const uint32_t bi = epa_wave::wave_min_u((lbest == best && lbest > -INFINITY) ? lbi : 0xffffffffu);
        if (bi == 0xffffffffu) break;
        if (!rule.accept(best, mx, tot, taken)) break;
        pbest = best;
        pbi = bi;
        if (taken < 64u) { if (lane == taken) cand = bi; }
        else if (lane == 0) so.put(q, bi, taken, status);
        ++taken;
      }
      if (lane < min(taken, 64u)) so.put(q, cand, lane, status);
    }
    if (lane == 0) {
      const uint32_t n = so.count(taken);
      counts[q] = n;
      if (hist && n) atomicAdd(&s_hist[epa_span_class(states, win_span[q])], n);
    }
  }
  __syncthreads();
  if (hist && threadIdx.x < EPA_N_CLS && s_hist[threadIdx.x]) atomicAdd(&hist[threadIdx.x], s_hist[threadIdx.x]);
}

// (the round-4 forms of k_select_seg / k_pack_pairs: profiles/variants/r5_preplace_db_duo_v1.hip; A/Bs in profiles/r5_select_pack_ab*.txt)

// Same selection, workgroup per query (4 waves): the row of up to 256 x NRT branches lives in the
// registers of the whole workgroup (element i in thread i % 256, slot i / 256), so the table is
// read exactly once; wave-level (max, argmax, sum) results are combined across the four waves
// through LDS.  Used for 4096 < B <= 16384.
template <int NRT>
__global__ void __launch_bounds__(256) k_select_wg(const double* __restrict__ lnl, uint32_t Q, uint32_t B, uint32_t pitch,
                                                   double threshold, int mode, uint32_t limit, SelOut so,
                                                   uint32_t* __restrict__ counts,
                                                   uint32_t* __restrict__ status) {
  __shared__ double s_val[2][4];
  __shared__ uint32_t s_idx[2][4];
  const uint32_t q = blockIdx.x;
  const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const double* src = lnl + (size_t)q * pitch;
  double v[NRT];
  double mx = -INFINITY;
#pragma unroll
  for (int r = 0; r < NRT; ++r) {
    const uint32_t i = r * 256 + t;
    v[r] = i < B ? src[i] : -INFINITY;
    mx = fmax(mx, v[r]);
  }
  int ph = 0;
  auto block_max = [&](double x) {
    x = epa_wave::shfl_max(x);
    if (lane == 0) s_val[ph][wv] = x;
    __syncthreads();
    x = fmax(fmax(s_val[ph][0], s_val[ph][1]), fmax(s_val[ph][2], s_val[ph][3]));
    ph ^= 1;
    return x;
  };
  mx = block_max(mx);
  double tot = 0.0;
#pragma unroll
  for (int r = 0; r < NRT; ++r) tot += exp(v[r] - mx);  // exp(-inf) == 0 for the padding
  tot = epa_wave::shfl_add(tot);
  if (lane == 0) s_val[ph][wv] = tot;
  __syncthreads();
  tot = (s_val[ph][0] + s_val[ph][1]) + (s_val[ph][2] + s_val[ph][3]);
  ph ^= 1;
  SelRule rule(mode, threshold, limit);
  uint32_t taken = 0;
  while (rule.more(taken, B)) {
    double best = -INFINITY;
    uint32_t bi = 0xffffffffu;
#pragma unroll
    for (int r = 0; r < NRT; ++r)
      if (v[r] > best) { best = v[r]; bi = r * 256 + t; }
#pragma unroll
    for (int o = 32; o; o >>= 1) {
      const double ob = __shfl_xor(best, o);
      const uint32_t oi = __shfl_xor(bi, o);
      if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if (lane == 0) { s_val[ph][wv] = best; s_idx[ph][wv] = bi; }
    __syncthreads();
    best = s_val[ph][0];
    bi = s_idx[ph][0];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      const double ob = s_val[ph][w];
      const uint32_t oi = s_idx[ph][w];
      if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    ph ^= 1;
    if (bi == 0xffffffffu) break;
    if (!rule.accept(best, mx, tot, taken)) break;
#pragma unroll
    for (int r = 0; r < NRT; ++r)
      if ((uint32_t)(r * 256) + t == bi) v[r] = -INFINITY;
    if (t == 0) so.put(q, bi, taken, status);
    ++taken;
  }
  if (t == 0) counts[q] = so.count(taken);
}

// Same selection for references with more than 16384 branches: the row does not fit the register file, so it is streamed
// from HBM/L2 -- workgroup of 256 per query, a fixed number of passes whatever the rule keeps (its predecessor streamed the row
// once per SELECTED branch and remembered the taken ones in a per-lane mask of 65536 bits: profiles/large_tree_select.md).  Every rule keeps a PREFIX of the row in
// selection order (lnL descending, branch ascending), so the work is: how long is the prefix (n), which key is its
// last (K), how many of the elements equal to K belong to it (r of m, the lowest branch ids) -- then one pass
// writes every element above K and the first r ties.  The order inside a query's staging row is free (the rows are
// compacted query by query and sorted stably on the branch bits; the bitmap has no order at all).
//   pass 1      row maximum;   pass 2   tot = sum exp(v - mx) (dynamic), strike-box hits (baseball)
//   n           fixed: the host's ceil(x B); baseball: hits + the reference's wrapped top-up;
//               dynamic, 0 < thr < 1: pass 3 compacts (seg_key, branch) of the elements within band_x of the maximum
//               (k_select_seg's bound: what lies below cannot be needed to reach thr) into LDS; up to SS_CAP of them
//               are sorted there by a bitonic network and SelRule walks the sorted prefix exactly as the other
//               kernels do -- the list is then written straight from LDS (3 passes in all);
//               dynamic otherwise (more than SS_CAP inside the band, thr >= 1): a radix select over the 64-bit keys,
//               8 passes, whose 256-bin LDS histograms hold the LWR sums beside the counts: the digit where the
//               accumulated LWR (from the top) reaches thr; the ties of the last key are added one by one.
//   K, r, m     fixed / baseball: the same radix select on the counts alone (the n-th key from the top)
//   last pass   elements above K, and the first r of the m ties in branch order (a running count per 256-branch
//               step, only when r < m).
// The LWR sums of the radix select are formed bin by bin (LDS atomics, then a scan), not in selection order: another
// association than SelRule::accept's loop, the same decision wherever rounding cannot flip it.
constexpr uint32_t SS_CAP = 2048;   // LDS list of the dynamic rule: 2048 x (8 + 4) B = 24 KB

template <typename T>
__device__ __forceinline__ T ss_block_scan(T v, T* __restrict__ s_w) {   // inclusive, 256 threads, s_w[4]
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T u = __shfl_up(v, o);
    if ((int)lane >= o) v += u;
  }
  __syncthreads();
  if (lane == 63) s_w[wv] = v;
  __syncthreads();
  T before = 0;
  for (uint32_t w = 0; w < wv; ++w) before += s_w[w];
  return v + before;
}

__global__ void __launch_bounds__(256) k_select_stream(const double* __restrict__ lnl, uint32_t Q, uint32_t B, uint32_t pitch,
                                                       double threshold, double band_x, int mode, uint32_t limit, SelOut so,
                                                       uint32_t* __restrict__ counts, uint32_t* __restrict__ status) {
  __shared__ unsigned long long s_key[SS_CAP];
  __shared__ uint32_t s_br[SS_CAP];
  __shared__ double s_hw[256];     // per digit: LWR sum, then its inclusive scan from the top digit down
  __shared__ uint32_t s_hc[256];   // per digit: count, then its scan
  __shared__ double s_wd[4];
  __shared__ uint32_t s_wu[4];
  __shared__ uint32_t s_cnt, s_first, s_last, s_n;
  const uint32_t q = blockIdx.x;
  if (q >= Q) return;
  const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
  const double* src = lnl + (size_t)q * pitch;
  // ---- pass 1: maximum
  double mx = -INFINITY;
  for (uint32_t i = t; i < B; i += 256) mx = fmax(mx, src[i]);
  mx = epa_wave::shfl_max(mx);
  if (lane == 0) s_wd[wv] = mx;
  if (t == 0) { s_cnt = 0u; s_n = 0xffffffffu; }
  __syncthreads();
  mx = fmax(fmax(s_wd[0], s_wd[1]), fmax(s_wd[2], s_wd[3]));
  __syncthreads();
  // ---- pass 2: total (dynamic) / strike-box hits (baseball)
  double tot = 1.0;
  uint32_t n = 0;
  if (mode == 0) {
    tot = 0.0;
    for (uint32_t i = t; i < B; i += 256) tot += exp(src[i] - mx);
    tot = epa_wave::shfl_add(tot);
    if (lane == 0) s_wd[wv] = tot;
    __syncthreads();
    tot = (s_wd[0] + s_wd[1]) + (s_wd[2] + s_wd[3]);
    __syncthreads();
  } else if (mode == 2) {
    uint32_t hits = 0;
    for (uint32_t i = t; i < B; i += 256) hits += !(src[i] < mx - 3.0) ? 1u : 0u;
#pragma unroll
    for (int o = 32; o; o >>= 1) hits += __shfl_xor(hits, o);
    if (lane == 0) s_wu[wv] = hits;
    __syncthreads();
    hits = s_wu[0] + s_wu[1] + s_wu[2] + s_wu[3];
    __syncthreads();
    // SelRule::accept: std::min(max_pitches - hits, max_strikes) in size_t arithmetic, clamped at B by more()
    n = (uint32_t)min((unsigned long long)B, (unsigned long long)hits + (hits > 40u ? 6u : min(40u - hits, 6u)));
  } else {
    n = min(limit, B);
  }
  const bool weighted = mode == 0;
  bool listed = false;
  if (weighted && threshold > 0.0 && threshold < 1.0) {
    // ---- pass 3 (dynamic): the elements that can be candidates, into LDS
    const double lo = mx - band_x;
    for (uint32_t i = t; i < B; i += 256) {
      const double v = src[i];
      if (v >= lo) {
        const uint32_t slot = atomicAdd(&s_cnt, 1u);
        if (slot < SS_CAP) { s_key[slot] = seg_key(v); s_br[slot] = i; }
      }
    }
    __syncthreads();
    const uint32_t cnt = s_cnt;
    if (cnt <= SS_CAP) {
      uint32_t N = 2;
      while (N < cnt) N <<= 1;
      for (uint32_t i = cnt + t; i < N; i += 256) { s_key[i] = 0ull; s_br[i] = 0xffffffffu; }
      __syncthreads();
      for (uint32_t k = 2; k <= N; k <<= 1)
        for (uint32_t j = k >> 1; j; j >>= 1) {
          for (uint32_t i = t; i < N; i += 256) {
            const uint32_t l = i ^ j;
            if (l > i) {
              const unsigned long long ka = s_key[i], kb = s_key[l];
              const uint32_t ba = s_br[i], bb = s_br[l];
              const bool inorder = ka > kb || (ka == kb && ba < bb);   // key descending, branch ascending
              if (((i & k) == 0u) != inorder) { s_key[i] = kb; s_key[l] = ka; s_br[i] = bb; s_br[l] = ba; }
            }
          }
          __syncthreads();
        }
      if (wv == 0) {   // the rule on the sorted prefix, wave-uniform
        SelRule rule(0, threshold, 0u);
        uint32_t taken = 0;
        while (taken < cnt && rule.more(taken, B)) {
          (void)rule.accept(seg_val(s_key[taken]), mx, tot, taken);
          ++taken;
        }
        // the band holds every candidate by construction; a list that ended first goes to the radix select below
        if (lane == 0 && !(taken == cnt && cnt < B && rule.more(taken, B))) s_n = taken;
      }
      __syncthreads();
      if (s_n != 0xffffffffu) {
        n = s_n;
        listed = true;
        for (uint32_t i = t; i < n; i += 256) so.put(q, s_br[i], i, status);
      }
    }
  }
  if (listed || (weighted && !(threshold > 0.0))) {   // (a threshold <= 0 keeps none)
    if (t == 0) counts[q] = so.count(n);
    return;
  }
  // ---- radix select, top digit first: K = key of the last kept element, r of its m ties are kept
  unsigned long long K = 0ull;
  uint32_t r = 0, m = 0;
  bool all = weighted ? false : n >= B;
  if (weighted || (n > 0 && !all)) {
    unsigned long long prefix = 0ull;
    uint32_t rem = n, cabove = 0;
    double sabove = 0.0;
    for (int p = 7; p >= 0 && !all; --p) {
      const uint32_t shift = 8u * (uint32_t)p;
      s_hc[t] = 0u;
      s_hw[t] = 0.0;
      if (t == 0) { s_first = 256u; s_last = 0u; }
      __syncthreads();
      for (uint32_t i = t; i < B; i += 256) {
        const double v = src[i];
        const unsigned long long k = seg_key(v);
        if (p == 7 || (k >> (shift + 8u)) == prefix) {
          const uint32_t d = (uint32_t)(k >> shift) & 255u;
          atomicAdd(&s_hc[d], 1u);
          if (weighted) atomicAdd(&s_hw[d], exp(v - mx) / tot);
        }
      }
      __syncthreads();
      // thread t owns digit 255 - t: scans run from the top digit down
      const uint32_t c = s_hc[255u - t];
      const double w = s_hw[255u - t];
      const uint32_t ic = ss_block_scan<uint32_t>(c, s_wu);
      const double iw = weighted ? ss_block_scan<double>(w, s_wd) : 0.0;
      __syncthreads();
      s_hc[t] = ic;   // from here on indexed by t, not by digit
      s_hw[t] = iw;
      if (c) {
        if (weighted ? (sabove + iw >= threshold) : (ic >= rem)) atomicMin(&s_first, t);
        atomicMax(&s_last, t);
      }
      __syncthreads();
      uint32_t ts = s_first;
      if (ts == 256u) {
        // the whole row stays below thr (thr >= 1 and the like): everything is kept.  Further down only another
        // rounding of the same sum can end here: the lowest digit present
        if (p == 7) { all = true; n = B; break; }
        ts = s_last;
      }
      const uint32_t ec = ts ? s_hc[ts - 1u] : 0u;
      const double ew = ts ? s_hw[ts - 1u] : 0.0;
      m = s_hc[ts] - ec;
      cabove += ec;
      rem -= weighted ? 0u : ec;
      sabove += ew;
      prefix = (prefix << 8) | (unsigned long long)(255u - ts);
      __syncthreads();
    }
    if (!all) {
      K = prefix;
      if (weighted) {
        const double w = exp(seg_val(K) - mx) / tot;
        double sum = sabove;
        while (r < m && sum < threshold) { sum += w; ++r; }
        n = cabove + r;
      } else {
        r = rem;
      }
    }
  }
  // ---- last pass: everything above K, the first r ties in branch order
  if (n > 0) {
    const bool ordered = !all && r < m;
    uint32_t tie_base = 0;
    if (t == 0) s_cnt = 0u;   // now the staging rows' slot counter
    __syncthreads();
    for (uint32_t base = 0; base < B; base += 256) {
      const uint32_t i = base + t;
      const unsigned long long k = i < B ? seg_key(src[i]) : 0ull;
      bool sel = i < B && (all || k > K);
      bool eq = i < B && !all && k == K;
      if (ordered) {
        const unsigned long long bal = __ballot(eq);
        if (lane == 0) s_wu[wv] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t before = tie_base + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
        for (uint32_t w = 0; w < wv; ++w) before += s_wu[w];
        tie_base += s_wu[0] + s_wu[1] + s_wu[2] + s_wu[3];
        eq = eq && before < r;
        __syncthreads();
      }
      sel = sel || eq;
      uint32_t slot = 0;
      if (!so.bitmap) {   // staging form: one slot per kept element, handed out per wave
        const unsigned long long bal = __ballot(sel);
        uint32_t wbase = 0;
        if (lane == 0 && bal) wbase = atomicAdd(&s_cnt, (uint32_t)__popcll(bal));
        wbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)wbase);
        slot = wbase + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
      }
      if (sel) so.put(q, i, slot, status);
    }
  }
  if (t == 0) counts[q] = so.count(n);
}

// span-class histogram of the selected pairs: sum of the per-query candidate counts by the class
// of the query's window (one atomic per wave and class present)
__global__ void __launch_bounds__(256) k_class_hist(const uint32_t* __restrict__ counts,
                                                   const uint32_t* __restrict__ win_span, uint32_t Q,
                                                   int states, uint32_t* __restrict__ hist) {
  const uint32_t q = blockIdx.x * 256 + threadIdx.x;
  const int cls = q < Q ? epa_span_class(states, win_span[q]) : -1;
  const uint32_t n = q < Q ? counts[q] : 0;
  for (int c = 0; c < EPA_N_CLS; ++c) {
    if (__ballot(cls == c) == 0ull) continue;
    uint32_t v = cls == c ? n : 0;
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(&hist[c], v);
  }
}

// everything the host reads after the selection, in one block (EpaReadback): the total, the selection's status words +
// class histogram (status: the EpaSelStatus block), the preplacement's window validation.
// tip_total (or null): the candidate pairs whose branch has a tip on the distal side.  When all pairs are of ONE span
// class that has a tip-distal half (epa_tip_class_ok), the class's count is split: out[RB_HIST + c] keeps the others,
// out[RB_HIST + epa_tip_class(c)] takes the tip pairs, out[RB_TIP_SPLIT] = 1 says that the split was made
// (SelectPending::tip_split).  With several span classes present the per-branch counters cannot tell the classes
// apart: no split, out[RB_TIP_SPLIT] = 0
__global__ void __launch_bounds__(64) k_pack_readback(const uint32_t* __restrict__ status,
                                                     const uint32_t* __restrict__ total,
                                                     const uint32_t* __restrict__ pre_status,
                                                     uint32_t* __restrict__ out,
                                                     const uint32_t* __restrict__ tip_total = nullptr) {
  const uint32_t t = threadIdx.x;
  if (t == 0) out[RB_TOTAL] = *total;
  if (t < SEL_HIST + EPA_N_CLS) out[RB_STATUS + t] = status[t];   // status words and histogram: RB_HIST - RB_STATUS == SEL_HIST
  else if (t < SEL_HIST + EPA_N_CLSX) out[RB_STATUS + t] = 0u;
  if (t == RB_TIP_SPLIT) out[RB_TIP_SPLIT] = 0u;
  if (t < RB_WORDS - RB_WINDOW) out[RB_WINDOW + t] = pre_status ? pre_status[t] : 0u;
  __syncthreads();   // the split below rewrites words other threads have just copied
  if (tip_total && t == 0) {
    int one = -1, n = 0;
    for (int c = 0; c < EPA_N_CLS; ++c)
      if (status[SEL_HIST + c]) { one = c; ++n; }
    if (n == 1 && epa_tip_class_ok(one)) {
      const uint32_t all = status[SEL_HIST + one], tips = min(*tip_total, all);
      out[RB_HIST + one] = all - tips;
      out[RB_HIST + epa_tip_class(one)] = tips;
      out[RB_TIP_SPLIT] = 1u;
    }
  }
}

__global__ void __launch_bounds__(256) k_compact(const unsigned long long* __restrict__ stage,
                                                 const uint32_t* __restrict__ counts,
                                                 const uint32_t* __restrict__ offsets, uint32_t Q,
                                                 uint32_t cap, unsigned long long* __restrict__ keys) {
  const uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (q >= Q) return;
  const uint32_t n = counts[q], o = offsets[q];
  for (uint32_t i = lane; i < n; i += 64) keys[o + i] = stage[(size_t)q * cap + i];
}

// Bitmap form of the selection: workgroup b walks row b of the bitmap in chunks of 256 words and
// writes the set bits -- queries ascending -- as pairs behind boffs[b] (exclusive scan of the per-
// branch counters): the candidate list in (branch, query) order.
__global__ void __launch_bounds__(256) k_emit_pairs(const uint32_t* __restrict__ bitmap, uint32_t wpr,
                                                    const uint32_t* __restrict__ boffs,
                                                    epa_pair* __restrict__ pairs, uint32_t nb, uint32_t max_pairs) {
  __shared__ uint32_t wsum[4];
  const uint32_t b = blockIdx.x, t = threadIdx.x, lane = t & 63u, wv = t >> 6;
  if (boffs[nb] > max_pairs) return;   // queued ahead of the host's overflow check (launch_select_emit): the list would not fit
  uint32_t base = boffs[b];
  const uint32_t end = boffs[b + 1];
  if (base == end) return;
  const uint32_t* row = bitmap + (size_t)b * wpr;
  for (uint32_t w0 = 0; w0 < wpr && base < end; w0 += 256) {
    const uint32_t wi = w0 + t;
    uint32_t bits = wi < wpr ? row[wi] : 0u;
    const uint32_t c = (uint32_t)__popc(bits);
    uint32_t inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t u = __shfl_up(inc, o);
      if ((int)lane >= o) inc += u;
    }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) {
      if (w < wv) before += wsum[w];
      total += wsum[w];
    }
    uint32_t o = base + before + inc - c;
    while (bits) {
      const uint32_t k = (uint32_t)__ffs((int)bits) - 1u;
      bits &= bits - 1u;
      pairs[o].branch_id = b;
      pairs[o].seq_id = wi * 32u + k;
      ++o;
    }
    base += total;
    __syncthreads();
  }
}

__global__ void k_keys_to_pairs(const unsigned long long* __restrict__ keys, uint64_t n,
                                epa_pair* __restrict__ pairs) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    pairs[i].branch_id = (uint32_t)(keys[i] >> 32);
    pairs[i].seq_id = (uint32_t)(keys[i] & 0xffffffffu);
  }
}

// bitmap form: the pair list in (branch, query) order behind the scanned counters
void emit_pairs(epa_ctx* ctx, const SelectPending* sp) {
  hipLaunchKernelGGL(k_emit_pairs, dim3(ctx->B), dim3(256), 0, ctx->stream, sp->bitmap, sp->wpr, sp->boffs, sp->d_pairs, ctx->B,
                     (uint32_t)std::min<uint64_t>(sp->max_pairs, 0xffffffffu));
}

}  // namespace

// The candidate selection in two halves, so that a caller with something else to queue (the chunk
// pipeline: the other slot's work) does not sit in the wait for the candidate count:
//   begin  queues k_select, the offsets scan, the span-class histogram and the read-back of
//          {total, status words, class histogram, window-validation words of the preplacement} into
//          `rb` (pinned host memory for a truly asynchronous copy; 64 words) -- no synchronisation;
//   end    waits for the stream, widens the staging rows and repeats on overflow (rare), then queues
//          compaction, the stable sort into Work order and the key -> pair conversion.
// the bitmap form (SelOut) unless the bitmap is over 64 MB, or the option select_sort asks for the staging form
static bool select_bitmap_form(const epa_ctx* ctx, uint32_t Q) {
  return !ctx->opt.select_sort && (size_t)ctx->B * ((Q + 31) / 32) * sizeof(uint32_t) <= ((size_t)64 << 20);
}

bool epa_select_takes_seg(const epa_ctx* ctx, const PreTable& t, uint32_t Q, double threshold) {
  // (A/B and test switch select_full_rows: the full-row kernels)
  return select_bitmap_form(ctx, Q) && t.segmax && !ctx->opt.select_full_rows && ctx->heur_mode == 0 && threshold < 1.0 &&
         (ctx->B + 63) / 64 <= 64;
}

int launch_select_begin(epa_ctx* ctx, const PreTable& t, const uint32_t* pre_status, uint32_t Q, double threshold,
                        epa_pair* d_pairs, uint64_t max_pairs, const uint32_t* d_span, uint32_t* rb, SelectPending* sp) {
  sp->have_hist = false;
  const uint32_t B = ctx->B;
  const double* const d_lnl = t.lnl;
  const uint32_t pitch = t.pitch;
  // selection rule of the context (epa_dev_set_heuristic); fixed: ceil(x * B) best, at least... none:
  // until_top_percent keeps ceil(x * B) elements, 0 for x == 0 (src/set_manipulators.cpp:82-88)
  const int mode = ctx->heur_mode;
  uint32_t limit = 0;
  if (mode == 1) {
    limit = (uint32_t)std::min<double>((double)B, std::ceil(ctx->heur_param * (double)B));
    ctx->select_cap = std::max(ctx->select_cap, std::max(limit, 1u));
  } else if (mode == 2) {
    ctx->select_cap = std::max(ctx->select_cap, std::min(B, 48u));
  }
  const uint32_t cap = ctx->select_cap;
  size_t scan_bytes = 0, sort_bytes = 0;
  (void)rocprim::exclusive_scan(nullptr, scan_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, Q,
                                rocprim::plus<uint32_t>(), ctx->stream);
  const size_t worst = std::min<uint64_t>(max_pairs, (uint64_t)Q * cap);
  (void)rocprim::radix_sort_keys<epa_radix_cfg>(nullptr, sort_bytes, (unsigned long long*)nullptr,
                                 (unsigned long long*)nullptr, worst, 0, 64, ctx->stream);
  const uint32_t wpr = (Q + 31) / 32;
  const bool bm = select_bitmap_form(ctx, Q);
  uint32_t* status = nullptr;
  size_t fill = 0;
  auto layout = [&](Carver c) {   // SLOT_SELECT, either form behind the status block
    status = c.take<uint32_t>(SEL_WORDS);
    if (bm) {
      sp->boffs = c.take<uint32_t>((size_t)B + 1);   // per-branch counters, scanned in place: [B] = the total
      sp->bitmap = c.take<uint32_t>((size_t)B * wpr);
      fill = c.off;                                  // status, counters, bitmap: one fill
      sp->counts = c.take<uint32_t>(Q + 1);
    } else {
      sp->counts = c.take<uint32_t>(Q + 1);
      sp->offsets = c.take<uint32_t>(Q + 1);
      sp->stage = c.take<unsigned long long>((size_t)Q * cap);
      sp->keys_a = c.take<unsigned long long>(worst);
      sp->keys_b = c.take<unsigned long long>(worst);
      sp->temp = c.tail(std::max(scan_bytes, sort_bytes));
    }
    return c.off;
  };
  char* base = (char*)epa_scratch(ctx, SLOT_SELECT, layout(Carver{}));
  if (!base) return epa_fail(ctx, EPA_ERR_HIP, "hipMalloc(select scratch)");
  sp->bitmap = nullptr; sp->offsets = nullptr;   // (the form not taken)
  layout(Carver{base});
  uint32_t* const counts = sp->counts;
  sp->wpr = wpr; sp->sort_bytes = sort_bytes;
  sp->table = t; sp->pre_status = pre_status; sp->Q = Q; sp->threshold = threshold; sp->d_pairs = d_pairs; sp->max_pairs = max_pairs;
  sp->d_span = d_span; sp->cap = cap; sp->rb = rb;
  sp->ev_rb = nullptr; sp->d_rb = nullptr; sp->emitted = false; sp->queued_cls = -1;
  if (bm) {
    const int zr = epa_zero_async(ctx, base, fill);
    if (zr) return zr;
  } else {   // status words and the trailing count: counts[Q] sits in the same allocation
    EPA_HIP(ctx, hipMemsetAsync(status, 0, sizeof(uint32_t) * SEL_WORDS, ctx->stream));
    EPA_HIP(ctx, hipMemsetAsync(counts + Q, 0, sizeof(uint32_t), ctx->stream));
  }
  epa_timer_start(ctx, epa_t(ctx, epa_ctx::T_SELECT));
  // The selection kernel for this tree and rule, writing through `so`; true: it summed the span-class histogram itself
  auto select_rows = [&](const SelOut& so) -> bool {
    const int nr = (int)((B + 63) / 64);
    if (so.bitmap && epa_select_takes_seg(ctx, t, Q, threshold)) {
      // band widths of the segment test (see k_select_seg): conservative margins, so the host's log is as good as the device's
      const double band_x = epa_select_band_x(threshold, B), band_t = epa_select_band_t(threshold, B);
      constexpr uint32_t sel_grid = 16;   // workgroups per CU of the persistent selection grid
      const dim3 grid_seg(std::min<uint32_t>((Q + 3) / 4, (uint32_t)ctx->n_cu * sel_grid));
      hipLaunchKernelGGL(k_select_seg<8>, grid_seg, dim3(256), 0, ctx->stream, d_lnl, t.segmax, t.segp, Q, B, pitch, threshold,
                         band_x, band_t, so, counts, status, d_span, ctx->s, d_span ? status + SEL_HIST : nullptr);
      return d_span != nullptr;
    }
    auto rows = [&](auto kernel, dim3 grid) {
      hipLaunchKernelGGL(kernel, grid, dim3(256), 0, ctx->stream, d_lnl, Q, B, pitch, threshold, mode, limit, so, counts, status);
    };
    const dim3 waves((Q + 3) / 4);   // a wave per query; k_select_wg / _stream: a workgroup
    if (nr <= 2) rows(k_select<2>, waves); else if (nr <= 4) rows(k_select<4>, waves); else if (nr <= 8) rows(k_select<8>, waves);
    else if (nr <= 16) rows(k_select<16>, waves); else if (nr <= 32) rows(k_select<32>, waves); else if (nr <= 64) rows(k_select<64>, waves);
    else if (nr <= 128) rows(k_select_wg<32>, dim3(Q)); else if (nr <= 256) rows(k_select_wg<64>, dim3(Q));
    else {
      // k_select_stream (B > 16384): how far below the row maximum a candidate of the dynamic rule can lie (k_select_seg's bound)
      const double stream_band = (mode == 0 && threshold > 0.0 && threshold < 1.0) ? 1.0 - std::log((1.0 - threshold) / (double)B) : 0.0;
      hipLaunchKernelGGL(k_select_stream, dim3(Q), dim3(256), 0, ctx->stream, d_lnl, Q, B, pitch, threshold, stream_band, mode, limit, so, counts, status);
    }
    return false;
  };
  const bool seg_hist = select_rows(bm ? SelOut{nullptr, 0u, sp->bitmap, sp->boffs, wpr} : SelOut{sp->stage, cap, nullptr, nullptr, 0u});
  // the candidate total behind the scan of the counts.  Bitmap form, SEL_TIP_TOTAL: the candidate pairs on branches that
  // end in a tip (summed with the scan; split off by k_pack_readback)
  uint32_t* const tip_total = (bm && epa_tipd_active(ctx) && d_span) ? status + SEL_TIP_TOTAL : nullptr;
  const uint32_t* total;
  if (bm) {
    launch_scan_counts(ctx, sp->boffs, B + 1, tip_total ? ctx->tip_row : nullptr, tip_total);
    total = sp->boffs + B;
  } else {
    EPA_HIP(ctx, rocprim::exclusive_scan(sp->temp, scan_bytes, counts, sp->offsets, 0u, Q + 1, rocprim::plus<uint32_t>(), ctx->stream));
    total = sp->offsets + Q;
  }
  if (d_span && !seg_hist)  // class histogram in the status block: read back with the total, no extra round trip
    hipLaunchKernelGGL(k_class_hist, dim3((Q + 255) / 256), dim3(256), 0, ctx->stream, counts, d_span, Q, ctx->s, status + SEL_HIST);
  // packed on the device so that ONE small copy brings everything the host waits for (EpaReadback)
  hipLaunchKernelGGL(k_pack_readback, dim3(1), dim3(64), 0, ctx->stream, status, total, sp->pre_status, status + SEL_READBACK,
                     (const uint32_t*)tip_total);
  EPA_HIP(ctx, hipMemcpyAsync(rb, status + SEL_READBACK, sizeof(uint32_t) * RB_WORDS, hipMemcpyDeviceToHost, ctx->stream));
  sp->have_status = sp->pre_status != nullptr;
  if (bm) {   // launch_select_end waits for the copy alone: what a caller queues behind it runs on
    if (!ctx->ev_rb[ctx->bank]) EPA_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_rb[ctx->bank], hipEventDisableTiming));
    EPA_HIP(ctx, hipEventRecord(ctx->ev_rb[ctx->bank], ctx->stream));
    sp->ev_rb = ctx->ev_rb[ctx->bank];
    sp->d_rb = status + SEL_READBACK;
  }
  return EPA_OK;
}

// Bitmap form: the pair list written behind the read-back without waiting for the host (the kernel itself refuses a
// list that would not fit); the selection's timer stops here.
int launch_select_emit(epa_ctx* ctx, SelectPending* sp) {
  if (!sp->bitmap || !sp->d_rb || sp->emitted) return EPA_OK;
  emit_pairs(ctx, sp);
  epa_timer_stop(ctx, epa_t(ctx, epa_ctx::T_SELECT));
  EPA_HIP(ctx, hipGetLastError());
  sp->emitted = true;
  return EPA_OK;
}

int launch_select_end(epa_ctx* ctx, SelectPending* sp, uint64_t* n_pairs) {
  const uint32_t B = ctx->B, Q = sp->Q;
  for (;;) {
    // everything up to the read-back copy; kernels queued behind it (launch_select_emit, launch_thorough_queued) run on
    if (sp->ev_rb) EPA_HIP(ctx, hipEventSynchronize(sp->ev_rb));
    else EPA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const uint32_t total = sp->rb[RB_TOTAL];
    const uint32_t overflow = sp->rb[RB_STATUS + SEL_OVERFLOW];
    if (overflow && !sp->bitmap) {  // some query selected more candidates than the staging row holds: widen, redo
      if (sp->cap >= B) return epa_fail(ctx, EPA_ERR_HIP, "select_candidates: staging overflow");
      ctx->select_cap = std::min<uint32_t>(B, std::max(sp->cap * 4, overflow));
      int rc = launch_select_begin(ctx, sp->table, sp->pre_status, Q, sp->threshold, sp->d_pairs, sp->max_pairs, sp->d_span, sp->rb, sp);
      if (rc) return rc;
      continue;
    }
    if (total > sp->max_pairs)
      return epa_fail(ctx, EPA_ERR_PAIR_OVERFLOW,
                      "select_candidates: " + std::to_string(total) + " candidates exceed max_pairs");
    if (total && sp->bitmap) {
      if (!sp->emitted) emit_pairs(ctx, sp);
    } else if (total) {
      const dim3 grid((Q + 3) / 4);
      hipLaunchKernelGGL(k_compact, grid, dim3(256), 0, ctx->stream, sp->stage, sp->counts, sp->offsets, Q, sp->cap,
                         sp->keys_a);
      // branch-major order == Work iteration order (std::map<branch, vector<seq>>).  The compacted
      // list is already ascending in the query id (and a query names a branch at most once), so a
      // STABLE sort on the branch bits alone gives (branch, query) order: 2 digit passes, not 6.
      int bits = 33;
      while ((1ull << (bits - 32)) <= B && bits < 64) ++bits;
      size_t sort_bytes = sp->sort_bytes;
      EPA_HIP(ctx, rocprim::radix_sort_keys<epa_radix_cfg>(sp->temp, sort_bytes, sp->keys_a, sp->keys_b, (size_t)total,
                                                           32, bits, ctx->stream));
      hipLaunchKernelGGL(k_keys_to_pairs, dim3((total + 255) / 256), dim3(256), 0, ctx->stream, sp->keys_b,
                         (uint64_t)total, sp->d_pairs);
    }
    if (!sp->emitted) epa_timer_stop(ctx, epa_t(ctx, epa_ctx::T_SELECT));   // (else stopped behind the queued k_emit_pairs)
    EPA_HIP(ctx, hipGetLastError());
    *n_pairs = total;
    if (sp->d_span) {   // the selected pairs' span classes, for the Newton launch of this chunk body only
      for (int c = 0; c < EPA_N_CLSX; ++c) sp->cls_hist[c] = sp->rb[RB_HIST + c];
      sp->have_hist = true;
      sp->tip_split = sp->rb[RB_TIP_SPLIT] != 0;
    }
    return EPA_OK;
  }
}

// what the preplacement's window validation found (read back by launch_select_begin into rb[RB_WINDOW ..])
int select_check_status(epa_ctx* ctx, const SelectPending* sp) {
  return sp->have_status ? preplace_window_error(ctx, sp->rb + RB_WINDOW) : EPA_OK;
}

int launch_select(epa_ctx* ctx, const PreTable& t, const uint32_t* pre_status, uint32_t Q, double threshold,
                  epa_pair* d_pairs, uint64_t max_pairs, uint64_t* n_pairs, const uint32_t* d_span) {
  uint32_t rb[64] = {};
  SelectPending sp;
  int rc = launch_select_begin(ctx, t, pre_status, Q, threshold, d_pairs, max_pairs, d_span, rb, &sp);
  if (rc) return rc;
  return launch_select_end(ctx, &sp, n_pairs);
}

