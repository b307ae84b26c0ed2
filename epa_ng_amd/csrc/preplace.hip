// Hot loop 1 on device: preplacement gather-sum (this file) + candidate selection (select.hip), no host in the loop.
//
// k_preplace replaces Lookup_Store::sum_precomputed_sitelk inside place()
// (src/core/Lookup_Store.hpp:110-141, src/core/place.cpp:65-91):
//     lnl[q][b] = sum_{site in window(q)} T[b][site][code(q, site)]
// with the reference's association order ((a0+a1)+(a2+a3) per group of 4, then singles).
//
// Pipeline (all on the stream; the host reads back one 36-word block: candidate total + status):
//   1. queries are sorted by window start -- the fast paths by a counting sort over (class, start
//      parity, start) (k_count_keys / k_scan_counts / k_scatter_sorted), the generic path by a device
//      radix sort -- and k_make_groups cuts the sorted list into groups whose starts fall into one
//      SPREAD-site bucket (<= 1024 queries on the fast paths, <= 256 on the generic one);
//   2. k_preplace (generic): workgroup = one query group x one tile of NB branches.  Per (branch,
//      160-site chunk) the slice of T the whole group can touch is staged through LDS once
//      (coalesced 16 B/lane loads), then every thread gathers its own query's values with
//      ds_read_b64.  Query codes sit in registers as packed byte offsets, partial sums in LDS.  For
//      the 16-column DNA table the LDS columns are XOR-swizzled by the row ((row >> 1) & 15).
//   2b. DNA fast path (k_preplace_pairs): queries whose windows hold only A/C/G/T/N-or-gap use a
//      second table T2[b][s][36] = T[b][s][c0] + T[b][s+1][c1] over {A,C,G,T,N,none}^2: one
//      ds_read_b64 per TWO sites, and the value is exactly the (a0 + a1) the reference forms
//      first, so the association order ((a0+a1)+(a2+a3)) and the results stay bit-identical to
//      the generic path.  Queries are additionally split by window-start parity (a group stages
//      only the pair rows of its own parity) and their per-pair LDS offsets are precomputed once
//      per chunk of queries (k_pack_pairs); queries with other ambiguity codes take the generic
//      kernel.  Persistent grid, XCD-contiguous walk of the (tile, group) items (item_walk),
//      branches per item chosen per launch (choose_tile), pair rows in LDS-bank order
//      (pair_entry, ROWL_NARROW), results written as whole 64-byte sectors.
//   2c. 20-state fast path (k_preplace_sites): the same machinery over the ordinary [W][24] table.
//   3. the candidate selection works on the table in HBM, and for the dynamic rule on the segment maxima the fast
//      paths leave behind (SegTrack): select.hip.
#include "epa_dev_internal.hpp"
#include "wave_util.hpp"

#include <cmath>
#include <cstdlib>
#include <cstring>

#include <algorithm>

namespace {

constexpr int GQ = 256;      // queries (threads) per group
constexpr int CH = 160;      // sites per chunk (multiple of 4)
constexpr int SPREAD = 96;   // window starts of a group lie in one bucket of SPREAD sites
constexpr int TROWS = CH + SPREAD;  // rows of T staged per (branch, chunk)
constexpr int NB = 16;       // branches per workgroup
constexpr int CW = CH / 4;   // packed code words per chunk

struct Group {
  uint32_t start;      // first index into the sorted order
  uint32_t count;      // 0 = unused slot of the over-provisioned group table
  uint32_t min_begin;  // 0; groups of the exact pass's cells (k_screen_band): their 64-branch segment
  uint32_t cls;        // 0 = site-pair fast path (or the only class), 1 = generic kernel
};

// window validation (error words read back by preplace_check_status)
__device__ __forceinline__ void validate_window(uint32_t i, uint32_t begin, uint32_t span, uint32_t W,
                                                uint32_t cmax, uint32_t* status) {
  if (span == 0) atomicMax(&status[0], 0x80000000u | i);                          // all-gap query
  else if ((uint64_t)begin + span > W || span > cmax) atomicMax(&status[1], 0x80000000u | i);  // width
}
__global__ void k_validate(const uint32_t* __restrict__ win_begin, const uint32_t* __restrict__ win_span,
                           uint32_t Q, uint32_t W, uint32_t cmax, uint32_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < Q) validate_window(i, win_begin[i], win_span[i], W, cmax, status);
}

__global__ void k_iota(uint32_t* v, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v[i] = i;
}

// Counting sort of the queries by their grouping key (the fast paths; K = key space, a few thousand
// values): a kernel counts every key and keeps each query's arrival rank, one workgroup turns
// the counts into offsets, a scatter writes (sorted_keys, perm).  Three short kernels instead of the
// ten launches of a two-pass device radix sort with its histogram fills (~75 us per chunk, the same for
// 5 000 reads as for 100 000).  The order of equal keys is arrival order: which lane of a group a
// query lands on varies from run to run, its sums do not.
// one thread per query: its key's count, the old value = the query's rank among equal keys (in the
// pack kernels, one returning atomic per WAVE, the same 100k atomics cost 50 us instead of 5)
__global__ void __launch_bounds__(256) k_count_keys(const uint32_t* __restrict__ keys, uint32_t Q,
                                                    uint32_t* __restrict__ cnt, uint32_t* __restrict__ rank) {
  const uint32_t q = blockIdx.x * 256 + threadIdx.x;
  if (q < Q) rank[q] = atomicAdd(&cnt[keys[q]], 1u);
}
// tip_row (or null): *tip_total = the sum of the counts of the first K - 1 entries k with tip_row[k] != 0xffffffff (the
// selection's per-branch counters: the candidate pairs whose branch has a tip on the distal side)
__global__ void __launch_bounds__(1024) k_scan_counts(uint32_t* __restrict__ cnt, uint32_t K,
                                                      const uint32_t* __restrict__ tip_row = nullptr,
                                                      uint32_t* __restrict__ tip_total = nullptr) {
  __shared__ uint32_t wsum[16];
  __shared__ uint32_t carry_s;
  __shared__ uint32_t tips_s;
  const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
  if (t == 0) { carry_s = 0; tips_s = 0; }
  __syncthreads();
  constexpr uint32_t PER = 8;
  uint32_t tips = 0;
  for (uint32_t base = 0; base < K; base += 1024 * PER) {
    uint32_t v[PER], tot = 0;
#pragma unroll
    for (uint32_t i = 0; i < PER; ++i) {
      const uint32_t k = base + t * PER + i;
      v[i] = k < K ? cnt[k] : 0u;
      tot += v[i];
      if (tip_row && k + 1 < K && tip_row[k] != 0xffffffffu) tips += v[i];
    }
    uint32_t inc = tot;                       // inclusive scan of the thread totals inside the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t u = __shfl_up(inc, o);
      if ((int)lane >= o) inc += u;
    }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    uint32_t before = carry_s;
    for (uint32_t w = 0; w < wv; ++w) before += wsum[w];
    uint32_t run = before + inc - tot;
#pragma unroll
    for (uint32_t i = 0; i < PER; ++i) {
      const uint32_t k = base + t * PER + i;
      if (k < K) cnt[k] = run;
      run += v[i];
    }
    __syncthreads();
    if (t == 1023) carry_s = run;
    __syncthreads();
  }
  if (tip_total) {
    if (tips) atomicAdd(&tips_s, tips);
    __syncthreads();
    if (t == 0) *tip_total = tips_s;
  }
}
__global__ void __launch_bounds__(256) k_scatter_sorted(const uint32_t* __restrict__ keys,
                                                        const uint32_t* __restrict__ rank,
                                                        const uint32_t* __restrict__ offs, uint32_t Q,
                                                        uint32_t* __restrict__ sorted_keys,
                                                        uint32_t* __restrict__ perm) {
  const uint32_t q = blockIdx.x * 256 + threadIdx.x;
  if (q >= Q) return;
  const uint32_t k = keys[q], pos = offs[k] + rank[q];
  sorted_keys[pos] = k;
  perm[pos] = q;
}

// One workgroup.  sorted_keys ascending (window start, or class / parity / start composed by
// k_pack_pairs: block = key / Wp, blocks >= class_blocks are class 1).  Every block is cut into
// runs of gq0 (class 0) / gq1 (class 1) consecutive queries; a run whose window starts spread over
// SPREAD sites or more (sparse data) is subdivided along the fixed SPREAD grid, so every group
// fits the staged slice.  n_dev (or null): the number of sorted entries when only the device knows it (at most Q);
// seg_div (or 0): a group's min_begin = its first key / seg_div (the exact pass's cells: the segment, see k_screen_band).
__global__ void __launch_bounds__(256) k_make_groups(const uint32_t* __restrict__ sorted_keys, uint32_t Q,
                                                     uint32_t Wp, uint32_t n_blocks,
                                                     uint32_t class_blocks, uint32_t gq0, uint32_t gq1,
                                                     uint32_t spr0, uint32_t max_runs, Group* __restrict__ groups,
                                                     uint32_t max_groups, uint32_t* __restrict__ status,
                                                     const uint32_t* __restrict__ n_dev = nullptr, uint32_t seg_div = 0) {
  extern __shared__ uint32_t sh[];
  if (n_dev) Q = min(Q, *n_dev);
  uint32_t* lo = sh;                       // [n_blocks + 1] first sorted index of each block
  uint32_t* runbase = lo + n_blocks + 1;   // [n_blocks + 1] first run of each block
  uint32_t* run_start = runbase + n_blocks + 1;  // [max_runs]
  uint32_t* run_end = run_start + max_runs;
  uint32_t* run_off = run_end + max_runs;        // first group slot of the run
  auto lower_bound = [&](uint32_t a, uint32_t b, uint64_t key) {
    while (a < b) {
      const uint32_t m = (a + b) >> 1;
      if ((uint64_t)sorted_keys[m] < key) a = m + 1; else b = m;
    }
    return a;
  };
  for (uint32_t k = threadIdx.x; k <= n_blocks; k += blockDim.x)
    lo[k] = k == n_blocks ? Q : lower_bound(0, Q, (uint64_t)k * Wp);
  for (uint32_t i = threadIdx.x; i < max_groups; i += blockDim.x) groups[i] = Group{0, 0, 0, 0};
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t r = 0;
    for (uint32_t b = 0; b < n_blocks; ++b) {
      const uint32_t gq = b >= class_blocks ? gq1 : gq0;
      runbase[b] = r;
      r += (lo[b + 1] - lo[b] + gq - 1) / gq;
    }
    runbase[n_blocks] = r;
  }
  __syncthreads();
  const uint32_t nruns = min(runbase[n_blocks], max_runs);
  for (uint32_t r = threadIdx.x; r < nruns; r += blockDim.x) {
    uint32_t b = 0;
    while (b + 1 < n_blocks && r >= runbase[b + 1]) ++b;
    const uint32_t gq = b >= class_blocks ? gq1 : gq0;
    const uint32_t start = lo[b] + (r - runbase[b]) * gq, end = min(lo[b + 1], start + gq);
    const uint32_t k0 = sorted_keys[start], k1 = sorted_keys[end - 1];
    const uint32_t spr = b >= class_blocks ? (uint32_t)SPREAD : spr0;   // class 0 may stage wider slices
    run_start[r] = start;
    run_end[r] = end;
    run_off[r] = (k1 - k0 < spr) ? 1u : (k1 / spr - k0 / spr + 1);
  }
  __syncthreads();
  // exclusive scan of the group counts: a few hundred runs, every thread sums its own prefix
  uint32_t* cnt = run_off + max_runs + 1;  // [max_runs] copy of the counts
  for (uint32_t r = threadIdx.x; r < nruns; r += blockDim.x) cnt[r] = run_off[r];
  __syncthreads();
  for (uint32_t r = threadIdx.x; r <= nruns; r += blockDim.x) {
    uint32_t g = 0;
    for (uint32_t i = 0; i < r; ++i) g += cnt[i];
    run_off[r] = g;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    // group ranges for the persistent kernels: class 0 = [0, status[5]), class 1 = [status[5], status[4])
    const uint32_t r1 = class_blocks < n_blocks ? min(runbase[class_blocks], nruns) : nruns;
    status[4] = min(run_off[nruns], max_groups);
    status[5] = min(run_off[r1], max_groups);
  }
  for (uint32_t r = threadIdx.x; r < nruns; r += blockDim.x) {
    uint32_t b = 0;
    while (b + 1 < n_blocks && r >= runbase[b + 1]) ++b;
    const uint32_t cls = b >= class_blocks ? 1u : 0u;
    const uint32_t start = run_start[r], end = run_end[r], g0 = run_off[r], n = run_off[r + 1] - g0;
    if (n == 1) {
      if (g0 < max_groups) groups[g0] = Group{start, end - start, seg_div ? sorted_keys[start] / seg_div : 0u, cls};
    } else {
      const uint32_t spr = cls ? (uint32_t)SPREAD : spr0;
      const uint32_t kb = sorted_keys[start] / spr;
      uint32_t a = start;
      for (uint32_t k = 0; k < n; ++k) {
        const uint32_t e = k + 1 == n ? end : lower_bound(a, end, (uint64_t)(kb + k + 1) * spr);
        if (g0 + k < max_groups) groups[g0 + k] = Group{a, e - a, (seg_div && e > a) ? sorted_keys[a] / seg_div : 0u, cls};
        a = e;
      }
    }
  }
}

// ACC: partial sums carried across 160-site chunks in LDS (windows longer than CH); the
// short-window instantiation keeps no accumulators and stages only the slice (32 KB of LDS,
// 4 workgroups per CU).
template <int NCOLS, bool ACC>
__global__ void __launch_bounds__(GQ, ACC ? 2 : 4) k_preplace(const double* __restrict__ lookup,
                                                 const uint8_t* __restrict__ codes,
                                                 const uint32_t* __restrict__ win_begin,
                                                 const uint32_t* __restrict__ win_span,
                                                 const uint32_t* __restrict__ perm,
                                                 const Group* __restrict__ groups, uint32_t W,
                                                 uint32_t cstride, uint32_t crel,
                                                 uint32_t B, uint32_t pitch, size_t codes_bytes, uint32_t want_cls,
                                                 const uint32_t* __restrict__ status,
                                                 double* __restrict__ lnl) {
  constexpr bool SWZ = NCOLS == 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* tile = reinterpret_cast<double*>(smem);                  // [TROWS][NCOLS]
  double* accs = tile + (size_t)TROWS * NCOLS;                     // [NB][GQ] (ACC only)
  __shared__ uint32_t s_maxspan;
  // Persistent grid: work item = (group, tile of NB branches), groups fastest (neighbouring groups
  // overlap in the rows of T they stage: L2 reuse).  The group range of this kernel's class comes
  // from k_make_groups (status[4], status[5]); no workgroup is launched for an empty slot.
  const uint32_t gbeg = want_cls ? status[5] : 0, gend = want_cls ? status[4] : status[5];
  const uint32_t ng = gend - gbeg, ntiles = (B + NB - 1) / NB;
  const int t = threadIdx.x;
  for (uint32_t item = blockIdx.x; item < ng * ntiles; item += gridDim.x) {
  const Group g = groups[gbeg + item % ng];
  const uint32_t b0 = (item / ng) * NB;
  const uint32_t nb = min((uint32_t)NB, B - b0);
  __syncthreads();  // the previous item's readers of s_maxspan / accs / tile are done
  if (g.count == 0) continue;
  const bool active = t < (int)g.count;
  uint32_t qi = 0, begin = 0, span = 0;
  if (active) {
    qi = perm[g.start + t];
    begin = win_begin[qi];
    span = win_span[qi];
    if ((uint64_t)begin + span > W || (crel && span > cstride)) span = 0;  // invalid window: flagged by the validation pass
  }
  if (t == 0) s_maxspan = 0;
  __syncthreads();
  atomicMax(&s_maxspan, span);
  if (ACC) for (uint32_t j = 0; j < nb; ++j) accs[j * GQ + t] = 0.0;
  __syncthreads();
  // the group is a run of the begin-sorted order: its first / last member bound the rows of T
  // any member can touch in a chunk -> stage only those (spread + CH <= TROWS rows)
  const uint32_t gmin = win_begin[perm[g.start]];
  const uint32_t gspread = win_begin[perm[g.start + g.count - 1]] - gmin;  // < SPREAD
  const uint32_t rel = begin - gmin;
  const uint32_t nchunks = ACC ? (s_maxspan + CH - 1) / CH : 1;

  for (uint32_t c = 0; c < nchunks; ++c) {
    const uint32_t cbase = c * CH;           // chunk offset inside every thread's own window
    const bool mine = active && cbase < span;
    const uint32_t rem = mine ? span - cbase : 0;  // sites of this thread in this chunk (cap CH)
    // ---- my CH codes as byte offsets (code * 8), packed 4 per register
    uint32_t cw[CW];
    if (mine) {
      // row of query qi: Q x W layout (window at +begin) or compact (window at 0)
      const size_t addr = (size_t)qi * cstride + (crel ? 0u : begin) + cbase;
      const size_t a0 = addr & ~(size_t)3;
      const uint32_t sh = (uint32_t)(addr & 3) * 8;
      const size_t last = (codes_bytes - 1) & ~(size_t)3;
      const uint32_t* p = reinterpret_cast<const uint32_t*>(codes);
      uint32_t prev = p[min(a0, last) >> 2];
#pragma unroll
      for (int i = 0; i < CW; ++i) {
        const uint32_t nxt = p[min(a0 + 4 * (i + 1), last) >> 2];
        const uint32_t v = __funnelshift_r(prev, nxt, sh);
        uint32_t o = v << 3;  // each byte < 32 -> *8 stays inside the byte
        if (SWZ) {  // fold the row swizzle into the offsets once per chunk, not once per gather
          const uint32_t r = rel + 4 * i;  // tile row of the word's first site
          o ^= (((r >> 1) & 15) << 3) | ((((r + 1) >> 1) & 15) << 11) | ((((r + 2) >> 1) & 15) << 19) |
               ((((r + 3) >> 1) & 15) << 27);
        }
        cw[i] = o;
        prev = nxt;
      }
    } else {
#pragma unroll
      for (int i = 0; i < CW; ++i) cw[i] = 0;
    }
    const uint32_t row0 = gmin + cbase;  // first alignment site of the staged slice
    const uint32_t need = min((uint32_t)TROWS, gspread + min((uint32_t)CH, s_maxspan - cbase));
    for (uint32_t j = 0; j < nb; ++j) {
      __syncthreads();  // previous consumers of `tile` are done
      {
        const uint32_t rows = (row0 < W) ? min(need, W - row0) : 0;
        const double2* src = reinterpret_cast<const double2*>(
            lookup + ((size_t)(b0 + j) * W + row0) * NCOLS);
        double2* dst = reinterpret_cast<double2*>(tile);
        const uint32_t n2 = rows * NCOLS / 2;
        constexpr int PF = (TROWS * NCOLS / 2 + GQ - 1) / GQ;
        double2 pf[PF];
#pragma unroll
        for (int u = 0; u < PF; ++u) {  // all loads of the slice in flight at once
          const uint32_t i = u * GQ + t;
          if (i < n2) pf[u] = src[i];
        }
#pragma unroll
        for (int u = 0; u < PF; ++u) {
          const uint32_t i = u * GQ + t;
          if (i < n2) {
            double2 v = pf[u];
            uint32_t o = i;
            if (SWZ) {  // column pair (2p, 2p+1) of row r goes to columns (2p ^ f, (2p+1) ^ f)
              const uint32_t r = i >> 3, f = (r >> 1) & 15;
              o = (r << 3) | ((i & 7) ^ (f >> 1));
              if (f & 1) { const double x = v.x; v.x = v.y; v.y = x; }
            }
            dst[o] = v;
          }
        }
      }
      __syncthreads();
      if (mine) {
        double sum = ACC ? accs[j * GQ + t] : 0.0;
        // the gather addresses (row base + per-site byte offset) are loop-invariant over the
        // branches: left alone hipcc hoists all 160 of them into VGPRs; the zero token ties
        // them to j so they are rebuilt (2 VALU per gather) and the kernel fits 4 workgroups/CU
        uint32_t zj;
        asm volatile("v_mov_b32 %0, 0" : "=v"(zj) : "v"(j));
        const char* base = reinterpret_cast<const char*>(tile);
        const char* mybase = base + (size_t)(rel * (NCOLS * 8) + zj);
        auto at = [&](uint32_t s, uint32_t boff) -> double {
          return *reinterpret_cast<const double*>(mybase + s * (NCOLS * 8) + boff);
        };
        // Branch-free main loop: every group of 4 is read and summed in the reference's
        // association order, groups past the window contribute an exact +0.0.  (A branch per
        // group would end the basic block after 4 reads and expose the full LDS latency 40
        // times per slice; this way up to 15 reads stay in flight.)
        const uint32_t cur = min(rem, (uint32_t)CH);
        const uint32_t nfull = cur >> 2, ntail = cur & 3;
        // Software pipeline: batch k+1 (2 groups = 8 ds_read_b64) is issued before batch k is
        // summed; sched_barriers pin that order (left alone, hipcc sinks every read next to its
        // use and each group of 4 waits out a full LDS round trip: measured 183 cycles/group).
        constexpr int GPB = 2, NBATCH = CW / GPB;
        double rb[2][GPB * 4];
        auto issue = [&](int bt) {
#pragma unroll
          for (int g = 0; g < GPB; ++g) {
            const int i = bt * GPB + g;
            const uint32_t w = cw[i], s0 = 4 * i;
            rb[bt & 1][g * 4 + 0] = at(s0 + 0, w & 0xff);
            rb[bt & 1][g * 4 + 1] = at(s0 + 1, (w >> 8) & 0xff);
            rb[bt & 1][g * 4 + 2] = at(s0 + 2, (w >> 16) & 0xff);
            rb[bt & 1][g * 4 + 3] = at(s0 + 3, w >> 24);
          }
        };
        issue(0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int bt = 0; bt < NBATCH; ++bt) {
          if (bt + 1 < NBATCH) issue(bt + 1);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int g = 0; g < GPB; ++g) {
            const double* v = &rb[bt & 1][g * 4];
            double s1 = v[0] + v[1];
            const double s2 = v[2] + v[3];
            s1 += s2;
            sum += ((uint32_t)(bt * GPB + g) < nfull) ? s1 : 0.0;
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        if (ntail) {  // tail of the window: singles, in order
          uint32_t w = 0;
#pragma unroll
          for (int i = 0; i < CW; ++i) w = ((uint32_t)i == nfull) ? cw[i] : w;
          const uint32_t s0 = 4 * nfull;
#pragma unroll
          for (int k = 0; k < 3; ++k)
            if ((uint32_t)k < ntail) sum += at(s0 + k, (w >> (8 * k)) & 0xff);
        }
        if (ACC) accs[j * GQ + t] = sum;
        else lnl[(size_t)qi * pitch + b0 + j] = sum;
      }
    }
  }
  if (ACC && active) {
    double* out = lnl + (size_t)qi * pitch + b0;
    for (uint32_t j = 0; j < nb; ++j) out[j] = accs[j * GQ + t];
  }
  }  // work items
}

// ---------------------------------------------------------------------------------------------
// Site-pair fast path (DNA).
// ---------------------------------------------------------------------------------------------
constexpr int NSYM = 6;                 // A C G T N(or gap) none
constexpr int PE = NSYM * NSYM;         // entries per pair row, in pair_entry() order
constexpr int PROWB = PE * 8;           // 288 bytes per pair row in HBM
// Entry order and LDS row stride are chosen for the LDS banks (64 dwords; a ds_read_b64 serves 32
// lanes per cycle when their 8-byte words sit on different bank pairs or coincide).  32 neighbouring
// queries of the sorted order start on one or two adjacent pair rows and, site pair by site pair, read
// one of the 16 plain-nucleotide entries of "their" row.  Those 16 entries come FIRST in a row (128
// contiguous bytes = 32 banks) and rows are ROWL_NARROW = 384 bytes apart in LDS (96 dwords = 32 mod
// 64): the hot halves of adjacent rows cover all 64 banks once, the gathers of a lane group are
// conflict-free.  exp/lds_gather.hip, 37 queries per start: 198 B/clk/CU against 143 for the old
// e = s0 * 6 + s1 order at 288 bytes (row r on bank 8 r: every second symbol of adjacent rows collides),
// which is why padding 288 -> 296 alone never helped.  Wide (small-chunk) and multi-chunk variants keep
// 288-byte rows: their slices would not fit the 16-bit offsets / the LDS at 384, and their lane groups
// span many rows anyway (12 queries per start: 125 vs 120 B/clk).
constexpr int ROWL_NARROW = 384;
constexpr int ROWL_PACKED = PROWB;
constexpr int CP = CH / 2;              // pair slots per chunk
constexpr int PW = CP / 2;              // packed words (2 x 16-bit LDS offsets) per chunk
constexpr int TROWS2 = TROWS / 2;       // pair rows staged per (branch, chunk)
constexpr int GQ2 = 1024;               // queries (threads) per group of the pair path: one
                                        // workgroup per CU, the staged slice is shared by 1024 queries
                                        // branches per item of the single-chunk fast paths: choose_tile()
constexpr int NB2_ACC = 15;             // branches per work item when partial sums live in LDS (multi-chunk
                                        // windows): 15 x 1024 doubles + the 36 KB slice fill the CU's 160 KB
constexpr int NB2_ACC_S = 14;           // the same for the 20-state site path (43 KB slice)
constexpr int NB2_BURST = 8;            // single-chunk variants: result rows staged per 64-byte burst
constexpr uint32_t ZERO_OFF = (PE - 1) * 8;  // (none, none) of the thread's own first row: exact +0.0

// (symbol of site, symbol of site + 1) -> entry of the pair row: the 16 plain pairs first
__device__ __forceinline__ uint32_t pair_entry(uint32_t s0, uint32_t s1) {
  if (s0 < 4 && s1 < 4) return s0 * 4 + s1;
  if (s0 < 4) return 16 + s0 * 2 + (s1 - 4);
  return 24 + (s0 - 4) * NSYM + s1;      // (5, 5) = PE - 1
}
__device__ __forceinline__ void pair_symbols(uint32_t e, uint32_t& s0, uint32_t& s1) {
  if (e < 16) { s0 = e >> 2; s1 = e & 3u; }
  else if (e < 24) { s0 = (e - 16) >> 1; s1 = 4 + ((e - 16) & 1u); }
  else { s0 = 4 + (e - 24) / NSYM; s1 = (e - 24) % NSYM; }
}

// state-set code (4-bit mask) -> symbol; 6 = any other ambiguity code (generic kernel).  Code 0 is a gap inside the
// window: its lookup column has N's state set (column_mask) and so N's bits, and it takes N's symbol.
__device__ __forceinline__ uint32_t dna_sym(uint32_t code) {
  if (code == 15 || code == 0) return 4;
  if (code == 1 || code == 2 || code == 4 || code == 8) return (uint32_t)__ffs((int)code) - 1;
  return 6;
}

// T2[b][s][e] = (i0 < 5 ? T[b][s][code(i0)] : 0) + (i1 < 5 ? T[b][s+1][code(i1)] : 0).  The sum is
// the very `a0 + a1` the reference's 4-way unrolled loop forms first (Lookup_Store.hpp:120-131),
// x + 0.0 == x covers the singles of the tail.
__global__ void __launch_bounds__(256) k_build_lookup2(const double* __restrict__ lookup, uint32_t W,
                                                       double* __restrict__ lookup2, uint32_t b0) {
  const uint32_t b = b0 + blockIdx.y;
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= W * PE) return;
  const uint32_t s = i / PE, e = i - s * PE;
  uint32_t i0, i1;
  pair_symbols(e, i0, i1);
  const uint32_t code[5] = {1, 2, 4, 8, 15};
  const double* T = lookup + (size_t)b * W * 16;
  const double v0 = i0 < 5 ? T[(size_t)s * 16 + code[i0]] : 0.0;
  const double v1 = (i1 < 5 && s + 1 < W) ? T[(size_t)(s + 1) * 16 + code[i1]] : 0.0;
  // rows of one start parity are contiguous: [b][s & 1][s >> 1][PE].  A group of queries uses the
  // rows of ONE parity; interleaved, its slice was 288 useful bytes out of every 576
  const uint32_t Wh = (W + 1) / 2;
  lookup2[(((size_t)b * 2 + (s & 1u)) * Wh + (s >> 1)) * PE + e] = v0 + v1;
}

// Per-pair LDS offsets relative to the query's first pair row, 16 bit each (pair p of the window sits in
// chunk p / CP at row p % CP), the three tail singles, the sort key (class, window-start parity, window
// start) for the grouping.
// (code of site, code of site + 1) -> 8 * pair entry, bit 15 = one of the two is a rare ambiguity code
// (the query then goes to the generic kernel); codes above 15 are mapped to code 0 first (same symbol).
struct PairTab {
  uint16_t v[256];
  constexpr PairTab() : v{} {
    for (uint32_t i = 0; i < 256; ++i) {
      const uint32_t c[2] = {i >> 4, i & 15u};
      uint32_t s[2] = {0, 0};
      for (int k = 0; k < 2; ++k)
        s[k] = (c[k] == 15 || c[k] == 0) ? 4u : c[k] == 1 ? 0u : c[k] == 2 ? 1u : c[k] == 4 ? 2u : c[k] == 8 ? 3u : 6u;   // = dna_sym
      const bool rare = s[0] > 4 || s[1] > 4;
      const uint32_t s0 = s[0] > 5 ? 5u : s[0], s1 = s[1] > 5 ? 5u : s[1];
      const uint32_t e = (s0 < 4 && s1 < 4) ? s0 * 4 + s1 : s0 < 4 ? 16 + s0 * 2 + (s1 - 4) : 24 + (s0 - 4) * NSYM + s1;   // = pair_entry
      v[i] = (uint16_t)(e * 8 | (rare ? 0x8000u : 0u));
    }
  }
};
__device__ const PairTab PAIR_TAB{};

// Sixteen lanes per query, four queries per wave, a persistent grid (grid-stride over blocks of sixteen
// queries).  Round 5: a lane forms one 32-bit WORD (two pairs = four sites) per step -- four code bytes, two
// table reads (LDS copy of PAIR_TAB), one add of the two row offsets, one 4-byte store (sixteen lanes: 64
// contiguous bytes) -- where the first form walked dna_sym / pair_entry per site (branches: 352 vector + 640
// scalar instructions per wave, 81 us per 100k reads: instruction-bound, profiles/r5_pmc_summary.txt).
// Offsets stay below 2^15 ((CP - 1) * rowl + 35 * 8 <= 30616), so the table's rare bit survives the add in
// bit 15 / 31 and is masked out of the stored word.
__global__ void __launch_bounds__(256) k_pack_pairs(const uint8_t* __restrict__ codes,
                                                    const uint32_t* __restrict__ win_begin,
                                                    const uint32_t* __restrict__ win_span, uint32_t Q,
                                                    uint32_t W, uint32_t cstride, uint32_t crel,
                                                    uint32_t span_bound, uint32_t Wp, uint32_t NP16,
                                                    uint32_t rowl, uint16_t* __restrict__ packed,
                                                    uint16_t* __restrict__ tails,
                                                    uint32_t* __restrict__ keys, uint32_t K,
                                                    uint32_t* __restrict__ status) {
  __shared__ uint16_t s_tab[256];
  s_tab[threadIdx.x] = PAIR_TAB.v[threadIdx.x];
  __syncthreads();
  const uint32_t l16 = threadIdx.x & 15, grp = (threadIdx.x >> 4) & 3u;
  // a window longer than the caller's max_span (or than a compact row) is an input error: the
  // kernel variant and the packed rows were sized by it
  const uint32_t cmax = min(span_bound, crel ? cstride : 0xffffffffu);
  constexpr uint32_t ZERO_W = ZERO_OFF | (ZERO_OFF << 16);
  constexpr int NWI = (PW + 15) / 16;     // word steps per chunk of CP pair slots
  const uint32_t lane_base = (2u * l16 * rowl) * 0x10001u + (rowl << 16);   // rows 2 l16 and 2 l16 + 1
  for (uint32_t q0 = blockIdx.x * 16; q0 < Q; q0 += gridDim.x * 16) {
    const uint32_t q = q0 + (threadIdx.x >> 4);
    const bool live = q < Q;
    const uint32_t begin = live ? win_begin[q] : 0u;
    uint32_t span = live ? win_span[q] : 0u;
    if (live && l16 == 0) validate_window(q, begin, span, W, cmax, status);
    if ((uint64_t)begin + span > W || span > cmax) span = 0;  // invalid window (flagged above)
    const uint8_t* c = codes + (size_t)(live ? q : 0u) * cstride + (crel ? 0u : begin);
    const uint32_t nfull = span >> 2, ntail = span & 3, npairs = 2 * nfull;
    uint32_t* prow = reinterpret_cast<uint32_t*>(packed + (size_t)(live ? q : 0u) * NP16);   // NP16 is even, the base 256-byte aligned
    uint32_t racc = 0;
    // the tail singles' codes are requested with the first chunk's
    uint32_t ctail = 0;
    if (l16 < ntail) ctail = c[4 * nfull + l16];
    for (uint32_t pb = 0; pb < NP16; pb += CP) {   // one chunk of CP = 80 pair slots = 40 words at a time
      uint32_t cb[NWI][4];
#pragma unroll
      for (int i = 0; i < NWI; ++i) {
        const uint32_t gw = pb / 2 + (uint32_t)i * 16 + l16;   // word = pairs 2 gw, 2 gw + 1 = sites 4 gw .. 4 gw + 3
        const bool on = (i * 16 + (int)l16 < PW) && gw < nfull;
#pragma unroll
        for (int k = 0; k < 4; ++k) cb[i][k] = on ? c[4 * gw + k] : 0u;
      }
#pragma unroll
      for (int i = 0; i < NWI; ++i) {
        const uint32_t wl = (uint32_t)i * 16 + l16, gw = pb / 2 + wl;
        if (i * 16 + (int)l16 >= PW) continue;
        uint32_t c0 = cb[i][0], c1 = cb[i][1], c2 = cb[i][2], c3 = cb[i][3];
        if (__builtin_expect(((c0 | c1 | c2 | c3) >> 4) != 0u, 0)) {   // not a 4-bit state set: the symbol of code 0
          c0 = c0 > 15u ? 0u : c0; c1 = c1 > 15u ? 0u : c1; c2 = c2 > 15u ? 0u : c2; c3 = c3 > 15u ? 0u : c3;
        }
        const uint32_t e0 = s_tab[(c0 << 4) | c1], e1 = s_tab[(c2 << 4) | c3];
        const uint32_t word = ((e1 << 16) | e0) + lane_base + (uint32_t)i * ((32u * rowl) * 0x10001u);
        const bool on = gw < nfull;
        if (on) racc |= word;
        if (live) prow[gw] = on ? (word & 0x7fff7fffu) : ZERO_W;
      }
    }
    bool rare = (racc & 0x80008000u) != 0u;
    if (l16 < 4) {
      uint32_t v = ZERO_OFF;
      if (l16 < ntail) {
        uint32_t sy = dna_sym(ctail);
        rare |= sy > 4;
        sy = min(sy, 5u);
        const uint32_t kt = npairs % CP;  // row of the first tail site inside its chunk (even)
        const uint32_t e = l16 == 1 ? pair_entry(5, sy) : pair_entry(sy, 5);
        v = (kt + (l16 == 2 ? 1u : 0u)) * rowl + e * 8;
      }
      if (live) tails[(size_t)q * 4 + l16] = (uint16_t)v;
    }
    const bool any_rare = ((__ballot(rare) >> (16 * grp)) & 0xffffull) != 0ull;
    if (live && l16 == 0) {   // an invalid window start (flagged above) must not leave the key space
      const uint32_t key = min((any_rare ? 2 * Wp : 0) + (begin & 1u) * Wp + min(begin, Wp - 1), K - 1);
      keys[q] = key;
    }
  }
}

// Walk of the (branch tile, group) work items by a persistent grid.  Workgroups are dealt to the
// eight XCDs round robin (workgroup w runs on XCD w % 8, each with its own 4 MB L2), and the groups
// are sorted by window start: neighbouring groups stage overlapping slices of the same branch rows
// (a site lies in the slices of ~6 groups at cfg2).  XCD x therefore takes the CONTIGUOUS eighth
// [x T / 8, (x + 1) T / 8) of the items in (tile, group) order and its workgroups stride through
// it, so that at any time one L2 serves neighbouring groups of one tile instead of every eighth:
// slice re-reads that reach the fabric 3.5 GB -> 1.5 GB per 100k-read launch (PMC, round 3).
#ifndef PP_XCD
#define PP_XCD 1
#endif
// ---- per-(query, 64-branch segment) maxima of the preplacement table, written by the single-chunk fast
// paths as a by-product (one fmax per branch, one atomic per segment and work item) and read by the
// candidate selection (k_select_seg): a query's candidates and every term that can move its LWR
// denominator lie in the one or two segments whose maximum is within a few dozen lnL units of the row
// maximum (cfg2: 1.5 of 16 segments on average), so the selection reads 128 bytes of maxima + those
// segments instead of the whole 8 KB row.  Stored as order-preserving 64-bit keys (atomicMax on unsigned
// integers: epa_wave::seg_key), 0 = nothing written (a query served by another kernel: the selection then reads its row).
using epa_wave::seg_key;
struct SegTrack {   // running maximum of the current segment of one query
  double m = -INFINITY;
  __device__ __forceinline__ void add(unsigned long long* __restrict__ segmax, uint32_t segp, uint32_t qi, uint32_t b,
                                      bool last, double v) {
    m = fmax(m, v);
    if ((b & 63u) == 63u || last) {
      atomicMax(&segmax[(size_t)qi * segp + (b >> 6)], seg_key(m));
      m = -INFINITY;
    }
  }
};

// Progress-based wave priority in the gather loops (round 5).  The SIMD's arbiter is oldest-first, so the sixteen waves
// of the workgroup get through a branch's gathers at different speeds and the average wave waited 1200 of a branch's
// 5200 clocks at the barrier for the slowest one (profiles/r4_preplace_cycles.txt).  A wave now starts its gathers at
// priority 3 and steps down to 0 a quarter of its batches at a time: whoever is behind issues first, the waves reach
// the barrier together.  Same box, cfg2: 0.965 -> 0.910 ms per launch (PP_PRIO=0: off; two levels 0.929, thresholds at
// 40 / 70 / 90 % 0.914, at 10 / 30 / 60 % 0.930; the double-buffered and two-branch loops still lose with it:
// 0.949 / 1.011; profiles/r5_preplace_prio_ab.txt).
#ifndef PP_PRIO
#define PP_PRIO 1
#endif
template <int NBATCH>
__device__ __forceinline__ void gather_prio(int bt) {
#if PP_PRIO == 1
  if (bt == 0) __builtin_amdgcn_s_setprio(3);
  else if (bt == NBATCH / 4) __builtin_amdgcn_s_setprio(2);
  else if (bt == NBATCH / 2) __builtin_amdgcn_s_setprio(1);
  else if (bt == (3 * NBATCH) / 4) __builtin_amdgcn_s_setprio(0);
#elif PP_PRIO == 2   // two levels
  if (bt == 0) __builtin_amdgcn_s_setprio(3);
  else if (bt == NBATCH / 2) __builtin_amdgcn_s_setprio(0);
#elif PP_PRIO == 3   // late thresholds
  if (bt == 0) __builtin_amdgcn_s_setprio(3);
  else if (bt == (2 * NBATCH) / 5) __builtin_amdgcn_s_setprio(2);
  else if (bt == (7 * NBATCH) / 10) __builtin_amdgcn_s_setprio(1);
  else if (bt == (9 * NBATCH) / 10) __builtin_amdgcn_s_setprio(0);
#elif PP_PRIO == 4   // early thresholds
  if (bt == 0) __builtin_amdgcn_s_setprio(3);
  else if (bt == NBATCH / 10) __builtin_amdgcn_s_setprio(2);
  else if (bt == (3 * NBATCH) / 10) __builtin_amdgcn_s_setprio(1);
  else if (bt == (6 * NBATCH) / 10) __builtin_amdgcn_s_setprio(0);
#endif
}

struct ItemWalk { uint32_t pos, end, step, lo; };
__device__ __forceinline__ ItemWalk item_walk(uint32_t total) {
  if (PP_XCD && (gridDim.x & 7u) == 0) {
    const uint32_t x = blockIdx.x & 7u, local = blockIdx.x >> 3;
    const uint32_t lo = (uint32_t)((uint64_t)total * x / 8), hi = (uint32_t)((uint64_t)total * (x + 1) / 8);
    return {lo + local, hi, gridDim.x >> 3, lo};
  }
  return {blockIdx.x, total, gridDim.x, 0u};
}

// Which (group, tile) a position v of an XCD's contiguous range [lo, hi) stands for.  The RANGES are cut in group-major
// order (u = group * ntiles + tile): an XCD owns ~ng / 8 whole groups (a boundary group is shared by two), so the
// packed offsets of a group -- 160 B per query, read again by every one of its tiles -- come out of ONE L2 instead of
// a different one per tile (0.2 GB of the launch's HBM-side traffic at cfg2).  INSIDE its range an XCD still walks
// tile-major (tile t: the range's groups ascending), so the workgroups running at the same time stage overlapping
// slices of the same branches.  With lo = 0, hi = total this is the plain tile-major order (tile = v / ng).
#ifndef PP_XCD_GROUPS
#define PP_XCD_GROUPS 1
#endif
__device__ __forceinline__ void item_group_tile(uint32_t v, uint32_t lo, uint32_t hi, uint32_t ng, uint32_t ntiles,
                                                uint32_t& grp, uint32_t& tile) {
  if (!PP_XCD_GROUPS) { grp = v % ng; tile = v / ng; return; }
  const uint32_t gl = lo / ntiles, tl = lo - gl * ntiles, gh = (hi - 1) / ntiles, th = (hi - 1) - gh * ntiles;
  uint32_t r = v - lo;
  for (uint32_t t = 0; t < ntiles; ++t) {
    const uint32_t first = gl + (t < tl ? 1u : 0u), last1 = gh + 1u - (t > th ? 1u : 0u);   // [first, last1)
    const uint32_t c = last1 > first ? last1 - first : 0u;
    if (r < c) { grp = first + r; tile = t; return; }
    r -= c;
  }
  grp = 0; tile = ntiles;   // not reached for lo <= v < hi
}

// Branches per work item of the single-chunk fast paths (ng groups x ceil(B / n) items on nwg
// persistent workgroups): the multiple of 8 (whole result bursts) in 16 .. 96 with the smallest
// rounds x (branches + per-item setup).  Per item a workgroup fetches its queries' offsets (160 B per
// query) and runs a chain of dependent loads before the first slice is staged, ~3 branch times: at
// cfg2 (98 groups, 1021 branches, 256 workgroups) 13 tiles of 80 are 5 rounds = 415 branch times
// where 32 tiles of 32 were 13 rounds = 455, and the offsets are read 13 times instead of 32; a
// 5000-read chunk (10 groups) gets 43 tiles of 24 instead of 1.25 rounds of 32.
__device__ __forceinline__ uint32_t choose_tile(uint32_t ng, uint32_t B, uint32_t nwg) {
  uint32_t best = 32, best_cost = 0xffffffffu;
  for (uint32_t n = 16; n <= 96; n += 8) {
    const uint32_t items = ng * ((B + n - 1) / n);
    const uint32_t cost = ((items + nwg - 1) / nwg) * (n + 3);
    if (cost <= best_cost) { best_cost = cost; best = n; }
  }
  return best;
}

// SPR: window starts of a group lie within SPR sites.  96 for large chunks (many reads per window
// start: 1024 consecutive reads of the sorted order span few starts); 288 for small ones (the
// reference's default --chunk-size 5000 puts ~2 reads on a start: a 96-site bucket holds ~180 reads,
// a workgroup's 1024 lanes would be 18 % full) -- the 16-bit LDS offsets still fit:
// (288 / 2 + 79) * 288 + 35 * 8 < 65536.  ROWL: byte stride of the staged pair rows in LDS (see above).
// (the batch structure was once pinned with sched_barriers; with two-word batches the compiler's own
// schedule is as good or better: -DPP_SCHED_PIN restores them for an A/B)
#ifdef PP_SCHED_PIN
#define PP_SCHED_BARRIER() __builtin_amdgcn_sched_barrier(0)
#else
#define PP_SCHED_BARRIER()
#endif
// Two other loop forms were built, measured and dropped (source kept under profiles/variants/r5_preplace_db_duo_v1.hip,
// A/Bs in profiles/r5_preplace_duo_ab.txt, r5_preplace_prio_ab.txt): slices of consecutive branches alternating between
// two LDS buffers with one barrier per branch (0.966 / 0.949 against 0.930 / 0.910 ms), and two branches staged and
// gathered between one pair of barriers (1.018 / 1.011 ms) -- the gather phase is bound by the LDS itself.
// SPARSE (the exact pass behind the fp32 screen, below): groups are groups of (query, segment) CELLS of one segment
// (Group::min_begin), perm holds a cell's query, an item is one group over the segment's 64 branches; staging, gathers,
// bursts and segment maxima are the same code, so a cell's value is the one the full pass writes.
template <bool ACC, int SPR, int ROWL, bool SPARSE = false>
__global__ void __launch_bounds__(GQ2, 4) k_preplace_pairs(
    const double* __restrict__ lookup2, const uint16_t* __restrict__ packed,
    const uint16_t* __restrict__ tails, const uint32_t* __restrict__ win_begin,
    const uint32_t* __restrict__ win_span, const uint32_t* __restrict__ perm,
    const Group* __restrict__ groups, uint32_t W, uint32_t B, uint32_t pitch, uint32_t NP16,
    const uint32_t* __restrict__ status, double* __restrict__ lnl,
    unsigned long long* __restrict__ segmax, uint32_t segp) {
  constexpr int TR2 = (CH + SPR) / 2;   // pair rows staged per (branch, chunk)
  extern __shared__ __attribute__((aligned(16))) char smem[];  // [TR2][PE] doubles, then accs
  static_assert(ROWL % 16 == 0 && ROWL >= PROWB && ((TR2 - 1) * ROWL + PROWB) < 65536, "16-bit LDS offsets");
  double* accs = reinterpret_cast<double*>(smem + (size_t)TR2 * ROWL);  // [NB2_ACC][GQ2] / burst rows
  __shared__ uint32_t s_maxspan;
  __shared__ uint32_t s_qi[GQ2];   // query of thread t (burst write-out), ~0 = nothing to write
  constexpr uint32_t BSTR = GQ2 + 4;    // burst staging rows 4 doubles apart in the banks: conflict-free
  // persistent grid over (group, branch tile) items of class 0, see k_preplace
  const uint32_t ng = status[5];
  const uint32_t NBP = SPARSE ? 64u : ACC ? NB2_ACC : choose_tile(ng, B, gridDim.x);
  const uint32_t ntiles = SPARSE ? 1u : (B + NBP - 1) / NBP;
  const int t = threadIdx.x;
  // SPARSE: plain striding.  The cells crowd into the few segments around the reads' placements, whose full groups are
  // neighbours in the segment-major order, so no XCD's contiguous eighth should hold them all; traced, the walk is
  // worth little (0.316 -> 0.306 ms per launch, profiles/r9_preplace_screen_ab.txt)
  const ItemWalk iw = SPARSE ? ItemWalk{blockIdx.x, ng, gridDim.x, 0u} : item_walk(ng * ntiles);
  for (uint32_t item = iw.pos; item < iw.end; item += iw.step) {
  uint32_t item_g = item, item_t = 0;
  if (!SPARSE) item_group_tile(item, iw.lo, iw.end, ng, ntiles, item_g, item_t);
  const Group g = groups[item_g];
  const uint32_t b0 = SPARSE ? min(g.min_begin * 64u, B - 1u) : item_t * NBP;
  const uint32_t nb = min(NBP, B - b0);
  __syncthreads();  // the previous item's readers of s_maxspan / accs / the tile are done
  if (g.count == 0) continue;
  const bool active = t < (int)g.count;
  uint32_t qi = 0, begin = 0, span = 0;
  if (active) {
    qi = perm[g.start + t];
    begin = win_begin[qi];
    span = win_span[qi];
    if ((uint64_t)begin + span > W) span = 0;
  }
  if (t == 0) s_maxspan = 0;
  const uint32_t my_q = (active && span > 0) ? qi : 0xffffffffu;
  s_qi[t] = my_q;
  __syncthreads();
  {   // one LDS atomic per wave, not per thread (1024 atomics on one word cost ~16k cycles per item)
    uint32_t m = span;
#pragma unroll
    for (int off = 32; off; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off));
    if ((t & 63) == 0) atomicMax(&s_maxspan, m);
  }
  if (ACC) for (uint32_t j = 0; j < nb; ++j) accs[j * GQ2 + t] = 0.0;
  __syncthreads();
  // all members share the parity of their window start: rel is even, pair rows line up
  const uint32_t gmin = win_begin[perm[g.start]];
  const uint32_t gspread = win_begin[perm[g.start + g.count - 1]] - gmin;  // < SPREAD
  const uint32_t rowoff = ((begin - gmin) >> 1) * ROWL;
  const uint32_t rowoff2 = rowoff | (rowoff << 16);
  const uint32_t nchunks = ACC ? (s_maxspan + CH - 1) / CH : 1;
  uint32_t t0 = 0, t1 = 0, t2 = 0, tailchunk = 0xffffffffu;
  if (active && (span & 3)) {
    const uint16_t* tq = tails + (size_t)qi * 4;
    t0 = tq[0] + rowoff; t1 = tq[1] + rowoff; t2 = tq[2] + rowoff;
    tailchunk = ((span >> 2) * 2) / CP;
  }
  auto at = [&](uint32_t off) -> double { return *reinterpret_cast<const double*>(smem + off); };
  SegTrack seg;

  for (uint32_t c = 0; c < nchunks; ++c) {
    const uint32_t cbase = c * CH;
    const bool mine = active && cbase < span;
    uint32_t cw[PW];  // two 16-bit LDS byte offsets per word = one group of 4 sites
    if (mine) {
      // 160 B per (query, chunk), 16 B aligned (NP16 is a multiple of CP = 80)
      const uint4* p = reinterpret_cast<const uint4*>(packed + (size_t)qi * NP16 + (size_t)c * CP);
#pragma unroll
      for (int i = 0; i < PW / 4; ++i) {  // no carry between the halves: offsets stay below 2^16
        const uint4 v = p[i];
        cw[4 * i] = v.x + rowoff2;
        cw[4 * i + 1] = v.y + rowoff2;
        cw[4 * i + 2] = v.z + rowoff2;
        cw[4 * i + 3] = v.w + rowoff2;
      }
    } else {
#pragma unroll
      for (int i = 0; i < PW; ++i) cw[i] = 0;
    }
    const uint32_t row0 = gmin + cbase;  // alignment site of pair row 0 of the staged slice
    const uint32_t need = min((uint32_t)TR2, (gspread >> 1) + (min((uint32_t)CH, s_maxspan - cbase) + 1) / 2);
    const uint32_t rows = (row0 < W) ? min(need, (W - row0 + 1) / 2) : 0;
    const uint32_t n2 = rows * (PE / 2);
    constexpr int PF = (TR2 * (PE / 2) + GQ2 - 1) / GQ2;
    auto request = [&](uint32_t j, double2 (&pfs)[PF]) {
      // pair row r = table row (row0 + 2r); the rows of one parity are contiguous in lookup2
      const double2* src = reinterpret_cast<const double2*>(
          lookup2 + (((size_t)(b0 + j) * 2 + (row0 & 1u)) * ((W + 1) / 2) + (row0 >> 1)) * PE);
#pragma unroll
      for (int u = 0; u < PF; ++u) {
        const uint32_t i = u * GQ2 + t;
        pfs[u] = make_double2(0.0, 0.0);
        if (i < n2) pfs[u] = src[i];
      }
    };
    auto stage = [&](const double2 (&pfs)[PF], uint32_t boff) {
#pragma unroll
      for (int u = 0; u < PF; ++u) {
        const uint32_t i = u * GQ2 + t;   // double2 index in the compact [rows][PE / 2] slice
        if (i < n2) {
          if (ROWL == PROWB) {
            reinterpret_cast<double2*>(smem + boff)[i] = pfs[u];
          } else {                         // padded rows
            const uint32_t r = i / (PE / 2), c2 = i - r * (PE / 2);
            *reinterpret_cast<double2*>(smem + boff + r * ROWL + c2 * 16) = pfs[u];
          }
        }
      }
    };
    // the gathers of branch j from the slice staged at byte boff; the sum goes to the staging rows
    auto gather = [&](uint32_t j, uint32_t boff) {
      if (mine) {
        double sum = ACC ? accs[j * GQ2 + t] : 0.0;
        // the offsets are invariant over the branches: without this hipcc hoists the 80 extracted
        // addresses out of the j loop into VGPRs (the kernel has to fit 4 workgroups per CU)
#pragma unroll
        for (int i = 0; i < PW; ++i) asm volatile("" : "+v"(cw[i]));
        // Software pipeline as in k_preplace: batch k+1 (4 words = 8 ds_read_b64) is issued
        // before batch k is summed.  Slots past the window read an exact +0.0.
#ifndef PP_WPB
#define PP_WPB 2   // round 4 A/B, ms per 100k-read launch: 1 -> 0.91, 2 -> 0.905 - 0.914, 4 -> 0.93 - 0.95, 5 -> 0.95, 8 -> 1.35
#endif
        constexpr int WPB = PP_WPB, NBATCH = PW / WPB;
        double rb[2][WPB * 2];
        auto issue = [&](int bt) {
#pragma unroll
          for (int w = 0; w < WPB; ++w) {
            const uint32_t v = cw[bt * WPB + w];
            rb[bt & 1][2 * w] = at((v & 0xffffu) + boff);
            rb[bt & 1][2 * w + 1] = at((v >> 16) + boff);
          }
        };
        issue(0);
        PP_SCHED_BARRIER();
#pragma unroll
        for (int bt = 0; bt < NBATCH; ++bt) {
          gather_prio<NBATCH>(bt);
          if (bt + 1 < NBATCH) issue(bt + 1);
          PP_SCHED_BARRIER();
#pragma unroll
          for (int w = 0; w < WPB; ++w) {
            const double s1 = rb[bt & 1][2 * w] + rb[bt & 1][2 * w + 1];  // (a0+a1) + (a2+a3)
            sum += s1;
          }
          PP_SCHED_BARRIER();
        }
        if (c == tailchunk) {  // singles of the window tail, in order
          sum += at(t0 + boff);
          sum += at(t1 + boff);
          sum += at(t2 + boff);
        }
        if (ACC) {
          accs[j * GQ2 + t] = sum;
        } else {
          accs[(j & 7u) * BSTR + t] = sum;
          if (segmax) seg.add(segmax, segp, qi, b0 + j, j + 1 == nb, sum);
        }
      }
    };
    // Results leave in bursts of 8 consecutive branches, 64 B per query, and the eight lanes
    // l, l+1 .. l+7 write the eight doubles of ONE query: every store instruction hands the
    // memory system whole 64-byte sectors (8 queries per wave and instruction).  History: single
    // 8-byte stores spread over the item were evicted sector by sector (1.76 GB written for a
    // 0.41 GB table); 8 stores per lane back to back, each lane its own sector, relied on L2
    // merging them before eviction (1.19 GB for 0.83 GB; 2.15 GB under the XCD-contiguous walk).
    // Burst kb = branches b0 + 8 kb .. of this item, staged in rows 0 .. 7.
    auto emit_burst = [&](uint32_t kb) {
      __builtin_amdgcn_wave_barrier();
      // four lanes per query, 16 bytes (two branches) per lane: a store instruction still hands over whole
      // 64-byte sectors (16 queries per wave and instruction) with half as many instructions as 8-byte
      // stores -- the write-out is store-issue bound (in-kernel cycle counters: 3.7k cycles per burst)
      const uint32_t lane = (uint32_t)t & 63u, wbase = (uint32_t)t & ~63u, c4 = lane & 3u;
      const uint32_t ncol = min(8u, nb - 8u * kb), bcol = b0 + 8u * kb + 2u * c4;
      const uint32_t r0 = 2u * c4, r1 = 2u * c4 + 1u;
#pragma unroll
      for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t tq = wbase + k * 16 + (lane >> 2);
        const uint32_t q = s_qi[tq];
        if (q != 0xffffffffu && 2u * c4 < ncol) {
          const double a0 = accs[r0 * BSTR + tq];
          double* dst = lnl + (size_t)q * pitch + bcol;
          if (2u * c4 + 1u < ncol) *reinterpret_cast<double2*>(dst) = make_double2(a0, accs[r1 * BSTR + tq]);
          else *dst = a0;
        }
      }
      __builtin_amdgcn_wave_barrier();
    };
    // All sixteen waves issue their bursts behind the same barrier, every eighth branch (535 of a branch's 5200 clocks
    // with the LDS gather path idle).  Round 6 built the stagger VERDICT round 5 asked for -- a ring of twelve staging
    // rows, wave w writing its burst (w & 3) branches late, four waves per branch on four of eight branches -- bit-
    // identical and 5 - 6 % SLOWER (0.956 - 0.972 against 0.906 - 0.912 ms per launch, three interleaved rounds:
    // profiles/r6_ab_spec_step_stagger.txt; source profiles/variants/r6_preplace_stagger.hip): the late waves arrive
    // late at that branch's barrier, and the barrier is what the other fifteen wait at.  The kernel is closed here.
    auto flush = [&](uint32_t j) {
      if (ACC) return;
      if ((j & 7u) == 7u) emit_burst(j >> 3);
      else if (j + 1 == nb) emit_burst(j >> 3);
    };
    {
      // The slice of branch j+1 is requested (into registers) before the gathers of branch j start
      // and written to LDS after them: its HBM latency hides under the gather phase.
      double2 pf[PF];
      request(0, pf);
      for (uint32_t j = 0; j < nb; ++j) {
        __syncthreads();  // previous consumers of the tile are done
        stage(pf, 0);
        __syncthreads();
        if (j + 1 < nb) request(j + 1, pf);
        PP_SCHED_BARRIER();
        gather(j, 0);
        flush(j);
      }
    }
  }
  if (ACC && active) {
    double* out = lnl + (size_t)qi * pitch + b0;
    for (uint32_t j = 0; j < nb; ++j) out[j] = accs[j * GQ2 + t];
  }
  }  // work items
}

// ---------------------------------------------------------------------------------------------
// fp32 two-branch screen of the pair path ("fp32 screen").  The selection reads only the table segments
// whose maximum lies within band_t of the row maximum; of every other segment it uses that one fact, which fp32 sums
// decide as well once the band is widened by their error bound.  lookup2f holds, per PAIR of branches (2p, 2p + 1) and
// in lookup2's own [parity][pair row][PE] layout, the two branches' entries rounded to fp32 side by side: an entry is
// still 8 bytes, so the packed 16-bit LDS offsets, the staged slice and the groups are those of k_preplace_pairs, and
// one ds_read_b64 + one packed add serve two (query, branch) cells.
typedef float f2 __attribute__((ext_vector_type(2)));

// order-preserving 32-bit key of a float (atomicMax on unsigned integers), 0 = nothing written: seg_key in fp32
__device__ __forceinline__ uint32_t seg_key32(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float seg_val32(uint32_t k) { return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k); }

// lookup2f[p][i] = {fl32(lookup2[2p][i]), fl32(lookup2[2p + 1][i])}, i over [parity][pair row][PE].  An odd tree's last
// pair has no second branch: -inf everywhere but the exact-zero (none, none) slot, so its sums are -inf and raise no
// maximum.  Rows past the alignment (odd W, parity 1) are never staged and hold zeros.  stats[0]: the largest |entry|
// as float bits, stats[1]: the number of non-finite entries (either disables the screen's error bound, see screen_delta).
__global__ void __launch_bounds__(256) k_build_lookup2f(const double* __restrict__ lookup2, uint32_t W, uint32_t B,
                                                        float2* __restrict__ lookup2f, uint32_t p0,
                                                        uint32_t* __restrict__ stats) {
  const uint32_t p = p0 + blockIdx.y, Wh = (W + 1) / 2, n = 2 * Wh * PE;
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  float amax = 0.f;
  uint32_t bad = 0;
  if (i < n) {
    const uint32_t par = i / (Wh * PE), rem = i - par * Wh * PE, r = rem / PE, e = rem - r * PE;
    const bool valid = 2 * r + par < W, two = 2 * p + 1 < B;
    float x = 0.f, y = 0.f;
    if (valid) {
      x = (float)lookup2[(size_t)(2 * p) * n + i];
      y = two ? (float)lookup2[(size_t)(2 * p + 1) * n + i] : (e == PE - 1 ? 0.f : -INFINITY);
      const bool fx = isfinite(x), fy = !two || isfinite(y);
      bad = (fx ? 0u : 1u) + (fy ? 0u : 1u);
      if (fx) amax = fabsf(x);
      if (two && fy) amax = fmaxf(amax, fabsf(y));
    }
    lookup2f[(size_t)p * n + i] = make_float2(x, y);
  }
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    amax = fmaxf(amax, __shfl_xor(amax, off));
    bad += (uint32_t)__shfl_xor((int)bad, off);
  }
  if ((threadIdx.x & 63) == 0) {
    if (amax > 0.f) atomicMax(&stats[0], __float_as_uint(amax));   // non-negative floats order as their bits
    if (bad) atomicAdd(&stats[1], bad);
  }
}

// ---- 16-bit screen ("16-bit screen").  The band test only compares sums of ONE read across branches, so
// every table entry may be shifted by a constant of its slot: base2[i] = the maximum over the real branches of lookup2's
// entry i, i over [parity][pair row][PE].  Relative entries are <= 0, a read's sums all lose the same C_q = sum of base2
// over its slots, and its best branches sum to a small negative number: 16-bit fixed point with quantum h holds them.
// lookup2q has, per QUAD of branches (4p .. 4p + 3) and in lookup2's own layout, four int16 per 8-byte entry --
// max(rint((entry - base2) / h), -32768) -- so the packed offsets, the staged slice and the groups stay those of
// k_preplace_pairs, and one ds_read_b64 + two packed saturating adds serve FOUR (query, branch) cells.
typedef short s4 __attribute__((ext_vector_type(4)));
constexpr int Q16_FLOOR = -32768;

// base2 and the table statistics in one pass over lookup2: thread = entry, loop over the branches.  stats as in
// k_build_lookup2f (the largest |entry| and the non-finite count of the entries rounded to fp32, so that either build
// leaves the same numbers in the context).  Rows past the alignment hold zeros.
__global__ void __launch_bounds__(256) k_build_base2(const double* __restrict__ lookup2, uint32_t W, uint32_t B,
                                                     double* __restrict__ base2, uint32_t* __restrict__ stats) {
  const uint32_t Wh = (W + 1) / 2, n = 2 * Wh * PE;
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  float amax = 0.f;
  uint32_t bad = 0;
  if (i < n) {
    const uint32_t par = i / (Wh * PE), rem = i - par * Wh * PE, r = rem / PE;
    double m = 0.0;
    if (2 * r + par < W) {
      m = -INFINITY;
#pragma unroll 8
      for (uint32_t b = 0; b < B; ++b) {
        const double v = lookup2[(size_t)b * n + i];
        const float x = (float)v;
        if (isfinite(x)) amax = fmaxf(amax, fabsf(x)); else ++bad;
        m = fmax(m, v);
      }
    }
    base2[i] = m;
  }
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    amax = fmaxf(amax, __shfl_xor(amax, off));
    bad += (uint32_t)__shfl_xor((int)bad, off);
  }
  if ((threadIdx.x & 63) == 0) {
    if (amax > 0.f) atomicMax(&stats[0], __float_as_uint(amax));
    if (bad) atomicAdd(&stats[1], bad);
  }
}

// lookup2q[p][i] = the four branches 4p .. 4p + 3 of entry i in units of h below base2[i].  h is a power of two: the
// division is exact, the only rounding is rint's (<= h / 2 per entry) and the clamp, which only raises an entry.  Phantom
// branches of the last quad hold the floor everywhere but the exact-zero (none, none) slot: their sums saturate.
__global__ void __launch_bounds__(256) k_build_lookup2q(const double* __restrict__ lookup2, const double* __restrict__ base2,
                                                        uint32_t W, uint32_t B, double inv_h, s4* __restrict__ lookup2q,
                                                        uint32_t p0) {
  const uint32_t p = p0 + blockIdx.y, Wh = (W + 1) / 2, n = 2 * Wh * PE;
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t par = i / (Wh * PE), rem = i - par * Wh * PE, r = rem / PE, e = rem - r * PE;
  s4 out = {0, 0, 0, 0};
  if (2 * r + par < W) {
    const double bs = base2[i];
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      const uint32_t b = 4 * p + k;
      double qv = e == PE - 1 ? 0.0 : (double)Q16_FLOOR;
      if (b < B) {
        const double d = rint((lookup2[(size_t)b * n + i] - bs) * inv_h);
        qv = d >= (double)Q16_FLOOR ? fmin(d, 0.0) : (double)Q16_FLOOR;   // (a NaN lands on the floor)
      }
      out[k] = (short)(int)qv;
    }
  }
  lookup2q[(size_t)p * n + i] = out;
}

// The cell types of the screening kernel: what one 8-byte table entry holds and how its sums are formed and tracked.
struct ScreenF32 {   // two branches in fp32
  using cell = f2;
  using run = float;                       // the running maximum of a segment
  static constexpr uint32_t SEGC = 32;     // entries (branch pairs) per 64-branch segment
  static constexpr bool RELATIVE = false;
  static __device__ __forceinline__ cell zero() { return cell{0.f, 0.f}; }
  static __device__ __forceinline__ cell add(cell a, cell b) { return a + b; }
  static __device__ __forceinline__ run none() { return -INFINITY; }
  static __device__ __forceinline__ run track(run m, cell s) { return fmaxf(m, fmaxf(s.x, s.y)); }
  static __device__ __forceinline__ uint32_t key(run m) { return seg_key32(m); }
};
// Four branches in 16-bit fixed point, saturating adds (v_pk_add_i16 clamp), the running maximum in 16 bits too
// (v_pk_max_i16).  Every entry is <= 0, so a partial sum never rises: a final sum above the floor was above it all the
// way and no add clamped -- it is the exact integer sum of entries none of which was clamped either (a clamped entry IS
// the floor and pins the sum there).  A sum at the floor stands for "at most the floor": clamps only raise.
struct ScreenI16 {
  using cell = s4;
  using run = s4;
  static constexpr uint32_t SEGC = 16;     // entries (branch quads) per 64-branch segment
  static constexpr bool RELATIVE = true;   // sums are relative to C_q: tile 0 gathers base2
  static __device__ __forceinline__ cell zero() { return cell{0, 0, 0, 0}; }
  static __device__ __forceinline__ cell add(cell a, cell b) { return __builtin_elementwise_add_sat(a, b); }
  static __device__ __forceinline__ run none() { return run{Q16_FLOOR, Q16_FLOOR, Q16_FLOOR, Q16_FLOOR}; }
  static __device__ __forceinline__ run track(run m, cell s) { return __builtin_elementwise_max(m, s); }
  static __device__ __forceinline__ uint32_t key(run m) {   // 1 .. 65536: order preserving, never 0
    const int v = max(max((int)m.x, (int)m.y), max((int)m.z, (int)m.w));
    return (uint32_t)(v - Q16_FLOOR) + 1u;
  }
};
__device__ __forceinline__ int seg_val16(uint32_t k) { return (int)k - 1 + Q16_FLOOR; }

// The screening pass: the item walk, slice staging, register prefetch, gather batches and priorities of
// k_preplace_pairs<false, SPR, ROWL> over BP entries' worth of branches (CELL = ScreenF32: ceil(B / 2) pairs, ScreenI16:
// ceil(B / 4) quads), sums in the cell type in the same association, no result rows: only the running maximum per query
// and 64-branch segment (CELL::SEGC entries: none straddles a segment) leaves, as a non-zero order-preserving key by
// atomicMax into seg32 [Q][segp] (cleared by the caller).  CELL::RELATIVE: the items of tile 0 first stage base2's slice
// as one more branch, gather it in fp64 through the same offsets and store cq[query] = C_q.
template <class CELL, int SPR, int ROWL>
__global__ void __launch_bounds__(GQ2, 4) k_preplace_screen(
    const typename CELL::cell* __restrict__ table, const uint16_t* __restrict__ packed,
    const uint16_t* __restrict__ tails, const uint32_t* __restrict__ win_begin,
    const uint32_t* __restrict__ win_span, const uint32_t* __restrict__ perm,
    const Group* __restrict__ groups, uint32_t W, uint32_t BP, uint32_t NP16,
    const uint32_t* __restrict__ status, uint32_t* __restrict__ seg32, uint32_t segp,
    const double* __restrict__ base2, double* __restrict__ cq) {
  using cell = typename CELL::cell;
  constexpr int TR2 = (CH + SPR) / 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];  // [TR2] rows of PE cells, ROWL bytes apart
  static_assert(ROWL % 16 == 0 && ROWL >= PROWB && ((TR2 - 1) * ROWL + PROWB) < 65536, "16-bit LDS offsets");
  __shared__ uint32_t s_maxspan;
  const uint32_t ng = status[5];
  const uint32_t NBP = choose_tile(ng, BP, gridDim.x);   // branch pairs per item
  const uint32_t ntiles = (BP + NBP - 1) / NBP;
  const int t = threadIdx.x;
  const ItemWalk iw = item_walk(ng * ntiles);
  for (uint32_t item = iw.pos; item < iw.end; item += iw.step) {
    uint32_t item_g, item_t;
    item_group_tile(item, iw.lo, iw.end, ng, ntiles, item_g, item_t);
    const Group g = groups[item_g];
    const uint32_t b0 = item_t * NBP;
    const uint32_t nb = min(NBP, BP - b0);
    __syncthreads();  // the previous item's readers of s_maxspan / the slice are done
    if (g.count == 0) continue;
    const bool active = t < (int)g.count;
    uint32_t qi = 0, begin = 0, span = 0;
    if (active) {
      qi = perm[g.start + t];
      begin = win_begin[qi];
      span = win_span[qi];
      if ((uint64_t)begin + span > W) span = 0;
    }
    if (t == 0) s_maxspan = 0;
    __syncthreads();
    {
      uint32_t m = span;
#pragma unroll
      for (int off = 32; off; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off));
      if ((t & 63) == 0) atomicMax(&s_maxspan, m);
    }
    __syncthreads();
    const uint32_t gmin = win_begin[perm[g.start]];
    const uint32_t gspread = win_begin[perm[g.start + g.count - 1]] - gmin;  // < SPR
    const uint32_t rowoff = ((begin - gmin) >> 1) * ROWL;
    const uint32_t rowoff2 = rowoff | (rowoff << 16);
    const bool mine = active && span > 0;
    uint32_t t0 = 0, t1 = 0, t2 = 0;
    if (mine && (span & 3)) {
      const uint16_t* tq = tails + (size_t)qi * 4;
      t0 = tq[0] + rowoff; t1 = tq[1] + rowoff; t2 = tq[2] + rowoff;
    }
    auto at = [&](uint32_t off) -> cell { return *reinterpret_cast<const cell*>(smem + off); };
    uint32_t cw[PW];
    if (mine) {
      const uint4* p = reinterpret_cast<const uint4*>(packed + (size_t)qi * NP16);
#pragma unroll
      for (int i = 0; i < PW / 4; ++i) {
        const uint4 v = p[i];
        cw[4 * i] = v.x + rowoff2;
        cw[4 * i + 1] = v.y + rowoff2;
        cw[4 * i + 2] = v.z + rowoff2;
        cw[4 * i + 3] = v.w + rowoff2;
      }
    } else {
#pragma unroll
      for (int i = 0; i < PW; ++i) cw[i] = 0;
    }
    const uint32_t row0 = gmin;
    const uint32_t need = min((uint32_t)TR2, (gspread >> 1) + (min((uint32_t)CH, s_maxspan) + 1) / 2);
    const uint32_t rows = (row0 < W) ? min(need, (W - row0 + 1) / 2) : 0;
    const uint32_t n2 = rows * (PE / 2);
    constexpr int PF = (TR2 * (PE / 2) + GQ2 - 1) / GQ2;
    const size_t slice0 = ((size_t)(row0 & 1u) * ((W + 1) / 2) + (row0 >> 1)) * PE;   // the slice inside one branch's rows
    auto request_at = [&](const void* first, float4 (&pfs)[PF]) {   // first: entry slice0 of a [2][ceil(W / 2)][PE] table of 8-byte entries
      const float4* src = reinterpret_cast<const float4*>(first);
#pragma unroll
      for (int u = 0; u < PF; ++u) {
        const uint32_t i = u * GQ2 + t;
        pfs[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < n2) pfs[u] = src[i];
      }
    };
    auto request = [&](uint32_t j, float4 (&pfs)[PF]) {
      request_at(table + (size_t)(b0 + j) * 2 * ((W + 1) / 2) * PE + slice0, pfs);
    };
    auto stage = [&](const float4 (&pfs)[PF]) {
#pragma unroll
      for (int u = 0; u < PF; ++u) {
        const uint32_t i = u * GQ2 + t;   // 16-byte index in the compact [rows][PE / 2] slice
        if (i < n2) {
          if (ROWL == PROWB) {
            reinterpret_cast<float4*>(smem)[i] = pfs[u];
          } else {
            const uint32_t r = i / (PE / 2), c2 = i - r * (PE / 2);
            *reinterpret_cast<float4*>(smem + r * ROWL + c2 * 16) = pfs[u];
          }
        }
      }
    };
    typename CELL::run segm = CELL::none();
    auto gather = [&](uint32_t j) {
      if (!mine) return;
      cell sum = CELL::zero();
#pragma unroll
      for (int i = 0; i < PW; ++i) asm volatile("" : "+v"(cw[i]));   // keep the extracted addresses out of VGPRs (k_preplace_pairs)
      constexpr int WPB = PP_WPB, NBATCH = PW / WPB;
      cell rb[2][WPB * 2];
      auto issue = [&](int bt) {
#pragma unroll
        for (int w = 0; w < WPB; ++w) {
          const uint32_t v = cw[bt * WPB + w];
          rb[bt & 1][2 * w] = at(v & 0xffffu);
          rb[bt & 1][2 * w + 1] = at(v >> 16);
        }
      };
      issue(0);
#pragma unroll
      for (int bt = 0; bt < NBATCH; ++bt) {
        gather_prio<NBATCH>(bt);
        if (bt + 1 < NBATCH) issue(bt + 1);
#pragma unroll
        for (int w = 0; w < WPB; ++w) {
          const cell s1 = CELL::add(rb[bt & 1][2 * w], rb[bt & 1][2 * w + 1]);  // (a0+a1) + (a2+a3), every branch of the entry
          sum = CELL::add(sum, s1);
        }
      }
      if (span & 3) {  // singles of the window tail, in order
        sum = CELL::add(sum, at(t0));
        sum = CELL::add(sum, at(t1));
        sum = CELL::add(sum, at(t2));
      }
      segm = CELL::track(segm, sum);
      const uint32_t bp = b0 + j;
      if ((bp & (CELL::SEGC - 1u)) == CELL::SEGC - 1u || j + 1 == nb) {
        atomicMax(&seg32[(size_t)qi * segp + bp / CELL::SEGC], CELL::key(segm));
        segm = CELL::none();
      }
    };
    float4 pf[PF];
    if (CELL::RELATIVE && item_t == 0) {   // C_q, once per read: base2 is laid out as one branch of lookup2
      request_at(base2 + slice0, pf);
      stage(pf);
      __syncthreads();
      if (mine) {
        auto at64 = [&](uint32_t off) -> double { return *reinterpret_cast<const double*>(smem + off); };
        double c = 0.0;
#pragma unroll   // (fully: a dynamic index would move cw[] from registers to scratch)
        for (int i = 0; i < PW; ++i) c += at64(cw[i] & 0xffffu) + at64(cw[i] >> 16);
        if (span & 3) c += at64(t0) + at64(t1) + at64(t2);
        cq[qi] = c;
      }
    }
    request(0, pf);
    for (uint32_t j = 0; j < nb; ++j) {
      __syncthreads();  // previous consumers of the slice are done
      stage(pf);
      __syncthreads();
      if (j + 1 < nb) request(j + 1, pf);
      gather(j);
    }
  }  // work items
}

// Band test of the screen, one thread per query of the pair path (qkeys[q] < KB: class 0; the others keep full rows
// from the generic kernel and all-zero keys).  r = the fp32 row maximum; segment s is INCLUDED when
// seg32[s] >= r - band, band = band_t + 2 delta: with |seg32 - exact segment maximum| <= delta an excluded segment's exact
// maximum lies more than band_t below the exact row maximum, so the selection never reads it, and the segment of the
// exact maximum is always included.  An excluded segment gets the key of seg32 + delta in segmax -- finite, not 0,
// below the selection's bands, so its masks come out as from the full table -- an included one stays 0 for the exact
// pass's SegTrack.  Every included (query, segment) cell is counted under the key s * KB + the query's sort key
// (ccnt; the old value is its rank among equal keys, as in k_count_keys) for the cell sort.  mask[q]: the included
// segments (0: not a query of the screen), *n_incl += their number.
// I16 (the 16-bit screen): the keys are integers in units of h below C_q = cq[q], and the comparison is made in those
// units: included when seg >= r - band_i, band_i = ceil((band_t + 2 delta) / h).  With the exact maximum of a segment
// <= C_q + h seg + delta always, and >= C_q + h seg - delta where seg is above the floor, an excluded segment lies
// more than band_t below the exact row maximum; its key is that of the upper bound C_q + h seg + delta.  A read whose
// row maximum is the floor cannot be screened: every segment equals r, the comparison includes them all.
template <bool I16>
__global__ void __launch_bounds__(256) k_screen_band(const uint32_t* __restrict__ seg32, uint32_t Q, uint32_t nseg,
                                                     uint32_t seg32p, double band, double delta,
                                                     const uint32_t* __restrict__ qkeys, uint32_t KB,
                                                     unsigned long long* __restrict__ segmax, uint32_t segp,
                                                     uint32_t* __restrict__ ccnt, uint32_t* __restrict__ rank,
                                                     unsigned long long* __restrict__ mask,
                                                     unsigned long long* __restrict__ n_incl,
                                                     const double* __restrict__ cq, double h, int band_i) {
  const uint32_t q = blockIdx.x * 256 + threadIdx.x;
  uint32_t cnt = 0;
  if (q < Q) {
    const uint32_t* row = seg32 + (size_t)q * seg32p;
    const uint32_t qk = qkeys[q];
    float r = -INFINITY;
    uint32_t rk = 0;
    bool all = qk < KB;
    for (uint32_t s = 0; s < nseg; ++s) {
      const uint32_t k = row[s];
      if (!k) all = false;
      else if (I16) rk = max(rk, k);
      else r = fmaxf(r, seg_val32(k));
    }
    unsigned long long m = 0;
    if (all) {   // every segment has its key: a query the screening kernel served
      const double lo = (double)r - band, c = I16 ? cq[q] : 0.0;
      const int lo_i = I16 ? seg_val16(rk) - band_i : 0;
      for (uint32_t s = 0; s < nseg; ++s) {
        const double v = I16 ? c + h * (double)seg_val16(row[s]) : (double)seg_val32(row[s]);
        if (I16 ? seg_val16(row[s]) >= lo_i : v >= lo) {
          m |= 1ull << s;
          if (ccnt) rank[(size_t)q * seg32p + s] = atomicAdd(&ccnt[s * KB + qk], 1u);
        } else if (segmax) {
          segmax[(size_t)q * segp + s] = seg_key(v + delta);
        }
      }
    }
    mask[q] = m;
    cnt = (uint32_t)__popcll(m);
  }
#pragma unroll
  for (int off = 32; off; off >>= 1) cnt += (uint32_t)__shfl_xor((int)cnt, off);
  if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(n_incl, (unsigned long long)cnt);
}

// the cells into sorted order (k_scatter_sorted for cells): offs = the scanned counts, perm[pos] = the cell's QUERY
__global__ void __launch_bounds__(256) k_scatter_cells(const unsigned long long* __restrict__ mask,
                                                       const uint32_t* __restrict__ qkeys, const uint32_t* __restrict__ rank,
                                                       const uint32_t* __restrict__ offs, uint32_t Q, uint32_t seg32p,
                                                       uint32_t KB, uint32_t ncell, uint32_t* __restrict__ sorted_keys,
                                                       uint32_t* __restrict__ perm) {
  const uint32_t q = blockIdx.x * 256 + threadIdx.x;
  if (q >= Q) return;
  unsigned long long m = mask[q];
  const uint32_t qk = qkeys[q];
  while (m) {
    const uint32_t s = (uint32_t)__ffsll((long long)m) - 1u;
    m &= m - 1;
    const uint32_t key = s * KB + qk, pos = offs[key] + rank[(size_t)q * seg32p + s];
    if (pos < ncell) {
      sorted_keys[pos] = key;
      perm[pos] = q;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Single-site fast path (20 states): the machinery of k_preplace_pairs -- per-site LDS offsets
// precomputed once per chunk of queries (16 bit each), 1024-query groups, one workgroup per CU,
// register prefetch of the next slice, persistent grid -- over the ordinary [W][24] table.  Sums in
// the reference's order: ((a0+a1)+(a2+a3)) per group of four sites, then the singles.
// ---------------------------------------------------------------------------------------------
constexpr int CHS = 128;              // sites per chunk
constexpr int PWS = CHS / 2;          // packed words per chunk (two 16-bit offsets each)
constexpr int TROWS_S = CHS + SPREAD; // table rows staged per (branch, chunk)

template <int NCOLS>
__global__ void __launch_bounds__(256) k_pack_sites(const uint8_t* __restrict__ codes,
                                                    const uint32_t* __restrict__ win_begin,
                                                    const uint32_t* __restrict__ win_span, uint32_t Q,
                                                    uint32_t W, uint32_t cstride, uint32_t crel,
                                                    uint32_t span_bound, uint32_t NP16,
                                                    uint16_t* __restrict__ packed,
                                                    uint16_t* __restrict__ tails,
                                                    uint32_t* __restrict__ keys, uint32_t K,
                                                    uint32_t* __restrict__ status) {
  const uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (q >= Q) return;
  const uint32_t begin = win_begin[q];
  uint32_t span = win_span[q];
  const uint32_t cmax = min(span_bound, crel ? cstride : 0xffffffffu);
  if (lane == 0) validate_window(q, begin, span, W, cmax, status);
  if ((uint64_t)begin + span > W || span > cmax) span = 0;
  const uint8_t* c = codes + (size_t)q * cstride + (crel ? 0u : begin);
  const uint32_t nsum = span & ~3u;  // sites summed in groups of four
  for (uint32_t p = lane; p < NP16; p += 64) {
    // slots past the last full group are masked by the kernel: any finite entry of the own row
    uint32_t v = 0;
    if (p < nsum) v = (p % CHS) * (NCOLS * 8) + min((uint32_t)c[p], (uint32_t)NCOLS - 1) * 8;
    packed[(size_t)q * NP16 + p] = (uint16_t)v;
  }
  if (lane < 4) {
    uint32_t v = 0;
    if (lane < (span & 3))
      v = ((nsum + lane) % CHS) * (NCOLS * 8) + min((uint32_t)c[nsum + lane], (uint32_t)NCOLS - 1) * 8;
    tails[(size_t)q * 4 + lane] = (uint16_t)v;
  }
  if (lane == 0) {
    const uint32_t key = min(begin, K - 1);
    keys[q] = key;
  }
}

template <int NCOLS, bool ACC>
__global__ void __launch_bounds__(GQ2, 4) k_preplace_sites(
    const double* __restrict__ lookup, const uint16_t* __restrict__ packed,
    const uint16_t* __restrict__ tails, const uint32_t* __restrict__ win_begin,
    const uint32_t* __restrict__ win_span, const uint32_t* __restrict__ perm,
    const Group* __restrict__ groups, uint32_t W, uint32_t B, uint32_t pitch, uint32_t NP16,
    const uint32_t* __restrict__ status, double* __restrict__ lnl,
    unsigned long long* __restrict__ segmax, uint32_t segp) {
  constexpr uint32_t ROWB = NCOLS * 8;
  extern __shared__ __attribute__((aligned(16))) char smem[];  // [TROWS_S][NCOLS] doubles, then accs
  double* accs = reinterpret_cast<double*>(smem + (size_t)TROWS_S * ROWB);  // [NB2_ACC][GQ2] / burst rows
  __shared__ uint32_t s_maxspan;
  __shared__ uint32_t s_qi[GQ2];        // query of thread t (burst write-out), ~0 = nothing to write
  constexpr uint32_t BSTR = GQ2 + 4;
  const uint32_t ng = status[5];
  const uint32_t NBP = ACC ? NB2_ACC_S : choose_tile(ng, B, gridDim.x);
  const uint32_t ntiles = (B + NBP - 1) / NBP;
  const int t = threadIdx.x;
  auto at = [&](uint32_t off) -> double { return *reinterpret_cast<const double*>(smem + off); };
  const ItemWalk iw = item_walk(ng * ntiles);
  for (uint32_t item = iw.pos; item < iw.end; item += iw.step) {
    const Group g = groups[item % ng];
    const uint32_t b0 = (item / ng) * NBP;
    const uint32_t nb = min(NBP, B - b0);
    __syncthreads();  // the previous item's readers of s_maxspan / accs / the tile are done
    SegTrack seg;
    if (g.count == 0) continue;
    const bool active = t < (int)g.count;
    uint32_t qi = 0, begin = 0, span = 0;
    if (active) {
      qi = perm[g.start + t];
      begin = win_begin[qi];
      span = win_span[qi];
      if ((uint64_t)begin + span > W) span = 0;
    }
    if (t == 0) s_maxspan = 0;
    s_qi[t] = (active && span > 0) ? qi : 0xffffffffu;
    __syncthreads();
    {   // one LDS atomic per wave, not per thread
      uint32_t m = span;
#pragma unroll
      for (int off = 32; off; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off));
      if ((t & 63) == 0) atomicMax(&s_maxspan, m);
    }
    if (ACC) for (uint32_t j = 0; j < nb; ++j) accs[j * GQ2 + t] = 0.0;
    __syncthreads();
    const uint32_t gmin = win_begin[perm[g.start]];
    const uint32_t gspread = win_begin[perm[g.start + g.count - 1]] - gmin;  // < SPREAD
    const uint32_t rowoff = (begin - gmin) * ROWB;
    const uint32_t rowoff2 = rowoff | (rowoff << 16);
    const uint32_t nchunks = ACC ? (s_maxspan + CHS - 1) / CHS : 1;
    const uint32_t nsum = span & ~3u, ntail = span & 3;
    uint32_t t0 = 0, t1 = 0, t2 = 0, tailchunk = 0xffffffffu;
    if (active && ntail) {
      const uint16_t* tq = tails + (size_t)qi * 4;
      t0 = tq[0] + rowoff; t1 = tq[1] + rowoff; t2 = tq[2] + rowoff;
      tailchunk = nsum / CHS;
    }
    for (uint32_t c = 0; c < nchunks; ++c) {
      const uint32_t cbase = c * CHS;
      const bool mine = active && cbase < span;
      // full groups of four sites of this thread inside the chunk
      const uint32_t gfull = mine ? (min(nsum, cbase + CHS) > cbase ? (min(nsum, cbase + CHS) - cbase) >> 2 : 0) : 0;
      uint32_t cw[PWS];
      if (mine) {
        const uint4* p = reinterpret_cast<const uint4*>(packed + (size_t)qi * NP16 + (size_t)c * CHS);
#pragma unroll
        for (int i = 0; i < PWS / 4; ++i) {
          const uint4 v = p[i];
          cw[4 * i] = v.x + rowoff2;
          cw[4 * i + 1] = v.y + rowoff2;
          cw[4 * i + 2] = v.z + rowoff2;
          cw[4 * i + 3] = v.w + rowoff2;
        }
      } else {
#pragma unroll
        for (int i = 0; i < PWS; ++i) cw[i] = 0;
      }
      const uint32_t row0 = gmin + cbase;
      const uint32_t need = min((uint32_t)TROWS_S, gspread + min((uint32_t)CHS, s_maxspan - cbase));
      const uint32_t rows = (row0 < W) ? min(need, W - row0) : 0;
      const uint32_t n2 = rows * (NCOLS / 2);
      constexpr int PF = (TROWS_S * (NCOLS / 2) + GQ2 - 1) / GQ2;
      double2 pf[PF];
      auto request = [&](uint32_t j) {
        const double2* src = reinterpret_cast<const double2*>(lookup + ((size_t)(b0 + j) * W + row0) * NCOLS);
#pragma unroll
        for (int u = 0; u < PF; ++u) {
          const uint32_t i = u * GQ2 + t;
          pf[u] = make_double2(0.0, 0.0);
          if (i < n2) pf[u] = src[i];
        }
      };
      request(0);
      for (uint32_t j = 0; j < nb; ++j) {
        __syncthreads();
        {
          double2* dst = reinterpret_cast<double2*>(smem);
#pragma unroll
          for (int u = 0; u < PF; ++u) {
            const uint32_t i = u * GQ2 + t;
            if (i < n2) dst[i] = pf[u];
          }
        }
        __syncthreads();
        if (j + 1 < nb) request(j + 1);
        __builtin_amdgcn_sched_barrier(0);
        if (mine) {
          double sum = ACC ? accs[j * GQ2 + t] : 0.0;
#pragma unroll
          for (int i = 0; i < PWS; ++i) asm volatile("" : "+v"(cw[i]));
          constexpr int WPB = 4, NBATCH = PWS / WPB;  // 4 words = 8 sites = 2 groups per batch
          double rb[2][WPB * 2];
          auto issue = [&](int bt) {
#pragma unroll
            for (int w = 0; w < WPB; ++w) {
              const uint32_t v = cw[bt * WPB + w];
              rb[bt & 1][2 * w] = at(v & 0xffffu);
              rb[bt & 1][2 * w + 1] = at(v >> 16);
            }
          };
          issue(0);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int bt = 0; bt < NBATCH; ++bt) {
            gather_prio<NBATCH>(bt);
            if (bt + 1 < NBATCH) issue(bt + 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int gq = 0; gq < 2; ++gq) {
              const double* v = &rb[bt & 1][gq * 4];
              double s1 = v[0] + v[1];
              const double s2 = v[2] + v[3];
              s1 += s2;
              sum += ((uint32_t)(bt * 2 + gq) < gfull) ? s1 : 0.0;
            }
            __builtin_amdgcn_sched_barrier(0);
          }
          if (c == tailchunk) {  // singles of the window tail, in order
            sum += at(t0);
            if (ntail > 1) sum += at(t1);
            if (ntail > 2) sum += at(t2);
          }
          if (ACC) {
            accs[j * GQ2 + t] = sum;
          } else {
            accs[(j & 7u) * BSTR + t] = sum;
            if (segmax) seg.add(segmax, segp, qi, b0 + j, j + 1 == nb, sum);
          }
        }
        if (!ACC && ((j & 7u) == 7u || j + 1 == nb)) {
          // bursts of 8 branches, eight lanes per query: whole 64-byte sectors (see k_preplace_pairs)
          __builtin_amdgcn_wave_barrier();
          const uint32_t lane = (uint32_t)t & 63u, wbase = (uint32_t)t & ~63u, col = lane & 7u;
          const uint32_t ncol = (j & 7u) + 1u, bcol = b0 + (j & ~7u) + col;
#pragma unroll
          for (uint32_t k = 0; k < 8; ++k) {
            const uint32_t tq = wbase + k * 8 + (lane >> 3);
            const uint32_t q = s_qi[tq];
            if (q != 0xffffffffu && col < ncol) lnl[(size_t)q * pitch + bcol] = accs[col * BSTR + tq];
          }
          __builtin_amdgcn_wave_barrier();
        }
      }
    }
    if (ACC && active) {
      double* out = lnl + (size_t)qi * pitch + b0;
      for (uint32_t j = 0; j < nb; ++j) out[j] = accs[j * GQ2 + t];
    }
  }  // work items
}

}  // namespace

void launch_scan_counts(epa_ctx* ctx, uint32_t* cnt, uint32_t K, const uint32_t* tip_row, uint32_t* tip_total) {
  hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(1024), 0, ctx->stream, cnt, K, tip_row, tip_total);
}

int launch_build_lookup2(epa_ctx* ctx) {
  if (!ctx->lookup2)
    EPA_HIP(ctx, hipMalloc(&ctx->lookup2, sizeof(double) * (size_t)ctx->B * 2 * ((ctx->W + 1) / 2) * PE));
  for (uint32_t b0 = 0; b0 < ctx->B; b0 += EPA_GRID_Y)   // branch in grid.y, in slices of its limit
    hipLaunchKernelGGL(k_build_lookup2, dim3((ctx->W * PE + 255) / 256, std::min<uint32_t>(EPA_GRID_Y, ctx->B - b0)), dim3(256), 0,
                       ctx->stream, ctx->lookup, ctx->W, ctx->lookup2, b0);
  EPA_HIP(ctx, hipGetLastError());
  return EPA_OK;
}

// blocked layout: the site-pair rows of a block from its lookup rows (both relative to the block buffer)
int launch_build_lookup2_block(epa_ctx* ctx, uint32_t nb, const double* blk_lookup, double* blk_lookup2) {
  for (uint32_t r0 = 0; r0 < nb; r0 += EPA_GRID_Y)
    hipLaunchKernelGGL(k_build_lookup2, dim3((ctx->W * PE + 255) / 256, std::min<uint32_t>(EPA_GRID_Y, nb - r0)), dim3(256), 0,
                       ctx->stream, blk_lookup, ctx->W, blk_lookup2, r0);
  EPA_HIP(ctx, hipGetLastError());
  return EPA_OK;
}

int launch_build_lookup2f(epa_ctx* ctx) {
  if (ctx->lookup2f || ctx->lookup2f_refused) return EPA_OK;
  if (!ctx->lookup2) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "the fp32 pair table needs the resident site-pair table");
  const uint32_t BP = (ctx->B + 1) / 2, n = 2 * ((ctx->W + 1) / 2) * PE;
  const size_t bytes = sizeof(float2) * (size_t)BP * n;
  char* buf = nullptr;
  // Best effort, and never the last memory of the device: epa_dev_footprint does not count this table and the chunk
  // scratch is allocated after it, so it is only taken while SCREEN_RESERVE stays free behind it.
  constexpr size_t SCREEN_RESERVE = (size_t)4 << 30;
  size_t free_b = 0, total_b = 0;
  const bool room = hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b >= bytes + 16 + SCREEN_RESERVE;
  if (!room || hipMalloc(&buf, bytes + 16) != hipSuccess) {   // (the two statistics words behind the table)
    (void)hipGetLastError();       // no room for it: the context keeps the one-pass preplacement
    ctx->lookup2f_refused = true;
    return EPA_OK;
  }
  uint32_t* stats = reinterpret_cast<uint32_t*>(buf + bytes);
  EPA_HIP(ctx, hipMemsetAsync(stats, 0, 16, ctx->stream));
  for (uint32_t p0 = 0; p0 < BP; p0 += EPA_GRID_Y)
    hipLaunchKernelGGL(k_build_lookup2f, dim3((n + 255) / 256, std::min<uint32_t>(EPA_GRID_Y, BP - p0)), dim3(256), 0, ctx->stream,
                       ctx->lookup2, ctx->W, ctx->B, reinterpret_cast<float2*>(buf), p0, stats);
  uint32_t h[4] = {0, 0, 0, 0};
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(h, stats, 16, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) { (void)hipFree(buf); EPA_HIP(ctx, e); }
  float m;
  memcpy(&m, &h[0], 4);
  ctx->screen_M = (double)m;
  ctx->screen_nonfinite = h[1];
  ctx->screen_stats = true;
  ctx->lookup2f = reinterpret_cast<float2*>(buf);
  return EPA_OK;
}

int launch_build_lookup2q(epa_ctx* ctx, uint32_t span_bound) {
  if (ctx->lookup2q_refused) return EPA_OK;
  if (!ctx->lookup2) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "the 16-bit quad table needs the resident site-pair table");
  const uint32_t BQ = (ctx->B + 3) / 4, n = 2 * ((ctx->W + 1) / 2) * PE;
  if (!ctx->base2) {
    const size_t bytes = sizeof(double) * n + sizeof(s4) * (size_t)BQ * n;
    constexpr size_t SCREEN_RESERVE = (size_t)4 << 30;   // best effort, as launch_build_lookup2f
    size_t free_b = 0, total_b = 0;
    const bool room = hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b >= bytes + 16 + SCREEN_RESERVE;
    char *b2 = nullptr, *q = nullptr;
    if (!room || hipMalloc(&b2, sizeof(double) * n + 16) != hipSuccess || hipMalloc(&q, sizeof(s4) * (size_t)BQ * n) != hipSuccess) {
      (void)hipGetLastError();       // no room for them: the context keeps the fp32 screen
      if (b2) (void)hipFree(b2);
      ctx->lookup2q_refused = true;
      return EPA_OK;
    }
    uint32_t* stats = reinterpret_cast<uint32_t*>(b2 + sizeof(double) * n);   // (the two statistics words behind base2)
    uint32_t hs[4] = {0, 0, 0, 0};
    hipError_t e = hipMemsetAsync(stats, 0, 16, ctx->stream);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(k_build_base2, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, (const double*)ctx->lookup2, ctx->W, ctx->B,
                         reinterpret_cast<double*>(b2), stats);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(hs, stats, 16, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { (void)hipFree(b2); (void)hipFree(q); EPA_HIP(ctx, e); }
    float m;
    memcpy(&m, &hs[0], 4);
    ctx->screen_M = (double)m;
    ctx->screen_nonfinite = hs[1];
    ctx->screen_stats = true;
    ctx->base2 = reinterpret_cast<double*>(b2);
    ctx->lookup2q = q;
    ctx->lookup2q_h = 0.0;
  }
  double h = 0.0;
  if (epa_screen16_delta(ctx, span_bound, &h) < 0.0 || h == ctx->lookup2q_h) return EPA_OK;
  // another quantum than the table's: no chunk of the other bank may still be reading it
  if (ctx->lookup2q_h != 0.0) EPA_HIP(ctx, hipDeviceSynchronize());
  for (uint32_t p0 = 0; p0 < BQ; p0 += EPA_GRID_Y)
    hipLaunchKernelGGL(k_build_lookup2q, dim3((n + 255) / 256, std::min<uint32_t>(EPA_GRID_Y, BQ - p0)), dim3(256), 0, ctx->stream,
                       (const double*)ctx->lookup2, (const double*)ctx->base2, ctx->W, ctx->B, 1.0 / h, reinterpret_cast<s4*>(ctx->lookup2q), p0);
  EPA_HIP(ctx, hipGetLastError());
  EPA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->lookup2q_h = h;
  return EPA_OK;
}

double epa_screen16_delta(const epa_ctx* ctx, uint32_t span_bound, double* h_out) {
  if (!ctx->screen_stats || ctx->screen_nonfinite) return -1.0;
  const double n = 2.0 * (span_bound >> 2) + 3.0;   // pair entries of the full quads + the tail singles
  const double cq_err = (n + 2.0) * n * ctx->screen_M * 0x1p-53;
  double h = 0.5;
  while (h > 0x1p-40 && 0.5 * n * h + cq_err > 1.0) h *= 0.5;
  h = ldexp(h, -std::min(std::max(ctx->opt.preplace_screen_i16_shift, 0), 20));
  *h_out = h;
  const double delta = (0.5 * n * h + cq_err) * (double)std::max(ctx->opt.preplace_screen_scale, 1);
  return delta <= 1.0 ? delta : -1.0;
}

double epa_screen_delta(const epa_ctx* ctx, uint32_t span_bound) {
  if (!ctx->screen_stats || ctx->screen_nonfinite) return -1.0;
  const double u = 0x1p-24, n = 2.0 * (span_bound >> 2) + 3.0;   // pair entries of the full quads + the tail singles
  const double delta = 2.0 * (n + 1.0) * u * n * ctx->screen_M * (double)std::max(ctx->opt.preplace_screen_scale, 1);
  return delta <= 1.0 ? delta : -1.0;
}

int launch_preplace(epa_ctx* ctx, const uint8_t* d_codes, const uint32_t* d_begin, const uint32_t* d_span, uint32_t Q,
                    const PreTable& t, uint32_t max_span, const uint32_t** d_status, PreScreenProbe* probe) {
  double* const d_lnl = t.lnl;
  const uint32_t pitch = t.pitch, segp = t.segp;
  unsigned long long* const segmax = t.segmax;
  const bool blocked = ctx->lookup_blocks;
  const bool pairs = ctx->s == 4 && (ctx->lookup2 || blocked) && !ctx->opt.preplace_generic;
  const bool sites = ctx->s == 20 && ctx->ncols == 24 && !ctx->opt.preplace_generic;
  const uint32_t crel = ctx->code_stride ? 1u : 0u, cstride = crel ? ctx->code_stride : ctx->W;
  const uint32_t n_buckets = (ctx->W + SPREAD - 1) / SPREAD;
  const uint32_t Wp = n_buckets * SPREAD;  // key space of one (class, parity) block
  const uint32_t n_blocks = pairs ? 4 : 1, class_blocks = pairs ? 2 : 1;
  const uint32_t gq0 = (pairs || sites) ? GQ2 : GQ, gq1 = GQ;
  const uint32_t max_runs = (Q + GQ - 1) / GQ + n_blocks;
  const uint32_t max_groups = max_runs + n_blocks * n_buckets;  // + one split per SPREAD boundary
  // pair offsets per query: whole chunks of CP, enough for the longest window
  const uint32_t span_bound = (max_span == 0 || max_span > ctx->W) ? ctx->W : max_span;
  const uint32_t NP16 = pairs ? ((span_bound + 1) / 2 + CP - 1) / CP * CP
                        : sites ? (span_bound + CHS - 1) / CHS * CHS : 0;
  const uint32_t K = pairs ? n_blocks * Wp : sites ? ctx->W + 1 : 0;   // key space of the counting sort (fast paths)
  size_t temp_bytes = 0;
  (void)rocprim::radix_sort_pairs<epa_radix_cfg>(nullptr, temp_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                  (uint32_t*)nullptr, (uint32_t*)nullptr, Q, 0, 32, ctx->stream);
  uint32_t *status, *key_cnt, *iota, *sorted_keys, *perm, *keys;
  // The two-pass route (fp32 screen -> band test and cell list -> exact pass over the included cells):
  // the single-chunk pair path on the resident tables, when the table's only reader is the selection from segment
  // maxima (t.band_t) -- or a probe of the screen alone -- and the table's error bound allows it (epa_screen_delta).
  const uint32_t nseg = (ctx->B + 63) / 64, seg32p = (nseg + 7u) & ~7u;
  const uint32_t KB = 2 * Wp, n_blocks_c = 2 * nseg;      // cell keys: (segment, start parity, window start)
  const uint64_t max_cells = (uint64_t)Q * nseg;
  const uint32_t Kc = nseg * KB + 1;                      // + one counter nobody counts under: the scan leaves the total there
  const uint32_t max_runs_c = (uint32_t)std::min<uint64_t>((max_cells + GQ2 - 1) / GQ2 + n_blocks_c, 0xffffffu);
  const uint32_t max_groups_c = max_runs_c + n_blocks_c * n_buckets;
  const size_t smem_c = sizeof(uint32_t) * (2 * (n_blocks_c + 1) + 4 * (size_t)max_runs_c + 2);   // k_make_groups over the cells
  double delta = -1.0, h16 = 0.0;
  bool i16 = false;
  // Worth it only for large chunks: the band test, the cell sort (a scan, a scatter, a single-workgroup k_make_groups) and
  // the wider clear cost ~ 60 us per chunk whatever its size, and the table build ~ 5 ms once; the two passes gain ~ 0.16 ms
  // per 10^8 cells.  Measured (profiles/r9_preplace_screen_ab.txt): + 2.2 % at 100 000 reads x 1021 branches, a LOSS at 5 000
  // reads (- 2 .. - 11 %), nothing at 50 000.  Chunks below SCREEN_MIN_CELLS -- twice the break-even -- stay on one pass and
  // never build the table (option preplace_screen = 2: no size condition, for the tests).
  constexpr uint64_t SCREEN_MIN_CELLS = 80000000ull;
  const bool big = ctx->opt.preplace_screen >= 2 || probe || (uint64_t)Q * ctx->B >= SCREEN_MIN_CELLS;
  if (pairs && !blocked && nseg <= 64 && max_span != 0 && max_span <= (uint32_t)CH && ctx->opt.preplace_screen && big &&
      (probe || (segmax && t.band_t > 0.0)) && max_cells < 0x80000000ull && smem_c <= 65536) {
    // The context's first chunk that screens builds its table, once (a chunk of this size takes milliseconds itself).
    // The 16-bit screen (option preplace_screen_i16, default) is taken exactly where the fp32 screen would be -- the fp32
    // bound must hold as well -- and its own scaled bound allows it; else the fp32 screen; else one pass.  lookup2f is only
    // built when that second route (or the fp32 probe) is actually needed.
    if (probe ? probe->i16 : ctx->opt.preplace_screen_i16 != 0) {   // (a probe names its screen itself)
      const int qrc = launch_build_lookup2q(ctx, span_bound);
      if (qrc) return qrc;
      const double d16 = epa_screen16_delta(ctx, span_bound, &h16);
      if (ctx->lookup2q && d16 >= 0.0 && ctx->lookup2q_h == h16 && epa_screen_delta(ctx, span_bound) >= 0.0) {
        i16 = true;
        delta = d16;
      }
    }
    if (!i16 && !(probe && probe->i16)) {
      const int brc = launch_build_lookup2f(ctx);
      if (brc) return brc;
      if (ctx->lookup2f) delta = epa_screen_delta(ctx, span_bound);
    }
  }
  const bool screen = delta >= 0.0;
  uint32_t *seg32, *cstatus, *ccnt, *crank, *csorted, *cperm;
  unsigned long long *seg_mask, *n_incl;
  double* cq;
  Group* cgroups;
  Group* groups;
  uint16_t *packed, *tails;
  void* temp;
  auto layout = [&](Carver c) {   // SLOT_PREPLACE
    status = c.take<uint32_t>(64);   // 256 B
    key_cnt = c.take<uint32_t>(K);
    seg32 = c.take<uint32_t>(screen ? (size_t)Q * seg32p : 0);   // cleared with the status words
    n_incl = c.take<unsigned long long>(screen ? 1 : 0);
    cstatus = c.take<uint32_t>(screen ? 64 : 0);           // k_make_groups over the cells: [4], [5] = their groups
    ccnt = c.take<uint32_t>(screen ? Kc : 0);
    iota = c.take<uint32_t>(Q);      // the counting sort keeps the arrival ranks here
    sorted_keys = c.take<uint32_t>(Q);
    perm = c.take<uint32_t>(Q);
    keys = c.take<uint32_t>(Q);
    groups = c.take<Group>(max_groups);
    packed = c.take<uint16_t>((size_t)Q * NP16);
    tails = c.take<uint16_t>((pairs || sites) ? 4 * (size_t)Q : 0);
    seg_mask = c.take<unsigned long long>(screen ? Q : 0);
    cq = c.take<double>(i16 ? Q : 0);
    crank = c.take<uint32_t>(screen ? (size_t)Q * seg32p : 0);
    csorted = c.take<uint32_t>(screen ? max_cells : 0);
    cperm = c.take<uint32_t>(screen ? max_cells : 0);
    cgroups = c.take<Group>(screen ? max_groups_c : 0);
    temp = c.tail(temp_bytes);       // rocprim
    return c.off;
  };
  char* base = (char*)epa_scratch(ctx, SLOT_PREPLACE, layout(Carver{}));
  if (!base) return epa_fail(ctx, EPA_ERR_HIP, "hipMalloc(preplace scratch)");
  layout(Carver{base});
  *d_status = status;
  {   // status words + key counts, and the segment maxima when they are wanted: one kernel
    const int zr = epa_zero_async(ctx, status, (char*)iota - (char*)status, segmax, sizeof(unsigned long long) * (size_t)Q * segp);
    if (zr) return zr;
  }
  // wide slices for the pair path when a chunk puts few reads on a window start (see k_preplace_pairs)
  const bool acc = max_span == 0 || max_span > (uint32_t)CH;
  const bool wide = pairs && !acc && (uint64_t)Q * SPREAD < (uint64_t)1400 * ctx->W;   // < ~700 reads per 96-site bucket and parity
  const uint32_t rowl = (wide || acc) ? ROWL_PACKED : ROWL_NARROW;  // LDS row stride the 16-bit offsets are built for
  if (pairs) {
    constexpr uint32_t pack_grid = 64;   // workgroups per CU of the persistent packing grid
    hipLaunchKernelGGL(k_pack_pairs, dim3(std::min<uint32_t>((Q + 15) / 16, (uint32_t)ctx->n_cu * pack_grid)), dim3(256), 0, ctx->stream, d_codes, d_begin,
                       d_span, Q, ctx->W, cstride, crel, span_bound, Wp, NP16, rowl, packed, tails, keys, K, status);
  } else if (sites) {
    hipLaunchKernelGGL(k_pack_sites<24>, dim3((Q + 3) / 4), dim3(256), 0, ctx->stream, d_codes, d_begin,
                       d_span, Q, ctx->W, cstride, crel, span_bound, NP16, packed, tails, keys, K, status);
  }
  if (pairs || sites) {
    hipLaunchKernelGGL(k_count_keys, dim3((Q + 255) / 256), dim3(256), 0, ctx->stream, keys, Q, key_cnt, iota);
    launch_scan_counts(ctx, key_cnt, K);
    hipLaunchKernelGGL(k_scatter_sorted, dim3((Q + 255) / 256), dim3(256), 0, ctx->stream, keys, iota, key_cnt, Q,
                       sorted_keys, perm);
  } else {
    hipLaunchKernelGGL(k_iota, dim3((Q + 255) / 256), dim3(256), 0, ctx->stream, iota, Q);
    hipLaunchKernelGGL(k_validate, dim3((Q + 255) / 256), dim3(256), 0, ctx->stream, d_begin, d_span, Q,
                       ctx->W, std::min(span_bound, crel ? cstride : 0xffffffffu), status);
    int wbits = 1;
    while (wbits < 32 && (1ull << wbits) <= (uint64_t)ctx->W) ++wbits;
    EPA_HIP(ctx, rocprim::radix_sort_pairs<epa_radix_cfg>(temp, temp_bytes, d_begin, sorted_keys, iota, perm, Q, 0, wbits,
                                           ctx->stream));
  }
  constexpr int SPREAD_WIDE = 288;
  hipLaunchKernelGGL(k_make_groups, dim3(1), dim3(256),
                     sizeof(uint32_t) * (2 * (n_blocks + 1) + 4 * (size_t)max_runs + 2), ctx->stream,
                     sorted_keys, Q, pairs ? Wp : 0xffffffffu, n_blocks, class_blocks, gq0, gq1,
                     (uint32_t)(wide ? SPREAD_WIDE : SPREAD), max_runs, groups, max_groups, status);
  // max_span: upper bound of the window spans when the caller knows it (0 = unknown) -> acc, above
  const size_t codes_bytes = (size_t)Q * cstride;
  const uint32_t want_cls = pairs ? 1u : 0u;
  // LDS sizes and the kernels' dynamic-LDS attribute: once per call, whatever the number of blocks
  const size_t lds = sizeof(double) * ((size_t)TROWS * ctx->ncols + (acc ? (size_t)NB * GQ : 0));
  const size_t lds2 = wide ? (size_t)((CH + SPREAD_WIDE) / 2) * ROWL_PACKED + sizeof(double) * NB2_BURST * (GQ2 + 4)
                           : (size_t)TROWS2 * rowl + sizeof(double) * (acc ? NB2_ACC * GQ2 : NB2_BURST * (GQ2 + 4));  // accs / result staging
  const bool acc_s = max_span == 0 || max_span > (uint32_t)CHS;
  const size_t lds_s = (size_t)TROWS_S * 24 * 8 + sizeof(double) * (acc_s ? NB2_ACC_S * GQ2 : NB2_BURST * (GQ2 + 4));  // accs / result staging
  // The kernel instantiations of this call, picked once for the dynamic-LDS attribute and for the launches: the fast
  // path of the model (site pairs: 4 states, sites: 20; fast_acc: a multi-chunk form, which publishes no segment
  // maxima) and the generic kernel (alone, or beside the pair path for the queries with rare ambiguity codes)
  using FastKernel = decltype(&k_preplace_sites<24, false>);   // k_preplace_pairs has the same parameters
  using GenericKernel = decltype(&k_preplace<16, false>);
  FastKernel k_fast = nullptr;
  if (pairs) k_fast = wide ? k_preplace_pairs<false, SPREAD_WIDE, ROWL_PACKED> : acc ? k_preplace_pairs<true, SPREAD, ROWL_PACKED> : k_preplace_pairs<false, SPREAD, ROWL_NARROW>;
  else if (sites) k_fast = acc_s ? k_preplace_sites<24, true> : k_preplace_sites<24, false>;
  const bool fast_acc = pairs ? acc : acc_s;
  const size_t lds_fast = pairs ? lds2 : lds_s;
  const GenericKernel k_generic = sites ? nullptr : ctx->ncols == 16 ? (acc ? k_preplace<16, true> : k_preplace<16, false>) : (acc ? k_preplace<24, true> : k_preplace<24, false>);
  if (k_fast) EPA_HIP(ctx, hipFuncSetAttribute((const void*)k_fast, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_fast));
  if (k_generic) EPA_HIP(ctx, hipFuncSetAttribute((const void*)k_generic, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  // The preplacement kernels over nB branches whose tables start at lk / lk2 (the resident tables, or a block
  // buffer), table rows at lnl, segment maxima at sm: the whole tree at once, or one block of it.  Which workgroup sums
  // which (query, branch) cell follows nB (choose_tile, ntiles); a cell's summation order does not.
  auto kernels = [&](const double* lk, const double* lk2, uint32_t nB, double* lnl, unsigned long long* sm, bool fast = true) {
    // persistent grids: every resident workgroup slot of the device, work items strided over them
    if (k_fast && fast) {
      const uint32_t tile = fast_acc ? (pairs ? NB2_ACC : NB2_ACC_S) : 16;   // single chunk: choose_tile, >= 16
      const dim3 grid_f((uint32_t)std::min<uint64_t>((uint64_t)max_groups * ((nB + tile - 1) / tile), (uint64_t)ctx->n_cu));  // 1 per CU
      hipLaunchKernelGGL(k_fast, grid_f, dim3(GQ2), (uint32_t)lds_fast, ctx->stream, pairs ? lk2 : lk, (const uint16_t*)packed,
                         (const uint16_t*)tails, d_begin, d_span, perm, groups, ctx->W, nB, pitch, NP16, status, lnl,
                         fast_acc ? nullptr : sm, segp);
    }
    if (!k_generic) return;
    // generic kernel: with the pair path on it only sees the few groups of queries with rare
    // ambiguity codes -> persistent grid; as the only kernel (20 states) one workgroup per item,
    // dispatched dynamically (items differ in cost, partial groups are cheaper)
    const uint32_t ntiles = (nB + NB - 1) / NB;
    const dim3 grid(pairs ? (uint32_t)std::min<uint64_t>((uint64_t)max_groups * ntiles, (uint64_t)ctx->n_cu * (acc ? 2 : 4))
                          : max_groups * ntiles);
    hipLaunchKernelGGL(k_generic, grid, dim3(GQ), (uint32_t)lds, ctx->stream, lk, d_codes, d_begin, d_span, perm, groups, ctx->W,
                       cstride, crel, nB, pitch, codes_bytes, want_cls, status, lnl);
  };
  if (probe) probe->ran = screen;
  if (probe && !screen) return EPA_OK;
  if (screen) {
    using ScreenKernel = decltype(&k_preplace_screen<ScreenF32, SPREAD, ROWL_NARROW>);
    using Screen16Kernel = decltype(&k_preplace_screen<ScreenI16, SPREAD, ROWL_NARROW>);
    const ScreenKernel k_screen = wide ? k_preplace_screen<ScreenF32, SPREAD_WIDE, ROWL_PACKED> : k_preplace_screen<ScreenF32, SPREAD, ROWL_NARROW>;
    const Screen16Kernel k_screen16 = wide ? k_preplace_screen<ScreenI16, SPREAD_WIDE, ROWL_PACKED> : k_preplace_screen<ScreenI16, SPREAD, ROWL_NARROW>;
    const FastKernel k_exact = wide ? k_preplace_pairs<false, SPREAD_WIDE, ROWL_PACKED, true> : k_preplace_pairs<false, SPREAD, ROWL_NARROW, true>;
    const size_t lds_scr = wide ? (size_t)((CH + SPREAD_WIDE) / 2) * ROWL_PACKED : (size_t)TROWS2 * ROWL_NARROW;
    EPA_HIP(ctx, hipFuncSetAttribute(i16 ? (const void*)k_screen16 : (const void*)k_screen, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_scr));
    EPA_HIP(ctx, hipFuncSetAttribute((const void*)k_exact, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_fast));
    const uint32_t BP = i16 ? (ctx->B + 3) / 4 : (ctx->B + 1) / 2;   // table entries' worth of branches: quads or pairs
    struct Events {   // the probe's three stamps, destroyed on every way out
      hipEvent_t e[3] = {nullptr, nullptr, nullptr};
      ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    } evs;
    hipEvent_t* const ev = evs.e;
    if (probe) for (hipEvent_t& e : evs.e) EPA_HIP(ctx, hipEventCreate(&e));
    if (probe) EPA_HIP(ctx, hipEventRecord(ev[0], ctx->stream));
    else epa_timer_start(ctx, epa_t(ctx, epa_ctx::T_PREPLACE));
    const dim3 grid_s((uint32_t)std::min<uint64_t>((uint64_t)max_groups * ((BP + 15) / 16), (uint64_t)ctx->n_cu));
    if (i16)
      hipLaunchKernelGGL(k_screen16, grid_s, dim3(GQ2), (uint32_t)lds_scr, ctx->stream, (const s4*)ctx->lookup2q, (const uint16_t*)packed,
                         (const uint16_t*)tails, d_begin, d_span, perm, groups, ctx->W, BP, NP16, status, seg32, seg32p,
                         (const double*)ctx->base2, cq);
    else
      hipLaunchKernelGGL(k_screen, grid_s, dim3(GQ2), (uint32_t)lds_scr, ctx->stream, (const f2*)ctx->lookup2f, (const uint16_t*)packed,
                         (const uint16_t*)tails, d_begin, d_span, perm, groups, ctx->W, BP, NP16, status, seg32, seg32p,
                         (const double*)nullptr, (double*)nullptr);
    if (probe) EPA_HIP(ctx, hipEventRecord(ev[1], ctx->stream));
    const double band = (probe ? probe->band_t : t.band_t) + 2.0 * delta;
    const int band_i = i16 ? (int)std::min(std::ceil(band / h16), 1e9) : 0;   // the band in units of h, rounded outwards
    hipLaunchKernelGGL(i16 ? k_screen_band<true> : k_screen_band<false>, dim3((Q + 255) / 256), dim3(256), 0, ctx->stream,
                       (const uint32_t*)seg32, Q, nseg, seg32p, band, delta, (const uint32_t*)keys, KB, probe ? nullptr : segmax, segp,
                       probe ? nullptr : ccnt, crank, seg_mask, n_incl, (const double*)cq, h16, band_i);
    if (probe) {
      EPA_HIP(ctx, hipEventRecord(ev[2], ctx->stream));
      EPA_HIP(ctx, hipGetLastError());
      EPA_HIP(ctx, hipEventSynchronize(ev[2]));
      (void)hipEventElapsedTime(&probe->ms_screen, ev[0], ev[1]);
      (void)hipEventElapsedTime(&probe->ms_band, ev[1], ev[2]);
      probe->delta = delta;
      probe->h = h16;
      probe->cq = cq;
      probe->seg32 = seg32;
      probe->mask = seg_mask;
      probe->n_incl = n_incl;
      return EPA_OK;
    }
    ++ctx->screen_runs;
    // the included cells sorted by (segment, start parity, window start) and cut into groups of one segment: the
    // queries' own counting sort and grouping, over cells (ranks by atomics as there: which lane a cell lands on
    // varies, its sums do not)
    launch_scan_counts(ctx, ccnt, Kc);
    hipLaunchKernelGGL(k_scatter_cells, dim3((Q + 255) / 256), dim3(256), 0, ctx->stream, (const unsigned long long*)seg_mask,
                       (const uint32_t*)keys, (const uint32_t*)crank, (const uint32_t*)ccnt, Q, seg32p, KB, (uint32_t)max_cells, csorted, cperm);
    hipLaunchKernelGGL(k_make_groups, dim3(1), dim3(256), smem_c, ctx->stream, (const uint32_t*)csorted, (uint32_t)max_cells, Wp, n_blocks_c,
                       n_blocks_c, (uint32_t)GQ2, (uint32_t)GQ2, (uint32_t)(wide ? SPREAD_WIDE : SPREAD), max_runs_c, cgroups, max_groups_c,
                       cstatus, (const uint32_t*)(ccnt + (Kc - 1)), KB);
    // exact pass: one item per group of cells, the 64 branches of its segment; groups dealt out in turn (see the kernel)
    hipLaunchKernelGGL(k_exact, dim3(std::min<uint32_t>(max_groups_c, (uint32_t)ctx->n_cu)), dim3(GQ2), (uint32_t)lds_fast, ctx->stream,
                       (const double*)ctx->lookup2, (const uint16_t*)packed, (const uint16_t*)tails, d_begin, d_span, (const uint32_t*)cperm,
                       (const Group*)cgroups, ctx->W, ctx->B, pitch, NP16, (const uint32_t*)cstatus, d_lnl, segmax, segp);
    kernels(ctx->lookup, ctx->lookup2, ctx->B, d_lnl, segmax, false);   // the queries with rare ambiguity codes: full rows
    epa_timer_stop(ctx, epa_t(ctx, epa_ctx::T_PREPLACE));
    EPA_HIP(ctx, hipGetLastError());
    return EPA_OK;
  }
  if (!blocked) {
    epa_timer_start(ctx, epa_t(ctx, epa_ctx::T_PREPLACE));
    kernels(ctx->lookup, ctx->lookup2, ctx->B, d_lnl, segmax);
    epa_timer_stop(ctx, epa_t(ctx, epa_ctx::T_PREPLACE));
    EPA_HIP(ctx, hipGetLastError());
    return EPA_OK;
  }
  // Blocked lookup layout: the prologue above ran once (its status words are only read from here on, so a window
  // error shows whatever the number of blocks); now, block by block on this bank's stream, the tables of the block are
  // built into the bank's buffer, consumed by the same preplacement kernels, and overwritten by the next block.
  // Blocks start at multiples of 64 branches: segment maxima and 64-byte result bursts keep their alignment.
  const uint32_t blk = epa_block_branches(ctx);
  size_t off2 = 0;
  (void)epa_block_bytes(ctx->s, ctx->W, blk, &off2);
  char* buf = (char*)epa_block_buffer(ctx);
  if (!buf) return epa_fail(ctx, EPA_ERR_NO_MEMORY, "hipMalloc(lookup block buffer): " + std::to_string(epa_block_bytes(ctx->s, ctx->W, blk, nullptr)) +
                                                    " bytes needed for blocks of " + std::to_string(blk) + " branches (option lookup_block)");
  double* blk_lookup = reinterpret_cast<double*>(buf);
  double* blk_lookup2 = ctx->s == 4 ? reinterpret_cast<double*>(buf + off2) : nullptr;
  const uint32_t nblocks = (ctx->B + blk - 1) / blk;
  // events e[0] build e[1] kernels e[2] build ...: "lookup_block" and "preplace" of epa_dev_last_kernel_ms
  std::vector<hipEvent_t>& ev = ctx->blk_ev[ctx->bank];
  const bool timed = ctx->opt.timers != 0;
  ctx->blk_ev_n[ctx->bank] = 0;
  (void)epa_t(ctx, epa_ctx::T_PREPLACE);   // the bank of the last preplacement
  auto mark = [&](uint32_t i) -> int {
    if (!timed) return EPA_OK;
    while (ev.size() <= i) { hipEvent_t e = nullptr; EPA_HIP(ctx, hipEventCreate(&e)); ev.push_back(e); }
    EPA_HIP(ctx, hipEventRecord(ev[i], ctx->stream));
    return EPA_OK;
  };
  for (uint32_t k = 0; k < nblocks; ++k) {
    const uint32_t b0 = k * blk, nB = std::min(blk, ctx->B - b0);
    int rc = mark(2 * k);
    if (!rc) rc = launch_build_lookup_block(ctx, b0, nB, blk_lookup);
    if (!rc && pairs) rc = launch_build_lookup2_block(ctx, nB, blk_lookup, blk_lookup2);
    if (!rc) rc = mark(2 * k + 1);
    if (rc) return rc;
    kernels(blk_lookup, blk_lookup2, nB, d_lnl + b0, segmax ? segmax + (b0 >> 6) : nullptr);
  }
  { const int rc = mark(2 * nblocks); if (rc) return rc; }
  if (timed) ctx->blk_ev_n[ctx->bank] = 2 * nblocks + 1;
  EPA_HIP(ctx, hipGetLastError());
  return EPA_OK;
}

// what the window validation (validate_window) found: st[0] an all-gap query, st[1] a window that leaves the alignment
int preplace_window_error(epa_ctx* ctx, const uint32_t* st) {
  if (st[0])
    return epa_fail(ctx, EPA_ERR_QUERY_ALL_GAP, "Sequence " + std::to_string(st[0] & 0x7fffffffu) +
                                                    " does not appear to have any non-gap sites!");
  if (st[1])
    return epa_fail(ctx, EPA_ERR_QUERY_WIDTH, "Query sequence length not same as reference alignment!");
  return EPA_OK;
}

// reads the window-validation words written by k_make_groups (call after a stream sync)
int preplace_check_status(epa_ctx* ctx, const uint32_t* d_status) {
  uint32_t st[4];
  EPA_HIP(ctx, hipMemcpy(st, d_status, sizeof(st), hipMemcpyDeviceToHost));
  return preplace_window_error(ctx, st);
}
