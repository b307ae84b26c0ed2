// What krd.hip (epa_dev_krd), squash.hip (epa_dev_squash) and epca.hip (epa_dev_epca, the table phase only) share:
// the kernels that bring a call's entries into sorted points, run starts, M and P, the pair pass with its fixed-shape reduction, and the host code that validates a call,
// lays out its scratch and queues those kernels.  Everything sits in an unnamed namespace: each of the translation
// units compiles its own copy, with contraction off, from this one text -- which is what makes a distance of
// epa_dev_squash the bits epa_dev_krd returns for the same two entry sequences.
#pragma once

#include "epa_dev_internal.hpp"

#include <string.h>

#pragma clang fp contract(off)

namespace {

constexpr uint32_t EDPL_DIST_BIT = 0x80000000u;   // EpaTopology::cinfo (treepath.hip)
constexpr uint32_t KRD_TILE = 1024;               // ranks per workgroup of k_krd_pairs: four per lane
constexpr uint32_t KRD_MAX_S = 4096;
constexpr size_t KRD_PART_BUDGET = (size_t)32 << 20;   // bytes of tile partials per launch of k_krd_pairs
enum : int { ST_BAD_BRANCH = 0, ST_BAD_SAMPLE = 1, ST_WORDS = 64 };

// entry i -> its sort keys.  An entry whose ids are out of range is counted, gets sample S (behind every run that is
// read) and nothing is read through its ids; the call is refused after the launches
__global__ void __launch_bounds__(256) k_krd_points(const uint32_t* __restrict__ cinfo, const uint32_t* __restrict__ rank,
                                                    const epa_pair* __restrict__ pairs, const double* __restrict__ distal,
                                                    const double* __restrict__ blen, uint32_t n, uint32_t B, uint32_t S,
                                                    unsigned long long* __restrict__ key, unsigned long long* __restrict__ xbits,
                                                    uint32_t* __restrict__ idx, uint32_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  idx[i] = i;
  const uint32_t b = pairs[i].branch_id, s = pairs[i].seq_id;
  if (b >= B || s >= S) {
    atomicAdd(&status[b >= B ? ST_BAD_BRANCH : ST_BAD_SAMPLE], 1u);
    key[i] = (unsigned long long)S << 32;
    xbits[i] = 0ull;
    return;
  }
  const uint32_t info = cinfo[b];
  const double dl = distal[i];
  double x = (info & EDPL_DIST_BIT) ? dl : blen[b] - dl;
  if (x == 0.0) x = 0.0;   // -0.0 has the sign bit set and would sort last
  key[i] = ((unsigned long long)s << 32) | rank[b];
  xbits[i] = (unsigned long long)__double_as_longlong(x);
}

__global__ void __launch_bounds__(256) k_krd_gather_keys(const unsigned long long* __restrict__ key, const uint32_t* __restrict__ idx,
                                                         uint32_t n, unsigned long long* __restrict__ out) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p < n) out[p] = key[idx[p]];
}

__global__ void __launch_bounds__(256) k_krd_gather(const unsigned long long* __restrict__ xbits, const double* __restrict__ weight,
                                                    const uint32_t* __restrict__ order, uint32_t n, double* __restrict__ px,
                                                    double* __restrict__ pw) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const uint32_t e = order[p];
  px[p] = __longlong_as_double((long long)xbits[e]);
  pw[p] = weight[e];
}

// rank-ordered copies of what k_krd_pairs reads per branch
__global__ void __launch_bounds__(256) k_krd_by_rank(const uint32_t* __restrict__ rank, const uint32_t* __restrict__ size,
                                                     const double* __restrict__ blen, uint32_t B, double* __restrict__ rlen,
                                                     uint32_t* __restrict__ rsize) {
  const uint32_t b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const uint32_t r = rank[b];
  rlen[r] = blen[b];
  rsize[r] = size[b];
}

// first sorted position whose key is >= k
__device__ __forceinline__ uint32_t krd_lower_bound(const unsigned long long* __restrict__ keys, uint32_t n, unsigned long long k) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (keys[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// g = s B + r: start[g], and M_s[r] into P (scanned in place afterwards) and into M when the masses are asked for;
// g == S B: the end of the last run
__global__ void __launch_bounds__(256) k_krd_runs(const unsigned long long* __restrict__ keys, const double* __restrict__ pw,
                                                  uint32_t n, uint32_t B, uint32_t S, uint32_t* __restrict__ start,
                                                  double* __restrict__ P, double* __restrict__ M) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x, G = (size_t)S * B;
  if (g > G) return;
  if (g == G) {
    start[g] = krd_lower_bound(keys, n, (unsigned long long)S << 32);
    return;
  }
  const uint32_t s = (uint32_t)(g / B), r = (uint32_t)(g - (size_t)s * B);
  const unsigned long long k = ((unsigned long long)s << 32) | r;
  const uint32_t j0 = krd_lower_bound(keys, n, k);
  start[g] = j0;
  double m = 0.0;
  for (uint32_t j = j0; j < n && keys[j] == k; ++j) m += pw[j];
  P[g] = m;
  if (M) M[g] = m;
}

// P_s[r] = M_s[0] + ... + M_s[r] in a fixed shape: blocks of 256 ranks, a Hillis-Steele scan within the block, the
// carry of the blocks before it added to every element
__global__ void __launch_bounds__(256) k_krd_scan(double* __restrict__ P, uint32_t B) {
  __shared__ double buf[2][256];
  double* __restrict__ row = P + (size_t)blockIdx.x * B;
  const uint32_t t = threadIdx.x;
  double carry = 0.0;
  for (uint32_t r0 = 0; r0 < B; r0 += 256) {
    const uint32_t r = r0 + t;
    int cur = 0;
    buf[0][t] = r < B ? row[r] : 0.0;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
      const double v = buf[cur][t];
      buf[cur ^ 1][t] = t >= d ? buf[cur][t - d] + v : v;
      cur ^= 1;
      __syncthreads();
    }
    const double mine = carry + buf[cur][t];
    if (r < B) row[r] = mine;
    carry = carry + buf[cur][255];
    __syncthreads();
  }
}

// pair index q over a < b, rows of a one after the other: consecutive workgroups share sample a
__device__ __forceinline__ void krd_pair_of(unsigned long long q, uint32_t S, uint32_t& a, uint32_t& b) {
  // pairs before row a: a (2 S - a - 1) / 2
  const double t = 2.0 * S - 1.0;
  long long g = (long long)((t - sqrt(t * t - 8.0 * (double)q)) * 0.5);
  if (g < 0) g = 0;
  if (g > (long long)S - 2) g = (long long)S - 2;
  auto before = [&](long long r) { return (unsigned long long)(r * (2ll * S - r - 1) / 2); };
  while (g > 0 && before(g) > q) --g;
  while (g < (long long)S - 2 && before(g + 1) <= q) ++g;
  a = (uint32_t)g;
  b = (uint32_t)(q - before(g)) + a + 1;
}

// the integral of |F_a - F_b| over the branch of rank r
__device__ __forceinline__ double krd_branch(const double* __restrict__ Pa, const double* __restrict__ Pb,
                                             const uint32_t* __restrict__ sa, const uint32_t* __restrict__ sb,
                                             const double* __restrict__ px, const double* __restrict__ pw, uint32_t r, uint32_t size,
                                             double L) {
  const double Ta = Pa[r + size - 1] - Pa[r], Tb = Pb[r + size - 1] - Pb[r];
  double f = Ta - Tb, xprev = 0.0, acc = 0.0;
  uint32_t ia = sa[r], ib = sb[r];
  const uint32_t ea = sa[r + 1], eb = sb[r + 1];
  while (ia < ea || ib < eb) {
    // the next x of the merge, and every point of either sample that sits there.  The point that sets x is consumed
    // before any comparison, so the loop advances whatever the values are
    double da = 0.0, db = 0.0, x;
    if (ia < ea && (ib >= eb || !(px[ib] < px[ia]))) { x = px[ia]; da += pw[ia]; ++ia; }
    else { x = px[ib]; db += pw[ib]; ++ib; }
    while (ia < ea && px[ia] == x) { da += pw[ia]; ++ia; }
    while (ib < eb && px[ib] == x) { db += pw[ib]; ++ib; }
    const double seg = x - xprev;
    const double term = fabs(f) * seg;
    acc += term;
    const double d = da - db;
    f += d;
    xprev = x;
  }
  const double seg = L - xprev;
  const double term = fabs(f) * seg;
  acc += term;
  return acc;
}

__global__ void __launch_bounds__(256) k_krd_pairs(const double* __restrict__ P, const uint32_t* __restrict__ start,
                                                   const double* __restrict__ px, const double* __restrict__ pw,
                                                   const double* __restrict__ rlen, const uint32_t* __restrict__ rsize, uint32_t B,
                                                   uint32_t S, uint32_t n_tiles, unsigned long long q0, double* __restrict__ part) {
  __shared__ double wave_sum[4];
  const uint32_t tile = blockIdx.x % n_tiles;
  const unsigned long long ql = blockIdx.x / n_tiles;
  uint32_t a, b;
  krd_pair_of(q0 + ql, S, a, b);
  const double* __restrict__ Pa = P + (size_t)a * B;
  const double* __restrict__ Pb = P + (size_t)b * B;
  const uint32_t* __restrict__ sa = start + (size_t)a * B;
  const uint32_t* __restrict__ sb = start + (size_t)b * B;
  double acc = 0.0;
#pragma unroll 1
  for (uint32_t k = 0; k < KRD_TILE / 256; ++k) {
    const uint32_t r = tile * KRD_TILE + k * 256 + threadIdx.x;
    if (r < B) acc += krd_branch(Pa, Pb, sa, sb, px, pw, r, rsize[r], rlen[r]);
  }
  // fixed shape: a butterfly within the wave (every lane ends with the same sum), then the four waves in order
  for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[ql * n_tiles + tile] = ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
}

__global__ void __launch_bounds__(256) k_krd_finish(const double* __restrict__ part, uint32_t n_tiles, unsigned long long q0,
                                                    uint32_t n_pairs, uint32_t S, double* __restrict__ krd) {
  const uint32_t ql = blockIdx.x * 256 + threadIdx.x;
  if (ql >= n_pairs) return;
  uint32_t a, b;
  krd_pair_of(q0 + ql, S, a, b);
  double acc = 0.0;
  for (uint32_t t = 0; t < n_tiles; ++t) acc += part[(size_t)ql * n_tiles + t];
  krd[(size_t)a * S + b] = acc;
  krd[(size_t)b * S + a] = acc;
}

__global__ void __launch_bounds__(256) k_krd_masses(const double* __restrict__ P, const double* __restrict__ M,
                                                    const uint32_t* __restrict__ rank, const uint32_t* __restrict__ size, uint32_t B,
                                                    uint32_t S, double* __restrict__ edge_mass, double* __restrict__ clade_mass) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= (size_t)S * B) return;
  const uint32_t s = (uint32_t)(g / B), b = (uint32_t)(g - (size_t)s * B);
  const uint32_t r = rank[b];
  const double* __restrict__ Ps = P + (size_t)s * B;
  const double m = M[(size_t)s * B + r];
  const double T = Ps[r + size[b] - 1] - Ps[r];
  if (edge_mass) edge_mass[g] = m;
  if (clade_mass) clade_mass[g] = T + m;
}

}  // namespace

namespace {

// ---- the host side of a call: validation, scratch layout, launches

// the checks of epa_dev_krd that need no device, worded for `who` ("krd" / "squash" / "epca"); out: what the caller's last
// argument check is (a null output)
int krd_validate(epa_ctx* ctx, const std::string& who, const epa_pair* pairs, const double* distal, const double* weight, uint64_t n,
                 uint32_t S) {
  if (!ctx->topo)
    return epa_fail(ctx, EPA_ERR_INVALID_ARG, who + ": no topology is set for this context: call epa_dev_set_topology first");
  if (S == 0 || S > KRD_MAX_S)
    return epa_fail(ctx, EPA_ERR_INVALID_ARG, who + ": " + std::to_string(S) + " samples: one call takes 1 .. " + std::to_string(KRD_MAX_S));
  if (n > 0xffffffffull) return epa_fail(ctx, EPA_ERR_INVALID_ARG, who + ": more than 2^32 - 1 entries in one call");
  if (n && (!pairs || !distal || !weight)) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "null argument");
  return EPA_OK;
}

// host arrays are validated (device arrays are the caller's responsibility; ids are checked by the kernels)
int krd_validate_entries(epa_ctx* ctx, const std::string& who, const epa_pair* pairs, const double* distal, const double* weight,
                         uint64_t n, uint32_t S) {
  const bool hp = n && !epa_is_device_ptr(pairs), hd = n && !epa_is_device_ptr(distal), hw = n && !epa_is_device_ptr(weight);
  auto bad = [&](uint64_t i, const char* what) {
    return epa_fail(ctx, EPA_ERR_INVALID_ARG, who + ": entry " + std::to_string(i) + ": " + what);
  };
  for (uint64_t i = 0; i < n; ++i) {
    if (hp && pairs[i].branch_id >= ctx->B) return bad(i, "branch id out of range");
    if (hp && pairs[i].seq_id >= S) return bad(i, "sample id out of range");
    if (hd && !(std::isfinite(distal[i]) && distal[i] >= 0.0)) return bad(i, "distal length is negative or not finite");
    if (hp && hd && distal[i] > ctx->h_blen[pairs[i].branch_id]) return bad(i, "distal length beyond the branch's length");
    if (hw && !(std::isfinite(weight[i]) && weight[i] >= 0.0)) return bad(i, "weight is negative or not finite");
  }
  return EPA_OK;
}

// the scratch of the common part and the shape of its launches
struct KrdLay {
  uint32_t *status, *start, *rsize, *idx, *idx1, *order;
  double *P, *M, *rlen, *px, *pw, *part;
  unsigned long long *key, *xbits, *xs, *k1, *ks;
  void* temp;
};
struct KrdShape {
  uint32_t n32, B, S, n_tiles;
  unsigned long long n_pairs, per_launch;
  size_t sort_x, sort_k, temp_bytes;
  int kbits;
  bool masses;
  bool own_points;   // px, pw and order are carved here (epa_dev_krd); false: the caller points them at storage of its own
};

KrdShape krd_shape(epa_ctx* ctx, uint32_t n32, uint32_t S, bool masses, bool own_points) {
  KrdShape sh{};
  sh.n32 = n32; sh.B = ctx->B; sh.S = S; sh.masses = masses; sh.own_points = own_points;
  sh.n_tiles = (sh.B + KRD_TILE - 1) / KRD_TILE;
  sh.n_pairs = (unsigned long long)S * (S - 1) / 2;
  sh.per_launch = std::max<unsigned long long>(1, std::min<unsigned long long>(std::max<unsigned long long>(sh.n_pairs, 1),
                                                                               KRD_PART_BUDGET / (sizeof(double) * sh.n_tiles)));
  sh.kbits = 33;   // the key's sample field holds 0 .. S
  while (sh.kbits < 64 && (1ull << (sh.kbits - 32)) <= (unsigned long long)S) ++sh.kbits;
  (void)rocprim::radix_sort_pairs<epa_radix_cfg>(nullptr, sh.sort_x, (unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                                 (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)n32, 0, 64, ctx->stream);
  (void)rocprim::radix_sort_pairs<epa_radix_cfg>(nullptr, sh.sort_k, (unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                                 (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)n32, 0, sh.kbits, ctx->stream);
  sh.temp_bytes = std::max(sh.sort_x, sh.sort_k);
  return sh;
}

void krd_layout(Carver& c, KrdLay& l, const KrdShape& sh) {
  const size_t SB = (size_t)sh.S * sh.B;
  l.status = c.take<uint32_t>(ST_WORDS);
  l.P = c.take<double>(SB);
  l.start = c.take<uint32_t>(SB + 1);
  l.rlen = c.take<double>(sh.B);
  l.rsize = c.take<uint32_t>(sh.B);
  l.key = c.take<unsigned long long>(sh.n32);
  l.xbits = c.take<unsigned long long>(sh.n32);
  l.xs = c.take<unsigned long long>(sh.n32);
  l.k1 = c.take<unsigned long long>(sh.n32);
  l.ks = c.take<unsigned long long>(sh.n32);
  l.idx = c.take<uint32_t>(sh.n32);
  l.idx1 = c.take<uint32_t>(sh.n32);
  l.order = sh.own_points ? c.take<uint32_t>(sh.n32) : nullptr;
  l.px = sh.own_points ? c.take<double>(sh.n32) : nullptr;
  l.pw = sh.own_points ? c.take<double>(sh.n32) : nullptr;
  l.part = c.take<double>((size_t)sh.per_launch * sh.n_tiles);
  l.M = sh.masses ? c.take<double>(SB) : nullptr;
  l.temp = c.tail(sh.temp_bytes);
}

// status words cleared, the matrix zeroed, points, sorts, tables and the full pair pass into d_krd, queued on the
// context's stream; sub_timers: "krd_sort", "krd_tables" and "krd_pairs" are recorded.  pair_pass false (epa_dev_epca):
// the table phase alone -- points, the two sorts, the gather, rank-ordered lengths and sizes, run starts, M and P --
// and d_krd is not touched
int krd_launch(epa_ctx* ctx, const KrdLay& ly, const KrdShape& sh, const epa_pair* d_pairs, const double* d_distal,
               const double* d_weight, double* d_krd, bool sub_timers, bool pair_pass = true) {
  const EpaTopology& tp = *ctx->topo;
  const uint32_t n32 = sh.n32, B = sh.B, S = sh.S, n_tiles = sh.n_tiles;
  const size_t SB = (size_t)S * B;
  const dim3 ngrid((n32 + 255) / 256), bgrid((B + 255) / 256), blk(256);
  size_t sort_x = sh.sort_x, sort_k = sh.sort_k;   // rocPRIM takes the size by reference
  EPA_HIP(ctx, hipMemsetAsync(ly.status, 0, sizeof(uint32_t) * ST_WORDS, ctx->stream));
  if (pair_pass)
    EPA_HIP(ctx, hipMemsetAsync(d_krd, 0, sizeof(double) * (size_t)S * S, ctx->stream));   // the diagonal, and everything when S == 1
  if (sub_timers) epa_timer_start(ctx, epa_t(ctx, epa_ctx::T_KRD_SORT));
  if (n32) {
    hipLaunchKernelGGL(k_krd_points, ngrid, blk, 0, ctx->stream, tp.cinfo, tp.rank, d_pairs, d_distal, ctx->blen, n32, B, S, ly.key,
                       ly.xbits, ly.idx, ly.status);
    EPA_HIP(ctx, rocprim::radix_sort_pairs<epa_radix_cfg>(ly.temp, sort_x, ly.xbits, ly.xs, ly.idx, ly.idx1, (size_t)n32, 0, 64,
                                                          ctx->stream));
    hipLaunchKernelGGL(k_krd_gather_keys, ngrid, blk, 0, ctx->stream, ly.key, ly.idx1, n32, ly.k1);
    EPA_HIP(ctx, rocprim::radix_sort_pairs<epa_radix_cfg>(ly.temp, sort_k, ly.k1, ly.ks, ly.idx1, ly.order, (size_t)n32, 0, sh.kbits,
                                                          ctx->stream));
    hipLaunchKernelGGL(k_krd_gather, ngrid, blk, 0, ctx->stream, ly.xbits, d_weight, ly.order, n32, ly.px, ly.pw);
  }
  if (sub_timers) epa_timer_stop(ctx, epa_t(ctx, epa_ctx::T_KRD_SORT));
  if (sub_timers) epa_timer_start(ctx, epa_t(ctx, epa_ctx::T_KRD_TABLES));
  hipLaunchKernelGGL(k_krd_by_rank, bgrid, blk, 0, ctx->stream, tp.rank, tp.size, ctx->blen, B, ly.rlen, ly.rsize);
  hipLaunchKernelGGL(k_krd_runs, dim3((uint32_t)((SB + 1 + 255) / 256)), blk, 0, ctx->stream, ly.ks, ly.pw, n32, B, S, ly.start, ly.P,
                     ly.M);
  hipLaunchKernelGGL(k_krd_scan, dim3(S), blk, 0, ctx->stream, ly.P, B);
  if (sub_timers) epa_timer_stop(ctx, epa_t(ctx, epa_ctx::T_KRD_TABLES));
  if (!pair_pass) return EPA_OK;
  if (sub_timers) epa_timer_start(ctx, epa_t(ctx, epa_ctx::T_KRD_PAIRS));
  for (unsigned long long q0 = 0; q0 < sh.n_pairs; q0 += sh.per_launch) {
    const uint32_t np = (uint32_t)std::min<unsigned long long>(sh.per_launch, sh.n_pairs - q0);
    hipLaunchKernelGGL(k_krd_pairs, dim3(np * n_tiles), blk, 0, ctx->stream, ly.P, ly.start, ly.px, ly.pw, ly.rlen, ly.rsize, B, S,
                       n_tiles, q0, ly.part);
    hipLaunchKernelGGL(k_krd_finish, dim3((np + 255) / 256), blk, 0, ctx->stream, ly.part, n_tiles, q0, np, S, d_krd);
  }
  if (sub_timers) epa_timer_stop(ctx, epa_t(ctx, epa_ctx::T_KRD_PAIRS));
  return EPA_OK;
}

}  // namespace
