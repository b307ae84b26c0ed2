// libepa_dev.so -- duplicate queries of a chunk (include/epa_dev.h, "Duplicate queries"): exact classes of identical
// (win_begin, win_span, window codes) rows, found on the device from the rows as they arrive (full-width, compact or
// compact 4-bit), and the chunk body over one representative per class.
//
//   k_dedup_keys    64-bit key per query from its window alone
//   rocprim         stable radix sort of (key, q) on the low dedup_sort_bits key bits: rows that agree there become runs,
//                   q ascending inside a run
//   k_dedup_class   every member of a run finds the FIRST member of its run with the same window, code for code:
//                   normally the run's first member (one comparison); a member a hash collision put into the run of other
//                   rows walks on through the run (past unequal full keys without a look at the rows) until it meets an
//                   equal row -- at the latest itself.  Equality is an equivalence, so the row found is the smallest q of
//                   the class and no pass depends on another
//   rocprim         exclusive scan of the head flags (query order) -> class numbers in order of first appearance
//   k_dedup_finish  rep / first / n_unique
//   k_dedup_gather  the representatives' rows and windows, compacted, in the context's own layout and packing
//
// A row is read as aligned 16-byte words whatever its alignment: window chunk c (128 bits of window codes) is cut out of
// the two words that hold it by a funnel shift, the bits past the window's end are masked off.  Nothing outside the
// window enters a key or a comparison, and nothing is expanded to bytes first.
#include "epa_dev_internal.hpp"

#include <string.h>

#include <rocprim/device/device_scan.hpp>

#include <algorithm>

namespace {

// how the context's rows lie in memory (epa_dev_set_query_layout / _packing)
struct DedupRows {
  const uint8_t* codes;
  const uint32_t *begin, *span;
  uint32_t Q, W;
  uint32_t row_len;   // codes per row: W (full-width rows) or the compact stride
  uint32_t pitch;     // bytes per row
  uint32_t bits;      // 8 or 4 per code
  uint32_t compact;   // 1: the row holds the window only, from code 0
};

// The sort looks at the low 32 bits of the key by default (option dedup_sort_bits): four Onesweep digit passes instead of
// eight, which were two thirds of the whole pass.  Rows that collide there (about Q^2 / 2^33 pairs: one in a chunk of
// 100 000) share a run and are told apart by the full key, then by their codes.  The option may ask for the whole key:
// the sort's temp storage is sized for that
constexpr int DEDUP_SORT_BITS_MAX = 64;

enum DedupStatus : int {
  DD_ALL_GAP = 0,    // 0x80000000 | largest q with an empty window (validate_window's convention, preplace.hip)
  DD_WIDTH = 1,      // 0x80000000 | largest q whose window leaves the row or the alignment
  DD_UNIQUE = 2,     // n_unique
  DD_WORDS = 64,
};

// the window of one query as aligned words
struct RowWin {
  const uint4* w;     // the aligned 16-byte word that holds the window's first code
  uint32_t sh;        // bit offset of that code in *w (in the code order of win_chunk: a multiple of `bits`)
  uint32_t nbits;     // bits of window codes
  uint32_t nwords;    // aligned words that hold window bits
  uint32_t begin, span;
  bool bad;           // the window does not fit: read as empty (and reported)
};

__host__ __device__ __forceinline__ RowWin row_window(const DedupRows& r, uint32_t q) {
  RowWin o;
  o.begin = r.begin[q];
  o.span = r.span[q];
  o.bad = (uint64_t)o.begin + o.span > r.W || o.span > r.row_len;
  const uint32_t span = o.bad ? 0u : o.span;
  const uint32_t code0 = r.compact ? 0u : (span ? o.begin : 0u);
  // bit address of the window's first code; a 4-bit window may start on either nibble of its first byte (full-width rows)
  const uint64_t bit0 = ((uint64_t)(uintptr_t)r.codes + (uint64_t)q * r.pitch) * 8u + (uint64_t)code0 * r.bits;
  o.w = reinterpret_cast<const uint4*>((uintptr_t)((bit0 >> 7) << 4));
  o.sh = (uint32_t)(bit0 & 127u);
  o.nbits = span * r.bits;
  o.nwords = (o.sh + o.nbits + 127u) >> 7;
  return o;
}

// the two codes of a packed byte change places: code i of a 4-bit row then sits at bits [4 i, 4 i + 4) of its word, as
// code i of a one-byte row sits at [8 i, 8 i + 8)
__host__ __device__ __forceinline__ uint64_t swap_nibbles(uint64_t x) {
  return ((x & 0x0f0f0f0f0f0f0f0full) << 4) | ((x >> 4) & 0x0f0f0f0f0f0f0f0full);
}

// window bits [128 c, 128 c + 128) of a row, c < ceil(nbits / 128); bits past the window's end are zero.  Only words
// that hold window bits are loaded: each of them shares its 16 aligned bytes with a byte of the row.  (Plain integer code,
// compiled for the host as well: a stand-alone program can check it against a byte-wise extraction)
template <bool PACKED>
__host__ __device__ __forceinline__ void win_chunk(const RowWin& r, uint32_t c, uint64_t& o0, uint64_t& o1) {
  const uint4 a = r.w[c];
  uint4 b = make_uint4(0u, 0u, 0u, 0u);
  if (c + 1 < r.nwords) b = r.w[c + 1];
  uint64_t v0 = (uint64_t)a.x | ((uint64_t)a.y << 32), v1 = (uint64_t)a.z | ((uint64_t)a.w << 32);
  uint64_t v2 = (uint64_t)b.x | ((uint64_t)b.y << 32), v3 = (uint64_t)b.z | ((uint64_t)b.w << 32);
  if (PACKED) { v0 = swap_nibbles(v0); v1 = swap_nibbles(v1); v2 = swap_nibbles(v2); v3 = swap_nibbles(v3); }
  uint32_t sh = r.sh;
  if (sh >= 64u) { v0 = v1; v1 = v2; v2 = v3; sh -= 64u; }
  o0 = sh ? (v0 >> sh) | (v1 << (64u - sh)) : v0;
  o1 = sh ? (v1 >> sh) | (v2 << (64u - sh)) : v1;
  const uint32_t rem = r.nbits - 128u * c;   // >= 1
  if (rem < 64u) { o0 &= (1ull << rem) - 1ull; o1 = 0ull; }
  else if (rem < 128u) o1 &= (1ull << (rem - 64u)) - 1ull;
}

__host__ __device__ __forceinline__ uint64_t mix64(uint64_t x) {   // the finaliser of splitmix64
  x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27; x *= 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}

template <int G>
__device__ __forceinline__ uint64_t group_sum(uint64_t v) {
#pragma unroll
  for (int d = 1; d < G; d <<= 1) v += __shfl_xor(v, d, 64);
  return v;
}
template <int G>
__device__ __forceinline__ uint32_t group_or(uint32_t v) {
#pragma unroll
  for (int d = 1; d < G; d <<= 1) v |= __shfl_xor(v, d, 64);
  return v;
}

// G lanes per query (a power of two up to the wavefront): lane l takes the window chunks l, l + G, ...  The key is a sum
// of position-salted chunk hashes, so the lanes' shares add up in any order; key_mask keeps its low dedup_key_bits bits
template <int G, bool PACKED>
__global__ void __launch_bounds__(256) k_dedup_keys(const DedupRows r, uint64_t key_mask, unsigned long long* __restrict__ keys,
                                                    uint32_t* __restrict__ idx, uint32_t* __restrict__ status) {
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const uint64_t q64 = t / G;
  const uint32_t lane = (uint32_t)(t % G);
  if (q64 >= r.Q) return;   // whole groups leave together
  const uint32_t q = (uint32_t)q64;
  const RowWin w = row_window(r, q);
  const uint32_t nch = (w.nbits + 127u) >> 7;
  uint64_t acc = 0;
  for (uint32_t c = lane; c < nch; c += G) {
    uint64_t o0, o1;
    win_chunk<PACKED>(w, c, o0, o1);
    acc += mix64(o0 ^ (0x9e3779b97f4a7c15ull * (2ull * c + 1ull))) + mix64(o1 ^ (0x9e3779b97f4a7c15ull * (2ull * c + 2ull)));
  }
  acc = group_sum<G>(acc);
  if (lane) return;
  keys[q] = mix64(acc + mix64((uint64_t)w.begin | ((uint64_t)w.span << 32))) & key_mask;
  idx[q] = q;
  if (w.bad) atomicMax(&status[DD_WIDTH], 0x80000000u | q);
  else if (w.span == 0) atomicMax(&status[DD_ALL_GAP], 0x80000000u | q);
}

// are the windows of queries a and b the same, code for code?  All G lanes of a group call it with the same (a, b)
template <int G, bool PACKED>
__device__ __forceinline__ bool same_window(const DedupRows& r, const RowWin& wa, uint32_t b, uint32_t lane) {
  const RowWin wb = row_window(r, b);
  if (wa.begin != wb.begin || wa.span != wb.span) return false;   // the same for the whole group
  const uint32_t nch = (wa.nbits + 127u) >> 7;                    // (a bad window reads as empty on both sides)
  uint32_t diff = 0;
  for (uint32_t c0 = 0; c0 < nch; c0 += G) {   // the trip count is the group's: the lanes stay together for the exchange
    const uint32_t c = c0 + lane;
    if (c < nch) {
      uint64_t a0, a1, b0, b1;
      win_chunk<PACKED>(wa, c, a0, a1);
      win_chunk<PACKED>(wb, c, b0, b1);
      diff |= (a0 != b0) | (a1 != b1);
    }
    if (group_or<G>(diff)) return false;
  }
  return true;
}

// One lane group per sorted position i.  lead[q] = the smallest query of q's class; flag[q] = (lead[q] == q).
// The run of equal sorted bits (sort_mask) begins at their lower bound (binary search in the sorted keys); its members
// are in ascending q (the sort is stable), so the first member with an equal window is the class's first query
template <int G, bool PACKED>
__global__ void __launch_bounds__(256) k_dedup_class(const DedupRows r, const unsigned long long* __restrict__ skeys,
                                                     uint64_t sort_mask, const uint32_t* __restrict__ order,
                                                     uint32_t* __restrict__ lead, uint32_t* __restrict__ flag) {
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const uint64_t i64 = t / G;
  const uint32_t lane = (uint32_t)(t % G);
  if (i64 >= r.Q) return;
  const uint32_t i = (uint32_t)i64;
  const unsigned long long key = skeys[i];
  uint32_t lo = 0, hi = i;   // first position of the key's sorted bits in [0, i]
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if ((skeys[mid] & sort_mask) < (key & sort_mask)) lo = mid + 1; else hi = mid;
  }
  const uint32_t q = order[i];
  const RowWin wq = row_window(r, q);
  uint32_t found = q;
  for (uint32_t j = lo; j < i; ++j) {
    if (skeys[j] != key) continue;   // the same for the whole group
    const uint32_t m = order[j];
    if (same_window<G, PACKED>(r, wq, m, lane)) { found = m; break; }
  }
  if (lane) return;
  lead[q] = found;
  flag[q] = found == q;
  if (i == 0) flag[r.Q] = 0u;   // the scan runs over Q + 1 flags: its last output is the number of classes
}

__global__ void __launch_bounds__(256) k_dedup_finish(const uint32_t* __restrict__ lead, const uint32_t* __restrict__ uidx, uint32_t Q,
                                                      uint32_t* __restrict__ rep, uint32_t* __restrict__ first,
                                                      uint32_t* __restrict__ status) {
  const uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (q >= Q) return;
  const uint32_t l = lead[q], u = uidx[l];
  rep[q] = u;
  if (l == (uint32_t)q) first[u] = (uint32_t)q;
  if (q == 0) status[DD_UNIQUE] = uidx[Q];
}

// rows and windows of the representatives, compacted: row u of the output is row first[u] of the input, the pitch
// unchanged.  T: the widest type that divides the pitch and both base addresses.  The grid covers Q rows; the number
// of classes is read on the device (status[DD_UNIQUE]), the host has not seen it yet
template <typename T>
__global__ void __launch_bounds__(256) k_dedup_gather(const DedupRows r, const uint32_t* __restrict__ first,
                                                      const uint32_t* __restrict__ status, uint8_t* __restrict__ o_codes,
                                                      uint32_t* __restrict__ o_begin, uint32_t* __restrict__ o_span) {
  const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const uint32_t per_row = r.pitch / (uint32_t)sizeof(T);
  const uint64_t u64 = e / per_row;
  if (u64 >= status[DD_UNIQUE]) return;
  const uint32_t u = (uint32_t)u64, k = (uint32_t)(e - u64 * per_row);
  const uint32_t q = first[u];
  reinterpret_cast<T*>(o_codes)[(uint64_t)u * per_row + k] = reinterpret_cast<const T*>(r.codes)[(uint64_t)q * per_row + k];
  if (k == 0) { o_begin[u] = r.begin[q]; o_span[u] = r.span[q]; }
}

// scratch of one dedup pass (SLOT_DEDUP), written once as a function of the carver
struct DedupWork {
  uint32_t* status;
  unsigned long long *keys, *skeys;
  uint32_t *idx, *order, *lead, *flag, *uidx;
  void* temp;
  void carve(Carver& cv, uint32_t Q, size_t temp_bytes) {
    status = cv.take<uint32_t>(DD_WORDS);
    keys = cv.take<unsigned long long>(Q);
    skeys = cv.take<unsigned long long>(Q);
    idx = cv.take<uint32_t>(Q);
    order = cv.take<uint32_t>(Q);
    lead = cv.take<uint32_t>(Q);
    flag = cv.take<uint32_t>((size_t)Q + 1);
    uidx = cv.take<uint32_t>((size_t)Q + 1);
    temp = cv.tail(temp_bytes);
  }
};

// the compacted chunk (SLOT_DEDUP_ROWS) and, where the caller's rep / first live on the host, their device images
struct DedupOut {
  uint8_t* codes;
  uint32_t *begin, *span, *rep, *first;
  void carve(Carver& cv, uint32_t Q, size_t code_bytes) {
    codes = static_cast<uint8_t*>(cv.tail(align256(code_bytes + 1024)));   // slack: kernels may over-read a few words
    begin = cv.take<uint32_t>(Q);
    span = cv.take<uint32_t>(Q);
    rep = cv.take<uint32_t>(Q);
    first = cv.take<uint32_t>(Q);
  }
};

template <int G>
void launch_keys_class(epa_ctx* ctx, const DedupRows& r, uint64_t key_mask, const DedupWork& wk, bool sorted) {
  const uint32_t grid = (uint32_t)(((uint64_t)r.Q * G + 255) / 256);
  // no bits to sort on: every query in one run, in query order -- the keys are written where the sort would have put them
  unsigned long long* keys = sorted ? wk.keys : wk.skeys;
  uint32_t* idx = sorted ? wk.idx : wk.order;
  if (r.bits == 4) hipLaunchKernelGGL((k_dedup_keys<G, true>), dim3(grid), dim3(256), 0, ctx->stream, r, key_mask, keys, idx, wk.status);
  else hipLaunchKernelGGL((k_dedup_keys<G, false>), dim3(grid), dim3(256), 0, ctx->stream, r, key_mask, keys, idx, wk.status);
}
template <int G>
void launch_class(epa_ctx* ctx, const DedupRows& r, uint64_t sort_mask, const DedupWork& wk) {
  const uint32_t grid = (uint32_t)(((uint64_t)r.Q * G + 255) / 256);
  if (r.bits == 4) hipLaunchKernelGGL((k_dedup_class<G, true>), dim3(grid), dim3(256), 0, ctx->stream, r, wk.skeys, sort_mask, wk.order, wk.lead, wk.flag);
  else hipLaunchKernelGGL((k_dedup_class<G, false>), dim3(grid), dim3(256), 0, ctx->stream, r, wk.skeys, sort_mask, wk.order, wk.lead, wk.flag);
}

template <typename T>
void launch_gather(epa_ctx* ctx, const DedupRows& r, const uint32_t* d_first, const uint32_t* d_status, const DedupOut& o) {
  const uint64_t n = (uint64_t)r.Q * (r.pitch / sizeof(T));
  hipLaunchKernelGGL((k_dedup_gather<T>), dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, ctx->stream, r, d_first, d_status,
                     o.codes, o.begin, o.span);
}

// The pass on device arrays.  Queues keys -> sort -> classes -> scan -> rep / first (-> gather) on the context's stream,
// timed as "dedup", then waits for the status words: window errors (all_gap_is_error: an empty window too, as the chunk
// body would report it), *n_unique.  rep / first: host or device; *out (may be null): the compacted chunk
int dedup_pass(epa_ctx* ctx, const char* who, const uint8_t* q_codes, const uint32_t* win_begin, const uint32_t* win_span,
               uint32_t Q, uint32_t max_span, bool all_gap_is_error, uint32_t* rep, uint32_t* first, uint32_t* n_unique,
               DedupOut* out) {
  EPA_HIP(ctx, hipSetDevice(ctx->device));
  DedupRows r{};
  r.Q = Q;
  r.W = ctx->W;
  r.compact = ctx->code_stride != 0;
  r.row_len = r.compact ? ctx->code_stride : ctx->W;
  r.bits = ctx->code_packed4 ? 4u : 8u;
  r.pitch = ctx->code_packed4 ? (r.row_len + 1u) / 2u : r.row_len;
  const size_t code_bytes = (size_t)Q * r.pitch;
  // host arrays are staged in a slot of their own: the chunk body that follows stages the compacted chunk in 0 .. 2 and 10
  const bool in_dev[3] = {epa_is_device_ptr(q_codes), epa_is_device_ptr(win_begin), epa_is_device_ptr(win_span)};
  const size_t in_bytes = (in_dev[0] ? 0 : align256(code_bytes + 1024)) + (in_dev[1] ? 0 : align256(sizeof(uint32_t) * (size_t)Q)) +
                          (in_dev[2] ? 0 : align256(sizeof(uint32_t) * (size_t)Q));
  Carver in{in_bytes ? (char*)epa_scratch(ctx, SLOT_DEDUP_IN, in_bytes) : nullptr};
  if (in_bytes && !in.base) return epa_fail(ctx, EPA_ERR_HIP, std::string(who) + ": hipMalloc(query staging)");
  auto stage = [&](const void* p, bool dev, size_t bytes, size_t room) -> const void* {
    if (dev) return p;
    void* d = in.tail(room);
    return hipMemcpyAsync(d, p, bytes, hipMemcpyHostToDevice, ctx->stream) == hipSuccess ? d : nullptr;
  };
  r.codes = (const uint8_t*)stage(q_codes, in_dev[0], code_bytes, align256(code_bytes + 1024));
  r.begin = (const uint32_t*)stage(win_begin, in_dev[1], sizeof(uint32_t) * (size_t)Q, align256(sizeof(uint32_t) * (size_t)Q));
  r.span = (const uint32_t*)stage(win_span, in_dev[2], sizeof(uint32_t) * (size_t)Q, align256(sizeof(uint32_t) * (size_t)Q));
  if (!r.codes || !r.begin || !r.span) return epa_fail(ctx, EPA_ERR_HIP, std::string(who) + ": query upload failed");

  const int key_bits = ctx->opt.dedup_key_bits;
  const uint64_t key_mask = key_bits >= 64 ? ~0ull : (1ull << key_bits) - 1ull;
  const int sort_bits = std::min(key_bits, ctx->opt.dedup_sort_bits);
  const uint64_t sort_mask = sort_bits >= 64 ? ~0ull : (1ull << sort_bits) - 1ull;
  size_t sort_bytes = 0, scan_bytes = 0;
  (void)rocprim::radix_sort_pairs<epa_radix_cfg>(nullptr, sort_bytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                                 (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)Q, 0, DEDUP_SORT_BITS_MAX, ctx->stream);
  (void)rocprim::exclusive_scan(nullptr, scan_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)Q + 1,
                                rocprim::plus<uint32_t>(), ctx->stream);
  const size_t temp_bytes = std::max(sort_bytes, scan_bytes);
  DedupWork wk;
  Carver measure;
  wk.carve(measure, Q, temp_bytes);
  Carver cv{(char*)epa_scratch(ctx, SLOT_DEDUP, measure.off)};
  if (!cv.base) return epa_fail(ctx, EPA_ERR_HIP, std::string(who) + ": hipMalloc(dedup scratch)");
  wk.carve(cv, Q, temp_bytes);
  const bool rep_dev = epa_is_device_ptr(rep), first_dev = epa_is_device_ptr(first);
  DedupOut o{};
  if (out || !rep_dev || !first_dev) {
    Carver m2;
    o.carve(m2, Q, out ? code_bytes : 0);
    Carver c2{(char*)epa_scratch(ctx, SLOT_DEDUP_ROWS, m2.off)};
    if (!c2.base) return epa_fail(ctx, EPA_ERR_HIP, std::string(who) + ": hipMalloc(compacted chunk)");
    o.carve(c2, Q, out ? code_bytes : 0);
  }
  uint32_t* d_rep = rep_dev ? rep : o.rep;
  uint32_t* d_first = first_dev ? first : o.first;

  // lanes per query: enough for the longest window the layout (or the caller's bound) allows, one 128-bit chunk each
  uint32_t bound = r.row_len;
  if (max_span && max_span < bound) bound = max_span;
  const uint32_t chunks = std::max<uint64_t>(1, ((uint64_t)bound * r.bits + 127) / 128);
  int G = 1;
  while (G < 64 && (uint32_t)G < chunks) G <<= 1;

  EvTimer& tm = epa_t(ctx, epa_ctx::T_DEDUP);
  epa_timer_start(ctx, tm);
  int rc = epa_zero_async(ctx, wk.status, sizeof(uint32_t) * DD_WORDS);
  if (rc) return rc;
  const bool sorted = sort_bits > 0;
  switch (G) {
    case 1: launch_keys_class<1>(ctx, r, key_mask, wk, sorted); break;
    case 2: launch_keys_class<2>(ctx, r, key_mask, wk, sorted); break;
    case 4: launch_keys_class<4>(ctx, r, key_mask, wk, sorted); break;
    case 8: launch_keys_class<8>(ctx, r, key_mask, wk, sorted); break;
    case 16: launch_keys_class<16>(ctx, r, key_mask, wk, sorted); break;
    case 32: launch_keys_class<32>(ctx, r, key_mask, wk, sorted); break;
    default: launch_keys_class<64>(ctx, r, key_mask, wk, sorted); break;
  }
  EPA_HIP(ctx, hipGetLastError());
  if (sorted)
    EPA_HIP(ctx, rocprim::radix_sort_pairs<epa_radix_cfg>(wk.temp, sort_bytes, wk.keys, wk.skeys, wk.idx, wk.order, (size_t)Q, 0,
                                                          (unsigned)sort_bits, ctx->stream));
  switch (G) {
    case 1: launch_class<1>(ctx, r, sort_mask, wk); break;
    case 2: launch_class<2>(ctx, r, sort_mask, wk); break;
    case 4: launch_class<4>(ctx, r, sort_mask, wk); break;
    case 8: launch_class<8>(ctx, r, sort_mask, wk); break;
    case 16: launch_class<16>(ctx, r, sort_mask, wk); break;
    case 32: launch_class<32>(ctx, r, sort_mask, wk); break;
    default: launch_class<64>(ctx, r, sort_mask, wk); break;
  }
  EPA_HIP(ctx, hipGetLastError());
  EPA_HIP(ctx, rocprim::exclusive_scan(wk.temp, scan_bytes, wk.flag, wk.uidx, 0u, (size_t)Q + 1, rocprim::plus<uint32_t>(), ctx->stream));
  hipLaunchKernelGGL(k_dedup_finish, dim3((uint32_t)(((uint64_t)Q + 255) / 256)), dim3(256), 0, ctx->stream, wk.lead, wk.uidx, Q, d_rep,
                     d_first, wk.status);
  EPA_HIP(ctx, hipGetLastError());
  if (out) {
    const uintptr_t al = (uintptr_t)r.codes | (uintptr_t)o.codes | r.pitch;
    if (!(al & 15u)) launch_gather<uint4>(ctx, r, d_first, wk.status, o);
    else if (!(al & 7u)) launch_gather<uint2>(ctx, r, d_first, wk.status, o);
    else if (!(al & 3u)) launch_gather<uint32_t>(ctx, r, d_first, wk.status, o);
    else if (!(al & 1u)) launch_gather<uint16_t>(ctx, r, d_first, wk.status, o);
    else launch_gather<uint8_t>(ctx, r, d_first, wk.status, o);
    EPA_HIP(ctx, hipGetLastError());
  }
  epa_timer_stop(ctx, tm);

  uint32_t st[4] = {};
  EPA_HIP(ctx, hipMemcpyAsync(st, wk.status, sizeof(st), hipMemcpyDeviceToHost, ctx->stream));
  EPA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (!all_gap_is_error) st[DD_ALL_GAP] = 0;
  rc = preplace_window_error(ctx, st);
  if (rc) return rc;
  const uint32_t U = st[DD_UNIQUE];
  *n_unique = U;
  if (!rep_dev) EPA_HIP(ctx, hipMemcpyAsync(rep, d_rep, sizeof(uint32_t) * (size_t)Q, hipMemcpyDeviceToHost, ctx->stream));
  if (!first_dev) EPA_HIP(ctx, hipMemcpyAsync(first, d_first, sizeof(uint32_t) * (size_t)U, hipMemcpyDeviceToHost, ctx->stream));
  if (!rep_dev || !first_dev) EPA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (out) *out = o;
  return EPA_OK;
}

}  // namespace

extern "C" int epa_dev_dedup_queries(epa_ctx* ctx, const uint8_t* q_codes, const uint32_t* win_begin, const uint32_t* win_span,
                                     uint32_t Q, uint32_t* rep, uint32_t* first, uint32_t* n_unique) {
  if (!ctx || !n_unique) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "dedup_queries: null argument");
  *n_unique = 0;
  if (Q == 0) return EPA_OK;
  if (!q_codes || !win_begin || !win_span || !rep || !first) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "dedup_queries: null argument");
  return dedup_pass(ctx, "dedup_queries", q_codes, win_begin, win_span, Q, 0, false, rep, first, n_unique, nullptr);
}

extern "C" int epa_dev_place_chunk_dedup(epa_ctx* ctx, const uint8_t* q_codes, const uint32_t* win_begin, const uint32_t* win_span,
                                         uint32_t Q, uint32_t max_span, double threshold, epa_pair* pairs, epa_result* results,
                                         uint64_t max_pairs, uint64_t* n_pairs, epa_thorough_stats* stats, uint32_t* rep,
                                         uint32_t* first, uint32_t* n_unique) {
  if (!ctx || !n_pairs || !n_unique) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "place_chunk_dedup: null argument");
  *n_pairs = 0;
  *n_unique = 0;
  if (stats) memset(stats, 0, sizeof(*stats));
  if (Q == 0) return EPA_OK;
  if (!q_codes || !win_begin || !win_span || !pairs || !results || !rep || !first)
    return epa_fail(ctx, EPA_ERR_INVALID_ARG, "place_chunk_dedup: null argument");
  DedupOut g{};
  int rc = dedup_pass(ctx, "place_chunk_dedup", q_codes, win_begin, win_span, Q, max_span, true, rep, first, n_unique, &g);
  if (rc) return rc;
  // the chunk body reads the compacted arrays in place (device pointers; 4-bit rows are expanded there as always)
  return epa_dev_place_chunk(ctx, g.codes, g.begin, g.span, *n_unique, max_span, threshold, pairs, results, max_pairs, n_pairs, stats);
}
