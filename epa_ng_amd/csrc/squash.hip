// Squash clustering of placement samples (epa_dev_squash; Matsen and Evans 2013, `guppy squash`, `gappa analyze squash`):
// hierarchical clustering under the Kantorovich-Rubinstein distance in which a merged cluster is the average of its
// members' mass distributions, so that its distances are recomputed on the tree.  The quantities are specified in
// include/epa_dev.h; the kernels of the initial state and the pair arithmetic are those of epa_dev_krd (krd_kernels.hpp).
//
// State on the device.  A cluster lives in a SLOT (0 .. S - 1; sample s starts in slot s, a merged cluster takes the slot
// of its smaller-id child).  A slot owns a row of D [S][S], a row of P [S][B] and a row of run starts [S][B + 1]; the run
// starts are absolute positions in the point arena (x, weight / |C|, entry index), where a cluster's points are one
// contiguous list sorted by (rank, x, sample id, entry order).  act[0 .. A) lists the active slots, in no particular order.
//   k_squash_setup        run starts in rows of B + 1, per-sample entry counts, the identity slot map
//   per merge step t:
//   k_squash_argmin_rows  one workgroup per active position i: the best (d, id_a, id_b) over the positions j > i
//   k_squash_argmin_final one workgroup: the best of the rows; records it, renames slot(a) to S + t, drops slot(b) from act
//   (the host reads the record: 24 bytes, the one read-back of the step)
//   k_squash_merge        one work item per rank: merges the two children's runs into the new list (its place is the sum
//                         of the children's run offsets), weight[e] / |C| formed from the original weight, and M of the
//                         new cluster summed along the run in list order, as k_krd_runs does
//   k_squash_copy_row     the new run starts, written beside the children's while those were read, into slot(a)'s row
//   k_krd_scan            P of the new cluster: the same kernel on one row
//   k_squash_row          THE HOT KERNEL: one workgroup per (active position, tile of KRD_TILE ranks), the new cluster as
//                         the fixed side: k_krd_pairs's lane -> rank mapping, krd_branch, butterfly and four-wave order
//   k_squash_row_finish   one work item per active position: the tile partials added in tile order, D[new][c] and D[c][new]
// A distance is therefore computed by the operations epa_dev_krd applies to the two clusters' entry sequences, in the
// same order and shape, from M and P rows formed the same way: the same bits.
// Point storage: two arenas of 2 n points.  New lists are appended; when one does not fit, the active lists (which
// partition the n entries) are copied to the front of the other arena (k_squash_compact_*) and the roles change.
// Contraction is off; there are no atomics on doubles.
#include "krd_kernels.hpp"

#include <string.h>

#include <chrono>

#pragma clang fp contract(off)

namespace {

constexpr uint32_t SQ_NONE = 0xffffffffu;

// a candidate of the argmin: the distance, (id_a << 32 | id_b) with id_a < id_b, (slot_a << 16 | slot_b)
struct SqBest {
  double d;
  unsigned long long ab;
  uint32_t slots;
  uint32_t valid;
};

// x wins over y: the smaller distance under <, then the smaller (id_a, id_b).  Whatever the values are (NaN compares
// false both ways and leaves the ids to decide), a valid candidate wins over an invalid one
__device__ __forceinline__ bool sq_better(const SqBest& x, const SqBest& y) {
  if (!x.valid) return false;
  if (!y.valid) return true;
  if (x.d < y.d) return true;
  if (y.d < x.d) return false;
  return x.ab < y.ab;
}

// fixed shape: a butterfly within the wave, then the four waves in order; the result is thread 0's
__device__ __forceinline__ SqBest sq_reduce(SqBest v, SqBest* wave_best) {
  for (int m = 32; m >= 1; m >>= 1) {
    SqBest o;
    o.d = __shfl_xor(v.d, m, 64);
    o.ab = __shfl_xor(v.ab, m, 64);
    o.slots = __shfl_xor(v.slots, m, 64);
    o.valid = __shfl_xor(v.valid, m, 64);
    if (sq_better(o, v)) v = o;
  }
  if ((threadIdx.x & 63) == 0) wave_best[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    v = wave_best[0];
    for (int w = 1; w < 4; ++w)
      if (sq_better(wave_best[w], v)) v = wave_best[w];
  }
  return v;
}

// g = s (B + 1) + r: sample s's run starts as a row of B + 1; r == 0 also: its entry count and the identity slot map
__global__ void __launch_bounds__(256) k_squash_setup(const uint32_t* __restrict__ start, uint32_t B, uint32_t S,
                                                      uint32_t* __restrict__ start2, uint32_t* __restrict__ cnt,
                                                      uint32_t* __restrict__ slot_id, uint32_t* __restrict__ act,
                                                      uint32_t* __restrict__ pos) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= (size_t)S * (B + 1)) return;
  const uint32_t s = (uint32_t)(g / (B + 1)), r = (uint32_t)(g - (size_t)s * (B + 1));
  start2[g] = start[(size_t)s * B + r];
  if (r == 0) {
    cnt[s] = start[(size_t)(s + 1) * B] - start[(size_t)s * B];
    slot_id[s] = s;
    act[s] = s;
    pos[s] = s;
  }
}

__global__ void __launch_bounds__(256) k_squash_argmin_rows(const double* __restrict__ D, uint32_t S, const uint32_t* __restrict__ act,
                                                            const uint32_t* __restrict__ slot_id, uint32_t A,
                                                            SqBest* __restrict__ rowbest) {
  __shared__ SqBest wave_best[4];
  const uint32_t i = blockIdx.x;
  const uint32_t si = act[i], idi = slot_id[si];
  const double* __restrict__ row = D + (size_t)si * S;
  SqBest v{0.0, 0ull, 0u, 0u};
  for (uint32_t j = i + 1 + threadIdx.x; j < A; j += 256) {
    const uint32_t sj = act[j], idj = slot_id[sj];
    SqBest c;
    c.d = row[sj];
    c.ab = idi < idj ? ((unsigned long long)idi << 32) | idj : ((unsigned long long)idj << 32) | idi;
    c.slots = idi < idj ? (si << 16) | sj : (sj << 16) | si;
    c.valid = 1u;
    if (sq_better(c, v)) v = c;
  }
  v = sq_reduce(v, wave_best);
  if (threadIdx.x == 0) rowbest[i] = v;
}

// the step's record, and the slot bookkeeping: slot(a) now holds cluster new_id, slot(b) leaves the active list (the last
// active position takes its place)
__global__ void __launch_bounds__(256) k_squash_argmin_final(const SqBest* __restrict__ rowbest, uint32_t A, uint32_t new_id,
                                                             uint32_t* __restrict__ slot_id, uint32_t* __restrict__ act,
                                                             uint32_t* __restrict__ pos, SqBest* __restrict__ res) {
  __shared__ SqBest wave_best[4];
  SqBest v{0.0, 0ull, 0u, 0u};
  for (uint32_t i = threadIdx.x; i < A; i += 256)
    if (sq_better(rowbest[i], v)) v = rowbest[i];
  v = sq_reduce(v, wave_best);
  if (threadIdx.x != 0) return;
  *res = v;
  if (!v.valid) return;
  const uint32_t sa = v.slots >> 16, sb = v.slots & 0xffffu;
  slot_id[sa] = new_id;
  slot_id[sb] = SQ_NONE;
  const uint32_t p = pos[sb], last = act[A - 1];
  act[p] = last;
  pos[last] = p;
}

// rank r < B: the children's runs on r merged by (x, sample id) -- each child's run is in that order already, the two
// hold different samples -- into the new list; r == B: the list's end.  The children's lists are read from the arena the
// new one is written to, at other positions.  size = |C| as a double
__global__ void __launch_bounds__(256) k_squash_merge(const uint32_t* __restrict__ sa, const uint32_t* __restrict__ sb,
                                                      const epa_pair* __restrict__ pairs, const double* __restrict__ weight,
                                                      double* px, double* pw, uint32_t* pe, uint32_t B, uint32_t new_base,
                                                      double size, uint32_t* __restrict__ new_start, double* __restrict__ Mrow) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r > B) return;
  uint32_t ia = sa[r], ib = sb[r];
  uint32_t out = new_base + (ia - sa[0]) + (ib - sb[0]);
  new_start[r] = out;
  if (r == B) return;
  const uint32_t ea = sa[r + 1], eb = sb[r + 1];
  double m = 0.0;
  while (ia < ea || ib < eb) {
    bool take_a;
    if (ib >= eb) take_a = true;
    else if (ia >= ea) take_a = false;
    else {
      const double xa = px[ia], xb = px[ib];
      take_a = xa < xb || (!(xb < xa) && pairs[pe[ia]].seq_id < pairs[pe[ib]].seq_id);
    }
    const uint32_t j = take_a ? ia++ : ib++;
    const uint32_t e = pe[j];
    const double w = weight[e] / size;
    px[out] = px[j];
    pe[out] = e;
    pw[out] = w;
    m += w;
    ++out;
  }
  Mrow[r] = m;
}

__global__ void __launch_bounds__(256) k_squash_copy_row(const uint32_t* __restrict__ src, uint32_t n, uint32_t* __restrict__ dst) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

// the new cluster (slot s_new) against the cluster at active position blockIdx.x / n_tiles: k_krd_pairs with the rows
// addressed by slot
__global__ void __launch_bounds__(256) k_squash_row(const double* __restrict__ P, const uint32_t* __restrict__ start2,
                                                    const double* __restrict__ px, const double* __restrict__ pw,
                                                    const double* __restrict__ rlen, const uint32_t* __restrict__ rsize, uint32_t B,
                                                    uint32_t n_tiles, const uint32_t* __restrict__ act, uint32_t s_new,
                                                    double* __restrict__ part) {
  __shared__ double wave_sum[4];
  const uint32_t tile = blockIdx.x % n_tiles;
  const uint32_t p = blockIdx.x / n_tiles;
  const uint32_t c = act[p];
  if (c == s_new) return;   // the whole workgroup
  const double* __restrict__ Pa = P + (size_t)s_new * B;
  const double* __restrict__ Pb = P + (size_t)c * B;
  const uint32_t* __restrict__ sa = start2 + (size_t)s_new * (B + 1);
  const uint32_t* __restrict__ sb = start2 + (size_t)c * (B + 1);
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
  if (threadIdx.x == 0) part[(size_t)p * n_tiles + tile] = ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
}

__global__ void __launch_bounds__(256) k_squash_row_finish(const double* __restrict__ part, uint32_t n_tiles,
                                                           const uint32_t* __restrict__ act, uint32_t A, uint32_t s_new, uint32_t S,
                                                           double* __restrict__ D) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= A) return;
  const uint32_t c = act[p];
  double acc = 0.0;
  if (c != s_new)
    for (uint32_t t = 0; t < n_tiles; ++t) acc += part[(size_t)p * n_tiles + t];
  D[(size_t)s_new * S + c] = acc;
  D[(size_t)c * S + s_new] = acc;
}

// compaction: the list of the cluster at active position blockIdx.y (position A: of slot `extra`, the child that has
// left the active list already) moves from old_base[slot] in the source arena to new_base[slot] in the other one ...
__global__ void __launch_bounds__(256) k_squash_compact_points(const uint32_t* __restrict__ act, uint32_t A, uint32_t extra,
                                                               const uint32_t* __restrict__ start2,
                                                               uint32_t B, const uint32_t* __restrict__ old_base,
                                                               const uint32_t* __restrict__ new_base, const double* __restrict__ px_in,
                                                               const double* __restrict__ pw_in, const uint32_t* __restrict__ pe_in,
                                                               double* __restrict__ px, double* __restrict__ pw,
                                                               uint32_t* __restrict__ pe) {
  const uint32_t c = blockIdx.y < A ? act[blockIdx.y] : extra;
  const uint32_t ob = old_base[c], nb = new_base[c], cnt = start2[(size_t)c * (B + 1) + B] - ob;
  for (uint32_t j = blockIdx.x * 256 + threadIdx.x; j < cnt; j += gridDim.x * 256) {
    px[nb + j] = px_in[ob + j];
    pw[nb + j] = pw_in[ob + j];
    pe[nb + j] = pe_in[ob + j];
  }
}
// ... and its run starts follow (a launch of its own, behind the one above that reads the old end)
__global__ void __launch_bounds__(256) k_squash_compact_starts(const uint32_t* __restrict__ act, uint32_t A, uint32_t extra,
                                                               uint32_t* __restrict__ start2, uint32_t B,
                                                               const uint32_t* __restrict__ old_base,
                                                               const uint32_t* __restrict__ new_base) {
  const uint32_t c = blockIdx.y < A ? act[blockIdx.y] : extra;
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r > B) return;
  uint32_t* row = start2 + (size_t)c * (B + 1);
  row[r] = row[r] - old_base[c] + new_base[c];
}

struct SqLay {
  double *D, *px[2], *pw[2], *part;
  uint32_t *start2, *pe[2], *slot_id, *act, *pos, *bases, *cnt;
  SqBest *rowbest, *res;
};

void squash_layout(Carver& c, SqLay& l, uint32_t S, uint32_t B, size_t cap, uint32_t n_tiles) {
  l.D = c.take<double>((size_t)S * S);
  l.start2 = c.take<uint32_t>((size_t)(S + 1) * (B + 1));   // row S: the new cluster's starts while the children's are read
  for (int k = 0; k < 2; ++k) {
    l.px[k] = c.take<double>(cap);
    l.pw[k] = c.take<double>(cap);
    l.pe[k] = c.take<uint32_t>(cap);
  }
  l.slot_id = c.take<uint32_t>(S);
  l.act = c.take<uint32_t>(S);
  l.pos = c.take<uint32_t>(S);
  l.bases = c.take<uint32_t>(2 * (size_t)S);
  l.cnt = c.take<uint32_t>(S);
  l.rowbest = c.take<SqBest>(S);
  l.res = c.take<SqBest>(S);
  l.part = c.take<double>((size_t)S * n_tiles);
}

// a small output array to the caller, on the host or on the device
template <typename T>
hipError_t squash_out(T* dst, const std::vector<T>& v) {
  if (v.empty()) return hipSuccess;
  if (epa_is_device_ptr(dst)) return hipMemcpy(dst, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice);
  memcpy(dst, v.data(), sizeof(T) * v.size());
  return hipSuccess;
}

}  // namespace

extern "C" int epa_dev_squash(epa_ctx* ctx, const epa_pair* pairs, const double* distal, const double* weight, uint64_t n, uint32_t S,
                              uint32_t* merge_a, uint32_t* merge_b, double* merge_dist, uint32_t* merge_size, double* krd) {
  if (!ctx) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "null argument");
  if (int rc = krd_validate(ctx, "squash", pairs, distal, weight, n, S)) return rc;
  if (S > 1 && (!merge_a || !merge_b || !merge_dist || !merge_size)) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "null argument");
  // the arenas hold 2 n points each and are addressed with 32 bits
  if (n > 0x7fffffffull) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "squash: more than 2^31 - 1 entries in one call");
  EPA_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = krd_validate_entries(ctx, "squash", pairs, distal, weight, n, S)) return rc;
  const uint32_t n32 = (uint32_t)n, B = ctx->B;
  const size_t cap = 2 * (size_t)n32;
  const epa_pair* d_pairs = n ? (const epa_pair*)epa_to_device(ctx, SLOT_PAIRS, pairs, sizeof(epa_pair) * n) : nullptr;
  const double* d_distal = n ? (const double*)epa_to_device(ctx, SLOT_DISTAL, distal, sizeof(double) * n) : nullptr;
  const double* d_weight = n ? (const double*)epa_to_device(ctx, SLOT_WEIGHT, weight, sizeof(double) * n) : nullptr;
  if (n && (!d_pairs || !d_distal || !d_weight)) return epa_fail(ctx, EPA_ERR_HIP, "squash input upload failed");
  // scratch: this call's state, then epa_dev_krd's layout with the sorted points in arena 0
  const KrdShape sh = krd_shape(ctx, n32, S, false, false);
  const uint32_t n_tiles = sh.n_tiles;
  SqLay sq;
  KrdLay ly;
  Carver cv;
  squash_layout(cv, sq, S, B, cap, n_tiles);
  krd_layout(cv, ly, sh);
  char* base = (char*)epa_scratch(ctx, SLOT_SQUASH, cv.off);
  if (!base) return epa_fail(ctx, EPA_ERR_HIP, "hipMalloc(squash scratch)");
  cv = Carver{base, 0};
  squash_layout(cv, sq, S, B, cap, n_tiles);
  krd_layout(cv, ly, sh);
  ly.px = sq.px[0];
  ly.pw = sq.pw[0];
  ly.order = sq.pe[0];
  const dim3 blk(256);
  const int bank = ctx->bank;
  double sums[3] = {0.0, 0.0, 0.0};
  const int step_timer[3] = {epa_ctx::T_SQUASH_ARGMIN, epa_ctx::T_SQUASH_MERGE, epa_ctx::T_SQUASH_ROW};
  auto add_ms = [&](int k) {   // the events of the step's last record are behind a synchronisation
    EvTimer& t = ctx->t_bank[bank][step_timer[k]];
    float ms = 0.f;
    if (ctx->opt.timers && t.valid && hipEventElapsedTime(&ms, t.a, t.b) == hipSuccess) sums[k] += (double)ms;
  };
  for (double& v : ctx->squash_ms) v = -1.0;

  // ---- the initial state: exactly epa_dev_krd's
  epa_timer_start(ctx, epa_t(ctx, epa_ctx::T_SQUASH));
  epa_timer_start(ctx, epa_t(ctx, epa_ctx::T_SQUASH_INIT));
  if (int rc = krd_launch(ctx, ly, sh, d_pairs, d_distal, d_weight, sq.D, false)) return rc;
  hipLaunchKernelGGL(k_squash_setup, dim3((uint32_t)(((size_t)S * (B + 1) + 255) / 256)), blk, 0, ctx->stream, ly.start, B, S, sq.start2,
                     sq.cnt, sq.slot_id, sq.act, sq.pos);
  epa_timer_stop(ctx, epa_t(ctx, epa_ctx::T_SQUASH_INIT));
  EPA_HIP(ctx, hipGetLastError());
  uint32_t status[2] = {0, 0};
  std::vector<uint32_t> cnt(2 * (size_t)S, 0u), csize(2 * (size_t)S, 1u), cbase(2 * (size_t)S, 0u);
  EPA_HIP(ctx, hipMemcpyAsync(status, ly.status, sizeof(status), hipMemcpyDeviceToHost, ctx->stream));
  EPA_HIP(ctx, hipMemcpyAsync(cnt.data(), sq.cnt, sizeof(uint32_t) * S, hipMemcpyDeviceToHost, ctx->stream));
  EPA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (status[ST_BAD_BRANCH]) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "squash: a branch id is out of range");
  if (status[ST_BAD_SAMPLE]) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "squash: a sample id is out of range");
  if (krd) EPA_HIP(ctx, hipMemcpy(krd, sq.D, sizeof(double) * (size_t)S * S, hipMemcpyDefault));
  size_t total = 0;
  for (uint32_t s = 0; s < S; ++s) { cbase[s] = (uint32_t)total; total += cnt[s]; }
  if (total != n32) return epa_fail(ctx, EPA_ERR_HIP, "squash: the per-sample entry counts do not add up");

  // ---- the loop.  The host mirrors the slot bookkeeping of k_squash_argmin_final and owns the arena
  std::vector<uint32_t> slot_id(S), act(S), pos(S), bases(2 * (size_t)S, 0u);
  for (uint32_t s = 0; s < S; ++s) slot_id[s] = act[s] = pos[s] = s;
  std::vector<uint32_t> h_a, h_b, h_size;
  std::vector<double> h_d;
  int cur = 0;
  size_t bump = n32;
  const auto loop_begin = std::chrono::steady_clock::now();
  for (uint32_t t = 0; t + 1 < S; ++t) {
    const uint32_t A = S - t, new_id = S + t;
    epa_timer_start(ctx, epa_t(ctx, epa_ctx::T_SQUASH_ARGMIN));
    hipLaunchKernelGGL(k_squash_argmin_rows, dim3(A), blk, 0, ctx->stream, sq.D, S, sq.act, sq.slot_id, A, sq.rowbest);
    hipLaunchKernelGGL(k_squash_argmin_final, dim3(1), blk, 0, ctx->stream, sq.rowbest, A, new_id, sq.slot_id, sq.act, sq.pos, sq.res + t);
    epa_timer_stop(ctx, epa_t(ctx, epa_ctx::T_SQUASH_ARGMIN));
    SqBest best{};
    EPA_HIP(ctx, hipMemcpyAsync(&best, sq.res + t, sizeof(SqBest), hipMemcpyDeviceToHost, ctx->stream));
    EPA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    add_ms(0);
    if (t) { add_ms(1); add_ms(2); }
    const uint32_t a = (uint32_t)(best.ab >> 32), b = (uint32_t)best.ab, s_a = best.slots >> 16, s_b = best.slots & 0xffffu;
    if (!best.valid || s_a >= S || s_b >= S || s_a == s_b || a >= b || slot_id[s_a] != a || slot_id[s_b] != b)
      return epa_fail(ctx, EPA_ERR_HIP, "squash: step " + std::to_string(t) + ": the device named a pair that is not active");
    slot_id[s_a] = new_id;
    slot_id[s_b] = SQ_NONE;
    {
      const uint32_t p = pos[s_b], last = act[A - 1];
      act[p] = last;
      pos[last] = p;
    }
    const uint32_t A2 = A - 1;
    cnt[new_id] = cnt[a] + cnt[b];
    csize[new_id] = csize[a] + csize[b];
    h_a.push_back(a); h_b.push_back(b); h_d.push_back(best.d); h_size.push_back(csize[new_id]);
    epa_timer_start(ctx, epa_t(ctx, epa_ctx::T_SQUASH_MERGE));
    if (bump + cnt[new_id] > cap) {
      // the children are still listed by the start rows of slots s_a and s_b; act no longer holds s_b, which is passed apart.
      // (`bases` is staged by the copy before it returns, and next written behind the next step's synchronisation)
      size_t at = 0;
      std::vector<uint32_t> movers(act.begin(), act.begin() + A2);
      movers.push_back(s_b);
      for (uint32_t s : movers) {
        const uint32_t id = s == s_a ? a : s == s_b ? b : slot_id[s];
        bases[s] = cbase[id];
        bases[S + s] = (uint32_t)at;
        cbase[id] = (uint32_t)at;
        at += cnt[id];
      }
      EPA_HIP(ctx, hipMemcpyAsync(sq.bases, bases.data(), sizeof(uint32_t) * 2 * S, hipMemcpyHostToDevice, ctx->stream));
      hipLaunchKernelGGL(k_squash_compact_points, dim3(64, A), blk, 0, ctx->stream, sq.act, A2, s_b, sq.start2, B, sq.bases,
                         sq.bases + S, sq.px[cur], sq.pw[cur], sq.pe[cur], sq.px[cur ^ 1], sq.pw[cur ^ 1], sq.pe[cur ^ 1]);
      hipLaunchKernelGGL(k_squash_compact_starts, dim3((B + 1 + 255) / 256, A), blk, 0, ctx->stream, sq.act, A2, s_b, sq.start2, B,
                         sq.bases, sq.bases + S);
      cur ^= 1;
      bump = at;
    }
    const uint32_t new_base = (uint32_t)bump;
    cbase[new_id] = new_base;
    bump += cnt[new_id];
    uint32_t* const row_a = sq.start2 + (size_t)s_a * (B + 1);
    uint32_t* const row_new = sq.start2 + (size_t)S * (B + 1);
    hipLaunchKernelGGL(k_squash_merge, dim3((B + 1 + 255) / 256), blk, 0, ctx->stream, row_a, sq.start2 + (size_t)s_b * (B + 1), d_pairs,
                       d_weight, sq.px[cur], sq.pw[cur], sq.pe[cur], B, new_base, (double)csize[new_id], row_new,
                       ly.P + (size_t)s_a * B);
    hipLaunchKernelGGL(k_squash_copy_row, dim3((B + 1 + 255) / 256), blk, 0, ctx->stream, row_new, B + 1, row_a);
    hipLaunchKernelGGL(k_krd_scan, dim3(1), blk, 0, ctx->stream, ly.P + (size_t)s_a * B, B);
    epa_timer_stop(ctx, epa_t(ctx, epa_ctx::T_SQUASH_MERGE));
    epa_timer_start(ctx, epa_t(ctx, epa_ctx::T_SQUASH_ROW));
    hipLaunchKernelGGL(k_squash_row, dim3(A2 * n_tiles), blk, 0, ctx->stream, ly.P, sq.start2, sq.px[cur], sq.pw[cur], ly.rlen, ly.rsize,
                       B, n_tiles, sq.act, s_a, sq.part);
    hipLaunchKernelGGL(k_squash_row_finish, dim3((A2 + 255) / 256), blk, 0, ctx->stream, sq.part, n_tiles, sq.act, A2, s_a, S, sq.D);
    epa_timer_stop(ctx, epa_t(ctx, epa_ctx::T_SQUASH_ROW));
  }
  epa_timer_stop(ctx, epa_t(ctx, epa_ctx::T_SQUASH));
  EPA_HIP(ctx, hipGetLastError());
  EPA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (S > 1) { add_ms(1); add_ms(2); }
  if (ctx->opt.timers) {
    for (int k = 0; k < 3; ++k) ctx->squash_ms[k] = sums[k];
    ctx->squash_ms[3] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - loop_begin).count();
  }
  EPA_HIP(ctx, squash_out(merge_a, h_a));
  EPA_HIP(ctx, squash_out(merge_b, h_b));
  EPA_HIP(ctx, squash_out(merge_dist, h_d));
  EPA_HIP(ctx, squash_out(merge_size, h_size));
  return EPA_OK;
}
