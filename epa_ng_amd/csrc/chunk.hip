// libepa_dev.so -- the chunk path: the fused chunk body (preplacement -> candidate selection -> Newton launch on
// device buffers), epa_dev_place_chunk, and the slot pipeline with its group launches (include/epa_dev.h).
#include "epa_dev_internal.hpp"

#include <string.h>

#include <algorithm>

// The body of the reference's chunk loop (src/core/place.cpp:219-235) on device buffers:
// place() -> apply_heuristic() -> place_thorough().  The Q x B table never leaves HBM; ONE host
// sync in the middle (the candidate count sizes the thorough launch); the thorough kernels are
// queued on return, nothing is waited for after them.
// begin: preplacement + first half of the selection, nothing waited for; end: the wait for the
// candidate count (and the window-validation words, read back in the same copy), compaction / sort,
// the thorough launches.  rb: 64-word host block (pinned in the chunk pipeline).
static int chunk_body_begin(epa_ctx* ctx, const uint8_t* d_codes, const uint32_t* d_begin, const uint32_t* d_span,
                            uint32_t Q, uint32_t max_span, double threshold, epa_pair* d_pairs,
                            uint64_t max_pairs, uint32_t* rb, SelectPending* sp, epa_result* d_res = nullptr,
                            unsigned long long* d_stats = nullptr) {
  // internal table: rows padded to whole 64-byte sectors (the preplacement kernels write 8
  // consecutive branches per burst; with rows of B doubles every burst straddled two sectors)
  const uint32_t pitch = (ctx->B + 7u) & ~7u;
  PreTable t{(double*)epa_scratch(ctx, SLOT_TABLE, sizeof(double) * (size_t)Q * pitch), pitch};
  if (!t.lnl) return epa_fail(ctx, EPA_ERR_HIP, "hipMalloc(chunk table)");
  // per-(query, 64-branch segment) maxima of the table: a by-product of the preplacement fast paths that lets
  // the dynamic rule read only the segments near a row's maximum (preplace.hip SegTrack, select.hip k_select_seg)
  const uint32_t nseg = (ctx->B + 63) / 64;
  if (nseg <= 64 && ctx->heur_mode == 0) {
    t.segp = (nseg + 7u) & ~7u;
    t.segmax = (unsigned long long*)epa_scratch(ctx, SLOT_SEGMAX, sizeof(unsigned long long) * (size_t)Q * t.segp);
    if (!t.segmax) return epa_fail(ctx, EPA_ERR_HIP, "hipMalloc(segment maxima)");
  }
  // the selection below is this table's only reader: where it reads by segment maxima, the preplacement may screen
  if (epa_select_takes_seg(ctx, t, Q, threshold)) t.band_t = epa_select_band_t(threshold, ctx->B);
  const uint32_t* pre_status = nullptr;
  int rc = launch_preplace(ctx, d_codes, d_begin, d_span, Q, t, max_span, &pre_status);
  if (!rc) rc = launch_select_begin(ctx, t, pre_status, Q, threshold, d_pairs, max_pairs, d_span, rb, sp);
  // what may be queued behind the selection's read-back: bitmap form, and a pair list k_emit_pairs can bound
  const bool behind_rb = !rc && d_stats && sp->d_rb && sp->bitmap && max_pairs <= 0xffffffffull;
  // One read length (the windows can only be of max_span's class): pair list and Newton kernel can be queued right
  // here, guarded on the device by the same read-back block the host will look at in chunk_body_end -- no host round
  // trip between the selection and the thorough kernel.  OPT-IN (EPA_QUEUED_THOROUGH=1):
  // measured (profiles/r4_queued_thorough.txt) it buys nothing -- a chunk's preplacement and its Newton kernel each
  // need whole CUs, so they serialise on the device whichever is queued first -- and with HIP's default four
  // hardware queues the early Newton kernel blocks the other slots' chains that share its queue (8.5 -> 7.7 M/s).
  // Bitmap form: the pair list is written behind the read-back at once (k_emit_pairs refuses a list that would not fit),
  // and the statistics block + work counters of the chunk's Newton launch are cleared behind it -- both in the shadow
  // of the host's round trip for the candidate count (15 - 25 us) instead of after it (profiles/r5_step_timeline.txt)
  if (behind_rb) {
    rc = launch_select_emit(ctx, sp);
    if (!rc) rc = epa_zero_async(ctx, d_stats, 128, epa_th_ctr(ctx), epa_th_ctr(ctx) ? 64 : 0);
    if (!rc) {
      ctx->clean_stats[ctx->bank] = d_stats;
      ctx->clean_ctr[ctx->bank] = epa_th_ctr(ctx) != nullptr;
    }
  }
  if (behind_rb && !rc && d_res) {
    const bool off = !ctx->opt.queued_thorough;
    const int cls = epa_span_class(ctx->s, max_span);
    const bool eligible = !off && ctx->s == 4 && !ctx->generic_thorough && ctx->dna.ng == 1 && epa_th_ctr(ctx) &&
                          epa_tip_class_ok(cls);   // the single-wave classes
    if (eligible) {
      rc = launch_select_emit(ctx, sp);
      if (!rc && ctx->clean_stats[ctx->bank] == d_stats) ctx->clean_stats[ctx->bank] = nullptr;
      else if (!rc) rc = epa_zero_async(ctx, d_stats, 128);
      if (!rc) {
        const int q = launch_thorough_queued(ctx, d_pairs, sp->d_rb, max_pairs, d_codes, d_begin, d_span, max_span, d_res, d_stats);
        if (q == -2) return EPA_ERR_HIP;
        sp->queued_cls = q;
      }
    }
  }
  return rc;
}

static int chunk_body_end(epa_ctx* ctx, SelectPending* sp, const uint8_t* d_codes, const uint32_t* d_begin,
                          const uint32_t* d_span, uint32_t max_span, epa_pair* d_pairs, epa_result* d_res,
                          unsigned long long* d_stats, uint64_t* n_out) {
  uint64_t n = 0;
  int rc = launch_select_end(ctx, sp, &n);  // syncs once
  if (rc) return rc;
  rc = select_check_status(ctx, sp);
  if (rc) return rc;
  *n_out = n;
  // the queued launch ran iff all n pairs are of its class (no overflow / window error: checked above) -- the test
  // k_thorough_dna applied to the same block
  // (both halves of the class where the selection counted its tip-distal pairs apart: the queued launch takes them all)
  if (sp->queued_cls >= 0 && sp->rb[RB_HIST + sp->queued_cls] + sp->rb[RB_HIST + epa_tip_class(sp->queued_cls)] == (uint32_t)n) return EPA_OK;
  if (ctx->clean_stats[ctx->bank] == d_stats && sp->queued_cls < 0) ctx->clean_stats[ctx->bank] = nullptr;   // cleared behind the selection
  else {
    ctx->clean_stats[ctx->bank] = nullptr;
    rc = epa_zero_async(ctx, d_stats, 128);
    if (rc) return rc;
  }
  if (n == 0) return EPA_OK;
  // the selection's class histogram travels in *sp: it describes these n pairs and nothing else
  // (a context that forms tip-distal keys needs them in the histogram: a selection that could not split them off --
  // several span classes, the staging form -- leaves the count to launch_thorough)
  const bool hist_ok = sp->have_hist && (sp->tip_split || !epa_tipd_active(ctx));
  return launch_thorough(ctx, d_pairs, n, d_codes, d_begin, d_span, max_span, d_res, d_stats,
                         hist_ok ? sp->cls_hist : nullptr);
}

static int chunk_body(epa_ctx* ctx, const uint8_t* d_codes, const uint32_t* d_begin, const uint32_t* d_span,
                      uint32_t Q, uint32_t max_span, double threshold, epa_pair* d_pairs, epa_result* d_res,
                      uint64_t max_pairs, unsigned long long* d_stats, uint64_t* n_out) {
  uint32_t rb[64] = {};
  SelectPending sp;
  int rc = chunk_body_begin(ctx, d_codes, d_begin, d_span, Q, max_span, threshold, d_pairs, max_pairs, rb, &sp, d_res, d_stats);
  if (rc) return rc;
  return chunk_body_end(ctx, &sp, d_codes, d_begin, d_span, max_span, d_pairs, d_res, d_stats, n_out);
}

int chunk_stats(epa_ctx* ctx, uint64_t n, const unsigned long long* hst, epa_thorough_stats* stats) {
  epa_xcd_feedback(ctx, n, hst);
  ctx->last_stats.pairs = n;
  ctx->last_stats.rounds = hst[0];
  ctx->last_stats.newton_evals = hst[1];
  ctx->last_stats.reverts = hst[2];
  if (stats) *stats = ctx->last_stats;
  if (hst[3])  // pairs whose lnL came out -inf / NaN
    return epa_fail(ctx, EPA_ERR_NEG_INF,
                    "-INF logl at branch " + std::to_string((uint32_t)(hst[4] >> 32)) +
                        " with sequence " + std::to_string((uint32_t)(hst[4] & 0xffffffffu)));
  return EPA_OK;
}

extern "C" int epa_dev_place_chunk(epa_ctx* ctx, const uint8_t* q_codes, const uint32_t* win_begin,
                                   const uint32_t* win_span, uint32_t Q, uint32_t max_span,
                                   double threshold, epa_pair* pairs, epa_result* results,
                                   uint64_t max_pairs, uint64_t* n_pairs, epa_thorough_stats* stats) {
  if (!ctx || !q_codes || !win_begin || !win_span || !pairs || !results || !n_pairs)
    return epa_fail(ctx, EPA_ERR_INVALID_ARG, "null argument");
  *n_pairs = 0;
  if (stats) memset(stats, 0, sizeof(*stats));
  if (Q == 0) return EPA_OK;
  EPA_HIP(ctx, hipSetDevice(ctx->device));
  int rc = epa_dev_build_lookup(ctx);
  if (rc) return rc;
  if (max_span == 0) {  // not supplied: look at the spans (host array, or one small D2H copy)
    std::vector<uint32_t> buf;
    const uint32_t* hs = host_view(win_span, Q, buf, ctx->stream);
    if (!hs) return epa_fail(ctx, EPA_ERR_HIP, "cannot read window spans");
    for (uint32_t q = 0; q < Q; ++q) max_span = std::max(max_span, hs[q]);
  }
  if (max_span > ctx->W) max_span = ctx->W;
  const uint8_t* d_codes = epa_codes_to_device(ctx, q_codes, Q);
  const uint32_t* d_begin = (const uint32_t*)epa_to_device(ctx, SLOT_BEGIN, win_begin, sizeof(uint32_t) * Q);
  const uint32_t* d_span = (const uint32_t*)epa_to_device(ctx, SLOT_SPAN, win_span, sizeof(uint32_t) * Q);
  if (!d_codes || !d_begin || !d_span) return epa_fail(ctx, EPA_ERR_HIP, "query upload failed");
  const bool pairs_dev = epa_is_device_ptr(pairs), res_dev = epa_is_device_ptr(results);
  epa_pair* d_pairs = pairs_dev ? pairs : (epa_pair*)epa_scratch(ctx, SLOT_PAIRS, sizeof(epa_pair) * max_pairs);
  epa_result* d_res = res_dev ? results : (epa_result*)epa_scratch(ctx, SLOT_RESULTS, sizeof(epa_result) * max_pairs);
  if (!d_pairs || !d_res) return epa_fail(ctx, EPA_ERR_HIP, "hipMalloc(chunk buffers)");
  // thorough counters: second half of the context's 256-byte counter block
  unsigned long long* d_stats = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(epa_th_ctr(ctx)) + 128);
  uint64_t n = 0;
  rc = chunk_body(ctx, d_codes, d_begin, d_span, Q, max_span, threshold, d_pairs, d_res, max_pairs, d_stats, &n);
  if (rc) return rc;
  *n_pairs = n;
  if (n == 0) return EPA_OK;
  unsigned long long hst[16];
  if (!pairs_dev)
    EPA_HIP(ctx, hipMemcpyAsync(pairs, d_pairs, sizeof(epa_pair) * n, hipMemcpyDeviceToHost, ctx->stream));
  if (!res_dev)
    EPA_HIP(ctx, hipMemcpyAsync(results, d_res, sizeof(epa_result) * n, hipMemcpyDeviceToHost, ctx->stream));
  EPA_HIP(ctx, hipMemcpyAsync(hst, d_stats, 128, hipMemcpyDeviceToHost, ctx->stream));
  EPA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return chunk_stats(ctx, n, hst, stats);
}

// ---------------------------------------------------------------------------------------------
// Double-buffered chunk pipeline (see include/epa_dev.h): stage -> launch -> finish per slot.
// ---------------------------------------------------------------------------------------------
static int slot_of(epa_ctx* ctx, int slot, ChunkSlot** out) {
  if (!ctx) return EPA_ERR_INVALID_ARG;
  if (slot < 0 || slot >= epa_ctx::N_SLOTS) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "chunk pipeline: slot must be 0 .. 23");
  ChunkSlot& s = ctx->slots[slot];
  if (!ctx->copy_stream) EPA_HIP(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
  if (!ctx->down_stream) EPA_HIP(ctx, hipStreamCreateWithFlags(&ctx->down_stream, hipStreamNonBlocking));
  if (!s.ev_up) {
    EPA_HIP(ctx, hipEventCreateWithFlags(&s.ev_up, hipEventDisableTiming));
    EPA_HIP(ctx, hipEventCreateWithFlags(&s.ev_done, hipEventDisableTiming));
    EPA_HIP(ctx, hipEventCreateWithFlags(&s.ev_down, hipEventDisableTiming));
    EPA_HIP(ctx, hipEventCreateWithFlags(&s.ev_base, hipEventDisableTiming));
    EPA_HIP(ctx, hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
    EPA_HIP(ctx, hipHostMalloc((void**)&s.h_stats, 128, hipHostMallocDefault));
    EPA_HIP(ctx, hipHostMalloc((void**)&s.h_sel, 256, hipHostMallocDefault));
    EPA_HIP(ctx, hipMalloc((void**)&s.d_stats, 128));
  }
  *out = &s;
  return EPA_OK;
}

template <class T>
static int grow_dev(epa_ctx* ctx, T** p, size_t* have, size_t want_bytes) {
  if (want_bytes <= *have) return EPA_OK;
  if (*p) (void)hipFree(*p);
  *p = nullptr; *have = 0;
  const size_t sz = want_bytes + want_bytes / 4 + 1024;
  EPA_HIP(ctx, hipMalloc((void**)p, sz));
  *have = sz;
  return EPA_OK;
}
static int grow_pinned(epa_ctx* ctx, void** p, size_t* have, size_t want_bytes) {
  if (want_bytes <= *have) return EPA_OK;
  if (*p) (void)hipHostFree(*p);
  *p = nullptr; *have = 0;
  const size_t sz = want_bytes + want_bytes / 4 + 1024;
  EPA_HIP(ctx, hipHostMalloc(p, sz, hipHostMallocDefault));
  *have = sz;
  return EPA_OK;
}

extern "C" int epa_dev_chunk_stage(epa_ctx* ctx, int slot, const uint8_t* q_codes, const uint32_t* win_begin,
                                   const uint32_t* win_span, uint32_t Q) {
  ChunkSlot* s;
  int rc = slot_of(ctx, slot, &s);
  if (rc) return rc;
  if (!q_codes || !win_begin || !win_span || Q == 0) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "chunk_stage: null / empty chunk");
  if (s->unfinished()) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "chunk_stage: the slot has an unfinished launch");
  if (s->g_left > 0) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "chunk_stage: members of this slot's group launch are not finished yet (their results live in its buffers)");
  EPA_HIP(ctx, hipSetDevice(ctx->device));
  s->stride = ctx->code_stride ? ctx->code_stride : ctx->W;
  s->packed4 = ctx->code_packed4;
  const size_t row = s->packed4 ? ((size_t)s->stride + 1) / 2 : s->stride;
  s->codes_bytes = ((size_t)Q * row + 255) & ~(size_t)255;
  const size_t total = s->codes_bytes + 2 * sizeof(uint32_t) * (size_t)Q;
  const bool dev_in = epa_is_device_ptr(q_codes);
  if (dev_in != epa_is_device_ptr(win_begin) || dev_in != epa_is_device_ptr(win_span))
    return epa_fail(ctx, EPA_ERR_INVALID_ARG, "chunk_stage: the three arrays must be all host or all device memory");
  if (dev_in) {
    // HBM-resident chunk: the slot reads the caller's arrays in place (no copy, no copy-stream
    // work); they must stay untouched until chunk_finish and be complete on the context's stream
    s->x_codes = q_codes; s->x_begin = win_begin; s->x_span = win_span;
    s->Q = Q;
    s->state = SlotState::Staged;
    return EPA_OK;
  }
  s->x_codes = nullptr;
  rc = grow_pinned(ctx, &s->h_in, &s->h_in_sz, total);
  if (!rc) rc = grow_dev(ctx, (char**)&s->d_in, &s->d_in_sz, total + 1024);
  if (rc) return rc;
  char* h = (char*)s->h_in;
  memcpy(h, q_codes, (size_t)Q * row);
  memcpy(h + s->codes_bytes, win_begin, sizeof(uint32_t) * (size_t)Q);
  memcpy(h + s->codes_bytes + sizeof(uint32_t) * (size_t)Q, win_span, sizeof(uint32_t) * (size_t)Q);
  EPA_HIP(ctx, hipMemcpyAsync(s->d_in, s->h_in, total, hipMemcpyHostToDevice, ctx->copy_stream));
  EPA_HIP(ctx, hipEventRecord(s->ev_up, ctx->copy_stream));
  s->Q = Q;
  s->state = SlotState::Staged;
  return EPA_OK;
}

namespace {
// the context's stream / scratch bank are the slot's for the duration of a pipeline call only
struct SlotScope {
  epa_ctx* c; hipStream_t st; uint32_t stride; bool packed;
  SlotScope(epa_ctx* ctx, ChunkSlot* s, int slot) : c(ctx), st(ctx->stream), stride(ctx->code_stride), packed(ctx->code_packed4) {
    ctx->stream = s->stream;
    ctx->bank = 1 + slot;
    ctx->code_stride = s->stride == ctx->W ? 0 : s->stride;   // the kernels read the layout the chunk was staged with
    ctx->code_packed4 = false;
  }
  ~SlotScope() { c->stream = st; c->bank = 0; c->code_stride = stride; c->code_packed4 = packed; }
};
}  // namespace

static int chunk_launch_begin_impl(epa_ctx* ctx, int slot, ChunkSlot* s, uint32_t max_span, double threshold,
                                   epa_pair* d_pairs, epa_result* d_results, uint64_t max_pairs, uint32_t flags) {
  int rc = EPA_OK;
  if (s->state != SlotState::Staged) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "chunk_launch: the slot holds no staged chunk");
  if ((d_pairs == nullptr) != (d_results == nullptr))
    return epa_fail(ctx, EPA_ERR_INVALID_ARG, "chunk_launch: pass both result buffers or neither");
  if (d_pairs && (!epa_is_device_ptr(d_pairs) || !epa_is_device_ptr(d_results)))
    return epa_fail(ctx, EPA_ERR_INVALID_ARG, "chunk_launch: result buffers must be device memory");
  EPA_HIP(ctx, hipSetDevice(ctx->device));
  rc = epa_dev_build_lookup(ctx);
  if (rc) return rc;
  const uint32_t Q = s->Q;
  if (max_span == 0 || max_span > ctx->W) max_span = ctx->W;
  if (!d_pairs) {
    rc = grow_dev(ctx, &s->d_pairs, &s->d_pairs_sz, sizeof(epa_pair) * max_pairs);
    if (!rc) rc = grow_dev(ctx, &s->d_res, &s->d_res_sz, sizeof(epa_result) * max_pairs);
    if (rc) return rc;
    d_pairs = s->d_pairs;
    d_results = s->d_res;
  }
  // The slot's kernels go to the slot's own stream and scratch bank, so that the two chunks in
  // flight overlap on the device (chunk k + 1's preplacement and selection fill the tail of chunk
  // k's Newton kernel) and the wait for chunk k + 1's candidate count does not wait for chunk k's
  // kernels.  The slot stream starts behind what the caller's stream has queued so far (lookup
  // build; with device-resident results, the caller's reads of the result buffers).
  if (!(flags & EPA_CHUNK_HOST_ORDERED)) {
    EPA_HIP(ctx, hipEventRecord(s->ev_base, ctx->stream));
    EPA_HIP(ctx, hipStreamWaitEvent(s->stream, s->ev_base, 0));
  }
  if (!s->x_codes) EPA_HIP(ctx, hipStreamWaitEvent(s->stream, s->ev_up, 0));
  SlotScope scope(ctx, s, slot);
  const ChunkInputs in = s->staged_inputs();
  const uint8_t* d_codes = in.codes;
  if (s->packed4) {
    rc = grow_dev(ctx, &s->d_unpacked, &s->d_unpacked_sz, (size_t)Q * s->stride + 1024);
    if (rc) return rc;
    launch_unpack4(ctx->stream, in.codes, s->d_unpacked, Q, s->stride);
    d_codes = s->d_unpacked;
  }
  s->l_codes = d_codes; s->l_begin = in.begin; s->l_span = in.span;
  s->l_pairs = d_pairs; s->l_res = d_results; s->l_max_span = max_span; s->l_flags = flags;
  rc = chunk_body_begin(ctx, d_codes, in.begin, in.span, Q, max_span, threshold, d_pairs, max_pairs, s->h_sel, &s->sel,
                        d_results, s->d_stats);
  if (rc) return rc;   // the slot stays staged
  s->state = SlotState::Begun;
  return EPA_OK;
}

extern "C" int epa_dev_chunk_launch_begin(epa_ctx* ctx, int slot, uint32_t max_span, double threshold,
                                          epa_pair* d_pairs, epa_result* d_results, uint64_t max_pairs,
                                          uint32_t flags) {
  ChunkSlot* s;
  int rc = slot_of(ctx, slot, &s);
  if (rc) return rc;
  return chunk_launch_begin_impl(ctx, slot, s, max_span, threshold, d_pairs, d_results, max_pairs, flags);
}

// ---- group launches ---------------------------------------------------------------------------------
namespace {
struct GroupDesc {
  const uint8_t* codes[EPA_MAX_GROUP];
  const uint32_t* begin[EPA_MAX_GROUP];
  const uint32_t* span[EPA_MAX_GROUP];
  uint32_t qoff[EPA_MAX_GROUP + 1];   // first merged query index of every member; [n] = total
  uint32_t n, row;                    // members; bytes per code row (the same for all of them)
};

__device__ __forceinline__ int group_member(const uint32_t* qoff, int n, uint32_t q) {
  int m = 0;
  for (int i = 1; i < n; ++i) m += q >= qoff[i];
  return m;
}

// the members' staged arrays -> one chunk: codes rows, window begins, window spans back to back
__global__ void __launch_bounds__(256) k_concat_chunks(const GroupDesc g, uint8_t* __restrict__ codes, uint32_t* __restrict__ begin,
                                                       uint32_t* __restrict__ span) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t total_bytes = (uint64_t)g.qoff[g.n] * g.row;
  const uint64_t nwords = (total_bytes + 3) / 4;
  if (i < nwords) {
    uint32_t v = 0;
    for (int k = 0; k < 4; ++k) {
      const uint64_t b = i * 4 + k;
      if (b >= total_bytes) break;
      const uint32_t q = (uint32_t)(b / g.row);
      const int m = group_member(g.qoff, (int)g.n, q);
      v |= (uint32_t)g.codes[m][b - (uint64_t)g.qoff[m] * g.row] << (8 * k);
    }
    if (i * 4 + 4 <= total_bytes) reinterpret_cast<uint32_t*>(codes)[i] = v;
    else for (int k = 0; i * 4 + k < total_bytes; ++k) codes[i * 4 + k] = (uint8_t)(v >> (8 * k));
    return;
  }
  const uint64_t q = i - nwords;
  if (q >= g.qoff[g.n]) return;
  const int m = group_member(g.qoff, (int)g.n, (uint32_t)q);
  begin[q] = g.begin[m][q - g.qoff[m]];
  span[q] = g.span[m][q - g.qoff[m]];
}

// Stable partition of the group's n (pair, result) rows by member: member m's rows keep their order (branch-major,
// queries ascending -- the order of its own chunk's Work, src/core/Work.hpp:21-113) and get their chunk-local
// sequence ids back; goff[m] = first row of member m, goff[n_members] = n.  One 1024-thread workgroup (group
// launches exist for SMALL chunks: tens of thousands of rows; correct for any n).
__global__ void __launch_bounds__(1024) k_split_group(const epa_pair* __restrict__ pairs, const epa_result* __restrict__ res,
                                                      uint32_t n, const GroupDesc g, epa_pair* __restrict__ o_pairs,
                                                      epa_result* __restrict__ o_res, uint32_t* __restrict__ goff) {
  __shared__ uint32_t wsum[16];
  __shared__ uint32_t base[EPA_MAX_GROUP + 1];
  const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const uint32_t per = (n + 1023) / 1024;
  const uint32_t lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
  uint32_t cnt[EPA_MAX_GROUP] = {};
  for (uint32_t i = lo; i < hi; ++i) {
    const int m = group_member(g.qoff, (int)g.n, pairs[i].seq_id);
#pragma unroll
    for (int k = 0; k < EPA_MAX_GROUP; ++k) cnt[k] += (k == m);
  }
  // per member: exclusive prefix of the threads' counts (wave scan + wave totals), then the members' bases
  uint32_t pre[EPA_MAX_GROUP];
  uint32_t run = 0;
  for (int k = 0; k < EPA_MAX_GROUP; ++k) {
    uint32_t v = cnt[k];
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t u = __shfl_up(v, d, 64);
      if ((int)lane >= d) v += u;
    }
    if (lane == 63) wsum[wv] = v;
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (int w = 0; w < 16; ++w) { const uint32_t x = wsum[w]; total += x; if (w < (int)wv) before += x; }
    pre[k] = run + before + v - cnt[k];
    if (t == 0) base[k] = run;
    run += total;
    __syncthreads();
  }
  if (t == 0) {
    for (int k = 0; k <= (int)g.n && k < EPA_MAX_GROUP; ++k) goff[k] = base[k];
    goff[g.n] = n;
  }
  for (uint32_t i = lo; i < hi; ++i) {
    epa_pair p = pairs[i];
    const int m = group_member(g.qoff, (int)g.n, p.seq_id);
    uint32_t dst = 0;
#pragma unroll
    for (int k = 0; k < EPA_MAX_GROUP; ++k)
      if (k == m) dst = pre[k]++;
    p.seq_id -= g.qoff[m];
    o_pairs[dst] = p;
    o_res[dst] = res[i];
  }
}

GroupDesc group_desc(const ChunkSlot* L) {   // what k_split_group reads of it
  GroupDesc g{};
  g.n = (uint32_t)L->g_n;
  for (int i = 0; i <= L->g_n; ++i) g.qoff[i] = L->g_qoff[i];
  return g;
}
}  // namespace

extern "C" int epa_dev_chunk_launch_many_begin(epa_ctx* ctx, const int* slots, int n_slots, uint32_t max_span,
                                               double threshold, uint64_t max_pairs, uint32_t flags) {
  if (!ctx || !slots || n_slots < 1 || n_slots > EPA_MAX_GROUP)
    return epa_fail(ctx, EPA_ERR_INVALID_ARG, "chunk_launch_many: 1 .. 8 slots");
  ChunkSlot* m[EPA_MAX_GROUP];
  for (int i = 0; i < n_slots; ++i) {
    int rc = slot_of(ctx, slots[i], &m[i]);
    if (rc) return rc;
    for (int j = 0; j < i; ++j)
      if (slots[j] == slots[i]) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "chunk_launch_many: a slot is listed twice");
    if (m[i]->state != SlotState::Staged) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "chunk_launch_many: slot " + std::to_string(slots[i]) + " holds no staged chunk");
    if (m[i]->stride != m[0]->stride || m[i]->packed4 != m[0]->packed4)
      return epa_fail(ctx, EPA_ERR_INVALID_ARG, "chunk_launch_many: the chunks were staged with different query layouts");
  }
  ChunkSlot* L = m[0];
  if (L->g_left > 0) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "chunk_launch_many: members of the leader's previous group are not finished yet");
  if (n_slots == 1) return chunk_launch_begin_impl(ctx, slots[0], L, max_span, threshold, nullptr, nullptr, max_pairs, flags);
  EPA_HIP(ctx, hipSetDevice(ctx->device));
  GroupDesc g{};
  g.n = (uint32_t)n_slots;
  g.row = L->packed4 ? (L->stride + 1) / 2 : L->stride;
  uint64_t total = 0;
  for (int i = 0; i < n_slots; ++i) {
    const ChunkInputs in = m[i]->staged_inputs();
    g.codes[i] = in.codes; g.begin[i] = in.begin; g.span[i] = in.span;
    g.qoff[i] = (uint32_t)total;
    total += m[i]->Q;
  }
  if (total > 0x7fffffffull) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "chunk_launch_many: too many queries in one group");
  g.qoff[n_slots] = (uint32_t)total;
  const size_t cbytes = ((size_t)total * g.row + 255) & ~(size_t)255;
  int rc = grow_dev(ctx, (char**)&L->d_merge, &L->d_merge_sz, cbytes + 2 * sizeof(uint32_t) * (size_t)total + 1024);
  if (rc) return rc;
  if (!L->d_goff) {
    EPA_HIP(ctx, hipMalloc((void**)&L->d_goff, sizeof(uint32_t) * (EPA_MAX_GROUP + 1)));
    EPA_HIP(ctx, hipHostMalloc((void**)&L->h_goff, sizeof(uint32_t) * (EPA_MAX_GROUP + 1), hipHostMallocDefault));
  }
  // the merge runs on the leader's stream, behind the caller's stream (device-resident chunks) and every member's upload
  if (!(flags & EPA_CHUNK_HOST_ORDERED)) {
    EPA_HIP(ctx, hipEventRecord(L->ev_base, ctx->stream));
    EPA_HIP(ctx, hipStreamWaitEvent(L->stream, L->ev_base, 0));
  }
  for (int i = 0; i < n_slots; ++i)
    if (!m[i]->x_codes) EPA_HIP(ctx, hipStreamWaitEvent(L->stream, m[i]->ev_up, 0));
  uint8_t* mc = (uint8_t*)L->d_merge;
  uint32_t* mb = (uint32_t*)(mc + cbytes);
  uint32_t* ms = mb + total;
  const uint64_t threads = ((uint64_t)total * g.row + 3) / 4 + total;
  hipLaunchKernelGGL(k_concat_chunks, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, L->stream, g, mc, mb, ms);
  EPA_HIP(ctx, hipGetLastError());
  L->lead_merged((uint32_t)total, mc, mb, ms);
  rc = chunk_launch_begin_impl(ctx, slots[0], L, max_span, threshold, nullptr, nullptr, max_pairs, flags);
  if (rc) { L->restore_own(); return rc; }   // every member stays staged
  L->group_begun(ctx->slots, slots, n_slots, g.qoff);
  return EPA_OK;
}

extern "C" int epa_dev_chunk_launch_many(epa_ctx* ctx, const int* slots, int n_slots, uint32_t max_span, double threshold,
                                         uint64_t max_pairs, uint32_t flags) {
  int rc = epa_dev_chunk_launch_many_begin(ctx, slots, n_slots, max_span, threshold, max_pairs, flags);
  if (rc) return rc;
  return epa_dev_chunk_launch_end(ctx, slots[0]);
}

// A failure that may leave kernels of the chunk in flight on the slot's stream: wait for them and free the slot (and the
// members of its group), so that it cannot be re-staged or re-launched (its result buffers re-allocated) under running kernels
static int abandon_slot(epa_ctx* ctx, ChunkSlot* s, int code) {
  (void)hipStreamSynchronize(s->stream);
  s->launch_over(ctx->slots, SlotState::Free);
  return code;
}
#define SLOT_HIP(call, what) \
  do { if ((call) != hipSuccess) return abandon_slot(ctx, s, epa_fail(ctx, EPA_ERR_HIP, what)); } while (0)

extern "C" int epa_dev_chunk_launch_end(epa_ctx* ctx, int slot) {
  ChunkSlot* s;
  int rc = slot_of(ctx, slot, &s);
  if (rc) return rc;
  if (s->state == SlotState::GroupMember) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "chunk_launch_end: the slot is a member of a group launch: end the group's first slot");
  if (s->state != SlotState::Begun) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "chunk_launch_end: no launch was begun on the slot");
  EPA_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t base = ctx->stream;
  uint64_t n = 0;
  epa_pair* d_pairs = s->l_pairs;
  epa_result* d_results = s->l_res;
  SlotScope scope(ctx, s, slot);
  rc = chunk_body_end(ctx, &s->sel, s->l_codes, s->l_begin, s->l_span, s->l_max_span, d_pairs, d_results, s->d_stats, &n);
  // Candidate overflow and the window-validation errors are found before any thorough kernel is queued: the slot, and
  // every member of its group, stays staged (launch again with a larger max_pairs, the group or one by one)
  if (rc == EPA_ERR_PAIR_OVERFLOW || rc == EPA_ERR_QUERY_ALL_GAP || rc == EPA_ERR_QUERY_WIDTH) {
    s->launch_over(ctx->slots, SlotState::Staged);
    return rc;
  }
  if (rc) return abandon_slot(ctx, s, rc);
  s->n = n;
  const bool group = s->g_n > 1;
  if (group) {
    // regroup the rows by member (stable), chunk-local sequence ids back
    if (s->g_cap < n) {
      if (s->d_gpairs) (void)hipFree(s->d_gpairs);
      if (s->d_gres) (void)hipFree(s->d_gres);
      s->d_gpairs = nullptr; s->d_gres = nullptr; s->g_cap = 0;
      const size_t want = n + n / 4 + 1024;
      SLOT_HIP(hipMalloc((void**)&s->d_gpairs, sizeof(epa_pair) * want), "hipMalloc(group rows)");
      SLOT_HIP(hipMalloc((void**)&s->d_gres, sizeof(epa_result) * want), "hipMalloc(group rows)");
      s->g_cap = want;
    }
    hipLaunchKernelGGL(k_split_group, dim3(1), dim3(1024), 0, ctx->stream, d_pairs, d_results, (uint32_t)n, group_desc(s),
                       s->d_gpairs, s->d_gres, s->d_goff);
    SLOT_HIP(hipGetLastError(), "k_split_group launch");
    d_pairs = s->d_gpairs;
    d_results = s->d_gres;
  }
  SLOT_HIP(hipEventRecord(s->ev_done, ctx->stream), "hipEventRecord(chunk done)");
  SLOT_HIP(hipStreamWaitEvent(ctx->down_stream, s->ev_done, 0), "hipStreamWaitEvent(chunk done)");
  if (group) {
    SLOT_HIP(hipMemcpyAsync(s->h_goff, s->d_goff, sizeof(uint32_t) * (EPA_MAX_GROUP + 1), hipMemcpyDeviceToHost, ctx->down_stream),
             "hipMemcpyAsync(group offsets)");
    s->group_launched(ctx->slots);
  }
  if (s->l_flags & EPA_CHUNK_NO_D2H) {
    s->out_pairs = d_pairs;
    s->out_res = d_results;
    // device-resident results are consumed on the caller's stream
    if (!(s->l_flags & EPA_CHUNK_HOST_ORDERED)) SLOT_HIP(hipStreamWaitEvent(base, s->ev_done, 0), "hipStreamWaitEvent (chunk_launch_end)");
  } else {
    const size_t off_r = (sizeof(epa_pair) * n + 255) & ~(size_t)255;
    rc = grow_pinned(ctx, &s->h_out, &s->h_out_sz, off_r + sizeof(epa_result) * n);
    if (rc) return abandon_slot(ctx, s, rc);
    if (n) {
      SLOT_HIP(hipMemcpyAsync(s->h_out, d_pairs, sizeof(epa_pair) * n, hipMemcpyDeviceToHost, ctx->down_stream), "hipMemcpyAsync (chunk_launch_end)");
      SLOT_HIP(hipMemcpyAsync((char*)s->h_out + off_r, d_results, sizeof(epa_result) * n, hipMemcpyDeviceToHost, ctx->down_stream),
               "hipMemcpyAsync (chunk_launch_end)");
    }
    s->out_pairs = (const epa_pair*)s->h_out;
    s->out_res = (const epa_result*)((char*)s->h_out + off_r);
  }
  SLOT_HIP(hipMemcpyAsync(s->h_stats, s->d_stats, 128, hipMemcpyDeviceToHost, ctx->down_stream), "hipMemcpyAsync (chunk_launch_end)");
  SLOT_HIP(hipEventRecord(s->ev_down, ctx->down_stream), "hipEventRecord (chunk_launch_end)");
  s->state = SlotState::Launched;
  return EPA_OK;
}
#undef SLOT_HIP

extern "C" int epa_dev_chunk_launch(epa_ctx* ctx, int slot, uint32_t max_span, double threshold,
                                    epa_pair* d_pairs, epa_result* d_results, uint64_t max_pairs,
                                    uint32_t flags) {
  int rc = epa_dev_chunk_launch_begin(ctx, slot, max_span, threshold, d_pairs, d_results, max_pairs, flags);
  if (rc) return rc;
  return epa_dev_chunk_launch_end(ctx, slot);
}

extern "C" int epa_dev_chunk_finish(epa_ctx* ctx, int slot, const epa_pair** pairs, const epa_result** results,
                                    uint64_t* n_pairs, epa_thorough_stats* stats) {
  ChunkSlot* s;
  int rc = slot_of(ctx, slot, &s);
  if (rc) return rc;
  if (s->state != SlotState::Launched) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "chunk_finish: the slot has no launch in flight");
  if (s->leader >= 0) {   // member of a group launch: its rows are a range of the leader's regrouped buffers
    ChunkSlot* L = &ctx->slots[s->leader];
    EPA_HIP(ctx, hipEventSynchronize(L->ev_down));
    const uint32_t lo = L->h_goff[s->g_index], hi = L->h_goff[s->g_index + 1];
    const uint64_t group_rows = L->n;   // (the leader's own n is replaced by its member count below)
    s->n = hi - lo;
    s->out_pairs = L->out_pairs + lo;
    s->out_res = L->out_res + lo;
    s->state = SlotState::Free;
    s->leader = -1;
    if (--L->g_left == 0) L->g_n = 0;
    if (pairs) *pairs = s->out_pairs;
    if (results) *results = s->out_res;
    if (n_pairs) *n_pairs = s->n;
    // the Newton launch was ONE launch for the group: its counters are reported with the group's first slot
    if (s->g_index == 0) {
      const int rc2 = chunk_stats(ctx, group_rows, L->h_stats, stats);
      ctx->last_stats.pairs = s->n;
      if (stats) stats->pairs = s->n;
      return rc2;
    }
    ctx->last_stats = epa_thorough_stats{};
    ctx->last_stats.pairs = s->n;
    if (stats) *stats = ctx->last_stats;
    return EPA_OK;
  }
  EPA_HIP(ctx, hipEventSynchronize(s->ev_down));
  s->state = SlotState::Free;
  if (pairs) *pairs = s->out_pairs;
  if (results) *results = s->out_res;
  if (n_pairs) *n_pairs = s->n;
  return chunk_stats(ctx, s->n, s->h_stats, stats);
}
