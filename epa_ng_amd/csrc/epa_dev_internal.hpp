// Internal declarations shared by the HIP translation units of libepa_dev.so.
// gfx950 (MI355X) only: wave64, 160 KiB LDS/CU, fp64 VALU.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>

#include "epa_dev.h"

// rocprim's radix sort falls back to a merge sort (block sort + log2 n merge passes: ~19 launches for
// the 262k candidate keys of a chunk) below one million items; the sorts of this library use a few key bits only
// (branch id, window start, span class, query), where Onesweep digit passes do: 4 - 5 launches.
using epa_radix_cfg = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config,
                                                 rocprim::default_config, 0>;

#define EPA_MAX_STATES 20
// EPA_MAX_CATS (16): include/epa_dev.h, where the host's model parser reads it too
#define EPA_MAX_COLS 24
// HIP's limit of grid.y / grid.z: a launch with the branch (or a record of a tree level) in grid.y goes out in slices
// of this many, the kernel adds the slice's first branch
#define EPA_GRID_Y 65535u

// Model constants handed to kernels by value (kernarg -> SGPRs via s_load).
struct ModelDNA {
  double U[16];     // [i][x]
  double Ui[16];    // [x][i]
  double lam[4];
  double rate[16];  // r_k (prop_invar folded in); ng groups of four categories
  double w[16];
  double pi[4];
  int ng;           // category groups: 1 (4 categories) .. 4 (16)
};

struct BloConsts {
  double min_branch, max_branch, default_branch, epsilon, pendant_default;
  uint32_t max_rounds, max_newton;
  uint32_t sliding;
  uint32_t newton_variant;  // EPA_FLAG_NEWTON_* bits: which pllmod_opt_minimize_newton is replicated
};

// Generic model block in HBM (used by the setup kernels and the 20-state path)
struct ModelDev {
  int s, c, ncols;
  double U[EPA_MAX_STATES * EPA_MAX_STATES];
  double Ui[EPA_MAX_STATES * EPA_MAX_STATES];
  double lam[EPA_MAX_STATES];
  double pi[EPA_MAX_STATES];
  double rate[EPA_MAX_CATS];
  double w[EPA_MAX_CATS];
  uint32_t colmask[EPA_MAX_COLS];  // lookup column -> state set
  // eigen-space image of each column's 0/1 tip vector: qt[col][x] = sum_{m in mask} Ui[x][m]
  double qt[EPA_MAX_COLS * EPA_MAX_STATES];
};

struct EvTimer {
  hipEvent_t a = nullptr, b = nullptr;
  bool valid = false;
};

// class keys of the thorough launches: the span classes (epa_span_class below), then the tip-distal halves of the
// single-wave DNA classes 0, 1, 2, 10, 11 (keys 12 .. 16: pairs whose branch has a tip on the distal side,
// thorough_dna.hip TIPD)
constexpr int EPA_N_CLS = 12;
constexpr int EPA_N_CLSX = 17;

// ---- the two word blocks of a candidate selection (select.hip)
// Read-back block: everything the host waits for after a selection, packed on the device (k_pack_readback) so that ONE
// small copy brings it.  launch_select_end, select_check_status and chunk_body_end read the host copy; a queued Newton
// launch (k_thorough_dna, ThArgs::spec) reads the device copy.
enum EpaReadback : int {   // int like the literals they replace: index arithmetic in the kernels keeps its type
  RB_TOTAL = 0,                  // candidate pairs
  RB_STATUS = RB_TOTAL + 1,      // the first eight words of the status block below
  RB_HIST = RB_STATUS + 8,       // [EPA_N_CLSX] pairs per class key
  RB_TIP_SPLIT = 30,             // 1: the histogram counts the tip-distal pairs apart (SelectPending::tip_split)
  RB_WINDOW = 32,                // the preplacement's window validation: [0] an all-gap query, [1] a window past the width
  RB_WORDS = RB_WINDOW + 4,
};
// Status block at the head of the selection's scratch (512 bytes, zeroed before the kernels)
enum EpaSelStatus : int {
  SEL_OVERFLOW = 2,              // staging form: the longest candidate list + 1 when a staging row was too short
  SEL_HIST = 8,                  // [EPA_N_CLS] span-class histogram of the candidate counts (k_class_hist / k_select_seg)
  SEL_TIP_TOTAL = 40,            // candidate pairs on branches that end in a tip (k_scan_counts)
  SEL_READBACK = 64,             // the packed read-back block
  SEL_WORDS = 128,
};
static_assert(RB_TOTAL == 0 && RB_STATUS == 1 && RB_HIST == 9 && RB_TIP_SPLIT == 30 && RB_WINDOW == 32 && RB_WORDS == 36,
              "the read-back block's layout is shared with queued kernels: move a word everywhere or nowhere");
static_assert(RB_HIST + EPA_N_CLSX <= RB_TIP_SPLIT && RB_TIP_SPLIT < RB_WINDOW, "read-back fields overlap");
static_assert(SEL_HIST == 8 && SEL_TIP_TOTAL == 40 && SEL_READBACK == 64, "the selection's status block moved");
static_assert(RB_HIST - RB_STATUS == SEL_HIST, "k_pack_readback copies status words and histogram in one run");
static_assert(SEL_HIST + EPA_N_CLS <= SEL_TIP_TOTAL && SEL_TIP_TOTAL < SEL_READBACK && SEL_READBACK + RB_WORDS <= SEL_WORDS,
              "status block fields overlap");

// The table a preplacement writes (launch_preplace) and a candidate selection reads (launch_select_begin)
struct PreTable {
  double* lnl = nullptr;                  // [Q][pitch]
  uint32_t pitch = 0;                     // row pitch in doubles: B, or more where the rows are padded
  // [Q][segp] order-preserving keys of the per-segment maxima of the table rows (written by the preplacement fast
  // paths of preplace.hip, which clears them first; read by k_select_seg of select.hip), or null: none wanted
  unsigned long long* segmax = nullptr;
  uint32_t segp = 0;
  // > 0: the table's only reader will be k_select_seg with this band (epa_select_takes_seg): the preplacement may then
  // leave unwritten every segment whose maximum lies further below the row maximum, given the key it writes for it
  double band_t = 0.0;
};

// Band widths of the selection from segment maxima (k_select_seg, dynamic rule, threshold < 1): candidates lie within
// band_x of the row maximum, terms that can move the LWR denominator within band_t.  The preplacement's screen
// (preplace.hip) decides with the same band_t which table segments it has to fill.
inline double epa_select_band_x(double threshold, uint32_t B) { return 1.0 - std::log((1.0 - threshold) / (double)B); }
inline double epa_select_band_t(double threshold, uint32_t B) {
  return std::max(epa_select_band_x(threshold, B), std::log((double)B) + 38.0);
}

// true: launch_select_begin reads table t (of Q rows) through k_select_seg, i.e. only the segments within band_t of a
// row's maximum (select.hip)
bool epa_select_takes_seg(const epa_ctx* ctx, const PreTable& t, uint32_t Q, double threshold);

// state of a candidate selection between launch_select_begin and launch_select_end (select.hip)
struct SelectPending {
  PreTable table;
  const uint32_t* pre_status = nullptr;   // status words of the preplacement that wrote the table, or null
  uint32_t Q = 0, cap = 0;
  double threshold = 0.0;
  epa_pair* d_pairs = nullptr;
  uint64_t max_pairs = 0;
  const uint32_t* d_span = nullptr;
  unsigned long long *stage = nullptr, *keys_a = nullptr, *keys_b = nullptr;
  uint32_t *counts = nullptr, *offsets = nullptr;
  uint32_t *bitmap = nullptr, *boffs = nullptr;   // bitmap form of the selection (select.hip, SelOut)
  uint32_t wpr = 0;
  void* temp = nullptr;
  size_t sort_bytes = 0;
  uint32_t* rb = nullptr;   // host read-back block (EpaReadback; the callers keep 64 words)
  bool have_status = false;
  hipEvent_t ev_rb = nullptr;      // recorded behind the read-back copy: launch_select_end waits for this, not for the stream
  const uint32_t* d_rb = nullptr;  // the packed read-back block on the device (bitmap form)
  bool emitted = false;            // k_emit_pairs (guarded by the total) is already queued behind the read-back
  int queued_cls = -1;             // >= 0: a thorough launch for this span class is queued too (launch_thorough_queued)
  // span-class histogram of the pairs this selection emitted (launch_select_end, when d_span was given): handed to the
  // launch_thorough of the SAME chunk body (chunk_body_end), which saves that launch's device round trip.  It lives
  // and dies with the selection: nothing in epa_ctx remembers it, so no other call can be partitioned by it
  uint32_t cls_hist[EPA_N_CLSX] = {};
  bool have_hist = false;
  bool tip_split = false;          // cls_hist counts the tip-distal pairs apart (classes EPA_N_CLS ..): rb[RB_TIP_SPLIT]
};

// One slot of the double-buffered chunk pipeline (epa_dev_chunk_stage / _launch / _finish, chunk.hip): the
// query upload of chunk k+1 and the result download of chunk k-1 run on the context's copy stream
// while the kernels of chunk k run on its compute stream.
enum class SlotState : int {
  Free,         // nothing staged, no launch in flight
  Staged,       // chunk_stage: the chunk waits for its launch (and stays so after a recoverable launch error)
  Begun,        // chunk_launch_begin: preplacement and selection are queued (a group's leader: for the merged chunk)
  Launched,     // chunk_launch_end: Newton kernels and downloads are queued; chunk_finish hands the rows out
  GroupMember,  // staged member, not the leader, of a group whose launch was begun: the leader's launch_end moves it on
};
constexpr int EPA_MAX_GROUP = 8;

struct ChunkInputs {          // the three query arrays of a chunk in HBM
  const uint8_t* codes;
  const uint32_t *begin, *span;
};

struct __attribute__((visibility("hidden"))) ChunkSlot {   // hidden: its inline functions are not exported
  void* h_in = nullptr;       // pinned bounce buffer: codes | win_begin | win_span
  size_t h_in_sz = 0;
  void* d_in = nullptr;       // the same three arrays in HBM
  const uint8_t* x_codes = nullptr;   // HBM-resident chunk staged in place (caller's arrays), else null
  const uint32_t* x_begin = nullptr;
  const uint32_t* x_span = nullptr;
  size_t d_in_sz = 0;
  uint8_t* d_unpacked = nullptr;  // one-byte codes when the chunk arrived in the 4-bit wire format
  size_t d_unpacked_sz = 0;
  size_t codes_bytes = 0;
  uint32_t Q = 0, stride = 0;
  bool packed4 = false;
  epa_pair* d_pairs = nullptr;    // slot-owned result buffers (used when the caller passes none)
  epa_result* d_res = nullptr;
  size_t d_pairs_sz = 0, d_res_sz = 0;
  void* h_out = nullptr;      // pinned: pairs | results
  size_t h_out_sz = 0;
  unsigned long long* h_stats = nullptr;  // pinned, 16 words
  unsigned long long* d_stats = nullptr;  // 16 words in HBM
  hipEvent_t ev_up = nullptr, ev_done = nullptr, ev_down = nullptr, ev_base = nullptr;
  hipStream_t stream = nullptr;  // the slot's own compute stream: the kernels of the two chunks in flight overlap
  const epa_pair* out_pairs = nullptr;    // what finish() hands out
  const epa_result* out_res = nullptr;
  uint64_t n = 0;
  SlotState state = SlotState::Free;
  bool unfinished() const { return state == SlotState::Begun || state == SlotState::Launched || state == SlotState::GroupMember; }
  ChunkInputs staged_inputs() const {   // the caller's arrays read in place, or the slot's upload
    if (x_codes) return {x_codes, x_begin, x_span};
    const char* d = (const char*)d_in;
    const uint32_t* b = (const uint32_t*)(d + codes_bytes);
    return {(const uint8_t*)d, b, b + Q};
  }
  // between launch_begin and launch_end
  SelectPending sel;
  uint32_t* h_sel = nullptr;  // pinned, 64 words: the selection's read-back block
  const uint8_t* l_codes = nullptr;
  const uint32_t *l_begin = nullptr, *l_span = nullptr;
  epa_pair* l_pairs = nullptr;
  epa_result* l_res = nullptr;
  uint32_t l_max_span = 0, l_flags = 0;
  // group launches (epa_dev_chunk_launch_many): ONE chunk body over the concatenated queries of up to
  // EPA_MAX_GROUP staged slots -- one preplacement, one selection, one Newton launch instead of one each per
  // small chunk -- run on the first slot (the leader); a kernel regroups the (pair, result) rows by member
  // afterwards (stable: every member keeps the branch-major order of its own chunk, sequence ids local again).
  int leader = -1;            // >= 0: this slot's chunk is member g_index of slot `leader`'s group (the leader: itself)
  int g_index = 0;
  int g_n = 0;                // leader: members of the group in flight (0: an ordinary launch)
  int g_left = 0;             // leader: members not finished yet (their results live in the leader's buffers)
  int g_slots[EPA_MAX_GROUP] = {};
  uint32_t g_qoff[EPA_MAX_GROUP + 1] = {};   // leader: first merged query index of every member
  uint32_t own_Q = 0;         // leader: its own chunk (restored after the group launch / on a recoverable error)
  const uint8_t* own_x_codes = nullptr;
  const uint32_t *own_x_begin = nullptr, *own_x_span = nullptr;
  void* d_merge = nullptr;    // leader: merged codes | win_begin | win_span
  size_t d_merge_sz = 0;
  epa_pair* d_gpairs = nullptr;   // leader: rows regrouped by member
  epa_result* d_gres = nullptr;
  size_t g_cap = 0;
  uint32_t* d_goff = nullptr;     // [9] member offsets into the regrouped rows (device / pinned)
  uint32_t* h_goff = nullptr;

  // ---- a group's bookkeeping, kept in its leader (`all`: epa_ctx::slots)
  // launch_many_begin: the leader stands for the merged chunk (read in place, like an HBM-resident one) ...
  void lead_merged(uint32_t total, const uint8_t* codes, const uint32_t* begin, const uint32_t* span) {
    own_Q = Q; own_x_codes = x_codes; own_x_begin = x_begin; own_x_span = x_span;
    Q = total; x_codes = codes; x_begin = begin; x_span = span;
  }
  void restore_own() { Q = own_Q; x_codes = own_x_codes; x_begin = own_x_begin; x_span = own_x_span; }
  // ... and once its launch is begun, the members are bound to it
  void group_begun(ChunkSlot* all, const int* slots, int n, const uint32_t* qoff) {
    g_n = n;
    for (int i = 0; i <= n; ++i) g_qoff[i] = qoff[i];
    for (int i = 0; i < n; ++i) {
      g_slots[i] = slots[i];
      all[slots[i]].leader = slots[0];
      all[slots[i]].g_index = i;
      if (i) all[slots[i]].state = SlotState::GroupMember;
    }
  }
  // launch_end: the group is launched -- the leader has its own chunk back, every member waits for its finish
  // (g_left counts them down: until then their rows live in the leader's buffers)
  void group_launched(ChunkSlot* all) {
    restore_own();
    g_left = g_n;
    for (int i = 1; i < g_n; ++i) {
      all[g_slots[i]].state = SlotState::Launched;
      all[g_slots[i]].l_flags = l_flags;
    }
  }
  // The launch that was begun on this slot is over without results: the slot, and with it every member of its group,
  // goes back to `to` -- Staged after a recoverable error, Free when the chunk is abandoned.  g_left is cleared as well:
  // a failure after the members were marked must not leave the leader refusing chunk_stage for ever
  void launch_over(ChunkSlot* all, SlotState to) {
    state = to;
    if (g_n <= 1) return;
    restore_own();
    for (int i = 0; i < g_n; ++i) {
      all[g_slots[i]].leader = -1;
      if (i) all[g_slots[i]].state = to;
    }
    g_n = 0;
    g_left = 0;
  }
};

// Diagnostic switches of a context (epa_dev_set_option; include/epa_dev.h lists them).  They select between code
// paths that return the same results -- cross-check kernels for the parity tests, A/B switches of the bench -- and
// replace the environment variables earlier rounds read inside the library.
struct EpaOptions {
  int thorough_generic = 0;   // every Newton launch on k_thorough_generic (the reference-shaped kernel)
  int preplace_generic = 0;   // preplacement on k_preplace (per-site gathers) instead of the pair / site fast paths
  int select_full_rows = 0;   // candidate selection from whole table rows instead of the segment maxima
  int select_sort = 0;        // candidate list through the sorted staging path instead of the bitmap
  int queued_thorough = 0;    // the Newton launch queued behind the selection, guarded by the device-side count
  int xcd_balance = 1;        // XCD shares of a Newton launch follow the measured speeds (epa_xcd_feedback)
  int aa_valu = 0;            // 20-state windows on the lane = site VALU kernel instead of the matrix-core kernel
  int timers = 1;             // hipEvent records around the kernel families (epa_dev_last_kernel_ms)
  int newton_lds = 0;         // single-wave 4-state Newton kernels read their table through LDS instead of DPP
  int tip_distal = 1;         // pairs whose branch ends in a tip run the TIPD Newton kernels (0: the row form for all)
  int dedup_key_bits = 64;    // low bits kept of a query's dedup key (dedup.hip): fewer force unequal rows into one run
  int preplace_screen = 1;    // the pair path's fp32 two-branch screen where its conditions hold (preplace.hip);
                              // 2: also for chunks below its size condition (tests)
  int preplace_screen_scale = 1;   // test only: the screen's error bound delta is multiplied by this
  int preplace_screen_i16 = 1;     // the screen in 16-bit fixed point, four branches per gather; 0: the fp32 screen
  int preplace_screen_i16_shift = 0;   // test only: the 16-bit quantum h is made smaller by this many powers of two
  int dedup_sort_bits = 32;   // low key bits the dedup sort looks at: rows equal there share a run, the full key and the codes part them
};

struct epa_ctx {
  int device = 0;
  EpaOptions opt;
  int n_cu = 256;  // compute units of the device (persistent-grid sizing)
  hipStream_t stream = nullptr;
  std::string err;

  int s = 0, c = 0, ncols = 0;
  int c_in = 0;  // rate categories of the caller's CLVs (1 or 2 are replicated to c = 4)
  uint32_t W = 0, B = 0;
  ModelDev hmodel;          // host copy
  ModelDev* dmodel = nullptr;
  ModelDNA dna;             // valid when s == 4 && c == 4
  bool dna_zero0 = false;   // eigenvalue 0 is the (exactly) zero one after the create-time reorder
  bool rate_scalers = false;  // per-rate scalers (EPA_FLAG_RATE_SCALERS): scSum is [B][c][W]
  // the tuned thorough kernels serve 4 categories + per-site scalers + sliding BLO; everything
  // else runs on k_thorough_generic (thorough_generic.hip)
  bool generic_thorough = false;
  bool generic_native = false;   // ... by the context's shape (generic_thorough may also be the option thorough_generic)
  BloConsts blo;
  int aa_x_as_n = 0;
  uint32_t code_stride = 0;  // 0: query codes are Q x W rows; S: compact rows of S bytes (window only)

  // HBM-resident reference data
  //   refT   [2B][c*s][W]  eigen-transformed CLVs, component-major (side 0 proximal, 1 distal)
  //   scSum  [B][W]        prox + dist per-site scaler counts ([B][c][W] with per-rate scalers)
  //   blen   [B]
  //   lookup [B][W][ncols]
  //   lookup2 [B][2][ceil(W/2)][36]  (start parity, site >> 1)  DNA: lookup[s][c0] + lookup[s+1][c1] over {A,C,G,T,N,none}^2
  double* refT = nullptr;
  uint32_t* scSum = nullptr;
  double* blen = nullptr;
  double* lookup = nullptr;
  double* refI = nullptr;     // c == 4: [B][c*s][W] U^-1 image of the inner CLV toward the query at
                              // the starting lengths (orig/2, orig/2), rescaled; resc0 [B][W] its flag
  uint8_t* resc0 = nullptr;
  double* cinv = nullptr;     // +I only: [W] p * pi[invariant state of the site] (0 where not invariant)
  double inv_w0 = 0.0;        // 1 / w_0: folds cinv into the zero-eigenvalue sumtable entry (thorough)
  double* lookup2 = nullptr;  // DNA only: [B][2][ceil(W/2)][36] site-pair sums (preplace.hip, k_preplace_pairs)
  // the screen's table: [ceil(B/2)][2][ceil(W/2)][36] float2 = lookup2's entries of branches 2p and 2p + 1 in fp32
  // (k_build_lookup2f; null until launch_build_lookup2f), the largest finite |entry| and the number of non-finite ones
  float2* lookup2f = nullptr;
  bool lookup2f_refused = false;   // no memory for it: the one-pass preplacement stays
  // the 16-bit screen's tables (k_build_base2 / k_build_lookup2q; null until launch_build_lookup2q): base2
  // [2][ceil(W/2)][36] = the maximum over the branches of lookup2's entry, lookup2q [ceil(B/4)][2][ceil(W/2)][36] x 4
  // int16 = the entries of branches 4p .. 4p + 3 below base2 in units of lookup2q_h
  double* base2 = nullptr;
  void* lookup2q = nullptr;
  double lookup2q_h = 0.0;
  bool lookup2q_refused = false;   // no memory for them: the fp32 screen stays
  bool screen_stats = false;       // screen_M / screen_nonfinite are set (by either table build)
  uint64_t screen_runs = 0;        // preplacements that took the two-pass route (epa_dev_preplace_screen_runs)
  double screen_M = 0.0;
  uint64_t screen_nonfinite = 0;
  // 4 states, reference built from the tree: tip_row [B] = the tip at the distal end of the branch (its row of tipmask)
  // or 0xffffffff, tipmask [tips][W] = the 4-bit state set of every tip character, tipd [16][4] = U^-1 (state set) --
  // what the TIPD instantiations of k_thorough_dna read instead of such a branch's distal block of refT
  uint32_t* tip_row = nullptr;
  uint8_t* tipmask = nullptr;
  double* tipd = nullptr;
  bool lookup_built = false;
  // the tree's geometry (treepath.hip), or null: set by epa_dev_set_topology, read by epa_dev_edpl alone
  struct EpaTopology* topo = nullptr;
  // profile queries (profile.hip): [B][s + 1][W] per (branch, site) exp(T_m - T_any) of the lookup table's pure-state
  // columns and, as component s, T_any itself; derived from `lookup` on the first profile preplacement (resident layout)
  double* prof_tab = nullptr;
  // Blocked lookup layout (EPA_FLAG_LOOKUP_BLOCKS): lookup / lookup2 / refI / resc0 stay null; every scratch bank that
  // runs a preplacement owns one block buffer -- lookup [blk][W][ncols], then (4 states) lookup2 [blk][2][ceil(W/2)][36]
  // -- rebuilt block by block inside launch_preplace (allocated exactly, on first use: epa_block_buffer)
  bool lookup_blocks = false;
  uint32_t lookup_block = 1024;   // branches per block, a multiple of 64
  std::vector<double> h_blen;

  // per-call scratch (grown on demand)
  // Banks: 0 = the direct entry points (caller's stream), 1 .. N_SLOTS = the slots of the chunk
  // pipeline, whose kernels run concurrently on their own streams and therefore share no scratch
  // (allocated on first use: a two-slot caller pays for two).
  static constexpr int N_SCRATCH = 30;   // named by EpaSlot below
  static constexpr int N_SLOTS = 24;
  static constexpr int N_BANKS = 1 + N_SLOTS;
  int bank = 0;
  void* scratch[N_BANKS * N_SCRATCH] = {};
  size_t scratch_sz[N_BANKS * N_SCRATCH] = {};

  // (NOT context state, but arguments and results of the launchers: the preplacement table's layout, PreTable; the
  // preplacement's status words, handed back by launch_preplace; the span-class histogram of a selection's pairs,
  // SelectPending::cls_hist)
  uint32_t select_cap = 64;       // staging slots per query of the candidate selection
  uint32_t* th_ctr = nullptr;  // work counters of the thorough kernel (one per XCD slice): 256 B per bank,
                               // [0, 64) the counters, [128, 256) the fused chunk's statistics
  bool code_packed4 = false;  // q_codes arrive in the 4-bit wire format (epa_dev_set_query_packing)
  int heur_mode = 0;        // EPA_HEUR_* (epa_dev_set_heuristic)
  double heur_param = 0.0;  // fixed: fraction of the branches

  // non-blocking copy streams of the chunk pipeline: uploads and downloads each have their own, so
  // the H2D of chunk k+1 is not queued behind the D2H of chunk k (which waits for k's kernels)
  hipStream_t copy_stream = nullptr, down_stream = nullptr;
  ChunkSlot slots[N_SLOTS];

  // kernel-family timers (epa_dev_last_kernel_ms): one set per scratch bank -- the pipeline slots run
  // concurrently on their own streams, a single set would have its start event re-recorded by slot k + 1
  // before slot k records its stop; t_last = the bank whose timer was stopped last
  enum { T_PREPLACE = 0, T_THOROUGH = 1, T_SELECT = 2, T_SCORE = 3, T_SITES = 4, T_RELL = 5, T_MARGINAL = 6, T_RELL_TESTS = 7, T_RELL_AU = 8, T_RELL_KH = 9, T_PREPLACE_PROFILE = 10, T_DEDUP = 11, T_EDPL = 12, T_KRD = 13, T_KRD_SORT = 14, T_KRD_TABLES = 15, T_KRD_PAIRS = 16, T_SQUASH = 17, T_SQUASH_INIT = 18, T_SQUASH_ARGMIN = 19, T_SQUASH_MERGE = 20, T_SQUASH_ROW = 21, T_EPCA = 22, T_EPCA_TABLES = 23, T_EPCA_GRAM = 24, T_EPCA_EIG = 25, T_EPCA_PROJECT = 26, N_TIMERS = 27 };
  EvTimer t_lookup;
  // blocked layout: events e[0] build e[1] preplace e[2] build ... of the bank's last chunk body (blk_ev_n valid)
  std::vector<hipEvent_t> blk_ev[N_BANKS];
  uint32_t blk_ev_n[N_BANKS] = {};
  void* blk_buf[N_BANKS] = {};
  size_t blk_sz[N_BANKS] = {};
  EvTimer t_bank[N_BANKS][N_TIMERS];
  // shares of the branch-sorted pair list the eight XCDs take in the single-wave Newton launches (cumulative, 20-bit
  // fixed point; thorough_dna.hip ThArgs::xcum), adapted to the speeds the XCDs showed: epa_xcd_feedback
  uint32_t xcd_cum[9] = {0u, 1u << 17, 2u << 17, 3u << 17, 4u << 17, 5u << 17, 6u << 17, 7u << 17, 1u << 20};
  double xcd_w[8] = {0.125, 0.125, 0.125, 0.125, 0.125, 0.125, 0.125, 0.125};
  double last_sclk_mhz = 0.0;   // shader clock of the last stamped Newton launch (s_memtime / s_memrealtime)
  bool xstamp_ok = false;   // launch_thorough: this call is ONE kernel launch (one span class): its stamps mean something
  hipEvent_t ev_rb[N_BANKS] = {};   // per bank: behind the selection's read-back copy (SelectPending::ev_rb)
  // per bank: the stream of the tip-distal Newton launches (beside the bank's own, so that one launch fills the
  // other's draining tail), forked and joined by these events
  hipStream_t side_stream[N_BANKS] = {};
  hipEvent_t ev_fork[N_BANKS] = {}, ev_join[N_BANKS] = {};
  // per bank: the statistics block / the work counters of the NEXT Newton launch were already zeroed behind the
  // selection (chunk_body_begin: in the shadow of the host's round trip); the launch that uses them clears the mark
  const void* clean_stats[N_BANKS] = {};
  bool clean_ctr[N_BANKS] = {};
  int t_last[N_TIMERS] = {};
  // epa_dev_squash records "squash_argmin", "squash_merge" and "squash_row" once per merge step: the sums over the steps
  // of the last call, and [3] the host's wall clock around its merge loop, "squash_loop_wall" (squash.hip); < 0: never
  // run, or the timers are off
  double squash_ms[4] = {-1.0, -1.0, -1.0, -1.0};
  // epa_dev_epca records "epca_eig" once per Jacobi sweep: [0] the sum over the sweeps of the last call, [1] the host's
  // wall clock around its Jacobi loop, "epca_loop_wall" (epca.hip); < 0: never run, or the timers are off
  double epca_ms[2] = {-1.0, -1.0};
  epa_thorough_stats last_stats{};
};

// the topology of epa_dev_set_topology (treepath.hip): device arrays carved from ONE allocation
struct EpaTopology {
  uint32_t n_nodes = 0, L = 0, levels = 0;
  void* base = nullptr;        // the one allocation
  const double* sparse = nullptr;
  const double* cdepth = nullptr;
  const uint32_t* cinfo = nullptr;
  const uint32_t* rank = nullptr;   // [B] pre-order position of branch b
  const uint32_t* size = nullptr;   // [B] branches in the subtree of child(b), b included
};
// releases the context's topology, if any (treepath.hip)
__attribute__((visibility("hidden"))) void epa_topology_free(epa_ctx* ctx);

// ---- helpers (epa_dev.hip)
int epa_fail(epa_ctx* ctx, int code, const std::string& msg);
void* epa_scratch(epa_ctx* ctx, int slot, size_t bytes);
// Bump carver of one scratch allocation: take<T>(n) hands out n elements and moves on to the next 256-byte boundary,
// tail(bytes) hands out the last piece as it is.  With a null base it only measures, so a layout is written ONCE, as a
// function of the carver that is run for the size (off) and again for the pointers.
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
struct Carver {
  char* base = nullptr;
  size_t off = 0;
  void* tail(size_t bytes) { char* p = base ? base + off : nullptr; off += bytes; return p; }
  template <typename T> T* take(size_t n) { return static_cast<T*>(tail(align256(sizeof(T) * n))); }
};
inline uint32_t* epa_th_ctr(epa_ctx* ctx) { return ctx->th_ctr ? ctx->th_ctr + 64 * ctx->bank : nullptr; }
// Zero `bytes` at p (and optionally a second range) with ONE plain kernel on the context's stream.  A hipMemsetAsync is
// a blit launch of its own with ~6 us of idle queue before and after it between kernels (profiles/r5_step_timeline.txt:
// five of them per chunk body); a plain kernel follows its predecessor without a gap.  Ranges must be 16-byte aligned
// multiples of 16 bytes (else: hipMemsetAsync).
int epa_zero_async(epa_ctx* ctx, void* p, size_t bytes, void* p2 = nullptr, size_t bytes2 = 0);
// the work counters of this bank's next Newton launch: zero them unless chunk_body_begin already did
// (bytes = 32: the first eight only -- the second eight belong to a tip-distal launch on the bank's side stream)
inline int epa_th_ctr_reset(epa_ctx* ctx, size_t bytes = 64) {
  if (ctx->clean_ctr[ctx->bank]) { ctx->clean_ctr[ctx->bank] = false; return 0; }
  return epa_zero_async(ctx, epa_th_ctr(ctx), bytes);
}
bool epa_is_device_ptr(const void* p);
// returns a device pointer holding `bytes` of *p (copying into scratch slot if p is on the host)
const void* epa_to_device(epa_ctx* ctx, int slot, const void* p, size_t bytes);
// query code rows -> device in the one-byte layout the kernels read (unpacks the 4-bit wire format)
const uint8_t* epa_codes_to_device(epa_ctx* ctx, const uint8_t* q_codes, uint32_t Q);
// the 4-bit wire format of Q code rows -> one byte per code, on stream st (chunk.hip: a slot's own upload)
__attribute__((visibility("hidden"))) void launch_unpack4(hipStream_t st, const uint8_t* d_packed, uint8_t* d_codes, uint32_t Q, uint32_t stride);
// a small u32 array as the host sees it: p itself, or (device memory) a copy in buf made after st has drained; null: the copy failed
__attribute__((visibility("hidden"))) const uint32_t* host_view(const uint32_t* p, size_t n, std::vector<uint32_t>& buf, hipStream_t st);
// hst: the 16 statistics words of a thorough launch ([7] start, [8 + x] last exit of XCD x: ThArgs::xstamp)
void epa_xcd_feedback(epa_ctx* ctx, uint64_t n_pairs, const unsigned long long* hst);
// what a Newton launch over n pairs left in hst: XCD feedback, ctx->last_stats (and *stats), EPA_ERR_NEG_INF (chunk.hip)
__attribute__((visibility("hidden"))) int chunk_stats(epa_ctx* ctx, uint64_t n, const unsigned long long* hst, epa_thorough_stats* stats);
// in-kernel s_memrealtime stamps are kept to 43 bits (24 h at 100 MHz) so that the XCD's share fits below them
#define EPA_XSTAMP_MASK 0x7ffffffffffull
// Kernel-family timers (hipEventRecord on the context's stream).  Each record costs ~5.5 us of idle queue between two
// kernels (profiles/r5_step_timeline.txt: six per chunk body); events riding on the launches themselves
// (hipExtLaunchKernelGGL start / stop events) were built and cost exactly the same on this runtime: not kept.
void epa_timer_start(epa_ctx* ctx, EvTimer& t);
void epa_timer_stop(epa_ctx* ctx, EvTimer& t);
// the current bank's timer of a kernel family (epa_ctx::T_*)
inline EvTimer& epa_t(epa_ctx* ctx, int which) { ctx->t_last[which] = ctx->bank; return ctx->t_bank[ctx->bank][which]; }

#define EPA_HIP(ctx, call)                                                               \
  do {                                                                                    \
    hipError_t e__ = (call);                                                              \
    if (e__ != hipSuccess)                                                                \
      return epa_fail(ctx, EPA_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e__)); \
  } while (0)

// ---- scratch slots of a bank (epa_scratch / epa_to_device).  0 .. 12: the placement path (epa_dev.hip and the
// launchers of preplace.hip, select.hip, thorough_*.hip); 0 .. 4, 7 .. 9 and 13 .. 20: the post-placement entry points
// (epa_dev_score_at, _site_lnl, _marginal_like, _rell_support, _rell_tests, _rell_au, _rell_kh) and their launchers
// (score_at.hip, marginal.hip, rell.hip); 21 .. 22: profile queries; 23 .. 25: duplicate queries (dedup.hip); 26: path
// distances (treepath.hip); 27: distances between samples (krd.hip); 28: squash clustering (squash.hip); 29: edge PCA
// (epca.hip).  Names that share a number never hold live data at the same time:
//   2   the tip map is read only by the transform kernels of epa_dev_create, queued before any call can stage a span
//       (SLOT_CLV_*, SLOT_SCALER_*: creation only, in the same way)
//   6   the preplacement's status words are read (preplace_check_status; k_pack_readback through SelectPending::
//       pre_status) inside the call that ran the preplacement, through the pointer launch_preplace handed back to it;
//       epa_dev_thorough and epa_dev_place_all keep statistics there in calls of their own, which run no preplacement,
//       and the chunk bodies keep theirs elsewhere (th_ctr, ChunkSlot::d_stats)
//   7   a Newton launch that carves its scratch here is queued on the bank's stream (or forked from it) behind the
//       k_emit_pairs that reads the selection's bitmap, and a grow goes through hipFree, which waits for the device;
//       the post-placement calls stage lengths / rule in calls of their own
//   9   epa_dev_tree_logl and the TH_TIMING build use it in calls of their own
//   10  the 4-bit codes are consumed by the unpack kernel (epa_codes_to_device) queued on the same stream ahead of the
//       fill that clears the segment maxima (launch_preplace)
// Among the post-placement calls 7 and 9 have two meanings.  A call with per-entry lengths stages them in 7 .. 9
// (EntryCall::stage); marginal_like has no lengths -- it hands the staging null for all three, so nothing of its own
// call sits there -- and keeps its rule and its waves' grid values in 7 and 9 instead.  Every call stages what it reads
// before it launches, so what the other meaning left behind in an earlier call is never read.
enum EpaSlot : int {
  SLOT_CODES = 0,         // query codes, one byte per site (epa_codes_to_device)
  SLOT_BEGIN = 1,         // win_begin [Q]
  SLOT_SPAN = 2,          // win_span [Q]
  SLOT_OUT = 3,           // the outputs the caller wants in host memory, one after the other (EntryCall::run, place_all)
  SLOT_PAIRS = 4,         // the entries' / the chunk's pairs [n]
  SLOT_CLV_PROX = 0,      // epa_dev_create: one side's CLV or tip characters of the branch being transformed
  SLOT_CLV_DIST = 1,
  SLOT_TIPMAP = 2,        // epa_dev_create: tip character -> state set
  SLOT_SCALER_PROX = 3,   // epa_dev_create: one side's scaler counts
  SLOT_SCALER_DIST = 4,
  SLOT_TABLE = 3,         // the Q x B preplacement table (host-side callers; the fused chunk body pads its rows)
  SLOT_RESULTS = 5,       // epa_result [n]
  SLOT_PREPLACE = 6,      // launch_preplace: status words (handed back to the caller) | sort, groups, packed offsets
  SLOT_STATS = 6,         // epa_dev_thorough, epa_dev_place_all: the Newton launch's 256-byte statistics block
  SLOT_SELECT = 7,        // launch_select_begin: status block | bitmap or staging form
  SLOT_NEWTON = 7,        // thorough kernels: sumtable slabs of the windows too long for registers / LDS
  SLOT_CLASS_SORT = 8,    // launch_thorough: the pair order by class key
  SLOT_TREE_LNL = 9,      // epa_dev_tree_logl: per-workgroup partial sums
  SLOT_TH_TIMING = 9,     // TH_TIMING build of thorough_dna.hip: cycle stamps
  SLOT_SEGMAX = 10,       // [Q][segp] segment maxima of the table (PreTable::segmax)
  SLOT_PACKED4 = 10,      // query codes in the 4-bit wire format, before the unpack into SLOT_CODES
  SLOT_ROWS_OUT = 11,     // epa_dev_place_all_rows: the filtered output of place_all
  SLOT_ROWS = 12,         //   and its rows
  SLOT_PENDANT = 7,       // per-entry lengths [n] each
  SLOT_DISTAL = 8,
  SLOT_PROXIMAL = 9,
  SLOT_MG_RULE = 7,       // marginal_like: x_frac [Kx] | x_logw [Kx] | p_len [Kp] | p_logw [Kp]
  SLOT_MG_WAVES = 9,      // marginal_like: [waves][Kx][Kp] grid values (launch_marginal)
  SLOT_RELL_SORT = 13,    // [keys n | idx n | sorted keys n | order n | wins n | rocprim temp]
  SLOT_RELL_BOUNDS = 14,  // [2][Q] first and one-past-last sorted position of every query
  SLOT_RELL_GROUPS = 15,  // one RellGroup per query that has entries
  SLOT_RELL_ROWS = 16,    // site rows of one batch [positions][pitch]
  SLOT_RELL_STREAMS = 17, // stream_id [Q]
  SLOT_RELL_TESTS = 18,   // rell_tests: [L n | T n | weight sums n | SH counts n]
  SLOT_RELL_AU = 19,      // rell_au: win counters [scale][n]
  SLOT_RELL_KH = 20,      // rell_kh: [L n | L_b - L n | L_k* - L n | T n | k* n | counters 3 n | matrix offsets | b | scale matrices | spilled scores]
  SLOT_PROFILE = 21,      // profile calls (profile.hip): the rows [Q][stride][s] of a call whose rows live on the host
  SLOT_PROFILE_EIGEN = 22,//   and [fault key, 256 bytes | the rows in the eigenbasis [Q][stride][s]] (k_profile_eigen)
  SLOT_DEDUP = 23,        // dedup.hip: [status | keys Q | sorted keys Q | idx Q | order Q | lead Q | flags Q + 1 | scan Q + 1 | rocprim temp]
  SLOT_DEDUP_IN = 24,     //   the chunk's codes | win_begin | win_span where the caller's live on the host (the chunk body behind
                          //   the pass stages the compacted chunk in 0 .. 2 and 10)
  SLOT_DEDUP_ROWS = 25,   //   the compacted chunk: codes | win_begin | win_span of the representatives, then rep | first for host callers
  SLOT_WEIGHT = 7,        // epa_dev_edpl (treepath.hip): weight [n]; its pairs and distal lengths in 4 and 8, its grouping in
                          //   13 and 14 as the RELL calls keep theirs, its host outputs in 3: a call of its own
  SLOT_EDPL = 26,         //   [status 256 bytes | D n | weight n | per-entry sums n | Euler index n], in grouped order
  SLOT_KRD = 27,          // epa_dev_krd (krd.hip): [status | P [S][B] | run starts S B + 1 | rank-ordered lengths and sizes B |
                          //   sort keys, indices and sorted points n | tile partials | M [S][B] when masses are asked | rocprim temp];
                          //   its inputs in 4, 7 and 8 and its host outputs in 3, as epa_dev_edpl keeps them
  SLOT_SQUASH = 28,       // epa_dev_squash (squash.hip): [D [S][S] | run starts [S][B + 1] and one spare row | two point arenas of 2 n
                          //   (x, weight, entry) | slot ids, active list, positions, new bases S each | row minima S | merge records
                          //   S | row partials S x tiles | SLOT_KRD's layout without its sorted points]; inputs and host outputs as
                          //   epa_dev_krd keeps them
  SLOT_EPCA = 29,         // epa_dev_epca (epca.hip): [XT [B][S up to 16] | the Jacobi matrix and the rotations' product [m][m] each, m = S
                          //   up to even | the circle method's pairs [m - 1][m / 2] | per-pair (c, s, t) | threshold and count | Gram
                          //   partials (tile pairs x slices x 256, at most 64 MiB a launch) | eigenvalues, columns, signs K each |
                          //   staged outputs | SLOT_KRD's layout with M]; inputs and host outputs as epa_dev_krd keeps them
};

// The entries of a post-placement call as the device sees them (EntryCall::stage, epa_dev.hip): n rows (pair, pendant,
// distal, proximal) over Q queries.  d_prx null: branch length - distal; all three lengths null: marginal_like
struct EntryStage {
  const epa_pair* d_pairs = nullptr;
  const double *d_pen = nullptr, *d_dis = nullptr, *d_prx = nullptr;
  uint64_t n = 0;
  const uint8_t* d_codes = nullptr;
  const uint32_t *d_begin = nullptr, *d_span = nullptr;
  const uint32_t* h_span = nullptr;   // the host's view of win_span
  // profile queries: eigen-space rows [Q][qe_stride][s] in place of d_codes (null: coded queries)
  const double* d_qe = nullptr;
  uint32_t qe_stride = 0;
  uint32_t Q = 0;
  uint32_t max_span = 0;              // the longest window of the Q queries
};

// ---- span classes of the thorough kernels: a launch covers pairs whose window needs the same
// kernel instantiation, so one long window does not drag a whole chunk onto the big-register
// variant.  DNA: sites per lane NCH in {1,2,3,4,6,8,12,16,24} (class 0..8), 9 = HBM-slab kernel;
// 20 states: 0 / 1 / 2 = windows up to 64 / 128 / 192 sites (k_thorough_aa_mfma<1/2/3>: sumtable
// in registers), 3 = longer (k_thorough_aa with the HBM slab).  (EPA_N_CLS of them, EPA_N_CLSX class keys: above)
__host__ __device__ inline bool epa_tip_class_ok(int cls) { return cls <= 2 || cls == 10 || cls == 11; }
__host__ __device__ inline int epa_tip_class(int cls) { return cls <= 2 ? 12 + cls : cls == 10 ? 15 : cls == 11 ? 16 : cls; }
__host__ __device__ inline int epa_base_class(int key) { return key < 12 ? key : key <= 14 ? key - 12 : key == 15 ? 10 : 11; }
// the context forms tip-distal keys: what the TIPD kernels serve (four categories, exact zero eigenvalue, sliding
// BLO, no +I) with the tip table of a reference built from the tree, unless the option tip_distal is 0
inline bool epa_tipd_active(const epa_ctx* ctx) {
  return ctx->tip_row && ctx->opt.tip_distal && ctx->s == 4 && !ctx->generic_thorough && ctx->dna.ng == 1 &&
         ctx->dna_zero0 && ctx->blo.sliding && !ctx->cinv;
}
constexpr uint32_t EPA_AA_LDS_MAX_SPAN = 102;
__host__ __device__ inline int epa_span_class(int states, uint32_t span) {
  if (states != 4) return span <= 64 ? 0 : span <= 128 ? 1 : span <= 192 ? 2 : 3;
  // DNA classes 10 / 11: windows of 65..96 / 129..160 sites, whose last 64-lane chunk is at most half
  // full: the half-chunk instantiations of k_thorough_dna (thorough_dna.hip, TAILH)
  if (span > 64 && span <= 96) return 10;
  if (span > 128 && span <= 160) return 11;
  const uint32_t nch = (span + 63) / 64;
  return nch <= 4 ? (nch ? (int)nch - 1 : 0) : nch <= 6 ? 4 : nch <= 8 ? 5 : nch <= 12 ? 6 : nch <= 16 ? 7 : nch <= 24 ? 8 : 9;
}

// ---- kernel launchers
int launch_transform(epa_ctx* ctx, const double* d_clv_or_null, const uint8_t* d_tip_or_null,
                     const uint32_t* d_tipmap, uint32_t tipmap_size, double* dst);
int launch_build_lookup(epa_ctx* ctx);
int launch_build_lookup2(epa_ctx* ctx);  // DNA site-pair table from `lookup` (preplace.hip)
// the fp32 branch-pair table of the screen from lookup2, with screen_M / screen_nonfinite (synchronises the stream)
int launch_build_lookup2f(epa_ctx* ctx);
// The screen's error bound for windows of at most span_bound sites: with u = 2^-24 and n gathered entries of magnitude
// <= M, |fp32 sum - fp64 sum| <= (n + 1) u n M (every entry rounded once, n - 1 additions); delta is twice that, times
// the option preplace_screen_scale.  < 0: no screen for this context (a non-finite entry, or delta > 1).
double epa_screen_delta(const epa_ctx* ctx, uint32_t span_bound);
// The 16-bit screen's quantum and error bound for windows of at most span_bound sites, n gathered entries: every entry
// is rounded to a multiple of h once (<= h / 2 each, integer addition is exact), C_q is a sum of n fp64 terms of
// magnitude <= M and C_q + h seg one more fp64 operation: delta = n h / 2 + (n + 2) n M 2^-53.  *h = the largest power of
// two that keeps this <= 1, made smaller by the option preplace_screen_i16_shift; the returned delta is for that *h and
// multiplied by preplace_screen_scale.  < 0: no 16-bit screen (no statistics, a non-finite entry, or delta > 1).
double epa_screen16_delta(const epa_ctx* ctx, uint32_t span_bound, double* h);
// base2 (once, with the table statistics: synchronises the stream) and lookup2q for the quantum h (again whenever h
// changes: a power of two, so only when the chunks' longest window moves across a few fixed lengths)
int launch_build_lookup2q(epa_ctx* ctx, uint32_t span_bound);
// what a screen-only run of launch_preplace leaves behind (device pointers into SLOT_PREPLACE, valid until the bank's
// next preplacement): the tests' and the measurements' view of the screen
struct PreScreenProbe {
  double band_t = 0.0;                   // in: the selection's band (launch_select_begin)
  bool ran = false;                      // the screen's conditions held
  bool i16 = false;                      // in: probe the 16-bit screen (else the fp32 screen, whatever the option says)
  double delta = 0.0;
  double h = 0.0;                        // 16-bit screen: the quantum
  const double* cq = nullptr;            // 16-bit screen: [Q] C_q
  const uint32_t* seg32 = nullptr;       // [Q][segp] keys of the segment maxima (seg_key32, or integer + 32769), 0 = none
  const unsigned long long* mask = nullptr;    // [Q] included segments
  const unsigned long long* n_incl = nullptr;  // their total
  float ms_screen = -1.f, ms_band = -1.f;
};
// blocked layout: branches per block buffer in effect, its bytes (lookup rows first, lookup2 rows at *off2), the
// current bank's buffer (allocated on first use) and the build of the tables of branches [b0, b0 + nb) into it
uint32_t epa_block_branches(const epa_ctx* ctx);
size_t epa_block_bytes(int s, uint32_t W, uint32_t blk, size_t* off2);
void* epa_block_buffer(epa_ctx* ctx);
int launch_build_lookup_block(epa_ctx* ctx, uint32_t b0, uint32_t nb, double* blk_lookup);
int launch_build_lookup2_block(epa_ctx* ctx, uint32_t nb, const double* blk_lookup, double* blk_lookup2);
// fills t.lnl (and, after clearing them, t.segmax when given); *d_status: the call's status words in SLOT_PREPLACE,
// [0 .. 4) the window validation -- for preplace_check_status after a synchronisation, or for the selection's read-back
// probe: run the screen it names (fp32, or 16 bit with probe->i16) and its band test INSTEAD of the table kernels and report
// them (t.lnl is not written)
int launch_preplace(epa_ctx* ctx, const uint8_t* d_codes, const uint32_t* d_begin, const uint32_t* d_span, uint32_t Q,
                    const PreTable& t, uint32_t max_span, const uint32_t** d_status, PreScreenProbe* probe = nullptr);
int preplace_check_status(epa_ctx* ctx, const uint32_t* d_status);
__attribute__((visibility("hidden"))) int preplace_window_error(epa_ctx* ctx, const uint32_t* st);   // the two window-validation words -> error code and text
// one workgroup: exclusive scan of cnt[0 .. K) in place; with tip_row also *tip_total = the sum over the first K - 1
// entries whose tip_row is not 0xffffffff (k_scan_counts, preplace.hip: the counting sort's and the selection's scan)
__attribute__((visibility("hidden"))) void launch_scan_counts(epa_ctx* ctx, uint32_t* cnt, uint32_t K, const uint32_t* tip_row = nullptr,
                                                               uint32_t* tip_total = nullptr);
int launch_thorough(epa_ctx* ctx, const epa_pair* d_pairs, uint64_t n_pairs, const uint8_t* d_codes,
                    const uint32_t* d_begin, const uint32_t* d_span, uint32_t max_span,
                    epa_result* d_out, unsigned long long* d_stats,
                    const uint32_t* cls_hist = nullptr);   // [EPA_N_CLS] span classes of exactly these pairs, or null: counted here
int launch_thorough_queued(epa_ctx* ctx, const epa_pair* d_pairs, const uint32_t* d_spec, uint64_t max_pairs,
                           const uint8_t* d_codes, const uint32_t* d_begin, const uint32_t* d_span, uint32_t max_span,
                           epa_result* d_out, unsigned long long* d_stats);
int launch_select_emit(epa_ctx* ctx, SelectPending* sp);   // queues the guarded k_emit_pairs behind launch_select_begin
int launch_thorough_aa(epa_ctx* ctx, const epa_pair* d_pairs, const uint32_t* d_order, uint64_t n_pairs,
                       const uint8_t* d_codes, const uint32_t* d_begin, const uint32_t* d_span,
                       uint32_t max_span, bool want_lds, epa_result* d_out, unsigned long long* d_stats);
int launch_thorough_generic(epa_ctx* ctx, const epa_pair* d_pairs, uint64_t n_pairs, const uint8_t* d_codes,
                            const uint32_t* d_begin, const uint32_t* d_span, uint32_t max_span,
                            epa_result* d_out, unsigned long long* d_stats,
                            const uint32_t* d_order = nullptr, bool caller_times = false,   // caller_times: a per-class launch inside launch_thorough's timed region
                            const double* d_qe = nullptr, uint32_t qe_stride = 0);   // d_qe: profile queries, eigen-space rows [Q][qe_stride][s] in place of d_codes
int launch_thorough_aa_mfma(epa_ctx* ctx, const epa_pair* d_pairs, const uint32_t* d_order, uint64_t n_pairs,
                            const uint8_t* d_codes, const uint32_t* d_begin, const uint32_t* d_span,
                            uint32_t max_span, epa_result* d_out, unsigned long long* d_stats);
// lookup column -> state set (epa_dev.hip)
__attribute__((visibility("hidden"))) uint32_t epa_column_mask(int s, int col);
// Profile queries (profile.hip): the rows of a call checked (host rows here, device rows by the kernel's fault key; the
// first offending query and position are named), staged and brought to the eigenbasis.  hb / hs: the host's view of the
// windows, checked against the width and the stride; *d_prof: the rows in HBM, *d_qe: their eigen-space image
__attribute__((visibility("hidden"))) int epa_profile_stage(epa_ctx* ctx, const char* who, const double* prof, uint32_t stride,
                                                            const uint32_t* hb, const uint32_t* hs, const uint32_t* d_span, uint32_t Q,
                                                            bool allow_empty, uint32_t* max_span, const double** d_prof, const double** d_qe);
// lnL of the entries at their lengths (score_at.hip); e.d_qe set: profile queries
int launch_score_at(epa_ctx* ctx, const EntryStage& e, double* d_lnl);
// per-site log-likelihoods of the same entries (k_score_at<S, true>): row i of d_rows [n_rows][pitch] takes entry
// d_order[i] (null: entry i), columns [0, span).  SITES_PAD: the columns from the span up to the pitch are written as
// 0.0; SITES_TIMED: records the "site_lnl" timer (the RELL driver times the whole call under its own instead)
enum SiteLnlFlags : unsigned { SITES_PLAIN = 0u, SITES_PAD = 1u, SITES_TIMED = 2u };
int launch_site_lnl(epa_ctx* ctx, const EntryStage& e, const uint32_t* d_order, uint64_t n_rows, uint32_t pitch,
                    double* d_rows, unsigned flags);
// The RELL calls (rell.hip): the entries compete per query; e.n < 2^32.  Which replicates are drawn:
struct RellDraws {
  const uint64_t* d_stream_id;   // [Q] or null: the query's index
  uint32_t replicates;
  uint64_t seed;
};
// The entries of a call grouped by query (rell.hip): a stable radix sort of the entry indices by seq_id, so a group keeps
// the caller's entry order.  sorted [n]: the seq_ids in grouped order; order [n]: grouped position -> entry; bounds
// [2][Q]: first and one-past-last grouped position of every query that has entries, 0 and 0 for the others (a seq_id >= Q
// owns no run); extra: extra_arrays x n further words of the same allocation for the caller (256-byte pitch), or null.
// SLOT_RELL_SORT and SLOT_RELL_BOUNDS; queued on the context's stream, nothing is waited for
struct EntryGroups {
  uint32_t *sorted, *order, *bounds, *extra;
};
__attribute__((visibility("hidden"))) int launch_group_entries(epa_ctx* ctx, const epa_pair* d_pairs, uint32_t n, uint32_t Q,
                                                               uint32_t extra_arrays, EntryGroups* g);
// bootstrap support [n]
int launch_rell(epa_ctx* ctx, const EntryStage& e, const RellDraws& dr, double* d_support);
// support, expected likelihood weights and SH p-values from the same replicates; each output [n] or null
int launch_rell_tests(epa_ctx* ctx, const EntryStage& e, const RellDraws& dr, double* d_support, double* d_elw, double* d_p_sh);
// AU p-values from multiscale replicates: h_scale_pm [n_scales <= 16] per mille (host); d_p_au [n], d_counts
// [n_scales][n], d_fit [n][2], each or null
int launch_rell_au(epa_ctx* ctx, const EntryStage& e, const RellDraws& dr, const uint32_t* h_scale_pm, uint32_t n_scales,
                   double* d_p_au, uint32_t* d_counts, double* d_fit);
// p-values of the KH, the weighted KH and the weighted SH test from the replicates of launch_rell; each output [n] or null.
// At most 1024 entries per query.  Not exported: the call adds one symbol to the library, its entry point
__attribute__((visibility("hidden"))) int launch_rell_kh(epa_ctx* ctx, const EntryStage& e, const RellDraws& dr, double* d_p_kh, double* d_p_wkh, double* d_p_wsh);
// marginal likelihood of the entries' pairs over a (distal x pendant) tensor rule (marginal.hip); d_rule: x_frac [Kx] |
// x_logw [Kx] | p_len [Kp] | p_logw [Kp]; d_grid: [n][Kx][Kp] or null
int launch_marginal(epa_ctx* ctx, const EntryStage& e, const double* d_rule, uint32_t Kx, uint32_t Kp, double* d_marginal,
                    double* d_grid);
// candidate selection (select.hip) from table t; pre_status: the status words of the preplacement that wrote t (their
// window validation travels in the read-back: select_check_status), or null when the table came from elsewhere
int launch_select(epa_ctx* ctx, const PreTable& t, const uint32_t* pre_status, uint32_t Q, double threshold,
                  epa_pair* d_pairs, uint64_t max_pairs, uint64_t* n_pairs,
                  const uint32_t* d_span = nullptr);  // d_span: also histogram the span classes
int launch_select_begin(epa_ctx* ctx, const PreTable& t, const uint32_t* pre_status, uint32_t Q, double threshold,
                        epa_pair* d_pairs, uint64_t max_pairs, const uint32_t* d_span, uint32_t* rb, SelectPending* sp);
int launch_select_end(epa_ctx* ctx, SelectPending* sp, uint64_t* n_pairs);
int select_check_status(epa_ctx* ctx, const SelectPending* sp);
