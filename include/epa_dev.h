/*
 * epa_dev.h -- C-ABI of the MI355X placement evaluator (libepa_dev.so).
 *
 * This is the drop-in boundary for EPA-ng's placement hot path.  The reference has no FFI for
 * this path; the seam is the pair of static templates called from the chunk loop
 *     place(chunk, tree, branches, preplace, options, lookups)            src/core/place.cpp:41-95,221
 *     place_thorough(blo_work, chunk, tree, branches, blo_sample, ...)    src/core/place.cpp:97-171,234
 * and, below them, the per-branch evaluator
 *     Tiny_Tree::Tiny_Tree(edge, branch_id, Tree&, opt_branches, ...)     src/tree/Tiny_Tree.cpp:48-129
 *     Placement Tiny_Tree::place(const Sequence&)                         src/tree/Tiny_Tree.cpp:131-218
 * together with the libpll / pll-modules calls they wrap.
 * Paths are relative to the reference checkout.  INTEGRATION.md shows the reference-side binding.
 *
 * Conventions
 *  - plain C, no torch / HIP types; every `const T*` data argument may be a host pointer or a
 *    device (HBM) pointer -- the library inspects it (hipPointerGetAttributes) and copies only
 *    when it lives on the host.  Outputs follow the same rule.
 *  - all likelihood arithmetic is fp64.
 *  - every entry point returns EPA_OK or a negative epa_status; epa_dev_last_error() returns
 *    the message the reference would have thrown (std::runtime_error text) where one exists.
 *  - one epa_ctx per GPU; a ctx is thread-compatible (one caller at a time), entry points are
 *    called once per chunk, outside any OpenMP region.
 */
#ifndef EPA_DEV_H
#define EPA_DEV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct epa_ctx epa_ctx;

typedef enum {
  EPA_OK = 0,
  EPA_ERR_INVALID_ARG = -1,   /* bad descriptor / null pointer / unsupported shape            */
  EPA_ERR_HIP = -2,           /* HIP runtime failure (message carries hipGetErrorString)       */
  EPA_ERR_NO_DEVICE = -3,     /* no gfx950 device visible: there is NO CPU fallback            */
  EPA_ERR_QUERY_WIDTH = -4,   /* "Query sequence length not same as reference alignment!"      *
                               *   Tiny_Tree.cpp:145-147                                       */
  EPA_ERR_QUERY_ALL_GAP = -5, /* "... does not appear to have any non-gap sites!" :153-156     */
  EPA_ERR_INVALID_CHAR = -6,  /* "char is invalid!" Lookup_Store.hpp:100-108 (quirk D5: the     *
                               *   reference does not validate; this library does on ingest)   */
  EPA_ERR_NEG_INF = -7,       /* "-INF logl at branch ..." Tiny_Tree.cpp:209-212               */
  EPA_ERR_UNSUPPORTED = -8,   /* feature marked "next" in SURVEY.md section 8f                 */
  EPA_ERR_PAIR_OVERFLOW = -9, /* the candidate selection found more pairs than max_pairs: call    *
                               *   again with larger buffers (a staged chunk stays staged)       */
  EPA_ERR_NO_MEMORY = -10     /* the reference does not fit the device (or the cap of            *
                               *   epa_dev_set_mem_cap): the message names needed and usable bytes */
} epa_status;

/* flags of epa_ref_desc.flags */
#define EPA_FLAG_SLIDING_BLO 0x1u  /* Options::sliding_blo (default on, src/util/Options.hpp:16) */
#define EPA_FLAG_RAXML_BLO 0x4u    /* --raxml-blo: pllmod_opt_optimize_branch_lengths_local, radius 1 *
                                    * (src/core/pll/optimize.cpp:274-279) instead of the sliding rule */
/* pllmod_opt_minimize_newton is not in the reference's tree; the routine this library replicates
 * by default is a recollection (see oracle/epa_oracle.c minimize_newton).  Two details differ
 * between published variants of it and are switchable (profiles/r2_sensitivity.md measures what
 * they change): */
#define EPA_FLAG_NEWTON_SLOW_BISECT 0x8u  /* also bisect when |2 f| > |dx_old f'| (Numerical Recipes rtsafe) */
#define EPA_FLAG_NEWTON_STRICT_DF 0x10u   /* first convergence test needs f' > 0 instead of f' >= 0          */
#define EPA_FLAG_KEEP_EIGENVALUES 0x20u   /* use the caller's eigenvalues verbatim: by default the stationary one
                                          * (a few 1e-17 of either sign out of libpll's eigen-solver, 0 in exact
                                          * arithmetic) is set to exactly 0 and the kernels drop its derivative terms.
                                          * With this flag nothing is snapped and the general kernel evaluates every
                                          * term as libpll does: the switch to A/B the snap against a real libpll
                                          * build (at saturated lengths the residue's sign decides a bisection,
                                          * DESIGN section 2).  Not available with prop_invar > 0. */
#define EPA_FLAG_RATE_SCALERS 0x2u /* PLL_ATTRIB_RATE_SCALERS: every rate category is rescaled on its *
                                    * own (src/tree/tiny_util.cpp:37-44; the reference turns it on    *
                                    * above 2000 tips, src/io/file_io.cpp:211-214, or with            *
                                    * --rate-scalers).  prox_scaler / dist_scaler rows are then      *
                                    * [W][rate_cats] (libpll layout)                                  */

/* Layout of the derived per-branch tables (lookup, lookup2, refI / resc0).  Neither bit: all of
 * them resident, [B]-sized, built once (805 B per branch x site for a 4-state, 4-category reference, 2117 B for 20
 * states).  EPA_FLAG_LOOKUP_BLOCKS: only refT / scSum stay resident (260 / 1284 B); every scratch bank that runs a
 * preplacement owns ONE block buffer of `lookup_block` branches, whose tables are rebuilt block by block inside every
 * chunk body, and the Newton kernels compute their own starting vectors.  Preplacement tables and candidate lists are the
 * same bits either way; the Newton results are not: a kernel that forms its starting vector itself rounds differently
 * from the lookup build that stores it -- measured, lnL within 3.4e-12 and lengths within 2.5e-14 of the resident layout
 * (a few ulp; both within the 1e-6 the tests hold against the oracle).
 * EPA_FLAG_LOOKUP_AUTO: resident when epa_dev_lookup_plan() says it fits the device's free memory (or the cap of
 * epa_dev_set_mem_cap), blocks otherwise. */
#define EPA_FLAG_LOOKUP_BLOCKS 0x40u
#define EPA_FLAG_LOOKUP_AUTO 0x80u

/*
 * Reference-side inputs: what Tiny_Tree's constructor pulls out of `Tree` per branch
 * (Tree::get_clv for the proximal and distal node, their scalers, the branch length:
 * src/tree/tiny_util.cpp:72-199) plus the model arrays the tiny partition shares by pointer
 * (:109-163).  Arrays use libpll's layouts: CLV [site][rate_cat][state] fp64, scaler
 * uint32[site] (or uint32[site][rate_cat] with EPA_FLAG_RATE_SCALERS).
 * Branch b is EPA-ng's branch_id == jplace edge_num (utree_query_branches order,
 * src/core/pll/pll_util.cpp:182-205).  Orientation is the caller's job exactly as in
 * Tiny_Tree.cpp:64-74: when one end of the branch is a tip it is passed as the DISTAL side.
 */
#define EPA_MAX_CATS 16 /* most rate categories a reference may have (the kernels' table sizes) */
typedef struct {
  uint32_t states;     /* 4 (DNA) or 20 (AA)                                                   */
  uint32_t rate_cats;  /* number of rate categories c, 1 .. EPA_MAX_CATS                       */
  uint32_t sites;      /* alignment width W after column pre-masking                           */
  uint32_t branches;   /* B = 2n-3                                                             */

  /* eigen system of the (single) rate matrix:  P(t) = U diag(exp(eigenvals r_k t)) U^-1.
   * libpll stores U as `inv_eigenvecs` and U^-1 as `eigenvecs` (pll_update_eigen).           */
  const double* eigenvals;   /* [states]                                                       */
  const double* eigenvecs_u; /* [states*states] row-major U                                    */
  const double* eigenvecs_uinv; /* [states*states] row-major U^-1                              */
  const double* freqs;       /* [states] stationary frequencies                                */
  const double* rates;       /* [rate_cats]                                                    */
  const double* rate_weights;/* [rate_cats]                                                    */
  double prop_invar;         /* proportion of invariant sites (+I), 0 <= p < 1; see invariant_state */

  /* per branch: B pointers each */
  const double* const* prox_clv;       /* [B] -> [W][c][s]                                     */
  const uint32_t* const* prox_scaler;  /* [B] -> [W], entry or whole array may be NULL (= 0)   */
  const double* const* dist_clv;       /* [B] -> [W][c][s]; NULL where dist_tipchars[b] is set */
  const uint8_t* const* dist_tipchars; /* [B] -> [W] tip codes (index into tipmap); may be NULL */
  const uint32_t* const* dist_scaler;  /* [B] -> [W], NULL for tips                            */
  const double* branch_length;         /* [B] original branch length                           */

  /* tip code -> state set (pll_map_nt / pll_map_aa semantics): bit i = state i allowed.
   * Used for dist_tipchars only; query codes are lookup columns, see epa_dev_preplace.        */
  const uint32_t* tipmap;
  uint32_t tipmap_size;

  /* constants of the branch-length optimiser.  They live in headers absent from the reference
   * tree (pll_optimize.h), hence runtime parameters; 0 selects the default in brackets.       */
  double blo_min_branch;     /* PLLMOD_OPT_MIN_BRANCH_LEN      [1e-4]  optimize.hpp:11          */
  double blo_max_branch;     /* PLLMOD_OPT_MAX_BRANCH_LEN      [100]   optimize.hpp:12          */
  double blo_default_branch; /* PLLMOD_OPT_DEFAULT_BRANCH_LEN  [0.1]   optimize.cpp:143         */
  double blo_epsilon;        /* OPT_BRANCH_EPSILON             [0.1]   optimize.hpp:9           */
  double pendant_default;    /* DEFAULT_BRANCH_LENGTH          [-ln 0.9] util/constants.hpp:12  */
  uint32_t blo_max_rounds;   /* smoothings                     [32]    optimize.cpp:269         */
  uint32_t blo_max_newton;   /* max_iters                      [30]    optimize.cpp:62          */
  uint32_t flags;            /* EPA_FLAG_*; neither BLO bit set selects EPA_FLAG_SLIDING_BLO     */
  uint32_t aa_x_as_n;        /* 1: reproduce quirk D4 (AA 'X' preplaced in the 'N' column,      *
                              *    Lookup_Store.hpp:63-66); 0 (default): 'X' = any             */
  /* +I: state of every site that is invariant over the REFERENCE tips (libpll
   * pll_update_invariant_sites: AND of the tips' state sets is a single state), -1 otherwise;
   * the array the tiny partition borrows at src/tree/tiny_util.cpp:153-156.  [sites]; required
   * by epa_dev_create when prop_invar > 0, optional for epa_dev_create_from_tree (derived from
   * the tip sequences when NULL).  With +I the library follows libpll: rates are divided by
   * (1 - p) in every P-matrix, a site's likelihood is (1-p) L + p pi_state (the second term is
   * added unscaled and regardless of the query's character, as libpll does).                  */
  const int8_t* invariant_state;
} epa_ref_desc;

/*
 * Reference precompute ON the device: instead of 2B host CLVs the caller hands over the tree and
 * the tip sequences and the library computes all 3(n-2) directional CLVs itself (the job of
 * precompute_clvs, src/core/pll/epa_pll_util.cpp:62-107 / Tree::Tree, src/tree/Tree.cpp:16-56),
 * level by level, directly in the eigen-transformed layout the kernels use (nothing but n x W
 * tip codes crosses PCIe).  `ref` carries the model, sizes, tip map, branch lengths and optimiser
 * constants; its per-branch CLV / scaler pointer arrays are ignored.
 * A directional CLV record r is the partial likelihood of the subtree seen from one end of a
 * branch; it is the product of its two children propagated over their branches.  Operand ids:
 * value < inner_records = record, EPA_TIP | t = tip t.  Every inner record must be the proximal
 * or distal side of exactly one branch; a tip end is always passed as the DISTAL side.
 */
#define EPA_TIP 0x80000000u
typedef struct {
  epa_ref_desc ref;
  uint32_t tips;                  /* n                                                          */
  uint32_t inner_records;         /* 3 (n - 2)                                                  */
  const uint8_t* tipchars;        /* [n][sites] tip codes (index into ref.tipmap)               */
  const uint32_t* rec_child_a;    /* [inner_records] operand ids of the two children            */
  const uint32_t* rec_child_b;
  const double* rec_length_a;     /* [inner_records] branch length toward each child            */
  const double* rec_length_b;
  const uint32_t* branch_prox;    /* [B] operand id of the proximal side (an inner record)      */
  const uint32_t* branch_dist;    /* [B] operand id of the distal side (record or tip)          */
} epa_tree_desc;

/* one unit of Work (src/core/Work.hpp:31-34 Work_Pair) */
typedef struct {
  uint32_t branch_id;
  uint32_t seq_id; /* index into the chunk's queries */
} epa_pair;

/* one Placement minus the LWR (src/sample/Placement.hpp:48-53) */
typedef struct {
  double lnl;
  double pendant_length;
  double distal_length;
} epa_result;

/* Counters of the last epa_dev_thorough call (optional diagnostics). */
typedef struct {
  uint64_t pairs;
  uint64_t rounds;       /* outer pplacer rounds over all pairs                               */
  uint64_t newton_evals; /* derivative evaluations over all pairs                             */
  uint64_t reverts;      /* pairs that hit the "worse -> restore" exit, optimize.cpp:224-232  */
} epa_thorough_stats;

/* Number of GPUs visible (0 => every other entry point fails with EPA_ERR_NO_DEVICE). */
int epa_dev_device_count(void);

/*
 * Replaces: Tree::get_clv + make_tiny_partition + make_tiny_tree_structure for every branch
 * (src/tree/tiny_util.cpp:72-306) -- copies the reference data to HBM once, transformed into the
 * eigenbasis of the model -- and the per-branch part of Tiny_Tree::Tiny_Tree + Lookup_Store
 * (src/tree/Tiny_Tree.cpp:88-128, src/core/Lookup_Store.hpp:73-81): the per-branch per-site
 * lookup tables are built on device by epa_dev_build_lookup (called lazily by preplace).
 */
int epa_dev_create(const epa_ref_desc* desc, int device, epa_ctx** out);
void epa_dev_destroy(epa_ctx* ctx);
const char* epa_dev_last_error(const epa_ctx* ctx); /* ctx may be NULL: last create() error */

/* Same context, reference CLVs computed on the device from the tree (see epa_tree_desc). */
int epa_dev_create_from_tree(const epa_tree_desc* tree, int device, epa_ctx** out);

/* Log-likelihood of the reference tree evaluated at branch `branch` (Tree::ref_tree_logl,
 * src/tree/Tree.cpp:119-131; equal on every branch up to rounding). */
int epa_dev_tree_logl(epa_ctx* ctx, uint32_t branch, double* lnl);

/* Optional: run all kernels of `ctx` on this hipStream_t (passed as void*). Default stream 0. */
int epa_dev_set_stream(epa_ctx* ctx, void* hip_stream);

/*
 * Diagnostic switches of a context, no reference counterpart.  Every switch selects between code paths that return
 * the same results (cross-check kernels of the parity tests, A/B switches of the bench); the library reads NO
 * environment variable for its compute path (RCCL's location and timeout excepted: EPA_RCCL_LIB, EPA_COMM_TIMEOUT_S).
 *   "thorough_generic"  1: every Newton launch on the general kernel (k_thorough_generic, the reference-shaped loop)
 *   "preplace_generic"  1: preplacement on k_preplace (one gather per site) instead of the pair / site fast paths
 *   "select_full_rows"  1: candidate selection from whole table rows instead of the segment maxima
 *   "select_sort"       1: candidate list through staging rows + a stable sort instead of the [B][Q] bitmap
 *   "queued_thorough"   1: the Newton launch queued behind the selection, guarded by the device-side count
 *   "xcd_balance"       0: the eight XCDs keep equal shares of a Newton launch (default 1: epa_dev_xcd_shares)
 *   "aa_valu"           1: 20-state windows on the lane = site VALU kernel instead of the matrix-core kernel
 *   "timers"            0: no hipEvent records around the kernel families (epa_dev_last_kernel_ms returns < 0)
 *   "lookup_block"      n: branches per block buffer of a context in the blocked lookup layout (default 1024, or what
 *                          epa_dev_lookup_plan shrank it to); a positive multiple of 64, before the first preplacement.
 *                          EPA_ERR_INVALID_ARG on a resident context
 *   "newton_lds"        1: the single-wave 4-state Newton kernels (windows up to 256 sites, exact zero eigenvalue,
 *                          sliding BLO) read their per-evaluation table through LDS instead of broadcasting it from registers
 *                          by DPP (default 0: DPP; bit-identical results)
 *   "tip_distal"        0: every pair on the row form of the single-wave 4-state Newton kernels (default 1: pairs whose
 *                          branch ends in a tip -- contexts created from the tree -- are launched apart on kernels that
 *                          read the tip's 4-bit state set per site instead of 16 rows of its eigen image; bit-identical
 *                          results)
 *   "dedup_key_bits"    n: the duplicate search (epa_dev_dedup_queries) keeps only the low n bits of a query's 64-bit key,
 *                          n = 0 .. 64 (default 64), else EPA_ERR_INVALID_ARG.  Classes do not depend on it: fewer bits give
 *                          unequal rows one key, and the exact comparison takes them apart again (what the tests force).
 *                          A run of m rows in k classes costs up to m k row comparisons: not for large chunks
 *   "dedup_sort_bits"   n: the low key bits its sort looks at, n = 0 .. 64 (default 32: four digit passes; rows that agree
 *                          there share a run and are parted by the full key first, then by their codes).  Classes do not
 *                          depend on it either
 *   "preplace_screen"   0: the chunk body's 4-state preplacement always fills the whole table in one pass (default 1: where
 *                          the selection reads by segment maxima -- dynamic rule, threshold < 1, at most 4096 branches,
 *                          resident tables, windows of one chunk -- and the chunk is large enough to pay for it -- reads x
 *                          branches >= 8e7, and at most ~ 4 million (read, 64-branch segment) cells, the limit of the cell
 *                          grouping's run table -- an fp32 pass over branch pairs finds the 64-branch segments that can
 *                          matter and only those are summed exactly; same candidates, same results.  2: the same without
 *                          the lower size condition, for tests.  The first screening chunk builds an fp32 table of half
 *                          the site-pair table's size, if 4 GiB stay free behind it)
 *   "preplace_screen_scale" n: test only, the screen's error bound is multiplied by n >= 1 (default 1); a bound above
 *                          1 lnL unit turns the screen off for the context
 *   "preplace_screen_i16" 0: the screen runs in fp32 over branch pairs (default 1: where the fp32 screen would run, and a
 *                          16-bit bound of at most 1 lnL unit holds, it runs over branch quads in 16-bit fixed point relative
 *                          to the per-slot maximum over the branches, quantum h = the largest power of two with bound <= 1,
 *                          2^-6 for 150-site reads; its tables take a quarter of the site-pair table's size, under the same
 *                          4 GiB rule, and the fp32 table is then not built; same candidates, same results)
 *   "preplace_screen_i16_shift" n: test only, h is made smaller by n powers of two (default 0): sums saturate earlier
 * Unknown key: EPA_ERR_INVALID_ARG.
 */
int epa_dev_set_option(epa_ctx* ctx, const char* key, int value);

/* Builds T[b][site][col] for all branches (idempotent).  Replaces precompute_sites_static x C
 * + Lookup_Store::init_branch (Tiny_Tree.cpp:18-46,114-128).  A context in the blocked lookup layout
 * builds its tables inside the chunk body: the call does nothing there and returns EPA_OK. */
int epa_dev_build_lookup(epa_ctx* ctx);

/*
 * Device memory of a reference, computed on the host (no device needed) with create's own padding rules:
 * nucleotide categories padded to a multiple of four, 1 or 2 categories replicated to four, lookup2 over
 * ceil(W / 2) site pairs.  flags: the EPA_FLAG_* the context would be created with (the lookup bits choose the
 * layout that is priced: EPA_FLAG_LOOKUP_BLOCKS = blocks, anything else = resident); from_tree: priced for
 * epa_dev_create_from_tree, whose per-side scaler counts and tip rows live until create returns;
 * block_branches: branches per block buffer (0 = the default 1024; at most B rounded up to 64 are allocated);
 * banks: scratch banks that will run a preplacement (the direct entry points are one, every pipeline slot in
 * use another).  refi is counted for the shapes the tuned Newton kernels serve (a proper GTR is assumed).
 * Not counted, because it is optional: the path-distance table of epa_dev_set_topology, 8 (2 n - 1) (floor(log2(2 n - 1)) + 1)
 * + 20 B bytes for n = B + 1 nodes (20.2 MB at 65 537 branches).
 */
typedef struct {
  uint64_t reft;          /* both CLVs of every branch in the eigenbasis                                  */
  uint64_t scsum;         /* per-site scaler counts                                                       */
  uint64_t lookup;        /* resident layout only: lookup [B][W][16 or 24]                                */
  uint64_t lookup2;       /* resident layout, 4 states only: lookup2 [B][2][ceil(W/2)][36]                */
  uint64_t refi;          /* resident layout, tuned Newton kernels only: refI + resc0                     */
  uint64_t misc;          /* branch lengths, model block, work counters                                   */
  uint64_t create_temp;   /* from_tree: buffers of the precompute, released before create returns         */
  uint64_t reference;     /* reft + scsum + lookup + lookup2 + refi + misc                                */
  uint64_t bank;          /* blocked layout: one block buffer (lookup + lookup2 rows of a block)          */
  uint64_t steady;        /* reference + banks x bank                                                     */
  uint64_t peak;          /* max(steady, reference + create_temp)                                         */
} epa_footprint;
int epa_dev_footprint(uint32_t states, uint32_t rate_cats, uint64_t sites, uint64_t branches, int flags, int from_tree,
                      uint32_t block_branches, int banks, epa_footprint* out);

/* Chooses the layout for `usable_bytes`: *mode = EPA_LOOKUP_RESIDENT when the resident peak fits (and flags do not
 * force blocks); else EPA_LOOKUP_BLOCKS with the largest *block_branches <= 1024 (a multiple of 64, at least 64)
 * whose peak fits; else EPA_ERR_NO_MEMORY (epa_dev_last_error(NULL) names needed and usable bytes).
 * Non-decreasing in usable_bytes. */
#define EPA_LOOKUP_RESIDENT 0
#define EPA_LOOKUP_BLOCKS 1
int epa_dev_lookup_plan(uint64_t usable_bytes, uint32_t states, uint32_t rate_cats, uint64_t sites, uint64_t branches,
                        int flags, int from_tree, int banks, int* mode, uint32_t* block_branches);
/* Process-wide bound of what epa_dev_create* may plan with, in place of the device's free memory (0 = none).  It
 * bounds the plan's decision under EPA_FLAG_LOOKUP_AUTO / _BLOCKS, not hipMalloc: for shared devices and tests. */
void epa_dev_set_mem_cap(uint64_t bytes);
/* What a context uses: *mode = EPA_LOOKUP_*, *block_branches = branches per block buffer (0 when resident). */
int epa_dev_lookup_mode(const epa_ctx* ctx, int* mode, uint32_t* block_branches);

/*
 * Query encoding (one byte per site, Q x W row-major): the lookup-column index of the
 * character, i.e. the position in NT_MAP / AA_MAP (src/util/maps.hpp:9-31; for DNA this is the
 * 4-bit code of the .bfast format, src/io/encoding.hpp) after the normalisation of
 * Lookup_Store's constructor (Lookup_Store.hpp:33-68).  epa_encode_queries() produces it from
 * ASCII.  win_begin/win_span = get_valid_range() per query (src/util/Range.hpp:34-49), or
 * (0, W) when premasking is off.
 */

/* ASCII -> column codes + windows on the host.  seqs: Q pointers to W characters each.
 * aa_x_as_n is accepted for ABI stability and ignored: quirk D4 lives in the lookup table of a
 * context created with epa_ref_desc.aa_x_as_n (preplacement only, as in the reference), the
 * code of 'X' is the same either way and the thorough placement always reads it as "any".
 * Returns EPA_OK, EPA_ERR_INVALID_CHAR or EPA_ERR_QUERY_ALL_GAP (first offender in *bad_query). */
int epa_encode_queries(uint32_t states, uint32_t sites, uint32_t Q, const char* const* seqs,
                       int premasking, int aa_x_as_n, uint8_t* codes, uint32_t* win_begin,
                       uint32_t* win_span, uint32_t* bad_query);

/*
 * Compact query layout (the wire format for real runs: a 150-column read of a 1500-column
 * alignment is 150 bytes instead of 1500).  Row q holds ONLY the window of query q:
 * codes[q*stride + i] = code of alignment column win_begin[q] + i, i < win_span[q] <= stride;
 * the rest of the row is padding.  Two passes: call with stride == 0 (codes may be NULL) to get
 * the windows, pick stride >= max(win_span) (a multiple of 16 keeps rows aligned), call again.
 * epa_dev_set_query_layout() tells a context which layout the q_codes of the following
 * preplace / thorough / place_chunk calls use: 0 (default) = Q x W rows as produced by
 * epa_encode_queries(), S > 0 = compact rows of S bytes.  Results are identical.
 */
/* Upper limit on the host threads the encoders use (0 = the hardware concurrency, at most 32). */
void epa_encode_set_threads(unsigned n);
int epa_encode_queries_compact(uint32_t states, uint32_t sites, uint32_t Q, const char* const* seqs,
                               int premasking, int aa_x_as_n, uint32_t stride, uint8_t* codes,
                               uint32_t* win_begin, uint32_t* win_span, uint32_t* bad_query);
int epa_dev_set_query_layout(epa_ctx* ctx, uint32_t code_stride);

/*
 * 4-bit wire format for nucleotide queries (the packing of the reference's FourBit,
 * src/io/encoding.hpp:18-27,81-97): two codes per byte, the earlier site in the high nibble, an
 * odd row padded with code 0 ('-').  The DNA column codes of epa_encode_queries*() are the 4-bit
 * state sets of NT_MAP (src/util/maps.hpp:9-26), so a row of `stride` codes packs into
 * (stride + 1) / 2 bytes.  epa_dev_set_query_packing(ctx, 4) tells a context that the q_codes of
 * the following calls are packed rows (row pitch (stride + 1) / 2, stride = the query layout's
 * row length); they are expanded on the device.  8 (default) = one byte per code.
 */
int epa_pack_codes_4bit(const uint8_t* codes, uint32_t Q, uint32_t stride, uint8_t* packed);
int epa_unpack_codes_4bit(const uint8_t* packed, uint32_t Q, uint32_t stride, uint8_t* codes);
int epa_dev_set_query_packing(epa_ctx* ctx, int bits);

/*
 * Replaces place() (src/core/place.cpp:41-95): lnl[q*B + b] = sum over the query's window of
 * T[b][site][code(q,site)]  (Lookup_Store::sum_precomputed_sitelk, Lookup_Store.hpp:110-141,
 * same summation order).  pendant = pendant_default and distal = branch_length/2 are implied.
 */
int epa_dev_preplace(epa_ctx* ctx, const uint8_t* q_codes, const uint32_t* win_begin,
                     const uint32_t* win_span, uint32_t Q, double* lnl);

/* epa_dev_preplace with what the fused chunk body adds to it.  max_span: an upper bound of win_span[] (0 = unknown, as
 * epa_dev_preplace; a longer window is EPA_ERR_INVALID_ARG when win_span is a host array) -- with a bound of at most
 * 160 sites (4 states) / 128 (20 states) the single-chunk kernels run, as in epa_dev_place_chunk.  seg_keys: NULL, or
 * (up to 4096 branches) [Q][pitch] with pitch = ceil(B / 64) rounded up to 8: the per-(query, 64-branch segment) maxima
 * of the table those kernels leave for the candidate selection, as order-preserving keys (a double's bits, negative:
 * inverted, else the sign bit set), 0 = not written (query served by another kernel, or max_span not bounded). */
int epa_dev_preplace_bounded(epa_ctx* ctx, const uint8_t* q_codes, const uint32_t* win_begin,
                             const uint32_t* win_span, uint32_t Q, uint32_t max_span, double* lnl, uint64_t* seg_keys);

/* Internal (tests and measurements): the fp32 two-branch screen of the pair preplacement and its band test, run alone on
 * the queries of one chunk.  seg32 [Q][nseg] (or null): the fp32 maxima of the 64-branch segments, NaN where
 * the screen left none (a query of the generic kernel); seg_mask [Q] (or null): the segments the exact pass has to fill
 * for the dynamic rule at `threshold`; info [8]: 0 the screen ran (its conditions: 4 states, resident tables, max_span
 * of at most one chunk, at most 4096 branches, a finite table, delta <= 1, option "preplace_screen"), 1 delta, 2 the
 * number of included (query, segment) cells, 3 the table's largest |entry|, 4 its non-finite entries, 5 band_t,
 * 6 / 7 the screening and the band kernel's time in ms. */
int epa_dev_preplace_screen_probe(epa_ctx* ctx, const uint8_t* q_codes, const uint32_t* win_begin,
                                  const uint32_t* win_span, uint32_t Q, uint32_t max_span, double threshold,
                                  float* seg32, uint64_t* seg_mask, double* info);
/* Internal (tests and measurements): the same for the 16-bit screen (four branches per table entry in fixed point relative
 * to the per-slot maximum over the branches), whatever "preplace_screen_i16" says.  seg16 [Q][nseg] (or null):
 * the relative integer maxima of the segments in units of h, -32768 = at most the floor, INT32_MIN = no key; cq [Q] (or
 * null): C_q, so that C_q + h seg16 + delta bounds a segment's exact maximum from above, and from below by 2 delta less
 * where seg16 is above the floor; seg_mask as above; info [8]: 0 the screen ran (the fp32 screen's conditions and its own
 * delta <= 1), 1 delta, 2 the included cells, 3 h, 4 the reads that could not be screened (row maximum at the floor: all
 * their segments are included), 5 band_t, 6 / 7 the kernels' times in ms. */
int epa_dev_preplace_screen16_probe(epa_ctx* ctx, const uint8_t* q_codes, const uint32_t* win_begin,
                                    const uint32_t* win_span, uint32_t Q, uint32_t max_span, double threshold,
                                    int32_t* seg16, double* cq, uint64_t* seg_mask, double* info);
/* Internal (tests): the number of chunk bodies of this context whose preplacement took the screen's two-pass route. */
uint64_t epa_dev_preplace_screen_runs(const epa_ctx* ctx);

/*
 * Replaces place_thorough() (src/core/place.cpp:97-171) = Tiny_Tree::place with opt_branches
 * (Tiny_Tree.cpp:159-204) -> call_focused(optimize_branch_triplet) -> opt_branch_lengths_pplacer
 * (src/core/pll/optimize.cpp:60-286).  One result per pair, in pair order.  `stats` may be NULL.
 */
int epa_dev_thorough(epa_ctx* ctx, const epa_pair* pairs, uint64_t n_pairs,
                     const uint8_t* q_codes, const uint32_t* win_begin, const uint32_t* win_span,
                     uint32_t Q, epa_result* out, epa_thorough_stats* stats);

/*
 * Log-likelihood of given placements at GIVEN branch lengths; no optimiser runs.  This is what Tiny_Tree::place
 * returns with opt_branches == false once the triplet's lengths are set (src/tree/Tiny_Tree.cpp:186-204:
 * pll_update_prob_matrices on the three edges, pll_update_partials of the inner node toward the query,
 * pll_compute_edge_loglikelihood on the pendant edge, summed over the sites of the query's window, scaler counts and
 * the +I term included), i.e. the `likelihood` of a jplace row at that row's own lengths.
 * entry i: pairs[i], pendant[i], distal[i], proximal[i].  proximal == NULL: branch_length[b] - distal[i]
 * (the sliding rule's convention and what a jplace row means).  One double per entry, in entry order.
 * Queries are staged as for epa_dev_thorough (query layout / packing of the context); entry arrays and lnl may be host
 * or device pointers; n == 0 returns EPA_OK.  Host arrays are validated, EPA_ERR_INVALID_ARG names the first offending
 * entry: branch_id >= B, seq_id >= Q, a non-finite or negative length, and with proximal == NULL a distal length beyond
 * the branch's.  A length of exactly 0 is valid (P = I).  An entry on a query with win_span == 0 gets 0.0 (the empty sum).
 * Reads only the transformed CLVs and scaler counts: the same bits in the resident and the blocked lookup layout.
 * Accuracy: P(t) is formed through the eigenbasis, where exp(lambda r t) cancels for tiny t: the absolute error of lnL
 * grows roughly like 1 / pendant below 1e-4.  The CLVs live in the eigenbasis too; an entry of a CLV brought back to
 * state space that does not exceed the rounding-error bound of its own sum (32 unit roundoffs of the sum of its terms'
 * magnitudes) is taken as 0, which is what libpll holds there: a state that a tip excludes, at a distal or proximal
 * length of exactly 0 (P(0) is the identity matrix).  Without that cut the residue of ~1e-16 was divided by a tiny
 * pendant length wherever the query shows such a state (up to 2.2e-6 at pendant 1e-4; tests/test_gpu_score_at.py).
 * Timer: "score_at" of epa_dev_last_kernel_ms.
 */
int epa_dev_score_at(epa_ctx* ctx, const epa_pair* pairs, const double* pendant, const double* distal,
                     const double* proximal /* may be NULL */, uint64_t n,
                     const uint8_t* q_codes, const uint32_t* win_begin, const uint32_t* win_span, uint32_t Q,
                     double* lnl);

/*
 * Per-site log-likelihoods of the same entries: what epa_dev_score_at sums.  Arguments, validation, the host-or-device
 * pointer rule and query staging are epa_dev_score_at's.  site_lnl is [n][pitch] doubles: row i, column j <
 * win_span[seq_id] holds the log of the site likelihood at window position j of entry i's query (the scaler counts
 * included as -256 count ln 2, the +I term included); the columns from the span up to pitch are exactly 0.0, an entry
 * on a query with win_span == 0 gets an all-zero row.  pitch smaller than the longest window among the entries' queries
 * (pairs on the device: among all Q queries) is EPA_ERR_INVALID_ARG; n == 0 returns EPA_OK.
 * The kernel is k_score_at with one store per lane in place of the product over the sites: the same noise cut, tables
 * and operand order, so a row's sum is score_at's lnL up to the rounding of the sum, and the same bits come out of the
 * resident and the blocked lookup layout.  Timer: "site_lnl".
 */
int epa_dev_site_lnl(epa_ctx* ctx, const epa_pair* pairs, const double* pendant, const double* distal,
                     const double* proximal /* may be NULL */, uint64_t n,
                     const uint8_t* q_codes, const uint32_t* win_begin, const uint32_t* win_span, uint32_t Q,
                     uint32_t pitch, double* site_lnl /* [n][pitch] */);

/*
 * Profile queries: a query given as per-site state LIKELIHOODS instead of one hard-called character per site -- reads
 * with per-base qualities (the tip-error model, Felsenstein 2004; RAxML-NG --prob-msa), consensus or profile columns.
 * A profile query q is a window (win_begin[q], win_span[q]) plus one row of S = states non-negative doubles per window
 * position, in the compact-row idiom of epa_encode_queries_compact:
 *   prof[((size_t)q * stride + j) * S + m],  j < win_span[q] <= stride,  is the likelihood of the observation at
 *   alignment column win_begin[q] + j given true state m (libpll's state order: A C G T / A R N D C Q E G H I L K M F P
 *   S T W Y V).  Rows from the span up to `stride` are padding and are never read.  prof may be a host or a device
 *   pointer, by the library's usual rule.
 * The site likelihood of the row v on branch b at given lengths is
 *   (1 - p_inv) sum_k w_k sum_i pi_i [P_k(pendant) v]_i [P_k(distal) D_k]_i [P_k(proximal) X_k]_i  +  p_inv pi_inv(site)
 * The +I term is added ONCE whatever v is: libpll's rule for coded queries (epa_ref_desc.invariant_state).  Scaler counts
 * are handled as in epa_dev_score_at.  It follows that a 0/1 row equal to the state set of a column code reproduces the
 * coded query: epa_dev_score_at_profile, _site_lnl_profile and _thorough_profile then return the bits of their coded
 * twins (the latter under the option "thorough_generic"); epa_dev_preplace_profile agrees with epa_dev_preplace up to
 * rounding (another order of operations).
 * Conditions, stated and not measured: every entry of a window row is finite and >= 0, and the row's largest entry lies
 * in [2^-64, 2^64], which keeps the kernels' scaling decisions the reference side's own.  Host rows are validated on the
 * host, device rows on the device (a status word read back before the call goes on); EPA_ERR_INVALID_ARG names the first
 * offending query and position: "... query Q position J: ...".  Windows are checked as for the coded calls; a window
 * longer than `stride` is EPA_ERR_INVALID_ARG.
 * The query layout and packing of the context (epa_dev_set_query_layout / _packing) do not concern profile calls and
 * are left as they are.
 *
 *   epa_dev_preplace_profile     lnl[q*B + b] = sum over the window of log(site likelihood) at pendant_default and
 *                                distal = proximal = branch_length[b] / 2: epa_dev_preplace for rows.  Computed from the
 *                                resident lookup table's pure-state columns, sum_m v_m exp(T[b][site][column of m]), with
 *                                the +I term, which every column holds once, counted once; the query-independent
 *                                exp(T_m - T_any) are a table derived once per context ((S + 2) x 8 bytes per branch x
 *                                site).  Timer: "preplace_profile"
 *   epa_dev_thorough_profile     epa_dev_thorough for rows: always the general Newton kernel (k_thorough_generic), both
 *                                BLO rules.  Timer: "thorough"
 *   epa_dev_score_at_profile, epa_dev_site_lnl_profile
 *                                the arguments, checks and outputs of epa_dev_score_at / epa_dev_site_lnl with
 *                                (prof, stride) in place of q_codes.  Timers: "score_at" / "site_lnl"
 *   epa_dev_place_chunk_profile  preplace_profile -> the context's candidate selection (epa_dev_set_heuristic, as
 *                                epa_dev_select_candidates applies it to that table) -> thorough_profile; the table never
 *                                leaves HBM.  Pairs and results are those of the three calls made one after the other, bit
 *                                for bit.  EPA_ERR_PAIR_OVERFLOW as in epa_dev_place_chunk: call again with larger buffers
 *                                (synchronous: nothing stays staged)
 * A context in the blocked lookup layout (EPA_FLAG_LOOKUP_BLOCKS) has no resident table: the two entry points that
 * preplace return EPA_ERR_UNSUPPORTED, the message names --memsave.  score_at / site_lnl / thorough on profiles read only
 * the transformed CLVs and work in both layouts.
 * Not available for profiles: pipeline slots and group launches, the RELL and marginal-likelihood statistics, the tuned
 * Newton kernels.
 */
int epa_dev_preplace_profile(epa_ctx* ctx, const double* prof, uint32_t stride, const uint32_t* win_begin,
                             const uint32_t* win_span, uint32_t Q, double* lnl);
int epa_dev_thorough_profile(epa_ctx* ctx, const epa_pair* pairs, uint64_t n_pairs, const double* prof, uint32_t stride,
                             const uint32_t* win_begin, const uint32_t* win_span, uint32_t Q, epa_result* out,
                             epa_thorough_stats* stats);
int epa_dev_score_at_profile(epa_ctx* ctx, const epa_pair* pairs, const double* pendant, const double* distal,
                             const double* proximal /* may be NULL */, uint64_t n, const double* prof, uint32_t stride,
                             const uint32_t* win_begin, const uint32_t* win_span, uint32_t Q, double* lnl);
int epa_dev_site_lnl_profile(epa_ctx* ctx, const epa_pair* pairs, const double* pendant, const double* distal,
                             const double* proximal /* may be NULL */, uint64_t n, const double* prof, uint32_t stride,
                             const uint32_t* win_begin, const uint32_t* win_span, uint32_t Q, uint32_t pitch,
                             double* site_lnl /* [n][pitch] */);
int epa_dev_place_chunk_profile(epa_ctx* ctx, const double* prof, uint32_t stride, const uint32_t* win_begin,
                                const uint32_t* win_span, uint32_t Q, double threshold, epa_pair* pairs,
                                epa_result* results, uint64_t max_pairs, uint64_t* n_pairs, epa_thorough_stats* stats);
/*
 * Host only, no device needed: profile rows from column codes and Phred scores, the standard tip-error model.  codes and
 * phred are compact rows ([Q][stride], the window only: epa_encode_queries_compact); phred holds the scores themselves
 * (0 .. 93, not their ASCII form).  At window position j of query q:
 *   a pure-state code with score s   eps = min(pow(10, -s / 10), (S - 1) / S);  v[called] = 1 - eps, v[other] = eps / (S - 1)
 *   any other code (ambiguity, gap)  its 0/1 state set, the score is ignored
 * Rows from the span up to the stride are left untouched.  EPA_ERR_INVALID_ARG: a score above 93 at a pure-state code, a
 * window longer than the stride; EPA_ERR_INVALID_CHAR: a code that is no lookup column (epa_dev_last_error(NULL) names
 * query and position).
 */
int epa_profile_from_phred(uint32_t states, uint32_t Q, uint32_t stride, const uint8_t* codes, const uint8_t* phred,
                           const uint32_t* win_span, double* prof);

/*
 * Marginal likelihood of "read q sits somewhere on edge b", integrated over where it attaches and how long its pendant
 * branch is.  The definition is this project's own (pplacer's -p mode, which writes the jplace fields marginal_like and
 * post_prob, is the motivation, not a parity target).  For an entry (branch b of length L_b, query q):
 *
 *   M(b,q) = log  int_0^1 dx  int_0^inf dp  (1/mu) e^{-p/mu} * Lik(b, q; pendant = p, distal = x L_b, proximal = L_b - x L_b)
 *
 * Lik is exactly what epa_dev_score_at returns the log of: taken over the query's window, scaler counts and the +I term
 * included.  The attachment point is uniform on the edge; the pendant length has an exponential prior of mean mu.  The
 * posterior probability of a row is exp(M_i) / sum_rows exp(M_i) over the rows of its placement object: an equal prior
 * over the object's edges, the normalisation compute_and_set_lwr applies to `likelihood` (the caller's business).
 * The device does not know about priors or quadrature rules.  The caller hands it a tensor rule and it evaluates exactly:
 *
 *   d_i   = x_frac[i] * blen[b]             proximal_i = blen[b] - d_i      (score_at's own expression for proximal == NULL)
 *   g_ij  = lnL(b, q; p_len[j], d_i, proximal_i)                            i < Kx, j < Kp
 *   v_ij  = (x_logw[i] + p_logw[j]) + g_ij
 *   m     = max v_ij ;   M = m + log( sum_{i ascending, then j ascending} exp(v_ij - m) )      plain fp64 adds in that order
 *
 * With epa_quadrature_legendre01 for x and epa_quadrature_laguerre for p (p_len[j] = mu t_j, p_logw[j] = log w_j: the
 * prior is the rule's weight function) this is the integral above; 8 x 16 nodes agree with 16 x 32 to 1e-8 in M on the
 * suite's references.
 * x_frac, x_logw, p_len, p_logw are HOST arrays.  pairs, marginal ([n]) and grid_lnl ([n][Kx][Kp] = g_ij, or NULL) may be
 * host or device pointers; queries are staged as for epa_dev_score_at (query layout / packing of the context).
 * EPA_ERR_INVALID_ARG, naming the offender: Kx or Kp outside 1 .. 64; an x_frac outside [0, 1] or not finite; a p_len
 * negative or not finite; a log weight that is not finite; branch_id >= B or seq_id >= Q (host pairs: the first offending
 * entry).  n == 0 returns EPA_OK.  An entry on a query with win_span == 0 has g_ij = 0.0 everywhere: its M is the log of
 * the rule's total weight.
 * k_marginal (marginal.hip) keeps k_score_at's operand order inside a site -- noise cut and tables included -- so g_ij is
 * score_at at the same point up to the order of the sum over the sites' lanes, and the same bits come out of the
 * resident and the blocked lookup layout.  Accuracy caveat inherited from epa_dev_score_at: through the eigenbasis the
 * error of lnL grows like 1 / pendant below 1e-4, so pendant nodes below 1e-4 are accepted but not covered by the 1e-6
 * bound.  Timer: "marginal".
 */
int epa_dev_marginal_like(epa_ctx* ctx, const epa_pair* pairs, uint64_t n,
                          const double* x_frac, const double* x_logw, uint32_t Kx,      /* host arrays */
                          const double* p_len,  const double* p_logw, uint32_t Kp,      /* host arrays */
                          const uint8_t* q_codes, const uint32_t* win_begin, const uint32_t* win_span, uint32_t Q,
                          double* marginal /* [n] */, double* grid_lnl /* [n][Kx][Kp] or NULL */);

/*
 * Quadrature rules for epa_dev_marginal_like; host only, no device needed.  K: 1 .. 64, else EPA_ERR_INVALID_ARG.  Nodes
 * ascending; the weights are returned as logarithms and sum to 1.
 *   legendre01: Gauss-Legendre on [0, 1]: sum_j w_j f(nodes_j) ~ int_0^1 f(x) dx, nodes in (0, 1)
 *   laguerre:   Gauss-Laguerre: sum_j w_j f(t_j) ~ int_0^inf e^-t f(t) dt, t_j > 0; the weights are formed in log space
 *               (w_j reaches e^-109 at K = 32)
 */
int epa_quadrature_legendre01(uint32_t K, double* nodes, double* log_weights);
int epa_quadrature_laguerre(uint32_t K, double* nodes, double* log_weights);

/*
 * RELL bootstrap support (resampling of estimated log-likelihoods).  The entries (as for epa_dev_score_at) of one query
 * compete, in any order -- branch-major as the chunk body emits them is the normal case: the query's sites are resampled
 * with replacement `replicates` times, every replicate is won by the entry with the largest resampled lnL, and
 * support[i] = (replicates entry i wins) / replicates, so the supports of a query add up to 1.
 * The resampling is specified exactly; a restatement anywhere reaches the same counts from the same site values:
 *   generator  Philox4x32-10 with the Random123 constants: multipliers 0xD2511F53 and 0xCD9E8D57, Weyl increments
 *              0x9E3779B9 and 0xBB67AE85; key = (seed low word, seed high word).  Known answers (counter / key -> output):
 *                0 0 0 0 / 0 0                                                   -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8
 *                ffffffff x 4 / ffffffff x 2                                     -> 408f276d 41c83b0e a20bc7c6 6d5451fd
 *                243f6a88 85a308d3 13198a2e 03707344 / a4093822 299f31d0         -> d16cfe09 94fdcceb 5001e420 24126ea1
 *   draws      replicate r of a query with stream id t and span n_q makes n_q draws; draw d uses output word d % 4 of
 *              counter (d / 4, r, t low word, t high word); the drawn site is j = (word * n_q) >> 32 (a bias of at
 *              most n_q / 2^32, accepted)
 *   score      an entry's score starts at 0.0 and adds, for d = 0 .. n_q - 1 in this order, its site value
 *              (epa_dev_site_lnl) at the drawn j: plain fp64 adds, no centring, no reassociation
 *   winner     the largest score; ties go to the smaller branch_id, then to the smaller entry index
 *   span 0     every score is 0.0: the tie rule gives the whole support to one entry
 * stream_id: [Q] (host or device), or NULL = the query's index seq_id.  A caller that splits its queries over several
 * calls passes ids that do not depend on the split (epa-ng-amd --rescore: the placement object's index in the file).
 * replicates: 1 .. 2^20, else EPA_ERR_INVALID_ARG; other errors as epa_dev_score_at (pairs on the device: a seq_id >= Q
 * is found and refused).  n < 2^32 per call; no bound on the entries per query or on the span.  The site rows live in
 * device scratch in batches of whole queries of at most 128 MiB (one query whose rows are larger is a batch alone).
 * Timer: "rell" (grouping, site rows and resampling together).
 */
int epa_dev_rell_support(epa_ctx* ctx, const epa_pair* pairs, const double* pendant, const double* distal,
                         const double* proximal /* may be NULL */, uint64_t n,
                         const uint8_t* q_codes, const uint32_t* win_begin, const uint32_t* win_span, uint32_t Q,
                         const uint64_t* stream_id /* [Q] or NULL = seq_id */,
                         uint32_t replicates, uint64_t seed, double* support /* [n] */);

/*
 * Three statistics from one set of RELL replicates: the bootstrap support above, the expected likelihood weight (ELW,
 * Strimmer & Rambaut 2002: the likelihood weight ratio averaged over the replicates; its cumulative sum gives a
 * confidence set of placements) and the p-value of the Shimodaira-Hasegawa (SH) test of every entry against the best
 * entry of its query.  Generator, draws and score are those of epa_dev_rell_support (above) and nothing else; the same
 * (seed, stream_id, replicates) give the same replicates in both calls.  For a query with span n_q and entries k (in the
 * caller's order), replicate r:
 *   score     s_k^(r): epa_dev_rell_support's score -- 0.0 plus the drawn site values in draw order, plain fp64 adds
 *   observed  L_k: 0.0 plus the entry's site values (epa_dev_site_lnl) at j = 0 .. n_q - 1 in this order, plain fp64
 *             adds: the site row summed sequentially; epa_dev_score_at's lnL up to the rounding of the sum
 *   support   epa_dev_rell_support's winner and tie rule; support[k] has the bits that call returns for the same arguments
 *   elw       m = max_k s_k^(r);  w_k^(r) = exp(s_k^(r) - m) / sum_k' exp(s_k'^(r) - m);  elw[k] = (sum_r w_k^(r)) / replicates.
 *             The order of the floating-point sums is not specified; a restatement agrees to 1e-12 absolute (the scores
 *             are bit-exact, exp and the sums differ by a few ulp each).  The same call returns the same bits every
 *             time: the sums run in a fixed order, no floating-point atomics.  Duplicated entries share the weight: no
 *             tie rule.  The elw of a query add up to 1
 *   p_sh      c_k^(r) = s_k^(r) - L_k;  t_k^(r) = (max_k' c_k'^(r)) - c_k^(r);  T_k = (max_k' L_k') - L_k;
 *             p_sh[k] = #{ r : t_k^(r) >= T_k } / replicates.  Every step is ONE fp64 subtraction, nothing fused or
 *             reassociated: the counts are a function of the site values alone and a restatement reaches them as
 *             integers.  The entry with the largest L has T = 0 and t >= 0: its p_sh is 1.0 exactly
 *   centring  the resampled scores are centred at L_k, the exact mean of the resampling distribution of s_k.  The
 *             classic SH recipe centres at the Monte-Carlo mean of the replicates instead; the two agree as
 *             `replicates` grows.  The exact centre needs no second pass over the replicates and makes the count
 *             reproducible from the site values
 *   span 0    every score and every L is 0.0: elw = 1 / (entries of the query), p_sh = 1, support by the tie rule
 *   one entry support = elw = p_sh = 1
 * Arguments, checks, error texts, the host-or-device pointer rule and query staging are epa_dev_rell_support's
 * (errors name "rell_tests").  support, elw, p_sh: [n] each (host or device), any of them NULL to leave it out; all three
 * NULL is EPA_ERR_INVALID_ARG.  replicates: 1 .. 2^20; n < 2^32; n == 0 returns EPA_OK.
 * Timer: "rell_tests" (grouping, site rows, observed sums and resampling together).
 */
int epa_dev_rell_tests(epa_ctx* ctx, const epa_pair* pairs, const double* pendant, const double* distal,
                       const double* proximal /* may be NULL */, uint64_t n,
                       const uint8_t* q_codes, const uint32_t* win_begin, const uint32_t* win_span, uint32_t Q,
                       const uint64_t* stream_id /* [Q] or NULL = seq_id */,
                       uint32_t replicates, uint64_t seed,
                       double* support /* [n] or NULL */, double* elw /* [n] or NULL */, double* p_sh /* [n] or NULL */);

/*
 * The p-value of the approximately unbiased (AU) test (Shimodaira 2002) of every entry, from multiscale RELL replicates:
 * the resampling above repeated at several replicate lengths n' != n_q, and the change of an entry's bootstrap
 * proportion with n' / n_q used to correct the proportion for the curvature of the boundary of the region in which the
 * entry wins.  Where the SH p-value above grows more conservative with every competing entry, this one does not.
 * Generator, draws, scales, fit and fallback are specified exactly; a restatement anywhere reaches the same counts from
 * the same site values, and the same p-values up to the rounding of the fit:
 *   scales     scale_pm: [n_scales] HOST array, replicate lengths per mille of the span, each 100 .. 4000, n_scales 1 .. 16;
 *              NULL with n_scales == 0: the default ten, 500, 600, ..., 1400
 *   draw count scale s of a query with span n_q makes n'_s = max(1, (n_q * scale_pm[s] + 500) / 1000) draws per replicate
 *              (64-bit integers, truncating division); n'_s = 0 when n_q = 0.  n'_s may exceed n_q: the sites are still
 *              drawn from the n_q sites
 *   draws      generator and key of the bootstrap support above.  Replicate r of scale s uses output word d % 4 of
 *              counter (d / 4, ((s + 1) << 20) | r, t low word, t high word) for d = 0 .. n'_s - 1; the drawn site is
 *              j = (word * n_q) >> 32.  r < 2^20: the second counter word never meets another scale's, nor that of the
 *              plain RELL calls, where it is r alone.  The scales are independent streams; no replicate is a prefix of
 *              another scale's
 *   score      0.0 plus the entry's site values at the drawn j in draw order, plain fp64 adds, as above; no rescaling by
 *              n_q / n'_s, on which the winner does not depend
 *   winner     the largest score; ties go to the smaller branch_id, then to the smaller entry index
 *   counts     counts[s][i]: the replicates of scale s that entry i wins, an integer; the counts of a query add up to
 *              `replicates` at every scale
 *   fit        per entry.  Scale s is usable if 0 < counts[s][i] < R (R = replicates).  With at least 3 usable scales that
 *              have at least 2 distinct n'_s among them, for each usable scale
 *                p_s = counts[s][i] / R,  r_s = n'_s / n_q,  z_s = -Phi^-1(p_s),  a_s = sqrt(r_s),  b_s = 1 / a_s,
 *                w_s = phi(z_s)^2 / (p_s (1 - p_s))
 *              and (d, c) minimise sum_s w_s (z_s - d a_s - c b_s)^2: the 2 x 2 normal equations, the five sums Saa, Sab,
 *              Sbb, Saz, Sbz accumulated in scale order, det = Saa Sbb - Sab^2.  p_au = Phi(c - d); fit = (d, c), the
 *              signed distance and the curvature
 *   fallback   otherwise -- an entry that wins always or never, span 0, span 1 (every n'_s is 1), a single entry --
 *              p_au = counts[s*][i] / R for the scale s* with the smallest |scale_pm[s] - 1000|, ties to the smaller s,
 *              and fit = (NaN, NaN).  A single entry gets p_au = 1
 *   rounding   the order of the floating-point operations inside Phi^-1, Phi and the solve is not specified beyond the
 *              above; a float64 restatement with other library functions agrees to 3.2e-12 in p_au, d and c (100 x its own error
 *              against the same fit at 50 digits; measured 5e-14).  The same call returns
 *              the same bits every time: integer atomics for the counts, one thread per entry for the fit, no
 *              floating-point atomics
 * Arguments, checks, error texts, the host-or-device pointer rule and query staging are those of the bootstrap support
 * above (errors name "rell_au").  p_au: [n], counts: [n_scales][n] (ten rows with the default scales), fit: [n][2], host or
 * device, any of them NULL to leave it out; all three NULL is EPA_ERR_INVALID_ARG.  replicates: 1 .. 2^20 per scale;
 * n < 2^32; n == 0 returns EPA_OK.  Timer: "rell_au" (grouping, site rows, resampling at every scale and fit together).
 */
int epa_dev_rell_au(epa_ctx* ctx, const epa_pair* pairs, const double* pendant, const double* distal,
                    const double* proximal /* may be NULL */, uint64_t n,
                    const uint8_t* q_codes, const uint32_t* win_begin, const uint32_t* win_span, uint32_t Q,
                    const uint64_t* stream_id /* [Q] or NULL = seq_id */,
                    uint32_t replicates, uint64_t seed,
                    const uint32_t* scale_pm /* [n_scales] per mille, or NULL = the default ten */, uint32_t n_scales,
                    double* p_au /* [n] or NULL */, uint32_t* counts /* [n_scales][n] or NULL */,
                    double* fit /* [n][2] = (d, c) or NULL */);

/*
 * The p-values of the Kishino-Hasegawa (KH) test, the weighted KH test and the weighted SH test (Shimodaira & Hasegawa
 * 1999, Shimodaira 1998; CONSEL's and IQ-TREE's p-KH, p-WKH, p-WSH) of every entry, from the RELL replicates above.  The
 * SH p-value of epa_dev_rell_tests grows more conservative with every competing entry; the weighted tests divide every
 * difference of two entries by its standard deviation under the resampling, so that an entry far off does not set the
 * scale for the others.  Generator, draws and score are those of epa_dev_rell_support and nothing else; the same (seed,
 * stream_id, replicates) give the same replicates.  Every step below is ONE fp64 operation, nothing fused or
 * reassociated: the three counts are a function of the site values alone and a restatement reaches them as integers.
 * For a query with span n_q, entries k (in the caller's order) with site values x_k[j] (epa_dev_site_lnl), replicate r:
 *   score      s_k^(r): epa_dev_rell_support's score
 *   observed   L_k: 0.0 plus x_k[j] for j = 0 .. n_q - 1 in this order, as in epa_dev_rell_tests
 *   centred    c_k^(r) = s_k^(r) - L_k
 *   best       b: the entry with the largest L; ties go to the smaller branch_id, then to the smaller entry index
 *   pair scale for k != k':  d_j = x_k'[j] - x_k[j];  a = 0.0 plus the d_j, j = 0 .. n_q - 1 in this order (sequential, no
 *              blocking);  m = a / n_q;  q = 0.0 plus (d_j - m) * (d_j - m) in the same order, the product rounded before
 *              it is added;  v = sqrt(q), the exact standard deviation of the resampled s_k' - s_k;  w_kk' = 1.0 / v.
 *              The pair is SKIPPED when q == 0 or w is not finite: equal rows, span 0 (m is NaN, q stays 0), span 1.
 *              w_kk' and w_k'k have the same bits
 *   p_kh       #{ r : c_b^(r) - c_k^(r) >= L_b - L_k } / replicates.  The best entry gets exactly 1.0
 *   p_wkh      the opponent k* maximises (L_k' - L_k) * w_kk' over the k' whose pair with k is not skipped; ties go to the
 *              smaller branch_id, then to the smaller entry index.  p_wkh[k] = #{ r : c_k*^(r) - c_k^(r) >= L_k* - L_k } /
 *              replicates; with no opponent (every pair skipped, or the best entry: below) it is 1.0
 *   p_wsh      T_k = max (L_k' - L_k) * w_kk' and t_k^(r) = max (c_k'^(r) - c_k^(r)) * w_kk', both over the k' not skipped;
 *              p_wsh[k] = #{ r : t_k^(r) >= T_k } / replicates; with no opponent it is 1.0.  p_wkh <= p_wsh, as counts
 *   best entry all three are exactly 1.0 for b, and for a copy of b: an entry k with L_b - L_k == 0 whose pair with b is
 *              skipped.  p_kh by its rule; for p_wkh and p_wsh such an entry has NO opponent whatever its other pairs are:
 *              the tests ask whether an entry is worse than the best, and the best is never rejected.  (CONSEL and
 *              IQ-TREE test the best entry against the one nearest below it instead and print values below 1 there.)
 *   one entry, span 0   all three are 1.0
 *   span 1     every pair is skipped: p_wkh = p_wsh = 1; p_kh by its rule: c = 0 for every entry, so it is 0 for an entry
 *              strictly worse than the best and 1 for the others
 *   bound      at most 1024 entries per query in this call; a larger group is EPA_ERR_INVALID_ARG, the text names the query
 *              and its count.  A condition, not a measurement: it holds one query's [K][K] scales to 8 MiB and the
 *              quadratic work of a replicate to a bounded launch
 * Arguments, checks, error texts, the host-or-device pointer rule and query staging are epa_dev_rell_support's (errors
 * name "rell_kh").  p_kh, p_wkh, p_wsh: [n] each (host or device), any of them NULL to leave it out; all three NULL is
 * EPA_ERR_INVALID_ARG.  replicates: 1 .. 2^20; n < 2^32; n == 0 returns EPA_OK.  The same call returns the same bits
 * every time: integer atomics for the counts, no floating-point atomics.
 * Timer: "rell_kh" (grouping, site rows, observed sums, pair scales and resampling together).
 */
int epa_dev_rell_kh(epa_ctx* ctx, const epa_pair* pairs, const double* pendant, const double* distal,
                    const double* proximal /* may be NULL */, uint64_t n,
                    const uint8_t* q_codes, const uint32_t* win_begin, const uint32_t* win_span, uint32_t Q,
                    const uint64_t* stream_id /* [Q] or NULL = seq_id */,
                    uint32_t replicates, uint64_t seed,
                    double* p_kh /* [n] or NULL */, double* p_wkh /* [n] or NULL */, double* p_wsh /* [n] or NULL */);

/*
 * Tree geometry: which branch touches which.  A context knows its branches' lengths but not how they join; this call
 * attaches the topology that path distances need (epa_dev_edpl and epa_dev_krd below).  node_prox[b] / node_dist[b] (HOST or device
 * arrays, [B]) are the node ids, 0 .. n_nodes - 1, at the proximal and the distal end of branch b, in the orientation of
 * epa_dev_score_at: distal[i] of an entry is measured from the node_dist[b] end, the remainder is branch_length[b] -
 * distal[i].  The lengths are the context's own.
 * Specified, so that a restatement anywhere reaches the same bits:
 *   root       node_prox[0]; depth[root] = 0.0
 *   depth      depth[child] = depth[parent] + branch_length[edge]: ONE fp64 add per level
 *   child(b)   the end of b that is farther from the root
 *   rank(b)    b's position, 0 .. B - 1, when the branches are listed in the order a depth-first walk from the root first
 *              reaches their child ends, a node's branches taken by ascending branch id: a pre-order
 *   size(b)    the number of branches in the subtree of child(b), b included: that subtree is the ranks [rank, rank + size)
 * EPA_ERR_INVALID_ARG, the text names the first offending branch: n_nodes != B + 1 (the text names both counts); a node id
 * >= n_nodes; a branch with both ends on one node or a length that is negative or not finite; a graph that is not connected (with n_nodes - 1 branches that also
 * rules out a cycle).  A refused call leaves the context, and a topology set before, as they were.  A second call
 * replaces the first.  No other entry point reads the topology: their results are the same bits with and without one.
 * Structure (treepath.hip): an Euler tour of the rooted tree and a sparse table of range minima over the tour's fp64
 * DEPTHS.  Lengths are >= 0 and a rounded add never decreases, so the minimum over the tour between two nodes is the
 * depth of their lowest common ancestor itself, zero-length branches included: a query is two 8-byte loads, O(1).
 * Built once per call on the host without recursion (a ladder tree is an ordinary input), kept in device memory:
 * 8 (2 n_nodes - 1) (floor(log2(2 n_nodes - 1)) + 1) + 20 B bytes (the table; per branch the child's depth, its Euler
 * index, the pre-order rank and the subtree size that epa_dev_krd reads), 20.2 MB at 65 537 branches.  The table is optional and
 * therefore NOT part of epa_dev_footprint's numbers.  (An all-pairs node distance matrix would be 34 GB there.)
 */
int epa_dev_set_topology(epa_ctx* ctx, uint32_t n_nodes, const uint32_t* node_prox /* [B] */,
                         const uint32_t* node_dist /* [B] */);

/*
 * Expected distance between placement locations (EDPL, Matsen et al.; `guppy edpl`, `gappa examine edpl`): where a query's
 * weight is spread over several rows, are they neighbours or on opposite sides of the tree?  Entry i is the point at
 * distal[i] on branch pairs[i].branch_id with weight[i] (the caller passes like_weight_ratios; they are used as given);
 * the entries of one query (seq_id) belong together as for epa_dev_rell_support: any order is accepted, they are
 * grouped through the same stable grouping, and "entry order" below is the order of appearance within the query.
 * Every line is ONE fp64 operation, nothing fused or reassociated; a restatement reaches the same bits.  Per query, with
 * e_i the branch of entry i and depth / child of epa_dev_set_topology:
 *   x_i        distal_i if child(e_i) == node_dist[e_i], else branch_length[e_i] - distal_i
 *   D_i        depth[child(e_i)] - x_i
 *   m_ij       min(depth[lca(child(e_i), child(e_j))], D_i, D_j)
 *   d_ij       (D_i - m_ij) + (D_j - m_ij)
 *   row_dist_i 0.0 plus weight_j * d_ij for j in entry order, the product rounded and then added
 *   edpl_q     0.0 plus weight_i * row_dist_i for i in entry order, likewise
 * The one rule for m_ij covers two points on one edge (|D_i - D_j|), an edge on the other's path to the root (D_j - D_i)
 * and unrelated edges.  edpl_q is the full double sum over i and j of w_i w_j d_ij, Matsen's definition; pendant lengths
 * do not enter, as in guppy and gappa.  A query with no entry gets 0.0, and so does a query with one.
 * pairs, distal, weight, row_dist ([n], or NULL to leave it out) and edpl ([Q]) may be host or device pointers.  Host
 * arrays are validated, EPA_ERR_INVALID_ARG names the first offending entry: branch_id >= B, seq_id >= Q, a distal length
 * that is negative, not finite or beyond the branch's length, a weight that is negative or not finite (device pairs: an
 * id out of range is found by the kernels, nothing is read through it, and the call is refused).  No topology set:
 * EPA_ERR_INVALID_ARG, the text says so.  n == 0 returns EPA_OK and writes Q zeros.  n < 2^32; no bound on the entries per
 * query.  No query codes: the call reads no CLV.
 * The same call returns the same bits every time: sequential sums, no floating-point atomics.  Timer: "edpl" (grouping,
 * points, pair sums and the per-query sum together).
 */
int epa_dev_edpl(epa_ctx* ctx, const epa_pair* pairs, const double* distal, const double* weight, uint64_t n, uint32_t Q,
                 double* row_dist /* [n] or NULL */, double* edpl /* [Q] */);

/*
 * Kantorovich-Rubinstein (earth mover's) distances between S placement samples on the reference tree, exponent 1 (Evans
 * and Matsen; `guppy kr`, `gappa analyze krd`), and the edge and clade masses squash clustering and edge PCA start from.
 * Entry i is a point mass weight[i] at distal[i] on branch pairs[i].branch_id, in epa_dev_edpl's orientation; it belongs
 * to sample pairs[i].seq_id < S.  Entries come in any order.  Weights are used as given: normalising a sample is the
 * caller's business.  Root, depth and child(b) are those of epa_dev_set_topology:
 *   x_i            the point's distance from the child end of its branch: EDPL's x_i, from the same expression
 *   child side     of a point y of the tree: everything that y separates from the root
 *   F_s(y)         the total weight of sample s's points strictly on the child side of y
 *   krd[a][b]      the integral of |F_a(y) - F_b(y)| over all branches by length
 * F is piecewise constant.  On a branch of length L whose points of a and b, merged by x ascending, are x_1 <= ... <= x_k,
 * the term is the sum over t of |f_t| (x_{t+1} - x_t) with x_0 = 0 and x_{k+1} = L; f_0 = T_a - T_b, T the mass of a sample
 * in the subtree hanging from child(b) without the branch's own points; f_t adds +w for a point of a and -w for one of b.
 * Points at equal x bound a segment of length zero.  With equal sample totals the value does not depend on the root; with
 * unequal totals it is this rooted definition.
 *   edge_mass[s][b]   the sum of sample s's weights on b
 *   clade_mass[s][b]  the mass in the subtree hanging from child(b), b's own points included
 * The order of the operations is the structure below and no more, so a restatement agrees within a bound, not bit for bit
 * (tests/krd_ref.py: 8 (B + n_a + n_b + 4) 2^-53 (W_a + W_b) times the tree's length).  Exact, and tested:
 *   (a) krd[a][a] == 0.0
 *   (b) krd[a][b] and krd[b][a] have the same bits: computed once, stored twice
 *   (c) krd[a][b] is a function of the tree and of the entries of a and b alone: the same two samples give the same bits
 *       in a call with S = 2 and among 65 samples, however the other samples' entries are interleaved and whichever of the
 *       two has the smaller id, as long as each sample's own entries keep their relative order.  Tile sizes and reduction
 *       shapes are compile-time constants; nothing depends on S, on the grid or on the other samples
 *   (d) two samples with the same entries in the same relative order are at 0.0 exactly, and their rows are bit-equal
 *   (e) the same call returns the same bits every time; there are no floating-point atomics
 * Structure (krd.hip).  Branches are addressed by pre-order rank: epa_dev_set_topology keeps rank(b), b's position in the
 * order its walk first reaches the child ends, and size(b), the branches in the subtree of child(b) with b; that subtree is
 * the ranks [rank, rank + size).  One work item per entry computes (sample, rank, x); two stable radix sorts order the
 * entries by x's bits (x >= 0) and then by (sample << 32 | rank), so equal x keep entry order.  Per sample, in rank order:
 * M_s[r], the run's weights added one after the other; P_s[r], the inclusive scan of M_s over the ranks (256 ranks at a
 * time, a fixed-shape scan plus the carry of the blocks before); T_s(b) = P_s[rank + size - 1] - P_s[rank]; clade_mass =
 * T + M.  The pair pass runs one 256-thread workgroup per (pair a < b, tile of 1024 ranks): lanes stride the ranks and merge
 * the two samples' points of their branches -- the points of both samples at one x are taken together, each sample's
 * weights there added in its own order and f moved by their difference -- and a fixed-shape wave and LDS reduction leaves
 * one partial per tile; a second kernel adds a pair's partials in tile order and stores [a][b] and [b][a].  A branch that
 * carries hundreds of points of one sample is one lane's long loop, as in epa_dev_edpl's pair sums.
 * pairs, distal, weight and the three outputs may be host or device pointers.  Host arrays are validated,
 * EPA_ERR_INVALID_ARG names the first offending entry: branch_id >= B, seq_id >= S ("sample id"), a distal length that is
 * negative, not finite or beyond the branch's length, a weight that is negative or not finite (device pairs: an id out of
 * range is found by the kernels, nothing is read through it, and the call is refused).  No topology set:
 * EPA_ERR_INVALID_ARG, the text says so.  S must be 1 .. 4096 (EPA_ERR_INVALID_ARG): the output stays within 128 MiB.
 * n < 2^32.  n == 0 writes zeros.  A sample without entries is legal: F = 0.
 * Scratch: about 12 S B bytes (P and the run starts), 8 S B more when a mass output is asked for, 68 n bytes of keys,
 * indices and sorted points plus rocPRIM's sort buffers, and at most 32 MiB of tile partials.  Timer: "krd" (points, sorts,
 * tables, pair pass and masses together), and inside it "krd_sort" (points, the two sorts, the gather), "krd_tables" (run
 * starts, M and P) and "krd_pairs" (the pair pass and the sum of its partials).
 */
int epa_dev_krd(epa_ctx* ctx, const epa_pair* pairs, const double* distal, const double* weight, uint64_t n, uint32_t S,
                double* krd /* [S][S] */, double* edge_mass /* [S][B] or NULL */, double* clade_mass /* [S][B] or NULL */);

/*
 * Squash clustering of the S samples (Matsen and Evans 2013; `guppy squash`, `gappa analyze squash`): hierarchical
 * clustering under the distance above in which a merged cluster is a new mass distribution on the tree, the average of
 * its member samples, whose distances to the other clusters are computed on the tree.  The inputs are epa_dev_krd's.
 *   cluster ids    the samples are clusters 0 .. S - 1; merge step t = 0 .. S - 2 creates cluster S + t
 *   a cluster      C with member samples m(C) is this entry sequence: the members in ascending sample id, each member's
 *                  entries in entry order, entry i with weight[i] / |m(C)| -- one fp64 division of the original weight,
 *                  never a product of earlier scalings.  (Squash's count-weighted average of the two merged clusters.)  A
 *                  cluster depends on its member set, not on the merge history
 *   D(C, C')       epa_dev_krd's value for two samples holding those two entry sequences, BIT FOR BIT (property (c) above
 *                  makes that well defined)
 *   step t         among all pairs of active clusters the smallest D, compared as doubles with <; on equal values the
 *                  smallest id a, then the smallest id b, a < b.  merge_a[t] = a, merge_b[t] = b, merge_dist[t] = D,
 *                  merge_size[t] = |m(a)| + |m(b)|; a and b retire, S + t is active with m(a) and m(b) united
 * The argmin takes a valid pair whatever the values are, so there are exactly S - 1 steps.  Distances need NOT grow with t
 * (an average can be nearer to a third cluster than either part was), and nothing assumes it.
 * krd, when given, receives the initial matrix: the bits epa_dev_krd returns for the same call.  S == 1 writes nothing to
 * the merge arrays.  n == 0 and samples without entries are legal: distances of 0.0, decided by the tie rule.
 * Every array may be a host or a device pointer.  Validation, its wording (led by "squash:") and the limits are
 * epa_dev_krd's -- S in 1 .. 4096, no topology refused, host arrays checked with the first offending entry named, ids in
 * device arrays found by the kernels and the call refused -- except that n < 2^31 (point storage is addressed with 32
 * bits).  A refused call leaves the context and the results of later calls as they were.
 * Structure (squash.hip).  The initial state is epa_dev_krd's own: its kernels, from one shared text (krd_kernels.hpp),
 * leave the sorted points, M, P, the run starts and the matrix.  Per step: a two-level fixed-shape argmin over the active
 * part of the device-resident matrix; ONE read-back of the winning record (24 bytes); one work item per rank merges the
 * children's runs into the new cluster's point list (sorted by rank, x, sample id, entry order; weight / |C| formed from the
 * original weight) and sums its M the way the run kernel does; the scan kernel forms its P; then one 256-thread workgroup
 * per (active cluster, tile of 1024 ranks) with the new cluster as the fixed side repeats the pair pass's lane -> rank
 * mapping, branch merge, butterfly and four-wave order, and a second kernel adds the partials in tile order into both
 * matrix entries.  The same operations in the same shape on rows formed the same way: hence the same bits.  Late steps
 * launch small grids (active x ceil(B / 1024) workgroups).  The argmin rereads the active part of the matrix every step.
 * Scratch (its own bank, beside epa_dev_krd's): 8 S^2 (matrix) + 12 S B (P and run starts) + 80 n (two arenas of 2 n
 * points of 20 bytes: new lists are appended, and the active lists, which always partition the entries, are compacted
 * into the other arena when one is full) + 48 n of sort keys and indices plus rocPRIM's buffers + 8 S ceil(B / 1024) of
 * row partials, at most 32 MiB of pair partials and a few arrays of S words.
 * Timers: "squash" (the whole call on the device's time line, the host's read-backs included), inside it "squash_init"
 * (the initial state) and, summed over the steps, "squash_argmin", "squash_merge" (list, M, P, compaction) and
 * "squash_row"; "squash_loop_wall" is the host's wall clock around the merge loop (no event pair), for the share of a
 * step that is not kernel time.
 */
int epa_dev_squash(epa_ctx* ctx, const epa_pair* pairs, const double* distal, const double* weight, uint64_t n, uint32_t S,
                   uint32_t* merge_a /* [S-1] */, uint32_t* merge_b /* [S-1] */, double* merge_dist /* [S-1] */,
                   uint32_t* merge_size /* [S-1] */, double* krd /* [S][S] or NULL */);

/*
 * Edge principal components of the S samples (Matsen and Evans 2013; `guppy epca`, `gappa analyze edgepca`): which edges
 * of the reference tree carry the differences between the samples, and where each sample sits on those axes.  The inputs
 * are epa_dev_krd's; root, child(b), rank(b), size(b), M_s, P_s and T_s(b) = P_s[rank + size - 1] - P_s[rank] are those of
 * its description above, computed by its kernels.
 *   W_s            the sample's total, P_s[B - 1]: the scan's last value, not summed again
 *   excluded       branch b with size(b) == 1 (a leaf at the child end) or size(b) == B (a leaf at the root end).  The edge
 *                  next to a leaf has the imbalance +-(W - own mass) and carries no signal (guppy and gappa leave such
 *                  edges out by default): its column is defined as 0.0
 *   X[s][b]        of a kept edge: T_s(b) - ((W_s - T_s(b)) - M_s[rank b]), the mass strictly on the child side minus the
 *                  mass strictly on the root side; the edge's own mass counts for neither.  Three fp64 subtractions in
 *                  this order.  The sign depends on the root (node_prox[0]): flipping an edge's orientation flips that
 *                  edge's entry in every eigenvector and nothing else
 *   mean[b]        (0.0 + X[0][b] + ... + X[S-1][b]) / S, added in ascending s, then one division
 *   Xc[s][b]       X[s][b] - mean[b].  Given X, a restatement reaches Xc bit for bit.  There is no column filter (a
 *                  constant column centres to about 0 and contributes nothing) and no kappa transform
 *   G              Xc Xc^T, [S][S]; the order of the B additions is the kernel's structure and no more.  G replaces the
 *                  B x B covariance matrix (34 GB at 65 537 branches); the two share their non-zero spectrum
 *   eigen-decomposition of G: cyclic two-sided Jacobi in the parallel (round-robin) ordering.  Index set 0 .. m - 1, m = S
 *                  rounded up to even; m - 1 is a dummy when S is odd.  Step t of a sweep pairs positions i and m - 1 - i of
 *                  the circle method's list, which is turned between steps as [idx0, idx_last, idx1 .. idx_{m-2}]: m - 1
 *                  steps per sweep.  Pair (p < q) is rotated iff |a_pq| > 2^-53 max_i |a_ii|, the maximum taken at the
 *                  start of the sweep; theta = (a_qq - a_pp) / (2 a_pq), t = sign(theta) / (|theta| + sqrt(theta^2 + 1))
 *                  with sign(0) = +1, c = 1 / sqrt(t^2 + 1), s = t c.  The loop ends after the first sweep without a
 *                  rotation or after EPCA_MAX_SWEEPS = 30.  (Centring makes G singular: a threshold relative to
 *                  sqrt(a_pp a_qq) does not terminate.)
 *   sweeps         the number of sweeps run, the rotation-free last one included.  Reaching 30 is not an error: the
 *                  results are then what 30 sweeps left
 *   lambda'        the Gram eigenvalues (the diagonal after the loop) sorted descending, equal values by ascending Jacobi
 *                  column; u_k the matching column of the accumulated rotations
 *   eigenvalue[k]  max(lambda'_k, 0) / (S - 1): the eigenvalue of the sample covariance Xc^T Xc / (S - 1)
 *   edge_vec[k][b] sigma_k (sum over s of Xc[s][b] u_k[s]) / sqrt(lambda'_k), added in ascending s: unit length, 0.0 on
 *                  excluded edges
 *   proj[s][k]     sigma_k sqrt(lambda'_k) u_k[s], which equals Xc v_k up to rounding
 *   sigma_k        +-1 such that the entry of edge_vec[k] with the largest |value| is positive; on equal |value| the
 *                  lowest branch id decides
 *   null component lambda'_k <= 2^-40 lambda'_0, or lambda'_0 <= 0: the eigenvalue is reported as above, edge_vec[k] and
 *                  proj[.][k] are all 0.0 (a tree with one inner edge, K beyond the rank, no inner edge at all)
 *   total_var      (sum over i of G[i][i]) / (S - 1), added one after the other from the diagonal as first computed: the
 *                  trace of the covariance, for "fraction of variance"
 *   imbalance      when given: X[s][b] by branch id (not centred);  gram, when given: G
 * The same call returns the same bits every time: no floating-point atomics (the only atomic is the integer count of a
 * sweep's rotations), all tile shapes and the slice length are compile-time constants, nothing depends on the grid.  gram
 * is bit-symmetric: an element is computed once and stored twice, before and during the rotations.
 * Every array may be a host or a device pointer.  Validation and its wording (led by "epca:") are epa_dev_krd's, except
 * that S must be 2 .. 1024 (EPCA_MAX_S; the refusal names the count) and K 1 .. S - 1.  A refused call changes nothing on
 * the context.  n == 0 and samples without entries are legal: their rows of X are zero.  Above 1024 samples the unblocked
 * Jacobi below would re-read a 128 MiB matrix 4095 times per sweep; a blocked solver for that range is not part of this
 * library.
 * Structure (epca.hip).  The table phase of epa_dev_krd (points, two sorts, M, P).  One work item per (branch, sample)
 * writes X edge-major, XT[rank][sample] with the pitch S rounded up to 16, excluded ranks and pad columns 0.0; one work
 * item per rank centres its row.  G: one wave per (pair of 16-sample tiles I <= J, slice of 1024 ranks) accumulates
 * v_mfma_f64_16x16x4_f64 over the slice, four ranks per instruction, into one partial tile; a second kernel adds a tile
 * pair's partials in slice order and stores [a][b] and [b][a].  Jacobi: the host drives, the matrix A and the rotations'
 * product V stay on the device; per step one kernel forms (c, s, t) of the step's pairs (the identity where the threshold
 * skips a pair or the dummy is involved) and counts them, and one kernel with a work item per (pair i <= pair j) forms
 * J_i^T . block . J_j of its 2 x 2 block and stores the block and its mirror image -- item (i, i) writes a_pq = a_qp = 0.0,
 * a_pp - t a_pq and a_qq + t a_pq -- and rotates columns p_i, q_i of V; in place, as the blocks of a step are disjoint.
 * One 4-byte read-back of the rotation count per sweep.  The sort of the eigenvalues runs on the host from one read-back
 * of the diagonal.  At S of a few hundred the Jacobi loop's 2 (S - 1) small launches per sweep dominate the call.
 * Scratch (its own bank): 8 B (S up to 16) (XT) + 16 m^2 (A and V) + 4 m^2 (the steps' pairs) + at most 64 MiB of Gram
 * partials + 8 K B + 8 S K, 8 S^2 and 8 S B more for gram and imbalance when asked, + epa_dev_krd's scratch with M.
 * Timers: "epca" (the whole call on the device's time line, the host's read-backs included), inside it "epca_tables"
 * (points, sorts, M, P, X, centring), "epca_gram", "epca_eig" (the sweeps' kernels, summed over the sweeps) and
 * "epca_project" (edge vectors, signs, projections); "epca_loop_wall" is the host's wall clock around the Jacobi loop (no
 * event pair).
 */
int epa_dev_epca(epa_ctx* ctx, const epa_pair* pairs, const double* distal, const double* weight, uint64_t n, uint32_t S, uint32_t K,
                 double* eigenvalue /* [K] */, double* edge_vec /* [K][B] */, double* proj /* [S][K] */, double* total_var /* [1] */,
                 uint32_t* sweeps /* [1] */, double* imbalance /* [S][B] by branch id, or NULL */, double* gram /* [S][S] or NULL */);

/*
 * Replaces apply_heuristic() for the default dynamic heuristic (src/core/heuristics.hpp:119-127,
 * until_accumulated_reached src/set_manipulators.cpp:90-114) on device, so the Q x B table never
 * leaves HBM: per query, branches in descending LWR order until the accumulated LWR reaches
 * `threshold` (the crossing element included).  lnl is the Q x B table of epa_dev_preplace.
 * Writes at most max_pairs pairs, branch-major sorted (Work iteration order); *n_pairs receives
 * the number selected (if larger than max_pairs the call fails with EPA_ERR_INVALID_ARG).
 */
int epa_dev_select_candidates(epa_ctx* ctx, const double* lnl, uint32_t Q, double threshold,
                              epa_pair* pairs, uint64_t max_pairs, uint64_t* n_pairs);

/*
 * Selection rule used by epa_dev_select_candidates() and epa_dev_place_chunk() of this context
 * (apply_heuristic, src/core/heuristics.hpp:119-127):
 *   EPA_HEUR_DYNAMIC   (default) accumulated LWR >= the call's `threshold`   (--dyn-heur)
 *   EPA_HEUR_FIXED     the ceil(param * B) best branches per query           (--fix-heur,
 *                      until_top_percent src/set_manipulators.cpp:82-88); `threshold` is ignored
 *   EPA_HEUR_BASEBALL  every branch within 3.0 lnL of the best, plus min(40 - hits, 6) more (6 more
 *                      when over 40 were hit: the reference's size_t wrap-around, heuristics.hpp:107)
 *                      (--baseball-heur, heuristics.hpp:70-117, clamped at B)
 */
#define EPA_HEUR_DYNAMIC 0
#define EPA_HEUR_FIXED 1
#define EPA_HEUR_BASEBALL 2
int epa_dev_set_heuristic(epa_ctx* ctx, int mode, double param);

/*
 * The body of the reference's chunk loop for the default configuration (src/core/place.cpp:
 * 219-235): place() -> apply_heuristic() [dynamic, `threshold`] -> place_thorough(), fused so
 * that the Q x B preplacement table never leaves HBM and the host is only consulted once (the
 * candidate count sizes the thorough launch).  pairs / results: caller buffers of max_pairs
 * entries (host or device), filled branch-major; *n_pairs = number of candidate placements.
 * max_span: an upper bound of win_span[] if the caller knows it, 0 to let the library find it.
 */
int epa_dev_place_chunk(epa_ctx* ctx, const uint8_t* q_codes, const uint32_t* win_begin,
                        const uint32_t* win_span, uint32_t Q, uint32_t max_span, double threshold,
                        epa_pair* pairs, epa_result* results, uint64_t max_pairs,
                        uint64_t* n_pairs, epa_thorough_stats* stats);

/*
 * Duplicate queries.  Amplicon and metabarcoding inputs hold each distinct read many times; a query's result does not
 * depend on the other queries of its chunk, so placing one representative per class of identical queries and handing its
 * rows to every member is exact.  (The reference has no counterpart: its users collapse duplicates in a step of their own
 * before placement.)
 * Two queries of a chunk are IDENTICAL when all three of these hold:
 *   - win_begin is equal;
 *   - win_span is equal;
 *   - the codes of the win_span window positions are equal.
 * Nothing else is compared: not the bytes of a compact row between span and stride, not the pad nibble of an odd 4-bit
 * row, not the columns outside the window of a full-width (Q x W) row.  The answer is the same in all three layouts
 * (full-width, compact, compact 4-bit: epa_dev_set_query_layout / _packing).  Queries with win_span == 0 are identical when
 * their win_begin is equal.
 * Classes are numbered in the order of their first appearance in the chunk:
 *   first[u]  the smallest query index of class u; first is strictly increasing
 *   rep[q]    the class of query q; rep[first[u]] == u
 * The result is exact: a 64-bit key of (win_begin, win_span, window codes) only brings candidates together (a stable sort
 * of (key, q) on the key's low bits), every member of a run is then compared code for code with the run's first member of
 * the same key, and a member that differs goes on through the run until it meets an equal row.  No two different rows
 * share a class and no two identical rows are split, whatever the keys do (options "dedup_key_bits", "dedup_sort_bits").
 *   epa_dev_dedup_queries      rep [Q], first [Q] capacity (the first *n_unique entries are written), *n_unique.  An empty
 *                              window is legal here; a window that leaves the alignment or its row is EPA_ERR_QUERY_WIDTH
 *   epa_dev_place_chunk_dedup  the classes as above, the representatives' rows and windows gathered into compacted device
 *                              arrays (the context's own layout and packing, row pitch unchanged), then epa_dev_place_chunk's
 *                              body over those arrays in place.  seq_id of a returned pair is a CLASS index; pairs and
 *                              results are bit for bit those of epa_dev_place_chunk on the representatives' rows alone, in
 *                              that order (max_span: of the whole chunk, 0 = unknown).  EPA_ERR_PAIR_OVERFLOW and the window
 *                              errors (an empty window included, the query named is the chunk's) as in epa_dev_place_chunk;
 *                              rep, first and *n_unique are valid after an overflow.  Both lookup layouts
 * Inputs and outputs may be host or device pointers; Q == 0 returns EPA_OK with *n_unique = 0.  Timer: "dedup" (keys,
 * sort, classes, scan and gather together; the chunk body keeps its own timers).
 * Out of scope: classes across chunks; pipeline slots and group launches; epa_dev_place_all; profile rows.
 */
int epa_dev_dedup_queries(epa_ctx* ctx, const uint8_t* q_codes, const uint32_t* win_begin, const uint32_t* win_span,
                          uint32_t Q, uint32_t* rep /* [Q] */, uint32_t* first /* [Q] capacity */, uint32_t* n_unique);
int epa_dev_place_chunk_dedup(epa_ctx* ctx, const uint8_t* q_codes, const uint32_t* win_begin, const uint32_t* win_span,
                              uint32_t Q, uint32_t max_span, double threshold,
                              epa_pair* pairs, epa_result* results, uint64_t max_pairs, uint64_t* n_pairs,
                              epa_thorough_stats* stats,
                              uint32_t* rep /* [Q] */, uint32_t* first /* [Q] capacity */, uint32_t* n_unique);

/*
 * The same chunk body as a double-buffered pipeline, the device-side counterpart of the
 * reference's read-ahead of the next chunk (src/seq/MSA_Stream.cpp:79-82, the prefetch in
 * src/core/place.cpp:190-215): the query upload of chunk k+1 and the result download of chunk k-1
 * run on a copy stream while the kernels of chunk k run.  Slots 0 .. 23 (the loops below use two; a
 * caller of many small chunks keeps more in flight, see launch_begin), each walks
 *     stage -> launch -> finish -> stage -> ...
 *   stage   copies the caller's HOST arrays (layout / packing as set for the context) into the
 *           slot's pinned buffer and starts the H2D transfer; returns at once.  DEVICE arrays (all
 *           three) are read in place instead: no copy; they must be complete on the context's
 *           stream at launch and stay untouched until finish.
 *   launch  preplace -> heuristic -> thorough on the compute stream as soon as the upload has
 *           landed; blocks only until the candidate count is known (it sizes the thorough launch),
 *           then queues the thorough kernels and the D2H of pairs / results and returns.
 *           d_pairs / d_results: optional DEVICE buffers of max_pairs entries that receive the
 *           results (e.g. the send buffers of a collective); NULL = buffers owned by the slot.
 *           EPA_CHUNK_NO_D2H: results stay in HBM (finish() hands out the device pointers).
 *           EPA_CHUNK_HOST_ORDERED: the caller orders this chunk through the HOST only -- device arrays staged in
 *           place were complete when launch was called, and device-resident results are touched only after finish()
 *           returned.  Without it the library orders the slot's stream behind the context's stream at launch and
 *           the context's stream behind the chunk at the end of launch (stream-ordered consumers); those two event
 *           hops put ~20 us of idle queue between one chunk's Newton kernel and the next chunk's first kernel.
 *   finish  waits for the slot's download; *pairs / *results point into the slot's pinned host
 *           buffer (or HBM with EPA_CHUNK_NO_D2H), valid until the slot is staged again.
 *   launch_begin / launch_end: launch in two halves for callers that keep two chunks in flight --
 *           begin queues preplacement + candidate selection and returns WITHOUT waiting; end waits
 *           for the candidate count (normally long there by then) and queues the rest.  Each slot
 *           has its own stream and scratch, so chunk k + 1's begin-half overlaps chunk k's Newton
 *           kernel on the device:
 *               for k in 0..2: { stage(k, c[k]); begin(k); }
 *               for k: { end(k%5); if (k >= 2) finish((k-2)%5); stage((k+3)%5, c[k+3]); begin((k+3)%5); }
 *           (five slots: chunk k's Newton kernel is queued while chunk k-1's still runs and fills
 *           its tail wave by wave -- what small chunks need: 6.6 -> 8.3 M placements/s at 5000 reads
 *           per chunk against the two-slot order; bench.py's chunk5000 leg).  For large chunks two
 *           slots do: begin(k&1); finish((k-1)&1); stage((k+1)&1); end(k&1).
 * A typical loop:  stage(0, c0); for k: { launch(k&1); finish((k-1)&1); stage((k+1)&1, c[k+1]); }
 * Candidate overflow (EPA_ERR_PAIR_OVERFLOW from launch, as epa_dev_place_chunk) leaves the slot
 * staged: launch again with a larger max_pairs.
 */
#define EPA_CHUNK_NO_D2H 0x1u
#define EPA_CHUNK_HOST_ORDERED 0x2u
int epa_dev_chunk_stage(epa_ctx* ctx, int slot, const uint8_t* q_codes, const uint32_t* win_begin,
                        const uint32_t* win_span, uint32_t Q);
int epa_dev_chunk_launch(epa_ctx* ctx, int slot, uint32_t max_span, double threshold,
                         epa_pair* d_pairs, epa_result* d_results, uint64_t max_pairs,
                         uint32_t flags);
int epa_dev_chunk_launch_begin(epa_ctx* ctx, int slot, uint32_t max_span, double threshold,
                               epa_pair* d_pairs, epa_result* d_results, uint64_t max_pairs,
                               uint32_t flags);
int epa_dev_chunk_launch_end(epa_ctx* ctx, int slot);
int epa_dev_chunk_finish(epa_ctx* ctx, int slot, const epa_pair** pairs, const epa_result** results,
                         uint64_t* n_pairs, epa_thorough_stats* stats);

/*
 * Small chunks (the reference's default --chunk-size is 5000, src/util/Options.hpp:26; the chunk body of
 * src/core/place.cpp:207-246 then runs once per 5000 reads): every launch of the Newton kernel costs a fixed
 * ~0.11 ms, a preplacement over a handful of query groups another ~0.15 ms, and a chunk body is ~23 dispatches.
 * A GROUP LAUNCH runs ONE chunk body -- one preplacement, one selection, one Newton launch -- over the
 * concatenated queries of up to 8 STAGED slots and regroups the rows by chunk afterwards:
 *   launch_many_begin  slots[0] is the group's leader; every listed slot must be staged (same query layout).
 *                      Queues merge + preplacement + selection on the leader's stream, returns without waiting.
 *                      max_pairs bounds the candidates of the WHOLE group; results live in library buffers.
 *   epa_dev_chunk_launch_end(ctx, slots[0])   as for a single slot: waits for the candidate count, queues the
 *                      Newton kernel, the regrouping and the D2H (one copy per group)
 *   epa_dev_chunk_finish(ctx, slot) for EVERY member, in any order: that chunk's rows, bit-identical to a launch
 *                      of its own -- branch-major, queries ascending, sequence ids local to the chunk -- as a
 *                      range of the leader's buffers: valid until the LEADER is staged again, which is refused
 *                      while members are unfinished.  The Newton counters of the one launch are reported with
 *                      slots[0] (the other members report their pair count only).
 * EPA_ERR_PAIR_OVERFLOW and the window errors leave every member staged.  A loop for 5000-read chunks, groups
 * of four on twelve slots, two groups begun ahead (bench.py's chunk5000 leg):
 *     stage + many_begin(g0); stage + many_begin(g1);
 *     for g: { launch_end(leader(g)); finish(members of g-1); stage + many_begin(g+2); }
 */
int epa_dev_chunk_launch_many_begin(epa_ctx* ctx, const int* slots, int n_slots, uint32_t max_span,
                                    double threshold, uint64_t max_pairs, uint32_t flags);
int epa_dev_chunk_launch_many(epa_ctx* ctx, const int* slots, int n_slots, uint32_t max_span, double threshold,
                              uint64_t max_pairs, uint32_t flags);

/*
 * --no-heur (src/core/place.cpp:189,228: every branch gets a thorough placement) with the
 * post-processing of the chunk loop fused in: thorough optimisation of all B x Q pairs (pairs are
 * generated on the device), then per query compute_and_set_lwr over all B placements and filter()
 * (src/set_manipulators.cpp:43-69,131-204) on the device, so that only the surviving placements
 * cross PCIe.  acc_threshold == 0: discard_by_support_threshold (keep lwr > min_lwr, at least
 * filter_min, at most filter_max); != 0: discard_by_accumulated_threshold (the reference's
 * min - 1 top-up quirk included).  1 <= filter_min <= filter_max <= 64.
 * Outputs (host or device buffers): query q owns slots [q*filter_max, q*filter_max + counts[q]) of
 * pairs / results / lwr, best placement first.
 */
int epa_dev_place_all(epa_ctx* ctx, const uint8_t* q_codes, const uint32_t* win_begin,
                      const uint32_t* win_span, uint32_t Q, uint32_t max_span, double min_lwr,
                      int acc_threshold, uint32_t filter_min, uint32_t filter_max, epa_pair* pairs,
                      epa_result* results, double* lwr, uint32_t* counts,
                      epa_thorough_stats* stats);

/*
 * Multi-GPU: one process per GPU.  Queries are split into contiguous per-rank slices without any
 * exchange (src/net/epa_mpi_util.cpp:10-30, local_seq_package); the path's ONLY collective is the
 * gather of every chunk's (pair, result) rows to rank 0, which writes the jplace
 * (src/io/jplace_writer.hpp:117-129 gathers the ranks' text with MPI_Gatherv; here the 32-byte numeric
 * rows travel over RCCL: point-to-point xGMI links into the root, one group per chunk).
 *   epa_comm_get_unique_id  rank 0: 128 bytes to hand to the other ranks out of band (a file, an
 *                           environment variable, MPI_Bcast -- whatever launched the processes)
 *   epa_comm_create         collective (ncclCommInitRank).  rows_cap: rows per rank and gather (size it
 *                           from the expected candidates per chunk, e.g. 4 x reads); depth: send /
 *                           receive slots used round robin (2: gather k travels while chunk k + 1 runs)
 *   epa_dev_gather_results  collective, asynchronous, every rank once per chunk in the same order:
 *                           packs n rows (DEVICE pairs / results, complete on the context's stream;
 *                           sequence ids + seq_offset = global ids) and posts the fixed-size exchange on
 *                           the communicator's own stream.  Never blocks the host; rows beyond rows_cap
 *                           are carried into the rank's next gather.  *ticket names the gather.
 *   epa_dev_gather_slot     the same for a chunk slot launched with EPA_CHUNK_NO_D2H (after launch_end)
 *   epa_comm_collect        rank 0: waits for gather `ticket` (at most the communicator's timeout), copies its VALID rows to pinned host
 *                           memory and hands out one row block and count per rank; the blocks stay
 *                           valid until gather ticket + depth is posted.  pending[r] (optional): rows rank
 *                           r still carried after this gather -- 0 means every row it has posted so far
 *                           has arrived (a chunk's rows are branch-major: a query is complete only then)
 *   epa_comm_flush          collective, at the end, REPEATED until it reports *n_extra == 0: agrees (one
 *                           all-reduce) on whether any rank still carries rows and posts up to `depth` extra
 *                           gathers (tickets *first .. *first + *n_extra - 1) that drain them; rank 0
 *                           collects those before the next call
 *   epa_comm_probe          collective, optional, right after create: one round trip through everything a gather
 *                           uses (a one-row gather naming each rank and the PCI id of its device, then an all-reduce),
 *                           every wait bounded by timeout_s -- so that a transport that cannot move data between THESE
 *                           processes shows up in seconds, before any work depends on it, instead of as a gather that
 *                           never completes.  Rank 0 receives device_ids[world] = (pci domain << 16 | bus << 8 | device)
 *                           of every rank's GPU ("RCCL saw N ranks on N devices").  On failure: epa_comm_abort.
 *   epa_comm_set_timeout    seconds a host-side wait of this communicator may take (collect, flush, probe); comm ==
 *                           NULL sets the process default, which also bounds epa_comm_create (ncclCommInitRank waits
 *                           for all ranks).  Default: EPA_COMM_TIMEOUT_S, else 600.
 * RCCL is loaded at run time (dlopen): EPA_ERR_UNSUPPORTED without it.  Which library: the path given to
 * epa_comm_set_library() (before the first communicator); else the environment's EPA_RCCL_LIB; else a librccl ALREADY
 * MAPPED in the process (a host program that brought its own RCCL -- PyTorch ships torch/lib/librccl.so -- must not get a
 * second copy beside it); else librccl.so.1 / librccl.so on the loader's search path (LD_LIBRARY_PATH), /opt/rocm/lib.
 * epa_comm_library_path() names the file that was bound ("" if none): log it.
 */
#define EPA_COMM_ID_BYTES 128
typedef struct epa_comm epa_comm;
typedef struct {
  uint32_t branch_id, seq_id;   /* seq_id is GLOBAL (rank's offset added) */
  double lnl, pendant_length, distal_length;
} epa_row;
int epa_comm_set_library(const char* path);
const char* epa_comm_library_path(void);
int epa_comm_set_timeout(epa_comm* comm_or_null, double seconds);
int epa_comm_get_unique_id(void* id128);
int epa_comm_create(epa_ctx* ctx, const void* id128, int rank, int world, uint32_t rows_cap, int depth,
                    epa_comm** out);
void epa_comm_destroy(epa_comm* comm);
int epa_comm_probe(epa_ctx* ctx, epa_comm* comm, double timeout_s, uint64_t* device_ids);
/* test hook: rank 0's own rows travel through ncclSend / ncclRecv to itself instead of a local copy (before the
 * first gather only) */
int epa_comm_set_self_send(epa_comm* comm, int on);
int epa_dev_gather_results(epa_ctx* ctx, epa_comm* comm, const epa_pair* d_pairs, const epa_result* d_results,
                           uint64_t n, uint32_t seq_offset, uint64_t* ticket);
int epa_dev_gather_slot(epa_ctx* ctx, epa_comm* comm, int slot, uint32_t seq_offset, uint64_t* ticket);
/* --no-heur (src/core/place.cpp:219-231 with prescoring == false) in the one-process-per-GPU mode: epa_dev_place_all with
 * its filtered placements left in HBM as gather rows -- per kept placement, best first, its row followed by a row
 * {branch_id = EPA_ROW_LWR, seq_id, lnl = its like-weight ratio} (normalised over ALL branches on the device: it cannot
 * be recomputed from the kept rows) -- and epa_dev_gather_rows posts such rows (collective, asynchronous, carry-over:
 * exactly as epa_dev_gather_results).  *d_rows stays valid until the context's next place_all_rows call. */
#define EPA_ROW_LWR 0xfffffffeu
int epa_dev_place_all_rows(epa_ctx* ctx, const uint8_t* q_codes, const uint32_t* win_begin, const uint32_t* win_span,
                           uint32_t Q, uint32_t max_span, double min_lwr, int acc_threshold, uint32_t filter_min,
                           uint32_t filter_max, uint32_t seq_offset, const epa_row** d_rows, uint64_t* n_rows,
                           epa_thorough_stats* stats);
int epa_dev_gather_rows(epa_ctx* ctx, epa_comm* comm, const epa_row* d_rows, uint64_t n, uint64_t* ticket);
int epa_comm_collect(epa_comm* comm, uint64_t ticket, const epa_row** rows, uint32_t* counts, uint64_t* pending);
/* rows == NULL in epa_comm_collect: counts / pending only, the rows stay in HBM; this is rank r's block
 * of gather `ticket` there (valid until gather ticket + depth is posted; NULL if the slot was reused) */
const epa_row* epa_comm_device_rows(const epa_comm* comm, uint64_t ticket, int rank);
int epa_comm_flush(epa_ctx* ctx, epa_comm* comm, uint64_t* first_extra_ticket, uint32_t* n_extra);
uint64_t epa_comm_carried_rows(const epa_comm* comm);
/* a rank that fails mid-job: ncclCommAbort + release, without waiting for the peers (their pending
 * collect / flush calls then fail or time out after the communicator's timeout, default 600 s, instead of
 * blocking for ever; the reference's MPI build aborts the whole job, src/main.cpp's MPI_Abort path) */
void epa_comm_abort(epa_comm* comm);

/* free / total bytes of the context's device (hipMemGetInfo): the chunk loop sizes its device chunks
 * against it -- every pipeline slot in use keeps its own preplacement table of Q x pitch(B) x 8 bytes
 * live (the CLI's loop owns 4 slots and budgets 4 tables plus a quarter within half of the free bytes;
 * `--chunk-size` is the user's memory knob, src/main.cpp:234-238). */
int epa_dev_mem_info(epa_ctx* ctx, uint64_t* free_bytes, uint64_t* total_bytes);

/* Diagnostics, no reference counterpart: the shares of a Newton launch's (branch-sorted) pair list that the device's
 * eight XCDs currently take.  0.125 each on a new context; every launch of one span class that ran for >= 1 ms reports
 * when each XCD ran out of pairs, and the next launches' shares move half way toward share / time (the XCDs of one
 * MI355X differ in speed by a few per cent: DESIGN.md 4.1).  Results do not depend on the shares. */
int epa_dev_xcd_shares(const epa_ctx* ctx, double shares[8]);

/* Diagnostics, no reference counterpart: the shader clock (MHz) the last single-class Newton launch really ran
 * at -- shader cycles (s_memtime) over 100 MHz ticks (s_memrealtime) of the launch's first wave, which lives as
 * long as the launch.  0 before the first such launch.  The bench line prices the kernel's fp64 rate against the
 * peak AT THIS CLOCK next to the spec-sheet peak at 2400 MHz (roofline.sclk_mhz, frac_at_measured_clock). */
double epa_dev_last_sclk_mhz(const epa_ctx* ctx);

/* duration in milliseconds of the last launch of the named kernel family on ctx's stream,
 * measured with HIP events ("preplace", "thorough", "lookup", "select", "score_at", "site_lnl", "rell", "marginal", "rell_tests", "rell_au", "rell_kh", "preplace_profile", "dedup", "edpl", "krd", "krd_sort", "krd_tables", "krd_pairs", "squash", "squash_init", "squash_argmin", "squash_merge", "squash_row", "squash_loop_wall", "epca", "epca_tables", "epca_gram", "epca_eig", "epca_project", "epca_loop_wall"); < 0 if never run.
 * Blocked lookup layout: "lookup_block" = the table builds of the last chunk body, summed over its
 * blocks; "preplace" = its preplacement kernels, summed likewise (the builds are not part of it). */
double epa_dev_last_kernel_ms(const epa_ctx* ctx, const char* which);

#ifdef __cplusplus
}
#endif
#endif /* EPA_DEV_H */
