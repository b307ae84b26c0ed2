// Profile queries: a query given as one row of per-state likelihoods per window position (include/epa_dev.h,
// "Profile queries") instead of one column code per site -- reads with base qualities, consensus or HMM columns.
//
// The site likelihood is linear in the query's tip vector, so the path differs from the coded one in three places:
//   k_profile_eigen     validates the rows and brings them to the eigenbasis once per call: qe = U^-1 v.  The general
//                       Newton kernel and k_score_at read qe where they read ModelDev::qt[code] (their PROFILE
//                       instantiations, thorough_generic.hip / score_at.hip)
//   k_profile_table     once per context: per (branch, site) the lookup table's pure-state columns relative to the
//                       any-state column, exp(T_m - T_any), which do not depend on the query
//   k_preplace_profile  the preplacement: per (query, branch) the window's product of sum_m v_m exp(T_m - T_any), kept
//                       as mantissa and exponent, plus the sum of T_any
// and in the entry points that stage the rows (this file; epa_dev_score_at_profile / _site_lnl_profile: epa_dev.hip).
#include "epa_dev_internal.hpp"
#include "wave_util.hpp"

#include <math.h>
#include <string.h>

#include <algorithm>

// ---- what a valid row is, on the host and on the device alike
// 0: valid; else the first fault in this order: an entry that is not finite, a negative entry, an all-zero row, a row
// whose largest entry lies outside [2^-64, 2^64]
template <int S>
__host__ __device__ static inline int profile_row_fault_s(const double* v) {
  double mx = 0.0;
#pragma unroll
  for (int m = 0; m < S; ++m) {
    const double x = v[m];
    if (!(x - x == 0.0)) return 1;   // NaN or infinite
    if (x < 0.0) return 2;
    mx = x > mx ? x : mx;
  }
  if (mx == 0.0) return 3;
  if (mx < 0x1p-64 || mx > 0x1p+64) return 4;
  return 0;
}
static inline int profile_row_fault(const double* v, int S) { return S == 4 ? profile_row_fault_s<4>(v) : profile_row_fault_s<20>(v); }

static const char* profile_fault_text(int fault) {
  switch (fault) {
    case 1: return "an entry is not finite";
    case 2: return "an entry is negative";
    case 3: return "every entry of the row is zero";
    default: return "the row's largest entry lies outside [2^-64, 2^64]";
  }
}

static int profile_row_error(epa_ctx* ctx, const char* who, uint32_t q, uint32_t j, int fault) {
  return epa_fail(ctx, EPA_ERR_INVALID_ARG, std::string(who) + ": query " + std::to_string(q) + " position " + std::to_string(j) +
                                                ": " + profile_fault_text(fault));
}

namespace {

using namespace epa_wave;

constexpr double LN2 = 0.6931471805599453094;
constexpr unsigned long long NO_FAULT = ~0ull;
// branches per work item of k_preplace_profile: the query's row is loaded once per 64-site chunk and meets this many
// branches' table rows; the accumulators of all of them live in registers
constexpr int PRE_TB = 8;

// qe[(q stride + j) S + x] = 0.0 + sum_{m ascending} Ui[x][m] v_m: the order of the loop that fills ModelDev::qt
// (epa_dev.hip, create_impl), so that a 0/1 row gives the bits of qt[column of that state set].  One thread per window
// position; rows from the span up to the stride are padding, neither read nor written.  The first faulty row in (query,
// position) order lands in *fault_key as (q << 32 | j).
template <int S>
__global__ void __launch_bounds__(256) k_profile_eigen(const ModelDev* __restrict__ m, const double* __restrict__ prof,
                                                       const uint32_t* __restrict__ span, uint32_t Q, uint32_t stride,
                                                       double* __restrict__ qe, unsigned long long* __restrict__ fault_key) {
  __shared__ double Ui[S * S];
  for (int i = threadIdx.x; i < S * S; i += 256) Ui[i] = m->Ui[i];
  __syncthreads();
  const uint64_t total = (uint64_t)Q * stride;
  for (uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (uint64_t)gridDim.x * 256) {
    const uint32_t q = (uint32_t)(idx / stride), j = (uint32_t)(idx - (uint64_t)q * stride);
    if (j >= span[q]) continue;
    double v[S];
#pragma unroll
    for (int x = 0; x < S; ++x) v[x] = prof[idx * S + x];
    if (profile_row_fault_s<S>(v)) atomicMin(fault_key, ((unsigned long long)q << 32) | j);
    // (20 states: the rows of U^-1 stay in LDS and are read where they are used; unrolled over x they were all hoisted
    // into registers and spilled)
#pragma unroll(S == 4 ? 4 : 1)
    for (int x = 0; x < S; ++x) {
      double acc = 0.0;
#pragma unroll
      for (int i = 0; i < S; ++i) acc += Ui[x * S + i] * v[i];
      qe[idx * S + x] = acc;
    }
  }
}

// lookup columns of the S pure states and of "any state" (from ModelDev::colmask, host side)
struct ProfCols {
  int pure[EPA_MAX_STATES];
  int any;
};

// tab [B][S + 2][W], component-major like refT so that 64 consecutive sites of one component are one 512-byte segment:
//   m < S   e_m = exp(T[b][site][pure column m] - T_any): the site likelihood of state m relative to "any state"
//   S       T_any = T[b][site][any-state column] (it carries the scaler counts)
//   S + 1   +I: every column holds the invariant term c once, so sum_m v_m e_m counts it sum(v) times; c at the table's
//           own scale is (sum_m e_m - 1) / (S - 1), whatever the scaler count.  Exactly 0 where the site is not invariant
//           (cinv says so), hence no rounding residue there
template <int S>
__global__ void __launch_bounds__(256) k_profile_table(const double* __restrict__ lookup, const double* __restrict__ cinv,
                                                       const ProfCols cols, int ncols, uint32_t W, uint32_t b0,
                                                       double* __restrict__ tab) {
  const uint32_t site = blockIdx.x * 256 + threadIdx.x;
  if (site >= W) return;
  const uint32_t b = b0 + blockIdx.y;   // b0: first branch of this slice of the launch (grid.y limit)
  const double* T = lookup + ((size_t)b * W + site) * ncols;
  double* out = tab + (size_t)b * (S + 2) * W + site;
  const double tn = T[cols.any];
  double sum = 0.0;
#pragma unroll
  for (int m = 0; m < S; ++m) {
    const double e = tn == -INFINITY ? 0.0 : exp(T[cols.pure[m]] - tn);
    out[(size_t)m * W] = e;
    sum += e;
  }
  out[(size_t)S * W] = tn;
  out[(size_t)(S + 1) * W] = (cinv && cinv[site] != 0.0) ? fmax((sum - 1.0) / (double)(S - 1), 0.0) : 0.0;
}

struct PreProfArgs {
  const double* tab;       // [B][S + 2][W]
  const double* prof;      // [Q][stride][S] state-space rows
  const uint32_t* win_begin;
  const uint32_t* win_span;
  double* lnl;             // [Q][pitch]
  uint32_t Q, B, W, stride, pitch;
};

// lnl[q pitch + b] = sum over the window of T_any + log(sum_m v_m e_m - (sum(v) - 1) c): one wavefront per (tile of
// PRE_TB branches, query), lane = site of the window (runtime loop over 64-site chunks), a persistent grid over the work
// items -- queries fastest, so that the waves in flight share a tile's table rows.  The window's product is kept as
// mantissa and exponent per lane (one log per lane and branch, not one per site), T_any is summed beside it.
// A window the validation refuses (empty, past the width, longer than the stride) is not read: its row is 0.0.
// INV: the reference has +I; without it component S + 1 is 0 everywhere and is not read.
template <int S, bool INV>
__global__ void __launch_bounds__(64) k_preplace_profile(const PreProfArgs a) {
  const int lane = threadIdx.x;
  const uint32_t nbt = (a.B + PRE_TB - 1) / PRE_TB;
  const uint64_t items = (uint64_t)nbt * a.Q;
  const size_t cW = a.W;
  for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint32_t tile = (uint32_t)(item / a.Q), q = (uint32_t)(item - (uint64_t)tile * a.Q);
    const uint32_t b0 = tile * PRE_TB, nb = min((uint32_t)PRE_TB, a.B - b0);
    const uint32_t begin = a.win_begin[q], n = a.win_span[q];
    const bool ok = n > 0 && n <= a.stride && (uint64_t)begin + n <= a.W;
    const uint32_t nch = ok ? (n + 63) / 64 : 0;
    double mant[PRE_TB], tsum[PRE_TB];
    int ex[PRE_TB];
#pragma unroll
    for (int t = 0; t < PRE_TB; ++t) { mant[t] = 1.0; tsum[t] = 0.0; ex[t] = 0; }
    for (uint32_t ch = 0; ch < nch; ++ch) {
      const uint32_t site = ch * 64 + lane;
      const bool valid = site < n;
      const uint32_t s = valid ? site : 0;
      const double* vr = a.prof + ((size_t)q * a.stride + s) * S;
      double v[S], sv = 0.0;
#pragma unroll
      for (int m = 0; m < S; ++m) { v[m] = vr[m]; sv += v[m]; }
      const double over = 1.0 - sv;   // -(sum(v) - 1)
#pragma unroll
      for (int t = 0; t < PRE_TB; ++t) {
        if ((uint32_t)t < nb) {   // wave-uniform
          const double* E = a.tab + (size_t)(b0 + t) * (S + 2) * cW + begin + s;
          double dot = 0.0;
#pragma unroll
          for (int m = 0; m < S; ++m) dot = fma(v[m], E[(size_t)m * cW], dot);
          double l = dot;
          if constexpr (INV) l = fma(over, E[(size_t)(S + 1) * cW], dot);
          double tn = E[(size_t)S * cW];
          if (!valid) { l = 1.0; tn = 0.0; }
          mant[t] *= __builtin_amdgcn_frexp_mant(l);
          ex[t] += __builtin_amdgcn_frexp_exp(l);
          ex[t] += __builtin_amdgcn_frexp_exp(mant[t]);
          mant[t] = __builtin_amdgcn_frexp_mant(mant[t]);
          tsum[t] += tn;
        }
      }
    }
    double mine = 0.0;
#pragma unroll
    for (int t = 0; t < PRE_TB; ++t) {
      const double r = wave_sum(log(mant[t]) + (double)ex[t] * LN2 + tsum[t]);
      if (lane == t) mine = r;
    }
    if ((uint32_t)lane < nb) a.lnl[(size_t)q * a.pitch + b0 + lane] = ok ? mine : 0.0;
  }
}

}  // namespace

// ---- staging

// The windows of a profile call as the host sees them: as check_windows of the coded calls, with the rows' stride in
// place of the compact code stride
static int profile_windows(epa_ctx* ctx, const char* who, const uint32_t* hb, const uint32_t* hs, uint32_t Q, uint32_t stride,
                           bool allow_empty, uint32_t* max_span) {
  uint32_t mx = 0;
  for (uint32_t q = 0; q < Q; ++q) {
    if (hs[q] == 0 && !allow_empty)
      return epa_fail(ctx, EPA_ERR_QUERY_ALL_GAP, "Sequence " + std::to_string(q) + " does not appear to have any non-gap sites!");
    if ((uint64_t)hb[q] + hs[q] > ctx->W)
      return epa_fail(ctx, EPA_ERR_QUERY_WIDTH, "Query sequence length not same as reference alignment!");
    if (hs[q] > stride)
      return epa_fail(ctx, EPA_ERR_INVALID_ARG, std::string(who) + ": query " + std::to_string(q) + ": the window (" +
                                                    std::to_string(hs[q]) + ") is longer than the profile stride (" +
                                                    std::to_string(stride) + ")");
    mx = std::max(mx, hs[q]);
  }
  *max_span = mx;
  return EPA_OK;
}

int epa_profile_stage(epa_ctx* ctx, const char* who, const double* prof, uint32_t stride, const uint32_t* hb,
                      const uint32_t* hs, const uint32_t* d_span, uint32_t Q, bool allow_empty, uint32_t* max_span,
                      const double** d_prof_out, const double** d_qe_out) {
  if (stride == 0) return epa_fail(ctx, EPA_ERR_INVALID_ARG, std::string(who) + ": the profile stride is 0");
  int rc = profile_windows(ctx, who, hb, hs, Q, stride, allow_empty, max_span);
  if (rc) return rc;
  const int S = ctx->s;
  const size_t rows = (size_t)Q * stride;
  const bool on_host = !epa_is_device_ptr(prof);
  if (on_host)   // host rows are validated here, the first offender in (query, position) order is named
    for (uint32_t q = 0; q < Q; ++q)
      for (uint32_t j = 0; j < hs[q]; ++j)
        if (const int fault = profile_row_fault(prof + ((size_t)q * stride + j) * S, S)) return profile_row_error(ctx, who, q, j, fault);
  const double* d_prof = (const double*)epa_to_device(ctx, SLOT_PROFILE, prof, sizeof(double) * rows * S);
  char* base = (char*)epa_scratch(ctx, SLOT_PROFILE_EIGEN, 256 + sizeof(double) * rows * S);
  if (!d_prof || !base) return epa_fail(ctx, EPA_ERR_HIP, std::string(who) + ": profile upload failed");
  unsigned long long* d_key = (unsigned long long*)base;
  double* d_qe = (double*)(base + 256);
  EPA_HIP(ctx, hipMemsetAsync(d_key, 0xff, sizeof(unsigned long long), ctx->stream));
  const uint32_t grid = (uint32_t)std::min<uint64_t>((rows + 255) / 256, (uint64_t)ctx->n_cu * 16);
  if (S == 4) hipLaunchKernelGGL(k_profile_eigen<4>, dim3(grid), dim3(256), 0, ctx->stream, ctx->dmodel, d_prof, d_span, Q, stride, d_qe, d_key);
  else hipLaunchKernelGGL(k_profile_eigen<20>, dim3(grid), dim3(256), 0, ctx->stream, ctx->dmodel, d_prof, d_span, Q, stride, d_qe, d_key);
  EPA_HIP(ctx, hipGetLastError());
  if (!on_host) {   // device rows: the kernel's status word, and the offending row itself for the reason
    unsigned long long key = NO_FAULT;
    EPA_HIP(ctx, hipMemcpyAsync(&key, d_key, sizeof(key), hipMemcpyDeviceToHost, ctx->stream));
    EPA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (key != NO_FAULT) {
      const uint32_t q = (uint32_t)(key >> 32), j = (uint32_t)key;
      double row[EPA_MAX_STATES];
      EPA_HIP(ctx, hipMemcpy(row, d_prof + ((size_t)q * stride + j) * S, sizeof(double) * S, hipMemcpyDeviceToHost));
      return profile_row_error(ctx, who, q, j, profile_row_fault(row, S));
    }
  }
  *d_prof_out = d_prof;
  *d_qe_out = d_qe;
  return EPA_OK;
}

// the call's three host-or-device arrays staged: windows read (and checked) on the host, rows validated and transformed
namespace {
struct ProfileCall {
  std::vector<uint32_t> hb_buf, hs_buf;
  const uint32_t *d_begin = nullptr, *d_span = nullptr;
  const double *d_prof = nullptr, *d_qe = nullptr;
  uint32_t max_span = 0;
  int stage(epa_ctx* ctx, const char* who, const double* prof, uint32_t stride, const uint32_t* win_begin,
            const uint32_t* win_span, uint32_t Q) {
    const uint32_t* hb = host_view(win_begin, Q, hb_buf, ctx->stream);
    const uint32_t* hs = host_view(win_span, Q, hs_buf, ctx->stream);
    if (!hb || !hs) return epa_fail(ctx, EPA_ERR_HIP, "cannot read window arrays");
    d_begin = (const uint32_t*)epa_to_device(ctx, SLOT_BEGIN, win_begin, sizeof(uint32_t) * Q);
    d_span = (const uint32_t*)epa_to_device(ctx, SLOT_SPAN, win_span, sizeof(uint32_t) * Q);
    if (!d_begin || !d_span) return epa_fail(ctx, EPA_ERR_HIP, std::string(who) + ": query upload failed");
    return epa_profile_stage(ctx, who, prof, stride, hb, hs, d_span, Q, false, &max_span, &d_prof, &d_qe);
  }
};
}  // namespace

// ---- preplacement

static int profile_needs_resident(epa_ctx* ctx, const char* who) {
  if (!ctx->lookup_blocks) return EPA_OK;
  return epa_fail(ctx, EPA_ERR_UNSUPPORTED, std::string(who) + ": profile queries are preplaced from the resident lookup table; this "
                                            "context keeps it in blocks (--memsave)");
}

// the resident lookup table, and (first call) the table derived from it
static int profile_table(epa_ctx* ctx) {
  int rc = epa_dev_build_lookup(ctx);
  if (rc || ctx->prof_tab) return rc;
  const int S = ctx->s;
  ProfCols cols;
  cols.any = -1;
  for (int m = 0; m < EPA_MAX_STATES; ++m) cols.pure[m] = -1;
  const uint32_t all = (S == 4 ? 0xfu : 0xfffffu);
  for (int col = ctx->ncols - 1; col >= 0; --col) {   // descending: the first column of a state set wins
    const uint32_t mask = ctx->hmodel.colmask[col];
    if (mask == all) cols.any = col;
    for (int m = 0; m < S; ++m) if (mask == (1u << m)) cols.pure[m] = col;
  }
  // (quirk D4, aa_x_as_n, gives the 'X' column asparagine's mask; 'N' itself is the earlier column and wins)
  for (int m = 0; m < S; ++m) if (cols.pure[m] < 0 || cols.any < 0) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "profile table: the lookup table lacks a pure-state column");
  double* tab = nullptr;
  if (hipMalloc(&tab, sizeof(double) * (size_t)ctx->B * (S + 2) * ctx->W) != hipSuccess) {
    (void)hipGetLastError();
    return epa_fail(ctx, EPA_ERR_HIP, "hipMalloc(profile table)");
  }
  for (uint32_t b0 = 0; b0 < ctx->B; b0 += EPA_GRID_Y) {   // branch in grid.y, in slices of its limit
    const dim3 grid((ctx->W + 255) / 256, std::min<uint32_t>(EPA_GRID_Y, ctx->B - b0));
    if (S == 4) hipLaunchKernelGGL(k_profile_table<4>, grid, dim3(256), 0, ctx->stream, ctx->lookup, ctx->cinv, cols, ctx->ncols, ctx->W, b0, tab);
    else hipLaunchKernelGGL(k_profile_table<20>, grid, dim3(256), 0, ctx->stream, ctx->lookup, ctx->cinv, cols, ctx->ncols, ctx->W, b0, tab);
  }
  if (hipGetLastError() != hipSuccess) { (void)hipFree(tab); return epa_fail(ctx, EPA_ERR_HIP, "k_profile_table launch failed"); }
  ctx->prof_tab = tab;
  return EPA_OK;
}

static int launch_preplace_profile(epa_ctx* ctx, const ProfileCall& c, uint32_t stride, uint32_t Q, double* d_lnl, uint32_t pitch) {
  PreProfArgs a;
  a.tab = ctx->prof_tab;
  a.prof = c.d_prof;
  a.win_begin = c.d_begin;
  a.win_span = c.d_span;
  a.lnl = d_lnl;
  a.Q = Q;
  a.B = ctx->B;
  a.W = ctx->W;
  a.stride = stride;
  a.pitch = pitch;
  // persistent grid: neither the branch nor the query reaches a grid dimension
  const uint64_t items = (uint64_t)((ctx->B + PRE_TB - 1) / PRE_TB) * Q;
  const uint32_t grid = (uint32_t)std::min<uint64_t>(items, (uint64_t)ctx->n_cu * 16);
  epa_timer_start(ctx, epa_t(ctx, epa_ctx::T_PREPLACE_PROFILE));
  const bool inv = ctx->cinv != nullptr;
  if (ctx->s == 4 && inv) hipLaunchKernelGGL((k_preplace_profile<4, true>), dim3(grid), dim3(64), 0, ctx->stream, a);
  else if (ctx->s == 4) hipLaunchKernelGGL((k_preplace_profile<4, false>), dim3(grid), dim3(64), 0, ctx->stream, a);
  else if (inv) hipLaunchKernelGGL((k_preplace_profile<20, true>), dim3(grid), dim3(64), 0, ctx->stream, a);
  else hipLaunchKernelGGL((k_preplace_profile<20, false>), dim3(grid), dim3(64), 0, ctx->stream, a);
  epa_timer_stop(ctx, epa_t(ctx, epa_ctx::T_PREPLACE_PROFILE));
  EPA_HIP(ctx, hipGetLastError());
  return EPA_OK;
}

extern "C" int epa_dev_preplace_profile(epa_ctx* ctx, const double* prof, uint32_t stride, const uint32_t* win_begin,
                                        const uint32_t* win_span, uint32_t Q, double* lnl) {
  if (!ctx || !prof || !win_begin || !win_span || !lnl) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "null argument");
  if (Q == 0) return EPA_OK;
  EPA_HIP(ctx, hipSetDevice(ctx->device));
  int rc = profile_needs_resident(ctx, "preplace_profile");
  if (!rc) rc = profile_table(ctx);
  if (rc) return rc;
  ProfileCall c;
  rc = c.stage(ctx, "preplace_profile", prof, stride, win_begin, win_span, Q);
  if (rc) return rc;
  const bool out_dev = epa_is_device_ptr(lnl);
  double* d_lnl = out_dev ? lnl : (double*)epa_scratch(ctx, SLOT_TABLE, sizeof(double) * (size_t)Q * ctx->B);
  if (!d_lnl) return epa_fail(ctx, EPA_ERR_HIP, "hipMalloc(lnl)");
  rc = launch_preplace_profile(ctx, c, stride, Q, d_lnl, ctx->B);
  if (rc) return rc;
  if (!out_dev) EPA_HIP(ctx, hipMemcpyAsync(lnl, d_lnl, sizeof(double) * (size_t)Q * ctx->B, hipMemcpyDeviceToHost, ctx->stream));
  EPA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return EPA_OK;
}

// ---- Newton step: always the general kernel

// the Newton launch over n pairs on device buffers, its statistics read back; the caller's outputs copied out
static int profile_thorough(epa_ctx* ctx, const ProfileCall& c, uint32_t stride, const epa_pair* d_pairs, uint64_t n, epa_pair* pairs_out,
                            epa_result* d_res, epa_result* res_out, epa_thorough_stats* stats) {
  unsigned long long* d_stats = (unsigned long long*)epa_scratch(ctx, SLOT_STATS, 256);
  if (!d_stats) return epa_fail(ctx, EPA_ERR_HIP, "hipMalloc(thorough statistics)");
  int rc = epa_zero_async(ctx, d_stats, 128);
  if (rc) return rc;
  rc = launch_thorough_generic(ctx, d_pairs, n, nullptr, c.d_begin, c.d_span, c.max_span, d_res, d_stats, nullptr, false, c.d_qe, stride);
  if (rc) return rc;
  unsigned long long hst[16];
  if (pairs_out) EPA_HIP(ctx, hipMemcpyAsync(pairs_out, d_pairs, sizeof(epa_pair) * n, hipMemcpyDeviceToHost, ctx->stream));
  if (res_out) EPA_HIP(ctx, hipMemcpyAsync(res_out, d_res, sizeof(epa_result) * n, hipMemcpyDeviceToHost, ctx->stream));
  EPA_HIP(ctx, hipMemcpyAsync(hst, d_stats, 128, hipMemcpyDeviceToHost, ctx->stream));
  EPA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return chunk_stats(ctx, n, hst, stats);
}

extern "C" int epa_dev_thorough_profile(epa_ctx* ctx, const epa_pair* pairs, uint64_t n_pairs, const double* prof, uint32_t stride,
                                        const uint32_t* win_begin, const uint32_t* win_span, uint32_t Q, epa_result* out,
                                        epa_thorough_stats* stats) {
  if (!ctx || !prof || !win_begin || !win_span || (n_pairs && (!pairs || !out))) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "null argument");
  if (stats) memset(stats, 0, sizeof(*stats));
  if (n_pairs == 0) return EPA_OK;
  EPA_HIP(ctx, hipSetDevice(ctx->device));
  ProfileCall c;
  int rc = c.stage(ctx, "thorough_profile", prof, stride, win_begin, win_span, Q);
  if (rc) return rc;
  if (!epa_is_device_ptr(pairs))
    for (uint64_t i = 0; i < n_pairs; ++i)
      if (pairs[i].branch_id >= ctx->B || pairs[i].seq_id >= Q) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "pair index out of range");
  const epa_pair* d_pairs = (const epa_pair*)epa_to_device(ctx, SLOT_PAIRS, pairs, sizeof(epa_pair) * n_pairs);
  const bool out_dev = epa_is_device_ptr(out);
  epa_result* d_out = out_dev ? out : (epa_result*)epa_scratch(ctx, SLOT_RESULTS, sizeof(epa_result) * n_pairs);
  if (!d_pairs || !d_out) return epa_fail(ctx, EPA_ERR_HIP, "thorough_profile: staging failed");
  return profile_thorough(ctx, c, stride, d_pairs, n_pairs, nullptr, d_out, out_dev ? nullptr : out, stats);
}

// ---- chunk body: preplace_profile -> the context's candidate selection -> thorough_profile, the table stays in HBM

extern "C" int epa_dev_place_chunk_profile(epa_ctx* ctx, const double* prof, uint32_t stride, const uint32_t* win_begin,
                                           const uint32_t* win_span, uint32_t Q, double threshold, epa_pair* pairs,
                                           epa_result* results, uint64_t max_pairs, uint64_t* n_pairs, epa_thorough_stats* stats) {
  if (!ctx || !prof || !win_begin || !win_span || !pairs || !results || !n_pairs) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "null argument");
  *n_pairs = 0;
  if (stats) memset(stats, 0, sizeof(*stats));
  if (Q == 0) return EPA_OK;
  EPA_HIP(ctx, hipSetDevice(ctx->device));
  int rc = profile_needs_resident(ctx, "place_chunk_profile");
  if (!rc) rc = profile_table(ctx);
  if (rc) return rc;
  ProfileCall c;
  rc = c.stage(ctx, "place_chunk_profile", prof, stride, win_begin, win_span, Q);
  if (rc) return rc;
  const bool pairs_dev = epa_is_device_ptr(pairs), res_dev = epa_is_device_ptr(results);
  double* d_tab = (double*)epa_scratch(ctx, SLOT_TABLE, sizeof(double) * (size_t)Q * ctx->B);
  epa_pair* d_pairs = pairs_dev ? pairs : (epa_pair*)epa_scratch(ctx, SLOT_PAIRS, sizeof(epa_pair) * max_pairs);
  epa_result* d_res = res_dev ? results : (epa_result*)epa_scratch(ctx, SLOT_RESULTS, sizeof(epa_result) * max_pairs);
  if (!d_tab || !d_pairs || !d_res) return epa_fail(ctx, EPA_ERR_HIP, "hipMalloc(chunk buffers)");
  rc = launch_preplace_profile(ctx, c, stride, Q, d_tab, ctx->B);
  if (rc) return rc;
  // (the windows were checked on the host: the selection has no status words of a preplacement to look at)
  uint64_t n = 0;
  rc = launch_select(ctx, PreTable{d_tab, ctx->B}, nullptr, Q, threshold, d_pairs, max_pairs, &n);
  if (rc) return rc;   // EPA_ERR_PAIR_OVERFLOW: nothing is kept between calls, the caller comes again with room
  *n_pairs = n;
  if (n == 0) return EPA_OK;
  return profile_thorough(ctx, c, stride, d_pairs, n, pairs_dev ? nullptr : pairs, d_res, res_dev ? nullptr : results, stats);
}

// ---- host only: rows from column codes and Phred scores

extern "C" int epa_profile_from_phred(uint32_t states, uint32_t Q, uint32_t stride, const uint8_t* codes, const uint8_t* phred,
                                      const uint32_t* win_span, double* prof) {
  if ((states != 4 && states != 20) || !codes || !phred || !win_span || !prof)
    return epa_fail(nullptr, EPA_ERR_INVALID_ARG, "profile_from_phred: null argument or states other than 4 / 20");
  const int S = (int)states, ncols = S == 4 ? 16 : 24;
  const double cap = (double)(S - 1) / (double)S;
  for (uint32_t q = 0; q < Q; ++q) {
    if (win_span[q] > stride)
      return epa_fail(nullptr, EPA_ERR_INVALID_ARG, "profile_from_phred: query " + std::to_string(q) + ": the window is longer than the stride");
    for (uint32_t j = 0; j < win_span[q]; ++j) {
      const size_t at = (size_t)q * stride + j;
      if (codes[at] >= ncols)
        return epa_fail(nullptr, EPA_ERR_INVALID_CHAR, "profile_from_phred: query " + std::to_string(q) + " position " + std::to_string(j) + ": char is invalid!");
      const uint32_t mask = epa_column_mask(S, codes[at]);
      double* v = prof + at * S;
      if (mask & (mask - 1)) {   // ambiguity code or gap: its state set, whatever the score
        for (int m = 0; m < S; ++m) v[m] = (mask >> m) & 1u ? 1.0 : 0.0;
        continue;
      }
      if (phred[at] > 93)
        return epa_fail(nullptr, EPA_ERR_INVALID_ARG, "profile_from_phred: query " + std::to_string(q) + " position " + std::to_string(j) +
                                                          ": Phred score " + std::to_string(phred[at]) + " is above 93");
      const double eps = std::min(pow(10.0, -(double)phred[at] / 10.0), cap);
      for (int m = 0; m < S; ++m) v[m] = (mask >> m) & 1u ? 1.0 - eps : eps / (double)(S - 1);
    }
  }
  return EPA_OK;
}
