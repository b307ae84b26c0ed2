// Tree geometry on the device: a topology attached to a context (epa_dev_set_topology), path distances between
// placement points, and the expected distance between placement locations on top of them (epa_dev_edpl; EDPL, Matsen et
// al., `guppy edpl`, `gappa examine edpl`).  The quantities are specified exactly in include/epa_dev.h.
//
// Structure.  The tree is rooted at node_prox[0]; depth[node] is the fp64 sum of the branch lengths down from the root,
// one rounded add per level.  An Euler tour of the rooted tree (2 n_nodes - 1 visits) with a sparse table of range
// minima answers "depth of the lowest common ancestor of u and v" in O(1): lengths are >= 0 and a rounded add of a
// non-negative number never decreases, so every node visited between the first visits of u and v lies at or below their
// LCA in DEPTH as well, and the minimum of the tour's depths over that range is depth[lca] itself -- the table holds the
// depths, not node ids, and a query is two 8-byte loads.  Zero-length branches change nothing: ties are ties of equal
// doubles.  The tour and the table are built on the host with an explicit stack (a ladder of 65 536 levels is an ordinary
// input), uploaded once per set_topology and kept in ONE device allocation:
//   sparse [levels][L] doubles, L = 2 n_nodes - 1, levels = floor(log2 L) + 1    (19.7 MB at 65 537 branches)
//   cdepth [B] doubles   depth[child(b)], child(b) = the end of b farther from the root
//   cinfo  [B] uint32    first Euler index of child(b), bit 31 set where child(b) == node_dist[b]
//   rank   [B] uint32    b's position in the order the walk first reaches the child ends: a pre-order
//   size   [B] uint32    branches in the subtree of child(b), b included: the subtree is the ranks [rank, rank + size)
// (EpaTopology, epa_dev_internal.hpp: krd.hip reads the last four.)
//
// epa_dev_edpl.  The entries are grouped by query with the stable radix sort of their indices that the RELL calls use
// (launch_group_entries, rell.hip: a group keeps the caller's entry order; the run bounds are read on the device), then
//   k_edpl_points  one work item per entry, in grouped order: (D, Euler index of the edge's child, weight)
//   k_edpl_pairs   one work item per entry i: walks the contiguous run of its query's points, j in entry order, and sums
//                  weight_j * d_ij -- ONE launch over all entries, no host loop over queries.  Objects have <= 7 rows as a
//                  rule: neighbouring lanes serve neighbouring queries and a wave stays full; a 1024-row object is a
//                  1024-iteration loop on 1024 work items whose lanes read the same point at the same time
//   k_edpl_sum     one work item per query: weight_i * row_dist_i in entry order
// Nothing is fused or reassociated (contraction is off for the whole file); there are no atomics on doubles.
#include "epa_dev_internal.hpp"

#include <string.h>

#pragma clang fp contract(off)   // every step of the specification is ONE fp64 operation: hipcc contracts by default

void epa_topology_free(epa_ctx* ctx) {
  if (!ctx->topo) return;
  if (ctx->topo->base) (void)hipFree(ctx->topo->base);
  delete ctx->topo;
  ctx->topo = nullptr;
}

namespace {

constexpr uint32_t EDPL_DIST_BIT = 0x80000000u;
// status words of a call (zeroed before the kernels): entries whose ids the kernels refused
enum : int { ST_BAD_BRANCH = 0, ST_BAD_SEQ = 1, ST_WORDS = 64 };

struct TopoView {
  const double* sparse;
  const double* cdepth;
  const uint32_t* cinfo;
  uint32_t L;
};

// the point of sorted position p: D = depth[child(e)] - x, x the distance from the child end
__global__ void __launch_bounds__(256) k_edpl_points(const TopoView t, const epa_pair* __restrict__ pairs,
                                                     const double* __restrict__ distal, const double* __restrict__ weight,
                                                     const double* __restrict__ blen, const uint32_t* __restrict__ order,
                                                     uint32_t n, uint32_t B, double* __restrict__ pD, uint32_t* __restrict__ pE,
                                                     double* __restrict__ pW, uint32_t* __restrict__ status) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const uint32_t e = order[p], b = pairs[e].branch_id;
  if (b >= B) {   // device pairs: nothing is read through the id; the call is refused after the launch
    atomicAdd(&status[ST_BAD_BRANCH], 1u);
    pD[p] = 0.0; pE[p] = 0u; pW[p] = 0.0;
    return;
  }
  const uint32_t info = t.cinfo[b];
  const double dl = distal[e];
  const double x = (info & EDPL_DIST_BIT) ? dl : blen[b] - dl;
  pD[p] = t.cdepth[b] - x;
  pE[p] = info & ~EDPL_DIST_BIT;
  pW[p] = weight[e];
}

// depth[lca] of the nodes first visited at Euler indices a and b: the minimum of the tour's depths over [lo, hi]
__device__ __forceinline__ double edpl_lca_depth(const TopoView& t, uint32_t a, uint32_t b) {
  const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
  const uint32_t k = 31u - (uint32_t)__clz((int)(hi - lo + 1u));
  const double* __restrict__ row = t.sparse + (size_t)k * t.L;
  const double u = row[lo], v = row[hi + 1u - (1u << k)];
  return u < v ? u : v;
}

__global__ void __launch_bounds__(256) k_edpl_pairs(const TopoView t, const uint32_t* __restrict__ sorted,
                                                    const uint32_t* __restrict__ bounds, const uint32_t* __restrict__ order,
                                                    uint32_t n, uint32_t Q, const double* __restrict__ pD,
                                                    const uint32_t* __restrict__ pE, const double* __restrict__ pW,
                                                    double* __restrict__ rowS, double* __restrict__ row_dist,
                                                    uint32_t* __restrict__ status) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const uint32_t q = sorted[p];
  double acc = 0.0;
  if (q >= Q) {   // device pairs: a sequence id that is no query owns no run; the call is refused after the launch
    atomicAdd(&status[ST_BAD_SEQ], 1u);
  } else {
    const uint32_t j0 = bounds[q], j1 = bounds[Q + q];
    const double Di = pD[p];
    const uint32_t Ei = pE[p];
    for (uint32_t j = j0; j < j1; ++j) {
      const double Dj = pD[j];
      double m = edpl_lca_depth(t, Ei, pE[j]);
      m = Di < m ? Di : m;
      m = Dj < m ? Dj : m;
      const double d = (Di - m) + (Dj - m);
      const double term = pW[j] * d;
      acc += term;
    }
  }
  rowS[p] = acc;
  if (row_dist) row_dist[order[p]] = acc;
}

__global__ void __launch_bounds__(256) k_edpl_sum(const uint32_t* __restrict__ bounds, uint32_t Q, const double* __restrict__ pW,
                                                  const double* __restrict__ rowS, double* __restrict__ edpl) {
  const uint32_t q = blockIdx.x * 256 + threadIdx.x;
  if (q >= Q) return;
  const uint32_t j0 = bounds[q], j1 = bounds[Q + q];
  double acc = 0.0;
  for (uint32_t j = j0; j < j1; ++j) {
    const double term = pW[j] * rowS[j];
    acc += term;
  }
  edpl[q] = acc;
}

}  // namespace

extern "C" int epa_dev_set_topology(epa_ctx* ctx, uint32_t n_nodes, const uint32_t* node_prox, const uint32_t* node_dist) {
  if (!ctx || !node_prox || !node_dist) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "null argument");
  const uint32_t B = ctx->B;
  if (B == 0 || (uint64_t)B + 1 != (uint64_t)n_nodes)
    return epa_fail(ctx, EPA_ERR_INVALID_ARG, "set_topology: a tree of " + std::to_string(n_nodes) + " nodes has " +
                                                  std::to_string((uint64_t)n_nodes - (n_nodes ? 1 : 0)) +
                                                  " branches, the context has " + std::to_string(B));
  EPA_HIP(ctx, hipSetDevice(ctx->device));
  std::vector<uint32_t> pbuf, dbuf;
  const uint32_t* prox = host_view(node_prox, B, pbuf, ctx->stream);
  const uint32_t* dist = host_view(node_dist, B, dbuf, ctx->stream);
  if (!prox || !dist) return epa_fail(ctx, EPA_ERR_HIP, "cannot read the node arrays");
  for (uint32_t b = 0; b < B; ++b) {
    for (const uint32_t v : {prox[b], dist[b]})
      if (v >= n_nodes)
        return epa_fail(ctx, EPA_ERR_INVALID_ARG, "set_topology: branch " + std::to_string(b) + ": node id " + std::to_string(v) +
                                                      " is out of range (" + std::to_string(n_nodes) + " nodes)");
    if (prox[b] == dist[b])
      return epa_fail(ctx, EPA_ERR_INVALID_ARG, "set_topology: branch " + std::to_string(b) + ": both ends are node " +
                                                    std::to_string(prox[b]));
    if (!(std::isfinite(ctx->h_blen[b]) && ctx->h_blen[b] >= 0.0))   // depths must not decrease down the tree
      return epa_fail(ctx, EPA_ERR_INVALID_ARG, "set_topology: branch " + std::to_string(b) + ": its length is negative or not finite");
  }
  // adjacency: the branches at every node
  std::vector<uint32_t> off((size_t)n_nodes + 1, 0), adj(2 * (size_t)B);
  for (uint32_t b = 0; b < B; ++b) { ++off[prox[b] + 1]; ++off[dist[b] + 1]; }
  for (uint32_t v = 0; v < n_nodes; ++v) off[v + 1] += off[v];
  {
    std::vector<uint32_t> fill(off.begin(), off.end() - 1);
    for (uint32_t b = 0; b < B; ++b) { adj[fill[prox[b]]++] = b; adj[fill[dist[b]]++] = b; }
  }
  // Euler tour from the root with an explicit stack: depth[child] = depth[parent] + length, one add per level
  const uint32_t root = prox[0], L = 2 * n_nodes - 1, NONE = 0xffffffffu;
  std::vector<double> depth(n_nodes, 0.0), tour;
  std::vector<uint32_t> first(n_nodes, NONE), up(n_nodes, NONE), cur(off.begin(), off.end() - 1), child(B, NONE), stack;
  std::vector<uint32_t> brank(B, 0), bsize(B, 0);   // pre-order position of every branch and the size of its subtree
  tour.reserve(L);
  stack.reserve(n_nodes);
  first[root] = 0;
  tour.push_back(0.0);
  stack.push_back(root);
  uint32_t seen = 1;
  while (!stack.empty()) {
    const uint32_t v = stack.back();
    if (cur[v] < off[v + 1]) {
      const uint32_t b = adj[cur[v]++];
      if (b == up[v]) continue;
      const uint32_t w = prox[b] == v ? dist[b] : prox[b];
      if (first[w] != NONE) continue;   // a second way to w: with n_nodes - 1 branches some node then stays unreached
      depth[w] = depth[v] + ctx->h_blen[b];
      up[w] = b;
      child[b] = w;
      brank[b] = seen - 1;   // the branches reached before this one
      first[w] = (uint32_t)tour.size();
      tour.push_back(depth[w]);
      stack.push_back(w);
      ++seen;
    } else {
      stack.pop_back();
      if (up[v] != NONE) bsize[up[v]] = seen - 1 - brank[up[v]];   // everything reached since, the branch itself included
      if (!stack.empty()) tour.push_back(depth[stack.back()]);
    }
  }
  if (seen != n_nodes) {
    for (uint32_t b = 0; b < B; ++b)
      if (first[prox[b]] == NONE || first[dist[b]] == NONE)
        return epa_fail(ctx, EPA_ERR_INVALID_ARG, "set_topology: the graph is not connected: branch " + std::to_string(b) +
                                                      " cannot be reached from node " + std::to_string(root) + ", the root");
    for (uint32_t v = 0; v < n_nodes; ++v)   // every branch is reached: a node that no branch names
      if (first[v] == NONE)
        return epa_fail(ctx, EPA_ERR_INVALID_ARG, "set_topology: the graph is not connected: node " + std::to_string(v) +
                                                      " is an end of no branch");
  }
  // sparse table of range minima over the tour's depths, and the per-branch records
  uint32_t levels = 1;
  while ((2u << (levels - 1)) <= L) ++levels;
  Carver cv;
  auto layout = [&](Carver& c, double*& sp, double*& cd, uint32_t*& ci, uint32_t*& rk, uint32_t*& sz) {
    sp = c.take<double>((size_t)levels * L);
    cd = c.take<double>(B);
    ci = c.take<uint32_t>(B);
    rk = c.take<uint32_t>(B);
    sz = c.take<uint32_t>(B);
  };
  double *sp = nullptr, *cd = nullptr;
  uint32_t *ci = nullptr, *rk = nullptr, *sz = nullptr;
  layout(cv, sp, cd, ci, rk, sz);
  const size_t bytes = cv.off;
  std::vector<char> host(bytes, 0);
  cv = Carver{host.data(), 0};
  layout(cv, sp, cd, ci, rk, sz);
  memcpy(sp, tour.data(), sizeof(double) * L);
  for (uint32_t k = 1; k < levels; ++k) {
    const double* lo = sp + (size_t)(k - 1) * L;
    double* hi = sp + (size_t)k * L;
    const uint32_t half = 1u << (k - 1);
    for (uint32_t i = 0; i + 2 * half <= L; ++i) hi[i] = std::min(lo[i], lo[i + half]);
  }
  for (uint32_t b = 0; b < B; ++b) {
    cd[b] = depth[child[b]];
    ci[b] = first[child[b]] | (child[b] == dist[b] ? EDPL_DIST_BIT : 0u);
    rk[b] = brank[b];
    sz[b] = bsize[b];
  }
  void* d_base = nullptr;
  EPA_HIP(ctx, hipMalloc(&d_base, bytes));
  if (hipMemcpy(d_base, host.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(d_base);
    return epa_fail(ctx, EPA_ERR_HIP, "set_topology: upload failed");
  }
  // the new topology replaces the old one only now: a refused call leaves the context as it was
  EPA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  epa_topology_free(ctx);
  EpaTopology* t = new EpaTopology;
  t->n_nodes = n_nodes;
  t->L = L;
  t->levels = levels;
  t->base = d_base;
  cv = Carver{(char*)d_base, 0};
  layout(cv, sp, cd, ci, rk, sz);
  t->sparse = sp;
  t->cdepth = cd;
  t->cinfo = ci;
  t->rank = rk;
  t->size = sz;
  ctx->topo = t;
  return EPA_OK;
}

extern "C" int epa_dev_edpl(epa_ctx* ctx, const epa_pair* pairs, const double* distal, const double* weight, uint64_t n,
                            uint32_t Q, double* row_dist, double* edpl) {
  if (!ctx || (Q && !edpl) || (n && (!pairs || !distal || !weight))) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "null argument");
  if (!ctx->topo)
    return epa_fail(ctx, EPA_ERR_INVALID_ARG, "edpl: no topology is set for this context: call epa_dev_set_topology first");
  if (n > 0xffffffffull) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "edpl: more than 2^32 - 1 entries in one call");
  EPA_HIP(ctx, hipSetDevice(ctx->device));
  const bool edpl_dev = edpl && epa_is_device_ptr(edpl);
  if (n == 0 || Q == 0) {
    if (n) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "edpl: entry 0: sequence id out of range");
    if (!Q) return EPA_OK;
    if (edpl_dev) {
      EPA_HIP(ctx, hipMemsetAsync(edpl, 0, sizeof(double) * Q, ctx->stream));
      EPA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    } else {
      memset(edpl, 0, sizeof(double) * Q);
    }
    return EPA_OK;
  }
  // host arrays are validated (device arrays are the caller's responsibility; ids are checked by the kernels)
  const bool hp = !epa_is_device_ptr(pairs), hd = !epa_is_device_ptr(distal), hw = !epa_is_device_ptr(weight);
  auto bad = [&](uint64_t i, const char* what) {
    return epa_fail(ctx, EPA_ERR_INVALID_ARG, "edpl: entry " + std::to_string(i) + ": " + what);
  };
  for (uint64_t i = 0; i < n; ++i) {
    if (hp && pairs[i].branch_id >= ctx->B) return bad(i, "branch id out of range");
    if (hp && pairs[i].seq_id >= Q) return bad(i, "sequence id out of range");
    if (hd && !(std::isfinite(distal[i]) && distal[i] >= 0.0)) return bad(i, "distal length is negative or not finite");
    if (hp && hd && distal[i] > ctx->h_blen[pairs[i].branch_id]) return bad(i, "distal length beyond the branch's length");
    if (hw && !(std::isfinite(weight[i]) && weight[i] >= 0.0)) return bad(i, "weight is negative or not finite");
  }
  const uint32_t n32 = (uint32_t)n, B = ctx->B;
  const epa_pair* d_pairs = (const epa_pair*)epa_to_device(ctx, SLOT_PAIRS, pairs, sizeof(epa_pair) * n);
  const double* d_distal = (const double*)epa_to_device(ctx, SLOT_DISTAL, distal, sizeof(double) * n);
  const double* d_weight = (const double*)epa_to_device(ctx, SLOT_WEIGHT, weight, sizeof(double) * n);
  if (!d_pairs || !d_distal || !d_weight) return epa_fail(ctx, EPA_ERR_HIP, "edpl input upload failed");
  // outputs: written in place on the device, or staged in SLOT_OUT and copied out
  const bool row_dev = row_dist && epa_is_device_ptr(row_dist);
  const size_t row_bytes = align256(sizeof(double) * n), q_bytes = sizeof(double) * (size_t)Q;
  const size_t staged = (row_dist && !row_dev ? row_bytes : 0) + (edpl_dev ? 0 : q_bytes);
  char* d_stage = staged ? (char*)epa_scratch(ctx, SLOT_OUT, staged) : nullptr;
  if (staged && !d_stage) return epa_fail(ctx, EPA_ERR_HIP, "hipMalloc(edpl out)");
  double* d_row = !row_dist ? nullptr : row_dev ? row_dist : (double*)d_stage;
  double* d_edpl = edpl_dev ? edpl : (double*)(d_stage + (row_dist && !row_dev ? row_bytes : 0));
  // scratch: the points and the per-entry sums; the grouping is the RELL calls' (never live at the same time)
  Carver cv;
  cv.tail(sizeof(uint32_t) * ST_WORDS);
  cv.take<double>(n); cv.take<double>(n); cv.take<double>(n); cv.take<uint32_t>(n);
  char* pts = (char*)epa_scratch(ctx, SLOT_EDPL, cv.off);
  if (!pts) return epa_fail(ctx, EPA_ERR_HIP, "hipMalloc(edpl scratch)");
  cv = Carver{pts, 0};
  uint32_t* d_status = (uint32_t*)cv.tail(sizeof(uint32_t) * ST_WORDS);
  double *pD = cv.take<double>(n), *pW = cv.take<double>(n), *rowS = cv.take<double>(n);
  uint32_t* pE = cv.take<uint32_t>(n);
  const EpaTopology& tp = *ctx->topo;
  const TopoView tv{tp.sparse, tp.cdepth, tp.cinfo, tp.L};
  const dim3 ngrid((n32 + 255) / 256), qgrid((Q + 255) / 256);

  epa_timer_start(ctx, epa_t(ctx, epa_ctx::T_EDPL));
  EPA_HIP(ctx, hipMemsetAsync(d_status, 0, sizeof(uint32_t) * ST_WORDS, ctx->stream));
  EntryGroups eg;
  const int grc = launch_group_entries(ctx, d_pairs, n32, Q, 0, &eg);
  if (grc) return grc;
  hipLaunchKernelGGL(k_edpl_points, ngrid, dim3(256), 0, ctx->stream, tv, d_pairs, d_distal, d_weight, ctx->blen, eg.order, n32, B,
                     pD, pE, pW, d_status);
  hipLaunchKernelGGL(k_edpl_pairs, ngrid, dim3(256), 0, ctx->stream, tv, eg.sorted, eg.bounds, eg.order, n32, Q, pD, pE, pW, rowS,
                     d_row, d_status);
  hipLaunchKernelGGL(k_edpl_sum, qgrid, dim3(256), 0, ctx->stream, eg.bounds, Q, pW, rowS, d_edpl);
  epa_timer_stop(ctx, epa_t(ctx, epa_ctx::T_EDPL));
  EPA_HIP(ctx, hipGetLastError());
  uint32_t status[2] = {0, 0};
  EPA_HIP(ctx, hipMemcpyAsync(status, d_status, sizeof(status), hipMemcpyDeviceToHost, ctx->stream));
  EPA_HIP(ctx, hipStreamSynchronize(ctx->stream));   // host inputs were staged from pageable memory: the wait in every case
  if (status[ST_BAD_BRANCH]) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "edpl: a branch id is out of range");
  if (status[ST_BAD_SEQ]) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "edpl: a sequence id is out of range");
  if (row_dist && !row_dev) EPA_HIP(ctx, hipMemcpy(row_dist, d_row, sizeof(double) * n, hipMemcpyDeviceToHost));
  if (!edpl_dev) EPA_HIP(ctx, hipMemcpy(edpl, d_edpl, q_bytes, hipMemcpyDeviceToHost));
  return EPA_OK;
}
