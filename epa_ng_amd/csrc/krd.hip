// Kantorovich-Rubinstein (earth mover's) distances between placement samples on one reference tree (epa_dev_krd; Evans
// and Matsen, `guppy kr`, `gappa analyze krd`), with the edge and clade masses that squash clustering and edge PCA start
// from.  The quantities are specified in include/epa_dev.h; the rooted view is that of epa_dev_set_topology.
//
// Structure.  Branches are addressed by their pre-order RANK (EpaTopology::rank): the subtree below branch b is the ranks
// [rank, rank + size), so the mass hanging from child(b) is a difference of two prefix values.
//   k_krd_points   one work item per entry: (sample << 32 | rank) and x, the distance from the child end (EDPL's x_i)
//   two stable rocPRIM radix sorts of the entry indices: on x's bits (x >= 0: a double's bits order as an unsigned
//                  integer), then on (sample << 32 | rank) -- a sample's points on one branch end up contiguous, by x
//                  ascending, equal x in entry order
//   k_krd_gather   x and weight in sorted order
//   k_krd_runs     one work item per (sample, rank): where its run starts (a binary search of the sorted keys) and
//                  M_s[r], the run's weights summed one after the other
//   k_krd_scan     one workgroup per sample: P_s[r], the inclusive scan of M_s over the ranks, 256 ranks at a time with
//                  a fixed-shape scan and a carry -- a function of the sample's own row and nothing else
//   k_krd_pairs    THE HOT KERNEL: one workgroup per (pair a < b, tile of KRD_TILE ranks); lanes stride the tile's
//                  ranks, each merges the two samples' points on its branches; a fixed-shape wave and LDS reduction
//   k_krd_finish   one work item per pair: the tile partials added in tile order, stored at [a][b] and [b][a]
//   k_krd_masses   edge_mass and clade_mass, one work item per (sample, branch)
// Tile sizes and reduction shapes are compile-time constants and nothing depends on S, on the grid or on the other
// samples: a pair's value is a function of the tree and the two samples' entries.  Points of the two samples at one x
// are taken TOGETHER (each sample's weights at that x summed in its own order, then one update of f by their
// difference), so that exchanging the roles of a and b negates every f exactly and changes no bit of the result.
// Nothing is fused or reassociated (contraction is off for the whole file); there are no atomics on doubles.
// A branch that carries hundreds of points of one sample is one lane's long loop, as in k_edpl_pairs.
#include "krd_kernels.hpp"

#pragma clang fp contract(off)

extern "C" int epa_dev_krd(epa_ctx* ctx, const epa_pair* pairs, const double* distal, const double* weight, uint64_t n, uint32_t S,
                           double* krd, double* edge_mass, double* clade_mass) {
  if (!ctx) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "null argument");
  if (int rc = krd_validate(ctx, "krd", pairs, distal, weight, n, S)) return rc;
  if (!krd) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "null argument");
  EPA_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = krd_validate_entries(ctx, "krd", pairs, distal, weight, n, S)) return rc;
  const uint32_t n32 = (uint32_t)n, B = ctx->B;
  const size_t SB = (size_t)S * B, out_bytes = sizeof(double) * (size_t)S * S, mass_bytes = sizeof(double) * SB;
  const bool masses = edge_mass || clade_mass;
  const epa_pair* d_pairs = n ? (const epa_pair*)epa_to_device(ctx, SLOT_PAIRS, pairs, sizeof(epa_pair) * n) : nullptr;
  const double* d_distal = n ? (const double*)epa_to_device(ctx, SLOT_DISTAL, distal, sizeof(double) * n) : nullptr;
  const double* d_weight = n ? (const double*)epa_to_device(ctx, SLOT_WEIGHT, weight, sizeof(double) * n) : nullptr;
  if (n && (!d_pairs || !d_distal || !d_weight)) return epa_fail(ctx, EPA_ERR_HIP, "krd input upload failed");
  // outputs: written in place on the device, or staged in SLOT_OUT and copied out
  const bool krd_dev = epa_is_device_ptr(krd), em_dev = edge_mass && epa_is_device_ptr(edge_mass),
             cm_dev = clade_mass && epa_is_device_ptr(clade_mass);
  Carver ov;
  auto out_layout = [&](Carver& c, double*& k, double*& e, double*& m) {
    k = krd_dev ? krd : (double*)c.tail(align256(out_bytes));
    e = !edge_mass ? nullptr : em_dev ? edge_mass : (double*)c.tail(align256(mass_bytes));
    m = !clade_mass ? nullptr : cm_dev ? clade_mass : (double*)c.tail(align256(mass_bytes));
  };
  double *d_krd = nullptr, *d_em = nullptr, *d_cm = nullptr;
  out_layout(ov, d_krd, d_em, d_cm);
  if (ov.off) {
    char* stage = (char*)epa_scratch(ctx, SLOT_OUT, ov.off);
    if (!stage) return epa_fail(ctx, EPA_ERR_HIP, "hipMalloc(krd out)");
    ov = Carver{stage, 0};
    out_layout(ov, d_krd, d_em, d_cm);
  }
  // scratch
  const KrdShape sh = krd_shape(ctx, n32, S, masses, true);
  KrdLay ly;
  Carver cv;
  krd_layout(cv, ly, sh);
  char* base = (char*)epa_scratch(ctx, SLOT_KRD, cv.off);
  if (!base) return epa_fail(ctx, EPA_ERR_HIP, "hipMalloc(krd scratch)");
  cv = Carver{base, 0};
  krd_layout(cv, ly, sh);
  const EpaTopology& tp = *ctx->topo;

  epa_timer_start(ctx, epa_t(ctx, epa_ctx::T_KRD));
  if (int rc = krd_launch(ctx, ly, sh, d_pairs, d_distal, d_weight, d_krd, true)) return rc;
  if (masses)
    hipLaunchKernelGGL(k_krd_masses, dim3((uint32_t)((SB + 255) / 256)), dim3(256), 0, ctx->stream, ly.P, ly.M, tp.rank, tp.size, B, S,
                       d_em, d_cm);
  epa_timer_stop(ctx, epa_t(ctx, epa_ctx::T_KRD));
  EPA_HIP(ctx, hipGetLastError());
  uint32_t status[2] = {0, 0};
  EPA_HIP(ctx, hipMemcpyAsync(status, ly.status, sizeof(status), hipMemcpyDeviceToHost, ctx->stream));
  EPA_HIP(ctx, hipStreamSynchronize(ctx->stream));   // host inputs were staged from pageable memory: the wait in every case
  if (status[ST_BAD_BRANCH]) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "krd: a branch id is out of range");
  if (status[ST_BAD_SAMPLE]) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "krd: a sample id is out of range");
  if (!krd_dev) EPA_HIP(ctx, hipMemcpy(krd, d_krd, out_bytes, hipMemcpyDeviceToHost));
  if (edge_mass && !em_dev) EPA_HIP(ctx, hipMemcpy(edge_mass, d_em, mass_bytes, hipMemcpyDeviceToHost));
  if (clade_mass && !cm_dev) EPA_HIP(ctx, hipMemcpy(clade_mass, d_cm, mass_bytes, hipMemcpyDeviceToHost));
  return EPA_OK;
}
