// Edge principal components of placement samples (epa_dev_epca; Matsen and Evans 2013, `guppy epca`, `gappa analyze
// edgepca`): per sample and inner edge the imbalance of the sample's mass across the edge, and the principal components
// of the centred [S][B] imbalance matrix.  The quantities are specified in include/epa_dev.h; M, P, rank and size are
// those of epa_dev_krd, from its own kernels (the table phase of krd_launch, krd_kernels.hpp).
//
// The B x B covariance matrix is never formed: G = Xc Xc^T, [S][S], has the same non-zero spectrum, and its eigenvectors
// u give the edge vectors as Xc^T u / sqrt(lambda').
//   k_epca_imbalance    one work item per (branch, sample): X from P, M, rank and size into XT [rank][sample] (edge-major,
//                       pitch S rounded up to 16; excluded ranks and pad columns are 0.0), and the optional imbalance[s][b]
//   k_epca_centre       one work item per rank: the mean over the samples, added one after the other, and Xc in place
//   k_epca_gram         THE HOT KERNEL for large trees: one wave per (pair of 16-sample tiles I <= J, slice of 1024
//                       ranks): v_mfma_f64_16x16x4_f64 over the slice, four ranks per instruction, both operands one
//                       128-byte row segment of XT per quarter-wave; one 16 x 16 partial per (tile pair, slice)
//   k_epca_gram_finish  one work item per element of a tile pair: the partials added in slice order, stored at [a][b] and
//                       [b][a] (diagonal tiles: the upper triangle's elements only), bit-symmetric by construction
//   k_epca_gram_out     the diagonal as first computed (total_var) and, when asked for, the matrix for the caller
//   per Jacobi sweep:   k_epca_sweep_begin  the threshold 2^-53 max |a_ii| (one workgroup, a fixed-shape maximum)
//     per step:         k_epca_rot          one work item per pair of the step: (c, s, t), or the identity where the
//                                           threshold skips the pair or the dummy index is involved; counts rotations
//                       k_epca_apply        one work item per (pair i <= pair j): its 2 x 2 block J_i^T . block . J_j, stored
//                                           with its mirror image; item (i, i) writes a_pq = a_qp = 0.0; item (i, j) also
//                                           rotates columns p_i, q_i of rows 2 j, 2 j + 1 of V.  In place: the blocks of a
//                                           step are disjoint
//     (the host reads the sweep's rotation count: 4 bytes, the one read-back of the sweep)
//   k_epca_vecs         one work item per (component, branch): the sum over the samples in ascending order / sqrt(lambda')
//   k_epca_sign         one workgroup per component: a fixed-shape arg-max of |value| (lowest branch id on ties), the sign
//                       applied in place
//   k_epca_proj         one work item per (sample, component)
// The host drives the loop and the matrices stay resident, as in squash.hip; there is no grid-wide barrier anywhere.
// Tile shapes and the slice length are compile-time constants; nothing depends on the grid.  The only atomic is the
// integer rotation count.  Contraction is off for the whole file (the matrix instruction is an FMA by itself).
#include "krd_kernels.hpp"

#include <string.h>

#include <chrono>

#pragma clang fp contract(off)

namespace {

constexpr uint32_t EPCA_MAX_S = 1024;
constexpr uint32_t EPCA_MAX_SWEEPS = 30;
constexpr uint32_t EPCA_SLICE = 1024;                    // ranks per wave of k_epca_gram
constexpr size_t EPCA_PART_BUDGET = (size_t)64 << 20;   // bytes of Gram partials per launch

typedef double epca_d4 __attribute__((ext_vector_type(4)));

// a rotation of one step: c, s, t = s / c, and whether it is one at all
struct EpcaRot {
  double c, s, t;
  uint32_t on, pad;
};

// a component as the host chose it from the sorted Gram eigenvalues
struct EpcaComp {
  double lam;      // lambda'_k
  uint32_t col;    // its Jacobi column
  uint32_t null;   // 1: edge_vec and proj are 0.0
};

// tile pair q (rows of I one after the other, I <= J) of nt tiles
__device__ __forceinline__ void epca_tiles_of(uint32_t q, uint32_t nt, uint32_t& I, uint32_t& J) {
  uint32_t i = 0;
  while (q >= nt - i) { q -= nt - i; ++i; }
  I = i;
  J = i + q;
}

__global__ void __launch_bounds__(256) k_epca_imbalance(const double* __restrict__ P, const double* __restrict__ M,
                                                        const uint32_t* __restrict__ rank, const uint32_t* __restrict__ size,
                                                        uint32_t B, uint32_t S, uint32_t Sp, double* __restrict__ XT,
                                                        double* __restrict__ imbalance) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= (size_t)B * Sp) return;
  const uint32_t b = (uint32_t)(g / Sp), s = (uint32_t)(g - (size_t)b * Sp);
  const uint32_t r = rank[b], sz = size[b];
  double x = 0.0;
  if (s < S && sz != 1 && sz != B) {
    const double* __restrict__ Ps = P + (size_t)s * B;
    const double T = Ps[r + sz - 1] - Ps[r];
    const double W = Ps[B - 1];
    const double rootside = (W - T) - M[(size_t)s * B + r];
    x = T - rootside;
  }
  XT[(size_t)r * Sp + s] = x;
  if (imbalance && s < S) imbalance[(size_t)s * B + b] = x;
}

__global__ void __launch_bounds__(256) k_epca_centre(double* __restrict__ XT, uint32_t B, uint32_t S, uint32_t Sp) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r >= B) return;
  double* __restrict__ row = XT + (size_t)r * Sp;
  double acc = 0.0;
  for (uint32_t s = 0; s < S; ++s) acc += row[s];
  const double mean = acc / (double)S;
  for (uint32_t s = 0; s < S; ++s) row[s] = row[s] - mean;
}

// Operand maps of v_mfma_f64_16x16x4_f64: lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]; result
// register g of lane l is D[row = (l >> 4) + 4 g][col = l & 15] -- NOT the f32 forms' row = 4 (l >> 4) + g.  With
// A[i][k] = XT[k0 + k][16 I + i] and B[k][j] = XT[k0 + k][16 J + j], D[i][j] is the tile's sum over the four ranks
__global__ void __launch_bounds__(64) k_epca_gram(const double* __restrict__ XT, uint32_t B, uint32_t Sp, uint32_t nt,
                                                  uint32_t n_slices, uint32_t q0, double* __restrict__ part) {
  const uint32_t slice = blockIdx.x % n_slices, ql = blockIdx.x / n_slices;
  uint32_t I, J;
  epca_tiles_of(q0 + ql, nt, I, J);
  const uint32_t lane = threadIdx.x, kq = lane >> 4, c = lane & 15;
  const uint32_t r0 = slice * EPCA_SLICE, r1 = min(B, r0 + EPCA_SLICE);
  const double* __restrict__ pa = XT + 16 * (size_t)I + c;
  const double* __restrict__ pb = XT + 16 * (size_t)J + c;
  epca_d4 acc = {0.0, 0.0, 0.0, 0.0};
  for (uint32_t k0 = r0; k0 < r1; k0 += 4) {
    const uint32_t r = k0 + kq;
    const double a = r < r1 ? pa[(size_t)r * Sp] : 0.0;
    const double b = r < r1 ? pb[(size_t)r * Sp] : 0.0;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
  }
  double* __restrict__ out = part + ((size_t)ql * n_slices + slice) * 256;
#pragma unroll
  for (int g = 0; g < 4; ++g) out[(kq + 4 * g) * 16 + c] = acc[g];
}

__global__ void __launch_bounds__(256) k_epca_gram_finish(const double* __restrict__ part, uint32_t nt, uint32_t n_slices, uint32_t q0,
                                                          uint32_t np, uint32_t S, uint32_t m, double* __restrict__ A) {
  const uint32_t ql = blockIdx.x, e = threadIdx.x;
  if (ql >= np) return;
  uint32_t I, J;
  epca_tiles_of(q0 + ql, nt, I, J);
  const uint32_t row = e >> 4, col = e & 15;
  if (I == J && row > col) return;
  const uint32_t i = 16 * I + row, j = 16 * J + col;
  if (i >= S || j >= S) return;
  double acc = 0.0;
  for (uint32_t sl = 0; sl < n_slices; ++sl) acc += part[((size_t)ql * n_slices + sl) * 256 + e];
  A[(size_t)i * m + j] = acc;
  A[(size_t)j * m + i] = acc;
}

__global__ void __launch_bounds__(256) k_epca_gram_out(const double* __restrict__ A, uint32_t S, uint32_t m, double* __restrict__ diag,
                                                       double* __restrict__ gram) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= (size_t)S * S) return;
  const uint32_t i = (uint32_t)(g / S), j = (uint32_t)(g - (size_t)i * S);
  const double v = A[(size_t)i * m + j];
  if (gram) gram[g] = v;
  if (i == j) diag[i] = v;
}

__global__ void __launch_bounds__(256) k_epca_identity(double* __restrict__ V, uint32_t m) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= (size_t)m * m) return;
  V[g] = g / m == g % m ? 1.0 : 0.0;
}

// thr = 2^-53 max_i |a_ii|: a maximum does not depend on the order it is taken in
__global__ void __launch_bounds__(256) k_epca_sweep_begin(const double* __restrict__ A, uint32_t S, uint32_t m, double* __restrict__ thr) {
  __shared__ double wave_max[4];
  double v = 0.0;
  for (uint32_t i = threadIdx.x; i < S; i += 256) v = fmax(v, fabs(A[(size_t)i * m + i]));
  for (int k = 32; k >= 1; k >>= 1) v = fmax(v, __shfl_xor(v, k, 64));
  if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) *thr = 0x1p-53 * fmax(fmax(wave_max[0], wave_max[1]), fmax(wave_max[2], wave_max[3]));
}

__global__ void __launch_bounds__(256) k_epca_rot(const double* __restrict__ A, uint32_t S, uint32_t m, const uint2* __restrict__ pairs,
                                                  uint32_t h, const double* __restrict__ thr, EpcaRot* __restrict__ rot,
                                                  uint32_t* __restrict__ count) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= h) return;
  const uint32_t p = pairs[i].x, q = pairs[i].y;   // p < q; q >= S: the dummy index
  EpcaRot r{1.0, 0.0, 0.0, 0u, 0u};
  if (q < S) {
    const double apq = A[(size_t)p * m + q];
    if (fabs(apq) > *thr) {
      const double theta = (A[(size_t)q * m + q] - A[(size_t)p * m + p]) / (2.0 * apq);
      const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
      const double c = 1.0 / sqrt(t * t + 1.0);
      r.c = c;
      r.s = t * c;
      r.t = t;
      r.on = 1u;
      atomicAdd(count, 1u);
    }
  }
  rot[i] = r;
}

__global__ void __launch_bounds__(256) k_epca_apply(double* __restrict__ A, double* __restrict__ V, uint32_t m,
                                                    const uint2* __restrict__ pairs, uint32_t h, const EpcaRot* __restrict__ rot) {
  const uint32_t i = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
  if (j >= h) return;
  const EpcaRot ri = rot[i];
  const uint32_t pi = pairs[i].x, qi = pairs[i].y;
  if (ri.on) {
    for (uint32_t k = 2 * j; k < 2 * j + 2; ++k) {   // 2 j + 1 < m: m is even
      double* __restrict__ row = V + (size_t)k * m;
      const double vp = row[pi], vq = row[qi];
      const double cp = ri.c * vp, sq = ri.s * vq, sp = ri.s * vp, cq = ri.c * vq;
      row[pi] = cp - sq;
      row[qi] = sp + cq;
    }
  }
  if (j < i) return;
  if (i == j) {
    if (!ri.on) return;
    const double apq = A[(size_t)pi * m + qi];
    const double d = ri.t * apq;
    A[(size_t)pi * m + pi] = A[(size_t)pi * m + pi] - d;
    A[(size_t)qi * m + qi] = A[(size_t)qi * m + qi] + d;
    A[(size_t)pi * m + qi] = 0.0;
    A[(size_t)qi * m + pi] = 0.0;
    return;
  }
  const EpcaRot rj = rot[j];
  if (!ri.on && !rj.on) return;
  const uint32_t pj = pairs[j].x, qj = pairs[j].y;
  double b00 = A[(size_t)pi * m + pj], b01 = A[(size_t)pi * m + qj], b10 = A[(size_t)qi * m + pj], b11 = A[(size_t)qi * m + qj];
  if (rj.on) {   // columns p_j, q_j
    const double n00 = rj.c * b00 - rj.s * b01, n01 = rj.s * b00 + rj.c * b01;
    const double n10 = rj.c * b10 - rj.s * b11, n11 = rj.s * b10 + rj.c * b11;
    b00 = n00; b01 = n01; b10 = n10; b11 = n11;
  }
  if (ri.on) {   // rows p_i, q_i
    const double n00 = ri.c * b00 - ri.s * b10, n10 = ri.s * b00 + ri.c * b10;
    const double n01 = ri.c * b01 - ri.s * b11, n11 = ri.s * b01 + ri.c * b11;
    b00 = n00; b01 = n01; b10 = n10; b11 = n11;
  }
  A[(size_t)pi * m + pj] = b00; A[(size_t)pj * m + pi] = b00;
  A[(size_t)pi * m + qj] = b01; A[(size_t)qj * m + pi] = b01;
  A[(size_t)qi * m + pj] = b10; A[(size_t)pj * m + qi] = b10;
  A[(size_t)qi * m + qj] = b11; A[(size_t)qj * m + qi] = b11;
}

__global__ void __launch_bounds__(256) k_epca_diag(const double* __restrict__ A, uint32_t S, uint32_t m, double* __restrict__ diag) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < S) diag[i] = A[(size_t)i * m + i];
}

__global__ void __launch_bounds__(256) k_epca_vecs(const double* __restrict__ XT, uint32_t Sp, const double* __restrict__ V, uint32_t m,
                                                   uint32_t S, const uint32_t* __restrict__ rank, const uint32_t* __restrict__ size,
                                                   uint32_t B, const EpcaComp* __restrict__ comp, double* __restrict__ ev) {
  const uint32_t b = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
  if (b >= B) return;
  const EpcaComp cp = comp[k];
  const uint32_t sz = size[b];
  double v = 0.0;
  if (!cp.null && sz != 1 && sz != B) {
    const double* __restrict__ row = XT + (size_t)rank[b] * Sp;
    const double* __restrict__ u = V + cp.col;
    double acc = 0.0;
    for (uint32_t s = 0; s < S; ++s) {
      const double term = row[s] * u[(size_t)s * m];
      acc += term;
    }
    v = acc / sqrt(cp.lam);
  }
  ev[(size_t)k * B + b] = v;
}

// the entry with the largest |value| becomes positive; on equal |value| the lowest branch id decides.  Fixed shape: a
// strided pass, a butterfly within the wave, the four waves in order
__global__ void __launch_bounds__(256) k_epca_sign(double* __restrict__ ev, uint32_t B, double* __restrict__ sigma) {
  __shared__ double wave_a[4];
  __shared__ uint32_t wave_b[4];
  __shared__ double sg_all;
  double* __restrict__ row = ev + (size_t)blockIdx.x * B;
  double a = -1.0;
  uint32_t at = 0xffffffffu;
  auto take = [&](double xa, uint32_t xb) {
    if (xa > a || (xa == a && xb < at)) { a = xa; at = xb; }
  };
  for (uint32_t b = threadIdx.x; b < B; b += 256) take(fabs(row[b]), b);
  for (int k = 32; k >= 1; k >>= 1) {
    const double oa = __shfl_xor(a, k, 64);
    const uint32_t ob = __shfl_xor(at, k, 64);
    take(oa, ob);
  }
  if ((threadIdx.x & 63) == 0) { wave_a[threadIdx.x >> 6] = a; wave_b[threadIdx.x >> 6] = at; }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = wave_a[0]; at = wave_b[0];
    for (int w = 1; w < 4; ++w) take(wave_a[w], wave_b[w]);
    const double sg = at < B && row[at] < 0.0 ? -1.0 : 1.0;
    sg_all = sg;
    sigma[blockIdx.x] = sg;
  }
  __syncthreads();
  if (sg_all < 0.0)
    for (uint32_t b = threadIdx.x; b < B; b += 256) {
      const double x = row[b];
      row[b] = x == 0.0 ? 0.0 : -x;
    }
}

__global__ void __launch_bounds__(256) k_epca_proj(const double* __restrict__ V, uint32_t m, uint32_t S, uint32_t K,
                                                   const EpcaComp* __restrict__ comp, const double* __restrict__ sigma,
                                                   double* __restrict__ proj) {
  const uint32_t g = blockIdx.x * 256 + threadIdx.x;
  if (g >= S * K) return;
  const uint32_t s = g / K, k = g - s * K;
  const EpcaComp cp = comp[k];
  double v = 0.0;
  if (!cp.null) {
    const double scale = sigma[k] * sqrt(cp.lam);
    v = scale * V[(size_t)s * m + cp.col];
  }
  proj[g] = v;
}

struct EpcaLay {
  double *XT, *A, *V, *thr, *part, *diag, *sigma, *ev, *proj, *gram, *imb;
  uint2* pairs;
  EpcaRot* rot;
  uint32_t* count;
  EpcaComp* comp;
};
struct EpcaShape {
  uint32_t B, S, K, Sp, m, h, nt, n_slices, n_tp, per_launch;
  bool gram, imb;
};

void epca_layout(Carver& c, EpcaLay& l, const EpcaShape& sh) {
  l.XT = c.take<double>((size_t)sh.B * sh.Sp);
  l.A = c.take<double>((size_t)sh.m * sh.m);
  l.V = c.take<double>((size_t)sh.m * sh.m);
  l.pairs = c.take<uint2>((size_t)(sh.m - 1) * sh.h);
  l.rot = c.take<EpcaRot>(sh.h);
  l.thr = c.take<double>(1);
  l.count = c.take<uint32_t>(EPCA_MAX_SWEEPS);
  l.part = c.take<double>((size_t)sh.per_launch * sh.n_slices * 256);
  l.diag = c.take<double>(sh.S);
  l.comp = c.take<EpcaComp>(sh.K);
  l.sigma = c.take<double>(sh.K);
  l.ev = c.take<double>((size_t)sh.K * sh.B);
  l.proj = c.take<double>((size_t)sh.S * sh.K);
  l.gram = sh.gram ? c.take<double>((size_t)sh.S * sh.S) : nullptr;
  l.imb = sh.imb ? c.take<double>((size_t)sh.S * sh.B) : nullptr;
}

}  // namespace

extern "C" int epa_dev_epca(epa_ctx* ctx, const epa_pair* pairs, const double* distal, const double* weight, uint64_t n, uint32_t S,
                            uint32_t K, double* eigenvalue, double* edge_vec, double* proj, double* total_var, uint32_t* sweeps,
                            double* imbalance, double* gram) {
  if (!ctx) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "null argument");
  if (ctx->topo && (S < 2 || S > EPCA_MAX_S))
    return epa_fail(ctx, EPA_ERR_INVALID_ARG, "epca: " + std::to_string(S) + " samples: one call takes 2 .. " + std::to_string(EPCA_MAX_S));
  if (int rc = krd_validate(ctx, "epca", pairs, distal, weight, n, S)) return rc;
  if (K < 1 || K >= S)
    return epa_fail(ctx, EPA_ERR_INVALID_ARG, "epca: " + std::to_string(K) + " components: " + std::to_string(S) + " samples have 1 .. " +
                                                  std::to_string(S - 1));
  if (!eigenvalue || !edge_vec || !proj || !total_var || !sweeps) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "null argument");
  EPA_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = krd_validate_entries(ctx, "epca", pairs, distal, weight, n, S)) return rc;
  const uint32_t n32 = (uint32_t)n, B = ctx->B;
  const epa_pair* d_pairs = n ? (const epa_pair*)epa_to_device(ctx, SLOT_PAIRS, pairs, sizeof(epa_pair) * n) : nullptr;
  const double* d_distal = n ? (const double*)epa_to_device(ctx, SLOT_DISTAL, distal, sizeof(double) * n) : nullptr;
  const double* d_weight = n ? (const double*)epa_to_device(ctx, SLOT_WEIGHT, weight, sizeof(double) * n) : nullptr;
  if (n && (!d_pairs || !d_distal || !d_weight)) return epa_fail(ctx, EPA_ERR_HIP, "epca input upload failed");

  // scratch: this call's state, then epa_dev_krd's layout with M
  EpcaShape es{};
  es.B = B; es.S = S; es.K = K;
  es.Sp = (S + 15) & ~15u;
  es.m = S + (S & 1);
  es.h = es.m / 2;
  es.nt = es.Sp / 16;
  es.n_slices = (B + EPCA_SLICE - 1) / EPCA_SLICE;
  es.n_tp = es.nt * (es.nt + 1) / 2;
  es.per_launch = (uint32_t)std::max<size_t>(1, std::min<size_t>(es.n_tp, EPCA_PART_BUDGET / (sizeof(double) * 256 * es.n_slices)));
  es.gram = gram != nullptr;
  es.imb = imbalance != nullptr;
  const KrdShape sh = krd_shape(ctx, n32, S, true, true);
  EpcaLay el;
  KrdLay ly;
  Carver cv;
  epca_layout(cv, el, es);
  krd_layout(cv, ly, sh);
  char* base = (char*)epa_scratch(ctx, SLOT_EPCA, cv.off);
  if (!base) return epa_fail(ctx, EPA_ERR_HIP, "hipMalloc(epca scratch)");
  cv = Carver{base, 0};
  epca_layout(cv, el, es);
  krd_layout(cv, ly, sh);
  const EpaTopology& tp = *ctx->topo;
  const uint32_t Sp = es.Sp, m = es.m, h = es.h;
  const dim3 blk(256);
  const int bank = ctx->bank;
  for (double& v : ctx->epca_ms) v = -1.0;

  // the circle method's pairs of every step: position i meets position m - 1 - i, then the list turns about its head
  std::vector<uint2> h_pairs((size_t)(m - 1) * h);
  {
    std::vector<uint32_t> idx(m), nxt(m);
    for (uint32_t i = 0; i < m; ++i) idx[i] = i;
    for (uint32_t step = 0; step + 1 < m; ++step) {
      for (uint32_t i = 0; i < h; ++i) {
        const uint32_t a = idx[i], b = idx[m - 1 - i];
        h_pairs[(size_t)step * h + i] = make_uint2(std::min(a, b), std::max(a, b));
      }
      nxt[0] = idx[0];
      nxt[1] = idx[m - 1];
      for (uint32_t i = 1; i + 1 < m; ++i) nxt[i + 1] = idx[i];
      idx.swap(nxt);
    }
  }

  epa_timer_start(ctx, epa_t(ctx, epa_ctx::T_EPCA));
  // ---- M and P (epa_dev_krd's table phase), X, Xc
  epa_timer_start(ctx, epa_t(ctx, epa_ctx::T_EPCA_TABLES));
  if (int rc = krd_launch(ctx, ly, sh, d_pairs, d_distal, d_weight, nullptr, false, false)) return rc;
  hipLaunchKernelGGL(k_epca_imbalance, dim3((uint32_t)(((size_t)B * Sp + 255) / 256)), blk, 0, ctx->stream, ly.P, ly.M, tp.rank, tp.size, B,
                     S, Sp, el.XT, el.imb);
  hipLaunchKernelGGL(k_epca_centre, dim3((B + 255) / 256), blk, 0, ctx->stream, el.XT, B, S, Sp);
  epa_timer_stop(ctx, epa_t(ctx, epa_ctx::T_EPCA_TABLES));
  // ---- G
  epa_timer_start(ctx, epa_t(ctx, epa_ctx::T_EPCA_GRAM));
  EPA_HIP(ctx, hipMemsetAsync(el.A, 0, sizeof(double) * (size_t)m * m, ctx->stream));   // the dummy's row and column stay 0.0
  for (uint32_t q0 = 0; q0 < es.n_tp; q0 += es.per_launch) {
    const uint32_t np = std::min(es.per_launch, es.n_tp - q0);
    hipLaunchKernelGGL(k_epca_gram, dim3(np * es.n_slices), dim3(64), 0, ctx->stream, el.XT, B, Sp, es.nt, es.n_slices, q0, el.part);
    hipLaunchKernelGGL(k_epca_gram_finish, dim3(np), blk, 0, ctx->stream, el.part, es.nt, es.n_slices, q0, np, S, m, el.A);
  }
  hipLaunchKernelGGL(k_epca_gram_out, dim3((uint32_t)(((size_t)S * S + 255) / 256)), blk, 0, ctx->stream, el.A, S, m, el.diag, el.gram);
  epa_timer_stop(ctx, epa_t(ctx, epa_ctx::T_EPCA_GRAM));
  hipLaunchKernelGGL(k_epca_identity, dim3((uint32_t)(((size_t)m * m + 255) / 256)), blk, 0, ctx->stream, el.V, m);
  EPA_HIP(ctx, hipMemsetAsync(el.count, 0, sizeof(uint32_t) * EPCA_MAX_SWEEPS, ctx->stream));
  EPA_HIP(ctx, hipMemcpyAsync(el.pairs, h_pairs.data(), sizeof(uint2) * h_pairs.size(), hipMemcpyHostToDevice, ctx->stream));
  EPA_HIP(ctx, hipGetLastError());
  uint32_t status[2] = {0, 0};
  std::vector<double> diag0(S), lam(S);
  EPA_HIP(ctx, hipMemcpyAsync(status, ly.status, sizeof(status), hipMemcpyDeviceToHost, ctx->stream));
  EPA_HIP(ctx, hipMemcpyAsync(diag0.data(), el.diag, sizeof(double) * S, hipMemcpyDeviceToHost, ctx->stream));
  EPA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (status[ST_BAD_BRANCH]) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "epca: a branch id is out of range");
  if (status[ST_BAD_SAMPLE]) return epa_fail(ctx, EPA_ERR_INVALID_ARG, "epca: a sample id is out of range");

  // ---- the Jacobi loop: the host drives, A and V stay on the device
  double eig_ms = 0.0;
  uint32_t n_sweeps = 0;
  const auto loop_begin = std::chrono::steady_clock::now();
  for (uint32_t sw = 0; sw < EPCA_MAX_SWEEPS; ++sw) {
    epa_timer_start(ctx, epa_t(ctx, epa_ctx::T_EPCA_EIG));
    hipLaunchKernelGGL(k_epca_sweep_begin, dim3(1), blk, 0, ctx->stream, el.A, S, m, el.thr);
    for (uint32_t step = 0; step + 1 < m; ++step) {
      const uint2* sp = el.pairs + (size_t)step * h;
      hipLaunchKernelGGL(k_epca_rot, dim3((h + 255) / 256), blk, 0, ctx->stream, el.A, S, m, sp, h, el.thr, el.rot, el.count + sw);
      hipLaunchKernelGGL(k_epca_apply, dim3((h + 255) / 256, h), blk, 0, ctx->stream, el.A, el.V, m, sp, h, el.rot);
    }
    epa_timer_stop(ctx, epa_t(ctx, epa_ctx::T_EPCA_EIG));
    uint32_t rotations = 0;
    EPA_HIP(ctx, hipMemcpyAsync(&rotations, el.count + sw, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    EPA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    {
      EvTimer& t = ctx->t_bank[bank][epa_ctx::T_EPCA_EIG];
      float ms = 0.f;
      if (ctx->opt.timers && t.valid && hipEventElapsedTime(&ms, t.a, t.b) == hipSuccess) eig_ms += (double)ms;
    }
    n_sweeps = sw + 1;
    if (!rotations) break;
  }
  const double loop_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - loop_begin).count();
  EPA_HIP(ctx, hipGetLastError());

  // ---- the Gram eigenvalues, sorted on the host: descending, equal values by ascending column
  hipLaunchKernelGGL(k_epca_diag, dim3((S + 255) / 256), blk, 0, ctx->stream, el.A, S, m, el.diag);
  EPA_HIP(ctx, hipMemcpyAsync(lam.data(), el.diag, sizeof(double) * S, hipMemcpyDeviceToHost, ctx->stream));
  EPA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  std::vector<uint32_t> order(S);
  for (uint32_t i = 0; i < S; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return lam[a] > lam[b]; });
  const double lam0 = lam[order[0]];
  std::vector<EpcaComp> comp(K);
  std::vector<double> h_eig(K);
  for (uint32_t k = 0; k < K; ++k) {
    const double l = lam[order[k]];
    comp[k].lam = l;
    comp[k].col = order[k];
    comp[k].null = (l <= 0x1p-40 * lam0 || lam0 <= 0.0 || !(l > 0.0)) ? 1u : 0u;
    h_eig[k] = std::max(l, 0.0) / (double)(S - 1);
  }
  double trace = 0.0;
  for (uint32_t i = 0; i < S; ++i) trace += diag0[i];
  const double h_total = trace / (double)(S - 1);

  // ---- edge vectors and projections
  epa_timer_start(ctx, epa_t(ctx, epa_ctx::T_EPCA_PROJECT));
  EPA_HIP(ctx, hipMemcpyAsync(el.comp, comp.data(), sizeof(EpcaComp) * K, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_epca_vecs, dim3((B + 255) / 256, K), blk, 0, ctx->stream, el.XT, Sp, el.V, m, S, tp.rank, tp.size, B, el.comp, el.ev);
  hipLaunchKernelGGL(k_epca_sign, dim3(K), blk, 0, ctx->stream, el.ev, B, el.sigma);
  hipLaunchKernelGGL(k_epca_proj, dim3((S * K + 255) / 256), blk, 0, ctx->stream, el.V, m, S, K, el.comp, el.sigma, el.proj);
  epa_timer_stop(ctx, epa_t(ctx, epa_ctx::T_EPCA_PROJECT));
  epa_timer_stop(ctx, epa_t(ctx, epa_ctx::T_EPCA));
  EPA_HIP(ctx, hipGetLastError());
  EPA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->opt.timers) {
    ctx->epca_ms[0] = eig_ms;
    ctx->epca_ms[1] = loop_ms;
  }
  EPA_HIP(ctx, hipMemcpy(eigenvalue, h_eig.data(), sizeof(double) * K, hipMemcpyDefault));
  EPA_HIP(ctx, hipMemcpy(total_var, &h_total, sizeof(double), hipMemcpyDefault));
  EPA_HIP(ctx, hipMemcpy(sweeps, &n_sweeps, sizeof(uint32_t), hipMemcpyDefault));
  EPA_HIP(ctx, hipMemcpy(edge_vec, el.ev, sizeof(double) * (size_t)K * B, hipMemcpyDefault));
  EPA_HIP(ctx, hipMemcpy(proj, el.proj, sizeof(double) * (size_t)S * K, hipMemcpyDefault));
  if (imbalance) EPA_HIP(ctx, hipMemcpy(imbalance, el.imb, sizeof(double) * (size_t)S * B, hipMemcpyDefault));
  if (gram) EPA_HIP(ctx, hipMemcpy(gram, el.gram, sizeof(double) * (size_t)S * S, hipMemcpyDefault));
  return EPA_OK;
}
