// Go / no-go for k_thorough_dna's Newton table in registers: what does an fp64 FMA stream pay for its wave-uniform
// operand when that operand comes (a) from a VGPR, (b) from another lane of the row through the FMA's own DPP control
// (v_fmac_f64_dpp ... row_newbcast:n, the one DPP control gfx950's fp64 ALU accepts), (c) from LDS, one wave-uniform
// ds_read_b128 feeding every 4 FMAs (the shape of today's evaluation: 27 ds_read_b128 for ~90 FMAs)?
// Two waves per SIMD (56 KB of LDS per 4-wave workgroup: two workgroups per CU), 8 independent accumulators per lane.
// Prints wall ms, shader cycles per FMA instruction per SIMD and the clock the waves saw; first checks that
// row_newbcast:n hands every lane of a row the value of lane n of that row.
//   hipcc --offload-arch=gfx950 -O3 profiles/dpp_bcast.hip -o /tmp/dpp_bcast && /tmp/dpp_bcast
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

template <int N>
__device__ __forceinline__ void fmac_bcast(double& acc, double t, double s) {
  asm("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(t), "v"(s), "i"(N));
}
__device__ __forceinline__ void fmac(double& acc, double t, double s) {
  asm("v_fmac_f64_e32 %0, %1, %2" : "+v"(acc) : "v"(t), "v"(s));
}

__global__ void k_check(double* out) {
  const int lane = threadIdx.x;
  double t = (double)lane, acc0 = 0.0, acc5 = 0.0;
  asm volatile("s_nop 1" : "+v"(t));   // VALU write -> DPP read: 2 wait states
  fmac_bcast<0>(acc0, t, 1.0 + 0.0 * t);
  fmac_bcast<5>(acc5, t, 1.0 + 0.0 * t);
  out[lane] = acc0;
  out[64 + lane] = acc5;
}

// MODE 0: VGPR operand, 1: row_newbcast operand, 2: VGPR operand loaded by one uniform ds_read_b128 per 4 FMAs
template <int MODE>
__global__ void __launch_bounds__(256) k_stream(double* out, unsigned long long* stamps, int iters) {
  __shared__ __attribute__((aligned(16))) double tab[7168];   // 56 KB: two workgroups (8 waves) per CU
  for (int i = threadIdx.x; i < 7168; i += 256) tab[i] = 1.0 + i * 1e-12;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  double t = 1.0 + lane * 1e-9, s[8], c[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { s[j] = 1.0 - j * 1e-12; c[j] = 0.125 * j; }
  asm volatile("s_nop 1" : "+v"(t));
  const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
  for (int i = 0; i < iters; ++i) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (MODE == 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) fmac(c[j], t, s[j]);
      } else if (MODE == 1) {
        fmac_bcast<1>(c[0], t, s[0]); fmac_bcast<4>(c[1], t, s[1]); fmac_bcast<7>(c[2], t, s[2]);
        fmac_bcast<10>(c[3], t, s[3]); fmac_bcast<2>(c[4], t, s[4]); fmac_bcast<5>(c[5], t, s[5]);
        fmac_bcast<8>(c[6], t, s[6]); fmac_bcast<11>(c[7], t, s[7]);
      } else {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const double2 v = *reinterpret_cast<const double2*>(&tab[((i * 8 + u * 2 + h) & 511) * 2]);   // wave-uniform
          fmac(c[4 * h], v.x, s[4 * h]); fmac(c[4 * h + 1], v.y, s[4 * h + 1]);
          fmac(c[4 * h + 2], v.x, s[4 * h + 2]); fmac(c[4 * h + 3], v.y, s[4 * h + 3]);
        }
      }
    }
  }
  const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
  double sum = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) sum += c[j];
  out[blockIdx.x * 256 + threadIdx.x] = sum;
  if (lane == 0) {
    const size_t w = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    stamps[2 * w] = t1 - t0;
    stamps[2 * w + 1] = r1 - r0;
  }
}

int main() {
  const int grid = 512;   // 256 CUs x 4 SIMDs x 2 waves
  double* d;
  unsigned long long* st;
  if (hipMalloc(&d, sizeof(double) * 256 * grid) != hipSuccess || hipMalloc(&st, 16 * 4 * grid) != hipSuccess) return 1;
  {
    hipLaunchKernelGGL(k_check, dim3(1), dim3(64), 0, 0, d);
    std::vector<double> h(128);
    if (hipMemcpy(h.data(), d, sizeof(double) * 128, hipMemcpyDeviceToHost) != hipSuccess) return 1;
    int bad = 0;
    for (int l = 0; l < 64; ++l) bad += (h[l] != (double)(l & ~15)) + (h[64 + l] != (double)((l & ~15) + 5));
    printf("# row_newbcast:n check (lane l reads lane 16 (l / 16) + n): %s\n", bad ? "FAILED" : "ok");
    if (bad) return 2;
  }
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  std::vector<unsigned long long> h(2 * 4 * grid);
  printf("# form                                      wall_ms   cycles/FMA/SIMD p50   sclk_MHz p50 (min..max)\n");
  auto run = [&](auto kern, const char* name, int iters) {
    for (int rep = 0; rep < 3; ++rep) {   // the third of three back-to-back launches is reported (clock settled)
      (void)hipEventRecord(e0);
      hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, 0, d, st, iters);
      (void)hipEventRecord(e1);
      (void)hipEventSynchronize(e1);
    }
    float ms;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipMemcpy(h.data(), st, 16 * 4 * grid, hipMemcpyDeviceToHost);
    std::vector<double> mhz, cpf;
    for (int w = 0; w < 4 * grid; ++w)
      if (h[2 * w + 1]) {
        mhz.push_back(100.0 * (double)h[2 * w] / (double)h[2 * w + 1]);
        cpf.push_back((double)h[2 * w] / ((double)iters * 32.0 * 2.0));   // two waves share the SIMD
      }
    std::sort(mhz.begin(), mhz.end());
    std::sort(cpf.begin(), cpf.end());
    printf("  %-40s %9.3f   %8.3f              %6.0f (%.0f..%.0f)\n", name, ms, cpf[cpf.size() / 2], mhz[mhz.size() / 2],
           mhz.front(), mhz.back());
  };
  const int it = 400000;
  run(k_stream<0>, "(a) v_fmac_f64, VGPR operand", it);
  run(k_stream<1>, "(b) v_fmac_f64_dpp row_newbcast:n", it);
  run(k_stream<2>, "(c) (a) + 1 ds_read_b128 per 4 FMAs", it);
  run(k_stream<0>, "(a) again", it);
  run(k_stream<1>, "(b) again", it);
  return 0;
}
