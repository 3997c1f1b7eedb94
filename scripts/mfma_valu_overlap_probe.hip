// Does fp64 VALU work overlap with v_mfma_f64_16x16x4_f64 on gfx950, or do both run on the same fp64
// datapath?  Each wave runs ITER x { 16 independent MFMAs, NV FMAs interleaved 1:NV/16 } with the FMAs
// in fp64, fp32 or absent; 2 waves per SIMD (as the fused posterior kernel).  Prints time per variant
// and the time the pure-VALU part takes alone, so "sum" vs "max" behaviour can be read off directly.
// Second part: what single fp64 instructions of the kernel-value chain cost beside the same MFMA stream - v_rndne_f64,
// v_cvt_i32_f64, v_ldexp_f64, v_max_f64, v_rsq_f64, with v_fma_f64 and the 32-bit integer add as yardsticks - as SIMD cycles per
// instruction at the device's nominal clock: (time with 64 of them per 16 MFMAs - time of the MFMAs alone) / instructions per SIMD.
//   hipcc -O3 --offload-arch=gfx950 scripts/mfma_valu_overlap_probe.hip -o /tmp/ovl && /tmp/ovl
#include <hip/hip_runtime.h>
#include <stdio.h>
typedef double d4 __attribute__((ext_vector_type(4)));

template <int MODE, int NV, bool MF>  // MODE 0: no VALU, 1: fp64 FMA, 2: fp32 FMA; MF: issue the MFMAs
__global__ __launch_bounds__(256, 2) void probe(double* out, int iters) {
  d4 acc[16];
  for (int j = 0; j < 16; j++) acc[j] = (d4){0, 0, 0, 0};
  double a = 1.0 + threadIdx.x * 1e-9, b = 1.0 - threadIdx.x * 1e-9;
  double x[8];
  float xf[8];
  for (int u = 0; u < 8; u++) { x[u] = 0.5 + u + threadIdx.x; xf[u] = 0.5f + u + threadIdx.x; }
  const double m = 0.999999, c = 1e-7;
  const float mf = 0.999999f, cf = 1e-7f;
  for (int it = 0; it < iters; it++) {
#pragma unroll
    for (int j = 0; j < 16; j++) {
      if (MF) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[j], 0, 0, 0);
#pragma unroll
      for (int v = 0; v < NV / 16; v++) {
        const int u = (j * (NV / 16) + v) % 8;
        if (MODE == 1) x[u] = fma(x[u], m, c);
        if (MODE == 2) xf[u] = fmaf(xf[u], mf, cf);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  double s = 0;
  for (int j = 0; j < 16; j++) s += acc[j][0] + acc[j][1] + acc[j][2] + acc[j][3];
  for (int u = 0; u < 8; u++) s += x[u] + xf[u];
  out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

// One instruction kind, NV per 16 MFMAs, on eight independent registers (inline assembly: the compiler neither folds nor moves them)
enum { OP_FMA, OP_RNDNE, OP_CVT_I32, OP_LDEXP, OP_MAX, OP_RSQ, OP_IADD };
template <int OP, int NV, bool MF>
__global__ __launch_bounds__(256, 2) void probe_op(double* out, int iters) {
  d4 acc[16];
  for (int j = 0; j < 16; j++) acc[j] = (d4){0, 0, 0, 0};
  double a = 1.0 + threadIdx.x * 1e-9, b = 1.0 - threadIdx.x * 1e-9;
  double x[8];
  int e[8];
  for (int u = 0; u < 8; u++) { x[u] = 1.5 + u + threadIdx.x; e[u] = (u & 1) ? 1 : -1; }
  const double m = 0.999999, c = 1e-7;
  for (int it = 0; it < iters; it++) {
#pragma unroll
    for (int j = 0; j < 16; j++) {
      if (MF) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[j], 0, 0, 0);
#pragma unroll
      for (int v = 0; v < NV / 16; v++) {
        const int u = (j * (NV / 16) + v) % 8;
        if (OP == OP_FMA) asm volatile("v_fma_f64 %0, %0, %1, %2" : "+v"(x[u]) : "v"(m), "v"(c));
        if (OP == OP_RNDNE) asm volatile("v_rndne_f64 %0, %0" : "+v"(x[u]));
        if (OP == OP_CVT_I32) asm volatile("v_cvt_i32_f64 %0, %1" : "=v"(e[u]) : "v"(x[u]));
        if (OP == OP_LDEXP) asm volatile("v_ldexp_f64 %0, %0, %1" : "+v"(x[u]) : "v"(e[u]));
        if (OP == OP_MAX) asm volatile("v_max_f64 %0, %0, %1" : "+v"(x[u]) : "v"(m));
        if (OP == OP_RSQ) asm volatile("v_rsq_f64 %0, %0" : "+v"(x[u]));
        if (OP == OP_IADD) asm volatile("v_add_u32 %0, %0, %1" : "+v"(e[u]) : "v"(e[(u + 1) % 8]));
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  double s = 0;
  for (int j = 0; j < 16; j++) s += acc[j][0] + acc[j][1] + acc[j][2] + acc[j][3];
  for (int u = 0; u < 8; u++) s += x[u] + e[u];
  out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

template <int OP, int NV, bool MF>
static float time_op(double* d, int grid, int iters) {
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  hipLaunchKernelGGL((probe_op<OP, NV, MF>), dim3(grid), dim3(256), 0, 0, d, iters);
  hipDeviceSynchronize();
  hipEventRecord(e0);
  hipLaunchKernelGGL((probe_op<OP, NV, MF>), dim3(grid), dim3(256), 0, 0, d, iters);
  hipEventRecord(e1);
  hipEventSynchronize(e1);
  float ms;
  hipEventElapsedTime(&ms, e0, e1);
  return ms;
}

// two waves per SIMD, each issuing iters * NV instructions: cycles per instruction = added time * clock / (2 iters NV)
template <int OP>
static void run_op(const char* name, double* d, int grid, int iters, float mfma_ms, double clock_khz) {
  constexpr int NV = 64;
  const float alone = time_op<OP, NV, false>(d, grid, iters), beside = time_op<OP, NV, true>(d, grid, iters);
  const double per = clock_khz * 1e3 / (2.0 * iters * NV) * 1e-3;  // cycles per ms of added time and instruction
  printf("%-16s alone %8.3f ms (%5.2f cycles)   beside MFMA %8.3f ms (+%5.2f cycles per instruction)\n", name, alone, alone * per, beside,
         (beside - mfma_ms) * per);
}

template <int MODE, int NV, bool MF>
static void run(const char* name, double* d, int grid, int iters) {
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  hipLaunchKernelGGL((probe<MODE, NV, MF>), dim3(grid), dim3(256), 0, 0, d, iters);
  hipDeviceSynchronize();
  hipEventRecord(e0);
  hipLaunchKernelGGL((probe<MODE, NV, MF>), dim3(grid), dim3(256), 0, 0, d, iters);
  hipEventRecord(e1);
  hipEventSynchronize(e1);
  float ms;
  hipEventElapsedTime(&ms, e0, e1);
  const double mfma_flops = MF ? (double)grid * 4 * iters * 16 * 2.0 * 16 * 16 * 4 : 0.0;
  printf("%-34s %8.3f ms   MFMA %6.1f TFLOP/s\n", name, ms, mfma_flops / ms * 1e-9);
}

int main() {
  const int grid = 512, iters = 20000;  // 2 blocks per CU -> 2 waves per SIMD
  double* d;
  hipMalloc(&d, sizeof(double) * grid * 256);
  run<0, 0, true>("MFMA only", d, grid, iters);
  run<1, 32, false>("fp64 FMA x32 only", d, grid, iters);
  run<1, 32, true>("MFMA + fp64 FMA x32", d, grid, iters);
  run<1, 64, false>("fp64 FMA x64 only", d, grid, iters);
  run<1, 64, true>("MFMA + fp64 FMA x64", d, grid, iters);
  run<1, 128, false>("fp64 FMA x128 only", d, grid, iters);
  run<1, 128, true>("MFMA + fp64 FMA x128", d, grid, iters);
  run<2, 64, false>("fp32 FMA x64 only", d, grid, iters);
  run<2, 64, true>("MFMA + fp32 FMA x64", d, grid, iters);
  run<2, 128, false>("fp32 FMA x128 only", d, grid, iters);
  run<2, 128, true>("MFMA + fp32 FMA x128", d, grid, iters);
  // single instructions of the kernel-value chain, 64 per 16 MFMAs
  int clock_khz = 0;
  hipDeviceGetAttribute(&clock_khz, hipDeviceAttributeClockRate, 0);
  const float mfma_ms = time_op<OP_FMA, 0, true>(d, grid, iters);
  printf("per-instruction cost at the nominal clock of %d MHz (MFMA stream alone: %.3f ms)\n", clock_khz / 1000, mfma_ms);
  run_op<OP_FMA>("v_fma_f64", d, grid, iters, mfma_ms, clock_khz);
  run_op<OP_RNDNE>("v_rndne_f64", d, grid, iters, mfma_ms, clock_khz);
  run_op<OP_CVT_I32>("v_cvt_i32_f64", d, grid, iters, mfma_ms, clock_khz);
  run_op<OP_LDEXP>("v_ldexp_f64", d, grid, iters, mfma_ms, clock_khz);
  run_op<OP_MAX>("v_max_f64", d, grid, iters, mfma_ms, clock_khz);
  run_op<OP_RSQ>("v_rsq_f64", d, grid, iters, mfma_ms, clock_khz);
  run_op<OP_IADD>("v_add_u32", d, grid, iters, mfma_ms, clock_khz);
  return 0;
}
