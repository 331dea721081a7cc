// float64 vector FMA rate of the GPU: the ceiling scripts/measure_ssim.py compares u8_ssim_kernel against.
//   hipcc --offload-arch=gfx950 -O3 scripts/fp64_fma_peak.hip -o fp64_fma_peak && ./fp64_fma_peak
// Every lane runs 16 independent fma chains (no memory traffic); the grid fills every CU 8 blocks deep.  Prints one
// JSON line with the best of 5 timed launches.
#include <hip/hip_runtime.h>

#include <cstdio>

constexpr int kChains = 16, kIters = 8192, kThreads = 256;

__global__ __launch_bounds__(kThreads) void fma_kernel(double* out, double a, double b) {
  double acc[kChains];
#pragma unroll
  for (int i = 0; i < kChains; ++i) acc[i] = (double)(threadIdx.x + i);
  for (int it = 0; it < kIters; ++it)
#pragma unroll
    for (int i = 0; i < kChains; ++i) acc[i] = __builtin_fma(acc[i], a, b);
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < kChains; ++i) s += acc[i];
  out[blockIdx.x * kThreads + threadIdx.x] = s;
}

#define CHECK(x)                                                              \
  do {                                                                        \
    hipError_t e = (x);                                                       \
    if (e != hipSuccess) {                                                    \
      std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e));             \
      return 1;                                                               \
    }                                                                         \
  } while (0)

int main() {
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, 0));
  const int blocks = prop.multiProcessorCount * 8;
  double* out = nullptr;
  CHECK(hipMalloc(&out, sizeof(double) * blocks * kThreads));
  hipEvent_t t0, t1;
  CHECK(hipEventCreate(&t0));
  CHECK(hipEventCreate(&t1));
  float best = 1e30f;
  for (int rep = 0; rep < 7; ++rep) {      // 2 warm-up launches, 5 timed
    CHECK(hipEventRecord(t0, 0));
    hipLaunchKernelGGL(fma_kernel, dim3(blocks), dim3(kThreads), 0, 0, out, 0.999999, 1e-9);
    CHECK(hipEventRecord(t1, 0));
    CHECK(hipEventSynchronize(t1));
    float ms = 0.f;
    CHECK(hipEventElapsedTime(&ms, t0, t1));
    if (rep >= 2 && ms < best) best = ms;
  }
  const double fmas = (double)blocks * kThreads * kChains * kIters;
  std::printf("{\"metric\": \"float64 vector FMA rate\", \"value\": %.3f, \"unit\": \"TFMA/s\", \"cus\": %d, "
              "\"ms\": %.4f, \"fmas\": %.0f}\n",
              fmas / (best * 1e-3) / 1e12, prop.multiProcessorCount, best, fmas);
  CHECK(hipFree(out));
  return 0;
}
