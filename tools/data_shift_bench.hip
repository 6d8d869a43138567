// tools/data_shift_bench.hip -- what the receding-horizon shifts of the problem data cost on the C1 handle (plan MFMA16, fp64) next to
// their roof: altro_hip_shift_dynamics and altro_hip_shift_linear_costs (kernels/shift_field.hip) read and write each byte they move
// once -- what a device-to-device copy of the same bytes does -- and a one-knot-point altro_hip_set_dynamics_range from a device array
// is set against the full altro_hip_set_dynamics it replaces in an MPC step.  Through the library's C ABI, all in one process,
// alternating, on the handle's own stream.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude tools/data_shift_bench.hip -Laltro_amd/lib -laltro_hip -Wl,-rpath,'$ORIGIN/../../altro_amd/lib' -o tools/bin/data_shift_bench
//   tools/bin/data_shift_bench [batch = 4096] [N = 256] [repeats = 50]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "altro_hip/altro_hip.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)
#define AK(x) do { int r_ = (x); if (r_ != 0) { printf("%s: %d %s\n", #x, r_, altro_hip_last_error()); return 1; } } while (0)

__global__ void fill_kernel(double* p, size_t count, double scale) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) p[i] = scale * (double)(i % 1000003);
}
static double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

int main(int argc, char** argv) {
  const int batch = argc > 1 ? atoi(argv[1]) : 4096, N = argc > 2 ? atoi(argv[2]) : 256, repeats = argc > 3 ? atoi(argv[3]) : 50;
  const int n = 12, m = 4;
  hipStream_t s; CK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  altro_hip_batch* h = nullptr;
  AK(altro_hip_batch_create(&h, N, n, m, batch, ALTRO_HIP_F64, ALTRO_HIP_PLAN_MFMA16, 0, 0, s));
  // the diagonal tracking cost, one reference for the sizes' sake (the shift moves the records whatever they hold)
  {
    std::vector<double> Qd(2 * n, 1.0), Rd(m, 0.01), xref(2 * n, 0.25), uref(m, 0.0);
    AK(altro_hip_set_tracking_cost(h, Qd.data(), Rd.data(), xref.data(), uref.data(), 1, 1));
  }
  const size_t cA = (size_t)batch * N * n * n, cB = (size_t)batch * N * n * m, cf = (size_t)batch * N * n;
  double *A, *B, *f;
  CK(hipMalloc(&A, cA * 8)); CK(hipMalloc(&B, cB * 8)); CK(hipMalloc(&f, cf * 8));
  hipLaunchKernelGGL(fill_kernel, dim3(4096), dim3(256), 0, s, A, cA, 1e-6);
  hipLaunchKernelGGL(fill_kernel, dim3(4096), dim3(256), 0, s, B, cB, 2e-6);
  hipLaunchKernelGGL(fill_kernel, dim3(4096), dim3(256), 0, s, f, cf, 3e-6);
  CK(hipStreamSynchronize(s));
  AK(altro_hip_set_pointer_mode(h, 1));
  AK(altro_hip_set_dynamics(h, A, B, f, 0, 0));
  // one shift, checked: knot point k holds what k + 1 held, the last one kept
  {
    if (N < 4) { printf("N >= 4, please\n"); return 1; }
    std::vector<double> a0((size_t)batch * n * n), a1(a0.size()), am(a0.size()), f0((size_t)batch * n), f1(f0.size());
    size_t wrong = 0;
    AK(altro_hip_get_dynamics_knot(h, 1, a1.data(), nullptr, f1.data()));
    AK(altro_hip_get_dynamics_knot(h, N / 2 + 1, am.data(), nullptr, nullptr));
    AK(altro_hip_shift_dynamics(h));
    AK(altro_hip_get_dynamics_knot(h, 0, a0.data(), nullptr, f0.data()));
    wrong += a0 != a1; wrong += f0 != f1;
    AK(altro_hip_get_dynamics_knot(h, N / 2, a0.data(), nullptr, nullptr));
    wrong += a0 != am;
    AK(altro_hip_get_dynamics_knot(h, N - 1, a0.data(), nullptr, nullptr));
    AK(altro_hip_get_dynamics_knot(h, N - 2, a1.data(), nullptr, nullptr));
    wrong += a0 != a1;
    printf("C1 handle: batch %d, N %d, (12, 4) fp64 on plan MFMA16; first shift %s\n", batch, N, wrong ? "WRONG" : "correct");
    if (wrong) return 1;
  }
  const size_t dyn_bytes = (size_t)batch * (N - 1) * 204 * 8, cost_bytes = (size_t)batch * (N - 1) * 17 * 8;   // what each shift reads (and writes)
  char *c0, *c1;
  CK(hipMalloc(&c0, dyn_bytes)); CK(hipMalloc(&c1, dyn_bytes));
  CK(hipMemsetAsync(c0, 1, dyn_bytes, s)); CK(hipMemsetAsync(c1, 2, dyn_bytes, s));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  constexpr int NV = 4;
  std::vector<double> t[NV];
  for (int it = -5; it < repeats; ++it) {   // (five warm-up rounds)
    for (int v = 0; v < NV; ++v) {
      CK(hipEventRecord(e0, s));
      switch (v) {
        case 0: CK(hipMemcpyAsync(c1, c0, dyn_bytes, hipMemcpyDeviceToDevice, s)); break;
        case 1: AK(altro_hip_shift_dynamics(h)); break;
        case 2: CK(hipMemcpyAsync(c1, c0, cost_bytes, hipMemcpyDeviceToDevice, s)); break;
        case 3: AK(altro_hip_shift_linear_costs(h)); break;
      }
      CK(hipEventRecord(e1, s));
      CK(hipEventSynchronize(e1));
      float ms; CK(hipEventElapsedTime(&ms, e0, e1));
      if (it >= 0) t[v].push_back(ms);
    }
  }
  const char* names[NV] = {"hipMemcpyAsync d2d of the DYN bytes moved", "altro_hip_shift_dynamics", "hipMemcpyAsync d2d of the q | r | c bytes moved",
                           "altro_hip_shift_linear_costs"};
  const double moved[NV] = {2.0 * dyn_bytes, 2.0 * dyn_bytes, 2.0 * cost_bytes, 2.0 * cost_bytes};
  printf("shifts (hipEvents on the handle's stream, medians of %d after 5 warm-up rounds; DYN %.1f MB, q | r | c %.1f MB of the 36-element COSTP records):\n", repeats,
         dyn_bytes / 1e6, cost_bytes / 1e6);
  for (int v = 0; v < NV; ++v) {
    const double ms = median(t[v]), roof = median(t[v & ~1]);
    printf("  %-48s median %8.4f ms  min %8.4f ms  %7.1f GB/s read + written  %.2f x its copy\n", names[v], ms, *std::min_element(t[v].begin(), t[v].end()),
           moved[v] / ms / 1e6, ms / roof);
  }
  // the data update of one MPC step: the whole horizon repacked against the new last knot point written (both from device arrays,
  // both synchronise before they return: wall clock)
  std::vector<double> whole, one;
  const int few = std::max(3, repeats / 10);
  for (int it = -1; it < few; ++it) {
    auto w0 = std::chrono::steady_clock::now();
    AK(altro_hip_set_dynamics(h, A, B, f, 0, 0));
    auto w1 = std::chrono::steady_clock::now();
    if (it >= 0) whole.push_back(std::chrono::duration<double, std::milli>(w1 - w0).count());
  }
  // (sources of one knot point per problem: [batch][1][block], packed)
  double *A1, *B1, *f1;
  CK(hipMalloc(&A1, (size_t)batch * n * n * 8)); CK(hipMalloc(&B1, (size_t)batch * n * m * 8)); CK(hipMalloc(&f1, (size_t)batch * n * 8));
  hipLaunchKernelGGL(fill_kernel, dim3(1024), dim3(256), 0, s, A1, (size_t)batch * n * n, 1e-6);
  hipLaunchKernelGGL(fill_kernel, dim3(1024), dim3(256), 0, s, B1, (size_t)batch * n * m, 2e-6);
  hipLaunchKernelGGL(fill_kernel, dim3(1024), dim3(256), 0, s, f1, (size_t)batch * n, 3e-6);
  CK(hipStreamSynchronize(s));
  for (int it = -5; it < repeats; ++it) {
    auto w0 = std::chrono::steady_clock::now();
    AK(altro_hip_set_dynamics_range(h, A1, B1, f1, N - 1, N - 1, 0));
    auto w1 = std::chrono::steady_clock::now();
    if (it >= 0) one.push_back(std::chrono::duration<double, std::milli>(w1 - w0).count());
  }
  const double shift_ms = median(t[1]);
  printf("the dynamics' update of one MPC step, from device arrays (wall clock, the calls synchronise):\n");
  printf("  altro_hip_set_dynamics, the whole horizon (%.1f MB of sources)   median %9.4f ms\n", (cA + cB + cf) * 8 / 1e6, median(whole));
  printf("  altro_hip_set_dynamics_range, knot point N-1 (%.2f MB)          median %9.4f ms\n", (double)batch * (n * n + n * m + n) * 8 / 1e6, median(one));
  printf("  shift + one-knot-point write                                     %9.4f ms  = whole / %.1f\n", shift_ms + median(one), median(whole) / (shift_ms + median(one)));
  altro_hip_batch_destroy(h);
  return 0;
}
