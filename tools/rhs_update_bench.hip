// tools/rhs_update_bench.hip -- what altro_hip_set_constraint_rhs and altro_hip_shift_constraint_rhs cost next to their roof (kernels/
// al_rhs.hip): the scatter reads a batch x (K * p) fp64 matrix and writes its transpose in the handle's element type, the shift reads
// and writes a block's segment once -- what a device-to-device copy of the same bytes does.  All in one process, alternating: the
// scatter through LDS (the library's form), the direct form, the shift, and hipMemcpyAsync of the fp64 source, for fp64 and fp32 pools.
// The kernels come from the library's own source.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude -Ialtro_amd/csrc tools/rhs_update_bench.hip -o tools/bin/rhs_update_bench
//   tools/bin/rhs_update_bench [batch = 4096] [K = 256] [p = 8] [repeats = 200]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kernels/al_rhs.hip"

using namespace altro_hip;
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

static double median(std::vector<float> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

template <typename T>
static void scatter_lds(hipStream_t s, T* dst, const double* src, int C, int batch) {
  const dim3 grid((batch + AL_RHS_TB - 1) / AL_RHS_TB, (C + AL_RHS_TC - 1) / AL_RHS_TC);
  if (C % 2 == 0) hipLaunchKernelGGL((al_rhs_scatter_kernel<T, true>), grid, dim3(AL_RHS_BLOCK), 0, s, dst, src, C, batch);
  else hipLaunchKernelGGL((al_rhs_scatter_kernel<T, false>), grid, dim3(AL_RHS_BLOCK), 0, s, dst, src, C, batch);
}
template <typename T>
static void scatter_lds_scalar(hipStream_t s, T* dst, const double* src, int C, int batch) {
  const dim3 grid((batch + AL_RHS_TB - 1) / AL_RHS_TB, (C + AL_RHS_TC - 1) / AL_RHS_TC);
  hipLaunchKernelGGL((al_rhs_scatter_kernel<T, false>), grid, dim3(AL_RHS_BLOCK), 0, s, dst, src, C, batch);
}
template <typename T>
static void scatter_direct(hipStream_t s, T* dst, const double* src, int C, int batch) {
  const dim3 grid((batch + AL_RHS_TB - 1) / AL_RHS_TB, (C + AL_RHS_TC - 1) / AL_RHS_TC);
  hipLaunchKernelGGL((al_rhs_scatter_direct_kernel<T>), grid, dim3(AL_RHS_TB), 0, s, dst, src, C, batch);
}
template <typename T>
static void shift(hipStream_t s, T* g, int K, int64_t stride) {
  hipLaunchKernelGGL((al_rhs_shift_kernel<T, AL_RHS_SHIFT_DEPTH>), dim3((unsigned)((stride + AL_RHS_SHIFT_BLOCK - 1) / AL_RHS_SHIFT_BLOCK)), dim3(AL_RHS_SHIFT_BLOCK), 0, s, g, K, stride);
}

template <typename T>
static int run(const char* type, int batch, int K, int p, int repeats) {
  const int C = K * p;
  const size_t count = (size_t)batch * C, sbytes = count * sizeof(double), dbytes = count * sizeof(T);
  double *src, *src2; T* dst;
  CK(hipMalloc(&src, sbytes)); CK(hipMalloc(&src2, sbytes)); CK(hipMalloc(&dst, dbytes));
  std::vector<double> host(count);
  for (size_t i = 0; i < count; ++i) host[i] = (double)(i % 16000057);
  CK(hipMemcpy(src, host.data(), sbytes, hipMemcpyHostToDevice));
  hipStream_t s; CK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  std::vector<T> got(count);
  // each scatter form once, checked on the host: dst[c][b] = src[b][c]; then one shift: dst[k] = old dst[k + 1], the last kept
  for (int form = 0; form < 3; ++form) {
    CK(hipMemsetAsync(dst, 0xff, dbytes, s));
    if (form == 0) scatter_lds<T>(s, dst, src, C, batch); else if (form == 1) scatter_lds_scalar<T>(s, dst, src, C, batch); else scatter_direct<T>(s, dst, src, C, batch);
    CK(hipStreamSynchronize(s));
    CK(hipMemcpy(got.data(), dst, dbytes, hipMemcpyDeviceToHost));
    size_t wrong = 0;
    for (int b = 0; b < batch; ++b)
      for (int c = 0; c < C; ++c) wrong += got[(size_t)c * batch + b] != (T)host[(size_t)b * C + c];
    if (wrong) { printf("%s scatter form %d WRONG (%zu)\n", type, form, wrong); return 1; }
  }
  shift<T>(s, dst, K, (int64_t)p * batch);
  CK(hipStreamSynchronize(s));
  std::vector<T> after(count);
  CK(hipMemcpy(after.data(), dst, dbytes, hipMemcpyDeviceToHost));
  size_t wrong = 0;
  const size_t stride = (size_t)p * batch;
  for (int k = 0; k < K; ++k)
    for (size_t e = 0; e < stride; ++e) wrong += after[k * stride + e] != got[(size_t)std::min(k + 1, K - 1) * stride + e];
  printf("%s: batch %d, %d knot points x %d rows: source %.1f MB fp64, segment %.1f MB; scatter forms and first shift %s\n", type, batch, K, p, sbytes / 1e6,
         dbytes / 1e6, wrong ? "WRONG" : "correct");
  if (wrong) return 1;
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  constexpr int NV = 6;
  std::vector<float> t[NV];
  for (int it = -10; it < repeats; ++it) {   // (ten warm-up rounds)
    for (int v = 0; v < NV; ++v) {
      CK(hipEventRecord(e0, s));
      switch (v) {
        case 0: CK(hipMemcpyAsync(src2, src, sbytes, hipMemcpyDeviceToDevice, s)); break;
        case 1: scatter_lds<T>(s, dst, src, C, batch); break;
        case 2: scatter_lds_scalar<T>(s, dst, src, C, batch); break;
        case 3: scatter_direct<T>(s, dst, src, C, batch); break;
        case 4: shift<T>(s, dst, K, (int64_t)p * batch); break;
        case 5: CK(hipMemcpyAsync(src2, dst, dbytes, hipMemcpyDeviceToDevice, s)); break;
      }
      CK(hipEventRecord(e1, s));
      CK(hipEventSynchronize(e1));
      float ms; CK(hipEventElapsedTime(&ms, e0, e1));
      if (it >= 0) t[v].push_back(ms);
    }
  }
  CK(hipGetLastError());
  const char* names[NV] = {"hipMemcpyAsync d2d of the fp64 source", "scatter through LDS, 16-byte reads (library)", "scatter through LDS, 8-byte reads",
                           "scatter, direct form", "shift (depth 16)", "hipMemcpyAsync d2d of the segment"};
  const double moved[NV] = {2.0 * sbytes, (double)sbytes + dbytes, (double)sbytes + dbytes, (double)sbytes + dbytes, 2.0 * dbytes, 2.0 * dbytes};
  for (int v = 0; v < NV; ++v) {
    const double ms = median(t[v]), roof = median(t[v == 4 || v == 5 ? 5 : 0]);
    printf("  %-46s median %8.4f ms  min %8.4f ms  %7.1f GB/s read + written  %.2f x its copy\n", names[v], ms, *std::min_element(t[v].begin(), t[v].end()),
           moved[v] / ms / 1e6, ms / roof);
  }
  CK(hipFree(src)); CK(hipFree(src2)); CK(hipFree(dst));
  return 0;
}

int main(int argc, char** argv) {
  const int batch = argc > 1 ? atoi(argv[1]) : 4096, K = argc > 2 ? atoi(argv[2]) : 256, p = argc > 3 ? atoi(argv[3]) : 8;
  const int repeats = argc > 4 ? atoi(argv[4]) : 200;
  if (run<double>("fp64", batch, K, p, repeats)) return 1;
  return run<float>("fp32", batch, K, p, repeats);
}
