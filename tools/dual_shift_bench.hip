// tools/dual_shift_bench.hip -- what the duals' receding-horizon shift (kernels/al_shift.hip, altro_hip_shift_duals) costs next to its
// roof: the kernel reads and writes every dual once, which is what a device-to-device copy of the dual array does.  Both in one
// process, alternating, on the same buffer size: z[rows][batch] of a uniform running block (rows_per_knot rows at knot points 0 .. N-1).
// The chains come from al_shift.h, the kernel from the library's own source, at its own depth (AL_SHIFT_DEPTH) and at others.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude -Ialtro_amd/csrc tools/dual_shift_bench.hip -o tools/bin/dual_shift_bench
//   tools/bin/dual_shift_bench [batch = 4096] [N = 256] [rows_per_knot = 8] [repeats = 200]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "al_shift.h"
#include "kernels/al_shift.hip"

using namespace altro_hip;
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

template <int DEPTH>
static void launch(hipStream_t s, double* z, const int* order, const int* start, int nchains, int batch) {
  hipLaunchKernelGGL((al_shift_duals_kernel<double, DEPTH>), dim3((batch + AL_SHIFT_BLOCK - 1) / AL_SHIFT_BLOCK, nchains), dim3(AL_SHIFT_BLOCK), 0, s,
                     z, order, start, nchains, batch, 0);
}
static double median(std::vector<float> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

int main(int argc, char** argv) {
  const int batch = argc > 1 ? atoi(argv[1]) : 4096, N = argc > 2 ? atoi(argv[2]) : 256, rpk = argc > 3 ? atoi(argv[3]) : 8;
  const int repeats = argc > 4 ? atoi(argv[4]) : 200;
  // the completed knot-point records of one block of rpk rows at 0 .. N-1 (al_tables.h packs the rows in knot-point order)
  std::vector<AlDef> defs(1);
  defs[0].cone = CONE_INEQUALITY; defs[0].p = rpk;
  std::vector<AlKnotBig> big((size_t)N + 1, AlKnotBig{});
  for (int k = 0; k < N; ++k) { big[k].ncon = 1; big[k].def[0] = 0; big[k].z_off[0] = k * rpk; big[k].p[0] = rpk; }
  const int rows = N * rpk;
  const capi::AlShift sh = capi::al_shift_build(big, defs, rows);
  const size_t count = (size_t)rows * batch, bytes = count * sizeof(double);
  double *z, *z2; int *order, *start;
  CK(hipMalloc(&z, bytes)); CK(hipMalloc(&z2, bytes));
  CK(hipMalloc(&order, sh.order.size() * sizeof(int))); CK(hipMalloc(&start, sh.start.size() * sizeof(int)));
  CK(hipMemcpy(order, sh.order.data(), sh.order.size() * sizeof(int), hipMemcpyHostToDevice));
  CK(hipMemcpy(start, sh.start.data(), sh.start.size() * sizeof(int), hipMemcpyHostToDevice));
  std::vector<double> host(count);
  for (size_t i = 0; i < count; ++i) host[i] = (double)i;
  CK(hipMemcpy(z, host.data(), bytes, hipMemcpyHostToDevice));
  hipStream_t s; CK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  const int nheads = (int)sh.heads.size();
  // one shift at the library's depth, checked on the host: z[row] = old z[row + rpk], the last knot point's rows kept
  launch<AL_SHIFT_DEPTH>(s, z, order, start, nheads, batch);
  CK(hipStreamSynchronize(s));
  std::vector<double> got(count);
  CK(hipMemcpy(got.data(), z, bytes, hipMemcpyDeviceToHost));
  size_t wrong = 0;
  for (int r = 0; r < rows; ++r)
    for (int b = 0; b < batch; ++b) wrong += got[(size_t)r * batch + b] != host[(size_t)std::min(r + rpk, rows - rpk + r % rpk) * batch + b];
  printf("batch %d, N %d, %d rows per knot point: %d chains of %d links, %.1f MB of duals; first shift %s\n", batch, N, rpk, nheads, N - 1, bytes / 1e6,
         wrong ? "WRONG" : "correct");
  if (wrong) return 1;
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  std::vector<float> t[5];
  for (int it = -10; it < repeats; ++it) {   // (ten warm-up rounds)
    for (int v = 0; v < 5; ++v) {
      CK(hipEventRecord(e0, s));
      switch (v) {
        case 0: CK(hipMemcpyAsync(z2, z, bytes, hipMemcpyDeviceToDevice, s)); break;
        case 1: launch<8>(s, z, order, start, nheads, batch); break;
        case 2: launch<16>(s, z, order, start, nheads, batch); break;
        case 3: launch<32>(s, z, order, start, nheads, batch); break;
        case 4: launch<4>(s, z, order, start, nheads, batch); break;
      }
      CK(hipEventRecord(e1, s));
      CK(hipEventSynchronize(e1));
      float ms; CK(hipEventElapsedTime(&ms, e0, e1));
      if (it >= 0) t[v].push_back(ms);
    }
  }
  CK(hipGetLastError());
  const char* names[5] = {"hipMemcpyAsync device to device", "shift kernel, depth 8", "shift kernel, depth 16 (the library's)", "shift kernel, depth 32", "shift kernel, depth 4"};
  const double roof = median(t[0]);
  for (int v = 0; v < 5; ++v) {
    const double ms = median(t[v]);
    printf("%-40s median %8.4f ms  min %8.4f ms  %7.1f GB/s read + written  %.2f x the copy\n", names[v], ms, *std::min_element(t[v].begin(), t[v].end()),
           2.0 * bytes / ms / 1e6, ms / roof);
  }
  return 0;
}
