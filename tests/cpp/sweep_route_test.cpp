// sweep_route.h against rows written out by hand from the launchers' arithmetic: which instantiation of generic_backward_kernel /
// generic_forward_kernel a launch takes.  Plain g++, nothing of the library linked.
//   carve of the backward kernel: (4 | 3) n^2 + 4 n m + 2 m^2 + 5 n + 3 m elements + 64 bytes; a compute unit holds
//   min(16, 163840 / carve) problems; late Q from batch 256 * per_cu(4 n^2 carve) + 1 up where the 3 n^2 carve holds more.
//     (24, 8) fp64: 2304 + 768 + 128 + 120 + 24 = 3344 el -> 26816 B (6 per CU); 2768 el -> 22208 B (7 per CU): late Q past 1536.
//     (33, 7) fp64: 4356 + 924 + 98 + 165 + 21 = 5564 el -> 44576 B (3); 4475 el -> 35864 B (4): past 768.
//     (40, 10) fp64: 6400 + 1600 + 200 + 200 + 30 = 8430 el -> 67504 B > 64 KB; 6830 el -> 54704 B: late Q at every batch.
//     (40, 6) fp64: 6400 + 960 + 72 + 200 + 18 = 7650 el -> 61264 B (2); 6050 el -> 48464 B (3): past 512, NOT at a batch of one.
#include <cstdio>
#include <initializer_list>

#include "sweep_route.h"

using namespace altro_hip;

static int failures = 0;
static const unsigned ON = ALTRO_HIP_FORM_GENERIC_LATE_Q_ON, OFF = ALTRO_HIP_FORM_GENERIC_LATE_Q_OFF;
static const int LQ = ALTRO_HIP_SWEEP_LATE_Q, WS = ALTRO_HIP_SWEEP_GLOBAL_WORKSPACE, ST = ALTRO_HIP_SWEEP_FORWARD_STAGED;

static void backward(int n, int m, size_t esz, long long batch, unsigned forms, int variant, size_t bytes) {
  const GenericBackwardRoute r = generic_backward_route(n, m, esz, batch, forms);
  if (r.variant() != variant || r.bytes != bytes || r.late_q != ((variant & LQ) != 0) || r.big != ((variant & WS) != 0)) {
    ++failures;
    std::printf("backward (%d, %d) esz %zu batch %lld forms %#x: variant %d bytes %zu; want %d, %zu\n", n, m, esz, batch, forms, r.variant(), r.bytes, variant, bytes);
  }
}

// NEVER: no batch takes late Q unforced; ALWAYS: every batch does; else the last batch that does not
enum { NEVER = -1, ALWAYS = 0 };
static void threshold(int n, int m, size_t esz, long long last_without, size_t lds4, size_t lds3) {
  const long long probe[] = {1, 5, 144, 256, 257, 512, 513, 768, 769, 1024, 1025, 1536, 1537, 1792, 1793, 2048, 2049, 2304, 2305, 2816, 2817, 3072, 3073, 4096, 65536, 1 << 20};
  for (long long b : probe) {
    const bool late = last_without == ALWAYS || (last_without != NEVER && b > last_without);
    backward(n, m, esz, b, 0u, late ? LQ : 0, late ? lds3 : lds4);
  }
  if (last_without > 0) {   // the two batches on either side of the rule
    backward(n, m, esz, last_without, 0u, 0, lds4);
    backward(n, m, esz, last_without + 1, 0u, LQ, lds3);
  }
  // forced: late Q wherever the three-block carve fits 64 KB, never with _OFF; both bits together (a solve's options on top of the
  // handle's: altro_hip_set_forms itself refuses the pair) are _ON
  for (long long b : {1LL, 5LL, 4096LL}) {
    backward(n, m, esz, b, ON, LQ, lds3);
    backward(n, m, esz, b, ON | OFF, LQ, lds3);
    backward(n, m, esz, b, OFF, lds4 > 65536 ? WS : 0, lds4);
  }
}
static void global_ws(int n, int m, size_t esz, size_t lds4) {   // neither carve fits: the work block in global memory whatever is asked
  for (long long b : {1LL, 3LL, 769LL, 4096LL})
    for (unsigned f : {0u, ON, OFF, ON | OFF}) backward(n, m, esz, b, f, WS, lds4);
}

static void forward(int n, int m, int want_y, size_t esz, size_t limit, int variant, size_t bytes) {
  const GenericForwardRoute r = generic_forward_route(n, m, want_y, esz, limit);
  if (r.variant() != variant || r.bytes != bytes) {
    ++failures;
    std::printf("forward (%d, %d) y %d esz %zu limit %zu: variant %d bytes %zu; want %d, %zu\n", n, m, want_y, esz, limit, r.variant(), r.bytes, variant, bytes);
  }
}

int main() {
  // carve sizes
  if (generic_backward_lds_bytes(24, 8, 8) != 26816 || generic_backward_lds_bytes(24, 8, 8, true) != 22208 ||
      generic_backward_lds_bytes(12, 4, 4) != 3552 || generic_backward_lds_bytes(12, 4, 4, true) != 2976 || generic_backward_per_cu(26816) != 6 ||
      generic_backward_per_cu(22208) != 7 || generic_backward_per_cu(376) != 16 || generic_backward_per_cu(170944) != 0) {
    ++failures;
    std::printf("carve sizes\n");
  }
  // shape, element size, last batch without late Q, four-block carve, three-block carve
  threshold(2, 1, 8, NEVER, 376, 344);
  threshold(7, 3, 8, NEVER, 2800, 2408);
  threshold(9, 6, 8, NEVER, 5464, 4816);
  threshold(12, 4, 8, NEVER, 7040, 5888);
  threshold(13, 4, 8, NEVER, 8008, 6656);
  threshold(14, 5, 8, NEVER, 9656, 8088);
  threshold(12, 4, 4, NEVER, 3552, 2976);
  threshold(13, 4, 4, NEVER, 4036, 3360);
  threshold(14, 5, 4, NEVER, 4860, 4076);
  threshold(16, 8, 8, 2816, 14208, 12160);
  threshold(16, 8, 4, NEVER, 7136, 6112);
  threshold(17, 5, 8, 3072, 13232, 10920);
  threshold(17, 5, 4, NEVER, 6648, 5492);
  threshold(20, 8, 8, 2048, 20000, 16800);
  threshold(20, 8, 4, NEVER, 10032, 8432);
  threshold(24, 8, 8, 1536, 26816, 22208);
  threshold(24, 8, 4, 3072, 13440, 11136);
  threshold(31, 1, 8, 1024, 33088, 25400);
  threshold(31, 1, 4, 2304, 16576, 12732);
  threshold(33, 7, 8, 768, 44576, 35864);
  threshold(33, 7, 4, 1792, 22320, 17964);
  threshold(40, 10, 8, ALWAYS, 67504, 54704);
  threshold(40, 10, 4, 1024, 33784, 27384);
  threshold(40, 6, 8, 512, 61264, 48464);
  threshold(62, 4, 4, ALWAYS, 66952, 51576);
  threshold(32, 32, 4, 768, 42048, 37952);
  global_ws(62, 4, 8, 133840);
  global_ws(32, 32, 8, 84032);
  global_ws(50, 4, 8, 88816);
  global_ws(64, 16, 8, 170944);
  global_ws(64, 16, 4, 85504);
  // the drop-in's call (one problem, no forms): late Q only where the four-block carve does not fit
  backward(40, 10, 8, 1, 0u, LQ, 54704);
  backward(40, 6, 8, 1, 0u, 0, 61264);
  backward(20, 8, 8, 1, 0u, 0, 20000);
  backward(50, 4, 8, 1, 0u, WS, 88816);

  // forward sweep, 3 n + m + n^2 + 2 n m + n + m (+ n^2 + n with y) elements + 64 bytes staged, 2 n + m elements + 64 bytes unstaged.
  // A batch stages up to 10 KB a problem: (13, 4) 515 el -> 4184 B and (20, 8) 1236 el -> 9952 B staged; (24, 8) 1672 el -> 13440 B not
  forward(13, 4, 1, 8, kGenericForwardStageLimit, ST, 4184);
  forward(7, 3, 1, 8, kGenericForwardStageLimit, ST, 1512);
  forward(20, 8, 1, 8, kGenericForwardStageLimit, ST, 9952);
  forward(24, 8, 1, 8, kGenericForwardStageLimit, 0, 512);
  forward(24, 8, 1, 4, kGenericForwardStageLimit, ST, 6752);
  forward(64, 16, 1, 4, kGenericForwardStageLimit, 0, 640);
  forward(64, 16, 1, 8, kGenericForwardStageLimit, 0, 1216);
  // the drop-in stages whatever fits 64 KB: (24, 8) and (40, 6) with y (3892 el -> 31200 B) staged, (64, 16) 84800 B not; without y less
  forward(24, 8, 1, 8, kGenericLdsLimit, ST, 13440);
  forward(24, 8, 0, 8, kGenericLdsLimit, ST, 8640);
  forward(40, 6, 1, 8, kGenericLdsLimit, ST, 31200);
  forward(64, 16, 1, 8, kGenericLdsLimit, 0, 1216);
  forward(64, 16, 0, 8, kGenericLdsLimit, ST, 51520);

  if (failures) {
    std::printf("sweep_route_test: %d failures\n", failures);
    return 1;
  }
  std::printf("sweep_route_test ok\n");
  return 0;
}
