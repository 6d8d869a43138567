// shift_fields.h -- what the receding-horizon shifts of the problem DATA move (altro_hip_shift_dynamics, altro_hip_shift_linear_costs),
// said in loop_fields.h's terms: where the dynamics given as data live on each plan, which of the cost's fields are the linear terms, and
// how one such field is walked by kernels/shift_field.hip.  Plain C++, no HIP: tests/cpp/shift_fields_test.cpp checks it with g++ against
// offsets written out by hand from the record pictures (kernels/mfma16_layout.h, lane_sizes).
//
//   plan MFMA16   the whole DYN record (Z 192 | f 12) of the [k][b][record] slab m_in, at Mfma16Strides::in_bs / in_ks
//   plan LANE     the A | B | f elements that open the l_in record ([k][element][batch]); the sweep's cost blocks follow them there
//   plan GENERIC  the arrays G_A, G_B, G_f, [b][k][block] (plan MFMA32 runs on the same arrays)
#pragma once
#include <cstdint>

#include "loop_fields.h"

namespace altro_hip {
namespace capi {

struct DynShape {
  int plan;                // ALTRO_HIP_PLAN_LANE / _MFMA16 / _GENERIC
  int n, m, N;
  int64_t batch;
  int64_t in_bs, in_ks;    // Mfma16Strides of the DYN records
};

// The dynamics of knot point k as fields, A | B | f in this order where they are fields of their own: one on plans MFMA16 and LANE (the
// three lie back to back), three on plan GENERIC.  Returns how many of out[0..2] it filled; 0 outside 0 .. N-1.
inline int dyn_fields(const DynShape& s, int k, FieldRef out[3]) {
  const int n = s.n, m = s.m;
  if (k < 0 || k >= s.N) return 0;
  if (s.plan == ALTRO_HIP_PLAN_MFMA16) {
    out[0] = FieldRef{LB_M_IN, LK_AOS, k * s.in_ks, s.in_bs, s.in_ks, 0, MF_DYN};
    return 1;
  }
  if (s.plan == ALTRO_HIP_PLAN_LANE) {
    const int e_in = 2 * n * n + 2 * n * m + m * m + 2 * n + m;   // A | B | f | Q | R | H | q | r (lane_sizes)
    out[0] = FieldRef{LB_L_IN, LK_LANE, 0, 1, (int64_t)e_in * s.batch, e_in, n * n + n * m + n};
    return 1;
  }
  const int blk[3] = {n * n, n * m, n};
  const int buf[3] = {LB_G_A, LB_G_B, LB_G_F};
  for (int i = 0; i < 3; ++i) out[i] = FieldRef{buf[i], LK_AOS, (int64_t)k * blk[i], (int64_t)s.N * blk[i], blk[i], 0, blk[i]};
  return 3;
}

// The fields altro_hip_update_linear_costs writes, at knot point 0: q | r | c of the cost form in effect.  Neighbours in one record are
// joined into one field (LANE always; the tile's COSTP record at the full (12, 4) shape), so that each is one launch.  Returns the count.
inline int linear_cost_fields(const LoopShape& s, FieldRef out[3]) {
  int count = 0;
  for (int f : {LF_COST_q, LF_COST_r, LF_COST_c}) {
    const FieldRef r = loop_field(s, f, 0);
    if (r.buf == LB_NONE || r.len <= 0) continue;
    if (count > 0) {
      FieldRef& p = out[count - 1];
      if (p.buf == r.buf && p.kind == r.kind && p.bs == r.bs && p.ks == r.ks && p.E == r.E && p.off + p.len == r.off) { p.len += r.len; continue; }
    }
    out[count++] = r;
  }
  return count;
}

// One field as the shift kernel walks it: element e < run of row r < rows at knot point k is base[first + r * rs + k * ks + e].
//   LK_AOS   rows = batch records, run = len, rs = bs; a slab's records that lie back to back (bs == len) are ONE row of batch * len elements
//   LK_LANE  one row: the field's len rows of `batch` problems are contiguous, run = len * batch
// vec: elements per access -- 16 bytes' worth where first, run, rs and ks are all multiples of that (the buffers themselves are aligned
// far beyond 16 bytes), else 1.
struct ShiftRun {
  int64_t first, rows, run, rs, ks;
  int K;      // knot points of the walk: k = 0 .. K-2 take what k + 1 held, K-1 keeps its values
  int vec;
  bool ok;    // shift_run_safe held
};

// A thread owns one (row, element) column and walks k ascending in place, reading k + 1 before it writes k.  No thread reads what another
// writes iff (row, k, element) -> address is one to one over the walk: a knot point's run must not reach into the next one's
// (run <= ks), and rows must not reach into each other -- either a row's whole walk fits inside the row stride (problem-major arrays)
// or all rows of a knot point fit inside the knot-point stride (knot-point-major slabs).
inline bool shift_run_safe(const ShiftRun& r) {
  if (r.rows < 1 || r.run < 1 || r.K < 1 || r.first < 0) return false;
  if (r.K > 1 && r.run > r.ks) return false;
  if (r.rows == 1) return true;
  const int64_t walk = (int64_t)(r.K - 1) * r.ks + r.run, slab = (r.rows - 1) * r.rs + r.run;
  return r.rs >= r.run && (walk <= r.rs || r.K == 1 || slab <= r.ks);
}

inline ShiftRun shift_run(const FieldRef& f, int64_t batch, int K, int esz) {
  ShiftRun r{};
  if (f.kind == LK_LANE) {
    r.first = f.off * batch; r.rows = 1; r.run = (int64_t)f.len * batch; r.rs = 0; r.ks = f.ks;
  } else if (f.bs == f.len && f.ks >= (int64_t)f.len * batch) {
    r.first = f.off; r.rows = 1; r.run = (int64_t)f.len * batch; r.rs = 0; r.ks = f.ks;
  } else {
    r.first = f.off; r.rows = batch; r.run = f.len; r.rs = f.bs; r.ks = f.ks;
  }
  r.K = K;
  const int v = 16 / esz;
  r.vec = (r.first % v == 0 && r.run % v == 0 && r.rs % v == 0 && r.ks % v == 0) ? v : 1;
  r.ok = shift_run_safe(r);
  return r;
}

}  // namespace capi
}  // namespace altro_hip
