// loop_fields.h -- where each field of the iLQR loop lives on each plan: the one place the host code of the C ABI (capi_core.hip,
// capi_ilqr.hip) reads a record offset from.  Plain C++, no HIP: tests/cpp/loop_fields_test.cpp checks the table with g++ against
// offsets written out by hand from the record pictures (kernels/mfma16_layout.h, kernels/ilqr_lane.hip).
//
//   plan LANE    [k][element][batch] records: cand x | y | u, nom x | u, cost Qd | Rd | q | r | c or Q | R | H | q | r | c (dense)
//   plan MFMA16  [k][b][record]: XUY, NOM, COSTP (diagonal cost) or the dense cost's COST-layout records + q_N in its TERM record
//   plan GENERIC [b][k][block] arrays, one per field; per-knot-point dimensions pack the blocks of a problem back to back
#pragma once
#include <cstdint>

#include "altro_hip/altro_hip.h"
#if !defined(__HIPCC__) && !defined(__host__)   // (the layout header marks its constexpr functions for both sides)
#define __host__
#define __device__
#endif
#include "kernels/mfma16_layout.h"

namespace altro_hip {
namespace capi {

struct LoopShape {
  int plan;                      // ALTRO_HIP_PLAN_LANE / _MFMA16 / _GENERIC
  bool ragged, cost_dense;
  int n, m, N;
  int64_t batch;
  int64_t xuy_bs, xuy_ks;        // Mfma16Strides of the candidate records
  const int *nxv, *nuv;          // ragged: nx[0..N], nu[0..N-1]
};

enum LoopField {
  LF_CAND_X, LF_CAND_U, LF_NOM_X, LF_NOM_U,
  LF_COST_q, LF_COST_r, LF_COST_c,            // at k = N: the terminal q_N, c_N
  LF_COST_Qd, LF_COST_Rd,                     // the diagonal cost (altro_hip_set_tracking_cost on plans LANE / MFMA16)
  LF_COST_Q, LF_COST_R, LF_COST_H,            // the dense cost (plan LANE's records, plan GENERIC's arrays)
  LF_NUM
};
// the handle's buffers (capi_internal.h: loop_buffer turns the id into the pointer)
enum LoopBuf {
  LB_NONE,   // the field does not exist there: no input at k = N, no Qd on a dense cost, ...
  LB_G_X, LB_G_U, LB_G_XN, LB_G_UN, LB_G_CQ, LB_G_CR, LB_G_CH, LB_G_Cq, LB_G_Cr, LB_G_Cc,
  LB_M_XUY, LB_M_NOM, LB_M_COSTP, LB_M_COSTD, LB_M_COSTD_TERM,
  LB_L_XUY, LB_L_NOM, LB_L_COST, LB_L_COSTQ,
  LB_M_IN, LB_L_IN, LB_G_A, LB_G_B, LB_G_F   // the dynamics given as data (shift_fields.h)
};
enum LoopKind { LK_AOS, LK_LANE };

// Field of knot point k.  LK_AOS: element e of problem b is buf[off + b * bs + e], the same field of knot point k + j sits j * ks
// further (as long as it stays in the same buffer: loop_field_run).  LK_LANE: buf[((k * E + off + e) * batch + b], ks = E * batch.
struct FieldRef {
  int buf, kind;
  int64_t off, bs, ks;
  int E;      // LK_LANE: elements of one record
  int len;    // elements of the field
};

inline FieldRef loop_field(const LoopShape& s, int field, int k) {
  const int n = s.n, m = s.m, N = s.N;
  const FieldRef none{LB_NONE, LK_AOS, 0, 0, 0, 0, 0};
  const bool is_u = field == LF_CAND_U || field == LF_NOM_U || field == LF_COST_r || field == LF_COST_Rd || field == LF_COST_R || field == LF_COST_H;
  if (k < 0 || k > N || (is_u && k == N)) return none;
  const bool diag_only = field == LF_COST_Qd || field == LF_COST_Rd, dense_only = field == LF_COST_Q || field == LF_COST_R || field == LF_COST_H;

  if (s.plan == ALTRO_HIP_PLAN_LANE) {
    if (s.cost_dense ? diag_only : dense_only) return none;
    const int oq = s.cost_dense ? n * n + m * m + m * n : n + m;   // q | r | c close both cost records
    const int e_cost = oq + n + m + 1;
    auto lane = [&](int buf, int E, int off, int len) { return FieldRef{buf, LK_LANE, off, 1, (int64_t)E * s.batch, E, len}; };
    const int cost = s.cost_dense ? LB_L_COSTQ : LB_L_COST;
    switch (field) {
      case LF_CAND_X: return lane(LB_L_XUY, 2 * n + m, 0, n);
      case LF_CAND_U: return lane(LB_L_XUY, 2 * n + m, 2 * n, m);
      case LF_NOM_X: return lane(LB_L_NOM, n + m, 0, n);
      case LF_NOM_U: return lane(LB_L_NOM, n + m, n, m);
      case LF_COST_q: return lane(cost, e_cost, oq, n);
      case LF_COST_r: return lane(cost, e_cost, oq + n, m);
      case LF_COST_c: return lane(cost, e_cost, oq + n + m, 1);
      case LF_COST_Qd: return lane(cost, e_cost, 0, n);
      case LF_COST_Rd: return lane(cost, e_cost, n, m);
      case LF_COST_Q: return lane(cost, e_cost, 0, n * n);
      case LF_COST_R: return lane(cost, e_cost, n * n, m * m);
      case LF_COST_H: return lane(cost, e_cost, n * n + m * m, m * n);
    }
    return none;
  }

  if (s.plan == ALTRO_HIP_PLAN_MFMA16) {   // knot-point-major slabs: record (k, b) at (k * batch + b) * record length
    auto slab = [&](int buf, int rec, int off, int len) { return FieldRef{buf, LK_AOS, (int64_t)k * s.batch * rec + off, rec, s.batch * rec, 0, len}; };
    switch (field) {
      case LF_CAND_X: return FieldRef{LB_M_XUY, LK_AOS, k * s.xuy_ks + MF_XUY_X, s.xuy_bs, s.xuy_ks, 0, n};
      case LF_CAND_U: return FieldRef{LB_M_XUY, LK_AOS, k * s.xuy_ks + MF_XUY_U, s.xuy_bs, s.xuy_ks, 0, m};
      case LF_NOM_X: return slab(LB_M_NOM, MF_NOM, MF_NOM_X, n);
      case LF_NOM_U: return slab(LB_M_NOM, MF_NOM, MF_NOM_U, m);
    }
    if (!s.cost_dense) switch (field) {
      case LF_COST_Qd: return slab(LB_M_COSTP, MF_COSTP, MF_COSTP_QD, n);
      case LF_COST_Rd: return slab(LB_M_COSTP, MF_COSTP, MF_COSTP_RD, m);
      case LF_COST_q: return slab(LB_M_COSTP, MF_COSTP, MF_COSTP_q, n);
      case LF_COST_r: return slab(LB_M_COSTP, MF_COSTP, MF_COSTP_r, m);
      case LF_COST_c: return slab(LB_M_COSTP, MF_COSTP, MF_COSTP_c, 1);
    }
    else switch (field) {   // the dense cost's own COST-layout records ([q r] slot, c in the first pad slot); its Q / R / H go through pack.hip
      case LF_COST_q: return k < N ? slab(LB_M_COSTD, MF_COST, MF_OFF_QR, n) : FieldRef{LB_M_COSTD_TERM, LK_AOS, MF_TERM_q, MF_TERM, 0, 0, n};
      case LF_COST_r: return slab(LB_M_COSTD, MF_COST, MF_OFF_QR + MF_N, m);
      case LF_COST_c: return slab(LB_M_COSTD, MF_COST, MF_COSTD_C, 1);
    }
    return none;
  }

  // plan GENERIC: the dense cost only; one array per field, [b][k][block] -- per-knot-point dimensions: the blocks back to back
  if (diag_only) return none;
  const bool ux = field == LF_CAND_U || field == LF_NOM_U || field == LF_COST_r || field == LF_COST_R;   // sized by the inputs alone
  auto block = [&](int j) -> int64_t {
    const int64_t nj = s.ragged ? s.nxv[j] : n, mj = j < N ? (s.ragged ? s.nuv[j] : m) : 0;
    switch (field) {
      case LF_COST_Q: return nj * nj;
      case LF_COST_R: return mj * mj;
      case LF_COST_H: return mj * nj;
      case LF_COST_c: return 1;
      default: return ux ? mj : nj;
    }
  };
  int64_t off = 0, total = 0;
  for (int j = 0; j <= N; ++j) { if (j < k) off += block(j); total += block(j); }
  int buf = LB_NONE;
  switch (field) {
    case LF_CAND_X: buf = LB_G_X; break;
    case LF_CAND_U: buf = LB_G_U; break;
    case LF_NOM_X: buf = LB_G_XN; break;
    case LF_NOM_U: buf = LB_G_UN; break;
    case LF_COST_q: buf = LB_G_Cq; break;
    case LF_COST_r: buf = LB_G_Cr; break;
    case LF_COST_c: buf = LB_G_Cc; break;
    case LF_COST_Q: buf = LB_G_CQ; break;
    case LF_COST_R: buf = LB_G_CR; break;
    case LF_COST_H: buf = LB_G_CH; break;
  }
  return FieldRef{buf, LK_AOS, off, total, block(k), 0, (int)block(k)};
}

// how many of the knot points k0 .. k1 the reference of k0 strides over: the run ends where the field moves to another buffer
inline int loop_field_run(const LoopShape& s, int field, int k0, int k1) {
  const int buf = loop_field(s, field, k0).buf;
  int k = k0 + 1;
  while (k <= k1 && loop_field(s, field, k).buf == buf) ++k;
  return k - k0;
}

}  // namespace capi
}  // namespace altro_hip
