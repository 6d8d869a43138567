// al_tables.h -- what the constraint tables contain: everything al_upload (capi_ilqr.hip) puts on the device for a handle's augmented-
// Lagrangian constraint blocks and every value it derives from them, built by one host function from the host description of the blocks;
// the slot rule of plan MFMA16 and the capacities of every plan (al_admit).  Plain C++, no HIP call, no handle:
// tests/cpp/al_tables_test.cpp checks the tables with g++ against recordings of the function this one replaced, against entries written
// out by hand from the layout comments of kernels/al_types.h, and every capacity at its limit.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "altro_hip/altro_hip.h"
#include "kernels/al_types.h"
#include "kernels/mfma16_layout.h"

namespace altro_hip {
namespace capi {

// the host description of a handle's blocks (altro_hip_batch: al_defs, al_knots, al_G, al_g) and the plain values the tables depend on
struct AlInput {
  int plan, n, m, N, batch;
  size_t esz;                                   // element size on the device
  bool ragged;
  const std::vector<int>&nxv, &nuv;             // ragged: nx[0..N], nu[0..N-1]
  const std::vector<AlDef>& defs;
  const std::vector<AlKnotBig>& knots;          // [N + 1]: ncon and def[] of every knot point
  const std::vector<double>& G;                 // pool of G blocks, column-major p x w as given
  const std::vector<std::vector<double>>& g;    // per block: [p] or [batch][p]; with AlDef::g_per_knot [K][p] or [batch][K][p]
};

// what the kernels' launchers and the solve loop read about the tables as a whole (AlTable's scalar members among them); the default is
// the handle without blocks
struct AlSummary {
  int all_sel = 0;          // every block is bound-type (rows +-e_idx: AlKnot::sel)
  bool all_gsel = false;    // plan GENERIC: every block is bound-type (the Hessian blocks change on their diagonals only)
  bool row32_ok = false;    // every block fits kernels/ilqr_row32.hip (row-wise cone, <= 32 rows)
  int has_soc = 0;          // some block is a second-order cone
  bool has_user = false;    // some block comes from the caller's source (AlDef::user)
  int max_ncon = 0;         // most blocks (plan MFMA16: slots) any knot point has
  int uniform = 0, rows_per_knot = 0;   // knot points 0..N-1 carry the same blocks (kernels/al_types.h)
  int G_count = 0, Gpad_count = 0;      // elements of the device G and Gpad pools
};

enum AlBuildError {
  AL_BUILD_OK = 0,
  AL_BUILD_SLOTS,    // knot point err_k has more slots than the plan's table holds
  AL_BUILD_WINDOW    // plan LANE: rows x batch x esz reaches the 2 GiB buffer window
};
struct AlTables {
  std::vector<double> G, Gpad, g;   // the value pools; the element type is applied at upload (al_pool_as)
  std::vector<AlKnot> knots;        // [N + 1] (plans LANE, MFMA16; empty on plan GENERIC)
  std::vector<AlKnotBig> big;       // [N + 1] completed (plan GENERIC's device table, the host's record on every plan)
  std::vector<int> gsel, guser;     // AlTable::gsel (uniform plan GENERIC), AlTable::guser (... with a block from source); else empty
  std::vector<AlDef> defs;          // the blocks as given, g_off filled in: where each one's segment of the g pool starts
  int rows = 0;                     // dual rows of one problem
  AlSummary sum;
  int error = AL_BUILD_OK, err_k = -1;
};

// a value pool in the device's element type ((float) of a double is the same float wherever it is taken; zeros stay zeros)
template <typename T>
std::vector<T> al_pool_as(const std::vector<double>& pool) { return std::vector<T>(pool.begin(), pool.end()); }

// Plan MFMA16 lays a block out over SLOTS of at most AL_MAXP rows (al_types.h: AL_TILE_MAXC): rows 8 s .. 8 s + 7 of a block in the
// zero / identity / orthant cones are a block of their own (those cones project row by row, cones.cpp:13-38) with the same duals
// in the same place; a second-order-cone block (p <= AL_MAXSOC) is one slot.  The other plans: one entry per block.
inline int al_slots(bool tile, int cone, int p) { return (tile && cone != CONE_SOC) ? (p + AL_MAXP - 1) / AL_MAXP : 1; }
// ... and the rows of slot sl
inline int al_slot_rows(bool tile, int cone, int p, int sl) { return (tile && cone != CONE_SOC) ? std::min(p - sl * AL_MAXP, AL_MAXP) : p; }

// Is row r of block d's G (as the caller gave it: p x w, column-major) +e_idx or -e_idx?  idx and sign are those of the row's only
// nonzero, whatever its size (the tables record them for a multiple of e_idx too, which is no bound row); idx < 0: not exactly one.
inline bool al_bound_row(const std::vector<double>& G, const AlDef& d, int r, int w, int& idx, int& sign) {
  int nz = 0; bool unit = true;
  for (int e = 0; e < w; ++e) {
    const double v = G[(size_t)d.G_off + r + (size_t)e * d.p];
    if (v != 0.0) { ++nz; idx = e; sign = v > 0 ? 1 : -1; unit = unit && (v == 1.0 || v == -1.0); }
  }
  if (nz != 1) idx = -1;
  return unit && nz == 1;
}

inline AlTables al_build(const AlInput& in) {
  AlTables t;
  if (in.defs.empty()) return t;
  const size_t nd = in.defs.size();
  const int64_t B = in.batch;
  const bool tile = in.plan == ALTRO_HIP_PLAN_MFMA16, gen = in.plan == ALTRO_HIP_PLAN_GENERIC;
  // G on the device: p x (n + m) column-major as given on plan LANE; on plan MFMA16 p x 16 in the tile's own column order
  // (states in columns 0..11, inputs in 12..15), so that a padded shape's blocks address the padded [x; u] correctly
  const int w_log = in.n + in.m, w_dev = tile ? MF_N + MF_M : w_log;
  auto dev_col = [&](int e) { return (tile && e >= in.n) ? MF_N + (e - in.n) : e; };
  auto nslots = [&](const AlDef& d) { return al_slots(tile, d.cone, d.p); };
  // slot_base[i]: first slot definition of block i, and gp_base[i] its first entry in the zero-padded pool Gpad (AL_TILE_MAXSLOTDEF of
  // them): a block from the caller's source has none -- its Jacobian is evaluated at every point (kernels/ilqr_merit2_dpp.hip,
  // MD_USER_BLOCKS)
  std::vector<int> slot_base(nd + 1, 0), gp_base(nd + 1, 0);
  for (size_t i = 0; i < nd; ++i) {
    slot_base[i + 1] = slot_base[i] + nslots(in.defs[i]);
    gp_base[i + 1] = gp_base[i] + (in.defs[i].user ? 0 : nslots(in.defs[i]));
  }
  // the G pool: per block (plan MFMA16: per slot, every slot its own ps x 16 column-major matrix -- the LDS-form kernels address a slot
  // like a block); with per-knot-point dimensions (plan GENERIC) the block as given, p x (nx[k] + nu[k]) of its knot points
  std::vector<int> G_off_dev((size_t)slot_base.back(), 0);   // per slot definition
  for (size_t i = 0; i < nd; ++i) {
    const AlDef& d = in.defs[i];
    for (int sl = 0; sl < nslots(d); ++sl) {
      const int r0 = sl * AL_MAXP, ps = al_slot_rows(tile, d.cone, d.p, sl);
      const size_t off = t.G.size();
      G_off_dev[(size_t)slot_base[i] + sl] = (int)off;
      if (in.ragged) {
        t.G.insert(t.G.end(), in.G.begin() + d.G_off, in.G.begin() + d.G_off + (size_t)d.p * d.w);
        continue;
      }
      t.G.resize(off + (size_t)ps * w_dev, 0.0);
      for (int e = 0; e < w_log; ++e)
        for (int r = 0; r < ps; ++r) t.G[off + r + (size_t)dev_col(e) * ps] = in.G[(size_t)d.G_off + (r0 + r) + (size_t)e * d.p];
    }
  }
  if (tile) {   // the same slots zero-padded for the row-layout kernels (al_types.h: AL_GP_DEF)
    t.Gpad.assign((size_t)gp_base.back() * (size_t)AL_GP_DEF, 0.0);
    for (size_t i = 0; i < nd; ++i) {
      const AlDef& d = in.defs[i];
      if (d.user) continue;
      for (int e = 0; e < w_log; ++e)
        for (int r = 0; r < d.p; ++r)
          t.Gpad[(size_t)(gp_base[i] + r / AL_MAXP) * AL_GP_DEF + (size_t)(r % AL_MAXP) * AL_GP_LD + dev_col(e)] = in.G[(size_t)d.G_off + r + (size_t)e * d.p];
    }
  }
  // the g pool: [p] shared, or [p][batch]; a block with g_per_knot has one such run per knot point of its range, [K][p] or [K][p][batch]
  // (al_types.h: al_g_index), given as [K][p] or [batch][K][p]
  std::vector<AlDef> defs = in.defs;
  for (size_t i = 0; i < nd; ++i) {
    defs[i].g_off = (int64_t)t.g.size();
    const AlDef& d = defs[i];
    const std::vector<double>& src = in.g[i];
    const int p = d.p;
    const int K = d.g_per_knot ? (int)(src.size() / ((size_t)p * (d.g_per_problem ? B : 1))) : 1;
    t.g.resize(t.g.size() + (size_t)K * p * (d.g_per_problem ? B : 1));
    for (int64_t b = 0; b < (d.g_per_problem ? B : 1); ++b)
      for (int kk = 0; kk < K; ++kk)
        for (int r = 0; r < p; ++r) t.g[(size_t)al_g_index(d, B, b, d.k_first + kk, r)] = src[((size_t)b * K + kk) * p + r];
  }
  t.defs = defs;
  // the knot points' records
  t.big = in.knots;
  t.knots.assign(gen ? 0 : t.big.size(), AlKnot{});
  int rows = 0;
  for (size_t k = 0; k < t.big.size(); ++k) {
    AlKnotBig& bk = t.big[k];
    int ns = 0;   // slots of knot point k so far (plan LANE: one per block)
    for (int j = 0; j < bk.ncon; ++j) {
      const AlDef& d = defs[bk.def[j]];
      const int s0 = slot_base[bk.def[j]];
      bk.z_off[j] = rows; rows += d.p;
      bk.cone[j] = d.cone; bk.p[j] = d.p; bk.g_per_problem[j] = d.g_per_problem; bk.G_off[j] = G_off_dev[s0];
      bk.g_off[j] = al_g_index(d, B, 0, (int)k, 0);   // this knot point's run of the block's segment
      if (gen) continue;
      AlKnot& kn = t.knots[k];
      for (int sl = 0; sl < nslots(d); ++sl, ++ns) {
        if (ns >= (tile ? AL_TILE_MAXC : AL_MAXC)) { t.error = AL_BUILD_SLOTS; t.err_k = (int)k; return t; }   // (al_admit counted the slots: not reached)
        const int r0 = sl * AL_MAXP, ps = al_slot_rows(tile, d.cone, d.p, sl);
        kn.def[ns] = bk.def[j];
        kn.z_off[ns] = bk.z_off[j] + r0;
        kn.cone[ns] = d.cone; kn.p[ns] = ps; kn.g_per_problem[ns] = d.g_per_problem;
        kn.G_off[ns] = G_off_dev[(size_t)s0 + sl];
        kn.g_off[ns] = al_g_index(d, B, 0, (int)k, r0);   // g is [p] or [p][batch] (per knot point with g_per_knot): row r0 on
        kn.user[ns] = d.user;
        kn.Gp_off[ns] = (tile && !d.user) ? (gp_base[bk.def[j]] + sl) * AL_GP_DEF : 0;
        // bound-type slot: every row of G is +-e_idx
        bool sel = d.cone != CONE_SOC;
        for (int r = 0, at, sg; r < ps && sel; ++r) {
          sel = al_bound_row(in.G, d, r0 + r, w_log, at, sg);
          if (at >= 0) kn.sidx[ns][r] = sg * (dev_col(at) + 1);
        }
        kn.sel[ns] = sel ? 1 : 0;
      }
      kn.ncon = ns;
    }
    t.sum.max_ncon = std::max(t.sum.max_ncon, gen ? bk.ncon : ns);
  }
  t.rows = rows;
  if (in.plan == ALTRO_HIP_PLAN_LANE && (uint64_t)rows * (uint64_t)B * in.esz >= (1ull << 31)) { t.error = AL_BUILD_WINDOW; return t; }
  t.sum.all_gsel = gen && !in.ragged;
  if (gen && !in.ragged) {   // plan GENERIC: which blocks are bound-type (AlTable::gsel; the expansion's Gauss-Newton term is then diagonal)
    t.gsel.assign(nd * (size_t)(1 + GEN_MAXP), 0);
    for (size_t i = 0; i < nd; ++i) {
      const AlDef& d = defs[i];
      bool sel = d.cone != CONE_SOC && !d.user && d.p <= GEN_MAXP;
      for (int r = 0, at, sg; r < d.p && sel; ++r) {
        sel = al_bound_row(in.G, d, r, w_log, at, sg);
        if (at >= 0) t.gsel[i * (size_t)(1 + GEN_MAXP) + 1 + r] = sg * (at + 1);
      }
      t.gsel[i * (size_t)(1 + GEN_MAXP)] = sel ? 1 : 0;
      if (!sel) t.sum.all_gsel = false;
    }
    // blocks from the caller's source (AlTable::guser): only the run-time compiled kernels read the table, and only a handle with
    // such a block has one
    for (const AlDef& d : defs)
      if (d.user) { t.guser.resize(nd); for (size_t i = 0; i < nd; ++i) t.guser[i] = defs[i].user; break; }
  }
  t.sum.row32_ok = true;   // (kernels/ilqr_row32.hip: a lane position per row, the row-wise cones)
  for (const AlDef& d : defs) {
    if (d.cone == CONE_SOC || d.p > 32 || d.user) t.sum.row32_ok = false;
    if (d.cone == CONE_SOC) t.sum.has_soc = 1;
    if (d.user) t.sum.has_user = true;
  }
  {   // uniform running knot points?  (then the dual rows of knot point k start k * rows_per_knot after those of 0)
    const AlKnotBig& k0 = t.big[0];
    int r0 = 0;
    for (int j = 0; j < k0.ncon; ++j) r0 += defs[k0.def[j]].p;
    bool uni = in.N >= 1 && k0.ncon > 0;
    for (int k = 1; k < in.N && uni; ++k) {
      uni = t.big[k].ncon == k0.ncon;
      for (int j = 0; j < k0.ncon && uni; ++j) uni = t.big[k].def[j] == k0.def[j] && t.big[k].z_off[j] == k0.z_off[j] + k * r0;
    }
    // a block with g_per_knot on a running knot point: every knot point reads its own record, whose g_off is its own
    for (int k = 0; k < in.N && uni; ++k)
      for (int j = 0; j < t.big[k].ncon && uni; ++j) uni = !defs[t.big[k].def[j]].g_per_knot;
    t.sum.uniform = uni ? 1 : 0;
    t.sum.rows_per_knot = r0;
  }
  t.sum.G_count = (int)t.G.size();
  t.sum.Gpad_count = (int)t.Gpad.size();
  t.sum.all_sel = gen ? 0 : 1;
  for (const AlKnot& kn : t.knots)
    for (int j = 0; j < kn.ncon; ++j) if (!kn.sel[j]) t.sum.all_sel = 0;
  return t;
}

// ---- capacities (stated in altro_hip.h): plan GENERIC loops over the blocks with one lane per row, plan LANE unrolls two blocks, plan
// MFMA16 lays the rows out over slots of eight (kernels/al_types.h: AL_TILE_MAXC).  Which limit, if any, does one more block of p rows
// in `cone` at knot points k_first .. k_last break (user != 0: a block from the caller's source), and with which numbers?
enum AlLimit {
  AL_ADMIT_OK = 0,
  // a block from source, before anything else is looked at (altro_hip_add_user_constraint)
  AL_LIMIT_USER_CONE,   // plan MFMA16: unknown cone
  AL_LIMIT_USER_ROWS,   // p outside [1, pmax]: one slot on plan MFMA16, GEN_USER_MAXROWS on plan GENERIC
  AL_LIMIT_USER_KNOT,   // knot point k would have `count` blocks (plan MFMA16) / rows (plan GENERIC) from source, more than cmax
  // any block
  AL_LIMIT_CONE,
  AL_LIMIT_ROWS,        // p outside [1, pmax]
  AL_LIMIT_RANGE,       // k_first .. k_last outside [0, N]
  AL_LIMIT_DEFS,        // more than dmax blocks (plan MFMA16: slots, blocks from source not counted) on the handle
  AL_LIMIT_KNOT,        // knot point k would have more than cmax blocks (plan MFMA16: `count` slots)
  AL_LIMIT_RAGGED       // knot point k differs from k_first in dimension: one block takes one [x; u] size
};
struct AlAdmit {
  int limit = AL_ADMIT_OK;
  int pmax = 0, cmax = 0, dmax = 0;   // of the stage that answered: rows per block, blocks / slots / rows per knot point, per handle
  int k = -1, count = 0;
  int w = 0;                          // admitted: columns of the block's G
};
inline AlAdmit al_admit(const AlInput& in, int k_first, int k_last, int cone, int p, int user) {
  const bool gen = in.plan == ALTRO_HIP_PLAN_GENERIC, tile = in.plan == ALTRO_HIP_PLAN_MFMA16;
  const bool cone_ok = cone >= CONE_EQUALITY && cone <= CONE_SOC;
  AlAdmit a;
  auto broken = [&a](int limit, int k = -1, int count = 0) { a.limit = limit; a.k = k; a.count = count; return a; };
  auto def_at = [&in](int k, int j) -> const AlDef& { return in.defs[in.knots[k].def[j]]; };
  if (user && (tile || gen)) {
    // plan MFMA16: one slot per block, AL_TILE_USER_MAXC such slots per knot point; plan GENERIC stages the user blocks' values and
    // Jacobians of a knot point in LDS, GEN_USER_MAXROWS rows (kernels/al_types.h)
    if (tile && !cone_ok) return broken(AL_LIMIT_USER_CONE);
    a.pmax = gen ? GEN_USER_MAXROWS : cone == CONE_SOC ? AL_MAXSOC : AL_MAXP;
    a.cmax = gen ? GEN_USER_MAXROWS : AL_TILE_USER_MAXC;
    if (p < 1 || p > a.pmax) return broken(AL_LIMIT_USER_ROWS);
    for (int k = std::max(k_first, 0); k <= std::min(k_last, in.N); ++k) {
      int count = gen ? p : 1;
      for (int j = 0; j < in.knots[k].ncon; ++j) if (def_at(k, j).user) count += gen ? def_at(k, j).p : 1;
      if (count > a.cmax) return broken(AL_LIMIT_USER_KNOT, k, count);
    }
  }
  if (!cone_ok) return broken(AL_LIMIT_CONE);
  const int tile_slots = in.esz == 8 ? AL_TILE_MAXC : AL_MAXC;   // (fp32 records: the two-slot kernels only)
  a.pmax = cone == CONE_SOC ? (gen ? GEN_MAXSOC : AL_MAXSOC) : (gen ? GEN_MAXP : tile ? tile_slots * AL_MAXP : AL_MAXP);
  a.cmax = gen ? GEN_MAXC : tile ? tile_slots : AL_MAXC;
  a.dmax = gen ? GEN_MAXDEF : tile ? AL_TILE_MAXSLOTDEF : AL_MAXDEF;
  if (p < 1 || p > a.pmax) return broken(AL_LIMIT_ROWS);
  if (k_first < 0 || k_last > in.N || k_first > k_last) return broken(AL_LIMIT_RANGE);
  if (tile) {   // slots: per handle and per knot point
    int defslots = user ? 0 : al_slots(true, cone, p);   // (a block from source has no entry in the padded pool: al_build's gp_base)
    for (const AlDef& d : in.defs) if (!d.user) defslots += al_slots(true, d.cone, d.p);
    if (defslots > a.dmax) return broken(AL_LIMIT_DEFS, -1, defslots);
    for (int k = k_first; k <= k_last; ++k) {
      int used = al_slots(true, cone, p);
      for (int j = 0; j < in.knots[k].ncon; ++j) used += al_slots(true, def_at(k, j).cone, def_at(k, j).p);
      if (used > a.cmax) return broken(AL_LIMIT_KNOT, k, used);
    }
  } else {
    if ((int)in.defs.size() >= a.dmax) return broken(AL_LIMIT_DEFS, -1, (int)in.defs.size() + 1);
    for (int k = k_first; k <= k_last; ++k)
      if (in.knots[k].ncon >= a.cmax) return broken(AL_LIMIT_KNOT, k, in.knots[k].ncon + 1);
  }
  a.w = in.n + in.m;
  if (in.ragged) {   // G is p x (nx[k] + nu[k]): every knot point of the range must have the dimensions of the first (the terminal one: its nx)
    const int nk = in.nxv[k_first], mk = k_first < in.N ? in.nuv[k_first] : 0;   // (a block of the terminal knot point alone: p x nx[N])
    for (int k = k_first; k <= k_last; ++k)
      if (in.nxv[k] != nk || (k < in.N && in.nuv[k] != mk)) return broken(AL_LIMIT_RAGGED, k);
    a.w = nk + mk;
  }
  return a;
}

}  // namespace capi
}  // namespace altro_hip
