// al_shift.h -- the chains altro_hip_shift_duals walks (kernels/al_shift.hip): for every dual row of one problem the row that holds the
// same (block definition, row in block) one knot point later, built from the completed knot-point records of al_tables.h.  The duals of a
// handle are one array z[rows][batch] on every plan, a block's rows start at AlKnotBig::z_off, and plan MFMA16's slots are consecutive rows
// of their block (al_tables.h: al_slots), so one table serves every plan.  Plain C++, no HIP call, no handle: tests/cpp/al_shift_test.cpp
// checks it with g++ against tables written out by hand.
#pragma once
#include <cassert>
#include <vector>

#include "kernels/al_types.h"

namespace altro_hip {
namespace capi {

// entries of zero behind AlShift::order: the kernel fetches the rows of two groups of links ahead of the one it stores without asking
// where a chain ends (kernels/al_shift.hip: AL_SHIFT_DEPTH is at most 32)
constexpr int AL_SHIFT_PAD = 72;

struct AlShift {
  std::vector<int> next;    // [rows]: the row of the same (definition, row in block) at k + 1, or -1 where the definition ends
  std::vector<int> heads;   // the rows nothing points to, ascending: one per chain (a block present at one knot point only is a chain of one)
  // what the device gets: the chains written out one after the other in walking order -- chain c is order[start[c] .. start[c + 1]),
  // order[i + 1] == next[order[i]] inside it -- so that the kernel reads its rows as runs of one array instead of chasing next[]
  // from load to load; AL_SHIFT_PAD zeros follow the last chain
  std::vector<int> order, start;   // [rows + AL_SHIFT_PAD], [heads.size() + 1]
};

// big: AlTables::big ([N + 1], z_off filled in); defs: the handle's block definitions (AlDef::p rows each); rows: AlTables::rows.
// A definition is identified by its id (what altro_hip_add_linear_constraint / _add_user_constraint returned): the same constraint
// registered knot point by knot point under separate ids makes chains of one.
inline AlShift al_shift_build(const std::vector<AlKnotBig>& big, const std::vector<AlDef>& defs, int rows) {
  AlShift s;
  s.next.assign((size_t)rows, -1);
  std::vector<char> pointed((size_t)rows, 0);
  for (size_t k = 0; k + 1 < big.size(); ++k) {
    const AlKnotBig &a = big[k], &b = big[k + 1];
    for (int j = 0; j < a.ncon; ++j) {
      int jn = -1;
      for (int i = 0; i < b.ncon && jn < 0; ++i) if (b.def[i] == a.def[j]) jn = i;
      if (jn < 0) continue;
      const int p = defs[(size_t)a.def[j]].p;
      for (int r = 0; r < p; ++r) {
        const int from = a.z_off[j] + r, to = b.z_off[jn] + r;
        assert(from >= 0 && from < rows && to < rows);
        assert(to > from);   // rows are packed in knot-point order: the in-place walk of kernels/al_shift.hip rests on it
        s.next[(size_t)from] = to;
        pointed[(size_t)to] = 1;
      }
    }
  }
  for (int r = 0; r < rows; ++r) if (!pointed[(size_t)r]) s.heads.push_back(r);
  s.order.reserve((size_t)rows + AL_SHIFT_PAD);
  for (int h : s.heads) {
    s.start.push_back((int)s.order.size());
    for (int r = h; r >= 0; r = s.next[(size_t)r]) s.order.push_back(r);
  }
  s.start.push_back((int)s.order.size());
  assert((int)s.order.size() == rows);   // every row is on exactly one chain
  s.order.resize((size_t)rows + AL_SHIFT_PAD, 0);
  return s;
}

}  // namespace capi
}  // namespace altro_hip
