// device_ledger.h -- what a batch handle owns: every device buffer and every pinned host buffer it allocated, with its size.  The handle's
// pointer fields stay raw pointers (the kernels' argument builders read them); the ledger is what frees them -- one at a time through
// capi_internal.h's dfree, all that is left through drain when the handle goes -- and what altro_hip_batch_device_bytes adds up.
// Entries are keyed by the pointer's VALUE, not by the field that holds it: replan_empty_handle exchanges two handles' contents
// (std::swap), and each ledger moves with the buffers it lists.  Plain C++, no HIP call, no handle: tests/cpp/device_ledger_test.cpp
// checks it with g++, malloc and free.
#pragma once
#include <cstddef>
#include <vector>

namespace altro_hip {
namespace capi {

enum MemKind { MEM_DEVICE = 0, MEM_PINNED = 1 };

struct LedgerEntry {
  void* p = nullptr;
  size_t bytes = 0;
  MemKind kind = MEM_DEVICE;
  bool counted = false;   // part of counted_bytes() (the staging buffer, the stationarity partials and pinned memory are not)
};

class DeviceLedger {
 public:
  // false (and nothing changes): p is null or already listed -- a programming error the caller may assert on
  bool add(void* p, size_t bytes, MemKind kind, bool counted) {
    if (!p || find(p) != e_.size()) return false;
    e_.push_back(LedgerEntry{p, bytes, kind, counted});
    return true;
  }
  // false (and nothing changes): p is not listed; otherwise the entry leaves the ledger and, if asked for, is handed back
  bool remove(const void* p, LedgerEntry* out = nullptr) {
    const size_t i = find(p);
    if (i == e_.size()) return false;
    if (out) *out = e_[i];
    e_[i] = e_.back();
    e_.pop_back();
    return true;
  }
  // the sum over the live counted entries, added up when asked: there is no running total that a missed update could leave wrong
  size_t counted_bytes() const {
    size_t sum = 0;
    for (const LedgerEntry& e : e_) if (e.counted) sum += e.bytes;
    return sum;
  }
  size_t bytes_of(const void* p) const {   // 0: not listed
    const size_t i = find(p);
    return i == e_.size() ? 0 : e_[i].bytes;
  }
  size_t size() const { return e_.size(); }
  // every live entry to the function of its kind, once; the ledger is empty afterwards
  template <typename FreeDevice, typename FreePinned>
  void drain(FreeDevice free_device, FreePinned free_pinned) {
    std::vector<LedgerEntry> all;
    all.swap(e_);
    for (const LedgerEntry& e : all) {
      if (e.kind == MEM_PINNED) (void)free_pinned(e.p);
      else (void)free_device(e.p);
    }
  }

 private:
  size_t find(const void* p) const {   // (a handle lists some hundred buffers at most, and looks one up next to a hipMalloc or a hipFree)
    size_t i = 0;
    while (i < e_.size() && e_[i].p != p) ++i;
    return i;
  }
  std::vector<LedgerEntry> e_;
};

}  // namespace capi
}  // namespace altro_hip
