// device_ledger.h on the CPU (plain g++, nothing of the library linked), with malloc / free standing in for the device and the pinned
// allocator: the counted sum against one recomputed by hand over add / remove / re-add; uncounted and pinned entries stay out of it; a
// double add and an unknown remove are reported and change nothing; two ledgers exchanged with std::swap (what replan_empty_handle does to
// two handles) each free exactly their new contents; drain hands every live entry to the function of its kind once and leaves nothing.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

#include "device_ledger.h"

using namespace altro_hip::capi;

static int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) { ++failures; std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); } \
  } while (0)

// the two backends: they free, and count how often each pointer came by
static std::map<void*, int> freed_device, freed_pinned;
static void free_device(void* p) { ++freed_device[p]; std::free(p); }
static int free_pinned(void* p) { ++freed_pinned[p]; std::free(p); return 0; }   // (a backend may return a status, like hipHostFree)

struct Want { void* p; size_t bytes; MemKind kind; bool counted; };
static size_t by_hand(const std::vector<Want>& live) {
  size_t sum = 0;
  for (const Want& w : live) if (w.counted) sum += w.bytes;
  return sum;
}

int main() {
  {   // add, remove, re-add: the count is the hand sum at every step; bytes_of for live and unknown pointers
    DeviceLedger L;
    std::vector<Want> live;
    const size_t sizes[] = {24, 0, 4096, 7, 1 << 20, 16};
    for (int i = 0; i < 6; ++i) {
      const Want w{std::malloc(sizes[i] ? sizes[i] : 16), sizes[i], i == 3 ? MEM_PINNED : MEM_DEVICE, i != 2 && i != 3};
      CHECK(L.add(w.p, w.bytes, w.kind, w.counted));
      live.push_back(w);
      CHECK(L.counted_bytes() == by_hand(live));
      CHECK(L.size() == live.size());
    }
    CHECK(L.counted_bytes() == 24 + 0 + (1 << 20) + 16);   // the uncounted 4096 and the pinned 7 never enter
    for (const Want& w : live) CHECK(L.bytes_of(w.p) == w.bytes);
    int on_stack = 0;
    CHECK(L.bytes_of(&on_stack) == 0 && L.bytes_of(nullptr) == 0);

    // a double add and an unknown remove: reported, nothing changes
    const size_t before = L.counted_bytes();
    CHECK(!L.add(live[0].p, 999, MEM_DEVICE, true));
    CHECK(!L.add(nullptr, 8, MEM_DEVICE, true));
    LedgerEntry e;
    e.bytes = 1234;
    CHECK(!L.remove(&on_stack, &e) && e.bytes == 1234);
    CHECK(!L.remove(nullptr));
    CHECK(L.counted_bytes() == before && L.size() == live.size() && L.bytes_of(live[0].p) == 24);

    // remove from the middle, the front and the back; the entry comes back as it went in
    for (size_t at : {size_t(2), size_t(0), live.size() - 3}) {
      const Want w = live[at];
      CHECK(L.remove(w.p, &e) && e.p == w.p && e.bytes == w.bytes && e.kind == w.kind && e.counted == w.counted);
      live.erase(live.begin() + at);
      CHECK(L.counted_bytes() == by_hand(live) && L.size() == live.size());
      CHECK(L.bytes_of(w.p) == 0 && !L.remove(w.p));   // gone: a second remove is the unknown one
      // re-add the same pointer value with another size (what a buffer that grows in place of a freed one may get from the allocator)
      const Want again{w.p, w.bytes + 100, w.kind, true};
      CHECK(L.add(again.p, again.bytes, again.kind, again.counted));
      live.push_back(again);
      CHECK(L.counted_bytes() == by_hand(live) && L.bytes_of(w.p) == w.bytes + 100);
    }

    // drain: the right backend, once per live entry, nothing left
    freed_device.clear(); freed_pinned.clear();
    L.drain(free_device, free_pinned);
    CHECK(L.size() == 0 && L.counted_bytes() == 0);
    CHECK(freed_device.size() + freed_pinned.size() == live.size());
    for (const Want& w : live) {
      CHECK((w.kind == MEM_PINNED ? freed_pinned : freed_device)[w.p] == 1);
      CHECK((w.kind == MEM_PINNED ? freed_device : freed_pinned).count(w.p) == 0);
      CHECK(L.bytes_of(w.p) == 0);
    }
    L.drain(free_device, free_pinned);   // an empty ledger frees nothing
    CHECK(freed_device.size() + freed_pinned.size() == live.size());
  }
  {   // two owners exchange their contents (std::swap of the structs that hold them): each ledger frees what it holds NOW
    struct Owner { void* a = nullptr; void* b = nullptr; DeviceLedger ledger; };
    Owner x, y;
    x.a = std::malloc(32); x.b = std::malloc(64);
    y.a = std::malloc(128);
    CHECK(x.ledger.add(x.a, 32, MEM_DEVICE, true) && x.ledger.add(x.b, 64, MEM_PINNED, false));
    CHECK(y.ledger.add(y.a, 128, MEM_DEVICE, true));
    void *const xa = x.a, *const xb = x.b, *const ya = y.a;
    std::swap(x, y);
    CHECK(x.a == ya && y.a == xa && y.b == xb);
    CHECK(x.ledger.counted_bytes() == 128 && y.ledger.counted_bytes() == 32);
    CHECK(x.ledger.bytes_of(ya) == 128 && x.ledger.bytes_of(xa) == 0 && y.ledger.bytes_of(xb) == 64);
    freed_device.clear(); freed_pinned.clear();
    y.ledger.drain(free_device, free_pinned);   // (the old handle goes)
    CHECK(freed_device.size() == 1 && freed_device[xa] == 1 && freed_pinned.size() == 1 && freed_pinned[xb] == 1);
    CHECK(x.ledger.size() == 1 && x.ledger.counted_bytes() == 128);   // the survivor is untouched
    CHECK(x.ledger.remove(ya));
    std::free(ya);
    CHECK(x.ledger.size() == 0);
  }
  if (failures) { std::printf("device_ledger_test: %d failures\n", failures); return 1; }
  std::printf("device_ledger_test ok\n");
  return 0;
}
