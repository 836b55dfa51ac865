// Slot policy of the pinned -> device plan rings (handle.h: PlanRing).  Host-pure (no HIP headers):
// tests/native/surface_plan_check.cpp checks it under sanitizers with a plain g++.
#pragma once

namespace lp {

// A call takes the next slot round-robin; the slot's previous use has to be waited for only if the slot is still marked busy,
// i.e. once the ring has wrapped.  take() returns the slot and whether its event must be waited on before the slot is
// written; the caller marks it busy again behind the new use (mark()).  The ring advances at take(): after a HIP error thrown
// between take() and mark() the slot is left unmarked rather than un-advanced.
template <int RING>
struct RingSlots {
  bool busy[RING] = {};
  int next = 0;
  int take(bool* wait) {
    const int slot = next;
    next = (next + 1) % RING;
    *wait = busy[slot];
    busy[slot] = false;
    return slot;
  }
  void mark(int slot) { busy[slot] = true; }
};

}  // namespace lp
