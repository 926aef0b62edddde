// async_slots.hpp -- ticket bookkeeping of p1hip_batch_submit /
// p1hip_batch_wait that needs no device: which of the kSlots slots are taken,
// by which ticket, and whether a ticket a caller presents is still the one
// its slot was given.  p1hip.hip holds one AsyncSlots under the runtime mutex
// (the class itself takes no lock); tests/async_slots_test.cpp runs it
// against a model.
//
// A ticket is (serial << 8) | (slot + 1): never 0, and no two tickets of one
// AsyncSlots are ever equal (the serial only grows; 2^56 of them), so a stale
// ticket -- released, claimed twice or cancelled -- can never name a later
// call that happens to sit in the same slot.
//
// Life of a slot:  idle --Alloc--> live --Claim--> claimed --Release--> idle
//   live     submitted, nobody waits for it yet
//   claimed  one p1hip_batch_wait owns it (a second wait on the same ticket
//            finds nothing to claim); it may be blocked on the slot's events
//            with the runtime mutex released
// Release also takes a live ticket (a submit that failed after Alloc).
// CancelAll (shutdown, re-init) makes every slot idle at once; the claimed
// ones' waiters find their ticket stale when they come back (Holds).
#pragma once
#include <stdint.h>

namespace p1 {

template <int kSlots>
class AsyncSlotsT {
 public:
  static_assert(kSlots >= 1 && kSlots <= 255, "the slot is one byte of the ticket");

  // A free slot becomes live; its ticket, or 0 when all kSlots are taken.
  uint64_t Alloc() {
    for (int s = 0; s < kSlots; ++s)
      if (state_[s] == kIdle) {
        state_[s] = kLive;
        ticket_[s] = (++serial_ << 8) | (uint64_t)(s + 1);
        return ticket_[s];
      }
    return 0;
  }

  // The slot (0 .. kSlots-1) `ticket` holds, live or claimed; -1 if it holds none.
  int Holds(uint64_t ticket) const {
    const int s = (int)(ticket & 0xff) - 1;
    if (ticket == 0 || s < 0 || s >= kSlots) return -1;
    return state_[s] != kIdle && ticket_[s] == ticket ? s : -1;
  }

  // live -> claimed; the slot, or -1 (unknown, already claimed, released or cancelled).
  int Claim(uint64_t ticket) {
    const int s = Holds(ticket);
    if (s < 0 || state_[s] != kLive) return -1;
    state_[s] = kClaimed;
    return s;
  }

  // live or claimed -> idle; false (and nothing changes) for a stale ticket.
  bool Release(uint64_t ticket) {
    const int s = Holds(ticket);
    if (s < 0) return false;
    state_[s] = kIdle;
    ticket_[s] = 0;
    return true;
  }

  // Every outstanding ticket becomes stale; returns how many there were.
  int CancelAll() {
    const int n = Outstanding();
    for (int s = 0; s < kSlots; ++s) {
      state_[s] = kIdle;
      ticket_[s] = 0;
    }
    return n;
  }

  // Slots that are not idle.
  int Outstanding() const {
    int n = 0;
    for (int s = 0; s < kSlots; ++s) n += state_[s] != kIdle;
    return n;
  }

 private:
  enum State : uint8_t { kIdle, kLive, kClaimed };
  State state_[kSlots] = {};
  uint64_t ticket_[kSlots] = {};
  uint64_t serial_ = 0;
};

}  // namespace p1
