// The sequential exchange sweep of a swap event, decided for every ladder of a wavefront at once with lane masks, stated once.
// Plain C++ (no HIP include): the step kernel (kernel.h, exchange groups of one wavefront) supplies the masks from wave
// ballots and walks them on the scalar unit; tests/swap_walk_test.cpp checks this header against a literal restatement of
// the sweep on the CPU.
//
// The sweep j = 0 .. T-2 of a ladder carries one state upward: at pair j the state now at position j (the carrier) meets the
// untouched state of position j + 1.  Accepted: the carrier moves on and position j takes the state of j + 1.  Refused: the
// carrier stays at position j and the state of j + 1 carries on.  The carrier is always one of the ladder's ORIGINAL states,
// and every value a pair's rule looks at is an original (kernel.h swap_decide), so the decision at pair j is a function of
// (which lane carries, j) alone.  Hence, with lane k of the wavefront holding position k - base of its ladder:
//   pass_j   bit k = "the state of lane k, were it the carrier, would be accepted at pair j of its ladder" - one compare
//            per lane and pair, taken on all 64 lanes at once (a ballot); bits of lanes outside live ladders may hold anything
//   seg0     a bit at the lane of position 0 of every live ladder (ladders are whole runs of T <= 64 consecutive lanes)
// and the walk keeps two 64-bit words that are the same for the whole wavefront,
//   carrier  one bit per ladder: the lane whose state is carried
//   rejected bit base + j + 1 set iff pair j of that ladder was refused (position j + 1's state became the carrier)
// Pair j, with next = seg0 << (j + 1) (position j + 1 of every ladder) and below = next - seg0 (bits base .. base + j of every
// ladder, the positions the sweep has passed: no borrow leaves a ladder's run):   failed = carrier & ~pass_j.  Inside a
// ladder's run, failed + below carries into bit base + j + 1 exactly when the ladder's carrier failed (the carrier's bit lies
// in base .. base + j, all of which are set in `below`), and failed + below < 2^(base + j + 2) <= 2^(base + T): no carry
// leaves the ladder's run, nothing overflows at T = 64.
// A position's outcome is read from `rejected` alone (swap_walk_source).
#pragma once
#include <stdint.h>

#ifndef PTRWM_HD
#ifdef __HIPCC__
#define PTRWM_HD __host__ __device__
#else
#define PTRWM_HD
#endif
#endif

namespace ptrwm {

struct SwapWalk {
  uint64_t carrier, rejected;
};

// before pair 0: every ladder carries the state of its position 0
PTRWM_HD inline SwapWalk swap_walk_begin(uint64_t seg0) { return SwapWalk{seg0, 0ull}; }

// pair j of every ladder (called for j = 0 .. T-2 in order; j + 1 <= 63), pass = pass_j
PTRWM_HD inline void swap_walk_step(SwapWalk &w, uint64_t seg0, int j, uint64_t pass) {
  const uint64_t next = seg0 << (j + 1);
  const uint64_t failed = w.carrier & ~pass;
  const uint64_t fresh = (failed + (next - seg0)) & next;  // position j + 1 of the ladders whose carrier failed
  w.carrier = (w.carrier & pass) | fresh;
  w.rejected |= fresh;
}

// After pair T-2: the lane whose original state (and log-density) ends up at the position held by lane `pos`, 0 <= pos < 64;
// has_pair = the position is not its ladder's last; pair_acc = its pair (pos, pos + 1) was accepted.  An accepted pair
// hands position pos the state of pos + 1.  Otherwise the carrier of that moment stays: the last position <= pos at which a
// state became the carrier - or the ladder's position 0 - which for the last position is the sweep's final carrier.
// (pos = 0 names lane 0, which always starts a ladder: the `| 1` only keeps the count of leading zeros defined for a caller
// whose seg0 is empty.)
PTRWM_HD inline int swap_walk_source(uint64_t rejected, uint64_t seg0, int pos, bool has_pair, bool &pair_acc) {
  pair_acc = has_pair && ((rejected >> pos) & 2ull) == 0ull;  // bit pos + 1 (pos = 63 has no pair)
  const uint64_t upto = (2ull << pos) - 1ull;                 // bits 0 .. pos (pos = 63: all)
  const int carrier = 63 - __builtin_clzll(((rejected | seg0) & upto) | 1ull);
  return pair_acc ? pos + 1 : carrier;
}

}  // namespace ptrwm
