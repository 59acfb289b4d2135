// Replica flow through a temperature ladder, stated once: the flow word that travels with a replica's row through every swap
// event, and what an event does to it - the round-trip count of every walker (cold -> hot -> cold) and, per temperature, the
// visits made by replicas that last touched the cold end ("up") or the hot end ("down"): Katzgraber et al. 2006.  Plain C++
// (no HIP include): the FULL twins of both step kernels (kernel.h, quad.h) and the stand-alone sweep kernel (capi.hip) build
// and update their words by calling this header, and tests/flow_test.cpp checks it against a literal restatement on the CPU.
//
// Flow word, one int32 per (ladder, position):   bits 0..15 the walker id,   bits 16..17 the direction
//   0 none (no end visited yet),  1 up (the last end visited was the cold one, t = 0),  2 down (... the hot one, t = T - 1).
// The caller starts a run with word[c, t] = t (id t, direction none).
//
// One swap event of a ladder of T >= 2 temperatures; src[t] = the position whose post-Metropolis vector the event puts at
// position t (kernel.h swap_decide):
//   1. new[t] = old[src[t]] for every t: the word moves exactly as the row moves.  PTRWM_SWAP_EXCHANGE: a permutation.
//      PTRWM_SWAP_REFERENCE_COPY: a copy - ids may repeat and vanish, as the rows do ("lineage": an id names where the vector
//      at a position descends from, no longer one of T distinct walkers).
//   2. ends.  t = 0: a word whose direction is down has completed a round trip, round_trips[c, id] += 1; its direction becomes
//      up.  t = T - 1: its direction becomes down.
//   3. visits.  Every t: direction up -> n_up[c, t] += 1, down -> n_down[c, t] += 1, none -> nothing.
// Everything is integer: the results are exact and do not depend on the order in which threads, launches or shards do their
// part.
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

constexpr int kFlowIdBits = 16;  // ids 0 .. n_temps - 1 (n_temps <= 256)
constexpr int32_t kFlowIdMask = (1 << kFlowIdBits) - 1;
constexpr int kFlowNone = 0, kFlowUp = 1, kFlowDown = 2;

PTRWM_HD inline int32_t flow_word(int id, int dir) { return (int32_t)id | ((int32_t)dir << kFlowIdBits); }
PTRWM_HD inline int flow_id(int32_t w) { return (int)(w & kFlowIdMask); }
PTRWM_HD inline int flow_dir(int32_t w) { return (int)((w >> kFlowIdBits) & 3); }

// Step 2 for the word that has just landed at position t of a ladder of T >= 2 temperatures: the word it becomes;
// trip = it has completed a round trip (t = 0 and it came down from the hot end): the caller counts it under flow_id(w).
PTRWM_HD inline int32_t flow_ends(int32_t w, int t, int T, bool &trip) {
  trip = t == 0 && flow_dir(w) == kFlowDown;
  if (t == 0) return flow_word(flow_id(w), kFlowUp);
  if (t == T - 1) return flow_word(flow_id(w), kFlowDown);
  return w;
}

// Step 3 for the word at a position after step 2: what the position's up / down visit counts gain
PTRWM_HD inline unsigned flow_visit_up(int32_t w) { return flow_dir(w) == kFlowUp ? 1u : 0u; }
PTRWM_HD inline unsigned flow_visit_down(int32_t w) { return flow_dir(w) == kFlowDown ? 1u : 0u; }

}  // namespace ptrwm
