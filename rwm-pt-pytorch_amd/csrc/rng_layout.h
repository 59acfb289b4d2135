// Where a replica's random numbers come from, stated once: the Philox4x32-10 key and counter words of every draw of the
// library, the ordinal a swap attempt is recorded under, and the threads of an exchange group.  Plain C++ (no HIP
// include): every kernel and host path of csrc/ builds these words by calling this header, and tests/rng_layout_test.cpp
// checks each helper against a literal restatement on the CPU.  (oracle/ptrwm_oracle.c, tests/init_reference.py and the
// layout paragraph of include/ptrwm.h restate the layout on purpose: they are what the kernels are checked AGAINST.)
//
// Counter layout:
//   c0 = block index within the step | (step >> 32) << 16
//   c1 = step (low 32 bits, 0-based)
//   c2 = global chain id (low 32 bits)
//   c3 = temperature index | stream << 8 | (global chain id >> 32) << 12
//   key = (seed low, seed high)
// stream 0 = MH proposal + accept draws, stream 1 = swap uniforms, stream 2 = stand-alone swap sweeps (the binding's
// default rng_stream for ptrwm_swap_sweep).
// stream 3 = starting points (ptrwm_init_states, capi.hip).  They are drawn before step 0, so the step words are free:
//   c0 = (coordinate / 4) | attempt << 16      one block per four coordinates, word d % 4 is coordinate d's
//   c1 = 0
//   c2 = global chain id (low 32 bits)
//   c3 = (per_temperature ? temperature index : 0) | 3 << 8 | (global chain id >> 32) << 12
#pragma once
#include <stdint.h>

#include "../../include/ptrwm.h"

// (inlined where they are written, before anything else is optimised: the step kernels sit at their register caps, and a
// word built by a call that is inlined later than the code around it has moved their register allocation)
#ifdef __HIPCC__
#define PTRWM_RNG_FN __host__ __device__ __forceinline__
#else
#define PTRWM_RNG_FN inline
#endif

namespace ptrwm {

constexpr uint32_t kStreamMH = 0u;
constexpr uint32_t kStreamSwap = 1u;
constexpr uint32_t kStreamInit = 3u;

struct PhiloxKey {
  uint32_t k0, k1;
};
PTRWM_RNG_FN PhiloxKey philox_key(uint64_t seed) { return {(uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32)}; }

// the step words of a 0-based step index: c0 without the block index (or-ed in per block by the proposals), and c1
PTRWM_RNG_FN uint32_t step_word_c0hi(unsigned long long step) { return (uint32_t)(step >> 32) << 16; }
PTRWM_RNG_FN uint32_t step_word_c1(unsigned long long step) { return (uint32_t)step; }

// the chain words of a global chain id (chain_offset + chain) and a temperature index: c2, and c3 without its stream - the
// "base word" the step kernels keep (the thread kernel parks it in LDS and reads the temperature index back from it)
PTRWM_RNG_FN uint32_t chain_word_c2(unsigned long long gchain) { return (uint32_t)gchain; }
PTRWM_RNG_FN uint32_t chain_word_c3(unsigned long long gchain, uint32_t t) { return t | ((uint32_t)(gchain >> 32) << 12); }
PTRWM_RNG_FN uint32_t with_stream(uint32_t c3_base, uint32_t stream) { return c3_base | (stream << 8); }
PTRWM_RNG_FN int temperature_of(uint32_t c3) { return (int)(c3 & 0xffu); }

// stream 3: the block that holds coordinate d of a starting point (its word: init_word_of(d)), and its c3
PTRWM_RNG_FN uint32_t init_word_c0(int d, int attempt) { return (uint32_t)(d / 4) | ((uint32_t)attempt << 16); }
PTRWM_RNG_FN int init_word_of(int d) { return d % 4; }
PTRWM_RNG_FN uint32_t init_word_c3(unsigned long long gchain, uint32_t t, bool per_temperature) {
  return with_stream(chain_word_c3(gchain, per_temperature ? t : 0u), kStreamInit);
}

// 1-based ordinal, counted from the start of the run, of the attempt of pair (t, t+1) in swap event `event` (0-based).
// Sequential order: T-1 attempts per event; even/odd events have a varying pair count, so the event number is recorded.
PTRWM_RNG_FN long long swap_attempt_ordinal(int order, long long event, int n_temps, int t) {
  return order == PTRWM_ORDER_SEQUENTIAL ? event * (n_temps - 1) + t + 1 : event + 1;
}

// Threads of an exchange group.  A ladder that fits one wavefront (lanes_per_replica * n_temps <= 64): the wavefront.
// Longer ladders: the group is the workgroup, whole waves.  One thread per replica (lanes_per_replica = 1): one ladder per
// workgroup.  Lane-split form (4): as many whole ladders as make the best use of the lanes within kPackThreads threads
// (T = 17: three ladders in 204 of 256 lanes instead of one in 68 of 128), one ladder when even one does not fit.
constexpr int kPackThreads = 256;
PTRWM_RNG_FN int packed_ladders_per_group(int need) {  // need = lanes of one ladder, > 64
  int best_k = 1;
  double best_use = 0.0;
  for (int k = 1; k * need <= kPackThreads; ++k) {
    const int b = (k * need + 63) & ~63;
    const double use = (double)(k * need) / b;
    if (use > best_use + 1e-9) {
      best_use = use;
      best_k = k;
    }
  }
  return best_k;
}
PTRWM_RNG_FN int group_threads(int n_temps, int lanes_per_replica) {
  if (lanes_per_replica == 1) return n_temps > 64 ? ((n_temps + 63) & ~63) : 64;
  const int need = lanes_per_replica * n_temps;
  return need > 64 ? ((lanes_per_replica == 1 ? 1 : packed_ladders_per_group(need)) * need + 63) & ~63 : 64;
}

}  // namespace ptrwm
