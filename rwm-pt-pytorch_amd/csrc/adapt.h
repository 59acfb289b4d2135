// Warm-up tuning of the proposal scale: the Robbins-Monro update of one temperature's scale from an adaptation window's pooled
// acceptance count.  Plain C++ (no HIP include): the update kernel of capi.hip uses it, and tests/adapt_test.cpp checks it on the
// CPU against NumPy float64.
//
// Windows.  With W = every, window k is the steps [k W, (k + 1) W); the ADAPTING windows are those that end at or before `until`
// (<= burn_in).  Steps behind them are ordinary burn-in under the final scale - the chains re-equilibrate under the frozen
// kernel - and past burn-in nothing adapts: what is sampled is a fixed-kernel Markov chain.  Everything is a function of the
// step index counted from the start of the RUN, so a run cut into calls anywhere adapts at the same steps.  The arithmetic of
// the windows, and what follows a launch that ends one, is schedule.h's (WarmupWindows, warmup_launch_at).
//
// Update.  After window k, for temperature t, with pooled[t] the acceptances of every replica of t over the window and
// pooled[T] the chain-steps counted (n_chains x W, summed over shards):
//   rate  = pooled[t] / pooled[T]                                    (pooled[T] = 0: the scale is left alone)
//   s_new = (float) clamp((double) s_old * exp(gain_k * (rate - target)), min_scale, max_scale)
// in double, rounded to float once at the end.  gain_k = gain / (k + 1)^decay is computed on the HOST (schedule.h window_gain)
// and passed in: the device needs no pow.  Integer counts in, one deterministic expression out: every shard that holds the same
// pooled integers computes the same bits.
#pragma once

#include <cmath>

#include "schedule.h"

namespace ptrwm {

// the update of one temperature (above)
PTRWM_HD inline float adapt_update(float s_old, long long accepted, long long counted, double gain_k, double target,
                                   float min_scale, float max_scale) {
  if (counted <= 0) return s_old;
  const double rate = (double)accepted / (double)counted;
  double s = (double)s_old * exp(gain_k * (rate - target));
  if (!(s >= (double)min_scale)) s = (double)min_scale;  // (a NaN lands on the lower bound)
  if (s > (double)max_scale) s = (double)max_scale;
  return (float)s;
}

}  // namespace ptrwm
