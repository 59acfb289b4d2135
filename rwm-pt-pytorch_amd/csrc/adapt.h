// Warm-up tuning of the proposal scale, stated once: which steps of burn-in belong to an adaptation window, where a window
// ends, and the Robbins-Monro update of one temperature's scale from the window's pooled acceptance count.  Plain C++ (no HIP
// include): the update kernel and the host paths of capi.hip use it, and tests/adapt_test.cpp replays it on the CPU against a
// brute-force loop and NumPy float64.
//
// Windows.  With W = every, window k is the steps [k W, (k + 1) W) (steps are numbered from 0, schedule.h).  The ADAPTING
// windows are those that end at or before `until` ((k + 1) W <= until, until <= burn_in): K = until / W of them, the steps
// [0, K W).  Steps [K W, burn_in) are ordinary burn-in under the final scale - the chains re-equilibrate under the frozen
// kernel - and past burn-in nothing adapts: what is sampled is a fixed-kernel Markov chain.  Everything is a function of the
// step index counted from the start of the RUN, so a run cut into calls anywhere adapts at the same steps.
//
// Update.  After window k, for temperature t, with pooled[t] the acceptances of every replica of t over the window and
// pooled[T] the chain-steps counted (n_chains x W, summed over shards):
//   rate  = pooled[t] / pooled[T]                                    (pooled[T] = 0: the scale is left alone)
//   s_new = (float) clamp((double) s_old * exp(gain_k * (rate - target)), min_scale, max_scale)
// in double, rounded to float once at the end.  gain_k = gain / (k + 1)^decay is computed on the HOST (adapt_gain) and
// passed in: the device needs no pow.  Integer counts in, one deterministic expression out: every shard that holds the same
// pooled integers computes the same bits.
#pragma once

#include <cmath>

#ifndef PTRWM_HD
#ifdef __HIPCC__
#define PTRWM_HD __host__ __device__
#else
#define PTRWM_HD
#endif
#endif

namespace ptrwm {

// K: the adapting windows of a run (every >= 1, until >= 0)
PTRWM_HD inline long long adapt_window_count(long long every, long long until) { return until / every; }

// the window step s lies in
PTRWM_HD inline long long adapt_window_of(long long step, long long every) { return step / every; }

// does window k adapt?
PTRWM_HD inline bool adapt_window_adapts(long long k, long long every, long long until) { return (k + 1) * every <= until; }

// does step s lie in an adapting window?  (s < K W)
PTRWM_HD inline bool adapt_step_adapts(long long step, long long every, long long until) {
  return adapt_window_adapts(adapt_window_of(step, every), every, until);
}

// steps from s to the end of its window (1 = s is the window's last step): a launch of that many steps from s ends exactly
// where the window does.  ptrwm_run_with_adaptation min-s it into the cap of launch_at for a step of an adapting window.
PTRWM_HD inline long long adapt_steps_to_window_end(long long step, long long every) { return every - step % every; }

// gain_k = gain / (k + 1)^decay, on the host in double
inline double adapt_gain(double gain, double decay, long long window) { return gain / std::pow((double)(window + 1), decay); }

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

// What one launch of a request is told about adaptation (host): is its first step in an adapting window, how far the
// launch may go at most, and which window it belongs to.
struct AdaptCut {
  bool adapting;       // the launch runs with the warm-up overrides (counts the window's acceptances, no swap event)
  long long window;    // its window (adapting only)
  long long to_end;    // steps to the window's end: the launch's cap (adapting only)
};
inline AdaptCut adapt_cut_at(long long step, long long every, long long until) {
  AdaptCut c;
  c.adapting = adapt_step_adapts(step, every, until);
  c.window = adapt_window_of(step, every);
  c.to_end = adapt_steps_to_window_end(step, every);
  return c;
}

// did a launch of n steps from `step` (inside an adapting window, n <= to_end) end its window?
inline bool adapt_launch_ends_window(long long step, long long n, long long every) { return (step + n) % every == 0; }

// defer_update: may a request of n steps from step0 run?  Not if it would step past the end of the adapting window step0 lies
// in - that window's update is then still pending (the caller all-reduces pooled and calls ptrwm_adapt_update first).
inline bool adapt_request_within_window(long long step0, long long n, long long every, long long until) {
  return !adapt_step_adapts(step0, every, until) || n <= adapt_steps_to_window_end(step0, every);
}

}  // namespace ptrwm
