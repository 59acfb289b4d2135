// Warm-up tuning of the temperature ladder: what a probe adds to the pooled counts, and the update of the ladder from one
// window's counts.  Plain C++ (no HIP include): the probe and update kernels of capi.hip use it, and tests/ladder_test.cpp checks
// it on the CPU against NumPy float64 (tests/ladder_reference.py).
//
// Windows.  With V = every, window j is the steps [j V, (j + 1) V); the ADAPTING windows are those that end at or before `until`
// (<= burn_in).  Steps behind them are ordinary burn-in under the final ladder, and past burn-in nothing adapts: what is sampled
// is a fixed-ladder chain.  Everything is a function of the step index counted from the start of the RUN, so a run cut into
// calls anywhere adapts at the same steps.  The arithmetic of the windows and of the probe steps, and what follows a launch that
// ends behind one, is schedule.h's (WarmupWindows, warmup_launch_at).
//
// Probes.  Step s of an adapting window is a PROBE step when (s + 1) % probe_every == 0; probe_every divides V, so a window's
// last step is always one.  Burn-in has no swap events and the probe adds none: it measures, from the states as they stand
// after the probe step, the probability with which every neighbouring pair WOULD swap, and moves nothing.  For chain c and
// pair t = 0 .. T - 2:
//   lp  = swap_log_prob(beta[t], beta[t + 1], logp[c, t], logp[c, t + 1])       kernel.h, operand order and roundings as there
//   thr = lp >= 0 ? 1.0f : hw_exp(lp)                                           the threshold of swap_accept_test
//   q   = thr == thr ? llrint((double) thr * 2^24) : 0                          ladder_quantum: a NaN counts as never accepted
//   pooled[t] += q,   and   pooled[T - 1] += 1 per (chain, probe)
// pooled is [T] int64: integer sums, exact whatever the order, which compose over launches, calls and shards.
//
// Update.  After window j one thread runs ladder_update: sequentially, in double, every sum over t ASCENDING.
//   pooled[T - 1] = 0: the ladder is left alone.
//   r_t   = pooled[t] / (pooled[T - 1] * 2^24)                  the pair's mean swap probability over the window
//   rbar  = (r_0 + r_1 + ... + r_{T-2}) / (T - 1)
//   g_t   = log(beta_t) - log(beta_{t+1}),   G = g_0 + ... + g_{T-2}
//   h_t   = log(g_t) + gain_j (r_t - rbar)                      gain_j = gain / (j + 1)^decay, on the host (window_gain)
//   w_t   = exp(h_t - max h),   S = w_0 + ... + w_{T-2},   c_t = w_0 + ... + w_t
//   beta_new[t + 1] = (float) ((double) beta_0 * exp(-G c_t / S))        t = 0 .. T - 3
// beta_0 and beta_{T-1} keep their bits.  A pair that swaps more often than the average is widened, one that swaps less is
// narrowed, both ends stay: the fixed point is equal swap rates.  Where the rounding to float leaves the new ladder not
// strictly decreasing (or anything in it is not a number) the WHOLE update is skipped: the ladder is kept and the caller
// counts one skip.  With rescale_scales the interior proposal scales follow their temperature,
//   temp_scale[t] = (float) ((double) temp_scale[t] * sqrt((double) beta_old[t] / (double) beta_new[t])),
// which an unchanged beta leaves unchanged bit for bit.
#pragma once

#include <cmath>

#include "schedule.h"

namespace ptrwm {

// what one (chain, pair, probe) adds to pooled[t], from the threshold of swap_accept_test
PTRWM_HD inline long long ladder_quantum(float thr) { return thr == thr ? llrint((double)thr * 16777216.0) : 0ll; }

enum LadderOutcome { kLadderUpdated = 0, kLadderNoProbes = 1, kLadderSkipped = 2 };

// The update (above): beta [T] and pooled [T] in, beta_new [T] out, work [T] doubles of scratch; T >= 3.  Whatever the outcome
// beta_new holds the ladder to go on with (kLadderNoProbes, kLadderSkipped: the bits of beta).
PTRWM_HD inline int ladder_update(const float *beta, const long long *pooled, int T, double gain_j, float *beta_new, double *work) {
  for (int t = 0; t < T; ++t) beta_new[t] = beta[t];
  const long long probes = pooled[T - 1];
  if (probes <= 0) return kLadderNoProbes;
  const int P = T - 1;  // pairs
  const double denom = (double)probes * 16777216.0;
  double rsum = 0.0;
  for (int t = 0; t < P; ++t) rsum += (double)pooled[t] / denom;
  const double rbar = rsum / (double)P;
  double G = 0.0, hmax = 0.0;
  for (int t = 0; t < P; ++t) {
    const double g = log((double)beta[t]) - log((double)beta[t + 1]);
    G += g;
    const double h = log(g) + gain_j * ((double)pooled[t] / denom - rbar);
    work[t] = h;
    if (t == 0 || h > hmax) hmax = h;
  }
  double S = 0.0;
  for (int t = 0; t < P; ++t) {
    const double w = exp(work[t] - hmax);
    work[t] = w;
    S += w;
  }
  double c = 0.0;
  for (int t = 0; t + 1 < P; ++t) {
    c += work[t];
    beta_new[t + 1] = (float)((double)beta[0] * exp(-G * c / S));
  }
  bool ok = true;
  for (int t = 0; t < P; ++t) ok = ok && beta_new[t] > beta_new[t + 1];  // (a NaN anywhere fails a comparison)
  if (!ok) {
    for (int t = 0; t < T; ++t) beta_new[t] = beta[t];
    return kLadderSkipped;
  }
  return kLadderUpdated;
}

// the scale of an interior temperature after its beta moved (rescale_scales; beta_old == beta_new: sqrt(1) = 1, the same bits)
PTRWM_HD inline float ladder_rescale(float scale, float beta_old, float beta_new) {
  return (float)((double)scale * sqrt((double)beta_old / (double)beta_new));
}

}  // namespace ptrwm
