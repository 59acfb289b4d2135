// The step schedule of a run, stated once: which step counters are past burn-in, which of them carry a swap event, a traced
// row or an accumulated step of the moments, how many of each lie in a range of steps, and where ptrwm_run cuts a long
// request into launches - and the warm-up windows of burn-in: which steps the proposal scale's and the ladder's tuning (adapt.h,
// ladder.h) adapt in, where their windows end, and what follows a launch that ends there.  Plain C++ (no HIP include): the
// kernels and host paths of capi.hip use it, and tests/schedule_test.cpp replays it step by step on the CPU.
//
// Steps are numbered from 0; step s has step_counter sc = s + 1 (the reference counts a step when it has happened), so a
// call with step0 covers the step counters (step0, step0 + n_steps].  What is periodic happens at the multiples of its
// period, counted from the start of the RUN (not of the call): that is what makes a cut, or a resumed run, invisible.
#pragma once

#include <cmath>

#ifdef __HIPCC__
#define PTRWM_HD __host__ __device__
#else
#define PTRWM_HD
#endif

namespace ptrwm {

// Is the step with step_counter sc past burn-in and a multiple of `period`?  The one rule of what happens every so many
// steps once burn-in is over: a swap event (swap_every), an accumulated step of the moments (every).  A traced row
// (trace_every) is the same rule with burn_in = 0: burn-in steps are traced too.
PTRWM_HD inline bool periodic_step_due(long long sc, long long burn_in, long long period) {
  return sc > burn_in && sc % period == 0;
}

// due steps with step_counter <= sc: the multiples m * period with burn_in < m * period <= sc
PTRWM_HD inline long long periodic_steps_upto(long long sc, long long burn_in, long long period) {
  const long long e = sc / period - burn_in / period;
  return e > 0 ? e : 0;
}

// ... with step_counter in (step0, step0 + n]: the due steps of n steps from step0
PTRWM_HD inline long long periodic_steps_in(long long step0, long long n, long long burn_in, long long period) {
  return periodic_steps_upto(step0 + n, burn_in, period) - periodic_steps_upto(step0, burn_in, period);
}

// steps from step0 to the first step whose step_counter is a multiple of `period` (1 = the step at step0 itself)
PTRWM_HD inline long long steps_to_next_multiple(long long step0, long long period) { return period - step0 % period; }

// steps from step0 to the next DUE step of a period, burn-in honoured (1 = the step at step0 itself): the distance to the
// first multiple of `period` above both step0 and burn_in.  A launch of that many steps from step0 ends exactly on a due
// step and holds no other; ptrwm_run_with_histogram min-s it into the cap of launch_at, so a snapshot kernel can read the
// state between two launches.
PTRWM_HD inline long long steps_to_next_due(long long step0, long long burn_in, long long period) {
  const long long base = step0 > burn_in ? step0 : burn_in;
  return (base / period + 1) * period - step0;
}

// 0-based number, since the start of the run, of the due step sc of a period (periodic_step_due(sc, ...) holds): the swap
// event of a swap step, the snapshot of a snapshot step (acf.h).  It comes from the step counter alone - nobody counts.
PTRWM_HD inline long long periodic_step_number(long long sc, long long burn_in, long long period) {
  return sc / period - burn_in / period - 1;
}
PTRWM_HD inline long long swap_event_number(long long sc, long long burn_in, long long swap_every) {
  return periodic_step_number(sc, burn_in, swap_every);
}

// One split step (ptrwm_split_accept): do its acceptances count, and does a swap event follow it?
struct SplitStepDue {
  bool count_on, swap_due;
};
PTRWM_HD inline SplitStepDue split_step_due(long long sc, long long burn_in, long long swap_every, int n_temps) {
  return {sc > burn_in, n_temps > 1 && periodic_step_due(sc, burn_in, swap_every)};
}

// One launch covers a bounded amount of work (32-bit in-kernel counters; no multi-second kernels on a shared GPU): at
// most 2^16 steps and about 2^33 chain-steps (~0.2 s at 4e10/s).  Longer requests become back-to-back launches on the
// same stream; step0 carries the swap schedule and the RNG position, so the split is invisible.
// 2^16 steps also bound how stale a launch-start decision can get: the verdict whether a replica's squared jumps may be
// taken from the proposal (proposals.h kJumpTrust) is re-taken at least that often - a coordinate cannot drift by more
// than a few hundred typical increments in between, which keeps the two definitions of the jump within ~1e-4 relative.
inline long long max_steps_per_launch(long long n_chains, int n_temps) {
  const long long by_work = (1ll << 33) / (n_chains * (long long)n_temps);
  return by_work < 1 ? 1 : (by_work > (1ll << 16) ? (1ll << 16) : by_work);
}

// The launch-invariant part of a request: ptrwm_run_args' schedule fields, trace_every already >= 1, moments_every = the
// accumulator's `every` (1 without one: mom_steps / steps_to_mom are then not looked at).
struct StepRequest {
  long long step0, n_steps, burn_in, swap_every, swap_event_offset, trace_every, trace_row0, moments_every;
};

// What the step kernel of one launch of a request is told (kernel.h KArgs / FullArgs: the fields of the same names)
struct LaunchCut {
  long long step0;             // first step of the launch
  int n;                       // its steps (<= cap)
  int burn_left;               // ... of which still in burn-in (step_counter <= burn_in)
  long long first_swap_event;  // number of the launch's first swap event (swap_event_offset included)
  long long events_before;     // swap events of the request's earlier launches: where the launch's ext_swap_u starts
  long long trace_row0;        // row of the launch's first traced step
  long long mom_steps;         // accumulated steps of the launch
  int steps_to_swap, steps_to_trace, steps_to_mom;  // countdowns to the first such step (1 = the launch's first step; > n: none)
};

// steps from step0 (>= 0) up to the next multiple of 2^32: as far as the high word of the step index - a part of every Philox
// counter (rng_layout.h step_word_c0hi) - holds.  No launch goes further: what a step kernel derives from that word at
// the start of a launch (kernel.h: the parked heads of its Philox blocks) then holds for the whole launch.
inline long long steps_to_step_word_wrap(long long step0) { return (1ll << 32) - (step0 & 0xffffffffll); }

// The launch of `r` that starts `done` steps into it, at most `cap` steps long (1 <= cap <= 2^16: max_steps_per_launch) and
// ending where the step index's high word changes, if that comes first: its length, and all of it
inline long long launch_steps(const StepRequest &r, long long done, long long cap) {
  const long long to_wrap = steps_to_step_word_wrap(r.step0 + done);
  if (to_wrap < cap) cap = to_wrap;
  return r.n_steps - done < cap ? r.n_steps - done : cap;
}
inline LaunchCut launch_at(const StepRequest &r, long long done, long long cap) {
  LaunchCut c;
  c.step0 = r.step0 + done;
  const long long n = launch_steps(r, done, cap);
  c.n = (int)n;
  const long long burn_left = r.burn_in - c.step0;
  c.burn_left = burn_left <= 0 ? 0 : (burn_left > n ? (int)n : (int)burn_left);
  c.events_before = periodic_steps_in(r.step0, done, r.burn_in, r.swap_every);
  c.first_swap_event = periodic_steps_upto(c.step0, r.burn_in, r.swap_every) + r.swap_event_offset;
  c.trace_row0 = r.trace_row0 + periodic_steps_in(r.step0, done, 0, r.trace_every);
  c.mom_steps = periodic_steps_in(c.step0, n, r.burn_in, r.moments_every);
  c.steps_to_swap = (int)steps_to_next_multiple(c.step0, r.swap_every);
  c.steps_to_trace = (int)steps_to_next_multiple(c.step0, r.trace_every);
  c.steps_to_mom = (int)steps_to_next_multiple(c.step0, r.moments_every);
  return c;
}

// ---- warm-up windows -----------------------------------------------------------------------------------------------------------
// A tuning of burn-in (the proposal scale's, adapt.h; the ladder's, ladder.h) works in windows of `every` steps: window k is the
// steps [k every, (k + 1) every), and the ADAPTING windows are those that end at or before `until` (<= burn_in): K = until /
// every of them, the steps [0, K every).  What lies behind is ordinary burn-in.  every = 0: no such tuning, nothing adapts.
struct WarmupWindows {
  long long every, until;
};

// K: the adapting windows of a run
inline long long window_count(const WarmupWindows &w) { return w.every > 0 ? w.until / w.every : 0; }

// the window step s lies in
inline long long window_of(const WarmupWindows &w, long long step) { return step / w.every; }

// does step s lie in an adapting window?  (s < K every)
inline bool step_adapts(const WarmupWindows &w, long long step) { return w.every > 0 && window_of(w, step) < window_count(w); }

// steps from s to the end of its window (1 = s is the window's last step): a launch of that many steps from s ends exactly
// where the window does
inline long long steps_to_window_end(const WarmupWindows &w, long long step) { return steps_to_next_multiple(step, w.every); }

// did a launch of n steps from `step` (inside an adapting window, n <= steps_to_window_end) end its window?
inline bool launch_ends_window(const WarmupWindows &w, long long step, long long n) { return (step + n) % w.every == 0; }

// A tuning that defers its update to the caller: may a request of n steps from step0 run?  Not if it would step past the end of
// the adapting window step0 lies in - that window's update is then still pending (the caller all-reduces the pooled counts and
// calls the stand-alone update first).
inline bool request_within_window(const WarmupWindows &w, long long step0, long long n) {
  return !step_adapts(w, step0) || n <= steps_to_window_end(w, step0);
}

// the gain of window k's update, gain / (k + 1)^decay: on the host in double, the device needs no pow
inline double window_gain(double gain, double decay, long long window) { return gain / std::pow((double)(window + 1), decay); }

// One launch of a request under the two tunings, and the small kernels behind it - in this order, after the histogram's
// snapshot: the scale's reduce and update, the ladder's probe and update.
struct WarmupLaunch {
  long long n;                       // its steps (<= cap)
  bool warmup;                       // it runs with the scale's warm-up overrides: acceptances counted from its first step, into
                                     // the window scratch, and no swap event
  bool scale_reduce, scale_update;   // it ends a window of the scale: the window's counts are pooled; the update follows
  bool ladder_probe, ladder_update;  // it ends behind a probe step of the ladder; ... a window's last: the update follows
  long long scale_window, ladder_window;  // the windows of the two updates
};

// The launch from `step` of at most `cap` steps (launch_steps: what the request and the step kernels allow).  Inside an adapting
// window of the scale it ends with the window at the latest, inside one of the ladder behind the next probe step - the steps s
// with (s + 1) % probe_every == 0; probe_every divides ladder.every, so a window's last step is one.  A tuning that defers its
// update (defer_*) gets the kernels that pool its counts and leaves the update to the caller.
inline WarmupLaunch warmup_launch_at(long long step, long long cap, const WarmupWindows &scale, bool defer_scale,
                                     const WarmupWindows &ladder, long long probe_every, bool defer_ladder) {
  WarmupLaunch l = {cap, step_adapts(scale, step), false, false, false, false, 0, 0};
  const bool probing = step_adapts(ladder, step);
  if (l.warmup && steps_to_window_end(scale, step) < l.n) l.n = steps_to_window_end(scale, step);
  if (probing && steps_to_next_multiple(step, probe_every) < l.n) l.n = steps_to_next_multiple(step, probe_every);
  if (l.warmup) {
    l.scale_window = window_of(scale, step);
    l.scale_reduce = launch_ends_window(scale, step, l.n);
    l.scale_update = l.scale_reduce && !defer_scale;
  }
  if (probing) {
    l.ladder_window = window_of(ladder, step);
    l.ladder_probe = (step + l.n) % probe_every == 0;
    l.ladder_update = l.ladder_probe && !defer_ladder && launch_ends_window(ladder, step, l.n);
  }
  return l;
}

}  // namespace ptrwm
