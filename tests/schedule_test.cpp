// csrc/schedule.h against brute force: every launch of every request of a grid is replayed step by step with the literal
// rules (step_counter sc = step + 1; due: sc > burn_in && sc % period == 0; traced: sc % trace_every == 0).  Plain C++,
// its own main: tests/test_host_logic.py compiles it with g++ -fsanitize=address,undefined and runs it.
#include <cstdio>
#include <cstdlib>

#include "../rwm-pt-pytorch_amd/csrc/schedule.h"
#include "warmup_test_util.h"

using namespace ptrwm;

static long long g_checks = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    ++g_checks;                                           \
    if (!(cond)) {                                        \
      std::printf("FAILED %s (line %d): ", #cond, __LINE__); \
      std::printf(__VA_ARGS__);                           \
      std::printf("\n");                                  \
      std::exit(1);                                       \
    }                                                     \
  } while (0)

static bool due(long long sc, long long burn_in, long long period) { return sc > burn_in && sc % period == 0; }

// due steps with step_counter in (s0, s0 + n]
static long long count_due(long long s0, long long n, long long burn_in, long long period) {
  long long c = 0;
  for (long long sc = s0 + 1; sc <= s0 + n; ++sc) c += due(sc, burn_in, period) ? 1 : 0;
  return c;
}

// steps from s0 to the first multiple of `period` within n steps (1 = the first step), 0 if there is none
static long long first_multiple(long long s0, long long n, long long period) {
  for (long long i = 1; i <= n; ++i)
    if ((s0 + i) % period == 0) return i;
  return 0;
}

static void check_countdown(long long got, long long s0, long long n, long long period, const char *what) {
  const long long want = first_multiple(s0, n, period);
  if (want > 0) CHECK(got == want, "%s: countdown %lld, first multiple of %lld after step %lld is %lld steps on", what, got, period, s0, want);
  else CHECK(got > n, "%s: countdown %lld points into a launch of %lld steps from %lld that has no multiple of %lld", what, got, n, s0, period);
}

int main() {
  // the single-step functions against the literal rules
  for (long long burn_in = 0; burn_in <= 9; ++burn_in)
    for (long long p = 1; p <= 5; ++p) {
      long long upto = 0;
      for (long long sc = 0; sc <= 60; ++sc) {
        const bool d = due(sc, burn_in, p);
        upto += d ? 1 : 0;
        CHECK(periodic_step_due(sc, burn_in, p) == d, "sc %lld burn_in %lld period %lld", sc, burn_in, p);
        CHECK(periodic_steps_upto(sc, burn_in, p) == upto, "sc %lld burn_in %lld period %lld", sc, burn_in, p);
        CHECK(swap_event_number(sc, burn_in, p) == sc / p - burn_in / p - 1, "sc %lld burn_in %lld period %lld", sc, burn_in, p);
        if (d) CHECK(swap_event_number(sc, burn_in, p) == upto - 1, "sc %lld burn_in %lld period %lld", sc, burn_in, p);  // 0-based
        for (int n_temps = 1; n_temps <= 2; ++n_temps) {
          const SplitStepDue s = split_step_due(sc, burn_in, p, n_temps);
          CHECK(s.count_on == (sc > burn_in) && s.swap_due == (n_temps > 1 && d), "sc %lld burn_in %lld period %lld n_temps %d", sc,
                burn_in, p, n_temps);
        }
      }
    }

  // the three regimes of the launch length and their boundaries: 2^16 steps up to 2^17 replicas, 2^33 / replicas steps up
  // to 2^33 replicas, one step above
  CHECK(max_steps_per_launch(1, 1) == 65536, "1 replica");
  CHECK(max_steps_per_launch(1ll << 12, 32) == 65536, "2^17 replicas");
  CHECK(max_steps_per_launch((1ll << 17) + 1, 1) == 65535, "2^17 + 1 replicas");
  CHECK(max_steps_per_launch(1ll << 28, 32) == 1, "2^33 replicas");
  CHECK(max_steps_per_launch((1ll << 33) + 1, 1) == 1, "2^33 + 1 replicas");

  // every launch of every request
  const long long kOffset = 3, kRow0 = 5;  // (non-zero: an omitted term shows)
  const long long caps[] = {1, 2, 3, 5, 7};
  long long launches = 0;
  for (long long burn_in = 0; burn_in <= 9; ++burn_in)
    for (long long se = 1; se <= 5; ++se)
      for (long long te = 1; te <= 4; ++te)
        for (long long me = 1; me <= 4; ++me)
          for (long long step0 = 0; step0 <= 11; ++step0)
            for (long long n_steps = 1; n_steps <= 13; ++n_steps)
              for (long long cap : caps) {
                const StepRequest req = {step0, n_steps, burn_in, se, kOffset, te, kRow0, me};
                long long done = 0, events = 0, rows = 0;
                while (done < n_steps) {
                  const LaunchCut c = launch_at(req, done, cap);
                  const long long s0 = step0 + done, n = c.n;
#define WHERE "burn_in %lld se %lld te %lld me %lld step0 %lld n_steps %lld cap %lld done %lld", burn_in, se, te, me, step0, n_steps, cap, done
                  // the launches tile the request
                  CHECK(c.step0 == s0 && n >= 1 && n == (n_steps - done < cap ? n_steps - done : cap), WHERE);
                  long long burn = 0;
                  for (long long sc = s0 + 1; sc <= s0 + n; ++sc) burn += sc <= burn_in ? 1 : 0;
                  CHECK(c.burn_left == burn, WHERE);
                  // what the launch holds, and what came before it
                  const long long ev = count_due(s0, n, burn_in, se), tr = count_due(s0, n, 0, te);
                  CHECK(periodic_steps_in(s0, n, burn_in, se) == ev, WHERE);
                  CHECK(periodic_steps_in(s0, n, 0, te) == tr, WHERE);
                  CHECK(c.mom_steps == count_due(s0, n, burn_in, me), WHERE);
                  CHECK(c.events_before == events, WHERE);
                  CHECK(c.first_swap_event == count_due(0, s0, burn_in, se) + kOffset, WHERE);
                  CHECK(c.trace_row0 == kRow0 + rows, WHERE);
                  // the countdowns run to the next multiple of the period, burn-in or not (the kernels gate swap events and
                  // accumulated steps with burn_left)
                  check_countdown(c.steps_to_swap, s0, n, se, "swap");
                  check_countdown(c.steps_to_trace, s0, n, te, "trace");
                  check_countdown(c.steps_to_mom, s0, n, me, "moments");
#undef WHERE
                  events += ev;
                  rows += tr;
                  done += n;
                  ++launches;
                }
                CHECK(done == n_steps, "request overrun");
              }
  // the warm-up windows against a loop over the windows, for the periods and ends the two tunings' own tests (adapt_test.cpp,
  // ladder_test.cpp) run with; the probe steps of a launch of one step; the rule of a deferred update
  long long positions = 0;
  const long long everys[] = {1, 6, 7, 50};
  for (long long W : everys) {
    const long long N = 4 * W + 7 + 5;
    const long long untils[] = {0, W - 1, W, 3 * W + 5, 3 * W + 7, 4 * W + 5, 4 * W + 7};
    for (long long until : untils) {
      const WarmupWindows w = {W, until};
      const long long K = window_count(w);
      long long k_bf = 0;
      while ((k_bf + 1) * W <= until) ++k_bf;
      CHECK(K == k_bf, "every %lld until %lld", W, until);
      for (long long k = 0; k < K + 3; ++k) CHECK(((k + 1) * W <= until) == (k < K), "every %lld until %lld window %lld", W, until, k);
      for (long long s = 0; s < N + 2 * W; ++s) {
#define WHERE "every %lld until %lld step %lld", W, until, s
        long long bw = -1;
        const bool ad = bf_step_adapts(s, W, until, &bw);
        CHECK(step_adapts(w, s) == ad && ad == (s < K * W), WHERE);
        CHECK(window_of(w, s) == s / W, WHERE);
        if (ad) CHECK(window_of(w, s) == bw && bw < K, WHERE);
        long long to_end = 1;
        while ((s + to_end) % W != 0) ++to_end;
        CHECK(steps_to_window_end(w, s) == to_end, WHERE);
        for (long long n = 1; n <= to_end; ++n) CHECK(launch_ends_window(w, s, n) == (n == to_end), WHERE);
        // a deferred update: a request may not step past the end of the adapting window it starts in
        for (long long n = 0; n <= 2 * W + 1; ++n) CHECK(request_within_window(w, s, n) == (!ad || n <= to_end), WHERE);
        // probe steps: (s + 1) % P == 0 inside an adapting window, P a divisor of the period - a window's last step is one
        for (long long P = 1; P <= W; ++P) {
          if (W % P != 0) continue;
          long long to_probe = 1;
          while ((s + to_probe) % P != 0) ++to_probe;
          CHECK(steps_to_next_multiple(s, P) == to_probe && to_probe <= to_end, WHERE);
          const WarmupLaunch one = warmup_launch_at(s, 1, {0, 0}, false, w, P, false);
          CHECK(one.n == 1 && !one.warmup && !one.scale_reduce && !one.scale_update, WHERE);
          CHECK(one.ladder_probe == (ad && (s + 1) % P == 0), WHERE);
          CHECK(one.ladder_update == (ad && (s + 1) % W == 0) && (!one.ladder_update || (one.ladder_probe && one.ladder_window == bw)), WHERE);
        }
#undef WHERE
        ++positions;
      }
    }
  }
  const WarmupWindows none = {0, 0};  // no such tuning
  CHECK(window_count(none) == 0 && !step_adapts(none, 0) && !step_adapts(none, 7) && request_within_window(none, 3, 1000), "every 0");
  CHECK(window_gain(3.0, 0.5, 0) == 3.0 && window_gain(3.0, 0.5, 3) == 1.5 && window_gain(3.0, 0.0, 99) == 3.0 && window_gain(3.0, 1.0, 2) == 1.0, "gain 3");
  CHECK(window_gain(2.0, 0.5, 0) == 2.0 && window_gain(2.0, 0.5, 3) == 1.0 && window_gain(2.0, 0.0, 99) == 2.0, "gain 2");
  std::printf("schedule ok: %lld launches, %lld window positions, %lld checks\n", launches, positions, g_checks);
  return 0;
}
