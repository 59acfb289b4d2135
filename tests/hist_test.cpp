// csrc/hist.h and the histogram cut of csrc/schedule.h against brute force.  Plain C++, its own main:
// tests/test_hist_host.py compiles it with g++ -fsanitize=address,undefined and runs it.
//  1. hist_bin against a double-precision restatement with floor and explicit edge cases, over a grid of ranges and values
//     that holds lo, hi, their neighbours, +-inf, NaN and denormals, for n_bins in {1, 2, 7, 64, 1024};
//  2. steps_to_next_due, and the cuts ptrwm_run_with_histogram makes with it (min-ed into launch_at's cap), replayed step by
//     step: every launch ends on a due step or at the cap or at the request's end, holds no due step before its last, the
//     launches cover the request, none exceeds the cap;
//  3. hist_geometry - how the snapshot kernel's grid tiles the td = temps * dim covered columns - for every n_bins the C ABI
//     accepts (1..1024) and every td it can be asked for (1..256 * 104): the group fits the workgroup and the LDS counters,
//     the groups cover the columns exactly, and `direct` is taken exactly where fewer than kHistMinCols columns would fit.
// With the argument "geometry" it reads pairs "n_bins td" from stdin and prints "direct cols groups last_cols" for each
// (tests/test_hist_host.py: the geometry that each GPU case of tests/test_gpu_hist.py is named for).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../rwm-pt-pytorch_amd/csrc/hist.h"
#include "../rwm-pt-pytorch_amd/csrc/schedule.h"

using namespace ptrwm;

static long long g_checks = 0;
#define CHECK(cond, ...)                                     \
  do {                                                       \
    ++g_checks;                                              \
    if (!(cond)) {                                           \
      std::printf("FAILED %s (line %d): ", #cond, __LINE__); \
      std::printf(__VA_ARGS__);                              \
      std::printf("\n");                                     \
      std::exit(1);                                          \
    }                                                        \
  } while (0)

// The rule restated in double.  double holds the exact difference and the exact product of two floats' worth of bits
// whenever they matter (53 >= 2 * 24 + 2: rounding the double result to float equals the correctly rounded float operation),
// so u is the float the rule computes; the bin is then floor(u) with the edge cases spelled out.
static int reference_bin(float x, float lo, float scale, int n_bins) {
  if (std::isnan(x)) return 0;  // the header's choice: NaN is counted as underflow
  const volatile float d = (float)((double)x - (double)lo);
  const volatile float u = (float)((double)d * (double)scale);
  if (std::isnan(u)) return 0;  // (inf - inf, 0 * inf: not a number either)
  if (u < 0.0f) return 0;
  if (std::isinf(u) || (double)u >= (double)n_bins) return n_bins + 1;
  return 1 + (int)std::floor((double)u);
}

static void test_bin_rule() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float dmin = std::numeric_limits<float>::denorm_min(), fmin = std::numeric_limits<float>::min();
  const float ranges[][2] = {{-6.0f, 6.0f}, {0.0f, 1.0f}, {-20.0f, 20.0f}, {-15.5f, -14.5f}, {0.1f, 0.7f}, {-1e-3f, 3e4f},
                             {0.0f, 1e-30f}, {-1e-35f, 1e-35f}, {1e30f, 2e30f}};  // (each with a finite scale)
  const int bins[] = {1, 2, 7, 64, 1024};
  long long in_range = 0, n_under = 0, n_over = 0;
  for (const auto &r : ranges)
    for (int nb : bins) {
      const float lo = r[0], hi = r[1];
      const float scale = (float)nb / (hi - lo);  // as the Python layer computes it, in float
      std::vector<float> xs = {lo, std::nextafterf(lo, -inf), std::nextafterf(lo, inf), hi, std::nextafterf(hi, -inf),
                               std::nextafterf(hi, inf), inf, -inf, nan, -nan, 0.0f, -0.0f, dmin, -dmin, 7.0f * dmin, fmin,
                               -fmin, std::numeric_limits<float>::max(), -std::numeric_limits<float>::max()};
      const float w = (hi - lo) / (float)nb;
      for (int i = 0; i <= nb; i += (nb > 64 ? 37 : 1)) {  // every inner edge (a sample of them for 1024 bins) and its neighbours
        const float e = lo + (float)i * w;
        xs.push_back(e);
        xs.push_back(std::nextafterf(e, -inf));
        xs.push_back(std::nextafterf(e, inf));
        xs.push_back(e + 0.5f * w);
      }
      for (int i = -8; i <= 40; ++i) xs.push_back(lo + (hi - lo) * (float)i / 32.0f + 0.013f * w);
      int prev_bin = -1;
      float prev_x = -inf;
      for (float x : xs) {
        const int got = hist_bin(x, lo, scale, nb), want = reference_bin(x, lo, scale, nb);
        CHECK(got == want, "hist_bin(%a, lo %a, scale %a, %d bins) = %d, the restatement says %d", x, lo, scale, nb, got, want);
        CHECK(got >= 0 && got <= nb + 1, "bin %d outside 0..%d", got, nb + 1);
        (got == 0 ? n_under : (got == nb + 1 ? n_over : in_range)) += 1;
      }
      // what holds for every range: lo itself opens bin 1, NaN and -inf are underflow, +inf is overflow, and the rule is
      // monotone (walk the finite values in increasing order)
      CHECK(hist_bin(lo, lo, scale, nb) == 1, "x = lo must land in bin 1");
      CHECK(hist_bin(nan, lo, scale, nb) == 0 && hist_bin(-inf, lo, scale, nb) == 0, "NaN and -inf are underflow");
      CHECK(hist_bin(inf, lo, scale, nb) == nb + 1, "+inf is overflow");
      CHECK(hist_bin(std::nextafterf(hi, inf), lo, scale, nb) >= nb, "just above hi: the last bin or overflow");
      std::vector<float> sorted;
      for (float x : xs)
        if (std::isfinite(x)) sorted.push_back(x);
      for (size_t i = 1; i < sorted.size(); ++i)  // (insertion sort: a few hundred values)
        for (size_t j = i; j > 0 && sorted[j - 1] > sorted[j]; --j) std::swap(sorted[j - 1], sorted[j]);
      for (float x : sorted) {
        const int b = hist_bin(x, lo, scale, nb);
        CHECK(b >= prev_bin, "not monotone: %a -> bin %d after %a -> bin %d", x, b, prev_x, prev_bin);
        prev_bin = b;
        prev_x = x;
      }
    }
  // ranges with short binary fractions, where real arithmetic and the float rule agree on every edge
  for (int nb : {1, 2, 64, 1024}) {
    const float lo = -8.0f, hi = 8.0f, scale = (float)nb / (hi - lo);
    CHECK(hist_bin(hi, lo, scale, nb) == nb + 1, "x = hi is overflow");
    // (the float just below hi = 8 is 8 - 2^-21; minus lo = -8 that is 16 - 2^-21, a tie that rounds to 16: the rule is evaluated
    // in float and says overflow where real arithmetic says the last bin - one unit in the last place, as the header states)
    CHECK(hist_bin(std::nextafterf(hi, -inf), lo, scale, nb) == nb + 1, "just below hi = 8 with lo = -8: rounds into the overflow bin");
    CHECK(hist_bin(7.999f, lo, scale, nb) == nb, "a little further below hi: the last bin");
    CHECK(hist_bin(std::nextafterf(lo, -inf), lo, scale, nb) == 0, "just below lo: underflow");
    for (int i = 0; i < nb; ++i) CHECK(hist_bin(lo + (float)i * (16.0f / (float)nb), lo, scale, nb) == 1 + i, "edge %d opens bin %d", i, 1 + i);
  }
  CHECK(in_range > 1000 && n_under > 100 && n_over > 100, "the grid must reach every kind of bin");
}

static bool due(long long sc, long long burn_in, long long period) { return sc > burn_in && sc % period == 0; }

static void test_cuts() {
  long long launches = 0;
  for (long long every : {1ll, 3ll, 10ll})
    for (long long burn_in : {0ll, 7ll, 11ll, 25ll})       // (7, 11, 25: no multiple of 3 or 10)
      for (long long step0 : {0ll, 1ll, 4ll, 13ll, 29ll})  // (mid-period starts)
        for (long long n_steps : {1ll, 2ll, 9ll, 60ll})
          for (long long cap : {1ll, 4ll, 7ll, 1000ll}) {
            // the helper against the literal rule
            for (long long s = step0; s < step0 + 40; ++s) {
              long long want = 1;
              while (!due(s + want, burn_in, every)) ++want;
              CHECK(steps_to_next_due(s, burn_in, every) == want, "steps_to_next_due(%lld, %lld, %lld) = %lld, brute force %lld", s,
                    burn_in, every, steps_to_next_due(s, burn_in, every), want);
            }
            // the loop of run_impl
            const StepRequest req = {step0, n_steps, burn_in, 3, 0, 1, 0, 1};
            long long done = 0, snapshots = 0;
            while (done < n_steps) {
              const long long to_snap = steps_to_next_due(step0 + done, burn_in, every);
              const LaunchCut cut = launch_at(req, done, to_snap < cap ? to_snap : cap);
              CHECK(cut.step0 == step0 + done, "launches must follow each other");
              CHECK(cut.n >= 1 && cut.n <= cap, "a launch of %d steps under a cap of %lld", cut.n, cap);
              CHECK(done + cut.n <= n_steps, "a launch runs past the request");
              for (long long i = 1; i < cut.n; ++i)
                CHECK(!due(cut.step0 + i, burn_in, every), "step counter %lld is due but lies inside a launch", cut.step0 + i);
              const bool ends_due = due(cut.step0 + cut.n, burn_in, every);
              CHECK(ends_due || cut.n == cap || done + cut.n == n_steps, "a launch ends early for no reason");
              snapshots += ends_due ? 1 : 0;
              done += cut.n;
              ++launches;
            }
            CHECK(done == n_steps, "the launches must cover the request");
            CHECK(snapshots == periodic_steps_in(step0, n_steps, burn_in, every), "%lld snapshots, %lld due steps", snapshots,
                  periodic_steps_in(step0, n_steps, burn_in, every));
            // a request without a due step: exactly the launches of a run without histograms
            if (periodic_steps_in(step0, n_steps, burn_in, every) == 0) {
              long long a = 0, b = 0;
              while (a < n_steps) {
                const long long to_snap = steps_to_next_due(step0 + a, burn_in, every);
                const LaunchCut with = launch_at(req, a, to_snap < cap ? to_snap : cap), without = launch_at(req, b, cap);
                CHECK(with.step0 == without.step0 && with.n == without.n, "a request without a due step must be cut as before");
                a += with.n;
                b += without.n;
              }
            }
          }
  CHECK(launches > 1000, "the grid must make launches");
}

static void test_geometry() {
  const int max_td = 256 * 104;  // PTRWM_MAX_TEMPS * PTRWM_MAX_DIM of include/ptrwm.h
  long long n_direct = 0, n_lds = 0, n_multi = 0, n_narrow_last = 0;
  for (int nb = 1; nb <= kHistMaxBins; ++nb)
    for (int td = 1; td <= max_td; ++td) {
      const HistGeometry g = hist_geometry(nb, td);
      const bool direct = g.direct != 0;
      CHECK(g.cols >= 1 && g.cols <= 256, "%d bins, td %d: cols %d", nb, td, g.cols);
      CHECK(g.cols <= td, "%d bins, td %d: cols %d above td", nb, td, g.cols);
      CHECK(direct || g.cols * (nb + 2) <= kHistLdsCounters, "%d bins, td %d: %d columns do not fit the LDS counters", nb, td, g.cols);
      CHECK(direct || g.cols >= (kHistMinCols < td ? kHistMinCols : td), "%d bins, td %d: an LDS group of %d columns", nb, td, g.cols);
      CHECK((long long)(g.groups - 1) * g.cols < td && td <= (long long)g.groups * g.cols, "%d bins, td %d: %d groups of %d", nb, td, g.groups, g.cols);
      CHECK(direct == (nb + 2 > kHistLdsCounters / kHistMinCols), "%d bins: direct %d", nb, g.direct);
      (direct ? n_direct : n_lds) += 1;
      n_multi += g.groups > 1;
      n_narrow_last += g.groups > 1 && td % g.cols != 0;
    }
  CHECK(n_direct > 0 && n_lds > 0 && n_multi > 0 && n_narrow_last > 0, "the grid must reach both strategies and several groups");
  CHECK(kHistChains == 256 && kHistMaxCols == 256, "the kernel's workgroup is 256 threads: tile and widest group");
}

static int print_geometry() {
  int nb, td;
  while (std::scanf("%d %d", &nb, &td) == 2) {
    const HistGeometry g = hist_geometry(nb, td);
    std::printf("%d %d %d %d\n", g.direct, g.cols, g.groups, td - (g.groups - 1) * g.cols);
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc > 1 && std::strcmp(argv[1], "geometry") == 0) return print_geometry();
  test_bin_rule();
  test_cuts();
  test_geometry();
  std::printf("hist ok: %lld checks\n", g_checks);
  return 0;
}
