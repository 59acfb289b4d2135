// csrc/acf.h and the autocovariance cut of csrc/schedule.h against brute force.  Plain C++, its own main:
// tests/test_acf_host.py compiles it with g++ -fsanitize=address,undefined and runs it.
//  1. snapshot number and slot arithmetic against a step-by-step replay of a run that counts its snapshots and keeps a ring
//     of snapshot numbers, for burn_in that is and is not a multiple of `every`: the number comes from the step counter alone,
//     the slot of every available lag holds exactly snapshot j - k, and the slot written is the one of lag max_lag;
//  2. the lags available before and after the ring first fills, and the pair counts a run of n snapshots ends with;
//  3. the cuts ptrwm_run_with_autocorr makes (steps_to_next_due of both periods min-ed into launch_at's cap) replayed step by
//     step with a histogram bound at a different period: every due step of either period ends a launch, no launch holds one
//     before its last step, and a request without a due step is cut as a plain one;
//  4. acf_geometry - how the snapshot kernel's grid tiles the td = temps * dim covered columns - for every td the C ABI can ask
//     for (1..256 * 104): the group fits the workgroup, the groups cover the columns exactly and are as equal as they come, the
//     chains in flight fit the workgroup, the tile is what the threads hold.
// With the argument "geometry" it reads td values from stdin and prints "cols groups per chains last_cols" for each; with
// "cuts step0 n_steps burn_in acf_every hist_every cap" it prints one line "step0 n acf hist" per launch.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../rwm-pt-pytorch_amd/csrc/acf.h"

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

static bool due(long long sc, long long burn_in, long long period) { return sc > burn_in && sc % period == 0; }

static void test_numbers_and_slots() {
  long long snapshots = 0;
  for (long long every : {1ll, 3ll, 7ll, 10ll})
    for (long long burn_in : {0ll, 7ll, 11ll, 20ll, 21ll, 30ll})  // (multiples of some periods, of none of others)
      for (int max_lag : {1, 2, 5, 32}) {
        std::vector<long long> ring((size_t)max_lag, -1);  // the snapshot number every slot holds
        std::vector<long long> pairs((size_t)max_lag + 1, 0);
        long long count = 0;  // the replay COUNTS its snapshots
        for (long long sc = 1; sc <= burn_in + every * (3 * max_lag + 3) + 5; ++sc) {
          CHECK(periodic_step_due(sc, burn_in, every) == due(sc, burn_in, every), "sc %lld", sc);
          if (!due(sc, burn_in, every)) continue;
          const long long j = periodic_step_number(sc, burn_in, every);
          CHECK(j == count, "step counter %lld (burn_in %lld, every %lld) is snapshot %lld, the rule says %lld", sc, burn_in, every, count, j);
          CHECK(swap_event_number(sc, burn_in, every) == j, "one expression for swap events and snapshots");
          const int lags = acf_lags(j, max_lag);
          CHECK(lags == (j < max_lag ? (int)j : max_lag), "snapshot %lld: %d lags", j, lags);
          for (int k = 1; k <= lags; ++k) {
            const int s = acf_lag_slot(j, k, max_lag);
            CHECK(s >= 0 && s < max_lag, "slot %d outside the ring of %d", s, max_lag);
            CHECK(ring[(size_t)s] == j - k, "snapshot %lld lag %d: slot %d holds snapshot %lld", j, k, s, ring[(size_t)s]);
          }
          if (lags < max_lag) CHECK(ring[(size_t)acf_slot(j, max_lag)] == -1, "before the ring fills the slot written is a fresh one");
          if (j >= max_lag) CHECK(acf_slot(j, max_lag) == acf_lag_slot(j, max_lag, max_lag), "the slot written is the one of lag max_lag");
          for (int k = 0; k <= lags; ++k) pairs[(size_t)k] += 1;
          ring[(size_t)acf_slot(j, max_lag)] = j;  // ... only after every lag has been read
          ++count;
          ++snapshots;
        }
        // n snapshots leave n - k pairs at lag k
        for (int k = 0; k <= max_lag; ++k)
          CHECK(pairs[(size_t)k] == (count - k > 0 ? count - k : 0), "lag %d: %lld pairs after %lld snapshots", k, pairs[(size_t)k], count);
        CHECK(count >= 3 * max_lag + 2, "the replay must wrap the ring several times");
      }
  CHECK(acf_lags(0, 32) == 0 && acf_lags(31, 32) == 31 && acf_lags(32, 32) == 32 && acf_lags(1000000, 32) == 32, "lags around the first fill");
  CHECK(acf_lags(5, 1) == 1 && acf_lag_slot(5, 1, 1) == 0 && acf_slot(5, 1) == 0, "a ring of one slot");
  CHECK(acf_term(3.0, -7.0) == -21.0 && acf_term(0.1, 0.1) == 0.1 * 0.1, "a term is the plain double product");
  CHECK(snapshots > 1000, "the grid must take snapshots");
}

struct Cut {
  long long step0, n;
  bool acf, hist;
};

// the loop of run_impl with both snapshot kernels bound (hist_every = 0: no histogram)
static std::vector<Cut> cuts(long long step0, long long n_steps, long long burn_in, long long acf_every, long long hist_every, long long cap) {
  const StepRequest req = {step0, n_steps, burn_in, 3, 0, 1, 0, 1};
  std::vector<Cut> out;
  for (long long done = 0; done < n_steps;) {
    long long to_snap = hist_every > 0 ? steps_to_next_due(step0 + done, burn_in, hist_every) : cap;
    if (acf_every > 0) {
      const long long t = steps_to_next_due(step0 + done, burn_in, acf_every);
      if (t < to_snap) to_snap = t;
    }
    const LaunchCut cut = launch_at(req, done, to_snap < cap ? to_snap : cap);
    out.push_back({cut.step0, cut.n, acf_every > 0 && due(cut.step0 + cut.n, burn_in, acf_every),
                   hist_every > 0 && due(cut.step0 + cut.n, burn_in, hist_every)});
    done += cut.n;
  }
  return out;
}

static void test_cuts() {
  long long launches = 0;
  for (long long every : {1ll, 3ll, 7ll})
    for (long long hist_every : {0ll, 2ll, 5ll, 7ll})
      for (long long burn_in : {0ll, 7ll, 11ll, 25ll})
        for (long long step0 : {0ll, 1ll, 4ll, 13ll, 29ll})
          for (long long n_steps : {1ll, 2ll, 9ll, 60ll})
            for (long long cap : {1ll, 4ll, 1000ll}) {
              const std::vector<Cut> cs = cuts(step0, n_steps, burn_in, every, hist_every, cap);
              long long at = step0, snaps = 0, hsnaps = 0, expect_j = -1;
              for (const Cut &c : cs) {
                CHECK(c.step0 == at, "launches must follow each other");
                CHECK(c.n >= 1 && c.n <= cap && at + c.n <= step0 + n_steps, "a launch of %lld steps", c.n);
                for (long long i = 1; i < c.n; ++i) {
                  CHECK(!due(c.step0 + i, burn_in, every), "step counter %lld is due but lies inside a launch", c.step0 + i);
                  CHECK(hist_every == 0 || !due(c.step0 + i, burn_in, hist_every), "a histogram step inside a launch");
                }
                CHECK(c.acf || c.hist || c.n == cap || at + c.n == step0 + n_steps, "a launch ends early for no reason");
                if (c.acf) {  // every due step, in order
                  const long long j = periodic_step_number(c.step0 + c.n, burn_in, every);
                  CHECK(expect_j < 0 || j == expect_j + 1, "snapshot %lld follows snapshot %lld", j, expect_j);
                  expect_j = j;
                }
                snaps += c.acf;
                hsnaps += c.hist;
                at += c.n;
                ++launches;
              }
              CHECK(at == step0 + n_steps, "the launches must cover the request");
              CHECK(snaps == periodic_steps_in(step0, n_steps, burn_in, every), "%lld snapshots", snaps);
              CHECK(hist_every == 0 || hsnaps == periodic_steps_in(step0, n_steps, burn_in, hist_every), "%lld histogram snapshots", hsnaps);
              // no due step of the autocovariance: exactly the launches of the same run without it
              if (snaps == 0) {
                const std::vector<Cut> plain = cuts(step0, n_steps, burn_in, 0, hist_every, cap);
                CHECK(plain.size() == cs.size(), "a request without a due step must be cut as before");
                for (size_t i = 0; i < cs.size(); ++i) CHECK(plain[i].step0 == cs[i].step0 && plain[i].n == cs[i].n, "... launch %zu", i);
              }
            }
  CHECK(launches > 1000, "the grid must make launches");
}

static void test_geometry() {
  const int max_td = 256 * 104;  // PTRWM_MAX_TEMPS * PTRWM_MAX_DIM of include/ptrwm.h
  long long n_multi = 0, n_shared = 0, n_idle = 0;
  for (int td = 1; td <= max_td; ++td) {
    const AcfGeometry g = acf_geometry(td);
    CHECK(g.cols >= 1 && g.cols <= kAcfThreads && g.cols <= td, "td %d: cols %d", td, g.cols);
    CHECK(g.groups >= 1 && g.groups == (td + kAcfThreads - 1) / kAcfThreads, "td %d: %d groups", td, g.groups);
    CHECK((long long)(g.groups - 1) * g.cols < td && td <= (long long)g.groups * g.cols, "td %d: %d groups of %d", td, g.groups, g.cols);
    CHECK((long long)g.groups * (g.cols - 1) < td, "td %d: groups of %d are wider than they need be", td, g.cols);
    const int last = td - (g.groups - 1) * g.cols;
    CHECK(last >= 1 && last <= g.cols && g.cols - last < g.groups, "td %d: a last group of %d of %d", td, last, g.cols);
    CHECK(g.per >= 1 && g.per * g.cols <= kAcfThreads && (g.per + 1) * g.cols > kAcfThreads, "td %d: %d chains of %d columns in flight", td, g.per, g.cols);
    CHECK(g.chains == g.per * kAcfChainsPerThread, "td %d: a tile of %d chains", td, g.chains);
    CHECK(g.groups == 1 || g.per == 1, "td %d: several groups are wide ones", td);
    n_multi += g.groups > 1;
    n_shared += g.per > 1;
    n_idle += g.per * g.cols < kAcfThreads;
  }
  CHECK(n_multi > 0 && n_shared > 0 && n_idle > 0, "the grid must reach several groups, shared columns and idle threads");
  const AcfGeometry cold30 = acf_geometry(30), one = acf_geometry(1), wide = acf_geometry(256), all = acf_geometry(32 * 30);
  CHECK(cold30.cols == 30 && cold30.per == 8 && cold30.groups == 1 && cold30.chains == 8 * kAcfChainsPerThread, "cold-only at dim 30");
  CHECK(one.cols == 1 && one.per == kAcfThreads, "the narrowest group");
  CHECK(wide.cols == 256 && wide.per == 1 && wide.groups == 1, "the widest group");
  CHECK(all.groups == 4 && all.cols == 240 && all.per == 1, "32 temperatures x dim 30");
  CHECK(kAcfThreads == 256 && kAcfMaxLag == 1024, "the kernel's workgroup and the ABI's lag limit");
}

int main(int argc, char **argv) {
  if (argc > 1 && std::strcmp(argv[1], "geometry") == 0) {
    int td;
    while (std::scanf("%d", &td) == 1) {
      const AcfGeometry g = acf_geometry(td);
      std::printf("%d %d %d %d %d\n", g.cols, g.groups, g.per, g.chains, td - (g.groups - 1) * g.cols);
    }
    return 0;
  }
  if (argc == 8 && std::strcmp(argv[1], "cuts") == 0) {
    for (const Cut &c : cuts(std::atoll(argv[2]), std::atoll(argv[3]), std::atoll(argv[4]), std::atoll(argv[5]), std::atoll(argv[6]), std::atoll(argv[7])))
      std::printf("%lld %lld %d %d\n", c.step0, c.n, (int)c.acf, (int)c.hist);
    return 0;
  }
  test_numbers_and_slots();
  test_cuts();
  test_geometry();
  std::printf("acf ok: %lld checks\n", g_checks);
  return 0;
}
