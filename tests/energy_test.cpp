// CPU checks of csrc/energy.h (plain C++, no HIP): the pooled log-density sums along the ladder.
//  1. the ordering of floats as integers that the ref kernel's maximum rests on, and the finite test;
//  2. a CPU replay of the snapshot kernel's tiling - workgroups by (group, tile), threads walking elements with the kernel's
//     incremental (temperature, chain) pair, partial sums parked in a per-workgroup table - against brute force: every (c, t)
//     has exactly one owner, no pad lane contributes, a chain lands in the group of its global id, and count / s1 / s2 on
//     integer log-densities are equal, for every n_temps in 1..256 and groups in {1, 3, 16, 64};
//  3. the cuts ptrwm_run_with_energy makes (steps_to_next_due of the periods min-ed into launch_at's cap) replayed step by step
//     with a covariance and a histogram bound at other periods.
// With the argument "geometry" it reads "n_temps n_chains groups chain_offset" lines from stdin and prints "tile_chains tiles
// max_members min_members last_tile_chains lds_doubles threads tile_elems" for each; with "cuts step0 n_steps burn_in
// energy_every cov_every hist_every cap" it prints one line "step0 n energy cov hist" per launch.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../rwm-pt-pytorch_amd/csrc/energy.h"

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

static void test_keys() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float v[] = {-inf, -3.4e38f, -1e6f, -1.5f, -1e-45f, -0.0f, 0.0f, 1e-45f, 1.0f, 2.5f, 1e6f, 3.4e38f, inf};
  const int n = (int)(sizeof v / sizeof v[0]);
  for (int i = 0; i < n; ++i) {
    CHECK(energy_key(v[i]) != kEnergyNoKey, "value %d has the key that means none", i);
    CHECK(energy_key_value(energy_key(v[i])) == v[i] && std::signbit(energy_key_value(energy_key(v[i]))) == std::signbit(v[i]), "value %d comes back", i);
    CHECK(energy_finite(v[i]) == (i != 0 && i != n - 1), "value %d: finite", i);
    if (i > 0) CHECK(energy_key(v[i - 1]) < energy_key(v[i]), "keys %d and %d must be ordered as the values", i - 1, i);
  }
  CHECK(!energy_finite(nan) && !energy_finite(-nan), "a NaN is not finite");
  CHECK(energy_ref_of(kEnergyNoKey) == 0.0 && energy_ref_of(energy_key(-1e6f)) == -1e6, "ref from a key");
  CHECK(energy_exp_arg(0.5f, 0.25f, 3.0, 1.0) == 0.5, "the argument of exp");
}

// one snapshot of integer log-densities replayed as energy_snapshot_kernel walks it; l[c * T + t], not finite where `hole`
static long long g_elements = 0;
static void replay(int T, long long n_chains, long long offset, int G) {
  std::vector<int> owners((size_t)(n_chains * T), 0);
  std::vector<long long> count((size_t)G * T, 0), s1((size_t)G * T, 0), s2((size_t)G * T, 0), bcount(count), bs1(s1), bs2(s2);
  long long bad = 0, bbad = 0;
  const auto value = [&](long long c, int t) { return (long long)((c * 7 + t * 3 + offset) % 23) - 11; };
  const auto hole = [&](long long c, int t) { return (c * 5 + t) % 17 == 3; };
  for (long long c = 0; c < n_chains; ++c)
    for (int t = 0; t < T; ++t) {
      const int g = energy_group(offset, c, G);
      CHECK(g >= 0 && g < G && g == (int)(((offset + c) % G + G) % G), "the group of chain %lld", c);
      if (hole(c, t)) {
        ++bbad;
        continue;
      }
      const long long x = value(c, t);
      bcount[(size_t)g * T + t] += 1, bs1[(size_t)g * T + t] += x, bs2[(size_t)g * T + t] += x * x;
    }
  const EnergyGeometry geo = energy_geometry(T, n_chains, offset, G);
  CHECK(geo.tile_chains == energy_tile_chains(T) && geo.tile_chains >= 1 && (long long)geo.tile_chains * T <= (kEnergyTileElems > T ? kEnergyTileElems : T),
        "T %d: a tile of %d chains", T, geo.tile_chains);
  CHECK(geo.lds_doubles == 4 * T && geo.groups == G, "T %d: the table", T);
  long long members_total = 0;
  for (int g = 0; g < G; ++g) {
    const long long members = energy_group_chains(n_chains, offset, G, g), first = energy_first_chain(offset, G, g);
    members_total += members;
    CHECK(first >= 0 && first < G && energy_group(offset, first, G) == g, "group %d starts at chain %lld", g, first);
    CHECK(members <= geo.max_members && members >= geo.min_members, "group %d: %lld chains", g, members);
    CHECK((geo.tiles - 1) * geo.tile_chains < geo.max_members || geo.max_members == 0, "a whole row of empty tiles");
    for (long long tile = 0; tile < geo.tiles; ++tile) {  // one workgroup
      const int n = energy_tile_elems(tile, members, T);
      CHECK(n >= 0 && n % T == 0 && n <= geo.tile_chains * T, "tile %lld: %d elements", tile, n);
      if (n == 0) {
        CHECK(members <= tile * geo.tile_chains, "an empty tile in front of the group's last chain");
        continue;
      }
      std::vector<long long> l_cnt((size_t)T, 0), l_s1((size_t)T, 0), l_s2((size_t)T, 0);
      long long l_bad = 0;
      const long long m0 = tile * energy_tile_chains(T);
      const int stride_t = kEnergyThreads % T, stride_k = kEnergyThreads / T;
      for (int tid = 0; tid < kEnergyThreads; ++tid) {
        int t = tid % T, k = tid / T, cur = t;
        long long cnt = 0, v1 = 0, v2 = 0;
        const auto park = [&]() { l_cnt[(size_t)cur] += cnt, l_s1[(size_t)cur] += v1, l_s2[(size_t)cur] += v2; };
        for (int e = tid; e < n; e += kEnergyThreads) {
          CHECK(t == energy_elem_temp(e, T) && m0 + k == energy_elem_member(tile, e, T), "element %d: (%d, %d)", e, t, k);
          if (t != cur) {
            park();
            cur = t, cnt = v1 = v2 = 0;
          }
          const long long c = energy_member_chain(offset, G, g, m0 + k);
          CHECK(m0 + k < members && c >= 0 && c < n_chains && energy_group(offset, c, G) == g, "chain %lld of group %d", c, g);
          ++owners[(size_t)(c * T + t)];
          ++g_elements;
          if (hole(c, t)) {
            ++l_bad;
          } else {
            const long long x = value(c, t);
            ++cnt, v1 += x, v2 += x * x;
          }
          t += stride_t, k += stride_k;
          if (t >= T) t -= T, ++k;
        }
        park();
      }
      for (int t = 0; t < T; ++t)  // the flush
        count[(size_t)g * T + t] += l_cnt[(size_t)t], s1[(size_t)g * T + t] += l_s1[(size_t)t], s2[(size_t)g * T + t] += l_s2[(size_t)t];
      bad += l_bad;
    }
  }
  CHECK(members_total == n_chains, "the groups must partition the chains");
  for (size_t i = 0; i < owners.size(); ++i) CHECK(owners[i] == 1, "T %d G %d: element %zu has %d owners", T, G, i, owners[i]);
  CHECK(count == bcount && s1 == bs1 && s2 == bs2 && bad == bbad, "T %d chains %lld offset %lld G %d: the sums", T, n_chains, offset, G);
}

static void test_replay() {
  int two_tiles = 0;
  for (int T = 1; T <= kEnergyMaxTemps; ++T)
    for (int G : {1, 3, 16, 64}) {
      replay(T, 70 + T % 7, 5, G);  // one tile, most groups uneven; with 64 groups some chains short of a second member
      if (T % 16 == 1) replay(T, 3, 0, G);  // fewer chains than groups
      // a second, partial tile for the largest group: all T with few groups, a handful of T with many
      const bool few = G <= 3, picked = T == 1 || T == 2 || T == 4 || T == 32 || T == 65 || T == 255 || T == 256;
      if (few || picked) {
        const long long n = (long long)G * energy_tile_chains(T) + 2 * G + 1;
        const EnergyGeometry geo = energy_geometry(T, n, 7, G);
        CHECK(geo.tiles == 2 && geo.last_tile_chains < geo.tile_chains && geo.last_tile_chains >= 1, "T %d G %d: %lld tiles", T, G, geo.tiles);
        replay(T, n, 7, G);
        ++two_tiles;
      }
    }
  CHECK(two_tiles == 2 * 256 + 2 * 7, "the grid of two-tile replays");
  replay(5, 40, -3, 16);  // (a negative global id: the mathematical mod)
}

struct Cut {
  long long step0, n;
  bool energy, cov, hist;
};

// the loop of run_impl with the snapshot kernels bound (a period of 0: that block is not bound)
static std::vector<Cut> cuts(long long step0, long long n_steps, long long burn_in, long long energy_every, long long cov_every,
                             long long hist_every, long long cap) {
  const StepRequest req = {step0, n_steps, burn_in, 3, 0, 1, 0, 1};
  std::vector<Cut> out;
  for (long long done = 0; done < n_steps;) {
    long long to_snap = cap;
    for (long long every : {hist_every, cov_every, energy_every})
      if (every > 0) {
        const long long t = steps_to_next_due(step0 + done, burn_in, every);
        if (t < to_snap) to_snap = t;
      }
    const LaunchCut cut = launch_at(req, done, to_snap < cap ? to_snap : cap);
    out.push_back({cut.step0, cut.n, energy_every > 0 && due(cut.step0 + cut.n, burn_in, energy_every),
                   cov_every > 0 && due(cut.step0 + cut.n, burn_in, cov_every), hist_every > 0 && due(cut.step0 + cut.n, burn_in, hist_every)});
    done += cut.n;
  }
  return out;
}

static void test_cuts() {
  long long launches = 0;
  for (long long every : {1ll, 3ll, 7ll})
    for (long long cov_every : {0ll, 2ll, 4ll})
      for (long long hist_every : {0ll, 5ll})
        for (long long burn_in : {0ll, 7ll, 11ll, 25ll})
          for (long long step0 : {0ll, 1ll, 4ll, 13ll, 29ll})
            for (long long n_steps : {1ll, 2ll, 9ll, 60ll})
              for (long long cap : {1ll, 4ll, 1000ll}) {
                const std::vector<Cut> cs = cuts(step0, n_steps, burn_in, every, cov_every, hist_every, cap);
                long long at = step0, snaps = 0, csnaps = 0, hsnaps = 0;
                for (const Cut &c : cs) {
                  CHECK(c.step0 == at, "launches must follow each other");
                  CHECK(c.n >= 1 && c.n <= cap && at + c.n <= step0 + n_steps, "a launch of %lld steps", c.n);
                  for (long long i = 1; i < c.n; ++i) {
                    CHECK(!due(c.step0 + i, burn_in, every), "step counter %lld is due but lies inside a launch", c.step0 + i);
                    CHECK(cov_every == 0 || !due(c.step0 + i, burn_in, cov_every), "a covariance step inside a launch");
                    CHECK(hist_every == 0 || !due(c.step0 + i, burn_in, hist_every), "a histogram step inside a launch");
                  }
                  CHECK(c.energy || c.cov || c.hist || c.n == cap || at + c.n == step0 + n_steps, "a launch ends early for no reason");
                  snaps += c.energy;
                  csnaps += c.cov;
                  hsnaps += c.hist;
                  at += c.n;
                  ++launches;
                }
                CHECK(at == step0 + n_steps, "the launches must cover the request");
                CHECK(snaps == periodic_steps_in(step0, n_steps, burn_in, every), "%lld snapshots", snaps);
                CHECK(cov_every == 0 || csnaps == periodic_steps_in(step0, n_steps, burn_in, cov_every), "%lld covariance snapshots", csnaps);
                CHECK(hist_every == 0 || hsnaps == periodic_steps_in(step0, n_steps, burn_in, hist_every), "%lld histogram snapshots", hsnaps);
                // no due step of the log-density sums: exactly the launches of the same run without them
                if (snaps == 0) {
                  const std::vector<Cut> plain = cuts(step0, n_steps, burn_in, 0, cov_every, hist_every, cap);
                  CHECK(plain.size() == cs.size(), "a request without a due step must be cut as before");
                  for (size_t i = 0; i < cs.size(); ++i) CHECK(plain[i].step0 == cs[i].step0 && plain[i].n == cs[i].n, "... launch %zu", i);
                }
              }
  CHECK(launches > 1000, "the grid must make launches");
}

int main(int argc, char **argv) {
  if (argc > 1 && std::strcmp(argv[1], "geometry") == 0) {
    int T, G;
    long long n, off;
    while (std::scanf("%d %lld %d %lld", &T, &n, &G, &off) == 4) {
      const EnergyGeometry g = energy_geometry(T, n, off, G);
      std::printf("%d %lld %lld %lld %d %d %d %d\n", g.tile_chains, g.tiles, g.max_members, g.min_members, g.last_tile_chains, g.lds_doubles,
                  kEnergyThreads, kEnergyTileElems);
    }
    return 0;
  }
  if (argc == 9 && std::strcmp(argv[1], "cuts") == 0) {
    for (const Cut &c : cuts(std::atoll(argv[2]), std::atoll(argv[3]), std::atoll(argv[4]), std::atoll(argv[5]), std::atoll(argv[6]),
                             std::atoll(argv[7]), std::atoll(argv[8])))
      std::printf("%lld %lld %d %d %d\n", c.step0, c.n, (int)c.energy, (int)c.cov, (int)c.hist);
    return 0;
  }
  test_keys();
  test_replay();
  test_cuts();
  std::printf("energy ok: %lld checks, %lld elements replayed\n", g_checks, g_elements);
  return 0;
}
