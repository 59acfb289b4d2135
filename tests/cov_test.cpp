// csrc/cov.h and the covariance cut of csrc/schedule.h against brute force.  Plain C++, its own main:
// tests/test_cov_host.py compiles it with g++ -fsanitize=address,undefined and runs it.
//  1. the geometry for every dim in 1..104: every (i, j) with j <= i < dim is owned by exactly one (wave, pair slot, lane,
//     register), no pad element is ever flushed, a wave's pairs fit its accumulators, every sx element has one owner; the
//     staging covers every (chain, coordinate) of a sub-tile once and stays inside its LDS row; a K-step's lanes read inside
//     the buffer;
//  2. a CPU replay of the snapshot kernel - staging through the LDS image, the block products in the matrix instruction's
//     operand and result layout, the flush - on integer states against the direct sums, for dims 1, 15, 16, 17, 30, 64, 70,
//     104 and chain counts 1, 3, 4, 5, 70 (and one count with a second, partial tile of chains);
//  3. the cuts ptrwm_run_with_covariance makes (steps_to_next_due of the three periods min-ed into launch_at's cap) replayed
//     step by step with a histogram and an autocovariance bound at other periods.
// With the argument "geometry" it reads dims from stdin and prints "blocks pairs stride lds_bytes chains sub_tile k waves" for
// each; with "cuts step0 n_steps burn_in cov_every acf_every hist_every cap" it prints one line "step0 n cov acf hist" per launch.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../rwm-pt-pytorch_amd/csrc/cov.h"

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

static void test_geometry() {
  static_assert(kCovThreads == 64 * kCovWaves && kCovChains == kCovSubTile * kCovSubTiles && kCovSubTile % kCovK == 0, "tiles");
  static_assert(kCovMaxBlocks == 7 && kCovMaxPairs == 28 && kCovPairsPerWave == 7, "the largest dim");
  for (int dim = 1; dim <= kCovMaxDim; ++dim) {
    const CovGeometry g = cov_geometry(dim);
    const int nb = g.blocks;
    CHECK(nb == (dim + 15) / 16 && cov_padded(dim) == 16 * nb && cov_padded(dim) >= dim && cov_padded(dim) - dim < 16, "dim %d: %d blocks", dim, nb);
    CHECK(g.pairs == nb * (nb + 1) / 2 && g.pairs <= kCovMaxPairs, "dim %d: %d pairs", dim, g.pairs);
    CHECK(g.stride >= cov_padded(dim) && g.stride % 16 == 0 && (g.stride / 16) % 2 == 1 && g.stride - cov_padded(dim) <= 16, "dim %d: stride %d", dim, g.stride);
    CHECK(g.lds_bytes == kCovSubTile * g.stride * 8 && g.lds_bytes <= 64 * 1024, "dim %d: %d bytes of LDS", dim, g.lds_bytes);
    // pairs: numbered without gaps, one (wave, slot) each
    std::vector<int> slot_used((size_t)kCovWaves * kCovPairsPerWave, 0);
    int next = 0;
    for (int bi = 0; bi < nb; ++bi)
      for (int bj = 0; bj <= bi; ++bj) {
        const int p = cov_pair_index(bi, bj);
        CHECK(p == next, "pair (%d, %d) is number %d, expected %d", bi, bj, p, next);
        CHECK(cov_pair_row(p) == bi && cov_pair_col(p) == bj, "pair %d is (%d, %d), not (%d, %d)", p, cov_pair_row(p), cov_pair_col(p), bi, bj);
        ++next;
        const int w = cov_pair_wave(p), s = cov_pair_slot(p);
        CHECK(w >= 0 && w < kCovWaves && s >= 0 && s < kCovPairsPerWave, "dim %d: pair %d on wave %d slot %d", dim, p, w, s);
        CHECK(slot_used[(size_t)w * kCovPairsPerWave + s]++ == 0, "dim %d: wave %d slot %d twice", dim, w, s);
        CHECK(cov_wave_pair(w, s) == p && s < cov_wave_pairs(w, g.pairs), "dim %d: wave %d slot %d holds pair %d", dim, w, s, p);
      }
    CHECK(next == g.pairs, "dim %d: %d pairs numbered", dim, next);
    int owned = 0;
    for (int w = 0; w < kCovWaves; ++w) {
      const int nq = cov_wave_pairs(w, g.pairs);
      CHECK(nq >= 0 && nq <= kCovPairsPerWave, "dim %d: wave %d owns %d pairs", dim, w, nq);
      for (int q = 0; q < kCovPairsPerWave; ++q) CHECK((q < nq) == (cov_wave_pair(w, q) < g.pairs), "dim %d: wave %d slot %d", dim, w, q);
      owned += nq;
    }
    CHECK(owned == g.pairs, "dim %d: the waves own %d of %d pairs", dim, owned, g.pairs);
    // flush: every (i, j), j <= i < dim, exactly once; nothing else
    const int P = cov_padded(dim);
    std::vector<int> owners((size_t)P * P, 0);
    for (int bi = 0; bi < nb; ++bi)
      for (int bj = 0; bj <= bi; ++bj)
        for (int lane = 0; lane < 64; ++lane)
          for (int reg = 0; reg < 4; ++reg) {
            const int i = cov_flush_i(bi, lane, reg), j = cov_flush_j(bj, lane);
            CHECK(i >= 16 * bi && i < 16 * bi + 16 && j >= 16 * bj && j < 16 * bj + 16, "dim %d: (%d, %d) outside block (%d, %d)", dim, i, j, bi, bj);
            if (cov_flushed(i, j, dim)) {
              CHECK(i < dim && j < dim && j <= i, "dim %d: pad or upper element (%d, %d) flushed", dim, i, j);
              ++owners[(size_t)i * P + j];
            }
          }
    for (int i = 0; i < P; ++i)
      for (int j = 0; j < P; ++j)
        CHECK(owners[(size_t)i * P + j] == (j <= i && i < dim ? 1 : 0), "dim %d: (%d, %d) has %d owners", dim, i, j, owners[(size_t)i * P + j]);
    // sx: one owner per coordinate, the wave of the diagonal pair
    std::vector<int> sx_owners((size_t)P, 0);
    for (int b = 0; b < nb; ++b) {
      CHECK(cov_sx_wave(b) == cov_pair_wave(cov_pair_index(b, b)), "sx of block %d", b);
      for (int lane = 0; lane < 64; ++lane)
        if (cov_sx_flushed(b, lane, dim)) ++sx_owners[(size_t)(16 * b + lane)];
    }
    for (int d = 0; d < P; ++d) CHECK(sx_owners[(size_t)d] == (d < dim ? 1 : 0), "dim %d: sx %d has %d owners", dim, d, sx_owners[(size_t)d]);
    // staging: every (chain, coordinate) of a sub-tile once, inside its row and the buffer; pad columns never written
    std::vector<int> written((size_t)kCovSubTile * g.stride, 0);
    for (int e = 0; e < kCovSubTile * dim; ++e) {
      const int ch = cov_stage_chain(e, dim), d = cov_stage_coord(e, dim);
      CHECK(ch >= 0 && ch < kCovSubTile && d >= 0 && d < dim, "dim %d: element %d is (%d, %d)", dim, e, ch, d);
      CHECK(e == 0 || ch * dim + d == e, "dim %d: consecutive elements are consecutive in a chain's row", dim);
      const int at = cov_lds_at(ch, d, dim);
      CHECK(at >= ch * g.stride && at < ch * g.stride + dim && at < cov_lds_doubles(dim), "dim %d: LDS offset %d", dim, at);
      ++written[(size_t)at];
    }
    for (int ch = 0; ch < kCovSubTile; ++ch)
      for (int d = 0; d < g.stride; ++d) CHECK(written[(size_t)ch * g.stride + d] == (d < dim ? 1 : 0), "dim %d: LDS (%d, %d)", dim, ch, d);
    // operands: the K-steps of a sub-tile take each chain once per coordinate, inside the padded row
    std::vector<int> taken((size_t)kCovSubTile * P, 0);
    for (int ks = 0; ks < kCovKSteps; ++ks)
      for (int b = 0; b < nb; ++b)
        for (int lane = 0; lane < 64; ++lane) {
          const int ch = cov_operand_chain(ks, lane), d = cov_operand_coord(b, lane);
          CHECK(ch >= 0 && ch < kCovSubTile && d >= 0 && d < P && d < g.stride, "dim %d: operand (%d, %d)", dim, ch, d);
          ++taken[(size_t)ch * P + d];
        }
    for (size_t k = 0; k < taken.size(); ++k) CHECK(taken[k] == 1, "dim %d: operand element %zu taken %d times", dim, k, taken[k]);
  }
  const CovGeometry h = cov_geometry(30), one = cov_geometry(1), top = cov_geometry(104), d64 = cov_geometry(64), d70 = cov_geometry(70);
  CHECK(h.blocks == 2 && h.pairs == 3 && h.stride == 48, "the headline's row: dim 30");
  CHECK(one.blocks == 1 && one.pairs == 1 && one.stride == 16, "dim 1");
  CHECK(d64.pairs == 10 && d70.pairs == 15 && d70.pairs > kCovWaves, "dims 64 and 70");
  CHECK(top.blocks == 7 && top.pairs == 28 && top.stride == 112 && top.lds_bytes == 28672, "the largest dim");
}

// deterministic small integers, |x| <= 9, no symmetry between coordinates or chains
static int state_at(long long c, int t, int d) {
  unsigned long long h = (unsigned long long)c * 2654435761ull + (unsigned long long)t * 40503ull + (unsigned long long)d * 97ull + 12345ull;
  h ^= h >> 13;
  h *= 0x9E3779B97F4A7C15ull;
  h ^= h >> 29;
  return (int)(h % 19ull) - 9;
}

// one snapshot of one temperature as the kernel takes it: workgroups of kCovChains chains, sub-tiles through an LDS image,
// the block products in the matrix instruction's layout (A[row = lane & 15][k = lane >> 4], B[k = lane >> 4][col = lane & 15],
// D[row = (lane >> 4) + 4 reg][col = lane & 15]), the flush
static void replay_snapshot(long long n_chains, int t, int dim, std::vector<double> &sxx, std::vector<double> &sx) {
  const CovGeometry g = cov_geometry(dim);
  const int nb = g.blocks;
  for (long long c0 = 0; c0 < n_chains; c0 += kCovChains) {
    std::vector<double> lds((size_t)cov_lds_doubles(dim), 0.0);  // (zeroed once: the pad columns)
    std::vector<double> acc((size_t)kCovWaves * kCovPairsPerWave * 64 * 4, 0.0), s((size_t)kCovMaxBlocks * 64, 0.0);
    for (int sub = 0; sub < kCovSubTiles; ++sub) {
      const long long cs = c0 + (long long)sub * kCovSubTile;
      if (cs >= n_chains) break;
      for (int e = 0; e < kCovSubTile * dim; ++e) {
        const int ch = cov_stage_chain(e, dim), d = cov_stage_coord(e, dim);
        lds[(size_t)cov_lds_at(ch, d, dim)] = cs + ch < n_chains ? (double)state_at(cs + ch, t, d) : 0.0;
      }
      for (int ks = 0; ks < kCovKSteps; ++ks)
        for (int bi = 0; bi < nb; ++bi) {
          for (int bj = 0; bj <= bi; ++bj) {
            const int p = cov_pair_index(bi, bj);
            double *a = &acc[((size_t)cov_pair_wave(p) * kCovPairsPerWave + cov_pair_slot(p)) * 256];
            double A[16][4], B[4][16];
            for (int lane = 0; lane < 64; ++lane) {
              const int row = cov_operand_chain(ks, lane) * g.stride;
              A[lane & 15][lane >> 4] = lds[(size_t)(row + cov_operand_coord(bi, lane))];
              B[lane >> 4][lane & 15] = lds[(size_t)(row + cov_operand_coord(bj, lane))];
            }
            for (int lane = 0; lane < 64; ++lane)
              for (int reg = 0; reg < 4; ++reg)
                for (int k = 0; k < kCovK; ++k) a[lane * 4 + reg] += A[(lane >> 4) + 4 * reg][k] * B[k][lane & 15];
          }
          for (int lane = 0; lane < 64; ++lane)
            s[(size_t)bi * 64 + lane] += lds[(size_t)(cov_operand_chain(ks, lane) * g.stride + cov_operand_coord(bi, lane))];
        }
    }
    for (int bi = 0; bi < nb; ++bi) {
      for (int bj = 0; bj <= bi; ++bj) {
        const int p = cov_pair_index(bi, bj);
        const double *a = &acc[((size_t)cov_pair_wave(p) * kCovPairsPerWave + cov_pair_slot(p)) * 256];
        for (int lane = 0; lane < 64; ++lane)
          for (int reg = 0; reg < 4; ++reg) {
            const int i = cov_flush_i(bi, lane, reg), j = cov_flush_j(bj, lane);
            if (cov_flushed(i, j, dim)) sxx[(size_t)i * dim + j] += a[lane * 4 + reg];
          }
      }
      for (int lane = 0; lane < 64; ++lane)
        if (cov_sx_flushed(bi, lane, dim)) {
          const double *q = &s[(size_t)bi * 64];
          sx[(size_t)(16 * bi + lane)] += q[lane] + q[lane + 16] + q[lane + 32] + q[lane + 48];
        }
    }
  }
}

static void test_replay() {
  const double sentinel = -12345.5;
  long long cases = 0;
  for (int dim : {1, 15, 16, 17, 30, 64, 70, 104})
    for (long long n_chains : {1ll, 3ll, 4ll, 5ll, 70ll, (long long)kCovChains + kCovSubTile + 3}) {
      const int t = (int)(n_chains % 3);
      std::vector<double> sxx((size_t)dim * dim, sentinel), sx((size_t)dim, 0.0);
      for (int i = 0; i < dim; ++i)
        for (int j = 0; j <= i; ++j) sxx[(size_t)i * dim + j] = 0.0;
      replay_snapshot(n_chains, t, dim, sxx, sx);
      for (int i = 0; i < dim; ++i) {
        double want_s = 0.0;
        for (long long c = 0; c < n_chains; ++c) want_s += state_at(c, t, i);
        CHECK(sx[(size_t)i] == want_s, "dim %d, %lld chains: sx[%d] = %g, want %g", dim, n_chains, i, sx[(size_t)i], want_s);
        for (int j = 0; j < dim; ++j) {
          double want = sentinel;
          if (j <= i) {
            want = 0.0;
            for (long long c = 0; c < n_chains; ++c) want += (double)state_at(c, t, i) * state_at(c, t, j);
          }
          CHECK(sxx[(size_t)i * dim + j] == want, "dim %d, %lld chains: sxx[%d, %d] = %g, want %g", dim, n_chains, i, j, sxx[(size_t)i * dim + j], want);
        }
      }
      ++cases;
    }
  CHECK(cases == 48, "the grid of replays");
}

struct Cut {
  long long step0, n;
  bool cov, acf, hist;
};

// the loop of run_impl with the three snapshot kernels bound (a period of 0: that block is not bound)
static std::vector<Cut> cuts(long long step0, long long n_steps, long long burn_in, long long cov_every, long long acf_every,
                             long long hist_every, long long cap) {
  const StepRequest req = {step0, n_steps, burn_in, 3, 0, 1, 0, 1};
  std::vector<Cut> out;
  for (long long done = 0; done < n_steps;) {
    long long to_snap = cap;
    for (long long every : {hist_every, acf_every, cov_every})
      if (every > 0) {
        const long long t = steps_to_next_due(step0 + done, burn_in, every);
        if (t < to_snap) to_snap = t;
      }
    const LaunchCut cut = launch_at(req, done, to_snap < cap ? to_snap : cap);
    out.push_back({cut.step0, cut.n, cov_every > 0 && due(cut.step0 + cut.n, burn_in, cov_every),
                   acf_every > 0 && due(cut.step0 + cut.n, burn_in, acf_every), hist_every > 0 && due(cut.step0 + cut.n, burn_in, hist_every)});
    done += cut.n;
  }
  return out;
}

static void test_cuts() {
  long long launches = 0;
  for (long long every : {1ll, 3ll, 7ll})
    for (long long acf_every : {0ll, 2ll, 7ll})
      for (long long hist_every : {0ll, 5ll})
        for (long long burn_in : {0ll, 7ll, 11ll, 25ll})
          for (long long step0 : {0ll, 1ll, 4ll, 13ll, 29ll})
            for (long long n_steps : {1ll, 2ll, 9ll, 60ll})
              for (long long cap : {1ll, 4ll, 1000ll}) {
                const std::vector<Cut> cs = cuts(step0, n_steps, burn_in, every, acf_every, hist_every, cap);
                long long at = step0, snaps = 0, asnaps = 0, hsnaps = 0;
                for (const Cut &c : cs) {
                  CHECK(c.step0 == at, "launches must follow each other");
                  CHECK(c.n >= 1 && c.n <= cap && at + c.n <= step0 + n_steps, "a launch of %lld steps", c.n);
                  for (long long i = 1; i < c.n; ++i) {
                    CHECK(!due(c.step0 + i, burn_in, every), "step counter %lld is due but lies inside a launch", c.step0 + i);
                    CHECK(acf_every == 0 || !due(c.step0 + i, burn_in, acf_every), "an autocovariance step inside a launch");
                    CHECK(hist_every == 0 || !due(c.step0 + i, burn_in, hist_every), "a histogram step inside a launch");
                  }
                  CHECK(c.cov || c.acf || c.hist || c.n == cap || at + c.n == step0 + n_steps, "a launch ends early for no reason");
                  snaps += c.cov;
                  asnaps += c.acf;
                  hsnaps += c.hist;
                  at += c.n;
                  ++launches;
                }
                CHECK(at == step0 + n_steps, "the launches must cover the request");
                CHECK(snaps == periodic_steps_in(step0, n_steps, burn_in, every), "%lld snapshots", snaps);
                CHECK(acf_every == 0 || asnaps == periodic_steps_in(step0, n_steps, burn_in, acf_every), "%lld autocovariance snapshots", asnaps);
                CHECK(hist_every == 0 || hsnaps == periodic_steps_in(step0, n_steps, burn_in, hist_every), "%lld histogram snapshots", hsnaps);
                // no due step of the covariance: exactly the launches of the same run without it
                if (snaps == 0) {
                  const std::vector<Cut> plain = cuts(step0, n_steps, burn_in, 0, acf_every, hist_every, cap);
                  CHECK(plain.size() == cs.size(), "a request without a due step must be cut as before");
                  for (size_t i = 0; i < cs.size(); ++i) CHECK(plain[i].step0 == cs[i].step0 && plain[i].n == cs[i].n, "... launch %zu", i);
                }
              }
  CHECK(launches > 1000, "the grid must make launches");
}

int main(int argc, char **argv) {
  if (argc > 1 && std::strcmp(argv[1], "geometry") == 0) {
    int dim;
    while (std::scanf("%d", &dim) == 1) {
      const CovGeometry g = cov_geometry(dim);
      std::printf("%d %d %d %d %d %d %d %d\n", g.blocks, g.pairs, g.stride, g.lds_bytes, g.chains, kCovSubTile, kCovK, kCovWaves);
    }
    return 0;
  }
  if (argc == 9 && std::strcmp(argv[1], "cuts") == 0) {
    for (const Cut &c : cuts(std::atoll(argv[2]), std::atoll(argv[3]), std::atoll(argv[4]), std::atoll(argv[5]), std::atoll(argv[6]),
                             std::atoll(argv[7]), std::atoll(argv[8])))
      std::printf("%lld %lld %d %d %d\n", c.step0, c.n, (int)c.cov, (int)c.acf, (int)c.hist);
    return 0;
  }
  test_geometry();
  test_replay();
  test_cuts();
  std::printf("cov ok: %lld checks\n", g_checks);
  return 0;
}
