// csrc/ladder.h on the CPU (plain C++, built under AddressSanitizer and UBSan by tests/test_ladder_host.py).
//   ladder_test           the launches / probe / update sequence that schedule.h's warmup_launch_at - the function run_impl
//                         (capi.hip) cuts its requests by - gives for uncut runs, runs cut into two requests at every position
//                         and runs cut into single steps, alone and next to the scale's adaptation (W = 7 beside V = 6),
//                         verified against a brute-force loop over the windows; a few fixed points of the update rule (the
//                         window helpers themselves: tests/schedule_test.cpp)
//   ladder_test update    reads lines "T gain_j beta_bits[T] pooled[T] scale_bits[T]" (floats as their uint32 bit patterns,
//                         gain_j as %.17g) and prints "outcome beta_new_bits[T] scale_new_bits[T]": the NumPy comparison of
//                         test_ladder_host.py
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../rwm-pt-pytorch_amd/csrc/ladder.h"
#include "warmup_test_util.h"

using namespace ptrwm;

static int g_fail = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      if (g_fail++ < 20) std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
    }                                                              \
  } while (0)

enum { kLaunch, kScaleReduce, kScaleUpdate, kProbe, kLadderUpdate };
struct Event {
  int kind;        // kLaunch: a = first step, b = steps.  kProbe: a = the probe step.  the others: a = window
  long long a, b;
};

struct Setup {
  long long V, P, until;    // the ladder
  long long W, adapt_until; // the scale (W = 0: off)
  long long cap;
  bool defer;
};

// one request as run_impl (capi.hip) cuts it: every launch, and what follows it in run_impl's order, is what warmup_launch_at
// says
static void request(long long step0, long long n, const Setup &u, std::vector<Event> &out) {
  long long m = 0;
  for (long long done = 0; done < n; done += m) {
    const long long s = step0 + done;
    const WarmupLaunch l = warmup_launch_at(s, n - done < u.cap ? n - done : u.cap, {u.W, u.adapt_until}, u.defer, {u.V, u.until}, u.P, u.defer);
    m = l.n;
    out.push_back({kLaunch, s, m});
    if (l.scale_reduce) out.push_back({kScaleReduce, l.scale_window, 0});
    if (l.scale_update) out.push_back({kScaleUpdate, l.scale_window, 0});
    if (l.ladder_probe) out.push_back({kProbe, s + m - 1, 0});
    if (l.ladder_update) out.push_back({kLadderUpdate, l.ladder_window, 0});
  }
}

// every step once and in order; no launch of an adapting ladder window across a probe step; behind the launch that performs a
// probe step the probe and, at a window's end, the update - after the scale's kernels where both end there
static void check_events(const std::vector<Event> &ev, long long N, const Setup &u) {
  long long next = 0, probes = 0, updates = 0;
  for (size_t i = 0; i < ev.size(); ++i) {
    if (ev[i].kind != kLaunch) continue;
    const Event &e = ev[i];
    CHECK(e.a == next && e.b >= 1);
    next = e.a + e.b;
    for (long long s = e.a; s + 1 < next; ++s) {  // no probe step but the last one of a launch
      long long w;
      CHECK(!(bf_step_adapts(s, u.V, u.until, &w) && (s + 1) % u.P == 0));
    }
    // what must follow, in order
    std::vector<Event> want;
    long long w = -1;
    if (u.W > 0 && bf_step_adapts(next - 1, u.W, u.adapt_until, &w) && next % u.W == 0) {
      want.push_back({kScaleReduce, w, 0});
      if (!u.defer) want.push_back({kScaleUpdate, w, 0});
    }
    if (bf_step_adapts(next - 1, u.V, u.until, &w) && next % u.P == 0) {
      want.push_back({kProbe, next - 1, 0});
      ++probes;
      if (next % u.V == 0) {
        ++updates;
        if (!u.defer) want.push_back({kLadderUpdate, w, 0});
      }
    }
    for (size_t k = 0; k < want.size(); ++k)
      CHECK(i + 1 + k < ev.size() && ev[i + 1 + k].kind == want[k].kind && ev[i + 1 + k].a == want[k].a);
    CHECK(i + 1 + want.size() == ev.size() || ev[i + 1 + want.size()].kind == kLaunch);
  }
  CHECK(next == N);
  const long long K = window_count({u.V, u.until});
  CHECK(updates == K && probes == K * (u.V / u.P));
}

static std::vector<Event> kernels_only(const std::vector<Event> &ev) {
  std::vector<Event> k;
  for (const Event &e : ev)
    if (e.kind != kLaunch) k.push_back(e);
  return k;
}

static bool same(const std::vector<Event> &x, const std::vector<Event> &y) {
  if (x.size() != y.size()) return false;
  for (size_t i = 0; i < x.size(); ++i)
    if (x[i].kind != y[i].kind || x[i].a != y[i].a) return false;
  return true;
}

static int update_mode() {
  int T;
  double gain_j;
  while (std::scanf("%d %lg", &T, &gain_j) == 2) {
    if (T < 3 || T > 256) return 2;
    std::vector<float> beta(T), beta_new(T), scale(T);
    std::vector<long long> pooled(T);
    std::vector<double> work(T);
    uint32_t b;
    for (int t = 0; t < T; ++t) {
      if (std::scanf("%" SCNu32, &b) != 1) return 2;
      beta[t] = from_bits(b);
    }
    for (int t = 0; t < T; ++t)
      if (std::scanf("%lld", &pooled[t]) != 1) return 2;
    for (int t = 0; t < T; ++t) {
      if (std::scanf("%" SCNu32, &b) != 1) return 2;
      scale[t] = from_bits(b);
    }
    const int outcome = ladder_update(beta.data(), pooled.data(), T, gain_j, beta_new.data(), work.data());
    std::printf("%d", outcome);
    for (int t = 0; t < T; ++t) std::printf(" %" PRIu32, to_bits(beta_new[t]));
    for (int t = 0; t < T; ++t)
      std::printf(" %" PRIu32, to_bits(t > 0 && t < T - 1 ? ladder_rescale(scale[t], beta[t], beta_new[t]) : scale[t]));
    std::printf("\n");
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc > 1 && std::strcmp(argv[1], "update") == 0) return update_mode();
  long long n_checked = 0;
  const long long Vs[] = {1, 6, 50};
  for (long long V : Vs) {
    const long long burn_in = 4 * V + 5, N = burn_in + 5;
    const long long untils[] = {0, V - 1, V, 3 * V + 5, burn_in};
    std::vector<long long> Ps = {1, V};
    if (V % 2 == 0) Ps.push_back(V / 2);
    for (long long P : Ps)
      for (long long until : untils) {
        // the launch sequence: uncut, cut in two at every position, cut into single steps - alone, and (V = 6) next to the
        // scale's adaptation with W = 7
        const long long caps[] = {1, 3, 1ll << 16};
        for (int with_scale = 0; with_scale < (V == 6 ? 2 : 1); ++with_scale)
          for (int defer = 0; defer < 2; ++defer)
            for (long long cap : caps) {
              const Setup u = {V, P, until, with_scale ? 7 : 0, burn_in, cap, defer != 0};
              std::vector<Event> whole;
              request(0, N, u, whole);
              check_events(whole, N, u);
              for (long long p = 0; p <= N; ++p) {
                std::vector<Event> cut;
                request(0, p, u, cut);
                request(p, N - p, u, cut);
                check_events(cut, N, u);
                CHECK(same(kernels_only(cut), kernels_only(whole)));
                ++n_checked;
              }
              std::vector<Event> steps;
              for (long long s = 0; s < N; ++s) request(s, 1, u, steps);
              check_events(steps, N, u);
              CHECK(same(kernels_only(steps), kernels_only(whole)));
            }
      }
  }
  // shared ends, spelled out: V = 6, W = 7, both end behind step 41 - scale reduce, scale update, ladder probe, ladder update
  {
    const Setup u = {6, 6, 48, 7, 49, 1ll << 16, false};
    std::vector<Event> ev;
    request(0, 60, u, ev);
    bool found = false;
    for (size_t i = 0; i + 4 < ev.size(); ++i)
      if (ev[i].kind == kLaunch && ev[i].a + ev[i].b == 42) {
        found = ev[i + 1].kind == kScaleReduce && ev[i + 1].a == 5 && ev[i + 2].kind == kScaleUpdate && ev[i + 2].a == 5 &&
                ev[i + 3].kind == kProbe && ev[i + 3].a == 41 && ev[i + 4].kind == kLadderUpdate && ev[i + 4].a == 6;
      }
    CHECK(found);
  }
  // the quantum
  CHECK(ladder_quantum(1.0f) == 16777216ll && ladder_quantum(0.0f) == 0 && ladder_quantum(0.5f) == 8388608ll);
  CHECK(ladder_quantum(std::nanf("")) == 0 && ladder_quantum(0x1p-25f) == 0 && ladder_quantum(0x1.8p-24f) == 2);  // ties to even
  // the update rule: fixed points
  {
    const float beta[4] = {1.0f, 0.5f, 0.25f, 0.125f};
    float out[4];
    double work[4];
    const long long none[4] = {5, 6, 7, 0};
    CHECK(ladder_update(beta, none, 4, 2.0, out, work) == kLadderNoProbes && std::memcmp(out, beta, sizeof beta) == 0);
    const long long equal[4] = {3 << 24, 3 << 24, 3 << 24, 10};  // equal rates: the geometric ladder stays within rounding
    CHECK(ladder_update(beta, equal, 4, 2.0, out, work) == kLadderUpdated);
    CHECK(out[0] == beta[0] && out[3] == beta[3]);
    for (int t = 1; t < 3; ++t) CHECK(std::fabs(out[t] / beta[t] - 1.0f) < 4e-7f);
    const long long first_hot[4] = {9 << 24, 1 << 24, 1 << 24, 10};  // pair 0 swaps most: it widens, beta_1 moves down
    CHECK(ladder_update(beta, first_hot, 4, 2.0, out, work) == kLadderUpdated && out[1] < beta[1] && out[0] == beta[0] && out[3] == beta[3]);
    CHECK(out[0] > out[1] && out[1] > out[2] && out[2] > out[3]);
    // gaps of one float ulp next to 1: whatever the update wants, the rounded ladder cannot stay strictly decreasing
    const float tight[4] = {1.0f, from_bits(0x3f7fffffu), from_bits(0x3f7ffffeu), from_bits(0x3f7ffffdu)};
    const long long skew[4] = {0, 10 << 24, 0, 10};  // the middle pair widens: beta_1 rounds back onto beta_0
    CHECK(ladder_update(tight, skew, 4, 2.0, out, work) == kLadderSkipped && std::memcmp(out, tight, sizeof tight) == 0);
    CHECK(ladder_rescale(3.0f, 0.5f, 0.5f) == 3.0f && ladder_rescale(3.0f, 0.5f, 0.125f) == 6.0f);
  }
  if (g_fail != 0) {
    std::printf("ladder FAILED: %d check(s)\n", g_fail);
    return 1;
  }
  std::printf("ladder ok: %lld positions\n", n_checked);
  return 0;
}
