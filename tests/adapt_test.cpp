// csrc/adapt.h on the CPU (plain C++, built under AddressSanitizer and UBSan by tests/test_adapt_host.py).
//   adapt_test            the launches / reduce / update sequence that schedule.h's warmup_launch_at - the function run_impl
//                         (capi.hip) cuts its requests by - gives for uncut runs and runs cut into two requests at every
//                         position, verified step by step against a brute-force loop over the windows, and a few fixed points of
//                         the update rule (the window helpers themselves: tests/schedule_test.cpp)
//   adapt_test update     reads lines "s_old_bits accepted counted gain_k target min_bits max_bits" (floats as their uint32 bit
//                         patterns, doubles as %.17g) and prints the bit pattern of adapt_update's result, one per line: the NumPy
//                         comparison of test_adapt_host.py
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../rwm-pt-pytorch_amd/csrc/adapt.h"
#include "warmup_test_util.h"

using namespace ptrwm;

static int g_fail = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      if (g_fail++ < 20) std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
    }                                                              \
  } while (0)

struct Event {
  int kind;  // 0: launch (a = first step, b = steps, c = adapting), 1: reduce (a = window), 2: update (a = window)
  long long a, b;
  bool c;
};

// one request as run_impl (capi.hip) cuts it: every launch, and what follows it, is what warmup_launch_at says (the scale's
// tuning alone; next to the ladder's: tests/ladder_test.cpp)
static void request(long long step0, long long n, long long W, long long until, long long cap, bool defer, std::vector<Event> &out) {
  long long m = 0;
  for (long long done = 0; done < n; done += m) {
    const long long s = step0 + done;
    const WarmupLaunch l = warmup_launch_at(s, n - done < cap ? n - done : cap, {W, until}, defer, {0, 0}, 1, false);
    m = l.n;
    out.push_back({0, s, m, l.warmup});
    if (l.scale_reduce) out.push_back({1, l.scale_window, 0, false});
    if (l.scale_update) out.push_back({2, l.scale_window, 0, false});
    CHECK(!l.ladder_probe && !l.ladder_update);  // (no ladder)
  }
}

// every step once, in order, with the right flag; no adapting launch beyond its window; reduce / update of window k right after
// the launch that performs step (k + 1) W - 1, in window order
static void check_events(const std::vector<Event> &ev, long long N, long long W, long long until, bool defer) {
  long long next = 0, next_window = 0;
  for (size_t i = 0; i < ev.size(); ++i) {
    const Event &e = ev[i];
    if (e.kind == 0) {
      CHECK(e.a == next && e.b >= 1);
      long long w0 = -1, w1 = -1;
      for (long long s = e.a; s < e.a + e.b; ++s) {
        long long w = -1;
        const bool ad = bf_step_adapts(s, W, until, &w);
        CHECK(ad == e.c);  // one flag for the whole launch: the warm-up overrides are per launch
        if (s == e.a) w0 = w;
        w1 = w;
      }
      if (e.c) CHECK(w0 == w1);  // never across a window end
      next = e.a + e.b;
      long long w = -1;
      const bool ends = bf_step_adapts(next - 1, W, until, &w) && next % W == 0;
      if (ends) {
        CHECK(i + 1 < ev.size() && ev[i + 1].kind == 1 && ev[i + 1].a == w && w == next_window);
        if (!defer) CHECK(i + 2 < ev.size() && ev[i + 2].kind == 2 && ev[i + 2].a == w);
        ++next_window;
      } else {
        CHECK(i + 1 == ev.size() || ev[i + 1].kind == 0);
      }
    } else if (e.kind == 2) {
      CHECK(!defer && i >= 1 && ev[i - 1].kind == 1 && ev[i - 1].a == e.a);
    }
  }
  CHECK(next == N);
  CHECK(next_window == window_count({W, until}));
}

static std::vector<Event> kernels_only(const std::vector<Event> &ev) {
  std::vector<Event> k;
  for (const Event &e : ev)
    if (e.kind != 0) k.push_back(e);
  return k;
}

static bool same(const std::vector<Event> &x, const std::vector<Event> &y) {
  if (x.size() != y.size()) return false;
  for (size_t i = 0; i < x.size(); ++i)
    if (x[i].kind != y[i].kind || x[i].a != y[i].a) return false;
  return true;
}

static int update_mode() {
  char line[512];
  while (std::fgets(line, sizeof line, stdin) != nullptr) {
    uint32_t sb, lo, hi;
    long long acc, cnt;
    double gk, target;
    if (std::sscanf(line, "%" SCNu32 " %lld %lld %lg %lg %" SCNu32 " %" SCNu32, &sb, &acc, &cnt, &gk, &target, &lo, &hi) != 7) return 2;
    std::printf("%" PRIu32 "\n", to_bits(adapt_update(from_bits(sb), acc, cnt, gk, target, from_bits(lo), from_bits(hi))));
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc > 1 && std::strcmp(argv[1], "update") == 0) return update_mode();
  long long n_checked = 0;
  const long long Ws[] = {1, 7, 50};
  for (long long W : Ws) {
    const long long burn_in = 4 * W + 7, N = burn_in + 5;
    const long long untils[] = {0, W - 1, W, 3 * W + 7, burn_in};
    for (long long until : untils) {
      // the launch sequence: uncut, and cut into two requests at every position, for several launch caps
      const long long caps[] = {1, 3, 1ll << 16};
      for (int defer = 0; defer < 2; ++defer)
        for (long long cap : caps) {
          std::vector<Event> whole;
          request(0, N, W, until, cap, defer != 0, whole);
          check_events(whole, N, W, until, defer != 0);
          for (long long p = 0; p <= N; ++p) {
            std::vector<Event> cut;
            request(0, p, W, until, cap, defer != 0, cut);
            request(p, N - p, W, until, cap, defer != 0, cut);
            check_events(cut, N, W, until, defer != 0);
            CHECK(same(kernels_only(cut), kernels_only(whole)));
            ++n_checked;
          }
          // ... and into many: one request per step
          std::vector<Event> steps;
          for (long long s = 0; s < N; ++s) request(s, 1, W, until, cap, defer != 0, steps);
          check_events(steps, N, W, until, defer != 0);
          CHECK(same(kernels_only(steps), kernels_only(whole)));
        }
    }
  }
  // the update rule: fixed points
  CHECK(adapt_update(2.0f, 0, 0, 3.0, 0.234, 1e-3f, 1e3f) == 2.0f);          // nothing counted: left alone, not even clamped
  CHECK(adapt_update(2000.0f, 0, 0, 3.0, 0.234, 1e-3f, 1e3f) == 2000.0f);
  CHECK(adapt_update(2.0f, 234, 1000, 3.0, 0.234, 1e-3f, 1e3f) == 2.0f);      // on target: exp(0) = 1
  CHECK(adapt_update(2.0f, 1000, 1000, 3.0, 0.234, 1e-3f, 1e3f) > 2.0f);      // accepts too often: larger steps
  CHECK(adapt_update(2.0f, 0, 1000, 3.0, 0.234, 1e-3f, 1e3f) < 2.0f);         // never accepts: smaller steps
  CHECK(adapt_update(2.0f, 1000, 1000, 3.0, 0.234, 1e-3f, 2.5f) == 2.5f);     // the clamps bind exactly
  CHECK(adapt_update(2.0f, 0, 1000, 3.0, 0.234, 1.75f, 1e3f) == 1.75f);
  if (g_fail != 0) {
    std::printf("adapt FAILED: %d check(s)\n", g_fail);
    return 1;
  }
  std::printf("adapt ok: %lld positions\n", n_checked);
  return 0;
}
