// csrc/flow.h - the flow word and what a swap event does to it - against a literal restatement: explicit arrays of ids and
// directions, the event's accepted pairs applied to them one by one as transpositions (exchange) or copies (reference_copy),
// and the three steps of the rule spelled out.  The header's side moves the words as the kernels do: through src[t], the
// position whose row lands at t, built from the accepted pairs the way kernel.h's swap_decide builds it (the carried index of
// the sequential exchange scan; the parallel forms of the other three).  A program of its own (compiled by
// tests/test_flow_host.py under AddressSanitizer and UBSan); prints "flow ok: <events> events, ..." or the first mismatch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../rwm-pt-pytorch_amd/csrc/flow.h"

namespace {

enum { kExchange = 0, kCopy = 1, kSequential = 0, kEvenOdd = 1 };

struct Rng {  // xorshift64*: the accept patterns
  uint64_t s;
  double next() {
    s ^= s >> 12, s ^= s << 25, s ^= s >> 27;
    return (double)((s * 2685821657736338717ull) >> 11) / 9007199254740992.0;
  }
};

// src[t] from the accepted pairs, as swap_decide leaves it
void sources(int T, int mode, int order, int par, const std::vector<char> &acc, std::vector<int> &src) {
  for (int t = 0; t < T; ++t) src[t] = t;
  if (order == kSequential && mode == kExchange) {
    int car = 0;  // the scan carries one state upward: it stays at pair j when the pair refuses
    for (int j = 0; j < T - 1; ++j) {
      src[j] = acc[j] ? j + 1 : car;
      car = acc[j] ? car : j + 1;
    }
    src[T - 1] = car;
  } else if (order == kSequential) {
    for (int j = 0; j < T - 1; ++j)
      if (acc[j]) src[j] = j + 1;
  } else {
    for (int j = par; j < T - 1; j += 2)
      if (acc[j]) {
        src[j] = j + 1;
        if (mode == kExchange) src[j + 1] = j;
      }
  }
}

struct Counters {
  std::vector<long long> trips, up, down;
  explicit Counters(int T) : trips(T, 0), up(T, 0), down(T, 0) {}
};

long long run_case(int T, int mode, int order, double p_accept, int events, uint64_t seed, long long &trips_total, long long &refused_total) {
  Rng rng{seed};
  // the header's side: flow words
  std::vector<int32_t> word(T), next(T);
  Counters h(T);
  // the literal side: ids and directions as arrays of their own (0 none, 1 up, 2 down)
  std::vector<int> id(T), dir(T, 0);
  Counters l(T);
  for (int t = 0; t < T; ++t) word[t] = ptrwm::flow_word(t, ptrwm::kFlowNone), id[t] = t;
  std::vector<char> acc(T, 0);
  std::vector<int> src(T);
  for (int e = 0; e < events; ++e) {
    const int par = e & 1;
    for (int j = 0; j < T - 1; ++j) {
      const bool attempted = order == kSequential || (j & 1) == par;
      acc[j] = attempted && rng.next() < p_accept;
      refused_total += attempted && !acc[j];
    }
    // ---- flow.h ----
    sources(T, mode, order, par, acc, src);
    for (int t = 0; t < T; ++t) {
      bool trip;
      next[t] = ptrwm::flow_ends(word[src[t]], t, T, trip);
      if (trip) h.trips[ptrwm::flow_id(next[t])] += 1;
      h.up[t] += ptrwm::flow_visit_up(next[t]);
      h.down[t] += ptrwm::flow_visit_down(next[t]);
    }
    word.swap(next);
    // ---- literal ----
    for (int j = 0; j < T - 1; ++j) {  // ascending; even/odd: the pairs are disjoint
      if (!acc[j]) continue;
      if (mode == kExchange) {
        std::swap(id[j], id[j + 1]);
        std::swap(dir[j], dir[j + 1]);
      } else {
        id[j] = id[j + 1];
        dir[j] = dir[j + 1];
      }
    }
    if (dir[0] == 2) l.trips[id[0]] += 1;
    dir[0] = 1;
    dir[T - 1] = 2;
    for (int t = 0; t < T; ++t) {
      if (dir[t] == 1) l.up[t] += 1;
      if (dir[t] == 2) l.down[t] += 1;
    }
    // ---- equal, after every event ----
    for (int t = 0; t < T; ++t) {
      if (ptrwm::flow_id(word[t]) != id[t] || ptrwm::flow_dir(word[t]) != dir[t] || word[t] != (int32_t)(id[t] | (dir[t] << 16)) ||
          h.trips[t] != l.trips[t] || h.up[t] != l.up[t] || h.down[t] != l.down[t]) {
        std::printf("MISMATCH T %d mode %d order %d event %d position %d: word %d|%d, literal %d|%d, trips %lld/%lld, up %lld/%lld, down %lld/%lld\n",
                    T, mode, order, e, t, ptrwm::flow_id(word[t]), ptrwm::flow_dir(word[t]), id[t], dir[t], h.trips[t], l.trips[t],
                    h.up[t], l.up[t], h.down[t], l.down[t]);
        std::exit(1);
      }
    }
    if (mode == kExchange) {  // a permutation of 0 .. T - 1
      std::vector<char> seen(T, 0);
      for (int t = 0; t < T; ++t) {
        if (seen[ptrwm::flow_id(word[t])]) {
          std::printf("MISMATCH T %d order %d event %d: id %d twice under exchange\n", T, order, e, ptrwm::flow_id(word[t]));
          std::exit(1);
        }
        seen[ptrwm::flow_id(word[t])] = 1;
      }
    }
  }
  // the invariants of the rule
  for (int t = 0; t < T; ++t)
    if (h.up[t] + h.down[t] > events || h.up[0] != events || h.down[T - 1] != events || h.up[T - 1] != 0 || h.down[0] != 0) {
      std::printf("MISMATCH T %d mode %d order %d: visit counts break an invariant at %d\n", T, mode, order, t);
      std::exit(1);
    }
  for (int t = 0; t < T; ++t) trips_total += h.trips[t];
  return events;
}

}  // namespace

int main() {
  const int temps[] = {2, 3, 5, 8, 64, 70, 256};
  const double probs[] = {0.2, 0.5, 0.9};
  long long events = 0, trips = 0, refused = 0;
  uint64_t seed = 0x9e3779b97f4a7c15ull;
  for (int T : temps)
    for (int mode = 0; mode < 2; ++mode)
      for (int order = 0; order < 2; ++order)
        for (double p : probs) {
          long long t = 0;
          // long ladders need many events for a round trip: more of them where they are cheap to check
          events += run_case(T, mode, order, p, T <= 8 ? 400 : 1200, seed += 0x632be59bd9b4e019ull, t, refused);
          if (T <= 8 && mode == kExchange && t == 0) {
            std::printf("MISMATCH T %d order %d p %.1f: no round trip in 400 events\n", T, order, p);
            return 1;
          }
          trips += t;
        }
  // pack / unpack over the whole id range, every direction
  for (int id = 0; id < 65536; id += 257)
    for (int d = 0; d < 3; ++d) {
      const int32_t w = ptrwm::flow_word(id, d);
      if (ptrwm::flow_id(w) != id || ptrwm::flow_dir(w) != d || w != (id | (d << 16))) {
        std::printf("MISMATCH word %d %d\n", id, d);
        return 1;
      }
    }
  if (trips <= 0 || refused <= 0) {
    std::printf("MISMATCH vacuous: %lld round trips, %lld refused pairs\n", trips, refused);
    return 1;
  }
  std::printf("flow ok: %lld events, 7 ladder lengths x 2 modes x 2 orders x 3 acceptance rates, every event equal\n", events);
  return 0;
}
