// csrc/swap_walk.h - the sequential exchange sweep decided with lane masks and a walk over 64-bit words - against a literal
// restatement of the sweep: the scan of kernel.h's swap_decide (a carried log-density and index, three selects and one
// landed[] entry per pair, every position picking up landed[t] behind the loop), written out here per ladder.  The header's
// side works as the step kernel does: one wavefront of 64 lanes holding whole ladders of T lanes, per pair one answer per
// lane ("would my own state pass pair j of my ladder, were it the carrier") gathered into a mask - with random bits in the
// lanes that hold no live ladder - swap_walk_step over the masks, swap_walk_source per position.  Both rules of a pair: the
// threshold form (c < thr_j) and the literal one (u_j < min(1, exp(..)) of the four-product sum), chosen per ladder and mixed
// within a wavefront.  A program of its own (compiled by tests/test_swap_walk_host.py under AddressSanitizer and UBSan);
// prints "swap walk ok: ..." or the first mismatch.
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <thread>
#include <vector>

#include "../rwm-pt-pytorch_amd/csrc/swap_walk.h"

namespace {

struct Rng {  // xorshift64*
  uint64_t s;
  uint64_t bits() {
    s ^= s >> 12, s ^= s << 25, s ^= s >> 27;
    return s * 2685821657736338717ull;
  }
  double next() { return (double)(bits() >> 11) / 9007199254740992.0; }
};

const float kInf = std::numeric_limits<float>::infinity();
const float kNaN = std::numeric_limits<float>::quiet_NaN();

// the literal rule of a pair (kernel.h swap_log_prob / swap_accept_test): four products summed left to right, the clamp a
// select of the threshold (compiled with -ffp-contract=off; both sides call this one function anyway)
float swap_log_prob(float bj, float bk, float lj, float lk) { return ((bj * lk + bk * lj) - bj * lj) - bk * lk; }
bool swap_accept_test(float u, float log_prob) {
  const float threshold = (log_prob >= 0.0f) ? 1.0f : std::exp(log_prob);
  return u < threshold;
}

struct Ladder {
  bool literal;
  float l[64];     // log-densities the ladder enters the event with
  float v[64];     // per pair: its threshold (threshold form) or its uniform (literal)
  float beta[64];  // literal only
  // exhaustive part only: the T answers of pair j as bits, looked up by the digit of the pair's threshold (pass_table) -
  // the same answers passes() gives, taken once per (log-densities, threshold value) instead of once per case
  const uint8_t *answers = nullptr;
  uint8_t digit[64];
};

// would a carried state of log-density c be accepted at pair j?
inline bool passes(const Ladder &a, int j, float c) {
  return a.literal ? swap_accept_test(a.v[j], swap_log_prob(a.beta[j], a.beta[j + 1], c, a.l[j + 1])) : c < a.v[j];
}

struct Tally {
  long long ladders = 0, accepted = 0, refused = 0, literal_accepted = 0, literal_refused = 0, partial_waves = 0;
  void add(const Tally &o) {
    ladders += o.ladders, accepted += o.accepted, refused += o.refused, literal_accepted += o.literal_accepted,
        literal_refused += o.literal_refused, partial_waves += o.partial_waves;
  }
};

bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// One wavefront: ladders lad[0 .. nl), ladder c in lanes c T .. c T + T - 1; every other lane is idle.  Returns false
// (after printing) on the first position whose outcome differs from the literal scan's.
bool check_wave(int T, const Ladder *lad, int nl, Rng &garbage, Tally &tally) {
  uint64_t seg0 = 0, live = 0;
  for (int c = 0; c < nl; ++c) {
    seg0 |= 1ull << (c * T);
    live |= (T == 64 ? ~0ull : ((1ull << T) - 1ull)) << (c * T);
  }
  // ---- swap_walk.h ----
  ptrwm::SwapWalk w = ptrwm::swap_walk_begin(seg0);
  for (int j = 0; j < T - 1; ++j) {
    uint64_t pass = garbage.bits() & ~live;
    for (int c = 0; c < nl; ++c) {
      if (lad[c].answers != nullptr) {
        pass |= (uint64_t)lad[c].answers[lad[c].digit[j]] << (c * T);
        continue;
      }
      for (int k = 0; k < T; ++k)
        if (passes(lad[c], j, lad[c].l[k])) pass |= 1ull << (c * T + k);
    }
    ptrwm::swap_walk_step(w, seg0, j, pass);
  }
  // ---- the literal scan, per ladder ----
  for (int c = 0; c < nl; ++c) {
    const Ladder &a = lad[c];
    int landed[64];
    float car_l = a.l[0];
    int car_i = 0;
    for (int j = 0; j < T - 1; ++j) {
      const int ik = j + 1;
      const float lk = a.l[ik];
      const bool ok = passes(a, j, car_l);
      landed[j] = ok ? ik : car_i;
      car_l = ok ? car_l : lk;
      car_i = ok ? car_i : ik;
      (a.literal ? (ok ? tally.literal_accepted : tally.literal_refused) : (ok ? tally.accepted : tally.refused)) += 1;
    }
    landed[T - 1] = car_i;
    for (int t = 0; t < T; ++t) {
      const int src = landed[t];
      const float my_l = a.l[src];
      const bool pair_acc = (t < T - 1) && (src == t + 1);
      bool got_acc = false;
      const int got = ptrwm::swap_walk_source(w.rejected, seg0, c * T + t, t < T - 1, got_acc);
      if (got < c * T || got >= c * T + T || got - c * T != src || got_acc != pair_acc || !same_bits(a.l[got - c * T], my_l)) {
        std::printf("MISMATCH T %d, %d ladders, ladder %d (%s) position %d: walk src %d acc %d, scan src %d acc %d\n", T, nl, c,
                    a.literal ? "literal" : "threshold", t, got - c * T, (int)got_acc, src, (int)pair_acc);
        return false;
      }
    }
  }
  tally.ladders += nl;
  tally.partial_waves += (nl < 64 / T);
  return true;
}

const float kSeven[7] = {-kInf, -1.5f, 0.0f, 0.25f, 2.0f, kInf, kNaN};

long long ipow7(int e) {
  long long p = 1;
  while (e-- > 0) p *= 7;
  return p;
}

// for every assignment of T log-densities (its index in base 7) and every threshold value: bit k = l[k] < threshold
std::vector<uint8_t> pass_table(int T) {
  std::vector<uint8_t> tab((size_t)ipow7(T) * 7);
  Ladder a;
  a.literal = false;
  for (long long li = 0; li < ipow7(T); ++li) {
    long long n = li;
    for (int k = 0; k < T; ++k, n /= 7) a.l[k] = kSeven[n % 7];
    for (int d = 0; d < 7; ++d) {
      a.v[0] = kSeven[d];
      uint8_t bits = 0;
      for (int k = 0; k < T; ++k) bits |= (uint8_t)(passes(a, 0, a.l[k]) << k);
      tab[(size_t)li * 7 + d] = bits;
    }
  }
  return tab;
}

// Exhaustive, threshold form: case index n in [lo, hi) in base 7 = the T log-densities and T - 1 thresholds of a ladder,
// consecutive cases side by side in a wavefront (the last one of a range holds fewer: idle lanes with random mask bits)
bool exhaustive_range(int T, long long lo, long long hi, const std::vector<uint8_t> &tab, Tally &tally) {
  const int per_wave = 64 / T;
  Rng garbage{0x2545f4914f6cdd1dull ^ (uint64_t)lo ^ ((uint64_t)T << 56)};
  std::vector<Ladder> lad(per_wave);
  for (long long n0 = lo; n0 < hi; n0 += per_wave) {
    const int nl = (int)((hi - n0 < per_wave) ? hi - n0 : per_wave);
    for (int c = 0; c < nl; ++c) {
      long long n = n0 + c;
      Ladder &a = lad[c];
      a.literal = false;
      a.answers = tab.data() + (size_t)(n % ipow7(T)) * 7;
      for (int k = 0; k < T; ++k, n /= 7) a.l[k] = kSeven[n % 7];
      for (int j = 0; j < T - 1; ++j, n /= 7) a.v[j] = kSeven[a.digit[j] = (uint8_t)(n % 7)];
    }
    if (!check_wave(T, lad.data(), nl, garbage, tally)) return false;
  }
  return true;
}

bool exhaustive(int T, Tally &tally) {
  const long long total = ipow7(2 * T - 1);
  const int n_threads = total < 1000000 ? 1 : 16;
  const std::vector<uint8_t> tab = pass_table(T);
  std::vector<Tally> part(n_threads);
  std::atomic<bool> ok{true};
  std::vector<std::thread> pool;
  for (int i = 0; i < n_threads; ++i)
    pool.emplace_back([&, i] {
      if (!exhaustive_range(T, total * i / n_threads, total * (i + 1) / n_threads, tab, part[i])) ok = false;
    });
  for (auto &t : pool) t.join();
  for (const Tally &p : part) tally.add(p);
  return ok;
}

float random_logp(Rng &r) {
  const double p = r.next();
  if (p < 0.03) return -kInf;
  if (p < 0.05) return kInf;
  if (p < 0.08) return kNaN;
  return (float)(-40.0 * r.next() * r.next());
}

void random_ladder(int T, Rng &r, Ladder &a) {
  a.literal = r.next() < 0.4;
  const bool tame = r.next() < 0.5;  // no special values: long runs of accepted and refused pairs
  for (int k = 0; k < T; ++k) a.l[k] = tame ? (float)(-40.0 * r.next()) : random_logp(r);
  if (a.literal) {
    const bool ordered = r.next() < 0.6;
    float b = 1.0f;
    for (int k = 0; k < T; ++k) {
      a.beta[k] = ordered ? b : (float)r.next();
      b *= (float)(0.7 + 0.3 * r.next());
    }
    for (int j = 0; j < T - 1; ++j) {
      const double p = r.next();
      a.v[j] = p < 0.03 ? 0.0f : (p < 0.06 ? 1.0f : (p < 0.08 ? 2.0f : (float)r.next()));
    }
  } else {
    for (int j = 0; j < T - 1; ++j) {
      const double p = r.next();
      a.v[j] = p < 0.04 ? kInf : (p < 0.08 ? -kInf : (p < 0.1 ? kNaN : (float)(-40.0 * r.next() + 10.0 * (r.next() - 0.5))));
    }
  }
}

}  // namespace

int main() {
  Tally ex, rnd;
  for (int T = 2; T <= 6; ++T)
    if (!exhaustive(T, ex)) return 1;
  if (ex.ladders != 343 + 16807 + 823543 + 40353607 + 1977326743ll) {
    std::printf("MISMATCH exhaustive part covered %lld ladders\n", ex.ladders);
    return 1;
  }
  const int temps[] = {7, 8, 16, 21, 31, 32, 63, 64};
  Rng r{0x9e3779b97f4a7c15ull}, garbage{0xd1b54a32d192ed03ull};
  std::vector<Ladder> lad(64);
  long long waves = 0;
  for (int T : temps)
    for (int nl = 1; nl <= 64 / T; ++nl)
      for (int rep = 0; rep < 600; ++rep, ++waves) {
        for (int c = 0; c < nl; ++c) random_ladder(T, r, lad[c]);
        if (!check_wave(T, lad.data(), nl, garbage, rnd)) return 1;
      }
  if (ex.accepted <= 0 || ex.refused <= 0 || rnd.accepted <= 0 || rnd.refused <= 0 || rnd.literal_accepted <= 0 ||
      rnd.literal_refused <= 0 || ex.partial_waves <= 0 || rnd.partial_waves <= 0) {
    std::printf("MISMATCH vacuous: pairs accepted / refused %lld / %lld exhaustive, %lld / %lld and literal %lld / %lld random\n",
                ex.accepted, ex.refused, rnd.accepted, rnd.refused, rnd.literal_accepted, rnd.literal_refused);
    return 1;
  }
  std::printf("swap walk ok: %lld ladders exhaustive (T = 2..6, seven values), %lld random wavefronts of %lld ladders over 8 ladder "
              "lengths x every ladder count, both rules mixed per ladder, every position equal\n",
              ex.ladders, waves, rnd.ladders);
  return 0;
}
