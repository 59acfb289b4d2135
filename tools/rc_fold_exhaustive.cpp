// Exhaustive host check of the folded rough-carpet dimension term (csrc/targets.h rc_fold_dim_term) against the two-term
// form it replaces (rc_dim_term<false, true>): for EVERY fp32 coordinate x (all 2^32 bit patterns) and a few axis scales,
// the per-dimension outputs must agree - the same mx bits and the same exponent argument (+-0 alike), or both arguments
// below -25 (then 1 + 2^arg rounds to 1 in either form), or both forms NaN-poisoned (a NaN log-density, rejected by the
// Metropolis test).  Parameter sets that csrc/capi.hip rough_carpet_fold would refuse are reported and skipped, unless
// --all is given (then they are expected to show mismatches: a check that the checker can see one).
//
//   g++ -O2 -std=c++17 -fopenmp -ffp-contract=off -o /tmp/rc_fold_exhaustive tools/rc_fold_exhaustive.cpp
//   /tmp/rc_fold_exhaustive [--all]
//
// The device's max / med3 are restated for non-NaN operands (IEEE maxNum, median of three); NaN operands are only ever
// compared as "poisoned".
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

static const float kRcScale = 0.84932180028801904f;
static const float kLog2e = 1.44269504088896340736f;

static float bits_f(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static uint32_t f_bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static float med3(float a, float b, float c) { return std::max(std::min(a, b), std::min(std::max(a, b), c)); }

struct Params { float m, ln_w[3]; };  // modes -m, 0, +m; natural-log weights in that order

// capi.hip rough_carpet_fold for modes (-m, 0, +m) (the two-term proof is taken from the far-mode margin, which implies it
// for these modes: the smallest term is the far outer one or below the margin's bound)
static bool eligible(const Params &p) {
  const double l2e = 1.4426950408889634, m = p.m;
  const double a_neg = l2e * (p.ln_w[0] - 0.5 * m * m), a_mid = l2e * p.ln_w[1], a_pos = l2e * (p.ln_w[2] - 0.5 * m * m);
  return std::max(a_mid, a_pos) - a_neg > 27.0 && std::max(a_mid, a_neg) - a_pos > 27.0;
}

static long long check(const Params &p, float scale) {
  const float sc = scale * kRcScale;
  const float m0 = -((-p.m) * kRcScale), m1 = -(0.0f * kRcScale), m2 = -(p.m * kRcScale);
  const float w0 = p.ln_w[0] * kLog2e, w1 = p.ln_w[1] * kLog2e, w2 = p.ln_w[2] * kLog2e;
  long long bad = 0;
#pragma omp parallel for reduction(+ : bad) schedule(static)
  for (long long i = 0; i < (1ll << 32); ++i) {
    const float y = bits_f((uint32_t)i);
    // two-term form
    const float d0 = std::fma(y, sc, m0), d1 = std::fma(y, sc, m1), d2 = std::fma(y, sc, m2);
    const float a0 = std::fma(-d0, d0, w0), a1 = std::fma(-d1, d1, w1), a2 = std::fma(-d2, d2, w2);
    const bool nan_old = std::isnan(a0) || std::isnan(a1) || std::isnan(a2);
    const float mx_old = std::max(std::max(a0, a1), a2);
    const float arg_old = med3(a0, a1, a2) - mx_old;
    // folded form
    const float f1 = y * sc;
    const float dn = std::fma(std::fabs(y), std::fabs(sc), m2);
    const uint32_t neg = (uint32_t)((int32_t)f_bits(f1) >> 31);
    const float wn = bits_f((neg & f_bits(w0)) | (~neg & f_bits(w2)));
    const float b1 = std::fma(-f1, f1, w1), bn = std::fma(-dn, dn, wn);
    const bool nan_new = std::isnan(b1) || std::isnan(bn);
    const float mx_new = std::max(b1, bn);
    const float arg_new = -std::fabs(b1 - bn);
    bool ok;
    if (nan_old || nan_new || std::isnan(arg_old) || std::isnan(arg_new))
      ok = (nan_old || std::isnan(arg_old)) == (nan_new || std::isnan(arg_new));
    else
      ok = f_bits(mx_old) == f_bits(mx_new) && (arg_old == arg_new || (arg_old < -25.0f && arg_new < -25.0f));
    if (!ok) {
      if (bad < 3)
#pragma omp critical
        std::printf("    mismatch x=%a: mx %a / %a, arg %a / %a\n", y, mx_old, mx_new, arg_old, arg_new);
      ++bad;
    }
  }
  return bad;
}

int main(int argc, char **argv) {
  const bool all = argc > 1 && std::strcmp(argv[1], "--all") == 0;
  const Params sets[] = {
      {15.0f, {std::log(0.5f), std::log(0.3f), std::log(0.2f)}},    // the benchmark target
      {15.0f, {std::log(1.f / 3), std::log(1.f / 3), std::log(1.f / 3)}},
      {15.0f, {std::log(0.98f), std::log(0.01f), std::log(0.01f)}},
      {15.0f, {std::log(0.01f), std::log(0.01f), std::log(0.98f)}},
      {6.2f, {std::log(1.f / 3), std::log(1.f / 3), std::log(1.f / 3)}},   // just above the margin
      {6.05f, {std::log(1.f / 3), std::log(1.f / 3), std::log(1.f / 3)}},  // just below it
      {4.0f, {std::log(0.5f), std::log(0.3f), std::log(0.2f)}},
  };
  const float scales[] = {1.0f, 0.5f, 1.7f, -1.3f};
  long long total = 0;
  for (const Params &p : sets) {
    const bool el = eligible(p);
    std::printf("m = %g, w = (%g, %g, %g): %s\n", p.m, std::exp(p.ln_w[0]), std::exp(p.ln_w[1]), std::exp(p.ln_w[2]),
                el ? "eligible" : "not eligible");
    if (!el && !all) continue;
    for (float s : scales) {
      const long long bad = check(p, s);
      std::printf("  scale %g: %lld mismatching coordinates\n", s, bad);
      if (el) total += bad;
    }
  }
  std::printf(total == 0 ? "OK: the folded form matches wherever it is eligible\n" : "FAIL: %lld mismatches\n", total);
  return total == 0 ? 0 : 1;
}
