// The running sums of the thread form that start from their first term instead of from zero (csrc/philox.h chain_add:
// philox_normal_step's jump[] and RoughCarpetT::logp_fold's sm[]) give the bits the sums from zero give, after the closing
// arithmetic of each user.  A program of its own, plain C++ (tests/test_sum_first_term_host.py builds and runs it under
// AddressSanitizer and UBSan).
//
// The claim (philox.h): 0 + x differs from x only for x = -0, so a range's sum differs only if every term is -0, and then
// only in the sign of a zero; the four-range tree keeps "equal, or zeros of different sign"; and neither user can see the
// sign of a zero: the squared jump is converted to double and added to a sum that starts at +0.0, the rough carpet's sum
// feeds fmaf(sum + lg, kLn2, p7) with p7 != 0.
//
// Checked here, for ranges of 1 to 8 terms drawn from {+-0, the smallest denormals, ordinary values of both signs, a value
// whose double overflows, +inf}:
//   1. every range: the chain from the first term and the chain from zero are equal bit for bit, or both are zeros; they
//      differ exactly when every term is -0;
//   2. the four-range tree over every combination of partial sums and of the zeros' signs: equal, or both zeros;
//   3. whole sums (one range of up to 6 terms beside three ranges of fixed patterns, every range spelt the same way), after
//      the closing arithmetic of each user: the same bits.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

static uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}
static uint64_t bits(double f) {
  uint64_t u;
  std::memcpy(&u, &f, 8);
  return u;
}
// (volatile: each operation is one IEEE single operation, as add_rn on the device - nothing contracted or reassociated)
static float add_rn(float a, float b) {
  volatile float r = a + b;
  return r;
}
static bool same(float a, float b) { return bits(a) == bits(b) || (std::isnan(a) && std::isnan(b)); }
static bool same(double a, double b) { return bits(a) == bits(b) || (std::isnan(a) && std::isnan(b)); }
static bool same_or_zeros(float a, float b) { return same(a, b) || (a == 0.0f && b == 0.0f); }

static const float kLn2 = 0.6931471805599453f;
static const float kInf = std::numeric_limits<float>::infinity();
static const float kTerms[] = {0.0f, -0.0f, 1e-45f, -1e-45f, 1.5f, -2.75f, 3.0e38f, kInf};
constexpr int kNumTerms = (int)(sizeof(kTerms) / sizeof(kTerms[0]));

static float chain(const float *t, int n, bool from_first) {
  float s = from_first ? t[0] : add_rn(0.0f, t[0]);
  for (int i = 1; i < n; ++i) s = add_rn(s, t[i]);
  return s;
}
static float tree4(const float *p) { return add_rn(add_rn(p[0], p[1]), add_rn(p[2], p[3])); }

// the squared jump's way out: a float, converted, added to a double sum (ds_add_f64 on the device) that started at +0.0 and
// has taken `before` such terms
static double close_jump(float j2, double before) { return before + (double)j2; }
// the rough carpet's: fmaf(sum + lg, kLn2, p7)
static float close_carpet(float sum, float lg, float p7) { return std::fmaf(add_rn(sum, lg), kLn2, p7); }

static long long failures = 0;
static void fail(const char *what, int n, const float *t) {
  if (++failures > 10) return;
  std::printf("FAIL %s:", what);
  for (int i = 0; i < n; ++i) std::printf(" %a", (double)t[i]);
  std::printf("\n");
}

int main() {
  long long ranges = 0, differing = 0, trees = 0, wholes = 0;
  float t[8];
  // 1. every range of 1 .. 8 terms
  for (int n = 1; n <= 8; ++n) {
    long long count = 1;
    for (int i = 0; i < n; ++i) count *= kNumTerms;
    for (long long c = 0; c < count; ++c) {
      long long r = c;
      bool all_negative_zero = true;
      for (int i = 0; i < n; ++i, r /= kNumTerms) {
        t[i] = kTerms[r % kNumTerms];
        all_negative_zero = all_negative_zero && bits(t[i]) == 0x80000000u;
      }
      const float a = chain(t, n, true), b = chain(t, n, false);
      ++ranges;
      if (!same_or_zeros(a, b)) fail("range", n, t);
      if (same(a, b) == all_negative_zero) fail("range differs exactly when every term is -0", n, t);
      differing += same(a, b) ? 0 : 1;
    }
  }
  // 2. the tree: partial sums from the same set (any of them can be a range's sum), zeros of either sign on either side
  for (int c = 0; c < kNumTerms * kNumTerms * kNumTerms * kNumTerms; ++c) {
    float p[4], q[4];
    int r = c, zeros = 0, where[4];
    for (int i = 0; i < 4; ++i, r /= kNumTerms) {
      p[i] = kTerms[r % kNumTerms];
      if (p[i] == 0.0f) where[zeros++] = i;
    }
    for (int flip = 0; flip < (1 << zeros); ++flip) {
      for (int i = 0; i < 4; ++i) q[i] = p[i];
      for (int z = 0; z < zeros; ++z)
        if (flip & (1 << z)) q[where[z]] = -q[where[z]];
      ++trees;
      if (!same_or_zeros(tree4(p), tree4(q))) fail("tree", 4, p);
    }
  }
  // 3. whole sums through each user's closing arithmetic
  const std::vector<std::vector<float>> others[] = {
      {{-0.0f, -0.0f, -0.0f}, {-0.0f}, {-0.0f, -0.0f}},  // with a varied range of -0s: every term of the sum is -0
      {{0.0f, -0.0f}, {-0.0f, 0.0f}, {-0.0f}},
      {{1.5f, -2.75f}, {-0.0f, -0.0f}, {1e-45f, -1e-45f}},
      {{-0.0f}, {3.0e38f, 3.0e38f}, {-0.0f, 1e-45f}},
  };
  const double befores[] = {0.0, 0x1p-1074, 12.25, 1e300};  // (the sum is never -0: it starts at +0.0 and +0 + -0 = +0)
  const float lgs[] = {0.0f, -0.0f, 1e-45f, 47.5f, -3.25f};  // log2 of products of factors in [1, 3]: >= 0; more is checked
  const float p7s[] = {-27.568156f /* -30 ln sqrt(2 pi) */, -0.9189385f, 1e-45f, -1e-45f, 5.0f};
  for (int n = 1; n <= 6; ++n) {
    long long count = 1;
    for (int i = 0; i < n; ++i) count *= kNumTerms;
    for (long long c = 0; c < count; ++c) {
      long long r = c;
      for (int i = 0; i < n; ++i, r /= kNumTerms) t[i] = kTerms[r % kNumTerms];
      for (const auto &o : others) {
        float pa[4], pb[4];
        pa[0] = chain(t, n, true), pb[0] = chain(t, n, false);
        for (int k = 0; k < 3; ++k) pa[k + 1] = chain(o[k].data(), (int)o[k].size(), true), pb[k + 1] = chain(o[k].data(), (int)o[k].size(), false);
        for (int rot = 0; rot < 4; ++rot) {  // the varied range in each of the four places
          float ra[4], rb[4];
          for (int k = 0; k < 4; ++k) ra[k] = pa[(k + rot) & 3], rb[k] = pb[(k + rot) & 3];
          const float sa = tree4(ra), sb = tree4(rb);
          ++wholes;
          for (double before : befores)
            if (!same(close_jump(sa, before), close_jump(sb, before))) fail("jump", n, t);
          for (float lg : lgs)
            for (float p7 : p7s)
              if (!same(close_carpet(sa, lg, p7), close_carpet(sb, lg, p7))) fail("carpet", n, t);
        }
      }
    }
  }
  if (failures) {
    std::printf("%lld failures\n", failures);
    return 1;
  }
  std::printf("sums from the first term ok: %lld ranges (%lld differ in a zero's sign), %lld trees, %lld whole sums\n", ranges, differing, trees, wholes);
  return 0;
}
