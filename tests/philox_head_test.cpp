// csrc/philox_head.h against a literal Philox4x32-10: philox_tail(philox_head(..)) must be the block philox4x32_10 gives, bit
// for bit, on the counter words of the run layout (csrc/rng_layout.h) - random keys, steps, chains and temperatures, every
// block index of a step, steps beyond 2^32 (c0's high part), chain ids beyond 2^32 (c3's high part), streams 0 and 1.  The
// literal block below is the textbook round function (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3") and
// is itself pinned to the published known answers.  Also here: the cut csrc/schedule.h makes where the step index's high word
// changes - the heads a kernel parks at the start of a launch hold until then - and u01_open0's one-fma form against the
// two-operation form it replaces, on every input.  Plain C++, its own main: tests/test_philox_head_host.py compiles it with
// g++ -fsanitize=address,undefined and runs it.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "../rwm-pt-pytorch_amd/csrc/philox_head.h"
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

// Philox4x32-10, literally: ten rounds of (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)),
// the key bumped by the Weyl constants after each
static void philox_literal(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  uint32_t c[4] = {ctr[0], ctr[1], ctr[2], ctr[3]}, k[2] = {key[0], key[1]};
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
    const uint32_t n[4] = {(uint32_t)(p1 / 4294967296ull) ^ c[1] ^ k[0], (uint32_t)(p1 % 4294967296ull),
                           (uint32_t)(p0 / 4294967296ull) ^ c[3] ^ k[1], (uint32_t)(p0 % 4294967296ull)};
    std::memcpy(c, n, sizeof c);
    k[0] += 0x9E3779B9u;
    k[1] += 0xBB67AE85u;
  }
  std::memcpy(out, c, sizeof c);
}

// splitmix64: the test's own stream of tuples
static uint64_t g_state = 0x0123456789abcdefull;
static uint64_t next64() {
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// one block of the run layout both ways
static void check_block(uint64_t seed, unsigned long long step, unsigned long long gchain, uint32_t t, uint32_t stream, uint32_t blk) {
  const PhiloxKey key = philox_key(seed);
  const uint32_t c0 = step_word_c0hi(step) | blk, c1 = step_word_c1(step), c2 = chain_word_c2(gchain),
                 c3 = with_stream(chain_word_c3(gchain, t), stream);
  const uint32_t ctr[4] = {c0, c1, c2, c3}, k[2] = {key.k0, key.k1};
  uint32_t want[4];
  philox_literal(ctr, k, want);
  // as the step kernel does: the chain word's product once per thread, the head per (thread, block), X once per step
  uint32_t chain_hi, chain_lo, x_hi, x_lo;
  philox_mul(kPhiloxM1, c2, chain_hi, chain_lo);
  const PhiloxHead head = philox_head(c0, chain_lo, c3, key.k0, key.k1);
  philox_step_product(chain_hi, c1, key.k0, x_hi, x_lo);
  const u32x4 got = philox_tail(head, c0, x_hi, x_lo, key.k0, key.k1);
  CHECK(got.x == want[0] && got.y == want[1] && got.z == want[2] && got.w == want[3],
        "seed %llx step %llu chain %llu t %u stream %u block %u: %08x %08x %08x %08x, literal %08x %08x %08x %08x", (unsigned long long)seed,
        step, gchain, t, stream, blk, got.x, got.y, got.z, got.w, want[0], want[1], want[2], want[3]);
}

// the two-operation form u01_open0 had: top 24 bits + 1, scaled
static float u01_open0_two_ops(uint32_t r) {
  volatile float k1 = (float)(r >> 8) + 1.0f;  // (volatile: rounded to float here, never contracted with the product)
  return k1 * 0x1p-24f;
}

int main() {
  // the literal block against the published known answers (Random123 kat_vectors, philox4x32 10 rounds)
  {
    const uint32_t z[4] = {0, 0, 0, 0}, zk[2] = {0, 0}, f[4] = {~0u, ~0u, ~0u, ~0u}, fk[2] = {~0u, ~0u};
    const uint32_t pi[4] = {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}, pik[2] = {0xa4093822u, 0x299f31d0u};
    uint32_t o[4];
    philox_literal(z, zk, o);
    CHECK(o[0] == 0x6627e8d5u && o[1] == 0xe169c58du && o[2] == 0xbc57ac4cu && o[3] == 0x9b00dbd8u, "known answer, zeros");
    philox_literal(f, fk, o);
    CHECK(o[0] == 0x408f276du && o[1] == 0x41c83b0eu && o[2] == 0xa20bc7c6u && o[3] == 0x6d5451fdu, "known answer, ones");
    philox_literal(pi, pik, o);
    CHECK(o[0] == 0xd16cfe09u && o[1] == 0x94fdccebu && o[2] == 0x5001e420u && o[3] == 0x24126ea1u, "known answer, pi");
  }

  // 10^6 random tuples: any key, steps and chain ids of up to 48 bits, any temperature, any block of a step, both streams
  for (int i = 0; i < 1000000; ++i) {
    const uint64_t seed = next64(), a = next64(), b = next64(), c = next64();
    check_block(seed, a >> 16, b >> 16, (uint32_t)(c & 0xffu), (uint32_t)((c >> 8) & 1u), (uint32_t)((c >> 16) % 27u));
  }
  // the corners, crossed: every block index 0..26, steps on both sides of 2^32 (c0hi = 0 and != 0), chain ids on both sides of
  // 2^32, the first and last temperatures, streams 0 and 1
  const unsigned long long k2p32 = 4294967296ull;
  const unsigned long long steps[] = {0ull, 1ull, k2p32 - 1, k2p32, k2p32 + 1, 5 * k2p32 + 12345, (1ull << 48) - 1};
  const unsigned long long chains[] = {0ull, 65535ull, k2p32 - 1, k2p32, k2p32 + 5, (1ull << 44) - 1};
  const uint32_t temps[] = {0u, 1u, 31u, 64u, 255u};
  const uint64_t seeds[] = {0ull, 2024ull, 0xC0FFEE1234ull, ~0ull};
  for (uint64_t seed : seeds)
    for (unsigned long long s : steps)
      for (unsigned long long g : chains)
        for (uint32_t t : temps)
          for (uint32_t stream = 0; stream < 2; ++stream)
            for (uint32_t blk = 0; blk <= 26; ++blk) check_block(seed, s, g, t, stream, blk);
  const long long block_checks = g_checks;

  // u01_open0 on all 2^24 values of r >> 8 (the low byte is dropped: one r per value, and the two ends with the low byte set)
  for (uint32_t k = 0; k < (1u << 24); ++k) {
    const uint32_t r = k << 8;
    const float want = u01_open0_two_ops(r), got = u01_open0(r);
    CHECK(std::memcmp(&want, &got, 4) == 0, "u01_open0(%08x): %a, two operations give %a", r, got, want);
  }
  CHECK(u01_open0(0xffu) == u01_open0(0u) && u01_open0(~0u) == 1.0f && u01_open0(0u) == 0x1p-24f, "u01_open0: ends, low byte");

  // the cut at the step index's high word: launches tile the request, none holds steps with different high words, each is as
  // long as the request, the cap and the boundary allow, and the countdown to the first swap step is the literal one
  long long launches = 0;
  for (long long wrap = 1; wrap <= 2; ++wrap)
    for (long long before = 0; before <= 9; ++before)
      for (long long n_steps = 1; n_steps <= 20; ++n_steps)
        for (long long cap : {1ll, 3ll, 7ll, 65536ll})
          for (long long se : {1ll, 3ll, 10ll}) {
            const long long step0 = wrap * (long long)k2p32 - before;
            const StepRequest req = {step0, n_steps, step0 + 2, se, 0, 1, 0, 1};
            long long done = 0;
            while (done < n_steps) {
              const LaunchCut c = launch_at(req, done, cap);
              const long long s0 = step0 + done, left = n_steps - done;
              const long long to_wrap = (s0 / (long long)k2p32 + 1) * (long long)k2p32 - s0;
              const long long want_n = left < cap ? (left < to_wrap ? left : to_wrap) : (cap < to_wrap ? cap : to_wrap);
              CHECK(c.step0 == s0 && c.n == want_n && c.n >= 1, "step0 %lld n_steps %lld cap %lld done %lld: launch of %d steps from %lld", step0,
                    n_steps, cap, done, c.n, c.step0);
              CHECK(step_word_c0hi((unsigned long long)s0) == step_word_c0hi((unsigned long long)(s0 + c.n - 1)),
                    "step0 %lld n_steps %lld cap %lld done %lld: the launch holds two high words", step0, n_steps, cap, done);
              long long first = 0;  // steps to the first multiple of se (1 = the launch's first step)
              for (long long i = 1; i <= c.n && first == 0; ++i)
                if ((s0 + i) % se == 0) first = i;
              CHECK(first > 0 ? c.steps_to_swap == first : c.steps_to_swap > c.n, "step0 %lld done %lld se %lld: countdown %d", step0, done, se,
                    c.steps_to_swap);
              long long burn = 0;
              for (long long sc = s0 + 1; sc <= s0 + c.n; ++sc) burn += sc <= req.burn_in ? 1 : 0;
              CHECK(c.burn_left == burn, "step0 %lld done %lld: burn_left %d", step0, done, c.burn_left);
              done += c.n;
              ++launches;
            }
            CHECK(done == n_steps, "request overrun");
          }
  CHECK(steps_to_step_word_wrap(0) == (long long)k2p32 && steps_to_step_word_wrap((long long)k2p32 - 1) == 1 &&
            steps_to_step_word_wrap((long long)k2p32) == (long long)k2p32, "steps_to_step_word_wrap");

  std::printf("philox head ok: %lld blocks, 16777216 u01_open0 inputs, %lld launches, %lld checks\n", block_checks, launches, g_checks);
  return 0;
}
