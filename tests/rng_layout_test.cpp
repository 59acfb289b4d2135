// csrc/rng_layout.h against literal restatements: every helper that builds a Philox key or counter word, the swap-attempt
// ordinal and the threads of an exchange group, over a grid that crosses every 32-bit boundary the layout has.  The
// restatements below use division, remainder and multiplication where the header shifts and masks.  Plain C++, its own
// main: tests/test_host_logic.py compiles it with g++ -fsanitize=address,undefined and runs it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../rwm-pt-pytorch_amd/csrc/rng_layout.h"

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

static const unsigned long long k2p32 = 4294967296ull;
static uint32_t low32(unsigned long long v) { return (uint32_t)(v % k2p32); }

// the layout, literally (include/ptrwm.h, "Random numbers"): c3 = temperature + 256 stream + 4096 (chain / 2^32)
static uint32_t c3_literal(unsigned long long gchain, unsigned t, unsigned stream) {
  return low32(t + 256ull * stream + 4096ull * (gchain / k2p32));
}

// the lane-split form's workgroup for a ladder of 4 T > 64 lanes (variants.h quad_block_threads): the number of whole
// ladders k, k * 4 T <= 256, with the largest used fraction of the whole waves they need - the smallest such k
static int lane_split_block_literal(int T) {
  const int need = 4 * T;
  int best_k = 1, best_b = (need + 63) / 64 * 64;
  for (int k = 2; k * need <= 256; ++k) {
    const int b = (k * need + 63) / 64 * 64;
    if ((long long)k * need * best_b > (long long)best_k * need * b) best_k = k, best_b = b;  // k need / b > best_k need / best_b
  }
  return best_b;
}

int main() {
  const unsigned long long steps[] = {0ull, 1ull, k2p32 - 1, k2p32, k2p32 + 1, (1ull << 48) - 1};
  const unsigned long long chains[] = {0ull, k2p32 - 1, k2p32, (1ull << 44) - 1};
  const unsigned temps[] = {0u, 1u, 255u};

  // key
  const uint64_t seeds[] = {0ull, 1ull, 2024ull, k2p32 - 1, k2p32, 0x123456789abcdef0ull, ~0ull};
  for (uint64_t seed : seeds) {
    const PhiloxKey k = philox_key(seed);
    CHECK(k.k0 == low32(seed) && k.k1 == (uint32_t)(seed / k2p32), "seed %llu: key (%u, %u)", (unsigned long long)seed, k.k0, k.k1);
  }

  // step words
  for (unsigned long long s : steps) {
    CHECK(step_word_c0hi(s) == low32(65536ull * (s / k2p32)), "step %llu: c0hi %u", s, step_word_c0hi(s));
    CHECK(step_word_c1(s) == low32(s), "step %llu: c1 %u", s, step_word_c1(s));
    for (unsigned block = 0; block < 40; ++block)  // (the proposals or the block index into c0: below bit 16, disjoint)
      CHECK((step_word_c0hi(s) | block) == step_word_c0hi(s) + block, "step %llu: block %u overlaps the high word", s, block);
  }

  // chain words, with every stream
  for (unsigned long long g : chains)
    for (unsigned t : temps) {
      CHECK(chain_word_c2(g) == low32(g), "chain %llu: c2 %u", g, chain_word_c2(g));
      CHECK(chain_word_c3(g, t) == c3_literal(g, t, 0u), "chain %llu, t %u: c3 base %u", g, t, chain_word_c3(g, t));
      for (unsigned stream = 0; stream <= 3; ++stream) {
        const uint32_t c3 = with_stream(chain_word_c3(g, t), stream);
        CHECK(c3 == c3_literal(g, t, stream), "chain %llu, t %u, stream %u: c3 %u", g, t, stream, c3);
        CHECK(temperature_of(c3) == (int)t, "chain %llu, t %u, stream %u: temperature read back as %d", g, t, stream, temperature_of(c3));
      }
    }
  CHECK(kStreamMH == 0u && kStreamSwap == 1u && kStreamInit == 3u, "stream numbers");

  // stream 3: starting points
  const int attempts[] = {0, 1, 65535};
  for (int attempt : attempts)
    for (int d = 0; d <= 103; ++d) {
      CHECK(init_word_c0(d, attempt) == low32((unsigned long long)(d / 4) + 65536ull * (unsigned long long)attempt), "d %d, attempt %d: c0 %u", d,
            attempt, init_word_c0(d, attempt));
      CHECK(init_word_of(d) == d - 4 * (d / 4), "d %d: word %d", d, init_word_of(d));
    }
  for (unsigned long long g : chains)
    for (unsigned t : temps)
      for (int per_temperature = 0; per_temperature <= 1; ++per_temperature)
        CHECK(init_word_c3(g, t, per_temperature != 0) == c3_literal(g, per_temperature ? t : 0u, 3u), "chain %llu, t %u, per_temperature %d: c3 %u", g, t,
              per_temperature, init_word_c3(g, t, per_temperature != 0));

  // the ordinal of a swap attempt, against counting the attempts (sequential: every pair of every event; even/odd: events)
  const int ladder[] = {2, 3, 17, 256};
  for (int T : ladder) {
    long long attempts_so_far = 0;
    for (long long event = 0; event < 50; ++event) {
      for (int t = 0; t < T - 1; ++t) {
        ++attempts_so_far;
        CHECK(swap_attempt_ordinal(PTRWM_ORDER_SEQUENTIAL, event, T, t) == attempts_so_far, "sequential, T %d, event %lld, pair %d: ordinal %lld, attempt %lld",
              T, event, t, swap_attempt_ordinal(PTRWM_ORDER_SEQUENTIAL, event, T, t), attempts_so_far);
        CHECK(swap_attempt_ordinal(PTRWM_ORDER_EVEN_ODD, event, T, t) == event + 1, "even/odd, T %d, event %lld, pair %d: ordinal %lld", T, event, t,
              swap_attempt_ordinal(PTRWM_ORDER_EVEN_ODD, event, T, t));
      }
    }
  }

  // threads of an exchange group
  for (int T = 1; T <= 256; ++T) {
    int waves = 1;
    while (64 * waves < T) ++waves;
    const int thread_form = T <= 64 ? 64 : 64 * waves;
    CHECK(group_threads(T, 1) == thread_form, "thread form, T %d: %d threads, expected %d", T, group_threads(T, 1), thread_form);
    const int lane_split = 4 * T <= 64 ? 64 : lane_split_block_literal(T);
    CHECK(group_threads(T, 4) == lane_split, "lane-split form, T %d: %d threads, expected %d", T, group_threads(T, 4), lane_split);
  }
  CHECK(group_threads(17, 4) == 256 && packed_ladders_per_group(4 * 17) == 3, "T = 17: three ladders in 204 of 256 lanes");

  std::printf("rng layout ok: %lld checks\n", g_checks);
  return 0;
}
