// What tests/schedule_test.cpp, adapt_test.cpp and ladder_test.cpp share: the brute-force statement of the warm-up windows that
// csrc/schedule.h is checked against, and floats as their bit patterns.
#pragma once

#include <cstdint>
#include <cstring>

// window k of `every` steps adapts iff it ends at or before `until`; step s adapts iff the window it lies in does
inline bool bf_step_adapts(long long s, long long every, long long until, long long *window) {
  for (long long k = 0; (k + 1) * every <= until; ++k)
    if (k * every <= s && s < (k + 1) * every) {
      *window = k;
      return true;
    }
  return false;
}

inline float from_bits(uint32_t b) {
  float f;
  std::memcpy(&f, &b, 4);
  return f;
}
inline uint32_t to_bits(float f) {
  uint32_t b;
  std::memcpy(&b, &f, 4);
  return b;
}
