// The step-invariant head of a Philox4x32-10 block of the run layout (rng_layout.h), and the tail that finishes the block
// from it.  Plain C++ (no HIP include): the production step kernel calls both (kernel.h, proposals.h), and
// tests/philox_head_test.cpp checks tail(head(..)) against a literal Philox4x32-10 on the CPU.
//
// In a step kernel c2 (chain) and c3 (temperature | stream) are fixed per thread, c0 (block index | step >> 32) and c1
// (step) are wave-uniform.  Follow the rounds of one block (M0, M1 the multipliers, W0, W1 the key increments):
//   round 0:  c2 <- A = hi(M0 c0) ^ c3 ^ k1              c1 <- lo(M1 chain)               both step-invariant
//             c0 <- hi(M1 chain) ^ step ^ k0             c3 <- lo(M0 c0)
//   round 1:  P = M1 A,  c0 <- B = hi(P) ^ lo(M1 chain) ^ (k0 + W0),  c1 <- lo(P)         step-invariant
//             X = M0 (hi(M1 chain) ^ step ^ k0): per step, but the same for every block of the step
//             c2 <- hi(X) ^ lo(M0 c0) ^ (k1 + W1)        c3 <- lo(X)
//   round 2:  Q = M0 B                                                                    step-invariant
//             (h, l) = M1 c2;  c0 <- h ^ lo(P) ^ (k0 + 2 W0),  c1 <- l,  c2 <- hi(Q) ^ lo(X) ^ (k1 + 2 W1),  c3 <- lo(Q)
//   round 3:  c2 <- hi(M0 c0) ^ lo(Q) ^ (k1 + 3 W1), and everything else is the plain round from here on.
// Three words per block hold all that is step-invariant - PK = lo(P) ^ (k0 + 2 W0), QK = hi(Q) ^ (k1 + 2 W1),
// QL = lo(Q) ^ (k1 + 3 W1) - and with them a step enters each block at round 2: two multiplies and two xors less per block,
// and three round keys folded into words that are already there.  A head holds as long as c0 does: per block index, and
// until step >> 32 changes (schedule.h cuts launches there).
#pragma once
#include <stdint.h>

#include "rng_layout.h"

namespace ptrwm {

struct u32x4 {
  uint32_t x, y, z, w;
};

constexpr uint32_t kPhiloxM0 = 0xD2511F53u;
constexpr uint32_t kPhiloxM1 = 0xCD9E8D57u;
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u;
constexpr uint32_t kPhiloxW1 = 0xBB67AE85u;

// both halves of the 32 x 32 -> 64 product with a round multiplier (one v_mad_u64_u32 on the device, philox.h mul_hilo)
PTRWM_RNG_FN void philox_mul(uint32_t m, uint32_t x, uint32_t &hi, uint32_t &lo) {
  const uint64_t p = (uint64_t)m * x;
  hi = (uint32_t)(p >> 32);
  lo = (uint32_t)p;
}

// a ^ b ^ c with a round key among them: one v_bitop3_b32 on the device (philox.h philox4x32_10 says why it is spelt out)
PTRWM_RNG_FN uint32_t philox_xor3(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
#else
  return a ^ b ^ c;
#endif
}

struct PhiloxHead {
  uint32_t pk, qk, ql;
};

// the head of the block with counter word c0 (block index | step >> 32) of the thread whose chain word has the low product
// chain_lo = lo(M1 chain) and whose c3 (stream included) is given
PTRWM_RNG_FN PhiloxHead philox_head(uint32_t c0, uint32_t chain_lo, uint32_t c3, uint32_t k0, uint32_t k1) {
  uint32_t h0, l0, ph, pl, qh, ql;
  philox_mul(kPhiloxM0, c0, h0, l0);
  const uint32_t a = h0 ^ c3 ^ k1;
  philox_mul(kPhiloxM1, a, ph, pl);
  const uint32_t b = ph ^ chain_lo ^ (k0 + kPhiloxW0);
  philox_mul(kPhiloxM0, b, qh, ql);
  return {pl ^ (k0 + 2u * kPhiloxW0), qh ^ (k1 + 2u * kPhiloxW1), ql ^ (k1 + 3u * kPhiloxW1)};
}

// the step's own product: (x_hi, x_lo) = M0 (hi(M1 chain) ^ step ^ k0), shared by every block of the step
PTRWM_RNG_FN void philox_step_product(uint32_t chain_hi, uint32_t c1, uint32_t k0, uint32_t &x_hi, uint32_t &x_lo) {
  philox_mul(kPhiloxM0, chain_hi ^ c1 ^ k0, x_hi, x_lo);
}

// rounds 2 .. 9 from a head: the block philox4x32_10(c0, c1, c2, c3, k0, k1), bit for bit
PTRWM_RNG_FN u32x4 philox_tail(const PhiloxHead &head, uint32_t c0, uint32_t x_hi, uint32_t x_lo, uint32_t k0, uint32_t k1) {
  uint32_t hi0, lo0, hi1, lo1;
  // round 2 (the wave-uniform part of its input, lo(M0 c0) ^ (k1 + W1), is scalar work)
  philox_mul(kPhiloxM1, x_hi ^ ((kPhiloxM0 * c0) ^ (k1 + kPhiloxW1)), hi1, lo1);
  uint32_t n0 = hi1 ^ head.pk;
  uint32_t c1 = lo1;
  uint32_t c2 = head.qk ^ x_lo;
  // round 3
  philox_mul(kPhiloxM0, n0, hi0, lo0);
  philox_mul(kPhiloxM1, c2, hi1, lo1);
  k0 += 3u * kPhiloxW0;
  k1 += 3u * kPhiloxW1;
  n0 = philox_xor3(hi1, c1, k0);
  c2 = hi0 ^ head.ql;
  c1 = lo1;
  uint32_t c3 = lo0;
#ifdef __clang__
#pragma unroll
#endif
  for (int r = 4; r < 10; ++r) {
    k0 += kPhiloxW0;
    k1 += kPhiloxW1;
    philox_mul(kPhiloxM0, n0, hi0, lo0);
    philox_mul(kPhiloxM1, c2, hi1, lo1);
    n0 = philox_xor3(hi1, c1, k0);
    c2 = philox_xor3(hi0, c3, k1);
    c1 = lo1;
    c3 = lo0;
  }
  return u32x4{n0, c1, c2, c3};
}

// top 24 bits of a raw word -> (0, 1]: (k + 1) 2^-24 as ONE fma, k 2^-24 + 2^-24.  Every (k + 1) 2^-24 with k < 2^24 is a
// float, so nothing rounds: the value of ((float)k + 1) * 2^-24 for every input, without the integer add in front of the
// conversion that form was compiled to (tests/philox_head_test.cpp walks all 2^24).
PTRWM_RNG_FN float u01_open0(uint32_t r) { return __builtin_fmaf((float)(r >> 8), 0x1p-24f, 0x1p-24f); }

}  // namespace ptrwm
