"""csrc/philox_head.h on the CPU (no GPU needed): the head / tail split of a Philox block that the production step kernel of
the headline shape runs, the launch cut that keeps a parked head valid, and the one-fma u01_open0."""
from host_harness import run_exe, sanitized_exe


def test_philox_head_and_tail_are_the_plain_block(tmp_path):
    """csrc/philox_head.h compiled as plain C++ under AddressSanitizer and UBSan into tests/philox_head_test.cpp, a program
    of its own: philox_tail(philox_head(..)) equals a literal Philox4x32-10 (itself pinned to the published known answers)
    on 10^6 random (key, step, chain, temperature, stream, block) tuples and on the crossed corners - every block index
    0..26, steps and chain ids on both sides of 2^32, streams 0 and 1; u01_open0 equals its former two-operation form on all
    2^24 inputs; csrc/schedule.h lets no launch hold steps with different high words, and cuts nothing else."""
    run_exe(sanitized_exe(tmp_path, "philox_head_test.cpp"),
            ok="philox head ok: 1045363 blocks, 16777216 u01_open0 inputs, 22320 launches")
