"""csrc/swap_walk.h on the CPU (no GPU needed): the lane-mask walk that decides the sequential exchange sweep of the step
kernel's one-wavefront exchange groups, against a literal restatement of the sweep."""
from host_harness import run_exe, sanitized_exe


def test_swap_walk_is_the_sequential_scan(tmp_path):
    """csrc/swap_walk.h compiled as plain C++ under AddressSanitizer and UBSan into tests/swap_walk_test.cpp, a program of
    its own.  Exhaustive: T = 2..6, every assignment of the T log-densities and T - 1 thresholds from seven values that
    include +-inf and NaN (7^(2T-1) ladders each, side by side in wavefronts, the last wavefront of a range partly idle).
    Random: T in {7, 8, 16, 21, 31, 32, 63, 64}, every number of ladders per wavefront, random bits in the idle lanes'
    mask positions, the threshold and the literal rule mixed per ladder within a wavefront.  For every position: the
    source lane, the travelled log-density (bit for bit) and pair_acc equal the scan's."""
    # -ffp-contract=off: the literal rule of a pair is four products summed left to right, each rounded on its own;
    # -O2 and -pthread: two billion exhaustive ladders, which the program spreads over 16 std::threads
    exe = sanitized_exe(tmp_path, "swap_walk_test.cpp", "-ffp-contract=off", "-pthread", opt="-O2")
    run_exe(exe, timeout=600, ok="swap walk ok: 2018521043 ladders exhaustive (T = 2..6, seven values), 18000 random wavefronts "
                                 "of 63000 ladders")
