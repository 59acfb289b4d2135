"""csrc/swap_walk.h on the CPU (no GPU needed): the lane-mask walk that decides the sequential exchange sweep of the step
kernel's one-wavefront exchange groups, against a literal restatement of the sweep."""
import os
import subprocess


def test_swap_walk_is_the_sequential_scan(tmp_path):
    """csrc/swap_walk.h compiled as plain C++ under AddressSanitizer and UBSan into tests/swap_walk_test.cpp, a program of
    its own.  Exhaustive: T = 2..6, every assignment of the T log-densities and T - 1 thresholds from seven values that
    include +-inf and NaN (7^(2T-1) ladders each, side by side in wavefronts, the last wavefront of a range partly idle).
    Random: T in {7, 8, 16, 21, 31, 32, 63, 64}, every number of ladders per wavefront, random bits in the idle lanes'
    mask positions, the threshold and the literal rule mixed per ladder within a wavefront.  For every position: the
    source lane, the travelled log-density (bit for bit) and pair_acc equal the scan's."""
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "swap_walk_test.cpp")
    exe = str(tmp_path / "swap_walk_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-pthread",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert ("swap walk ok: 2018521043 ladders exhaustive (T = 2..6, seven values), 18000 random wavefronts of 63000 ladders"
            in out.stdout)
