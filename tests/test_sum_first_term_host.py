"""The thread form's running sums that start from their first term (csrc/philox.h chain_add) on the CPU (no GPU needed):
the argument that no output bit can tell them from the sums that start from zero."""
import os
import subprocess


def test_sums_from_the_first_term_close_to_the_bits_of_sums_from_zero(tmp_path):
    """tests/sum_first_term_test.cpp, a program of its own, built under AddressSanitizer and UBSan: for ranges of 1 to 8
    terms drawn from {+-0, denormals, ordinary values, a value that overflows, +inf} the chain from the first term and the
    chain from zero are equal or zeros of different sign - different exactly when every term is -0; the four-range tree
    keeps that; and after the closing arithmetic of each user - the double accumulation from +0.0 of the squared jump,
    fmaf(sum + lg, kLn2, p7) with p7 != 0 of the rough carpet - the bits are the same."""
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sum_first_term_test.cpp")
    exe = str(tmp_path / "sum_first_term_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-ffp-contract=off", src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "sums from the first term ok: 19173960 ranges (8 differ in a zero's sign)" in out.stdout
