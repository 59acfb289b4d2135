"""The thread form's running sums that start from their first term (csrc/philox.h chain_add) on the CPU (no GPU needed):
the argument that no output bit can tell them from the sums that start from zero."""
from host_harness import run_exe, sanitized_exe


def test_sums_from_the_first_term_close_to_the_bits_of_sums_from_zero(tmp_path):
    """tests/sum_first_term_test.cpp, a program of its own, built under AddressSanitizer and UBSan: for ranges of 1 to 8
    terms drawn from {+-0, denormals, ordinary values, a value that overflows, +inf} the chain from the first term and the
    chain from zero are equal or zeros of different sign - different exactly when every term is -0; the four-range tree
    keeps that; and after the closing arithmetic of each user - the double accumulation from +0.0 of the squared jump,
    fmaf(sum + lg, kLn2, p7) with p7 != 0 of the rough carpet - the bits are the same."""
    # -ffp-contract=off: the claim is about chains of single IEEE additions, as add_rn on the device - nothing may be contracted
    # into an fma on the way to the closing fmaf
    exe = sanitized_exe(tmp_path, "sum_first_term_test.cpp", "-ffp-contract=off")
    run_exe(exe, ok="sums from the first term ok: 19173960 ranges (8 differ in a zero's sign)")
