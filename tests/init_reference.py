"""NumPy restatement of the starting-point draw of ptrwm_init_states (include/ptrwm.h, "starting points"): what the GPU
tests of the feature compare against - never the code under test.  Philox blocks come from the oracle's own
Philox4x32-10 (oracle.philox4x32_10, known-answer tested in tests/test_oracle_golden.py); everything after the block is
float32 NumPy, one rounding per operation as the header prescribes.  Not a test module."""
import numpy as np

from oracle import oracle as O

STREAM_INIT = 3


def expected_box_starts(seed, chain_offset, n_chains, n_temps, dim, lo, hi, attempt=0, per_temperature=False):
    """float32 [n_chains, n_temps, dim]: row (c, t), coordinate d, with g = chain_offset + c and tt = t if per_temperature
    else 0, is  lo[d] + (hi[d] - lo[d]) * u,  u = (word d % 4 >> 8) * 2^-24  of the block with counter
    (d // 4 | attempt << 16,  0,  g & 0xffffffff,  tt | 3 << 8 | (g >> 32) << 12)  and key (seed low, seed high)."""
    assert 0 <= attempt < 65536
    lo = np.broadcast_to(np.asarray(lo, dtype=np.float32), (dim,))
    hi = np.broadcast_to(np.asarray(hi, dtype=np.float32), (dim,))
    width = (hi - lo).astype(np.float32)  # sub_rn
    seed = int(seed) & (2**64 - 1)
    key = (seed & 0xFFFFFFFF, seed >> 32)
    n_blocks = (dim + 3) // 4
    out = np.empty((n_chains, n_temps, dim), dtype=np.float32)
    for c in range(n_chains):
        g = (int(chain_offset) + c) & (2**64 - 1)
        for tt in range(n_temps if per_temperature else 1):
            words = []
            for b in range(n_blocks):
                words += O.philox4x32_10((b | attempt << 16, 0, g & 0xFFFFFFFF, tt | STREAM_INIT << 8 | (g >> 32) << 12), key)
            w = np.array(words[:dim], dtype=np.uint64)
            u = (w >> np.uint64(8)).astype(np.float32) * np.float32(2.0**-24)  # < 2^24: exact in float
            row = (lo + (width * u).astype(np.float32)).astype(np.float32)  # mul_rn, add_rn
            if per_temperature:
                out[c, tt] = row
            else:
                out[c, :] = row
    return out
