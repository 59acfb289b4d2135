"""The Metropolis commit of the one-thread-per-replica step kernels is done in place: no basic block of the loop of
Metropolis steps of a production kernel holds a register-to-register copy per dimension (tools/commit_copies.py, the
ratchet the library's Makefile runs on every object).  Checked here on the BUILT library, for the kernels of BASELINE
configs[2] (RoughCarpet dim 30) and of the dim-50 rough carpet.  CPU only: the library is disassembled, not run."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def library():
    import ptrwm_hip

    if not os.path.exists(ptrwm_hip.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__

        __graft_entry__.build()
    return ptrwm_hip.LIB_PATH


# the folded rough carpet (RoughCarpetT<dim, 2>: the kernel bench.py's flagship workload runs) and the general one
@pytest.mark.parametrize("dim", [30, 50])
def test_rough_carpet_commit_is_in_place(library, dim):
    import commit_copies

    res = commit_copies.check([library], f"RoughCarpetTILi{dim}E")
    names = [r[0] for r in res]
    # every proposal, classic and streaming twin, of the folded and the general specialisation
    assert any(f"RoughCarpetTILi{dim}ELi2EEENS_14NormalProposalILi{dim}EEELi{dim}ELb1ELb0ELb0E" in n for n in names), names
    assert len(res) >= 6
    for sym, dp, worst, entry in res:
        assert dp == dim
        assert worst is not None, f"{sym}: no loop of Metropolis steps found in the disassembly"
        print(f"{sym}: worst block of the Metropolis loop {worst} copies, entry block {entry}")
        assert worst < dp, f"{sym}: a block of the Metropolis loop holds {worst} v_mov_b32 v, v: the commit is copied, not in place"


def test_the_check_sees_a_copy_block():
    """the block splitter and the copy count on a hand-written loop: a latch block of four copies is found"""
    import commit_copies

    ins = [(0, "v_mad_u64_u32", "v[0:1], s[0:1], v2, v3, 0", None), (8, "v_cndmask_b32_e32", "v9, v4, v5, vcc", None),
           (12, "s_cbranch_vccnz", "3", 28), (16, "v_mov_b32_e32", "v4, v9", None), (20, "v_mov_b32_e32", "v5, v10", None),
           (24, "v_mov_b32_e32", "v6, s3", None), (28, "v_mov_b32_e32", "v7, v11", None), (32, "s_cbranch_scc0", "65527", 0),
           (36, "s_endpgm", "", None)]
    assert commit_copies.metropolis_loop(ins) == (0, 32)
    blocks = commit_copies.blocks_of(ins)
    assert [len(b) for b in blocks] == [3, 3, 2, 1]
    copies = [sum(op.startswith("v_mov_b32") and commit_copies.COPY.match(a) is not None for _, op, a, _ in b) for b in blocks]
    assert copies == [0, 2, 1, 0]
