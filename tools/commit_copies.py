"""Ratchet: the Metropolis commit of the one-thread-per-replica step kernels stays IN PLACE.

    python tools/commit_copies.py --check [--objs a.o b.o ... | libptrwm_hip.so] [--filter SUBSTRING]

Until round 6 every ordinary step of these kernels ended with DP + 1 v_mov_b32 v, v: the selects of the commit
x[d] = acc ? y[d] : x[d] wrote temporaries, and a block before the loop latch copied them into the registers of x[]
(62 VALU instructions of a dim-30 step's 977; profiles/r06_commit_in_place.txt, kernel.h "The step loop is two loops").
This tool disassembles the gfx950 code objects of built objects (or of the linked library) with llvm-objdump, finds in every
PRODUCTION thread-form step kernel (ptrwm_step_kernel<.., DP, EXACT, FULL = false, STREAM>) the loop of Metropolis steps -
the innermost loop that holds the Philox multiplies of a proposal - and fails if any basic block inside it holds DP or more
register-to-register v_mov_b32.  (The block that ENTERS that loop, once per swap_every steps, may hold such copies: the
row read back in a swap event lands next to the old state it is compared with.  It is reported, not failed.)

What --check fails on: any kernel with dim compiled in (EXACT: every BASELINE config runs one) of width >= MIN_WIDTH - below
that, DP copies in a block cannot be told from the handful of moves any block holds (widths 2 and 3 show 7 unrelated ones).
The run-time-dim kernels are counted against GENERIC_COPYING_CEILING, a ratchet: when the loop was reshaped, the Laplace
kernels of the generic widths (DP + 4 copies: the block-of-four dimension loop with the squared jump taken from the states)
and the width-8 Normal kernels (9) still copied - 118 kernels.  Lower the ceiling when they are fixed; never raise it.

Run by csrc/Makefile next to tools/kernel_stats.py --check, and by tests/test_commit_in_place.py on the built library."""
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
# production thread-form step kernel: <Target, Proposal, DP, EXACT, false, STREAM>
PROD = re.compile(r"^_ZN5ptrwm17ptrwm_step_kernelI.*ELi(\d+)ELb([01])ELb0ELb[01]EEEvNS_5KArgsE$")
MIN_WIDTH = 8
GENERIC_COPYING_CEILING = 118


def code_objects(path, tmp):
    """paths of the gfx950 code objects bundled in the .hip_fatbin section of a host object or shared library (a library
    holds one bundle per translation unit, back to back)"""
    fat = os.path.join(tmp, "fat")
    r = subprocess.run([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", path, os.path.join(tmp, "discard")],
                       capture_output=True)
    if r.returncode != 0 or not os.path.exists(fat):
        return []
    data = open(fat, "rb").read()
    out, pos = [], data.find(MAGIC)
    while pos >= 0:
        (n,) = struct.unpack_from("<Q", data, pos + len(MAGIC))
        p = pos + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", data, p)
            triple = data[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if "gfx950" in triple and size:
                co = os.path.join(tmp, f"co{len(out)}")
                open(co, "wb").write(data[pos + off:pos + off + size])
                out.append(co)
        pos = data.find(MAGIC, pos + len(MAGIC))
    return out


def production_kernels(co):
    names = subprocess.run([f"{LLVM}/llvm-readelf", "--symbols", "-W", co], capture_output=True, text=True, check=True).stdout
    return sorted({l.split()[-1] for l in names.splitlines() if " FUNC " in l and PROD.match(l.split()[-1])})


INS = re.compile(r"^\s+([a-z][a-z0-9_]+)\s*(.*?)\s*// ([0-9A-F]+): ([0-9A-F]{8})")
COPY = re.compile(r"^v\d+, v\d+$")
BRANCH = ("s_cbranch", "s_branch")


HEAD = re.compile(r"^[0-9a-f]+ <(\S+)>:$")


def instructions_of(co, symbols):
    """{symbol: [(address, opcode, operands, branch target or None)]} for the kernels named in `symbols` (the code object is
    disassembled once, whole)"""
    txt = subprocess.run([f"{LLVM}/llvm-objdump", "-d", co], capture_output=True, text=True, check=True).stdout
    out, cur = {}, None
    for l in txt.splitlines():
        m = HEAD.match(l)
        if m:
            cur = out.setdefault(m.group(1), []) if m.group(1) in symbols else None
            continue
        if cur is None:
            continue
        m = INS.match(l)
        if not m:
            continue
        addr, word = int(m.group(3), 16), int(m.group(4), 16)
        target = None
        if m.group(1).startswith(BRANCH):  # SOPP: the target is the next instruction plus a signed word offset
            off = word & 0xFFFF
            target = addr + 4 + 4 * (off - 0x10000 if off & 0x8000 else off)
        cur.append((addr, m.group(1), m.group(2), target))
    return out


def blocks_of(ins):
    """basic blocks (lists of instructions): split behind every branch and in front of every branch target"""
    targets = {i[3] for i in ins if i[3] is not None}
    blocks, cur = [], []
    for i in ins:
        if i[0] in targets and cur:
            blocks.append(cur)
            cur = []
        cur.append(i)
        if i[1].startswith(BRANCH + ("s_endpgm", "s_setpc")):
            blocks.append(cur)
            cur = []
    if cur:
        blocks.append(cur)
    return blocks


def metropolis_loop(ins):
    """(lo, hi) address range of the innermost loop that holds the Philox multiplies of a proposal: among the backward
    branches whose range holds at least half of the kernel's v_mad_u64_u32 / v_mul_hi_u32, the shortest range"""
    mults = [i[0] for i in ins if i[1].startswith(("v_mad_u64_u32", "v_mul_hi_u32"))]
    best = None
    for addr, _, _, target in ins:
        if target is None or target > addr:
            continue
        inside = sum(target <= x <= addr for x in mults)
        if mults and 2 * inside >= len(mults) and (best is None or addr - target < best[1] - best[0]):
            best = (target, addr)
    return best


def copy_blocks(symbol, ins):
    """(dp, worst copies in a block of the Metropolis loop, copies in the block that enters it) of one production kernel"""
    dp = int(PROD.match(symbol).group(1))
    blocks = blocks_of(ins)
    loop = metropolis_loop(ins)
    if loop is None:
        return dp, None, None
    n_copies = lambda b: sum(op.startswith("v_mov_b32") and COPY.match(args) is not None for _, op, args, _ in b)
    inside = [b for b in blocks if loop[0] <= b[0][0] <= loop[1]]
    before = [b for b in blocks if b[0][0] < loop[0]]
    return dp, max(n_copies(b) for b in inside), (n_copies(before[-1]) if before else 0)


def check_one(job):
    path, flt = job
    out = []
    with tempfile.TemporaryDirectory(prefix="commit_copies_") as tmp:
        for co in code_objects(path, tmp):
            wanted = {s for s in production_kernels(co) if flt in s}
            if wanted:
                for sym, ins in sorted(instructions_of(co, wanted).items()):
                    out.append((sym,) + copy_blocks(sym, ins))
    return out


def check(paths, flt=""):
    """[(symbol, dp, worst, entry)] for every production thread-form step kernel whose name contains `flt`"""
    jobs = [(p, flt) for p in paths]
    if len(jobs) == 1:
        return check_one(jobs[0])
    import multiprocessing
    with multiprocessing.Pool(min(8, len(jobs))) as pool:
        return [r for part in pool.map(check_one, jobs) for r in part]


def is_exact(symbol):
    return PROD.match(symbol).group(2) == "1"


def main():
    args = sys.argv[1:]
    flt = ""
    if "--filter" in args:
        i = args.index("--filter")
        flt = args[i + 1]
        del args[i:i + 2]
    strict = "--check" in args
    paths = [a for a in args if not a.startswith("--")]
    if not paths:
        paths = [os.path.join(ROOT, "rwm-pt-pytorch_amd", "lib", "libptrwm_hip.so")]
    res = check(paths, flt)
    copying = [r for r in res if r[2] is None or (r[1] >= MIN_WIDTH and r[2] >= r[1])]
    bad = [r for r in copying if r[2] is None or is_exact(r[0])]
    generic = [r for r in copying if r not in bad]
    for sym, dp, worst, entry in (copying if not strict else bad):
        print(f"{sym}: " + ("no Metropolis loop found" if worst is None else
                            f"a block of its Metropolis loop holds {worst} v_mov_b32 v, v (width {dp}): the commit is not in place"))
    if not strict:
        for sym, dp, worst, entry in res:
            print(f"{sym}: width {dp}, worst block of the Metropolis loop {worst} copies, entry block {entry}")
    if strict and not res:
        sys.exit("commit_copies --check: no production thread-form step kernel found: nothing was checked")
    if strict and bad:
        sys.exit(f"commit_copies --check: {len(bad)} of {len(res)} production thread-form step kernels with dim compiled in copy "
                 "their state every step")
    if strict and len(generic) > GENERIC_COPYING_CEILING:
        sys.exit(f"commit_copies --check: {len(generic)} run-time-dim kernels copy their state every step, ceiling "
                 f"{GENERIC_COPYING_CEILING} (a ratchet: find what made new ones copy)")
    print(f"commit_copies: {len(res)} production thread-form step kernels; dim compiled in, width >= {MIN_WIDTH}: none holds a "
          f"block of >= width copies in its Metropolis loop; run-time dim: {len(generic)} do (ceiling {GENERIC_COPYING_CEILING})")


if __name__ == "__main__":
    main()
