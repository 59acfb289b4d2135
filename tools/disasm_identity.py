"""Which machine code changed between two builds of csrc/?

    python tools/disasm_identity.py PARENT_OBJDIR THIS_OBJDIR

The comparison behind profiles/r07_lds_layout_identity.txt, r08_chain_moments_disasm.txt, r09_moments_one_path_disasm.txt and
r11_swap_event_once.txt: both trees are built with csrc/Makefile into object directories of their own (make OBJDIR=... OUTDIR=...),
and for every object of either directory the gfx950 code object is extracted (tools/commit_copies.py code_objects) and
disassembled with llvm-objdump -d.  Per function symbol the sequence of (opcode, operands) is hashed - branch targets left out
(they move with the code around them), the s_nop padding behind a function's last instruction dropped - and the hashes of the
two sides are compared.  Kernels are classed by their template arguments:
  thread production / thread streaming / thread FULL twin      ptrwm_step_kernel<.., DP, EXACT, FULL, STREAM>
  lane-split production / lane-split FULL twin                 ptrwm_quad_step_kernel<.., W, DEXACT, MAXT, FULL, F64>
  other                                                        everything else (capi.o, the stand-alone log-density kernels)
Prints, per object, {class: [functions, identical to the parent's, not in the parent]} and the functions of the classes that
may not move, and exits non-zero if a production or streaming step kernel differs or exists on one side only: those kernels
sit at their register caps, and "the same machine code" is how a refactor of their source is shown to cost nothing.

It compares; it does not look for particular instructions."""
import hashlib
import json
import multiprocessing
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from commit_copies import BRANCH, HEAD, INS, LLVM, code_objects  # noqa: E402

THREAD = re.compile(r"^_ZN5ptrwm17ptrwm_step_kernelI.*ELi\d+ELb[01]ELb([01])ELb([01])EEEvNS_5KArgsE$")
QUAD = re.compile(r"^_ZN5ptrwm22ptrwm_quad_step_kernelI.*ELi\d+ELi\d+ELi\d+ELb([01])ELb[01]EEEvNS_5KArgsE$")
CLASSES = ("thread streaming", "thread FULL twin", "thread production", "lane-split FULL twin", "lane-split production", "other")
PINNED = ("thread streaming", "thread production", "lane-split production")  # must be the parent's, instruction for instruction


def kernel_class(symbol):
    m = THREAD.match(symbol)
    if m:
        return "thread FULL twin" if m.group(1) == "1" else ("thread streaming" if m.group(2) == "1" else "thread production")
    m = QUAD.match(symbol)
    if m:
        return "lane-split FULL twin" if m.group(1) == "1" else "lane-split production"
    return "other"


def function_hashes(path):
    """{function symbol: sha1 of its instruction sequence} over the gfx950 code objects of one host object"""
    out = {}
    with tempfile.TemporaryDirectory(prefix="disasm_identity_") as tmp:
        for co in code_objects(path, tmp):
            syms = subprocess.run([f"{LLVM}/llvm-readelf", "--symbols", "-W", co], capture_output=True, text=True, check=True).stdout
            funcs = {l.split()[-1] for l in syms.splitlines() if " FUNC " in l}
            txt = subprocess.run([f"{LLVM}/llvm-objdump", "-d", co], capture_output=True, text=True, check=True).stdout
            cur = None
            seqs = {}
            for l in txt.splitlines():
                m = HEAD.match(l)
                if m:
                    cur = seqs.setdefault(m.group(1), []) if m.group(1) in funcs else None
                    continue
                m = INS.match(l) if cur is not None else None
                if m:
                    cur.append((m.group(1), "" if m.group(1).startswith(BRANCH) else m.group(2)))
            for sym, seq in seqs.items():
                while seq and seq[-1][0] == "s_nop":
                    seq.pop()
                out[sym] = hashlib.sha1("\n".join(f"{op} {args}" for op, args in seq).encode()).hexdigest()
    return out


def objects_of(d):
    return {f for f in os.listdir(d) if f.endswith(".o")}


def demangle(symbols):
    if not symbols:
        return []
    tool = next((t for t in (f"{LLVM}/llvm-cxxfilt", shutil.which("llvm-cxxfilt"), shutil.which("c++filt")) if t and os.path.exists(t)), None)
    if tool is None:
        return list(symbols)
    r = subprocess.run([tool], input="\n".join(symbols), capture_output=True, text=True)
    return r.stdout.splitlines() if r.returncode == 0 else list(symbols)


def main():
    if len(sys.argv) != 3 or not all(os.path.isdir(a) for a in sys.argv[1:]):
        sys.exit(__doc__)
    parent_dir, this_dir = sys.argv[1:]
    names = sorted(objects_of(parent_dir) | objects_of(this_dir))
    jobs = [os.path.join(d, n) for n in names for d in (parent_dir, this_dir) if os.path.exists(os.path.join(d, n))]
    with multiprocessing.Pool(min(16, len(jobs) or 1)) as pool:
        hashed = dict(zip(jobs, pool.map(function_hashes, jobs)))
    total = {c: [0, 0, 0] for c in CLASSES}
    moved = []  # (object, class, symbol, what) of the pinned classes
    print("Per object: {class: [functions, identical to the parent's, not in the parent]}")
    for n in names:
        old = hashed.get(os.path.join(parent_dir, n))
        new = hashed.get(os.path.join(this_dir, n))
        if old is None or new is None:
            print(f"{n} only in {'the parent' if new is None else 'this tree'}")
            for sym in sorted(old or new):
                if kernel_class(sym) in PINNED:
                    moved.append((n, kernel_class(sym), sym, "missing in this tree" if new is None else "not in the parent"))
            continue
        row = {}
        for sym, h in new.items():
            c = kernel_class(sym)
            r = row.setdefault(c, [0, 0, 0])
            r[0] += 1
            r[1] += old.get(sym) == h
            r[2] += sym not in old
            if c in PINNED and old.get(sym) != h:
                moved.append((n, c, sym, "differs" if sym in old else "not in the parent"))
        for sym in old:
            if sym not in new and kernel_class(sym) in PINNED:
                moved.append((n, kernel_class(sym), sym, "missing in this tree"))
        for c, r in row.items():
            total[c] = [a + b for a, b in zip(total[c], r)]
        print(n, json.dumps({c: row[c] for c in CLASSES if c in row}))
    print("TOTAL [functions, identical to parent, new]", json.dumps({c: total[c] for c in CLASSES if total[c][0]}))
    if moved:
        print(f"\n{len(moved)} production / streaming step kernel(s) do not have the parent's machine code:")
        for (n, c, _, what), name in zip(moved, demangle([m[2] for m in moved])):
            print(f"  {n}  {c}  {what}: {name}")
        sys.exit(1)
    if not sum(total[c][0] for c in PINNED):
        sys.exit("disasm_identity: no production or streaming step kernel found: nothing was compared")
    print("\nevery production and streaming step kernel has the parent's machine code")


if __name__ == "__main__":
    main()
