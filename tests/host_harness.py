"""What the host tests (tests/*_host.py, test_capi_library.py, test_host_logic.py, test_multiprocess_cpu.py) share, stated once:
stand-alone C++ programs built under AddressSanitizer and UBSan and run as child processes, the C layout of the ctypes mirrors
read from include/ptrwm.h by a compiled probe, arguments that every entry point of the C ABI accepts up to its first HIP call,
and a gloo world of spawned CPU ranks.  A plain module next to helpers.py (which the GPU smoke run imports, so none of this
lives there); torch is imported only inside gloo_world."""
import ctypes as C
import os
import socket
import subprocess

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
HEADER = os.path.join(ROOT, "include", "ptrwm.h")

# ---- 1. sanitized stand-alone programs ----------------------------------------------------------------------------------
SANITIZE = ("-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def sanitized_exe(tmp_dir, source, *extra_flags, opt="-O1"):
    """tests/<source>, a program with its own main, compiled as plain C++ under AddressSanitizer and UBSan into tmp_dir; the
    executable's path.  A program that needs another flag passes it here, with the reason in a comment at the call."""
    exe = os.path.join(str(tmp_dir), os.path.splitext(source)[0])
    subprocess.check_call(["g++", "-std=c++17", opt, *SANITIZE, *extra_flags, os.path.join(TESTS, source), "-o", exe])
    return exe


def run_exe(exe, *argv, input=None, timeout=300, ok=None):
    """Run a built program as a child process; its stdout.  The exit status is always 0 - a sanitizer report is not - and
    where `ok` is given the program printed it."""
    out = subprocess.run([str(exe), *map(str, argv)], input=input, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    if ok is not None:
        assert ok in out.stdout, out.stdout[-2000:]
    return out.stdout


# ---- 2. the C layout of the ctypes mirrors ------------------------------------------------------------------------------
def c_layout(tmp_path, structs, macros=()):
    """A probe compiled with gcc against include/ptrwm.h: {"ptrwm_x_args": sizeof, "ptrwm_x_args.field": offsetof, ...} for
    structs = {"ptrwm_x_args": [field, ...]}, and {"PTRWM_Y": value} for every integer macro asked for."""
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){"]
    for s, fields in structs.items():
        lines.append(f'printf("{s} %zu\\n", sizeof({s}));')
        lines += [f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));' for f in fields]
    lines += [f'printf("{m} %d\\n", {m});' for m in macros]
    lines.append("return 0;}")
    src, exe = os.path.join(str(tmp_path), "probe.c"), os.path.join(str(tmp_path), "probe")
    with open(src, "w") as f:
        f.write("\n".join(lines))
    subprocess.check_call(["gcc", "-o", exe, src])
    return {k: int(v) for k, v in (ln.split() for ln in subprocess.check_output([exe], text=True).splitlines())}


def assert_layout(cls, c_name, fields, got):
    """The ctypes class has the size of the C struct and every field sits at its C offset."""
    who = f"{cls.__module__}.{cls.__name__} against {c_name}"
    assert C.sizeof(cls) == got[c_name], f"{who}: sizeof {C.sizeof(cls)}, in C {got[c_name]}"
    for f in fields:
        mine, in_c = getattr(cls, f).offset, got[f"{c_name}.{f}"]
        assert mine == in_c, f"{who}: {f} at {mine}, in C at {in_c}"


# ---- 3. arguments that pass every check up to the first HIP call --------------------------------------------------------
def valid_args(*blocks, n_temps=4, burn_in=0):
    """{"buf", "ptr", "td", "pd", "ra"} plus one entry per optional block asked for, all filled so that every entry point
    accepts them up to its first HIP call: rough carpet dim 30, Normal proposal, 4 chains, 10 steps, a swap event every step.
    Every pointer points at one 64-byte host buffer that a refused call never reads.  A test that leans on another value sets it
    on the returned structs and says which assertion needs it."""
    import ptrwm_hip as E

    buf = C.create_string_buffer(64)
    ptr = C.cast(buf, C.c_void_p)
    td, pd, ra = E.TargetDesc(), E.ProposalDesc(), E.RunArgs()
    td.kind, td.dim = E.TARGET_ROUGH_CARPET, 30
    pd.kind, pd.temp_scale = E.PROPOSAL_NORMAL, ptr
    ra.struct_size, ra.n_temps, ra.n_chains, ra.n_steps, ra.swap_every = C.sizeof(E.RunArgs), n_temps, 4, 10, 1
    ra.burn_in = burn_in
    ra.state = ra.logp = ra.beta = ptr
    v = {"buf": buf, "ptr": ptr, "td": td, "pd": pd, "ra": ra}
    for key in blocks:
        v[key] = b = getattr(E, _BLOCKS[key][0])()
        b.struct_size = C.sizeof(b)
        _BLOCKS[key][1](b, ptr, burn_in)
    return v


def _accumulator(m, ptr, _):
    m.temps, m.every, m.sum, m.sum_sq = 1, 1, ptr, ptr


def _flow(fl, ptr, _):
    fl.walker = ptr


def _hist(hi, ptr, _):
    hi.temps, hi.every, hi.n_bins = 1, 1, 64
    hi.lo = hi.scale = hi.counts = ptr


def _adapt(ad, ptr, burn_in):  # ten windows of 10 steps in a burn-in of 100; no window at all without a burn-in
    ad.every, ad.until, ad.target, ad.gain, ad.decay, ad.min_scale, ad.max_scale = 10, burn_in, 0.234, 3.0, 0.5, 1e-6, 1e6
    ad.temp_scale = ad.window_accept = ad.pooled = ptr


def _ladder(ld, ptr, burn_in):
    ld.every, ld.probe_every, ld.until, ld.gain, ld.decay, ld.rescale_scales = 10, 5, burn_in, 2.0, 0.5, 1
    ld.beta = ld.temp_scale = ld.pooled = ptr


def _acf(ac, ptr, _):
    ac.temps, ac.every, ac.max_lag = 1, 1, 8
    ac.ring = ac.sxy = ac.head = ac.tail = ac.pairs = ptr


def _cov(cv, ptr, _):
    cv.temps, cv.every = 1, 1
    cv.sxx = cv.sx = cv.count = ptr


def _precond(pa, ptr, _):
    pa.chol = ptr


def _precond_update(up, ptr, _):
    up.chol = up.sxx = up.sx = up.count = up.run_xx = up.run_x = up.run_w = ptr
    up.memory, up.jitter, up.min_count, up.windows = 0.5, 1e-6, 20.0, 3


def _init(init, ptr, _):
    init.lo = init.hi = ptr


# key -> (the block's ctypes class in ptrwm_hip, its one default filling); struct_size is set for all of them above
_BLOCKS = {"mom": ("MomentsArgs", _accumulator), "cmom": ("ChainMomentsArgs", _accumulator),
           "fl": ("FlowArgs", _flow), "hi": ("HistArgs", _hist), "ad": ("AdaptArgs", _adapt),
           "ld": ("LadderArgs", _ladder), "ac": ("AcfArgs", _acf), "cv": ("CovArgs", _cov),
           "pa": ("PrecondArgs", _precond), "up": ("PrecondUpdateArgs", _precond_update),
           "init": ("InitArgs", _init)}


# ---- 4. a gloo world of spawned CPU ranks -------------------------------------------------------------------------------
def _gloo_rank(rank, world, port, q, fn, args):
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    q.put((rank, fn(rank, *args)))
    dist.barrier()
    dist.destroy_process_group()


def gloo_world(fn, world=2, args=(), timeout=180):
    """fn(rank, *args) in each of `world` spawned processes that share a gloo process group; [(rank, fn's return value)] by
    rank.  fn is a top-level function of its module (spawn pickles it by name); what it asserts fails the test: a rank that
    raises exits non-zero, which is noticed here within a second instead of at the queue's timeout."""
    import queue
    import time

    import torch.multiprocessing as mp

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_rank, args=(r, world, port, q, fn, args)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        got, deadline = [], time.monotonic() + timeout
        while len(got) < world:
            try:
                got.append(q.get(timeout=1))
                continue
            except queue.Empty:
                pass
            assert not any(p.exitcode for p in procs), "a rank failed: its traceback is on stderr"
            assert time.monotonic() < deadline, f"no result from every rank within {timeout} s"
        for p in procs:
            p.join(60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
    return sorted(got, key=lambda t: t[0])
