"""Preconditioned Gaussian proposals restated in plain Python (csrc/precond.h is what is checked AGAINST this): the update of
the factor from one window's covariance sums in Python floats - IEEE doubles, every operation rounded on its own - and the
proposal rule with an exact float32 fused multiply-add.

fmaf is libm's, through ctypes (NumPy has none).  fmaf_vec is the same function on arrays: the product of two floats is exact in a
double, TwoSum gives the exact error of the double sum with the addend, and the sum is nudged to an odd last bit where it is inexact
(rounding to odd), after which the rounding to float32 is the rounding of the exact value - a double keeps 29 bits more than a
float, and two suffice.  tests/test_precond_host.py holds fmaf_vec to libm's fmaf."""
import ctypes
import ctypes.util
import math

import numpy as np

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fmaf.restype = ctypes.c_float
_libm.fmaf.argtypes = [ctypes.c_float, ctypes.c_float, ctypes.c_float]

BLOCK = 16  # the chain of coordinate i runs to the end of i's block of 16 (precond.h prec_chain_end)


def fmaf(a, b, c) -> float:
    return _libm.fmaf(float(a), float(b), float(c))


def fmaf_vec(a, b, c):
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(invalid="ignore"):  # (an infinite sum has no error term: it is left alone below)
        p = a * b  # exact: 24 + 24 bits
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)  # TwoSum: s + err == p + c exactly
    s = np.ascontiguousarray(np.broadcast_to(s, np.broadcast(s, err).shape)).copy()
    bits = s.view(np.int64)
    inexact = (err != 0) & np.isfinite(s) & ((bits & 1) == 0)
    away = (err > 0) == (s > 0)  # the exact value lies further from zero than s
    bits[inexact & away] += 1
    bits[inexact & ~away] -= 1
    with np.errstate(over="ignore"):
        return s.astype(np.float32)


def chain_end(i: int) -> int:
    return BLOCK * (i // BLOCK + 1)


ROWS = 64  # replica rows per tile (precond.h kPrecRows)
GROUPS_PER_CU = 8  # (precond.h kPrecGroupsPerCu)


def grid(n_tiles: int, cus: int) -> int:
    """Workgroups the proposal kernel is launched with (precond.h prec_grid): workgroup b walks tiles b, b + grid, ..."""
    return min(n_tiles, GROUPS_PER_CU * (cus if cus > 0 else 256))


def tiles(n_rows: int) -> int:
    return -(-n_rows // ROWS)


def propose_rows(x, chol, z, scale, exact_libm: bool = False):
    """y [n, dim] of the rule: inc_i = the fmaf chain over k = 0 .. chain_end(i) - 1 ascending of L[i][k] z[k] from +0 (L zero
    above the diagonal, z zero at and past dim), y_i = fmaf(s, inc_i, x_i).  x, z [n, dim] float32, chol [dim, dim] (only k <= i
    read), scale [n] float32.  exact_libm: every fmaf through libm, one by one (slow: small cases)."""
    x, z = np.asarray(x, np.float32), np.asarray(z, np.float32)
    chol, scale = np.asarray(chol, np.float32), np.asarray(scale, np.float32)
    n, dim = x.shape
    y = np.empty_like(x)
    if exact_libm:
        for r in range(n):
            for i in range(dim):
                acc = 0.0
                for k in range(chain_end(i)):
                    acc = fmaf(chol[i, k] if k <= i else 0.0, z[r, k] if k < dim else 0.0, acc)
                y[r, i] = fmaf(scale[r], acc, x[r, i])
        return y
    for i in range(dim):
        acc = np.zeros(n, np.float32)
        for k in range(chain_end(i)):
            acc = fmaf_vec(chol[i, k] if k <= i else np.float32(0), z[:, k] if k < dim else np.zeros(n, np.float32), acc)
        y[:, i] = fmaf_vec(scale, acc, x[:, i])
    return y


UPDATED, FEW_DRAWS, NOT_POSITIVE = 0, 1, 2


def update(sxx, sx, count, run_xx, run_x, run_w, memory, jitter, min_count, chol):
    """The update rule in Python floats.  sxx, run_xx [dim, dim] (lower triangle read), sx, run_x [dim], count, run_w scalars,
    chol float32 [dim, dim].  Returns (outcome, chol_new, run_xx_new, run_x_new, run_w_new): chol_new is chol where the update is
    skipped, else the rounded factor on the lower triangle and chol's own values above it."""
    dim = len(sx)
    memory, jitter, min_count = float(memory), float(jitter), float(min_count)
    rxx = [[0.0] * dim for _ in range(dim)]
    for i in range(dim):
        for j in range(i + 1):
            rxx[i][j] = memory * float(run_xx[i][j]) + float(sxx[i][j])
    rx = [memory * float(run_x[i]) + float(sx[i]) for i in range(dim)]
    w = memory * float(run_w) + float(int(count))
    out_xx = np.array(run_xx, np.float64)
    for i in range(dim):
        for j in range(i + 1):
            out_xx[i, j] = rxx[i][j]
    out = lambda code, c: (code, c, out_xx, np.array(rx, np.float64), w)  # noqa: E731
    keep = np.array(chol, np.float32)
    if not (w >= min_count and math.isfinite(w)):
        return out(FEW_DRAWS, keep)
    m = [_div(rx[i], w) for i in range(dim)]
    A = [[_div(rxx[i][j], w) - m[i] * m[j] for j in range(i + 1)] for i in range(dim)]
    tr = 0.0
    for i in range(dim):
        tr = tr + A[i][i]
    jt = jitter * _div(tr, float(dim))
    for i in range(dim):
        A[i][i] = A[i][i] + jt
    for j in range(dim):
        for i in range(j, dim):
            s = A[i][j]
            for k in range(j):
                s = s - A[i][k] * A[j][k]
            A[i][j] = s
        piv = A[j][j]
        if not (piv > 0.0 and math.isfinite(piv)):
            return out(NOT_POSITIVE, keep)
        d = math.sqrt(piv)
        A[j][j] = d
        for i in range(j + 1, dim):
            A[i][j] = _div(A[i][j], d)
    new = keep.copy()
    with np.errstate(over="ignore"):
        for i in range(dim):
            for j in range(i + 1):
                new[i, j] = np.float32(A[i][j])
    if not np.isfinite(np.tril(new)).all():
        return out(NOT_POSITIVE, keep)
    return out(UPDATED, new)


def _div(a: float, b: float) -> float:
    """IEEE division where Python raises (b == 0) or has no answer"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))
