"""NumPy float64 restatement of csrc/ladder.h: the ladder update, the rescaling of the proposal scales, and the probe (every
pair's swap probability, with the bound of what a float32 evaluation of the same inputs may differ by).  The tests compare the
header (CPU) and the kernels (GPU) against this file; nothing here is used by the library."""
import numpy as np

Q = 16777216.0  # 2^24: the probe's quantum


def update(beta, pooled, gain_j):
    """beta float32 [T], pooled integers [T] (pair sums, chain-probes last), gain_j = gain / (j + 1)^decay.  Returns
    (beta_new float32 [T], outcome): 0 updated, 1 nothing probed, 2 skipped (the rounded ladder is not strictly decreasing).
    Every sum over t ascending (np.cumsum adds in order)."""
    beta = np.asarray(beta, np.float32)
    pooled = np.asarray(pooled, np.int64)
    T = beta.size
    if pooled[T - 1] <= 0:
        return beta.copy(), 1
    b = beta.astype(np.float64)
    r = pooled[:T - 1].astype(np.float64) / (float(pooled[T - 1]) * Q)
    rbar = np.cumsum(r)[-1] / (T - 1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        g = np.log(b[:-1]) - np.log(b[1:])
        G = np.cumsum(g)[-1]
        h = np.log(g) + gain_j * (r - rbar)
        w = np.exp(h - h.max())
        c = np.cumsum(w)
        new = beta.copy()
        new[1:T - 1] = (b[0] * np.exp(-G * c[:T - 2] / c[-1])).astype(np.float32)
    if not (new[:-1] > new[1:]).all():
        return beta.copy(), 2
    return new, 0


def rescale(scale, beta_old, beta_new):
    """temp_scale after the ladder moved: interior temperatures only, in double, rounded once."""
    s = np.asarray(scale, np.float32).copy()
    bo, bn = np.asarray(beta_old, np.float32).astype(np.float64), np.asarray(beta_new, np.float32).astype(np.float64)
    s[1:-1] = (s[1:-1].astype(np.float64) * np.sqrt(bo[1:-1] / bn[1:-1])).astype(np.float32)
    return s


def ulps(a, b):
    """Distance in float32 units in the last place between two arrays of finite floats of one sign."""
    return np.abs(np.asarray(a, np.float32).view(np.int32).astype(np.int64) - np.asarray(b, np.float32).view(np.int32).astype(np.int64))


def pair_rates(logp, beta):
    """Mean over chains of min(1, exp(lp)) for every neighbouring pair, in float64: logp [C, T], beta [T] -> [T - 1]."""
    lp64, _ = _log_prob(np.asarray(logp, np.float32), np.asarray(beta, np.float32))
    with np.errstate(over="ignore", invalid="ignore"):
        thr = np.where(lp64 >= 0, 1.0, np.exp(lp64))
    return np.where(np.isnan(thr), 0.0, thr).mean(0)


def _log_prob(logp, beta):
    """swap_log_prob's expression in float64 from the float32 inputs, [C, T - 1], and the sum of the magnitudes its seven float32
    roundings act on (four products, three running sums)."""
    l = logp.astype(np.float64)
    b = beta.astype(np.float64)
    bj, bk, lj, lk = b[None, :-1], b[None, 1:], l[:, :-1], l[:, 1:]
    with np.errstate(invalid="ignore", over="ignore"):
        p1, p2, p3, p4 = bj * lk, bk * lj, bj * lj, bk * lk  # (exact in double: 24 x 24 bits)
        s1 = p1 + p2
        s2 = s1 - p3
        s3 = s2 - p4
        mag = np.abs(p1) + np.abs(p2) + np.abs(p3) + np.abs(p4) + np.abs(s1) + np.abs(s2) + np.abs(s3)
    return s3, mag


def probe(logp, beta):
    """What ladder_probe_kernel adds to pooled for logp float32 [C, T] and beta float32 [T], evaluated in float64, and how far
    the kernel's integers may lie from it: (expected float64 [T - 1] in quanta, bound float64 [T - 1] in quanta, chains).

    The bound, element by element, with u = 2^-24 (half a float32 ulp, relative):
      * swap_log_prob rounds four products and three sums, each by at most u times its own magnitude:
            |lp32 - lp64| <= E = 1.001 u (|p1| + |p2| + |p3| + |p4| + |s1| + |s2| + |s3|)
        (magnitudes from the float64 evaluation; the 1.001 covers the second-order terms, the rounded magnitudes against the
        exact ones);
      * hw_exp(lp) = exp2(fl(lp * kLog2e)): the constant is log2(e) rounded to float (relative u), the product rounds once more
        (u), so the exponent is off by at most 2.001 u |lp| log2(e) on top of E log2(e); in natural-log units
            a = E + 2.001 u |lp32|  <=  E + 2.001 u (|lp64| + E);
      * v_exp_f32 is accurate to one unit in the last place of its result: a relative 2^-23;
      * so |thr32 - thr64| <= thr64 expm1(a) + 2^-23 min(1, thr64 e^a), which also covers an lp on the other side of 0 in
        float32 than in float64 (|lp| <= E there: 1 - e^-E <= thr64 expm1(a));
      * both thresholds lie in [0, 1], so no element is ever off by more than 1;
      * the quantisation llrint(thr 2^24) moves the value by at most half a quantum; one whole quantum is allowed.
    An element whose float64 lp is NaN (an infinite log-density on either side, or both) adds exactly 0 and has bound 0: the
    float32 evaluation meets the same inf - inf."""
    logp, beta = np.asarray(logp, np.float32), np.asarray(beta, np.float32)
    u = 2.0 ** -24
    lp64, mag = _log_prob(logp, beta)
    nan = np.isnan(lp64)
    with np.errstate(over="ignore", invalid="ignore"):
        thr = np.where(lp64 >= 0, 1.0, np.exp(lp64))
        E = 1.001 * u * mag
        a = E + 2.001 * u * (np.abs(lp64) + E)
        ok = a <= 50.0  # (beyond: magnitudes near the float range, nothing is claimed but that both thresholds lie in [0, 1])
        a = np.where(ok, a, 0.0)
        err = np.where(ok, np.minimum(1.0, thr * np.expm1(a) + 2.0 ** -23 * np.minimum(1.0, thr * np.exp(a))), 1.0)
    expected = np.where(nan, 0.0, thr * Q)
    bound = np.where(nan, 0.0, err * Q + 1.0)
    return expected.sum(0), bound.sum(0), logp.shape[0]
