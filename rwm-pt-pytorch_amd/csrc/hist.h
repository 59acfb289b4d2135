// The bin rule of the pooled marginal histograms, stated once: which of the n_bins + 2 counters of a coordinate a value
// lands in - and, below it, the geometry of the snapshot kernel's grid (hist_geometry).  Plain C++ (no HIP include): the
// snapshot kernel of capi.hip calls the rule, tests/hist_test.cpp checks it on the CPU against a double-precision
// restatement, and NumPy can replay it bit for bit (np.float32 arithmetic, astype(np.int64)).
//
// A coordinate d has n_bins equal bins over [lo[d], hi[d]) and two end bins; its counters are
//   bin 0             underflow: x < lo[d] - and NaN, see below
//   bin 1 .. n_bins   the bins proper, bin 1 + i covering [lo + i w, lo + (i + 1) w), w = (hi - lo) / n_bins
//   bin n_bins + 1    overflow: x >= hi[d], +inf included
// The caller supplies scale[d] = n_bins / (hi[d] - lo[d]) as a float (the Python layer computes
// float32(n_bins) / (float32(hi) - float32(lo)) in float32).  For a value x (a float; a double state is rounded to float first,
// as the log-density kernels do):
//   u   = (x - lo[d]) * scale[d]      two float operations, each rounded on its own.  (A difference followed by a product has
//                                     no fused form - contraction fuses a product INTO a sum - so no compiler flag changes it.)
//   bin = 0                           if !(u >= 0)
//   bin = n_bins + 1                  if u >= n_bins
//   bin = 1 + (int)u                  otherwise (truncation; 0 <= u < n_bins, so the conversion is always defined)
// NaN: every comparison with NaN is false, so !(u >= 0) holds and a NaN coordinate is counted in bin 0, the UNDERFLOW bin - a
// state that has gone NaN shows up as out-of-range mass instead of vanishing from the totals.  -0.0 >= 0 holds: bin 1.
// Because the rule is evaluated in float, a value within a rounding error of an edge (hi included: (hi - lo) * scale may
// round to just below n_bins) can land in the neighbouring bin of where real arithmetic would put it.  x = lo always lands in
// bin 1, and the rule is monotone in x.  What the counters hold is therefore defined by THIS rule, not by the real edges.
#pragma once

#ifndef PTRWM_HD
#ifdef __HIPCC__
#define PTRWM_HD __host__ __device__
#else
#define PTRWM_HD
#endif
#endif

namespace ptrwm {

constexpr int kHistMaxBins = 1024;  // PTRWM_HIST_MAX_BINS of include/ptrwm.h

PTRWM_HD inline int hist_bin(float x, float lo, float scale, int n_bins) {
  const float d = x - lo;
  const float u = d * scale;
  if (!(u >= 0.0f)) return 0;
  if (u >= (float)n_bins) return n_bins + 1;
  return 1 + (int)u;
}

// The geometry of one snapshot (capi.hip hist_snapshot_kernel), stated once: how the td = temps * dim covered columns of a
// chain's run are tiled into groups (blockIdx.y) of `cols` columns, chains into tiles of kHistChains (blockIdx.x).  A
// workgroup has 256 threads, so a group has at most 256 columns; the LDS strategy keeps n_bins + 2 32-bit counters per column
// of its group in kHistLdsCounters counters (32 KiB: up to five workgroups per CU), as many columns as fit; `direct` - no LDS,
// every sample a global atomic - when fewer than kHistMinCols columns (a wavefront's worth) would fit.  The last group holds
// td - (groups - 1) * cols columns.  Host code: launch_hist calls it, tests/hist_test.cpp checks it for every n_bins and td
// the C ABI accepts.
constexpr int kHistChains = 256;
constexpr int kHistLdsCounters = 8192;
constexpr int kHistMinCols = 64;
constexpr int kHistMaxCols = 256;  // the workgroup's threads

struct HistGeometry {
  int direct, cols, groups;
};

inline HistGeometry hist_geometry(int n_bins, int td) {
  const int nbp = n_bins + 2;
  HistGeometry g;
  g.direct = nbp > kHistLdsCounters / kHistMinCols ? 1 : 0;
  int cols = g.direct ? kHistMaxCols : kHistLdsCounters / nbp;  // (>= kHistMinCols)
  if (cols > kHistMaxCols) cols = kHistMaxCols;
  if (cols > td) cols = td;
  g.cols = cols;
  g.groups = (td + cols - 1) / cols;
  return g;
}

}  // namespace ptrwm
