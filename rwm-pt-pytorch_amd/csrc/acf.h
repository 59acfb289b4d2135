// The rule of the pooled lagged autocovariance, stated once: which snapshot a step is, which ring slot holds it, which lags a
// snapshot can pair with, what one term of a sum is - and, below it, the geometry of the snapshot kernel's grid (acf_geometry).
// Plain C++ (no HIP include): the snapshot kernel of capi.hip calls it, tests/acf_test.cpp checks it on the CPU against a
// step-by-step replay, and NumPy can replay every term bit for bit.
//
// Snapshots.  A snapshot is due at every step with periodic_step_due(step_counter, burn_in, every) (schedule.h: the rule of
// the histograms).  Its 0-based number j = periodic_step_number(step_counter, burn_in, every) comes from the step counter
// alone: nothing about "how many snapshots so far" lives on the host, so a snapshot can sit inside a captured block of split
// steps.
// Ring.  ring[max_lag][n_chains][temps * dim] holds the state's own type (float; double with state_f64).  Snapshot j lives in
// slot j % max_lag.  At snapshot j the lags k = 1 .. min(j, max_lag) are available (lag 0 always): x_{j-k} is read from slot
// (j - k) % max_lag.  The thread that owns an element reads it for every available lag and only THEN overwrites slot
// j % max_lag (which is also the slot of lag max_lag) with the current value; no other thread touches that element, so no
// ordering between workgroups is needed.
// Accumulators, for the first `temps` temperatures t, lags k = 0 .. max_lag and coordinates d, all += and all double:
//   sxy[t, k, d]  += sum over chains of x_j[t, d] * x_{j-k}[t, d]
//   head[t, k, d] += sum over chains of x_j[t, d]
//   tail[t, k, d] += sum over chains of x_{j-k}[t, d]
//   pairs[k]      += n_chains                                     (int64)
// x is the state in slot t of the ladder after the whole step (MH move and that step's swap event): the values a trace with
// trace_every = every records.  One term is acf_term: both values converted to double, ONE double product rounded once, never
// contracted into an fma with the running sum (for float states the product is exact anyway; for double states this is what
// makes a replay reproduce the term).  Only the order of the additions is free - tile sums are flushed with fp64 atomics, as
// the pooled moments are.  Estimators, on the host:  c_k = sxy_k / n_k - (head_k / n_k)(tail_k / n_k),  rho_k = c_k / c_0.
// Contract.  EVERY due step is snapshotted, in order: a skipped snapshot leaves a stale slot that later snapshots pair with
// as if it were x_{j-k}.  ptrwm_run_with_autocorr guarantees it; a stand-alone caller of ptrwm_autocorr is responsible for it.
#pragma once

#include "schedule.h"

namespace ptrwm {

constexpr int kAcfMaxLag = 1024;  // PTRWM_ACF_MAX_LAG of include/ptrwm.h

// the ring slot of snapshot j (>= 0)
PTRWM_HD inline int acf_slot(long long j, int max_lag) { return (int)(j % max_lag); }

// the largest lag snapshot j can pair with: lags 0 .. acf_lags(j, max_lag) are available
PTRWM_HD inline int acf_lags(long long j, int max_lag) { return j < max_lag ? (int)j : max_lag; }

// the slot that holds x_{j-k}, 1 <= k <= acf_lags(j, max_lag)
PTRWM_HD inline int acf_lag_slot(long long j, int k, int max_lag) { return acf_slot(j - k, max_lag); }

// one term of sxy: a product of its own, rounded once (see above)
PTRWM_HD inline double acf_term(double x, double y) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double p = x * y;
  return p;
}

// The geometry of one snapshot (capi.hip acf_snapshot_kernel), stated once.  The td = temps * dim covered columns of a chain's
// run are cut into `groups` groups (blockIdx.y) of `cols` columns, as equal as they come: groups = ceil(td / 256) - a workgroup
// has 256 threads, one column each at most - and cols = ceil(td / groups); the last group holds td - (groups - 1) * cols.  Where
// a group is narrower than the workgroup its threads take per = 256 / cols chains at a time (cold-only at dim 30: 8 chains of
// 30 columns, 240 threads).  A thread keeps kAcfChainsPerThread values of x_j in registers - its column of the chains
// sub, sub + per, sub + 2 per, ... of the tile - so a workgroup takes a tile of chains = per * kAcfChainsPerThread chains
// (blockIdx.x) and flushes one atomic per (lag, column) for it.
constexpr int kAcfThreads = 256;
constexpr int kAcfChainsPerThread = 32;

struct AcfGeometry {
  int cols, groups, per, chains;
};

inline AcfGeometry acf_geometry(int td) {
  AcfGeometry g;
  g.groups = (td + kAcfThreads - 1) / kAcfThreads;
  g.cols = (td + g.groups - 1) / g.groups;
  g.per = kAcfThreads / g.cols;
  g.chains = g.per * kAcfChainsPerThread;
  return g;
}

}  // namespace ptrwm
