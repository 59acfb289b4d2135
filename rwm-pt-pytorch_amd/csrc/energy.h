// The rule of the pooled log-density sums along the ladder, stated once: when a snapshot is due, what one snapshot adds to which
// sum - and, below it, the geometry of the snapshot kernel (energy_geometry and the index maps next to it).  Plain C++ (no HIP
// include): the two kernels of capi.hip call it, tests/energy_test.cpp replays the kernel's tiling with it against brute force.
//
// Snapshots.  A snapshot is due at every step with periodic_step_due(step_counter, burn_in, every) (schedule.h: the rule of the
// histograms, the autocovariance and the covariance).
// Sums, for every local chain c and temperature t, with l = logp[c, t] (float32, after the whole step: MH move and that step's
// swap event) and g = (chain_offset + c) mod groups, the chain's group by its GLOBAL id:
//   l not finite:  nonfinite[0] += 1, and nothing else
//   otherwise, x = (double) l, y = x - ref[t] (one double subtraction):
//     count[g, t] += 1 (int64)     s1[g, t] += x     s2[g, t] += x * x   (exact in double: fusing it into the sum changes nothing)
//     t >= 1:          colder[g, t] += exp(((double) beta[t - 1] - (double) beta[t]) * y)
//     t <= n_temps - 2: hotter[g, t] += exp(((double) beta[t + 1] - (double) beta[t]) * y)
// No addition follows the product in front of exp, so nothing can be contracted into it.  colder[:, 0] and hotter[:, n_temps - 1]
// are never written; with one temperature neither array is touched.  An overflowing exp leaves inf in its sum.  Only the order of
// the additions is free.
// ref [n_temps] (double) is the level the exponential sums are taken against, so that an unnormalised log-density - one offset by
// -1e6, say - neither overflows nor underflows.  While the flag ref_set[0] is 0, a due snapshot first sets ref[t] to the largest
// finite l of temperature t over the local chains (0 where none is finite) and the flag to 1 (energy_ref_of below); a non-zero
// flag leaves ref alone - a caller may pin ref and pre-set the flag, and shards that share a pinned ref have sums that add.
// Groups are disjoint sets of independent chains: the delete-one-group jackknife over them gives error bars that hold whatever
// the chains' autocorrelation in time, and a sharded run puts every chain in the group the unsharded run does.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#include "schedule.h"

namespace ptrwm {

constexpr int kEnergyMaxGroups = 64;  // PTRWM_ENERGY_MAX_GROUPS of include/ptrwm.h
constexpr int kEnergyMaxTemps = 256;  // PTRWM_MAX_TEMPS

// the group of local chain c: the mathematical mod, whatever the sign of the global id
PTRWM_HD constexpr int energy_group(long long chain_offset, long long c, int groups) {
  return (int)(((chain_offset + c) % groups + groups) % groups);
}

// ---- the reference level ---------------------------------------------------------------------------------------------------------
// Floats ordered as integers: a key that grows with the value, -0 below +0, every finite value between the infinities; no finite
// value (and no infinity) has the key kEnergyNoKey, which therefore stands for "no finite value yet".
constexpr int32_t kEnergyNoKey = INT32_MIN;
PTRWM_HD inline int32_t energy_float_bits(float v) {
  int32_t b;
  __builtin_memcpy(&b, &v, sizeof b);
  return b;
}
PTRWM_HD inline int32_t energy_key(float v) {
  const int32_t b = energy_float_bits(v);
  return b >= 0 ? b : (int32_t)(b ^ 0x7fffffff);
}
PTRWM_HD inline float energy_key_value(int32_t key) {
  const int32_t b = key >= 0 ? key : (int32_t)(key ^ 0x7fffffff);
  float v;
  __builtin_memcpy(&v, &b, sizeof v);
  return v;
}
PTRWM_HD inline bool energy_finite(float v) { return (energy_float_bits(v) & 0x7f800000) != 0x7f800000; }
// ref[t] from the largest key of the temperature's finite values
PTRWM_HD inline double energy_ref_of(int32_t key) { return key == kEnergyNoKey ? 0.0 : (double)energy_key_value(key); }

// ---- one term --------------------------------------------------------------------------------------------------------------------
// the argument of exp: (beta_to - beta_at) * (l - ref), every operand a double
PTRWM_HD inline double energy_exp_arg(float beta_to, float beta_at, double x, double ref) {
  const double d = (double)beta_to - (double)beta_at, y = x - ref;
  return d * y;
}

// ---- the geometry of one snapshot (capi.hip energy_snapshot_kernel) ----------------------------------------------------------------
// A workgroup of kEnergyThreads threads serves chains of ONE group (blockIdx.y = g): the local chains c with
// energy_group(chain_offset, c, groups) == g are energy_first_chain + k * groups, k = 0, 1, ...; blockIdx.x takes a tile of
// energy_tile_chains(n_temps) of them, about kEnergyTileElems floats.  Element e of a tile is temperature e % n_temps of the
// tile's chain e / n_temps, and thread i takes elements i, i + kEnergyThreads, ...: a chain's row is contiguous in t and lanes run
// along the rows, so a wave's load is whole cache lines for every n_temps - no power of two, longer than a wave - and where
// n_temps divides kEnergyThreads a thread stays on one temperature for the whole tile.  Per-(g, t) partial sums then need a table
// of 4 n_temps doubles (and n_temps counters) in LDS, flushed once per workgroup with zeros skipped.
constexpr int kEnergyThreads = 256;
constexpr int kEnergyTileElems = 4096;

PTRWM_HD constexpr int energy_tile_chains(int n_temps) { return kEnergyTileElems / n_temps > 1 ? kEnergyTileElems / n_temps : 1; }
// the first local chain of group g, and how many of the n_chains local chains belong to it
PTRWM_HD constexpr long long energy_first_chain(long long chain_offset, int groups, int g) {
  return ((long long)g - chain_offset % groups + groups) % groups;
}
PTRWM_HD constexpr long long energy_group_chains(long long n_chains, long long chain_offset, int groups, int g) {
  return energy_first_chain(chain_offset, groups, g) < n_chains
             ? (n_chains - energy_first_chain(chain_offset, groups, g) + groups - 1) / groups
             : 0;
}
// element e of tile `tile` of group g: its temperature, the chain's number within the group, and the local chain
PTRWM_HD constexpr int energy_elem_temp(int e, int n_temps) { return e % n_temps; }
PTRWM_HD constexpr long long energy_elem_member(long long tile, int e, int n_temps) {
  return tile * energy_tile_chains(n_temps) + e / n_temps;
}
PTRWM_HD constexpr long long energy_member_chain(long long chain_offset, int groups, int g, long long member) {
  return energy_first_chain(chain_offset, groups, g) + member * groups;
}
// the elements of tile `tile` of a group of `members` chains (0: the tile lies behind the group's last chain)
PTRWM_HD constexpr int energy_tile_elems(long long tile, long long members, int n_temps) {
  return members <= tile * energy_tile_chains(n_temps)
             ? 0
             : (int)((members - tile * energy_tile_chains(n_temps) < energy_tile_chains(n_temps)
                          ? members - tile * energy_tile_chains(n_temps)
                          : energy_tile_chains(n_temps)) *
                     n_temps);
}

struct EnergyGeometry {
  int tile_chains;      // chains of one group a workgroup takes
  long long tiles;      // workgroups along x: the tiles of the largest group
  int groups;           // workgroups along y
  long long max_members, min_members;  // chains of the largest and of the smallest group
  int last_tile_chains;                // chains in the last tile of the largest group
  int lds_doubles;                     // the table of partial sums
};

inline EnergyGeometry energy_geometry(int n_temps, long long n_chains, long long chain_offset, int groups) {
  EnergyGeometry g;
  g.tile_chains = energy_tile_chains(n_temps);
  g.groups = groups;
  g.max_members = 0;
  g.min_members = n_chains;
  for (int i = 0; i < groups; ++i) {
    const long long m = energy_group_chains(n_chains, chain_offset, groups, i);
    g.max_members = m > g.max_members ? m : g.max_members;
    g.min_members = m < g.min_members ? m : g.min_members;
  }
  g.tiles = (g.max_members + g.tile_chains - 1) / g.tile_chains;
  g.last_tile_chains = g.tiles > 0 ? (int)(g.max_members - (g.tiles - 1) * g.tile_chains) : 0;
  g.lds_doubles = 4 * n_temps;
  return g;
}

}  // namespace ptrwm
