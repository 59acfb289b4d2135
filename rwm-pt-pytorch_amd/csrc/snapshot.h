// What the accumulators that read `state` after a due step share - the pooled histograms (hist.h), the lagged autocovariance
// (acf.h), the posterior covariance (cov.h) and, for the due rule, the two split-moment kernels - stated once: when the step just
// performed is due, the head of a snapshot kernel's arguments, the tail of its launch, and the two questions ptrwm_run's launch
// loop asks of a block.  capi.hip's alone (HIP: it launches).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/ptrwm.h"
#include "schedule.h"

namespace ptrwm {

// Is the step just performed a due one of the block's period?  Its step counter (*sc, where asked for) is step + 1, or, on the
// device counter (include/ptrwm.h device_step), *device_step + step + 1.  (grid-uniform: every kernel of the family opens with it)
__device__ inline bool snapshot_step_due(long long step, const long long *device_step, long long burn_in, long long every,
                                         long long *sc = nullptr) {
  const long long c = (device_step != nullptr ? *device_step + step : step) + 1;
  if (sc != nullptr) *sc = c;
  return periodic_step_due(c, burn_in, every);
}

// The fields every snapshot kernel takes - what to read and whether the step counts - around the block's own pointers (Own: its
// sums and scratch).  Those sit behind `state`, where they always have: the kernels' argument offsets, and with them their
// machine code, are what they were when each block spelled the eight fields out.
template <class Own>
struct SnapHead {
  const void *state;  // float or double [n_chains, n_temps, dim]
  Own own;
  long long n_chains, step, burn_in, every;
  const long long *device_step;
  int n_temps, dim;
  __device__ bool due(long long *sc = nullptr) const { return snapshot_step_due(step, device_step, burn_in, every, sc); }
};

// One snapshot of the state after step `step` (device_step != NULL: *device_step + step), at the block's period
template <class Own>
inline void fill_snap_head(SnapHead<Own> &h, const ptrwm_run_args *args, int dim, long long every, long long step,
                           const long long *device_step) {
  h.state = args->state;
  h.n_chains = args->n_chains;
  h.step = step;
  h.burn_in = args->burn_in;
  h.every = every;
  h.device_step = device_step;
  h.n_temps = args->n_temps;
  h.dim = dim;
}

// the launch of a snapshot kernel, from its two instances: gx workgroups along x (refused where that is no grid), float or
// double states
template <class Args>
inline int32_t launch_snapshot(void (*of_float)(Args), void (*of_double)(Args), bool state_f64, long long gx, unsigned gy,
                               unsigned block, size_t lds_bytes, hipStream_t stream, const Args &a) {
  if (gx > 0x7fffffffll) return PTRWM_E_ARG;
  hipLaunchKernelGGL(state_f64 ? of_double : of_float, dim3((unsigned)gx, gy), dim3(block), lds_bytes, stream, a);
  return hipGetLastError() == hipSuccess ? PTRWM_OK : PTRWM_E_LAUNCH;
}

// ptrwm_run's launch loop (block: a ptrwm_hist_args, ptrwm_acf_args, ptrwm_cov_args or ptrwm_energy_args, or NULL - none): a launch ends at every
// due step of a block, since the snapshot kernel reads the state between launches ...
template <class Block>
inline long long steps_to_snapshot(const Block *b, long long step0, long long burn_in, long long cap) {
  return b != nullptr ? std::min(cap, steps_to_next_due(step0, burn_in, b->every)) : cap;
}
// ... and behind a launch whose last step has counter `sc`, the block's snapshot if that step is due (Launch: launch_hist,
// launch_acf, launch_cov or launch_energy of capi.hip)
template <auto Launch, class Block>
inline int32_t snapshot_if_due(const Block *b, const ptrwm_run_args *args, int32_t dim, long long sc, hipStream_t stream) {
  if (b == nullptr || !periodic_step_due(sc, args->burn_in, b->every)) return PTRWM_OK;
  return Launch(args, dim, b, sc - 1, nullptr, stream);
}

}  // namespace ptrwm
