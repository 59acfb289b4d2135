/*
 * ptrwm.h -- C ABI of the MI355X (gfx950) PT-RWM sampling engine.
 *
 * This is the drop-in boundary for the per-step hot loop of the reference
 * (aidanmrli/rwm-pt-pytorch):
 *
 *   algorithms/rwm_gpu_optimized.py:289-336   _single_step_ultra_fused
 *   algorithms/rwm_gpu_optimized.py:402-488   generate_samples (the `for i in range(total_steps)` loop)
 *   algorithms/pt_rwm_gpu_optimized.py:541-574 step
 *   algorithms/pt_rwm_gpu_optimized.py:594-633 _attempt_all_swaps
 *   algorithms/pt_rwm_gpu_optimized.py:694-770 generate_samples
 *
 * The reference has no FFI of its own (it is pure Python on torch tensors); the
 * binding a maintainer adds is the ctypes stub shown in INTEGRATION.md.  All
 * pointers named "device" are raw HIP device pointers (e.g. torch
 * `tensor.data_ptr()` on a ROCm build); `stream` is a `hipStream_t` passed as
 * `void*` (torch: `torch.cuda.current_stream().cuda_stream`).  Nothing here
 * retains a pointer past the call, allocates device memory, or synchronises:
 * every entry point only enqueues kernels on `stream`.
 *
 * Device contract (the usual HIP one): the device that owns `stream` and every
 * pointer must be the CURRENT device of the calling thread (hipSetDevice); the
 * library never switches devices.  The Python binding does this around every
 * call (ptrwm_hip.on_device), so `device="cuda:1"` works without set_device.
 *
 * All entry points return 0 on success or a negative PTRWM_E_* code; no C++
 * exception crosses this boundary.
 */
#ifndef PTRWM_H
#define PTRWM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PTRWM_ABI_VERSION 3
#define PTRWM_SPLIT_NO_SWEEP 1 /* ptrwm_run_args.split_flags, device-step mode: do not enqueue the swap kernel for this step */
#define PTRWM_MAX_DIM 104  /* dim-vector lives in VGPRs; widest compiled variant */
#define PTRWM_MAX_TEMPS 256 /* one ladder lives in one wavefront (<= 64 temps) or one workgroup; above dim 64 (lane-split
                              kernel only, 512-thread workgroups): at most 128, longer ladders get PTRWM_E_NOVARIANT */

/* ---- status codes ------------------------------------------------------ */
enum {
  PTRWM_OK = 0,
  PTRWM_E_NULL = -1,        /* required pointer is NULL */
  PTRWM_E_DIM = -2,         /* dim outside [1, PTRWM_MAX_DIM] or invalid for the target */
  PTRWM_E_TEMPS = -3,       /* n_temps outside [1, PTRWM_MAX_TEMPS] */
  PTRWM_E_KIND = -4,        /* unknown target / proposal kind */
  PTRWM_E_ARG = -5,         /* other invalid argument (negative counts, swap_every < 1 ...) */
  PTRWM_E_STRUCT = -6,      /* struct_size does not match this ABI version */
  PTRWM_E_LAUNCH = -7,      /* HIP reported a launch error */
  PTRWM_E_NOVARIANT = -8    /* (target, proposal, dim) variant not compiled into this build */
};

/* ---- target densities ---------------------------------------------------
 * Each kind restates the fp32 `log_density` of one reference class. */
enum {
  /* target_distributions/multimodal_torch.py:470-510 RoughCarpetDistributionTorch
   *   p[0..2] = modes, p[3..5] = log weights, p[6] = log_jacobian (0 if unscaled)
   *   vec0 = scaling_factors[dim] or NULL */
  PTRWM_TARGET_ROUGH_CARPET = 0,
  /* multimodal_torch.py:173-242 ThreeMixtureDistributionTorch (cov = I)
   *   p[0..2] = log_norm_const_k + log_mixing_weight_k (+ log_jacobian if scaled)
   *   vec0 = means[3*dim] (row-major [3][dim]); vec1 = scaling_factors[dim] or NULL
   *   ip[0] = 1: the caller DECLARES that the three mean vectors are equal in every coordinate but the first (the
   *   class's default centres (-5,0,..), (0,..), (5,0,..) and the +-15 centres of experiment_pt_GPU.py:48-52 are): the
   *   kernel then evaluates the part of |s x - mu_k|^2 the components share once instead of three times (a third of the
   *   work, same tolerance).  ip[0] = 0: no assumption.  A false declaration gives a wrong density. */
  PTRWM_TARGET_THREE_MIXTURE = 1,
  /* rosenbrock_torch.py:67-84 FullRosenbrockTorch: p[0]=a, p[1]=b, vec0 = mu[dim-1] */
  PTRWM_TARGET_FULL_ROSENBROCK = 2,
  /* rosenbrock_torch.py:194-210 EvenRosenbrockTorch: p[0]=a, p[1]=b, vec0 = mu[dim/2] */
  PTRWM_TARGET_EVEN_ROSENBROCK = 3,
  /* rosenbrock_torch.py:312-351 HybridRosenbrockTorch: p[0]=a, p[1]=b, p[2]=mu,
   *   ip[0]=n1, ip[1]=n2, dim = 1 + n2*(n1-1) */
  PTRWM_TARGET_HYBRID_ROSENBROCK = 4,
  /* iid_product_torch.py:52-91 IIDGammaTorch: p[0]=shape, p[1]=scale, p[2]=log_norm_const (dim * 1d) */
  PTRWM_TARGET_IID_GAMMA = 5,
  /* iid_product_torch.py:188-229 IIDBetaTorch: p[0]=alpha, p[1]=beta, p[2]=log_norm_const (dim * 1d) */
  PTRWM_TARGET_IID_BETA = 6,
  /* Gaussians with diagonal structure:
   *   ip[0] = 0: multivariate_normal_torch.py:62-92 MultivariateNormalTorch with a DIAGONAL covariance:
   *              -0.5 sum_d vec1[d] (x_d - vec0[d])^2 + p[0];  vec0 = mean, vec1 = diag(cov_inv), p[0] = log_norm_const
   *   ip[0] = 1: multivariate_normal_torch.py:199-224 ScaledMultivariateNormalTorch:
   *              p[0] - 0.5 sum_d (vec0[d] x_d)^2;  vec0 = scaling_factors, p[0] = log_norm_const */
  PTRWM_TARGET_DIAG_GAUSSIAN = 7,
  /* hypercube_torch.py:49-78 HypercubeTorch: p[0] = left, p[1] = right, p[2] = log uniform density; -inf outside */
  PTRWM_TARGET_HYPERCUBE = 8,
  /* funnel_torch.py:39-76 NealFunnelTorch: p[0] = mu_v, p[1] = sigma_v^2, p[2] = mu_z; x[0] = v, x[1..] = z */
  PTRWM_TARGET_NEAL_FUNNEL = 9,
  PTRWM_TARGET_COUNT = 10
};

typedef struct ptrwm_target_desc {
  int32_t kind;
  int32_t dim;
  float p[12];
  int32_t ip[4];
  const float *vec0; /* device, see kind */
  const float *vec1; /* device, see kind */
} ptrwm_target_desc;

/* ---- proposal increments -------------------------------------------------
 * increment[d] for the replica at temperature t. */
enum {
  /* proposal_distributions/normal.py:33-36,46-55 and pt_rwm_gpu_optimized.py:445-455,576-592
   *   inc_d = temp_scale[t] * z_d,  z ~ N(0,1) */
  PTRWM_PROPOSAL_NORMAL = 0,
  /* proposal_distributions/laplace.py:24-37,46-69
   *   u = U[0,1) - 0.5;  inc_d = -(dim_scale[d]*temp_scale[t]) * sign(u) * log1p(max(-2|u|, -0.999999)) */
  PTRWM_PROPOSAL_LAPLACE = 1,
  /* proposal_distributions/uniform.py:27-37,47-73
   *   g = N(0,I_dim); n = |g| (1 if <= 1e-12); inc = g/n * temp_scale[t] * U^{inv_dim} */
  PTRWM_PROPOSAL_UNIFORM_RADIUS = 2,
  PTRWM_PROPOSAL_COUNT = 3
};

typedef struct ptrwm_proposal_desc {
  int32_t kind;
  float inv_dim;           /* UNIFORM_RADIUS: 1/dim as the reference stores it */
  const float *temp_scale; /* device [n_temps] */
  const float *dim_scale;  /* device [dim], LAPLACE only (NULL otherwise) */
} ptrwm_proposal_desc;

/* ---- swap semantics (pt_rwm_gpu_optimized.py:594-633) ---- */
enum {
  PTRWM_SWAP_EXCHANGE = 0,       /* rows j and k trade places (algorithms/pt_rwm.py:141-150) */
  PTRWM_SWAP_REFERENCE_COPY = 1  /* row j <- row k, row k unchanged: what
                                    fused_swap_execution_no_clone (pt_rwm_gpu_optimized.py:51-59) does */
};
enum {
  PTRWM_ORDER_SEQUENTIAL = 0, /* j = 0..T-2 in order, each sees the previous outcome (reference) */
  PTRWM_ORDER_EVEN_ODD = 1    /* n-th swap event (0-based) attempts the disjoint pairs j == n (mod 2) */
};

/* ---- form of the fused step kernel ---------------------------------------
 * ptrwm_run has two bit-identical implementations of the same loop (same Philox words, same per-dimension arithmetic,
 * every sum over dimensions in one canonical order): one thread per (chain, temperature) replica, and a lane-split
 * form with four lanes per replica for launches that would otherwise under-fill the GPU (fewer than two wavefronts
 * per SIMD); above dim 64 only the lane-split form exists.  AUTO picks by batch size and dim; the choice cannot change
 * a result, only the speed.  ptrwm_set_kernel_form pins it process-wide (tests, tuning) and returns the previous
 * value, or PTRWM_E_ARG. */
enum {
  PTRWM_FORM_AUTO = 0,
  PTRWM_FORM_THREAD = 1, /* one thread per replica wherever that variant exists (dim <= 64) */
  PTRWM_FORM_QUAD = 2    /* lane-split wherever that variant exists (dim <= 64: n_temps <= 128; dim > 64: all) */
};
int32_t ptrwm_set_kernel_form(int32_t form);
/* 1 if ptrwm_run has a lane-split variant for (target, proposal, dim, n_temps), else 0. */
int32_t ptrwm_has_quad_variant(int32_t target_kind, int32_t proposal_kind, int32_t dim, int32_t n_temps);
/* 1 if ptrwm_run has a one-thread-per-replica variant for (target, proposal, dim), else 0 (never above dim 64).  Where it
 * returns 0 PTRWM_FORM_THREAD runs the lane-split kernel: a comparison of the two forms is vacuous there. */
int32_t ptrwm_has_thread_variant(int32_t target_kind, int32_t proposal_kind, int32_t dim);
/* The form PTRWM_FORM_AUTO runs for a float-state launch of this shape on the current device (PTRWM_FORM_THREAD or
 * PTRWM_FORM_QUAD), or a negative status.  Introspection only: the forms give the same bits. */
int32_t ptrwm_auto_form(int32_t target_kind, int32_t proposal_kind, int32_t dim, int32_t n_temps, int64_t n_chains);
/* The same rule for a device of n_simds SIMDs (no HIP call: a pure function of its arguments and of the fitted table). */
int32_t ptrwm_auto_form_for(int32_t target_kind, int32_t proposal_kind, int32_t dim, int32_t n_temps, int64_t n_chains,
                            int32_t n_simds);
/* SIMDs (compute units x 4) of the device that owns `stream` (NULL: the calling thread's current device): what the AUTO
 * rule of ptrwm_run scales by; PTRWM_E_LAUNCH if the runtime cannot say (AUTO then keeps the thread form). */
int32_t ptrwm_device_simds(void *stream);
/* Identity of the build as far as kernel speed goes: sha256 over the kernel sources (tools/source_hash.py), and the hash
 * of the sources the AUTO form table (csrc/form_table.inc) was fitted on.  Different strings: the table is stale - the
 * forms still give the same bits, AUTO may just not pick the faster one - re-fit with tools/form_sweep.py + form_fit.py. */
const char *ptrwm_source_hash(void);
const char *ptrwm_form_table_source_hash(void);

/* ---- short launches ------------------------------------------------------
 * A launch of one step over a large batch (the reference's step()-at-a-time loops, rwm_gpu_optimized.py:456-457,
 * pt_rwm_gpu_optimized.py:736-737) is bound by memory traffic; for it ptrwm_run has a STREAMING form of the
 * one-thread-per-replica kernel: persistent wavefronts that walk the batch with the next group's state already in flight
 * while the current one is stepped and the previous one's results drain.  Same Philox words and arithmetic: the same bits
 * as the classic kernel.  AUTO takes it for one-step launches whose arrays total about the size of the Infinity Cache
 * (192-448 MiB: where it measured faster, csrc/capi.hip), where the variant has a streaming twin (dim compiled in,
 * n_temps <= 64) and the batch's layout allows whole aligned 16-byte vectors per group; OFF never; ON wherever twin and
 * layout allow (tests, tuning).  Process-wide; returns the previous value, or PTRWM_E_ARG. */
enum {
  PTRWM_STREAM_AUTO = 0,
  PTRWM_STREAM_OFF = 1,
  PTRWM_STREAM_ON = 2
};
int32_t ptrwm_set_stream_mode(int32_t mode);
/* 1 if the one-thread-per-replica variant for (target, proposal, dim) has a streaming twin, else 0. */
int32_t ptrwm_has_stream_variant(int32_t target_kind, int32_t proposal_kind, int32_t dim);

/* Which kernel the calling thread's most recent successful ptrwm_run enqueued (introspection for tests and benchmark
 * records; 0 before the first call). */
enum {
  PTRWM_LAUNCH_THREAD = 1, /* one thread per replica, classic form */
  PTRWM_LAUNCH_QUAD = 2,   /* lane-split form */
  PTRWM_LAUNCH_STREAM = 3  /* one thread per replica, streaming form */
};
int32_t ptrwm_last_launch_kind(void);

/* Which specialisation of the target's functor the calling thread's most recent successful ptrwm_run used
 * (introspection for tests; 0 before the first call): the general functor, the specialised one (RoughCarpet: the
 * smallest mixture term proven negligible; ThreeMixture: means that differ in the first coordinate only), or the
 * folded RoughCarpet (modes -m, 0, +m). */
enum {
  PTRWM_FUNCTOR_GENERAL = 0,
  PTRWM_FUNCTOR_SPECIALISED = 1,
  PTRWM_FUNCTOR_FOLDED = 2
};
int32_t ptrwm_last_launch_functor(void);

/* Number of raw random numbers one MH proposal consumes from `ext_prop`
 * (NORMAL: dim normals; LAPLACE: dim uniforms in [0,1); UNIFORM_RADIUS: dim
 * normals then one uniform). */
int32_t ptrwm_ext_raw_per_step(int32_t proposal_kind, int32_t dim);

typedef struct ptrwm_run_args {
  uint32_t struct_size; /* sizeof(ptrwm_run_args) */
  int32_t n_temps;
  int64_t n_chains;     /* independent ladders (RWM: independent chains) on this device */
  int64_t chain_offset; /* global id of local chain 0: the Philox subsequence, so results do not
                           depend on how chains are sharded over devices */
  /* state, device, updated in place */
  float *state; /* [n_chains, n_temps, dim] */
  float *logp;  /* [n_chains, n_temps] log-density of `state` */
  const float *beta; /* [n_temps] inverse temperatures, beta[0] is the cold chain */
  /* statistics, device, accumulated (+=); any may be NULL */
  int64_t *n_accept;    /* [n_chains, n_temps] MH acceptances at steps with step_counter > burn_in */
  double *sq_jump;      /* [n_chains, n_temps] sum of |x_t - x_{t-1}|^2 over those steps (swap moves included).  For an
                         * accepted Metropolis move of the Normal / UniformRadius proposals in Philox mode this is the
                         * squared length of the increment itself, which equals that of the float sum x + inc to ~3e-5
                         * relative or better wherever it is used: a replica whose largest |coordinate| exceeds 256
                         * typical increments when a launch loads it takes the jump from the states instead.
                         * That choice is made once per LAUNCH, from the state the launch starts with: state, logp and
                         * every counter are independent of how a run is cut into launches, sq_jump is too unless a
                         * replica crosses that bound in the middle of a launch - then the two cuts differ in the last
                         * bits of that replica's sum (both within the ~3e-5 above; the oracle follows the same rule
                         * per launch, tests/test_gpu_engine_parity.py test_squared_jump_across_the_trust_boundary). */
  int64_t *swap_accept; /* [n_chains, n_temps] accepted swaps of pair (t, t+1); column n_temps-1 unused */
  int64_t *last_swap_ordinal; /* [n_chains, n_temps] max 1-based attempt ordinal at which pair t accepted */
  /* schedule: this call performs steps step0 .. step0+n_steps-1 (0-based); step i has
   * step_counter = i+1.  Swaps happen after the MH move of a step when
   * step_counter % swap_every == 0 and step_counter > burn_in (pt_rwm_gpu_optimized.py:544,570). */
  int64_t step0;
  int64_t n_steps;
  int64_t burn_in;
  int32_t swap_every;
  int32_t swap_mode;
  int32_t swap_order;
  int32_t swap_event_offset; /* swap events performed outside ptrwm_run (ptrwm_swap_sweep) before this call: added to
                                the event numbers this call derives from step0 (attempt ordinals, even/odd parity) */
  uint64_t seed; /* Philox4x32-10 key */
  /* external randoms (test / fixture mode); all NULL => in-kernel Philox */
  const float *ext_prop;   /* [n_steps, n_chains, n_temps, ptrwm_ext_raw_per_step()] */
  const float *ext_u;      /* [n_steps, n_chains, n_temps] accept uniforms */
  const float *ext_swap_u; /* [n_swap_events_in_call, n_chains, n_temps-1] */
  /* optional per-step outputs */
  float *trace;        /* [trace_rows, trace_chains, trace_temps, dim] state after each traced step of this call */
  float *trace_logp;   /* [trace_rows, trace_chains, trace_temps] */
  int64_t trace_chains; /* first trace_chains local chains are traced */
  int32_t trace_temps;  /* first trace_temps temperatures are traced (1 = cold chain only) */
  int32_t trace_every;  /* thinning: a step is traced when step_counter % trace_every == 0 (0 or 1 = every step) */
  int64_t trace_row0;   /* row written by the first traced step of this call */
  uint8_t *accept_flags; /* [n_steps, n_chains, n_temps] MH accept decision of every step, or NULL */
  /* 0: as declared above.  1 (ptrwm_run only): `state`, `trace` and `ext_prop` point to DOUBLE arrays of the same shapes -
   * the reference's dtype=torch.float64 (pt_rwm_gpu_optimized.py:134,431-449; experiment_pt_GPU.py:236
   * --use_double_precision): states, the proposals x + scale * z and the squared-jump sums are carried in double, so a
   * state far from the origin keeps the low bits of its increments; log-densities (evaluated on the proposal rounded to
   * float), uniforms, temperatures and proposal scales stay float.  ext_prop in this mode: NORMAL proposal only (the
   * reference's PT class is Gaussian only).  Always the lane-split form of the kernel; ladders of <= 128 temperatures. */
  int32_t state_f64;
  int32_t split_flags; /* device-step mode of the split steps only (below); must be 0 everywhere else */
  /* Split steps only (ptrwm_split_propose / ptrwm_split_accept / ptrwm_split_advance; must be NULL for ptrwm_run and
   * ptrwm_swap_sweep): device pointer to a step counter.  When set, the step a call performs is *device_step + step0 -
   * the kernels read the counter from device memory, `step0` is an OFFSET baked into the call - and burn-in and swap
   * schedule are derived from that on the device: the argument list of the k-th step of a block no longer depends on
   * where the run stands, so a block of split steps - the caller's density evaluation included - can be captured ONCE in
   * a HIP graph (torch.cuda.CUDAGraph) with step0 = 0, 1, ..., n - 1 and ONE ptrwm_split_advance (n_steps = n) as its last
   * node, and replayed.  ptrwm_split_accept enqueues the swap kernel with every step (it returns at once when no event is
   * due) unless split_flags has PTRWM_SPLIT_NO_SWEEP set: the caller's assertion that the step is NOT a swap step - its
   * to keep (a caller that replays a block only from counters that are multiples of swap_every knows which offsets are
   * swap steps; a wrong assertion loses the event silently).  External randoms (ext_prop / ext_u / ext_swap_u) are not
   * available in this mode. */
  const int64_t *device_step;
} ptrwm_run_args;

/* Advance every (chain, temperature) replica by n_steps Metropolis steps (with
 * swaps) in one fused kernel launch on `stream`. */
int32_t ptrwm_run(const ptrwm_target_desc *target, const ptrwm_proposal_desc *proposal,
                  const ptrwm_run_args *args, void *stream);

/* ---- posterior moments pooled over every replica ------------------------------------------------------------------
 * A moments accumulator covers the first `temps` temperatures (1 = the cold chain only, n_temps = all).  For each such
 * temperature t, over every local chain, at every step whose step_counter > burn_in and step_counter % every == 0:
 *   sum[t, d] += x_d,   sum_sq[t, d] += x_d * x_d,   sum_logp[t] += logp,   count[t] += 1
 * where x / logp are the replica's state and log-density after the whole step (MH move and that step's swap event) - the
 * values a trace with trace_every = every records at that step.  Sums are fp64 and only ever added to (+=), so launches,
 * calls and shards compose; the order of the additions is unspecified (atomics), so two runs may differ in the last bits
 * of a sum.  ptrwm_swap_sweep events are not steps and add nothing.  No other output of the run changes: state, logp and
 * every counter are bit-identical to the same run without moments.
 * Limits:
 *  - the accumulators must be ordinary device memory of the current device (hipMalloc / a torch tensor): they are
 *    added to with hardware fp64 atomics, which fine-grained host memory does not support;
 *  - ptrwm_run_with_moments runs the fixture / trace twin of the step kernel (never the streaming form) and keeps the
 *    partial sums in LDS: temps * (2 dim + 1) doubles per exchange group (a wavefront of up to 64 / n_temps ladders in the
 *    thread form, of up to 16 / n_temps ladders in the lane-split form; the whole workgroup for longer ladders), on top
 *    of what the kernel already holds, at most 160 KiB per workgroup.  Cold-only (temps = 1) fits every shape; all
 *    temperatures fit e.g. dim 30 with up to 64 temperatures in the thread form.  A shape that does not fit returns
 *    PTRWM_E_ARG before anything is enqueued (use fewer temps, or pin the other form with ptrwm_set_kernel_form);
 *  - partial sums are flushed once per launch (ptrwm_run splits requests of more than 2^16 steps into several). */
typedef struct ptrwm_moments_args {
  uint32_t struct_size; /* sizeof(ptrwm_moments_args) */
  int32_t temps;        /* 1..n_temps: the first `temps` temperatures */
  int32_t every;        /* >= 1: thinning period of the accumulated steps */
  double *sum;          /* [temps, dim] device, += (required) */
  double *sum_sq;       /* [temps, dim] device, += (required) */
  double *sum_logp;     /* [temps] device, +=, or NULL */
  int64_t *count;       /* [temps] device, +=, or NULL: the number of (chain, step) pairs added per temperature */
} ptrwm_moments_args;

/* ptrwm_run, and the moments of `moments` accumulated over the steps it performs.  moments == NULL: exactly ptrwm_run.
 * PTRWM_E_STRUCT for a wrong struct_size; PTRWM_E_ARG for temps outside 1..n_temps, every < 1, or an accumulator too
 * big for the kernel's LDS (above); PTRWM_E_NULL for a NULL sum / sum_sq. */
int32_t ptrwm_run_with_moments(const ptrwm_target_desc *target, const ptrwm_proposal_desc *proposal,
                               const ptrwm_run_args *args, const ptrwm_moments_args *moments, void *stream);

/* Split steps: the moments of the step ptrwm_split_accept just performed (enqueue it after ptrwm_split_accept, which
 * includes the step's swap event).  Reads from `args`: n_temps, n_chains, state, logp, burn_in, step0, device_step.  The
 * step is args->step0, or *device_step + step0 in device-step mode - read on the device, so the call can sit inside a
 * captured block of split steps.  A step that does not count adds nothing.  Same argument checks as
 * ptrwm_run_with_moments (no LDS limit: a small stand-alone kernel). */
int32_t ptrwm_split_moments(const ptrwm_run_args *args, int32_t dim, const ptrwm_moments_args *moments, void *stream);

/* ---- posterior moments of every chain on its own: R-hat and ESS without a trace -----------------------------------------
 * The same accumulation as ptrwm_moments_args, kept apart per local chain c (RWM: chain; PT: ladder) instead of pooled.
 * For chain c and each of the first `temps` temperatures t, at every step whose step_counter > burn_in and
 * step_counter % every == 0:
 *   sum[c, t, d] += x_d,   sum_sq[c, t, d] += x_d * x_d,   sum_logp[c, t] += logp
 * where x / logp are the state and log-density at position (c, t) after the whole step (MH move and that step's swap
 * event) - exactly what a trace with trace_every = every records at that step - and count[t] += 1: the accumulated steps
 * of every chain.  Everything is device memory and is added to (+=), so launches and calls compose.
 * Determinism: each element is the SEQUENTIAL fp64 sum of its terms in step order (x_d * x_d is the exact fp64 product of
 * the state element) - no atomics between chains, one exchange group owns each element.  It does not depend on where a run
 * is cut into launches, on the kernel form (pinned or AUTO's choice) or on how chains are sharded over devices; two runs
 * give the same bits.  No other output of the run changes: state, logp and every counter are bit-identical to the same run
 * without moments.  ptrwm_swap_sweep events are not steps and add nothing.
 * How: the fixture / trace twin of the step kernel (never the streaming form) loads its exchange group's part of the
 * accumulators into LDS when a launch begins, adds to it there, and stores it back with plain stores when the launch ends;
 * a launch without an accumulated step touches nothing.
 * Limit: the LDS region is  L * temps * (2 dim + 1)  doubles per exchange group, L = ladders per group:
 *   thread form, n_temps <= 64:       L = 64 / n_temps,  four groups (waves) per workgroup
 *   thread form, n_temps  > 64:       L = 1,             one group per workgroup
 *   lane-split form, n_temps <= 16:   L = 16 / n_temps,  four groups (waves) per workgroup
 *   lane-split form, n_temps  > 16:   L = the whole ladders (4 n_temps lanes each) that best fill a workgroup of up to 256
 *                                     threads (n_temps 20: 3; n_temps >= 33: 1), one group per workgroup
 * and  groups per workgroup * region * 8 bytes  plus what the kernel already holds (thread form: 4 (DP + 8) bytes per thread,
 * DP = register width >= dim; lane-split: 4 (W + 2) bytes per thread, W = ceil(dim / 4) rounded up to a compiled width,
 * twice W for double states) must stay within 160 KiB per workgroup (RWM at dim 30, thread form: 4 x 64 chains x 61 doubles
 * on top of 38 912 bytes is exactly 160 KiB - one workgroup per CU; lane-split form: 4 x 16 x 61 doubles on top of 10 240).
 * Under PTRWM_FORM_AUTO, where both forms exist and the form AUTO would run needs more than half of that (or does not fit),
 * the other form runs if it needs less - RWM at dim 30 runs the lane-split form; the forms give the same bits.
 * PTRWM_E_ARG - before anything is enqueued - only when the pinned form, or neither form, fits. */
typedef struct ptrwm_chain_moments_args {
  uint32_t struct_size; /* sizeof(ptrwm_chain_moments_args) */
  int32_t temps;        /* 1..n_temps: the first `temps` temperatures */
  int32_t every;        /* >= 1: thinning period of the accumulated steps */
  double *sum;          /* [n_chains, temps, dim] device, += (required) */
  double *sum_sq;       /* [n_chains, temps, dim] device, += (required) */
  double *sum_logp;     /* [n_chains, temps] device, +=, or NULL */
  int64_t *count;       /* [temps] device, +=, or NULL: the accumulated steps per chain */
} ptrwm_chain_moments_args;

/* ptrwm_run, and the per-chain moments accumulated over the steps it performs.  chain_moments == NULL: exactly ptrwm_run.
 * Checked before anything is enqueued, as ptrwm_run_with_moments: PTRWM_E_STRUCT for a wrong struct_size; PTRWM_E_ARG for
 * temps outside 1..n_temps, every < 1, or a region too big for the kernel's LDS (above); PTRWM_E_NULL for a NULL sum / sum_sq. */
int32_t ptrwm_run_with_chain_moments(const ptrwm_target_desc *target, const ptrwm_proposal_desc *proposal,
                                     const ptrwm_run_args *args, const ptrwm_chain_moments_args *chain_moments, void *stream);

/* Split steps: the per-chain moments of the step ptrwm_split_accept just performed (enqueue it after ptrwm_split_accept).
 * Reads from `args` what ptrwm_split_moments reads; the step is args->step0, or *device_step + step0 in device-step mode -
 * read on the device, so the call can sit inside a captured block of split steps.  A step that does not count adds
 * nothing.  One thread per (chain, t < temps, d), a plain read-modify-write: the same sequential sums as the fused kernels.
 * Same argument checks as ptrwm_run_with_chain_moments (no LDS limit). */
int32_t ptrwm_split_chain_moments(const ptrwm_run_args *args, int32_t dim, const ptrwm_chain_moments_args *chain_moments,
                                  void *stream);

/* ---- replica flow through the ladder: round trips and up-fraction without a trace ----------------------------------------
 * swap_accept says how often neighbouring temperatures trade; it does not say whether anything travels the ladder.  Replica
 * flow does (Katzgraber et al. 2006): every position (c, t) carries a FLOW WORD that moves with its row through every swap
 * event - bits 0..15 a walker id, bits 16..17 a direction: 0 none, 1 up (the last end it touched was the cold one, t = 0),
 * 2 down (the hot one, t = n_temps - 1).  The caller starts a run with walker[c, t] = t (direction none) and zeroed counters.
 * At every swap event of ladder c, with src[t] the position whose post-Metropolis row the event puts at position t:
 *   1. new[t] = old[src[t]] for every t.  PTRWM_SWAP_EXCHANGE: a permutation, T distinct walkers for ever.
 *      PTRWM_SWAP_REFERENCE_COPY: a copy, as the rows are copied - ids repeat and vanish; an id then names the LINEAGE of the
 *      vector at a position (which starting position it descends from), and round_trips counts by lineage;
 *   2. ends: at t = 0 a word whose direction is down has completed a round trip (cold -> hot -> cold):
 *      round_trips[c, id] += 1 (an id >= n_temps, which only a walker array the caller did not initialise can hold, is
 *      counted nowhere), and its direction becomes up; at t = n_temps - 1 its direction becomes down;
 *   3. visits: for every t, direction up: n_up[c, t] += 1; down: n_down[c, t] += 1; none: nothing.
 * f(t) = n_up / (n_up + n_down) is the fraction of visits to temperature t by replicas coming from the cold end: 1 at t = 0,
 * 0 at the hot end, falling roughly linearly over a well-placed ladder; a plateau or a cliff shows where replicas turn back.
 * Determinism: everything is integer, each element has one writer per event and events are ordered by the stream - the
 * results are exact and do not depend on where a run is cut into launches, on the kernel form (pinned or AUTO's choice),
 * on how chains are sharded over devices (chain_offset), or on whether the events come from ptrwm_run, from split steps or
 * from stand-alone sweeps.  No other output of a run changes: state, logp and every counter are bit-identical to the same
 * run without flow.
 * How: the fixture / trace twin of the step kernel (never the streaming form) parks the word of every position in LDS when a
 * launch begins, exchanges it next to the rows in every swap event (round_trips is updated there, by the thread of
 * temperature 0), and stores the words back and adds the launch's visit counts when the launch ends.
 * Limits: n_temps >= 2; 16 bytes of LDS per replica on top of what the kernel and its moments regions hold (thread form:
 * 16 per thread; lane-split form: 4 per thread), at most 160 KiB per workgroup together - a shape that does not fit returns
 * PTRWM_E_ARG before anything is enqueued; the arrays are ordinary device memory of the current device. */
typedef struct ptrwm_flow_args {
  uint32_t struct_size; /* sizeof(ptrwm_flow_args) */
  int32_t reserved;     /* 0 */
  int32_t *walker;      /* [n_chains, n_temps] device, in/out, required: flow words */
  int64_t *round_trips; /* [n_chains, n_temps] device, +=, indexed by walker id; or NULL */
  int64_t *n_up;        /* [n_chains, n_temps] device, +=, indexed by temperature; or NULL */
  int64_t *n_down;      /* [n_chains, n_temps] device, +=, indexed by temperature; or NULL */
} ptrwm_flow_args;

/* ptrwm_run with any of its diagnostics: pooled moments OR per-chain moments (at most one of the two non-NULL, else
 * PTRWM_E_ARG), and replica flow.  flow == NULL: exactly ptrwm_run / ptrwm_run_with_moments / ptrwm_run_with_chain_moments.
 * Checked before anything is enqueued, after the accumulator's checks: PTRWM_E_STRUCT for a wrong flow->struct_size;
 * PTRWM_E_NULL for a NULL walker; PTRWM_E_ARG for n_temps < 2, reserved != 0, or flow regions that do not fit the kernel's LDS
 * together with the moments regions (above). */
int32_t ptrwm_run_with_diagnostics(const ptrwm_target_desc *target, const ptrwm_proposal_desc *proposal,
                                   const ptrwm_run_args *args, const ptrwm_moments_args *moments,
                                   const ptrwm_chain_moments_args *chain_moments, const ptrwm_flow_args *flow, void *stream);

/* ptrwm_swap_sweep (below), and the flow update of that event.  flow == NULL: exactly ptrwm_swap_sweep.  The flow checks
 * (as above; no LDS limit) come after ptrwm_swap_sweep's own argument checks and before its empty-batch return. */
int32_t ptrwm_swap_sweep_with_flow(const ptrwm_run_args *args, int32_t dim, int64_t event_index, int32_t rng_stream,
                                   const ptrwm_flow_args *flow, void *stream);

/* ptrwm_split_accept (below), and the flow update of the step's swap event, inside the swap kernel it enqueues: in
 * device-step mode the call can sit in a captured block; a step without an event (the kernel returns at once, or is not
 * enqueued: PTRWM_SPLIT_NO_SWEEP) leaves flow untouched.  flow == NULL: exactly ptrwm_split_accept. */
int32_t ptrwm_split_accept_with_flow(const ptrwm_run_args *args, int32_t dim, float *proposals, const float *accept_u,
                                     const float *logp_proposed, const ptrwm_flow_args *flow, void *stream);

/* ---- pooled marginal histograms: mode weights and quantiles without a trace -------------------------------------------------
 * Mean and variance cannot tell a population stuck in one mode from one that splits its mass over three.  A histogram
 * accumulator covers the first `temps` temperatures.  For each such temperature t, every coordinate d and every local chain, at
 * every step whose step_counter > burn_in and step_counter % every == 0:
 *   counts[t, d, bin(x_d)] += 1,   count[t] += 1
 * where x is the replica's state after the whole step (MH move and that step's swap event) - the values a trace with
 * trace_every = every records at that step.  The bin rule (csrc/hist.h), with n_bins equal bins over [lo[d], hi[d]) and the
 * caller's scale[d] = n_bins / (hi[d] - lo[d]) as a float:
 *   u = (x_d - lo[d]) * scale[d]      in float, each operation rounded on its own (a double state is rounded to float first)
 *   bin = 0            if !(u >= 0)   underflow; a NaN coordinate lands HERE too
 *   bin = n_bins + 1   if u >= n_bins overflow, +inf included
 *   bin = 1 + (int)u   otherwise
 * Everything is integer and only ever added to (+=): results are exact, do not depend on the order of the additions, and
 * launches, calls and shards compose.  ptrwm_swap_sweep events are not steps and add nothing.
 * How: NOT in the step kernels.  A small stand-alone snapshot kernel reads `state` between launches: ptrwm_run_with_histogram
 * ends a launch at every due step and enqueues the snapshot kernel behind it on the same stream.  A workgroup takes a tile of
 * chains and a group of the temps * dim columns (csrc/hist.h hist_geometry states the sizes); it counts in 32-bit LDS counters
 * and flushes each non-zero counter with one 64-bit atomic.  Where too few columns of counters would fit the LDS - many
 * bins - the kernel adds to `counts` with global atomics directly.  The accumulators must be ordinary device memory of the
 * current device. */
#define PTRWM_HIST_MAX_BINS 1024
typedef struct ptrwm_hist_args {
  uint32_t struct_size; /* sizeof(ptrwm_hist_args) */
  int32_t temps;        /* 1..n_temps: the first `temps` temperatures */
  int32_t every;        /* >= 1: a snapshot at every step past burn-in whose step_counter is a multiple */
  int32_t n_bins;       /* 1..PTRWM_HIST_MAX_BINS */
  const float *lo;      /* device [dim] */
  const float *scale;   /* device [dim]: n_bins / (hi - lo), as float */
  int64_t *counts;      /* device [temps, dim, n_bins + 2], +=; bin 0 underflow, bin n_bins + 1 overflow */
  int64_t *count;       /* device [temps], +=, or NULL: (chain, step) pairs added per temperature */
} ptrwm_hist_args;

/* One snapshot: the state as it stands after step args->step0 (device-step mode: *device_step + step0 - read on the device,
 * so the call can sit inside a captured block of split steps, after ptrwm_split_accept); a step that is not due adds
 * nothing.  Reads from `args`: n_temps, n_chains, state, state_f64, burn_in, step0, device_step.
 * Checked, in this order, before anything is enqueued: PTRWM_E_NULL for a NULL args / hist; PTRWM_E_STRUCT for a wrong
 * struct_size of args; PTRWM_E_DIM / PTRWM_E_TEMPS as everywhere; PTRWM_E_ARG for state_f64 outside 0..1 or a negative
 * n_chains, step0 or burn_in; then the block's own checks as below; an empty batch returns PTRWM_OK; PTRWM_E_NULL for a NULL
 * state. */
int32_t ptrwm_histogram(const ptrwm_run_args *args, int32_t dim, const ptrwm_hist_args *hist, void *stream);

/* ptrwm_run_with_diagnostics, plus histograms.  hist == NULL: exactly ptrwm_run_with_diagnostics.
 * A launch of the request additionally ends at every step whose step_counter is past burn_in and a multiple of hist->every,
 * and the snapshot kernel is enqueued right after it on `stream`; a request without such a step performs exactly the launches
 * it performs without `hist`.  No step kernel is told about the histogram: a run with histograms and nothing else runs the
 * production kernel.  Everything else of the run is bit-identical with and without `hist` - state, logp, every counter,
 * moments, flow, traces - with the one exception that holds for any change of where a run is cut into launches
 * (ptrwm_run_args.sq_jump above): the sq_jump sum of a replica that crosses the trust bound in the middle of a launch can
 * differ in its last bits.  External randoms are allowed (the cuts advance ext_* by the steps done).
 * Checked before anything is enqueued, after the accumulators' and flow's checks: PTRWM_E_STRUCT for a wrong
 * hist->struct_size; PTRWM_E_ARG for temps outside 1..n_temps, every < 1 or n_bins outside 1..PTRWM_HIST_MAX_BINS;
 * PTRWM_E_NULL for a NULL lo, scale or counts.  An empty batch returns PTRWM_OK. */
int32_t ptrwm_run_with_histogram(const ptrwm_target_desc *target, const ptrwm_proposal_desc *proposal,
                                 const ptrwm_run_args *args, const ptrwm_moments_args *moments,
                                 const ptrwm_chain_moments_args *chain_moments, const ptrwm_flow_args *flow,
                                 const ptrwm_hist_args *hist, void *stream);

/* ---- warm-up tuning of the proposal scale, per temperature, on the device ------------------------------------------------------
 * temp_scale[t] = sqrt(var / beta_t) is exact for Gaussians only; elsewhere the hot rungs of a ladder sit far from the
 * acceptance rate a random-walk Metropolis kernel works best at.  During burn-in the library can tune every temperature's
 * scale towards a target acceptance rate, pooled over every replica (csrc/adapt.h states the rule once).
 * Windows: with W = every, window k is the steps [k W, (k + 1) W).  The K = until / W windows that end at or before `until`
 * (<= burn_in) adapt; steps [K W, burn_in) are ordinary burn-in under the final scale; past burn-in nothing adapts, so the
 * chain that is sampled is a fixed-kernel Markov chain.  After window k, for every temperature t:
 *   rate  = pooled[t] / pooled[n_temps]       acceptances / chain-steps of the window (pooled[n_temps] = 0: scale left alone)
 *   s_new = (float) clamp((double) s_old * exp(gain_k * (rate - target)), min_scale, max_scale),   gain_k = gain / (k + 1)^decay
 * in double (gain_k on the host).  Suggested: target 0.234, gain 3, decay 0.5.
 * How: NOT in the step kernels.  Every launch reads temp_scale from device memory when it starts, so a kernel enqueued between
 * two launches rewrites the scales in stream order.  A launch inside an adapting window ends with the window at the latest; it
 * is the production kernel, told to count acceptances from its first step into `window_accept` (which accumulates: a window
 * may span launches and calls), with no squared-jump sum and no swap step - exactly what a burn-in step does to state and
 * logp, which are bit-identical to the same steps run as ordinary burn-in under the same scales (the Philox words depend on
 * seed, step and chain only).  n_accept, sq_jump, the swap counters, moments, flow and histograms see post-burn-in steps only,
 * as always; traces and accept_flags behave as in any burn-in.  After the launch that ends window k the reduce kernel
 * (window_accept summed over chains into pooled, the scratch left zero) and, unless defer_update, the update kernel
 * (temp_scale, the histories; pooled left zero) are enqueued.  Everything between scratch and scale is integer or one
 * deterministic double expression, and the window comes from step0: a run cut into calls anywhere gives the same bits, and a
 * request at or past `until` adapts nothing.
 * Shards: with defer_update = 1 a request ends at window ends (one that would step past the end of the adapting window its
 * step0 lies in returns PTRWM_E_ARG before anything is enqueued); the caller all-reduces (SUM) `pooled` over the shards and
 * calls ptrwm_adapt_update on each: every shard applies the same update to the same integers, so a sharded run equals the
 * unsharded one bit for bit.
 * Split steps: a warm-up step is ptrwm_split_propose / ptrwm_split_accept with burn_in = 0, swap_every = INT32_MAX,
 * n_accept = window_accept and sq_jump = NULL in ptrwm_run_args; ptrwm_adapt_reduce, then ptrwm_adapt_update, after the last
 * step of every adapting window. */
typedef struct ptrwm_adapt_args {
  uint32_t struct_size;    /* sizeof(ptrwm_adapt_args) */
  int32_t every;           /* W >= 1: the window length */
  int64_t until;           /* 0..burn_in: windows that end at or before this step adapt */
  float target;            /* in (0, 1): the acceptance rate aimed at */
  float gain, decay;       /* gain_k = gain / (k + 1)^decay; gain > 0 and finite, decay in 0..1 */
  float min_scale, max_scale; /* 0 < min_scale <= max_scale, finite: every scale is clamped to this range */
  int32_t defer_update;    /* 0: update after every window.  1: the caller does (ptrwm_adapt_update), see "Shards" */
  float *temp_scale;       /* [n_temps] device, in/out; must be the memory proposal->temp_scale points to */
  int64_t *window_accept;  /* [n_chains, n_temps] device scratch, zero before the run, zero again after every window */
  int64_t *pooled;         /* [n_temps + 1] device, zero before the run */
  float *scale_history;    /* [K + 1, n_temps] device or NULL: row 0 the starting scales, row k + 1 those after window k */
  int64_t *accept_history; /* [K, n_temps] device or NULL: pooled[t] of window k */
} ptrwm_adapt_args;

/* ptrwm_run_with_histogram, plus adaptation.  adapt == NULL: exactly ptrwm_run_with_histogram.
 * Checked before anything is enqueued, after the existing checks: PTRWM_E_STRUCT for a wrong adapt->struct_size; PTRWM_E_NULL
 * for a NULL temp_scale, window_accept or pooled; PTRWM_E_ARG for every < 1, until outside 0..burn_in, target not in (0, 1),
 * gain not positive and finite, decay outside 0..1, min_scale / max_scale not 0 < min <= max and finite,
 * temp_scale != proposal->temp_scale, defer_update outside 0..1, or (defer_update = 1) a request that steps past a pending
 * window end.  External randoms are allowed, as with histograms. */
int32_t ptrwm_run_with_adaptation(const ptrwm_target_desc *target, const ptrwm_proposal_desc *proposal,
                                  const ptrwm_run_args *args, const ptrwm_moments_args *moments,
                                  const ptrwm_chain_moments_args *chain_moments, const ptrwm_flow_args *flow,
                                  const ptrwm_hist_args *hist, const ptrwm_adapt_args *adapt, void *stream);

/* The end of a window, stand-alone (split steps; shards): adapt->window_accept [args->n_chains, args->n_temps] summed over
 * chains into adapt->pooled[t], args->n_chains * adapt->every added to pooled[n_temps], the scratch left zero.  Reads n_temps
 * and n_chains from `args`.  PTRWM_E_NULL / PTRWM_E_STRUCT / PTRWM_E_TEMPS / PTRWM_E_ARG as above; an empty batch: PTRWM_OK. */
int32_t ptrwm_adapt_reduce(const ptrwm_run_args *args, const ptrwm_adapt_args *adapt, void *stream);
/* The update of window `window` (0 <= window < K = until / every, else PTRWM_E_ARG) from adapt->pooled: temp_scale and the
 * histories written, pooled[0 .. n_temps] left zero.  One small workgroup. */
int32_t ptrwm_adapt_update(const ptrwm_adapt_args *adapt, int32_t n_temps, int64_t window, void *stream);

/* ---- warm-up tuning of the temperature ladder, on the device ---------------------------------------------------------------------
 * The other tuning knob of parallel tempering: where the rungs sit.  During burn-in the library can move the interior betas
 * towards equal swap rates between neighbours, pooled over every replica; both ends of the ladder keep their bits
 * (csrc/ladder.h states the rule once).
 * Windows: with V = every, window j is the steps [j V, (j + 1) V).  The K = until / V windows that end at or before `until`
 * (<= burn_in) adapt; steps [K V, burn_in) are ordinary burn-in under the final ladder; past burn-in nothing adapts.
 * Probes: step s of an adapting window is a probe step when (s + 1) % probe_every == 0 (probe_every divides every, so a
 * window's last step is one).  Burn-in has no swap events and none is added: behind a probe step a small kernel reads logp
 * and beta and adds, for every chain c and pair t = 0 .. n_temps - 2,
 *   q = llrint(thr * 2^24),  thr = min(1, exp(lp)) exactly as the swap test forms it (a NaN: q = 0),
 *   lp = beta[t] logp[c,t+1] + beta[t+1] logp[c,t] - beta[t] logp[c,t] - beta[t+1] logp[c,t+1]   (float, left to right)
 * to pooled[t], and 1 per chain to pooled[n_temps - 1].  It moves nothing.  Integer sums: exact, whatever the order.
 * Update, after window j, one thread, in double, sums over t ascending (pooled[n_temps - 1] = 0: the ladder is left alone):
 *   r_t = pooled[t] / (pooled[n_temps - 1] 2^24),  rbar = mean r,  g_t = log beta_t - log beta_{t+1},  G = sum g,
 *   h_t = log g_t + gain_j (r_t - rbar),  gain_j = gain / (j + 1)^decay (on the host),  w_t = exp(h_t - max h),  S = sum w,
 *   beta[t + 1] = (float) ((double) beta_0 exp(-G (w_0 + ... + w_t) / S))        t = 0 .. n_temps - 3
 * A new ladder that is not strictly decreasing after the rounding to float is dropped whole: the ladder is kept and
 * *skipped += 1.  With rescale_scales = 1 the interior proposal scales follow, temp_scale[t] *= sqrt(beta_old[t] / beta_new[t])
 * (in double, rounded once).  Suggested: gain 2, decay 0.5.
 * How: NOT in the step kernels.  Every launch reads beta and temp_scale from device memory when it starts.  A launch that
 * starts in an adapting window ends behind the next probe step at the latest; it is the ordinary burn-in launch, told
 * nothing, so state and logp are bit-identical to the same steps run as plain burn-in under the same ladder and scales.
 * The probe kernel follows it on the same stream and, at a window's end and unless defer_update, the update kernel (beta,
 * temp_scale, the histories; pooled left zero).  Where a window of ptrwm_adapt_args ends at the same step the order is: scale
 * reduce, scale update, ladder probe, ladder update.  Windows and probes come from step0: a run cut into calls anywhere
 * gives the same bits, and a request at or past `until` adapts nothing.
 * Shards: with defer_update = 1 a request ends at window ends (one that would step past the end of the adapting window its
 * step0 lies in returns PTRWM_E_ARG before anything is enqueued); the caller all-reduces (SUM) `pooled` over the shards and
 * calls ptrwm_ladder_update on each.
 * Split steps: ordinary burn-in split steps; ptrwm_ladder_probe behind every probe step, ptrwm_ladder_update behind the last
 * step of every adapting window.
 * The library cannot read device memory before it enqueues: that beta is positive and strictly decreasing is the caller's
 * to check. */
typedef struct ptrwm_ladder_args {
  uint32_t struct_size;    /* sizeof(ptrwm_ladder_args) */
  int32_t every;           /* V >= 1: the window length */
  int32_t probe_every;     /* >= 1 and a divisor of every: a probe behind every step s with (s + 1) % probe_every == 0 */
  int64_t until;           /* 0..burn_in: windows that end at or before this step adapt */
  float gain, decay;       /* gain_j = gain / (j + 1)^decay; gain > 0 and finite, decay in 0..1 */
  int32_t rescale_scales;  /* 0: temp_scale is left alone.  1: interior scales follow their beta */
  int32_t defer_update;   /* 0: update after every window.  1: the caller does (ptrwm_ladder_update), see "Shards" */
  float *beta;             /* [n_temps] device, in/out; must be the memory args->beta points to */
  float *temp_scale;       /* [n_temps] device, in/out; must be the memory proposal->temp_scale points to; NULL allowed with
                              rescale_scales = 0 only */
  int64_t *pooled;         /* [n_temps] device, zero before the run */
  float *beta_history;     /* [K + 1, n_temps] device or NULL: row 0 the starting ladder, row j + 1 the one after window j */
  int64_t *rate_history;   /* [K, n_temps] device or NULL: the pooled row of window j */
  int64_t *skipped;        /* [1] device or NULL: updates dropped because the rounded ladder was not strictly decreasing */
} ptrwm_ladder_args;

/* ptrwm_run_with_adaptation, plus the ladder.  ladder == NULL: exactly ptrwm_run_with_adaptation.
 * Checked before anything is enqueued, after the existing checks: PTRWM_E_STRUCT for a wrong ladder->struct_size;
 * PTRWM_E_NULL for a NULL beta or pooled, or a NULL temp_scale with rescale_scales = 1; PTRWM_E_ARG for n_temps < 3,
 * every < 1, probe_every < 1 or not a divisor of every, until outside 0..burn_in, gain not positive and finite, decay outside
 * 0..1, rescale_scales or defer_update outside 0..1, beta != args->beta, a non-NULL temp_scale != proposal->temp_scale, or
 * (defer_update = 1) a request that steps past a pending window end. */
int32_t ptrwm_run_with_ladder(const ptrwm_target_desc *target, const ptrwm_proposal_desc *proposal,
                              const ptrwm_run_args *args, const ptrwm_moments_args *moments,
                              const ptrwm_chain_moments_args *chain_moments, const ptrwm_flow_args *flow,
                              const ptrwm_hist_args *hist, const ptrwm_adapt_args *adapt, const ptrwm_ladder_args *ladder,
                              void *stream);

/* One probe, stand-alone (split steps; shards): reads args->logp [args->n_chains, args->n_temps] and ladder->beta, adds to
 * ladder->pooled.  PTRWM_E_NULL / PTRWM_E_STRUCT / PTRWM_E_TEMPS / PTRWM_E_ARG as above (ladder->beta must equal args->beta);
 * an empty batch: PTRWM_OK. */
int32_t ptrwm_ladder_probe(const ptrwm_run_args *args, const ptrwm_ladder_args *ladder, void *stream);
/* The update of window `window` (0 <= window < K = until / every, else PTRWM_E_ARG) from ladder->pooled: beta, temp_scale and
 * the histories written, pooled left zero.  One small workgroup. */
int32_t ptrwm_ladder_update(const ptrwm_ladder_args *ladder, int32_t n_temps, int64_t window, void *stream);

/* ---- pooled lagged autocovariance: autocorrelation time and effective sample size without a trace --------------------------------
 * How correlated are successive draws?  An autocovariance accumulator covers the first `temps` temperatures.  A snapshot is
 * due at every step whose step_counter > burn_in and step_counter % every == 0 (the histograms' rule); its 0-based number is
 * j = step_counter / every - burn_in / every - 1, from the step counter alone.  ring [max_lag, n_chains, temps * dim], of the
 * state's own type (float; double with state_f64), keeps the last max_lag snapshots: snapshot j lives in slot j % max_lag.  At
 * snapshot j, for every covered temperature t, coordinate d and lag k = 0 .. min(j, max_lag), summed over the local chains:
 *   sxy[t, k, d]  += x_j[t, d] * x_{j-k}[t, d]      head[t, k, d] += x_j[t, d]      tail[t, k, d] += x_{j-k}[t, d]
 *   pairs[k]      += n_chains
 * where x is the replica's state after the whole step (MH move and that step's swap event) - the values a trace with
 * trace_every = every records.  Each product is one double product of the two values converted to double, rounded once and
 * not fused with the sum: a replay reproduces every term bit for bit and only the order of the additions is free (tile sums
 * are flushed with fp64 atomics, as the pooled moments are).  On the host:
 *   c_k = sxy_k / pairs_k - (head_k / pairs_k)(tail_k / pairs_k),   rho_k = c_k / c_0.
 * The rule is csrc/acf.h's.  Everything is added to (+=): launches, calls and shards compose (sum the shards' sums).
 * ptrwm_swap_sweep events are not steps and add nothing.  The ring needs no zeroing: a slot is written before it is read.
 * Contract: EVERY due step is snapshotted, in order - a skipped one leaves a stale slot that later snapshots pair with.
 * ptrwm_run_with_autocorr guarantees it; a stand-alone caller of ptrwm_autocorr is responsible for it.
 * How: NOT in the step kernels.  A small stand-alone snapshot kernel reads `state` between launches, as the histograms' does:
 * a workgroup takes a tile of chains and a group of the temps * dim columns (csrc/acf.h acf_geometry), keeps its x_j in
 * registers, streams the ring slots of the available lags past it, and flushes one fp64 atomic per non-zero tile sum.  It
 * reads (min(j, max_lag) + 1) * n_chains * temps * dim elements and writes one slot.  The accumulators and the ring must be
 * ordinary device memory of the current device. */
#define PTRWM_ACF_MAX_LAG 1024
typedef struct ptrwm_acf_args {
  uint32_t struct_size; /* sizeof(ptrwm_acf_args) */
  int32_t temps;        /* 1..n_temps: the first `temps` temperatures */
  int32_t every;        /* >= 1: a snapshot at every step past burn-in whose step_counter is a multiple */
  int32_t max_lag;      /* 1..PTRWM_ACF_MAX_LAG: lags 0..max_lag, in snapshots */
  void *ring;           /* device [max_lag, n_chains, temps * dim], float or double as the state; scratch */
  double *sxy;          /* device [temps, max_lag + 1, dim], += */
  double *head;         /* device [temps, max_lag + 1, dim], += */
  double *tail;         /* device [temps, max_lag + 1, dim], += */
  int64_t *pairs;       /* device [max_lag + 1], += */
} ptrwm_acf_args;

/* One snapshot: the state as it stands after step args->step0 (device-step mode: *device_step + step0 - read on the device,
 * so the call can sit inside a captured block of split steps, after ptrwm_split_accept); a step that is not due adds
 * nothing.  Reads from `args`: n_temps, n_chains, state, state_f64, burn_in, step0, device_step.
 * Checked, in this order, before anything is enqueued: PTRWM_E_NULL for a NULL args / acf; PTRWM_E_STRUCT for a wrong
 * struct_size of args; PTRWM_E_DIM / PTRWM_E_TEMPS as everywhere; PTRWM_E_ARG for state_f64 outside 0..1 or a negative
 * n_chains, step0 or burn_in; then the block's own checks as below; an empty batch returns PTRWM_OK; PTRWM_E_NULL for a NULL
 * state. */
int32_t ptrwm_autocorr(const ptrwm_run_args *args, int32_t dim, const ptrwm_acf_args *acf, void *stream);

/* ptrwm_run_with_ladder, plus the autocovariance.  acf == NULL: exactly ptrwm_run_with_ladder.
 * A launch of the request additionally ends at every step whose step_counter is past burn_in and a multiple of acf->every,
 * and the snapshot kernel is enqueued right after it on `stream` (behind the histogram's, where both are due); a request
 * without such a step performs exactly the launches it performs without `acf`.  No step kernel is told about it, and
 * everything else of the run is bit-identical with and without `acf`, with the one exception that holds for any change of
 * where a run is cut into launches (ptrwm_run_args.sq_jump above).
 * Checked before anything is enqueued, after every other block's checks: PTRWM_E_STRUCT for a wrong acf->struct_size;
 * PTRWM_E_ARG for temps outside 1..n_temps, every < 1 or max_lag outside 1..PTRWM_ACF_MAX_LAG; PTRWM_E_NULL for a NULL ring,
 * sxy, head, tail or pairs.  An empty batch returns PTRWM_OK. */
int32_t ptrwm_run_with_autocorr(const ptrwm_target_desc *target, const ptrwm_proposal_desc *proposal,
                                const ptrwm_run_args *args, const ptrwm_moments_args *moments,
                                const ptrwm_chain_moments_args *chain_moments, const ptrwm_flow_args *flow,
                                const ptrwm_hist_args *hist, const ptrwm_adapt_args *adapt, const ptrwm_ladder_args *ladder,
                                const ptrwm_acf_args *acf, void *stream);

/* ---- pooled posterior covariance: how coordinates move together, without a trace --------------------------------------------------
 * A covariance accumulator covers the first `temps` temperatures.  A snapshot is due at every step whose step_counter > burn_in
 * and step_counter % every == 0 (the histograms' and the autocovariance's rule).  At a due step, for every covered
 * temperature t, summed over the local chains:
 *   sxx[t, i, j] += x[t, i] * x[t, j]   for j <= i < dim      sx[t, i] += x[t, i]      count += n_chains
 * where x is the replica's state after the whole step (MH move and that step's swap event) - the values a trace with
 * trace_every = every records.  Only the lower triangle of sxx (j <= i, diagonal included) is ever written; the strict upper
 * triangle stays as the caller left it.  One term is both values converted to double and multiplied: exact for float states;
 * for state_f64 states the product may be fused into the running sum.  Only the order of the additions is free (tile sums are
 * flushed with fp64 atomics, as the pooled moments are).  On the host, with n = count:
 *   cov[i, j] = sxx[i, j] / n - (sx[i] / n)(sx[j] / n),   mirrored to both triangles.
 * These are raw sums: fp64 loses about log10(1 + mean^2 / var) digits per coordinate, as the moments' sum_sq does.
 * The rule is csrc/cov.h's.  Everything is added to (+=): launches, calls and shards compose (sum the shards' sums).
 * ptrwm_swap_sweep events are not steps and add nothing.
 * How: NOT in the step kernels.  A small stand-alone snapshot kernel reads `state` between launches, as the histograms' does:
 * a workgroup takes one covered temperature and a tile of chains, stages their rows through LDS as doubles, accumulates the
 * lower-triangle 16 x 16 blocks of the Gram matrix with the fp64 matrix instruction (K runs over chains) and flushes one fp64
 * atomic per non-zero element.  It reads n_chains * temps * dim elements.  The accumulators must be ordinary device memory of
 * the current device. */
typedef struct ptrwm_cov_args {
  uint32_t struct_size; /* sizeof(ptrwm_cov_args) */
  int32_t temps;        /* 1..n_temps: the first `temps` temperatures */
  int32_t every;        /* >= 1: a snapshot at every step past burn-in whose step_counter is a multiple */
  double *sxx;          /* device [temps, dim, dim], += on j <= i */
  double *sx;           /* device [temps, dim], += */
  int64_t *count;       /* device [1], += */
} ptrwm_cov_args;

/* One snapshot: the state as it stands after step args->step0 (device-step mode: *device_step + step0 - read on the device,
 * so the call can sit inside a captured block of split steps, after ptrwm_split_accept); a step that is not due adds
 * nothing.  Reads from `args`: n_temps, n_chains, state, state_f64, burn_in, step0, device_step.
 * Checked, in this order, before anything is enqueued: PTRWM_E_NULL for a NULL args / cov; PTRWM_E_STRUCT for a wrong
 * struct_size of args; PTRWM_E_DIM / PTRWM_E_TEMPS as everywhere; PTRWM_E_ARG for state_f64 outside 0..1 or a negative
 * n_chains, step0 or burn_in; then the block's own checks as below; an empty batch returns PTRWM_OK; PTRWM_E_NULL for a NULL
 * state. */
int32_t ptrwm_covariance(const ptrwm_run_args *args, int32_t dim, const ptrwm_cov_args *cov, void *stream);

/* ptrwm_run_with_autocorr, plus the covariance.  cov == NULL: exactly ptrwm_run_with_autocorr.
 * A launch of the request additionally ends at every step whose step_counter is past burn_in and a multiple of cov->every,
 * and the snapshot kernel is enqueued right after it on `stream` (behind the histogram's and the autocovariance's, where
 * those are due at the same step); a request without such a step performs exactly the launches it performs without `cov`.
 * No step kernel is told about it, and everything else of the run is bit-identical with and without `cov`, with the one
 * exception that holds for any change of where a run is cut into launches (ptrwm_run_args.sq_jump above).
 * Checked before anything is enqueued, after every other block's checks: PTRWM_E_STRUCT for a wrong cov->struct_size;
 * PTRWM_E_ARG for temps outside 1..n_temps or every < 1; PTRWM_E_NULL for a NULL sxx, sx or count.  An empty batch returns
 * PTRWM_OK. */
int32_t ptrwm_run_with_covariance(const ptrwm_target_desc *target, const ptrwm_proposal_desc *proposal,
                                  const ptrwm_run_args *args, const ptrwm_moments_args *moments,
                                  const ptrwm_chain_moments_args *chain_moments, const ptrwm_flow_args *flow,
                                  const ptrwm_hist_args *hist, const ptrwm_adapt_args *adapt, const ptrwm_ladder_args *ladder,
                                  const ptrwm_acf_args *acf, const ptrwm_cov_args *cov, void *stream);

/* ---- pooled log-density sums along the ladder: normalising-constant ratios and the energy per rung, without a trace ------------
 * What is log Z(beta_a) / Z(beta_b), Z(beta) = integral of pi(x)^beta dx, and where does the ladder need rungs?  A snapshot is
 * due at every step whose step_counter > burn_in and step_counter % every == 0 (the histograms', the autocovariance's and the
 * covariance's rule).  At a due step, for every local chain c and temperature t, with l = logp[c, t] - the float32 log-density
 * after the whole step, swap event included - and g = (chain_offset + c) mod groups, the chain's group by its global id:
 *   l not finite:  nonfinite[0] += 1 and nothing else.
 *   otherwise, with x = (double) l and y = x - ref[t] (one double subtraction):
 *     count[g, t] += 1      s1[g, t] += x      s2[g, t] += x * x
 *     t >= 1:            colder[g, t] += exp(((double) beta[t - 1] - (double) beta[t]) * y)
 *     t <= n_temps - 2:  hotter[g, t] += exp(((double) beta[t + 1] - (double) beta[t]) * y)
 * colder[:, 0] and hotter[:, n_temps - 1] are never written; with n_temps = 1 neither array is touched.  An overflowing exp
 * leaves inf in its sum.  Only the order of the additions is free (tile sums are flushed with fp64 atomics, the counters with
 * integer atomics).
 * ref, the level the exponential sums are taken against, keeps an unnormalised log-density (one offset by -1e6, say) from
 * overflowing or underflowing.  While ref_set[0] is 0, a due snapshot first sets ref[t] to the largest finite l of temperature
 * t over the local chains at that snapshot (0 where none is finite) and ref_set[0] to 1 - a maximum, so ref is deterministic;
 * a non-zero flag leaves ref alone.  A caller may pin ref and pre-set the flag: shards that share a pinned ref have sums that
 * add directly; shards with their own ref rescale colder / hotter to a common one on the host before they add.
 * The groups are disjoint sets of independent chains - a sharded run puts every chain in the group the unsharded run does -
 * and the delete-one-group jackknife over them gives error bars that hold whatever the chains' autocorrelation in time.
 * On the host, with n[t] = sum_g count[g, t] and the sums added over g, for t = 1 .. n_temps - 1:
 *   forward[t] =   log(colder[t] / n[t])         + (beta[t-1] - beta[t]) ref[t]
 *   reverse[t] = -(log(hotter[t-1] / n[t-1])     + (beta[t] - beta[t-1]) ref[t-1])
 * both estimate log Z(beta[t-1]) / Z(beta[t]) (stepping stones; E forward <= truth <= E reverse), and s1 / n, s2 / n give the
 * mean and variance of l per rung: thermodynamic integration, and the heat capacity beta^2 Var(l).
 * The rule is csrc/energy.h's.  Everything is added to (+=): launches, calls and shards compose.  ptrwm_swap_sweep events are
 * not steps and add nothing.  beta is read at the snapshot: after a ladder tuning it is the final ladder (past burn-in nothing
 * adapts).  The accumulators must be ordinary device memory of the current device.
 * How: NOT in the step kernels.  Two small kernels read logp between launches: one workgroup that sets ref (it returns at once
 * where the flag is set), and the accumulating kernel - a workgroup serves chains of one group, lanes run along the rows of
 * logp, partial sums per temperature sit in LDS and are flushed once per workgroup.  It reads n_chains * n_temps floats. */
#define PTRWM_ENERGY_MAX_GROUPS 64
typedef struct ptrwm_energy_args {
  uint32_t struct_size; /* sizeof(ptrwm_energy_args) */
  int32_t groups;       /* 1..PTRWM_ENERGY_MAX_GROUPS */
  int32_t every;        /* >= 1: a snapshot at every step past burn-in whose step_counter is a multiple */
  double *ref;          /* device [n_temps]; written once while *ref_set == 0, else only read */
  int32_t *ref_set;     /* device [1]; 0: the next due snapshot sets ref and this flag */
  int64_t *count;       /* device [groups, n_temps], += */
  int64_t *nonfinite;   /* device [1], +=; may be NULL */
  double *s1;           /* device [groups, n_temps], += */
  double *s2;           /* device [groups, n_temps], += */
  double *colder;       /* device [groups, n_temps], += on t >= 1; may be NULL with n_temps = 1 */
  double *hotter;       /* device [groups, n_temps], += on t <= n_temps - 2; may be NULL with n_temps = 1 */
} ptrwm_energy_args;

/* One snapshot: logp as it stands after step args->step0 (device-step mode: *device_step + step0 - read on the device, as is
 * ref_set, so the call can sit inside a captured block of split steps, after ptrwm_split_accept); a step that is not due adds
 * nothing.  Reads from `args`: n_temps, n_chains, chain_offset, logp, beta, burn_in, step0, device_step.
 * Checked, in this order, before anything is enqueued: PTRWM_E_NULL for a NULL args / energy; PTRWM_E_STRUCT for a wrong
 * struct_size of args; PTRWM_E_TEMPS as everywhere; PTRWM_E_ARG for a negative n_chains, step0 or burn_in; then
 * the block's own checks as below; an empty batch returns PTRWM_OK; PTRWM_E_NULL for a NULL logp or beta. */
int32_t ptrwm_energy(const ptrwm_run_args *args, const ptrwm_energy_args *energy, void *stream);

/* ptrwm_run_with_covariance, plus the log-density sums.  energy == NULL: exactly ptrwm_run_with_covariance.
 * A launch of the request additionally ends at every step whose step_counter is past burn_in and a multiple of energy->every,
 * and the two kernels are enqueued right after it on `stream` (behind the histogram's, the autocovariance's and the
 * covariance's, where those are due at the same step); a request without such a step performs exactly the launches it performs
 * without `energy`.  No step kernel is told about it, and everything else of the run is bit-identical with and without
 * `energy`, with the one exception that holds for any change of where a run is cut into launches (ptrwm_run_args.sq_jump above).
 * Checked before anything is enqueued, after every other block's checks: PTRWM_E_STRUCT for a wrong energy->struct_size;
 * PTRWM_E_ARG for groups outside 1..PTRWM_ENERGY_MAX_GROUPS or every < 1; PTRWM_E_NULL for a NULL ref, ref_set, count, s1 or
 * s2, and for a NULL colder or hotter with n_temps >= 2 (nonfinite may be NULL).  An empty batch returns PTRWM_OK. */
int32_t ptrwm_run_with_energy(const ptrwm_target_desc *target, const ptrwm_proposal_desc *proposal,
                              const ptrwm_run_args *args, const ptrwm_moments_args *moments,
                              const ptrwm_chain_moments_args *chain_moments, const ptrwm_flow_args *flow,
                              const ptrwm_hist_args *hist, const ptrwm_adapt_args *adapt, const ptrwm_ladder_args *ladder,
                              const ptrwm_acf_args *acf, const ptrwm_cov_args *cov, const ptrwm_energy_args *energy,
                              void *stream);

/* One stand-alone swap event over the current states: what the reference's
 * ParallelTemperingRWM_GPU_Optimized._attempt_all_swaps() does when called on its own
 * (pt_rwm_gpu_optimized.py:594-633; tests/debug_pt_performance.py:156).  Exactly the swap part of a ptrwm_run step:
 * same decision rule, modes and orders.  Reads from `args`: n_temps, n_chains, chain_offset, state, logp, beta,
 * swap_accept, last_swap_ordinal (both may be NULL), swap_mode, swap_order, seed, ext_swap_u (device
 * [n_chains, n_temps-1] or NULL), and step0 = the Philox step index the swap uniforms are drawn at.
 * `event_index` = 0-based number of this event in the run (attempt ordinals, even/odd parity); `rng_stream` in
 * 1..15 selects the Philox stream (1 = the stream ptrwm_run's own swap events use, so a sweep with step0 = s,
 * rng_stream = 1 reproduces the swap ptrwm_run would perform at step s).  sq_jump is not touched. */
int32_t ptrwm_swap_sweep(const ptrwm_run_args *args, int32_t dim, int64_t event_index, int32_t rng_stream,
                         void *stream);

/* Split step, for target densities the library has no kernel for (a user-defined
 * TorchTargetDistribution.log_density: SURVEY 8b "anything unrecognised"; the reference calls target.log_density on
 * the proposals inside step(), pt_rwm_gpu_optimized.py:551, rwm_gpu_optimized.py:289-336).  One step = three calls:
 *   1. ptrwm_split_propose: for step args->step0, proposals[c,t,:] = state[c,t,:] + increment and
 *      accept_u[c,t] = the step's accept uniform - the same Philox words (or ext_prop [n_chains, n_temps, raw] /
 *      ext_u [n_chains, n_temps] of THIS step) and the same arithmetic as ptrwm_run;
 *   2. the caller evaluates logp_proposed[c,t] = log_density(proposals[c,t,:]) on the device, any way it likes;
 *   3. ptrwm_split_accept: Metropolis rule, state / logp / statistics update and, when this step's step_counter is a
 *      swap step, the swap event (ext_swap_u [n_chains, n_temps-1] of THIS event in external-randoms mode) - exactly
 *      what ptrwm_run does for the step.  Reads from `args`: everything ptrwm_run reads except n_steps and the
 *      trace fields (accept_flags, if set, is [n_chains, n_temps] for this step).
 * `proposals` [n_chains, n_temps, dim] and `accept_u` [2, n_chains, n_temps] are device scratch owned by the caller
 * (accept_u plane 0: the accept uniforms; plane 1: the squared length of the increment as the fused kernel counts it -
 * the Philox paths of the Normal and UniformRadius proposals know it without a pass over the dimensions - or -1);
 * after ptrwm_split_accept of a SWAP step `proposals` holds the states from before the step (the swap kernel reads them);
 * after any other step its contents are unspecified.  Driven with ptrwm_logdensity as the
 * density, a split step reproduces ptrwm_run bit for bit (tests/test_gpu_engine_parity.py) - state, log-densities and
 * counters always; sq_jump as ptrwm_run called one step at a time does: the split step takes the trust verdict of
 * ptrwm_run_args.sq_jump's comment from the state every step, ptrwm_run once per launch, so the two differ (within that
 * comment's ~3e-5) only for a replica that crosses the bound in the middle of a longer launch. */
int32_t ptrwm_split_propose(const ptrwm_proposal_desc *proposal, const ptrwm_run_args *args, int32_t dim,
                            float *proposals, float *accept_u, void *stream);
int32_t ptrwm_split_accept(const ptrwm_run_args *args, int32_t dim, float *proposals, const float *accept_u,
                           const float *logp_proposed, void *stream);
/* *args->device_step += max(1, args->n_steps) on `stream` (one thread): the last node of a block of split steps in
 * device-step mode. */
int32_t ptrwm_split_advance(const ptrwm_run_args *args, void *stream);

/* ---- preconditioned Gaussian proposals: increments s_t L z, and the factor learned during burn-in ---------------------
 * Every Normal proposal above is x + s_t z with one scalar per temperature: its efficiency is set by the conditioning of the
 * posterior covariance (ptrwm_cov_args measures it).  ptrwm_split_propose_precond is ptrwm_split_propose for
 * PTRWM_PROPOSAL_NORMAL with a lower-triangular factor L, L L^T ~ the posterior covariance, shared by all temperatures:
 *   inc_i = acc after  acc = +0;  acc = fmaf(L[i][k], z[k], acc)  for k = 0, 1, ..., 16 (i / 16 + 1) - 1 ascending
 *   y_i   = fmaf(s_t, inc_i, x_i)                                           s_t = proposal->temp_scale[t]
 * with L[i][k] taken as zero for k > i and z[k] as zero for k >= dim (csrc/precond.h states the rule and the kernel's index
 * maps).  `chol` is float [dim, dim], row-major; only its entries k <= i are ever read.  z is the Box-Muller normals of the
 * step's Philox blocks at unit scale - the words, counter layout and stream of the Normal proposal; the accept uniform is
 * word 2 ceil(dim / 2), as there - or ext_prop (dim raw values per row) with ext_u as the accept uniform.  Plane 1 of accept_u
 * is -1: ptrwm_split_accept takes the squared jump from the states.  The same fields of `args` are read as by
 * ptrwm_split_propose, device-step mode included, and the same scratch contract holds: ptrwm_split_accept, the sweep and the
 * moments / histogram / autocovariance / covariance snapshots follow it unchanged.  It is a split-step proposal only: the fused
 * step kernels know nothing of it.
 * How: one run-time-dim kernel.  A 256-thread workgroup stages L into LDS once and walks tiles of 64 rows; the product
 * Z [rows, dim] L^T is taken on the f32 matrix unit (v_mfma_f32_16x16x4_f32, whose result is the k-ordered fmaf chain above).
 * Checked, in this order, before anything is enqueued: PTRWM_E_NULL for a NULL proposal or precond; the checks of
 * ptrwm_split_propose on args and dim (PTRWM_E_ARG for state_f64); PTRWM_E_KIND for any proposal kind but
 * PTRWM_PROPOSAL_NORMAL; PTRWM_E_STRUCT for a wrong precond->struct_size; an empty batch returns PTRWM_OK; PTRWM_E_NULL for a
 * NULL state, proposals, accept_u, temp_scale or chol, and for ext_prop without ext_u. */
typedef struct ptrwm_precond_args {
  uint32_t struct_size; /* sizeof(ptrwm_precond_args) */
  uint32_t reserved;    /* 0 */
  const float *chol;    /* device [dim, dim]: the factor, entries k <= i read */
} ptrwm_precond_args;
int32_t ptrwm_split_propose_precond(const ptrwm_proposal_desc *proposal, const ptrwm_run_args *args, int32_t dim,
                                    const ptrwm_precond_args *precond, float *proposals, float *accept_u, void *stream);

/* The factor learned from one warm-up window.  The window's sums are ptrwm_covariance's of ONE temperature (sxx lower
 * triangle, sx, count - its layout with temps = 1), gathered by the caller at the probe steps of the window.  With the running
 * triple (run_xx, run_x, run_w), all double, every operation rounded on its own:
 *   run_xx = memory run_xx + sxx,   run_x = memory run_x + sx,   run_w = memory run_w + count;   the window sums are zeroed
 *   run_w < min_count: skip
 *   m = run_x / run_w,   A = run_xx / run_w - m m^T,   A += jitter (tr A / dim) I
 *   C = the left-looking column Cholesky factor of A, inner products over k ascending; a pivot that is not finite or not > 0,
 *       or an entry that does not fit a float: skip
 * On success chol[i][j] = (float) C[i][j] for j <= i (the strict upper triangle of chol is not touched).  On a skip chol keeps
 * its bits and *skipped += 1; the running triple keeps what the window added either way.  Row 0 of chol_history is written by
 * window 0 (the factor that window ran with), row window + 1 by every window (the factor in force behind it; zeros above the
 * diagonal); weight_history[window] = run_w.  memory = 1 is the all-history estimate of Haario et al. (2001).
 * The sums come from fp64 atomics, so the factor is reproducible up to the order of those additions - unlike the integer
 * tunings above, not bit for bit across launch cuts or shards.  Shards: all-reduce (SUM) sxx, sx and count before the call.
 * One workgroup; enqueues only: neither allocates nor synchronises.
 * Checked, in this order, before anything is enqueued: PTRWM_E_NULL for NULL args; PTRWM_E_STRUCT for a wrong struct_size;
 * PTRWM_E_DIM; PTRWM_E_ARG for memory not in (0, 1], jitter not finite or < 0, min_count not >= 1, windows < 1 or a window
 * outside 0..windows - 1; PTRWM_E_NULL for a NULL chol, sxx, sx, count, run_xx, run_x or run_w. */
typedef struct ptrwm_precond_update_args {
  uint32_t struct_size;   /* sizeof(ptrwm_precond_update_args) */
  uint32_t reserved;      /* 0 */
  float *chol;            /* device [dim, dim], in/out (entries j <= i) */
  double *sxx;            /* device [dim, dim]: the window's sums, zeroed */
  double *sx;             /* device [dim], zeroed */
  int64_t *count;         /* device [1], zeroed */
  double *run_xx;         /* device [dim, dim], in/out (entries j <= i) */
  double *run_x;          /* device [dim], in/out */
  double *run_w;          /* device [1], in/out */
  double memory;          /* in (0, 1] */
  double jitter;          /* >= 0, relative to the mean variance */
  double min_count;       /* >= 1 */
  int64_t windows;        /* K >= 1: the histories have rows for windows 0 .. K - 1 */
  float *chol_history;    /* device [K + 1, dim, dim] or NULL */
  double *weight_history; /* device [K] or NULL */
  int64_t *skipped;       /* device [1] or NULL, += 1 per skipped update */
} ptrwm_precond_update_args;
int32_t ptrwm_precond_update(const ptrwm_precond_update_args *update, int32_t dim, int64_t window, void *stream);

/* ---- starting points: over-dispersed starts for multi-chain runs ----------------------------------------------------
 * Writes rows of `state` before step 0: each coordinate drawn uniformly from the box [lo[d], hi[d]], or copied from
 * `fallback`.  R-hat over many chains (ptrwm_chain_moments_args) says something about mixing between modes only when the
 * chains start over-dispersed; the draw lives here, keyed like every other random of a run by `seed` and the GLOBAL chain id
 * chain_offset + c, so the starts - and with them the whole run - do not depend on how chains are sharded over devices.
 *
 * The draw.  For row (c, t) and coordinate d, with g = chain_offset + c and tt = per_temperature ? t : 0: one
 * Philox4x32-10 block per four coordinates,
 *   counter  c0 = (d / 4) | attempt << 16
 *            c1 = 0
 *            c2 = low 32 bits of g
 *            c3 = tt | 3 << 8 | (g >> 32) << 12
 *   key      (seed low, seed high)
 * - stream 3 of the layout ptrwm_run uses (0: Metropolis moves, 1: swaps, 2: stand-alone sweeps) - and
 *   u = (word d % 4 of the block >> 8) * 2^-24                    in [0, 1): the lattice of torch.rand(float32)
 *   x = lo[d] + (hi[d] - lo[d]) * u                                in float, every operation rounded on its own (no fma)
 * With state_f64 the stored value is that float, widened.  (x <= hi[d] up to the rounding of hi - lo and of the sum: a bound
 * that is not a short binary fraction can be exceeded by one unit in the last place.)
 *
 * Redraw.  attempt = 0 writes every row.  attempt = a > 0 rewrites ONLY the rows whose args->logp[c, t] is not finite (NaN,
 * +inf or -inf) - starts outside the support of the target - drawing with attempt number a; every other row keeps its
 * bits.  The caller evaluates the density between attempts; a last call with `fallback` puts the rows still outside on
 * a point known to be inside.
 *
 * Reads from `args`: n_temps, n_chains, chain_offset, state, seed, state_f64, and logp when attempt > 0.  Enqueues one small
 * kernel (one wavefront per 64 rows); neither allocates nor synchronises.
 * Checked, in this order, before anything is enqueued: PTRWM_E_NULL for a NULL args / init; PTRWM_E_STRUCT for a wrong
 * struct_size of either; PTRWM_E_DIM / PTRWM_E_TEMPS as everywhere; PTRWM_E_ARG for attempt outside 0..65535,
 * per_temperature or state_f64 outside 0..1 or a negative n_chains; an empty batch (n_chains = 0) returns PTRWM_OK; then
 * PTRWM_E_NULL for a NULL state, lo or hi, and for a NULL logp with attempt > 0. */
typedef struct ptrwm_init_args {
  uint32_t struct_size;     /* sizeof(ptrwm_init_args) */
  int32_t per_temperature;  /* 0: the temperatures of a ladder share the chain's draw; 1: every (chain, t) draws its own */
  int32_t attempt;          /* 0: write every row.  a > 0: rewrite ONLY rows whose args->logp[c,t] is not finite
                               (NaN, +inf or -inf), drawing with attempt number a; 0 <= attempt < 65536 */
  const float *lo, *hi;     /* device [dim]: the box */
  const float *fallback;    /* device [dim] or NULL.  Non-NULL: the rows this call writes get fallback[d] instead
                               of a draw (used with attempt > 0 as the last resort) */
} ptrwm_init_args;
int32_t ptrwm_init_states(const ptrwm_run_args *args, int32_t dim, const ptrwm_init_args *init, void *stream);

/* out[i] = log_density(x[i, :]) for i < n; x is device [n, dim], out device [n]. */
int32_t ptrwm_logdensity(const ptrwm_target_desc *target, const float *x, float *out, int64_t n,
                         void *stream);

/* Proposal increments only (unit parity of the three samplers):
 * out[i, t, :] for i < n.  If ext_raw != NULL it is device [n, n_temps, raw_per_step]
 * and the transform is applied to it; otherwise Philox(seed) with the same
 * counter layout as ptrwm_run at step index i, chain id 0.. */
int32_t ptrwm_propose(const ptrwm_proposal_desc *proposal, int32_t dim, int32_t n_temps, int64_t n,
                      const float *ext_raw, uint64_t seed, float *out, void *stream);

/* Raw Philox4x32-10 blocks: out[i*4 .. i*4+3] = philox(counter = (c0 + i, c1, c2, c3), key = seed).
 * out is device [n, 4] uint32.  Known-answer tested against the Random123 vectors. */
int32_t ptrwm_philox_raw(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                         int64_t n, uint32_t *out, void *stream);

/* 1 if the (target, proposal, dim) variant is compiled in, else 0. */
int32_t ptrwm_has_variant(int32_t target_kind, int32_t proposal_kind, int32_t dim);

int32_t ptrwm_abi_version(void);
const char *ptrwm_strerror(int32_t code);

#ifdef __cplusplus
}
#endif
#endif /* PTRWM_H */
