// C ABI of the PT-RWM engine (include/ptrwm.h): argument validation, variant
// dispatch and launch.  No allocation, no synchronisation, no retained pointers.
#include <algorithm>
#include <cmath>

#include "../../include/ptrwm.h"
#include "acf.h"
#include "adapt.h"
#include "cov.h"
#include "energy.h"
#include "ladder.h"
#include "hist.h"
#include "precond.h"
#include "schedule.h"
#include "snapshot.h"
#include "variants.h"

namespace ptrwm {

struct VariantPair {
  const TargetVariants *narrow, *wide;  // each holds null entries for the other group's widths (variants.h)
  RunLaunchFn run(int proposal, int dpi) const {
    const RunLaunchFn f = narrow->run[proposal][dpi];
    return f != nullptr ? f : wide->run[proposal][dpi];
  }
  LogpLaunchFn logp(int dpi) const {
    const LogpLaunchFn f = narrow->logp[dpi];
    return f != nullptr ? f : wide->logp[dpi];
  }
};

// ---- which form of the step kernel runs (quad.h) ------------------------------------------------------------------
// The two forms are bit-identical on the same Philox stream, so this is a speed decision only; ptrwm_set_kernel_form()
// pins it for tests and tuning.  AUTO compares a model of both forms' throughput at the launch's size
// (tools/form_fit.py, fitted to profiles/r04_form_sweep_dense.txt - both forms timed over waves per SIMD, ladder lengths
// and dims on one MI355X - and checked on a held-out sweep, profiles/r04_form_sweep_heldout.txt).  With w = wavefronts
// per SIMD the one-thread-per-replica form would launch:
//   thread form   rate = A(k) w / k, k = ceil(w): a launch lasts as long as its fullest SIMDs, so at w = 1.25 the form
//                 runs at 0.625 of its two-waves rate, not at its one-wave rate (the dips of profiles/r02_form_sweep.txt)
//   lane-split    four times the waves with a quarter of the work each: the same saw-tooth on a four times finer scale,
//                 rate = Q(kq / 4) 4 w / kq, kq = ceil(4 w), Q read off the measured curve
//   dim < 16      never lane-split (a lane would own <= 3 dims: profiles/r02_single_ladder.txt)
//   dim > 64      always: it is the only form there (the one-thread-per-replica kernel needed 340-420 VGPRs and sat in
//                 the register regime in which hipcc miscompiled it twice; see variants.h)
//   w > 4         never (the thread form is saturated; the lane-split form repeats the per-replica scalar work)
#include "form_table.inc"

static void form_lerp(const float *a, const float *b, float t, float *out, int n) {
  for (int i = 0; i < n; ++i) out[i] = a[i] + (b[i] - a[i]) * t;
}

// interpolated model parameters at (dim, n_temps): dims within the lane-width class of `dim`, ladder lengths in log2
static void form_params(int dim, int n_temps, float *thread4, float *quad) {
  // A dim with kernels of its own (dim compiled in) has its own row; every other dim runs the run-time-dim kernels: last
  // generic grid dim <= dim and first generic grid dim >= dim within dim's lane-width class
  int d0 = -1, d1 = -1;
  for (int i = 0; i < kFormND; ++i)
    if (kFormDimExact[i] && kFormDims[i] == dim) d0 = d1 = i;
  const bool own_row = d0 >= 0;
  for (int i = 0; i < kFormND && !own_row; ++i) {
    if (kFormDimExact[i] || (kFormDims[i] <= 32) != (dim <= 32)) continue;
    if (kFormDims[i] <= dim) d0 = i;
    if (kFormDims[i] >= dim && d1 < 0) d1 = i;
  }
  if (d0 < 0) d0 = d1;  // below the class's first grid dim: clamp
  if (d1 < 0) d1 = d0;  // above its last
  const float td = d0 == d1 ? 0.0f : (float)(dim - kFormDims[d0]) / (float)(kFormDims[d1] - kFormDims[d0]);
  int t0 = 0, t1 = kFormNT - 1;
  for (int i = 0; i < kFormNT; ++i) {
    if (kFormTemps[i] <= n_temps) t0 = i;
    if (kFormTemps[i] >= n_temps) { t1 = i; break; }
  }
  if (t1 < t0) t1 = t0;
  const float tt = t0 == t1 ? 0.0f
                            : (float)((__builtin_log2((double)n_temps) - __builtin_log2((double)kFormTemps[t0])) /
                                      (__builtin_log2((double)kFormTemps[t1]) - __builtin_log2((double)kFormTemps[t0])));
  float lo[kFormNW], hi[kFormNW];
  form_lerp(kFormThread[d0][t0], kFormThread[d1][t0], td, lo, 4);
  form_lerp(kFormThread[d0][t1], kFormThread[d1][t1], td, hi, 4);
  form_lerp(lo, hi, tt, thread4, 4);
  form_lerp(kFormQuad[d0][t0], kFormQuad[d1][t0], td, lo, kFormNW);
  form_lerp(kFormQuad[d0][t1], kFormQuad[d1][t1], td, hi, kFormNW);
  form_lerp(lo, hi, tt, quad, kFormNW);
}

static bool lane_split_is_faster(int dim, int n_temps, double w) {
  if (dim < 16 || w > kFormW[kFormNW - 1]) return false;
  float a[4], q[kFormNW];
  form_params(dim, n_temps, a, q);
  int k = (int)__builtin_ceil(w - 1e-9);
  if (k < 1) k = 1;
  const double thread = a[k - 1] * w / k;
  // the lane-split form: the same saw-tooth on its four times finer scale - the measured rate at the next whole number of
  // lane-split waves per SIMD, times the fill of that last wave slot
  // (ladders of more than 16 temperatures: a whole workgroup of 2-8 waves per ladder is the unit and the dispatcher spreads
  // them over the CUs: no saw-tooth of its own, the measured curve is interpolated as it is)
  double kq = 4.0 * w;
  if (n_temps <= 16) {
    kq = __builtin_ceil(4.0 * w - 1e-9);
    if (kq < 1.0) kq = 1.0;
  }
  double wu = kq / 4.0, b;
  if (wu <= kFormW[0]) {
    b = q[0];
  } else {
    if (wu > kFormW[kFormNW - 1]) wu = kFormW[kFormNW - 1];
    int i = 0;
    while (i + 2 < kFormNW && kFormW[i + 1] <= wu + 1e-9) ++i;
    b = q[i] + (q[i + 1] - q[i]) * (wu - kFormW[i]) / (kFormW[i + 1] - kFormW[i]);
  }
  return b * (4.0 * w / kq) > thread;
}

static int g_kernel_form = PTRWM_FORM_AUTO;  // read / written with __atomic builtins (ptrwm_set_kernel_form may race with a launch)
static int g_stream_mode = PTRWM_STREAM_AUTO;  // likewise (ptrwm_set_stream_mode)

// ---- short launches: the streaming form of the one-thread-per-replica kernel (kernel.h STREAM) ---------------------------
// A launch of ONE Metropolis step over a large batch - the reference's step()-at-a-time loops
// (rwm_gpu_optimized.py:456-457, pt_rwm_gpu_optimized.py:736-737), the harness's benchmark_performance - is bound by
// memory traffic, not by instruction issue: the state is read, stepped once and written back.  The classic kernel gives
// every wave ONE group: load, compute, store, exit - the phases of a wave do not overlap and a SIMD's resident waves run
// them nearly in lock-step.  The streaming form keeps as many waves as the device holds resident and lets each walk many
// groups with the next group's state already in flight (LDS-DMA) and the previous group's stores still draining.  Same
// Philox words, same arithmetic, same canonical order: bit-identical to the classic kernel
// (tests/test_gpu_engine_parity.py test_streaming_form_*).
// Where it pays (profiles/r04_stream_variants.txt, BASELINE configs[2]'s shape over batch sizes, four boxes): two slabs of
// rows per wave in LDS leave room for half the classic kernel's waves, so it wins where overlap is worth more than
// residency - launches of one step whose arrays total about the size of the 256 MiB Infinity Cache (+12-13 % at
// 65 536 ladders x 32 x dim 30, 280 MiB: reads partly served on-die, the classic kernel's lock-step the bottleneck); it
// ties (+-2 %) on batches that fit the cache and trails by 1-6 % where everything streams from HBM (both forms then move
// 0.86-0.9 of what a plain copy moves); from two steps per launch on the classic kernel's residency wins.  AUTO takes it
//   - for launches of one step (kStreamMaxSteps),
//   - whose arrays total kStreamMinBytes..kStreamMaxBytes (0.75x .. 1.75x the Infinity Cache),
//   - where the variant has a streaming twin (dim compiled in, n_temps <= 64) and the layout allows whole aligned 16-byte
//     vectors per group (every group full: n_chains a multiple of the ladders per wave; cpw * n_temps * dim a multiple of
//     4 and cpw * n_temps even; state, sq_jump and n_accept 16-byte aligned) - otherwise the classic kernel's general staging.
constexpr int kStreamMaxSteps = 1;
constexpr long long kStreamMinBytes = 192ll << 20, kStreamMaxBytes = 448ll << 20;

// what the calling thread's most recent ptrwm_run launched (ptrwm_last_launch_kind: tests and the benchmark's record)
static thread_local int t_last_launch_kind = 0;
static thread_local int t_last_launch_functor = 0;  // ... and with which functor (ptrwm_last_launch_functor)

static bool stream_layout_ok(const ptrwm_run_args *args, int dim, int cpw) {
  return args->n_temps <= 64 && args->n_chains % cpw == 0 && ((long long)cpw * args->n_temps * dim) % 4 == 0 &&
         (cpw * args->n_temps) % 2 == 0 && (reinterpret_cast<uintptr_t>(args->state) & 15u) == 0 &&
         (reinterpret_cast<uintptr_t>(args->sq_jump) & 15u) == 0 && (reinterpret_cast<uintptr_t>(args->n_accept) & 15u) == 0;
}

// SIMDs (compute units x 4) of the device that owns `stream` - the device the launch will run on - or, for the NULL
// stream, of the calling thread's current device; asked once per device; 0 if the runtime cannot say.  The form rule is
// stated in wavefronts per SIMD, so a partitioned or CU-masked device (or another CDNA part) gets the rule scaled to what
// it really has - and where the count is unknown AUTO keeps the one-thread-per-replica form (never wrong, only a speed).
static long long device_simds(hipStream_t stream) {
  constexpr int kMaxDevices = 64;
  static int cached[kMaxDevices];  // 0 = not asked yet (a race merely asks twice)
  int dev = -1;
  hipDevice_t owner;
  if (stream != nullptr && hipStreamGetDevice(stream, &owner) == hipSuccess) dev = (int)owner;
  else if (hipGetDevice(&dev) != hipSuccess) dev = -1;
  if (dev < 0 || dev >= kMaxDevices) return 0;
  int n = __atomic_load_n(&cached[dev], __ATOMIC_RELAXED);
  if (n == 0) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) return 0;
    n = 4 * cus;
    __atomic_store_n(&cached[dev], n, __ATOMIC_RELAXED);
  }
  return n;
}

// AUTO's choice for a launch of n_chains ladders on a device of n_simds SIMDs where both forms exist
static bool auto_prefers_lane_split(int dim, int n_temps, long long n_chains, long long n_simds) {
  if (n_simds <= 0) return false;
  const long long cpw1 = n_temps > 64 ? 1 : 64 / n_temps;
  const long long waves1 = n_temps > 64 ? n_chains * ((n_temps + 63) / 64) : (n_chains + cpw1 - 1) / cpw1;
  return lane_split_is_faster(dim, n_temps, (double)waves1 / (double)n_simds);
}

#ifndef PTRWM_SOURCE_HASH
#define PTRWM_SOURCE_HASH "unknown (built without csrc/Makefile)"
#endif


// alt: the specialised functor of the kind (0: none) - for RoughCarpet 1 = RoughCarpet2 (the host proved the third
// mixture term negligible, rough_carpet_two_term), 2 = RoughCarpetSym (also modes -m, 0, +m, rough_carpet_fold); for
// ThreeMixture 1 = ThreeMixture1 (the caller declared means that differ in the first coordinate only, ip[0] = 1)
static const QuadVariants &quad_variants(int kind, int alt) {
  switch (kind) {
    case PTRWM_TARGET_ROUGH_CARPET:
      return alt == 2 ? rough_carpet_sym_variants_quad() : (alt == 1 ? rough_carpet2_variants_quad() : rough_carpet_variants_quad());
    case PTRWM_TARGET_THREE_MIXTURE: return alt != 0 ? three_mixture1_variants_quad() : three_mixture_variants_quad();
    case PTRWM_TARGET_FULL_ROSENBROCK: return full_rosenbrock_variants_quad();
    case PTRWM_TARGET_EVEN_ROSENBROCK: return even_rosenbrock_variants_quad();
    case PTRWM_TARGET_HYBRID_ROSENBROCK: return hybrid_rosenbrock_variants_quad();
    case PTRWM_TARGET_IID_GAMMA: return iid_gamma_variants_quad();
    case PTRWM_TARGET_IID_BETA: return iid_beta_variants_quad();
    case PTRWM_TARGET_DIAG_GAUSSIAN: return diag_gaussian_variants_quad();
    case PTRWM_TARGET_HYPERCUBE: return hypercube_variants_quad();
    default: return neal_funnel_variants_quad();
  }
}

static VariantPair target_variants(int kind, int alt = 0) {
#define PTRWM_PAIR(SYMBOL) VariantPair{&SYMBOL##_narrow(), &SYMBOL##_wide()}
  switch (kind) {
    case PTRWM_TARGET_ROUGH_CARPET:
      // (the folded tables have no wide object: nothing of theirs lives above width 64)
      return alt == 2 ? VariantPair{&rough_carpet_sym_variants_narrow(), &rough_carpet_sym_variants_narrow()}
                      : (alt == 1 ? PTRWM_PAIR(rough_carpet2_variants) : PTRWM_PAIR(rough_carpet_variants));
    case PTRWM_TARGET_THREE_MIXTURE: return alt != 0 ? PTRWM_PAIR(three_mixture1_variants) : PTRWM_PAIR(three_mixture_variants);
    case PTRWM_TARGET_FULL_ROSENBROCK: return PTRWM_PAIR(full_rosenbrock_variants);
    case PTRWM_TARGET_EVEN_ROSENBROCK: return PTRWM_PAIR(even_rosenbrock_variants);
    case PTRWM_TARGET_HYBRID_ROSENBROCK: return PTRWM_PAIR(hybrid_rosenbrock_variants);
    case PTRWM_TARGET_IID_GAMMA: return PTRWM_PAIR(iid_gamma_variants);
    case PTRWM_TARGET_IID_BETA: return PTRWM_PAIR(iid_beta_variants);
    case PTRWM_TARGET_DIAG_GAUSSIAN: return PTRWM_PAIR(diag_gaussian_variants);
    case PTRWM_TARGET_HYPERCUBE: return PTRWM_PAIR(hypercube_variants);
    default: return PTRWM_PAIR(neal_funnel_variants);
  }
#undef PTRWM_PAIR
}

static int check_target(const ptrwm_target_desc *t) {
  if (t == nullptr) return PTRWM_E_NULL;
  if (t->kind < 0 || t->kind >= PTRWM_TARGET_COUNT) return PTRWM_E_KIND;
  if (t->dim < 1 || t->dim > PTRWM_MAX_DIM) return PTRWM_E_DIM;
  switch (t->kind) {
    case PTRWM_TARGET_THREE_MIXTURE:
      if (t->vec0 == nullptr) return PTRWM_E_NULL;
      if (t->ip[0] != 0 && t->ip[0] != 1) return PTRWM_E_ARG;
      break;
    case PTRWM_TARGET_FULL_ROSENBROCK:
      if (t->dim < 2) return PTRWM_E_DIM;
      if (t->vec0 == nullptr) return PTRWM_E_NULL;
      break;
    case PTRWM_TARGET_EVEN_ROSENBROCK:
      if (t->dim < 2 || (t->dim & 1)) return PTRWM_E_DIM;
      if (t->vec0 == nullptr) return PTRWM_E_NULL;
      break;
    case PTRWM_TARGET_DIAG_GAUSSIAN:
      if (t->vec0 == nullptr || (t->ip[0] == 0 && t->vec1 == nullptr)) return PTRWM_E_NULL;
      break;
    case PTRWM_TARGET_HYBRID_ROSENBROCK:
      if (t->ip[0] < 2 || t->ip[1] < 1) return PTRWM_E_ARG;
      if (t->dim != 1 + t->ip[1] * (t->ip[0] - 1)) return PTRWM_E_DIM;
      break;
    default:
      break;
  }
  return PTRWM_OK;
}

// Checks of ptrwm_run_args that several entry points make (each where it always has: the order of an entry point's checks is
// the code a caller with two defects gets).
static bool has_abi_size(const ptrwm_run_args *args) { return args->struct_size == sizeof(ptrwm_run_args); }
static bool temps_in_range(int n_temps) { return n_temps >= 1 && n_temps <= PTRWM_MAX_TEMPS; }
static bool is_flag(int v) { return v == 0 || v == 1; }
static bool swap_rule_known(const ptrwm_run_args *args) {
  return (args->swap_mode == PTRWM_SWAP_EXCHANGE || args->swap_mode == PTRWM_SWAP_REFERENCE_COPY) &&
         (args->swap_order == PTRWM_ORDER_SEQUENTIAL || args->swap_order == PTRWM_ORDER_EVEN_ODD);
}
// a fused run or a stand-alone sweep: float or double states, none of the split steps' fields
static bool fused_fields_ok(const ptrwm_run_args *args) {
  return is_flag(args->state_f64) && args->split_flags == 0 && args->device_step == nullptr;
}

// RoughCarpet: is the smallest of the three per-dimension mixture terms always < 2^-27 of the largest?
// In log2 units a_k(x) = -0.5 log2(e) (x - m_k)^2 + log2 w_k; the three parabolas share their curvature, so every
// difference a_j - a_k is LINEAR in x and g(x) = max_k a_k - min_k a_k is the maximum of six lines: convex and
// piecewise linear.  Its minimum over the real line is therefore attained where two of the lines cross (or g is
// constant), so checking the (at most 15) crossings is exact.  A few dozen flops: this runs on every ptrwm_run.
static bool rough_carpet_two_term(const float *p) {
  const double l2e = 1.4426950408889634;
  double sl[6], ic[6];  // line i: sl[i] * x + ic[i]
  int n = 0;
  for (int j = 0; j < 3; ++j)
    for (int k = 0; k < 3; ++k) {
      if (j == k) continue;
      const double mj = p[j], mk = p[k];
      sl[n] = l2e * (mj - mk);
      ic[n] = l2e * (-0.5 * (mj * mj - mk * mk) + ((double)p[3 + j] - (double)p[3 + k]));
      if (!(sl[n] == sl[n]) || !(ic[n] == ic[n])) return false;  // NaN parameters
      ++n;
    }
  auto g = [&](double x) {
    double v = -1e300;
    for (int i = 0; i < 6; ++i) {
      const double y = sl[i] * x + ic[i];
      v = y > v ? y : v;
    }
    return v;
  };
  double gmin = g(0.0);  // covers the all-slopes-equal (constant) case
  for (int i = 0; i < 6; ++i)
    for (int j = i + 1; j < 6; ++j) {
      if (sl[i] == sl[j]) continue;
      const double x = (ic[j] - ic[i]) / (sl[i] - sl[j]);
      if (!(x == x) || x > 1e30 || x < -1e30) continue;
      const double v = g(x);
      gmin = v < gmin ? v : gmin;
    }
  return gmin > 27.0;
}

// RoughCarpet, folded form (targets.h rc_fold_dim_term): may the kernel evaluate only the middle mode and the outer mode
// on the coordinate's own side?  Needs the two-term property (the three-term form's smallest term drops out, so the
// fold is compared with the two-term form), fp32-exact symmetry - one mode +-0, the other two exact negatives of each
// other, in any order - and that the FAR outer mode, wherever it is not the smallest of the three, lies more than 27
// (log2 units) below the largest.  On the side s x >= 0 the far mode is -m and every difference a_k - a_far is linear
// and increasing in s x (a common curvature; slope log2(e) (m_k + m) > 0 for k != far), so max_k a_k - a_far is
// increasing there and the bound at s x = 0 holds on the whole side; the other side is the mirror image.  On success
// `perm` holds the target's indices of the modes -m, 0, +m: the order the kernel reads p[0..2] / p[3..5] in.
static bool rough_carpet_fold(const float *p, int perm[3]) {
  for (int i = 0; i < 6; ++i)
    if (!std::isfinite(p[i])) return false;
  int z = -1;
  for (int i = 0; i < 3 && z < 0; ++i)
    if (p[i] == 0.0f) z = i;
  if (z < 0) return false;
  const int i = (z + 1) % 3, j = (z + 2) % 3;
  if (p[i] == 0.0f || p[i] != -p[j]) return false;
  perm[0] = p[i] < 0.0f ? i : j;
  perm[1] = z;
  perm[2] = p[i] < 0.0f ? j : i;
  if (!rough_carpet_two_term(p)) return false;
  const double l2e = 1.4426950408889634, m = p[perm[2]];
  const double a_neg = l2e * ((double)p[3 + perm[0]] - 0.5 * m * m), a_mid = l2e * (double)p[3 + perm[1]],
               a_pos = l2e * ((double)p[3 + perm[2]] - 0.5 * m * m);
  return std::max(a_mid, a_pos) - a_neg > 27.0 && std::max(a_mid, a_neg) - a_pos > 27.0;
}

// the specialised functor of a run's target (the `alt` of target_variants / quad_variants); fills `perm` for the folded
// rough carpet
static int specialised_form(const ptrwm_target_desc *t, int perm[3]) {
  if (t->kind == PTRWM_TARGET_ROUGH_CARPET) return rough_carpet_fold(t->p, perm) ? 2 : (rough_carpet_two_term(t->p) ? 1 : 0);
  if (t->kind == PTRWM_TARGET_THREE_MIXTURE) return t->ip[0] == 1 ? 1 : 0;
  return 0;
}

static TParams make_tparams(const ptrwm_target_desc *t) {
  TParams tp;
  for (int i = 0; i < 12; ++i) tp.p[i] = t->p[i];
  for (int i = 0; i < 4; ++i) tp.ip[i] = t->ip[i];
  tp.vec0 = t->vec0;
  tp.vec1 = t->vec1;
  tp.mask[0] = tp.mask[1] = 0;
  if (t->kind == PTRWM_TARGET_ROUGH_CARPET) {
    // fold the per-dimension -log(sqrt(2 pi)) of multimodal_torch.py:500 into one constant
    tp.p[7] = -(float)t->dim * 0.91893853320467274178f;
  }
  if (t->kind == PTRWM_TARGET_HYBRID_ROSENBROCK) {
    const int blk = t->ip[0] - 1;
    for (int i = 1; i < t->dim; ++i)
      if ((i - 1) % blk == 0) tp.mask[i >> 6] |= (1ull << (i & 63));
  }
  return tp;
}

static PParams make_pparams(const ptrwm_proposal_desc *proposal) { return {proposal->dim_scale, proposal->inv_dim}; }

__global__ void split_advance_kernel(long long *device_step, long long n) { *device_step += n; }

__global__ void philox_raw_kernel(uint32_t *__restrict__ out, long long n, uint32_t c0, uint32_t c1, uint32_t c2,
                                  uint32_t c3, uint32_t k0, uint32_t k1) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const u32x4 r = philox4x32_10(c0 + (uint32_t)i, c1, c2, c3, k0, k1);
  out[4 * i + 0] = r.x;
  out[4 * i + 1] = r.y;
  out[4 * i + 2] = r.z;
  out[4 * i + 3] = r.w;
}

// Stand-alone swap event: one workgroup per ladder, thread t = temperature t.  The decision is swap_decide(), the
// code the fused kernel runs; the row permutation goes through LDS in column chunks (a permutation of rows can be
// applied to every block of columns independently), so any (n_temps, dim) fits the 32 KB static buffer.
struct SweepArgs {
  float *state, *logp;
  const float *beta, *ext_swap_u;
  long long *swap_accept, *last_swap_ordinal;
  const float *prev;  // split step: states before the step's MH move, or NULL
  double *sq_jump;    // split step: += |final - prev|^2 per replica (the fused kernel's swap-step jump), or NULL
  long long chain_offset, event_index;
  unsigned long long step;
  int n_temps, dim, swap_mode, swap_order, rng_stream, chunk;
  unsigned k0, k1;
  // device-step mode (include/ptrwm.h device_step): the step index, whether an event is due and its number come from here
  const long long *device_step;
  long long burn_in, swap_every, event_offset;
  // replica flow (include/ptrwm.h ptrwm_flow_args, flow.h; NULL flow_walker = off)
  int *flow_walker;
  long long *flow_round_trips, *flow_up, *flow_down;
};
constexpr int kSweepLdsBytes = 32768;  // at most: rows (and, in a split step, the pre-step rows) of one column chunk

// state_t: float, or double for the reference's dtype=torch.float64 states (ptrwm_swap_sweep with state_f64 = 1: the
// permutation only - the squared-jump bookkeeping belongs to split steps, which carry float states).
// LDS is sized by the launch to what the ladder needs (rows of one column chunk, twice that in a split step): round 3's
// fixed 32 KB left four workgroups - four wavefronts - per CU and the kernel at a tenth of the memory rate.
template <class state_t>
__global__ void __launch_bounds__(256) swap_sweep_kernel(SweepArgs a) {
  if (a.device_step != nullptr) {
    // the swap event of step *device_step, if that step has one (ptrwm_split_accept's host-side rule, on the device)
    const long long s0 = *a.device_step + (long long)a.step, sc = s0 + 1;  // (a.step: this call's offset, include/ptrwm.h)
    if (!periodic_step_due(sc, a.burn_in, a.swap_every)) return;  // (grid-uniform)
    a.step = (unsigned long long)s0;
    a.event_index = swap_event_number(sc, a.burn_in, a.swap_every) + a.event_offset;
  }
  extern __shared__ __attribute__((aligned(16))) unsigned char s_sweep[];
  __shared__ float s_l[256], s_u[256];
  __shared__ int s_src[256];
  const int T = a.n_temps, D = a.dim, tid = threadIdx.x, nthr = blockDim.x;
  state_t *const s_rows = reinterpret_cast<state_t *>(s_sweep);
  state_t *const s_prev = s_rows + T * a.chunk;  // (split steps only)
  const long long chain = blockIdx.x;
  const bool live = tid < T;
  const int t = live ? tid : 0;
  float my_l = a.logp[chain * T + t];
  // event 0 of the call, on the counter words of the fused kernel's swap uniforms with this call's stream (kernel.h swap_uniform_*)
  const unsigned long long gchain = (unsigned long long)(a.chain_offset + chain);
  float us;
  if (a.ext_swap_u != nullptr) us = swap_uniform_ext(a.ext_swap_u, 0, 0, chain, T, t);
  else us = swap_uniform_philox(step_word_c0hi(a.step), step_word_c1(a.step), chain_word_c2(gchain),
                                with_stream(chain_word_c3(gchain, (uint32_t)t), (uint32_t)a.rng_stream), a.k0, a.k1);
  if (live) {
    s_l[tid] = my_l;
    s_u[tid] = us;
  }
  // the ladder's verdict on the form of its sequential sweep, from the values it enters the event with (kernel.h)
  const bool plain = __syncthreads_and(swap_pair_plain(T, t, sub_rn(a.beta[t], a.beta[t < T - 1 ? t + 1 : t]), my_l, us) ? 1 : 0) != 0;
  int src = t;
  bool pair_acc = false;
  __shared__ int s_landed[256];
  swap_decide(T, t, 0, t, a.swap_mode, a.swap_order, (int)(a.event_index & 1), a.beta, a.beta[t], us, s_l, s_u, s_landed,
              my_l, src, pair_acc, [] { __syncthreads(); }, plain);
  if (live) s_src[tid] = src;
  __syncthreads();
  if (a.flow_walker != nullptr) {  // (grid-uniform)
    // replica flow, all of it behind swap_decide (flow.h): the word travels as the row does.  Every thread fetches the word
    // of position `src` from HBM; the barrier keeps the stores below behind every fetch of the ladder.  Thread 0 is the
    // ladder's one writer of round_trips.
    int *const wk = a.flow_walker + chain * T;
    const int32_t w_src = live ? wk[src] : 0;
    __syncthreads();
    if (live) {
      bool trip;
      const int32_t fw = flow_ends(w_src, t, T, trip);
      wk[t] = fw;
      if (trip && flow_id(fw) < T && a.flow_round_trips != nullptr) a.flow_round_trips[chain * T + flow_id(fw)] += 1;
      if (a.flow_up != nullptr && flow_visit_up(fw) != 0u) a.flow_up[chain * T + t] += 1;
      if (a.flow_down != nullptr && flow_visit_down(fw) != 0u) a.flow_down[chain * T + t] += 1;
    }
  }
  state_t *gs = reinterpret_cast<state_t *>(a.state) + chain * T * (long long)D;
  const float *prev = a.prev != nullptr ? a.prev + chain * T * (long long)D : nullptr;
  // |final - prev|^2 of this thread's replica in the canonical four-range order of the fused kernel (philox.h)
  const int W = canon_width(D);
  float j2p0 = 0.0f, j2p1 = 0.0f, j2p2 = 0.0f, j2p3 = 0.0f;
  for (int c0 = 0; c0 < D; c0 += a.chunk) {
    const int w = (D - c0 < a.chunk) ? D - c0 : a.chunk;
    const bool whole = w == D;  // one chunk holds whole rows: element i of the tile is element i of the ladder's run
    for (int i = tid; i < T * w; i += nthr) {
      const int tt = whole ? 0 : i / w, dd = whole ? i : i - tt * w;
      s_rows[i] = gs[tt * D + c0 + dd];
      if (prev != nullptr) s_prev[i] = static_cast<state_t>(prev[tt * D + c0 + dd]);
    }
    __syncthreads();
    for (int i = tid; i < T * w; i += nthr) {
      const int tt = i / w, dd = i - tt * w;
      gs[tt * D + c0 + dd] = s_rows[s_src[tt] * w + dd];
    }
    if (live && prev != nullptr) {
      for (int dd = 0; dd < w; ++dd) {
        const float dl = sub_rn(static_cast<float>(s_rows[src * w + dd]), static_cast<float>(s_prev[t * w + dd]));
        const int qi = (c0 + dd) / W;
        if (qi == 0) j2p0 = fmaf(dl, dl, j2p0);
        else if (qi == 1) j2p1 = fmaf(dl, dl, j2p1);
        else if (qi == 2) j2p2 = fmaf(dl, dl, j2p2);
        else j2p3 = fmaf(dl, dl, j2p3);
      }
    }
    __syncthreads();
  }
  if (live) {
    const long long rep = chain * T + t;
    a.logp[rep] = my_l;
    if (a.sq_jump != nullptr) a.sq_jump[rep] += (double)add_rn(add_rn(j2p0, j2p1), add_rn(j2p2, j2p3));
    if (pair_acc) {
      if (a.swap_accept != nullptr) a.swap_accept[rep] += 1;
      if (a.last_swap_ordinal != nullptr) {
        const long long ord = swap_attempt_ordinal(a.swap_order, a.event_index, T, t);
        if (ord > a.last_swap_ordinal[rep]) a.last_swap_ordinal[rep] = ord;
      }
    }
  }
}

// Split step, second half: Metropolis rule on caller-evaluated log-densities, one thread per replica.  `proposals`
// comes back holding the pre-step states (the swap event of this step, if any, needs them for the jump distance).
struct SplitAcceptArgs {
  float *state, *logp, *proposals;
  const float *beta, *accept_u, *logp_new;
  long long *n_accept;
  double *sq_jump;
  unsigned char *accept_flags;
  long long n_reps;
  int n_temps, dim, count_on, swap_due;
  const long long *device_step;  // device-step mode: count_on / swap_due are derived from *device_step + step_offset
  long long step_offset;
  long long burn_in, swap_every;
};

// One wavefront per tile of 64 replicas (64-thread workgroups): the tile's rows of `state` and of `proposals` go through two
// slabs of LDS in both directions (kernel.h stage_copy: coalesced 16-byte transfers), every lane works on its own row in
// LDS.  (Round 3's version walked its rows in HBM, 64 cache lines per instruction: 2.6 ms per step at 65 536 x 32 x
// dim 30 - 70 % of a split step - where moving the bytes takes 0.2.)
__global__ void __launch_bounds__(64) split_accept_kernel(SplitAcceptArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_tiles[];
  const int lane = (int)threadIdx.x;
  const long long first = (long long)blockIdx.x * 64;
  if (first >= a.n_reps) return;
  if (a.device_step != nullptr) {
    const SplitStepDue due = split_step_due(*a.device_step + a.step_offset + 1, a.burn_in, a.swap_every, a.n_temps);
    a.count_on = due.count_on;
    a.swap_due = due.swap_due;
  }
  const int D = a.dim;
  const int n_rows = (a.n_reps - first < 64) ? (int)(a.n_reps - first) : 64;
  float *const xs = s_tiles, *const ys = s_tiles + (64 * D + 4);
  float *__restrict__ gx = a.state + first * D;
  float *__restrict__ gy = a.proposals + first * D;
  stage_copy<true>(xs, gx, n_rows * D, lane, 64);
  stage_copy<true>(ys, gy, n_rows * D, lane, 64);
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const bool live = lane < n_rows;
  const long long i = first + (live ? lane : 0);
  bool acc = false;
  float lp_new = 0.0f, j2 = 0.0f;
  if (live) {
    const int t = (int)(i % a.n_temps);
    const float lp = a.logp[i];
    lp_new = a.logp_new[i];
    acc = mh_accept(a.beta[t], lp_new, lp, a.accept_u[i]);
    float *__restrict__ x = xs + stage_head(gx) + lane * D;
    float *__restrict__ y = ys + stage_head(gy) + lane * D;
    // squared jump in the canonical four-range order of the fused kernel (philox.h)
    const int W = canon_width(D);
    float j2p[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int d1 = (q + 1) * W < D ? (q + 1) * W : D;
      for (int d = q * W; d < d1; ++d) {
        const float xo = x[d], yn = y[d];
        const float dl = sub_rn(yn, xo);
        j2p[q] = fmaf(dl, dl, j2p[q]);
        if (acc) x[d] = yn;
        y[d] = xo;
      }
    }
    // (the proposal's own squared jump when ptrwm_split_propose recorded one: second plane of accept_u, kernel.h)
    const float given = a.accept_u[a.n_reps + i];
    j2 = given >= 0.0f ? given : tree4_add(j2p);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  stage_copy<false>(xs, gx, n_rows * D, lane, 64);
  // the pre-step states go back in place of the proposals only where somebody reads them: the swap kernel of a swap step
  // (its squared jump is |final - pre-step|^2).  A quarter of this kernel's HBM traffic on the other nine steps in ten.
  if (a.swap_due) stage_copy<false>(ys, gy, n_rows * D, lane, 64);
  if (!live) return;
  if (acc) a.logp[i] = lp_new;
  if (a.accept_flags != nullptr) a.accept_flags[i] = acc ? 1 : 0;
  if (a.count_on) {
    if (a.n_accept != nullptr) a.n_accept[i] += acc ? 1 : 0;
    // a swap step's jump (MH move and swap together) is added by the sweep that follows
    if (a.sq_jump != nullptr && !a.swap_due && acc) a.sq_jump[i] += (double)j2;
  }
}

template <template <int> class Proposal>
static hipError_t launch_split_propose(int wi, const float *state, float *proposals, float *accept_u, long long n_chains,
                                       long long chain_offset, unsigned long long step, int D, int T, const float *ts,
                                       const PParams &pp, const float *ext_raw, const float *ext_u, int n_raw,
                                       unsigned k0, unsigned k1, const long long *dstep, hipStream_t st) {
  const long long tot = n_chains * T;
  const dim3 grid((unsigned)((tot + 63) / 64)), block(64);  // one wavefront per tile of 64 replicas (kernel.h)
  const unsigned lds = split_tile_lds_bytes(D);
  int idx = 0;
#define PTRWM_X_SPLIT(W, E)                                                                                       \
  if (wi == idx++)                                                                                                \
    hipLaunchKernelGGL((ptrwm_split_propose_kernel<Proposal<W>, W>), grid, block, lds, st, state, proposals,     \
                       accept_u, n_chains, chain_offset, step, D, T, ts, pp, ext_raw, ext_u, n_raw, k0, k1, dstep);
  PTRWM_WIDTHS(PTRWM_X_SPLIT)
#undef PTRWM_X_SPLIT
  return hipGetLastError();
}

template <template <int> class Proposal>
static hipError_t launch_propose(int wi, float *out, long long n, int D, int T, const float *ts, const PParams &pp,
                                 const float *ext_raw, int n_raw, unsigned k0, unsigned k1, hipStream_t st) {
  const long long tot = n * T;
  const dim3 grid((unsigned)((tot + kBlockThreads - 1) / kBlockThreads)), block(kBlockThreads);
  int idx = 0;
#define PTRWM_X_PROPOSE(W, E)                                                                              \
  if (wi == idx++)                                                                                         \
    hipLaunchKernelGGL((ptrwm_propose_kernel<Proposal<W>, W>), grid, block, 0, st, out, n, D, T, ts, pp,   \
                       ext_raw, n_raw, k0, k1);
  PTRWM_WIDTHS(PTRWM_X_PROPOSE)
#undef PTRWM_X_PROPOSE
  return hipGetLastError();
}

// One swap event over the current states (ptrwm_swap_sweep, and the swap step of ptrwm_split_accept).
static int32_t launch_sweep(const ptrwm_run_args *args, int32_t dim, int64_t event_index, int32_t rng_stream,
                            const float *prev, double *sq_jump, const ptrwm_flow_args *flow, hipStream_t stream) {
  SweepArgs a;
  a.flow_walker = flow != nullptr ? flow->walker : nullptr;
  a.flow_round_trips = flow != nullptr ? (long long *)flow->round_trips : nullptr;
  a.flow_up = flow != nullptr ? (long long *)flow->n_up : nullptr;
  a.flow_down = flow != nullptr ? (long long *)flow->n_down : nullptr;
  a.state = args->state;
  a.logp = args->logp;
  a.beta = args->beta;
  a.ext_swap_u = args->ext_swap_u;
  a.swap_accept = (long long *)args->swap_accept;
  a.last_swap_ordinal = (long long *)args->last_swap_ordinal;
  a.prev = prev;
  a.sq_jump = sq_jump;
  a.chain_offset = args->chain_offset;
  a.event_index = event_index;
  a.step = (unsigned long long)args->step0;
  a.n_temps = args->n_temps;
  a.dim = dim;
  a.swap_mode = args->swap_mode;
  a.swap_order = args->swap_order;
  a.rng_stream = rng_stream;
  // columns per pass: whole rows where they fit the LDS budget (a split step stages the pre-step rows beside them)
  const bool f64 = args->state_f64 == 1;
  const int per_elem = (f64 ? 8 : 4) * (prev != nullptr ? 2 : 1);
  int chunk = kSweepLdsBytes / (per_elem * args->n_temps);  // >= 16 columns
  if (chunk > dim) chunk = dim;
  a.chunk = chunk;
  const unsigned lds = (unsigned)(chunk * args->n_temps * per_elem);
  a.k0 = philox_key(args->seed).k0;
  a.k1 = philox_key(args->seed).k1;
  a.device_step = prev != nullptr ? (const long long *)args->device_step : nullptr;  // (split steps only)
  a.burn_in = args->burn_in;
  a.swap_every = args->swap_every;
  a.event_offset = args->swap_event_offset;
  const unsigned block = (unsigned)group_threads(args->n_temps, 1);  // one ladder per workgroup, thread t = temperature t
  if (f64)
    hipLaunchKernelGGL(swap_sweep_kernel<double>, dim3((unsigned)args->n_chains), dim3(block), lds, stream, a);
  else
    hipLaunchKernelGGL(swap_sweep_kernel<float>, dim3((unsigned)args->n_chains), dim3(block), lds, stream, a);
  return hipGetLastError() == hipSuccess ? PTRWM_OK : PTRWM_E_LAUNCH;
}

// Moments of one split step (ptrwm_split_moments): the state / log-density after the step, summed over a tile of
// kSplitMomChains chains per workgroup - thread k owns element k of the first temps * dim floats of every chain's run
// (contiguous: coalesced reads chain after chain) and keeps its two sums in registers - then one no-return fp64 atomic
// per element and workgroup.
constexpr int kSplitMomChains = 256;
struct SplitMomentsArgs {  // (of both kernels)
  const float *state, *logp;
  double *sum, *sum_sq, *sum_logp;
  long long *count;
  long long n_chains, step, burn_in, every;
  const long long *device_step;
  int n_temps, dim, temps;
};

__global__ void __launch_bounds__(256) split_moments_kernel(SplitMomentsArgs a) {
  if (!snapshot_step_due(a.step, a.device_step, a.burn_in, a.every)) return;  // (is the step just performed an accumulated one?)
  const long long c0 = (long long)blockIdx.x * kSplitMomChains;
  const long long c1 = (a.n_chains - c0 < kSplitMomChains) ? a.n_chains : c0 + kSplitMomChains;
  const int td = a.temps * a.dim;
  const long long run = (long long)a.n_temps * a.dim;
  for (int k = threadIdx.x; k < td; k += blockDim.x) {
    double s = 0.0, q = 0.0;
    for (long long c = c0; c < c1; ++c) {
      const double v = (double)a.state[c * run + k];
      s += v;
      q += v * v;
    }
    unsafeAtomicAdd(a.sum + k, s);
    unsafeAtomicAdd(a.sum_sq + k, q);
  }
  if (a.sum_logp != nullptr) {
    for (int t = threadIdx.x; t < a.temps; t += blockDim.x) {
      double s = 0.0;
      for (long long c = c0; c < c1; ++c) s += (double)a.logp[c * a.n_temps + t];
      unsafeAtomicAdd(a.sum_logp + t, s);
    }
  }
  if (a.count != nullptr)
    for (int t = threadIdx.x; t < a.temps; t += blockDim.x) count_add(&a.count[t], c1 - c0);
}

// Per-chain moments of one split step (ptrwm_split_chain_moments): one thread per (chain, t < temps, d), a plain
// read-modify-write of its own two elements - the same sequential fp64 sums as the fused kernels' (v * v is exact in fp64).
__global__ void __launch_bounds__(256) split_chain_moments_kernel(SplitMomentsArgs a) {
  if (!snapshot_step_due(a.step, a.device_step, a.burn_in, a.every)) return;  // (is the step just performed an accumulated one?)
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const int td = a.temps * a.dim;
  if (i >= a.n_chains * td) return;
  const long long c = i / td;
  const int k = (int)(i - c * td), t = k / a.dim, d = k - t * a.dim;
  const long long rep = c * a.n_temps + t;
  const double v = (double)a.state[rep * a.dim + d];
  a.sum[i] += v;
  a.sum_sq[i] += v * v;
  if (d == 0 && a.sum_logp != nullptr) a.sum_logp[c * a.temps + t] += (double)a.logp[rep];
  if (i < a.temps && a.count != nullptr) a.count[i] += 1;
}

// Pooled marginal histograms (ptrwm_histogram, and the snapshots of ptrwm_run_with_histogram): one snapshot of `state`,
// shaped as split_moments_kernel - a workgroup takes a tile of kHistChains chains (blockIdx.x) and a group of `cols` of the
// first temps * dim elements of every chain's run (blockIdx.y); consecutive threads read consecutive elements of a chain, and
// where a group has fewer than 256 columns the workgroup's threads take 256 / cols chains at a time.  Counters: 32-bit, in
// LDS, n_bins + 2 per column of the group, added to with ds_add_u32 (columns are shared between the chains in flight) and
// flushed once per workgroup, one no-return 64-bit atomic per NON-ZERO counter (count_add).  kHistLdsCounters = 32 KiB of
// LDS: up to five workgroups per CU.  `direct` (n_bins + 2 > kHistLdsCounters / kHistMinCols: fewer than a wavefront's worth
// of columns would fit): no LDS, every sample is one global atomic.  The constants and the host's choice of `cols` and
// `direct` are hist.h's (hist_geometry).
struct HistOwn {
  const float *lo, *scale;
  long long *counts, *count;
};
struct HistSnapArgs : SnapHead<HistOwn> {
  int temps, n_bins, cols, direct;
};

template <class state_t>
__global__ void __launch_bounds__(256) hist_snapshot_kernel(HistSnapArgs a) {
  if (!a.due()) return;  // (snapshot.h)
  __shared__ unsigned s_cnt[kHistLdsCounters];
  const int tid = (int)threadIdx.x, nbp = a.n_bins + 2, td = a.temps * a.dim;
  const int k0 = (int)blockIdx.y * a.cols;
  const int cols = td - k0 < a.cols ? td - k0 : a.cols;  // (1..256; cols * nbp <= kHistLdsCounters unless direct)
  const long long c0 = (long long)blockIdx.x * kHistChains;
  const long long c1 = (a.n_chains - c0 < kHistChains) ? a.n_chains : c0 + kHistChains;
  const bool direct = a.direct != 0;
  if (!direct) {
    for (int i = tid; i < cols * nbp; i += 256) s_cnt[i] = 0u;
    __syncthreads();
  }
  const int per = 256 / cols, sub = tid / cols, kk = tid - sub * cols;  // chains in flight; this thread's; its column
  if (sub < per) {
    const int k = k0 + kk;
    const float lo = a.own.lo[k % a.dim], sc = a.own.scale[k % a.dim];
    const long long run = (long long)a.n_temps * a.dim;
    const state_t *__restrict__ p = reinterpret_cast<const state_t *>(a.state) + k;
    for (long long c = c0 + sub; c < c1; c += per) {
      const int b = hist_bin(static_cast<float>(p[c * run]), lo, sc, a.n_bins);
      if (direct) count_add(&a.own.counts[(long long)k * nbp + b], 1ll);
      else atomicAdd(&s_cnt[kk * nbp + b], 1u);
    }
  }
  if (!direct) {
    __syncthreads();
    for (int i = tid; i < cols * nbp; i += 256) {
      const unsigned v = s_cnt[i];
      if (v != 0u) count_add(&a.own.counts[(long long)k0 * nbp + i], (long long)v);
    }
  }
  if (blockIdx.y == 0 && a.own.count != nullptr)
    for (int t = tid; t < a.temps; t += 256) count_add(&a.own.count[t], c1 - c0);
}

// Pooled lagged autocovariance (ptrwm_autocorr, and the snapshots of ptrwm_run_with_autocorr; acf.h states the rule and the
// geometry): one snapshot of `state`, shaped as hist_snapshot_kernel - a workgroup takes a tile of a.chains chains (blockIdx.x)
// and a group of a.cols of the first temps * dim elements of every chain's run (blockIdx.y); consecutive threads read
// consecutive elements of a chain, and where a group has fewer than 256 columns the threads take a.per chains at a time.  A
// thread keeps its column of kAcfChainsPerThread chains of x_j in registers (read once), streams the same elements of the ring
// slot of every available lag past them - kAcfChainsPerThread independent loads in flight per lag - and sums its products and
// the ring's values in double.  Per lag the a.per threads of a column meet in LDS (ds_add_f64 into one of two buffers, taken
// in turn: one barrier per lag), and the column's first thread flushes the tile's three sums, one no-return fp64 atomic per
// non-zero sum.  (head: the sum of x_j, the same for every lag - it is the lag-0 `tail`.)  Then the thread overwrites its
// elements of slot j % max_lag: nobody else reads or writes them.
struct AcfOwn {
  void *ring;  // the state's type [max_lag, n_chains, temps * dim]
  double *sxy, *head, *tail;
  long long *pairs;
};
struct AcfSnapArgs : SnapHead<AcfOwn> {
  int temps, max_lag, cols, per, chains;
};

template <class state_t>
__global__ void __launch_bounds__(kAcfThreads) acf_snapshot_kernel(AcfSnapArgs a) {
  long long sc;
  if (!a.due(&sc)) return;  // (snapshot.h)
  constexpr int R = kAcfChainsPerThread;
  __shared__ double s_red[2][2][kAcfThreads];  // [buffer][sxy, tail][column of the group]
  const long long j = periodic_step_number(sc, a.burn_in, a.every);
  const int lags = acf_lags(j, a.max_lag);
  const int tid = (int)threadIdx.x, td = a.temps * a.dim;
  const int sub = tid / a.cols, kk = tid - sub * a.cols, k = (int)blockIdx.y * a.cols + kk;
  const bool live = sub < a.per && k < td;
  const bool first = live && sub == 0;
  const bool pooled = a.per > 1;  // (grid-uniform)
  const long long c0 = (long long)blockIdx.x * a.chains + sub;  // this thread's chains: c0, c0 + per, ...
  long long left = live ? (a.n_chains - c0 + a.per - 1) / a.per : 0;
  const int nv = left < 0 ? 0 : (left > R ? R : (int)left);  // ... nv of them
  if (pooled) {
    s_red[0][0][tid] = s_red[0][1][tid] = s_red[1][0][tid] = s_red[1][1][tid] = 0.0;
    __syncthreads();
  }
  const long long run = (long long)a.n_temps * a.dim, cstep = (long long)a.per * td;
  const long long slot_elems = a.n_chains * td, own = c0 * td + k;  // (of a slot: this thread's first element)
  state_t x[R];
  {
    const state_t *__restrict__ p = reinterpret_cast<const state_t *>(a.state) + c0 * run + k;
#pragma unroll
    for (int i = 0; i < R; ++i) x[i] = i < nv ? p[(long long)i * a.per * run] : state_t(0);
  }
  state_t *ring = reinterpret_cast<state_t *>(a.own.ring);
  const int t = k / a.dim, d = k - t * a.dim;
  const long long acc0 = (long long)t * (a.max_lag + 1) * a.dim + d;  // element [t, 0, d] of the sums
  double hsum = 0.0;
  for (int lag = 0; lag <= lags; ++lag) {
    double sx = 0.0, tl = 0.0;
    if (lag == 0) {
#pragma unroll
      for (int i = 0; i < R; ++i) {
        const double v = (double)x[i];
        sx += acf_term(v, v);
        tl += v;
      }
    } else if (nv > 0) {
      const state_t *r = ring + (long long)acf_lag_slot(j, lag, a.max_lag) * slot_elems + own;
      state_t y[R];
#pragma unroll
      for (int i = 0; i < R; ++i) y[i] = i < nv ? r[(long long)i * cstep] : state_t(0);
#pragma unroll
      for (int i = 0; i < R; ++i) {
        const double v = (double)y[i];
        sx += acf_term((double)x[i], v);
        tl += v;
      }
    }
    if (pooled) {
      const int b = lag & 1;
      if (live) {
        if (sx != 0.0) unsafeAtomicAdd(&s_red[b][0][kk], sx);
        if (tl != 0.0) unsafeAtomicAdd(&s_red[b][1][kk], tl);
      }
      __syncthreads();
      if (first) {
        sx = s_red[b][0][kk];
        tl = s_red[b][1][kk];
        s_red[b][0][kk] = 0.0;  // (added to again two lags on, behind the next barrier)
        s_red[b][1][kk] = 0.0;
      }
    }
    if (first) {
      if (lag == 0) hsum = tl;
      const long long e = acc0 + (long long)lag * a.dim;
      if (sx != 0.0) unsafeAtomicAdd(a.own.sxy + e, sx);
      if (hsum != 0.0) unsafeAtomicAdd(a.own.head + e, hsum);
      if (tl != 0.0) unsafeAtomicAdd(a.own.tail + e, tl);
    }
  }
  if (nv > 0) {
    state_t *w = ring + (long long)acf_slot(j, a.max_lag) * slot_elems + own;
#pragma unroll
    for (int i = 0; i < R; ++i)
      if (i < nv) w[(long long)i * cstep] = x[i];
  }
  if (blockIdx.x == 0 && blockIdx.y == 0)
    for (int lag = tid; lag <= lags; lag += kAcfThreads) count_add(&a.own.pairs[lag], a.n_chains);
}

// Pooled posterior covariance (ptrwm_covariance, and the snapshots of ptrwm_run_with_covariance; cov.h states the rule and the
// geometry): one snapshot of `state`.  A workgroup takes one covered temperature (blockIdx.y) and a tile of kCovChains chains
// (blockIdx.x), which pass through LDS in sub-tiles of kCovSubTile chains: rows of doubles, one per chain, consecutive lanes
// reading consecutive elements of a chain; the pad columns are zeroed once and never written, the rows past the last chain are
// written as zeros.  The Gram matrix of the tile is the lower triangle of 16 x 16 coordinate blocks; a block pair is one
// accumulator of v_mfma_f64_16x16x4_f64 (8 VGPRs), K running over the chains, and a wave owns its pairs for the whole tile
// (cov_pair_wave / cov_pair_slot): pair w + 4 q sits in the wave's accumulator q.  Per K-step and pair a lane reads its two
// operands from LDS, ONE double each - coordinate 16 bi + (lane & 15), and 16 bj + (lane & 15), of chain 4 ks + (lane >> 4) -
// and the owner of a diagonal pair adds the value to that block's sx.  The loop over a wave's pairs is unrolled over the
// compile-time maximum and guarded wave-uniformly, so that the accumulators are indexed statically (registers, no scratch).
// Flush: one no-return fp64 atomic per non-zero (i, j), j <= i < dim, and per sx element.
// The kernel only reads `state`.
struct CovOwn {
  double *sxx, *sx;
  long long *count;
};
struct CovSnapArgs : SnapHead<CovOwn> {};

typedef double cov_acc_t __attribute__((ext_vector_type(4)));

template <class state_t>
__global__ void __launch_bounds__(kCovThreads, 2) cov_snapshot_kernel(CovSnapArgs a) {
  if (!a.due()) return;  // (snapshot.h)
  extern __shared__ double s_cov[];  // [kCovSubTile][cov_row_stride(dim)]
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int dim = a.dim;
  const int t = (int)blockIdx.y;
  const long long c0 = (long long)blockIdx.x * kCovChains, run = (long long)a.n_temps * dim;
  const state_t *__restrict__ base = reinterpret_cast<const state_t *>(a.state) + (long long)t * dim;
  for (int e = tid; e < cov_lds_doubles(dim); e += kCovThreads) s_cov[e] = 0.0;  // (the pad columns stay zero)
  // this wave's pairs: accumulator q holds pair cov_wave_pair(w, q), q < nq
  const int nq = cov_wave_pairs(w, cov_pairs(cov_blocks(dim)));
  cov_acc_t acc[kCovPairsPerWave];
  double s[kCovPairsPerWave];
  int bi[kCovPairsPerWave], bj[kCovPairsPerWave];
#pragma unroll
  for (int q = 0; q < kCovPairsPerWave; ++q) {
    const int p = cov_wave_pair(w, q);
    bi[q] = cov_pair_row(p);
    bj[q] = cov_pair_col(p);
    acc[q] = cov_acc_t{0.0, 0.0, 0.0, 0.0};
    s[q] = 0.0;
  }
  const int per = kCovSubTile * dim;
  for (int sub = 0; sub < kCovSubTiles; ++sub) {
    const long long cs = c0 + (long long)sub * kCovSubTile;
    if (cs >= a.n_chains) break;  // (workgroup-uniform)
    __syncthreads();              // (the zeroing, or the previous sub-tile's reads)
    for (int e = tid; e < per; e += kCovThreads) {
      const int ch = cov_stage_chain(e, dim), d = cov_stage_coord(e, dim);
      const long long c = cs + ch;
      s_cov[cov_lds_at(ch, d, dim)] = c < a.n_chains ? (double)base[c * run + d] : 0.0;
    }
    __syncthreads();
#pragma unroll 2
    for (int ks = 0; ks < kCovKSteps; ++ks) {
      const double *row = s_cov + cov_lds_at(cov_operand_chain(ks, lane), 0, dim);
#pragma unroll
      for (int q = 0; q < kCovPairsPerWave; ++q)
        if (q < nq) {
          const double vi = row[cov_operand_coord(bi[q], lane)], vj = row[cov_operand_coord(bj[q], lane)];
          acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(vi, vj, acc[q], 0, 0, 0);
          s[q] += vi;  // (flushed for a diagonal pair only)
        }
    }
  }
  double *__restrict__ sxx = a.own.sxx + (long long)t * dim * dim;
#pragma unroll
  for (int q = 0; q < kCovPairsPerWave; ++q)
    if (q < nq) {
      const int j = cov_flush_j(bj[q], lane);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = cov_flush_i(bi[q], lane, r);
        const double val = acc[q][r];
        if (cov_flushed(i, j, dim) && val != 0.0) unsafeAtomicAdd(sxx + (long long)i * dim + j, val);
      }
      if (bi[q] == bj[q]) {        // the diagonal pair of a block: its sx (cov_sx_wave)
        double m = s[q];           // (the four K-quarters of a column meet: lanes l, l + 16, l + 32, l + 48)
        m += __shfl_xor(m, 16);
        m += __shfl_xor(m, 32);
        if (cov_sx_flushed(bi[q], lane, dim) && m != 0.0) unsafeAtomicAdd(a.own.sx + (long long)t * dim + kCovBlock * bi[q] + lane, m);
      }
    }
  if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) count_add(a.own.count, a.n_chains);
}

// ---- pooled log-density sums along the ladder (energy.h; include/ptrwm.h ptrwm_energy_args) -----------------------------------------
// Two kernels behind a due step (ptrwm_energy, and the snapshots of ptrwm_run_with_energy); both only read logp and beta, and
// both decide on the device whether the step counts (snapshot.h) - the first also whether ref is still to be set - so the pair
// can sit in a captured block of split steps.  logp is float32 for state_f64 runs too: one instance each.
struct EnergySnapArgs {
  const float *logp;  // [n_chains, n_temps]
  const float *beta;  // [n_temps]
  double *ref;        // [n_temps]
  int *ref_set;       // [1]
  long long *count, *nonfinite;       // [groups, n_temps], [1] or NULL
  double *s1, *s2, *colder, *hotter;  // [groups, n_temps]
  long long n_chains, chain_offset, step, burn_in, every;
  const long long *device_step;
  int n_temps, groups;
};

// ref: ONE workgroup, to any effect at most once per run (it need not be fast).  Thread i walks elements i, i + 256, ... of logp
// and keeps the largest key (energy.h: floats ordered as integers) of the temperature it stands on; the keys meet in LDS by an
// integer atomic max - a maximum does not depend on the order of evaluation.
__global__ void __launch_bounds__(kEnergyThreads) energy_ref_kernel(EnergySnapArgs a) {
  if (!snapshot_step_due(a.step, a.device_step, a.burn_in, a.every)) return;
  if (*a.ref_set != 0) return;  // (workgroup-uniform: nobody writes the flag in front of the barriers below)
  __shared__ int s_key[PTRWM_MAX_TEMPS];
  const int tid = (int)threadIdx.x, T = a.n_temps;
  for (int t = tid; t < T; t += kEnergyThreads) s_key[t] = kEnergyNoKey;
  __syncthreads();
  const long long n = a.n_chains * T;
  const int stride_t = kEnergyThreads % T;
  int t = tid % T, cur = t, best = kEnergyNoKey;  // (t == e % T throughout)
  for (long long e = tid; e < n; e += kEnergyThreads) {
    if (t != cur) {
      if (best != kEnergyNoKey) atomicMax(&s_key[cur], best);
      cur = t, best = kEnergyNoKey;
    }
    const float l = a.logp[e];
    if (energy_finite(l)) {
      const int key = energy_key(l);
      best = key > best ? key : best;
    }
    t += stride_t;
    if (t >= T) t -= T;
  }
  if (best != kEnergyNoKey) atomicMax(&s_key[cur], best);
  __syncthreads();
  for (int u = tid; u < T; u += kEnergyThreads) a.ref[u] = energy_ref_of(s_key[u]);
  if (tid == 0) *a.ref_set = 1;
}

// The sums: a workgroup serves one group's chains (blockIdx.y) and a tile of them (blockIdx.x), energy.h's geometry.  A thread
// keeps the five partial sums of the temperature its elements stand on in registers - for the whole tile where n_temps divides
// the workgroup - and adds them to the workgroup's LDS table when they move on; one atomic per non-zero (workgroup, sum,
// temperature) flushes.
__global__ void __launch_bounds__(kEnergyThreads) energy_snapshot_kernel(EnergySnapArgs a) {
  if (!snapshot_step_due(a.step, a.device_step, a.burn_in, a.every)) return;
  const int tid = (int)threadIdx.x, T = a.n_temps, G = a.groups, g = (int)blockIdx.y;
  const long long members = energy_group_chains(a.n_chains, a.chain_offset, G, g);
  const int n = energy_tile_elems((long long)blockIdx.x, members, T);  // (1 .. tile_chains * n_temps <= max(kEnergyTileElems, n_temps))
  if (n == 0) return;  // (workgroup-uniform: the tile lies behind the group's last chain)
  __shared__ double s_sum[4][PTRWM_MAX_TEMPS];  // s1, s2, colder, hotter
  __shared__ unsigned long long s_cnt[PTRWM_MAX_TEMPS];
  __shared__ double s_ref[PTRWM_MAX_TEMPS], s_dc[PTRWM_MAX_TEMPS], s_dh[PTRWM_MAX_TEMPS];
  __shared__ unsigned s_bad;
  for (int t = tid; t < T; t += kEnergyThreads) {
    s_sum[0][t] = s_sum[1][t] = s_sum[2][t] = s_sum[3][t] = 0.0;
    s_cnt[t] = 0ull;
    s_ref[t] = a.ref[t];
    s_dc[t] = t >= 1 ? (double)a.beta[t - 1] - (double)a.beta[t] : 0.0;
    s_dh[t] = t <= T - 2 ? (double)a.beta[t + 1] - (double)a.beta[t] : 0.0;
  }
  if (tid == 0) s_bad = 0u;
  __syncthreads();
  const long long first = energy_first_chain(a.chain_offset, G, g);
  const long long m0 = (long long)blockIdx.x * energy_tile_chains(T);
  const int stride_t = kEnergyThreads % T, stride_k = kEnergyThreads / T;
  int t = tid % T, k = tid / T;  // (t == e % T, k == e / T throughout: energy_elem_temp, energy_elem_member)
  int cur = t;
  unsigned cnt = 0u, bad = 0u;
  double v1 = 0.0, v2 = 0.0, vc = 0.0, vh = 0.0;
  const auto park = [&]() {
    if (cnt == 0u) return;
    atomicAdd(&s_cnt[cur], (unsigned long long)cnt);
    atomicAdd(&s_sum[0][cur], v1);
    atomicAdd(&s_sum[1][cur], v2);
    if (cur >= 1) atomicAdd(&s_sum[2][cur], vc);
    if (cur <= T - 2) atomicAdd(&s_sum[3][cur], vh);
  };
  for (int e = tid; e < n; e += kEnergyThreads) {
    if (t != cur) {
      park();
      cur = t, cnt = 0u, v1 = v2 = vc = vh = 0.0;
    }
    const long long c = first + (m0 + k) * G;  // (m0 + k < members: c < n_chains)
    const float l = a.logp[c * T + t];
    if (energy_finite(l)) {
      const double x = (double)l, y = x - s_ref[t];
      ++cnt;
      v1 += x;
      v2 += x * x;
      if (t >= 1) vc += exp(s_dc[t] * y);
      if (t <= T - 2) vh += exp(s_dh[t] * y);
    } else {
      ++bad;
    }
    t += stride_t, k += stride_k;
    if (t >= T) t -= T, ++k;
  }
  park();
  if (bad != 0u) atomicAdd(&s_bad, bad);
  __syncthreads();
  const long long row = (long long)g * T;
  for (int u = tid; u < T; u += kEnergyThreads) {
    const unsigned long long c = s_cnt[u];
    if (c == 0ull) continue;
    count_add(&a.count[row + u], (long long)c);
    if (s_sum[0][u] != 0.0) unsafeAtomicAdd(&a.s1[row + u], s_sum[0][u]);
    if (s_sum[1][u] != 0.0) unsafeAtomicAdd(&a.s2[row + u], s_sum[1][u]);
    if (u >= 1 && s_sum[2][u] != 0.0) unsafeAtomicAdd(&a.colder[row + u], s_sum[2][u]);
    if (u <= T - 2 && s_sum[3][u] != 0.0) unsafeAtomicAdd(&a.hotter[row + u], s_sum[3][u]);
  }
  if (tid == 0 && s_bad != 0u && a.nonfinite != nullptr) count_add(a.nonfinite, (long long)s_bad);
}

// ---- preconditioned Gaussian proposals (precond.h; include/ptrwm.h ptrwm_split_propose_precond) -----------------------------------
// ptrwm_split_propose's job for the Normal proposal with increments s_t L z: one run-time-dim kernel.  Geometry and index maps in
// precond.h.  A workgroup stages the factor into LDS once - zeros above the diagonal and in the pad; the caller's strict upper
// triangle is never read - and then walks tiles of kPrecRows rows: the tile's states come in through stage_copy, the step's
// normals are computed one Philox block per work item into the z slab, wave w multiplies its 16 rows by the factor on the matrix
// unit - block rows in pairs, so that two independent accumulators are in flight - and the epilogue is fmaf(s_t, acc, x) in place,
// behind which the slab leaves through stage_copy as the proposals.
struct PrecondProposeArgs {
  const float *state, *chol, *temp_scale, *ext_raw, *ext_u;
  float *proposals, *accept_u;
  long long n_reps, chain_offset;
  unsigned long long step;
  const long long *device_step;
  int n_temps, dim;
  unsigned k0, k1;
};

typedef float prec_acc_t __attribute__((ext_vector_type(4)));

// (two waves per SIMD as the register budget, as cov_snapshot_kernel: the accumulators then stay in VGPRs - the build gate admits
// no AGPRs)
__global__ void __launch_bounds__(kPrecThreads, 2) precond_propose_kernel(PrecondProposeArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_prec[];
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int D = a.dim, T = a.n_temps;
  const int B = prec_blocks(D);
  unsigned long long step = a.step;
  if (a.device_step != nullptr) step += (unsigned long long)*a.device_step;
  {
    const int passes = prec_l_passes(D);
    for (int p = 0; p < passes; ++p) {
      const int i = prec_l_stage_i(p, tid), k = prec_l_stage_k(p, tid);
      s_prec[prec_l_at(i, k, D)] = prec_l_live(i, k, D) ? a.chol[i * D + k] : 0.0f;
    }
  }
  const long long n_tiles = (a.n_reps + kPrecRows - 1) / kPrecRows;
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long first = tile * kPrecRows;
    const int n_rows = (a.n_reps - first < kPrecRows) ? (int)(a.n_reps - first) : kPrecRows;
    const int total = n_rows * D;
    float *__restrict__ gx = const_cast<float *>(a.state) + first * D;
    float *__restrict__ gy = a.proposals + first * D;
    float *const xs = s_prec + prec_x_offset(D);
    const int head = stage_head(gy);
    __syncthreads();  // (the previous tile's copy out has read the slab)
    // the states land where the proposals leave from: in vectors where the two runs are aligned alike, else one by one
    if (stage_head(gx) == head) stage_copy<true>(xs, gx, total, tid, kPrecThreads);
    else
      for (int e = tid; e < total; e += kPrecThreads) xs[head + e] = gx[e];
    // the normals: item e is Philox block c of row r
    const int n_items = prec_z_items(D), c_acc = prec_accept_word(D) / 4, nb = prec_philox_blocks(D);
    for (int e = tid; e < n_items; e += kPrecThreads) {
      const int r = prec_z_item_row(e), c = prec_z_item_block(e);
      if (r >= n_rows) continue;
      const long long i = first + r;
      float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      if (a.ext_raw != nullptr) {
        const float *er = a.ext_raw + i * D;
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (4 * c + q < D) z[q] = er[4 * c + q];
        if (c == c_acc) a.accept_u[i] = a.ext_u[i];
      } else if (c < nb) {
        const long long chain = i / T;
        const int t = (int)(i - chain * T);
        const unsigned long long gchain = (unsigned long long)(a.chain_offset + chain);
        const u32x4 rr = philox4x32_10(step_word_c0hi(step) | (uint32_t)c, step_word_c1(step), chain_word_c2(gchain),
                                       with_stream(chain_word_c3(gchain, (uint32_t)t), kStreamMH), a.k0, a.k1);
        if (4 * c < D) box_muller(rr.x, rr.y, z[0], z[1]);
        if (4 * c + 2 < D) box_muller(rr.z, rr.w, z[2], z[3]);
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (4 * c + q >= D) z[q] = 0.0f;
        if (c == c_acc) a.accept_u[i] = u01((prec_accept_word(D) & 2) ? rr.z : rr.x);
      }
      if (prec_z_written(c, D)) {
        float *zr = s_prec + prec_z_at(r, 4 * c, D);
#pragma unroll
        for (int q = 0; q < 4; ++q) zr[q] = z[q];
      }
      if (c == c_acc) a.accept_u[a.n_reps + i] = -1.0f;  // the squared jump is taken from the states
    }
    __syncthreads();
    // wave w: rows 16 w .. 16 w + 15, block rows bi and bi + 1 together
    if (kPrecBlock * w < n_rows) {
      const int row = prec_acc_row(w, lane);
      const long long ir = first + (row < n_rows ? row : 0);
      const float s_t = a.temp_scale[(int)(ir % T)];
      const float *zb = s_prec + prec_z_at(prec_b_row(w, lane), prec_operand_k(0, lane), D);
      for (int bi = 0; bi < B; bi += 2) {
        const bool two = bi + 1 < B;
        const float *la0 = s_prec + prec_l_at(prec_a_row(bi, lane), prec_operand_k(0, lane), D);
        const float *la1 = s_prec + prec_l_at(prec_a_row(two ? bi + 1 : bi, lane), prec_operand_k(0, lane), D);
        prec_acc_t acc0 = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = {0.0f, 0.0f, 0.0f, 0.0f};
        const int ks0 = prec_ksteps(bi);
        for (int ks = 0; ks < ks0; ++ks) {
          const float zv = zb[kPrecK * ks];
          acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(la0[kPrecK * ks], zv, acc0, 0, 0, 0);
          if (two) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(la1[kPrecK * ks], zv, acc1, 0, 0, 0);
        }
        if (two)
          for (int ks = ks0; ks < prec_ksteps(bi + 1); ++ks)
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(la1[kPrecK * ks], zb[kPrecK * ks], acc1, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int d0 = prec_acc_dim(bi, lane, r), d1 = prec_acc_dim(bi + 1, lane, r);
          if (prec_acc_live(row, d0, n_rows, D)) {
            float *px = s_prec + prec_x_at(head, row, d0, D);
            *px = fmaf(s_t, acc0[r], *px);
          }
          if (two && prec_acc_live(row, d1, n_rows, D)) {
            float *px = s_prec + prec_x_at(head, row, d1, D);
            *px = fmaf(s_t, acc1[r], *px);
          }
        }
      }
    }
    __syncthreads();
    stage_copy<false>(xs, gy, total, tid, kPrecThreads);
  }
}

// The update of the factor from one window's sums (precond.h): one workgroup, thread i owns row i, the work matrix is the packed
// lower triangle in LDS, every inner product runs over k ascending - the result is the host function's, bit for bit.
struct PrecondUpdateArgs {
  float *chol;
  double *sxx, *sx;
  long long *count;
  double *run_xx, *run_x, *run_w;
  float *chol_history;     // [K + 1, dim, dim] or NULL
  double *weight_history;  // [K] or NULL
  long long *skipped;      // [1] or NULL
  double memory, jitter, min_count;
  long long window;
  int dim;
};

__global__ void __launch_bounds__(kPrecUpdateThreads) precond_update_kernel(PrecondUpdateArgs a) {
  extern __shared__ double s_upd[];  // A: prec_tri_size(dim), then m: dim
  __shared__ double s_piv, s_w;
  __shared__ int s_fail;
  const int i = (int)threadIdx.x, D = a.dim;
  double *const A = s_upd, *const m = s_upd + prec_tri_size(D);
  const bool mine = i < D;
  if (i == 0) s_fail = 0;
  // history row 0: the factor the first window ran with
  if (a.chol_history != nullptr && a.window == 0 && mine)
    for (int j = 0; j < D; ++j) a.chol_history[i * D + j] = j <= i ? a.chol[i * D + j] : 0.0f;
  if (mine) {
    for (int j = 0; j <= i; ++j) {
      a.run_xx[i * D + j] = prec_decay_add(a.memory, a.run_xx[i * D + j], a.sxx[i * D + j]);
      a.sxx[i * D + j] = 0.0;
    }
    a.run_x[i] = prec_decay_add(a.memory, a.run_x[i], a.sx[i]);
    a.sx[i] = 0.0;
  }
  if (i == 0) {
    const double wn = prec_decay_add(a.memory, *a.run_w, (double)*a.count);
    *a.run_w = wn;
    *a.count = 0;
    s_w = wn;
    if (a.weight_history != nullptr) a.weight_history[a.window] = wn;
  }
  __syncthreads();
  const double wt = s_w;
  bool ok = prec_weight_ok(wt, a.min_count);  // (workgroup-uniform)
  if (ok) {
    if (mine) m[i] = a.run_x[i] / wt;
    __syncthreads();
    if (mine)
      for (int j = 0; j <= i; ++j) A[prec_tri(i, j)] = prec_centered(a.run_xx[i * D + j], wt, m[i], m[j]);
    __syncthreads();
    double tr = 0.0;
    for (int k = 0; k < D; ++k) tr = tr + A[prec_tri(k, k)];
    __syncthreads();
    if (mine) A[prec_tri(i, i)] = A[prec_tri(i, i)] + prec_jitter_term(a.jitter, tr, D);
    __syncthreads();
    for (int j = 0; j < D; ++j) {
      double s = 0.0;
      if (mine && i >= j) {
        s = A[prec_tri(i, j)];
        for (int k = 0; k < j; ++k) s = prec_sub_prod(s, A[prec_tri(i, k)], A[prec_tri(j, k)]);
        if (i == j) {
          if (prec_pivot_ok(s)) s_piv = sqrt(s);
          else s_fail = 1;
        }
      }
      __syncthreads();
      if (s_fail != 0) break;  // (workgroup-uniform)
      if (mine && i >= j) A[prec_tri(i, j)] = i == j ? s_piv : s / s_piv;
      __syncthreads();
    }
    if (s_fail == 0 && mine)
      for (int j = 0; j <= i; ++j)
        if (!prec_finite((double)(float)A[prec_tri(i, j)])) s_fail = 1;
    __syncthreads();
    ok = s_fail == 0;
  }
  if (ok && mine)
    for (int j = 0; j <= i; ++j) a.chol[i * D + j] = (float)A[prec_tri(i, j)];
  if (!ok && i == 0 && a.skipped != nullptr) *a.skipped += 1;
  // history row window + 1: the factor in force behind this window (a thread reads back its own row)
  if (a.chol_history != nullptr && mine)
    for (int j = 0; j < D; ++j) a.chol_history[((a.window + 1) * D + i) * D + j] = j <= i ? a.chol[i * D + j] : 0.0f;
}

// ---- warm-up tuning of the proposal scale (adapt.h; include/ptrwm.h ptrwm_adapt_args) ---------------------------------------
// Two small kernels between launches, as the histogram's snapshot: the step kernels are told nothing.  A launch inside an
// adapting window adds its acceptances to window_accept [n_chains, n_temps]; at the window's end adapt_reduce_kernel sums
// that scratch over chains into pooled[t], adds the window's chain-steps to pooled[n_temps] and leaves the scratch zero;
// adapt_update_kernel then applies adapt.h's rule to temp_scale, which the next launch reads when it starts.
//
// Reduce: a workgroup takes a tile of whole chains, about kAdaptTileElems elements - one contiguous run of the scratch that
// starts at a chain, so element e of the tile belongs to temperature e % n_temps whatever n_temps is.  The run is read and
// zeroed in 16-byte vectors (two counters; an element in front of the first 16-byte boundary and one behind the last vector
// are taken on their own).  A thread keeps the sum of a temperature in a register for as long as its elements stay on it
// (its stride is 512 elements: for ever where n_temps divides 512) and adds it to the workgroup's 64-bit LDS counter of
// that temperature when they move on; one 64-bit global atomic per non-zero (workgroup, temperature) flushes.  All integer:
// exact, whatever the order.
constexpr int kAdaptTileElems = 4096;
struct AdaptReduceArgs {
  long long *window_accept;  // [n_chains, n_temps]
  long long *pooled;         // [n_temps + 1]
  long long n_chains, every;
  int n_temps, tile_chains;  // tile_chains = max(1, kAdaptTileElems / n_temps)
};
inline int adapt_tile_chains(int n_temps) { return kAdaptTileElems / n_temps > 1 ? kAdaptTileElems / n_temps : 1; }

__global__ void __launch_bounds__(256) adapt_reduce_kernel(AdaptReduceArgs a) {
  typedef long long ll2 __attribute__((ext_vector_type(2)));
  __shared__ unsigned long long s_sum[PTRWM_MAX_TEMPS];
  const int tid = (int)threadIdx.x, T = a.n_temps;
  for (int t = tid; t < T; t += 256) s_sum[t] = 0ull;
  __syncthreads();
  const long long c0 = (long long)blockIdx.x * a.tile_chains;
  const long long c1 = (a.n_chains - c0 < a.tile_chains) ? a.n_chains : c0 + a.tile_chains;
  const int n = (int)((c1 - c0) * T);  // the tile's elements (1 .. tile_chains * n_temps <= kAdaptTileElems)
  long long *const p = a.window_accept + c0 * T;
  const int head = (reinterpret_cast<uintptr_t>(p) & 15u) != 0 ? 1 : 0;  // (counters are 8-byte aligned)
  const int n_vec = (n - head) / 2;
  const auto add = [&](int t, long long v) {
    if (v != 0) atomicAdd(&s_sum[t], (unsigned long long)v);
  };
  ll2 *const pv = reinterpret_cast<ll2 *>(p + head);
  int cur0 = 0, cur1 = 0;
  long long acc0 = 0, acc1 = 0;
  for (int v = tid; v < n_vec; v += 256) {
    const ll2 x = pv[v];
    pv[v] = ll2{0ll, 0ll};
    const int t0 = (head + 2 * v) % T;
    const int t1 = t0 + 1 == T ? 0 : t0 + 1;
    if (t0 != cur0) add(cur0, acc0), cur0 = t0, acc0 = 0;
    if (t1 != cur1) add(cur1, acc1), cur1 = t1, acc1 = 0;
    acc0 += x.x;
    acc1 += x.y;
  }
  add(cur0, acc0);
  add(cur1, acc1);
  if (tid == 0 && head != 0) {  // the element in front of the vectors: the tile's first, temperature 0
    add(0, p[0]);
    p[0] = 0;
  }
  const int tail = head + 2 * n_vec;  // the element behind them, if any
  if (tid == 64 && tail < n) {
    add(tail % T, p[tail]);
    p[tail] = 0;
  }
  __syncthreads();
  for (int t = tid; t < T; t += 256) {
    const unsigned long long v = s_sum[t];
    if (v != 0ull) count_add(&a.pooled[t], (long long)v);
  }
  if (tid == 0) count_add(&a.pooled[T], (c1 - c0) * a.every);
}

// Update: one workgroup, thread t < n_temps.  Every thread reads what it needs of `pooled` before any of it is zeroed.
struct AdaptUpdateArgs {
  float *temp_scale;          // [n_temps] in/out
  long long *pooled;          // [n_temps + 1], zeroed
  float *scale_history;       // [K + 1, n_temps] or NULL
  long long *accept_history;  // [K, n_temps] or NULL
  long long window;           // k (0 <= k < K: checked on the host)
  double gain_k, target;
  float min_scale, max_scale;
  int n_temps;
};

__global__ void __launch_bounds__(256) adapt_update_kernel(AdaptUpdateArgs a) {
  const int t = (int)threadIdx.x, T = a.n_temps;
  long long accepted = 0, counted = 0;
  if (t < T) {
    accepted = a.pooled[t];
    counted = a.pooled[T];
  }
  __syncthreads();
  if (t < T) {
    const float s_old = a.temp_scale[t];
    const float s_new = adapt_update(s_old, accepted, counted, a.gain_k, a.target, a.min_scale, a.max_scale);
    a.temp_scale[t] = s_new;
    if (a.scale_history != nullptr) {
      if (a.window == 0) a.scale_history[t] = s_old;
      a.scale_history[(a.window + 1) * T + t] = s_new;
    }
    if (a.accept_history != nullptr) a.accept_history[a.window * T + t] = accepted;
    a.pooled[t] = 0;
  }
  if (t == 0) a.pooled[T] = 0;
}

// ---- warm-up tuning of the temperature ladder (ladder.h; include/ptrwm.h ptrwm_ladder_args) -------------------------------------
// Two more small kernels between launches; the step kernels are told nothing.  Behind every probe step ladder_probe_kernel
// reads logp and beta and adds, per pair, the quantised probability with which the pair would swap to pooled[t]; at a window's
// end ladder_update_kernel applies ladder.h's rule to beta (and temp_scale), which the next launch reads when it starts.
//
// Probe: tiled as adapt_reduce_kernel - a workgroup takes a tile of whole chains, about kAdaptTileElems elements of logp, one
// contiguous run that starts at a chain, so element e of the tile is temperature e % n_temps.  Thread i takes elements i,
// i + 256, ...: consecutive lanes read consecutive floats (and their right-hand neighbours, the same cache lines).  Element e
// with t < n_temps - 1 is the pair (t, t + 1) of its chain; the last element of a chain is no pair.  A thread keeps a pair's
// sum in a register for as long as its elements stay on that pair (for ever where n_temps divides 256) and adds it to the
// workgroup's 64-bit LDS counter of the pair when they move on; one 64-bit global atomic per non-zero (workgroup, pair)
// flushes, and one adds the tile's chains to pooled[n_temps - 1].  All integer: exact, whatever the order.
struct LadderProbeArgs {
  const float *logp;   // [n_chains, n_temps]
  const float *beta;   // [n_temps]
  long long *pooled;   // [n_temps]
  long long n_chains;
  int n_temps, tile_chains;  // tile_chains = adapt_tile_chains(n_temps)
};

__global__ void __launch_bounds__(256) ladder_probe_kernel(LadderProbeArgs a) {
  __shared__ unsigned long long s_sum[PTRWM_MAX_TEMPS];
  __shared__ float s_beta[PTRWM_MAX_TEMPS];
  const int tid = (int)threadIdx.x, T = a.n_temps;
  for (int t = tid; t < T; t += 256) s_sum[t] = 0ull, s_beta[t] = a.beta[t];
  __syncthreads();
  const long long c0 = (long long)blockIdx.x * a.tile_chains;
  const long long c1 = (a.n_chains - c0 < a.tile_chains) ? a.n_chains : c0 + a.tile_chains;
  const int n = (int)((c1 - c0) * T);  // the tile's elements (1 .. tile_chains * n_temps <= max(kAdaptTileElems, n_temps))
  const float *const p = a.logp + c0 * T;
  int cur = 0;
  long long acc = 0;
  for (int e = tid; e < n; e += 256) {
    const int t = e % T;
    if (t == T - 1) continue;  // (e + 1 < n: the pair's upper rung is in the same chain)
    if (t != cur) {
      if (acc != 0) atomicAdd(&s_sum[cur], (unsigned long long)acc);
      cur = t, acc = 0;
    }
    const float lp = swap_log_prob(s_beta[t], s_beta[t + 1], p[e], p[e + 1]);
    const float thr = (lp >= 0.0f) ? 1.0f : hw_exp(lp);  // the threshold of swap_accept_test
    acc += ladder_quantum(thr);
  }
  if (acc != 0) atomicAdd(&s_sum[cur], (unsigned long long)acc);
  __syncthreads();
  for (int t = tid; t < T - 1; t += 256) {
    const unsigned long long v = s_sum[t];
    if (v != 0ull) count_add(&a.pooled[t], (long long)v);
  }
  if (tid == 0) count_add(&a.pooled[T - 1], c1 - c0);
}

// Update: one workgroup.  Thread 0 runs ladder.h's sequential rule into LDS; behind the barrier thread t < n_temps writes its
// beta, its scale and the histories, and zeroes its counter (which only thread 0 read before the barrier, and itself after).
struct LadderUpdateArgs {
  float *beta;              // [n_temps] in/out
  float *temp_scale;        // [n_temps] in/out, or NULL (rescale_scales = 0)
  long long *pooled;        // [n_temps], zeroed
  float *beta_history;      // [K + 1, n_temps] or NULL
  long long *rate_history;  // [K, n_temps] or NULL
  long long *skipped;       // [1] or NULL
  long long window;         // j (0 <= j < K: checked on the host)
  double gain_j;
  int n_temps;
};

__global__ void __launch_bounds__(256) ladder_update_kernel(LadderUpdateArgs a) {
  __shared__ float s_old[PTRWM_MAX_TEMPS], s_new[PTRWM_MAX_TEMPS];
  __shared__ long long s_pooled[PTRWM_MAX_TEMPS];
  __shared__ double s_work[PTRWM_MAX_TEMPS];
  const int t = (int)threadIdx.x, T = a.n_temps;
  if (t < T) s_old[t] = a.beta[t], s_pooled[t] = a.pooled[t];
  __syncthreads();
  if (t == 0) {
    const int outcome = ladder_update(s_old, s_pooled, T, a.gain_j, s_new, s_work);
    if (outcome == kLadderSkipped && a.skipped != nullptr) *a.skipped += 1;
  }
  __syncthreads();
  if (t < T) {
    const float b_old = s_old[t], b_new = s_new[t];
    a.beta[t] = b_new;
    if (a.temp_scale != nullptr && t > 0 && t < T - 1) a.temp_scale[t] = ladder_rescale(a.temp_scale[t], b_old, b_new);
    if (a.beta_history != nullptr) {
      if (a.window == 0) a.beta_history[t] = b_old;
      a.beta_history[(a.window + 1) * T + t] = b_new;
    }
    if (a.rate_history != nullptr) a.rate_history[a.window * T + t] = s_pooled[t];
    a.pooled[t] = 0;
  }
}

// Starting points (ptrwm_init_states): row (c, t) of `state` drawn uniformly from the box [lo, hi], or set to `fallback`.
// The draw is Philox stream kStreamInit (rng_layout.h: the counter layout; include/ptrwm.h restates it), keyed by the GLOBAL chain
// id like every other random of a run, so the starts do not depend on how chains are sharded over devices.
struct InitStatesArgs {
  void *state;                             // float (or double, F64) [n_reps, dim]
  const float *logp, *lo, *hi, *fallback;  // logp: read when attempt > 0 only; fallback: NULL = draw
  long long n_reps, chain_offset;
  int n_temps, dim, per_temperature, attempt;
  unsigned k0, k1;
};

// One wavefront per tile of 64 rows (64-thread workgroups), as the split-step kernels: every lane builds its own row in a
// slab of LDS and the tile's run of 64 x dim floats leaves through stage_copy (coalesced 16-byte stores whatever the run's
// alignment); double states are written element by element, consecutive lanes to consecutive doubles.
// attempt > 0 rewrites only the rows whose log-density is not finite: a tile without one exits before it touches `state`;
// a float tile with some stages itself in first, so that the rows it keeps go back bit for bit; a double tile stores
// the rewritten rows only.
template <bool F64>
__global__ void __launch_bounds__(64) init_states_kernel(InitStatesArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_init[];
  const int lane = (int)threadIdx.x;
  const long long first = (long long)blockIdx.x * 64;
  if (first >= a.n_reps) return;
  const int D = a.dim;
  const int n_rows = (a.n_reps - first < 64) ? (int)(a.n_reps - first) : 64;
  const bool live = lane < n_rows;
  const long long i = first + (live ? lane : 0);
  bool mine = live;
  if (a.attempt > 0) mine = live && (__float_as_uint(a.logp[i]) & 0x7f800000u) == 0x7f800000u;  // NaN, +inf or -inf
  const unsigned long long todo = __ballot(mine);
  if (todo == 0ull) return;  // (wave-uniform)
  const unsigned long long all = n_rows == 64 ? ~0ull : (1ull << n_rows) - 1ull;
  float *__restrict__ gf = reinterpret_cast<float *>(a.state) + first * D;  // (float states)
  const int head = F64 ? 0 : stage_head(gf);
  if (!F64 && todo != all) {
    stage_copy<true>(s_init, gf, n_rows * D, lane, 64);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  if (mine) {
    float *__restrict__ row = s_init + head + lane * D;
    if (a.fallback != nullptr) {
      const const_float_ptr fb = uniform_vec(a.fallback);
      for (int d = 0; d < D; ++d) row[d] = fb[d];
    } else {
      const const_float_ptr lo = uniform_vec(a.lo), hi = uniform_vec(a.hi);
      const long long chain = i / a.n_temps;
      const unsigned long long g = (unsigned long long)(a.chain_offset + chain);
      const uint32_t c2 = chain_word_c2(g), c3 = init_word_c3(g, (uint32_t)(i - chain * a.n_temps), a.per_temperature != 0);  // (stream 3: rng_layout.h)
      for (int b = 0; 4 * b < D; ++b) {
        const u32x4 r = philox4x32_10(init_word_c0(4 * b, a.attempt), 0u, c2, c3, a.k0, a.k1);  // word k: coordinate 4 b + k
        const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int d = 4 * b + k;
          if (d < D) row[d] = add_rn(lo[d], mul_rn(sub_rn(hi[d], lo[d]), u01(w[k])));
        }
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  if (!F64) {
    stage_copy<false>(s_init, gf, n_rows * D, lane, 64);
  } else {
    double *__restrict__ gd = reinterpret_cast<double *>(a.state) + first * D;
    const int total = n_rows * D;
    for (int e = lane; e < total; e += 64)
      if ((todo >> (e / D)) & 1ull) gd[e] = (double)s_init[e];
  }
}

}  // namespace ptrwm

using namespace ptrwm;

// The two public accumulator structs are one layout: ptrwm_moments_args is the view through which both are checked and read,
// and a MomSpec says which kind it holds (m == NULL: none).
#define PTRWM_SAME_FIELD(f) \
  (offsetof(ptrwm_moments_args, f) == offsetof(ptrwm_chain_moments_args, f) && sizeof(ptrwm_moments_args::f) == sizeof(ptrwm_chain_moments_args::f))
static_assert(sizeof(ptrwm_moments_args) == sizeof(ptrwm_chain_moments_args) && PTRWM_SAME_FIELD(struct_size) && PTRWM_SAME_FIELD(temps) &&
                  PTRWM_SAME_FIELD(every) && PTRWM_SAME_FIELD(sum) && PTRWM_SAME_FIELD(sum_sq) && PTRWM_SAME_FIELD(sum_logp) && PTRWM_SAME_FIELD(count),
              "ptrwm_moments_args and ptrwm_chain_moments_args: the same fields at the same offsets");
#undef PTRWM_SAME_FIELD
struct MomSpec {
  const ptrwm_moments_args *m;
  bool per_chain;
  MomSpec() : m(nullptr), per_chain(false) {}
  MomSpec(const ptrwm_moments_args *pooled) : m(pooled), per_chain(false) {}
  MomSpec(const ptrwm_chain_moments_args *chain) : m(reinterpret_cast<const ptrwm_moments_args *>(chain)), per_chain(true) {}
};

// the accumulator checks shared by ptrwm_run_with_*moments and ptrwm_split_*moments (args already checked); none: ok
static int32_t check_moments(const ptrwm_run_args *args, const MomSpec &mom) {
  const ptrwm_moments_args *const m = mom.m;
  if (m == nullptr) return PTRWM_OK;
  if (m->struct_size != sizeof(ptrwm_moments_args)) return PTRWM_E_STRUCT;
  if (m->temps < 1 || m->temps > args->n_temps || m->every < 1) return PTRWM_E_ARG;
  if (m->sum == nullptr || m->sum_sq == nullptr) return PTRWM_E_NULL;
  return PTRWM_OK;
}

// the flow checks shared by the three entry points that take ptrwm_flow_args (args already checked); none: ok
static int32_t check_flow(const ptrwm_run_args *args, const ptrwm_flow_args *flow) {
  if (flow == nullptr) return PTRWM_OK;
  if (flow->struct_size != sizeof(ptrwm_flow_args)) return PTRWM_E_STRUCT;
  if (flow->walker == nullptr) return PTRWM_E_NULL;
  if (args->n_temps < 2 || flow->reserved != 0) return PTRWM_E_ARG;
  return PTRWM_OK;
}

// what the three snapshot blocks' checks open with: the struct's size, then the covered temperatures and the period
template <class Block>
static int32_t check_snapshot_block(const ptrwm_run_args *args, const Block *b) {
  if (b->struct_size != sizeof(Block)) return PTRWM_E_STRUCT;
  if (b->temps < 1 || b->temps > args->n_temps || b->every < 1) return PTRWM_E_ARG;
  return PTRWM_OK;
}

// the histogram checks shared by ptrwm_run_with_histogram and ptrwm_histogram (args already checked); none: ok
static int32_t check_hist(const ptrwm_run_args *args, const ptrwm_hist_args *h) {
  if (h == nullptr) return PTRWM_OK;
  if (int rc = check_snapshot_block(args, h)) return rc;
  if (h->n_bins < 1 || h->n_bins > PTRWM_HIST_MAX_BINS) return PTRWM_E_ARG;
  if (h->lo == nullptr || h->scale == nullptr || h->counts == nullptr) return PTRWM_E_NULL;
  return PTRWM_OK;
}
static_assert(PTRWM_HIST_MAX_BINS == kHistMaxBins, "hist.h and include/ptrwm.h: one bin limit");

// One snapshot of the state after step `step` (device_step != NULL: *device_step + step); everything checked
static int32_t launch_hist(const ptrwm_run_args *args, int32_t dim, const ptrwm_hist_args *h, long long step,
                           const long long *device_step, hipStream_t stream) {
  HistSnapArgs a;
  fill_snap_head(a, args, dim, h->every, step, device_step);
  a.own = {h->lo, h->scale, (long long *)h->counts, (long long *)h->count};
  a.temps = h->temps;
  a.n_bins = h->n_bins;
  const HistGeometry g = hist_geometry(h->n_bins, h->temps * dim);
  a.direct = g.direct;
  a.cols = g.cols;
  const long long gx = (args->n_chains + kHistChains - 1) / kHistChains;
  return launch_snapshot(hist_snapshot_kernel<float>, hist_snapshot_kernel<double>, args->state_f64 == 1, gx, (unsigned)g.groups /* <= 256 * 104 / 64 */,
                         256, 0, stream, a);
}

// the autocovariance checks shared by ptrwm_run_with_autocorr and ptrwm_autocorr (args already checked); none: ok
static int32_t check_acf(const ptrwm_run_args *args, const ptrwm_acf_args *ac) {
  if (ac == nullptr) return PTRWM_OK;
  if (int rc = check_snapshot_block(args, ac)) return rc;
  if (ac->max_lag < 1 || ac->max_lag > PTRWM_ACF_MAX_LAG) return PTRWM_E_ARG;
  if (ac->ring == nullptr || ac->sxy == nullptr || ac->head == nullptr || ac->tail == nullptr || ac->pairs == nullptr) return PTRWM_E_NULL;
  return PTRWM_OK;
}
static_assert(PTRWM_ACF_MAX_LAG == kAcfMaxLag, "acf.h and include/ptrwm.h: one lag limit");

// One snapshot of the state after step `step` (device_step != NULL: *device_step + step); everything checked
static int32_t launch_acf(const ptrwm_run_args *args, int32_t dim, const ptrwm_acf_args *ac, long long step,
                          const long long *device_step, hipStream_t stream) {
  AcfSnapArgs a;
  fill_snap_head(a, args, dim, ac->every, step, device_step);
  a.own = {ac->ring, ac->sxy, ac->head, ac->tail, (long long *)ac->pairs};
  a.temps = ac->temps;
  a.max_lag = ac->max_lag;
  const AcfGeometry g = acf_geometry(ac->temps * dim);
  a.cols = g.cols;
  a.per = g.per;
  a.chains = g.chains;
  const long long gx = (args->n_chains + g.chains - 1) / g.chains;
  return launch_snapshot(acf_snapshot_kernel<float>, acf_snapshot_kernel<double>, args->state_f64 == 1, gx, (unsigned)g.groups /* <= 104 */,
                         kAcfThreads, 0, stream, a);
}

// the covariance checks shared by ptrwm_run_with_covariance and ptrwm_covariance (args already checked); none: ok
static int32_t check_cov(const ptrwm_run_args *args, const ptrwm_cov_args *cv) {
  if (cv == nullptr) return PTRWM_OK;
  if (int rc = check_snapshot_block(args, cv)) return rc;
  if (cv->sxx == nullptr || cv->sx == nullptr || cv->count == nullptr) return PTRWM_E_NULL;
  return PTRWM_OK;
}
static_assert(PTRWM_MAX_DIM == kCovMaxDim, "cov.h and include/ptrwm.h: one largest dim");

// One snapshot of the state after step `step` (device_step != NULL: *device_step + step); everything checked
static int32_t launch_cov(const ptrwm_run_args *args, int32_t dim, const ptrwm_cov_args *cv, long long step,
                          const long long *device_step, hipStream_t stream) {
  CovSnapArgs a;
  fill_snap_head(a, args, dim, cv->every, step, device_step);
  a.own = {cv->sxx, cv->sx, (long long *)cv->count};
  const CovGeometry g = cov_geometry(dim);
  const long long gx = (args->n_chains + g.chains - 1) / g.chains;
  return launch_snapshot(cov_snapshot_kernel<float>, cov_snapshot_kernel<double>, args->state_f64 == 1, gx, (unsigned)cv->temps /* <= 256 */,
                         kCovThreads, (size_t)g.lds_bytes, stream, a);
}

// the checks of the log-density sums shared by ptrwm_run_with_energy and ptrwm_energy (args already checked); none: ok
static int32_t check_energy(const ptrwm_run_args *args, const ptrwm_energy_args *en) {
  if (en == nullptr) return PTRWM_OK;
  if (en->struct_size != sizeof(ptrwm_energy_args)) return PTRWM_E_STRUCT;
  if (en->groups < 1 || en->groups > PTRWM_ENERGY_MAX_GROUPS || en->every < 1) return PTRWM_E_ARG;
  if (en->ref == nullptr || en->ref_set == nullptr || en->count == nullptr || en->s1 == nullptr || en->s2 == nullptr) return PTRWM_E_NULL;
  if (args->n_temps >= 2 && (en->colder == nullptr || en->hotter == nullptr)) return PTRWM_E_NULL;
  return PTRWM_OK;
}
static_assert(PTRWM_ENERGY_MAX_GROUPS == kEnergyMaxGroups && PTRWM_MAX_TEMPS == kEnergyMaxTemps, "energy.h and include/ptrwm.h: one set of limits");

// One snapshot of logp after step `step` (device_step != NULL: *device_step + step): the ref kernel, then the sums; everything
// checked, logp and beta there (`dim`: unused - the signature of the snapshot launchers, snapshot.h)
static int32_t launch_energy(const ptrwm_run_args *args, int32_t /*dim*/, const ptrwm_energy_args *en, long long step,
                             const long long *device_step, hipStream_t stream) {
  EnergySnapArgs a;
  a.logp = args->logp;
  a.beta = args->beta;
  a.ref = en->ref;
  a.ref_set = en->ref_set;
  a.count = (long long *)en->count;
  a.nonfinite = (long long *)en->nonfinite;
  a.s1 = en->s1, a.s2 = en->s2, a.colder = en->colder, a.hotter = en->hotter;
  a.n_chains = args->n_chains;
  a.chain_offset = args->chain_offset;
  a.step = step;
  a.burn_in = args->burn_in;
  a.every = en->every;
  a.device_step = device_step;
  a.n_temps = args->n_temps;
  a.groups = en->groups;
  const EnergyGeometry g = energy_geometry(args->n_temps, args->n_chains, args->chain_offset, en->groups);
  if (int rc = launch_snapshot(energy_ref_kernel, energy_ref_kernel, false, 1, 1u, kEnergyThreads, 0, stream, a)) return rc;
  return launch_snapshot(energy_snapshot_kernel, energy_snapshot_kernel, false, g.tiles, (unsigned)g.groups /* <= 64 */, kEnergyThreads, 0,
                         stream, a);
}

// the adaptation checks shared by ptrwm_run_with_adaptation, ptrwm_adapt_reduce and ptrwm_adapt_update (none: ok); what
// needs the run (until <= burn_in, temp_scale == proposal->temp_scale) is checked by run_impl itself (tuning_fits_run)
static int32_t check_tuning(const ptrwm_adapt_args *ad) {
  if (ad == nullptr) return PTRWM_OK;
  if (ad->struct_size != sizeof(ptrwm_adapt_args)) return PTRWM_E_STRUCT;
  if (ad->temp_scale == nullptr || ad->window_accept == nullptr || ad->pooled == nullptr) return PTRWM_E_NULL;
  if (ad->every < 1 || ad->until < 0) return PTRWM_E_ARG;
  if (!(ad->target > 0.0f && ad->target < 1.0f)) return PTRWM_E_ARG;
  if (!(ad->gain > 0.0f) || !std::isfinite(ad->gain)) return PTRWM_E_ARG;
  if (!(ad->decay >= 0.0f && ad->decay <= 1.0f)) return PTRWM_E_ARG;
  if (!(ad->min_scale > 0.0f && ad->min_scale <= ad->max_scale) || !std::isfinite(ad->max_scale)) return PTRWM_E_ARG;
  if (!is_flag(ad->defer_update)) return PTRWM_E_ARG;
  return PTRWM_OK;
}

// the window scratch of n_chains x n_temps summed into pooled and zeroed; everything checked, n_chains >= 1
static int32_t launch_adapt_reduce(const ptrwm_adapt_args *ad, long long n_chains, int n_temps, hipStream_t stream) {
  AdaptReduceArgs a;
  a.window_accept = (long long *)ad->window_accept;
  a.pooled = (long long *)ad->pooled;
  a.n_chains = n_chains;
  a.every = ad->every;
  a.n_temps = n_temps;
  a.tile_chains = adapt_tile_chains(n_temps);
  const long long blocks = (n_chains + a.tile_chains - 1) / a.tile_chains;
  if (blocks > 0x7fffffffll) return PTRWM_E_ARG;
  hipLaunchKernelGGL(adapt_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? PTRWM_OK : PTRWM_E_LAUNCH;
}

// the update of window k (0 <= k < K); everything checked
static int32_t launch_adapt_update(const ptrwm_adapt_args *ad, int n_temps, long long window, hipStream_t stream) {
  AdaptUpdateArgs a;
  a.temp_scale = ad->temp_scale;
  a.pooled = (long long *)ad->pooled;
  a.scale_history = ad->scale_history;
  a.accept_history = (long long *)ad->accept_history;
  a.window = window;
  a.gain_k = window_gain((double)ad->gain, (double)ad->decay, window);
  a.target = (double)ad->target;
  a.min_scale = ad->min_scale;
  a.max_scale = ad->max_scale;
  a.n_temps = n_temps;
  hipLaunchKernelGGL(adapt_update_kernel, dim3(1), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? PTRWM_OK : PTRWM_E_LAUNCH;
}
static_assert(PTRWM_MAX_TEMPS <= 256, "adapt_update_kernel: one thread per temperature in one 256-thread workgroup");

// the ladder checks shared by ptrwm_run_with_ladder, ptrwm_ladder_probe and ptrwm_ladder_update (none: ok); what needs the run
// (until <= burn_in, the pointer identities, n_temps) is checked by the callers
static int32_t check_tuning(const ptrwm_ladder_args *ld) {
  if (ld == nullptr) return PTRWM_OK;
  if (ld->struct_size != sizeof(ptrwm_ladder_args)) return PTRWM_E_STRUCT;
  if (ld->beta == nullptr || ld->pooled == nullptr || (ld->rescale_scales == 1 && ld->temp_scale == nullptr)) return PTRWM_E_NULL;
  if (!is_flag(ld->rescale_scales) || !is_flag(ld->defer_update)) return PTRWM_E_ARG;
  if (ld->every < 1 || ld->probe_every < 1 || ld->every % ld->probe_every != 0 || ld->until < 0) return PTRWM_E_ARG;
  if (!(ld->gain > 0.0f) || !std::isfinite(ld->gain)) return PTRWM_E_ARG;
  if (!(ld->decay >= 0.0f && ld->decay <= 1.0f)) return PTRWM_E_ARG;
  return PTRWM_OK;
}

// one probe of n_chains x n_temps log-densities added to pooled; everything checked, n_chains >= 1, n_temps >= 3
static int32_t launch_ladder_probe(const ptrwm_ladder_args *ld, const float *logp, long long n_chains, int n_temps, hipStream_t stream) {
  LadderProbeArgs a;
  a.logp = logp;
  a.beta = ld->beta;
  a.pooled = (long long *)ld->pooled;
  a.n_chains = n_chains;
  a.n_temps = n_temps;
  a.tile_chains = adapt_tile_chains(n_temps);
  const long long blocks = (n_chains + a.tile_chains - 1) / a.tile_chains;
  if (blocks > 0x7fffffffll) return PTRWM_E_ARG;
  hipLaunchKernelGGL(ladder_probe_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? PTRWM_OK : PTRWM_E_LAUNCH;
}

// the update of window j (0 <= j < K); everything checked
static int32_t launch_ladder_update(const ptrwm_ladder_args *ld, int n_temps, long long window, hipStream_t stream) {
  LadderUpdateArgs a;
  a.beta = ld->beta;
  a.temp_scale = ld->rescale_scales == 1 ? ld->temp_scale : nullptr;
  a.pooled = (long long *)ld->pooled;
  a.beta_history = ld->beta_history;
  a.rate_history = (long long *)ld->rate_history;
  a.skipped = (long long *)ld->skipped;
  a.window = window;
  a.gain_j = window_gain((double)ld->gain, (double)ld->decay, window);
  a.n_temps = n_temps;
  hipLaunchKernelGGL(ladder_update_kernel, dim3(1), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? PTRWM_OK : PTRWM_E_LAUNCH;
}
static_assert(PTRWM_MAX_TEMPS <= 256, "ladder_update_kernel: one thread per temperature in one 256-thread workgroup");

// What the four stand-alone calls of the two tunings check first.  The calls between launches (ptrwm_adapt_reduce,
// ptrwm_ladder_probe) take the run's arguments; the updates take n_temps and the window, one of the K the histories have rows for.
template <class Tuning>
static int32_t check_tuning_call(const Tuning *tu, bool per_run, const ptrwm_run_args *args, int32_t n_temps, int64_t window) {
  if (tu == nullptr || (per_run && args == nullptr)) return PTRWM_E_NULL;
  if (per_run && !has_abi_size(args)) return PTRWM_E_STRUCT;
  if (!temps_in_range(per_run ? args->n_temps : n_temps)) return PTRWM_E_TEMPS;
  if (per_run && args->n_chains < 0) return PTRWM_E_ARG;
  if (int rc = check_tuning(tu)) return rc;
  if (!per_run && (window < 0 || window >= window_count({tu->every, tu->until}))) return PTRWM_E_ARG;
  return PTRWM_OK;
}

// What a tuning asks of the run it is bound to (tu != nullptr, its own checks passed): windows that end within burn-in, the
// run's own array (the scale's temp_scale, the ladder's beta), and - where the caller applies the update between requests
// (defer_update) - no request that steps past a window end that awaits it
template <class Tuning>
static bool tuning_fits_run(const Tuning *tu, const ptrwm_run_args *args, const void *tuned, const void *of_run) {
  return tu->until <= args->burn_in && tuned == of_run &&
         (tu->defer_update == 0 || request_within_window({tu->every, tu->until}, args->step0, args->n_steps));
}

// The optional blocks of a run (NULL / no moments: off), in the order the ptrwm_run_with_* entry points grew them
struct RunBlocks {
  MomSpec spec;
  const ptrwm_flow_args *flow = nullptr;
  const ptrwm_hist_args *hist = nullptr;
  const ptrwm_adapt_args *adapt = nullptr;
  const ptrwm_ladder_args *ladder = nullptr;
  const ptrwm_acf_args *acf = nullptr;
  const ptrwm_cov_args *cov = nullptr;
  const ptrwm_energy_args *energy = nullptr;
};
static int32_t run_impl(const ptrwm_target_desc *target, const ptrwm_proposal_desc *proposal, const ptrwm_run_args *args,
                        const RunBlocks &blocks, void *hip_stream);
// ... as the entry points that take both kinds of moments hand them over: one accumulator, pooled or per chain
static int32_t run_with_blocks(const ptrwm_target_desc *target, const ptrwm_proposal_desc *proposal, const ptrwm_run_args *args,
                               const ptrwm_moments_args *moments, const ptrwm_chain_moments_args *chain_moments, RunBlocks blocks,
                               void *stream) {
  if (moments != nullptr && chain_moments != nullptr) return PTRWM_E_ARG;
  blocks.spec = chain_moments != nullptr ? MomSpec(chain_moments) : MomSpec(moments);
  return run_impl(target, proposal, args, blocks, stream);
}
// ptrwm_histogram, ptrwm_autocorr, ptrwm_covariance: one snapshot of `state` if the step just performed is due (Check: the
// block's check_*, Launch: its launch_*)
template <auto Check, auto Launch, class Block>
static int32_t snapshot_call(const ptrwm_run_args *args, int32_t dim, const Block *block, void *stream) {
  if (args == nullptr || block == nullptr) return PTRWM_E_NULL;
  if (!has_abi_size(args)) return PTRWM_E_STRUCT;
  if (dim < 1 || dim > PTRWM_MAX_DIM) return PTRWM_E_DIM;
  if (!temps_in_range(args->n_temps)) return PTRWM_E_TEMPS;
  if (!is_flag(args->state_f64) || args->n_chains < 0 || args->step0 < 0 || args->burn_in < 0) return PTRWM_E_ARG;
  if (int rc = Check(args, block)) return rc;
  if (args->n_chains == 0) return PTRWM_OK;
  if (args->state == nullptr) return PTRWM_E_NULL;
  if (args->device_step == nullptr && !periodic_step_due(args->step0 + 1, args->burn_in, block->every))
    return PTRWM_OK;  // (known on the host: no snapshot is due)
  return Launch(args, dim, block, args->step0, (const long long *)args->device_step, (hipStream_t)stream);
}
static int32_t swap_sweep_impl(const ptrwm_run_args *args, int32_t dim, int64_t event_index, int32_t rng_stream,
                               const ptrwm_flow_args *flow, void *stream);
static int32_t split_accept_impl(const ptrwm_run_args *args, int32_t dim, float *proposals, const float *accept_u,
                                 const float *logp_proposed, const ptrwm_flow_args *flow, void *stream);
static int32_t split_moments_impl(const ptrwm_run_args *args, int32_t dim, const MomSpec &spec, void *stream);

extern "C" {

int32_t ptrwm_abi_version(void) { return PTRWM_ABI_VERSION; }

const char *ptrwm_strerror(int32_t code) {
  switch (code) {
    case PTRWM_OK: return "ok";
    case PTRWM_E_NULL: return "required pointer is NULL";
    case PTRWM_E_DIM: return "dim out of range or invalid for this target";
    case PTRWM_E_TEMPS: return "n_temps out of range (1..256)";
    case PTRWM_E_KIND: return "unknown target or proposal kind";
    case PTRWM_E_ARG: return "invalid argument";
    case PTRWM_E_STRUCT: return "struct_size mismatch (ABI version)";
    case PTRWM_E_LAUNCH: return "HIP launch error";
    case PTRWM_E_NOVARIANT: return "variant not compiled";
    default: return "unknown error";
  }
}

int32_t ptrwm_set_kernel_form(int32_t form) {
  if (form != PTRWM_FORM_AUTO && form != PTRWM_FORM_THREAD && form != PTRWM_FORM_QUAD) return PTRWM_E_ARG;
  return __atomic_exchange_n(&g_kernel_form, form, __ATOMIC_RELAXED);
}

int32_t ptrwm_set_stream_mode(int32_t mode) {
  if (mode != PTRWM_STREAM_AUTO && mode != PTRWM_STREAM_OFF && mode != PTRWM_STREAM_ON) return PTRWM_E_ARG;
  return __atomic_exchange_n(&g_stream_mode, mode, __ATOMIC_RELAXED);
}

int32_t ptrwm_last_launch_kind(void) { return t_last_launch_kind; }

int32_t ptrwm_last_launch_functor(void) { return t_last_launch_functor; }

int32_t ptrwm_has_stream_variant(int32_t target_kind, int32_t proposal_kind, int32_t dim) {
  if (ptrwm_has_thread_variant(target_kind, proposal_kind, dim) == 0) return 0;
  const int dpi = width_index_for_dim(dim, target_kind);
  return has_stream_variant(kWidths[dpi].dp, kWidths[dpi].exact) ? 1 : 0;
}

int32_t ptrwm_has_quad_variant(int32_t target_kind, int32_t proposal_kind, int32_t dim, int32_t n_temps) {
  if (target_kind < 0 || target_kind >= PTRWM_TARGET_COUNT) return 0;
  if (proposal_kind < 0 || proposal_kind >= PTRWM_PROPOSAL_COUNT) return 0;
  const int qi = quad_index_for(dim, n_temps, target_kind);
  return qi >= 0 && quad_variants(target_kind, 0).run[proposal_kind][qi] != nullptr ? 1 : 0;
}

int32_t ptrwm_device_simds(void *stream) {
  const long long n = device_simds((hipStream_t)stream);
  return n > 0 ? (int32_t)n : PTRWM_E_LAUNCH;
}

int32_t ptrwm_auto_form_for(int32_t target_kind, int32_t proposal_kind, int32_t dim, int32_t n_temps, int64_t n_chains,
                            int32_t n_simds) {
  if (!temps_in_range(n_temps) || n_chains < 1 || n_simds < 1) return PTRWM_E_ARG;
  const bool th = ptrwm_has_thread_variant(target_kind, proposal_kind, dim) != 0;
  const bool qu = ptrwm_has_quad_variant(target_kind, proposal_kind, dim, n_temps) != 0;
  if (!th && !qu) return PTRWM_E_NOVARIANT;
  if (!th) return PTRWM_FORM_QUAD;
  if (!qu) return PTRWM_FORM_THREAD;
  return auto_prefers_lane_split(dim, n_temps, n_chains, n_simds) ? PTRWM_FORM_QUAD : PTRWM_FORM_THREAD;
}

int32_t ptrwm_auto_form(int32_t target_kind, int32_t proposal_kind, int32_t dim, int32_t n_temps, int64_t n_chains) {
  const int32_t n = ptrwm_device_simds(nullptr);
  return n < 0 ? n : ptrwm_auto_form_for(target_kind, proposal_kind, dim, n_temps, n_chains, n);
}

const char *ptrwm_source_hash(void) { return PTRWM_SOURCE_HASH; }
const char *ptrwm_form_table_source_hash(void) { return kFormTableSourceHash; }

int32_t ptrwm_has_thread_variant(int32_t target_kind, int32_t proposal_kind, int32_t dim) {
  if (target_kind < 0 || target_kind >= PTRWM_TARGET_COUNT) return 0;
  if (proposal_kind < 0 || proposal_kind >= PTRWM_PROPOSAL_COUNT) return 0;
  const int dpi = width_index_for_dim(dim, target_kind);
  return dim >= 1 && dpi >= 0 && target_variants(target_kind).run(proposal_kind, dpi) != nullptr ? 1 : 0;
}

int32_t ptrwm_ext_raw_per_step(int32_t proposal_kind, int32_t dim) {
  switch (proposal_kind) {
    case PTRWM_PROPOSAL_NORMAL: return dim;
    case PTRWM_PROPOSAL_LAPLACE: return dim;
    case PTRWM_PROPOSAL_UNIFORM_RADIUS: return dim + 1;
    default: return PTRWM_E_KIND;
  }
}

int32_t ptrwm_has_variant(int32_t target_kind, int32_t proposal_kind, int32_t dim) {
  if (target_kind < 0 || target_kind >= PTRWM_TARGET_COUNT) return 0;
  if (proposal_kind < 0 || proposal_kind >= PTRWM_PROPOSAL_COUNT) return 0;
  const int dpi = width_index_for_dim(dim, target_kind);
  if (dim < 1 || dpi < 0) return 0;
  if (target_variants(target_kind).run(proposal_kind, dpi) != nullptr) return 1;
  const int qi = quad_index_for(dim, 1, target_kind);  // above width 64 the lane-split kernel is the fused kernel
  return qi >= 0 && quad_variants(target_kind, 0).run[proposal_kind][qi] != nullptr ? 1 : 0;
}

int32_t ptrwm_run(const ptrwm_target_desc *target, const ptrwm_proposal_desc *proposal, const ptrwm_run_args *args,
                  void *hip_stream) {
  return run_impl(target, proposal, args, RunBlocks{}, hip_stream);
}

int32_t ptrwm_run_with_moments(const ptrwm_target_desc *target, const ptrwm_proposal_desc *proposal,
                               const ptrwm_run_args *args, const ptrwm_moments_args *moments, void *stream) {
  return run_impl(target, proposal, args, RunBlocks{moments}, stream);
}

int32_t ptrwm_run_with_chain_moments(const ptrwm_target_desc *target, const ptrwm_proposal_desc *proposal,
                                     const ptrwm_run_args *args, const ptrwm_chain_moments_args *chain_moments, void *stream) {
  return run_impl(target, proposal, args, RunBlocks{chain_moments}, stream);
}

int32_t ptrwm_run_with_diagnostics(const ptrwm_target_desc *target, const ptrwm_proposal_desc *proposal, const ptrwm_run_args *args,
                                   const ptrwm_moments_args *moments, const ptrwm_chain_moments_args *chain_moments,
                                   const ptrwm_flow_args *flow, void *stream) {
  return run_with_blocks(target, proposal, args, moments, chain_moments, {{}, flow}, stream);
}

int32_t ptrwm_run_with_histogram(const ptrwm_target_desc *target, const ptrwm_proposal_desc *proposal, const ptrwm_run_args *args,
                                 const ptrwm_moments_args *moments, const ptrwm_chain_moments_args *chain_moments,
                                 const ptrwm_flow_args *flow, const ptrwm_hist_args *hist, void *stream) {
  return run_with_blocks(target, proposal, args, moments, chain_moments, {{}, flow, hist}, stream);
}

int32_t ptrwm_run_with_adaptation(const ptrwm_target_desc *target, const ptrwm_proposal_desc *proposal, const ptrwm_run_args *args,
                                  const ptrwm_moments_args *moments, const ptrwm_chain_moments_args *chain_moments,
                                  const ptrwm_flow_args *flow, const ptrwm_hist_args *hist, const ptrwm_adapt_args *adapt,
                                  void *stream) {
  return run_with_blocks(target, proposal, args, moments, chain_moments, {{}, flow, hist, adapt}, stream);
}

int32_t ptrwm_adapt_reduce(const ptrwm_run_args *args, const ptrwm_adapt_args *adapt, void *stream) {
  if (int rc = check_tuning_call(adapt, true, args, 0, 0)) return rc;
  if (args->n_chains == 0) return PTRWM_OK;
  return launch_adapt_reduce(adapt, args->n_chains, args->n_temps, (hipStream_t)stream);
}

int32_t ptrwm_adapt_update(const ptrwm_adapt_args *adapt, int32_t n_temps, int64_t window, void *stream) {
  if (int rc = check_tuning_call(adapt, false, nullptr, n_temps, window)) return rc;
  return launch_adapt_update(adapt, n_temps, window, (hipStream_t)stream);
}

int32_t ptrwm_run_with_ladder(const ptrwm_target_desc *target, const ptrwm_proposal_desc *proposal, const ptrwm_run_args *args,
                              const ptrwm_moments_args *moments, const ptrwm_chain_moments_args *chain_moments,
                              const ptrwm_flow_args *flow, const ptrwm_hist_args *hist, const ptrwm_adapt_args *adapt,
                              const ptrwm_ladder_args *ladder, void *stream) {
  return run_with_blocks(target, proposal, args, moments, chain_moments, {{}, flow, hist, adapt, ladder}, stream);
}

int32_t ptrwm_run_with_autocorr(const ptrwm_target_desc *target, const ptrwm_proposal_desc *proposal, const ptrwm_run_args *args,
                                const ptrwm_moments_args *moments, const ptrwm_chain_moments_args *chain_moments,
                                const ptrwm_flow_args *flow, const ptrwm_hist_args *hist, const ptrwm_adapt_args *adapt,
                                const ptrwm_ladder_args *ladder, const ptrwm_acf_args *acf, void *stream) {
  return run_with_blocks(target, proposal, args, moments, chain_moments, {{}, flow, hist, adapt, ladder, acf}, stream);
}

int32_t ptrwm_run_with_covariance(const ptrwm_target_desc *target, const ptrwm_proposal_desc *proposal, const ptrwm_run_args *args,
                                  const ptrwm_moments_args *moments, const ptrwm_chain_moments_args *chain_moments,
                                  const ptrwm_flow_args *flow, const ptrwm_hist_args *hist, const ptrwm_adapt_args *adapt,
                                  const ptrwm_ladder_args *ladder, const ptrwm_acf_args *acf, const ptrwm_cov_args *cov, void *stream) {
  return run_with_blocks(target, proposal, args, moments, chain_moments, {{}, flow, hist, adapt, ladder, acf, cov}, stream);
}

int32_t ptrwm_run_with_energy(const ptrwm_target_desc *target, const ptrwm_proposal_desc *proposal, const ptrwm_run_args *args,
                              const ptrwm_moments_args *moments, const ptrwm_chain_moments_args *chain_moments,
                              const ptrwm_flow_args *flow, const ptrwm_hist_args *hist, const ptrwm_adapt_args *adapt,
                              const ptrwm_ladder_args *ladder, const ptrwm_acf_args *acf, const ptrwm_cov_args *cov,
                              const ptrwm_energy_args *energy, void *stream) {
  return run_with_blocks(target, proposal, args, moments, chain_moments, {{}, flow, hist, adapt, ladder, acf, cov, energy}, stream);
}

int32_t ptrwm_ladder_probe(const ptrwm_run_args *args, const ptrwm_ladder_args *ladder, void *stream) {
  if (int rc = check_tuning_call(ladder, true, args, 0, 0)) return rc;
  if (args->n_temps < 3 || ladder->beta != args->beta) return PTRWM_E_ARG;
  if (args->n_chains == 0) return PTRWM_OK;
  if (args->logp == nullptr) return PTRWM_E_NULL;
  return launch_ladder_probe(ladder, args->logp, args->n_chains, args->n_temps, (hipStream_t)stream);
}

int32_t ptrwm_ladder_update(const ptrwm_ladder_args *ladder, int32_t n_temps, int64_t window, void *stream) {
  if (int rc = check_tuning_call(ladder, false, nullptr, n_temps, window)) return rc;
  if (n_temps < 3) return PTRWM_E_ARG;  // (the same code as a window out of range: their order does not show)
  return launch_ladder_update(ladder, n_temps, window, (hipStream_t)stream);
}

int32_t ptrwm_histogram(const ptrwm_run_args *args, int32_t dim, const ptrwm_hist_args *hist, void *stream) {
  return snapshot_call<check_hist, launch_hist>(args, dim, hist, stream);
}

int32_t ptrwm_autocorr(const ptrwm_run_args *args, int32_t dim, const ptrwm_acf_args *acf, void *stream) {
  return snapshot_call<check_acf, launch_acf>(args, dim, acf, stream);
}

int32_t ptrwm_covariance(const ptrwm_run_args *args, int32_t dim, const ptrwm_cov_args *cov, void *stream) {
  return snapshot_call<check_cov, launch_cov>(args, dim, cov, stream);
}

int32_t ptrwm_energy(const ptrwm_run_args *args, const ptrwm_energy_args *energy, void *stream) {
  if (args == nullptr || energy == nullptr) return PTRWM_E_NULL;
  if (!has_abi_size(args)) return PTRWM_E_STRUCT;
  if (!temps_in_range(args->n_temps)) return PTRWM_E_TEMPS;
  if (args->n_chains < 0 || args->step0 < 0 || args->burn_in < 0) return PTRWM_E_ARG;
  if (int rc = check_energy(args, energy)) return rc;
  if (args->n_chains == 0) return PTRWM_OK;
  if (args->logp == nullptr || args->beta == nullptr) return PTRWM_E_NULL;
  if (args->device_step == nullptr && !periodic_step_due(args->step0 + 1, args->burn_in, energy->every))
    return PTRWM_OK;  // (known on the host: no snapshot is due)
  return launch_energy(args, 0, energy, args->step0, (const long long *)args->device_step, (hipStream_t)stream);
}

}  // extern "C"

// ---- ptrwm_run: check, choose the kernel, fill its arguments, cut the request into launches --------------------------------

// swap events whose uniforms the caller supplies (ext_swap_u) in this request
static long long ext_swap_events(const ptrwm_run_args *args) {
  if (args->ext_prop == nullptr || args->n_temps < 2) return 0;
  return periodic_steps_in(args->step0, args->n_steps, args->burn_in, args->swap_every);
}

// Job 1: everything that can be refused from the arguments alone.  *empty: a valid request with nothing to do.
static int32_t check_run(const ptrwm_target_desc *target, const ptrwm_proposal_desc *proposal, const ptrwm_run_args *args,
                         const MomSpec &spec, const ptrwm_flow_args *flow, const ptrwm_hist_args *hist, bool *empty) {
  if (proposal == nullptr || args == nullptr) return PTRWM_E_NULL;
  if (int rc = check_target(target)) return rc;
  if (!has_abi_size(args)) return PTRWM_E_STRUCT;
  if (proposal->kind < 0 || proposal->kind >= PTRWM_PROPOSAL_COUNT) return PTRWM_E_KIND;
  if (!temps_in_range(args->n_temps)) return PTRWM_E_TEMPS;
  if (int rc = check_moments(args, spec)) return rc;
  if (int rc = check_flow(args, flow)) return rc;
  if (int rc = check_hist(args, hist)) return rc;
  if (args->n_chains < 0 || args->n_steps < 0 || args->step0 < 0 || args->burn_in < 0 || args->swap_every < 1 ||
      !swap_rule_known(args) || !fused_fields_ok(args))
    return PTRWM_E_ARG;
  *empty = args->n_chains == 0 || args->n_steps == 0;  // empty batch: nothing to touch
  if (*empty) return PTRWM_OK;
  if (args->state == nullptr || args->logp == nullptr || args->beta == nullptr || proposal->temp_scale == nullptr)
    return PTRWM_E_NULL;
  if (proposal->kind == PTRWM_PROPOSAL_LAPLACE && proposal->dim_scale == nullptr) return PTRWM_E_NULL;
  const bool ext = args->ext_prop != nullptr;
  // (double state / trace / ext_prop, include/ptrwm.h state_f64: external randoms for the Normal proposal only)
  if (args->state_f64 == 1 && ext && proposal->kind != PTRWM_PROPOSAL_NORMAL) return PTRWM_E_ARG;
  if (ext && args->ext_u == nullptr) return PTRWM_E_NULL;
  if (args->trace != nullptr && (args->trace_chains < 1 || args->trace_temps < 1 || args->trace_row0 < 0 ||
                                 args->trace_temps > args->n_temps || args->trace_chains > args->n_chains ||
                                 args->trace_every < 0))
    return PTRWM_E_ARG;
  return PTRWM_OK;
}

// what of a launch depends on the kernel form alone
struct FormShape {
  bool quad;  // lane-split form
  bool wide;  // exchange groups: one wavefront holding whole ladders, or ("wide") one workgroup per ladder
  int ladders_per_group;
};
static FormShape form_shape(bool quad, int n_temps) {
  const bool wide = n_temps * (quad ? kQuad : 1) > 64;
  return {quad, wide, quad ? quad_ladders_per_group(n_temps) : (wide ? 1 : 64 / n_temps)};
}

// Job 2: what runs.  status != PTRWM_OK: nothing can, and why.
struct RunChoice {
  int32_t status;
  RunLaunchFn fn;
  int alt;         // the kind's specialised functor (quad_variants)
  int rc_perm[3];  // alt == 2: the target's indices of the modes -m, 0, +m
  FormShape shape;
  int mode;        // kRunFull / kRunStream / kRunProd
  unsigned n_blocks;
};

// the workgroup's LDS with the moments regions (if any) and the flow regions (if any) behind it, as the launcher will ask for
// it at most (variants.h LaunchShape)
static unsigned moments_lds_bytes(const FormShape &f, int n_temps, int dim, int dpi, bool f64, const MomSpec &spec, bool flow) {
  KArgs k{};  // (the launch shapes read these five fields)
  k.n_temps = n_temps;
  k.dim = dim;
  k.chains_per_wave = f.ladders_per_group;
  k.full.mom_temps = spec.m != nullptr ? spec.m->temps : 0;
  k.full.mom_chain = spec.per_chain ? 1 : 0;
  return (f.quad ? quad_launch_shape(k, canon_width(dim), f64) : thread_launch_shape(k, kWidths[dpi].dp)).full_bytes(spec.m != nullptr, flow);
}

static RunChoice choose_kernel(const ptrwm_target_desc *target, const ptrwm_proposal_desc *proposal, const ptrwm_run_args *args,
                               const MomSpec &spec, bool flow, hipStream_t stream, bool allow_stream = true) {
  RunChoice c{};
  auto refuse = [&c](int32_t status) {
    c.status = status;
    return c;
  };
  const int kind = target->kind, dim = target->dim, T = args->n_temps, pk = proposal->kind;
  const bool f64 = args->state_f64 == 1;  // lane-split form only
  const int dpi = width_index_for_dim(dim, kind);
  if (dpi < 0) return refuse(PTRWM_E_DIM);
  const int qi = quad_index_for(dim, T, kind);
  c.alt = specialised_form(target, c.rc_perm);
  if (c.alt == 2) {
    // the folded tables hold no state_f64 kernels (quad_rough_carpet_sym.hip): where they lack a kernel that the
    // two-term tables have for this launch, the two-term functor runs (the same bits)
    const QuadVariants &q2 = quad_variants(kind, 2), &q1 = quad_variants(kind, 1);
    const bool thread_ok = target_variants(kind, 2).run(pk, dpi) != nullptr || target_variants(kind, 1).run(pk, dpi) == nullptr;
    const bool quad_ok = qi < 0 || (f64 ? q2.run_f64 : q2.run)[pk][qi] != nullptr || (f64 ? q1.run_f64 : q1.run)[pk][qi] == nullptr;
    if (!thread_ok || !quad_ok) c.alt = 1;
  }
  // The form (bit-identical results: a speed decision, see g_kernel_form - except above dim 64, where the lane-split form
  // is the only one, and for double states, which only it holds in registers: null = ladder too long for its workgroup)
  const RunLaunchFn thread_fn = target_variants(kind, c.alt).run(pk, dpi);  // null above width 64
  const QuadVariants &qv = quad_variants(kind, c.alt);
  const RunLaunchFn quad_fn = qi >= 0 ? (f64 ? qv.run_f64 : qv.run)[pk][qi] : nullptr;
  const int form = __atomic_load_n(&g_kernel_form, __ATOMIC_RELAXED);
  bool quad = f64;
  if (!f64 && quad_fn != nullptr && (thread_fn == nullptr || form != PTRWM_FORM_THREAD))
    quad = thread_fn == nullptr || form == PTRWM_FORM_QUAD || auto_prefers_lane_split(dim, T, args->n_chains, device_simds(stream));
  c.fn = quad ? quad_fn : thread_fn;
  if (c.fn == nullptr) return refuse(PTRWM_E_NOVARIANT);
  // (an argument check, made here: a caller who also asks for a missing variant has always been told of that first)
  if (ext_swap_events(args) > 0 && args->ext_swap_u == nullptr) return refuse(PTRWM_E_NULL);
  c.shape = form_shape(quad, T);
  if (spec.m != nullptr || flow) {
    unsigned need = moments_lds_bytes(c.shape, T, dim, dpi, f64, spec, flow);
    // Per-chain regions grow with the ladders of a group.  Where AUTO chose the form and both exist, a workgroup that needs
    // more than half of the CU's LDS (one workgroup resident: one wave per SIMD in the thread form) - or does not fit at
    // all - hands over to the other form if that one needs less (the same bits).  A pinned form is taken as it is.
    const bool both = !f64 && form == PTRWM_FORM_AUTO && thread_fn != nullptr && quad_fn != nullptr;
    if (spec.per_chain && both && need > kMaxLdsBytes / 2u) {
      const FormShape other = form_shape(!quad, T);
      const unsigned other_need = moments_lds_bytes(other, T, dim, dpi, f64, spec, flow);
      if (other_need < need) {
        c.fn = quad ? thread_fn : quad_fn;
        c.shape = other;
        need = other_need;
      }
    }
    if (need > kMaxLdsBytes) return refuse(PTRWM_E_ARG);
  }
  // moments are accumulated, and flow words exchanged, by the fixture / trace twin (kernel.h FullArgs)
  const bool full = args->ext_prop != nullptr || args->trace != nullptr || args->accept_flags != nullptr || spec.m != nullptr || flow;
  // the streaming form for short launches of the one-thread-per-replica kernel (see kStreamMaxSteps above)
  bool streaming = false;
  if (allow_stream && !c.shape.quad && !full && has_stream_variant(kWidths[dpi].dp, kWidths[dpi].exact) && stream_layout_ok(args, dim, c.shape.ladders_per_group)) {
    const int mode = __atomic_load_n(&g_stream_mode, __ATOMIC_RELAXED);
    if (mode == PTRWM_STREAM_ON) {
      streaming = true;
    } else if (mode == PTRWM_STREAM_AUTO && args->n_steps <= kStreamMaxSteps) {
      // state + log-density + the two statistics every launch touches (acceptance count, squared-jump sum)
      const long long bytes = args->n_chains * (long long)T * (4ll * dim + 20ll);
      streaming = bytes >= kStreamMinBytes && bytes <= kStreamMaxBytes;
    }
  }
  c.mode = full ? kRunFull : (streaming ? kRunStream : kRunProd);
  const long long n_groups = (args->n_chains + c.shape.ladders_per_group - 1) / c.shape.ladders_per_group;
  const long long n_blocks = c.shape.wide ? n_groups : (n_groups + kWavesPerBlock - 1) / kWavesPerBlock;  // wide: one group per block
  if (n_blocks > 0x7fffffffll) return refuse(PTRWM_E_ARG);
  c.n_blocks = (unsigned)n_blocks;
  return c;
}

// Job 3: the kernel arguments that every launch of the request shares
static KArgs fill_kargs(const ptrwm_target_desc *target, const ptrwm_proposal_desc *proposal, const ptrwm_run_args *args,
                        const MomSpec &spec, const ptrwm_flow_args *flow, const RunChoice &c) {
  KArgs k;
  k.state = args->state;
  k.logp = args->logp;
  k.beta = args->beta;
  k.temp_scale = proposal->temp_scale;
  k.n_accept = (long long *)args->n_accept;
  k.sq_jump = args->sq_jump;
  k.swap_accept = (long long *)args->swap_accept;
  k.last_swap_ordinal = (long long *)args->last_swap_ordinal;
  k.n_chains = args->n_chains;
  k.chain_offset = args->chain_offset;
  k.n_temps = args->n_temps;
  k.dim = target->dim;
  k.swap_every = args->swap_every;
  k.swap_mode = args->swap_mode;
  k.swap_order = args->swap_order;
  k.chains_per_wave = c.shape.ladders_per_group;
  k.k0 = philox_key(args->seed).k0;
  k.k1 = philox_key(args->seed).k1;
  k.tp = make_tparams(target);
  if (target->kind == PTRWM_TARGET_ROUGH_CARPET && c.alt == 2)  // the folded form reads the modes as -m, 0, +m
    for (int i = 0; i < 3; ++i) k.tp.p[i] = target->p[c.rc_perm[i]], k.tp.p[3 + i] = target->p[3 + c.rc_perm[i]];
  k.pp = make_pparams(proposal);
  k.full.trace = args->trace;
  k.full.trace_logp = args->trace_logp;
  k.full.trace_chains = args->trace != nullptr ? args->trace_chains : 0;
  k.full.trace_temps = args->trace != nullptr ? (unsigned)args->trace_temps : 0u;  // (checked: 1..n_temps with a trace)
  k.full.trace_every = args->trace_every > 1 ? args->trace_every : 1;
  k.full_flow_lds = 0;  // (set by the launcher for a launch with flow, variants.h launch_twins)
  const ptrwm_moments_args *const mom = spec.m;
  k.full.mom_sum = nullptr;  // (set per launch: a launch without an accumulated step leaves the accumulators and its LDS alone)
  k.full.mom_sum_sq = mom != nullptr ? mom->sum_sq : nullptr;
  k.full.mom_sum_logp = mom != nullptr ? mom->sum_logp : nullptr;
  k.full.mom_count = mom != nullptr ? (long long *)mom->count : nullptr;
  k.full_mom_steps = 0;
  k.full.mom_temps = mom != nullptr ? mom->temps : 0;
  k.full.mom_every = mom != nullptr ? mom->every : 1;
  k.full.steps_to_mom = kNoStepInLaunch;
  k.full.mom_chain = (mom != nullptr && spec.per_chain) ? 1 : 0;
  k.full.flow_walker = flow != nullptr ? flow->walker : nullptr;
  k.full.flow_round_trips = flow != nullptr ? (long long *)flow->round_trips : nullptr;
  k.full.flow_up = flow != nullptr ? (long long *)flow->n_up : nullptr;
  k.full.flow_down = flow != nullptr ? (long long *)flow->n_down : nullptr;
  return k;
}

static int32_t run_impl(const ptrwm_target_desc *target, const ptrwm_proposal_desc *proposal, const ptrwm_run_args *args,
                        const RunBlocks &blocks, void *hip_stream) {
  const auto &[spec, flow, hist, adapt, ladder, acf, cov, energy] = blocks;
  bool empty = false;
  if (int rc = check_run(target, proposal, args, spec, flow, hist, &empty)) return rc;
  // the two tunings (adapt.h, ladder.h): their own checks after the existing ones, all before anything is enqueued
  if (int rc = check_tuning(adapt)) return rc;
  if (adapt != nullptr && !tuning_fits_run(adapt, args, adapt->temp_scale, proposal->temp_scale)) return PTRWM_E_ARG;
  if (int rc = check_tuning(ladder)) return rc;
  if (ladder != nullptr) {
    if (args->n_temps < 3 || !tuning_fits_run(ladder, args, ladder->beta, args->beta)) return PTRWM_E_ARG;
    if (ladder->temp_scale != nullptr && ladder->temp_scale != proposal->temp_scale) return PTRWM_E_ARG;
  }
  if (int rc = check_acf(args, acf)) return rc;  // (the autocovariance: after every existing block's checks)
  if (int rc = check_cov(args, cov)) return rc;  // (the covariance: after those)
  if (int rc = check_energy(args, energy)) return rc;  // (the log-density sums: after those)
  if (empty) return PTRWM_OK;
  // (every = 0: no such tuning, schedule.h)
  const WarmupWindows scale_w = adapt != nullptr ? WarmupWindows{adapt->every, adapt->until} : WarmupWindows{0, 0};
  const WarmupWindows ladder_w = ladder != nullptr ? WarmupWindows{ladder->every, ladder->until} : WarmupWindows{0, 0};
  // (a request that touches an adapting window keeps to the classic kernels: the streaming form prefetches the counters
  // it adds to, and a warm-up launch has no squared-jump sum)
  const bool adapts = step_adapts(scale_w, args->step0);
  const RunChoice c = choose_kernel(target, proposal, args, spec, flow != nullptr, (hipStream_t)hip_stream, !adapts);
  if (c.status != PTRWM_OK) return c.status;
  KArgs k = fill_kargs(target, proposal, args, spec, flow, c);
  t_last_launch_kind = c.shape.quad ? PTRWM_LAUNCH_QUAD : (c.mode == kRunStream ? PTRWM_LAUNCH_STREAM : PTRWM_LAUNCH_THREAD);
  t_last_launch_functor = c.alt;

  // Job 4: one launch per cut of the schedule (schedule.h); the per-step arrays advance by the steps, rows and events done
  const bool ext = args->ext_prop != nullptr;
  const StepRequest req = {args->step0, args->n_steps, args->burn_in, args->swap_every, args->swap_event_offset,
                           k.full.trace_every, args->trace_row0, k.full.mom_every};
  const long long cap = max_steps_per_launch(args->n_chains, args->n_temps);
  const long long reps = args->n_chains * args->n_temps, raw = ext_raw_per_step(proposal->kind, target->dim);
  // (a launch's trace pointers stand at the row of its first traced step; a row: trace_chains x trace_temps replicas)
  const long long trace_row = args->trace != nullptr ? args->trace_chains * (long long)args->trace_temps : 0;
  const auto countdown = [](int steps) { return (unsigned)(steps < kNoStepInLaunch ? steps : kNoStepInLaunch); };  // (a launch: <= 2^16 steps)
  for (long long done = 0; done < args->n_steps; done += k.n_steps) {
    // (a launch also ends at the nearest due step of a snapshot block, each at its own period: snapshot.h)
    const long long s0 = args->step0 + done, b0 = args->burn_in;
    const long long to_snap = std::min({steps_to_snapshot(hist, s0, b0, cap), steps_to_snapshot(acf, s0, b0, cap), steps_to_snapshot(cov, s0, b0, cap),
                                        steps_to_snapshot(energy, s0, b0, cap)});
    // (the tunings, schedule.h warmup_launch_at: a launch inside an adapting window of the scale ends with the window at the
    // latest - the reduce and update kernels run between two launches - and is the production kernel told to count from its
    // first step, into the window scratch, and that no multiple of swap_every lies in it: count_on holds and swap_due never
    // does, kernel.h.  One that starts in an adapting window of the ladder ends behind the next probe step at the latest - the
    // probe kernel reads logp between two launches - and is otherwise told nothing: an ordinary burn-in launch)
    const WarmupLaunch wl = warmup_launch_at(args->step0 + done, launch_steps(req, done, to_snap), scale_w,
                                             adapt != nullptr && adapt->defer_update == 1, ladder_w,
                                             ladder != nullptr ? ladder->probe_every : 1, ladder != nullptr && ladder->defer_update == 1);
    const LaunchCut cut = launch_at(req, done, wl.n);
    k.step0 = cut.step0;
    k.n_steps = cut.n;
    k.burn_left = wl.warmup ? 0 : cut.burn_left;
    k.first_swap_event = cut.first_swap_event;
    k.steps_to_swap = wl.warmup ? kNoStepInLaunch : cut.steps_to_swap;
    k.n_accept = wl.warmup ? (long long *)adapt->window_accept : (long long *)args->n_accept;
    k.sq_jump = wl.warmup ? nullptr : args->sq_jump;
    k.full.ext_prop = ext ? args->ext_prop + done * reps * raw * (args->state_f64 == 1 ? 2 : 1) : nullptr;  // (f64: a double array)
    k.full.ext_u = ext ? args->ext_u + done * reps : nullptr;
    k.full.ext_swap_u = (ext && args->ext_swap_u != nullptr) ? args->ext_swap_u + cut.events_before * args->n_chains * (args->n_temps - 1) : nullptr;
    k.full.accept_flags = args->accept_flags != nullptr ? args->accept_flags + done * reps : nullptr;
    k.full.trace = args->trace != nullptr ? args->trace + cut.trace_row0 * trace_row * target->dim * (args->state_f64 == 1 ? 2 : 1) : nullptr;
    k.full.trace_logp = args->trace_logp != nullptr ? args->trace_logp + cut.trace_row0 * trace_row : nullptr;
    k.full.steps_to_trace = countdown(cut.steps_to_trace);
    if (spec.m != nullptr) {
      k.full_mom_steps = (unsigned)cut.mom_steps;  // (per chain: count[t] += mom_steps; pooled: += live ladders x mom_steps)
      k.full.mom_sum = cut.mom_steps > 0 ? spec.m->sum : nullptr;
      k.full.steps_to_mom = countdown(cut.steps_to_mom);
    }
    if (c.fn(k, c.n_blocks, c.mode, (hipStream_t)hip_stream) != hipSuccess) return PTRWM_E_LAUNCH;
    // (whatever snapshot is due behind this cut: histogram, autocovariance, covariance, log-density sums, in front of the
    // tunings' kernels)
    const long long sc = cut.step0 + cut.n;
    if (int rc = snapshot_if_due<launch_hist>(hist, args, target->dim, sc, (hipStream_t)hip_stream)) return rc;
    if (int rc = snapshot_if_due<launch_acf>(acf, args, target->dim, sc, (hipStream_t)hip_stream)) return rc;
    if (int rc = snapshot_if_due<launch_cov>(cov, args, target->dim, sc, (hipStream_t)hip_stream)) return rc;
    if (int rc = snapshot_if_due<launch_energy>(energy, args, target->dim, sc, (hipStream_t)hip_stream)) return rc;
    if (wl.scale_reduce)
      if (int rc = launch_adapt_reduce(adapt, args->n_chains, args->n_temps, (hipStream_t)hip_stream)) return rc;
    if (wl.scale_update)
      if (int rc = launch_adapt_update(adapt, args->n_temps, wl.scale_window, (hipStream_t)hip_stream)) return rc;
    if (wl.ladder_probe)  // (behind the scale's kernels)
      if (int rc = launch_ladder_probe(ladder, args->logp, args->n_chains, args->n_temps, (hipStream_t)hip_stream)) return rc;
    if (wl.ladder_update)
      if (int rc = launch_ladder_update(ladder, args->n_temps, wl.ladder_window, (hipStream_t)hip_stream)) return rc;
  }
  return PTRWM_OK;
}

extern "C" {

int32_t ptrwm_swap_sweep(const ptrwm_run_args *args, int32_t dim, int64_t event_index, int32_t rng_stream,
                         void *stream) {
  return swap_sweep_impl(args, dim, event_index, rng_stream, nullptr, stream);
}

int32_t ptrwm_swap_sweep_with_flow(const ptrwm_run_args *args, int32_t dim, int64_t event_index, int32_t rng_stream,
                                   const ptrwm_flow_args *flow, void *stream) {
  return swap_sweep_impl(args, dim, event_index, rng_stream, flow, stream);
}

int32_t ptrwm_split_accept(const ptrwm_run_args *args, int32_t dim, float *proposals, const float *accept_u,
                           const float *logp_proposed, void *stream) {
  return split_accept_impl(args, dim, proposals, accept_u, logp_proposed, nullptr, stream);
}

int32_t ptrwm_split_accept_with_flow(const ptrwm_run_args *args, int32_t dim, float *proposals, const float *accept_u,
                                     const float *logp_proposed, const ptrwm_flow_args *flow, void *stream) {
  return split_accept_impl(args, dim, proposals, accept_u, logp_proposed, flow, stream);
}

}  // extern "C"

static int32_t swap_sweep_impl(const ptrwm_run_args *args, int32_t dim, int64_t event_index, int32_t rng_stream,
                               const ptrwm_flow_args *flow, void *stream) {
  if (args == nullptr) return PTRWM_E_NULL;
  if (!has_abi_size(args)) return PTRWM_E_STRUCT;
  if (!fused_fields_ok(args)) return PTRWM_E_ARG;
  if (dim < 1 || dim > PTRWM_MAX_DIM) return PTRWM_E_DIM;
  if (!temps_in_range(args->n_temps)) return PTRWM_E_TEMPS;
  if (args->n_chains < 0 || args->n_chains > 0x7fffffffll || args->step0 < 0 || event_index < 0 || rng_stream < 1 ||
      rng_stream > 15 || !swap_rule_known(args))
    return PTRWM_E_ARG;
  if (int rc = check_flow(args, flow)) return rc;
  if (args->n_chains == 0 || args->n_temps == 1) return PTRWM_OK;  // nothing to exchange
  if (args->state == nullptr || args->logp == nullptr || args->beta == nullptr) return PTRWM_E_NULL;
  return launch_sweep(args, dim, event_index, rng_stream, nullptr, nullptr, flow, (hipStream_t)stream);
}

extern "C" {

static int32_t split_common_checks(const ptrwm_run_args *args, int32_t dim) {
  if (args == nullptr) return PTRWM_E_NULL;
  if (!has_abi_size(args)) return PTRWM_E_STRUCT;
  if (args->state_f64 != 0) return PTRWM_E_ARG;  // float states only
  if ((args->split_flags & ~PTRWM_SPLIT_NO_SWEEP) != 0 || (args->split_flags != 0 && args->device_step == nullptr)) return PTRWM_E_ARG;
  if (dim < 1 || dim > PTRWM_MAX_DIM) return PTRWM_E_DIM;
  if (!temps_in_range(args->n_temps)) return PTRWM_E_TEMPS;
  if (args->n_chains < 0 || args->n_chains > 0x7fffffffll || args->step0 < 0 || args->burn_in < 0 ||
      args->swap_every < 1 || !swap_rule_known(args))
    return PTRWM_E_ARG;
  if (args->device_step != nullptr && (args->ext_prop != nullptr || args->ext_u != nullptr || args->ext_swap_u != nullptr))
    return PTRWM_E_ARG;  // device-step mode draws from Philox only
  return PTRWM_OK;
}

int32_t ptrwm_split_propose(const ptrwm_proposal_desc *proposal, const ptrwm_run_args *args, int32_t dim,
                            float *proposals, float *accept_u, void *stream) {
  if (proposal == nullptr) return PTRWM_E_NULL;
  if (int rc = split_common_checks(args, dim)) return rc;
  if (proposal->kind < 0 || proposal->kind >= PTRWM_PROPOSAL_COUNT) return PTRWM_E_KIND;
  if (args->n_chains == 0) return PTRWM_OK;
  if (args->state == nullptr || proposals == nullptr || accept_u == nullptr || proposal->temp_scale == nullptr)
    return PTRWM_E_NULL;
  if (proposal->kind == PTRWM_PROPOSAL_LAPLACE && proposal->dim_scale == nullptr) return PTRWM_E_NULL;
  if (args->ext_prop != nullptr && args->ext_u == nullptr) return PTRWM_E_NULL;
  const int dpi = width_index_for_dim(dim);
  if (dpi < 0) return PTRWM_E_DIM;
  const PParams pp = make_pparams(proposal);
  const unsigned k0 = philox_key(args->seed).k0, k1 = philox_key(args->seed).k1;
  const int n_raw = ptrwm_ext_raw_per_step(proposal->kind, dim);
  hipError_t err;
#define PTRWM_SPLIT_CALL(P)                                                                                          \
  launch_split_propose<P>(dpi, args->state, proposals, accept_u, args->n_chains, args->chain_offset,                 \
                          (unsigned long long)args->step0, dim, args->n_temps, proposal->temp_scale, pp,             \
                          args->ext_prop, args->ext_prop != nullptr ? args->ext_u : nullptr, n_raw, k0, k1,         \
                          (const long long *)args->device_step, (hipStream_t)stream)
  switch (proposal->kind) {
    case PTRWM_PROPOSAL_NORMAL: err = PTRWM_SPLIT_CALL(NormalProposal); break;
    case PTRWM_PROPOSAL_LAPLACE: err = PTRWM_SPLIT_CALL(LaplaceProposal); break;
    default: err = PTRWM_SPLIT_CALL(UniformRadiusProposal); break;
  }
#undef PTRWM_SPLIT_CALL
  return err == hipSuccess ? PTRWM_OK : PTRWM_E_LAUNCH;
}

static_assert(PTRWM_MAX_DIM == kPrecMaxDim, "precond.h and include/ptrwm.h: one largest dim");

int32_t ptrwm_split_propose_precond(const ptrwm_proposal_desc *proposal, const ptrwm_run_args *args, int32_t dim,
                                    const ptrwm_precond_args *precond, float *proposals, float *accept_u, void *stream) {
  if (proposal == nullptr || precond == nullptr) return PTRWM_E_NULL;
  if (int rc = split_common_checks(args, dim)) return rc;
  if (proposal->kind != PTRWM_PROPOSAL_NORMAL) return PTRWM_E_KIND;
  if (precond->struct_size != sizeof(ptrwm_precond_args)) return PTRWM_E_STRUCT;
  if (args->n_chains == 0) return PTRWM_OK;
  if (args->state == nullptr || proposals == nullptr || accept_u == nullptr || proposal->temp_scale == nullptr ||
      precond->chol == nullptr)
    return PTRWM_E_NULL;
  if (args->ext_prop != nullptr && args->ext_u == nullptr) return PTRWM_E_NULL;
  PrecondProposeArgs a;
  a.state = args->state;
  a.chol = precond->chol;
  a.temp_scale = proposal->temp_scale;
  a.ext_raw = args->ext_prop;
  a.ext_u = args->ext_prop != nullptr ? args->ext_u : nullptr;
  a.proposals = proposals;
  a.accept_u = accept_u;
  a.n_reps = args->n_chains * (long long)args->n_temps;
  a.chain_offset = args->chain_offset;
  a.step = (unsigned long long)args->step0;
  a.device_step = (const long long *)args->device_step;
  a.n_temps = args->n_temps;
  a.dim = dim;
  a.k0 = philox_key(args->seed).k0;
  a.k1 = philox_key(args->seed).k1;
  const unsigned lds = (unsigned)prec_lds_bytes(dim);
  if (lds > 48u * 1024u) {  // (above the default dynamic-LDS allowance; raised once per device)
    static unsigned long long raised_mask = 0;
    if (raise_dynamic_lds((const void *)precond_propose_kernel, (const void *)precond_propose_kernel,
                          prec_lds_bytes(PTRWM_MAX_DIM), raised_mask) != hipSuccess)
      return PTRWM_E_LAUNCH;
  }
  // a workgroup stages the factor once and walks tiles (precond.h prec_grid)
  const long long tiles = (a.n_reps + kPrecRows - 1) / kPrecRows;
  hipLaunchKernelGGL(precond_propose_kernel, dim3((unsigned)prec_grid(tiles, device_cus())), dim3(kPrecThreads), lds,
                     (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? PTRWM_OK : PTRWM_E_LAUNCH;
}

int32_t ptrwm_precond_update(const ptrwm_precond_update_args *up, int32_t dim, int64_t window, void *stream) {
  if (up == nullptr) return PTRWM_E_NULL;
  if (up->struct_size != sizeof(ptrwm_precond_update_args)) return PTRWM_E_STRUCT;
  if (dim < 1 || dim > PTRWM_MAX_DIM) return PTRWM_E_DIM;
  if (!(up->memory > 0.0 && up->memory <= 1.0) || !(up->jitter >= 0.0) || !std::isfinite(up->jitter) ||
      !(up->min_count >= 1.0) || up->windows < 1 || window < 0 || window >= up->windows)
    return PTRWM_E_ARG;
  if (up->chol == nullptr || up->sxx == nullptr || up->sx == nullptr || up->count == nullptr || up->run_xx == nullptr ||
      up->run_x == nullptr || up->run_w == nullptr)
    return PTRWM_E_NULL;
  PrecondUpdateArgs a;
  a.chol = up->chol;
  a.sxx = up->sxx;
  a.sx = up->sx;
  a.count = (long long *)up->count;
  a.run_xx = up->run_xx;
  a.run_x = up->run_x;
  a.run_w = up->run_w;
  a.chol_history = up->chol_history;
  a.weight_history = up->weight_history;
  a.skipped = (long long *)up->skipped;
  a.memory = up->memory;
  a.jitter = up->jitter;
  a.min_count = up->min_count;
  a.window = window;
  a.dim = dim;
  static_assert(prec_update_lds_bytes(PTRWM_MAX_DIM) <= 48 * 1024, "precond_update_kernel: within the default dynamic-LDS allowance");
  hipLaunchKernelGGL(precond_update_kernel, dim3(1), dim3(kPrecUpdateThreads), (size_t)prec_update_lds_bytes(dim),
                     (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? PTRWM_OK : PTRWM_E_LAUNCH;
}

}  // extern "C"

static int32_t split_accept_impl(const ptrwm_run_args *args, int32_t dim, float *proposals, const float *accept_u,
                                 const float *logp_proposed, const ptrwm_flow_args *flow, void *stream) {
  if (int rc = split_common_checks(args, dim)) return rc;
  if (int rc = check_flow(args, flow)) return rc;
  if (args->n_chains == 0) return PTRWM_OK;
  if (args->state == nullptr || args->logp == nullptr || args->beta == nullptr || proposals == nullptr ||
      accept_u == nullptr || logp_proposed == nullptr)
    return PTRWM_E_NULL;
  const long long sc = args->step0 + 1;  // step_counter of this step
  const SplitStepDue due = split_step_due(sc, args->burn_in, args->swap_every, args->n_temps);
  if (due.swap_due && args->ext_prop != nullptr && args->ext_swap_u == nullptr) return PTRWM_E_NULL;
  SplitAcceptArgs a;
  a.state = args->state;
  a.logp = args->logp;
  a.proposals = proposals;
  a.beta = args->beta;
  a.accept_u = accept_u;
  a.logp_new = logp_proposed;
  a.n_accept = (long long *)args->n_accept;
  a.sq_jump = args->sq_jump;
  a.accept_flags = args->accept_flags;
  a.n_reps = args->n_chains * (long long)args->n_temps;
  a.n_temps = args->n_temps;
  a.dim = dim;
  a.count_on = due.count_on ? 1 : 0;
  a.swap_due = due.swap_due ? 1 : 0;
  a.device_step = (const long long *)args->device_step;
  a.step_offset = args->step0;
  a.burn_in = args->burn_in;
  a.swap_every = args->swap_every;
  {
    const unsigned lds = 2u * split_tile_lds_bytes(dim);
    if (lds > 48u * 1024u) {  // (dim > 95: above the default dynamic-LDS allowance; raised once per device)
      static unsigned long long raised_mask = 0;
      if (raise_dynamic_lds((const void *)split_accept_kernel, (const void *)split_accept_kernel,
                            (int)(2u * split_tile_lds_bytes(PTRWM_MAX_DIM)), raised_mask) != hipSuccess)
        return PTRWM_E_LAUNCH;
    }
    hipLaunchKernelGGL(split_accept_kernel, dim3((unsigned)((a.n_reps + 63) / 64)), dim3(64), lds, (hipStream_t)stream, a);
  }
  if (hipGetLastError() != hipSuccess) return PTRWM_E_LAUNCH;
  if (args->device_step != nullptr) {
    // device-step mode: the sweep is enqueued with every step and decides on the device whether its event is due - unless
    // the caller vouches that this step has none (PTRWM_SPLIT_NO_SWEEP)
    if (args->n_temps < 2 || (args->split_flags & PTRWM_SPLIT_NO_SWEEP) != 0) return PTRWM_OK;
    return launch_sweep(args, dim, 0, (int)kStreamSwap, proposals, args->sq_jump, flow, (hipStream_t)stream);
  }
  if (!due.swap_due) return PTRWM_OK;
  // the swap event of this step: event number as ptrwm_run counts them, swap uniforms from the fused kernel's stream
  const long long ev = swap_event_number(sc, args->burn_in, args->swap_every) + args->swap_event_offset;
  return launch_sweep(args, dim, ev, (int)kStreamSwap, proposals, args->sq_jump, flow, (hipStream_t)stream);
}

extern "C" {

int32_t ptrwm_split_chain_moments(const ptrwm_run_args *args, int32_t dim, const ptrwm_chain_moments_args *cm, void *stream) {
  return split_moments_impl(args, dim, cm, stream);
}

int32_t ptrwm_split_moments(const ptrwm_run_args *args, int32_t dim, const ptrwm_moments_args *moments, void *stream) {
  return split_moments_impl(args, dim, moments, stream);
}

int32_t ptrwm_split_advance(const ptrwm_run_args *args, void *stream) {
  if (args == nullptr) return PTRWM_E_NULL;
  if (!has_abi_size(args)) return PTRWM_E_STRUCT;
  if (args->device_step == nullptr) return PTRWM_E_NULL;
  hipLaunchKernelGGL(split_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (long long *)args->device_step,
                     args->n_steps > 0 ? (long long)args->n_steps : 1ll);
  return hipGetLastError() == hipSuccess ? PTRWM_OK : PTRWM_E_LAUNCH;
}

int32_t ptrwm_init_states(const ptrwm_run_args *args, int32_t dim, const ptrwm_init_args *init, void *stream) {
  if (args == nullptr || init == nullptr) return PTRWM_E_NULL;
  if (!has_abi_size(args) || init->struct_size != sizeof(ptrwm_init_args)) return PTRWM_E_STRUCT;
  if (dim < 1 || dim > PTRWM_MAX_DIM) return PTRWM_E_DIM;
  if (!temps_in_range(args->n_temps)) return PTRWM_E_TEMPS;
  if (args->n_chains < 0 || args->n_chains > 0x7fffffffll || !is_flag(args->state_f64) || init->attempt < 0 ||
      init->attempt > 65535 || !is_flag(init->per_temperature))
    return PTRWM_E_ARG;
  if (args->n_chains == 0) return PTRWM_OK;
  if (args->state == nullptr || init->lo == nullptr || init->hi == nullptr || (init->attempt > 0 && args->logp == nullptr))
    return PTRWM_E_NULL;
  InitStatesArgs a;
  a.state = args->state;
  a.logp = args->logp;
  a.lo = init->lo;
  a.hi = init->hi;
  a.fallback = init->fallback;
  a.n_reps = args->n_chains * (long long)args->n_temps;
  a.chain_offset = args->chain_offset;
  a.n_temps = args->n_temps;
  a.dim = dim;
  a.per_temperature = init->per_temperature;
  a.attempt = init->attempt;
  a.k0 = philox_key(args->seed).k0;
  a.k1 = philox_key(args->seed).k1;
  const long long grid = (a.n_reps + 63) / 64;  // one wavefront per tile of 64 rows
  if (grid > 0x7fffffffll) return PTRWM_E_ARG;
  const unsigned lds = split_tile_lds_bytes(dim);  // (at most 26 640 bytes: within the default dynamic-LDS allowance)
  if (args->state_f64)
    hipLaunchKernelGGL(init_states_kernel<true>, dim3((unsigned)grid), dim3(64), lds, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(init_states_kernel<false>, dim3((unsigned)grid), dim3(64), lds, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? PTRWM_OK : PTRWM_E_LAUNCH;
}

int32_t ptrwm_logdensity(const ptrwm_target_desc *target, const float *x, float *out, int64_t n, void *stream) {
  if (int rc = check_target(target)) return rc;
  if (n < 0) return PTRWM_E_ARG;
  if (n == 0) return PTRWM_OK;
  if (x == nullptr || out == nullptr) return PTRWM_E_NULL;
  const int dpi = width_index_for_dim(target->dim, target->kind);
  if (dpi < 0) return PTRWM_E_DIM;
  // (RoughCarpet: the three-term functor always - the two-term one has the same bits where it applies; ThreeMixture1: a
  // different summation order, so a target declared that way is evaluated that way everywhere)
  const LogpLaunchFn fn = target_variants(target->kind, target->kind == PTRWM_TARGET_THREE_MIXTURE && target->ip[0] == 1 ? 1 : 0).logp(dpi);
  if (fn == nullptr) return PTRWM_E_NOVARIANT;
  const hipError_t err = fn(x, out, n, target->dim, make_tparams(target), (hipStream_t)stream);
  return err == hipSuccess ? PTRWM_OK : PTRWM_E_LAUNCH;
}

int32_t ptrwm_propose(const ptrwm_proposal_desc *proposal, int32_t dim, int32_t n_temps, int64_t n,
                      const float *ext_raw, uint64_t seed, float *out, void *stream) {
  if (proposal == nullptr) return PTRWM_E_NULL;
  if (proposal->kind < 0 || proposal->kind >= PTRWM_PROPOSAL_COUNT) return PTRWM_E_KIND;
  if (dim < 1 || dim > PTRWM_MAX_DIM) return PTRWM_E_DIM;
  if (!temps_in_range(n_temps)) return PTRWM_E_TEMPS;
  if (n < 0) return PTRWM_E_ARG;
  if (n == 0) return PTRWM_OK;
  if (out == nullptr || proposal->temp_scale == nullptr) return PTRWM_E_NULL;
  if (proposal->kind == PTRWM_PROPOSAL_LAPLACE && proposal->dim_scale == nullptr) return PTRWM_E_NULL;
  const int dpi = width_index_for_dim(dim);
  if (dpi < 0) return PTRWM_E_DIM;
  const PParams pp = make_pparams(proposal);
  const int n_raw = ptrwm_ext_raw_per_step(proposal->kind, dim);
  const unsigned k0 = philox_key(seed).k0, k1 = philox_key(seed).k1;
  hipError_t err;
  switch (proposal->kind) {
    case PTRWM_PROPOSAL_NORMAL:
      err = launch_propose<NormalProposal>(dpi, out, n, dim, n_temps, proposal->temp_scale, pp, ext_raw, n_raw, k0, k1, (hipStream_t)stream);
      break;
    case PTRWM_PROPOSAL_LAPLACE:
      err = launch_propose<LaplaceProposal>(dpi, out, n, dim, n_temps, proposal->temp_scale, pp, ext_raw, n_raw, k0, k1, (hipStream_t)stream);
      break;
    default:
      err = launch_propose<UniformRadiusProposal>(dpi, out, n, dim, n_temps, proposal->temp_scale, pp, ext_raw, n_raw, k0, k1, (hipStream_t)stream);
      break;
  }
  return err == hipSuccess ? PTRWM_OK : PTRWM_E_LAUNCH;
}

int32_t ptrwm_philox_raw(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, int64_t n, uint32_t *out,
                         void *stream) {
  if (n < 0) return PTRWM_E_ARG;
  if (n == 0) return PTRWM_OK;
  if (out == nullptr) return PTRWM_E_NULL;
  const unsigned grid = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(philox_raw_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, out, (long long)n, c0, c1, c2,
                     c3, philox_key(seed).k0, philox_key(seed).k1);
  return hipGetLastError() == hipSuccess ? PTRWM_OK : PTRWM_E_LAUNCH;
}

}  // extern "C"

// ptrwm_split_moments / ptrwm_split_chain_moments: the same checks, the same arguments, one of the two kernels
static int32_t split_moments_impl(const ptrwm_run_args *args, int32_t dim, const MomSpec &spec, void *stream) {
  if (int rc = split_common_checks(args, dim)) return rc;
  const ptrwm_moments_args *const m = spec.m;
  if (m == nullptr) return PTRWM_E_NULL;
  if (int rc = check_moments(args, spec)) return rc;
  if (args->n_chains == 0) return PTRWM_OK;
  if (args->state == nullptr || args->logp == nullptr) return PTRWM_E_NULL;
  if (args->device_step == nullptr && !periodic_step_due(args->step0 + 1, args->burn_in, m->every))
    return PTRWM_OK;  // (known on the host: this step does not count)
  SplitMomentsArgs a;
  a.state = args->state;
  a.logp = args->logp;
  a.sum = m->sum;
  a.sum_sq = m->sum_sq;
  a.sum_logp = m->sum_logp;
  a.count = (long long *)m->count;
  a.n_chains = args->n_chains;
  a.step = args->step0;
  a.burn_in = args->burn_in;
  a.every = m->every;
  a.device_step = (const long long *)args->device_step;
  a.n_temps = args->n_temps;
  a.dim = dim;
  a.temps = m->temps;
  // pooled: a workgroup per tile of chains; per chain: a thread per element
  const long long grid = spec.per_chain ? (args->n_chains * (long long)m->temps * dim + 255) / 256 : (args->n_chains + kSplitMomChains - 1) / kSplitMomChains;
  if (grid > 0x7fffffffll) return PTRWM_E_ARG;
  hipLaunchKernelGGL(spec.per_chain ? split_chain_moments_kernel : split_moments_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? PTRWM_OK : PTRWM_E_LAUNCH;
}
