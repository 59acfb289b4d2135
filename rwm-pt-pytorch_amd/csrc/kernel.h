// The fused PT-RWM kernel: one (chain, temperature) replica per thread, the
// temperatures of one chain contiguous inside one 64-lane wavefront.
//
// Replaces, per launch, n_steps iterations of
//   algorithms/rwm_gpu_optimized.py:289-336    (_single_step_ultra_fused, T = 1)
//   algorithms/pt_rwm_gpu_optimized.py:541-574 (step) + :594-633 (_attempt_all_swaps)
// with the replica's dim-vector, log-density and counters held in registers for
// the whole launch: HBM is touched once to load and once to store the state.
//
// Thread map.  T <= 64 ("narrow"): an exchange group is one wavefront, lane = cw * T + t (cw = chain slot within
// the wave, t = temperature), chains_per_wave = 64 / T; lanes >= chains_per_wave*T idle (only when T does not divide
// 64); a workgroup is four independent groups (measured 2 % faster than one-wave workgroups).  64 < T <= 256
// ("wide"): one ladder per workgroup of ceil(T / 64) waves, t = threadIdx.x.
// Either way a ladder lives inside one workgroup and swaps go through LDS (broadcast reads of the ladder's
// log-densities, row exchange through the staging rows), never HBM.
#pragma once
#include <cstddef>
#include <type_traits>

#include "flow.h"
#include "philox.h"
#include "proposals.h"
#include "swap_walk.h"
#include "targets.h"

namespace ptrwm {

#ifndef PTRWM_BLOCK_THREADS
#define PTRWM_BLOCK_THREADS 256
#endif
constexpr int kBlockThreads = PTRWM_BLOCK_THREADS;
constexpr int kWavesPerBlock = kBlockThreads / 64;
// The dynamic LDS of a ptrwm_step_kernel<.., DP, .., STREAM> workgroup, described ONCE: the kernel takes every pointer and
// the host (variants.h, capi.hip) every size from here.  Offsets in floats; gt = threads of the exchange group: 64 (narrow:
// a workgroup is kBlockThreads / 64 one-wave groups, kWaveFloats apart) or the workgroup (wide: one ladder, n_temps > 64).
//   classic, per group:  [rows: gt x DP][s_l][s_u][landed][c3][swap count][last event][squared-jump sums: gt doubles]
//                        behind ALL groups: [wide only: the ladder's vote word][FULL twin with moments: the regions]
//                        [FULL twin with flow: a flow region per group: the flow word of even events, of odd events, the
//                        launch's up visits, its down visits - gt ints each (flow.h)]
//   streaming, per wave: [slab 0: 64 x DP][slab 1][s_l .. squared-jump sums, gt = 64][zone 0][zone 1]
//                        zone: [64 log-densities][64 squared-jump sums (double)][64 acceptance counts (64-bit)]
// rows: up to DP floats per thread, packed (row stride = dim) for the coalesced state copy and a swap's row exchange; the
// streaming form has TWO slabs - the current group's and the one the next group's state lands in by LDS-DMA - and landing
// zones for that group's log-densities and statistics.  s_l / s_u / landed: log-density, swap uniform, outcome of a swap
// sweep.  Parked for the whole launch, touched only in swap events and the epilogue (out of the VGPR budget of the MH part:
// five VGPRs spilled to scratch otherwise, 42 MB of HBM traffic per launch): the Philox word with the temperature index,
// the accepted swaps of pair (t, t+1), the last event it accepted in, the sum of squared jumps (a double, ds_add_f64 -
// profiles/r04_scratch_ab.txt).  Vote word: a wide ladder's objection to the threshold form of a swap event.
// Between the prologue, the swap events and the epilogue the rows and the first swap-scratch words of the kernels of
// philox_heads_in_lds hold the parked heads of the thread's Philox blocks: StepLds::heads.
struct StepLdsWords {  // what does not depend on the register width
  static constexpr int kSwapWords = 3;                                  // s_l, s_u, landed
  static constexpr int kParkedInts = 3;                                 // c3, swap count, last event
  static constexpr int kExtraPerThread = kSwapWords + kParkedInts + 2;  // ... and the squared-jump sum, a double
  static constexpr int kStreamSlabs = 2;
  static constexpr int kStreamStatPerThread = 5;  // floats per thread and landing zone: a float, a double, a 64-bit integer
  static constexpr unsigned kVoteBytes = 16u;
  static constexpr unsigned kFlowLdsUnit = 8u;  // the flow regions start at a multiple of this (behind floats x whole waves, doubles)
  static constexpr int kFlowIntsPerThread = 4;  // flow region (FULL twin with flow): two word buffers, up visits, down visits
  static constexpr int kFlowUp = 2, kFlowDown = 3;  // from the region's start, in units of gt (the word buffers: 0 and 1)
  static constexpr unsigned flow_bytes(int threads) { return (unsigned)(threads * kFlowIntsPerThread) * 4u; }  // of a workgroup: one region per group
  static constexpr int floats_per_thread(int dp, bool stream) { return (stream ? kStreamSlabs * (dp + kStreamStatPerThread) : dp) + kExtraPerThread; }
  // what a launch of `threads` threads asks for (the moments regions of a FULL twin come on top)
  static constexpr unsigned bytes(int threads, int dp, bool stream, bool wide) { return (unsigned)(threads * floats_per_thread(dp, stream)) * 4u + (wide ? kVoteBytes : 0u); }
};
template <int DP, bool STREAM = false>
struct StepLds : StepLdsWords {
  static constexpr int kWaveFloats = 64 * floats_per_thread(DP, STREAM);  // the wave stride of a narrow workgroup
  static constexpr int kSlabFloats = 64 * DP;                             // streaming form: slab `cur` at cur * kSlabFloats
  static constexpr int kSlabVectorsPerLane = (kSlabFloats + 255) / 256;   // 16-byte vectors per lane that fill a slab
  static constexpr int s_l(int gt) { return STREAM ? kStreamSlabs * kSlabFloats : gt * DP; }  // these four: from the group's base (classic) / the wave's (streaming)
  static constexpr int parked(int gt) { return STREAM ? s_l(64) + kSwapWords * 64 : gt * (DP + kSwapWords); }
  static constexpr int sq_jump(int gt) { return STREAM ? s_l(64) + (kSwapWords + kParkedInts) * 64 : gt * (DP + (kSwapWords + kParkedInts)); }
  static constexpr int vote(int gt) { return gt * (DP + kExtraPerThread); }  // wide: behind the one group
  static constexpr int kSu = 1, kLanded = 2, kParked = kSwapWords, kVote = kExtraPerThread;  // from s_l, in units of gt
  static constexpr int kSwapCount = 1, kLastEvent = 2, kSqJump = kParkedInts;  // from the parked block, in units of gt (ints; doubles from there on)
  static constexpr int kZoneFloats = 64 * kStreamStatPerThread;  // streaming landing zones, from the wave's base; the arrays of a zone, from its start
  static constexpr int zone(int slab) { return s_l(64) + 64 * kExtraPerThread + slab * kZoneFloats; }
  static constexpr int kZoneLogp = 0, kZoneSqJump = 64, kZoneAccept = 64 + 2 * 64;
  // the moments regions (FULL twin), from s_dyn, behind all of the above: `stride` doubles per wave (narrow), one region for a wide ladder
  static constexpr int moments(bool wide, int gt) { return wide ? gt * (DP + kExtraPerThread) + (int)(kVoteBytes / 4u) : kBlockThreads * (DP + kExtraPerThread); }
  __device__ __forceinline__ static double *moments_region(float *s_dyn, bool wide, int gt, int wave, int stride) {
    return reinterpret_cast<double *>(s_dyn + moments(wide, gt)) + (wide ? 0 : wave * stride);
  }
  // the flow regions (FULL twin), behind the moments regions of this launch: one per wave (narrow), one for a wide ladder.
  // Where they begin is the launch's LDS size without them - the host knows it (variants.h LaunchShape) and says so in
  // KArgs::full_flow_lds, in units of kFlowLdsUnit bytes: nothing of the moments' shape is rebuilt at a swap event
  __device__ __forceinline__ static int *flow_region(float *s_dyn, bool wide, int wave, unsigned flow_lds) {
    return reinterpret_cast<int *>(s_dyn) + (int)flow_lds * (int)(kFlowLdsUnit / 4u) + (wide ? 0 : wave * (64 * kFlowIntsPerThread));
  }
  static constexpr unsigned bytes(int threads, bool wide) { return StepLdsWords::bytes(threads, DP, STREAM, wide); }
  // The parked Philox heads (philox_head.h; the kernels of philox_heads_in_lds, below): per WAVE normal_blocks(DP) blocks of
  // 64 slots of 16 bytes, block-major (proposals.h PhiloxHeadSlot), from heads(wide, wave) floats behind s_dyn.  They lie
  // OVER the rows and - width 30: 8 x 64 x 4 = 2048 words against 64 x 30 of rows - over the first words of the swap scratch
  // behind them: all dead between the prologue, the swap events and the epilogue, i.e. in nine steps of ten.  Never over the
  // parked words.  Narrow: a wave's heads lie in its own group's region, program order keeps them apart from the rows.
  // Wide: wave w's lie w * kHeadWaveWords into the one group's region, over rows and scratch words that OTHER waves read and
  // write in a swap event - the group's barrier stands between a step's last head read and the event's first store, and
  // between the event's last row read and the store of the heads.
  static constexpr int kHeadWaveWords = normal_blocks(DP) * kHeadBlockSlots * kHeadSlotWords;
  static constexpr bool kHeadsFit = !STREAM && kHeadWaveWords <= 64 * (DP + kSwapWords) && kWaveFloats % kHeadSlotWords == 0;
  static constexpr int heads(bool wide, int wave) { return wave * (wide ? kHeadWaveWords : kWaveFloats); }
  // A swap event that leaves the parked heads alone (event_keeps_heads, below: one-wavefront groups whose sweep is decided by
  // the walk) publishes its two arrays in words no head read uses, from the wave's base: the log-densities (s_l) in the 64
  // words of landed[], which the walk never writes and which lie behind the heads; the thresholds / uniforms (s_u) in the
  // spare fourth word of the slots of block 0, kKeptUStride words apart.  The rows travel through the lanes (ds_bpermute),
  // so nothing else of the event touches LDS below the parked words.
  static constexpr int kKeptL = s_l(64) + kLanded * 64;
  static constexpr int kKeptU = kHeadSlotWords - 1, kKeptUStride = kHeadSlotWords;
  static constexpr bool kKeptFit = kHeadsFit && kKeptL >= kHeadWaveWords && kKeptL + 64 <= parked(64) &&
                                   kKeptU + 63 * kKeptUStride < kHeadBlockSlots * kHeadSlotWords && kKeptU % kHeadSlotWords == 3;
};
namespace lds_check {
using C = StepLds<30>;
using S = StepLds<30, true>;
static_assert(C::s_l(256) == 256 * 30 && C::parked(256) == C::s_l(256) + C::kParked * 256 &&
                  C::sq_jump(256) == C::parked(256) + C::kSqJump * 256 && C::vote(256) == C::sq_jump(256) + 2 * 256 &&
                  C::vote(256) == C::s_l(256) + C::kVote * 256 && C::moments(true, 256) * 4 == (int)C::bytes(256, true) &&
                  C::moments(false, 64) * 4 == (int)C::bytes(kBlockThreads, false) && C::kWaveFloats == C::vote(64) && 0 < C::kSu &&
                  C::kSu < C::kLanded && C::kLanded < C::kParked && 0 < C::kSwapCount && C::kSwapCount < C::kLastEvent && C::kLastEvent < C::kSqJump,
              "classic layout: rows, swap scratch, parked ints, squared-jump doubles, vote word, moments regions: disjoint, in this order");
static_assert(S::s_l(64) == 2 * S::kSlabFloats && S::parked(64) == S::s_l(64) + 3 * 64 && S::sq_jump(64) == S::parked(64) + 3 * 64 &&
                  S::zone(0) == S::sq_jump(64) + 2 * 64 && S::zone(1) == S::zone(0) + S::kZoneFloats &&
                  S::zone(1) + S::kZoneFloats == S::kWaveFloats && S::kZoneSqJump == S::kZoneLogp + 64 &&
                  S::kZoneAccept == S::kZoneSqJump + 2 * 64 && S::kZoneAccept + 2 * 64 == S::kZoneFloats,
              "streaming layout: two slabs, swap scratch, parked words, two landing zones of three arrays");
template <int DP>  // doubles / 64-bit integers start 8-byte aligned; wave strides, slabs and landing zones (16-byte copies, DMA) 16-byte
constexpr bool aligned(bool ok = true) {
  using A = StepLds<DP>;
  using B = StepLds<DP, true>;
  for (int gt = 64; gt <= 256; gt += 64) ok = ok && A::sq_jump(gt) % 2 == 0 && A::moments(true, gt) % 2 == 0 && A::moments(false, gt) % 2 == 0;
  for (int z = 0; z < 2; ++z) ok = ok && B::zone(z) % 4 == 0 && (B::zone(z) + B::kZoneSqJump) % 4 == 0 && (B::zone(z) + B::kZoneAccept) % 4 == 0;
  return ok && A::kWaveFloats % 4 == 0 && B::kWaveFloats % 4 == 0 && B::kSlabFloats % 4 == 0 && B::sq_jump(64) % 2 == 0;
}
static_assert(aligned<2>() && aligned<3>() && aligned<5>() && aligned<9>() && aligned<29>() && aligned<30>() && aligned<50>() && aligned<64>(), "alignment");
static_assert(C::bytes(256, false) == 38912u && S::bytes(256, false) == 79872u && C::bytes(256, true) == 38928u, "LDS bytes, as before the layout had a name");
static_assert(C::kHeadsFit && C::kHeadWaveWords == 2048 && C::heads(false, 3) + C::kHeadWaveWords <= 3 * C::kWaveFloats + C::parked(64) &&
                  C::heads(true, 3) + C::kHeadWaveWords <= C::parked(256) && C::heads(true, 1) + C::kHeadWaveWords <= C::parked(128) &&
                  !StepLds<8>::kHeadsFit && !S::kHeadsFit,
              "parked heads: 16-byte slots over the rows and the swap scratch of the wave's group, below the parked words; width 8 has no room");
static_assert(C::kKeptFit && C::kKeptL == C::kHeadWaveWords && C::kKeptL + 64 == C::parked(64) && C::kKeptU == 3 && C::kKeptUStride == 4 &&
                  !StepLds<8>::kKeptFit && !S::kKeptFit && C::bytes(256, false) == 38912u,
              "an event that keeps the heads: log-densities in the landed[] words right behind the heads and below the parked words, "
              "thresholds in the spare word of block 0's slots (a head read uses words 0..2); no byte more of LDS");
static_assert(0 < C::kFlowUp &&C::kFlowUp < C::kFlowDown && C::kFlowDown < C::kFlowIntsPerThread && C::flow_bytes(256) == 4096u &&
                  C::flow_bytes(kBlockThreads) == (unsigned)kWavesPerBlock * 64u * C::kFlowIntsPerThread * 4u,
              "flow region: two word buffers, up visits, down visits, one region per group; nothing of it in a launch without flow");
}  // namespace lds_check

// Arguments only the fixture / trace variant of the kernel (FULL = true) reads.  Keeping them out
// of the production variant keeps its wave-uniform state inside the 100-odd SGPRs of a wave.
// The struct keeps its SIZE (static_assert behind KArgs): the hidden arguments of every step kernel - production and streaming
// ones too, which read the grid's and the workgroup's extent there - follow the explicit ones, so a KArgs that grows moves
// them and with them an s_load offset in kernels this struct has nothing to do with.  What is small is therefore packed: the
// countdowns and the count of a launch (at most 2^16 steps: kNoStepInLaunch stands for "none in this launch"), the two
// temperature counts, the flag; two more live in the four bytes KArgs had to spare (KArgs::full_mom_steps, full_flow_lds).  The
// raw random numbers per proposal of ext_prop are not passed at all: ext_raw_per_step(kind, dim), below.
constexpr int kNoStepInLaunch = (1 << 16) + 1;
struct FullArgs {
  const float *__restrict__ ext_prop;
  const float *__restrict__ ext_u;
  const float *__restrict__ ext_swap_u;
  float *__restrict__ trace;       // (both: at the row of this launch's first traced step - the host adds the rows before it)
  float *__restrict__ trace_logp;
  unsigned char *__restrict__ accept_flags;
  long long trace_chains;
  int trace_every;  // thinning period (>= 1)
  int mom_every;
  unsigned steps_to_trace : 17;  // steps until the first traced step of this launch (1 = the first step; kNoStepInLaunch: none)
  unsigned trace_temps : 9;
  unsigned steps_to_mom : 17;    // steps until the first step whose step_counter % mom_every == 0 (likewise)
  unsigned mom_temps : 9;
  // 1: per-chain accumulators (include/ptrwm.h ptrwm_chain_moments_args): mom_sum / mom_sum_sq are [n_chains, mom_temps, dim],
  // mom_sum_logp [n_chains, mom_temps]; the group's region has a row per (ladder of the group, temperature), is LOADED from
  // them in the prologue and stored back with plain stores (one group owns each element); mom_count[t] += mom_steps
  unsigned mom_chain : 1;
  // moments accumulator (include/ptrwm.h ptrwm_moments_args; NULL mom_sum = off): fp64 partial sums in a region of the
  // dynamic LDS per exchange group, added to at every accumulated step and flushed to HBM once at the end of the launch
  double *__restrict__ mom_sum;       // [mom_temps, dim]
  double *__restrict__ mom_sum_sq;    // [mom_temps, dim]
  double *__restrict__ mom_sum_logp;  // [mom_temps] or NULL
  long long *__restrict__ mom_count;  // [mom_temps] or NULL (KArgs::full_mom_steps: count[t] += live ladders x that)
  // replica flow (include/ptrwm.h ptrwm_flow_args, flow.h; NULL flow_walker = off): the flow word of every position is parked
  // in the group's flow region for the launch, travels with the rows in every swap event, and is stored back in the epilogue
  int *__restrict__ flow_walker;             // [n_chains, n_temps] flow words, in / out
  long long *__restrict__ flow_round_trips;  // [n_chains, n_temps] by walker id, += at event time by the thread of temperature 0; or NULL
  long long *__restrict__ flow_up;           // [n_chains, n_temps] visits by temperature, += in the epilogue; or NULL
  long long *__restrict__ flow_down;
};

typedef const __attribute__((address_space(4))) FullArgs *kargs_full_ptr;

struct KArgs {
  float *__restrict__ state;
  float *__restrict__ logp;
  const float *__restrict__ beta;
  const float *__restrict__ temp_scale;
  long long *__restrict__ n_accept;
  double *__restrict__ sq_jump;
  long long *__restrict__ swap_accept;
  long long *__restrict__ last_swap_ordinal;
  long long n_chains, chain_offset, step0;
  long long first_swap_event;  // 0-based index (since the start of the run) of the first swap event in this call
  int n_steps;                 // steps in this launch (the C ABI splits longer requests)
  int burn_left;               // steps of this launch that still belong to burn-in (step_counter <= burn_in)
  int n_temps, dim, swap_every, swap_mode, swap_order, chains_per_wave;
  int steps_to_swap;  // steps until the next step whose step_counter is a multiple of swap_every (1 = the first step)
  unsigned k0, k1;
  // (of FullArgs, in the four bytes in front of the 8-byte aligned TParams: the accumulated steps of this launch, and where
  // this launch's flow regions begin in the dynamic LDS, in units of StepLdsWords::kFlowLdsUnit bytes - set by the launcher)
  unsigned full_mom_steps : 17;
  unsigned full_flow_lds : 15;
  TParams tp;
  PParams pp;
  FullArgs full;
};
static_assert(sizeof(FullArgs) == 136 && sizeof(KArgs) == 392 && offsetof(KArgs, tp) == 144, "the kernel arguments keep their size: see FullArgs");
// what the packed fields must hold: temperature counts up to PTRWM_MAX_TEMPS (9 bits), countdowns and counts of a launch of at
// most 2^16 steps up to kNoStepInLaunch (17 bits; schedule.h max_steps_per_launch), an LDS offset up to a CU's 160 KiB (15 bits)
static_assert(PTRWM_MAX_TEMPS < (1 << 9) && kNoStepInLaunch < (1 << 17) && 160u * 1024u / StepLdsWords::kFlowLdsUnit < (1u << 15), "FullArgs bitfield widths");
// raw random numbers one proposal reads from ext_prop (include/ptrwm.h ptrwm_ext_raw_per_step): the radius word of UniformRadius
__host__ __device__ constexpr int ext_raw_per_step(int proposal_kind, int dim) { return dim + (proposal_kind == PTRWM_PROPOSAL_UNIFORM_RADIUS ? 1 : 0); }

// log swap probability exactly as fused_swap_probability_calculation evaluates it
// (algorithms/pt_rwm_gpu_optimized.py:37-48): four products summed left to right.
__device__ __forceinline__ float swap_log_prob(float bj, float bk, float lj, float lk) {
  return sub_rn(sub_rn(add_rn(mul_rn(bj, lk), mul_rn(bk, lj)), mul_rn(bj, lj)), mul_rn(bk, lk));
}

// swap_random < min(1, exp(log_prob))  (:617-621).  torch.min propagates NaN and NaN compares
// false; v_min_f32 would drop the NaN, so the clamp is a select of the threshold (one compare on the result:
// selecting between two finished compares costs the compiler four more instructions per pair).
__device__ __forceinline__ bool swap_accept_test(float u, float log_prob) {
  const float threshold = (log_prob >= 0.0f) ? 1.0f : hw_exp(log_prob);  // NaN log_prob -> NaN threshold -> false
  return u < threshold;
}

// ultra_fused_mcmc_step_basic (rwm_gpu_optimized.py:9-32) / ultra_fused_parallel_mcmc_step
// (pt_rwm_gpu_optimized.py:62-84):  r = beta (l' - l);  accept = (r > 0) | (u < exp r).  Shared by the fused step
// kernel and the split-step accept kernel.
__device__ __forceinline__ bool mh_accept(float beta_t, float lp_new, float lp, float u_acc) {
  const float ratio = mul_rn(beta_t, sub_rn(lp_new, lp));
  return (ratio > 0.0f) || (u_acc < hw_exp(ratio));
}

// The decision part of one swap event (pt_rwm_gpu_optimized.py:594-633), shared by the fused step kernel and the
// stand-alone sweep kernel (capi.hip).  In: this thread's temperature t (0 for idle threads), base = slot of
// temperature 0 of its ladder, slot = base + t, us = its swap uniform, my_l = its log-density; s_l / s_u = the
// ladder's published log-densities and uniforms (already synchronised), landed = one int of LDS scratch per slot;
// par = parity of the event (even/odd order); sync = the group's barrier (called by every thread of the group, or by
// none); plain = this thread's ladder takes the threshold form of the sequential sweep in this event (the same value on
// every thread of the ladder, below; ladders of one wavefront may differ).
// Out: my_l = the log-density that ends up at temperature t, src = the slot whose vector does, pair_acc = pair
// (t, t+1) accepted (recorded on the thread of temperature t).
//
// Sequential exchange sweep, threshold form.  The sweep j = 0..T-2 carries one state upward: at pair j the state now at
// position j (log-density c) meets the untouched state of position j+1 (log-density l_k), and the reference accepts when
//   u_j < min(1, exp((b_j - b_k)(l_k - c)))          (fused_swap_probability_calculation, :37-48, :617-621).
// For b_j > b_k (a ladder ordered cold to hot) that is   c < l_k - ln(u_j) / (b_j - b_k) =: thr_j,   and thr_j does not
// depend on the carried state: every thread computes the threshold of its own pair ONCE (one v_log_f32, one v_rcp_f32),
// publishes it in place of its uniform, and the scan that every thread of the ladder replays shrinks from four products,
// three sums, an exponential and two compares per pair to ONE compare per pair (plus the selects that carry the state):
// ~22 -> ~6 VALU instructions per pair, 4 % of BASELINE configs[2]'s instructions.  Same decisions up to rounding of the
// threshold (both forms are within a few ulp of the exact boundary; tests prove every decision that differs from the
// oracle's literal evaluation).  The reference's corner cases keep its literal rule: a LADDER in which any pair has
// b_j <= b_k, any replica enters the event with a log-density of -inf or NaN (the reference's four-product sum is then NaN
// and the swap is refused), or any pair's uniform is exactly 0 or >= 1 (ln u = -inf: the threshold would accept where
// u < exp(..) with an underflowed exponential refuses; u = 1 can never accept) takes the literal scan below - `plain`, a
// verdict of the ladder alone, taken at every event from the values it enters the event with (ladder_votes_plain): it
// cannot depend on which other ladders share the exchange group (kernel form, sharding) nor on where launches are cut.
// this thread's part of its ladder's verdict: its pair's temperatures are ordered (db = b_t - b_{t+1} > 0), its log-density
// is finite and its pair's uniform lies strictly inside (0, 1) (the last temperature has no pair: neither db nor the
// uniform is looked at).  ONE compare: u (1 - u) > 0 exactly for 0 < u < 1, lp * 0 is 0 for a finite log-density and NaN
// otherwise - three lane masks less in the SGPR file than the four compares spelt out (the run-time-dim lane-split kernels
// of the dim > 64 class live at the spilled-SGPR ceiling of tools/kernel_stats.py).
__device__ __forceinline__ bool swap_pair_plain(int T, int t, float db, float lp, float us) {
  const bool last = t >= T - 1;
  const float u = last ? 0.5f : us;
  const float d = last ? 1.0f : db;
  const float inside = mul_rn(u, sub_rn(1.0f, u));
  return add_rn(__builtin_fminf(inside, d), mul_rn(lp, 0.0f)) > 0.0f;  // (a NaN anywhere compares false)
}
// the AND of `mine` over the `lanes_per_ladder` consecutive lanes of a wavefront that start at `first_lane` (the ladder
// this thread belongs to), the same value on every one of them
__device__ __forceinline__ bool ladder_votes_plain(bool mine, int first_lane, int lanes_per_ladder) {
  const unsigned long long against = __builtin_amdgcn_ballot_w64(!mine);
  const unsigned long long ladder = (lanes_per_ladder >= 64 ? ~0ull : ((1ull << lanes_per_ladder) - 1ull)) << first_lane;
  return (against & ladder) == 0ull;
}

// Wide exchange groups (the workgroup: no ballot reaches a whole ladder): an objection is the event's own stamp (1 + its
// index in the call) in the ladder's word `word`, written together with the published values - the one barrier `sync`
// orders both, the vote has no barrier of its own - and nothing has to be armed again: the stamp of an earlier event is
// not this event's.  (The word is read for the last time before this event's row-exchange barrier, the next objection is
// written after it.)  Returns the ladder's verdict.
template <class Sync>
__device__ __forceinline__ bool wide_ladder_votes_plain(int *word, bool mine, int stamp, Sync sync) {
  if (!mine) *word = stamp;
  sync();
  return *word != stamp;
}

// This thread's pair uniform in a swap event, in its two kinds (the caller keeps the `if`: folded into one function, the
// pair moved the register allocation of 60 production kernels, profiles/r11_swap_event_once.txt).  External: row `event`
// of the caller's ext_swap_u[event, chain, T - 1] (the stand-alone sweep is event 0 of its call); the last temperature has
// no pair: 2.0, which no rule accepts.  Philox: the first word of the block of the step and chain words c0hi, c1, c2 and
// c3 = the thread's base word with the stream of the swap uniforms (rng_layout.h).
__device__ __forceinline__ float swap_uniform_ext(const float *__restrict__ ext_swap_u, long long event, long long n_chains,
                                                  long long chain, int T, int t) {
  return (t < T - 1) ? ext_swap_u[(event * n_chains + chain) * (T - 1) + t] : 2.0f;
}
__device__ __forceinline__ float swap_uniform_philox(uint32_t c0hi, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  const u32x4 r = philox4x32_10(c0hi, c1, c2, c3, k0, k1);
  return u01(r.x);
}

// The sequential scan of one ladder (slots base .. base + T - 1), from the carried state (car_l, car_i) the caller starts at
// position 0: at pair j the carried state meets the untouched one of position j + 1, and accept(j, car_l, l_k) decides -
// from a published threshold, a threshold built in place or the literal rule (swap_decide; quad.h's one-lane scan).
// Every thread that runs the scan computes the same values, so the outcome for position j (which slot's vector lands
// there) is written to LDS by all of them, identically, and each thread picks up its own position after the loop: one
// ds_write per pair instead of a compare and three selects on t == j.
// The loops stay where they are, each with its own unroll factor, and the body is a macro: as a function - a scan taking
// the rule as a functor, or this body taking the carried state by reference - it moved the register allocation of
// production kernels (profiles/r11_swap_event_once.txt).  OK: the pair accepted; IK: the slot of position j + 1, LK its
// log-density; LANDED_J: position j's outcome; CAR_L / CAR_I: the carried state.
#define PTRWM_SWAP_SCAN_PAIR(OK, IK, LK, LANDED_J, CAR_L, CAR_I) \
  do {                                                           \
    (LANDED_J) = (OK) ? (IK) : (CAR_I);                          \
    (CAR_L) = (OK) ? (CAR_L) : (LK);                             \
    (CAR_I) = (OK) ? (CAR_I) : (IK);                             \
  } while (0)

// SCAN = false: a caller whose sequential exchange sweeps never come here (the streaming step kernels that walk: narrow ladders
// only, swap_walk_decide below) compiles the scan out.
template <bool SCAN = true, class Sync>
__device__ __forceinline__ void swap_decide(int T, int t, int base, int slot, int swap_mode, int swap_order, int par,
                                            const float *__restrict__ beta, float beta_t, float us, const float *s_l,
                                            float *s_u, int *landed, float &my_l, int &src, bool &pair_acc, Sync sync,
                                            bool plain) {
  if (swap_order == PTRWM_ORDER_SEQUENTIAL) {
    if (swap_mode == PTRWM_SWAP_EXCHANGE) {
      if constexpr (!SCAN) return;
      const bool has_k = t < T - 1;
      const float db = has_k ? sub_rn(beta_t, beta[t + 1]) : 1.0f;
      float car_l = s_l[base];
      int car_i = base;
      if (plain) {
        // own pair's threshold in place of its uniform (u = 0: ln = -inf, threshold +inf: accepted, as u < exp(..) is)
        const float lk = s_l[has_k ? slot + 1 : slot];
        s_u[slot] = fmaf(-hw_ln(us), __builtin_amdgcn_rcpf(db), lk);
        sync();
#pragma unroll 2
        for (int j = 0; j < T - 1; ++j) {
          const int ik = base + j + 1;
          const float lkj = s_l[ik];
          const bool ok = car_l < s_u[base + j];
          PTRWM_SWAP_SCAN_PAIR(ok, ik, lkj, landed[base + j], car_l, car_i);
        }
      } else {
        // the literal scan: every thread of the ladder replays the sweep from the published original values (uniform
        // addresses: LDS broadcasts, no dependent cross-lane traffic) and keeps what lands on its own position
#pragma unroll 2
        for (int j = 0; j < T - 1; ++j) {
          const float lk = s_l[base + j + 1];
          const float u = s_u[base + j];
          const float bj = beta[j], bk = beta[j + 1];
          const bool ok = swap_accept_test(u, swap_log_prob(bj, bk, car_l, lk));
          const int ik = base + j + 1;
          PTRWM_SWAP_SCAN_PAIR(ok, ik, lk, landed[base + j], car_l, car_i);
        }
      }
      landed[base + T - 1] = car_i;
      // (a wave's LDS operations complete in program order, and every wave of a wide ladder writes all positions
      // itself before reading its own: no barrier needed)
      src = landed[base + t];
      my_l = s_l[src];  // log-densities travel with the states: s_l still holds the originals
      pair_acc = (t < T - 1) && (src == base + t + 1);
    } else {
      // reference_copy: row j <- row k, row k untouched, so every pair compares the original rows j and j+1:
      // no carried state, fully parallel.
      if (t < T - 1) {
        const float lk = s_l[slot + 1];
        const bool ok = swap_accept_test(us, swap_log_prob(beta_t, beta[t + 1], my_l, lk));
        if (ok) {
          my_l = lk;
          src = slot + 1;
        }
        pair_acc = ok;
      }
    }
  } else {
    // even/odd: event n attempts the disjoint pairs (j, j+1) with j == n (mod 2)
    const bool lower = ((t & 1) == par);          // this thread is the lower index j of its pair
    const int partner_t = lower ? t + 1 : t - 1;
    const bool valid = partner_t >= 0 && partner_t < T;
    if (valid) {
      const int partner = base + partner_t;
      const float l_other = s_l[partner];
      const float u_low = lower ? us : s_u[partner];
      const int tj = lower ? t : partner_t;
      const float lj = lower ? my_l : l_other;
      const float lk = lower ? l_other : my_l;
      const bool ok = swap_accept_test(u_low, swap_log_prob(beta[tj], beta[tj + 1], lj, lk));
      if (ok && (lower || swap_mode == PTRWM_SWAP_EXCHANGE)) {
        my_l = l_other;
        src = partner;
      }
      pair_acc = ok && lower;
    }
  }
}

// The sequential exchange sweep of an exchange group that is ONE wavefront (T <= 64: the step kernel's narrow groups), by
// lane masks and a scalar walk (swap_walk.h) instead of the scan above, which every lane of a ladder replays: 64 lanes then
// compute the same T - 1 decisions - a compare, three selects and a ds_write per pair on the vector unit that bounds the
// kernel - while the scalar unit idles.  Here lane k answers, per pair j, ONE question about its own published log-density
// my_l: would it be accepted at pair j of its ladder, were it the carried state?  The ballot of the answers is a wave-uniform
// word, the walk over the words runs on the scalar unit for all ladders of the wavefront at once, and every lane reads its
// outcome from the walk's `rejected` word once.  Same compares on the same values as the scan: same decisions, bit for bit.
// In / out as swap_decide; every lane of the wavefront calls it (idle lanes shadow position 0 of ladder 0, as there).
// plain (the ladder's verdict, swap_decide): the threshold form - own pair's threshold published in place of its uniform,
// the question is my_l < thr_j.  A ladder that must take the literal rule asks swap_accept_test(u_j, swap_log_prob(b_j,
// b_j+1, my_l, l_j+1)) instead - also a function of (carrier, j) alone.  The rule is chosen per LADDER: a wavefront with a
// literal ladder anywhere runs the loop in which every lane selects its own ladder's answer (cold: corner cases only), and a
// plain ladder's answers there are the compares of the fast loop.
// SU: the stride of s_u in words (an event that keeps the parked heads publishes it in the spare word of 16-byte slots,
// StepLds::kKeptU).
// LEAN (the fixture twins, whose speed nobody measures): the one general loop only - the library's size budget
// (tools/kernel_stats.py --size) has no room for a fast loop in every twin.
template <bool LEAN, int SU = 1, class Sync>
__device__ __forceinline__ void swap_walk_decide(int T, int t, int base, int slot, const float *__restrict__ beta, float db,
                                                 float us, const float *s_l, float *s_u, float &my_l, int &src, bool &pair_acc,
                                                 Sync sync, bool plain) {
  const bool has_k = t < T - 1;
  if (plain) {
    // own pair's threshold in place of its uniform (swap_decide)
    const float lk = s_l[has_k ? slot + 1 : slot];
    s_u[slot * SU] = fmaf(-hw_ln(us), __builtin_amdgcn_rcpf(db), lk);  // (the last position's: b_t - b_t = 0, read by no pair)
  }
  sync();
  const uint64_t seg0 = __builtin_amdgcn_ballot_w64(slot == base);  // (an idle lane's base is 0; lane 0 is never idle)
  const float *const pair = s_u + base * SU;  // pair j of this lane's ladder: one address, j an immediate offset
  const bool all_plain = __builtin_amdgcn_ballot_w64(!plain) == 0ull;
  SwapWalk w = swap_walk_begin(seg0);
  int j = 0;
  if constexpr (!LEAN) {
    // the fast loop: one ds_read2 and two compares per trip on the vector unit, the rest scalar.  (Two pairs per trip written
    // out: a ballot is a convergent operation, and the compiler unrolls no loop of a run-time trip count around one.)
    if (all_plain)
      for (; j + 2 <= T - 1; j += 2) {
        swap_walk_step(w, seg0, j, __builtin_amdgcn_ballot_w64(my_l < pair[j * SU]));
        swap_walk_step(w, seg0, j + 1, __builtin_amdgcn_ballot_w64(my_l < pair[(j + 1) * SU]));
      }
  }
  // the general loop: the fast loop's odd last pair; the whole sweep of a wavefront with a literal ladder, or of a LEAN kernel
#pragma unroll 1
  for (; j < T - 1; ++j) {
    const float v = pair[j * SU];  // the pair's threshold (plain ladders) or its uniform
    bool ok = my_l < v;
    if (!all_plain) {
      PTRWM_COLD_PATH();
      const bool literal = swap_accept_test(v, swap_log_prob(beta[j], beta[j + 1], my_l, s_l[base + j + 1]));
      ok = plain ? ok : literal;
    }
    swap_walk_step(w, seg0, j, __builtin_amdgcn_ballot_w64(ok));
  }
  src = swap_walk_source(w.rejected, seg0, base + t, has_k, pair_acc);
  my_l = s_l[src];  // log-densities travel with the states: s_l still holds the originals
}

// Staging between a group's contiguous run of `total` floats in HBM (`g`, any 4-byte alignment) and its LDS slab, 16 bytes
// per lane per instruction (global_load_dwordx4 / ds_write_b128 and the reverse).  Element i of the run lives at
// lds[stage_head(g) + i], stage_head = the run's first float index modulo 4: an aligned 16-byte vector of HBM is then an
// aligned 16-byte vector of the slab (slabs start 256-byte aligned), so whole vectors move as vectors; the <= 3 elements
// before the first and after the last whole vector are moved one by one.  The slab needs room for total + 3 floats: the
// rows fill it exactly when every slot is live and dim equals the register width, and the overhang then lands in the
// swap scratch behind the rows, which is dead while a copy runs.
// Four independent vectors in flight per lane: full chunks unpredicated, then one predicated chunk.  (A plain loop waits
// for every load before issuing the next one when the stride is a run-time value: 1.7x slower for one step per launch.)
__device__ __forceinline__ int stage_head(const float *g) { return (int)((reinterpret_cast<uintptr_t>(g) >> 2) & 3u); }

template <bool LOAD>  // LOAD: HBM -> LDS, else LDS -> HBM
__device__ __forceinline__ void stage_copy(float *__restrict__ lds, float *__restrict__ g, int total, int tid, int nthr) {
  typedef float vec4 __attribute__((ext_vector_type(4)));
  const int head = stage_head(g);
  vec4 *__restrict__ gv = reinterpret_cast<vec4 *>(g - head);  // the aligned frame; vector 0 is touched only if head == 0
  vec4 *__restrict__ lv = reinterpret_cast<vec4 *>(lds);
  const int v_lo = head ? 1 : 0;          // first whole vector
  const int v_hi = (head + total) >> 2;   // one past the last whole vector
  constexpr int kDepth = 4;
  int v0 = v_lo + tid;
  for (; v0 + (kDepth - 1) * nthr < v_hi; v0 += kDepth * nthr) {
    vec4 t[kDepth];
#pragma unroll
    for (int k = 0; k < kDepth; ++k) t[k] = LOAD ? gv[v0 + k * nthr] : lv[v0 + k * nthr];
#pragma unroll
    for (int k = 0; k < kDepth; ++k) (LOAD ? lv : gv)[v0 + k * nthr] = t[k];
  }
  if (v0 < v_hi) {
    vec4 t[kDepth - 1];
#pragma unroll
    for (int k = 0; k < kDepth - 1; ++k) {
      const int v = v0 + k * nthr;
      if (v < v_hi) t[k] = LOAD ? gv[v] : lv[v];
    }
#pragma unroll
    for (int k = 0; k < kDepth - 1; ++k) {
      const int v = v0 + k * nthr;
      if (v < v_hi) (LOAD ? lv : gv)[v] = t[k];
    }
  }
  // the ragged ends: elements [0, e_lo) before the first whole vector and [e_hi, total) after the last one
  const int e_lo = (4 * v_lo - head < total) ? 4 * v_lo - head : total;
  const int e_hi = (4 * v_hi - head > e_lo) ? 4 * v_hi - head : e_lo;
  if (tid < 6) {
    const int i = tid < 3 ? tid : e_hi + (tid - 3);
    const bool mine = tid < 3 ? (i < e_lo) : (i < total);
    if (mine) {
      if (LOAD) lds[head + i] = g[i];
      else g[i] = lds[head + i];
    }
  }
}

// The thread's index in its (one-dimensional) workgroup, re-derived from the hardware where it is needed - the lane from
// v_mbcnt, the wave's index in the workgroup from an SGPR set once at kernel entry (lanes fill the waves of a 1-D workgroup
// in order) - so that neither threadIdx.x nor anything computed from it has to live in a VGPR, i.e. in scratch, across the
// step loop: at the 128-VGPR cap the allocator spilled it and four words derived from it (28 B of scratch per thread,
// 13 % of a launch's HBM traffic at 2 000 steps per launch).  Used by the swap path and the epilogue alike: with the
// epilogue alone re-deriving it the headline kernel ran 2 % slower (95.1 against 93.1 ms per 2 000-step launch, same box,
// profiles/r03_scratch_ab.txt) - register allocation at the cap is that sensitive; candidates are A/B-timed.
__device__ __forceinline__ int wave_in_block() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }
__device__ __forceinline__ int thread_index_now(int wave) {
  unsigned all = ~0u;
  PTRWM_VALUE_BARRIER("+s"(all));  // (v_mbcnt is pure: without this it is computed once, before the loop, and kept)
  return wave * 64 + (int)__builtin_amdgcn_mbcnt_hi(all, __builtin_amdgcn_mbcnt_lo(all, 0u));
}

// `*p += v` for an integer statistic that this thread alone updates, as a no-return atomic executed at the L2
// (global_atomic_add_x2): the same sum without a load, a dependent add and a store at the very end of a wave's life - the
// tail that keeps the wave's slot occupied in short launches (one step per launch: 0.130 -> 0.125 ms; long launches: no
// change).  The double sum of squared jumps stays a read-modify-write: a hardware fp64 atomic would do the same for another
// 1 %, but is not guaranteed on every kind of device allocation a caller of the C ABI may hand in.
__device__ __forceinline__ void count_add(long long *p, long long v) {
  (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The moments region of one exchange group: [rows * dim] sums of x, [rows * dim] sums of x^2, [rows] sums of the
// log-density, as doubles, behind everything else the kernel keeps in its dynamic LDS.  One region per group:
// narrow groups (one wave) never meet at a workgroup barrier, so they cannot share one.
constexpr unsigned moments_region_doubles(int rows, int dim) { return (unsigned)(rows * (2 * dim + 1)); }
// Rows of a region: pooled, one per covered temperature; per chain (FullArgs::mom_chain), one per (ladder of the exchange
// group, covered temperature), row = ladder * temps + t - kernel and host (variants.h with_moments) size the region from here
constexpr int moments_rows(bool per_chain, int ladders_per_group, int temps) { return per_chain ? ladders_per_group * temps : temps; }

// ds_add_f64: lanes of one wave with equal temperature (the ladders of a narrow group) hit the same address - the LDS
// atomic unit serialises them
__device__ __forceinline__ void moments_add(double *p, double v) {
  (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// The accumulator of one exchange group (FULL twins of both step kernels): the one place that knows the rows and the three
// sub-arrays of a region, and how the pooled and the per-chain kind (FullArgs::mom_chain) differ - in the row a thread adds
// to, and in how the region starts and ends a launch.  `reg` is set from the layout (StepLds / QuadLds::moments_region, which
// places a narrow group's region by doubles()).  The arguments come as a pointer: &a.full in the prologue and the step,
// late_args() in the epilogue (loaded there, not held across the step loop).
struct MomentsAcc {
  double *reg = nullptr;
  int temps, rows, dim;
  bool per_chain;
  struct Row { double *sum, *sum_sq, *logp; };

  template <class F>
  __device__ __forceinline__ MomentsAcc(F f, int ladders_per_group, int dim_)
      : temps(f->mom_temps), rows(moments_rows(f->mom_chain != 0, ladders_per_group, temps)), dim(dim_), per_chain(f->mom_chain != 0) {}
  __device__ __forceinline__ int doubles() const { return (int)moments_region_doubles(rows, dim); }
  // where the replica at (ladder cw of the group, temperature t < temps) adds: sum[d], sum_sq[d], d < dim, and *logp
  __device__ __forceinline__ Row row(int cw, int t) const {
    const int r = per_chain ? cw * temps + t : t;
    return {reg + r * dim, reg + (rows + r) * dim, reg + 2 * rows * dim + r};
  }
  // Per chain, the region's live rows and the group's part of the global arrays are the same contiguous runs (row0 = first
  // chain of the group x temps).  LOAD: global -> region - each element then is the sequential fp64 sum over ALL steps so
  // far, wherever launches are cut; else region -> global, plain 8-byte stores: no other group touches these elements.
  template <bool LOAD, class F>
  __device__ __forceinline__ void chain_copy(F f, int live_ladders, long long chain0, int tid, int nthr) const {
    const int live_rows = live_ladders * temps, n = live_rows * dim, rd = rows * dim;
    const long long row0 = chain0 * temps;
    double *const sum_logp = f->mom_sum_logp, *const gs = f->mom_sum + row0 * dim, *const gq = f->mom_sum_sq + row0 * dim;
    for (int i = tid; i < n; i += nthr) {
      if (LOAD) reg[i] = gs[i], reg[rd + i] = gq[i];
      else gs[i] = reg[i], gq[i] = reg[rd + i];
    }
    if (sum_logp != nullptr)
      for (int i = tid; i < live_rows; i += nthr) {
        if (LOAD) reg[2 * rd + i] = sum_logp[row0 + i];
        else sum_logp[row0 + i] = reg[2 * rd + i];
      }
  }
  // prologue (ordered before the first add by the group's barrier): per chain the region is loaded, pooled it starts at zero
  template <class F>
  __device__ __forceinline__ void begin(F f, int live_ladders, long long chain0, int tid, int nthr) const {
    if (per_chain) chain_copy<true>(f, live_ladders, chain0, tid, nthr);
    else
      for (int i = tid; i < doubles(); i += nthr) reg[i] = 0.0;
  }
  // epilogue, behind the barrier after the launch's last add.  Per chain: stored back, and the group of chain 0 counts the
  // steps per chain.  Pooled: one no-return global_atomic_add_f64 per non-zero partial sum (device memory: include/ptrwm.h)
  // and count[t] += live ladders x steps.
  template <class F>
  __device__ __forceinline__ void end(F f, long long mom_steps, long long live_ladders, long long chain0, int tid, int nthr) const {
    long long *const count = f->mom_count;
    if (per_chain) {
      chain_copy<false>(f, (int)live_ladders, chain0, tid, nthr);
      if (chain0 != 0) return;
    } else {
      const int td = temps * dim;
      double *const sum = f->mom_sum, *const sum_sq = f->mom_sum_sq, *const sum_logp = f->mom_sum_logp;
      const int n = 2 * td + (sum_logp != nullptr ? temps : 0);
      for (int i = tid; i < n; i += nthr) {
        const double v = reg[i];
        if (v != 0.0) unsafeAtomicAdd(i < td ? sum + i : (i < 2 * td ? sum_sq + (i - td) : sum_logp + (i - 2 * td)), v);
      }
    }
    const long long add = (per_chain ? 1 : live_ladders) * mom_steps;
    if (count != nullptr)
      for (int i = tid; i < temps; i += nthr) count_add(&count[i], add);
  }
};

// The wave-uniform thinning countdowns of the FULL twins (trace rows, accumulated steps): true at every period-th step
__device__ __forceinline__ bool countdown_due(int &left, int period) {
  --left;
  const bool due = (left == 0);
  if (due) left = period;
  return due;
}

template <bool EXACT>
__device__ __forceinline__ int fresh_dim(int d0) {
  if constexpr (!EXACT) PTRWM_VALUE_BARRIER("+s"(d0));
  return d0;
}

// The kernel's arguments as they sit in the kernarg segment (KArgs is the kernel's only parameter: offset 0), through a
// pointer the optimiser cannot relate to `a`: what is read through it is loaded where it is used - one s_load in the
// epilogue - instead of being loaded at kernel entry and held in SGPRs, i.e. in spill lanes, across the whole step loop
// (the epilogue alone needs eight pointers and three scalars: ~20 SGPRs of the 102 a wave has).
typedef const __attribute__((address_space(4))) KArgs *kargs_ptr;
__device__ __forceinline__ kargs_ptr late_args() {
  uintptr_t p = (uintptr_t)__builtin_amdgcn_kernarg_segment_ptr();
  PTRWM_VALUE_BARRIER("+s"(p));
  return (kargs_ptr)p;
}

// Register budget: the replica's x[DP] and y[DP] plus ~30 temporaries must stay in VGPRs.  Without a
// bound hipcc hoists every Philox block of a step ahead of its consumers and lands far above that.
#ifndef PTRWM_J2_FENCE_MASK  // fence cadence of the update / squared-jump loop (A/B-timed, tools/ab_bench.sh)
#define PTRWM_J2_FENCE_MASK 7
#endif
#ifndef PTRWM_WAVES_SMALL  // tuning knobs (profiles/r01_bench_variants.txt: 4 beats 3, 5 and 6 at dim 30)
#define PTRWM_WAVES_SMALL 4
#endif
#ifndef PTRWM_WAVES_40
#define PTRWM_WAVES_40 3
#endif
#ifndef PTRWM_WAVES_MID
#define PTRWM_WAVES_MID 2
#endif
// (Width 40 at 4 waves/SIMD spilled ~75 VGPRs; 3 waves/SIMD = 168 VGPRs holds it.  The generic width 32 sat at 125 of the
// 128 VGPRs that 4 waves/SIMD allow and spilled two of them to scratch once the swap event grew its threshold form: it
// is compiled for 3 waves/SIMD as well - dims 31 and 32 run at ~0.97 of the 4-wave rate (profiles/r03_form_sweep_dense.txt,
// A(3)), everything up to the exact width 30 keeps 4.)
constexpr int min_waves_per_simd(int dp) {
  return dp <= 30 ? PTRWM_WAVES_SMALL : (dp <= 44 ? PTRWM_WAVES_40 : (dp <= 64 ? PTRWM_WAVES_MID : 1));
}
// the widths whose step loop fills the 128 VGPRs of four waves per SIMD (in the shipped table: the compiled-in dim 30, and 29
// for HybridRosenbrock): what is loop-invariant there is recomputed rather than kept (ptrwm_step_kernel, the chain word)
constexpr bool step_loop_at_register_cap(int dp, bool stream) { return !stream && min_waves_per_simd(dp) >= 4 && dp > 24; }

// Which step kernels park the step-invariant heads of their Philox blocks in LDS (philox_head.h, StepLds::heads) and enter
// every block at round 2: the production thread-form kernel of the compiled-in width 30 with the Normal proposal - the
// headline shape, whose step loop is bound by VALU issue while LDS idles.  The heads live in LDS, never in registers: held
// in VGPRs (24 of them) that kernel spills 16, and at five waves per SIMD 45.  FULL twins, the streaming form and the
// lane-split kernels keep the plain block; so does every other width and proposal until it is measured.
constexpr bool philox_heads_in_lds(int dp, bool exact, bool full, bool stream, int proposal_kind) {
  return !full && !stream && exact && dp == 30 && proposal_kind == PTRWM_PROPOSAL_NORMAL;
}

// The streaming form (STREAM, below) keeps two slabs of rows per wave in LDS: fewer waves per SIMD fit (and each gets the
// registers of that residency).
constexpr int stream_waves_per_simd(int dp) {  // what two slabs per wave leave room for in 160 KB of LDS per CU, at most 4
  return dp <= 10 ? 4 : (dp <= 20 ? 2 : (dp <= 30 ? 2 : 1));
}

// (the register budget it is compiled for: never that of ONE wave per SIMD - 512 registers invite AGPR copies, the regime
// tools/kernel_stats.py --check keeps every kernel out of - even where LDS admits no second wave)
constexpr int stream_register_waves(int dp) { return stream_waves_per_simd(dp) < 2 ? 2 : stream_waves_per_simd(dp); }

// Which step kernels decide the sequential exchange sweep of their one-wavefront groups by the walk (swap_walk_decide): the
// widths up to 44, compiled for three or four waves per SIMD.  The wider ones already keep 40 to 150 scalars spilled in VGPR
// lanes, and the six scalar registers the walk holds across its loop cost them more than the scan's selects: with the walk
// the width-50 kernel of BASELINE configs[4] spilled 44 SGPRs instead of 40 and ran 0.8 % SLOWER (503.4 against 499.4 ms per
// launch, three alternating runs each, no overlap), and the streaming twin of Hypercube<50> with the UniformRadius proposal
// went one above the spilled-SGPR ratchet of tools/kernel_stats.py (129, ceiling 128; 117 with the scan).  They keep the
// scan, and their machine code (profiles/r16_swap_walk.txt).
constexpr bool swap_walk_in_kernel(int dp) { return dp <= 44; }

// Which step kernels leave their parked heads alone in a swap event: those that park them, in the events of a one-wavefront
// group that the walk decides (sequential order, exchange mode - a run-time condition of the launch, ptrwm_step_kernel).
// Nothing a head depends on changes in an event - chain word, temperature index, key, step >> 32: states move between threads,
// temperatures do not - so the only reason to rebuild them was that the event wrote over them.  Such an event publishes its two
// arrays beside the heads (StepLds::kKeptL / kKeptU) and moves the rows through the lanes: one ds_bpermute_b32 per dimension
// - the LDS pipe, but no LDS memory, and local to the wavefront: no barrier - in place of a ds_write, a barrier and a ds_read.
// Wide ladders, even_odd order and reference_copy mode keep the slab exchange and the restore behind it.
constexpr bool event_keeps_heads(int dp, bool exact, bool full, bool stream, int proposal_kind) {
  return philox_heads_in_lds(dp, exact, full, stream, proposal_kind) && swap_walk_in_kernel(dp);
}
// Which step kernels carry the thread's lane index in ONE VGPR across the step loop and take the head slot, the squared-jump
// slot and the event's slots from it, instead of rebuilding it from v_mbcnt at each of the three (thread_index_now: written
// when these kernels sat at 127 of 128 VGPRs; with the heads parked they have a dozen to spare).  The kernels of
// philox_heads_in_lds; the others keep the rebuilds, and their machine code, until they are measured.
constexpr bool lane_index_carried(int dp, bool exact, bool full, bool stream, int proposal_kind) {
  return philox_heads_in_lds(dp, exact, full, stream, proposal_kind);
}

// threads of this kernel's exchange group (rng_layout.h; the streaming form serves narrow ladders only: one wave, folded)
template <bool STREAM>
__device__ __forceinline__ int step_group_threads(int T) { return STREAM ? 64 : group_threads(T, 1); }

// Rows of the FULL twins' per-step arrays (both step kernels).  The replica's index in step i of the launch - the row of
// accept_flags and ext_u, and of ext_prop in units of n_raw_ext elements; the row of the trace (from its first) a launch that has already
// written rows_written rows writes for (chain, t).
__device__ __forceinline__ long long step_replica_index(int i, long long n_chains, long long chain, int T, int t) {
  return ((long long)i * n_chains + chain) * T + t;
}
template <class F>  // (words: 32-bit words per element of ext_prop - 2 for the double states of the lane-split form)
__device__ __forceinline__ const float *ext_prop_row(F f, int n_raw_ext, long long srep, int words) {
  return f->ext_prop + srep * n_raw_ext * words;
}
template <class F>
__device__ __forceinline__ long long trace_row_index(F f, int rows_written, long long chain, int t) {
  return ((long long)rows_written * f->trace_chains + chain) * (long long)f->trace_temps + t;
}

// DP    compile-time width of the per-thread register arrays (>= dim)
// EXACT dim == DP is known at compile time: every per-dimension predicate folds away.  Otherwise
//       dim is a wave-uniform run-time value, re-read (opaquely) every step so the compiler tests
//       `d < dim` with one scalar compare in place instead of hoisting DP booleans into SGPRs.
// FULL  fixture/trace variant: external randoms, per-step trace and accept-flag outputs.
template <class Target, class Proposal, int DP, bool EXACT, bool FULL, bool STREAM = false>
__global__ void __launch_bounds__(kBlockThreads, STREAM ? stream_register_waves(DP) : min_waves_per_simd(DP)) ptrwm_step_kernel(const KArgs a) {
  static_assert(!(STREAM && FULL), "the streaming form is a production kernel: no fixture / trace arguments");
  const int T = a.n_temps;
  const int D0 = EXACT ? DP : a.dim;
  const int cpw = a.chains_per_wave;
  // An exchange group is one wavefront holding cpw = 64 / T whole ladders (T <= 64, "narrow": a workgroup is four
  // independent groups), or ceil(T / 64) wavefronts = the whole workgroup holding one ladder ("wide", cpw = 1).
  // Thread tid of its group is (cw, t) with tid = cw * T + t either way.
  const bool wide = !STREAM && T > 64;  // grid-uniform (the streaming form serves narrow ladders only)
  const int wave = wave_in_block();  // (an SGPR for the whole launch: thread_index_now)
  const int tid = wide ? (int)threadIdx.x : (int)(threadIdx.x & 63);
  // The group this wave (narrow) / workgroup (wide) works on.  Classic form: one group per wave, fixed by the grid.
  // Streaming form: the grid is sized to the device (capi.hip) and every wave walks the groups gw, gw + stride, ... with
  // the NEXT group's state, log-densities and squared-jump sums already on their way from HBM while it computes (below).
  // (the classic form derives it from threadIdx.x, as it always did: its register allocation at the 128-VGPR cap follows
  // every such detail; the streaming form carries it across groups in scalar registers)
  long long group = STREAM ? (long long)blockIdx.x * kWavesPerBlock + wave
                           : (wide ? (long long)blockIdx.x : (long long)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
  [[maybe_unused]] const long long n_groups = STREAM ? a.n_chains / cpw : 0;  // (streaming: every group is whole, capi.hip)
  [[maybe_unused]] const long long group_stride = STREAM ? (long long)gridDim.x * kWavesPerBlock : 0;
  if (STREAM ? (group >= n_groups) : (group * cpw >= a.n_chains)) return;  // narrow only (wave-uniform; narrow waves never meet at a workgroup barrier)
  extern __shared__ __attribute__((aligned(16))) float s_dyn[];
  // ---- streaming form: LDS-DMA double buffering ---------------------------------------------------------------------
  // A group's state is one run of cpw * T * dim floats, 16-byte aligned and a whole number of 16-byte vectors (capi.hip
  // takes the classic kernel otherwise).  Each wave owns TWO slabs: while the group in slab `cur` is being stepped, the
  // next group's run is on its way from HBM straight into the other slab (global_load_lds_dwordx4: 1 KiB per wave
  // instruction, no VGPR destination - the step keeps every register it has in the classic kernel), issued right after
  // the current group's rows have been picked up and waited for (a counted vmcnt placed by the compiler: the builtin is
  // a tracked memory operation) only when the next group's rows are read - the current group's stores, issued later,
  // stay in flight behind it.  HBM reads, the Metropolis step and HBM writes of different groups overlap inside ONE
  // wave, not only across waves.  The next group's log-densities and squared-jump sums travel the same way into two
  // small landing zones: an ordinary load to a VGPR anywhere in this loop would make the compiler drain every
  // outstanding DMA and store (vmcnt(0)) at its first use.
  typedef float pf_vec4 __attribute__((ext_vector_type(4)));
  typedef StepLds<DP, STREAM> L;  // where everything in the dynamic LDS lives
  constexpr int NV = STREAM ? L::kSlabVectorsPerLane : 1;  // 16-byte vectors per lane and group
  constexpr int kWaveFloats = L::kWaveFloats;
  [[maybe_unused]] int cur = 0;  // which slab / landing zone holds the current group (streaming form; wave-uniform)
  typedef const __attribute__((address_space(1))) void *dma_src;
  typedef __attribute__((address_space(3))) void *dma_dst;
  [[maybe_unused]] auto prefetch = [&](long long g, int slab) {
    const int tid = thread_index_now(wave) & 63;  // (re-derived: no per-lane address parts kept, or spilled, across the step)
    const kargs_ptr ap = late_args();             // (and the array pointers are loaded here, not held in SGPRs across it)
    const int n_vec = (cpw * T * D0) >> 2;
    const int n_live = cpw * T;
    float *const wbase = s_dyn + wave * kWaveFloats;
    // log-densities: one dword per lane (idle lanes re-read replica 0 of the group)
    const long long r0 = g * n_live;
    float *const zone = wbase + L::zone(slab);
    __builtin_amdgcn_global_load_lds((dma_src)(ap->logp + r0 + (tid < n_live ? tid : 0)), (dma_dst)(uintptr_t)(zone + L::kZoneLogp), 4, 0, 0);
    // squared-jump sums: 16 bytes = two doubles per lane (n_live is even, capi.hip)
    if (ap->sq_jump != nullptr && 2 * tid < n_live)
      __builtin_amdgcn_global_load_lds((dma_src)(ap->sq_jump + r0 + 2 * tid), (dma_dst)(uintptr_t)(zone + L::kZoneSqJump), 16, 0, 0);
    // acceptance counts likewise: read ahead and stored back as old + delta.  (The classic kernel adds them by no-return
    // atomics to keep a load off the end of a wave's life; here the old value is in LDS before the step begins, and plain
    // 8-byte stores stream at several times the rate the memory-side atomics do.)
    if (ap->n_accept != nullptr && 2 * tid < n_live)
      __builtin_amdgcn_global_load_lds((dma_src)(ap->n_accept + r0 + 2 * tid), (dma_dst)(uintptr_t)(zone + L::kZoneAccept), 16, 0, 0);
    const pf_vec4 *__restrict__ gv = reinterpret_cast<const pf_vec4 *>(ap->state + g * cpw * T * (long long)D0);
    float *const dst = wbase + slab * L::kSlabFloats;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int v = tid + 64 * k;
      if (v < n_vec) __builtin_amdgcn_global_load_lds((dma_src)(gv + v), (dma_dst)(uintptr_t)(dst + 256 * k), 16, 0, 0);
    }
  };
  // (streaming form: what depends on the thread's temperature only is loaded ONCE, before the first DMA is issued - any
  // ordinary global load behind an LDS-DMA makes the compiler drain the DMA at the load's first use, which would put the
  // next group's HBM latency back in front of the current group's step)
  [[maybe_unused]] float beta_t_s = 0.0f, tscale_s = 0.0f;
  [[maybe_unused]] float db_s = 1.0f;  // b_t - b_{t+1} of this thread's pair (swap_pair_plain)
  // Outgoing results of the group just finished wait in registers until the NEXT group's rows have been picked up, and
  // are stored then (flush_pending): at the top of an iteration the only vector-memory operations that can still be
  // outstanding are the DMA of the group about to be stepped and the stores issued a whole step earlier - so the wait for
  // the DMA is a plain vmcnt(0) that never waits for a store just issued.
  [[maybe_unused]] pf_vec4 pend_o[NV];
  [[maybe_unused]] float pend_lp = 0.0f;
  [[maybe_unused]] unsigned pend_n_swap = 0u;
  [[maybe_unused]] long long pend_acc = 0;
  [[maybe_unused]] bool pend_acc_on = false;
  [[maybe_unused]] double pend_sq = 0.0;
  [[maybe_unused]] long long pend_ord = 0, pend_group = 0;
  [[maybe_unused]] bool pend_sq_on = false, pend_ord_on = false, have_pending = false;
  [[maybe_unused]] auto flush_pending = [&]() {
    const kargs_ptr ap = late_args();
    const int tid = thread_index_now(wave) & 63;
    const int n_live = cpw * T;
    const int n_vec = (n_live * D0) >> 2;
    pf_vec4 *__restrict__ gv = reinterpret_cast<pf_vec4 *>(ap->state + pend_group * n_live * (long long)D0);
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int v = tid + 64 * k;
      if (v < n_vec) gv[v] = pend_o[k];
    }
    if (tid < n_live) {
      const long long r = pend_group * n_live + tid;
      ap->logp[r] = pend_lp;
      // statistics: only where the launch has something to add (kernel epilogue below)
      if (pend_acc_on) ap->n_accept[r] = pend_acc;
      if (pend_sq_on) ap->sq_jump[r] = pend_sq;
      if (ap->swap_accept != nullptr && pend_n_swap != 0u) count_add(&ap->swap_accept[r], (long long)pend_n_swap);
      // (the same maximum as the classic kernel's compare-and-store, as a no-return atomic at the L2: no load)
      if (pend_ord_on) (void)__hip_atomic_fetch_max(&ap->last_swap_ordinal[r], pend_ord, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  };
  if constexpr (STREAM) {
    const int cw_s = tid / T;
    const int t_s = cw_s < cpw ? tid - cw_s * T : 0;
    beta_t_s = a.beta[t_s];
    tscale_s = a.temp_scale[t_s];
    db_s = sub_rn(beta_t_s, a.beta[t_s < T - 1 ? t_s + 1 : t_s]);
    prefetch(group, 0);
  }
  do {
  const long long chain0 = group * cpw;
  const int cw_raw = tid / T;
  const int t_raw = tid - cw_raw * T;
  const bool live = (cw_raw < cpw) && (chain0 + cw_raw < a.n_chains);
  // idle threads shadow replica (chain0, 0): they compute but never store and are never an exchange source
  const int cw = live ? cw_raw : 0;
  const int t = live ? t_raw : 0;
  const long long chain = chain0 + cw;
  const long long rep = chain0 * T + (live ? tid : 0);  // cw * T + t == tid for a live thread

  // ---- LDS (dynamic, sized by the launch: StepLds).  s_stage: the group's rows (streaming form: the current group's slab)
  float *const s_stage = STREAM ? s_dyn + wave * kWaveFloats + cur * L::kSlabFloats
                                : s_dyn + (wide ? 0 : (int)(threadIdx.x >> 6) * kWaveFloats);
  // group-wide ordering of LDS accesses: the group is one wave (narrow) or the workgroup (wide)
  auto sync_group = [&]() {
    if (wide) {
      __syncthreads();
    } else {
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
  };

  // ---- state load: coalesced HBM reads staged through LDS ------------------------------------------------
  // The group's live replicas are one contiguous run of n_live * dim floats in `state`.  The group copies that
  // run with fully coalesced dword loads (thread i takes elements i, i+n, ...) into its slab and each thread then
  // reads its own row (stride dim words: at most a 2-way bank conflict for even dim).  A direct per-thread row
  // read would touch 64 different cache lines per instruction.
  float x[DP], y[DP];
  {
    const long long live_chains = (a.n_chains - chain0 < cpw) ? (a.n_chains - chain0) : cpw;
    const int stage_total = (int)live_chains * T * D0;  // floats of this group's run
    float *__restrict__ gs = a.state + chain0 * T * (long long)D0;
    const int nthr = step_group_threads<STREAM>(T);  // threads of the group = of the workgroup
    int row_head = 0;
    if constexpr (!STREAM) {
      stage_copy<true>(s_stage, gs, stage_total, tid, nthr);
      row_head = stage_head(gs);
      if (wide) reinterpret_cast<int *>(s_dyn)[L::vote(nthr)] = 0;  // no objection yet
      if constexpr (FULL) {
        if (a.full.mom_sum != nullptr) {
          MomentsAcc m(&a.full, cpw, D0);
          m.reg = L::moments_region(s_dyn, wide, nthr, wave, m.doubles());
          m.begin(&a.full, (int)live_chains, chain0, tid, nthr);
        }
        if (a.full.flow_walker != nullptr) {  // the word of this position in the buffer of even events, no visits yet
          int *const fl = L::flow_region(s_dyn, wide, wave, a.full_flow_lds) + tid;
          fl[0] = live ? a.full.flow_walker[rep] : 0;
          fl[L::kFlowUp * nthr] = 0;
          fl[L::kFlowDown * nthr] = 0;
        }
      }
    }
    // (streaming form: the run is landing in slab `cur` by LDS-DMA.  The compiler does not order LDS reads behind it:
    // this wait does - every DMA of this wave, and nothing younger than a whole step, see flush_pending)
    if constexpr (STREAM) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    sync_group();
    const float *row = s_stage + row_head + (live ? tid : 0) * D0;  // idle threads shadow row 0 = replica (chain0, 0)
#pragma unroll
    for (int d = 0; d < DP; ++d) x[d] = (d < D0) ? row[d] : 0.0f;
  }
  float lp;
  [[maybe_unused]] double sq_old = 0.0;
  [[maybe_unused]] long long acc_old = 0;
  if constexpr (STREAM) {
    {
      const float *zone = s_dyn + wave * kWaveFloats + L::zone(cur);
      lp = (zone + L::kZoneLogp)[tid];
      if (a.sq_jump != nullptr) sq_old = reinterpret_cast<const double *>(zone + L::kZoneSqJump)[tid < cpw * T ? tid : 0];
      if (a.n_accept != nullptr) acc_old = reinterpret_cast<const long long *>(zone + L::kZoneAccept)[tid < cpw * T ? tid : 0];
    }
    // the previous group's results leave now, and behind them the next group's DMA is issued: the other slab is free,
    // the previous group's outgoing rows were read back into pend_o before this group began
    if (have_pending) flush_pending();
    if (group + group_stride < n_groups) prefetch(group + group_stride, cur ^ 1);
  } else {
    lp = a.logp[rep];
  }
  const float beta_t = STREAM ? beta_t_s : a.beta[t];
  const float tscale = STREAM ? tscale_s : a.temp_scale[t];
  // may the proposal's own squared increment stand for |y - x|^2 for this replica?  (proposals.h kJumpTrust)
  bool jump_trusted = false;
  if constexpr (Proposal::kKnowsJump) {
    float xmax = 0.0f;
#pragma unroll
    for (int d = 0; d < DP; ++d) xmax = __builtin_fmaxf(xmax, __builtin_fabsf(x[d]));  // (slots >= dim hold 0)
    jump_trusted = xmax <= kJumpTrust * Proposal::increment_scale(tscale, a.pp);  // (NaN: false)
  }

  const unsigned long long gchain = (unsigned long long)(a.chain_offset + chain);
  constexpr bool kHeads = philox_heads_in_lds(DP, EXACT, FULL, STREAM, Proposal::kKind);
  static_assert(!kHeads || L::kHeadsFit, "the parked heads need room over the rows and the swap scratch");
  constexpr bool kKeepHeads = event_keeps_heads(DP, EXACT, FULL, STREAM, Proposal::kKind);
  static_assert(!kKeepHeads || L::kKeptFit, "an event that keeps the heads needs its words beside them");
  // the thread's lane, one VGPR for the whole launch (lane_index_carried; opaque, so that it is neither rebuilt from
  // threadIdx.x, which would then live across the loop beside it, nor folded into three addresses kept instead of one index)
  constexpr bool kLane = lane_index_carried(DP, EXACT, FULL, STREAM, Proposal::kKind);
  [[maybe_unused]] int lane_c = 0;
  if constexpr (kLane) {
    lane_c = (int)(threadIdx.x & 63);
    PTRWM_VALUE_BARRIER("+v"(lane_c));
  }
  typename std::conditional<kHeads, RngCtxHeads, RngCtx>::type rc;  // (counter words: rng_layout.h)
  rc.c2 = chain_word_c2(gchain);
  rc.k0 = a.k0;
  rc.k1 = a.k1;
  const uint32_t c3_base = chain_word_c3(gchain, (uint32_t)t);
  // This thread's slot of block 0 of the parked heads, from the carried lane index, and the store of all its heads for the
  // counter word c0hi: in the prologue, and behind the row exchange of every swap event that goes through the slab
  // (event_keeps_heads says which do not), each time behind the group's barrier (StepLds::heads).  c0hi holds for the
  // launch: schedule.h cuts at 2^32 steps.
  [[maybe_unused]] auto head_slot0 = [&]() __attribute__((always_inline)) {
    return reinterpret_cast<PhiloxHeadSlot *>(s_dyn + L::heads(wide, wave)) + (kLane ? lane_c : (thread_index_now(wave) & 63));
  };
  [[maybe_unused]] auto store_heads = [&](uint32_t c0hi, uint32_t c3) __attribute__((always_inline)) {
    PhiloxHeadSlot *const slot0 = head_slot0();
    uint32_t chain_hi, chain_lo;
    philox_mul(kPhiloxM1, rc.c2, chain_hi, chain_lo);
#pragma unroll
    for (int c = 0; c < normal_blocks(DP); ++c) {
      const PhiloxHead h = philox_head(c0hi | (uint32_t)c, chain_lo, c3, rc.k0, rc.k1);
      slot0[c * kHeadBlockSlots] = PhiloxHeadSlot{h.pk, h.qk, h.ql, 0u};
    }
  };
  if constexpr (kHeads) {
    sync_group();  // every row of the group has been read
    store_heads(step_word_c0hi((unsigned long long)a.step0), with_stream(c3_base, kStreamMH));
  }

  unsigned n_acc = 0;
  {
    // parked in LDS (StepLds): the Philox word with the temperature index, the number of accepted
    // swaps of pair (t, t+1) and the index within this launch of the last swap event in which it accepted
    const int gt = step_group_threads<STREAM>(T);
    int *const park = reinterpret_cast<int *>(STREAM ? s_dyn + wave * kWaveFloats + L::parked(gt) : s_stage + L::parked(gt)) + tid;
    park[0] = (int)c3_base;
    park[L::kSwapCount * gt] = 0;
    park[L::kLastEvent * gt] = -1;
    // ... and this launch's sum of squared jumps behind them: a no-return ds_add_f64 per counted step - the same IEEE
    // additions in the same order as a register would see, without two VGPRs across the step loop (at the 128-VGPR cap)
    reinterpret_cast<double *>(park - tid + L::kSqJump * gt)[tid] = 0.0;
  }

  const bool ext = FULL && a.full.ext_prop != nullptr;
  const bool trace_on =
      FULL && live && a.full.trace != nullptr && (chain < a.full.trace_chains) && (t < (int)a.full.trace_temps);
  int to_swap = a.steps_to_swap;
  int to_trace = FULL ? (int)a.full.steps_to_trace : 0;
  [[maybe_unused]] int to_mom = FULL ? (int)a.full.steps_to_mom : 0;
  int trace_rows = 0;    // rows of the trace written by this launch
  int swap_in_call = 0;  // swap events already done in this launch
  const int ev_par0 = (int)(a.first_swap_event & 1);
  unsigned long long s = (unsigned long long)a.step0;  // 0-based global step index

  constexpr int W = canon_width(DP);
  // The move of a step without a swap event, x[d] = acc ? y[d] : x[d], and its squared jump.  It is committed IN PLACE, one
  // select per dimension: the loop below is shaped so that no path on which the old state is still needed meets this one
  // before the next step begins (see there).
  auto commit_plain = [&](bool acc, float jump, int jump_kind, int D) __attribute__((always_inline)) -> float {
    float j2;
    if (jump_kind != kJumpNone) {
      // the proposal knows the length of its own increment: the move itself is one select per dimension.  Replicas whose
      // state is too large for that to equal |y - x|^2 (jump_trusted, decided at the start of the launch: none, normally -
      // the branch is skipped) take it from the states
      float from_states = 0.0f;
      if (!jump_trusted) {
        PTRWM_COLD_PATH();
        float j2p[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        PTRWM_DIM_LOOP(d, DP, D, {
          const float dl = sub_rn(y[d], x[d]);
          j2p[d / W] = fmaf(dl, dl, j2p[d / W]);
        })
        from_states = tree4_add(j2p);
      }
      PTRWM_DIM_LOOP(d, DP, D, {
        x[d] = acc ? y[d] : x[d];
        if ((d & PTRWM_J2_FENCE_MASK) == PTRWM_J2_FENCE_MASK) sched_fence_soft();
      })
      j2 = acc ? (jump_trusted ? jump : from_states) : 0.0f;
    } else {
      float j2p[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // squared jump in the canonical four-range order (philox.h)
      PTRWM_DIM_LOOP(d, DP, D, {
        const float dl = sub_rn(y[d], x[d]);
        j2p[d / W] = fmaf(dl, dl, j2p[d / W]);
        x[d] = acc ? y[d] : x[d];
        if ((d & PTRWM_J2_FENCE_MASK) == PTRWM_J2_FENCE_MASK) sched_fence_soft();
      })
      j2 = tree4_add(j2p);
      if (!acc) j2 = 0.0f;
    }
    return j2;
  };
  // what every step ends with: the launch's statistics, and the trace / moments of the fixture twin
  auto finish_step = [&](bool count_on, bool acc, float j2, int D) __attribute__((always_inline)) {
    if (count_on) {
      n_acc += acc ? 1u : 0u;
      // (the slot's address is rebuilt here, not carried across the step - from the carried lane index where there is one)
      const int tid_q = kLane ? wave * 64 + lane_c : thread_index_now(wave);
      const int gt_q = wide ? group_threads(T, 1) : 64;  // (not step_group_threads: that moved the production kernels' registers here)
      double *const sq_slot = reinterpret_cast<double *>(
                                  STREAM ? s_dyn + wave * kWaveFloats + L::sq_jump(64)
                                         : s_dyn + (wide ? 0 : wave * kWaveFloats) + L::sq_jump(gt_q)) +
                              (wide ? tid_q : (kLane ? lane_c : (tid_q & 63)));
      // (the counted jump's zero is selected on the float: left to the compiler, the select sinks below the conversion and
      // becomes two v_cndmask on the halves of the double.  In the kernels above only: the others keep their machine code)
      float j2c = j2;
      if constexpr (kLane) PTRWM_VALUE_BARRIER("+v"(j2c));
      (void)__hip_atomic_fetch_add(sq_slot, (double)j2c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    }
    if constexpr (FULL) {
      const bool trace_now = a.full.trace != nullptr && countdown_due(to_trace, a.full.trace_every);
      if (trace_now && trace_on) {
        const long long row = trace_row_index(&a.full, trace_rows, chain, t);
        float *__restrict__ tr = a.full.trace + row * D;
        PTRWM_DIM_LOOP(d, DP, D, { tr[d] = x[d]; })
        if (a.full.trace_logp != nullptr) a.full.trace_logp[row] = lp;
      }
      trace_rows += trace_now ? 1 : 0;
      // the state after the whole step
      if (a.full.mom_sum != nullptr && countdown_due(to_mom, a.full.mom_every) && count_on && live && t < (int)a.full.mom_temps) {
        MomentsAcc m(&a.full, cpw, D);
        m.reg = L::moments_region(s_dyn, wide, step_group_threads<STREAM>(T), wave, m.doubles());
        const MomentsAcc::Row r = m.row(cw, t);
        PTRWM_DIM_LOOP(d, DP, D, {
          const double v = (double)x[d];
          moments_add(r.sum + d, v);
          moments_add(r.sum_sq + d, v * v);
        })
        moments_add(r.logp, (double)lp);
      }
    }
  };

  // The step loop is two loops.  The INNER one holds nothing but Metropolis steps: it runs up to the next step whose counter
  // is a multiple of swap_every (or the end of the launch) and leaves, with that step's proposal decided but not committed,
  // to the OUTER one, which commits it - with a swap event if one is due - and starts the next run.  As one loop, an
  // ordinary step's commit met the swap path again before the latch (the compiler linearises the divergent parts of a
  // loop body into `if (!swap) commit; if (swap) exchange;`): the new state and the old one the exchange still needs were
  // both live there, so every select wrote a temporary and DP + 1 v_mov_b32 copied them back at the end of EVERY step -
  // 62 of the 977 VALU instructions of a dim-30 step (profiles/r06_commit_in_place.txt).  Step for step the same work in the
  // same order: count_on / burn_left, to_swap, the countdowns of the fixture twin and swap_in_call keep their meaning.
  int i = 0;
  while (i < a.n_steps) {
    const int left = a.n_steps - i;
    const bool to_multiple = to_swap <= left;      // this run ends on a multiple of swap_every (else: with the launch)
    int run = to_multiple ? to_swap : left;        // its steps, the last one included (>= 1)
    to_swap = to_multiple ? a.swap_every : to_swap - left;
    bool count_on, acc;
    float lp_mh;
    float jump;     // the squared length of the increment, if the proposal knows it (proposals.h)
    int jump_kind;  // (a constant in production kernels)
    int D;
    for (;; ++i, ++s) {
      count_on = i >= a.burn_left;
      rc.c0hi = step_word_c0hi(s);
      rc.c1 = step_word_c1(s);
      rc.c3 = with_stream(c3_base, kStreamMH);
      // (at the register cap the chain word is made opaque per step: its product with the Philox multiplier is otherwise
      // hoisted out of the step loop as a 64-bit pair, which THERE is spilled and fetched back from scratch at the top of
      // every step - one v_mad_u64_u32 per step instead.  Only there: every kernel with registers to spare keeps the hoisted
      // product and runs 2-5 % faster for it - dims 24 / 48 / 50 in profiles/r04_scratch_ab.txt, table 6)
      // (with the heads parked that product is in the loop no more: only its high half is, one register)
      if constexpr (step_loop_at_register_cap(DP, STREAM) && !kHeads) asm volatile("" : "+v"(rc.c2));
      if constexpr (kHeads) rc.heads = head_slot0();  // (from the carried lane index: what is carried is that one register)

      long long srep = 0;
      const float *ext_raw = nullptr;
      float ext_u = 0.0f;
      if constexpr (FULL) {
        srep = step_replica_index(i, a.n_chains, chain, T, t);
        if (ext) {
          ext_raw = ext_prop_row(&a.full, ext_raw_per_step(Proposal::kKind, D0), srep, 1);
          ext_u = a.full.ext_u[srep];
        }
      }

      jump = 0.0f;
      const float u_acc = Proposal::propose(y, x, fresh_dim<EXACT>(D0), tscale, a.pp, rc, ext_raw, ext_u, jump, jump_kind);
      const float lp_new = Target::template logp<false>(y, fresh_dim<EXACT>(D0), a.tp);
      D = fresh_dim<EXACT>(D0);

      // ultra_fused_mcmc_step_basic / ultra_fused_parallel_mcmc_step:
      //   r = beta (l' - l);  accept = (r > 0) | (u < exp r)
      acc = mh_accept(beta_t, lp_new, lp, u_acc);
      lp_mh = acc ? lp_new : lp;
      if constexpr (FULL) {
        if (a.full.accept_flags != nullptr && live) a.full.accept_flags[srep] = acc ? 1 : 0;
      }

      if (--run == 0) break;  // the last step of the run is committed below
      const float j2 = commit_plain(acc, jump, jump_kind, D);
      lp = lp_mh;
      finish_step(count_on, acc, j2, D);
    }
    const bool swap_due = to_multiple && count_on && (T > 1);

    float j2;
    if (!swap_due) {
      j2 = commit_plain(acc, jump, jump_kind, D);
      lp = lp_mh;
    } else {
      // ---- temperature swaps on the post-MH log-densities (pt_rwm_gpu_optimized.py:594-633) ----
      // The exchange indices are rebuilt here from an opaque copy of threadIdx.x, so that none of them occupies a
      // register (or a scratch slot) across the MH part of the step (lane_index_carried: from the one index that does).
      // (the index through a value barrier: what the event derives from it - slots, the parked words' address - is computed
      // here, in one step of ten, and not hoisted out of the step loop into registers of its own)
      int lane_s = lane_c;
      if constexpr (kLane) PTRWM_VALUE_BARRIER("+v"(lane_s));
      const int tid_s = kLane ? wave * 64 + lane_s : thread_index_now(wave);
      const int slot = wide ? tid_s : (kLane ? lane_s : (tid_s & 63));  // this thread's slot in s_l / s_u and its row in s_stage
      const int group_threads = step_group_threads<STREAM>(T);
      float *const rows = STREAM ? s_dyn + wave * kWaveFloats + cur * L::kSlabFloats
                                 : s_dyn + (wide ? 0 : (kLane ? wave : (tid_s >> 6)) * kWaveFloats);
      float *const s_l = STREAM ? s_dyn + wave * kWaveFloats + L::s_l(64) : rows + L::s_l(group_threads);
      float *const s_u = s_l + L::kSu * group_threads;
      int *const park = reinterpret_cast<int *>(s_l + L::kParked * group_threads) + slot;
      const uint32_t c3_s = (uint32_t)park[0];
      const int t = temperature_of(c3_s);  // the temperature index, as the Philox counter holds it
      const int base = live ? slot - t : 0;            // slot of temperature 0 of this thread's ladder
      // src = slot whose post-MH vector ends up at this thread's temperature
      int src = slot;
      float my_l = lp_mh;
      bool pair_acc = false;  // did pair (t, t+1) accept (recorded on the thread of temperature t)
      float us;
      if (ext) us = swap_uniform_ext(a.full.ext_swap_u, swap_in_call, a.n_chains, chain, T, t);
      else us = swap_uniform_philox(rc.c0hi, rc.c1, rc.c2, with_stream(c3_s, kStreamSwap), rc.k0, rc.k1);
      // An event that the walk decides (below) leaves the parked heads alone (event_keeps_heads): it publishes beside them and
      // moves the rows through the lanes.  Every other event of a kernel with parked heads writes over them, and stores them
      // again at its end.  (Spelt out for these kernels only: every other kernel keeps its event, and its machine code.)
      [[maybe_unused]] bool keep_heads = false;
      [[maybe_unused]] float *kept_l = nullptr, *kept_u = nullptr;
      if constexpr (kKeepHeads) {
        keep_heads = !wide && a.swap_order == PTRWM_ORDER_SEQUENTIAL && a.swap_mode == PTRWM_SWAP_EXCHANGE;
        kept_l = rows + L::kKeptL, kept_u = rows + L::kKeptU;  // (narrow: rows = the wave's base)
      }
      if constexpr (kKeepHeads) {
        // (parked heads lie under the scratch words and the rows: every thread of the group has read this step's)
        if (!keep_heads) sync_group();
        if (keep_heads) {
          kept_l[slot] = my_l;
          kept_u[slot * L::kKeptUStride] = us;
        } else {
          s_l[slot] = my_l;
          s_u[slot] = us;
        }
      } else {
      // (parked heads lie under the scratch words and the rows: every thread of the group has read this step's)
      if constexpr (kHeads) sync_group();
      // publish this thread's log-density and swap uniform; the sweep reads them back with broadcast ds_reads
      s_l[slot] = my_l;
      s_u[slot] = us;
      }
      // may this ladder's sequential sweep take the threshold form in THIS event?  (swap_decide: a verdict of the ladder)
      const float db_pair = STREAM ? db_s : sub_rn(beta_t, a.beta[t < T - 1 ? t + 1 : t]);  // b_t - b_{t+1}; the last position: 0
      const bool pair_plain = swap_pair_plain(T, t, db_pair, my_l, us);
      // (narrow groups: a ballot over the ladder's lanes.  Wide: the ladder's word behind the parked words,
      // wide_ladder_votes_plain)
      bool swap_plain;
      if (wide) {
        swap_plain = wide_ladder_votes_plain(reinterpret_cast<int *>(s_l + L::kVote * group_threads), pair_plain, swap_in_call + 1, sync_group);
      } else {
        swap_plain = ladder_votes_plain(pair_plain, base, T);
        sync_group();
      }
      // (one-wavefront groups decide the sequential exchange sweep by lane masks and a scalar walk; wide ladders keep the scan)
      if (swap_walk_in_kernel(DP) && !wide && a.swap_order == PTRWM_ORDER_SEQUENTIAL && a.swap_mode == PTRWM_SWAP_EXCHANGE) {
        if constexpr (kKeepHeads)
          swap_walk_decide<FULL, L::kKeptUStride>(T, t, base, slot, a.beta, db_pair, us, kept_l, kept_u, my_l, src, pair_acc, sync_group, swap_plain);
        else
          swap_walk_decide<FULL>(T, t, base, slot, a.beta, db_pair, us, s_l, s_u, my_l, src, pair_acc, sync_group, swap_plain);
      } else
        swap_decide<!(STREAM && swap_walk_in_kernel(DP))>(T, t, base, slot, a.swap_mode, a.swap_order, (ev_par0 + swap_in_call) & 1, a.beta, beta_t, us, s_l, s_u,
                    reinterpret_cast<int *>(s_u + (L::kLanded - L::kSu) * group_threads), my_l, src, pair_acc, sync_group, swap_plain);
      if (pair_acc) {
        park[L::kSwapCount * group_threads] += 1;
        park[L::kLastEvent * group_threads] = swap_in_call;
      }
      // commit MH move and swap in one pass: every thread publishes its post-MH vector as its slab row, then
      // fetches the row of slot `src` (rows exchanged through LDS: 2 LDS ops per dimension, no HBM)
      {
        float j2p[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // (a swap step's jump is taken from the rows, in the canonical order)
        if (keep_heads) {
          // ... or, with the heads kept, straight from the lane that holds it: slot = lane in a one-wavefront group, every lane
          // of the wavefront is here (idle ones shadow a live position), and src is a lane of a live ladder - or the thread's own
          const int src_lane = src << 2;
          // (y[d] through a value barrier: these selects are then not the slab path's, and stay here, eight at a time between
          // the fences - seen as the same expression they were hoisted above the branch, all DP of them live beside x[] and
          // the fetched row, and the kernel went from 113 to 127 VGPRs)
          PTRWM_DIM_LOOP(d, DP, D, {
            float yd = y[d];
            PTRWM_VALUE_BARRIER("+v"(yd));
            const float v = acc ? yd : x[d];
            const float w = __int_as_float(__builtin_amdgcn_ds_bpermute(src_lane, __float_as_int(v)));
            const float dl = sub_rn(w, x[d]);
            j2p[d / W] = fmaf(dl, dl, j2p[d / W]);
            x[d] = w;
            if ((d & 7) == 7) sched_fence_soft();
          })
          j2 = tree4_add(j2p);
        } else {
          float *my_row = rows + slot * D;
          PTRWM_DIM_LOOP(d, DP, D, { my_row[d] = acc ? y[d] : x[d]; })
          sync_group();
          const int Dr = fresh_dim<EXACT>(D0);  // generic widths: fresh d < dim compares instead of 2*DP live masks
          const float *src_row = rows + src * Dr;
          PTRWM_DIM_LOOP(d, DP, Dr, {
            const float w = src_row[d];
            const float dl = sub_rn(w, x[d]);
            j2p[d / W] = fmaf(dl, dl, j2p[d / W]);
            x[d] = w;
            if ((d & 7) == 7) sched_fence_soft();
          })
          j2 = tree4_add(j2p);
          if constexpr (kHeads) {
            sync_group();  // every row of the group has been fetched: the heads go back over them
            store_heads(rc.c0hi, with_stream(c3_s, kStreamMH));
          }
        }
        if constexpr (FULL) {
          // replica flow (flow.h): the word travels as the row does - fetched from slot `src` behind the barrier above, which
          // also orders it behind that slot's write of the previous event, and written to the OTHER buffer: slot `slot` of this
          // event's buffer may still be read by the thread it lands at.  The next write to this event's buffer is two events
          // away, behind the barriers of the next one.
          if (a.full.flow_walker != nullptr && live) {
            int *const fl = L::flow_region(s_dyn, wide, wave, a.full_flow_lds);
            const int buf = swap_in_call & 1;
            bool trip;
            const int32_t fw = flow_ends(fl[buf * group_threads + src], t, T, trip);
            fl[(buf ^ 1) * group_threads + slot] = fw;
            if (trip && flow_id(fw) < T && a.full.flow_round_trips != nullptr) {  // (t = 0: the ladder's one writer; an id the caller never set counts nowhere)
              // (the row's address from an opaque copy of the chain index: it is loop-invariant, and hoisted out of the step
              // loop it was a register pair kept - at the 128-VGPR cap: in scratch - for the whole launch)
              long long ch = chain;
              PTRWM_VALUE_BARRIER("+v"(ch));
              a.full.flow_round_trips[ch * T + flow_id(fw)] += 1;
            }
            fl[L::kFlowUp * group_threads + slot] += (int)flow_visit_up(fw);
            fl[L::kFlowDown * group_threads + slot] += (int)flow_visit_down(fw);
          }
        }
      }
      lp = my_l;
      ++swap_in_call;
    }
    finish_step(count_on, acc, j2, D);
    ++i;
    ++s;
  }

  // ---- state store: rows -> LDS slab -> coalesced HBM writes -----------------------------------------------
  const kargs_ptr ae = late_args();  // the epilogue's arguments are loaded here, not kept in SGPRs across the step loop
  long long c0_out;
  {
    // everything is recomputed from opaque copies so that nothing of the prologue stays live across the step loop
    const int T2 = fresh_dim<false>(T), D2 = EXACT ? DP : fresh_dim<false>(D0), cpw2 = fresh_dim<false>(cpw);
    const bool wide2 = T2 > 64;
    const int tx2 = thread_index_now(wave);
    const int tid2 = wide2 ? tx2 : (tx2 & 63);
    float *const rows2 = STREAM ? s_dyn + wave * kWaveFloats + cur * L::kSlabFloats : s_dyn + (wide2 ? 0 : wave * kWaveFloats);
    long long c0;
    if constexpr (STREAM) {
      c0 = group * cpw2;
    } else {
      const long long bid = (long long)fresh_dim<false>((int)blockIdx.x);  // re-read here, not carried in a VGPR
      c0 = (wide2 ? bid : bid * kWavesPerBlock + wave) * cpw2;
    }
    const long long n_chains2 = ae->n_chains;
    const long long live_chains = (n_chains2 - c0 < cpw2) ? (n_chains2 - c0) : cpw2;
    const int stage_total = (int)live_chains * T2 * D2;
    const long long stage_g0 = c0 * T2 * (long long)D2;
    c0_out = c0;
    float *__restrict__ gs = ae->state + stage_g0;
    sync_group();  // the last swap's row reads are done before the rows are overwritten
    if (live) {
      float *row = rows2 + stage_head(gs) + tid2 * D2;
#pragma unroll
      for (int d = 0; d < DP; ++d)
        if (d < D2) row[d] = x[d];
    }
    sync_group();
    const int nthr = group_threads(T2, 1);
    if constexpr (FULL) {
      // every add of the launch is behind the barrier above: the group's partial sums go to HBM, once
      const kargs_full_ptr fa = &ae->full;
      if (fa->mom_sum != nullptr) {
        MomentsAcc m(fa, cpw2, D2);
        m.reg = L::moments_region(s_dyn, wide2, nthr, wave, m.doubles());
        m.end(fa, (long long)ae->full_mom_steps, live_chains, c0, tid2, nthr);
      }
    }
    if constexpr (STREAM) {
      // whole aligned vectors only (capi.hip): slab -> registers now, registers -> HBM in flush_pending
      const pf_vec4 *__restrict__ lv = reinterpret_cast<const pf_vec4 *>(rows2);
      const int n_vec = stage_total >> 2;
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        const int v = tid2 + 64 * k;
        if (v < n_vec) pend_o[k] = lv[v];
      }
    } else {
      stage_copy<false>(rows2, gs, stage_total, tid2, nthr);
    }
  }
  if (live) {
    const int tid_o = thread_index_now(wave);
    const int T_o = fresh_dim<false>(T);
    const long long rep = c0_out * T_o + (T_o > 64 ? tid_o : (tid_o & 63));  // live: replica index in group == tid
    const int gt_o = group_threads(T_o, 1);
    const int *const park = reinterpret_cast<const int *>(STREAM ? s_dyn + wave * kWaveFloats + L::parked(64)
                                                                 : s_dyn + (T_o > 64 ? 0 : (tid_o >> 6) * kWaveFloats) + L::parked(gt_o)) +
                            (T_o > 64 ? tid_o : (tid_o & 63));
    const int t = temperature_of((uint32_t)park[0]);
    const unsigned n_swap_acc = (unsigned)park[L::kSwapCount * gt_o];
    const int last_event = park[L::kLastEvent * gt_o];
    const int tid_g = T_o > 64 ? tid_o : (tid_o & 63);
    const double sq = reinterpret_cast<const double *>(park - tid_g + L::kSqJump * gt_o)[tid_g];
    if constexpr (STREAM) {
      // handed to flush_pending (the old squared-jump sum came in with the prefetch: the same double addition as the classic
      // kernel's read-modify-write, without a load)
      pend_lp = lp;
      pend_acc_on = ae->n_accept != nullptr && n_acc != 0u;
      pend_acc = acc_old + (long long)n_acc;
      pend_n_swap = n_swap_acc;
      pend_sq_on = ae->sq_jump != nullptr && sq != 0.0;
      pend_sq = sq_old + sq;
      pend_ord_on = ae->last_swap_ordinal != nullptr && last_event >= 0;
      const long long ev = ae->first_swap_event + last_event;
      pend_ord = swap_attempt_ordinal(ae->swap_order, ev, T_o, t);
    } else {
    // (the classic results store is written out here and in quad.h: as one function it moved the register allocation of
    // both forms' production kernels, profiles/r11_swap_event_once.txt)
    ae->logp[rep] = lp;
    // statistics: read-modify-write only where this launch has something to add (a launch without a swap event - nine in
    // ten at one step per launch - then leaves the swap counters' cache lines alone)
    if (ae->n_accept != nullptr && n_acc != 0u) count_add(&ae->n_accept[rep], (long long)n_acc);
    if (ae->sq_jump != nullptr && sq != 0.0) ae->sq_jump[rep] += sq;
    if (ae->swap_accept != nullptr && n_swap_acc != 0u) count_add(&ae->swap_accept[rep], (long long)n_swap_acc);
    if (ae->last_swap_ordinal != nullptr && last_event >= 0) {
      const long long ev = ae->first_swap_event + last_event;
      const long long ord = swap_attempt_ordinal(ae->swap_order, ev, T_o, t);
      if (ord > ae->last_swap_ordinal[rep]) ae->last_swap_ordinal[rep] = ord;
    }
    if constexpr (FULL) {
      // replica flow: the word this position holds now (the buffer the next event would read) and the launch's visits
      const kargs_full_ptr fa = &ae->full;
      if (fa->flow_walker != nullptr) {
        const int *const fl = L::flow_region(s_dyn, T_o > 64, wave, ae->full_flow_lds) + tid_g;
        fa->flow_walker[rep] = fl[(swap_in_call & 1) * gt_o];
        const int n_up = fl[L::kFlowUp * gt_o], n_down = fl[L::kFlowDown * gt_o];
        if (fa->flow_up != nullptr && n_up != 0) count_add(&fa->flow_up[rep], (long long)n_up);
        if (fa->flow_down != nullptr && n_down != 0) count_add(&fa->flow_down[rep], (long long)n_down);
      }
    }
    }
  }
  if constexpr (!STREAM) break;
  pend_group = group;
  have_pending = true;
  group += group_stride;
  cur ^= 1;
  } while (group < n_groups);
  if constexpr (STREAM) flush_pending();
}

// ---- standalone log-density kernel (unit parity of the targets; initial log-density) ----
template <class Target, int DP>
__global__ void __launch_bounds__(kBlockThreads) ptrwm_logdensity_kernel(const float *__restrict__ x,
                                                                          float *__restrict__ out,
                                                                          long long n, int D, TParams tp) {
  const long long i = (long long)blockIdx.x * kBlockThreads + threadIdx.x;
  if (i >= n) return;
  float y[DP];
  const float *__restrict__ xp = x + i * D;
#pragma unroll
  for (int d = 0; d < DP; ++d) y[d] = (d < D) ? xp[d] : 0.0f;
  out[i] = Target::template logp<true>(y, D, tp);
}

// The two stand-alone proposal kernels below hold x[DP] and y[DP] in registers: above width 64 they are compiled for two
// waves per SIMD, i.e. a budget of 256 registers, so that what does not fit goes to scratch (speed is irrelevant here)
// and not into AGPRs - the build gate (tools/kernel_stats.py --check) admits no kernel with AGPRs or > 256 VGPRs.
constexpr int standalone_min_waves(int dp) { return dp > 64 ? 2 : 1; }

// ---- standalone proposal kernel (unit parity of the three samplers) ----
template <class Proposal, int DP>
__global__ void __launch_bounds__(kBlockThreads, standalone_min_waves(DP)) ptrwm_propose_kernel(
    float *__restrict__ out, long long n, int D, int T, const float *__restrict__ temp_scale, PParams pp,
    const float *__restrict__ ext_raw, int n_raw_ext, unsigned k0, unsigned k1) {
  const long long i = (long long)blockIdx.x * kBlockThreads + threadIdx.x;
  if (i >= n * T) return;
  const long long row = i / T;
  const int t = (int)(i - row * T);
  float x[DP], y[DP];
#pragma unroll
  for (int d = 0; d < DP; ++d) x[d] = 0.0f;
  RngCtx rc;
  rc.c0hi = step_word_c0hi((unsigned long long)row);
  rc.c1 = step_word_c1((unsigned long long)row);  // "step" = row, chain 0
  rc.c2 = chain_word_c2(0ull);
  rc.c3 = with_stream(chain_word_c3(0ull, (uint32_t)t), kStreamMH);
  rc.k0 = k0;
  rc.k1 = k1;
  const float *er = ext_raw != nullptr ? ext_raw + i * n_raw_ext : nullptr;
  float jump = 0.0f;
  int jump_kind;
  Proposal::propose(y, x, D, temp_scale[t], pp, rc, er, 0.0f, jump, jump_kind);
  float *__restrict__ op = out + i * D;
#pragma unroll
  for (int d = 0; d < DP; ++d)
    if (d < D) op[d] = y[d];
}

// ---- split step, first half: proposals for one step written to HBM (targets evaluated by the caller) ----
// Same Philox words and the same arithmetic as the fused kernel's Proposal::propose call, so a split step driven
// with the library's own log-density reproduces ptrwm_run bit for bit.
// One wavefront per 64 replicas (64-thread workgroups): the tile's run of 64 x dim floats goes through a slab of LDS in both
// directions (stage_copy: coalesced 16-byte transfers whatever the run's alignment), each lane working on its own row -
// round 3's version read and wrote its row straight from HBM, 64 cache lines per instruction: 0.36 ms per step at
// 65 536 x 32 x dim 30, where moving the bytes takes 0.1.
constexpr unsigned split_tile_lds_bytes(int dim) { return (unsigned)(64 * dim + 4) * 4u; }

template <class Proposal, int DP>
__global__ void __launch_bounds__(64, standalone_min_waves(DP)) ptrwm_split_propose_kernel(
    const float *__restrict__ state, float *__restrict__ proposals, float *__restrict__ accept_u, long long n_chains,
    long long chain_offset, unsigned long long step, int D, int T, const float *__restrict__ temp_scale, PParams pp,
    const float *__restrict__ ext_raw, const float *__restrict__ ext_u, int n_raw_ext, unsigned k0, unsigned k1,
    const long long *__restrict__ device_step) {
  extern __shared__ __attribute__((aligned(16))) float s_tile[];
  const int lane = (int)threadIdx.x;
  const long long n_reps = n_chains * T;
  const long long first = (long long)blockIdx.x * 64;
  if (first >= n_reps) return;
  if (device_step != nullptr) step += (unsigned long long)*device_step;  // (include/ptrwm.h: the counter plus this call's offset)
  const int n_rows = (n_reps - first < 64) ? (int)(n_reps - first) : 64;
  const bool live = lane < n_rows;
  const long long i = first + (live ? lane : 0);
  const long long chain = i / T;
  const int t = (int)(i - chain * T);
  float x[DP], y[DP];
  float *__restrict__ gx = const_cast<float *>(state) + first * D;
  stage_copy<true>(s_tile, gx, n_rows * D, lane, 64);
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  {
    const float *row = s_tile + stage_head(gx) + (live ? lane : 0) * D;
#pragma unroll
    for (int d = 0; d < DP; ++d) x[d] = (d < D) ? row[d] : 0.0f;
  }
  const unsigned long long gchain = (unsigned long long)(chain_offset + chain);
  RngCtx rc;
  rc.c0hi = step_word_c0hi(step);
  rc.c1 = step_word_c1(step);
  rc.c2 = chain_word_c2(gchain);
  rc.c3 = with_stream(chain_word_c3(gchain, (uint32_t)t), kStreamMH);
  rc.k0 = k0;
  rc.k1 = k1;
  const float *er = ext_raw != nullptr ? ext_raw + i * n_raw_ext : nullptr;
  float jump = 0.0f;
  int jump_kind;
  const float u = Proposal::propose(y, x, D, temp_scale[t], pp, rc, er, ext_u != nullptr ? ext_u[i] : 0.0f, jump, jump_kind);
  float *__restrict__ gy = proposals + first * D;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();  // every lane has its row in registers: the slab takes the proposals
  if (live) {
    float *row = s_tile + stage_head(gy) + lane * D;
#pragma unroll
    for (int d = 0; d < DP; ++d)
      if (d < D) row[d] = y[d];
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  stage_copy<false>(s_tile, gy, n_rows * D, lane, 64);
  if (!live) return;
  accept_u[i] = u;
  // second plane of the scratch array: the proposal's own squared jump, exactly as the fused kernel counts it, or -1 when
  // it is to be taken from the states (external randoms, Laplace): split_accept_kernel then reproduces ptrwm_run's sums
  float xmax = 0.0f;
#pragma unroll
  for (int d = 0; d < DP; ++d) xmax = __builtin_fmaxf(xmax, __builtin_fabsf(x[d]));
  const bool trusted = Proposal::kKnowsJump && xmax <= kJumpTrust * Proposal::increment_scale(temp_scale[t], pp);  // (proposals.h)
  accept_u[n_reps + i] = (jump_kind == kJumpTotal && trusted) ? jump : -1.0f;
}

}  // namespace ptrwm
