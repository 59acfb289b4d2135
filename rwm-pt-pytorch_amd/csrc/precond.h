// Preconditioned Gaussian proposals, stated once: the proposal rule, the rule by which the factor is learned from one warm-up
// window's covariance sums, and the geometry of the proposal kernel (the index maps below).  Plain C++ (no HIP include): the two
// kernels of capi.hip call it, tests/precond_test.cpp checks it on the CPU and replays the proposal kernel's staging, K-steps
// and epilogue with it, tests/precond_reference.py restates both rules in plain Python.
//
// Proposal.  For replica row (c, t) with state x, factor L (float [dim, dim], row-major, only the entries j <= i are ever read),
// per-temperature scale s_t = temp_scale[t] and standard normals z[0 .. dim):
//   inc_i = the chain  acc = +0;  for k = 0, 1, ..., prec_chain_end(i) - 1 ascending:  acc = fmaf(Lp[i][k], zp[k], acc)
//   y_i   = fmaf(s_t, inc_i, x_i)
// where prec_chain_end(i) = 16 (i / 16 + 1) - the chain of coordinate i runs to the end of i's block of 16 - and Lp, zp are L
// and z with zeros where k > i (Lp) and where k >= dim (zp).  Every product behind k = i is therefore (+0)(zp[k]): for finite
// z it adds a zero, which changes nothing but the sign of a zero sum.
//   Philox path: z is box_muller (philox.h) at unit scale of the step's blocks - the words, counter layout and stream of
//   NormalProposal (proposals.h) - and the accept uniform is word prec_accept_word(dim) = 2 ceil(dim / 2), as there.
//   External randoms: z = ext_prop (dim raw values per row), the accept uniform is ext_u.
// Plane 1 of accept_u is -1: the accept kernel takes the squared jump from the states, as it does for Laplace.
//
// Update.  From the window sums of one temperature (cov.h's layout: sxx lower triangle, sx, count) and a running triple
// (R_xx, R_x, w), all double, every operation rounded on its own (no fma), sqrt and division IEEE:
//   R_xx[i][j] = memory * R_xx[i][j] + sxx[i][j]   (j <= i)      R_x[i] = memory * R_x[i] + sx[i]      w = memory * w + count
//   the window sums are zeroed
//   w < min_count (or w not a number): skip
//   m_i = R_x[i] / w        A[i][j] = R_xx[i][j] / w - m_i * m_j   (j <= i)
//   tr = A[0][0] + A[1][1] + ... ascending from +0;   A[i][i] += jitter * (tr / dim)
//   left-looking column Cholesky, column j = 0 .. dim - 1:
//     s_i = A[i][j];  for k = 0 .. j - 1 ascending:  s_i = s_i - C[i][k] * C[j][k]            (i >= j)
//     s_j not finite or not > 0: skip;   C[j][j] = sqrt(s_j);   C[i][j] = s_i / C[j][j]       (i > j)
//   any C[i][j] not finite: skip
// On success L[i][j] = (float) C[i][j] for j <= i (the strict upper triangle of L is not touched).  On a skip L keeps its bits
// and the caller counts one skip; the running triple keeps what the window added either way.
#pragma once

#include <cmath>

#include "schedule.h"

namespace ptrwm {

// ---- the geometry of the proposal kernel (capi.hip precond_propose_kernel) ------------------------------------------------------
// A workgroup of kPrecThreads threads (kPrecWaves waves) takes tiles of kPrecRows replica rows; wave w owns rows 16 w .. 16 w + 15
// of a tile.  dim is padded to prec_blocks(dim) blocks of kPrecBlock = 16.  The increment of block bi of a wave's 16 rows is a
// 16 x 16 product accumulated by v_mfma_f32_16x16x4_f32 over the K-steps ks with 4 ks <= 16 bi + 15 (the triangle halves the
// work), kPrecK = 4 values of k at a time, k ascending inside the instruction and from one instruction to the next.
constexpr int kPrecBlock = 16;
constexpr int kPrecK = 4;
constexpr int kPrecThreads = 256;
constexpr int kPrecWaves = kPrecThreads / 64;
constexpr int kPrecRows = kPrecBlock * kPrecWaves;  // 64
constexpr int kPrecMaxDim = 104;                    // PTRWM_MAX_DIM of include/ptrwm.h

// the launch: workgroup b walks tiles b, b + grid, ... - no more workgroups than keep every compute unit busy, since each stages
// the factor once (cus: the device's compute units; 256 where the count is unknown)
constexpr int kPrecGroupsPerCu = 8;
PTRWM_HD constexpr long long prec_grid_cap(int cus) { return (long long)kPrecGroupsPerCu * (cus > 0 ? cus : 256); }
PTRWM_HD constexpr long long prec_grid(long long n_tiles, int cus) { return n_tiles < prec_grid_cap(cus) ? n_tiles : prec_grid_cap(cus); }

PTRWM_HD constexpr int prec_blocks(int dim) { return (dim + kPrecBlock - 1) / kPrecBlock; }
PTRWM_HD constexpr int prec_padded(int dim) { return kPrecBlock * prec_blocks(dim); }
// one past the last k the chain of coordinate i visits, and the K-steps of block bi
PTRWM_HD constexpr int prec_chain_end(int i) { return kPrecBlock * (i / kPrecBlock + 1); }
PTRWM_HD constexpr int prec_ksteps(int bi) { return kPrecBlock * (bi + 1) / kPrecK; }
// the word of the accept uniform, and the Philox blocks of a step (NormalProposal's: proposals.h normal_blocks)
PTRWM_HD constexpr int prec_accept_word(int dim) { return 2 * ((dim + 1) / 2); }
PTRWM_HD constexpr int prec_philox_blocks(int dim) { return prec_accept_word(dim) / 4 + 1; }

// LDS, in floats: the factor slab [padded][stride], the z slab [kPrecRows][stride], the x slab of a tile's contiguous run
// (kernel.h stage_copy: the run sits at float prec_x_at(head, row, d), head = 0..3 the alignment of the PROPOSALS' run, and
// needs room for 3 floats more).  stride = padded + 2: a half-wave's operand read - 16 rows x 2 values of k - then touches 32
// different banks.
PTRWM_HD constexpr int prec_stride(int dim) { return prec_padded(dim) + 2; }
PTRWM_HD constexpr int prec_l_floats(int dim) { return prec_padded(dim) * prec_stride(dim); }
PTRWM_HD constexpr int prec_z_floats(int dim) { return kPrecRows * prec_stride(dim); }
PTRWM_HD constexpr int prec_x_floats(int dim) { return (kPrecRows * dim + 4 + 3) & ~3; }
PTRWM_HD constexpr int prec_l_offset(int) { return 0; }
PTRWM_HD constexpr int prec_z_offset(int dim) { return prec_l_floats(dim); }
PTRWM_HD constexpr int prec_x_offset(int dim) { return (prec_l_floats(dim) + prec_z_floats(dim) + 3) & ~3; }  // (16-byte aligned)
PTRWM_HD constexpr int prec_lds_floats(int dim) { return prec_x_offset(dim) + prec_x_floats(dim); }
PTRWM_HD constexpr int prec_lds_bytes(int dim) { return 4 * prec_lds_floats(dim); }

PTRWM_HD constexpr int prec_l_at(int i, int k, int dim) { return prec_l_offset(dim) + i * prec_stride(dim) + k; }
PTRWM_HD constexpr int prec_z_at(int row, int k, int dim) { return prec_z_offset(dim) + row * prec_stride(dim) + k; }
PTRWM_HD constexpr int prec_x_at(int head, int row, int d, int dim) { return prec_x_offset(dim) + head + row * dim + d; }

// staging of the factor, once per workgroup: pass p = 0 .. prec_l_passes - 1 is block pair (bi, bk), bk <= bi, numbered row by
// row through the lower triangle of blocks (the blocks above it are never read); thread tid writes element
// (16 bi + tid / 16, 16 bk + tid % 16), the caller's value where k <= i < dim and zero elsewhere
PTRWM_HD constexpr int prec_l_passes(int dim) { return prec_blocks(dim) * (prec_blocks(dim) + 1) / 2; }
PTRWM_HD constexpr int prec_l_pass_row(int p) { return (p >= 1) + (p >= 3) + (p >= 6) + (p >= 10) + (p >= 15) + (p >= 21); }
PTRWM_HD constexpr int prec_l_pass_col(int p) { return p - prec_l_pass_row(p) * (prec_l_pass_row(p) + 1) / 2; }
PTRWM_HD constexpr int prec_l_stage_i(int p, int tid) { return kPrecBlock * prec_l_pass_row(p) + (tid >> 4); }
PTRWM_HD constexpr int prec_l_stage_k(int p, int tid) { return kPrecBlock * prec_l_pass_col(p) + (tid & 15); }
PTRWM_HD constexpr bool prec_l_live(int i, int k, int dim) { return k <= i && i < dim; }

// the normals of a tile: work item e = 0 .. prec_z_items - 1 is Philox block e / kPrecRows of row e % kPrecRows; it writes
// z[row][4 c .. 4 c + 3] - zeros at and past dim, so that the pad columns of the slab are written too - and, where
// c == prec_accept_word / 4, the accept uniform (word prec_accept_word % 4 of the block: 0 or 2).  Where dim is a multiple of 16
// that block lies behind the slab's columns: it writes the uniform only (prec_z_written).
PTRWM_HD constexpr int prec_z_blocks(int dim) {
  return prec_padded(dim) / 4 > prec_philox_blocks(dim) ? prec_padded(dim) / 4 : prec_philox_blocks(dim);
}
PTRWM_HD constexpr int prec_z_items(int dim) { return kPrecRows * prec_z_blocks(dim); }
PTRWM_HD constexpr bool prec_z_written(int c, int dim) { return 4 * c < prec_padded(dim); }
PTRWM_HD constexpr int prec_z_item_row(int e) { return e % kPrecRows; }
PTRWM_HD constexpr int prec_z_item_block(int e) { return e / kPrecRows; }

// operands of K-step ks for block bi: lane l of wave w reads A = Lp[16 bi + (l & 15)][4 ks + (l >> 4)] and
// B = zp[row 16 w + (l & 15)][4 ks + (l >> 4)]
PTRWM_HD constexpr int prec_a_row(int bi, int lane) { return kPrecBlock * bi + (lane & 15); }
PTRWM_HD constexpr int prec_b_row(int w, int lane) { return kPrecBlock * w + (lane & 15); }
PTRWM_HD constexpr int prec_operand_k(int ks, int lane) { return kPrecK * ks + (lane >> 4); }
// accumulator: register reg = 0..3 of lane l holds coordinate 16 bi + 4 (l >> 4) + reg of row 16 w + (l & 15)
PTRWM_HD constexpr int prec_acc_dim(int bi, int lane, int reg) { return kPrecBlock * bi + 4 * (lane >> 4) + reg; }
PTRWM_HD constexpr int prec_acc_row(int w, int lane) { return kPrecBlock * w + (lane & 15); }
// ... and it is written to the slab when it is a live coordinate of a live row
PTRWM_HD constexpr bool prec_acc_live(int row, int d, int n_rows, int dim) { return row < n_rows && d < dim; }

// ---- the proposal rule on the host (the direct chain: what the kernel is held to) -------------------------------------------------
// y [dim] from x, the factor (row stride dim), z [dim] and the scale
inline void precond_propose_row(const float *x, const float *chol, const float *z, float s_t, int dim, float *y) {
  for (int i = 0; i < dim; ++i) {
    float acc = 0.0f;
    for (int k = 0; k < prec_chain_end(i); ++k) {
      const float l = (k <= i) ? chol[i * dim + k] : 0.0f, zz = (k < dim) ? z[k] : 0.0f;
      acc = fmaf(l, zz, acc);
    }
    y[i] = fmaf(s_t, acc, x[i]);
  }
}

// ---- the update rule ------------------------------------------------------------------------------------------------------------------
// The element operations, each rounded on its own.  (The pragma keeps the device compiler from contracting them; a host compiler
// is given -ffp-contract=off.)
#if defined(__clang__)
#define PTRWM_PREC_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define PTRWM_PREC_NO_CONTRACT
#endif
PTRWM_HD inline double prec_decay_add(double memory, double running, double window) {
  PTRWM_PREC_NO_CONTRACT
  const double p = memory * running;
  return p + window;
}
PTRWM_HD inline double prec_centered(double rxx, double w, double mi, double mj) {
  PTRWM_PREC_NO_CONTRACT
  const double q = rxx / w, p = mi * mj;
  return q - p;
}
PTRWM_HD inline double prec_jitter_term(double jitter, double tr, int dim) {
  PTRWM_PREC_NO_CONTRACT
  const double q = tr / (double)dim;
  return jitter * q;
}
PTRWM_HD inline double prec_sub_prod(double s, double a, double b) {
  PTRWM_PREC_NO_CONTRACT
  const double p = a * b;
  return s - p;
}
PTRWM_HD inline bool prec_pivot_ok(double s) { return s > 0.0 && s - s == 0.0; }  // (finite and positive; a NaN fails both)
PTRWM_HD inline bool prec_finite(double v) { return v - v == 0.0; }
PTRWM_HD inline bool prec_weight_ok(double w, double min_count) { return w >= min_count && prec_finite(w); }

// packed lower triangle: element (i, j), j <= i
PTRWM_HD constexpr int prec_tri(int i, int j) { return i * (i + 1) / 2 + j; }
PTRWM_HD constexpr int prec_tri_size(int dim) { return dim * (dim + 1) / 2; }
// one thread per row in one workgroup, the work matrix in LDS as doubles
constexpr int kPrecUpdateThreads = 128;
PTRWM_HD constexpr int prec_update_lds_bytes(int dim) { return 8 * (prec_tri_size(dim) + dim); }
static_assert(kPrecMaxDim <= kPrecUpdateThreads, "precond_update_kernel: one thread per row in one workgroup");

enum PrecondOutcome { kPrecUpdated = 0, kPrecFewDraws = 1, kPrecNotPositive = 2 };

// The update on the host, sequentially: sxx [dim, dim] (lower triangle read), sx [dim], count; run_xx [dim, dim] (lower
// triangle), run_x [dim], run_w [1]; chol [dim, dim] in/out; work: prec_tri_size(dim) + dim doubles of scratch.
inline int precond_update(double *sxx, double *sx, long long *count, double *run_xx, double *run_x, double *run_w, double memory,
                          double jitter, double min_count, int dim, float *chol, double *work) {
  double *A = work, *m = work + prec_tri_size(dim);
  for (int i = 0; i < dim; ++i) {
    for (int j = 0; j <= i; ++j) {
      run_xx[i * dim + j] = prec_decay_add(memory, run_xx[i * dim + j], sxx[i * dim + j]);
      sxx[i * dim + j] = 0.0;
    }
    run_x[i] = prec_decay_add(memory, run_x[i], sx[i]);
    sx[i] = 0.0;
  }
  const double w = prec_decay_add(memory, *run_w, (double)*count);
  *run_w = w;
  *count = 0;
  if (!prec_weight_ok(w, min_count)) return kPrecFewDraws;
  for (int i = 0; i < dim; ++i) m[i] = run_x[i] / w;
  for (int i = 0; i < dim; ++i)
    for (int j = 0; j <= i; ++j) A[prec_tri(i, j)] = prec_centered(run_xx[i * dim + j], w, m[i], m[j]);
  double tr = 0.0;
  for (int i = 0; i < dim; ++i) tr = tr + A[prec_tri(i, i)];
  const double jt = prec_jitter_term(jitter, tr, dim);
  for (int i = 0; i < dim; ++i) A[prec_tri(i, i)] = A[prec_tri(i, i)] + jt;
  for (int j = 0; j < dim; ++j) {
    for (int i = j; i < dim; ++i) {
      double s = A[prec_tri(i, j)];
      for (int k = 0; k < j; ++k) s = prec_sub_prod(s, A[prec_tri(i, k)], A[prec_tri(j, k)]);
      A[prec_tri(i, j)] = s;
    }
    const double piv = A[prec_tri(j, j)];
    if (!prec_pivot_ok(piv)) return kPrecNotPositive;
    const double d = sqrt(piv);
    A[prec_tri(j, j)] = d;
    for (int i = j + 1; i < dim; ++i) A[prec_tri(i, j)] = A[prec_tri(i, j)] / d;
  }
  for (int e = 0; e < prec_tri_size(dim); ++e)
    if (!prec_finite((double)(float)A[e])) return kPrecNotPositive;  // (as the float it is stored as)
  for (int i = 0; i < dim; ++i)
    for (int j = 0; j <= i; ++j) chol[i * dim + j] = (float)A[prec_tri(i, j)];
  return kPrecUpdated;
}

}  // namespace ptrwm
