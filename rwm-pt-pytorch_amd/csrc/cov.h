// The rule of the pooled posterior covariance, stated once: when a snapshot is due, what one snapshot adds to which sum - and,
// below it, the geometry of the snapshot kernel (cov_geometry and the index maps next to it).  Plain C++ (no HIP include): the
// snapshot kernel of capi.hip calls it, tests/cov_test.cpp checks it on the CPU against brute force and replays the kernel's
// staging, block products and flush with it.
//
// Snapshots.  A snapshot is due at every step with periodic_step_due(step_counter, burn_in, every) (schedule.h: the rule of the
// histograms and of the autocovariance).
// Sums, for the first `temps` temperatures t, all += and all double, summed over the local chains:
//   sxx[t, i, j] += x[t, i] * x[t, j]     for j <= i < dim  (the lower triangle, diagonal included; the strict upper triangle
//                                                            is never written)
//   sx[t, i]     += x[t, i]
//   count        += n_chains                                 (int64, one scalar)
// x is the state in slot t of the ladder after the whole step (MH move and that step's swap event): the values a trace with
// trace_every = every records.  One term is both values converted to double and multiplied: exact in fp64 for float states;
// for double states the product may be fused into the running sum (the matrix unit does).  Only the order of the additions is
// free.  Estimators, on the host, with n = count and m = sx / n:  cov = sxx / n - m m^T, mirrored to both triangles.
// Raw sums: fp64 loses about log10(1 + mean^2 / var) digits per coordinate, as the moments' sum_sq does.
#pragma once

#include "schedule.h"

namespace ptrwm {

// ---- the geometry of one snapshot (capi.hip cov_snapshot_kernel) ---------------------------------------------------------------
// A workgroup of kCovThreads threads (kCovWaves waves) takes ONE covered temperature (blockIdx.y) and a tile of kCovChains
// chains (blockIdx.x).  The dim coordinates are padded to cov_blocks(dim) blocks of kCovBlock = 16; the Gram matrix of the tile
// is the lower triangle of blocks, pair (bi, bj), bj <= bi, each a 16 x 16 product accumulated by the fp64 matrix instruction
// v_mfma_f64_16x16x4_f64 with K running over chains, kCovK = 4 at a time.
constexpr int kCovBlock = 16;
constexpr int kCovK = 4;
constexpr int kCovThreads = 256;
constexpr int kCovWaves = kCovThreads / 64;
constexpr int kCovMaxDim = 104;                                             // PTRWM_MAX_DIM of include/ptrwm.h
constexpr int kCovMaxBlocks = (kCovMaxDim + kCovBlock - 1) / kCovBlock;     // 7
constexpr int kCovMaxPairs = kCovMaxBlocks * (kCovMaxBlocks + 1) / 2;       // 28
constexpr int kCovPairsPerWave = (kCovMaxPairs + kCovWaves - 1) / kCovWaves;  // 7 accumulators of 8 VGPRs a wave
// The chains of a tile pass through LDS in kCovSubTiles sub-tiles of kCovSubTile chains: rows of doubles, one per chain.
constexpr int kCovSubTile = 32;
constexpr int kCovSubTiles = 8;
constexpr int kCovChains = kCovSubTile * kCovSubTiles;  // 256
constexpr int kCovKSteps = kCovSubTile / kCovK;         // matrix instructions per pair and sub-tile

PTRWM_HD constexpr int cov_blocks(int dim) { return (dim + kCovBlock - 1) / kCovBlock; }
PTRWM_HD constexpr int cov_padded(int dim) { return kCovBlock * cov_blocks(dim); }
// doubles from one chain's LDS row to the next: the padded dim, made an ODD number of 16-double (128-byte) blocks, so that the
// two rows a 32-lane half of a ds_read_b64 touches lie in different halves of the 256-byte bank row
PTRWM_HD constexpr int cov_row_stride(int dim) { return kCovBlock * (cov_blocks(dim) | 1); }
PTRWM_HD constexpr int cov_lds_doubles(int dim) { return kCovSubTile * cov_row_stride(dim); }

// block pairs: numbered row by row through the lower triangle, dealt to the waves round-robin; a wave keeps pair p in its
// accumulator cov_pair_slot(p) for the whole tile
PTRWM_HD constexpr int cov_pairs(int blocks) { return blocks * (blocks + 1) / 2; }
PTRWM_HD constexpr int cov_pair_index(int bi, int bj) { return bi * (bi + 1) / 2 + bj; }
// ... and back: the block row of pair p is the largest bi with bi (bi + 1) / 2 <= p (p < kCovMaxPairs)
PTRWM_HD constexpr int cov_pair_row(int p) { return (p >= 1) + (p >= 3) + (p >= 6) + (p >= 10) + (p >= 15) + (p >= 21); }
PTRWM_HD constexpr int cov_pair_col(int p) { return p - cov_pair_index(cov_pair_row(p), 0); }
PTRWM_HD constexpr int cov_pair_wave(int p) { return p % kCovWaves; }
PTRWM_HD constexpr int cov_pair_slot(int p) { return p / kCovWaves; }
// ... and back: the pair in accumulator `slot` of wave w, and how many pairs of `pairs` wave w owns
PTRWM_HD constexpr int cov_wave_pair(int w, int slot) { return w + kCovWaves * slot; }
PTRWM_HD constexpr int cov_wave_pairs(int w, int pairs) { return pairs > w ? (pairs - w + kCovWaves - 1) / kCovWaves : 0; }
// sx of block b is summed by the wave that owns the diagonal pair (b, b): it reads that block's values anyway
PTRWM_HD constexpr int cov_sx_wave(int b) { return cov_pair_wave(cov_pair_index(b, b)); }

// staging: element e = 0 .. kCovSubTile * dim - 1 of a sub-tile (thread e % kCovThreads) is coordinate e % dim of the
// sub-tile's chain e / dim - consecutive lanes read consecutive elements of a chain - and lands at cov_lds_at
PTRWM_HD constexpr int cov_stage_chain(int e, int dim) { return e / dim; }
PTRWM_HD constexpr int cov_stage_coord(int e, int dim) { return e % dim; }
PTRWM_HD constexpr int cov_lds_at(int chain, int coord, int dim) { return chain * cov_row_stride(dim) + coord; }

// operands: at K-step ks a lane reads, for block b, coordinate 16 b + (lane & 15) of the sub-tile's chain 4 ks + (lane >> 4) -
// the A operand of a pair (b, .) and the B operand of a pair (., b): one f64 per lane
PTRWM_HD constexpr int cov_operand_chain(int ks, int lane) { return kCovK * ks + (lane >> 4); }
PTRWM_HD constexpr int cov_operand_coord(int b, int lane) { return kCovBlock * b + (lane & 15); }

// flush: register reg = 0..3 of a lane's accumulator of pair (bi, bj) is element (i, j) of sxx
PTRWM_HD constexpr int cov_flush_i(int bi, int lane, int reg) { return kCovBlock * bi + (lane >> 4) + 4 * reg; }
PTRWM_HD constexpr int cov_flush_j(int bj, int lane) { return kCovBlock * bj + (lane & 15); }
// ... and it is flushed when it lies in the lower triangle of the live coordinates (a pad element never is)
PTRWM_HD constexpr bool cov_flushed(int i, int j, int dim) { return j <= i && i < dim; }
// sx: after the four K-quarters of a column have met, lanes 0..15 of the owning wave flush coordinate 16 b + lane
PTRWM_HD constexpr bool cov_sx_flushed(int b, int lane, int dim) { return lane < kCovBlock && kCovBlock * b + lane < dim; }

struct CovGeometry {
  int blocks, pairs, stride, lds_bytes, chains;
};

inline CovGeometry cov_geometry(int dim) {
  CovGeometry g;
  g.blocks = cov_blocks(dim);
  g.pairs = cov_pairs(g.blocks);
  g.stride = cov_row_stride(dim);
  g.lds_bytes = cov_lds_doubles(dim) * (int)sizeof(double);
  g.chains = kCovChains;
  return g;
}

}  // namespace ptrwm
