// csrc/precond.h on the CPU.  Plain C++, its own main: tests/test_precond_host.py compiles it with
// g++ -fsanitize=address,undefined and runs it.
//  1. the index maps of the proposal kernel for dims 1, 3, 4, 5, 16, 17, 30, 33, 64, 104 and row counts 1, 5, 64: every
//     (row, coordinate) of a tile is produced by exactly one accumulator element, every operand read lands inside the staged
//     slabs on an element that was written, and the LDS byte count is what the maps touch;
//  2. a replay of the kernel - staging of the factor, the states and the normals through an LDS image, the K-steps in the matrix
//     instruction's operand and result layout (k ascending inside an instruction), the epilogue in place - against the direct
//     chain of the rule, bit for bit;
//  3. the update rule: L L^T against A within float rounding plus Cholesky's backward error, the three skips, `memory`;
//  4. the launch: 1 <= prec_grid <= n_tiles and prec_grid <= 8 cus (256 compute units where the count is unknown).
// With "update" it reads cases from stdin (one per line: dim memory jitter min_count count, then as bit patterns sxx, sx,
// run_xx, run_x, run_w (uint64) and chol (uint32)) and prints "outcome zeroed chol.. run_xx.. run_x.. run_w" per case; with
// "propose" lines "dim n s_bits x.. chol.. z.." (uint32 bit patterns, x and z [n, dim]) give "y.." of the REPLAY and of the
// direct chain; with "geometry" dims give "blocks padded stride lds_bytes z_items l_passes"; with "grid" pairs "n_tiles cus"
// give the workgroups of the launch.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../rwm-pt-pytorch_amd/csrc/precond.h"

using namespace ptrwm;

static long long g_checks = 0;
#define CHECK(cond, ...)                                     \
  do {                                                       \
    ++g_checks;                                              \
    if (!(cond)) {                                           \
      std::printf("FAILED %s (line %d): ", #cond, __LINE__); \
      std::printf(__VA_ARGS__);                              \
      std::printf("\n");                                     \
      std::exit(1);                                          \
    }                                                        \
  } while (0)

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint64_t next_u64() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return g_rng;
}
static double uniform() { return (double)(next_u64() >> 11) * 0x1p-53; }
static double normal() { return std::sqrt(-2.0 * std::log(1.0 - uniform())) * std::cos(6.283185307179586 * uniform()); }

static uint32_t fbits(float v) {
  uint32_t b;
  std::memcpy(&b, &v, 4);
  return b;
}
static float bits_f(uint32_t b) {
  float v;
  std::memcpy(&v, &b, 4);
  return v;
}
static uint64_t dbits(double v) {
  uint64_t b;
  std::memcpy(&b, &v, 8);
  return b;
}
static double bits_d(uint64_t b) {
  double v;
  std::memcpy(&v, &b, 8);
  return v;
}

// The kernel, replayed: an LDS image that starts as NaN everywhere with a map of what was written; `head` is the alignment of
// the proposals' run.  Returns y [n_rows, dim]; counts the reads and the largest float touched.
struct Replay {
  std::vector<float> lds;
  std::vector<char> written;
  int max_touched = -1;
  long long reads = 0;
  int dim;
  explicit Replay(int d) : lds((size_t)prec_lds_floats(d), std::numeric_limits<float>::quiet_NaN()), written((size_t)prec_lds_floats(d), 0), dim(d) {}
  void put(int at, float v) {
    CHECK(at >= 0 && at < (int)lds.size(), "dim %d: write at %d of %zu", dim, at, lds.size());
    lds[(size_t)at] = v;
    written[(size_t)at] = 1;
    if (at > max_touched) max_touched = at;
  }
  float get(int at) {
    CHECK(at >= 0 && at < (int)lds.size(), "dim %d: read at %d of %zu", dim, at, lds.size());
    CHECK(written[(size_t)at], "dim %d: float %d read before it was written", dim, at);
    ++reads;
    return lds[(size_t)at];
  }
};

static std::vector<float> replay_tile(int dim, int n_rows, int head, const float *x, const float *chol, const float *z, const float *scale,
                                      std::vector<int> *owners, int *max_touched) {
  Replay r(dim);
  // the factor: one pass per lower block pair, 256 threads
  for (int p = 0; p < prec_l_passes(dim); ++p)
    for (int tid = 0; tid < kPrecThreads; ++tid) {
      const int i = prec_l_stage_i(p, tid), k = prec_l_stage_k(p, tid);
      CHECK(i < prec_padded(dim) && k < prec_padded(dim) && k / kPrecBlock <= i / kPrecBlock, "dim %d: pass %d stages (%d, %d)", dim, p, i, k);
      // (the caller's strict upper triangle is never read: prec_l_live guards the load)
      r.put(prec_l_at(i, k, dim), prec_l_live(i, k, dim) ? chol[i * dim + k] : 0.0f);
    }
  // the states: element e of the run at head + e
  for (int e = 0; e < n_rows * dim; ++e) r.put(prec_x_offset(dim) + head + e, x[e]);
  // the normals
  std::vector<int> z_writes((size_t)kPrecRows * prec_padded(dim), 0);
  int uniforms = 0;
  for (int e = 0; e < prec_z_items(dim); ++e) {
    const int row = prec_z_item_row(e), c = prec_z_item_block(e);
    CHECK(row >= 0 && row < kPrecRows && c >= 0 && c < prec_z_blocks(dim), "dim %d: item %d is (%d, %d)", dim, e, row, c);
    if (row >= n_rows) continue;
    if (c == prec_accept_word(dim) / 4) ++uniforms;
    if (!prec_z_written(c, dim)) continue;
    for (int q = 0; q < 4; ++q) {
      const int k = 4 * c + q;
      CHECK(k < prec_padded(dim), "dim %d: z column %d", dim, k);
      r.put(prec_z_at(row, k, dim), k < dim ? z[row * dim + k] : 0.0f);
      ++z_writes[(size_t)row * prec_padded(dim) + k];
    }
  }
  CHECK(uniforms == n_rows, "dim %d: %d accept uniforms for %d rows", dim, uniforms, n_rows);
  for (int row = 0; row < n_rows; ++row)
    for (int k = 0; k < prec_padded(dim); ++k) CHECK(z_writes[(size_t)row * prec_padded(dim) + k] == 1, "dim %d: z (%d, %d) written %d times", dim, row, k, z_writes[(size_t)row * prec_padded(dim) + k]);
  // the waves
  if (owners) owners->assign((size_t)n_rows * dim, 0);
  for (int w = 0; w < kPrecWaves; ++w) {
    if (kPrecBlock * w >= n_rows) continue;
    for (int bi = 0; bi < prec_blocks(dim); ++bi) {
      float acc[64][4];
      for (auto &l : acc) l[0] = l[1] = l[2] = l[3] = 0.0f;
      CHECK(kPrecK * prec_ksteps(bi) == prec_chain_end(kPrecBlock * bi) && kPrecK * (prec_ksteps(bi) - 1) <= kPrecBlock * bi + 15, "block %d: %d K-steps", bi, prec_ksteps(bi));
      for (int ks = 0; ks < prec_ksteps(bi); ++ks) {
        float A[16][4], Bm[4][16];
        for (int lane = 0; lane < 64; ++lane) {
          const int ar = prec_a_row(bi, lane), br = prec_b_row(w, lane), k = prec_operand_k(ks, lane);
          CHECK(ar < prec_padded(dim) && k < prec_padded(dim) && br < kPrecRows, "dim %d: operand (%d | %d, %d)", dim, ar, br, k);
          A[lane & 15][lane >> 4] = r.get(prec_l_at(ar, k, dim));
          // (a dead row's column of B is never written: it feeds a dead column of the result only)
          Bm[lane >> 4][lane & 15] = br < n_rows ? r.get(prec_z_at(br, k, dim)) : std::numeric_limits<float>::quiet_NaN();
        }
        // D[i][j] = the chain over the instruction's four k, ascending, onto C; lane l, register reg holds D[4 (l >> 4) + reg][l & 15]
        for (int lane = 0; lane < 64; ++lane)
          for (int reg = 0; reg < 4; ++reg) {
            const int i = 4 * (lane >> 4) + reg, j = lane & 15;
            for (int kk = 0; kk < kPrecK; ++kk) acc[lane][reg] = fmaf(A[i][kk], Bm[kk][j], acc[lane][reg]);
          }
      }
      for (int lane = 0; lane < 64; ++lane)
        for (int reg = 0; reg < 4; ++reg) {
          const int row = prec_acc_row(w, lane), d = prec_acc_dim(bi, lane, reg);
          if (!prec_acc_live(row, d, n_rows, dim)) continue;
          if (owners) ++(*owners)[(size_t)row * dim + d];
          const int at = prec_x_at(head, row, d, dim);
          r.put(at, fmaf(scale[row], acc[lane][reg], r.get(at)));
        }
    }
  }
  std::vector<float> y((size_t)n_rows * dim);
  for (int e = 0; e < n_rows * dim; ++e) y[(size_t)e] = r.get(prec_x_offset(dim) + head + e);
  if (max_touched) *max_touched = r.max_touched;
  return y;
}

static const int kDims[] = {1, 3, 4, 5, 16, 17, 30, 33, 64, 104};
static const int kRows[] = {1, 5, 64};

// the launch: at least one workgroup, none without a tile, at most kPrecGroupsPerCu per compute unit (256 where unknown)
static void test_grid() {
  static_assert(kPrecGroupsPerCu == 8, "the launch");
  for (int cus : {-1, 0, 1, 2, 7, 64, 256, 304, 1 << 20})
    for (long long n_tiles : {1ll, 2ll, 15ll, 16ll, 17ll, 2047ll, 2048ll, 2049ll, 4134ll, 32768ll, 1ll << 31, 1ll << 40}) {
      const long long g = prec_grid(n_tiles, cus), cap = 8ll * (cus > 0 ? cus : 256);
      CHECK(1 <= g && g <= n_tiles && g <= cap, "grid(%lld, %d) = %lld", n_tiles, cus, g);
      CHECK(g == n_tiles || g == cap, "grid(%lld, %d) = %lld: neither every tile nor the cap", n_tiles, cus, g);
    }
}

static void test_maps_and_replay() {
  static_assert(kPrecRows == 64 && kPrecThreads == 256 && kPrecBlock == 16 && kPrecK == 4, "the tile");
  for (int dim : kDims) {
    CHECK(prec_blocks(dim) == (dim + 15) / 16 && prec_padded(dim) >= dim && prec_padded(dim) - dim < 16, "dim %d", dim);
    CHECK(prec_stride(dim) >= prec_padded(dim) && prec_stride(dim) % 32 == 2 + (prec_padded(dim) % 32), "dim %d: stride %d", dim, prec_stride(dim));
    CHECK(prec_x_offset(dim) % 4 == 0 && prec_z_offset(dim) == prec_l_floats(dim) && prec_x_offset(dim) >= prec_z_offset(dim) + prec_z_floats(dim), "dim %d: slabs", dim);
    CHECK(prec_lds_bytes(dim) <= 160 * 1024, "dim %d: %d bytes of LDS", dim, prec_lds_bytes(dim));
    CHECK(prec_philox_blocks(dim) == (2 * ((dim + 1) / 2)) / 4 + 1 && prec_z_blocks(dim) >= prec_philox_blocks(dim) && 4 * prec_z_blocks(dim) >= prec_padded(dim), "dim %d: blocks", dim);
    CHECK(prec_accept_word(dim) % 4 == 0 || prec_accept_word(dim) % 4 == 2, "dim %d: accept word", dim);
    for (int n_rows : kRows)
      for (int head = 0; head < 4; head += 3) {
        std::vector<float> x((size_t)n_rows * dim), z((size_t)n_rows * dim), chol((size_t)dim * dim), scale((size_t)n_rows);
        for (auto &v : x) v = (float)normal();
        for (auto &v : z) v = (float)normal();
        for (int i = 0; i < dim; ++i)
          for (int k = 0; k < dim; ++k) chol[(size_t)i * dim + k] = k <= i ? (float)normal() : std::numeric_limits<float>::quiet_NaN();
        for (auto &v : scale) v = (float)(0.1 + uniform());
        std::vector<int> owners;
        int max_touched = -1;
        const std::vector<float> y = replay_tile(dim, n_rows, head, x.data(), chol.data(), z.data(), scale.data(), &owners, &max_touched);
        for (int e = 0; e < n_rows * dim; ++e) CHECK(owners[(size_t)e] == 1, "dim %d rows %d: element %d has %d owners", dim, n_rows, e, owners[(size_t)e]);
        std::vector<float> want((size_t)dim);
        for (int row = 0; row < n_rows; ++row) {
          precond_propose_row(x.data() + (size_t)row * dim, chol.data(), z.data() + (size_t)row * dim, scale[(size_t)row], dim, want.data());
          for (int d = 0; d < dim; ++d)
            CHECK(fbits(want[(size_t)d]) == fbits(y[(size_t)row * dim + d]), "dim %d rows %d head %d: (%d, %d) replay %a chain %a", dim, n_rows, head, row, d, y[(size_t)row * dim + d], want[(size_t)d]);
        }
        // the byte count is what the maps touch: with every row live and the run three floats in, the last float of the run is
        // the last float touched, and the slab ends within its rounding to 16 bytes plus the copy's overhang (kernel.h stage_copy)
        if (n_rows == kPrecRows && head == 3) {
          CHECK(max_touched == prec_x_offset(dim) + 3 + kPrecRows * dim - 1, "dim %d: last float touched %d", dim, max_touched);
          CHECK(prec_lds_floats(dim) > max_touched && prec_lds_floats(dim) - (max_touched + 1) < 4, "dim %d: %d floats, last touched %d", dim, prec_lds_floats(dim), max_touched);
          CHECK(prec_lds_bytes(dim) == 4 * prec_lds_floats(dim), "dim %d: bytes", dim);
        }
      }
  }
}

// ---- the update rule ------------------------------------------------------------------------------------------------------------------
struct Sums {
  int dim;
  std::vector<double> sxx, sx, run_xx, run_x;
  double run_w = 0.0;
  long long count = 0;
  std::vector<float> chol;
};

// n draws of N(mu, M M^T), M random with singular values between 1 and cond
static Sums random_sums(int dim, int n, double spread) {
  Sums s;
  s.dim = dim;
  s.sxx.assign((size_t)dim * dim, 0.0);
  s.sx.assign((size_t)dim, 0.0);
  s.run_xx.assign((size_t)dim * dim, 0.0);
  s.run_x.assign((size_t)dim, 0.0);
  s.chol.assign((size_t)dim * dim, 0.0f);
  for (int i = 0; i < dim; ++i) s.chol[(size_t)i * dim + i] = 1.0f;
  std::vector<double> M((size_t)dim * dim), mu((size_t)dim), xv((size_t)dim), g((size_t)dim);
  for (int i = 0; i < dim; ++i) {
    mu[(size_t)i] = normal();
    for (int j = 0; j < dim; ++j) M[(size_t)i * dim + j] = normal() * std::pow(spread, (double)j / (dim > 1 ? dim - 1 : 1)) / std::sqrt((double)dim);
  }
  for (int c = 0; c < n; ++c) {
    for (auto &v : g) v = normal();
    for (int i = 0; i < dim; ++i) {
      double a = mu[(size_t)i];
      for (int j = 0; j < dim; ++j) a += M[(size_t)i * dim + j] * g[(size_t)j];
      xv[(size_t)i] = (double)(float)a;
    }
    for (int i = 0; i < dim; ++i) {
      s.sx[(size_t)i] += xv[(size_t)i];
      for (int j = 0; j <= i; ++j) s.sxx[(size_t)i * dim + j] += xv[(size_t)i] * xv[(size_t)j];
    }
  }
  s.count = n;
  return s;
}

static int run_update(Sums &s, double memory, double jitter, double min_count) {
  std::vector<double> work((size_t)prec_tri_size(s.dim) + s.dim);
  return precond_update(s.sxx.data(), s.sx.data(), &s.count, s.run_xx.data(), s.run_x.data(), &s.run_w, memory, jitter, min_count, s.dim,
                        s.chol.data(), work.data());
}

static void test_update() {
  for (int dim : {1, 2, 5, 16, 30, 64, 104}) {
    for (double spread : {1.0, 30.0, 1000.0}) {
      Sums s = random_sums(dim, 6 * dim + 10, spread);
      const Sums before = s;
      const double jitter = 1e-6;
      const int outcome = run_update(s, 0.5, jitter, 4.0 * dim);
      CHECK(outcome == kPrecUpdated, "dim %d spread %g: outcome %d", dim, spread, outcome);
      CHECK(s.count == 0 && s.run_w == (double)before.count, "dim %d: count %lld w %g", dim, s.count, s.run_w);
      // A, recomputed here from the sums (the running triple started empty: R = the window sums)
      const double w = (double)before.count;
      std::vector<double> A((size_t)dim * dim);
      double tr = 0.0;
      for (int i = 0; i < dim; ++i)
        for (int j = 0; j <= i; ++j) A[(size_t)i * dim + j] = before.sxx[(size_t)i * dim + j] / w - (before.sx[(size_t)i] / w) * (before.sx[(size_t)j] / w);
      for (int i = 0; i < dim; ++i) tr += A[(size_t)i * dim + i];
      for (int i = 0; i < dim; ++i) A[(size_t)i * dim + i] += jitter * (tr / dim);
      // |L L^T - A|_ij <= (2^-23 + 2^-48 + (dim + 1) 2^-52) (|L| |L^T|)_ij: the float rounding of both factors and Cholesky's
      // backward error
      const double bound = 0x1p-23 + 0x1p-48 + (dim + 1) * 0x1p-52;
      for (int i = 0; i < dim; ++i)
        for (int j = 0; j <= i; ++j) {
          double llt = 0.0, abs_llt = 0.0;
          for (int k = 0; k <= j; ++k) {
            const double p = (double)s.chol[(size_t)i * dim + k] * (double)s.chol[(size_t)j * dim + k];
            llt += p;
            abs_llt += std::fabs(p);
          }
          CHECK(std::fabs(llt - A[(size_t)i * dim + j]) <= bound * abs_llt, "dim %d spread %g: (%d, %d) L L^T %a A %a", dim, spread, i, j, llt, A[(size_t)i * dim + j]);
        }
      for (int i = 0; i < dim; ++i) {
        CHECK(s.chol[(size_t)i * dim + i] > 0.0f, "dim %d: diagonal %d", dim, i);
        for (int j = i + 1; j < dim; ++j) CHECK(s.chol[(size_t)i * dim + j] == 0.0f, "dim %d: the upper triangle was written", dim);
        for (int j = 0; j <= i; ++j) CHECK(s.sxx[(size_t)i * dim + j] == 0.0, "dim %d: sxx not zeroed", dim);
        CHECK(s.sx[(size_t)i] == 0.0, "dim %d: sx not zeroed", dim);
      }
    }
    // the skips: the factor keeps its bits, the outcome says which
    auto same_bits = [&](const Sums &a, const Sums &b) { return std::memcmp(a.chol.data(), b.chol.data(), a.chol.size() * 4) == 0; };
    {
      Sums s = random_sums(dim, 3 * dim, 10.0);  // w < min_count
      for (auto &v : s.chol) v = (float)normal();
      const Sums before = s;
      CHECK(run_update(s, 1.0, 1e-6, 4.0 * dim) == kPrecFewDraws && same_bits(s, before), "dim %d: few draws", dim);
      CHECK(s.run_w == 3.0 * dim && s.count == 0, "dim %d: the running triple keeps the window", dim);
      // ... and the next window brings the weight over the bar (memory 1: 3 dim + 3 dim draws)
      Sums t = random_sums(dim, 3 * dim, 10.0);
      s.sxx = t.sxx, s.sx = t.sx, s.count = t.count;
      CHECK(run_update(s, 1.0, 1e-6, 4.0 * dim) == kPrecUpdated && s.run_w == 6.0 * dim, "dim %d: second window", dim);
    }
    {
      Sums s = random_sums(dim, 6 * dim + 10, 10.0);  // a non-positive pivot: a variance of minus one
      for (auto &v : s.chol) v = (float)normal();
      s.sxx[(size_t)(dim - 1) * dim + (dim - 1)] = -(double)s.count;
      s.sx[(size_t)dim - 1] = 0.0;
      for (int j = 0; j < dim - 1; ++j) s.sxx[(size_t)(dim - 1) * dim + j] = 0.0;
      const Sums before = s;
      CHECK(run_update(s, 0.5, 0.0, 4.0 * dim) == kPrecNotPositive && same_bits(s, before), "dim %d: non-positive pivot", dim);
    }
    for (double bad : {std::numeric_limits<double>::infinity(), std::numeric_limits<double>::quiet_NaN()}) {
      Sums s = random_sums(dim, 6 * dim + 10, 10.0);  // a sum that is not finite
      for (auto &v : s.chol) v = (float)normal();
      s.sxx[(size_t)(dim / 2) * dim + 0] = bad;
      const Sums before = s;
      CHECK(run_update(s, 0.5, 1e-6, 4.0 * dim) == kPrecNotPositive && same_bits(s, before), "dim %d: a sum that is not finite", dim);
    }
    {
      // memory: R = memory R + window, w likewise
      Sums s = random_sums(dim, 6 * dim + 10, 3.0);
      for (auto &v : s.run_xx) v = 7.0;
      for (auto &v : s.run_x) v = -3.0;
      s.run_w = 100.0;
      const Sums before = s;
      run_update(s, 0.25, 1e-6, 1.0);
      CHECK(s.run_w == 0.25 * 100.0 + (double)before.count, "dim %d: w %g", dim, s.run_w);
      for (int i = 0; i < dim; ++i) {
        CHECK(s.run_x[(size_t)i] == 0.25 * -3.0 + before.sx[(size_t)i], "dim %d: run_x", dim);
        for (int j = 0; j < dim; ++j)
          CHECK(s.run_xx[(size_t)i * dim + j] == (j <= i ? 0.25 * 7.0 + before.sxx[(size_t)i * dim + j] : 7.0), "dim %d: run_xx (%d, %d)", dim, i, j);
      }
    }
  }
}

static bool read_u32(uint32_t *v) { return std::scanf("%" SCNu32, v) == 1; }
static bool read_u64(uint64_t *v) { return std::scanf("%" SCNu64, v) == 1; }

static int mode_update() {
  int dim;
  while (std::scanf("%d", &dim) == 1) {
    double memory, jitter, min_count;
    long long count;
    if (dim < 1 || dim > kPrecMaxDim || std::scanf("%lf %lf %lf %lld", &memory, &jitter, &min_count, &count) != 4) return 2;
    Sums s;
    s.dim = dim;
    s.count = count;
    auto read_d = [&](std::vector<double> &v, size_t n) {
      v.resize(n);
      for (auto &e : v) {
        uint64_t b;
        if (!read_u64(&b)) std::exit(2);
        e = bits_d(b);
      }
    };
    read_d(s.sxx, (size_t)dim * dim);
    read_d(s.sx, (size_t)dim);
    read_d(s.run_xx, (size_t)dim * dim);
    read_d(s.run_x, (size_t)dim);
    std::vector<double> w1;
    read_d(w1, 1);
    s.run_w = w1[0];
    s.chol.resize((size_t)dim * dim);
    for (auto &e : s.chol) {
      uint32_t b;
      if (!read_u32(&b)) return 2;
      e = bits_f(b);
    }
    const int outcome = run_update(s, memory, jitter, min_count);
    bool zeroed = s.count == 0;
    for (int i = 0; i < dim; ++i) {
      zeroed = zeroed && s.sx[(size_t)i] == 0.0;
      for (int j = 0; j <= i; ++j) zeroed = zeroed && s.sxx[(size_t)i * dim + j] == 0.0;
    }
    std::printf("%d %d", outcome, zeroed ? 1 : 0);
    for (float v : s.chol) std::printf(" %" PRIu32, fbits(v));
    for (double v : s.run_xx) std::printf(" %" PRIu64, dbits(v));
    for (double v : s.run_x) std::printf(" %" PRIu64, dbits(v));
    std::printf(" %" PRIu64 "\n", dbits(s.run_w));
  }
  return 0;
}

static int mode_propose() {
  int dim, n;
  while (std::scanf("%d %d", &dim, &n) == 2) {
    if (dim < 1 || dim > kPrecMaxDim || n < 1 || n > kPrecRows) return 2;
    std::vector<float> scale((size_t)n), x((size_t)n * dim), chol((size_t)dim * dim), z((size_t)n * dim);
    for (auto *v : {&scale, &x, &chol, &z})
      for (auto &e : *v) {
        uint32_t b;
        if (!read_u32(&b)) return 2;
        e = bits_f(b);
      }
    const std::vector<float> y = replay_tile(dim, n, 1, x.data(), chol.data(), z.data(), scale.data(), nullptr, nullptr);
    for (float v : y) std::printf("%" PRIu32 " ", fbits(v));
    std::vector<float> want((size_t)dim);
    for (int row = 0; row < n; ++row) {
      precond_propose_row(x.data() + (size_t)row * dim, chol.data(), z.data() + (size_t)row * dim, scale[(size_t)row], dim, want.data());
      for (float v : want) std::printf("%" PRIu32 " ", fbits(v));
    }
    std::printf("\n");
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc > 1 && std::strcmp(argv[1], "update") == 0) return mode_update();
  if (argc > 1 && std::strcmp(argv[1], "propose") == 0) return mode_propose();
  if (argc > 1 && std::strcmp(argv[1], "geometry") == 0) {
    int dim;
    while (std::scanf("%d", &dim) == 1)
      std::printf("%d %d %d %d %d %d\n", prec_blocks(dim), prec_padded(dim), prec_stride(dim), prec_lds_bytes(dim), prec_z_items(dim), prec_l_passes(dim));
    return 0;
  }
  if (argc > 1 && std::strcmp(argv[1], "grid") == 0) {
    long long n_tiles;
    int cus;
    while (std::scanf("%lld %d", &n_tiles, &cus) == 2) std::printf("%lld\n", prec_grid(n_tiles, cus));
    return 0;
  }
  test_grid();
  test_maps_and_replay();
  test_update();
  std::printf("precond ok: %lld checks\n", g_checks);
  return 0;
}
