// brax_learner.h -- definitions shared by the kernels and the host entry of the Brax learner's minibatch gradient
// (brax_learner.hip, quad_brax_ppo_grad): the per-block partial image, the workspace and the block split.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/quadenv.h"

namespace quadenv {
namespace braxl {

constexpr int HB = 128;        // both hidden layers of both nets: the family of quad_brax_ppo_grad
constexpr int OBSB = QUAD_OBS_BRAX, NLOG = 8;
constexpr int LB = 256;        // threads per block: 4 waves, wave w owns neurons 32w .. 32w + 31
constexpr int RND = 64;        // rows per round (two 32-row MFMA tiles)
constexpr int MAX_NB = 128;    // gradient blocks per net: 2 x 128 = one block per CU
constexpr int MAX_L = 64;
constexpr int GAE_BLOCKS = 256;  // upper bound of the GAE launch's grid = slots of the advantage sums
constexpr uint32_t ENTROPY_STREAM = 0x500u;  // Philox stream of the entropy sample (0x100 .. 0x400 are taken)

// per-block partial image of one net (floats), every tensor in flax's [in, out] layout, so the reduction copies
// ranges: W1 [21][128], b1, W2 [128][128], b2, W3 [128][NOUT], b3 [NOUT], then the block's loss sums
constexpr int P_W1 = 0, P_B1 = P_W1 + OBSB * HB, P_W2 = P_B1 + HB, P_B2 = P_W2 + HB * HB, P_W3 = P_B2 + HB;
constexpr int P_B3 = P_W3 + HB * NLOG, P_STATS = P_B3 + NLOG;  // 0: sum min(s1, s2); 1: sum (vs - v)^2; 2: sum entropy
constexpr int PSTRIDE = P_STATS + 8;
static_assert(PSTRIDE % 4 == 0, "16-byte partial images");

struct Net {
  const float *w0, *b0, *w1, *b1, *w2, *b2;
};

struct Layout {
  int32_t rows_loss, rows_all;  // L * mb, (L + 1) * mb
  int32_t nb, rpb;              // gradient blocks per net, rounds per block
  int32_t nbv;                  // value-forward blocks (one round each)
  int32_t gae_blocks;
  int64_t o_values, o_vs, o_adv, o_adv_part, o_part, bytes;  // workspace offsets (bytes)
};

inline int64_t up16(int64_t x) { return (x + 15) & ~int64_t(15); }

inline Layout layout_of(int32_t mb, int32_t L) {
  Layout l{};
  l.rows_loss = L * mb;
  l.rows_all = (L + 1) * mb;
  const int rounds = (l.rows_loss + RND - 1) / RND;
  const int nb0 = rounds < MAX_NB ? rounds : MAX_NB;
  l.rpb = (rounds + nb0 - 1) / nb0;
  l.nb = (rounds + l.rpb - 1) / l.rpb;
  l.nbv = (l.rows_all + RND - 1) / RND;
  const int gb = (mb + 255) / 256;
  l.gae_blocks = gb < GAE_BLOCKS ? gb : GAE_BLOCKS;
  l.o_values = 0;
  l.o_vs = up16(int64_t(l.rows_all) * 4);
  l.o_adv = l.o_vs + up16(int64_t(l.rows_loss) * 4);
  l.o_adv_part = l.o_adv + up16(int64_t(l.rows_loss) * 4);
  l.o_part = l.o_adv_part + int64_t(GAE_BLOCKS) * 2 * 8;
  l.bytes = l.o_part + int64_t(2) * l.nb * PSTRIDE * 4;
  return l;
}

// what the four kernels read (by value)
struct Args {
  Net pi, vf;
  const float *mean, *std;
  const float *obs, *next_obs, *raw, *logp, *reward, *discount, *trunc;
  const int64_t* idx;
  const float* noise;
  float *noise_out, *d_values, *d_vs, *d_adv;  // optional outputs
  float *values, *vs, *adv;                    // workspace
  double* adv_part;
  float* part;
  int32_t U, L, N, mb, rows_loss, rows_all, nb, rpb, gae_blocks, norm_adv;
  float min_std, clip, ent_cost, gamma, lam, rscale, inv_rows;
  uint32_t noise_step;
  uint64_t seed;
};

struct RArgs {
  QuadBraxPPOGrads gr;
  const float* part;
  float* stats;
  int32_t nb;
  double inv_rows, ent_cost;
};

}  // namespace braxl
}  // namespace quadenv
