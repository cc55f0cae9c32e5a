// learner_arch.h -- definitions shared by the kernels and the host entry of the general learner's minibatch gradient
// (learner_arch.hip, quad_ppo_arch_grad): the family, the workspace images, the block and split-K layout.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/quadenv.h"
#include "learner.h"

namespace quadenv {
namespace lrna {

constexpr int LB = 256;        // threads per block: 4 waves
constexpr int RND = 32;        // rows per round of the forward launch (one 32-row MFMA tile)
constexpr int CHUNK = 64;      // rows per fresh accumulator of the weight-gradient launch (four k-steps)
constexpr int XW = 16;         // observation image row: 12 features, 1.0, 3 zeros
constexpr int MAX_NBK = 128;   // forward blocks per net: 2 x 128 = one block per CU
constexpr int MAX_SPLITS = 64;
constexpr int WAVE_TARGET = 2048;  // weight-gradient waves wanted: two per SIMD
constexpr int32_t MAX_BATCH = 1 << 22;

inline bool in_family(const QuadActorArch* a) {
  return a && a->h1 >= 32 && a->h1 <= 512 && a->h1 % 32 == 0 && (a->h2 == 64 || a->h2 == 128 || a->h2 == 256) &&
         (a->activation == QUAD_ACTFN_RELU || a->activation == QUAD_ACTFN_TANH);
}

// per-block sums of the forward launch (floats): b2 [h2], W3 [4][h2] (torch's [out, in]; the critic uses row 0),
// b3 [4], log_std [4], then pg sum, vf sum, clipped count, pad
__host__ __device__ constexpr int sp_w3(int h2) { return h2; }
__host__ __device__ constexpr int sp_b3(int h2) { return 5 * h2; }
__host__ __device__ constexpr int sp_ls(int h2) { return 5 * h2 + 4; }
__host__ __device__ constexpr int sp_st(int h2) { return 5 * h2 + 8; }
__host__ __device__ constexpr int sp_stride(int h2) { return 5 * h2 + 12; }
// per-split image of the weight-gradient launch (floats): dW2 [h2][h1], then [h1][16]: dW1 in columns 0 .. 11, db1 in 12
__host__ __device__ constexpr int pb_stride(int h1, int h2) { return h2 * h1 + h1 * XW; }

inline int64_t up16(int64_t x) { return (x + 15) & ~int64_t(15); }

struct Layout {
  int32_t bp;             // batch rounded up to CHUNK: the rows of every workspace image
  int32_t nbk, rpb;       // forward blocks per net, rounds per block
  int32_t tiles;          // 32 x 32 output tiles per net: dW2's, then dW1's
  int32_t splits, rps;    // split-K: row ranges of rps rows (a multiple of CHUNK)
  int32_t lds_bytes;      // what this arch's forward block uses (the launch asks for the widest member's)
  // workspace offsets (bytes); the per-net images are [2 nets][bp][width]
  int64_t o_adv, o_x, o_h1, o_dh2, o_dh1, o_sp, o_pb, bytes;
};

inline Layout layout_of(int h1, int h2, int32_t batch) {
  Layout l{};
  l.bp = (batch + CHUNK - 1) / CHUNK * CHUNK;
  const int rounds = l.bp / RND;
  const int nb0 = rounds < MAX_NBK ? rounds : MAX_NBK;
  l.rpb = (rounds + nb0 - 1) / nb0;
  l.nbk = (rounds + l.rpb - 1) / l.rpb;
  l.tiles = (h2 / 32) * (h1 / 32) + h1 / 32;
  int s = WAVE_TARGET / (2 * l.tiles);
  s = s < 1 ? 1 : (s > MAX_SPLITS ? MAX_SPLITS : s);
  const int chunks = l.bp / CHUNK;
  if (s > chunks) s = chunks;
  l.rps = (chunks + s - 1) / s * CHUNK;
  l.splits = (l.bp + l.rps - 1) / l.rps;
  // LDS of the forward launch (floats): X [32][20], H1 [32][h1 + 4], H2 and DH2 [32][h2 + 4], LOGIT and D [32][4],
  // W3 [4][h2], double [2][256]
  l.lds_bytes = (RND * 20 + RND * (h1 + 4) + 2 * RND * (h2 + 4) + 2 * RND * 4 + 4 * h2 + 4 * LB) * 4;
  const int64_t bp = l.bp;
  l.o_adv = 0;
  l.o_x = int64_t(lrn::ADV_BLOCKS) * 2 * 8;
  l.o_h1 = l.o_x + bp * XW * 4;
  l.o_dh2 = l.o_h1 + 2 * bp * h1 * 4;
  l.o_dh1 = l.o_dh2 + 2 * bp * h2 * 4;
  l.o_sp = l.o_dh1 + 2 * bp * h1 * 4;
  l.o_pb = l.o_sp + up16(int64_t(2) * l.nbk * sp_stride(h2) * 4);
  l.bytes = l.o_pb + up16(int64_t(2) * l.splits * pb_stride(h1, h2) * 4);
  return l;
}

// what the three launches read (by value). g carries what learner.h's row_terms and adv_norm read: the minibatch
// buffers, the advantage sums, batch, clip, inv_batch, vf_coef; its two NetW are the nets
struct Args {
  lrn::GArgs g;
  QuadPolicyGrads gr;
  float* stats;
  float *x, *h1, *dh2, *dh1;  // workspace images
  float *sp, *pb;             // forward-block sums, split-K images
  int32_t h1w, h2w, bp, nbk, rpb, tiles, splits, rps;
  float ent_coef;
};

}  // namespace lrna
}  // namespace quadenv
