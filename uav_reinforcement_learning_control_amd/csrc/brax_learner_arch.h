// brax_learner_arch.h -- definitions shared by the kernels and the host entry of the Brax learner's minibatch gradient
// for the Brax actor's whole family (brax_learner_arch.hip, quad_brax_ppo_arch_grad): the family, the workspace
// images of each net, the block and split-K layout.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/quadenv.h"
#include "brax_learner.h"

namespace quadenv {
namespace braxa {

using braxl::NLOG;
using braxl::OBSB;

constexpr int LB = braxl::LB;  // threads per block: 4 waves
constexpr int RND = 32;        // rows per round of the value and the forward launch (one 32-row MFMA tile)
constexpr int CHUNK = 64;      // rows per fresh accumulator of the weight-gradient launch (four k-steps)
constexpr int XW = 32;         // observation image row: 21 normalised features, 1.0, 10 zeros
constexpr int XS = XW + 4;     // its LDS row
constexpr int W1R = OBSB + 1;  // rows of a split's dW1 | db1 image
constexpr int MAX_NBK = 128;   // forward blocks per net: 2 x 128 = one block per CU
constexpr int MAX_NBV = 256;   // value-forward blocks
constexpr int MAX_SPLITS = 64;
constexpr int WAVE_TARGET = 2048;         // weight-gradient waves wanted over both nets: two per SIMD
constexpr int32_t MAX_ROWS = 1 << 22;     // loss rows L * mb: every image index below stays under 2^31 * 4 as int64 /
                                          // size_t, every row index and (L + 1) * mb <= 2^23 in int32
constexpr int MAX_H1 = 512, MAX_H2 = 256;

inline bool net_in_family(int h1, int h2) {
  return h1 >= 32 && h1 <= MAX_H1 && h1 % 32 == 0 && (h2 == 64 || h2 == 128 || h2 == 256);
}
inline bool in_family(const QuadBraxPPOParams* p) {
  return p && net_in_family(p->policy_h1, p->policy_h2) && net_in_family(p->value_h1, p->value_h2) &&
         (p->activation == QUAD_ACTFN_RELU || p->activation == QUAD_ACTFN_TANH || p->activation == QUAD_ACTFN_SILU);
}
inline bool in_limits(int32_t mb, int32_t L) {
  return mb >= 1 && L >= 1 && L <= braxl::MAX_L && int64_t(L) * mb <= MAX_ROWS;
}

// per-block sums of the forward launch (floats): b2 [h2], W3 [h2][8] (flax's [in, out]; the value net uses column 0),
// b3 [8], then sum min(s1, s2), sum (vs - v)^2, sum entropy, pad
__host__ __device__ constexpr int sp_w3(int h2) { return h2; }
__host__ __device__ constexpr int sp_b3(int h2) { return 9 * h2; }
__host__ __device__ constexpr int sp_st(int h2) { return 9 * h2 + 8; }
__host__ __device__ constexpr int sp_stride(int h2) { return 9 * h2 + 12; }
// per-split image of the weight-gradient launch (floats), both in flax's layout: dW2 [h1][h2], then [22][h1]: dW1 in
// rows 0 .. 20, db1 in row 21
__host__ __device__ constexpr int pb_stride(int h1, int h2) { return h1 * h2 + W1R * h1; }
// LDS of a forward block (floats): X [32][36], H1 [32][h1 + 4], H2 and DH2 [32][h2 + 4], LOGIT and D [32][8],
// W3 [h2][8], mean | std [64], double [2][256]
__host__ __device__ constexpr int lds_floats(int h1, int h2) {
  return RND * XS + RND * (h1 + 4) + 2 * RND * (h2 + 4) + 2 * RND * 8 + 8 * h2 + 64 + 4 * LB;
}
constexpr int LDS_MAX_BYTES = lds_floats(MAX_H1, MAX_H2) * 4;  // 151,808 B: what every launch asks for
static_assert(LDS_MAX_BYTES <= 160 * 1024, "LDS budget");
// the end-of-launch sums ([256][9] floats, then double [32][12]) alias the H2 and DH2 images of the narrowest net
static_assert(LB * 9 + RND * 12 * 2 <= 2 * RND * (64 + 4), "block sums fit the narrowest H2 | DH2 images");

inline int64_t up16(int64_t x) { return (x + 15) & ~int64_t(15); }

struct NetLayout {
  int32_t h1, h2;
  int32_t tiles;        // 32 x 32 output tiles: dW2's, then dW1 | db1's
  int32_t splits, rps;  // split-K: row ranges of rps rows (a multiple of CHUNK)
  int32_t lds_bytes;    // what this net's forward block uses
  int64_t o_h1, o_dh2, o_dh1, o_sp, o_pb;  // workspace offsets (bytes) of its [bp][width] images and its sums
};

struct Layout {
  int32_t rows_loss, rows_all;
  int32_t bp;           // loss rows rounded up to CHUNK: the rows of every workspace image
  int32_t nbk, rpb;     // forward blocks per net, rounds per block
  int32_t nbv, rpbv;    // value-forward blocks, rounds per block
  int32_t gae_blocks;
  NetLayout net[2];     // policy, value
  int64_t o_values, o_vs, o_adv, o_adv_part, o_x, bytes;
};

inline Layout layout_of(int p1, int p2, int v1, int v2, int32_t mb, int32_t L) {
  Layout l{};
  l.rows_loss = L * mb;
  l.rows_all = (L + 1) * mb;
  l.bp = (l.rows_loss + CHUNK - 1) / CHUNK * CHUNK;
  const int rounds = l.bp / RND;
  const int nb0 = rounds < MAX_NBK ? rounds : MAX_NBK;
  l.rpb = (rounds + nb0 - 1) / nb0;
  l.nbk = (rounds + l.rpb - 1) / l.rpb;
  const int rv = (l.rows_all + RND - 1) / RND;
  const int nv0 = rv < MAX_NBV ? rv : MAX_NBV;
  l.rpbv = (rv + nv0 - 1) / nv0;
  l.nbv = (rv + l.rpbv - 1) / l.rpbv;
  const int gb = (mb + 255) / 256;
  l.gae_blocks = gb < braxl::GAE_BLOCKS ? gb : braxl::GAE_BLOCKS;
  const int64_t bp = l.bp;
  l.o_values = 0;
  l.o_vs = up16(int64_t(l.rows_all) * 4);
  l.o_adv = l.o_vs + up16(int64_t(l.rows_loss) * 4);
  l.o_adv_part = l.o_adv + up16(int64_t(l.rows_loss) * 4);
  l.o_x = l.o_adv_part + int64_t(braxl::GAE_BLOCKS) * 2 * 8;
  int64_t o = l.o_x + bp * XW * 4;
  const int hs[2][2] = {{p1, p2}, {v1, v2}};
  const int chunks = l.bp / CHUNK;
  const int tiles_all = (p1 / 32) * (p2 / 32) + p1 / 32 + (v1 / 32) * (v2 / 32) + v1 / 32;
  for (int n = 0; n < 2; n++) {
    NetLayout& nl = l.net[n];
    nl.h1 = hs[n][0];
    nl.h2 = hs[n][1];
    nl.tiles = (nl.h1 / 32) * (nl.h2 / 32) + nl.h1 / 32;
    int s = WAVE_TARGET / tiles_all;
    s = s < 1 ? 1 : (s > MAX_SPLITS ? MAX_SPLITS : s);
    if (s > chunks) s = chunks;
    nl.rps = (chunks + s - 1) / s * CHUNK;
    nl.splits = (l.bp + nl.rps - 1) / nl.rps;
    nl.lds_bytes = lds_floats(nl.h1, nl.h2) * 4;
    nl.o_h1 = o;
    nl.o_dh2 = nl.o_h1 + bp * nl.h1 * 4;
    nl.o_dh1 = nl.o_dh2 + bp * nl.h2 * 4;
    nl.o_sp = nl.o_dh1 + bp * nl.h1 * 4;
    nl.o_pb = nl.o_sp + up16(int64_t(l.nbk) * sp_stride(nl.h2) * 4);
    o = nl.o_pb + up16(int64_t(nl.splits) * pb_stride(nl.h1, nl.h2) * 4);
  }
  l.bytes = o;
  return l;
}

// one net's side of the launches
struct NetArgs {
  float *h1, *dh2, *dh1;  // workspace images [bp][width]
  float *sp, *pb;         // forward-block sums, split-K images
  int32_t h1w, h2w, tiles, splits, rps;
};

// what the launches read (by value). g carries what brax_learner_common.h's pieces and k_brax_gae read: the nets, the
// normaliser, the unroll buffers, the index, the values / vs / advantages arrays and the loss constants
struct Args {
  braxl::Args g;
  QuadBraxPPOGrads gr;
  float* stats;
  float* x;  // workspace image [bp][32], written by the policy's blocks
  NetArgs net[2];
  int32_t bp, nbk, rpb, nbv, rpbv;
  double inv_rows, ent_cost;
};

}  // namespace braxa
}  // namespace quadenv
