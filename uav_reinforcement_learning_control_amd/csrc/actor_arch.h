// actor_arch.h -- a deterministic actor 12 -> H1 -> H2 -> 4 of any supported width and activation on MFMA
// (device only): mean = W3 act(W2 act(W1 x + b1) + b2) + b3, H1 a multiple of 32 up to 512, H2 in {64, 128,
// 256}, act ReLU or tanh. The reference's optimize.py family ([128,128], [256,256], [512,256] x relu / tanh)
// and SB3's MlpPolicy default ([64,64] tanh) are members.
//
// Arithmetic, loop order and pipeline: actor_core.h's forward with one layer-1 k-step (12 features of 16), a
// head of 4 and the activation family {ReLU, tanh}. This header adds the family's layout and its input convention.
// W1 pieces, biases and head weights are staged in LDS (56.3 KB at H1 = 512); the pre-split W2 pieces stream
// from global memory / L2, two k-steps ahead of their use.
//
// Packed image (floats; quad_actor_pack writes it, quad_actor_packed_floats sizes it; lane maps and acc_row:
// actor_core.h):
//   B1 : [NB1][2 half][16 reg]             b1[32 n + acc_row(reg, half)]
//   B2 : [MB][2 half][16 reg]              b2[32 m + acc_row(reg, half)]
//   W3 : [MB][16 reg][2 half][4 out]       W3[out][32 m + acc_row(reg, half)]
//   B3 : [4]
//   W1P: [NB1 n][3 piece][64 lane] x 16 B  pieces of A[neuron 32 n + r][feature 8 h + j] (features 12..15 zero)
//   ---- the image up to here is staged in LDS (lds_floats) ----
//   W2P: [g][3 piece][64 lane] x 16 B      layer-2 k-step g = (n * 2 + t) * MB + m: pieces of
//                                          A[neuron 32 m + r][input 32 n + acc_row(8 t + j, h)] -- k-step (n, t)
//                                          consumes registers 8t .. 8t + 7 of act(h1) block n
#pragma once

#include "actor_core.h"

namespace quadenv {
namespace arch {

using Layout = actor::Layout<1, ACT, 0>;  // one layer-1 k-step, four outputs, nothing between B3 and W1P

// The forward of the wave's tile, all 64 lanes: xq[k] = x[env lane & 31][feature 8 (lane >> 5) + k] (zero past
// feature 11; fragments<1>), out = the four means of env lane & 31 (both lane halves get them).
// L: the staged image (Layout{net.nb1, MB}); packed: the global image (the W2 pieces are read from it).
template <int MB>
__device__ __forceinline__ void forward(const float* __restrict__ L, const float* packed, const actor::Net& net,
                                        const float (&xq)[8], float (&out)[ACT]) {
  const Layout lay{net.nb1, MB};
  gbf16x8* wp = actor::lane_pieces(packed + lay.w2p());
  const P3 xp = split8(xq);
  actor::forward<MB, 2>(L, lay, net.actfn, xp, xp, wp, wp, out);
}

}  // namespace arch
}  // namespace quadenv
