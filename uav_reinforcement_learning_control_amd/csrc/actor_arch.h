// actor_arch.h -- a deterministic actor 12 -> H1 -> H2 -> 4 of any supported width and activation on MFMA
// (device only): mean = W3 act(W2 act(W1 x + b1) + b2) + b3, H1 a multiple of 32 up to 512, H2 in {64, 128,
// 256}, act ReLU or tanh. The reference's optimize.py family ([128,128], [256,256], [512,256] x relu / tanh)
// and SB3's MlpPolicy default ([64,64] tanh) are members.
//
// Arithmetic: policy_net.h's, exactly -- v_mfma_f32_32x32x16_bf16 over three-piece round-to-nearest bf16
// splits of both operands (split8 / split_pair), the six piece products in mfma6's order, f32 accumulators
// initialised with the bias, the head in f32 FMAs over the neurons in accumulator order, the two lane halves
// summed through permlane32_swap. tanh is tanh_f32 below (branch-free, <= 2 ulp).
//
// One wave per 32-env tile (policy_net.h's NT = 1: lanes l and l + 32 carry env l & 31). Loop order, net_core's:
// the outer loop over the NB1 = H1 / 32 layer-1 blocks is a RUNTIME loop; block n makes act(h1) block n as
// pieces, and its two k-steps go into all MB = H2 / 32 layer-2 accumulators at once. Only two blocks of h1
// pieces are ever live (block n's, and block n + 1's whose layer-1 MFMAs issue before block n's steps); the
// accumulators are MB x 16 <= 128 registers. Only MB is a compile-time constant; the activation is a
// wave-uniform branch around each block of 16 values. Activations never go through LDS.
// W1 pieces, biases and head weights are staged in LDS (56.3 KB at H1 = 512); the pre-split W2 pieces stream
// from global memory / L2 (768 KB at [512, 256], shared by every wave), two k-steps ahead of their use.
//
// Packed image (floats; quad_actor_pack writes it, quad_actor_packed_floats sizes it). Operand element j of
// lane l (r = l & 31, h = l >> 5) is k = 8h + j of the 32x32x16 MFMA; acc_row(reg, h) is the neuron a lane
// half's accumulator register holds (policy_net.h):
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

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "policy_net.h"

namespace quadenv {
namespace arch {

constexpr int MAX_H1 = 512;
constexpr int UNIT_F = 3 * 64 * 4;  // one three-piece fragment: [3 piece][64 lane] x 16 bytes, in floats

struct Layout {
  int nb1, mb;
  __host__ __device__ constexpr int b1() const { return 0; }
  __host__ __device__ constexpr int b2() const { return 32 * nb1; }
  __host__ __device__ constexpr int w3() const { return b2() + 32 * mb; }
  __host__ __device__ constexpr int b3() const { return w3() + ACT * 32 * mb; }
  __host__ __device__ constexpr int w1p() const { return b3() + 4; }
  __host__ __device__ constexpr int lds_floats() const { return w1p() + nb1 * UNIT_F; }
  __host__ __device__ constexpr int w2p() const { return lds_floats(); }
  __host__ __device__ constexpr int steps() const { return nb1 * 2 * mb; }  // layer-2 k-steps
  __host__ __device__ constexpr int64_t floats() const { return int64_t(w2p()) + int64_t(steps()) * UNIT_F; }
};
static_assert(Layout{MAX_H1 / 32, 8}.lds_floats() * 4 <= 64 * 1024, "the staged image fits the default LDS limit");
static_assert(Layout{1, 2}.w1p() % 4 == 0 && Layout{1, 2}.lds_floats() % 4 == 0, "16-byte aligned pieces");

// what a kernel needs of the arch: the layer-1 block count and the activation (wave-uniform)
struct Net {
  int nb1;
  int tanh_act;
};

// tanh without a per-lane branch. Device libm's tanhf takes one per value; with 160 inlined copies of it the
// register allocator put the layer-2 accumulators in VGPRs across the head's basic blocks and the MB = 8 form
// spilled 1,108 bytes per lane. |x| < 0.625: x + x z P(z), z = x^2, P the degree-5 least-squares fit of
// (tanh(x) / x - 1) / z over [0, 0.625^2] (0.7 ulp in f32); otherwise 1 - 2 / (exp(2|x|) + 1) with libm's expf
// and the correctly rounded division (1.3 ulp: the quotient is below 0.45 where the result is above 0.55).
// exp overflow gives 1, NaN gives NaN.
__device__ __forceinline__ float tanh_f32(float x) {
  const float t = fabsf(x), z = t * t;
  float p = 0.002142803743481636f;
  p = fmaf(p, z, -0.008177093230187893f);
  p = fmaf(p, z, 0.021700501441955566f);
  p = fmaf(p, z, -0.05394670367240906f);
  p = fmaf(p, z, 0.1333320587873459f);
  p = fmaf(p, z, -0.3333333134651184f);
  const float tz = t * z;
  const float small = fmaf(tz, p, t);
  const float e = expf(2.f * t);
  const float q = 2.f / (e + 1.f);
  const float big = 1.f - q;
  return copysignf(t < 0.625f ? small : big, x);
}

// act() of one accumulator block; `tanh_act` is wave-uniform, so this is a scalar branch
__device__ __forceinline__ void activate16(const f32x16& a, int tanh_act, float (&v)[16]) {
  if (tanh_act) {
#pragma unroll
    for (int i = 0; i < 16; i++) v[i] = tanh_f32(a[i]);
  } else {
#pragma unroll
    for (int i = 0; i < 16; i++) v[i] = relu(a[i]);
  }
}

__device__ __forceinline__ void act_split(const f32x16& a, int tanh_act, Q3 (&hq)[2]) {
  float v[16];
  activate16(a, tanh_act, v);
#pragma unroll
  for (int t = 0; t < 2; t++)
#pragma unroll
    for (int k = 0; k < 4; k++) split_pair(v[8 * t + 2 * k], v[8 * t + 2 * k + 1], hq[t], k);
}

__device__ __forceinline__ P3 lds_pieces(const float* L, int off) {
  P3 x;
#pragma unroll
  for (int p = 0; p < 3; p++) x.p[p] = *reinterpret_cast<const bf16x8*>(L + off + p * 256);
  return x;
}

// the W2 fragment of layer-2 k-step g (wp: this lane's unit of step 0, piece 0)
__device__ __forceinline__ P3 w2_step(gbf16x8* wp, int g) {
  P3 x;
#pragma unroll
  for (int p = 0; p < 3; p++) x.p[p] = wp[(g * 3 + p) * 64];
  return x;
}

// the head's partial sums of this lane half: part[q] += W3[q][neuron] act(h2[neuron]) over the half's neurons in
// accumulator order (o3: the lane half's offset into W3)
template <int MB, bool TANH>
__device__ __forceinline__ void head(const float* __restrict__ L, int o3, const f32x16 (&acc)[MB], float (&part)[ACT]) {
#pragma unroll
  for (int m = 0; m < MB; m++) {
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const float v = TANH ? tanh_f32(acc[m][i]) : relu(acc[m][i]);
      const float4 w = ld4(L, o3 + (m * 16 + i) * 8);
      part[0] = fmaf(w.x, v, part[0]);
      part[1] = fmaf(w.y, v, part[1]);
      part[2] = fmaf(w.z, v, part[2]);
      part[3] = fmaf(w.w, v, part[3]);
    }
    __builtin_amdgcn_sched_barrier(0);  // one block's accumulators in VGPRs at a time
  }
}

// The forward of the wave's tile, all 64 lanes: xq[k] = x[env lane & 31][feature 8 (lane >> 5) + k] (zero past
// feature 11; fragments<1>), out = the four means of env lane & 31 (both lane halves get them).
// L: the staged image (Layout{net.nb1, MB}); packed: the global image (the W2 pieces are read from it).
template <int MB>
__device__ __forceinline__ void forward(const float* __restrict__ L, const float* packed, const Net& net,
                                        const float (&xq)[8], float (&out)[ACT]) {
  const int lane = threadIdx.x & 63, h = lane >> 5;
  const int nb1 = net.nb1;
  const Layout lay{nb1, MB};
  constexpr int S = 2 * MB;   // layer-2 k-steps per layer-1 block
  const int G = nb1 * S;
  // the pieces' scalar base, opaque per call: the loads stay inside the callers' step loops (policy_net.h)
  uint64_t pb = reinterpret_cast<uint64_t>(packed + lay.w2p());
  asm volatile("" : "+s"(pb));
  gbf16x8* wp = reinterpret_cast<gbf16x8*>(pb) + lane;
  const int ob = lay.b1() + h * 16, ow1 = lay.w1p() + lane * 4;

  const P3 xp = split8(xq);
  f32x16 acc[MB];
#pragma unroll
  for (int m = 0; m < MB; m++) bias_init(acc[m], L, lay.b2() + m * 32 + h * 16);
  P3 r0 = w2_step(wp, 0), r1 = w2_step(wp, 1);  // G >= 4
  Q3 hq[2];
  {
    f32x16 b;
    bias_init(b, L, ob);
    act_split(mfma6(lds_pieces(L, ow1), xp, b), net.tanh_act, hq);
  }
  for (int n = 0; n < nb1; n++) {
    // layer 1 of the next block first, so its result is there when this block's steps are through
    // (wave-uniform: the last block has no next one)
    const bool more = n + 1 < nb1;
    f32x16 a1n;
    if (more) {
      f32x16 b1n;
      bias_init(b1n, L, ob + (n + 1) * 32);
      a1n = mfma6(lds_pieces(L, ow1 + (n + 1) * UNIT_F), xp, b1n);
    }
    P3 ring[3];
    ring[0] = r0;
    ring[1] = r1;
#pragma unroll
    for (int s = 0; s < S; s++) {
      const int g2 = n * S + s + 2;  // two steps ahead, into the slot step s - 1 freed; clamped in range
      ring[(s + 2) % 3] = w2_step(wp, g2 < G ? g2 : G - 1);
      acc[s % MB] = mfma6(ring[s % 3], hq[s / MB].p(), acc[s % MB]);
      __builtin_amdgcn_sched_barrier(0);  // one step per scheduling region: at most three fragments in flight
    }
    r0 = ring[S % 3];
    r1 = ring[(S + 1) % 3];
    if (more) act_split(a1n, net.tanh_act, hq);
  }
  float part[ACT] = {0.f, 0.f, 0.f, 0.f};
  // one branch around the whole head, not one per block: each form is straight-line code that reads an
  // accumulator block out of the AGPRs when its turn comes (a branch per block put all 128 values in VGPRs)
  if (net.tanh_act) head<MB, true>(L, lay.w3() + h * 4, acc, part);
  else head<MB, false>(L, lay.w3() + h * 4, acc, part);
  // lower half's partial + upper half's, in every lane (policy_net.h net_core)
#pragma unroll
  for (int q = 0; q < ACT; q++) {
    const auto p = __builtin_amdgcn_permlane32_swap(__float_as_uint(part[q]), __float_as_uint(part[q]), false, false);
    out[q] = (__uint_as_float(p[0]) + __uint_as_float(p[1])) + L[lay.b3() + q];
  }
}

// the image's LDS part, global -> LDS, by the whole block; ends with a barrier
template <int BLK>
__device__ __forceinline__ void stage(float* lds, const float* __restrict__ packed, const Layout& lay) {
  const int nv = lay.lds_floats() / 4;
  const float4* src = reinterpret_cast<const float4*>(packed);
  float4* dst = reinterpret_cast<float4*>(lds);
  for (int k = threadIdx.x; k < nv; k += BLK) dst[k] = src[k];
  __syncthreads();
}

}  // namespace arch
}  // namespace quadenv
