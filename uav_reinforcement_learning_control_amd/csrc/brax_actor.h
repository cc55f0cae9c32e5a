// brax_actor.h -- the Brax-profile policy network 21 -> H1 -> H2 -> 8 on MFMA (device only; the host
// entries of its launches are brax_episode.h's): ppo/brax_ppo.py BraxActorCritic.policy with two hidden layers,
//   logits = W3 act(W2 act(W1 xh + b1) + b2) + b3,   xh = (obs21 - mean) / std  (f32, correctly rounded division:
//   RunningStats.normalize's expression, so xh has torch's bits),
// H1 a multiple of 32 up to 512, H2 in {64, 128, 256}, act ReLU, tanh or SiLU; loc = logits[0:4],
// scale = softplus(logits[4:8]) + min_std (NormalTanh.split).
//
// Arithmetic: actor_arch.h's, exactly -- three-piece bf16 splits of both operands, the six piece products small
// terms first (mfma6), f32 accumulators initialised with the bias, the head in f32 FMAs over the neurons in
// accumulator order, the lane halves summed through permlane32_swap. One wave per 32-env tile (lanes l and l + 32
// carry env l & 31), the outer loop over the NB1 = H1 / 32 layer-1 blocks a runtime loop, MB = H2 / 32 a
// compile-time constant, the activation a wave-uniform branch.
//
// New against arch::forward<MB>:
//   * layer 1 has K = 32: two k-steps per block, features 0-15 and 16-31 (21-31 zero). Lane half h holds features
//     8h + j of k-step 0 and 16 + 8h + j of k-step 1, so the upper half's k-step-1 operand is all zeros.
//   * the head has 8 outputs (two float4 weight rows per hidden value).
//   * SiLU and softplus, branch-free (below).
//   * the normaliser: mean and std ride in the image, padded to 32 with (0, 1): a padding feature is 0 / 1 = 0.
//
// LDS: the k-step-0 W1 pieces, biases, head weights and the normaliser are staged (59.3 KB at H1 = 512, under the
// 64 KB that needs no opt-in). The k-step-1 W1 pieces (another 48 KB at H1 = 512) stream from global memory / L2
// like the W2 pieces, one layer-1 block ahead of their use.
//
// Packed image (floats; acc_row, lane maps: policy_net.h / actor_arch.h):
//   B1  : [NB1][2 half][16 reg]              b1[32 n + acc_row(reg, half)]
//   B2  : [MB][2 half][16 reg]
//   W3  : [MB][16 reg][2 half][8 out]        W3[32 m + acc_row(reg, half)][out]      (flax [in, out] source)
//   B3  : [8]
//   MEAN: [32]   STD: [32]                   padded with 0 / 1
//   MISC: [4]                                min_std, 0, 0, 0
//   W1P : [NB1 n][3 piece][64 lane] x 16 B   pieces of A[neuron 32 n + r][feature 8 h + j]
//   ---- the image up to here is staged in LDS ----
//   W1Q : [NB1 n][3 piece][64 lane] x 16 B   pieces of A[neuron 32 n + r][feature 16 + 8 h + j] (zero past 20)
//   W2P : [g][3 piece][64 lane] x 16 B       layer-2 k-step g = (n * 2 + t) * MB + m, actor_arch.h's
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/quadenv.h"
#include "actor_arch.h"
#include "brax_episode.h"
#include "env_tiles.h"
#include "policy_net.h"

namespace quadenv {
namespace brax {

constexpr int OBSB = QUAD_OBS_BRAX;  // 21
constexpr int NLOG = 8;              // logits: loc 4, raw scale 4
constexpr int UNIT_F = arch::UNIT_F;
constexpr uint32_t NOISE_STREAM = 0x400u;

struct Layout {
  int nb1, mb;
  __host__ __device__ constexpr int b1() const { return 0; }
  __host__ __device__ constexpr int b2() const { return 32 * nb1; }
  __host__ __device__ constexpr int w3() const { return b2() + 32 * mb; }
  __host__ __device__ constexpr int b3() const { return w3() + NLOG * 32 * mb; }
  __host__ __device__ constexpr int mean() const { return b3() + NLOG; }
  __host__ __device__ constexpr int stdv() const { return mean() + 32; }
  __host__ __device__ constexpr int misc() const { return stdv() + 32; }
  __host__ __device__ constexpr int w1p() const { return misc() + 4; }
  __host__ __device__ constexpr int lds_floats() const { return w1p() + nb1 * UNIT_F; }
  __host__ __device__ constexpr int w1q() const { return lds_floats(); }
  __host__ __device__ constexpr int w2p() const { return w1q() + nb1 * UNIT_F; }
  __host__ __device__ constexpr int steps() const { return nb1 * 2 * mb; }
  __host__ __device__ constexpr int64_t floats() const { return int64_t(w2p()) + int64_t(steps()) * UNIT_F; }
};
static_assert(Layout{arch::MAX_H1 / 32, 8}.lds_floats() * 4 <= 64 * 1024, "the staged image fits the default LDS limit");
static_assert(Layout{1, 2}.w1p() % 4 == 0 && Layout{1, 2}.lds_floats() % 4 == 0 && Layout{1, 2}.w2p() % 4 == 0,
              "16-byte aligned pieces");

enum { ACT_RELU = QUAD_ACTFN_RELU, ACT_TANH = QUAD_ACTFN_TANH, ACT_SILU = QUAD_ACTFN_SILU };
struct Net {  // what a kernel needs of the arch (wave-uniform)
  int nb1;
  int actfn;
};

// SiLU x sigmoid(x) = x / (1 + exp(-x)) without a branch: libm's expf, one add, the correctly rounded division.
// Largest error against float64 over every f32 in [-87, 88], in ulps of the result (tools/diag/brax_act_ulp.c):
// 2.38 ulp with a correctly rounded expf (at x = -16.68, where 1 + e rounds at e's 2^24 and the quotient sits at the
// bottom of its binade), 4.28 ulp with an expf one ulp off either way, which is what HIP documents for the device's.
// SILU_ULP is the bound the tests use. exp overflow (x < -88.7) gives x / inf = -0; NaN gives NaN.
constexpr float SILU_ULP = 4.5f;
__device__ __forceinline__ float silu_f32(float x) {
  const float e = expf(-x);
  return __fdiv_rn(x, 1.f + e);
}

// softplus log(1 + exp(x)) = max(x, 0) + log1p(exp(-|x|)) without a branch: libm's expf and log1pf. Largest error
// against float64 over every f32 in [-87, 88] (same tool): 1.49 ulp with both calls correctly rounded, 5.26 ulp with
// each one ulp off either way (at x = -2.02, where exp(x) is just above 2^-3 and the result just below it).
// SOFTPLUS_ULP is the bound the tests use. NaN gives NaN; x > 88 gives x.
constexpr float SOFTPLUS_ULP = 5.5f;
__device__ __forceinline__ float softplus_f32(float x) {
  const float t = fabsf(x);
  const float l = log1pf(expf(-t));
  const float m = x > 0.f ? x : 0.f;  // a select; NaN falls to the sum below through l
  return m + l;
}

template <int ACTF>
__device__ __forceinline__ float act1(float x) {
  return ACTF == ACT_TANH ? arch::tanh_f32(x) : (ACTF == ACT_SILU ? silu_f32(x) : relu(x));
}

// act() of one accumulator block as pieces; `actfn` is wave-uniform, so these are scalar branches
__device__ __forceinline__ void act_split(const f32x16& a, int actfn, Q3 (&hq)[2]) {
  float v[16];
  if (actfn == ACT_TANH) {
#pragma unroll
    for (int i = 0; i < 16; i++) v[i] = arch::tanh_f32(a[i]);
  } else if (actfn == ACT_SILU) {
#pragma unroll
    for (int i = 0; i < 16; i++) v[i] = silu_f32(a[i]);
  } else {
#pragma unroll
    for (int i = 0; i < 16; i++) v[i] = relu(a[i]);
  }
#pragma unroll
  for (int t = 0; t < 2; t++)
#pragma unroll
    for (int k = 0; k < 4; k++) split_pair(v[8 * t + 2 * k], v[8 * t + 2 * k + 1], hq[t], k);
}

// the head's partial sums of this lane half: part[q] += W3[neuron][q] act(h2[neuron]) over the half's neurons in
// accumulator order (o3: the lane half's offset into W3)
template <int MB, int ACTF>
__device__ __forceinline__ void head(const float* __restrict__ L, int o3, const f32x16 (&acc)[MB], float (&part)[NLOG]) {
#pragma unroll
  for (int m = 0; m < MB; m++) {
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const float v = act1<ACTF>(acc[m][i]);
      const float4 wa = ld4(L, o3 + (m * 16 + i) * 16), wb = ld4(L, o3 + (m * 16 + i) * 16 + 4);
      part[0] = fmaf(wa.x, v, part[0]);
      part[1] = fmaf(wa.y, v, part[1]);
      part[2] = fmaf(wa.z, v, part[2]);
      part[3] = fmaf(wa.w, v, part[3]);
      part[4] = fmaf(wb.x, v, part[4]);
      part[5] = fmaf(wb.y, v, part[5]);
      part[6] = fmaf(wb.z, v, part[6]);
      part[7] = fmaf(wb.w, v, part[7]);
    }
    __builtin_amdgcn_sched_barrier(0);  // one block's accumulators in VGPRs at a time
  }
}

// this lane's layer-1 operand from its env's raw observation row: xa = features 8 h + j, xb = features
// 16 + 8 h + j, normalised ((x - mean) / std, f32); padding features are (0 - 0) / 1
__device__ __forceinline__ void normalise(const float* __restrict__ L, const Layout& lay, const float (&ob)[OBSB],
                                          float (&xa)[8], float (&xb)[8]) {
  const bool h = (threadIdx.x & 32) != 0;
  const int om = lay.mean() + (h ? 8 : 0), os = lay.stdv() + (h ? 8 : 0);
#pragma unroll
  for (int j = 0; j < 8; j++) {
    // both candidates pinned in registers: left as it is, the select becomes a load of ob[8 h + j] at a per-lane
    // index and the row goes through scratch (96 bytes per lane)
    float lo = ob[j], hi = ob[8 + j];
    asm volatile("" : "+v"(lo), "+v"(hi));
    const float x = h ? hi : lo;
    xa[j] = __fdiv_rn(__fsub_rn(x, L[om + j]), L[os + j]);
  }
#pragma unroll
  for (int j = 0; j < 8; j++) {
    if (j < OBSB - 16) {
      float lo = ob[16 + j];
      asm volatile("" : "+v"(lo));
      const float x = h ? 0.f : lo;
      xb[j] = __fdiv_rn(__fsub_rn(x, L[om + 16 + j]), L[os + 16 + j]);
    } else {
      xb[j] = 0.f;
    }
  }
}

// the k-step-1 W1 fragment of layer-1 block n (wq: this lane's unit of block 0, piece 0)
__device__ __forceinline__ P3 w1q_block(gbf16x8* wq, int n) {
  P3 x;
#pragma unroll
  for (int p = 0; p < 3; p++) x.p[p] = wq[(n * 3 + p) * 64];
  return x;
}

// The forward of the wave's tile, all 64 lanes: ob = the raw observation row of env lane & 31; out = its eight
// logits (both lane halves get them). L: the staged image (Layout{net.nb1, MB}); packed: the global image.
template <int MB>
__device__ __forceinline__ void forward(const float* __restrict__ L, const float* packed, const Net& net,
                                        const float (&ob)[OBSB], float (&out)[NLOG]) {
  const int lane = threadIdx.x & 63, h = lane >> 5;
  const int nb1 = net.nb1;
  const Layout lay{nb1, MB};
  constexpr int S = 2 * MB;  // layer-2 k-steps per layer-1 block
  const int G = nb1 * S;
  // the pieces' scalar bases, opaque per call: the loads stay inside the callers' step loops (policy_net.h)
  uint64_t pb = reinterpret_cast<uint64_t>(packed + lay.w2p()), qb = reinterpret_cast<uint64_t>(packed + lay.w1q());
  asm volatile("" : "+s"(pb), "+s"(qb));
  gbf16x8* wp = reinterpret_cast<gbf16x8*>(pb) + lane;
  gbf16x8* wq = reinterpret_cast<gbf16x8*>(qb) + lane;
  const int obi = lay.b1() + h * 16, ow1 = lay.w1p() + lane * 4;

  float xa[8], xb[8];
  normalise(L, lay, ob, xa, xb);
  const P3 xpa = split8(xa), xpb = split8(xb);
  f32x16 acc[MB];
#pragma unroll
  for (int m = 0; m < MB; m++) bias_init(acc[m], L, lay.b2() + m * 32 + h * 16);
  P3 r0 = arch::w2_step(wp, 0), r1 = arch::w2_step(wp, 1);  // G >= 4
  Q3 hq[2];
  {
    f32x16 b;
    bias_init(b, L, obi);
    b = mfma6(arch::lds_pieces(L, ow1), xpa, b);
    act_split(mfma6(w1q_block(wq, 0), xpb, b), net.actfn, hq);
  }
  for (int n = 0; n < nb1; n++) {
    // layer 1 of the next block first, so its result is there when this block's steps are through
    // (wave-uniform: the last block has no next one)
    const bool more = n + 1 < nb1;
    f32x16 a1n;
    if (more) {
      f32x16 b1n;
      bias_init(b1n, L, obi + (n + 1) * 32);
      b1n = mfma6(arch::lds_pieces(L, ow1 + (n + 1) * UNIT_F), xpa, b1n);
      a1n = mfma6(w1q_block(wq, n + 1), xpb, b1n);
    }
    P3 ring[3];
    ring[0] = r0;
    ring[1] = r1;
#pragma unroll
    for (int s = 0; s < S; s++) {
      const int g2 = n * S + s + 2;  // two steps ahead, into the slot step s - 1 freed; clamped in range
      ring[(s + 2) % 3] = arch::w2_step(wp, g2 < G ? g2 : G - 1);
      acc[s % MB] = mfma6(ring[s % 3], hq[s / MB].p(), acc[s % MB]);
      __builtin_amdgcn_sched_barrier(0);  // one step per scheduling region: at most three fragments in flight
    }
    r0 = ring[S % 3];
    r1 = ring[(S + 1) % 3];
    if (more) act_split(a1n, net.actfn, hq);
  }
  float part[NLOG] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  // one branch around the whole head (actor_arch.h)
  const int o3 = lay.w3() + h * NLOG;
  if (net.actfn == ACT_TANH) head<MB, ACT_TANH>(L, o3, acc, part);
  else if (net.actfn == ACT_SILU) head<MB, ACT_SILU>(L, o3, acc, part);
  else head<MB, ACT_RELU>(L, o3, acc, part);
#pragma unroll
  for (int q = 0; q < NLOG; q++) {
    const auto p = __builtin_amdgcn_permlane32_swap(__float_as_uint(part[q]), __float_as_uint(part[q]), false, false);
    out[q] = (__uint_as_float(p[0]) + __uint_as_float(p[1])) + L[lay.b3() + q];
  }
}

// Box-Muller on Philox(seed; env, step, 0x400) -> 4 standard normals: policy_net.h gauss4's draw on the Brax
// actor's own stream
__device__ __forceinline__ void gauss4_brax(uint64_t seed, uint64_t env, uint32_t step, float z[4]) {
  uint32_t c[4] = {uint32_t(env), uint32_t(env >> 32), step, NOISE_STREAM};
  philox4x32_10(c, uint32_t(seed), uint32_t(seed >> 32));
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const float u1 = (float(c[2 * k] >> 8) + 1.0f) * 0x1p-24f;  // (0, 1]
    const float u2 = float(c[2 * k + 1] >> 8) * 0x1p-24f;
    const float r = __builtin_amdgcn_sqrtf(-1.38629436111989061f * __builtin_amdgcn_logf(u1));  // -2 ln u1
    z[2 * k] = r * __builtin_amdgcn_cosf(u2);
    z[2 * k + 1] = r * __builtin_amdgcn_sinf(u2);
  }
}

// NormalTanh on the logits: tanh(loc) or tanh(loc + scale z), scale = softplus(raw) + min_std; the products and
// sums are separate f32 roundings (no contraction), as torch forms them
__device__ __forceinline__ void env_action(const float (&lg)[NLOG], float min_std, bool deterministic, uint64_t seed,
                                           uint64_t env, uint32_t step, float (&a)[4]) {
  if (deterministic) {
#pragma unroll
    for (int k = 0; k < 4; k++) a[k] = arch::tanh_f32(lg[k]);
    return;
  }
  float z[4];
  gauss4_brax(seed, env, step, z);
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const float sc = __fadd_rn(softplus_f32(lg[4 + k]), min_std);
    a[k] = arch::tanh_f32(__fadd_rn(lg[k], __fmul_rn(sc, z[k])));
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

}  // namespace brax

}  // namespace quadenv
