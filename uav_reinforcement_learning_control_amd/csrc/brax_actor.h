// brax_actor.h -- the Brax-profile policy network 21 -> H1 -> H2 -> 8 on MFMA (device only; the host
// entries of its launches are brax_episode.h's): ppo/brax_ppo.py BraxActorCritic.policy with two hidden layers,
//   logits = W3 act(W2 act(W1 xh + b1) + b2) + b3,   xh = (obs21 - mean) / std  (f32, correctly rounded division:
//   RunningStats.normalize's expression, so xh has torch's bits),
// H1 a multiple of 32 up to 512, H2 in {64, 128, 256}, act ReLU, tanh or SiLU; loc = logits[0:4],
// scale = softplus(logits[4:8]) + min_std (NormalTanh.split).
//
// Arithmetic, loop order and pipeline: actor_core.h's forward with two layer-1 k-steps, a head of 8 and the
// activation family {ReLU, tanh, SiLU}. This header adds:
//   * the layout. Layer 1 has K = 32: two k-steps per block, features 0-15 and 16-31 (21-31 zero). Lane half h holds
//     features 8h + j of k-step 0 and 16 + 8h + j of k-step 1, so the upper half's k-step-1 operand is all zeros.
//   * the normaliser: mean and std ride in the image, padded to 32 with (0, 1): a padding feature is 0 / 1 = 0.
//   * softplus (branch-free, below), the error bounds of SiLU and softplus, and the NormalTanh action draw.
//
// LDS: the k-step-0 W1 pieces, biases, head weights and the normaliser are staged (59.3 KB at H1 = 512, under the
// 64 KB that needs no opt-in). The k-step-1 W1 pieces (another 48 KB at H1 = 512) stream from global memory / L2
// like the W2 pieces, one layer-1 block ahead of their use.
//
// Packed image (floats; acc_row, lane maps: actor_core.h):
//   B1  : [NB1][2 half][16 reg]              b1[32 n + acc_row(reg, half)]
//   B2  : [MB][2 half][16 reg]
//   W3  : [MB][16 reg][2 half][8 out]        W3[32 m + acc_row(reg, half)][out]      (flax [in, out] source)
//   B3  : [8]
//   MEAN: [32]   STD: [32]                   padded with 0 / 1
//   MISC: [4]                                min_std, 0, 0, 0
//   W1P : [NB1 n][3 piece][64 lane] x 16 B   pieces of A[neuron 32 n + r][feature 8 h + j]
//   ---- the image up to here is staged in LDS ----
//   W1Q : [NB1 n][3 piece][64 lane] x 16 B   pieces of A[neuron 32 n + r][feature 16 + 8 h + j] (zero past 20)
//   W2P : [g][3 piece][64 lane] x 16 B       layer-2 k-step g = (n * 2 + t) * MB + m, actor_core.h's
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/quadenv.h"
#include "actor_core.h"
#include "brax_episode.h"
#include "env_tiles.h"
#include "policy_net.h"

namespace quadenv {
namespace brax {

constexpr int OBSB = QUAD_OBS_BRAX;  // 21
constexpr int NLOG = 8;              // logits: loc 4, raw scale 4
constexpr uint32_t NOISE_STREAM = 0x400u;

// two layer-1 k-steps, eight outputs, and MEAN | STD | MISC between B3 and W1P
struct Layout : actor::Layout<2, NLOG, 32 + 32 + 4> {
  __host__ __device__ constexpr Layout(int nb1, int mb) : actor::Layout<2, NLOG, 32 + 32 + 4>{nb1, mb} {}
  __host__ __device__ constexpr int mean() const { return extra(); }
  __host__ __device__ constexpr int stdv() const { return mean() + 32; }
  __host__ __device__ constexpr int misc() const { return stdv() + 32; }
};
static_assert(Layout{1, 2}.w1p() == Layout{1, 2}.misc() + 4 && Layout{1, 2}.w2p() % 4 == 0, "16-byte aligned pieces");

// SiLU (actor_core.h silu_f32) x sigmoid(x) = x / (1 + exp(-x)): libm's expf, one add, the correctly rounded division.
// Largest error against float64 over every f32 in [-87, 88], in ulps of the result (tools/diag/brax_act_ulp.c):
// 2.38 ulp with a correctly rounded expf (at x = -16.68, where 1 + e rounds at e's 2^24 and the quotient sits at the
// bottom of its binade), 4.28 ulp with an expf one ulp off either way, which is what HIP documents for the device's.
// SILU_ULP is the bound the tests use.
constexpr float SILU_ULP = 4.5f;

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

// The forward of the wave's tile, all 64 lanes: ob = the raw observation row of env lane & 31; out = its eight
// logits (both lane halves get them). L: the staged image (Layout{net.nb1, MB}); packed: the global image.
template <int MB>
__device__ __forceinline__ void forward(const float* __restrict__ L, const float* packed, const actor::Net& net,
                                        const float (&ob)[OBSB], float (&out)[NLOG]) {
  const Layout lay{net.nb1, MB};
  gbf16x8 *wp = actor::lane_pieces(packed + lay.w2p()), *wq = actor::lane_pieces(packed + lay.w1q());
  float xa[8], xb[8];
  normalise(L, lay, ob, xa, xb);
  const P3 xpa = split8(xa), xpb = split8(xb);
  actor::forward<MB, 3>(L, lay, net.actfn, xpa, xpb, wp, wq, out);
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

// NormalTanh's sample on the logits: raw = loc + scale z, scale = softplus(raw scale) + min_std; the products and
// sums are separate f32 roundings (no contraction), as torch forms them. The one definition of the draw: the
// env action below, quad_brax_actor_sample and the unroll kernel (brax_unroll.hip) all take raw from here.
__device__ __forceinline__ void sample_raw(const float (&lg)[NLOG], float min_std, uint64_t seed, uint64_t env,
                                           uint32_t step, float (&raw)[4], float (&sc)[4]) {
  float z[4];
  gauss4_brax(seed, env, step, z);
#pragma unroll
  for (int k = 0; k < 4; k++) {
    sc[k] = __fadd_rn(softplus_f32(lg[4 + k]), min_std);
    raw[k] = __fadd_rn(lg[k], __fmul_rn(sc[k], z[k]));
  }
}

// NormalTanh on the logits: tanh(loc) or tanh(raw)
__device__ __forceinline__ void env_action(const float (&lg)[NLOG], float min_std, bool deterministic, uint64_t seed,
                                           uint64_t env, uint32_t step, float (&a)[4]) {
  if (deterministic) {
#pragma unroll
    for (int k = 0; k < 4; k++) a[k] = actor::tanh_f32(lg[k]);
    return;
  }
  float raw[4], sc[4];
  sample_raw(lg, min_std, seed, env, step, raw, sc);
#pragma unroll
  for (int k = 0; k < 4; k++) a[k] = actor::tanh_f32(raw[k]);
}

// NormalTanh.log_prob(logits, raw) (ppo/brax_ppo.py) from the stored raw action, not from z -- the expression the
// loss evaluates later on the same raw: sum over the four components of
//   -0.5 ((raw - loc) / scale)^2 - 0.5 log 2 pi - log scale - 2 (log 2 - raw - softplus(-2 raw)),
// every operation its own f32 rounding in torch's order (no contraction), libm's logf, softplus_f32 above and the
// correctly rounded division. sc: sample_raw's scale.
__device__ __forceinline__ float log_prob(const float (&lg)[NLOG], const float (&raw)[4], const float (&sc)[4]) {
  constexpr float HALF_LOG_2PI = 0.918938533204672742f, LOG2 = 0.693147180559945309f;
  float lp[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const float t = __fdiv_rn(__fsub_rn(raw[k], lg[k]), sc[k]);
    const float n = __fsub_rn(__fsub_rn(__fmul_rn(-0.5f, __fmul_rn(t, t)), HALF_LOG_2PI), logf(sc[k]));
    const float sp = softplus_f32(__fmul_rn(-2.0f, raw[k]));
    const float det = __fmul_rn(2.0f, __fsub_rn(__fsub_rn(LOG2, raw[k]), sp));
    lp[k] = __fsub_rn(n, det);
  }
  return __fadd_rn(__fadd_rn(__fadd_rn(lp[0], lp[1]), lp[2]), lp[3]);
}

// One sampled step of a row, the definition quad_brax_actor_sample and the unroll kernel share: raw, its log-prob
// and the env action tanh(raw) (env_action's bits for deterministic = 0)
__device__ __forceinline__ void sample_action(const float (&lg)[NLOG], float min_std, uint64_t seed, uint64_t env,
                                              uint32_t step, float (&raw)[4], float& logp, float (&a)[4]) {
  float sc[4];
  sample_raw(lg, min_std, seed, env, step, raw, sc);
  logp = log_prob(lg, raw, sc);
#pragma unroll
  for (int k = 0; k < 4; k++) a[k] = actor::tanh_f32(raw[k]);
}

}  // namespace brax

}  // namespace quadenv
