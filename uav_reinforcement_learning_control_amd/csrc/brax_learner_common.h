// brax_learner_common.h -- the device pieces of the Brax loss that quad_brax_ppo_grad (brax_learner.hip) and
// quad_brax_ppo_arch_grad (brax_learner_arch.hip) share: the trajectory gather with the running statistics'
// normalisation, the entropy sample's Philox draw, the advantage normalisation from the GAE launch's float64 sums and
// the policy's per-row loss terms with dL/dlogits. The GAE launch itself is k_brax_gae in brax_learner.hip, started
// through launch_gae. All of them read brax_learner.h's Args.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/quadenv.h"
#include "brax_actor.h"
#include "brax_learner.h"

namespace quadenv {
namespace braxl {

// launch 2 of both gradients (brax_learner.hip): brax_gae per trajectory from a.values into a.vs / a.adv and the
// a.gae_blocks blocks' float64 advantage sums into a.adv_part
hipError_t launch_gae(const Args& a, hipStream_t s);

// trajectory m = u N + n, step t -> row (u L + t) N + n of the time-major buffers
__device__ __forceinline__ size_t step_row(const Args& a, int64_t m, int t) {
  const int64_t u = m / a.N, n = m - u * a.N;
  return size_t((u * a.L + t) * a.N + n);
}

// mean [32], std [32] (padded with 0 / 1) into `ms`
__device__ __forceinline__ void stage_norm(const Args& a, float* ms) {
  const int tid = threadIdx.x;
  if (tid < 32) {
    ms[tid] = tid < OBSB ? a.mean[tid] : 0.f;
    ms[32 + tid] = tid < OBSB ? a.std[tid] : 1.f;
  }
}

// features f0 .. f0 + 7 of row q of the time-major minibatch (row q = t mb + j: step t of trajectory index[j]; t = L
// is the bootstrap row, from next_obs) normalised as RunningStats.normalize does, feature 21 = 1.0, the rest zero; a
// row past `nrows` is all zero, its 1.0 column included
__device__ __forceinline__ void gather_row8(const Args& a, const float* ms, int q, int nrows, int f0, float v[8]) {
#pragma unroll
  for (int j = 0; j < 8; j++) v[j] = 0.f;
  if (q < nrows) {
    const int t = q / a.mb, jj = q - t * a.mb;
    const int64_t m = a.idx[jj];
    const float* src = t < a.L ? a.obs + step_row(a, m, t) * OBSB : a.next_obs + size_t(m) * OBSB;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const int f = f0 + j;
      if (f < OBSB) v[j] = __fdiv_rn(__fsub_rn(src[f], ms[f]), ms[32 + f]);
      else if (f == OBSB) v[j] = 1.f;
    }
  }
}

// Box-Muller on Philox(seed; trajectory, step, ENTROPY_STREAM): brax_actor.h gauss4_brax's draw on the entropy
// sample's own stream
__device__ __forceinline__ void gauss4_entropy(uint64_t seed, uint64_t traj, uint32_t step, float z[4]) {
  uint32_t c[4] = {uint32_t(traj), uint32_t(traj >> 32), step, ENTROPY_STREAM};
  philox4x32_10(c, uint32_t(seed), uint32_t(seed >> 32));
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const float u1 = (float(c[2 * k] >> 8) + 1.0f) * 0x1p-24f;  // (0, 1]
    const float u2 = float(c[2 * k + 1] >> 8) * 0x1p-24f;
    const float rr = __builtin_amdgcn_sqrtf(-1.38629436111989061f * __builtin_amdgcn_logf(u1));  // -2 ln u1
    z[2 * k] = rr * __builtin_amdgcn_cosf(u2);
    z[2 * k + 1] = rr * __builtin_amdgcn_sinf(u2);
  }
}

// the advantage normalisation of the minibatch: a fixed-order float64 tree over the GAE launch's block sums (red0,
// red1: LB doubles each; every thread of the LB-thread block calls), then mean and std(unbiased=False) + 1e-8 as
// brax_ppo_loss forms them; {0, 1} without normalisation
struct AdvNorm { float mu, den; };
__device__ __forceinline__ AdvNorm adv_norm(const Args& a, double* red0, double* red1) {
  if (!a.norm_adv) return AdvNorm{0.f, 1.f};
  const int tid = threadIdx.x;
  red0[tid] = tid < a.gae_blocks ? a.adv_part[2 * tid] : 0.0;
  red1[tid] = tid < a.gae_blocks ? a.adv_part[2 * tid + 1] : 0.0;
  __syncthreads();
  for (int o = LB / 2; o > 0; o >>= 1) {
    if (tid < o) { red0[tid] += red0[tid + o]; red1[tid] += red1[tid + o]; }
    __syncthreads();
  }
  const double n = double(a.rows_loss), s = red0[0], s2 = red1[0];
  const double var = fmax((s2 - s * s / n) / n, 0.0);
  return AdvNorm{float(s / n), float(sqrt(var)) + 1e-8f};
}

// the policy's loss terms of minibatch row q < rows_loss from its eight head outputs `lgp`: NormalTanh.log_prob at
// the stored raw, rho, the clipped surrogate, the entropy at one sample (given, or drawn and written to noise_out);
// d = dL/d(head output); st0 / st1 gain the row's min(s1, s2) and entropy. ce = entropy_cost / rows
__device__ __forceinline__ void policy_row_terms(const Args& a, const float* lgp, int q, const AdvNorm& an, float ce,
                                                 float d[NLOG], float& st0, float& st1) {
  const int t = q / a.mb, jj = q - t * a.mb;
  const int64_t m = a.idx[jj];
  const size_t row = step_row(a, m, t);
  const float4 r4 = reinterpret_cast<const float4*>(a.raw)[row];
  const float raw[4] = {r4.x, r4.y, r4.z, r4.w};
  float z[4];
  if (a.noise) {
    const float4 z4 = reinterpret_cast<const float4*>(a.noise)[q];
    z[0] = z4.x; z[1] = z4.y; z[2] = z4.z; z[3] = z4.w;
  } else {
    gauss4_entropy(a.seed, uint64_t(m), a.noise_step * uint32_t(a.L) + uint32_t(t), z);
  }
  if (a.noise_out) reinterpret_cast<float4*>(a.noise_out)[q] = make_float4(z[0], z[1], z[2], z[3]);
  float lg[NLOG], sc[4];
#pragma unroll
  for (int o = 0; o < NLOG; o++) lg[o] = lgp[o];
#pragma unroll
  for (int k = 0; k < 4; k++) sc[k] = __fadd_rn(brax::softplus_f32(lg[4 + k]), a.min_std);
  const float lp = brax::log_prob(lg, raw, sc);
  const float rho = expf(lp - a.logp[row]);
  const float A = a.norm_adv ? __fdiv_rn(a.adv[q] - an.mu, an.den) : a.adv[q];
  if (a.d_adv) a.d_adv[q] = A;
  // the clipped surrogate and its derivative: learner.h row_terms' tie rule and closed clamp interval
  const float cr = fminf(fmaxf(rho, 1.f - a.clip), 1.f + a.clip);
  const float sa = rho * A, sb = cr * A;
  const float w1 = sa < sb ? 1.f : (sa == sb ? 0.5f : 0.f);
  const float inr = (rho >= 1.f - a.clip && rho <= 1.f + a.clip) ? 1.f : 0.f;
  const float dlp = -a.inv_rows * A * (w1 + (1.f - w1) * inr) * rho;
  st0 += fminf(sa, sb);
  // the entropy at x = loc + scale z: sum of 1/2 + 1/2 log 2 pi + log scale + 2 (log 2 - x - softplus(-2x));
  // d/dx of the last term is -2 tanh(x)
  constexpr float HALF_LOG_2PI = 0.918938533204672742f, LOG2 = 0.693147180559945309f;
  float ent = 0.f;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const float x = __fadd_rn(lg[k], __fmul_rn(sc[k], z[k]));
    const float th = actor::tanh_f32(x);
    const float det = 2.f * ((LOG2 - x) - brax::softplus_f32(-2.f * x));
    ent += ((0.5f + HALF_LOG_2PI) + logf(sc[k])) + det;
    const float isc = __fdiv_rn(1.f, sc[k]);
    const float tt = (raw[k] - lg[k]) * isc;
    const float dloc = dlp * tt * isc + ce * 2.f * th;
    const float dscale = dlp * (tt * tt - 1.f) * isc - ce * (isc - 2.f * th * z[k]);
    const float sig = __fdiv_rn(1.f, 1.f + expf(-lg[4 + k]));  // d softplus
    d[k] = dloc;
    d[4 + k] = dscale * sig;
  }
  st1 += ent;
}

}  // namespace braxl
}  // namespace quadenv
