// brax_learner.hip -- the Brax learner's minibatch gradient (quad_brax_ppo_grad): the gradient of
// ppo/brax_ppo.py brax_ppo_loss (brax's compute_ppo_loss) with respect to the policy net 21 -> 128 -> 128 -> 8 and
// the value net 21 -> 128 -> 128 -> 1 (ReLU), gathered straight from the time-major unroll buffers through the
// minibatch's trajectory index. Four launches on the caller's stream, no host synchronisation:
//
//   k_brax_value    V of all (L + 1) mb rows (baseline and bootstrap)            -> workspace values [L + 1][mb]
//   k_brax_gae      brax_gae's backward scan, one lane per trajectory           -> vs, advantages [L][mb]; per-block
//                   float64 sums of the advantages and of their squares, in a fixed order
//   k_brax_grad     blocks [0, nb): the policy net over rounds of 64 loss rows -- forward, NormalTanh.log_prob at
//                   the stored raw, rho, the clipped surrogate, the entropy term at one sample, dL/dlogits, backward;
//                   blocks [nb, 2 nb): the value net over the same rows -- forward, dv = -0.5 (vs - v) / (L mb),
//                   backward (the bootstrap rows carry no gradient)                  -> per-block partial images
//   k_brax_reduce   the partials in block order, in float64                     -> gradients (flax layout), stats
//
// Every matrix product (layer 1, layer 2, dW2, dh1, dW1) runs on v_mfma_f32_32x32x16_bf16 over three-piece bf16
// splits of both operands (learner_x3_common.h split8 / mma3s: f32-level error). Wave w owns neurons 32w .. 32w + 31
// of both hidden layers, as in learner_x3.hip. Unlike that kernel the activations live in LDS as f32 images and every
// operand is split where it is used: a minibatch of the recommended command is 160 rounds for 128 blocks per net, so
// a block runs one or two rounds and the launch is bound by its latency, not by the split's VALU work.
// The 1.0 in column 21 of the observation image makes row 21 of dW1 the first layer's bias gradient.
// The head (8 or 1 outputs), the loss terms, dh2, dW3 and the bias sums are f32 VALU work in a fixed order.
//
// MFMA maps (cdna_hip_programming.md, bf16 32x32x16): lane l, r = l & 31, h = l >> 5; operand element j of A is
// A[r][8h + j], of B is B[8h + j][r]; accumulator register g is D[acc_row(g, h)][r].
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/quadenv.h"
#include "brax_actor.h"
#include "brax_learner.h"
#include "brax_learner_common.h"
#include "dispatch.h"
#include "learner_x3_common.h"

namespace quadenv {

int set_error(int code, const char* msg);  // quadenv.hip

namespace braxl {
namespace {

namespace x3 = lrn::x3;
using x3::X3;

// LDS (floats)
constexpr int XS = 36;    // observation image row: 21 normalised features, 1.0, 10 zeros, 4 pad
constexpr int HS = 132;   // hidden image row: 128 + 4 pad
constexpr int O_X = 0;
constexpr int O_H1 = O_X + RND * XS;
constexpr int O_H2 = O_H1 + RND * HS;    // relu(h2); dh1 after dh2 was formed
constexpr int O_DH2 = O_H2 + RND * HS;
constexpr int O_LOGIT = O_DH2 + RND * HS;  // [64][8] head outputs
constexpr int O_D = O_LOGIT + RND * 8;     // [64][8] dL/d(head output)
constexpr int O_W3 = O_D + RND * 8;        // [128][NOUT]
constexpr int O_MS = O_W3 + HB * NLOG;     // mean [32], std [32] (padded with 0 / 1)
constexpr int O_RED = O_MS + 64;           // double [2][256]
constexpr int L_TOTAL = O_RED + 2 * LB * 2;
constexpr int LDS_BYTES = L_TOTAL * 4;     // 123,136 B
static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
static_assert(O_RED % 2 == 0 && O_H1 % 4 == 0 && O_H2 % 4 == 0 && O_DH2 % 4 == 0 && HS % 4 == 0 && XS % 4 == 0, "alignment");
static_assert(RND * 12 <= RND * HS && HB * 9 <= RND * HS, "the end-of-launch sums alias the H1 and DH2 images");

struct Lane {
  int tid, w, r, h;
  __device__ __forceinline__ Lane() {
    tid = threadIdx.x;
    w = tid >> 6;
    r = tid & 31;
    h = (tid >> 5) & 1;
  }
};

// one k-step of 16 of a 32 x 32 product: fa(j) = A[r][8h + j], fb(j) = B[8h + j][r]
template <class FA, class FB>
__device__ __forceinline__ void kstep(f32x16& big, f32x16& sm, FA&& fa, FB&& fb) {
  float av[8], bv[8];
#pragma unroll
  for (int j = 0; j < 8; j++) { av[j] = fa(j); bv[j] = fb(j); }
  x3::mma3s(x3::split8(av), x3::split8(bv), big, sm);
}
template <class F>
__device__ __forceinline__ X3 operand(F&& f) {
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; j++) v[j] = f(j);
  return x3::split8(v);
}

__device__ __forceinline__ f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int g = 0; g < 16; g++) z[g] = 0.f;
  return z;
}

// rows q0 .. q0 + 63 of the time-major minibatch (row q = t mb + j: step t of trajectory index[j]; t = L is the
// bootstrap row, from next_obs) normalised as RunningStats.normalize does, into the observation image; rows past
// `nrows` are all zero, their 1.0 column included
__device__ __forceinline__ void stage_x(const Args& a, float* Lf, int q0, int nrows) {
  const int tid = threadIdx.x, row = tid >> 2, f0 = (tid & 3) * 8;
  float v[8];
  gather_row8(a, Lf + O_MS, q0 + row, nrows, f0, v);
#pragma unroll
  for (int j = 0; j < 8; j++) Lf[O_X + row * XS + f0 + j] = v[j];
}

// relu(h1), relu(h2) of the round into the H1 / H2 images; ends with a barrier
__device__ __forceinline__ void forward(const Net& W, float* Lf, const Lane& ln) {
  const int w = ln.w, r = ln.r, h = ln.h;
  {  // layer 1: h1^T block w = W1^T x^T, K = 32 (features 21 .. 31 of A are zero)
    X3 a1[2];
#pragma unroll
    for (int s = 0; s < 2; s++)
      a1[s] = operand([&](int j) {
        const int f = 16 * s + 8 * h + j;
        return f < OBSB ? W.w0[f * HB + 32 * w + r] : 0.f;
      });
#pragma unroll
    for (int t = 0; t < 2; t++) {
      f32x16 big, sm = zero16();
#pragma unroll
      for (int g = 0; g < 16; g++) big[g] = W.b0[32 * w + acc_row(g, h)];
#pragma unroll
      for (int s = 0; s < 2; s++) {
        const X3 b = operand([&](int j) { return Lf[O_X + (32 * t + r) * XS + 16 * s + 8 * h + j]; });
        x3::mma3s(a1[s], b, big, sm);
      }
      big += sm;
#pragma unroll
      for (int g = 0; g < 16; g++) Lf[O_H1 + (32 * t + r) * HS + 32 * w + acc_row(g, h)] = relu(big[g]);
    }
  }
  __syncthreads();
  {  // layer 2: h2^T block w = W2^T h1^T, K = 128
    f32x16 big[2], sm[2];
#pragma unroll
    for (int g = 0; g < 16; g++) big[0][g] = W.b1[32 * w + acc_row(g, h)];
    big[1] = big[0];
    sm[0] = sm[1] = zero16();
#pragma unroll
    for (int s = 0; s < 8; s++) {
      const X3 a2 = operand([&](int j) { return W.w1[(16 * s + 8 * h + j) * HB + 32 * w + r]; });
#pragma unroll
      for (int t = 0; t < 2; t++) {
        const X3 b = operand([&](int j) { return Lf[O_H1 + (32 * t + r) * HS + 16 * s + 8 * h + j]; });
        x3::mma3s(a2, b, big[t], sm[t]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int t = 0; t < 2; t++) {
      big[t] += sm[t];
#pragma unroll
      for (int g = 0; g < 16; g++) Lf[O_H2 + (32 * t + r) * HS + 32 * w + acc_row(g, h)] = relu(big[t][g]);
    }
  }
  __syncthreads();
}

// the head of the round's rows into the LOGIT image, neurons in index order; ends with a barrier.
// Thread 4 row + q: NOUT = 8: outputs 2q, 2q + 1 over all 128 neurons; NOUT = 1: neurons 32q .. 32q + 31, the four
// partial sums added in the order of q
template <int NOUT>
__device__ __forceinline__ void head(const float* b3, float* Lf) {
  const int tid = threadIdx.x, row = tid >> 2, q = tid & 3;
  const float* hrow = Lf + O_H2 + row * HS;
  if constexpr (NOUT == NLOG) {
    float s0 = 0.f, s1 = 0.f;
#pragma unroll 8
    for (int n = 0; n < HB; n++) {
      const float hv = hrow[n];
      s0 = fmaf(hv, Lf[O_W3 + n * NLOG + 2 * q], s0);
      s1 = fmaf(hv, Lf[O_W3 + n * NLOG + 2 * q + 1], s1);
    }
    Lf[O_LOGIT + row * 8 + 2 * q] = s0 + b3[2 * q];
    Lf[O_LOGIT + row * 8 + 2 * q + 1] = s1 + b3[2 * q + 1];
  } else {
    float p = 0.f;
#pragma unroll 8
    for (int i = 0; i < 32; i++) p = fmaf(hrow[32 * q + i], Lf[O_W3 + 32 * q + i], p);
    const int b = (tid & 63) & ~3;
    const float s = ((__shfl(p, b) + __shfl(p, b + 1)) + __shfl(p, b + 2)) + __shfl(p, b + 3);
    if (q == 0) Lf[O_LOGIT + row * 8] = s + b3[0];
  }
  __syncthreads();
}

template <int NOUT>
__device__ __forceinline__ void stage_head_weights(const Net& W, float* Lf) {
  for (int i = threadIdx.x; i < HB * NOUT; i += LB) Lf[O_W3 + i] = W.w2[i];
}

// ---- launch 1: the value net's forward over all (L + 1) mb rows, one round per block
__global__ __launch_bounds__(LB, 1) void k_brax_value(Args a) {
  extern __shared__ __attribute__((aligned(16))) float lds_v[];
  float* const Lf = lds_v;
  const Lane ln;
  stage_norm(a, Lf + O_MS);
  stage_head_weights<1>(a.vf, Lf);
  __syncthreads();
  const int q0 = blockIdx.x * RND;
  stage_x(a, Lf, q0, a.rows_all);
  __syncthreads();
  forward(a.vf, Lf, ln);
  head<1>(a.vf.b2, Lf);
  if (ln.tid < RND && q0 + ln.tid < a.rows_all) {
    const float v = Lf[O_LOGIT + ln.tid * 8];
    a.values[q0 + ln.tid] = v;
    if (a.d_values) a.d_values[q0 + ln.tid] = v;
  }
}

// ---- launch 2: brax_gae per trajectory (ppo/brax_ppo.py brax_gae: every operation its own f32 rounding, in torch's
// order) and the block's advantage sums
__global__ __launch_bounds__(256) void k_brax_gae(Args a) {
  __shared__ double red[2][256];
  const int tid = threadIdx.x;
  double s = 0.0, s2 = 0.0;
  for (int j = blockIdx.x * 256 + tid; j < a.mb; j += gridDim.x * 256) {
    const int64_t m = a.idx[j];
    const float boot = a.values[a.L * a.mb + j];
    float acc = 0.f, v_next = boot, vs_next = boot;
    for (int t = a.L - 1; t >= 0; t--) {
      const size_t row = step_row(a, m, t);
      const float rw = __fmul_rn(a.reward[row], a.rscale);
      const float tr = a.trunc[row], tm = __fsub_rn(1.f, tr);
      const float term = __fmul_rn(__fsub_rn(1.f, a.discount[row]), __fsub_rn(1.f, tr));
      const float g = __fmul_rn(a.gamma, __fsub_rn(1.f, term));
      const float v = a.values[t * a.mb + j];
      const float delta = __fmul_rn(__fsub_rn(__fadd_rn(rw, __fmul_rn(g, v_next)), v), tm);
      acc = __fadd_rn(delta, __fmul_rn(__fmul_rn(__fmul_rn(g, tm), a.lam), acc));
      const float vs = __fadd_rn(acc, v);
      const float adv = __fmul_rn(__fsub_rn(__fadd_rn(rw, __fmul_rn(g, vs_next)), v), tm);
      a.vs[t * a.mb + j] = vs;
      a.adv[t * a.mb + j] = adv;
      if (a.d_vs) a.d_vs[t * a.mb + j] = vs;
      const double d = adv;
      s += d;
      s2 += d * d;
      v_next = v;
      vs_next = vs;
    }
  }
  red[0][tid] = s;
  red[1][tid] = s2;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) { red[0][tid] += red[0][tid + o]; red[1][tid] += red[1][tid + o]; }
    __syncthreads();
  }
  if (tid == 0) { a.adv_part[2 * blockIdx.x] = red[0][0]; a.adv_part[2 * blockIdx.x + 1] = red[1][0]; }
}

// a pointer the compiler cannot see through: loads from it stay inside the round loop (learner_x3.hip: hoisted out,
// the loop-invariant weight operands take more registers than there are)
__device__ __forceinline__ const float* opaque(const float* p) {
  uint64_t b = reinterpret_cast<uint64_t>(p);
  asm volatile("" : "+s"(b));
  return reinterpret_cast<const float*>(b);
}

// ---- launch 3: one net's gradient over the block's rounds
template <int NOUT>
__device__ __forceinline__ void grad_body(const Args& a, float* Lf, int blk) {
  const Net& W0 = NOUT == NLOG ? a.pi : a.vf;
  const Lane ln;
  const int tid = ln.tid, w = ln.w, r = ln.r, h = ln.h;
  AdvNorm an{0.f, 1.f};
  if constexpr (NOUT == NLOG) an = adv_norm(a, reinterpret_cast<double*>(Lf + O_RED), reinterpret_cast<double*>(Lf + O_RED) + LB);
  stage_norm(a, Lf + O_MS);
  stage_head_weights<NOUT>(W0, Lf);
  __syncthreads();

  // accumulators of the whole launch
  f32x16 dW2[4], dW1 = zero16();
#pragma unroll
  for (int jb = 0; jb < 4; jb++) dW2[jb] = zero16();
  const int hn = tid & 127, hf = tid >> 7;  // dh2 / dW3 / db2: neuron hn, rows hf, hf + 2, ..
  float w3r[NOUT], dW3[NOUT], dB2 = 0.f;
#pragma unroll
  for (int o = 0; o < NOUT; o++) { w3r[o] = Lf[O_W3 + hn * NOUT + o]; dW3[o] = 0.f; }
  float db3[NOUT], st0 = 0.f, st1 = 0.f;  // threads 0 .. 63, one row each: head bias gradient and the loss sums
#pragma unroll
  for (int o = 0; o < NOUT; o++) db3[o] = 0.f;
  const float ce = a.ent_cost * a.inv_rows;

  const int rd1 = min((blk + 1) * a.rpb, (a.rows_loss + RND - 1) / RND);
  for (int rd = blk * a.rpb; rd < rd1; rd++) {
    const int q0 = rd * RND;
    const Net W{opaque(W0.w0), opaque(W0.b0), opaque(W0.w1), opaque(W0.b1), W0.w2, W0.b2};
    stage_x(a, Lf, q0, a.rows_loss);
    __syncthreads();
    forward(W, Lf, ln);
    head<NOUT>(W.b2, Lf);

    // ---- per-row loss terms and dL/d(head output): wave 0, one row per lane
    if (tid < RND) {
      const int q = q0 + tid;
      float d[NOUT];
#pragma unroll
      for (int o = 0; o < NOUT; o++) d[o] = 0.f;
      if (q < a.rows_loss) {
        if constexpr (NOUT == NLOG) {
          policy_row_terms(a, Lf + O_LOGIT + tid * 8, q, an, ce, d, st0, st1);
        } else {
          const float err = a.vs[q] - Lf[O_LOGIT + tid * 8];
          d[0] = -0.5f * err * a.inv_rows;
          st0 += err * err;
        }
      }
#pragma unroll
      for (int o = 0; o < NOUT; o++) {
        Lf[O_D + tid * 8 + o] = d[o];
        db3[o] += d[o];
      }
    }
    __syncthreads();

    // ---- dh2 = relu'(h2) (d W3^T) -> DH2 image; dW3 and db2 per thread (neuron hn, every second row)
#pragma unroll 4
    for (int i = 0; i < RND / 2; i++) {
      const int row = hf + 2 * i;
      const float h2 = Lf[O_H2 + row * HS + hn];
      float g = 0.f;
#pragma unroll
      for (int o = 0; o < NOUT; o++) {
        const float dv = Lf[O_D + row * 8 + o];
        g = fmaf(dv, w3r[o], g);
        dW3[o] = fmaf(dv, h2, dW3[o]);
      }
      const float dh = h2 > 0.f ? g : 0.f;
      Lf[O_DH2 + row * HS + hn] = dh;
      dB2 += dh;
    }
    __syncthreads();

    // ---- dW2 slab [in 32 jb + r][out 32 w + ..] = sum over the round's rows of h1[row][in] dh2[row][out]: fresh
    // accumulators per round, added to the launch total with VALU adds (learner_x3.hip: an MFMA chain over many
    // rounds drifts by the instruction's truncation)
#pragma unroll
    for (int jb = 0; jb < 4; jb++) {
      f32x16 big = zero16(), sm = zero16();
#pragma unroll
      for (int s = 0; s < 4; s++) {
        kstep(big, sm, [&](int j) { return Lf[O_DH2 + (16 * s + 8 * h + j) * HS + 32 * w + r]; },
              [&](int j) { return Lf[O_H1 + (16 * s + 8 * h + j) * HS + 32 * jb + r]; });
        __builtin_amdgcn_sched_barrier(0);  // one k-step's operands live at a time
      }
      dW2[jb] += big + sm;
    }
    // ---- dh1^T block w = relu'(h1) . (W2 dh2^T) -> the H2 image's place (its readers finished before the barrier)
    {
      f32x16 big[2], sm[2];
      big[0] = big[1] = sm[0] = sm[1] = zero16();
#pragma unroll
      for (int s = 0; s < 8; s++) {
        const X3 av = operand([&](int j) { return W.w1[(32 * w + r) * HB + 16 * s + 8 * h + j]; });
#pragma unroll
        for (int t = 0; t < 2; t++) {
          const X3 bv = operand([&](int j) { return Lf[O_DH2 + (32 * t + r) * HS + 16 * s + 8 * h + j]; });
          x3::mma3s(av, bv, big[t], sm[t]);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int t = 0; t < 2; t++) {
        big[t] += sm[t];
#pragma unroll
        for (int g = 0; g < 16; g++) {
          const int o = (32 * t + r) * HS + 32 * w + acc_row(g, h);
          Lf[O_H2 + o] = Lf[O_H1 + o] > 0.f ? big[t][g] : 0.f;
        }
      }
    }
    __syncthreads();
    // ---- dW1 slab [feature r][out 32 w + ..] = sum over the rows of x[row][feature] dh1[row][out]; feature 21 is
    // the 1.0 column: db1
    {
      f32x16 big = zero16(), sm = zero16();
#pragma unroll
      for (int s = 0; s < 4; s++) {
        kstep(big, sm, [&](int j) { return Lf[O_H2 + (16 * s + 8 * h + j) * HS + 32 * w + r]; },
              [&](int j) { return Lf[O_X + (16 * s + 8 * h + j) * XS + r]; });
        __builtin_amdgcn_sched_barrier(0);
      }
      dW1 += big + sm;
    }
    __syncthreads();  // the next round's staging overwrites the images
  }

  // ---- the block's partial image, in the gradients' layout
  float* const P = a.part + size_t(blk + (NOUT == NLOG ? 0 : a.nb)) * PSTRIDE;
#pragma unroll
  for (int g = 0; g < 16; g++) {
    const int n = 32 * w + acc_row(g, h);
    if (r < OBSB) P[P_W1 + r * HB + n] = dW1[g];
    if (r == OBSB) P[P_B1 + n] = dW1[g];
#pragma unroll
    for (int jb = 0; jb < 4; jb++) P[P_W2 + (32 * jb + r) * HB + n] = dW2[jb][g];
  }
  // dW3 / db2: the two row halves of each neuron, even rows + odd rows
  float* const S1 = Lf + O_DH2;  // [128][9]
  float* const S2 = Lf + O_H1;   // [64][12]
  if (hf == 1) {
#pragma unroll
    for (int o = 0; o < NOUT; o++) S1[hn * 9 + o] = dW3[o];
    S1[hn * 9 + 8] = dB2;
  }
  if (tid < RND) {
#pragma unroll
    for (int o = 0; o < NOUT; o++) S2[tid * 12 + o] = db3[o];
    S2[tid * 12 + 8] = st0;
    S2[tid * 12 + 9] = st1;
  }
  __syncthreads();
  if (hf == 0) {
#pragma unroll
    for (int o = 0; o < NOUT; o++) P[P_W3 + hn * NOUT + o] = dW3[o] + S1[hn * 9 + o];
    P[P_B2 + hn] = dB2 + S1[hn * 9 + 8];
  }
  if (tid < 10 && (tid < NOUT || tid >= 8)) {  // head bias gradient and the loss sums over the 64 row lanes, in order
    double s = 0.0;
    for (int i = 0; i < RND; i++) s += double(S2[i * 12 + tid]);
    if (tid < NOUT) P[P_B3 + tid] = float(s);
    else if (NOUT == NLOG) P[P_STATS + (tid == 8 ? 0 : 2)] = float(s);
    else if (tid == 8) P[P_STATS + 1] = float(s);
  }
}

__global__ __launch_bounds__(LB, 1) void k_brax_grad(Args a) {
  extern __shared__ __attribute__((aligned(16))) float lds_g[];
  if (int(blockIdx.x) < a.nb)
    grad_body<NLOG>(a, lds_g, blockIdx.x);
  else
    grad_body<1>(a, lds_g, blockIdx.x - a.nb);
}

// ---- launch 4: element e of a net's partial image summed over its blocks in block order (float64) into the
// gradient tensor that owns it; the three loss statistics
__global__ __launch_bounds__(256) void k_brax_reduce(RArgs ra) {
  const int net = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x;
  if (e >= PSTRIDE) return;
  const int nout = net == 0 ? NLOG : 1;
  if (e >= P_W3 && e < P_B3 && e - P_W3 >= HB * nout) return;
  if (e >= P_B3 && e < P_STATS && e - P_B3 >= nout) return;
  if (e >= P_STATS && (!ra.stats || e >= P_STATS + 3 || (net == 0) == (e == P_STATS + 1))) return;
  const float* p = ra.part + size_t(net) * size_t(ra.nb) * PSTRIDE + e;
  double s = 0.0;
  for (int b = 0; b < ra.nb; b++) s += double(p[size_t(b) * PSTRIDE]);
  const QuadBraxPPOGrads& g = ra.gr;
  if (e >= P_STATS) {
    const int k = e - P_STATS;
    ra.stats[k] = float(k == 0 ? -s * ra.inv_rows : (k == 1 ? 0.25 * s * ra.inv_rows : -ra.ent_cost * s * ra.inv_rows));
    return;
  }
  float* dst;
  int off;
  if (e < P_B1) { dst = net ? g.vf_w0 : g.pi_w0; off = e - P_W1; }
  else if (e < P_W2) { dst = net ? g.vf_b0 : g.pi_b0; off = e - P_B1; }
  else if (e < P_B2) { dst = net ? g.vf_w1 : g.pi_w1; off = e - P_W2; }
  else if (e < P_W3) { dst = net ? g.vf_b1 : g.pi_b1; off = e - P_B2; }
  else if (e < P_B3) { dst = net ? g.vf_w2 : g.pi_w2; off = e - P_W3; }
  else { dst = net ? g.vf_b2 : g.pi_b2; off = e - P_B3; }
  dst[off] = float(s);
}

int fail(int code, const char* msg) { return set_error(code, msg); }

bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

}  // namespace

hipError_t launch_gae(const Args& a, hipStream_t s) {
  hipLaunchKernelGGL(k_brax_gae, dim3(a.gae_blocks), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace braxl
}  // namespace quadenv

using namespace quadenv;
using namespace quadenv::braxl;

extern "C" {

int64_t quad_brax_ppo_workspace_bytes(int32_t mb, int32_t L) {
  if (mb < 1 || L < 1 || L > MAX_L || int64_t(L + 1) * mb > (int64_t(1) << 28)) return 0;
  return layout_of(mb, L).bytes;
}

int quad_brax_ppo_grad(const QuadBraxPPOParams* p, const QuadBraxPPOBatch* b, const QuadBraxPPOGrads* gr,
                       void* workspace, int64_t workspace_bytes, void* stream) {
  if (!p || !b || !gr || !workspace) return fail(QUAD_EINVAL, "quad_brax_ppo_grad: NULL argument");
  if (p->policy_h1 != HB || p->policy_h2 != HB || p->value_h1 != HB || p->value_h2 != HB ||
      p->activation != QUAD_ACTFN_RELU)
    return fail(QUAD_EINVAL, "quad_brax_ppo_grad: the family is policy and value nets (128, 128) with QUAD_ACTFN_RELU");
  const void* prm[] = {p->pi_w0, p->pi_b0, p->pi_w1, p->pi_b1, p->pi_w2, p->pi_b2, p->vf_w0, p->vf_b0,
                       p->vf_w1, p->vf_b1, p->vf_w2, p->vf_b2, p->mean,  p->std};
  for (const void* q : prm)
    if (!q || misaligned(q, 4)) return fail(QUAD_EINVAL, "quad_brax_ppo_grad: a parameter pointer is NULL or misaligned");
  const void* grd[] = {gr->pi_w0, gr->pi_b0, gr->pi_w1, gr->pi_b1, gr->pi_w2, gr->pi_b2,
                       gr->vf_w0, gr->vf_b0, gr->vf_w1, gr->vf_b1, gr->vf_w2, gr->vf_b2};
  for (const void* q : grd)
    if (!q || misaligned(q, 4)) return fail(QUAD_EINVAL, "quad_brax_ppo_grad: a gradient pointer is NULL or misaligned");
  const void* buf[] = {b->obs, b->next_obs, b->log_prob, b->reward, b->discount, b->truncation};
  for (const void* q : buf)
    if (!q || misaligned(q, 4)) return fail(QUAD_EINVAL, "quad_brax_ppo_grad: an unroll buffer is NULL or misaligned");
  if (!b->raw || misaligned(b->raw, 16)) return fail(QUAD_EINVAL, "quad_brax_ppo_grad: raw must be 16-byte aligned");
  if (!b->index || misaligned(b->index, 8)) return fail(QUAD_EINVAL, "quad_brax_ppo_grad: index is NULL or misaligned");
  if (misaligned(b->entropy_noise, 16) || misaligned(b->noise_out, 16))
    return fail(QUAD_EINVAL, "quad_brax_ppo_grad: entropy_noise and noise_out must be 16-byte aligned");
  if (misaligned(b->values, 4) || misaligned(b->vs, 4) || misaligned(b->advantages, 4) || misaligned(b->stats, 4))
    return fail(QUAD_EINVAL, "quad_brax_ppo_grad: a diagnostic output is misaligned");
  if (misaligned(workspace, 16)) return fail(QUAD_EINVAL, "quad_brax_ppo_grad: workspace must be 16-byte aligned");
  if (b->mb < 1) return fail(QUAD_EINVAL, "quad_brax_ppo_grad: mb must be >= 1");
  if (b->L < 1 || b->L > MAX_L) return fail(QUAD_EINVAL, "quad_brax_ppo_grad: L must be in [1, 64]");
  if (b->U < 1 || b->N < 1) return fail(QUAD_EINVAL, "quad_brax_ppo_grad: U and N must be >= 1");
  if (int64_t(b->L + 1) * b->mb > (int64_t(1) << 28))
    return fail(QUAD_EINVAL, "quad_brax_ppo_grad: (L + 1) * mb must be <= 2^28");
  if (!(b->clipping_epsilon > 0.f)) return fail(QUAD_EINVAL, "quad_brax_ppo_grad: clipping_epsilon must be > 0");
  const Layout l = layout_of(b->mb, b->L);
  if (workspace_bytes < l.bytes) return fail(QUAD_EINVAL, "quad_brax_ppo_grad: workspace too small");

  char* const ws = static_cast<char*>(workspace);
  Args a{};
  a.pi = Net{p->pi_w0, p->pi_b0, p->pi_w1, p->pi_b1, p->pi_w2, p->pi_b2};
  a.vf = Net{p->vf_w0, p->vf_b0, p->vf_w1, p->vf_b1, p->vf_w2, p->vf_b2};
  a.mean = p->mean; a.std = p->std; a.min_std = p->min_std;
  a.obs = b->obs; a.next_obs = b->next_obs; a.raw = b->raw; a.logp = b->log_prob; a.reward = b->reward;
  a.discount = b->discount; a.trunc = b->truncation; a.idx = b->index;
  a.noise = b->entropy_noise; a.noise_out = b->noise_out;
  a.d_values = b->values; a.d_vs = b->vs; a.d_adv = b->advantages;
  a.values = reinterpret_cast<float*>(ws + l.o_values);
  a.vs = reinterpret_cast<float*>(ws + l.o_vs);
  a.adv = reinterpret_cast<float*>(ws + l.o_adv);
  a.adv_part = reinterpret_cast<double*>(ws + l.o_adv_part);
  a.part = reinterpret_cast<float*>(ws + l.o_part);
  a.U = b->U; a.L = b->L; a.N = b->N; a.mb = b->mb;
  a.rows_loss = l.rows_loss; a.rows_all = l.rows_all; a.nb = l.nb; a.rpb = l.rpb; a.gae_blocks = l.gae_blocks;
  a.norm_adv = b->normalize_advantage != 0;
  a.clip = b->clipping_epsilon; a.ent_cost = b->entropy_cost; a.gamma = b->discounting; a.lam = b->gae_lambda;
  a.rscale = b->reward_scaling; a.inv_rows = 1.0f / float(l.rows_loss);
  a.noise_step = b->noise_step; a.seed = b->seed;

  hipStream_t s = static_cast<hipStream_t>(stream);
  if (launch_lds<&k_brax_value>(dim3(l.nbv), dim3(LB), LDS_BYTES, s, a) != hipSuccess)
    return fail(QUAD_EHIP, "k_brax_value launch failed");
  if (launch_gae(a, s) != hipSuccess) return fail(QUAD_EHIP, "k_brax_gae launch failed");
  if (launch_lds<&k_brax_grad>(dim3(2 * l.nb), dim3(LB), LDS_BYTES, s, a) != hipSuccess)
    return fail(QUAD_EHIP, "k_brax_grad launch failed");
  RArgs ra{};
  ra.gr = *gr; ra.part = a.part; ra.stats = b->stats; ra.nb = l.nb;
  ra.inv_rows = 1.0 / double(l.rows_loss); ra.ent_cost = double(b->entropy_cost);
  hipLaunchKernelGGL(k_brax_reduce, dim3((PSTRIDE + 255) / 256, 2), dim3(256), 0, s, ra);
  if (hipGetLastError() != hipSuccess) return fail(QUAD_EHIP, "k_brax_reduce launch failed");
  return QUAD_OK;
}

}  // extern "C"
