// brax_learner_arch.hip -- the Brax learner's minibatch gradient for the Brax actor's whole family
// (quad_brax_ppo_arch_grad): the gradient of ppo/brax_ppo.py brax_ppo_loss (quad_brax_ppo_grad's semantics) for the
// policy net 21 -> P1 -> P2 -> 8 and the value net 21 -> V1 -> V2 -> 1, each first width a multiple of 32 up to 512,
// each second width in {64, 128, 256}, the two nets' sizes independent, ReLU, tanh or SiLU, rows gathered straight
// from the time-major unroll buffers through the minibatch's trajectory index. Five launches on the caller's stream,
// no host synchronisation:
//
//   k_brax_arch_value  V of all (L + 1) mb rows (baseline and bootstrap), rounds of 32 rows      -> workspace values
//   k_brax_gae         brax_learner.hip's launch (launch_gae): vs, advantages, the float64 advantage sums
//   k_brax_arch_fwd    block (b, net): the net over rounds of 32 loss rows -- gather and normalise, forward, the loss
//                      terms (brax_learner_common.h policy_row_terms; dv = -0.5 (vs - v) / (L mb) with v read back
//                      from launch 1's values), dL/d(head), dh2, dh1; the x | 1, h1, dh2, dh1 images of every row
//                      -> workspace images; dW3, db2, db3 and the loss sums of the block's rows   -> per-block sums
//   k_brax_arch_wgrad  wave (net, split, tile): one 32 x 32 tile of dW2 = h1^T dh2 or of dW1 | db1 = [x | 1]^T dh1
//                      over the split's rows in index order                                      -> per-split images
//   k_brax_arch_reduce the splits and the blocks in order, in float64                            -> gradients, stats
//
// k_brax_grad keeps a net's dW2 in accumulators and its activations as 64-row LDS images; at (512, 256) that is 512
// registers per lane and 130 KB for H1 alone, so this file takes learner_arch.hip's shape: the weight gradients are
// output-stationary products over stored images, a tile's sum runs over the minibatch positions in a fixed order
// whatever the rows are, and the result is bit-identical from run to run and under a physical move of the
// trajectories into index order. No atomics.
//
// Every matrix product (layer 1, layer 2, dh1, dW2, dW1) runs on v_mfma_f32_32x32x16_bf16 over three-piece bf16
// splits of both operands (learner_x3_common.h split8 / mma3s), big and small terms in separate accumulators; a chain
// is at most four k-steps long and is then added to a VALU total. The 1.0 in column 21 of the observation image makes
// row 21 of the dW1 tile the first layer's bias gradient. The head (float64, rounded once), the loss terms, dh2, dW3
// and the bias sums are VALU work in a fixed order.
//
// Activations are actor_core.h's tanh_f32 / silu_f32, the actor kernels'. tanh's derivative 1 - h^2 and ReLU's h > 0
// come from the stored activation. SiLU's sigma(x) (1 + x (1 - sigma(x))) needs the pre-activation x, and 160 KB of
// LDS does not hold a second image per layer at (512, 256): layer 2 writes its derivative into the DH2 image, which is
// free until dh2 is formed there in place (same thread reads and writes an element); layer 1's pre-activation tile
// is formed again (two k-steps from the X image still in LDS, against H2 / 16 k-steps of the dh1 product) by the
// lane that forms the dh1 element it scales, so no image and no workspace traffic is added.
//
// MFMA maps (brax_learner.hip): lane l, r = l & 31, h = l >> 5; operand element j of A is A[r][8h + j], of B is
// B[8h + j][r]; accumulator register g is D[acc_row(g, h)][r].
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/quadenv.h"
#include "actor_core.h"
#include "brax_learner_arch.h"
#include "brax_learner_common.h"
#include "dispatch.h"
#include "learner_x3_common.h"

namespace quadenv {

int set_error(int code, const char* msg);  // quadenv.hip

namespace braxa {
namespace {

namespace x3 = lrn::x3;
using x3::X3;
using braxl::AdvNorm;
using braxl::Net;

constexpr int FCH = 4;  // k-steps per accumulator chain of layer 2 and dh1

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

// d act / d pre-activation times g, from the stored activation a (ReLU, tanh)
template <int ACTF>
__device__ __forceinline__ float dact(float a, float g) {
  return ACTF == QUAD_ACTFN_TANH ? g * (1.f - a * a) : (a > 0.f ? g : 0.f);
}
// SiLU's derivative from the pre-activation: sigma (1 + x (1 - sigma)); exp overflow (x < -88.7) gives sigma = 0 and 0
__device__ __forceinline__ float dsilu(float x) {
  const float sg = __fdiv_rn(1.f, 1.f + expf(-x));
  return sg * (1.f + x * (1.f - sg));
}

// rows [0, 32) of an LDS image (row stride `stride`, `width` floats a row, both multiples of 4) to `dst`, row-major
__device__ __forceinline__ void copy_out(const float* img, int stride, int width, float* dst) {
  const int w4 = width >> 2;
  for (int e = threadIdx.x; e < RND * w4; e += LB) {
    const int row = e / w4, c = e - row * w4;
    reinterpret_cast<float4*>(dst)[size_t(row) * w4 + c] = *reinterpret_cast<const float4*>(img + row * stride + 4 * c);
  }
}

// ---- launches 1 and 3: one net over the block's rounds. VALUE_ONLY (NOUT = 1): the forward and the head over all
// (L + 1) mb rows into values
template <int NOUT, int ACTF, bool VALUE_ONLY>
__device__ __forceinline__ void fwd_body(const Args& a, float* Lf, int blk) {
  constexpr int net = NOUT == NLOG ? 0 : 1;
  const braxl::Args& g0 = a.g;
  const Net& W = net == 0 ? g0.pi : g0.vf;
  const NetArgs& na = a.net[net];
  const int H1 = na.h1w, H2 = na.h2w, HS1 = H1 + 4, HS2 = H2 + 4;
  const int O_X = 0, O_H1 = RND * XS, O_H2 = O_H1 + RND * HS1, O_DH2 = O_H2 + RND * HS2;
  const int O_LOGIT = O_DH2 + RND * HS2, O_D = O_LOGIT + RND * 8, O_W3 = O_D + RND * 8, O_MS = O_W3 + 8 * H2;
  const int O_RED = O_MS + 64;
  const int tid = threadIdx.x, w = tid >> 6, r = tid & 31, h = (tid >> 5) & 1;
  const int nb1 = H1 >> 5, nb2 = H2 >> 5;

  AdvNorm an{0.f, 1.f};
  if constexpr (NOUT == NLOG) {
    double* const red0 = reinterpret_cast<double*>(Lf + O_RED);
    an = braxl::adv_norm(g0, red0, red0 + LB);
  }
  braxl::stage_norm(g0, Lf + O_MS);
  for (int i = tid; i < NOUT * H2; i += LB) Lf[O_W3 + i] = W.w2[i];  // flax [h2][NOUT]
  float b3[NOUT];
#pragma unroll
  for (int o = 0; o < NOUT; o++) b3[o] = W.b2[o];
  __syncthreads();

  // sums of the whole launch: thread (neuron hn, row group hf) of the dh2 phase; lanes 0 .. 31 of wave 0, one row each
  const int hn = tid & (H2 - 1), hf = tid / H2, nrg = LB / H2;
  float w3r[NOUT], dW3[NOUT], dB2 = 0.f;
#pragma unroll
  for (int o = 0; o < NOUT; o++) { w3r[o] = Lf[O_W3 + hn * NOUT + o]; dW3[o] = 0.f; }
  double db3[NOUT], st0 = 0.0, st1 = 0.0;  // float64: a lane adds one row of every round of the block
#pragma unroll
  for (int o = 0; o < NOUT; o++) db3[o] = 0.0;
  const float ce = g0.ent_cost * g0.inv_rows;

  // the first layer's pre-activation tile nb: h1^T block = W1^T x^T, K = 32 (features 21 .. 31 of A are zero)
  auto pre1 = [&](int nb) {
    f32x16 big, sm = zero16();
#pragma unroll
    for (int g = 0; g < 16; g++) big[g] = W.b0[32 * nb + acc_row(g, h)];
#pragma unroll
    for (int s = 0; s < 2; s++) {
      const X3 a1 = operand([&](int j) {
        const int f = 16 * s + 8 * h + j;
        return f < OBSB ? W.w0[f * H1 + 32 * nb + r] : 0.f;
      });
      const X3 xb = operand([&](int j) { return Lf[O_X + r * XS + 16 * s + 8 * h + j]; });
      x3::mma3s(a1, xb, big, sm);
    }
    big += sm;
    return big;
  };

  const int nrows = VALUE_ONLY ? g0.rows_all : g0.rows_loss;
  const int rounds = VALUE_ONLY ? (g0.rows_all + RND - 1) / RND : a.bp / RND;
  const int rpb = VALUE_ONLY ? a.rpbv : a.rpb;
  const int rd1 = min((blk + 1) * rpb, rounds);
  for (int rd = blk * rpb; rd < rd1; rd++) {
    const int q0 = rd * RND;
    // ---- the observation image: thread 4 row + c: features 8c .. 8c + 7; a row past the minibatch is all zero
    if (tid < 4 * RND) {
      const int row = tid >> 2, c = tid & 3, q = q0 + row;
      float v[8];
      braxl::gather_row8(g0, Lf + O_MS, q, nrows, 8 * c, v);
      const float4 lo = make_float4(v[0], v[1], v[2], v[3]), hi = make_float4(v[4], v[5], v[6], v[7]);
      float4* const xl = reinterpret_cast<float4*>(Lf + O_X + row * XS + 8 * c);
      xl[0] = lo;
      xl[1] = hi;
      if constexpr (net == 0) {
        float4* const xg = reinterpret_cast<float4*>(a.x) + size_t(q) * (XW / 4) + 2 * c;
        xg[0] = lo;
        xg[1] = hi;
      }
    }
    __syncthreads();
    // ---- layer 1
    for (int nb = w; nb < nb1; nb += 4) {
      const f32x16 p = pre1(nb);
#pragma unroll
      for (int g = 0; g < 16; g++) Lf[O_H1 + r * HS1 + 32 * nb + acc_row(g, h)] = actor::act1<ACTF>(p[g]);
    }
    __syncthreads();
    if constexpr (!VALUE_ONLY) copy_out(Lf + O_H1, HS1, H1, na.h1 + size_t(q0) * H1);
    // ---- layer 2: h2^T block mb = W2^T h1^T, K = H1
    for (int mb = w; mb < nb2; mb += 4) {
      f32x16 tot;
#pragma unroll
      for (int g = 0; g < 16; g++) tot[g] = W.b1[32 * mb + acc_row(g, h)];
      for (int s0 = 0; s0 < H1 / 16; s0 += FCH) {
        f32x16 big = zero16(), sm = zero16();
        const int s1 = min(s0 + FCH, H1 / 16);
        for (int s = s0; s < s1; s++) {
          const X3 a2 = operand([&](int j) { return W.w1[size_t(16 * s + 8 * h + j) * H2 + 32 * mb + r]; });
          const X3 b = operand([&](int j) { return Lf[O_H1 + r * HS1 + 16 * s + 8 * h + j]; });
          x3::mma3s(a2, b, big, sm);
        }
        tot += big + sm;
      }
#pragma unroll
      for (int g = 0; g < 16; g++) {
        const int o = r * HS2 + 32 * mb + acc_row(g, h);
        Lf[O_H2 + o] = actor::act1<ACTF>(tot[g]);
        if constexpr (ACTF == QUAD_ACTFN_SILU && !VALUE_ONLY) Lf[O_DH2 + o] = dsilu(tot[g]);
      }
    }
    __syncthreads();
    // ---- the head, in float64 and rounded once: thread 8 row + q sums neurons q, q + 8, .., the eight partial sums
    // are added in the order of q (learner_arch.hip: an f32 dot product over up to 256 neurons leaves about an ulp
    // of the output in every row's value, and the bias gradients keep it)
    {
      const int row = tid >> 3, q = tid & 7;
      const float* hrow = Lf + O_H2 + row * HS2;
      double p[NOUT];
#pragma unroll
      for (int o = 0; o < NOUT; o++) p[o] = 0.0;
      for (int n = q; n < H2; n += 8) {
        const double hv = hrow[n];
#pragma unroll
        for (int o = 0; o < NOUT; o++) p[o] = fma(hv, double(Lf[O_W3 + n * NOUT + o]), p[o]);
      }
      const int b = (tid & 63) & ~7;
#pragma unroll
      for (int o = 0; o < NOUT; o++) {
        double s = __shfl(p[o], b);
#pragma unroll
        for (int i = 1; i < 8; i++) s += __shfl(p[o], b + i);
        if (q == 0) Lf[O_LOGIT + row * 8 + o] = float(s + double(b3[o]));
      }
    }
    __syncthreads();
    if constexpr (VALUE_ONLY) {
      if (tid < RND && q0 + tid < nrows) {
        const float v = Lf[O_LOGIT + tid * 8];
        g0.values[q0 + tid] = v;
        if (g0.d_values) g0.d_values[q0 + tid] = v;
      }
      continue;  // the next round's first write to an image this round read comes after a barrier
    }
    // ---- per-row loss terms and dL/d(head output): wave 0, one row per lane
    if (tid < RND) {
      const int q = q0 + tid;
      float d[NOUT];
#pragma unroll
      for (int o = 0; o < NOUT; o++) d[o] = 0.f;
      if (q < g0.rows_loss) {
        if constexpr (NOUT == NLOG) {
          float s0 = 0.f, s1 = 0.f;
          braxl::policy_row_terms(g0, Lf + O_LOGIT + tid * 8, q, an, ce, d, s0, s1);
          st0 += s0;
          st1 += s1;
        } else {
          const float err = g0.vs[q] - g0.values[q];  // launch 1's bits of this row's v
          d[0] = -0.5f * err * g0.inv_rows;
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
    // ---- dh2 = act'(.) (d W3^T) -> DH2 image; dW3 and db2 per thread (neuron hn, rows hf, hf + nrg, ..)
    for (int row = hf; row < RND; row += nrg) {
      const float h2v = Lf[O_H2 + row * HS2 + hn];
      float g = 0.f;
#pragma unroll
      for (int o = 0; o < NOUT; o++) {
        const float dv = Lf[O_D + row * 8 + o];
        g = fmaf(dv, w3r[o], g);
        dW3[o] = fmaf(dv, h2v, dW3[o]);
      }
      float dh;
      if constexpr (ACTF == QUAD_ACTFN_SILU) dh = Lf[O_DH2 + row * HS2 + hn] * g;
      else dh = dact<ACTF>(h2v, g);
      Lf[O_DH2 + row * HS2 + hn] = dh;
      dB2 += dh;
    }
    __syncthreads();
    copy_out(Lf + O_DH2, HS2, H2, na.dh2 + size_t(q0) * H2);
    // ---- dh1^T block nb = act'(.) . (W2 dh2^T), K = H2, into the H1 image (h1 is in the workspace; ReLU and tanh
    // read the activation they overwrite, each element read and written by the same lane)
    for (int nb = w; nb < nb1; nb += 4) {
      f32x16 tot = zero16();
      for (int s0 = 0; s0 < H2 / 16; s0 += FCH) {  // H2 / 16 is 4, 8 or 16
        f32x16 big = zero16(), sm = zero16();
        for (int s = s0; s < s0 + FCH; s++) {
          const X3 av = operand([&](int j) { return W.w1[size_t(32 * nb + r) * H2 + 16 * s + 8 * h + j]; });
          const X3 bv = operand([&](int j) { return Lf[O_DH2 + r * HS2 + 16 * s + 8 * h + j]; });
          x3::mma3s(av, bv, big, sm);
        }
        tot += big + sm;
      }
      f32x16 p = zero16();
      if constexpr (ACTF == QUAD_ACTFN_SILU) p = pre1(nb);
#pragma unroll
      for (int g = 0; g < 16; g++) {
        const int o = O_H1 + r * HS1 + 32 * nb + acc_row(g, h);
        if constexpr (ACTF == QUAD_ACTFN_SILU) Lf[o] = dsilu(p[g]) * tot[g];
        else Lf[o] = dact<ACTF>(Lf[o], tot[g]);
      }
    }
    __syncthreads();
    copy_out(Lf + O_H1, HS1, H1, na.dh1 + size_t(q0) * H1);
    __syncthreads();  // the next round's staging and layer 1 overwrite the X and H1 images
  }
  if constexpr (VALUE_ONLY) return;
  __syncthreads();  // the sums below alias the H2 and DH2 images

  // ---- the block's sums
  float* const P = na.sp + size_t(blk) * sp_stride(H2);
  float* const S1 = Lf + O_H2;                                       // [256][9]
  double* const S2 = reinterpret_cast<double*>(Lf + O_H2 + LB * 9);  // [32][12]
#pragma unroll
  for (int o = 0; o < NOUT; o++) S1[tid * 9 + o] = dW3[o];
  S1[tid * 9 + 8] = dB2;
  if (tid < RND) {
#pragma unroll
    for (int o = 0; o < NOUT; o++) S2[tid * 12 + o] = db3[o];
    S2[tid * 12 + 8] = st0;
    S2[tid * 12 + 9] = st1;
  }
  __syncthreads();
  if (hf == 0) {  // the row groups of each neuron, in order
#pragma unroll
    for (int o = 0; o <= NOUT; o++) {
      const int c = o < NOUT ? o : 8;
      float s = S1[hn * 9 + c];
      for (int f = 1; f < nrg; f++) s += S1[(f * H2 + hn) * 9 + c];
      if (o < NOUT) P[sp_w3(H2) + hn * NLOG + o] = s;
      else P[hn] = s;
    }
  }
  if (tid < 10 && (tid < NOUT || tid >= 8)) {  // the 32 row lanes, in order
    double s = 0.0;
    for (int i = 0; i < RND; i++) s += S2[i * 12 + tid];
    if (tid < NOUT) P[sp_b3(H2) + tid] = float(s);
    else if (NOUT == NLOG) P[sp_st(H2) + (tid == 8 ? 0 : 2)] = float(s);
    else if (tid == 8) P[sp_st(H2) + 1] = float(s);
  }
}

template <int ACTF>
__global__ __launch_bounds__(LB) void k_brax_arch_value(Args a) {
  extern __shared__ __attribute__((aligned(16))) float lds_v[];
  fwd_body<1, ACTF, true>(a, lds_v, blockIdx.x);
}

template <int ACTF>
__global__ __launch_bounds__(LB) void k_brax_arch_fwd(Args a) {
  extern __shared__ __attribute__((aligned(16))) float lds_f[];
  if (blockIdx.y == 0)
    fwd_body<NLOG, ACTF, false>(a, lds_f, blockIdx.x);
  else
    fwd_body<1, ACTF, false>(a, lds_f, blockIdx.x);
}

// ---- launch 4: wave (net, split, tile); the policy's waves come first
__global__ __launch_bounds__(LB) void k_brax_arch_wgrad(Args a) {
  int wid = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int w0 = a.net[0].splits * a.net[0].tiles;
  const int net = wid < w0 ? 0 : 1;
  const NetArgs& na = a.net[net];
  if (net) wid -= w0;
  if (wid >= na.splits * na.tiles) return;
  const int sp = wid / na.tiles, t = wid - sp * na.tiles;
  const int H1 = na.h1w, H2 = na.h2w, nb2 = H2 >> 5;
  const int r = threadIdx.x & 31, h = (threadIdx.x >> 5) & 1;
  const int t2 = (H1 >> 5) * nb2;
  const bool w2 = t < t2;
  // out[m][n] = sum over rows of A[row][32 mblk + m] B[row][32 nblk + n]: dW2 [h1][h2] from h1 and dh2; dW1 | db1
  // [32][h1] from the x | 1 image and dh1
  const int mblk = w2 ? t / nb2 : 0, nblk = w2 ? t - mblk * nb2 : t - t2;
  const int wa = w2 ? H1 : XW, wb = w2 ? H2 : H1;
  const float* A = (w2 ? na.h1 : a.x) + 32 * mblk + r;
  const float* B = (w2 ? na.dh2 : na.dh1) + 32 * nblk + r;

  f32x16 tot = zero16();
  const int row1 = min(a.bp, (sp + 1) * na.rps);
  for (int c = sp * na.rps; c < row1; c += CHUNK) {
    f32x16 big = zero16(), sm = zero16();
#pragma unroll
    for (int s = 0; s < CHUNK / 16; s++) {
      const size_t k0 = size_t(c + 16 * s + 8 * h);
      const X3 av = operand([&](int j) { return A[(k0 + j) * wa]; });
      const X3 bv = operand([&](int j) { return B[(k0 + j) * wb]; });
      x3::mma3s(av, bv, big, sm);
      __builtin_amdgcn_sched_barrier(0);  // one k-step's operands live at a time
    }
    tot += big + sm;
  }
  float* const P = na.pb + size_t(sp) * pb_stride(H1, H2);
#pragma unroll
  for (int g = 0; g < 16; g++) {
    const int m = 32 * mblk + acc_row(g, h);
    if (w2) P[size_t(m) * H2 + 32 * nblk + r] = tot[g];
    else if (m < W1R) P[size_t(H1) * H2 + m * H1 + 32 * nblk + r] = tot[g];
  }
}

// ---- launch 5: element e of a net summed over the splits or the forward blocks in order (float64) into the
// gradient tensor that owns it; the three loss statistics
__global__ __launch_bounds__(256) void k_brax_arch_reduce(Args a) {
  const int net = blockIdx.y;
  const NetArgs& na = a.net[net];
  const int H1 = na.h1w, H2 = na.h2w;
  const int nout = net == 0 ? NLOG : 1;
  const int eb = pb_stride(H1, H2), e = blockIdx.x * 256 + threadIdx.x;
  if (e >= eb + sp_stride(H2)) return;
  const QuadBraxPPOGrads& g = a.gr;
  if (e < eb) {
    float* dst;
    if (e < H1 * H2) dst = (net ? g.vf_w1 : g.pi_w1) + e;
    else if (e < H1 * H2 + OBSB * H1) dst = (net ? g.vf_w0 : g.pi_w0) + (e - H1 * H2);
    else dst = (net ? g.vf_b0 : g.pi_b0) + (e - H1 * H2 - OBSB * H1);
    const float* p = na.pb + e;
    double s = 0.0;
    for (int k = 0; k < na.splits; k++) s += double(p[size_t(k) * eb]);
    *dst = float(s);
    return;
  }
  const int o = e - eb;
  int k = -1;
  if (o >= sp_w3(H2) && o < sp_b3(H2) && (o - sp_w3(H2)) % NLOG >= nout) return;
  if (o >= sp_b3(H2) && o < sp_st(H2) && o - sp_b3(H2) >= nout) return;
  if (o >= sp_st(H2)) {
    k = o - sp_st(H2);
    if (!a.stats || k > 2 || (k == 1) != (net == 1)) return;
  }
  const int sps = sp_stride(H2);
  const float* p = na.sp + o;
  double s = 0.0;
  for (int b = 0; b < a.nbk; b++) s += double(p[size_t(b) * sps]);
  if (o < sp_w3(H2)) { (net ? g.vf_b1 : g.pi_b1)[o] = float(s); return; }
  if (o < sp_b3(H2)) {
    const int i = o - sp_w3(H2), n = i / NLOG, c = i - n * NLOG;
    (net ? g.vf_w2 : g.pi_w2)[n * nout + c] = float(s);
    return;
  }
  if (o < sp_st(H2)) { (net ? g.vf_b2 : g.pi_b2)[o - sp_b3(H2)] = float(s); return; }
  a.stats[k] = float(k == 0 ? -s * a.inv_rows : (k == 1 ? 0.25 * s * a.inv_rows : -a.ent_cost * s * a.inv_rows));
}

int fail(const char* msg) { return set_error(QUAD_EINVAL, msg); }

bool misaligned(const void* p, uintptr_t al) { return (reinterpret_cast<uintptr_t>(p) & (al - 1)) != 0; }

// every arch launches with the widest member's LDS (LDS_MAX_BYTES): dispatch.h caches the opt-in per kernel, not per
// size, and the grid is at most one block per CU, so a narrow net loses nothing to the larger request
template <int ACTF>
hipError_t launch_value(const Layout& l, hipStream_t s, const Args& a) {
  return launch_lds<&k_brax_arch_value<ACTF>>(dim3(l.nbv), dim3(LB), LDS_MAX_BYTES, s, a);
}
template <int ACTF>
hipError_t launch_fwd(const Layout& l, hipStream_t s, const Args& a) {
  return launch_lds<&k_brax_arch_fwd<ACTF>>(dim3(l.nbk, 2), dim3(LB), LDS_MAX_BYTES, s, a);
}

}  // namespace
}  // namespace braxa
}  // namespace quadenv

using namespace quadenv;
using namespace quadenv::braxa;

extern "C" {

int64_t quad_brax_ppo_arch_workspace_bytes(const QuadBraxPPOParams* p, int32_t mb, int32_t L) {
  if (!in_family(p) || !in_limits(mb, L)) return 0;
  return layout_of(p->policy_h1, p->policy_h2, p->value_h1, p->value_h2, mb, L).bytes;
}

int quad_brax_ppo_arch_grad(const QuadBraxPPOParams* p, const QuadBraxPPOBatch* b, const QuadBraxPPOGrads* gr,
                            void* workspace, int64_t workspace_bytes, void* stream) {
  if (!p || !b || !gr || !workspace) return fail("quad_brax_ppo_arch_grad: NULL argument");
  if (!in_family(p))
    return fail("quad_brax_ppo_arch_grad: the family is policy and value nets (h1, h2), each h1 a multiple of 32 in "
                "[32, 512], each h2 in {64, 128, 256}, QUAD_ACTFN_RELU, QUAD_ACTFN_TANH or QUAD_ACTFN_SILU");
  const void* prm[] = {p->pi_w0, p->pi_b0, p->pi_w1, p->pi_b1, p->pi_w2, p->pi_b2, p->vf_w0, p->vf_b0,
                       p->vf_w1, p->vf_b1, p->vf_w2, p->vf_b2, p->mean,  p->std};
  for (const void* q : prm)
    if (!q || misaligned(q, 4)) return fail("quad_brax_ppo_arch_grad: a parameter pointer is NULL or misaligned");
  const void* grd[] = {gr->pi_w0, gr->pi_b0, gr->pi_w1, gr->pi_b1, gr->pi_w2, gr->pi_b2,
                       gr->vf_w0, gr->vf_b0, gr->vf_w1, gr->vf_b1, gr->vf_w2, gr->vf_b2};
  for (const void* q : grd)
    if (!q || misaligned(q, 4)) return fail("quad_brax_ppo_arch_grad: a gradient pointer is NULL or misaligned");
  const void* buf[] = {b->obs, b->next_obs, b->log_prob, b->reward, b->discount, b->truncation};
  for (const void* q : buf)
    if (!q || misaligned(q, 4)) return fail("quad_brax_ppo_arch_grad: an unroll buffer is NULL or misaligned");
  if (!b->raw || misaligned(b->raw, 16)) return fail("quad_brax_ppo_arch_grad: raw must be 16-byte aligned");
  if (!b->index || misaligned(b->index, 8)) return fail("quad_brax_ppo_arch_grad: index is NULL or misaligned");
  if (misaligned(b->entropy_noise, 16) || misaligned(b->noise_out, 16))
    return fail("quad_brax_ppo_arch_grad: entropy_noise and noise_out must be 16-byte aligned");
  if (misaligned(b->values, 4) || misaligned(b->vs, 4) || misaligned(b->advantages, 4) || misaligned(b->stats, 4))
    return fail("quad_brax_ppo_arch_grad: a diagnostic output is misaligned");
  if (misaligned(workspace, 16)) return fail("quad_brax_ppo_arch_grad: workspace must be 16-byte aligned");
  if (b->mb < 1) return fail("quad_brax_ppo_arch_grad: mb must be >= 1");
  if (b->L < 1 || b->L > braxl::MAX_L) return fail("quad_brax_ppo_arch_grad: L must be in [1, 64]");
  if (b->U < 1 || b->N < 1) return fail("quad_brax_ppo_arch_grad: U and N must be >= 1");
  if (!in_limits(b->mb, b->L)) return fail("quad_brax_ppo_arch_grad: L * mb must be <= 2^22");
  if (!(b->clipping_epsilon > 0.f)) return fail("quad_brax_ppo_arch_grad: clipping_epsilon must be > 0");
  const Layout l = layout_of(p->policy_h1, p->policy_h2, p->value_h1, p->value_h2, b->mb, b->L);
  if (workspace_bytes < l.bytes) return fail("quad_brax_ppo_arch_grad: workspace too small");

  char* const ws = static_cast<char*>(workspace);
  auto at = [&](int64_t o) { return reinterpret_cast<float*>(ws + o); };
  Args a{};
  braxl::Args& g = a.g;
  g.pi = braxl::Net{p->pi_w0, p->pi_b0, p->pi_w1, p->pi_b1, p->pi_w2, p->pi_b2};
  g.vf = braxl::Net{p->vf_w0, p->vf_b0, p->vf_w1, p->vf_b1, p->vf_w2, p->vf_b2};
  g.mean = p->mean; g.std = p->std; g.min_std = p->min_std;
  g.obs = b->obs; g.next_obs = b->next_obs; g.raw = b->raw; g.logp = b->log_prob; g.reward = b->reward;
  g.discount = b->discount; g.trunc = b->truncation; g.idx = b->index;
  g.noise = b->entropy_noise; g.noise_out = b->noise_out;
  g.d_values = b->values; g.d_vs = b->vs; g.d_adv = b->advantages;
  g.values = at(l.o_values); g.vs = at(l.o_vs); g.adv = at(l.o_adv);
  g.adv_part = reinterpret_cast<double*>(ws + l.o_adv_part);
  g.U = b->U; g.L = b->L; g.N = b->N; g.mb = b->mb;
  g.rows_loss = l.rows_loss; g.rows_all = l.rows_all; g.gae_blocks = l.gae_blocks;
  g.norm_adv = b->normalize_advantage != 0;
  g.clip = b->clipping_epsilon; g.ent_cost = b->entropy_cost; g.gamma = b->discounting; g.lam = b->gae_lambda;
  g.rscale = b->reward_scaling; g.inv_rows = 1.0f / float(l.rows_loss);
  g.noise_step = b->noise_step; g.seed = b->seed;
  a.gr = *gr;
  a.stats = b->stats;
  a.x = at(l.o_x);
  for (int n = 0; n < 2; n++) {
    const NetLayout& nl = l.net[n];
    a.net[n] = NetArgs{at(nl.o_h1), at(nl.o_dh2), at(nl.o_dh1), at(nl.o_sp), at(nl.o_pb),
                       nl.h1,       nl.h2,        nl.tiles,     nl.splits,   nl.rps};
  }
  a.bp = l.bp; a.nbk = l.nbk; a.rpb = l.rpb; a.nbv = l.nbv; a.rpbv = l.rpbv;
  a.inv_rows = 1.0 / double(l.rows_loss); a.ent_cost = double(b->entropy_cost);

  hipStream_t s = static_cast<hipStream_t>(stream);
  const int act = p->activation;
  hipError_t e = act == QUAD_ACTFN_TANH   ? launch_value<QUAD_ACTFN_TANH>(l, s, a)
                 : act == QUAD_ACTFN_SILU ? launch_value<QUAD_ACTFN_SILU>(l, s, a)
                                          : launch_value<QUAD_ACTFN_RELU>(l, s, a);
  if (e != hipSuccess) return set_error(QUAD_EHIP, "k_brax_arch_value launch failed");
  if (braxl::launch_gae(g, s) != hipSuccess) return set_error(QUAD_EHIP, "k_brax_gae launch failed");
  e = act == QUAD_ACTFN_TANH   ? launch_fwd<QUAD_ACTFN_TANH>(l, s, a)
      : act == QUAD_ACTFN_SILU ? launch_fwd<QUAD_ACTFN_SILU>(l, s, a)
                               : launch_fwd<QUAD_ACTFN_RELU>(l, s, a);
  if (e != hipSuccess) return set_error(QUAD_EHIP, "k_brax_arch_fwd launch failed");
  const int waves = l.net[0].splits * l.net[0].tiles + l.net[1].splits * l.net[1].tiles;
  hipLaunchKernelGGL(k_brax_arch_wgrad, dim3((waves + 3) / 4), dim3(LB), 0, s, a);
  if (hipGetLastError() != hipSuccess) return set_error(QUAD_EHIP, "k_brax_arch_wgrad launch failed");
  int elems = 0;
  for (int n = 0; n < 2; n++) {
    const int en = pb_stride(l.net[n].h1, l.net[n].h2) + sp_stride(l.net[n].h2);
    elems = en > elems ? en : elems;
  }
  hipLaunchKernelGGL(k_brax_arch_reduce, dim3((elems + 255) / 256, 2), dim3(256), 0, s, a);
  if (hipGetLastError() != hipSuccess) return set_error(QUAD_EHIP, "k_brax_arch_reduce launch failed");
  return QUAD_OK;
}

}  // extern "C"
