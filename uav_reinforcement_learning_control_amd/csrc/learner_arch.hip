// learner_arch.hip -- the PPO minibatch gradient of the general actor's family (quad_ppo_arch_grad): the gradient of
// ppo/ppo.py ppo_loss (quad_ppo_grad's semantics) for the policy net 12 -> H1 -> H2 -> 4 and the value net
// 12 -> H1 -> H2 -> 1, H1 a multiple of 32 up to 512, H2 in {64, 128, 256}, ReLU or tanh, rows gathered through the
// minibatch index. Launches on the caller's stream, no host synchronisation:
//
//   k_arch_adv_stats  normalize_advantage == 1 only: learner.h adv_stats_block                    -> workspace sums
//   k_arch_fwd        block (b, net): the net over rounds of 32 rows -- forward, learner.h row_terms, dL/d(head),
//                     dh2, dh1; the x, h1, dh2, dh1 images of every row                           -> workspace images;
//                     dW3, db2, db3, the log_std gradient and the loss sums of the block's rows    -> per-block sums
//   k_arch_wgrad      wave (net, split, tile): one 32 x 32 tile of dW2 = dh2^T h1 or of dW1 | db1 = dh1^T [x | 1]
//                     over the split's rows in index order                                        -> per-split images
//   k_arch_reduce     the splits and the blocks in order, in float64                              -> gradients, stats
//
// A block cannot keep a whole dW2 in accumulators as k_brax_grad does (512 x 256 floats = 512 registers per lane), so
// the weight gradients are output-stationary products over the stored images: a tile's sum runs over the minibatch
// positions in a fixed order whatever the rows are, which makes the gradient bit-identical from run to run and under
// a physical reordering of the rows into index order. No atomics.
//
// Every matrix product (layer 1, layer 2, dh1, dW2, dW1) runs on v_mfma_f32_32x32x16_bf16 over three-piece bf16
// splits of both operands (learner_x3_common.h split8 / mma3s), big and small terms in separate accumulators; an
// accumulator chain is at most four k-steps long and is then added to a VALU
// total (learner_x3.hip: long MFMA chains drift by the instruction's truncation). The 1.0 in column 12 of the
// observation image makes column 12 of the dW1 tile the first layer's bias gradient. The head, the loss terms, dh2,
// dW3 and the bias sums are f32 VALU work in a fixed order. tanh is actor_core.h tanh_f32 (the forward kernels'),
// its derivative 1 - h^2 from the stored activation.
//
// MFMA maps (brax_learner.hip): lane l, r = l & 31, h = l >> 5; operand element j of A is A[r][8h + j], of B is
// B[8h + j][r]; accumulator register g is D[acc_row(g, h)][r].
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/quadenv.h"
#include "actor_core.h"
#include "dispatch.h"
#include "learner_arch.h"
#include "learner_x3_common.h"

namespace quadenv {

int set_error(int code, const char* msg);  // quadenv.hip

namespace lrna {
namespace {

namespace x3 = lrn::x3;
using x3::X3;

constexpr int XS = 20;  // LDS observation image row: XW + 4 pad
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

template <int ACTF>
__device__ __forceinline__ float act(float x) {
  return ACTF == QUAD_ACTFN_TANH ? actor::tanh_f32(x) : relu(x);
}
// d act / d pre-activation from the stored activation a
template <int ACTF>
__device__ __forceinline__ float dact(float a, float g) {
  return ACTF == QUAD_ACTFN_TANH ? g * (1.f - a * a) : (a > 0.f ? g : 0.f);
}

// rows [0, 32) of an LDS image (row stride `stride`, `width` floats a row, both multiples of 4) to `dst`, row-major
__device__ __forceinline__ void copy_out(const float* img, int stride, int width, float* dst) {
  const int w4 = width >> 2;
  for (int e = threadIdx.x; e < RND * w4; e += LB) {
    const int row = e / w4, c = e - row * w4;
    reinterpret_cast<float4*>(dst)[size_t(row) * w4 + c] = *reinterpret_cast<const float4*>(img + row * stride + 4 * c);
  }
}

__global__ __launch_bounds__(256) void k_arch_adv_stats(const float* __restrict__ adv, const int64_t* __restrict__ idx,
                                                        int batch, double* __restrict__ part) {
  __shared__ double red[2][256];
  lrn::adv_stats_block(adv, idx, batch, part, blockIdx.x, red);
}

// ---- the forward launch: one net over the block's rounds
template <int NOUT, int ACTF>
__device__ __forceinline__ void fwd_body(const Args& a, float* Lf, int blk) {
  const int net = NOUT == ACT ? 0 : 1;
  const lrn::NetW& W = NOUT == ACT ? a.g.actor : a.g.critic;
  const int H1 = a.h1w, H2 = a.h2w, HS1 = H1 + 4, HS2 = H2 + 4;
  const int O_X = 0, O_H1 = RND * XS, O_H2 = O_H1 + RND * HS1, O_DH2 = O_H2 + RND * HS2;
  const int O_LOGIT = O_DH2 + RND * HS2, O_D = O_LOGIT + RND * 4, O_W3 = O_D + RND * 4, O_RED = O_W3 + 4 * H2;
  const int tid = threadIdx.x, w = tid >> 6, r = tid & 31, h = (tid >> 5) & 1;
  const int nb1 = H1 >> 5, nb2 = H2 >> 5;

  double* const red0 = reinterpret_cast<double*>(Lf + O_RED);
  const lrn::AdvNorm an = lrn::adv_norm<NOUT>(a.g, red0, red0 + LB);
  for (int i = tid; i < NOUT * H2; i += LB) Lf[O_W3 + i] = W.w2[i];
  float b3[NOUT], ls[ACT], isd[ACT];
#pragma unroll
  for (int o = 0; o < NOUT; o++) b3[o] = W.b2[o];
#pragma unroll
  for (int k = 0; k < ACT; k++) { ls[k] = 0.f; isd[k] = 1.f; }
  if constexpr (NOUT == ACT) {
#pragma unroll
    for (int k = 0; k < ACT; k++) { ls[k] = a.g.log_std[k]; isd[k] = 1.f / expf(ls[k]); }
  }
  __syncthreads();

  // sums of the whole launch: thread (neuron hn, row group hf) of the dh2 phase; lanes 0 .. 31 of wave 0, one row each
  const int hn = tid & (H2 - 1), hf = tid / H2, nrg = LB / H2;
  float w3r[NOUT], dW3[NOUT], dB2 = 0.f;
#pragma unroll
  for (int o = 0; o < NOUT; o++) { w3r[o] = Lf[O_W3 + o * H2 + hn]; dW3[o] = 0.f; }
  double db3[NOUT], dls[ACT], st[3] = {0.0, 0.0, 0.0};  // float64: a lane adds one row of every round of the block
#pragma unroll
  for (int o = 0; o < NOUT; o++) db3[o] = 0.0;
#pragma unroll
  for (int k = 0; k < ACT; k++) dls[k] = 0.0;

  float* const gh1 = a.h1 + size_t(net) * a.bp * H1;
  float* const gdh1 = a.dh1 + size_t(net) * a.bp * H1;
  float* const gdh2 = a.dh2 + size_t(net) * a.bp * H2;

  const int rd1 = min((blk + 1) * a.rpb, a.bp / RND);
  for (int rd = blk * a.rpb; rd < rd1; rd++) {
    const int q0 = rd * RND;
    // ---- the observation image: thread 4 row + c: features 4c .. 4c + 3 (c = 3: the 1.0 column and zeros); a row
    // past the minibatch is all zero
    if (tid < 4 * RND) {
      const int row = tid >> 2, c = tid & 3, q = q0 + row;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (q < a.g.batch) {
        if (c < 3) v = reinterpret_cast<const float4*>(a.g.obs)[size_t(a.g.idx[q]) * 3 + c];
        else v.x = 1.f;
      }
      *reinterpret_cast<float4*>(Lf + O_X + row * XS + 4 * c) = v;
      if (net == 0) reinterpret_cast<float4*>(a.x)[size_t(q) * 4 + c] = v;
    }
    __syncthreads();
    // ---- layer 1: h1^T block nb = W1 x^T, K = 16 (features 12 .. 15 of A are zero)
    {
      const X3 xb = operand([&](int j) { return Lf[O_X + r * XS + 8 * h + j]; });
      for (int nb = w; nb < nb1; nb += 4) {
        const X3 a1 = operand([&](int j) {
          const int f = 8 * h + j;
          return f < OBS ? W.w0[(32 * nb + r) * OBS + f] : 0.f;
        });
        f32x16 big, sm = zero16();
#pragma unroll
        for (int g = 0; g < 16; g++) big[g] = W.b0[32 * nb + acc_row(g, h)];
        x3::mma3s(a1, xb, big, sm);
        big += sm;
#pragma unroll
        for (int g = 0; g < 16; g++) Lf[O_H1 + r * HS1 + 32 * nb + acc_row(g, h)] = act<ACTF>(big[g]);
      }
    }
    __syncthreads();
    copy_out(Lf + O_H1, HS1, H1, gh1 + size_t(q0) * H1);
    // ---- layer 2: h2^T block mb = W2 h1^T, K = H1
    for (int mb = w; mb < nb2; mb += 4) {
      f32x16 tot;
#pragma unroll
      for (int g = 0; g < 16; g++) tot[g] = W.b1[32 * mb + acc_row(g, h)];
      for (int s0 = 0; s0 < H1 / 16; s0 += FCH) {
        f32x16 big = zero16(), sm = zero16();
        const int s1 = min(s0 + FCH, H1 / 16);
        for (int s = s0; s < s1; s++) {
          const X3 a2 = operand([&](int j) { return W.w1[size_t(32 * mb + r) * H1 + 16 * s + 8 * h + j]; });
          const X3 b = operand([&](int j) { return Lf[O_H1 + r * HS1 + 16 * s + 8 * h + j]; });
          x3::mma3s(a2, b, big, sm);
        }
        tot += big + sm;
      }
#pragma unroll
      for (int g = 0; g < 16; g++) Lf[O_H2 + r * HS2 + 32 * mb + acc_row(g, h)] = act<ACTF>(tot[g]);
    }
    __syncthreads();
    // ---- the head, in float64 and rounded once: thread 8 row + q sums neurons q, q + 8, .., the eight partial sums
    // are added in the order of q. An f32 dot product over up to 256 neurons leaves about an ulp of the output in
    // every row's value, and the bias gradients (means of value - return over the rows) keep it
    {
      const int row = tid >> 3, q = tid & 7;
      const float* hrow = Lf + O_H2 + row * HS2;
      double p[NOUT];
#pragma unroll
      for (int o = 0; o < NOUT; o++) p[o] = 0.0;
      for (int n = q; n < H2; n += 8) {
        const double hv = hrow[n];
#pragma unroll
        for (int o = 0; o < NOUT; o++) p[o] = fma(hv, double(Lf[O_W3 + o * H2 + n]), p[o]);
      }
      const int b = (tid & 63) & ~7;
#pragma unroll
      for (int o = 0; o < NOUT; o++) {
        double s = __shfl(p[o], b);
#pragma unroll
        for (int i = 1; i < 8; i++) s += __shfl(p[o], b + i);
        if (q == 0) Lf[O_LOGIT + row * 4 + o] = float(s + double(b3[o]));
      }
    }
    __syncthreads();
    // ---- per-row loss terms and dL/d(head output): wave 0, one row per lane
    if (tid < RND) {
      const int q = q0 + tid;
      const bool valid = q < a.g.batch;
      alignas(16) float sc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (valid) {
        const int64_t row = a.g.idx[q];
        if constexpr (NOUT == ACT) {
          const float4 a4 = reinterpret_cast<const float4*>(a.g.act)[row];
          sc[0] = a4.x; sc[1] = a4.y; sc[2] = a4.z; sc[3] = a4.w;
          sc[4] = a.g.logp_old[row];
          sc[5] = a.g.adv[row];
        } else {
          sc[6] = a.g.ret[row];
        }
      }
      float out[NOUT];
#pragma unroll
      for (int o = 0; o < NOUT; o++) out[o] = Lf[O_LOGIT + tid * 4 + o];
      const lrn::RowTerms<NOUT> rt = lrn::row_terms<NOUT>(a.g, out, sc, ls, isd, an, valid);
      if (valid) {
        if constexpr (NOUT == ACT) {
          st[0] += rt.pg;
          st[2] += rt.clipped;
#pragma unroll
          for (int k = 0; k < ACT; k++) dls[k] += rt.dlp * (rt.z[k] * rt.z[k] - 1.f);
        } else {
          st[1] += rt.diff * rt.diff;
        }
      }
#pragma unroll
      for (int o = 0; o < NOUT; o++) {
        Lf[O_D + tid * 4 + o] = rt.dd[o];
        db3[o] += rt.dd[o];
      }
    }
    __syncthreads();
    // ---- dh2 = act'(h2) (d W3) -> DH2 image; dW3 and db2 per thread (neuron hn, rows hf, hf + nrg, ..)
    for (int row = hf; row < RND; row += nrg) {
      const float h2v = Lf[O_H2 + row * HS2 + hn];
      float g = 0.f;
#pragma unroll
      for (int o = 0; o < NOUT; o++) {
        const float dv = Lf[O_D + row * 4 + o];
        g = fmaf(dv, w3r[o], g);
        dW3[o] = fmaf(dv, h2v, dW3[o]);
      }
      const float dh = dact<ACTF>(h2v, g);
      Lf[O_DH2 + row * HS2 + hn] = dh;
      dB2 += dh;
    }
    __syncthreads();
    copy_out(Lf + O_DH2, HS2, H2, gdh2 + size_t(q0) * H2);
    // ---- dh1^T block nb = act'(h1) . (W2^T dh2^T), K = H2, over the H1 image in place (h1 is in the workspace, and
    // each element is read and written by the same lane)
    for (int nb = w; nb < nb1; nb += 4) {
      f32x16 tot = zero16();
      for (int s0 = 0; s0 < H2 / 16; s0 += FCH) {  // H2 / 16 is 4, 8 or 16
        f32x16 big = zero16(), sm = zero16();
        for (int s = s0; s < s0 + FCH; s++) {
          const X3 av = operand([&](int j) { return W.w1[size_t(16 * s + 8 * h + j) * H1 + 32 * nb + r]; });
          const X3 bv = operand([&](int j) { return Lf[O_DH2 + r * HS2 + 16 * s + 8 * h + j]; });
          x3::mma3s(av, bv, big, sm);
        }
        tot += big + sm;
      }
#pragma unroll
      for (int g = 0; g < 16; g++) {
        const int o = O_H1 + r * HS1 + 32 * nb + acc_row(g, h);
        Lf[o] = dact<ACTF>(Lf[o], tot[g]);
      }
    }
    __syncthreads();
    copy_out(Lf + O_H1, HS1, H1, gdh1 + size_t(q0) * H1);
  }
  __syncthreads();  // the sums below alias the H2 and DH2 images

  // ---- the block's sums
  float* const P = a.sp + size_t(net * a.nbk + blk) * sp_stride(H2);
  float* const S1 = Lf + O_H2;            // [256][5]
  double* const S2 = reinterpret_cast<double*>(Lf + O_H2 + LB * 5);  // [32][12]
#pragma unroll
  for (int o = 0; o < NOUT; o++) S1[tid * 5 + o] = dW3[o];
  S1[tid * 5 + 4] = dB2;
  if (tid < RND) {
#pragma unroll
    for (int o = 0; o < NOUT; o++) S2[tid * 12 + o] = db3[o];
#pragma unroll
    for (int k = 0; k < ACT; k++) S2[tid * 12 + 4 + k] = dls[k];
#pragma unroll
    for (int k = 0; k < 3; k++) S2[tid * 12 + 8 + k] = st[k];
  }
  __syncthreads();
  if (hf == 0) {  // the row groups of each neuron, in order
#pragma unroll
    for (int o = 0; o <= NOUT; o++) {
      const int c = o < NOUT ? o : 4;
      float s = S1[hn * 5 + c];
      for (int f = 1; f < nrg; f++) s += S1[(f * H2 + hn) * 5 + c];
      if (o < NOUT) P[sp_w3(H2) + o * H2 + hn] = s;
      else P[hn] = s;
    }
  }
  if (tid < 11 && (tid < NOUT || tid >= 4)) {  // the 32 row lanes, in order
    double s = 0.0;
    for (int i = 0; i < RND; i++) s += S2[i * 12 + tid];
    P[sp_b3(H2) + tid] = float(s);
  }
}

template <int ACTF>
__global__ __launch_bounds__(LB) void k_arch_fwd(Args a) {
  extern __shared__ __attribute__((aligned(16))) float lds_f[];
  if (blockIdx.y == 0)
    fwd_body<ACT, ACTF>(a, lds_f, blockIdx.x);
  else
    fwd_body<1, ACTF>(a, lds_f, blockIdx.x);
}

// A member's table entry (population.h) holds the epoch's bases; the launch of minibatch `slot` moves the index
// slice, the advantage sums and the statistics row to it, as k_pop_ppo_grad_x3_sep and k_pop_ppo_reduce do
__device__ __forceinline__ Args pop_args(const Args* __restrict__ tab, int32_t m, int32_t slot) {
  Args a = tab[m];
  a.g.idx += size_t(slot) * size_t(a.g.batch);
  if (a.g.adv_part) a.g.adv_part += size_t(slot) * QUAD_ADV_SUM_DOUBLES;
  if (a.stats) a.stats += 4 * size_t(slot);
  return a;
}

// the population form (population.h): block (b, net, k) is block (b, net) of member active[k]'s launch
template <int ACTF>
__global__ __launch_bounds__(LB) void k_pop_arch_fwd(const Args* __restrict__ tab, const int32_t* __restrict__ active,
                                                     int32_t slot) {
  extern __shared__ __attribute__((aligned(16))) float lds_f[];
  const Args a = pop_args(tab, active[blockIdx.z], slot);
  if (blockIdx.y == 0)
    fwd_body<ACT, ACTF>(a, lds_f, blockIdx.x);
  else
    fwd_body<1, ACTF>(a, lds_f, blockIdx.x);
}

// ---- the weight-gradient launch: wave (net, split, tile)
__device__ __forceinline__ void wgrad_body(const Args& a) {
  const int wid = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int per_net = a.splits * a.tiles;
  if (wid >= 2 * per_net) return;
  const int net = wid / per_net, rem = wid - net * per_net, sp = rem / a.tiles, t = rem - sp * a.tiles;
  const int H1 = a.h1w, H2 = a.h2w, nb1 = H1 >> 5;
  const int r = threadIdx.x & 31, h = (threadIdx.x >> 5) & 1;
  const int t2 = (H2 >> 5) * nb1;
  const bool w2 = t < t2;
  // out[m][n] = sum over rows of A[row][32 mblk + m] B[row][32 nblk + n]
  const int mblk = w2 ? t / nb1 : t - t2, nblk = w2 ? t - mblk * nb1 : 0;
  const int wa = w2 ? H2 : H1, wb = w2 ? H1 : XW;
  const float* A = (w2 ? a.dh2 + size_t(net) * a.bp * H2 : a.dh1 + size_t(net) * a.bp * H1) + 32 * mblk + r;
  const float* B = (w2 ? a.h1 + size_t(net) * a.bp * H1 + 32 * nblk : a.x) + (r < wb ? r : 0);
  const bool bcol = r < wb;  // the observation image has 16 columns

  f32x16 tot = zero16();
  const int row1 = min(a.bp, (sp + 1) * a.rps);
  for (int c = sp * a.rps; c < row1; c += CHUNK) {
    f32x16 big = zero16(), sm = zero16();
#pragma unroll
    for (int s = 0; s < CHUNK / 16; s++) {
      const size_t k0 = size_t(c + 16 * s + 8 * h);
      const X3 av = operand([&](int j) { return A[(k0 + j) * wa]; });
      const X3 bv = operand([&](int j) { return bcol ? B[(k0 + j) * wb] : 0.f; });
      x3::mma3s(av, bv, big, sm);
      __builtin_amdgcn_sched_barrier(0);  // one k-step's operands live at a time
    }
    tot += big + sm;
  }
  float* const P = a.pb + size_t(net * a.splits + sp) * pb_stride(H1, H2);
#pragma unroll
  for (int g = 0; g < 16; g++) {
    const int m = 32 * mblk + acc_row(g, h);
    if (w2) P[size_t(m) * H1 + 32 * nblk + r] = tot[g];
    else if (r < XW) P[size_t(H2) * H1 + m * XW + r] = tot[g];
  }
}

__global__ __launch_bounds__(LB) void k_arch_wgrad(Args a) { wgrad_body(a); }

// the population form: block (b, k) is block b of member active[k]'s launch
__global__ __launch_bounds__(LB) void k_pop_arch_wgrad(const Args* __restrict__ tab, const int32_t* __restrict__ active,
                                                       int32_t slot) {
  wgrad_body(pop_args(tab, active[blockIdx.y], slot));
}

// ---- the reduction: element e of a net summed over the splits or the forward blocks in order (float64) into the
// gradient tensor that owns it; the four loss statistics
__device__ __forceinline__ void reduce_body(const Args& a) {
  const int net = blockIdx.y, H1 = a.h1w, H2 = a.h2w;
  const int nout = net == 0 ? ACT : 1;
  const int eb = pb_stride(H1, H2), e = blockIdx.x * 256 + threadIdx.x;
  if (e >= eb + sp_stride(H2)) return;
  const QuadPolicyGrads& g = a.gr;
  if (e < eb) {
    float* dst;
    if (e < H2 * H1) {
      dst = (net ? g.vf_w1 : g.pi_w1) + e;
    } else {
      const int o = e - H2 * H1, n = o / XW, f = o - n * XW;
      if (f > OBS) return;
      dst = f < OBS ? (net ? g.vf_w0 : g.pi_w0) + n * OBS + f : (net ? g.vf_b0 : g.pi_b0) + n;
    }
    const float* p = a.pb + size_t(net) * a.splits * eb + e;
    double s = 0.0;
    for (int k = 0; k < a.splits; k++) s += double(p[size_t(k) * eb]);
    *dst = float(s);
    return;
  }
  const int o = e - eb;
  if (o >= sp_w3(H2) && o < sp_b3(H2) && o - sp_w3(H2) >= nout * H2) return;
  if (o >= sp_b3(H2) && o < sp_ls(H2) && o - sp_b3(H2) >= nout) return;
  if (o >= sp_ls(H2) && o < sp_st(H2) && net != 0) return;
  if (o >= sp_st(H2)) {
    const int k = o - sp_st(H2);
    if (!a.stats || k > 3 || (k == 1) != (net == 1)) return;
    if (k == 3) {  // the entropy of the state-independent Gaussian
      float en = 0.f;
      for (int i = 0; i < ACT; i++) en += 0.5f + 0.91893853320467274f + a.g.log_std[i];
      a.stats[2] = en;
      return;
    }
  }
  const int sps = sp_stride(H2);
  const float* p = a.sp + size_t(net) * a.nbk * sps + o;
  double sd = 0.0;
  for (int b = 0; b < a.nbk; b++) sd += double(p[size_t(b) * sps]);
  const float s = float(sd);
  if (o < sp_w3(H2)) { (net ? g.vf_b1 : g.pi_b1)[o] = s; return; }
  if (o < sp_b3(H2)) { (net ? g.val_w : g.act_w)[o - sp_w3(H2)] = s; return; }
  if (o < sp_ls(H2)) { (net ? g.val_b : g.act_b)[o - sp_b3(H2)] = s; return; }
  if (o < sp_st(H2)) { g.log_std[o - sp_ls(H2)] = s - a.ent_coef; return; }  // + d(-ent_coef * entropy)
  const int k = o - sp_st(H2);
  if (k == 0) a.stats[0] = s * a.g.inv_batch;
  else if (k == 1) a.stats[1] = s * a.g.inv_batch;
  else a.stats[3] = s * a.g.inv_batch;
}

__global__ __launch_bounds__(256) void k_arch_reduce(Args a) { reduce_body(a); }

// the population form: block (b, net, k) is block (b, net) of member active[k]'s launch
__global__ __launch_bounds__(256) void k_pop_arch_reduce(const Args* __restrict__ tab,
                                                         const int32_t* __restrict__ active, int32_t slot) {
  reduce_body(pop_args(tab, active[blockIdx.z], slot));
}

int fail(const char* msg) { return set_error(QUAD_EINVAL, msg); }

bool bad(const void* p, uintptr_t al) { return !p || (reinterpret_cast<uintptr_t>(p) & (al - 1)) != 0; }

template <int ACTF>
hipError_t launch_fwd(const Layout& l, hipStream_t s, const Args& a) {
  // every arch launches with the widest member's LDS (144,384 B): dispatch.h caches the opt-in per kernel, not per
  // size, and the grid is at most one block per CU, so a narrow net loses nothing to the larger request
  static_assert(RND * 20 + RND * 516 + 2 * RND * 260 + 2 * RND * 4 + 4 * 256 + 4 * LB <= 160 * 1024 / 4, "LDS budget");
  return launch_lds<&k_arch_fwd<ACTF>>(dim3(l.nbk, 2), dim3(LB), layout_of(512, 256, 1).lds_bytes, s, a);
}

// the workspace images and the block / split-K layout of an arch and a batch
void set_layout(Args& a, const QuadActorArch& arch, const Layout& l, char* ws) {
  a.x = reinterpret_cast<float*>(ws + l.o_x);
  a.h1 = reinterpret_cast<float*>(ws + l.o_h1);
  a.dh2 = reinterpret_cast<float*>(ws + l.o_dh2);
  a.dh1 = reinterpret_cast<float*>(ws + l.o_dh1);
  a.sp = reinterpret_cast<float*>(ws + l.o_sp);
  a.pb = reinterpret_cast<float*>(ws + l.o_pb);
  a.h1w = arch.h1; a.h2w = arch.h2; a.bp = l.bp; a.nbk = l.nbk; a.rpb = l.rpb;
  a.tiles = l.tiles; a.splits = l.splits; a.rps = l.rps;
}

template <int ACTF>
hipError_t launch_pop_fwd(const Layout& l, hipStream_t s, const Args* tab, const int32_t* active, int count, int slot) {
  return launch_lds<&k_pop_arch_fwd<ACTF>>(dim3(l.nbk, 2, count), dim3(LB), layout_of(512, 256, 1).lds_bytes, s, tab,
                                           active, slot);
}

}  // namespace

// ---- the population launches of this file's kernels (population.h)
Args pop_entry(const QuadActorArch& arch, const lrn::GArgs& g, const QuadPopMember& m, int32_t batch) {
  Args a{};
  a.g = g;
  a.gr = m.grads;
  a.stats = m.mb_stats;
  a.ent_coef = m.ent_coef;
  set_layout(a, arch, layout_of(arch.h1, arch.h2, batch), static_cast<char*>(m.workspace));
  return a;
}

int launch_pop_grad(const QuadActorArch& arch, int32_t batch, const Args* tab, const int32_t* active, int count,
                    int slot, hipStream_t s) {
  const Layout l = layout_of(arch.h1, arch.h2, batch);
  const hipError_t e = arch.activation == QUAD_ACTFN_TANH
                           ? launch_pop_fwd<QUAD_ACTFN_TANH>(l, s, tab, active, count, slot)
                           : launch_pop_fwd<QUAD_ACTFN_RELU>(l, s, tab, active, count, slot);
  if (e != hipSuccess) return set_error(QUAD_EHIP, "k_pop_arch_fwd launch failed");
  hipLaunchKernelGGL(k_pop_arch_wgrad, dim3((2 * l.splits * l.tiles + 3) / 4, count), dim3(LB), 0, s, tab, active, slot);
  if (hipGetLastError() != hipSuccess) return set_error(QUAD_EHIP, "k_pop_arch_wgrad launch failed");
  const int elems = pb_stride(arch.h1, arch.h2) + sp_stride(arch.h2);
  hipLaunchKernelGGL(k_pop_arch_reduce, dim3((elems + 255) / 256, 2, count), dim3(256), 0, s, tab, active, slot);
  if (hipGetLastError() != hipSuccess) return set_error(QUAD_EHIP, "k_pop_arch_reduce launch failed");
  return QUAD_OK;
}

}  // namespace lrna
}  // namespace quadenv

using namespace quadenv;
using namespace quadenv::lrna;

extern "C" {

int64_t quad_ppo_arch_workspace_bytes(const QuadActorArch* arch, int32_t batch) {
  if (!in_family(arch) || batch < 1 || batch > MAX_BATCH) return 0;
  return layout_of(arch->h1, arch->h2, batch).bytes;
}

int quad_ppo_arch_grad(const QuadActorArch* arch, const QuadPolicyParams* p, const QuadPPOBatch* b,
                       const QuadPolicyGrads* gr, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!arch || !p || !b || !gr || !workspace) return fail("quad_ppo_arch_grad: NULL argument");
  if (!in_family(arch))
    return fail("quad_ppo_arch_grad: the family is h1 a multiple of 32 in [32, 512], h2 in {64, 128, 256}, "
                "QUAD_ACTFN_RELU or QUAD_ACTFN_TANH");
  const void* prm[] = {p->pi_w0, p->pi_b0, p->pi_w1, p->pi_b1, p->act_w, p->act_b, p->vf_w0,
                       p->vf_b0, p->vf_w1, p->vf_b1, p->val_w, p->val_b, p->log_std};
  for (const void* q : prm)
    if (bad(q, 4)) return fail("quad_ppo_arch_grad: a policy parameter pointer is NULL or misaligned");
  const void* grd[] = {gr->pi_w0, gr->pi_b0, gr->pi_w1, gr->pi_b1, gr->act_w, gr->act_b, gr->vf_w0,
                       gr->vf_b0, gr->vf_w1, gr->vf_b1, gr->val_w, gr->val_b, gr->log_std};
  for (const void* q : grd)
    if (bad(q, 4)) return fail("quad_ppo_arch_grad: a gradient pointer is NULL or misaligned");
  if (bad(b->obs, 16) || bad(b->actions, 16)) return fail("quad_ppo_arch_grad: obs and actions must be 16-byte aligned");
  if (bad(b->log_prob, 4) || bad(b->advantages, 4) || bad(b->returns, 4) || bad(b->index, 8))
    return fail("quad_ppo_arch_grad: a minibatch buffer is NULL or misaligned");
  if (b->stats && bad(b->stats, 4)) return fail("quad_ppo_arch_grad: stats is misaligned");
  if (bad(workspace, 16)) return fail("quad_ppo_arch_grad: workspace must be 16-byte aligned");
  if (b->batch < 1 || b->batch > MAX_BATCH) return fail("quad_ppo_arch_grad: batch must be in [1, 2^22]");
  if (!(b->clip_range > 0.f)) return fail("quad_ppo_arch_grad: clip_range must be > 0");
  const int na = b->normalize_advantage;
  if (na != 0 && na != 1 && na != QUAD_ADV_GIVEN)
    return fail("quad_ppo_arch_grad: normalize_advantage must be 0, 1 or QUAD_ADV_GIVEN");
  const bool norm = na != 0 && b->batch > 1;
  if (norm && na == QUAD_ADV_GIVEN && bad(b->adv_sums, 8)) return fail("quad_ppo_arch_grad: QUAD_ADV_GIVEN needs adv_sums");
  const Layout l = layout_of(arch->h1, arch->h2, b->batch);
  if (workspace_bytes < l.bytes) return fail("quad_ppo_arch_grad: workspace too small");

  char* const ws = static_cast<char*>(workspace);
  Args a{};
  lrn::GArgs& g = a.g;
  g.actor = lrn::NetW{p->pi_w0, p->pi_b0, p->pi_w1, p->pi_b1, p->act_w, p->act_b};
  g.critic = lrn::NetW{p->vf_w0, p->vf_b0, p->vf_w1, p->vf_b1, p->val_w, p->val_b};
  g.log_std = p->log_std;
  g.obs = b->obs; g.act = b->actions; g.logp_old = b->log_prob; g.adv = b->advantages; g.ret = b->returns;
  g.idx = b->index;
  double* const adv_part = na == QUAD_ADV_GIVEN ? const_cast<double*>(b->adv_sums) : reinterpret_cast<double*>(ws + l.o_adv);
  g.adv_part = norm ? adv_part : nullptr;
  g.batch = b->batch;
  g.clip = b->clip_range; g.inv_batch = 1.0f / float(b->batch); g.vf_coef = b->vf_coef;
  a.gr = *gr;
  a.stats = b->stats;
  a.ent_coef = b->ent_coef;
  set_layout(a, *arch, l, ws);

  hipStream_t s = static_cast<hipStream_t>(stream);
  if (norm && na == 1) {
    hipLaunchKernelGGL(k_arch_adv_stats, dim3(lrn::ADV_BLOCKS), dim3(256), 0, s, b->advantages, b->index, b->batch, adv_part);
    if (hipGetLastError() != hipSuccess) return set_error(QUAD_EHIP, "k_arch_adv_stats launch failed");
  }
  const hipError_t e = arch->activation == QUAD_ACTFN_TANH ? launch_fwd<QUAD_ACTFN_TANH>(l, s, a)
                                                           : launch_fwd<QUAD_ACTFN_RELU>(l, s, a);
  if (e != hipSuccess) return set_error(QUAD_EHIP, "k_arch_fwd launch failed");
  hipLaunchKernelGGL(k_arch_wgrad, dim3((2 * l.splits * l.tiles + 3) / 4), dim3(LB), 0, s, a);
  if (hipGetLastError() != hipSuccess) return set_error(QUAD_EHIP, "k_arch_wgrad launch failed");
  const int elems = pb_stride(arch->h1, arch->h2) + sp_stride(arch->h2);
  hipLaunchKernelGGL(k_arch_reduce, dim3((elems + 255) / 256, 2), dim3(256), 0, s, a);
  if (hipGetLastError() != hipSuccess) return set_error(QUAD_EHIP, "k_arch_reduce launch failed");
  return QUAD_OK;
}

}  // extern "C"
