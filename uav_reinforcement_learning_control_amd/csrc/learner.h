// learner.h -- definitions shared by the two forms of the PPO minibatch-gradient kernel (device
// and host): learner.hip (f32-input MFMA, k_ppo_grad) and learner_x3.hip (bf16x3 split MFMA,
// k_ppo_grad_x3). Both write the same per-block partial image, summed by k_ppo_reduce.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/quadenv.h"
#include "policy_net.h"

namespace quadenv {

namespace lrn {

constexpr int LB = 256;       // threads per block: 4 waves, one per SIMD
constexpr int RND = 64;       // rows per round (two 32-row MFMA tiles)
constexpr int ADV_BLOCKS = 256;
constexpr int MAX_NB = 128;   // blocks per net on average (the device has 256 CUs)

// per-net partial image (floats): W1 [128][12], b1, W2 [128][128], b2, W3 [NOUT][128], b3,
// log_std [4] (actor), then 4 statistic slots
constexpr int P_W1 = 0, P_B1 = P_W1 + H * OBS, P_W2 = P_B1 + H, P_B2 = P_W2 + H * H, P_W3 = P_B2 + H;
constexpr int P_B3A = P_W3 + ACT * H, P_LS = P_B3A + ACT, P_STATS = P_LS + ACT;  // 18,696
constexpr int P_B3C = P_W3 + H;
constexpr int PSTRIDE = P_STATS + 8;   // 18,704 (16-byte multiple)
static_assert(P_STATS == 18696 && P_B3C + 1 == 18305, "SB3 parameter counts (actor 18,696, critic 18,305)");

struct NetW {
  const float *w0, *b0, *w1, *b1, *w2, *b2;
};

struct GArgs {
  NetW actor, critic;
  const float* log_std;
  const float *obs, *act, *logp_old, *adv, *ret;
  const int64_t* idx;
  const double* adv_part;  // [ADV_BLOCKS][2] or NULL (no normalization)
  float* part;             // [nb + nbc][PSTRIDE]: actor blocks, then critic blocks
  int32_t batch, nb, per_block;     // actor: nb blocks of per_block rows
  int32_t nbc, per_block_c;         // critic: nbc blocks of per_block_c rows
  float clip, inv_batch, vf_coef;
  float* dump;  // diagnostics only (k_ppo_grad*_dump): [2 nets][batch][256] hidden pre-activations
  const void* wimg;  // bf16x3 form: the W2 fragments of every wave as bf16 pieces (k_x3_prep, WIMG_BYTES)
};

// k_ppo_reduce's arguments
struct RArgs {
  QuadPolicyGrads gr;
  const float* part;
  const float* log_std;
  float* stats;
  int32_t nb, nbc;
  float inv_batch, ent_coef;
};

// k_grad_sumsq's and k_adam's arguments (quad_clip_adam)
struct AdamArgs {
  QuadAdam a;
  int32_t offs[QUAD_ADAM_MAX_TENSORS + 1];  // prefix sums of numel
  float* part;                              // [nblocks] sums of squares
  int32_t nblocks;
};

struct Layout {
  int nb, per_block, nbc, per_block_c;
  int64_t part_bytes, adv_bytes, wimg_bytes;
};

// the bf16x3 form's pre-split W2 image (learner_x3.hip k_x3_prep / split_w2_unit): 2 nets x 4 waves x 2 uses x
// 8 k-steps x 3 pieces x 64 lanes x 16 bytes, after the partial image in the workspace
constexpr int64_t WIMG_BYTES = int64_t(2) * 4 * 2 * 8 * 3 * 64 * 16;

// Block split of a minibatch of `batch` rows: the two nets share the 2 * MAX_NB block slots in
// proportion `actor_share` / 1000 (a critic round costs less than an actor round: no log-prob /
// ratio work). The partial image is sized for every split (nb + nbc <= slots).
inline Layout layout_of(int32_t batch, int actor_share) {
  Layout l{};
  const int rounds = (batch + RND - 1) / RND;
  const int slots = rounds < MAX_NB ? 2 * rounds : 2 * MAX_NB;
  int na = int((int64_t(slots) * actor_share + 500) / 1000);
  na = na < 1 ? 1 : (na > slots - 1 ? slots - 1 : na);
  l.nb = na < rounds ? na : rounds;
  l.nbc = slots - na < rounds ? slots - na : rounds;
  l.per_block = ((rounds + l.nb - 1) / l.nb) * RND;
  l.per_block_c = ((rounds + l.nbc - 1) / l.nbc) * RND;
  l.part_bytes = int64_t(slots) * PSTRIDE * int64_t(sizeof(float));
  l.adv_bytes = int64_t(ADV_BLOCKS) * 2 * int64_t(sizeof(double));
  l.wimg_bytes = WIMG_BYTES;
  return l;
}

// The bf16x3 form (learner_x3.hip): every block runs both nets over the same rows (the actor's
// rounds, then the critic's), X3_BLOCKS blocks = one per CU, so every CU carries the same work. A
// split of the CUs between the nets (the f32 form's actor share) left the slower net's blocks ~5 %
// longer than the average at any share (round granularity).
constexpr int X3_BLOCKS = 256;
inline Layout layout_both(int32_t batch) {
  Layout l{};
  const int rounds = (batch + RND - 1) / RND;
  const int nb = rounds < X3_BLOCKS ? rounds : X3_BLOCKS;
  l.nb = l.nbc = nb;
  l.per_block = l.per_block_c = ((rounds + nb - 1) / nb) * RND;
  l.part_bytes = int64_t(2) * nb * PSTRIDE * int64_t(sizeof(float));
  l.adv_bytes = int64_t(ADV_BLOCKS) * 2 * int64_t(sizeof(double));
  l.wimg_bytes = WIMG_BYTES;
  return l;
}
// k_x3_prep (the W2 split, + the advantage statistics when adv_stats != NULL) + k_ppo_grad_x3
int launch_ppo_grad_x3(const GArgs& g, hipStream_t s, double* adv_stats, const float* adv);
int launch_ppo_grad_x3_dump(const GArgs& g, hipStream_t s, double* adv_stats, const float* adv);

// Block `blk` of the minibatch advantage statistics (sum and sum of squares in float64; fixed
// order: per-thread strided over i = blk * 256 + tid + k * ADV_BLOCKS * 256, then a tree) into
// part[2 blk], part[2 blk + 1]. The index loads and the gathers go out 8 at a time (the sums keep the
// same order): one at a time, each thread waited out 8 dependent HBM round trips (12.4 us per
// 524,288-row minibatch under rocprof). Needs 256 threads and `red` [2][256] in LDS.
__device__ __forceinline__ void adv_stats_block(const float* __restrict__ adv, const int64_t* __restrict__ idx,
                                                int batch, double* __restrict__ part, int blk, double (*red)[256]) {
  const int tid = threadIdx.x;
  double s = 0.0, s2 = 0.0;
  constexpr int STRIDE = ADV_BLOCKS * 256, U = 8;
  for (int i0 = blk * 256 + tid; i0 < batch; i0 += U * STRIDE) {
    int64_t j[U];
#pragma unroll
    for (int u = 0; u < U; u++) j[u] = i0 + u * STRIDE < batch ? idx[i0 + u * STRIDE] : int64_t(-1);
    float v[U];
#pragma unroll
    for (int u = 0; u < U; u++) v[u] = j[u] >= 0 ? adv[j[u]] : 0.f;
#pragma unroll
    for (int u = 0; u < U; u++) {
      if (j[u] < 0) continue;
      const double d = v[u];
      s += d;
      s2 += d * d;
    }
  }
  red[0][tid] = s;
  red[1][tid] = s2;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) { red[0][tid] += red[0][tid + o]; red[1][tid] += red[1][tid + o]; }
    __syncthreads();
  }
  if (tid == 0) { part[2 * blk] = red[0][0]; part[2 * blk + 1] = red[1][0]; }
}

// Diagnostics (quad_ppo_hidden): the kernels' own hidden pre-activations of minibatch row `pos`
// (before the ReLU; layer 0 = h1, 1 = h2) -- the dump instantiation of the same body, so the same
// arithmetic as the gradient launch
__device__ __forceinline__ void dump_pre(float* dump, int net, int batch, int pos, int layer, int neuron, float v) {
  dump[(size_t(net) * size_t(batch) + size_t(pos)) * 256 + size_t(128 * layer + neuron)] = v;
}

// ---- What the two kernel bodies (body<> of learner.hip and learner_x3.hip) share. The products, the LDS
// layouts and the per-row accumulation (a*b + c fuses only within one source expression) stay in the bodies.

// The actor's advantage normalization constants: a fixed-order float64 tree over the pre-pass
// partials (adv_stats_block), then mean and 1 / (std + 1e-8) as SB3 forms them. {0, 1} for the
// critic and without normalization. Needs 256 threads and two double[LB] in LDS.
struct AdvNorm { float mu, rden; };
template <int NOUT>
__device__ __forceinline__ AdvNorm adv_norm(const GArgs& g, double* red0, double* red1) {
  const int tid = threadIdx.x;
  float adv_mu = 0.f, adv_den = 1.f;
  if (NOUT == ACT && g.adv_part) {
    red0[tid] = g.adv_part[2 * tid];
    red1[tid] = g.adv_part[2 * tid + 1];
    __syncthreads();
    for (int o = LB / 2; o > 0; o >>= 1) {
      if (tid < o) { red0[tid] += red0[tid + o]; red1[tid] += red1[tid + o]; }
      __syncthreads();
    }
    const double n = double(g.batch), s = red0[0], s2 = red1[0];
    const double var = fmax((s2 - s * s / n) / (n - 1.0), 0.0);
    adv_mu = float(s / n);
    adv_den = float(sqrt(var)) + 1e-8f;
  }
  return AdvNorm{adv_mu, 1.f / adv_den};
}

// b1, b2 and the head weights neuron-major ([128][4], zero past NOUT) into LDS, at float offsets
// o_b1 / o_b2 / o_w3t of the body's image L (indexed as the bodies index it: same address arithmetic)
template <int NOUT>
__device__ __forceinline__ void stage_small_weights(const NetW& W, float* L, int o_b1, int o_b2, int o_w3t) {
  for (int i = threadIdx.x; i < H; i += LB) {
    L[o_b1 + i] = W.b0[i];
    L[o_b2 + i] = W.b1[i];
#pragma unroll
    for (int k = 0; k < 4; k++) L[o_w3t + 4 * i + k] = k < NOUT ? W.w2[k * H + i] : 0.f;
  }
}

// Row staging, one round ahead: a block's slice [s0, s1) of the minibatch in rounds of RND rows.
// Threads 0..191 gather the observation rows (float4 each), threads 192..255 the row scalars; the
// minibatch indices are loaded two rounds ahead, so no gather waits on its index load. Rows past
// the slice stage zeros (and are masked as invalid).
template <int NOUT>
struct RowStage {
  const GArgs& g;
  int tid, s0, s1, rounds, srow;
  float4 pf;
  float pfs[3];

  __device__ __forceinline__ RowStage(const GArgs& g_, int blk) : g(g_) {
    tid = threadIdx.x;
    const int per_block = NOUT == ACT ? g.per_block : g.per_block_c;
    s0 = blk * per_block;
    s1 = min(g.batch, s0 + per_block);
    rounds = s1 > s0 ? (s1 - s0 + RND - 1) / RND : 0;
    srow = tid < 3 * RND ? tid / 3 : tid - 3 * RND;
    pf = make_float4(0.f, 0.f, 0.f, 0.f);
    pfs[0] = pfs[1] = pfs[2] = 0.f;
  }
  // the minibatch index of this thread's row of round rd (-1: past the slice); written as `rd < rounds &&
  // i < s1` the round test folds into a select and three bf16x3 kernels allocate 3-12 more or fewer registers
  __device__ __forceinline__ int64_t index_of(int rd) const {
    if (rd >= rounds) return -1;
    const int i = s0 + rd * RND + srow;
    return i < s1 ? g.idx[i] : int64_t(-1);
  }
  __device__ __forceinline__ void gather(int64_t row) {
    pf = make_float4(0.f, 0.f, 0.f, 0.f);
    pfs[0] = pfs[1] = pfs[2] = 0.f;
    if (row < 0) return;
    if (tid < 3 * RND) {
      pf = reinterpret_cast<const float4*>(g.obs)[size_t(row) * 3 + tid % 3];
    } else if (NOUT == ACT) {
      pf = reinterpret_cast<const float4*>(g.act)[row];
      pfs[0] = g.logp_old[row];
      pfs[1] = g.adv[row];
    } else {
      pfs[2] = g.ret[row];
    }
  }
  // threads 192..255: the scalars into row srow of the [64][8] image `sci` (action 4, old logp, adv, return)
  __device__ __forceinline__ void store_scalars(float* sci) const {
    *reinterpret_cast<float4*>(sci + srow * 8) = pf;
    sci[srow * 8 + 4] = pfs[0]; sci[srow * 8 + 5] = pfs[1]; sci[srow * 8 + 6] = pfs[2];
  }
};

// head output of row e: the four waves' partial sums ([4][64][4] at float offset `o` of L) in a
// fixed order, + bias
template <int NOUT>
__device__ __forceinline__ void head_out(const float* L, int o, int e, const float (&b3)[NOUT], float (&out)[NOUT]) {
#pragma unroll
  for (int k = 0; k < NOUT; k++)
    out[k] = (((L[o + e * 4 + k] + L[o + (RND + e) * 4 + k]) + L[o + (2 * RND + e) * 4 + k]) +
              L[o + (3 * RND + e) * 4 + k]) + b3[k];
}

// The loss of SB3's PPO.train (stable_baselines3/ppo/ppo.py, third-party) for one minibatch row:
// what the row contributes to the gradient and to the logged statistics. `sc` is the row's 8 staged
// scalars (action 4, old logp, adv, return), `out` the head output (mean / value).
template <int NOUT>
struct RowTerms {
  float dd[NOUT];  // dL/d(head output); 0 on an invalid row
  // actor: dL/dlogp (0 on an invalid row), (a - mean) / std, the policy loss term, 1 if |ratio - 1| > clip
  float dlp, z[ACT], pg, clipped;
  float diff;  // critic: value - return
};
template <int NOUT>
__device__ __forceinline__ RowTerms<NOUT> row_terms(const GArgs& g, const float (&out)[NOUT], const float* sc,
                                                    const float (&ls)[ACT], const float (&isd)[ACT], AdvNorm an,
                                                    bool valid) {
  RowTerms<NOUT> t;
  if constexpr (NOUT == ACT) {
    const float4 a4 = *reinterpret_cast<const float4*>(sc);
    const float a4k[4] = {a4.x, a4.y, a4.z, a4.w};
    float lp = 0.f;
#pragma unroll
    for (int k = 0; k < ACT; k++) {
      t.z[k] = (a4k[k] - out[k]) * isd[k];
      lp += -0.5f * t.z[k] * t.z[k] - ls[k] - 0.91893853320467274f;
    }
    // ratio = exp(logp - old) on the hardware exp2 (~1 ulp; the correctly rounded expf is ~10 VALU)
    const float r = __builtin_amdgcn_exp2f((lp - sc[4]) * 1.44269504088896341f);
    const float A = g.adv_part ? (sc[5] - an.mu) * an.rden : sc[5];
    const float cr = fminf(fmaxf(r, 1.f - g.clip), 1.f + g.clip);
    const float sa = A * r, sb = A * cr;
    // d min(sa, sb): the unclipped branch where it is the smaller, half of each on a tie (torch.min's
    // backward), else the clipped branch, whose derivative is r's inside the clip range only
    const float w1 = sa < sb ? 1.f : (sa == sb ? 0.5f : 0.f);
    const float inr = (r >= 1.f - g.clip && r <= 1.f + g.clip) ? 1.f : 0.f;
    t.dlp = valid ? -g.inv_batch * A * (w1 + (1.f - w1) * inr) * r : 0.f;
#pragma unroll
    for (int k = 0; k < ACT; k++) t.dd[k] = t.dlp * t.z[k] * isd[k];
    t.pg = -fminf(sa, sb);
    t.clipped = fabsf(r - 1.f) > g.clip ? 1.f : 0.f;
  } else {
    t.diff = out[0] - sc[6];
    t.dd[0] = valid ? 2.f * g.vf_coef * g.inv_batch * t.diff : 0.f;
  }
  return t;
}

// The block's per-row sums v (head bias gradient [NOUT], log_std gradient [ACT], pg sum, vf sum, clipped
// count), already summed over wave 0's lanes, into its partial image P. The lane sum stays in the bodies: in
// here it changes the bf16x3 round loop's FMA packing (+2.7 % time, profiles/r07/learner_shared_helpers.txt)
template <int NOUT>
__device__ __forceinline__ void store_row_sums(float* P, const float (&v)[NOUT + ACT + 3]) {
  const int b3off = NOUT == ACT ? P_B3A : P_B3C;
#pragma unroll
  for (int k = 0; k < NOUT; k++) P[b3off + k] = v[k];
  if (NOUT == ACT) {
#pragma unroll
    for (int k = 0; k < ACT; k++) P[P_LS + k] = v[NOUT + k];
  }
#pragma unroll
  for (int k = 0; k < 3; k++) P[P_STATS + k] = v[NOUT + ACT + k];
}

}  // namespace lrn
}  // namespace quadenv
