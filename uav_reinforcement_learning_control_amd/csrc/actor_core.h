// actor_core.h -- the one MFMA forward, packed-image skeleton, pack kernel and act-launch scaffolding of the
// two-hidden-layer actors IN -> H1 -> H2 -> NOUT: the general actor (actor_arch.h: 12 -> . -> . -> 4, ReLU / tanh)
// and the Brax-profile policy (brax_actor.h: 21 -> . -> . -> 8, ReLU / tanh / SiLU behind a normaliser). A family
// is four compile-time facts: K1 layer-1 k-steps (1: up to 16 inputs, 2: up to 32), NOUT head outputs (4 / 8), NACT
// activations (2: ReLU, tanh; 3: + SiLU) and what it does to its input before the split (its own header).
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
// The k-step-0 W1 pieces, biases, head weights and the family's extra floats are staged in LDS; the pre-split W2
// pieces stream from global memory / L2 (768 KB at [512, 256], shared by every wave) two k-steps ahead of their
// use, and with K1 = 2 the k-step-1 W1 pieces stream the same way, one layer-1 block ahead.
//
// Packed image (floats). Operand element j of lane l (r = l & 31, h = l >> 5) is k = 8h + j of the 32x32x16 MFMA;
// acc_row(reg, h) is the neuron a lane half's accumulator register holds (policy_net.h):
//   B1 : [NB1][2 half][16 reg]             b1[32 n + acc_row(reg, half)]
//   B2 : [MB][2 half][16 reg]              b2[32 m + acc_row(reg, half)]
//   W3 : [MB][16 reg][2 half][NOUT out]    W3[out][32 m + acc_row(reg, half)]
//   B3 : [NOUT]
//   the family's EXTRA floats (brax_actor.h: the normaliser)
//   W1P: [NB1 n][3 piece][64 lane] x 16 B  pieces of A[neuron 32 n + r][input 8 h + j] (zero past the last input)
//   ---- the image up to here is staged in LDS (lds_floats) ----
//   W1Q: the same of inputs 16 + 8 h + j   (K1 = 2 only)
//   W2P: [g][3 piece][64 lane] x 16 B      layer-2 k-step g = (n * 2 + t) * MB + m: pieces of
//                                          A[neuron 32 m + r][input 32 n + acc_row(8 t + j, h)] -- k-step (n, t)
//                                          consumes registers 8t .. 8t + 7 of act(h1) block n
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/quadenv.h"
#include "policy_episode.h"
#include "policy_net.h"

namespace quadenv {

int set_error(int code, const char* msg);  // quadenv.hip

namespace actor {

constexpr int MAX_H1 = 512;
constexpr int UNIT_F = 3 * 64 * 4;  // one three-piece fragment: [3 piece][64 lane] x 16 bytes, in floats

template <int K1_, int NOUT_, int EXTRA_>
struct Layout {
  static constexpr int K1 = K1_, NOUT = NOUT_, EXTRA = EXTRA_;
  int nb1, mb;
  __host__ __device__ constexpr int b1() const { return 0; }
  __host__ __device__ constexpr int b2() const { return 32 * nb1; }
  __host__ __device__ constexpr int w3() const { return b2() + 32 * mb; }
  __host__ __device__ constexpr int b3() const { return w3() + NOUT * 32 * mb; }
  __host__ __device__ constexpr int extra() const { return b3() + NOUT; }
  __host__ __device__ constexpr int w1p() const { return extra() + EXTRA; }
  __host__ __device__ constexpr int lds_floats() const { return w1p() + nb1 * UNIT_F; }
  __host__ __device__ constexpr int lds_bytes() const { return lds_floats() * int(sizeof(float)); }
  __host__ __device__ constexpr int w1q() const { return lds_floats(); }
  __host__ __device__ constexpr int w2p() const { return w1q() + (K1 - 1) * nb1 * UNIT_F; }
  __host__ __device__ constexpr int steps() const { return nb1 * 2 * mb; }  // layer-2 k-steps
  __host__ __device__ constexpr int64_t floats() const { return int64_t(w2p()) + int64_t(steps()) * UNIT_F; }
  // <= 64 KB of LDS (no opt-in) at the largest member, 16-byte aligned pieces
  static constexpr bool fits() {
    return Layout{MAX_H1 / 32, 8}.lds_bytes() <= 64 * 1024 && Layout{1, 2}.w1p() % 4 == 0 && UNIT_F % 4 == 0;
  }
};

// what a kernel needs of the arch: the layer-1 block count and the activation (wave-uniform)
struct Net {
  int nb1;
  int actfn;
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

// SiLU x sigmoid(x) = x / (1 + exp(-x)) without a branch: libm's expf, one add, the correctly rounded division
// (error bound: brax_actor.h SILU_ULP). exp overflow (x < -88.7) gives x / inf = -0; NaN gives NaN.
__device__ __forceinline__ float silu_f32(float x) {
  const float e = expf(-x);
  return __fdiv_rn(x, 1.f + e);
}

template <int ACTF>
__device__ __forceinline__ float act1(float x) {
  return ACTF == QUAD_ACTFN_TANH ? tanh_f32(x) : (ACTF == QUAD_ACTFN_SILU ? silu_f32(x) : relu(x));
}

// the wave-uniform activation tests of a family of NACT members: a family of two tests actfn != 0 for tanh and
// has no SiLU branch (the two-member kernels' code depends on both)
template <int NACT>
__device__ __forceinline__ bool is_tanh(int actfn) {
  return NACT == 2 ? actfn != 0 : actfn == QUAD_ACTFN_TANH;
}
template <int NACT>
__device__ __forceinline__ bool is_silu(int actfn) {
  return NACT == 3 && actfn == QUAD_ACTFN_SILU;
}

// act() of one accumulator block as pieces; `actfn` is wave-uniform, so these are scalar branches
template <int NACT>
__device__ __forceinline__ void act_split(const f32x16& a, int actfn, Q3 (&hq)[2]) {
  float v[16];
  if (is_tanh<NACT>(actfn)) {
#pragma unroll
    for (int i = 0; i < 16; i++) v[i] = tanh_f32(a[i]);
  } else if (is_silu<NACT>(actfn)) {
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

__device__ __forceinline__ P3 lds_pieces(const float* L, int off) {
  P3 x;
#pragma unroll
  for (int p = 0; p < 3; p++) x.p[p] = *reinterpret_cast<const bf16x8*>(L + off + p * 256);
  return x;
}

// this lane's pointer into a streamed piece region (unit 0, piece 0). The scalar base is opaque per call: the
// loads stay inside the callers' step loops (policy_net.h)
__device__ __forceinline__ gbf16x8* lane_pieces(const float* region) {
  uint64_t b = reinterpret_cast<uint64_t>(region);
  asm volatile("" : "+s"(b));
  return reinterpret_cast<gbf16x8*>(b) + (threadIdx.x & 63);
}

// fragment u of a streamed region: the W2 pieces of layer-2 k-step u, the k-step-1 W1 pieces of layer-1 block u
__device__ __forceinline__ P3 global_pieces(gbf16x8* w, int u) {
  P3 x;
#pragma unroll
  for (int p = 0; p < 3; p++) x.p[p] = w[(u * 3 + p) * 64];
  return x;
}

// the head's partial sums of this lane half: part[q] += W3[q][neuron] act(h2[neuron]) over the half's neurons in
// accumulator order (o3: the lane half's offset into W3)
template <int MB, int NOUT, int ACTF>
__device__ __forceinline__ void head(const float* __restrict__ L, int o3, const f32x16 (&acc)[MB], float (&part)[NOUT]) {
#pragma unroll
  for (int m = 0; m < MB; m++) {
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const float v = act1<ACTF>(acc[m][i]);
      float4 w[NOUT / 4];
#pragma unroll
      for (int q = 0; q < NOUT / 4; q++) w[q] = ld4(L, o3 + (m * 16 + i) * 2 * NOUT + 4 * q);
#pragma unroll
      for (int q = 0; q < NOUT / 4; q++) {
        part[4 * q + 0] = fmaf(w[q].x, v, part[4 * q + 0]);
        part[4 * q + 1] = fmaf(w[q].y, v, part[4 * q + 1]);
        part[4 * q + 2] = fmaf(w[q].z, v, part[4 * q + 2]);
        part[4 * q + 3] = fmaf(w[q].w, v, part[4 * q + 3]);
      }
    }
    __builtin_amdgcn_sched_barrier(0);  // one block's accumulators in VGPRs at a time
  }
}

// layer 1 of block n before its activation: the bias, the staged k-step, then (K1 = 2) the streamed one
template <int K1>
__device__ __forceinline__ f32x16 layer1(const float* __restrict__ L, int ob, int ow1, gbf16x8* wq, int n, const P3& xpa,
                                         const P3& xpb) {
  f32x16 b;
  bias_init(b, L, ob + n * 32);
  b = mfma6(lds_pieces(L, ow1 + n * UNIT_F), xpa, b);
  if constexpr (K1 == 2) b = mfma6(global_pieces(wq, n), xpb, b);
  return b;
}

// The forward of the wave's tile, all 64 lanes. xpa / xpb: the split layer-1 operand of k-steps 0 / 1, element j of
// lane l = input 8 (l >> 5) + j (+ 16) of env l & 31, zero past the last input (xpb is read with K1 = 2 only);
// out = the NOUT outputs of env lane & 31 (both lane halves get them). L: the staged image; wp / wq: lane_pieces
// of the global image's W2P / W1Q (wq is read with K1 = 2 only).
template <int MB, int NACT, int K1, int NOUT, int EXTRA>
__device__ __forceinline__ void forward(const float* __restrict__ L, const Layout<K1, NOUT, EXTRA>& lay, int actfn,
                                        const P3& xpa, const P3& xpb, gbf16x8* wp, gbf16x8* wq, float (&out)[NOUT]) {
  static_assert(Layout<K1, NOUT, EXTRA>::fits() && NOUT % 4 == 0, "the staged image fits the default LDS limit");
  const int lane = threadIdx.x & 63, h = lane >> 5;
  const int nb1 = lay.nb1;
  constexpr int S = 2 * MB;  // layer-2 k-steps per layer-1 block
  const int G = nb1 * S;
  const int ob = lay.b1() + h * 16, ow1 = lay.w1p() + lane * 4;

  f32x16 acc[MB];
#pragma unroll
  for (int m = 0; m < MB; m++) bias_init(acc[m], L, lay.b2() + m * 32 + h * 16);
  P3 r0 = global_pieces(wp, 0), r1 = global_pieces(wp, 1);  // G >= 4
  Q3 hq[2];
  act_split<NACT>(layer1<K1>(L, ob, ow1, wq, 0, xpa, xpb), actfn, hq);
  for (int n = 0; n < nb1; n++) {
    // layer 1 of the next block first, so its result is there when this block's steps are through
    // (wave-uniform: the last block has no next one)
    const bool more = n + 1 < nb1;
    f32x16 a1n;
    if (more) a1n = layer1<K1>(L, ob, ow1, wq, n + 1, xpa, xpb);
    P3 ring[3];
    ring[0] = r0;
    ring[1] = r1;
#pragma unroll
    for (int s = 0; s < S; s++) {
      const int g2 = n * S + s + 2;  // two steps ahead, into the slot step s - 1 freed; clamped in range
      ring[(s + 2) % 3] = global_pieces(wp, g2 < G ? g2 : G - 1);
      acc[s % MB] = mfma6(ring[s % 3], hq[s / MB].p(), acc[s % MB]);
      __builtin_amdgcn_sched_barrier(0);  // one step per scheduling region: at most three fragments in flight
    }
    r0 = ring[S % 3];
    r1 = ring[(S + 1) % 3];
    if (more) act_split<NACT>(a1n, actfn, hq);
  }
  float part[NOUT] = {};
  // one branch around the whole head, not one per block: each form is straight-line code that reads an
  // accumulator block out of the AGPRs when its turn comes (a branch per block put all 128 values in VGPRs)
  const int o3 = lay.w3() + h * NOUT;
  if (is_tanh<NACT>(actfn)) head<MB, NOUT, QUAD_ACTFN_TANH>(L, o3, acc, part);
  else if (is_silu<NACT>(actfn)) head<MB, NOUT, QUAD_ACTFN_SILU>(L, o3, acc, part);
  else head<MB, NOUT, QUAD_ACTFN_RELU>(L, o3, acc, part);
  // lower half's partial + upper half's, in every lane (policy_net.h net_core)
#pragma unroll
  for (int q = 0; q < NOUT; q++) {
    const auto p = __builtin_amdgcn_permlane32_swap(__float_as_uint(part[q]), __float_as_uint(part[q]), false, false);
    out[q] = (__uint_as_float(p[0]) + __uint_as_float(p[1])) + L[lay.b3() + q];
  }
}

// the image's LDS part, global -> LDS, by the whole block; ends with a barrier
template <int BLK>
__device__ __forceinline__ void stage(float* lds, const float* __restrict__ packed, int lds_floats) {
  const int nv = lds_floats / 4;
  const float4* src = reinterpret_cast<const float4*>(packed);
  float4* dst = reinterpret_cast<float4*>(lds);
  for (int k = threadIdx.x; k < nv; k += BLK) dst[k] = src[k];
  __syncthreads();
}

// ---- act kernels: wave w of the grid takes the 32-row tiles w, w + waves, ...; lanes l and l + 32 carry row
// l & 31. f(row, row < n, lane half) runs on the full wave for every tile of the wave.
constexpr int ACT_BLK = 256, ACT_MAX_GRID = 512;
template <class F>
__device__ __forceinline__ void act_tiles(int32_t n, F&& f) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int tiles = (n + TILE - 1) / TILE;
  for (int tile = blockIdx.x * (ACT_BLK / 64) + wave; tile < tiles; tile += gridDim.x * (ACT_BLK / 64)) {
    const int row = tile * TILE + (lane & 31);
    f(row, row < n, lane >> 5);
  }
}
inline dim3 act_grid(int32_t n) {
  const int tiles = (n + TILE - 1) / TILE, want = (tiles + ACT_BLK / 64 - 1) / (ACT_BLK / 64);
  return dim3(want < ACT_MAX_GRID ? want : ACT_MAX_GRID);
}

// ---- pack: one thread per float of the f32 regions, then one per (fragment, lane) unit of the piece regions,
// which follow each other from W1P on: K1 x NB1 layer-1 fragments (k-step t, block n), then the layer-2 k-steps.
// P: Quad*ActorParams, its weights torch's [out, in] (TORCH) or flax's [in, out]; NIN: the observation size.
template <bool TORCH>
__device__ __forceinline__ float weight(const float* w, int out, int n_out, int in, int n_in) {
  return TORCH ? w[size_t(out) * n_in + in] : w[size_t(in) * n_out + out];
}
template <class LAY, bool TORCH, int NIN, class P>
__device__ __forceinline__ void pack_body(const P& p, int h1, int h2, float* __restrict__ out) {
  constexpr int NOUT = LAY::NOUT;
  const LAY lay{h1 / 32, h2 / 32};
  const int nf = lay.w1p(), n1 = LAY::K1 * lay.nb1 * 64, n2 = lay.steps() * 64;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= nf + n1 + n2) return;
  if (idx < nf) {
    float v = 0.f;
    if (idx < lay.w3()) {  // B1 | B2: [block][half][reg]
      const bool second = idx >= lay.b2();
      const int t = idx - (second ? lay.b2() : 0);
      v = (second ? p.b1 : p.b0)[32 * (t / 32) + acc_row(t % 16, (t / 16) % 2)];
    } else if (idx < lay.b3()) {  // W3: [m][reg][half][out]
      const int t = idx - lay.w3();
      v = weight<TORCH>(p.w2, t % NOUT, NOUT, 32 * (t / (32 * NOUT)) + acc_row((t / (2 * NOUT)) % 16, (t / NOUT) % 2), h2);
    } else if (idx < lay.extra()) {
      v = p.b2[idx - lay.b3()];
    } else if constexpr (LAY::EXTRA > 0) {  // the normaliser (brax_actor.h): MEAN | STD padded with 0 / 1, MISC
      const int f = idx - (idx < lay.stdv() ? lay.mean() : lay.stdv());
      if (idx < lay.stdv()) v = f < NIN ? p.mean[f] : 0.f;
      else if (idx < lay.misc()) v = f < NIN ? p.std[f] : 1.f;
      else v = idx == lay.misc() ? p.min_std : 0.f;
    }
    out[idx] = v;
    return;
  }
  const int u = idx - nf, frag = u / 64;
  const int lane = u % 64, r = lane & 31, h = lane >> 5;
  float v8[8];
  if (u < n1) {  // A[neuron 32 n + r][input 16 t + 8 h + j]
    const int t = LAY::K1 == 1 ? 0 : frag / lay.nb1, n = frag - t * lay.nb1;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const int f = 16 * t + 8 * h + j;
      v8[j] = f < NIN ? weight<TORCH>(p.w0, 32 * n + r, h1, f, NIN) : 0.f;
    }
  } else {  // A[neuron 32 m + r][input 32 n + acc_row(8 t + j, h)] of k-step g = (n * 2 + t) * MB + m
    const int g = frag - n1 / 64, m = g % lay.mb, t = (g / lay.mb) % 2, n = g / (2 * lay.mb);
#pragma unroll
    for (int j = 0; j < 8; j++) v8[j] = weight<TORCH>(p.w1, 32 * m + r, h2, 32 * n + acc_row(8 * t + j, h), h1);
  }
  const P3 x = split8(v8);
  bf16x8* dst = reinterpret_cast<bf16x8*>(out + lay.w1p()) + frag * 3 * 64 + lane;
#pragma unroll
  for (int q = 0; q < 3; q++) dst[q * 64] = x.p[q];
}
template <class LAY, bool TORCH, int NIN, class P>
__global__ void k_pack(P p, int h1, int h2, float* __restrict__ out) {
  pack_body<LAY, TORCH, NIN>(p, h1, h2, out);
}
// the grid of k_pack and of its population form (actor_rollout.hip)
template <class LAY>
inline int pack_blocks(const LAY& lay) {
  return (lay.w1p() + (LAY::K1 * lay.nb1 + lay.steps()) * 64 + 255) / 256;
}
template <class LAY, bool TORCH, int NIN, class P>
hipError_t launch_pack(const LAY& lay, const P& p, float* packed, hipStream_t s) {
  hipLaunchKernelGGL((k_pack<LAY, TORCH, NIN, P>), dim3(pack_blocks(lay)), dim3(256), 0, s, p, lay.nb1 * 32,
                     lay.mb * 32, packed);
  return hipGetLastError();
}

// ---- the checked arch of either family (A: Quad*ActorArch). who: the messages' prefix; silu: is SiLU a member?
// QUAD_OK and *out, or QUAD_EINVAL with a message for an arch outside the family
template <class A>
int net_of(const A* a, const char* who, bool silu, ActorNet* out) {
  const auto bad = [&](const char* m) { return set_error(QUAD_EINVAL, (std::string(who) + m).c_str()); };
  if (!a) return bad(" is NULL");
  if (a->h1 < 32 || a->h1 > MAX_H1 || a->h1 % 32 != 0) return bad(": h1 must be a multiple of 32 in [32, 512]");
  if (a->h2 != 64 && a->h2 != 128 && a->h2 != 256) return bad(": h2 must be 64, 128 or 256");
  if (a->activation != QUAD_ACTFN_RELU && a->activation != QUAD_ACTFN_TANH && !(silu && a->activation == QUAD_ACTFN_SILU))
    return bad(silu ? ": activation must be QUAD_ACTFN_RELU, _TANH or _SILU"
                    : ": activation must be QUAD_ACTFN_RELU or QUAD_ACTFN_TANH");
  *out = ActorNet{a->h1 / 32, a->h2 / 32, a->activation};
  return QUAD_OK;
}

}  // namespace actor
}  // namespace quadenv
