// rvo3d_policy_mlp_x3.hpp -- config 3's policy step at float32-class precision in ONE kernel: the network, the
// observation rows, the per-row tail and the outputs of policy_mlp_kernel (rvo3d_policy_mlp.hpp), with every product
// of the three layers computed as split bf16, a_hi b_hi + a_lo b_hi + a_hi b_lo with float32 accumulation
// (v_mfma_f32_32x32x16_bf16; hi = bf16_rne(x), lo = bf16_rne(x - hi): ~16 bits of each factor, the dropped a_lo b_lo
// is below 2^-16 of the product).
// Reference: train/policy/policy_rnn_ac.py:57-69 (ac.step), :197-235 (GaussianActor), :238-257 (Critic), float32.
// Part of the gfx950 device code (see rvo3d_device.hpp for the overview).
//
// Orientation, fragment maps and the permuted k order between layers (mfma_k_perm) are those of policy_mlp_kernel:
// weights are the A operand, activations the B operand, a wave takes 32 batch rows per pass through all layers and
// finishes 64 rows (one per lane) after two passes.  The pass -> row map, the observation descriptor and the count of
// data k-steps are its functions (MlpWave, mlp_obs_rsrc, mlp_data_steps), the pack's decoding mlp_pack_elements; the
// arithmetic of the split is rvo3d_mfma_tiles.hpp's.  What changes is the weight and register budget ("The
// float32-class policy step"): hi and lo double both.
//  * Registers: H1 as hi and lo fragments is 128 VGPRs; with two accumulators, the head tile, the split second-layer
//    activations and two small weight rings the kernel stays at two waves per SIMD (256 registers) without spilling.
//  * Weights: the hi halves of the second layer (128 KB), its bias table and the head rows (hi and lo) stay in LDS for
//    the workgroup's life (133 KB); the first layer (hi and lo, 16 KS1 KB) and the lo halves of the second layer
//    (128 KB) every wave streams from L2, a few fragments ahead.  Per k-step of the second layer that is one LDS and
//    one L2 fragment for three MFMAs, against one fragment per MFMA in the bf16 kernel.
// The first layer's bias rides as hi and lo in the weight column k_in against the exact constant 1; the second layer's
// bias (float32) is the C operand of a tile's first MFMA; the heads' bias (float32) is added in the tail.  ReLU acts
// on the float32 accumulators, the split follows it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "rvo3d_mfma_tiles.hpp"
#include "rvo3d_policy_mlp.hpp"
#include "rvo3d_rollout_kernels.hpp"

namespace rvo3d {

// Blob of one network (16-byte aligned pieces, in this order):
//   W1     [8 tiles][KS1 k-steps][2: hi, lo][64 lanes][8] bf16     16 KS1 KB   (L2)
//   W2 hi  [8 tiles][16 k-steps][64 lanes][8] bf16                 128 KB  \
//   b2     [8 tiles][2 lane halves][16 registers] float            1 KB     > the LDS image, one contiguous copy
//   W3     [16 k-steps][2: hi, lo][4 rows][2 lane halves][8] bf16  4 KB    /
//   W2 lo  [8 tiles][16 k-steps][64 lanes][8] bf16                 128 KB  (L2)
//   head bias float[4]
constexpr int kX3W2Bytes = 8 * 16 * 1024;   // one half (hi or lo) of the second layer
constexpr int kX3W3Bytes = 16 * 2 * 4 * 2 * 16;
constexpr int kX3LdsBytes = kX3W2Bytes + kMlpB2Bytes + kX3W3Bytes;
__host__ __device__ constexpr int64_t mlp_x3_net_bytes(int ks1) {
  return (int64_t)16 * 1024 * ks1 + kX3LdsBytes + kX3W2Bytes + kMlpHeadBiasBytes;
}

__global__ void __launch_bounds__(256) mlp_x3_pack_kernel(const MlpPackArgs A) {
  const int net = blockIdx.y;
  const int ks1 = A.ks1;
  unsigned char* const blob = A.blob + net * mlp_x3_net_bytes(ks1);
  uint16_t* const w1 = reinterpret_cast<uint16_t*>(blob);
  uint16_t* const w2h = reinterpret_cast<uint16_t*>(blob + (int64_t)16 * 1024 * ks1);
  float* const b2 = reinterpret_cast<float*>(blob + (int64_t)16 * 1024 * ks1 + kX3W2Bytes);
  uint16_t* const w3 = reinterpret_cast<uint16_t*>(blob + (int64_t)16 * 1024 * ks1 + kX3W2Bytes + kMlpB2Bytes);
  uint16_t* const w2l = reinterpret_cast<uint16_t*>(blob + (int64_t)16 * 1024 * ks1 + kX3LdsBytes);
  float* const hb = reinterpret_cast<float*>(blob + (int64_t)16 * 1024 * ks1 + kX3LdsBytes + kX3W2Bytes);
  // every weight as hi and lo: W1 and W3 interleave them per k-step, W2 keeps two arrays; b2 and the head bias are float
  mlp_pack_elements(A, net, [&](int section, int i, float v) RVO3D_INLINE {
    if (section == kPackB2) { b2[i] = v; return; }
    if (section == kPackHeadBias) { hb[i] = v; return; }
    uint16_t hi, lo;
    bf16_split(v, hi, lo);
    if (section == kPackW1) {         // [m][s][lane][j] -> [m][s][hi, lo][lane][j]
      w1[(int64_t)(i >> 9) * 1024 + (i & 511)] = hi;
      w1[(int64_t)(i >> 9) * 1024 + 512 + (i & 511)] = lo;
    } else if (section == kPackW2) {
      w2h[i] = hi;
      w2l[i] = lo;
    } else {                          // [t][row][h][j] -> [t][hi, lo][row][h][j]
      w3[(i >> 6) * 128 + (i & 63)] = hi;
      w3[(i >> 6) * 128 + 64 + (i & 63)] = lo;
    }
  });
}

// relu, then the split of two accumulator registers into one packed hi pair and one packed lo pair
__device__ __forceinline__ Bf16x2Split relu_split2(float a, float b) {
  Bf16x2Split p = split_bf16x2(relu_f32(a), relu_f32(b));
  asm volatile("" : "+v"(p.hi), "+v"(p.lo));  // (pinned to this slot of the pipeline)
  return p;
}

template <int KS1, int NW>
__global__ void __launch_bounds__(64 * NW) policy_mlp_x3_kernel(const PolicyMlpArgs A) {
  static_assert(kX3LdsBytes <= 160 * 1024, "LDS");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const unsigned char* const w2s = smem;                                                  // W2 hi
  const float* const b2t = reinterpret_cast<const float*>(smem + kX3W2Bytes);
  const unsigned char* const w3s = smem + kX3W2Bytes + kMlpB2Bytes;

  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // the actor's and the critic's workgroup of one group of rows on the same XCD (as policy_mlp_kernel)
  const bool paired = (gridDim.x & 15) == 0;
  const int net = paired ? (blockIdx.x >> 3) & 1 : blockIdx.x & 1;
  const int g = paired ? (blockIdx.x >> 4) * 8 + (blockIdx.x & 7) : blockIdx.x >> 1, G = gridDim.x >> 1;
  const unsigned char* const blob = A.blob + net * A.net_bytes;
  // the streamed weights through a buffer descriptor too: one lane offset in a VGPR, the fragment's offset a scalar
  // (with plain global loads the compiler keeps a 64-bit address per fragment live across the pass loop)
  const __amdgpu_buffer_rsrc_t blob_rs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned char*>(blob), 0, (int)A.net_bytes, 0x00020000);
  constexpr int kW2lo = 16 * 1024 * KS1 + kX3LdsBytes;  // byte offset of W2 lo in the net's blob
  auto stream16 = [&](int off) {
    return __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(blob_rs, lane * 16, off, 0));
  };
  const int64_t rows = A.S.rows;
  const MlpWave<NW> W{r, wave, g, G, rows};
  const int iters = W.iters();

  {  // the resident weights: the only workgroup-wide step of the kernel
    uint4* dst = reinterpret_cast<uint4*>(smem);
    const uint4* src = reinterpret_cast<const uint4*>(blob + (int64_t)16 * 1024 * KS1);
    for (int i = tid; i < kX3LdsBytes / 16; i += 64 * NW) dst[i] = src[i];
  }
  __syncthreads();
  const float4 head_bias = *reinterpret_cast<const float4*>(blob + A.net_bytes - kMlpHeadBiasBytes);
  const SampleConsts SC = sample_consts(A.S);

  const __amdgpu_buffer_rsrc_t obs_rs = mlp_obs_rsrc(A);
  // (wrapped in a lambda on purpose: called straight from the pass, the function changes the register allocation)
  auto data_steps = [&](int pass) -> int { return mlp_data_steps<KS1>(A, W, pass); };

  float zs0 = 0.f, zs1 = 0.f, zs2 = 0.f;
#pragma unroll 1
  for (int pass = 0; pass < 2 * iters; ++pass) {
    const int n_data = data_steps(pass);
    // ---- 32 observation rows as the hi / lo B fragments of the first product ----
    bf16x8 Xh[KS1], Xl[KS1];
    {
      const uint32_t off = (uint32_t)((W.obs_row(pass) * A.ld_obs + 8 * h) * 4);
#pragma unroll
      for (int s = 0; s < KS1; ++s) {
        f32x8 v = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (s < n_data) {
          const float4 a = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(obs_rs, off + 64 * s, 0, 0));
          const float4 b = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(obs_rs, off + 64 * s + 16, 0, 0));
          v = f32x8{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        }
        if (s == KS1 - 1) {  // the row's tail, the constant 1 that multiplies the bias column, zeros
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int k = 16 * s + 8 * h + j;
            v[j] = k < A.k_in ? v[j] : (k == A.k_in ? 1.0f : 0.0f);
          }
        }
        split8(v, Xh[s], Xl[s]);
      }
    }
    u32x4 H1h[16], H1l[16];  // H1^T [256][32] as hi / lo B fragments of the second product
    f32x16 accs[2];
    constexpr int DL = 3;    // second-layer lo fragments in flight (from L2)
    bf16x8 lring[DL];
    auto w2lo = [&](int i) { return stream16(kW2lo + i * 1024); };  // flat index i = 16 m2 + t
    // ---- layer 1: H1^T = relu(W1 X^T), the weights from L2 (hi, lo per k-step, D1 k-steps ahead) ----
    // Three straight-line versions, chosen per pass (wave-uniform) as in policy_mlp_kernel: every k-step; the first
    // two plus the bias step; the first plus the bias step.
    auto layer1 = [&](auto nd_tag) {
      constexpr int ND = decltype(nd_tag)::value;
      constexpr int NSTEP = ND < KS1 ? ND + 1 : KS1;
      constexpr int D1 = 2, kSteps = 8 * NSTEP;
      // the previous tile's epilogue overlapped with this tile's MFMAs (two accumulators) - except in a pass over six
      // or more k-steps, where the split observation rows leave no room for the second accumulator
      constexpr bool kOverlap = NSTEP < 6;
      auto k_of = [](int j) constexpr { return j < ND ? j : KS1 - 1; };
      auto frag = [&](int i, int part) { return stream16((((i / NSTEP) * KS1 + k_of(i % NSTEP)) * 2 + part) * 1024); };
      bf16x8 rh[D1], rl[D1];
#pragma unroll
      for (int i = 0; i < D1; ++i) { rh[i] = frag(i, 0); rl[i] = frag(i, 1); }
#pragma unroll
      for (int m = 0; m < 8; ++m)
#pragma unroll
      for (int j = 0; j < NSTEP; ++j) {
        const int i = m * NSTEP + j, s = k_of(j);
        const bf16x8 ah = rh[i % D1], al = rl[i % D1];
        if (i + D1 < kSteps) { rh[i % D1] = frag(i + D1, 0); rl[i % D1] = frag(i + D1, 1); }
        const f32x16 z = {0};
        accs[m & 1] = mfma_x3(ah, al, Xh[s], Xl[s], j == 0 ? z : accs[m & 1]);
        if (!kOverlap && j == NSTEP - 1) {  // (wide dense pass: the tile's epilogue at once, one accumulator live)
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            const Bf16x2Split p = relu_split2(accs[m & 1][2 * q], accs[m & 1][2 * q + 1]);
            H1h[2 * m + (q >> 2)][q & 3] = p.hi;
            H1l[2 * m + (q >> 2)][q & 3] = p.lo;
          }
        }
        if (kOverlap && m > 0) {  // the previous tile's epilogue: 8 steps over NSTEP k-steps
#pragma unroll
          for (int q = (8 * j) / NSTEP; q < (8 * (j + 1)) / NSTEP; ++q) {
            const Bf16x2Split p = relu_split2(accs[(m - 1) & 1][2 * q], accs[(m - 1) & 1][2 * q + 1]);
            H1h[2 * (m - 1) + (q >> 2)][q & 3] = p.hi;
            H1l[2 * (m - 1) + (q >> 2)][q & 3] = p.lo;
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int q = 0; q < 8 * kOverlap; ++q) {
        const Bf16x2Split p = relu_split2(accs[1][2 * q], accs[1][2 * q + 1]);
        H1h[14 + (q >> 2)][q & 3] = p.hi;
        H1l[14 + (q >> 2)][q & 3] = p.lo;
      }
    };
    constexpr int ND_SPARSE = 2;
    if (KS1 > ND_SPARSE + 1 && n_data <= 1) layer1(std::integral_constant<int, (KS1 > ND_SPARSE + 1 ? 1 : KS1)>{});
    else if (KS1 > ND_SPARSE + 1 && n_data <= ND_SPARSE) layer1(std::integral_constant<int, (KS1 > ND_SPARSE + 1 ? ND_SPARSE : KS1)>{});
    else layer1(std::integral_constant<int, KS1>{});

    // ---- layer 2 + heads: H2^T = relu(W2 H1^T + b2), head^T += W3 H2^T ----
    f32x16 hd = {0};
    {
      constexpr int D2 = 2;  // hi fragments in flight (LDS)
      auto read_bias = [&](int m2) { return load_ctab(b2t, m2, h); };  // (a lambda on purpose, as data_steps)
      const unsigned char* const wb = w2s + lane * 16;
      auto w2hi = [&](int i) { return *reinterpret_cast<const bf16x8*>(wb + i * 1024); };
      bf16x8 hring[D2];
#pragma unroll
      for (int i = 0; i < D2; ++i) hring[i] = w2hi(i);
#pragma unroll
      for (int u = 0; u < DL; ++u) lring[u] = w2lo(u);
      accs[0] = read_bias(0);
      const unsigned char* const w3l = w3s + ((r < 3 ? r : 3) * 2 + h) * 16;  // (row 3 is zeros)
      auto w3f = [&](int t, int part) { return *reinterpret_cast<const bf16x8*>(w3l + t * 256 + part * 128); };
      u32x4 h2h[2], h2l[2];
      bf16x8 a3h, a3l;
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int m2 = 0; m2 < 8; ++m2) {
        f32x16& cur = accs[m2 & 1];
        f32x16& prev = accs[(m2 & 1) ^ 1];
#pragma unroll
        for (int t = 0; t < 16; ++t) {
          const int i = m2 * 16 + t;
          const bf16x8 ah = hring[i % D2], al = lring[i % DL];
          if (i + D2 < 128) hring[i % D2] = w2hi(i + D2);
          if (i + DL < 128) lring[i % DL] = w2lo(i + DL);
          cur = mfma_x3(ah, al, __builtin_bit_cast(bf16x8, H1h[t]), __builtin_bit_cast(bf16x8, H1l[t]), cur);
          if (m2 > 0 && t >= 1 && t <= 8) {  // the previous tile's epilogue, one packed pair per k-step
            const int q = t - 1;
            const Bf16x2Split p = relu_split2(prev[2 * q], prev[2 * q + 1]);
            h2h[q >> 2][q & 3] = p.hi;
            h2l[q >> 2][q & 3] = p.lo;
          }
          if (m2 > 0 && (t == 3 || t == 7)) {
            const int u = 2 * (m2 - 1) + (t == 7);
            a3h = w3f(u, 0); a3l = w3f(u, 1);
          }
          if (m2 > 0 && (t == 5 || t == 9)) {  // the previous tile's two head k-steps, each as soon as it is split
            const int q = t == 9;
            hd = mfma_x3(a3h, a3l, __builtin_bit_cast(bf16x8, h2h[q]), __builtin_bit_cast(bf16x8, h2l[q]), hd);
          }
          if (t == 14 && m2 < 7) prev = read_bias(m2 + 1);  // (the next tile's accumulator: its epilogue is done)
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      // the last tile's epilogue and head products
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const Bf16x2Split p = relu_split2(accs[1][2 * q], accs[1][2 * q + 1]);
        h2h[q >> 2][q & 3] = p.hi;
        h2l[q >> 2][q & 3] = p.lo;
      }
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        a3h = w3f(14 + q, 0); a3l = w3f(14 + q, 1);
        hd = mfma_x3(a3h, a3l, __builtin_bit_cast(bf16x8, h2h[q]), __builtin_bit_cast(bf16x8, h2l[q]), hd);
      }
    }
    asm volatile("" :: "v"(hd));
    // ---- rows 0..2 of a head tile sit in registers 0..2 of lanes 0..31: the lower half keeps the first pass's and
    // finishes those 32 rows after the second pass, when the upper half takes the second pass's ----
    if ((pass & 1) == 0) {
      zs0 = hd[0]; zs1 = hd[1]; zs2 = hd[2];
      continue;
    }
    const float o0 = __shfl_xor(hd[0], 32, 64), o1 = __shfl_xor(hd[1], 32, 64), o2 = __shfl_xor(hd[2], 32, 64);
    const float z0 = (h ? o0 : zs0) + head_bias.x, z1 = (h ? o1 : zs1) + head_bias.y, z2 = (h ? o2 : zs2) + head_bias.z;
    const int64_t row = W.chunk(pass) * 64 + lane;
    if (row < rows) {
      if (net == 0) finish_row(A.S, SC, row, z0, z1, z2);
      else A.S.val[row] = z0;
    }
  }
}

}  // namespace rvo3d
