// rvo3d_policy_rnn_tiles.hpp -- the biGRU actor-critic's policy step for the rows WITH velocity-obstacle rows, in
// 32-row tiles on the matrix cores (v_mfma_f32_32x32x16_bf16): the (bi)GRU over each row's vo_count VO rows, the
// direction sum, concat + LayerNorm, both 268 -> 256 -> 256 -> 3 / 1 stacks, then rvo3d_policy_rows' per-row tail
// (tanh, Philox sample with counter (row, step), log-probability, np.round(a, 2), the stores).
// Reference: train/policy/policy_rnn_ac.py:75-168 (rnn_Reader), :197-257 (GaussianActor, Critic), :57-69 (ac.step).
// Part of the gfx950 device code (see rvo3d_device.hpp for the overview).
//
// Input.  The device list rvo3d_reader_zero_features builds (row indices, count).  A first launch
// (rnn_tiles_bucket_kernel) sorts it into per-count sub-lists in a caller-owned work area - one region of max_rows
// entries per count 1..slots, a cursor per count -, so that a tile's recurrence runs exactly as long as its rows: a
// tile of single-VO-row rows does one input product per direction and no recurrent product at all.  The second launch
// (policy_rnn_tiles_kernel) is persistent: a fixed grid (one workgroup of four waves per CU), every wave takes tiles
// off the sub-lists, longest counts first, reading the cursors on the device.  The last workgroup out zeroes the
// cursors, the count and the finished-workgroups word.  No host synchronisation; the grid never depends on the count.
//
// Orientation (as rvo3d_policy_mlp.hpp).  Every product is computed TRANSPOSED - weights are the A operand, the tile's
// 32 rows the B operand's columns -, so a 32 x 32 result tile holds the batch row on the lane and 16 hidden units in
// the accumulator registers (unit 8 (i >> 2) + 4 h + (i & 3) of register i, lane half h).  The next product sums over
// those units: the converted accumulators ARE its B fragments, in the permuted k order mfma_k_perm(); the packed weights of
// every product that reads hidden units (W_hh, the hidden part of W1, W2, W3) are stored in that order.  So the GRU's
// hidden state, the features and both hidden layers never leave the registers: no LDS traffic between products.
//
// Weights.  Nothing is resident: W_hh alone is 384 KB per direction at hidden 256 and the two 268-wide first layers
// 272 KB, more than the 160 KB of LDS, and a wave reads every fragment exactly once per tile.  All of them stream from
// L2 as lane-linear 1 KB wave-loads (16 B per lane, coalesced), a fixed distance ahead of their MFMA.  The hidden state
// of the running direction is kept in LDS (float32, lane-linear, conflict-free), the forward direction's final state in
// registers while the reverse one runs.
// Precision.  The GRU's products (W_ih x, W_hh h) are split bf16 - a_hi b_hi + a_hi b_lo + a_lo b_hi, hi = bf16(v),
// lo = bf16(v - hi), as rvo3d_policy_mlp_x3.hpp does -: float32-class, so a row's many recurrent steps add no bf16 error
// of their own (with plain bf16 operands a 12-step row's mu was 2.5x further from the float32 module than the library
// GEMM path's).  The first step needs no recurrent product (h = 0).  The stacks behind the LayerNorm are bf16 operands
// with float32 accumulation, as the "heads" path's GEMMs; gate math, LayerNorm and the hidden state are float32.
// The X3 instantiations (rvo3d_policy_rnn_tiles_x3, float32 rollouts and evaluations) split the stacks as well: the
// LayerNorm output and the ReLU'd float32 sums of both hidden layers become hi and lo B fragments, W1 / W2 / W3 are packed
// as hi and lo blocks and go through mfma_x3_part - float32-class from end to end (mu and v within 1e-4 of a float64
// forward, where the bf16 stacks are 1e-3 off).  Their blob has its own magic word and size; a kernel given the other
// precision's blob computes nothing.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>
#include <utility>

#include "rvo3d_mfma_tiles.hpp"
#include "rvo3d_rollout_kernels.hpp"

namespace rvo3d {

constexpr int kRnnTilesMaxSlots = 12;
constexpr int kRnnTilesWaves = 4;         // waves per workgroup (independent: one tile each)
constexpr int kRnnTilesWorkHeader = 32;   // int32 cursors (count 1..slots) before the sub-lists
constexpr int32_t kRnnTilesMagic = 0x524e5431;
constexpr int32_t kRnnTilesMagicX3 = 0x524e5833;  // the float32-class blob (X3 = true below): its own word, its own size
constexpr int kRnnTilesHeadBytes = 64;

// byte offsets inside the blob (every section 16-byte aligned; one fragment = 64 lanes x 8 bf16 = 1 KB)
struct RnnTilesLayout {
  int64_t wih[2], whh[2], bih[2], bhn[2], ln_hg, ln_hb, ln_pg, ln_pb, w1[2], b1[2], w2[2], b2[2], w3[2], hb[2], total;
};
// X3: the stacks' weights as split fragments too (a hi 1 KB block followed by its lo block, as wih / whh)
__host__ __device__ inline RnnTilesLayout rnn_tiles_layout(int H, int ND, bool X3 = false) {
  const int HT = H / 32, KH = H / 16, KS1 = KH + 1, FB = X3 ? 2048 : 1024;
  RnnTilesLayout L{};
  int64_t o = kRnnTilesHeadBytes;
  for (int d = 0; d < 2; ++d) {
    const bool on = d < ND;
    L.wih[d] = o; o += on ? (int64_t)3 * HT * 2048 : 0;            // [gate, tile][hi, lo][lane][8]
    L.whh[d] = o; o += on ? (int64_t)3 * HT * KH * 2048 : 0;       // [gate, tile][k-step][hi, lo][lane][8]
    L.bih[d] = o; o += on ? (int64_t)3 * HT * 128 : 0;             // [gate, tile][h][16] float: b_i + b_h (r, z), b_in (n)
    L.bhn[d] = o; o += on ? (int64_t)HT * 128 : 0;                 // [tile][h][16] float: b_hn
  }
  L.ln_hg = o; o += (int64_t)HT * 128;                             // [tile][h][16] float
  L.ln_hb = o; o += (int64_t)HT * 128;
  L.ln_pg = o; o += 64;                                            // [16] float
  L.ln_pb = o; o += 64;
  for (int n = 0; n < 2; ++n) {
    L.w1[n] = o; o += (int64_t)8 * KS1 * FB;                       // [tile][k-step][lane][8]; k-step KH = the state
    L.b1[n] = o; o += 8 * 128;                                     // [tile][h][16] float
    L.w2[n] = o; o += (int64_t)8 * 16 * FB;
    L.b2[n] = o; o += 8 * 128;
    L.w3[n] = o; o += 16 * FB;                                     // [k-step][lane][8]: rows 0..2 (actor) / 0 (critic)
    L.hb[n] = o; o += 16;                                          // float[4]
  }
  L.total = o;
  return L;
}

// ---- packing: the modules' float32 tensors -> the blob ------------------------------------------------------------
struct RnnTilesPackArgs {
  int32_t H, ND, SD, IN;
  float eps;                                          // LayerNorm eps (header word 5)
  const float *w_ih[2], *w_hh[2], *b_ih[2], *b_hh[2];  // nn.GRU, gates r, z, n
  const float *ln_w, *ln_b;                           // [SD + H]
  const float *w1[2], *b1[2], *w2[2], *b2[2], *w3[2], *b3[2];
  unsigned char* blob;
};
template <bool X3>
__global__ void __launch_bounds__(256) rnn_tiles_pack_kernel(const RnnTilesPackArgs A) {
  const int H = A.H, HT = H / 32, KH = H / 16, KS1 = KH + 1, SD = A.SD, IN = A.IN, D = SD + H;
  const RnnTilesLayout L = rnn_tiles_layout(H, A.ND, X3);
  unsigned char* const b = A.blob;
  auto fl = [&](int64_t off, int64_t i, float v) { reinterpret_cast<float*>(b + off)[i] = v; };
  // a split fragment: element i of the logical [..][lane][8] array at 1 KB blocks 2 f (hi = bf16(v)) and 2 f + 1 (lo)
  auto split = [&](int64_t off, int64_t i, float v) {
    const int64_t at = ((i >> 9) << 10) + (i & 511);
    uint16_t hi, lo;
    bf16_split(v, hi, lo);
    reinterpret_cast<uint16_t*>(b + off)[at] = hi;
    reinterpret_cast<uint16_t*>(b + off)[at + 512] = lo;
  };
  // a fragment of the stacks: one bf16 block, or - X3 - split like the GRU's
  auto bf = [&](int64_t off, int64_t i, float v) {
    if constexpr (X3) split(off, i, v);
    else reinterpret_cast<uint16_t*>(b + off)[i] = f32_to_bf16_rne(v);
  };
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t0 < 16) reinterpret_cast<int32_t*>(b)[t0] = t0 == 0 ? (X3 ? kRnnTilesMagicX3 : kRnnTilesMagic) : t0 == 1 ? H : t0 == 2 ? SD : t0 == 3 ? A.ND : t0 == 4 ? IN : t0 == 5 ? __builtin_bit_cast(int32_t, A.eps) : 0;
  for (int d = 0; d < A.ND; ++d) {
    for (int64_t i = t0; i < (int64_t)3 * HT * 512; i += stride) {  // W_ih, columns IN..15 zero
      const int j = i & 7, lane = (i >> 3) & 63, gm = (int)(i >> 9), g = gm / HT, m = gm % HT;
      const int u = g * H + 32 * m + (lane & 31), k = 8 * (lane >> 5) + j;
      split(L.wih[d], i, k < IN ? A.w_ih[d][(int64_t)u * IN + k] : 0.f);
    }
    for (int64_t i = t0; i < (int64_t)3 * HT * 32; i += stride) {
      // r and z: b_ih + b_hh both enter the pre-activation; n: b_ih only (b_hn sits inside r * (.))
      const int reg = i & 15, h = (i >> 4) & 1, gm = (int)(i >> 5), g = gm / HT, m = gm % HT;
      const int u = g * H + 32 * m + mlp_acc_row(reg, h);
      fl(L.bih[d], i, A.b_ih[d][u] + (g < 2 ? A.b_hh[d][u] : 0.f));
    }
    for (int64_t i = t0; i < (int64_t)3 * HT * KH * 512; i += stride) {
      const int j = i & 7, lane = (i >> 3) & 63, t = (int)((i >> 9) % KH), gm = (int)((i >> 9) / KH), g = gm / HT, m = gm % HT;
      const int u = g * H + 32 * m + (lane & 31);
      split(L.whh[d], i, A.w_hh[d][(int64_t)u * H + mfma_k_perm(t, lane >> 5, j)]);
    }
    for (int64_t i = t0; i < (int64_t)HT * 32; i += stride) {
      const int reg = i & 15, h = (i >> 4) & 1, m = (int)(i >> 5);
      fl(L.bhn[d], i, A.b_hh[d][2 * H + 32 * m + mlp_acc_row(reg, h)]);
    }
  }
  for (int64_t i = t0; i < (int64_t)HT * 32; i += stride) {
    const int reg = i & 15, h = (i >> 4) & 1, m = (int)(i >> 5), u = SD + 32 * m + mlp_acc_row(reg, h);
    fl(L.ln_hg, i, A.ln_w[u]);
    fl(L.ln_hb, i, A.ln_b[u]);
  }
  if (t0 < 16) { fl(L.ln_pg, t0, t0 < SD ? A.ln_w[t0] : 0.f); fl(L.ln_pb, t0, t0 < SD ? A.ln_b[t0] : 0.f); }
  for (int n = 0; n < 2; ++n) {
    const int n_out = n == 0 ? 3 : 1;
    for (int64_t i = t0; i < (int64_t)8 * KS1 * 512; i += stride) {  // W1: k-steps 0..KH-1 the hidden part, KH the state
      const int j = i & 7, lane = (i >> 3) & 63, s = (int)((i >> 9) % KS1), m = (int)((i >> 9) / KS1);
      const int row = 32 * m + (lane & 31), h = lane >> 5;
      const int col = s < KH ? SD + mfma_k_perm(s, h, j) : (8 * h + j < SD ? 8 * h + j : -1);
      bf(L.w1[n], i, col >= 0 ? A.w1[n][(int64_t)row * D + col] : 0.f);
    }
    for (int64_t i = t0; i < 8 * 16 * 512; i += stride) {
      const int j = i & 7, lane = (i >> 3) & 63, t = (int)((i >> 9) & 15), m = (int)(i >> 13);
      bf(L.w2[n], i, A.w2[n][(32 * m + (lane & 31)) * 256 + mfma_k_perm(t, lane >> 5, j)]);
    }
    for (int64_t i = t0; i < 8 * 32; i += stride) {
      const int reg = i & 15, h = (i >> 4) & 1, m = (int)(i >> 5), u = 32 * m + mlp_acc_row(reg, h);
      fl(L.b1[n], i, A.b1[n][u]);
      fl(L.b2[n], i, A.b2[n][u]);
    }
    for (int64_t i = t0; i < 16 * 512; i += stride) {
      const int j = i & 7, lane = (i >> 3) & 63, t = (int)(i >> 9), row = lane & 31;
      bf(L.w3[n], i, row < n_out ? A.w3[n][row * 256 + mfma_k_perm(t, lane >> 5, j)] : 0.f);
    }
    if (t0 < 4) fl(L.hb[n], t0, t0 < n_out ? A.b3[n][t0] : 0.f);
  }
}

// ---- sort the list into per-count sub-lists -------------------------------------------------------------------------
struct RnnTilesArgs {
  const unsigned char* blob;
  const float* obs; int64_t obs_ld;
  const int32_t* cnt; const int32_t* list; int32_t* count; int32_t* done_blocks;
  int32_t* work; int64_t max_rows;      // [kRnnTilesWorkHeader + slots * max_rows]; rows of obs / cnt / the outputs
  int32_t SD, slots;
  PolicySampleArgs S;
};
__global__ void __launch_bounds__(256) rnn_tiles_bucket_kernel(const RnnTilesArgs A) {
  const int64_t n = *A.count;
  const int64_t n_use = n < A.max_rows ? n : A.max_rows;
  const int lane = threadIdx.x & 63;
  // one atomic per wave and count, not per row (a dense world lists thousands of rows, most of one count: per-row
  // atomics on that one cursor took ~100 us); the rank inside the wave comes from the ballot
  for (int64_t i0 = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~63); i0 < n_use; i0 += (int64_t)gridDim.x * 256) {
    const int64_t i = i0 + lane;
    int32_t row = i < n_use ? A.list[i] : -1;
    if (row >= A.max_rows) row = -1;  // (not a row of this call: left alone)
    int c = 0;
    if (row >= 0) {
      c = A.cnt[row];
      c = c < 1 ? 1 : (c > A.slots ? A.slots : c);
    }
    for (int q = 1; q <= A.slots; ++q) {
      const uint64_t m = __ballot(c == q);
      if (m == 0) continue;
      const int leader = __ffsll((unsigned long long)m) - 1;
      int base = 0;
      if (lane == leader) base = atomicAdd(A.work + (q - 1), __popcll(m));
      base = __shfl(base, leader, 64);
      const int pos = base + __popcll(m & ((1ull << lane) - 1));
      // (a work area that was not zero before the call could push a cursor past its region: clamped here and in the
      // tiles kernel)
      if (c == q && pos < A.max_rows) A.work[kRnnTilesWorkHeader + (int64_t)(q - 1) * A.max_rows + pos] = row;
    }
  }
}

__device__ __forceinline__ int64_t min_i64(int64_t a, int64_t b) { return a < b ? a : b; }
__device__ __forceinline__ float sigmoid_fast(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
// One flat stream of N weight fragments (1 KB each, lane-linear) through the MFMAs of `body(i, a)`: fragment i + D is
// requested before MFMA i, and a scheduling barrier per MFMA keeps the compiler from hoisting the whole stream (it
// would, and spill).  off(i): the fragment's byte offset in the blob.  The stream is expanded at compile time (a pack
// expansion, not a loop: a 408-step loop exceeds the unroller's budget, and a rolled loop would index the register
// arrays - hidden state, fragments - dynamically, i.e. through scratch), so every index is a constant.
template <int D, int N, class Off, class Body, int... I>
__device__ __forceinline__ void frag_stream_seq(const unsigned char* base, Off& off, Body& body,
                                                std::integer_sequence<int, I...>) {
  bf16x8 ring[D];
#pragma unroll
  for (int i = 0; i < D && i < N; ++i) ring[i] = ld_blob<bf16x8>(base + off(i));
  (
      [&]() RVO3D_INLINE {
        constexpr int i = I;
        const bf16x8 a = ring[i % D];
        if constexpr (i + D < N) ring[i % D] = ld_blob<bf16x8>(base + off(i + D));
        body(std::integral_constant<int, i>{}, a);
        __builtin_amdgcn_sched_barrier(0);
      }(),
      ...);
}
template <int D, int N, class Off, class Body>
__device__ __forceinline__ void frag_stream(const unsigned char* base, Off off, Body body) {
  frag_stream_seq<D, N>(base, off, body, std::make_integer_sequence<int, N>{});
}
constexpr int kRnnTilesDepth = 16;  // fragments in flight per wave

// ---- the policy step of the listed rows ------------------------------------------------------------------------------
// H: reader hidden width (64 or 256), ND: directions (1 GRU, 2 biGRU).  One wave = one 32-row tile at a time.
// X3: the stacks behind the LayerNorm in split bf16 as well (float32-class from end to end), on a blob packed for it.
template <int H, int ND, bool X3 = false>
__global__ void __launch_bounds__(64 * kRnnTilesWaves) policy_rnn_tiles_kernel(const RnnTilesArgs A) {
  constexpr int HT = H / 32, KH = H / 16, KS1 = KH + 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // the running direction's hidden state, float32, in LDS (VGPRs are short: fragments, accumulators and the state's
  // bf16 operand copy live there): [tile][register / 4][lane] float4, lane-linear
  float4* const hst = reinterpret_cast<float4*>(smem) + wave * HT * 4 * 64;
  const RnnTilesLayout L = rnn_tiles_layout(H, ND, X3);
  const unsigned char* const blob0 = A.blob;
  const int32_t* const hdr = reinterpret_cast<const int32_t*>(blob0);
  const bool shape_ok = hdr[0] == (X3 ? kRnnTilesMagicX3 : kRnnTilesMagic) && hdr[1] == H && hdr[2] == A.SD && hdr[3] == ND;
  const SampleConsts SC = sample_consts(A.S);
  // tiles per count, longest counts first
  int ntile[kRnnTilesMaxSlots], total = 0;
#pragma unroll
  for (int c = 0; c < kRnnTilesMaxSlots; ++c) {
    int v = c < A.slots ? __builtin_amdgcn_readfirstlane(A.work[c]) : 0;
    v = v < 0 ? 0 : (v > A.max_rows ? (int)A.max_rows : v);
    ntile[c] = (v + 31) >> 5;
    total += ntile[c];
  }
  if (!shape_ok) total = 0;
  const int gw = blockIdx.x * kRnnTilesWaves + wave, nw = gridDim.x * kRnnTilesWaves;

#pragma unroll 1
  for (int tile = gw; tile < total; tile += nw) {
    int c = 0, j = tile;  // sub-list c (count c + 1), tile j of it
#pragma unroll
    for (int q = kRnnTilesMaxSlots - 1; q >= 0; --q) {
      if (q < A.slots && c == 0 && j >= 0) {
        if (j < ntile[q]) { c = q + 1; } else { j -= ntile[q]; }
      }
    }
    const int n = c;  // every row of the tile has this many VO rows (the tile's recurrence length)
    const int32_t* const sub = A.work + kRnnTilesWorkHeader + (int64_t)(n - 1) * A.max_rows;
    const int e = 32 * j + r;
    const bool valid = e < min_i64(__builtin_amdgcn_readfirstlane(A.work[n - 1]), A.max_rows);
    const int64_t row = sub[valid ? e : 32 * j];  // (an empty lane re-reads the tile's first row; nothing is stored)
    const float* const orow = A.obs + row * A.obs_ld;
    const unsigned char* blob = blob0;
    asm volatile("" : "+s"(blob));  // (as in the recurrence)

    // ---- the (bi)GRU: forward over VO rows 0..n-1, reverse over n-1..0; final states summed ----
    f32x16 hs[HT], hfw[HT];  // the final sum; the forward direction's final state (biGRU)
    // (one expansion per direction: which array a direction writes, and where its weights are, are compile-time facts)
    auto direction = [&](auto d_tag) RVO3D_INLINE {
      constexpr int d = decltype(d_tag)::value;
#pragma unroll
      for (int k = 0; k < HT * 4; ++k) hst[k * 64 + lane] = float4{0.f, 0.f, 0.f, 0.f};
      u32x4 hf[KH], hl[KH];  // the state as B fragments: hi and lo bf16 halves
#pragma unroll 1
      for (int s = 0; s < n; ++s) {
        const int pos = d == 0 ? s : n - 1 - s;
        // x as the B fragment: k 0..8 the VO row, zeros behind
        f32x8 xv;
        const float* xp = orow + A.SD + pos * 9;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int k = 8 * h + q;
          xv[q] = k < 9 ? xp[k < 9 ? k : 0] : 0.0f;
        }
        // (split8's arithmetic, written element by element: with split8 itself this kernel's registers are allocated
        // differently; the same holds for split_bf16x2 and the state fragments below)
        const bf16x8 X = __builtin_convertvector(xv, bf16x8);
        f32x8 xr;
#pragma unroll
        for (int q = 0; q < 8; ++q) xr[q] = xv[q] - (float)X[q];
        const bf16x8 XL = __builtin_convertvector(xr, bf16x8);
        // per unit tile m: the three input fragments (r, z, n), then - from the second step on - the recurrent ones
        // (k-step t: r, z, n); the gate math of tile m rides behind its last MFMA
        // (the blob's address made opaque per step: otherwise every weight / bias load, being loop-invariant, is hoisted
        // out of the step and tile loops - hundreds of registers, spilled)
        const unsigned char* blob = blob0;
        asm volatile("" : "+s"(blob));
        const unsigned char* const bt = blob + L.bih[d];
        const unsigned char* const base = blob + lane * 16;
        const int64_t o_ih = L.wih[d], o_hh = L.whh[d];
        f32x16 ar, az, an, ahn;
        auto gates = [&](int m) RVO3D_INLINE {
#pragma unroll
          for (int q = 0; q < 4; ++q) {  // nn.GRU: r, z, n = tanh(i_n + r (W_hn h + b_hn)), h' = (1 - z) n + z h
            float4 hv = hst[(m * 4 + q) * 64 + lane];
            float* const hp = reinterpret_cast<float*>(&hv);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const int i = 4 * q + u;
              const float rg = sigmoid_fast(ar[i]), zg = sigmoid_fast(az[i]);
              const float ng = tanh_fast(an[i] + rg * ahn[i]);
              hp[u] = (1.0f - zg) * ng + zg * hp[u];
            }
            hst[(m * 4 + q) * 64 + lane] = hv;
          }
        };
        auto step = [&](auto rec_tag) RVO3D_INLINE {
          constexpr bool REC = decltype(rec_tag)::value;
          constexpr int PER = REC ? 6 + 6 * KH : 6;  // fragments per unit tile: (gate, k-step) x (hi, lo)
          // every product is split bf16, a fragment at a time (mfma_x3_part)
          frag_stream<kRnnTilesDepth, HT * PER>(
              base,
              [&](int i) RVO3D_INLINE -> int64_t {
                const int m = i / PER, q = i % PER;
                if (q < 6) return o_ih + (int64_t)((q >> 1) * HT + m) * 2048 + (q & 1) * 1024;
                const int f = (q - 6) >> 1, t = f / 3, g = f % 3;
                return o_hh + (int64_t)((g * HT + m) * KH + t) * 2048 + (q & 1) * 1024;
              },
              [&](auto ic, const bf16x8& a) RVO3D_INLINE {
                constexpr int i = decltype(ic)::value, m = i / PER, q = i % PER, part = q & 1;
                if constexpr (q == 0) {
                  ar = load_ctab_global(bt, m, h);
                  az = load_ctab_global(bt, HT + m, h);
                  an = load_ctab_global(bt, 2 * HT + m, h);
                  ahn = load_ctab_global(blob + L.bhn[d], m, h);
                }
                if constexpr (q < 6) {
                  constexpr int g = q >> 1;
                  mfma_x3_part(g == 0 ? ar : g == 1 ? az : an, a, part, X, XL);
                } else {
                  constexpr int f = (q - 6) >> 1, t = f / 3, g = f % 3;
                  mfma_x3_part(g == 0 ? ar : g == 1 ? az : ahn, a, part, __builtin_bit_cast(bf16x8, hf[t]),
                               __builtin_bit_cast(bf16x8, hl[t]));
                }
                if constexpr (q == PER - 1) gates(m);
              });
        };
        // (from h = 0 the recurrent product is zero: the first step has none)
        if (s == 0) step(std::integral_constant<bool, false>{});
        else step(std::integral_constant<bool, true>{});
        if (s + 1 < n) {  // the new state as the next step's B fragments (hi / lo; the state itself stays float32)
#pragma unroll
          for (int m = 0; m < HT; ++m)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const float4 hv = hst[(m * 4 + q) * 64 + lane];
              const uint32_t p0 = pack_bf16x2(hv.x, hv.y), p1 = pack_bf16x2(hv.z, hv.w);
              hf[2 * m + (q >> 1)][2 * (q & 1)] = p0;
              hf[2 * m + (q >> 1)][2 * (q & 1) + 1] = p1;
              const bf16x2 b0 = __builtin_bit_cast(bf16x2, p0), b1 = __builtin_bit_cast(bf16x2, p1);
              hl[2 * m + (q >> 1)][2 * (q & 1)] = pack_bf16x2(hv.x - (float)b0[0], hv.y - (float)b0[1]);
              hl[2 * m + (q >> 1)][2 * (q & 1) + 1] = pack_bf16x2(hv.z - (float)b1[0], hv.w - (float)b1[1]);
            }
        }
      }
#pragma unroll
      for (int m = 0; m < HT; ++m)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 hv = hst[(m * 4 + q) * 64 + lane];
          const float v4[4] = {hv.x, hv.y, hv.z, hv.w};
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            if constexpr (ND == 2 && d == 0) hfw[m][4 * q + u] = v4[u];  // (kept while the reverse direction runs)
            else hs[m][4 * q + u] = (ND == 2 ? hfw[m][4 * q + u] : 0.f) + v4[u];
          }
        }
    };
    direction(std::integral_constant<int, 0>{});
    if constexpr (ND == 2) direction(std::integral_constant<int, 1>{});

    // ---- LayerNorm(concat(p, hsum)): the row's units sit in lanes r and r + 32 ----
    float p[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) p[k] = k < A.SD ? orow[k] : 0.f;
    float s1 = 0.f;
#pragma unroll
    for (int m = 0; m < HT; ++m)
#pragma unroll
      for (int i = 0; i < 16; ++i) s1 += hs[m][i];
    s1 += __shfl_xor(s1, 32, 64);
#pragma unroll
    for (int k = 0; k < 16; ++k) s1 += p[k];
    const float Df = (float)(A.SD + H);
    const float mean = s1 / Df;
    float s2 = 0.f;
#pragma unroll
    for (int m = 0; m < HT; ++m)
#pragma unroll
      for (int i = 0; i < 16; ++i) { const float dv = hs[m][i] - mean; s2 += dv * dv; }
    s2 += __shfl_xor(s2, 32, 64);
#pragma unroll
    for (int k = 0; k < 16; ++k) if (k < A.SD) { const float dv = p[k] - mean; s2 += dv * dv; }
    const float rstd = 1.0f / __builtin_sqrtf(s2 / Df + __builtin_bit_cast(float, hdr[5]));
    if constexpr (X3) {
      // ---- float32-class stacks: every operand hi / lo, every product mfma_x3_part, one fixed summation order ----
      // The features' hidden k-steps go to LDS as split B fragments, [k-step][hi, lo][lane]: the state area is dead
      // once the recurrence is over and exactly that large, and a lane reads back only what it wrote itself (no
      // barrier).  Both stacks re-read them; the state k-step stays in registers.
      u32x4* const fl = reinterpret_cast<u32x4*>(hst);
#pragma unroll
      for (int m = 0; m < HT; ++m) {
        const f32x16 g = load_ctab_global(blob + L.ln_hg, m, h), bb = load_ctab_global(blob + L.ln_hb, m, h);
        u32x4 fh[2], fo[2];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const Bf16x2Split sp = split_bf16x2((hs[m][2 * q] - mean) * rstd * g[2 * q] + bb[2 * q],
                                              (hs[m][2 * q + 1] - mean) * rstd * g[2 * q + 1] + bb[2 * q + 1]);
          fh[q >> 2][q & 3] = sp.hi;
          fo[q >> 2][q & 3] = sp.lo;
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          fl[(2 * (2 * m + t)) * 64 + lane] = fh[t];
          fl[(2 * (2 * m + t) + 1) * 64 + lane] = fo[t];
        }
      }
      u32x4 fsh, fsl;  // the state k-step
      {
        float pg[16], pb[16];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const f32x4 g4 = ld_blob<f32x4>(blob + L.ln_pg + 16 * k), b4 = ld_blob<f32x4>(blob + L.ln_pb + 16 * k);
#pragma unroll
          for (int u = 0; u < 4; ++u) { pg[4 * k + u] = g4[u]; pb[4 * k + u] = b4[u]; }
        }
        f32x8 fv;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const float pk = h ? p[8 + q] : p[q];
          fv[q] = 8 * h + q < A.SD ? (pk - mean) * rstd * pg[8 * h + q] + pb[8 * h + q] : 0.f;
        }
        bf16x8 sh, sl;
        split8(fv, sh, sl);
        fsh = __builtin_bit_cast(u32x4, sh);
        fsl = __builtin_bit_cast(u32x4, sl);
      }
#pragma unroll 1
      for (int net = 0; net < 2; ++net) {
        const unsigned char* blob = blob0;
        asm volatile("" : "+s"(blob));  // (as in the recurrence)
        const unsigned char* const base = blob + lane * 16;
        // (every offset of this net read once, here: L is indexed by a runtime net, i.e. it lives in scratch, and a
        // bias table fetched by L.b1[net] inside a stream is a scratch read between its MFMAs)
        const int64_t o1 = L.w1[net], o2 = L.w2[net], o3 = L.w3[net], ob1 = L.b1[net], ob2 = L.b2[net], ohb = L.hb[net];
        // The second layer is summed over k as the first layer produces it: unit tile m of H1 (two k-steps, split after
        // the ReLU) goes straight into all eight output tiles of the second layer, whose accumulators are kept - so H1
        // is never held whole (hi and lo of 16 k-steps would be 128 registers next to the fragment ring).  Per output
        // element the k-steps still come in ascending order, hi-hi, hi-lo, lo-hi each.
        constexpr int PER1 = 2 * KS1, PER = PER1 + 32;  // fragments per unit tile: W1's, then W2's (tile, k-step, hi / lo)
        f32x16 acc, acc2[8];
        u32x4 bh, bl, h1h[2], h1l[2];
        frag_stream<kRnnTilesDepth, 8 * PER>(
            base,
            [&](int i) RVO3D_INLINE -> int64_t {
              const int m = i / PER, q = i % PER;
              if (q < PER1) return o1 + (int64_t)(m * PER1 + q) * 1024;
              const int j = q - PER1, m2 = j >> 2, t = (j >> 1) & 1;
              return o2 + (int64_t)((m2 * 16 + 2 * m + t) * 2 + (j & 1)) * 1024;
            },
            [&](auto ic, const bf16x8& a) RVO3D_INLINE {
              constexpr int i = decltype(ic)::value, m = i / PER, q = i % PER;
              if constexpr (q < PER1) {
                constexpr int s1 = q >> 1, part = q & 1;
                if constexpr (q == 0) acc = load_ctab_global(blob + ob1, m, h);
                if constexpr (part == 0) {
                  if constexpr (s1 < KH) { bh = fl[(2 * s1) * 64 + lane]; bl = fl[(2 * s1 + 1) * 64 + lane]; }
                  else { bh = fsh; bl = fsl; }
                }
                mfma_x3_part(acc, a, part, __builtin_bit_cast(bf16x8, bh), __builtin_bit_cast(bf16x8, bl));
                if constexpr (q == PER1 - 1) {
#pragma unroll
                  for (int k = 0; k < 8; ++k) {
                    const Bf16x2Split sp = split_bf16x2(relu_f32(acc[2 * k]), relu_f32(acc[2 * k + 1]));
                    h1h[k >> 2][k & 3] = sp.hi;
                    h1l[k >> 2][k & 3] = sp.lo;
                  }
                }
              } else {
                constexpr int j = q - PER1, m2 = j >> 2, t = (j >> 1) & 1, part = j & 1;
                if constexpr (m == 0 && t == 0 && part == 0) acc2[m2] = load_ctab_global(blob + ob2, m2, h);
                mfma_x3_part(acc2[m2], a, part, __builtin_bit_cast(bf16x8, h1h[t]), __builtin_bit_cast(bf16x8, h1l[t]));
              }
            });
        // the head: output tile m2 of the second layer, ReLU, split, its two k-steps
        f32x16 hd = {0};
        u32x4 h2h[2], h2l[2];
        frag_stream<kRnnTilesDepth, 32>(
            base, [&](int i) RVO3D_INLINE -> int64_t { return o3 + (int64_t)i * 1024; },
            [&](auto ic, const bf16x8& a) RVO3D_INLINE {
              constexpr int i = decltype(ic)::value, m2 = i >> 2, t = (i >> 1) & 1, part = i & 1;
              if constexpr ((i & 3) == 0) {
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                  const Bf16x2Split sp = split_bf16x2(relu_f32(acc2[m2][2 * k]), relu_f32(acc2[m2][2 * k + 1]));
                  h2h[k >> 2][k & 3] = sp.hi;
                  h2l[k >> 2][k & 3] = sp.lo;
                }
              }
              mfma_x3_part(hd, a, part, __builtin_bit_cast(bf16x8, h2h[t]), __builtin_bit_cast(bf16x8, h2l[t]));
            });
        const f32x4 hb4 = ld_blob<f32x4>(blob + ohb);
        if (h == 0 && valid) {
          if (net == 0) finish_row(A.S, SC, row, hd[0] + hb4[0], hd[1] + hb4[1], hd[2] + hb4[2]);
          else A.S.val[row] = hd[0] + hb4[0];
        }
      }
    } else {
      u32x4 F[KS1];  // the features as the B fragments of the first layers
  #pragma unroll
      for (int m = 0; m < HT; ++m) {
        const f32x16 g = load_ctab_global(blob + L.ln_hg, m, h), bb = load_ctab_global(blob + L.ln_hb, m, h);
  #pragma unroll
        for (int q = 0; q < 8; ++q)
          F[2 * m + (q >> 2)][q & 3] = pack_bf16x2((hs[m][2 * q] - mean) * rstd * g[2 * q] + bb[2 * q],
                                                   (hs[m][2 * q + 1] - mean) * rstd * g[2 * q + 1] + bb[2 * q + 1]);
      }
      {
        float pg[16], pb[16];
  #pragma unroll
        for (int k = 0; k < 4; ++k) {
          const f32x4 g4 = ld_blob<f32x4>(blob + L.ln_pg + 16 * k), b4 = ld_blob<f32x4>(blob + L.ln_pb + 16 * k);
  #pragma unroll
          for (int u = 0; u < 4; ++u) { pg[4 * k + u] = g4[u]; pb[4 * k + u] = b4[u]; }
        }
        f32x8 fv;
  #pragma unroll
        for (int q = 0; q < 8; ++q) {
          const float pk = h ? p[8 + q] : p[q];
          fv[q] = 8 * h + q < A.SD ? (pk - mean) * rstd * pg[8 * h + q] + pb[8 * h + q] : 0.f;
        }
        F[KH] = __builtin_bit_cast(u32x4, __builtin_convertvector(fv, bf16x8));
      }

      // ---- the two stacks: relu(W1 f + b1) -> relu(W2 . + b2) -> W3 . + b3 ----
  #pragma unroll 1
      for (int net = 0; net < 2; ++net) {
        const unsigned char* blob = blob0;
        asm volatile("" : "+s"(blob));  // (as in the recurrence)
        const unsigned char* const base = blob + lane * 16;
        const int64_t o1 = L.w1[net], o2 = L.w2[net], o3 = L.w3[net];
        u32x4 H1[16];
        f32x16 acc;
        frag_stream<kRnnTilesDepth, 8 * KS1>(
            base, [&](int i) RVO3D_INLINE -> int64_t { return o1 + (int64_t)i * 1024; },
            [&](auto ic, const bf16x8& a) RVO3D_INLINE {
              constexpr int i = decltype(ic)::value, m = i / KS1, s1 = i % KS1;
              acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, __builtin_bit_cast(bf16x8, F[s1]),
                                                            s1 == 0 ? load_ctab_global(blob + L.b1[net], m, h) : acc, 0, 0, 0);
              if constexpr (s1 == KS1 - 1) {
  #pragma unroll
                for (int q = 0; q < 8; ++q) H1[2 * m + (q >> 2)][q & 3] = pack_bf16x2(relu_f32(acc[2 * q]), relu_f32(acc[2 * q + 1]));
              }
            });
        // second layer (16 k-steps per tile) with the head's two k-steps of the tile behind it: 18 fragments per tile
        f32x16 hd = {0};
        u32x4 h2[2];
        frag_stream<kRnnTilesDepth, 8 * 18>(
            base,
            [&](int i) RVO3D_INLINE -> int64_t {
              const int m = i / 18, q = i % 18;
              return q < 16 ? o2 + (int64_t)(m * 16 + q) * 1024 : o3 + (int64_t)(2 * m + q - 16) * 1024;
            },
            [&](auto ic, const bf16x8& a) RVO3D_INLINE {
              constexpr int i = decltype(ic)::value, m = i / 18, q = i % 18;
              if constexpr (q < 16) {
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, __builtin_bit_cast(bf16x8, H1[q]),
                                                              q == 0 ? load_ctab_global(blob + L.b2[net], m, h) : acc, 0, 0, 0);
                if constexpr (q == 15) {
  #pragma unroll
                  for (int k = 0; k < 8; ++k) h2[k >> 2][k & 3] = pack_bf16x2(relu_f32(acc[2 * k]), relu_f32(acc[2 * k + 1]));
                }
              } else {
                hd = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, __builtin_bit_cast(bf16x8, h2[q - 16]), hd, 0, 0, 0);
              }
            });
        // head rows 0..2 sit in registers 0..2 of lanes 0..31
        const f32x4 hb4 = ld_blob<f32x4>(blob + L.hb[net]);
        const float4 hb = {hb4[0], hb4[1], hb4[2], hb4[3]};
        if (h == 0 && valid) {
          if (net == 0) finish_row(A.S, SC, row, hd[0] + hb.x, hd[1] + hb.y, hd[2] + hb.z);
          else A.S.val[row] = hd[0] + hb.x;
        }
      }
    }
  }
  // the last workgroup out resets the sub-lists' cursors, the list's count and its own counter for the next step
  __syncthreads();
  if (tid == 0) {
    __threadfence();
    if (atomicAdd(A.done_blocks, 1) == (int)gridDim.x - 1) {
      for (int c = 0; c < kRnnTilesWorkHeader; ++c) A.work[c] = 0;
      *A.count = 0;
      *A.done_blocks = 0;
      __threadfence();
    }
  }
}

}  // namespace rvo3d
