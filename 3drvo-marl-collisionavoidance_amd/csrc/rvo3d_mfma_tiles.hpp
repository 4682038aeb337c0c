// rvo3d_mfma_tiles.hpp -- what the three matrix-core policy kernels (rvo3d_policy_mlp.hpp, rvo3d_policy_mlp_x3.hpp,
// rvo3d_policy_rnn_tiles.hpp) rest on, each written once: the vector types of v_mfma_f32_32x32x16_bf16's operands, the
// accumulator and k maps of chained TRANSPOSED products, the ReLU, the bf16 pack and hi / lo split, the split product
// and the read of a per-tile float table.  The packs and the kernels must agree on these bit for bit.
// Part of the gfx950 device code (see rvo3d_device.hpp for the overview).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rvo3d_rollout_kernels.hpp"

namespace rvo3d {

#define RVO3D_INLINE __attribute__((always_inline))  // for lambdas: inlined before the optimiser runs, like the functions here

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// hidden unit (within a 32-unit tile) that accumulator register i of lane half h holds
__host__ __device__ constexpr int mlp_acc_row(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }
// The permuted k order between chained products: k index of element j of lane half h in k-step t of a product that
// sums over the previous product's units - the unit that product's converted accumulator holds there (see
// mlp_acc_row).  Every packed weight that multiplies hidden units is stored in this order.
__host__ __device__ constexpr int mfma_k_perm(int t, int h, int j) {
  return 32 * (t >> 1) + 16 * (t & 1) + 8 * (j >> 2) + 4 * h + (j & 3);
}

__device__ __forceinline__ float relu_f32(float x) {
  // ONE instruction beside the MFMAs (v_max_i32: as integers, negative floats are negative, positive ones keep their
  // order).  fmaxf / fmed3 cost two - the compiler canonicalises the operand first -, and inline asm is out: the
  // compiler pads the MFMA -> VALU read hazard for its own instructions only.
  const int i = __builtin_bit_cast(int, x);
  return __builtin_bit_cast(float, i > 0 ? i : 0);
}
__device__ __forceinline__ uint32_t pack_bf16x2(float a, float b) {
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{a, b}, bf16x2));
}

// ---- the hi / lo split of float32-class products: hi = bf16_rne(v), lo = bf16_rne(v - hi) ----
__device__ __forceinline__ void bf16_split(float v, uint16_t& hi, uint16_t& lo) {
  hi = f32_to_bf16_rne(v);
  lo = f32_to_bf16_rne(v - __builtin_bit_cast(float, (uint32_t)hi << 16));
}
__device__ __forceinline__ void split8(const f32x8& v, bf16x8& hi, bf16x8& lo) {
  hi = __builtin_convertvector(v, bf16x8);
  const f32x8 vh = __builtin_convertvector(hi, f32x8);
  lo = __builtin_convertvector(v - vh, bf16x8);
}
// two floats into one packed hi pair and one packed lo pair
struct Bf16x2Split { uint32_t hi, lo; };
__device__ __forceinline__ Bf16x2Split split_bf16x2(float x, float y) {
  const uint32_t hi = pack_bf16x2(x, y);
  const float xh = __builtin_bit_cast(float, hi << 16), yh = __builtin_bit_cast(float, hi & 0xffff0000u);
  return Bf16x2Split{hi, pack_bf16x2(x - xh, y - yh)};
}
// The three products of one split k-step into acc: a_hi b_hi + a_lo b_hi + a_hi b_lo (the dropped a_lo b_lo is below
// 2^-16 of the product).  Two forms, because float32 sums depend on their order and each kernel keeps its own:
// mfma_x3 for a kernel that holds both halves of A (hh, lh, hl); mfma_x3_part for one that streams them one fragment
// at a time - part 0, the hi fragment, adds hh then hl; part 1, the lo fragment, adds lh.
__device__ __forceinline__ f32x16 mfma_x3(const bf16x8& ah, const bf16x8& al, const bf16x8& bh, const bf16x8& bl,
                                          const f32x16& c) {
  f32x16 acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, c, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
}
__device__ __forceinline__ void mfma_x3_part(f32x16& acc, const bf16x8& a, int part, const bf16x8& bh,
                                             const bf16x8& bl) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bh, acc, 0, 0, 0);
  if (part == 0) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bl, acc, 0, 0, 0);
}

// ---- a [tile][lane half][16] float table (a bias, a LayerNorm gain) as the accumulator-shaped f32x16 of tile m ----
__device__ __forceinline__ f32x16 load_ctab(const float* tab, int m, int h) {  // tab: in LDS
  f32x16 b;
  const float4* bp = reinterpret_cast<const float4*>(tab + (m * 2 + h) * 16);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 v = bp[q];
    b[4 * q] = v.x; b[4 * q + 1] = v.y; b[4 * q + 2] = v.z; b[4 * q + 3] = v.w;
  }
  return b;
}
// A load from a weight blob through a GLOBAL pointer: where the blob's address passes an empty asm (see
// policy_rnn_tiles_kernel) it comes out a generic one, whose flat loads the compiler can only wait for all together
// (vmcnt and lgkmcnt both to 0) - that would drain the fragment pipeline at every MFMA.  So the global variant of the
// table read below cannot share the generic-pointer one above.
// (T: a clang vector type - HIP's float4 is a class whose copy constructor takes a generic reference: flat again)
template <class T>
__device__ __forceinline__ T ld_blob(const unsigned char* p) {
  return *(const __attribute__((address_space(1))) T*)(p);
}
__device__ __forceinline__ f32x16 load_ctab_global(const unsigned char* p, int m, int h) {
  f32x4 q[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] = ld_blob<f32x4>(p + (m * 2 + h) * 64 + 16 * k);
  f32x16 v;
#pragma unroll
  for (int k = 0; k < 16; ++k) v[k] = q[k >> 2][k & 3];
  return v;
}

}  // namespace rvo3d
