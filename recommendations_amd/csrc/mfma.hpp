// MFMA operand types, the two bf16 MFMA shapes and the LDS fragment reads shared by the
// matrix kernels (gemm, attention, towers, loss, retrieve, mlp).
//
// Only what two or more files use and what does not depend on an LDS layout belongs here.
// Swizzles, offset tables and staging routines stay in the file whose layout they encode;
// a call site computes its own addresses and hands them to the reads below.  The one image
// here, swz32 / ko32, is the 32x32x16 tile engine's, which loss.hip and retrieve.hip share.
#pragma once
#include "common.hpp"

namespace lthm {

// ---- operand types ----
typedef __bf16 bf16x8v __attribute__((ext_vector_type(8)));  // A / B operand of both bf16 MFMA shapes
typedef short s16x4 __attribute__((ext_vector_type(4)));     // what one transposed read returns
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));   // 32x32 accumulator

typedef __attribute__((address_space(3))) unsigned char lds_u8;

// ---- MFMA ----
__device__ __forceinline__ f32x16 mfma32(bf16x8v a, bf16x8v b, f32x16 c) {  // v_mfma_f32_32x32x16_bf16
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma16(bf16x8v a, bf16x8v b, f32x4 c) {  // v_mfma_f32_16x16x32_bf16
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// eight consecutive floats v[o] .. v[o + 7] (an array or an accumulator vector) packed to a
// bf16 operand; with o = 8 s, registers 8 s .. 8 s + 7 of a 32x32 accumulator as the
// fragment of k-step s
template <typename V>
__device__ __forceinline__ bf16x8v pack_frag(const V& v, int o) {
  const u32x4 w = {pack_bf16x2(v[o], v[o + 1]), pack_bf16x2(v[o + 2], v[o + 3]), pack_bf16x2(v[o + 4], v[o + 5]),
                   pack_bf16x2(v[o + 6], v[o + 7])};
  return __builtin_bit_cast(bf16x8v, w);
}

// ---- LDS fragment reads ----
// row fragment: the 16 bytes at p (8 consecutive k of one row) as an operand (ds_read_b128)
__device__ __forceinline__ bf16x8v frag_at(const unsigned char* p) {
  return __builtin_bit_cast(bf16x8v, *reinterpret_cast<const u32x4*>(p));
}
// transposed fragment: two ds_read_b64_tr_b16 (tr_half), lo / hi the lane's LDS byte addresses
// in the lower and the upper four k-rows of the fragment.  tr_frag(lo, hi) forms both
// addresses, then reads; a site that forms hi only after reading lo writes
// tr_frag(tr_half(lo), tr_half(hi)) and so keeps that instruction order (the scheduler's
// tie-breaks follow it).
__device__ __forceinline__ s16x4 tr_half(const lds_u8* p) {
  typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p);
}
__device__ __forceinline__ s16x4 tr_half(const unsigned char* p) { return tr_half((const lds_u8*)p); }
__device__ __forceinline__ bf16x8v tr_frag(s16x4 lo, s16x4 hi) {
  const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8v, v);
}
__device__ __forceinline__ bf16x8v tr_frag(const unsigned char* lo, const unsigned char* hi) {
  return tr_frag(tr_half(lo), tr_half(hi));
}

// The 32x32x16 tile engine's image (cdna_hip_programming.md T10, image (b)): chunk ch of
// row r at slot ch ^ swz32(r), conflict-free for the ds_read_b128 row fragments of the
// 32x32x16 A operand and for the ds_read_b64_tr_b16 transposed B fragments (each aligned
// quad of rows takes four distinct aligned blocks of four slots).
__device__ __forceinline__ int swz32(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }
__device__ __forceinline__ int ko32(int row, int ch) { return row * 256 + ((ch ^ swz32(row)) << 4); }

}  // namespace lthm
