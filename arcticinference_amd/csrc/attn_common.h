// Device helpers shared by the attention bodies (verify_attn.hip: decode / verify, prefill_attn.hip: chunked prefill):
// MFMA fragment types, the 32-token KV tile image read both row-wise and transposed, the fp8 -> 16-bit converts, the
// 16-bit element types the bodies are instantiated for (bf16 | f16) and the 4-lane row reductions of the S^T layout.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace aic {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) short s16x4;

// The block table is read-only for the kernels: addressed through the constant address space with wave-uniform
// indices its lookups become scalar loads (s_load_dword, lgkmcnt) and stay out of the vector-memory queue, where
// a dependent lookup between data loads would force the in-order vmcnt to drain every load issued before it.
typedef const int32_t __attribute__((address_space(4)))* const_i32_ptr;

constexpr int kTile = 32;  // tokens per inner step

// 16-byte load of KV bytes, non-temporal: every byte of the cache is read once per call, and with the default
// policy the stream evicts itself through the L2 (measured on the B = 64 x 4096-token case: 190.7 -> 171.0 us per
// call, 5.63 -> 6.28 TB/s).
typedef __attribute__((ext_vector_type(4))) unsigned u32x4_t;
__device__ __forceinline__ uint4 ld_kv16(const char* p) {
  const u32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(p));
  return make_uint4(v.x, v.y, v.z, v.w);
}

// Byte offset of 16-byte chunk `ch` (0..15) of token `t` (0..31) in the wave's V tile.  256-byte rows with
// the chunk index XOR-ed by a function of the row (cdna guide T10, image (b)), and token groups 4-7 /
// 8-11 swapped between rows so that the two 4-row blocks a 32-lane half reads transposed sit 8 rows
// apart: both the ds_write_b128 fill and the ds_read_b64_tr_b16 reads are then bank-conflict free.
__device__ __forceinline__ int v_tile_off(int t, int ch) {
  const int row = (t & ~12) | ((t & 4) << 1) | ((t & 8) >> 1);
  return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
}

// Image of a 32-token tile for head size D: D = 128 is v_tile_off; D = 64 (128-byte rows, 8 chunks) XORs the chunk
// with the row (the secondary head size: correct and DMA-fillable first, bank-optimal second).
template <int D>
__device__ __forceinline__ int tile_off(int t, int ch) {
  if constexpr (D == 128) {
    return v_tile_off(t, ch);
  } else {
    return 128 * t + 16 * (ch ^ (t & 7));
  }
}

// Lanes c16 + 16 g (g = 0..3) hold the same query row.  gfx950's row / half swaps combine them on the VALU
// (ds_bpermute costs an LDS round trip per step, and the long-draft kernel is VALU/latency bound).  The
// s_nops are the VALU-write -> permlane-swap -> VALU-read hazards the assembler does not see inside asm.
__device__ __forceinline__ void swap16(float& a, float& b) {
  asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 0" : "+v"(a), "+v"(b));
}
__device__ __forceinline__ void swap32(float& a, float& b) {
  asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 0" : "+v"(a), "+v"(b));
}

__device__ __forceinline__ float rowgroup_max(float x) {
  float a = x, b = x;
  swap16(a, b);
  a = a > b ? a : b;
  b = a;
  swap32(a, b);
  return a > b ? a : b;
}
__device__ __forceinline__ float rowgroup_sum(float x) {
  float a = x, b = x;
  swap16(a, b);
  a += b;
  b = a;
  swap32(a, b);
  return a + b;
}

// 8 e4m3 bytes (two dwords) -> 8 bf16 (exact: every e4m3 value is a bf16 value).  gfx950's scaled converts take two
// fp8 to two bf16 in ONE instruction (v_cvt_scalef32_pk_bf16_fp8, scale 1.0): 4 VALU per 8 elements where the
// fp8 -> f32 -> bf16 route took 8.  SQ counters on the fp8 short body (profiles/r02_pmc_secondary_kernels.txt): 70.8 % of
// its wave cycles were instruction issue (bf16 body: 32 %), 1.15e8 VALU instructions for half the bytes of the bf16
// body's 8.3e7 — the conversion made it issue-bound.
__device__ __forceinline__ bf16x8 fp8x8_to_bf16x8(uint32_t lo, uint32_t hi) {
  typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
  const bf16x2_t a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(static_cast<int>(lo), 1.0f, false);
  const bf16x2_t b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(static_cast<int>(lo), 1.0f, true);
  const bf16x2_t c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(static_cast<int>(hi), 1.0f, false);
  const bf16x2_t d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(static_cast<int>(hi), 1.0f, true);
  return __builtin_shufflevector(__builtin_shufflevector(a, b, 0, 1, 2, 3), __builtin_shufflevector(c, d, 0, 1, 2, 3), 0, 1,
                                 2, 3, 4, 5, 6, 7);
}

// The same for an f16 body (v_cvt_scalef32_pk_f16_fp8, scale 1.0).  Exact too: e4m3 spans 2^-9 .. 448 with 4 significant
// bits, inside f16's normal range (2^-14 .. 65504, 11 bits).
__device__ __forceinline__ f16x8 fp8x8_to_f16x8(uint32_t lo, uint32_t hi) {
  typedef __attribute__((ext_vector_type(2))) _Float16 f16x2_t;
  const f16x2_t a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(static_cast<int>(lo), 1.0f, false);
  const f16x2_t b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(static_cast<int>(lo), 1.0f, true);
  const f16x2_t c = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(static_cast<int>(hi), 1.0f, false);
  const f16x2_t d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(static_cast<int>(hi), 1.0f, true);
  return __builtin_shufflevector(__builtin_shufflevector(a, b, 0, 1, 2, 3), __builtin_shufflevector(c, d, 0, 1, 2, 3), 0, 1,
                                 2, 3, 4, 5, 6, 7);
}

// The 16-bit element type of a call: q, out, a 16-bit cache and the tile images an fp8 cache is converted into all have
// it.  Everything that moves bytes (loads, LDS-DMA, transposed LDS reads, paging, masks) is the same code for both; an
// attention body takes one of these as its last template argument for the four places where the type matters: the MFMA,
// the fp8 -> 16-bit tile conversion, the P operand (p = head + tail, both of the type) and the rounding of the output
// (round-to-nearest-even, one hardware convert each).
struct ElemBf16 {
  typedef __bf16 elem;
  typedef bf16x8 vec8;
  static __device__ __forceinline__ f32x4 mfma(vec8 a, vec8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ vec8 from_fp8(uint32_t lo, uint32_t hi) { return fp8x8_to_bf16x8(lo, hi); }
  static __device__ __forceinline__ elem head(float p) { return static_cast<__bf16>(p); }
  static __device__ __forceinline__ void pin(vec8&) {}
  static __device__ __forceinline__ elem tail(float p, elem h) { return static_cast<__bf16>(p - static_cast<float>(h)); }
  static __device__ __forceinline__ uint16_t round(float f) { return __builtin_bit_cast(uint16_t, static_cast<__bf16>(f)); }
};
struct ElemF16 {
  typedef _Float16 elem;
  typedef f16x8 vec8;
  static __device__ __forceinline__ f32x4 mfma(vec8 a, vec8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ vec8 from_fp8(uint32_t lo, uint32_t hi) { return fp8x8_to_f16x8(lo, hi); }
  static __device__ __forceinline__ elem head(float p) { return static_cast<_Float16>(p); }
  // long-draft body: the packed heads of a row tile are final before its tails are formed.  Left to itself the scheduler
  // interleaves the f16 -> f32 converts of the tails with the heads' packing, and the 256-VGPR body then keeps two
  // values in scratch across its tile loop; with this the f16 form needs 254 registers and no scratch.
  static __device__ __forceinline__ void pin(vec8& x) { asm volatile("" : "+v"(x)); }
  static __device__ __forceinline__ elem tail(float p, elem h) { return static_cast<_Float16>(p - static_cast<float>(h)); }
  static __device__ __forceinline__ uint16_t round(float f) { return __builtin_bit_cast(uint16_t, static_cast<_Float16>(f)); }
};

constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

}  // namespace aic
