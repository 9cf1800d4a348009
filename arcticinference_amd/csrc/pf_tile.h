// The 32-token tile step of the flash-attention bodies that work on 128 query rows per workgroup (four waves of two
// 16-row MFMA tiles): the chunked-prefill body (prefill_attn.hip) and the shared-prefix body (prefix_attn.hip).  One
// place for what they have in common: how a thread's 16-byte chunks of a K/V tile go into the LDS image (an fp8 cache
// converted exactly on the way), and one tile of S^T = K Q^T -> lazy-maximum soft-max -> O^T += V^T P^T with P carried
// as a 16-bit head + tail.  What differs between the bodies (where the pages come from, which keys a row sees) stays
// with them: the caller fetches the chunks, and passes the mask as a functor.
#pragma once

#include "attn_common.h"

namespace aic {

constexpr int kPfWaves = 4;
constexpr int kPfMT = 2;                        // 16-row MFMA tiles per wave
constexpr int kPfRows = kPfWaves * kPfMT * 16;  // query rows (token x head of the group) per workgroup
constexpr float kPfSlack = 6.0f;                // lazy maximum: a row's adopted maximum may trail the true one by 2^6

// D = head size: 128 (16-bit or fp8 cache) or 64 (16-bit cache).  E = the call's 16-bit element type.
template <int D, bool KV8, typename E>
struct PfTile {
  static_assert(D == 128 || (D == 64 && !KV8), "head size 128, or 64 with a 16-bit cache");
  using V8 = typename E::vec8;
  static constexpr int DT = D / 16;   // 16-wide output tiles
  static constexpr int NS = D / 32;   // k-steps of the 16x16x32 MFMA per S tile
  static constexpr int ES = KV8 ? 1 : 2;
  // a token row of one head is 128 bytes: one 16-byte chunk of K and of V per thread (else two of each)
  static constexpr bool ONE_CHUNK = KV8 || D == 64;
  static constexpr int kTileU4 = kTile * D / 8;   // uint4 per K (or V) tile image

  // what one of the 256 threads holds of a tile between its global loads and the LDS stores.  ONE_CHUNK: token tid / 8,
  // chunk tid % 8 in k0 / v0.  Else: tokens tid / 16 (k0, v0) and 16 + tid / 16 (k1, v1), chunk tid % 16.
  struct Regs {
    uint4 k0, k1, v0, v1;
  };

  static __device__ __forceinline__ void store(char* kt, char* vt, int tid, const Regs& r) {
    if constexpr (KV8) {
      const int ti = tid >> 3, ch = 2 * (tid & 7);
      *reinterpret_cast<V8*>(kt + v_tile_off(ti, ch)) = E::from_fp8(r.k0.x, r.k0.y);
      *reinterpret_cast<V8*>(kt + v_tile_off(ti, ch + 1)) = E::from_fp8(r.k0.z, r.k0.w);
      *reinterpret_cast<V8*>(vt + v_tile_off(ti, ch)) = E::from_fp8(r.v0.x, r.v0.y);
      *reinterpret_cast<V8*>(vt + v_tile_off(ti, ch + 1)) = E::from_fp8(r.v0.z, r.v0.w);
    } else if constexpr (D == 64) {
      const int ti = tid >> 3, ch = tid & 7;
      *reinterpret_cast<uint4*>(kt + tile_off<64>(ti, ch)) = r.k0;
      *reinterpret_cast<uint4*>(vt + tile_off<64>(ti, ch)) = r.v0;
    } else {
      const int ti = tid >> 4, ch = tid & 15;
      *reinterpret_cast<uint4*>(kt + v_tile_off(ti, ch)) = r.k0;
      *reinterpret_cast<uint4*>(kt + v_tile_off(16 + ti, ch)) = r.k1;
      *reinterpret_cast<uint4*>(vt + v_tile_off(ti, ch)) = r.v0;
      *reinterpret_cast<uint4*>(vt + v_tile_off(16 + ti, ch)) = r.v1;
    }
  }

  // One tile (images at kt / vt) against the wave's 32 rows; a wave-uniform call (the transposed reads need every lane).
  // qf: the rows' query fragments (B operand: lane (row c16, k-group g), d = 32 s + 8 g + j).  m_run (log2 units) / l_run
  // (this lane's share of the row's sum) / o_acc: the rows' running state.  mask(mt, sc): lane (c16, g) holds row c16's
  // raw scores of keys tile + 4 g + e (sc[e]) and tile + 16 + 4 g + e (sc[4 + e]); it sets what the row does not see
  // to -inf.
  template <typename Mask>
  static __device__ __forceinline__ void compute(const char* kt, const char* vt, int g, int c16,
                                                 const uint4 (&qf)[kPfMT][NS], float (&m_run)[kPfMT],
                                                 float (&l_run)[kPfMT], f32x4 (&o_acc)[kPfMT][DT], float scale_log2,
                                                 float inv_scale, Mask&& mask) {
    V8 kf[2][NS];  // A operand: key 16 th + c16, d = 32 s + 8 g + j
#pragma unroll
    for (int th = 0; th < 2; ++th)
#pragma unroll
      for (int s = 0; s < NS; ++s) kf[th][s] = *reinterpret_cast<const V8*>(kt + tile_off<D>(16 * th + c16, 4 * s + g));
    V8 pf[kPfMT], pl[kPfMT];  // P = head + tail (E each): one 16-bit P would put 2^-9 on every weight
#pragma unroll
    for (int mt = 0; mt < kPfMT; ++mt) {
      f32x4 a0 = f32x4{0.f, 0.f, 0.f, 0.f}, a1 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        a0 = E::mfma(kf[0][s], __builtin_bit_cast(V8, qf[mt][s]), a0);
        a1 = E::mfma(kf[1][s], __builtin_bit_cast(V8, qf[mt][s]), a1);
      }
      float sc[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        sc[e] = a0[e];
        sc[4 + e] = a1[e];
      }
      mask(mt, sc);
      float lmax = sc[0];
#pragma unroll
      for (int e = 1; e < 8; ++e) lmax = fmaxf(lmax, sc[e]);
      // raw score above which the row adopts a new maximum (-inf while nothing is visible: any finite score does)
      const float thr = __builtin_fmaf(m_run[mt], inv_scale, kPfSlack * inv_scale);
      if (__any(lmax > thr)) {
        const float m_new = fmaxf(m_run[mt], rowgroup_max(lmax) * scale_log2);
        const float m_to = m_new == -INFINITY ? 0.0f : m_new;
        const float alpha = __builtin_amdgcn_exp2f(m_run[mt] - m_to);
        m_run[mt] = m_new;
        l_run[mt] *= alpha;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) o_acc[mt][dt] *= alpha;
      }
      const float m_use = m_run[mt] == -INFINITY ? 0.0f : m_run[mt];
      float ls = 0.0f;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[e], scale_log2, -m_use));
        pf[mt][e] = E::head(p);
        pl[mt][e] = E::tail(p, pf[mt][e]);
        ls += p;
      }
      l_run[mt] += ls;
    }
    // O^T += V^T P^T: lane 4q+p of a 16-lane group supplies row q of the 4-token block, columns 4p..4p+3
    const int q4 = c16 >> 2, p4 = c16 & 3;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      const char* a_lo = vt + tile_off<D>(4 * g + q4, 2 * dt + (p4 >> 1)) + 8 * (p4 & 1);
      const char* a_hi = vt + tile_off<D>(16 + 4 * g + q4, 2 * dt + (p4 >> 1)) + 8 * (p4 & 1);
      const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(const_cast<char*>(a_lo)));
      const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(const_cast<char*>(a_hi)));
      typedef __attribute__((ext_vector_type(8))) short s16x8;
      const V8 vfrag = __builtin_bit_cast(V8, static_cast<s16x8>(__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7)));
#pragma unroll
      for (int mt = 0; mt < kPfMT; ++mt) {
        o_acc[mt][dt] = E::mfma(vfrag, pf[mt], o_acc[mt][dt]);
        o_acc[mt][dt] = E::mfma(vfrag, pl[mt], o_acc[mt][dt]);
      }
    }
  }
};

}  // namespace aic
