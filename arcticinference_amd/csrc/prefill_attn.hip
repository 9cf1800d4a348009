// Chunked-prefill paged attention (requests with q_len > MAX_SPEC_LEN + 1 = 33) and aic_step_attention, the one call
// that serves a whole engine step: decodes and long drafts through the verify bodies (verify_attn.hip), prefill chunks
// through the body below.
//
// Reference path: every step goes through one attention call of vLLM's backend, whatever its query lengths
// (the reference's arctic_inference/vllm/ulysses.py:510).  Semantics are those of aic_verify_attention (and of
// oracle/spec_oracle.py verify_attention): query i of a request sits at position seq_len - q_len + i and sees keys
// 0 .. its position; the new K/V are already in the cache.
//
// Roofline: MFMA.  A 2048-token chunk at a 4096-token context (Llama-3.1-8B, Hq 32, Hkv 8) is 1.0e11 FLOP against
// 2 x 8 x 4096 x 256 B = 16.8 MB of KV: ~6000 FLOP/B, far over the ridge.  So the body is a flash-attention forward:
//   * one workgroup = 4 waves = 128 query rows of one (request, kv head); the G query heads of the kv head are packed
//     into the rows (row = token * G + head of the group), so a K/V tile is read once for all of them;
//   * K/V go through LDS in 32-token tiles (bf16 image; an fp8 cache is converted on the way in, exactly), double
//     buffered with one barrier per tile: the next tile's global loads are in flight while the current one is computed;
//   * S^T = K Q^T, as in the verify bodies: a lane holds 8 keys of ONE query row, so the soft-max is lane-local plus two
//     permlane swaps, and the scores are directly the B operand of O^T = V^T P^T (V read transposed, ds_read_b64_tr_b16);
//   * lazy running maximum (kept while no score exceeds it by 2^6), running max / sum in f32; P goes into P.V as a bf16
//     head + bf16 tail (p = hi + lo to 2^-17), as in the verify bodies: a single bf16 P misses the 1e-3 bar on short
//     contexts (measured: 6.8e-3 at q_len = ctx = 34), at the price of a third more MFMA issue;
//   * a workgroup walks K/V only up to its last row's position; only tiles that cross a wave's first row are masked;
//   * workgroups are dispatched last query block first (the blocks with the most keys), and the kv head is the fastest
//     index, so with Hkv = 8 every block of one head lands on the same XCD (workgroups are dealt round-robin over 8)
//     and re-reads its K/V through that XCD's L2;
//   * a call with fewer workgroups than CUs (a short chunk, an SP = 8 slice with one kv head) splits the key range and
//     merges the partials in a second launch, as the decode path does.
// gpt-oss layers (aic_step_attention_win): head size 64 halves the Q / K fragments and the output tiles and uses the
// verify bodies' 128-byte-row tile image (tile_off<64>); a sliding window starts a workgroup's key range at the tile of
// its first row's first key and adds a lower edge to the mask; a sink is the (max, sum) = (sink, 1) start of split 0.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "aic_common.h"
#include "attn_common.h"
#include "pf_tile.h"

namespace aic {
namespace {

// (workgroup shape — kPfWaves, kPfMT, kPfRows — and the tile step itself: pf_tile.h, shared with prefix_attn.hip)
constexpr int kPfTargetWgs = 256;               // below this many workgroups a call splits its key ranges (MI355X: 256 CUs)
constexpr int kPfMaxSplits = 16;
constexpr int kPfMinSplitTiles = 8;             // at least 256 keys per split

struct PrefillParams {
  const uint16_t* q;
  const char* k_cache;
  const char* v_cache;
  const int32_t* block_table;
  const int32_t* seq_lens;
  const int32_t* query_start_loc;
  const int32_t* reqs;   // prefill request ids (device)
  const float* k_scale;  // fp8 cache: per-tensor scales (device scalars)
  const float* v_scale;
  uint16_t* out;
  float* ws_o;   // split mode: [n_splits][n_wg][kPfRows][head size] unnormalised partials
  float* ws_ml;  // [n_splits][n_wg][kPfRows][2] {max (natural log units), sum}
  int64_t q_stride;
  int64_t out_stride;
  int64_t block_stride;  // elements
  int max_blocks;
  int num_q_heads;
  int num_kv_heads;
  int block_size;
  int bs_shift;  // log2(block_size) for powers of two, else -1
  int n_req;
  int n_qb;      // query blocks per request (of the longest)
  int n_wg;      // n_req * n_qb * num_kv_heads
  int n_splits;
  float sm_scale;
  // gpt-oss layers, as in the verify bodies.  window > 0: query position p sees keys p - window + 1 .. p only.  sinks
  // (f32 [num_q_heads] or null): one extra logit per head, the initial (max, sum = 1) state of split 0 of every row.
  int window;
  const float* sinks;
};

// workgroup index (without the split) -> (kv head, request slot, query block): kv head fastest, last query block first
struct PfItem {
  int h, ridx, qb;
};
__device__ __forceinline__ PfItem pf_item(const PrefillParams& P, int wgi) {
  PfItem it;
  it.h = wgi % P.num_kv_heads;
  const int rest = wgi / P.num_kv_heads;
  it.ridx = rest % P.n_req;
  it.qb = P.n_qb - 1 - rest / P.n_req;
  return it;
}

// D = head size: 128 (bf16 or fp8 cache) or 64 (bf16 cache; the verify bodies' rule).  WIN: the layer has a sliding
// window (P.window > 0).  Without one the window terms fold away and the tile loop is the plain causal one: they cost
// the D = 128 body ~2.5 % when kept as runtime tests (measured on the Llama-8B 2048-token chunk at ctx 4096).
// E = the call's 16-bit element type (attn_common.h: ElemBf16 | ElemF16): q, out, a 16-bit cache and the tile images.
template <int D, bool KV8, bool WIN, typename E = ElemBf16>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) prefill_attn_kernel(PrefillParams P) {
  static_assert(D == 128 || (D == 64 && !KV8), "head size 128, or 64 with a 16-bit cache");
  using T = PfTile<D, KV8, E>;
  constexpr int DT = T::DT, NS = T::NS, ES = T::ES;
  constexpr bool ONE_CHUNK = T::ONE_CHUNK;
  // [buffer][K, V] 32-token tiles in the verify bodies' image (tile_off<D>): read row-wise for K, transposed for V
  __shared__ uint4 lds[2][2][T::kTileU4];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, c16 = lane & 15;
  const int wgi = blockIdx.x / P.n_splits;
  const int split = blockIdx.x - wgi * P.n_splits;
  const PfItem it = pf_item(P, wgi);
  const int Hkv = P.num_kv_heads, G = P.num_q_heads / Hkv, h = it.h;
  const int req = __builtin_amdgcn_readfirstlane(P.reqs[it.ridx]);
  const int q0 = __builtin_amdgcn_readfirstlane(P.query_start_loc[req]);
  const int q_len = __builtin_amdgcn_readfirstlane(P.query_start_loc[req + 1]) - q0;
  const int ctx = __builtin_amdgcn_readfirstlane(P.seq_lens[req]);
  const int n_rows = q_len * G;
  const int blk_row0 = it.qb * kPfRows;
  if (blk_row0 >= n_rows) return;  // a shorter request of the call: no such block (whole workgroup)
  const int ctx0 = ctx - q_len;    // position of the request's first query token
  const int kv_end = ctx0 + (min(blk_row0 + kPfRows, n_rows) - 1) / G + 1;  // keys the block's last row sees
  const int wnd = WIN ? P.window : (1 << 30);
  // sliding window: the block's first row sees nothing below key ctx0 + blk_row0 / G - window + 1, nor does any later row
  const int key_lo = WIN ? max(0, ctx0 + blk_row0 / G - wnd + 1) : 0;
  const int tile_lo = key_lo / kTile;
  const int tiles = (kv_end + kTile - 1) / kTile;
  const int tps = (tiles - tile_lo + P.n_splits - 1) / P.n_splits;
  const int t_first = tile_lo + split * tps, t_last = min(tiles, t_first + tps);

  // this wave's rows: keys up to w_lim_lo are visible to all of them, none beyond w_lim_hi to any; with a window, keys
  // at or below w_lim_lo - window are visible to none of them, keys above w_lim_hi - window to all
  const int w_row0 = blk_row0 + wave * (kPfMT * 16);
  const bool wave_live = w_row0 < n_rows;
  const int w_lim_lo = ctx0 + w_row0 / G;
  const int w_lim_hi = ctx0 + (min(w_row0 + kPfMT * 16, n_rows) - 1) / G;

  // ---- query fragments (B operand of S^T = K Q^T): lane (row c16, k-group g), d = 32 s + 8 g + j ------------
  // ---- and the row state: (max, sum) = (-inf, 0), or (sink, 1) in split 0 of a layer with sinks
  uint4 qf[kPfMT][NS];
  int lim[kPfMT];  // last key a lane's row sees (the first is lim - window + 1)
  float m_run[kPfMT], l_run[kPfMT];
  f32x4 o_acc[kPfMT][DT];
#pragma unroll
  for (int mt = 0; mt < kPfMT; ++mt) {
    const int rc = min(w_row0 + mt * 16 + c16, n_rows - 1);
    const int pos = rc / G, gq = rc - pos * G;
    lim[mt] = ctx0 + pos;
    const uint16_t* qrow = P.q + static_cast<int64_t>(q0 + pos) * P.q_stride + static_cast<int64_t>(h * G + gq) * D;
#pragma unroll
    for (int s = 0; s < NS; ++s) qf[mt][s] = *reinterpret_cast<const uint4*>(qrow + 32 * s + 8 * g);
    m_run[mt] = -INFINITY;
    l_run[mt] = 0.0f;
    if (P.sinks != nullptr && split == 0) {
      m_run[mt] = P.sinks[h * G + gq] * kLog2e;  // log2 units, like the scaled scores; not multiplied by sm_scale
      l_run[mt] = g == 0 ? 1.0f : 0.0f;          // l_run is this lane's share of the row's sum: one lane carries the 1
    }
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o_acc[mt][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const float scale_log2 = P.sm_scale * kLog2e * (KV8 ? *P.k_scale : 1.0f);
  const float inv_scale = 1.0f / scale_log2;
  const float out_scale = KV8 ? *P.v_scale : 1.0f;

  // ---- tile staging: bf16 D = 128 = two 16-byte chunks of K and of V per thread (tokens t/16 and 16 + t/16, chunk
  // t%16); fp8 = one of each (token t/8, 8-byte halves of chunk t%8 -> bf16 chunks 2 (t%8), 2 (t%8) + 1); bf16 D = 64 =
  // one of each (token t/8, chunk t%8).  A 16-token group never straddles two pages (block_size is a multiple of 16):
  // its page lookup is one scalar per group.
  const int64_t kv_row = static_cast<int64_t>(Hkv) * D;  // elements between consecutive tokens of a page
  const unsigned row_bytes = static_cast<unsigned>(kv_row) * ES;
  const_i32_ptr btab = (const_i32_ptr)(P.block_table + static_cast<int64_t>(req) * P.max_blocks);
  const int last_group = (ctx - 1) & ~15;
  const int tid = threadIdx.x;
  typename T::Regs r;
  auto group_base = [&](int first) -> int64_t {   // element offset of token `first` of kv head h
    const unsigned f = static_cast<unsigned>(first), bs = static_cast<unsigned>(P.block_size);
    const unsigned pg = P.bs_shift >= 0 ? f >> P.bs_shift : f / bs;
    const unsigned po = f - pg * bs;
    return static_cast<int64_t>(btab[pg]) * P.block_stride + static_cast<int64_t>(po) * kv_row + h * D;
  };
  auto load_tile = [&](int tt) {
    const int f0 = min(tt, last_group), f1 = min(tt + 16, last_group);
    const int64_t b0 = group_base(f0), b1 = group_base(f1);
    if (ONE_CHUNK) {
      const int ti = tid >> 3, ch = tid & 7;
      const int first = ti < 16 ? f0 : f1;
      const int64_t base = ti < 16 ? b0 : b1;
      const unsigned off = static_cast<unsigned>(min(tt + ti, ctx - 1) - first);
      const size_t byte = static_cast<size_t>(base) * ES + __umul24(off, row_bytes) + 16u * ch;
      r.k0 = ld_kv16(P.k_cache + byte);
      r.v0 = ld_kv16(P.v_cache + byte);
    } else {
      const int ti = tid >> 4, ch = tid & 15;
      const unsigned off0 = static_cast<unsigned>(min(tt + ti, ctx - 1) - f0);
      const unsigned off1 = static_cast<unsigned>(min(tt + 16 + ti, ctx - 1) - f1);
      const size_t y0 = static_cast<size_t>(b0) * 2 + __umul24(off0, row_bytes) + 16u * ch;
      const size_t y1 = static_cast<size_t>(b1) * 2 + __umul24(off1, row_bytes) + 16u * ch;
      r.k0 = ld_kv16(P.k_cache + y0);
      r.k1 = ld_kv16(P.k_cache + y1);
      r.v0 = ld_kv16(P.v_cache + y0);
      r.v1 = ld_kv16(P.v_cache + y1);
    }
  };
  // V of keys below every row's window (the first tile of a windowed range) is staged as zeros: their weights are 0,
  // and a page that lies wholly below the windows may then hold anything, NaN included, without reaching the output
  auto store_tile = [&](int buf, int tt) {
    char* kt = reinterpret_cast<char*>(lds[buf][0]);
    char* vt = reinterpret_cast<char*>(lds[buf][1]);
    if (WIN && tt < key_lo) {
      const uint4 z = make_uint4(0, 0, 0, 0);
      if (ONE_CHUNK) {
        if (tt + (tid >> 3) < key_lo) r.v0 = z;
      } else {
        if (tt + (tid >> 4) < key_lo) r.v0 = z;
        if (tt + 16 + (tid >> 4) < key_lo) r.v1 = z;
      }
    }
    T::store(kt, vt, tid, r);
  };

  // one 32-token tile against the wave's 32 rows (wave-uniform call: the transposed reads need every lane)
  auto compute_tile = [&](int buf, int tt) {
    // the tile crosses the causal edge of a row of the wave, or (window) holds a key at or below a row's lim - window
    const bool need_mask = tt + kTile - 1 > w_lim_lo || (WIN && tt <= w_lim_hi - wnd);
    T::compute(reinterpret_cast<const char*>(lds[buf][0]), reinterpret_cast<const char*>(lds[buf][1]), g, c16, qf, m_run, l_run,
               o_acc, scale_log2, inv_scale, [&](int mt, float (&sc)[8]) {
                 if (need_mask) {
#pragma unroll
                   for (int e = 0; e < 8; ++e) {
                     const int key = tt + 16 * (e >> 2) + 4 * g + (e & 3);
                     if (key > lim[mt] || (WIN && key <= lim[mt] - wnd)) sc[e] = -INFINITY;
                   }
                 }
               });
  };

  if (t_first < t_last) {
    load_tile(t_first * kTile);
    store_tile(0, t_first * kTile);
    __syncthreads();
    for (int t = t_first; t < t_last; ++t) {
      const int buf = (t - t_first) & 1;
      const int tt = t * kTile;
      const bool more = t + 1 < t_last;
      if (more) load_tile(tt + kTile);                        // in flight during the tile's MFMAs
      // tiles past all of the wave's rows, or below all of their windows: nothing to do
      if (wave_live && tt <= w_lim_hi && (!WIN || tt + kTile - 1 > w_lim_lo - wnd)) compute_tile(buf, tt);
      if (more) store_tile(buf ^ 1, tt + kTile);                          // last read in the previous iteration, before its barrier
      __syncthreads();
    }
  }
  if (!wave_live) return;

#pragma unroll
  for (int mt = 0; mt < kPfMT; ++mt) {
    const float l = rowgroup_sum(l_run[mt]);
    const int rr = w_row0 + mt * 16 + c16;
    if (rr >= n_rows) continue;
    const int pos = rr / G, gq = rr - pos * G;
    if (P.n_splits == 1) {
      const float inv = l > 0.0f ? out_scale / l : 0.0f;
      uint16_t* op = P.out + static_cast<int64_t>(q0 + pos) * P.out_stride + static_cast<int64_t>(h * G + gq) * D + 4 * g;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const uint32_t lo = static_cast<uint32_t>(E::round(o_acc[mt][dt][0] * inv)) |
                            (static_cast<uint32_t>(E::round(o_acc[mt][dt][1] * inv)) << 16);
        const uint32_t hi = static_cast<uint32_t>(E::round(o_acc[mt][dt][2] * inv)) |
                            (static_cast<uint32_t>(E::round(o_acc[mt][dt][3] * inv)) << 16);
        *reinterpret_cast<uint2*>(op + dt * 16) = make_uint2(lo, hi);
      }
    } else {
      const int64_t slot = (static_cast<int64_t>(split) * P.n_wg + wgi) * kPfRows + (rr - blk_row0);
      float* op = P.ws_o + slot * D + 4 * g;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
        *reinterpret_cast<float4*>(op + dt * 16) = make_float4(o_acc[mt][dt][0] * out_scale, o_acc[mt][dt][1] * out_scale,
                                                               o_acc[mt][dt][2] * out_scale, o_acc[mt][dt][3] * out_scale);
      if (g == 0) *reinterpret_cast<float2*>(P.ws_ml + slot * 2) = make_float2(m_run[mt] * kLn2, l);
    }
  }
}

// Merge of the split partials: one wave per row of the prefill grid (lane = two elements of the head dimension; D = 64
// leaves the upper half of the wave idle).
template <int D, typename E = ElemBf16>
__global__ void __launch_bounds__(256) prefill_combine_kernel(PrefillParams P) {
  const int lane = threadIdx.x & 63;
  if (2 * lane >= D) return;
  const int64_t row = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  const int wgi = static_cast<int>(row / kPfRows), r = static_cast<int>(row - static_cast<int64_t>(wgi) * kPfRows);
  if (wgi >= P.n_wg) return;
  const PfItem it = pf_item(P, wgi);
  const int G = P.num_q_heads / P.num_kv_heads;
  const int req = P.reqs[it.ridx];
  const int q0 = P.query_start_loc[req], q_len = P.query_start_loc[req + 1] - q0;
  const int rr = it.qb * kPfRows + r;
  if (rr >= q_len * G) return;
  const int pos = rr / G, gq = rr - pos * G;
  float M = -INFINITY;
  for (int s = 0; s < P.n_splits; ++s)
    M = fmaxf(M, P.ws_ml[((static_cast<int64_t>(s) * P.n_wg + wgi) * kPfRows + r) * 2]);
  float L = 0.0f, acc0 = 0.0f, acc1 = 0.0f;
  for (int s = 0; s < P.n_splits; ++s) {
    const int64_t slot = (static_cast<int64_t>(s) * P.n_wg + wgi) * kPfRows + r;
    const float2 ml = *reinterpret_cast<const float2*>(P.ws_ml + slot * 2);
    if (ml.x == -INFINITY) continue;  // a split whose keys this row does not see
    const float w = __expf(ml.x - M);
    const float2 o = *reinterpret_cast<const float2*>(P.ws_o + slot * D + 2 * lane);
    L += w * ml.y;
    acc0 += w * o.x;
    acc1 += w * o.y;
  }
  const float inv = L > 0.0f ? 1.0f / L : 0.0f;
  uint16_t* op = P.out + static_cast<int64_t>(q0 + pos) * P.out_stride + static_cast<int64_t>(it.h * G + gq) * D + 2 * lane;
  *reinterpret_cast<uint32_t*>(op) =
      static_cast<uint32_t>(E::round(acc0 * inv)) | (static_cast<uint32_t>(E::round(acc1 * inv)) << 16);
}

// Rows of the decode part of a mixed step: gather (dst[i] = src[index[i]]) or scatter (dst[index[i]] = src[i]) of
// `row_bytes` (a multiple of 16) per row.
__global__ void __launch_bounds__(256) step_rows_kernel(const char* __restrict__ src, int64_t src_stride_bytes,
                                                        char* __restrict__ dst, int64_t dst_stride_bytes,
                                                        const int32_t* __restrict__ index, int row_bytes, int scatter) {
  const int i = blockIdx.x;
  const int64_t t = index[i];
  const int64_t s_row = scatter ? i : t, d_row = scatter ? t : i;
  for (int b = 16 * threadIdx.x; b < row_bytes; b += 16 * blockDim.x)
    *reinterpret_cast<uint4*>(dst + d_row * dst_stride_bytes + b) =
        *reinterpret_cast<const uint4*>(src + s_row * src_stride_bytes + b);
}

// Geometry of the prefill grid of a call: workgroups without the split, and the split count.  The workspace query
// (which knows no context length, nor the window) takes the largest split count the call could choose.  With a sliding
// window a workgroup reads at most window + its kPfRows / G tokens + one tile of rounding, whatever the context: the
// split count follows that key count.
struct PfGrid {
  int n_qb, n_wg, n_splits;
};
PfGrid pf_grid(int n_prefill, int max_prefill_q_len, int num_q_heads, int num_kv_heads, int max_seq_len, int window = 0) {
  PfGrid gr;
  const int G = num_q_heads / num_kv_heads;
  gr.n_qb = static_cast<int>((static_cast<int64_t>(max_prefill_q_len) * G + kPfRows - 1) / kPfRows);
  gr.n_wg = n_prefill * gr.n_qb * num_kv_heads;
  gr.n_splits = 1;
  if (max_seq_len > 0 && window > 0) max_seq_len = std::min(max_seq_len, window + kPfRows / G + kTile);
  if (gr.n_wg < kPfTargetWgs) {
    int s = std::min(kPfMaxSplits, kPfTargetWgs / std::max(1, gr.n_wg));
    if (max_seq_len > 0) s = std::min(s, std::max(1, (max_seq_len + kTile - 1) / kTile / kPfMinSplitTiles));
    gr.n_splits = std::max(1, s);
  }
  return gr;
}

size_t pf_partial_bytes(const PfGrid& gr, int head_size) {
  if (gr.n_splits <= 1) return 0;
  const size_t slots = static_cast<size_t>(gr.n_splits) * gr.n_wg * kPfRows;
  return (slots * (head_size + 2) * sizeof(float) + 255) & ~static_cast<size_t>(255);
}

size_t pf_workspace_bytes(int n_prefill, int max_prefill_q_len, int num_q_heads, int num_kv_heads, int head_size) {
  if (n_prefill <= 0) return 0;
  return pf_partial_bytes(pf_grid(n_prefill, max_prefill_q_len, num_q_heads, num_kv_heads, 0), head_size) + 256;
}

template <int D, bool WIN, typename E>
int launch_prefill_e(const PrefillParams& P, bool kv8, dim3 grid, hipStream_t s) {
  if constexpr (D == 128) {
    if (kv8)
      hipLaunchKernelGGL((prefill_attn_kernel<128, true, WIN, E>), grid, dim3(256), 0, s, P);
    else
      hipLaunchKernelGGL((prefill_attn_kernel<128, false, WIN, E>), grid, dim3(256), 0, s, P);
  } else {
    hipLaunchKernelGGL((prefill_attn_kernel<D, false, WIN, E>), grid, dim3(256), 0, s, P);
  }
  int rc = launch_status("prefill_attn_kernel");
  if (rc != AIC_OK || P.n_splits == 1) return rc;
  const int64_t rows = static_cast<int64_t>(P.n_wg) * kPfRows;
  hipLaunchKernelGGL((prefill_combine_kernel<D, E>), dim3(static_cast<unsigned>((rows + 3) / 4)), dim3(256), 0, s, P);
  return launch_status("prefill_combine_kernel");
}

template <int D, bool WIN>
int launch_prefill(const PrefillParams& P, bool kv8, bool f16, dim3 grid, hipStream_t s) {
  return f16 ? launch_prefill_e<D, WIN, ElemF16>(P, kv8, grid, s) : launch_prefill_e<D, WIN, ElemBf16>(P, kv8, grid, s);
}

}  // namespace
}  // namespace aic

using namespace aic;

extern "C" {

size_t aic_step_attention_workspace_bytes(int num_decode_tokens, int n_prefill, int max_prefill_q_len, int num_q_heads,
                                          int num_kv_heads, int head_size, int num_splits_max) {
  if (num_q_heads <= 0 || num_kv_heads <= 0 || num_q_heads % num_kv_heads != 0) return 0;
  const int splits = num_splits_max > 0 ? num_splits_max : 64;
  size_t dec = 0;
  if (num_decode_tokens > 0)  // a mixed call stages the decode rows in one split's worth of the decode workspace
    dec = aic_verify_attention_workspace_bytes(num_decode_tokens, num_q_heads, head_size,
                                               n_prefill > 0 ? std::max(splits, 2) : splits);
  return dec + pf_workspace_bytes(n_prefill, max_prefill_q_len, num_q_heads, num_kv_heads, head_size);
}

int aic_step_attention(const void* q, int64_t q_stride, const void* k_cache, const void* v_cache, int64_t block_stride,
                       int kv_dtype, const float* k_scale, const float* v_scale, const int32_t* block_table,
                       int max_blocks_per_seq, const int32_t* seq_lens, const int32_t* query_start_loc, int batch,
                       int num_tokens, int num_q_heads, int num_kv_heads, int head_size, int block_size, float sm_scale,
                       void* out, int64_t out_stride, void* workspace, size_t workspace_bytes, int max_seq_len,
                       const int32_t* req_lists, int n_short, int n_prefill, int n_long,
                       const int32_t* decode_query_start_loc, const int32_t* decode_token_index, int num_decode_tokens,
                       int max_decode_q_len, int max_prefill_q_len, void* stream) {
  return aic_step_attention_win(q, q_stride, k_cache, v_cache, block_stride, kv_dtype, k_scale, v_scale, block_table,
                                max_blocks_per_seq, seq_lens, query_start_loc, batch, num_tokens, num_q_heads, num_kv_heads,
                                head_size, block_size, sm_scale, out, out_stride, workspace, workspace_bytes, max_seq_len,
                                req_lists, n_short, n_prefill, n_long, decode_query_start_loc, decode_token_index,
                                num_decode_tokens, max_decode_q_len, max_prefill_q_len, 0, nullptr, stream);
}

int aic_step_attention_win(const void* q, int64_t q_stride, const void* k_cache, const void* v_cache, int64_t block_stride,
                           int kv_dtype, const float* k_scale, const float* v_scale, const int32_t* block_table,
                           int max_blocks_per_seq, const int32_t* seq_lens, const int32_t* query_start_loc, int batch,
                           int num_tokens, int num_q_heads, int num_kv_heads, int head_size, int block_size,
                           float sm_scale, void* out, int64_t out_stride, void* workspace, size_t workspace_bytes,
                           int max_seq_len, const int32_t* req_lists, int n_short, int n_prefill, int n_long,
                           const int32_t* decode_query_start_loc, const int32_t* decode_token_index,
                           int num_decode_tokens, int max_decode_q_len, int max_prefill_q_len, int sliding_window,
                           const float* sinks, void* stream) {
  return aic_step_attention_dt(q, q_stride, k_cache, v_cache, block_stride, kv_dtype, k_scale, v_scale, block_table,
                               max_blocks_per_seq, seq_lens, query_start_loc, batch, num_tokens, num_q_heads, num_kv_heads,
                               head_size, block_size, sm_scale, out, out_stride, workspace, workspace_bytes, max_seq_len,
                               req_lists, n_short, n_prefill, n_long, decode_query_start_loc, decode_token_index,
                               num_decode_tokens, max_decode_q_len, max_prefill_q_len, sliding_window, sinks, AIC_DT_BF16,
                               stream);
}

// The whole-step call for a model of either 16-bit type: one attention call per step whatever the dtype, as the
// reference has it (arctic_inference/vllm/ulysses.py:510).  q_dtype is the type of q AND of out.
int aic_step_attention_dt(const void* q, int64_t q_stride, const void* k_cache, const void* v_cache, int64_t block_stride,
                          int kv_dtype, const float* k_scale, const float* v_scale, const int32_t* block_table,
                          int max_blocks_per_seq, const int32_t* seq_lens, const int32_t* query_start_loc, int batch,
                          int num_tokens, int num_q_heads, int num_kv_heads, int head_size, int block_size,
                          float sm_scale, void* out, int64_t out_stride, void* workspace, size_t workspace_bytes,
                          int max_seq_len, const int32_t* req_lists, int n_short, int n_prefill, int n_long,
                          const int32_t* decode_query_start_loc, const int32_t* decode_token_index,
                          int num_decode_tokens, int max_decode_q_len, int max_prefill_q_len, int sliding_window,
                          const float* sinks, int q_dtype, void* stream) {
  if (batch == 0 || num_tokens == 0) return AIC_OK;
  AIC_REQUIRE(sliding_window >= 0, "sliding_window must be >= 0 (0 = none)");
  AIC_REQUIRE(req_lists && n_short >= 0 && n_prefill >= 0 && n_long >= 0 && n_short + n_prefill + n_long == batch,
              "short / prefill / long request lists must partition the batch");
  const int32_t* short_reqs = req_lists;
  const int32_t* prefill_reqs = req_lists + n_short;
  const int32_t* long_reqs = req_lists + n_short + n_prefill;
  if (n_prefill == 0)  // a decode step: exactly aic_verify_attention_dt
    return aic_verify_attention_dt(q, q_stride, k_cache, v_cache, block_stride, kv_dtype, k_scale, v_scale, block_table,
                                   max_blocks_per_seq, seq_lens, query_start_loc, batch, num_tokens, max_decode_q_len,
                                   num_q_heads, num_kv_heads, head_size, block_size, sm_scale, out, out_stride, workspace,
                                   workspace_bytes, max_seq_len, short_reqs, n_short, long_reqs, n_long, sliding_window,
                                   sinks, q_dtype, stream);

  AIC_REQUIRE(q && k_cache && v_cache && block_table && seq_lens && query_start_loc && out && workspace,
              "null pointer argument to aic_step_attention");
  AIC_REQUIRE(num_q_heads > 0 && num_kv_heads > 0 && num_q_heads % num_kv_heads == 0,
              "num_q_heads must be a positive multiple of num_kv_heads");
  AIC_REQUIRE(num_q_heads / num_kv_heads <= 8, "prefill body: at most 8 query heads per kv head");
  AIC_REQUIRE(max_prefill_q_len > 0 && max_seq_len > 0 && max_blocks_per_seq > 0, "non-positive size argument");
  if (const int drc = attn_check_dtypes(q_dtype, kv_dtype); drc != AIC_OK) return drc;
  const bool kv8 = kv_dtype == AIC_DT_FP8_E4M3, f16 = q_dtype == AIC_DT_F16;
  if (head_size != 128 && !(head_size == 64 && !kv8)) {
    set_error("prefill body: head_size %d with a%s cache not supported (128, or 64 with a 16-bit cache)", head_size,
              kv8 ? "n fp8" : " 16-bit");
    return AIC_ERR_UNSUPPORTED;
  }
  AIC_REQUIRE(!kv8 || (k_scale && v_scale), "an fp8 kv cache needs k_scale and v_scale (device scalars)");
  AIC_REQUIRE(q_stride % 8 == 0 && out_stride % 8 == 0 && block_stride % 16 == 0, "strides must keep 16-byte alignment");
  if (block_size % 16 != 0) {
    set_error("block_size %d not supported (must be a multiple of 16)", block_size);
    return AIC_ERR_UNSUPPORTED;
  }
  const int n_dec_req = n_short + n_long;
  AIC_REQUIRE(n_dec_req == 0 || (decode_query_start_loc && decode_token_index && num_decode_tokens >= 0 && max_decode_q_len > 0),
              "a mixed step needs the compact decode query_start_loc and token index");
  AIC_NEED_DEVICE();

  const PfGrid gr = pf_grid(n_prefill, max_prefill_q_len, num_q_heads, num_kv_heads, max_seq_len, sliding_window);
  const size_t pf_bytes = pf_workspace_bytes(n_prefill, max_prefill_q_len, num_q_heads, num_kv_heads, head_size);
  AIC_REQUIRE(workspace_bytes >= pf_bytes, "workspace too small (%zu bytes, the prefill part needs %zu)", workspace_bytes,
              pf_bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);

  // ---- decode part: a compact sub-call on the decode rows (prefill requests have empty ranges in its query_start_loc
  // and ride in its short list), so that neither its workspace nor its combine launch sees a prefill token
  if (n_dec_req > 0 && num_decode_tokens > 0) {
    const size_t row_bytes = static_cast<size_t>(num_q_heads) * head_size * 2;
    const size_t stage = static_cast<size_t>(num_decode_tokens) * row_bytes;   // multiple of 256
    char* dec = ws + pf_bytes;
    AIC_REQUIRE(workspace_bytes >= pf_bytes + 2 * stage, "workspace too small (%zu bytes)", workspace_bytes);
    char* q_dec = dec;
    char* o_dec = dec + stage;
    hipLaunchKernelGGL(step_rows_kernel, dim3(num_decode_tokens), dim3(256), 0, s, static_cast<const char*>(q),
                       q_stride * 2, q_dec, static_cast<int64_t>(row_bytes), decode_token_index, static_cast<int>(row_bytes), 0);
    int rc = launch_status("step_rows_kernel");
    if (rc != AIC_OK) return rc;
    rc = aic_verify_attention_dt(q_dec, num_q_heads * head_size, k_cache, v_cache, block_stride, kv_dtype, k_scale,
                                 v_scale, block_table, max_blocks_per_seq, seq_lens, decode_query_start_loc, batch,
                                 num_decode_tokens, max_decode_q_len, num_q_heads, num_kv_heads, head_size, block_size,
                                 sm_scale, o_dec, num_q_heads * head_size, dec + 2 * stage,
                                 workspace_bytes - pf_bytes - 2 * stage, max_seq_len, short_reqs, n_short + n_prefill,
                                 long_reqs, n_long, sliding_window, sinks, q_dtype, stream);
    if (rc != AIC_OK) return rc;
    hipLaunchKernelGGL(step_rows_kernel, dim3(num_decode_tokens), dim3(256), 0, s, static_cast<const char*>(o_dec),
                       static_cast<int64_t>(row_bytes), static_cast<char*>(out), out_stride * 2, decode_token_index,
                       static_cast<int>(row_bytes), 1);
    rc = launch_status("step_rows_kernel");
    if (rc != AIC_OK) return rc;
  }

  // ---- prefill part
  PrefillParams P;
  P.q = static_cast<const uint16_t*>(q);
  P.k_cache = static_cast<const char*>(k_cache);
  P.v_cache = static_cast<const char*>(v_cache);
  P.block_table = block_table;
  P.seq_lens = seq_lens;
  P.query_start_loc = query_start_loc;
  P.reqs = prefill_reqs;
  P.k_scale = k_scale;
  P.v_scale = v_scale;
  P.out = static_cast<uint16_t*>(out);
  P.ws_o = reinterpret_cast<float*>(ws);
  P.ws_ml = P.ws_o + static_cast<size_t>(gr.n_splits) * gr.n_wg * kPfRows * head_size;
  P.q_stride = q_stride;
  P.out_stride = out_stride;
  P.block_stride = block_stride;
  P.max_blocks = max_blocks_per_seq;
  P.num_q_heads = num_q_heads;
  P.num_kv_heads = num_kv_heads;
  P.block_size = block_size;
  P.bs_shift = (block_size & (block_size - 1)) == 0 ? __builtin_ctz(static_cast<unsigned>(block_size)) : -1;
  P.n_req = n_prefill;
  P.n_qb = gr.n_qb;
  P.n_wg = gr.n_wg;
  P.n_splits = gr.n_splits;
  P.sm_scale = sm_scale;
  P.window = sliding_window;
  P.sinks = sinks;
  const dim3 grid(static_cast<unsigned>(gr.n_wg) * gr.n_splits);
  if (head_size == 128)
    return sliding_window > 0 ? launch_prefill<128, true>(P, kv8, f16, grid, s) : launch_prefill<128, false>(P, kv8, f16, grid, s);
  return sliding_window > 0 ? launch_prefill<64, true>(P, kv8, f16, grid, s) : launch_prefill<64, false>(P, kv8, f16, grid, s);
}

}  // extern "C"
