// Shared-prefix phase of cascade attention (aic_verify_attention_prefix, verify_attn.hip): every query row of a step
// against keys 0 .. P - 1 that all requests of the step have in common, read ONCE for the step instead of once per
// request.
//
// Reference path: vLLM's FlashAttention backend serves such a step by cascade attention when its metadata says
// use_cascade (the one attention call of a step, the reference's arctic_inference/vllm/ulysses.py:510).  The three
// phases here: this body (keys [0, P), non-causal: every row's position is >= P by the entry's precondition), the verify
// bodies restricted to keys [P, ctx) of each request, and verify_attn_combine_kernel over the (m, l, O) partials of both.
//
// The body is the chunked-prefill one (prefill_attn.hip) and shares its tile step (pf_tile.h): one workgroup = 4 waves
// = 128 query rows of one kv head, K/V in 32-token tiles double buffered through LDS with one barrier per tile,
// S^T = K Q^T, lazy running maximum, P as a 16-bit head + tail, an fp8 cache converted exactly on the way in.  What
// differs:
//   * the rows of a kv head are ALL tokens of the call (row = token * G + head of the group; T * G rows, the last row
//     block padded and not stored), not those of one request;
//   * pages come from one table, there is no causal mask, no window and no partial tile (P is a multiple of 32);
//   * the result is always un-normalised f32 partials in slots of the verify workspace — never a finished row;
//   * the key range is split over n_splits workgroups per row block (chosen on the host) so that a step of a few
//     hundred rows still fills the chip.
// Workgroup index = row block * (Hkv * n_splits) + kv head * n_splits + split: the row blocks of one (kv head, split)
// are 8 k workgroups apart whenever Hkv * n_splits is a multiple of 8, land on the same XCD (workgroups are dealt
// round-robin over 8) and re-read their keys through that XCD's L2.
//
// aic_verify_attention_prefix_groups runs the same body (prefix_body) once per GROUP of requests with a prefix of its own,
// all groups in one launch (prefix_groups_attn_kernel, below): the rows, the table and the tile count of a workgroup are
// then its group's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "aic_common.h"
#include "attn_common.h"
#include "pf_tile.h"
#include "prefix_attn.h"

namespace aic {
namespace {

constexpr int kPxMinSplitTiles = 4;   // at least 128 keys per split
constexpr int kPxMaxSplits = 16;

struct PrefixParams {
  const uint16_t* q;
  const char* k_cache;
  const char* v_cache;
  const int32_t* table;
  const float* k_scale;
  const float* v_scale;
  float* ws_o;
  float* ws_ml;
  int64_t q_stride;
  int64_t block_stride;  // elements
  int num_q_heads;
  int num_kv_heads;
  int block_size;
  int bs_shift;    // log2(block_size) for powers of two, else -1
  int n_rows;      // num_tokens * G: rows of one kv head
  int total_rows;  // num_tokens * Hq: rows of a workspace slot
  int n_tiles;     // prefix_len / 32
  int n_splits;
  float sm_scale;
};

// The rows a workgroup serves.  One shared prefix (GR = false): row r of the call is token r / G, the table and the tile
// count are the call's.  Groups (GR = true, aic_verify_attention_prefix_groups): row r of the GROUP is token
// tok_index[r / G] (tok_index already advanced to the group's first entry), the table is the leader's block-table row,
// the tile count the group's.  All wave-uniform.
struct PrefixRows {
  const int32_t* table;
  const int32_t* tok_index;   // GR only
  int blk_row0;               // first row of the workgroup's row block (within the call / the group)
  int n_rows;                 // rows of the call / the group, for one kv head
  int n_tiles;
};

template <int D, bool KV8, typename E, bool GR>
__device__ __forceinline__ void prefix_body(const PrefixParams& P, const PrefixRows& R, const int h, const int split) {
  using T = PfTile<D, KV8, E>;
  constexpr int DT = T::DT, NS = T::NS, ES = T::ES;
  __shared__ uint4 lds[2][2][T::kTileU4];   // [buffer][K, V] tile images (tile_off<D>)

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c16 = lane & 15;
  const int Hkv = P.num_kv_heads, Hq = P.num_q_heads, G = Hq / Hkv;
  const int tps = (R.n_tiles + P.n_splits - 1) / P.n_splits;
  const int t_first = split * tps, t_last = min(R.n_tiles, t_first + tps);   // may be empty: the slot then says so

  const int w_row0 = R.blk_row0 + wave * (kPfMT * 16);
  const bool wave_live = w_row0 < R.n_rows;
  auto token_of = [&](int row_token) -> int { return GR ? R.tok_index[row_token] : row_token; };

  // ---- query fragments and the row state (max, sum) = (-inf, 0): sinks belong to the first suffix partial
  uint4 qf[kPfMT][NS];
  float m_run[kPfMT], l_run[kPfMT];
  f32x4 o_acc[kPfMT][DT];
#pragma unroll
  for (int mt = 0; mt < kPfMT; ++mt) {
    const int rc = min(w_row0 + mt * 16 + c16, R.n_rows - 1);   // rows past the end: a copy of the last one, not stored
    const int rt = rc / G, gq = rc - rt * G;
    const int tok = token_of(rt);
    const uint16_t* qrow = P.q + static_cast<int64_t>(tok) * P.q_stride + static_cast<int64_t>(h * G + gq) * D;
#pragma unroll
    for (int s = 0; s < NS; ++s) qf[mt][s] = *reinterpret_cast<const uint4*>(qrow + 32 * s + 8 * g);
    m_run[mt] = -INFINITY;
    l_run[mt] = 0.0f;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o_acc[mt][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const float scale_log2 = P.sm_scale * kLog2e * (KV8 ? *P.k_scale : 1.0f);
  const float inv_scale = 1.0f / scale_log2;
  const float out_scale = KV8 ? *P.v_scale : 1.0f;

  // ---- tile staging, the prefill body's thread mapping (PfTile::Regs).  Every token of every tile is below P, so no
  // index is clamped; a 16-token group never straddles two pages (block_size is a multiple of 16).
  const int64_t kv_row = static_cast<int64_t>(Hkv) * D;  // elements between consecutive tokens of a page
  const unsigned row_bytes = static_cast<unsigned>(kv_row) * ES;
  const_i32_ptr btab = (const_i32_ptr)R.table;
  typename T::Regs r;
  auto group_base = [&](int first) -> int64_t {   // element offset of token `first` of kv head h
    const unsigned f = static_cast<unsigned>(first), bs = static_cast<unsigned>(P.block_size);
    const unsigned pg = P.bs_shift >= 0 ? f >> P.bs_shift : f / bs;
    const unsigned po = f - pg * bs;
    return static_cast<int64_t>(btab[pg]) * P.block_stride + static_cast<int64_t>(po) * kv_row + h * D;
  };
  auto load_tile = [&](int tt) {
    const int64_t b0 = group_base(tt), b1 = group_base(tt + 16);
    if (T::ONE_CHUNK) {
      const int ti = tid >> 3, ch = tid & 7;
      const int64_t base = ti < 16 ? b0 : b1;
      const size_t byte = static_cast<size_t>(base) * ES + __umul24(static_cast<unsigned>(ti & 15), row_bytes) + 16u * ch;
      r.k0 = ld_kv16(P.k_cache + byte);
      r.v0 = ld_kv16(P.v_cache + byte);
    } else {
      const int ti = tid >> 4, ch = tid & 15;
      const unsigned off = __umul24(static_cast<unsigned>(ti), row_bytes) + 16u * ch;
      const size_t y0 = static_cast<size_t>(b0) * 2 + off, y1 = static_cast<size_t>(b1) * 2 + off;
      r.k0 = ld_kv16(P.k_cache + y0);
      r.k1 = ld_kv16(P.k_cache + y1);
      r.v0 = ld_kv16(P.v_cache + y0);
      r.v1 = ld_kv16(P.v_cache + y1);
    }
  };
  auto store_tile = [&](int buf) {
    T::store(reinterpret_cast<char*>(lds[buf][0]), reinterpret_cast<char*>(lds[buf][1]), tid, r);
  };
  auto no_mask = [](int, float (&)[8]) {};

  if (t_first < t_last) {
    load_tile(t_first * kTile);
    store_tile(0);
    __syncthreads();
    for (int t = t_first; t < t_last; ++t) {
      const int buf = (t - t_first) & 1;
      const bool more = t + 1 < t_last;
      if (more) load_tile((t + 1) * kTile);   // in flight during the tile's MFMAs
      if (wave_live)
        T::compute(reinterpret_cast<const char*>(lds[buf][0]), reinterpret_cast<const char*>(lds[buf][1]), g, c16, qf, m_run,
                   l_run, o_acc, scale_log2, inv_scale, no_mask);
      if (more) store_tile(buf ^ 1);          // last read in the previous iteration, before its barrier
      __syncthreads();
    }
  }
  if (!wave_live) return;

  // ---- the slot of this split: un-normalised O (v_scale folded in), max in natural-log units, sum
#pragma unroll
  for (int mt = 0; mt < kPfMT; ++mt) {
    const float l = rowgroup_sum(l_run[mt]);
    const int rr = w_row0 + mt * 16 + c16;
    if (rr >= R.n_rows) continue;
    const int rt = rr / G, gq = rr - rt * G;
    const int tok = token_of(rt);
    const int64_t grow = static_cast<int64_t>(tok) * Hq + h * G + gq;
    const int64_t slot = static_cast<int64_t>(split) * P.total_rows + grow;
    float* op = P.ws_o + slot * D + 4 * g;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
      *reinterpret_cast<float4*>(op + dt * 16) = make_float4(o_acc[mt][dt][0] * out_scale, o_acc[mt][dt][1] * out_scale,
                                                             o_acc[mt][dt][2] * out_scale, o_acc[mt][dt][3] * out_scale);
    if (g == 0) *reinterpret_cast<float2*>(P.ws_ml + slot * 2) = make_float2(m_run[mt] * kLn2, l);
  }
}

template <int D, bool KV8, typename E>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) prefix_attn_kernel(PrefixParams P) {
  const int split = blockIdx.x % P.n_splits;
  const int rest = blockIdx.x / P.n_splits;
  PrefixRows R;
  R.table = P.table;
  R.tok_index = nullptr;
  R.blk_row0 = (rest / P.num_kv_heads) * kPfRows;
  R.n_rows = P.n_rows;
  R.n_tiles = P.n_tiles;
  prefix_body<D, KV8, E, false>(P, R, rest % P.num_kv_heads, split);
}

// ---- groups (aic_verify_attention_prefix_groups) ----------------------------------------------------------------------
// One launch for every group of the call.  Workgroup index = row block * (Hkv * n_splits) + kv head * n_splits + split as
// above, the row blocks counted through the groups in order (group g owns row blocks rb_end[g - 1] .. rb_end[g] - 1), so the
// row blocks of one (kv head, split) keep their XCD.  The <= 16 descriptors travel by value and are scanned with constant
// indices: scalar loads from the kernel arguments and scalar selects, no table in memory.
// Behind the group workgroups come the FILL workgroups, one wave per request: a request whose prefix length rounds to 0
// (no group, or a group below one tile) has no row in any group, and its rows' prefix slots are given the empty partial
// (max, sum) = (-inf, 0) here, so that the merge never reads what an earlier call left in the workspace.  (The values of
// an empty slot are never read: verify_attn_combine_kernel redirects the load of a weight-0 slot.)
struct PrefixGroupDesc {
  int rb_end;      // row blocks of groups 0 .. g
  int tok_start;   // first entry of the group in tok_index
  int n_rows;      // tokens of the group * G
  int n_tiles;     // P_g / 32 > 0
  int leader;      // request whose block-table row holds the group's pages
};

struct PrefixGroupsParams {
  PrefixParams P;   // table = the call's block table; n_rows and n_tiles unused
  PrefixGroupDesc grp[kPrefixMaxGroups];
  const int32_t* tok_index;
  const int32_t* req_prefix_len;
  const int32_t* query_start_loc;
  int n_group_wgs;
  int max_blocks;
  int batch;
};

template <int D, bool KV8, typename E>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
prefix_groups_attn_kernel(PrefixGroupsParams A) {
  const int b = blockIdx.x;
  if (b >= A.n_group_wgs) {
    const int req = (b - A.n_group_wgs) * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (req >= A.batch || (A.req_prefix_len[req] & ~(kTile - 1)) > 0) return;
    const int q0 = A.query_start_loc[req], q1 = A.query_start_loc[req + 1];
    const int first = q0 * A.P.num_q_heads, n = (q1 - q0) * A.P.num_q_heads;   // the request's rows of a slot
    for (int i = threadIdx.x & 63; i < n * A.P.n_splits; i += 64) {
      const int slot = i / n, r = i - slot * n;
      *reinterpret_cast<float2*>(A.P.ws_ml + (static_cast<int64_t>(slot) * A.P.total_rows + first + r) * 2) =
          make_float2(-INFINITY, 0.0f);
    }
    return;
  }
  const int split = b % A.P.n_splits;
  const int rest = b / A.P.n_splits;
  const int rb = rest / A.P.num_kv_heads;
  int rb_first = 0, tok_start = 0, n_rows = 0, n_tiles = 0, leader = 0;
  bool found = false;
#pragma unroll
  for (int i = 0; i < kPrefixMaxGroups; ++i) {
    const bool hit = !found && rb < A.grp[i].rb_end;   // (descriptors behind the last group repeat its rb_end: never hit)
    if (hit) {
      tok_start = A.grp[i].tok_start;
      n_rows = A.grp[i].n_rows;
      n_tiles = A.grp[i].n_tiles;
      leader = A.grp[i].leader;
    }
    found = found || hit;
    if (!found) rb_first = A.grp[i].rb_end;
  }
  if (!found) return;
  PrefixRows R;
  R.table = A.P.table + static_cast<int64_t>(leader) * A.max_blocks;
  R.tok_index = A.tok_index + tok_start;
  R.blk_row0 = (rb - rb_first) * kPfRows;
  R.n_rows = n_rows;
  R.n_tiles = n_tiles;
  prefix_body<D, KV8, E, true>(A.P, R, rest % A.P.num_kv_heads, split);
}

int g_prefix_splits = 0;   // aic_debug_attn_prefix_splits: 0 = choose

template <typename E>
int launch_prefix_e(const PrefixParams& P, int head_size, bool kv8, dim3 grid, hipStream_t s) {
  if (head_size == 64)
    hipLaunchKernelGGL((prefix_attn_kernel<64, false, E>), grid, dim3(256), 0, s, P);
  else if (kv8)
    hipLaunchKernelGGL((prefix_attn_kernel<128, true, E>), grid, dim3(256), 0, s, P);
  else
    hipLaunchKernelGGL((prefix_attn_kernel<128, false, E>), grid, dim3(256), 0, s, P);
  return launch_status("prefix_attn_kernel");
}

template <typename E>
int launch_prefix_groups_e(const PrefixGroupsParams& A, int head_size, bool kv8, dim3 grid, hipStream_t s) {
  if (head_size == 64)
    hipLaunchKernelGGL((prefix_groups_attn_kernel<64, false, E>), grid, dim3(256), 0, s, A);
  else if (kv8)
    hipLaunchKernelGGL((prefix_groups_attn_kernel<128, true, E>), grid, dim3(256), 0, s, A);
  else
    hipLaunchKernelGGL((prefix_groups_attn_kernel<128, false, E>), grid, dim3(256), 0, s, A);
  return launch_status("prefix_groups_attn_kernel");
}

int64_t row_blocks(int64_t tokens, int G) { return (tokens * G + kPfRows - 1) / kPfRows; }

// split count for `n_rb` row blocks of `tiles` key tiles at most
int pick_splits_for(int64_t n_rb, int num_kv_heads, int tiles, int max_slots, int n_cus) {
  const int cap = std::max(1, std::min(tiles, max_slots));
  if (g_prefix_splits > 0) return std::min(g_prefix_splits, cap);
  const int64_t n_wg = std::max<int64_t>(1, n_rb * num_kv_heads);
  int s = static_cast<int>(std::min<int64_t>(kPxMaxSplits, (n_cus + n_wg - 1) / n_wg));
  s = std::min(s, std::max(1, tiles / kPxMinSplitTiles));
  return std::max(1, std::min(s, cap));
}

void fill_params(PrefixParams& P, const PrefixArgs& a) {
  P.q = static_cast<const uint16_t*>(a.q);
  P.k_cache = static_cast<const char*>(a.k_cache);
  P.v_cache = static_cast<const char*>(a.v_cache);
  P.table = a.table;
  P.k_scale = a.k_scale;
  P.v_scale = a.v_scale;
  P.ws_o = a.ws_o;
  P.ws_ml = a.ws_ml;
  P.q_stride = a.q_stride;
  P.block_stride = a.block_stride;
  P.num_q_heads = a.num_q_heads;
  P.num_kv_heads = a.num_kv_heads;
  P.block_size = a.block_size;
  P.bs_shift = (a.block_size & (a.block_size - 1)) == 0 ? __builtin_ctz(static_cast<unsigned>(a.block_size)) : -1;
  const int G = a.num_q_heads / a.num_kv_heads;
  P.n_rows = static_cast<int>(static_cast<int64_t>(a.num_tokens) * G);
  P.total_rows = a.num_tokens * a.num_q_heads;
  P.n_tiles = a.prefix_len / kTile;
  P.n_splits = a.n_splits;
  P.sm_scale = a.sm_scale;
}

}  // namespace

int prefix_groups_pick_splits(const PrefixGroupsArgs& a, int max_slots, int n_cus) {
  const int G = a.base.num_q_heads / a.base.num_kv_heads;
  int64_t n_rb = 0;
  int tiles = 1;
  for (int g = 0; g < a.n_groups; ++g) {
    n_rb += row_blocks(a.n_tokens[g], G);
    tiles = std::max(tiles, a.prefix_len[g] / kTile);
  }
  return pick_splits_for(n_rb, a.base.num_kv_heads, tiles, max_slots, n_cus);
}

int launch_prefix_groups_attention(const PrefixGroupsArgs& a, hipStream_t s) {
  PrefixGroupsParams A;
  fill_params(A.P, a.base);
  const int G = a.base.num_q_heads / a.base.num_kv_heads;
  int64_t rb = 0;
  for (int g = 0; g < kPrefixMaxGroups; ++g) {
    PrefixGroupDesc& d = A.grp[g];
    if (g < a.n_groups) {
      rb += row_blocks(a.n_tokens[g], G);
      d.tok_start = a.token_start[g];
      d.n_rows = a.n_tokens[g] * G;
      d.n_tiles = a.prefix_len[g] / kTile;
      d.leader = a.leader[g];
    } else {
      d.tok_start = d.n_rows = d.n_tiles = d.leader = 0;
    }
    d.rb_end = static_cast<int>(rb);
  }
  A.tok_index = a.token_index;
  A.req_prefix_len = a.req_prefix_len;
  A.query_start_loc = a.query_start_loc;
  A.max_blocks = a.max_blocks;
  A.batch = a.batch;
  const int64_t n_group_wgs = rb * a.base.num_kv_heads * a.base.n_splits;
  A.n_group_wgs = static_cast<int>(n_group_wgs);
  const dim3 grid(static_cast<unsigned>(n_group_wgs + (a.batch + 3) / 4));
  return a.base.f16 ? launch_prefix_groups_e<ElemF16>(A, a.base.head_size, a.base.kv8, grid, s)
                    : launch_prefix_groups_e<ElemBf16>(A, a.base.head_size, a.base.kv8, grid, s);
}

int prefix_pick_splits(int num_tokens, int num_q_heads, int num_kv_heads, int prefix_len, int max_slots, int n_cus) {
  const int tiles = prefix_len / kTile;
  const int cap = std::max(1, std::min(tiles, max_slots));
  if (g_prefix_splits > 0) return std::min(g_prefix_splits, cap);
  const int64_t n_rows = static_cast<int64_t>(num_tokens) * (num_q_heads / num_kv_heads);
  const int64_t n_wg = (n_rows + kPfRows - 1) / kPfRows * num_kv_heads;
  int s = static_cast<int>(std::min<int64_t>(kPxMaxSplits, (n_cus + n_wg - 1) / n_wg));
  s = std::min(s, std::max(1, tiles / kPxMinSplitTiles));
  return std::max(1, std::min(s, cap));
}

int launch_prefix_attention(const PrefixArgs& a, hipStream_t s) {
  PrefixParams P;
  fill_params(P, a);
  const int64_t n_rb = row_blocks(a.num_tokens, a.num_q_heads / a.num_kv_heads);
  const dim3 grid(static_cast<unsigned>(n_rb * a.num_kv_heads * a.n_splits));
  return a.f16 ? launch_prefix_e<ElemF16>(P, a.head_size, a.kv8, grid, s)
               : launch_prefix_e<ElemBf16>(P, a.head_size, a.kv8, grid, s);
}

}  // namespace aic

extern "C" {

// debug: split count of the shared-prefix launch (0 = choose); every setting computes the same result
int aic_debug_attn_prefix_splits(int n) {
  aic::g_prefix_splits = n > 0 ? n : 0;
  return AIC_OK;
}

}  // extern "C"
