// Shared-prefix phase of aic_verify_attention_prefix (prefix_attn.hip), as verify_attn.hip calls it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace aic {

struct PrefixArgs {
  const void* q;             // [num_tokens][num_q_heads][head_size], the call's 16-bit type
  const void* k_cache;
  const void* v_cache;
  const int32_t* table;      // device int32[>= prefix_len / block_size]: the pages of keys 0 .. prefix_len - 1
  const float* k_scale;      // fp8 cache: device scalars
  const float* v_scale;
  float* ws_o;               // the verify workspace: [slot][total_rows][head_size]
  float* ws_ml;              // [slot][total_rows][2]
  int64_t q_stride;
  int64_t block_stride;
  int num_tokens;
  int num_q_heads;
  int num_kv_heads;
  int head_size;
  int block_size;
  int prefix_len;            // a positive multiple of 32
  int n_splits;              // slots 0 .. n_splits - 1 of every row are written
  float sm_scale;
  bool kv8;
  bool f16;
};

// Split count of the prefix launch: enough workgroups for the chip, at least 128 keys per split, at most `max_slots`
// (>= 1).  aic_debug_attn_prefix_splits overrides the choice (still within the tile count and max_slots).
int prefix_pick_splits(int num_tokens, int num_q_heads, int num_kv_heads, int prefix_len, int max_slots, int n_cus);

// Launches the prefix body on `s`.  Arguments are those of a call aic_verify_attention_dt has accepted.
int launch_prefix_attention(const PrefixArgs& a, hipStream_t s);

// ---- groups of requests with a prefix each (aic_verify_attention_prefix_groups) ----
constexpr int kPrefixMaxGroups = 16;

struct PrefixGroupsArgs {
  PrefixArgs base;                    // table = the call's block table (every row); prefix_len unused; n_splits of the call
  int n_groups;                       // 1 .. kPrefixMaxGroups, every one with a prefix of at least one tile
  int prefix_len[kPrefixMaxGroups];   // positive multiples of 32
  int leader[kPrefixMaxGroups];       // request whose block-table row is the group's prefix table
  int token_start[kPrefixMaxGroups];  // first entry of the group in token_index
  int n_tokens[kPrefixMaxGroups];
  const int32_t* token_index;         // device: token rows of the call, sorted by group
  const int32_t* req_prefix_len;      // device int32[batch]: a request whose length rounds to 0 gets empty prefix slots
  const int32_t* query_start_loc;     // device int32[batch + 1]
  int batch;
  int max_blocks;                     // columns of the block table
};

// One split count for the call, from the groups' row blocks and the longest prefix; rules as prefix_pick_splits.
int prefix_groups_pick_splits(const PrefixGroupsArgs& a, int max_slots, int n_cus);

// Launches the grouped prefix body on `s`: slots 0 .. n_splits - 1 of EVERY row of the call are written.
int launch_prefix_groups_attention(const PrefixGroupsArgs& a, hipStream_t s);

}  // namespace aic
