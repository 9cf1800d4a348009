// KV compaction after tree acceptance (aic_kv_compact_paths).
//
// The reference verifies one path per request (arctic_inference/vllm/model_runner.py:734-740), so its cache never holds
// more than the accepted chain plus rejected tail.  A tree step writes node t's K/V at key position base + t
// (base = seq_len - q_len); after acceptance the node at depth d of the accepted path, path[d], must sit at base + d —
// what decoding the accepted chain alone would have left.  This is that move, for K and V of every layer in one launch.
//
// CDNA4 mapping: pure byte movement of a few rows per request, latency- rather than bandwidth-bound.  A workgroup owns
// (request, layer, K | V) and walks the token row in 256-byte column chunks; a unit of work is one chunk: its rows are read
// into LDS (at most 64 rows x 256 B = 16 KiB), the workgroup synchronises, and only then are the destination slots
// written: source and destination sets overlap (path [0, 2, 3] moves slot 2 to slot 1 and slot 3 to slot 2), and with
// every read ahead of every write the result is the gather cache[base + d] = old cache[base + path[d]] whatever the order
// of the path.  Requests whose path is the identity (a chain accepted from the front, or no draft) leave after reading
// their path — most workgroups of a step, which is why the grid is (layer, K | V, request) and not spread over the chunks
// as well.  The layers' cache pointers ride in the kernel arguments, as in A16.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "aic_common.h"

namespace aic {

constexpr int kCompactLayersPerLaunch = 32;
constexpr int kCompactMaxPath = 64;
constexpr int kCompactChunk = 256;   // bytes of a token row a workgroup moves per trip: 16 lanes x 16 bytes

struct KvCompactTables {
  void* kc[kCompactLayersPerLaunch];
  void* vc[kCompactLayersPerLaunch];
};

__global__ void __launch_bounds__(256)
kv_compact_paths_kernel(KvCompactTables tab, const int32_t* __restrict__ block_table, int max_blocks,
                        const int32_t* __restrict__ seq_lens, const int32_t* __restrict__ qsl,
                        const int32_t* __restrict__ path, const int32_t* __restrict__ n_path_of, int max_q_len,
                        int block_size, int64_t block_stride_bytes, int row_bytes) {
  __shared__ uint4 rows_lds[kCompactMaxPath * (kCompactChunk / 16)];
  __shared__ int src_of[kCompactMaxPath];
  const int req = blockIdx.z;
  const int q_len = qsl[req + 1] - qsl[req];
  const int base = seq_lens[req] - q_len;
  const int n_path = min(min(n_path_of[req], max_q_len), min(q_len, kCompactMaxPath));
  if (n_path <= 0 || base < 0) return;
  const int32_t* prow = path + static_cast<int64_t>(req) * max_q_len;
  // depths whose node already sits in place (path[d] == d), is no node of the request, or lies in a page the table does
  // not have are left alone: src_of = -1
  bool any = false;
  if (threadIdx.x < kCompactMaxPath) {
    int src = -1;
    if (static_cast<int>(threadIdx.x) < n_path) {
      const int p = prow[threadIdx.x];
      const int d = threadIdx.x;
      if (p != d && p >= 0 && p < q_len && (base + p) / block_size < max_blocks && (base + d) / block_size < max_blocks)
        src = p;
    }
    src_of[threadIdx.x] = src;
    any = src >= 0;
  }
  if (!__syncthreads_or(any)) return;   // the identity path: nothing moves

  const int layer = blockIdx.y >> 1;
  char* cache = static_cast<char*>((blockIdx.y & 1) ? tab.vc[layer] : tab.kc[layer]);
  const int32_t* btab = block_table + static_cast<int64_t>(req) * max_blocks;
  const int r0 = threadIdx.x >> 4;                                        // 16 rows per pass
  auto slot_ptr = [&](int key, int col) -> char* {
    const int page = btab[key / block_size];
    return cache + page * block_stride_bytes + static_cast<int64_t>(key % block_size) * row_bytes + col;
  };
  for (int c0 = 0; c0 < row_bytes; c0 += kCompactChunk) {                 // (uniform: every thread makes every trip)
    const int col = c0 + (threadIdx.x & 15) * 16;                         // byte column of this lane in the token row
    if (col < row_bytes) {
      for (int d = r0; d < n_path; d += 16) {
        const int p = src_of[d];
        if (p >= 0) rows_lds[d * (kCompactChunk / 16) + (threadIdx.x & 15)] = *reinterpret_cast<const uint4*>(slot_ptr(base + p, col));
      }
    }
    __syncthreads();   // every source row of the unit is in LDS before any destination slot is written
    if (col < row_bytes) {
      for (int d = r0; d < n_path; d += 16) {
        if (src_of[d] >= 0) *reinterpret_cast<uint4*>(slot_ptr(base + d, col)) = rows_lds[d * (kCompactChunk / 16) + (threadIdx.x & 15)];
      }
    }
    __syncthreads();   // ... and the LDS rows are free again before the next chunk fills them
  }
}

}  // namespace aic

using namespace aic;

extern "C" int aic_kv_compact_paths(void* const* key_cache_ptrs, void* const* value_cache_ptrs, int num_layers,
                                    const int32_t* block_table, int max_blocks_per_seq, const int32_t* seq_lens,
                                    const int32_t* query_start_loc, const int32_t* path, const int32_t* num_accepted,
                                    int batch, int max_q_len, int num_kv_heads, int head_size, int elem_bytes,
                                    int block_size, int64_t block_stride, void* stream) {
  if (num_layers == 0 || batch == 0) return AIC_OK;
  AIC_REQUIRE(key_cache_ptrs && value_cache_ptrs && block_table && seq_lens && query_start_loc && path && num_accepted,
              "null pointer argument to aic_kv_compact_paths");
  AIC_REQUIRE(num_layers > 0 && batch > 0 && num_kv_heads > 0 && head_size > 0 && block_size > 0 && max_blocks_per_seq > 0,
              "non-positive size argument");
  AIC_REQUIRE(max_q_len >= 1 && max_q_len <= kCompactMaxPath, "max_q_len must be 1 .. %d", kCompactMaxPath);
  AIC_REQUIRE(elem_bytes == 1 || elem_bytes == 2 || elem_bytes == 4, "elem_bytes must be 1, 2 or 4");
  AIC_REQUIRE(batch <= 65535, "batch %d above the grid's 65535", batch);
  const int64_t row_bytes = static_cast<int64_t>(num_kv_heads) * head_size * elem_bytes;
  if (row_bytes % 16 != 0 || (block_stride * elem_bytes) % 16 != 0) {
    set_error("token rows of %lld bytes / block stride of %lld bytes: both must be multiples of 16",
              static_cast<long long>(row_bytes), static_cast<long long>(block_stride * elem_bytes));
    return AIC_ERR_UNSUPPORTED;
  }
  for (int l = 0; l < num_layers; ++l) {
    AIC_REQUIRE(key_cache_ptrs[l] && value_cache_ptrs[l], "null cache pointer for layer %d", l);
    AIC_REQUIRE(reinterpret_cast<uintptr_t>(key_cache_ptrs[l]) % 16 == 0 &&
                    reinterpret_cast<uintptr_t>(value_cache_ptrs[l]) % 16 == 0,
                "cache of layer %d is not 16-byte aligned", l);
  }
  AIC_NEED_DEVICE();
  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int l0 = 0; l0 < num_layers; l0 += kCompactLayersPerLaunch) {
    const int L = std::min(kCompactLayersPerLaunch, num_layers - l0);
    KvCompactTables tab;
    for (int l = 0; l < kCompactLayersPerLaunch; ++l) {
      tab.kc[l] = l < L ? key_cache_ptrs[l0 + l] : nullptr;
      tab.vc[l] = l < L ? value_cache_ptrs[l0 + l] : nullptr;
    }
    hipLaunchKernelGGL(kv_compact_paths_kernel, dim3(1, 2 * L, batch), dim3(256), 0, s, tab, block_table,
                       max_blocks_per_seq, seq_lens, query_start_loc, path, num_accepted, max_q_len, block_size,
                       block_stride * elem_bytes, static_cast<int>(row_bytes));
    const int rc = launch_status("kv_compact_paths_kernel");
    if (rc != AIC_OK) return rc;
  }
  return AIC_OK;
}
