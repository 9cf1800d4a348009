// A6 — rejection acceptance of draft tokens against the target model's verify logits.
//
// The reference delegates this to vllm.v1.sample.rejection_sampler.RejectionSampler
// (call site /root/reference/arctic_inference/vllm/model_runner.py:405-411, output parsed at
// :456-459; draft_probs is always None there, :407).  Semantics restated in oracle/spec_oracle.py.
//
// CDNA4 mapping.  The cost is reading the [num_draft, vocab] logits once (770 KB per request at
// k=3, bf16): an HBM-bound row reduction.  num_draft is small (<= ~200 rows at B=64), far fewer
// than the 256 CUs need, so every row is split into S vocab segments -> grid (rows, S) of
// 256-thread workgroups streaming 16 bytes per lane, each writing a partial (max, argmax); the
// accept step is one wavefront per request: lane p owns draft position p, folds that row's S
// partials, and the first rejected position comes from a 64-bit ballot + ffs (the "accept scan"),
// so the whole scan is two cross-lane operations instead of a serial loop.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "aic_common.h"

namespace aic {

constexpr int kMaxSplits = 64;
constexpr int kSegQuantum = 2048;  // 256 threads x 8 elements

template <typename T>
struct Elem;
template <>
struct Elem<float> {
  static constexpr int kVec = 4;
  static __device__ __forceinline__ float get(const float* p, int e) { return p[e]; }
  static __device__ __forceinline__ float round(float x) { return x; }
};
struct bf16_t { uint16_t b; };
struct f16_t { uint16_t b; };
template <>
struct Elem<bf16_t> {
  static constexpr int kVec = 8;
  static __device__ __forceinline__ float get(const bf16_t* p, int e) { return bf16_to_f32(p[e].b); }
  static __device__ __forceinline__ float round(float x) { return round_bf16(x); }
};
template <>
struct Elem<f16_t> {
  static constexpr int kVec = 8;
  static __device__ __forceinline__ float get(const f16_t* p, int e) { return f16_to_f32(p[e].b); }
  static __device__ __forceinline__ float round(float x) { return round_f16(x); }
};

// x = l / T (IEEE division).  The rejection sampler's compute_probs divides in place in the logits dtype, so its x is
// rounded to that dtype; the token sampler (SAMPLER) converts to f32 first and keeps x in f32.
template <typename T, bool SAMPLER>
__device__ __forceinline__ float scaled_logit(float l, float temp) {
  const float x = __fdiv_rn(l, temp);
  return SAMPLER ? x : Elem<T>::round(x);
}

struct Best {
  float v;
  int i;
};
__device__ __forceinline__ Best better(Best a, Best b) {
  // larger value wins; equal values -> lower index (torch.argmax on a row returns the first maximum)
  if (b.v > a.v || (b.v == a.v && b.i < a.i)) return b;
  return a;
}
__device__ __forceinline__ Best wave_best(Best x) {
  for (int off = 32; off > 0; off >>= 1) {
    Best o;
    o.v = __shfl_xor(x.v, off);
    o.i = __shfl_xor(x.i, off);
    x = better(x, o);
  }
  return x;
}
__device__ __forceinline__ float wave_max(float x) {
  for (int off = 32; off > 0; off >>= 1) x = fmaxf(x, __shfl_xor(x, off));
  return x;
}
__device__ __forceinline__ float wave_sum(float x) {
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
  return x;
}

__device__ __forceinline__ int request_of_row(const int32_t* cu, int batch, int row) {
  int lo = 0, hi = batch - 1;  // first request whose inclusive prefix sum exceeds row
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cu[mid] > row) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// MODE 0: arg-max of the raw logits (greedy rows).
// MODE 1: softmax statistics of x = round(l / T): partial (max, sum exp(x - max)).
// MODE 2: recovered-token arg-max of p_v / q_v with p[draft] := 0, and p[draft] itself;
//         greedy rows (T <= 0) fall back to the MODE 0 arg-max.
// SAMPLER (aic_sample_topk_topp, MODE 1 only): one row per request (no cu / draft ids), x kept in f32.
template <typename T, int MODE, bool VEC_OK, bool SAMPLER = false>
__global__ void __launch_bounds__(256)
logits_row_kernel(const T* __restrict__ logits, int64_t row_stride, int vocab, int seg_len, int n_splits,
                  const int32_t* __restrict__ draft_ids, const int32_t* __restrict__ cu, int batch,
                  const float* __restrict__ temperature, const float* __restrict__ exp_noise,
                  float* __restrict__ part_val, int32_t* __restrict__ part_idx, float* __restrict__ stat_max,
                  float* __restrict__ stat_sum, float* __restrict__ p_draft, const int64_t* __restrict__ row_index,
                  const int64_t* __restrict__ bonus_row_index, int n_draft_rows) {
  constexpr int V = Elem<T>::kVec;
  const int row = blockIdx.x;
  const int seg = blockIdx.y;
  const int begin = seg * seg_len;
  const int end = min(begin + seg_len, vocab);
  // row r of the call lives at logits[row_index[r]] when the caller passes the un-gathered [T, V] logits; rows past
  // the draft rows are the requests' bonus rows (greedy sampler folded into this launch)
  const T* base = logits + (row >= n_draft_rows ? bonus_row_index[row - n_draft_rows]
                                                : (row_index ? row_index[row] : static_cast<int64_t>(row))) * row_stride;
  __shared__ float s_v[4];
  __shared__ int s_i[4];
  __shared__ float s_m, s_z;

  float inv_t_is_greedy = 0.0f;
  float temp = 1.0f;
  int req = 0, draft = -1;
  const float* q = nullptr;
  bool greedy_row = (MODE == 0);
  if (MODE != 0) {
    req = SAMPLER ? row : request_of_row(cu, batch, row);
    temp = temperature[req];
    greedy_row = !(temp > 0.0f);
    if constexpr (SAMPLER) {
      if (!exp_noise) greedy_row = true;  // the sampler without noise: every row is greedy
    }
    draft = SAMPLER ? -1 : draft_ids[row];
    q = exp_noise ? exp_noise + static_cast<int64_t>(req) * vocab : nullptr;
  }
  (void)inv_t_is_greedy;
  if (MODE == 1 && !SAMPLER && seg == 0 && threadIdx.x == 0) p_draft[row] = 0.0f;  // a draft id outside the vocab has p = 0

  float row_max = 0.0f, row_z = 1.0f;
  if (MODE == 2 && !greedy_row) {
    // fold the softmax partials of this row (every block redoes this tiny reduction)
    if (threadIdx.x < 64) {
      float m = -INFINITY;
      for (int s = threadIdx.x; s < n_splits; s += 64) m = fmaxf(m, stat_max[row * n_splits + s]);
      m = wave_max(m);
      float z = 0.0f;
      for (int s = threadIdx.x; s < n_splits; s += 64) {
        const float pm = stat_max[row * n_splits + s];
        if (pm > -INFINITY) z += stat_sum[row * n_splits + s] * __expf(pm - m);
      }
      z = wave_sum(z);
      if (threadIdx.x == 0) {
        s_m = m;
        s_z = z;
      }
    }
    __syncthreads();
    row_max = s_m;
    row_z = s_z;
  }

  Best best;
  best.v = -INFINITY;
  best.i = begin;
  float run_m = -INFINITY, run_z = 0.0f;

  auto visit = [&](int idx, float l) {
    if (MODE == 0 || (MODE == 2 && greedy_row)) {
      if (l > best.v) {
        best.v = l;
        best.i = idx;
      }
    } else {
      const float x = scaled_logit<T, SAMPLER>(l, temp);  // logits.div_(temperature) in the logits dtype (sampler: in f32)
      if (MODE == 1) {
        if (x > run_m) {
          run_z = run_z * __expf(run_m - x) + 1.0f;
          run_m = x;
        } else if (x > -INFINITY) {
          run_z += __expf(x - run_m);
        }
      } else {
        float p = __fdiv_rn(__expf(x - row_max), row_z);
        if (idx == draft) {
          p_draft[row] = p;
          p = 0.0f;
        }
        const float r = __fdiv_rn(p, q[idx]);
        if (r > best.v) {
          best.v = r;
          best.i = idx;
        }
      }
    }
  };

  if (VEC_OK) {
    for (int i = begin + threadIdx.x * V; i < end; i += 256 * V) {
      if (i + V <= end) {
        T buf[V];
        *reinterpret_cast<uint4*>(buf) = *reinterpret_cast<const uint4*>(base + i);
#pragma unroll
        for (int e = 0; e < V; ++e) visit(i + e, Elem<T>::get(buf, e));
      } else {
        for (int e = 0; i + e < end; ++e) visit(i + e, Elem<T>::get(base + i, e));
      }
    }
  } else {
    for (int i = begin + threadIdx.x; i < end; i += 256) visit(i, Elem<T>::get(base + i, 0));
  }

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (MODE == 1 && !greedy_row) {
    // combine (max, sum) pairs across the block
    float m = wave_max(run_m);
    float z = run_m > -INFINITY ? run_z * __expf(run_m - m) : 0.0f;
    z = wave_sum(z);
    if (lane == 0) {
      s_v[wave] = m;
      reinterpret_cast<float*>(s_i)[wave] = z;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      float M = fmaxf(fmaxf(s_v[0], s_v[1]), fmaxf(s_v[2], s_v[3]));
      float Z = 0.0f;
      for (int w = 0; w < 4; ++w)
        if (s_v[w] > -INFINITY) Z += reinterpret_cast<float*>(s_i)[w] * __expf(s_v[w] - M);
      stat_max[row * n_splits + seg] = M;
      stat_sum[row * n_splits + seg] = Z;
    }
    return;
  }
  if (MODE == 1) return;  // greedy row: nothing to prepare

  best = wave_best(best);
  if (lane == 0) {
    s_v[wave] = best.v;
    s_i[wave] = best.i;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    Best b;
    b.v = s_v[0];
    b.i = s_i[0];
    for (int w = 1; w < 4; ++w) {
      Best o;
      o.v = s_v[w];
      o.i = s_i[w];
      b = better(b, o);
    }
    part_val[row * n_splits + seg] = b.v;
    part_idx[row * n_splits + seg] = b.i;
  }
}

// One wavefront per request; lane p owns draft position p.
template <bool RANDOM>
__global__ void __launch_bounds__(64)
accept_kernel(const float* __restrict__ part_val, const int32_t* __restrict__ part_idx, int n_splits,
              const int32_t* __restrict__ draft_ids, const int32_t* __restrict__ cu,
              const int32_t* __restrict__ bonus, const float* __restrict__ temperature,
              const double* __restrict__ uniform, const float* __restrict__ p_draft, int max_spec_len,
              int32_t* __restrict__ out, int32_t* __restrict__ num_accepted, int32_t* __restrict__ last_token,
              int32_t* __restrict__ hidden_index, int bonus_part_row0) {
  const int req = blockIdx.x;
  const int lane = threadIdx.x;
  const int start = req == 0 ? 0 : cu[req - 1];
  const int n = cu[req] - start;
  const int width = max_spec_len + 1;
  int32_t* orow = out + static_cast<int64_t>(req) * width;

  // bonus token: the sampler's id, or (bonus_part_row0 >= 0) the arg-max partials of this request's bonus row
  int bonus_tok;
  if (bonus_part_row0 >= 0) {
    const int brow = bonus_part_row0 + req;
    Best b;
    b.v = part_val[brow * n_splits];
    b.i = part_idx[brow * n_splits];
    for (int s = 1; s < n_splits; ++s) {
      Best o;
      o.v = part_val[brow * n_splits + s];
      o.i = part_idx[brow * n_splits + s];
      b = better(b, o);
    }
    bonus_tok = b.i;
  } else {
    bonus_tok = bonus[req];
  }
  bool reject = false;
  int token = -1;
  if (lane < n) {
    const int row = start + lane;
    Best b;
    b.v = part_val[row * n_splits];
    b.i = part_idx[row * n_splits];
    for (int s = 1; s < n_splits; ++s) {
      Best o;
      o.v = part_val[row * n_splits + s];
      o.i = part_idx[row * n_splits + s];
      b = better(b, o);
    }
    const int draft = draft_ids[row];
    bool greedy = true;
    if (RANDOM) greedy = !(temperature[req] > 0.0f);
    if (greedy) {
      token = b.i;  // the target's own arg-max is emitted whether or not it equals the draft
      reject = (draft != b.i);
    } else {
      const bool accept = static_cast<double>(p_draft[row]) >= uniform[row];
      token = accept ? draft : b.i;  // b.i = recovered token
      reject = !accept;
    }
  }
  const unsigned long long rej = __ballot(reject);
  const int first_rej = rej ? (__ffsll(static_cast<long long>(rej)) - 1) : n;  // accept scan
  const int written = first_rej < n ? first_rej + 1 : n + 1;
  if (lane < width) {
    int32_t v = -1;
    if (lane < n && lane <= first_rej) v = token;
    if (lane == n && first_rej == n) v = bonus_tok;
    orow[lane] = v;
  }
  // what the proposer needs next (arctic_proposer.py:133-147)
  const int last_lane = written - 1;
  int last = __shfl(token, min(last_lane, 63));
  if (last_lane == n) last = bonus_tok;
  if (lane == 0) {
    if (num_accepted) num_accepted[req] = written;
    if (last_token) last_token[req] = last;
    if (hidden_index) hidden_index[req] = (written - 1) + start + req;
  }
}

static int pick_splits(int rows, int vocab) {
  int s = (1024 + rows - 1) / rows;
  const int max_by_len = (vocab + kSegQuantum - 1) / kSegQuantum;
  if (s > max_by_len) s = max_by_len;
  if (s > kMaxSplits) s = kMaxSplits;
  if (s < 1) s = 1;
  return s;
}

template <typename T>
static int run_rejection(const void* logits, int64_t row_stride, int vocab, const int32_t* draft,
                         const int32_t* cu, const int32_t* bonus, const float* temperature, const double* uniform,
                         const float* noise, int batch, int rows, int max_spec_len, int32_t* out, int32_t* nacc,
                         int32_t* last, int32_t* hidx, const int64_t* row_index, const int64_t* bonus_rows, void* workspace,
                         hipStream_t stream, bool random) {
  const int grid_rows = rows + (bonus_rows ? batch : 0);   // bonus rows are reduced in the same launch
  const int S = grid_rows > 0 ? pick_splits(grid_rows, vocab) : 1;  // a step without drafts still emits bonus tokens
  int seg_len = (vocab + S - 1) / S;
  seg_len = (seg_len + kSegQuantum - 1) / kSegQuantum * kSegQuantum;
  const int n_splits = (vocab + seg_len - 1) / seg_len;
  float* part_val = static_cast<float*>(workspace);
  const size_t wr = static_cast<size_t>(grid_rows);
  int32_t* part_idx = reinterpret_cast<int32_t*>(part_val + wr * kMaxSplits);
  float* stat_max = reinterpret_cast<float*>(part_idx + wr * kMaxSplits);
  float* stat_sum = stat_max + wr * kMaxSplits;
  float* p_draft = stat_sum + wr * kMaxSplits;
  const T* lg = static_cast<const T*>(logits);
  const bool vec_ok = (reinterpret_cast<uintptr_t>(logits) % 16 == 0) && ((row_stride * sizeof(T)) % 16 == 0);
  if (grid_rows > 0) {
    dim3 grid(grid_rows, n_splits);
#define AIC_ROW_LAUNCH(MODE)                                                                                      \
  if (vec_ok)                                                                                                     \
    hipLaunchKernelGGL((logits_row_kernel<T, MODE, true>), grid, dim3(256), 0, stream, lg, row_stride, vocab,     \
                       seg_len, n_splits, draft, cu, batch, temperature, noise, part_val, part_idx, stat_max,     \
                       stat_sum, p_draft, row_index, bonus_rows, rows);                                           \
  else                                                                                                            \
    hipLaunchKernelGGL((logits_row_kernel<T, MODE, false>), grid, dim3(256), 0, stream, lg, row_stride, vocab,    \
                       seg_len, n_splits, draft, cu, batch, temperature, noise, part_val, part_idx, stat_max,     \
                       stat_sum, p_draft, row_index, bonus_rows, rows);
    if (!random) {
      AIC_ROW_LAUNCH(0)
    } else {
      AIC_ROW_LAUNCH(1)
      int rc = launch_status("logits_row_kernel<stats>");
      if (rc != AIC_OK) return rc;
      AIC_ROW_LAUNCH(2)
    }
#undef AIC_ROW_LAUNCH
    int rc = launch_status("logits_row_kernel");
    if (rc != AIC_OK) return rc;
  }
  if (random)
    hipLaunchKernelGGL((accept_kernel<true>), dim3(batch), dim3(64), 0, stream, part_val, part_idx, n_splits, draft,
                       cu, bonus, temperature, uniform, p_draft, max_spec_len, out, nacc, last, hidx, bonus_rows ? rows : -1);
  else
    hipLaunchKernelGGL((accept_kernel<false>), dim3(batch), dim3(64), 0, stream, part_val, part_idx, n_splits, draft,
                       cu, bonus, temperature, uniform, p_draft, max_spec_len, out, nacc, last, hidx, bonus_rows ? rows : -1);
  return launch_status("accept_kernel");
}

static int dispatch(const void* logits, int dtype, int64_t row_stride, int vocab, const int32_t* draft,
                    const int32_t* cu, const int32_t* bonus, const float* temperature, const double* uniform,
                    const float* noise, int batch, int rows, int max_spec_len, int32_t* out, int32_t* nacc,
                    int32_t* last, int32_t* hidx, const int64_t* row_index, const int64_t* bonus_rows, void* ws, void* stream,
                    bool random) {
  if (batch == 0) return AIC_OK;
  AIC_REQUIRE(cu && (bonus || bonus_rows) && out && batch > 0 && rows >= 0 && vocab > 0, "bad arguments to rejection");
  AIC_REQUIRE(rows == 0 || (logits && draft && ws), "null logits / draft ids / workspace");
  AIC_REQUIRE(!bonus_rows || (!random && logits && ws), "bonus rows are folded into the greedy launch only");
  AIC_REQUIRE(max_spec_len >= 0 && max_spec_len + 1 <= 64, "max_spec_len must be <= 63 (one lane per position)");
  AIC_REQUIRE(!random || (temperature && uniform && noise), "random rejection needs temperature, uniform and noise");
  AIC_NEED_DEVICE();
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (dtype) {
    case AIC_DT_F32:
      return run_rejection<float>(logits, row_stride, vocab, draft, cu, bonus, temperature, uniform, noise, batch,
                                  rows, max_spec_len, out, nacc, last, hidx, row_index, bonus_rows, ws, s, random);
    case AIC_DT_BF16:
      return run_rejection<bf16_t>(logits, row_stride, vocab, draft, cu, bonus, temperature, uniform, noise, batch,
                                   rows, max_spec_len, out, nacc, last, hidx, row_index, bonus_rows, ws, s, random);
    case AIC_DT_F16:
      return run_rejection<f16_t>(logits, row_stride, vocab, draft, cu, bonus, temperature, uniform, noise, batch,
                                  rows, max_spec_len, out, nacc, last, hidx, row_index, bonus_rows, ws, s, random);
    default:
      set_error("unsupported logits dtype %d", dtype);
      return AIC_ERR_UNSUPPORTED;
  }
}


// ================================================================================================
// Top-k / top-p rows (aic_rejection_random_topk_topp): vLLM 0.9.2's compute_probs / apply_top_k_top_p restated as a
// radix select on the order-preserving key of x = round(l / T), never a sort.
//
// Launches over the grid (rows, S) — S vocab segments per row, the split of aic_rejection_random:
//   stats   logits_row_kernel<T, 1>: per-segment (max, sum exp) partials, unchanged;
//   K d     top-k, digit d (8 bits, most significant first): per-segment LDS count histogram of the keys whose higher
//           digits equal the prefix chosen so far;
//   P d     mass histogram (fixed point, 2^-40 units of exp(x - max), integer LDS atomics: order-free, deterministic)
//           over the top-k survivors; P 0 also yields Z_k, the survivors' mass;
//   final   p = exp(x - max) / Z_kept over kept tokens, 0 elsewhere: p[draft] and the recovered-token partials that
//           accept_kernel<true> reads, in the workspace layout of aic_rejection_random.
// Every launch folds the previous launch's per-segment histograms of its row in its prologue (fixed segment order) and
// picks the next digit; per-row state and histograms are ping-ponged between launches.  Keys are 16 bits for bf16 /
// fp16 (two digit passes) and 32 bits for f32 (four).  Rows without a filter leave the K / P launches at once and take
// exactly the arithmetic of aic_rejection_random's mode-2 pass.  The token sampler at the end of this file instantiates the
// same kernels with SAMPLER: x is not rounded, so its keys are 32 bits for every storage type.
// ================================================================================================
template <typename T>
struct KeyOf;
template <>
struct KeyOf<float> {
  static constexpr int kBits = 32;
  static __device__ __forceinline__ uint32_t key(float x) {
    const uint32_t b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  }
};
template <>
struct KeyOf<bf16_t> {
  static constexpr int kBits = 16;
  static __device__ __forceinline__ uint32_t key(float x) {  // x is bf16-exact: its low 16 bits are zero
    const uint32_t b = __float_as_uint(x) >> 16;
    return (b & 0x8000u) ? (~b & 0xFFFFu) : (b | 0x8000u);
  }
};
template <>
struct KeyOf<f16_t> {
  static constexpr int kBits = 16;
  static __device__ __forceinline__ uint32_t key(float x) {
    const uint32_t b = f32_to_f16(x);
    return (b & 0x8000u) ? (~b & 0xFFFFu) : (b | 0x8000u);
  }
};
// value-based rules: -0 and +0 are the same value
template <typename T>
__device__ __forceinline__ uint32_t key_of(float x) { return KeyOf<T>::key(x == 0.0f ? 0.0f : x); }

// Key width and key of x: those of the storage type for the rejection sampler (x is rounded to it), 32 bits whatever
// the storage type for the token sampler (x stays f32; rounding merges values, so 16-bit keys would keep other sets).
template <typename T, bool SAMPLER>
struct Arith {
  static constexpr int kBits = SAMPLER ? 32 : KeyOf<T>::kBits;
  static __device__ __forceinline__ uint32_t key(float x) { return SAMPLER ? key_of<float>(x) : key_of<T>(x); }
};

constexpr float kMassScale = 1099511627776.0f;  // 2^40: fixed-point unit of the mass histograms
constexpr double kMassUnit = 1.0 / 1099511627776.0;
typedef unsigned long long u64;

__device__ __forceinline__ u64 fixed_mass(float e) { return static_cast<u64>(e * kMassScale); }

enum { kPassStats = -1, kPassK = 0, kPassP = 1, kPassFinal = 2 };

struct TopState {
  u64 krem;      // top-k: k minus the tokens above the prefix's range
  u64 prem;      // top-p: T minus the mass below the prefix's range
  u64 zk;        // mass of the top-k survivors
  u64 thr;       // T = floor((1 - p) * zk)
  float m;       // row max of x
  uint32_t kprefix, pprefix, pad;
};

struct TopkArgs {
  const void* logits;
  int64_t row_stride;
  const int32_t* draft;
  const int32_t* cu;
  const float* temperature;
  const float* exp_noise;
  const int32_t* top_k;
  const float* top_p;
  const int64_t* row_index;
  float* part_val;
  int32_t* part_idx;
  const float* stat_max;
  const float* stat_sum;
  float* p_draft;
  TopState* state;  // [2][rows]
  uint32_t* cnt;    // [2][rows][n_splits][256]
  u64* mass;        // [2][rows][n_splits][256]
  int batch, rows, vocab, seg_len, n_splits;
  int launch;       // 0 for the first launch after the stats pass: ping-pong parity
  int digit;        // digit of this K / P pass
  int prev_pass, prev_digit;
};

struct RowFilter {
  int req;
  float temp;
  bool greedy, fk, fp;
  int k;
  float p;
};

// SAMPLER: temperature / top_k / top_p / noise are per row (a.cu is unused)
template <bool SAMPLER>
__device__ __forceinline__ RowFilter row_filter(const TopkArgs& a, int row) {
  RowFilter f;
  f.req = SAMPLER ? row : request_of_row(a.cu, a.batch, row);
  f.temp = a.temperature[f.req];
  f.greedy = !(f.temp > 0.0f);
  if constexpr (SAMPLER) {
    if (!a.exp_noise) f.greedy = true;  // the sampler without noise: every row is greedy
  }
  f.k = a.top_k ? a.top_k[f.req] : 0;
  f.p = a.top_p ? a.top_p[f.req] : 1.0f;
  f.fk = !f.greedy && f.k > 0 && f.k < a.vocab;  // k <= 0 or k >= vocab: no top-k
  f.fp = !f.greedy && f.p < 1.0f;                // p >= 1: no top-p
  return f;
}

// Visits the elements of [begin, end) of a row (thread-strided, 16-byte loads when VEC_OK).
template <typename T, bool VEC_OK, typename F>
__device__ __forceinline__ void for_each_elem(const T* base, int begin, int end, F&& f) {
  constexpr int V = Elem<T>::kVec;
  if (VEC_OK) {
    for (int i = begin + threadIdx.x * V; i < end; i += 256 * V) {
      if (i + V <= end) {
        T buf[V];
        *reinterpret_cast<uint4*>(buf) = *reinterpret_cast<const uint4*>(base + i);
#pragma unroll
        for (int e = 0; e < V; ++e) f(i + e, Elem<T>::get(buf, e));
      } else {
        for (int e = 0; i + e < end; ++e) f(i + e, Elem<T>::get(base + i, e));
      }
    }
  } else {
    for (int i = begin + threadIdx.x; i < end; i += 256) f(i, Elem<T>::get(base + i, 0));
  }
}

// Sum of the previous launch's per-segment histograms of `row`, in segment order: s_c / s_m [256].
__device__ void fold_hist(const TopkArgs& a, int row, bool want_mass, u64* s_c, u64* s_m) {
  const size_t base = (static_cast<size_t>((a.launch - 1) & 1) * a.rows + row) * a.n_splits * 256 + threadIdx.x;
  u64 c = 0, m = 0;
  for (int s = 0; s < a.n_splits; ++s) {
    c += a.cnt[base + static_cast<size_t>(s) * 256];
    if (want_mass) m += a.mass[base + static_cast<size_t>(s) * 256];
  }
  s_c[threadIdx.x] = c;
  s_m[threadIdx.x] = m;
}

// Wave 0: the first bin (ascending bins if `asc`, else descending) at which the running sum of s_val exceeds `target`,
// the sum before it (the last bin if the sum never does) and the total; the same answer in every lane.
struct Sel {
  int bin;
  u64 before, total;
};
__device__ Sel select_bin(const u64* s_val, bool asc, u64 target) {
  const int lane = threadIdx.x;
  u64 v[4], sum = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int j = lane * 4 + i;
    v[i] = s_val[asc ? j : 255 - j];
    sum += v[i];
  }
  u64 incl = sum;
  for (int off = 1; off < 64; off <<= 1) {
    const u64 t = __shfl_up(incl, off);
    if (lane >= off) incl += t;
  }
  const unsigned long long hit = __ballot(incl > target);
  const int L = hit ? (__ffsll(static_cast<long long>(hit)) - 1) : 63;
  u64 cum = incl - sum;
  int i = 0;
  for (; i < 3; ++i) {
    if (cum + v[i] > target) break;
    cum += v[i];
  }
  const int j = lane * 4 + i;
  Sel r;
  r.bin = __shfl(asc ? j : 255 - j, L);
  r.before = __shfl(cum, L);
  r.total = __shfl(incl, 63);
  return r;
}

__device__ __forceinline__ int digit_shift(int bits, int d) { return bits - 8 * (d + 1); }
__device__ __forceinline__ bool prefix_match(uint32_t key, uint32_t prefix, int bits, int d) {
  return d == 0 || (key >> (bits - 8 * d)) == (prefix >> (bits - 8 * d));
}

// Block-wide exclusive prefix sum of `c` in thread order; `total` gets the block's sum.
__device__ __forceinline__ int block_excl_scan(int c, int* s_w, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = c;
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_up(incl, off);
    if (lane >= off) incl += t;
  }
  if (lane == 63) s_w[wave] = incl;
  __syncthreads();
  int before = 0;
  for (int w = 0; w < wave; ++w) before += s_w[w];
  *total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
  __syncthreads();
  return before + incl - c;
}


template <typename T, int PASS, bool VEC_OK, bool SAMPLER = false>
__global__ void __launch_bounds__(256) topk_row_kernel(TopkArgs a) {
  using A = Arith<T, SAMPLER>;
  constexpr int BITS = A::kBits;
  const int row = blockIdx.x;
  const int seg = blockIdx.y;
  const int tid = threadIdx.x;
  const int begin = seg * a.seg_len;
  const int end = min(begin + a.seg_len, a.vocab);
  const RowFilter f = row_filter<SAMPLER>(a, row);
  const bool filtered = f.fk || f.fp;
  if (PASS != kPassFinal && !filtered) return;  // unfiltered and greedy rows only take the final pass
  const T* base = static_cast<const T*>(a.logits) + (a.row_index ? a.row_index[row] : static_cast<int64_t>(row)) * a.row_stride;

  __shared__ u64 s_c[256], s_m[256];  // folded histograms of the previous launch
  __shared__ uint32_t s_hc[256];      // this block's histograms
  __shared__ u64 s_hm[256];
  __shared__ TopState s_st;
  __shared__ float s_rmax, s_rz, s_zf;
  __shared__ uint32_t s_tau_p;
  __shared__ int s_dlocal, s_ties_here;
  __shared__ int s_w[4];
  __shared__ float s_v[4];
  __shared__ int s_i[4];

  // ---- the row's softmax statistics, folded exactly as the mode-2 pass of aic_rejection_random folds them
  float row_max = 0.0f, row_z = 1.0f;
  if (!f.greedy) {
    if (tid < 64) {
      float m = -INFINITY;
      for (int s = tid; s < a.n_splits; s += 64) m = fmaxf(m, a.stat_max[row * a.n_splits + s]);
      m = wave_max(m);
      float z = 0.0f;
      for (int s = tid; s < a.n_splits; s += 64) {
        const float pm = a.stat_max[row * a.n_splits + s];
        if (pm > -INFINITY) z += a.stat_sum[row * a.n_splits + s] * __expf(pm - m);
      }
      z = wave_sum(z);
      if (tid == 0) {
        s_rmax = m;
        s_rz = z;
      }
    }
    __syncthreads();
    row_max = s_rmax;
    row_z = s_rz;
  }

  // ---- fold the previous launch's histograms into the row's selection state
  if (filtered) {
    if (tid == 0) {
      TopState st;
      if (a.launch == 0) {
        st.krem = static_cast<u64>(f.fk ? f.k : 0);
        st.prem = st.zk = st.thr = 0;
        st.kprefix = st.pprefix = st.pad = 0;
      } else {
        st = a.state[static_cast<size_t>((a.launch - 1) & 1) * a.rows + row];
      }
      s_st = st;
    }
    const bool fold_k = a.prev_pass == kPassK && f.fk;
    const bool fold_p = a.prev_pass == kPassP && (a.prev_digit == 0 || f.fp);
    if (fold_k || fold_p) fold_hist(a, row, fold_p, s_c, s_m);
    __syncthreads();
    if (tid < 64 && (fold_k || fold_p)) {
      TopState st = s_st;
      if (fold_k) {  // the bin of the k-th largest key, counting from the top
        const Sel s = select_bin(s_c, false, st.krem - 1);
        st.kprefix |= static_cast<uint32_t>(s.bin) << digit_shift(BITS, a.prev_digit);
        st.krem -= s.before;
      } else {
        if (a.prev_digit == 0) {  // Z_k and T = (1 - p) Z_k
          st.zk = select_bin(s_m, true, ~0ull).total;
          if (f.fp) {
            st.thr = f.p > 0.0f ? static_cast<u64>(static_cast<double>(st.zk) * (1.0 - static_cast<double>(f.p)))
                                : st.zk - 1;  // p <= 0: only the largest survivor stays
            st.prem = st.thr;
          }
        }
        if (f.fp) {  // the first bin, counting from the bottom, whose cumulative mass exceeds T
          const Sel s = select_bin(s_m, true, st.prem);
          st.pprefix |= static_cast<uint32_t>(s.bin) << digit_shift(BITS, a.prev_digit);
          st.prem -= s.before;
          if (PASS == kPassFinal && tid == 0) {
            // boundary value tau_p: its n ties carry qe each; the lowest d of them (index order) are dropped, d the
            // number of j in 1..n with L + j qe <= T (prem = T - L); the largest survivor always stays
            const u64 n = s_c[s.bin];
            const u64 qe = n ? s_m[s.bin] / n : 0;
            u64 d = qe ? st.prem / qe : 0;
            if (d > n) d = n;
            if (st.pprefix == A::key(row_max) && d >= n) d = n ? n - 1 : 0;
            const u64 zkept = st.zk - (st.thr - st.prem) - d * qe;
            s_zf = static_cast<float>(static_cast<double>(zkept) * kMassUnit);
            s_tau_p = st.pprefix;
            const size_t hb = (static_cast<size_t>((a.launch - 1) & 1) * a.rows + row) * a.n_splits * 256 + (st.pprefix & 0xFF);
            u64 before = 0;
            for (int s2 = 0; s2 < seg; ++s2) before += a.cnt[hb + static_cast<size_t>(s2) * 256];
            s_ties_here = static_cast<int>(a.cnt[hb + static_cast<size_t>(seg) * 256]);
            s_dlocal = d > before ? static_cast<int>(d - before) : 0;
          }
        }
      }
      if (tid == 0) s_st = st;
    }
    if (PASS == kPassFinal && tid == 0 && !f.fp) {
      s_zf = static_cast<float>(static_cast<double>(s_st.zk) * kMassUnit);
      s_tau_p = 0;
      s_dlocal = 0;
      s_ties_here = 0;
    }
    __syncthreads();
    if (PASS != kPassFinal && seg == 0 && tid == 0) a.state[static_cast<size_t>(a.launch & 1) * a.rows + row] = s_st;
  }

  if (PASS != kPassFinal) {
    if (PASS == kPassK ? !f.fk : (a.digit > 0 && !f.fp)) return;
    const TopState st = s_st;
    const int d = a.digit;
    const int sh = digit_shift(BITS, d);
    const uint32_t prefix = PASS == kPassK ? st.kprefix : st.pprefix;
    const bool cut_k = PASS == kPassP && f.fk;
    s_hc[tid] = 0;
    s_hm[tid] = 0;
    __syncthreads();
    // runs of equal bins are added to LDS once (the high digits of a row's keys take few values)
    int cur = -1;
    uint32_t cc = 0;
    u64 cm = 0;
    auto flush = [&]() {
      if (cur >= 0) {
        atomicAdd(&s_hc[cur], cc);
        if (PASS == kPassP) atomicAdd(&s_hm[cur], cm);
      }
    };
    for_each_elem<T, VEC_OK>(base, begin, end, [&](int idx, float l) {
      (void)idx;
      const float x = scaled_logit<T, SAMPLER>(l, f.temp);
      const uint32_t key = A::key(x);
      if (!prefix_match(key, prefix, BITS, d)) return;
      u64 q = 0;
      if (PASS == kPassP) {
        if (cut_k && key < st.kprefix) return;
        q = fixed_mass(__expf(x - row_max));
        if (q == 0) return;  // no mass: below any top-p boundary, nothing to add to Z_k
      }
      const int b = (key >> sh) & 0xFF;
      if (b != cur) {
        flush();
        cur = b;
        cc = 0;
        cm = 0;
      }
      ++cc;
      cm += q;
    });
    flush();
    __syncthreads();
    const size_t o = (static_cast<size_t>(a.launch & 1) * a.rows + row) * a.n_splits * 256 + static_cast<size_t>(seg) * 256 + tid;
    a.cnt[o] = s_hc[tid];
    if (PASS == kPassP) a.mass[o] = s_hm[tid];
    return;
  }

  // ---- final pass: p over the kept set, p[draft], recovered-token partials (SAMPLER: no draft token is removed)
  const int draft = SAMPLER ? -1 : a.draft[row];
  const float* q = a.exp_noise + static_cast<int64_t>(f.req) * a.vocab;
  const uint32_t tau_k = s_st.kprefix, tau_p = s_tau_p;
  const float zf = s_zf;
  const int dlocal = s_dlocal, ties_here = s_ties_here;
  Best best;
  best.v = -INFINITY;
  best.i = begin;
  auto visit = [&](int idx, float l, bool tie_keep) {
    if (f.greedy) {
      if (l > best.v) {
        best.v = l;
        best.i = idx;
      }
      return;
    }
    const float x = scaled_logit<T, SAMPLER>(l, f.temp);
    float p;
    if (!filtered) {
      p = __fdiv_rn(__expf(x - row_max), row_z);
    } else {
      const uint32_t key = A::key(x);
      const bool kept = (!f.fk || key >= tau_k) && (!f.fp || key > tau_p || (key == tau_p && tie_keep));
      p = kept ? __fdiv_rn(__expf(x - row_max), zf) : 0.0f;
    }
    if (!SAMPLER && idx == draft) {
      a.p_draft[row] = p;
      p = 0.0f;
    }
    const float r = __fdiv_rn(p, q[idx]);
    if (r > best.v) {
      best.v = r;
      best.i = idx;
    }
  };
  if (f.fp && dlocal > 0 && dlocal < ties_here) {
    // the cut falls inside this segment's ties: rank them in index order (8 contiguous elements per thread)
    const int n_iter = (end - begin + 2047) / 2048;
    int seen = 0;
    for (int it = 0; it < n_iter; ++it) {
      const int i0 = begin + it * 2048 + tid * 8;
      float lv[8];
      int c = 0;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        lv[e] = i0 + e < end ? Elem<T>::get(base, i0 + e) : 0.0f;
        if (i0 + e < end && A::key(scaled_logit<T, SAMPLER>(lv[e], f.temp)) == tau_p) ++c;
      }
      int total;
      int rank = seen + block_excl_scan(c, s_w, &total);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if (i0 + e >= end) continue;
        const bool tie = A::key(scaled_logit<T, SAMPLER>(lv[e], f.temp)) == tau_p;
        visit(i0 + e, lv[e], !tie || rank >= dlocal);
        rank += tie;
      }
      seen += total;
    }
  } else {
    const bool keep_ties = dlocal <= 0;  // 0 < ties_here <= dlocal: every tie of this segment is dropped
    for_each_elem<T, VEC_OK>(base, begin, end, [&](int idx, float l) { visit(idx, l, keep_ties); });
  }

  const int wave = tid >> 6, lane = tid & 63;
  best = wave_best(best);
  if (lane == 0) {
    s_v[wave] = best.v;
    s_i[wave] = best.i;
  }
  __syncthreads();
  if (tid == 0) {
    Best b;
    b.v = s_v[0];
    b.i = s_i[0];
    for (int w = 1; w < 4; ++w) {
      Best o;
      o.v = s_v[w];
      o.i = s_i[w];
      b = better(b, o);
    }
    a.part_val[row * a.n_splits + seg] = b.v;
    a.part_idx[row * a.n_splits + seg] = b.i;
  }
}

// The K / P digit passes and the final pass of one call, after its stats pass: `a` is filled but for the pass fields.
template <typename T, bool SAMPLER>
static int run_select_passes(TopkArgs& a, dim3 grid, bool vec_ok, hipStream_t stream) {
  a.launch = 0;
  a.digit = 0;
  a.prev_pass = kPassStats;
  a.prev_digit = 0;
  auto go = [&](int pass, int digit) -> int {
    a.digit = digit;
#define AIC_TOPK_LAUNCH(P)                                                                                       \
  if (vec_ok)                                                                                                    \
    hipLaunchKernelGGL((topk_row_kernel<T, P, true, SAMPLER>), grid, dim3(256), 0, stream, a);                  \
  else                                                                                                           \
    hipLaunchKernelGGL((topk_row_kernel<T, P, false, SAMPLER>), grid, dim3(256), 0, stream, a);
    if (pass == kPassK) {
      AIC_TOPK_LAUNCH(kPassK)
    } else if (pass == kPassP) {
      AIC_TOPK_LAUNCH(kPassP)
    } else {
      AIC_TOPK_LAUNCH(kPassFinal)
    }
#undef AIC_TOPK_LAUNCH
    a.prev_pass = pass;
    a.prev_digit = digit;
    ++a.launch;
    return launch_status("topk_row_kernel");
  };
  constexpr int digits = Arith<T, SAMPLER>::kBits / 8;
  int rc = AIC_OK;
  if (a.top_k)
    for (int d = 0; d < digits && rc == AIC_OK; ++d) rc = go(kPassK, d);
  if (rc == AIC_OK && (a.top_k || a.top_p)) rc = go(kPassP, 0);  // Z_k (and the first top-p digit)
  if (a.top_p)
    for (int d = 1; d < digits && rc == AIC_OK; ++d) rc = go(kPassP, d);
  if (rc == AIC_OK) rc = go(kPassFinal, 0);
  return rc;
}

static void split_geometry(int rows, int vocab, int* seg_len, int* n_splits) {
  const int S = rows > 0 ? pick_splits(rows, vocab) : 1;
  int len = (vocab + S - 1) / S;
  len = (len + kSegQuantum - 1) / kSegQuantum * kSegQuantum;
  *seg_len = len;
  *n_splits = (vocab + len - 1) / len;
}

static size_t topk_region_offset(int rows, int vocab);

template <typename T>
static int run_rejection_topk(const void* logits, int64_t row_stride, int vocab, const int32_t* draft,
                              const int32_t* cu, const int32_t* bonus, const float* temperature, const double* uniform,
                              const float* noise, const int32_t* top_k, const float* top_p, int batch, int rows,
                              int max_spec_len, int32_t* out, int32_t* nacc, int32_t* last, int32_t* hidx,
                              const int64_t* row_index, void* workspace, hipStream_t stream) {
  int seg_len, n_splits;
  split_geometry(rows, vocab, &seg_len, &n_splits);
  // the layout of aic_rejection_random (accept_kernel<true> reads it unchanged), then the selection state
  float* part_val = static_cast<float*>(workspace);
  const size_t wr = static_cast<size_t>(rows);
  int32_t* part_idx = reinterpret_cast<int32_t*>(part_val + wr * kMaxSplits);
  float* stat_max = reinterpret_cast<float*>(part_idx + wr * kMaxSplits);
  float* stat_sum = stat_max + wr * kMaxSplits;
  float* p_draft = stat_sum + wr * kMaxSplits;
  TopState* state = reinterpret_cast<TopState*>(static_cast<char*>(workspace) + topk_region_offset(rows, vocab));
  uint32_t* cnt = reinterpret_cast<uint32_t*>(state + 2 * wr);
  u64* mass = reinterpret_cast<u64*>(cnt + 2 * wr * n_splits * 256);
  const T* lg = static_cast<const T*>(logits);
  const bool vec_ok = (reinterpret_cast<uintptr_t>(logits) % 16 == 0) && ((row_stride * sizeof(T)) % 16 == 0);
  if (rows > 0) {
    dim3 grid(rows, n_splits);
    if (vec_ok)
      hipLaunchKernelGGL((logits_row_kernel<T, 1, true>), grid, dim3(256), 0, stream, lg, row_stride, vocab, seg_len,
                         n_splits, draft, cu, batch, temperature, noise, part_val, part_idx, stat_max, stat_sum,
                         p_draft, row_index, nullptr, rows);
    else
      hipLaunchKernelGGL((logits_row_kernel<T, 1, false>), grid, dim3(256), 0, stream, lg, row_stride, vocab, seg_len,
                         n_splits, draft, cu, batch, temperature, noise, part_val, part_idx, stat_max, stat_sum,
                         p_draft, row_index, nullptr, rows);
    int rc = launch_status("logits_row_kernel<stats>");
    if (rc != AIC_OK) return rc;
    TopkArgs a;
    a.logits = logits;
    a.row_stride = row_stride;
    a.draft = draft;
    a.cu = cu;
    a.temperature = temperature;
    a.exp_noise = noise;
    a.top_k = top_k;
    a.top_p = top_p;
    a.row_index = row_index;
    a.part_val = part_val;
    a.part_idx = part_idx;
    a.stat_max = stat_max;
    a.stat_sum = stat_sum;
    a.p_draft = p_draft;
    a.state = state;
    a.cnt = cnt;
    a.mass = mass;
    a.batch = batch;
    a.rows = rows;
    a.vocab = vocab;
    a.seg_len = seg_len;
    a.n_splits = n_splits;
    rc = run_select_passes<T, false>(a, grid, vec_ok, stream);
    if (rc != AIC_OK) return rc;
  }
  hipLaunchKernelGGL((accept_kernel<true>), dim3(batch), dim3(64), 0, stream, part_val, part_idx, n_splits, draft, cu,
                     bonus, temperature, uniform, p_draft, max_spec_len, out, nacc, last, hidx, -1);
  return launch_status("accept_kernel");
}

static size_t topk_region_offset(int rows, int vocab) {
  const size_t r = static_cast<size_t>(rows > 0 ? rows : 1);
  const size_t base = r * kMaxSplits * 4 * sizeof(float) + r * sizeof(float) + 256;  // aic_rejection_workspace_bytes
  (void)vocab;
  return (base + 255) / 256 * 256;
}

static size_t topk_workspace_bytes(int rows, int vocab) {
  int seg_len, n_splits;
  split_geometry(rows, vocab, &seg_len, &n_splits);
  const size_t r = static_cast<size_t>(rows > 0 ? rows : 1);
  return topk_region_offset(rows, vocab) + 2 * r * sizeof(TopState) +
         2 * r * static_cast<size_t>(n_splits) * 256 * (sizeof(uint32_t) + sizeof(u64)) + 256;
}

static int dispatch_topk(const void* logits, int dtype, int64_t row_stride, int vocab, const int32_t* draft,
                         const int32_t* cu, const int32_t* bonus, const float* temperature, const double* uniform,
                         const float* noise, const int32_t* top_k, const float* top_p, int batch, int rows,
                         int max_spec_len, int32_t* out, int32_t* nacc, int32_t* last, int32_t* hidx,
                         const int64_t* row_index, void* ws, void* stream) {
  if (!top_k && !top_p)  // no filter anywhere: aic_rejection_random itself
    return dispatch(logits, dtype, row_stride, vocab, draft, cu, bonus, temperature, uniform, noise, batch, rows,
                    max_spec_len, out, nacc, last, hidx, row_index, nullptr, ws, stream, true);
  if (batch == 0) return AIC_OK;
  AIC_REQUIRE(cu && bonus && out && batch > 0 && rows >= 0 && vocab > 0, "bad arguments to rejection");
  AIC_REQUIRE(rows == 0 || (logits && draft && ws), "null logits / draft ids / workspace");
  AIC_REQUIRE(max_spec_len >= 0 && max_spec_len + 1 <= 64, "max_spec_len must be <= 63 (one lane per position)");
  AIC_REQUIRE(temperature && uniform && noise, "random rejection needs temperature, uniform and noise");
  AIC_NEED_DEVICE();
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (dtype) {
    case AIC_DT_F32:
      return run_rejection_topk<float>(logits, row_stride, vocab, draft, cu, bonus, temperature, uniform, noise, top_k,
                                       top_p, batch, rows, max_spec_len, out, nacc, last, hidx, row_index, ws, s);
    case AIC_DT_BF16:
      return run_rejection_topk<bf16_t>(logits, row_stride, vocab, draft, cu, bonus, temperature, uniform, noise, top_k,
                                        top_p, batch, rows, max_spec_len, out, nacc, last, hidx, row_index, ws, s);
    case AIC_DT_F16:
      return run_rejection_topk<f16_t>(logits, row_stride, vocab, draft, cu, bonus, temperature, uniform, noise, top_k,
                                       top_p, batch, rows, max_spec_len, out, nacc, last, hidx, row_index, ws, s);
    default:
      set_error("unsupported logits dtype %d", dtype);
      return AIC_ERR_UNSUPPORTED;
  }
}

// ================================================================================================
// Token sampler (aic_sample_topk_topp): vLLM 0.9.2's Sampler for temperature / top-k / top-p.  Sampling a token from a
// filtered row is the recovered-token computation with no draft token removed, on x = f32(l) / T kept in f32: the
// SAMPLER instantiations of the kernels above (32-bit keys whatever the storage type, per-row temperature and
// filters), then one wavefront per row that reduces the per-segment partials to the token.
// ================================================================================================
__global__ void __launch_bounds__(64)
sample_finish_kernel(const float* __restrict__ part_val, const int32_t* __restrict__ part_idx, int n_splits,
                     int32_t* __restrict__ out) {
  const int row = blockIdx.x;
  Best b;
  b.v = -INFINITY;
  b.i = INT_MAX;
  for (int s = threadIdx.x; s < n_splits; s += 64) {
    Best o;
    o.v = part_val[row * n_splits + s];
    o.i = part_idx[row * n_splits + s];
    b = better(b, o);
  }
  b = wave_best(b);
  if (threadIdx.x == 0) out[row] = b.i;
}

template <typename T>
static int run_sample(const void* logits, int64_t row_stride, int vocab, const int64_t* row_index,
                      const float* temperature, const float* noise, const int32_t* top_k, const float* top_p, int rows,
                      int32_t* out, void* workspace, hipStream_t stream) {
  int seg_len, n_splits;
  split_geometry(rows, vocab, &seg_len, &n_splits);
  float* part_val = static_cast<float*>(workspace);  // the layout of run_rejection_topk
  const size_t wr = static_cast<size_t>(rows);
  int32_t* part_idx = reinterpret_cast<int32_t*>(part_val + wr * kMaxSplits);
  float* stat_max = reinterpret_cast<float*>(part_idx + wr * kMaxSplits);
  float* stat_sum = stat_max + wr * kMaxSplits;
  TopState* state = reinterpret_cast<TopState*>(static_cast<char*>(workspace) + topk_region_offset(rows, vocab));
  uint32_t* cnt = reinterpret_cast<uint32_t*>(state + 2 * wr);
  u64* mass = reinterpret_cast<u64*>(cnt + 2 * wr * n_splits * 256);
  const T* lg = static_cast<const T*>(logits);
  const bool vec_ok = (reinterpret_cast<uintptr_t>(logits) % 16 == 0) && ((row_stride * sizeof(T)) % 16 == 0);
  dim3 grid(rows, n_splits);
  if (vec_ok)
    hipLaunchKernelGGL((logits_row_kernel<T, 1, true, true>), grid, dim3(256), 0, stream, lg, row_stride, vocab, seg_len,
                       n_splits, nullptr, nullptr, rows, temperature, noise, part_val, part_idx, stat_max, stat_sum,
                       nullptr, row_index, nullptr, rows);
  else
    hipLaunchKernelGGL((logits_row_kernel<T, 1, false, true>), grid, dim3(256), 0, stream, lg, row_stride, vocab, seg_len,
                       n_splits, nullptr, nullptr, rows, temperature, noise, part_val, part_idx, stat_max, stat_sum,
                       nullptr, row_index, nullptr, rows);
  int rc = launch_status("logits_row_kernel<stats>");
  if (rc != AIC_OK) return rc;
  TopkArgs a;
  a.logits = logits;
  a.row_stride = row_stride;
  a.draft = nullptr;
  a.cu = nullptr;
  a.temperature = temperature;
  a.exp_noise = noise;
  a.top_k = top_k;
  a.top_p = top_p;
  a.row_index = row_index;
  a.part_val = part_val;
  a.part_idx = part_idx;
  a.stat_max = stat_max;
  a.stat_sum = stat_sum;
  a.p_draft = nullptr;
  a.state = state;
  a.cnt = cnt;
  a.mass = mass;
  a.batch = rows;
  a.rows = rows;
  a.vocab = vocab;
  a.seg_len = seg_len;
  a.n_splits = n_splits;
  rc = run_select_passes<T, true>(a, grid, vec_ok, stream);
  if (rc != AIC_OK) return rc;
  hipLaunchKernelGGL(sample_finish_kernel, dim3(rows), dim3(64), 0, stream, part_val, part_idx, n_splits, out);
  return launch_status("sample_finish_kernel");
}

static int dispatch_sample(const void* logits, int dtype, int64_t row_stride, int vocab, const int64_t* row_index,
                           const float* temperature, const float* noise, const int32_t* top_k, const float* top_p,
                           int rows, int32_t* out, void* ws, void* stream) {
  if (rows == 0) return AIC_OK;
  AIC_REQUIRE(rows > 0 && vocab > 0 && row_stride >= 0, "bad arguments to the sampler");
  AIC_REQUIRE(logits && temperature && out && ws, "null logits / temperature / output / workspace");
  AIC_NEED_DEVICE();
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (dtype) {
    case AIC_DT_F32:
      return run_sample<float>(logits, row_stride, vocab, row_index, temperature, noise, top_k, top_p, rows, out, ws, s);
    case AIC_DT_BF16:
      return run_sample<bf16_t>(logits, row_stride, vocab, row_index, temperature, noise, top_k, top_p, rows, out, ws, s);
    case AIC_DT_F16:
      return run_sample<f16_t>(logits, row_stride, vocab, row_index, temperature, noise, top_k, top_p, rows, out, ws, s);
    default:
      set_error("unsupported logits dtype %d", dtype);
      return AIC_ERR_UNSUPPORTED;
  }
}

// ================================================================================================
// Token logprobs (aic_token_logprobs): vLLM 0.9.2's Sampler.compute_logprobs + gather_logprobs on the raw rows, for the
// steps whose tokens the kernels above draw.  Launches over the grid (rows, S), the split of the sampler:
//   first    per-segment (max, arg-max) partials and the count histogram of the keys' first digit;
//   digit d  folds the previous histogram (the select of a top-k with k = n, on the raw values' keys: 16 bits for
//            bf16 / fp16, 32 for f32) and counts digit d; the launch of digit 1 knows the row maximum m and the selected
//            token's value, so the fixed-point sum of exp(x - m) and the rank count ride in it;
//   gather   everything above the cut value, and the ties at it from the lowest index up, into <= 32 candidate slots
//            (slot order is arbitrary: an integer atomic hands them out);
//   finish   one wavefront per row: folds the partials, orders the candidates by (value descending, index ascending)
//            and writes the row's outputs.
// n = 0 needs no select: first, the sum launch, finish: 2 passes over the row.  With n > 0 a bf16 / fp16 row is read 3
// times (first, digit 1, gather) and an f32 row 5 times; aic_sample_topk_topp with both filters on reads either 10 times.
// ================================================================================================
constexpr int kLogprobsMax = 32;
enum { kLpFirst = 0, kLpDigit = 1, kLpGather = 2 };

struct LpState {
  uint32_t prefix;  // the cut key's digits chosen so far
  uint32_t krem;    // n minus the entries above the prefix's range
};

struct LpArgs {
  const void* logits;
  int64_t row_stride;
  const int64_t* row_index;
  const int32_t* token_ids;
  float* part_val;     // [rows][n_splits] per-segment maximum
  int32_t* part_idx;   //                  and its lowest index
  u64* seg_sum;        // [rows][n_splits] sum exp(x - m) in 2^-40 units
  int32_t* seg_ge;     // [rows][n_splits] #{x >= x_token}
  LpState* state;      // [digits + 1][rows], entry L written by launch L
  uint32_t* cnt;       // [2][rows][n_splits][256]
  int32_t* cand_n;     // [rows]
  float* cand_val;     // [rows][kLogprobsMax]
  int32_t* cand_idx;
  int rows, vocab, seg_len, n_splits, n;
  int launch;          // kLpDigit: this pass's digit; kLpGather: the number of digits
  int with_sum, with_hist;
};

__device__ __forceinline__ u64 wave_sum_u64(u64 x) {
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
  return x;
}

template <typename T, int KIND, bool VEC_OK>
__global__ void __launch_bounds__(256) logprobs_row_kernel(LpArgs a) {
  constexpr int BITS = KeyOf<T>::kBits;
  const int row = blockIdx.x;
  const int seg = blockIdx.y;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int begin = seg * a.seg_len;
  const int end = min(begin + a.seg_len, a.vocab);
  const T* base = static_cast<const T*>(a.logits) + (a.row_index ? a.row_index[row] : static_cast<int64_t>(row)) * a.row_stride;

  __shared__ u64 s_c[256];        // folded histogram of the previous launch
  __shared__ uint32_t s_hc[256];  // this block's histogram
  __shared__ LpState s_st;
  __shared__ float s_m;
  __shared__ int s_need, s_here;
  __shared__ int s_w[4];
  __shared__ float s_v[4];
  __shared__ int s_i[4];
  __shared__ u64 s_q[4];

  if (KIND == kLpFirst) {
    if (a.with_hist) s_hc[tid] = 0;
    __syncthreads();
    Best best;
    best.v = -INFINITY;
    best.i = begin;
    int cur = -1;
    uint32_t cc = 0;
    for_each_elem<T, VEC_OK>(base, begin, end, [&](int idx, float l) {
      if (l > best.v) {
        best.v = l;
        best.i = idx;
      }
      if (a.with_hist) {
        const int b = key_of<T>(l) >> (BITS - 8);
        if (b != cur) {
          if (cur >= 0) atomicAdd(&s_hc[cur], cc);
          cur = b;
          cc = 0;
        }
        ++cc;
      }
    });
    if (cur >= 0) atomicAdd(&s_hc[cur], cc);
    best = wave_best(best);
    if (lane == 0) {
      s_v[wave] = best.v;
      s_i[wave] = best.i;
    }
    __syncthreads();
    if (tid == 0) {
      Best b;
      b.v = s_v[0];
      b.i = s_i[0];
      for (int w = 1; w < 4; ++w) {
        Best o;
        o.v = s_v[w];
        o.i = s_i[w];
        b = better(b, o);
      }
      a.part_val[row * a.n_splits + seg] = b.v;
      a.part_idx[row * a.n_splits + seg] = b.i;
      if (seg == 0) a.cand_n[row] = 0;
    }
    if (a.with_hist)
      a.cnt[(static_cast<size_t>(row) * a.n_splits + seg) * 256 + tid] = s_hc[tid];
    return;
  }

  // ---- the row's maximum; the select state after the previous launch's histogram
  const int L = a.launch;
  if (tid < 64) {
    Best b;
    b.v = -INFINITY;
    b.i = INT_MAX;
    for (int s = tid; s < a.n_splits; s += 64) {
      Best o;
      o.v = a.part_val[row * a.n_splits + s];
      o.i = a.part_idx[row * a.n_splits + s];
      b = better(b, o);
    }
    b = wave_best(b);
    if (tid == 0) s_m = b.v;
  }
  const size_t prev_hist = (static_cast<size_t>((L - 1) & 1) * a.rows + row) * a.n_splits * 256;
  if (a.n > 0) {
    u64 c = 0;
    for (int s = 0; s < a.n_splits; ++s) c += a.cnt[prev_hist + static_cast<size_t>(s) * 256 + tid];
    s_c[tid] = c;
    if (tid == 0) {
      LpState st;
      st.prefix = 0;
      st.krem = static_cast<uint32_t>(a.n);
      if (L > 1) st = a.state[static_cast<size_t>(L - 1) * a.rows + row];
      s_st = st;
    }
  }
  __syncthreads();
  if (a.n > 0) {
    if (tid < 64) {  // the bin of the n-th largest key, counting from the top
      LpState st = s_st;
      const Sel s = select_bin(s_c, false, static_cast<u64>(st.krem) - 1);
      st.prefix |= static_cast<uint32_t>(s.bin) << digit_shift(BITS, L - 1);
      st.krem -= static_cast<uint32_t>(s.before);
      if (tid == 0) {
        s_st = st;
        if (KIND == kLpDigit && seg == 0) a.state[static_cast<size_t>(L) * a.rows + row] = st;
        if (KIND == kLpGather) {  // the cut value's ties: how many the earlier segments hold, and this one
          const size_t hb = prev_hist + (st.prefix & 0xFF);
          u64 before = 0;
          for (int s2 = 0; s2 < seg; ++s2) before += a.cnt[hb + static_cast<size_t>(s2) * 256];
          s_here = static_cast<int>(a.cnt[hb + static_cast<size_t>(seg) * 256]);
          s_need = before >= st.krem ? 0 : static_cast<int>(st.krem - before);
        }
      }
    }
    __syncthreads();
  }
  const float m = s_m;

  if (KIND == kLpDigit) {
    float xtok = m;  // token_ids == NULL: the arg-max
    if (a.token_ids) {
      const int tok = a.token_ids[row];
      xtok = (tok >= 0 && tok < a.vocab) ? Elem<T>::get(base, tok) : NAN;  // never indexed out of the row
    }
    const uint32_t prefix = s_st.prefix;
    const int sh = digit_shift(BITS, L);
    if (a.with_hist) s_hc[tid] = 0;
    __syncthreads();
    u64 acc = 0;
    int ge = 0;
    int cur = -1;
    uint32_t cc = 0;
    for_each_elem<T, VEC_OK>(base, begin, end, [&](int idx, float l) {
      (void)idx;
      if (a.with_sum) {
        if (l > -INFINITY) acc += fixed_mass(expf(l - m));
        ge += l >= xtok;
      }
      if (a.with_hist) {
        const uint32_t key = key_of<T>(l);
        if (!prefix_match(key, prefix, BITS, L)) return;
        const int b = (key >> sh) & 0xFF;
        if (b != cur) {
          if (cur >= 0) atomicAdd(&s_hc[cur], cc);
          cur = b;
          cc = 0;
        }
        ++cc;
      }
    });
    if (cur >= 0) atomicAdd(&s_hc[cur], cc);
    if (a.with_sum) {
      acc = wave_sum_u64(acc);
      for (int off = 32; off > 0; off >>= 1) ge += __shfl_xor(ge, off);
      if (lane == 0) {
        s_q[wave] = acc;
        s_w[wave] = ge;
      }
    }
    __syncthreads();
    if (a.with_sum && tid == 0) {
      a.seg_sum[row * a.n_splits + seg] = s_q[0] + s_q[1] + s_q[2] + s_q[3];
      a.seg_ge[row * a.n_splits + seg] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    }
    if (a.with_hist)
      a.cnt[((static_cast<size_t>(L & 1) * a.rows + row) * a.n_splits + seg) * 256 + tid] = s_hc[tid];
    return;
  }

  // ---- gather: the entries above the cut value tau, and tau's ties from the lowest index up
  const uint32_t tau = s_st.prefix;
  const int need = s_need, here = s_here;
  auto push = [&](int idx, float l) {
    const int slot = atomicAdd(&a.cand_n[row], 1);
    if (slot < kLogprobsMax) {
      a.cand_val[row * kLogprobsMax + slot] = l;
      a.cand_idx[row * kLogprobsMax + slot] = idx;
    }
  };
  if (need > 0 && need < here) {
    // the cut falls inside this segment's ties: rank them in index order (8 contiguous elements per thread)
    const int n_iter = (end - begin + 2047) / 2048;
    int seen = 0;
    for (int it = 0; it < n_iter; ++it) {
      const int i0 = begin + it * 2048 + tid * 8;
      float lv[8];
      int c = 0;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        lv[e] = i0 + e < end ? Elem<T>::get(base, i0 + e) : 0.0f;
        if (i0 + e < end && key_of<T>(lv[e]) == tau) ++c;
      }
      int total;
      int rank = seen + block_excl_scan(c, s_w, &total);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if (i0 + e >= end) continue;
        const uint32_t key = key_of<T>(lv[e]);
        if (key > tau) {
          push(i0 + e, lv[e]);
        } else if (key == tau) {
          if (rank < need) push(i0 + e, lv[e]);
          ++rank;
        }
      }
      seen += total;
    }
  } else {
    const bool take_ties = need > 0;  // need >= here: every tie of this segment is inside the cut
    for_each_elem<T, VEC_OK>(base, begin, end, [&](int idx, float l) {
      const uint32_t key = key_of<T>(l);
      if (key > tau || (key == tau && take_ties)) push(idx, l);
    });
  }
}

template <typename T>
__global__ void __launch_bounds__(64)
logprobs_finish_kernel(LpArgs a, int32_t* __restrict__ out_ids, float* __restrict__ out_lp, int64_t* __restrict__ out_rank) {
  const int row = blockIdx.x;
  const int lane = threadIdx.x;
  Best b;
  b.v = -INFINITY;
  b.i = INT_MAX;
  u64 sum = 0;
  long long ge = 0;
  for (int s = lane; s < a.n_splits; s += 64) {
    Best o;
    o.v = a.part_val[row * a.n_splits + s];
    o.i = a.part_idx[row * a.n_splits + s];
    b = better(b, o);
    sum += a.seg_sum[row * a.n_splits + s];
    ge += a.seg_ge[row * a.n_splits + s];
  }
  b = wave_best(b);
  sum = wave_sum_u64(sum);
  ge = static_cast<long long>(wave_sum_u64(static_cast<u64>(ge)));
  const float m = b.v;
  const float log_s = logf(static_cast<float>(static_cast<double>(sum) * kMassUnit));
  const int cols = 1 + a.n;
  if (lane == 0) {
    int tok = b.i;
    float xtok = m;
    if (a.token_ids) {
      const T* base = static_cast<const T*>(a.logits) + (a.row_index ? a.row_index[row] : static_cast<int64_t>(row)) * a.row_stride;
      tok = a.token_ids[row];
      xtok = (tok >= 0 && tok < a.vocab) ? Elem<T>::get(base, tok) : NAN;
    }
    out_ids[static_cast<size_t>(row) * cols] = tok;
    out_lp[static_cast<size_t>(row) * cols] = (xtok - m) - log_s;
    out_rank[row] = ge;
  }
  if (a.n == 0) return;
  // order the candidates: position = how many of the others come first (value descending, index ascending)
  const int cn = min(a.cand_n[row], a.n);
  Best c;
  c.v = -INFINITY;
  c.i = INT_MAX;
  if (lane < cn) {
    c.v = a.cand_val[row * kLogprobsMax + lane];
    c.i = a.cand_idx[row * kLogprobsMax + lane];
  }
  int pos = 0;
  for (int k = 0; k < cn; ++k) {
    const float vk = __shfl(c.v, k);
    const int ik = __shfl(c.i, k);
    pos += (vk > c.v) || (vk == c.v && ik < c.i);
  }
  if (lane < cn) {
    out_ids[static_cast<size_t>(row) * cols + 1 + pos] = c.i;
    out_lp[static_cast<size_t>(row) * cols + 1 + pos] = (c.v - m) - log_s;
  } else if (lane < a.n) {  // fewer than n entries can only come from NaN logits, which are outside the contract
    out_ids[static_cast<size_t>(row) * cols + 1 + lane] = -1;
    out_lp[static_cast<size_t>(row) * cols + 1 + lane] = NAN;
  }
}

static size_t lp_align(size_t x) { return (x + 255) / 256 * 256; }

static size_t logprobs_workspace_bytes(int rows, int vocab) {
  int seg_len, n_splits;
  split_geometry(rows, vocab, &seg_len, &n_splits);
  const size_t r = static_cast<size_t>(rows > 0 ? rows : 1);
  return lp_align(r * kMaxSplits * sizeof(u64)) + lp_align(5 * r * sizeof(LpState)) +
         3 * lp_align(r * kMaxSplits * sizeof(int32_t)) + lp_align(r * sizeof(int32_t)) +
         2 * lp_align(r * kLogprobsMax * sizeof(int32_t)) +
         lp_align(2 * r * static_cast<size_t>(n_splits) * 256 * sizeof(uint32_t)) + 256;
}

template <typename T>
static int run_logprobs(const void* logits, int64_t row_stride, int vocab, const int64_t* row_index,
                        const int32_t* token_ids, int rows, int n, int32_t* out_ids, float* out_lp, int64_t* out_rank,
                        void* workspace, hipStream_t stream) {
  LpArgs a;
  split_geometry(rows, vocab, &a.seg_len, &a.n_splits);
  const size_t r = static_cast<size_t>(rows);
  char* p = static_cast<char*>(workspace);
  auto carve = [&](size_t bytes) {
    char* q = p;
    p += lp_align(bytes);
    return q;
  };
  a.seg_sum = reinterpret_cast<u64*>(carve(r * kMaxSplits * sizeof(u64)));
  a.state = reinterpret_cast<LpState*>(carve(5 * r * sizeof(LpState)));
  a.part_val = reinterpret_cast<float*>(carve(r * kMaxSplits * sizeof(float)));
  a.part_idx = reinterpret_cast<int32_t*>(carve(r * kMaxSplits * sizeof(int32_t)));
  a.seg_ge = reinterpret_cast<int32_t*>(carve(r * kMaxSplits * sizeof(int32_t)));
  a.cand_n = reinterpret_cast<int32_t*>(carve(r * sizeof(int32_t)));
  a.cand_val = reinterpret_cast<float*>(carve(r * kLogprobsMax * sizeof(float)));
  a.cand_idx = reinterpret_cast<int32_t*>(carve(r * kLogprobsMax * sizeof(int32_t)));
  a.cnt = reinterpret_cast<uint32_t*>(carve(2 * r * static_cast<size_t>(a.n_splits) * 256 * sizeof(uint32_t)));
  a.logits = logits;
  a.row_stride = row_stride;
  a.row_index = row_index;
  a.token_ids = token_ids;
  a.rows = rows;
  a.vocab = vocab;
  a.n = n;
  const bool vec_ok = (reinterpret_cast<uintptr_t>(logits) % 16 == 0) && ((row_stride * sizeof(T)) % 16 == 0);
  const dim3 grid(rows, a.n_splits);
  auto go = [&](int kind, int launch, bool with_sum, bool with_hist) -> int {
    a.launch = launch;
    a.with_sum = with_sum;
    a.with_hist = with_hist;
#define AIC_LP_LAUNCH(K)                                                                          \
  if (vec_ok)                                                                                     \
    hipLaunchKernelGGL((logprobs_row_kernel<T, K, true>), grid, dim3(256), 0, stream, a);         \
  else                                                                                            \
    hipLaunchKernelGGL((logprobs_row_kernel<T, K, false>), grid, dim3(256), 0, stream, a);
    if (kind == kLpFirst) {
      AIC_LP_LAUNCH(kLpFirst)
    } else if (kind == kLpDigit) {
      AIC_LP_LAUNCH(kLpDigit)
    } else {
      AIC_LP_LAUNCH(kLpGather)
    }
#undef AIC_LP_LAUNCH
    return launch_status("logprobs_row_kernel");
  };
  constexpr int digits = KeyOf<T>::kBits / 8;
  int rc = go(kLpFirst, 0, false, n > 0);
  if (rc == AIC_OK) rc = go(kLpDigit, 1, true, n > 0);
  if (n > 0) {
    for (int d = 2; d < digits && rc == AIC_OK; ++d) rc = go(kLpDigit, d, false, true);
    if (rc == AIC_OK) rc = go(kLpGather, digits, false, false);
  }
  if (rc != AIC_OK) return rc;
  hipLaunchKernelGGL((logprobs_finish_kernel<T>), dim3(rows), dim3(64), 0, stream, a, out_ids, out_lp, out_rank);
  return launch_status("logprobs_finish_kernel");
}

static int dispatch_logprobs(const void* logits, int dtype, int64_t row_stride, int vocab, const int64_t* row_index,
                             const int32_t* token_ids, int rows, int n, int32_t* out_ids, float* out_lp,
                             int64_t* out_rank, void* ws, void* stream) {
  AIC_REQUIRE(n >= 0 && n <= kLogprobsMax, "num_logprobs %d outside 0 .. %d", n, kLogprobsMax);
  if (dtype != AIC_DT_F32 && dtype != AIC_DT_BF16 && dtype != AIC_DT_F16) {
    set_error("unsupported logits dtype %d", dtype);
    return AIC_ERR_UNSUPPORTED;
  }
  if (rows == 0) return AIC_OK;
  AIC_REQUIRE(rows > 0 && vocab > 0 && row_stride >= 0, "bad arguments to the logprobs call");
  AIC_REQUIRE(n <= vocab, "num_logprobs %d exceeds the vocabulary %d", n, vocab);
  AIC_REQUIRE(logits && out_ids && out_lp && out_rank && ws, "null logits / outputs / workspace");
  AIC_NEED_DEVICE();
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (dtype) {
    case AIC_DT_F32:
      return run_logprobs<float>(logits, row_stride, vocab, row_index, token_ids, rows, n, out_ids, out_lp, out_rank, ws, s);
    case AIC_DT_BF16:
      return run_logprobs<bf16_t>(logits, row_stride, vocab, row_index, token_ids, rows, n, out_ids, out_lp, out_rank, ws, s);
    default:
      return run_logprobs<f16_t>(logits, row_stride, vocab, row_index, token_ids, rows, n, out_ids, out_lp, out_rank, ws, s);
  }
}


// ================================================================================================
// Greedy acceptance over tree-shaped drafts (aic_rejection_tree_greedy).  The reference accepts paths only
// (arctic_inference/vllm/model_runner.py:405-411 hands vLLM's RejectionSampler a chain); the rule over a tree is the
// same walk with a choice of child: emit the arg-max of the current node's row, step to the child that carries it.
// Phase 1 is the greedy row phase above, unchanged, over all T query rows (logits_row_kernel MODE 0: per-segment
// (max, arg-max) partials, ties to the lowest index).  Phase 2 is one wavefront per request: lane t folds row t's
// partials, learns through one shuffle whether node t carries its parent's arg-max, and the walk is a ballot + ffs per
// level — wave-uniform, at most q_len - 1 levels.
// ================================================================================================
__global__ void __launch_bounds__(64)
tree_accept_kernel(const float* __restrict__ part_val, const int32_t* __restrict__ part_idx, int n_splits,
                   const int32_t* __restrict__ draft_ids, const int32_t* __restrict__ parent,
                   const int32_t* __restrict__ qsl, int width, int32_t* __restrict__ out, int32_t* __restrict__ num_accepted,
                   int32_t* __restrict__ last_token, int32_t* __restrict__ hidden_index, int32_t* __restrict__ path) {
  const int req = blockIdx.x;
  const int lane = threadIdx.x;
  const int start = qsl[req];
  const int n = min(qsl[req + 1] - start, 64);   // one lane per node
  int amax = -1, par = -1, tok = -1;
  if (lane < n) {
    const int row = start + lane;
    Best b;
    b.v = part_val[row * n_splits];
    b.i = part_idx[row * n_splits];
    for (int s = 1; s < n_splits; ++s) {
      Best o;
      o.v = part_val[row * n_splits + s];
      o.i = part_idx[row * n_splits + s];
      b = better(b, o);
    }
    amax = b.i;
    if (lane > 0) {
      par = parent[row];
      tok = draft_ids[row];
    }
  }
  // node t continues the walk from its parent iff it carries the parent's arg-max (a parent precedes its child)
  const int par_amax = __shfl(amax, min(max(par, 0), 63));
  const bool carries = lane > 0 && lane < n && par >= 0 && par < lane && tok == par_amax;
  int cur = 0, depth = 0, my_tok = -1, my_node = -1, last = -1;
  while (n > 0) {
    const int a = __shfl(amax, cur);
    if (lane == depth) {
      my_tok = a;
      my_node = cur;
    }
    last = a;
    ++depth;
    const unsigned long long next = __ballot(carries && par == cur);
    if (!next) break;
    cur = __ffsll(static_cast<long long>(next)) - 1;   // the lowest child that carries it (siblings carry distinct tokens)
  }
  if (lane < width) {
    out[static_cast<int64_t>(req) * width + lane] = my_tok;
    if (path) path[static_cast<int64_t>(req) * width + lane] = my_node;
  }
  if (lane == 0) {
    if (num_accepted) num_accepted[req] = depth;
    if (last_token) last_token[req] = last;
    if (hidden_index) hidden_index[req] = start + cur;
  }
}

template <typename T>
static int run_rejection_tree(const void* logits, int64_t row_stride, int vocab, const int32_t* draft,
                              const int32_t* parent, const int32_t* qsl, int batch, int rows, int max_q_len, int32_t* out,
                              int32_t* nacc, int32_t* last, int32_t* hidx, int32_t* path, const int64_t* row_index,
                              void* workspace, hipStream_t stream) {
  const int S = pick_splits(rows, vocab);
  int seg_len = (vocab + S - 1) / S;
  seg_len = (seg_len + kSegQuantum - 1) / kSegQuantum * kSegQuantum;
  const int n_splits = (vocab + seg_len - 1) / seg_len;
  float* part_val = static_cast<float*>(workspace);
  int32_t* part_idx = reinterpret_cast<int32_t*>(part_val + static_cast<size_t>(rows) * kMaxSplits);
  const T* lg = static_cast<const T*>(logits);
  const bool vec_ok = (reinterpret_cast<uintptr_t>(logits) % 16 == 0) && ((row_stride * sizeof(T)) % 16 == 0);
  const dim3 grid(rows, n_splits);
  // MODE 0 reads neither the draft ids, the request offsets nor the random-row state
  if (vec_ok)
    hipLaunchKernelGGL((logits_row_kernel<T, 0, true>), grid, dim3(256), 0, stream, lg, row_stride, vocab, seg_len, n_splits,
                       nullptr, nullptr, batch, nullptr, nullptr, part_val, part_idx, nullptr, nullptr, nullptr, row_index,
                       nullptr, rows);
  else
    hipLaunchKernelGGL((logits_row_kernel<T, 0, false>), grid, dim3(256), 0, stream, lg, row_stride, vocab, seg_len, n_splits,
                       nullptr, nullptr, batch, nullptr, nullptr, part_val, part_idx, nullptr, nullptr, nullptr, row_index,
                       nullptr, rows);
  int rc = launch_status("logits_row_kernel");
  if (rc != AIC_OK) return rc;
  hipLaunchKernelGGL(tree_accept_kernel, dim3(batch), dim3(64), 0, stream, part_val, part_idx, n_splits, draft, parent, qsl,
                     max_q_len, out, nacc, last, hidx, path);
  return launch_status("tree_accept_kernel");
}

}  // namespace aic

using namespace aic;

extern "C" {

size_t aic_rejection_workspace_bytes(int num_draft_total, int vocab) {
  (void)vocab;
  const size_t rows = static_cast<size_t>(num_draft_total > 0 ? num_draft_total : 1);
  return rows * kMaxSplits * 4 * sizeof(float) + rows * sizeof(float) + 256;
}

int aic_rejection_greedy(const void* target_logits, int logits_dtype, int64_t row_stride, int vocab,
                         const int32_t* draft_token_ids, const int32_t* cu_num_draft, const int32_t* bonus_token_ids,
                         int batch, int num_draft_total, int max_spec_len, int32_t* out_token_ids,
                         int32_t* num_accepted, int32_t* last_token, int32_t* hidden_index,
                         const int64_t* target_row_index, const int64_t* bonus_row_index, void* workspace,
                         void* stream) {
  return dispatch(target_logits, logits_dtype, row_stride, vocab, draft_token_ids, cu_num_draft, bonus_token_ids,
                  nullptr, nullptr, nullptr, batch, num_draft_total, max_spec_len, out_token_ids, num_accepted,
                  last_token, hidden_index, target_row_index, bonus_row_index, workspace, stream, false);
}

int aic_rejection_tree_greedy(const void* target_logits, int logits_dtype, int64_t row_stride, int vocab,
                              const int32_t* draft_token_ids, const int32_t* parent, const int32_t* query_start_loc,
                              int batch, int num_tokens, int max_q_len, int32_t* out_token_ids, int32_t* num_accepted,
                              int32_t* last_token, int32_t* hidden_index, int32_t* path, const int64_t* row_index,
                              void* workspace, void* stream) {
  if (batch == 0) return AIC_OK;
  AIC_REQUIRE(target_logits && draft_token_ids && parent && query_start_loc && out_token_ids && workspace,
              "null pointer argument to aic_rejection_tree_greedy");
  AIC_REQUIRE(batch > 0 && num_tokens > 0 && vocab > 0, "non-positive size argument");
  AIC_REQUIRE(max_q_len >= 1 && max_q_len <= 64, "max_q_len must be 1 .. 64 (one lane per node)");
  if (logits_dtype != AIC_DT_F32 && logits_dtype != AIC_DT_BF16 && logits_dtype != AIC_DT_F16) {
    set_error("unsupported logits dtype %d", logits_dtype);
    return AIC_ERR_UNSUPPORTED;
  }
  AIC_NEED_DEVICE();
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (logits_dtype) {
    case AIC_DT_F32:
      return run_rejection_tree<float>(target_logits, row_stride, vocab, draft_token_ids, parent, query_start_loc, batch,
                                       num_tokens, max_q_len, out_token_ids, num_accepted, last_token, hidden_index, path,
                                       row_index, workspace, s);
    case AIC_DT_BF16:
      return run_rejection_tree<bf16_t>(target_logits, row_stride, vocab, draft_token_ids, parent, query_start_loc, batch,
                                        num_tokens, max_q_len, out_token_ids, num_accepted, last_token, hidden_index, path,
                                        row_index, workspace, s);
    default:
      return run_rejection_tree<f16_t>(target_logits, row_stride, vocab, draft_token_ids, parent, query_start_loc, batch,
                                       num_tokens, max_q_len, out_token_ids, num_accepted, last_token, hidden_index, path,
                                       row_index, workspace, s);
  }
}

int aic_rejection_random(const void* target_logits, int logits_dtype, int64_t row_stride, int vocab,
                         const int32_t* draft_token_ids, const int32_t* cu_num_draft, const int32_t* bonus_token_ids,
                         const float* temperature, const double* uniform, const float* exp_noise, int batch,
                         int num_draft_total, int max_spec_len, int32_t* out_token_ids, int32_t* num_accepted,
                         int32_t* last_token, int32_t* hidden_index, const int64_t* target_row_index, void* workspace,
                         void* stream) {
  return dispatch(target_logits, logits_dtype, row_stride, vocab, draft_token_ids, cu_num_draft, bonus_token_ids,
                  temperature, uniform, exp_noise, batch, num_draft_total, max_spec_len, out_token_ids, num_accepted,
                  last_token, hidden_index, target_row_index, nullptr, workspace, stream, true);
}

size_t aic_rejection_topk_topp_workspace_bytes(int num_draft_total, int vocab, int logits_dtype) {
  (void)logits_dtype;  // the key width changes the number of passes, not the state
  return topk_workspace_bytes(num_draft_total, vocab > 0 ? vocab : 1);
}

int aic_rejection_random_topk_topp(const void* target_logits, int logits_dtype, int64_t row_stride, int vocab,
                                   const int32_t* draft_token_ids, const int32_t* cu_num_draft,
                                   const int32_t* bonus_token_ids, const float* temperature, const double* uniform,
                                   const float* exp_noise, const int32_t* top_k, const float* top_p, int batch,
                                   int num_draft_total, int max_spec_len, int32_t* out_token_ids, int32_t* num_accepted,
                                   int32_t* last_token, int32_t* hidden_index, const int64_t* target_row_index,
                                   void* workspace, void* stream) {
  return dispatch_topk(target_logits, logits_dtype, row_stride, vocab, draft_token_ids, cu_num_draft, bonus_token_ids,
                       temperature, uniform, exp_noise, top_k, top_p, batch, num_draft_total, max_spec_len,
                       out_token_ids, num_accepted, last_token, hidden_index, target_row_index, workspace, stream);
}

size_t aic_sample_workspace_bytes(int rows, int vocab, int logits_dtype) {
  (void)logits_dtype;  // the keys are 32 bits whatever the storage type
  return topk_workspace_bytes(rows, vocab > 0 ? vocab : 1);
}

int aic_sample_topk_topp(const void* logits, int logits_dtype, int64_t row_stride, int vocab, const int64_t* row_index,
                         const float* temperature, const float* exp_noise, const int32_t* top_k, const float* top_p,
                         int rows, int32_t* out_token_ids, void* workspace, void* stream) {
  return dispatch_sample(logits, logits_dtype, row_stride, vocab, row_index, temperature, exp_noise, top_k, top_p, rows,
                         out_token_ids, workspace, stream);
}

int aic_logprobs_max(void) { return kLogprobsMax; }

size_t aic_logprobs_workspace_bytes(int rows, int vocab, int logits_dtype, int num_logprobs) {
  (void)logits_dtype;  // the key width and n change the number of passes, not the state
  (void)num_logprobs;
  return logprobs_workspace_bytes(rows, vocab > 0 ? vocab : 1);
}

int aic_token_logprobs(const void* logits, int logits_dtype, int64_t row_stride, int vocab, const int64_t* row_index,
                       const int32_t* token_ids, int rows, int num_logprobs, int32_t* out_token_ids, float* out_logprobs,
                       int64_t* out_ranks, void* workspace, void* stream) {
  return dispatch_logprobs(logits, logits_dtype, row_stride, vocab, row_index, token_ids, rows, num_logprobs,
                           out_token_ids, out_logprobs, out_ranks, workspace, stream);
}

}  // extern "C"
