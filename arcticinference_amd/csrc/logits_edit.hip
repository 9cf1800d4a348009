// Logits edits (aic_logits_edit): the edits vLLM 0.9.2's Sampler makes to a row before it samples it — the allowed-token
// mask, bad words and the min_tokens stop ids, the logit bias, the repetition / frequency / presence penalties and
// min-p — as one pass from the raw rows (bf16 / fp16 / f32, read in place) to contiguous f32 rows.  The raw rows are
// never written: vLLM reports logprobs of the raw logits, and aic_token_logprobs keeps reading them.
//
// Launch 1, grid (row, segment of kSegment tokens), kThreads threads:
//   walk     the workgroup reads its row's ban, bias, prompt and output lists (int32 CSR; a few thousand entries, L2
//            hits for every segment after the first) and marks the tokens of ITS segment in one 32-bit LDS word per
//            token with integer LDS atomics: bits 0..29 the output count (atomic add), bit 30 "a ban or a bias names
//            this token" (atomic or), bit 31 "in the prompt" (atomic or).  No [rows, V] count matrix in HBM, nothing
//            to zero there.  A row whose lists are all empty skips the walk and the LDS altogether.
//   stream   16-byte loads of the raw row, everything in registers, 16-byte stores of the f32 row; a token with bit 30
//            set looks its ban / bias up in the (short) lists.  Each arithmetic step rounds once in f32 (the file is
//            built with -ffp-contract=off and the steps use the _rn intrinsics), the reciprocal is an IEEE division.
//            The segment's maximum of the edited values goes to the workspace when min-p is asked for.
// Launch 2 (only with min_p), same grid: rows with temperature > 0 and min_p > 0 fold the row's segment maxima and set
//   everything with (x - m) / T < ln(min_p) to -inf; every other row returns at once.
//
// kSegment * 4 B = 32 KiB (+ 32 B of partial maxima) of LDS per workgroup of 8 wavefronts: the 160 KiB of a CU hold 4 such
// workgroups = 32 wavefronts, all a CU can hold (8 per SIMD), so the LDS array does not bound the occupancy of the
// streaming part below the wavefront limit.
#include <hip/hip_runtime.h>

#include <cmath>

#include "aic_common.h"

namespace aic {
namespace {

constexpr int kSegment = 8192;
constexpr int kThreads = 512;
constexpr uint32_t kPromptBit = 1u << 31;
constexpr uint32_t kListedBit = 1u << 30;
constexpr uint32_t kCountMask = kListedBit - 1u;

struct EditArgs {
  const void* logits;
  int64_t row_stride;
  const int64_t* row_index;
  const uint8_t* mask;
  const int32_t* ban_off;
  const int32_t* ban_tok;
  const int32_t* bias_off;
  const int32_t* bias_tok;
  const float* bias_val;
  const int32_t* prompt_off;
  const int32_t* prompt_tok;
  const int32_t* out_off;
  const int32_t* out_tok;
  const float* rep;
  const float* freq;
  const float* pres;
  float* out;
  float* seg_max;
  int vocab, n_seg;
  int n_ban, n_bias, n_prompt, n_out;
};

struct bf16x { uint16_t b; };
struct f16x { uint16_t b; };
__device__ inline float to_f32(float v) { return v; }
__device__ inline float to_f32(bf16x v) { return bf16_to_f32(v.b); }
__device__ inline float to_f32(f16x v) { return f16_to_f32(v.b); }

// [begin, end) of one row of a CSR list, held inside [0, count] whatever the offsets say
__device__ inline void csr_range(const int32_t* off, int row, int count, int* begin, int* end) {
  *begin = *end = 0;
  if (!off) return;
  const int b = min(max(off[row], 0), count);
  const int e = min(max(off[row + 1], b), count);
  *begin = b;
  *end = e;
}

struct RowEdit {
  const int32_t* ban_tok;
  const int32_t* bias_tok;
  const float* bias_val;
  int ban_b, ban_e, bias_b, bias_e;
  float rep, freq, pres;
  bool penalties;
};

// One token: x = f32(raw), `w` its LDS word, `masked` the allowed-token mask's byte.  The order is vLLM's Sampler.forward.
__device__ inline float edit_one(float x, int tok, uint32_t w, bool masked, const RowEdit& r) {
  if (masked) x = -INFINITY;
  if (w & kListedBit) {
    for (int j = r.ban_b; j < r.ban_e; ++j)
      if (r.ban_tok[j] == tok) x = -INFINITY;
    for (int j = r.bias_b; j < r.bias_e; ++j)
      if (r.bias_tok[j] == tok) x = __fadd_rn(x, r.bias_val[j]);
  }
  if (r.penalties) {
    const uint32_t count = w & kCountMask;
    const bool seen = (w & kPromptBit) || count > 0;
    const float p = seen ? r.rep : 1.0f;
    x = __fmul_rn(x, x > 0.0f ? __fdiv_rn(1.0f, p) : p);
    x = __fsub_rn(x, __fmul_rn(r.freq, static_cast<float>(count)));
    x = __fsub_rn(x, __fmul_rn(r.pres, count > 0 ? 1.0f : 0.0f));
  }
  return x;
}

__device__ inline float wave_max(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

template <typename T, bool VEC>
__global__ void __launch_bounds__(kThreads) logits_edit_kernel(EditArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t word[kSegment];
  __shared__ float part[kThreads / 64];
  const int row = blockIdx.x;
  const int seg = blockIdx.y;
  const int lo = seg * kSegment;
  const int n = min(kSegment, a.vocab - lo);  // > 0: the grid has ceil(vocab / kSegment) segments
  const int tid = threadIdx.x;

  RowEdit r;
  r.ban_tok = a.ban_tok;
  r.bias_tok = a.bias_tok;
  r.bias_val = a.bias_val;
  csr_range(a.ban_off, row, a.n_ban, &r.ban_b, &r.ban_e);
  csr_range(a.bias_off, row, a.n_bias, &r.bias_b, &r.bias_e);
  int pr_b, pr_e, ou_b, ou_e;
  csr_range(a.prompt_off, row, a.n_prompt, &pr_b, &pr_e);
  csr_range(a.out_off, row, a.n_out, &ou_b, &ou_e);
  r.penalties = a.rep || a.freq || a.pres;
  r.rep = a.rep ? a.rep[row] : 1.0f;
  r.freq = a.freq ? a.freq[row] : 0.0f;
  r.pres = a.pres ? a.pres[row] : 0.0f;
  if (!r.penalties) pr_b = pr_e = ou_b = ou_e = 0;  // the histories matter to the penalties only
  const bool listed = r.ban_e > r.ban_b || r.bias_e > r.bias_b || pr_e > pr_b || ou_e > ou_b;  // uniform in the workgroup

  if (listed) {
    for (int i = tid; i < n; i += kThreads) word[i] = 0u;
    __syncthreads();
    const uint32_t ulo = static_cast<uint32_t>(lo), un = static_cast<uint32_t>(n);
    for (int j = r.ban_b + tid; j < r.ban_e; j += kThreads) {
      const uint32_t d = static_cast<uint32_t>(a.ban_tok[j]) - ulo;  // ids outside [0, vocab) fall outside every segment
      if (d < un) atomicOr(&word[d], kListedBit);
    }
    for (int j = r.bias_b + tid; j < r.bias_e; j += kThreads) {
      const uint32_t d = static_cast<uint32_t>(a.bias_tok[j]) - ulo;
      if (d < un) atomicOr(&word[d], kListedBit);
    }
    for (int j = pr_b + tid; j < pr_e; j += kThreads) {
      const uint32_t d = static_cast<uint32_t>(a.prompt_tok[j]) - ulo;
      if (d < un) atomicOr(&word[d], kPromptBit);
    }
    for (int j = ou_b + tid; j < ou_e; j += kThreads) {
      const uint32_t d = static_cast<uint32_t>(a.out_tok[j]) - ulo;
      if (d < un) atomicAdd(&word[d], 1u);  // a row's output is far shorter than 2^30 tokens: the count stays below bit 30
    }
    __syncthreads();
  }

  const int64_t src_row = a.row_index ? a.row_index[row] : static_cast<int64_t>(row);
  const T* src = static_cast<const T*>(a.logits) + src_row * a.row_stride + lo;
  float* dst = a.out + static_cast<size_t>(row) * a.vocab + lo;
  const uint8_t* mk = a.mask ? a.mask + static_cast<size_t>(row) * a.vocab + lo : nullptr;
  float best = -INFINITY;

  int done = 0;
  if constexpr (VEC) {
    // 8 tokens per lane and step: one 16-byte load of a 16-bit row (two of an f32 row), two 16-byte stores
    constexpr int kPer = 8;
    const int n_vec = n / kPer;
    for (int v = tid; v < n_vec; v += kThreads) {
      const int base = v * kPer;
      float x[kPer];
      if constexpr (sizeof(T) == 2) {
        const uint4 q = *reinterpret_cast<const uint4*>(src + base);
        const uint32_t u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          T e0, e1;
          e0.b = static_cast<uint16_t>(u[k] & 0xffffu);
          e1.b = static_cast<uint16_t>(u[k] >> 16);
          x[2 * k] = to_f32(e0);
          x[2 * k + 1] = to_f32(e1);
        }
      } else {
        const float4 q0 = *reinterpret_cast<const float4*>(src + base);
        const float4 q1 = *reinterpret_cast<const float4*>(src + base + 4);
        x[0] = q0.x; x[1] = q0.y; x[2] = q0.z; x[3] = q0.w;
        x[4] = q1.x; x[5] = q1.y; x[6] = q1.z; x[7] = q1.w;
      }
      uint32_t w[kPer];
      if (listed) {
        const uint4 w0 = *reinterpret_cast<const uint4*>(&word[base]);
        const uint4 w1 = *reinterpret_cast<const uint4*>(&word[base + 4]);
        w[0] = w0.x; w[1] = w0.y; w[2] = w0.z; w[3] = w0.w;
        w[4] = w1.x; w[5] = w1.y; w[6] = w1.z; w[7] = w1.w;
      } else {
#pragma unroll
        for (int k = 0; k < kPer; ++k) w[k] = 0u;
      }
#pragma unroll
      for (int k = 0; k < kPer; ++k) {
        x[k] = edit_one(x[k], lo + base + k, w[k], mk && mk[base + k], r);
        best = fmaxf(best, x[k]);
      }
      *reinterpret_cast<float4*>(dst + base) = make_float4(x[0], x[1], x[2], x[3]);
      *reinterpret_cast<float4*>(dst + base + 4) = make_float4(x[4], x[5], x[6], x[7]);
    }
    done = n_vec * kPer;
  }
  // the ragged tail of a row whose length is no multiple of 8, and every token of an unaligned call
  for (int i = done + tid; i < n; i += kThreads) {
    const float x = edit_one(to_f32(src[i]), lo + i, listed ? word[i] : 0u, mk && mk[i], r);
    best = fmaxf(best, x);
    dst[i] = x;
  }

  if (a.seg_max) {
    best = wave_max(best);
    if ((tid & 63) == 0) part[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {
      float m = part[0];
      for (int k = 1; k < kThreads / 64; ++k) m = fmaxf(m, part[k]);
      a.seg_max[static_cast<size_t>(row) * a.n_seg + seg] = m;
    }
  }
}

// min-p on the edited f32 rows: keep v iff (x_v - m) / T >= ln(min_p).  Rows that do not use it return at once.
template <bool VEC>
__global__ void __launch_bounds__(kThreads)
min_p_kernel(float* __restrict__ out, const float* __restrict__ seg_max, const float* __restrict__ min_p,
             const float* __restrict__ temperature, int vocab, int n_seg) {
  const int row = blockIdx.x;
  const float mp = min_p[row];
  const float t = temperature[row];
  if (!(mp > 0.0f) || !(t > 0.0f)) return;
  float m = -INFINITY;
  for (int s = 0; s < n_seg; ++s) m = fmaxf(m, seg_max[static_cast<size_t>(row) * n_seg + s]);
  const float cut = logf(mp);
  const int lo = blockIdx.y * kSegment;
  const int n = min(kSegment, vocab - lo);
  float* dst = out + static_cast<size_t>(row) * vocab + lo;
  const int tid = threadIdx.x;
  int done = 0;
  if constexpr (VEC) {
    const int n_vec = n / 4;
    for (int v = tid; v < n_vec; v += kThreads) {
      float4 q = *reinterpret_cast<float4*>(dst + 4 * v);
      const bool k0 = __fdiv_rn(__fsub_rn(q.x, m), t) >= cut, k1 = __fdiv_rn(__fsub_rn(q.y, m), t) >= cut;
      const bool k2 = __fdiv_rn(__fsub_rn(q.z, m), t) >= cut, k3 = __fdiv_rn(__fsub_rn(q.w, m), t) >= cut;
      if (k0 && k1 && k2 && k3) continue;
      q.x = k0 ? q.x : -INFINITY;
      q.y = k1 ? q.y : -INFINITY;
      q.z = k2 ? q.z : -INFINITY;
      q.w = k3 ? q.w : -INFINITY;
      *reinterpret_cast<float4*>(dst + 4 * v) = q;
    }
    done = n_vec * 4;
  }
  for (int i = done + tid; i < n; i += kThreads)
    if (!(__fdiv_rn(__fsub_rn(dst[i], m), t) >= cut)) dst[i] = -INFINITY;
}

template <typename T>
int run_edit(const EditArgs& a, int rows, const float* min_p, const float* temperature, hipStream_t stream) {
  const uintptr_t in = reinterpret_cast<uintptr_t>(a.logits), out = reinterpret_cast<uintptr_t>(a.out);
  // 16-byte accesses need every row start aligned on both sides: the f32 rows are contiguous, so vocab % 4 == 0
  const bool vec = in % 16 == 0 && (a.row_stride * sizeof(T)) % 16 == 0 && out % 16 == 0 && a.vocab % 4 == 0;
  const dim3 grid(rows, a.n_seg);
  if (vec)
    hipLaunchKernelGGL((logits_edit_kernel<T, true>), grid, dim3(kThreads), 0, stream, a);
  else
    hipLaunchKernelGGL((logits_edit_kernel<T, false>), grid, dim3(kThreads), 0, stream, a);
  int rc = launch_status("logits_edit_kernel");
  if (rc != AIC_OK || !min_p) return rc;
  if (vec)
    hipLaunchKernelGGL((min_p_kernel<true>), grid, dim3(kThreads), 0, stream, a.out, a.seg_max, min_p, temperature,
                       a.vocab, a.n_seg);
  else
    hipLaunchKernelGGL((min_p_kernel<false>), grid, dim3(kThreads), 0, stream, a.out, a.seg_max, min_p, temperature,
                       a.vocab, a.n_seg);
  return launch_status("min_p_kernel");
}

int segments_of(int vocab) { return (vocab + kSegment - 1) / kSegment; }

}  // namespace
}  // namespace aic

extern "C" {

int aic_logits_edit_segment(void) { return aic::kSegment; }

size_t aic_logits_edit_workspace_bytes(int rows, int vocab) {
  if (rows <= 0 || vocab <= 0) return 0;
  return static_cast<size_t>(rows) * aic::segments_of(vocab) * sizeof(float);
}

int aic_logits_edit(const void* logits, int logits_dtype, int64_t row_stride, int vocab, const int64_t* row_index, int rows,
                    const uint8_t* allowed_mask, const int32_t* ban_offsets, const int32_t* ban_tokens, int num_ban,
                    const int32_t* bias_offsets, const int32_t* bias_tokens, const float* bias_values, int num_bias,
                    const int32_t* prompt_offsets, const int32_t* prompt_tokens, int num_prompt,
                    const int32_t* output_offsets, const int32_t* output_tokens, int num_output,
                    const float* repetition, const float* frequency, const float* presence, const float* min_p,
                    const float* temperature, float* out, void* workspace, void* stream) {
  using namespace aic;
  if (rows == 0) return AIC_OK;
  AIC_REQUIRE(rows > 0 && vocab > 0 && row_stride >= 0, "bad arguments to the logits edit");
  AIC_REQUIRE(logits && out, "null logits / output");
  AIC_REQUIRE(num_ban >= 0 && num_bias >= 0 && num_prompt >= 0 && num_output >= 0, "negative list length");
  AIC_REQUIRE(!ban_offsets || ban_tokens || num_ban == 0, "ban_offsets without ban_tokens");
  AIC_REQUIRE(!bias_offsets || (bias_tokens && bias_values) || num_bias == 0, "bias_offsets without tokens / values");
  AIC_REQUIRE(!prompt_offsets || prompt_tokens || num_prompt == 0, "prompt_offsets without prompt_tokens");
  AIC_REQUIRE(!output_offsets || output_tokens || num_output == 0, "output_offsets without output_tokens");
  AIC_REQUIRE(!min_p || temperature, "min_p needs the rows' temperature");
  AIC_REQUIRE(!min_p || workspace, "min_p needs the workspace");
  AIC_REQUIRE(segments_of(vocab) <= 65535, "vocab too large");
  if (logits_dtype != AIC_DT_F32 && logits_dtype != AIC_DT_BF16 && logits_dtype != AIC_DT_F16) {
    set_error("unsupported logits dtype %d", logits_dtype);
    return AIC_ERR_UNSUPPORTED;
  }
  AIC_NEED_DEVICE();
  EditArgs a;
  a.logits = logits;
  a.row_stride = row_stride;
  a.row_index = row_index;
  a.mask = allowed_mask;
  a.ban_off = num_ban ? ban_offsets : nullptr;
  a.ban_tok = ban_tokens;
  a.bias_off = num_bias ? bias_offsets : nullptr;
  a.bias_tok = bias_tokens;
  a.bias_val = bias_values;
  a.prompt_off = num_prompt ? prompt_offsets : nullptr;
  a.prompt_tok = prompt_tokens;
  a.out_off = num_output ? output_offsets : nullptr;
  a.out_tok = output_tokens;
  a.rep = repetition;
  a.freq = frequency;
  a.pres = presence;
  a.out = out;
  a.seg_max = min_p ? static_cast<float*>(workspace) : nullptr;
  a.vocab = vocab;
  a.n_seg = segments_of(vocab);
  a.n_ban = num_ban;
  a.n_bias = num_bias;
  a.n_prompt = num_prompt;
  a.n_out = num_output;
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (logits_dtype) {
    case AIC_DT_F32:
      return run_edit<float>(a, rows, min_p, temperature, s);
    case AIC_DT_BF16:
      return run_edit<bf16x>(a, rows, min_p, temperature, s);
    default:
      return run_edit<f16x>(a, rows, min_p, temperature, s);
  }
}

}  // extern "C"
