"""torch-facing wrappers over the C ABI (include/arctic_hip.h).  PyTorch is plumbing here: it owns
device memory and streams; every op below is a single call into libarctic_hip.so on the current
stream.  Nothing falls back to torch or the CPU — a missing library or device raises.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import torch

from . import _native as N


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _need_cuda(*ts: torch.Tensor) -> None:
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("arcticinference_amd ops run on the GPU only (got a CPU tensor); there is no CPU fallback")


def _check_kv_layout(k_cache: torch.Tensor, v_cache: torch.Tensor) -> None:
    """The cache layout every paged kernel assumes and none can check: [num_blocks, block_size, Hkv, D] with contiguous
    pages (only the block stride is free: it is handed to the kernel), K and V alike.  A permuted view (an HND cache seen
    as [nb, bs, Hkv, D]) would be read or written in the wrong places.  ValueError before anything is launched."""
    if k_cache.dim() != 4:
        raise ValueError(f"a kv cache is [num_blocks, block_size, Hkv, D], not {tuple(k_cache.shape)}")
    nb, bs, Hkv, D = k_cache.shape
    if k_cache.stride(3) != 1 or k_cache.stride(2) != D or k_cache.stride(1) != Hkv * D:
        raise ValueError("caches must be [num_blocks, block_size, Hkv, D] with contiguous pages (strides "
                         f"{tuple(k_cache.stride())} for shape {tuple(k_cache.shape)})")
    if v_cache.shape != k_cache.shape or v_cache.dtype != k_cache.dtype or v_cache.stride() != k_cache.stride():
        raise ValueError("key and value caches must share shape, dtype and strides "
                         f"({tuple(k_cache.shape)} {k_cache.dtype} {tuple(k_cache.stride())} / "
                         f"{tuple(v_cache.shape)} {v_cache.dtype} {tuple(v_cache.stride())})")


# ------------------------------------------------------------------------------------------------
# A16 bulk KV write — same signature as arctic_inference.py_custom_ops.reshape_and_cache_flash_bulk
# (/root/reference/arctic_inference/py_custom_ops.py:40-54)
# ------------------------------------------------------------------------------------------------
_KV_DTYPES = {"auto": None, "fp8": N.DT_FP8_E4M3, "fp8_e4m3": N.DT_FP8_E4M3, "fp8_e5m2": N.DT_FP8_E5M2}


class KvBulkWriter:
    """reshape_and_cache_flash_bulk for a fixed set of caches: the checks and the per-layer pointer tables of the
    wrapper are done once (an engine calls it every step with the same caches)."""

    def __init__(self, key_caches: List[torch.Tensor], value_caches: List[torch.Tensor], kv_cache_dtype: str,
                 k_scales: List[torch.Tensor], v_scales: List[torch.Tensor], num_heads: int, head_size: int):
        L = len(key_caches)
        # same checks as the reference launcher (kernels.cu:103-106)
        if not (L == len(value_caches) == len(k_scales) == len(v_scales)):
            raise RuntimeError("key_caches, value_caches, k_scales and v_scales must have the same length")
        if kv_cache_dtype not in _KV_DTYPES:
            raise RuntimeError(f"unsupported kv cache dtype '{kv_cache_dtype}'")
        self.L = L
        if L == 0:
            return
        for l, (kc, vc) in enumerate(zip(key_caches, value_caches)):   # every layer: one block stride serves the launch
            _check_kv_layout(kc, vc)
            if kc.shape != key_caches[0].shape or kc.dtype != key_caches[0].dtype or kc.stride() != key_caches[0].stride():
                raise ValueError(f"layer {l}: every cache of the call must share shape, dtype and strides")
        _need_cuda(*key_caches, *value_caches)
        self.kvd = _KV_DTYPES[kv_cache_dtype]
        self.cache_dtype = key_caches[0].dtype
        self.block_size = int(key_caches[0].size(1))
        self.block_stride = int(key_caches[0].stride(0))
        VP = ctypes.c_void_p * L
        self._keep = (list(key_caches), list(value_caches), list(k_scales), list(v_scales))   # the tables hold raw pointers
        self.kc = VP(*[c.data_ptr() for c in key_caches])
        self.vc = VP(*[c.data_ptr() for c in value_caches])
        self.ks = VP(*[s.data_ptr() for s in k_scales])
        self.vs = VP(*[s.data_ptr() for s in v_scales])
        self.num_heads, self.head_size = int(num_heads), int(head_size)

    def __call__(self, keys: torch.Tensor, values: torch.Tensor, slot_mapping: torch.Tensor, stream: Optional[int] = None) -> None:
        if self.L == 0:
            return
        _need_cuda(keys, values, slot_mapping)
        if slot_mapping.dtype != torch.int64:
            raise RuntimeError("slot_mapping must be int64")
        src = N.torch_dtype_code(keys.dtype)
        kvd = self.kvd
        if kvd is None:
            kvd = src
            if self.cache_dtype != keys.dtype:
                raise RuntimeError("kv_cache_dtype 'auto' needs caches of the source dtype")
        N.check(N.lib().aic_reshape_and_cache_flash_bulk(
            keys.data_ptr(), values.data_ptr(), self.kc, self.vc, slot_mapping.data_ptr(), slot_mapping.size(0), self.L,
            self.num_heads, self.head_size, self.block_size, self.block_stride, int(keys.stride(0)),
            int(values.stride(0)), src, kvd, self.ks, self.vs, N.current_stream_ptr() if stream is None else stream))


def reshape_and_cache_flash_bulk(keys: torch.Tensor, values: torch.Tensor, key_caches: List[torch.Tensor],
                                 value_caches: List[torch.Tensor], slot_mapping: torch.Tensor, kv_cache_dtype: str,
                                 k_scales: List[torch.Tensor], v_scales: List[torch.Tensor], num_heads: int,
                                 head_size: int) -> None:
    if len(key_caches) == 0:
        return
    KvBulkWriter(key_caches, value_caches, kv_cache_dtype, k_scales, v_scales, num_heads, head_size)(keys, values, slot_mapping)


# ------------------------------------------------------------------------------------------------
# A6 rejection acceptance
# ------------------------------------------------------------------------------------------------
class RejectionResult:
    __slots__ = ("output_token_ids", "num_accepted", "last_token", "hidden_index")

    def __init__(self, output_token_ids, num_accepted, last_token, hidden_index):
        self.output_token_ids = output_token_ids
        self.num_accepted = num_accepted
        self.last_token = last_token
        self.hidden_index = hidden_index


_ws_cache = {}
_ws_retired = []     # outgrown workspaces stay alive: a kernel on a caller-supplied stream may still be reading one


def _workspace(nbytes: int, device, stream: Optional[int] = None, purpose: str = "attn") -> torch.Tensor:
    """Scratch memory of one (device, stream, purpose): calls enqueued on different streams never share partials, and
    attention (per-layer, possibly on a side stream) never shares with the acceptance kernel.  Sizes only grow (by
    doubling), so the retired list stays a handful of blocks."""
    if stream is None:
        stream = N.current_stream_ptr()
    key = (device.index, int(stream or 0), purpose)
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < nbytes:
        if ws is not None:
            _ws_retired.append(ws)
        ws = torch.empty(max(nbytes, 1 << 20, 0 if ws is None else 2 * ws.numel()), dtype=torch.uint8, device=device)
        _ws_cache[key] = ws
    return ws


def rejection_sample(target_logits: torch.Tensor, draft_token_ids: torch.Tensor, cu_num_draft_tokens: torch.Tensor,
                     bonus_token_ids: torch.Tensor, max_spec_len: int, temperature: Optional[torch.Tensor] = None,
                     uniform_probs: Optional[torch.Tensor] = None, exp_noise: Optional[torch.Tensor] = None,
                     target_row_index: Optional[torch.Tensor] = None,
                     bonus_row_index: Optional[torch.Tensor] = None, *, top_k: Optional[torch.Tensor] = None,
                     top_p: Optional[torch.Tensor] = None) -> RejectionResult:
    """out[B, max_spec_len+1] int32 (-1 padded) as vLLM's RejectionSampler returns it for
    draft_probs=None (call site model_runner.py:405-411), plus the proposer inputs of the next step.
    `target_row_index` (int64 [num_draft_total]): pass the model's full [T, V] logits as `target_logits` and the
    rows to read (SpecDecodeMetadata.target_logits_indices) instead of a gathered copy.  `bonus_row_index` (int64 [B],
    greedy only): the bonus tokens are the arg-max of those rows of `target_logits`, computed in the same launch
    (`bonus_token_ids` may then be None).
    `top_k` (int [B]) / `top_p` (float [B]), with `temperature` only: the random rows' probabilities are vLLM's
    compute_probs after apply_top_k_top_p (aic_rejection_random_topk_topp: k <= 0 or k >= vocab, p >= 1 disable a
    filter for that request)."""
    if (top_k is not None or top_p is not None) and temperature is None:
        raise ValueError("top_k / top_p apply to random rows: they need temperature")
    _need_cuda(target_logits, draft_token_ids, cu_num_draft_tokens, bonus_token_ids, target_row_index, bonus_row_index,
               top_k, top_p)
    if bonus_row_index is not None and (temperature is not None or bonus_row_index.dtype != torch.int64 or
                                        bonus_row_index.numel() != cu_num_draft_tokens.numel()):
        raise ValueError("bonus_row_index: int64, one row per request, greedy acceptance only")
    if bonus_token_ids is None and bonus_row_index is None:
        raise ValueError("bonus_token_ids or bonus_row_index is required")
    if target_row_index is not None and (target_row_index.dtype != torch.int64 or
                                         target_row_index.numel() != draft_token_ids.numel()):
        raise ValueError("target_row_index must be int64 with one entry per draft token")
    B = cu_num_draft_tokens.numel()
    rows = draft_token_ids.numel()
    V = target_logits.size(-1) if (rows or bonus_row_index is not None) else 1
    dev = cu_num_draft_tokens.device
    out = torch.empty((B, max_spec_len + 1), dtype=torch.int32, device=dev)
    nacc = torch.empty(B, dtype=torch.int32, device=dev)
    last = torch.empty(B, dtype=torch.int32, device=dev)
    hidx = torch.empty(B, dtype=torch.int32, device=dev)
    ws = _workspace(N.lib().aic_rejection_workspace_bytes(rows + (B if bonus_row_index is not None else 0), V), dev,
                    purpose="accept")
    draft = draft_token_ids.to(torch.int32)
    cu = cu_num_draft_tokens.to(torch.int32)
    bonus = None if bonus_token_ids is None else bonus_token_ids.reshape(-1).to(torch.int32)
    has_logits = rows > 0 or bonus_row_index is not None
    dt = N.torch_dtype_code(target_logits.dtype) if has_logits else N.DT_F32
    stride = target_logits.stride(0) if has_logits else 0
    if temperature is None:
        N.check(N.lib().aic_rejection_greedy(_ptr(target_logits) if has_logits else None, dt, stride, V, draft.data_ptr(),
                                             cu.data_ptr(), _ptr(bonus), B, rows, max_spec_len, out.data_ptr(),
                                             nacc.data_ptr(), last.data_ptr(), hidx.data_ptr(), _ptr(target_row_index),
                                             _ptr(bonus_row_index), ws.data_ptr(), N.current_stream_ptr()))
    elif top_k is not None or top_p is not None:
        tk = None if top_k is None else top_k.reshape(-1).to(torch.int32)
        tp = None if top_p is None else top_p.reshape(-1).float()
        if (tk is not None and tk.numel() != B) or (tp is not None and tp.numel() != B):
            raise ValueError("top_k / top_p: one value per request")
        ws = _workspace(N.lib().aic_rejection_topk_topp_workspace_bytes(rows, V, dt), dev, purpose="accept")
        N.check(N.lib().aic_rejection_random_topk_topp(
            _ptr(target_logits) if rows else None, dt, stride, V, draft.data_ptr(), cu.data_ptr(), bonus.data_ptr(),
            temperature.float().data_ptr(), uniform_probs.double().data_ptr(), exp_noise.float().data_ptr(), _ptr(tk),
            _ptr(tp), B, rows, max_spec_len, out.data_ptr(), nacc.data_ptr(), last.data_ptr(), hidx.data_ptr(),
            _ptr(target_row_index), ws.data_ptr(), N.current_stream_ptr()))
    else:
        N.check(N.lib().aic_rejection_random(_ptr(target_logits) if rows else None, dt, stride, V, draft.data_ptr(),
                                             cu.data_ptr(), bonus.data_ptr(), temperature.float().data_ptr(),
                                             uniform_probs.double().data_ptr(), exp_noise.float().data_ptr(), B, rows,
                                             max_spec_len, out.data_ptr(), nacc.data_ptr(), last.data_ptr(),
                                             hidx.data_ptr(), _ptr(target_row_index), ws.data_ptr(),
                                             N.current_stream_ptr()))
    return RejectionResult(out, nacc, last, hidx)


def sample_tokens(logits: torch.Tensor, temperature: torch.Tensor, exp_noise: Optional[torch.Tensor], *,
                  top_k: Optional[torch.Tensor] = None, top_p: Optional[torch.Tensor] = None,
                  row_index: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int32 [rows]: one token per row as vLLM's Sampler draws it for temperature / top-k / top-p
    (aic_sample_topk_topp): arg-max of the raw row where temperature <= 0, else argmax(p / exp_noise) with p the f32
    softmax of f32(logits) / temperature over the kept set (k <= 0 or k >= vocab, p >= 1 disable a filter for that row).
    `logits` [T, V] is read in place in its own dtype; `row_index` (int64 [rows]) names the rows to sample
    (SpecDecodeMetadata.bonus_logits_indices) instead of a gathered copy, else every row is sampled.  `temperature`,
    `top_k`, `top_p`: one value per row; `exp_noise` f32 [rows, V] (draw_sampler_noise), or None for an all-greedy
    batch: every row is then the arg-max of its raw logits whatever its temperature."""
    if logits.dim() != 2 or logits.stride(1) != 1:
        raise ValueError("logits must be [T, V] with contiguous rows")
    if row_index is not None and (row_index.dtype != torch.int64 or row_index.dim() != 1):
        raise ValueError("row_index must be int64 [rows]")
    rows = int(row_index.numel()) if row_index is not None else int(logits.size(0))
    V = int(logits.size(1))
    temp = temperature.reshape(-1).float()
    tk = None if top_k is None else top_k.reshape(-1).to(torch.int32)
    tp = None if top_p is None else top_p.reshape(-1).float()
    if temp.numel() != rows or (tk is not None and tk.numel() != rows) or (tp is not None and tp.numel() != rows):
        raise ValueError("temperature / top_k / top_p: one value per row")
    if exp_noise is not None and (exp_noise.dtype != torch.float32 or tuple(exp_noise.shape) != (rows, V) or
                                  not exp_noise.is_contiguous()):
        raise ValueError("exp_noise must be contiguous float32 [rows, V]")
    _need_cuda(logits, temperature, exp_noise, top_k, top_p, row_index)
    dev = logits.device
    out = torch.empty(rows, dtype=torch.int32, device=dev)
    if rows == 0:
        return out
    dt = N.torch_dtype_code(logits.dtype)
    ws = _workspace(N.lib().aic_sample_workspace_bytes(rows, V, dt), dev, purpose="accept")
    N.check(N.lib().aic_sample_topk_topp(logits.data_ptr(), dt, int(logits.stride(0)), V, _ptr(row_index), temp.data_ptr(),
                                         _ptr(exp_noise), _ptr(tk), _ptr(tp), rows, out.data_ptr(), ws.data_ptr(),
                                         N.current_stream_ptr()))
    return out


def token_logprobs(logits: torch.Tensor, num_logprobs: int, *, token_ids: Optional[torch.Tensor] = None,
                   row_index: Optional[torch.Tensor] = None, check_token_ids: bool = True
                   ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(token ids int32 [rows, 1+n], logprobs f32 [rows, 1+n], ranks int64 [rows]) as vLLM's Sampler.compute_logprobs +
    gather_logprobs give them (aic_token_logprobs): column 0 is the selected token, columns 1..n the n = `num_logprobs`
    largest entries of the row by (value descending, index ascending); logprobs are the f32 log-softmax of the raw row,
    the rank counts the raw values >= the selected token's.  `logits` [T, V] is read in place in its own dtype;
    `row_index` (int64 [rows]) names the rows (SpecDecodeMetadata.bonus_logits_indices) instead of a gathered copy, else
    every row is served.  `token_ids` (int [rows]): the selected tokens; None: each row's arg-max (ties to the lowest
    index).  Ids outside [0, V) raise; reading them back costs a host synchronisation, so the check is skipped while the
    stream is being captured and with `check_token_ids=False` (a caller whose ids come from ops.sample_tokens): the
    kernel then answers such a row with a NaN logprob and rank 0 and never indexes out of the row."""
    if logits.dim() != 2 or logits.stride(1) != 1:
        raise ValueError("logits must be [T, V] with contiguous rows")
    if row_index is not None and (row_index.dtype != torch.int64 or row_index.dim() != 1):
        raise ValueError("row_index must be int64 [rows]")
    rows = int(row_index.numel()) if row_index is not None else int(logits.size(0))
    V = int(logits.size(1))
    n = int(num_logprobs)
    cap = int(N.lib().aic_logprobs_max())
    if not 0 <= n <= cap or n > V:
        raise ValueError(f"num_logprobs must be in 0 .. {min(cap, V)} (got {n})")
    tok = None if token_ids is None else token_ids.reshape(-1).to(torch.int32)
    if tok is not None and tok.numel() != rows:
        raise ValueError("token_ids: one token per row")
    _need_cuda(logits, token_ids, row_index)
    dev = logits.device
    out_ids = torch.empty((rows, 1 + n), dtype=torch.int32, device=dev)
    out_lp = torch.empty((rows, 1 + n), dtype=torch.float32, device=dev)
    out_rank = torch.empty(rows, dtype=torch.int64, device=dev)
    if rows == 0:
        return out_ids, out_lp, out_rank
    if tok is not None and check_token_ids and not torch.cuda.is_current_stream_capturing():
        if bool(((tok < 0) | (tok >= V)).any()):
            raise ValueError(f"token_ids outside [0, {V})")
    dt = N.torch_dtype_code(logits.dtype)
    ws = _workspace(N.lib().aic_logprobs_workspace_bytes(rows, V, dt, n), dev, purpose="accept")
    N.check(N.lib().aic_token_logprobs(logits.data_ptr(), dt, int(logits.stride(0)), V, _ptr(row_index), _ptr(tok), rows, n,
                                       out_ids.data_ptr(), out_lp.data_ptr(), out_rank.data_ptr(), ws.data_ptr(),
                                       N.current_stream_ptr()))
    return out_ids, out_lp, out_rank


def _csr(name: str, lists, rows: int, n_parts: int):
    """Checks one CSR edit input of edit_logits: (offsets int32 [rows + 1], tokens int32 [n][, values f32 [n]])."""
    if lists is None:
        return (None,) * n_parts + (0,)
    if len(lists) != n_parts:
        raise ValueError(f"{name}: {n_parts} tensors (offsets, tokens{', values' if n_parts == 3 else ''})")
    off, tok = lists[0], lists[1]
    if off.dtype != torch.int32 or off.dim() != 1 or off.numel() != rows + 1 or not off.is_contiguous():
        raise ValueError(f"{name}: offsets must be contiguous int32 [rows + 1]")
    if tok.dtype != torch.int32 or tok.dim() != 1 or not tok.is_contiguous():
        raise ValueError(f"{name}: tokens must be contiguous int32 [n]")
    if n_parts == 3:
        val = lists[2]
        if val.dtype != torch.float32 or val.dim() != 1 or val.numel() != tok.numel() or not val.is_contiguous():
            raise ValueError(f"{name}: values must be contiguous float32, one per token")
    _need_cuda(*lists)
    return tuple(lists) + (int(tok.numel()),)


def logits_edit_segment() -> int:
    """The tokens one workgroup of aic_logits_edit serves (tests place histories on both sides of a boundary)."""
    return int(N.lib().aic_logits_edit_segment())


def edit_logits(logits: torch.Tensor, *, allowed_mask: Optional[torch.Tensor] = None, ban=None, bias=None, prompt=None,
                output=None, repetition: Optional[torch.Tensor] = None, frequency: Optional[torch.Tensor] = None,
                presence: Optional[torch.Tensor] = None, min_p: Optional[torch.Tensor] = None,
                temperature: Optional[torch.Tensor] = None, row_index: Optional[torch.Tensor] = None) -> torch.Tensor:
    """f32 [rows, V]: the rows of `logits` as vLLM's Sampler leaves them before it samples (aic_logits_edit): allowed
    mask, bans, bias, repetition / frequency / presence penalties, then min-p on the rows with temperature > 0 and
    min_p > 0.  `logits` [T, V] (bf16 / fp16 / f32) is only read, in place; `row_index` (int64 [rows]) names the rows
    (SpecDecodeMetadata.bonus_logits_indices), else every row is edited.  Every edit input may be None:
    `allowed_mask` bool / uint8 [rows, V], non-zero = not allowed; `ban` = (offsets, tokens), `bias` = (offsets, tokens,
    values), `prompt` / `output` = (offsets, tokens): int32 CSR, offsets [rows + 1], values f32; token ids outside
    [0, V) are ignored; `repetition` / `frequency` / `presence` / `min_p` / `temperature` f32 [rows].  Wrong dtypes or
    shapes, and min_p without temperature, raise before anything is launched."""
    if logits.dim() != 2 or logits.stride(1) != 1:
        raise ValueError("logits must be [T, V] with contiguous rows")
    if logits.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise ValueError(f"logits must be bf16, fp16 or f32 (got {logits.dtype})")
    if row_index is not None and (row_index.dtype != torch.int64 or row_index.dim() != 1):
        raise ValueError("row_index must be int64 [rows]")
    rows = int(row_index.numel()) if row_index is not None else int(logits.size(0))
    V = int(logits.size(1))
    if allowed_mask is not None and (allowed_mask.dtype not in (torch.bool, torch.uint8) or
                                     tuple(allowed_mask.shape) != (rows, V) or not allowed_mask.is_contiguous()):
        raise ValueError("allowed_mask must be contiguous bool / uint8 [rows, V]")
    for name, t in (("repetition", repetition), ("frequency", frequency), ("presence", presence), ("min_p", min_p),
                    ("temperature", temperature)):
        if t is not None and (t.dtype != torch.float32 or t.dim() != 1 or t.numel() != rows or not t.is_contiguous()):
            raise ValueError(f"{name} must be contiguous float32 [rows]")
    if min_p is not None and temperature is None:
        raise ValueError("min_p needs the rows' temperature")
    ban_off, ban_tok, n_ban = _csr("ban", ban, rows, 2)
    bias_off, bias_tok, bias_val, n_bias = _csr("bias", bias, rows, 3)
    pr_off, pr_tok, n_pr = _csr("prompt", prompt, rows, 2)
    ou_off, ou_tok, n_ou = _csr("output", output, rows, 2)
    _need_cuda(logits, allowed_mask, repetition, frequency, presence, min_p, temperature, row_index)
    dev = logits.device
    out = torch.empty((rows, V), dtype=torch.float32, device=dev)
    if rows == 0:
        return out
    ws = None
    if min_p is not None:
        ws = _workspace(N.lib().aic_logits_edit_workspace_bytes(rows, V), dev, purpose="accept")
    N.check(N.lib().aic_logits_edit(
        logits.data_ptr(), N.torch_dtype_code(logits.dtype), int(logits.stride(0)), V, _ptr(row_index), rows,
        _ptr(allowed_mask), _ptr(ban_off), _ptr(ban_tok), n_ban, _ptr(bias_off), _ptr(bias_tok), _ptr(bias_val), n_bias,
        _ptr(pr_off), _ptr(pr_tok), n_pr, _ptr(ou_off), _ptr(ou_tok), n_ou, _ptr(repetition), _ptr(frequency),
        _ptr(presence), _ptr(min_p), _ptr(temperature), out.data_ptr(), _ptr(ws), N.current_stream_ptr()))
    return out


# ------------------------------------------------------------------------------------------------
# A5 verify attention
# ------------------------------------------------------------------------------------------------
_ATTN_Q_DTYPES = {torch.bfloat16: N.DT_BF16, torch.float16: N.DT_F16}


def _attn_dtypes(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, out: Optional[torch.Tensor]):
    """(q_dtype, kv_dtype) codes of an attention call, after the dtype rules of aic_verify_attention_dt: q is bf16 or
    fp16, out has q's dtype, a 16-bit cache has q's dtype (else float8_e4m3fn).  ValueError before anything is launched."""
    qd = _ATTN_Q_DTYPES.get(q.dtype)
    if qd is None:
        raise ValueError(f"attention serves bfloat16 and float16 queries, not {q.dtype}")
    if out is not None and out.dtype != q.dtype:
        raise ValueError(f"out must have the query's dtype ({q.dtype}), not {out.dtype}")
    if k_cache.dtype != v_cache.dtype:
        raise ValueError(f"key and value caches must share a dtype ({k_cache.dtype} / {v_cache.dtype})")
    if k_cache.dtype in _ATTN_Q_DTYPES and k_cache.dtype != q.dtype:
        raise ValueError(f"a 16-bit kv cache must have the query's dtype ({q.dtype}), not {k_cache.dtype}")
    return qd, N.torch_dtype_code(k_cache.dtype)


def _check_shared_prefix(shared_prefix_len: int, table: Optional[torch.Tensor], q: torch.Tensor, block_size: int,
                         sliding_window: int, q_lens_host, seq_lens_host, seq_lens: torch.Tensor, max_seq_len: int) -> None:
    """The argument rules of aic_verify_attention_prefix that can be told on the host.  ValueError before anything is
    launched (and before the device check: none of this needs a GPU)."""
    if shared_prefix_len < 0:
        raise ValueError(f"shared_prefix_len must be >= 0, not {shared_prefix_len}")
    if sliding_window > 0:
        raise ValueError("a shared prefix is not served on a layer with a sliding window")
    need = -(-shared_prefix_len // block_size)
    if table is None:
        raise ValueError("a shared prefix needs prefix_block_table (the pages of its tokens)")
    if table.dtype != torch.int32 or table.dim() != 1 or not table.is_contiguous():
        raise ValueError(f"prefix_block_table: contiguous int32 [n], not {table.dtype} {tuple(table.shape)}")
    if table.numel() < need:
        raise ValueError(f"prefix_block_table has {table.numel()} pages, {shared_prefix_len} tokens in pages of "
                         f"{block_size} need {need}")
    if table.device != q.device:
        raise ValueError(f"prefix_block_table is on {table.device}, the call on {q.device}")
    if max_seq_len <= shared_prefix_len:
        raise ValueError(f"max_seq_len {max_seq_len} leaves no query token behind a shared prefix of {shared_prefix_len}")
    if seq_lens_host is None and q_lens_host is not None and not seq_lens.is_cuda:
        seq_lens_host = seq_lens.tolist()
    if q_lens_host is not None and seq_lens_host is not None:
        for i, (s, ql) in enumerate(zip(seq_lens_host, q_lens_host)):
            if int(s) - int(ql) < shared_prefix_len:
                raise ValueError(f"request {i}: seq_len {int(s)} - q_len {int(ql)} < shared_prefix_len {shared_prefix_len} "
                                 "(every query token must lie behind the shared prefix)")


def prefix_max_groups() -> int:
    """How many groups one aic_verify_attention_prefix_groups call takes."""
    return int(N.lib().aic_prefix_max_groups())


class PrefixGroups:
    """The groups of a step for verify_attention(..., prefix_groups=): requests that begin with the same tokens held in
    the same pages, a prefix per group, beside requests that share nothing (aic_verify_attention_prefix_groups).
    `req_group[i]` is request i's group index, or -1; `group_prefix_len[g]` the tokens group g's members share (served
    rounded down to a multiple of 32); `q_lens_host` the per-request query lengths.  The leader of a group — the request
    whose block-table row names the group's pages — is its first member.  The five arrays of the call are laid out in one
    host buffer (pinned when `device` is a GPU) and the two the kernels read go up in one copy; build it once per step and
    hand it to every layer's call.  ValueError, before anything touches a device: more groups than
    prefix_max_groups(), a group index out of range, a group without members, a negative length, no `q_lens_host`."""

    def __init__(self, req_group: Sequence[int], group_prefix_len: Sequence[int], q_lens_host: Sequence[int], device):
        import numpy as np
        if q_lens_host is None:
            raise ValueError("PrefixGroups needs q_lens_host (the per-request query lengths)")
        rg = np.asarray(req_group, dtype=np.int64).reshape(-1)
        gl = np.asarray(group_prefix_len, dtype=np.int64).reshape(-1)
        ql = np.asarray(q_lens_host, dtype=np.int64).reshape(-1)
        n, B = int(gl.size), int(rg.size)
        if ql.size != B:
            raise ValueError(f"req_group names {B} requests, q_lens_host {ql.size}")
        if n > prefix_max_groups():
            raise ValueError(f"{n} prefix groups: one call takes at most {prefix_max_groups()}")
        if B and (int(rg.min()) < -1 or int(rg.max()) >= n):
            bad = int(np.flatnonzero((rg < -1) | (rg >= n))[0])
            raise ValueError(f"request {bad}: group index {int(rg[bad])} out of range (-1, or 0 .. {n - 1})")
        if n and int(gl.min()) < 0:
            raise ValueError("group_prefix_len must be >= 0")
        members = np.bincount(rg[rg >= 0], minlength=n) if n else np.zeros(0, dtype=np.int64)
        if n and int(members.min()) == 0:
            raise ValueError(f"prefix group {int(np.argmin(members))} has no members")
        qsl = np.concatenate([[0], np.cumsum(ql)])
        tok_req = np.repeat(np.arange(B), ql)                       # request of every token row
        tok_grp = rg[tok_req] if B else np.zeros(0, dtype=np.int64)
        grouped = np.flatnonzero(tok_grp >= 0)
        token_index = grouped[np.argsort(tok_grp[grouped], kind="stable")]
        start = np.concatenate([[0], np.cumsum(np.bincount(tok_grp[grouped], minlength=n))]) if n else np.zeros(1)
        leader = np.array([int(np.flatnonzero(rg == g)[0]) for g in range(n)], dtype=np.int64)
        req_len = np.where(rg >= 0, gl[np.maximum(rg, 0)] if n else 0, 0)
        device = torch.device(device)
        parts = [gl, leader, start, token_index, req_len]
        sizes = [int(np.size(x)) for x in parts]
        host = torch.empty(sum(sizes), dtype=torch.int32, pin_memory=device.type == "cuda")
        hv = host.numpy()
        offs = np.concatenate([[0], np.cumsum(sizes)])
        for x, o in zip(parts, offs):
            hv[o:o + np.size(x)] = x
        self._host = host                                           # keeps the three host arrays alive
        self.group_prefix_len, self.group_leader, self.group_token_start = (hv[offs[i]:offs[i + 1]] for i in range(3))
        dev = host[int(offs[3]):].to(device, non_blocking=True)     # the one copy of the step
        self.group_token_index, self.req_prefix_len = dev[:sizes[3]], dev[sizes[3]:]
        self.n_groups, self.batch, self.num_tokens = n, B, int(qsl[-1])
        self.req_group, self.q_lens = rg, ql
        self.max_prefix_len = int(gl.max()) if n else 0

    def check_call(self, batch: int, num_tokens: int, sliding_window: int, max_seq_len: int, seq_lens_host) -> None:
        """The argument rules of the grouped call that can be told on the host (ValueError, before the device check)."""
        if sliding_window > 0:
            raise ValueError("prefix groups are not served on a layer with a sliding window")
        if batch != self.batch or num_tokens != self.num_tokens:
            raise ValueError(f"prefix_groups describes {self.batch} requests / {self.num_tokens} tokens, the call has "
                             f"{batch} / {num_tokens}")
        if self.n_groups and max_seq_len <= (self.max_prefix_len & ~31):
            raise ValueError(f"max_seq_len {max_seq_len} leaves no query token behind a group prefix of "
                             f"{self.max_prefix_len}")
        if seq_lens_host is not None:
            for i, (s_, ql, g) in enumerate(zip(seq_lens_host, self.q_lens, self.req_group)):
                if g >= 0 and int(s_) - int(ql) < int(self.group_prefix_len[g]):
                    raise ValueError(f"request {i}: seq_len {int(s_)} - q_len {int(ql)} < its group's prefix length "
                                     f"{int(self.group_prefix_len[g])} (every query token must lie behind the prefix)")


def verify_attention(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, block_table: torch.Tensor,
                     seq_lens: torch.Tensor, query_start_loc: torch.Tensor, max_q_len: int, max_seq_len: int,
                     sm_scale: float, out: Optional[torch.Tensor] = None, num_splits_max: int = 64,
                     q_lens_host: Optional[Sequence[int]] = None, req_split=None,
                     k_scale: Optional[torch.Tensor] = None, v_scale: Optional[torch.Tensor] = None,
                     stream: Optional[int] = None, sliding_window: int = 0,
                     sinks: Optional[torch.Tensor] = None, shared_prefix_len: int = 0,
                     prefix_block_table: Optional[torch.Tensor] = None,
                     seq_lens_host: Optional[Sequence[int]] = None,
                     prefix_groups: Optional[PrefixGroups] = None) -> torch.Tensor:
    """q [T, Hq, D] in bf16 or fp16 (token stride may exceed Hq*D: a view into an all-to-all receive buffer works),
    caches [num_blocks, block_size, Hkv, D] in q's dtype, or float8_e4m3fn with per-tensor `k_scale` / `v_scale`
    (device scalars, the scales A16 divided by); returns [T, Hq, D] in q's dtype (aic_verify_attention_dt).  `q_lens_host` (the per-request query
    lengths, which vLLM has on the host) lets long drafts take the shared-tile kernel.  `stream`: raw HIP stream
    handle (default: torch's current stream; a caller that issues one call per layer looks it up once).
    `sliding_window` W > 0 / `sinks` f32 [Hq]: the per-layer features of gpt-oss-class models.
    `shared_prefix_len` P > 0 with `prefix_block_table` (int32 [>= ceil(P / block_size)], contiguous, on q's device: the
    pages of tokens 0 .. P - 1, e.g. `block_table[0]`): every request of the call begins with the same P tokens in the
    same pages (prefix caching), and those keys are read once for the call (aic_verify_attention_prefix: cascade
    attention) instead of once per request.  PRECONDITION: seq_len - q_len >= P for every request; checked here when the
    lengths are on the host (`q_lens_host` together with `seq_lens_host`, or with a `seq_lens` that is a CPU tensor),
    otherwise the caller's to keep.  Not with a sliding window.  0 (the default) is the call as it always was.
    `prefix_groups` (a PrefixGroups of the step): groups of requests with a shared prefix each, beside requests that share
    nothing (aic_verify_attention_prefix_groups); the same precondition per group (a member's block-table columns below
    its group's length are its leader's), checked here when `seq_lens_host` or a CPU `seq_lens` is given.  Not together
    with `shared_prefix_len`, not with a sliding window.  None (the default) makes exactly the calls made without it."""
    qd, kvd = _attn_dtypes(q, k_cache, v_cache, out)
    _check_kv_layout(k_cache, v_cache)
    shared_prefix_len = int(shared_prefix_len or 0)
    if prefix_groups is not None:
        if shared_prefix_len:
            raise ValueError("prefix_groups and shared_prefix_len are two forms of the call: give one")
        host = seq_lens_host
        if host is None and not seq_lens.is_cuda:
            host = seq_lens.tolist()
        prefix_groups.check_call(int(seq_lens.numel()), int(q.shape[0]), int(sliding_window or 0), int(max_seq_len), host)
    if shared_prefix_len:
        _check_shared_prefix(shared_prefix_len, prefix_block_table, q, int(k_cache.shape[1]), int(sliding_window or 0),
                             q_lens_host, seq_lens_host, seq_lens, int(max_seq_len))
    _need_cuda(q, k_cache, v_cache, block_table, seq_lens, query_start_loc, sinks)
    if sinks is not None and (sinks.dtype != torch.float32 or sinks.numel() != q.shape[1] or not sinks.is_contiguous()):
        raise ValueError("sinks: contiguous float32, one value per query head")
    T, Hq, D = q.shape
    nb, bs, Hkv, D2 = k_cache.shape
    assert D == D2 and q.stride(2) == 1 and q.stride(1) == D
    if out is None:
        out = torch.empty((T, Hq, D), dtype=q.dtype, device=q.device)
    B = seq_lens.numel()
    wsb = N.lib().aic_verify_attention_workspace_bytes(T, Hq, D, num_splits_max)
    ws = _workspace(wsb, q.device, stream)
    if req_split is None and q_lens_host is not None:
        req_split = split_requests(q_lens_host, Hq // Hkv, q.device)
    short, n_short, long_, n_long = req_split if req_split is not None else (None, 0, None, 0)
    if prefix_groups is not None:
        g = prefix_groups
        _need_cuda(g.group_token_index, g.req_prefix_len)
        N.check(N.lib().aic_verify_attention_prefix_groups(
            q.data_ptr(), q.stride(0), k_cache.data_ptr(), v_cache.data_ptr(), k_cache.stride(0), kvd, _ptr(k_scale),
            _ptr(v_scale), block_table.data_ptr(), block_table.size(1), seq_lens.data_ptr(), query_start_loc.data_ptr(), B,
            T, int(max_q_len), Hq, Hkv, D, bs, float(sm_scale), out.data_ptr(), out.stride(0), ws.data_ptr(), ws.numel(),
            int(max_seq_len), _ptr(short) if n_short else None, n_short, _ptr(long_) if n_long else None, n_long, 0,
            _ptr(sinks), qd, g.n_groups, g.group_prefix_len.ctypes.data, g.group_leader.ctypes.data,
            g.group_token_start.ctypes.data, g.group_token_index.data_ptr(), g.req_prefix_len.data_ptr(),
            N.current_stream_ptr() if stream is None else stream))
        return out
    if shared_prefix_len:
        _need_cuda(prefix_block_table)
        N.check(N.lib().aic_verify_attention_prefix(
            q.data_ptr(), q.stride(0), k_cache.data_ptr(), v_cache.data_ptr(), k_cache.stride(0), kvd, _ptr(k_scale),
            _ptr(v_scale), block_table.data_ptr(), block_table.size(1), seq_lens.data_ptr(), query_start_loc.data_ptr(), B,
            T, int(max_q_len), Hq, Hkv, D, bs, float(sm_scale), out.data_ptr(), out.stride(0), ws.data_ptr(), ws.numel(),
            int(max_seq_len), _ptr(short) if n_short else None, n_short, _ptr(long_) if n_long else None, n_long, 0,
            _ptr(sinks), qd, shared_prefix_len, prefix_block_table.data_ptr(),
            N.current_stream_ptr() if stream is None else stream))
        return out
    N.check(N.lib().aic_verify_attention_dt(
        q.data_ptr(), q.stride(0), k_cache.data_ptr(), v_cache.data_ptr(), k_cache.stride(0), kvd, _ptr(k_scale),
        _ptr(v_scale), block_table.data_ptr(), block_table.size(1), seq_lens.data_ptr(), query_start_loc.data_ptr(), B, T,
        int(max_q_len), Hq, Hkv, D, bs, float(sm_scale), out.data_ptr(), out.stride(0), ws.data_ptr(), ws.numel(),
        int(max_seq_len), _ptr(short) if n_short else None, n_short, _ptr(long_) if n_long else None, n_long,
        int(sliding_window or 0), _ptr(sinks), qd, N.current_stream_ptr() if stream is None else stream))
    return out


class VerifyAttentionPlan:
    """verify_attention for a caller that issues one call per layer with only the cache pointers changing (every layer
    of a step shares the batch geometry): argument checks, workspace sizing and the ctypes argument list are built once
    per step, `run(k_cache, v_cache)` is one foreign call.  Same semantics as verify_attention(), for bf16 only (the
    stand-alone engine's dtype: aic_verify_attention_ex / aic_verify_attention_layers carry no query dtype)."""

    def __init__(self, q: torch.Tensor, out: torch.Tensor, kv_like: torch.Tensor, block_table: torch.Tensor,
                 seq_lens: torch.Tensor, query_start_loc: torch.Tensor, max_q_len: int, max_seq_len: int, sm_scale: float,
                 req_split=None, k_scale: Optional[torch.Tensor] = None, v_scale: Optional[torch.Tensor] = None,
                 num_splits_max: int = 64, stream: Optional[int] = None):
        if q.dtype != torch.bfloat16 or out.dtype != torch.bfloat16 or kv_like.dtype == torch.float16:
            raise ValueError("VerifyAttentionPlan serves bfloat16 queries and outputs with a bfloat16 or fp8 cache "
                             f"(got q {q.dtype}, out {out.dtype}, cache {kv_like.dtype}); fp16 models call verify_attention()")
        _check_kv_layout(kv_like, kv_like)
        _need_cuda(q, out, kv_like, block_table, seq_lens, query_start_loc)
        T, Hq, D = q.shape
        nb, bs, Hkv, D2 = kv_like.shape
        assert D == D2 and q.stride(2) == 1 and q.stride(1) == D and out.shape == q.shape
        ws = _workspace(N.lib().aic_verify_attention_workspace_bytes(T, Hq, D, num_splits_max), q.device, stream)
        short, n_short, long_, n_long = req_split if req_split is not None else (None, 0, None, 0)
        self._keep = (q, out, block_table, seq_lens, query_start_loc, ws, short, long_, k_scale, v_scale)
        self._fn = N.lib().aic_verify_attention_ex
        self._args = [q.data_ptr(), q.stride(0), 0, 0, kv_like.stride(0), N.torch_dtype_code(kv_like.dtype), _ptr(k_scale),
                      _ptr(v_scale), block_table.data_ptr(), block_table.size(1), seq_lens.data_ptr(),
                      query_start_loc.data_ptr(), seq_lens.numel(), T, int(max_q_len), Hq, Hkv, D, bs, float(sm_scale),
                      out.data_ptr(), out.stride(0), ws.data_ptr(), ws.numel(), int(max_seq_len),
                      _ptr(short) if n_short else None, n_short, _ptr(long_) if n_long else None, n_long,
                      N.current_stream_ptr() if stream is None else stream]
        self._kv_shape, self._kv_dtype, self._kv_stride = tuple(kv_like.shape), kv_like.dtype, tuple(kv_like.stride())

    def _check_cache(self, c: torch.Tensor) -> None:
        if tuple(c.shape) != self._kv_shape or c.dtype is not self._kv_dtype or tuple(c.stride()) != self._kv_stride:
            raise ValueError("the plan was made for caches of another shape / dtype / strides")

    def layer_tables(self, k_caches: Sequence[torch.Tensor], v_caches: Sequence[torch.Tensor]):
        """Pointer tables for run_layers() (build once for a fixed set of caches)."""
        if len(k_caches) != len(v_caches):
            raise ValueError("k_caches and v_caches must have the same length")
        for c in list(k_caches) + list(v_caches):
            self._check_cache(c)
        VP = ctypes.c_void_p * len(k_caches)
        return (VP(*[c.data_ptr() for c in k_caches]), VP(*[c.data_ptr() for c in v_caches]), len(k_caches),
                (list(k_caches), list(v_caches)))

    def run_layers(self, tables) -> None:
        """Every layer of the step in ONE foreign call (aic_verify_attention_layers): same q / out for all layers, as
        the stand-alone engine has them."""
        a = self._args
        kt, vt, n, _keep = tables
        N.check(N.lib().aic_verify_attention_layers(a[0], a[1], 0, kt, vt, n, *a[4:20], a[20], a[21], 0, *a[22:]))

    def run(self, k_cache: torch.Tensor, v_cache: torch.Tensor) -> None:
        self._check_cache(k_cache)
        self._check_cache(v_cache)
        a = self._args
        a[2] = k_cache.data_ptr()
        a[3] = v_cache.data_ptr()
        N.check(self._fn(*a))


def split_order(q_lens_host: Sequence[int], group_size: int):
    """Host half of split_requests: (request ids with the short ones first, as int32; number of short requests).
    Short = q_len * Hq/Hkv <= 32 query rows.  A batch of short requests only still gets its (identity) list: the
    partitioned call is what lets every workgroup take the one- or two-row-tile form by its own request's rows, where
    the call without lists has to size every request for the longest."""
    import numpy as np
    ql = np.asarray(q_lens_host)
    # same rule as aic_verify_attention_ex
    is_short = ql * group_size <= 32
    n_short = int(is_short.sum())
    if n_short == len(ql):
        return np.arange(len(ql), dtype=np.int32), n_short
    order = np.concatenate([np.nonzero(is_short)[0], np.nonzero(~is_short)[0]]).astype(np.int32)
    return order, n_short


def split_requests(q_lens_host: Sequence[int], group_size: int, device, order_dev: Optional[torch.Tensor] = None):
    """Partition a batch by query length for aic_verify_attention_ex: (short_ids, n_short, long_ids, n_long) with
    device int32 id lists.  Build it once per engine step and pass it to every layer's verify_attention call.
    `order_dev`: the id list already on the device (a caller that stages all of a step's index arrays in one copy
    passes split_order()'s array through that copy)."""
    order, n_short = split_order(q_lens_host, group_size)
    lists = order_dev if order_dev is not None else torch.from_numpy(order).to(device, non_blocking=True)
    return lists[:n_short], n_short, lists[n_short:], len(order) - n_short


# ------------------------------------------------------------------------------------------------
# Tree-shaped drafts: tree-mask attention, greedy acceptance over the tree, KV compaction
# ------------------------------------------------------------------------------------------------
class TreeDrafts:
    """The tree-shaped drafts of a step for verify_attention_tree / rejection_sample_tree / compact_accepted_paths:
    per-request `(token_ids, parents)` in SuffixSpecResult form (tree_drafts.build_tree_layout checks and lays them out),
    uploaded in one copy.  Build it once per step and hand it to every layer's call, like PrefixGroups.  Device tensors:
    `tree_mask` (uint64 words as int64 [T]), `draft_token_ids` / `parents` int32 [T], `query_start_loc` int32 [B + 1];
    `layout` keeps the host arrays (depths, q_lens: the model's rotary positions are tree_drafts.positions(layout, ...))."""

    def __init__(self, trees: Sequence, device, root_tokens: Optional[Sequence[int]] = None):
        import numpy as np

        from . import tree_drafts as TD
        lay = TD.build_tree_layout(trees, root_tokens)
        self.layout = lay
        self.batch, self.num_tokens = int(lay.q_lens.size), int(lay.tokens.size)
        self.max_q_len = int(lay.q_lens.max()) if self.batch else 0
        device = torch.device(device)
        T, B = self.num_tokens, self.batch
        # one buffer, the 8-byte mask words first: [masks as 2 T int32 | tokens T | parents T | query_start_loc B + 1]
        host = torch.empty(4 * T + B + 1, dtype=torch.int32, pin_memory=device.type == "cuda")
        hv = host.numpy()
        hv[:2 * T] = lay.masks.view(np.int32)
        hv[2 * T:3 * T] = lay.tokens
        hv[3 * T:4 * T] = lay.parents
        hv[4 * T:] = lay.query_start_loc
        dev = host.to(device, non_blocking=True)
        self._host, self._dev = host, dev
        self.tree_mask = dev[:2 * T].view(torch.int64)
        self.draft_token_ids, self.parents, self.query_start_loc = dev[2 * T:3 * T], dev[3 * T:4 * T], dev[4 * T:]


def verify_attention_tree(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, block_table: torch.Tensor,
                          seq_lens: torch.Tensor, tree: TreeDrafts, max_seq_len: int, sm_scale: float,
                          out: Optional[torch.Tensor] = None, num_splits_max: int = 64,
                          k_scale: Optional[torch.Tensor] = None, v_scale: Optional[torch.Tensor] = None,
                          stream: Optional[int] = None, sinks: Optional[torch.Tensor] = None, sliding_window: int = 0,
                          shared_prefix_len: int = 0) -> torch.Tensor:
    """verify_attention for tree-shaped drafts (aic_verify_attention_tree): query token t of a request sees every key
    below base = seq_len - q_len and the keys base + u of its ancestors-or-self u (`tree.tree_mask`).  Tensors, dtypes and
    conventions as verify_attention; `seq_lens` counts the step's query tokens, whose K/V are already written at
    base + t by the ordinary slot mapping.  `sliding_window` / `shared_prefix_len`: a layer's settings, forwarded so that a
    non-zero value is refused (NativeError, AIC_ERR_UNSUPPORTED) rather than ignored."""
    qd, kvd = _attn_dtypes(q, k_cache, v_cache, out)
    _check_kv_layout(k_cache, v_cache)
    T, Hq, D = q.shape
    nb, bs, Hkv, D2 = k_cache.shape
    if T != tree.num_tokens or seq_lens.numel() != tree.batch:
        raise ValueError(f"the TreeDrafts describes {tree.batch} requests / {tree.num_tokens} tokens, the call has "
                         f"{seq_lens.numel()} / {T}")
    if sinks is not None and (sinks.dtype != torch.float32 or sinks.numel() != Hq or not sinks.is_contiguous()):
        raise ValueError("sinks: contiguous float32, one value per query head")
    assert D == D2 and q.stride(2) == 1 and q.stride(1) == D
    refused = int(sliding_window or 0) != 0 or int(shared_prefix_len or 0) != 0
    if not refused:
        _need_cuda(q, k_cache, v_cache, block_table, seq_lens, tree.tree_mask, sinks)
    if out is None:
        out = torch.empty((T, Hq, D), dtype=q.dtype, device=q.device)
    ws = None
    if not refused:
        ws = _workspace(N.lib().aic_verify_attention_workspace_bytes(T, Hq, D, num_splits_max), q.device, stream)
    N.check(N.lib().aic_verify_attention_tree(
        q.data_ptr(), q.stride(0), k_cache.data_ptr(), v_cache.data_ptr(), k_cache.stride(0), kvd, _ptr(k_scale),
        _ptr(v_scale), block_table.data_ptr(), block_table.size(1), seq_lens.data_ptr(), tree.query_start_loc.data_ptr(),
        tree.batch, T, max(1, tree.max_q_len), Hq, Hkv, D, bs, float(sm_scale), out.data_ptr(), out.stride(0), _ptr(ws),
        0 if ws is None else ws.numel(), int(max_seq_len), int(sliding_window or 0), int(shared_prefix_len or 0),
        _ptr(sinks), qd, tree.tree_mask.data_ptr(), 0 if refused else (N.current_stream_ptr() if stream is None else stream)))
    return out


class TreeRejectionResult(RejectionResult):
    __slots__ = ("path",)

    def __init__(self, output_token_ids, num_accepted, last_token, hidden_index, path):
        super().__init__(output_token_ids, num_accepted, last_token, hidden_index)
        self.path = path


def rejection_sample_tree(target_logits: torch.Tensor, tree: TreeDrafts,
                          row_index: Optional[torch.Tensor] = None) -> TreeRejectionResult:
    """Greedy acceptance over the step's trees (aic_rejection_tree_greedy).  `target_logits` [rows, V] with one row per
    query token — row t of the step, or `target_logits[row_index[t]]` with `row_index` int64 [T] (the model's full
    logits, un-gathered).  Per request: emit the arg-max of the current node's row, step to the child that carries it,
    stop when none does.  Result: RejectionResult's fields (`output_token_ids` int32 [B, max_q_len], -1 padded) plus
    `path` int32 [B, max_q_len], the nodes taken (path[:, 0] = 0, -1 behind the last).  Random acceptance over trees is
    not served."""
    if target_logits.dim() != 2 or target_logits.stride(1) != 1:
        raise ValueError("target_logits must be [rows, V] with contiguous rows")
    T, B = tree.num_tokens, tree.batch
    if row_index is not None and (row_index.dtype != torch.int64 or row_index.numel() != T):
        raise ValueError("row_index must be int64 with one entry per query token")
    if row_index is None and target_logits.size(0) != T:
        raise ValueError(f"target_logits has {target_logits.size(0)} rows, the step {T} query tokens")
    _need_cuda(target_logits, tree.draft_token_ids, row_index)
    dev = target_logits.device
    W = max(1, tree.max_q_len)
    V = int(target_logits.size(1))
    out = torch.empty((B, W), dtype=torch.int32, device=dev)
    path = torch.empty((B, W), dtype=torch.int32, device=dev)
    nacc = torch.empty(B, dtype=torch.int32, device=dev)
    last = torch.empty(B, dtype=torch.int32, device=dev)
    hidx = torch.empty(B, dtype=torch.int32, device=dev)
    if B == 0:
        return TreeRejectionResult(out, nacc, last, hidx, path)
    ws = _workspace(N.lib().aic_rejection_workspace_bytes(T, V), dev, purpose="accept")
    N.check(N.lib().aic_rejection_tree_greedy(
        target_logits.data_ptr(), N.torch_dtype_code(target_logits.dtype), int(target_logits.stride(0)), V,
        tree.draft_token_ids.data_ptr(), tree.parents.data_ptr(), tree.query_start_loc.data_ptr(), B, T, W,
        out.data_ptr(), nacc.data_ptr(), last.data_ptr(), hidx.data_ptr(), path.data_ptr(), _ptr(row_index), ws.data_ptr(),
        N.current_stream_ptr()))
    return TreeRejectionResult(out, nacc, last, hidx, path)


class KvPathCompactor:
    """compact_accepted_paths for a fixed set of caches: the checks and the per-layer pointer tables are done once (a
    runner calls it every step with the same caches), as KvBulkWriter does for the KV write."""

    def __init__(self, key_caches: List[torch.Tensor], value_caches: List[torch.Tensor]):
        L = len(key_caches)
        if L != len(value_caches):
            raise RuntimeError("key_caches and value_caches must have the same length")
        self.L = L
        if L == 0:
            return
        kc0 = key_caches[0]
        for c in list(key_caches) + list(value_caches):
            if c.shape != kc0.shape or c.dtype != kc0.dtype or c.stride() != kc0.stride():
                raise ValueError("every cache of the call must share shape, dtype and strides")
        _check_kv_layout(kc0, value_caches[0])
        _need_cuda(*key_caches, *value_caches)
        nb, bs, Hkv, D = kc0.shape
        VP = ctypes.c_void_p * L
        self._keep = (list(key_caches), list(value_caches))   # the tables hold raw pointers
        self.kc = VP(*[c.data_ptr() for c in key_caches])
        self.vc = VP(*[c.data_ptr() for c in value_caches])
        self.geom = (int(Hkv), int(D), int(kc0.element_size()), int(bs), int(kc0.stride(0)))

    def __call__(self, block_table: torch.Tensor, seq_lens: torch.Tensor, tree: TreeDrafts, path: torch.Tensor,
                 num_accepted: torch.Tensor, stream: Optional[int] = None) -> None:
        if self.L == 0 or tree.batch == 0:
            return
        _need_cuda(block_table, seq_lens, path, num_accepted)
        if path.dtype != torch.int32 or path.dim() != 2 or path.size(0) != tree.batch or not path.is_contiguous():
            raise ValueError("path must be contiguous int32 [B, max_q_len]")
        if num_accepted.dtype != torch.int32 or num_accepted.numel() != tree.batch:
            raise ValueError("num_accepted must be int32 [B]")
        N.check(N.lib().aic_kv_compact_paths(
            self.kc, self.vc, self.L, block_table.data_ptr(), block_table.size(1), seq_lens.data_ptr(),
            tree.query_start_loc.data_ptr(), path.data_ptr(), num_accepted.data_ptr(), tree.batch, int(path.size(1)),
            *self.geom, N.current_stream_ptr() if stream is None else stream))


def compact_accepted_paths(key_caches: List[torch.Tensor], value_caches: List[torch.Tensor], block_table: torch.Tensor,
                           seq_lens: torch.Tensor, tree: TreeDrafts, path: torch.Tensor, num_accepted: torch.Tensor,
                           stream: Optional[int] = None) -> None:
    """After acceptance: node path[i][d]'s K and V move to key position seq_lens[i] - q_len_i + d in every layer's
    caches, one launch (aic_kv_compact_paths).  `seq_lens` is the attention call's (query tokens counted); `path` /
    `num_accepted` are rejection_sample_tree's.  Bytes are copied: any cache dtype.  Nothing outside the destination
    slots changes; afterwards the cache is what decoding the accepted chain alone would have left.  A caller with a fixed
    set of caches builds a KvPathCompactor once instead."""
    KvPathCompactor(key_caches, value_caches)(block_table, seq_lens, tree, path, num_accepted, stream)


# ------------------------------------------------------------------------------------------------
# A5p whole-step attention: decodes, long drafts and prefill chunks in one call
# ------------------------------------------------------------------------------------------------
MAX_DECODE_Q_LEN = 33     # MAX_SPEC_LEN + 1: longer queries are prefill chunks (aic_step_attention's prefill body)


def split_order3(q_lens_host: Sequence[int], group_size: int):
    """Three-way partition of a step for aic_step_attention: (request ids as int32 = the short requests, then the
    prefill requests, then the long drafts, each in batch order; n_short, n_prefill, n_long).  Prefill = q_len >
    MAX_DECODE_Q_LEN; short = q_len * Hq/Hkv <= 32 query rows (split_order's rule); long = the rest."""
    import numpy as np
    ql = np.asarray(q_lens_host, dtype=np.int64)
    is_pf = ql > MAX_DECODE_Q_LEN
    is_short = ~is_pf & (ql * group_size <= 32)
    is_long = ~is_pf & ~is_short
    order = np.concatenate([np.nonzero(is_short)[0], np.nonzero(is_pf)[0], np.nonzero(is_long)[0]]).astype(np.int32)
    return order, int(is_short.sum()), int(is_pf.sum()), int(is_long.sum())


def decode_index(q_lens_host: Sequence[int]):
    """Compact layout of a step's decode rows: (query_start_loc int32 [B + 1] in which every prefill request has an empty
    range, token of the call of each compact row int32 [num_decode_tokens], max decode q_len)."""
    import numpy as np
    ql = np.asarray(q_lens_host, dtype=np.int64)
    dec = np.where(ql > MAX_DECODE_Q_LEN, 0, ql)
    qsl = np.zeros(len(ql) + 1, dtype=np.int32)
    np.cumsum(dec, out=qsl[1:])
    starts = np.zeros(len(ql), dtype=np.int64)
    np.cumsum(ql[:-1], out=starts[1:])
    idx = np.concatenate([np.arange(s, s + n, dtype=np.int32) for s, n in zip(starts, dec) if n > 0]) \
        if dec.sum() > 0 else np.zeros(0, dtype=np.int32)
    return qsl, idx.astype(np.int32), int(dec.max()) if len(dec) else 0


class StepSplit:
    """What aic_step_attention needs of a step's per-request query lengths, built once per step (host + one upload)
    and shared by every layer: the three-way request lists and the compact decode layout."""

    def __init__(self, q_lens_host: Sequence[int], group_size: int, device):
        import numpy as np
        ql = np.asarray(q_lens_host, dtype=np.int64)
        order, self.n_short, self.n_prefill, self.n_long = split_order3(ql, group_size)
        qsl, idx, self.max_decode_q_len = decode_index(ql)
        self.num_decode_tokens = int(idx.size)
        self.max_prefill_q_len = int(ql[ql > MAX_DECODE_Q_LEN].max()) if self.n_prefill else 0
        self.num_tokens = int(ql.sum())
        self.batch = int(ql.size)
        staged = torch.from_numpy(np.concatenate([order, qsl, idx]).astype(np.int32)).to(device, non_blocking=True)
        B = self.batch
        self.req_lists = staged[:B]
        self.decode_qsl = staged[B:2 * B + 1]
        self.decode_index = staged[2 * B + 1:]


def step_attention(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, block_table: torch.Tensor,
                   seq_lens: torch.Tensor, query_start_loc: torch.Tensor, max_seq_len: int, sm_scale: float,
                   q_lens_host: Optional[Sequence[int]] = None, step_split: Optional[StepSplit] = None,
                   out: Optional[torch.Tensor] = None, num_splits_max: int = 64,
                   k_scale: Optional[torch.Tensor] = None, v_scale: Optional[torch.Tensor] = None,
                   stream: Optional[int] = None, sliding_window: int = 0,
                   sinks: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Attention for a whole step whatever its query lengths (aic_step_attention_dt): prefill chunks (q_len > 33)
    beside decodes and long drafts, in any batch order.  Same tensors, dtypes and conventions as verify_attention; the step's
    geometry comes from `q_lens_host` or a StepSplit built from it once per step (pass that to every layer).
    `sliding_window` W > 0 / `sinks` f32 [Hq]: the per-layer features of gpt-oss-class models, as in verify_attention."""
    if sinks is not None and (sinks.dtype != torch.float32 or sinks.numel() != q.shape[1] or not sinks.is_contiguous()):
        raise ValueError("sinks: contiguous float32, one value per query head")
    qd, kvd = _attn_dtypes(q, k_cache, v_cache, out)
    _check_kv_layout(k_cache, v_cache)
    _need_cuda(q, k_cache, v_cache, block_table, seq_lens, query_start_loc, sinks)
    T, Hq, D = q.shape
    nb, bs, Hkv, D2 = k_cache.shape
    assert D == D2 and q.stride(2) == 1 and q.stride(1) == D
    if step_split is None:
        if q_lens_host is None:
            raise ValueError("step_attention needs the step's per-request query lengths (q_lens_host or step_split)")
        step_split = StepSplit(q_lens_host, Hq // Hkv, q.device)
    sp = step_split
    if sp.batch != seq_lens.numel() or sp.num_tokens > T:
        raise ValueError("the step split does not describe this call")
    if out is None:
        out = torch.empty((T, Hq, D), dtype=q.dtype, device=q.device)
    wsb = N.lib().aic_step_attention_workspace_bytes(sp.num_decode_tokens, sp.n_prefill, sp.max_prefill_q_len, Hq, Hkv, D,
                                                     num_splits_max)
    ws = _workspace(wsb, q.device, stream)
    N.check(N.lib().aic_step_attention_dt(
        q.data_ptr(), q.stride(0), k_cache.data_ptr(), v_cache.data_ptr(), k_cache.stride(0),
        kvd, _ptr(k_scale), _ptr(v_scale), block_table.data_ptr(), block_table.size(1),
        seq_lens.data_ptr(), query_start_loc.data_ptr(), sp.batch, sp.num_tokens, Hq, Hkv, D, bs, float(sm_scale),
        out.data_ptr(), out.stride(0), ws.data_ptr(), ws.numel(), int(max_seq_len), sp.req_lists.data_ptr(), sp.n_short,
        sp.n_prefill, sp.n_long, sp.decode_qsl.data_ptr(), _ptr(sp.decode_index) if sp.num_decode_tokens else None,
        sp.num_decode_tokens, max(1, sp.max_decode_q_len), sp.max_prefill_q_len, int(sliding_window or 0), _ptr(sinks),
        qd, N.current_stream_ptr() if stream is None else stream))
    return out


# ------------------------------------------------------------------------------------------------
# A12 Ulysses repartition copies
# ------------------------------------------------------------------------------------------------
def ulysses_pack_qkv(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, sp: int) -> torch.Tensor:
    """q [n, SP*qw], k/v [n, SP*kw] -> send [SP*n, qw+2kw] (rank-major), ulysses.py:493-499."""
    _need_cuda(q, k, v)
    n = q.size(0)
    qw, kw = q.size(1) // sp, k.size(1) // sp
    send = torch.empty((sp * n, qw + 2 * kw), dtype=q.dtype, device=q.device)
    N.check(N.lib().aic_ulysses_pack_qkv(q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(0), k.stride(0),
                                         v.stride(0), send.data_ptr(), n, sp, qw, kw, N.current_stream_ptr()))
    return send


def ulysses_split_qkv(recv: torch.Tensor, qw: int, kw: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    _need_cuda(recv)
    rows = recv.size(0)
    q = torch.empty((rows, qw), dtype=recv.dtype, device=recv.device)
    k = torch.empty((rows, kw), dtype=recv.dtype, device=recv.device)
    v = torch.empty((rows, kw), dtype=recv.dtype, device=recv.device)
    N.check(N.lib().aic_ulysses_split_qkv(recv.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(), rows, qw, kw,
                                          N.current_stream_ptr()))
    return q, k, v


def ulysses_unpack_out(recv: torch.Tensor, sp: int) -> torch.Tensor:
    """recv [SP*n, w] (rank-major) -> out [n, SP*w], ulysses.py:515-517."""
    _need_cuda(recv)
    n = recv.size(0) // sp
    w = recv.size(1)
    out = torch.empty((n, sp * w), dtype=recv.dtype, device=recv.device)
    N.check(N.lib().aic_ulysses_unpack_out(recv.data_ptr(), out.data_ptr(), n, sp, w, N.current_stream_ptr()))
    return out


def ulysses_pack_pair(a: torch.Tensor, b: Optional[torch.Tensor], parts: int) -> torch.Tensor:
    """KV-replicated variant (ulysses.py:463-474): a [n, parts*aw] (and b [n, parts*bw]) -> send [parts*n, aw (+ bw)],
    part-major: the q pack for the all-to-all over SP (b None) and the K|V pack for the all-to-all inside SP_AA."""
    _need_cuda(a, b)
    n = a.size(0)
    aw = a.size(1) // parts
    bw = 0 if b is None else b.size(1) // parts
    send = torch.empty((parts * n, aw + bw), dtype=a.dtype, device=a.device)
    N.check(N.lib().aic_ulysses_pack_pair(a.data_ptr(), _ptr(b), a.stride(0), 0 if b is None else b.stride(0),
                                          send.data_ptr(), n, parts, aw, bw, N.current_stream_ptr()))
    return send


def ulysses_reorder_split_kv(gathered: torch.Tensor, sp: int, order: Sequence[int]) -> Tuple[torch.Tensor, torch.Tensor]:
    """gathered [sp*n, 2*kw] in all-gather chunk order -> (k, v) [sp*n, kw] each with chunk c taken from chunk order[c]
    (ulysses.py:486-490: chunk / cat in `self.order` / split)."""
    _need_cuda(gathered)
    rows, w2 = gathered.shape
    n, kw = rows // sp, w2 // 2
    k = torch.empty((rows, kw), dtype=gathered.dtype, device=gathered.device)
    v = torch.empty((rows, kw), dtype=gathered.dtype, device=gathered.device)
    arr = (ctypes.c_int32 * sp)(*[int(x) for x in order])
    N.check(N.lib().aic_ulysses_reorder_split_kv(gathered.data_ptr(), k.data_ptr(), v.data_ptr(), n, sp, kw, arr,
                                                 N.current_stream_ptr()))
    return k, v


def quantize_fp8_per_tensor(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    _need_cuda(x)
    x = x.contiguous()
    q = torch.empty(x.shape, dtype=torch.float8_e4m3fn, device=x.device)
    scale = torch.empty(1, dtype=torch.float32, device=x.device)
    N.check(N.lib().aic_quantize_fp8_per_tensor(x.data_ptr(), q.data_ptr(), scale.data_ptr(), x.numel(),
                                                N.current_stream_ptr()))
    return q, scale
