"""A vLLM SamplingMetadata's logits edits as the packed arguments of ops.edit_logits (aic_logits_edit): which requests
ban which tokens this step, their bias, their histories and their penalties.  vLLM-free, and free of device
synchronisation: everything that lives on the host (output tokens, bad words, min_tokens, bias dicts) is gathered into
ONE pinned int32 buffer and copied once per step; the prompt matrix and the per-request tensors are already on the
device.  Field layouts as vLLM 0.9.2's InputBatch._make_sampling_metadata fills them (recalled; tests/stubs carries the
same): `logit_bias` a list with one Optional[dict] per request, `min_tokens` {index: (min_tokens, stop ids)},
`bad_words_token_ids` {index: [[token, ...], ...]}, `output_token_ids` a list of lists, `prompt_token_ids` an integer
[requests, longest prompt] matrix padded with the vocabulary size, None unless a request has penalties.

Row i of the one Sampler call of a step is request i — every row of a draft-free step, the bonus rows of a verify
step — so the packed arguments are per request in both; a verify step passes its bonus rows as `row_index`."""
from __future__ import annotations

import os
from typing import Dict, List, Sequence

import numpy as np
import torch

LOGITS_EDITS_ENV = "ARCTIC_INFERENCE_HIP_LOGITS_EDITS"   # 1: steps with penalties / min-p / bias / bans stay on the HIP routes (default off)


def logits_edits_switch() -> bool:
    return os.environ.get(LOGITS_EDITS_ENV, "0").strip().lower() in ("1", "true", "yes", "on")


def has_edits(sm) -> bool:
    """Whether any request of this SamplingMetadata edits its logits before sampling: exactly the fields that
    runner_logic.hip_sampler_ok / hip_acceptance_kind exclude without `logits_edits`."""
    if not getattr(sm, "no_penalties", True):
        return True
    if getattr(sm, "allowed_token_ids_mask", None) is not None or getattr(sm, "bad_words_token_ids", None):
        return True
    if any(b is not None and len(b) > 0 for b in (getattr(sm, "logit_bias", None) or ())):
        return True
    return bool(getattr(sm, "min_tokens", None)) or getattr(sm, "min_p", None) is not None


def banned_tokens(sm, num_reqs: int) -> List[List[int]]:
    """Per request, the tokens whose logit becomes -inf this step: the stop ids of a request whose output is still
    shorter than its min_tokens (apply_min_token_penalties), and the last token of every bad-word sequence whose other
    tokens equal the tail of the request's output — a one-token sequence always (apply_bad_words)."""
    outputs = getattr(sm, "output_token_ids", None) or []
    bans: List[List[int]] = [[] for _ in range(num_reqs)]
    for i, (min_tokens, stop_ids) in (getattr(sm, "min_tokens", None) or {}).items():
        if i < num_reqs and len(outputs[i]) < min_tokens:
            bans[i].extend(int(t) for t in stop_ids)
    for i, words in (getattr(sm, "bad_words_token_ids", None) or {}).items():
        if i >= num_reqs:
            continue
        past = outputs[i]
        for word in words:
            n = len(word) - 1
            if n < 0 or n > len(past):
                continue
            if n == 0 or list(past[len(past) - n:]) == list(word[:n]):
                bans[i].append(int(word[-1]))
    return bans


def _csr(lists: Sequence[Sequence], parts: List[np.ndarray]) -> None:
    """Appends the int32 offsets [len(lists) + 1] and the concatenation of `lists` to `parts`."""
    off = np.zeros(len(lists) + 1, dtype=np.int32)
    np.cumsum([len(x) for x in lists], out=off[1:])
    parts.append(off)
    parts.append(np.fromiter((v for x in lists for v in x), dtype=np.int32, count=int(off[-1])))


def pack_edits(sm, num_reqs: int, device) -> Dict[str, object]:
    """The keyword arguments of ops.edit_logits for this step (without `row_index`): only the edits some request uses
    are present.  min-p is left out of an all-greedy batch: it touches no greedy row."""
    device = torch.device(device)
    kw: Dict[str, object] = {}
    mask = getattr(sm, "allowed_token_ids_mask", None)
    if mask is not None:
        kw["allowed_mask"] = mask[:num_reqs].contiguous()
    bans = banned_tokens(sm, num_reqs)
    biases = [(b or {}) for b in (getattr(sm, "logit_bias", None) or ())][:num_reqs]
    biases += [{}] * (num_reqs - len(biases))
    penalties = not getattr(sm, "no_penalties", True)
    # one host buffer: [ban offsets | ban tokens | bias offsets | bias tokens | bias values (f32 bits) | output offsets |
    # output tokens], every piece int32-sized
    parts: List[np.ndarray] = []
    names: List[str] = []
    if any(bans):
        _csr(bans, parts)
        names += ["ban_off", "ban_tok"]
    if any(biases):
        _csr([list(b.keys()) for b in biases], parts)
        parts.append(np.fromiter((v for b in biases for v in b.values()), dtype=np.float32).view(np.int32))
        names += ["bias_off", "bias_tok", "bias_val"]
    if penalties:
        outputs = list(getattr(sm, "output_token_ids", None) or [])[:num_reqs]
        outputs += [[]] * (num_reqs - len(outputs))
        _csr(outputs, parts)
        names += ["out_off", "out_tok"]
    if parts:
        total = sum(p.size for p in parts)
        host = torch.empty(total, dtype=torch.int32, pin_memory=device.type == "cuda")
        view = host.numpy()
        at = 0
        for p in parts:
            view[at:at + p.size] = p
            at += p.size
        dev = host.to(device, non_blocking=True)          # the one copy of the step
        pieces, at = {}, 0
        for name, p in zip(names, parts):
            pieces[name] = dev[at:at + p.size]
            at += p.size
        if "ban_off" in pieces:
            kw["ban"] = (pieces["ban_off"], pieces["ban_tok"])
        if "bias_off" in pieces:
            kw["bias"] = (pieces["bias_off"], pieces["bias_tok"], pieces["bias_val"].view(torch.float32))
        if "out_off" in pieces:
            kw["output"] = (pieces["out_off"], pieces["out_tok"])
    if penalties:
        prompt = getattr(sm, "prompt_token_ids", None)
        if prompt is not None:
            prompt = prompt[:num_reqs]
            width = int(prompt.shape[1])
            # rows of equal width: the padding (the vocabulary size) is outside [0, vocab) and ignored by the kernel
            kw["prompt"] = (torch.arange(num_reqs + 1, dtype=torch.int32, device=device) * width,
                            prompt.to(device=device, dtype=torch.int32).reshape(-1).contiguous())
        for key, field in (("repetition", "repetition_penalties"), ("frequency", "frequency_penalties"),
                           ("presence", "presence_penalties")):
            t = getattr(sm, field, None)
            if t is not None:
                kw[key] = t[:num_reqs].to(device=device, dtype=torch.float32).contiguous()
    min_p = getattr(sm, "min_p", None)
    temperature = getattr(sm, "temperature", None)
    if min_p is not None and temperature is not None and not getattr(sm, "all_greedy", False):
        kw["min_p"] = min_p[:num_reqs].to(device=device, dtype=torch.float32).contiguous()
        kw["temperature"] = temperature[:num_reqs].to(device=device, dtype=torch.float32).contiguous()
    return kw
