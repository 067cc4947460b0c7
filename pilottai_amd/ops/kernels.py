"""Dispatch layer for the CDNA4 HIP kernels (pilottai_amd/_C.so).

Device tensors ALWAYS go to the native kernels: if the extension failed to load
on a machine with a GPU, every call raises (no silent PyTorch fallback — the
round-end driver checks which .so files the GPU tests actually loaded). CPU
tensors run the fp32 reference implementations in ops/reference.py, which is
how the control-plane tests execute the whole engine without a GPU.
"""
from __future__ import annotations

import importlib
import os
from typing import Optional

import torch

from . import reference as ref

_C = None
_LOAD_ERROR: Optional[BaseException] = None


def _load():
    global _C, _LOAD_ERROR
    if _C is not None or _LOAD_ERROR is not None:
        return _C
    try:
        _C = importlib.import_module("pilottai_amd._C")
        if os.environ.get("PILOTTAI_DECODE_VARIANT"):  # A/B switch of the packed decode GEMM
            _C.decode_set_variant(int(os.environ["PILOTTAI_DECODE_VARIANT"]))
    except BaseException as e:  # noqa: BLE001 — surfaced by require_native()
        _LOAD_ERROR = e
    return _C


def native_available() -> bool:
    return _load() is not None


def require_native():
    mod = _load()
    if mod is None:
        raise RuntimeError(
            "pilottai_amd native kernels (_C.so) are not available: "
            f"{_LOAD_ERROR!r}. Build them with `python -m pilottai_amd._build` "
            "(hipcc --offload-arch=gfx950).")
    return mod


def native_module_path() -> Optional[str]:
    mod = _load()
    return getattr(mod, "__file__", None) if mod is not None else None


def _on_gpu(t: torch.Tensor) -> bool:
    return t.device.type == "cuda"


# ---------------------------------------------------------------------------


def empty_handoff(numel: int, dtype=torch.float32, device=None) -> torch.Tensor:
    """A buffer that one workgroup writes and another reads INSIDE one launch (split-K slabs,
    attention partition partials). On the GPU it lives in uncached device memory
    (hipDeviceMallocUncached): no CU or XCD can hold a stale copy of its lines, so the
    in-launch hand-off is correct for any workgroup placement with a relaxed ticket and the
    last arriver's acquire, and needs no producer-side L2 write-back (VERDICT r3 weak #1,
    profiles/r4_handoff_uncached.md). Zero-filled. Allocate outside graph capture."""
    device = torch.device(device) if device is not None else torch.device("cpu")
    if device.type == "cuda":
        idx = device.index if device.index is not None else torch.cuda.current_device()
        return require_native().empty_uncached(int(numel), dtype, int(idx))
    return torch.zeros(int(numel), dtype=dtype, device=device)


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float, out: Optional[torch.Tensor] = None):
    if _on_gpu(x):
        out = torch.empty_like(x) if out is None else out
        require_native().rmsnorm(out, x, w, float(eps))
        return out
    r = ref.rmsnorm(x, w, eps)
    if out is not None:
        out.copy_(r)
        return out
    return r


def fused_add_rmsnorm(resid: torch.Tensor, x: torch.Tensor, w: torch.Tensor, eps: float,
                      out: Optional[torch.Tensor] = None):
    """resid <- resid + x (in place); returns rmsnorm(resid) * w."""
    if _on_gpu(x):
        out = torch.empty_like(x) if out is None else out
        require_native().fused_add_rmsnorm(out, resid, x, w, float(eps))
        return out
    y, nr = ref.fused_add_rmsnorm(resid, x, w, eps)
    resid.copy_(nr)
    if out is not None:
        out.copy_(y)
        return out
    return y


def silu_mul(x: torch.Tensor, out: Optional[torch.Tensor] = None):
    if _on_gpu(x):
        F = x.shape[-1] // 2
        out = torch.empty(*x.shape[:-1], F, dtype=x.dtype, device=x.device) if out is None else out
        require_native().silu_mul(out, x)
        return out
    r = ref.silu_mul(x)
    if out is not None:
        out.copy_(r)
        return out
    return r


def rope_cache(q_out, k_cache, v_cache, qkv, positions, slot_mapping, cos_sin, H: int, KV: int,
               apply_rope: bool = True):
    if _on_gpu(qkv):
        require_native().rope_cache(q_out, k_cache, v_cache, qkv, positions, slot_mapping, cos_sin,
                                    int(H), int(KV), bool(apply_rope))
        return q_out
    ref.rope_cache(q_out, k_cache, v_cache, qkv, positions, slot_mapping, cos_sin, H, KV,
                   apply_rope)
    return q_out


def kv_copy(k_cache, v_cache, n_copies, copies) -> None:
    """Partial-block prefix reuse (csrc/ops/kv_copy.hip): for each of the first `n_copies[0]`
    (donor block, new block, j) triples of `copies`, copy the first j key slots of the donor's
    K and V pages to the new block, in every layer and KV head. `k_cache` is
    [layers, blocks, KV, 16, 16, 8], `v_cache` [layers, blocks, KV, 128, 16]; the count and the
    triples are int32 tensors on the caches' device (graph-capturable: a fixed launch shape)."""
    if _on_gpu(k_cache):
        require_native().kv_copy(k_cache, v_cache, n_copies, copies)
        return
    ref.kv_copy(k_cache, v_cache, n_copies, copies)


def kv_gather_blocks(k_cache, v_cache, ids, n: int, stage) -> None:
    """Host tier of the prefix cache (csrc/ops/kv_pages.hip): for i < n, every layer's K and V
    pages of block `ids[i]` go to record i of `stage` [records, layers * 2 * KV * 2048], laid
    out [layer][K|V][KV][page]. `ids` is an int32 tensor on the caches' device, `n` a plain
    number (not graph-capturable); an id outside [0, blocks) leaves its record alone."""
    if _on_gpu(k_cache):
        require_native().kv_gather_blocks(k_cache, v_cache, ids, int(n), stage)
        return
    ref.kv_gather_blocks(k_cache, v_cache, ids, n, stage)


def kv_scatter_blocks(k_cache, v_cache, ids, n: int, stage) -> None:
    """The inverse of kv_gather_blocks: record i of `stage` goes to the pages of block `ids[i]`;
    nothing outside the listed blocks is written."""
    if _on_gpu(k_cache):
        require_native().kv_scatter_blocks(k_cache, v_cache, ids, int(n), stage)
        return
    ref.kv_scatter_blocks(k_cache, v_cache, ids, n, stage)


def span_pool(hn, n_seg, segs, pool) -> None:
    """Span pooling (csrc/ops/span_pool.hip): for each of the first `n_seg[0]` (first_row, n_rows,
    slot, init) quadruples of `segs`, pool[slot] = (0 if init else pool[slot]) + hn[first_row] + ...
    + hn[first_row + n_rows - 1], the rows added one by one in that order in fp32. `hn` is [T, d]
    bf16 with d % 8 == 0 (ValueError otherwise), `pool` [slots, d] fp32; the count and the
    quadruples are int32 tensors on hn's device (graph-capturable: a fixed launch shape). A segment
    that leaves hn's rows or pool's slots is skipped."""
    if hn.shape[-1] % 8 != 0:
        raise ValueError(f"span_pool: the row length {hn.shape[-1]} must be a multiple of 8")
    if _on_gpu(hn):
        require_native().span_pool(hn, n_seg, segs, pool)
        return
    ref.span_pool(hn, n_seg, segs, pool)


def paged_attention(out, part_o, part_ml, q, k_cache, v_cache, items, n_items, counters,
                    q_start, q_len, ctx_len, block_table, scale: float, num_seqs: Optional[int] = None,
                    part_size: Optional[torch.Tensor] = None, waves: int = 4):
    """Attention over the paged cache. On GPU `items` must be a device int32
    [max, 4] tensor with a device count (graph-capturable) and `counters` a
    zero-initialised int32 tensor of >= seqs * KV entries (partition tickets; the
    kernel leaves it zeroed); on CPU the reference path ignores both. `waves` 8: 512-thread workgroups for the decode and 32-column prefill items (small decode
    batches; wide items run as their 32-column sub-items)."""
    if _on_gpu(q):
        require_native().paged_attention(out, part_o, part_ml, q, k_cache, v_cache, items, n_items,
                                         counters, q_start, q_len, ctx_len, block_table,
                                         float(scale), part_size, int(waves))
        return out
    ns = len(q_len) if num_seqs is None else num_seqs
    r = ref.paged_attention(q, k_cache, v_cache, q_start[:ns], q_len[:ns], ctx_len[:ns],
                            block_table, scale)
    n_tok = int(q_start[ns - 1] + q_len[ns - 1]) if ns > 0 else 0
    out[:n_tok].copy_(r[:n_tok])
    return out


def sample_workspace(rows: int, V: int, device) -> torch.Tensor:
    n = require_native().sample_workspace_floats(rows, V)
    return torch.empty(n, dtype=torch.float32, device=device)


def topkp_threshold(logits, V: int, temperature, top_k, top_p, mask_class, class_masks,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-row logit threshold tau for top-k / top-p (csrc/ops/sampling.hip).

    `logits` is [rows, V] or a TP all-gather [shards, rows, V/shards]."""
    rows = logits.shape[-2]
    tau = out if out is not None else torch.empty(rows, dtype=torch.float32, device=logits.device)
    if _on_gpu(logits):
        require_native().topkp_threshold(tau, logits, int(V), temperature, top_k, top_p, mask_class,
                                         class_masks)
        return tau
    full = logits if logits.dim() == 2 else logits.permute(1, 0, 2).reshape(rows, V)
    tau[:rows].copy_(ref.topkp_threshold(full, temperature, top_k, top_p, mask_class, class_masks))
    return tau


def patch_pending_ids(ids: torch.Tensor, sampled: torch.Tensor) -> None:
    """In place: ids[t] = sampled[-ids[t] - 1] where ids[t] < 0 (pipelined engine steps:
    a row's pending token comes from the previous step's sampler, csrc/ops/sampling.hip)."""
    if _on_gpu(ids):
        require_native().patch_pending_ids(ids, sampled)
        return
    neg = ids < 0
    if bool(neg.any()):
        r = (-ids[neg] - 1).long()
        ids[neg] = torch.where(r < sampled.numel(), sampled[r.clamp(max=sampled.numel() - 1)],
                               torch.zeros_like(r, dtype=ids.dtype))


def sample(logits, temperature, mask_class, class_masks, seeds, offsets, forced=None,
           out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
           vocab_offset: int = 0, out_keys: Optional[torch.Tensor] = None,
           tau: Optional[torch.Tensor] = None):
    rows = logits.shape[0]
    if _on_gpu(logits):
        C = require_native()
        out = torch.empty(rows, dtype=torch.int32, device=logits.device) if out is None else out
        if workspace is None:
            workspace = sample_workspace(rows, logits.shape[1], logits.device)
        C.sample(out, out_keys, workspace, logits, int(vocab_offset), temperature, mask_class,
                 class_masks, seeds, offsets, forced, tau)
        return out
    toks, keys = ref.sample(logits, temperature, mask_class, class_masks, seeds, offsets, forced,
                            vocab_offset, return_keys=True, tau=tau)
    if out_keys is not None:
        out_keys[:rows].copy_(keys)
    if out is not None:
        out[:rows].copy_(toks)
        return out
    return toks


SPEC_VERIFY_LAUNCHES = 1  # kernels spec_verify() launches on the GPU (it replaces the sampler's final merge)
NO_TOKEN = 0x7FFFFFFF     # id of a sampler partial with no allowed token


def sample_partials(logits, temperature, mask_class, class_masks, seeds, offsets, workspace: torch.Tensor,
                    tau: Optional[torch.Tensor] = None):
    """The sampler's chunk pass alone (csrc/ops/sampling.hip): returns (part_k fp32, part_i int32)
    [rows, nchunk], views of `workspace`, for spec_verify(). On the CPU: one partial per row from
    the reference sampler."""
    rows, V = logits.shape
    if _on_gpu(logits):
        C = require_native()
        C.sample_partials(workspace, logits, 0, temperature, mask_class, class_masks, seeds, offsets, tau)
        nchunk = C.sample_workspace_floats(1, V) // 2
        return (workspace[:rows * nchunk].view(rows, nchunk),
                workspace[rows * nchunk:2 * rows * nchunk].view(torch.int32).view(rows, nchunk))
    toks, keys = ref.sample(logits, temperature, mask_class, class_masks, seeds, offsets, None, 0,
                            return_keys=True, tau=tau)
    toks = torch.where(torch.isinf(keys) & (keys < 0), torch.full_like(toks, NO_TOKEN), toks)
    return keys.view(rows, 1), toks.view(rows, 1)


def spec_verify(part_k, part_i, forced, input_ids, logit_rows, run_first, run_len,
                out_tokens: Optional[torch.Tensor] = None, accept_len: Optional[torch.Tensor] = None):
    """Final merge of the sampler's partials plus draft verification (csrc/ops/spec_verify.hip):
    out_tokens[row] = forced[row] if >= 0, else the id of the row's best partial (larger key,
    equal keys by smaller id; 0 when the row has no allowed token). Rows [first, first + len) of a
    run belong to one drafting request; the draft token row j verifies is the input id of row
    j + 1, input_ids[logit_rows[first + j + 1]]. accept_len[first] = 1 + the number of leading
    rows whose token equals their draft token, 0 on the run's other rows; a plain row is a run of
    length 1 and gets 1. A descriptor that is not a valid run makes the row a run of its own.
    Returns (out_tokens, accept_len), int32 [rows]."""
    rows = part_k.shape[0]
    dev = part_k.device
    out_tokens = torch.empty(rows, dtype=torch.int32, device=dev) if out_tokens is None else out_tokens
    accept_len = torch.empty(rows, dtype=torch.int32, device=dev) if accept_len is None else accept_len
    if _on_gpu(part_k):
        require_native().spec_verify(out_tokens, accept_len, part_k, part_i, forced, input_ids, logit_rows,
                                     run_first, run_len)
        return out_tokens, accept_len
    toks, acc = ref.spec_verify(part_k, part_i, forced, input_ids, logit_rows, run_first, run_len)
    out_tokens[:rows].copy_(toks)
    accept_len[:rows].copy_(acc)
    return out_tokens, accept_len


LOGPROB_TOP = 20             # alternatives per token the log-probability pass can return
TOKEN_LOGPROBS_LAUNCHES = 2  # kernels token_logprobs() launches on the GPU (chunk pass + row merge)


def token_logprobs_workspace(rows: int, V: int, device) -> torch.Tensor:
    n = require_native().logprob_workspace_floats(rows, V)
    return torch.empty(n, dtype=torch.float32, device=device)


def token_logprobs(logits, tokens, lp_n, forced, mask_class, class_masks, out=None,
                   workspace: Optional[torch.Tensor] = None):
    """Log-probabilities of the sampled `tokens` and of the lp_n[row] most likely alternatives
    (csrc/ops/sampling.hip): natural log of softmax(logits) over the tokens the row's mask class
    allows, at temperature 1. Returns / fills `out` = (logprob fp32 [rows], top_ids int32
    [rows, 20], top_lp fp32 [rows, 20]); the lists are sorted by logit descending, equal logits
    by smaller id, and end with id -1 / -inf. Rows with lp_n < 0 are left untouched; rows with
    forced >= 0 get (0.0, [(forced, 0.0)]); a row whose mask allows nothing gets -inf and an
    empty list. The outputs may be strided columns of one record buffer."""
    rows = logits.shape[0]
    if out is None:
        out = (torch.empty(rows, dtype=torch.float32, device=logits.device),
               torch.empty(rows, LOGPROB_TOP, dtype=torch.int32, device=logits.device),
               torch.empty(rows, LOGPROB_TOP, dtype=torch.float32, device=logits.device))
    lp, ids, lps = out
    if _on_gpu(logits):
        C = require_native()
        if workspace is None:
            workspace = token_logprobs_workspace(rows, logits.shape[1], logits.device)
        C.token_logprobs(lp, ids, lps, workspace, logits, tokens, lp_n, forced, mask_class, class_masks)
        return out
    r_lp, r_ids, r_lps = ref.token_logprobs(logits, tokens, lp_n, forced, mask_class, class_masks)
    asked = (lp_n[:rows] >= 0).cpu()
    if bool(asked.any()):
        lp[:rows][asked] = r_lp[asked]
        ids[:rows][asked] = r_ids[asked]
        lps[:rows][asked] = r_lps[asked]
    return out


SCORE_TOKENS_LAUNCHES = 2  # kernels score_tokens() launches on the GPU (chunk pass + row merge)


def score_tokens_workspace(rows: int, V: int, device) -> torch.Tensor:
    n = require_native().score_workspace_floats(rows, V)
    return torch.empty(n, dtype=torch.float32, device=device)


def score_tokens(logits, target, lp_n, out=None, workspace: Optional[torch.Tensor] = None):
    """Prompt scoring (csrc/ops/scoring.hip): per row with target[row] >= 0, the natural-log
    probability of that token under softmax(logits) over the whole vocabulary at temperature 1,
    its rank (1 + the tokens with a larger logit or an equal logit and a smaller id, compared on
    the bf16 order key, so exact) and the lp_n[row] (0..20) most likely tokens. Returns / fills
    `out` = (logprob fp32 [rows], rank int32 [rows], top_ids int32 [rows, 20], top_lp fp32
    [rows, 20]); the lists are those of token_logprobs (id -1 / -inf past the end). Rows with
    target < 0 are left untouched; a target >= V gives (-inf, rank 0). The outputs may be strided
    columns of one record buffer."""
    rows = logits.shape[0]
    if out is None:
        out = (torch.empty(rows, dtype=torch.float32, device=logits.device),
               torch.empty(rows, dtype=torch.int32, device=logits.device),
               torch.empty(rows, LOGPROB_TOP, dtype=torch.int32, device=logits.device),
               torch.empty(rows, LOGPROB_TOP, dtype=torch.float32, device=logits.device))
    lp, rank, ids, lps = out
    if _on_gpu(logits):
        C = require_native()
        if workspace is None:
            workspace = score_tokens_workspace(rows, logits.shape[1], logits.device)
        C.score_tokens(lp, rank, ids, lps, workspace, logits, target, lp_n)
        return out
    r_lp, r_rank, r_ids, r_lps = ref.score_tokens(logits, target, lp_n)
    asked = (target[:rows] >= 0).cpu()
    if bool(asked.any()):
        lp[:rows][asked] = r_lp[asked]
        rank[:rows][asked] = r_rank[asked]
        ids[:rows][asked] = r_ids[asked]
        lps[:rows][asked] = r_lps[asked]
    return out


PENALTY_LAUNCHES = 1  # kernels apply_penalties() launches on the GPU


def penalty_state(slots: int, V: int, cap: int, device):
    """Zeroed device state of `slots` penalty slots: (counts int32 [slots, V], distinct int32
    [slots, cap] -- the tokens whose count is non-zero -- and n_distinct int32 [slots])."""
    return (torch.zeros(slots, V, dtype=torch.int32, device=device),
            torch.zeros(slots, cap, dtype=torch.int32, device=device),
            torch.zeros(slots, dtype=torch.int32, device=device))


def apply_penalties(logits, state, pen_slot, pen_reset, presence, frequency, forced, pair_start, pair_n,
                    pair_tok):
    """Presence / frequency penalties, in place on `logits` [rows, V] bf16 (csrc/ops/penalties.hip).

    Row r with slot s = pen_slot[r] >= 0 and forced[r] < 0: if pen_reset[r], the slot's counts
    are cleared first; the tokens pair_tok[pair_start[r] : pair_start[r] + pair_n[r]] are added
    to the slot's counts; then every token t with count c > 0 gets
    logit[t] <- bf16(float(logit[t]) - (presence[r] + frequency[r] * c)), fp32 arithmetic, one
    round-to-nearest-even conversion. Every other row, and the state of its slot, is untouched.
    `state` = penalty_state(...), updated in place. A slot may appear in one row only."""
    counts, distinct, n_distinct = state
    if _on_gpu(logits):
        require_native().apply_penalties(logits, counts, distinct, n_distinct, pen_slot, pen_reset, presence,
                                         frequency, forced, pair_start, pair_n, pair_tok)
        return logits
    ref.apply_penalties(logits, state, pen_slot, pen_reset, presence, frequency, forced, pair_start, pair_n,
                        pair_tok)
    return logits


REPETITION_LAUNCHES = 1  # kernels apply_repetition_penalty() launches on the GPU


def repetition_state(slots: int, V: int, cap: int, device):
    """Zeroed device state of `slots` repetition-penalty slots: (seen int32 [slots, ceil(V / 32)]
    -- bit t & 31 of word t >> 5 = token t occurred --, seen_list int32 [slots, cap] -- the
    tokens that occurred, each once -- and n_seen int32 [slots])."""
    return (torch.zeros(slots, (V + 31) // 32, dtype=torch.int32, device=device),
            torch.zeros(slots, cap, dtype=torch.int32, device=device),
            torch.zeros(slots, dtype=torch.int32, device=device))


def apply_repetition_penalty(logits, state, rep_slot, rep_reset, rep_r, rep_inv_r, forced, rep_start, rep_n,
                             rep_tok):
    """Repetition penalty, in place on `logits` [rows, V] bf16 (csrc/ops/repetition.hip).

    Row i with slot s = rep_slot[i] >= 0 and forced[i] < 0: if rep_reset[i], the slot's set is
    cleared first; the tokens rep_tok[rep_start[i] : rep_start[i] + rep_n[i]] join the slot's
    set (ids outside [0, V) are skipped, a window that leaves rep_tok is not applied); then every
    token t of the set gets logit[t] <- bf16(x > 0 ? x * rep_inv_r[i] : x * rep_r[i]) with
    x = float(logit[t]) -- one correctly rounded fp32 product, one round-to-nearest-even
    conversion. Every other row, and the state of its slot, is untouched.
    `state` = repetition_state(...), updated in place. A slot may appear in one row only."""
    seen, seen_list, n_seen = state
    if _on_gpu(logits):
        require_native().apply_repetition_penalty(logits, seen, seen_list, n_seen, rep_slot, rep_reset, rep_r,
                                                  rep_inv_r, forced, rep_start, rep_n, rep_tok)
        return logits
    ref.apply_repetition_penalty(logits, state, rep_slot, rep_reset, rep_r, rep_inv_r, forced, rep_start, rep_n,
                                 rep_tok)
    return logits


LOGIT_BIAS_MAX = 300        # entries of one request's logit_bias (the OpenAI API's bound)
LOGIT_BIAS_LAUNCHES = 1     # kernels apply_logit_bias() launches on the GPU
MINP_THRESHOLD_LAUNCHES = 1  # kernels minp_threshold() launches on the GPU


def apply_logit_bias(logits, bias_start, bias_n, bias_tok, bias_val, forced):
    """logit_bias, in place on `logits` [rows, V] bf16 (csrc/ops/logit_shaping.hip).

    Row r with bias_n[r] > 0 and forced[r] < 0: for i in [bias_start[r], bias_start[r] +
    bias_n[r]), logit[bias_tok[i]] <- bf16(float(logit[bias_tok[i]]) + bias_val[i]) -- one fp32
    add, one round-to-nearest-even conversion. Token ids outside [0, V) are skipped, a list that
    leaves bias_tok is not applied, nothing else in the row is touched. A row's ids are unique."""
    if _on_gpu(logits):
        require_native().apply_logit_bias(logits, bias_start, bias_n, bias_tok, bias_val, forced)
        return logits
    ref.apply_logit_bias(logits, bias_start, bias_n, bias_tok, bias_val, forced)
    return logits


def minp_threshold(logits, temperature, min_p, ln_min_p, forced, mask_class, class_masks,
                   tau: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """min_p truncation as a per-row logit threshold (csrc/ops/logit_shaping.hip).

    Row r with min_p[r] > 0, temperature[r] > 0 and forced[r] < 0: m = the largest logit among
    the tokens its mask class allows, tau_mp = fadd_rn(m, fmul_rn(temperature[r], ln_min_p[r]))
    (ln_min_p = float32(ln p), computed by the caller). `tau` = the step's top-k / top-p
    thresholds: updated in place to max(tau, tau_mp), other rows keep their value. Without
    `tau` the result goes to `out` (or a new tensor), other rows get -inf = no truncation, as
    do rows whose mask allows nothing."""
    rows = logits.shape[0]
    has_tau = tau is not None
    if not has_tau:
        tau = out if out is not None else torch.empty(rows, dtype=torch.float32, device=logits.device)
    if _on_gpu(logits):
        require_native().minp_threshold(tau, has_tau, logits, temperature, min_p, ln_min_p, forced,
                                        mask_class, class_masks)
        return tau
    tau[:rows].copy_(ref.minp_threshold(logits, temperature, min_p, ln_min_p, forced, mask_class, class_masks,
                                        tau[:rows] if has_tau else None))
    return tau


COSINE_MAX_Q = 64  # queries per index pass (LDS-resident query tiles)


def cosine_topk(queries, index, n_valid: int, K: int, row_priority, row_tags, row_expiry,
                q_min_priority, q_tags, now: float, workspace: Optional[torch.Tensor] = None):
    if _on_gpu(index):
        C = require_native()
        Q = queries.shape[0]
        out_s = torch.empty(Q, K, dtype=torch.float32, device=index.device)
        out_r = torch.empty(Q, K, dtype=torch.int32, device=index.device)
        qc = min(Q, COSINE_MAX_Q)
        need = C.cosine_topk_workspace_bytes(qc, max(1, int(n_valid)), K)
        if workspace is None or workspace.numel() * workspace.element_size() < need:
            workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=index.device)
        # one pass over the index per <= 64 queries (csrc/ops/similarity.hip)
        for q0 in range(0, Q, COSINE_MAX_Q):
            q1 = min(Q, q0 + COSINE_MAX_Q)
            C.cosine_topk(out_s[q0:q1], out_r[q0:q1], workspace, queries[q0:q1].contiguous(), index,
                          int(n_valid), int(K), row_priority, row_tags, row_expiry,
                          q_min_priority[q0:q1].contiguous(), q_tags[q0:q1].contiguous(), float(now))
        return out_s, out_r
    if index.dim() == 4:  # packed tiles (memory/semantic_index.py) -> row-major for the reference
        index = unpack_decode_weight(index)
    return ref.cosine_topk(queries, index, n_valid, K, row_priority, row_tags, row_expiry,
                           q_min_priority, q_tags, now)


# ---- 16-bit fixed-point index (csrc/ops/similarity_q16.hip; memory/semantic_index.py storage="q16")
Q16_MAX = 32512  # |v| <= 127 * 256: hi = floor((v + 128) / 256) stays in [-127, 127]


def q16_quantize(x: torch.Tensor):
    """Rows of x (any float) -> (hi int8 [n, D], lo int8 [n, D], scale fp32 [n], bound fp32 [n]):
    v = round(x / scale) = 256 hi + lo exactly (|v| <= Q16_MAX, scale = max|x| / Q16_MAX), and
    bound = scale * ||lo||_2 (a hair above: the stage-1 error bound's row factor)."""
    x = x.float()
    m = x.abs().amax(1)
    sc = torch.where(m > 0, m / Q16_MAX, torch.ones_like(m))
    v = torch.round(x / sc[:, None]).clamp_(-Q16_MAX, Q16_MAX)
    hi = torch.floor((v + 128) / 256)
    lo = v - 256 * hi
    bound = (sc.double() * lo.double().norm(dim=1)).float() * (1 + 1e-6)
    return hi.to(torch.int8), lo.to(torch.int8), sc, bound


def q16_pack(plane: torch.Tensor) -> torch.Tensor:
    """int8 [n = 16 T, D] -> fragment-major tiles [T, D/64, 64, 16]: lane 16 g + c of (t, s) holds
    row 16 t + c, dims 64 s + 16 g .. + 16 (the v_mfma_i32_16x16x64_i8 operand)."""
    n, D = plane.shape
    return plane.reshape(n // 16, 16, D // 64, 4, 16).permute(0, 2, 3, 1, 4).reshape(n // 16, D // 64, 64, 16)


def q16_unpack(tiles: torch.Tensor) -> torch.Tensor:
    T, DS = tiles.shape[0], tiles.shape[1]
    return tiles.view(T, DS, 4, 16, 16).permute(0, 3, 1, 2, 4).reshape(T * 16, DS * 64)


def q16_queries(q: torch.Tensor):
    """Queries -> (qv int8 [Q, 2, D] = (qh, ql), qmeta fp32 [Q, 2] = (scale, scale * ||v||_2))."""
    hi, lo, sc, _ = q16_quantize(q)
    v = 256 * hi.double() + lo.double()
    cq = (sc.double() * v.norm(dim=1)).float() * (1 + 1e-6)
    return torch.stack([hi, lo], 1).contiguous(), torch.stack([sc, cq], 1).contiguous()


def q16_topk(queries, hi, lo, rmeta, n_valid: int, K: int, row_priority, row_tags, row_expiry,
             q_min_priority, q_tags, now: float, workspace: Optional[torch.Tensor] = None, exact: bool = False,
             stats: Optional[dict] = None):
    """Exact filtered top-k over a q16 index (scores of the 16-bit fixed-point vectors, the
    same on the GPU and in ops.reference.q16_topk). GPU: the two-stage kernel, hi plane only in
    the streaming pass; a batch whose drop check fails is re-run with the exact scan (counted
    in stats["q16_fallbacks"]). queries: fp32 / bf16 [Q, D] (quantised here)."""
    qv, qm = q16_queries(queries)
    if _on_gpu(hi):
        C = require_native()
        Q = qv.shape[0]
        out_s = torch.empty(Q, K, dtype=torch.float32, device=hi.device)
        out_r = torch.empty(Q, K, dtype=torch.int32, device=hi.device)
        unsafe = torch.zeros(Q, dtype=torch.int32, device=hi.device)
        qc = min(Q, COSINE_MAX_Q)
        need = C.q16_topk_workspace_bytes(qc, max(1, int(n_valid)))
        if workspace is None or workspace.numel() * workspace.element_size() < need:
            workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=hi.device)
        for q0 in range(0, Q, COSINE_MAX_Q):
            q1 = min(Q, q0 + COSINE_MAX_Q)
            C.q16_topk(out_s[q0:q1], out_r[q0:q1], unsafe[q0:q1], workspace, qv[q0:q1], qm[q0:q1], hi, lo, rmeta,
                       int(n_valid), int(K), row_priority, row_tags, row_expiry,
                       q_min_priority[q0:q1].contiguous(), q_tags[q0:q1].contiguous(), float(now), int(exact))
        if not exact and bool(unsafe.any()):  # a slice refused a row that might be in the top-k
            if stats is not None:
                stats["q16_fallbacks"] = stats.get("q16_fallbacks", 0) + 1
            for q0 in range(0, Q, COSINE_MAX_Q):
                q1 = min(Q, q0 + COSINE_MAX_Q)
                C.q16_topk(out_s[q0:q1], out_r[q0:q1], unsafe[q0:q1], workspace, qv[q0:q1], qm[q0:q1], hi, lo,
                           rmeta, int(n_valid), int(K), row_priority, row_tags, row_expiry,
                           q_min_priority[q0:q1].contiguous(), q_tags[q0:q1].contiguous(), float(now), 1)
        return out_s, out_r
    return ref.q16_topk(qv, qm, hi, lo, rmeta, n_valid, K, row_priority, row_tags, row_expiry,
                        q_min_priority, q_tags, now)


MMR_MAX_CANDIDATES = 64  # candidates per query of one mmr_select call (csrc/ops/similarity_mmr.hip)


def mmr_weights(diversity) -> tuple:
    """Per-query MMR weights (wr, wd) = (float32(1 - d), float32(d)), fp32 CPU tensors [Q]."""
    d = torch.as_tensor(diversity, dtype=torch.float64).reshape(-1)
    return (1.0 - d).float(), d.float()


def mmr_select(rows, scores, planes, k: int, wr, wd, out=None):
    """Diversity-aware re-ranking (maximal marginal relevance) of a scan's candidate lists:
    `rows` [Q, m] int32 / `scores` [Q, m] fp32 as cosine_topk / q16_topk return them for K = m
    (best first, rows -1 past the hits, m <= 64), `planes` the index's row storage -- (packed,)
    for bf16, (hi, lo, rmeta) for q16 -- and `wr` / `wd` [Q] fp32 the per-query weights
    (mmr_weights). Returns (scores [Q, k], rows [Q, k]): the greedy picks in selection order with
    their cosine scores, (-inf, -1) past them (semantics: ops.reference.mmr_select). GPU: one
    launch of csrc/ops/similarity_mmr.hip; q16 agrees with the reference bit for bit."""
    planes = tuple(planes)
    if len(planes) not in (1, 3):
        raise ValueError("planes must be (packed,) or (hi, lo, rmeta)")
    Q, m = rows.shape
    k = int(k)
    if not 1 <= m <= MMR_MAX_CANDIDATES or not 1 <= k <= MMR_MAX_CANDIDATES:
        raise ValueError(f"mmr_select takes 1..{MMR_MAX_CANDIDATES} candidates and picks per query, not m={m}, k={k}")
    if _on_gpu(planes[0]):
        C = require_native()
        dev = planes[0].device
        out_s, out_r = out if out is not None else (torch.empty(Q, k, dtype=torch.float32, device=dev),
                                                    torch.empty(Q, k, dtype=torch.int32, device=dev))
        if Q == 0:
            return out_s, out_r
        args = (out_s, out_r, rows.to(dev, torch.int32).contiguous(), scores.to(dev, torch.float32).contiguous())
        w = (torch.as_tensor(wr, dtype=torch.float32).to(dev).contiguous(),
             torch.as_tensor(wd, dtype=torch.float32).to(dev).contiguous())
        if len(planes) == 1:
            C.mmr_select_bf16(*args, planes[0], *w, k)
        else:
            C.mmr_select_q16(*args, *planes, *w, k)
        return out_s, out_r
    out_s = torch.full((Q, k), float("-inf"))
    out_r = torch.full((Q, k), -1, dtype=torch.int32)
    wr = torch.as_tensor(wr, dtype=torch.float32).cpu()
    wd = torch.as_tensor(wd, dtype=torch.float32).cpu()
    for q in range(Q):
        rq = rows[q].cpu()
        sims = ref.q16_pairwise(*planes, rq) if len(planes) == 3 else ref.bf16_pairwise(planes[0], rq)
        out_s[q], out_r[q] = ref.mmr_select(scores[q], rq, sims, k, float(wr[q]), float(wd[q]))
    return out_s, out_r


def record_bytes(dim: int, q16: bool) -> int:
    """Bytes of one exchange record of a stored row (csrc/ops/similarity_mmr_rows.hip)."""
    return 2 * int(dim) + (16 if q16 else 0)


def gather_rows(planes, rows, out=None):
    """Exchange records of stored rows, for MMR re-ranking where the rows' shard is not:
    `planes` the index's row storage -- (packed,) for bf16, (hi, lo, rmeta) for q16 -- and `rows`
    [n] int32 row ids, ANY values (they come from another rank). Returns recs [n, rowbytes]
    uint8: per row its D bf16 values row-major (2 D bytes), or D int8 hi, D int8 lo, the fp32
    scale and 12 zero bytes (2 D + 16); an id that names no row of the planes gives the all-zero
    record. GPU: one launch of csrc/ops/similarity_mmr_rows.hip (gather_rows_kernel)."""
    planes = tuple(planes)
    if len(planes) not in (1, 3):
        raise ValueError("planes must be (packed,) or (hi, lo, rmeta)")
    if not _on_gpu(planes[0]):
        rec = ref.gather_rows(planes, rows)
        if out is not None:
            out.copy_(rec)
            return out
        return rec
    C = require_native()
    dev = planes[0].device
    q16 = len(planes) == 3
    rows = torch.as_tensor(rows).to(dev, torch.int32).reshape(-1).contiguous()
    rb = record_bytes(planes[0].shape[1] * (64 if q16 else 32), q16)
    recs = out if out is not None else torch.empty(rows.shape[0], rb, dtype=torch.uint8, device=dev)
    if rows.shape[0] == 0:
        return recs
    if q16:
        C.gather_rows_q16(recs, rows, *planes)
    else:
        C.gather_rows_bf16(recs, rows, planes[0])
    return recs


def mmr_select_rows(recs, slot, scores, k: int, wr, wd, out=None, q16: Optional[bool] = None):
    """mmr_select over exchange records instead of the index tiles: `recs` [R, rowbytes] uint8
    (gather_rows), `slot` [Q, m] int32 the record of every candidate, best first -- the first entry
    that is negative or >= R ends a list -- `scores` [Q, m] fp32 their cosines, `wr` / `wd` [Q]
    (mmr_weights). Returns (scores [Q, k], pos [Q, k] int32): the greedy picks in selection order
    with their cosine scores and LIST POSITIONS, (-inf, -1) past them. `q16`: the records'
    format; None tells it from rowbytes (2 D + 16 with D a multiple of 64 is q16, 2 D with D a
    multiple of 32 is bf16, and no length is both). GPU: one launch of
    csrc/ops/similarity_mmr_rows.hip (mmr_rows_kernel), the tile kernel's arithmetic."""
    R, rb = recs.shape
    if q16 is None:
        q16 = rb % 64 == 16
    Q, m = slot.shape
    k = int(k)
    if not 1 <= m <= MMR_MAX_CANDIDATES or not 1 <= k <= MMR_MAX_CANDIDATES:
        raise ValueError(f"mmr_select_rows takes 1..{MMR_MAX_CANDIDATES} candidates and picks per query, "
                         f"not m={m}, k={k}")
    if _on_gpu(recs):
        C = require_native()
        dev = recs.device
        out_s, out_p = out if out is not None else (torch.empty(Q, k, dtype=torch.float32, device=dev),
                                                    torch.empty(Q, k, dtype=torch.int32, device=dev))
        if Q == 0:
            return out_s, out_p
        C.mmr_select_rows(out_s, out_p, recs, slot.to(dev, torch.int32).contiguous(),
                          scores.to(dev, torch.float32).contiguous(),
                          torch.as_tensor(wr, dtype=torch.float32).to(dev).contiguous(),
                          torch.as_tensor(wd, dtype=torch.float32).to(dev).contiguous(), k, bool(q16))
        return out_s, out_p
    out_s = torch.full((Q, k), float("-inf"))
    out_p = torch.full((Q, k), -1, dtype=torch.int32)
    wr = torch.as_tensor(wr, dtype=torch.float32).cpu()
    wd = torch.as_tensor(wd, dtype=torch.float32).cpu()
    pair = ref.q16_record_pairwise if q16 else ref.bf16_record_pairwise
    for q in range(Q):
        sq = slot[q].long().cpu()
        bad = ((sq < 0) | (sq >= R)).nonzero().flatten()
        n = int(bad[0]) if len(bad) else m
        pos = torch.full((m,), -1, dtype=torch.int64)
        pos[:n] = torch.arange(n)
        sims = pair(recs, torch.where(pos >= 0, sq, pos))
        out_s[q], out_p[q] = ref.mmr_select(scores[q], pos, sims, k, float(wr[q]), float(wd[q]))
    return out_s, out_p


def skinny_gemm(x: torch.Tensor, w: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = x @ w.T via the weight-streaming MFMA kernel (csrc/ops/gemm_skinny.hip)."""
    y = out if out is not None else torch.empty(x.shape[0], w.shape[0], dtype=x.dtype, device=x.device)
    if not _on_gpu(x):
        y.copy_(torch.nn.functional.linear(x.float(), w.float()).to(y.dtype))
        return y
    if not require_native().skinny_gemm(y, x, w):
        raise ValueError(f"skinny_gemm does not handle M={x.shape[0]} N={w.shape[0]} K={x.shape[1]}")
    return y


# Largest token count at which the skinny kernel beats hipBLASLt, per projection
# kind, measured cache-cold on MI355X with Llama-3-8B shapes
# (tools/gemm_bench.py, profiles/r1_skinny_gemm_cold.md). 0 = never.
SKINNY_MAX_M = {"qkv": 8, "o": 32, "gate_up": 16, "down": 0, "lm_head": 0}


def linear(x: torch.Tensor, w: torch.Tensor, kind: str) -> torch.Tensor:
    """Projection dispatcher: skinny MFMA kernel at decode sizes, hipBLASLt otherwise.

    The choice depends only on the (static) token count, so it is fixed per
    captured hipGraph bucket."""
    M, K = x.shape
    if (_on_gpu(x) and M <= SKINNY_MAX_M.get(kind, 0) and K % 256 == 0 and w.shape[0] % 16 == 0
            and x.is_contiguous()):
        return skinny_gemm(x, w)
    return torch.nn.functional.linear(x, w)


# ---------------------------------------------------------------------------
# Decode-step projections on fragment-major packed weights (csrc/ops/gemm_decode.hip)

DECODE_EPI = {"plain": 0, "silu": 1, "resid": 2}


def pack_decode_weight(w: torch.Tensor) -> torch.Tensor:
    """[N, K] row-major -> [N/16, K/32, 64, 8]: lane l = 16*g + c of tile (t, s)
    holds w[16t + c, 32s + 8g : 32s + 8g + 8] (the MFMA 16x16x32 B fragment)."""
    N, K = w.shape
    if N % 16 or K % 32:
        raise ValueError(f"cannot pack a [{N}, {K}] weight (needs N % 16 == 0, K % 32 == 0)")
    return w.reshape(N // 16, 16, K // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous().view(N // 16, K // 32, 64, 8)


def pack_decode_gate_up(w13: torch.Tensor) -> torch.Tensor:
    """[2F, K] = [gate; up] -> packed tiles interleaved (gate t, up t, gate t+1, ...),
    so one workgroup holds both halves of the same 16 outputs (EPI silu)."""
    F2, K = w13.shape
    F = F2 // 2
    g = pack_decode_weight(w13[:F])
    u = pack_decode_weight(w13[F:])
    return torch.stack([g, u], 1).reshape(F2 // 16, K // 32, 64, 8)


def unpack_decode_weight(wp: torch.Tensor) -> torch.Tensor:
    T, S = wp.shape[0], wp.shape[1]
    return wp.view(T, S, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(T * 16, S * 32)


def unpack_decode_gate_up(wp: torch.Tensor) -> torch.Tensor:
    T, S = wp.shape[0], wp.shape[1]
    pairs = wp.view(T // 2, 2, S, 64, 8)
    return torch.cat([unpack_decode_weight(pairs[:, 0]), unpack_decode_weight(pairs[:, 1])], 0)


def decode_gemm(x: torch.Tensor, wp: torch.Tensor, epi: str = "plain", norm: bool = False,
                eps: float = 1e-5, resid: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None, nt: int = 0, waves: int = 0, splits: int = 0) -> torch.Tensor:
    """y = epi(rownorm(x) @ W.T) for M <= 64 rows with W packed by pack_decode_weight
    (gate_up: pack_decode_gate_up). `norm` scales each row by rsqrt(mean(x^2)+eps)
    (the RMSNorm weight must already be folded into W); epi "silu" returns
    silu(gate)*up [M, F]; epi "resid" returns resid + acc (out may alias resid)."""
    M, K = x.shape
    N = wp.shape[0] * 16
    code = DECODE_EPI[epi]
    NO = N // 2 if code == 1 else N
    if out is None:
        out = torch.empty(M, NO, dtype=x.dtype, device=x.device)
    if _on_gpu(x):
        ws, cnt = decode_workspace(x.device)
        if not require_native().decode_gemm(out, x, wp, resid, code, bool(norm), float(eps), int(nt), int(waves),
                                            int(splits), ws, cnt):
            raise ValueError(f"decode_gemm does not handle M={M} N={N} K={K} epi={epi} nt={nt} waves={waves}")
        return out
    xf = x.float()
    W = unpack_decode_gate_up(wp) if code == 1 else unpack_decode_weight(wp)
    acc = xf @ W.float().T
    if norm:
        acc = acc * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    if code == 1:
        g, u = acc[:, :NO], acc[:, NO:]
        acc = g * torch.sigmoid(g) * u
    elif code == 2:
        acc = acc + resid.float()
    out.copy_(acc.to(out.dtype))
    return out


# per-head tile order of the rope-fused QKV weights: tiles (i, i + 4) adjacent
_ROPE_TILE_ORDER = (0, 4, 1, 5, 2, 6, 3, 7)


def pack_decode_qkv_rope(wqkv: torch.Tensor) -> torch.Tensor:
    """Packed QKV weights for decode_qkv_rope: within every 128-row head the
    16-row tiles are reordered to (0, 4, 1, 5, 2, 6, 3, 7), so one workgroup of
    two tiles holds rotary dims i and i + 64 (csrc/ops/gemm_decode.hip EPI_ROPE)."""
    N, K = wqkv.shape
    if N % 128:
        raise ValueError("QKV rows must be a multiple of the 128-wide head")
    idx = torch.tensor(_ROPE_TILE_ORDER, device=wqkv.device)
    w = wqkv.reshape(N // 128, 8, 16, K).index_select(1, idx).reshape(N, K)
    return pack_decode_weight(w)


def unpack_decode_qkv_rope(wp: torch.Tensor) -> torch.Tensor:
    w = unpack_decode_weight(wp)
    N, K = w.shape
    inv = torch.argsort(torch.tensor(_ROPE_TILE_ORDER)).to(w.device)
    return w.reshape(N // 128, 8, 16, K).index_select(1, inv).reshape(N, K)


def decode_qkv_rope(x: torch.Tensor, wp: torch.Tensor, eps: float, q_out: torch.Tensor, k_cache, v_cache,
                    positions, slots, cos_sin, H: int, KV: int, splits: int = 0) -> torch.Tensor:
    """Decode QKV projection with the RMSNorm folded in (norm weight pre-multiplied
    into the packed weights), RoPE and the paged KV write fused in the epilogue:
    replaces rmsnorm + QKV GEMM + rope_cache on decode-sized steps."""
    if _on_gpu(x):
        ws, cnt = decode_workspace(x.device)
        require_native().decode_qkv_rope(x, wp, float(eps), q_out, k_cache, v_cache, positions, slots,
                                         cos_sin, int(H), int(KV), int(splits), ws, cnt)
        return q_out
    xf = x.float()
    w = unpack_decode_qkv_rope(wp).float()
    qkv = (xf @ w.T) * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    ref.rope_cache(q_out, k_cache, v_cache, qkv.to(x.dtype), positions, slots, cos_sin, H, KV)
    return q_out


# ---------------------------------------------------------------------------
# FP8 (e4m3) copies of the packed decode weights (csrc/ops/gemm_decode_fp8.hip).
# Per output channel a power-of-two scale (reference.quantize_fp8_rows), so q * scale is exact
# in bf16 and the FP8 kernel equals the bf16 kernel on the dequantised weights bit for bit.
# The packed tensors keep the index layout of the bf16 packers with 1-byte elements; the
# scales travel in PACKED column order (the order in which the kernel's tiles hold columns).

quantize_fp8_rows = ref.quantize_fp8_rows
dequantize_fp8_rows = ref.dequantize_fp8_rows
_F8 = torch.float8_e4m3fn


def _quantized(w):
    """(q, scale) from a weight matrix, or a (q, scale) pair passed through."""
    if isinstance(w, (tuple, list)):
        q, s = w
        if q.dtype != _F8:
            raise ValueError(f"quantised weights must be float8_e4m3fn, got {q.dtype}")
        return q, s.float()
    return quantize_fp8_rows(w)


def _u8(f, q, *a):
    # layout ops run on the bytes: not every indexing op exists for float8 tensors
    return f(q.view(torch.uint8), *a).view(_F8)


def pack_decode_weight_fp8(w):
    """[N, K] (or a quantised (q, scale) pair) -> (wp8 [N/16, K/32, 64, 8] e4m3, scale_p [N])."""
    q, s = _quantized(w)
    return _u8(pack_decode_weight, q), s.contiguous()


def pack_decode_gate_up_fp8(w13):
    """[gate; up] -> (wp8 with gate/up tiles interleaved, scale_p interleaved the same way)."""
    q, s = _quantized(w13)
    F2 = q.shape[0]
    if F2 % 32:
        raise ValueError(f"cannot pack a [{F2}, {q.shape[1]}] gate_up weight (needs 2F % 32 == 0)")
    return _u8(pack_decode_gate_up, q), s.view(2, F2 // 32, 16).permute(1, 0, 2).reshape(F2).contiguous()


def pack_decode_qkv_rope_fp8(wqkv):
    """QKV rows -> (wp8 in the per-head rope tile order, scale_p in the same order)."""
    q, s = _quantized(wqkv)
    N = q.shape[0]
    wp8 = _u8(pack_decode_qkv_rope, q)
    idx = torch.tensor(_ROPE_TILE_ORDER, device=s.device)
    return wp8, s.view(N // 128, 8, 16).index_select(1, idx).reshape(N).contiguous()


def unpack_decode_weight_fp8(wp8, scale_p):
    """-> (q [N, K] e4m3, scale [N]) in model row order."""
    return _u8(unpack_decode_weight, wp8), scale_p


def unpack_decode_gate_up_fp8(wp8, scale_p):
    F2 = scale_p.shape[0]
    return _u8(unpack_decode_gate_up, wp8), scale_p.view(F2 // 32, 2, 16).permute(1, 0, 2).reshape(F2)


def unpack_decode_qkv_rope_fp8(wp8, scale_p):
    N = scale_p.shape[0]
    inv = torch.argsort(torch.tensor(_ROPE_TILE_ORDER)).to(scale_p.device)
    return _u8(unpack_decode_qkv_rope, wp8), scale_p.view(N // 128, 8, 16).index_select(1, inv).reshape(N)


def _dequant_packed(wp8, scale_p, dtype=torch.bfloat16):
    """Packed bf16 fragments q * scale from the packed FP8 copy (layout unchanged)."""
    T, S = wp8.shape[0], wp8.shape[1]
    sc = scale_p.float().view(T, 1, 1, 16, 1)
    return (wp8.float().view(T, S, 4, 16, 8) * sc).to(dtype).view(T, S, 64, 8)


def decode_gemm_fp8(x: torch.Tensor, wp8: torch.Tensor, scale_p: torch.Tensor, epi: str = "plain",
                    norm: bool = False, eps: float = 1e-5, resid: Optional[torch.Tensor] = None,
                    out: Optional[torch.Tensor] = None, nt: int = 0, waves: int = 0, splits: int = 0) -> torch.Tensor:
    """decode_gemm on the FP8 packed copy (pack_decode_weight_fp8 / pack_decode_gate_up_fp8):
    equal, bit for bit, to decode_gemm on the bf16 pack of q * scale with the same config."""
    M, K = x.shape
    N = wp8.shape[0] * 16
    code = DECODE_EPI[epi]
    if not _on_gpu(x):
        return decode_gemm(x, _dequant_packed(wp8, scale_p, x.dtype), epi, norm=norm, eps=eps, resid=resid, out=out,
                           nt=nt, waves=waves, splits=splits)
    if out is None:
        out = torch.empty(M, N // 2 if code == 1 else N, dtype=x.dtype, device=x.device)
    ws, cnt = decode_workspace(x.device)
    if not require_native().decode_gemm_fp8(out, x, wp8, scale_p, resid, code, bool(norm), float(eps), int(nt),
                                            int(waves), int(splits), ws, cnt):
        raise ValueError(f"decode_gemm_fp8 does not handle M={M} N={N} K={K} epi={epi} nt={nt} waves={waves}")
    return out


def decode_qkv_rope_fp8(x: torch.Tensor, wp8: torch.Tensor, scale_p: torch.Tensor, eps: float, q_out: torch.Tensor,
                        k_cache, v_cache, positions, slots, cos_sin, H: int, KV: int, splits: int = 0) -> torch.Tensor:
    """decode_qkv_rope on the FP8 packed copy (pack_decode_qkv_rope_fp8)."""
    if _on_gpu(x):
        ws, cnt = decode_workspace(x.device)
        require_native().decode_qkv_rope_fp8(x, wp8, scale_p, float(eps), q_out, k_cache, v_cache, positions, slots,
                                             cos_sin, int(H), int(KV), int(splits), ws, cnt)
        return q_out
    return decode_qkv_rope(x, _dequant_packed(wp8, scale_p, x.dtype), eps, q_out, k_cache, v_cache, positions, slots,
                           cos_sin, H, KV, splits=splits)


# split-K slabs + tickets of the packed decode kernels (decode_gemm / decode_qkv_rope)
DECODE_WS_FLOATS = 8 << 20  # 32 MB of split-K slabs per device
_decode_ws = {}


def decode_workspace(device):
    """(slabs, tickets) for decode_gemm / decode_qkv_rope on `device`; allocate before
    hipGraph capture (the tickets must start zeroed; every launch leaves them zeroed)."""
    key = str(device)
    if key not in _decode_ws:
        _decode_ws[key] = (empty_handoff(DECODE_WS_FLOATS, torch.float32, device),
                           torch.zeros(16384, dtype=torch.int32, device=device))
    return _decode_ws[key]


# ---------------------------------------------------------------------------
# Mid-size projections (48 < M <= 512) on the packed weights (csrc/ops/gemm_mid.hip)

MID_EPI = {"plain": 0, "silu": 1, "resid": 2, "rope_perm": 3}
MID_WS_FLOATS = 16 << 20  # 64 MB of split-K slabs per device
_mid_ws = {}


def mid_workspace(device):
    """(slabs, tickets) for mid_gemm / mid_qkv_rope on `device`; allocate before hipGraph
    capture (the tickets start zeroed and every launch leaves them zeroed)."""
    key = str(device)
    if key not in _mid_ws:
        _mid_ws[key] = (empty_handoff(MID_WS_FLOATS, torch.float32, device),
                        torch.zeros(16384, dtype=torch.int32, device=device))
    return _mid_ws[key]


def _unpack_for(code: int, wp: torch.Tensor) -> torch.Tensor:
    if code == 3:
        return unpack_decode_qkv_rope(wp)
    if code == 1:
        return unpack_decode_gate_up(wp)
    return unpack_decode_weight(wp)


def row_sumsq(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[m] = sum_k x[m, k]^2 in fp32 (RMSNorm row statistics)."""
    out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device) if out is None else out
    if _on_gpu(x):
        require_native().row_sumsq(out, x)
        return out
    out[:x.shape[0]].copy_(x.float().pow(2).sum(-1))
    return out


def mid_gemm(x: torch.Tensor, wp: torch.Tensor, epi: str = "plain", resid: Optional[torch.Tensor] = None,
             out: Optional[torch.Tensor] = None, norm: bool = False, eps: float = 1e-5, fm: int = 0, fn: int = 0,
             splits: int = 0, ss_in: Optional[torch.Tensor] = None, ss_out: Optional[torch.Tensor] = None,
             ss_zero: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = epi(rownorm(x) @ W.T) for mid-size M with W packed by pack_decode_weight (gate_up:
    pack_decode_gate_up + epi "silu"; QKV: pack_decode_qkv_rope + epi "rope_perm", which
    returns the natural column order); "resid": resid + acc (out may alias resid).

    `norm` scales rows by rsqrt(mean(x^2) + eps) (RMSNorm weight folded into W); the row
    statistics are `ss_in` ([M] fp32 sum of x^2, e.g. the `ss_out` of the residual epilogue
    that produced x) or computed here by row_sumsq. `ss_out` (resid only): [M] += row sums
    of the written output squared. `ss_zero`: an [M] buffer zeroed by the launch."""
    M, K = x.shape
    N = wp.shape[0] * 16
    code = MID_EPI[epi]
    NO = N // 2 if code == 1 else N
    if out is None:
        out = torch.empty(M, NO, dtype=x.dtype, device=x.device)
    if norm and ss_in is None:
        ss_in = row_sumsq(x)
    if _on_gpu(x):
        ws, cnt = mid_workspace(x.device)
        if not require_native().mid_gemm(out, x, wp, resid, ws, cnt, code, ss_in if norm else None, ss_out, ss_zero,
                                          float(eps), int(fm), int(fn), int(splits)):
            raise ValueError(f"mid_gemm does not handle M={M} N={N} K={K} epi={epi} fm={fm} fn={fn} S={splits}")
        return out
    W = _unpack_for(code, wp)
    acc = x.float() @ W.float().T
    if norm:
        acc = acc * torch.rsqrt(ss_in[:M].float().unsqueeze(-1) / K + eps)
    if code == 1:
        acc = torch.nn.functional.silu(acc[:, :NO]) * acc[:, NO:]
    elif code == 2:
        acc = acc + resid.float()
    y = acc.to(out.dtype)
    if ss_zero is not None:
        ss_zero[:M].zero_()
    if ss_out is not None:
        ss_out[:M] += y.float().pow(2).sum(-1)
    out.copy_(y)
    return out


# ---------------------------------------------------------------------------
# Weight-streaming projections (16 < M <= 256) on the packed weights (csrc/ops/gemm_stream.hip)

STREAM_EPI = {"plain": 0, "silu": 1, "resid": 2, "rope_perm": 3}
STREAM_WS_FLOATS = 24 << 20  # 96 MB of split-K partial fragments per device (uncached)
_stream_ws = {}
# Split-K group hand-off of gemm_stream.hip (rel bit 0 = the producer's agent-scope release,
# buffer_wbl2 sc1 + drain, before it arrives). Shipped: 0, the form of MI355X_MICROARCH.md's
# measured-valid hand-off table, row 1 (16-B sc1 slab stores drained by every wave, workgroup
# barrier, one lane's agent-scope add; sc1 poll; sc1 slab loads behind a barrier), plus the
# consumer's agent-scope acquire. Round 5 ran 100,000 NaN-poisoned, varied-input repetitions of
# every production plan (the RoPE + paged-KV epilogue included) in both forms: 0 bad runs
# (profiles/r5_handoff_stream.md); the release costs 2.5-5 us per launch (+10-18 %, about +5 %
# on a 64-row step), so it stays an option (PILOTTAI_STREAM_REL=1). The decode / mid / prefill
# last-arriver hand-offs keep their release (they failed without it, profiles/r4_handoff_uncached.md).
STREAM_REL = int(os.environ.get("PILOTTAI_STREAM_REL", "0"))


def stream_workspace(device):
    """(slabs, counters, err) for stream_gemm / stream_qkv_rope on `device`; allocate before
    hipGraph capture. Slabs live in uncached memory (empty_handoff); the group counters start
    zeroed and every launch leaves them zeroed; err[0] != 0 means a group barrier timed out."""
    key = str(device)
    if key not in _stream_ws:
        _stream_ws[key] = (empty_handoff(STREAM_WS_FLOATS, torch.float32, device),
                           torch.zeros(16384, dtype=torch.int32, device=device),
                           torch.zeros(16, dtype=torch.int32, device=device))
    return _stream_ws[key]


def stream_gemm_plan(M: int, N: int, K: int, epi: str = "plain"):
    """Default decomposition (mg, rg, tpw, wt, wk, S, D) of stream_gemm for this shape."""
    code = 4 if epi == "rope_kv" else STREAM_EPI[epi]
    return tuple(require_native().stream_gemm_plan(int(M), int(N), int(K), code)[:7])


def stream_gemm(x: torch.Tensor, wp: torch.Tensor, epi: str = "plain", resid: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None, norm: bool = False, eps: float = 1e-5,
                ss_in: Optional[torch.Tensor] = None, ss_out: Optional[torch.Tensor] = None,
                ss_zero: Optional[torch.Tensor] = None, plan=None, rel: Optional[int] = None,
                stamps: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = epi(rownorm(x) @ W.T) for 16 < M <= 256 with W packed by pack_decode_weight (gate_up:
    pack_decode_gate_up + "silu"; QKV: pack_decode_qkv_rope + "rope_perm"); same epilogue and
    row-statistics conventions as mid_gemm. `plan`: (mg, rg, tpw, wt, wk, S, D) or None for
    the kernel's default decomposition (csrc/ops/gemm_stream.hip).
    rel: bit 0 = producer-side agent-scope release before the group barrier, bit 1 = each
    workgroup streams its K slice from a rotated starting chunk; None = STREAM_REL."""
    M, K = x.shape
    N = wp.shape[0] * 16
    code = STREAM_EPI[epi]
    NO = N // 2 if code == 1 else N
    if out is None:
        out = torch.empty(M, NO, dtype=x.dtype, device=x.device)
    if norm and ss_in is None:
        ss_in = row_sumsq(x)
    if _on_gpu(x):
        ws, cnt, err = stream_workspace(x.device)
        if not require_native().stream_gemm(out, x, wp, resid, ws, cnt, err, code, ss_in if norm else None, ss_out,
                                             ss_zero, float(eps), list(plan) if plan else [],
                                             rel=int(STREAM_REL if rel is None else rel),
                                             stamps=stamps):
            raise ValueError(f"stream_gemm does not handle M={M} N={N} K={K} epi={epi} plan={plan}")
        return out
    return mid_gemm(x, wp, epi, resid=resid, out=out, norm=norm, eps=eps, ss_in=ss_in, ss_out=ss_out,
                    ss_zero=ss_zero)


def stream_qkv_rope(x: torch.Tensor, wp: torch.Tensor, eps: float, q_out: torch.Tensor, k_cache, v_cache,
                    positions, slots, cos_sin, H: int, KV: int, ss_in: Optional[torch.Tensor] = None, plan=None,
                    rel: Optional[int] = None) -> torch.Tensor:
    """QKV projection for 16 < M <= 256 (RMSNorm folded, row statistics ss_in) with RoPE and the
    paged KV write in the epilogue (csrc/ops/gemm_stream.hip, EP_ROPEKV)."""
    if ss_in is None:
        ss_in = row_sumsq(x)
    if _on_gpu(x):
        ws, cnt, err = stream_workspace(x.device)
        if not require_native().stream_gemm(None, x, wp, None, ws, cnt, err, 4, ss_in, None, None, float(eps),
                                             list(plan) if plan else [], q_out, k_cache, v_cache, positions, slots,
                                             cos_sin, int(H), int(KV), int(STREAM_REL if rel is None else rel)):
            raise ValueError(f"stream_qkv_rope does not handle M={x.shape[0]} K={x.shape[1]} plan={plan}")
        return q_out
    return mid_qkv_rope(x, wp, eps, q_out, k_cache, v_cache, positions, slots, cos_sin, H, KV, ss_in=ss_in)


# ---------------------------------------------------------------------------
# Large-M projections (prefill-heavy steps) on the packed weights (csrc/ops/gemm_prefill.hip)

PREFILL_WS_FLOATS = 64 << 20  # 256 MB of split slabs per device (= gemm_prefill.hip kWsFloats)
_prefill_ws = {}


def prefill_workspace(device):
    """(slabs, tickets) for prefill_gemm / prefill_qkv_rope on `device`; allocate before
    hipGraph capture (the tickets start zeroed and every launch leaves them zeroed)."""
    key = str(device)
    if key not in _prefill_ws:
        _prefill_ws[key] = (empty_handoff(PREFILL_WS_FLOATS, torch.float32, device),
                            torch.zeros(16384, dtype=torch.int32, device=device))
    return _prefill_ws[key]


def prefill_gemm(x: torch.Tensor, wp: torch.Tensor, epi: str = "plain", resid: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None, norm: bool = False, eps: float = 1e-5, full: int = -1,
                 splits: int = 0, ss_in: Optional[torch.Tensor] = None, ss_out: Optional[torch.Tensor] = None,
                 ss_zero: Optional[torch.Tensor] = None, bn: int = 0, variant: int = -1) -> torch.Tensor:
    """y = epi(rownorm(x) @ W.T) for large M (256 x `bn` MFMA tiles, bn 128 / 256, 0 = the
    kernel's pick) with W packed by pack_decode_weight; same epilogues and row-statistics
    conventions as mid_gemm. `full` tiles run whole, the rest over `splits` K-slices (-1 / 0:
    the kernel's plan). `variant`: kernel family (3 ping-pong, 1 read-ahead / 3-stage;
    -1 = the process default)."""
    M, K = x.shape
    N = wp.shape[0] * 16
    code = MID_EPI[epi]
    NO = N // 2 if code == 1 else N
    if out is None:
        out = torch.empty(M, NO, dtype=x.dtype, device=x.device)
    if norm and ss_in is None:
        ss_in = row_sumsq(x)
    if _on_gpu(x):
        ws, cnt = prefill_workspace(x.device)
        if not require_native().prefill_gemm(out, x, wp, resid, ws, cnt, code, ss_in if norm else None, ss_out,
                                              ss_zero, float(eps), int(full), int(splits), int(bn), int(variant)):
            raise ValueError(f"prefill_gemm does not handle M={M} N={N} K={K} epi={epi} full={full} S={splits}")
        return out
    return mid_gemm(x, wp, epi, resid=resid, out=out, norm=norm, eps=eps, ss_in=ss_in, ss_out=ss_out,
                    ss_zero=ss_zero)


def prefill_qkv_rope(x: torch.Tensor, wp: torch.Tensor, eps: float, q_out: torch.Tensor, k_cache, v_cache,
                     positions, slots, cos_sin, H: int, KV: int, full: int = -1, splits: int = 0,
                     ss_in: Optional[torch.Tensor] = None, bn: int = 0, variant: int = -1) -> torch.Tensor:
    """Large-M QKV projection (RMSNorm folded, row statistics ss_in) with RoPE and the paged
    KV write in the epilogue (csrc/ops/gemm_prefill.hip EP_ROPEKV)."""
    if ss_in is None:
        ss_in = row_sumsq(x)
    if _on_gpu(x):
        ws, cnt = prefill_workspace(x.device)
        if not require_native().prefill_qkv_rope(x, wp, ss_in, float(eps), q_out, k_cache, v_cache, positions,
                                                  slots, cos_sin, int(H), int(KV), ws, cnt, int(full),
                                                  int(splits), int(bn), int(variant)):
            raise ValueError(f"prefill_qkv_rope does not handle M={x.shape[0]} K={x.shape[1]}")
        return q_out
    return mid_qkv_rope(x, wp, eps, q_out, k_cache, v_cache, positions, slots, cos_sin, H, KV, ss_in=ss_in)


def mid_qkv_rope(x: torch.Tensor, wp: torch.Tensor, eps: float, q_out: torch.Tensor, k_cache, v_cache, positions,
                 slots, cos_sin, H: int, KV: int, fm: int = 0, fn: int = 0, splits: int = 0,
                 ss_in: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Mid-size QKV projection with the RMSNorm folded in (norm weight pre-multiplied into
    the rope-packed weights; row statistics `ss_in`, computed here if absent), RoPE and the
    paged KV write in the epilogue: replaces rmsnorm + QKV GEMM + rope_cache on 49-512-token
    steps."""
    if ss_in is None:
        ss_in = row_sumsq(x)
    if _on_gpu(x):
        ws, cnt = mid_workspace(x.device)
        if not require_native().mid_qkv_rope(x, wp, ss_in, float(eps), q_out, k_cache, v_cache, positions, slots,
                                              cos_sin, int(H), int(KV), ws, cnt, int(fm), int(fn), int(splits)):
            raise ValueError(f"mid_qkv_rope does not handle M={x.shape[0]} K={x.shape[1]} fm={fm} fn={fn}")
        return q_out
    M, K = x.shape
    w = unpack_decode_qkv_rope(wp).float()
    qkv = (x.float() @ w.T) * torch.rsqrt(ss_in[:M].float().unsqueeze(-1) / K + eps)
    ref.rope_cache(q_out, k_cache, v_cache, qkv.to(x.dtype), positions, slots, cos_sin, H, KV)
    return q_out
