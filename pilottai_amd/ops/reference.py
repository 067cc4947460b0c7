"""Plain-PyTorch fp32 reference implementations of every HIP kernel.

They define the semantics the CDNA4 kernels are tested against (GPU numerics
tests compare kernel output with these on the same inputs) and serve as the CPU
execution path for the control-plane tests that run without a GPU. On a GPU box
the native kernels are mandatory (see ops/kernels.py) — these are never a
silent fallback for device tensors.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

# ---------------------------------------------------------------------------
# normalisation / activation
# ---------------------------------------------------------------------------


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    xf = x.float()
    inv = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return ((xf * inv).to(x.dtype).float() * w.float()).to(x.dtype)


def fused_add_rmsnorm(resid: torch.Tensor, x: torch.Tensor, w: torch.Tensor, eps: float):
    """Returns (normed, new_resid); new_resid = bf16(resid + x)."""
    new_resid = (resid.float() + x.float()).to(resid.dtype)
    return rmsnorm(new_resid, w, eps), new_resid


def silu_mul(x: torch.Tensor) -> torch.Tensor:
    F = x.shape[-1] // 2
    g, u = x[..., :F].float(), x[..., F:].float()
    return (torch.nn.functional.silu(g).to(x.dtype).float() * u).to(x.dtype)


# ---------------------------------------------------------------------------
# RoPE + paged KV cache
# ---------------------------------------------------------------------------


def rope_cos_sin(max_pos: int, head_dim: int = 128, theta: float = 500000.0,
                 scaling: Optional[dict] = None) -> torch.Tensor:
    """fp32 [max_pos, head_dim] table: cos in [:, :hd/2], sin in [:, hd/2:].

    `scaling` follows the Llama-3.1 "llama3" rope_scaling dict (factor,
    low_freq_factor, high_freq_factor, original_max_position_embeddings).
    """
    half = head_dim // 2
    inv = 1.0 / (theta ** (torch.arange(0, half, dtype=torch.float64) / half))
    if scaling:
        factor = scaling.get("factor", 8.0)
        lo = scaling.get("low_freq_factor", 1.0)
        hi = scaling.get("high_freq_factor", 4.0)
        old = scaling.get("original_max_position_embeddings", 8192)
        lo_wl, hi_wl = old / lo, old / hi
        wl = 2 * math.pi / inv
        smooth = (old / wl - lo) / (hi - lo)
        scaled = torch.where(wl > lo_wl, inv / factor, inv)
        mid = (wl <= lo_wl) & (wl >= hi_wl)
        scaled = torch.where(mid, (1 - smooth) * inv / factor + smooth * inv, scaled)
        inv = scaled
    pos = torch.arange(max_pos, dtype=torch.float64)
    ang = torch.outer(pos, inv)
    return torch.cat([ang.cos(), ang.sin()], dim=1).float()


def apply_rope(x: torch.Tensor, positions: torch.Tensor, cos_sin: torch.Tensor) -> torch.Tensor:
    """x [T, heads, 128] -> rotated (bf16 rounding as in the kernel)."""
    half = x.shape[-1] // 2
    cs = cos_sin[positions.long()]
    c, s = cs[:, None, :half], cs[:, None, half:]
    x1, x2 = x[..., :half].float(), x[..., half:].float()
    o1 = x1 * c - x2 * s
    o2 = x2 * c + x1 * s
    return torch.cat([o1, o2], dim=-1).to(x.dtype)


def rope_cache(q_out, k_cache, v_cache, qkv, positions, slot_mapping, cos_sin, H, KV,
               apply: bool = True):
    T = qkv.shape[0]
    hd = 128
    q = qkv[:, : H * hd].reshape(T, H, hd)
    k = qkv[:, H * hd:(H + KV) * hd].reshape(T, KV, hd)
    v = qkv[:, (H + KV) * hd:(H + 2 * KV) * hd].reshape(T, KV, hd)
    if apply:
        q = apply_rope(q, positions[:T], cos_sin)
        k = apply_rope(k, positions[:T], cos_sin)
    q_out[:T].copy_(q.reshape(q_out[:T].shape))
    blk = k_cache.shape[3]  # K page: [KV, 128/8, block, 8] (fragment-major)
    for t in range(T):
        slot = int(slot_mapping[t])
        if slot < 0:
            continue
        b, o = divmod(slot, blk)
        k_cache[b, :, :, o, :] = k[t].reshape(KV, hd // 8, 8)
        v_cache[b, :, :, o] = v[t]


def kv_copy(k_cache, v_cache, n_copies, copies):
    """k_cache [layers, blocks, KV, 16, block, 8], v_cache [layers, blocks, KV, 128, block]: the
    first j slots of block `src` go to block `dst` for each of the first n_copies[0] triples."""
    blk = k_cache.shape[4]
    tri = copies.reshape(-1)[: 3 * int(n_copies.reshape(-1)[0])].reshape(-1, 3).tolist()
    for src, dst, j in tri:
        j = min(int(j), blk)
        if j <= 0 or src == dst:
            continue
        k_cache[:, dst, :, :, :j, :] = k_cache[:, src, :, :, :j, :]
        v_cache[:, dst, :, :, :j] = v_cache[:, src, :, :, :j]


def _kv_records(k_cache, stage):
    layers, blocks, KV = k_cache.shape[:3]
    return stage.view(stage.shape[0], layers, 2, KV, -1), blocks


def kv_gather_blocks(k_cache, v_cache, ids, n, stage):
    """stage [records, layers * 2 * KV * 2048]: record i = [layer][K|V][KV][page] of block ids[i]
    for i < n; ids outside [0, blocks) are skipped."""
    rec, blocks = _kv_records(k_cache, stage)
    for i, b in enumerate(ids.reshape(-1)[: int(n)].tolist()):
        if not 0 <= b < blocks:
            continue
        rec[i, :, 0] = k_cache[:, b].reshape(rec.shape[1], rec.shape[3], -1)
        rec[i, :, 1] = v_cache[:, b].reshape(rec.shape[1], rec.shape[3], -1)


def kv_scatter_blocks(k_cache, v_cache, ids, n, stage):
    """The inverse of kv_gather_blocks: record i goes to block ids[i]."""
    rec, blocks = _kv_records(k_cache, stage)
    for i, b in enumerate(ids.reshape(-1)[: int(n)].tolist()):
        if not 0 <= b < blocks:
            continue
        k_cache[:, b] = rec[i, :, 0].reshape(k_cache[:, b].shape)
        v_cache[:, b] = rec[i, :, 1].reshape(v_cache[:, b].shape)


def span_pool(hn, n_seg, segs, pool):
    """hn [T, d] bf16, pool [slots, d] fp32 (updated in place): for each of the first n_seg[0]
    (first_row, n_rows, slot, init) quadruples, the rows are added to the slot's accumulator one by
    one in ascending order, each a round-to-nearest fp32 add of the exactly converted bf16 value,
    starting from +0 (init) or from the accumulator. Segments out of bounds are skipped."""
    x = hn.detach().cpu().float().numpy()
    acc_all = pool.detach().cpu().numpy() if isinstance(pool, torch.Tensor) else pool
    T, slots = x.shape[0], acc_all.shape[0]
    words = segs.detach().cpu().reshape(-1) if isinstance(segs, torch.Tensor) else np.asarray(segs).reshape(-1)
    n = min(int(n_seg.reshape(-1)[0]), len(words) // 4)
    for first, rows, slot, init in np.asarray(words[: 4 * max(0, n)]).reshape(-1, 4).tolist():
        if rows <= 0 or first < 0 or first + rows > T or not 0 <= slot < slots:
            continue
        acc = np.zeros(x.shape[1], np.float32) if init else acc_all[slot].astype(np.float32, copy=True)
        for r in range(first, first + rows):
            acc = acc + x[r]
        acc_all[slot] = acc
    if isinstance(pool, torch.Tensor) and pool.device.type != "cpu":
        pool.copy_(torch.from_numpy(acc_all))
    return pool


def paged_attention(q, k_cache, v_cache, q_start, q_len, ctx_len, block_table, scale):
    """q [T, H, 128]; returns out [T, H, 128] (fp32 math, causal within context)."""
    T, H, hd = q.shape
    KV = k_cache.shape[1]
    G = H // KV
    blk = k_cache.shape[3]
    out = torch.zeros_like(q)
    for s in range(len(q_len)):
        ql, ctx, q0 = int(q_len[s]), int(ctx_len[s]), int(q_start[s])
        if ql <= 0:
            continue
        nb = (ctx + blk - 1) // blk
        blocks = block_table[s, :nb].long()
        K = k_cache[blocks].permute(1, 0, 3, 2, 4).reshape(KV, nb * blk, hd)[:, :ctx].float()
        V = v_cache[blocks].permute(1, 0, 3, 2).reshape(KV, nb * blk, hd)[:, :ctx].float()
        Kh = K.repeat_interleave(G, dim=0)  # [H, ctx, hd]
        Vh = V.repeat_interleave(G, dim=0)
        qs = q[q0:q0 + ql].float().permute(1, 0, 2)  # [H, ql, hd]
        sc = torch.matmul(qs, Kh.transpose(1, 2)) * scale  # [H, ql, ctx]
        pos = torch.arange(ctx - ql, ctx)[:, None]
        keys = torch.arange(ctx)[None, :]
        sc = sc.masked_fill(keys > pos, float("-inf"))
        p = torch.softmax(sc, dim=-1)
        o = torch.matmul(p, Vh)  # [H, ql, hd]
        out[q0:q0 + ql] = o.permute(1, 0, 2).to(q.dtype)
    return out


# ---------------------------------------------------------------------------
# sampling — same counter-based hash as csrc/ops/common.h (uniform01)
# ---------------------------------------------------------------------------

_M32 = np.uint64(0xFFFFFFFF)


def _mix32(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.uint64) & _M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & _M32
    x ^= x >> np.uint64(16)
    return x


def uniform01(seed: int, row_off: int, cols: np.ndarray) -> np.ndarray:
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    lo, hi = seed & 0xFFFFFFFF, seed >> 32
    a = _mix32(np.array([(row_off * 0x9E3779B9 + hi) & 0xFFFFFFFF], dtype=np.uint64))
    h = _mix32(np.uint64(lo) ^ a)
    c = (cols.astype(np.uint64) * np.uint64(0x85EBCA6B) + np.uint64(0x27D4EB2F)) & _M32
    h = _mix32(h ^ c)
    return ((h >> np.uint64(8)).astype(np.float64) + 0.5) * (1.0 / 16777216.0)


def topkp_threshold(logits: torch.Tensor, temperature, top_k, top_p, mask_class, class_masks):
    """Exact top-k / top-p logit threshold per row (fp64 math, sort based).

    Kept set = allowed tokens with logit >= tau; tau is the larger of the k-th
    largest allowed logit and the value at which the descending cumulative
    softmax(logit / T) mass first reaches p. -inf = no truncation."""
    rows, V = logits.shape
    out = torch.full((rows,), float("-inf"), dtype=torch.float32)
    lg = logits.float().cpu().numpy().astype(np.float64)
    cm = class_masks.cpu().numpy().view(np.uint32) if class_masks is not None else None
    for r in range(rows):
        T, k, p = float(temperature[r]), int(top_k[r]), float(top_p[r])
        if T <= 0 or ((k <= 0 or k >= V) and not p < 1.0):
            continue
        vals = lg[r]
        mc = int(mask_class[r])
        if mc >= 0 and cm is not None:
            idx = np.arange(V)
            ok = ((cm[mc][idx >> 5] >> (idx & 31).astype(np.uint32)) & 1).astype(bool)
            vals = vals[ok]
        if vals.size == 0:
            continue
        s = np.sort(vals)[::-1]
        t = -np.inf
        if 0 < k < s.size:
            t = max(t, s[k - 1])
        if p < 1.0:
            w = np.exp((s - s[0]) / T)
            c = np.cumsum(w)
            j = int(np.searchsorted(c, p * c[-1] * (1 - 1e-6)))
            t = max(t, s[min(j, s.size - 1)])
        out[r] = t
    return out


def sample(logits: torch.Tensor, temperature, mask_class, class_masks, seeds, offsets,
           forced=None, vocab_offset: int = 0, return_keys: bool = False, tau=None):
    """Gumbel-max sampling with grammar masks (and optional top-k/p threshold
    tau: logits below it are excluded); returns int32 tokens [rows]."""
    rows, V = logits.shape
    toks = torch.zeros(rows, dtype=torch.int32)
    keys_out = torch.zeros(rows, dtype=torch.float32)
    lg = logits.float().cpu().numpy().astype(np.float64)
    cm = class_masks.cpu().numpy().view(np.uint32) if class_masks is not None else None
    for r in range(rows):
        f = int(forced[r]) if forced is not None else -1
        T = float(temperature[r])
        mc = int(mask_class[r])
        idx = np.arange(V) + vocab_offset
        valid = np.ones(V, dtype=bool)
        if mc >= 0 and cm is not None:
            words = cm[mc][idx >> 5]
            valid = ((words >> (idx & 31).astype(np.uint32)) & 1).astype(bool)
        if T <= 0:
            key = lg[r].copy()
        else:
            key = lg[r] / T
            u = uniform01(int(seeds[r]), int(offsets[r]), idx)
            key = key + (-np.log(-np.log(u)))
        if tau is not None:
            valid &= lg[r] >= float(tau[r])
        key[~valid] = -np.inf
        best = int(np.argmax(key)) if valid.any() else 0
        keys_out[r] = float(key[best]) if valid.any() else float("-inf")
        toks[r] = f if f >= 0 else best + vocab_offset
    return (toks, keys_out) if return_keys else toks


def spec_verify(part_k, part_i, forced, input_ids, logit_rows, run_first, run_len):
    """Final merge of the sampler's partials plus draft verification (csrc/ops/spec_verify.hip),
    plain Python over the rows. part_k fp32 / part_i int32 [rows, nchunk]; the other arguments
    hold at least `rows` int32 entries, input_ids the step's token ids. Returns (tokens,
    accept_len), int32 [rows]:
      tokens[r]     forced[r] if >= 0, else the id of the best partial (larger key, equal keys by
                    smaller id), 0 when that id is 0x7fffffff (no allowed token);
      accept_len[r] for the first row of a run, 1 + the number of leading rows j of the run whose
                    token equals the input id of row j + 1 (input_ids[logit_rows[r + j + 1]]; a
                    logit row outside input_ids ends the count); 0 for the run's other rows.
    A (first, len) pair that is not a valid run containing its row (first outside [0, r], r outside
    the run, the run past `rows`, len < 1) makes the row a run of length 1."""
    pk = part_k.detach().cpu().float().numpy()
    pi = part_i.detach().cpu().numpy()
    rows = pk.shape[0]
    fc = forced.detach().cpu().numpy()
    ids = input_ids.detach().cpu().numpy()
    lr = logit_rows.detach().cpu().numpy()
    rf = run_first.detach().cpu().numpy()
    rl = run_len.detach().cpu().numpy()
    toks = np.zeros(rows, dtype=np.int32)
    for r in range(rows):
        bk, bi = -np.inf, 0x7FFFFFFF
        for c in range(pk.shape[1]):
            k, i = float(pk[r, c]), int(pi[r, c])
            if k > bk or (k == bk and i < bi):
                bk, bi = k, i
        toks[r] = int(fc[r]) if fc[r] >= 0 else (0 if bi == 0x7FFFFFFF else bi)
    acc = np.zeros(rows, dtype=np.int32)
    for r in range(rows):
        first, n = int(rf[r]), int(rl[r])
        if first < 0 or first > r or n < 1 or n > rows - first or r - first >= n:
            first, n = r, 1
        if first != r:
            continue
        a = 0
        while a + 1 < n:
            row = int(lr[r + a + 1])
            if row < 0 or row >= ids.shape[0] or int(ids[row]) != int(toks[r + a]):
                break
            a += 1
        acc[r] = a + 1
    return torch.from_numpy(toks), torch.from_numpy(acc)


def token_logprobs(logits: torch.Tensor, tokens, lp_n, forced, mask_class, class_masks, top: int = 20):
    """Per-token log-probabilities (fp64 math, sort based): log softmax(logits) over the tokens
    the row's mask class allows, at temperature 1.

    Returns (logprob fp32 [rows], top_ids int32 [rows, top], top_lp fp32 [rows, top]). A row
    lists its min(lp_n, top) most likely allowed tokens by descending logit, equal logits by
    smaller id, then id -1 / -inf. Rows with lp_n < 0 keep NaN / -1 / NaN (skipped); rows with
    forced >= 0 give (0.0, [(forced, 0.0)]); a row whose mask allows nothing gives -inf and an
    empty list. A chosen token the mask does not allow has logprob -inf; logits of -inf are
    never listed."""
    rows, V = logits.shape
    out_lp = torch.full((rows,), float("nan"), dtype=torch.float32)
    out_ids = torch.full((rows, top), -1, dtype=torch.int32)
    out_lps = torch.full((rows, top), float("nan"), dtype=torch.float32)
    lg = logits.float().cpu().numpy().astype(np.float64)
    cm = class_masks.cpu().numpy().view(np.uint32) if class_masks is not None else None
    idx = np.arange(V)
    for r in range(rows):
        n = int(lp_n[r])
        if n < 0:
            continue
        n = min(n, top)
        out_lps[r] = float("-inf")
        f = int(forced[r]) if forced is not None else -1
        if f >= 0:
            out_lp[r] = 0.0
            if n > 0:
                out_ids[r, 0] = f
                out_lps[r, 0] = 0.0
            continue
        mc = int(mask_class[r])
        valid = np.ones(V, dtype=bool)
        if mc >= 0 and cm is not None:
            valid = ((cm[mc][idx >> 5] >> (idx & 31).astype(np.uint32)) & 1).astype(bool)
        x = np.where(valid, lg[r], -np.inf)
        mx = x.max()
        if not mx > -np.inf:
            out_lp[r] = float("-inf")
            continue
        lse = mx + np.log(np.exp(x - mx).sum())
        t = int(tokens[r])
        out_lp[r] = float(x[t] - lse) if 0 <= t < V else float("-inf")
        if n > 0:
            order = np.argsort(-x, kind="stable")[:n]  # stable: equal logits keep ascending ids
            order = order[x[order] > -np.inf]
            out_ids[r, :order.size] = torch.from_numpy(order.astype(np.int32))
            out_lps[r, :order.size] = torch.from_numpy((x[order] - lse).astype(np.float32))
    return out_lp, out_ids, out_lps


def bf16_order_keys(logits: torch.Tensor) -> np.ndarray:
    """The 16-bit order key of every logit's bf16 value (int64 array): monotone in the value,
    -0 below +0 (csrc/ops/logprob_common.h bf16_order_key)."""
    b = logits.detach().cpu().to(torch.bfloat16).contiguous().view(torch.int16).numpy().astype(np.int64) & 0xFFFF
    return np.where(b & 0x8000, ~b & 0xFFFF, b | 0x8000)


def score_tokens(logits: torch.Tensor, target, lp_n, top: int = 20):
    """Prompt scoring (fp64 math): per row with target t >= 0, log softmax(logits)[t] over the
    whole vocabulary at temperature 1, the rank of t by the integer rule
        1 + #{ i : key(x[i]) > key(x[t]) or (key(x[i]) == key(x[t]) and i < t) }
    on the bf16 order key, and the min(lp_n, top) most likely tokens in that order.

    Returns (logprob fp32 [rows], rank int32 [rows], top_ids int32 [rows, top], top_lp fp32
    [rows, top]). Rows with target < 0 keep NaN / -1 / -1 / NaN (skipped). A target >= V gives
    (-inf, rank 0); a logit of -inf gives -inf and is never listed; lists end with id -1 / -inf."""
    rows, V = logits.shape
    out_lp = torch.full((rows,), float("nan"), dtype=torch.float32)
    out_rank = torch.full((rows,), -1, dtype=torch.int32)
    out_ids = torch.full((rows, top), -1, dtype=torch.int32)
    out_lps = torch.full((rows, top), float("nan"), dtype=torch.float32)
    lg = logits.detach().cpu().to(torch.bfloat16).float().numpy().astype(np.float64)
    keys = bf16_order_keys(logits)
    idx = np.arange(V)
    for r in range(rows):
        t = int(target[r])
        if t < 0:
            continue
        n = min(max(int(lp_n[r]), 0), top)
        out_lps[r] = float("-inf")
        x, k = lg[r], keys[r]
        out_rank[r] = 1 + int(((k > k[t]) | ((k == k[t]) & (idx < t))).sum()) if t < V else 0
        mx = x.max()
        if not mx > -np.inf:
            out_lp[r] = float("-inf")
            continue
        lse = mx + np.log(np.exp(x - mx).sum())
        out_lp[r] = float(x[t] - lse) if t < V else float("-inf")
        if n > 0:
            order = np.argsort(-k, kind="stable")[:n]  # stable: equal keys keep ascending ids
            order = order[x[order] > -np.inf]
            out_ids[r, :order.size] = torch.from_numpy(order.astype(np.int32))
            out_lps[r, :order.size] = torch.from_numpy((x[order] - lse).astype(np.float32))
    return out_lp, out_rank, out_ids, out_lps


def apply_penalties(logits: torch.Tensor, state, pen_slot, pen_reset, presence, frequency, forced,
                    pair_start, pair_n, pair_tok):
    """Presence / frequency penalties in place on `logits` [rows, V] (see ops.apply_penalties),
    with the device kernel's data flow: the slot's distinct list is walked to clear it, the
    row's new tokens are counted and appended on their first occurrence, and the logits of the
    listed tokens are rewritten in fp32 with one conversion back to the logits' dtype."""
    counts, distinct, n_distinct = state
    rows, V = logits.shape
    slots, cap = distinct.shape
    for r in range(rows):
        s = int(pen_slot[r])
        if s < 0 or s >= slots or int(forced[r]) >= 0:
            continue
        if int(pen_reset[r]) != 0:
            n_old = min(max(int(n_distinct[s]), 0), cap)
            for t in distinct[s, :n_old].tolist():
                if 0 <= t < V:
                    counts[s, t] = 0
            n_distinct[s] = 0
        a0, n_new = int(pair_start[r]), int(pair_n[r])
        if a0 < 0 or n_new < 0 or a0 + n_new > pair_tok.numel():
            n_new = 0
        for t in pair_tok[a0:a0 + n_new].tolist():
            if not 0 <= t < V:
                continue
            if int(counts[s, t]) == 0:
                at = int(n_distinct[s])
                if at < cap:
                    distinct[s, at] = t
                n_distinct[s] = at + 1
            counts[s, t] += 1
        n = min(max(int(n_distinct[s]), 0), cap)
        if n == 0:
            continue
        idx = distinct[s, :n].long()
        idx = idx[(idx >= 0) & (idx < V)]
        c = counts[s, idx]
        idx, c = idx[c > 0], c[c > 0].float()
        a = presence[r].float()
        b = frequency[r].float()
        logits[r, idx] = (logits[r, idx].float() - (a + b * c)).to(logits.dtype)
    return logits


def inv_repetition_penalty(r: float) -> float:
    """float32(1 / r), the form in which a request's repetition penalty divides on the device:
    computed in double precision, rounded once. 1.0 for r = 1 (off)."""
    return float(np.float32(1.0 / np.float64(r)))


def apply_repetition_penalty(logits: torch.Tensor, state, rep_slot, rep_reset, rep_r, rep_inv_r, forced,
                             rep_start, rep_n, rep_tok):
    """Repetition penalty in place on `logits` [rows, V] (see ops.apply_repetition_penalty), with
    the device kernel's data flow: the slot's list is walked to clear its membership words, the
    row's new tokens are appended when their bit flips, and the logits of the listed tokens are
    rewritten with one fp32 product and one conversion back to the logits' dtype."""
    seen, seen_list, n_seen = state
    rows, V = logits.shape
    slots, cap = seen_list.shape
    bits = seen.numpy().view(np.uint32)  # shares the tensor's memory
    for i in range(rows):
        s = int(rep_slot[i])
        if s < 0 or s >= slots or int(forced[i]) >= 0:
            continue
        if int(rep_reset[i]) != 0:
            n_old = min(max(int(n_seen[s]), 0), cap)
            for t in seen_list[s, :n_old].tolist():
                if 0 <= t < V:
                    bits[s, t >> 5] = 0
            n_seen[s] = 0
        a0, n_new = int(rep_start[i]), int(rep_n[i])
        if a0 < 0 or n_new < 0 or a0 + n_new > rep_tok.numel():
            n_new = 0
        for t in rep_tok[a0:a0 + n_new].tolist():
            if not 0 <= t < V:
                continue
            w, b = t >> 5, np.uint32(1 << (t & 31))
            if bits[s, w] & b:
                continue
            bits[s, w] |= b
            at = int(n_seen[s])
            if at < cap:
                seen_list[s, at] = t
            n_seen[s] = at + 1
        n = min(max(int(n_seen[s]), 0), cap)
        if n == 0:
            continue
        idx = seen_list[s, :n].long()
        idx = idx[(idx >= 0) & (idx < V)]
        x = logits[i, idx].float()
        y = torch.where(x > 0, x * rep_inv_r[i].float(), x * rep_r[i].float())  # fp32 products, correctly rounded
        logits[i, idx] = y.to(logits.dtype)
    return logits


def apply_logit_bias(logits: torch.Tensor, bias_start, bias_n, bias_tok, bias_val, forced):
    """logit_bias in place on `logits` [rows, V] (see ops.apply_logit_bias): one fp32 add per
    listed token, one conversion back to the logits' dtype."""
    rows, V = logits.shape
    for r in range(rows):
        n, a0 = int(bias_n[r]), int(bias_start[r])
        if n <= 0 or int(forced[r]) >= 0 or a0 < 0 or a0 + n > bias_tok.numel():
            continue
        idx = bias_tok[a0:a0 + n].long()
        val = bias_val[a0:a0 + n].float()
        ok = (idx >= 0) & (idx < V)
        idx, val = idx[ok], val[ok]
        logits[r, idx] = (logits[r, idx].float() + val).to(logits.dtype)
    return logits


def ln_min_p(p: float) -> float:
    """float32(ln p), the form in which a request's min_p travels to the device: computed in
    double precision, rounded once. 0.0 for p outside (0, 1] (min_p off)."""
    p = float(p)
    return float(np.float32(np.log(np.float64(p)))) if 0.0 < p <= 1.0 else 0.0


def minp_threshold(logits: torch.Tensor, temperature, min_p, ln_min_p, forced, mask_class, class_masks,
                   tau=None):
    """min_p as a logit threshold per row (see ops.minp_threshold): tau_mp = m + T * L with m
    the largest allowed logit, the product and the sum each rounded to float32. Rows with
    min_p <= 0, T <= 0, a forced token or a mask that allows nothing keep `tau` (-inf without
    it); the others get max(tau, tau_mp). Returns fp32 [rows]."""
    rows, V = logits.shape
    out = (tau.detach().cpu().float().clone() if tau is not None
           else torch.full((rows,), float("-inf"), dtype=torch.float32))
    lg = logits.float().cpu().numpy()  # bf16 -> fp32 is exact
    cm = class_masks.cpu().numpy().view(np.uint32) if class_masks is not None else None
    idx = np.arange(V)
    for r in range(rows):
        p, T = float(min_p[r]), float(temperature[r])
        mc = int(mask_class[r])
        if not p > 0.0 or not T > 0.0 or int(forced[r]) >= 0 or (cm is not None and mc >= cm.shape[0]):
            continue
        vals = lg[r]
        if mc >= 0 and cm is not None:
            vals = vals[((cm[mc][idx >> 5] >> (idx & 31).astype(np.uint32)) & 1).astype(bool)]
        if vals.size == 0:
            continue
        m = np.float32(vals.max())
        with np.errstate(invalid="ignore", over="ignore"):
            t_mp = np.float32(m + np.float32(np.float32(T) * np.float32(float(ln_min_p[r]))))
        out[r] = max(float(out[r]), float(t_mp))
    return out


# ---------------------------------------------------------------------------
# semantic index
# ---------------------------------------------------------------------------


def cosine_topk(queries, index, n_valid, K, row_priority, row_tags, row_expiry, q_min_priority,
                q_tags, now):
    """Returns (scores [Q,K] fp32, rows [Q,K] int32), rows -1 past the matches."""
    Q = queries.shape[0]
    sc = queries.float() @ index[:n_valid].float().T  # [Q, N]
    out_s = torch.full((Q, K), float("-inf"))
    out_r = torch.full((Q, K), -1, dtype=torch.int32)
    prio = row_priority[:n_valid].long()
    tags = row_tags[:n_valid].long()
    exp = row_expiry[:n_valid].float()
    alive = (exp == 0) | (exp > now)
    for q in range(Q):
        qt = int(q_tags[q])
        ok = (prio >= int(q_min_priority[q])) & ((tags & qt) == qt) & alive
        s = sc[q].masked_fill(~ok, float("-inf"))
        k = min(K, int(ok.sum()))
        if k == 0:
            continue
        v, i = torch.topk(s, k)
        out_s[q, :k] = v
        out_r[q, :k] = i.int()
    return out_s, out_r


def q16_topk(qv, qmeta, hi, lo, rmeta, n_valid, K, row_priority, row_tags, row_expiry, q_min_priority, q_tags,
             now):
    """Exact top-k over the 16-bit fixed-point index (csrc/ops/similarity_q16.hip semantics):
    score = float32(float64(v_q . v_r) * (float64(s_r) * float64(s_q))) with v = 256 hi + lo,
    the integer dot products exact in int64. qv [Q, 2, D] int8 (qh, ql), qmeta [Q, 2] (s_q, .),
    hi / lo fragment-major int8 tiles, rmeta [N, 2] (s_r, .)."""
    T, DS = hi.shape[0], hi.shape[1]
    unpack = lambda t: t.view(T, DS, 4, 16, 16).permute(0, 3, 1, 2, 4).reshape(T * 16, DS * 64)  # noqa: E731
    n = int(n_valid)
    vr = 256 * unpack(hi)[:n].long().cpu() + unpack(lo)[:n].long().cpu()
    vq = 256 * qv[:, 0].long().cpu() + qv[:, 1].long().cpu()
    dots = vq @ vr.T  # exact int64
    sc = (dots.double() * (rmeta[:n, 0].double().cpu()[None, :] * qmeta[:, 0].double().cpu()[:, None])).float()
    return cosine_topk_from_scores(sc, n, K, row_priority, row_tags, row_expiry, q_min_priority, q_tags, now)


def cosine_topk_from_scores(sc, n_valid, K, row_priority, row_tags, row_expiry, q_min_priority, q_tags, now):
    """The filtered top-k of precomputed scores [Q, n_valid] (the reference kernels' common tail)."""
    Q = sc.shape[0]
    out_s = torch.full((Q, K), float("-inf"))
    out_r = torch.full((Q, K), -1, dtype=torch.int32)
    prio = row_priority[:n_valid].long().cpu()
    tags = row_tags[:n_valid].long().cpu()
    exp = row_expiry[:n_valid].float().cpu()
    alive = (exp == 0) | (exp > now)
    for q in range(Q):
        qt = int(q_tags[q])
        ok = (prio >= int(q_min_priority[q])) & ((tags & qt) == qt) & alive
        s = sc[q].masked_fill(~ok, float("-inf"))
        k = min(K, int(ok.sum()))
        if k == 0:
            continue
        v, i = torch.topk(s, k)
        out_s[q, :k] = v
        out_r[q, :k] = i.int()
    return out_s, out_r


def _tile_rows(plane, rows, groups: int):
    """Row-major [m, D] copy of rows `rows` (>= 0) of a fragment-major plane [T, S, 64, w]
    (lane 16 g + c of (t, s) holds row 16 t + c, dims (4 s + g) w .. + w)."""
    T, S, _, w = plane.shape
    rows = torch.as_tensor(rows).long().to(plane.device)
    return plane.view(T, S, groups, 16, w)[rows // 16, :, :, rows % 16, :].reshape(len(rows), S * groups * w).cpu()


def q16_pairwise(hi, lo, rmeta, rows):
    """s_ij of the listed q16 rows (csrc/ops/similarity_mmr.hip): float32(float64(v_i . v_j) *
    (float64(s_i) * float64(s_j))), v = 256 hi + lo, the dot products exact in int64. `rows` [m]
    (entries < 0: a zero row). Returns [m, m] fp32."""
    rows = torch.as_tensor(rows).long().cpu()
    ok = rows >= 0
    safe = rows.clamp(min=0)
    v = 256 * _tile_rows(hi, safe, 4).long() + _tile_rows(lo, safe, 4).long()
    v = v * ok[:, None].long()
    sc = rmeta[safe.to(rmeta.device), 0].double().cpu() * ok.double()
    return ((v @ v.T).double() * (sc[:, None] * sc[None, :])).float()


def bf16_pairwise(packed, rows):
    """s_ij of the listed bf16 rows: the dot products of the stored rows, in fp64 ([m, m] fp64;
    the kernel accumulates the same products in fp32)."""
    rows = torch.as_tensor(rows).long().cpu()
    ok = rows >= 0
    v = _tile_rows(packed, rows.clamp(min=0), 4).double() * ok[:, None].double()
    return v @ v.T


def gather_rows(planes, rows):
    """Exchange records of stored rows (csrc/ops/similarity_mmr_rows.hip): [n, rowbytes] uint8,
    one row each -- bf16 `planes` = (packed,): the D bf16 values row-major (2 D bytes); q16
    `planes` = (hi, lo, rmeta): D int8 hi, D int8 lo, the fp32 scale and 12 zero bytes. An id
    outside [0, rows held by the planes) gives the all-zero record ("no row")."""
    planes = tuple(planes)
    rows = torch.as_tensor(rows).long().cpu()
    nrows = planes[0].shape[0] * 16 if len(planes) == 1 else min(planes[0].shape[0] * 16, planes[2].shape[0])
    ok = (rows >= 0) & (rows < nrows)
    safe = torch.where(ok, rows, torch.zeros_like(rows))
    if len(planes) == 1:
        rec = _tile_rows(planes[0], safe, 4).contiguous().view(torch.uint8)
    else:
        hi, lo, rmeta = planes
        sc = rmeta[safe.to(rmeta.device), 0].float().cpu().contiguous()
        tail = torch.zeros(len(rows), 16, dtype=torch.uint8)
        tail[:, :4] = sc.view(torch.uint8).view(len(rows), 4)
        rec = torch.cat([_tile_rows(hi, safe, 4).contiguous().view(torch.uint8),
                         _tile_rows(lo, safe, 4).contiguous().view(torch.uint8), tail], 1)
    return rec * ok[:, None].to(torch.uint8)


def q16_record_pairwise(recs, slots):
    """q16_pairwise over exchange records: s_ij of records `slots` [m] of `recs` [R, 2 D + 16]
    uint8 (entries < 0: a zero row). Returns [m, m] fp32."""
    recs = recs.cpu()
    slots = torch.as_tensor(slots).long().cpu()
    D = (recs.shape[1] - 16) // 2
    ok = slots >= 0
    r = recs[slots.clamp(min=0)]
    v = 256 * r[:, :D].contiguous().view(torch.int8).long() + r[:, D:2 * D].contiguous().view(torch.int8).long()
    v = v * ok[:, None].long()
    sc = r[:, 2 * D:2 * D + 4].contiguous().view(torch.float32)[:, 0].double() * ok.double()
    return ((v @ v.T).double() * (sc[:, None] * sc[None, :])).float()


def bf16_record_pairwise(recs, slots):
    """bf16_pairwise over exchange records `recs` [R, 2 D] uint8: [m, m] fp64."""
    recs = recs.cpu()
    slots = torch.as_tensor(slots).long().cpu()
    ok = slots >= 0
    v = recs[slots.clamp(min=0)].contiguous().view(torch.bfloat16).double() * ok[:, None].double()
    return v @ v.T


def mmr_select(scores, rows, sims, k: int, wr, wd):
    """Greedy maximal-marginal-relevance selection for ONE query (csrc/ops/similarity_mmr.hip):
    `scores` / `rows` [m] are the scan's top-m, best first, rows -1 past the hits; `sims` [m, m]
    the candidates' pairwise similarities. Every step picks, among the open candidates, the
    largest float32(float32(wr * rel_i) - float32(wd * M_i)) -- M_i the largest s_ij over the
    picks so far, the subtrahend 0 at the first step -- ties to the smaller position. Returns
    (scores [k] fp32, rows [k] int32): the picks in order with their cosine scores, (-inf, -1)
    past them."""
    rel = np.asarray(torch.as_tensor(scores).float().cpu().numpy(), dtype=np.float32)
    rid = np.asarray(torch.as_tensor(rows).cpu().numpy(), dtype=np.int64)
    S = np.asarray(torch.as_tensor(sims).float().cpu().numpy(), dtype=np.float32)
    wr, wd = np.float32(wr), np.float32(wd)
    bad = np.nonzero(rid < 0)[0]
    n = int(bad[0]) if len(bad) else len(rid)
    out_s = torch.full((k,), float("-inf"))
    out_r = torch.full((k,), -1, dtype=torch.int32)
    t = (wr * rel[:n]).astype(np.float32)
    M = np.zeros(n, dtype=np.float32)
    open_ = np.ones(n, dtype=bool)
    for step in range(min(k, n)):
        u = np.zeros(n, dtype=np.float32) if step == 0 else (wd * M).astype(np.float32)
        v = (t - u).astype(np.float32)
        cand = np.flatnonzero(open_)
        best = int(cand[np.argmax(v[cand])])  # the first of equal maxima: the smaller position
        out_s[step] = float(rel[best])
        out_r[step] = int(rid[best])
        open_[best] = False
        M = S[:n, best].copy() if step == 0 else np.maximum(M, S[:n, best])
    return out_s, out_r


def pack_mask(allowed) -> torch.Tensor:
    """bool [V] -> int32 words, bit i of word i // 32 set iff token i is allowed."""
    a = np.asarray(allowed, dtype=bool)
    pad = (-len(a)) % 32
    if pad:
        a = np.concatenate([a, np.zeros(pad, dtype=bool)])
    return torch.from_numpy(np.packbits(a, bitorder="little").view(np.int32).copy())


# ---------------------------------------------------------------------------
# FP8 (OCP e4m3fn) weight quantisation, per output channel, power-of-two scales
# ---------------------------------------------------------------------------

FP8_MAX = 448.0  # largest finite e4m3fn magnitude


def _pow2_scale(amax: torch.Tensor) -> torch.Tensor:
    """Smallest power of two s with amax <= 448 * s (fp32, exact); 1 where amax == 0."""
    _, e = torch.frexp(amax / FP8_MAX)
    s = torch.ldexp(torch.ones_like(amax), e)
    # frexp's mantissa is in [0.5, 1): s is within one binade of the answer; settle it exactly
    s = torch.where(amax > FP8_MAX * s, s * 2, s)
    s = torch.where(amax <= FP8_MAX / 2 * s, s / 2, s)
    return torch.where(amax > 0, s, torch.ones_like(s))


def quantize_fp8_rows(w: torch.Tensor):
    """[N, K] -> (q [N, K] float8_e4m3fn, scale [N] fp32) with w ~ q * scale[:, None].

    scale_n = 2^ceil(log2(amax_n / 448)) (1 for an all-zero row); q = e4m3fn(w / scale_n),
    round-to-nearest-even, saturating at +-448, so the NaN codes 0x7F / 0xFF never appear.
    A row whose maximum would round DOWN to 224 (amax / scale in (224, 232]) takes the next
    smaller scale instead: its maximum then saturates to 448 * scale / 2, the same value, and
    every smaller element keeps one more bit. With that, max |q| of a non-zero row is always in
    (224, 448] and quantising q * scale again returns the same q and scale.
    q * scale is exactly representable in bf16 (3 mantissa bits times a power of two)."""
    wf = w.float()
    amax = wf.abs().amax(dim=1)
    s = _pow2_scale(amax)
    top = (amax / s).to(torch.float8_e4m3fn).float()  # the row maximum as it would be stored
    s = torch.where((amax > 0) & (top <= FP8_MAX / 2), s / 2, s)
    q = (wf / s[:, None]).clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn)
    return q, s


def dequantize_fp8_rows(q: torch.Tensor, scale: torch.Tensor, dtype=torch.bfloat16) -> torch.Tensor:
    """q * scale per row, exact in bf16."""
    return (q.float() * scale.float()[:, None]).to(dtype)
