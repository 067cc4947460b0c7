"""On-node LLM inference engine (replaces the reference's remote litellm provider,
pilott/engine/llm.py:12-219, with a local Llama-3 on MI355X).

Architecture (one engine per GPU / per TP group, one process per GPU):

    asyncio agents ──submit()──► inbox ──► engine thread ──► native Scheduler (C++)
                                                  │   schedule(): writes the whole step into a
                                                  │   pinned int32 buffer (ids, positions, KV slots,
                                                  │   block tables, attention items, sampling params)
                                                  ▼
                        one H2D copy ─► hipGraph replay of [embed → 32 x layer → LM head → sample]
                                                  │   captured per token bucket (ragged batches of
                                                  │   decode + prefill + grammar jump-forward tokens)
                                                  ▼
                        sampled ids ─► Scheduler.commit(): grammar advance, jump-forward, stops,
                                       prefix-cache registration ─► completion callbacks

The LLM protocol used by agents (generate_response / apredict) lives in
engine/local_llm.py on top of `LLMEngine.submit`.

Tensor parallelism (Llama-3-70B, TP=8 over xGMI): only TP rank 0 (the driver)
owns requests, the scheduler, grammars and the tokenizer. Each step it sends a
7-int header over a gloo group, then broadcasts the step metadata it already
holds on the device (one RCCL broadcast); the other ranks sit in `follow()`,
replay the same hipGraph, and take part in the row-parallel all-reduces and
the vocab-parallel sampling collectives inside it (all-gather of per-shard winners; top-k /
top-p thresholds from all-reduced radix histograms, engine/tp_sampling.py). Their schedulers stay idle, so
nothing on the host has to be kept consistent between ranks.
"""
from __future__ import annotations

import logging
import math
import os
import queue
import sys
from collections import deque
import threading
import time
import weakref
from dataclasses import dataclass, field
from numbers import Integral
from typing import Any, Callable, Dict, List, Mapping, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from pilottai_amd import ops
from pilottai_amd.engine.tp_sampling import tp_topkp_threshold
from pilottai_amd.models.llama import KVCache, LlamaModel, StepMeta, get_config
from pilottai_amd.ops.reference import inv_repetition_penalty as ref_inv_repetition_penalty
from pilottai_amd.ops.reference import ln_min_p as ref_ln_min_p
from pilottai_amd.parallel.comm import TPGroup
from pilottai_amd.utils.tracing import trace_range

from .grammar import MAX_CLASSES, GrammarCompiler
from .tokenizer import Tokenizer, get_tokenizer

log = logging.getLogger("pilottai_amd.engine")

# hipGraph token buckets: a step of T tokens replays the smallest bucket >= T, so
# the spacing bounds the padded (wasted) work: 16-token steps up to 512 (graph padding 1.9 ->
# 1.1 % of step tokens at 64 workers; profiles/r2_buckets16_ab.jsonl), 64 up to 2048
# (prefill-heavy agent steps sit at 400-1000 tokens).
def _unregister_pool(pool: torch.Tensor):
    try:
        torch.cuda.cudart().cudaHostUnregister(pool.data_ptr())
    except Exception:  # interpreter shutdown: the runtime is gone, and the registration with it
        pass


HOST_STAGE_RECORDS = 16  # records of the host tier's device staging buffer (2 MiB each on Llama-3-8B)

DEFAULT_BUCKETS = ([8, 16, 32, 48, 64, 80] + list(range(96, 513, 16)) + list(range(576, 2049, 64))
                   + [3072, 4096, 6144, 8192])


@dataclass
class EngineConfig:
    model: str = "llama-3-8b"
    max_num_seqs: int = 256
    max_num_batched_tokens: int = 2048
    max_prefill_tokens: int = 2048
    max_model_len: int = 8192
    block_size: int = 16
    num_kv_blocks: Optional[int] = None
    kv_cache_gb: Optional[float] = None
    kv_cache_fraction: float = 0.5
    kv_reserve_gb: float = 20.0  # HBM always left outside the KV pool (graphs, activations, workspaces)
    prefix_caching: bool = True
    dedup_inflight_prefix: bool = True  # requests wait for an identical prefix another request is prefilling
    # a request whose prefix another request computes in this very step joins the step and reads
    # those blocks instead of waiting a step for them (scheduler.h same_step_prefix)
    same_step_prefix: bool = os.environ.get("PILOTTAI_PREFIX_SAME_STEP", "1") != "0"
    # a prompt that leaves the cached prefix inside a 16-token block copies the common head of
    # the best cached block instead of computing it (scheduler.h partial_block_reuse; the step
    # graph's first kernel, csrc/ops/kv_copy.hip). TP = 1 only.
    partial_block_reuse: bool = os.environ.get("PILOTTAI_PREFIX_PARTIAL", "1") != "0"
    # host tier under the prefix cache (block_manager.h "Host tier", csrc/ops/kv_pages.hip):
    # evicted full blocks are spilled to this much pinned host memory and copied back when a
    # prompt's hash chain reaches them, instead of being computed again. 0 = off (nothing
    # changes). host_cache_blocks, when given, sets the size in blocks instead (tests);
    # host_cache_step_blocks caps the blocks brought back per step (the rest of the chain is
    # computed). TP = 1 and the plain (not pipelined) loop only; needs prefix_caching.
    host_cache_gb: float = 0.0
    host_cache_blocks: Optional[int] = None
    host_cache_step_blocks: int = 256
    # waiting embedding requests are admitted before waiting generation prompts (scheduler.h)
    embed_first: bool = os.environ.get("PILOTTAI_EMBED_FIRST", "1") != "0"
    split_decode: bool = True
    # > 0: mid / large steps size their decode partitions for about this many (partition, KV
    # head) workgroups (scheduler.h decode_part_target): no split once the decode rows fill a
    # round of 4-wave attention workgroups (2 per CU), equal partitions otherwise; 0 = the
    # 512 / 256-key partitions. 32 / 64 / 128-row steps (ctx 600) 4.10 / 4.87 / 5.54 ->
    # 4.05 / 4.67 / 5.45 ms (profiles/r4_att_mid_options_ab.jsonl); headline bench, same box:
    # 1,024 2 % worse than 512, 384 1 % better (profiles/r4_engine_knobs_ab.jsonl)
    decode_part_target: int = int(os.environ.get("PILOTTAI_DECODE_PART_TARGET", "384"))
    # decode-sized steps on 8-wave attention (scheduler.h small_step_part): the smallest
    # flash-decoding partition they use; 4096 = whole contexts (no merge) up to 4,096 keys
    small_step_part: int = int(os.environ.get("PILOTTAI_SMALL_STEP_PART", "4096"))
    # > 0: decode-sized steps size their partitions for about this many (partition, KV head)
    # 8-wave workgroups (scheduler.h small_step_target); 0 = small_step_part alone. 8-row steps
    # (ctx 600 / 1,200) 3.228 / 3.461 -> 3.172 / 3.331 ms, 16 rows unchanged
    # (profiles/r4_small_step_partitions_ab.jsonl)
    small_step_target: int = int(os.environ.get("PILOTTAI_SMALL_STEP_TARGET", "192"))
    use_graphs: bool = True
    token_buckets: Optional[List[int]] = None
    seed: int = 0
    weights_path: Optional[str] = None
    capture_on_start: bool = True
    token_align: int = 256   # GEMM-friendly step sizes (runtime/scheduler.h); 0 = off
    align_slack: int = 96
    decode_fused: Optional[bool] = None  # packed-weight fused decode path; None = when it fits in HBM
    decode_fused_max_t: Optional[int] = None  # largest step (tokens) on that path; None = model default
    mid_max_t: Optional[int] = None  # largest step on the LDS-DMA tiled mid-size path; None = model default
    # largest step on the fused packed-weight path with the 256 x 256 prefill kernels (above
    # mid_max_t); 0 = such steps take the library (hipBLASLt) path; None = model default
    prefill_max_t: Optional[int] = None
    # keep the row-major projection weights beside the packed ones (None: only when some step can
    # leave the packed-weight path, i.e. prefill_max_t / mid_max_t below max_num_batched_tokens)
    keep_dense: Optional[bool] = None
    # "fp8": the layer projections quantised per output channel to e4m3 with power-of-two scales,
    # one weight set on every kernel route (models/llama.py); fp8_decode: decode-sized steps
    # stream the FP8 packed copy (half the bytes, same bits) instead of the bf16 one
    weight_quant: Optional[str] = None
    fp8_decode: bool = True
    # projections ("qkv", "o", "gate_up", "down") whose PF_CFG prefill-kernel rows also apply to
    # <= 256-token steps (None: model default)
    pf_midrange: Optional[List[str]] = None
    # LlamaModel class-level tunables to override on this engine's model (name -> value),
    # e.g. {"DEC_QKV_MAX_T": 64}; for A/B tools (tools/engine_ab.py)
    model_overrides: Optional[Dict[str, Any]] = None
    att_qcols: int = 128  # prefill attention item width in MFMA columns (128: LDS-staged 4-wave items)
    # ... used only for steps with at least this many prefill tokens (1,024: 1,024-2,048-token steps
    # 1-2 % faster than with 2,048, which most mixed steps never reached; profiles/r2_att_wide_min_ab.jsonl)
    att_wide_min_tokens: int = 1024
    # wide prefill items of at least this many causal keys are split into partitions merged
    # in-kernel (scheduler.h prefill_split_keys); 0 = off, the default: the wide path runs only
    # on steps whose items already fill the chip's 2 x 256 workgroup slots, where a split adds a
    # second round (profiles/r6_attention_split.md: 2,048-token prompt 69.7 -> 97.9 us at 512);
    # on few long items narrow items beat wide + split (cont256x4096: 32.4 vs 55.4 us)
    prefill_split_keys: int = int(os.environ.get("PILOTTAI_PREFILL_SPLIT_KEYS", "0"))
    # attention workgroup width on decode-sized steps (<= the model's DECODE_FUSED_MAX_T
    # tokens): 8 waves stream a whole context per workgroup (the scheduler then skips the
    # flash-decoding split for such steps when they have few rows); None = model default
    att_decode_waves: Optional[int] = None
    reply_tokens: Optional[int] = None  # fixed length of every reply schema's free-text slot (grammar.py)
    # interpreter thread-switch interval while the engine thread runs (sys.setswitchinterval);
    # None = env PILOTTAI_GIL_SWITCH_S or the interpreter default (5 ms)
    gil_switch_interval: Optional[float] = None
    # pipelined steps: step N+1 is scheduled and launched while step N runs;
    # rows sampling in N continue speculatively (runtime/scheduler.h). TP = 1 only.
    async_steps: bool = False
    # start(): gc.freeze() everything alive (model, graphs, tokenizer) so later cyclic
    # collections skip it (a full pass stalled the engine thread 60-85 ms). PROCESS-GLOBAL:
    # frozen objects are never reclaimed by the cycle collector until stop() unfreezes, so it
    # is opt-in, for serving entry points that build one engine (bench.py freezes after its
    # warm-up instead; the HTTP server sets it)
    freeze_heap: bool = False
    # keep every captured hipGraph's node list (torch keep_graph=True) so tools can count its
    # kernels (utils/tracing.py graph_node_counts); costs host memory, off in serving
    keep_graphs: bool = False
    # device slots for presence / frequency penalty counts: min(max_num_seqs, penalty_slots)
    # requests with a non-zero penalty run at once, further ones wait for a slot. The state
    # (slots x vocabulary int32 counts, 33 MB at 64 x 128,256) is allocated on the first such request.
    penalty_slots: int = 64
    # drafts (submit(prediction=, prompt_lookup=)): tokens proposed behind a drafting request's
    # decode row and verified in the same step (runtime/scheduler.h, csrc/ops/spec_verify.hip).
    # 3: with the 8B model's 4 query heads per KV head the 1 + 3-token run is exactly one kv-split
    # attention item; longer runs become narrow prefill items. max_draft_len bounds submit(draft_len=).
    draft_len: int = 3
    max_draft_len: int = 8
    # span pooling (submit(embed=True, spans=[...]); csrc/ops/span_pool.hip): fp32 accumulator rows
    # on the device, one per span of a running span request; further requests wait for free rows.
    # The rows (slots x hidden_size x 4 bytes, 4 MB at 256 x 4,096) are allocated on the first such step.
    embed_span_slots: int = 256
    # True: a step that pools spans runs its mid / prefill route "ordered" (LlamaModel._forward_mid),
    # so that the rows the spans sum, and with them the span means, are the same bits from run to
    # run, eager or replayed; about 10 % of such a step. False: such a step runs the kernels every
    # other step runs; the span sums stay ordered, the rows they read may differ in their last bits.
    embed_span_ordered: bool = True


# TP step header: [op, T, ns, nsamp, bucket, masks_changed, n_copy, truncate, embed]
_OP_STOP, _OP_STEP = 0, 1


@dataclass
class GenerationOutput:
    request_id: int
    token_ids: List[int]
    finish_reason: str
    prompt_tokens: int
    cached_prompt_tokens: int
    completion_tokens: int
    sampled_tokens: int
    forced_tokens: int
    t_arrival: float
    t_first_token: float
    t_finish: float
    _tok: Optional[Tokenizer] = field(default=None, repr=False)
    embedding: Optional[np.ndarray] = field(default=None, repr=False)  # embedding requests: mean final hidden
    # submit(logprobs=n >= 0): per entry of token_ids (logprob of the token, [(token id, logprob)]
    # of the <= n most likely tokens the grammar allowed there, most likely first); natural log
    # of softmax(logits) over the allowed tokens at temperature 1; grammar-forced tokens have 0.0
    logprobs: Optional[List[Tuple[float, List[Tuple[int, float]]]]] = field(default=None, repr=False)
    cumulative_logprob: Optional[float] = None  # sum of the tokens' logprobs (None: not asked)
    # submit(score_from=k): per prompt position k .. len-1 (logprob of the prompt's token there given
    # the tokens before it, its rank in the vocabulary -- 1 = most likely --, [(token id, logprob)] of
    # the <= n most likely tokens); natural log of softmax(logits) over the whole vocabulary at
    # temperature 1. finish_reason is "score", token_ids is empty, cumulative_logprob their sum
    prompt_logprobs: Optional[List[Tuple[float, int, List[Tuple[int, float]]]]] = field(default=None, repr=False)
    # submit(prediction= / prompt_lookup=): tokens of the reply that draft steps took from the
    # prediction or the lookup (confirmed draft tokens, plus a step's own last token when it is the
    # prediction's next one), and proposed draft tokens the sampler did not confirm; 0 otherwise
    accepted_prediction_tokens: int = 0
    rejected_prediction_tokens: int = 0
    # submit(embed=True, spans=[(a, b), ...]): [len(spans), hidden] fp32, row i the mean final-norm
    # hidden state of prompt tokens a_i .. b_i - 1, summed in ascending token order in fp32
    span_embeddings: Optional[np.ndarray] = field(default=None, repr=False)

    @property
    def text(self) -> str:
        return self._tok.decode(self.token_ids) if self._tok else ""

    @property
    def ttft(self) -> float:
        return max(0.0, self.t_first_token - self.t_arrival) if self.t_first_token > 0 else 0.0

    @property
    def latency(self) -> float:
        return max(0.0, self.t_finish - self.t_arrival)


_REASONS = {0: "stop", 1: "length", 2: "abort", 3: "embed", 4: "score"}


@dataclass
class _Request:
    rid: int
    prompt_ids: List[int]
    temperature: float
    max_tokens: int
    seed: int
    ignore_eos: bool
    stop_ids: List[int]
    grammar: Optional[list]
    callback: Callable[[GenerationOutput], None]
    t_arrival: float
    top_k: int = 0
    top_p: float = 1.0
    embed: bool = False
    embed_last: bool = False  # last-token pooling (prefix-cache reuse allowed)
    logprobs: int = -1        # -1 off, 0 the chosen token only, 1..20 with that many alternatives
    presence_penalty: float = 0.0   # OpenAI penalties over the generated tokens, each in [-2, 2]
    frequency_penalty: float = 0.0
    logit_bias: tuple = ()          # ((token id, bias), ...): unique ids, non-zero values in [-100, 100]
    min_p: float = 0.0              # 0 off; else in (0, 1]
    ln_min_p: float = 0.0           # float32(ln min_p), computed once here for host and device
    repetition_penalty: float = 1.0      # 1 off; else in (0, 2]
    inv_repetition_penalty: float = 1.0  # float32(1 / r), computed once here for host and device
    score_from: int = -1                 # -1 off; k: a scoring request over prompt positions k .. len-1
    prediction: tuple = ()               # token ids the reply is expected to repeat (draft source)
    prompt_lookup: bool = False          # n-gram drafts from the request's own tokens
    draft_len: int = 0                   # draft tokens per step; 0 = not a drafting request
    spans: tuple = ()                    # ((a, b), ...) token ranges of an embedding request, sorted by a


class LLMEngine:
    def __init__(self, cfg: Optional[EngineConfig] = None, device=None, tp: Optional[TPGroup] = None,
                 tokenizer: Optional[Tokenizer] = None):
        from pilottai_amd import _runtime

        self._rt = _runtime
        self.cfg = cfg = cfg or EngineConfig()
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() \
                else torch.device("cpu")
        self.device = torch.device(device)
        self.on_gpu = self.device.type == "cuda"
        if self.on_gpu:
            ops.require_native()
            torch.cuda.set_device(self.device)
        self.tp = tp or TPGroup.single()
        self._check_host_cache(cfg, self.tp.size)
        self.tok = tokenizer or get_tokenizer()
        self.grammar = GrammarCompiler(self.tok, reply_tokens=cfg.reply_tokens)
        self.model_cfg = get_config(cfg.model)
        mc = self.model_cfg
        if self.on_gpu:
            from .gemm_tuning import load_tuned_gemms

            self.tuned_gemms = load_tuned_gemms(mc.name, self.tp.size)
        t0 = time.time()
        keep_dense = cfg.keep_dense
        if keep_dense is None and (cfg.prefill_max_t is not None or cfg.mid_max_t is not None):
            lim = max(LlamaModel.MID_MAX_T if cfg.mid_max_t is None else int(cfg.mid_max_t),
                      LlamaModel.PREFILL_MAX_T if cfg.prefill_max_t is None else int(cfg.prefill_max_t))
            keep_dense = True if lim < cfg.max_num_batched_tokens else None
        self.model = LlamaModel(mc, self.device, tp=self.tp, seed=cfg.seed, weights_path=cfg.weights_path,
                                decode_pack=cfg.decode_fused, keep_dense=keep_dense,
                                weight_quant=cfg.weight_quant, fp8_decode=cfg.fp8_decode)
        if cfg.decode_fused_max_t is not None:
            self.model.DECODE_FUSED_MAX_T = int(cfg.decode_fused_max_t)
        if cfg.mid_max_t is not None:
            self.model.MID_MAX_T = int(cfg.mid_max_t)
        if cfg.prefill_max_t is not None:
            self.model.PREFILL_MAX_T = int(cfg.prefill_max_t)
        for k, v in (cfg.model_overrides or {}).items():
            if not hasattr(self.model, k):
                raise ValueError(f"unknown model tunable {k!r}")
            setattr(self.model, k, frozenset(v) if isinstance(getattr(self.model, k), frozenset) else v)
        if cfg.att_decode_waves is not None:
            self.model.ATT_DECODE_WAVES = int(cfg.att_decode_waves)
        if cfg.pf_midrange is not None:
            self.model.PF_MIDRANGE = frozenset(cfg.pf_midrange)
        self.load_time = time.time() - t0
        self.max_model_len = min(cfg.max_model_len, mc.max_position)
        # ---- KV cache sizing (288 GB HBM: the default leaves room for graphs/activations)
        kv_local = self.model.kv_local
        bpb = KVCache.bytes_per_block(mc.num_layers, kv_local, cfg.block_size)
        nb = cfg.num_kv_blocks
        if nb is None:
            if cfg.kv_cache_gb is not None:
                nb = int(cfg.kv_cache_gb * (1 << 30)) // bpb
            elif self.on_gpu:
                free, _total = torch.cuda.mem_get_info(self.device)
                # a fraction of what is free, but never into the reserve: beside a 205 GB
                # memory index (config 4) 15 % of the rest is too little for the graphs
                nb = int(max(0.0, min(free * cfg.kv_cache_fraction, free - cfg.kv_reserve_gb * (1 << 30)))) // bpb
            else:
                nb = 2048
        need_min = (self.max_model_len + cfg.block_size - 1) // cfg.block_size + 1
        nb = max(nb, need_min)
        if self.tp.size > 1:  # block ids travel in the metadata: every rank needs the same pool
            t = torch.tensor([nb], dtype=torch.int64)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MIN, group=self.tp.cpu_group)
            nb = int(t.item())
        self.kv = KVCache(mc.num_layers, nb, kv_local, self.device, block_size=cfg.block_size)
        self.num_kv_blocks = nb
        # ---- host tier: a pinned pool of one record (every layer's K and V pages of a block)
        # per slot, and a small device staging buffer that spills and fills share
        hb = cfg.host_cache_blocks if cfg.host_cache_blocks is not None \
            else int(float(cfg.host_cache_gb) * (1 << 30)) // bpb
        self.host_cache_blocks = int(hb)
        self.kv_block_bytes = bpb
        self._host_pool = self._host_stage = None
        if hb > 0:
            if cfg.block_size != 16:
                raise ValueError("the host KV tier needs block_size 16")
            rec = bpb // 2  # bf16 elements of a record
            self._host_pool = self._pinned_pool(hb, rec)
            self._host_stage = torch.empty(HOST_STAGE_RECORDS, rec, dtype=torch.bfloat16, device=self.device)
        # ---- native scheduler + step buffers
        # the model runs 8-wave decode attention on the fused decode path only, keyed on the
        # graph bucket: the scheduler's whole-context (unsplit) items for small steps must
        # follow the same rule, keyed on the step size -> the largest bucket on that path
        buckets = cfg.token_buckets or DEFAULT_BUCKETS
        self.buckets = sorted({b for b in buckets if b <= cfg.max_num_batched_tokens} |
                              {cfg.max_num_batched_tokens})
        small = [b for b in self.buckets if b <= self.model.DECODE_FUSED_MAX_T]
        # the copy list travels in a region of its own, which TP followers do not receive
        self._partial = bool(cfg.partial_block_reuse) and bool(cfg.prefix_caching) and self.tp.size == 1
        small_step = max(small) if (small and self.model.ATT_DECODE_WAVES == 8 and self.model.decode_packed) else 0
        self.sched = _runtime.Scheduler({
            "num_blocks": nb, "block_size": cfg.block_size, "max_num_seqs": cfg.max_num_seqs,
            "max_num_batched_tokens": cfg.max_num_batched_tokens,
            "max_prefill_tokens": cfg.max_prefill_tokens, "max_model_len": self.max_model_len,
            "gqa_group": self.model.h_local // self.model.kv_local,
            "att_qcols": cfg.att_qcols,
            "att_wide_min_tokens": cfg.att_wide_min_tokens,
            "prefill_split_keys": cfg.prefill_split_keys,
            "prefix_caching": cfg.prefix_caching, "split_decode": cfg.split_decode,
            "dedup_inflight_prefix": cfg.dedup_inflight_prefix,
            "same_step_prefix": bool(cfg.same_step_prefix),
            "partial_block_reuse": self._partial,
            "embed_first": bool(cfg.embed_first),
            "token_align": cfg.token_align, "align_slack": cfg.align_slack,
            "kv_heads": self.model.kv_local,
            "small_step_tokens": small_step,
            "small_step_part": int(cfg.small_step_part) if small_step else 0,
            "small_step_target": int(cfg.small_step_target) if small_step else 0,
            "decode_part_target": int(cfg.decode_part_target),
            "penalty_slots": max(0, min(int(cfg.max_num_seqs), int(cfg.penalty_slots))),
            "embed_span_slots": max(0, int(cfg.embed_span_slots)),
            "host_slots": self.host_cache_blocks, "host_cache_step_blocks": int(cfg.host_cache_step_blocks),
            "eos_ids": list(self.tok.eos_ids)})
        L = self.L = self.sched.layout()
        pin = self.on_gpu
        # pipelined steps: two host-side step descriptions (one being copied / in flight,
        # one being scheduled); the device copy is stream-ordered behind the previous step
        self._async = bool(cfg.async_steps) and self.tp.size == 1
        nbuf = 2 if self._async else 1
        self._host_metas = [torch.zeros(L["span_total"], dtype=torch.int32, pin_memory=pin) for _ in range(nbuf)]
        self._host_meta = self._host_metas[0]
        self._host_ptr = self._host_meta.data_ptr()
        self._host_np = self._host_meta.numpy()
        self._dev_meta = torch.zeros(L["span_total"], dtype=torch.int32, device=self.device) \
            if (self.on_gpu or self._async) else self._host_meta
        # attention tickets: one per (sequence, KV head) for split decode rows, then -- only with
        # prefill_split_keys on -- one per (partial slot, KV head) for split prefill items
        # (csrc/ops/attention.hip prefill_item_wg). Without that room the kernel runs its
        # instantiation with the partition hand-off compiled out (no register spills).
        pf_slots = L["max_items"] if cfg.prefill_split_keys > 0 else 0
        self._att_counters = torch.zeros((L["max_seqs"] + pf_slots) * kv_local, dtype=torch.int32,
                                         device=self.device)
        self._init_views()
        V = mc.vocab_size
        self._mask_words = (V + 31) // 32
        self._class_masks = torch.zeros(MAX_CLASSES, self._mask_words, dtype=torch.int32, device=self.device)
        self._mask_version = -1
        self._sync_masks()
        S = cfg.max_num_seqs
        S4 = (S + 3) & ~3  # the TP winners' all-gather moves 16-byte vectors (custom_ar.hip co_kernel)
        self._sampled_dev = torch.zeros(S4, dtype=torch.int32, device=self.device)
        self._sampled_hosts = [torch.zeros(S, dtype=torch.int32, pin_memory=pin) for _ in range(nbuf)]
        self._sampled_host = self._sampled_hosts[0]
        self._inflight: "deque" = deque()  # launched, not yet committed steps (pipelined mode)
        self._slot = 0
        self._last_done = 0.0
        self._keys_dev = torch.zeros(S4, dtype=torch.float32, device=self.device)
        # TP top-k / top-p: workspace of the HIP phase kernels (engine/tp_sampling.py)
        self._tkp_ws = None
        if self.tp.size > 1 and self.on_gpu:
            from .tp_sampling import tkp_ws_floats

            self._tkp_ws = torch.empty(tkp_ws_floats(S), dtype=torch.float32, device=self.device)
        # embedding requests: per-request pooling rows (+ one row that collects every other
        # token), summed in the step graph, read and cleared when the request finishes
        self._embed_pool = torch.zeros(L["max_seqs"] + 1, mc.hidden_size, dtype=torch.float32, device=self.device)
        self._embed_rows = self._dev_meta[L["embed_rows"]:L["embed_rows"] + L["max_tokens"]]
        # pipelined steps: a stream-ordered snapshot of the pool per step slot, taken right
        # behind the step that pools into it, so the commit reads host memory instead of
        # waiting (.cpu()) for the step queued after it
        self._embed_hosts = [torch.zeros_like(self._embed_pool, device="cpu", pin_memory=self.on_gpu)
                             for _ in range(2)] if self._async else None
        tpw = 16 // (self.model.h_local // self.model.kv_local)
        self._tpw = tpw
        self._max_parts = (self.max_model_len + ops.ATT_PART - 1) // ops.ATT_PART
        max_items = L["max_items"]
        # attention partition partials: written and merged inside one launch -> uncached memory
        self._part_o = ops.empty_handoff(max_items * kv_local * 16 * 128, torch.float32, self.device)
        self._part_ml = ops.empty_handoff(max_items * kv_local * 16 * 2, torch.float32, self.device)
        self._sample_ws = ops.sample_workspace(S, self.model.v_local, self.device) if self.on_gpu else None
        # log-probabilities (submit(logprobs=n)): one 41-word record per sampling row (logprob,
        # 20 ids, 20 logprobs: the scheduler's LogprobRecord), written by ops.token_logprobs
        # behind the sampler in the step graph's logprob variant and copied to the host with the
        # sampled tokens. TP > 1 is refused at submit() (vocab-parallel LM head).
        W = self._rt.Scheduler.LOGPROB_RECORD_WORDS
        assert W == 1 + 2 * ops.LOGPROB_TOP
        self._lp_rec = torch.zeros(S, W, dtype=torch.int32, device=self.device)
        recf = self._lp_rec.view(torch.float32)
        self._lp_out = (recf[:, 0], self._lp_rec[:, 1:1 + ops.LOGPROB_TOP], recf[:, 1 + ops.LOGPROB_TOP:])
        self._lp_hosts = [torch.zeros(S, W, dtype=torch.int32, pin_memory=pin) for _ in range(nbuf)]
        self._lp_ws = ops.token_logprobs_workspace(S, self.model.v_local, self.device) \
            if (self.on_gpu and self.tp.size == 1) else None
        # prompt scoring (submit(score_from=k)): one 42-word record per scoring row (logprob, rank,
        # 20 ids, 20 logprobs: the scheduler's ScoreRecord), written by ops.score_tokens behind the
        # sampler in the step graph's scoring variant and copied to the host with the sampled
        # tokens. TP > 1 is refused at submit().
        W2 = self._rt.Scheduler.SCORE_RECORD_WORDS
        assert W2 == 2 + 2 * ops.LOGPROB_TOP
        self._sc_rec = torch.zeros(S, W2, dtype=torch.int32, device=self.device)
        scf = self._sc_rec.view(torch.float32)
        self._sc_out = (scf[:, 0], self._sc_rec[:, 1], self._sc_rec[:, 2:2 + ops.LOGPROB_TOP],
                        scf[:, 2 + ops.LOGPROB_TOP:])
        self._sc_hosts = [torch.zeros(S, W2, dtype=torch.int32, pin_memory=pin) for _ in range(nbuf)]
        self._sc_ws = ops.score_tokens_workspace(S, self.model.v_local, self.device) \
            if (self.on_gpu and self.tp.size == 1) else None
        self._score_bit = int(self._rt.Scheduler.COUNTS9_SCORE_BIT)
        # draft steps (submit(prediction= / prompt_lookup=)): ops.spec_verify takes the place of the
        # sampler's final merge in the step graph's draft variant and writes, beside the sampled
        # tokens, the acceptance length of every run; both are copied to the host together
        self._spec_bit = int(self._rt.Scheduler.COUNTS9_SPEC_BIT)
        self._accept_dev = torch.zeros(S4, dtype=torch.int32, device=self.device)
        self._accept_hosts = [torch.zeros(S, dtype=torch.int32, pin_memory=pin) for _ in range(nbuf)]
        self._draft_counts: Dict[int, tuple] = {}  # request id -> (proposed, accepted, prediction matched)
        # span pooling (submit(embed=True, spans=)): ops.span_pool runs right behind the whole-prompt
        # pooling in the step graph's span variant, on the same final-norm rows, and adds each
        # listed segment into its span's accumulator row; the rows of a request are read at the
        # commit that finishes it. Allocated on the first step that has a segment.
        self._span_bit = int(self._rt.Scheduler.COUNTS9_SPAN_BIT)
        self._span_pool = None
        self._span_ready: Dict[int, np.ndarray] = {}  # request id -> span means read at its step's commit
        # presence / frequency penalties (submit(presence_penalty=, frequency_penalty=)): per-slot
        # token counts on the device, allocated on the first penalised request; ops.apply_penalties
        # rewrites the logits behind the LM head in the step graph's penalty variant
        self._pen_slots = max(0, min(int(cfg.max_num_seqs), int(cfg.penalty_slots)))
        self._pen_state = None
        # repetition penalty (submit(repetition_penalty=)): the seen set of each slot (the same
        # slot indices, separate arrays), allocated on the first such request;
        # ops.apply_repetition_penalty is the first pass behind the LM head in the step graph's
        # repetition variant
        self._rep_state = None
        # one graph per (token bucket, top-k/top-p pass, embedding pooling); truncating variants
        # are captured on first use, so steps without truncation pay nothing for it. The variant
        # with the log-probability pass has the 4-tuple key (bucket, trunc, embed, True), a step
        # with a penalised row the 5-tuple key (bucket, trunc, embed, lp, True), a step with a
        # logit_bias / min_p row the 6-tuple key (bucket, trunc, embed, lp, pen, True), a step
        # with a repetition-penalty row the 7-tuple key (bucket, trunc, embed, lp, pen, shape, True),
        # a step with scoring rows the 8-tuple key (bucket, trunc, embed, lp, pen, shape, rep, True),
        # a step with draft rows the 9-tuple key (bucket, trunc, embed, lp, pen, shape, rep, score, True),
        # a step with span segments the 10-tuple key (..., score, spec, True).
        self._graphs: Dict[tuple, "torch.cuda.CUDAGraph"] = {}
        self._tau = torch.empty(S, dtype=torch.float32, device=self.device)
        self._graph_pool = None
        self.use_graphs = cfg.use_graphs and self.on_gpu
        if self.use_graphs and self.tp.size > 1 and getattr(self.tp, "custom", None) is None:
            # a TP step graph would capture RCCL collectives; every TP collective of a step
            # (activations, sampling winners, threshold histograms) needs the custom P2P path
            log.warning("TP=%d without the custom P2P collectives: running the steps eagerly", self.tp.size)
            self.use_graphs = False
        self.is_driver = self.tp.rank == 0
        self._tp_header = torch.zeros(9, dtype=torch.int64)
        self._tp_closed = False
        # ---- request plumbing
        self._inbox: "queue.SimpleQueue" = queue.SimpleQueue()
        self._aborts: "queue.SimpleQueue" = queue.SimpleQueue()
        self._wake = threading.Event()
        self._reqs: Dict[int, _Request] = {}
        self._pending_out: list = []  # finished outputs delivered during the next step's GPU time
        self._embed_ready: dict = {}  # pooling slot -> embedding read at its step's commit
        self._next_id = 1
        self._id_lock = threading.Lock()
        self._thread: Optional[threading.Thread] = None
        self._stop = False
        self._err: Optional[BaseException] = None
        self.timings: "deque" = deque(maxlen=1 << 20)  # (ttft_s, tpot_s, output_tokens) per request
        self.stats = {"steps": 0, "tokens": 0, "sampled": 0, "requests": 0, "finished": 0,
                      "embed_requests": 0, "embed_tokens": 0,
                      "busy_s": 0.0, "prefill_tokens": 0, "decode_steps": 0, "graph_replays": 0, "graph_captures": 0,
                      "bucket_tokens": 0, "host_sched_s": 0.0, "host_launch_s": 0.0, "device_wait_s": 0.0,
                      "host_commit_s": 0.0, "host_deliver_s": 0.0, "host_move_s": 0.0}
        self.bucket_hist: Dict[int, list] = {}  # bucket -> [steps, seconds]
        # called on the engine thread right after a step is launched with its token count (the
        # memory batcher co-schedules its index scans with compute-bound steps, memory/batcher.py)
        self._step_listeners: List[Callable[[int], None]] = []
        # custom all-reduce health: its spin-waits give up after ~5 s and set an error word
        # instead of hanging; the word is copied back with every step and checked after the
        # step's synchronize, failing the engine rather than continuing on partial sums
        self._car = getattr(self.tp, "custom", None) if self.tp.size > 1 else None
        # device health words read back with every step (non-blocking, behind the step) and
        # checked after its synchronize: [0] the custom all-reduce's barrier timeout, [1] the
        # weight-streaming GEMM's split-K group-barrier timeout (gemm_stream.hip: a partner
        # workgroup never became resident, so the reduced slabs would be partial)
        self._health_dev = []
        if self._car is not None:
            self._health_dev.append(("custom all-reduce barrier timed out (a TP peer stalled > 5 s): "
                                     "the step's activations are partial", self._car.err))
        if self.on_gpu:
            self._health_dev.append(("weight-streaming GEMM split-K group barrier timed out (a "
                                     "partner workgroup never ran): the step's projections are partial",
                                     ops.stream_workspace(self.device)[2]))
        self._health_host = torch.zeros(max(1, len(self._health_dev)), dtype=torch.int32, pin_memory=pin)
        self._tp_ring = None
        if self.tp.size > 1:
            self._open_tp_ring()
        if self.tp.size > 1:  # ranks reach graph capture together (their init times differ)
            torch.distributed.barrier(group=self.tp.cpu_group)
        # graphs contain the TP collectives, so every rank captures every bucket up front
        if self.use_graphs and (cfg.capture_on_start or self.tp.size > 1):
            self.capture_graphs()

    # ------------------------------------------------------------------ setup
    def _init_views(self):
        L, d = self.L, self._dev_meta
        ms, mb = L["max_seqs"], L["max_blocks"]

        def sl(name, n):
            o = L[name]
            return d[o:o + n]

        self.meta = StepMeta(
            input_ids=sl("input_ids", L["max_tokens"]),
            positions=sl("positions", L["max_tokens"]),
            slots=sl("slots", L["max_tokens"]),
            q_start=sl("q_start", ms), q_len=sl("q_len", ms), ctx_len=sl("ctx_len", ms),
            block_table=sl("block_table", ms * mb).view(ms, mb),
            items=sl("items", 4 * L["max_items"]).view(L["max_items"], 4),
            n_items=sl("n_items", 1),
            att_counters=self._att_counters,
            part_size=sl("part_size", 1),
            logit_rows=sl("logit_rows", ms))
        self._temp = sl("temperature", ms).view(torch.float32)
        self._top_k = sl("top_k", ms)
        self._top_p = sl("top_p", ms).view(torch.float32)
        self._mask_cls = sl("mask_class", ms)
        self._forced = sl("forced", ms)
        self._offsets = sl("offsets", ms)
        self._seeds = sl("seeds", 2 * ms).view(torch.int64)
        self._lp_n = sl("lp_n", ms)
        self._pen_slot = sl("pen_slot", ms)
        self._pen_reset = sl("pen_reset", ms)
        self._pen_presence = sl("pen_presence", ms).view(torch.float32)
        self._pen_frequency = sl("pen_frequency", ms).view(torch.float32)
        self._pair_start = sl("pair_start", ms)
        self._pair_n = sl("pair_n", ms)
        self._pair_tok = sl("pair_tok", L["pair_cap"])
        self._bias_start = sl("bias_start", ms)
        self._bias_n = sl("bias_n", ms)
        self._minp = sl("minp", ms).view(torch.float32)
        self._ln_minp = sl("ln_minp", ms).view(torch.float32)
        self._bias_tok = sl("bias_tok", L["bias_cap"])
        self._bias_val = sl("bias_val", L["bias_cap"]).view(torch.float32)
        self._rep_slot = sl("rep_slot", ms)
        self._rep_reset = sl("rep_reset", ms)
        self._rep_r = sl("rep_r", ms).view(torch.float32)
        self._rep_inv_r = sl("rep_inv_r", ms).view(torch.float32)
        self._rep_start = sl("rep_start", ms)
        self._rep_n = sl("rep_n", ms)
        self._rep_tok = sl("rep_tok", L["rep_cap"])
        self._score_target = sl("score_target", ms)
        self._n_copies = sl("n_copies", 1)
        self._copy_list = sl("copy_list", 3 * ms)
        self._run_first = sl("run_first", ms)
        self._run_len = sl("run_len", ms)
        self._span_n = sl("span_n", 1)
        self._span_segs = sl("span_segs", 4 * L["span_slots"])

    def _sync_masks(self) -> bool:
        reg = self.grammar.reg
        if reg.version == self._mask_version:
            return False
        packed = torch.from_numpy(reg.packed())
        self._class_masks[: packed.shape[0]].copy_(packed.to(self.device))
        self._mask_version = reg.version
        return True

    def _items_for_bucket(self, bucket: int, s_b: int) -> int:
        return min(self.L["max_items"], bucket // (2 * self._tpw) + s_b * (self._max_parts + 1) + 4)

    def _meta_for(self, bucket: int, s_b: int, ns: int) -> StepMeta:
        m = self.meta
        n_it = self._items_for_bucket(bucket, s_b)
        return StepMeta(m.input_ids, m.positions, m.slots, m.q_start, m.q_len, m.ctx_len,
                        m.block_table, m.items[:n_it], m.n_items, m.att_counters, m.logit_rows, num_seqs=ns,
                        part_size=m.part_size)

    def _ensure_pen_state(self):
        """Allocate the penalty slots' device state (engine thread, never inside a capture)."""
        if self._pen_state is None:
            self._pen_state = ops.penalty_state(self._pen_slots, self.model.v_local, self.max_model_len,
                                                self.device)

    def _ensure_rep_state(self):
        """Allocate the slots' seen sets (engine thread, never inside a capture)."""
        if self._rep_state is None:
            self._rep_state = ops.repetition_state(self._pen_slots, self.model.v_local, self.max_model_len,
                                                   self.device)

    def _ensure_span_state(self):
        """Allocate the span accumulator rows (engine thread, never inside a capture). Never
        cleared: a span's first segment starts its row from zero."""
        if self._span_pool is None:
            self._span_pool = torch.zeros(max(1, self.L["span_slots"]), self.model_cfg.hidden_size,
                                          dtype=torch.float32, device=self.device)

    def _forward_and_sample(self, bucket: int, s_b: int, ns: int, trunc: bool = False, embed: bool = False,
                            lp: bool = False, pen: bool = False, shape: bool = False, rep: bool = False,
                            score: bool = False, spec: bool = False, span: bool = False):
        meta = self._meta_for(bucket, s_b, ns)
        if self._partial:
            # partial-block prefix hits: the cached heads go into the new blocks before any layer
            # writes or reads KV (a step without copies: the kernel reads a zero count and exits)
            ops.kv_copy(self.kv.k, self.kv.v, self._n_copies, self._copy_list)
        if self._async:  # pending tokens of rows that sampled in the previous step
            ops.patch_pending_ids(meta.input_ids[:bucket], self._sampled_dev)
        pooling = (self._embed_rows, self._embed_pool) if embed else None
        if span:  # span steps pool: the segments are rows of embedding requests (capture_graphs)
            pooling = pooling + ((self._span_n, self._span_segs, self._span_pool, bool(self.cfg.embed_span_ordered)),)
        logits = self.model.forward(meta, self.kv, bucket, s_b, self._part_o, self._part_ml, embed=pooling)
        if rep:
            # on the raw logits, before the additive penalties and everything else
            ops.apply_repetition_penalty(logits, self._rep_state, self._rep_slot[:s_b], self._rep_reset[:s_b],
                                         self._rep_r[:s_b], self._rep_inv_r[:s_b], self._forced[:s_b],
                                         self._rep_start[:s_b], self._rep_n[:s_b], self._rep_tok)
        if pen:
            # before anything reads the logits: the threshold, the sampler and the logprob pass
            # all see the penalised distribution
            ops.apply_penalties(logits, self._pen_state, self._pen_slot[:s_b],
                                self._pen_reset[:s_b], self._pen_presence[:s_b], self._pen_frequency[:s_b],
                                self._forced[:s_b], self._pair_start[:s_b], self._pair_n[:s_b], self._pair_tok)
        if shape:
            # logit_bias behind the penalties: the grammar mask, the thresholds, the sampler and
            # the logprob pass all see the biased logits
            ops.apply_logit_bias(logits, self._bias_start[:s_b], self._bias_n[:s_b], self._bias_tok,
                                 self._bias_val, self._forced[:s_b])
        tau = None
        if trunc:
            # exact top-k / top-p threshold on the full vocabulary; under TP from all-reduced
            # per-shard radix histograms (engine/tp_sampling.py), not an all-gather of the logits
            if self.tp.size == 1:
                tau = ops.topkp_threshold(logits, self.model_cfg.vocab_size, self._temp[:s_b], self._top_k[:s_b],
                                          self._top_p[:s_b], self._mask_cls[:s_b], self._class_masks,
                                          out=self._tau[:s_b])
            else:
                tau = tp_topkp_threshold(logits, self.model.vocab_offset, self.model_cfg.vocab_size,
                                         self._temp[:s_b], self._top_k[:s_b], self._top_p[:s_b],
                                         self._mask_cls[:s_b], self._class_masks, self.tp, out=self._tau[:s_b],
                                         ws=self._tkp_ws)
        if shape:
            # min_p: raises the row's threshold to the larger of the two (the intersection of
            # the kept sets); without a top-k / top-p pass it writes every row's tau
            tau = ops.minp_threshold(logits, self._temp[:s_b], self._minp[:s_b], self._ln_minp[:s_b],
                                     self._forced[:s_b], self._mask_cls[:s_b], self._class_masks,
                                     tau=tau, out=self._tau[:s_b])
        if spec:
            # a draft step (TP = 1): the sampler's chunk pass, then one launch that merges the
            # partials like the sampler's final kernel and checks every run's draft against them
            pk, pi = ops.sample_partials(logits, self._temp[:s_b], self._mask_cls[:s_b], self._class_masks,
                                         self._seeds[:s_b], self._offsets[:s_b], workspace=self._sample_ws,
                                         tau=tau)
            ops.spec_verify(pk, pi, self._forced[:s_b], self.meta.input_ids, self.meta.logit_rows[:s_b],
                            self._run_first[:s_b], self._run_len[:s_b], out_tokens=self._sampled_dev[:s_b],
                            accept_len=self._accept_dev[:s_b])
        elif self.tp.size == 1:
            ops.sample(logits, self._temp[:s_b], self._mask_cls[:s_b], self._class_masks,
                       self._seeds[:s_b], self._offsets[:s_b], self._forced[:s_b],
                       out=self._sampled_dev[:s_b], workspace=self._sample_ws, tau=tau)
        else:
            # vocab-parallel: local winners + keys, all-gather, global argmax (identical
            # to the TP=1 token because the Gumbel noise is keyed on the global index)
            ops.sample(logits, self._temp[:s_b], self._mask_cls[:s_b], self._class_masks,
                       self._seeds[:s_b], self._offsets[:s_b], self._forced[:s_b],
                       out=self._sampled_dev[:s_b], workspace=self._sample_ws,
                       vocab_offset=self.model.vocab_offset, out_keys=self._keys_dev[:s_b], tau=tau)
            s4 = (s_b + 3) & ~3  # whole 16-byte vectors for the custom all-gather
            keys = self.tp.all_gather(self._keys_dev[:s4])[:, :s_b]        # [tp, s_b]
            toks = self.tp.all_gather(self._sampled_dev[:s4])[:, :s_b]     # [tp, s_b]
            best = keys.argmax(0, keepdim=True)
            self._sampled_dev[:s_b].copy_(toks.gather(0, best).squeeze(0))
        if lp:
            o_lp, o_ids, o_lps = self._lp_out
            ops.token_logprobs(logits, self._sampled_dev[:s_b], self._lp_n[:s_b], self._forced[:s_b],
                               self._mask_cls[:s_b], self._class_masks,
                               out=(o_lp[:s_b], o_ids[:s_b], o_lps[:s_b]), workspace=self._lp_ws)
        if score:
            # on the logits as every other pass of the step left them: scoring rows are forced, so
            # no penalty / bias pass touched theirs, and no grammar mask applies
            s_lp, s_rank, s_ids, s_lps = self._sc_out
            ops.score_tokens(logits, self._score_target[:s_b], self._lp_n[:s_b],
                             out=(s_lp[:s_b], s_rank[:s_b], s_ids[:s_b], s_lps[:s_b]), workspace=self._sc_ws)

    @staticmethod
    def _graph_key(bucket: int, trunc: bool, embed: bool, lp: bool = False, pen: bool = False,
                   shape: bool = False, rep: bool = False, score: bool = False, spec: bool = False,
                   span: bool = False) -> tuple:
        if span:
            return (bucket, trunc, embed, lp, pen, shape, rep, score, spec, True)
        if spec:
            return (bucket, trunc, embed, lp, pen, shape, rep, score, True)
        if score:
            return (bucket, trunc, embed, lp, pen, shape, rep, True)
        if rep:
            return (bucket, trunc, embed, lp, pen, shape, True)
        if shape:
            return (bucket, trunc, embed, lp, pen, True)
        if pen:
            return (bucket, trunc, embed, lp, True)
        return (bucket, trunc, embed, True) if lp else (bucket, trunc, embed)

    def _run(self, bucket: int, ns: int, trunc: bool, n_copy: int, embed: bool = False, lp: bool = False,
             pen: bool = False, shape: bool = False, rep: bool = False, score: bool = False,
             spec: bool = False, span: bool = False):
        """Replay the (bucket, trunc, embed[, logprobs[, penalties[, shaping[, repetition[, scoring[, drafts[, spans]]]]]]]) graph
        — capturing it first if needed — or run eagerly."""
        if pen:
            self._ensure_pen_state()
        if rep:
            self._ensure_rep_state()
        if span:
            self._ensure_span_state()
        if not self.use_graphs:
            self._forward_and_sample(bucket, self._seq_bucket(bucket), ns, trunc, embed, lp, pen, shape, rep,
                                     score, spec, span)
            return
        key = self._graph_key(bucket, trunc, embed, lp, pen, shape, rep, score, spec, span)
        g = self._graphs.get(key)
        if g is None:
            # the regions of shaped / repetition / scoring rows, the copy list, the runs and the
            # span segments lie behind the copied prefix: keep the whole buffer
            n_copy = self.L["span_total"]
            saved = self._dev_meta[:n_copy].clone()
            pool = self._embed_pool.clone()
            samp = self._sampled_dev.clone()  # the previous step's tokens (pipelined mode)
            self.capture_graphs([bucket], trunc=trunc, embed=embed, lp=lp, pen=pen,
                                shape=shape, rep=rep, score=score, spec=spec, span=span)  # clobbers the device metadata
            self.stats["graph_captures"] += 1  # a first-use capture inside serving (tens of ms)
            self._dev_meta[:n_copy].copy_(saved)
            self._embed_pool.copy_(pool)
            self._sampled_dev.copy_(samp)
            g = self._graphs[key]
        g.replay()
        self.stats["graph_replays"] += 1

    def _copy_shaping(self, hm: torch.Tensor, n_bias: int):
        """Host -> device copy of the logit_bias / min_p regions of a step with a shaped row: the
        per-row words and the `n_bias` bias tokens in one piece, the bias values in a second."""
        L = self.L
        a, b = L["bias_start"], L["bias_tok"] + n_bias
        self._dev_meta[a:b].copy_(hm[a:b], non_blocking=self.on_gpu)
        if n_bias:
            a = L["bias_val"]
            self._dev_meta[a:a + n_bias].copy_(hm[a:a + n_bias], non_blocking=self.on_gpu)

    def _copy_scoring(self, hm: torch.Tensor):
        """Host -> device copy of the scoring region of a step with scoring rows (the per-row targets)."""
        a, b = self.L["score_target"], self.L["score_target"] + self.L["max_seqs"]
        self._dev_meta[a:b].copy_(hm[a:b], non_blocking=self.on_gpu)

    def _copy_runs(self, hm: torch.Tensor):
        """Host -> device copy of the run regions of a draft step (run_first and run_len, adjacent)."""
        a, b = self.L["run_first"], self.L["run_len"] + self.L["max_seqs"]
        self._dev_meta[a:b].copy_(hm[a:b], non_blocking=self.on_gpu)

    def _copy_spans(self, hm: torch.Tensor):
        """Host -> device copy of the span region of a step with segments: the count and the
        quadruples in use, one piece."""
        a = self.L["span_n"]
        b = self.L["span_segs"] + 4 * int(hm[a])
        self._dev_meta[a:b].copy_(hm[a:b], non_blocking=self.on_gpu)

    def _copy_copies(self, hm: torch.Tensor, n: int):
        """Host -> device copy of the `n` partial-block copy triples of a step that has some (the
        count itself lies in the header every step copies)."""
        a = self.L["copy_list"]
        self._dev_meta[a:a + 3 * n].copy_(hm[a:a + 3 * n], non_blocking=self.on_gpu)

    def _copy_repetition(self, hm: torch.Tensor, n_tok: int):
        """Host -> device copy of the repetition regions of a step with such a row: the per-row
        words and the `n_tok` token words in use, one piece."""
        a, b = self.L["rep_slot"], self.L["rep_tok"] + n_tok
        self._dev_meta[a:b].copy_(hm[a:b], non_blocking=self.on_gpu)

    def _seq_bucket(self, bucket: int) -> int:
        return min(bucket, self.cfg.max_num_seqs)

    def _dummy_meta(self):
        """A metadata state under which a forward touches no KV and no attention item."""
        L = self.L
        # n_copies = 0: the copy kernel touches nothing; span_n = 0: nor does the span pass
        d = torch.zeros(L["span_total"], dtype=torch.int32)
        d[L["slots"]:L["slots"] + L["max_tokens"]] = -1
        d[L["embed_rows"]:L["embed_rows"] + L["max_tokens"]] = L["max_seqs"]
        d[L["pen_slot"]:L["pen_slot"] + L["max_seqs"]] = -1  # the penalty pass touches nothing
        # bias_n = 0 and min_p = 0 (the zeros above): the logit_bias / min_p passes touch nothing
        d[L["rep_slot"]:L["rep_slot"] + L["max_seqs"]] = -1  # the repetition pass touches nothing
        d[L["score_target"]:L["score_target"] + L["max_seqs"]] = -1  # the scoring pass touches nothing
        d[L["run_first"]:L["run_first"] + L["max_seqs"]] = torch.arange(L["max_seqs"], dtype=torch.int32)
        d[L["run_len"]:L["run_len"] + L["max_seqs"]] = 1  # every row a run of its own
        self._dev_meta.copy_(d.to(self.device))

    def capture_embed_graphs(self):
        """Capture every bucket's embedding-pooling variant now (before start()), so embedding
        requests never pay a first-use capture (tens of ms each) while serving."""
        if self._thread is not None:
            raise RuntimeError("capture_embed_graphs() runs before start()")
        self.capture_graphs(embed=True)

    def capture_graphs(self, buckets: Optional[Sequence[int]] = None, trunc: bool = False, embed: bool = False,
                       lp: bool = False, pen: bool = False, shape: bool = False, rep: bool = False,
                       score: bool = False, spec: bool = False, span: bool = False):
        """Capture one hipGraph per token bucket (shared memory pool); the top-k/top-p,
        embedding-pooling, log-probability, penalty, logit_bias / min_p (`shape`), repetition
        penalty (`rep`), prompt-scoring (`score`), draft (`spec`) and span-pooling (`span`) variants are captured on
        first use, or up front by a call with the flag set. `span` implies `embed`: a step with
        span segments always pools, so span=True alone captures the variant such a step replays."""
        if not self.use_graphs:
            return
        embed = embed or span
        if pen:
            self._ensure_pen_state()
        if rep:
            self._ensure_rep_state()
        if span:
            self._ensure_span_state()
        self._dummy_meta()
        if self._graph_pool is None:
            self._graph_pool = torch.cuda.graph_pool_handle()
        t0 = time.time()
        for b in sorted(buckets or self.buckets, reverse=True):
            key = self._graph_key(b, trunc, embed, lp, pen, shape, rep, score, spec, span)
            if key in self._graphs:
                continue
            s_b = self._seq_bucket(b)
            st = torch.cuda.Stream(device=self.device)
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                for _ in range(2):
                    self._forward_and_sample(b, s_b, 0, trunc, embed, lp, pen, shape, rep, score, spec, span)
            torch.cuda.current_stream().wait_stream(st)
            g = torch.cuda.CUDAGraph(keep_graph=True) if self.cfg.keep_graphs else torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=self._graph_pool):
                self._forward_and_sample(b, s_b, 0, trunc, embed, lp, pen, shape, rep, score, spec, span)
            if self.cfg.keep_graphs:
                g.instantiate()
            self._graphs[key] = g
        if embed:
            self._embed_pool.zero_()  # the capture's dummy steps pooled into row max_seqs only
        torch.cuda.synchronize()
        log.info("captured %d hipGraphs in %.1fs", len(self._graphs), time.time() - t0)

    # ------------------------------------------------------------------ API
    def new_request_id(self) -> int:
        with self._id_lock:
            rid = self._next_id
            self._next_id += 1
            return rid

    @staticmethod
    def check_logit_bias(logit_bias, vocab_size: Optional[int] = None) -> tuple:
        """Validate a `logit_bias` mapping (None = empty) and return it as ((id, bias), ...) sorted
        by id with the zero entries dropped; ValueError for anything outside the rules."""
        if logit_bias is None:
            return ()
        if not isinstance(logit_bias, Mapping):
            raise ValueError("logit_bias must be a mapping of token id to bias")
        if len(logit_bias) > ops.LOGIT_BIAS_MAX:
            raise ValueError(f"logit_bias takes at most {ops.LOGIT_BIAS_MAX} entries, not {len(logit_bias)}")
        out = {}
        for t, b in logit_bias.items():
            if isinstance(t, bool) or not isinstance(t, Integral) or t < 0 or (vocab_size is not None and t >= vocab_size):
                raise ValueError(f"logit_bias token id {t!r} is not an integer in [0, vocab_size)")
            if isinstance(b, bool) or not isinstance(b, (int, float)) or not -100.0 <= b <= 100.0:  # NaN fails too
                raise ValueError(f"logit_bias[{t}] must be a finite number in [-100, 100], not {b!r}")
            if b != 0:
                out[int(t)] = float(b)
        return tuple(sorted(out.items()))

    @staticmethod
    def check_min_p(min_p) -> float:
        """Validate `min_p` (None = 0 = off): a finite number in [0, 1], else ValueError."""
        v = 0.0 if min_p is None else min_p
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 <= v <= 1.0:  # NaN fails too
            raise ValueError(f"min_p must be a number in [0, 1], not {v!r}")
        return float(v)

    @staticmethod
    def check_repetition_penalty(repetition_penalty) -> float:
        """Validate `repetition_penalty` (None = 1 = off): a finite number in (0, 2], else ValueError."""
        v = 1.0 if repetition_penalty is None else repetition_penalty
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 < v <= 2.0:  # NaN fails too
            raise ValueError(f"repetition_penalty must be a number in (0, 2], not {v!r}")
        return float(v)

    def submit(self, prompt_ids: Sequence[int], callback: Callable[[GenerationOutput], None], *,
               temperature: float = 0.7, max_tokens: int = 256, seed: Optional[int] = None,
               ignore_eos: bool = False, stop_ids: Sequence[int] = (), grammar: Optional[list] = None,
               request_id: Optional[int] = None, top_k: int = 0, top_p: float = 1.0,
               embed: Union[bool, str] = False, logprobs: int = -1, presence_penalty: float = 0.0,
               frequency_penalty: float = 0.0, logit_bias: Optional[Mapping[int, float]] = None,
               min_p: float = 0.0, repetition_penalty: float = 1.0, score_from: Optional[int] = None,
               prediction: Sequence[int] = (), prompt_lookup: bool = False,
               draft_len: Optional[int] = None, spans: Optional[Sequence[Tuple[int, int]]] = None) -> int:
        """Thread-safe; `callback` runs on the engine thread when the request finishes.

        top_k > 0 / top_p < 1 truncate the (grammar-masked) distribution before
        sampling (exact threshold kernel, csrc/ops/sampling.hip). embed=True (or "mean"): an
        embedding request — the prompt is prefilled in the continuous batch (no prefix-cache
        reuse), nothing is sampled, and the output carries the mean final-norm hidden state.
        embed="last": the final-norm hidden state of the prompt's last token; since a token's
        state depends only on its prefix, such requests reuse cached prefix blocks (shared
        task text across an agent's lookups is computed once).

        logprobs = n: -1 off; 0..20: the output carries, per generated token, its log-probability
        and the n most likely alternatives (GenerationOutput.logprobs) under softmax(logits) over
        the tokens the grammar allowed, at temperature 1 -- whatever temperature / top_k / top_p
        the token was sampled with. Not for embedding requests, not on a TP > 1 engine.

        presence_penalty a / frequency_penalty b, each in [-2, 2] (OpenAI semantics): at every
        sampling step, before the grammar mask, top-k / top-p, the sampler and the logprob pass,
        logit[t] -= a * [c_t > 0] + b * c_t with c_t the occurrences of t among the request's
        generated tokens so far (sampled and grammar-forced; the prompt is not counted). Both 0:
        the request is exactly what it is without them. Not for embedding requests, not on a
        TP > 1 engine, not with async_steps.

        logit_bias {token id: b}, at most 300 entries, ids in [0, vocab_size), b finite in
        [-100, 100] (zero entries are dropped): at every sampling step, behind the penalties and
        before everything else, logit[t] <- bf16(float(logit[t]) + b). The grammar mask still
        applies, so a biased token the grammar does not allow stays impossible; logprobs are those
        of the biased distribution. min_p p in [0, 1] (0 off): at temperature T > 0 the row keeps
        the allowed tokens with logit >= m + T * float32(ln p), m the largest allowed logit (i.e.
        probability >= p * the largest), intersected with top_k / top_p; greedy rows and logprobs
        ignore it. Both are stateless on the device: they work with async_steps and across
        preemption. An empty bias with min_p = 0 is exactly the request without them. Not for
        embedding requests, not on a TP > 1 engine.

        repetition_penalty r in (0, 2] (1 off), the HF / vLLM rule with 1 / r rounded once to
        float32: at every sampling step, on the raw logits before the additive penalties, every
        token t that occurs in the prompt (whatever part of it the prefix cache served) or among
        the tokens generated so far (sampled and grammar-forced) gets logit[t] <- bf16(x > 0 ?
        x * float32(1 / r) : x * r), x = float(logit[t]); a row whose token the grammar forces is
        not touched. Greedy rows are penalised, logprobs are those of the penalised distribution.
        The request holds a penalty slot (shared with its additive penalties); its tokens do not
        depend on what it is batched with and survive preemption. Not for embedding requests, not
        on a TP > 1 engine, not with async_steps.

        score_from = k, 1 <= k <= len(prompt_ids) - 1: a scoring request. Nothing is generated;
        for every prompt position p in [k, len) the output's prompt_logprobs carries the
        log-probability of prompt_ids[p] given the tokens before it (softmax over the whole
        vocabulary at temperature 1, no grammar mask), its rank in the vocabulary (1 = most likely;
        larger logit first, equal logits by smaller id, on the bf16 logits) and the `logprobs` = n
        (0..20, default 0) most likely tokens there. finish_reason is "score", token_ids is empty,
        cumulative_logprob the sum. Positions before k - 1 may come from the prefix cache and the
        request's blocks are cached like any other's, so K candidates over one context pay for the
        context once. temperature, top_k, top_p, seed and max_tokens are ignored; embed, a grammar,
        any penalty, logit_bias, min_p and repetition_penalty are refused, as is a TP > 1 engine.

        prediction (token ids the reply is expected to repeat: OpenAI's Predicted Outputs) and
        prompt_lookup (n-gram drafts from the request's own prompt and reply) make a drafting
        request: when its decode row is planned, up to draft_len (None: EngineConfig.draft_len;
        0 = off; at most EngineConfig.max_draft_len) tokens are proposed behind it and run in the
        same step, one sampling row each, and the device keeps the tokens up to the first row
        whose sample differs from its draft token (csrc/ops/spec_verify.hip). The sampler's noise
        is keyed on (seed, position, vocab index), so every emitted token is the token a plain
        step samples at that position from the same logits: no rejection sampling, greedy and
        sampled alike. The prediction is followed by a cursor that resyncs on the last 4 / 3 / 2
        tokens after a mismatch; prompt lookup runs when the prediction proposes nothing
        (runtime/scheduler.cpp propose). Works with grammars, temperature / top_k / top_p / seed,
        logit_bias and min_p; the output carries accepted_prediction_tokens /
        rejected_prediction_tokens. A draft never preempts a request and never takes a sampling
        row from a plain decode row. draft_len without a prediction or prompt_lookup changes
        nothing. Refused: prediction ids outside the vocabulary, draft_len outside
        [0, max_draft_len], logprobs, any penalty, score_from, embed, a TP > 1 engine, async_steps.

        spans = [(a, b), ...] on an embed=True request: token ranges of the prompt, 0 <= a < b <=
        len(prompt_ids), sorted by a, overlap allowed, at most EngineConfig.embed_span_slots. Beside
        the whole-prompt `embedding` the output carries span_embeddings [len(spans), hidden] fp32:
        row i is the mean final-norm hidden state of tokens a_i .. b_i - 1 of this prompt -- each
        token has seen the whole prompt before it, so one prefill yields a document vector and all
        of its chunk vectors. The bf16 rows of a span are added one by one in ascending token
        order into an fp32 accumulator that starts at +0 (csrc/ops/span_pool.hip) and the sum is
        divided by b - a once on the host: the bits do not depend on how the prompt was cut into
        prefill chunks, on what it was batched with, or on the run. Refused: malformed spans, a
        prompt of max_model_len tokens or more, spans without embed or with embed="last", a TP > 1
        engine, async_steps (the pipelined loop reads pooling rows from per-step host snapshots,
        which hold no span rows)."""
        if self._err is not None:
            raise RuntimeError(f"engine failed: {self._err!r}")
        span_list = self._check_spans(spans, prompt_ids, embed, score_from)
        pred, n_draft = self._check_drafts(prediction, prompt_lookup, draft_len)
        if n_draft and score_from is not None:
            raise ValueError("prediction / prompt_lookup are not available on a scoring request")
        if score_from is not None:
            return self._submit_score(prompt_ids, callback, score_from, logprobs, request_id,
                                      dict(embed=embed, grammar=grammar, presence_penalty=presence_penalty,
                                           frequency_penalty=frequency_penalty, logit_bias=logit_bias,
                                           min_p=min_p, repetition_penalty=repetition_penalty))
        logprobs = -1 if logprobs is None else int(logprobs)
        if not -1 <= logprobs <= ops.LOGPROB_TOP:
            raise ValueError(f"logprobs must be -1 (off) or 0..{ops.LOGPROB_TOP}, not {logprobs}")
        if logprobs >= 0 and embed:
            raise ValueError("logprobs are not available on embedding requests")
        if logprobs >= 0 and self.tp.size > 1:
            raise ValueError("logprobs are not supported on a tensor-parallel (TP > 1) engine")
        pens = []
        for name, v in (("presence_penalty", presence_penalty), ("frequency_penalty", frequency_penalty)):
            v = 0.0 if v is None else v
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not -2.0 <= v <= 2.0:  # NaN fails too
                raise ValueError(f"{name} must be a number in [-2, 2], not {v!r}")
            pens.append(float(v))
        if pens[0] != 0.0 or pens[1] != 0.0:
            if embed:
                raise ValueError("penalties are not available on embedding requests")
            if self.tp.size > 1:
                raise ValueError("penalties are not supported on a tensor-parallel (TP > 1) engine")
            if self.cfg.async_steps:
                raise ValueError("penalties are not supported on an async_steps engine")
            if self._pen_slots < 1:
                raise ValueError("penalties need EngineConfig.penalty_slots >= 1")
        bias = self.check_logit_bias(logit_bias, self.model_cfg.vocab_size)
        min_p = self.check_min_p(min_p)
        if bias or min_p > 0.0:
            if embed:
                raise ValueError("logit_bias / min_p are not available on embedding requests")
            if self.tp.size > 1:
                raise ValueError("logit_bias / min_p are not supported on a tensor-parallel (TP > 1) engine")
        rep_r = self.check_repetition_penalty(repetition_penalty)
        if rep_r != 1.0:
            if embed:
                raise ValueError("repetition_penalty is not available on embedding requests")
            if self.tp.size > 1:
                raise ValueError("repetition_penalty is not supported on a tensor-parallel (TP > 1) engine")
            if self.cfg.async_steps:
                raise ValueError("repetition_penalty is not supported on an async_steps engine")
            if self._pen_slots < 1:
                raise ValueError("repetition_penalty needs EngineConfig.penalty_slots >= 1")
        if n_draft:
            if embed:
                raise ValueError("prediction / prompt_lookup are not available on embedding requests")
            if logprobs >= 0:
                raise ValueError("prediction / prompt_lookup are not supported together with logprobs")
            if pens[0] != 0.0 or pens[1] != 0.0 or rep_r != 1.0:
                raise ValueError("prediction / prompt_lookup are not supported together with presence_penalty, "
                                 "frequency_penalty or repetition_penalty (their device state is kept per "
                                 "committed token)")
        rid = request_id if request_id is not None else self.new_request_id()
        if seed is None:
            seed = (self.cfg.seed * 0x9E3779B1 + rid * 0x85EBCA77) & 0x7FFFFFFFFFFFFFFF
        req = _Request(rid, list(prompt_ids), float(temperature), int(max_tokens), int(seed),
                       bool(ignore_eos), list(stop_ids), grammar, callback, self._rt.now(),
                       int(top_k or 0), float(1.0 if top_p is None else top_p), bool(embed), embed == "last",
                       logprobs, pens[0], pens[1], bias, min_p, ref_ln_min_p(min_p), rep_r,
                       ref_inv_repetition_penalty(rep_r), prediction=pred if n_draft else (),
                       prompt_lookup=bool(prompt_lookup) and n_draft > 0, draft_len=n_draft, spans=span_list)
        self._inbox.put(req)
        self._wake.set()
        return rid

    def _check_spans(self, spans, prompt_ids, embed, score_from) -> tuple:
        """Validate submit()'s `spans` (None or empty: none): ((a, b), ...); ValueError for anything
        outside the rules."""
        if spans is None or len(spans) == 0:
            return ()
        if embed is not True and embed != "mean":
            raise ValueError("spans need embed=True" if not embed or score_from is not None
                             else 'spans are mean-pooled: embed="last" is not supported with them')
        if score_from is not None:
            raise ValueError("spans are not available on a scoring request")
        if self.tp.size > 1:
            raise ValueError("spans are not supported on a tensor-parallel (TP > 1) engine")
        if self.cfg.async_steps:
            raise ValueError("spans are not supported on an async_steps engine")
        n, slots = len(prompt_ids), int(self.L["span_slots"])
        if n >= self.max_model_len:
            raise ValueError(f"spans: {n} tokens do not fit max_model_len {self.max_model_len}")
        if len(spans) > slots:
            raise ValueError(f"spans: at most embed_span_slots = {slots} per request, not {len(spans)}")
        out, prev = [], 0
        for sp in spans:
            try:
                a, b = sp
            except (TypeError, ValueError):
                raise ValueError(f"spans: {sp!r} is not an (a, b) pair") from None
            if any(isinstance(v, bool) or not isinstance(v, Integral) for v in (a, b)) or not 0 <= a < b <= n:
                raise ValueError(f"spans: {sp!r} is not a range 0 <= a < b <= {n} of integers")
            if a < prev:
                raise ValueError("spans must be sorted by their first token")
            prev = a
            out.append((int(a), int(b)))
        return tuple(out)

    def _check_drafts(self, prediction, prompt_lookup, draft_len) -> Tuple[tuple, int]:
        """Validate submit()'s draft arguments: (prediction ids, draft tokens per step -- 0 when the
        request has no draft source or drafts are off); ValueError for anything outside the rules."""
        K = self.cfg.draft_len if draft_len is None else draft_len
        if isinstance(K, bool) or not isinstance(K, Integral) or not 0 <= K <= self.cfg.max_draft_len:
            raise ValueError(f"draft_len must be an integer in [0, {self.cfg.max_draft_len}], not {K!r}")
        if K > self._rt.Scheduler.MAX_DRAFT_LEN:
            raise ValueError(f"draft_len {K} exceeds the scheduler's limit {self._rt.Scheduler.MAX_DRAFT_LEN}")
        pred = () if prediction is None else tuple(prediction)
        V = self.model_cfg.vocab_size
        for t in pred:
            if isinstance(t, bool) or not isinstance(t, Integral) or not 0 <= t < V:
                raise ValueError(f"prediction token id {t!r} is not an integer in [0, {V})")
        if not pred and not prompt_lookup:
            return (), 0
        if self.tp.size > 1:
            raise ValueError("prediction / prompt_lookup are not supported on a tensor-parallel (TP > 1) engine")
        if self.cfg.async_steps:
            raise ValueError("prediction / prompt_lookup are not supported on an async_steps engine")
        return tuple(int(t) for t in pred), int(K)

    def _submit_score(self, prompt_ids, callback, score_from, logprobs, request_id, others) -> int:
        """submit(score_from=k): validate and queue a scoring request."""
        ids = list(prompt_ids)
        k = score_from
        if isinstance(k, bool) or not isinstance(k, Integral) or not 1 <= k <= len(ids) - 1:
            raise ValueError(f"score_from must be an integer in [1, len(prompt_ids) - 1], not {k!r}")
        V = self.model_cfg.vocab_size
        for t in ids:
            if isinstance(t, bool) or not isinstance(t, Integral) or not 0 <= t < V:
                raise ValueError(f"scoring request: token id {t!r} is not an integer in [0, {V})")
        if len(ids) >= self.max_model_len:
            raise ValueError(f"scoring request: {len(ids)} tokens do not fit max_model_len {self.max_model_len}")
        n = 0 if logprobs is None or int(logprobs) == -1 else int(logprobs)
        if not 0 <= n <= ops.LOGPROB_TOP:
            raise ValueError(f"logprobs must be 0..{ops.LOGPROB_TOP} on a scoring request, not {logprobs}")
        if others["embed"]:
            raise ValueError("a scoring request cannot be an embedding request")
        if others["grammar"] is not None:
            raise ValueError("scoring under a grammar is not supported")
        for name, off in (("presence_penalty", 0.0), ("frequency_penalty", 0.0), ("min_p", 0.0),
                          ("repetition_penalty", 1.0)):
            v = others[name]
            if v is not None and v != off:
                raise ValueError(f"{name} is not available on a scoring request")
        if others["logit_bias"]:
            raise ValueError("logit_bias is not available on a scoring request")
        if self.tp.size > 1:
            raise ValueError("scoring is not supported on a tensor-parallel (TP > 1) engine")
        rid = request_id if request_id is not None else self.new_request_id()
        req = _Request(rid, [int(t) for t in ids], 0.0, 1, 0, True, [], None, callback, self._rt.now(),
                       logprobs=n, score_from=int(k))
        self._inbox.put(req)
        self._wake.set()
        return rid

    def score(self, context_ids: Sequence[int], candidates_ids: Sequence[Sequence[int]],
              top: int = 0) -> List[GenerationOutput]:
        """Score each candidate continuation of one context: one scoring request per candidate,
        context + candidate with score_from = len(context), so output i carries the logprob, rank
        and `top` alternatives of every token of candidate i (prompt_logprobs) and their sum
        (cumulative_logprob). The requests share the context's KV through the prefix cache.
        Blocking; thread-safe; drives the loop inline if no engine thread is running."""
        ctx = list(context_ids)
        if not ctx:
            raise ValueError("score() needs a non-empty context (the first token has nothing to condition on)")
        cands = [list(c) for c in candidates_ids]
        if any(not c for c in cands):
            raise ValueError("score() needs non-empty candidates")
        if not cands:
            return []
        results: Dict[int, GenerationOutput] = {}
        done = threading.Event()
        lock = threading.Lock()

        def cb(o: GenerationOutput):
            with lock:
                results[o.request_id] = o
                if len(results) == len(cands):
                    done.set()

        rids = [self.submit(ctx + c, cb, score_from=len(ctx), logprobs=top) for c in cands]
        if self._thread is None:
            while not done.is_set():
                if not self.step() and not self.sched.has_work() and self._inbox.empty():
                    break
        else:
            done.wait()
        if self._err is not None:
            raise RuntimeError(f"engine failed: {self._err!r}")
        return [results[i] for i in rids]

    def add_step_listener(self, fn: Callable[[int], None]):
        """fn(tokens) runs on the engine thread right after each step is launched (keep it cheap:
        e.g. loop.call_soon_threadsafe). The kind of step the device is about to run."""
        self._step_listeners = self._step_listeners + [fn]  # copy-on-write: the engine thread iterates

    def remove_step_listener(self, fn: Callable[[int], None]):
        self._step_listeners = [f for f in self._step_listeners if f is not fn]

    def _notify_launch(self, T: int):
        for fn in self._step_listeners:
            try:
                fn(T)
            except Exception:  # noqa: BLE001 -- a listener must not stop the engine
                log.exception("step listener failed")

    def abort(self, rid: int):
        self._aborts.put(rid)
        self._wake.set()

    def generate(self, prompts: Sequence[Sequence[int]], **kw) -> List[GenerationOutput]:
        """Blocking batch generation (drives the loop inline if no thread is running)."""
        results: Dict[int, GenerationOutput] = {}
        done = threading.Event()
        ids = []
        lock = threading.Lock()

        def cb(o: GenerationOutput):
            with lock:
                results[o.request_id] = o
                if len(results) == len(prompts):
                    done.set()

        for p in prompts:
            ids.append(self.submit(p, cb, **kw))
        if self._thread is None:
            while not done.is_set():
                if not self.step():
                    if not self.sched.has_work() and self._inbox.empty():
                        break
        else:
            done.wait()
        if self._err is not None:
            raise RuntimeError(f"engine failed: {self._err!r}")
        return [results[i] for i in ids]

    def embed(self, prompts: Sequence[Sequence[int]], pooling: str = "mean") -> np.ndarray:
        """Final-norm hidden state of each prompt, mean-pooled (pooling="mean") or of its last
        token ("last": reuses cached prefix blocks), [B, hidden] fp32, computed as embedding
        requests inside the continuous batch (the engine's own kernels and graphs, batched
        with whatever else is running). Blocking; thread-safe."""
        if pooling not in ("mean", "last"):
            raise ValueError(f"pooling must be 'mean' or 'last', not {pooling!r}")
        outs = self.generate([list(p) or [0] for p in prompts], embed="last" if pooling == "last" else True,
                             temperature=0.0, max_tokens=1)
        bad = [o.finish_reason for o in outs if o.embedding is None]
        if bad:
            raise RuntimeError(f"embedding requests did not complete: {bad}")
        return np.stack([o.embedding for o in outs]) if outs else np.zeros((0, self.model_cfg.hidden_size), np.float32)

    def embed_spans(self, prompt_ids: Sequence[int], spans: Sequence[Tuple[int, int]]) -> Tuple[np.ndarray, np.ndarray]:
        """One embedding request with spans (submit(embed=True, spans=)): (the whole-prompt mean
        [hidden], the span means [len(spans), hidden]), both fp32. Blocking; thread-safe."""
        o = self.generate([list(prompt_ids)], embed=True, spans=list(spans), temperature=0.0, max_tokens=1)[0]
        if o.embedding is None or (len(spans) and o.span_embeddings is None):
            raise RuntimeError(f"embedding request did not complete: {o.finish_reason}")
        se = o.span_embeddings if len(spans) else np.zeros((0, self.model_cfg.hidden_size), np.float32)
        return o.embedding, se

    def prewarm(self, prompt_ids: Sequence[int], timeout: float = 300.0) -> int:
        """Compute and cache the KV of `prompt_ids` (prefix cache) without keeping
        the request; returns the number of prompt tokens. Works with or without
        the engine thread running."""
        if self._thread is None:
            return self.generate([list(prompt_ids)], temperature=0.0, max_tokens=1, ignore_eos=True)[0].prompt_tokens
        done = threading.Event()
        box = {}

        def cb(o):
            box["o"] = o
            done.set()

        self.submit(list(prompt_ids), cb, temperature=0.0, max_tokens=1, ignore_eos=True)
        if not done.wait(timeout):
            raise TimeoutError("prewarm did not finish")
        return box["o"].prompt_tokens

    def start(self):
        if self._thread is not None:
            return
        sw = self.cfg.gil_switch_interval
        if sw is None and os.environ.get("PILOTTAI_GIL_SWITCH_S"):
            sw = float(os.environ["PILOTTAI_GIL_SWITCH_S"])
        if sw is not None and sw > 0:
            sys.setswitchinterval(sw)
        self._stop = False
        if self.cfg.freeze_heap:
            # the model, graphs and tokenizer are in place: keep them out of every later GC
            # pass (a full collection otherwise stalls the engine thread for tens of ms)
            from pilottai_amd.utils.gc_tune import freeze_heap

            self._froze = freeze_heap() > 0
        self._thread = threading.Thread(target=self._loop, name="pilottai-engine", daemon=True)
        self._thread.start()

    def stop(self):
        self._stop = True
        self._wake.set()
        if self._thread is not None:
            self._thread.join(timeout=30)
            self._thread = None
        if getattr(self, "_froze", False):  # give the frozen heap back to the collector
            import gc

            gc.unfreeze()
            self._froze = False
        self.release_followers()

    # ------------------------------------------------------------------ TP
    def _open_tp_ring(self):
        """The per-step TP header travels through a shared-memory ring (csrc/runtime/shm_ring.cpp;
        SURVEY §5: shared-memory rings, not sockets, for the node-local control hop): the
        driver publishes, every follower polls its own read position. PILOTTAI_TP_HEADER=gloo
        (or a node without POSIX shared memory) keeps the gloo broadcast."""
        if os.environ.get("PILOTTAI_TP_HEADER", "shm") == "gloo":
            return
        box = [f"pilottai_tp_{os.getpid()}_{self.tp.root}_{os.urandom(4).hex()}" if self.is_driver else None]
        torch.distributed.broadcast_object_list(box, src=self.tp.root, group=self.tp.cpu_group)
        # Symmetric two-phase handshake: every rank reaches the same two collectives whatever
        # fails where (a driver-side create failure must not leave the followers in a barrier
        # that the driver skipped). Phase 1: the driver creates, all ranks agree on the status;
        # phase 2: the followers attach, all ranks agree again. Any failure -> gloo everywhere.
        created = self._tp_ring_phase(lambda rt: self._set_tp_ring(rt.ShmRing(box[0], 9, 64, self.tp.size - 1, True))
                                      if self.is_driver else None, "create")
        attached = created and self._tp_ring_phase(
            lambda rt: self._set_tp_ring(rt.ShmRing(box[0], 9, 64, self.tp.size - 1, False, 120.0))
            if not self.is_driver else None, "attach")
        if not attached:
            self._tp_ring = None

    def _set_tp_ring(self, ring):
        self._tp_ring = ring

    def _tp_ring_phase(self, fn, what: str) -> bool:
        """Run fn(_runtime) on this rank, then all-reduce the failure flag over the TP group:
        True iff the phase succeeded on every rank."""
        bad = torch.zeros(1, dtype=torch.int32)
        try:
            from pilottai_amd import _runtime

            if os.environ.get("PILOTTAI_TP_RING_FAIL") == f"{what}:{self.tp.rank}":  # fault injection (tests)
                raise RuntimeError(f"injected TP ring {what} failure")
            fn(_runtime)
        except Exception as e:  # noqa: BLE001 — fall back to the gloo broadcast on every rank
            log.warning("TP header ring %s failed on rank %d (%s): using the gloo broadcast", what, self.tp.rank, e)
            bad[0] = 1
        torch.distributed.all_reduce(bad, group=self.tp.cpu_group)
        return int(bad[0]) == 0

    def _tp_send(self, op: int, *vals: int):
        h = self._tp_header
        h.zero_()
        h[0] = op
        for i, v in enumerate(vals):
            h[1 + i] = int(v)
        if self._tp_ring is not None:
            if not self._tp_ring.put(h.tolist(), 600.0):
                raise RuntimeError("TP follower stopped reading step headers (ring full for 600 s)")
        else:
            self.tp.broadcast(h, cpu=True)

    def _tp_recv(self):
        if self._tp_ring is not None:
            rec = self._tp_ring.get(self.tp.rank - 1, 3600.0)
            if rec is None:
                raise RuntimeError("no TP step header from the driver for an hour")
            return rec
        self.tp.broadcast(self._tp_header, cpu=True)
        return self._tp_header.tolist()

    def release_followers(self):
        """Driver: tell the follower ranks to leave `follow()` (idempotent)."""
        if self.tp.size > 1 and self.is_driver and not self._tp_closed:
            self._tp_closed = True
            self._tp_send(_OP_STOP)

    def follow(self) -> int:
        """Follower ranks (TP rank > 0): mirror the driver's steps until it stops.

        Returns the number of steps executed."""
        if self.is_driver:
            raise RuntimeError("follow() is for TP ranks > 0")
        if self.on_gpu:
            torch.cuda.set_device(self.device)
        n = 0
        with torch.inference_mode():
            while True:
                op, T, ns, nsamp, bucket, masks_changed, n_copy, trunc, embed = (int(v) for v in self._tp_recv())
                if op == _OP_STOP:
                    break
                if masks_changed:
                    self.tp.broadcast(self._class_masks)
                self.tp.broadcast(self._dev_meta[:n_copy])
                self._run(bucket, ns, bool(trunc), n_copy, bool(embed))
                self._health_fetch()
                if self.on_gpu:
                    torch.cuda.current_stream().synchronize()
                self._health_check()
                n += 1
        self.stats["steps"] += n
        return n

    def _health_fetch(self):
        for i, (_, w) in enumerate(self._health_dev):
            self._health_host[i:i + 1].copy_(w[:1], non_blocking=True)

    def _health_check(self):
        """Fail the engine (rather than continue on partial sums) if a device health word is
        set; call after the step's synchronize."""
        for i, (what, _) in enumerate(self._health_dev):
            if int(self._health_host[i]) != 0:
                raise RuntimeError(f"{what}; engine stopped")

    @property
    def failed(self) -> Optional[BaseException]:
        return self._err

    # ------------------------------------------------------------------ loop
    def _drain_inbox(self):
        while True:
            try:
                req: _Request = self._inbox.get_nowait()
            except queue.Empty:
                break
            self._reqs[req.rid] = req
            self.sched.add_request(req.rid, req.prompt_ids, req.temperature, req.max_tokens, req.seed,
                                   req.ignore_eos, req.stop_ids, req.grammar, req.top_k, req.top_p, req.embed,
                                   req.embed_last, req.logprobs, req.presence_penalty, req.frequency_penalty,
                                   list(req.logit_bias), req.min_p, req.ln_min_p, req.repetition_penalty,
                                   req.inv_repetition_penalty, req.score_from, list(req.prediction),
                                   req.prompt_lookup, req.draft_len, list(req.spans))
            self.stats["requests"] += 1
        while True:
            try:
                rid = self._aborts.get_nowait()
            except queue.Empty:
                break
            self.sched.abort(rid)
        for o in self.sched.drain_aborted():
            self._deliver(o)

    def _deliver(self, o):
        rid, toks, reason, plen, cached, nsamp, nforced, t_first, t_fin, eslot, lps = o
        emb = None
        if eslot >= 0 and eslot in self._embed_ready:  # read back when its step committed
            emb = self._embed_ready.pop(eslot)
        elif eslot >= 0:  # (aborted / not yet read) the request's pooling row: read and clear it
            if reason == 3:
                emb = (self._embed_pool[eslot] / self._pool_div(rid, plen)).cpu().numpy()
            self._embed_pool[eslot].zero_()
        if reason == 3:
            self.stats["embed_requests"] += 1
            self.stats["embed_tokens"] += plen - cached
            self.stats["embed_cached_tokens"] = self.stats.get("embed_cached_tokens", 0) + cached
        req = self._reqs.pop(rid, None)
        self.stats["finished"] += 1
        if req is None:
            return
        out = GenerationOutput(rid, list(toks), _REASONS.get(reason, "stop"), plen, cached, len(toks),
                               nsamp, nforced, req.t_arrival, t_first, t_fin, self.tok, emb,
                               lps, None if lps is None else float(sum(e[0] for e in lps)))
        if req.spans:
            out.span_embeddings = self._span_ready.pop(rid, None)
        if req.score_from >= 0:  # a scoring request's records are per prompt position: (logprob, rank, top)
            out.logprobs, out.prompt_logprobs = None, lps
        if req.draft_len > 0:
            for did, proposed, accepted, matched in self.sched.take_draft_counts():
                self._draft_counts[did] = (proposed, accepted, matched)
            proposed, accepted, matched = self._draft_counts.pop(rid, (0, 0, 0))
            out.accepted_prediction_tokens = matched
            out.rejected_prediction_tokens = proposed - accepted
        # per-request timings: TTFT = arrival -> first token, TPOT = later tokens' mean gap
        # (generation only: a scoring request has no first token and no token gaps)
        if t_first > 0 and req.score_from < 0:
            n_out = max(1, len(toks))
            self.timings.append((out.ttft, (t_fin - t_first) / max(1, n_out - 1), n_out))
        try:
            req.callback(out)
        except Exception:  # noqa: BLE001 — a bad callback must not kill the engine
            log.exception("completion callback failed")

    def step(self) -> bool:
        """Run one engine step. Returns False when there was nothing to run."""
        if self._async:
            return self._step_pipelined()
        self._drain_inbox()
        if not self.sched.has_work():
            self._flush_deliveries()
            return False
        L = self.L
        t0 = time.perf_counter()
        with trace_range("engine.schedule"):
            T = self.sched.schedule(self._host_ptr, self._host_meta.numel())
        t_sched = time.perf_counter()
        t_moves = 0.0  # counted in host_move_s, not in host_launch_s
        if self._host_pool is not None:  # after every schedule(), one that plans no step included
            t_moves = self._run_kv_moves()
        if T == 0:
            self._flush_deliveries()
            if self.sched.num_running == 0 and self.sched.num_waiting > 0:
                raise RuntimeError("KV cache too small for the head request")
            return False
        c = self._host_np[L["counts"]:L["counts"] + 12]
        ns, nsamp, trunc, embed, lp = int(c[1]), int(c[2]), int(c[6]) > 0, int(c[7]) > 0, int(c[8]) > 0
        pen = (int(c[9]) & 1) > 0
        score = (int(c[9]) & self._score_bit) > 0  # the step has scoring rows
        spec = (int(c[9]) & self._spec_bit) > 0  # the step has draft rows
        span = (int(c[9]) & self._span_bit) > 0  # the step has span segments
        # 0, or 1 + 2 * the token words of the step's repetition-penalty rows. The mask ends below
        # the lowest flag bit, which is now the span bit (28) and was the draft bit (29). Every
        # step decodes the value it decoded before: the field holds 3 + 4 * words at most, below
        # 2^28 while the repetition region has fewer than 2^26 words (64 M tokens per step, far
        # above any configuration; the scheduler refuses spans otherwise), so bit 28 was clear
        rep = (int(c[9]) & (self._span_bit - 1)) >> 1
        shape = int(c[11])  # 0, or 1 + the bias words of the step's logit_bias / min_p rows
        bucket = next(b for b in self.buckets if b >= T)
        s_b = self._seq_bucket(bucket)
        masks_changed = self._sync_masks()
        n_copy = L["embed_rows"] + bucket if embed else L["block_table"] + ns * L["max_blocks"]
        if pen:  # up to the end of the pair words the step's penalised rows use
            n_copy = L["pair_tok"] + int(c[10])
        resets = self.sched.take_embed_resets()
        if resets:  # preempted embedding requests restart from token 0
            self._embed_pool[torch.tensor(resets, dtype=torch.long, device=self.device)] = 0.0
        if self.on_gpu:
            self._dev_meta[:n_copy].copy_(self._host_meta[:n_copy], non_blocking=True)
            if shape:
                self._copy_shaping(self._host_meta, shape - 1)
            if rep:
                self._copy_repetition(self._host_meta, rep >> 1)
            if score:
                self._copy_scoring(self._host_meta)
            if spec:
                self._copy_runs(self._host_meta)
            if span:
                self._copy_spans(self._host_meta)
            ncp = int(self._host_np[L["n_copies"]])
            if ncp:
                self._copy_copies(self._host_meta, ncp)
        if self.tp.size > 1:
            self._tp_send(_OP_STEP, T, ns, nsamp, bucket, int(masks_changed), n_copy, int(trunc), int(embed))
            if masks_changed:
                self.tp.broadcast(self._class_masks)
            self.tp.broadcast(self._dev_meta[:n_copy])
        with torch.inference_mode(), trace_range("engine.forward"):
            self._run(bucket, ns, trunc, n_copy, embed, lp, pen, shape > 0, rep > 0, score, spec, span)
        if self._step_listeners:
            self._notify_launch(T)
        if nsamp:
            self._sampled_host[:nsamp].copy_(self._sampled_dev[:nsamp], non_blocking=self.on_gpu)
        if spec:
            self._accept_hosts[0][:nsamp].copy_(self._accept_dev[:nsamp], non_blocking=self.on_gpu)
        if lp:
            self._lp_hosts[0][:nsamp].copy_(self._lp_rec[:nsamp], non_blocking=self.on_gpu)
        if score:
            self._sc_hosts[0][:nsamp].copy_(self._sc_rec[:nsamp], non_blocking=self.on_gpu)
        self._health_fetch()
        t_launch = time.perf_counter()
        # the previous step's finished requests are handed to their callers while this step
        # runs on the GPU (host/device overlap): delivery needs nothing from it
        self._flush_deliveries()
        t_flush = time.perf_counter()
        if self.on_gpu:
            torch.cuda.current_stream().synchronize()
        self._health_check()
        t_sync = time.perf_counter()
        with trace_range("engine.commit"):
            outs = self.sched.commit(self._sampled_host.data_ptr(), nsamp,
                                     self._lp_hosts[0].data_ptr() if lp else 0,
                                     self._sc_hosts[0].data_ptr() if score else 0,
                                     self._accept_hosts[0].data_ptr() if spec else 0)
        if embed:
            self._read_embeddings(outs)
        if self._span_pool is not None:
            self._read_spans(outs)
        st = self.stats
        # host-side phases: schedule, metadata copy + launch, device wait, commit
        st["host_sched_s"] += t_sched - t0
        st["host_launch_s"] += t_launch - t_sched - t_moves
        st["device_wait_s"] += t_sync - t_launch
        st["steps"] += 1
        st["tokens"] += T
        st["bucket_tokens"] += bucket
        st["sampled"] += nsamp
        dt = time.perf_counter() - t0
        st["busy_s"] += dt
        bh = self.bucket_hist.setdefault(bucket, [0, 0.0])
        bh[0] += 1
        bh[1] += dt
        st["host_commit_s"] += time.perf_counter() - t_sync
        st["host_deliver_s"] += t_flush - t_launch  # overlapped with the device
        self._pending_out.extend(outs)
        if not self.sched.has_work():
            self._flush_deliveries()  # nothing to overlap with: deliver now
        return True

    # ------------------------------------------------------------- host KV tier
    @staticmethod
    def _check_host_cache(cfg: "EngineConfig", tp_size: int):
        gb, nb, cap = cfg.host_cache_gb, cfg.host_cache_blocks, cfg.host_cache_step_blocks
        if gb is None or not math.isfinite(float(gb)) or float(gb) < 0 or (nb is not None and int(nb) < 0):
            raise ValueError(f"host_cache_gb / host_cache_blocks must not be negative ({gb!r}, {nb!r})")
        if int(cap) < 0:
            raise ValueError(f"host_cache_step_blocks must not be negative, not {cap!r}")
        if not (int(nb) if nb is not None else float(gb) > 0):
            return
        if not cfg.prefix_caching:
            raise ValueError("the host KV tier (host_cache_gb) extends the prefix cache: it needs prefix_caching")
        if tp_size > 1:
            raise ValueError("the host KV tier (host_cache_gb) is not supported on a tensor-parallel (TP > 1) engine")
        if cfg.async_steps:
            raise ValueError("the host KV tier (host_cache_gb) is not supported on an async_steps engine")

    def _pinned_pool(self, slots: int, rec: int) -> torch.Tensor:
        """The host tier's pool [slots, rec] bf16, page-locked at exactly its size: the bytes are
        allocated pageable and registered with the runtime, because torch's pinned allocator may
        round a request of this size up (to the next power of two) and host_cache_gb is a
        promise about memory. Raises an error that names the size; the registration is undone
        when the engine is collected."""
        nbytes = slots * rec * 2
        what = f"{nbytes / 2**30:.2f} GiB of pinned host memory ({slots} blocks of {rec * 2} bytes)"
        try:
            pool = torch.empty(slots, rec, dtype=torch.bfloat16)
        except RuntimeError as e:
            raise RuntimeError(f"host KV tier: cannot allocate {what}: {e}") from e
        if not self.on_gpu:
            return pool
        rt = torch.cuda.cudart()
        rc = int(rt.cudaHostRegister(pool.data_ptr(), nbytes, 0))
        if rc != 0:
            raise RuntimeError(f"host KV tier: cannot page-lock {what}: runtime error {rc}")
        weakref.finalize(self, _unregister_pool, pool)
        if not pool.is_pinned():
            raise RuntimeError(f"host KV tier: {what} were registered but do not read as pinned")
        return pool

    def _run_kv_moves(self) -> float:
        """-> host seconds spent. Execute the moves of the schedule() call just made, on the engine's stream and outside
        the step graphs: every spill (gather into the staging buffer, one async copy per record
        into its host slot), then every fill (one async copy per record out of its slot, scatter).
        Stream order is all the synchronisation there is: the step launched next reads the blocks
        behind the scatter, and a chunk reuses the staging buffer behind the copies out of it."""
        spills, fills = self.sched.take_kv_moves()
        if not spills and not fills:
            return 0.0
        t0 = time.perf_counter()
        self._execute_kv_moves(spills, fills)
        return time.perf_counter() - t0

    def _execute_kv_moves(self, spills, fills):
        """spills: [(block, slot)], fills: [(slot, block)] (benchmarks/host_kv_cache.py times it)."""
        t0 = time.perf_counter()
        pool, stage, cap = self._host_pool, self._host_stage, self._host_stage.shape[0]
        nb = self.on_gpu
        blocks = torch.tensor([b for b, _ in spills] + [b for _, b in fills], dtype=torch.int32)
        if self.on_gpu:
            blocks = blocks.pin_memory().to(self.device, non_blocking=True)
        with torch.inference_mode():
            for c0 in range(0, len(spills), cap):
                ch = spills[c0:c0 + cap]
                ops.kv_gather_blocks(self.kv.k, self.kv.v, blocks[c0:c0 + len(ch)], len(ch), stage)
                for i, (_, slot) in enumerate(ch):
                    pool[slot].copy_(stage[i], non_blocking=nb)
            # a chunk never lists a block twice (a block filled, released and filled again within
            # one schedule() call): the second fill runs in a later launch, so it lands last
            c0, base = 0, len(spills)
            while c0 < len(fills):
                seen, m = set(), 0
                while c0 + m < len(fills) and m < cap and fills[c0 + m][1] not in seen:
                    seen.add(fills[c0 + m][1])
                    m += 1
                for i in range(m):
                    stage[i].copy_(pool[fills[c0 + i][0]], non_blocking=nb)
                ops.kv_scatter_blocks(self.kv.k, self.kv.v, blocks[base + c0:base + c0 + m], m, stage)
                c0 += m
        self.stats["host_move_s"] += time.perf_counter() - t0

    def prefix_blocks(self, token_ids: Sequence[int]) -> List[Tuple[str, int]]:
        """Where the leading full blocks of a prompt are cached: ("device", block id) or
        ("host", slot) per 16-token block of its hash chain, up to the first miss. Takes no
        reference and changes no LRU order. Call it between steps (not from another thread while
        the engine loop runs)."""
        return [("host" if tier else "device", int(i))
                for tier, i in self.sched.prefix_blocks([int(t) for t in token_ids])]

    # ------------------------------------------------------------- pipelined steps
    def _step_pipelined(self) -> bool:
        """One turn of the pipelined loop: launch the next step if fewer than two are in
        flight, then (with two in flight, or nothing new to launch) wait for the oldest and
        commit it. In steady state step N+1 is scheduled, copied and launched while step N
        runs on the device, so the device never waits for the host's schedule / launch /
        commit (0.5-0.6 ms per step in the serial loop, BENCH_r02 step_phase_ms)."""
        self._drain_inbox()
        launched = False
        if len(self._inflight) < 2 and self.sched.has_work():
            launched = self._launch_next()
        if self._inflight and (len(self._inflight) == 2 or not launched):
            self._complete(self._inflight.popleft())
            return True
        if not launched:
            self._flush_deliveries()
        return launched

    def _launch_next(self) -> bool:
        L = self.L
        slot = self._slot
        hm = self._host_metas[slot]
        t0 = time.perf_counter()
        with trace_range("engine.schedule"):
            T = self.sched.schedule(hm.data_ptr(), hm.numel())
        t_sched = time.perf_counter()
        if T == 0:
            if not self._inflight and self.sched.num_running == 0 and self.sched.num_waiting > 0:
                raise RuntimeError("KV cache too small for the head request")
            return False
        c = hm.numpy()[L["counts"]:L["counts"] + 12]
        ns, nsamp, trunc, embed, lp = int(c[1]), int(c[2]), int(c[6]) > 0, int(c[7]) > 0, int(c[8]) > 0
        shape = int(c[11])  # 0, or 1 + the bias words of the step's logit_bias / min_p rows
        score = (int(c[9]) & self._score_bit) > 0  # the step has scoring rows
        bucket = next(b for b in self.buckets if b >= T)
        self._sync_masks()
        n_copy = L["embed_rows"] + bucket if embed else L["block_table"] + ns * L["max_blocks"]
        resets = self.sched.take_embed_resets()
        if resets:
            self._embed_pool[torch.tensor(resets, dtype=torch.long, device=self.device)] = 0.0
        self._dev_meta[:n_copy].copy_(hm[:n_copy], non_blocking=self.on_gpu)
        if shape:
            self._copy_shaping(hm, shape - 1)
        if score:
            self._copy_scoring(hm)
        ncp = int(hm.numpy()[L["n_copies"]])
        if ncp:
            self._copy_copies(hm, ncp)
        with torch.inference_mode(), trace_range("engine.forward"):
            self._run(bucket, ns, trunc, n_copy, embed, lp, shape=shape > 0, score=score)
        if self._step_listeners:
            self._notify_launch(T)
        if nsamp:
            self._sampled_hosts[slot][:nsamp].copy_(self._sampled_dev[:nsamp], non_blocking=self.on_gpu)
        if lp:
            self._lp_hosts[slot][:nsamp].copy_(self._lp_rec[:nsamp], non_blocking=self.on_gpu)
        if score:
            self._sc_hosts[slot][:nsamp].copy_(self._sc_rec[:nsamp], non_blocking=self.on_gpu)
        if embed:
            self._embed_hosts[slot].copy_(self._embed_pool, non_blocking=self.on_gpu)
        self._health_fetch()
        ev = None
        if self.on_gpu:
            ev = torch.cuda.Event()
            ev.record()
        t_launch = time.perf_counter()
        self._inflight.append((slot, T, bucket, nsamp, embed, ev, t0, lp, score))
        self._slot = (slot + 1) % len(self._host_metas)
        st = self.stats
        st["host_sched_s"] += t_sched - t0
        st["host_launch_s"] += t_launch - t_sched
        self._flush_deliveries()  # the previous step's outputs, while this one is queued
        st["host_deliver_s"] += time.perf_counter() - t_launch
        return True

    def _complete(self, rec):
        slot, T, bucket, nsamp, embed, ev, t0, lp, score = rec
        t_w = time.perf_counter()
        if ev is not None:
            ev.synchronize()
        self._health_check()
        t_sync = time.perf_counter()
        with trace_range("engine.commit"):
            outs = self.sched.commit(self._sampled_hosts[slot].data_ptr(), nsamp,
                                     self._lp_hosts[slot].data_ptr() if lp else 0,
                                     self._sc_hosts[slot].data_ptr() if score else 0)
        if embed:
            self._read_embeddings(outs, self._embed_hosts[slot])
        st = self.stats
        st["device_wait_s"] += t_sync - t_w
        st["steps"] += 1
        st["tokens"] += T
        st["bucket_tokens"] += bucket
        st["sampled"] += nsamp
        # device time attributable to this step: from its launch (or the previous step's
        # completion, whichever is later) to its completion
        dt = t_sync - max(t0, self._last_done)
        self._last_done = t_sync
        st["busy_s"] += dt
        bh = self.bucket_hist.setdefault(bucket, [0, 0.0])
        bh[0] += 1
        bh[1] += dt
        st["host_commit_s"] += time.perf_counter() - t_sync
        self._pending_out.extend(outs)
        if not self._inflight and not self.sched.has_work():
            self._flush_deliveries()

    def _read_embeddings(self, outs, host: Optional[torch.Tensor] = None):
        """Pooled rows of the embedding requests this step finished. Serial loop: read from
        the device while it is idle (step synchronised). Pipelined loop: from `host`, the
        pinned snapshot taken behind this step (the next step is already queued, so a device
        read would wait for it too). Delivery runs during the NEXT step either way."""
        done = [(o[9], self._pool_div(o[0], o[3])) for o in outs if o[9] >= 0 and o[2] == 3]
        if not done:
            return
        slots = [e for e, _ in done]
        idx = torch.tensor(slots, dtype=torch.long, device=self.device)
        rows = host.numpy()[slots] if host is not None else self._embed_pool.index_select(0, idx).cpu().numpy()
        # stream-ordered: a finished request's row takes no more tokens in the queued step
        self._embed_pool.index_fill_(0, idx, 0.0)
        for (e, plen), r in zip(done, rows):
            self._embed_ready[e] = r / plen

    def _read_spans(self, outs):
        """Span means of the span requests this step finished: their accumulator rows are read
        now, before the next step is scheduled (a finished request's slots are free again, and
        their next holders' first segments overwrite them), and divided by the span lengths once,
        in fp32."""
        done = {o[0] for o in outs if o[2] == 3}
        for rid, slots in self.sched.take_span_finishes():
            req = self._reqs.get(rid)
            if rid not in done or req is None or len(slots) != len(req.spans):
                continue  # aborted: nothing to report
            idx = torch.tensor(slots, dtype=torch.long, device=self.device)
            sums = self._span_pool.index_select(0, idx).cpu().numpy()
            lens = np.array([b - a for a, b in req.spans], dtype=np.float32)
            self._span_ready[rid] = sums / lens[:, None]

    def _pool_div(self, rid: int, plen: int) -> int:
        """Tokens pooled into an embedding request's row: its prompt (mean), or 1 (last)."""
        req = self._reqs.get(rid)
        return 1 if (req is not None and req.embed_last) else max(1, plen)

    def _flush_deliveries(self):
        if self._pending_out:
            outs, self._pending_out = self._pending_out, []
            for o in outs:
                self._deliver(o)

    def _loop(self):
        if self.on_gpu:
            torch.cuda.set_device(self.device)
        try:
            while not self._stop:
                if not self.step():
                    self._wake.wait(0.01)
                    self._wake.clear()
        except BaseException as e:  # noqa: BLE001
            self._err = e
            log.exception("engine loop crashed")
            # requests that already finished (held for overlapped delivery) get their outputs
            try:
                self._flush_deliveries()
            except Exception:  # noqa: BLE001
                log.exception("delivery after the crash failed")
            # fail every other pending request loudly
            for rid in list(self._reqs):
                req = self._reqs.pop(rid)
                try:
                    req.callback(GenerationOutput(rid, [], "error", len(req.prompt_ids), 0, 0, 0, 0,
                                                  req.t_arrival, -1.0, self._rt.now(), self.tok))
                except Exception:  # noqa: BLE001
                    pass

    # ------------------------------------------------------------------ info
    def latency_summary(self, since: int = 0) -> dict:
        """p50/p99 TTFT and TPOT (ms) over requests finished after index `since`."""
        tm = list(self.timings)[since:]
        if not tm:
            return {}
        ttft = sorted(t[0] for t in tm)
        tpot = sorted(t[1] for t in tm if t[2] > 1)
        pick = lambda v, q: 1000 * v[min(len(v) - 1, int(q * len(v)))] if v else None  # noqa: E731
        return {"requests": len(tm), "ttft_p50_ms": pick(ttft, 0.5), "ttft_p99_ms": pick(ttft, 0.99),
                "tpot_p50_ms": pick(tpot, 0.5), "tpot_p99_ms": pick(tpot, 0.99)}

    def metrics(self) -> dict:
        s = self.sched
        st = dict(self.stats)
        st.update({
            "running": s.num_running, "waiting": s.num_waiting, "free_kv_blocks": s.num_free_blocks,
            "total_kv_blocks": self.num_kv_blocks, "cached_kv_blocks": s.num_cached_blocks,
            "prompt_tokens": s.total_prompt_tokens, "prefix_cache_hit_tokens": s.total_cached_tokens,
            "preemptions": s.total_preemptions, "graphs": len(self._graphs), "aligned_steps": s.aligned_steps,
            "prefix_defers": s.prefix_defers,
            "partial_hit_tokens": s.partial_hit_tokens, "same_step_shares": s.same_step_shares,
            "spec_rows": s.spec_rows, "spec_voided": s.spec_voided,
            "spec_draft_tokens": s.spec_draft_tokens, "spec_accepted_tokens": s.spec_accepted_tokens,
            "spec_draft_steps": s.spec_draft_steps, "spec_runs_full": s.spec_runs_full,
            "kv_cache_gb": self.kv.k.numel() * 2 * 2 / 2**30,
            "weights_gb": self.model.weight_bytes() / 2**30,
            "weight_quant": self.model.weight_quant, "fp8_decode": self.model.fp8_decode,
            "host_cache_blocks": self.host_cache_blocks, "num_host_cached": s.num_host_cached,  # blocks in the tier
            "host_hit_blocks": s.host_hit_blocks, "host_spilled_blocks": s.host_spilled_blocks,
            "host_evicted_blocks": s.host_evicted_blocks,
            "host_cache_gb": 0.0 if self._host_pool is None else self._host_pool.numel() * 2 / 2**30,
            "host_hit_tokens": s.host_hit_blocks * self.cfg.block_size,
        })
        if self.on_gpu:
            st["hbm_used_gb"] = torch.cuda.memory_allocated(self.device) / 2**30
        return st
