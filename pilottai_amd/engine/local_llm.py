"""LLM protocol adapters: the reference's `LLMHandler` contract served on-node.

Reference contract (pilott/engine/llm.py:38-219):
    await generate_response(messages, tools=None) -> {content, role, tool_calls, model, usage}
    await apredict(prompt) -> str
    await apredict_messages(messages, functions) -> dict
with a sliding-window RPM limiter, bounded concurrency and linear-backoff retries.

`LocalLLM` keeps that contract but every call becomes a request in the local
continuous batch (engine/engine.py), so 64 agents' concurrent calls share one
forward per step instead of queueing behind a 5-slot HTTP semaphore. Replies
can be constrained to a schema via `response_format` (source/rules.yaml
`schemas:`); agents and the orchestrator always pass one, so every reply parses.

Task queue on the GPU stream: an agent step's call is
`engine.submit()` -> the engine thread batches it into the next captured step on
the GPU's stream; the completion callback resolves the caller's asyncio future
with `loop.call_soon_threadsafe`, so the orchestrator's event loop never blocks
on the device.

`SchemaLLM` is a model-free implementation of the same protocol that emits
schema-valid JSON directly (used by CPU tests and the plumbing benchmark,
BASELINE config 1).
"""
from __future__ import annotations

import asyncio
import json
import logging
import random
import re
import threading
import time
from collections import deque
from numbers import Integral
from typing import Any, Deque, Dict, List, Mapping, Optional, Sequence, Union

import numpy as np

from .tokenizer import END_HEADER_ID, EOT_ID, START_HEADER_ID, BOS_ID, Tokenizer

log = logging.getLogger("pilottai_amd.llm")


def encode_chat(tok: Tokenizer, messages: Sequence[Dict[str, str]]) -> List[int]:
    """Llama-3 chat layout with the same special-token ids."""
    ids = [BOS_ID]
    for m in messages:
        ids.append(START_HEADER_ID)
        ids += tok.encode(str(m.get("role", "user")))
        ids.append(END_HEADER_ID)
        ids += tok.encode("\n\n" + str(m.get("content", "")))
        ids.append(EOT_ID)
    ids.append(START_HEADER_ID)
    ids += tok.encode("assistant")
    ids.append(END_HEADER_ID)
    ids += tok.encode("\n\n")
    return ids


def logprob_entries(tok: Tokenizer, token_ids: Sequence[int], logprobs) -> List[Dict[str, Any]]:
    """GenerationOutput.logprobs in the OpenAI `logprobs.content` shape (plus token ids): one
    {"token", "token_id", "logprob", "bytes", "top_logprobs": [{"token", "token_id", "logprob",
    "bytes"}]} per generated token, every token decoded on its own."""

    def one(tid: int, lp: float) -> Dict[str, Any]:
        raw = tok.decode_bytes([int(tid)])
        return {"token": raw.decode("utf-8", errors="replace"), "token_id": int(tid), "logprob": float(lp),
                "bytes": list(raw)}

    out = []
    for tid, (lp, top) in zip(token_ids, logprobs):
        e = one(tid, lp)
        e["top_logprobs"] = [one(i, v) for i, v in top]
        out.append(e)
    return out


def _cfg_get(config: Any, key: str, default=None):
    if config is None:
        return default
    if isinstance(config, dict):
        v = config.get(key, default)
    else:
        v = getattr(config, key, default)
    if hasattr(v, "get_secret_value"):
        v = v.get_secret_value()
    return default if v is None else v


class _RateLimiter:
    """Sliding 60 s window limiter (reference llm.py:68-89)."""

    def __init__(self, max_rpm: Optional[int]):
        self.max_rpm = max_rpm
        self.calls: Deque[float] = deque()
        self.lock = asyncio.Lock()

    async def acquire(self):
        if not self.max_rpm:
            return
        async with self.lock:
            now = time.monotonic()
            while self.calls and self.calls[0] <= now - 60.0:
                self.calls.popleft()
            if len(self.calls) >= self.max_rpm:
                await asyncio.sleep(max(0.0, 60.0 - (now - self.calls[0])))
            self.calls.append(time.monotonic())


class BaseLLM:
    """Shared protocol surface (rate limit, retries, response shaping)."""

    provider = "base"
    supports_logprobs = False  # response_format["logprobs"] is honoured and r["logprobs"] returned
    # response_format["presence_penalty"] / ["frequency_penalty"] are honoured
    supports_penalties = False
    # response_format["logit_bias"] ({token id: bias}) / ["min_p"] are honoured
    supports_logit_shaping = False
    supports_repetition_penalty = False  # response_format["repetition_penalty"] is honoured
    supports_scoring = False  # score() / choose(): log-probabilities of given candidate texts
    # response_format["prediction"] (text the reply is expected to repeat) / ["prompt_lookup"] are
    # honoured and r["usage"]["completion_tokens_details"] returned
    supports_prediction = False
    supports_embeddings = False  # embed(): pooled final hidden states of given texts / token ids

    async def embed(self, inputs: Sequence[Union[str, Sequence[int]]],
                    chunking: Optional[Dict[str, int]] = None) -> List[Dict[str, Any]]:
        """One {"embedding": fp32 [hidden], L2-normalised, "prompt_tokens": n} per input (a text or
        a list of token ids). chunking = {"chunk_tokens": c, "overlap": o} adds "chunks":
        [{"index", "span": [a, b], "text", "embedding"}], the chunk vectors computed inside the
        document (late chunking). Backends without a model to ask refuse."""
        raise NotImplementedError(f"the {self.provider!r} LLM backend cannot embed text "
                                  "(supports_embeddings is False): use the local engine or a pilottai_amd server")

    async def score(self, messages_or_text: Union[str, Sequence[Dict[str, str]]], candidates: Sequence[str],
                    top: int = 0) -> List[Dict[str, Any]]:
        """Log-probability of each candidate text as the continuation of the context (a chat as
        messages, or plain text): one {"logprob": sum, "tokens": [{token, token_id, logprob, rank,
        bytes, top_logprobs}]} per candidate. Backends without a model to ask refuse."""
        raise NotImplementedError(f"the {self.provider!r} LLM backend cannot score text "
                                  "(supports_scoring is False): use the local engine or a pilottai_amd server")

    async def choose(self, messages_or_text: Union[str, Sequence[Dict[str, str]]], options: Sequence[str],
                     normalize: bool = False):
        """Pick one of `options` by scoring them instead of decoding: returns (index, logprobs)
        with the index of the largest summed logprob (or the largest mean per token when
        `normalize` is set) and every option's figure."""
        if not options:
            raise ValueError("choose() needs at least one option")
        res = await self.score(messages_or_text, list(options))
        vals = [r["logprob"] / max(1, len(r["tokens"])) if normalize else r["logprob"] for r in res]
        return max(range(len(vals)), key=lambda i: vals[i]), vals

    def __init__(self, config: Any = None):
        self.config = config
        self.model_name = _cfg_get(config, "model_name", "llama-3-8b")
        self.temperature = float(_cfg_get(config, "temperature", 0.7))
        self.top_p = float(_cfg_get(config, "top_p", 1.0))
        self.top_k = int(_cfg_get(config, "top_k", 0))
        # request defaults of the OpenAI penalties over the generated tokens (0 = off)
        self.presence_penalty = float(_cfg_get(config, "presence_penalty", 0.0) or 0.0)
        self.frequency_penalty = float(_cfg_get(config, "frequency_penalty", 0.0) or 0.0)
        # request default of min_p truncation (0 = off); a logit_bias has no config default
        self.min_p = float(_cfg_get(config, "min_p", 0.0) or 0.0)
        # request default of the multiplicative repetition penalty (1 = off)
        rp = _cfg_get(config, "repetition_penalty", 1.0)
        self.repetition_penalty = 1.0 if rp is None else float(rp)
        # request default of prompt-lookup drafts (off); a prediction has no config default
        self.prompt_lookup = bool(_cfg_get(config, "prompt_lookup", False))
        self.max_tokens = int(_cfg_get(config, "max_tokens", 2000))
        self.retry_attempts = max(1, int(_cfg_get(config, "retry_attempts", 3)))
        self.retry_delay = float(_cfg_get(config, "retry_delay", 1.0))
        mc = _cfg_get(config, "max_concurrent", None)
        self._sem = asyncio.Semaphore(int(mc)) if mc else None
        self._limiter = _RateLimiter(_cfg_get(config, "max_rpm", None))
        self.usage = {"calls": 0, "prompt_tokens": 0, "completion_tokens": 0}

    async def _complete(self, messages, response_format, tools) -> Dict[str, Any]:
        raise NotImplementedError

    async def _call(self, messages, response_format=None, tools=None) -> Dict[str, Any]:
        if not messages:
            raise ValueError("Messages cannot be empty")
        await self._limiter.acquire()
        last: Optional[BaseException] = None
        for attempt in range(self.retry_attempts):
            try:
                if self._sem:
                    async with self._sem:
                        r = await self._complete(messages, response_format, tools)
                else:
                    r = await self._complete(messages, response_format, tools)
                self.usage["calls"] += 1
                self.usage["prompt_tokens"] += r["usage"]["prompt_tokens"]
                self.usage["completion_tokens"] += r["usage"]["completion_tokens"]
                return r
            except asyncio.CancelledError:
                raise
            except Exception as e:  # noqa: BLE001
                last = e
                if attempt < self.retry_attempts - 1:
                    log.warning("LLM attempt %d failed: %s", attempt + 1, e)
                    await asyncio.sleep(self.retry_delay * (attempt + 1))
        raise RuntimeError(f"LLM call failed after {self.retry_attempts} attempts: {last}")

    # -- reference protocol -------------------------------------------------
    async def generate_response(self, messages: List[Dict[str, str]], tools: Optional[List[Dict]] = None,
                                response_format: Optional[Dict[str, Any]] = None) -> Dict[str, Any]:
        return await self._call(messages, response_format, tools)

    async def apredict(self, prompt: str, response_format: Optional[Dict[str, Any]] = None) -> str:
        if not prompt:
            raise ValueError("Prompt cannot be empty")
        r = await self._call([{"role": "user", "content": prompt}], response_format)
        return r["content"]

    async def apredict_messages(self, messages: List[Dict], functions: List[Dict]) -> Dict[str, Any]:
        return await self._call(messages, None, functions)

    @staticmethod
    def _format_tools(tools: Optional[List[Dict]]) -> List[Dict]:
        out = []
        for t in tools or []:
            if not isinstance(t, dict) or "name" not in t:
                raise ValueError("Invalid tool format")
            out.append({"type": "function", "function": {"name": t["name"],
                                                         "description": t.get("description", ""),
                                                         "parameters": t.get("parameters", {})}})
        return out


def tool_call_schema(tools: Sequence[Dict]) -> Dict[str, Any]:
    """Function-calling reply schema: {"name": <tool>, "arguments": {...}}."""
    return {"name": "str(4)", "arguments": "obj()"}


class LocalLLM(BaseLLM):
    """Reference LLMHandler contract backed by the local MI355X engine."""

    provider = "local"
    supports_logprobs = True
    supports_penalties = True
    supports_logit_shaping = True
    supports_repetition_penalty = True
    supports_scoring = True
    supports_prediction = True
    supports_embeddings = True
    prefix_cache_layout = True  # agents put the shared task text first (core/agent.py)

    def __init__(self, config: Any = None, engine=None):
        super().__init__(config)
        if engine is None:
            from .registry import get_engine

            wq = _cfg_get(config, "weight_quant", None)
            hc = _cfg_get(config, "host_cache_gb", None)
            engine = get_engine(self.model_name, **({"weight_quant": wq} if wq is not None else {}),
                                **({"host_cache_gb": float(hc)} if hc is not None else {}))
        self.engine = engine
        # node-wide shared context (Serve.broadcast_context): a leading system
        # message whose KV every GPU pre-warmed into its prefix cache
        self.shared_context: Optional[str] = None
        self.tok: Tokenizer = engine.tok
        if engine._thread is None:
            engine.start()

    def context_ids(self, messages_or_text) -> List[int]:
        """Token ids of a scoring context: a chat in the reply layout (the candidate is the
        assistant's text), or plain text behind the begin-of-text token."""
        if isinstance(messages_or_text, str):
            return [BOS_ID] + self.tok.encode(messages_or_text)
        messages = list(messages_or_text)
        if not messages:
            raise ValueError("Messages cannot be empty")
        if self.shared_context:
            messages = [{"role": "system", "content": self.shared_context}] + messages
        return encode_chat(self.tok, messages)

    async def score(self, messages_or_text, candidates: Sequence[str], top: int = 0) -> List[Dict[str, Any]]:
        """One scoring request per candidate in the local continuous batch (engine.submit(score_from=)).
        The context and each candidate are tokenised separately and concatenated, which fixes the
        boundary; the candidates share the context's KV through the prefix cache."""
        return (await self.score_usage(messages_or_text, candidates, top))[0]

    async def score_usage(self, messages_or_text, candidates: Sequence[str], top: int = 0):
        """score() plus what it cost: (results, {"prompt_tokens", "cached_prompt_tokens"}) summed
        over the candidates' requests (the HTTP server's `usage`)."""
        if isinstance(candidates, str) or not all(isinstance(c, str) for c in candidates):
            raise ValueError("candidates must be a list of strings")
        top = int(top)
        if not 0 <= top <= 20:
            raise ValueError(f"top must be 0..20, not {top}")
        ctx = self.context_ids(messages_or_text)
        cands = [self.tok.encode(c) for c in candidates]
        if any(not c for c in cands):
            raise ValueError("every candidate must hold at least one token")
        loop = asyncio.get_running_loop()
        futs, rids = [], []
        try:
            for c in cands:
                fut = loop.create_future()
                futs.append(fut)
                rids.append(self.engine.submit(
                    ctx + c, lambda out, fut=fut: loop.call_soon_threadsafe(lambda: fut.done() or fut.set_result(out)),
                    score_from=len(ctx), logprobs=top))
            outs = await asyncio.gather(*futs)
        except asyncio.CancelledError:
            for rid in rids:
                self.engine.abort(rid)
            raise
        res = []
        for c, out in zip(cands, outs):
            if out.finish_reason != "score" or out.prompt_logprobs is None or len(out.prompt_logprobs) != len(c):
                raise RuntimeError(f"scoring request did not complete: {out.finish_reason}")
            toks = logprob_entries(self.tok, c, [(lp, alt) for lp, _, alt in out.prompt_logprobs])
            for e, (_, rank, _) in zip(toks, out.prompt_logprobs):
                e["rank"] = int(rank)
            res.append({"logprob": float(out.cumulative_logprob), "tokens": toks})
        usage = {"prompt_tokens": sum(o.prompt_tokens for o in outs),
                 "cached_prompt_tokens": sum(o.cached_prompt_tokens for o in outs)}
        self.usage["calls"] += 1
        self.usage["prompt_tokens"] += usage["prompt_tokens"]
        return res, usage

    async def embed(self, inputs, chunking: Optional[Dict[str, int]] = None) -> List[Dict[str, Any]]:
        """Embedding requests in the local continuous batch (engine.submit(embed=True)): the
        L2-normalised mean final-norm hidden state of each input's tokens. Texts are tokenised as
        they are (no begin-of-text token, like memory/embedding.EngineEmbedder); token ids must lie
        in the vocabulary. With `chunking` every context window of the input (span_windows over
        max_model_len - 1 tokens) is ONE span request (submit(spans=)) that yields the window's
        vector and all of its chunk vectors, so inputs longer than the context are allowed; the
        input's own vector is then the token-weighted mean of its windows' (the overlap tokens
        between two windows count in both). ValueError for anything outside these rules."""
        from pilottai_amd.memory.embedding import span_windows

        eng = self.engine
        if isinstance(inputs, str) or not isinstance(inputs, Sequence) or not len(inputs):
            raise ValueError("inputs must be a non-empty list of texts or token id lists")
        c = o = None
        if chunking is not None:
            if not isinstance(chunking, Mapping) or set(chunking) - {"chunk_tokens", "overlap"}:
                raise ValueError('chunking must be {"chunk_tokens": n, "overlap": m}')
            c, o = chunking.get("chunk_tokens"), chunking.get("overlap", 0)
            if eng.tp.size > 1 or eng.cfg.async_steps:
                raise ValueError("chunking is not supported on a tensor-parallel or async_steps engine")
        V = eng.model_cfg.vocab_size
        jobs = []  # (input index, ids, window start, [(a, b)] in window coordinates)
        all_ids, spans_of = [], []
        for i, x in enumerate(inputs):
            if isinstance(x, str):
                ids = self.tok.encode(x)
            elif isinstance(x, Sequence):
                ids = list(x)
                for t in ids:
                    if isinstance(t, bool) or not isinstance(t, Integral) or not 0 <= t < V:
                        raise ValueError(f"input {i}: token id {t!r} is not an integer in [0, {V})")
            else:
                raise ValueError(f"input {i} is neither a text nor a list of token ids")
            if not ids:
                raise ValueError(f"input {i} is empty")
            all_ids.append(ids)
            if chunking is None:
                if len(ids) >= eng.max_model_len:
                    raise ValueError(f"input {i}: {len(ids)} tokens do not fit max_model_len {eng.max_model_len} "
                                     "(send `chunking` to embed it in windows)")
                spans_of.append(None)
                jobs.append((i, ids, 0, None))
            else:
                wins = span_windows(len(ids), c, o, eng.max_model_len - 1, int(eng.L["span_slots"]))
                spans_of.append([sp for _, _, w in wins for sp in w])
                jobs += [(i, ids[s:e], s, [(a - s, b - s) for a, b in w]) for s, e, w in wins]
        loop = asyncio.get_running_loop()
        futs, rids = [], []
        try:
            for _, ids, _, spans in jobs:
                fut = loop.create_future()
                futs.append(fut)
                rids.append(eng.submit(
                    ids, lambda out, fut=fut: loop.call_soon_threadsafe(lambda: fut.done() or fut.set_result(out)),
                    embed=True, spans=spans, temperature=0.0, max_tokens=1))
            outs = await asyncio.gather(*futs)
        except asyncio.CancelledError:
            for rid in rids:
                eng.abort(rid)
            raise

        def unit(v):
            v = np.asarray(v, dtype=np.float32)
            n = np.float32(np.linalg.norm(v))
            return v / n if n > 0 else v

        res = [{"embedding": np.zeros(eng.model_cfg.hidden_size, np.float32), "prompt_tokens": len(ids)}
               for ids in all_ids]
        for r, sp in zip(res, spans_of):
            if sp is not None:
                r["chunks"] = []
        for (i, ids, _, spans), out in zip(jobs, outs):
            if out.embedding is None or (spans and out.span_embeddings is None):
                raise RuntimeError(f"embedding request did not complete: {out.finish_reason}")
            res[i]["embedding"] = res[i]["embedding"] + np.float32(len(ids)) * out.embedding
            for v in (out.span_embeddings if spans else ()):
                k = len(res[i]["chunks"])
                a, b = spans_of[i][k]
                res[i]["chunks"].append({"index": k, "span": [a, b], "text": self.tok.decode(all_ids[i][a:b]),
                                         "embedding": unit(v)})
        for r in res:
            r["embedding"] = unit(r["embedding"])
        self.usage["calls"] += 1
        self.usage["prompt_tokens"] += sum(r["prompt_tokens"] for r in res)
        return res

    async def _complete(self, messages, response_format, tools) -> Dict[str, Any]:
        grammar = None
        fixed = None
        if tools:
            names = [t["name"] for t in tools]
            fixed = {"name": names[0]} if len(names) == 1 else None
            grammar = self.engine.grammar.compile(tool_call_schema(tools), fixed)
        elif response_format:
            schema = response_format.get("schema")
            fixed = response_format.get("fixed")
            if schema is not None:
                grammar = self.engine.grammar.compile(schema, fixed)
        if self.shared_context:
            messages = [{"role": "system", "content": self.shared_context}] + list(messages)
        ids = encode_chat(self.tok, messages)
        loop = asyncio.get_running_loop()
        fut = loop.create_future()

        def done(out):
            loop.call_soon_threadsafe(lambda: fut.done() or fut.set_result(out))

        rf = response_format or {}
        temp = float(rf.get("temperature", self.temperature))
        # a prediction is text: tokenised on its own, without special tokens (the engine resyncs its
        # cursor on the reply's tokens, so the boundary to the chat template plays no part)
        pred = rf.get("prediction")
        if pred is not None and not isinstance(pred, str):
            raise ValueError("response_format['prediction'] must be a string")
        drafts = dict(prediction=self.tok.encode(pred) if pred else (),
                      prompt_lookup=bool(rf.get("prompt_lookup", self.prompt_lookup)))
        if rf.get("draft_len") is not None:
            drafts["draft_len"] = rf["draft_len"]
        rid = self.engine.submit(ids, done, temperature=temp, max_tokens=int(rf.get("max_tokens", self.max_tokens)),
                                 grammar=grammar,
                                 seed=rf.get("seed"), top_k=int(rf.get("top_k", self.top_k)),
                                 top_p=float(rf.get("top_p", self.top_p)),
                                 logprobs=-1 if rf.get("logprobs") is None else int(rf["logprobs"]),
                                 presence_penalty=rf.get("presence_penalty", self.presence_penalty),
                                 frequency_penalty=rf.get("frequency_penalty", self.frequency_penalty),
                                 logit_bias=rf.get("logit_bias"), min_p=rf.get("min_p", self.min_p),
                                 repetition_penalty=rf.get("repetition_penalty", self.repetition_penalty),
                                 **drafts)
        try:
            out = await fut
        except asyncio.CancelledError:
            self.engine.abort(rid)
            raise
        if out.finish_reason == "error":
            raise RuntimeError("local engine failed")
        text = out.text
        tool_calls = None
        if tools:
            try:
                call = json.loads(text)
                tool_calls = [{"id": f"call_{rid}", "type": "function",
                               "function": {"name": call.get("name"),
                                            "arguments": json.dumps(call.get("arguments", {}))}}]
            except json.JSONDecodeError:
                tool_calls = None
        return {
            "content": text,
            "role": "assistant",
            "tool_calls": tool_calls,
            # response_format["logprobs"] = n (0..20): per generated token, its log-probability and
            # the n most likely alternatives among the tokens the grammar allowed (None: not asked)
            "logprobs": None if out.logprobs is None else logprob_entries(self.tok, out.token_ids, out.logprobs),
            "model": self.engine.model_cfg.name,
            "usage": {"prompt_tokens": out.prompt_tokens, "completion_tokens": out.completion_tokens,
                      "total_tokens": out.prompt_tokens + out.completion_tokens,
                      "completion_tokens_details": {
                          "accepted_prediction_tokens": out.accepted_prediction_tokens,
                          "rejected_prediction_tokens": out.rejected_prediction_tokens}},
            "timing": {"ttft": out.ttft, "latency": out.latency,
                       "cached_prompt_tokens": out.cached_prompt_tokens,
                       "sampled_tokens": out.sampled_tokens},
        }


# ---------------------------------------------------------------------------
# model-free schema LLM (CPU tests, plumbing benchmark)
# ---------------------------------------------------------------------------

_TYPE = re.compile(r"^(\w+)\((.*)\)$")


def fake_value(spec: Any, path: str, fixed: Dict[str, Any], rng: random.Random) -> Any:
    if path in fixed:
        return fixed[path]
    if isinstance(spec, dict):
        if "objlist" in spec:
            return [fake_value(spec["item"], f"{path}[{i}]", fixed, rng) for i in range(int(spec["objlist"]))]
        return {k: fake_value(v, f"{path}.{k}" if path else k, fixed, rng) for k, v in spec.items()}
    s = str(spec)
    if s == "bool":
        return rng.random() < 0.5
    m = _TYPE.match(s)
    kind, arg = m.group(1), m.group(2)
    if kind == "int":
        lo, hi = (int(x) for x in arg.split(","))
        return rng.randint(lo, hi)
    if kind == "str":
        return " ".join(rng.choice(["alpha", "beta", "gamma", "delta", "task", "plan"])
                        for _ in range(max(1, min(3, int(arg)))))
    if kind == "enum":
        return rng.choice(arg.split("|"))
    if kind == "list":
        if not arg:
            return []
        mx = int(arg.rsplit(",", 1)[1])
        return ["item"] * mx
    if kind == "map":
        return {"key": "value"}
    if kind == "obj":
        return {}
    raise ValueError(s)


class SchemaLLM(BaseLLM):
    """Deterministic model-free LLM: replies are schema-valid JSON (CPU / plumbing)."""

    provider = "schema"

    def __init__(self, config: Any = None, seed: int = 0, latency_s: float = 0.0):
        super().__init__(config)
        self.rng = random.Random(seed)
        self.latency_s = latency_s
        self.calls: List[Dict[str, Any]] = []
        self._lock = threading.Lock()

    async def _complete(self, messages, response_format, tools) -> Dict[str, Any]:
        from .grammar import load_schemas

        if self.latency_s:
            await asyncio.sleep(self.latency_s)
        fixed = dict((response_format or {}).get("fixed") or {})
        if tools:
            obj = {"name": fixed.get("name", tools[0]["name"]), "arguments": {}}
            content = json.dumps(obj)
            tool_calls = [{"id": "call_0", "type": "function",
                           "function": {"name": obj["name"], "arguments": "{}"}}]
        else:
            schema = (response_format or {}).get("schema")
            if schema is None:
                content = "ok"
            else:
                spec = load_schemas()[schema] if isinstance(schema, str) else schema
                with self._lock:
                    content = json.dumps(fake_value(spec, "", fixed, self.rng))
            tool_calls = None
        n_prompt = sum(len(str(m.get("content", ""))) // 4 for m in messages)
        return {"content": content, "role": "assistant", "tool_calls": tool_calls, "model": "schema",
                "usage": {"prompt_tokens": n_prompt, "completion_tokens": len(content) // 4,
                          "total_tokens": n_prompt + len(content) // 4}}


def make_llm(config: Union[Dict[str, Any], Any, None] = None, engine=None) -> BaseLLM:
    """LLM factory keyed by provider: "local" (MI355X engine, default), "schema" (model-free),
    or "openai" (any OpenAI-compatible endpoint, e.g. a remote pilottai_amd server)."""
    provider = str(_cfg_get(config, "provider", "local")).lower()
    if provider in ("schema", "fake", "mock"):
        return SchemaLLM(config)
    if provider in ("local", "pilottai", "amd", "rocm", "mi355x"):
        return LocalLLM(config, engine=engine)
    if provider in ("openai", "http", "openai_compat", "remote"):
        from .http_llm import OpenAICompatLLM

        return OpenAICompatLLM(config)
    raise ValueError(f"unsupported LLM provider {provider!r}: use 'local' (on-node engine), 'schema' "
                     "or 'openai' (an OpenAI-compatible endpoint with base_url)")
