"""OpenAI-compatible HTTP front end for the on-node engine.

The reference reaches its model over HTTPS through litellm (`pilott/engine/llm.py:59`,
SURVEY C14); here the model runs on the MI355X in the same process, and this module
publishes it to other processes and hosts with the wire format those clients already
speak:

    GET  /                     landing page with live engine metrics (serving/site.py)
    GET  /health               liveness + engine metrics (steps, tokens/s, KV use, HBM)
    GET  /v1/models            the served model
    POST /v1/chat/completions  messages -> one completion (stream=true: SSE, one delta + [DONE])
    POST /v1/score             {"context": str | messages, "candidates": [str, ...], "top_logprobs": 0..20}
                               -> {"object": "score", "model", "scores": [{"index", "logprob", "tokens":
                               [{token, token_id, logprob, rank, bytes, top_logprobs}]}], "usage"}: the
                               log-probability of each candidate as the continuation of the context
                               (nothing is generated; the candidates share the context's KV). -inf is
                               sent as -9999.0; malformed bodies and the model-free backend answer 400
    POST /v1/embeddings        OpenAI's shape: {"input": text | [text, ...] | [token id, ...] | [[token id, ...], ...],
                               "model", "encoding_format": "float" | "base64" (little-endian fp32)} ->
                               {"object": "list", "data": [{"object": "embedding", "index", "embedding"}], "model",
                               "usage": {"prompt_tokens", "total_tokens"}}: the L2-normalised mean final-norm
                               hidden state of each input, `hidden_size` entries (`dimensions` may only name that
                               size). Extension "chunking": {"chunk_tokens": n, "overlap": m} adds to each item
                               "chunks": [{"index", "span": [a, b], "text", "embedding"}] -- the vectors of
                               overlapping token chunks, each computed inside the document in the same prefill
                               (the engine's span requests) -- and lifts the context limit: a longer input is
                               embedded in windows of whole chunks. Empty input, ids outside the vocabulary, an
                               input of max_model_len tokens or more without chunking, a malformed chunking object
                               and the model-free backend answer 400

`response_format` accepts the OpenAI forms and one extension:
* {"type": "json_schema", "json_schema": {"name": ..., "schema": {...}}}: a JSON Schema
  subset (objects, strings with maxLength or enum, bounded integers, booleans, arrays of
  strings or objects) compiled to the engine's token grammar, so the reply parses;
* {"type": "pilottai_schema", "schema": "agent.task_analysis", "fixed": {...}}: a schema
  of source/rules.yaml by name, with pinned fields. This is what
  `engine/http_llm.OpenAICompatLLM` sends, so agents on another host run the same
  constrained protocol as agents in-process.
`tools` (OpenAI function tools) produce a constrained `{"name", "arguments"}` call,
returned as `tool_calls`.

`logprobs: true` (with `top_logprobs: 0..20`) returns `choices[0].logprobs.content`: per
generated token its log-probability and the most likely alternatives, under softmax(logits)
over the tokens the reply's grammar allowed at that position, at temperature 1 (a
grammar-forced token has 0.0). Each entry also carries `token_id`; -inf is sent as -9999.0.

`presence_penalty` / `frequency_penalty` (numbers in [-2, 2], OpenAI semantics over the
GENERATED tokens: logit[t] -= presence * [c_t > 0] + frequency * c_t) are applied by the engine
before the grammar mask, top-k / top-p, the sampler and the logprob pass; 0 or absent means
nothing. `repetition_penalty` (a number in (0, 2], the HF / vLLM extension; 1 or absent means
nothing) is applied before them, on the raw logits: every token t of the prompt or of the reply so
far gets logit[t] <- x > 0 ? x * float32(1 / r) : x * r. `n > 1` is not supported.

`logit_bias` (the OpenAI wire form: an object of at most 300 entries whose keys are token ids
as strings and whose values are numbers in [-100, 100]) is added to those logits at every
sampling step, behind the penalties and before the grammar mask -- a token the reply's grammar
does not allow stays impossible, so -100 bans an enum value or a tool name and the reply still
parses. `min_p` (a number in [0, 1], the vLLM extension) keeps, at temperature > 0, the allowed
tokens whose probability is at least min_p times the most likely one's, intersected with
top_k / top_p. Malformed values answer 400.

Every request becomes one `LocalLLM` call, i.e. one sequence in the engine's continuous
batch. Concurrent HTTP clients share the engine's steps exactly like in-process agents.

    python -m pilottai_amd.serving.http_server --model llama-3-8b --port 8000   # MI355X
    python -m pilottai_amd.serving.http_server --schema --port 8000             # model-free
"""
from __future__ import annotations

import argparse
import json
import time
import uuid
from typing import Any, Dict, List, Optional

from fastapi import FastAPI, HTTPException
from fastapi.responses import HTMLResponse, JSONResponse, StreamingResponse

DEFAULT_STR_TOKENS = 32


def json_schema_to_spec(js: Dict[str, Any], path: str = "") -> Any:
    """Convert a JSON Schema subset to the rules.yaml schema language (engine/grammar.py)."""
    if not isinstance(js, dict):
        raise ValueError(f"schema at {path or '<root>'} must be an object")
    t = js.get("type")
    if "enum" in js:
        vals = [str(v) for v in js["enum"]]
        if not vals or any("|" in v for v in vals):
            raise ValueError(f"unsupported enum at {path or '<root>'}")
        return "enum(" + "|".join(vals) + ")"
    if t == "object":
        props = js.get("properties")
        if props:
            return {k: json_schema_to_spec(v, f"{path}.{k}" if path else k) for k, v in props.items()}
        add = js.get("additionalProperties")
        if isinstance(add, dict) and add.get("type") == "string":
            return f"map(str({_str_tokens(add)}))"
        return "obj()"
    if t == "string":
        return f"str({_str_tokens(js)})"
    if t == "boolean":
        return "bool"
    if t == "integer":
        lo, hi = int(js.get("minimum", 0)), int(js.get("maximum", 100))
        if hi < lo or hi - lo > 1000:
            raise ValueError(f"integer range at {path or '<root>'} must span at most 1000 values")
        return f"int({lo},{hi})"
    if t == "array":
        item = js.get("items") or {"type": "string"}
        mn = int(js.get("minItems", 1))
        mx = int(js.get("maxItems", max(mn, 4)))
        if item.get("type") == "object":
            return {"objlist": max(1, mn), "item": json_schema_to_spec(item, f"{path}[]")}
        if item.get("type", "string") != "string":
            raise ValueError(f"arrays at {path or '<root>'} must hold strings or objects")
        return f"list(str({_str_tokens(item)}),{mn},{mx})"
    raise ValueError(f"unsupported schema type {t!r} at {path or '<root>'}")


def _str_tokens(js: Dict[str, Any]) -> int:
    n = js.get("maxLength")
    return max(1, int(n) // 4) if n else DEFAULT_STR_TOKENS


def _response_format(body: Dict[str, Any]) -> Optional[Dict[str, Any]]:
    rf = body.get("response_format")
    out: Dict[str, Any] = {}
    for k in ("temperature", "top_p", "top_k", "seed"):
        if body.get(k) is not None:
            out[k] = body[k]
    if not rf:
        return out or None
    kind = rf.get("type")
    if kind == "pilottai_schema":
        out.update(schema=rf["schema"], fixed=rf.get("fixed") or {})
    elif kind == "json_schema":
        js = (rf.get("json_schema") or {}).get("schema")
        if js is None:
            raise ValueError("json_schema.schema is required")
        out.update(schema=json_schema_to_spec(js), fixed={})
    elif kind == "text":
        pass
    else:
        raise ValueError(f"unsupported response_format type {kind!r}")
    return out


def _penalties(body: Dict[str, Any]) -> Dict[str, float]:
    """The request's non-zero `presence_penalty` / `frequency_penalty` (0 or absent: nothing)."""
    out: Dict[str, float] = {}
    for k in ("presence_penalty", "frequency_penalty"):
        v = body.get(k)
        if v is None:
            continue
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not -2.0 <= v <= 2.0:  # NaN fails too
            raise ValueError(f"{k} must be a number between -2 and 2")
        if v != 0:
            out[k] = float(v)
    return out


def _repetition(body: Dict[str, Any]) -> Dict[str, float]:
    """The request's `repetition_penalty` when it is not 1 (1 or absent: nothing)."""
    v = body.get("repetition_penalty")
    if v is None:
        return {}
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 < v <= 2.0:  # NaN fails too
        raise ValueError("repetition_penalty must be a number greater than 0 and at most 2")
    return {"repetition_penalty": float(v)} if v != 1 else {}


LOGIT_BIAS_MAX = 300  # entries of one request's logit_bias (ops.LOGIT_BIAS_MAX)


def _shaping(body: Dict[str, Any], vocab_size: Optional[int] = None) -> Dict[str, Any]:
    """The request's `logit_bias` ({token id: bias}, zero entries dropped) and non-zero `min_p`."""
    out: Dict[str, Any] = {}
    lb = body.get("logit_bias")
    if lb is not None:
        if not isinstance(lb, dict):
            raise ValueError("logit_bias must be an object of token id -> bias")
        if len(lb) > LOGIT_BIAS_MAX:
            raise ValueError(f"logit_bias takes at most {LOGIT_BIAS_MAX} entries")
        bias: Dict[int, float] = {}
        for k, v in lb.items():
            try:
                if isinstance(k, bool) or not isinstance(k, (str, int)):
                    raise ValueError
                t = int(k.strip(), 10) if isinstance(k, str) else k
            except ValueError:
                raise ValueError(f"logit_bias key {k!r} is not a token id") from None
            if t < 0 or (vocab_size is not None and t >= vocab_size):
                raise ValueError(f"logit_bias token id {t} is outside the vocabulary")
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not -100.0 <= v <= 100.0:  # NaN fails too
                raise ValueError(f"logit_bias[{t}] must be a number between -100 and 100")
            if t in bias:
                raise ValueError(f"logit_bias names token id {t} twice")
            if v != 0:
                bias[t] = float(v)
            else:
                bias.setdefault(t, 0.0)
        bias = {t: v for t, v in bias.items() if v != 0}
        if bias:
            out["logit_bias"] = bias
    mp = body.get("min_p")
    if mp is not None:
        if isinstance(mp, bool) or not isinstance(mp, (int, float)) or not 0.0 <= mp <= 1.0:  # NaN fails too
            raise ValueError("min_p must be a number between 0 and 1")
        if mp != 0:
            out["min_p"] = float(mp)
    return out


def _logprobs(body: Dict[str, Any]) -> int:
    """The number of alternatives asked for (-1: no logprobs), from `logprobs` / `top_logprobs`."""
    want, top = body.get("logprobs"), body.get("top_logprobs")
    if want is not None and not isinstance(want, bool):
        raise ValueError("logprobs must be a boolean")
    if top is None:
        return 0 if want else -1
    if isinstance(top, bool) or not isinstance(top, int) or not 0 <= top <= 20:
        raise ValueError("top_logprobs must be an integer between 0 and 20")
    if not want:
        raise ValueError("top_logprobs requires logprobs: true")
    return top


def _wire_logprobs(entries: List[Dict[str, Any]]) -> Dict[str, Any]:
    def lp(v: float) -> float:
        return -9999.0 if v == float("-inf") or v != v else float(v)

    def one(e: Dict[str, Any]) -> Dict[str, Any]:
        return {"token": e["token"], "token_id": e.get("token_id"), "logprob": lp(e["logprob"]),
                "bytes": e.get("bytes")}

    return {"content": [dict(one(e), top_logprobs=[one(t) for t in e.get("top_logprobs", [])]) for e in entries]}


def _prediction(body: Dict[str, Any]) -> Dict[str, Any]:
    """OpenAI's Predicted Outputs (`prediction`: {"type": "content", "content": text or a list of
    {"type": "text", "text": ...} parts, concatenated}) and the `prompt_lookup` extension, as
    response_format entries; {} when the request asks for neither. ValueError -> 400."""
    out: Dict[str, Any] = {}
    pred = body.get("prediction")
    if pred is not None:
        if not isinstance(pred, dict) or pred.get("type") != "content":
            raise ValueError('prediction must be an object of type "content"')
        content = pred.get("content")
        if isinstance(content, list):
            parts = []
            for part in content:
                if not isinstance(part, dict) or part.get("type") != "text" or not isinstance(part.get("text"), str):
                    raise ValueError('prediction.content parts must be {"type": "text", "text": string}')
                parts.append(part["text"])
            content = "".join(parts)
        if not isinstance(content, str):
            raise ValueError("prediction.content must be a string or a list of text parts")
        if content:
            out["prediction"] = content
    pl = body.get("prompt_lookup")
    if pl is not None:
        if not isinstance(pl, bool):
            raise ValueError("prompt_lookup must be a boolean")
        if pl:
            out["prompt_lookup"] = True
    return out


def _embedding_inputs(inp: Any) -> List[Any]:
    """The `input` of /v1/embeddings as a list of texts or token id lists: a string, a list of
    strings, a list of token ids, or a list of such lists. ValueError -> 400."""
    is_id = lambda t: isinstance(t, int) and not isinstance(t, bool)  # noqa: E731
    if isinstance(inp, str):
        inp = [inp]
    elif isinstance(inp, list) and inp and all(is_id(t) for t in inp):
        inp = [inp]
    if not isinstance(inp, list) or not inp:
        raise ValueError("input must be a non-empty string, list of strings, list of token ids or list of such lists")
    if all(isinstance(x, str) for x in inp):
        if any(not x for x in inp):
            raise ValueError("input texts must not be empty")
    elif all(isinstance(x, list) and x and all(is_id(t) for t in x) for x in inp):
        pass
    else:
        raise ValueError("input must hold only non-empty strings or only non-empty lists of token ids")
    return inp


def _chunking(ch: Any) -> Optional[Dict[str, int]]:
    """The `chunking` extension of /v1/embeddings: {"chunk_tokens": n >= 1, "overlap": 0 <= m < n}
    (overlap 0 when absent); None when the request has none. ValueError -> 400."""
    if ch is None:
        return None
    if not isinstance(ch, dict) or set(ch) - {"chunk_tokens", "overlap"} or "chunk_tokens" not in ch:
        raise ValueError('chunking must be an object {"chunk_tokens": n, "overlap": m}')
    c, o = ch["chunk_tokens"], ch.get("overlap", 0)
    if isinstance(c, bool) or not isinstance(c, int) or c < 1:
        raise ValueError("chunking.chunk_tokens must be an integer >= 1")
    if isinstance(o, bool) or not isinstance(o, int) or not 0 <= o < c:
        raise ValueError("chunking.overlap must be an integer in [0, chunk_tokens)")
    return {"chunk_tokens": c, "overlap": o}


def _tools(body: Dict[str, Any]) -> Optional[List[Dict[str, Any]]]:
    tools = body.get("tools")
    if not tools:
        return None
    out = []
    for t in tools:
        f = t.get("function", t)
        out.append({"name": f["name"], "description": f.get("description", ""),
                    "parameters": f.get("parameters", {})})
    return out


def create_app(llm, model_name: Optional[str] = None, engine=None) -> FastAPI:
    """FastAPI app serving `llm` (a BaseLLM: LocalLLM on the GPU, SchemaLLM model-free)."""
    app = FastAPI(title="pilottai_amd", version="0.1.0")
    name = model_name or getattr(llm, "model_name", "local")
    started = time.time()

    @app.get("/", response_class=HTMLResponse)
    async def index():
        from pilottai_amd.serving.site import render

        return render(name)

    @app.get("/health")
    async def health():
        out = {"status": "ok", "model": name, "uptime_s": round(time.time() - started, 1),
               "usage": dict(getattr(llm, "usage", {}))}
        eng = engine or getattr(llm, "engine", None)
        if eng is not None:
            if getattr(eng, "failed", None) is not None:
                return JSONResponse({"status": "failed", "error": str(eng.failed)}, status_code=503)
            out["engine"] = m = eng.metrics()
            # the host KV tier (EngineConfig.host_cache_gb; all 0 while it is off)
            for k in ("host_cache_gb", "host_hit_tokens", "host_spilled_blocks"):
                out[k] = m.get(k, 0)
            out["host_cached_blocks"] = m.get("num_host_cached", 0)
        return out

    @app.get("/v1/models")
    async def models():
        entry = {"id": name, "object": "model", "owned_by": "pilottai_amd"}
        eng = engine or getattr(llm, "engine", None)
        model = getattr(eng, "model", None)
        if model is not None:
            entry["weight_quant"] = getattr(model, "weight_quant", None)
            entry["fp8_decode"] = bool(getattr(model, "fp8_decode", False))
        return {"object": "list", "data": [entry]}

    @app.post("/v1/chat/completions")
    async def chat(body: Dict[str, Any]):
        messages = body.get("messages")
        if not messages:
            raise HTTPException(400, "messages must be a non-empty list")
        try:
            rf = _response_format(body)
            tools = _tools(body)
            n_lp = _logprobs(body)
            pens = _penalties(body)
            rep = _repetition(body)
            eng = engine or getattr(llm, "engine", None)
            shaping = _shaping(body, getattr(getattr(eng, "model_cfg", None), "vocab_size", None))
            drafts = _prediction(body)
        except (KeyError, ValueError) as e:
            raise HTTPException(400, str(e))
        if drafts:
            if not getattr(llm, "supports_prediction", False):
                raise HTTPException(400, f"the {getattr(llm, 'provider', 'configured')} backend cannot use "
                                         "a prediction / prompt_lookup")
            if n_lp >= 0 or pens or rep:
                raise HTTPException(400, "prediction / prompt_lookup cannot be combined with logprobs, "
                                         "presence / frequency penalties or a repetition_penalty")
            if eng is not None and (eng.tp.size > 1 or eng.cfg.async_steps):
                raise HTTPException(400, "prediction / prompt_lookup are not supported on a tensor-parallel "
                                         "or async_steps engine")
            tok = getattr(llm, "tok", None)
            if tok is not None and eng is not None and "prediction" in drafts and \
                    len(tok.encode(drafts["prediction"])) > eng.max_model_len:
                raise HTTPException(400, f"prediction is longer than max_model_len ({eng.max_model_len} tokens)")
            rf = dict(rf or {}, **drafts)
        if shaping:
            if not getattr(llm, "supports_logit_shaping", False):
                raise HTTPException(400, f"the {getattr(llm, 'provider', 'configured')} backend cannot apply "
                                         "logit_bias / min_p")
            rf = dict(rf or {}, **shaping)
        if rep:
            if not getattr(llm, "supports_repetition_penalty", False):
                raise HTTPException(400, f"the {getattr(llm, 'provider', 'configured')} backend cannot apply "
                                         "a repetition_penalty")
            rf = dict(rf or {}, **rep)
        if pens:
            if not getattr(llm, "supports_penalties", False):
                raise HTTPException(400, f"the {getattr(llm, 'provider', 'configured')} backend cannot apply "
                                         "presence / frequency penalties")
            rf = dict(rf or {}, **pens)
        if n_lp >= 0:
            if not getattr(llm, "supports_logprobs", False):
                raise HTTPException(400, f"the {getattr(llm, 'provider', 'configured')} backend cannot provide logprobs")
            rf = dict(rf or {}, logprobs=n_lp)
        mt = body.get("max_tokens") or body.get("max_completion_tokens")
        if mt:
            rf = dict(rf or {}, max_tokens=int(mt))  # per request: the shared llm object is not mutated
        try:
            r = await llm.generate_response(messages, tools=tools, response_format=rf)
        except Exception as e:  # noqa: BLE001
            raise HTTPException(500, f"generation failed: {e}")
        cid = "chatcmpl-" + uuid.uuid4().hex[:24]
        created = int(time.time())
        finish = "tool_calls" if r.get("tool_calls") else "stop"
        msg = {"role": "assistant", "content": r["content"]}
        if r.get("tool_calls"):
            msg["tool_calls"] = r["tool_calls"]
        usage = r.get("usage", {})
        lps = None
        if n_lp >= 0:
            if r.get("logprobs") is None:
                raise HTTPException(500, "the backend returned no logprobs")
            lps = _wire_logprobs(r["logprobs"])
        extra = {"logprobs": lps} if lps is not None else {}  # only replies that asked carry the key
        if not body.get("stream"):
            return {"id": cid, "object": "chat.completion", "created": created, "model": name,
                    "choices": [{"index": 0, "message": msg, **extra, "finish_reason": finish}], "usage": usage}

        def sse():
            first = {"id": cid, "object": "chat.completion.chunk", "created": created, "model": name,
                     "choices": [{"index": 0, "delta": msg, **extra, "finish_reason": None}]}
            last = {"id": cid, "object": "chat.completion.chunk", "created": created, "model": name,
                    "choices": [{"index": 0, "delta": {}, "finish_reason": finish}], "usage": usage}
            yield f"data: {json.dumps(first)}\n\n"
            yield f"data: {json.dumps(last)}\n\n"
            yield "data: [DONE]\n\n"

        return StreamingResponse(sse(), media_type="text/event-stream")

    @app.post("/v1/score")
    async def score(body: Dict[str, Any]):
        ctx, cands, top = body.get("context"), body.get("candidates"), body.get("top_logprobs", 0)
        if isinstance(ctx, str):
            ok = len(ctx) > 0
        else:
            ok = isinstance(ctx, list) and len(ctx) > 0 and all(isinstance(m, dict) for m in ctx)
        if not ok:
            raise HTTPException(400, "context must be a non-empty string or a non-empty list of messages")
        if not isinstance(cands, list) or not cands or not all(isinstance(c, str) and c for c in cands):
            raise HTTPException(400, "candidates must be a non-empty list of non-empty strings")
        if isinstance(top, bool) or not isinstance(top, int) or not 0 <= top <= 20:
            raise HTTPException(400, "top_logprobs must be an integer between 0 and 20")
        if not getattr(llm, "supports_scoring", False):
            raise HTTPException(400, f"the {getattr(llm, 'provider', 'configured')} backend cannot score text")
        try:
            if hasattr(llm, "score_usage"):  # a backend that also reports what the call cost
                res, used = await llm.score_usage(ctx, cands, top=top)
            else:
                res, used = await llm.score(ctx, cands, top=top), {}
        except ValueError as e:
            raise HTTPException(400, str(e))
        except Exception as e:  # noqa: BLE001
            raise HTTPException(500, f"scoring failed: {e}")
        lp = lambda v: -9999.0 if v == float("-inf") or v != v else float(v)  # noqa: E731
        scores = []
        for i, r in enumerate(res):
            wire = _wire_logprobs(r["tokens"])["content"]
            for w, e in zip(wire, r["tokens"]):
                w["rank"] = e["rank"]
            scores.append({"index": i, "logprob": lp(r["logprob"]), "tokens": wire})
        pt = int(used.get("prompt_tokens", 0))
        return {"id": "score-" + uuid.uuid4().hex[:24], "object": "score", "created": int(time.time()),
                "model": name, "scores": scores,
                "usage": {"prompt_tokens": pt, "completion_tokens": 0, "total_tokens": pt,
                          "cached_prompt_tokens": int(used.get("cached_prompt_tokens", 0))}}

    @app.post("/v1/embeddings")
    async def embeddings(body: Dict[str, Any]):
        import base64

        import numpy as np

        if not getattr(llm, "supports_embeddings", False):
            raise HTTPException(400, f"the {getattr(llm, 'provider', 'configured')} backend cannot embed text")
        try:
            inputs = _embedding_inputs(body.get("input"))
            fmt = body.get("encoding_format", "float")
            if fmt not in ("float", "base64"):
                raise ValueError('encoding_format must be "float" or "base64"')
            eng = engine or getattr(llm, "engine", None)
            hidden = getattr(getattr(eng, "model_cfg", None), "hidden_size", None)
            dims = body.get("dimensions")
            if dims is not None and (isinstance(dims, bool) or not isinstance(dims, int) or dims != hidden):
                raise ValueError(f"dimensions must be the model's hidden size {hidden}")
            chunking = _chunking(body.get("chunking"))
            res = await llm.embed(inputs, chunking=chunking)
        except (NotImplementedError, ValueError) as e:
            raise HTTPException(400, str(e))
        except Exception as e:  # noqa: BLE001
            raise HTTPException(500, f"embedding failed: {e}")

        def wire(v):
            v = np.ascontiguousarray(v, dtype="<f4")
            return base64.b64encode(v.tobytes()).decode("ascii") if fmt == "base64" else [float(x) for x in v]

        data = []
        for i, r in enumerate(res):
            item = {"object": "embedding", "index": i, "embedding": wire(r["embedding"])}
            if "chunks" in r:
                item["chunks"] = [{"index": c["index"], "span": list(c["span"]), "text": c["text"],
                                   "embedding": wire(c["embedding"])} for c in r["chunks"]]
            data.append(item)
        pt = sum(int(r.get("prompt_tokens") or 0) for r in res)
        return {"object": "list", "data": data, "model": body.get("model") or name,
                "usage": {"prompt_tokens": pt, "total_tokens": pt}}

    return app


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", default="llama-3-8b")
    ap.add_argument("--host", default="127.0.0.1")
    ap.add_argument("--port", type=int, default=8000)
    ap.add_argument("--schema", action="store_true", help="model-free SchemaLLM backend (no GPU)")
    ap.add_argument("--kv-gb", type=float, default=48.0)
    ap.add_argument("--weight-quant", choices=["fp8"], default=None,
                    help="quantise the layer projections (fp8: e4m3, per-channel power-of-two scales)")
    ap.add_argument("--no-fp8-decode", dest="fp8_decode", action="store_false",
                    help="with --weight-quant fp8: keep decode steps on the bf16 kernels (no FP8 copy in HBM)")
    ap.add_argument("--host-cache-gb", type=float, default=0.0,
                    help="pinned host memory for KV blocks evicted from the prefix cache (GiB; 0 = off): "
                         "a prompt whose prefix was spilled there gets it copied back instead of recomputed")
    return ap


def main():
    a = build_parser().parse_args()
    import uvicorn

    from pilottai_amd.core.config import LLMConfig
    from pilottai_amd.engine.local_llm import LocalLLM, SchemaLLM

    if a.schema:
        llm = SchemaLLM(LLMConfig(model_name=a.model, provider="schema"))
        app = create_app(llm, a.model)
    else:
        import torch

        from pilottai_amd.engine.engine import EngineConfig, LLMEngine

        dev = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
        eng = LLMEngine(EngineConfig(model=a.model if dev.type == "cuda" else "tiny",
                                     kv_cache_gb=a.kv_gb if dev.type == "cuda" else None,
                                     num_kv_blocks=None if dev.type == "cuda" else 1024,
                                     freeze_heap=True, weight_quant=a.weight_quant,
                                     fp8_decode=a.fp8_decode, host_cache_gb=a.host_cache_gb), device=dev)
        eng.start()
        llm = LocalLLM(LLMConfig(model_name=eng.model_cfg.name, max_tokens=1024), engine=eng)
        app = create_app(llm, eng.model_cfg.name, engine=eng)
    uvicorn.run(app, host=a.host, port=a.port, log_level="warning")


if __name__ == "__main__":
    main()
