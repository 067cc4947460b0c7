"""`OpenAICompatLLM`: the reference's LLMHandler contract over an OpenAI-compatible HTTP API.

The reference calls providers over HTTPS through litellm (`pilott/engine/llm.py:59-120`).
Here the same protocol (generate_response / apredict / apredict_messages, with the RPM
limiter, concurrency cap and retries of `BaseLLM`) is spoken to any
`/v1/chat/completions` endpoint — typically `pilottai_amd.serving.http_server` on
another host or in another process, whose GPU engine then batches these calls with
everything else it serves.

Structured replies: agents pass `response_format={"schema": <rules.yaml name>,
"fixed": {...}}`. Against a pilottai server that is forwarded as the
`pilottai_schema` extension (grammar-constrained on the server). Against another
OpenAI-compatible server, pass `schema_mode="json_object"` to send
`{"type": "json_object"}` instead. `response_format["logprobs"] = n` (0..20) is sent as
`logprobs: true, top_logprobs: n`; the reply's `logprobs.content` comes back as `r["logprobs"]`.
`response_format["presence_penalty"]` / `["frequency_penalty"]` (or the `LLMConfig` defaults of
the same names) are sent under their OpenAI names when non-zero. `response_format["logit_bias"]`
({token id: bias}) is sent in the OpenAI wire form (keys as strings), `response_format["min_p"]`
(default `LLMConfig.min_p`) as `min_p` when non-zero, `response_format["repetition_penalty"]`
(default `LLMConfig.repetition_penalty`) as `repetition_penalty` when it is not 1.
`score()` / `choose()` call `POST /v1/score` when the server is a pilottai one.

    LLMConfig(provider="openai", base_url="http://10.0.0.5:8000/v1", api_key=...)
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional

from .local_llm import BaseLLM, _cfg_get


class OpenAICompatLLM(BaseLLM):
    provider = "openai"
    supports_logprobs = True
    supports_penalties = True
    supports_logit_shaping = True
    supports_repetition_penalty = True
    supports_embeddings = True  # POST /v1/embeddings (OpenAI's endpoint; `chunking` is a pilottai_amd extension)

    def __init__(self, config: Any = None, base_url: Optional[str] = None, timeout_s: float = 600.0,
                 schema_mode: str = "pilottai"):
        super().__init__(config)
        self.base_url = (base_url or _cfg_get(config, "base_url", None) or "http://127.0.0.1:8000/v1").rstrip("/")
        key = _cfg_get(config, "api_key", None)
        if key is not None and hasattr(key, "get_secret_value"):
            key = key.get_secret_value()
        self._headers = {"Authorization": f"Bearer {key}"} if key else {}
        self.timeout_s = float(_cfg_get(config, "timeout", timeout_s) or timeout_s)
        self.schema_mode = schema_mode
        # score() / choose() go to POST /v1/score, which only a pilottai_amd server has
        self.supports_scoring = schema_mode == "pilottai"
        self.supports_prediction = True  # `prediction` is OpenAI's field; a server may ignore it
        self._client = None

    def _http(self):
        import httpx

        if self._client is None:
            self._client = httpx.AsyncClient(timeout=self.timeout_s, headers=self._headers)
        return self._client

    async def aclose(self):
        if self._client is not None:
            await self._client.aclose()
            self._client = None

    def _body(self, messages, response_format, tools) -> Dict[str, Any]:
        rf = dict(response_format or {})
        body: Dict[str, Any] = {"model": self.model_name, "messages": list(messages),
                                "temperature": float(rf.get("temperature", self.temperature)),
                                "top_p": float(rf.get("top_p", self.top_p)),
                                "max_tokens": int(rf.get("max_tokens", self.max_tokens))}
        if rf.get("seed") is not None:
            body["seed"] = rf["seed"]
        if rf.get("logprobs") is not None and int(rf["logprobs"]) >= 0:
            body["logprobs"] = True
            body["top_logprobs"] = int(rf["logprobs"])
        for k in ("presence_penalty", "frequency_penalty"):
            v = rf.get(k, getattr(self, k))
            if v:
                body[k] = float(v)
        if rf.get("logit_bias"):
            body["logit_bias"] = {str(int(t)): float(b) for t, b in rf["logit_bias"].items()}
        mp = rf.get("min_p", self.min_p)
        if mp:
            body["min_p"] = float(mp)
        rp = rf.get("repetition_penalty", self.repetition_penalty)
        if rp is not None and float(rp) != 1.0:
            body["repetition_penalty"] = float(rp)
        # OpenAI's Predicted Outputs; prompt_lookup is a pilottai_amd server's extension
        if rf.get("prediction"):
            if not isinstance(rf["prediction"], str):
                raise ValueError("response_format['prediction'] must be a string")
            body["prediction"] = {"type": "content", "content": rf["prediction"]}
        if self.schema_mode == "pilottai" and rf.get("prompt_lookup", self.prompt_lookup):
            body["prompt_lookup"] = True
        if tools:
            body["tools"] = self._format_tools(tools)
        elif rf.get("schema") is not None:
            if self.schema_mode == "pilottai":
                body["response_format"] = {"type": "pilottai_schema", "schema": rf["schema"],
                                           "fixed": rf.get("fixed") or {}}
            else:
                body["response_format"] = {"type": "json_object"}
        return body

    async def _complete(self, messages, response_format, tools) -> Dict[str, Any]:
        r = await self._http().post(f"{self.base_url}/chat/completions",
                                    json=self._body(messages, response_format, tools))
        if r.status_code != 200:
            raise RuntimeError(f"HTTP {r.status_code}: {r.text[:300]}")
        data = r.json()
        ch = data["choices"][0]
        msg = ch.get("message") or {}
        usage = data.get("usage") or {}
        pt, ct = int(usage.get("prompt_tokens", 0)), int(usage.get("completion_tokens", 0))
        return {"content": msg.get("content") or "", "role": msg.get("role", "assistant"),
                "tool_calls": msg.get("tool_calls"), "model": data.get("model", self.model_name),
                "logprobs": (ch.get("logprobs") or {}).get("content"),
                "usage": {"prompt_tokens": pt, "completion_tokens": ct, "total_tokens": pt + ct,
                          "completion_tokens_details": {
                              k: int((usage.get("completion_tokens_details") or {}).get(k, 0))
                              for k in ("accepted_prediction_tokens", "rejected_prediction_tokens")}}}

    async def score(self, messages_or_text, candidates, top: int = 0) -> List[Dict[str, Any]]:
        """POST /v1/score of a pilottai_amd server (schema_mode "pilottai"); other OpenAI-compatible
        servers have no such endpoint, so this raises NotImplementedError for them."""
        if not self.supports_scoring:
            return await super().score(messages_or_text, candidates, top)
        ctx = messages_or_text if isinstance(messages_or_text, str) else list(messages_or_text)
        r = await self._http().post(f"{self.base_url}/score", json={"context": ctx, "candidates": list(candidates),
                                                                    "top_logprobs": int(top)})
        if r.status_code == 404:
            raise NotImplementedError(f"the server at {self.base_url} has no /score endpoint")
        if r.status_code == 400:
            raise ValueError(f"HTTP 400: {r.text[:300]}")
        if r.status_code != 200:
            raise RuntimeError(f"HTTP {r.status_code}: {r.text[:300]}")
        data = r.json()
        inf = lambda v: float("-inf") if v == -9999.0 else float(v)  # noqa: E731 -- the wire form of -inf
        out = []
        for s in sorted(data["scores"], key=lambda s: s["index"]):
            toks = [dict(t, logprob=inf(t["logprob"]),
                         top_logprobs=[dict(a, logprob=inf(a["logprob"])) for a in t.get("top_logprobs", [])])
                    for t in s["tokens"]]
            out.append({"logprob": inf(s["logprob"]), "tokens": toks})
        self.usage["calls"] += 1
        self.usage["prompt_tokens"] += int((data.get("usage") or {}).get("prompt_tokens", 0))
        return out

    async def embed(self, inputs, chunking: Optional[Dict[str, int]] = None) -> List[Dict[str, Any]]:
        """POST /v1/embeddings: one {"embedding": fp32 array, "prompt_tokens"} per input (texts or
        token id lists), vectors sent as base64 so they arrive bit for bit. `chunking`
        ({"chunk_tokens", "overlap"}, a pilottai_amd server's extension) adds each input's "chunks".
        The server reports token counts only in total, so "prompt_tokens" is None here."""
        import base64

        import numpy as np

        if isinstance(inputs, str) or not len(inputs):
            raise ValueError("inputs must be a non-empty list of texts or token id lists")
        body: Dict[str, Any] = {"model": self.model_name, "input": [x if isinstance(x, str) else list(x) for x in inputs],
                                "encoding_format": "base64"}
        if chunking is not None:
            if self.schema_mode != "pilottai":
                raise NotImplementedError("chunking is an extension of a pilottai_amd server (schema_mode 'pilottai')")
            body["chunking"] = dict(chunking)
        r = await self._http().post(f"{self.base_url}/embeddings", json=body)
        if r.status_code == 404:
            raise NotImplementedError(f"the server at {self.base_url} has no /embeddings endpoint")
        if r.status_code == 400:
            raise ValueError(f"HTTP 400: {r.text[:300]}")
        if r.status_code != 200:
            raise RuntimeError(f"HTTP {r.status_code}: {r.text[:300]}")
        data = r.json()

        def vec(v):
            return np.frombuffer(base64.b64decode(v), dtype="<f4").astype(np.float32) if isinstance(v, str) \
                else np.asarray(v, dtype=np.float32)

        out = []
        for d in sorted(data["data"], key=lambda d: d["index"]):
            item: Dict[str, Any] = {"embedding": vec(d["embedding"]), "prompt_tokens": None}
            if "chunks" in d:
                item["chunks"] = [dict(c, embedding=vec(c["embedding"])) for c in d["chunks"]]
            out.append(item)
        self.usage["calls"] += 1
        self.usage["prompt_tokens"] += int((data.get("usage") or {}).get("prompt_tokens", 0))
        return out

    async def list_models(self) -> List[str]:
        r = await self._http().get(f"{self.base_url}/models")
        r.raise_for_status()
        return [m["id"] for m in r.json().get("data", [])]
