"""Predicted Outputs over HTTP: `prediction` / `prompt_lookup` on POST /v1/chat/completions, the
usage details, streaming, the 400s, and the clients (LocalLLM, OpenAICompatLLM) -- with the tiny
CPU engine behind the server."""
import asyncio
import json
import socket
import threading
import time

import httpx
import pytest
import uvicorn

from pilottai_amd.core.config import LLMConfig
from pilottai_amd.engine.local_llm import LocalLLM, SchemaLLM, make_llm
from pilottai_amd.serving.http_server import create_app


class _Server:
    def __init__(self, app):
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        self.port = s.getsockname()[1]
        s.close()
        self.server = uvicorn.Server(uvicorn.Config(app, host="127.0.0.1", port=self.port, log_level="error"))
        self.thread = threading.Thread(target=self.server.run, daemon=True)

    def __enter__(self):
        self.thread.start()
        t0 = time.time()
        while not self.server.started:
            assert time.time() - t0 < 30, "server did not start"
            time.sleep(0.05)
        return f"http://127.0.0.1:{self.port}/v1"

    def __exit__(self, *exc):
        self.server.should_exit = True
        self.thread.join(timeout=10)


MSG = [{"role": "user", "content": "1 2 3 4 1 2 3 4 1 2 3 4 1 2 3 4"}]
BASE = {"model": "tiny", "messages": MSG, "temperature": 0.0, "max_tokens": 16}


@pytest.fixture(scope="module")
def served():
    from pilottai_amd.engine.engine import EngineConfig, LLMEngine

    eng = LLMEngine(EngineConfig(model="tiny", max_num_seqs=8, max_num_batched_tokens=256, max_model_len=256,
                                 num_kv_blocks=128, use_graphs=False), device="cpu")
    eng.start()
    backend = LocalLLM(LLMConfig(model_name="tiny", max_tokens=16, temperature=0.0), engine=eng)
    try:
        with _Server(create_app(backend, "tiny", engine=eng)) as url:
            yield url, eng, backend
    finally:
        eng.stop()


def _post(url, body):
    return httpx.post(f"{url}/chat/completions", json=body, timeout=120)


@pytest.fixture(scope="module")
def plain(served):
    """The plain reply: its text is the prediction of the tests below."""
    r = _post(served[0], BASE)
    assert r.status_code == 200
    out = r.json()
    assert out["usage"]["completion_tokens_details"] == {"accepted_prediction_tokens": 0,
                                                         "rejected_prediction_tokens": 0}
    return out["choices"][0]["message"]["content"], out["usage"]["completion_tokens"]


def test_prediction_in_both_content_forms_and_usage_details(served, plain):
    url, eng, _ = served
    text, n = plain
    assert text and n == 16
    half = len(text) // 2
    forms = [text, [{"type": "text", "text": text[:half]}, {"type": "text", "text": text[half:]}]]
    for content in forms:
        d0 = eng.metrics()["spec_draft_steps"]
        out = _post(url, dict(BASE, prediction={"type": "content", "content": content})).json()
        assert out["choices"][0]["message"]["content"] == text
        det = out["usage"]["completion_tokens_details"]
        assert set(det) == {"accepted_prediction_tokens", "rejected_prediction_tokens"}
        assert det["accepted_prediction_tokens"] > 0 and det["rejected_prediction_tokens"] >= 0
        assert out["usage"]["completion_tokens"] == n
        assert eng.metrics()["spec_draft_steps"] > d0
    h = httpx.get(url.replace("/v1", "/health")).json()["engine"]
    assert h["spec_draft_tokens"] >= h["spec_accepted_tokens"] > 0 and h["spec_draft_steps"] > 0
    assert "spec_runs_full" in h


def test_prompt_lookup_extension(served, plain):
    url, eng, _ = served
    d0 = eng.metrics()["spec_draft_tokens"]
    out = _post(url, dict(BASE, prompt_lookup=True)).json()
    assert out["choices"][0]["message"]["content"] == plain[0]
    assert eng.metrics()["spec_draft_tokens"] > d0      # the prompt repeats itself: drafts were proposed
    d1 = eng.metrics()["spec_draft_tokens"]
    out = _post(url, dict(BASE, prompt_lookup=False)).json()
    assert out["choices"][0]["message"]["content"] == plain[0] and eng.metrics()["spec_draft_tokens"] == d1


def test_streaming_carries_the_reply_and_the_details(served, plain):
    url, _, _ = served
    body = dict(BASE, stream=True, prediction={"type": "content", "content": plain[0]})
    lines = [ln for ln in _post(url, body).text.split("\n") if ln.startswith("data: ")]
    assert lines[-1] == "data: [DONE]"
    assert json.loads(lines[0][6:])["choices"][0]["delta"]["content"] == plain[0]
    det = json.loads(lines[-2][6:])["usage"]["completion_tokens_details"]
    assert det["accepted_prediction_tokens"] > 0
    lines = [ln for ln in _post(url, dict(BASE, stream=True, prompt_lookup=True)).text.split("\n")
             if ln.startswith("data: ")]
    assert json.loads(lines[0][6:])["choices"][0]["delta"]["content"] == plain[0]


@pytest.mark.parametrize("extra", [
    {"prediction": {"type": "file", "content": "x"}},
    {"prediction": "just text"},
    {"prediction": {"type": "content", "content": 7}},
    {"prediction": {"type": "content", "content": [{"type": "text", "text": 7}]}},
    {"prediction": {"type": "content", "content": [{"type": "image", "text": "x"}]}},
    {"prediction": {"type": "content", "content": ["x"]}},
    {"prompt_lookup": "yes"},
    {"prediction": {"type": "content", "content": "7 " * 300}},                      # > max_model_len tokens
    {"prediction": {"type": "content", "content": "x"}, "logprobs": True},
    {"prediction": {"type": "content", "content": "x"}, "presence_penalty": 0.5},
    {"prediction": {"type": "content", "content": "x"}, "frequency_penalty": 0.5},
    {"prediction": {"type": "content", "content": "x"}, "repetition_penalty": 1.2},
    {"prompt_lookup": True, "logprobs": True, "top_logprobs": 2},
    {"prompt_lookup": True, "repetition_penalty": 1.2},
])
def test_bad_requests_get_400(served, extra):
    url, eng, _ = served
    n0 = eng.stats["requests"]
    r = _post(url, dict(BASE, **extra))
    assert r.status_code == 400, r.text
    assert eng.stats["requests"] == n0  # nothing reached the engine


def test_model_free_backend_answers_400():
    with _Server(create_app(SchemaLLM(seed=5), "schema-test")) as url:
        for extra in ({"prediction": {"type": "content", "content": "x"}}, {"prompt_lookup": True}):
            r = _post(url, dict(BASE, **extra))
            assert r.status_code == 400 and "schema" in r.text
        assert _post(url, dict(BASE, prompt_lookup=False)).status_code == 200
        assert _post(url, dict(BASE, prediction={"type": "content", "content": ""})).status_code == 200


def test_clients_forward_both_fields(served, plain):
    url, eng, backend = served

    async def go():
        remote = make_llm(LLMConfig(provider="openai", base_url=url, model_name="tiny", retry_attempts=1,
                                    temperature=0.0, max_tokens=16, timeout=120))
        assert remote.supports_prediction and backend.supports_prediction
        body = remote._body(MSG, {"prediction": plain[0], "prompt_lookup": True}, None)
        assert body["prediction"] == {"type": "content", "content": plain[0]} and body["prompt_lookup"] is True
        assert "prediction" not in remote._body(MSG, None, None) and "prompt_lookup" not in remote._body(MSG, None, None)
        a = await remote.generate_response(MSG, response_format={"prediction": plain[0]})
        b = await backend.generate_response(MSG, response_format={"prediction": plain[0]})
        c = await backend.generate_response(MSG, response_format={"prompt_lookup": True})
        d = await backend.generate_response(MSG)
        await remote.aclose()
        return a, b, c, d

    a, b, c, d = asyncio.run(go())
    for r in (a, b, c, d):
        assert r["content"] == plain[0]
    assert a["usage"]["completion_tokens_details"]["accepted_prediction_tokens"] > 0
    assert b["usage"]["completion_tokens_details"] == a["usage"]["completion_tokens_details"]
    assert d["usage"]["completion_tokens_details"] == {"accepted_prediction_tokens": 0,
                                                       "rejected_prediction_tokens": 0}
    lookup_default = LocalLLM(LLMConfig(model_name="tiny", max_tokens=16, temperature=0.0, prompt_lookup=True),
                              engine=eng)
    assert lookup_default.prompt_lookup is True and backend.prompt_lookup is False
    with pytest.raises(RuntimeError, match="prediction"):
        asyncio.run(LocalLLM(LLMConfig(model_name="tiny", retry_attempts=1), engine=eng).generate_response(
            MSG, response_format={"prediction": 5}))
