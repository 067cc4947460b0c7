"""POST /v1/embeddings with the tiny CPU engine behind create_app: every input form, both
encodings, the `chunking` extension, usage, each 400, the model-free backend, and
OpenAICompatLLM.embed against the app."""
import asyncio
import base64
import socket
import threading
import time

import httpx
import numpy as np
import pytest
import uvicorn

from pilottai_amd.core.config import LLMConfig
from pilottai_amd.memory.embedding import chunk_spans, span_windows
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


@pytest.fixture(scope="module")
def served():
    from pilottai_amd.engine.engine import EngineConfig, LLMEngine
    from pilottai_amd.engine.local_llm import LocalLLM

    eng = LLMEngine(EngineConfig(model="tiny", max_num_seqs=8, max_num_batched_tokens=64, max_model_len=128,
                                 num_kv_blocks=128, use_graphs=False), device="cpu")
    eng.start()
    backend = LocalLLM(LLMConfig(model_name="tiny", max_tokens=16), engine=eng)
    try:
        with _Server(create_app(backend, "tiny", engine=eng)) as url:
            yield url, eng
    finally:
        eng.stop()


def _post(url, body):
    return httpx.post(url + "/embeddings", json=body, timeout=60)


def _vec(v):
    return np.frombuffer(base64.b64decode(v), dtype="<f4") if isinstance(v, str) else np.asarray(v, dtype=np.float32)


def test_every_input_form_and_both_encodings(served):
    url, eng = served
    text = "alpha beta gamma delta"
    ids = eng.tok.encode(text)
    want = eng.embed([ids])[0]
    want = want / np.linalg.norm(want)
    for inp, n in ((text, 1), ([text, "second text"], 2), (ids, 1), ([ids, ids[:2]], 2)):
        r = _post(url, {"input": inp, "model": "my-name"})
        assert r.status_code == 200, r.text
        d = r.json()
        assert d["object"] == "list" and d["model"] == "my-name" and len(d["data"]) == n
        assert [x["index"] for x in d["data"]] == list(range(n)) and all(x["object"] == "embedding" for x in d["data"])
        v = _vec(d["data"][0]["embedding"])
        assert v.shape == (512,) and abs(float(np.linalg.norm(v)) - 1.0) < 1e-5
        assert float(np.linalg.norm(v - want)) < 2e-2  # the engine's own vector (another batch: bf16 noise)
        assert "chunks" not in d["data"][0]
    toks = len(ids) + len(eng.tok.encode("second text"))
    d = _post(url, {"input": [text, "second text"]}).json()
    assert d["usage"] == {"prompt_tokens": toks, "total_tokens": toks} and d["model"] == "tiny"
    # float and base64 carry the same values (float32 -> JSON double -> float32 is exact)
    f = _post(url, {"input": ids, "encoding_format": "float", "dimensions": 512}).json()["data"][0]["embedding"]
    b = _post(url, {"input": ids, "encoding_format": "base64"}).json()["data"][0]["embedding"]
    assert isinstance(f, list) and isinstance(b, str) and len(base64.b64decode(b)) == 4 * 512
    assert np.array_equal(_vec(f), _vec(b)) and abs(float(np.linalg.norm(_vec(b))) - 1.0) < 1e-5


def test_chunking_output_shape_spans_and_windows(served):
    url, eng = served
    text = "The orchestrator delegates a task to worker agents and collects every result. " * 5
    ids = eng.tok.encode(text)
    assert len(ids) < 128
    spans = chunk_spans(len(ids), 16, 4)
    d = _post(url, {"input": text, "chunking": {"chunk_tokens": 16, "overlap": 4}, "encoding_format": "base64"})
    assert d.status_code == 200, d.text
    item = d.json()["data"][0]
    assert [c["index"] for c in item["chunks"]] == list(range(len(spans)))
    assert [tuple(c["span"]) for c in item["chunks"]] == spans
    assert [c["text"] for c in item["chunks"]] == [eng.tok.decode(ids[a:b]) for a, b in spans]
    emb, se = eng.embed_spans(ids, spans)
    for c, want in zip(item["chunks"], se):
        v = _vec(c["embedding"])
        assert v.shape == (512,) and float(np.linalg.norm(v - want / np.linalg.norm(want))) < 2e-2
    assert float(np.linalg.norm(_vec(item["embedding"]) - emb / np.linalg.norm(emb))) < 2e-2
    # longer than the context: windows of whole chunks, as many span requests as windows
    long_ids = (ids * 4)[:300]
    wins = span_windows(300, 16, 4, 127, 256)
    before = eng.stats["embed_requests"]
    d = _post(url, {"input": [long_ids, ids[:5]], "chunking": {"chunk_tokens": 16}})
    assert d.status_code == 200, d.text
    data = d.json()
    assert eng.stats["embed_requests"] - before == len(wins) + 1 and len(wins) > 2
    assert [tuple(c["span"]) for c in data["data"][0]["chunks"]] == chunk_spans(300, 16, 0)
    assert [tuple(c["span"]) for c in data["data"][1]["chunks"]] == [(0, 5)]
    assert data["usage"]["prompt_tokens"] == 305
    assert abs(float(np.linalg.norm(_vec(data["data"][0]["embedding"]))) - 1.0) < 1e-5
    assert eng.sched.num_free_span_slots == 256


def test_each_400(served):
    url, eng = served
    V = eng.model_cfg.vocab_size
    bad = [{}, {"input": ""}, {"input": []}, {"input": [""]}, {"input": [[]]}, {"input": ["a", [1]]},
           {"input": [1, "a"]}, {"input": 5}, {"input": [1.5]}, {"input": [True]},
           {"input": [V]}, {"input": [[3, -1]]},                      # ids outside the vocabulary
           {"input": list(range(128))},                               # max_model_len tokens without chunking
           {"input": "x", "dimensions": 64}, {"input": "x", "dimensions": "512"},
           {"input": "x", "encoding_format": "hex"},
           {"input": "x", "chunking": 16}, {"input": "x", "chunking": {}}, {"input": "x", "chunking": {"overlap": 1}},
           {"input": "x", "chunking": {"chunk_tokens": 0}}, {"input": "x", "chunking": {"chunk_tokens": 4, "overlap": 4}},
           {"input": "x", "chunking": {"chunk_tokens": 4, "overlap": -1}},
           {"input": "x", "chunking": {"chunk_tokens": 4.0}}, {"input": "x", "chunking": {"chunk_tokens": 4, "size": 1}},
           {"input": "x", "chunking": {"chunk_tokens": 200}}]         # a chunk that fits no window
    for body in bad:
        r = _post(url, body)
        assert r.status_code == 400, (body if len(str(body)) < 200 else "long", r.status_code, r.text)
    assert _post(url, {"input": list(range(127))}).status_code == 200  # the longest prompt that fits
    assert eng.sched.num_free_span_slots == 256 and eng.failed is None


def test_model_free_backend_answers_400():
    from pilottai_amd.engine.local_llm import SchemaLLM

    schema = SchemaLLM(seed=5)
    assert not schema.supports_embeddings
    with pytest.raises(NotImplementedError):
        asyncio.run(schema.embed(["x"]))
    with _Server(create_app(schema, "schema-test")) as url:
        r = _post(url, {"input": "hello"})
        assert r.status_code == 400 and "embed" in r.text


def test_openai_compat_client_embed(served):
    from pilottai_amd.engine.http_llm import OpenAICompatLLM

    url, eng = served
    ids = eng.tok.encode("alpha beta gamma delta epsilon zeta eta theta iota kappa lambda mu")

    async def go():
        llm = OpenAICompatLLM(LLMConfig(provider="openai", base_url=url, model_name="tiny", retry_attempts=1))
        assert llm.supports_embeddings
        plain = await llm.embed(["alpha beta", "gamma"]) + await llm.embed([ids])
        chunked = await llm.embed([ids], chunking={"chunk_tokens": 8, "overlap": 2})
        with pytest.raises(ValueError):
            await llm.embed([[eng.model_cfg.vocab_size]])
        with pytest.raises(ValueError):
            await llm.embed([])
        other = OpenAICompatLLM(LLMConfig(provider="openai", base_url=url, model_name="tiny"), schema_mode="openai")
        with pytest.raises(NotImplementedError):
            await other.embed([ids], chunking={"chunk_tokens": 8})
        assert len(await other.embed(["alpha"])) == 1
        await llm.aclose()
        await other.aclose()
        return plain, chunked, llm.usage

    plain, chunked, usage = asyncio.run(go())
    assert len(plain) == 3 and all(p["embedding"].shape == (512,) and p["embedding"].dtype == np.float32 for p in plain)
    assert "chunks" not in plain[0]
    spans = chunk_spans(len(ids), 8, 2)
    assert [tuple(c["span"]) for c in chunked[0]["chunks"]] == spans
    assert all(c["embedding"].shape == (512,) and abs(float(np.linalg.norm(c["embedding"])) - 1) < 1e-5
               for c in chunked[0]["chunks"])
    assert usage["prompt_tokens"] == len(eng.tok.encode("alpha beta")) + len(eng.tok.encode("gamma")) + 2 * len(ids)
