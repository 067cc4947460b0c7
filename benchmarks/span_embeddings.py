"""Cost of span pooling and of document ingestion with it (BENCHMARKS.md, "Span embeddings").

(a) The span launch: `ops.span_pool` over the final-norm rows of a 2,048-token step at the model's
    hidden size, with the segments of 256-token chunks overlapping by 32 -- device time per launch
    from a captured graph -- beside the engine's 2,048-token embedding step with and without the
    launch (one request with spans, one without, alternated in one process; HIP events around the
    step).
(b) Ingestion: an 8,000-token seeded document through `EngineEmbedder.embed_document(late=True)`
    (one prefill, every chunk a span) and through `late=False` (every chunk a request of its own:
    only code that existed before spans), alternated after a warm-up; wall time and tokens / s.

Needs a GPU; prints one JSON line.

    python -m benchmarks.span_embeddings --model llama-3-8b
"""
from __future__ import annotations

import argparse
import json
import random
import statistics
import time

import torch

from pilottai_amd import ops
from pilottai_amd.memory.embedding import EngineEmbedder, chunk_spans


def _spread(xs) -> dict:
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3), "n": len(xs)}


def _graph_us(fn, calls: int = 50, replays: int = 20) -> dict:
    """Device time per call: `calls` launches captured into one graph, per replay."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(calls):
            fn()
    out = []
    for _ in range(replays + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / calls)
    return _spread(out[2:])


def kernel_cost(dev, T: int, d: int, chunk: int, overlap: int, slots: int) -> dict:
    g = torch.Generator(device=dev).manual_seed(0)
    hn = torch.randn(T, d, device=dev, generator=g).to(torch.bfloat16)
    spans = chunk_spans(T, chunk, overlap)
    words = torch.zeros(4 * slots, dtype=torch.int32)
    for i, (a, b) in enumerate(spans):
        words[4 * i:4 * i + 4] = torch.tensor([a, b - a, i, 1], dtype=torch.int32)
    segs, n = words.to(dev), torch.tensor([len(spans)], dtype=torch.int32, device=dev)
    pool = torch.zeros(slots, d, dtype=torch.float32, device=dev)
    return {"tokens": T, "hidden": d, "segments": len(spans), "rows_read": sum(b - a for a, b in spans),
            "span_pool_device_us": _graph_us(lambda: ops.span_pool(hn, n, segs, pool))}


def _doc_ids(tok, n: int, seed: int):
    rng = random.Random(seed)
    words = ["revenue", "quarter", "agent", "memory", "costs", "region", "report", "growth", "margin", "plan",
             "the", "of", "and", "in", "for", "grew", "fell", "stayed", "flat", "while"]
    text = ""
    while len(tok.encode(text)) < n:
        text += " ".join(rng.choice(words) for _ in range(400)) + ". "
    return tok.encode(text)[:n]


def step_cost(engine, T: int, chunk: int, overlap: int, repeats: int) -> dict:
    """One T-token embedding request alone in the engine, with and without spans, alternated."""
    ids = _doc_ids(engine.tok, T, 1)
    spans = chunk_spans(T, chunk, overlap)
    runs = {"with_spans": lambda: engine.embed_spans(ids, spans), "without": lambda: engine.embed([ids])}
    for fn in runs.values():  # graph captures and allocations
        fn(), fn()
    ms = {k: [] for k in runs}
    for _ in range(repeats):
        for k, fn in runs.items():
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {"tokens": T, "spans": len(spans), "request_ms": {k: _spread(v) for k, v in ms.items()}}


def ingestion(engine, n_tokens: int, chunk: int, overlap: int, repeats: int) -> dict:
    emb = EngineEmbedder(engine, dim=1024)
    text = engine.tok.decode(_doc_ids(engine.tok, n_tokens, 2))
    n = len(engine.tok.encode(text))
    runs = {"late": lambda: emb.embed_document(text, chunk, overlap, late=True),
            "per_chunk": lambda: emb.embed_document(text, chunk, overlap, late=False)}
    chunks = len(runs["late"]()[0])
    runs["per_chunk"]()
    wall = {k: [] for k in runs}
    for _ in range(repeats):
        for k, fn in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
    return {"document_tokens": n, "chunks": chunks, "chunk_tokens": chunk, "overlap": overlap,
            "wall_ms": {k: _spread(v) for k, v in wall.items()},
            "tokens_per_s": {k: round(n / (statistics.median(v) / 1e3)) for k, v in wall.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama-3-8b")
    ap.add_argument("--step-tokens", type=int, default=2048)
    ap.add_argument("--doc-tokens", type=int, default=8000)
    ap.add_argument("--chunk-tokens", type=int, default=256)
    ap.add_argument("--overlap", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--kv-gb", type=float, default=8.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("span_embeddings needs a GPU")
    ops.require_native()
    from pilottai_amd.engine.engine import EngineConfig, LLMEngine

    dev = torch.device("cuda", torch.cuda.current_device())
    engine = LLMEngine(EngineConfig(model=a.model, kv_cache_gb=a.kv_gb, max_num_batched_tokens=a.step_tokens,
                                    max_prefill_tokens=a.step_tokens), device=dev)
    try:
        res = {"model": a.model,
               "kernel": kernel_cost(dev, a.step_tokens, engine.model_cfg.hidden_size, a.chunk_tokens, a.overlap,
                                     int(engine.L["span_slots"])),
               "step": step_cost(engine, a.step_tokens, a.chunk_tokens, a.overlap, a.repeats),
               "ingestion": ingestion(engine, a.doc_tokens, a.chunk_tokens, a.overlap, a.repeats)}
    finally:
        engine.stop()
    print(json.dumps({"span_embeddings": res}))


if __name__ == "__main__":
    main()
