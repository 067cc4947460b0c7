"""Predicted outputs: what draft steps buy on the serving model (BENCHMARKS.md, "Predicted outputs").

Llama-3-8B with random-init weights, N concurrent requests over a 600-token prompt each, 128
greedy tokens. Three arms per draft length K:
  (a) plain            no prediction (K plays no part: measured once per N)
  (b) prediction       the run's own output as the prediction: the acceptance ceiling
  (c) prediction / 8   the same prediction with every 8th token replaced
Random-init weights leave the greedy choice nearly tied at most positions, so a drafted run --
other attention item shapes, other GEMM row counts -- soon leaves the plain run's tokens (the
kernel-path caveat of the README) and no fixed text stays a prediction of it: measured, the plain
output is followed for a few tokens at 8 and 32 requests. What a step costs does not depend on
which tokens it carries, so every request of every arm gets a `logit_bias` of +100 on one token of
its own: the reply is that token 128 times on every kernel path, the plain arm pays the same
bias launch, and acceptance is exactly what the prediction's text allows. (Arm (c) then resyncs
at once -- the last four tokens always occur in the prediction -- where real text needs two
matching tokens first.)
For every (N, arm, K): tokens/s over the generation, engine steps, steps with draft rows, draft
tokens proposed / accepted, and milliseconds per step (host clock around steps that end in a
device synchronise). `--verify-launch` also times the acceptance launch alone (ops.spec_verify
beside the sampler's final merge it replaces), device time per call from a captured graph.
Needs a GPU; prints one JSON line per measurement.

    python -m benchmarks.predicted_outputs --model llama-3-8b --concurrency 1 8 32 --draft-len 1 3 7
"""
from __future__ import annotations

import argparse
import json
import time

import torch

from pilottai_amd import ops
from pilottai_amd.engine.engine import EngineConfig, LLMEngine


def _prompts(n: int, length: int, vocab: int, seed: int):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(1000, vocab - 1000, (length,), generator=g).tolist() for _ in range(n)]


def _run(eng: LLMEngine, prompts, gen: int, predictions=None, draft_len=None):
    """One timed generation of all prompts together. The prompts are prefilled first by a request
    of their own (prefix cache), so the window is decode work."""
    eng.generate(prompts, temperature=0.0, max_tokens=1, ignore_eos=True)
    st0, m0 = dict(eng.stats), eng.metrics()
    done, ids = {}, []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i, p in enumerate(prompts):
        kw = dict(logit_bias={5000 + i: 100.0})
        if predictions is not None:
            kw.update(prediction=predictions[i], draft_len=draft_len)
        ids.append(eng.submit(p, lambda o: done.__setitem__(o.request_id, o), temperature=0.0, max_tokens=gen,
                              ignore_eos=True, **kw))
    while len(done) < len(ids):
        if not eng.step() and not eng.sched.has_work() and eng._inbox.empty():
            break
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    m1 = eng.metrics()
    outs = [done[i] for i in ids]
    steps = eng.stats["steps"] - st0["steps"]
    toks = sum(len(o.token_ids) for o in outs)
    return outs, {
        "seconds": round(dt, 4), "tokens": toks, "tokens_per_s": round(toks / dt, 1), "steps": steps,
        "ms_per_step": round(1000 * (eng.stats["busy_s"] - st0["busy_s"]) / max(1, steps), 3),
        "draft_steps": m1["spec_draft_steps"] - m0["spec_draft_steps"],
        "draft_tokens": m1["spec_draft_tokens"] - m0["spec_draft_tokens"],
        "accepted_tokens": m1["spec_accepted_tokens"] - m0["spec_accepted_tokens"],
        "runs_full": m1["spec_runs_full"] - m0["spec_runs_full"],
        "graph_captures": eng.stats["graph_captures"] - st0["graph_captures"]}


def _graph_us(fn, calls: int = 200, replays: int = 20) -> float:
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
    for _ in range(2):
        graph.replay()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(replays):
        graph.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / (replays * calls)


def verify_launch(rows: int, vocab: int, run_len: int):
    """Device time of ops.spec_verify over `rows` rows in runs of `run_len` (all accepted: the
    longest walk), and of ops.sample over the same rows (chunk pass + final merge) with
    ops.sample_partials (chunk pass alone) for the difference."""
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev).manual_seed(0)
    logits = torch.randn(rows, vocab, device=dev, generator=g).bfloat16()
    zi = torch.zeros(rows, dtype=torch.int32, device=dev)
    temp = torch.zeros(rows, dtype=torch.float32, device=dev)
    mc = torch.full((rows,), -1, dtype=torch.int32, device=dev)
    masks = torch.zeros(1, (vocab + 31) // 32, dtype=torch.int32, device=dev)
    seeds = torch.zeros(rows, dtype=torch.int64, device=dev)
    forced = torch.full((rows,), -1, dtype=torch.int32, device=dev)
    ws = ops.sample_workspace(rows, vocab, dev)
    out, acc = torch.zeros(rows, dtype=torch.int32, device=dev), torch.zeros(rows, dtype=torch.int32, device=dev)
    first = (torch.arange(rows, device=dev, dtype=torch.int32) // run_len) * run_len
    length = torch.minimum(torch.full_like(first, run_len), rows - first)
    lr = torch.arange(rows, device=dev, dtype=torch.int32)
    pk, pi = ops.sample_partials(logits, temp, mc, masks, seeds, zi, workspace=ws)
    toks = ops.sample(logits, temp, mc, masks, seeds, zi, forced, workspace=ws)
    ids = torch.roll(toks, 1).contiguous()  # row j + 1's input = row j's token: everything is accepted
    full = _graph_us(lambda: ops.sample(logits, temp, mc, masks, seeds, zi, forced, out=out, workspace=ws))
    chunk = _graph_us(lambda: ops.sample_partials(logits, temp, mc, masks, seeds, zi, workspace=ws))
    ver = _graph_us(lambda: ops.spec_verify(pk, pi, forced, ids, lr, first, length, out_tokens=out, accept_len=acc))
    return {"bench": "spec_verify_launch", "rows": rows, "vocab": vocab, "run_len": run_len,
            "spec_verify_us": round(ver, 2), "sample_us": round(full, 2), "sample_chunk_pass_us": round(chunk, 2),
            "sample_final_merge_us": round(full - chunk, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama-3-8b")
    ap.add_argument("--concurrency", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--draft-len", type=int, nargs="+", default=[1, 3, 7])
    ap.add_argument("--prompt-tokens", type=int, default=600)
    ap.add_argument("--gen-tokens", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=2, help="timed runs per arm (the first also warms the graphs)")
    ap.add_argument("--verify-launch", action="store_true")
    ap.add_argument("--kv-gb", type=float, default=8.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("benchmarks.predicted_outputs needs a GPU")
    ops.require_native()
    eng = LLMEngine(EngineConfig(model=a.model, max_num_seqs=max(64, 8 * max(a.concurrency)),
                                 max_num_batched_tokens=2048, max_model_len=2048, kv_cache_gb=a.kv_gb, seed=1234),
                    device=torch.device("cuda", torch.cuda.current_device()))
    V = eng.model_cfg.vocab_size
    if a.verify_launch:
        for rows, rl in ((4, 4), (32, 4), (64, 4), (64, 8), (64, 1)):
            print(json.dumps(verify_launch(rows, V, rl)), flush=True)
    for n in a.concurrency:
        prompts = _prompts(n, a.prompt_tokens, V, seed=100 + n)
        best = None
        for _ in range(a.repeats + 1):  # the first run is the warm-up
            outs, r = _run(eng, prompts, a.gen_tokens)
            best = r if best is None or r["tokens_per_s"] > best["tokens_per_s"] else best
        plain = [o.token_ids for o in outs]
        print(json.dumps(dict(bench="predicted_outputs", model=a.model, concurrency=n, arm="plain", K=0, **best)),
              flush=True)
        wrong = [[(t + 1) % V if i % 8 == 7 else t for i, t in enumerate(p)] for p in plain]
        for K in a.draft_len:
            for arm, preds in (("prediction", plain), ("prediction_every_8th_wrong", wrong)):
                best, same = None, True
                for _ in range(a.repeats + 1):
                    outs, r = _run(eng, prompts, a.gen_tokens, preds, K)
                    same = same and all(o.token_ids == p for o, p in zip(outs, plain))
                    best = r if best is None or r["tokens_per_s"] > best["tokens_per_s"] else best
                print(json.dumps(dict(bench="predicted_outputs", model=a.model, concurrency=n, arm=arm, K=K,
                                      tokens_equal_plain=same, **best)), flush=True)
    eng.stop()


if __name__ == "__main__":
    main()
