"""Measurements of prompt scoring on one GPU (BENCHMARKS.md "Prompt scoring").

    python tools/score_bench.py kernel   # ops.score_tokens next to ops.token_logprobs, device time
    python tools/score_bench.py choose   # LocalLLM.choose against a grammar-constrained enum reply

`kernel`: [rows, 128256] bf16 logits, rows in {16, 128, 256}, n alternatives in {0, 5, 20}; the two
passes alternate, five rounds; every figure is the mean over one window of back-to-back calls
between two device events, the window sized to last about half a second.
`choose`: one Llama-3-8B engine (random init), a fresh 1,000-token chat per call, eight
single-token options (the grammar's enum takes no others); wall time of both calls.
Each prints one JSON line at the end; --out writes it to a file as well."""
import argparse
import asyncio
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pilottai_amd import ops  # noqa: E402

V = 128256


def _window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters * 1000.0  # us per call


def kernel(args):
    dev = torch.device("cuda", 0)
    out = {}
    for rows in (16, 128, 256):
        g = torch.Generator().manual_seed(rows)
        logits = (torch.randn(rows, V, generator=g) * 3).to(torch.bfloat16).to(dev)
        target = torch.randint(0, V, (rows,), generator=g, dtype=torch.int32).to(dev)
        none = torch.full((rows,), -1, dtype=torch.int32, device=dev)
        cm = torch.zeros(1, (V + 31) // 32, dtype=torch.int32, device=dev)
        sc_out = (torch.empty(rows, device=dev), torch.empty(rows, dtype=torch.int32, device=dev),
                  torch.empty(rows, 20, dtype=torch.int32, device=dev), torch.empty(rows, 20, device=dev))
        lp_out = (torch.empty(rows, device=dev), torch.empty(rows, 20, dtype=torch.int32, device=dev),
                  torch.empty(rows, 20, device=dev))
        sc_ws = ops.score_tokens_workspace(rows, V, dev)
        lp_ws = ops.token_logprobs_workspace(rows, V, dev)
        for n in (0, 5, 20):
            lp_n = torch.full((rows,), n, dtype=torch.int32, device=dev)
            fns = {"score_tokens": lambda: ops.score_tokens(logits, target, lp_n, out=sc_out, workspace=sc_ws),
                   "token_logprobs": lambda: ops.token_logprobs(logits, target, lp_n, none, none, cm, out=lp_out,
                                                                workspace=lp_ws)}
            iters = {k: max(200, int(args.window_s * 1e6 / _window(f, 200))) for k, f in fns.items()}  # + warm-up
            times = {k: [] for k in fns}
            for _ in range(args.rounds):
                for k, f in fns.items():
                    times[k].append(round(_window(f, iters[k]), 2))
            out[f"rows={rows},n={n}"] = dict(times, calls_per_window=iters)
            print(rows, n, out[f"rows={rows},n={n}"], flush=True)
    return out


def choose(args):
    from pilottai_amd.engine.engine import EngineConfig, LLMEngine
    from pilottai_amd.engine.local_llm import LocalLLM, encode_chat

    cpu = args.rehearse  # tiny model on the CPU: checks the script, measures nothing
    eng = LLMEngine(EngineConfig(model="tiny" if cpu else "llama-3-8b", max_num_seqs=64, max_num_batched_tokens=2048,
                                 kv_cache_gb=None if cpu else 8.0, num_kv_blocks=512 if cpu else None,
                                 token_buckets=[16, 64, 256, 1024, 2048]),
                    device=torch.device("cpu") if cpu else torch.device("cuda", 0))
    llm = LocalLLM({"model_name": eng.model_cfg.name, "temperature": 0.0, "max_tokens": 64, "retry_attempts": 1},
                   engine=eng)
    tok = eng.tok
    pool = ("search summary email schedule translate extract classify report memo plan write read send call stop "
            "start open close low medium high other positive neutral negative").split()
    options = [w for w in pool if len(tok.encode(w)) == 1][:8]
    assert len(options) == 8, options
    schema = {"choice": "enum(" + "|".join(options) + ")"}
    words = ("agent task report plan memory tool result quarter customer ticket latency budget review "
             "owner deadline summary context").split()

    def context(seed):
        """A chat of about 1,000 tokens that no earlier call shares a prefix with."""
        import random

        rng = random.Random(seed)
        text = f"case {seed}: "
        while True:
            text += " ".join(rng.choice(words) for _ in range(20)) + ". "
            msgs = [{"role": "user", "content": text + "\nWhich tool handles this task?"}]
            if len(encode_chat(tok, msgs)) >= 1000:
                return msgs

    async def main():
        res = {"choose_s": [], "enum_s": [], "enum_tokens": [], "choose_steps": [], "enum_steps": [], "picked": []}
        for rnd in range(args.rounds + 2):  # the first two rounds warm up (first-use graph captures)
            m, m2 = context(100 + rnd), context(200 + rnd)
            s0 = eng.stats["steps"]
            t0 = time.perf_counter()
            idx, _ = await llm.choose(m, options)
            t1 = time.perf_counter()
            s1 = eng.stats["steps"]
            r = await llm.generate_response(m2, response_format={"schema": schema, "temperature": 0.0})
            t2 = time.perf_counter()
            s2 = eng.stats["steps"]
            assert json.loads(r["content"])["choice"] in options
            print(rnd, "choose", round(t1 - t0, 4), "s", s1 - s0, "steps; enum reply", round(t2 - t1, 4), "s",
                  r["usage"]["completion_tokens"], "tokens", s2 - s1, "steps", flush=True)
            if rnd >= 2:
                res["choose_s"].append(round(t1 - t0, 5))
                res["enum_s"].append(round(t2 - t1, 5))
                res["enum_tokens"].append(r["usage"]["completion_tokens"])
                res["choose_steps"].append(s1 - s0)
                res["enum_steps"].append(s2 - s1)
                res["picked"].append(idx)
        res["context_tokens"] = len(encode_chat(tok, context(100)))
        res["options"] = options
        return res

    try:
        return asyncio.run(main())
    finally:
        eng.stop()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("what", choices=["kernel", "choose"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.5, help="kernel: seconds of back-to-back calls per figure")
    ap.add_argument("--rehearse", action="store_true", help="choose: tiny model on the CPU (no measurement)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.what == "kernel" or not a.rehearse:
        assert torch.cuda.is_available(), "this measurement needs a GPU"
    result = kernel(a) if a.what == "kernel" else choose(a)
    line = json.dumps({a.what: result})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
