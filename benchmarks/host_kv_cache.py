"""Host KV tier (EngineConfig.host_cache_gb): what a prefix served from pinned host memory costs.

Two Llama-3-8B engines (random-init bf16, step graphs) with the same device pool, small enough
that a few long prompts evict a 2,048-token prefix: one with a host tier that keeps it, one with
the tier off. Measured:

  ttft      time to first token of a request with the 2,048-token shared prefix and a 64-token
            tail when the prefix is a miss on the engine without the tier and a full pool (a
            prompt never seen: what a request pays after eviction without the tier), the same
            miss on the engine with the tier (its ~133 new blocks each evict a block the tier
            has not seen, so ~133 spills run inside it), a device hit, and a host hit
  moves     32 blocks spilled (gather + one device-to-host copy per record) and 32 blocks filled
            (one host-to-device copy per record + scatter) through the engine's own path: device
            time between two events, the host time to issue the moves, and the GB/s achieved

Every figure is the median of --repeats runs; one JSON line per result (also appended to --out).

  python -m benchmarks.host_kv_cache --out profiles/host_kv_cache.jsonl
"""
import argparse
import json
import os
import statistics
import time

import torch

PREFIX, TAIL = 2048, 64


def _tokens(g, n):
    return torch.randint(1000, 100000, (n,), generator=g).tolist()


def _ttft(eng, prompt):
    """Wall time from submit to the first (only) token, the engine driven inline."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    o = eng.generate([prompt], temperature=0.0, max_tokens=1, ignore_eos=True)[0]
    return 1000 * (time.perf_counter() - t0), o.cached_prompt_tokens


def ttft_mode(eng, off, a, emit):
    g = torch.Generator().manual_seed(a.seed)
    P = _tokens(g, PREFIX)
    res = {"miss": [], "miss_tier_on": [], "device_hit": [], "host_hit": []}
    for _ in range(6):  # fill the pool of the engine without the tier: its misses evict, as the other's do
        off.generate([_tokens(g, PREFIX + TAIL)], temperature=0.0, max_tokens=1, ignore_eos=True)
    for rep in range(a.repeats + 1):  # the first round warms graphs and allocators up
        miss_off, cached = _ttft(off, _tokens(g, PREFIX + TAIL))
        assert cached == 0 and off.metrics()["host_spilled_blocks"] == 0
        s0 = eng.metrics()["host_spilled_blocks"]
        miss, cached = _ttft(eng, _tokens(g, PREFIX + TAIL))
        assert cached == 0
        miss_spills = eng.metrics()["host_spilled_blocks"] - s0
        eng.generate([P + _tokens(g, TAIL)], temperature=0.0, max_tokens=1, ignore_eos=True)  # P is resident now
        assert all(t == "device" for t, _ in eng.prefix_blocks(P)) and len(eng.prefix_blocks(P)) == PREFIX // 16
        dev, cached = _ttft(eng, P + _tokens(g, TAIL))
        assert cached == PREFIX, cached
        # P was reused, so it sits in the protected segment of the LRU: only other reused prefixes
        # push it out. Distinct long prompts, each served twice, until P lives in the host tier only.
        for _ in range(64):
            if all(t == "host" for t, _ in eng.prefix_blocks(P)):
                break
            f = _tokens(g, PREFIX + TAIL)
            for _ in range(2):
                eng.generate([f], temperature=0.0, max_tokens=1, ignore_eos=True)
        assert all(t == "host" for t, _ in eng.prefix_blocks(P)) and len(eng.prefix_blocks(P)) == PREFIX // 16
        h0 = eng.metrics()["host_hit_blocks"]
        host, cached = _ttft(eng, P + _tokens(g, TAIL))
        assert cached == PREFIX and eng.metrics()["host_hit_blocks"] - h0 == PREFIX // 16
        if rep:
            res["miss"].append(miss_off)
            res["miss_tier_on"].append(miss)
            res["device_hit"].append(dev)
            res["host_hit"].append(host)
    m = eng.metrics()
    emit({"bench": "host_kv_ttft", "model": a.model, "prefix_tokens": PREFIX, "tail_tokens": TAIL,
          "kv_blocks": m["total_kv_blocks"], "host_cache_blocks": m["host_cache_blocks"],
          **{f"{k}_ms": round(statistics.median(v), 3) for k, v in res.items()},
          **{f"{k}_ms_all": [round(x, 3) for x in v] for k, v in res.items()},
          "miss_tier_on_spills": miss_spills,
          "host_spilled_blocks": m["host_spilled_blocks"], "host_hit_blocks": m["host_hit_blocks"]})


def moves_mode(eng, a, emit):
    n = 32
    rec_bytes = eng._host_pool.shape[1] * 2
    eng.sched.reset_prefix_cache()  # nothing is running: every block and slot is free to overwrite
    blocks, slots = list(range(n)), list(range(n))
    res = {"spill": [], "fill": []}
    host = {"spill": [], "fill": []}
    for rep in range(a.repeats + 1):
        for kind in ("spill", "fill"):
            moves = (list(zip(blocks, slots)), []) if kind == "spill" else ([], list(zip(slots, blocks)))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            eng._execute_kv_moves(*moves)
            e1.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            if rep:
                res[kind].append(e0.elapsed_time(e1))
                host[kind].append(1000 * (t1 - t0))
    for kind in ("spill", "fill"):
        ms = statistics.median(res[kind])
        emit({"bench": "host_kv_moves", "model": a.model, "kind": kind, "blocks": n, "record_mib": rec_bytes / 2**20,
              "device_ms": round(ms, 3), "host_issue_ms": round(statistics.median(host[kind]), 3),
              "gb_per_s": round(n * rec_bytes / 1e9 / (ms / 1000), 2),
              "device_ms_all": [round(x, 3) for x in res[kind]]})


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", default="llama-3-8b")
    ap.add_argument("--kv-blocks", type=int, default=640, help="device pool: 10,240 tokens, five of the prompts")
    ap.add_argument("--host-cache-gb", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/host_kv_cache.py measures on the GPU: no device found")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    from pilottai_amd.engine.engine import EngineConfig, LLMEngine

    cfg = dict(model=a.model, max_num_seqs=8, max_num_batched_tokens=2048, max_model_len=4096,
               num_kv_blocks=a.kv_blocks, use_graphs=True)
    eng = LLMEngine(EngineConfig(host_cache_gb=a.host_cache_gb, **cfg))
    off = LLMEngine(EngineConfig(host_cache_gb=0.0, **cfg))
    try:
        ttft_mode(eng, off, a, emit)
        moves_mode(eng, a, emit)
    finally:
        eng.stop()
        off.stop()


if __name__ == "__main__":
    main()
