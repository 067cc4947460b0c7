"""FP8 decode weights: what streaming half the bytes buys on decode-sized steps.

Two measurements, each alternating the variants inside one process and reporting every repeat:

  --mode gemm    per projection (Llama-3-8B or 70B layer shapes, the engine's epilogues and
                 default configs), M = 1, 8, 16: the FP8 kernel (csrc/ops/gemm_decode_fp8.hip)
                 against the bf16 kernel on the dequantised weights. Cache-cold: one hipGraph
                 holds a call per weight copy, rotating over >= 1.5 GB of bf16 copies (and the
                 same number of FP8 copies), and is replayed. Reports us per call and the
                 effective TB/s of the weight stream (weight bytes of that kernel / time).
  --mode engine  8- and 16-token decode steps of the engine in graph mode: weight_quant="fp8"
                 with fp8_decode on and off (the same quantised model) and the unquantised
                 engine, ms per step. (That the two quantised engines compute the same bits is
                 the tests' business, tests/test_fp8_decode_gpu.py, not this script's.)

    python benchmarks/fp8_decode.py --mode gemm --model 8b --out results/fp8_decode.jsonl
    python benchmarks/fp8_decode.py --mode engine --out results/fp8_decode.jsonl
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pilottai_amd import ops  # noqa: E402
from pilottai_amd.ops import reference as ref  # noqa: E402

# name -> (N, K, kind); qkv: (H, KV) heads of 128
SHAPES = {
    "8b": {"qkv": (6144, 4096, "rope", 32, 8), "o": (4096, 4096, "resid"), "gate_up": (28672, 4096, "silu"),
           "down": (4096, 14336, "resid")},
    "70b": {"qkv": (10240, 8192, "rope", 64, 8), "o": (8192, 8192, "resid"), "gate_up": (57344, 8192, "silu"),
            "down": (8192, 28672, "resid")},
}


def graph_us(fn, ncopies: int, iters: int) -> float:
    """Device us per call: a hipGraph of one call per weight copy, replayed `iters` times."""
    for i in range(2):
        fn(i % ncopies)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(ncopies):
            fn(i)
    g.replay()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        g.replay()
    e.record()
    e.synchronize()
    del g
    return s.elapsed_time(e) * 1000 / (iters * ncopies)


def gemm_mode(a, emit):
    dev = torch.device("cuda", torch.cuda.current_device())
    ops.decode_workspace(dev)
    cs = ref.rope_cos_sin(4096, 128, 500000.0).to(dev)
    for name, spec in SHAPES[a.model].items():
        N, K, kind = spec[:3]
        gb16, gb8 = N * K * 2 / 1e9, (N * K + 4 * N) / 1e9
        ncopies = max(2, int(1.5 / gb16) + 1)
        pack, pack8 = {"rope": (ops.pack_decode_qkv_rope, ops.pack_decode_qkv_rope_fp8),
                       "silu": (ops.pack_decode_gate_up, ops.pack_decode_gate_up_fp8),
                       "resid": (ops.pack_decode_weight, ops.pack_decode_weight_fp8)}[kind]
        wps, wp8s, sps = [], [], []
        for c in range(ncopies):
            w = (torch.randn(N, K, device=dev) * 0.02).to(torch.bfloat16)
            q, s = ops.quantize_fp8_rows(w)
            del w
            wps.append(pack(ops.dequantize_fp8_rows(q, s)))
            w8, sp = pack8((q, s))
            wp8s.append(w8)
            sps.append(sp)
            del q, s
        for M in a.rows:
            x = torch.randn(M, K, device=dev).to(torch.bfloat16)
            if kind == "rope":
                H, KV = spec[3], spec[4]
                qo = torch.empty(M, H, 128, dtype=torch.bfloat16, device=dev)
                kc = torch.zeros(4, KV, 16, 16, 8, dtype=torch.bfloat16, device=dev)
                vc = torch.zeros(4, KV, 128, 16, dtype=torch.bfloat16, device=dev)
                pos = torch.arange(M, dtype=torch.int32, device=dev)
                slots = torch.arange(M, dtype=torch.int32, device=dev)
                f16 = lambda i: ops.decode_qkv_rope(x, wps[i], 1e-5, qo, kc, vc, pos, slots, cs, H, KV)  # noqa: E731
                f8 = lambda i: ops.decode_qkv_rope_fp8(x, wp8s[i], sps[i], 1e-5, qo, kc, vc, pos, slots, cs,  # noqa: E731
                                                       H, KV)
                outs = lambda: (qo.clone(), kc.clone(), vc.clone())  # noqa: E731
            else:
                NO = N // 2 if kind == "silu" else N
                y = torch.empty(M, NO, dtype=torch.bfloat16, device=dev)
                resid = torch.randn(M, N, device=dev).to(torch.bfloat16) if kind == "resid" else None
                kw = dict(norm=kind == "silu", resid=resid, out=y)
                f16 = lambda i: ops.decode_gemm(x, wps[i], kind, **kw)  # noqa: E731
                f8 = lambda i: ops.decode_gemm_fp8(x, wp8s[i], sps[i], kind, **kw)  # noqa: E731
                outs = lambda: (y.clone(),)  # noqa: E731
            f16(0)
            r16 = outs()
            f8(0)
            r8 = outs()
            same = all(torch.equal(p.view(torch.int16), q.view(torch.int16)) for p, q in zip(r16, r8))
            t16, t8 = [], []
            for _ in range(a.repeats):  # alternating
                t16.append(graph_us(f16, ncopies, a.iters))
                t8.append(graph_us(f8, ncopies, a.iters))
            m16, m8 = statistics.median(t16), statistics.median(t8)
            emit({"bench": "fp8_decode_gemm", "model": a.model, "proj": name, "N": N, "K": K, "epi": kind, "M": M,
                  "copies": ncopies, "bit_identical": same,
                  "bf16_us": round(m16, 2), "bf16_us_all": [round(t, 2) for t in t16],
                  "fp8_us": round(m8, 2), "fp8_us_all": [round(t, 2) for t in t8],
                  "bf16_TBps": round(gb16 / m16 * 1e3, 2), "fp8_TBps": round(gb8 / m8 * 1e3, 2),
                  "speedup": round(m16 / m8, 3)})
        del wps, wp8s, sps
        torch.cuda.empty_cache()


def _decode_run(eng, prompts, gen: int):
    """ms per step of one generation of all prompts together (prefilled by a request before)."""
    eng.generate(prompts, temperature=0.0, max_tokens=1, ignore_eos=True)
    st0 = dict(eng.stats)
    done, ids = {}, []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for p in prompts:
        ids.append(eng.submit(p, lambda o: done.__setitem__(o.request_id, o), temperature=0.0, max_tokens=gen,
                              ignore_eos=True))
    while len(done) < len(ids):
        if not eng.step() and not eng.sched.has_work() and eng._inbox.empty():
            break
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    steps = eng.stats["steps"] - st0["steps"]
    return {"ms_per_step": round(1000 * (eng.stats["busy_s"] - st0["busy_s"]) / max(1, steps), 4),
            "wall_ms_per_step": round(1000 * dt / max(1, steps), 4), "steps": steps}


def engine_mode(a, emit):
    from pilottai_amd.engine.engine import EngineConfig, LLMEngine

    variants = {"fp8_decode": dict(weight_quant="fp8", fp8_decode=True),
                "fp8_on_bf16_kernels": dict(weight_quant="fp8", fp8_decode=False),
                "unquantised": dict()}
    engines = {}
    for k, kw in variants.items():
        t0 = time.time()
        engines[k] = LLMEngine(EngineConfig(model=a.engine_model, max_num_seqs=16, max_num_batched_tokens=2048,
                                            max_model_len=4096, kv_cache_gb=a.kv_gb, use_graphs=True, **kw))
        m = engines[k].metrics()
        emit({"bench": "fp8_decode_engine_load", "variant": k, "model": a.engine_model,
              "weights_gb": round(m["weights_gb"], 3), "load_s": round(time.time() - t0, 1)})
    tok = next(iter(engines.values())).tok
    for rows in a.rows:
        if rows < 2:
            continue
        prompts = [tok.encode(f"Request {i}: summarise the quarterly report of unit {i} in detail. " * 8)
                   for i in range(rows)]
        res = {k: [] for k in engines}
        for _ in range(a.repeats):  # alternating
            for k, e in engines.items():
                r = _decode_run(e, prompts, a.gen)
                res[k].append(r)
        emit({"bench": "fp8_decode_engine", "model": a.engine_model, "rows": rows, "gen": a.gen,
              **{k: {"ms_per_step": statistics.median(r["ms_per_step"] for r in v),
                     "ms_per_step_all": [r["ms_per_step"] for r in v],
                     "wall_ms_per_step_all": [r["wall_ms_per_step"] for r in v], "steps": v[0]["steps"]}
                 for k, v in res.items()}})
    for e in engines.values():
        e.stop()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mode", choices=["gemm", "engine"], required=True)
    ap.add_argument("--model", choices=list(SHAPES), default="8b", help="layer shapes of --mode gemm")
    ap.add_argument("--engine-model", default="llama-3-8b")
    ap.add_argument("--rows", default="1,8,16", help="M of --mode gemm / decode rows per step of --mode engine")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20, help="graph replays per repeat (gemm)")
    ap.add_argument("--gen", type=int, default=96, help="decode steps per repeat (engine)")
    ap.add_argument("--kv-gb", type=float, default=8.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    a.rows = [int(r) for r in a.rows.split(",")]
    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/fp8_decode.py measures on the GPU: no device found")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    (gemm_mode if a.mode == "gemm" else engine_mode)(a, emit)


if __name__ == "__main__":
    main()
