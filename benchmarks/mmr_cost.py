"""Cost of the MMR re-ranking launch beside the scan it follows (BENCHMARKS.md, "MMR re-ranking").

Times, with HIP events on one stream, `ops.mmr_select` alone (Q queries x m candidates -> k picks;
eager calls, and device time per call from a captured graph of 200 calls) and the index pass
that produces its candidates (the top m of Q queries over `--rows` rows), for both storages.
Needs a GPU; prints one JSON line.

    python -m benchmarks.mmr_cost --rows 1000000 --dim 1024

`--records` times the two launches of cross-shard MMR (csrc/ops/similarity_mmr_rows.hip) on the
same Q x m candidates instead: `ops.gather_rows` of the Q m candidate rows into exchange records
(the owner's side) and `ops.mmr_select_rows` over those records (the requester's side), with the
tile kernel's `ops.mmr_select` in the same run as their yardstick.

    python -m benchmarks.mmr_cost --records --rows 100000 --dim 1024
"""
from __future__ import annotations

import argparse
import json

import torch

from pilottai_amd import ops
from pilottai_amd.memory.semantic_index import SemanticIndex


def _time_us(fn, warmup: int, iters: int) -> float:
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def _graph_us(fn, calls: int = 200, replays: int = 20) -> float:
    """Device time per call: `calls` launches captured into one graph, so the host's per-call
    work (argument checks, the Python wrapper) is not in the figure."""
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
    return _time_us(graph.replay, 2, replays) / calls


def measure(storage: str, rows: int, dim: int, Q: int, m: int, k: int, seed: int = 0) -> dict:
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev).manual_seed(seed)
    idx = SemanticIndex(dim=dim, capacity=rows, device=dev, growable=False, storage=storage)
    chunk = 1 << 16
    for r0 in range(0, rows, chunk):
        n = min(chunk, rows - r0)
        idx.add_device(torch.randn(n, dim, device=dev, generator=g), torch.zeros(n, dtype=torch.int32, device=dev),
                       torch.zeros(n, dtype=torch.int64, device=dev))
    q = torch.nn.functional.normalize(torch.randn(Q, dim, device=dev, generator=g), dim=1)
    minp = torch.zeros(Q, dtype=torch.int32, device=dev)
    qt = torch.zeros(Q, dtype=torch.int64, device=dev)
    if storage == "q16":
        scan = lambda: ops.q16_topk(q, idx.hi, idx.lo, idx.rmeta, idx.count, m, idx.priority, idx.tagbits,  # noqa: E731
                                    idx.expiry, minp, qt, 0.0)
    else:
        qb = q.to(torch.bfloat16)
        scan = lambda: ops.cosine_topk(qb, idx.packed, idx.count, m, idx.priority, idx.tagbits, idx.expiry,  # noqa: E731
                                       minp, qt, 0.0)
    s, r = scan()
    wr, wd = (t.to(dev) for t in ops.mmr_weights([0.5] * Q))
    out = (torch.empty(Q, k, device=dev), torch.empty(Q, k, dtype=torch.int32, device=dev))
    planes = idx._mmr_planes()
    rerank = lambda: ops.mmr_select(r, s, planes, k, wr, wd, out=out)  # noqa: E731
    res = {"storage": storage, "rows": rows, "dim": dim, "Q": Q, "m": m, "k": k,
           "mmr_select_us": round(_time_us(rerank, 20, 2000), 2),        # eager: bounded by the host's enqueue rate
           "mmr_select_device_us": round(_graph_us(rerank), 2),          # the launch itself
           "scan_us": round(_time_us(scan, 3, 20), 1)}
    res["candidate_bytes"] = Q * m * dim * 2
    return res


def measure_records(storage: str, rows: int, dim: int, Q: int, m: int, k: int, seed: int = 0) -> dict:
    """The record path on the scan's own Q x m candidates: gather, select over records, and the
    tile kernel on the same lists."""
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev).manual_seed(seed)
    idx = SemanticIndex(dim=dim, capacity=rows, device=dev, growable=False, storage=storage)
    chunk = 1 << 16
    for r0 in range(0, rows, chunk):
        n = min(chunk, rows - r0)
        idx.add_device(torch.randn(n, dim, device=dev, generator=g), torch.zeros(n, dtype=torch.int32, device=dev),
                       torch.zeros(n, dtype=torch.int64, device=dev))
    q = torch.nn.functional.normalize(torch.randn(Q, dim, device=dev, generator=g), dim=1)
    s, r = idx.search_tensors(q, m, [0] * Q, [0] * Q)
    torch.cuda.synchronize()
    planes = idx._mmr_planes()
    want = r.reshape(-1).contiguous()  # Q m row ids, as an owner receives them
    recs = torch.empty(Q * m, ops.record_bytes(dim, storage == "q16"), dtype=torch.uint8, device=dev)
    slot = torch.arange(Q * m, dtype=torch.int32, device=dev).view(Q, m)
    wr, wd = (t.to(dev) for t in ops.mmr_weights([0.5] * Q))
    out = (torch.empty(Q, k, device=dev), torch.empty(Q, k, dtype=torch.int32, device=dev))
    out_t = (torch.empty(Q, k, device=dev), torch.empty(Q, k, dtype=torch.int32, device=dev))
    gather = lambda: ops.gather_rows(planes, want, out=recs)  # noqa: E731
    select = lambda: ops.mmr_select_rows(recs, slot, s, k, wr, wd, out=out, q16=storage == "q16")  # noqa: E731
    tile = lambda: ops.mmr_select(r, s, planes, k, wr, wd, out=out_t)  # noqa: E731
    gather(), select(), tile()
    torch.cuda.synchronize()
    same = bool(torch.equal(torch.gather(r, 1, out[1].long().clamp(min=0)), out_t[1]) and torch.equal(out[0], out_t[0]))
    return {"storage": storage, "rows": rows, "dim": dim, "Q": Q, "m": m, "k": k,
            "gathered_rows": Q * m, "record_bytes": int(recs.shape[1]), "records_mib": round(recs.numel() / 2 ** 20, 2),
            "gather_rows_us": round(_time_us(gather, 20, 2000), 2),
            "gather_rows_device_us": round(_graph_us(gather), 2),
            "mmr_select_rows_us": round(_time_us(select, 20, 2000), 2),
            "mmr_select_rows_device_us": round(_graph_us(select), 2),
            "mmr_select_us": round(_time_us(tile, 20, 2000), 2),
            "mmr_select_device_us": round(_graph_us(tile), 2),
            "same_picks_as_tile_kernel": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--candidates", type=int, default=64)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--records", action="store_true",
                    help="time gather_rows and mmr_select_rows (cross-shard MMR) beside the tile kernel")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mmr_cost needs a GPU")
    ops.require_native()
    if a.records:
        print(json.dumps({"mmr_records_cost": [measure_records(st, a.rows, a.dim, a.queries, a.candidates, a.k)
                                               for st in ("bf16", "q16")]}))
        return
    print(json.dumps({"mmr_cost": [measure(st, a.rows, a.dim, a.queries, a.candidates, a.k) for st in ("bf16", "q16")]}))


if __name__ == "__main__":
    main()
