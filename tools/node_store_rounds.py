"""Round overhead of NodeSemanticStore at W gloo CPU ranks.

Every rank holds a shard of ROWS/W rows (dim 1024) and submits Q queries per round (k = 64) for
R rounds; reports per-round wall time, the scan's share, and the overhead outside the scan
(collectives, packing, merge), plus what an idle round costs.

    python tools/node_store_rounds.py --world 8 --queries 64 --rounds 20

`--diversity D` (0 < D <= 1) runs the same rounds with every query diverse, on stores built with
cross_shard_mmr=True: the round then also requests the merged candidates' rows from their shards
and selects over the records (two more all-to-alls; mmr_ms, mmr_rows per round), so a round's
added cost can be read next to the plain round's.

    python tools/node_store_rounds.py --world 8 --queries 64 --rounds 20 --k 5 --diversity 0.5
"""
import argparse
import json
import os
import socket
import time

import sys

import numpy as np
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _entry(rank, world, port, a, q):
    import torch
    import torch.distributed as dist

    torch.set_num_threads(1)
    from pilottai_amd.memory.node_store import NodeSemanticStore
    from pilottai_amd.memory.semantic_index import SemanticIndex

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    g = np.random.default_rng(rank)
    n = a.rows // world
    idx = SemanticIndex(dim=a.dim, capacity=n, device="cpu")
    idx.add(g.standard_normal((n, a.dim)).astype(np.float32), [0] * n, [()] * n, [None] * n)
    store = NodeSemanticStore(idx, group=dist.new_group(backend="gloo"), max_queries=a.queries,
                              cross_shard_mmr=a.diversity > 0)
    store.start()
    qs = g.standard_normal((a.queries, a.dim)).astype(np.float32)
    kw = {"diversity": a.diversity} if a.diversity > 0 else {}
    store.search_rows_blocking(qs, a.k, [0] * a.queries, [()] * a.queries, **kw)  # warm-up round
    dist.barrier()
    s0 = dict(store.stats)
    w0 = store._host.waited_s
    t0 = time.perf_counter()
    for _ in range(a.rounds):
        store.search_rows_blocking(qs, a.k, [0] * a.queries, [()] * a.queries, **kw)
    wall = time.perf_counter() - t0
    s1 = dict(store.stats)
    waited = store._host.waited_s - w0
    dist.barrier()
    # idle: time a burst of idle rounds (every rank idle)
    i0 = store.stats["idle_rounds"]
    time.sleep(1.0)
    idle_n = store.stats["idle_rounds"] - i0
    store.stop()
    rounds = s1["rounds"] - s0["rounds"]
    q.put((rank, {"rounds": rounds, "wall_ms_per_round": 1e3 * wall / a.rounds,
                  "round_ms": 1e3 * (s1["round_s"] - s0["round_s"]) / max(1, rounds),
                  "scan_ms": 1e3 * (s1["scan_s"] - s0["scan_s"]) / max(1, rounds),
                  "peer_wait_ms": 1e3 * waited / max(1, rounds),
                  "mmr_ms": 1e3 * (s1["mmr_s"] - s0["mmr_s"]) / max(1, rounds),
                  "mmr_rows": (s1["mmr_rows"] - s0["mmr_rows"]) / max(1, rounds),
                  "idle_rounds_per_s": idle_n}))
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--rows", type=int, default=80000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--diversity", type=float, default=0.0,
                    help="MMR diversity of every query (0: plain rounds; > 0: stores built with cross_shard_mmr)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    ps = [ctx.Process(target=_entry, args=(r, a.world, port, a, q)) for r in range(a.world)]
    for p in ps:
        p.start()
    got = {}
    while len(got) < a.world:
        try:
            r, v = q.get(timeout=5)
            got[r] = v
        except Exception:  # noqa: BLE001
            if any(p.exitcode not in (None, 0) for p in ps):
                raise SystemExit("a rank failed")
    for p in ps:
        p.join(60)
    per = [got[r] for r in range(a.world)]
    rec = {"world": a.world, "queries_per_rank": a.queries, "k": a.k, "rows": a.rows, "dim": a.dim,
           "round_ms_max": round(max(p["round_ms"] for p in per), 3),
           "scan_ms_max": round(max(p["scan_ms"] for p in per), 3),
           "diversity": a.diversity, "mmr_ms_max": round(max(p["mmr_ms"] for p in per), 3),
           "mmr_rows_per_round_max": round(max(p["mmr_rows"] for p in per), 1),
           "overhead_ms_max": round(max(p["round_ms"] - p["scan_ms"] for p in per), 3),
           # the round's own host work: without the scan and without waiting for slower peers
           # (on this oversubscribed 8-CPU container the peers' CPU scans skew by 10-30 ms)
           "own_overhead_ms_max": round(max(p["round_ms"] - p["scan_ms"] - p["peer_wait_ms"] for p in per), 3),
           "transport": "shm" if os.environ.get("PILOTTAI_HOST_GATHER") != "gloo" else "gloo",
           "wall_ms_per_round": round(max(p["wall_ms_per_round"] for p in per), 3),
           "idle_rounds_per_s": min(p["idle_rounds_per_s"] for p in per), "backend": "gloo-cpu"}
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
