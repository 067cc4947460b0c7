"""Cross-shard MMR on the node-wide store and the sharded index (memory/node_store.py
cross_shard_mmr=True, ShardedSemanticIndex(cross_shard_mmr=True)) over gloo ranks on CPU.

Every expectation comes from ONE SemanticIndex holding all rows (the same global row ids) or from
ops.reference: a diverse search from any rank returns the rows SemanticIndex.search(diversity=)
returns, in the same order (q16: the same scores bit for bit; bf16: within the 1e-6 of the plain
node test, the candidate scores of every query being more than 1e-5 apart so that a last-bit
difference between shard scans cannot reorder a list).
"""
import asyncio
import os
import queue
import socket
import time
import traceback

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from pilottai_amd.memory.semantic_index import SemanticIndex, ShardedSemanticIndex
from pilottai_amd.ops import reference as ref

DIM, PER, CLUSTERS = 64, 12, 100
N = PER * CLUSTERS  # 1,200 rows; a cluster's members have consecutive global ids: different shards
SEED = 156  # chosen so that test_the_data_separates_adjacent_candidates holds for bf16

# one round's worth of queries: (cluster the query is near, k, min_priority, tags, diversity, fetch_k)
CASES = [
    (0, 3, 0, (), 0.0, None),          # plain queries in a diverse round
    (1, 6, 0, (), 0.0, 64),
    (2, 1, 0, (), 0.3, None),
    (3, 3, 0, (), 0.3, None),
    (4, 6, 0, (), 0.7, None),
    (5, 3, 0, (), 0.7, 64),
    (6, 6, 0, (), 1.0, 64),
    (7, 3, 0, (), 1.0, 7),
    (8, 3, 0, ("even",), 0.5, None),   # tag filter
    (9, 6, 3, (), 0.5, 30),            # priority filter
    (10, 6, 2, ("odd", "x3"), 0.7, None),
    (11, 6, 0, ("rare",), 0.5, 64),    # 13 rows carry the tag: fewer hits than fetch_k
    (12, 3, 0, ("nosuch",), 0.5, None),  # no hit at all
    (13, 3, 99, (), 0.3, None),        # no row has the priority
]
K = [c[1] for c in CASES]
MINP = [c[2] for c in CASES]
TAGS = [c[3] for c in CASES]
DIV = [c[4] for c in CASES]
FETCH = [c[5] for c in CASES]

# the tie data: exact copies of one row on different shards (world 2 and world 4)
TIE_N, TIE_COPIES, TIE_K, TIE_FETCH, TIE_DIV = 240, [6, 7, 9, 12, 131], 6, 8, 0.5


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _data():
    """Near-duplicate clusters: a base row plus small distinct perturbations."""
    g = np.random.default_rng(SEED)
    base = g.standard_normal((CLUSTERS, DIM)).astype(np.float32)
    vecs = np.repeat(base, PER, axis=0) + 0.12 * g.standard_normal((N, DIM)).astype(np.float32)
    prio = [int(i % 5) for i in range(N)]
    tags = [({"even"} if i % 2 == 0 else {"odd"}) | ({"x3"} if i % 3 == 0 else set()) |
            ({"rare"} if i % 97 == 0 else set()) for i in range(N)]
    queries = np.stack([base[c[0]] for c in CASES]) + 0.05 * g.standard_normal((len(CASES), DIM)).astype(np.float32)
    return vecs, prio, tags, queries.astype(np.float32)


def _tie_data():
    """Five copies of the unit vector e_0 (its score is the query's first component whatever the
    order of the accumulation, so the copies tie exactly on every shard) among random rows; the
    query is near e_0, so the tie group leads the candidate list."""
    g = np.random.default_rng(11)
    vecs = g.standard_normal((TIE_N, DIM)).astype(np.float32)
    for r in TIE_COPIES:
        vecs[r] = 0.0
        vecs[r, 0] = 1.0
    q = 0.1 * g.standard_normal((1, DIM)).astype(np.float32)
    q[0, 0] = 1.0
    return vecs, q


def _shard(vecs, prio, tags, rank, world, storage):
    local = SemanticIndex(dim=DIM, capacity=64, device="cpu", storage=storage)
    mine = list(range(rank, len(vecs), world))  # global row g = local_row * world + rank
    local.add(vecs[mine], [prio[i] for i in mine], [tags[i] for i in mine], [None] * len(mine))
    return local


def _entry(rank, world, port, storage, q):
    import torch.distributed as dist

    from pilottai_amd.memory.enhanced_memory import MemoryItem
    from pilottai_amd.memory.node_store import NodeSemanticStore

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        vecs, prio, tags, queries = _data()
        local = _shard(vecs, prio, tags, rank, world, storage)
        grp = dist.new_group(backend="gloo")
        store = NodeSemanticStore(local, group=grp, cross_shard_mmr=True)
        # count the all-to-alls of every round
        per_round, inner_x, inner_r = [], store._exchange, store._round

        def counted_exchange(t):
            per_round[-1] += 1
            return inner_x(t)

        def counted_round():
            per_round.append(0)
            return inner_r()

        store._exchange, store._round = counted_exchange, counted_round
        store.start()
        out = {}
        # 1) a busy round without a diverse query: two exchanges, no MMR round
        store.search_rows_blocking(queries[:3], 3, [0] * 3, [()] * 3)
        dist.barrier()
        out["plain_counts"] = sorted(set(c for c in per_round if c))
        out["plain_mmr_rounds"] = store.stats["mmr_rounds"]
        dist.barrier()
        # 2) one diverse query from rank 0 only: one busy round on every rank, four exchanges
        if rank == 0:
            store.search_rows_blocking(queries[2:3], 3, [0], [()], diversity=0.5)
        dist.barrier()
        # (every busy round so far, in order: a round's entry is appended when the round starts,
        # which may be long before its header gather completes, so positions say nothing)
        out["div_counts"] = [c for c in per_round if c]
        out["div_mmr_rounds"] = store.stats["mmr_rounds"]
        dist.barrier()
        # 3) the mixed round, from every rank
        out["mixed"] = store.search_rows_blocking(queries, K, MINP, TAGS, diversity=DIV, fetch_k=FETCH)
        out["mmr_rows"] = store.stats["mmr_rows"]
        dist.barrier()
        # 4) lockstep: rank 0 asks plain queries only, rank 1 nothing, the others diverse ones
        #    (world 2: rank 1 asks the diverse ones in a second step while rank 0 asks nothing)
        if rank == 0:
            out["lock_plain"] = store.search_rows_blocking(queries[:2], 3, [0] * 2, [()] * 2)
        elif rank >= 2:
            out["lock_div"] = store.search_rows_blocking(queries[3:5], 3, [0] * 2, [()] * 2, diversity=0.6)
        dist.barrier()
        if rank == 1:
            out["lock_div"] = store.search_rows_blocking(queries[3:5], 3, [0] * 2, [()] * 2, diversity=0.6)
        dist.barrier()
        # 5) a row written on the last rank is picked by a diverse search from rank 0
        probe = queries[0] * 3.0
        if rank == world - 1:
            out["written"] = store.store_rows_blocking(
                probe[None], [MemoryItem(text="finding from the last rank", tags={"fresh"}, priority=4)])[0]
        dist.barrier()
        if rank == 0:
            out["probe"] = store.search_rows_blocking(probe[None], 3, [0], [()], diversity=0.5)[0]
        dist.barrier()
        store.stop()
        # 6) ties: copies of one row on different shards
        tv, tq = _tie_data()
        tstore = NodeSemanticStore(_shard(tv, [0] * TIE_N, [set()] * TIE_N, rank, world, storage), group=grp,
                                   cross_shard_mmr=True)
        tstore.start()
        out["ties"] = tstore.search_rows_blocking(tq, TIE_K, [0], [()], diversity=TIE_DIV, fetch_k=TIE_FETCH)[0]
        dist.barrier()
        tstore.stop()
        # 7) the sharded index, collectively with the same queries
        if world == 2:
            sh = ShardedSemanticIndex(_shard(vecs, prio, tags, rank, world, storage), grp, cross_shard_mmr=True)
            out["sharded"] = sh.search(queries, 3, MINP, TAGS, diversity=DIV, fetch_k=16)
            dist.barrier()
        q.put((rank, out))
    except BaseException:
        q.put((rank, {"error": traceback.format_exc()}))
        raise
    finally:
        dist.destroy_process_group()


def _spawn_ranks(target, world, args, budget_s=240.0):
    """Start `world` ranks of `target(rank, world, port, *args, queue)` and collect {rank: result}.
    A rank that reports an error or dies ends the wait at once -- its peers would otherwise sit in
    a collective until that times out -- and whatever is still running is killed."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port) + tuple(args) + (q,)) for r in range(world)]
    for p in procs:
        p.start()
    got = {}
    deadline = time.monotonic() + budget_s
    try:
        while len(got) < world:
            try:
                r, v = q.get(timeout=0.5)
            except queue.Empty:
                dead = [(i, p.exitcode) for i, p in enumerate(procs) if p.exitcode not in (None, 0)]
                assert not dead, f"ranks died (rank, exit code): {dead}"
                assert time.monotonic() < deadline, "the ranks did not answer in time"
                continue
            assert not (isinstance(v, dict) and "error" in v), f"rank {r} failed:\n{v['error']}"
            got[r] = v
        for p in procs:
            p.join(timeout=60)
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
                p.join(timeout=10)
    assert [p.exitcode for p in procs] == [0] * world
    return got


_SINGLE = {}


def _single(storage):
    """The one index holding all rows, and everything expected of the stores (computed once)."""
    if storage not in _SINGLE:
        vecs, prio, tags, queries = _data()
        idx = SemanticIndex(dim=DIM, capacity=2048, device="cpu", storage=storage)
        idx.add(vecs, prio, tags, [None] * N)
        Q = len(CASES)
        exp = {"mixed": [idx.search(queries[i:i + 1], K[i], [MINP[i]], [TAGS[i]], diversity=DIV[i],
                                    fetch_k=FETCH[i])[0] for i in range(Q)],
               "plain": [idx.search(queries[i:i + 1], K[i], [MINP[i]], [TAGS[i]])[0] for i in range(Q)],
               "cands": idx.search(queries, 64, MINP, TAGS),
               "sharded": idx.search(queries, 3, MINP, TAGS, diversity=DIV, fetch_k=16),
               "lock_plain": idx.search(queries[:2], 3, [0] * 2, [()] * 2),
               "lock_div": idx.search(queries[3:5], 3, [0] * 2, [()] * 2, diversity=0.6)}
        tv, tq = _tie_data()
        tidx = SemanticIndex(dim=DIM, capacity=256, device="cpu", storage=storage)
        tidx.add(tv, [0] * TIE_N, [set()] * TIE_N, [None] * TIE_N)
        cand = sorted(tidx.search(tq, TIE_FETCH, [0], [()])[0], key=lambda rs: (-rs[1], rs[0]))
        rows = torch.tensor([r for r, _ in cand])
        sims = ref.q16_pairwise(tidx.hi, tidx.lo, tidx.rmeta, rows) if storage == "q16" \
            else ref.bf16_pairwise(tidx.packed, rows)
        s, r = ref.mmr_select(torch.tensor([s for _, s in cand]), rows, sims, TIE_K, np.float32(1 - TIE_DIV),
                              np.float32(TIE_DIV))
        exp["tie_cands"] = cand
        exp["ties"] = list(zip(r.tolist(), s.tolist()))
        _SINGLE[storage] = exp
    return _SINGLE[storage]


def _same(got, want, storage):
    assert [r for r, _ in got] == [r for r, _ in want], (got, want)
    if storage == "q16":
        assert [s for _, s in got] == [s for _, s in want]
    else:
        np.testing.assert_allclose([s for _, s in got], [s for _, s in want], rtol=0, atol=1e-6)


_RUNS = {}


def _run(world, storage):
    """One spawned run per (world, storage), shared by the tests; a failed run is remembered and
    fails every test that needs it without being started again."""
    if (world, storage) not in _RUNS:
        try:
            _RUNS[(world, storage)] = _spawn_ranks(_entry, world, (storage,))
        except BaseException as e:  # noqa: BLE001
            _RUNS[(world, storage)] = e
            raise
    if isinstance(_RUNS[(world, storage)], BaseException):
        raise AssertionError(f"the world-{world} {storage} run failed: {_RUNS[(world, storage)]}")
    return _RUNS[(world, storage)]


@pytest.mark.parametrize("storage", ["bf16", "q16"])
def test_the_data_separates_adjacent_candidates(storage):
    """bf16: no two adjacent candidates of a query -- its top fetch_k (a plain query: its top k),
    and the first row left out -- are within 1e-5 (the seed is chosen so), and the cases really
    exercise short and empty lists."""
    exp = _single(storage)
    if storage == "bf16":
        for i, lst in enumerate(exp["cands"]):
            fk = (FETCH[i] or min(64, 4 * K[i])) if DIV[i] > 0 else K[i]
            s = np.array([sc for _, sc in lst[:fk + 1]], dtype=np.float64)
            assert len(s) < 2 or np.min(s[:-1] - s[1:]) > 1e-5
    assert len(exp["cands"][11]) == 13 and exp["cands"][12] == [] and exp["cands"][13] == []
    # diversity changes something: the diverse picks are not the plain top-k everywhere
    assert any(exp["mixed"][i] != exp["plain"][i] for i in range(len(CASES)) if DIV[i] > 0)
    # the tie group lies wholly inside the top fetch_k, at its head
    assert [r for r, _ in exp["tie_cands"][:len(TIE_COPIES)]] == TIE_COPIES
    assert len({s for _, s in exp["tie_cands"][:len(TIE_COPIES)]}) == 1
    assert exp["tie_cands"][len(TIE_COPIES)][1] < exp["tie_cands"][0][1]


@pytest.mark.parametrize("storage", ["bf16", "q16"])
@pytest.mark.parametrize("world", [2, 4])
def test_node_store_diverse_search_equals_one_index(world, storage):
    got, exp = _run(world, storage), _single(storage)
    for r in range(world):
        assert len(got[r]["mixed"]) == len(CASES)
        for i in range(len(CASES)):
            _same(got[r]["mixed"][i], exp["mixed"][i], storage)
            if DIV[i] == 0:  # a diversity-0 query in a diverse round: the plain top-k
                _same(got[r]["mixed"][i], exp["plain"][i], storage)
        assert got[r]["mmr_rows"] > 0
    # lockstep: plain-only, idle and diverse ranks in the same rounds all complete
    for lst, want in zip(got[0]["lock_plain"], exp["lock_plain"]):
        _same(lst, want, storage)
    for r in range(1, world):
        for lst, want in zip(got[r]["lock_div"], exp["lock_div"]):
            _same(lst, want, storage)
    # a write on the last rank, picked by a diverse search from rank 0
    w = got[world - 1]["written"]
    assert w % world == world - 1 and w in [row for row, _ in got[0]["probe"]]


@pytest.mark.parametrize("storage", ["bf16", "q16"])
@pytest.mark.parametrize("world", [2, 4])
def test_collectives_per_round(world, storage):
    got = _run(world, storage)
    for r in range(world):
        assert got[r]["plain_counts"] == [2] and got[r]["plain_mmr_rounds"] == 0
        busy = got[r]["div_counts"]  # the plain rounds, then the one round with a diverse query
        assert busy[-1] == 4 and set(busy[:-1]) == {2} and got[r]["div_mmr_rounds"] == 1, busy


@pytest.mark.parametrize("storage", ["bf16", "q16"])
def test_ties_do_not_depend_on_the_shard_count(storage):
    exp = _single(storage)
    a, b = _run(2, storage), _run(4, storage)
    for world, got in ((2, a), (4, b)):
        for r in range(world):
            _same(got[r]["ties"], exp["ties"], storage)
    assert [r for r, _ in a[0]["ties"]] == [r for r, _ in b[0]["ties"]]
    if storage == "q16":
        assert a[0]["ties"] == b[0]["ties"]
    # the selection walked into the tie group: copies beyond the first are among the picks
    assert len(set(TIE_COPIES) & {r for r, _ in exp["ties"]}) >= 2


@pytest.mark.parametrize("storage", ["bf16", "q16"])
def test_sharded_index_equals_one_index(storage):
    got, exp = _run(2, storage), _single(storage)
    for r in range(2):
        for lst, want in zip(got[r]["sharded"], exp["sharded"]):
            _same(lst, want, storage)


def _mismatch_entry(rank, world, port, q):
    import torch.distributed as dist

    from pilottai_amd.memory.node_store import NodeSemanticStore

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        vecs, prio, tags, queries = _data()
        grp = dist.new_group(backend="gloo")
        store = NodeSemanticStore(_shard(vecs[:64], prio[:64], tags[:64], rank, world, "bf16"), group=grp,
                                  cross_shard_mmr=(rank == 0))
        store.start()
        try:
            store.search_rows_blocking(queries[:1], 3, [0], [()], timeout=120)
            res = "answered"
        except RuntimeError as e:
            res = f"RuntimeError: {e}"
        store.stop(timeout=30)
        q.put((rank, res))
    except BaseException:
        q.put((rank, {"error": traceback.format_exc()}))
        raise
    finally:
        dist.destroy_process_group()


def test_flag_mismatch_fails_every_waiter():
    got = _spawn_ranks(_mismatch_entry, 2, ())
    for r in range(2):
        assert got[r].startswith("RuntimeError") and "cross_shard_mmr differs" in got[r], got[r]


def test_the_flag_is_opt_in(monkeypatch):
    from pilottai_amd.memory.node_store import NodeSemanticStore

    monkeypatch.delenv("PILOTTAI_NODE_MMR", raising=False)
    vecs, prio, tags, queries = _data()
    idx = SemanticIndex(dim=DIM, capacity=2048, device="cpu")
    idx.add(vecs, prio, tags, [None] * N)
    store = NodeSemanticStore(idx)  # default: the refusal stays, before any queueing
    assert store.cross_shard_mmr is False
    with pytest.raises(ValueError, match="other ranks"):
        asyncio.run(store.search_batch(["anything"], diversity=0.5))
    with pytest.raises(ValueError, match="other ranks"):
        store.search_rows_blocking(queries[:1], 3, [0], [()], diversity=0.5)
    with pytest.raises(ValueError, match="other ranks"):
        ShardedSemanticIndex(idx).search(queries[:1], 3, [0], [()], diversity=0.3)
    assert NodeSemanticStore(idx, cross_shard_mmr=True).cross_shard_mmr is True
    monkeypatch.setenv("PILOTTAI_NODE_MMR", "1")
    assert NodeSemanticStore(idx).cross_shard_mmr is True
    # validation is the single index's
    flagged = NodeSemanticStore(idx, cross_shard_mmr=True)
    for bad in ({"diversity": 1.5}, {"diversity": [0.5, 0.5]}, {"fetch_k": 2}, {"fetch_k": 65}):
        with pytest.raises(ValueError):
            flagged.search_rows_blocking(queries[:1], 3, [0], [()], **bad)
    # world 1 goes through the same steps and equals the index
    sh = ShardedSemanticIndex(idx, cross_shard_mmr=True)
    assert [[r for r, _ in lst] for lst in sh.search(queries, 3, MINP, TAGS, diversity=DIV)] == \
        [[r for r, _ in lst] for lst in idx.search(queries, 3, MINP, TAGS, diversity=DIV)]


DUP = "the deploy failed because the disk of the build host was full"
DISTINCT = ["the deploy succeeded after the disk of the build host was cleaned", "kernel tuning notes for the decode gemm",
            "quarterly revenue of unit seven grew", "the deploy failed because a certificate expired",
            "lunch menu of the canteen on tuesday"]
ASK = "what went wrong with the deploy"


def test_batcher_and_agent_over_a_flagged_node_store():
    """MemoryLookupBatcher.search(diversity=) and BaseAgent(memory_diversity=) over a world-1 node
    store with the flag on: one member per cluster where the plain search returns three copies."""
    from pilottai_amd.core.agent import BaseAgent
    from pilottai_amd.core.task import Task
    from pilottai_amd.memory.batcher import MemoryLookupBatcher
    from pilottai_amd.memory.embedding import HashingEmbedder
    from pilottai_amd.memory.node_store import NodeSemanticStore

    store = NodeSemanticStore(SemanticIndex(dim=256, capacity=64, device="cpu"), embedder=HashingEmbedder(256),
                              cross_shard_mmr=True)
    store.start()

    async def go():
        await store.store_semantic_batch([DUP] * 10 + DISTINCT)
        b = MemoryLookupBatcher(store)
        plain, div = await asyncio.gather(b.search(ASK, limit=3), b.search(ASK, limit=3, diversity=0.5))
        agent = BaseAgent(role="worker", goal="g", memory_lookup=b, memory_diversity=0.5)
        ctx = await agent._memory_context(Task(description=ASK), "")
        direct = await store.semantic_search(ASK, limit=3, diversity=0.5)
        return plain, div, ctx, direct

    try:
        plain, div, ctx, direct = asyncio.run(go())
    finally:
        store.stop()
    assert [m.text for m in plain] == [DUP] * 3
    assert len({m.text for m in div}) == 3 and DUP in {m.text for m in div}
    assert len({m.text for m in direct}) == 3
    assert len(set(ctx.split("; "))) == 3
    assert store.stats["mmr_lookups"] >= 3 and store.stats["mmr_rows"] > 0
