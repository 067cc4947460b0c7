"""Diversity-aware memory search (maximal marginal relevance) on the CPU tier: the reference
semantics (ops/reference.py mmr_select), ops.mmr_select on CPU tensors, SemanticIndex in both
storages, and the keyword's way up through EnhancedMemory, the batcher and BaseAgent.
The GPU kernel (csrc/ops/similarity_mmr.hip) is tested in tests/test_mmr_gpu.py."""
import asyncio
import math

import numpy as np
import pytest
import torch

from pilottai_amd import ops
from pilottai_amd.core.agent import BaseAgent
from pilottai_amd.core.task import Task
from pilottai_amd.memory.batcher import MemoryLookupBatcher
from pilottai_amd.memory.enhanced_memory import EnhancedMemory
from pilottai_amd.memory.semantic_index import SemanticIndex, ShardedSemanticIndex
from pilottai_amd.ops import reference as ref

# ---- the hand-worked example: six candidates, every value a dyadic fraction (exact in fp32).
# Candidate 1 duplicates 0 and candidate 4 duplicates 3.
REL = [1.0, 0.75, 0.75, 0.5, 0.5, 0.25]
ROWS = [10, 11, 12, 13, 14, 15]
SIM = torch.tensor([[1.00, 1.00, 0.50, 0.00, 0.00, 0.00],
                    [1.00, 1.00, 0.50, 0.00, 0.00, 0.00],
                    [0.50, 0.50, 1.00, 0.25, 0.25, 0.00],
                    [0.00, 0.00, 0.25, 1.00, 1.00, 0.00],
                    [0.00, 0.00, 0.25, 1.00, 1.00, 0.00],
                    [0.00, 0.00, 0.00, 0.00, 0.00, 1.00]])


def _picks(k, d, rel=REL, rows=ROWS, sim=SIM):
    s, r = ref.mmr_select(torch.tensor(rel), torch.tensor(rows, dtype=torch.int32), sim, k,
                          np.float32(1 - d), np.float32(d))
    assert s.dtype == torch.float32 and r.dtype == torch.int32 and s.shape == (k,) and r.shape == (k,)
    return r.tolist(), s.tolist()


def test_reference_hand_worked_example():
    # d = 0: the list unchanged
    assert _picks(3, 0.0) == ([10, 11, 12], [1.0, 0.75, 0.75])
    # d = 0.5, by hand (wr = wd = 0.5):
    #  step 0: t = .5 .375 .375 .25 .25 .125                       -> 0
    #  step 1: M = 1 .5 0 0 0 -> -.125 .125 .25 .25 .125: 3 and 4 tie -> 3 (the smaller position)
    #  step 2: M = 1 .5 . 1 0 -> -.125 .125 . -.25 .125:  2 and 5 tie -> 2
    #  step 3: M = 1 . . 1 0  -> -.125 . . -.25 .125                -> 5, then 1 (-.125), then 4 (-.25)
    # k = 8 > m = 6: two empty entries; every pick is reported with its cosine, not its MMR value
    r, s = _picks(8, 0.5)
    assert r == [10, 13, 12, 15, 11, 14, -1, -1]
    assert s[:6] == [1.0, 0.5, 0.75, 0.25, 0.75, 0.5] and s[6:] == [-math.inf, -math.inf]
    # d = 1 (wr = 0): step 0 is an all-zero tie -> 0; then 0 - M: 3, 4, 5 tie at 0 -> 3; then 5
    # (the only one at 0); then 2 (-.5); then 1 and 4 tie at -1 -> 1; then 4
    assert _picks(6, 1.0)[0] == [10, 13, 15, 12, 11, 14]
    # prefix consistency: the first L picks of a k-selection are the L-selection
    for d in (0.0, 0.25, 0.5, 1.0):
        full = _picks(6, d)[0]
        for L in range(1, 6):
            assert _picks(L, d)[0] == full[:L]


def test_reference_zero_signs_tie_and_list_end():
    # wr = 0 makes t = (-0, +0): equal, so the smaller position wins
    assert _picks(2, 1.0, rel=[-0.5, 0.5], rows=[7, 3], sim=torch.eye(2))[0] == [7, 3]
    # the list ends at the first -1; an empty list gives an empty result
    assert _picks(3, 0.5, rows=[10, 11, -1, 13, 14, 15])[0] == [10, 11, -1]
    assert _picks(2, 0.5, rows=[-1] * 6) == ([-1, -1], [-math.inf, -math.inf])


# ---- index data: 4 cluster centres x 16 near-duplicates, the query pulled towards the centres
# with weights 1 / 0.9 / 0.8 / 0.7
def _clusters(D, seed=0, per=16, noise=1e-3):
    g = torch.Generator().manual_seed(seed)
    centres = torch.nn.functional.normalize(torch.randn(4, D, generator=g), dim=1)
    rows = torch.cat([centres[c] + noise * torch.randn(per, D, generator=g) for c in range(4)])
    perm = torch.randperm(4 * per, generator=g)  # clusters spread over the tiles
    query = (torch.tensor([1.0, 0.9, 0.8, 0.7])[:, None] * centres).sum(0, keepdim=True)
    return rows[perm], (perm // per), query


def _cluster_index(storage, D=256, device="cpu"):
    rows, cluster_of, query = _clusters(D)
    idx = SemanticIndex(dim=D, capacity=64, device=device, growable=False, storage=storage)
    idx.add(rows.numpy(), [0] * 64, [()] * 64, [None] * 64)
    return idx, cluster_of, query


def _random_lists(idx, Q, m, seed):
    """Candidate lists of mixed lengths over a filled index: distinct rows, scores descending."""
    g = torch.Generator().manual_seed(seed)
    rows = torch.full((Q, m), -1, dtype=torch.int32)
    scores = torch.full((Q, m), float("-inf"))
    for q in range(Q):
        n = int(torch.randint(0, m + 1, (1,), generator=g)) if q else m
        rows[q, :n] = torch.randperm(idx.count, generator=g)[:n].int()
        scores[q, :n] = torch.sort(torch.rand(n, generator=g), descending=True).values
    return rows, scores


@pytest.mark.parametrize("storage", ["bf16", "q16"])
def test_ops_mmr_select_on_cpu_is_the_reference(storage):
    idx, _, _ = _cluster_index(storage, D=128)
    rows, scores = _random_lists(idx, Q=5, m=17, seed=1)
    d = [0.0, 0.25, 0.5, 1.0, 0.5]
    wr, wd = ops.mmr_weights(d)
    assert wr.dtype == torch.float32 and wr.tolist() == [1.0, 0.75, 0.5, 0.0, 0.5] and wd.tolist() == d
    s, r = ops.mmr_select(rows, scores, idx._mmr_planes(), 6, wr, wd)
    dense = idx.read_rows(0, 64).double()
    for q in range(5):
        if storage == "q16":
            sims = ref.q16_pairwise(idx.hi, idx.lo, idx.rmeta, rows[q])
        else:
            sims = ref.bf16_pairwise(idx.packed, rows[q])
        n = int((rows[q] >= 0).sum())
        # the pairwise matrix is the Gram matrix of the stored rows
        want = dense[rows[q, :n].long()] @ dense[rows[q, :n].long()].T
        assert torch.allclose(sims[:n, :n].double(), want, atol=1e-6, rtol=0)
        es, er = ref.mmr_select(scores[q], rows[q], sims, 6, wr[q], wd[q])
        assert torch.equal(r[q], er) and torch.equal(s[q], es)
        if d[q] == 0.0:
            assert torch.equal(r[q, :min(n, 6)], rows[q, :min(n, 6)])


@pytest.mark.parametrize("storage", ["bf16", "q16"])
def test_index_search_with_diversity(storage):
    idx, cluster_of, query = _cluster_index(storage)
    plain = idx.search(query, 8, [0], [()])
    assert {int(cluster_of[r]) for r, _ in plain[0]} == {0}  # 8 near-duplicates
    assert idx.search(query, 8, [0], [()], diversity=0.0, fetch_k=64) == plain
    for d in (0.5, 0.75):
        hits = idx.search(query, 8, [0], [()], diversity=d, fetch_k=64)
        assert len(hits[0]) == 8 and len({r for r, _ in hits[0]}) == 8
        assert sorted(int(cluster_of[r]) for r, _ in hits[0][:4]) == [0, 1, 2, 3]
        assert hits[0][0] == plain[0][0]  # the first pick is the best hit
        score_of = dict(idx.search(query, 64, [0], [()])[0])
        assert all(sc == score_of[r] for r, sc in hits[0])  # cosine scores, not MMR values
    # a mixed batch: the query with d = 0 comes out as its plain top-k
    two = torch.cat([query, query])
    mixed = idx.search(two, 8, [0, 0], [(), ()], diversity=[0.0, 0.5], fetch_k=64)
    alone = idx.search(two, 8, [0, 0], [(), ()], fetch_k=64)[0], idx.search(two, 8, [0, 0], [(), ()], diversity=0.5,
                                                                            fetch_k=64)[1]
    assert mixed[0] == alone[0] and mixed[1] == alone[1]
    assert [r for r, _ in mixed[0]] == [r for r, _ in plain[0]]
    # the default fetch_k is min(64, 4 k)
    assert idx.search(query, 4, [0], [()], diversity=0.5) == idx.search(query, 4, [0], [()], diversity=0.5, fetch_k=16)
    # search_tensors returns the same picks as tensors
    s, r = idx.search_tensors(query, 8, [0], [0], diversity=0.75, fetch_k=64)
    assert r.shape == (1, 8) and [(int(a), float(b)) for a, b in zip(r[0], s[0])] == hits[0]


def test_overflow_tags_are_rechecked_before_the_reranking():
    D = 128
    rows, cluster_of, query = _clusters(D, seed=3)
    idx = SemanticIndex(dim=D, capacity=256, device="cpu", growable=False)
    g = torch.Generator().manual_seed(9)
    idx.add(torch.randn(63, D, generator=g).numpy(), [0] * 63, [(f"t{i}",) for i in range(63)], [None] * 63)
    # "zz" and "yy" both land on the shared overflow bit; the "yy" rows are copies of the best hit
    idx.add(rows[:32].numpy(), [0] * 32, [("zz",)] * 32, [None] * 32)
    idx.add(query.repeat(8, 1).numpy(), [0] * 8, [("yy",)] * 8, [None] * 8)
    assert not idx.query_masks([("zz",)])[1][0]
    hits = idx.search(query, 3, [0], [("zz",)], diversity=0.5, fetch_k=64)[0]
    assert len(hits) == 3 and all(63 <= r < 95 for r, _ in hits)
    assert len({int(cluster_of[r - 63]) for r, _ in hits}) == 3
    assert hits[0] == idx.search(query, 3, [0], [("zz",)])[0][0]


def test_zero_diversity_never_reaches_mmr_select(monkeypatch):
    idx, _, query = _cluster_index("bf16")
    before = idx.search(query, 5, [0], [()])

    def boom(*a, **kw):
        raise AssertionError("mmr_select called for diversity 0")

    monkeypatch.setattr(ops, "mmr_select", boom)
    assert idx.search(query, 5, [0], [()], diversity=0.0) == before
    assert idx.search(query, 5, [0], [()], diversity=[0], fetch_k=20) == before
    s, r = idx.search_tensors(query, 5, [0], [0], diversity=0.0)
    es, er = idx.search_tensors(query, 5, [0], [0])
    assert torch.equal(s, es) and torch.equal(r, er)
    mem = EnhancedMemory(dim=64, device="cpu")

    async def go():
        await mem.store_semantic_batch(["a note", "another note"])
        return await mem.semantic_search("note", limit=2, diversity=0.0)

    assert len(asyncio.run(go())) == 2
    with pytest.raises(AssertionError):
        idx.search(query, 5, [0], [()], diversity=0.5)


DUP = "the deploy failed because the disk of the build host was full"
DISTINCT = ["the deploy succeeded after the disk of the build host was cleaned", "kernel tuning notes for the decode gemm",
            "quarterly revenue of unit seven grew", "the deploy failed because a certificate expired",
            "lunch menu of the canteen on tuesday"]


# the query is a paraphrase: with the stored text itself, rel_j == s_j0 for every candidate j and
# all MMR values after the first pick are rounding noise around 0
ASK = "what went wrong with the deploy"


async def _dup_memory(device="cpu", storage="bf16"):
    mem = EnhancedMemory(dim=256, device=device, storage=storage)
    for _ in range(10):
        await mem.store_semantic(DUP)
    for t in DISTINCT:
        await mem.store_semantic(t)
    return mem


@pytest.mark.parametrize("storage", ["bf16", "q16"])
def test_enhanced_memory_duplicates(storage):
    async def go():
        mem = await _dup_memory(storage=storage)
        return (await mem.semantic_search(ASK, limit=3, diversity=0.5), await mem.semantic_search(ASK, limit=3),
                await mem.search_batch([ASK, ASK], limit=3, diversity=[0.0, 0.5]))

    div, plain, both = asyncio.run(go())
    assert [m.text for m in plain] == [DUP] * 3
    assert len({m.text for m in div}) == 3 and DUP in {m.text for m in div}
    assert [m.text for m in both[0]] == [DUP] * 3 and len({m.text for m in both[1]}) == 3


def test_batcher_carries_per_lookup_diversity_in_one_pass():
    async def go():
        mem = await _dup_memory()
        seen = []
        inner = mem.search_batch

        async def spy(queries, **kw):
            seen.append(kw.get("diversity", "absent"))
            return await inner(queries, **kw)

        mem.search_batch = spy
        b = MemoryLookupBatcher(mem)
        res = await asyncio.gather(b.search(ASK, limit=3), b.search(ASK, limit=3, diversity=0.5),
                                   b.search(ASK, limit=3, diversity=0.25))
        plain = await b.search(ASK, limit=3)
        return res, plain, seen, b.stats["passes"]

    res, plain, seen, passes = asyncio.run(go())
    assert seen == [[0.0, 0.5, 0.25], "absent"] and passes == 2  # a plain batch calls the store as before
    assert [m.text for m in res[0]] == [DUP] * 3 and [m.text for m in plain] == [DUP] * 3
    assert len({m.text for m in res[1]}) == 3 and len({m.text for m in res[2]}) >= 2


def test_agent_memory_diversity_reaches_the_store():
    class Lookup:
        def __init__(self):
            self.calls = []

        async def search(self, query, **kw):
            self.calls.append(kw)
            return []

    async def go(d):
        lk = Lookup()
        agent = BaseAgent(role="worker", goal="extract findings", memory_lookup=lk, memory_top_k=2, **d)
        await agent._memory_context(Task(description="Summarize the report"), "{}")
        return lk.calls

    assert asyncio.run(go({"memory_diversity": 0.5})) == [{"limit": 2, "diversity": 0.5}]
    assert asyncio.run(go({})) == [{"limit": 2}]
    for bad in (-0.1, 1.5, float("nan"), "0.5", None):
        with pytest.raises(ValueError):
            BaseAgent(role="worker", goal="g", memory_diversity=bad)

    async def end_to_end():
        mem = await _dup_memory()
        agent = BaseAgent(role="worker", goal="g", memory_lookup=MemoryLookupBatcher(mem), memory_diversity=0.5)
        return await agent._memory_context(Task(description=ASK), "")

    assert len(set(asyncio.run(end_to_end()).split("; "))) == 3


def test_both_stores_take_the_keywords_and_the_sharded_ones_refuse():
    from pilottai_amd.memory.node_store import NodeSemanticStore
    from pilottai_amd.memory.store_protocol import SemanticStore, signature_mismatches
    import inspect

    for name in ("search_batch", "semantic_search"):
        params = inspect.signature(getattr(SemanticStore, name)).parameters
        assert "diversity" in params and "fetch_k" in params
    assert signature_mismatches(EnhancedMemory) == []
    assert signature_mismatches(NodeSemanticStore) == []

    idx, _, query = _cluster_index("bf16")
    store = NodeSemanticStore(idx)  # world 1, round thread not started: refused before any queueing

    async def node(**kw):
        return await store.search_batch(["anything"], **kw)

    for call in (lambda: asyncio.run(node(diversity=0.5)), lambda: asyncio.run(node(diversity=[0.2])),
                 lambda: asyncio.run(store.semantic_search("anything", diversity=1.0))):
        with pytest.raises(ValueError, match="other ranks"):
            call()
    sh = ShardedSemanticIndex(idx)
    assert sh.search(query, 3, [0], [()], diversity=0.0) == idx.search(query, 3, [0], [()])
    with pytest.raises(ValueError, match="other ranks"):
        sh.search(query, 3, [0], [()], diversity=0.3)


def test_validation_errors():
    idx, _, query = _cluster_index("bf16")
    for bad in (-0.01, 1.01, float("nan"), float("inf"), "0.5", None, [0.5, 0.5], [2.0], True):
        with pytest.raises(ValueError):
            idx.search(query, 3, [0], [()], diversity=bad)
        with pytest.raises(ValueError):
            idx.search_tensors(query, 3, [0], [0], diversity=bad)
    for bad in (2, 65, 0, -1, 2.5):  # outside [limit, 64]
        with pytest.raises(ValueError):
            idx.search(query, 3, [0], [()], diversity=0.5, fetch_k=bad)
        with pytest.raises(ValueError):
            idx.search_tensors(query, 3, [0], [0], fetch_k=bad)
    assert len(idx.search(query, 3, [0], [()], diversity=0.5, fetch_k=3)[0]) == 3
    assert len(idx.search(query, 3, [0], [()], diversity=0.5, fetch_k=64)[0]) == 3

    async def go():
        mem = await _dup_memory()
        for kw in ({"diversity": 1.5}, {"diversity": float("nan")}, {"fetch_k": 2, "diversity": 0.5}, {"fetch_k": 65},
                   {"mode": "substring", "diversity": 0.5}):
            with pytest.raises(ValueError):
                await mem.semantic_search(ASK, limit=3, **kw)
        assert len(await mem.semantic_search("deploy", limit=3, mode="substring", diversity=0.0)) == 3
        with pytest.raises(ValueError):
            await MemoryLookupBatcher(mem).search(DUP, diversity=-1)

    asyncio.run(go())
    rows = torch.zeros(1, 65, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.mmr_select(rows, rows.float(), idx._mmr_planes(), 3, [1.0], [0.0])
