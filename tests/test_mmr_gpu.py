"""The MMR re-ranking kernel (csrc/ops/similarity_mmr.hip) on the GPU.

q16 storage: the pairwise scores are exact integer dot products, so rows and scores must equal
ops/reference.py bit for bit. bf16 storage: the MFMA's fp32 accumulation order is not the
reference's, so the test follows the kernel's own pick sequence (teacher forcing) and requires
every pick to be a best candidate within the accumulation error bound; see
test_bf16_teacher_forced. Output buffers are poisoned before every launch."""
import asyncio

import pytest
import torch

from pilottai_amd import ops
from pilottai_amd.memory.enhanced_memory import EnhancedMemory
from pilottai_amd.memory.semantic_index import SemanticIndex
from pilottai_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

N = 203  # the last 16-row tile is partial
DIVERSITY = (0.0, 0.25, 0.5, 1.0)
QMAX = 70
POISON_ROW = 0x7F7F7F7F


def _poisoned(Q, k, dev):
    return (torch.full((Q, k), float("nan"), device=dev), torch.full((Q, k), POISON_ROW, dtype=torch.int32, device=dev))


def _vectors(D, seed):
    """N unit rows; rows 5, 37 and 200 are exact copies of row 0, row 101 of row 100."""
    g = torch.Generator().manual_seed(seed)
    v = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=1)
    v[5] = v[37] = v[200] = v[0]
    v[101] = v[100]
    return v


def _index(storage, D, dev, seed=0):
    idx = SemanticIndex(dim=D, capacity=N, device=dev, growable=False, storage=storage)
    idx.add(_vectors(D, seed).numpy(), [0] * N, [()] * N, [None] * N)
    torch.cuda.synchronize()
    return idx


def _lists(m, seed):
    """QMAX candidate lists of m entries: lengths 0..m (query 0 full, query 1 empty). Even
    queries take neighbours -- one tile while it lasts (tile 0 with the copies 0 and 5), then the
    partial last tile and tiles 1..3; odd queries spread over all tiles, the duplicate rows first.
    Scores descend, with ties."""
    g = torch.Generator().manual_seed(seed)
    rows = torch.full((QMAX, m), -1, dtype=torch.int32)
    scores = torch.full((QMAX, m), float("-inf"))
    near = torch.cat([torch.arange(0, 16), torch.arange(192, N), torch.arange(16, 64)])
    dups = [0, 5, 100, 101, 200, 37]
    for q in range(QMAX):
        n = m if q == 0 else (0 if q == 1 else int(torch.randint(0, m + 1, (1,), generator=g)))
        if q % 2 == 0:
            pool = near[:max(16, n)]
        else:
            pool = torch.tensor(dups + [x for x in torch.randperm(N, generator=g).tolist() if x not in dups])[:max(6, n)]
        pick = pool[torch.randperm(len(pool), generator=g)][:n]
        rows[q, :n] = pick.int()
        scores[q, :n] = torch.sort(torch.round(torch.rand(n, generator=g) * 16) / 16 - 0.25, descending=True).values
    return rows, scores


_q16_cache = {}


def _q16_case(D, m, dev):
    """(index, rows, scores, wr, wd, reference rows, reference scores for k = m), computed once."""
    key = (D, m)
    if key not in _q16_cache:
        idx = _q16_cache.get(D) or _index("q16", D, dev)
        _q16_cache[D] = idx
        rows, scores = _lists(m, seed=m)
        wr, wd = ops.mmr_weights([DIVERSITY[q % 4] for q in range(QMAX)])
        if ("gram", D) not in _q16_cache:  # s_ij of all N rows, once per index
            _q16_cache["gram", D] = ref.q16_pairwise(idx.hi.cpu(), idx.lo.cpu(), idx.rmeta.cpu(), torch.arange(N))
        gram = _q16_cache["gram", D]
        er = torch.empty(QMAX, m, dtype=torch.int32)
        es = torch.empty(QMAX, m)
        for q in range(QMAX):
            c = rows[q].long().clamp(min=0)  # entries past the list end are never read
            es[q], er[q] = ref.mmr_select(scores[q], rows[q], gram[c][:, c], m, wr[q], wd[q])
        _q16_cache[key] = (idx, rows, scores, wr, wd, er, es)
    return _q16_cache[key]


def _prefix(full_r, full_s, k):
    """The k-selection from the m-selection (greedy selection is prefix-consistent:
    tests/test_mmr.py), padded past m."""
    Q, m = full_r.shape
    r = torch.full((Q, k), -1, dtype=torch.int32)
    s = torch.full((Q, k), float("-inf"))
    r[:, :min(k, m)] = full_r[:, :k]
    s[:, :min(k, m)] = full_s[:, :k]
    return r, s


@pytest.mark.parametrize("m", [1, 2, 17, 64])
@pytest.mark.parametrize("D", [64, 192, 1024])
def test_q16_bit_identical(gpu, D, m):
    idx, rows, scores, wr, wd, full_r, full_s = _q16_case(D, m, gpu)
    for Q in (1, 3, QMAX):
        for k in sorted({1, 5, m}):
            er, es = _prefix(full_r[:Q], full_s[:Q], k)
            out = _poisoned(Q, k, gpu)
            s, r = ops.mmr_select(rows[:Q].to(gpu), scores[:Q].to(gpu), idx._mmr_planes(), k, wr[:Q], wd[:Q], out=out)
            assert torch.equal(r.cpu(), er), (D, m, Q, k)
            assert torch.equal(s.cpu().view(torch.int32), es.view(torch.int32)), (D, m, Q, k)  # bit for bit
            # d = 0 (queries 0, 4, 8, ...): the first k candidates, unchanged
            n0 = (rows[:Q:4] >= 0).sum(1).clamp(max=k)
            for i, n in enumerate(n0.tolist()):
                assert torch.equal(r[4 * i, :n].cpu(), rows[4 * i, :n]) and torch.equal(s[4 * i, :n].cpu(), scores[4 * i, :n])


@pytest.mark.parametrize("D", [96, 1024])
def test_bf16_teacher_forced(gpu, D):
    """Every pick of the kernel must be, in the fp64 reference, within 2 eps of the best open
    candidate, eps = 2 (D + 8) 2^-24: the worst-case error of a D-term fp32 accumulation of
    unit-norm rows (|sum - exact| <= D u sum|a_i b_i| <= D u, u = 2^-24, doubled for the unknown
    summation tree, + 8 u for the three fp32 operations of the MMR value and the unit-norm slack
    of bf16 rows). It bounds the error of rel (the scan's sum) and of s_ij (this kernel's) alike,
    and wr + wd = 1, so each candidate's MMR value is off by at most eps; the pick and the
    reference's best are two candidates, hence 2 eps. No step is exempt."""
    idx = _index("bf16", D, gpu, seed=1)
    g = torch.Generator().manual_seed(D)
    Q, m = QMAX, 64
    queries = torch.nn.functional.normalize(
        _vectors(D, 1)[torch.randint(0, N, (Q,), generator=g)] + 0.7 * torch.randn(Q, D, generator=g) / D ** 0.5, dim=1)
    stored = idx.read_rows(0, N).double().cpu()
    qb = queries.to(torch.bfloat16).double()
    # rel as a scan gives it: a D-term fp32 sum of the bf16 products, the top m best first
    scores, rows = torch.topk(qb.float() @ stored.float().T, m, dim=1)
    rows = rows.int()
    lens = torch.randint(0, m + 1, (Q,), generator=g)
    lens[0], lens[1] = m, 0
    for q in range(Q):
        rows[q, lens[q]:] = -1
        scores[q, lens[q]:] = float("-inf")
    d = [DIVERSITY[q % 4] for q in range(Q)]
    wr, wd = ops.mmr_weights(d)
    gram = ref.bf16_pairwise(idx.packed.cpu(), torch.arange(N))  # fp64 s_ij of all N rows
    eps = 2 * (D + 8) * 2.0 ** -24
    for k in (1, 5, m):
        out = _poisoned(Q, k, gpu)
        s, r = ops.mmr_select(rows.to(gpu), scores.to(gpu), idx._mmr_planes(), k, wr, wd, out=out)
        s, r = s.cpu(), r.cpu()
        for q in range(Q):
            n = int(lens[q])
            cand = rows[q, :n].long()
            picks = min(k, n)
            assert (r[q, picks:] == -1).all() and (s[q, picks:] == float("-inf")).all()
            if d[q] == 0.0:  # the first k candidates, bit for bit
                assert torch.equal(r[q, :picks], rows[q, :picks]) and torch.equal(s[q, :picks], scores[q, :picks])
            rel = stored[cand] @ qb[q]
            sims = gram[cand][:, cand]
            pos = {int(x): i for i, x in enumerate(cand)}
            open_ = torch.ones(n, dtype=torch.bool)
            M = torch.zeros(n, dtype=torch.float64)
            for step in range(picks):
                p = pos[int(r[q, step])]  # a listed candidate ...
                assert open_[p]           # ... not picked before
                assert s[q, step] == scores[q, p]  # reported with its cosine score
                val = float(wr[q]) * rel - (float(wd[q]) * M if step else 0.0)
                best = val[open_].max()
                assert val[p] >= best - 2 * eps, (D, k, q, step, float(best - val[p]), eps)
                open_[p] = False
                M = sims[:, p].clone() if step == 0 else torch.maximum(M, sims[:, p])


def _clusters(D, seed=0, per=16, noise=1e-3):
    """4 cluster centres x 16 near-duplicates; the query pulled towards the centres with weights
    1 / 0.9 / 0.8 / 0.7."""
    g = torch.Generator().manual_seed(seed)
    centres = torch.nn.functional.normalize(torch.randn(4, D, generator=g), dim=1)
    rows = torch.cat([centres[c] + noise * torch.randn(per, D, generator=g) for c in range(4)])
    perm = torch.randperm(4 * per, generator=g)
    query = (torch.tensor([1.0, 0.9, 0.8, 0.7])[:, None] * centres).sum(0, keepdim=True)
    return rows[perm], perm // per, query


@pytest.mark.parametrize("storage", ["bf16", "q16"])
@pytest.mark.parametrize("D", [256, 1024])
def test_clusters_and_index_matches_cpu(gpu, D, storage):
    vec, cluster_of, query = _clusters(D)
    res = {}
    for dev in (gpu, "cpu"):
        idx = SemanticIndex(dim=D, capacity=64, device=dev, growable=False, storage=storage)
        idx.add(vec.numpy(), [0] * 64, [()] * 64, [None] * 64)
        res[str(dev)] = [idx.search(query, 8, [0], [()], diversity=d, fetch_k=64)[0] for d in (0.0, 0.5, 0.75, 1.0)]
        batch = idx.search(query.repeat(4, 1), 8, [0] * 4, [()] * 4, diversity=[0.0, 0.5, 0.75, 1.0], fetch_k=64)
        assert [[r for r, _ in h] for h in batch] == [[r for r, _ in h] for h in res[str(dev)]]
    on_gpu, on_cpu = res[str(gpu)], res["cpu"]
    clusters = lambda hits: [int(cluster_of[r]) for r, _ in hits]  # noqa: E731
    assert clusters(on_gpu[0]) == [0] * 8  # d = 0: eight near-duplicates
    for hits in on_gpu[1:]:  # d >= 0.5: the first four picks from four clusters
        assert len(hits) == 8 and len({r for r, _ in hits}) == 8
        assert sorted(clusters(hits)[:4]) == [0, 1, 2, 3]
    if storage == "q16":  # exact scores: identical to the CPU index
        assert on_gpu == on_cpu
    else:  # within-cluster margins are ~1e-5: cluster-level agreement
        assert [clusters(h)[:4] for h in on_gpu] == [clusters(h)[:4] for h in on_cpu]


@pytest.mark.parametrize("storage", ["bf16", "q16"])
def test_enhanced_memory_duplicates_on_the_gpu_index(gpu, storage):
    dup = "the deploy failed because the disk of the build host was full"
    distinct = ["the deploy succeeded after the disk of the build host was cleaned",
                "kernel tuning notes for the decode gemm", "quarterly revenue of unit seven grew",
                "the deploy failed because a certificate expired", "lunch menu of the canteen on tuesday"]
    ask = "what went wrong with the deploy"

    async def go():
        mem = EnhancedMemory(dim=256, device=gpu, storage=storage)
        for _ in range(10):
            await mem.store_semantic(dup)
        for t in distinct:
            await mem.store_semantic(t)
        return await mem.semantic_search(ask, limit=3, diversity=0.5), await mem.semantic_search(ask, limit=3)

    div, plain = asyncio.run(go())
    assert [m.text for m in plain] == [dup] * 3
    assert len({m.text for m in div}) == 3 and dup in {m.text for m in div}
