"""Cross-shard MMR on the GPU (csrc/ops/similarity_mmr_rows.hip): the owner-side record gather,
the requester-side selection over records, and the node store's round over GPU indexes.

gather_rows must reproduce ops.reference._tile_rows bit for bit. mmr_select_rows: q16 equals
ops.reference.mmr_select bit for bit; bf16 is bit-identical to the tile kernel (the same
instruction on the same fragments in the same slab order) and passes the accumulation-bound check
of tests/test_mmr_gpu.py::test_bf16_teacher_forced, re-implemented here. The kernels under test
never produce an expectation: records come from the reference gather. Output buffers are
poisoned before every launch."""
import os
import queue
import socket
import time
import traceback

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from pilottai_amd import ops
from pilottai_amd.memory.semantic_index import SemanticIndex
from pilottai_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

N = 203  # the last 16-row tile is partial
DIVERSITY = (0.0, 0.25, 0.5, 1.0)
QMAX = 70
POISON = 0x7F7F7F7F
BIG = 2 ** 31 - 1


def _vectors(D, seed):
    """N unit rows; rows 5, 37 and 200 are exact copies of row 0, row 101 of row 100."""
    g = torch.Generator().manual_seed(seed)
    v = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=1)
    v[5] = v[37] = v[200] = v[0]
    v[101] = v[100]
    return v


_idx_cache = {}


def _index(storage, D, dev):
    if (storage, D) not in _idx_cache:
        idx = SemanticIndex(dim=D, capacity=N, device=dev, growable=False, storage=storage)
        idx.add(_vectors(D, 1).numpy(), [0] * N, [()] * N, [None] * N)
        torch.cuda.synchronize()
        _idx_cache[storage, D] = idx
    return _idx_cache[storage, D]


def _cpu_planes(idx):
    return tuple(p.cpu() for p in idx._mmr_planes())


# ---------------------------------------------------------------------------- gather_rows
def _expected_records(idx, rows):
    """Row-major records through _tile_rows; ids outside [0, N): zero records."""
    planes = _cpu_planes(idx)
    rows = torch.as_tensor(rows).long()
    ok = (rows >= 0) & (rows < N)
    safe = torch.where(ok, rows, torch.zeros_like(rows))
    if idx.storage == "q16":
        hi, lo, rmeta = planes
        sc = rmeta[safe, 0].contiguous().view(torch.uint8).view(-1, 4)
        rec = torch.cat([ref._tile_rows(hi, safe, 4).contiguous().view(torch.uint8),
                         ref._tile_rows(lo, safe, 4).contiguous().view(torch.uint8), sc,
                         torch.zeros(len(rows), 12, dtype=torch.uint8)], 1)
    else:
        rec = ref._tile_rows(planes[0], safe, 4).contiguous().view(torch.uint8)
    rec[~ok] = 0
    return rec


def _row_lists(n):
    """Lists of n ids: row 0, row N - 1, repeats of one row, and -1 / N / 2^31 - 1 (zero records)."""
    special = [0, N - 1, 7, 7, -1, N, BIG, 7, -(2 ** 31), N + 5]
    if n == 1:
        return [[s] for s in special]
    g = torch.Generator().manual_seed(n)
    body = torch.randint(0, N, (n,), generator=g).tolist()
    at = torch.randperm(n, generator=g)[:len(special)].tolist()
    for p, s in zip(at, special):
        body[p] = s
    return [body]


@pytest.mark.parametrize("storage,D", [("bf16", 32), ("bf16", 96), ("bf16", 1024), ("q16", 64), ("q16", 192),
                                       ("q16", 1024)])
def test_gather_rows_is_tile_rows(gpu, storage, D):
    idx = _index(storage, D, gpu)
    rb = ops.record_bytes(D, storage == "q16")
    for n in (1, 63, 64, 65, 1000):
        for rows in _row_lists(n):
            want = _expected_records(idx, rows)
            assert want.shape == (n, rb)
            buf = torch.full((n + 1, rb), 0xA5, dtype=torch.uint8, device=gpu)  # poison + canary record
            got = ops.gather_rows(idx._mmr_planes(), torch.tensor(rows, dtype=torch.int64).to(torch.int32), out=buf[:n])
            torch.cuda.synchronize()
            assert torch.equal(got.cpu(), want), (storage, D, n)
            assert bool((buf[n] == 0xA5).all())
            if n > 1:
                assert want[[i for i, r in enumerate(rows) if not 0 <= r < N]].sum() == 0
                assert want[[i for i, r in enumerate(rows) if 0 <= r < N]].any()
    # through the index (its lock and stream), on its device
    rows = torch.tensor([0, N - 1, -1, 5], dtype=torch.int32)
    got = idx.gather_rows(rows)
    torch.cuda.synchronize()
    assert got.device == idx.device and torch.equal(got.cpu(), _expected_records(idx, rows))
    assert torch.equal(got.cpu(), ref.gather_rows(_cpu_planes(idx), rows))  # the CPU path agrees


# ---------------------------------------------------------------------------- mmr_select_rows
def _lists(m, seed):
    """QMAX candidate lists of m entries: lengths 0..m (query 0 full, query 1 empty). Even
    queries take neighbours (tile 0 with the copies 0 and 5, then the partial last tile and tiles
    1..3); odd queries spread over all tiles, the duplicate rows first. Scores descend, with ties."""
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


def _shuffled_records(idx, seed):
    """All N rows' records (the reference gather) at shuffled places of a buffer with spare
    records; returns (recs on the GPU, place of every row)."""
    g = torch.Generator().manual_seed(seed)
    R = N + 9
    place = torch.randperm(R, generator=g)[:N]
    rec = ref.gather_rows(_cpu_planes(idx), torch.arange(N))
    buf = torch.randint(0, 256, (R, rec.shape[1]), generator=g).to(torch.uint8)  # spare records: never read
    buf[place] = rec
    return buf.to(idx.device), place


def _slots(rows, place, R, seed):
    """slot lists of the row lists: the list ends at -1 (even queries) or at an entry >= R (odd
    ones: R itself, or 2^31 - 1); what follows the end is arbitrary and never dereferenced."""
    g = torch.Generator().manual_seed(seed)
    Q, m = rows.shape
    slot = torch.randint(0, R, (Q, m), generator=g).int()
    ok = rows >= 0
    slot[ok] = place[rows[ok].long()].int()
    for q in range(Q):
        n = int(ok[q].sum())
        if n < m:
            slot[q, n] = -1 if q % 2 == 0 else (R if q % 4 == 1 else BIG)
    return slot


def _poisoned(Q, k, dev):
    return (torch.full((Q, k), float("nan"), device=dev), torch.full((Q, k), POISON, dtype=torch.int32, device=dev))


def _prefix(full_p, full_s, k):
    """The k-selection from the m-selection (greedy selection is prefix-consistent), padded past m."""
    Q, m = full_p.shape
    p = torch.full((Q, k), -1, dtype=torch.int32)
    s = torch.full((Q, k), float("-inf"))
    p[:, :min(k, m)] = full_p[:, :k]
    s[:, :min(k, m)] = full_s[:, :k]
    return p, s


_q16_cache = {}


def _q16_case(D, m, dev):
    key = (D, m)
    if key not in _q16_cache:
        idx = _index("q16", D, dev)
        rows, scores = _lists(m, seed=m)
        wr, wd = ops.mmr_weights([DIVERSITY[q % 4] for q in range(QMAX)])
        if ("gram", D) not in _q16_cache:  # s_ij of all N rows and the record buffer, once per index
            _q16_cache["gram", D] = ref.q16_pairwise(*_cpu_planes(idx), torch.arange(N))
            _q16_cache["recs", D] = _shuffled_records(idx, seed=D)
        gram = _q16_cache["gram", D]
        ep = torch.empty(QMAX, m, dtype=torch.int32)
        es = torch.empty(QMAX, m)
        for q in range(QMAX):
            c = rows[q].long().clamp(min=0)
            n = int((rows[q] >= 0).sum())
            pos = torch.full((m,), -1, dtype=torch.int64)
            pos[:n] = torch.arange(n)
            es[q], ep[q] = ref.mmr_select(scores[q], pos, gram[c][:, c], m, wr[q], wd[q])
        _q16_cache[key] = (idx, rows, scores, wr, wd, ep, es)
    return _q16_cache[key] + _q16_cache["recs", D]


def _rows_of(pos, rows):
    """List positions -> the rows listed there (-1 past the picks)."""
    g = torch.gather(rows.long(), 1, pos.long().clamp(min=0))
    return torch.where(pos >= 0, g, torch.full_like(g, -1)).int()


@pytest.mark.parametrize("m", [1, 2, 17, 64])
@pytest.mark.parametrize("D", [64, 192, 1024])
def test_select_rows_q16_bit_identical(gpu, D, m):
    idx, rows, scores, wr, wd, full_p, full_s, recs, place = _q16_case(D, m, gpu)
    slot = _slots(rows, place, recs.shape[0], seed=D + m)
    for Q in (1, 3, QMAX):
        for k in sorted({1, 5, m}):
            ep, es = _prefix(full_p[:Q], full_s[:Q], k)
            out = _poisoned(Q, k, gpu)
            s, p = ops.mmr_select_rows(recs, slot[:Q].to(gpu), scores[:Q].to(gpu), k, wr[:Q], wd[:Q], out=out)
            assert torch.equal(p.cpu(), ep), (D, m, Q, k)
            assert torch.equal(s.cpu().view(torch.int32), es.view(torch.int32)), (D, m, Q, k)  # bit for bit
            # mapped to rows: the tile kernel on the same candidates
            ts, tr = ops.mmr_select(rows[:Q].to(gpu), scores[:Q].to(gpu), idx._mmr_planes(), k, wr[:Q], wd[:Q],
                                    out=_poisoned(Q, k, gpu))
            assert torch.equal(_rows_of(p.cpu(), rows[:Q]), tr.cpu())
            assert torch.equal(s.cpu().view(torch.int32), ts.cpu().view(torch.int32))


@pytest.mark.parametrize("D", [96, 1024])
def test_select_rows_bf16_is_the_tile_kernel_and_within_the_bound(gpu, D):
    """Bit-identical to mmr_select on the same candidates; and every pick is, in the fp64
    reference, within 2 eps of the best open candidate, eps = 2 (D + 8) 2^-24: the worst-case error
    of a D-term fp32 accumulation of unit-norm rows (D u sum|a_i b_i| <= D u, u = 2^-24, doubled
    for the unknown summation tree, + 8 u for the three fp32 operations of the MMR value and the
    unit-norm slack of bf16 rows); it bounds rel and s_ij alike and wr + wd = 1, so each
    candidate's value is off by at most eps, and the pick and the best are two candidates."""
    idx = _index("bf16", D, gpu)
    g = torch.Generator().manual_seed(D)
    Q, m = QMAX, 64
    queries = torch.nn.functional.normalize(
        _vectors(D, 1)[torch.randint(0, N, (Q,), generator=g)] + 0.7 * torch.randn(Q, D, generator=g) / D ** 0.5, dim=1)
    stored = idx.read_rows(0, N).double().cpu()
    qb = queries.to(torch.bfloat16).double()
    scores, rows = torch.topk(qb.float() @ stored.float().T, m, dim=1)
    rows = rows.int()
    lens = torch.randint(0, m + 1, (Q,), generator=g)
    lens[0], lens[1] = m, 0
    for q in range(Q):
        rows[q, lens[q]:] = -1
        scores[q, lens[q]:] = float("-inf")
    d = [DIVERSITY[q % 4] for q in range(Q)]
    wr, wd = ops.mmr_weights(d)
    recs, place = _shuffled_records(idx, seed=D)
    slot = _slots(rows, place, recs.shape[0], seed=D)
    gram = ref.bf16_pairwise(idx.packed.cpu(), torch.arange(N))  # fp64 s_ij of all N rows
    eps = 2 * (D + 8) * 2.0 ** -24
    for k in (1, 5, m):
        s, p = ops.mmr_select_rows(recs, slot.to(gpu), scores.to(gpu), k, wr, wd, out=_poisoned(Q, k, gpu))
        ts, tr = ops.mmr_select(rows.to(gpu), scores.to(gpu), idx._mmr_planes(), k, wr, wd, out=_poisoned(Q, k, gpu))
        s, p = s.cpu(), p.cpu()
        assert torch.equal(_rows_of(p, rows), tr.cpu()), (D, k)
        assert torch.equal(s.view(torch.int32), ts.cpu().view(torch.int32)), (D, k)
        for q in range(Q):
            n = int(lens[q])
            cand = rows[q, :n].long()
            picks = min(k, n)
            assert (p[q, picks:] == -1).all() and (s[q, picks:] == float("-inf")).all()
            if d[q] == 0.0:  # the first k candidates, bit for bit
                assert p[q, :picks].tolist() == list(range(picks)) and torch.equal(s[q, :picks], scores[q, :picks])
            rel = stored[cand] @ qb[q]
            sims = gram[cand][:, cand]
            open_ = torch.ones(n, dtype=torch.bool)
            M = torch.zeros(n, dtype=torch.float64)
            for step in range(picks):
                at = int(p[q, step])
                assert 0 <= at < n and open_[at]  # a listed candidate, not picked before
                assert s[q, step] == scores[q, at]  # reported with its cosine score
                val = float(wr[q]) * rel - (float(wd[q]) * M if step else 0.0)
                best = val[open_].max()
                assert val[at] >= best - 2 * eps, (D, k, q, step, float(best - val[at]), eps)
                open_[at] = False
                M = sims[:, at].clone() if step == 0 else torch.maximum(M, sims[:, at])


# ---------------------------------------------------------------------------- the node store
CL_D, CL_PER, CL_N = 256, 10, 40


def _cluster_data(dim=CL_D, seed=5):
    g = np.random.default_rng(seed)
    base = g.standard_normal((CL_N, dim)).astype(np.float32)
    vecs = np.repeat(base, CL_PER, axis=0) + 0.12 * g.standard_normal((CL_N * CL_PER, dim)).astype(np.float32)
    queries = base[:6] + 0.05 * g.standard_normal((6, dim)).astype(np.float32)
    return vecs, queries.astype(np.float32)


NODE_K = [1, 3, 6, 6, 3, 3]
NODE_DIV = [0.3, 0.7, 1.0, 0.5, 0.0, 0.5]
NODE_FETCH = [None, None, 64, 8, None, 16]


@pytest.mark.parametrize("storage", ["bf16", "q16"])
def test_world1_node_store_on_a_gpu_index(gpu, storage):
    from pilottai_amd.memory.node_store import NodeSemanticStore

    vecs, queries = _cluster_data()
    n = len(vecs)
    idx = SemanticIndex(dim=CL_D, capacity=512, device=gpu, storage=storage)
    idx.add(vecs, [0] * n, [()] * n, [None] * n)
    want = [idx.search(queries[i:i + 1], NODE_K[i], [0], [()], diversity=NODE_DIV[i], fetch_k=NODE_FETCH[i])[0]
            for i in range(6)]
    plain = [idx.search(queries[i:i + 1], NODE_K[i], [0], [()])[0] for i in range(6)]
    store = NodeSemanticStore(idx, cross_shard_mmr=True)
    store.start()
    try:
        got = store.search_rows_blocking(queries, NODE_K, [0] * 6, [()] * 6, timeout=60, diversity=NODE_DIV,
                                         fetch_k=NODE_FETCH)
    finally:
        store.stop(timeout=30)
    assert [[r for r, _ in lst] for lst in got] == [[r for r, _ in lst] for lst in want]
    if storage == "q16":
        assert got == want  # scores bit for bit
    else:
        np.testing.assert_allclose([s for lst in got for _, s in lst], [s for lst in want for _, s in lst],
                                   rtol=0, atol=1e-6)
    assert any(w != p for w, p, d in zip(want, plain, NODE_DIV) if d > 0)  # the re-ranking changed something
    assert store.stats["mmr_rows"] > 0 and store.stats["mmr_lookups"] == 5 and store.stats["mmr_rounds"] == 1


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _gpu_rank(rank, world, port, q):
    import torch.distributed as dist

    from pilottai_amd.memory.node_store import NodeSemanticStore

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        vecs, queries = _cluster_data(dim=64)
        mine = list(range(rank, len(vecs), world))
        local = SemanticIndex(dim=64, capacity=256, device="cuda:0", storage="q16")
        local.add(vecs[mine], [0] * len(mine), [()] * len(mine), [None] * len(mine))
        grp = dist.new_group(backend="gloo")
        store = NodeSemanticStore(local, group=grp, cross_shard_mmr=True)
        store.start()
        got = store.search_rows_blocking(queries, NODE_K, [0] * 6, [()] * 6, timeout=60, diversity=NODE_DIV,
                                         fetch_k=NODE_FETCH)
        rows = store.stats["mmr_rows"]
        dist.barrier()
        store.stop(timeout=30)
        q.put((rank, got, rows))
    except BaseException:
        q.put((rank, traceback.format_exc(), -1))
        raise
    finally:
        dist.destroy_process_group()


def test_two_ranks_with_gpu_indexes_over_gloo(gpu):
    """The shared-GPU rehearsal layout: two ranks, each with a q16 shard on the GPU, a gloo group
    (the records pass through the host). Equal to a CPU index holding all rows: the same rows in
    the same order. The scores are compared within the 1e-6 of tests/test_node_memory.py, not bit
    for bit: a query is normalised in fp32 on the device of the index that scans it, and the GPU's
    and the CPU's reductions differ in the last bit, so the query's scale and fixed-point digits --
    and with them every score -- can differ by an ulp or two (6e-8 each) between the two."""
    vecs, queries = _cluster_data(dim=64)
    n = len(vecs)
    single = SemanticIndex(dim=64, capacity=512, device="cpu", storage="q16")
    single.add(vecs, [0] * n, [()] * n, [None] * n)
    want = [single.search(queries[i:i + 1], NODE_K[i], [0], [()], diversity=NODE_DIV[i], fetch_k=NODE_FETCH[i])[0]
            for i in range(6)]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gpu_rank, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = []
    deadline = time.monotonic() + 150
    try:
        while len(got) < 2:  # wait on the queue, but not for a rank that has failed or died
            try:
                item = q.get(timeout=0.5)
            except queue.Empty:
                assert all(p.exitcode in (None, 0) for p in procs), [p.exitcode for p in procs]
                assert time.monotonic() < deadline, "the ranks did not answer in time"
                continue
            assert item[2] >= 0, f"rank {item[0]} failed:\n{item[1]}"
            got.append(item)
        for p in procs:
            p.join(timeout=60)
    finally:
        for p in procs:  # no retries; nothing is left running
            if p.is_alive():
                p.kill()
    assert [p.exitcode for p in procs] == [0, 0]
    for rank, lists, rows in got:
        assert [[r for r, _ in lst] for lst in lists] == [[r for r, _ in lst] for lst in want], rank
        np.testing.assert_allclose([s for lst in lists for _, s in lst], [s for lst in want for _, s in lst],
                                   rtol=0, atol=1e-6)
        assert rows > 0
