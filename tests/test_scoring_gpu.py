"""Prompt scoring on the GPU: the HIP pass (csrc/ops/scoring.hip) against ops.reference.score_tokens,
and the engine's scoring step graphs end to end.

Tolerance of the kernel tests: ids and ranks exactly (every ordering decision is an integer
comparison on the bf16 order key), logprobs within 5e-4 absolute -- the tolerance
tests/test_logprobs_gpu.py derives for this same chunked fp32 log-sum-exp: it is within 1e-6 of
fp64 at these sizes, fast-math exp/log add a few 1e-6 relative, and the smallest structural error
the small-V cases produce (one dropped 16-byte vector at V = 264) moves the normaliser by about
3e-2 -- and such a dropped vector also moves a rank there."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from scoring_checks import Server, record_consistent  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENTINEL = -7
TOL = 5e-4
NEG_INF = float("-inf")


def _run(dev, logits, target, lp_n):
    """The kernel on poisoned outputs / workspace, and the reference; both on the CPU."""
    from pilottai_amd import ops
    from pilottai_amd.ops import reference as ref

    rows, V = logits.shape
    target = torch.as_tensor(target, dtype=torch.int32)
    lp_n = torch.as_tensor(lp_n, dtype=torch.int32)
    lp = torch.full((rows,), NAN, dtype=torch.float32, device=dev)
    rank = torch.full((rows,), SENTINEL, dtype=torch.int32, device=dev)
    ids = torch.full((rows, 20), SENTINEL, dtype=torch.int32, device=dev)
    lps = torch.full((rows, 20), NAN, dtype=torch.float32, device=dev)
    ws = ops.score_tokens_workspace(rows, V, dev).fill_(NAN)
    ops.score_tokens(logits, target.to(dev), lp_n.to(dev), out=(lp, rank, ids, lps), workspace=ws)
    torch.cuda.synchronize()
    want = ref.score_tokens(logits.cpu(), target, lp_n)
    return (lp.cpu(), rank.cpu(), ids.cpu(), lps.cpu()), want, target


def _close(a, b, what):
    assert not torch.isnan(a).any(), (what, a)
    assert torch.equal(torch.isinf(a), torch.isinf(b)), (what, a, b)
    fin = ~torch.isinf(b)
    err = float((a[fin].double() - b[fin].double()).abs().max()) if bool(fin.any()) else 0.0
    print(f"{what}: max |logprob error| = {err:.3e}")
    assert err <= TOL, (what, err)


def _check(got, want, target):
    (lp, rank, ids, lps), (r_lp, r_rank, r_ids, r_lps) = got, want
    for r in range(lp.shape[0]):
        if int(target[r]) < 0:  # skipped: the poison is still there
            assert math.isnan(float(lp[r])) and int(rank[r]) == SENTINEL, r
            assert bool((ids[r] == SENTINEL).all()) and bool(torch.isnan(lps[r]).all()), r
            continue
        assert int(rank[r]) == int(r_rank[r]), (r, int(rank[r]), int(r_rank[r]))
        assert torch.equal(ids[r], r_ids[r]), (r, ids[r], r_ids[r])
        _close(lp[r:r + 1], r_lp[r:r + 1], f"row {r} target")
        _close(lps[r], r_lps[r], f"row {r} list")


def _logits(V, ld, rows, seed):
    """Random bf16 rows inside a wider buffer whose padding would win every comparison."""
    g = torch.Generator().manual_seed(seed)
    buf = torch.full((rows, ld), 30000.0, dtype=torch.bfloat16)
    buf[:, :V] = (torch.randn(rows, V, generator=g) * 3).to(torch.bfloat16)
    return buf


@pytest.mark.parametrize("V,ld,rows", [(264, 272, 3), (4104, 4104, 3), (4104, 4104, 17), (12288, 12288, 2)])
def test_kernel_shapes_targets_and_skipped_rows(gpu, V, ld, rows):
    """Padded rows, a second chunk of 8 entries, one / several chunks, 2..17 rows; targets at id 0,
    id V-1, in the short tail chunk, at a logit of -inf, outside the vocabulary, and skipped rows."""
    buf = _logits(V, ld, rows, V + rows)
    kinds = ["zero", "last", "tail", "neginf", "outside", "skip", "mid"]
    target, lp_n = [], []
    for r in range(rows):
        kind = kinds[r % len(kinds)] if rows > 3 else ("zero", "last", "tail")[r]
        t = {"zero": 0, "last": V - 1, "tail": V - 5, "neginf": 17 + r, "outside": V + 3 * r, "skip": -1,
             "mid": (V // 2 + 11 * r) % V}[kind]
        if kind == "neginf":
            buf[r, t] = NEG_INF
            buf[r, 3] = NEG_INF  # and one that is not the target: never listed, still ranked
        target.append(t)
        lp_n.append((0, 1, 20)[r % 3])
    if rows == 2:  # the 12,288 case: a -inf target and an id >= V, with lists
        buf[0, 9000] = NEG_INF
        target, lp_n = [9000, V], [20, 1]
    logits = buf.to(gpu)[:, :V]
    assert rows == 1 or logits.stride(0) == ld
    got, want, tg = _run(gpu, logits, target, lp_n)
    _check(got, want, tg)
    lp, rank, ids, lps = got
    assert int(ids.max()) < V
    for r in range(rows):
        t, n = target[r], lp_n[r]
        if t >= V:
            assert float(lp[r]) == NEG_INF and int(rank[r]) == 0
        if t >= 0:
            assert ids[r, n:].tolist() == [-1] * (20 - n) and bool(torch.isinf(lps[r, n:]).all())
        if 0 <= t < V and float(buf[r, t]) == NEG_INF:
            assert float(lp[r]) == NEG_INF and int(rank[r]) >= V - 1 and t not in ids[r].tolist()
        if 0 <= t < V:
            record_consistent(t, float(lp[r]), int(rank[r]), ids[r].tolist(), lps[r].tolist(), n)


def test_kernel_llama_vocab_row_pair(gpu):
    """One row pair at 128,256: the last (partial) chunk, a target deep in the tail of the
    distribution and the most likely token."""
    V = 128256
    logits = _logits(V, V, 2, 1)
    low = int(torch.argsort(logits[0].float(), descending=True, stable=True)[100000])
    top = int(torch.argmax(logits[1].float()))
    got, want, tg = _run(gpu, logits.to(gpu), [low, top], [20, 5])
    _check(got, want, tg)
    lp, rank, ids, lps = got
    assert int(rank[0]) == 100001 and low not in ids[0].tolist() and float(lp[0]) < float(lps[0, 19])
    assert int(rank[1]) == 1 and int(ids[1, 0]) == top and float(lp[1]) == float(lps[1, 0])
    assert ids[1, 5:].tolist() == [-1] * 15


def test_kernel_ties_across_a_chunk_boundary_and_signed_zero(gpu):
    """80 equal logits over ids 4056..4135 (the chunk boundary is at 4096): the rank of a tied
    target is its place among them by id. All-equal rows rank t + 1; -0 ranks below +0."""
    V = 12288
    g = torch.Generator().manual_seed(3)
    rows = (torch.randn(5, V, generator=g) * 2).to(torch.bfloat16)
    tied = list(range(4056, 4136))
    rows[0, tied] = 19.0  # above everything else
    rows[1, tied] = 0.5   # in the middle of the distribution
    rows[2] = 1.25        # an all-equal row
    rows[3] = 0.0
    rows[3, ::2] = -0.0   # even ids hold -0, odd ids +0
    rows[4] = rows[0]
    target = [4100, 4130, 7777, 6, tied[0]]
    got, want, tg = _run(gpu, rows.to(gpu), target, [20, 20, 20, 20, 1])
    _check(got, want, tg)
    lp, rank, ids, lps = got
    assert int(rank[0]) == 1 + (4100 - 4056) and ids[0].tolist() == tied[:20]
    above = int((rows[1].float() > 0.5).sum())
    equal_before = int((rows[1, :4130].float() == 0.5).sum())  # the 74 tied ids in front, and any random 0.5
    assert equal_before >= 4130 - 4056 and int(rank[1]) == 1 + above + equal_before
    assert int(rank[2]) == 7777 + 1 and ids[2].tolist() == list(range(20))
    assert abs(float(lp[2]) + math.log(V)) <= TOL
    assert int(rank[3]) == 1 + V // 2 + 3  # every +0 (odd id) first, then the -0 ids 0, 2, 4 before 6
    assert ids[3].tolist() == list(range(1, 41, 2))
    assert int(rank[4]) == 1 and ids[4].tolist() == [tied[0]] + [-1] * 19


# ---------------------------------------------------------------------------
# engine
# ---------------------------------------------------------------------------

def _make_engine(gpu, **kw):
    from pilottai_amd.engine.engine import EngineConfig, LLMEngine

    return LLMEngine(EngineConfig(model="tiny-gqa4", max_num_seqs=16, max_num_batched_tokens=512,
                                  max_model_len=2048, num_kv_blocks=512, token_buckets=[16, 64, 256], **kw),
                     device=gpu)


@pytest.fixture(scope="module")
def engine(gpu):
    e = _make_engine(gpu, keep_graphs=True)
    yield e
    e.stop()


def test_engine_scoring_graph_is_captured_on_first_use_and_leaves_the_plain_graphs_alone(engine):
    from pilottai_amd import ops
    from pilottai_amd.utils.tracing import graph_node_counts

    tok = engine.tok
    ctx, cand = tok.encode("hi there"), tok.encode(" you")
    assert len(ctx) + len(cand) <= 16
    before = set(engine._graphs)
    assert all(len(k) < 8 for k in before) and (16, False, False) in before
    g_plain = engine._graphs[(16, False, False)]
    o = engine.score(ctx, [cand], top=2)[0]
    key = (16, False, False, False, False, False, False, True)
    assert set(engine._graphs) == before | {key}
    assert o.finish_reason == "score" and o.token_ids == [] and len(o.prompt_logprobs) == len(cand)
    plain = graph_node_counts(g_plain)
    scored = graph_node_counts(engine._graphs[key])
    assert scored["kernel"] == plain["kernel"] + ops.SCORE_TOKENS_LAUNCHES
    assert {k: v for k, v in scored.items() if k != "kernel"} == {k: v for k, v in plain.items() if k != "kernel"}
    n_graphs, captures = len(engine._graphs), engine.stats["graph_captures"]
    g = engine.generate([ctx], temperature=0.0, max_tokens=4, ignore_eos=True)[0]
    assert g.prompt_logprobs is None and len(g.token_ids) == 4
    assert engine._graphs[(16, False, False)] is g_plain and len(engine._graphs) == n_graphs
    assert engine.stats["graph_captures"] == captures
    engine.score(ctx, [cand], top=2)  # replayed, not captured again
    assert engine.stats["graph_captures"] == captures


def test_engine_records_match_the_reference_forward_and_are_self_consistent(engine):
    """Each logprob is within 0.1 of log_softmax of the dense fp32 forward, the tolerance
    tests/test_logprobs_gpu.py::test_engine_logprobs_match_the_reference_forward uses against the
    same reference; every record is self-consistent, checked exactly. The 40-token candidate is
    scored over several steps of at most 16 rows."""
    tok = engine.tok
    ctx = tok.encode("The orchestrator analyses a task and delegates it to worker agents " * 3)
    cands = [tok.encode(" and waits"), tok.encode(" then it collects every result and judges it again" * 8)[:40]]
    assert len(cands[1]) == 40
    n = 5
    outs = engine.score(ctx, cands, top=n)
    for c, o in zip(cands, outs):
        full = ctx + c
        ref = torch.log_softmax(engine.model.reference_logits(full).float(), dim=-1)
        assert o.finish_reason == "score" and o.token_ids == [] and len(o.prompt_logprobs) == len(c)
        assert o.prompt_tokens == len(full) and o.cached_prompt_tokens <= len(ctx) - 1
        assert abs(o.cumulative_logprob - sum(e[0] for e in o.prompt_logprobs)) < 1e-9
        for i, (lp, rank, top) in enumerate(o.prompt_logprobs):
            p = len(ctx) + i
            want = float(ref[p - 1, full[p]])
            print(f"position {p}: engine {lp:.4f} reference {want:.4f} rank {rank}")
            assert abs(lp - want) <= 0.1, (p, lp, want)
            ids = [t for t, _ in top] + [-1] * (20 - len(top))
            lps = [v for _, v in top] + [NEG_INF] * (20 - len(top))
            record_consistent(full[p], lp, rank, ids, lps, n)
    assert outs[1].cached_prompt_tokens > 0  # the second candidate found the context in the prefix cache


def test_engine_mixed_batch_of_decoding_logprob_and_scoring_requests(engine):
    tok = engine.tok
    ctx = tok.encode("request number seven asks the agents for a plan")
    res = {}
    for i in range(9):
        cb = lambda o, i=i: res.__setitem__(i, o)  # noqa: E731
        if i % 3 == 0:
            engine.submit(ctx + tok.encode(f" option {i} is the one to take"), cb, score_from=len(ctx), logprobs=3)
        else:
            engine.submit(tok.encode(f"request number {i} asks for a plan"), cb, temperature=0.8, max_tokens=10,
                          ignore_eos=True, seed=100 + i, logprobs=3 if i % 3 == 1 else -1)
    while len(res) < 9:
        assert engine.step() or len(res) == 9
    for i in range(9):
        o = res[i]
        if i % 3 == 0:
            n_c = len(tok.encode(f" option {i} is the one to take"))
            assert o.finish_reason == "score" and o.token_ids == [] and len(o.prompt_logprobs) == n_c
            assert o.logprobs is None
            for lp, rank, top in o.prompt_logprobs:
                assert math.isfinite(lp) and lp <= 0.0 and rank >= 1 and len(top) == 3
        else:
            assert o.finish_reason == "length" and len(o.token_ids) == 10 and o.prompt_logprobs is None
            assert (o.logprobs is not None and len(o.logprobs) == 10) if i % 3 == 1 else o.logprobs is None
    assert engine.sched.num_running == 0 and engine.sched.num_waiting == 0


def test_http_score_on_the_gpu_engine(engine):
    import httpx

    from pilottai_amd.core.config import LLMConfig
    from pilottai_amd.engine.local_llm import LocalLLM
    from pilottai_amd.serving.http_server import create_app

    engine.start()
    try:
        backend = LocalLLM(LLMConfig(model_name="tiny-gqa4", max_tokens=64, retry_attempts=1), engine=engine)
        with Server(create_app(backend, "tiny-gqa4", engine=engine)) as url:
            r = httpx.post(f"{url}/score", timeout=60, json={
                "context": [{"role": "user", "content": "which agent takes the task?"}],
                "candidates": ["the planner", "the reviewer agent"], "top_logprobs": 2})
        assert r.status_code == 200, r.text
        data = r.json()
        assert data["object"] == "score" and data["model"] == "tiny-gqa4" and len(data["scores"]) == 2
        for s, text in zip(data["scores"], ["the planner", "the reviewer agent"]):
            assert "".join(t["token"] for t in s["tokens"]) == text
            assert abs(s["logprob"] - sum(t["logprob"] for t in s["tokens"])) < 1e-6
            for t in s["tokens"]:
                assert t["rank"] >= 1 and t["logprob"] <= 0.0 and len(t["top_logprobs"]) == 2
        assert data["usage"]["prompt_tokens"] > 0 and data["usage"]["completion_tokens"] == 0
    finally:
        engine.stop()
