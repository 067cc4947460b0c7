"""Prompt scoring, CPU tier: the fp64 reference op against a brute force, the scheduler's scoring
rows with fabricated records, the tiny CPU engine (serial and pipelined loop, chunked and
unchunked), the refusals, and the LocalLLM / HTTP surfaces."""
import asyncio
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from scoring_checks import Server, brute_rank, order_keys, record_consistent  # noqa: E402

from pilottai_amd import _runtime  # noqa: E402

W = 42  # 32-bit words per score record: logprob, rank, 20 ids, 20 logprobs
POISON = -777
SCORE_BIT = 1 << 30
FINISH_SCORE = 4


# ---------------------------------------------------------------------------
# reference op
# ---------------------------------------------------------------------------

def test_reference_matches_a_brute_force():
    """fp64 log-softmax by numpy and the rank as a literal double loop, on random bf16 rows at
    V = 264, an all-equal row (rank t + 1), a row of +-0 and a target at -inf."""
    from pilottai_amd.ops import reference as ref

    V = 264
    g = torch.Generator().manual_seed(0)
    rows = (torch.randn(8, V, generator=g) * 3).to(torch.bfloat16)
    rows[3] = 0.75                      # all equal
    rows[4] = 0.0
    rows[4, ::2] = -0.0                 # even ids -0, odd ids +0
    rows[5, 100] = float("-inf")        # the target itself
    rows[5, 7] = float("-inf")
    rows[6, :50] = rows[6, 60]          # a block of ties in a random row
    target = [0, V - 1, 131, 200, 6, 100, 60, -1]
    lp_n = [20, 0, 5, 20, 20, 3, 20, 20]
    lp, rank, ids, lps = ref.score_tokens(rows, torch.tensor(target), torch.tensor(lp_n))
    bits = rows.view(torch.int16).numpy()
    x = rows.float().numpy().astype(np.float64)
    for r, (t, n) in enumerate(zip(target, lp_n)):
        if t < 0:  # skipped
            assert math.isnan(float(lp[r])) and int(rank[r]) == -1 and bool((ids[r] == -1).all())
            continue
        keys = order_keys(bits[r])
        assert int(rank[r]) == brute_rank(keys, t), r
        with np.errstate(divide="ignore"):
            want = x[r] - np.log(np.exp(x[r]).sum())
        assert float(lp[r]) == pytest.approx(want[t], abs=1e-6) if np.isfinite(want[t]) else float(lp[r]) == -math.inf
        order = sorted((i for i in range(V) if x[r, i] > -np.inf), key=lambda i: (-int(keys[i]), i))[:n]
        assert ids[r, :len(order)].tolist() == order and ids[r, len(order):].tolist() == [-1] * (20 - len(order))
        assert np.allclose(lps[r, :len(order)].numpy(), want[order], atol=1e-6)
        assert bool(torch.isinf(lps[r, len(order):]).all())
        record_consistent(t, float(lp[r]), int(rank[r]), ids[r].tolist(), lps[r].tolist(), n)
    assert int(rank[3]) == 200 + 1
    assert int(rank[4]) == 1 + V // 2 + 3 and ids[4, :3].tolist() == [1, 3, 5]  # -0 ranks below +0
    assert float(lp[5]) == -math.inf and int(rank[5]) == V and 100 not in ids[5].tolist()
    assert int(rank[6]) >= 51 or float(rows[6, 60]) >= float(rows[6].float().max())
    out = ref.score_tokens(rows[:1], torch.tensor([V + 5]), torch.tensor([2]))
    assert float(out[0][0]) == -math.inf and int(out[1][0]) == 0 and int(out[2][0, 0]) >= 0


def test_ops_dispatch_leaves_skipped_rows_alone():
    from pilottai_amd import ops

    g = torch.Generator().manual_seed(1)
    rows = (torch.randn(3, 64, generator=g)).to(torch.bfloat16)
    out = (torch.full((3,), 5.0), torch.full((3,), -9, dtype=torch.int32),
           torch.full((3, 20), -9, dtype=torch.int32), torch.full((3, 20), 5.0))
    ops.score_tokens(rows, torch.tensor([3, -1, 63], dtype=torch.int32), torch.tensor([1, 1, 0], dtype=torch.int32),
                     out=out)
    assert float(out[0][1]) == 5.0 and int(out[1][1]) == -9 and bool((out[2][1] == -9).all())
    assert float(out[0][0]) < 0 and int(out[1][2]) >= 1 and out[2][2].tolist() == [-1] * 20


# ---------------------------------------------------------------------------
# scheduler
# ---------------------------------------------------------------------------

def _sched(**kw):
    cfg = {"num_blocks": 64, "block_size": 16, "max_num_seqs": 8, "max_num_batched_tokens": 256,
           "max_prefill_tokens": 256, "max_model_len": 512, "eos_ids": [2]}
    cfg.update(kw)
    s = _runtime.Scheduler(cfg)
    L = s.layout()
    buf = np.full(L["score_total"], POISON, dtype=np.int32)
    return s, L, buf


def _fabricate(target: int, pos: int) -> np.ndarray:
    """A score record that names the row it was made for."""
    rec = np.zeros(W, dtype=np.int32)
    rec[:1].view(np.float32)[0] = -(target % 89) - pos / 1024.0
    rec[1] = pos * 1000 + target % 1000 + 1
    rec[2:22] = -1
    rec[2] = target
    rec[22:42].view(np.float32)[:] = -np.inf
    rec[22:23].view(np.float32)[0] = -0.25
    return rec


def _drive(s, L, buf, prompts, on_step=None, max_steps=400, words=None):
    """schedule / commit until idle. Checks every step's row bookkeeping and returns (outputs by id,
    per-step dicts). `prompts`: id -> token list, to check the targets."""
    outs, steps = {}, []
    ms = L["max_seqs"]
    for step in range(max_steps):
        if on_step is not None:
            on_step(step)
        if not s.has_work():
            break
        buf[:] = POISON
        T = s.schedule(buf.ctypes.data, buf.size if words is None else words)
        if T == 0:
            break
        c = buf[L["counts"]:L["counts"] + 12]
        ns, nsamp = int(c[1]), int(c[2])
        assert nsamp <= ms and ns <= ms
        scoring = bool(int(c[9]) & SCORE_BIT)
        tg = buf[L["score_target"]:L["score_target"] + ms]
        forced = buf[L["forced"]:L["forced"] + ms]
        rows = buf[L["logit_rows"]:L["logit_rows"] + ms]
        off = buf[L["offsets"]:L["offsets"] + ms]
        ids = buf[L["input_ids"]:L["input_ids"] + T]
        pos = buf[L["positions"]:L["positions"] + T]
        recs = np.zeros((max(1, nsamp), W), dtype=np.int32)
        n_score = 0
        if scoring:
            assert bool((tg[nsamp:] == -1).all())
            for r in range(nsamp):
                t = int(tg[r])
                if t < 0:
                    continue
                n_score += 1
                # the row sits on the token before the target and is inert for the sampler
                assert int(forced[r]) == t and int(buf[L["mask_class"] + r]) == -1
                assert int(off[r]) == int(pos[rows[r]]) + 1
                recs[r] = _fabricate(t, int(off[r]))
        else:
            assert bool((tg == POISON).all())  # the region is not written
        steps.append({"T": T, "nsamp": nsamp, "n_score": n_score, "scoring": scoring,
                      "words": buf[:L["rep_total"]].copy(), "ids": ids.copy(), "pos": pos.copy()})
        sampled = np.where(forced[:max(1, nsamp)] >= 0, forced[:max(1, nsamp)], 7).astype(np.int32)
        for o in s.commit(sampled.ctypes.data, nsamp, 0, recs.ctypes.data if scoring else 0):
            outs[o[0]] = o
    for o in s.drain_aborted():
        outs[o[0]] = o
    return outs, steps


def _expected(prompt, k, n=0):
    out = []
    for p in range(k, len(prompt)):
        rec = _fabricate(prompt[p], p)
        out.append((float(rec[:1].view(np.float32)[0]), int(rec[1]), [(int(rec[2]), -0.25)][:n]))
    return out


def test_scheduler_long_continuation_is_cut_to_the_row_budget_and_decode_rows_come_first():
    """A 40-token continuation under max_num_seqs = 8 takes at least 5 steps, no step has more than
    8 rows, and two decoding requests get their row in every one of them."""
    s, L, buf = _sched()
    ctx = list(range(100, 130))
    prompt = ctx + list(range(500, 540))
    for rid in (1, 2):  # two decoding requests, running before the scoring request arrives
        s.add_request(rid, list(range(10 * rid, 10 * rid + 5)), 0.0, 30, rid, True, [], None)
    outs, steps = _drive(s, L, buf, {}, max_steps=1)
    assert steps[0]["nsamp"] == 2
    s.add_request(3, prompt, 0.0, 1, 3, True, [], None, logprobs=1, score_from=len(ctx))
    outs, steps = _drive(s, L, buf, {3: prompt})
    sc = [st for st in steps if st["scoring"]]
    assert len(sc) >= 5 and sum(st["n_score"] for st in sc) == 40
    for st in sc:
        assert st["nsamp"] <= 8 and st["nsamp"] - st["n_score"] == 2, (st["nsamp"], st["n_score"])  # decode rows first
    assert max(st["n_score"] for st in sc) == 6
    o = outs[3]
    assert o[2] == FINISH_SCORE and o[1] == [] and o[3] == len(prompt) and len(o) == 11
    assert o[10] == _expected(prompt, len(ctx), 1)
    assert outs[1][2] == 1 and len(outs[1][1]) == 30  # the decoding requests ran to their length
    # the last prompt token predicts nothing: it is never an input and takes no row
    fed = [int(t) for st in sc for t in st["ids"]]
    assert prompt[-1] not in fed and prompt[-2] in fed
    assert sum(st["T"] for st in sc) - 2 * len(sc) == len(prompt) - 1


def test_scheduler_shares_the_context_through_the_prefix_cache():
    s, L, buf = _sched()
    ctx = list(range(100, 150))  # 50 tokens: three full blocks
    a, b = ctx + [7, 8, 9], ctx + [9, 8, 7, 6]
    s.add_request(1, a, 0.0, 1, 1, True, [], None, score_from=len(ctx))
    outs, steps = _drive(s, L, buf, {1: a})
    assert outs[1][4] == 0 and steps[0]["T"] == len(a) - 1 and steps[0]["n_score"] == 3
    s.add_request(2, b, 0.0, 1, 2, True, [], None, score_from=len(ctx))
    s.add_request(3, ctx[:33] + [1, 2], 0.0, 1, 3, True, [], None, score_from=33)
    outs, steps = _drive(s, L, buf, {2: b, 3: ctx[:33] + [1, 2]})
    assert outs[2][4] == 48 and 0 < outs[2][4] <= len(ctx) - 1  # never beyond k - 1
    # k - 1 = 32 is a block boundary: position 32 is computed, so only two blocks are reused
    assert outs[3][4] == 32 and outs[3][10] == _expected(ctx[:33] + [1, 2], 33)
    assert outs[2][10] == _expected(b, len(ctx))
    # a request whose k - 1 lies inside the first block reuses nothing
    s.add_request(4, ctx, 0.0, 1, 4, True, [], None, score_from=10)
    outs, _ = _drive(s, L, buf, {4: ctx})
    assert outs[4][4] == 0 and len(outs[4][10]) == 40
    # ... and what a scoring request computed serves a generation request
    s.add_request(5, a + [1], 0.0, 1, 5, True, [], None)
    outs, _ = _drive(s, L, buf, {})
    assert outs[5][4] == 48


def test_scheduler_preemption_gives_the_undisturbed_records():
    """Few KV blocks: a decoding request that keeps growing forces the scoring request out; it
    starts over and its final output equals that of an undisturbed run."""
    prompt = list(range(100, 140)) + list(range(700, 760))  # 100 tokens, scored from 40
    s, L, buf = _sched()
    s.add_request(1, prompt, 0.0, 1, 1, True, [], None, logprobs=1, score_from=40)
    calm, _ = _drive(s, L, buf, {1: prompt})
    s, L, buf = _sched(num_blocks=9, prefix_caching=False)
    s.add_request(2, list(range(10, 60)), 0.0, 60, 2, True, [], None)  # grows to 110 tokens: 7 blocks
    s.add_request(1, prompt, 0.0, 1, 1, True, [], None, logprobs=1, score_from=40)
    outs, steps = _drive(s, L, buf, {1: prompt})
    assert s.total_preemptions >= 1
    assert outs[1][2] == FINISH_SCORE and outs[1][10] == calm[1][10] == _expected(prompt, 40, 1)
    assert sum(st["n_score"] for st in steps) > 60  # some positions were scored twice


def test_scheduler_abort_of_a_scoring_request():
    s, L, buf = _sched()
    prompt = list(range(100, 160))
    s.add_request(1, prompt, 0.0, 1, 1, True, [], None, score_from=20)
    s.add_request(2, prompt[:30], 0.0, 1, 2, True, [], None, score_from=5)

    def on_step(step):
        if step == 2:
            assert s.abort(1)

    outs, steps = _drive(s, L, buf, {}, on_step=on_step)
    assert outs[1][2] == 2 and outs[1][1] == [] and len(outs[1][10]) == 16  # two steps of 8 rows: the partial records
    assert s.abort(2) is False and s.num_running == 0 and s.num_waiting == 0
    assert s.num_free_blocks + s.num_cached_blocks >= 60


def test_scheduler_steps_without_scoring_rows_are_unchanged():
    """The same generation requests through a scheduler that has served a scoring request and one
    that never saw one write the same words, header included; `total` and `rep_total` stay put."""
    def run(with_score):
        s, L, buf = _sched(prefix_caching=False)
        # the first request takes and returns the same two KV blocks either way, so the block ids
        # of the requests under comparison do not depend on it
        s.add_request(9, list(range(300, 330)), 0.0, 1, 9, True, [], None, score_from=10 if with_score else -1)
        assert _drive(s, L, buf, {})[1][0]["scoring"] == with_score
        s.add_request(1, list(range(100, 120)), 0.0, 6, 1, True, [], None)
        s.add_request(2, list(range(200, 207)), 0.8, 6, 2, True, [], None, logprobs=2)
        return L, _drive(s, L, buf, {})[1]

    (L, plain), (_, after) = run(False), run(True)
    assert len(plain) == len(after) > 3
    for a, b in zip(plain, after):
        assert not a["scoring"] and not b["scoring"] and np.array_equal(a["words"], b["words"])
        assert int(a["words"][L["counts"] + 9]) == 0
    o = (L["bias_val"] + L["bias_cap"] + 3) & ~3
    assert L["total"] == o
    assert L["score_target"] == L["rep_total"] and L["score_total"] == (L["rep_total"] + L["max_seqs"] + 3) & ~3
    assert _runtime.Scheduler.SCORE_RECORD_WORDS == W and _runtime.Scheduler.LOGPROB_RECORD_WORDS == 41
    assert _runtime.Scheduler.COUNTS9_SCORE_BIT == SCORE_BIT and _runtime.Scheduler.FINISH_SCORE == FINISH_SCORE


def test_scheduler_refuses_a_short_buffer_and_bad_requests():
    s, L, buf = _sched()
    s.add_request(1, list(range(100, 110)), 0.0, 2, 1, True, [], None)
    assert s.schedule(buf.ctypes.data) == 10  # no scoring request yet: the old call works
    s.commit(np.full(1, 7, dtype=np.int32).ctypes.data, 1)
    s.add_request(2, list(range(200, 210)), 0.0, 1, 2, True, [], None, score_from=4)
    buf[:] = POISON
    for words in (0, L["total"], L["rep_total"], L["score_total"] - 1):
        with pytest.raises(ValueError, match="score_total"):
            s.schedule(buf.ctypes.data, words)
        assert bool((buf == POISON).all()) and s.num_running == 1 and s.num_waiting == 1  # nothing planned
    assert s.schedule(buf.ctypes.data, buf.size) == 10 and int(buf[L["counts"] + 9]) == SCORE_BIT
    for k in (0, 10, 11, -2):
        with pytest.raises(ValueError, match="score_from"):
            s.add_request(3, list(range(10)), 0.0, 1, 3, True, [], None, score_from=k)
    for kw in ({"embed": True}, {"presence_penalty": 0.5}, {"min_p": 0.1, "ln_min_p": -2.3},
               {"repetition_penalty": 1.2}, {"logit_bias": [(3, 1.0)]}):
        with pytest.raises(ValueError):
            s.add_request(3, list(range(10)), 0.0, 1, 3, True, [], None, score_from=5, **kw)


# ---------------------------------------------------------------------------
# CPU engine
# ---------------------------------------------------------------------------

def _engine(async_steps=False, **kw):
    from pilottai_amd.engine.engine import EngineConfig, LLMEngine

    cfg = dict(model="tiny", max_num_seqs=8, max_num_batched_tokens=128, max_model_len=512, num_kv_blocks=128,
               use_graphs=False, async_steps=async_steps)
    cfg.update(kw)
    return LLMEngine(EngineConfig(**cfg), device="cpu")


@pytest.fixture(scope="module", params=[False, True], ids=["serial", "pipelined"])
def engine(request):
    e = _engine(async_steps=request.param)
    assert e._async == request.param
    yield e
    e.stop()


def _texts(tok):
    ctx = tok.encode("The orchestrator analyses a task and delegates it to the agent that fits best. " * 2)
    cands = [tok.encode(" yes"), tok.encode(" no, the task stays where it is until somebody asks for it again")]
    return ctx, cands


def _spy_on_the_scored_rows(monkeypatch):
    """Record, for every row the engine scores, what the integer rule gives on that very logits row:
    {(target, logprob as the engine reports it): (rank by the literal loop, the row's bf16 bits)}."""
    from pilottai_amd.ops import reference as ref

    seen = {}
    real = ref.score_tokens

    def spy(logits, target, lp_n, top=20):
        out = real(logits, target, lp_n, top)
        bits = logits.detach().to(torch.bfloat16).contiguous().view(torch.int16).numpy()
        for r in range(logits.shape[0]):
            t = int(target[r])
            if t >= 0:
                seen[(t, float(out[0][r]))] = (brute_rank(order_keys(bits[r]), t), bits[r].copy())
        return out

    monkeypatch.setattr(ref, "score_tokens", spy)
    return seen


def _check_run(e, ctx, cands, outs, n, seen):
    """Every record of a run: logprob within 0.1 of log_softmax(model.reference_logits), the
    tolerance tests/test_logprobs.py::test_engine_logprobs_match_the_reference_forward uses for the
    same comparison; rank equal to the integer rule applied to the logits the engine itself scored;
    the record consistent with itself, exactly."""
    for c, o in zip(cands, outs):
        full = ctx + c
        want = torch.log_softmax(e.model.reference_logits(full).float(), dim=-1)
        assert o.finish_reason == "score" and o.token_ids == [] and o.completion_tokens == 0 and o.logprobs is None
        assert o.prompt_tokens == len(full) and len(o.prompt_logprobs) == len(c)
        assert o.cumulative_logprob == sum(rec[0] for rec in o.prompt_logprobs)
        for i, (lp, rank, top) in enumerate(o.prompt_logprobs):
            p = len(ctx) + i
            assert abs(lp - float(want[p - 1, full[p]])) <= 0.1, (p, lp)
            assert rank == seen[(full[p], lp)][0], (p, rank)
            assert len(top) == n
            record_consistent(full[p], lp, rank, [t for t, _ in top] + [-1] * (20 - n),
                              [v for _, v in top] + [-math.inf] * (20 - n), n)


def test_engine_records_match_the_reference_forward_and_the_rank_rule(engine, monkeypatch):
    seen = _spy_on_the_scored_rows(monkeypatch)
    ctx, cands = _texts(engine.tok)
    _check_run(engine, ctx, cands, engine.score(ctx, cands, top=4), 4, seen)


@pytest.mark.parametrize("kw", [{"max_num_seqs": 4}, {"max_num_batched_tokens": 16, "max_num_seqs": 3}],
                         ids=["rows4", "tokens16-rows3"])
def test_engine_chunked_runs_give_the_one_step_records(engine, monkeypatch, kw):
    """A run cut into many steps by a small token or row budget gives the one-step run's records:
    the same positions and targets in the same order, and per position

    * where the two runs scored bit-equal logits rows, the whole record is equal, exactly;
    * elsewhere no logit differs by more than 2 bf16 ulps of the row's largest magnitude, and the
      logprobs differ by no more than those rows allow: |d logprob| <= |d x[t]| + max_i |d x[i]|
      (the log-sum-exp is 1-Lipschitz in the maximum norm), plus 1e-5 for the fp32 outputs; the
      ranks are each the integer rule on the run's own row (_check_run).

    The rows are not always bit-equal because the CPU reference forward rounds differently for
    different step shapes (a 4-row step and a 46-row step take different GEMM paths): every run
    rounds to bf16 after each projection, the two roundings can fall on neighbouring values, and a
    one-ulp step in the hidden state moves every logit by an amount relative to the scale of the
    row's sums, not to the logit itself (small logits are differences of large terms). About half
    of a row's logits move, by 2^-7 at most here (one ulp at the row's scale; 2e-3 in a logprob);
    2 ulps leaves room for one rounding step in the hidden state and one in the LM head."""
    seen = _spy_on_the_scored_rows(monkeypatch)
    ctx, cands = _texts(engine.tok)
    whole = engine.score(ctx, cands, top=2)
    rows_whole = dict(seen)
    seen.clear()
    e = _engine(async_steps=engine._async, prefix_caching=False, **kw)
    try:
        got = e.score(ctx, cands, top=2)
        assert e.stats["steps"] > 3
    finally:
        e.stop()
    _check_run(engine, ctx, cands, whole, 2, rows_whole)
    _check_run(e, ctx, cands, got, 2, seen)
    equal_rows = 0
    for c, a, b in zip(cands, whole, got):
        assert len(a.prompt_logprobs) == len(b.prompt_logprobs) == len(c)
        for t, ra, rb in zip(c, a.prompt_logprobs, b.prompt_logprobs):
            bits_a, bits_b = rows_whole[(t, ra[0])][1], seen[(t, rb[0])][1]  # keyed by the position's target
            if np.array_equal(bits_a, bits_b):
                assert ra == rb, (t, ra, rb)
                equal_rows += 1
                continue
            xa, xb = (torch.from_numpy(x.copy()).view(torch.bfloat16).double().numpy() for x in (bits_a, bits_b))
            dx = np.abs(xa - xb)
            scale = max(np.abs(xa).max(), np.abs(xb).max())
            assert dx.max() <= 2 * 2.0 ** (math.floor(math.log2(scale)) - 7), (dx.max(), scale)  # 2 bf16 ulps there
            assert abs(ra[0] - rb[0]) <= dx[t] + dx.max() + 1e-5, (t, ra[0], rb[0], dx[t], dx.max())
            for (ia, la), (ib, lb) in zip(ra[2], rb[2]):  # the alternatives: the same bound wherever the id agrees
                assert ia != ib or abs(la - lb) <= dx[ia] + dx.max() + 1e-5
    assert equal_rows >= 1  # the first scored position of the long candidate sits in equal-shaped steps


def test_pipelined_loop_gives_the_serial_loop_s_records():
    outs = []
    for a in (False, True):
        e = _engine(async_steps=a, max_num_seqs=4)
        try:
            ctx, cands = _texts(e.tok)
            outs.append(e.score(ctx, cands, top=3))
        finally:
            e.stop()
    for a, b in zip(*outs):
        assert a.prompt_logprobs == b.prompt_logprobs and a.finish_reason == b.finish_reason == "score"


def test_engine_generation_does_not_depend_on_scoring_requests_in_the_batch(engine, monkeypatch):
    tok = engine.tok
    ctx, cands = _texts(tok)
    prompts = [tok.encode(f"request number {i} asks for a plan") for i in range(4)]

    def run(with_scoring):
        res = {}
        for i, p in enumerate(prompts):
            engine.submit(p, lambda o, i=i: res.__setitem__(i, o), temperature=0.8, max_tokens=8, ignore_eos=True,
                          seed=100 + i, logprobs=2 if i == 0 else -1)
        n = len(prompts)
        if with_scoring:
            for j, c in enumerate(cands):
                engine.submit(ctx + c, lambda o, k=n + j: res.__setitem__(k, o), score_from=len(ctx), logprobs=1)
            n += len(cands)
        while len(res) < n:
            assert engine.step() or len(res) == n
        return res

    seen = _spy_on_the_scored_rows(monkeypatch)
    plain, mixed = run(False), run(True)
    for i in range(len(prompts)):
        assert plain[i].token_ids == mixed[i].token_ids and len(mixed[i].token_ids) == 8
        assert mixed[i].prompt_logprobs is None and (mixed[i].logprobs is not None) == (i == 0)
    _check_run(engine, ctx, cands, [mixed[len(prompts) + j] for j in range(len(cands))], 1, seen)


def test_submit_refuses_bad_scoring_requests(engine):
    cb = lambda o: None  # noqa: E731
    ids = [5, 6, 7, 8]
    V = engine.model_cfg.vocab_size
    for k in (0, 4, 5, -1, True, 1.5):
        with pytest.raises(ValueError):
            engine.submit(ids, cb, score_from=k)
    for bad in ([5, V, 7], [5, -1, 7]):
        with pytest.raises(ValueError):
            engine.submit(bad, cb, score_from=1)
    segs = engine.grammar.compile("orchestrator.result_evaluation")
    for kw in ({"embed": True}, {"embed": "last"}, {"grammar": segs}, {"presence_penalty": 0.5},
               {"frequency_penalty": -0.5}, {"logit_bias": {3: 1.0}}, {"min_p": 0.2}, {"repetition_penalty": 1.3},
               {"logprobs": 21}, {"logprobs": -2}):
        with pytest.raises(ValueError):
            engine.submit(ids, cb, score_from=2, **kw)
    with pytest.raises(ValueError):
        engine.score([], [[1, 2]])
    assert engine._inbox.empty()
    # what scoring ignores is accepted
    o = engine.score(ids[:2], [ids[2:]])[0]
    assert o.finish_reason == "score" and len(o.prompt_logprobs) == 2 and o.prompt_logprobs[0][2] == []
    res = []
    engine.submit(ids, res.append, score_from=2, temperature=1.3, top_k=5, top_p=0.5, seed=3, max_tokens=99)
    while not res:
        assert engine.step() or res
    assert res[0].prompt_logprobs == o.prompt_logprobs


def _tp_worker(rank, world, port, out_path):
    import json

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    from pilottai_amd.engine.engine import EngineConfig, LLMEngine
    from pilottai_amd.parallel.comm import init_distributed, new_tp_groups

    init_distributed("gloo")
    e = LLMEngine(EngineConfig(model="tiny-gqa4", max_num_seqs=8, max_num_batched_tokens=128, max_model_len=512,
                               num_kv_blocks=96, use_graphs=False), device="cpu", tp=new_tp_groups(world))
    if rank != 0:
        e.follow()
        torch.distributed.destroy_process_group()
        return
    res = {}
    try:
        e.submit([1, 2, 3], lambda o: None, score_from=1)
        res["refused"] = False
    except ValueError as err:
        res["refused"] = True
        res["message"] = str(err)
    res["tokens"] = len(e.generate([[1, 2, 3]], temperature=0.0, max_tokens=2, ignore_eos=True)[0].token_ids)
    e.release_followers()
    torch.distributed.destroy_process_group()
    with open(out_path, "w") as f:
        json.dump(res, f)


def test_submit_refuses_scoring_on_a_tp_engine(tmp_path):
    import json
    import socket

    import torch.multiprocessing as mp

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / "tp.json")
    mp.start_processes(_tp_worker, args=(2, port, out), nprocs=2, join=True, start_method="spawn")
    res = json.load(open(out))
    assert res["refused"] and "TP" in res["message"] and res["tokens"] == 2


# ---------------------------------------------------------------------------
# LocalLLM, HTTP and clients
# ---------------------------------------------------------------------------

def test_local_llm_score_choose_and_the_http_round_trip():
    import httpx

    from pilottai_amd.core.config import LLMConfig
    from pilottai_amd.engine.http_llm import OpenAICompatLLM
    from pilottai_amd.engine.local_llm import LocalLLM, SchemaLLM, make_llm
    from pilottai_amd.serving.http_server import create_app

    eng = _engine()
    eng.start()
    messages = [{"role": "user", "content": "which agent takes the task?"}]
    options = ["the planner", "the reviewer agent", "nobody"]

    n_tok = [len(eng.tok.encode(o)) for o in options]

    def same(a, b, tokens=None):
        """Two runs of one request that were batched differently (alone, with the other candidates,
        behind a prefix-cache hit). The CPU forward is not bit-stable across step shapes: the two
        runs' bf16 logits differ by at most 2 ulps of the row's largest magnitude (asserted element
        by element in test_engine_chunked_runs_give_the_one_step_records), an ulp is 2^-6 below
        |logit| = 4 (the tiny model's logits stay below 2.5), and a logprob moves by at most the
        target's change plus the largest change in the row: 2 * 2 * 2^-6 = 0.0625 per token; a sum
        over a candidate, that times its number of tokens (`tokens`)."""
        tokens = tokens or [1] * len(a)
        return len(a) == len(b) == len(tokens) and all(abs(x - y) <= 0.0625 * n for x, y, n in zip(a, b, tokens))

    try:
        backend = LocalLLM(LLMConfig(model_name="tiny", max_tokens=96, retry_attempts=1), engine=eng)
        assert backend.supports_scoring and not SchemaLLM.supports_scoring
        direct = asyncio.run(backend.score(messages, options, top=2))
        ctx = backend.context_ids(messages)
        for text, r in zip(options, direct):
            c = eng.tok.encode(text)  # tokenised on its own: the boundary is fixed
            assert [t["token_id"] for t in r["tokens"]] == c and "".join(t["token"] for t in r["tokens"]) == text
            assert r["logprob"] == sum(t["logprob"] for t in r["tokens"])
            assert all(t["rank"] >= 1 and len(t["top_logprobs"]) == 2 for t in r["tokens"])
            assert set(r["tokens"][0]) == {"token", "token_id", "logprob", "rank", "bytes", "top_logprobs"}
            assert set(r) == {"logprob", "tokens"}
            o = eng.score(ctx, [c])[0]  # the same request through the engine's own entry point
            assert same([t["logprob"] for t in r["tokens"]], [e[0] for e in o.prompt_logprobs])
        idx, vals = asyncio.run(backend.choose(messages, options))
        assert same(vals, [r["logprob"] for r in direct], n_tok) and idx == max(range(3), key=lambda i: vals[i])
        idx_n, vals_n = asyncio.run(backend.choose(messages, options, normalize=True))
        assert same(vals_n, [r["logprob"] / len(r["tokens"]) for r in direct])
        assert idx_n == max(range(3), key=lambda i: vals_n[i])
        plain = asyncio.run(backend.score("The task goes to", [" the planner"]))  # plain-text context
        assert len(plain) == 1 and plain[0]["logprob"] < 0
        with pytest.raises(ValueError):
            asyncio.run(backend.score(messages, ["ok", ""]))
        with pytest.raises(ValueError):
            asyncio.run(backend.score(messages, options, top=21))
        with pytest.raises(ValueError):
            asyncio.run(backend.choose(messages, []))

        with Server(create_app(backend, "tiny", engine=eng)) as url:
            post = lambda **kw: httpx.post(f"{url}/score", json=kw, timeout=120)  # noqa: E731
            r = post(context=messages, candidates=options, top_logprobs=2)
            assert r.status_code == 200, r.text
            data = r.json()
            assert data["object"] == "score" and data["model"] == "tiny" and len(data["scores"]) == 3
            assert data["usage"]["completion_tokens"] == 0 and data["usage"]["prompt_tokens"] > 0
            for s, d in zip(data["scores"], direct):
                assert s["logprob"] == sum(t["logprob"] for t in s["tokens"])
                assert [(t["token"], t["token_id"], t["bytes"]) for t in s["tokens"]] == \
                    [(t["token"], t["token_id"], t["bytes"]) for t in d["tokens"]]
                assert same([t["logprob"] for t in s["tokens"]], [t["logprob"] for t in d["tokens"]])
                assert all(len(t["top_logprobs"]) == 2 and t["rank"] >= 1 for t in s["tokens"])
            r0 = post(context="The task goes to", candidates=[" the planner"])  # text context, no alternatives
            assert r0.status_code == 200 and r0.json()["scores"][0]["tokens"][0]["top_logprobs"] == []
            assert same([r0.json()["scores"][0]["logprob"]], [plain[0]["logprob"]], [len(plain[0]["tokens"])])
            for bad in (dict(candidates=options), dict(context="", candidates=options), dict(context=messages),
                        dict(context=messages, candidates=[]), dict(context=messages, candidates="the planner"),
                        dict(context=messages, candidates=["a", ""]), dict(context=messages, candidates=[1]),
                        dict(context=[], candidates=options), dict(context=messages, candidates=options, top_logprobs=21),
                        dict(context=messages, candidates=options, top_logprobs=-1),
                        dict(context=messages, candidates=options, top_logprobs=True)):
                assert post(**bad).status_code == 400, bad

            async def go():
                llm = make_llm(LLMConfig(provider="openai", base_url=url, model_name="tiny", retry_attempts=1,
                                         timeout=120))
                assert llm.supports_scoring
                res = await llm.score(messages, options, top=1)
                pick = await llm.choose(messages, options)
                await llm.aclose()
                return res, pick

            remote, pick = asyncio.run(go())
        assert same([r["logprob"] for r in remote], [r["logprob"] for r in direct], n_tok) and pick[0] == idx
        assert [t["token_id"] for t in remote[1]["tokens"]] == [t["token_id"] for t in direct[1]["tokens"]]
        assert all(t["rank"] >= 1 and len(t["top_logprobs"]) == 1 for r in remote for t in r["tokens"])
    finally:
        eng.stop()
    # backends without scoring say so
    schema = SchemaLLM(seed=1)
    with pytest.raises(NotImplementedError, match="score"):
        asyncio.run(schema.score(messages, options))
    with pytest.raises(NotImplementedError):
        asyncio.run(schema.choose(messages, options))
    other = OpenAICompatLLM(LLMConfig(provider="openai", base_url="http://127.0.0.1:9/v1", model_name="x"),
                            schema_mode="json_object")
    assert not other.supports_scoring
    with pytest.raises(NotImplementedError):
        asyncio.run(other.score(messages, options))
    with Server(create_app(schema, "schema-test")) as url:
        r = httpx.post(f"{url}/score", json={"context": messages, "candidates": options}, timeout=60)
        assert r.status_code == 400 and "score" in r.text


def test_minus_infinity_travels_through_the_endpoint_and_the_client():
    """A candidate with an impossible token: /v1/score sends -inf as -9999.0 (the token, its
    alternatives and the sum), and OpenAICompatLLM.score turns it back into -inf."""
    import httpx

    from pilottai_amd.core.config import LLMConfig
    from pilottai_amd.engine.local_llm import BaseLLM, make_llm
    from pilottai_amd.serving.http_server import create_app

    class Stub(BaseLLM):
        provider = "stub"
        supports_scoring = True

        async def score(self, messages_or_text, candidates, top=0):
            tok = {"token": "a", "token_id": 1, "logprob": -math.inf, "rank": 9, "bytes": [97],
                   "top_logprobs": [{"token": "b", "token_id": 2, "logprob": -0.5, "bytes": [98]},
                                    {"token": "c", "token_id": 3, "logprob": -math.inf, "bytes": [99]}]}
            fine = dict(tok, logprob=-1.5, rank=2)
            return [{"logprob": -math.inf, "tokens": [fine, tok]} for _ in candidates]

    with Server(create_app(Stub(), "stub")) as url:
        r = httpx.post(f"{url}/score", json={"context": "x", "candidates": ["ab"], "top_logprobs": 2}, timeout=60)
        assert r.status_code == 200, r.text
        s = r.json()["scores"][0]
        assert s["logprob"] == -9999.0 and [t["logprob"] for t in s["tokens"]] == [-1.5, -9999.0]
        assert [a["logprob"] for a in s["tokens"][1]["top_logprobs"]] == [-0.5, -9999.0] and s["tokens"][1]["rank"] == 9
        assert r.json()["usage"]["prompt_tokens"] == 0  # a backend that reports no usage

        async def go():
            llm = make_llm(LLMConfig(provider="openai", base_url=url, model_name="stub", retry_attempts=1, timeout=60))
            res = await llm.score("x", ["ab"], top=2)
            await llm.aclose()
            return res

        back = asyncio.run(go())[0]
    assert back["logprob"] == -math.inf and [t["logprob"] for t in back["tokens"]] == [-1.5, -math.inf]
    assert [a["logprob"] for a in back["tokens"][1]["top_logprobs"]] == [-0.5, -math.inf]
    assert back["tokens"][1]["rank"] == 9 and set(back) == {"logprob", "tokens"}
