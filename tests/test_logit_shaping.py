"""logit_bias and min_p, CPU tier: the reference ops on hand-worked rows, the scheduler's step
buffer regions row by row (serial and pipelined planning, chunked prefill, forced runs, preemption,
abort), the tiny CPU engine in both loops, the refusals, and the HTTP / client surfaces."""
import asyncio
import json
import math
import os
import socket
import sys
import threading
import time
from collections import deque

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from logprob_checks import consistent  # noqa: E402
from shaping_checks import forbidden_id, minp_bound, minp_gaps, teacher_forced_bias  # noqa: E402

from pilottai_amd import _runtime  # noqa: E402

i32 = lambda x: torch.tensor(x, dtype=torch.int32)  # noqa: E731
f32 = lambda x: torch.tensor(x, dtype=torch.float32)  # noqa: E731


def bf16_bits(x):
    return x.to(torch.bfloat16).view(torch.int16).tolist()


# ---------------------------------------------------------------------------
# reference ops, hand-worked rows
# ---------------------------------------------------------------------------

def test_reference_bias_rounds_once_to_nearest_even_and_touches_nothing_else():
    from pilottai_amd import ops

    assert ops.LOGIT_BIAS_MAX == 300
    V = 12
    # bf16 has 8 significant bits: the spacing in [1, 2) is 2^-7, so +2^-8 lands exactly between
    # two values. 1.0 = 0x3F80 (even) stays; 1.0078125 = 0x3F81 (odd) goes up to 0x3F82.
    row = [1.0, 1.0078125, -3.0, 0.5, 2.0, 7.0, 1.0, 0.0, -1.0, 4.0, 9.0, 1.0078125]
    logits = torch.tensor([row, row, row], dtype=torch.bfloat16)
    half = 2.0 ** -8
    #         row 0: ties + an ordinary add + ids outside [0, V);  row 1: forced;  row 2: no list
    tok = i32([0, 1, 4, -1, V, 11, 0, 1, 5])
    val = f32([half, half, -100.0, 50.0, 50.0, -half, 9.0, 9.0, 9.0])
    out = logits.clone()
    ops.apply_logit_bias(out, i32([0, 6, 9]), i32([6, 2, 0]), tok, val, i32([-1, 3, -1]))
    want0 = list(row)
    want0[0], want0[1], want0[4], want0[11] = 1.0, 1.015625, -98.0, 1.0
    assert out[0].float().tolist() == want0
    assert bf16_bits(out[0])[:2] == [0x3F80, 0x3F82] and bf16_bits(out[0])[11] == 0x3F80  # 0x3F81 - 2^-8: even, down
    assert torch.equal(out[1:].view(torch.int16), logits[1:].view(torch.int16))  # forced row, empty list
    # a list that leaves the region is not applied
    out = logits.clone()
    ops.apply_logit_bias(out, i32([7, 0, 0]), i32([3, 0, 0]), tok, val, i32([-1, -1, -1]))
    assert torch.equal(out.view(torch.int16), logits.view(torch.int16))


def _masks(V, *allowed_sets):
    from pilottai_amd.ops.reference import pack_mask

    rows = []
    for a in allowed_sets:
        m = np.zeros(V, dtype=bool)
        m[list(a)] = True
        rows.append(pack_mask(m).numpy())
    return torch.from_numpy(np.stack(rows))


def test_reference_min_p_hand_worked_rows():
    from pilottai_amd import ops
    from pilottai_amd.ops import reference as ref

    V = 40
    L3 = ref.ln_min_p(0.3)
    assert L3 == float(np.float32(math.log(0.3))) and ref.ln_min_p(1.0) == 0.0 and ref.ln_min_p(0.0) == 0.0
    base = torch.linspace(-4, 3.75, V).to(torch.bfloat16)  # exact in bf16, maximum 3.75 at id 39
    lg = base.repeat(8, 1)
    lg[1, 7] = 3.75                                          # row 1: a second maximum
    masks = _masks(V, range(0, 30), [], range(V))            # class 0 excludes the maximum, class 1 allows nothing
    #          free  p=1  masked  T=0  forced  nothing  off   free(+tau)
    mc = i32([-1,   2,   0,      -1,  -1,     1,       -1,   -1])
    T = f32([1.5,  0.7, 1.5,    0.0, 1.5,    1.5,     1.5,  2.0])
    p = f32([0.3,  1.0, 0.3,    0.3, 0.3,    0.3,     0.0,  0.3])
    Lp = f32([ref.ln_min_p(float(x)) for x in p])
    forced = i32([-1, -1, -1, -1, 5, -1, -1, -1])
    tau = ops.minp_threshold(lg, T, p, Lp, forced, mc, masks)
    inf = float("-inf")
    t0 = np.float32(np.float32(3.75) + np.float32(np.float32(1.5) * np.float32(L3)))
    assert float(tau[0]) == float(t0) and abs(float(t0) - (3.75 + 1.5 * math.log(0.3))) < 1e-6
    assert float(tau[1]) == 3.75                              # p = 1: tau_mp = m, the ties of the maximum stay
    assert set(torch.nonzero(lg[1].float() >= tau[1]).flatten().tolist()) == {7, 39}
    m2 = float(lg[2, 29])                                     # the largest ALLOWED logit; 3.75 is masked
    assert float(tau[2]) == float(np.float32(np.float32(m2) + np.float32(np.float32(1.5) * np.float32(L3))))
    assert tau[3:7].tolist() == [inf] * 4                     # T = 0, forced, nothing allowed, min_p off
    t7 = float(np.float32(np.float32(3.75) + np.float32(np.float32(2.0) * np.float32(L3))))
    assert float(tau[7]) == t7
    # behind a top-k / top-p pass the larger threshold wins, untouched rows keep theirs
    tin = f32([3.5, -1.0, inf, 2.5, 2.5, 2.5, inf, 0.0])
    tau2 = tin.clone()
    assert ops.minp_threshold(lg, T, p, Lp, forced, mc, masks, tau=tau2) is tau2
    assert tau2.tolist() == [3.5, 3.75, float(tau[2]), 2.5, 2.5, 2.5, inf, t7]
    # the sampler under tau never leaves the kept set (greedy rows ignore nothing: tau is -inf there)
    seeds = torch.arange(8, dtype=torch.int64) + 5
    for off in range(20):
        toks = ops.sample(lg, T, mc, masks, seeds, i32([off] * 8), forced, tau=tau).tolist()
        assert float(lg[0, toks[0]]) >= float(tau[0]) and toks[1] in (7, 39) and toks[2] < 30
        assert float(lg[2, toks[2]]) >= float(tau[2]) and toks[3] == 39 and toks[4] == 5


# ---------------------------------------------------------------------------
# scheduler: the step buffer regions
# ---------------------------------------------------------------------------

LIT, STR = 0, 2
POISON = 0x5a5a5a5a


def _lit(toks):
    return (LIT, list(toks), -1, -1, -1, -1, 0, 1, 1)


def _str(end, n):
    return (STR, [], -1, -1, end, -1, n, 1, 1)


def _segs():
    """30 forced tokens (jump-forwarded into the prompt), then free strings between forced runs."""
    return [_lit(range(5000, 5030)), _str(9001, 5), _lit([6000, 6001, 6000]), _str(9002, 4), _lit([7001])]


def _sched(**kw):
    cfg = {"num_blocks": 64, "block_size": 16, "max_num_seqs": 8, "max_num_batched_tokens": 128,
           "max_model_len": 512, "prefix_caching": False, "eos_ids": [128009]}
    cfg.update(kw)
    s = _runtime.Scheduler(cfg)
    L = s.layout()
    return s, L, np.zeros(L["total"], dtype=np.int32)


class _Run:
    """Drives a scheduler with a host sampler, serially (depth 1) or with one step in flight
    (depth 2, the pipelined loop's planning), and compares the shaping regions of every step
    with the requests, row by row."""

    def __init__(self, s, L, depth=1):
        self.s, self.L, self.depth = s, L, depth
        self.bufs = [np.zeros(L["total"], dtype=np.int32) for _ in range(depth)]
        self.req = {}      # rid -> (sorted bias list, min_p, ln_min_p)
        self.rows = {}     # rid -> sampling rows seen, forced rows among them
        self.outs = {}
        self.shaped_steps = self.plain_steps = 0

    def add(self, rid, prompt, max_tokens, segs=None, bias=(), min_p=0.0, temperature=0.8, **kw):
        from pilottai_amd.ops.reference import ln_min_p

        lnp = ln_min_p(min_p)
        self.req[rid] = (sorted((int(t), float(np.float32(b))) for t, b in bias), float(np.float32(min_p)), lnp)
        self.rows[rid] = [0, 0]
        self.s.add_request(rid, prompt, temperature, max_tokens, rid, segs is None, [], segs,
                           logit_bias=list(bias), min_p=min_p, ln_min_p=lnp, **kw)

    def check(self, buf):
        L = self.L
        ms = L["max_seqs"]
        c = buf[L["counts"]:L["counts"] + 12]
        nsamp, flag = int(c[2]), int(c[11])
        seeds = buf[L["seeds"]:L["seeds"] + 2 * ms].view(np.int64)
        forced = buf[L["forced"]:L["forced"] + ms]
        rids = [int(seeds[r]) for r in range(nsamp)]
        want_flag = any(self.req[rid][0] or self.req[rid][1] > 0 for rid in rids)
        if not want_flag:
            assert flag == 0
            assert bool((buf[L["bias_start"]:] == POISON).all())  # nothing behind the penalty regions is written
            self.plain_steps += 1
            return nsamp, forced
        self.shaped_steps += 1
        start, n = buf[L["bias_start"]:L["bias_start"] + ms], buf[L["bias_n"]:L["bias_n"] + ms]
        minp = buf[L["minp"]:L["minp"] + ms].view(np.float32)
        lnp = buf[L["ln_minp"]:L["ln_minp"] + ms].view(np.float32)
        tok = buf[L["bias_tok"]:L["bias_tok"] + L["bias_cap"]]
        val = buf[L["bias_val"]:L["bias_val"] + L["bias_cap"]].view(np.float32)
        end = 0
        for r, rid in enumerate(rids):
            bias, mp_, ln_ = self.req[rid]
            assert int(start[r]) == end and int(n[r]) == len(bias), (r, rid)  # packed, in row order
            assert list(zip(tok[end:end + len(bias)].tolist(), val[end:end + len(bias)].tolist())) == bias
            assert float(minp[r]) == mp_ and float(lnp[r]) == np.float32(ln_), (r, rid)
            end += len(bias)
            self.rows[rid][0] += 1
            self.rows[rid][1] += int(forced[r] >= 0)
        assert flag == 1 + end and end <= L["bias_cap"]
        assert bool((n[nsamp:] == 0).all()) and bool((minp[nsamp:] == 0).all())  # padding rows: nothing to do
        assert bool((buf[L["bias_tok"] + end:L["bias_val"]] == POISON).all())    # only the words in use are written
        return nsamp, forced

    def run(self, pick, on_step=None, max_steps=3000):
        s, pending = self.s, deque()
        for step in range(max_steps):
            buf = self.bufs[step % self.depth]
            buf[self.L["bias_start"]:] = POISON
            T = s.schedule(buf.ctypes.data)
            if T:
                nsamp, forced = self.check(buf)
                sampled = np.array([int(forced[r]) if forced[r] >= 0 else pick(step, r) for r in range(nsamp)] or [0],
                                   dtype=np.int32)
                pending.append((sampled, nsamp))
                if on_step is not None:
                    on_step(step)
            if pending and (len(pending) == self.depth or not T):
                arr, n = pending.popleft()
                for o in s.commit(arr.ctypes.data, n):
                    self.outs[o[0]] = o
            elif not T:
                break
        return self.outs


def _pick(step, r):
    return (40 + step % 3) if step % 5 else 9001 + step % 3


BIAS_A = [(7, -100.0), (3, 2.5), (128255, 100.0)]
BIAS_300 = [(1000 + 3 * i, -99.75 + i / 2) for i in range(300)]  # 300 non-zero values


@pytest.mark.parametrize("depth", [1, 2], ids=["serial", "pipelined"])
def test_scheduler_regions_across_chunks_forced_runs_and_mixed_rows(depth):
    """16-token chunks of 20..60-token prompts, a grammar with a forced prefix and forced runs, shaped
    rows next to plain ones; every sampling row of a shaped request carries its list and min_p."""
    s, L, _ = _sched(max_num_batched_tokens=16)
    assert L["bias_cap"] == 8 * 300
    run = _Run(s, L, depth)
    run.add(1, list(range(100, 130)), 40, _segs(), bias=BIAS_A, min_p=0.3)
    run.add(2, list(range(200, 221)), 40, _segs())                          # plain, same grammar
    run.add(3, list(range(300, 309)), 12, None, min_p=1.0)                  # min_p alone
    run.add(4, list(range(400, 420)), 10, None, bias=BIAS_300)              # a full list alone
    # the raw entry point drops what submit() refuses: a negative id, NaN, zero, an id's second entry
    run.add(5, list(range(500, 505)), 6, None, bias=[(9, 4.0), (9, 5.0), (-2, 1.0), (11, float("nan")), (12, 0.0)])
    run.req[5] = ([(9, 4.0)], 0.0, 0.0)
    run.add(6, list(range(600, 607)), 6, None, bias=[(12, 0.0)], min_p=1.5)  # nothing valid is left: plain
    run.req[6] = ([], 0.0, 0.0)
    outs = run.run(_pick)
    assert set(outs) == {1, 2, 3, 4, 5, 6}
    assert run.rows[3][0] == 12 and run.rows[4][0] == 10 and run.rows[1][0] >= 3
    assert run.shaped_steps >= 12 and run.plain_steps >= 1
    if depth == 2:
        assert s.spec_rows > 0                      # speculative rows were planned, and checked like the others


def test_scheduler_regions_after_preemption_and_abort():
    s, L, _ = _sched(num_blocks=10, max_num_seqs=4, max_num_batched_tokens=256, max_model_len=256)
    run = _Run(s, L)
    run.add(1, list(range(40)), 44, None, bias=BIAS_A)
    run.add(2, list(range(1000, 1040)), 44, None, bias=BIAS_300[:17], min_p=0.05)
    outs = run.run(lambda step, r: 2000 + (step * 7 + r) % 5)
    assert s.total_preemptions >= 1
    assert len(outs[1][1]) == 44 and len(outs[2][1]) == 44
    assert run.rows[1][0] >= 44 and run.rows[2][0] >= 44  # a resumed request's rows carry them again
    # abort: the shaped request leaves, the steps of the plain one are unflagged again
    run.add(3, list(range(300, 310)), 50, None, bias=BIAS_A, min_p=0.5)
    run.add(4, list(range(400, 410)), 8, None)
    seen = run.shaped_steps
    aborted = []

    def on_step(step):
        if run.rows[3][0] >= 3 and not aborted:
            aborted.append(s.abort(3))

    outs = run.run(lambda step, r: 50 + step % 2, on_step=on_step)
    assert aborted == [True] and 4 in outs and 3 not in outs
    assert run.shaped_steps - seen == 3 and {o[0] for o in s.drain_aborted()} == {3}


def test_scheduler_layout_and_unshaped_steps_are_the_parents():
    s, L, buf = _sched()
    # the new regions lie behind every region the parent layout has, 4-word aligned, in this order
    ms = L["max_seqs"]
    o = (L["pair_tok"] + L["pair_cap"] + 3) & ~3
    for name, n in (("bias_start", ms), ("bias_n", ms), ("minp", ms), ("ln_minp", ms), ("bias_tok", ms * 300),
                    ("bias_val", ms * 300)):
        assert L[name] == o, name
        o = (o + n + 3) & ~3
    assert L["total"] == o and L["bias_cap"] == ms * 300

    def drive(sched, b, extra):
        sched.add_request(1, list(range(100, 120)), 0.0, 3, 7, True, [], None)                      # 8 arguments
        sched.add_request(2, list(range(200, 220)), 0.8, 3, 8, True, [], None, 5, 0.9)              # top-k / top-p
        sched.add_request(3, list(range(300, 320)), 0.8, 3, 9, True, [], None, 0, 1.0, False, False, 2, 0.5, 0.5,
                          *extra)                                                                   # penalised
        snaps = []
        for step in range(20):
            b[L["bias_start"]:] = POISON
            if sched.schedule(b.ctypes.data) == 0:
                break
            assert int(b[L["counts"] + 11]) == 0
            assert bool((b[L["bias_start"]:] == POISON).all())
            snaps.append(b[:L["bias_start"]].copy())
            n = int(b[L["counts"] + 2])
            sampled = np.full(max(1, n), 7, dtype=np.int32)
            sched.commit(sampled.ctypes.data, n)
        return snaps

    a = drive(s, buf, ())
    s2, _, buf2 = _sched()
    b = drive(s2, buf2, ([], 0.0, 0.0))  # explicit empty shaping: the same request
    s3, _, buf3 = _sched()
    c = drive(s3, buf3, ([(5, 0.0)], 0.0, -1.2))  # a zero entry and a stray ln: still the same request
    assert len(a) == len(b) == len(c) >= 3
    assert all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in zip(a, b, c))
    # an embedding request never carries shaping
    s4, L4, buf4 = _sched()
    s4.add_request(1, list(range(30)), 0.0, 1, 1, True, [], None, embed=True, logit_bias=[(3, 5.0)], min_p=0.5,
                   ln_min_p=-0.69)
    assert s4.schedule(buf4.ctypes.data) == 30 and int(buf4[L4["counts"] + 11]) == 0


# ---------------------------------------------------------------------------
# CPU engine
# ---------------------------------------------------------------------------

def _engine(**kw):
    from pilottai_amd.engine.engine import EngineConfig, LLMEngine

    cfg = dict(model="tiny", max_num_seqs=8, max_num_batched_tokens=128, max_model_len=512, num_kv_blocks=128,
               use_graphs=False)
    cfg.update(kw)
    return LLMEngine(EngineConfig(**cfg), device="cpu")


@pytest.fixture(scope="module")
def engine():
    e = _engine(max_num_seqs=16)
    yield e
    e.stop()


def _prompts(tok):
    return [tok.encode("The orchestrator analyses a task and delegates it"), tok.encode("evaluate this result please")]


@pytest.mark.parametrize("mode", ["greedy", "t0.8", "grammar"])
def test_engine_empty_shaping_is_the_plain_request(mode):
    e = _engine()
    try:
        shaped_steps = []
        run = e._run
        e._run = lambda *a, **k: (shaped_steps.append(k.get("shape", a[7] if len(a) > 7 else False)), run(*a, **k))[1]
        segs = e.grammar.compile("orchestrator.result_evaluation") if mode == "grammar" else None
        kw = dict(temperature=0.0 if mode == "greedy" else 0.8, max_tokens=200 if segs else 8,
                  ignore_eos=segs is None, seed=4321, grammar=segs)
        plain = e.generate(_prompts(e.tok), **kw)
        empty = e.generate(_prompts(e.tok), logit_bias={}, min_p=0, **kw)
        zeros = e.generate(_prompts(e.tok), logit_bias={11: 0, 12: 0.0}, min_p=0.0, **kw)
        none = e.generate(_prompts(e.tok), logit_bias=None, min_p=None, **kw)
        assert [o.token_ids for o in plain] == [o.token_ids for o in empty] == [o.token_ids for o in zeros] \
            == [o.token_ids for o in none]
        assert shaped_steps and not any(shaped_steps) and all(len(k) < 6 for k in e._graphs)
        assert int(e._host_np[e.L["counts"] + 11]) == 0
    finally:
        e.stop()


def test_engine_bias_forces_bans_and_respects_the_grammar(engine):
    p = _prompts(engine.tok)
    kw = dict(temperature=0.8, max_tokens=12, ignore_eos=True, seed=77)
    plain = engine.generate(p, **kw)
    # +100 on one id in free text: every sampled token is that id
    for o in engine.generate(p, logit_bias={4242: 100}, **kw):
        assert o.token_ids == [4242] * 12
    # -100 on a set of ids: none appears (here: every id the plain replies used)
    banned = {t for o in plain for t in o.token_ids}
    outs = engine.generate(p, logit_bias={t: -100 for t in banned}, **kw)
    assert all(len(o.token_ids) == 12 and not set(o.token_ids) & banned for o in outs)
    # the same +100 under a grammar that forbids the id: it never appears and the reply parses
    segs = engine.grammar.compile("orchestrator.result_evaluation")
    bad = forbidden_id(engine)
    gkw = dict(temperature=0.8, max_tokens=200, seed=5, grammar=segs)
    plain_g = engine.generate(p, **gkw)
    shaped_g = engine.generate(p, logit_bias={bad: 100}, min_p=0.05, **gkw)
    for a, b in zip(plain_g, shaped_g):
        assert b.finish_reason == "stop" and bad not in b.token_ids and bad not in a.token_ids
        json.loads(b.text)
    # greedy teacher forcing: the biased reference's argmax, token by token
    g = dict(temperature=0.0, max_tokens=16, ignore_eos=True)
    greedy = engine.generate(p[:1], **g)[0].token_ids
    bias = {t: -100 for t in set(greedy)}
    out = engine.generate(p[:1], logit_bias=bias, **g)[0].token_ids
    assert not set(out) & set(greedy)
    teacher_forced_bias(engine, p[0], out, bias)


def test_engine_min_p_bounds_the_gap_to_the_maximum(engine):
    p = _prompts(engine.tok)[0]
    T, mp_ = 1.5, 0.3
    bound, worst_plain = minp_bound(T, mp_), 0.0
    for seed in (11, 12, 13):
        kw = dict(temperature=T, max_tokens=12, ignore_eos=True, seed=seed)
        out = engine.generate([p], min_p=mp_, **kw)[0].token_ids
        gaps = minp_gaps(engine, p, out)
        assert len(out) == 12 and all(g <= bound for g in gaps), (seed, gaps)
        worst_plain = max(worst_plain, max(minp_gaps(engine, p, engine.generate([p], **kw)[0].token_ids)))
    assert worst_plain > bound  # the same seeds leave the min_p set without it
    # T = 0: min_p has no effect
    g = dict(temperature=0.0, max_tokens=12, ignore_eos=True)
    assert engine.generate([p], min_p=0.9, **g)[0].token_ids == engine.generate([p], **g)[0].token_ids
    # with top-k: the intersection (never outside either set)
    out = engine.generate([p], min_p=mp_, top_k=3, temperature=T, max_tokens=12, ignore_eos=True, seed=11)[0].token_ids
    assert all(g_ <= bound for g_ in minp_gaps(engine, p, out))


def _shaped_kw(i):
    return dict(temperature=0.9, max_tokens=20, logit_bias={3000 + i: 100, 4242: -100} if i % 2 else {4242: -50.5},
                min_p=0.0 if i == 1 else 0.2)


def test_engine_shaped_request_alone_and_among_fifteen(engine):
    tok = engine.tok
    prompts = [_prompts(tok)[0]] + [tok.encode(f"request number {i} asks for a plan") for i in range(1, 16)]

    def run(which):
        res = {}
        for i in which:
            kw = _shaped_kw(0) if i == 0 else (_shaped_kw(i) if i < 4 else dict(temperature=0.8, max_tokens=16))
            if i == 5:
                kw.update(presence_penalty=1.0)
            engine.submit(prompts[i], lambda o, i=i: res.__setitem__(i, o), ignore_eos=True, seed=100 + i, **kw)
        while len(res) < len(which):
            assert engine.step() or len(res) == len(which)
        return res

    alone, mixed = run([0]), run(range(16))
    assert alone[0].token_ids == mixed[0].token_ids and len(alone[0].token_ids) == 20
    plain = engine.generate([prompts[0]], temperature=0.9, max_tokens=20, ignore_eos=True, seed=100)[0]
    assert plain.token_ids != alone[0].token_ids  # the shaping was at work
    assert mixed[1].token_ids == [3001] * 20 and mixed[3].token_ids == [3003] * 20


def test_engine_pipelined_loop_matches_the_serial_loop(engine):
    tok = engine.tok
    segs_name = "orchestrator.result_evaluation"
    prompts = _prompts(tok) + [tok.encode("a third request of another length altogether")]
    e = _engine(async_steps=True, max_num_seqs=16)
    try:
        outs = []
        for eng in (engine, e):
            segs = eng.grammar.compile(segs_name)
            free = eng.generate(prompts, temperature=0.9, max_tokens=24, ignore_eos=True, seed=31,
                                logit_bias={4242: -100, 17: 3.5}, min_p=0.2, logprobs=2)
            gram = eng.generate(prompts[:2], temperature=0.8, max_tokens=200, seed=32, grammar=segs,
                                logit_bias={tok.token_id('"'): -2.0}, min_p=0.1)
            outs.append(([o.token_ids for o in free], [o.token_ids for o in gram]))
            assert all(o.finish_reason == "stop" for o in gram)
        assert outs[0] == outs[1]
        assert e.sched.spec_rows > 0  # the pipelined engine did plan speculative shaped rows
    finally:
        e.stop()


def test_engine_bias_with_logprobs(engine):
    p = _prompts(engine.tok)
    for o in engine.generate(p, temperature=0.8, max_tokens=8, ignore_eos=True, seed=3, logprobs=2, min_p=0.2,
                             logit_bias={4242: 100}):
        consistent(engine, o, 2)
        assert o.token_ids == [4242] * 8
        assert all(lp > -1e-3 and top[0][0] == 4242 for lp, top in o.logprobs)  # on the biased logits
    plain = engine.generate(p[:1], temperature=0.0, max_tokens=12, ignore_eos=True, logprobs=3)[0]
    banned = {i for _, top in plain.logprobs for i, _ in top}
    o = engine.generate(p[:1], temperature=0.0, max_tokens=12, ignore_eos=True, logprobs=3,
                        logit_bias={t: -100 for t in banned})[0]
    consistent(engine, o, 3, greedy=True)
    assert not {i for _, top in o.logprobs for i, _ in top} & banned
    # min_p does not enter the logprobs: the same tokens and the same records as top-k / top-p ignore it
    a = engine.generate(p[:1], temperature=0.0, max_tokens=6, ignore_eos=True, logprobs=3)[0]
    b = engine.generate(p[:1], temperature=0.0, max_tokens=6, ignore_eos=True, logprobs=3, min_p=0.5)[0]
    assert a.token_ids == b.token_ids and a.logprobs == b.logprobs
    segs = engine.grammar.compile("orchestrator.result_evaluation")
    for o in engine.generate(p, temperature=0.0, max_tokens=200, grammar=segs, logprobs=3, min_p=0.3,
                             logit_bias={engine.tok.token_id('"'): -1.5}):
        assert o.finish_reason == "stop"
        json.loads(o.text)
        consistent(engine, o, 3, greedy=True, segs=segs)


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------

def test_submit_refuses_bad_shaping(engine):
    cb = lambda o: None  # noqa: E731
    V = engine.model_cfg.vocab_size
    bad_bias = [{i: 1.0 for i in range(301)}, {V: 1.0}, {-1: 1.0}, {5: math.nan}, {5: math.inf}, {5: -math.inf},
                {5: 100.5}, {5: -101}, {5: True}, {5: "1"}, {"5": 1.0}, {2.0: 1.0}, {True: 1.0}, [(5, 1.0)], "x"]
    for bad in bad_bias:
        with pytest.raises(ValueError):
            engine.submit([1, 2, 3], cb, logit_bias=bad)
    for bad in (-0.1, 1.01, math.nan, math.inf, "0.5", True):
        with pytest.raises(ValueError):
            engine.submit([1, 2, 3], cb, min_p=bad)
    for emb in (True, "last"):
        with pytest.raises(ValueError, match="embedding"):
            engine.submit([1, 2, 3], cb, embed=emb, logit_bias={5: 1.0})
        with pytest.raises(ValueError, match="embedding"):
            engine.submit([1, 2, 3], cb, embed=emb, min_p=0.5)
    assert engine._inbox.empty()
    # the edges are accepted: 300 entries, ids 0 and V - 1, values +-100, min_p 1
    o = engine.generate([[1, 2, 3]], temperature=0.7, max_tokens=2, ignore_eos=True, min_p=1,
                        logit_bias={**{i: -100 for i in range(1, 299)}, 0: 100, V - 1: -100.0})[0]
    assert o.token_ids == [0, 0]


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _tp_worker(rank, world, port, out_path):
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
    res = {"messages": []}
    for kw in (dict(logit_bias={5: 1.0}), dict(min_p=0.5)):
        try:
            e.submit([1, 2, 3], lambda o: None, **kw)
            res["messages"].append(None)
        except ValueError as err:
            res["messages"].append(str(err))
    o = e.generate([[1, 2, 3]], temperature=0.0, max_tokens=2, ignore_eos=True, logit_bias={}, min_p=0.0)[0]
    res["tokens"] = len(o.token_ids)
    e.release_followers()
    torch.distributed.destroy_process_group()
    with open(out_path, "w") as f:
        json.dump(res, f)


def test_submit_refuses_shaping_on_a_tp_engine(tmp_path):
    out = str(tmp_path / "tp.json")
    mp.start_processes(_tp_worker, args=(2, _free_port(), out), nprocs=2, join=True, start_method="spawn")
    res = json.load(open(out))
    assert all(m is not None and "TP" in m for m in res["messages"]) and res["tokens"] == 2


# ---------------------------------------------------------------------------
# HTTP and clients
# ---------------------------------------------------------------------------

class _Server:
    def __init__(self, app):
        import uvicorn

        self.port = _free_port()
        self.server = uvicorn.Server(uvicorn.Config(app, host="127.0.0.1", port=self.port, log_level="error"))
        self.thread = threading.Thread(target=self.server.run, daemon=True)

    def __enter__(self):
        self.thread.start()
        t0 = time.time()
        while not self.server.started:
            assert time.time() - t0 < 30, "server did not start"
            time.sleep(0.02)
        return f"http://127.0.0.1:{self.port}/v1"

    def __exit__(self, *exc):
        self.server.should_exit = True
        self.thread.join(timeout=10)


def test_http_shaping_validation_backends_and_client():
    import httpx

    from pilottai_amd.core.config import LLMConfig
    from pilottai_amd.engine.http_llm import OpenAICompatLLM
    from pilottai_amd.engine.local_llm import LocalLLM, SchemaLLM
    from pilottai_amd.serving.http_server import create_app

    eng = _engine()
    eng.start()
    try:
        V = eng.model_cfg.vocab_size
        backend = LocalLLM(LLMConfig(model_name="tiny", max_tokens=16, retry_attempts=1), engine=eng)
        assert backend.supports_logit_shaping and backend.min_p == 0.0 and not SchemaLLM.supports_logit_shaping
        body = {"messages": [{"role": "user", "content": "task 1"}], "temperature": 0.9, "seed": 3, "max_tokens": 16,
                "logprobs": True}
        ids = lambda r: [e["token_id"] for e in r.json()["choices"][0]["logprobs"]["content"]]  # noqa: E731
        with _Server(create_app(backend, "tiny", engine=eng)) as url:
            post = lambda **kw: httpx.post(f"{url}/chat/completions", json=dict(body, **kw), timeout=120)  # noqa: E731
            plain = post()
            assert plain.status_code == 200, plain.text
            empty = post(logit_bias={}, min_p=0)
            assert empty.status_code == 200 and ids(empty) == ids(plain)
            both = post(logit_bias={str(t): -100 for t in set(ids(plain))}, min_p=0.1)
            assert both.status_code == 200, both.text
            assert len(ids(both)) == 16 and not set(ids(both)) & set(ids(plain))
            forced = post(logit_bias={"4242": 100, " 17 ": 0})
            assert forced.status_code == 200 and ids(forced) == [4242] * 16
            only_mp = post(min_p=1.0)
            assert only_mp.status_code == 200 and ids(only_mp) != ids(plain)
            for bad in (dict(logit_bias=[1, 2]), dict(logit_bias="7"), dict(logit_bias={"x": 1}), dict(logit_bias={"1.5": 1}),
                        dict(logit_bias={"7": 101}), dict(logit_bias={"7": "1"}), dict(logit_bias={"7": True}),
                        dict(logit_bias={"7": None}), dict(logit_bias={"-1": 1}), dict(logit_bias={str(V): 1}),
                        dict(logit_bias={"7": 1, "07": 2}), dict(logit_bias={str(i): 1 for i in range(301)}),
                        dict(min_p=1.5), dict(min_p=-0.1), dict(min_p="0.5"), dict(min_p=True)):
                r = post(**bad)
                assert r.status_code == 400 and ("logit_bias" in r.text or "min_p" in r.text), (bad, r.text)

            sent = []

            class _Spy(OpenAICompatLLM):
                def _body(self, *args):
                    sent.append(super()._body(*args))
                    return sent[-1]

            async def go():
                llm = _Spy(LLMConfig(provider="openai", base_url=url, model_name="tiny", retry_attempts=1,
                                     timeout=120, max_tokens=16, temperature=0.9, min_p=0.1))
                assert llm.supports_logit_shaping
                a = await llm.generate_response([{"role": "user", "content": "task 1"}],
                                                response_format={"seed": 3, "logprobs": 0,
                                                                 "logit_bias": {t: -100 for t in set(ids(plain))}})
                b = await llm.generate_response([{"role": "user", "content": "task 1"}],
                                                response_format={"seed": 3, "logprobs": 0, "min_p": 0})
                await llm.aclose()
                return a, b

            a, b = asyncio.run(go())
        assert sent[0]["min_p"] == 0.1 and sent[0]["logit_bias"] == {str(t): -100.0 for t in set(ids(plain))}
        assert "min_p" not in sent[1] and "logit_bias" not in sent[1]  # nothing stays off the wire
        assert [e["token_id"] for e in a["logprobs"]] == ids(both) and [e["token_id"] for e in b["logprobs"]] == ids(plain)
        # LLMConfig.min_p is the default in process as well; the request's value overrides it
        local = LocalLLM(LLMConfig(model_name="tiny", max_tokens=16, retry_attempts=1, temperature=0.9, min_p=1.0),
                         engine=eng)
        msg = [{"role": "user", "content": "task 1"}]
        r = asyncio.run(local.generate_response(msg, response_format={"seed": 3, "logprobs": 0}))
        assert [e["token_id"] for e in r["logprobs"]] == ids(only_mp)
        r = asyncio.run(local.generate_response(msg, response_format={"seed": 3, "logprobs": 0, "min_p": 0.0}))
        assert [e["token_id"] for e in r["logprobs"]] == ids(plain)
        with pytest.raises(Exception):
            LLMConfig(model_name="tiny", min_p=1.5)
    finally:
        eng.stop()
    # the model-free backend refuses shaping and accepts its absence
    schema = SchemaLLM(seed=1)
    sbody = {"messages": [{"role": "user", "content": "x"}],
             "response_format": {"type": "pilottai_schema", "schema": "orchestrator.result_evaluation"}}
    with _Server(create_app(schema, "schema-test")) as url:
        r = httpx.post(f"{url}/chat/completions", json=dict(sbody, logit_bias={"5": -100}), timeout=60)
        assert r.status_code == 400 and "logit_bias" in r.text
        r = httpx.post(f"{url}/chat/completions", json=dict(sbody, min_p=0.2), timeout=60)
        assert r.status_code == 400 and "min_p" in r.text
        assert httpx.post(f"{url}/chat/completions", json=dict(sbody, logit_bias={}, min_p=0), timeout=60).status_code == 200
        assert httpx.post(f"{url}/chat/completions", json=dict(sbody, min_p=7), timeout=60).status_code == 400
