"""Presence / frequency penalties, CPU tier: the reference op, the scheduler's slot and delta
plumbing against a Python model of the device state, the tiny CPU engine, the refusals, and the
HTTP / client surfaces."""
import asyncio
import json
import math
import os
import socket
import sys
import threading
import time
from collections import Counter

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from logprob_checks import consistent  # noqa: E402
from penalty_checks import teacher_forced  # noqa: E402

from pilottai_amd import _runtime  # noqa: E402

# ---------------------------------------------------------------------------
# reference op
# ---------------------------------------------------------------------------

def _formula(logits, counts, a, b):
    """The issue's formula in fp64, rounded once; entries with count 0 keep their bits."""
    c = counts.double()
    out = (logits.double() - (a * (c > 0).double() + b * c)).to(logits.dtype)
    return torch.where(c > 0, out, logits)


def test_reference_op_formula_untouched_rows_and_state():
    from pilottai_amd import ops
    from pilottai_amd.ops import reference as ref

    V, rows, cap, slots = 520, 6, 64, 5
    g = torch.Generator().manual_seed(2)
    logits0 = (torch.randn(rows, V, generator=g) * 4).to(torch.bfloat16)
    state = ops.penalty_state(slots, V, cap, "cpu")
    assert [t.shape for t in state] == [(slots, V), (slots, cap), (slots,)] and all(t.dtype == torch.int32 for t in state)
    i32 = lambda x: torch.tensor(x, dtype=torch.int32)  # noqa: E731
    #            plain  forced  pen     pen    pen(neg)  pen(empty list)
    pen_slot = i32([-1, 1, 0, 3, 2, 4])
    forced = i32([-1, 9, -1, -1, -1, -1])
    presence = torch.tensor([1.0, 1.0, 1.5, 0.0, -0.5, 2.0])
    frequency = torch.tensor([1.0, 1.0, 0.5, 2.0, -0.125, 2.0])
    fed = [Counter() for _ in range(slots)]
    rng = np.random.default_rng(0)
    logits = logits0.clone()
    for call in range(3):
        lists = [[5, 6], [7, 7], rng.integers(0, 40, 30).tolist(), [0, V - 1, 0, 17, 17, 17],
                 rng.integers(0, V, 9).tolist(), [] if call else [3, 3]]
        start = np.cumsum([0] + [len(x) for x in lists[:-1]]).tolist()
        logits = logits0.clone()
        ops.apply_penalties(logits, state, pen_slot, i32([0] * rows), presence, frequency, forced, i32(start),
                            i32([len(x) for x in lists]), i32([t for x in lists for t in x]))
        for r in (2, 3, 4, 5):
            fed[int(pen_slot[r])].update(lists[r])
        for r in range(rows):
            if r < 2:  # slot -1 and forced rows: bit-identical, and the forced row's slot stays empty
                assert torch.equal(logits[r].view(torch.int16), logits0[r].view(torch.int16))
                continue
            s = int(pen_slot[r])
            want = _formula(logits0[r], state[0][s], float(presence[r]), float(frequency[r]))
            assert torch.equal(logits[r].view(torch.int16), want.view(torch.int16)), (call, r)
        for s in range(slots):
            assert {t: int(c) for t, c in enumerate(state[0][s].tolist()) if c} == dict(fed[s]), (call, s)
            n = int(state[2][s])
            assert sorted(state[1][s, :n].tolist()) == sorted(fed[s])
    assert int(state[2][1]) == 0 and not fed[1]
    # a reset clears what the slot's list names, then counts the row's own list
    ref.apply_penalties(logits0[:1].clone(), state, i32([0]), i32([1]), presence[:1], frequency[:1], i32([-1]),
                        i32([0]), i32([3]), i32([8, 8, 2]))
    assert {t: c for t, c in enumerate(state[0][0].tolist()) if c} == {8: 2, 2: 1} and int(state[2][0]) == 2


# ---------------------------------------------------------------------------
# scheduler against a model of the device
# ---------------------------------------------------------------------------

LIT, STR = 0, 2
BIG = 1 << 20


def _lit(toks):
    return (LIT, list(toks), -1, -1, -1, -1, 0, 1, 1)


def _str(end, n):
    return (STR, [], -1, -1, end, -1, n, 1, 1)


def _long_prefix_segs():
    """40 forced tokens, then free strings separated by forced runs that repeat tokens."""
    return [_lit(range(5000, 5040)), _str(9001, 5), _lit([6000, 6001, 6000, 6002]), _str(9002, 4),
            _lit([6000, 5000, 7000]), _str(9003, 3), _lit([7001])]


def _sched(**kw):
    cfg = {"num_blocks": 64, "block_size": 16, "max_num_seqs": 8, "max_num_batched_tokens": 128,
           "max_model_len": 512, "prefix_caching": False, "eos_ids": [128009]}
    cfg.update(kw)
    s = _runtime.Scheduler(cfg)
    L = s.layout()
    return s, L, np.zeros(L["total"], dtype=np.int32)


class _Run:
    """Drives a scheduler with a host sampler and a model of the device's penalty slots; the
    requests' generated tokens are mirrored on the host (grammar replayed), so that at every
    sampling row of a penalised request the model's counts can be compared with the truth."""

    def __init__(self, s, L, buf, slots):
        self.s, self.L, self.buf = s, L, buf
        self.dev = [Counter() for _ in range(slots)]
        self.req = {}        # rid -> dict(pen, gen, gr, slot, checked, resets, sent)
        self.outs = {}
        self.pen_steps = 0
        self.cached_resume = 0

    def add(self, rid, prompt, max_tokens, segs=None, pen=(0.0, 0.0), **kw):
        gr = _runtime.Grammar(segs) if segs is not None else None
        gen = list(gr.take_forced_run(BIG)) if gr is not None else []
        self.req[rid] = dict(pen=pen, gen=gen, gr=gr, slot=None, checked=0, resets=0, sent=0, plen=len(prompt))
        self.s.add_request(rid, prompt, 0.0, max_tokens, rid, segs is None, [], segs,
                           presence_penalty=pen[0], frequency_penalty=pen[1], **kw)

    def step(self, step, pick):
        s, L, buf = self.s, self.L, self.buf
        if s.schedule(buf.ctypes.data) == 0:
            return False
        ms = L["max_seqs"]
        c = buf[L["counts"]:L["counts"] + 12]
        nsamp = int(c[2])
        seeds = buf[L["seeds"]:L["seeds"] + 2 * ms].view(np.int64)
        forced = buf[L["forced"]:L["forced"] + ms]
        arr = {k: buf[L[k]:L[k] + ms] for k in ("pen_slot", "pen_reset", "pair_start", "pair_n")}
        fl = {k: buf[L[k]:L[k] + ms].view(np.float32) for k in ("pen_presence", "pen_frequency")}
        pair_tok = buf[L["pair_tok"]:L["pair_tok"] + L["pair_cap"]]
        pen_step = int(c[9]) == 1
        assert int(c[9]) in (0, 1)
        if pen_step:  # what the kernel does, row by row
            self.pen_steps += 1
            assert bool((arr["pen_slot"][nsamp:] == -1).all())
            seen, end = set(), 0
            for r in range(nsamp):
                slot = int(arr["pen_slot"][r])
                if slot < 0 or forced[r] >= 0:
                    continue
                assert slot not in seen and 0 <= slot < len(self.dev)
                seen.add(slot)
                if arr["pen_reset"][r]:
                    self.dev[slot].clear()
                a0, n = int(arr["pair_start"][r]), int(arr["pair_n"][r])
                assert a0 == end and a0 + n <= L["pair_cap"]  # packed, in row order
                end = a0 + n
                self.dev[slot].update(pair_tok[a0:a0 + n].tolist())
            assert int(c[10]) == end
        sampled = np.zeros(max(1, nsamp), dtype=np.int32)
        for r in range(nsamp):
            q = self.req[int(seeds[r])]
            f = int(forced[r])
            if q["pen"] != (0.0, 0.0) and f < 0:
                assert pen_step
                slot = int(arr["pen_slot"][r])
                assert slot >= 0 and (q["slot"] is None or q["slot"] == slot)  # one slot, kept to the end
                q["slot"] = slot
                assert self.dev[slot] == Counter(q["gen"]), (step, r, self.dev[slot], Counter(q["gen"]))
                assert (float(fl["pen_presence"][r]), float(fl["pen_frequency"][r])) == q["pen"]
                q["sent"] += int(arr["pair_n"][r])
                assert q["sent"] == len(q["gen"])  # everything sent, nothing twice
                assert int(arr["pen_reset"][r]) == (1 if q["checked"] == 0 else 0)  # first sampling row only
                q["checked"] += 1
            elif pen_step:
                assert int(arr["pen_slot"][r]) == -1 or f >= 0
                assert int(arr["pair_n"][r]) == 0 and int(arr["pen_reset"][r]) == 0
            t = f if f >= 0 else pick(step, r)
            sampled[r] = t
            q["gen"].append(t)
            if q["gr"] is not None:
                q["gr"].advance(t)
                if not q["gr"].done():
                    q["gen"] += list(q["gr"].take_forced_run(BIG))
        for o in s.commit(sampled.ctypes.data, nsamp):
            self.outs[o[0]] = o
        return True

    def run(self, pick, on_step=None, max_steps=3000):
        for step in range(max_steps):
            if not self.step(step, pick):
                break
            if on_step is not None:
                on_step(step)
        return self.outs


def test_scheduler_counts_follow_forced_runs_jump_forward_and_chunks():
    """A 40-token forced prefix jump-forwarded at admission and prefilled in 16-token chunks,
    jump-forward runs that repeat tokens, next to an unpenalised request on the same grammar."""
    s, L, buf = _sched(max_num_batched_tokens=16)
    run = _Run(s, L, buf, 8)
    segs = _long_prefix_segs()
    run.add(1, list(range(100, 130)), 200, segs, pen=(1.5, 0.5))
    run.add(2, list(range(200, 221)), 200, segs)
    run.add(3, list(range(300, 309)), 12, None, pen=(0.0, -1.0))
    assert s.num_free_penalty_slots == 8
    outs = run.run(lambda step, r: (40 + step % 3) if step % 5 else 9001 + step % 3)
    assert set(outs) == {1, 2, 3}
    for rid in (1, 2, 3):
        assert list(outs[rid][1]) == run.req[rid]["gen"]  # the host mirror is the scheduler's truth
    assert outs[1][6] >= 40 + 8 and outs[1][2] == 0  # forced prefix + jump-forward runs, stopped by the grammar
    assert run.req[1]["checked"] >= 3 and run.req[3]["checked"] == 12 and run.req[2]["checked"] == 0
    assert s.num_free_penalty_slots == 8  # finish returns the slots


def test_scheduler_preemption_keeps_the_slot_and_sends_nothing_twice():
    s, L, buf = _sched(num_blocks=10, max_num_seqs=4, max_num_batched_tokens=256, max_model_len=256,
                       prefix_caching=True)
    run = _Run(s, L, buf, 4)
    run.add(1, list(range(40)), 44, None, pen=(1.0, 0.25))
    # the same first block as request 1: the victim's own copy of it is private (unhashed), so the
    # survivor's next block comes from there and the victim's hashed blocks outlive the preemption
    run.add(2, list(range(16)) + list(range(1000, 1024)), 44, None, pen=(0.5, 0.0))
    cached = []

    was_running = {}

    def watch(step):  # the first row of a preempted request: what it skips came from the prefix cache
        seeds = buf[L["seeds"]:L["seeds"] + 4].view(np.int64)
        # rows are sequences in plan order; every row of these steps samples, so row r has seed r
        for r in range(int(buf[L["counts"] + 1])):
            rid = int(seeds[r])
            if s.total_preemptions > 0 and was_running.get(rid) is False:
                cached.append(int(buf[L["ctx_len"] + r]) - int(buf[L["q_len"] + r]))
        was_running.update({st[0]: bool(st[1]) for st in s.debug_state()})

    outs = run.run(lambda step, r: 2000 + (step * 7 + r) % 5, on_step=watch)
    assert s.total_preemptions >= 1
    assert cached and all(x > 0 and x % 16 == 0 for x in cached)  # the resume hit the prefix cache
    assert len(outs[1][1]) == 44 and len(outs[2][1]) == 44
    for rid in (1, 2):
        assert list(outs[rid][1]) == run.req[rid]["gen"] and run.req[rid]["checked"] == 44
    assert s.num_free_penalty_slots == 4


def test_scheduler_slots_exhausted_abort_and_reuse():
    s, L, buf = _sched(penalty_slots=1)
    run = _Run(s, L, buf, 1)
    assert s.num_free_penalty_slots == 1
    run.add(1, list(range(100, 110)), 6, None, pen=(1.0, 0.0))
    run.add(2, list(range(200, 210)), 6, None, pen=(0.0, 1.0))   # waits for the slot
    run.add(3, list(range(300, 310)), 3, None)                   # unpenalised, behind it: proceeds
    pick = lambda step, r: 50 + step % 2  # noqa: E731
    assert run.step(0, pick)
    assert s.num_free_penalty_slots == 0 and s.num_running == 2 and s.num_waiting == 1
    for step in range(1, 4):
        assert run.step(step, pick)
    assert 3 in run.outs and 1 not in run.outs and run.req[2]["checked"] == 0
    run.run(pick)
    assert set(run.outs) == {1, 2, 3} and run.req[2]["checked"] == 6  # reused slot: reset on its first row only
    assert run.req[1]["slot"] == run.req[2]["slot"] == 0
    assert s.num_free_penalty_slots == 1
    # abort returns the slot, before and after admission
    run.add(4, list(range(400, 410)), 50, None, pen=(1.0, 1.0))
    run.add(5, list(range(500, 510)), 50, None, pen=(1.0, 1.0))
    for step in range(3):
        assert run.step(step, pick)
    assert s.num_free_penalty_slots == 0
    assert s.abort(5) and s.num_free_penalty_slots == 0
    assert s.abort(4) and s.num_free_penalty_slots == 1
    assert {o[0] for o in s.drain_aborted()} == {4, 5}
    run.add(6, list(range(600, 610)), 2, None, pen=(2.0, -2.0))
    run.run(pick)
    assert 6 in run.outs and run.req[6]["checked"] == 2 and s.num_free_penalty_slots == 1


def test_scheduler_pair_region_overflow_leaves_the_entry_out():
    """Two rows whose backlogs together exceed the pair region: the second waits for the next
    step, and never samples on incomplete counts."""
    s, L, buf = _sched(max_num_batched_tokens=16, max_model_len=64)
    assert L["pair_cap"] == 16 + 64
    run = _Run(s, L, buf, 8)
    segs = [_lit(range(5000, 5045)), _str(9001, 3)]
    run.add(1, list(range(100, 104)), 60, segs, pen=(1.0, 1.0))
    run.add(2, list(range(200, 204)), 60, segs, pen=(1.0, 1.0))
    outs = run.run(lambda step, r: 40)
    assert set(outs) == {1, 2} and all(run.req[r]["checked"] >= 1 for r in (1, 2))
    assert all(list(outs[r][1]) == run.req[r]["gen"] for r in (1, 2))


def test_scheduler_old_signatures_and_unpenalised_runs_are_unchanged():
    names = ["counts", "n_items", "part_size", "input_ids", "positions", "slots", "q_start", "q_len", "ctx_len",
             "logit_rows", "mask_class", "forced", "offsets", "temperature", "top_k", "top_p", "seeds", "lp_n",
             "items", "block_table", "embed_rows"]
    s, L, buf = _sched()
    # the parent's layout: the same regions in the same order, 4-word aligned, from offset 0
    ms, mt = L["max_seqs"], L["max_tokens"]
    size = {"counts": 12, "n_items": 1, "part_size": 1, "input_ids": mt, "positions": mt, "slots": mt,
            "seeds": 2 * ms, "items": 4 * L["max_items"], "block_table": ms * L["max_blocks"], "embed_rows": mt}
    o = 0
    for n in names:
        assert L[n] == o, n
        o = (o + size.get(n, ms) + 3) & ~3
    assert L["pen_slot"] == o and L["pen_slot"] < L["pen_reset"] < L["pen_presence"] < L["pen_frequency"] \
        < L["pair_start"] < L["pair_n"] < L["pair_tok"] and L["pair_tok"] + L["pair_cap"] <= L["total"]
    assert L["pair_cap"] == mt + 512

    def drive(sched, b, penalty_args):
        sched.add_request(1, list(range(100, 120)), 0.0, 3, 7, True, [], None)                      # 8 arguments
        sched.add_request(2, list(range(200, 220)), 0.8, 3, 8, True, [], None, 5, 0.9)              # top-k / top-p
        sched.add_request(3, list(range(300, 320)), 0.0, 3, 9, True, [], None, 0, 1.0, False, False, 2,
                          *penalty_args)
        snaps = []
        for step in range(20):
            b[L["pen_slot"]:] = 0x5a5a5a5a  # poison: an unpenalised step writes nothing behind embed_rows
            if sched.schedule(b.ctypes.data) == 0:
                break
            assert int(b[L["counts"] + 9]) == 0 and int(b[L["counts"] + 10]) == 0
            assert bool((b[L["pen_slot"]:] == 0x5a5a5a5a).all())
            snaps.append(b[:L["embed_rows"] + mt].copy())
            n = int(b[L["counts"] + 2])
            sampled = np.full(max(1, n), 7, dtype=np.int32)
            sched.commit(sampled.ctypes.data, n)
        return snaps

    a = drive(s, buf, ())
    s2, _, buf2 = _sched()
    b = drive(s2, buf2, (0.0, 0.0))  # explicit zeros: the same request
    assert len(a) == len(b) >= 3 and all(np.array_equal(x, y) for x, y in zip(a, b))
    assert s.num_free_penalty_slots == 8 and s2.num_free_penalty_slots == 8


# ---------------------------------------------------------------------------
# CPU engine (serial loop)
# ---------------------------------------------------------------------------

def _engine(**kw):
    from pilottai_amd.engine.engine import EngineConfig, LLMEngine

    cfg = dict(model="tiny", max_num_seqs=8, max_num_batched_tokens=128, max_model_len=512, num_kv_blocks=128,
               use_graphs=False)
    cfg.update(kw)
    return LLMEngine(EngineConfig(**cfg), device="cpu")


@pytest.fixture(scope="module")
def engine():
    e = _engine()
    yield e
    e.stop()


def _prompts(tok):
    return [tok.encode("The orchestrator analyses a task and delegates it"), tok.encode("evaluate this result please")]


@pytest.mark.parametrize("mode", ["greedy", "t0.8", "grammar"])
def test_engine_zero_penalties_are_the_plain_request(mode):
    e = _engine()
    try:
        segs = e.grammar.compile("orchestrator.result_evaluation") if mode == "grammar" else None
        kw = dict(temperature=0.0 if mode == "greedy" else 0.8, max_tokens=200 if segs else 8,
                  ignore_eos=segs is None, seed=4321, grammar=segs)
        plain = e.generate(_prompts(e.tok), **kw)
        zero = e.generate(_prompts(e.tok), presence_penalty=0, frequency_penalty=0.0, **kw)
        assert [o.token_ids for o in plain] == [o.token_ids for o in zero]
        assert e._pen_state is None and all(len(k) < 5 for k in e._graphs)
        assert e.sched.num_free_penalty_slots == 8
    finally:
        e.stop()


def test_engine_teacher_forced_penalised_greedy(engine):
    p = _prompts(engine.tok)[0]
    kw = dict(temperature=0.0, max_tokens=24, ignore_eos=True)
    plain = engine.generate([p], **kw)[0].token_ids
    pen = engine.generate([p], presence_penalty=1.5, frequency_penalty=0.5, **kw)[0].token_ids
    assert pen != plain and len(pen) == 24  # the penalties change this prompt's greedy reply
    teacher_forced(engine, p, pen, 1.5, 0.5)
    assert engine._pen_state is not None and engine.sched.num_free_penalty_slots == 8


def test_engine_penalised_request_alone_and_in_a_mixed_batch(engine):
    tok = engine.tok
    prompts = [_prompts(tok)[0]] + [tok.encode(f"request number {i} asks for a plan") for i in range(1, 8)]

    def run(which):
        res = {}
        for i in which:
            kw = dict(temperature=0.0, max_tokens=24, presence_penalty=1.5, frequency_penalty=0.5) if i == 0 \
                else dict(temperature=0.8, max_tokens=16)
            engine.submit(prompts[i], lambda o, i=i: res.__setitem__(i, o), ignore_eos=True, seed=100 + i, **kw)
        while len(res) < len(which):
            assert engine.step() or len(res) == len(which)
        return res

    alone, mixed = run([0]), run(range(8))
    assert alone[0].token_ids == mixed[0].token_ids
    unpen = engine.generate([prompts[0]], temperature=0.0, max_tokens=24, ignore_eos=True)[0]
    assert unpen.token_ids != alone[0].token_ids  # the penalties were at work


def test_engine_preempted_penalised_request_gives_the_same_tokens():
    tok_kw = dict(temperature=0.0, max_tokens=40, ignore_eos=True, presence_penalty=0.5, frequency_penalty=0.5)
    outs = []
    for blocks in (128, 6):
        e = _engine(num_kv_blocks=blocks, max_model_len=64, max_num_seqs=4, prefix_caching=False)
        try:
            ps = [e.tok.encode("the first agent plans the whole task now")[:8],
                  e.tok.encode("a second agent checks every result twice")[:8],
                  e.tok.encode("third in line and the one to be preempted")[:8]]
            outs.append([o.token_ids for o in e.generate(ps, **tok_kw)])
            assert (e.sched.total_preemptions > 0) == (blocks == 6)
            assert e.sched.num_free_penalty_slots == 4
        finally:
            e.stop()
    assert outs[0] == outs[1]


def test_engine_penalties_with_logprobs_and_grammar(engine):
    segs = engine.grammar.compile("orchestrator.result_evaluation")
    p = _prompts(engine.tok)
    free = engine.generate(p, temperature=0.8, max_tokens=12, ignore_eos=True, seed=5, logprobs=3,
                           presence_penalty=1.0, frequency_penalty=1.0)
    for o in free:
        consistent(engine, o, 3)
    gram = engine.generate(p, temperature=0.0, max_tokens=200, grammar=segs, logprobs=3, frequency_penalty=1.5)
    for o in gram:
        assert o.finish_reason == "stop"
        json.loads(o.text)
        consistent(engine, o, 3, greedy=True, segs=segs)


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------

def test_submit_refuses_bad_penalties(engine):
    cb = lambda o: None  # noqa: E731
    for name in ("presence_penalty", "frequency_penalty"):
        for bad in (2.5, -2.01, math.nan, math.inf, "1", True):
            with pytest.raises(ValueError):
                engine.submit([1, 2, 3], cb, **{name: bad})
        for emb in (True, "last"):
            with pytest.raises(ValueError):
                engine.submit([1, 2, 3], cb, embed=emb, **{name: 0.5})
    assert engine._inbox.empty()
    e = _engine(async_steps=True)
    try:
        with pytest.raises(ValueError, match="async_steps"):
            e.submit([1, 2, 3], cb, frequency_penalty=1.0)
        assert len(e.generate([[1, 2, 3]], temperature=0.0, max_tokens=2, ignore_eos=True, presence_penalty=0.0,
                              frequency_penalty=0)[0].token_ids) == 2
    finally:
        e.stop()


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
    res = {}
    try:
        e.submit([1, 2, 3], lambda o: None, presence_penalty=0.5)
        res["refused"] = False
    except ValueError as err:
        res["refused"] = True
        res["message"] = str(err)
    o = e.generate([[1, 2, 3]], temperature=0.0, max_tokens=2, ignore_eos=True, frequency_penalty=0.0)[0]
    res["tokens"] = len(o.token_ids)
    e.release_followers()
    torch.distributed.destroy_process_group()
    with open(out_path, "w") as f:
        json.dump(res, f)


def test_submit_refuses_penalties_on_a_tp_engine(tmp_path):
    out = str(tmp_path / "tp.json")
    mp.start_processes(_tp_worker, args=(2, _free_port(), out), nprocs=2, join=True, start_method="spawn")
    res = json.load(open(out))
    assert res["refused"] and "TP" in res["message"] and res["tokens"] == 2


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


def test_http_penalties_validation_backends_and_client():
    import httpx

    from pilottai_amd.core.config import LLMConfig
    from pilottai_amd.engine.http_llm import OpenAICompatLLM
    from pilottai_amd.engine.local_llm import LocalLLM, SchemaLLM
    from pilottai_amd.serving.http_server import create_app

    eng = _engine()
    eng.start()
    try:
        backend = LocalLLM(LLMConfig(model_name="tiny", max_tokens=24, retry_attempts=1), engine=eng)
        assert backend.supports_penalties and backend.presence_penalty == 0.0
        body = {"messages": [{"role": "user", "content": "task 1"}], "temperature": 0.0, "max_tokens": 24}
        with _Server(create_app(backend, "tiny", engine=eng)) as url:
            post = lambda **kw: httpx.post(f"{url}/chat/completions", json=dict(body, **kw), timeout=120)  # noqa: E731
            plain = post()
            assert plain.status_code == 200, plain.text
            zero = post(presence_penalty=0, frequency_penalty=0.0)
            assert zero.status_code == 200 and eng._pen_state is None
            text = lambda r: r.json()["choices"][0]["message"]["content"]  # noqa: E731
            assert text(zero) == text(plain)
            pen = post(frequency_penalty=1.0, presence_penalty=-0.5)
            assert pen.status_code == 200 and eng._pen_state is not None
            assert text(pen) != text(plain)
            for bad in (dict(presence_penalty=2.5), dict(frequency_penalty="1"), dict(frequency_penalty=-3),
                        dict(presence_penalty=True)):
                r = post(**bad)
                assert r.status_code == 400 and "penalty" in r.text, (bad, r.text)

            sent = []

            class _Spy(OpenAICompatLLM):
                def _body(self, *args):
                    sent.append(super()._body(*args))
                    return sent[-1]

            async def go():
                llm = _Spy(LLMConfig(provider="openai", base_url=url, model_name="tiny", retry_attempts=1,
                                     timeout=120, max_tokens=24, temperature=0.0, frequency_penalty=1.0))
                a = await llm.generate_response([{"role": "user", "content": "task 1"}],
                                                response_format={"presence_penalty": -0.5})
                b = await llm.generate_response([{"role": "user", "content": "task 1"}],
                                                response_format={"frequency_penalty": 0})
                await llm.aclose()
                return a, b

            a, b = asyncio.run(go())
        assert sent[0]["frequency_penalty"] == 1.0 and sent[0]["presence_penalty"] == -0.5
        assert "frequency_penalty" not in sent[1] and "presence_penalty" not in sent[1]  # zeros stay off the wire
        assert a["content"] == text(pen) and b["content"] == text(plain)
        # LLMConfig defaults reach the engine in process as well
        local = LocalLLM(LLMConfig(model_name="tiny", max_tokens=24, retry_attempts=1, temperature=0.0,
                                   frequency_penalty=1.0, presence_penalty=-0.5), engine=eng)
        assert asyncio.run(local.generate_response([{"role": "user", "content": "task 1"}]))["content"] == text(pen)
    finally:
        eng.stop()
    # the model-free backend refuses a non-zero penalty and accepts zero
    schema = SchemaLLM(seed=1)
    sbody = {"messages": [{"role": "user", "content": "x"}],
             "response_format": {"type": "pilottai_schema", "schema": "orchestrator.result_evaluation"}}
    with _Server(create_app(schema, "schema-test")) as url:
        r = httpx.post(f"{url}/chat/completions", json=dict(sbody, frequency_penalty=0.5), timeout=60)
        assert r.status_code == 400 and "penalties" in r.text
        assert httpx.post(f"{url}/chat/completions", json=dict(sbody, frequency_penalty=0, presence_penalty=0.0),
                          timeout=60).status_code == 200
        assert httpx.post(f"{url}/chat/completions", json=dict(sbody, presence_penalty=9), timeout=60).status_code == 400
