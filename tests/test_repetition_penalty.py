"""Repetition penalty, CPU tier: the reference op, the scheduler's slot and delta plumbing against
a Python model of the device state, the tiny CPU engine, the refusals, and the HTTP / client
surfaces."""
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
from penalty_checks import LOGIT_TOL  # noqa: E402
from repetition_checks import f32, formula, i32, inv, members, penalised_rows, teacher_forced_rep  # noqa: E402

from pilottai_amd import _runtime  # noqa: E402

# ---------------------------------------------------------------------------
# reference op
# ---------------------------------------------------------------------------


def _bits(t):
    return t.view(torch.int16)


def test_reference_op_hand_worked_rows():
    """r = 1.25: float32(1 / r) = 0.800000011920929; 5, 3, 2 and 1 times that round (fp32, then
    bf16 with its 8 significant bits) to 4.0, 2.40625, 1.6015625 and 0.80078125; negatives are
    multiplied by 1.25 exactly. r = 0.5: 1 / r = 2 exactly, positives double and negatives halve."""
    from pilottai_amd import ops

    V = 16
    x = torch.tensor([[5.0, 2.0, 1.0, -4.0, -1.0, 0.0, -0.0, 3.0, -3.0, 7.0, -7.0, float("nan"), 0.5, -0.5, 9.0, -9.0]] * 2,
                     dtype=torch.bfloat16)
    seen = [0, 1, 2, 3, 4, 5, 6, 7, 8, 11]  # 9, 10 and 12..15 never occurred
    state = ops.repetition_state(2, V, 32, "cpu")
    assert [tuple(t.shape) for t in state] == [(2, 1), (2, 32), (2,)] and all(t.dtype == torch.int32 for t in state)
    got = x.clone()
    assert ops.apply_repetition_penalty(got, state, i32([1, 0]), i32([0, 0]), f32([1.25, 0.5]), f32([inv(1.25), 2.0]),
                                        i32([-1, -1]), i32([0, len(seen)]), i32([len(seen)] * 2), i32(seen * 2)) is got
    assert inv(1.25) == 0.800000011920929
    want0 = [4.0, 1.6015625, 0.80078125, -5.0, -1.25, 0.0, -0.0, 2.40625, -3.75, 7.0, -7.0, math.nan, 0.5, -0.5, 9.0, -9.0]
    want1 = [10.0, 4.0, 2.0, -2.0, -0.5, 0.0, -0.0, 6.0, -1.5, 7.0, -7.0, math.nan, 0.5, -0.5, 9.0, -9.0]
    want = torch.tensor([want0, want1], dtype=torch.bfloat16)
    ok = (_bits(got) == _bits(want)) | (got.isnan() & want.isnan())
    assert bool(ok.all()), (got, want)
    assert _bits(got)[0, 6] == _bits(x)[0, 6] and _bits(got)[1, 6] == _bits(x)[0, 6]  # -0 keeps its sign
    assert members(state, 1) == set(seen) == members(state, 0) and state[2].tolist() == [len(seen)] * 2
    assert sorted(state[1][0, :len(seen)].tolist()) == seen


def test_reference_op_duplicates_ranges_forced_rows_reset_and_tail_word():
    from pilottai_amd import ops
    from pilottai_amd.ops import reference as ref

    V, rows, cap, slots = 1037, 6, 64, 6  # 33 membership words, the last one 13 bits wide
    g = torch.Generator().manual_seed(3)
    logits0 = (torch.randn(rows, V, generator=g) * 4).to(torch.bfloat16)
    state = ops.repetition_state(slots, V, cap, "cpu")
    assert state[0].shape == (slots, 33)
    #             plain  forced  dup    range  tail   empty
    rep_slot = i32([-1, 1, 0, 3, 2, 4])
    forced = i32([-1, 9, -1, -1, -1, -1])
    rs = [1.5, 1.5, 1.25, 0.5, 2.0, 1.3]
    fed = [set() for _ in range(slots)]
    rng = np.random.default_rng(0)
    for call in range(3):
        lists = [[5, 6], [7, 7], [17, 17, 3, 17, 3] + rng.integers(0, 40, 30).tolist(),
                 [0, V, -1, V - 1, 1 << 30, V + 5, 0, -(1 << 31)], [1036, 1024, 1035, 1036, 1023, 992],
                 [] if call else [3, 3]]
        start = np.cumsum([0] + [len(x) for x in lists[:-1]]).tolist()
        logits = logits0.clone()
        ops.apply_repetition_penalty(logits, state, rep_slot, i32([0] * rows), f32(rs), f32([inv(r) for r in rs]),
                                     forced, i32(start), i32([len(x) for x in lists]), i32([t for x in lists for t in x]))
        for r in (2, 3, 4, 5):
            fed[int(rep_slot[r])].update(t for t in lists[r] if 0 <= t < V)  # out-of-range ids are skipped
        for r in range(rows):
            if r < 2:  # slot -1 and forced rows: bit-identical, and the forced row's slot stays empty
                assert torch.equal(_bits(logits[r]), _bits(logits0[r]))
                continue
            s = int(rep_slot[r])
            assert torch.equal(_bits(logits[r]), _bits(formula(logits0[r], fed[s], rs[r]))), (call, r)
        for s in range(slots):
            n = int(state[2][s])
            assert members(state, s) == fed[s], (call, s)
            assert sorted(state[1][s, :n].tolist()) == sorted(fed[s])  # each id appended once
    assert int(state[2][1]) == 0 and not fed[1] and int(state[0][1].abs().sum()) == 0
    assert fed[2] == {1036, 1024, 1035, 1023, 992} and int(state[0][2, 32]) == (1 << 12) | (1 << 11) | 1
    assert int(state[0][2, 31]) == -(1 << 31) + 1  # bits 31 (token 1023) and 0 (token 992)
    # a window that leaves the token list is not applied
    before = [t.clone() for t in state]
    lg = logits0[:1].clone()
    ref.apply_repetition_penalty(lg, state, i32([5]), i32([0]), f32([1.5]), f32([inv(1.5)]), i32([-1]), i32([2]),
                                 i32([3]), i32([8, 9, 10, 11]))
    assert all(torch.equal(x, y) for x, y in zip(before, state)) and torch.equal(_bits(lg), _bits(logits0[:1]))
    # a reset clears what the slot's list names -- also a poisoned list and length --, then inserts
    n0 = int(state[2][0])
    assert 2 < n0 < cap
    state[1][0, n0:] = torch.tensor([V + 5, -3] * cap, dtype=torch.int32)[:cap - n0]
    state[2][0] = cap + 1000
    ref.apply_repetition_penalty(logits0[:1].clone(), state, i32([0]), i32([1]), f32([1.5]), f32([inv(1.5)]),
                                 i32([-1]), i32([0]), i32([3]), i32([8, 8, 2]))
    assert int(state[2][0]) == 2 and state[1][0, :2].tolist() == [8, 2] and members(state, 0) == {8, 2}


# ---------------------------------------------------------------------------
# scheduler against a model of the device
# ---------------------------------------------------------------------------

LIT, STR = 0, 2
BIG = 1 << 20
POISON = 0x5a5a5a5a


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
    return s, L, np.zeros(L["rep_total"], dtype=np.int32)


class _Run:
    """Drives a scheduler with a host sampler and a model of the device's slots (the repetition
    sets and the additive penalties' counts); the requests' tokens are mirrored on the host
    (grammar replayed), so that at every sampling row of a request with a repetition penalty the
    modelled set can be compared with set(prompt + generated so far)."""

    def __init__(self, s, L, buf, slots):
        self.s, self.L, self.buf = s, L, buf
        self.dev = [set() for _ in range(slots)]
        self.cnt = [Counter() for _ in range(slots)]
        self.req = {}
        self.outs = {}
        self.rep_steps = self.other_steps = 0
        self.max_words = 0

    def add(self, rid, prompt, max_tokens, segs=None, r=None, pen=(0.0, 0.0), **kw):
        gr = _runtime.Grammar(segs) if segs is not None else None
        gen = list(gr.take_forced_run(BIG)) if gr is not None else []
        self.req[rid] = dict(r=1.0 if r is None else r, pen=pen, prompt=list(prompt), gen=gen, gr=gr, slot=None,
                             checked=0, sent=0, pen_sent=0)
        if r is not None:
            kw["repetition_penalty"] = r
        self.s.add_request(rid, prompt, 0.0, max_tokens, rid, segs is None, [], segs, presence_penalty=pen[0],
                           frequency_penalty=pen[1], **kw)

    def step(self, step, pick):
        s, L, buf = self.s, self.L, self.buf
        buf[L["pen_slot"]:] = POISON
        if s.schedule(buf.ctypes.data, buf.size) == 0:
            return False
        ms = L["max_seqs"]
        c = buf[L["counts"]:L["counts"] + 12]
        nsamp, c9 = int(c[2]), int(c[9])
        seeds = buf[L["seeds"]:L["seeds"] + 2 * ms].view(np.int64)
        forced = buf[L["forced"]:L["forced"] + ms]
        arr = {k: buf[L[k]:L[k] + ms] for k in ("rep_slot", "rep_reset", "rep_start", "rep_n", "pen_slot",
                                                "pen_reset", "pair_start", "pair_n")}
        fl = {k: buf[L[k]:L[k] + ms].view(np.float32) for k in ("rep_r", "rep_inv_r")}
        rep_tok = buf[L["rep_tok"]:L["rep_tok"] + L["rep_cap"]]
        pair_tok = buf[L["pair_tok"]:L["pair_tok"] + L["pair_cap"]]
        rep_step, pen_step = bool(c9 & 2), bool(c9 & 1)
        if not rep_step:
            assert c9 in (0, 1)  # the values every step had before
            assert bool((buf[L["total"]:] == POISON).all())  # nothing is written behind the shaping regions
            self.other_steps += 1
        else:  # what the kernel does, row by row
            self.rep_steps += 1
            assert bool((arr["rep_slot"][nsamp:] == -1).all()) and bool((arr["rep_n"][nsamp:] == 0).all())
            seen, end = set(), 0
            for r in range(nsamp):
                slot = int(arr["rep_slot"][r])
                if slot < 0 or forced[r] >= 0:
                    continue
                assert slot not in seen and 0 <= slot < len(self.dev)
                seen.add(slot)
                if arr["rep_reset"][r]:
                    self.dev[slot].clear()
                a0, n = int(arr["rep_start"][r]), int(arr["rep_n"][r])
                assert a0 == end and a0 + n <= L["rep_cap"]  # packed, in row order
                end = a0 + n
                self.dev[slot].update(rep_tok[a0:a0 + n].tolist())
            assert c9 >> 2 == end
            assert bool((rep_tok[end:] == POISON).all())  # only the words in use are written
            self.max_words = max(self.max_words, end)
        if pen_step:
            for r in range(nsamp):
                slot = int(arr["pen_slot"][r])
                if slot < 0 or forced[r] >= 0:
                    continue
                if arr["pen_reset"][r]:
                    self.cnt[slot].clear()
                a0, n = int(arr["pair_start"][r]), int(arr["pair_n"][r])
                self.cnt[slot].update(pair_tok[a0:a0 + n].tolist())
        sampled = np.zeros(max(1, nsamp), dtype=np.int32)
        for r in range(nsamp):
            q = self.req[int(seeds[r])]
            f = int(forced[r])
            if q["r"] != 1.0 and f < 0:
                assert rep_step
                slot = int(arr["rep_slot"][r])
                assert slot >= 0 and (q["slot"] is None or q["slot"] == slot)  # one slot, kept to the end
                q["slot"] = slot
                hist = q["prompt"] + q["gen"]
                assert self.dev[slot] == set(hist), (step, r, self.dev[slot] ^ set(hist))
                r32 = np.float32(q["r"])
                assert fl["rep_r"][r] == r32 and fl["rep_inv_r"][r] == np.float32(1.0 / float(r32))
                q["sent"] += int(arr["rep_n"][r])
                assert q["sent"] == len(hist)  # everything sent, nothing twice
                assert int(arr["rep_reset"][r]) == (1 if q["checked"] == 0 else 0)  # first sampling row only
                q["checked"] += 1
                if q["pen"] != (0.0, 0.0):  # both kinds of penalty: the same one slot
                    assert pen_step and int(arr["pen_slot"][r]) == slot
                    assert self.cnt[slot] == Counter(q["gen"])
            elif rep_step:
                assert int(arr["rep_slot"][r]) == -1 or f >= 0
                assert int(arr["rep_n"][r]) == 0 and int(arr["rep_reset"][r]) == 0
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


def test_scheduler_refuses_a_buffer_not_stated_to_hold_the_new_regions():
    """`total` is the parent's extent; a scheduler that was given a repetition penalty writes up to
    `rep_total` and says so instead of writing past a buffer sized by `total`."""
    s, L, buf = _sched()
    assert L["total"] < L["rep_total"] == buf.size
    s.add_request(1, list(range(100, 110)), 0.0, 2, 1, True, [], None)
    assert s.schedule(buf.ctypes.data) == 10  # no such request yet: the old call works
    s.commit(np.full(1, 7, dtype=np.int32).ctypes.data, 1)
    s.add_request(2, list(range(200, 210)), 0.0, 2, 2, True, [], None, repetition_penalty=1.3)
    buf[:] = POISON
    for words in (None, 0, L["total"], L["rep_total"] - 1):
        with pytest.raises(ValueError, match="rep_total"):
            s.schedule(buf.ctypes.data) if words is None else s.schedule(buf.ctypes.data, words)
        assert bool((buf == POISON).all()) and s.num_running == 1 and s.num_waiting == 1  # nothing planned
    assert s.schedule(buf.ctypes.data, buf.size) == 11 and int(buf[L["counts"] + 9]) == 2 | (10 << 2)


def test_scheduler_layout_keeps_the_parents_regions():
    s, L, _ = _sched()
    ms = L["max_seqs"]
    o = (L["bias_val"] + L["bias_cap"] + 3) & ~3
    assert L["total"] == o  # what the parent's buffer was: no existing region moved or grew
    for name, n in (("rep_slot", ms), ("rep_reset", ms), ("rep_r", ms), ("rep_inv_r", ms), ("rep_start", ms),
                    ("rep_n", ms), ("rep_tok", L["max_tokens"] + 512)):
        assert L[name] == o, name
        o = (o + n + 3) & ~3
    assert L["rep_total"] == o and L["rep_cap"] == L["max_tokens"] + 512 and L["counts"] == 0 and L["n_items"] == 12


def test_scheduler_sets_follow_chunked_prefill_forced_runs_and_jump_forward():
    """A 100-token prompt prefilled in 16-token chunks, a 40-token forced prefix jump-forwarded at
    admission, jump-forward runs that repeat tokens, next to plain requests on the same grammar."""
    s, L, buf = _sched(max_num_batched_tokens=16)
    run = _Run(s, L, buf, 8)
    segs = _long_prefix_segs()
    run.add(1, list(range(100, 130)), 200, segs, r=1.25)
    run.add(2, list(range(200, 221)), 200, segs)
    run.add(3, [300 + i % 7 for i in range(100)], 12, None, r=0.5)
    run.add(4, list(range(400, 409)), 12, None, r=1.0)  # explicit 1: a plain request
    assert s.num_free_penalty_slots == 8
    outs = run.run(lambda step, r: (40 + step % 3) if step % 5 else 9001 + step % 3)
    assert set(outs) == {1, 2, 3, 4}
    for rid in (1, 2, 3, 4):
        assert list(outs[rid][1]) == run.req[rid]["gen"]  # the host mirror is the scheduler's truth
    assert outs[1][6] >= 40 + 8 and outs[1][2] == 0  # forced prefix + jump-forward runs, stopped by the grammar
    assert run.req[1]["checked"] >= 3 and run.req[3]["checked"] == 12
    assert run.req[2]["checked"] == run.req[4]["checked"] == 0 and run.req[4]["slot"] is None
    assert run.max_words >= 100  # a whole prompt went in one piece
    assert run.rep_steps >= 12 and run.other_steps >= 6
    assert s.num_free_penalty_slots == 8  # finish returns the slots


def test_scheduler_prefix_cached_prompt_still_arrives_whole():
    s, L, buf = _sched(prefix_caching=True)
    run = _Run(s, L, buf, 8)
    prompt = [700 + (i * 7) % 90 for i in range(100)]
    pick = lambda step, r: 40 + step % 3  # noqa: E731
    run.add(1, prompt, 6, None, r=1.3)
    run.run(pick)
    run.add(2, prompt, 6, None, r=1.3)
    run.add(3, prompt, 6, None)
    outs = run.run(pick)
    assert outs[1][4] == 0 and outs[2][4] >= 64 and outs[3][4] >= 64  # cached_prompt_tokens: the cache served them
    assert run.req[1]["checked"] == run.req[2]["checked"] == 6
    assert run.req[2]["sent"] == 100 + 5  # every prompt id and every generated token before the last row


def test_scheduler_preemption_keeps_the_slot_and_sends_nothing_twice():
    s, L, buf = _sched(num_blocks=10, max_num_seqs=4, max_num_batched_tokens=256, max_model_len=256,
                       prefix_caching=True)
    run = _Run(s, L, buf, 4)
    run.add(1, list(range(40)), 44, None, r=1.3)
    run.add(2, list(range(16)) + list(range(1000, 1024)), 44, None, r=0.7)
    outs = run.run(lambda step, r: 2000 + (step * 7 + r) % 5)
    assert s.total_preemptions >= 1
    assert len(outs[1][1]) == 44 and len(outs[2][1]) == 44
    for rid in (1, 2):
        assert list(outs[rid][1]) == run.req[rid]["gen"] and run.req[rid]["checked"] == 44
        assert run.req[rid]["sent"] == 40 + 43
    assert s.num_free_penalty_slots == 4


def test_scheduler_slots_exhausted_abort_reuse_and_one_slot_for_both_kinds():
    s, L, buf = _sched(penalty_slots=1)
    run = _Run(s, L, buf, 1)
    assert s.num_free_penalty_slots == 1
    run.add(1, list(range(100, 110)), 6, None, r=1.2, pen=(1.0, 0.5))  # both kinds: one slot
    run.add(2, list(range(200, 210)), 6, None, r=1.5)                  # waits for the slot
    run.add(3, list(range(300, 310)), 3, None)                         # plain, behind it: proceeds
    pick = lambda step, r: 50 + step % 2  # noqa: E731
    assert run.step(0, pick)
    assert s.num_free_penalty_slots == 0 and s.num_running == 2 and s.num_waiting == 1
    for step in range(1, 4):
        assert run.step(step, pick)
    assert 3 in run.outs and 1 not in run.outs and run.req[2]["checked"] == 0
    run.run(pick)
    assert set(run.outs) == {1, 2, 3} and run.req[1]["checked"] == 6
    assert run.req[2]["checked"] == 6  # reused slot: reset on its first row only (checked row by row)
    assert run.req[1]["slot"] == run.req[2]["slot"] == 0
    assert s.num_free_penalty_slots == 1
    # a penalised-only request takes the slot next, then a repetition request: each kind resets its own state
    run.add(7, list(range(700, 710)), 3, None, pen=(0.5, 0.5))
    run.run(pick)
    # abort returns the slot, before and after admission
    run.add(4, list(range(400, 410)), 50, None, r=1.1)
    run.add(5, list(range(500, 510)), 50, None, r=1.1, pen=(1.0, 1.0))
    for step in range(3):
        assert run.step(step, pick)
    assert s.num_free_penalty_slots == 0
    assert s.abort(5) and s.num_free_penalty_slots == 0
    assert s.abort(4) and s.num_free_penalty_slots == 1
    assert {o[0] for o in s.drain_aborted()} == {4, 5}
    run.add(6, list(range(600, 610)), 2, None, r=2.0)
    run.run(pick)
    assert 6 in run.outs and run.req[6]["checked"] == 2 and s.num_free_penalty_slots == 1


def test_scheduler_token_region_overflow_leaves_the_entry_out():
    """Two rows whose backlogs together exceed the token region: the second waits for the next
    step, and never samples on an incomplete set."""
    s, L, buf = _sched(max_num_batched_tokens=16, max_model_len=64)
    assert L["rep_cap"] == 16 + 64
    run = _Run(s, L, buf, 8)
    segs = [_lit(range(5000, 5045)), _str(9001, 3)]
    run.add(1, list(range(100, 104)), 60, segs, r=1.3)
    run.add(2, list(range(200, 204)), 60, segs, r=1.3)
    outs = run.run(lambda step, r: 40)
    assert set(outs) == {1, 2} and all(run.req[r]["checked"] >= 1 for r in (1, 2))
    assert all(list(outs[r][1]) == run.req[r]["gen"] for r in (1, 2))
    assert 49 <= run.max_words <= 80  # one backlog of 4 + 45 tokens per step, never both


def test_scheduler_step_whose_only_repetition_row_is_forced_writes_nothing():
    """max_tokens cuts the jump-forward of a 45-token forced prefix short, so the request's one
    sampling row is grammar-forced: the device would read nothing, so nothing is written behind
    `total` and the step is not flagged (checked in _Run.step); the slot still comes back."""
    s, L, buf = _sched()
    run = _Run(s, L, buf, 8)
    run.add(1, list(range(100, 104)), 20, [_lit(range(5000, 5045)), _str(9001, 3)], r=1.3)
    outs = run.run(lambda step, r: 40)
    assert list(outs[1][1]) == list(range(5000, 5020)) and outs[1][2] == 1  # 19 jump-forwarded + 1 forced row, length
    assert run.rep_steps == 0 and run.other_steps == 1 and run.req[1]["checked"] == 0
    assert s.num_free_penalty_slots == 8


def test_scheduler_r_one_and_the_other_penalties_write_what_they_wrote():
    """repetition_penalty = 1 passed explicitly is the request without it, word for word; steps
    with penalised-only and shaped-only rows keep counts[9] / counts[11] and write nothing behind
    the shaping regions."""
    s, L, buf = _sched()

    def drive(sched, b, extra):
        sched.add_request(1, list(range(100, 120)), 0.0, 3, 7, True, [], None, **extra)                # plain
        sched.add_request(2, list(range(200, 220)), 0.8, 3, 8, True, [], None, 5, 0.9, **extra)         # top-k / top-p
        sched.add_request(3, list(range(300, 320)), 0.0, 3, 9, True, [], None, 0, 1.0, False, False, 2, 0.5, 0.5,
                          **extra)                                                                      # penalised
        sched.add_request(4, list(range(400, 420)), 0.8, 5, 10, True, [], None, logit_bias=[(5, 2.0)], min_p=0.1,
                          ln_min_p=float(np.float32(np.log(0.1))), **extra)                             # shaped
        snaps, kinds = [], set()
        for step in range(20):
            b[L["embed_rows"] + L["max_tokens"]:] = POISON
            if sched.schedule(b.ctypes.data) == 0:
                break
            c = b[L["counts"]:L["counts"] + 12]
            assert int(c[9]) in (0, 1) and bool((b[L["total"]:] == POISON).all())
            if int(c[9]) == 0:
                assert int(c[10]) == 0 and bool((b[L["pen_slot"]:L["bias_start"]] == POISON).all())
            if int(c[11]) == 0:
                assert bool((b[L["bias_start"]:] == POISON).all())
            else:
                assert int(c[11]) == 1 + 1  # one bias word
            kinds.add((int(c[9]), int(c[11])))
            snaps.append(b.copy())
            n = int(c[2])
            sampled = np.full(max(1, n), 7, dtype=np.int32)
            sched.commit(sampled.ctypes.data, n)
        return snaps, kinds

    a, kinds = drive(s, buf, {})
    assert kinds == {(1, 2), (0, 2), (0, 0)} or kinds == {(1, 2), (0, 2)}, kinds
    s2, _, buf2 = _sched()
    b, _ = drive(s2, buf2, {"repetition_penalty": 1.0})
    s3, _, buf3 = _sched()
    c, _ = drive(s3, buf3, {"repetition_penalty": 1.0, "inv_repetition_penalty": 0.37})  # a stray inverse
    assert len(a) == len(b) == len(c) >= 3
    assert all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in zip(a, b, c))
    assert s.num_free_penalty_slots == s2.num_free_penalty_slots == 8
    # the raw entry point treats what submit() refuses as off, and an embedding request never carries one
    s4, L4, buf4 = _sched()
    for i, bad in enumerate((0.0, -1.0, 2.5, math.nan, math.inf)):
        s4.add_request(10 + i, [1, 2, 3], 0.0, 1, 1, True, [], None, repetition_penalty=bad)
    s4.add_request(20, list(range(30)), 0.0, 1, 1, True, [], None, embed=True, repetition_penalty=1.5)
    buf4[L4["total"]:] = POISON
    assert s4.schedule(buf4.ctypes.data) == 45 and int(buf4[L4["counts"] + 9]) == 0
    assert bool((buf4[L4["total"]:] == POISON).all()) and s4.num_free_penalty_slots == 8


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


def test_engine_r_one_is_the_plain_request():
    e = _engine()
    try:
        for mode in ("greedy", "t0.8", "grammar"):
            segs = e.grammar.compile("orchestrator.result_evaluation") if mode == "grammar" else None
            kw = dict(temperature=0.0 if mode == "greedy" else 0.8, max_tokens=200 if segs else 8,
                      ignore_eos=segs is None, seed=4321, grammar=segs)
            plain = e.generate(_prompts(e.tok), **kw)
            one = e.generate(_prompts(e.tok), repetition_penalty=1, **kw)
            none = e.generate(_prompts(e.tok), repetition_penalty=None, **kw)
            assert [o.token_ids for o in plain] == [o.token_ids for o in one] == [o.token_ids for o in none], mode
        assert e._rep_state is None and e._pen_state is None and all(len(k) < 5 for k in e._graphs)
        assert e.sched.num_free_penalty_slots == 8
    finally:
        e.stop()


def test_engine_teacher_forced_greedy(engine):
    p = _prompts(engine.tok)[0]
    kw = dict(temperature=0.0, max_tokens=24, ignore_eos=True)
    plain = engine.generate([p], **kw)[0].token_ids
    rep = engine.generate([p], repetition_penalty=1.3, **kw)[0].token_ids
    assert rep != plain and len(rep) == 24  # the penalty changes this prompt's greedy reply
    teacher_forced_rep(engine, p, rep, 1.3)
    assert engine._rep_state is not None and engine._pen_state is None
    assert engine.sched.num_free_penalty_slots == 8


def test_engine_alone_and_in_a_mixed_batch(engine):
    tok = engine.tok
    prompts = [_prompts(tok)[0]] + [tok.encode(f"request number {i} asks for a plan") for i in range(1, 8)]

    def run(which):
        res = {}
        for i in which:
            kw = dict(temperature=0.0, max_tokens=24, repetition_penalty=1.3) if i == 0 else \
                dict(temperature=0.8, max_tokens=16, repetition_penalty=0.8) if i == 1 else \
                dict(temperature=0.8, max_tokens=16)
            engine.submit(prompts[i], lambda o, i=i: res.__setitem__(i, o), ignore_eos=True, seed=100 + i, **kw)
        while len(res) < len(which):
            assert engine.step() or len(res) == len(which)
        return res

    alone, alone1, mixed = run([0]), run([1]), run(range(8))
    assert alone[0].token_ids == mixed[0].token_ids and alone1[1].token_ids == mixed[1].token_ids
    plain = engine.generate([prompts[0]], temperature=0.0, max_tokens=24, ignore_eos=True)[0]
    assert plain.token_ids != alone[0].token_ids  # the penalty was at work


def test_engine_preempted_request_gives_the_same_tokens():
    tok_kw = dict(temperature=0.0, max_tokens=40, ignore_eos=True, repetition_penalty=1.3)
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


def test_engine_with_additive_penalties_bias_logprobs_and_grammar(engine):
    """Greedy with all the logit controls at once, teacher-forced in the stated order: repetition
    penalty, presence / frequency, logit_bias; the logprobs are those of that distribution. Their
    bound: a reference logit the engine matches within LOGIT_TOL is scaled by at most
    max(r, 1 / r) = 1.3, and a log-softmax moves by at most twice its inputs' largest error."""
    p = _prompts(engine.tok)[0]
    r, a, b = 1.3, 1.0, 0.5
    plain = engine.generate([p], temperature=0.0, max_tokens=16, ignore_eos=True)[0].token_ids
    bias = {plain[0]: -100.0, (plain[0] + 1) % 1000: 1.5}
    o = engine.generate([p], temperature=0.0, max_tokens=16, ignore_eos=True, logprobs=3, repetition_penalty=r,
                        presence_penalty=a, frequency_penalty=b, logit_bias=bias)[0]
    assert plain[0] not in o.token_ids
    rows = teacher_forced_rep(engine, p, o.token_ids, r, a, b, bias)
    consistent(engine, o, 3, greedy=True)
    ref_lp = torch.log_softmax(rows, dim=-1)
    for i, (t, (lp, top)) in enumerate(zip(o.token_ids, o.logprobs)):
        print(f"token {i}: logprob {lp:.4f}, reference {float(ref_lp[i, t]):.4f}")
        assert abs(lp - float(ref_lp[i, t])) <= 2 * 1.3 * LOGIT_TOL
    segs = engine.grammar.compile("orchestrator.result_evaluation")
    gram = engine.generate(_prompts(engine.tok), temperature=0.0, max_tokens=200, grammar=segs, logprobs=3,
                           repetition_penalty=1.5)
    for g in gram:
        assert g.finish_reason == "stop"
        json.loads(g.text)
        consistent(engine, g, 3, greedy=True, segs=segs)
    assert engine.sched.num_free_penalty_slots == 8


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------

def test_submit_refuses_bad_values_embeds_async_and_no_slots(engine):
    cb = lambda o: None  # noqa: E731
    for bad in (0, 0.0, -1.0, 2.01, 3, math.nan, math.inf, -math.inf, "1.2", True, False, [1.2]):
        with pytest.raises(ValueError, match="repetition_penalty"):
            engine.submit([1, 2, 3], cb, repetition_penalty=bad)
    for emb in (True, "last"):
        with pytest.raises(ValueError, match="embedding"):
            engine.submit([1, 2, 3], cb, embed=emb, repetition_penalty=1.2)
    assert engine._inbox.empty()
    for kw, what in ((dict(async_steps=True), "async_steps"), (dict(penalty_slots=0), "penalty_slots")):
        e = _engine(**kw)
        try:
            with pytest.raises(ValueError, match=what):
                e.submit([1, 2, 3], cb, repetition_penalty=1.2)
            assert len(e.generate([[1, 2, 3]], temperature=0.0, max_tokens=2, ignore_eos=True,
                                  repetition_penalty=1.0)[0].token_ids) == 2
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
        e.submit([1, 2, 3], lambda o: None, repetition_penalty=1.2)
        res["refused"] = False
    except ValueError as err:
        res["refused"] = True
        res["message"] = str(err)
    o = e.generate([[1, 2, 3]], temperature=0.0, max_tokens=2, ignore_eos=True, repetition_penalty=1.0)[0]
    res["tokens"] = len(o.token_ids)
    e.release_followers()
    torch.distributed.destroy_process_group()
    with open(out_path, "w") as f:
        json.dump(res, f)


def test_submit_refuses_a_repetition_penalty_on_a_tp_engine(tmp_path):
    out = str(tmp_path / "tp.json")
    mp.start_processes(_tp_worker, args=(2, _free_port(), out), nprocs=2, join=True, start_method="spawn")
    res = json.load(open(out))
    assert res["refused"] and "TP" in res["message"] and "repetition_penalty" in res["message"]
    assert res["tokens"] == 2


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


def test_http_validation_backends_and_clients():
    import httpx
    from pydantic import ValidationError

    from pilottai_amd.core.config import LLMConfig
    from pilottai_amd.engine.http_llm import OpenAICompatLLM
    from pilottai_amd.engine.local_llm import LocalLLM, SchemaLLM
    from pilottai_amd.serving.http_server import create_app

    assert LLMConfig(model_name="tiny").repetition_penalty == 1.0
    for bad in (0.0, 2.5, -1.0):
        with pytest.raises(ValidationError):
            LLMConfig(model_name="tiny", repetition_penalty=bad)
    eng = _engine()
    eng.start()
    try:
        backend = LocalLLM(LLMConfig(model_name="tiny", max_tokens=24, retry_attempts=1), engine=eng)
        assert backend.supports_repetition_penalty and backend.repetition_penalty == 1.0
        body = {"messages": [{"role": "user", "content": "task 1"}], "temperature": 0.0, "max_tokens": 24}
        with _Server(create_app(backend, "tiny", engine=eng)) as url:
            post = lambda **kw: httpx.post(f"{url}/chat/completions", json=dict(body, **kw), timeout=120)  # noqa: E731
            plain = post()
            assert plain.status_code == 200, plain.text
            one = post(repetition_penalty=1)
            assert one.status_code == 200 and eng._rep_state is None
            text = lambda r: r.json()["choices"][0]["message"]["content"]  # noqa: E731
            assert text(one) == text(plain)
            rep = post(repetition_penalty=1.3)
            assert rep.status_code == 200 and eng._rep_state is not None
            assert text(rep) != text(plain)  # on the parent the field is ignored: the same text
            for bad in (dict(repetition_penalty=0), dict(repetition_penalty="1.2"), dict(repetition_penalty=2.5),
                        dict(repetition_penalty=-1), dict(repetition_penalty=True)):
                r = post(**bad)
                assert r.status_code == 400 and "repetition_penalty" in r.text, (bad, r.text)

            sent = []

            class _Spy(OpenAICompatLLM):
                def _body(self, *args):
                    sent.append(super()._body(*args))
                    return sent[-1]

            async def go():
                llm = _Spy(LLMConfig(provider="openai", base_url=url, model_name="tiny", retry_attempts=1,
                                     timeout=120, max_tokens=24, temperature=0.0, repetition_penalty=1.3))
                a = await llm.generate_response([{"role": "user", "content": "task 1"}])
                b = await llm.generate_response([{"role": "user", "content": "task 1"}],
                                                response_format={"repetition_penalty": 1.0})
                await llm.aclose()
                return a, b

            a, b = asyncio.run(go())
        assert sent[0]["repetition_penalty"] == 1.3 and "repetition_penalty" not in sent[1]  # 1 stays off the wire
        assert a["content"] == text(rep) and b["content"] == text(plain)
        # LLMConfig defaults and response_format reach the engine in process as well
        local = LocalLLM(LLMConfig(model_name="tiny", max_tokens=24, retry_attempts=1, temperature=0.0,
                                   repetition_penalty=1.3), engine=eng)
        msgs = [{"role": "user", "content": "task 1"}]
        assert asyncio.run(local.generate_response(msgs))["content"] == text(rep)
        assert asyncio.run(local.generate_response(msgs, response_format={"repetition_penalty": 1.0}))["content"] \
            == text(plain)
    finally:
        eng.stop()
    # the model-free backend refuses a penalty and accepts 1
    schema = SchemaLLM(seed=1)
    assert not getattr(schema, "supports_repetition_penalty", False)
    sbody = {"messages": [{"role": "user", "content": "x"}],
             "response_format": {"type": "pilottai_schema", "schema": "orchestrator.result_evaluation"}}
    with _Server(create_app(schema, "schema-test")) as url:
        r = httpx.post(f"{url}/chat/completions", json=dict(sbody, repetition_penalty=1.2), timeout=60)
        assert r.status_code == 400 and "repetition_penalty" in r.text
        assert httpx.post(f"{url}/chat/completions", json=dict(sbody, repetition_penalty=1.0),
                          timeout=60).status_code == 200
        assert httpx.post(f"{url}/chat/completions", json=dict(sbody, repetition_penalty=9), timeout=60).status_code == 400
