"""Prefix cache below the block: partial-block reuse (donor index, copy list) and same-step
prefix sharing, through the native runtime's bindings and the tiny engine on the CPU."""
import numpy as np
import pytest

from pilottai_amd import _runtime

B = 16
CFG = {"num_blocks": 64, "block_size": B, "max_num_seqs": 8, "max_num_batched_tokens": 256,
       "max_prefill_tokens": 256, "max_model_len": 512, "gqa_group": 4, "eos_ids": [2]}


# ------------------------------------------------------------------ block manager
def _register(bm, parent, toks):
    b = bm.allocate(1)[0]
    bm.register_block(b, _runtime.hash_block(parent, toks), toks, parent)
    return b


def test_block_manager_longest_head_wins():
    bm = _runtime.BlockManager(32, B, True)
    parent = 1234
    q = list(range(500, 516))
    blocks = {}
    for head in (0, 1, 7, 15):
        blocks[head] = _register(bm, parent, q[:head] + [9000 + 100 * head + i for i in range(B - head)])
    assert bm.num_donors == 4
    d, j = bm.match_head(parent, q)
    assert (d, j) == (blocks[15], 15)
    assert bm.ref_count(d) == 2  # its owner's and the match's
    bm.release(d)
    assert bm.ref_count(d) == 1
    # the cap (one token of the prompt is always computed) and the minimum
    assert bm.match_head(parent, q, max_j=7) == (blocks[7], 7)
    bm.release(blocks[7])
    d, j = bm.match_head(parent, q, max_j=4)
    assert j == 4 and d in (blocks[7], blocks[15])
    bm.release(d)
    assert bm.match_head(parent, q[:1] + [1] * 15, min_j=2) == (-1, 0)
    # j = 0: nothing to copy, no reference taken
    assert bm.match_head(parent, [7] * B) == (-1, 0)
    assert bm.match_head(parent + 1, q) == (-1, 0)  # another chain
    assert [bm.ref_count(b) for b in blocks.values()] == [1, 1, 1, 1]


def test_block_manager_partial_tail_offers_its_fill():
    bm = _runtime.BlockManager(32, B, True)
    q = list(range(500, 516))
    t = bm.allocate(1)[0]
    bm.register_partial(t, 77, q[:5])
    assert bm.match_head(77, q) == (t, 5)
    bm.release(t)
    assert bm.match_head(77, q, max_j=3) == (t, 3)
    bm.release(t)
    # the filled block raises the entry to a full one
    bm.register_block(t, _runtime.hash_block(77, q), q, 77)
    assert bm.num_donors == 1
    assert bm.match_head(77, q[:12] + [1] * 4) == (t, 12)
    bm.release(t)
    # released by its owner it stays cached (evictable), a hashed block or not
    t2 = bm.allocate(1)[0]
    bm.register_partial(t2, 78, q[:9])
    free = bm.num_free
    bm.release(t2)
    assert bm.num_free == free + 1
    assert bm.match_head(78, q) == (t2, 9)


def test_block_manager_reallocated_donor_is_dropped():
    bm = _runtime.BlockManager(2, B, True)
    q = list(range(500, 516))
    b = _register(bm, 5, q)
    t = bm.allocate(1)[0]
    bm.register_partial(t, 6, q[:5])
    bm.release(b)
    bm.release(t)
    assert bm.num_free == 2 and bm.num_donors == 2
    assert bm.match_head(5, q[:8] + [0] * 8) == (b, 8)
    bm.release(b)
    again = bm.allocate(2)  # evicts both
    assert sorted(again) == sorted([b, t])
    assert bm.num_donors == 0 and bm.num_cached == 0
    assert bm.match_head(5, q) == (-1, 0) and bm.match_head(6, q) == (-1, 0)


# ------------------------------------------------------------------ scheduler
class _Run:
    def __init__(self, **over):
        self.s = _runtime.Scheduler(dict(CFG, **over))
        self.L = self.s.layout()
        self.buf = np.zeros(self.L["copy_total"], dtype=np.int32)
        self.outs = {}

    def add(self, rid, prompt, max_tokens=1):
        self.s.add_request(rid, prompt, 0.0, max_tokens, rid, True, [], None)

    def schedule(self):
        return self.s.schedule(self.buf.ctypes.data, self.buf.size)

    def commit(self):
        nsamp = int(self.buf[self.L["counts"] + 2])
        for o in self.s.commit(np.full(max(1, nsamp), 7, np.int32).ctypes.data, nsamp):
            self.outs[o[0]] = o

    def step(self):
        T = self.schedule()
        if T:
            self.commit()
        return T

    def drain(self):
        for _ in range(100):
            if not self.s.has_work():
                break
            self.step()

    def field(self, name, n):
        return self.buf[self.L[name]:self.L[name] + n].copy()

    def table(self, row, n):
        o = self.L["block_table"] + row * self.L["max_blocks"]
        return [int(x) for x in self.buf[o:o + n]]

    def copies(self):
        n = int(self.buf[self.L["n_copies"]])
        return [tuple(int(x) for x in self.buf[self.L["copy_list"] + 3 * i:self.L["copy_list"] + 3 * i + 3])
                for i in range(n)]


A = list(range(1000, 1064))  # 4 full blocks


@pytest.mark.parametrize("off", [1, 15, 16, 17, 31])
def test_scheduler_partial_block_hit(off):
    """A prompt equal to a cached one up to offset `off` of its second block computes exactly
    len - common prefix tokens; the step lists the copy of the head it did not compute."""
    r = _Run(partial_block_reuse=True)
    r.add(1, A, max_tokens=8)  # stays alive: its blocks keep one reference
    assert r.step() == 64
    a_blocks = r.table(0, 4)
    assert r.copies() == []
    c = B + off
    p = A[:c] + [5000 + i for i in range(60 - c)]
    r.add(2, p)
    T = r.schedule()
    q_len = r.field("q_len", 2)
    assert T == 1 + (60 - c) and list(q_len) == [1, 60 - c]
    j = c % B
    if j == 0:
        assert r.copies() == []
    else:
        new = r.table(1, 4)
        assert new[:c // B] == a_blocks[:c // B]
        assert r.copies() == [(a_blocks[c // B], new[c // B], j)]
        assert new[c // B] not in a_blocks
        # the reference on the donor went back when the plan was handed over
        assert r.s.block_ref(a_blocks[c // B]) == 1
        # the computed tokens start at slot j of the new block
        assert int(r.field("slots", 2)[1]) == new[c // B] * B + j
        assert int(r.field("positions", 2)[1]) == c
    r.commit()
    r.drain()
    assert r.outs[2][4] == c and r.s.partial_hit_tokens == j
    assert r.s.total_cached_tokens == c


def test_scheduler_partial_hit_leaves_one_token():
    r = _Run(partial_block_reuse=True)
    r.add(1, A)
    r.drain()
    r.add(2, A[:40])  # everything is cached; the last token is computed all the same
    assert r.schedule() == 1
    (src, dst, j), = r.copies()
    assert j == 7 and int(r.field("positions", 1)[0]) == 39
    r.commit()
    assert r.outs[2][4] == 39 and r.s.partial_hit_tokens == 7
    # the minimum head
    r2 = _Run(partial_block_reuse=True, partial_block_min=8)
    r2.add(1, A)
    r2.drain()
    r2.add(2, A[:39] + [1] * 10)
    assert r2.schedule() == 49 - 32 and r2.copies() == []


def test_scheduler_partial_tail_donor_and_small_buffer():
    """The partly filled last block of a finished prefill serves a prompt that continues it; a
    scheduler whose buffer has no room for the copy list plans no partial hit."""
    r = _Run(partial_block_reuse=True)
    r.add(1, A[:37], max_tokens=4)  # 2 blocks + a tail of 5
    assert r.step() == 37
    tail = r.table(0, 3)[2]
    assert r.s.num_donor_blocks == 3
    r.add(2, A[:37] + [8000 + i for i in range(20)])
    assert r.schedule() == 1 + 20
    assert r.copies() == [(tail, r.table(1, 3)[2], 5)]
    r.commit()
    r.drain()
    small = _runtime.Scheduler(dict(CFG, partial_block_reuse=True))
    L = small.layout()
    buf = np.zeros(L["score_total"], dtype=np.int32)
    for rid, p in ((1, A), (2, A[:40] + [3] * 9)):
        small.add_request(rid, p, 0.0, 1, rid, True, [], None)
        T = small.schedule(buf.ctypes.data, buf.size)
        small.commit(np.full(1, 7, np.int32).ctypes.data, 1)
    assert T == 49 - 32 and buf[L["n_copies"]] == 0 and small.partial_hit_tokens == 0


P40 = list(range(3000, 3040))


def test_scheduler_same_step_prefix():
    """Two requests sharing 40 leading tokens, submitted together."""
    r = _Run(same_step_prefix=True)
    r.add(1, P40 + [5] * 20)
    r.add(2, P40 + [6] * 24)
    assert r.schedule() == 60 + (64 - 32)
    assert int(r.buf[r.L["counts"] + 1]) == 2
    assert r.table(1, 2) == r.table(0, 2)
    assert r.table(1, 4)[2] != r.table(0, 4)[2]
    assert list(r.field("q_len", 2)) == [60, 32] and list(r.field("ctx_len", 2)) == [60, 64]
    assert [r.s.block_ref(b) for b in r.table(0, 2)] == [2, 2]
    assert r.s.prefix_defers == 0 and r.s.same_step_shares == 1
    r.commit()
    r.drain()
    assert r.outs[2][4] == 32 and set(r.outs) == {1, 2}
    assert r.s.num_free_blocks == CFG["num_blocks"]
    # switch off: today's deferral
    o = _Run(same_step_prefix=False)
    o.add(1, P40 + [5] * 20)
    o.add(2, P40 + [6] * 24)
    assert o.schedule() == 60 and int(o.buf[o.L["counts"] + 1]) == 1
    assert o.s.prefix_defers == 1 and o.s.same_step_shares == 0
    o.commit()
    o.drain()
    assert o.outs[2][4] == 32


def test_scheduler_same_step_prefix_survives_the_alignment_trim():
    """token_align trims chunk tails, newest first: the entry whose blocks another entry of the
    step reads keeps the tokens that fill them."""
    r = _Run(same_step_prefix=True, token_align=16, align_slack=15)
    r.add(0, list(range(7000, 7020)))
    r.add(1, P40[:36])
    r.add(2, P40[:35])
    T = r.schedule()
    q_len = list(r.field("q_len", 3))
    assert r.s.aligned_steps == 1 and T % 16 == 0 and T == sum(q_len)
    assert r.table(2, 2) == r.table(1, 2)
    assert q_len[1] >= 32, q_len  # both shared blocks are computed in this step
    assert q_len == [15, 32, 1]
    r.commit()
    r.drain()
    assert set(r.outs) == {0, 1, 2}


# ------------------------------------------------------------------ engine on the CPU
def _stream(e, tok):
    base = tok.encode("shared system prompt for every agent of the workflow, with the task text " * 3)
    assert len(base) > 48
    outs = []
    gen = dict(temperature=0.0, max_tokens=3, ignore_eos=True)
    outs += e.generate([base + tok.encode(" first call")], **gen)
    # leaves the cached text inside a block
    cut = (len(base) // 16) * 16 - 9
    outs += e.generate([base[:cut] + tok.encode(" another ending of the same prompt")], **gen)
    outs += e.generate([base[:cut + 5] + tok.encode(" and one more")], **gen)
    # two new prompts with a common head, submitted together
    head = tok.encode("a different task text that two calls of one agent share from its first word on " * 3)
    assert len(head) > 40
    outs += e.generate([head + tok.encode("analysis"), head + tok.encode("tool selection, please")], **gen)
    return [o.token_ids for o in outs], [o.cached_prompt_tokens for o in outs]


def _run_engine(on: bool, async_steps: bool):
    from pilottai_amd.engine.engine import EngineConfig, LLMEngine
    from pilottai_amd.engine.tokenizer import get_tokenizer

    e = LLMEngine(EngineConfig(model="tiny", max_num_seqs=8, max_num_batched_tokens=128, max_model_len=512,
                               num_kv_blocks=128, async_steps=async_steps, partial_block_reuse=on,
                               same_step_prefix=on), device="cpu")
    try:
        toks, cached = _stream(e, get_tokenizer())
        return toks, cached, e.metrics()
    finally:
        e.stop()


@pytest.fixture(scope="module")
def switches_off():
    """The request stream with both switches off: the tokens every other run must give."""
    toks, cached, m = _run_engine(False, False)
    assert m["partial_hit_tokens"] == 0 and m["same_step_shares"] == 0 and m["prefix_defers"] >= 1
    return toks, cached


@pytest.mark.parametrize("async_steps", [False, True])
def test_engine_cpu_same_tokens_with_and_without(switches_off, async_steps):
    toks, cached, m = _run_engine(True, async_steps)
    assert m["partial_hit_tokens"] > 0 and m["same_step_shares"] >= 1 and m["prefix_defers"] == 0
    assert toks == switches_off[0]
    assert sum(cached) > sum(switches_off[1])
