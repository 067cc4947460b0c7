"""Span embeddings without a GPU: the reference pass on hand-worked rows, chunk_spans, the native
scheduler's span slots and segments against a small device model, the CPU engine on the tiny model
(delivered span means bit-identical to the reference replay of the recorded launches: rows, flags,
slots and the division, not the summation, which on the CPU is the reference itself), every
refusal, EngineEmbedder.embed_document and EnhancedMemory.store_document."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from span_checks import SpanProbe, dense_span_means, rel_l2, run_until, same_bits  # noqa: E402

from pilottai_amd import _runtime  # noqa: E402
from pilottai_amd.memory.embedding import chunk_spans, span_windows  # noqa: E402
from pilottai_amd.ops import reference as ref  # noqa: E402

SPAN_BIT = _runtime.Scheduler.COUNTS9_SPAN_BIT


# ------------------------------------------------------------------ the reference pass
def test_reference_rows_worked_by_hand():
    """Column 0: 2^24, 1, 1, -2^24 in that order is 0 (2^24 + 1 rounds back to 2^24 twice); any
    other order gives 1 or 2. Column 1: 1, 1, 2^24, -2^24 is 2. All values are exact in bf16."""
    big = float(2 ** 24)
    hn = torch.tensor([[big, 1.0], [1.0, 1.0], [1.0, big], [-big, -big], [3.0, 5.0]] + [[0.0, 0.0]] * 3,
                      dtype=torch.bfloat16)
    hn = torch.cat([hn, torch.zeros(8, 6, dtype=torch.bfloat16)], dim=1)  # d = 8
    pool = torch.full((4, 8), float("nan"))
    pool[2] = 10.0
    segs = torch.tensor([0, 4, 0, 1,   # the four rows into slot 0, from +0
                         3, 2, 2, 0,   # rows 3, 4 continue slot 2 (below 2^24 the spacing is 1): 10 - 2^24 + 3, 10 - 2^24 + 5
                         4, 1, 1, 1,   # one row
                         6, 3, 3, 1,   # rows 6..8 leave hn: skipped
                         0, 1, 3, 1], dtype=torch.int32)  # beyond the count: not read
    ref.span_pool(hn, torch.tensor([4], dtype=torch.int32), segs, pool)
    assert pool[0, :2].tolist() == [0.0, 2.0] and pool[0, 2:].abs().sum() == 0
    assert pool[2, :2].tolist() == [-big + 13.0, -big + 15.0] and pool[2, 2] == 10.0
    assert pool[1, :2].tolist() == [3.0, 5.0]
    assert torch.isnan(pool[3]).all()
    # the ops entry point on the CPU is the reference, and refuses d % 8 != 0
    from pilottai_amd import ops

    p2 = torch.full((4, 8), float("nan"))
    ops.span_pool(hn, torch.tensor([1], dtype=torch.int32), segs, p2)
    assert p2[0, :2].tolist() == [0.0, 2.0] and torch.isnan(p2[1:]).all()
    with pytest.raises(ValueError):
        ops.span_pool(torch.zeros(2, 12, dtype=torch.bfloat16), torch.tensor([0], dtype=torch.int32), segs,
                      torch.zeros(1, 12))


# ------------------------------------------------------------------ chunk_spans
def test_chunk_spans_edge_cases():
    assert chunk_spans(5, 8, 2) == [(0, 5)]                                  # one chunk
    assert chunk_spans(8, 8, 2) == [(0, 8)]
    assert chunk_spans(12, 4, 0) == [(0, 4), (4, 8), (8, 12)]                # an exact multiple
    assert chunk_spans(10, 4, 2) == [(0, 4), (2, 6), (4, 8), (6, 10)]        # ... with overlap
    assert chunk_spans(9, 8, 4) == [(0, 8), (4, 9)]                          # a tail shorter than the overlap
    assert chunk_spans(11, 4, 1) == [(0, 4), (3, 7), (6, 10), (9, 11)]
    assert chunk_spans(0, 4, 1) == []
    s = chunk_spans(1000, 256, 32)
    assert s[0] == (0, 256) and s[1] == (224, 480) and s[-1][1] == 1000 and all(b - a <= 256 for a, b in s)
    assert all(s[i + 1][0] == s[i][1] - 32 for i in range(len(s) - 1))
    for bad in [(10, 0, 0), (10, 4, 4), (10, 4, -1), (10, 4, 5), (-1, 4, 0), (10, 4.0, 0), (10, True, 0)]:
        with pytest.raises(ValueError):
            chunk_spans(*bad)


def test_span_windows_start_on_a_chunk_stride_and_no_chunk_straddles():
    wins = span_windows(100, 16, 4, 40, 256)
    spans = chunk_spans(100, 16, 4)
    assert [sp for _, _, w in wins for sp in w] == spans
    for s, e, w in wins:
        assert s % 12 == 0 and e - s <= 40 and w[0][0] == s and w[-1][1] == e
        assert all(s <= a < b <= e for a, b in w)
    assert len(wins) > 1 and wins[1][0] == wins[0][2][-1][1] - 4  # neighbours share the overlap
    assert all(len(w) <= 2 for _, _, w in span_windows(100, 16, 4, 1000, 2))
    with pytest.raises(ValueError):
        span_windows(100, 50, 4, 40, 256)


# ------------------------------------------------------------------ scheduler against a device model
B = 16
CFG = dict(num_blocks=64, block_size=B, max_num_seqs=8, max_num_batched_tokens=64, max_prefill_tokens=64,
           max_model_len=512, gqa_group=4, prefix_caching=True, eos_ids=[2], embed_span_slots=8)


def prompt_of(rid, n):
    return [rid * 1000 + p for p in range(n)]  # a token names its request and its position


class Device:
    """A scheduler and a device whose 'hidden state' of a token is the token id and whose
    'accumulator' is the list of ids added, so order, init flags and slots can be read back."""

    def __init__(self, **over):
        self.s = _runtime.Scheduler(dict(CFG, **over))
        self.L = self.s.layout()
        self.buf = np.zeros(self.L["span_total"], dtype=np.int32)
        self.acc = {}            # span slot -> ids added since its last init
        self.steps = []          # per step with segments: [(first_row, n_rows, slot, init)]
        self.outs, self.fin = {}, {}

    def add(self, rid, n, spans, **kw):
        self.s.add_request(rid, prompt_of(rid, n), 0.0, 1, 0, True, [], None, embed=True, spans=spans, **kw)

    def add_gen(self, rid, n, max_tokens):
        self.s.add_request(rid, prompt_of(rid, n), 0.0, max_tokens, 0, True, [], None)

    def step(self):
        L = self.L
        self.buf[:] = -99
        T = self.s.schedule(self.buf.ctypes.data, self.buf.size)
        if T == 0:
            return 0
        c = self.buf[L["counts"]:L["counts"] + 12]
        ids = self.buf[L["input_ids"]:L["input_ids"] + T]
        if c[9] & SPAN_BIT:
            n = int(self.buf[L["span_n"]])
            q = self.buf[L["span_segs"]:L["span_segs"] + 4 * n].reshape(n, 4).tolist()
            assert 0 < n <= L["span_slots"] and len({x[2] for x in q}) == n  # one segment per slot
            self.steps.append(q)
            for first, rows, slot, init in q:
                assert 0 <= first and rows > 0 and first + rows <= T and 0 <= slot < L["span_slots"]
                if init:
                    self.acc[slot] = []
                self.acc[slot] += ids[first:first + rows].tolist()
        else:  # a step without segments leaves the region alone
            assert (self.buf[L["spec_total"]:] == -99).all()
        nsamp = int(c[2])
        sampled = np.full(max(1, nsamp), 7, dtype=np.int32)
        for o in self.s.commit(sampled.ctypes.data, nsamp):
            self.outs[o[0]] = o
        for rid, slots in self.s.take_span_finishes():
            self.fin[rid] = [list(self.acc.get(s, [])) for s in slots]
        for o in self.s.drain_aborted():
            self.outs[o[0]] = o
        return T

    def drain(self, limit=200):
        for _ in range(limit):
            if not self.s.has_work():
                return
            self.step()
        raise AssertionError("the scheduler did not finish")


def test_scheduler_segments_follow_spans_across_prefill_chunks():
    """150 tokens in chunks of 64: spans inside one chunk, across two and across three, overlapping,
    a one-token span and the whole prompt. Every slot ends up holding exactly its span's tokens in
    order, and a segment carries init exactly when it starts at the span's first token."""
    d = Device()
    spans = [(0, 150), (10, 70), (50, 140), (60, 130), (70, 100), (149, 150)]
    d.add(1, 150, spans)
    d.drain()
    assert d.outs[1][2] == 3 and len(d.outs[1]) == 11  # FINISH_EMBED; the output tuple is unchanged
    assert d.fin[1] == [prompt_of(1, 150)[a:b] for a, b in spans]
    assert [len(q) for q in d.steps] == [4, 5, 4]  # chunks [0, 64), [64, 128), [128, 150)
    first = {}
    for q in d.steps:
        for _, _, slot, init in q:
            assert init == (0 if slot in first else 1)
            first.setdefault(slot, True)
    assert d.s.num_free_span_slots == 8


def test_scheduler_preempted_span_request_restarts_and_reinitialises():
    """10 blocks: a decoding request and a 100-token span request (7 blocks) do not fit together,
    so the span request is preempted (it restarts at token 0) until the other finishes. Every
    restart re-initialises the slots by itself: the final lists are exactly the spans."""
    d = Device(num_blocks=10)
    d.add_gen(1, 60, 6)
    d.step()
    spans = [(0, 100), (5, 90), (64, 100)]
    d.add(2, 100, spans)
    d.drain()
    assert d.s.total_preemptions >= 1
    assert d.fin[2] == [prompt_of(2, 100)[a:b] for a, b in spans]
    assert d.outs[1][2] == 1 and d.s.num_free_span_slots == 8


def test_scheduler_slot_exhaustion_abort_and_limits():
    d = Device(embed_span_slots=4)
    d.add(1, 150, [(0, 10), (5, 150), (100, 150)])
    d.add(2, 20, [(0, 20), (3, 4)])      # needs 2 slots: 1 is free while request 1 runs
    d.add(3, 20, [])                      # a plain embedding request behind it is not held up
    d.step()
    d.step()  # request 1 fills both steps: nothing else is looked at
    assert not d.outs and d.s.num_free_span_slots == 1
    d.step()  # its last 22 tokens leave room: request 2 still lacks a slot, request 3 goes ahead of it
    assert set(d.outs) == {1, 3} and d.s.num_free_span_slots == 4
    assert [(x[0], x[1]) for x in d.s.debug_state()] == [(2, False)]
    d.drain()
    assert d.fin[1] == [prompt_of(1, 150)[a:b] for a, b in [(0, 10), (5, 150), (100, 150)]]
    assert d.fin[2] == [prompt_of(2, 20), prompt_of(2, 20)[3:4]] and d.outs[2][2] == 3
    assert 3 not in d.fin and d.outs[3][2] == 3 and d.s.num_free_span_slots == 4
    # abort: the slots come back, mid-prompt
    d.add(4, 150, [(0, 150), (1, 2), (2, 3), (3, 4)])
    d.step()
    assert d.s.num_free_span_slots == 0
    assert d.s.abort(4)
    assert [o[2] for o in d.s.drain_aborted()] == [2] and d.s.num_free_span_slots == 4
    fin = d.s.take_span_finishes()  # the record names the slots it held
    assert [r for r, _ in fin] == [4] and sorted(fin[0][1]) == [0, 1, 2, 3]
    # more spans than there are slots, and malformed spans, throw at add_request
    for spans in [[(0, 1)] * 5, [(0, 0)], [(3, 2)], [(0, 21)], [(-1, 2)], [(5, 8), (4, 9)]]:
        with pytest.raises(ValueError):
            d.add(5, 20, spans)
    with pytest.raises(ValueError):  # spans belong to a mean-pooled embedding request
        d.s.add_request(5, prompt_of(5, 20), 0.0, 1, 0, True, [], None, spans=[(0, 4)])
    with pytest.raises(ValueError):
        d.s.add_request(5, prompt_of(5, 20), 0.0, 1, 0, True, [], None, embed=True, embed_last=True, spans=[(0, 4)])
    with pytest.raises(ValueError):  # a prompt the scheduler would cut
        d.add(5, 512, [(0, 4)])
    assert not d.s.has_work()


def test_scheduler_refuses_spans_in_a_buffer_not_stated_to_hold_them():
    s = _runtime.Scheduler(dict(CFG))
    L = s.layout()
    assert L["span_n"] == L["spec_total"] and L["span_segs"] == L["span_n"] + 4
    assert L["span_total"] == L["span_segs"] + 4 * 8 and L["span_slots"] == 8
    buf = np.zeros(L["span_total"], dtype=np.int32)
    s.add_request(1, prompt_of(1, 20), 0.0, 1, 0, True, [], None, embed=True)
    assert s.schedule(buf.ctypes.data, L["spec_total"]) == 20  # plain requests: the parent's buffer is enough
    s.commit(buf.ctypes.data, 0)
    s.add_request(2, prompt_of(2, 20), 0.0, 1, 0, True, [], None, embed=True, spans=[(0, 4)])
    for words in (0, L["spec_total"], L["span_total"] - 1):
        with pytest.raises(ValueError):
            s.schedule(buf.ctypes.data, words)
    assert s.schedule(buf.ctypes.data, L["span_total"]) == 20


def test_steps_without_spans_are_byte_identical_to_the_layout_before_spans():
    """The same plain workload (a generation request and a plain embedding request) through a
    scheduler given the whole buffer and through one given only the spec_total words every
    scheduler had before spans: the same bytes, no bit 28, and nothing behind spec_total --
    also after a span request has been through."""
    def plain(s, base):
        s.add_request(base + 1, prompt_of(1, 70), 0.0, 3, 5, True, [], None)
        s.add_request(base + 2, prompt_of(2, 90), 0.0, 1, 0, True, [], None, embed=True)

    a, b = _runtime.Scheduler(dict(CFG)), _runtime.Scheduler(dict(CFG))
    L = a.layout()
    bufa = np.zeros(L["span_total"], dtype=np.int32)
    bufb = np.zeros(L["spec_total"], dtype=np.int32)
    sampled = np.full(8, 7, dtype=np.int32)

    def compare(base):
        plain(a, base)
        plain(b, base)
        n = 0
        while a.has_work():
            bufa[:] = -99
            bufb[:] = -99
            Ta, Tb = a.schedule(bufa.ctypes.data, bufa.size), b.schedule(bufb.ctypes.data, bufb.size)
            assert Ta == Tb and Ta > 0
            assert bufa[: L["spec_total"]].tobytes() == bufb.tobytes()
            assert (bufa[L["spec_total"]:] == -99).all()
            c9 = int(bufa[L["counts"] + 9])
            assert not c9 & SPAN_BIT
            ns = int(bufa[L["counts"] + 2])
            assert [o[:7] for o in a.commit(sampled.ctypes.data, ns)] == [o[:7] for o in b.commit(sampled.ctypes.data, ns)]
            n += 1
        assert n >= 3 and not b.has_work()

    compare(0)
    a.add_request(50, prompt_of(50, 30), 0.0, 1, 0, True, [], None, embed=True, spans=[(0, 30), (7, 9)])
    bufa[:] = -99
    assert a.schedule(bufa.ctypes.data, bufa.size) == 30 and int(bufa[L["counts"] + 9]) & SPAN_BIT
    assert bufa[L["span_n"]] == 2
    a.commit(sampled.ctypes.data, 0)
    assert a.take_span_finishes() == [(50, [0, 1])]
    b.add_request(50, prompt_of(50, 30), 0.0, 1, 0, True, [], None, embed=True)  # the same blocks and rows taken
    assert b.schedule(bufb.ctypes.data, bufb.size) == 30
    b.commit(sampled.ctypes.data, 0)
    compare(100)


def test_bit_28_is_clear_of_the_repetition_words():
    """counts[9] keeps the repetition pass's token words above bit 1: they count at most rep_cap
    tokens, which stays below 2^26 -- so below bit 28 -- for every configuration that accepts spans."""
    s = _runtime.Scheduler(dict(CFG))
    assert (s.layout()["rep_cap"] << 2) < SPAN_BIT
    big = _runtime.Scheduler(dict(CFG, max_model_len=1 << 26, num_blocks=8))
    with pytest.raises(ValueError):
        big.add_request(1, [1, 2, 3], 0.0, 1, 0, True, [], None, embed=True, spans=[(0, 2)])


# ------------------------------------------------------------------ the CPU engine on the tiny model
@pytest.fixture(scope="module")
def engine():
    from pilottai_amd.engine.engine import EngineConfig, LLMEngine

    return LLMEngine(EngineConfig(model="tiny", max_num_seqs=8, max_num_batched_tokens=64, max_model_len=512,
                                  num_kv_blocks=128, embed_span_slots=16), device="cpu")


@pytest.fixture(scope="module")
def long_prompt(engine):
    return engine.tok.encode("Task: summarize the quarterly report for the board. " * 20)[:150]


def test_engine_span_embeddings_are_the_reference_replay_bit_for_bit(engine, long_prompt):
    """A 150-token prompt prefilled in chunks of at most 64 beside a generating request, and a
    short one: the delivered span means are bit-identical to ops.reference.span_pool replayed over
    the recorded launches and divided by the span lengths; against the dense forward they hold the
    bound test_engine_embedding_requests_match_dense_forward uses for whole prompts (2e-2).

    On the CPU ops.kernels.span_pool is ops.reference.span_pool, so the replay does not check the
    summation itself (the reference against itself): it checks what the engine hands to the pass
    and does with its result -- rows, init flags, slots, the host division. The summation is
    checked independently in test_reference_rows_worked_by_hand and, for the kernel, in
    tests/test_span_pool_gpu.py."""
    tok = engine.tok
    short = tok.encode("alpha beta gamma delta")
    spans_long = [(0, 150), (0, 40), (30, 100), (60, 140), (100, 150), (149, 150)]
    spans_short = [(0, len(short)), (1, 2)]
    outs = {}
    with SpanProbe(engine) as probe:
        gen = engine.submit(long_prompt[:40] + [5, 6, 7], lambda o: outs.__setitem__(o.request_id, o),
                            temperature=0.0, max_tokens=6, ignore_eos=True)
        r1 = probe.submit(long_prompt, spans_long, outs)
        r2 = probe.submit(short, spans_short, outs)
        run_until(engine, outs, [gen, r1, r2])
    assert len(probe.calls) >= 3 and any(len(q) >= 3 for q in probe.segments())
    for rid, ids, spans in ((r1, long_prompt, spans_long), (r2, short, spans_short)):
        o = outs[rid]
        assert o.finish_reason == "embed" and o.span_embeddings.shape == (len(spans), 512)
        assert o.span_embeddings.dtype == np.float32
        assert same_bits(o.span_embeddings, probe.expected(rid))
        big = [i for i, (a, b) in enumerate(spans) if b - a >= 16]
        if big:
            errs = rel_l2(o.span_embeddings[big], dense_span_means(engine.model, ids, [spans[i] for i in big]))
            print("span errors against the dense forward:", [f"{e:.2e}" for e in errs])
            assert max(errs) < 2e-2
        whole = engine.model.hidden_states([ids]).float()
        assert rel_l2(o.embedding[None], whole)[0] < 2e-2
    # the whole-prompt span is the whole-prompt embedding up to the order of the adds
    assert rel_l2(outs[r1].span_embeddings[:1], outs[r1].embedding[None])[0] < 1e-5
    assert outs[gen].finish_reason == "length" and outs[gen].span_embeddings is None
    assert engine.sched.num_free_span_slots == 16
    emb0, se0 = engine.embed_spans(short, [])  # no spans: the plain request, an empty array
    assert se0.shape == (0, 512) and rel_l2(emb0[None], outs[r2].embedding[None])[0] < 2e-2  # another batch
    v = engine.embed([short])  # the plain path is what it was
    assert float(engine._embed_pool[:-1].abs().sum()) == 0.0 and v.shape == (1, 512)


def test_embed_span_ordered_switches_the_route_of_span_steps_only(engine, long_prompt, monkeypatch):
    """EngineConfig.embed_span_ordered (default True): a span step on the mid route takes its row
    statistics from row_sumsq behind every residual launch (1 + 2 per layer launches); with the
    switch off it runs what every other step runs (1 launch). Plain embedding steps never change."""
    from pilottai_amd import ops

    calls, orig = [], ops.row_sumsq
    monkeypatch.setattr(ops, "row_sumsq", lambda *a, **kw: (calls.append(1), orig(*a, **kw))[1])
    layers = len(engine.model.layers)
    ids, spans = long_prompt[:60], [(0, 60), (10, 50)]
    assert engine.cfg.embed_span_ordered is True
    _, on = engine.embed_spans(ids, spans)
    assert len(calls) == 1 + 2 * layers
    del calls[:]
    engine.embed([ids])
    assert len(calls) == 1
    del calls[:]
    monkeypatch.setattr(engine.cfg, "embed_span_ordered", False)
    _, off = engine.embed_spans(ids, spans)
    assert len(calls) == 1
    assert max(rel_l2(off, on)) < 2e-2 and engine.sched.num_free_span_slots == 16


def test_engine_refusals(engine):
    cb = lambda o: None  # noqa: E731
    ids = list(range(10, 30))
    bad = [[(0, 21)], [(-1, 3)], [(4, 4)], [(5, 3)], [(4, 8), (2, 9)], [(0, 1)] * 17, [(0.0, 3)], [(True, 3)],
           [(1, 2, 3)], [5]]
    for spans in bad:
        with pytest.raises(ValueError):
            engine.submit(ids, cb, embed=True, spans=spans)
    with pytest.raises(ValueError, match="embed"):
        engine.submit(ids, cb, spans=[(0, 4)])
    with pytest.raises(ValueError, match="last"):
        engine.submit(ids, cb, embed="last", spans=[(0, 4)])
    with pytest.raises(ValueError):
        engine.submit(ids, cb, score_from=3, spans=[(0, 4)])
    with pytest.raises(ValueError, match="max_model_len"):
        engine.submit(list(range(512)), cb, embed=True, spans=[(0, 4)])
    assert engine._inbox.empty()  # nothing of it was queued
    from pilottai_amd.engine.engine import EngineConfig, LLMEngine

    a = LLMEngine(EngineConfig(model="tiny", max_num_seqs=4, max_num_batched_tokens=64, max_model_len=128,
                               num_kv_blocks=32, async_steps=True), device="cpu")
    with pytest.raises(ValueError, match="async_steps"):
        a.submit(ids, cb, embed=True, spans=[(0, 4)])
    assert a.embed([ids]).shape == (1, 512)  # plain embedding requests still run there


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
        e.submit([1, 2, 3], lambda o: None, embed=True, spans=[(0, 2)])
        res["refused"] = False
    except ValueError as err:
        res["refused"] = True
        res["message"] = str(err)
    res["tokens"] = len(e.generate([[1, 2, 3]], temperature=0.0, max_tokens=2, ignore_eos=True)[0].token_ids)
    e.release_followers()
    torch.distributed.destroy_process_group()
    with open(out_path, "w") as f:
        json.dump(res, f)


def test_submit_refuses_spans_on_a_tp_engine(tmp_path):
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
    assert res["refused"] and "tensor-parallel" in res["message"] and res["tokens"] == 2


# ------------------------------------------------------------------ embedder and memory
def test_embed_document_late_and_isolated(engine):
    from pilottai_amd.memory.embedding import EngineEmbedder

    emb = EngineEmbedder(engine, dim=64)
    text = "The orchestrator delegates a task to worker agents and collects every result. " * 12
    ids = engine.tok.encode(text)
    spans = chunk_spans(len(ids), 32, 8)
    texts, vecs, got_spans = emb.embed_document(text, chunk_tokens=32, overlap=8, return_spans=True)
    assert got_spans == spans and texts == [engine.tok.decode(ids[a:b]) for a, b in spans]
    assert vecs.shape == (len(spans), 64) and np.allclose(np.linalg.norm(vecs, axis=1), 1.0, atol=1e-5)
    # the vectors are the engine's span means through the embedder's projection
    _, se = engine.embed_spans(ids, spans)
    assert np.allclose(vecs, emb._project(se), atol=1e-6)
    t2, v2 = emb.embed_document(text, chunk_tokens=32, overlap=8, late=False)
    assert t2 == texts and v2.shape == vecs.shape
    # the first chunk has nothing before it: both ways embed the same tokens in the same context
    assert float(vecs[0] @ v2[0]) > 0.999
    assert float(np.min(np.sum(vecs[1:] * v2[1:], axis=1))) < 0.999  # later chunks have seen the document
    assert emb.embed_document("", chunk_tokens=32, overlap=8)[1].shape == (0, 64)
    # a document longer than the context goes through several windows of whole chunks
    from pilottai_amd.engine.engine import EngineConfig, LLMEngine

    small = LLMEngine(EngineConfig(model="tiny", max_num_seqs=4, max_num_batched_tokens=64, max_model_len=100,
                                   num_kv_blocks=32), device="cpu")
    es = EngineEmbedder(small, dim=64)
    assert len(ids) > 150
    before = small.stats["embed_requests"]
    t3, v3 = es.embed_document(text, chunk_tokens=32, overlap=8)
    wins = span_windows(len(ids), 32, 8, 99, 256)
    assert small.stats["embed_requests"] - before == len(wins) > 1
    assert t3 == texts and v3.shape == vecs.shape
    # a window's first chunk is embedded as in the unwindowed run only for the first window
    assert np.allclose(v3[: len(wins[0][2])], vecs[: len(wins[0][2])], atol=2e-2)


async def test_store_document_with_the_engine_and_with_a_hashing_embedder(engine):
    from pilottai_amd.memory.embedding import EngineEmbedder
    from pilottai_amd.memory.enhanced_memory import EnhancedMemory

    text = "The orchestrator delegates a task to worker agents and collects every result. " * 8
    mem = EnhancedMemory(embedder=EngineEmbedder(engine, dim=64), dim=64, device="cpu")
    rows = await mem.store_document(text, metadata={"source": "report.pdf"}, tags={"doc"}, priority=2,
                                    chunk_tokens=32, overlap=8)
    ids = engine.tok.encode(text)
    spans = chunk_spans(len(ids), 32, 8)
    assert len(rows) == len(spans) == len(set(rows))
    items = [mem._items[r] for r in rows]
    assert len({it.metadata["document"] for it in items}) == 1
    assert [it.metadata["chunk"] for it in items] == list(range(len(spans)))
    assert [tuple(it.metadata["span"]) for it in items] == spans
    assert all(it.metadata["source"] == "report.pdf" and it.tags == {"doc"} and it.priority == 2 for it in items)
    assert [it.text for it in items] == [engine.tok.decode(ids[a:b]) for a, b in spans]
    hits = await mem.semantic_search(items[2].text, limit=3)
    assert hits and all(h.metadata["document"] == items[0].metadata["document"] for h in hits)
    # an embedder without embed_document: chunks of whitespace-separated words, embedded one by one
    plain = EnhancedMemory(dim=128, device="cpu")
    words = text.split()
    rows = await plain.store_document(text, chunk_tokens=20, overlap=5, ttl=60.0)
    wspans = chunk_spans(len(words), 20, 5)
    items = [plain._items[r] for r in rows]
    assert [tuple(it.metadata["span"]) for it in items] == wspans
    assert [it.text for it in items] == [" ".join(words[a:b]) for a, b in wspans]
    assert all(it.expires_at is not None for it in items)
    hit = (await plain.semantic_search(items[-1].text, limit=1))[0]
    assert hit.metadata["document"] == items[0].metadata["document"]
    with pytest.raises(ValueError):
        await plain.store_document("")
    with pytest.raises(ValueError):
        await plain.store_document(text, chunk_tokens=4, overlap=4)
