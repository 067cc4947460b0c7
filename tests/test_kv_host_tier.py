"""Host tier under the prefix cache: spills, fills and their order through the native runtime's
bindings, and the tiny engine on the CPU (where the moves run through the torch references)."""
import os
import sys

import numpy as np
import pytest

from pilottai_amd import _runtime

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from host_tier_checks import GEN, flood, prompt_a, spill_and_restore  # noqa: E402

B = 16
CFG = {"num_blocks": 8, "block_size": B, "max_num_seqs": 4, "max_num_batched_tokens": 256,
       "max_prefill_tokens": 256, "max_model_len": 256, "gqa_group": 4, "eos_ids": [2],
       "host_slots": 16}


class _Run:
    def __init__(self, **over):
        self.s = _runtime.Scheduler(dict(CFG, **over))
        self.L = self.s.layout()
        self.buf = np.zeros(self.L["span_total"], dtype=np.int32)
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
        """-> (tokens, spills, fills) of one schedule() call, committed."""
        T = self.schedule()
        spills, fills = self.s.take_kv_moves()
        if T:
            self.commit()
        return T, spills, fills

    def drain(self):
        spills, fills = [], []
        for _ in range(400):
            if not self.s.has_work():
                break
            _, sp, fi = self.step()
            spills += sp
            fills += fi
        return spills, fills

    def table(self, row, n):
        o = self.L["block_table"] + row * self.L["max_blocks"]
        return [int(x) for x in self.buf[o:o + n]]


A = list(range(1000, 1067))          # 4 full blocks and a tail of 3
X = list(range(3000, 3100))          # 6 full blocks and a tail: 7 blocks
Y = list(range(5000, 5100))


def _a_then_x(**over):
    """A is served and finished, then X takes 7 of the 8 blocks: A's first three go to the host."""
    r = _Run(**over)
    r.add(1, A)
    T, sp, fi = r.step()
    assert T == len(A) and sp == [] and fi == []
    a_blocks = r.table(0, 4)
    assert r.s.prefix_blocks(A) == [(0, b) for b in a_blocks]
    r.add(2, X)
    T, sp, fi = r.step()
    assert T == len(X) and fi == []
    return r, a_blocks, sp


def test_eviction_lists_a_spill_and_a_new_request_the_fills():
    r, a_blocks, sp = _a_then_x()
    assert [b for b, _ in sp] == a_blocks[:3]  # oldest first; the tail of 3 tokens was simply freed
    slots = [s for _, s in sp]
    assert len(set(slots)) == 3 and all(0 <= s < 16 for s in slots)
    assert r.s.host_spilled_blocks == 3 and r.s.num_host_cached == 3 and r.s.host_hit_blocks == 0
    assert r.s.prefix_blocks(A) == [(1, slots[0]), (1, slots[1]), (1, slots[2]), (0, a_blocks[3])]
    before = r.s.total_cached_tokens
    r.add(3, A)
    T = r.schedule()
    spills, fills = r.s.take_kv_moves()
    assert T == len(A) - 64
    new = r.table(0, 4)
    assert [s for s, _ in fills] == slots and [b for _, b in fills] == new[:3]
    assert r.s.host_hit_blocks == 3
    # a resident tail of the chain is never evicted by the restore of its head: A's fourth block
    # was the oldest evictable block of the pool when the restore began
    assert new[3] == a_blocks[3] and a_blocks[3] not in [b for b, _ in spills]
    assert a_blocks[3] not in new[:3]
    # the restores evicted blocks of X instead, which went to the host in their turn
    assert len(spills) == 3 and r.s.host_spilled_blocks == 6
    r.commit()
    assert r.outs[3][4] == 64 and r.s.total_cached_tokens - before == 64
    assert r.s.take_kv_moves() == ([], [])


def test_restored_block_is_not_spilled_twice():
    r, a_blocks, _ = _a_then_x()
    r.add(3, A)
    T, _, fills = r.step()
    restored = [b for _, b in fills]
    assert len(restored) == 3
    spilled = r.s.host_spilled_blocks
    r.add(4, Y)  # 7 blocks again: the restored blocks are evicted a second time
    T, spills, fills = r.step()
    assert T == len(Y) and fills == []
    tiers = r.s.prefix_blocks(A)
    assert [t for t, _ in tiers[:3]] == [1, 1, 1]            # evicted, and still in the tier
    assert not set(restored) & {b for b, _ in spills}        # ... without another copy
    assert r.s.host_spilled_blocks - spilled == len(spills)


def _chain(bm, n, base):
    """n registered blocks of one hash chain, all released: -> [(block, hash, tokens)]."""
    out, parent = [], 0
    for i in range(n):
        toks = [base + 100 * i + j for j in range(B)]
        h = _runtime.hash_block(parent, toks)
        b = bm.allocate(1)[0]
        bm.register_block(b, h, toks, parent)
        out.append((b, h, toks))
        parent = h
    for b, _, _ in out:
        bm.release(b)
    return out


def test_full_host_tier_evicts_its_oldest_unpinned_slot():
    bm = _runtime.BlockManager(4, B, True, host_slots=2)
    ch = _chain(bm, 4, 100)
    got = bm.allocate(3)  # evicts the three oldest
    spills, fills = bm.take_moves()
    # both slots were taken by moves not yet executed (pinned): the third block was dropped
    assert [b for b, _ in spills] == [ch[0][0], ch[1][0]] and fills == []
    assert bm.host_spilled_blocks == 2 and bm.host_evicted_blocks == 0
    assert bm.host_peek(ch[0][1], ch[0][2]) >= 0 and bm.host_peek(ch[2][1], ch[2][2]) == -1
    for b in got:
        bm.release(b)
    # the moves were taken: the next eviction of a hashed block replaces the oldest slot
    bm.allocate(4)
    spills, _ = bm.take_moves()
    assert spills == [(ch[3][0], spills[0][1])] and bm.host_evicted_blocks == 1
    assert bm.host_peek(ch[0][1], ch[0][2]) == -1           # the oldest went
    assert bm.host_peek(ch[1][1], ch[1][2]) >= 0 and bm.host_peek(ch[3][1], ch[3][2]) >= 0
    assert bm.num_host_cached == 2
    # verification tokens: the same hash with other tokens is no hit
    assert bm.host_peek(ch[1][1], [1] * B) == -1


def test_block_manager_without_host_slots_plans_nothing():
    bm = _runtime.BlockManager(4, B, True)
    ch = _chain(bm, 4, 100)
    bm.allocate(4)
    assert bm.take_moves() == ([], []) and bm.num_host_cached == 0
    assert bm.host_peek(ch[0][1], ch[0][2]) == -1 and bm.restore(0) == -1


def test_fill_cap_ends_the_chain():
    r, a_blocks, sp = _a_then_x(host_cache_step_blocks=2)
    r.add(3, A)
    T = r.schedule()
    _, fills = r.s.take_kv_moves()
    # two blocks come back, the chain ends there: the third is computed although it is in the
    # tier, and so is the fourth although it is resident
    assert len(fills) == 2 and T == len(A) - 32
    assert r.table(0, 4)[3] != a_blocks[3]
    r.commit()
    assert r.outs[3][4] == 32 and r.s.host_hit_blocks == 2
    # the cap is per schedule() call
    r.drain()
    off = _a_then_x(host_cache_step_blocks=0)[0]
    off.add(3, A)
    T, _, fills = off.step()
    assert fills == [] and off.s.host_hit_blocks == 0


def test_moves_of_a_schedule_call_without_a_step():
    r = _Run()
    r.add(1, A)
    r.step()
    r.add(2, list(range(3000, 3127)))  # 8 blocks: every block of A goes to the host
    T, sp, _ = r.step()
    assert T == 127 and len(sp) == 4
    # 10 blocks do not fit the pool of 8: nothing is scheduled, but the head of the prompt was
    # brought back for it, and those fills (and the spills that made room) must still be run
    r.add(3, A[:64] + list(range(7000, 7096)))
    assert r.schedule() == 0
    spills, fills = r.s.take_kv_moves()
    assert len(fills) == 4 and [s for s, _ in fills] == [s for _, s in sp]
    assert len(spills) >= 1
    assert r.s.take_kv_moves() == ([], [])
    assert r.schedule() == 0 and r.s.take_kv_moves() == ([], [])
    assert r.s.abort(3)
    assert r.s.num_free_blocks == 8


def test_preempted_request_resumes_with_host_hits():
    r = _Run()
    r.add(1, list(range(100, 140)), max_tokens=60)
    r.add(2, list(range(200, 240)), max_tokens=60)
    spills, fills = r.drain()
    assert set(r.outs) == {1, 2} and len(r.outs[1][1]) == 60 and len(r.outs[2][1]) == 60
    assert r.s.total_preemptions >= 1
    assert spills and fills and r.s.host_hit_blocks == len(fills)
    assert r.s.num_free_blocks == 8


def test_reset_prefix_cache_clears_the_host_directory():
    r, _, _ = _a_then_x()
    assert r.s.num_host_cached == 3
    r.s.reset_prefix_cache()
    assert r.s.num_host_cached == 0 and r.s.num_cached_blocks == 0 and r.s.prefix_blocks(A) == []


def test_scheduler_refusals_and_the_default():
    with pytest.raises(ValueError):
        _runtime.Scheduler(dict(CFG, host_slots=-1))
    with pytest.raises(ValueError):
        _runtime.Scheduler(dict(CFG, host_cache_step_blocks=-1))
    with pytest.raises(ValueError):
        _runtime.Scheduler(dict(CFG, prefix_caching=False))
    r = _Run(host_slots=0)
    r.add(1, A)
    r.step()
    r.add(2, X)
    assert r.step() == (len(X), [], [])
    assert r.s.num_host_cached == 0 and r.s.prefix_blocks(A) == []  # evicted means gone, as ever


# ------------------------------------------------------------------ engine on the CPU
def _engine(**kw):
    from pilottai_amd.engine.engine import EngineConfig, LLMEngine

    cfg = dict(model="tiny", max_num_seqs=4, max_num_batched_tokens=128, max_model_len=256, num_kv_blocks=24)
    cfg.update(kw)
    return LLMEngine(EngineConfig(**cfg), device="cpu")


@pytest.mark.parametrize("kw", [
    dict(host_cache_gb=-1.0), dict(host_cache_blocks=-4), dict(host_cache_gb=float("nan")),
    dict(host_cache_blocks=8, host_cache_step_blocks=-1),
    dict(host_cache_gb=0.5, prefix_caching=False), dict(host_cache_blocks=8, prefix_caching=False),
    dict(host_cache_gb=0.5, async_steps=True), dict(host_cache_blocks=8, async_steps=True),
])
def test_engine_refusals(kw):
    with pytest.raises(ValueError):
        _engine(**kw)


def test_engine_refuses_tensor_parallel():
    from pilottai_amd.engine.engine import EngineConfig, LLMEngine

    with pytest.raises(ValueError, match="TP > 1"):
        LLMEngine._check_host_cache(EngineConfig(host_cache_gb=1.0), 2)
    LLMEngine._check_host_cache(EngineConfig(host_cache_gb=0.0), 2)  # off: nothing to refuse
    LLMEngine._check_host_cache(EngineConfig(host_cache_gb=0.0, prefix_caching=False, async_steps=True), 1)


def test_engine_cpu_serves_a_spilled_prompt_from_the_host():
    # partial-block reuse off on both engines: the tail donor of the first run is not spilled, so
    # with it on the device hit would compute 1 token where the host hit computes 7
    e = _engine(host_cache_blocks=64, partial_block_reuse=False)
    try:
        assert e.metrics()["host_cache_blocks"] == 64
        A_ids, first, again = spill_and_restore(e)
    finally:
        e.stop()
    # the same prompt as a device hit on an engine with a large pool: the same step shapes, so
    # on the CPU the same tokens
    big = _engine(num_kv_blocks=256, partial_block_reuse=False)
    try:
        miss = big.generate([A_ids], **GEN)[0]
        hit = big.generate([A_ids], **GEN)[0]
        assert hit.cached_prompt_tokens == 80 and big.metrics()["host_hit_blocks"] == 0
    finally:
        big.stop()
    assert first.token_ids == miss.token_ids
    assert again.token_ids == hit.token_ids


def test_engine_cpu_partial_reuse_behind_host_blocks():
    """After A is spilled, A[:39] + tail gets its two full blocks from the host and computes
    the rest: the donor of its third, partly shared block was not spilled."""
    e = _engine(host_cache_blocks=64, partial_block_reuse=True)
    try:
        A_ids = prompt_a(e.tok)
        e.generate([A_ids], **GEN)
        flood(e, A_ids)
        m0 = e.metrics()
        o = e.generate([A_ids[:39] + e.tok.encode(" and then another ending")], **GEN)[0]
        m1 = e.metrics()
        assert o.cached_prompt_tokens == 32
        assert m1["host_hit_blocks"] - m0["host_hit_blocks"] == 2
        assert m1["partial_hit_tokens"] == m0["partial_hit_tokens"]
    finally:
        e.stop()


def _scripted(e):
    tok = e.tok
    base = tok.encode("shared system prompt for every agent of the workflow, with the task text " * 2)
    outs = []
    for i in range(3):
        outs += e.generate([base + tok.encode(f" call {i} " * (1 + i))], **GEN)
    outs += e.generate([base + tok.encode(" call 0 ")], **GEN)
    keys = ("steps", "tokens", "sampled", "prompt_tokens", "prefix_cache_hit_tokens", "preemptions",
            "free_kv_blocks", "cached_kv_blocks", "partial_hit_tokens", "host_hit_blocks",
            "host_spilled_blocks", "host_evicted_blocks", "num_host_cached", "host_cache_blocks", "host_move_s")
    m = e.metrics()
    return [o.token_ids for o in outs], [o.cached_prompt_tokens for o in outs], {k: m[k] for k in keys}


def test_engine_off_is_the_engine_without_the_field():
    a = _engine()
    try:
        ra = _scripted(a)
    finally:
        a.stop()
    b = _engine(host_cache_gb=0.0)
    try:
        rb = _scripted(b)
        assert b._host_pool is None and b._host_stage is None
    finally:
        b.stop()
    assert ra == rb
    assert ra[2]["host_cache_blocks"] == 0 and ra[2]["host_spilled_blocks"] == 0 and ra[2]["host_move_s"] == 0.0


# ------------------------------------------------------------------ public surface
def test_llm_config_registry_http_and_cli():
    import asyncio

    from pilottai_amd.core.config import LLMConfig
    from pilottai_amd.engine import registry
    from pilottai_amd.engine.local_llm import LocalLLM, SchemaLLM
    from pilottai_amd.serving import http_server

    assert LLMConfig().host_cache_gb is None
    with pytest.raises(ValueError):
        LLMConfig(host_cache_gb=-1.0)
    gb = 1.0 / 1024  # 64 blocks of the tiny model's 16 KiB
    # sized in blocks: the registry compares the effective size, not the configuration field
    eng, plain = _engine(host_cache_blocks=64), _engine()
    saved = dict(registry._ENGINES)
    try:
        assert eng.host_cache_blocks == 64 and plain.host_cache_blocks == 0
        registry._ENGINES.clear()
        registry.register_engine("tiny", eng)
        assert LocalLLM(LLMConfig(model_name="tiny", host_cache_gb=gb)).engine is eng
        assert LocalLLM(LLMConfig(model_name="tiny")).engine is eng  # no preference stated
        with pytest.raises(ValueError, match="one engine per model"):
            LocalLLM(LLMConfig(model_name="tiny", host_cache_gb=2 * gb))
        registry.register_engine("tiny", plain)
        with pytest.raises(ValueError, match="one engine per model"):
            LocalLLM(LLMConfig(model_name="tiny", host_cache_gb=gb))
        assert LocalLLM(LLMConfig(model_name="tiny", host_cache_gb=0.0)).engine is plain
        seen = {}
        orig = registry.LLMEngine
        registry._ENGINES.clear()
        registry.LLMEngine = lambda cfg: seen.setdefault("cfg", cfg) and eng
        try:
            LocalLLM(LLMConfig(model_name="tiny", host_cache_gb=gb))
        finally:
            registry.LLMEngine = orig
        assert seen["cfg"].host_cache_gb == gb and seen["cfg"].model == "tiny"
        SchemaLLM(LLMConfig(model_name="tiny", provider="schema", host_cache_gb=gb))  # ignored

        def health(e):
            app = http_server.create_app(LocalLLM(LLMConfig(model_name="tiny"), engine=e), "tiny", engine=e)
            fn = next(r.endpoint for r in app.routes if getattr(r, "path", None) == "/health")
            return asyncio.run(fn())

        h = health(eng)
        assert h["host_cache_gb"] == gb and h["host_cached_blocks"] == 0
        assert h["host_hit_tokens"] == 0 and h["host_spilled_blocks"] == 0
        assert h["engine"]["host_cache_blocks"] == 64 and "host_cached_blocks" not in h["engine"]
        h = health(plain)
        assert h["host_cache_gb"] == 0.0 and h["engine"]["host_cache_blocks"] == 0
    finally:
        registry._ENGINES.clear()
        registry._ENGINES.update(saved)
        eng.stop()
        plain.stop()
    ap = http_server.build_parser()
    assert ap.parse_args([]).host_cache_gb == 0.0
    assert ap.parse_args(["--host-cache-gb", "64"]).host_cache_gb == 64.0
