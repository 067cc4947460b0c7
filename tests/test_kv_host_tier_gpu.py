"""Host KV tier on the GPU: the tiny-dims engine serves a prompt whose blocks were spilled to pinned
host memory, with step graphs and without. Counters and restored bytes are checked exactly; the
greedy tokens by the rule of tests/test_engine_gpu.py (token identity between runs is not
asserted: the split-K reductions are not run-to-run deterministic)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from host_tier_checks import GEN, flood, prompt_a, spill_and_restore  # noqa: E402

pytestmark = pytest.mark.gpu


def _engine(gpu, **kw):
    from pilottai_amd.engine.engine import EngineConfig, LLMEngine

    cfg = dict(model="tiny-gqa4", max_num_seqs=4, max_num_batched_tokens=128, max_model_len=256,
               num_kv_blocks=24, host_cache_blocks=64, token_buckets=[16, 128])
    cfg.update(kw)
    return LLMEngine(EngineConfig(**cfg), device=gpu)


def _check_greedy(engine, prompt, gen):
    """Each greedy token is the fp32 reference's argmax within 0.05 (tests/test_engine_gpu.py)."""
    ref = engine.model.reference_logits(prompt + gen[:-1])
    for i, tok in enumerate(gen):
        row = ref[len(prompt) - 1 + i]
        assert row[tok] >= row.max() - 0.05, (i, tok, int(row.argmax()), float(row[tok]), float(row.max()))


@pytest.mark.parametrize("use_graphs", [True, False])
def test_engine_serves_a_spilled_prompt_from_the_host(gpu, use_graphs):
    e = _engine(gpu, use_graphs=use_graphs)
    try:
        # page-locked at exactly its size: 64 records of 2 layers x (K, V) x 2 KV heads x 4 KiB
        assert e._host_pool.is_pinned() and e._host_pool.numel() * 2 == 64 * 2 * 2 * 2 * 4096
        assert e.metrics()["host_cache_gb"] == 64 * 32768 / 2**30
        A, first, again = spill_and_restore(e)
        assert len(again.token_ids) == GEN["max_tokens"]
        _check_greedy(e, A, first.token_ids)
        _check_greedy(e, A, again.token_ids)
        assert (e.metrics()["graph_replays"] > 0) == use_graphs
    finally:
        e.stop()


def test_engine_partial_reuse_behind_host_blocks(gpu):
    """After A is spilled, A[:39] + tail gets its two full blocks from the host: the donor of
    the third, partly shared block was not spilled, so 32 tokens are cached, not 39."""
    e = _engine(gpu, partial_block_reuse=True)
    try:
        A = prompt_a(e.tok)
        e.generate([A], **GEN)
        flood(e, A)
        m0 = e.metrics()
        p = A[:39] + e.tok.encode(" and then another ending")
        o = e.generate([p], **GEN)[0]
        m1 = e.metrics()
        assert o.cached_prompt_tokens == 32
        assert m1["host_hit_blocks"] - m0["host_hit_blocks"] == 2
        assert m1["partial_hit_tokens"] == m0["partial_hit_tokens"]
        _check_greedy(e, p, o.token_ids)
    finally:
        e.stop()
