"""Partial-block prefix reuse on the GPU: the KV copy kernel against the torch reference, and the
tiny-dims engine's logits after a partial-block hit and after a same-step prefix share."""
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC1  # a bf16 NaN pattern no kernel produces by itself


def _caches(layers, blocks, kv, gpu, seed):
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(-(1 << 15), 1 << 15, (layers, blocks, kv, 16, 16, 8), generator=g, dtype=torch.int16)
    v = torch.randint(-(1 << 15), 1 << 15, (layers, blocks, kv, 128, 16), generator=g, dtype=torch.int16)
    return k, v


@pytest.mark.parametrize("kv", [8, 1])
def test_kv_copy_matches_reference_bit_for_bit(gpu, kv):
    from pilottai_amd import ops
    from pilottai_amd.ops import reference as ref

    layers, blocks = 2, 6
    k, v = _caches(layers, blocks, kv, gpu, seed=kv)
    copies = [(0, 3, 1), (1, 4, 8), (2, 5, 15)]
    for _, dst, _ in copies:  # everything the copy must not touch is NaN beforehand
        k[:, dst] = NAN_BITS
        v[:, dst] = NAN_BITS
    lst = torch.zeros(3 * 8, dtype=torch.int32)
    lst[:9] = torch.tensor(copies, dtype=torch.int32).reshape(-1)
    lst[9:12] = torch.tensor([0, 1, 16])  # behind the count: never read
    kd, vd = k.to(gpu).view(torch.bfloat16), v.to(gpu).view(torch.bfloat16)
    # a launch with count 0 changes nothing
    ops.kv_copy(kd, vd, torch.zeros(1, dtype=torch.int32, device=gpu), lst.to(gpu))
    torch.cuda.synchronize()
    assert torch.equal(kd.view(torch.int16).cpu(), k) and torch.equal(vd.view(torch.int16).cpu(), v)
    # three copies in one launch
    ops.kv_copy(kd, vd, torch.tensor([3], dtype=torch.int32, device=gpu), lst.to(gpu))
    torch.cuda.synchronize()
    k_ref, v_ref = k.clone(), v.clone()
    ref.kv_copy(k_ref, v_ref, torch.tensor([3], dtype=torch.int32), lst)
    k_out, v_out = kd.view(torch.int16).cpu(), vd.view(torch.int16).cpu()
    for src, dst, j in copies:
        assert torch.equal(k_out[:, dst, :, :, :j], k[:, src, :, :, :j])
        assert torch.equal(v_out[:, dst, :, :, :j], v[:, src, :, :, :j])
        assert bool((k_out[:, dst, :, :, j:] == NAN_BITS).all()) and bool((v_out[:, dst, :, :, j:] == NAN_BITS).all())
    assert torch.equal(k_out, k_ref) and torch.equal(v_out, v_ref)  # every other byte as it was


@pytest.fixture(scope="module")
def engine(gpu):
    from pilottai_amd.engine.engine import EngineConfig, LLMEngine

    e = LLMEngine(EngineConfig(model="tiny-gqa4", max_num_seqs=16, max_num_batched_tokens=512,
                               max_model_len=2048, num_kv_blocks=512, token_buckets=[16, 64, 256]),
                  device=gpu)
    yield e
    e.stop()


def _check_greedy(engine, prompt, gen):
    """Each greedy token is the fp32 reference's argmax within 0.05 (tests/test_engine_gpu.py)."""
    ref = engine.model.reference_logits(prompt + gen[:-1])
    for i, tok in enumerate(gen):
        row = ref[len(prompt) - 1 + i]
        assert row[tok] >= row.max() - 0.05, (i, tok, int(row.argmax()), float(row[tok]), float(row.max()))


def test_engine_partial_block_hit_matches_reference(engine):
    tok = engine.tok
    base = tok.encode("shared system prompt for every agent of the workflow, with the task text " * 4)
    tail = tok.encode(" but this call ends in its own way")
    c = 2 * 16 + 7
    assert len(base) >= 48 and tail[0] != base[c]  # the donor block is full
    gen = dict(temperature=0.0, max_tokens=6, ignore_eos=True)
    engine.generate([base], **gen)
    before = engine.metrics()
    p = base[:c] + tail
    o = engine.generate([p], **gen)[0]
    m = engine.metrics()
    assert m["partial_hit_tokens"] - before["partial_hit_tokens"] == 7
    assert o.cached_prompt_tokens == c
    _check_greedy(engine, p, o.token_ids)


def test_engine_same_step_share_matches_reference(engine):
    tok = engine.tok
    head = tok.encode("a different task text that two calls of one agent share from its first word on " * 3)[:40]
    p1, p2 = head + tok.encode(" analysis of the task"), head + tok.encode(" tool selection, please")
    assert p1[40] != p2[40]
    before = engine.metrics()
    o1, o2 = engine.generate([p1, p2], temperature=0.0, max_tokens=6, ignore_eos=True)
    m = engine.metrics()
    assert m["same_step_shares"] - before["same_step_shares"] == 1
    assert m["prefix_defers"] == before["prefix_defers"]
    assert o2.cached_prompt_tokens == 32
    _check_greedy(engine, p1, o1.token_ids)
    _check_greedy(engine, p2, o2.token_ids)
