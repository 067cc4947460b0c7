"""The host KV tier's engine scenario, shared by the CPU and the GPU tests: serve a prompt, flood the
device pool until the prompt's blocks live in the host tier only, serve it again."""
import torch

GEN = dict(temperature=0.0, max_tokens=6, ignore_eos=True)
A_TEXT = "the task text and the head of the prompt template that every call of one agent task starts with, "


def prompt_a(tok, n_tokens: int = 87):
    ids = tok.encode(A_TEXT * 4)
    assert len(ids) >= n_tokens
    return ids[:n_tokens]


def block_bytes(e, block: int):
    """The K and V pages of one block in every layer, as bit patterns."""
    return (e.kv.k[:, block].contiguous().view(torch.int16).cpu().clone(),
            e.kv.v[:, block].contiguous().view(torch.int16).cpu().clone())


def flood(e, A, tag: str = "f", limit: int = 40):
    """Distinct prompts, one at a time, until every block of A's chain is a host slot."""
    for i in range(limit):
        if all(t == "host" for t, _ in e.prefix_blocks(A)):
            return i
        e.generate([e.tok.encode(f"{tag}{i}: an unrelated prompt number {i} that shares no first block " * 2)[:100]],
                   temperature=0.0, max_tokens=2, ignore_eos=True)
    raise AssertionError(f"the flood did not move A to the host tier: {e.prefix_blocks(A)}")


def spill_and_restore(e, n_tokens: int = 87):
    """-> (A, tokens of the first run, output of the run served from the host tier). Asserts the
    counters and that the restored blocks hold the bytes the first run computed."""
    A = prompt_a(e.tok, n_tokens)
    full = len(A) // 16
    assert full >= 5 and len(A) % 16
    first = e.generate([A], **GEN)[0]
    assert first.cached_prompt_tokens == 0
    where = e.prefix_blocks(A)
    assert [t for t, _ in where] == ["device"] * full
    snap = [block_bytes(e, b) for _, b in where]
    flood(e, A)
    slots = e.prefix_blocks(A)
    assert [t for t, _ in slots] == ["host"] * full and len({s for _, s in slots}) == full
    m0 = e.metrics()
    assert m0["host_spilled_blocks"] >= full and m0["num_host_cached"] >= full
    again = e.generate([A], **GEN)[0]
    m1 = e.metrics()
    assert m1["host_hit_blocks"] - m0["host_hit_blocks"] == full
    assert again.cached_prompt_tokens == 16 * full
    assert m1["prefix_cache_hit_tokens"] - m0["prefix_cache_hit_tokens"] == 16 * full
    back = e.prefix_blocks(A)
    assert [t for t, _ in back] == ["device"] * full
    for (_, b), (k0, v0) in zip(back, snap):
        k1, v1 = block_bytes(e, b)
        assert torch.equal(k1, k0) and torch.equal(v1, v0), f"block {b} came back with other bytes"
    assert m1["host_move_s"] > 0.0
    return A, first, again
