"""Whole-block KV moves of the prefix cache's host tier on the GPU (csrc/ops/kv_pages.hip): gather
and scatter against the torch references, bit for bit. The copies are pure, so equality of the
bit patterns (int16 views: the caches hold NaN patterns too) is the right test."""
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC1  # a bf16 NaN pattern no kernel produces by itself
LAYERS, BLOCKS = 2, 6


def _caches(kv, seed):
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(-(1 << 15), 1 << 15, (LAYERS, BLOCKS, kv, 16, 16, 8), generator=g, dtype=torch.int16)
    v = torch.randint(-(1 << 15), 1 << 15, (LAYERS, BLOCKS, kv, 128, 16), generator=g, dtype=torch.int16)
    return k, v


def _dev(t, gpu):
    return t.to(gpu).view(torch.bfloat16)


def _bits(t):
    return t.view(torch.int16).cpu()


def _ids(lst, gpu):
    return torch.tensor(lst, dtype=torch.int32, device=gpu)


@pytest.mark.parametrize("kv", [8, 1])
def test_gather_matches_reference_bit_for_bit(gpu, kv):
    from pilottai_amd import ops
    from pilottai_amd.ops import reference as ref

    k, v = _caches(kv, seed=10 + kv)
    rec = LAYERS * 2 * kv * 2048
    ids = [4, 0, BLOCKS, 3, -1, 5]  # two of them out of range; 5 lies behind n
    n = 5
    stage = torch.full((6, rec), NAN_BITS, dtype=torch.int16)
    kd, vd, sd = _dev(k, gpu), _dev(v, gpu), _dev(stage, gpu)
    ops.kv_gather_blocks(kd, vd, _ids(ids, gpu), 0, sd)  # n = 0 touches nothing
    torch.cuda.synchronize()
    assert torch.equal(_bits(sd), stage) and torch.equal(_bits(kd), k) and torch.equal(_bits(vd), v)
    ops.kv_gather_blocks(kd, vd, _ids(ids, gpu), n, sd)
    torch.cuda.synchronize()
    want = stage.clone()
    ref.kv_gather_blocks(k.view(torch.bfloat16), v.view(torch.bfloat16), torch.tensor(ids, dtype=torch.int32), n,
                         want.view(torch.bfloat16))
    out = _bits(sd)
    assert torch.equal(out, want)
    # the layout, spelled out: [layer][K|V][KV][page]; skipped records and the one behind n keep the pattern
    r = out.view(6, LAYERS, 2, kv, 2048)
    for i, b in enumerate(ids[:n]):
        if 0 <= b < BLOCKS:
            assert torch.equal(r[i, :, 0], k[:, b].reshape(LAYERS, kv, 2048))
            assert torch.equal(r[i, :, 1], v[:, b].reshape(LAYERS, kv, 2048))
        else:
            assert bool((r[i] == NAN_BITS).all())
    assert bool((r[5] == NAN_BITS).all())
    assert torch.equal(_bits(kd), k) and torch.equal(_bits(vd), v)  # a gather reads the caches only


@pytest.mark.parametrize("kv", [8, 1])
def test_scatter_matches_reference_bit_for_bit(gpu, kv):
    from pilottai_amd import ops
    from pilottai_amd.ops import reference as ref

    k, v = _caches(kv, seed=20 + kv)
    rec = LAYERS * 2 * kv * 2048
    g = torch.Generator().manual_seed(30 + kv)
    stage = torch.randint(-(1 << 15), 1 << 15, (5, rec), generator=g, dtype=torch.int16)
    ids = [2, BLOCKS + 3, 5, -7, 1]  # 1 lies behind n
    n = 4
    for b in (2, 5):  # the destination blocks hold the pattern beforehand
        k[:, b] = NAN_BITS
        v[:, b] = NAN_BITS
    kd, vd, sd = _dev(k, gpu), _dev(v, gpu), _dev(stage, gpu)
    ops.kv_scatter_blocks(kd, vd, _ids(ids, gpu), 0, sd)
    torch.cuda.synchronize()
    assert torch.equal(_bits(kd), k) and torch.equal(_bits(vd), v)
    ops.kv_scatter_blocks(kd, vd, _ids(ids, gpu), n, sd)
    torch.cuda.synchronize()
    k_ref, v_ref = k.clone(), v.clone()
    ref.kv_scatter_blocks(k_ref.view(torch.bfloat16), v_ref.view(torch.bfloat16),
                          torch.tensor(ids, dtype=torch.int32), n, stage.view(torch.bfloat16))
    k_out, v_out = _bits(kd), _bits(vd)
    assert torch.equal(k_out, k_ref) and torch.equal(v_out, v_ref)
    r = stage.view(5, LAYERS, 2, kv, 2048)
    for i, b in ((0, 2), (2, 5)):
        assert torch.equal(k_out[:, b].reshape(LAYERS, kv, 2048), r[i, :, 0])
        assert torch.equal(v_out[:, b].reshape(LAYERS, kv, 2048), r[i, :, 1])
    for b in (0, 1, 3, 4):  # every byte outside the listed blocks is as it was
        assert torch.equal(k_out[:, b], k[:, b]) and torch.equal(v_out[:, b], v[:, b])
    assert torch.equal(_bits(sd), stage)


@pytest.mark.parametrize("kv", [8, 1])
def test_round_trip_through_pinned_host_memory(gpu, kv):
    """gather -> pinned host tensor -> scatter into other block ids: the path of a spill and a
    later fill, record by record on one stream."""
    from pilottai_amd import ops

    k, v = _caches(kv, seed=40 + kv)
    rec = LAYERS * 2 * kv * 2048
    src, dst = [0, 3, 4], [5, 1, 2]
    kd, vd = _dev(k, gpu), _dev(v, gpu)
    stage = torch.full((4, rec), NAN_BITS, dtype=torch.int16, device=gpu).view(torch.bfloat16)
    pool = torch.full((8, rec), NAN_BITS, dtype=torch.int16).view(torch.bfloat16).pin_memory()
    slots = [6, 0, 3]
    ops.kv_gather_blocks(kd, vd, _ids(src, gpu), 3, stage)
    for i, s in enumerate(slots):
        pool[s].copy_(stage[i], non_blocking=True)
    stage.view(torch.int16).fill_(NAN_BITS)
    for i, s in enumerate(slots):
        stage[i].copy_(pool[s], non_blocking=True)
    ops.kv_scatter_blocks(kd, vd, _ids(dst, gpu), 3, stage)
    torch.cuda.synchronize()
    k_out, v_out = _bits(kd), _bits(vd)
    for a, b in zip(src, dst):
        assert torch.equal(k_out[:, b], k[:, a]) and torch.equal(v_out[:, b], v[:, a])
    for a in src:
        assert torch.equal(k_out[:, a], k[:, a]) and torch.equal(v_out[:, a], v[:, a])
    untouched = [s for s in range(8) if s not in slots]
    assert bool((pool.view(torch.int16)[untouched] == NAN_BITS).all())


def test_bindings_refuse_what_would_leave_the_buffers(gpu):
    from pilottai_amd import ops

    k, v = _caches(1, seed=1)
    kd, vd = _dev(k, gpu), _dev(v, gpu)
    rec = LAYERS * 2 * 2048
    stage = torch.zeros(2, rec, dtype=torch.bfloat16, device=gpu)
    ids = _ids([0, 1, 2], gpu)
    for fn in (ops.kv_gather_blocks, ops.kv_scatter_blocks):
        with pytest.raises(RuntimeError):
            fn(kd, vd, ids, 3, stage)           # more records than the staging buffer has
        with pytest.raises(RuntimeError):
            fn(kd, vd, ids, 4, torch.zeros(4, rec, dtype=torch.bfloat16, device=gpu))  # n beyond the list
        with pytest.raises(RuntimeError):
            fn(kd, vd, ids, 1, torch.zeros(2, rec + 8, dtype=torch.bfloat16, device=gpu))  # another record size
        with pytest.raises(RuntimeError):
            fn(kd, vd, ids.to(torch.int64), 1, stage)
