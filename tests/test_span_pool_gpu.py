"""Span pooling on the GPU: the HIP pass (csrc/ops/span_pool.hip) against ops.reference.span_pool.

The bound is zero: both sides add the same exactly converted bf16 values to an fp32 accumulator in
the same order, one correctly rounded add each, so every comparison here is on the bytes. Inputs
are seeded N(0, 1) bf16 values without subnormals, NaNs or infinities (the denormal mode is not
part of the contract). The accumulators sit between two canary rows, and every slot no segment
names is poisoned: all of them must keep their bits."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

POISON = np.array([0x7FC0BEEF], dtype=np.uint32).view(np.float32)[0]  # a NaN with a payload
SLOTS, CAP = 12, 16
DIMS = [4096, 264]  # 264: the last (only) column group is partly filled


@functools.lru_cache(maxsize=None)
def _rows(T, d):
    g = torch.Generator().manual_seed(1000 * T + d)
    x = torch.randn(T, d, generator=g).to(torch.bfloat16)
    a = x.float().abs()
    assert bool(torch.isfinite(x.float()).all()) and bool(((a == 0) | (a >= 2.0 ** -126)).all())
    return x


def _poisoned(d):
    return np.full((SLOTS + 2, d), POISON, dtype=np.float32)


def _launch(dev, hn, segs, n, big, cap=CAP):
    """One launch on the device over `big` (canary row, SLOTS accumulators, canary row), and the
    reference on a copy: (device bytes, reference bytes) of the whole of `big`."""
    from pilottai_amd import ops
    from pilottai_amd.ops import reference as ref

    words = np.full(4 * cap, -12345, dtype=np.int32)  # descriptors past the list are junk
    flat = np.asarray(segs, dtype=np.int32).reshape(-1)
    words[: len(flat)] = flat
    want = big.copy()
    ref.span_pool(hn, torch.tensor([n], dtype=torch.int32), torch.from_numpy(words), want[1:-1])
    dbig = torch.from_numpy(big.copy()).to(dev)
    ops.span_pool(hn.to(dev), torch.tensor([n], dtype=torch.int32, device=dev), torch.from_numpy(words).to(dev),
                  dbig[1:-1])
    torch.cuda.synchronize()
    return dbig.cpu().numpy(), want


def _same(got, want):
    assert got.tobytes() == want.tobytes(), np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:8]


@pytest.mark.parametrize("d", DIMS)
def test_segment_lengths_around_the_unroll_overlap_and_init_over_poison(gpu, d):
    """T = 300: lengths 1, 2, 3, 4, 5, 7, 8, 9 and 300, rows shared between segments (overlap),
    every segment with init = 1 over a NaN-poisoned accumulator; slots 9..11 are not named."""
    hn = _rows(300, d)
    segs = [(0, 300, 0, 1), (17, 1, 1, 1), (17, 2, 2, 1), (100, 3, 3, 1), (296, 4, 4, 1), (5, 5, 5, 1),
            (290, 7, 6, 1), (8, 8, 7, 1), (291, 9, 8, 1)]
    got, want = _launch(gpu, hn, segs, len(segs), _poisoned(d))
    _same(got, want)
    assert not np.isnan(got[1:10]).any() and np.isnan(got[10:]).all() and np.isnan(got[0]).all()
    # the reference is the sequential sum: check one value by hand
    acc = np.float32(0)
    for r in range(290, 297):
        acc = np.float32(acc + hn[r, 3].float().numpy())
    assert got[1 + 6, 3] == acc


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("T", [1, 17])
def test_small_steps(gpu, d, T):
    hn = _rows(T, d)
    segs = [(0, T, 3, 1), (T - 1, 1, 0, 1)] + ([(5, 9, 7, 1), (2, 8, 11, 1)] if T == 17 else [])
    got, want = _launch(gpu, hn, segs, len(segs), _poisoned(d))
    _same(got, want)
    assert not np.isnan(got[1 + 3]).any() and np.isnan(got[1 + 1]).all()


@pytest.mark.parametrize("d", DIMS)
def test_init_0_continues_a_known_accumulator(gpu, d):
    hn = _rows(17, d)
    big = _poisoned(d)
    g = torch.Generator().manual_seed(7)
    big[1 + 4] = torch.randn(d, generator=g).numpy()
    big[1 + 5] = big[1 + 4]
    got, want = _launch(gpu, hn, [(3, 9, 4, 0), (3, 9, 5, 1)], 2, big)
    _same(got, want)
    assert (got[1 + 4] != got[1 + 5]).any()  # the accumulator's old contents count when init = 0


@pytest.mark.parametrize("d", DIMS)
def test_one_launch_and_three_launches_give_the_same_bits(gpu, d):
    """The chunk-independence claim: 300 rows in one launch, or as three launches of 100 rows with
    init only on the first (a prompt prefilled in three steps), leave the same accumulator."""
    from pilottai_amd import ops

    hn = _rows(300, d)
    one, want = _launch(gpu, hn, [(0, 300, 2, 1)], 1, _poisoned(d))
    _same(one, want)
    dbig = torch.from_numpy(_poisoned(d)).to(gpu)
    for k in range(3):  # each step sees only its own 100 rows, as rows 0..99 of its hn
        words = torch.tensor([0, 100, 2, 1 if k == 0 else 0] + [-1] * (4 * CAP - 4), dtype=torch.int32, device=gpu)
        ops.span_pool(hn[100 * k:100 * (k + 1)].contiguous().to(gpu), torch.tensor([1], dtype=torch.int32, device=gpu),
                      words, dbig[1:-1])
    torch.cuda.synchronize()
    _same(dbig.cpu().numpy(), one)


@pytest.mark.parametrize("d", DIMS)
def test_count_0_count_at_capacity_and_descriptors_out_of_bounds(gpu, d):
    hn = _rows(17, d)
    # count 0: nothing is written, whatever the descriptors say
    got, want = _launch(gpu, hn, [(0, 17, 0, 1)], 0, _poisoned(d))
    _same(got, want)
    assert np.isnan(got).all()
    # count = capacity: the last descriptor of the list is served too
    segs = [(i, 2, i, 1) for i in range(4)]
    got, want = _launch(gpu, hn, segs, 4, _poisoned(d), cap=4)
    _same(got, want)
    assert not np.isnan(got[1:5]).any() and np.isnan(got[5:]).all()
    # rows or slot out of bounds, empty and negative lengths: skipped, between two served segments
    segs = [(0, 3, 0, 1), (-1, 3, 1, 1), (15, 3, 2, 1), (17, 1, 3, 1), (4, 0, 4, 1), (4, -2, 5, 1),
            (0, 3, -1, 1), (0, 3, SLOTS, 1), (0, 1 << 30, 6, 1), ((1 << 31) - 2, 4, 7, 1), (14, 3, 8, 1)]
    got, want = _launch(gpu, hn, segs, len(segs), _poisoned(d))
    _same(got, want)
    served = [1 + 0, 1 + 8]
    assert not np.isnan(got[served]).any()
    assert np.isnan(np.delete(got, served, axis=0)).all()


def test_a_row_length_that_is_no_multiple_of_8_raises(gpu):
    from pilottai_amd import _C, ops

    hn = torch.zeros(4, 260, dtype=torch.bfloat16, device=gpu)
    pool = torch.zeros(2, 260, dtype=torch.float32, device=gpu)
    n, segs = torch.zeros(1, dtype=torch.int32, device=gpu), torch.zeros(8, dtype=torch.int32, device=gpu)
    with pytest.raises(ValueError):
        ops.span_pool(hn, n, segs, pool)
    with pytest.raises(ValueError):  # the binding itself refuses too
        _C.span_pool(hn, n, segs, pool)
