"""csrc/ops/spec_verify.hip against ops.reference.spec_verify: the outputs are integers, so the
comparison is exact."""
import numpy as np
import pytest
import torch

from pilottai_amd import ops
from pilottai_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

NONE = 0x7FFFFFFF
SENTINEL = -12345
PAD = 7  # sentinel words behind the rows: nothing beyond the rows may be written


def _case(rng, lens, nchunk, vocab=997, p_accept=0.7, p_forced=0.15):
    """Random partials for runs of the given lengths. Each run's draft follows the tokens its rows
    sample with probability p_accept per position, so all acceptance lengths occur."""
    rows = sum(lens)
    # few distinct keys: equal best keys are common, the smaller id must win
    pk = rng.integers(-3, 4, size=(rows, nchunk)).astype(np.float32) * 0.5
    pi = rng.integers(0, vocab, size=(rows, nchunk)).astype(np.int32)
    forced = np.where(rng.random(rows) < p_forced, rng.integers(0, vocab, size=rows), -1).astype(np.int32)
    run_first = np.concatenate([np.full(n, s) for n, s in zip(lens, np.cumsum([0] + lens[:-1]))]).astype(np.int32)
    run_len = np.concatenate([np.full(n, n) for n in lens]).astype(np.int32)
    # tokens laid out like a step: every row's input token sits at logit_rows[row], shuffled over a
    # longer id buffer so the indirection is exercised
    n_ids = rows + 5
    logit_rows = rng.permutation(n_ids)[:rows].astype(np.int32)
    ids = rng.integers(0, vocab, size=n_ids).astype(np.int32)
    t = lambda a: torch.from_numpy(a)
    toks, _ = ref.spec_verify(t(pk), t(pi), t(forced), t(ids), t(logit_rows), t(run_first), t(run_len))
    toks = toks.numpy()
    for r in range(1, rows):
        if run_first[r] != r and rng.random() < p_accept:  # row r's input = the token row r - 1 samples
            ids[logit_rows[r]] = toks[r - 1]
    return pk, pi, forced, ids, logit_rows, run_first, run_len


def _run(gpu, pk, pi, forced, ids, logit_rows, run_first, run_len):
    rows = pk.shape[0]
    host = [torch.from_numpy(np.ascontiguousarray(a)) for a in (pk, pi, forced, ids, logit_rows, run_first, run_len)]
    want_t, want_a = ref.spec_verify(*host)
    dev = [h.to(gpu) for h in host]
    out_t = torch.full((rows + PAD,), SENTINEL, dtype=torch.int32, device=gpu)
    out_a = torch.full((rows + PAD,), SENTINEL, dtype=torch.int32, device=gpu)
    ops.spec_verify(*dev, out_tokens=out_t, accept_len=out_a)
    torch.cuda.synchronize()
    got_t, got_a = out_t.cpu(), out_a.cpu()
    assert torch.equal(got_t[:rows], want_t), (got_t[:rows].tolist(), want_t.tolist())
    assert torch.equal(got_a[:rows], want_a), (got_a[:rows].tolist(), want_a.tolist())
    assert bool((got_t[rows:] == SENTINEL).all()) and bool((got_a[rows:] == SENTINEL).all())
    assert SENTINEL not in got_t[:rows].tolist() and SENTINEL not in got_a[:rows].tolist()  # every row written
    return got_t[:rows].tolist(), got_a[:rows].tolist()


def _split(rng, rows, only_ones=False):
    lens = []
    while sum(lens) < rows:
        lens.append(1 if only_ones else int(min(rng.integers(1, 10), rows - sum(lens))))
    return lens


@pytest.mark.parametrize("nchunk", [1, 32, 33, 65, 130])
@pytest.mark.parametrize("rows", [1, 9, 16, 40])
def test_random_runs_match_the_reference(gpu, nchunk, rows):
    rng = np.random.default_rng(1000 * nchunk + rows)
    _run(gpu, *_case(rng, _split(rng, rows), nchunk))
    _run(gpu, *_case(rng, _split(rng, rows, only_ones=True), nchunk))  # a launch of plain rows only
    if rows >= 9:
        _run(gpu, *_case(rng, [9] + _split(rng, rows - 9), nchunk))    # the longest run, then a mix


def test_every_run_length_in_one_launch(gpu):
    rng = np.random.default_rng(7)
    lens = list(range(1, 10))  # 45 rows
    _, acc = _run(gpu, *_case(rng, lens, 33, p_accept=1.0, p_forced=0.0))
    firsts = np.cumsum([0] + lens[:-1])
    assert [acc[f] for f in firsts] == lens  # all accepted: a + 1 = the run's length
    assert sum(acc) == sum(lens)             # 0 everywhere else


def _constructed(k, nchunk, best, draft, forced=None, vocab_keys=None):
    """One run of 1 + k rows whose row j samples best[j] (key 2.0 in one chunk, everything else
    lower) and whose draft tokens are draft[0:k]."""
    rows = k + 1
    pk = np.full((rows, nchunk), -1.0, dtype=np.float32)
    pi = np.arange(rows * nchunk, dtype=np.int32).reshape(rows, nchunk) + 5000
    for j in range(rows):
        pk[j, (3 * j) % nchunk] = 2.0
        pi[j, (3 * j) % nchunk] = best[j]
    fc = np.full(rows, -1, dtype=np.int32) if forced is None else np.asarray(forced, dtype=np.int32)
    ids = np.zeros(rows + 2, dtype=np.int32)
    ids[0] = 4242                      # the run's last real token
    ids[1:1 + k] = draft
    logit_rows = np.arange(rows, dtype=np.int32)
    return pk, pi, fc, ids, logit_rows, np.zeros(rows, dtype=np.int32), np.full(rows, rows, dtype=np.int32)


@pytest.mark.parametrize("nchunk", [1, 33])
def test_constructed_acceptance_lengths(gpu, nchunk):
    k = 8
    best = [100 + j for j in range(k + 1)]
    toks, acc = _run(gpu, *_constructed(k, nchunk, best, best[:k]))           # all accepted
    assert toks == best and acc == [k + 1] + [0] * k
    toks, acc = _run(gpu, *_constructed(k, nchunk, best, [9] * k))            # none accepted
    assert toks == best and acc == [1] + [0] * k
    for m in range(k):                                                        # first mismatch at each position
        draft = best[:k]
        draft[m] = 9
        _, acc = _run(gpu, *_constructed(k, nchunk, best, draft))
        assert acc == [m + 1] + [0] * k
    draft = best[:k]                                                          # a later match does not count
    draft[2] = 9
    assert _run(gpu, *_constructed(k, nchunk, best, draft))[1][0] == 3


def test_equal_best_keys_take_the_smaller_id(gpu):
    k, nchunk = 2, 130
    pk, pi, fc, ids, lr, rf, rl = _constructed(k, nchunk, [50, 60, 70], [20, 60])
    pk[0, 7] = pk[0, 129] = 2.0   # three chunks tie on row 0: ids 50 (chunk 0), 20 and 30
    pi[0, 7], pi[0, 129] = 30, 20
    toks, acc = _run(gpu, pk, pi, fc, ids, lr, rf, rl)
    assert toks[0] == 20 and acc[0] == 3  # the draft's 20 is accepted only if the smaller id won


def test_forced_rows(gpu):
    k = 3
    best = [100, 101, 102, 103]
    # row 1 is forced to its draft token (not what its partials say): accepted, and the run goes on
    toks, acc = _run(gpu, *_constructed(k, 32, best, [100, 555, 102], forced=[-1, 555, -1, -1]))
    assert toks == [100, 555, 102, 103] and acc[0] == 4
    # row 1 is forced to something else than its draft token: the forced token is the correction
    toks, acc = _run(gpu, *_constructed(k, 32, best, [100, 101, 102], forced=[-1, 555, -1, -1]))
    assert toks == [100, 555, 102, 103] and acc[0] == 2


def test_row_without_an_allowed_token_gives_zero(gpu):
    k = 2
    pk, pi, fc, ids, lr, rf, rl = _constructed(k, 65, [100, 101, 102], [100, 0])
    pk[1, :] = -np.inf
    pi[1, :] = NONE
    toks, acc = _run(gpu, pk, pi, fc, ids, lr, rf, rl)
    assert toks == [100, 0, 102] and acc[0] == 3  # token 0, which here is also the draft token


def test_draft_token_zero(gpu):
    toks, acc = _run(gpu, *_constructed(2, 32, [0, 0, 5], [0, 0]))
    assert toks == [0, 0, 5] and acc[0] == 3
    toks, acc = _run(gpu, *_constructed(2, 32, [0, 7, 5], [0, 0]))
    assert acc[0] == 2


def test_malformed_descriptors_stay_in_range(gpu):
    """Descriptors come from a host buffer: whatever they hold, every row is written, nothing else
    is, and the result is the reference's (a bad pair makes the row a run of its own)."""
    rng = np.random.default_rng(3)
    pk, pi, fc, ids, lr, rf, rl = _case(rng, [4, 4, 4], 33)
    rf[:] = [0, 0, 0, 0, 9, 3, -1, 4, 8, 8, 8, 1 << 30]
    rl[:] = [4, 4, 4, 4, 4, 2, 4, 100, 0, -5, 1 << 30, 1]
    lr[2], lr[10] = -7, 1 << 30
    _run(gpu, pk, pi, fc, ids, lr, rf, rl)
