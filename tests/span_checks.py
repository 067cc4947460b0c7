"""Shared bodies of the span-embedding tests (tests/test_span_embeddings.py on the CPU engine,
tests/test_span_embeddings_gpu.py on the GPU engine).

`SpanProbe` watches an eager engine from the outside: it wraps `ops.kernels.span_pool` to record
the final-norm rows and the segment words of every launch, replays them through
`ops.reference.span_pool` on a pool of its own, and -- whenever the scheduler hands finished span
requests to the engine -- checks that the engine's accumulator rows hold the replayed bits and
notes the rows of each finished request. `expected(rid)` is then the reference's span means, which
the delivered `span_embeddings` must equal bit for bit: rows, init flags, slots and the division
are all checked without a tolerance."""
import numpy as np
import torch

from pilottai_amd import ops
from pilottai_amd.ops import reference as ref


class _Sched:
    """The engine's scheduler with take_span_finishes observed."""

    def __init__(self, real, probe):
        self._real, self._probe = real, probe

    def __getattr__(self, name):
        return getattr(self._real, name)

    def take_span_finishes(self):
        fin = self._real.take_span_finishes()
        self._probe.on_finishes(fin)
        return fin


class SpanProbe:
    def __init__(self, engine):
        self.e = engine
        self.calls = []        # (hn [T, d] bf16 on the CPU, segment words in use) per launch
        self.pool = None       # the replayed accumulators
        self.sums = {}         # request id -> its slots' replayed sums at its finish
        self.slots = {}
        self.spans = {}

    def __enter__(self):
        self._orig = ops.kernels.span_pool
        self._sched = self.e.sched

        def wrapped(hn, n_seg, segs, pool):
            n = int(n_seg.reshape(-1)[0])
            self.calls.append((hn.detach().cpu().clone(), segs.detach().cpu().reshape(-1)[: 4 * n].clone()))
            if self.pool is None:
                self.pool = pool.detach().cpu().numpy().copy()  # the engine's rows before the first launch seen
            assert hn.shape[0] > 0 and pool.shape == self.pool.shape
            ref.span_pool(self.calls[-1][0], torch.tensor([n], dtype=torch.int32), self.calls[-1][1], self.pool)
            return self._orig(hn, n_seg, segs, pool)

        ops.kernels.span_pool = wrapped
        self.e.sched = _Sched(self._sched, self)
        return self

    def __exit__(self, *exc):
        ops.kernels.span_pool = self._orig
        self.e.sched = self._sched

    def on_finishes(self, fin):
        if not fin:
            return
        got = self.e._span_pool.detach().cpu().numpy()
        assert got.tobytes() == self.pool.tobytes(), "the engine's accumulators differ from the replayed segments"
        for rid, slots in fin:
            self.slots[rid] = list(slots)
            self.sums[rid] = self.pool[list(slots)].copy()

    def submit(self, ids, spans, outs):
        rid = self.e.submit(list(ids), lambda o: outs.__setitem__(o.request_id, o), embed=True, spans=list(spans),
                            temperature=0.0, max_tokens=1)
        self.spans[rid] = list(spans)
        return rid

    def expected(self, rid):
        lens = np.array([b - a for a, b in self.spans[rid]], dtype=np.float32)
        return self.sums[rid] / lens[:, None]

    def segments(self):
        """Every launch's (first_row, n_rows, slot, init) quadruples."""
        return [c[1].reshape(-1, 4).tolist() for c in self.calls]


def run_until(engine, outs, rids, limit=2000):
    for _ in range(limit):
        if all(r in outs for r in rids):
            return
        assert engine.step() or all(r in outs for r in rids), "the engine stalled"
    raise AssertionError("the requests did not finish")


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def dense_span_means(model, ids, spans, batch=32):
    """Span means of the dense forward (LlamaModel.hidden_states, the reference the whole-prompt
    embedding tests use): token t's final-norm state is the last-token state of the prefix
    ids[:t + 1] (a causal model), computed only for the tokens some span needs."""
    need = sorted({t for a, b in spans for t in range(a, b)})
    states = {}
    for i in range(0, len(need), batch):
        ts = need[i:i + batch]
        h = model.hidden_states([list(ids[:t + 1]) for t in ts], pooling="last").float().cpu()
        states.update(zip(ts, h))
    return torch.stack([torch.stack([states[t] for t in range(a, b)]).double().mean(0) for a, b in spans])


def rel_l2(got, want):
    got, want = torch.as_tensor(np.asarray(got)).double(), torch.as_tensor(np.asarray(want)).double()
    return ((got - want).norm(dim=-1) / want.norm(dim=-1)).tolist()
