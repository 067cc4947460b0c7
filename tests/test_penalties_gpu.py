"""Presence / frequency penalties on the GPU: the HIP pass (csrc/ops/penalties.hip) against the
reference, bit for bit, and the engine's penalty step graphs end to end.

The kernel cases use penalties that are multiples of 1/8 and |logit| <= 64: a bf16 logit of that
size is a multiple of 2^-14 below 2^7, the penalty (count <= 2,047) a multiple of 1/8 below 2^13,
so the fp32 difference is exact and the one bf16 rounding is the only rounding -- equality over
the whole padded logit buffer and the state is the right test. `distinct` is compared as a set
(the append order of one step's tokens is the atomics' arrival order)."""
import os
import sys
from collections import Counter

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from logprob_checks import consistent as _consistent  # noqa: E402
from penalty_checks import teacher_forced  # noqa: E402

pytestmark = pytest.mark.gpu

PENS = [(0.5, 0.25), (1.5, 0.0), (0.0, 2.0), (-0.5, -0.125), (2.0, 2.0), (-2.0, 1.875)]


def _i32(x):
    return torch.as_tensor(x, dtype=torch.int32)


def _logits(rows, V, ld, seed):
    """[rows, ld] bf16 with |logit| <= 64 in the first V columns and 30000.0 in the padding."""
    g = torch.Generator().manual_seed(seed)
    buf = torch.full((rows, ld), 30000.0, dtype=torch.bfloat16)
    buf[:, :V] = (torch.randn(rows, V, generator=g) * 16).clamp(-64, 64).to(torch.bfloat16)
    return buf


def _fill(state, slot, counter):
    """Put a consistent history into a slot of a CPU state."""
    counts, distinct, nd = state
    for i, (t, c) in enumerate(counter.items()):
        counts[slot, t] = c
        distinct[slot, i] = t
    nd[slot] = len(counter)


def _call(dev, buf, V, st_cpu, st_dev, pen_slot, pen_reset, pens, forced, lists):
    """One apply_penalties call on the device and on the CPU reference from the same inputs;
    compares the whole padded logit buffer and the whole state bit for bit."""
    from pilottai_amd import ops

    rows = buf.shape[0]
    start = np.cumsum([0] + [len(x) for x in lists[:-1]]).tolist()
    flat = [t for x in lists for t in x] or [0]
    args = (_i32(pen_slot), _i32(pen_reset), torch.tensor([p[0] for p in pens], dtype=torch.float32),
            torch.tensor([p[1] for p in pens], dtype=torch.float32), _i32(forced), _i32(start),
            _i32([len(x) for x in lists]), _i32(flat))
    want = buf.clone()
    ops.apply_penalties(want[:, :V], st_cpu, *args)
    got = buf.to(dev)
    view = got[:, :V]
    assert rows == 1 or view.stride(0) == buf.shape[1]
    ops.apply_penalties(view, st_dev, *(a.to(dev) for a in args))
    torch.cuda.synchronize()
    got = got.cpu()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), \
        (got.view(torch.int16) != want.view(torch.int16)).nonzero()[:8]
    changed = int((want.view(torch.int16) != buf.view(torch.int16)).sum())
    counts, distinct, nd = (t.cpu() for t in st_dev)
    assert torch.equal(counts, st_cpu[0]) and torch.equal(nd, st_cpu[2])
    for s in range(nd.numel()):
        n = int(nd[s])
        assert sorted(distinct[s, :n].tolist()) == sorted(st_cpu[1][s, :n].tolist()), s
        assert len(set(distinct[s, :n].tolist())) == n
    return got, changed


def test_kernel_llama_vocab_three_calls_with_growing_history(gpu):
    from pilottai_amd import ops

    V, rows, slots, cap = 128256, 9, 10, 512
    buf = _logits(rows, V, V, 1)
    st_cpu = ops.penalty_state(slots, V, cap, "cpu")
    rng = np.random.default_rng(7)
    stale = Counter({int(t): int(c) for t, c in zip(rng.choice(V, 300, replace=False), rng.integers(1, 2048, 300))})
    stale[V - 1] = 2047
    _fill(st_cpu, 6, stale)                        # row 2 takes this slot over: must vanish
    _fill(st_cpu, 5, Counter({77: 3, 9: 1}))       # row 1 is forced: must stay
    old = Counter({int(t): int(c) for t, c in zip(rng.choice(V, 40, replace=False), rng.integers(1, 9, 40))})
    _fill(st_cpu, 2, old)                          # row 6 sends nothing: penalised by this alone
    st_dev = tuple(t.to(gpu) for t in st_cpu)
    #           plain forced reset  x6   edges neg  empty hist hist
    pen_slot = [-1,   5,     6,     0,   1,    3,   2,    4,   9]
    forced =   [-1,   77,    -1,    -1,  -1,   -1,  -1,   -1,  -1]  # noqa: E222
    pens = [(1.0, 1.0), (1.0, 1.0), PENS[0], PENS[1], PENS[2], PENS[3], PENS[4], PENS[5], PENS[0]]
    fed = {s: Counter() for s in range(slots)}
    fed[5], fed[2] = Counter({77: 3, 9: 1}), Counter(old)
    for call in range(3):
        lists = [[11, 12], [77, 77, 5], rng.integers(0, V, 50).tolist(), [4242] * 6 + [17], [0, V - 1, V - 1],
                 rng.integers(0, 64, 100).tolist(), [], rng.integers(0, 300, 40).tolist(),
                 rng.integers(V - 300, V, 40).tolist()]
        reset = [0, 1, 1 if call == 0 else 0, 0, 0, 0, 0, 0, 0]  # a forced row's reset flag is not acted on
        got, changed = _call(gpu, buf, V, st_cpu, st_dev, pen_slot, reset, pens, forced, lists)
        for r in (2, 3, 4, 5, 7, 8):
            fed[pen_slot[r]].update(lists[r])
        for s in range(slots):  # the state is the history, and nothing of the poison is left
            assert {t: c for t, c in enumerate(st_cpu[0][s].tolist()) if c} == dict(fed[s]), (call, s)
        assert changed > 0
        assert torch.equal(got[:2].view(torch.int16), buf[:2].view(torch.int16))
    assert st_cpu[0][0, 4242] == 18 and st_cpu[0][1, V - 1] == 6 and int(st_cpu[2][6]) == len(fed[6])


def test_kernel_padded_rows_keep_their_padding(gpu):
    from pilottai_amd import ops

    V, ld, rows = 264, 272, 3
    buf = _logits(rows, V, ld, 2)
    st_cpu = ops.penalty_state(4, V, 32, "cpu")
    st_dev = tuple(t.to(gpu) for t in st_cpu)
    for call in range(2):
        got, changed = _call(gpu, buf, V, st_cpu, st_dev, [2, -1, 0], [0, 0, 0], [PENS[4], PENS[0], PENS[5]],
                             [-1, -1, -1], [[V - 1, 0, 263, 5, 5], [1, 2, 3], [V - 1, V - 2, 100]])
        assert changed > 0
        assert bool((got[:, V:] == 30000.0).all())


@pytest.mark.parametrize("rows", [1, 17])
def test_kernel_one_and_seventeen_rows(gpu, rows):
    from pilottai_amd import ops

    V = 4104
    buf = _logits(rows, V, V, 3 + rows)
    st_cpu = ops.penalty_state(rows, V, 600, "cpu")
    st_dev = tuple(t.to(gpu) for t in st_cpu)
    rng = np.random.default_rng(rows)
    slots = list(reversed(range(rows)))
    for call in range(2):
        lists = [rng.integers(0, V, 260 if r == 0 else 1 + r).tolist() for r in range(rows)]  # row 0: > 256 threads
        _, changed = _call(gpu, buf, V, st_cpu, st_dev, slots, [0] * rows, [PENS[r % 6] for r in range(rows)],
                           [-1] * rows, lists)
        assert changed > 0


# ---------------------------------------------------------------------------
# engine
# ---------------------------------------------------------------------------

PEN_KEY = (16, False, False, False, True)


@pytest.fixture(scope="module")
def engine(gpu):
    from pilottai_amd.engine.engine import EngineConfig, LLMEngine

    e = LLMEngine(EngineConfig(model="tiny-gqa4", max_num_seqs=16, max_num_batched_tokens=512, max_model_len=2048,
                               num_kv_blocks=512, token_buckets=[16, 64, 256], keep_graphs=True), device=gpu)
    yield e
    e.stop()


@pytest.mark.parametrize("mode", ["greedy", "t0.8", "grammar"])
def test_engine_zero_penalties_change_nothing(engine, mode):
    tok = engine.tok
    segs = engine.grammar.compile("agent.result_evaluation") if mode == "grammar" else None
    kw = dict(temperature=0.0 if mode == "greedy" else 0.8, max_tokens=400 if segs else 12,
              ignore_eos=segs is None, seed=4321, grammar=segs)
    batches = [[tok.encode("evaluate it")]] if segs else [[tok.encode("probe one"), tok.encode("second probe")]]
    engine.bucket_hist.clear()
    n_graphs, state = len(engine._graphs), engine._pen_state
    plain = [o.token_ids for ps in batches for o in engine.generate(ps, **kw)]
    zero = [o.token_ids for ps in batches for o in engine.generate(ps, presence_penalty=0.0, frequency_penalty=0, **kw)]
    assert set(engine.bucket_hist) == {16}, engine.bucket_hist
    assert plain == zero and len(engine._graphs) == n_graphs and engine._pen_state is state


def test_engine_teacher_forced_alone_mixed_and_graphs(engine):
    """Greedy with presence 1.5 / frequency 0.5: every chosen token is the penalised reference's
    argmax within the engine's logit tolerance; the same tokens alone and among seven unpenalised
    requests; the penalty graph is the plain graph plus one kernel; plain graphs stay untouched."""
    from pilottai_amd import ops
    from pilottai_amd.utils.tracing import graph_node_counts

    tok = engine.tok
    p = tok.encode("probe one")
    kw = dict(temperature=0.0, max_tokens=24, ignore_eos=True)
    engine.bucket_hist.clear()
    plain = engine.generate([p], **kw)[0].token_ids
    pen = engine.generate([p], presence_penalty=1.5, frequency_penalty=0.5, **kw)[0].token_ids
    assert max(Counter(plain).values()) > 1 and pen != plain  # the plain reply repeats, the penalised one differs
    teacher_forced(engine, p, pen, 1.5, 0.5)
    # graphs
    assert PEN_KEY in engine._graphs and (16, False, False) in engine._graphs and engine._pen_state is not None
    g_plain = engine._graphs[(16, False, False)]
    a, b = graph_node_counts(g_plain), graph_node_counts(engine._graphs[PEN_KEY])
    assert b["kernel"] == a["kernel"] + ops.PENALTY_LAUNCHES
    assert {k: v for k, v in b.items() if k != "kernel"} == {k: v for k, v in a.items() if k != "kernel"}
    n_graphs, captures = len(engine._graphs), engine.stats["graph_captures"]
    assert engine.generate([p], **kw)[0].token_ids == plain  # an unpenalised request after a penalised one
    assert engine._graphs[(16, False, False)] is g_plain and len(engine._graphs) == n_graphs
    assert engine.stats["graph_captures"] == captures
    # mixed batch: 3 + 7 prompt tokens, so every step stays on the 16-token bucket
    res = {}
    engine.submit(p, lambda o: res.__setitem__(0, o), presence_penalty=1.5, frequency_penalty=0.5, **kw)
    for i in range(1, 8):
        engine.submit([1000 + i], lambda o, i=i: res.__setitem__(i, o), temperature=0.8, max_tokens=16,
                      ignore_eos=True, seed=100 + i)
    while len(res) < 8:
        assert engine.step() or len(res) == 8
    assert res[0].token_ids == pen
    assert set(engine.bucket_hist) == {16}, engine.bucket_hist
    assert engine.sched.num_free_penalty_slots == 16


def test_engine_penalties_with_logprobs(engine):
    tok = engine.tok
    segs = engine.grammar.compile("agent.result_evaluation")
    free = engine.generate([tok.encode("probe one")], temperature=0.0, max_tokens=16, ignore_eos=True, logprobs=3,
                           presence_penalty=1.0, frequency_penalty=1.0)[0]
    _consistent(engine, free, 3, greedy=True)
    gram = engine.generate([tok.encode("evaluate it")], temperature=0.8, max_tokens=400, seed=9, grammar=segs,
                           logprobs=3, frequency_penalty=1.5)[0]
    assert gram.finish_reason == "stop"
    _consistent(engine, gram, 3, segs=segs)
    assert (16, False, False, True, True) in engine._graphs


class _Server:
    """The app on a uvicorn thread, as tests/test_http_serving.py runs it."""

    def __init__(self, app):
        import socket
        import threading

        import uvicorn

        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        self.port = s.getsockname()[1]
        s.close()
        self.server = uvicorn.Server(uvicorn.Config(app, host="127.0.0.1", port=self.port, log_level="error"))
        self.thread = threading.Thread(target=self.server.run, daemon=True)

    def __enter__(self):
        import time

        self.thread.start()
        t0 = time.time()
        while not self.server.started:
            assert time.time() - t0 < 30, "server did not start"
            time.sleep(0.02)
        return f"http://127.0.0.1:{self.port}/v1"

    def __exit__(self, *exc):
        self.server.should_exit = True
        self.thread.join(timeout=10)


def test_http_frequency_penalty_on_the_gpu_engine(engine):
    import httpx

    from pilottai_amd.core.config import LLMConfig
    from pilottai_amd.engine.local_llm import LocalLLM
    from pilottai_amd.serving.http_server import create_app

    engine.start()
    try:
        backend = LocalLLM(LLMConfig(model_name="tiny-gqa4", max_tokens=32, retry_attempts=1), engine=engine)
        body = {"messages": [{"role": "user", "content": "hi"}], "temperature": 0.0, "max_tokens": 32,
                "logprobs": True}
        with _Server(create_app(backend, "tiny-gqa4", engine=engine)) as url:
            plain = httpx.post(f"{url}/chat/completions", timeout=60, json=body)
            pen = httpx.post(f"{url}/chat/completions", timeout=60, json=dict(body, frequency_penalty=1.0))
        assert plain.status_code == 200 and pen.status_code == 200, (plain.text, pen.text)
        ids = lambda r: [e["token_id"] for e in r.json()["choices"][0]["logprobs"]["content"]]  # noqa: E731
        print("plain:", ids(plain), "\npenalised:", ids(pen))
        assert ids(pen) != ids(plain)
        assert max(Counter(ids(pen)).values()) < max(Counter(ids(plain)).values())  # the loop is broken
    finally:
        engine.stop()
