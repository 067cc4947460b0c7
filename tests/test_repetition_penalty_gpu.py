"""Repetition penalty on the GPU: the HIP pass (csrc/ops/repetition.hip) against the reference,
bit for bit, and the engine's repetition step graphs end to end.

The pass is one correctly rounded fp32 product of two exactly representable inputs and one RNE
conversion per listed logit, which is what the CPU reference computes, so equality over the whole
padded logit buffer, the membership words and the list length is the right test for any r and any
logits. The list is compared as a set (the append order of one step's tokens is the atomics'
arrival order)."""
import math
import os
import sys
from collections import Counter

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from logprob_checks import consistent as _consistent  # noqa: E402
from penalty_checks import LOGIT_TOL  # noqa: E402
from repetition_checks import f32, i32, inv, members, teacher_forced_rep  # noqa: E402

pytestmark = pytest.mark.gpu

RS = [1.3, 0.5, 2.0, 1.25, 0.77, 1.05]
CANARY = 30000.0


def _logits(rows, V, ld, seed):
    """[rows, ld] bf16: random logits of both signs with some exact zeros, NaNs and infinities
    (columns 11, 7 and 3 among them) in the first V columns, CANARY in the padding."""
    g = torch.Generator().manual_seed(seed)
    buf = torch.full((rows, ld), CANARY, dtype=torch.bfloat16)
    x = torch.randn(rows, V, generator=g) * 8
    x[:, ::97] = 0.0
    x[:, 5::193] = -0.0
    x[:, 11::389] = float("nan")
    x[:, 7::401] = float("inf")
    x[:, 3::409] = float("-inf")
    buf[:, :V] = x.to(torch.bfloat16)
    return buf


def _fill(state, slot, toks, n_poison=None, tail=()):
    """Put a consistent history into a slot of a CPU state; optionally a garbage length and
    garbage entries behind the history."""
    seen, lst, n = state
    bits = seen.numpy().view(np.uint32)
    toks = list(dict.fromkeys(toks))
    for i, t in enumerate(toks):
        bits[slot, t >> 5] |= np.uint32(1 << (t & 31))
        lst[slot, i] = t
    for i, t in enumerate(tail):
        lst[slot, len(toks) + i] = t
    n[slot] = len(toks) if n_poison is None else n_poison


def _call(dev, buf, V, st_cpu, st_dev, rep_slot, rep_reset, rs, forced, lists, start=None, tok_pad=0):
    """One apply_repetition_penalty call on the device and on the CPU reference from the same
    inputs; compares the whole padded logit buffer and the whole state."""
    from pilottai_amd import ops

    rows = buf.shape[0]
    if start is None:
        start = np.cumsum([0] + [len(x) for x in lists[:-1]]).tolist()
    flat = ([t for x in lists for t in x] or [0]) + [7] * tok_pad
    args = (i32(rep_slot), i32(rep_reset), f32(rs), f32([inv(r) for r in rs]), i32(forced), i32(start),
            i32([len(x) for x in lists]), i32(flat))
    want = buf.clone()
    ops.apply_repetition_penalty(want[:, :V], st_cpu, *args)
    got = buf.to(dev)
    view = got[:, :V]
    assert rows == 1 or view.stride(0) == buf.shape[1]
    ops.apply_repetition_penalty(view, st_dev, *(a.to(dev) for a in args))
    torch.cuda.synchronize()
    got = got.cpu()
    same = (got.view(torch.int16) == want.view(torch.int16)) | (got.isnan() & want.isnan())
    assert bool(same.all()), (~same).nonzero()[:8]
    assert bool((got[:, V:] == CANARY).all())
    changed = int((want.view(torch.int16) != buf.view(torch.int16)).sum())
    seen, lst, n = (t.cpu() for t in st_dev)
    assert torch.equal(seen, st_cpu[0]) and torch.equal(n, st_cpu[2])
    for s in range(n.numel()):
        k = min(max(int(n[s]), 0), lst.shape[1])
        assert sorted(lst[s, :k].tolist()) == sorted(st_cpu[1][s, :k].tolist()), s
    return got, changed


def test_kernel_llama_vocab_padded_three_calls_with_growing_history(gpu):
    """V = 128,256 in rows of 128,320 with canaries; a recycled slot whose old contents are
    poisoned, a forced row, slot -1, out-of-range ids, ids sharing one membership word, a
    4,000-token delta with many duplicates, a row that sends nothing."""
    from pilottai_amd import ops

    V, ld, rows, slots, cap = 128256, 128320, 9, 10, 4096
    buf = _logits(rows, V, ld, 1)
    st_cpu = ops.repetition_state(slots, V, cap, "cpu")
    rng = np.random.default_rng(7)
    stale = rng.choice(V, 300, replace=False).tolist() + [V - 1, 0, 31, 32]
    _fill(st_cpu, 6, stale, n_poison=cap + 7, tail=[V + 1, -5, 1 << 30])  # row 2 takes this slot over: must vanish
    _fill(st_cpu, 5, [77, 9])                                              # row 1 is forced: must stay
    old = rng.choice(V, 40, replace=False).tolist()
    _fill(st_cpu, 2, old)                                                  # row 6 sends nothing: this alone
    st_dev = tuple(t.to(gpu) for t in st_cpu)
    #           plain forced reset  dup  edges word empty hist hist
    rep_slot = [-1,   5,     6,     0,   1,    3,   2,    4,   9]
    forced =   [-1,   77,    -1,    -1,  -1,   -1,  -1,   -1,  -1]  # noqa: E222
    rs = [1.5, 1.5] + RS + [1.3]
    fed = {s: set() for s in range(slots)}
    fed[5], fed[2] = {77, 9}, set(old)
    for call in range(3):
        lists = [[11, 12], [77, 77, 5], rng.integers(0, V, 50).tolist(), rng.integers(0, 700, 4000).tolist() + [11, 7, 3],
                 [0, V - 1, V - 1, V, -1, V + 31, 1 << 30, -(1 << 31), 31, 32],
                 [64 * 7 + b for b in range(32)] * 2 + [64 * 7 + 32 + 2 * call], [],
                 rng.integers(0, 300, 40).tolist(), rng.integers(V - 300, V, 40).tolist()]
        reset = [0, 1, 1 if call == 0 else 0, 0, 0, 0, 0, 0, 0]  # a forced row's reset flag is not acted on
        got, changed = _call(gpu, buf, V, st_cpu, st_dev, rep_slot, reset, rs, forced, lists)
        for r in (2, 3, 4, 5, 7, 8):
            fed[rep_slot[r]].update(t for t in lists[r] if 0 <= t < V)
        for s in range(slots):  # the state is the history, and nothing of the poison is left
            assert members(st_cpu, s) == fed[s], (call, s)
            assert int(st_cpu[2][s]) == len(fed[s])
        assert changed > 0
        assert torch.equal(got[:2].view(torch.int16), buf[:2].view(torch.int16))
        # NaN stays NaN and the infinities keep their sign, on the device too (a -ffast-math build)
        assert bool(got[3, 11].isnan()) and float(got[3, 7]) == math.inf and float(got[3, 3]) == -math.inf
    assert len(fed[0]) <= 700 and len(fed[3]) == 32 + 3 and fed[1] == {0, V - 1, 31, 32}


@pytest.mark.parametrize("rows", [1, 17])
def test_kernel_tail_word_delta_lengths_and_windows(gpu, rows):
    """V = 1,037 (33 membership words, the last 13 bits wide) in rows of 1,040; delta lengths 0, 1,
    255, 256, 257 around the 256-thread workgroup and 1,025 around its 4-deep unrolling; a delta
    window that reaches outside the token region is not applied."""
    from pilottai_amd import ops

    V, ld = 1037, 1040
    buf = _logits(rows, V, ld, 3 + rows)
    st_cpu = ops.repetition_state(rows + 1, V, 1100, "cpu")
    st_dev = tuple(t.to(gpu) for t in st_cpu)
    rng = np.random.default_rng(rows)
    slots = list(reversed(range(rows)))
    lens = [257, 0, 1, 255, 256, 1025]
    for call in range(2):
        lists = [rng.integers(0, V, lens[(r + call) % 6]).tolist() for r in range(rows)]
        lists[0] = lists[0] + [1036, 1024]
        _, changed = _call(gpu, buf, V, st_cpu, st_dev, slots, [0] * rows, [RS[r % 6] for r in range(rows)],
                           [-1] * rows, lists)
        assert changed > 0
    assert {1036, 1024} <= members(st_cpu, slots[0])
    # windows outside the region: start + n past the end, a negative start, a negative length
    before = [t.cpu() for t in st_dev]  # the device's own list order
    for start, n in ((3, 6), (-1, 2), (0, -4), (1 << 30, 1 << 30)):
        lists = [[1, 2, 3, 4, 5, 6, 7, 8]] + [[] for _ in range(rows - 1)]
        flat_n = [n] + [0] * (rows - 1)
        args = (i32([rows] + [-1] * (rows - 1)), i32([0] * rows), f32([1.5] * rows), f32([inv(1.5)] * rows),
                i32([-1] * rows), i32([start] + [0] * (rows - 1)), i32(flat_n), i32(lists[0]))
        got = buf.to(gpu)
        ops.apply_repetition_penalty(got[:, :V], st_dev, *(a.to(gpu) for a in args))
        torch.cuda.synchronize()
        assert torch.equal(got.cpu().view(torch.int16), buf.view(torch.int16))
        assert all(torch.equal(a.cpu(), b) for a, b in zip(st_dev, before))


# ---------------------------------------------------------------------------
# engine
# ---------------------------------------------------------------------------

REP_KEY = (16, False, False, False, False, False, True)
CFG = dict(model="tiny-gqa4", max_num_seqs=16, max_num_batched_tokens=512, max_model_len=2048, num_kv_blocks=512,
           token_buckets=[16, 64, 256])


@pytest.fixture(scope="module")
def engine(gpu):
    from pilottai_amd.engine.engine import EngineConfig, LLMEngine

    e = LLMEngine(EngineConfig(keep_graphs=True, **CFG), device=gpu)
    yield e
    e.stop()


@pytest.fixture(scope="module")
def eager(gpu):
    from pilottai_amd.engine.engine import EngineConfig, LLMEngine

    e = LLMEngine(EngineConfig(use_graphs=False, **CFG), device=gpu)
    yield e
    e.stop()


@pytest.mark.parametrize("mode", ["greedy", "t0.8", "grammar"])
def test_engine_r_one_changes_nothing(engine, eager, mode):
    tok = engine.tok
    outs = []
    for e in (engine, eager):
        segs = e.grammar.compile("agent.result_evaluation") if mode == "grammar" else None
        kw = dict(temperature=0.0 if mode == "greedy" else 0.8, max_tokens=400 if segs else 12,
                  ignore_eos=segs is None, seed=4321, grammar=segs)
        batches = [[tok.encode("evaluate it")]] if segs else [[tok.encode("probe one"), tok.encode("second probe")]]
        e.bucket_hist.clear()
        n_graphs, state = len(e._graphs), e._rep_state
        plain = [o.token_ids for ps in batches for o in e.generate(ps, **kw)]
        one = [o.token_ids for ps in batches for o in e.generate(ps, repetition_penalty=1.0, **kw)]
        assert set(e.bucket_hist) == {16}, e.bucket_hist
        assert plain == one and len(e._graphs) == n_graphs and e._rep_state is state
        outs.append(plain)
    assert outs[0] == outs[1]


def test_engine_teacher_forced_alone_mixed_graphs_on_and_off(engine, eager):
    """Greedy with r = 1.3: every chosen token is the penalised reference's argmax within the
    engine's logit tolerance; the same tokens alone and among seven other requests, with step
    graphs and without; the repetition graph is the plain graph plus one kernel; plain graphs
    stay untouched."""
    from pilottai_amd import ops
    from pilottai_amd.utils.tracing import graph_node_counts

    tok = engine.tok
    p = tok.encode("probe one")
    kw = dict(temperature=0.0, max_tokens=24, ignore_eos=True)
    engine.bucket_hist.clear()
    plain = engine.generate([p], **kw)[0].token_ids
    rep = engine.generate([p], repetition_penalty=1.3, **kw)[0].token_ids
    assert max(Counter(plain).values()) > 1 and rep != plain  # the plain reply repeats, the penalised one differs
    teacher_forced_rep(engine, p, rep, 1.3)
    assert eager.generate([p], repetition_penalty=1.3, **kw)[0].token_ids == rep
    assert eager.generate([p], **kw)[0].token_ids == plain and not eager._graphs
    # graphs
    assert REP_KEY in engine._graphs and (16, False, False) in engine._graphs and engine._rep_state is not None
    g_plain = engine._graphs[(16, False, False)]
    a, b = graph_node_counts(g_plain), graph_node_counts(engine._graphs[REP_KEY])
    assert b["kernel"] == a["kernel"] + ops.REPETITION_LAUNCHES
    assert {k: v for k, v in b.items() if k != "kernel"} == {k: v for k, v in a.items() if k != "kernel"}
    n_graphs, captures = len(engine._graphs), engine.stats["graph_captures"]
    assert engine.generate([p], **kw)[0].token_ids == plain  # a plain request after a penalised one
    assert engine._graphs[(16, False, False)] is g_plain and len(engine._graphs) == n_graphs
    assert engine.stats["graph_captures"] == captures
    # mixed batch: 3 + 7 prompt tokens, so every step stays on the 16-token bucket
    for e in (engine, eager):
        res = {}
        e.submit(p, lambda o: res.__setitem__(0, o), repetition_penalty=1.3, **kw)
        for i in range(1, 8):
            e.submit([1000 + i], lambda o, i=i: res.__setitem__(i, o), temperature=0.8, max_tokens=16,
                     ignore_eos=True, seed=100 + i, repetition_penalty=0.8 if i == 1 else 1.0)
        while len(res) < 8:
            assert e.step() or len(res) == 8
        assert res[0].token_ids == rep
        assert e.sched.num_free_penalty_slots == 16
    assert set(engine.bucket_hist) == {16}, engine.bucket_hist


def test_engine_with_additive_penalties_bias_and_logprobs(engine, eager):
    """All the logit controls at once, greedy, teacher-forced in the stated order (repetition,
    presence / frequency, logit_bias); logprobs are those of that distribution: a reference logit
    the engine matches within LOGIT_TOL is scaled by at most max(r, 1 / r) = 1.3, and a
    log-softmax moves by at most twice its inputs' largest error."""
    tok = engine.tok
    p = tok.encode("probe one")
    r, a, b = 1.3, 1.0, 0.5
    plain = engine.generate([p], temperature=0.0, max_tokens=16, ignore_eos=True)[0].token_ids
    bias = {plain[0]: -100.0, (plain[0] + 1) % 1000: 1.5}
    kw = dict(temperature=0.0, max_tokens=16, ignore_eos=True, logprobs=3, repetition_penalty=r, presence_penalty=a,
              frequency_penalty=b, logit_bias=bias)
    o = engine.generate([p], **kw)[0]
    assert plain[0] not in o.token_ids
    rows = teacher_forced_rep(engine, p, o.token_ids, r, a, b, bias)
    _consistent(engine, o, 3, greedy=True)
    ref_lp = torch.log_softmax(rows, dim=-1)
    for i, (t, (lp, top)) in enumerate(zip(o.token_ids, o.logprobs)):
        print(f"token {i}: logprob {lp:.4f}, reference {float(ref_lp[i, t]):.4f}")
        assert abs(lp - float(ref_lp[i, t])) <= 2 * 1.3 * LOGIT_TOL
    assert (16, False, False, True, True, True, True) in engine._graphs
    assert eager.generate([p], **kw)[0].token_ids == o.token_ids
    segs = engine.grammar.compile("agent.result_evaluation")
    gram = engine.generate([tok.encode("evaluate it")], temperature=0.8, max_tokens=400, seed=9, grammar=segs,
                           logprobs=3, repetition_penalty=1.5)[0]
    assert gram.finish_reason == "stop"
    _consistent(engine, gram, 3, segs=segs)


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


def test_http_repetition_penalty_on_the_gpu_engine(engine):
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
            rep = httpx.post(f"{url}/chat/completions", timeout=60, json=dict(body, repetition_penalty=1.3))
            bad = httpx.post(f"{url}/chat/completions", timeout=60, json=dict(body, repetition_penalty=0))
        assert plain.status_code == 200 and rep.status_code == 200, (plain.text, rep.text)
        assert bad.status_code == 400 and "repetition_penalty" in bad.text
        ids = lambda r: [e["token_id"] for e in r.json()["choices"][0]["logprobs"]["content"]]  # noqa: E731
        print("plain:", ids(plain), "\npenalised:", ids(rep))
        assert ids(rep) != ids(plain)  # on the parent the field is ignored: the same tokens
    finally:
        engine.stop()
