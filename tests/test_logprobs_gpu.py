"""Per-token log-probabilities on the GPU: the HIP pass (csrc/ops/sampling.hip logprob_*_kernel)
against the fp64 reference, and the engine's logprob step graphs end to end.

Tolerance of the kernel tests: ids exactly (ordering and ties are integer comparisons on bf16
values), logprobs within 5e-4 absolute -- a chunked fp32 log-sum-exp over 4,096-entry chunks is
within 1e-6 of fp64 at these sizes and fast-math exp/log add a few 1e-6 relative, while the
smallest structural error the small-V cases produce (one dropped 16-byte vector at V = 264) moves
the normaliser by about 3e-2."""
import json
import math

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from logprob_checks import consistent as _consistent  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENTINEL = -7
TOL = 5e-4


def _masks(V, rows_of_ids):
    """class_masks [len, ceil(V / 32)] int32 with the given allowed ids per class (None = all)."""
    from pilottai_amd.ops.reference import pack_mask

    out = []
    for ids in rows_of_ids:
        m = np.ones(V, dtype=bool) if ids is None else np.zeros(V, dtype=bool)
        if ids is not None and len(ids):
            m[np.asarray(ids)] = True
        out.append(pack_mask(m))
    return torch.stack(out)


def _run(dev, logits, tokens, lp_n, forced, mask_class, class_masks):
    """The kernel on poisoned outputs / workspace, and the reference; returns both on the CPU."""
    from pilottai_amd import ops
    from pilottai_amd.ops import reference as ref

    rows, V = logits.shape
    i32 = lambda x: torch.as_tensor(x, dtype=torch.int32)  # noqa: E731
    tokens, lp_n, forced, mask_class = i32(tokens), i32(lp_n), i32(forced), i32(mask_class)
    lp = torch.full((rows,), NAN, dtype=torch.float32, device=dev)
    ids = torch.full((rows, 20), SENTINEL, dtype=torch.int32, device=dev)
    lps = torch.full((rows, 20), NAN, dtype=torch.float32, device=dev)
    ws = ops.token_logprobs_workspace(rows, V, dev).fill_(NAN)
    ops.token_logprobs(logits, tokens.to(dev), lp_n.to(dev), forced.to(dev), mask_class.to(dev),
                       class_masks.to(dev), out=(lp, ids, lps), workspace=ws)
    torch.cuda.synchronize()
    want = ref.token_logprobs(logits.cpu(), tokens, lp_n, forced, mask_class, class_masks)
    return (lp.cpu(), ids.cpu(), lps.cpu()), want, lp_n


def _close(a, b, what):
    assert not torch.isnan(a).any(), (what, a)
    assert torch.equal(torch.isinf(a), torch.isinf(b)), (what, a, b)
    fin = ~torch.isinf(b)
    err = float((a[fin].double() - b[fin].double()).abs().max()) if bool(fin.any()) else 0.0
    print(f"{what}: max |logprob error| = {err:.3e}")
    assert err <= TOL, (what, err)


def _check(got, want, lp_n):
    (lp, ids, lps), (r_lp, r_ids, r_lps) = got, want
    for r in range(lp.shape[0]):
        if int(lp_n[r]) < 0:  # skipped: the poison is still there
            assert math.isnan(float(lp[r])) and bool((ids[r] == SENTINEL).all()) and bool(torch.isnan(lps[r]).all()), r
            continue
        assert torch.equal(ids[r], r_ids[r]), (r, ids[r], r_ids[r])
        _close(lp[r:r + 1], r_lp[r:r + 1], f"row {r} chosen")
        _close(lps[r], r_lps[r], f"row {r} list")


def test_kernel_llama_vocab_masks_and_counts(gpu):
    from pilottai_amd import ops

    V, rows = 128256, 9
    g = torch.Generator().manual_seed(1)
    logits = (torch.randn(rows, V, generator=g) * 3).to(torch.bfloat16).to(gpu)
    four = [5, 4100, 70001, 128000]  # the last one lives in the last (partial) chunk
    cm = _masks(V, [None, four, [90000], []])
    #             none all  4-tok 1-tok empty skip none low-rank forced
    mask_class = [-1,  0,   1,    2,    3,    -1,  -1,  0,       -1]
    lp_n =       [20,  5,   20,   1,    5,    -1,  0,   5,       1]  # noqa: E222
    forced =     [-1,  -1,  -1,   -1,   -1,   -1,  -1,  -1,      77]  # noqa: E222
    temp = torch.tensor([0.0, 0.8, 0.8, 0.8, 0.0, 0.8, 1.3, 0.0, 0.8], device=gpu)
    tokens = ops.sample(logits, temp, torch.tensor(mask_class, dtype=torch.int32, device=gpu), cm.to(gpu),
                        torch.arange(rows, dtype=torch.int64, device=gpu) + 11,
                        torch.arange(rows, dtype=torch.int32, device=gpu) + 3,
                        torch.tensor(forced, dtype=torch.int32, device=gpu)).cpu()
    assert int(tokens[8]) == 77 and int(tokens[3]) == 90000 and int(tokens[4]) == 0 and int(tokens[2]) in four
    low = int(torch.argsort(logits[7].float(), descending=True, stable=True)[1000])  # allowed, far outside the top 5
    tokens[7] = low
    got, want, n = _run(gpu, logits, tokens, lp_n, forced, mask_class, cm)
    _check(got, want, n)
    lp, ids, lps = got
    assert low not in ids[7].tolist() and -20.0 < float(lp[7]) < float(lps[7, 4])
    assert float(lp[8]) == 0.0 and ids[8].tolist() == [77] + [-1] * 19 and float(lps[8, 0]) == 0.0
    assert float(lp[3]) == 0.0 and ids[3].tolist() == [90000] + [-1] * 19 and float(lps[3, 0]) == 0.0
    assert float(lp[4]) == -math.inf and ids[4].tolist() == [-1] * 20
    assert sorted(ids[2, :4].tolist()) == sorted(four) and ids[2, 4:].tolist() == [-1] * 16
    assert ids[6].tolist() == [-1] * 20 and math.isfinite(float(lp[6]))
    assert int(ids[0, 0]) == int(tokens[0])  # greedy: the chosen token leads its list
    assert abs(float(torch.exp(lps[0].double()).sum()) - float(torch.softmax(logits[0].double().cpu(), 0)
                                                              .topk(20).values.sum())) < 1e-3


@pytest.mark.parametrize("V,ld,rows", [(4104, 4104, 3), (264, 272, 3), (32000, 32000, 1), (4104, 4104, 17)])
def test_kernel_small_vocab_padding_and_row_counts(gpu, V, ld, rows):
    """A second chunk of 8 entries; a padded row whose padding would win every comparison; one
    and seventeen rows."""
    g = torch.Generator().manual_seed(V + rows)
    buf = torch.full((rows, ld), 30000.0, dtype=torch.bfloat16)
    buf[:, :V] = (torch.randn(rows, V, generator=g) * 3).to(torch.bfloat16)
    logits = buf.to(gpu)[:, :V]
    assert logits.stride(0) == ld
    cm = _masks(V, [None, [1, V - 1, V - 8]])
    mask_class = [(-1, 0, 1)[r % 3] for r in range(rows)]
    lp_n = [(20, 5, 20, 0, 1)[r % 5] for r in range(rows)]
    tokens = [int(V - 1 - 7 * r) if mask_class[r] != 1 else V - 8 for r in range(rows)]
    got, want, n = _run(gpu, logits, tokens, lp_n, [-1] * rows, mask_class, cm)
    _check(got, want, n)
    assert int(got[1].max()) < V


def test_kernel_ties_take_the_smallest_ids(gpu):
    """30 ids share the row's maximum, spread over chunks, waves and lanes: the 20 listed are
    exactly the 20 smallest, in ascending order."""
    V = 128256
    g = torch.Generator().manual_seed(5)
    row = (torch.randn(2, V, generator=g) * 2).to(torch.bfloat16)
    tied = [4099 * k for k in range(1, 31)]
    assert tied[-1] < V
    row[0, tied] = 17.0
    row[1, tied] = 17.0
    row[1, 3] = 17.0  # and one more tie in front of them all
    got, want, n = _run(gpu, row.to(gpu), [tied[25], tied[0]], [20, 20], [-1, -1], [-1, -1], _masks(V, [None]))
    _check(got, want, n)
    assert got[1][0].tolist() == tied[:20]
    assert got[1][1].tolist() == [3] + tied[:19]
    assert abs(float(got[0][0]) - float(got[2][0, 0])) < 1e-6  # the chosen (unlisted) tie has the same logprob


def test_kernel_short_list_wide_range_and_skipped_rows(gpu):
    V = 4104
    lin = torch.linspace(-80.0, 80.0, V).to(torch.bfloat16)
    g = torch.Generator().manual_seed(9)
    rnd = (torch.randn(V, generator=g) * 3).to(torch.bfloat16)
    logits = torch.stack([rnd, lin, rnd, lin.flip(0), rnd]).to(gpu)
    cm = _masks(V, [[7, 2050, 4100]])
    got, want, n = _run(gpu, logits, [2050, V - 1, 1, 0, 9], [20, 20, -1, 5, -1], [-1] * 5, [0, -1, -1, -1, 0], cm)
    _check(got, want, n)
    lp, ids, lps = got
    assert sorted(ids[0, :3].tolist()) == [7, 2050, 4100] and ids[0, 3:].tolist() == [-1] * 17
    assert bool(torch.isinf(lps[0, 3:]).all()) and bool(torch.isfinite(lps[0, :3]).all())
    assert bool(torch.isfinite(lps[1]).all()) and bool(torch.isfinite(lp[[1, 3]]).all())
    assert bool(torch.isfinite(lps[3, :5]).all())


# ---------------------------------------------------------------------------
# engine
# ---------------------------------------------------------------------------

def _make_engine(gpu, **kw):
    from pilottai_amd.engine.engine import EngineConfig, LLMEngine

    return LLMEngine(EngineConfig(model="tiny-gqa4", max_num_seqs=16, max_num_batched_tokens=512,
                                  max_model_len=2048, num_kv_blocks=512, token_buckets=[16, 64, 256], **kw),
                     device=gpu)


@pytest.fixture(scope="module")
def engine(gpu):
    e = _make_engine(gpu, keep_graphs=True)
    yield e
    e.stop()


def _prompts(tok):
    return [tok.encode("The orchestrator analyses a task and delegates it to worker agents " * k) for k in (1, 3)] \
        + [tok.encode("evaluate this result please")]


@pytest.mark.parametrize("mode", ["greedy", "t0.8", "grammar"])
def test_engine_tokens_do_not_depend_on_logprobs(engine, mode):
    """The same prompts and seed with and without logprobs=5 give identical tokens. The requests
    are sized so that every step stays on the 16-token bucket (free text: three short prompts
    together; grammar: one request at a time), where two runs are bit-identical; see
    test_engine_pipelined_loop_matches_serial."""
    tok = engine.tok
    segs = engine.grammar.compile("agent.result_evaluation") if mode == "grammar" else None
    kw = dict(temperature=0.0 if mode == "greedy" else 0.8, max_tokens=400 if segs else 12,
              ignore_eos=segs is None, seed=4321, grammar=segs)
    batches = [[tok.encode("evaluate it")], [tok.encode("judge this")]] if segs else \
        [[tok.encode("probe one"), tok.encode("second probe"), tok.encode("third")]]

    def run(**extra):
        return [o for ps in batches for o in engine.generate(ps, **kw, **extra)]

    engine.bucket_hist.clear()
    plain, asked = run(), run(logprobs=5)
    assert set(engine.bucket_hist) == {16}, engine.bucket_hist
    for a, b in zip(plain, asked):
        assert a.token_ids == b.token_ids and a.logprobs is None and a.cumulative_logprob is None
        _consistent(engine, b, 5, greedy=mode == "greedy", segs=segs)
        if segs:
            assert b.finish_reason == "stop" and b.forced_tokens > 0
            json.loads(b.text)
            assert any(lp == 0.0 for lp, _ in b.logprobs) and any(lp < 0.0 for lp, _ in b.logprobs)


def test_engine_logprobs_match_the_reference_forward(engine):
    """Free-text greedy logprobs are within 0.1 of log_softmax of the dense fp32 forward at the
    chosen token: twice the 0.05 logit tolerance tests/test_engine_gpu.py grants the engine
    against the same reference (one for the token's logit, one for the normaliser)."""
    tok = engine.tok
    prompts = _prompts(tok)[:2]
    outs = engine.generate(prompts, temperature=0.0, max_tokens=10, ignore_eos=True, logprobs=0)
    for p, o in zip(prompts, outs):
        ref = torch.log_softmax(engine.model.reference_logits(p + o.token_ids[:-1]).float(), dim=-1)
        for i, (t, (lp, top)) in enumerate(zip(o.token_ids, o.logprobs)):
            want = float(ref[len(p) - 1 + i, t])
            print(f"token {i}: engine {lp:.4f} reference {want:.4f}")
            assert top == [] and abs(lp - want) <= 0.1, (i, lp, want)


def test_engine_logprob_graphs_leave_the_plain_graphs_alone(engine):
    from pilottai_amd import ops
    from pilottai_amd.utils.tracing import graph_node_counts

    tok = engine.tok
    p = tok.encode("hi there")
    engine.generate([p], temperature=0.0, max_tokens=4, ignore_eos=True, logprobs=2)
    assert (16, False, False, True) in engine._graphs and (16, False, False) in engine._graphs
    plain = graph_node_counts(engine._graphs[(16, False, False)])
    with_lp = graph_node_counts(engine._graphs[(16, False, False, True)])
    assert with_lp["kernel"] == plain["kernel"] + ops.TOKEN_LOGPROBS_LAUNCHES
    assert {k: v for k, v in with_lp.items() if k != "kernel"} == {k: v for k, v in plain.items() if k != "kernel"}
    g_plain = engine._graphs[(16, False, False)]
    n_graphs, captures = len(engine._graphs), engine.stats["graph_captures"]
    o = engine.generate([p], temperature=0.0, max_tokens=4, ignore_eos=True)[0]
    assert o.logprobs is None
    assert engine._graphs[(16, False, False)] is g_plain and len(engine._graphs) == n_graphs
    assert engine.stats["graph_captures"] == captures
    assert all(len(k) == 3 or (len(k) == 4 and k[3] is True) for k in engine._graphs)


def test_engine_mixed_batch(engine):
    tok = engine.tok
    prompts = [tok.encode(f"request number {i} asks the agents for a plan") for i in range(8)]

    def run(ask):
        res = {}
        for i, p in enumerate(prompts):
            engine.submit(p, lambda o, i=i: res.__setitem__(i, o), temperature=0.8, max_tokens=10, ignore_eos=True,
                          seed=100 + i, logprobs=3 if (ask and i % 2 == 0) else -1)
        while len(res) < len(prompts):
            assert engine.step() or len(res) == len(prompts)
        return [res[i] for i in range(len(prompts))]

    nobody, half = run(False), run(True)
    for i, (a, b) in enumerate(zip(nobody, half)):
        assert a.token_ids == b.token_ids and a.logprobs is None
        if i % 2 == 0:
            _consistent(engine, b, 3)
        else:
            assert b.logprobs is None and b.cumulative_logprob is None


def test_engine_pipelined_loop_matches_serial(engine, gpu):
    """With async_steps=True the tokens and the logprobs equal the serial loop's, bit for bit.

    Every step of both engines stays on the 16-token bucket, i.e. on the packed decode kernels,
    whose results do not depend on what a row is batched with or on the run
    (tests/test_engine_gpu.py::test_sampling_batch_invariance). Larger steps would take the
    weight-streaming / tiled GEMMs, whose next-norm row statistics are summed with fp32 global
    atomics in arrival order (csrc/ops/gemm_stream.hip, gemm_mid.hip, gemm_pingpong.h `ss_out`),
    so their bf16 outputs can differ by an ulp between two runs of either loop; the CPU tier
    compares the loops exactly on such steps as well (tests/test_logprobs.py)."""
    tok = engine.tok
    free = dict(temperature=0.8, max_tokens=10, ignore_eos=True, seed=77, logprobs=4)
    gram = dict(temperature=0.8, max_tokens=400, logprobs=4)
    ps = [tok.encode("probe one"), tok.encode("second probe"), tok.encode("third")]
    assert sum(len(p) for p in ps) <= 16

    def run(e):
        segs = e.grammar.compile("agent.result_evaluation")
        e.bucket_hist.clear()
        outs = e.generate(ps, **free)
        for seed in (78, 79):  # one at a time: a jump-forward run stays inside the 16-token bucket
            outs += e.generate([tok.encode("judge it")], seed=seed, grammar=segs, **gram)
        assert set(e.bucket_hist) == {16}, e.bucket_hist
        return outs, segs

    serial, _ = run(engine)
    eng = _make_engine(gpu, async_steps=True)
    try:
        assert eng._async
        piped, segs2 = run(eng)
        for a, b in zip(serial, piped):
            assert a.token_ids == b.token_ids
            assert a.logprobs == b.logprobs and a.cumulative_logprob == b.cumulative_logprob
        for o in piped[3:]:
            assert o.finish_reason == "stop"
            _consistent(eng, o, 4, segs=segs2)
        assert eng.sched.spec_rows > 0 and eng.sched.inflight_steps == 0
    finally:
        eng.stop()


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


def test_http_logprobs_on_the_gpu_engine(engine):
    import httpx

    from pilottai_amd.core.config import LLMConfig
    from pilottai_amd.engine.local_llm import LocalLLM
    from pilottai_amd.serving.http_server import create_app

    engine.start()
    try:
        backend = LocalLLM(LLMConfig(model_name="tiny-gqa4", max_tokens=64, retry_attempts=1), engine=engine)
        with _Server(create_app(backend, "tiny-gqa4", engine=engine)) as url:
            r = httpx.post(f"{url}/chat/completions", timeout=60, json={
                "messages": [{"role": "user", "content": "evaluate result 3"}], "logprobs": True, "top_logprobs": 3,
                "temperature": 0.0,
                "response_format": {"type": "pilottai_schema", "schema": "orchestrator.result_evaluation"}})
        assert r.status_code == 200, r.text
        ch = r.json()["choices"][0]
        content = ch["logprobs"]["content"]
        assert "".join(e["token"] for e in content) == ch["message"]["content"]
        json.loads(ch["message"]["content"])
        for e in content:
            assert set(e) >= {"token", "logprob", "bytes", "top_logprobs"} and e["logprob"] <= 0.0
            assert bytes(e["bytes"]).decode("utf-8", errors="replace") == e["token"]
            assert 1 <= len(e["top_logprobs"]) <= 3
            assert all(set(t) >= {"token", "logprob", "bytes"} for t in e["top_logprobs"])
        assert any(e["logprob"] == 0.0 for e in content) and any(e["logprob"] < 0.0 for e in content)
    finally:
        engine.stop()
