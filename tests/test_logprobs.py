"""Per-token log-probabilities, CPU tier: the fp64 reference op, the scheduler's record plumbing
with fabricated records, the tiny CPU engine (serial and pipelined loop), the refusals, and the
HTTP / client surfaces."""
import asyncio
import json
import math
import os
import socket
import sys
import threading
import time

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from logprob_checks import consistent  # noqa: E402

from pilottai_amd import _runtime  # noqa: E402

W = 41  # 32-bit words per record: logprob, 20 ids, 20 logprobs


# ---------------------------------------------------------------------------
# reference op
# ---------------------------------------------------------------------------

def test_reference_matches_log_softmax_and_stable_sort():
    from pilottai_amd import ops
    from pilottai_amd.ops import reference as ref
    from pilottai_amd.ops.reference import pack_mask

    V, rows = 520, 7
    g = torch.Generator().manual_seed(3)
    logits = (torch.randn(rows, V, generator=g) * 3).to(torch.bfloat16)
    logits[1, [40, 300, 7, 511]] = 12.0  # ties at the top
    allowed = torch.ones(3, V, dtype=torch.bool)
    allowed[1] = False
    allowed[1, [9, 40, 300, 511, 100]] = True
    allowed[2] = False
    cm = torch.stack([pack_mask(a.numpy()) for a in allowed])
    mask_class = torch.tensor([-1, 1, 0, 1, 2, -1, 0], dtype=torch.int32)
    lp_n = torch.tensor([20, 20, 5, 0, 3, -1, 1], dtype=torch.int32)
    forced = torch.tensor([-1, -1, -1, -1, -1, -1, 33], dtype=torch.int32)
    tokens = torch.tensor([5, 100, 17, 9, 0, 1, 33], dtype=torch.int32)
    lp, ids, lps = ref.token_logprobs(logits, tokens, lp_n, forced, mask_class, cm)
    for r in range(rows):
        n = int(lp_n[r])
        if n < 0:
            assert math.isnan(float(lp[r])) and ids[r].tolist() == [-1] * 20
            continue
        if int(forced[r]) >= 0:
            assert float(lp[r]) == 0.0 and ids[r].tolist() == [33] + [-1] * 19 and float(lps[r, 0]) == 0.0
            continue
        ok = allowed[int(mask_class[r])] if int(mask_class[r]) >= 0 else torch.ones(V, dtype=torch.bool)
        if not bool(ok.any()):
            assert float(lp[r]) == -math.inf and ids[r].tolist() == [-1] * 20
            continue
        x = logits[r].double().masked_fill(~ok, -math.inf)
        want = torch.log_softmax(x, 0)
        vals, order = torch.sort(x, descending=True, stable=True)
        k = min(n, int(ok.sum()))
        assert ids[r, :k].tolist() == order[:k].tolist() and ids[r, k:].tolist() == [-1] * (20 - k)
        assert torch.allclose(lps[r, :k].double(), want[order[:k]], atol=1e-6)
        assert bool(torch.isinf(lps[r, k:]).all())
        assert abs(float(lp[r]) - float(want[int(tokens[r])])) < 1e-6
    assert ids[1, :4].tolist() == [40, 300, 511, 9]  # 12.0 x 3 by ascending id (7 is masked), then the rest
    # the op's CPU path is the reference and leaves rows that did not ask untouched
    out = (torch.full((rows,), 7.0), torch.full((rows, 20), -7, dtype=torch.int32), torch.full((rows, 20), 7.0))
    ops.token_logprobs(logits, tokens, lp_n, forced, mask_class, cm, out=out)
    assert float(out[0][5]) == 7.0 and out[1][5].tolist() == [-7] * 20
    assert torch.equal(out[1][[0, 1, 2, 3, 4, 6]], ids[[0, 1, 2, 3, 4, 6]])


# ---------------------------------------------------------------------------
# scheduler with fabricated records
# ---------------------------------------------------------------------------

def _fab(tok):
    """The record a test 'device' writes for sampled token `tok`: values that name the token."""
    lp = -(tok % 1000) / 8.0 - 0.125
    return lp, [(tok, lp), (tok + 1, lp - 1.0)]


def _record(lp, top):
    r = np.zeros(W, dtype=np.int32)
    f = r.view(np.float32)
    f[0] = lp
    r[1:21] = -1
    f[21:41] = -np.inf
    for i, (t, v) in enumerate(top):
        r[1 + i] = t
        f[21 + i] = v
    return r


def _drive(s, buf, L, masks=None, pick=lambda step, row: 7, with_records=True, max_steps=500, on_step=None):
    """Run the scheduler to completion with a host 'sampler'; returns every output tuple."""
    outs = []
    for step in range(max_steps):
        if s.schedule(buf.ctypes.data) == 0:
            break
        c = buf[L["counts"]:L["counts"] + 9]
        nsamp = int(c[2])
        lpn = buf[L["lp_n"]:L["lp_n"] + L["max_seqs"]]
        assert int(c[8]) == int((lpn[:nsamp] >= 0).sum()) and bool((lpn[nsamp:] == -1).all())
        sampled = np.zeros(max(1, nsamp), dtype=np.int32)
        recs = np.zeros((max(1, nsamp), W), dtype=np.int32)
        for r in range(nsamp):
            cls, f = int(buf[L["mask_class"] + r]), int(buf[L["forced"] + r])
            if f >= 0:
                t, rec = f, (0.0, [(f, 0.0)])  # what the kernel writes for a forced row
            else:
                t = int(np.nonzero(masks[cls])[0][(step + r) % int(masks[cls].sum())]) if cls >= 0 else pick(step, r)
                rec = _fab(t)
            sampled[r] = t
            recs[r] = _record(rec[0], rec[1][:max(0, int(lpn[r]))])
        if with_records:
            outs += s.commit(sampled.ctypes.data, nsamp, recs.ctypes.data)
        else:
            outs += s.commit(sampled.ctypes.data, nsamp)
        if on_step is not None:
            on_step(step)
    return outs


def _aligned(o, n):
    """Every record of output tuple `o` is the forced record or the fabricated one of its token."""
    toks, recs = o[1], o[10]
    assert recs is not None and len(recs) == len(toks)
    forced = 0
    for t, (lp, top) in zip(toks, recs):
        if lp == 0.0:
            assert top == [(t, 0.0)][:n]
            forced += 1
        else:
            flp, ftop = _fab(t)
            assert lp == flp and top == ftop[:n], (t, lp, top)
    return forced


def _sched(**kw):
    cfg = {"num_blocks": 64, "block_size": 16, "max_num_seqs": 8, "max_num_batched_tokens": 128,
           "max_model_len": 512, "prefix_caching": False, "eos_ids": [128009]}
    cfg.update(kw)
    s = _runtime.Scheduler(cfg)
    L = s.layout()
    return s, L, np.zeros(L["total"], dtype=np.int32)


def test_scheduler_layout_carries_lp_n_in_the_single_copy():
    s, L, buf = _sched()
    assert L["seeds"] < L["lp_n"] < L["block_table"]  # among the per-sequence arrays the engine copies
    assert L["lp_n"] + L["max_seqs"] <= L["block_table"] and L["counts"] + 9 <= L["n_items"]
    assert _runtime.Scheduler.LOGPROB_RECORD_WORDS == W


def test_scheduler_attaches_records_forced_and_jump_forward_entries():
    from pilottai_amd.engine.grammar import GrammarCompiler
    from pilottai_amd.engine.tokenizer import get_tokenizer

    tok = get_tokenizer()
    gc = GrammarCompiler(tok)
    segs = gc.compile("orchestrator.result_evaluation")
    masks = [np.asarray(r, dtype=bool) for r in gc.reg.rows]
    s, L, buf = _sched()
    s.add_request(1, list(range(100, 130)), 0.8, 200, 1, False, [], segs, logprobs=2)
    s.add_request(2, list(range(200, 220)), 0.8, 200, 2, False, [], segs)            # did not ask
    s.add_request(3, list(range(300, 310)), 0.8, 6, 3, True, [], None, logprobs=0)   # free text, chosen only
    s.add_request(4, list(range(400, 410)), 0.8, 200, 4, False, [], segs, 0, 1.0, False, False, 20)
    outs = {o[0]: o for o in _drive(s, buf, L, masks, pick=lambda step, r: 1000 + step)}
    assert set(outs) == {1, 2, 3, 4} and all(len(o) == 11 for o in outs.values())
    assert outs[2][10] is None
    for rid, n in ((1, 2), (4, 20)):
        o = outs[rid]
        assert o[2] == 0 and o[6] > 0  # stopped by the grammar, with jump-forward tokens
        json.loads(tok.decode(o[1]))
        assert _aligned(o, n) >= o[6]
        assert o[10][0] == (0.0, [(o[1][0], 0.0)])  # the reply starts with forced text (added at add_request)
    assert _aligned(outs[3], 0) == 0 and len(outs[3][1]) == 6 and all(top == [] for _, top in outs[3][10])


def test_scheduler_old_signatures_and_missing_records():
    s, L, buf = _sched()
    s.add_request(1, list(range(100, 120)), 0.0, 3, 7, True, [], None)          # the 8-argument form
    s.add_request(2, list(range(200, 220)), 0.0, 3, 7, True, [], None, logprobs=1)
    outs = {o[0]: o for o in _drive(s, buf, L, with_records=False)}              # commit(ptr, n)
    assert len(outs[1]) == 11 and outs[1][10] is None and outs[1][1] == [7, 7, 7]
    recs = outs[2][10]  # asked, but the steps carried no records: aligned placeholders
    assert len(recs) == 3 and all(math.isnan(lp) and top == [] for lp, top in recs)


def test_scheduler_abort_returns_the_partial_records():
    s, L, buf = _sched()
    s.add_request(1, list(range(100, 120)), 0.0, 50, 7, True, [], None, logprobs=2)

    def stop_after(step):
        if step == 3:
            assert s.abort(1)

    assert _drive(s, buf, L, pick=lambda step, r: 50 + step, on_step=stop_after) == []
    (o,) = s.drain_aborted()
    assert o[2] == 2 and o[1] == [50, 51, 52, 53] and _aligned(o, 2) == 0


def test_scheduler_preemption_keeps_records_aligned():
    s, L, buf = _sched(num_blocks=6, max_num_seqs=4, max_num_batched_tokens=256, max_model_len=256)
    s.add_request(1, list(range(40)), 0.0, 40, 1, True, [], None, logprobs=2)
    s.add_request(2, list(range(1000, 1030)), 0.0, 40, 1, True, [], None, logprobs=1)
    outs = {o[0]: o for o in _drive(s, buf, L, pick=lambda step, r: 2000 + 3 * step + r)}
    assert s.total_preemptions >= 1
    assert len(outs[1][1]) == 40 and len(outs[2][1]) == 40
    assert _aligned(outs[1], 2) == 0 and _aligned(outs[2], 1) == 0


# ---------------------------------------------------------------------------
# CPU engine
# ---------------------------------------------------------------------------

def _engine(async_steps=False, **kw):
    from pilottai_amd.engine.engine import EngineConfig, LLMEngine

    return LLMEngine(EngineConfig(model="tiny", max_num_seqs=8, max_num_batched_tokens=128, max_model_len=512,
                                  num_kv_blocks=128, use_graphs=False, async_steps=async_steps, **kw), device="cpu")


@pytest.fixture(scope="module", params=[False, True], ids=["serial", "pipelined"])
def engine(request):
    e = _engine(async_steps=request.param)
    assert e._async == request.param
    yield e
    e.stop()


def _prompts(tok):
    return [tok.encode("The orchestrator analyses a task and delegates it"), tok.encode("evaluate this result please")]


@pytest.mark.parametrize("mode", ["greedy", "t0.8", "grammar"])
def test_engine_tokens_do_not_depend_on_logprobs(engine, mode):
    tok = engine.tok
    segs = engine.grammar.compile("orchestrator.result_evaluation") if mode == "grammar" else None
    kw = dict(temperature=0.0 if mode == "greedy" else 0.8, max_tokens=200 if segs else 8,
              ignore_eos=segs is None, seed=4321, grammar=segs)
    plain = engine.generate(_prompts(tok), **kw)
    asked = engine.generate(_prompts(tok), logprobs=5, **kw)
    for a, b in zip(plain, asked):
        assert a.token_ids == b.token_ids and a.logprobs is None and a.cumulative_logprob is None
        consistent(engine, b, 5, greedy=mode == "greedy", segs=segs)
        if segs:
            assert b.finish_reason == "stop" and b.forced_tokens > 0
            assert any(lp == 0.0 for lp, _ in b.logprobs) and any(lp < 0.0 for lp, _ in b.logprobs)


def test_engine_logprobs_match_the_reference_forward(engine):
    tok = engine.tok
    p = _prompts(tok)[0]
    o = engine.generate([p], temperature=0.0, max_tokens=6, ignore_eos=True, logprobs=0)[0]
    ref = torch.log_softmax(engine.model.reference_logits(p + o.token_ids[:-1]).float(), dim=-1)
    for i, (t, (lp, top)) in enumerate(zip(o.token_ids, o.logprobs)):
        assert top == [] and abs(lp - float(ref[len(p) - 1 + i, t])) <= 0.1


def test_engine_mixed_batch(engine):
    tok = engine.tok
    prompts = [tok.encode(f"request number {i} asks for a plan") for i in range(8)]

    def run(ask):
        res = {}
        for i, p in enumerate(prompts):
            engine.submit(p, lambda o, i=i: res.__setitem__(i, o), temperature=0.8, max_tokens=6, ignore_eos=True,
                          seed=100 + i, logprobs=3 if (ask and i % 2 == 0) else -1)
        while len(res) < len(prompts):
            assert engine.step() or len(res) == len(prompts)
        return [res[i] for i in range(len(prompts))]

    nobody, half = run(False), run(True)
    for i, (a, b) in enumerate(zip(nobody, half)):
        assert a.token_ids == b.token_ids and a.logprobs is None
        if i % 2 == 0:
            consistent(engine, b, 3)
        else:
            assert b.logprobs is None and b.cumulative_logprob is None


def test_pipelined_loop_gives_the_serial_loop_s_logprobs():
    outs = []
    for a in (False, True):
        e = _engine(async_steps=a)
        try:
            segs = e.grammar.compile("orchestrator.result_evaluation")
            outs.append(e.generate(_prompts(e.tok), temperature=0.8, max_tokens=8, ignore_eos=True, seed=5, logprobs=4)
                        + e.generate(_prompts(e.tok), temperature=0.8, max_tokens=200, seed=6, grammar=segs, logprobs=4))
        finally:
            e.stop()
    for a, b in zip(*outs):
        assert a.token_ids == b.token_ids and a.logprobs == b.logprobs


def test_submit_refuses_bad_requests(engine):
    cb = lambda o: None  # noqa: E731
    for bad in (21, -2):
        with pytest.raises(ValueError):
            engine.submit([1, 2, 3], cb, logprobs=bad)
    for emb in (True, "last"):
        with pytest.raises(ValueError):
            engine.submit([1, 2, 3], cb, embed=emb, logprobs=0)
    assert engine._inbox.empty()


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _tp_worker(rank, world, port, out_path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    from pilottai_amd.engine.engine import EngineConfig, LLMEngine
    from pilottai_amd.parallel.comm import init_distributed, new_tp_groups

    init_distributed("gloo")
    e = LLMEngine(EngineConfig(model="tiny-gqa4", max_num_seqs=8, max_num_batched_tokens=128, max_model_len=512,
                               num_kv_blocks=96, use_graphs=False), device="cpu", tp=new_tp_groups(world))
    if rank != 0:
        e.follow()
        torch.distributed.destroy_process_group()
        return
    res = {}
    try:
        e.submit([1, 2, 3], lambda o: None, logprobs=0)
        res["refused"] = False
    except ValueError as err:
        res["refused"] = True
        res["message"] = str(err)
    o = e.generate([[1, 2, 3]], temperature=0.0, max_tokens=2, ignore_eos=True)[0]  # the engine still serves
    res["tokens"] = len(o.token_ids)
    res["logprobs"] = o.logprobs
    e.release_followers()
    torch.distributed.destroy_process_group()
    with open(out_path, "w") as f:
        json.dump(res, f)


def test_submit_refuses_logprobs_on_a_tp_engine(tmp_path):
    out = str(tmp_path / "tp.json")
    mp.start_processes(_tp_worker, args=(2, _free_port(), out), nprocs=2, join=True, start_method="spawn")
    res = json.load(open(out))
    assert res["refused"] and "TP" in res["message"] and res["tokens"] == 2 and res["logprobs"] is None


# ---------------------------------------------------------------------------
# HTTP and clients
# ---------------------------------------------------------------------------

class _Server:
    def __init__(self, app):
        import uvicorn

        self.port = _free_port()
        self.server = uvicorn.Server(uvicorn.Config(app, host="127.0.0.1", port=self.port, log_level="error"))
        self.thread = threading.Thread(target=self.server.run, daemon=True)

    def __enter__(self):
        self.thread.start()
        t0 = time.time()
        while not self.server.started:
            assert time.time() - t0 < 30, "server did not start"
            time.sleep(0.02)
        return f"http://127.0.0.1:{self.port}/v1"

    def __exit__(self, *exc):
        self.server.should_exit = True
        self.thread.join(timeout=10)


def test_http_logprobs_shape_errors_stream_and_client():
    import httpx

    from pilottai_amd.core.config import LLMConfig
    from pilottai_amd.engine.local_llm import LocalLLM, SchemaLLM, make_llm
    from pilottai_amd.serving.http_server import _wire_logprobs, create_app

    eng = _engine()
    eng.start()
    try:
        backend = LocalLLM(LLMConfig(model_name="tiny", max_tokens=96, retry_attempts=1), engine=eng)
        body = {"messages": [{"role": "user", "content": "task 1"}], "temperature": 0.0,
                "response_format": {"type": "pilottai_schema", "schema": "orchestrator.result_evaluation"}}
        with _Server(create_app(backend, "tiny", engine=eng)) as url:
            post = lambda **kw: httpx.post(f"{url}/chat/completions", json=dict(body, **kw), timeout=120)  # noqa: E731
            r = post(logprobs=True, top_logprobs=3)
            assert r.status_code == 200, r.text
            ch = r.json()["choices"][0]
            content = ch["logprobs"]["content"]
            assert "".join(e["token"] for e in content) == ch["message"]["content"]
            assert len(content) == r.json()["usage"]["completion_tokens"]
            for e in content:
                assert set(e) >= {"token", "logprob", "bytes", "top_logprobs"} and e["logprob"] <= 0.0
                assert bytes(e["bytes"]).decode("utf-8", errors="replace") == e["token"]
                assert 1 <= len(e["top_logprobs"]) <= 3
                assert [t["logprob"] for t in e["top_logprobs"]] == sorted((t["logprob"] for t in e["top_logprobs"]),
                                                                          reverse=True)
            assert any(e["logprob"] == 0.0 for e in content) and any(e["logprob"] < 0.0 for e in content)
            r0 = post(logprobs=True)  # no alternatives asked
            assert r0.status_code == 200 and all(e["top_logprobs"] == [] for e in r0.json()["choices"][0]["logprobs"]["content"])
            assert "logprobs" not in post().json()["choices"][0]  # replies that did not ask are unchanged
            assert post(logprobs=True, top_logprobs=21).status_code == 400
            assert post(logprobs=True, top_logprobs=-1).status_code == 400
            assert post(top_logprobs=2).status_code == 400
            assert post(logprobs=False, top_logprobs=2).status_code == 400
            lines = [ln[6:] for ln in post(logprobs=True, top_logprobs=1, stream=True).text.split("\n")
                     if ln.startswith("data: ") and ln != "data: [DONE]"]
            first, last = json.loads(lines[0]), json.loads(lines[-1])
            assert "".join(e["token"] for e in first["choices"][0]["logprobs"]["content"]) == \
                first["choices"][0]["delta"]["content"]
            assert "logprobs" not in last["choices"][0]

            async def go():
                llm = make_llm(LLMConfig(provider="openai", base_url=url, model_name="tiny", retry_attempts=1,
                                         timeout=120))
                asked = await llm.generate_response([{"role": "user", "content": "task 2"}], response_format={
                    "schema": "orchestrator.result_evaluation", "temperature": 0.0, "logprobs": 2})
                plain = await llm.generate_response([{"role": "user", "content": "task 2"}], response_format={
                    "schema": "orchestrator.result_evaluation", "temperature": 0.0})
                await llm.aclose()
                return asked, plain

            asked, plain = asyncio.run(go())
        assert plain["logprobs"] is None and asked["content"] == plain["content"]
        assert "".join(e["token"] for e in asked["logprobs"]) == asked["content"]
        assert all(len(e["top_logprobs"]) <= 2 and "token_id" in e for e in asked["logprobs"])
        # in process: LocalLLM returns the same shape
        direct = asyncio.run(backend.generate_response([{"role": "user", "content": "task 2"}], response_format={
            "schema": "orchestrator.result_evaluation", "temperature": 0.0, "logprobs": 2}))
        assert [e["token_id"] for e in direct["logprobs"]] == [e["token_id"] for e in asked["logprobs"]]
        assert set(direct["logprobs"][0]) == {"token", "token_id", "logprob", "bytes", "top_logprobs"}
    finally:
        eng.stop()
    # a backend without logprobs refuses; SchemaLLM ignores the field in process
    schema = SchemaLLM(seed=1)
    with _Server(create_app(schema, "schema-test")) as url:
        r = httpx.post(f"{url}/chat/completions", json=dict(body, logprobs=True, top_logprobs=1), timeout=60)
        assert r.status_code == 400 and "logprobs" in r.text
        assert httpx.post(f"{url}/chat/completions", json=body, timeout=60).status_code == 200
    rs = asyncio.run(schema.generate_response([{"role": "user", "content": "x"}], response_format={
        "schema": "orchestrator.result_evaluation", "logprobs": 3}))
    assert not rs.get("logprobs") and json.loads(rs["content"])
    wire = _wire_logprobs([{"token": "a", "token_id": 1, "logprob": -math.inf, "bytes": [97], "top_logprobs": []}])
    assert wire["content"][0]["logprob"] == -9999.0
