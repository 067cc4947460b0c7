"""logit_bias and min_p on the GPU: the two HIP kernels (csrc/ops/logit_shaping.hip) against the
reference bit for bit, the sampler under the kernel's threshold, and the engine's shaped step
graphs end to end.

Both kernels do IEEE fp32 arithmetic the reference repeats operation by operation (one add and
one round-to-nearest-even bf16 conversion; one multiply and one add), so equality of the bits --
of the whole padded logit buffer, of tau -- is the right test for any finite inputs."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from logprob_checks import consistent as _consistent  # noqa: E402
from shaping_checks import forbidden_id, kept_set, minp_bound, minp_gaps, teacher_forced_bias  # noqa: E402

pytestmark = pytest.mark.gpu

# (V, row stride): the issue's two vocabularies (the engine's logits are contiguous: stride = V),
# a V that is no multiple of the 8-entry vector, and an odd stride (rows not 16-byte aligned)
SHAPES = [(1000, 1024), (128256, 128256), (1003, 1008), (1003, 1003)]
CANARY = 0x7fc1  # a NaN bit pattern in the padding columns


def _i32(x):
    return torch.as_tensor(x, dtype=torch.int32)


def _f32(x):
    return torch.as_tensor(x, dtype=torch.float32)


def _logits(rows, V, ld, seed):
    """[rows, ld] bf16: N(0, 4^2) in the first V columns, the NaN canary in the padding."""
    g = torch.Generator().manual_seed(seed)
    buf = torch.full((rows, ld), CANARY, dtype=torch.int16).view(torch.bfloat16)
    buf[:, :V] = (torch.randn(rows, V, generator=g) * 4).to(torch.bfloat16)
    return buf


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


# ---------------------------------------------------------------------------
# bias kernel
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("rows", [1, 3, 17])
@pytest.mark.parametrize("V,ld", SHAPES)
def test_bias_kernel_bit_for_bit(gpu, V, ld, rows):
    from pilottai_amd import ops

    buf = _logits(rows, V, ld, 10 + rows)
    rng = np.random.default_rng(V + rows)
    lists, forced = [], []
    for r in range(rows):
        kind = (r + rows) % 3  # 300 entries (with both edges and both out-of-range ids), 1 entry, none
        if kind == 1 or rows == 1:
            ids = [0, V - 1, -1, V] + rng.choice(np.arange(1, V - 1), 296, replace=False).tolist()
            rng.shuffle(ids)
        elif kind == 2:
            ids = [V - 1 if r % 2 else int(rng.integers(0, V))]
        else:
            ids = []
        lists.append([(int(t), float(np.float32(rng.uniform(-100, 100)))) for t in ids])
        forced.append(5 if r % 4 == 3 else -1)
    start = np.cumsum([0] + [len(x) for x in lists[:-1]]).tolist()
    flat = [e for x in lists for e in x] + [(3, 50.0)] * 4  # unused tail entries of the region
    args = (_i32(start), _i32([len(x) for x in lists]), _i32([t for t, _ in flat]), _f32([b for _, b in flat]),
            _i32(forced))
    want = buf.clone()
    ops.apply_logit_bias(want[:, :V], *args)
    got = buf.clone().to(gpu)
    view = got[:, :V]
    assert rows == 1 or view.stride(0) == ld
    ops.apply_logit_bias(view, *(a.to(gpu) for a in args))
    torch.cuda.synchronize()
    got = got.cpu()
    assert torch.equal(_bits(got), _bits(want)), (_bits(got) != _bits(want)).nonzero()[:8]
    assert bool((_bits(got)[:, V:] == CANARY).all())
    changed = (_bits(want) != _bits(buf)).any(dim=1).tolist()
    for r in range(rows):  # forced rows and empty lists are untouched, the others are not
        assert changed[r] == (forced[r] < 0 and len(lists[r]) > 0), r
    if rows == 17:
        assert sum(changed) >= 8 and not all(changed)


# ---------------------------------------------------------------------------
# min_p kernel
# ---------------------------------------------------------------------------

def _minp_case(rows, V, ld, seed):
    """Rows of every kind the issue lists; returns the tensors and the per-row kinds."""
    buf = _logits(rows, V, ld, seed)
    lg = buf[:, :V]
    words = (V + 31) // 32
    rng = np.random.default_rng(seed)
    classes = [np.zeros(words * 32, dtype=bool)]                 # class 0 allows nothing
    sub = rng.random(words * 32) < 0.5
    sub[V:] = True                                               # bits past V must not matter
    classes.append(sub)                                          # class 1: a random half
    kinds, mc, T, p, forced = [], [], [], [], []
    for r in range(rows):
        kind = ["free", "nomax", "nothing", "greedy", "off", "ties", "forced"][(r + rows) % 7]
        kinds.append(kind)
        cls, t, q, f = -1, 1.5, 0.3, -1
        if kind == "nomax":     # a class of its own that excludes the row's global maximum
            m = np.ones(words * 32, dtype=bool)
            top = int(lg[r].float().argmax())
            lg[r, top] = 40.0  # the one global maximum, whatever ties the random row has
            m[top] = False
            classes.append(m)
            cls = len(classes) - 1
        elif kind == "nothing":
            cls = 0
        elif kind == "greedy":
            t = 0.0
        elif kind == "off":
            q = 0.0
        elif kind == "ties":   # p = 1 keeps exactly the ties of the maximum: two of them, allowed
            a, b = (int(x) for x in np.flatnonzero(sub[:V])[[3, -1]])
            lg[r, a] = lg[r, b] = 48.0
            cls, q = 1, 1.0
        elif kind == "forced":
            f = 7
        mc.append(cls); T.append(t); p.append(q); forced.append(f)
    masks = torch.from_numpy(np.stack([np.packbits(c.reshape(-1, 32), axis=1, bitorder="little").view(np.uint32)[:, 0]
                                       for c in classes]).view(np.int32))
    assert masks.shape == (len(classes), words)
    from pilottai_amd.ops.reference import ln_min_p

    return buf, masks, kinds, _i32(mc), _f32(T), _f32(p), _f32([ln_min_p(x) for x in p]), _i32(forced)


@pytest.mark.parametrize("rows", [1, 3, 17])
@pytest.mark.parametrize("V,ld", SHAPES)
def test_minp_kernel_tau_bits(gpu, V, ld, rows):
    from pilottai_amd import ops
    from pilottai_amd.ops import reference as ref

    buf, masks, kinds, mc, T, p, L, forced = _minp_case(rows, V, ld, 20 + rows)
    lg = buf[:, :V]
    dev = buf.clone().to(gpu)
    view = dev[:, :V]
    targs = (T, p, L, forced, mc, masks)
    # (a) a step without a top-k / top-p pass: tau is written for every row
    want = ref.minp_threshold(lg, *targs)
    tau = torch.full((rows,), float("nan"), device=gpu)
    got = ops.minp_threshold(view, *(a.to(gpu) for a in targs), out=tau)
    torch.cuda.synchronize()
    assert got.data_ptr() == tau.data_ptr()
    assert torch.equal(_bits(got.cpu()), _bits(want)), (kinds, got.cpu(), want)
    for r, kind in enumerate(kinds):
        live = kind in ("free", "nomax", "ties")
        assert (float(want[r]) > -math.inf) == live, (r, kind)
        if kind == "ties":
            assert float(want[r]) == 48.0 and kept_set(lg[r], float(want[r])) == set(torch.nonzero(lg[r] == 48.0).flatten().tolist())
        if kind == "nomax":  # below the threshold a global maximum would have given
            assert float(want[r]) < float(lg[r].float().max()) + 1.5 * float(L[r])
    # (b) behind a top-k / top-p pass: incoming tau above tau_mp on even rows, below on odd rows
    m = torch.nan_to_num(want, neginf=0.0) - 1.5 * L  # the allowed maximum of the live rows
    tau_in = torch.where(torch.arange(rows) % 2 == 0, m - 0.5, m - 10.0)
    tau_in[rows // 2] = -math.inf if rows > 1 else tau_in[0]
    want2 = ref.minp_threshold(lg, *targs, tau_in)
    tau2 = tau_in.clone().to(gpu)
    ops.minp_threshold(view, *(a.to(gpu) for a in targs), tau=tau2)
    torch.cuda.synchronize()
    assert torch.equal(_bits(tau2.cpu()), _bits(want2)), (kinds, tau2.cpu(), want2)
    for r, kind in enumerate(kinds):
        if kind not in ("free", "nomax", "ties"):
            assert _bits(want2)[r] == _bits(tau_in)[r]          # kept the incoming value
        else:
            assert float(want2[r]) == max(float(tau_in[r]), float(want[r]))
    if rows == 17:
        live = [r for r, k in enumerate(kinds) if k in ("free", "nomax", "ties")]
        assert any(want2[r] == tau_in[r] and want2[r] > want[r] for r in live)   # top-k tau above tau_mp
        assert any(want2[r] == want[r] and want2[r] > tau_in[r] for r in live)   # and below
    assert torch.equal(_bits(dev.cpu()), _bits(buf))  # the logits are only read


def test_sampler_keeps_to_the_min_p_set(gpu):
    """64 (seed, offset) pairs on 3 rows at T = 1.5, p = 0.3: with the kernel's tau every sampled
    token lies in the reference kept set; without it the same pairs leave the set."""
    from pilottai_amd import ops
    from pilottai_amd.ops import reference as ref

    V, pairs = 1000, 64
    base = _logits(3, V, V, 31)
    n = 3 * pairs
    lg = base.repeat(pairs, 1).contiguous()
    T, p = _f32([1.5] * n), _f32([0.3] * n)
    L = _f32([ref.ln_min_p(0.3)] * n)
    mc, forced = _i32([-1] * n), _i32([-1] * n)
    masks = torch.zeros(1, (V + 31) // 32, dtype=torch.int32)
    seeds = torch.arange(n, dtype=torch.int64) // 3 * 7919 + 17
    offsets = _i32([(i // 3) * 5 + 1 for i in range(n)])
    tau_ref = ref.minp_threshold(base, T[:3], p[:3], L[:3], forced[:3], mc[:3], masks)
    kept = [kept_set(base[r], float(tau_ref[r])) for r in range(3)]
    assert all(0 < len(k) < V // 4 for k in kept)
    d = lambda t: t.to(gpu)  # noqa: E731
    tau = ops.minp_threshold(d(lg), d(T), d(p), d(L), d(forced), d(mc), d(masks))
    assert torch.equal(_bits(tau.cpu()), _bits(tau_ref.repeat(pairs)))
    with_tau = ops.sample(d(lg), d(T), d(mc), d(masks), d(seeds), d(offsets), d(forced), tau=tau).cpu().tolist()
    without = ops.sample(d(lg), d(T), d(mc), d(masks), d(seeds), d(offsets), d(forced)).cpu().tolist()
    assert all(t in kept[i % 3] for i, t in enumerate(with_tau))
    left = sum(t not in kept[i % 3] for i, t in enumerate(without))
    print(f"without tau {left} of {n} samples leave the kept sets (sizes {[len(k) for k in kept]})")
    assert left >= 1


# ---------------------------------------------------------------------------
# engine
# ---------------------------------------------------------------------------

SHAPE_KEY = (16, False, False, False, False, True)


@pytest.fixture(scope="module", params=[True, False], ids=["graphs", "eager"])
def engine(gpu, request):
    from pilottai_amd.engine.engine import EngineConfig, LLMEngine

    e = LLMEngine(EngineConfig(model="tiny-gqa4", max_num_seqs=16, max_num_batched_tokens=512, max_model_len=2048,
                               num_kv_blocks=512, token_buckets=[16, 64, 256], keep_graphs=True,
                               use_graphs=request.param), device=gpu)
    yield e
    e.stop()


@pytest.mark.parametrize("mode", ["greedy", "t0.8", "grammar"])
def test_engine_empty_shaping_changes_nothing(engine, mode):
    tok = engine.tok
    segs = engine.grammar.compile("agent.result_evaluation") if mode == "grammar" else None
    kw = dict(temperature=0.0 if mode == "greedy" else 0.8, max_tokens=400 if segs else 12,
              ignore_eos=segs is None, seed=4321, grammar=segs)
    batches = [[tok.encode("evaluate it")]] if segs else [[tok.encode("probe one"), tok.encode("second probe")]]
    keys = set(engine._graphs)
    plain = [o.token_ids for ps in batches for o in engine.generate(ps, **kw)]
    keys_plain = set(engine._graphs)
    empty = [o.token_ids for ps in batches for o in engine.generate(ps, logit_bias={}, min_p=0.0, **kw)]
    zeros = [o.token_ids for ps in batches for o in engine.generate(ps, logit_bias={5: 0, 9: 0.0}, min_p=0, **kw)]
    assert plain == empty == zeros
    assert set(engine._graphs) == keys_plain and all(len(k) < 6 for k in keys_plain - keys)


def test_engine_teacher_forced_bias_alone_mixed_and_graphs(engine):
    """Greedy with a -100 bias on every id the unbiased greedy reply used: the reply changes, and
    each of its tokens is the biased reference's argmax within the engine's logit tolerance; the
    same tokens among plain and penalised requests; the shaped graph is the plain one plus the
    two shaping kernels."""
    from pilottai_amd import ops
    from pilottai_amd.utils.tracing import graph_node_counts

    p = engine.tok.encode("probe one")
    kw = dict(temperature=0.0, max_tokens=24, ignore_eos=True)
    engine.bucket_hist.clear()
    plain = engine.generate([p], **kw)[0].token_ids
    bias = {t: -100 for t in set(plain)}
    out = engine.generate([p], logit_bias=bias, **kw)[0].token_ids
    assert len(out) == 24 and not set(out) & set(plain)
    teacher_forced_bias(engine, p, out, bias)
    if engine.use_graphs:
        assert SHAPE_KEY in engine._graphs and (16, False, False) in engine._graphs
        g_plain = engine._graphs[(16, False, False)]
        a, b = graph_node_counts(g_plain), graph_node_counts(engine._graphs[SHAPE_KEY])
        assert b["kernel"] == a["kernel"] + ops.LOGIT_BIAS_LAUNCHES + ops.MINP_THRESHOLD_LAUNCHES
        assert {k: v for k, v in b.items() if k != "kernel"} == {k: v for k, v in a.items() if k != "kernel"}
        n_graphs, captures = len(engine._graphs), engine.stats["graph_captures"]
        assert engine.generate([p], **kw)[0].token_ids == plain  # a plain request behind a shaped one
        assert engine._graphs[(16, False, False)] is g_plain and len(engine._graphs) == n_graphs
        assert engine.stats["graph_captures"] == captures
    # mixed: 3 + 7 prompt tokens, every step stays on the 16-token bucket
    res = {}
    engine.submit(p, lambda o: res.__setitem__(0, o), logit_bias=bias, **kw)
    for i in range(1, 8):
        extra = dict(presence_penalty=1.0, frequency_penalty=0.5) if i % 2 else {}
        engine.submit([1000 + i], lambda o, i=i: res.__setitem__(i, o), temperature=0.8, max_tokens=16,
                      ignore_eos=True, seed=100 + i, **extra)
    while len(res) < 8:
        assert engine.step() or len(res) == 8
    assert res[0].token_ids == out
    assert set(engine.bucket_hist) == {16}, engine.bucket_hist


def test_engine_teacher_forced_min_p(engine):
    """T = 1.5, min_p = 0.3: every sampled token's reference logit is within -T ln p (+ the
    engine's logit tolerance) of its row's reference maximum; without min_p the same seeds are not."""
    p = engine.tok.encode("probe one")
    T, mp = 1.5, 0.3
    bound = minp_bound(T, mp)
    worst, worst_plain = 0.0, 0.0
    for seed in (11, 12, 13, 14):
        kw = dict(temperature=T, max_tokens=16, ignore_eos=True, seed=seed)
        out = engine.generate([p], min_p=mp, **kw)[0].token_ids
        gaps = minp_gaps(engine, p, out)
        worst = max(worst, max(gaps))
        print(f"seed {seed}: min_p gaps max {max(gaps):.4f} (bound {bound:.4f})")
        assert len(out) == 16 and all(g <= bound for g in gaps), (seed, gaps)
        plain = engine.generate([p], **kw)[0].token_ids
        worst_plain = max(worst_plain, max(minp_gaps(engine, p, plain)))
    print(f"largest gap with min_p {worst:.4f}, without {worst_plain:.4f}, bound {bound:.4f}")
    assert worst_plain > bound


def test_engine_bias_with_logprobs(engine):
    tok = engine.tok
    p = tok.encode("probe one")
    plain = engine.generate([p], temperature=0.0, max_tokens=16, ignore_eos=True)[0].token_ids
    banned = {t: -100.0 for t in set(plain)}
    o = engine.generate([p], temperature=0.0, max_tokens=16, ignore_eos=True, logprobs=3, logit_bias=banned)[0]
    _consistent(engine, o, 3, greedy=True)
    assert not set(o.token_ids) & set(plain)
    assert not {i for _, top in o.logprobs for i, _ in top} & set(plain)  # the records see the biased logits
    # +100 on one id: it is sampled at T = 0.8 with logprob ~ 0 and heads every record
    o = engine.generate([p], temperature=0.8, max_tokens=8, ignore_eos=True, seed=3, logprobs=2, min_p=0.2,
                        logit_bias={4242: 100})[0]
    _consistent(engine, o, 2)
    assert o.token_ids == [4242] * 8
    assert all(lp > -1e-3 and top[0][0] == 4242 for lp, top in o.logprobs)
    segs = engine.grammar.compile("agent.result_evaluation")
    bad = forbidden_id(engine)
    g = engine.generate([tok.encode("evaluate it")], temperature=0.8, max_tokens=400, seed=9, grammar=segs,
                        logprobs=3, min_p=0.1, logit_bias={bad: 100})[0]
    assert g.finish_reason == "stop" and bad not in g.token_ids  # the grammar still decides
    json.loads(g.text)
    _consistent(engine, g, 3, segs=segs)


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


def test_http_logit_bias_and_min_p_on_the_gpu_engine(engine):
    import httpx

    from pilottai_amd.core.config import LLMConfig
    from pilottai_amd.engine.local_llm import LocalLLM
    from pilottai_amd.serving.http_server import create_app

    engine.start()
    try:
        backend = LocalLLM(LLMConfig(model_name="tiny-gqa4", max_tokens=24, retry_attempts=1), engine=engine)
        body = {"messages": [{"role": "user", "content": "hi"}], "temperature": 0.8, "seed": 5, "max_tokens": 24,
                "logprobs": True}
        ids = lambda r: [e["token_id"] for e in r.json()["choices"][0]["logprobs"]["content"]]  # noqa: E731
        with _Server(create_app(backend, "tiny-gqa4", engine=engine)) as url:
            plain = httpx.post(f"{url}/chat/completions", timeout=60, json=body)
            assert plain.status_code == 200, plain.text
            ban = ids(plain)[0]
            shaped = httpx.post(f"{url}/chat/completions", timeout=60,
                                json=dict(body, logit_bias={str(ban): -100}, min_p=0.05))
        assert shaped.status_code == 200, shaped.text
        print("plain:", ids(plain), "\nshaped:", ids(shaped))
        assert ban in ids(plain) and ban not in ids(shaped) and len(ids(shaped)) > 0
    finally:
        engine.stop()
