"""FP8 (e4m3) layer weights on the CPU reference paths: the quantiser's rule, the packed layouts
and their scale order, one weight set on every route of the model, and the public surface
(engine, registry, HTTP). The kernels are compared in tests/test_fp8_decode_gpu.py."""
import asyncio
import json
import os

import pytest
import torch

import fp8_checks as fc
from pilottai_amd import ops
from pilottai_amd.ops import reference as ref

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "fp8_unquantised_tokens.json")
F8 = torch.float8_e4m3fn


def _quantiser_input():
    w = fc.spread_weight(256, 512, seed=1)
    w[7] = 0  # an all-zero row
    w[9] = 0
    w[9, 3] = -0.37  # a row holding a single value
    return w


def test_quantiser_rule():
    w = _quantiser_input()
    q, s = ops.quantize_fp8_rows(w)
    assert q.dtype == F8 and s.dtype == torch.float32 and q.shape == w.shape and s.shape == (256,)
    assert torch.equal(torch.frexp(s)[0], torch.full_like(s, 0.5)), "scales are powers of two"
    assert s[7] == 1 and not q[7].float().any()
    amax = w.float().abs().amax(1)
    mx = q.float().abs().amax(1)[amax > 0]
    assert (mx > 224).all() and (mx <= 448).all()
    codes = q.view(torch.uint8)
    assert not ((codes & 0x7F) == 0x7F).any(), "NaN codes 0x7F / 0xFF"
    d = q.float() * s[:, None]
    assert torch.equal(d.bfloat16().float(), d), "q * s is exact in bf16"
    assert ((d - w.float()).abs() <= amax[:, None] / 14).all()
    normal = (w.float().abs() / s[:, None] >= 2.0 ** -6) & (w.float().abs() / s[:, None] <= 448)
    assert ((d - w.float()).abs()[normal] <= w.float().abs()[normal] / 16).all()
    assert q[9, 3].float() * s[9] == d[9, 3] and int((q[9].float() != 0).sum()) == 1
    # deterministic and idempotent
    q1, s1 = ops.quantize_fp8_rows(w)
    q2, s2 = ops.quantize_fp8_rows(ops.dequantize_fp8_rows(q, s))
    for qq, ss in ((q1, s1), (q2, s2)):
        assert torch.equal(qq.view(torch.uint8), codes) and torch.equal(ss, s)


def test_quantiser_saturates_and_rounds_to_nearest_even():
    # ties go to the even code; what is below half the smallest subnormal becomes 0
    w = torch.tensor([[448.0, 20.0, 21.0, -22.0, 23.0], [1.0, 0.5625, 0.6875, 2.0 ** -20, 0.0]]).bfloat16()
    q, s = ops.quantize_fp8_rows(w)
    assert s.tolist() == [1.0, 2.0 ** -8]
    assert q[0].float().tolist() == [448.0, 20.0, 20.0, -22.0, 24.0]  # 21, 23: ties to the even code
    assert q[1].float().tolist() == [256.0, 144.0, 176.0, 0.0, 0.0]
    # a row maximum that would round down to 224 takes the smaller scale and saturates instead
    w = torch.tensor([[225.0, 100.0, -7.5]]).bfloat16()
    q, s = ops.quantize_fp8_rows(w)
    assert s.item() == 0.5 and q.float().tolist() == [[448.0, 192.0, -15.0]]  # 450 saturates; 200 ties to even


PACKERS = {
    "plain": (ops.pack_decode_weight, ops.unpack_decode_weight, ops.pack_decode_weight_fp8,
              ops.unpack_decode_weight_fp8),
    "gate_up": (ops.pack_decode_gate_up, ops.unpack_decode_gate_up, ops.pack_decode_gate_up_fp8,
                ops.unpack_decode_gate_up_fp8),
    "rope": (ops.pack_decode_qkv_rope, ops.unpack_decode_qkv_rope, ops.pack_decode_qkv_rope_fp8,
             ops.unpack_decode_qkv_rope_fp8),
}


@pytest.mark.parametrize("kind", list(PACKERS))
def test_packers_invert_and_scales_follow_the_packed_columns(kind):
    pack, unpack, pack8, unpack8 = PACKERS[kind]
    w = fc.spread_weight(256, 96, seed=2)
    q, s = ops.quantize_fp8_rows(w)
    wp8, sp = pack8(w)
    assert wp8.dtype == F8 and wp8.shape == (16, 3, 64, 8) and sp.shape == (256,) and sp.dtype == torch.float32
    # lane 16 g + c of tile (t, s) holds q[16 t + c, 32 s + 8 g : + 8] of the packer's row order
    assert torch.equal(wp8.view(torch.uint8), pack(q.view(torch.uint8)))
    uq, us = unpack8(wp8, sp)
    assert torch.equal(uq.view(torch.uint8), q.view(torch.uint8)) and torch.equal(us, s)
    for a, b in zip(pack8((q, s)), (wp8, sp)):  # a quantised pair passes through
        assert torch.equal(a.view(torch.uint8) if a.dtype == F8 else a, b.view(torch.uint8) if b.dtype == F8 else b)
    # packed FP8 columns times packed scales == the bf16 pack of the dequantised matrix
    deq = ops.dequantize_fp8_rows(q, s)
    wp = pack(deq)
    T, S = wp8.shape[:2]
    got = wp8.float().view(T, S, 4, 16, 8) * sp.view(T, 1, 1, 16, 1)
    assert torch.equal(got.view(T, S, 64, 8), wp.float())
    assert torch.equal((uq.float() * us[:, None]).bfloat16(), unpack(wp))


def _x(M, K, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(M, K, generator=g).to(torch.bfloat16)


@pytest.mark.parametrize("epi,norm", [("plain", False), ("plain", True), ("resid", False), ("silu", True)])
def test_cpu_reference_equals_the_bf16_op_on_the_dequantised_pack(epi, norm):
    w = fc.spread_weight(256, 96, seed=4)
    wp, wp8, sp = fc.quantized_pair(w, "gate_up" if epi == "silu" else "plain")
    x = _x(9, 96)
    resid = _x(9, 256, seed=5) if epi == "resid" else None
    want = ops.decode_gemm(x, wp, epi, norm=norm, resid=resid)
    got = ops.decode_gemm_fp8(x, wp8, sp, epi, norm=norm, resid=resid)
    assert torch.equal(got, want)
    if epi == "resid":  # in place on the residual stream
        r2 = resid.clone()
        ops.decode_gemm_fp8(x, wp8, sp, "resid", resid=r2, out=r2)
        assert torch.equal(r2, want)


def test_cpu_reference_qkv_rope():
    H, KV, K, M = 4, 1, 96, 5
    w = fc.spread_weight((H + 2 * KV) * 128, K, seed=6, lo=-2.0, hi=0.0)
    wp, wp8, sp = fc.quantized_pair(w, "rope")
    x = _x(M, K)
    cs = ref.rope_cos_sin(64, 128, 10000.0)
    pos = torch.tensor([3, 9, 0, 17, 5], dtype=torch.int32)
    slots = torch.tensor([35, -1, 16, 49, 2], dtype=torch.int32)
    outs = []
    for f, args in ((ops.decode_qkv_rope, (wp,)), (ops.decode_qkv_rope_fp8, (wp8, sp))):
        q = torch.zeros(M, H, 128, dtype=torch.bfloat16)
        kc = torch.full((4, KV, 16, 16, 8), 7.0, dtype=torch.bfloat16)
        vc = torch.full((4, KV, 128, 16), 7.0, dtype=torch.bfloat16)
        f(x, *args, 1e-5, q, kc, vc, pos, slots, cs, H, KV)
        outs.append((q, kc, vc))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert (outs[0][1] != 7.0).any()


# -- model -----------------------------------------------------------------------------------------

def _tiny(**kw):
    from pilottai_amd.models.llama import LlamaModel, get_config

    return LlamaModel(get_config("tiny"), "cpu", **kw)


@pytest.fixture(scope="module")
def tiny_models():
    return _tiny(), _tiny(weight_quant="fp8"), _tiny(weight_quant="fp8", fp8_decode=False)


def test_tiny_model_holds_one_quantised_weight_set(tiny_models):
    plain, m8, m16 = tiny_models
    assert plain.weight_quant is None and not plain.fp8_decode
    assert m8.weight_quant == "fp8" and m8.fp8_decode and m16.weight_quant == "fp8" and not m16.fp8_decode
    packs = {"wqkv": (ops.pack_decode_qkv_rope, ops.pack_decode_qkv_rope_fp8, "ln1"),
             "wo": (ops.pack_decode_weight, ops.pack_decode_weight_fp8, None),
             "w13": (ops.pack_decode_gate_up, ops.pack_decode_gate_up_fp8, "ln2"),
             "w2": (ops.pack_decode_weight, ops.pack_decode_weight_fp8, None)}
    extra = 0
    for L0, L8, L16 in zip(plain.layers, m8.layers, m16.layers):
        assert not [k for k in L0 if k.endswith("8")] and not [k for k in L16 if k.endswith("8")]
        for kind, (pack, pack8, ln) in packs.items():
            folded = L0[kind] * L0[ln][None, :] if ln else L0[kind]
            q, s = ops.quantize_fp8_rows(folded)
            want = pack(ops.dequantize_fp8_rows(q, s))
            assert torch.equal(L8[kind + "_p"], want) and torch.equal(L16[kind + "_p"], want)
            assert not torch.equal(want, L0[kind + "_p"])  # it IS quantised
            wp8, sp = pack8((q, s))
            assert torch.equal(L8[kind + "_p8"].view(torch.uint8), wp8.view(torch.uint8))
            assert torch.equal(L8[kind + "_s8"], sp)
            # the kept row-major copy and dense() see the same weights (unit norm weights: exact)
            assert torch.equal(m8.dense(L8, kind), ops.dequantize_fp8_rows(q, s))
            extra += q.numel() + 4 * s.numel()
    assert m16.weight_bytes() == plain.weight_bytes()
    assert m8.weight_bytes() == plain.weight_bytes() + extra
    assert m8.lm_head_p.dtype == torch.bfloat16 and torch.equal(m8.lm_head_p, plain.lm_head_p)


@pytest.mark.parametrize("q_lens,ctx_lens", [([5], [5]), ([40], [40]), ([1, 1, 1], [7, 20, 33])])
def test_tiny_model_forward_is_identical_with_and_without_the_fp8_copy(tiny_models, q_lens, ctx_lens):
    plain, m8, m16 = tiny_models
    build = fc.make_step(m8, q_lens, ctx_lens)
    a, b = fc.run_step(m8, build), fc.run_step(m16, build)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert not torch.equal(a[0], fc.run_step(plain, build)[0])  # the quantised model is another model


def test_model_refusals():
    from pilottai_amd.parallel.comm import TPGroup

    with pytest.raises(ValueError, match="weight_quant"):
        _tiny(weight_quant="int4")
    with pytest.raises(ValueError, match="decode_pack"):
        _tiny(weight_quant="fp8", decode_pack=False)
    tp2 = TPGroup(None, 0, 2)
    with pytest.raises(ValueError, match="tensor-parallel"):
        _tiny(weight_quant="fp8", tp=tp2)


# -- engine ----------------------------------------------------------------------------------------

def _engine(**kw):
    from pilottai_amd.engine.engine import EngineConfig, LLMEngine

    return LLMEngine(EngineConfig(model="tiny", max_num_seqs=8, max_num_batched_tokens=128, max_model_len=512,
                                  num_kv_blocks=128, use_graphs=False, **kw), device="cpu")


@pytest.fixture(scope="module")
def engines():
    es = {"plain": _engine(), "fp8": _engine(weight_quant="fp8"),
          "fp8_bf16": _engine(weight_quant="fp8", fp8_decode=False)}
    yield es
    for e in es.values():
        e.stop()


def test_engine_tokens_identical_with_and_without_the_fp8_copy(engines):
    a = fc.request_tokens(engines["fp8"], with_prediction=True)
    b = fc.request_tokens(engines["fp8_bf16"], with_prediction=True)
    assert a == b
    m = engines["fp8"].metrics()
    assert m["weight_quant"] == "fp8" and m["fp8_decode"] is True
    m = engines["fp8_bf16"].metrics()
    assert m["weight_quant"] == "fp8" and m["fp8_decode"] is False


def test_unquantised_engine_is_unchanged(engines):
    """The default engine holds no FP8 entries and gives the tokens recorded from the commit
    before this option existed (tests/golden/fp8_unquantised_tokens.json; same seeds)."""
    e = engines["plain"]
    m = e.metrics()
    assert m["weight_quant"] is None and m["fp8_decode"] is False
    assert e.cfg.weight_quant is None and e.cfg.fp8_decode is True
    for L in e.model.layers:
        assert not [k for k in L if k.endswith("_p8") or k.endswith("_s8")]
    with open(GOLDEN) as f:
        want = json.load(f)
    got = fc.request_tokens(e)
    assert {k: got[k] for k in want} == want


def test_engine_refusals():
    from pilottai_amd.engine.engine import EngineConfig, LLMEngine
    from pilottai_amd.parallel.comm import TPGroup

    with pytest.raises(ValueError, match="weight_quant"):
        _engine(weight_quant="fp4")
    with pytest.raises(ValueError, match="decode_fused"):
        _engine(weight_quant="fp8", decode_fused=False)
    tp2 = TPGroup(None, 0, 2)
    with pytest.raises(ValueError, match="tensor-parallel"):
        LLMEngine(EngineConfig(model="tiny", num_kv_blocks=64, max_model_len=256, use_graphs=False,
                               weight_quant="fp8"), device="cpu", tp=tp2)


def test_registry_passes_weight_quant_and_refuses_another_setting(engines):
    from pilottai_amd.core.config import LLMConfig
    from pilottai_amd.engine import registry
    from pilottai_amd.engine.local_llm import LocalLLM, SchemaLLM

    assert LLMConfig().weight_quant is None
    saved = dict(registry._ENGINES)
    try:
        registry._ENGINES.clear()
        registry.register_engine("tiny", engines["fp8"])
        assert LocalLLM(LLMConfig(model_name="tiny", weight_quant="fp8")).engine is engines["fp8"]
        assert LocalLLM(LLMConfig(model_name="tiny")).engine is engines["fp8"]  # no preference stated
        registry.register_engine("tiny", engines["plain"])
        with pytest.raises(ValueError, match="one engine per model"):
            LocalLLM(LLMConfig(model_name="tiny", weight_quant="fp8"))
        seen = {}
        orig = registry.LLMEngine
        registry._ENGINES.clear()
        registry.LLMEngine = lambda cfg: seen.setdefault("cfg", cfg) and engines["fp8"]
        try:
            LocalLLM(LLMConfig(model_name="tiny", weight_quant="fp8"))
        finally:
            registry.LLMEngine = orig
        assert seen["cfg"].weight_quant == "fp8" and seen["cfg"].model == "tiny"
        SchemaLLM(LLMConfig(model_name="tiny", provider="schema", weight_quant="fp8"))  # ignored
    finally:
        registry._ENGINES.clear()
        registry._ENGINES.update(saved)


def test_http_reports_the_quantisation_and_the_cli_accepts_the_flags(engines):
    from pilottai_amd.core.config import LLMConfig
    from pilottai_amd.engine.local_llm import LocalLLM
    from pilottai_amd.serving import http_server

    def call(app, path):
        fn = next(r.endpoint for r in app.routes if getattr(r, "path", None) == path)
        return asyncio.run(fn())

    for key, wq, f8 in (("fp8", "fp8", True), ("fp8_bf16", "fp8", False), ("plain", None, False)):
        eng = engines[key]
        app = http_server.create_app(LocalLLM(LLMConfig(model_name="tiny"), engine=eng), "tiny", engine=eng)
        h = call(app, "/health")
        assert h["engine"]["weight_quant"] == wq and h["engine"]["fp8_decode"] is f8
        entry = call(app, "/v1/models")["data"][0]
        assert entry["id"] == "tiny" and entry["weight_quant"] == wq and entry["fp8_decode"] is f8
        json.dumps(h), json.dumps(entry)
    ap = http_server.build_parser()
    a = ap.parse_args([])
    assert a.weight_quant is None and a.fp8_decode is True
    a = ap.parse_args(["--weight-quant", "fp8", "--no-fp8-decode"])
    assert a.weight_quant == "fp8" and a.fp8_decode is False
    with pytest.raises(SystemExit):
        ap.parse_args(["--weight-quant", "int4"])
