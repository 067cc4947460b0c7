"""FP8 (e4m3) decode weights on the GPU: the FP8 instantiation of the packed decode kernel
(csrc/ops/gemm_decode_fp8.hip) against the bf16 instantiation on the dequantised weights.

The comparison is EQUALITY of bits: e4m3 -> bf16 is exact, both kernels feed the same MFMAs in
the same chunk order through the same reductions, and the per-column scale is a power of two,
which commutes with every fp32 rounding. Weights carry row magnitudes spanning 2^13 or more in
shuffled order, so a scale read from the wrong column cannot pass."""
import pytest
import torch

import fp8_checks as fc
from pilottai_amd import ops

pytestmark = pytest.mark.gpu

NAN = float("nan")
CONFIGS = [(1, 8, 1), (1, 16, 1), (2, 4, 1), (2, 8, 1), (2, 16, 1), (4, 8, 1), (4, 16, 1), (2, 8, 3), (1, 16, 2),
           (4, 8, 2)]
MS = [1, 3, 9, 16, 17, 33, 64]  # MT = 1, 2, 4 and ragged last row groups
RAISES = (ValueError, RuntimeError)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _x(M, K, gpu, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(M, K, generator=g).to(torch.bfloat16).to(gpu)


def _poison(gpu):
    ws, _ = ops.decode_workspace(gpu)
    ws.fill_(NAN)


def _both(gpu, x, wp, wp8, sp, epi, norm, resid, inplace, **cfg):
    """(bf16 kernel, FP8 kernel) outputs, each launched twice on NaN-poisoned outputs and slabs
    (the second launch runs on the tickets the first one left)."""
    M = x.shape[0]
    NO = wp.shape[0] * (8 if epi == "silu" else 16)
    outs = []
    for fn, args in ((ops.decode_gemm, (wp,)), (ops.decode_gemm_fp8, (wp8, sp))):
        for _ in range(2):
            _poison(gpu)
            if inplace:
                out = resid.clone()
                fn(x, *args, "resid", resid=out, out=out, **cfg)
            else:
                out = torch.full((M, NO), NAN, dtype=torch.bfloat16, device=gpu)
                fn(x, *args, epi, norm=norm, resid=resid, out=out, **cfg)
        outs.append(out)
    return outs


@pytest.mark.parametrize("K", [96, 512, 1056])  # 3 chunks < waves; one chunk per wave at 16; 33 = rounds + tail
@pytest.mark.parametrize("epi,norm,inplace", [("plain", False, False), ("plain", True, False),
                                              ("resid", False, False), ("resid", False, True),
                                              ("silu", True, False)])
def test_bit_identical_to_the_bf16_kernel(gpu, K, epi, norm, inplace):
    N = 256
    w = fc.spread_weight(N, K, seed=K)
    wp, wp8, sp = (t.to(gpu) for t in fc.quantized_pair(w, "gate_up" if epi == "silu" else "plain"))
    ran = 0
    for M in MS:
        x = _x(M, K, gpu, seed=M)
        resid = _x(M, N, gpu, seed=100 + M) if epi == "resid" else None
        for nt, waves, splits in CONFIGS:
            cfg = dict(nt=nt, waves=waves, splits=splits)
            try:
                ops.decode_gemm(x, wp, epi, norm=norm, resid=resid, **cfg)
            except ValueError:  # the dispatcher has no such kernel for this MT / epilogue:
                with pytest.raises(ValueError):  # the FP8 one refuses the same
                    ops.decode_gemm_fp8(x, wp8, sp, epi, norm=norm, resid=resid, **cfg)
                continue
            a, b = _both(gpu, x, wp, wp8, sp, epi, norm, resid, inplace, **cfg)
            assert torch.equal(_bits(a), _bits(b)), (M, cfg, (a.float() - b.float()).abs().max().item())
            assert not torch.isnan(b.float()).any(), (M, cfg)
            ran += 1
    assert ran >= 40, ran  # most configs exist for most MT


@pytest.mark.parametrize("M,H,KV,K,splits", [(1, 8, 2, 512, 0), (9, 4, 1, 1056, 3), (16, 4, 1, 96, 0)])
def test_qkv_rope_bit_identical(gpu, M, H, KV, K, splits):
    from pilottai_amd.ops import reference as ref

    N = (H + 2 * KV) * 128
    w = fc.spread_weight(N, K, seed=K + 1, lo=-3.5, hi=0.5)
    wp, wp8, sp = (t.to(gpu) for t in fc.quantized_pair(w, "rope"))
    x = _x(M, K, gpu, seed=3)
    cs = ref.rope_cos_sin(256, 128, 10000.0).to(gpu)
    g = torch.Generator().manual_seed(5)
    pos = torch.randint(0, 256, (M,), generator=g, dtype=torch.int32).to(gpu)
    NB = 8
    slots = torch.randperm(NB * 16, generator=g)[:M].to(torch.int32)
    slots[M // 2] = -1
    res = []
    for fn, args in ((ops.decode_qkv_rope, (wp,)), (ops.decode_qkv_rope_fp8, (wp8, sp))):
        for _ in range(2):
            _poison(gpu)
            q = torch.full((M, H, 128), NAN, dtype=torch.bfloat16, device=gpu)
            kc = torch.full((NB, KV, 16, 16, 8), 7.0, dtype=torch.bfloat16, device=gpu)
            vc = torch.full((NB, KV, 128, 16), 7.0, dtype=torch.bfloat16, device=gpu)
            fn(x, *args, 1e-5, q, kc, vc, pos, slots.to(gpu), cs, H, KV, splits=splits)
        res.append((q, kc, vc))
    for a, b in zip(*res):
        assert torch.equal(_bits(a), _bits(b))
    q, kc, vc = (t.clone() for t in res[1])
    assert not torch.isnan(q.float()).any()
    for s in slots.tolist():  # only the slots' entries changed
        if s >= 0:
            assert (kc[s >> 4, :, :, s & 15, :] != 7.0).any() and (vc[s >> 4, :, :, s & 15] != 7.0).any()
            kc[s >> 4, :, :, s & 15, :] = 7.0
            vc[s >> 4, :, :, s & 15] = 7.0
    assert (kc == 7.0).all() and (vc == 7.0).all()


def _gpu_weight(N, K, gpu, seed):
    """spread_weight at model shapes, generated on the device: row magnitudes over 10^4 ~ 2^13."""
    g = torch.Generator(device=gpu).manual_seed(seed)
    mag = torch.logspace(-3.5, 0.5, N, device=gpu)[torch.randperm(N, generator=g, device=gpu)]
    return (torch.randn(N, K, generator=g, device=gpu) * mag[:, None]).to(torch.bfloat16)


@pytest.mark.parametrize("M,N,K,epi", [(8, 6144, 4096, "rope"), (16, 28672, 4096, "silu"),
                                       (8, 4096, 14336, "resid"), (13, 4096, 4096, "resid"),
                                       (13, 4096, 4096, "plain")])
def test_default_configs_at_model_shapes(gpu, M, N, K, epi):
    """default_cfg depends on N and M: the shapes of the 8B layer, no (nt, waves, splits) given."""
    w = _gpu_weight(N, K, gpu, seed=N + K)
    kind = {"rope": "rope", "silu": "gate_up"}.get(epi, "plain")
    wp, wp8, sp = fc.quantized_pair(w, kind)
    x = _x(M, K, gpu, seed=7)
    if epi == "rope":
        from pilottai_amd.ops import reference as ref

        H, KV = 32, 8
        cs = ref.rope_cos_sin(64, 128, 10000.0).to(gpu)
        pos = torch.arange(M, dtype=torch.int32, device=gpu)
        slots = torch.arange(3, 3 + M, dtype=torch.int32, device=gpu)
        res = []
        for fn, args in ((ops.decode_qkv_rope, (wp,)), (ops.decode_qkv_rope_fp8, (wp8, sp))):
            q = torch.full((M, H, 128), NAN, dtype=torch.bfloat16, device=gpu)
            kc = torch.zeros(2, KV, 16, 16, 8, dtype=torch.bfloat16, device=gpu)
            vc = torch.zeros(2, KV, 128, 16, dtype=torch.bfloat16, device=gpu)
            fn(x, *args, 1e-5, q, kc, vc, pos, slots, cs, H, KV)
            res.append((q, kc, vc))
        for a, b in zip(*res):
            assert torch.equal(_bits(a), _bits(b))
        return
    norm = epi == "silu"
    resid = _x(M, N, gpu, seed=8) if epi == "resid" else None
    a, b = _both(gpu, x, wp, wp8, sp, epi, norm, resid, False)
    assert torch.equal(_bits(a), _bits(b))
    if epi == "plain":
        want = x.float() @ ops.unpack_decode_weight(wp).float().T
        torch.testing.assert_close(b.float(), want, atol=3e-2, rtol=2e-2)


def test_refused_shapes(gpu):
    w = fc.spread_weight(256, 96, seed=1)
    wp, wp8, sp = (t.to(gpu) for t in fc.quantized_pair(w, "plain"))
    for M, K in ((4, 80), (65, 96)):  # K % 32 != 0; more than 64 rows
        x = _x(M, K, gpu)
        with pytest.raises(RAISES):
            ops.decode_gemm(x, wp, "plain")
        with pytest.raises(RAISES):
            ops.decode_gemm_fp8(x, wp8, sp, "plain")
    w = fc.spread_weight(48, 96, seed=2)  # 3 tiles: no gate/up pairs
    wp, wp8, sp = (t.to(gpu) for t in fc.quantized_pair(w, "plain"))
    x = _x(4, 96, gpu)
    with pytest.raises(RAISES):
        ops.decode_gemm(x, wp, "silu", norm=True)
    with pytest.raises(RAISES):
        ops.decode_gemm_fp8(x, wp8, sp, "silu", norm=True)
    with pytest.raises(RAISES):  # scales of another length
        ops.decode_gemm_fp8(x, wp8, sp[:32].contiguous(), "plain")


# -- engine ----------------------------------------------------------------------------------------

_ENGINES = {}


def _engine(gpu, graphs, fp8_decode):
    from pilottai_amd.engine.engine import EngineConfig, LLMEngine

    key = (graphs, fp8_decode)
    if key not in _ENGINES:
        _ENGINES[key] = LLMEngine(EngineConfig(model="tiny-gqa4", max_num_seqs=16, max_num_batched_tokens=512,
                                               max_model_len=2048, num_kv_blocks=512, token_buckets=[16, 64, 256],
                                               use_graphs=graphs, weight_quant="fp8", fp8_decode=fp8_decode),
                                  device=gpu)
    return _ENGINES[key]


@pytest.fixture(scope="module", autouse=True)
def _stop_engines():
    yield
    for e in _ENGINES.values():
        e.stop()
    _ENGINES.clear()


@pytest.mark.parametrize("graphs", [False, True])
def test_engine_tokens_identical_with_and_without_the_fp8_copy(gpu, graphs):
    e8, e16 = _engine(gpu, graphs, True), _engine(gpu, graphs, False)
    assert e8.metrics()["fp8_decode"] is True and e16.metrics()["fp8_decode"] is False
    assert all("wqkv_p8" in L for L in e8.model.layers) and not any("wqkv_p8" in L for L in e16.model.layers)
    a = fc.request_tokens(e8, with_prediction=True)
    b = fc.request_tokens(e16, with_prediction=True)
    assert a == b
    if graphs:
        assert e8.metrics()["graphs"] > 0
    assert e8.metrics()["spec_draft_steps"] > 0  # the prediction made draft steps of 1 + k tokens


def test_decode_step_logits_and_weight_bytes(gpu):
    m8, m16 = _engine(gpu, False, True).model, _engine(gpu, False, False).model
    build = fc.make_step(m8, [1] * 8, [5, 17, 33, 64, 100, 7, 16, 250])
    a, b = fc.run_step(m8, build), fc.run_step(m16, build)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    extra = 0
    for L in m8.layers:
        for kind in ("wqkv", "wo", "w13", "w2"):
            assert L[kind + "_p8"].dtype == torch.float8_e4m3fn and L[kind + "_p8"].shape == L[kind + "_p"].shape
            extra += L[kind + "_p"].numel() + 4 * L[kind + "_p"].shape[0] * 16
    assert m8.weight_bytes() == m16.weight_bytes() + extra
