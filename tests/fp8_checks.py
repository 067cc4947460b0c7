"""Shared pieces of the FP8-weight tests (tests/test_fp8_weights.py on the CPU reference paths,
tests/test_fp8_decode_gpu.py on the kernels): test matrices whose row magnitudes span many
binades (a scale applied to the wrong column cannot pass), a hand-built step for
LlamaModel.forward, and the request set whose token ids are compared between engines."""
import numpy as np
import torch

from pilottai_amd import ops
from pilottai_amd.models.llama import KVCache, StepMeta

N_GEN = 24
PROMPT = "The orchestrator analyses a task and delegates it to worker agents"


def spread_weight(N, K, seed=0, lo=-3.0, hi=1.5, device="cpu"):
    """[N, K] bf16, row n of magnitude logspace(lo, hi)[perm(n)]: 10^4.5 ~ 2^15 between rows,
    shuffled so that neighbouring rows (and tiles) differ by many binades."""
    g = torch.Generator().manual_seed(seed)
    mag = torch.logspace(lo, hi, N)[torch.randperm(N, generator=g)]
    w = (torch.randn(N, K, generator=g) * mag[:, None]).to(torch.bfloat16)
    return w.to(device)


def quantized_pair(w, kind):
    """(bf16 pack of the dequantised weights, FP8 pack, packed scales) for packer `kind`."""
    pack, pack8 = {"plain": (ops.pack_decode_weight, ops.pack_decode_weight_fp8),
                   "gate_up": (ops.pack_decode_gate_up, ops.pack_decode_gate_up_fp8),
                   "rope": (ops.pack_decode_qkv_rope, ops.pack_decode_qkv_rope_fp8)}[kind]
    q, s = ops.quantize_fp8_rows(w)
    wp8, sp = pack8((q, s))
    return pack(ops.dequantize_fp8_rows(q, s)), wp8, sp


def make_step(model, q_lens, ctx_lens, seed=0):
    """One step of sum(q_lens) tokens for model.forward: sequence s feeds its last q_lens[s]
    tokens of a ctx_lens[s]-token context whose earlier keys are random cache contents.
    Returns a function that builds fresh (meta, kv, T, n_logit_rows, part_o, part_ml)."""
    dev, cfg = model.device, model.cfg
    KV, G = model.kv_local, model.h_local // model.kv_local
    ns, T = len(q_lens), int(sum(q_lens))
    nbs = [(c + 15) // 16 for c in ctx_lens]
    g = torch.Generator().manual_seed(seed)
    shape_k = (cfg.num_layers, sum(nbs) + 2, KV, 16, 16, 8)
    k0 = (torch.randn(shape_k, generator=g) * 0.5).to(torch.bfloat16)
    v0 = (torch.randn(cfg.num_layers, sum(nbs) + 2, KV, 128, 16, generator=g) * 0.5).to(torch.bfloat16)
    bt = torch.zeros(ns, max(nbs), dtype=torch.int32)
    nxt = 1
    for s, nb in enumerate(nbs):
        bt[s, :nb] = torch.arange(nxt, nxt + nb, dtype=torch.int32)
        nxt += nb
    pos, slots = [], []
    for s, (ql, ctx) in enumerate(zip(q_lens, ctx_lens)):
        for p in range(ctx - ql, ctx):
            pos.append(p)
            slots.append(int(bt[s, p // 16]) * 16 + p % 16)
    q_start = np.concatenate([[0], np.cumsum(q_lens)[:-1]]).astype(np.int32)
    ids = torch.randint(0, cfg.vocab_size, (T,), generator=g, dtype=torch.int32)
    items, nslots = ops.build_attention_items(q_lens, ctx_lens, G)
    maxit = max(len(items), nslots) + 1
    it = torch.tensor(items + [(0, 0, 0, 0)] * (maxit - len(items)), dtype=torch.int32)
    rows = [int(q_start[s]) + q_lens[s] - 1 for s in range(ns)]
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=dev)  # noqa: E731

    def build():
        kv = KVCache(cfg.num_layers, shape_k[1], KV, dev)
        kv.k.copy_(k0)
        kv.v.copy_(v0)
        meta = StepMeta(input_ids=ids.to(dev), positions=i32(pos), slots=i32(slots), q_start=i32(q_start),
                        q_len=i32(list(q_lens)), ctx_len=i32(list(ctx_lens)), block_table=bt.to(dev),
                        items=it.to(dev), n_items=i32([len(items)]),
                        att_counters=torch.zeros((ns + maxit) * KV, dtype=torch.int32, device=dev),
                        logit_rows=i32(rows), num_seqs=ns, part_size=i32([ops.ATT_PART]))
        part_o = torch.empty(maxit * KV * 16 * 128, dtype=torch.float32, device=dev)
        part_ml = torch.empty(maxit * KV * 16 * 2, dtype=torch.float32, device=dev)
        return meta, kv, T, ns, part_o, part_ml

    return build


def run_step(model, build):
    meta, kv, T, n_rows, part_o, part_ml = build()
    logits = model.forward(meta, kv, T, n_rows, part_o, part_ml)
    return logits.float().cpu(), kv.k.float().cpu(), kv.v.float().cpu()


def request_tokens(engine, with_prediction=False):
    """Token ids of the request set: greedy, seeded temperature 0.8, a JSON grammar, three greedy
    requests batched (multi-row decode steps); with_prediction: the greedy request again with its
    own output as the prediction, with every fourth token wrong (draft steps of 1 + k tokens,
    accepted and rejected drafts)."""
    tok = engine.tok
    p = tok.encode(PROMPT)
    out = {}
    out["greedy"] = engine.generate([p], temperature=0.0, max_tokens=N_GEN, ignore_eos=True)[0].token_ids
    out["seeded"] = engine.generate([p], temperature=0.8, seed=1234, max_tokens=N_GEN,
                                    ignore_eos=True)[0].token_ids
    segs = engine.grammar.compile("orchestrator.result_evaluation")
    out["grammar"] = engine.generate([tok.encode("Task: evaluate. Result: ok")], temperature=0.7, seed=7,
                                     max_tokens=N_GEN, grammar=segs)[0].token_ids
    batch = [tok.encode(PROMPT + " today" * k) for k in (1, 2, 3)]
    out["batch"] = [o.token_ids for o in engine.generate(batch, temperature=0.0, max_tokens=N_GEN, ignore_eos=True)]
    if with_prediction:
        V = engine.model_cfg.vocab_size
        wrong = [(t + 1) % V if i % 4 == 3 else t for i, t in enumerate(out["greedy"])]
        out["predicted"] = engine.generate([p], temperature=0.0, max_tokens=N_GEN, ignore_eos=True,
                                           prediction=wrong)[0].token_ids
    for k, v in out.items():
        assert len(v) > 0, k
    return out
