"""Checks shared by tests/test_spec_decode.py (CPU tier) and tests/test_spec_decode_gpu.py:
predicted outputs and prompt-lookup drafts through the engine.

A drafted run moves steps to other attention item shapes and GEMM row counts than the plain run,
so its tokens are bit-identical to the plain run's only up to bf16 rounding of the logits
(tests/test_engine_gpu.py test_sampling_batch_invariance). The comparisons therefore run on a
prompt whose plain run has, at every generated position, a top-2 margin in the fp32 reference
logits of twice the project's own tolerance (the 0.05 of _check_greedy): 0.1 on the logits for
greedy runs, 0.1 / T on the Gumbel keys for runs sampled at temperature T. The prompt is the first
of a fixed list that meets the condition; the tests assert that there is one."""
import json
import math
import types

import numpy as np
import pytest
import torch

from pilottai_amd.ops import reference as ref

N_GEN = 24
MARGIN = 0.1  # 2 x the 0.05 of _check_greedy: neither run can cross the runner-up
T_SAMPLED, TOP_P = 0.8, 0.9

# Random-init weights give nearly flat logits: a free-text prompt's greedy run has top-2 margins
# of a few hundredths, and no 24 positions in a row clear 0.1. Prompts that repeat a short
# pattern often enough drive these models into a stable continuation with margins of 0.1 - 0.4,
# so the greedy list is made of those (the CPU tier's model and the GPU tests' model have
# different weights and take different ones). For the sampled case the Gumbel noise dominates:
# the top-2 gap of the keys is about Exp(1), so 24 gaps above 0.125 in a row happen for about one
# seed in twenty, and the list is one prompt under many seeds.
GREEDY_CANDIDATES = [(pat * n).strip() for pat, n in (
    ("1 2 3 4 ", 8), ("5 ", 28), ("10 20 30 ", 20), ("9 8 7 ", 40), ("yes no ", 14), ("5 ", 20),
    ("10 20 30 ", 28), ("1 2 3 4 ", 14), ("5 ", 40), ("10 20 30 ", 40), ("2 4 6 8 ", 14), ("7 ", 28))]
SAMPLED_CANDIDATES = [(GREEDY_CANDIDATES[0], seed) for seed in [1592, 2776] + [1000 + 37 * i for i in range(62)]]
CANDIDATES = [(t, 0) for t in GREEDY_CANDIDATES] + SAMPLED_CANDIDATES  # (prompt text, seed)

_cache = {}


def _kw(mode, seed):
    if mode == "greedy":
        return dict(temperature=0.0, max_tokens=N_GEN, ignore_eos=True)
    return dict(temperature=T_SAMPLED, top_p=TOP_P, seed=seed, max_tokens=N_GEN, ignore_eos=True)


def margins(engine, prompt, gen, mode, seed, allowed=None):
    """Per generated position: (the fp32 reference's choice there, its margin over the runner-up).
    greedy: on the logits; sampled: on logit / T + Gumbel noise over the tokens top-p keeps, the
    noise from ops.reference.uniform01 at the token's position. `allowed`: per position a bool
    mask of the tokens the grammar allows (None: all)."""
    logits = engine.model.reference_logits(list(prompt) + list(gen[:-1])).double().cpu().numpy()
    V = logits.shape[1]
    out = []
    for i in range(len(gen)):
        row = logits[len(prompt) - 1 + i].copy()
        if allowed is not None and allowed[i] is not None:
            row[~allowed[i]] = -np.inf
        if mode == "greedy":
            key = row
        else:
            one = lambda v, dt: torch.tensor([v], dtype=dt)
            tau = float(ref.topkp_threshold(torch.from_numpy(row[None]).float(), one(T_SAMPLED, torch.float32),
                                            one(0, torch.int32), one(TOP_P, torch.float32),
                                            one(-1, torch.int32), None)[0])
            u = ref.uniform01(seed, len(prompt) + i, np.arange(V))
            key = row / T_SAMPLED - np.log(-np.log(u))
            key[row < tau] = -np.inf
        best = int(np.argmax(key))
        rest = np.delete(key, best).max()
        out.append((best, float(key[best] - rest)))
    return out


def pick(engine, mode):
    """(prompt ids, plain output, seed) of the first candidate whose plain run follows the fp32
    reference with the margin at all N_GEN positions."""
    ck = (id(engine), mode)
    if ck in _cache:
        return _cache[ck]
    need = MARGIN if mode == "greedy" else MARGIN / T_SAMPLED
    seen = []
    for text, seed in ([(t, 0) for t in GREEDY_CANDIDATES] if mode == "greedy" else SAMPLED_CANDIDATES):
        p = engine.tok.encode(text)
        o = engine.generate([p], **_kw(mode, seed))[0]
        m = margins(engine, p, o.token_ids, mode, seed)
        seen.append(min(x[1] for x in m))
        if len(o.token_ids) == N_GEN and all(t == c and g > need for t, (c, g) in zip(o.token_ids, m)):
            _cache[ck] = (p, o.token_ids, seed)
            return _cache[ck]
    raise AssertionError(f"no candidate prompt meets the {mode} margin {need}: smallest margins {seen}")


def _steps(engine):
    return engine.stats["steps"]


def check_prediction_equal_to_the_plain_output(engine, mode):
    p, plain, seed = pick(engine, mode)
    K = engine.cfg.draft_len
    s0 = _steps(engine)
    o = engine.generate([p], prediction=plain, **_kw(mode, seed))[0]
    steps = _steps(engine) - s0
    assert o.token_ids == plain
    assert o.accepted_prediction_tokens == N_GEN - 1 and o.rejected_prediction_tokens == 0
    # one prefill step, then decode steps of K + 1 tokens each
    assert steps - 1 <= math.ceil(N_GEN / (K + 1)) + 1, steps
    return o


def check_corrupted_prediction(engine):
    p, plain, seed = pick(engine, "greedy")
    V = engine.model_cfg.vocab_size
    bad = list(plain)
    for i in (5, 13):
        bad[i] = next(t for t in range(plain[i] + 1, plain[i] + V) if t % V not in plain) % V
    o = engine.generate([p], prediction=bad, **_kw("greedy", seed))[0]
    assert o.token_ids == plain
    assert o.rejected_prediction_tokens >= 2
    # the resync: the same prediction cut behind position 13 behaves identically up to there and
    # accepts fewer tokens, so the difference was accepted after position 13
    cut = engine.generate([p], prediction=bad[:14], **_kw("greedy", seed))[0]
    assert cut.token_ids == plain
    assert o.accepted_prediction_tokens > cut.accepted_prediction_tokens


def simulate_lookup(prompt, out, K, max_tokens):
    """Draft tokens the prompt-lookup rule gets accepted on a run that emits `out`: the host's
    replay of the scheduler's rule (latest earlier occurrence of the last 4 / 3 / 2 tokens)."""
    def lookup(t, k):
        for n in (4, 3, 2):
            if len(t) <= n:
                continue
            for i in range(len(t) - 1, n - 1, -1):
                if t[i - n:i] == t[-n:]:
                    return t[i:i + k]
        return []

    t, g, acc = list(prompt) + [out[0]], 1, 0
    while g < len(out):
        draft = lookup(t, min(K, max_tokens - g - 1))
        a = 0
        while a < len(draft) and draft[a] == out[g + a]:
            a += 1
        t += out[g:g + a + 1]
        g += a + 1
        acc += a
    return acc


def check_prompt_lookup(engine):
    """A prompt that contains the first 12 tokens of its own plain continuation: the reply goes on
    from them, and whatever it repeats of the prompt or of itself is drafted from there."""
    p, plain, seed = pick(engine, "greedy")
    K = engine.cfg.draft_len
    p2 = list(p) + plain[:12]
    plain2 = engine.generate([p2], **_kw("greedy", seed))[0].token_ids
    m = margins(engine, p2, plain2, "greedy", seed)
    safe = next((i for i, (t, (c, g)) in enumerate(zip(plain2, m)) if t != c or g <= MARGIN), N_GEN)
    assert plain2[:12] == plain[12:] and safe >= 12  # the candidate's own margins cover these
    o = engine.generate([p2], prompt_lookup=True, **_kw("greedy", seed))[0]
    assert o.token_ids[:safe] == plain2[:safe]
    assert o.accepted_prediction_tokens > 0
    if o.token_ids == plain2:
        assert o.accepted_prediction_tokens == simulate_lookup(p2, plain2, K, N_GEN)
        assert o.rejected_prediction_tokens >= 0


def _grammar_masks(engine, segs, toks):
    """Per generated token: the bool mask of the tokens the grammar allowed there, None where the
    token was forced (a literal or a jump-forward run)."""
    gr = engine._rt.Grammar(segs)
    rows = engine.grammar.reg.rows
    run = list(gr.take_forced_run(1 << 20))
    out = []
    for tok in toks:
        if run:
            assert tok == run.pop(0)
            out.append(None)
            continue
        cls, forced = gr.next()
        out.append(None if forced >= 0 else (np.asarray(rows[cls], dtype=bool) if cls >= 0 else
                                             np.ones(engine.model_cfg.vocab_size, dtype=bool)))
        gr.advance(tok)
        if not gr.done():
            run = list(gr.take_forced_run(1 << 20))
    return out


def check_grammar(engine):
    tok = engine.tok
    segs = engine.grammar.compile("agent.result_evaluation")
    p = tok.encode("evaluate this result please")
    kw = dict(temperature=0.0, max_tokens=400, grammar=segs)
    plain = engine.generate([p], **kw)[0]
    o = engine.generate([p], prediction=tok.encode(plain.text), **kw)[0]
    obj = json.loads(o.text)
    assert set(obj) >= {"success", "quality_score", "reasoning"} and o.finish_reason == "stop"
    masks = _grammar_masks(engine, segs, plain.token_ids)
    m = margins(engine, p, plain.token_ids, "greedy", 0, allowed=masks)
    safe = next((i for i, (t, mk, (c, g)) in enumerate(zip(plain.token_ids, masks, m))
                 if mk is not None and (t != c or g <= MARGIN)), len(plain.token_ids))
    assert o.token_ids[:safe] == plain.token_ids[:safe]
    assert o.accepted_prediction_tokens > 0
    assert o.forced_tokens + o.sampled_tokens == len(o.token_ids)


def run_mixed(engine, requests):
    """Submit requests with their own arguments and drive the loop inline: [(prompt, kwargs)] ->
    outputs in order."""
    done = {}
    ids = [engine.submit(p, lambda o: done.__setitem__(o.request_id, o), **kw) for p, kw in requests]
    while len(done) < len(ids):
        if not engine.step() and not engine.sched.has_work() and engine._inbox.empty():
            break
    return [done[i] for i in ids]


def check_batching(engine):
    p, plain, seed = pick(engine, "greedy")
    tok = engine.tok
    others = [tok.encode(t) for t in ("hi there", "ok then", "and now")]
    d0 = engine.metrics()["spec_draft_steps"]
    outs = run_mixed(engine, [(p, dict(prediction=plain, **_kw("greedy", seed)))] +
                     [(q, _kw("greedy", seed)) for q in others])
    assert outs[0].token_ids == plain and outs[0].accepted_prediction_tokens > 0
    assert engine.metrics()["spec_draft_steps"] > d0
    alone = engine.generate(others, **_kw("greedy", seed))
    for a, b in zip(alone, outs[1:]):  # the plain requests beside it: untouched
        assert b.accepted_prediction_tokens == 0 and b.rejected_prediction_tokens == 0
        mm = margins(engine, others[alone.index(a)], a.token_ids, "greedy", seed)
        safe = next((i for i, (t, (c, g)) in enumerate(zip(a.token_ids, mm)) if t != c or g <= MARGIN), N_GEN)
        assert a.token_ids[:safe] == b.token_ids[:safe]


def check_draft_len_alone_changes_nothing(engine):
    p, plain, seed = pick(engine, "greedy")
    d0 = engine.metrics()["spec_draft_tokens"]
    o = engine.generate([p], draft_len=5, **_kw("greedy", seed))[0]
    assert o.token_ids == plain and engine.metrics()["spec_draft_tokens"] == d0
    o = engine.generate([p], prediction=plain, draft_len=0, **_kw("greedy", seed))[0]
    assert o.token_ids == plain and engine.metrics()["spec_draft_tokens"] == d0
    assert o.accepted_prediction_tokens == 0 and o.rejected_prediction_tokens == 0


def check_refusals(engine):
    p = engine.tok.encode("refuse this")
    V = engine.model_cfg.vocab_size
    cb = lambda o: None
    bad = [dict(prediction=[1, V]), dict(prediction=[-1]), dict(prediction=[1.5]),
           dict(prediction=[1, 2], draft_len=-1), dict(prediction=[1, 2], draft_len=engine.cfg.max_draft_len + 1),
           dict(prompt_lookup=True, draft_len=engine.cfg.max_draft_len + 1),
           dict(draft_len=engine.cfg.max_draft_len + 1),
           dict(prediction=[1, 2], logprobs=0), dict(prompt_lookup=True, logprobs=3),
           dict(prediction=[1, 2], presence_penalty=0.5), dict(prediction=[1, 2], frequency_penalty=-0.5),
           dict(prompt_lookup=True, repetition_penalty=1.2),
           dict(prediction=[1, 2], score_from=1), dict(prompt_lookup=True, score_from=1),
           dict(prediction=[1, 2], embed=True), dict(prompt_lookup=True, embed="last")]
    for kw in bad:
        with pytest.raises(ValueError):
            engine.submit(p, cb, **kw)
    tp, was = engine.tp, engine.cfg.async_steps
    try:
        engine.tp = types.SimpleNamespace(size=2, rank=0)
        for kw in (dict(prediction=[1, 2]), dict(prompt_lookup=True)):
            with pytest.raises(ValueError, match="tensor-parallel"):
                engine.submit(p, cb, **kw)
        engine.tp = tp
        engine.cfg.async_steps = True
        for kw in (dict(prediction=[1, 2]), dict(prompt_lookup=True)):
            with pytest.raises(ValueError, match="async_steps"):
                engine.submit(p, cb, **kw)
    finally:
        engine.tp, engine.cfg.async_steps = tp, was
    assert engine._inbox.empty()  # nothing of the above was queued
