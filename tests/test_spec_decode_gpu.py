"""Predicted outputs and prompt-lookup drafts on the GPU engine (hipGraph steps, the HIP
acceptance pass). The bodies are in tests/spec_checks.py, shared with tests/test_spec_decode.py."""
import pytest

import spec_checks as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine(gpu):
    from pilottai_amd.engine.engine import EngineConfig, LLMEngine

    e = LLMEngine(EngineConfig(model="tiny-gqa4", max_num_seqs=16, max_num_batched_tokens=512,
                               max_model_len=2048, num_kv_blocks=512, token_buckets=[16, 64, 256]),
                  device=gpu)
    yield e
    e.stop()


def _check_greedy(engine, prompt, gen, rel: float = 0.0):
    """Each greedy token is the fp32 reference's argmax within 0.05 (tests/test_engine_gpu.py)."""
    ref = engine.model.reference_logits(prompt + gen[:-1])  # [T, V] fp32
    T0 = len(prompt)
    for i, tok in enumerate(gen):
        row = ref[T0 - 1 + i]
        tol = 0.05 + rel * float(row.max().abs())
        assert row[tok] >= row.max() - tol, (i, tok, int(row.argmax()), float(row[tok]), float(row.max()))


def test_candidate_list_contains_a_prompt_with_the_margins(engine):
    for mode in ("greedy", "sampled"):
        assert len(sc.pick(engine, mode)[1]) == sc.N_GEN


@pytest.mark.parametrize("mode", ["greedy", "sampled"])
def test_prediction_equal_to_the_plain_output(engine, mode):
    sc.check_prediction_equal_to_the_plain_output(engine, mode)


def test_corrupted_prediction_resyncs(engine):
    sc.check_corrupted_prediction(engine)


def test_prompt_lookup(engine):
    sc.check_prompt_lookup(engine)


def test_grammar_request_with_a_prediction(engine):
    sc.check_grammar(engine)


def test_drafting_request_beside_plain_requests(engine):
    sc.check_batching(engine)


def test_draft_len_alone_changes_nothing(engine):
    sc.check_draft_len_alone_changes_nothing(engine)


def test_refusals(engine):
    sc.check_refusals(engine)


def test_drafted_greedy_tokens_follow_the_reference(engine):
    """Whatever the margins: every token of drafted greedy runs -- a right prediction, a wrong one,
    prompt lookup -- is the fp32 reference's argmax within the project's tolerance."""
    tok = engine.tok
    kw = dict(temperature=0.0, max_tokens=sc.N_GEN, ignore_eos=True)
    for text, _ in sc.CANDIDATES[:3]:
        p = tok.encode(text)
        plain = engine.generate([p], **kw)[0].token_ids
        wrong = [(t + 1) % engine.model_cfg.vocab_size if i % 4 == 3 else t for i, t in enumerate(plain)]
        for extra in (dict(prediction=plain), dict(prediction=wrong), dict(prompt_lookup=True),
                      dict(prediction=wrong, prompt_lookup=True, draft_len=7)):
            o = engine.generate([p], **kw, **extra)[0]
            assert len(o.token_ids) == sc.N_GEN
            _check_greedy(engine, p, o.token_ids)


def test_draft_steps_replay_graphs_of_their_own(engine):
    p, plain, seed = sc.pick(engine, "greedy")
    plain_keys = {k for k in engine._graphs if len(k) < 9}
    engine.generate([p], prediction=plain, temperature=0.0, max_tokens=sc.N_GEN, ignore_eos=True)
    spec_keys = {k for k in engine._graphs if len(k) == 9}
    assert spec_keys and all(k[-1] is True for k in spec_keys)
    assert plain_keys <= set(engine._graphs)  # the plain graphs are the ones captured before
