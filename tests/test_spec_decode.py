"""Predicted outputs and prompt-lookup drafts through the engine, CPU tier (the reference ops:
ops.reference.spec_verify is the acceptance pass). The bodies are in tests/spec_checks.py, shared
with tests/test_spec_decode_gpu.py."""
import pytest

import spec_checks as sc


@pytest.fixture(scope="module")
def engine():
    from pilottai_amd.engine.engine import EngineConfig, LLMEngine

    e = LLMEngine(EngineConfig(model="tiny", max_num_seqs=16, max_num_batched_tokens=128, max_model_len=512,
                               num_kv_blocks=128, use_graphs=False), device="cpu")
    yield e
    e.stop()


def test_candidate_list_contains_a_prompt_with_the_margins(engine):
    assert len(sc.CANDIDATES) >= 8
    for mode in ("greedy", "sampled"):
        p, plain, _ = sc.pick(engine, mode)
        assert len(plain) == sc.N_GEN


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


def test_the_cpu_tier_runs_the_reference_acceptance_pass(engine, monkeypatch):
    from pilottai_amd.ops import reference as ref

    calls = []
    real = ref.spec_verify
    monkeypatch.setattr(ref, "spec_verify", lambda *a: calls.append(1) or real(*a))
    p, plain, seed = sc.pick(engine, "greedy")
    d0 = engine.metrics()["spec_draft_steps"]
    o = engine.generate([p], prediction=plain, temperature=0.0, max_tokens=sc.N_GEN, ignore_eos=True)[0]
    assert o.token_ids == plain
    assert len(calls) == engine.metrics()["spec_draft_steps"] - d0 > 0  # once per draft step
