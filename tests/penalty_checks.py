"""Checks shared by tests/test_penalties.py (CPU tier) and tests/test_penalties_gpu.py."""
from collections import Counter

import torch

LOGIT_TOL = 0.05  # what tests/test_engine_gpu.py::_check_greedy grants the engine against reference_logits


def teacher_forced(engine, prompt, out, a, b, tol=LOGIT_TOL):
    """Each generated token's penalised reference logit is within `tol` of its row's maximum:
    reference_logits of the real prefix, the reference penalty with Counter(out[:i])."""
    from pilottai_amd import ops
    from pilottai_amd.ops import reference as ref

    full = engine.model.reference_logits(list(prompt) + list(out[:-1])).float().cpu()
    V = full.shape[1]
    i32 = lambda x: torch.tensor(x, dtype=torch.int32)  # noqa: E731
    for i, t in enumerate(out):
        row = full[len(prompt) - 1 + i:len(prompt) + i].clone()
        state = ops.penalty_state(1, V, max(1, i), "cpu")
        ref.apply_penalties(row, state, i32([0]), i32([0]), torch.tensor([a]), torch.tensor([b]), i32([-1]),
                            i32([0]), i32([i]), i32(list(out[:i])))
        assert {k: int(v) for k, v in enumerate(state[0][0].tolist()) if v} == dict(Counter(out[:i]))
        gap = float(row[0].max() - row[0, t])
        print(f"token {i}: id {t} penalised logit {float(row[0, t]):.4f}, row max {float(row[0].max()):.4f}")
        assert gap <= tol, (i, t, int(row[0].argmax()), gap)
