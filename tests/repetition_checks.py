"""Checks shared by tests/test_repetition_penalty.py (CPU tier) and tests/test_repetition_penalty_gpu.py."""
from collections import Counter

import numpy as np
import torch

from penalty_checks import LOGIT_TOL  # the engine's tolerance against reference_logits


def i32(x):
    return torch.as_tensor(x, dtype=torch.int32)


def f32(x):
    return torch.as_tensor(x, dtype=torch.float32)


def inv(r):
    """float32(1 / r): the double-precision quotient rounded once."""
    return float(np.float32(1.0 / float(r)))


def members(state, slot):
    """Token ids whose membership bit is set in `slot` of a (CPU) repetition state."""
    words = state[0][slot].numpy().view(np.uint32)
    return {w * 32 + b for w in np.flatnonzero(words).tolist() for b in range(32) if (int(words[w]) >> b) & 1}


def formula(row, seen, r):
    """The issue's formula on one row of any float dtype, independent of the op: per listed token
    one float32 product (numpy), one conversion back; every other entry keeps its bits."""
    out = row.clone()
    x = row.float().numpy()
    ir, rr = np.float32(inv(r)), np.float32(r)
    for t in seen:
        xt = np.float32(x[t])
        with np.errstate(invalid="ignore", over="ignore"):
            y = xt * ir if xt > 0 else xt * rr
        out[t] = torch.tensor(float(y), dtype=torch.float32).to(row.dtype)
    return out


def penalised_rows(engine, prompt, out, r, a=0.0, b=0.0, bias=None):
    """fp32 reference_logits rows of the positions that produced out[0], out[1], ... (the real
    prefix teacher-forced), shaped in the engine's order: repetition penalty over
    set(prompt + out[:i]) through the reference op, then presence a / frequency b over
    Counter(out[:i]), then `bias` {token: b}."""
    from pilottai_amd import ops
    from pilottai_amd.ops import reference as ref

    full = engine.model.reference_logits(list(prompt) + list(out[:-1])).float().cpu()
    V = full.shape[1]
    rows = []
    for i in range(len(out)):
        row = full[len(prompt) - 1 + i:len(prompt) + i].clone()
        hist = list(prompt) + list(out[:i])
        if r != 1.0:
            state = ops.repetition_state(1, V, len(hist), "cpu")
            ref.apply_repetition_penalty(row, state, i32([0]), i32([0]), f32([r]), f32([inv(r)]), i32([-1]),
                                         i32([0]), i32([len(hist)]), i32(hist))
            assert members(state, 0) == set(hist) and int(state[2][0]) == len(set(hist))
        for t, c in Counter(out[:i]).items():
            row[0, t] -= a + b * c
        for t, v in (bias or {}).items():
            row[0, t] += v
        rows.append(row[0])
    return torch.stack(rows)


def teacher_forced_rep(engine, prompt, out, r, a=0.0, b=0.0, bias=None, tol=LOGIT_TOL):
    """Greedy under a repetition penalty: each generated token's penalised reference logit is
    within `tol` of its row's penalised maximum."""
    rows = penalised_rows(engine, prompt, out, r, a, b, bias)
    for i, t in enumerate(out):
        gap = float(rows[i].max() - rows[i, t])
        print(f"token {i}: id {t} penalised logit {float(rows[i, t]):.4f}, row max {float(rows[i].max()):.4f}")
        assert gap <= tol, (i, t, int(rows[i].argmax()), gap)
    return rows
