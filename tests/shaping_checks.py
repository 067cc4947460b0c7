"""Checks shared by tests/test_logit_shaping.py (CPU tier) and tests/test_logit_shaping_gpu.py."""
import math

import numpy as np
import torch

from penalty_checks import LOGIT_TOL  # the engine's tolerance on a difference of two reference logits


def reference_rows(engine, prompt, out, bias=None):
    """fp32 reference_logits rows of the positions that produced out[0], out[1], ... (the real
    prefix teacher-forced), with `bias` {token: b} added."""
    full = engine.model.reference_logits(list(prompt) + list(out[:-1])).float().cpu()
    rows = full[len(prompt) - 1:len(prompt) - 1 + len(out)].clone()
    for t, b in (bias or {}).items():
        rows[:, t] += b
    return rows


def teacher_forced_bias(engine, prompt, out, bias, tol=LOGIT_TOL):
    """Greedy under a logit_bias: each generated token's biased reference logit is within `tol`
    of its row's biased maximum."""
    rows = reference_rows(engine, prompt, out, bias)
    for i, t in enumerate(out):
        gap = float(rows[i].max() - rows[i, t])
        print(f"token {i}: id {t} biased logit {float(rows[i, t]):.4f}, row max {float(rows[i].max()):.4f}")
        assert gap <= tol, (i, t, int(rows[i].argmax()), gap)


def minp_gaps(engine, prompt, out):
    """m_ref - l_ref[t] for every generated token t (free text: every token is allowed)."""
    rows = reference_rows(engine, prompt, out)
    return [float(rows[i].max() - rows[i, t]) for i, t in enumerate(out)]


def minp_bound(T, p, tol=LOGIT_TOL):
    """The largest gap to the row maximum a token kept by min_p = p at temperature T can have."""
    return -T * math.log(p) + tol


def kept_set(logits_row, tau):
    """Token ids of a row (any float dtype) at or above the threshold."""
    return set(torch.nonzero(logits_row.float() >= tau).flatten().tolist())


def forbidden_id(engine):
    """A token id that no grammar mask class registered so far allows (compile the grammar first)."""
    rows = engine.grammar.reg.rows
    allowed = np.zeros(len(rows[0]), dtype=bool)
    for r in rows:
        allowed |= np.asarray(r, dtype=bool)
    return int(np.flatnonzero(~allowed)[-1])
