"""Checks shared by tests/test_logprobs.py (CPU tier) and tests/test_logprobs_gpu.py."""
import math


def consistent(engine, o, n, greedy=False, segs=None):
    """What holds for every output that asked for n alternatives; with `segs` the grammar is
    replayed on the host: forced tokens have 0.0 and every listed id was allowed there."""
    assert o.logprobs is not None and len(o.logprobs) == len(o.token_ids)
    assert abs(o.cumulative_logprob - sum(e[0] for e in o.logprobs)) < 1e-6
    gr = engine._rt.Grammar(segs) if segs is not None else None
    rows = engine.grammar.reg.rows
    run = list(gr.take_forced_run(1 << 20)) if gr is not None else []  # jump-forwarded at add_request
    for tok, (lp, top) in zip(o.token_ids, o.logprobs):
        assert len(top) <= n and lp <= 1e-6 and not math.isnan(lp)
        vals = [v for _, v in top]
        assert vals == sorted(vals, reverse=True)
        assert sum(math.exp(v) for v in vals) <= 1 + 1e-3
        listed = dict(top)
        if tok in listed:
            assert listed[tok] == lp
        if greedy and n > 0:  # free text, any grammar class, forced and jump-forward tokens alike
            assert top[0][0] == tok
        if gr is None:
            continue
        if run:  # a jump-forward token
            assert tok == run.pop(0) and lp == 0.0 and top == [(tok, 0.0)][:n]
            continue
        cls, forced = gr.next()
        if forced >= 0:
            assert tok == forced and lp == 0.0 and top == [(tok, 0.0)][:n]
        elif cls >= 0:
            assert rows[cls][tok] and all(rows[cls][i] for i in listed), (tok, cls)
        gr.advance(tok)
        if not gr.done():
            run = list(gr.take_forced_run(1 << 20))
