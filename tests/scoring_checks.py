"""Helpers shared by tests/test_scoring.py and tests/test_scoring_gpu.py."""
import socket
import threading
import time

import numpy as np


def order_keys(bits: np.ndarray) -> np.ndarray:
    """The 16-bit order key of raw bf16 bit patterns (csrc/ops/logprob_common.h bf16_order_key)."""
    b = bits.astype(np.int64) & 0xFFFF
    return np.where(b & 0x8000, ~b & 0xFFFF, b | 0x8000)


def brute_rank(keys: np.ndarray, t: int) -> int:
    """The issue's rule as a literal loop over the vocabulary."""
    rank = 1
    for i in range(keys.shape[0]):
        if keys[i] > keys[t] or (keys[i] == keys[t] and i < t):
            rank += 1
    return rank


def record_consistent(target: int, lp: float, rank: int, ids, lps, n: int) -> None:
    """A score record agrees with itself, exactly: rank <= n means the target is ids[rank - 1] with
    the same logprob; rank > n means it is absent from the list and no likelier than its last entry."""
    assert rank >= 1, rank
    listed = [i for i in ids[:n] if i >= 0]
    assert len(set(listed)) == len(listed) and list(ids[len(listed):]) == [-1] * (len(ids) - len(listed))
    assert all(a >= b for a, b in zip(lps[:len(listed)], lps[1:len(listed)])), lps
    if rank <= n:
        assert ids[rank - 1] == target and lp == lps[rank - 1], (target, lp, rank, ids, lps)
    else:
        assert target not in listed, (target, rank, ids)
        if n > 0 and len(listed) == n:
            assert lp <= lps[n - 1], (lp, lps)


class Server:
    """The app on a uvicorn thread, as tests/test_http_serving.py runs it."""

    def __init__(self, app):
        import uvicorn

        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        self.port = s.getsockname()[1]
        s.close()
        self.server = uvicorn.Server(uvicorn.Config(app, host="127.0.0.1", port=self.port, log_level="error"))
        self.thread = threading.Thread(target=self.server.run, daemon=True)

    def __enter__(self):
        self.thread.start()
        t0 = time.time()
        while not self.server.started:
            assert time.time() - t0 < 30, "server did not start"
            time.sleep(0.02)
        return f"http://127.0.0.1:{self.port}/v1"

    def __exit__(self, *exc):
        self.server.should_exit = True
        self.thread.join(timeout=10)
