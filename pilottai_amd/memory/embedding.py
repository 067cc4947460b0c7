"""Text embedders for the semantic store.

`HashingEmbedder` (default): signed feature hashing of lower-cased word unigrams
and bigrams plus character trigrams into D=1024 dims, L2-normalised. It is
deterministic, needs no weights, and makes cosine similarity track lexical
overlap — a strict generalisation of the reference's case-insensitive
substring search (pilott/memory/enhanced_memory.py:110), which it replaces.

`EngineEmbedder`: mean-pooled final hidden states of the local Llama engine's model,
projected to D by a fixed random orthogonal map (meaningful with real weights). By
default (`pool="engine"`) the texts go through the serving engine itself as embedding
requests — same kernels, same continuous batch as the agents' calls.

`chunk_spans` / `span_windows` cut a tokenised document into overlapping chunks, and
`EngineEmbedder.embed_document` embeds all of them in one prefill per context window
(`LLMEngine.embed_spans`): each chunk vector is the mean of the final hidden states of its
tokens, every one of which has seen the document up to there ("late chunking").
"""
from __future__ import annotations

import re
import zlib
from typing import List, Sequence, Tuple

import numpy as np

_TOK = re.compile(r"[a-z0-9]+")


def _h(s: str) -> int:
    return zlib.crc32(s.encode("utf-8"))


def chunk_spans(n_tokens: int, chunk_tokens: int, overlap: int) -> List[Tuple[int, int]]:
    """Token ranges [(0, c), (c - o, 2c - o), ...] of chunks of `chunk_tokens` = c tokens, each
    starting `overlap` = o tokens before the end of the one before; the last one ends at
    n_tokens (and may be shorter). No range lies inside the one before it."""
    if isinstance(chunk_tokens, bool) or not isinstance(chunk_tokens, int) or chunk_tokens < 1:
        raise ValueError(f"chunk_tokens must be an integer >= 1, not {chunk_tokens!r}")
    if isinstance(overlap, bool) or not isinstance(overlap, int) or not 0 <= overlap < chunk_tokens:
        raise ValueError(f"overlap must be an integer in [0, chunk_tokens), not {overlap!r}")
    if isinstance(n_tokens, bool) or not isinstance(n_tokens, int) or n_tokens < 0:
        raise ValueError(f"n_tokens must be an integer >= 0, not {n_tokens!r}")
    out, a = [], 0
    while n_tokens > 0:
        b = min(a + chunk_tokens, n_tokens)
        out.append((a, b))
        if b == n_tokens:
            break
        a += chunk_tokens - overlap
    return out


def span_windows(n_tokens: int, chunk_tokens: int, overlap: int, max_window: int,
                 max_spans: int) -> List[Tuple[int, int, List[Tuple[int, int]]]]:
    """The chunks of chunk_spans grouped into windows of at most `max_window` tokens and
    `max_spans` chunks: [(start, end, [(a, b), ...])] with the chunk ranges in document
    coordinates. A window starts where its first chunk starts (a multiple of the chunk stride)
    and ends where its last one ends, so no chunk straddles two windows; neighbouring windows
    share the overlap tokens."""
    spans = chunk_spans(n_tokens, chunk_tokens, overlap)
    if spans and (chunk_tokens > max_window or max_spans < 1):
        raise ValueError(f"a chunk of {chunk_tokens} tokens does not fit a window of {max_window} tokens")
    out: List[Tuple[int, int, List[Tuple[int, int]]]] = []
    for a, b in spans:
        if out and b - out[-1][0] <= max_window and len(out[-1][2]) < max_spans:
            out[-1] = (out[-1][0], b, out[-1][2] + [(a, b)])
        else:
            out.append((a, b, [(a, b)]))
    return out


class HashingEmbedder:
    def __init__(self, dim: int = 1024):
        self.dim = dim

    def features(self, text: str):
        t = text.lower()
        words = _TOK.findall(t)
        feats = [("w", w) for w in words]
        feats += [("b", f"{a} {b}") for a, b in zip(words, words[1:])]
        squeezed = " ".join(words)
        feats += [("c", squeezed[i:i + 3]) for i in range(max(0, len(squeezed) - 2))]
        return feats

    def embed(self, texts: Sequence[str]) -> np.ndarray:
        out = np.zeros((len(texts), self.dim), dtype=np.float32)
        wts = {"w": 1.0, "b": 0.7, "c": 0.35}
        for r, text in enumerate(texts):
            row = out[r]
            for kind, f in self.features(text):
                h = _h(kind + ":" + f)
                row[h % self.dim] += wts[kind] * (1.0 if (h >> 31) & 1 else -1.0)
            n = np.linalg.norm(row)
            if n > 0:
                row /= n
        return out

    def __call__(self, texts: Sequence[str]) -> np.ndarray:
        return self.embed(texts)


class EngineEmbedder:
    """Embeddings from the serving model itself: final-norm hidden states
    mean-pooled over the text's tokens (pooling="last": the last token's state, which lets
    the engine reuse cached prefixes), projected to `dim` by a fixed orthonormal matrix and
    L2-normalised; texts truncated to `max_tokens`.

    pool="engine" (default): embedding requests through `LLMEngine.embed` — prefilled by
    the engine's kernels inside its continuous batch, pooled in the step graph.
    pool="hidden": a separate dense PyTorch forward (LlamaModel.hidden_states), the
    reference the engine path is tested against. pool="tokens": the (much cheaper) mean
    of the input token embeddings."""

    def __init__(self, engine, dim: int = 1024, seed: int = 0, pool: str = "engine", batch_size: int = 16,
                 max_tokens: int = 512, pooling: str = "mean"):
        import torch

        self.engine = engine
        self.dim = dim
        d = engine.model_cfg.hidden_size
        g = torch.Generator().manual_seed(seed)
        if d >= dim:  # [d, dim] with orthonormal columns
            q, _ = torch.linalg.qr(torch.randn(d, dim, generator=g))
        else:  # a model narrower than the index (test shapes): orthonormal rows
            q = torch.linalg.qr(torch.randn(dim, d, generator=g))[0].T
        self.proj = q.contiguous().to(engine.device, torch.float32)
        self.pool = pool if (pool == "engine" or getattr(engine.model.tp, "size", 1) == 1) else "tokens"
        self.batch_size = batch_size
        self.max_tokens = max_tokens
        if pooling not in ("mean", "last"):
            raise ValueError(f"pooling must be 'mean' or 'last', not {pooling!r}")
        # "last": the last token's state — embedding requests then reuse the engine's prefix
        # cache (texts that share a prefix, like an agent's successive lookups, share its work)
        self.pooling = pooling
        self._stream = None

    def embed(self, texts: Sequence[str]) -> np.ndarray:
        import torch
        import torch.nn.functional as F

        m = self.engine.model
        rows: List[np.ndarray] = []
        if self.pool == "engine":
            ids = [self.engine.tok.encode(t)[: self.max_tokens] or [0] for t in texts]
            if not ids:
                return np.zeros((0, self.dim), np.float32)
            return self._project(self.engine.embed(ids, pooling=self.pooling))
        with torch.inference_mode():
            if self.pool == "hidden":
                for i in range(0, len(texts), self.batch_size):
                    ids = [self.engine.tok.encode(t)[: self.max_tokens] or [0] for t in texts[i:i + self.batch_size]]
                    v = F.normalize(m.hidden_states(ids, pooling=self.pooling) @ self.proj, dim=1)
                    rows.extend(v.cpu().numpy())
            else:
                for t in texts:
                    ids = torch.tensor(self.engine.tok.encode(t)[: self.max_tokens] or [0], device=self.engine.device)
                    h = F.embedding(ids, m.embed).float().mean(0)
                    rows.append(F.normalize(h @ self.proj, dim=0).cpu().numpy())
        return np.stack(rows) if rows else np.zeros((0, self.dim), np.float32)

    def __call__(self, texts):
        return self.embed(texts)

    def _project(self, h: np.ndarray) -> np.ndarray:
        """Pooled hidden states [n, hidden] -> projected, L2-normalised [n, dim]."""
        import torch
        import torch.nn.functional as F

        if not len(h):
            return np.zeros((0, self.dim), np.float32)
        hd = torch.from_numpy(np.ascontiguousarray(h, dtype=np.float32))
        if self.proj.device.type != "cuda":
            return F.normalize(hd @ self.proj, dim=1).numpy()
        # the projection on a stream of its own: on the device's default stream it would
        # queue behind the engine steps already in flight there (1-2 steps of latency)
        if self._stream is None:
            self._stream = torch.cuda.Stream(device=self.proj.device, priority=-1)
        with torch.cuda.stream(self._stream):
            return F.normalize(hd.to(self.proj.device) @ self.proj, dim=1).cpu().numpy()

    def embed_document(self, text: str, chunk_tokens: int = 256, overlap: int = 32, late: bool = True,
                       return_spans: bool = False):
        """Chunk vectors of one document: (chunk_texts, vectors [S, dim]) -- with return_spans the
        chunks' token ranges as a third entry. The document is tokenised once and cut by
        chunk_spans; it is NOT truncated to max_tokens.

        late=True: one span request per context window (span_windows over max_model_len - 1
        tokens, LLMEngine.embed_spans): a chunk's vector is the mean final hidden state of its
        tokens inside the document, so it has seen everything before it in its window, and the
        document costs one prefill per window. late=False: every chunk is embedded alone, as a
        request of its own through LLMEngine.embed -- the comparison baseline, and what a
        tensor-parallel engine (which takes no spans) falls back to. Both go through this
        embedder's projection and L2 normalisation."""
        eng = self.engine
        ids = eng.tok.encode(text)
        W = eng.max_model_len - 1
        wins = span_windows(len(ids), chunk_tokens, overlap, W, int(eng.L["span_slots"]))
        spans = [sp for _, _, w in wins for sp in w]
        texts = [eng.tok.decode(ids[a:b]) for a, b in spans]
        if not spans:
            out = ([], np.zeros((0, self.dim), np.float32))
        elif late and getattr(eng.tp, "size", 1) == 1 and not eng.cfg.async_steps:
            means = [eng.embed_spans(ids[s:e], [(a - s, b - s) for a, b in w])[1] for s, e, w in wins]
            out = (texts, self._project(np.concatenate(means, axis=0)))
        else:
            out = (texts, self._project(eng.embed([ids[a:b] for a, b in spans], pooling="mean")))
        return out + (spans,) if return_spans else out
