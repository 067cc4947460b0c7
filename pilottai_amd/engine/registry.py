"""Process-wide engine registry: one LLMEngine per model per process (= per GPU)."""
from __future__ import annotations

import threading
from typing import Dict, Optional

from .engine import EngineConfig, LLMEngine

_ENGINES: Dict[str, LLMEngine] = {}
_LOCK = threading.Lock()
_DEFAULTS: Dict[str, dict] = {}


def configure_engine(model: str, **overrides):
    """Set EngineConfig overrides used when `model` is first instantiated."""
    _DEFAULTS[model.lower()] = dict(overrides)


def register_engine(model: str, engine: LLMEngine):
    with _LOCK:
        _ENGINES[model.lower()] = engine


def get_engine(model: str = "llama-3-8b", **overrides) -> LLMEngine:
    key = model.lower()
    with _LOCK:
        eng = _ENGINES.get(key)
        if eng is not None and "weight_quant" in overrides:
            have = getattr(eng.model, "weight_quant", None)
            if have != overrides["weight_quant"]:
                raise ValueError(f"this process already holds an engine for {key!r} with weight_quant={have!r} "
                                 f"(asked for {overrides['weight_quant']!r}): one engine per model per process")
        if eng is not None and "host_cache_gb" in overrides:
            # the effective size: an engine sized by host_cache_blocks has no host_cache_gb to compare
            have = int(getattr(eng, "host_cache_blocks", 0))
            want = int(float(overrides["host_cache_gb"]) * (1 << 30)) // max(1, int(getattr(eng, "kv_block_bytes", 1)))
            if have != want:
                raise ValueError(f"this process already holds an engine for {key!r} with a host KV tier of {have} "
                                 f"blocks (host_cache_gb={overrides['host_cache_gb']!r} asks for {want}): "
                                 "one engine per model per process")
        if eng is None:
            kw = dict(_DEFAULTS.get(key, {}))
            kw.update(overrides)
            eng = LLMEngine(EngineConfig(model=key, **kw))
            _ENGINES[key] = eng
        return eng


def shutdown_engines():
    with _LOCK:
        for e in _ENGINES.values():
            e.stop()
        _ENGINES.clear()


def peek_engine(model: str) -> Optional[LLMEngine]:
    return _ENGINES.get(model.lower())
