"""bench.py driver contract over 2 ranks (gloo, tiny model on CPU).

The driver launches `torch.distributed.run --nproc-per-node N ... bench.py --gpus N --steps K
--warmup W` and reads ONE JSON line from rank 0. This runs that exact launch shape with
world_size 2 on CPU and checks the line: one line only, the BASELINE metric, agent-DP over
both ranks, the timed-step count, and tasks from both ranks' shards.
"""
import json
import os
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


import pytest


@pytest.mark.parametrize("n,launcher,rehearsal", [(2, True, None), (8, True, None), (2, False, None),
                                                  (2, True, "share-gpu"), (2, True, "hybrid")])
def test_bench_multi_rank_json_contract(tmp_path, n, launcher, rehearsal):
    """n ranks under the driver's torchrun launch shape; (2, False): `bench.py --gpus 2`
    without a launcher must start the 2 ranks itself, never silently run one. The scale-run
    evidence fields: n_gpus counts the physical devices the ranks used (0 on
    CPU), the rehearsal flags are named, and the process group's backend / world size and every
    rank's device are reported."""
    env = dict(os.environ, PILOTTAI_DIST_BACKEND="gloo", CUDA_VISIBLE_DEVICES="")
    env.pop("WORLD_SIZE", None)
    args = [os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--cpu", "--steps", "1", "--warmup", "1",
            "--workers", str(n), "--doc-words", "20"]
    args += {"share-gpu": ["--share-gpu"], "hybrid": ["--hybrid-latency", "0.01"]}.get(rehearsal, [])
    cmd = ([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
            "--master-addr", "127.0.0.1", "--master-port", str(_free_port())] if launcher else [sys.executable]) + args
    p = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    baseline = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    assert d["metric"] == baseline["metric"]
    assert d["steps"] == 1 and d["warmup"] == 1
    assert d["config"]["parallelism"] == f"agent-dp{n}"
    assert d["config"]["workers"] == n
    assert d["config"]["managers"] == 1  # ONE manager Serve over the node-wide pool
    assert d["tasks"] >= n  # one worker per rank, each completes >= 1 task per timed step
    assert len(d["llm_calls_per_rank"]) == n
    if rehearsal != "hybrid":  # (hybrid: the CPU tiny-model rank 0 is slower than the schema ranks)
        assert all(c > 0 for c in d["llm_calls_per_rank"])
    assert d["value"] > 0 and d["ms_per_step"] > 0
    for k in ("unit", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in d
    assert d["n_gpus"] == 0 and d["physical_devices"] == []  # CPU ranks: no GPU used
    assert d["rehearsal"] == rehearsal
    assert d["dist_backend"] == "gloo" and d["world_size"] == n
    assert d["devices"] == ["cpu"] * n


def _load_bench():
    import importlib.util

    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_bench_dump_outputs_full_and_step_count(tmp_path):
    """One rank (tiny model on CPU) with `--full --dump-outputs DIR`: --steps sets the number
    of timed steps (every worker completes exactly that many timed tasks), ms_per_step is the
    timed region over the steps, and DIR holds the last timed step's tasks, one row per client:
    documents, success flags, control fields and tool results as float .npy arrays within the
    64 MB limit, and the replies the caller received as task_replies.jsonl."""
    import numpy as np

    env = dict(os.environ, CUDA_VISIBLE_DEVICES="")
    env.pop("WORLD_SIZE", None)
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--cpu", "--steps", "2", "--warmup", "1",
           "--workers", "3", "--doc-words", "20", "--full", "--dump-outputs", str(out)]
    p = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["tasks"] == 2 * 3
    assert d["full"] is True and d["seed"] == _load_bench().parse([]).seed
    assert abs(d["ms_per_step"] - 1000.0 * d["seconds"] / 2) <= 0.01 * d["ms_per_step"] + 0.01
    assert d["unit"] == "tasks/s" and d["higher_is_better"] is True and d["dtype"] == "bf16"
    files = sorted(f for f in os.listdir(out))
    assert files == ["task_control.npy", "task_document_bytes.npy", "task_replies.jsonl", "task_success.npy",
                     "task_tool_results_bytes.npy"]
    arrs = {f[:-4]: np.load(out / f) for f in files if f.endswith(".npy")}
    assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 * 2**20
    assert d["dumped_outputs"] == {k: list(a.shape) for k, a in arrs.items()}
    assert arrs["task_success"].tolist() == [1.0, 1.0, 1.0]  # a failed task ends the run
    # one row per client, in order; the fixed policy's control flow: one iteration, one executed
    # echo step that succeeded, can_execute, one selected tool, a success verdict
    assert arrs["task_control"].tolist() == [[0.0, c, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0] for c in (0.0, 1.0, 2.0)]
    for row in arrs["task_tool_results_bytes"]:  # whole JSON, nothing cut
        assert json.loads(_row_text(row)) == [{"output": {"echo": {}}, "status": "success"}]
    docs = [_row_text(row) for row in arrs["task_document_bytes"]]
    words = set(_load_bench()._WORDS)
    assert len(set(docs)) == 3 and all(len(t.split()) == 20 and set(t.split()) <= words for t in docs)
    # the model's replies, as the caller received them, beside the arrays: one line per client
    replies = [json.loads(ln) for ln in open(out / "task_replies.jsonl")]
    assert [r["client"] for r in replies] == [0, 1, 2] and [r["document"] for r in replies] == docs
    for r in replies:
        assert r["evaluation"]["success"] is True and r["analysis"]["can_execute"] is True
        assert r["output"][0]["step"]["tool"] == "echo"


def _row_text(row) -> str:
    import numpy as np

    return bytes(row[row >= 0].astype(np.uint8)).decode("utf-8")


def test_bench_inputs_repeat_from_run_to_run(tmp_path):
    """The documents a run submits follow --seed and nothing else: two runs with the same
    arguments dump the same documents (and the same arrays altogether), a run with another
    seed dumps other documents. Three one-step runs of the tiny CPU model, side by side."""
    import numpy as np

    env = dict(os.environ, CUDA_VISIBLE_DEVICES="")
    env.pop("WORLD_SIZE", None)
    runs = {"a": [], "b": [], "c": ["--seed", "7"]}
    procs = {k: subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--cpu", "--steps", "1",
                                  "--warmup", "0", "--workers", "2", "--doc-words", "20",
                                  "--dump-outputs", str(tmp_path / k), *extra],
                                 cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for k, extra in runs.items()}
    lines = {}
    for k, p in procs.items():
        out, err = p.communicate(timeout=900)
        assert p.returncode == 0, err[-3000:]
        lines[k] = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][0])
    assert lines["a"]["seed"] == lines["b"]["seed"] != lines["c"]["seed"] == 7
    names = sorted(f for f in os.listdir(tmp_path / "a") if f.endswith(".npy"))
    arrs = {k: {f: np.load(tmp_path / k / f) for f in names} for k in runs}
    for f in names:
        assert arrs["a"][f].shape == arrs["b"][f].shape and (arrs["a"][f] == arrs["b"][f]).all(), f
    docs = {k: [_row_text(r) for r in arrs[k]["task_document_bytes.npy"]] for k in runs}
    assert docs["a"] == docs["b"] and not set(docs["a"]) & set(docs["c"])


def test_bench_device_identity_counts_physical_cards():
    """n_gpus is the number of DISTINCT physical cards over the ranks (unit check of the
    identity helper on fake device properties)."""
    import importlib.util
    import types

    import torch

    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert bench._device_identity(torch.device("cpu")) == {"device": "cpu", "physical": None}
    props = types.SimpleNamespace(pci_domain_id=0, pci_bus_id=0x75, pci_device_id=0, name="MI355X", uuid="u")
    orig = torch.cuda.get_device_properties
    try:
        torch.cuda.get_device_properties = lambda i: props
        ident = bench._device_identity(torch.device("cuda", 3))
    finally:
        torch.cuda.get_device_properties = orig
    assert ident["device"] == "cuda:3" and ident["physical"] == "pci:0000:75:00"


def test_bench_node_memory_is_one_sharded_store(tmp_path):
    """in node mode `--memory-rows R` is ONE node-wide store -- R rows in
    total, sharded over the ranks (not R per rank) -- and every agent step's lookups go through
    it (2 gloo ranks, tiny model on CPU)."""
    env = dict(os.environ, PILOTTAI_DIST_BACKEND="gloo", CUDA_VISIBLE_DEVICES="")
    env.pop("WORLD_SIZE", None)
    R = 20000
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "bench.py"), "--gpus", "2", "--cpu", "--steps", "1", "--warmup", "1",
           "--workers", "2", "--doc-words", "20", "--memory-rows", str(R)]
    p = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][0])
    m = d["memory"]
    assert m["store"] == "node-sharded"
    per = m["rows_per_rank"]
    assert len(per) == 2 and R <= sum(per) == m["rows_total"] < R + 1000
    assert all(R // 2 <= r < R // 2 + 1000 for r in per)  # a shard each, plus write-backs
    assert m["lookups"] > 0 and m["node_rounds"] > 0
    # the agents' write-backs reach the node store (none failed), and
    # lookups return rows held by the other rank's shard
    assert m["stores"] > 0 and m["store_failures"] == 0 and m["lookup_failures"] == 0
    assert m["node_hits"] > 0 and m["node_remote_hits"] > 0


def test_bench_agent_dp_over_tp_groups(tmp_path):
    """`--gpus 4 --tp 2` runs 2 agent-DP replicas, each a TP=2 engine (its
    TP rank 1 follows the driver's steps); the node plane and the clients see 2 replicas, the
    JSON line names the layout, and every rank's device is reported (4 gloo ranks on CPU)."""
    env = dict(os.environ, PILOTTAI_DIST_BACKEND="gloo", CUDA_VISIBLE_DEVICES="")
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "4",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "bench.py"), "--gpus", "4", "--tp", "2", "--cpu", "--steps", "1", "--warmup", "1",
           "--workers", "4", "--doc-words", "20"]
    p = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["config"]["parallelism"] == "agent-dp2-tp2"
    assert d["config"]["managers"] == 1 and d["tasks"] >= 4
    assert len(d["llm_calls_per_rank"]) == 2 and all(c > 0 for c in d["llm_calls_per_rank"])
    assert d["world_size"] == 4 and d["devices"] == ["cpu"] * 4
    st = d["tp_selftest"]  # the start-up all-reduce round trip of the TP groups
    assert st["ok"] and st["tp"] == 2 and st["us_64x4096"] > 0 and st["us_2048x4096"] > 0
