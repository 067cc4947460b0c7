"""The prefix cache's host tier under AddressSanitizer + UndefinedBehaviorSanitizer.

Builds csrc/runtime/tests/stress_host_tier.cpp together with the runtime sources with
-fsanitize=address,undefined and runs it: a scheduler with 24 device blocks and 12 host slots,
a memory model of one tag per KV entry, and the check that every sequence of every step reads
the KV of its own prefix after the step's spills, fills, copies and writes. Any sanitizer
report, a wrong tag, or a run without spills, fills, host-slot evictions and preemptions fails
the test. CPU tier.
"""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT = os.path.join(ROOT, "csrc", "runtime")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_host_tier_stress_under_asan_ubsan():
    srcs = [os.path.join(RT, "tests", "stress_host_tier.cpp")] + [
        os.path.join(RT, f) for f in ("scheduler.cpp", "block_manager.cpp", "grammar.cpp", "tokenizer.cpp")]
    flags = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all"]
    with tempfile.TemporaryDirectory() as d:
        # whether the toolchain has the sanitizer runtimes is asked of a trivial program, so that
        # no compile error of the driver itself can pass for a missing runtime
        probe = os.path.join(d, "probe.cpp")
        with open(probe, "w") as f:
            f.write("int main() { return 0; }\n")
        r = subprocess.run(["g++", *flags, probe, "-o", os.path.join(d, "probe")], capture_output=True, text=True,
                           timeout=120)
        if r.returncode != 0:
            pytest.skip("toolchain has no AddressSanitizer / UndefinedBehaviorSanitizer runtime")
        exe = os.path.join(d, "stress_host_tier")
        r = subprocess.run(["g++", *flags, f"-I{RT}", *srcs, "-o", exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-4000:]
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
                   UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
        r = subprocess.run([exe, "6"], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
        assert "host tier stress: ok" in r.stdout
        runs = re.findall(r"host tier seed \d+: (\d+) steps, (\d+) spills, (\d+) fills, (\d+) host evictions, "
                          r"(\d+) preemptions", r.stdout)
        assert len(runs) == 6
        for steps, spills, fills, evicted, preempted in runs:
            assert int(steps) > 500 and min(int(spills), int(fills), int(evicted), int(preempted)) > 0
