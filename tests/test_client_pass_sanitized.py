"""The client passes' HIP-free plan header (``csrc/client_pass_plan.hpp``: the
fp32 statistics, the bf16 / fp16 / fp64 statistics and the fused SGD step)
under AddressSanitizer + UndefinedBehaviorSanitizer (no GPU), built as
tests/test_native_sanitized.py builds its programs: g++ compiles
``tests/native/client_pass_check.cpp``, a stand-alone program, with
``-fsanitize=address,undefined``; it fuzzes key counts 1..5,000, empty keys
and numels around the unit edges, fills tables in buffers of exactly the
reserved bytes for both table entries and element sizes 2, 4 and 8, checks
every written byte and every ``unit_start``, and that each key-list check
refuses exactly the constructed bad key.
"""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "mobile-federated-learning_amd" / "csrc"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def _gxx():
    return shutil.which("g++")


@pytest.mark.skipif(_gxx() is None, reason="g++ not found")
def test_client_pass_plan_under_asan_ubsan(tmp_path):
    exe = tmp_path / "client_pass_check"
    cmd = [_gxx(), "-std=c++17", "-O1", "-g", *SAN, f"-I{CSRC}",
           str(ROOT / "tests" / "native" / "client_pass_check.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for seed in (1234, 99):
        r = subprocess.run([str(exe), "60", str(seed)], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stdout + r.stderr
        assert " 0 failures" in r.stdout and "ERROR" not in r.stderr, r.stdout + r.stderr
