"""stage_device_round_vec (csrc/staging.hpp), the host staging of
fedavg_device_round_{f64,f16,bf16}, under AddressSanitizer +
UndefinedBehaviorSanitizer (no GPU): ``tests/native/segvec_fuzz.cpp`` is a
stand-alone program built by g++ and run as a child process -- key counts
1..5,000, 1..128 clients, empty keys, ``key_index`` NULL and permuted, into
buffers of exactly the reserved bytes.
"""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "mobile-federated-learning_amd" / "csrc"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_segvec_staging_fuzz_under_asan_ubsan(tmp_path):
    exe = tmp_path / "segvec_fuzz"
    cmd = [shutil.which("g++"), "-std=c++17", "-O1", "-g", *SAN, f"-I{ROOT / 'include'}", f"-I{CSRC}",
           str(ROOT / "tests" / "native" / "segvec_fuzz.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for seed in (4321, 7):
        r = subprocess.run([str(exe), "150", str(seed)], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "0 failures" in r.stdout and "ERROR" not in r.stderr, r.stdout + r.stderr
