"""The case table of the C-ABI contract tests (tests/abi_cases.py), checked
without a GPU: every entry point of the three product headers that takes a
stream has cases, and every case's inputs and expectations can be drawn."""
import re
from pathlib import Path

import numpy as np
import pytest

import abi_cases as A

INCLUDE = Path(__file__).resolve().parents[1] / "include"
HEADERS = ("fedavg_amd.h", "fedavg_amd_fusedvec.h", "fedavg_amd_segvec.h")


def stream_entries(text):
    """Names of the prototypes with a `void* stream` parameter."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return [m.group(1) for m in re.finditer(r"\b(fedavg_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S)
            if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2))]


def test_the_parser_finds_prototypes():
    sample = "/* int fedavg_not(void* stream); */ int fedavg_a(int x,\n void* stream);\nint64_t fedavg_b(int64_t K);"
    assert stream_entries(sample) == ["fedavg_a"]


def test_every_stream_entry_has_cases():
    names = [n for h in HEADERS for n in stream_entries((INCLUDE / h).read_text())]
    assert len(names) >= 36 and len(set(names)) == len(names)
    for must in ("fedavg_reduce_f32_timed", "fedavg_round_f32", "fedavg_device_round_bf16", "fedavg_reduce_sqdist_f64"):
        assert must in names
    covered = {c.entry for c in A.CASES}
    missing = sorted(set(names) - covered)
    assert not missing, f"entry points without contract cases in tests/abi_cases.py: {missing}"
    assert covered <= set(names), sorted(covered - set(names))


def test_the_multi_launch_shape_round_splits():
    """The issue's search at K = 2 finds nothing (up to 4 clients take one
    launch by rule); the table's shape is one the schedule splits into rounds
    on a 256-CU device, with a kernel whose launch size no occupancy query sets."""
    assert A.multi_launch_P(2) is None
    K, P = A.MULTI_LAUNCH
    sc = A._lib.f32_schedule(K, P)
    assert sc["launches"] >= 2 and sc["kernel"] == "reduce_f32x4_var_kernel", sc
    assert any(c.name == f"reduce_f32-multilaunch-{K}x{P}" for c in A.CASES)


def _has_special_rows(case):
    return case.entry in ("fedavg_fpf_index_f32", "fedavg_fpf_index_f64", "fedavg_fpf_index_lru")


@pytest.mark.parametrize("case", A.CASES, ids=lambda c: c.name)
def test_case_builds_without_a_gpu(case):
    inp = case.build(np.random.default_rng(1))
    roles = {b.role for b in inp.bufs.values()}
    assert "out" in roles
    exp = case.expected(inp)
    assert set(exp) == set(inp.cmp) and exp
    for name, want in exp.items():
        buf = inp.bufs[name]
        assert buf.role == "out" and buf.data is not None
        want = np.asarray(want)
        if inp.cmp[name] not in ("pair32", "between64"):
            assert want.shape == buf.data.shape and want.dtype == buf.data.dtype, (name, want.shape, buf.data.shape)
        vals = A._as_f64(want, "bf16") if (want.dtype == np.uint16 and "bf16" in case.entry) else want.astype(np.float64)
        if not _has_special_rows(case):  # the special-value FPF rows keep their own rules (NaN / inf scrubbed to 0)
            written = A.bits(want) != A.bits(buf.data)  # padding the call leaves alone may hold NaN
            assert written.any() and np.isfinite(vals[written]).all(), name
        if vals.size > 1:
            assert np.unique(vals[np.isfinite(vals)]).size > 1, f"{name}: a constant expectation proves nothing"
    for name, buf in inp.bufs.items():
        if buf.ptr_of is not None:
            assert {p for p in buf.ptr_of if p} <= set(inp.bufs), name
        assert (buf.role == "ws") == (buf.data is None), name
    # a second draw gives other data of the same shapes (the dirty-scratch and two-stream tests rely on it)
    again = case.build(np.random.default_rng(2))
    assert set(again.bufs) == set(inp.bufs)
    differs = False
    for name, buf in inp.bufs.items():
        if buf.data is not None:
            assert again.bufs[name].data.shape == buf.data.shape, name
            differs |= (buf.role == "value" or buf.inout) and again.bufs[name].data.tobytes() != buf.data.tobytes()
    assert differs
