"""libfedavg_amd_clientwide.so (include/fedavg_amd_clientwide.h), the sixteenth native library, in a tuple of its own
beside the fifteen ``described_libs()`` keeps.  CPU only: everything here is validated before any HIP call."""
import dataclasses
import importlib.util
from pathlib import Path

import numpy as np
import pytest

from mfl_amd import _lib, build, cohort_train
from mfl_amd.client_passes import wide_limits, wide_max_slices, wide_slice_rows
from test_abi import _exported, declared_functions

HERE = Path(__file__).parent
HEADER = "fedavg_amd_clientwide.h"
ENTRY = "fedavg_client_cohort_wide_f32"
DECLARED = ("fedavg_clientwide_abi_version", "fedavg_clientwide_last_error", "fedavg_client_wide_limits",
            "fedavg_client_wide_slice_rows", "fedavg_client_wide_max_slices", "fedavg_client_wide_workspace_bytes", ENTRY)


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load_clientwide()


def test_the_sixteenth_has_a_table_of_its_own_after_the_fifteen(lib):
    assert set(build.WIDE_BY_KEY) == {"clientwide"} == set(_lib._WIDE_BINDING)
    d = build.WIDE_BY_KEY["clientwide"]
    assert len(build.described_libs()) == 15 and build.described_libs()[-1] is build.COSPLIT_LIBS[0]
    assert build.WIDE_LIBS == (d,) and build.every_described_lib() == build.described_libs() + build.WIDE_LIBS
    assert d.path == build.CLIENTWIDE_LIB_PATH and d.header == HEADER
    assert d.units == ("fedavg_client_wide.hip",) and d.needs == "" and d.link == ()
    assert d.defines == build.COSPLIT_LIBS[0].defines  # the cosplit library's flags
    assert set(d.sources) <= set(build.sources()) and all(src.exists() for src in d.sources)
    assert build.later_up_to_date()


def test_exports_are_exactly_the_header_and_the_kernels_the_listed_ones(lib):
    declared = declared_functions((HEADER,))
    assert declared == sorted(DECLARED) == _exported(build.CLIENTWIDE_LIB_PATH) == sorted(_lib.CLIENTWIDE_SIGNATURES)
    assert lib.fedavg_clientwide_abi_version() == _lib.CLIENTWIDE_ABI_VERSION == 1
    data = build.CLIENTWIDE_LIB_PATH.read_bytes()
    assert b"gfx950" in data and b"getenv" not in data
    spec = importlib.util.spec_from_file_location("kernel_inventory", HERE.parent / "scripts" / "kernel_inventory.py")
    inv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(inv)
    if inv.have_tools():
        listed = (HERE / "clientwide_kernels.txt").read_text().splitlines()
        found = inv.inventory(build.CLIENTWIDE_LIB_PATH)
        # setup, gradient x direct loads, sum, step x Adam, track
        assert sorted(found) == listed and len(listed) == 7
        assert all(row["scratch"] == 0 for row in found.values())


def test_load_refuses_another_abi_version(lib, monkeypatch):
    d = build.WIDE_BY_KEY["clientwide"]
    monkeypatch.setitem(build.WIDE_BY_KEY, "clientwide", dataclasses.replace(d, abi=(d.abi[0], 2)))
    monkeypatch.setattr(_lib, "_clientwide", None)
    with pytest.raises(_lib.FedAvgLibraryError, match="ABI version 1 != expected 2; rebuild the library"):
        _lib.load_clientwide()
    assert _lib._clientwide is None


def test_limits_and_the_slices_a_workgroup_may_walk(lib):
    assert wide_limits() == (4096, 16384, 4096, 128, 128 * 4097) and wide_slice_rows() == 64
    most = [wide_max_slices(C) for C in range(2, 129)]
    assert all(a >= b for a, b in zip(most, most[1:])) and most[-1] >= 1
    # the header's rule: the dz stores beside the two unit buffers inside the streamed loop's LDS budget
    budget = 132864 - 2 * 64 * 132 * 4
    assert most == [min(15, budget // (64 * (16 * -(-C // 16) + 1) * 4)) for C in range(2, 129)]
    assert wide_max_slices(1) == wide_max_slices(129) == 0


def workspace_bytes(lib, Bs, D, C, q, optimizer):
    sizes = np.asarray(Bs, dtype=np.int64)
    return lib.fedavg_client_wide_workspace_bytes(sizes.ctypes.data, len(sizes), D, C, q, optimizer)


# the header's formula: 104 K + 24 N + 40 K NC + 4 P (N + K (2 + 3 a))
@pytest.mark.parametrize("Bs, D, C, q, optimizer", [
    ([1], 784, 62, 1, 0), ([64, 65, 1, 129, 323], 784, 62, 2, 1), ([600] * 100, 3072, 100, 1, 0),
    ([16384, 1], 4096, 128, 1, 1), ([16384], 1, 2, 15, 1), ([134, 3], 1025, 17, 3, 0)])
def test_workspace_bytes_is_the_headers_formula(lib, Bs, D, C, q, optimizer):
    K, P, N = len(Bs), C * D + C, sum(-(-(-(-b // 64)) // q) for b in Bs)
    want = 104 * K + 24 * N + 40 * K * -(-P // 8192) + 4 * P * (N + K * (2 + 3 * optimizer))
    assert workspace_bytes(lib, Bs, D, C, q, optimizer) == want
    assert workspace_bytes(lib, Bs, D, C, wide_max_slices(C) + 1, optimizer) == 0


ADAM = dict(optimizer=1, form=15)


@pytest.mark.parametrize("change, code, words", [
    (dict(D=4097), "EINVAL", b"D = 4097 outside [1, 4096]"),
    (dict(C=1), "EINVAL", b"C = 1 outside [2, 128]"), (dict(C=129), "EINVAL", b"C = 129 outside [2, 128]"),
    (dict(slices_per_group=0), "EINVAL", b"slices_per_group = 0 outside [1, 3] at C = 62"),
    (dict(slices_per_group=4), "EINVAL", b"slices_per_group = 4 outside [1, 3] at C = 62"),
    (dict(B2=16385), "EINVAL", b"entry 2: B = 16385 outside [1, 16384]"),
    (dict(model=None), "EINVAL", b"null"), (dict(workspace=None), "EINVAL", b"null"),
    (dict(ADAM, coef=None), "EINVAL", b"null coef"), (dict(x1=None), "EINVAL", b"entry 1: null x or y"),
    (dict(rec=324), "EALIGN", b"8-B"), (dict(x1=130), "EALIGN", b"entry 1: x must be 4-B"),
    (dict(workspace_bytes=-1), "EINVAL", b"bytes below the"),  # one byte short
    (dict(ADAM, workspace_bytes=0), "EINVAL", b"bytes below the"),  # Adam's m, v, vmax are missing
    (dict(optimizer=2), "EMODE", b"optimizer 2 is neither"), (dict(activation=2), "EMODE", b"activation 2"),
    (dict(ld=48669), "EINVAL", b"ld = 48669 below P = 48670"),
    (dict(), "EINVAL", b"clients is not pinned host memory"),  # well-formed: as far as the checks that need a GPU
])
def test_cohort_wide_entry_refusals(lib, change, code, words):
    buf = np.zeros(256, np.float64)  # ordinary host memory: the table in it is well-formed and not pinned
    base = buf.ctypes.data
    a = dict(model=0, rows=64, ld=48672, clients=1024, K=3, D=784, C=62, iters=5, activation=0, optimizer=0, lr=0.05,
             lr_ratio=50.0, form=1, coef=256, rec=320, slices_per_group=2, workspace=448, workspace_bytes=0, stream=None)
    entries = {f"{f}{g}": v for g in range(3) for f, v in (("x", 128), ("y", 192), ("B", 256 - g), ("row", g))}
    for k in list(change):
        if k in entries:
            entries[k] = change.pop(k)
    a.update(change)
    a["workspace_bytes"] += workspace_bytes(lib, [256, 255, 254], 784, 62, 2, 0)  # four slices: two workgroups each
    table = buf[128:140].view(np.int64).reshape(3, 4)
    for g in range(3):
        x, y = entries[f"x{g}"], entries[f"y{g}"]
        table[g] = (0 if x is None else base + x, 0 if y is None else base + y, entries[f"B{g}"], entries[f"row{g}"])
    for k in ("model", "rows", "clients", "coef", "rec", "workspace"):  # offsets into the buffer become addresses
        a[k] = None if a[k] is None else base + a[k]
    assert getattr(lib, ENTRY)(*a.values()) == getattr(_lib, "FEDAVG_" + code)
    msg = lib.fedavg_clientwide_last_error()
    assert msg.startswith(ENTRY.encode()) and words in msg, msg
    with pytest.raises(_lib.FedAvgLibraryError, match=ENTRY):
        _lib.check_clientwide(-1, ENTRY)


def test_wide_and_split_together_are_refused_before_anything_is_read():
    with pytest.raises(ValueError, match="wide=True and split=True"):
        cohort_train([object()], None, 1, wide=True, split=True)
