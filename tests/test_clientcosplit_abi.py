"""libfedavg_amd_clientcosplit.so (include/fedavg_amd_clientcosplit.h), the fifteenth native library, in a tuple of its
own and held as test_clientsplit_abi.py holds the fourteenth.  CPU only: everything here is validated before any HIP
call."""
import dataclasses
import importlib.util
from pathlib import Path

import numpy as np
import pytest

from mfl_amd import _lib, build
from test_abi import _exported, declared_functions

HERE = Path(__file__).parent
HEADER = "fedavg_amd_clientcosplit.h"
ENTRY = "fedavg_client_cohort_split_f32"
DECLARED = ("fedavg_clientcosplit_abi_version", "fedavg_clientcosplit_last_error",
            "fedavg_client_cosplit_workspace_bytes", ENTRY)


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load_clientcosplit()


def test_the_fifteenth_has_a_table_of_its_own_at_the_end_of_the_described(lib):
    assert set(build.COSPLIT_BY_KEY) == {"clientcosplit"} == set(_lib._COSPLIT_BINDING)
    d = build.COSPLIT_BY_KEY["clientcosplit"]
    assert d is build.COSPLIT_LIBS[0] is build.described_libs()[-1] and len(build.described_libs()) == 15
    assert d.path == build.CLIENTCOSPLIT_LIB_PATH and d.header == HEADER
    assert d.units == ("fedavg_client_cosplit.hip",) and d.needs == "" and d.link == ()
    assert set(d.sources) <= set(build.sources()) and all(src.exists() for src in d.sources)
    assert build.later_up_to_date()


def test_exports_are_exactly_the_header_and_the_kernels_the_listed_ones(lib):
    declared = declared_functions((HEADER,))
    assert declared == sorted(DECLARED) == _exported(build.CLIENTCOSPLIT_LIB_PATH) == sorted(_lib.CLIENTCOSPLIT_SIGNATURES)
    assert lib.fedavg_clientcosplit_abi_version() == _lib.CLIENTCOSPLIT_ABI_VERSION == 1
    data = build.CLIENTCOSPLIT_LIB_PATH.read_bytes()
    assert b"gfx950" in data and b"getenv" not in data
    spec = importlib.util.spec_from_file_location("kernel_inventory", HERE.parent / "scripts" / "kernel_inventory.py")
    inv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(inv)
    if inv.have_tools():
        listed = (HERE / "clientcosplit_kernels.txt").read_text().splitlines()
        found = inv.inventory(build.CLIENTCOSPLIT_LIB_PATH)
        assert sorted(found) == listed and len(listed) == 5  # setup, gradient x direct loads, step x Adam
        assert all(row["scratch"] == 0 for row in found.values())


def test_load_refuses_another_abi_version(lib, monkeypatch):
    d = build.COSPLIT_BY_KEY["clientcosplit"]
    monkeypatch.setitem(build.COSPLIT_BY_KEY, "clientcosplit", dataclasses.replace(d, abi=(d.abi[0], 2)))
    monkeypatch.setattr(_lib, "_clientcosplit", None)
    with pytest.raises(_lib.FedAvgLibraryError, match="ABI version 1 != expected 2; rebuild the library"):
        _lib.load_clientcosplit()
    assert _lib._clientcosplit is None


def workspace_bytes(lib, Bs, D, C, q, optimizer):
    sizes = np.asarray(Bs, dtype=np.int64)
    return lib.fedavg_client_cosplit_workspace_bytes(sizes.ctypes.data, len(sizes), D, C, q, optimizer)


# the header's formula, R as test_clientsplit_abi.py pins it: 104 K + 24 N + 4 P (N + K (1 + 3 a))
@pytest.mark.parametrize("Bs, D, R, C, q, optimizer", [
    ([1], 784, 32, 10, 1, 0), ([32, 33, 1, 65, 163], 784, 32, 10, 1, 1), ([32, 33, 1, 65, 163], 784, 32, 10, 2, 0),
    ([600] * 100, 784, 32, 10, 1, 0), ([16384, 1], 1024, 32, 16, 7, 1), ([16384], 1, 256, 2, 1 << 40, 1),
    ([134, 3], 250, 128, 5, 3, 1)])
def test_workspace_bytes_is_the_headers_formula(lib, Bs, D, R, C, q, optimizer):
    K, P, N = len(Bs), C * D + C, sum(-(-(-(-b // R)) // q) for b in Bs)
    assert workspace_bytes(lib, Bs, D, C, q, optimizer) == 104 * K + 24 * N + 4 * P * (N + K * (1 + 3 * optimizer))


@pytest.mark.parametrize("Bs, D, C, q, optimizer", [
    ([], 784, 10, 1, 0), ([1] * 4097, 784, 10, 1, 0), ([0], 784, 10, 1, 0), ([5, 16385], 784, 10, 1, 0),
    ([5], 0, 10, 1, 0), ([5], 1025, 10, 1, 0), ([5], 784, 1, 1, 0), ([5], 784, 17, 1, 0), ([5], 784, 10, 0, 0),
    ([5], 784, 10, 1, 2), ([5], 784, 10, 1, -1)])
def test_workspace_bytes_is_0_outside_the_ranges(lib, Bs, D, C, q, optimizer):
    assert workspace_bytes(lib, Bs, D, C, q, optimizer) == 0
    assert lib.fedavg_client_cosplit_workspace_bytes(None, 1, 784, 10, 1, 0) == 0


ADAM = dict(optimizer=1, form=15)


@pytest.mark.parametrize("change, code, words", [
    (dict(model=None), "EINVAL", b"null"), (dict(rows=None), "EINVAL", b"null"), (dict(clients=None), "EINVAL", b"null"),
    (dict(rec=None), "EINVAL", b"null"), (dict(workspace=None), "EINVAL", b"null"),
    (dict(ADAM, coef=None), "EINVAL", b"null coef"), (dict(x1=None), "EINVAL", b"entry 1: null x or y"),
    (dict(ld=7849), "EINVAL", b"ld = 7849 below P = 7850"), (dict(iters=-1), "EINVAL", b"negative iteration count"),
    (dict(K=0), "EINVAL", b"K = 0 outside [1, 4096]"), (dict(K=4097), "EINVAL", b"K = 4097 outside"),
    (dict(D=0), "EINVAL", b"D = 0 outside [1, 1024]"), (dict(D=1025), "EINVAL", b"D = 1025 outside [1, 1024]"),
    (dict(C=1), "EINVAL", b"C = 1 outside [2, 16]"), (dict(C=17), "EINVAL", b"C = 17 outside"),
    (dict(B1=0), "EINVAL", b"entry 1: B = 0 outside [1, 16384]"), (dict(B2=16385), "EINVAL", b"entry 2: B = 16385"),
    (dict(row1=0), "EINVAL", b"entry 1: row 0 used twice"), (dict(row1=3), "EINVAL", b"entry 1: row 3 outside [0, 3)"),
    (dict(slices_per_group=0), "EINVAL", b"slices_per_group = 0 below 1"),
    (dict(activation=2), "EMODE", b"activation 2"), (dict(optimizer=2), "EMODE", b"optimizer 2"),
    (dict(form=2), "EMODE", b"form 2"), (dict(optimizer=1, form=16), "EMODE", b"form 16"),
    (dict(model=2), "EALIGN", b"4-B"), (dict(rows=66), "EALIGN", b"4-B"), (dict(clients=1028), "EALIGN", b"8-B aligned"),
    (dict(rec=324), "EALIGN", b"8-B"), (dict(ADAM, coef=260), "EALIGN", b"8-B"), (dict(workspace=452), "EALIGN", b"workspace 8-B"),
    (dict(x1=130), "EALIGN", b"entry 1: x must be 4-B"), (dict(y2=196), "EALIGN", b"entry 2: x must be 4-B, y 8-B"),
    (dict(workspace_bytes=-1), "EINVAL", b"bytes below the"),  # one byte short
    (dict(B2=129, workspace_bytes=0), "EINVAL", b"bytes below the"),  # entry 2 alone has a third workgroup
    (dict(ADAM, workspace_bytes=0), "EINVAL", b"bytes below the"),  # Adam's m, v, vmax are missing
    (dict(), "EINVAL", b"clients is not pinned host memory"),  # well-formed: as far as the checks that need a GPU
    (dict(ADAM, workspace_bytes=3 * 12 * 7850), "EINVAL", b"clients is not pinned host memory"),
])
def test_cohort_split_entry_refusals(lib, change, code, words):
    buf = np.zeros(256, np.float64)  # ordinary host memory: the table in it is well-formed and not pinned
    base = buf.ctypes.data
    a = dict(model=0, rows=64, ld=7872, clients=1024, K=3, D=784, C=10, iters=5, activation=0, optimizer=0, lr=0.05,
             lr_ratio=50.0, form=1, coef=256, rec=320, slices_per_group=2, workspace=448, workspace_bytes=0, stream=None)
    entries = {f"{f}{g}": v for g in range(3) for f, v in (("x", 128), ("y", 192), ("B", 128 - g), ("row", g))}
    for k in list(change):
        if k in entries:
            entries[k] = change.pop(k)
    a.update(change)
    a["workspace_bytes"] += workspace_bytes(lib, [128, 127, 126], 784, 10, 2, 0)  # four slices of 32 rows: two workgroups each
    table = buf[128:140].view(np.int64).reshape(3, 4)
    for g in range(3):
        x, y = entries[f"x{g}"], entries[f"y{g}"]
        table[g] = (0 if x is None else base + x, 0 if y is None else base + y, entries[f"B{g}"], entries[f"row{g}"])
    for k in ("model", "rows", "clients", "coef", "rec", "workspace"):  # offsets into the buffer become addresses
        a[k] = None if a[k] is None else base + a[k]
    assert getattr(lib, ENTRY)(*a.values()) == getattr(_lib, "FEDAVG_" + code)
    msg = lib.fedavg_clientcosplit_last_error()
    assert msg.startswith(ENTRY.encode()) and words in msg, msg
    with pytest.raises(_lib.FedAvgLibraryError, match=ENTRY):
        _lib.check_clientcosplit(-1, ENTRY)
