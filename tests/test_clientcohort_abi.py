"""libfedavg_amd_clientcohort.so (include/fedavg_amd_clientcohort.h), the eleventh native library, held as
test_clientstream_abi.py holds the tenth.  CPU only: nulls, sizes, codes, alignments and the client table's contents
are validated before any HIP call."""
import dataclasses
import importlib.util
from pathlib import Path

import numpy as np
import pytest

from mfl_amd import _lib, build, client_passes
from test_abi import _exported, declared_functions

HERE = Path(__file__).parent
HEADER = "fedavg_amd_clientcohort.h"
ENTRY = "fedavg_client_cohort_f32"
DECLARED = ("fedavg_clientcohort_abi_version", "fedavg_clientcohort_last_error", "fedavg_client_cohort_limits", ENTRY)


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load_clientcohort()


def test_the_ten_stay_and_the_eleventh_has_a_table_of_its_own(lib, monkeypatch):
    assert len(build.BUILT_LIBS) == 8 and set(build.STREAM_BY_KEY) == {"clientstream"} == set(_lib._STREAM_BINDING)
    assert set(build.COHORT_BY_KEY) == {"clientcohort"} == set(_lib._COHORT_BINDING)
    d = build.COHORT_BY_KEY["clientcohort"]
    assert d is build.COHORT_LIBS[0] and d.path == build.CLIENTCOHORT_LIB_PATH and d.header == HEADER
    assert d.units == ("fedavg_client_cohort.hip",) and d.needs == "" and d.link == ()
    assert set(d.sources) <= set(build.sources()) and all(src.exists() for src in d.sources)
    assert build.later_up_to_date()
    monkeypatch.setattr(build, "COHORT_LIBS", (dataclasses.replace(d, file="libfedavg_amd_no_such.so"),))
    assert not build.later_up_to_date()


def test_exports_are_exactly_the_header_and_the_kernels_the_listed_ones(lib):
    declared = declared_functions((HEADER,))
    assert declared == sorted(DECLARED) == _exported(build.CLIENTCOHORT_LIB_PATH) == sorted(_lib.CLIENTCOHORT_SIGNATURES)
    assert lib.fedavg_clientcohort_abi_version() == _lib.CLIENTCOHORT_ABI_VERSION == 1
    assert client_passes.cohort_limits() == (4096, *client_passes.linear_stream_limits()[:3])
    data = build.CLIENTCOHORT_LIB_PATH.read_bytes()
    assert b"gfx950" in data and b"getenv" not in data
    spec = importlib.util.spec_from_file_location("kernel_inventory", HERE.parent / "scripts" / "kernel_inventory.py")
    inv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(inv)
    if inv.have_tools():
        listed = (HERE / "clientcohort_kernels.txt").read_text().splitlines()
        assert sorted(inv.inventory(build.CLIENTCOHORT_LIB_PATH)) == listed and len(listed) == 4  # Adam x direct loads


def test_load_refuses_another_abi_version(lib, monkeypatch):
    d = build.COHORT_BY_KEY["clientcohort"]
    monkeypatch.setitem(build.COHORT_BY_KEY, "clientcohort", dataclasses.replace(d, abi=(d.abi[0], 2)))
    monkeypatch.setattr(_lib, "_clientcohort", None)
    with pytest.raises(_lib.FedAvgLibraryError, match="ABI version 1 != expected 2; rebuild the library"):
        _lib.load_clientcohort()
    assert _lib._clientcohort is None


@pytest.mark.parametrize("change, code, words", [
    (dict(model=None), "EINVAL", b"null"), (dict(rows=None), "EINVAL", b"null"), (dict(clients=None), "EINVAL", b"null"),
    (dict(rec=None), "EINVAL", b"null"), (dict(optimizer=1, form=15, coef=None), "EINVAL", b"null coef"),
    (dict(x1=None), "EINVAL", b"entry 1: null x or y"),
    (dict(ld=7849), "EINVAL", b"ld = 7849 below P = 7850"),
    (dict(K=0), "EINVAL", b"K = 0 outside [1, 4096]"), (dict(K=4097), "EINVAL", b"K = 4097 outside"),
    (dict(D=1025), "EINVAL", b"D = 1025 outside [1, 1024]"), (dict(C=17), "EINVAL", b"C = 17 outside"),
    (dict(B1=0), "EINVAL", b"entry 1: B = 0 outside [1, 16384]"),
    (dict(row1=0), "EINVAL", b"entry 1: row 0 used twice"), (dict(row1=3), "EINVAL", b"entry 1: row 3 outside [0, 3)"),
    (dict(activation=2), "EMODE", b"activation 2"), (dict(optimizer=2), "EMODE", b"optimizer 2"),
    (dict(form=2), "EMODE", b"form 2"), (dict(optimizer=1, form=16), "EMODE", b"form 16"),
    (dict(rows=2), "EALIGN", b"4-B"), (dict(clients=1028), "EALIGN", b"8-B aligned"),
    (dict(x1=130), "EALIGN", b"entry 1: x must be 4-B"),
    (dict(), "EINVAL", b"clients is not pinned host memory"),  # well-formed: as far as the checks that need a GPU
])
def test_cohort_entry_refusals(lib, change, code, words):
    buf = np.zeros(256, np.float64)  # ordinary host memory: the table in it is well-formed and not pinned
    base = buf.ctypes.data
    a = dict(model=0, rows=64, ld=7872, clients=1024, K=3, D=784, C=10, iters=5, activation=0, optimizer=0, lr=0.05,
             lr_ratio=50.0, form=1, coef=256, rec=320, stream=None)
    entries = {f"{f}{g}": v for g in range(3) for f, v in (("x", 128), ("y", 192), ("B", 100 - g), ("row", g))}
    for k in list(change):
        if k in entries:
            entries[k] = change.pop(k)
    a.update(change)
    table = buf[128:140].view(np.int64).reshape(3, 4)
    for g in range(3):
        x, y = entries[f"x{g}"], entries[f"y{g}"]
        table[g] = (0 if x is None else base + x, 0 if y is None else base + y, entries[f"B{g}"], entries[f"row{g}"])
    for k in ("model", "rows", "clients", "coef", "rec"):  # offsets into the buffer become addresses
        a[k] = None if a[k] is None else base + a[k]
    assert getattr(lib, ENTRY)(*a.values()) == getattr(_lib, "FEDAVG_" + code)
    msg = lib.fedavg_clientcohort_last_error()
    assert msg.startswith(ENTRY.encode()) and words in msg, msg
    with pytest.raises(_lib.FedAvgLibraryError, match=ENTRY):
        _lib.check_clientcohort(-1, ENTRY)
