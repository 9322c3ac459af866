"""libfedavg_amd_clienteval.so (include/fedavg_amd_clienteval.h), the twelfth native library, held as
test_clientcohort_abi.py holds the eleventh.  CPU only: nulls, sizes, codes, alignments, the client table's contents and
the workspace size are validated before any HIP call."""
import dataclasses
import importlib.util
from pathlib import Path

import numpy as np
import pytest

from mfl_amd import _lib, build, client_passes
from test_abi import _exported, declared_functions

HERE = Path(__file__).parent
HEADER = "fedavg_amd_clienteval.h"
ENTRY = "fedavg_client_eval_f32"
DECLARED = ("fedavg_clienteval_abi_version", "fedavg_clienteval_last_error", "fedavg_client_eval_limits",
            "fedavg_client_eval_workspace_bytes", ENTRY)


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load_clienteval()


def test_the_eleven_stay_and_the_twelfth_has_a_table_of_its_own(lib, monkeypatch):
    assert len(build.BUILT_LIBS) == 8 and set(build.STREAM_BY_KEY) == {"clientstream"} == set(_lib._STREAM_BINDING)
    assert set(build.COHORT_BY_KEY) == {"clientcohort"} == set(_lib._COHORT_BINDING)
    assert set(build.EVAL_BY_KEY) == {"clienteval"} == set(_lib._EVAL_BINDING)
    d = build.EVAL_BY_KEY["clienteval"]
    assert d is build.EVAL_LIBS[0] and d.path == build.CLIENTEVAL_LIB_PATH and d.header == HEADER
    assert d.units == ("fedavg_client_eval.hip",) and d.needs == "" and d.link == ()
    assert set(d.sources) <= set(build.sources()) and all(src.exists() for src in d.sources)
    assert build.later_up_to_date()
    monkeypatch.setattr(build, "EVAL_LIBS", (dataclasses.replace(d, file="libfedavg_amd_no_such.so"),))
    assert not build.later_up_to_date()


def test_exports_are_exactly_the_header_and_the_kernels_the_listed_ones(lib):
    declared = declared_functions((HEADER,))
    assert declared == sorted(DECLARED) == _exported(build.CLIENTEVAL_LIB_PATH) == sorted(_lib.CLIENTEVAL_SIGNATURES)
    assert lib.fedavg_clienteval_abi_version() == _lib.CLIENTEVAL_ABI_VERSION == 1
    assert client_passes.eval_limits() == client_passes.cohort_limits() == (4096, 16384, 1024, 16)
    data = build.CLIENTEVAL_LIB_PATH.read_bytes()
    assert b"gfx950" in data and b"getenv" not in data
    spec = importlib.util.spec_from_file_location("kernel_inventory", HERE.parent / "scripts" / "kernel_inventory.py")
    inv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(inv)
    if inv.have_tools():
        listed = (HERE / "clienteval_kernels.txt").read_text().splitlines()
        assert sorted(inv.inventory(build.CLIENTEVAL_LIB_PATH)) == listed and len(listed) == 4  # setup, 2 loads, finish


def test_load_refuses_another_abi_version(lib, monkeypatch):
    d = build.EVAL_BY_KEY["clienteval"]
    monkeypatch.setitem(build.EVAL_BY_KEY, "clienteval", dataclasses.replace(d, abi=(d.abi[0], 2)))
    monkeypatch.setattr(_lib, "_clienteval", None)
    with pytest.raises(_lib.FedAvgLibraryError, match="ABI version 1 != expected 2; rebuild the library"):
        _lib.load_clienteval()
    assert _lib._clienteval is None


# the well-formed call needs 32 + 3 * 32 + 3 * 32 = 224 bytes of workspace (K = 3, one chunk each)
@pytest.mark.parametrize("change, code, words", [
    (dict(model=None), "EINVAL", b"null"), (dict(clients=None), "EINVAL", b"null"), (dict(rec=None), "EINVAL", b"null"),
    (dict(workspace=None), "EINVAL", b"null"), (dict(x1=None), "EINVAL", b"entry 1: null x or y"),
    (dict(K=0), "EINVAL", b"K = 0 outside [1, 4096]"), (dict(K=4097), "EINVAL", b"K = 4097 outside"),
    (dict(D=0), "EINVAL", b"D = 0 outside [1, 1024]"), (dict(D=1025), "EINVAL", b"D = 1025 outside [1, 1024]"),
    (dict(C=1), "EINVAL", b"C = 1 outside [2, 16]"), (dict(C=17), "EINVAL", b"C = 17 outside"),
    (dict(B1=0), "EINVAL", b"entry 1: B = 0 outside [1, 16384]"), (dict(B1=16385), "EINVAL", b"entry 1: B = 16385"),
    (dict(slot1=0), "EINVAL", b"entry 1: slot 0 used twice"), (dict(slot1=3), "EINVAL", b"entry 1: slot 3 outside [0, 3)"),
    (dict(slot2=-1), "EINVAL", b"entry 2: slot -1 outside"),
    (dict(workspace_bytes=223), "EINVAL", b"workspace of 223 bytes below the 224 needed"),
    (dict(B0=257, workspace_bytes=255), "EINVAL", b"workspace of 255 bytes below the 256 needed"),
    (dict(activation=2), "EMODE", b"activation 2"), (dict(activation=-1), "EMODE", b"activation -1"),
    (dict(model=2), "EALIGN", b"4-B"), (dict(clients=1028), "EALIGN", b"8-B"), (dict(rec=324), "EALIGN", b"8-B"),
    (dict(workspace=520), "EALIGN", b"workspace 16-B aligned"),
    (dict(x1=130), "EALIGN", b"entry 1: x must be 4-B"), (dict(y2=196), "EALIGN", b"entry 2: x must be 4-B, y 8-B"),
    (dict(), "EINVAL", b"clients is not pinned host memory"),  # well-formed: as far as the checks that need a GPU
])
def test_eval_entry_refusals(lib, change, code, words):
    buf = np.zeros(256, np.float64)  # ordinary host memory: the table in it is well-formed and not pinned
    base = buf.ctypes.data
    assert base % 16 == 0
    a = dict(model=0, clients=1024, K=3, D=784, C=10, activation=1, rec=320, workspace=512, workspace_bytes=224,
             stream=None)
    entries = {f"{f}{g}": v for g in range(3) for f, v in (("x", 128), ("y", 192), ("B", 100 - g), ("slot", g))}
    for k in list(change):
        if k in entries:
            entries[k] = change.pop(k)
    a.update(change)
    table = buf[128:140].view(np.int64).reshape(3, 4)
    for g in range(3):
        x, y = entries[f"x{g}"], entries[f"y{g}"]
        table[g] = (0 if x is None else base + x, 0 if y is None else base + y, entries[f"B{g}"], entries[f"slot{g}"])
    for k in ("model", "clients", "rec", "workspace"):  # offsets into the buffer become addresses
        a[k] = None if a[k] is None else base + a[k]
    assert getattr(lib, ENTRY)(*a.values()) == getattr(_lib, "FEDAVG_" + code)
    msg = lib.fedavg_clienteval_last_error()
    assert msg.startswith(ENTRY.encode()) and words in msg, msg
    with pytest.raises(_lib.FedAvgLibraryError, match=ENTRY):
        _lib.check_clienteval(-1, ENTRY)


@pytest.mark.parametrize("Bs, D, want", [
    ((1,), 5, 32 + 32 * 1 + 32 * 1),                        # 4 * 2 = 8 -> 32; one entry; one chunk
    ((256, 257, 513), 784, 32 + 32 * 3 + 32 * (1 + 2 + 3)),  # 4 * 4 = 16 -> 32; chunks at the edge, edge + 1, 2 edges + 1
    ((16384,) * 8 + (1,), 1024, 64 + 32 * 9 + 32 * (8 * 64 + 1)),  # 4 * 10 = 40 -> 64
])
def test_workspace_bytes_by_hand(lib, Bs, D, want):
    table = np.array([[16, 16, B, g] for g, B in enumerate(Bs)], np.int64)
    assert lib.fedavg_client_eval_workspace_bytes(table.ctypes.data, len(Bs), D) == want
    assert client_passes.EVAL_CHUNK_ROWS == 256
    table[-1, 2] = 16385
    assert lib.fedavg_client_eval_workspace_bytes(table.ctypes.data, len(Bs), D) == _lib.FEDAVG_EINVAL
    assert lib.fedavg_client_eval_workspace_bytes(None, len(Bs), D) == _lib.FEDAVG_EINVAL
