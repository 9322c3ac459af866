"""libfedavg_amd_clientsplit.so (include/fedavg_amd_clientsplit.h), the fourteenth native library, in the thirteenth's
tuple and held as test_clientchain_abi.py holds that one.  CPU only: everything here is validated before any HIP call."""
import dataclasses
import importlib.util
from pathlib import Path

import numpy as np
import pytest

from mfl_amd import _lib, build, client_passes
from test_abi import _exported, declared_functions

HERE = Path(__file__).parent
HEADER = "fedavg_amd_clientsplit.h"
ENTRY = "fedavg_client_chain_split_f32"
DECLARED = ("fedavg_clientsplit_abi_version", "fedavg_clientsplit_last_error", "fedavg_client_split_slice_rows",
            "fedavg_client_split_workspace_bytes", ENTRY)


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load_clientsplit()


def test_the_fourteenth_is_described_built_and_loaded(lib):
    assert set(build.CHAIN_BY_KEY) == {"clientchain", "clientsplit"} == set(_lib._CHAIN_BINDING)
    d = build.CHAIN_BY_KEY["clientsplit"]
    assert d in build.CHAIN_LIBS and d.path == build.CLIENTSPLIT_LIB_PATH and d.header == HEADER
    assert d.units == ("fedavg_client_split.hip",) and d.needs == "" and d.link == ()
    assert set(d.sources) <= set(build.sources()) and all(src.exists() for src in d.sources)
    assert build.later_up_to_date()


def test_exports_are_exactly_the_header_and_the_kernels_the_listed_ones(lib):
    declared = declared_functions((HEADER,))
    assert declared == sorted(DECLARED) == _exported(build.CLIENTSPLIT_LIB_PATH) == sorted(_lib.CLIENTSPLIT_SIGNATURES)
    assert lib.fedavg_clientsplit_abi_version() == _lib.CLIENTSPLIT_ABI_VERSION == 1
    assert client_passes.split_limits() == client_passes.chain_limits()
    data = build.CLIENTSPLIT_LIB_PATH.read_bytes()
    assert b"gfx950" in data and b"getenv" not in data
    spec = importlib.util.spec_from_file_location("kernel_inventory", HERE.parent / "scripts" / "kernel_inventory.py")
    inv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(inv)
    if inv.have_tools():
        listed = (HERE / "clientsplit_kernels.txt").read_text().splitlines()
        found = inv.inventory(build.CLIENTSPLIT_LIB_PATH)
        assert sorted(found) == listed and len(listed) == 5  # labels, gradient x direct loads, step x Adam
        assert all(row["scratch"] == 0 for row in found.values())


def test_load_refuses_another_abi_version(lib, monkeypatch):
    d = build.CHAIN_BY_KEY["clientsplit"]
    monkeypatch.setitem(build.CHAIN_BY_KEY, "clientsplit", dataclasses.replace(d, abi=(d.abi[0], 2)))
    monkeypatch.setattr(_lib, "_clientsplit", None)
    with pytest.raises(_lib.FedAvgLibraryError, match="ABI version 1 != expected 2; rebuild the library"):
        _lib.load_clientsplit()
    assert _lib._clientsplit is None


# R: the most multiples of 16 rows of 4 ceil(D / 4) + 4 floats in the stream library's LDS budget, at most 256
@pytest.mark.parametrize("D, rows", [(1, 256), (252, 128), (253, 112), (512, 64), (513, 48), (1024, 32), (0, 0), (1025, 0)])
def test_slice_rows_and_workspace_bytes(lib, D, rows):
    assert lib.fedavg_client_split_slice_rows(D) == client_passes.split_slice_rows(D) == rows
    for max_b, C in ((1, 2), (rows, 16), (rows + 1, 10), (16384, 16)):
        want = 256 + -(-max_b // rows) * (8 + 4 * (C * D + C)) if rows and max_b else 0
        assert lib.fedavg_client_split_workspace_bytes(max_b, D, C) == want


ADAM = dict(optimizer=1, form=15)


@pytest.mark.parametrize("change, code, words", [
    (dict(model=None), "EINVAL", b"null"), (dict(clients=None), "EINVAL", b"null"), (dict(losses=None), "EINVAL", b"null"),
    (dict(rec=None), "EINVAL", b"null"), (dict(workspace=None), "EINVAL", b"null"), (dict(ADAM, state=None), "EINVAL", b"null state"),
    (dict(ADAM, coef=None), "EINVAL", b"null coef"), (dict(x1=None), "EINVAL", b"entry 1: null x or y"),
    (dict(K=0), "EINVAL", b"K = 0 outside [1, 4096]"), (dict(K=4097), "EINVAL", b"K = 4097 outside"),
    (dict(D=0), "EINVAL", b"D = 0 outside [1, 1024]"), (dict(D=1025), "EINVAL", b"D = 1025 outside [1, 1024]"),
    (dict(C=1), "EINVAL", b"C = 1 outside [2, 16]"), (dict(C=17), "EINVAL", b"C = 17 outside"),
    (dict(B1=0), "EINVAL", b"entry 1: B = 0 outside [1, 16384]"), (dict(B2=16385), "EINVAL", b"entry 2: B = 16385"),
    (dict(rounds=0), "EINVAL", b"rounds = 0 outside [1, 715827882]"), (dict(rounds=715827883), "EINVAL", b"rounds = "),
    (dict(step0=-1), "EINVAL", b"step0 = -1 is negative"),
    (dict(activation=2), "EMODE", b"activation 2"), (dict(optimizer=2), "EMODE", b"optimizer 2"),
    (dict(form=2), "EMODE", b"form 2"), (dict(optimizer=1, form=16), "EMODE", b"form 16"),
    (dict(model=2), "EALIGN", b"4-B"), (dict(ADAM, state=66), "EALIGN", b"4-B"), (dict(clients=1028), "EALIGN", b"8-B"),
    (dict(losses=388), "EALIGN", b"8-B"), (dict(rec=324), "EALIGN", b"8-B"), (dict(ADAM, coef=260), "EALIGN", b"8-B"),
    (dict(workspace=452), "EALIGN", b"workspace 8-B"),
    (dict(x1=130), "EALIGN", b"entry 1: x must be 4-B"), (dict(y2=196), "EALIGN", b"entry 2: x must be 4-B, y 8-B"),
    (dict(workspace_bytes=-1), "EINVAL", b"bytes below the"),  # one byte short of the largest batch's three slices
    (dict(B2=97, workspace_bytes=0), "EINVAL", b"bytes below the"),  # entry 2 alone has a fourth slice
    (dict(), "EINVAL", b"clients is not pinned host memory"),  # well-formed: as far as the checks that need a GPU
    (dict(ADAM), "EINVAL", b"clients is not pinned host memory"),
])
def test_split_entry_refusals(lib, change, code, words):
    buf = np.zeros(256, np.float64)  # ordinary host memory: the table in it is well-formed and not pinned
    base = buf.ctypes.data
    a = dict(model=0, state=64, clients=1024, K=3, D=784, C=10, rounds=2, step0=0, activation=0, optimizer=0, lr=0.05,
             form=1, coef=256, losses=384, rec=320, workspace=448, workspace_bytes=0, stream=None)
    entries = {f"{f}{g}": v for g in range(3) for f, v in (("x", 128), ("y", 192), ("B", 96 - g), ("unused", 0))}
    for k in list(change):
        if k in entries:
            entries[k] = change.pop(k)
    a.update(change)
    a["workspace_bytes"] += lib.fedavg_client_split_workspace_bytes(96, 784, 10)  # B = 96: three slices of 32 rows
    table = buf[128:140].view(np.int64).reshape(3, 4)
    for g in range(3):
        x, y = entries[f"x{g}"], entries[f"y{g}"]
        table[g] = (0 if x is None else base + x, 0 if y is None else base + y, entries[f"B{g}"], 0)
    for k in ("model", "state", "clients", "coef", "losses", "rec", "workspace"):  # offsets become addresses
        a[k] = None if a[k] is None else base + a[k]
    assert getattr(lib, ENTRY)(*a.values()) == getattr(_lib, "FEDAVG_" + code)
    msg = lib.fedavg_clientsplit_last_error()
    assert msg.startswith(ENTRY.encode()) and words in msg, msg
    with pytest.raises(_lib.FedAvgLibraryError, match=ENTRY):
        _lib.check_clientsplit(-1, ENTRY)
