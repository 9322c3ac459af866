"""libfedavg_amd_clientchain.so (include/fedavg_amd_clientchain.h), the thirteenth native library, held as
test_clienteval_abi.py holds the twelfth, except that its tuple is not pinned to one key: the next library joins it.
CPU only: nulls, sizes, codes, alignments and the client table's contents are validated before any HIP call.  The
refusal of 1 - beta1 needs to know that coef is pinned and not device memory, which is a HIP call: it is held in
test_gpu_client_chain.py."""
import dataclasses
import importlib.util
from pathlib import Path

import numpy as np
import pytest

from mfl_amd import _lib, build, client_passes
from test_abi import _exported, declared_functions

HERE = Path(__file__).parent
HEADER = "fedavg_amd_clientchain.h"
ENTRY = "fedavg_client_chain_f32"
DECLARED = ("fedavg_clientchain_abi_version", "fedavg_clientchain_last_error", "fedavg_client_chain_limits", ENTRY)


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load_clientchain()


def test_the_twelve_stay_and_the_thirteenth_is_described_built_and_loaded(lib, monkeypatch):
    assert len(build.BUILT_LIBS) == 8 and set(build.EVAL_BY_KEY) == {"clienteval"} == set(_lib._EVAL_BINDING)
    assert set(build.CHAIN_BY_KEY) == {d.key for d in build.CHAIN_LIBS} == set(_lib._CHAIN_BINDING)
    d = build.CHAIN_BY_KEY["clientchain"]
    assert d in build.CHAIN_LIBS and d.path == build.CLIENTCHAIN_LIB_PATH and d.header == HEADER
    assert d.units == ("fedavg_client_chain.hip",) and d.needs == "" and d.link == ()
    assert set(d.sources) <= set(build.sources()) and all(src.exists() for src in d.sources)
    assert build.later_up_to_date()
    monkeypatch.setattr(build, "CHAIN_LIBS", (dataclasses.replace(d, file="libfedavg_amd_no_such.so"),))
    assert not build.later_up_to_date()


def test_exports_are_exactly_the_header_and_the_kernels_the_listed_ones(lib):
    declared = declared_functions((HEADER,))
    assert declared == sorted(DECLARED) == _exported(build.CLIENTCHAIN_LIB_PATH) == sorted(_lib.CLIENTCHAIN_SIGNATURES)
    assert lib.fedavg_clientchain_abi_version() == _lib.CLIENTCHAIN_ABI_VERSION == 1
    assert client_passes.chain_limits() == client_passes.cohort_limits() == (4096, 16384, 1024, 16)
    data = build.CLIENTCHAIN_LIB_PATH.read_bytes()
    assert b"gfx950" in data and b"getenv" not in data
    spec = importlib.util.spec_from_file_location("kernel_inventory", HERE.parent / "scripts" / "kernel_inventory.py")
    inv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(inv)
    if inv.have_tools():
        listed = (HERE / "clientchain_kernels.txt").read_text().splitlines()
        assert sorted(inv.inventory(build.CLIENTCHAIN_LIB_PATH)) == listed and len(listed) == 4  # Adam x direct loads


def test_load_refuses_another_abi_version(lib, monkeypatch):
    d = build.CHAIN_BY_KEY["clientchain"]
    monkeypatch.setitem(build.CHAIN_BY_KEY, "clientchain", dataclasses.replace(d, abi=(d.abi[0], 2)))
    monkeypatch.setattr(_lib, "_clientchain", None)
    with pytest.raises(_lib.FedAvgLibraryError, match="ABI version 1 != expected 2; rebuild the library"):
        _lib.load_clientchain()
    assert _lib._clientchain is None


ADAM = dict(optimizer=1, form=15)


@pytest.mark.parametrize("change, code, words", [
    (dict(model=None), "EINVAL", b"null"), (dict(clients=None), "EINVAL", b"null"), (dict(losses=None), "EINVAL", b"null"),
    (dict(rec=None), "EINVAL", b"null"), (dict(ADAM, state=None), "EINVAL", b"null state"),
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
    (dict(x1=130), "EALIGN", b"entry 1: x must be 4-B"), (dict(y2=196), "EALIGN", b"entry 2: x must be 4-B, y 8-B"),
    (dict(), "EINVAL", b"clients is not pinned host memory"),  # well-formed: as far as the checks that need a GPU
    (dict(ADAM), "EINVAL", b"clients is not pinned host memory"),
])
def test_chain_entry_refusals(lib, change, code, words):
    buf = np.zeros(256, np.float64)  # ordinary host memory: the table in it is well-formed and not pinned
    base = buf.ctypes.data
    a = dict(model=0, state=64, clients=1024, K=3, D=784, C=10, rounds=2, step0=0, activation=0, optimizer=0, lr=0.05,
             form=1, coef=256, losses=384, rec=320, stream=None)
    entries = {f"{f}{g}": v for g in range(3) for f, v in (("x", 128), ("y", 192), ("B", 100 - g), ("unused", 0))}
    for k in list(change):
        if k in entries:
            entries[k] = change.pop(k)
    a.update(change)
    table = buf[128:140].view(np.int64).reshape(3, 4)
    for g in range(3):
        x, y = entries[f"x{g}"], entries[f"y{g}"]
        table[g] = (0 if x is None else base + x, 0 if y is None else base + y, entries[f"B{g}"], 0)
    for k in ("model", "state", "clients", "coef", "losses", "rec"):  # offsets into the buffer become addresses
        a[k] = None if a[k] is None else base + a[k]
    assert getattr(lib, ENTRY)(*a.values()) == getattr(_lib, "FEDAVG_" + code)
    msg = lib.fedavg_clientchain_last_error()
    assert msg.startswith(ENTRY.encode()) and words in msg, msg
    with pytest.raises(_lib.FedAvgLibraryError, match=ENTRY):
        _lib.check_clientchain(-1, ENTRY)
