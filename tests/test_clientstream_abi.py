"""libfedavg_amd_clientstream.so (include/fedavg_amd_clientstream.h), the tenth native library, held as
test_clientlinear_abi.py holds the ninth.  CPU only: nulls, sizes, codes and alignments are validated before any HIP call."""
import dataclasses
import importlib.util
from pathlib import Path

import numpy as np
import pytest

from mfl_amd import _lib, build, client_passes
from test_abi import _exported, declared_functions

HERE = Path(__file__).parent
HEADER = "fedavg_amd_clientstream.h"
ENTRY = "fedavg_client_linear_stream_f32"
DECLARED = ("fedavg_clientstream_abi_version", "fedavg_clientstream_last_error", "fedavg_client_stream_limits",
            "fedavg_client_stream_group_rows", ENTRY)
EARLIER = {"SIGNATURES": 49, "TUNING_SIGNATURES": 22, "FUSEDVEC_SIGNATURES": 7, "SEGVEC_SIGNATURES": 8,
           "CLIENTVEC_SIGNATURES": 11, "CLIENTSTEP_SIGNATURES": 9, "CLIENTADAM_SIGNATURES": 9, "CLIENTLOOP_SIGNATURES": 14,
           "CLIENTLINEAR_SIGNATURES": 4}


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load_clientstream()


def test_the_nine_stay_and_the_tenth_has_a_table_of_its_own(lib, monkeypatch):
    assert len(build.BUILT_LIBS) == 8 and set(build.LINEAR_BY_KEY) == {"clientlinear"} == set(_lib._LINEAR_BINDING)
    assert set(build.STREAM_BY_KEY) == {"clientstream"} == set(_lib._STREAM_BINDING)
    assert {name: len(getattr(_lib, name)) for name in EARLIER} == EARLIER  # the earlier libraries' tables
    d = build.STREAM_BY_KEY["clientstream"]
    assert d is build.STREAM_LIBS[0] and d.path == build.CLIENTSTREAM_LIB_PATH and d.header == HEADER
    assert d.units == ("fedavg_client_stream.hip",) and d.needs == "" and d.link == ()
    assert set(d.sources) <= set(build.sources()) and all(src.exists() for src in d.sources)
    text = d.sources[0].read_text()  # the step and guard arithmetic stays in the shared headers
    assert '"client_step_rules.hpp"' in text and '"client_adam_rules.hpp"' in text and '"client_linear_core.hpp"' in text
    assert "struct CsF32" not in text and "struct CaF32" not in text and "struct LinBatch" not in text
    assert build.later_up_to_date()
    monkeypatch.setattr(build, "STREAM_LIBS", (dataclasses.replace(d, file="libfedavg_amd_no_such.so"),))
    assert not build.later_up_to_date()


def test_exports_are_exactly_the_header_and_the_kernels_the_listed_ones(lib):
    declared = declared_functions((HEADER,))
    assert declared == sorted(DECLARED) == _exported(build.CLIENTSTREAM_LIB_PATH) == sorted(_lib.CLIENTSTREAM_SIGNATURES)
    assert lib.fedavg_clientstream_abi_version() == _lib.CLIENTSTREAM_ABI_VERSION == 1
    max_b, max_d, max_c, lds = client_passes.linear_stream_limits()
    assert (max_b, max_d, max_c) == (16384, 1024, 16) and max_b * max_d <= 2 ** 24
    assert lds == client_passes.linear_limits()[3] and 2 * 16 * (1024 + 4) * 4 == 131584 <= lds
    data = build.CLIENTSTREAM_LIB_PATH.read_bytes()
    assert b"gfx950" in data and b"getenv" not in data
    spec = importlib.util.spec_from_file_location("kernel_inventory", HERE.parent / "scripts" / "kernel_inventory.py")
    inv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(inv)
    if inv.have_tools():
        listed = (HERE / "clientstream_kernels.txt").read_text().splitlines()
        assert sorted(inv.inventory(build.CLIENTSTREAM_LIB_PATH)) == listed and len(listed) == 4  # Adam x direct loads


@pytest.mark.parametrize("D, rows", [(1, 64), (252, 64), (253, 32), (512, 32), (513, 16), (1024, 16), (0, 0), (1025, 0)])
def test_group_rows_is_the_largest_of_64_32_16_whose_two_buffers_fit(lib, D, rows):
    assert lib.fedavg_client_stream_group_rows(D) == rows
    lds = client_passes.linear_stream_limits()[3]
    if rows:
        S = 4 * ((D + 3) // 4) + 4
        assert 2 * rows * S * 4 <= lds and (rows == 64 or 2 * (2 * rows) * S * 4 > lds)


def test_load_refuses_another_abi_version(lib, monkeypatch):
    d = build.STREAM_BY_KEY["clientstream"]
    monkeypatch.setitem(build.STREAM_BY_KEY, "clientstream", dataclasses.replace(d, abi=(d.abi[0], 2)))
    monkeypatch.setattr(_lib, "_clientstream", None)
    with pytest.raises(_lib.FedAvgLibraryError, match="ABI version 1 != expected 2; rebuild the library"):
        _lib.load_clientstream()
    assert _lib._clientstream is None


@pytest.mark.parametrize("change, code, words", [
    (dict(w=None), "EINVAL", b"null"), (dict(x=None), "EINVAL", b"null"), (dict(rec=None), "EINVAL", b"null"),
    (dict(optimizer=1, form=15, coef=None), "EINVAL", b"null coef"),
    (dict(B=0), "EINVAL", b"B = 0 outside [1, 16384]"), (dict(B=16385), "EINVAL", b"B = 16385 outside"),
    (dict(D=1025), "EINVAL", b"D = 1025 outside [1, 1024]"), (dict(C=1), "EINVAL", b"C = 1 outside [2, 16]"),
    (dict(C=17), "EINVAL", b"C = 17 outside"), (dict(iters=-1), "EINVAL", b"negative iteration count"),
    (dict(activation=2), "EMODE", b"activation 2"), (dict(optimizer=2), "EMODE", b"optimizer 2"),
    (dict(form=2), "EMODE", b"form 2"), (dict(optimizer=1, form=16), "EMODE", b"form 16"),
    (dict(rec=324), "EALIGN", b"8-B aligned"), (dict(y=196), "EALIGN", b"8-B aligned"), (dict(w=2), "EALIGN", b"4-B"),
    (dict(), "EINVAL", b"must be device memory"),  # well-formed: as far as the pointer checks, which need a GPU
])
def test_stream_entry_refusals(lib, change, code, words):
    buf = np.zeros(64, np.float64)
    a = dict(w=0, b=64, x=128, y=192, B=1000, D=784, C=10, iters=5, activation=0, optimizer=0, lr=0.05, lr_ratio=50.0,
             form=1, coef=256, rec=320, stream=None)
    a.update(change)
    for k in ("w", "b", "x", "y", "coef", "rec"):  # offsets into the buffer become addresses
        a[k] = None if a[k] is None else buf.ctypes.data + a[k]
    assert getattr(lib, ENTRY)(*a.values()) == getattr(_lib, "FEDAVG_" + code)
    msg = lib.fedavg_clientstream_last_error()
    assert msg.startswith(ENTRY.encode()) and words in msg, msg
    with pytest.raises(_lib.FedAvgLibraryError, match=ENTRY):
        _lib.check_clientstream(-1, ENTRY)
