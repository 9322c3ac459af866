"""libfedavg_amd_clientloop.so (include/fedavg_amd_clientloop.h), the eighth
native library: what test_clientadam_abi.py asserts of the seventh (exports
equal the header and the signature table, a gfx950 code object that reads no
environment, no project library among NEEDED, the listed kernel set, no
scratch and no spills, the loader's four refusals word for word), then the
span / workspace / partials arithmetic and every refusal of the guard and of
the gated step entries.

CPU only: nulls, sizes, tables and alignments are validated before any HIP
call, and the span, workspace and partials functions are host arithmetic.
"""
import ctypes
import dataclasses
import importlib.util
import subprocess
from pathlib import Path

import numpy as np
import pytest

from mfl_amd import _lib, build
from test_abi import _exported, declared_functions

ROOT = Path(__file__).resolve().parents[1]
HERE = Path(__file__).parent
HEADER = "fedavg_amd_clientloop.h"
FILE = "libfedavg_amd_clientloop.so"
KEYS = ("f32", "bf16", "f64")
GUARD = tuple(f"fedavg_client_guard_{k}" for k in KEYS)
SGD = tuple(f"fedavg_client_sgd_step_gated_{k}" for k in KEYS)
ADAM = tuple(f"fedavg_client_adam_step_gated_{k}" for k in KEYS)
DECLARED = ("fedavg_clientloop_abi_version", "fedavg_clientloop_last_error", "fedavg_client_loop_span",
            "fedavg_client_loop_workspace", "fedavg_client_loop_partials", *GUARD, *SGD, *ADAM)
OTHER_HEADERS = ("fedavg_amd.h", "fedavg_amd_tuning.h", "fedavg_amd_fusedvec.h", "fedavg_amd_segvec.h",
                 "fedavg_amd_clientvec.h", "fedavg_amd_clientstep.h", "fedavg_amd_clientadam.h")
OTHER_TABLES = ("SIGNATURES", "TUNING_SIGNATURES", "FUSEDVEC_SIGNATURES", "SEGVEC_SIGNATURES", "CLIENTVEC_SIGNATURES",
                "CLIENTSTEP_SIGNATURES", "CLIENTADAM_SIGNATURES")
OTHER_KERNELS = ("product_kernels.txt", "fusedvec_kernels.txt", "segvec_kernels.txt", "clientvec_kernels.txt",
                 "clientstep_kernels.txt", "clientadam_kernels.txt")
ES = {"f32": 4, "bf16": 2, "f64": 8}
NOT_BUILT = ("{path} not built: run __graft_entry__.build(); there is no fallback for the device-side client guard "
             "and the gated steps")


def es_of(entry):
    return ES[entry.rsplit("_", 1)[1]]


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load_clientloop()


def last(lib):
    return lib.fedavg_clientloop_last_error()


# ------------------------------------------------------------------ structure
def test_the_seven_stay_and_the_eighth_has_a_table_of_its_own():
    assert len(build.ALL_LIBS) == 6 and len(build.EVERY_LIB) == 7
    assert build.EVERY_LIB == build.ALL_LIBS + build.NEWER_LIBS
    assert tuple(lib.key for lib in build.NEWER_LIBS) == ("clientadam",)
    assert set(build.DESCRIBED) == set(build.BY_KEY) | {"clientadam"} == set(_lib._BINDING)
    assert set(build.EXTRA_BY_KEY) == {"clientloop"} == set(_lib._EXTRA_BINDING)
    assert tuple(lib.key for lib in build.EXTRA_LIBS) == ("clientloop",)
    assert build.BUILT_LIBS == build.EVERY_LIB + build.EXTRA_LIBS and len(build.BUILT_LIBS) == 8
    d = build.EXTRA_BY_KEY["clientloop"]
    assert d is build.EXTRA_LIBS[0] and isinstance(d, build.NativeLib)
    assert d.path == build.CLIENTLOOP_LIB_PATH == build.LIB_DIR / FILE and d.header == HEADER
    assert d.abi == ("fedavg_clientloop_abi_version", 1) and d.needs == "" and d.link == ()
    assert d.units == ("fedavg_client_loop.hip",)
    assert (ROOT / "include" / HEADER).exists() and all(src.exists() for src in d.sources)
    assert set(d.sources) <= set(build.sources())
    for shared in ("client_step_rules.hpp", "client_adam_rules.hpp"):  # the step arithmetic, once
        assert build.CSRC_DIR / shared in build.sources()


def test_the_step_arithmetic_exists_once():
    """The per-dtype rules live in the two headers and in no translation unit."""
    csrc = build.CSRC_DIR
    for rule in ("struct CsF32", "struct CsHalf", "struct CsF64", "step_unit("):
        assert rule in (csrc / "client_step_rules.hpp").read_text()
    for rule in ("struct CaF32", "struct CaHalf", "struct CaF64", "adam_elem(", "adam_unit("):
        assert rule in (csrc / "client_adam_rules.hpp").read_text()
    for unit in ("fedavg_client_step.hip", "fedavg_client_adam.hip", "fedavg_client_loop.hip"):
        text = (csrc / unit).read_text()
        assert '_rules.hpp"' in text, unit
        for rule in ("struct CsF32", "struct CaF32", "struct CsHalf", "struct CaHalf"):
            assert rule not in text, (unit, rule)


def test_later_up_to_date_covers_the_new_library(lib, monkeypatch, tmp_path):
    assert build.later_up_to_date()
    d = build.EXTRA_BY_KEY["clientloop"]
    gone = dataclasses.replace(d, file="libfedavg_amd_no_such.so")
    monkeypatch.setattr(build, "EXTRA_LIBS", (gone,))
    assert not build.later_up_to_date()


def test_exports_are_exactly_the_header(lib):
    declared = declared_functions((HEADER,))
    assert declared == sorted(DECLARED)
    assert _exported(build.CLIENTLOOP_LIB_PATH) == declared
    assert sorted(_lib.CLIENTLOOP_SIGNATURES) == declared
    assert not any(name.endswith("_f16") for name in declared)  # no fp16 entry: no fused step is offered for it
    for other in OTHER_HEADERS:
        assert not set(declared) & set(declared_functions((other,))), other
    for other in OTHER_TABLES:
        assert not set(_lib.CLIENTLOOP_SIGNATURES) & set(getattr(_lib, other)), other
    raw = ctypes.CDLL(str(build.CLIENTLOOP_LIB_PATH))
    assert all(hasattr(raw, name) for name in declared)
    assert lib.fedavg_clientloop_abi_version() == _lib.CLIENTLOOP_ABI_VERSION == 1


def test_gfx950_code_object_and_no_environment_variable(lib):
    data = build.CLIENTLOOP_LIB_PATH.read_bytes()
    assert b"gfx950" in data
    assert b"getenv" not in data


def test_needs_no_project_library(lib):
    out = subprocess.run(["readelf", "-d", str(build.CLIENTLOOP_LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    assert "libfedavg_amd" not in "".join(ln for ln in out.splitlines() if "NEEDED" in ln)


@pytest.fixture(scope="module")
def inventory(lib):
    spec = importlib.util.spec_from_file_location("kernel_inventory", ROOT / "scripts" / "kernel_inventory.py")
    inv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(inv)
    if not inv.have_tools():
        pytest.skip("llvm-objcopy / llvm-readelf not found")
    return inv.inventory(build.CLIENTLOOP_LIB_PATH)


def test_kernel_set_is_the_listed_one_and_disjoint(inventory):
    listed = (HERE / "clientloop_kernels.txt").read_text().splitlines()
    built_set = sorted(inventory)
    assert sorted(set(built_set) - set(listed)) == [], "kernels built but not listed"
    assert sorted(set(listed) - set(built_set)) == [], "kernels listed but not built"
    # 3 dtypes x (guard, finalize, SGD form 0 / 1, Adam first / later)
    assert built_set == listed and len(built_set) == 18
    assert not any("::F16Pk" in name for name in listed)  # no fp16 instance
    for other in OTHER_KERNELS:
        assert not set(listed) & set((HERE / other).read_text().splitlines()), other


def test_no_instance_uses_scratch(inventory):
    for name, row in inventory.items():
        assert row["scratch"] == 0 and row["vgpr_spill"] == 0 and row["sgpr_spill"] == 0, (name, row)


# ---------------------------------------------------------------- the loader's refusals, word for word
def refusal():
    with pytest.raises(_lib.FedAvgLibraryError) as info:
        _lib.load_clientloop()
    assert _lib._clientloop is None  # a refused load leaves nothing cached
    return str(info.value)


def test_load_refuses_a_missing_file(lib, monkeypatch, tmp_path):
    path = tmp_path / FILE
    monkeypatch.setattr(_lib, "CLIENTLOOP_LIB_PATH", path)
    monkeypatch.setattr(_lib, "_clientloop", None)
    assert refusal() == NOT_BUILT.format(path=path)


def test_load_refuses_a_file_that_does_not_load(lib, monkeypatch, tmp_path):
    path = tmp_path / FILE
    path.touch()
    monkeypatch.setattr(_lib, "CLIENTLOOP_LIB_PATH", path)
    monkeypatch.setattr(_lib, "_clientloop", None)
    text = refusal()
    head = f"{path} does not load: "
    assert text.startswith(head) and str(path) in text[len(head):]  # the dynamic loader's own words follow


def test_load_refuses_a_library_without_a_typed_name(lib, monkeypatch):
    monkeypatch.setitem(_lib.CLIENTLOOP_SIGNATURES, "fedavg_no_such_entry", (ctypes.c_int, []))
    monkeypatch.setattr(_lib, "_clientloop", None)
    assert refusal() == f"{build.CLIENTLOOP_LIB_PATH} does not export fedavg_no_such_entry"


def test_load_refuses_another_abi_version(lib, monkeypatch):
    d = build.EXTRA_BY_KEY["clientloop"]
    monkeypatch.setitem(build.EXTRA_BY_KEY, "clientloop", dataclasses.replace(d, abi=(d.abi[0], 2)))
    monkeypatch.setattr(_lib, "_clientloop", None)
    assert refusal() == "ABI version 1 != expected 2; rebuild the library"


# ------------------------------------------------------------------ arithmetic
def test_span_workspace_and_partials_are_the_steps(lib):
    step, adam = _lib.load_clientstep(), _lib.load_clientadam()
    span, ws, parts = lib.fedavg_client_loop_span, lib.fedavg_client_loop_workspace, lib.fedavg_client_loop_partials
    assert span(4) == 4096 and span(2) == 8192 and span(8) == 2048  # 16 KiB of the tensor
    for es in (0, 1, 2, 3, 4, 8, 16, -2):
        assert span(es) == step.fedavg_client_step_span(es)
    for n in (-1, 0, 1, 3, 5):
        assert ws(n, 0) == step.fedavg_client_step_workspace(n) == max(n, 0) * 32
        assert ws(n, 1) == adam.fedavg_client_adam_workspace(n) == max(n, 0) * 40
    for es in (2, 4, 8, 3):
        for numels in ([1], [4096], [4097, 0, 63], [0, 0, 0]):
            numel = np.array(numels, np.int64)
            assert parts(numel.ctypes.data, len(numel), es) == \
                step.fedavg_client_step_partials(numel.ctypes.data, len(numel), es), (es, numels)
        assert parts(None, 3, es) == 0 and parts(numel.ctypes.data, 0, es) == 0
    numel = np.array([4097, 0, 63], np.int64)
    assert [parts(numel.ctypes.data, 3, es) for es in (4, 2, 8)] == [9, 6, 12]


# ------------------------------------------------------------------ the guard's refusals
@pytest.mark.parametrize("entry", GUARD)
def test_guard_rejects_bad_arguments_without_gpu(lib, entry):
    fn = getattr(lib, entry)
    buf = np.zeros(16, np.float64)  # a host address where only non-null and alignment matter
    p = buf.ctypes.data
    good = [p + 32, p, p + 96, p + 112, 0.05, 3, None]
    for idx in range(4):
        args = list(good)
        args[idx] = None
        assert fn(*args) == _lib.FEDAVG_EINVAL, idx
        assert last(lib).startswith(entry.encode()) and b"null" in last(lib)
        args = list(good)
        args[idx] += 4
        assert fn(*args) == _lib.FEDAVG_EALIGN, idx
        assert last(lib).startswith(entry.encode()) and b"8-B aligned" in last(lib)
    args = list(good)
    args[5] = -1
    assert fn(*args) == _lib.FEDAVG_EINVAL and b"negative epoch" in last(lib)
    # well-formed: the call gets as far as the pointer-attribute check, which nothing passes without a GPU
    assert fn(*good) == _lib.FEDAVG_EINVAL and b"records must be device memory" in last(lib)


# ------------------------------------------------------------------ the gated steps' refusals
def _extras(buf):
    p = buf.ctypes.data
    return [p + 32, p + 112, p + 64, p + 96]  # g_stats, gate, state, loss


def _sgd_args(n_keys=2, ws=64, parts=6, form=1, w=(4096, 8192), g=(12288, 16384), numel=(5, 7)):
    keep = [np.array(w, np.int64), np.array(g, np.int64), np.array(numel, np.int64), np.zeros(64, np.float64)]
    buf = keep[3]
    args = [keep[0].ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data, n_keys, 0.03, form, buf.ctypes.data, parts,
            buf.ctypes.data, 4096, 8192, ws, None, *_extras(buf)]
    return args, keep


COEFS = (0.001, 0.1, 0.999, 0.001, 0.0316, 1e-8, -0.01)


def _adam_args(n_keys=2, ws=80, parts=6, form=15, w=(4096, 8192), g=(12288, 16384), numel=(5, 7), offset=(0, 16),
               state_elems=64, coef=COEFS):
    keep = [np.array(w, np.int64), np.array(g, np.int64), np.array(numel, np.int64), np.array(offset, np.int64),
            np.array(coef, np.float64), np.zeros(64, np.float64)]
    buf = keep[5]
    args = [keep[0].ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data, keep[3].ctypes.data, n_keys, 20480,
            state_elems, keep[4].ctypes.data, 0, form, buf.ctypes.data, parts, buf.ctypes.data, 4096, 8192, ws, None,
            *_extras(buf)]
    return args, keep


def _with(i, value):
    c = list(COEFS)
    c[i] = value
    return tuple(c)


def _refused(lib, fn, entry, make, cases):
    for change, code, words in cases:
        args, keep = make(**change)
        rc = fn(*args)
        assert rc == getattr(_lib, "FEDAVG_" + code), (change, rc, last(lib))
        assert last(lib).startswith(entry.encode()) and words in last(lib), (change, last(lib))


def _gate_refusals(lib, fn, entry, make, first_extra):
    """A null or misaligned g_stats, gate, state or loss, refused before anything else is looked at."""
    for idx in range(first_extra, first_extra + 4):
        for spoil in (dict(), dict(n_keys=-1), dict(form=99)):  # also when another argument is bad
            args, keep = make(**spoil)
            args[idx] = None
            assert fn(*args) == _lib.FEDAVG_EINVAL, idx
            assert last(lib).startswith(entry.encode()) and b"null g_stats, gate, state or loss" in last(lib)
        args, keep = make()
        args[idx] += 4
        assert fn(*args) == _lib.FEDAVG_EALIGN, idx
        assert last(lib).startswith(entry.encode()) and b"8-B aligned" in last(lib)


@pytest.mark.parametrize("entry", SGD)
def test_gated_sgd_step_rejects_bad_arguments_without_gpu(lib, entry):
    es = es_of(entry)
    fn = getattr(lib, entry)
    _refused(lib, fn, entry, _sgd_args, [
        (dict(n_keys=-1), "EINVAL", b"negative"),
        (dict(numel=(5, -1)), "EINVAL", b"negative"),
        (dict(form=2), "EMODE", b"form 2"),
        (dict(form=-1), "EMODE", b"form -1"),
        (dict(w=(0, 8192)), "EINVAL", b"null tensor"),
        (dict(g=(12288, 0)), "EINVAL", b"null tensor"),
        (dict(w=(4096, 8192 + es // 2)), "EINVAL", b"multiple of %d bytes" % es),
        (dict(g=(12288 + es // 2, 16384)), "EINVAL", b"multiple of %d bytes" % es),
        (dict(ws=63), "EINVAL", b"workspace needs 64 bytes"),
        (dict(parts=5), "EINVAL", b"partials need 6 doubles"),
    ])
    for idx, off in ((9, 8), (10, 8), (6, 4), (8, 4)):  # host_ws, dev_ws, partials, stats
        args, keep = _sgd_args()
        args[idx] += off
        assert fn(*args) == _lib.FEDAVG_EALIGN, idx
    for idx in (0, 1, 2, 6, 8, 9, 10):  # tables and buffers
        args, keep = _sgd_args()
        args[idx] = None
        assert fn(*args) == _lib.FEDAVG_EINVAL and b"null" in last(lib), idx
    _gate_refusals(lib, fn, entry, _sgd_args, 13)
    # well-formed calls reach the pointer-attribute checks, which nothing passes without a GPU; with no keys or no
    # elements that check is the one of stats
    for change in (dict(w=(4096 + es, 8192)), dict(form=0), dict()):
        args, keep = _sgd_args(**change)
        assert fn(*args) == _lib.FEDAVG_EINVAL
        assert b"pinned" in last(lib) or b"device memory" in last(lib)
    for change in (dict(n_keys=0), dict(numel=(0, 0), parts=0)):
        args, keep = _sgd_args(**change)
        assert fn(*args) == _lib.FEDAVG_EINVAL and b"stats must be device memory" in last(lib)


@pytest.mark.parametrize("entry", ADAM)
def test_gated_adam_step_rejects_bad_arguments_without_gpu(lib, entry):
    es = es_of(entry)
    per = 16 // es
    fn = getattr(lib, entry)
    _refused(lib, fn, entry, _adam_args, [
        (dict(n_keys=-1), "EINVAL", b"negative"),
        (dict(state_elems=-16), "EINVAL", b"negative"),
        (dict(numel=(5, -1)), "EINVAL", b"negative"),
        (dict(form=16), "EMODE", b"form 16"),
        (dict(form=-1), "EMODE", b"form -1"),
        (dict(coef=_with(1, 0.5)), "EMODE", b"lerp"),
        (dict(coef=_with(1, float("nan"))), "EMODE", b"lerp"),
        (dict(w=(0, 8192)), "EINVAL", b"null tensor"),
        (dict(g=(12288, 0)), "EINVAL", b"null tensor"),
        (dict(w=(4096, 8192 + es // 2)), "EINVAL", b"multiple of %d bytes" % es),
        (dict(offset=(0, 64)), "EINVAL", b"key 1 lies outside a state plane of 64"),
        (dict(offset=(0, 16 + per // 2)), "EALIGN", b"key 1: state offset must be a multiple of %d" % per),
        (dict(state_elems=64 + per // 2), "EALIGN", b"state_elems a multiple of %d" % per),
        (dict(ws=79), "EINVAL", b"workspace needs 80 bytes"),
        (dict(parts=5), "EINVAL", b"partials need 6 doubles"),
    ])
    for idx, off in ((5, 8), (13, 8), (14, 8), (10, 4), (12, 4)):  # state, host_ws, dev_ws, partials, stats
        args, keep = _adam_args()
        args[idx] += off
        assert fn(*args) == _lib.FEDAVG_EALIGN, idx
    for idx in (0, 1, 2, 3, 5, 7, 10, 12, 13, 14):
        args, keep = _adam_args()
        args[idx] = None
        assert fn(*args) == _lib.FEDAVG_EINVAL and b"null" in last(lib), idx
    _gate_refusals(lib, fn, entry, _adam_args, 17)
    for change in (dict(form=0), dict()):
        args, keep = _adam_args(**change)
        assert fn(*args) == _lib.FEDAVG_EINVAL
        assert b"pinned" in last(lib) or b"device memory" in last(lib)
    for change in (dict(n_keys=0), dict(numel=(0, 0), parts=0)):
        args, keep = _adam_args(**change)
        assert fn(*args) == _lib.FEDAVG_EINVAL and b"stats must be device memory" in last(lib)


def test_check_clientloop_raises_with_the_librarys_message(lib):
    args, keep = _sgd_args(form=77)
    rc = lib.fedavg_client_sgd_step_gated_f32(*args)
    with pytest.raises(_lib.FedAvgLibraryError,
                       match=r"fedavg_client_sgd_step_gated_f32 failed \(rc=-10003\).*form 77"):
        _lib.check_clientloop(rc, "fedavg_client_sgd_step_gated_f32")
    _lib.check_clientloop(0, "fedavg_client_sgd_step_gated_f32")
