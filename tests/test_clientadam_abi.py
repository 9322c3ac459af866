"""libfedavg_amd_clientadam.so (include/fedavg_amd_clientadam.h), the seventh
native library: what test_clientstep_abi.py asserts of the sixth (exports
equal the header and the signature table, a gfx950 code object that reads no
environment, no project library among NEEDED, the listed kernel set, no
scratch and no spills, the loader's four refusals word for word), then the
span / workspace / partials arithmetic and every refusal of
fedavg_client_adam_step_*.

CPU only: sizes, tables and alignments are validated before any HIP call, and
the span, workspace and partials functions are host arithmetic.
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
HEADER = "fedavg_amd_clientadam.h"
FILE = "libfedavg_amd_clientadam.so"
STEP = ("fedavg_client_adam_step_f32", "fedavg_client_adam_step_bf16", "fedavg_client_adam_step_f16",
        "fedavg_client_adam_step_f64")
DECLARED = ("fedavg_clientadam_abi_version", "fedavg_clientadam_last_error", "fedavg_client_adam_span",
            "fedavg_client_adam_workspace", "fedavg_client_adam_partials", *STEP)
OTHER_HEADERS = ("fedavg_amd.h", "fedavg_amd_tuning.h", "fedavg_amd_fusedvec.h", "fedavg_amd_segvec.h",
                 "fedavg_amd_clientvec.h", "fedavg_amd_clientstep.h")
OTHER_TABLES = ("SIGNATURES", "TUNING_SIGNATURES", "FUSEDVEC_SIGNATURES", "SEGVEC_SIGNATURES", "CLIENTVEC_SIGNATURES",
                "CLIENTSTEP_SIGNATURES")
OTHER_KERNELS = ("product_kernels.txt", "fusedvec_kernels.txt", "segvec_kernels.txt", "clientvec_kernels.txt",
                 "clientstep_kernels.txt")
ES = {"f32": 4, "bf16": 2, "f16": 2, "f64": 8}
NOT_BUILT = "{path} not built: run __graft_entry__.build(); there is no fallback for the fused client Adam step"


def es_of(entry):
    return ES[entry.rsplit("_", 1)[1]]


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load_clientadam()


# ------------------------------------------------------------------ structure
def test_the_description_keeps_six_and_adds_one_in_a_third_tuple():
    assert len(build.ALL_LIBS) == 6 and len(build.EVERY_LIB) == 7
    assert build.EVERY_LIB == build.ALL_LIBS + build.NEWER_LIBS
    d = build.DESCRIBED["clientadam"]
    assert tuple(lib.key for lib in build.NEWER_LIBS) == ("clientadam",) and d is build.NEWER_LIBS[0]
    assert "clientadam" not in build.BY_KEY and set(build.DESCRIBED) == set(build.BY_KEY) | {"clientadam"}
    assert d.path == build.CLIENTADAM_LIB_PATH == build.LIB_DIR / FILE and d.header == HEADER
    assert d.abi == ("fedavg_clientadam_abi_version", 1) and d.needs == "" and d.link == ()
    assert set(_lib._BINDING) == set(build.DESCRIBED)
    assert (ROOT / "include" / HEADER).exists() and all(src.exists() for src in d.sources)
    assert set(d.sources) <= set(build.sources())


def test_exports_are_exactly_the_header(lib):
    declared = declared_functions((HEADER,))
    assert declared == sorted(DECLARED)
    assert _exported(build.CLIENTADAM_LIB_PATH) == declared
    assert sorted(_lib.CLIENTADAM_SIGNATURES) == declared
    for other in OTHER_HEADERS:
        assert not set(declared) & set(declared_functions((other,))), other
    for other in OTHER_TABLES:
        assert not set(_lib.CLIENTADAM_SIGNATURES) & set(getattr(_lib, other)), other
    raw = ctypes.CDLL(str(build.CLIENTADAM_LIB_PATH))
    assert all(hasattr(raw, name) for name in declared)
    assert lib.fedavg_clientadam_abi_version() == _lib.CLIENTADAM_ABI_VERSION == 1


def test_gfx950_code_object_and_no_environment_variable(lib):
    data = build.CLIENTADAM_LIB_PATH.read_bytes()
    assert b"gfx950" in data
    assert b"getenv" not in data


def test_needs_no_project_library(lib):
    out = subprocess.run(["readelf", "-d", str(build.CLIENTADAM_LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    assert "libfedavg_amd" not in "".join(ln for ln in out.splitlines() if "NEEDED" in ln)


@pytest.fixture(scope="module")
def inventory(lib):
    spec = importlib.util.spec_from_file_location("kernel_inventory", ROOT / "scripts" / "kernel_inventory.py")
    inv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(inv)
    if not inv.have_tools():
        pytest.skip("llvm-objcopy / llvm-readelf not found")
    return inv.inventory(build.CLIENTADAM_LIB_PATH)


def test_kernel_set_is_the_listed_one_and_disjoint(inventory):
    listed = (HERE / "clientadam_kernels.txt").read_text().splitlines()
    built_set = sorted(inventory)
    assert sorted(set(built_set) - set(listed)) == [], "kernels built but not listed"
    assert sorted(set(listed) - set(built_set)) == [], "kernels listed but not built"
    assert built_set == listed and len(built_set) == 9  # 4 dtypes x {first, later} and the finalize
    for other in OTHER_KERNELS:
        assert not set(listed) & set((HERE / other).read_text().splitlines()), other


def test_no_instance_uses_scratch(inventory):
    for name, row in inventory.items():
        assert row["scratch"] == 0 and row["vgpr_spill"] == 0 and row["sgpr_spill"] == 0, (name, row)


# ---------------------------------------------------------------- the loader's refusals, word for word
def refusal():
    with pytest.raises(_lib.FedAvgLibraryError) as info:
        _lib.load_clientadam()
    assert _lib._clientadam is None  # a refused load leaves nothing cached
    return str(info.value)


def test_load_refuses_a_missing_file(lib, monkeypatch, tmp_path):
    path = tmp_path / FILE
    monkeypatch.setattr(_lib, "CLIENTADAM_LIB_PATH", path)
    monkeypatch.setattr(_lib, "_clientadam", None)
    assert refusal() == NOT_BUILT.format(path=path)


def test_load_refuses_a_file_that_does_not_load(lib, monkeypatch, tmp_path):
    path = tmp_path / FILE
    path.touch()
    monkeypatch.setattr(_lib, "CLIENTADAM_LIB_PATH", path)
    monkeypatch.setattr(_lib, "_clientadam", None)
    text = refusal()
    head = f"{path} does not load: "
    assert text.startswith(head) and str(path) in text[len(head):]  # the dynamic loader's own words follow


def test_load_refuses_a_library_without_a_typed_name(lib, monkeypatch):
    monkeypatch.setitem(_lib.CLIENTADAM_SIGNATURES, "fedavg_no_such_entry", (ctypes.c_int, []))
    monkeypatch.setattr(_lib, "_clientadam", None)
    assert refusal() == f"{build.CLIENTADAM_LIB_PATH} does not export fedavg_no_such_entry"


def test_load_refuses_another_abi_version(lib, monkeypatch):
    d = build.DESCRIBED["clientadam"]
    monkeypatch.setitem(build.DESCRIBED, "clientadam", dataclasses.replace(d, abi=(d.abi[0], 2)))
    monkeypatch.setattr(_lib, "_clientadam", None)
    assert refusal() == "ABI version 1 != expected 2; rebuild the library"


# ------------------------------------------------------------------ arithmetic
def test_span_workspace_and_partials_literal_values(lib):
    span, ws, parts = lib.fedavg_client_adam_span, lib.fedavg_client_adam_workspace, lib.fedavg_client_adam_partials
    assert span(4) == 4096 and span(2) == 8192 and span(8) == 2048  # 16 KiB of the tensor
    for es in (0, 1, 3, 16, -2):
        assert span(es) == 0
    assert ws(0) == 0 and ws(-1) == 0 and ws(1) == 40 and ws(3) == 120 and ws(5) == 200  # five fields per key
    # numels [1], [4096], [4097, 0, 63] at each element size: 3 doubles per unit
    want = {4: (3, 3, 9), 2: (3, 3, 6), 8: (3, 6, 12)}
    for es, (one, unit, three) in want.items():
        for numels, doubles in (([1], one), ([4096], unit), ([4097, 0, 63], three)):
            numel = np.array(numels, np.int64)
            assert parts(numel.ctypes.data, len(numel), es) == doubles, (es, numels)
        numel = np.array([4097, 0, 63], np.int64)
        assert parts(None, 3, es) == 0 and parts(numel.ctypes.data, 0, es) == 0
        assert parts(numel.ctypes.data, -1, es) == 0
        empty = np.zeros(3, np.int64)
        assert parts(empty.ctypes.data, 3, es) == 0
    numel = np.array([5], np.int64)
    for es in (0, 1, 3, 16):
        assert parts(numel.ctypes.data, 1, es) == 0


# ------------------------------------------------------------------ refusals
# argument positions of fedavg_client_adam_step_*
W, G, NUMEL, OFFSET, NKEYS, STATE, NSTATE, COEF, FIRST, FORM, PARTS, NPARTS, STATS, HOST, DEV, WS, STREAM = range(17)
COEFS = (0.001, 0.1, 0.999, 0.001, 0.0316, 1e-8, -0.01)


def _args(n_keys=2, ws=80, parts=6, form=15, w=(4096, 8192), g=(12288, 16384), numel=(5, 7), offset=(0, 16),
          state_elems=64, coef=COEFS):
    keep = [np.array(w, np.int64), np.array(g, np.int64), np.array(numel, np.int64), np.array(offset, np.int64),
            np.array(coef, np.float64)]
    buf = np.zeros(64, np.float64)  # a host address where only non-null matters (rejected before any use)
    args = [keep[0].ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data, keep[3].ctypes.data, n_keys, 20480,
            state_elems, keep[4].ctypes.data, 0, form, buf.ctypes.data, parts, buf.ctypes.data, 4096, 8192, ws, None]
    return args, keep + [buf]


def _with(i, value):
    c = list(COEFS)
    c[i] = value
    return tuple(c)


def _cases(es):
    per = 16 // es
    return [
        (dict(n_keys=-1), "EINVAL", b"negative"),                       # a negative count
        (dict(state_elems=-16), "EINVAL", b"negative"),
        (dict(numel=(5, -1)), "EINVAL", b"negative"),                   # a negative key size
        (dict(form=16), "EMODE", b"form 16"),
        (dict(form=-1), "EMODE", b"form -1"),
        (dict(coef=_with(1, 0.5)), "EMODE", b"lerp"),                   # 1 - beta1 >= 0.5: Lerp.h's other branch
        (dict(coef=_with(1, 0.75)), "EMODE", b"lerp"),
        (dict(coef=_with(1, float("nan"))), "EMODE", b"lerp"),
        (dict(w=(0, 8192)), "EINVAL", b"null tensor"),                  # null tensors, either side
        (dict(g=(12288, 0)), "EINVAL", b"null tensor"),
        (dict(w=(4096, 8192 + es // 2)), "EINVAL", b"multiple of %d bytes" % es),  # not aligned to the element size
        (dict(g=(12288 + es // 2, 16384)), "EINVAL", b"multiple of %d bytes" % es),
        (dict(offset=(0, 64)), "EINVAL", b"key 1 lies outside a state plane of 64"),   # 64 + 7 > 64
        (dict(offset=(-16, 16)), "EINVAL", b"key 0 lies outside"),
        (dict(offset=(0, 16 + per // 2)), "EALIGN", b"key 1: state offset must be a multiple of %d" % per),
        (dict(state_elems=64 + per // 2), "EALIGN", b"state_elems a multiple of %d" % per),
        (dict(ws=79), "EINVAL", b"workspace needs 80 bytes"),
        (dict(parts=5), "EINVAL", b"partials need 6 doubles"),
    ]


@pytest.mark.parametrize("entry", STEP)
def test_step_rejects_bad_arguments_without_gpu(lib, entry):
    es = es_of(entry)
    fn = getattr(lib, entry)
    for change, code, words in _cases(es):
        args, keep = _args(**change)
        rc = fn(*args)
        msg = lib.fedavg_clientadam_last_error()
        assert rc == getattr(_lib, "FEDAVG_" + code), (change, rc, msg)
        assert msg.startswith(entry.encode()) and words in msg, (change, msg)
    # misaligned state, workspaces, partials and stats
    for idx, off in ((STATE, 8), (HOST, 8), (DEV, 8), (PARTS, 4), (STATS, 4)):
        args, keep = _args()
        args[idx] += off
        assert fn(*args) == _lib.FEDAVG_EALIGN, idx
        assert lib.fedavg_clientadam_last_error().startswith(entry.encode())
    # null tables and buffers
    for idx in (W, G, NUMEL, OFFSET, STATE, COEF, PARTS, STATS, HOST, DEV):
        args, keep = _args()
        args[idx] = None
        assert fn(*args) == _lib.FEDAVG_EINVAL, idx
        assert lib.fedavg_clientadam_last_error().startswith(entry.encode()) and b"null" in \
            lib.fedavg_clientadam_last_error()
    # a tensor that is element-aligned but not 16-B aligned is NOT refused for that (the element path takes it), and
    # every mask is a form: the call gets as far as the pointer-attribute checks, which nothing passes without a GPU
    for change in (dict(w=(4096 + es, 8192)), dict(g=(12288 + es, 16384)), dict(form=0), dict(form=15), dict()):
        args, keep = _args(**change)
        assert fn(*args) == _lib.FEDAVG_EINVAL
        assert b"pinned" in lib.fedavg_clientadam_last_error() or b"device memory" in lib.fedavg_clientadam_last_error()
    # no keys, or keys without elements: nothing to launch, and stats (a host address here) is refused as not device
    # memory rather than written
    for change in (dict(n_keys=0), dict(numel=(0, 0), parts=0)):
        args, keep = _args(**change)
        assert fn(*args) == _lib.FEDAVG_EINVAL
        assert b"stats must be device memory" in lib.fedavg_clientadam_last_error()


def test_check_clientadam_raises_with_the_librarys_message(lib):
    args, keep = _args(form=77)
    rc = lib.fedavg_client_adam_step_f32(*args)
    with pytest.raises(_lib.FedAvgLibraryError, match=r"fedavg_client_adam_step_f32 failed \(rc=-10003\).*form 77"):
        _lib.check_clientadam(rc, "fedavg_client_adam_step_f32")
    _lib.check_clientadam(0, "fedavg_client_adam_step_f32")
