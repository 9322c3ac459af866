"""libfedavg_amd_clientvec.so (include/fedavg_amd_clientvec.h): argument
validation and the span / workspace / partials arithmetic (exports, kernel
set and no scratch: test_native_libs.py).

CPU only: sizes, tables and alignments are validated before any HIP call, and
the span, workspace and partials functions are host arithmetic.
"""
import numpy as np
import pytest

from mfl_amd import _lib, build

STATS = ("fedavg_client_stats_bf16", "fedavg_client_stats_f16", "fedavg_client_stats_f64")
TRACK = ("fedavg_client_track_bf16", "fedavg_client_track_f16", "fedavg_client_track_f64")
ES = {"bf16": 2, "f16": 2, "f64": 8}
SPAN = {2: 8192, 8: 2048}


def es_of(entry):
    return ES[entry.rsplit("_", 1)[1]]


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load_clientvec()


# ------------------------------------------------------------------ arithmetic
def test_span_workspace_and_partials_arithmetic(lib):
    span, ws, parts = (lib.fedavg_client_stats_vec_span, lib.fedavg_client_stats_vec_workspace,
                       lib.fedavg_client_stats_vec_partials)
    assert span(2) == 8192 and span(8) == 2048  # 16 KiB of the tensor
    for es in (0, 1, 3, 4, 16, -2):
        assert span(es) == 0
    assert ws(0) == 0 and ws(-1) == 0 and ws(1) == 32 and ws(5) == 5 * 32
    for es, sp in SPAN.items():
        for n, units in ((0, 0), (1, 1), (sp - 1, 1), (sp, 1), (sp + 1, 2), (3 * sp + 5, 4)):
            one = np.array([n], np.int64)
            assert parts(one.ctypes.data, 1, es) == 3 * units, (es, n)
        numel = np.array([1, 0, sp, sp + 1, 0, 3 * sp + 5, sp - 1], np.int64)  # empty keys take no unit
        assert parts(numel.ctypes.data, len(numel), es) == 3 * (1 + 0 + 1 + 2 + 0 + 4 + 1)
        empty = np.zeros(3, np.int64)
        assert parts(empty.ctypes.data, 3, es) == 0
        assert parts(None, 3, es) == 0 and parts(numel.ctypes.data, 0, es) == 0 and parts(numel.ctypes.data, -1, es) == 0
    numel = np.array([5], np.int64)
    for es in (0, 1, 4, 16):
        assert parts(numel.ctypes.data, 1, es) == 0


# ------------------------------------------------------------------ refusals
def _stats_args(es, n_keys=2, P=32, ws=64, parts=6, snap=1024, ptrs=(4096, 8192), numel=(5, 7), offset=(0, 16)):
    keep = [np.array(ptrs, np.int64), np.array(numel, np.int64), np.array(offset, np.int64)]
    buf = np.zeros(64, np.float64)  # a host address where only non-null matters (rejected before any use)
    args = [keep[0].ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data, n_keys, snap, P, 1, buf.ctypes.data,
            parts, buf.ctypes.data, 4096, 8192, ws, None]
    return args, keep + [buf]


def _cases(es):
    per16 = 16 // es
    return [
        (dict(n_keys=-1), "EINVAL"),
        (dict(P=-1), "EINVAL"),
        (dict(ws=63), "EINVAL"),                         # workspace too small for 2 keys
        (dict(parts=5), "EINVAL"),                       # partials too small for 2 units
        (dict(numel=(5, -1)), "EINVAL"),                 # a negative key size
        (dict(offset=(0, -16)), "EINVAL"),               # a negative offset
        (dict(offset=(0, 32)), "EINVAL"),                # key runs past P
        (dict(offset=(0, 16), numel=(5, 17)), "EINVAL"),  # its end does
        (dict(ptrs=(4096, 8192 + es // 2)), "EINVAL"),   # tensor address no multiple of the element size
        (dict(ptrs=(0, 8192)), "EINVAL"),                # null tensor
        (dict(snap=None), "EINVAL"),
        (dict(snap=1024 + es), "EALIGN"),                # snapshot not 16-B aligned
        (dict(offset=(0, 16 + per16 // 2)), "EALIGN"),   # snapshot key offset not a multiple of 16 B
    ]


@pytest.mark.parametrize("entry", STATS)
def test_stats_rejects_bad_arguments_without_gpu(lib, entry):
    es = es_of(entry)
    fn = getattr(lib, entry)
    for change, code in _cases(es):
        args, keep = _stats_args(es, **change)
        rc = fn(*args)
        assert rc == getattr(_lib, "FEDAVG_" + code), (change, rc, lib.fedavg_clientvec_last_error())
        assert lib.fedavg_clientvec_last_error().startswith(entry.encode()), change
    # misaligned workspaces
    for idx in (10, 11):
        args, keep = _stats_args(es)
        args[idx] += 8
        assert fn(*args) == _lib.FEDAVG_EALIGN, idx
        assert lib.fedavg_clientvec_last_error().startswith(entry.encode())
    # a tensor that is element-aligned but not 16-B aligned is NOT refused for that (the scalar form reads it):
    # the call gets as far as the pointer-attribute checks, which nothing passes without a GPU
    args, keep = _stats_args(es, ptrs=(4096 + es, 8192))
    assert fn(*args) == _lib.FEDAVG_EINVAL
    assert b"pinned" in lib.fedavg_clientvec_last_error() or b"device memory" in lib.fedavg_clientvec_last_error()


@pytest.mark.parametrize("entry", STATS)
def test_stats_null_tables_and_buffers_rejected(lib, entry):
    for idx in (0, 1, 2, 7, 9, 10, 11):  # cur_ptrs, key_numel, key_offset, partials, stats, host_ws, dev_ws
        args, keep = _stats_args(es_of(entry))
        args[idx] = None
        assert getattr(lib, entry)(*args) == _lib.FEDAVG_EINVAL, idx
        assert lib.fedavg_clientvec_last_error().startswith(entry.encode())


@pytest.mark.parametrize("entry", TRACK)
def test_track_rejects_bad_arguments_without_gpu(lib, entry):
    fn = getattr(lib, entry)
    buf = np.zeros(8, np.float64)
    p = buf.ctypes.data
    assert fn(None, p, p, 0.5, None) == _lib.FEDAVG_EINVAL
    assert fn(p, None, p, 0.5, None) == _lib.FEDAVG_EINVAL
    assert fn(p, p, None, 0.5, None) == _lib.FEDAVG_EINVAL
    assert lib.fedavg_clientvec_last_error().startswith(entry.encode())
    assert fn(p + 4, p, p, 0.5, None) == _lib.FEDAVG_EALIGN
    assert lib.fedavg_clientvec_last_error().startswith(entry.encode())
    # host memory is not device memory: refused before any launch
    assert fn(p, p, p, 0.5, None) == _lib.FEDAVG_EINVAL


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "CLIENTVEC_LIB_PATH", tmp_path / "libfedavg_amd_clientvec.so")
    monkeypatch.setattr(_lib, "_clientvec", None)
    with pytest.raises(_lib.FedAvgLibraryError):
        _lib.load_clientvec()
