"""libfedavg_amd_segvec.so (include/fedavg_amd_segvec.h): argument validation
and the plan / workspace arithmetic (exports, kernel set and no scratch:
test_native_libs.py).

CPU only: sizes, tables and sources are validated before any HIP call, and
the plan, workspace and partials functions are host arithmetic.
"""
import numpy as np
import pytest

from mfl_amd import _lib, build

ENTRIES = ("fedavg_device_round_f64", "fedavg_device_round_f16", "fedavg_device_round_bf16")
ES = {"fedavg_device_round_f64": 8, "fedavg_device_round_f16": 2, "fedavg_device_round_bf16": 2}
MAX_K = {8: 64, 2: 128}  # the one-wave bands the header states


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load_segvec()


class _Round:
    """A valid 3-key, 2-client call on host memory (fake, 16-B aligned device
    addresses: nothing dereferences them before the pointer-attribute checks,
    which no CPU test gets past)."""

    def __init__(self, lib, K=2, numel=(5, 0, 300)):
        self.K, self.n = K, len(numel)
        self.ptrs = np.array([[0x7F0000000000 + ((k * self.n + j) << 8) for j in range(self.n)] for k in range(K)],
                             dtype=np.int64)
        self.numel = np.array(numel, dtype=np.int64)
        self.offset = np.concatenate([[0], np.cumsum(self.numel)[:-1]]).astype(np.int64)
        self.w = np.full(K, 1.0 / K)
        self.buf = np.zeros(1 << 16, dtype=np.float64)  # stands in for out / partials / sumsq / dev_ws
        need = lib.fedavg_device_round_vec_workspace(K, self.n)
        self.ws = np.zeros(need // 8 + 2, dtype=np.float64)
        self.ws_bytes = need

    def args(self, **kw):
        p = self.buf.ctypes.data
        a = dict(client_ptrs=self.ptrs.ctypes.data, ptr_ld=self.n, key_index=None, key_numel=self.numel.ctypes.data,
                 key_offset=self.offset.ctypes.data, n_keys=self.n, K=self.K, weights=self.w.ctypes.data, out=p,
                 partials=p, partial_elems=self.buf.size, sumsq=p, host_ws=self.ws.ctypes.data, dev_ws=p,
                 ws_bytes=self.ws_bytes, stream=None)
        a.update(kw)
        return list(a.values())


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_validation_without_gpu(lib, entry):
    fn = getattr(lib, entry)
    r = _Round(lib)
    assert r.ws.ctypes.data % 16 == 0 and r.buf.ctypes.data % 16 == 0

    def refused(code=_lib.FEDAVG_EINVAL, **kw):
        lib_rc = fn(*r.args(**kw))
        assert lib_rc == code, (kw, lib_rc, lib.fedavg_segvec_last_error())
        assert lib.fedavg_segvec_last_error().startswith(entry.encode()), kw

    refused(K=0)
    refused(K=-3)
    refused(n_keys=-1)
    refused(n_keys=0)
    for null in ("client_ptrs", "key_numel", "key_offset", "weights", "out", "partials", "sumsq", "host_ws", "dev_ws"):
        refused(**{null: None})
    refused(ptr_ld=r.n - 1)  # key_index NULL: the row must hold every key's column
    refused(ws_bytes=r.ws_bytes - 1)  # one byte short
    refused(partial_elems=0)
    bad = r.numel.copy()
    bad[2] = -1
    refused(key_numel=bad.ctypes.data)
    bad = r.offset.copy()
    bad[0] = -8
    refused(key_offset=bad.ctypes.data)
    idx = np.array([0, 1, 7], dtype=np.int64)  # a column outside the pointer row
    refused(key_index=idx.ctypes.data)
    ptrs = r.ptrs.copy()
    ptrs[1, 2] = 0  # a null source of a non-empty key
    refused(client_ptrs=ptrs.ctypes.data)
    ptrs = r.ptrs.copy()
    ptrs[1, 0] += ES[entry]  # 2 B / 8 B off 16-B alignment
    refused(code=_lib.FEDAVG_EALIGN, client_ptrs=ptrs.ctypes.data)
    ptrs = r.ptrs.copy()
    ptrs[:, 1] = (0, 3)  # the EMPTY key's sources are never read: not refused for them
    rc = fn(*r.args(client_ptrs=ptrs.ctypes.data))
    assert rc not in (_lib.FEDAVG_EALIGN, _lib.FEDAVG_EMODE)
    # beyond the bands: the caller packs rows
    big = _Round(lib, K=MAX_K[ES[entry]] + 1)
    assert fn(*big.args()) == _lib.FEDAVG_EMODE
    assert lib.fedavg_segvec_last_error().startswith(entry.encode())
    # a valid call on host memory stops at the pointer checks (no GPU: nothing is device memory), before any launch
    assert fn(*r.args()) == _lib.FEDAVG_EINVAL


def test_plan_names_one_band_per_k(lib):
    plan = lib.fedavg_device_round_vec_plan_of
    fused = _lib.load_fusedvec().fedavg_fused_vec_plan_of
    for es, kmax in MAX_K.items():
        for bf in (0, 1):
            seen = []
            for K in range(1, kmax + 1):
                code = plan(K, es, bf)
                kind, S, sb = code // 1_000_000, code // 100 % 10_000, code % 100
                assert kind == 3 and S >= K and sb in (4, 8, 16) and sb % (2 if es == 2 else 8) == 0, (K, code)
                assert code == fused(K, 1000, es, bf)  # the fused-vec library's bands
                if not seen or seen[-1] != (S, sb):
                    seen.append((S, sb))
            assert len(seen) == (5 if es == 2 else 3)
            assert [s for s, _ in seen] == sorted(s for s, _ in seen)  # one band per K, in order
            for K in (kmax + 1, kmax + 2, 1000):
                assert plan(K, es, bf) == 0
        assert plan(0, es, 0) == 0 and plan(-1, es, 0) == 0
    assert plan(4, 4, 0) == 0 and plan(4, 3, 0) == 0  # fp32: fedavg_device_round_f32


def test_workspace_and_partials_are_monotone(lib):
    ws, parts = lib.fedavg_device_round_vec_workspace, lib.fedavg_device_round_vec_partials
    Ks = (1, 2, 16, 17, 32, 33, 64, 65, 100, 101, 128)
    Ns = (1, 2, 62, 350, 5000, 100_000)
    for K in Ks:
        vals = [ws(K, n) for n in Ns]
        assert vals == sorted(vals) and vals[0] > 0 and all(v % 16 == 0 for v in vals)
    for n in Ns:
        vals = [ws(K, n) for K in Ks]
        assert vals == sorted(vals)
        # key table, the padded pointer table, the weights
        assert all(ws(K, n) >= 32 * n + 8 * (n * K + 128) + 8 * K for K in Ks)
    assert ws(0, 5) == 0 and ws(5, 0) == 0 and ws(-1, 5) == 0 and ws(5, -1) == 0
    for es in (2, 8):
        vals = [parts(K, es) for K in Ks]
        assert vals == sorted(vals) and vals[0] > 0
        # no instance launches more than 4 workgroups of 4 waves on each of 256 CUs
        assert all(parts(K, es) >= K * 256 * 4 * 4 for K in Ks)
        assert parts(0, es) == 0 and parts(-2, es) == 0
    for es in (0, 1, 3, 4, 16):
        assert parts(8, es) == 0


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "SEGVEC_LIB_PATH", tmp_path / "libfedavg_amd_segvec.so")
    monkeypatch.setattr(_lib, "_segvec", None)
    with pytest.raises(_lib.FedAvgLibraryError):
        _lib.load_segvec()
