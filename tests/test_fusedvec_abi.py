"""libfedavg_amd_fusedvec.so (include/fedavg_amd_fusedvec.h): argument validation
and the plan / workspace arithmetic (exports, kernel set and no scratch:
test_native_libs.py).

CPU only: argument validation runs before any HIP call, and the plan and
workspace functions are host arithmetic.
"""
import pytest

from mfl_amd import _lib, build

# the fused ranges the header states
FUSED_MAX_K = {8: 64, 2: 128}


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load_fusedvec()


@pytest.mark.parametrize("entry", ["fedavg_reduce_sqdist_f64", "fedavg_reduce_sqdist_f16", "fedavg_reduce_sqdist_bf16"])
@pytest.mark.parametrize("K,P,ld", [(0, 16, 16), (-1, 16, 16), (2, 16, 8), (2, -1, 0), (1 << 31, 16, 16)])
def test_rejects_bad_sizes_without_gpu(lib, entry, K, P, ld):
    rc = getattr(lib, entry)(None, K, P, ld, None, None, None, 0, None, None)
    assert rc == _lib.FEDAVG_EINVAL
    assert lib.fedavg_fusedvec_last_error().startswith(entry.encode())


@pytest.mark.parametrize("entry", ["fedavg_reduce_sqdist_f64", "fedavg_reduce_sqdist_f16", "fedavg_reduce_sqdist_bf16"])
def test_null_buffers_rejected_without_gpu(lib, entry):
    import numpy as np

    buf = np.zeros(256, np.float64)
    p = buf.ctypes.data
    fn = getattr(lib, entry)
    for args in ((None, 2, 16, 16, p, p, p, 64, p, None), (p, 2, 16, 16, None, p, p, 64, p, None),
                 (p, 2, 16, 16, p, None, p, 64, p, None), (p, 2, 16, 16, p, p, None, 64, p, None),
                 (p, 2, 16, 16, p, p, p, 64, None, None)):
        assert fn(*args) == _lib.FEDAVG_EINVAL, args
    # misaligned rows / stride / out: refused before any work (host pointers never reach a kernel)
    es = 8 if entry.endswith("f64") else 2
    assert fn(p + es, 2, 16, 16, p, p, p, 64, p, None) == _lib.FEDAVG_EALIGN
    assert fn(p, 2, 15, 17, p, p, p, 64, p, None) == _lib.FEDAVG_EALIGN  # a row stride of 34 / 136 bytes
    assert fn(p, 2, 16, 16, p, p + es, p, 64, p, None) == _lib.FEDAVG_EALIGN


def test_plan_covers_the_stated_ranges(lib):
    for es, kmax in FUSED_MAX_K.items():
        for bf in (0, 1):
            for P in (1, 63, 4097, 1_200_000, 25_000_000):
                seen = set()
                for K in range(1, kmax + 1):
                    code = lib.fedavg_fused_vec_plan_of(K, P, es, bf)
                    kind, S, slots = code // 1_000_000, code // 100 % 10_000, code % 100
                    assert kind == 3 and S >= K and slots in (4, 8, 16) and slots % (2 if es == 2 else 8) == 0, (K, code)
                    seen.add((S, slots))
                assert len(seen) == (5 if es == 2 else 3)
                for K in (kmax + 1, kmax + 2, 1000, 5000):
                    assert lib.fedavg_fused_vec_plan_of(K, P, es, bf) == 0
        assert lib.fedavg_fused_vec_plan_of(0, 100, es, 0) == 0
        assert lib.fedavg_fused_vec_plan_of(4, 0, es, 0) == 0
    assert lib.fedavg_fused_vec_plan_of(4, 100, 4, 0) == 0  # fp32 rows: fedavg_reduce_sqdist_f32


def test_workspace_is_monotone_and_covers_both_routes(lib):
    """The instance a plan names writes K x waves partials, waves = 4 x
    min(ceil(windows / 4), 256 CUs x workgroups per CU) with windows of 64
    lanes x `slots` bytes and at most 4 workgroups per CU; the two-pass route
    needs the distance pass's workspace."""
    prod = _lib.load()
    ws = lib.fedavg_reduce_sqdist_vec_workspace
    Ks = (1, 2, 16, 17, 32, 33, 64, 65, 100, 101, 128, 129, 500, 2000)
    Ps = (1, 7, 64, 129, 4097, 100_003, 1_200_000, 11_200_000, 25_000_000)
    for es in (2, 8):
        for K in Ks:
            for P in Ps:
                n = ws(K, P, es)
                code = lib.fedavg_fused_vec_plan_of(K, P, es, 0)
                if code:
                    slots = code % 100
                    windows = -(-P * es // (64 * slots))
                    assert n >= K * 4 * min(-(-windows // 4), 256 * 4), (es, K, P)
                assert n >= prod.fedavg_client_sqdist_workspace_elems(K, P, es), (es, K, P)
        for P in Ps:
            vals = [ws(K, P, es) for K in Ks]
            assert vals == sorted(vals) and vals[0] > 0
        for K in Ks:
            vals = [ws(K, P, es) for P in Ps]
            assert vals == sorted(vals)
        assert ws(0, 10, es) == 0 and ws(3, 0, es) == 0
    assert ws(3, 10, 4) == 0 and ws(3, 10, 3) == 0


def test_p_zero_is_noop(lib):
    """P == 0 returns 0 (with a sumsq it is zeroed on the stream: the GPU tests)."""
    for entry in ("fedavg_reduce_sqdist_f64", "fedavg_reduce_sqdist_f16", "fedavg_reduce_sqdist_bf16"):
        assert getattr(lib, entry)(None, 3, 0, 0, None, None, None, 0, None, None) == 0


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "FUSEDVEC_LIB_PATH", tmp_path / "libfedavg_amd_fusedvec.so")
    monkeypatch.setattr(_lib, "_fusedvec", None)
    with pytest.raises(_lib.FedAvgLibraryError):
        _lib.load_fusedvec()


def test_eligibility_of_the_three_dtypes(monkeypatch):
    """aggregate.fuse_eligible_vec: fp64 / fp16 / bf16 rows with start and
    stride multiples of 16 BYTES; column chunks keep that."""
    import sys

    import torch

    import mfl_amd

    A = sys.modules[mfl_amd.DeviceAggregator.__module__]
    for dt in (torch.float64, torch.float16, torch.bfloat16):
        es = torch.empty((), dtype=dt).element_size()
        per16 = 16 // es
        rows = torch.empty((10, 64 + per16), dtype=dt)
        assert A.fuse_eligible_vec(torch.empty((1, 64), dtype=dt))
        assert A.fuse_eligible_vec(torch.empty((1024, 64), dtype=dt)) and not A.fuse_eligible_vec(
            torch.empty((1025, 64), dtype=dt))
        assert A.fuse_eligible_vec(rows[:, :64]) and A.fuse_eligible_vec(rows[:, per16:64 + per16])
        assert not A.fuse_eligible_vec(rows[:, 1:65])  # start 2 or 8 bytes off
        assert not A.fuse_eligible_vec(torch.empty((10, 64 + per16 // 2), dtype=dt)[:, :64])  # stride 8 bytes off
        assert not A.fuse_eligible_vec(torch.empty((0, 64), dtype=dt))
        out = torch.empty(64 + per16, dtype=dt)
        assert A.fuse_eligible_vec(rows[:, :64], out) and not A.fuse_eligible_vec(rows[:, :64], out[1:])
    assert not A.fuse_eligible_vec(torch.empty((10, 64)))  # fp32: fuse_eligible's
    for P in (1, 1000, (2 << 20) * 3 + 5, 25_000_003):
        for c0, _ in A.column_chunks(P):
            assert (c0 * 2) % 16 == 0
    monkeypatch.setattr(A, "FUSE_DISTANCES", False)
    assert not A.fuse_eligible_vec(torch.empty((10, 64), dtype=torch.bfloat16))
