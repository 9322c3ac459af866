"""Launch geometry and workspace contract of the fused aggregate + :291 passes.

Geometry: every plan, workspace and partials figure the libraries answer --
the sizes of the grids their launches take -- equals, value for value, the
figures recorded from the commit named in tests/launch_geometry_parent.json
(``scripts/record_launch_geometry.py``, run at that commit on an MI355X).
Same kernels + same grid, block and LDS = the same launch.  No kernel runs.

Workspace contract: a workspace one double short of what a launch needs is
refused with FEDAVG_EINVAL before anything is written (``out`` and ``sumsq``
keep their sentinel), the message starts with the entry point's name, and
the exact size succeeds -- one case per plan kind of the rows pass, the
zero-copy tile, window and split forms, and the fp64 / fp16 / bf16 pass.
(A null workspace, bad sizes and unaligned rows: test_fusedvec_abi,
test_gpu_fused_vec::test_fused_vec_unaligned_rows_are_refused,
test_gpu_fused::test_fused_rejects_unaligned_rows,
test_gpu_device_round::test_device_round_refusals.)
"""
import importlib.util
import json
import re
from pathlib import Path

import numpy as np
import pytest

from mfl_amd import _lib

ROOT = Path(__file__).resolve().parents[1]
FIXTURE = Path(__file__).with_name("launch_geometry_parent.json")

# every edge of fused_plan, the window hole and the windows-per-wave rule
ROW_K = [1, 2, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 96, 97, 100, 101, 128, 129, 159, 160, 192, 193, 256, 257, 288,
         289, 320, 321, 368, 369, 512, 513, 1024, 1025]
ROW_P = [1, 63, 64, 4097, 100003, 399999, 400000, 1200000, 11227812, 25000000]
SEG_K = [1, 16, 17, 100, 128, 129, 256, 257, 500, 1024]
# test_fusedvec_abi's grids
VEC_K = [1, 2, 16, 17, 32, 33, 64, 65, 100, 101, 128, 129, 500, 2000]
VEC_P = [1, 7, 64, 129, 4097, 100_003, 1_200_000, 11_200_000, 25_000_000]
VEC_PLAN_K = list(range(1, 131)) + [1000, 5000]
VEC_PLAN_P = [1, 63, 4097, 1_200_000, 25_000_000]


def _key_lists():
    """name -> (key_numel, key_kind): one long key, mnist_lr, resnet56 (its
    num_batches_tracked keys int64, kind 1)."""
    spec = importlib.util.spec_from_file_location("model_shapes", ROOT / "scripts" / "model_shapes.py")
    ms = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ms)
    r56 = ms.resnet56_shapes()
    assert len(r56) == 350
    return {
        "flat_25m": ([25_000_000], [0]),
        "mnist_lr": ([7840, 10], [0, 0]),
        "resnet56": ([int(np.prod(s, dtype=np.int64)) for _, s in r56],
                     [1 if n.endswith("num_batches_tracked") else 0 for n, _ in r56]),
    }


def collect_rows(lib):
    return {
        "K": ROW_K, "P": ROW_P,
        "fused_plan_of": [[lib.fedavg_fused_plan_of(K, P) for P in ROW_P] for K in ROW_K],
        "reduce_sqdist_workspace": [[lib.fedavg_reduce_sqdist_workspace(K, P) for P in ROW_P] for K in ROW_K],
        "client_sqdist_workspace": [[lib.fedavg_client_sqdist_workspace(K, P) for P in ROW_P] for K in ROW_K],
        # the fp16 / bf16 (2), fp32-sized (4) and fp64 (8) distance pass
        "client_sqdist_workspace_elems": {str(es): [[lib.fedavg_client_sqdist_workspace_elems(K, P, es) for P in ROW_P]
                                                    for K in ROW_K] for es in (2, 4, 8)},
    }


def collect_segments(lib):
    got = {"K": SEG_K, "reduce_sqdist_segments_partials": [lib.fedavg_reduce_sqdist_segments_partials(K) for K in SEG_K]}
    for name, (numel, kind) in _key_lists().items():
        n = np.ascontiguousarray(numel, dtype=np.int64)
        k = np.ascontiguousarray(kind, dtype=np.int64)
        got[name] = {
            "segments_partials": [lib.fedavg_segments_partials(n.ctypes.data, len(n), K) for K in SEG_K],
            "device_round_scratch": [lib.fedavg_device_round_scratch(n.ctypes.data, k.ctypes.data, len(n), K)
                                     for K in SEG_K],
        }
    return got


def collect_fusedvec(fv):
    return {
        "K": VEC_K, "P": VEC_P, "plan_K": VEC_PLAN_K, "plan_P": VEC_PLAN_P,
        "reduce_sqdist_vec_workspace": {str(es): [[fv.fedavg_reduce_sqdist_vec_workspace(K, P, es) for P in VEC_P]
                                                  for K in VEC_K] for es in (2, 8)},
        "fused_vec_plan_of": {f"{es}_{bf}": [[fv.fedavg_fused_vec_plan_of(K, P, es, bf) for P in VEC_PLAN_P]
                                             for K in VEC_PLAN_K] for es in (2, 8) for bf in (0, 1)},
    }


def _assert_same(got, want, where):
    """value for value, naming the first figure that differs"""
    if isinstance(want, dict):
        assert sorted(got) == sorted(want), where
        for k in want:
            _assert_same(got[k], want[k], f"{where}.{k}")
    elif isinstance(want, list):
        assert len(got) == len(want), where
        for i, (g, w) in enumerate(zip(got, want)):
            _assert_same(g, w, f"{where}[{i}]")
    else:
        assert got == want, (where, got, want)


@pytest.fixture(scope="module")
def recorded():
    rec = json.loads(FIXTURE.read_text())
    assert re.fullmatch(r"[0-9a-f]{40}", rec["recorded_at_commit"])
    return rec


def test_fusedvec_geometry_is_the_recorded_one(recorded):
    """Host arithmetic only: runs without a GPU."""
    _assert_same(collect_fusedvec(_lib.load_fusedvec()), recorded["fusedvec"], "fusedvec")


@pytest.fixture
def gpu(gpu_available):
    import torch

    _lib.load()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.mark.gpu
def test_rows_geometry_is_the_recorded_one(gpu, recorded):
    _assert_same(collect_rows(_lib.load()), recorded["rows"], "rows")


@pytest.mark.gpu
def test_segments_geometry_is_the_recorded_one(gpu, recorded):
    _assert_same(collect_segments(_lib.load()), recorded["segments"], "segments")


# ---------------------------------------------------------------------------
# Workspace contract
# ---------------------------------------------------------------------------
SENTINEL = 7.0


def _needed(msg: bytes) -> int:
    """the size a refusal names: '... need(s) N doubles'"""
    m = re.search(rb"needs? (\d+) doubles", msg)
    assert m, msg
    return int(m.group(1))


def _untouched(*tensors):
    import torch

    torch.cuda.synchronize()
    for t in tensors:
        assert bool((t == SENTINEL).all())


# (K, P): plan kind 2 (register-staged tiles), 1 (LDS-DMA tiles) twice, 3
# (one-wave windows, in the 65-96 hole), 4 (split-row windows)
ROWS_CASES = [(8, 4097), (32, 4097), (100, 400000), (80, 400000), (369, 4097)]


@pytest.mark.gpu
def test_rows_cases_cover_every_plan_kind(gpu):
    lib = _lib.load()
    assert {lib.fedavg_fused_plan_of(K, P) // 1_000_000 for K, P in ROWS_CASES} == {1, 2, 3, 4}


@pytest.mark.gpu
@pytest.mark.parametrize("K,P", ROWS_CASES)
def test_rows_workspace_one_short_is_refused(gpu, K, P):
    import torch

    lib = _lib.load()
    entry = b"fedavg_reduce_sqdist_f32"
    need = lib.fedavg_reduce_sqdist_workspace(K, P)
    # the fused launch's K x grid doubles, not the two-pass bound, is the size in force
    assert lib.fedavg_fused_plan_of(K, P) != 0 and need > lib.fedavg_client_sqdist_workspace(K, P)
    ld = (P + 63) // 64 * 64
    x = torch.zeros((K, ld), device=gpu)
    w = torch.full((K,), 1.0 / K, device=gpu)
    out = torch.full((P,), SENTINEL, device=gpu)
    sumsq = torch.full((K,), SENTINEL, dtype=torch.float64, device=gpu)
    ws = torch.empty(need, dtype=torch.float64, device=gpu)

    def call(n):
        return lib.fedavg_reduce_sqdist_f32(x.data_ptr(), K, P, ld, w.data_ptr(), out.data_ptr(), ws.data_ptr(), n,
                                            sumsq.data_ptr(), None)

    assert call(need - 1) == _lib.FEDAVG_EINVAL
    msg = lib.fedavg_last_error()
    assert msg.startswith(entry) and _needed(msg) == need
    _untouched(out, sumsq)
    assert call(need) == 0
    torch.cuda.synchronize()
    assert bool((out == 0.0).all()) and bool((sumsq == 0.0).all())


# zero-copy (fedavg_device_round_f32): K clients of (key shapes); the LDS-DMA
# tiles at 8 and 100 clients of mnist_lr, the split-row windows at 300, the
# one-wave windows on a model long enough for them at 17 clients
MNIST_LR = [(10, 784), (10,)]
SEG_CASES = [(8, MNIST_LR), (100, MNIST_LR), (300, MNIST_LR), (17, [(8_500_000,)])]


@pytest.mark.gpu
@pytest.mark.parametrize("K,shapes", SEG_CASES, ids=lambda v: str(v) if isinstance(v, int) else f"{len(v)}keys")
def test_device_round_partials_one_short_are_refused(gpu, K, shapes):
    import torch

    lib = _lib.load()
    entry = b"fedavg_device_round_f32"
    numel = np.array([int(np.prod(s)) for s in shapes], dtype=np.int64)
    offset = np.concatenate([[0], np.cumsum(numel)[:-1]]).astype(np.int64)
    kind = np.zeros(len(shapes), dtype=np.int64)
    n, P = len(shapes), int(numel.sum())
    # client k's key j: row k of keys[j], rows 16-B aligned (a fused round's condition)
    keys = [torch.zeros((K, (int(m) + 3) // 4 * 4), device=gpu) for m in numel]
    ptrs = np.array([[keys[j][k].data_ptr() for j in range(n)] for k in range(K)], dtype=np.int64)
    w64 = np.full(K, 1.0 / K, dtype=np.float64)
    out = torch.full((P,), SENTINEL, device=gpu)
    sumsq = torch.full((K,), SENTINEL, dtype=torch.float64, device=gpu)
    bound = lib.fedavg_reduce_sqdist_segments_partials(K)
    partials = torch.empty(bound, dtype=torch.float64, device=gpu)
    nws = lib.fedavg_device_round_workspace(K, n)
    ws_h = torch.empty(nws, dtype=torch.uint8, pin_memory=True)
    ws_d = torch.empty(nws, dtype=torch.uint8, device=gpu)

    def call(elems):
        rc = lib.fedavg_device_round_f32(ptrs.ctypes.data, n, None, numel.ctypes.data, offset.ctypes.data,
                                         kind.ctypes.data, n, K, w64.ctypes.data, out.data_ptr(),
                                         partials.data_ptr(), elems, sumsq.data_ptr(), None, 0, ws_h.data_ptr(),
                                         ws_d.data_ptr(), nws, None)
        torch.cuda.synchronize()  # the pinned tables are rewritten by the next call
        return rc

    assert call(0) == _lib.FEDAVG_EINVAL
    need = _needed(lib.fedavg_last_error())  # this launch's K x grid
    assert 0 < need <= bound and need % K == 0
    assert call(need - 1) == _lib.FEDAVG_EINVAL
    msg = lib.fedavg_last_error()
    assert msg.startswith(entry) and _needed(msg) == need
    _untouched(out, sumsq)
    assert call(need) == 0
    torch.cuda.synchronize()
    assert bool((out == 0.0).all()) and bool((sumsq == 0.0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["f64", "f16", "bf16"])
def test_fused_vec_workspace_one_short_is_refused(gpu, name):
    import torch

    fv = _lib.load_fusedvec()
    dtype = {"f64": torch.float64, "f16": torch.float16, "bf16": torch.bfloat16}[name]
    entry = f"fedavg_reduce_sqdist_{name}".encode()
    fn = getattr(fv, entry.decode())
    K, P, ld = 16, 4097, 4160
    es = torch.empty((), dtype=dtype).element_size()
    x = torch.zeros((K, ld), dtype=dtype, device=gpu)
    w = torch.full((K,), 1.0 / K, dtype=torch.float64 if es == 8 else torch.float32, device=gpu)
    out = torch.full((ld,), SENTINEL, dtype=dtype, device=gpu)
    sumsq = torch.full((K,), SENTINEL, dtype=torch.float64, device=gpu)
    bound = fv.fedavg_reduce_sqdist_vec_workspace(K, P, es)
    ws = torch.empty(bound, dtype=torch.float64, device=gpu)

    def call(elems):
        return fn(x.data_ptr(), K, P, ld, w.data_ptr(), out.data_ptr(), ws.data_ptr(), elems, sumsq.data_ptr(), None)

    assert fv.fedavg_fused_vec_plan_of(K, P, es, int(name == "bf16")) != 0
    assert call(0) == _lib.FEDAVG_EINVAL
    need = _needed(fv.fedavg_fusedvec_last_error())  # this launch's K x waves
    assert 0 < need <= bound and need % K == 0
    assert call(need - 1) == _lib.FEDAVG_EINVAL
    msg = fv.fedavg_fusedvec_last_error()
    assert msg.startswith(entry) and _needed(msg) == need
    _untouched(out, sumsq)
    assert call(need) == 0
    torch.cuda.synchronize()
    assert bool((out[:P] == 0.0).all()) and bool((sumsq == 0.0).all())
