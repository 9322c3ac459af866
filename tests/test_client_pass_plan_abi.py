"""The three client libraries plan one pass (csrc/client_pass_plan.hpp): through
their C ABI, the fp32 statistics of libfedavg_amd.so, the bf16 / fp16 / fp64
statistics of libfedavg_amd_clientvec.so and the fused step of
libfedavg_amd_clientstep.so count the same units for the same key list and
reserve the same table bytes.  What stays a library's own stays: the clientvec
library has no fp32 pass, the step library has one.

CPU only: these functions are host arithmetic.
"""
import ctypes

import numpy as np
import pytest

from mfl_amd import _lib

UNIT_BYTES = 16384


@pytest.fixture(scope="module")
def libs():
    return _lib.load(), _lib.load_clientvec(), _lib.load_clientstep()


def key_lists():
    """Random key lists with empty keys, sizes around the unit edges of every element size."""
    rng = np.random.default_rng(20240)
    edges = [UNIT_BYTES // es * m + d for es in (2, 4, 8) for m in (1, 2, 5) for d in (-1, 0, 1)]
    lists = [[0], [0, 0, 0], [1], [0, 5, 0], edges]
    for n_keys in (1, 2, 7, 130, 4100):
        numel = rng.choice(edges + [1, 3, 63, 70_001], size=n_keys)
        numel[rng.random(n_keys) < 0.25] = 0
        lists.append(numel.tolist())
    return lists


def test_the_three_libraries_count_the_same_units(libs):
    product, vec, step = libs
    ptr = ctypes.POINTER(ctypes.c_int64)
    for numel in key_lists():
        arr = np.asarray(numel, dtype=np.int64)
        p, n = arr.ctypes.data_as(ptr), len(numel)
        want = {es: 3 * sum(-(-k // (UNIT_BYTES // es)) for k in numel) for es in (2, 4, 8)}
        assert product.fedavg_client_stats_partials(p, n) == step.fedavg_client_step_partials(p, n, 4) == want[4]
        for es in (2, 8):
            assert (vec.fedavg_client_stats_vec_partials(p, n, es) == step.fedavg_client_step_partials(p, n, es)
                    == want[es])
        assert vec.fedavg_client_stats_vec_partials(p, n, 4) == 0  # no fp32 pass in this library
        assert (product.fedavg_client_stats_workspace(n) == vec.fedavg_client_stats_vec_workspace(n)
                == step.fedavg_client_step_workspace(n) == 32 * n)


def test_each_library_keeps_its_own_element_sizes(libs):
    product, vec, step = libs
    assert vec.fedavg_client_stats_vec_span(4) == 0 and step.fedavg_client_step_span(4) == 4096
    for es in (2, 8):
        assert vec.fedavg_client_stats_vec_span(es) == step.fedavg_client_step_span(es) == UNIT_BYTES // es
    for n in (0, -3):
        assert (product.fedavg_client_stats_workspace(n) == vec.fedavg_client_stats_vec_workspace(n)
                == step.fedavg_client_step_workspace(n) == 0)
