"""The FPF2 entry points of include/fedavg_amd.h refuse bad arguments before
any launch (CPU only, like test_abi.py), and the inputs that
tests/test_gpu_fpf_kernels.py draws from its committed seeds meet the
conditions its bit-for-bit checks rest on (tests/fpf_kernel_ref.py)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import fpf_kernel_ref as R
from mfl_amd import _lib, build

OK16 = 0x10000  # a 16-B aligned address; nothing is dereferenced before the checks return
OFF = 0x10004  # 4-B aligned only
EINVAL, EALIGN, EMODE = _lib.FEDAVG_EINVAL, _lib.FEDAVG_EALIGN, _lib.FEDAVG_EMODE


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def _refused(lib, name, args, code):
    rc = getattr(lib, name)(*args)
    assert rc == code, (name, args, rc, lib.fedavg_last_error())
    assert lib.fedavg_last_error().startswith(name.encode()), lib.fedavg_last_error()


def _replace(args, **kw):
    out = dict(args)
    out.update(kw)
    return out


# diffs, n_rows, ld, P of the entry points that take the [n_rows, ld] state
STATE_BAD = [
    (dict(n_rows=0), EINVAL), (dict(n_rows=-3), EINVAL), (dict(n_rows=2**31), EINVAL),
    (dict(P=0), EINVAL), (dict(P=-1), EINVAL), (dict(ld=8, P=9), EINVAL), (dict(ld=10, P=9), EINVAL),
    (dict(diffs=None), EINVAL), (dict(diffs=OFF), EALIGN),
]

SET_ROWS = dict(diffs=OK16, n_rows=5, ld=12, row_idx=OK16, K=2, rows=OK16, ld_rows=12, last_w=OK16, P=9, stream=None)
END_ROUND = dict(diffs=OK16, n_rows=5, ld=2048, keep_rows=OK16, a_mat=OK16, w_glob=OK16, last_w=OK16, P=2048, g2=2.0,
                 workspace=OK16, workspace_elems=2, stream=None)
INDEX_F32 = dict(diffs=OK16, n_rows=5, ld=12, P=9, a_mat=OK16, g_mat=OK16, fpf=OK16, stream=None)
INDEX_F64 = dict(INDEX_F32)
PROMOTED = dict(diffs=OK16, n_rows=5, ld=2048, keep_rows=OK16, a_mat=OK16, gdiff=OK16, P=2048, t_kind=0, g2=2.0,
                workspace=OK16, workspace_elems=2, stream=None)
UPDATE_G = dict(g_mat=OK16, itr_row=OK16, lru_itr=None, selected=OK16, n_rows=5, local_itr=1.0, record=1, g1=2.0,
                stream=None)
INDEX_LRU = dict(lru_itr=OK16, g_mat=OK16, n_rows=5, fpf=OK16, stream=None)

STATE_ENTRIES = {"fedavg_fpf_set_rows_f32": SET_ROWS, "fedavg_fpf_end_round_f32": END_ROUND,
                 "fedavg_fpf_index_f32": INDEX_F32, "fedavg_fpf_index_f64": INDEX_F64,
                 "fedavg_fpf_end_round_promoted": PROMOTED}


@pytest.mark.parametrize("name", sorted(STATE_ENTRIES))
@pytest.mark.parametrize("bad,code", STATE_BAD)
def test_state_arguments_refused(lib, name, bad, code):
    _refused(lib, name, list(_replace(STATE_ENTRIES[name], **bad).values()), code)


@pytest.mark.parametrize("bad,code", [
    (dict(K=0), EINVAL), (dict(K=-1), EINVAL), (dict(K=65536), EINVAL),
    (dict(row_idx=None), EINVAL), (dict(rows=None), EINVAL), (dict(last_w=None), EINVAL),
    (dict(ld_rows=8), EINVAL), (dict(ld_rows=14), EINVAL),
    (dict(rows=OFF), EALIGN), (dict(last_w=OFF), EALIGN),
])
def test_set_rows_refusals(lib, bad, code):
    _refused(lib, "fedavg_fpf_set_rows_f32", list(_replace(SET_ROWS, **bad).values()), code)


@pytest.mark.parametrize("bad,code", [
    (dict(keep_rows=None), EINVAL), (dict(a_mat=None), EINVAL), (dict(w_glob=None), EINVAL),
    (dict(last_w=None), EINVAL), (dict(workspace=None), EINVAL),
    (dict(a_mat=OFF), EALIGN), (dict(w_glob=OFF), EALIGN), (dict(last_w=OFF), EALIGN),
    (dict(workspace_elems=1), EINVAL),  # P = 2,048: 512 float4 = 2 blocks of 256
    (dict(g2=0.0), EINVAL), (dict(g2=-0.0), EINVAL), (dict(g2=math.nan), EINVAL),
])
def test_end_round_f32_refusals(lib, bad, code):
    _refused(lib, "fedavg_fpf_end_round_f32", list(_replace(END_ROUND, **bad).values()), code)


@pytest.mark.parametrize("bad,code", [
    (dict(keep_rows=None), EINVAL), (dict(a_mat=None), EINVAL), (dict(gdiff=None), EINVAL),
    (dict(workspace=None), EINVAL), (dict(workspace_elems=1), EINVAL),
    (dict(g2=0.0), EINVAL), (dict(g2=math.nan), EINVAL),
    (dict(t_kind=-1), EINVAL), (dict(t_kind=5), EINVAL),
])
def test_end_round_promoted_refusals(lib, bad, code):
    _refused(lib, "fedavg_fpf_end_round_promoted", list(_replace(PROMOTED, **bad).values()), code)


@pytest.mark.parametrize("bad,code", [
    (dict(n_rows=0), EINVAL), (dict(n_rows=-1), EINVAL),
    (dict(g_mat=None), EINVAL), (dict(itr_row=None), EINVAL), (dict(selected=None), EINVAL),
    (dict(g1=0.0), EINVAL), (dict(g1=math.nan), EINVAL),
])
def test_update_g_refusals(lib, bad, code):
    _refused(lib, "fedavg_fpf_update_g", list(_replace(UPDATE_G, **bad).values()), code)


@pytest.mark.parametrize("name,args", [("fedavg_fpf_index_f32", INDEX_F32), ("fedavg_fpf_index_f64", INDEX_F64)])
@pytest.mark.parametrize("bad", ["a_mat", "g_mat", "fpf"])
def test_index_null_buffers_refused(lib, name, args, bad):
    _refused(lib, name, list(_replace(args, **{bad: None}).values()), EINVAL)


def test_index_f32_misaligned_a_mat(lib):
    _refused(lib, "fedavg_fpf_index_f32", list(_replace(INDEX_F32, a_mat=OFF).values()), EALIGN)


@pytest.mark.parametrize("bad", [dict(n_rows=0), dict(n_rows=-1), dict(lru_itr=None), dict(g_mat=None), dict(fpf=None)])
def test_index_lru_refusals(lib, bad):
    _refused(lib, "fedavg_fpf_index_lru", list(_replace(INDEX_LRU, **bad).values()), EINVAL)


def _groups(kinds):
    g = _lib.FpfGroups()
    for i, k in enumerate(kinds):
        g.base[i], g.ld[i], g.kind[i] = OK16, 16, k
    return g


def _cat_args(cur_g, last_g, **kw):
    a = dict(keys=OK16, n_keys=2, P=9, cur=ctypes.addressof(cur_g), K=3, last=ctypes.addressof(last_g), row_idx=OK16,
             n_rows=5, out=OK16, ld_out=12, out_f64=0, stream=None)
    a.update(kw)
    return list(a.values())


@pytest.mark.parametrize("bad", [
    dict(keys=None), dict(n_keys=0), dict(cur=None), dict(last=None), dict(out=None),
    dict(P=0), dict(ld_out=8), dict(K=0), dict(K=65536), dict(n_rows=0),
    dict(row_idx=None, n_rows=2),  # rows 0..K-1 of a 2-row output
])
def test_cat_diff_refusals(lib, bad):
    cur, last = _groups([0, 1, 2, 3]), _groups([0, 1, 2, 3])
    _refused(lib, "fedavg_fpf_cat_diff", _cat_args(cur, last, **bad), EINVAL)


@pytest.mark.parametrize("cur_kinds,last_kinds", [
    ([0, 1, 2, 3], [0, 1, 3, 2]),  # mismatched
    ([0, 0, 0, 4], [0, 0, 0, 4]), ([-1, 0, 0, 0], [-1, 0, 0, 0]),  # out of range, equal in both
])
def test_cat_diff_refuses_bad_kinds(lib, cur_kinds, last_kinds):
    cur, last = _groups(cur_kinds), _groups(last_kinds)
    _refused(lib, "fedavg_fpf_cat_diff", _cat_args(cur, last), EINVAL)


def test_workspace_sizes(lib):
    assert lib.fedavg_fpf_workspace(0) == 0
    assert lib.fedavg_fpf_workspace(-5) == 0
    for P in (1, 4, 1024, 1025, 262_144, 262_145, 1_048_576 - 1, 1_048_576, 1_048_577, 2**31 + 7, 2**40):
        assert lib.fedavg_fpf_workspace(P) == min(-(-(-(-P // 4)) // 256), 1024), P
    for P in R.P_EDGE + R.P_CAPS:
        assert lib.fedavg_fpf_workspace(P) == min(-(-(-(-P // 4)) // 256), 1024), P


def test_probe_index_variant_refusals(lib):
    probe = _lib.load_probe()
    n, P, ld = 5, 2048, 2048
    need = probe.fedavg_fpf_index_workspace(n, P)
    assert need == n * 2 * 4  # cols = 1: 2 column blocks, one partial per wave
    assert probe.fedavg_fpf_index_workspace(0, P) == 0 and probe.fedavg_fpf_index_workspace(n, 0) == 0
    base = [OK16, n, ld, P, OK16, OK16, OK16, OK16, need]
    for unroll, cols in ((5, 1), (4, 2), (16, 4), (8, 8), (0, 1)):
        assert probe.fedavg_fpf_index_variant(*base, unroll, cols, 1, None) == EMODE, (unroll, cols)
        assert probe.fedavg_last_error().startswith(b"fedavg_fpf_index_variant")
    assert probe.fedavg_fpf_index_variant(*base, 4, 3, 1, None) == EMODE
    for unroll, cols in R.VARIANT_PAIRS:
        short = n * -(-512 // (256 * cols)) * 4 - 1
        assert probe.fedavg_fpf_index_variant(*base[:8], short, unroll, cols, 1, None) == EINVAL, (unroll, cols)
        assert probe.fedavg_last_error().startswith(b"fedavg_fpf_index_variant")


# ---------------------------------------------------------------------------
# conditions on the committed inputs of tests/test_gpu_fpf_kernels.py
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("P", R.END_ROUND_P)
def test_end_round_inputs_have_an_unambiguous_fp32_mean(P):
    _, _, last_w, w_glob = R.state_f32(P, 1, R.end_round_seed(P))
    g = R.gdiff_f32(w_glob, last_w)
    assert R.mean_is_unambiguous(torch.float32, g), (P, R.sum_ratio(g))


@pytest.mark.parametrize("t_kind", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("P", R.PROMOTED_P)
def test_promoted_inputs_meet_their_condition(P, t_kind):
    g = R.gdiff_T(P, t_kind, R.promoted_seed(P, t_kind))
    if t_kind in (1, 4):
        # no rounding step to pin: A_mat is compared at rtol 1e-12.  The kernel's fixed order puts every value
        # through fewer than 64 fp64 additions, so its mean is within 64 * 2^-53 * sum|g| / |sum g| < 1e-13 of the
        # exact one; g > 0 and A_mat > 0 keep the sum A * c2 + g / g2 / mean free of cancellation.
        assert R.sum_ratio(g) <= 10.0 and (g > 0).all()
    else:
        assert R.mean_is_unambiguous(R.KIND_DTYPE[t_kind], g), (P, t_kind, R.sum_ratio(g))


@pytest.mark.parametrize("P", R.P_EDGE)
def test_index_inputs_have_few_ambiguous_rows(P):
    n = R.n_rows_for(P)
    diffs, a, G = R.index_state(P, n, R.index_seed(P))
    pair = R.index_f32(diffs, a, G, P)
    assert R.ambiguous_rows(pair).sum() <= 0.01 * len(G)
    assert (pair[n:n + 2] == 0).all() and (pair[n + 3:n + 6] == 0).all()  # G = 0 / NaN, inf / NaN / zero rows
    assert (pair[n + 2] < 0).all() and (pair[n + 6] > 0).all() and (pair[:n] > 0).all()


@pytest.mark.parametrize("shape", R.VARIANT_SHAPES)
def test_variant_inputs_have_few_ambiguous_rows(shape):
    n, P = shape
    diffs, a, G = R.variant_state(n, P)
    assert diffs.shape == (n, P) and G.shape == (n,)
    pair = R.index_f32(diffs, a, G, P)
    assert R.ambiguous_rows(pair).sum() <= 0.01 * n
    if n <= len(R.SPECIAL_ROWS):  # too few rows for the specials: every row's result tells what was summed
        assert np.isfinite(pair).all() and (pair != 0).all()
        assert (pair[n - 2] < 0).all() and (0 < pair[n - 1]).all() and (pair[n - 1] < 1e-36).all()
    else:
        r = n - len(R.SPECIAL_ROWS)
        assert (pair[:r] > 0).all() and (pair[r + 2] < 0).all() and (pair[r + 6] > 0).all()


def test_index_state_refuses_a_negative_row_count():
    with pytest.raises(ValueError):
        R.index_state(70_001, -2, 0)
    with pytest.raises(ValueError):
        R.variant_state(2, 1013)


def test_helper_mean_and_pair_on_known_values():
    """The helper on values worked out by hand."""
    g = np.array([1.0, 2.0, 4.0], dtype=np.float32)
    assert R.exact_mean(g) == 7.0 / 3.0
    assert R.mean_as(torch.float32, g).item() == np.float32(7.0 / 3.0)
    assert R.mean_as(torch.float16, g).item() == float(np.float16(np.float32(7.0 / 3.0)))
    assert R.mean_is_unambiguous(torch.float32, g) and R.mean_is_unambiguous(torch.bfloat16, g)
    assert not R.mean_is_unambiguous(torch.float32, np.array([1.0, -1.0], dtype=np.float32))  # mean 0
    # a mean that sits on an fp32 rounding boundary: 1 + 2^-24 (a tie)
    tie = np.array([1.0, 1.0 + 2.0 ** -23], dtype=np.float64)
    assert not R.mean_is_unambiguous(torch.float32, tie)
    d = np.array([[3.0, 4.0, 0.0, 9.0]], dtype=np.float32)  # the last column is padding (P = 3)
    pair = R.index_f32(d, np.ones(4, np.float32), np.array([2.0], np.float32), 3)
    assert pair.tolist() == [[2.5, 2.5]] and not R.ambiguous_rows(pair).any()
    pair64 = R.index_f64(d, np.ones(4), np.array([2.0], np.float32), 3)
    assert pair64[0, 0] < 2.5 < pair64[0, 1] and R.between_pair(np.array([2.5]), pair64).all()
    assert not R.between_pair(np.array([2.5000001]), pair64).any()
