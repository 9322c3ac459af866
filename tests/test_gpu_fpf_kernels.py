"""The FPF2 kernels of csrc/fedavg_fpf.hip through the C ABI on buffers the
test owns, against tests/fpf_kernel_ref.py: float4 tails, the grid caps and
stride loops, poisoned padding, skipped rows, key-table edges, small row
counts, non-finite and subnormal values, the probe library's index variants.

Elementwise results are compared bit for bit (every NaN counts as one value:
a generated NaN's sign and payload differ between x86 and the GPU).  A_mat is
bit-identical because the inputs are drawn so that the mean's rounding to T
is decided (fpf_kernel_ref.mean_is_unambiguous, asserted here and, without a
GPU, in tests/test_fpf_abi.py).  An fp32 index must be one of the pair of
results at the two ends of the fp64 summation bound.  An fp64 index cannot be
held to "one of the pair": the bound is hundreds of fp64 ulps wide, so the two
ends always differ; it must lie between them, and on rows of small integers
(every partial sum exact in any order) it must match bit for bit.
"""
import ctypes

import numpy as np
import pytest
import torch

import fpf_kernel_ref as R
from mfl_amd import _lib

pytestmark = pytest.mark.gpu

NAN = np.float32(np.nan)
PAD_D = R.PAD_D
PAD_A64 = np.uint64(0x7FF8000012345678)  # an fp64 A_mat's padding: a NaN with a payload, compared as bits


@pytest.fixture(scope="module")
def dev(gpu_available):
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def lib(dev):
    return _lib.load()


def _up(arr, dev):
    t = (arr if isinstance(arr, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(arr))).to(dev)
    assert t.data_ptr() % 16 == 0
    return t


def _ptrs(args):
    """Device tensors as addresses; the tensors stay referenced by `args` until the call has run."""
    return [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]


def _call(lib, name, *args):
    rc = getattr(lib, name)(*_ptrs(args), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, name, lib)
    torch.cuda.synchronize()


def _same(got, want, what=""):
    g, w = R.bits(got), R.bits(want)
    assert g.shape == w.shape
    bad = np.argwhere(g != w)
    assert bad.size == 0, f"{what}: {len(bad)} differ, first at {bad[0].tolist()}: " \
                          f"{np.asarray(got)[tuple(bad[0])]!r} != {np.asarray(want)[tuple(bad[0])]!r}"


def _a_padded(a, ld):
    """A_mat [ld] with the payload NaN in the padding columns."""
    out = np.full(ld, NAN, dtype=np.float32)
    out.view(np.uint32)[:] = R.PAD_A
    out[:a.size] = a
    return out


def _a_pad_untouched(got, P):
    assert (np.asarray(got)[P:].view(np.uint32) == R.PAD_A).all()


# ---------------------------------------------------------------------------
# a. set_rows
# ---------------------------------------------------------------------------
# columns 0..5: last_w's value and the row values that rows k = 0, 1, 2 (mod 3) pair with it: -0.0, +-inf, NaN,
# an exact 0 and differences that are fp32 subnormals (no inf - inf: that NaN is generated, not propagated)
SPECIAL_LAST = (0.0, 0.25, 1.0, 1.0, 1.0, 1.4e-38)
SPECIAL_ROW = ((-0.0, 0.0, 1e-45), (0.25, np.inf, -0.25), (np.inf, -np.inf, np.nan), (-np.inf, np.nan, 1.0),
               (np.nan, 1.0 + 2.0 ** -23, np.inf), (1.5e-38, 1.4e-38, -1.4e-38))


@pytest.mark.parametrize("extra", [0, 8])
@pytest.mark.parametrize("P", R.P_EDGE + (R.P_CAPS[1],))
def test_set_rows(lib, dev, P, extra):
    n = R.n_rows_for(P)
    ld = R.round4(P) + extra
    ld_rows = ld + 4 if extra else ld
    rng = np.random.default_rng(R.SEED_BASE + 100 + P % 97)
    last_w = R.padded(rng.normal(0.0, 0.05, P).astype(np.float32), ld, NAN)
    for K in sorted({1, 2, n} & set(range(1, n + 1))):
        for mixed in (False, True):
            valid = rng.permutation(n)[:K].tolist()  # no duplicates within one call
            idx = valid if not mixed else [-1] + valid[:1] + [n] + valid[1:] + [2**40]
            rows = R.padded((last_w[:P] + rng.normal(0.0, 1e-2, (len(idx), P))).astype(np.float32), ld_rows, NAN)
            lw = last_w.copy()
            for c in range(min(P, len(SPECIAL_LAST))):
                lw[c] = SPECIAL_LAST[c]
                for k in range(len(idx)):
                    rows[k, c] = SPECIAL_ROW[c][k % 3]
            d0 = np.full((n, ld), PAD_D, dtype=np.float32)
            want = R.set_rows(d0, idx, rows, lw, P)
            D = _up(d0, dev)
            _call(lib, "fedavg_fpf_set_rows_f32", D, n, ld, _up(np.array(idx, dtype=np.int64), dev),
                  len(idx), _up(rows, dev), ld_rows, _up(lw, dev), P)
            got = D.cpu().numpy()
            _same(got, want, f"P={P} K={K} mixed={mixed}")
            for r in range(n):
                if r in valid:
                    assert (got[r, P:R.round4(P)] == 0).all() and (got[r, R.round4(P):] == PAD_D).all()
                else:
                    assert (got[r] == PAD_D).all()  # rows not named, or named only by skipped entries
            if P >= 6 and not mixed:  # row 0 of the call: 1.5e-38 - 1.4e-38, kept as a subnormal
                sub = np.abs(want[valid[0], :P])
                assert ((sub > 0) & (sub < np.finfo(np.float32).tiny)).any()


# ---------------------------------------------------------------------------
# b. end_round_f32
# ---------------------------------------------------------------------------
# the cap shapes run with ld = P rounded up only (their state is 21 MB)
@pytest.mark.parametrize("P,extra", [(P, 0) for P in R.END_ROUND_P] + [(P, 8) for P in R.P_EDGE])
def test_end_round_f32(lib, dev, P, extra):
    n = R.n_rows_for(P)
    ld = R.round4(P) + extra
    diffs, a, last_w, w_glob = R.state_f32(P, n, R.end_round_seed(P))
    g = R.gdiff_f32(w_glob, last_w)
    assert R.mean_is_unambiguous(torch.float32, g)
    mean = R.mean_as(torch.float32, g)
    nws = lib.fedavg_fpf_workspace(P)
    assert nws == min(-(-(-(-P // 4)) // 256), 1024)
    d0, a0 = R.padded(diffs, ld, PAD_D), _a_padded(a, ld)
    LW, WG = _up(R.padded(last_w, ld, NAN), dev), _up(R.padded(w_glob, ld, NAN), dev)
    ws = torch.full((nws,), float("nan"), dtype=torch.float64, device=dev)
    for form in R.KEEP_FORMS:
        keep = R.keep_form(form, n)
        for g2 in (2.0, 3.0):
            want_d, want_a = R.end_round_f32(d0, keep, a0, w_glob, last_w, P, g2, mean)
            D, A = _up(d0, dev), _up(a0, dev)
            _call(lib, "fedavg_fpf_end_round_f32", D, n, ld, _up(keep, dev), A,
                  WG, LW, P, g2, ws, nws)
            got_a = A.cpu().numpy()
            _same(D.cpu().numpy(), want_d, f"diffs P={P} {form} g2={g2}")
            _same(got_a[:P], want_a[:P], f"A_mat P={P} {form} g2={g2}")
            _a_pad_untouched(got_a, P)


def test_end_round_mean_zero_gives_the_reference_nan_pattern(lib, dev):
    P, n = 1025, 5
    ld = R.round4(P)
    diffs, a, last_w, _ = R.state_f32(P, n, 1500)
    w_glob = last_w.copy()
    keep = R.keep_form("alt", n)
    d0, a0 = R.padded(diffs, ld, PAD_D), _a_padded(a, ld)
    mean = torch.tensor(0.0, dtype=torch.float32)
    want_d, want_a = R.end_round_f32(d0, keep, a0, w_glob, last_w, P, 2.0, mean)
    assert np.isnan(want_a[:P]).all()  # 0 / 2 / 0
    D, A = _up(d0, dev), _up(a0, dev)
    W = _up(R.padded(last_w, ld, NAN), dev)
    ws = torch.zeros(lib.fedavg_fpf_workspace(P), dtype=torch.float64, device=dev)
    _call(lib, "fedavg_fpf_end_round_f32", D, n, ld, _up(keep, dev), A, W,
          W, P, 2.0, ws, ws.numel())
    _same(D.cpu().numpy(), want_d, "diffs")
    _same(A.cpu().numpy()[:P], want_a[:P], "A_mat")
    _a_pad_untouched(A.cpu().numpy(), P)
    out = torch.full((n,), -7.0, dtype=torch.float32, device=dev)
    G = _up(np.full(n, 2.0, dtype=np.float32), dev)
    _call(lib, "fedavg_fpf_index_f32", D, n, ld, P, A, G, out)
    assert (R.bits(out.cpu().numpy()) == 0).all()  # NaN norms scrubbed to +0


# ---------------------------------------------------------------------------
# c. update_g
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1,) + R.N_ROWS_1D)
def test_update_g(lib, dev, n):
    rng = np.random.default_rng(R.SEED_BASE + 200 + n)
    G0 = rng.uniform(0.0, 5.0, n).astype(np.float32)
    itr0 = rng.integers(0, 9, n).astype(np.float32)
    lru0 = rng.integers(0, 40, n).astype(np.float32)
    patterns = {"none": np.zeros(n, np.uint8), "all": np.ones(n, np.uint8), "straddle": np.zeros(n, np.uint8)}
    patterns["straddle"][max(0, min(250, n - 1)):260] = 1  # rows 250..259: both sides of the 256-row block edge
    for record in (0, 1):
        for with_lru in (False, True):
            for name, sel in patterns.items():
                for g1 in (2.0, 3.0):
                    for local_itr in (0.0, 1.0, 7.0):
                        wG, wi, wl = R.update_g(G0, itr0, lru0 if with_lru else None, sel, local_itr, record, g1)
                        G, it, lru = _up(G0, dev), _up(itr0, dev), _up(lru0, dev)
                        _call(lib, "fedavg_fpf_update_g", G, it,
                              lru if with_lru else None, _up(sel, dev), n, local_itr, record, g1)
                        what = f"n={n} record={record} lru={with_lru} {name} g1={g1} itr={local_itr}"
                        _same(G.cpu().numpy(), wG, "G_mat " + what)
                        _same(it.cpu().numpy(), wi, "itr_row " + what)
                        _same(lru.cpu().numpy(), wl if with_lru else lru0, "lru_itr " + what)


# ---------------------------------------------------------------------------
# d. index_f32, index_f64, index_lru
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [0, 8])
@pytest.mark.parametrize("P", R.P_EDGE)
def test_index_f32_and_f64(lib, dev, P, extra):
    n = R.n_rows_for(P)
    ld = R.round4(P) + extra
    diffs, a, G = R.index_state(P, n, R.index_seed(P))
    m = len(G)
    D = _up(R.padded(diffs, ld, NAN), dev)
    Gd = _up(G, dev)
    # fp32
    pair = R.index_f32(diffs, a, G, P)
    assert R.ambiguous_rows(pair).sum() <= 0.01 * m
    out = torch.full((m,), -7.0, dtype=torch.float32, device=dev)
    _call(lib, "fedavg_fpf_index_f32", D, m, ld, P, _up(_a_padded(a, ld), dev), Gd,
          out)
    got = out.cpu().numpy()
    assert R.in_pair(got, pair).all(), np.argwhere(~R.in_pair(got, pair)).ravel()
    assert (got[n + 6] > 0) and got[n + 6] < np.finfo(np.float32).tiny * 64  # the subnormal row is not flushed
    # fp64 A_mat (not fp32-representable), NaN in its padding
    a64 = a.astype(np.float64) * (1.0 + 2.0 ** -30)
    pair64 = R.index_f64(diffs, a64, G, P)
    out64 = torch.full((m,), -7.0, dtype=torch.float64, device=dev)
    _call(lib, "fedavg_fpf_index_f64", D, m, ld, P, _up(R.padded(a64, ld, np.nan), dev),
          Gd, out64)
    got64 = out64.cpu().numpy()
    assert R.between_pair(got64, pair64).all(), np.argwhere(~R.between_pair(got64, pair64)).ravel()
    special = np.arange(n, n + 6)
    special = special[special != n + 2]
    assert (R.bits(got64[special]) == 0).all() and (R.bits(got[special]) == 0).all()


@pytest.mark.parametrize("P", [5, 1025, 8193])
def test_index_on_exactly_summable_rows_is_bit_identical(lib, dev, P):
    """Small integers times powers of two: every product, square and partial
    sum is exact in any order, so both index kernels have one right answer."""
    n, ld = 5, R.round4(P) + 8
    rng = np.random.default_rng(R.SEED_BASE + 300 + P)
    diffs = rng.integers(-8, 9, (n, P)).astype(np.float32)
    a = np.exp2(rng.integers(-1, 2, P)).astype(np.float32)
    G = np.array([1.0, 3.0, -0.75, 7.0, 0.1], dtype=np.float32)
    s = ((diffs.astype(np.float64) * a) ** 2).sum(axis=1)
    want32 = (np.sqrt(s).astype(np.float32) / G).astype(np.float32)
    want64 = np.sqrt(s) / G.astype(np.float64)
    D, Gd = _up(R.padded(diffs, ld, NAN), dev), _up(G, dev)
    out = torch.empty(n, dtype=torch.float32, device=dev)
    _call(lib, "fedavg_fpf_index_f32", D, n, ld, P, _up(_a_padded(a, ld), dev), Gd,
          out)
    _same(out.cpu().numpy(), want32, "fp32 index")
    out64 = torch.empty(n, dtype=torch.float64, device=dev)
    _call(lib, "fedavg_fpf_index_f64", D, n, ld, P,
          _up(R.padded(a.astype(np.float64), ld, np.nan), dev), Gd, out64)
    _same(out64.cpu().numpy(), want64, "fp64 index")


@pytest.mark.parametrize("n", (1,) + R.N_ROWS_1D)
def test_index_lru(lib, dev, n):
    rng = np.random.default_rng(R.SEED_BASE + 400 + n)
    lru = rng.integers(0, 40, n).astype(np.float32)
    G = rng.uniform(0.1, 5.0, n).astype(np.float32)
    for j, (l, g) in enumerate([(0.0, 0.0), (3.0, 0.0), (5.0, np.nan), (np.nan, 2.0), (7.0, -2.0), (np.inf, 1.0),
                                (1e-30, 1e30)]):
        lru[(n - 1 - j) % n], G[(n - 1 - j) % n] = l, g  # from the last row back: the tail of the last block
    out = torch.full((n,), -7.0, dtype=torch.float32, device=dev)
    _call(lib, "fedavg_fpf_index_lru", _up(lru, dev), _up(G, dev), n, out)
    _same(out.cpu().numpy(), R.index_lru(lru, G), f"n={n}")


# ---------------------------------------------------------------------------
# e. cat_diff
# ---------------------------------------------------------------------------
NUMEL_CYCLE = (1, 3, 4, 5, 63, 64, 65, 257)
KEY_TABLES = {
    "one": [37],
    "empty_first": [0, 5, 7],
    "empty_middle": [5, 0, 7],
    "empty_last": [5, 7, 0],
    "empty_pair": [5, 0, 0, 7],
    "forty": [NUMEL_CYCLE[(3 * j) % 8] for j in range(40)],
    "big": [131_072 + 257],
}
# per key, cycled: (group kind, rnd); rnd 2 / 3 marks an integer key held as fp32
DTYPE_GROUPS = {
    "f32": [(0, 0)], "f64": [(1, 0)], "f16": [(2, 0)], "bf16": [(3, 0)],
    "f32_f64": [(0, 0), (1, 0)], "f32_f16": [(0, 0), (2, 0)], "f16_bf16": [(2, 0), (3, 0)],
    "f16_int": [(2, 0), (0, 2), (2, 0)], "bf16_int": [(3, 0), (0, 3)],
}


def _model(numels, kinds):
    """Key table and group order for keys of `numels` with (kind, rnd) cycled from `kinds`."""
    order = []
    for kind, _ in kinds:
        if kind not in order:
            order.append(kind)
    keys, goff, cat = [], {k: 0 for k in order}, 0
    for j, numel in enumerate(numels):
        kind, rnd = kinds[j % len(kinds)]
        keys.append((numel, cat, order.index(kind), goff[kind], rnd))
        cat += numel
        goff[kind] += numel
    return keys, order, goff, cat


def _group_data(kind, size, K, has_int, rng):
    """cur [K, ld_g] and last [ld_g] of the group's dtype, ld_g = size + 5."""
    T = R.KIND_DTYPE[kind]
    ld = size + 5
    last = torch.from_numpy(rng.normal(0.0, 1.0, ld)).to(T)
    cur = (last.to(torch.float64) + torch.from_numpy(rng.normal(0.0, 0.1, (K, ld)))).to(T)
    if kind == 0 and has_int:  # integer keys live here: differences that round in 16 bits (2049 -> 2048, 257 -> 256)
        last = torch.from_numpy(rng.integers(0, 50, ld).astype(np.float32))
        cur = last + torch.from_numpy(rng.choice([2049.0, 257.0, 100003.0, 1.0, 4099.0], (K, ld)).astype(np.float32))
    sp = {0: [(-0.0, 0.0), (np.inf, 1.0), (1.0 + 2.0 ** -12, 2.0 ** -13), (1.5e-38, 1.4e-38)],
          1: [(-0.0, 0.0), (np.inf, 1.0), (1.0 + 2.0 ** -40, 2.0 ** -41), (1e-300, 3e-301)],
          2: [(-0.0, 0.0), (np.inf, 1.0), (6.104e-5, 6.0e-5), (1.0009765625, 0.00048828125)],  # a subnormal fp16 difference
          3: [(-0.0, 0.0), (np.inf, 1.0), (1.5e-38, 1.2e-38), (1.0078125, 0.00390625)]}[kind]  # a subnormal bf16 one
    if not (kind == 0 and has_int):
        for k in range(K):
            for c, (cv, lv) in enumerate(sp):
                if c < size:
                    cur[k, c] = cv
                    last[c] = lv
    return cur.contiguous(), last.contiguous()


# a table of one key has one dtype: it runs with the single kinds only
@pytest.mark.parametrize("table,dtypes", [(t, d) for t in sorted(KEY_TABLES) for d in sorted(DTYPE_GROUPS)
                                          if t not in ("one", "big") or len(DTYPE_GROUPS[d]) == 1])
def test_cat_diff(lib, dev, table, dtypes):
    numels, kinds = KEY_TABLES[table], DTYPE_GROUPS[dtypes]
    if table in ("one", "big"):
        kinds = kinds[:1]
    keys, order, sizes, P = _model(numels, kinds)
    has_int = any(rnd for _, rnd in kinds)
    rng = np.random.default_rng(R.SEED_BASE + 500 + len(numels) * 16 + sorted(DTYPE_GROUPS).index(dtypes))
    n, ld_out = 5, P + 3
    keys_d = _up(np.array(keys, dtype=np.int64), dev)
    for K, idx in ((1, None), (1, [2]), (3, None), (3, [4, -1, 1]), (3, [2**40, 0, n])):
        cur, last = {}, {}
        for g, kind in enumerate(order):
            cur[g], last[g] = _group_data(kind, max(sizes[kind], 1), K, has_int, rng)
        cur_d = {g: t.to(dev) for g, t in cur.items()}
        last_d = {g: t.to(dev) for g, t in last.items()}
        cg, lg = _lib.FpfGroups(), _lib.FpfGroups()
        for g, kind in enumerate(order):
            cg.base[g], cg.ld[g], cg.kind[g] = cur_d[g].data_ptr(), cur[g].shape[1], kind
            lg.base[g], lg.ld[g], lg.kind[g] = last_d[g].data_ptr(), last[g].shape[0], kind
        for out_f64 in (0, 1):
            ref = R.cat_diff(keys, cur, last, K, bool(out_f64))
            np_t = np.float64 if out_f64 else np.float32
            want = np.full((n, ld_out), 123.0, dtype=np_t)
            for k in range(K):
                r = k if idx is None else idx[k]
                if 0 <= r < n:
                    want[r, :P] = ref[k]
            out = _up(np.full((n, ld_out), 123.0, dtype=np_t), dev)
            _call(lib, "fedavg_fpf_cat_diff", keys_d, len(keys), P, ctypes.addressof(cg), K,
                  ctypes.addressof(lg), None if idx is None else _up(np.array(idx, dtype=np.int64), dev), n,
                  out, ld_out, out_f64)
            _same(out.cpu().numpy(), want, f"{table} {dtypes} K={K} idx={idx} f64={out_f64}")


# ---------------------------------------------------------------------------
# f. end_round_promoted
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("t_kind", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("P", R.PROMOTED_P)
def test_end_round_promoted(lib, dev, P, t_kind):
    n = R.n_rows_for(P)
    big = P > 100_000
    ld = R.round4(P) + (0 if big else 8)
    f64 = t_kind in (1, 4)
    gd = R.gdiff_T(P, t_kind, R.promoted_seed(P, t_kind))
    T = torch.float64 if f64 else R.KIND_DTYPE[t_kind]
    if f64:
        assert R.sum_ratio(gd) <= 10.0 and (gd > 0).all()
    else:
        assert R.mean_is_unambiguous(T, gd)
    mean = R.mean_as(T, gd)
    rng = np.random.default_rng(R.SEED_BASE + 600 + P % 89 + t_kind)
    diffs = rng.normal(0.0, 1e-3, (n, P)).astype(np.float32)
    a = rng.uniform(0.5, 1.5, P).astype(np.float32)  # not all ones: t_kind 4's fp32 product shows
    d0 = R.padded(diffs, ld, PAD_D)
    if f64:
        a0 = R.padded(a.astype(np.float64) * ((1.0 + 2.0 ** -30) if t_kind == 1 else 1.0), ld, np.nan)
        a0.view(np.uint64)[P:] = PAD_A64
    else:
        a0 = _a_padded(a, ld)
    GD = _up(R.padded(gd, ld, np.nan), dev)
    nws = lib.fedavg_fpf_workspace(P)
    ws = torch.full((nws,), float("nan"), dtype=torch.float64, device=dev)
    for form in (("alt", "last0") if big else R.KEEP_FORMS):
        keep = R.keep_form(form, n)
        for g2 in (2.0, 3.0):
            want_d, want_a = R.end_round_promoted(d0, keep, a0, gd, P, t_kind, g2, mean)
            D, A = _up(d0, dev), _up(a0, dev)
            _call(lib, "fedavg_fpf_end_round_promoted", D, n, ld, _up(keep, dev), A,
                  GD, P, t_kind, g2, ws, nws)
            what = f"P={P} t_kind={t_kind} {form} g2={g2}"
            _same(D.cpu().numpy(), want_d, "diffs " + what)
            got_a = A.cpu().numpy()
            if f64:
                np.testing.assert_allclose(got_a[:P], want_a[:P], rtol=1e-12, atol=0.0, err_msg="A_mat " + what)
                assert (got_a[P:].view(np.uint64) == PAD_A64).all()
            else:
                _same(got_a[:P], want_a[:P], "A_mat " + what)
                _a_pad_untouched(got_a, P)


# ---------------------------------------------------------------------------
# g. fedavg_fpf_index_variant (probe library)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.VARIANT_SHAPES)
def test_index_variants(dev, shape):
    probe = _lib.load_probe()
    n, P = shape
    ld = R.round4(P) + 8
    diffs, a, G = R.variant_state(n, P)
    assert diffs.shape == (n, P)
    pair = R.index_f32(diffs, a, G, P)
    assert R.ambiguous_rows(pair).sum() <= 0.01 * n
    if n <= len(R.SPECIAL_ROWS):
        assert np.isfinite(pair).all() and (pair != 0).all()  # no row is scrubbed: each shows what was summed
    D, A, Gd = _up(R.padded(diffs, ld, NAN), dev), _up(_a_padded(a, ld), dev), _up(G, dev)
    nws = probe.fedavg_fpf_index_workspace(n, P)
    ws = torch.full((nws,), float("nan"), dtype=torch.float64, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    for unroll, cols in R.VARIANT_PAIRS:
        need = n * -(-R.round4(P) // 4 // (256 * cols)) * 4
        for groups in (0, 1, n):
            out = torch.full((n,), -7.0, dtype=torch.float32, device=dev)
            args = (D, n, ld, P, A, Gd, out, ws)
            _call(probe, "fedavg_fpf_index_variant", *args, need, unroll, cols, groups)
            ok = R.in_pair(out.cpu().numpy(), pair)
            assert ok.all(), (unroll, cols, groups, np.argwhere(~ok).ravel())
        assert probe.fedavg_fpf_index_variant(*_ptrs(args), need - 1, unroll, cols, 1, s) == _lib.FEDAVG_EINVAL
    for unroll, cols in ((5, 1), (8, 8), (16, 2)):
        assert probe.fedavg_fpf_index_variant(*_ptrs(args), nws, unroll, cols, 1, s) == _lib.FEDAVG_EMODE
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# h. three rounds through the C ABI
# ---------------------------------------------------------------------------
def test_three_round_sequence(lib, dev):
    n, P = R.SEQ_ROWS, R.SEQ_P
    ld = R.round4(P) + 8
    d = R.padded(np.zeros((n, P), np.float32), ld, 0.0)
    a = _a_padded(np.ones(P, np.float32), ld)
    G = np.zeros(n, np.float32)
    itr = np.zeros((R.SEQ_ROUNDS, n), np.float32)
    D, A, Gd, It = _up(d, dev), _up(a, dev), _up(G, dev), _up(itr, dev)
    ws = torch.zeros(lib.fedavg_fpf_workspace(P), dtype=torch.float64, device=dev)
    out = torch.full((n,), -7.0, dtype=torch.float32, device=dev)

    def check_index(when):
        _call(lib, "fedavg_fpf_index_f32", D, n, ld, P, A, Gd, out)
        pair = R.index_f32(d, a, G, P)
        ok = R.in_pair(out.cpu().numpy(), pair)
        assert ok.all(), (when, np.argwhere(~ok).ravel())

    for t in range(R.SEQ_ROUNDS):
        last_w, rows, idx, w_glob, local_itr = R.sequence_inputs(t)
        assert R.mean_is_unambiguous(torch.float32, R.gdiff_f32(w_glob, last_w))
        LW, WG = _up(R.padded(last_w, ld, NAN), dev), _up(R.padded(w_glob, ld, NAN), dev)
        _call(lib, "fedavg_fpf_set_rows_f32", D, n, ld, _up(idx, dev), len(idx),
              _up(R.padded(rows, ld, NAN), dev), ld, LW, P)
        d = R.set_rows(d, idx, rows, last_w, P)
        _same(D.cpu().numpy(), d, f"round {t}: set_rows")
        check_index(f"round {t}: after set_rows")
        keep = np.zeros(n, np.uint8)
        keep[idx] = 1
        # the two launches of end_round and the update that follows go out back to back on one stream
        s = torch.cuda.current_stream().cuda_stream
        kd, sd = _up(keep, dev), _up(keep, dev)
        row_t = It[t]
        _lib.check(lib.fedavg_fpf_end_round_f32(*_ptrs((D, n, ld, kd, A, WG, LW, P, 2.0, ws, ws.numel())), s),
                   "fedavg_fpf_end_round_f32", lib)
        _lib.check(lib.fedavg_fpf_update_g(*_ptrs((Gd, row_t, None, sd, n, local_itr, 1, 2.0)), s),
                   "fedavg_fpf_update_g", lib)
        torch.cuda.synchronize()
        d, a = R.end_round_f32(d, keep, a, w_glob, last_w, P, 2.0, R.mean_as(torch.float32, R.gdiff_f32(w_glob, last_w)))
        G, itr[t], _ = R.update_g(G, itr[t], None, keep, local_itr, 1, 2.0)
        _same(D.cpu().numpy(), d, f"round {t}: end_round diffs")
        _same(A.cpu().numpy()[:P], a[:P], f"round {t}: A_mat")
        _a_pad_untouched(A.cpu().numpy(), P)
        _same(Gd.cpu().numpy(), G, f"round {t}: G_mat")
        _same(It.cpu().numpy(), itr, f"round {t}: local_itr_lst")
        check_index(f"round {t}: after end_round")
