"""Plain CPU references for the FPF2 entry points of include/fedavg_amd.h
(csrc/fedavg_fpf.hip) -- TEST INFRASTRUCTURE ONLY, no GPU import.

One function per entry point.  The elementwise parts are the reference's own
torch CPU expressions in the stated dtype (fedavg_trainer.py:210, :316-327,
oracle/fpf_oracle.py), so a result holds the bits ATen gives.  The two
reductions are not restated in fp32: the mean is computed exactly
(``math.fsum``) and rounded the way the kernel and ATen round it, with a test
on the inputs (``mean_is_unambiguous``) that tells whether any fp64 summation
order must land on the same T value; the row norms come as the pair of results
at the two ends of the fp64 summation-order bound.

The second half of the file draws the inputs of tests/test_gpu_fpf_kernels.py
from committed seeds, so that tests/test_fpf_abi.py can check the conditions
on those inputs (unambiguous means, few ambiguous rows, the sum|g| / |sum g|
bound) without a GPU.
"""
from __future__ import annotations

import math

import numpy as np
import torch

F32, F64, F16, BF16 = torch.float32, torch.float64, torch.float16, torch.bfloat16
KIND_DTYPE = {0: F32, 1: F64, 2: F16, 3: BF16}  # fedavg_fpf_groups.kind / t_kind 0..3
KIND_F64_FROM_F32 = 4  # t_kind 4: fp64 T, A_mat still the fp32 tensor (widened)
NAN_POISON = np.float32(np.nan)
PAD_A = 0x7FC12345  # a_mat's padding: a NaN with a payload, compared as bits
PAD_D = np.float32(123.0)  # diffs' padding and unnamed rows


def round4(P: int) -> int:
    return (P + 3) // 4 * 4


def bits(x) -> np.ndarray:
    """The array's bit patterns with every NaN mapped to one value: IEEE 754
    leaves a generated NaN's sign and payload open (x86 gives 0xFFC00000 for
    0/0 and inf - inf, the GPU 0x7FC00000), everything else is compared bit
    for bit (-0.0 != 0.0, subnormals kept)."""
    if isinstance(x, torch.Tensor):  # numpy has no bf16: take the bits in torch
        x = x.detach().contiguous()
        nan = torch.isnan(x).numpy()
        u = x.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[x.element_size()]).numpy().copy()
        u = u.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[u.dtype.itemsize])
    else:
        a = np.ascontiguousarray(x)
        nan = np.isnan(a)
        u = a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]).copy()
    u[nan] = np.iinfo(u.dtype).max
    return u


# ---------------------------------------------------------------------------
# the mean (:319)
# ---------------------------------------------------------------------------
def _f64_list(g):
    if isinstance(g, torch.Tensor):
        g = g.to(F64).numpy()
    return np.asarray(g, dtype=np.float64)


def exact_mean(g) -> float:
    """math.fsum of the values (exact, one rounding) divided by P."""
    v = _f64_list(g)
    return math.fsum(v.tolist()) / v.size


def _round_to(T, m: float) -> torch.Tensor:
    t = torch.tensor(m, dtype=F64)
    if T == F64:
        return t
    t = t.to(F32)  # one rounding; a 16-bit T goes through fp32 like the kernel and ATen's accumulate type
    return t if T == F32 else t.to(T)


def mean_as(T, g) -> torch.Tensor:
    """The mean as a 0-dim tensor of dtype T: fp64 unrounded, fp32 one
    rounding, fp16 / bf16 to fp32 and then to T."""
    return _round_to(T, exact_mean(g))


def sum_ratio(g) -> float:
    """sum|g| / |sum g|: the condition number of the sum."""
    v = _f64_list(g)
    s = math.fsum(v.tolist())
    return math.inf if s == 0.0 else math.fsum(np.abs(v).tolist()) / abs(s)


def mean_is_unambiguous(T, g) -> bool:
    """Whether every value in [m(1-eps), m(1+eps)] rounds to the same T.
    eps = 4 * P * 2^-53 * sum|g| / |sum g| is the error bound of an fp64 sum
    in any fixed order with a factor 4 of slack, plus 2^-23 for a 16-bit T
    (the intermediate fp32 rounding).  Rounding is monotone, so the two ends
    decide."""
    if T == F64:
        raise ValueError("an fp64 mean is not rounded: compare with a tolerance instead")
    v = _f64_list(g)
    ratio = sum_ratio(v)
    if not math.isfinite(ratio):
        return False
    eps = 4.0 * v.size * 2.0 ** -53 * ratio
    if T in (F16, BF16):
        eps += 2.0 ** -23
    m = exact_mean(v)
    lo, hi = _round_to(T, m * (1.0 - eps)), _round_to(T, m * (1.0 + eps))
    return bool(torch.isfinite(lo)) and bits(lo.reshape(1))[0] == bits(hi.reshape(1))[0]


# ---------------------------------------------------------------------------
# elementwise entry points
# ---------------------------------------------------------------------------
def _t(a) -> torch.Tensor:
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))


def set_rows(diffs, row_idx, rows, last_w, P: int) -> np.ndarray:
    """fedavg_fpf_set_rows_f32: diffs[row_idx[k], :P] = rows[k, :P] - last_w[:P]
    in fp32; the 16-B tail [P, round4(P)) of a written row becomes 0;
    out-of-range entries are skipped; everything else is left as it was."""
    out = np.array(diffs, dtype=np.float32, copy=True)
    lw = _t(last_w)[:P]
    for k, r in enumerate(row_idx):
        r = int(r)
        if 0 <= r < out.shape[0]:
            out[r, :P] = (_t(rows)[k, :P] - lw).numpy()
            out[r, P:round4(P)] = 0.0
    return out


def end_round_f32(diffs, keep_rows, a_mat, w_glob, last_w, P: int, g2, mean):
    """fedavg_fpf_end_round_f32 with `mean` a 0-dim fp32 tensor: returns
    (diffs, a_mat); padding columns are left alone."""
    g = _t(w_glob)[:P] - _t(last_w)[:P]
    d = np.array(diffs, dtype=np.float32, copy=True)
    for r in range(d.shape[0]):
        if not keep_rows[r]:
            d[r, :P] = (_t(d[r, :P].copy()) - g).numpy()
    a = np.array(a_mat, dtype=np.float32, copy=True)
    a[:P] = (_t(a[:P].copy()) * (1 - 1 / g2) + g / g2 / mean).numpy()
    return d, a


def end_round_promoted(diffs, keep_rows, a_mat, gdiff, P: int, t_kind: int, g2, mean):
    """fedavg_fpf_end_round_promoted.  gdiff: fp64 array of T values; a_mat:
    fp32 (t_kind 0, 2, 3) or fp64 (1, 4); mean: 0-dim tensor of dtype T.
    Rows: (row_f32 - gdiff_T).to(float32); A_mat: A * (1 - 1/g2) + gdiff / g2
    / mean in T's arithmetic, for t_kind 4 with the first product in fp32."""
    T = F64 if t_kind == KIND_F64_FROM_F32 else KIND_DTYPE[t_kind]
    g = _t(np.asarray(gdiff, dtype=np.float64)[:P].copy()).to(T)
    assert mean.dtype == T and mean.dim() == 0
    d = np.array(diffs, dtype=np.float32, copy=True)
    for r in range(d.shape[0]):
        if not keep_rows[r]:
            d[r, :P] = (_t(d[r, :P].copy()) - g).to(F32).numpy()
    a = np.array(a_mat, copy=True)
    A = _t(a[:P].copy())
    term = g / g2 / mean
    if t_kind == KIND_F64_FROM_F32:
        assert A.dtype == F64
        new = A.to(F32) * (1 - 1 / g2) + term  # fp32 product, widened by the sum
    else:
        assert A.dtype == (F64 if t_kind == 1 else F32)
        new = A * (1 - 1 / g2) + term
    assert new.dtype == A.dtype
    a[:P] = new.numpy()
    return d, a


def update_g(g_mat, itr_row, lru_itr, selected, local_itr, record, g1):
    """fedavg_fpf_update_g in fp32: returns (G_mat, itr_row, lru_itr or None)."""
    G, it = _t(np.array(g_mat, dtype=np.float32)), _t(np.array(itr_row, dtype=np.float32))
    lru = None if lru_itr is None else _t(np.array(lru_itr, dtype=np.float32))
    sel = _t(np.asarray(selected).astype(bool))
    if record:
        it[sel] = float(local_itr)
        if lru is not None:
            lru += float(local_itr)
            lru[sel] = 0
    G = G * (1 - 1 / g1) + it / g1
    return G.numpy(), it.numpy(), None if lru is None else lru.numpy()


def index_lru(lru_itr, g_mat) -> np.ndarray:
    """fedavg_fpf_index_lru: lru / G in fp32, NaN/inf -> 0."""
    f = (_t(np.array(lru_itr, dtype=np.float32)) / _t(np.array(g_mat, dtype=np.float32))).numpy()
    f[~np.isfinite(f)] = 0
    return f


def cat_diff(keys, cur, last, K: int, out_f64: bool) -> np.ndarray:
    """fedavg_fpf_cat_diff for rows 0..K-1 of `cur`: [K, P] fp32 or fp64.
    keys: rows of (numel, cat_off, grp, grp_off, rnd); cur[g]: [K, ld_g] torch
    tensor of the group's dtype, last[g]: [ld_g].  Each key's difference is
    formed in the key's dtype, an integer key's (rnd 2 / 3) is cast to the
    16-bit T, torch.cat promotes, and the row is stored as fp32 or fp64."""
    rows = []
    for k in range(K):
        pieces = []
        for numel, _off, grp, goff, rnd in keys:
            d = cur[grp][k, goff:goff + numel] - last[grp][goff:goff + numel]
            pieces.append(d.to(KIND_DTYPE[rnd]) if rnd else d)
        rows.append(torch.cat(pieces).to(F64 if out_f64 else F32))
    return torch.stack(rows).numpy()


# ---------------------------------------------------------------------------
# the row norms (:272)
# ---------------------------------------------------------------------------
def _exact_square_terms(q: np.ndarray) -> np.ndarray:
    """fp64 terms whose exact sum is sum(q^2): Veltkamp's split q = h + l into
    26-bit halves, q^2 = h^2 + 2hl + l^2 with every product exact."""
    c = 134217729.0 * q
    h = c - (c - q)
    l = q - h
    return np.concatenate([h * h, 2.0 * h * l, l * l])


def _sumsq(q: np.ndarray) -> float:
    q = np.asarray(q, dtype=np.float64)
    if not np.isfinite(q).all():
        return math.nan if np.isnan(q).any() else math.inf
    terms = q * q if (q == q.astype(np.float32)).all() else _exact_square_terms(q)  # fp32 squares are exact
    return math.fsum(terms.tolist())


def _finish32(s: float, G) -> np.float32:
    with np.errstate(all="ignore"):
        f = np.float32(np.sqrt(np.float64(s))) / np.float32(G)
    return f if np.isfinite(f) else np.float32(0)


def _finish64(s: float, G) -> np.float64:
    with np.errstate(all="ignore"):
        f = np.sqrt(np.float64(s)) / np.float64(np.float32(G))
    return f if np.isfinite(f) else np.float64(0)


def _pairs(sums, g_mat, P, finish, dtype):
    eps = (P + 8) * 2.0 ** -53  # any fp64 summation order of P non-negative terms stays within this
    out = np.zeros((len(sums), 2), dtype=dtype)
    for r, s in enumerate(sums):
        out[r] = finish(s * (1.0 - eps), g_mat[r]), finish(s * (1.0 + eps), g_mat[r])
    return out


def index_f32(diffs, a_mat, g_mat, P: int) -> np.ndarray:
    """fedavg_fpf_index_f32: [n_rows, 2] fp32, the results at both ends of
    the summation bound; s = fsum of the exact squares of fl32(d * a);
    f = fl32(fl32(sqrt(s)) / G), non-finite -> 0."""
    a = _t(np.array(a_mat, dtype=np.float32)[:P].copy())
    sums = [_sumsq((_t(np.array(row[:P], dtype=np.float32)) * a).numpy()) for row in diffs]
    return _pairs(sums, g_mat, P, _finish32, np.float32)


def index_f64(diffs, a_mat, g_mat, P: int) -> np.ndarray:
    """fedavg_fpf_index_f64: [n_rows, 2] fp64; s = fsum of the exact squares
    of fl64(d) * a; f = sqrt(s) / fl64(G), non-finite -> 0."""
    a = _t(np.array(a_mat, dtype=np.float64)[:P].copy())
    sums = [_sumsq((_t(np.array(row[:P], dtype=np.float32)).to(F64) * a).numpy()) for row in diffs]
    return _pairs(sums, g_mat, P, _finish64, np.float64)


def ambiguous_rows(pair: np.ndarray) -> np.ndarray:
    return bits(pair[:, 0]) != bits(pair[:, 1])


def in_pair(got: np.ndarray, pair: np.ndarray) -> np.ndarray:
    """Per row: got is one of the pair (bit for bit)."""
    g = bits(np.asarray(got))
    return (g == bits(pair[:, 0])) | (g == bits(pair[:, 1]))


def between_pair(got: np.ndarray, pair: np.ndarray) -> np.ndarray:
    """Per row: got lies in the closed interval the pair spans.  f is monotone
    in s (correctly rounded sqrt and division), so every summation order within
    the bound lands here.  For an fp64 result the two ends always differ (the
    bound is many fp64 ulps wide), so this is the form of the pair test there."""
    lo, hi = np.minimum(pair[:, 0], pair[:, 1]), np.maximum(pair[:, 0], pair[:, 1])
    got = np.asarray(got)
    # equal ends (0 for a scrubbed row): bit for bit, so that -0.0 does not pass for +0.0
    return ((got >= lo) & (got <= hi) & (lo != hi)) | in_pair(got, pair)


# ---------------------------------------------------------------------------
# inputs of tests/test_gpu_fpf_kernels.py, drawn from committed seeds
# ---------------------------------------------------------------------------
P_EDGE = (1, 3, 4, 5, 1023, 1024, 1025, 8191, 8193)
P_CAPS = (131_072 + 257, 262_144 + 5, 524_288 + 1027, 1_048_576 + 4099)
N_ROWS = (1, 3, 4, 5, 9)
N_ROWS_1D = (255, 256, 257)  # update_g / index_lru: around the 256-thread block
KEEP_FORMS = ("all1", "all0", "alt", "last0")
END_ROUND_P = P_EDGE + (P_CAPS[2], P_CAPS[3])  # fpf_end_round_kernel: 512-block cap, 1024 partials, 4 fold trips
PROMOTED_P = P_EDGE + (P_CAPS[0], P_CAPS[3])  # fpf_end_round_promoted_kernel: 512 x 256-column cap
SEED_BASE = 20260  # one stream per (test family, P, variant)


def lds(P: int):
    """The two row strides of the issue: P rounded up to 4, and 8 more."""
    return round4(P), round4(P) + 8


def keep_form(form: str, n: int) -> np.ndarray:
    k = np.ones(n, dtype=np.uint8)
    if form == "all0":
        k[:] = 0
    elif form == "alt":
        k[1::2] = 0
    elif form == "last0":
        k[-1] = 0
    return k


def n_rows_for(P: int) -> int:
    """The cap shapes always use 5 rows; the edge shapes walk N_ROWS."""
    return 5 if P > 100_000 else N_ROWS[P_EDGE.index(P) % len(N_ROWS)]


def padded(values: np.ndarray, ld: int, fill) -> np.ndarray:
    """[.., P] -> [.., ld] with `fill` in the padding columns."""
    out = np.full(values.shape[:-1] + (ld,), fill, dtype=values.dtype)
    out[..., :values.shape[-1]] = values
    return out


def state_f32(P: int, n: int, seed: int):
    """Model-like state: diffs N(0, 1e-3^2) rows, A_mat around 1, last_w
    N(0, 0.05^2) and w_glob = last_w + N(0.03, 0.05^2) (a non-zero mean)."""
    rng = np.random.default_rng(SEED_BASE + seed)
    last_w = rng.normal(0.0, 0.05, P).astype(np.float32)  # drawn first: the same for every n
    w_glob = (last_w + rng.normal(0.03, 0.05, P)).astype(np.float32)
    a = (1.0 + rng.normal(0.0, 0.25, P)).astype(np.float32)
    diffs = rng.normal(0.0, 1e-3, (n, P)).astype(np.float32)
    return diffs, a, last_w, w_glob


def gdiff_f32(w_glob, last_w) -> np.ndarray:
    return (_t(w_glob) - _t(last_w)).numpy()


def end_round_seed(P: int) -> int:
    return 1000 + END_ROUND_P.index(P)


def gdiff_T(P: int, t_kind: int, seed: int) -> np.ndarray:
    """global_w_diff of dtype T as fp64 values: N(0.03, 0.05^2) rounded to T;
    for an fp64 T (t_kind 1, 4) its absolute value plus 1e-3, so that the
    A_mat sum has no cancellation (its check there is a relative tolerance)."""
    T = F64 if t_kind == KIND_F64_FROM_F32 else KIND_DTYPE[t_kind]
    rng = np.random.default_rng(SEED_BASE + seed)
    g = rng.normal(0.03, 0.05, P)
    if T == F64:
        g = np.abs(g) + 1e-3
    return torch.from_numpy(g).to(T).to(F64).numpy()


# draws whose mean sits too close to a rounding boundary of T (mean_is_unambiguous) take the next stream
PROMOTED_RESEED = {(P_CAPS[3], 0): 1}


def promoted_seed(P: int, t_kind: int) -> int:
    return 2000 + 10 * PROMOTED_P.index(P) + t_kind + 500 * PROMOTED_RESEED.get((P, t_kind), 0)


SPECIAL_ROWS = ("g_zero", "g_nan", "g_neg", "row_inf", "row_nan", "row_zero", "row_subnormal")


def index_state(P: int, n: int, seed: int):
    """diffs / A_mat / G_mat for the index kernels: n random rows followed by
    the seven special rows of SPECIAL_ROWS."""
    if n < 0:
        raise ValueError(f"index_state: {n} random rows")
    rng = np.random.default_rng(SEED_BASE + seed)
    m = n + len(SPECIAL_ROWS)
    diffs = rng.normal(0.0, 1e-3, (m, P)).astype(np.float32)
    a = (1.0 + rng.normal(0.0, 0.25, P)).astype(np.float32)
    G = rng.uniform(0.5, 4.0, m).astype(np.float32)
    G[n + 0] = 0.0
    G[n + 1] = np.nan
    G[n + 2] = -1.5
    diffs[n + 3, P // 2] = np.inf
    diffs[n + 4, P - 1] = np.nan
    diffs[n + 5] = 0.0
    diffs[n + 6] = (rng.uniform(1.0, 2.0, P) * 1e-40).astype(np.float32)  # subnormal, and so are the products
    return diffs, a, G


def index_seed(P: int) -> int:
    return 3000 + P_EDGE.index(P)


VARIANT_SHAPES = ((37, 1013), (5, 70_001))


def variant_state(n: int, P: int):
    """diffs / A_mat / G_mat of a variant shape with exactly n rows.  With room
    for them, n - 7 random rows and the seven special rows; a shape with fewer
    rows gets n random rows whose results are all finite and non-zero, the last
    two with a negative G and with subnormal products, so that every row of it
    tells what the kernel summed."""
    seed = 3100 + P % 7
    if n > len(SPECIAL_ROWS):
        return index_state(P, n - len(SPECIAL_ROWS), seed)
    if n < 3:
        raise ValueError("variant_state: at least 3 rows")
    rng = np.random.default_rng(SEED_BASE + seed)
    diffs = rng.normal(0.0, 1e-3, (n, P)).astype(np.float32)
    a = (1.0 + rng.normal(0.0, 0.25, P)).astype(np.float32)
    G = rng.uniform(0.5, 4.0, n).astype(np.float32)
    G[n - 2] = -1.5
    diffs[n - 1] = (rng.uniform(1.0, 2.0, P) * 1e-40).astype(np.float32)
    return diffs, a, G
VARIANT_PAIRS = ((4, 1), (8, 1), (16, 1), (8, 2), (4, 4), (8, 4), (4, 8))

SEQ_ROWS, SEQ_P, SEQ_ROUNDS = 9, 1025, 3


def sequence_inputs(t: int):
    """Round t of the three-round sequence on 9 rows x 1025 columns: last_w,
    the 3 trained clients' rows and indexes, w_glob and local_itr."""
    rng = np.random.default_rng(SEED_BASE + 4000 + t)
    last_w = rng.normal(0.0, 0.05, SEQ_P).astype(np.float32)
    idx = rng.permutation(SEQ_ROWS)[:3].astype(np.int64)
    rows = (last_w + rng.normal(0.0, 1e-2, (3, SEQ_P))).astype(np.float32)
    w_glob = (last_w + rng.normal(0.03, 0.05, SEQ_P)).astype(np.float32)
    return last_w, rows, idx, w_glob, float(t + 2)
