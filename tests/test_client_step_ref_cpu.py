"""tests/client_step_ref.py against rational arithmetic: every element's w', d
and the record's sums recomputed with fractions.Fraction and rounded by the
integer code below (round to nearest even into (precision, emin, emax), with
subnormals, overflow to inf, signed zeros, inf and NaN), on random model-like
values, values mined next to rounding boundaries, cancelling, subnormal and
overflowing values and the special values of the GPU tests; constructed cases
on which rounding an fp64 (or unfused) result a second time gives the wrong
bits; and the counts the GPU tests' claim to tell the two forms apart rests on
(tests/client_step_cases.py)."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import client_step_cases as C
import client_step_ref as R

# precision (with the hidden bit), emin, emax, width
FMT = {"f16": (11, -14, 15, 16), "bf16": (8, -126, 127, 16), "f32": (24, -126, 127, 32), "f64": (53, -1022, 1023, 64)}
OP = {"f16": "f32", "bf16": "f32", "f32": "f32", "f64": "f64"}
NAN = ("nan",)


# A value is NAN, ("inf", sign) or ("num", sign, magnitude as a Fraction >= 0); sign 1 is negative.
def decode(u, fmt):
    p, emin, emax, width = FMT[fmt]
    ebits = width - p
    sign, e, m = u >> (width - 1), (u >> (p - 1)) & ((1 << ebits) - 1), u & ((1 << (p - 1)) - 1)
    if e == (1 << ebits) - 1:
        return NAN if m else ("inf", sign)
    if e == 0:
        return ("num", sign, Fraction(m) * Fraction(2) ** (emin - (p - 1)))
    return ("num", sign, Fraction(m | (1 << (p - 1))) * Fraction(2) ** (e - emax - (p - 1)))


def encode(v, fmt):
    """The bit pattern of a value of the format (NaN: None)."""
    p, emin, emax, width = FMT[fmt]
    ebits = width - p
    if v == NAN:
        return None
    top = v[1] << (width - 1)
    if v[0] == "inf":
        return top | (((1 << ebits) - 1) << (p - 1))
    m = v[2] / Fraction(2) ** (emin - (p - 1))  # in units of the smallest subnormal
    assert m.denominator == 1, "not a value of the format"
    m = m.numerator
    e = 0
    while m >= 1 << p:
        assert m % 2 == 0, "not a value of the format"
        m >>= 1
        e += 1
    if m >= 1 << (p - 1):  # normal: biased exponent e + 1
        assert e + 1 < (1 << ebits) - 1
        return top | ((e + 1) << (p - 1)) | (m - (1 << (p - 1)))
    assert e == 0
    return top | m


def rnd(v, fmt):
    """Round to nearest, ties to even, into the format."""
    if v[0] != "num" or v[2] == 0:
        return v
    p, emin, emax, _ = FMT[fmt]
    x = v[2]
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    assert Fraction(2) ** e <= x < Fraction(2) ** (e + 1)
    quantum = Fraction(2) ** (max(e, emin) - (p - 1))
    scaled = x / quantum
    n = scaled.numerator // scaled.denominator
    rem = scaled - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1):
        n += 1
    out = n * quantum
    return ("inf", v[1]) if out >= Fraction(2) ** (emax + 1) else ("num", v[1], out)


def mul(a, b):
    if a == NAN or b == NAN:
        return NAN
    sign = a[1] ^ b[1]
    if a[0] == "inf" or b[0] == "inf":
        other = b if a[0] == "inf" else a
        return NAN if other[0] == "num" and other[2] == 0 else ("inf", sign)
    return ("num", sign, a[2] * b[2])


def add(a, b):
    if a == NAN or b == NAN:
        return NAN
    if a[0] == "inf" or b[0] == "inf":
        if a[0] == b[0]:
            return a if a[1] == b[1] else NAN
        return a if a[0] == "inf" else b
    total = (-a[2] if a[1] else a[2]) + (-b[2] if b[1] else b[2])
    if total == 0:
        return ("num", a[1] & b[1], Fraction(0))  # -0 only from (-0) + (-0); an exact cancellation is +0
    return ("num", int(total < 0), abs(total))


def neg(a):
    return a if a == NAN else (a[0], a[1] ^ 1, *a[2:])


def oracle_step(key, form, alpha, w, g):
    """form 0 / 1, or "once": r16(exact) for fp16"""
    op = OP[key]
    if form == "once":
        return rnd(add(mul(alpha, g), w), key)
    if form:
        r = rnd(add(mul(alpha, g), w), op)
    else:
        r = rnd(add(rnd(mul(alpha, g), op), w), op)
    return rnd(r, key)


def oracle_diff(key, w_new, w):
    return rnd(rnd(add(w_new, neg(w)), OP[key]), key)


def _unsigned(t):
    width = 8 * t.element_size()
    return [int(v) & ((1 << width) - 1) for v in R.bits(t).tolist()]


def _alpha_value(key, alpha):
    t = torch.tensor([float(alpha)], dtype=R.DTYPES[OP[key]])
    assert float(t[0]) == float(alpha)
    return decode(_unsigned(t)[0], OP[key])


def check_against_oracle(key, form, alpha, w, g, sums=True):
    """R.step / R.step_f16_once, R.difference and R.record on (w, g) against the rational oracle."""
    got = R.step_f16_once(alpha, w, g) if form == "once" else R.step(key, form, alpha, w, g)
    a = _alpha_value(key, alpha)
    wv = [decode(u, key) for u in _unsigned(w)]
    gv = [decode(u, key) for u in _unsigned(g)]
    want = [oracle_step(key, form, a, x, y) for x, y in zip(wv, gv)]
    got_bits, got_nan = _unsigned(got), torch.isnan(got).tolist()
    for i, (v, u, is_nan) in enumerate(zip(want, got_bits, got_nan)):
        assert (v == NAN) == is_nan and (is_nan or encode(v, key) == u), (key, form, i, w[i].item(), g[i].item(), v, u)
    if form == "once":
        return got
    d = R.difference(key, got, w)
    d_bits, d_nan = _unsigned(d), torch.isnan(d).tolist()
    dv = [oracle_diff(key, v, x) for v, x in zip(want, wv)]
    for i, (v, u, is_nan) in enumerate(zip(dv, d_bits, d_nan)):
        assert (v == NAN) == is_nan and (is_nan or encode(v, key) == u), (key, form, "d", i, v, u)
    nans, s_w, s_d = R.record(key, got, w)
    assert nans == sum(v == NAN for v in want)
    if sums and all(v[0] == "num" for v in want + dv):
        for have, vals in ((s_w, want), (s_d, dv)):
            exact = sum(v[2] * v[2] for v in vals)
            if key == "f64":  # each fp64 square is rounded once: 2^-53 relative, or 2^-1075 where it underflows
                slack = exact * Fraction(1, 2 ** 52) + len(vals) * Fraction(1, 2 ** 1074)
                assert abs(Fraction(have) - exact) <= slack, (key, form, have, float(exact))
            else:             # exact squares, fsum: the correctly rounded exact sum
                assert have == float(exact), (key, form, have, float(exact))
    return got


# ------------------------------------------------------------------- the data
def _datasets(key):
    """name -> (lr, w, g): values at which a step's roundings go wrong."""
    dt = R.DTYPES[key]
    fi = torch.finfo(dt)
    rng = np.random.default_rng(77)
    out = {}
    out["model_lr0.03"] = (0.03, *C._normal(5, 1500, dt))
    out["model_lr0.001"] = (0.001, *C._normal(6, 700, dt))
    out["mined"] = (C.LR, *C.mined(key))  # next to a rounding boundary of the type
    g = torch.from_numpy(rng.normal(0.0, 1.0, 400)).to(dt)
    w = (g.double() * 0.03).to(dt)  # w' is the small residual of a cancellation
    out["cancel"] = (0.03, w, g)
    # results around the smallest normal: subnormal operands, products and results
    w = torch.from_numpy(rng.normal(0.0, 1.0, 300) * fi.smallest_normal).to(dt)
    g = torch.from_numpy(rng.normal(0.0, 30.0, 300) * fi.smallest_normal).to(dt)
    out["subnormal"] = (0.03, w, g)
    # results around the largest finite value: some round to inf
    sign = torch.from_numpy(rng.choice([-1.0, 1.0], 300))
    w = (sign * fi.max * torch.from_numpy(rng.uniform(0.9, 1.0, 300))).to(dt)
    g = (-sign * fi.max * torch.from_numpy(rng.uniform(0.0, 1.0, 300))).to(dt)
    out["overflow"] = (0.03 if key != "f16" else 0.08, w, g)
    for nonfinite in (True, False):
        w, g = C.specials(key, nonfinite)
        keep = torch.cat([torch.arange(24), torch.arange(len(w) - 8, len(w))])
        for lr in (0.03, 40.0):
            out[f"specials_{int(nonfinite)}_lr{lr}"] = (lr, w[keep].clone(), g[keep].clone())
    return out


DATASETS = sorted(_datasets("f32"))


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("name", DATASETS)
@pytest.mark.parametrize("key", C.KEYS)
def test_reference_equals_rational_arithmetic(key, name, form):
    lr, w, g = _datasets(key)[name]
    got = check_against_oracle(key, form, R.alpha_of(key, lr), w, g)
    if name == "subnormal":
        tiny = torch.finfo(R.DTYPES[key]).smallest_normal
        assert int(((got.abs() < tiny) & (got != 0)).sum()) >= 16  # subnormal results were met
    if name == "overflow":
        assert 16 <= int(torch.isinf(got).sum()) <= len(got) - 16  # on both sides of the overflow threshold


def test_fp16_single_rounding_equals_rational_arithmetic():
    alpha = R.alpha_of("f16", C.LR)
    for name, (lr, w, g) in _datasets("f16").items():
        check_against_oracle("f16", "once", R.alpha_of("f16", lr), w, g)
    # the pool's elements on which one rounding and form 1's two roundings part
    w, g = C.pool("f16")
    parts = torch.nonzero(R.bits(R.step_f16_once(alpha, w, g)) != R.bits(R.step("f16", 1, alpha, w, g))).view(-1)
    print(f"fp16 pool: one rounding differs from form 1 on {len(parts)} of {len(w)} elements")
    assert len(parts) >= 1
    check_against_oracle("f16", "once", alpha, w[parts[:64]], g[parts[:64]])
    check_against_oracle("f16", 1, alpha, w[parts[:64]], g[parts[:64]])


def test_alpha_is_minus_lr_rounded_once_to_opmath():
    for lr in (0.03, 0.001, 40.0):
        assert R.alpha_of("f64", lr) == -lr and R.alpha_of("f64", lr).dtype == np.float64
        for key in ("f32", "bf16", "f16"):
            a = R.alpha_of(key, lr)
            assert a.dtype == np.float32
            assert encode(rnd(("num", 1, Fraction(lr)), "f32"), "f32") == int(np.array([a]).view(np.uint32)[0])


# ------------------------------------------- where rounding twice is wrong
def _double_rounding_cases(op):
    """alpha = 1 + 2^-a, g = 2^-q (1 - 2^-a), w = 1 + 2^-(q-1), with q the
    precision: alpha g = 2^-q - 2^(-q-2a) lies just under half an ulp of the
    odd w, so the exact sum rounds down to w, while a sum that first loses
    the 2^(-q-2a) lands on the midpoint and then goes up to even.  Both signs,
    three scales."""
    q, a_range, dt = (24, range(15, 24), np.float32) if op == "f32" else (53, range(27, 53), np.float64)
    alpha, w, g = [], [], []
    for a in a_range:
        for sign in (1.0, -1.0):
            for scale in (0, -7, 11):
                alpha.append(dt(1.0 + 2.0 ** -a))
                g.append(sign * 2.0 ** (scale - q) * (1.0 - 2.0 ** -a))
                w.append(sign * 2.0 ** scale * (1.0 + 2.0 ** -(q - 1)))
    wa, ga = np.array(w, dtype=dt), np.array(g, dtype=dt)
    assert wa.astype(np.float64).tolist() == w and ga.astype(np.float64).tolist() == g  # values of the type
    return alpha, wa, ga


@pytest.mark.parametrize("op", ["f32", "f64"])
def test_constructed_double_rounding_cases(op):
    alphas, w, g = _double_rounding_cases(op)
    assert len(w) >= 16
    naive_wrong = 0
    for i, alpha in enumerate(alphas):
        wi, gi = torch.from_numpy(w[i:i + 1].copy()), torch.from_numpy(g[i:i + 1].copy())
        want = encode(oracle_step(op, 1, _alpha_value(op, alpha), decode(_unsigned(wi)[0], op),
                                  decode(_unsigned(gi)[0], op)), op)
        assert want == _unsigned(wi)[0]  # the exact sum rounds back to w
        with np.errstate(all="ignore"):
            if op == "f32":  # the sum rounded to fp64, then to fp32
                naive = (np.float64(alpha) * g[i:i + 1].astype(np.float64) + w[i:i + 1].astype(np.float64)).astype(
                    np.float32)
            else:            # no wider type: the product rounded to fp64, then the sum
                naive = w[i:i + 1] + alpha * g[i:i + 1]
        naive_wrong += _unsigned(torch.from_numpy(naive))[0] != want
        assert _unsigned(R.step(op, 1, alpha, wi, gi))[0] == want, (op, i)
    print(f"{op} opmath: the twice-rounded route is wrong on {naive_wrong} of {len(w)} constructed cases")
    assert naive_wrong == len(w)


# ----------------------------------- what the GPU tests' discrimination rests on
def test_pool_discrimination_counts():
    """The elements of the seeded pool of 2^21 on which the reference's two forms differ."""
    counts = {key: {lr: len(C.pool_differ(key, lr)) for lr in (0.03, 0.001)} for key in C.KEYS}
    print(f"forms differ, of {C.POOL}: {counts}")
    for key in C.KEYS:
        assert counts[key][C.LR] >= C.MIN_DIFFER
        assert len(C.mined(key)[0]) >= C.MIN_DIFFER
    for key in ("f32", "f64"):  # random data alone tells the forms apart
        assert counts[key][0.03] > C.POOL // 8 and counts[key][0.001] > C.POOL // 64
    for key in ("bf16", "f16"):  # ... and does not in a 16-bit type: hence the mining, and lr 0.03
        assert counts[key][0.03] < 256 and counts[key][0.001] < C.MIN_DIFFER


@pytest.mark.parametrize("name", C.CASES)
@pytest.mark.parametrize("key", C.KEYS)
def test_every_case_tells_the_forms_apart(key, name):
    c = C.case(name, key)
    U, P = C.UNIT[key], C.KPER[key]
    n = c.assert_discriminates()
    print(f"{name} {key}: {len(c.numel)} keys, {len(c.w)} elements, {c.units} units, forms differ on {n}")
    if name == "k130":
        assert len(c.numel) > 64 and c.numel[0] == c.numel[9] == c.numel[10] == c.numel[-1] == 0
        assert set(c.numel.tolist()) == {0, 1, P - 1, P, P + 1, 63, U - 1, U, U + 1}
        d = c.differ()
        assert set(c.slice_s[d].tolist()) == {0, 1, 2, 3} and set(c.half[d].tolist()) == {0, 1}
        assert set(c.ragged[d].tolist()) == {0, 1, 2}  # 2: the ragged last slice of a U + 1 key
        assert bool((d & ~c.wvec & ~c.gvec).any())     # a key read and written element by element
    if name == "k4100":
        assert len(c.numel) > 4096 and c.units > 256 and c.units % 256 != 0 and int(c.numel.max()) <= 3
    if name in ("k130", "k4100"):
        assert c.branches() == {(False, False), (False, True), (True, False), (True, True)}
        live = c.numel > 0
        assert set(c.w_off[live].tolist()) == set(range(P)) and set(c.g_off[live].tolist()) == set(range(P))
        for side in ("w", "g"):  # the buffer: keys in order, PAD sentinels or more around each
            end = c.start[side] + c.numel
            assert c.start[side][0] >= C.PAD and c.size[side] - end[-1] >= C.PAD
            assert bool((c.start[side][1:] - end[:-1] >= C.PAD).all())
            assert bool((c.start[side] % P == (c.w_off if side == "w" else c.g_off)).all())
    if name == "long":
        assert c.units > 256 and len(c.numel) == 1 and c.numel[0] == 257 * U + 3
    if name == "one":
        assert c.numel.tolist() == [U + 1]
