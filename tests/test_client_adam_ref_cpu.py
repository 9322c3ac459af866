"""tests/client_adam_ref.py against rational arithmetic: every operation of
the Adam step (the products, sums, the difference, the quotient, the square
root, the NaN-keeping maximum) is recomputed per element in
fractions.Fraction and rounded to the opmath format and to the model's type
by test_client_step_ref_cpu.py's integer code, for all four dtypes, every
form bit alone, none and all, a first step and a later one, wd = 0, and the
special values.  Then: on the seeded inputs the GPU tests use, toggling each of
the four fusion bits changes a stored element in every dtype.  In fp32 and
fp64 the chained cases show that for all four bits; in bf16 and fp16 they show
it for A, B and E (with pairs mined from a seeded pool), and site C, which no
random value reaches in a 16-bit type, by the later-step launch on
client_adam_cases.site_c()'s pairs that test_gpu_client_adam_ref.py sends as
well."""
import math
from fractions import Fraction

import pytest
import torch

import client_adam_cases as C
import client_adam_ref as A
from test_client_step_ref_cpu import NAN, OP, _unsigned, add, decode, encode, mul, neg, rnd

MASKS = (0, 15, 1, 2, 4, 8)


def div(a, b):
    if a == NAN or b == NAN:
        return NAN
    sign = a[1] ^ b[1]
    if a[0] == "inf":
        return NAN if b[0] == "inf" else ("inf", sign)
    if b[0] == "inf":
        return ("num", sign, Fraction(0))
    if b[2] == 0:
        return NAN if a[2] == 0 else ("inf", sign)
    return ("num", sign, a[2] / b[2])


def sqrt(a):
    """A value that rounds as sqrt(a) does in any format here: the integer root of a * 4^300, plus half a unit when
    it is not exact (sticky), so that it lies strictly on the true root's side of every midpoint."""
    if a == NAN:
        return NAN
    if a[0] == "num" and a[2] == 0:
        return a  # sqrt(-0) = -0
    if a[1]:
        return NAN
    if a[0] == "inf":
        return a
    scaled = a[2] * Fraction(4) ** 1400
    n = scaled.numerator // scaled.denominator
    r = math.isqrt(n)
    exact = r * r == n and scaled.denominator == 1
    return ("num", 0, (Fraction(r) if exact else Fraction(2 * r + 1, 2)) / Fraction(2) ** 1400)


def gt(a, b):
    """a > b of two non-NaN values."""
    val = lambda v: (math.inf if v[0] == "inf" else v[2]) * (-1 if v[1] else 1)  # noqa: E731
    return val(a) > val(b)


def axpy(x, s, y, fused, op):
    return rnd(add(x, mul(s, y)), op) if fused else rnd(add(x, rnd(mul(s, y), op)), op)


def oracle(key, form, coef, has_wd, w, g, m, v, x):
    op = OP[key]
    rT = lambda val: rnd(val, key)  # noqa: E731
    wd, lw, beta2, value, bc2s, eps, step = coef
    g1 = rT(axpy(g, wd, w, form & 1, op)) if has_wd else g
    diff = rnd(add(g1, neg(m)), op)
    mn = rT(axpy(m, lw, diff, form & 2, op))
    v1 = rT(rnd(mul(v, beta2), op))
    vn = rT(axpy(v1, value, rnd(mul(g1, g1), op), form & 4, op))
    xn = x if (x == NAN or (vn != NAN and gt(x, vn))) else vn
    s1 = rT(rnd(sqrt(xn), op))
    s2 = rT(rnd(div(s1, bc2s), op))
    s3 = rT(rnd(add(s2, eps), op))
    wn = rT(axpy(w, step, rnd(div(mn, s3), op), form & 8, op))
    return wn, mn, vn, xn


def _coef_values(key, coef):
    t = torch.tensor(coef, dtype=torch.float64).to(A.DTYPES[OP[key]])
    return [decode(u, OP[key]) for u in _unsigned(t)]


def check(key, form, coef, first, w, g, m, v, x):
    got, _ = A.reference(key, form, coef, first, w, g, m, v, x)
    if first:
        m = v = x = torch.zeros_like(w)
    cv = _coef_values(key, coef)
    cols = [[decode(u, key) for u in _unsigned(t)] for t in (w, g, m, v, x)]
    got_bits = [(_unsigned(t), torch.isnan(t).tolist()) for t in got]
    for i, vals in enumerate(zip(*cols)):
        want = oracle(key, form, cv, coef[0] != 0, *vals)
        for name, wv, (ub, nb) in zip("wmvx", want, got_bits):
            assert (wv == NAN) == nb[i] and (nb[i] or encode(wv, key) == ub[i]), (key, form, first, i, name, wv, ub[i])


def _inputs(key, n=40):
    dt = A.DTYPES[key]
    w, g = C.normal(5, n, dt), C.normal(6, n, dt)
    m, v = C.normal(7, n, dt, 0.3), C.normal(8, n, dt, 0.5) ** 2
    x = torch.maximum(v, C.normal(9, n, dt, 0.5) ** 2)
    tiny = torch.finfo(dt).smallest_normal
    g[0], g[1], g[2] = math.nan, math.inf, -math.inf
    w[3], g[3], m[3], v[3], x[3] = 0.0, 0.0, 0.0, 0.0, 0.0          # s3 = eps, 0 / eps
    w[4], g[4], v[4], x[4] = -0.0, -0.0, 0.0, 0.0
    g[5], w[5], v[5], x[5] = math.sqrt(tiny) / 4, 0.0, tiny / 4, tiny / 4  # subnormal v and vmax
    g[6], w[6] = 6.0e4, 6.0e4
    x[7] = math.nan                                                  # a NaN that stays in vmax
    v[8], x[8] = 4.0, 1.0                                            # vmax below v': replaced
    return w, g, m, v, x


@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("form", MASKS)
@pytest.mark.parametrize("key", C.KEYS)
def test_reference_equals_rational_arithmetic(key, form, first):
    w, g, m, v, x = _inputs(key)
    check(key, form, C.coef(2), first, w, g, m, v, x)
    if form in (0, 15):
        check(key, form, C.coef(3, wd=0.0), first, w, g, m, v, x)
        check(key, form, A.coef_of(0.001, 0.9, 0.999, 1e-8, 0.001, 1), first, w, g, m, v, x)  # the reference's own


def test_mined_pairs_tell_the_fusion_sites_apart_in_a_16_bit_type():
    for key in ("bf16", "f16"):
        w, g0, g1 = C.mined(key)
        base = C._two_steps(key, 0, w, g0, g1)
        for bit in (1, 2, 8):  # site C: the next test
            out = C._two_steps(key, bit, w, g0, g1)
            assert any(not torch.equal(A.bits(a), A.bits(b)) for a, b in zip(base, out)), (key, bit)


@pytest.mark.parametrize("key", ("bf16", "f16"))
def test_site_c_changes_a_stored_element_on_the_mined_later_step(key):
    """The host mining computes the fused form in fp64 (a filter); the exact reference decides here."""
    coef, w, g, m, v, x = C.site_c(key)
    assert len(v) >= 8, key
    apart = A.reference(key, 0, coef, False, w, g, m, v, x)[0]
    once = A.reference(key, 4, coef, False, w, g, m, v, x)[0]
    differ = A.bits(apart[2]) != A.bits(once[2])
    print(key, len(v), int(differ.sum()))
    assert bool(differ.all()), key  # v' on every mined pair
    for form in (0, 4):
        check(key, form, coef, False, w, g, m, v, x)


@pytest.mark.parametrize("key", C.KEYS)
def test_every_fusion_bit_changes_a_stored_element_on_the_gpu_tests_inputs(key):
    c = C.case("edges", key)
    counts = {bit: C.stored_differ(c, 0, bit) for bit in (1, 2, 4, 8)}
    if key in ("bf16", "f16"):  # site C: the chained cases cannot reach it there, the site_c() launch does
        coef, w, g, m, v, x = C.site_c(key)
        counts[4] += int((A.bits(A.reference(key, 0, coef, False, w, g, m, v, x)[0][2]) !=
                          A.bits(A.reference(key, 4, coef, False, w, g, m, v, x)[0][2])).sum())
    print(key, counts)
    assert all(counts[bit] > 0 for bit in (1, 2, 4, 8)), counts
