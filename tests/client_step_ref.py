"""An exact host reference of the fused client SGD step (the definition at the
top of csrc/fedavg_client_step.hip), in numpy and torch-CPU only:

    w' = rT(fma(alpha, g, w))          form 1 (one rounding in opmath)
    w' = rT(w + fl(alpha * g))         form 0 (product and sum rounded apart)
    d  = rT(w' - w)                    the difference in the model's type
    count of isnan(w'), sum w'^2, sum d^2

alpha = opmath(-lr); opmath is fp32 for f32 / bf16 / f16 and fp64 for f64.

Every w' is the correctly rounded value of its definition, not "fp64 is
close enough":

* form 1, fp32 opmath: alpha * g is exact in fp64 (48 bits).  The fp64 sum
  with w may round, and rounding that to fp32 would round twice; so the sum
  is rounded to odd (TwoSum gives the sign of what RN dropped), after which
  one rounding to fp32 is the rounding of the exact value (53 >= 24 + 2).
* form 1, fp64: an fma from fp64 operations alone (Python 3.10 has no
  math.fma): Dekker's TwoProduct, TwoSum, and Boldo and Melquiond's
  RN(th + RO(tl + ul)).  The error-free steps need room above underflow and
  below overflow; elements whose operands leave [2^-400, 2^400] (the special
  values) go one by one through fractions.Fraction, whose conversion to
  float is correctly rounded.  Zero and non-finite operands take the plain
  IEEE path, where one of the two roundings is exact.
* form 0: numpy's separate multiply and add in the opmath type (numpy does
  not contract).
* 16-bit types: widened exactly, fp32 -> type by torch-CPU .to(dtype) (RNE).
* step_f16_once: r16(exact(alpha * g + w)), one rounding: the
  sum rounded to odd in fp64, then fp64 -> fp16 by numpy, which rounds once
  (torch-CPU converts through fp32 and would round twice).  With
  fp16 w and g the fp64 sum spans at most 46 bits whenever its low bits can
  reach an fp16 midpoint, so its round-to-odd step never fires; it is kept so
  that the function is exact by construction for any fp32 operands too.

The record's sums are math.fsum over fp64 squares.  The square of an fp32 or
widened 16-bit value is exact in fp64, so those sums are the correctly rounded
exact sums; an fp64 square carries one rounding (2^-53 relative).

tests/test_client_step_ref_cpu.py checks all of it against Fraction arithmetic
rounded by integer code."""
import math
from fractions import Fraction

import numpy as np
import torch

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "f64": torch.float64}
BITS = {2: torch.int16, 4: torch.int32, 8: torch.int64}
_SAFE_LO, _SAFE_HI = 2.0 ** -400, 2.0 ** 400  # fp64 operands the error-free transformations are exact on


def alpha_of(key, lr):
    """opmath(-lr): the scalar rounded once, as the kernel and ATen do."""
    return np.float64(-lr) if key == "f64" else np.float32(-lr)


def bits(t):
    """The bit pattern of a tensor as signed integers of its width."""
    return t.contiguous().view(BITS[t.element_size()])


# ------------------------------------------------------------ fp64 building blocks
def _two_sum(a, b):
    """s = RN(a + b) and e with s + e = a + b exactly (Knuth; finite a, b)."""
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _round_to_odd(s, e):
    """RO(s + e) for s = RN(s + e), |e| <= ulp(s) / 2: s where the sum was
    exact or s is odd, else its neighbour on e's side (which is odd)."""
    s = np.array(s, dtype=np.float64)
    fix = np.isfinite(s) & np.isfinite(e) & (e != 0.0) & ((s.view(np.int64) & 1) == 0)
    if fix.any():
        s[fix] = np.nextafter(s[fix], np.copysign(np.inf, e[fix]))
    return s


def _sum_to_odd(a, b):
    with np.errstate(all="ignore"):
        return _round_to_odd(*_two_sum(a, b))


def _split(a):
    """Veltkamp: a = hi + lo with 26-bit halves."""
    c = 134217729.0 * a  # 2^27 + 1
    hi = c - (c - a)
    return hi, a - hi


def _two_product(a, b):
    """p = RN(a * b) and e with p + e = a * b exactly (Dekker)."""
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _fma64_scalar(a, x, w):
    """fma of finite non-zero fp64 values, exactly (float(Fraction) is correctly rounded; an exact 0 is +0)."""
    exact = Fraction(a) * Fraction(x) + Fraction(w)
    try:
        return float(exact)
    except OverflowError:  # past fp64's range
        return math.inf if exact > 0 else -math.inf


def fma64(alpha, x, w):
    """RN(alpha * x + w) on fp64 arrays, one rounding."""
    a = np.full(x.shape, alpha, dtype=np.float64)
    with np.errstate(all="ignore"):
        out = a * x + w  # exact in one of its two steps when an operand is 0; IEEE's answer when one is not finite
        mag = lambda v: (np.abs(v) >= _SAFE_LO) & (np.abs(v) <= _SAFE_HI)
        plain = ~(np.isfinite(a) & np.isfinite(x) & np.isfinite(w)) | (a == 0.0) | (x == 0.0) | (w == 0.0)
        fast = ~plain & mag(a) & mag(x) & mag(w)
        if fast.any():
            uh, ul = _two_product(a[fast], x[fast])
            th, tl = _two_sum(w[fast], uh)
            out[fast] = th + _sum_to_odd(tl, ul)
        for i in np.flatnonzero(~plain & ~fast):
            out[i] = _fma64_scalar(float(a[i]), float(x[i]), float(w[i]))
    return out


# -------------------------------------------------------------------- the step
def _exact_sum_to_odd(alpha, g32, w32):
    """RO64(alpha * g + w) for fp32 alpha, g, w (fp64 array)."""
    with np.errstate(all="ignore"):
        p = np.float64(alpha) * g32.astype(np.float64)  # 24 x 24 bits, exponents far inside fp64: exact
    return _sum_to_odd(p, w32.astype(np.float64))


def _opmath_step(key, form, alpha, w, g):
    """The step's result in opmath, before the rounding to a 16-bit type (numpy array)."""
    with np.errstate(all="ignore"):
        if key == "f64":
            wn, gn = w.numpy(), g.numpy()
            alpha = np.float64(alpha)
            return fma64(alpha, gn, wn) if form else wn + alpha * gn
        wf, gf = w.float().numpy(), g.float().numpy()
        alpha = np.float32(alpha)
        if form:
            return _exact_sum_to_odd(alpha, gf, wf).astype(np.float32)
        return wf + alpha * gf


def step(key, form, alpha, w, g):
    """w' of form `form` for 1-d CPU tensors w, g of DTYPES[key]; alpha in opmath (alpha_of)."""
    assert w.dtype == g.dtype == DTYPES[key] and w.dim() == g.dim() == 1 and form in (0, 1)
    return torch.from_numpy(_opmath_step(key, form, alpha, w, g)).to(DTYPES[key])


def step_f16_once(alpha, w, g):
    """fp16 only: r16(exact(alpha * g + w)), a single rounding."""
    assert w.dtype == g.dtype == torch.float16
    s = _exact_sum_to_odd(np.float32(alpha), g.float().numpy(), w.float().numpy())
    with np.errstate(all="ignore"):
        return torch.from_numpy(s.astype(np.float16))  # numpy rounds fp64 -> fp16 once; torch-CPU goes through fp32


def difference(key, w_new, w_old):
    """d = rT(w' - w): formed in fp32 from the widened values for a 16-bit type, in the type itself otherwise."""
    with np.errstate(all="ignore"):
        if key in ("f32", "f64"):
            return torch.from_numpy(w_new.numpy() - w_old.numpy())
        return torch.from_numpy(w_new.float().numpy() - w_old.float().numpy()).to(DTYPES[key])


def _sum_sq(t):
    x = t.double().numpy()
    with np.errstate(all="ignore"):
        sq = x * x
    return math.nan if np.isnan(sq).any() else math.fsum(sq)  # squares are >= 0: inf, if any, is +inf


def record(key, w_new, w_old):
    """(NaN count of w', sum w'^2, sum d^2), the sums in fp64."""
    return int(torch.isnan(w_new).sum()), _sum_sq(w_new), _sum_sq(difference(key, w_new, w_old))


def reference(key, form, alpha, w, g):
    """(w', record) of one call over the concatenated elements of all keys."""
    w_new = step(key, form, alpha, w, g)
    return w_new, record(key, w_new, w)
