"""An exact host reference of the fused client Adam step (the definition at the
top of csrc/fedavg_client_adam.hip), in numpy and torch-CPU only, built on
tests/client_step_ref.py's tools:

    A  g1    = rT(g + wd * w)               skipped entirely when wd == 0
    B  m'    = rT(m + lw * (g1 - m))
       v1    = rT(v * beta2)
    C  v'    = rT(v1 + value * (g1 * g1))
       vmax' = max(vmax, v')                (isnan(a) || a > b) ? a : b
       s1    = rT(sqrt(vmax'))
       s2    = rT(s1 / bc2s)
       s3    = rT(s2 + eps)
    E  w'    = rT(w + step * (m' / s3))
       d     = rT(w' - w)
    count of isnan(w'), sum w'^2, sum d^2

Bit i of ``form`` makes site A, B, C, E (i = 0..3) one fma; a clear bit rounds
product and sum apart.  Opmath is fp32 for f32 / bf16 / f16 and fp64 for f64;
every coefficient is rounded once to opmath (coef_of forms them as
torch/optim/adam.py does, in Python floats).

Every operation is the correctly rounded value of its definition:

* a fused site in fp32 opmath: the fp64 product of two fp32 values is exact,
  the fp64 sum is rounded to odd and then once to fp32 (client_step_ref);
  in fp64: client_step_ref.fma64, the error-free fma.
* an unfused site, the difference, the square, v * beta2, s2 + eps: numpy's
  own operation in the opmath type (numpy does not contract).
* quotient and square root of fp32 operands: formed in fp64 and rounded once
  more to fp32.  53 >= 2 * 24 + 2, so the two roundings equal one (Figueroa).
  fp64: numpy's IEEE division and square root.
* rT for a 16-bit type: torch-CPU .to(dtype) of the fp32 value (RNE).

tests/test_client_adam_ref_cpu.py checks all of it against Fraction arithmetic
rounded by integer code."""
import numpy as np
import torch

import client_step_ref as R

DTYPES, bits = R.DTYPES, R.bits
SITES = 4
MASKS = tuple(range(1 << SITES))
COEFS = ("wd", "lw", "beta2", "value", "bc2s", "eps", "step")


def coef_of(lr, beta1, beta2, eps, wd, t):
    """The seven coefficients of step t (from 1) as Python floats, formed as _multi_tensor_adam forms them."""
    t = float(t)
    bias_correction1 = 1 - beta1 ** t
    bias_correction2 = 1 - beta2 ** t
    step_size = (lr / bias_correction1) * -1
    return [float(wd), 1 - beta1, float(beta2), 1 - beta2, bias_correction2 ** 0.5, float(eps), step_size]


def opmath(key):
    return np.float64 if key == "f64" else np.float32


def _widen(key, t):
    """A CPU tensor of DTYPES[key] as an opmath numpy array (exact)."""
    return t.numpy() if key in ("f32", "f64") else t.float().numpy()


def _rT(key, x):
    """An opmath array rounded to the model's type, widened again."""
    if key in ("f32", "f64"):
        return x
    return torch.from_numpy(np.ascontiguousarray(x)).to(DTYPES[key]).float().numpy()


def axpy(key, fused, s, y, x):
    """x + s * y in opmath: one rounding when ``fused``, else two."""
    with np.errstate(all="ignore"):
        if not fused:
            return x + s * y
        if key == "f64":
            return R.fma64(s, y, x)
        return R._exact_sum_to_odd(s, y, x).astype(np.float32)


def divide(key, a, b):
    with np.errstate(all="ignore"):
        if key == "f64":
            return a / b
        return (a.astype(np.float64) / np.float64(b)).astype(np.float32)


def sqrt(key, a):
    with np.errstate(all="ignore"):
        if key == "f64":
            return np.sqrt(a)
        return np.sqrt(a.astype(np.float64)).astype(np.float32)


def max_nan(a, b):
    """ATen's maximum functor: (isnan(a) || a > b) ? a : b."""
    with np.errstate(all="ignore"):
        return np.where(np.isnan(a) | (a > b), a, b)


def step(key, form, coef, w, g, m, v, x):
    """(w', m', v', vmax') as CPU tensors of DTYPES[key] for 1-d CPU tensors of that type."""
    dt, op = DTYPES[key], opmath(key)
    assert all(t.dtype == dt and t.dim() == 1 for t in (w, g, m, v, x)) and form in MASKS
    wd, lw, beta2, value, bc2s, eps, step_size = (op(c) for c in coef)
    w_, g_, m_, v_, x_ = (_widen(key, t) for t in (w, g, m, v, x))
    with np.errstate(all="ignore"):
        g1 = g_ if coef[0] == 0 else _rT(key, axpy(key, form & 1, wd, w_, g_))
        mn = _rT(key, axpy(key, form & 2, lw, g1 - m_, m_))
        v1 = _rT(key, v_ * beta2)
        vn = _rT(key, axpy(key, form & 4, value, g1 * g1, v1))
        xn = max_nan(x_, vn)
        s1 = _rT(key, sqrt(key, xn))
        s2 = _rT(key, divide(key, s1, np.full_like(s1, bc2s)))
        s3 = _rT(key, s2 + eps)
        wn = _rT(key, axpy(key, form & 8, step_size, divide(key, mn, s3), w_))
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dt) for a in (wn, mn, vn, xn))


ONCE_OPS = ("A", "B", "mul", "C", "sqrt", "div", "add", "E")


def _r16(x64):
    """An fp64 array rounded ONCE to fp16 (numpy converts fp64 -> fp16 directly), widened to fp32."""
    with np.errstate(all="ignore"):
        return x64.astype(np.float16).astype(np.float32)


def step_f16_once(coef, w, g, m, v, x, once=ONCE_OPS):
    """fp16 only: the step with every op named in ``once`` rounded a single time, from its exact fp32-operand
    result straight to fp16 (a mixed-precision operation that keeps no fp32 intermediate), and every other op as
    the definition has it under mask 15 (rounded to fp32, then to fp16).  The fma sites: the fp64 product of two
    fp32 values is exact, the fp64 sum is rounded to odd, and numpy rounds fp64 to fp16 once
    (client_step_ref.step_f16_once).  The single operations (v * beta2, sqrt, s1 / bc2s, s2 + eps): formed in fp64,
    where product and sum are exact and quotient and root carry 53 >= 2 * 11 + 2 bits, then rounded to fp16."""
    key = "f16"
    assert all(t.dtype == torch.float16 and t.dim() == 1 for t in (w, g, m, v, x)) and set(once) <= set(ONCE_OPS)
    wd, lw, beta2, value, bc2s, eps, step_size = (np.float32(c) for c in coef)
    w_, g_, m_, v_, x_ = (_widen(key, t) for t in (w, g, m, v, x))

    def fma(name, s, y, a):
        if name in once:
            return _r16(R._exact_sum_to_odd(s, y, a))
        return _rT(key, axpy(key, 1, s, y, a))

    def one(name, exact64, plain32):
        return _r16(exact64()) if name in once else _rT(key, plain32())

    f64 = lambda a: a.astype(np.float64)  # noqa: E731
    with np.errstate(all="ignore"):
        g1 = g_ if coef[0] == 0 else fma("A", wd, w_, g_)
        mn = fma("B", lw, g1 - m_, m_)
        v1 = one("mul", lambda: f64(v_) * np.float64(beta2), lambda: v_ * beta2)
        vn = fma("C", value, g1 * g1, v1)
        xn = max_nan(x_, vn)
        s1 = one("sqrt", lambda: np.sqrt(f64(xn)), lambda: sqrt(key, xn))
        s2 = one("div", lambda: f64(s1) / np.float64(bc2s), lambda: divide(key, s1, np.full_like(s1, bc2s)))
        s3 = one("add", lambda: f64(s2) + np.float64(eps), lambda: s2 + eps)
        wn = fma("E", step_size, divide(key, mn, s3), w_)
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(torch.float16) for a in (wn, mn, vn, xn))


def reference(key, form, coef, first, w, g, m=None, v=None, x=None):
    """((w', m', v', vmax'), record) of one call over the concatenated elements of all keys; ``first``: zero state."""
    if first:
        m = v = x = torch.zeros_like(w)
    out = step(key, form, coef, w, g, m, v, x)
    return out, R.record(key, out[0], w)
