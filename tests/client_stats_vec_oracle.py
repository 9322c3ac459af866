"""Oracle of the client statistics (client.py:52-86) for bf16, fp16 and fp64
models, parametrised by dtype (a plain module, not a conftest): the record,
``norm``, the :71 guard, ``Track`` and ``replay`` of tests/client_stats_oracle.py
with the rules of include/fedavg_amd_clientvec.h.

T is the model's dtype.  Rounding to T goes through torch CPU tensors (numpy
has no bf16); fp32 operations are torch CPU fp32 operations (IEEE, rounded
once).  Sums of squares are ``math.fsum`` of fp64 squares: exact squares of
widened 16-bit values, fp64-rounded squares of fp64 values.
"""
from __future__ import annotations

import math

import numpy as np
import torch

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "f64": torch.float64}
MANT_BITS = {torch.bfloat16: 7, torch.float16: 10, torch.float64: 52}
MIN_EXP = {torch.bfloat16: -126, torch.float16: -14, torch.float64: -1022}


def ulp(x: float, dtype) -> float:
    """The spacing of T at |x| (the subnormal spacing below the smallest normal)."""
    if x == 0 or math.isnan(x) or math.isinf(x):
        e = MIN_EXP[dtype]
    else:
        e = max(math.frexp(abs(x))[1] - 1, MIN_EXP[dtype])
    return math.ldexp(1.0, e - MANT_BITS[dtype])


def rT(x, dtype) -> float:
    """rT(fl32(x)): a Python float rounded to fp32, then to T, as ATen casts an opmath result."""
    if dtype == torch.float64:
        return float(x)
    return float(torch.tensor(float(x), dtype=torch.float64).to(torch.float32).to(dtype))


def _f32(x) -> torch.Tensor:
    return torch.tensor(float(x), dtype=torch.float64).to(torch.float32)


def _sumsq(t: torch.Tensor) -> float:
    a = t.detach().reshape(-1).to(torch.float64).numpy()
    if a.size == 0:
        return 0.0
    with np.errstate(all="ignore"):
        sq = a * a
    if not np.all(np.isfinite(sq)):
        with np.errstate(all="ignore"):
            return float(np.sum(sq))  # NaN / inf propagate; no cancellation (all terms >= 0)
    return math.fsum(sq.tolist())


def diff(cur: torch.Tensor, snap: torch.Tensor) -> torch.Tensor:
    """d in the model's type: rT(f32(cur) - f32(snap)) for 16-bit types, cur - snap for fp64."""
    if cur.dtype == torch.float64:
        return cur - snap
    return (cur.to(torch.float32) - snap.to(torch.float32)).to(cur.dtype)


def record(cur: torch.Tensor, snap: torch.Tensor = None):
    """(nan_count, sum cur^2, sum d^2) of flattened CPU tensors of type T; the last is 0 without a snapshot."""
    cur = cur.detach().reshape(-1).cpu()
    nan_count = int(torch.isnan(cur).sum())
    s_cur = _sumsq(cur)
    s_d = 0.0 if snap is None else _sumsq(diff(cur, snap.detach().reshape(-1).cpu()))
    return nan_count, s_cur, s_d


def norm(sumsq: float, dtype) -> float:
    """rT(fl32(sqrt(S))); fp64: sqrt(S)."""
    with np.errstate(all="ignore"):
        return rT(float(np.sqrt(np.float64(sumsq))), dtype)


def update(x, tmp):
    """client.py:79 / :83: ``if not x or tmp > x: x = tmp`` (None = unset)."""
    if x is None or x == 0 or tmp > x:
        return tmp
    return x


class Track:
    def __init__(self, dtype):
        self.dtype = dtype
        self.rho = None
        self.beta = None

    def step(self, sum_dw: float, sum_dg: float, abs_dloss: float):
        dt = self.dtype
        n_w, n_g = norm(sum_dw, dt), norm(sum_dg, dt)
        if dt == torch.float64:
            with np.errstate(all="ignore"):
                recip = np.float64(1.0) / np.float64(n_w)
                rho_tmp = float(recip * np.float64(abs_dloss))
                beta_tmp = float(np.float64(n_g) / np.float64(n_w))
        else:
            # python_float / tensor = tensor.reciprocal() * python_float: each an fp32 operation rounded to T
            recip = (_f32(1.0) / _f32(n_w)).to(dt)
            rho_tmp = float((recip.to(torch.float32) * _f32(abs_dloss)).to(dt))
            beta_tmp = float((_f32(n_g) / _f32(n_w)).to(dt))
        self.rho = update(self.rho, rho_tmp)
        self.beta = update(self.beta, beta_tmp)
        return rho_tmp, beta_tmp


def guard_terms(sum_g: float, sum_last_w: float, lr: float, ratio: float, dtype):
    """(norm(g), bound) of client.py:71."""
    n_g, n_w = norm(sum_g, dtype), norm(sum_last_w, dtype)
    if dtype == torch.float64:
        with np.errstate(all="ignore"):
            return n_g, float(np.float64(n_w) * np.float64(lr * ratio))
    return n_g, float((_f32(n_w) * _f32(lr * ratio)).to(dtype))


def guard(nan_count: int, sum_g: float, sum_last_w: float, loss: float, lr: float, ratio: float, dtype) -> bool:
    n_g, bound = guard_terms(sum_g, sum_last_w, lr, ratio, dtype)
    return bool(nan_count > 0 or math.isnan(loss) or n_g > bound)


def replay(w, g, loss, lr, ratio, dtype, margins=None):
    """w[0], g[0], loss[0]: the prologue; then per iteration t >= 1 the
    gradients g[t], the loss and, unless the guard trips, the weights w[t]
    (CPU tensors of type T).  Returns (tripped_at or None, beta, rho).
    ``margins`` collects, per guard evaluation that neither a NaN count nor a
    NaN loss decides, |norm(g) - bound| in ulps of T at the larger of the two."""
    track = Track(dtype)
    for t in range(1, len(g)):
        nan_g, sum_g, sum_dg = record(g[t], g[t - 1])
        _, sum_last_w, _ = record(w[t - 1])
        if margins is not None and nan_g == 0 and not math.isnan(float(loss[t])):
            n_g, bound = guard_terms(sum_g, sum_last_w, lr, ratio, dtype)
            margins.append(abs(n_g - bound) / ulp(max(abs(n_g), abs(bound)), dtype))
        if guard(nan_g, sum_g, sum_last_w, float(loss[t]), lr, ratio, dtype):
            return t - 1, None, None
        _, _, sum_dw = record(w[t], w[t - 1])
        track.step(sum_dw, sum_dg, abs(float(loss[t]) - float(loss[t - 1])))
    return None, track.beta, track.rho


def same(a, b) -> bool:
    """Equal as values of T held in Python floats (None = unset, NaN equals NaN)."""
    if a is None or b is None:
        return a is None and b is None
    return (math.isnan(a) and math.isnan(b)) or a == b


def within_ulps(a, b, n, dtype) -> bool:
    if a is None or b is None or math.isnan(a) or math.isnan(b) or math.isinf(a) or math.isinf(b):
        return same(a, b)
    return abs(a - b) <= n * ulp(max(abs(a), abs(b)), dtype)


def cast_sequence(case, dtype):
    """The fixture's recorded (w_t, g_t) as CPU tensors of type T."""
    w = [torch.from_numpy(np.array(a)).to(dtype) for a in case["w"]]
    g = [torch.from_numpy(np.array(a)).to(dtype) for a in case["g"]]
    return w, g
