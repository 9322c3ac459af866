"""Each of the nine foreach ops of torch's multi-tensor Adam (amsgrad, coupled
weight decay), alone on the GPU on seeded values, against the candidates of
the exact host reference (tests/client_adam_ref.py): which rounding sequence
does this torch build compute?

    python scripts/probe_adam_ops.py [--out profiles/client_adam/ops_probe.json]

Per dtype and op: the number of elements, and per candidate the number of
elements whose bits differ from torch's (NaN payloads aside).  A candidate at
0 whose rivals are not explains the op; an op with no candidate at 0 computes
something the kernel's form mask has no bit for.  (_foreach_div_ is probed in
both overloads: by a LIST of scalars, which is what adam.py calls and a true
division, and by ONE scalar, which Adam never calls and which multiplies by
the reciprocal.)  Then client_stats.adam_form's
own finding for the dtype (all 16 masks against three whole steps).
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import client_adam_ref as A  # noqa: E402
from mfl_amd import client_stats  # noqa: E402

H = dict(lr=0.001, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.001)
N = {"f32": 1 << 16, "f64": 1 << 16, "bf16": 1 << 20, "f16": 1 << 20}


def values(key):
    dt = A.DTYPES[key]
    rng = np.random.default_rng(20252)
    n = N[key]
    w = torch.from_numpy(rng.normal(0.0, 0.05, n)).to(dt)
    g = torch.from_numpy(rng.normal(0.0, 1.0, n)).to(dt)
    m = torch.from_numpy(rng.normal(0.0, 0.1, n)).to(dt)
    v = torch.from_numpy(rng.normal(0.0, 0.03, n) ** 2).to(dt)
    x = torch.maximum(v, torch.from_numpy(rng.normal(0.0, 0.03, n) ** 2).to(dt))
    s = torch.from_numpy(np.abs(rng.normal(0.0, 0.03, n)) + 1e-4).to(dt)
    return w, g, m, v, x, s


def off(got, want_np, key):
    """Elements of the GPU result whose bits differ from rT(candidate)."""
    want = torch.from_numpy(np.ascontiguousarray(A._rT(key, want_np))).to(A.DTYPES[key])
    got = got.cpu()
    both_nan = torch.isnan(got) & torch.isnan(want)
    return int(((A.bits(got) != A.bits(want)) & ~both_nan).sum())


def probe(key, dev):
    op = A.opmath(key)
    t = 2
    wd, lw, beta2, value, bc2s, eps, step = (op(c) for c in A.coef_of(H["lr"], H["beta1"], H["beta2"], H["eps"],
                                                                      H["wd"], t))
    py = A.coef_of(H["lr"], H["beta1"], H["beta2"], H["eps"], H["wd"], t)
    w, g, m, v, x, s = values(key)
    W, G, M, V, X, S = (A._widen(key, a) for a in (w, g, m, v, x, s))
    d = lambda a: a.to(dev).clone()  # noqa: E731
    out = {}
    with np.errstate(all="ignore"):
        r = torch._foreach_add([d(g)], [d(w)], alpha=py[0])[0]
        out["add_alpha"] = {"apart": off(r, A.axpy(key, 0, wd, W, G), key),
                            "fma": off(r, A.axpy(key, 1, wd, W, G), key)}
        r = d(m)
        torch._foreach_lerp_([r], [d(g)], py[1])
        out["lerp"] = {"apart": off(r, A.axpy(key, 0, lw, G - M, M), key),
                       "fma": off(r, A.axpy(key, 1, lw, G - M, M), key)}
        r = d(v)
        torch._foreach_mul_([r], py[2])
        out["mul"] = {"product": off(r, V * beta2, key)}
        r = d(v)
        torch._foreach_addcmul_([r], [d(g)], [d(g)], py[3])
        out["addcmul"] = {"apart": off(r, A.axpy(key, 0, value, G * G, V), key),
                          "fma": off(r, A.axpy(key, 1, value, G * G, V), key),
                          "scaled_first": off(r, V + (value * G) * G, key)}
        r = d(x)
        torch._foreach_maximum_([r], [d(v * 2)])
        out["maximum"] = {"max": off(r, A.max_nan(X, A._widen(key, v * 2)), key)}
        r = torch._foreach_sqrt([d(x)])[0]
        out["sqrt"] = {"correctly_rounded": off(r, A.sqrt(key, X), key)}
        r = d(s)
        torch._foreach_div_([r], [py[4]])  # a list of scalars, as adam.py passes bias_correction2_sqrt
        out["div_scalarlist"] = {"true_division": off(r, A.divide(key, S, np.full_like(S, bc2s)), key),
                                 "reciprocal_multiply": off(r, S * (op(1) / bc2s), key)}
        r = d(s)
        torch._foreach_div_([r], py[4])    # one scalar: another overload, not the one Adam calls
        out["div_scalar"] = {"true_division": off(r, A.divide(key, S, np.full_like(S, bc2s)), key),
                             "reciprocal_multiply": off(r, S * (op(1) / bc2s), key)}
        r = d(s)
        torch._foreach_add_([r], py[5])
        out["add_scalar"] = {"sum": off(r, S + eps, key)}
        r = d(w)
        torch._foreach_addcdiv_([r], [d(m)], [d(s)], [py[6]])  # a list of scalars, as adam.py passes step_size
        q = A.divide(key, M, S)
        out["addcdiv"] = {"apart": off(r, A.axpy(key, 0, step, q, W), key),
                          "fma": off(r, A.axpy(key, 1, step, q, W), key),
                          "scaled_numerator": off(r, W + A.divide(key, step * M, S), key)}
    torch.cuda.synchronize()
    return {"n": N[key], "ops": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "client_adam" / "ops_probe.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    found = {"torch": torch.__version__, "device": torch.cuda.get_device_name(0), "hyper": H, "dtypes": {}}
    for key, dt in A.DTYPES.items():
        res = probe(key, dev)
        res["adam_form"] = client_stats._probe_adam_form(dev, dt)
        found["dtypes"][key] = res
        print(key, json.dumps(res), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(found, indent=1) + "\n")


if __name__ == "__main__":
    main()
