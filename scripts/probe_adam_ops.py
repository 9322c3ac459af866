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


def off16(got, want32):
    """Elements of the GPU's fp16 result whose bits differ from an fp32 array of fp16 values."""
    want = torch.from_numpy(np.ascontiguousarray(want32)).to(torch.float16)
    got = got.cpu()
    return int(((A.bits(got) != A.bits(want)) & ~(torch.isnan(got) & torch.isnan(want))).sum())


def probe_fp16_ties(dev, eg):
    """The fp16 ops again, on the values of tests/client_adam_cases.py's chain at gradient scale 2^eg (fp16 w ~
    N(0, 1), g, and the state the host reference leaves after step 1): with the reference's decimal scalars many
    exact results there lie just above an fp16 rounding midpoint.  Per op two candidates: ``twice`` (the
    definition: the op, fused where it has two parts, rounded to fp32 and then to fp16) and ``once`` (the exact
    result rounded straight to fp16)."""
    import client_adam_cases as C

    key, t = "f16", 2
    c = C.chain(key, (eg, 0))
    w, m, v, x = C.chain_reference(key, (eg, 0), "a")[0]
    g = c.g[1]
    py = A.coef_of(H["lr"], H["beta1"], H["beta2"], H["eps"], H["wd"], t)
    wd, lw, beta2, value, bc2s, eps, step = (np.float32(c_) for c_ in py)
    W, G, M, V, X = (A._widen(key, a) for a in (w, g, m, v, x))
    f64 = lambda a: a.astype(np.float64)  # noqa: E731
    once = lambda s, y, a: A._r16(A.R._exact_sum_to_odd(s, y, a))  # noqa: E731
    twice = lambda s, y, a: A._rT(key, A.axpy(key, 1, s, y, a))  # noqa: E731
    d = lambda a: a.to(dev).clone()  # noqa: E731
    out = {}
    with np.errstate(all="ignore"):
        S32 = A._rT(key, A.sqrt(key, X) / bc2s + np.float32(1e-3))  # a denominator fp16 keeps above 0
        s = torch.from_numpy(S32).to(torch.float16)
        r = torch._foreach_add([d(g)], [d(w)], alpha=py[0])[0]
        out["add_alpha"] = {"twice": off16(r, twice(wd, W, G)), "once": off16(r, once(wd, W, G))}
        r = d(m)
        torch._foreach_lerp_([r], [d(g)], py[1])
        out["lerp"] = {"twice": off16(r, twice(lw, G - M, M)), "once": off16(r, once(lw, G - M, M))}
        r = d(v)
        torch._foreach_mul_([r], py[2])
        out["mul"] = {"twice": off16(r, A._rT(key, V * beta2)), "once": off16(r, A._r16(f64(V) * np.float64(beta2)))}
        r = d(v)
        torch._foreach_addcmul_([r], [d(g)], [d(g)], py[3])
        out["addcmul"] = {"twice": off16(r, twice(value, G * G, V)), "once": off16(r, once(value, G * G, V))}
        r = torch._foreach_sqrt([d(x)])[0]
        out["sqrt"] = {"twice": off16(r, A._rT(key, A.sqrt(key, X))), "once": off16(r, A._r16(np.sqrt(f64(X))))}
        r = d(s)
        torch._foreach_div_([r], [py[4]])
        out["div_scalarlist"] = {"twice": off16(r, A._rT(key, A.divide(key, S32, np.full_like(S32, bc2s)))),
                                 "once": off16(r, A._r16(f64(S32) / np.float64(bc2s)))}
        r = d(s)
        torch._foreach_add_([r], py[5])
        out["add_scalar"] = {"twice": off16(r, A._rT(key, S32 + eps)),
                             "once": off16(r, A._r16(f64(S32) + np.float64(eps)))}
        r = d(w)
        torch._foreach_addcdiv_([r], [d(m)], [d(s)], [py[6]])
        q = A.divide(key, M, S32)
        out["addcdiv"] = {"twice": off16(r, twice(step, q, W)), "once": off16(r, once(step, q, W))}
    torch.cuda.synchronize()
    return {"n": int(w.numel()), "scale": f"g ~ 2^{eg} N(0, 1), w ~ N(0, 1)", "ops": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "client_adam" / "ops_probe.json"))
    ap.add_argument("--fp16-ties", metavar="OUT", help="probe only the fp16 ops on the chain values where exact "
                    "results lie next to fp16 rounding midpoints (e.g. profiles/client_adam/ops_probe_fp16_ties.json)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    if args.fp16_ties:
        found = {"torch": torch.__version__, "device": torch.cuda.get_device_name(0), "hyper": H, "scales": {}}
        for eg in (0, -6, -10):
            found["scales"][str(eg)] = probe_fp16_ties(dev, eg)
            print(eg, json.dumps(found["scales"][str(eg)]), flush=True)
        Path(args.fp16_ties).parent.mkdir(parents=True, exist_ok=True)
        Path(args.fp16_ties).write_text(json.dumps(found, indent=1) + "\n")
        return
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
