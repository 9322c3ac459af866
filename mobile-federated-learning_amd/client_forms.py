"""The form probes behind ``client_stats.sgd_form`` / ``adam_form``: which form
of the fused SGD and Adam step kernels leaves torch's own bits on this GPU.
Each runs torch's optimizer and every form of the kernel on the same seeded
values, once per (device, dtype); ``client_stats`` caches what they find."""
from __future__ import annotations

import numpy as np
import torch

from .client_passes import ADAM_SITES, _AdamPass, _StepPass, adam_coef

_BITS = {2: torch.int16, 4: torch.int32, 8: torch.int64}
_PROBE_LR = 0.03
_PROBE_N = 512
_PROBE_POOL = 1 << 21
# The form is a property of torch's compiled kernels, not of the hyperparameters, so the probe picks hyperparameters
# and values at which both terms of every site are of one magnitude (w, g ~ N(0, 1)): there two forms of a site leave
# different fp32 bits on about every third element.  At the reference's own (wd = 0.001 against g ~ 1) they hardly
# ever do.
_ADAM_PROBE = dict(lr=0.3, betas=(0.6, 0.7), eps=1e-8, weight_decay=0.3)
_ADAM_PROBE_STEPS = 3


def _probe_values(dtype):
    """Seeded model-like weights N(0, 0.05^2) and gradients N(0, 1) of type
    ``dtype`` for the probe.  In fp32 and fp64 the two forms differ on about
    every third random element.  In a 16-bit type they differ only where the
    fp32 results lie on either side of a rounding boundary of the type (one
    element in tens of thousands), so the first _PROBE_N values of a larger
    seeded pool are joined by those of its elements at which a host
    computation of the two forms differs; whether they differ on the device
    is sgd_form's own check."""
    wide = dtype in (torch.float32, torch.float64)
    rng = np.random.default_rng(20250)
    n = _PROBE_N if wide else _PROBE_POOL
    w = torch.from_numpy(rng.normal(0.0, 0.05, n)).to(dtype)
    g = torch.from_numpy(rng.normal(0.0, 1.0, n)).to(dtype)
    if wide:
        return w, g
    wf, gf = w.float().numpy(), g.float().numpy()
    alpha = np.float32(-_PROBE_LR)
    with np.errstate(all="ignore"):
        apart = torch.from_numpy(wf + alpha * gf).to(dtype)  # two fp32 roundings, then the type's
        once = torch.from_numpy((wf.astype(np.float64) + np.float64(alpha) * gf.astype(np.float64))
                                .astype(np.float32)).to(dtype)  # the product is exact in fp64
    picked = torch.nonzero(apart.view(torch.int16) != once.view(torch.int16)).view(-1).numpy()[:_PROBE_N]
    idx = torch.from_numpy(np.union1d(np.arange(_PROBE_N), picked))
    return w[idx].clone(), g[idx].clone()


def _probe_sgd_form(device, dtype):
    w, g = _probe_values(dtype)
    bits = _BITS[w.element_size()]
    with torch.cuda.device(device):
        w, g = w.to(device), g.to(device)
        p = torch.nn.Parameter(w.clone())
        p.grad = g.clone()
        torch.optim.SGD([p], lr=_PROBE_LR).step()
        want = p.detach().view(bits)
        step = _StepPass([w.numel()], dtype, device)
        rec = torch.empty(4, dtype=torch.float64, device=device)
        st = torch.cuda.current_stream(device)
        got = []
        for form in (0, 1):
            c = w.clone()
            step.launch(np.array([c.data_ptr()], dtype=np.int64), np.array([g.data_ptr()], dtype=np.int64),
                        _PROBE_LR, form, rec.data_ptr(), st)
            got.append(c.view(bits))
        differ = int((got[0] != got[1]).sum())
        match = tuple(bool(torch.equal(c, want)) for c in got)
    form = None
    if differ:  # equal outputs would say nothing about which one torch computes
        form = 0 if match[0] else 1 if match[1] else None
    return {"form": form, "differ": differ, "match": match, "n": int(w.numel())}


def _adam_probe_values(dtype):
    """Seeded weights and gradients N(0, 1), the pool of 2^21: in a 16-bit
    type the two forms of site A, B or E leave different bits on tens to
    hundreds of its elements."""
    rng = np.random.default_rng(20251)
    return (torch.from_numpy(rng.normal(0.0, 1.0, _PROBE_POOL)).to(dtype),
            torch.from_numpy(rng.normal(0.0, 1.0, _PROBE_POOL)).to(dtype))


def _mine_site_c(dtype, most=64):
    """``(beta2, g, v)`` for a 16-bit ``dtype`` on which site C's two forms,
    ``v' = rT(v1 + value * g^2)`` with ``v1 = rT(v * beta2)`` and ``value = 1
    - beta2``, store different bits: a Python float, one gradient value and up
    to ``most`` second moments.

    Random values never reach this site in a 16-bit type.  Both terms are
    non-negative and ``v1`` is a value of the type, so the forms part only
    when ``fl32(value * g^2)`` is inexact and lies half an fp32 ulp of the
    sum from a rounding boundary of the type: its low 24 - p bits are all
    ones with the exact product below it, or 0...01 with it above (p the
    type's precision).  That is a property of ``(value, g)`` alone, one pair
    in 2^(25 - p); a seeded search over ``value`` in (0.2, 0.4) and ``g ~ N(0,
    1)`` finds such pairs, and for one of them every ``v`` of the type in
    [2^-6, 16) is tried.  The forms are computed here in fp64 (the product
    exact, the sum rounded once more): a filter, as in ``_probe_values``;
    whether they differ on the device is adam_form's own check."""
    prec = {torch.float16: 11, torch.bfloat16: 8}[dtype]
    rng = np.random.default_rng(20253)
    n = 1 << 21
    value = rng.uniform(0.2, 0.4, n).astype(np.float32)
    g = torch.from_numpy(rng.normal(0.0, 1.0, n)).to(dtype).float().numpy()
    exact = value.astype(np.float64) * (g * g).astype(np.float64)  # g * g is exact in fp32 for a 16-bit g
    with np.errstate(all="ignore"):
        c = exact.astype(np.float32)
    low = c.view(np.uint32) & np.uint32((1 << (24 - prec)) - 1)
    cand = np.flatnonzero(((low == (1 << (24 - prec)) - 1) & (exact < c)) | ((low == 1) & (exact > c)))
    every = torch.arange(0, 1 << 15, dtype=torch.int16).view(dtype).float().numpy()
    every = every[(every >= 2.0 ** -6) & (every < 16.0)]
    to_type = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dtype).float().numpy()  # noqa: E731
    for i in cand:
        beta2 = 1.0 - float(value[i])
        if np.float32(1.0 - beta2) != value[i]:
            continue
        with np.errstate(all="ignore"):
            v1 = to_type(every * np.float32(beta2))
            apart = to_type(v1 + c[i])
            once = to_type((v1.astype(np.float64) + exact[i]).astype(np.float32))
        hit = np.flatnonzero(apart != once)[:most]
        if len(hit):
            return beta2, torch.tensor(float(g[i]), dtype=dtype), torch.from_numpy(every[hit]).to(dtype)
    raise RuntimeError(f"no pair found for site C in {dtype}")


def _probe_adam_form(device, dtype):
    h = dict(_ADAM_PROBE)
    w, g = _adam_probe_values(dtype)
    mined = None
    if dtype in (torch.float16, torch.bfloat16):
        # the last elements of the probe are site C's: w = 0 (so g1 = g), and before step 2 their v and vmax are
        # set to the mined second moments, in torch's state and in the kernel's alike
        beta2, g_c, v_c = _mine_site_c(dtype)
        h["betas"] = (h["betas"][0], beta2)
        mined = slice(w.numel() - v_c.numel(), w.numel())
        w[mined] = 0.0
    bits = _BITS[w.element_size()]
    n = w.numel()
    with torch.cuda.device(device):
        w, g = w.to(device), g.to(device)
        grads = [torch.roll(g, 7 * t) for t in range(_ADAM_PROBE_STEPS)]  # another gradient every step
        if mined is not None:
            v_c = v_c.to(device)
            grads[1][mined] = g_c.to(device)

        def inject(w_t, v_t, vmax_t):
            w_t[mined] = 0.0
            v_t[mined] = v_c
            vmax_t[mined] = v_c

        p = torch.nn.Parameter(w.clone())
        opt = torch.optim.Adam([p], lr=h["lr"], betas=h["betas"], eps=h["eps"], weight_decay=h["weight_decay"],
                               amsgrad=True)
        want = []
        for t in range(_ADAM_PROBE_STEPS):
            if mined is not None and t == 1:
                with torch.no_grad():
                    inject(p, opt.state[p]["exp_avg_sq"], opt.state[p]["max_exp_avg_sq"])
            p.grad = grads[t].clone()
            opt.step()
            state = opt.state[p]
            want.append([x.detach().view(bits).clone() for x in
                         (p, state["exp_avg"], state["exp_avg_sq"], state["max_exp_avg_sq"])])
        rec = torch.empty(4, dtype=torch.float64, device=device)
        st = torch.cuda.current_stream(device)
        numel, offset = np.array([n], dtype=np.int64), np.zeros(1, dtype=np.int64)
        step = _AdamPass(numel, offset, n, dtype, device)
        off = []
        for form in range(1 << ADAM_SITES):
            c = w.clone()
            differ = torch.zeros((), dtype=torch.int64, device=device)
            for t in range(_ADAM_PROBE_STEPS):
                if mined is not None and t == 1:
                    inject(c, step.plane(1), step.plane(2))
                coef = adam_coef(h["lr"], *h["betas"], h["eps"], h["weight_decay"], t + 1)
                step.launch(np.array([c.data_ptr()], dtype=np.int64), np.array([grads[t].data_ptr()], dtype=np.int64),
                            coef, t == 0, form, rec.data_ptr(), st)
                for a, b in zip([c.view(bits)] + [step.plane(i).view(bits) for i in range(3)], want[t]):
                    differ += (a != b).sum()
            off.append(int(differ))  # the one read per mask
    # two masks that both equal torch equal each other on the whole probe: it cannot tell them apart, and a mask that
    # equals torch differs from every one that does not.  So the answer is the ONE mask at 0, if there is exactly one.
    match = tuple(o == 0 for o in off)
    form = match.index(True) if sum(match) == 1 else None
    return {"form": form, "match": match, "off": tuple(off), "n": int(n), "steps": _ADAM_PROBE_STEPS,
            "mined_site_c": 0 if mined is None else int(v_c.numel()), "betas": h["betas"]}
