"""The launches tests/test_gpu_client_adam_ref.py sends through
fedavg_client_adam_step_*, built on the host: keys (sizes in elements), the
offset in elements of each key's weights and gradients from a 16-B boundary,
seeded values, and the host reference's answer over chained steps.

Hyperparameters and values are client_stats._ADAM_PROBE's kind (w, g ~ N(0, 1),
wd = 0.3, betas (0.6, 0.7), lr = 0.3): both terms of every site are of one
magnitude, so in fp32 and fp64 every bit of the form mask changes about a
third of the elements.  Site C in a 16-bit type is reached by no random value:
site_c() gives the pairs mined for it (client_stats._mine_site_c) and the
later-step launch they are sent through.  In a 16-bit type a bit changes a stored element only
where an fp32 result lies at a rounding boundary of the type, so such a case
is joined by mined elements (mined()): pairs of a seeded pool on which the
host reference's answers under the two settings of the bit differ.

The second half builds the chains that tests/test_gpu_client_adam_torch.py
holds against torch.optim.Adam itself: twelve steps at the reference's own
hyperparameters and three other sets, at gradient and weight scales down to
where the second moment is subnormal or underflows, and the conditions those
inputs must meet (tests/test_client_adam_torch_cases_cpu.py)."""
import functools
import math

import numpy as np
import torch

import client_adam_ref as A

DTYPES = A.DTYPES
KEYS = tuple(DTYPES)
UNIT = {"f32": 4096, "bf16": 8192, "f16": 8192, "f64": 2048}  # elements of 16 KiB
KPER = {"f32": 4, "bf16": 8, "f16": 8, "f64": 2}              # elements of 16 B
HYPER = dict(lr=0.3, beta1=0.6, beta2=0.7, eps=1e-8, wd=0.3)
MASKS = (0, 15, 1, 2, 4, 8)  # none, all, each single bit
SENTINEL = 123.0
PAD = 8
POOL = 1 << 20


def coef(t, **change):
    h = {**HYPER, **change}
    return A.coef_of(h["lr"], h["beta1"], h["beta2"], h["eps"], h["wd"], t)


def normal(seed, n, dt, scale=1.0):
    return torch.from_numpy(np.random.default_rng(seed).normal(0.0, scale, n)).to(dt)


def _two_steps(key, form, w, g0, g1):
    """Everything the reference stores over steps 1 and 2 from a zero state."""
    first, _ = A.reference(key, form, coef(1), True, w, g0)
    second, _ = A.reference(key, form, coef(2), False, first[0], g1, *first[1:])
    return first + second


@functools.lru_cache(maxsize=None)
def mined(key, most=16):
    """(w, g of step 1, g of step 2) of the seeded pool on which, for each of the four fusion bits, the reference
    under mask 0 and under that bit alone stores different bits in step 1 or 2 (site C adds to v = 0 in step 1,
    where one rounding and two are the same): `most` elements per bit (fewer if the pool has fewer; none for site
    C in a 16-bit type, which site_c() covers)."""
    dt = DTYPES[key]
    w, g0, g1 = normal(77, POOL, dt), normal(78, POOL, dt), normal(79, POOL, dt)
    base = _two_steps(key, 0, w, g0, g1)
    picked = []
    for bit in (1, 2, 4, 8):
        differ = torch.zeros(POOL, dtype=torch.bool)
        for a, b in zip(base, _two_steps(key, bit, w, g0, g1)):
            differ |= (A.bits(a) != A.bits(b)) & ~(torch.isnan(a) & torch.isnan(b))
        picked.append(torch.nonzero(differ).view(-1)[:most])
    idx = torch.unique(torch.cat(picked))
    return w[idx].clone(), g0[idx].clone(), g1[idx].clone()


@functools.lru_cache(maxsize=None)
def site_c(key):
    """For a 16-bit type: (coef of step 2 at the mined beta2, w = 0, g, m = 0, v, vmax = v) of one later step on
    which site C's two forms store different v' (client_stats._mine_site_c, which explains the construction)."""
    from mfl_amd import client_stats

    beta2, g1, v = client_stats._mine_site_c(DTYPES[key])
    g = torch.full_like(v, float(g1))
    zero = torch.zeros_like(v)
    return coef(2, beta2=beta2), zero, g, zero.clone(), v, v.clone()


def sizes(name, key):
    U, P = UNIT[key], KPER[key]
    if name == "edges":
        return [1, U - 1, U, U + 1, 2 * U + 3]
    if name == "k130":
        cycle = [0, 1, P - 1, P, P + 1, 63, 2 * P + 1]
        n = [cycle[j % 7] for j in range(130)]
        n[129] = 0
        return n
    if name == "long":
        return [257 * U + 3]
    if name == "chain":
        return [1, 3, P - 1, P, P + 1, 63, U - 1, U + 1, 2 * U + 3]
    raise KeyError(name)


class Case:
    """Keys in one buffer per side (w, g), PAD or more sentinels around each; the state planes are laid out as
    ClientStepStats lays them out: every key at the next multiple of 16 B."""

    def __init__(self, name, key, steps=3, values=None):
        """``values``: (w, [g of step 1, ...]) in place of the seeded N(0, 1) draws and the mined elements."""
        self.name, self.key, self.dt, self.steps = name, key, DTYPES[key], steps
        P = KPER[key]
        self.numel = np.array(sizes(name, key), dtype=np.int64)
        n_keys, total = len(self.numel), int(self.numel.sum())
        j = np.arange(n_keys)
        if name in ("k130", "chain"):  # every sub-16-B offset on either side, and all four (aligned, aligned) pairs
            self.off = {"w": j % P, "g": (3 * j + 1) % P}
            self.off["g"][j % (4 * P) == 0] = 0
            self.off["g"][j % (4 * P) == 1] = 1
        else:
            self.off = {"w": np.zeros(n_keys, np.int64), "g": np.zeros(n_keys, np.int64)}
        self.start, self.size = {}, {}
        for side in "wg":
            start, cursor = np.empty(n_keys, dtype=np.int64), 0
            for k in range(n_keys):
                start[k] = -(-(cursor + PAD) // P) * P + self.off[side][k]
                cursor = start[k] + self.numel[k]
            self.start[side], self.size[side] = start, int(-(-(cursor + PAD) // P) * P)
        padded = (self.numel + P - 1) // P * P
        self.state_offset = (np.cumsum(padded) - padded).astype(np.int64)
        self.state_elems = int(max(padded.sum(), P))
        key_of = np.repeat(j, self.numel)
        first = np.cumsum(self.numel) - self.numel
        i = np.arange(total) - first[key_of]
        self.pos = {side: self.start[side][key_of] + i for side in "wg"}
        self.pos["s"] = self.state_offset[key_of] + i
        self._ref = {}
        if values is not None:
            self.w, self.g = values[0], list(values[1])
            assert len(self.g) == steps and all(len(t) == total and t.dtype == self.dt for t in (self.w, *self.g))
            return
        seed = sum(map(ord, name)) * 7 + len(key)
        self.w = normal(seed, total, self.dt)
        self.g = [normal(seed + 1 + t, total, self.dt) for t in range(steps)]
        if self.dt in (torch.bfloat16, torch.float16) and total >= 64:
            mw, mg0, mg1 = mined(key)
            at = torch.from_numpy(np.random.default_rng(n_keys).choice(total, min(len(mw), total), replace=False))
            self.w[at], self.g[0][at] = mw[:len(at)], mg0[:len(at)]
            if steps > 1:
                self.g[1][at] = mg1[:len(at)]

    def reference(self, form, **change):
        """Per step t = 1..steps: ((w', m', v', vmax'), record), each step from the one before; the first from zeros."""
        tag = (form, tuple(sorted(change.items())))
        if tag not in self._ref:
            out, w, state = [], self.w, (None, None, None)
            for t in range(self.steps):
                res, rec = A.reference(self.key, form, coef(t + 1, **change), t == 0, w, self.g[t], *state)
                out.append((res, rec))
                w, state = res[0], res[1:]
            self._ref[tag] = out
        return self._ref[tag]

    def host_buffer(self, side, values):
        buf = torch.full((self.size[side],), SENTINEL, dtype=self.dt)
        buf[torch.from_numpy(self.pos[side])] = values
        return buf

    def views(self, buf, side):
        return [buf[s:s + n] for s, n in zip(self.start[side].tolist(), self.numel.tolist())]


@functools.lru_cache(maxsize=None)
def case(name, key):
    return Case(name, key, steps=1 if name == "long" else 3)


def stored_differ(c, form_a, form_b, **change):
    """Elements of any stored tensor at any step on which the reference's answers under two masks differ."""
    n = 0
    for (ra, _), (rb, _) in zip(c.reference(form_a, **change), c.reference(form_b, **change)):
        for a, b in zip(ra, rb):
            n += int(((A.bits(a) != A.bits(b)) & ~(torch.isnan(a) & torch.isnan(b))).sum())
    return n


# --------------------------------------------------- chains held against torch.optim.Adam itself
# tests/test_gpu_client_adam_torch.py runs these through torch.optim.Adam, through ClientStepStats.adam_step() and
# through the host reference; tests/test_client_adam_torch_cases_cpu.py holds them to the conditions below.
#
# Twelve steps, a fresh seeded gradient each: g ~ 2^eg N(0, 1) in steps 1-6 and 2^(eg - 5) N(0, 1) in steps 7-12 (the
# second moment then decays below its maximum and amsgrad engages), w ~ 2^ew N(0, 1).  A scale is the pair (eg, ew).
#
# ew = 0 is a model of ordinary weights under gradients of every size.  With weight decay it cannot reach a small
# second moment: g1 = g + wd w is then wd w whatever g is, so at the reference's wd = 1e-3 and w ~ N(0, 1) v' is about
# 1e-9 w^2, far above the subnormal range of bf16, fp32 and fp64 (it does reach fp16's).  The last scale of those
# three types therefore shrinks the weights with the gradients (a "small model"), far enough that v' is subnormal or
# underflows: v' = 0.001 g1^2 is below the least normal value (2^-126, fp64 2^-1022) for g1 below 2^-58 (fp64
# 2^-506).  There sqrt(v) is far below eps, the step is lr m / eps, and with weight decay w grows about a
# hundredfold a step (lr wd / eps = 100), so under (a) and (c) v' is subnormal in the first five steps from 2^-70
# (fp64 2^-520); under (b), without weight decay, in all twelve.
HYPERS = {
    "a": dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-3),  # the reference's
    "b": dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0),   # no op A
    "c": dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-3, wd=1e-3),  # an eps fp16 keeps: a finite fp16 chain
    "d": dict(HYPER),                                               # the probe's, here at small magnitudes too
}
CHAIN_STEPS = 12
CHAIN_SHRINK = 5  # steps 7-12: the gradient scale over 32
CHAIN_SCALES = {
    "f32": ((0, 0), (-10, 0), (-20, 0), (-62, 0), (-70, -70)),
    "bf16": ((0, 0), (-10, 0), (-20, 0), (-62, 0), (-70, -70)),
    "f16": ((0, 0), (-6, 0), (-10, 0)),
    "f64": ((0, 0), (-10, 0), (-20, 0), (-62, 0), (-520, -520)),
}
STORED = ("w", "exp_avg", "exp_avg_sq", "max_exp_avg_sq")


def scale_id(scale):
    return f"g2^{scale[0]}_w2^{scale[1]}"


@functools.lru_cache(maxsize=None)
def chain(key, scale):
    """The Case of one dtype and scale: the "chain" sizes (1, 3, 16 B - 1, 16 B, 16 B + 1, 63, unit - 1, unit + 1
    and 2 units + 3 elements), k130's offsets for the flat layout, CHAIN_STEPS seeded gradients."""
    eg, ew = scale
    dt, total = DTYPES[key], sum(sizes("chain", key))
    seed = 5000 + 100 * KEYS.index(key) + 17 * CHAIN_SCALES[key].index(scale)
    w = normal(seed, total, dt, 2.0 ** ew)
    g = [normal(seed + 1 + t, total, dt, 2.0 ** (eg - (CHAIN_SHRINK if t >= CHAIN_STEPS // 2 else 0)))
         for t in range(CHAIN_STEPS)]
    return Case("chain", key, steps=CHAIN_STEPS, values=(w, g))


def chain_reference(key, scale, hyper, form=15):
    """Per step the host reference's (w', m', v', vmax') of the chain under hyperparameter set ``hyper`` (cached)."""
    return [res for res, _ in chain(key, scale).reference(form, **HYPERS[hyper])]


def subnormal(t):
    """Elements of t that are non-zero and below the least normal value of its type."""
    return (t != 0) & (t.abs() < torch.finfo(t.dtype).smallest_normal)


def chain_counts(stored, g):
    """What the conditions are about, per step, from the stored (w', m', v', vmax') of every step and the steps'
    gradients: elements with vmax' > v', with a subnormal v', with v' == 0 under g != 0 (underflowed), and whether
    all four tensors are finite."""
    out = {"vmax_gt_v": [], "subnormal_v": [], "underflowed_v": [], "finite": []}
    for (w, m, v, x), g_t in zip(stored, g):
        out["vmax_gt_v"].append(int((x > v).sum()))
        out["subnormal_v"].append(int(subnormal(v).sum()))
        out["underflowed_v"].append(int(((v == 0) & (g_t != 0)).sum()))
        out["finite"].append(all(bool(torch.isfinite(t).all()) for t in (w, m, v, x)))
    return out


def condition_sets(key):
    """The hyperparameter sets check_conditions() reads for a dtype."""
    return {"f16": ("a", "c"), "bf16": ("a", "d")}.get(key, ("a",))


def check_conditions(key, counts):
    """The conditions the chains' inputs must meet, on the counts (chain_counts) of every scale of one dtype:
    ``counts[hyper][scale]`` for the sets of condition_sets(key).  They are the same for the host reference's states
    and for torch's.  All are about set (a), the reference's, with two exceptions that arithmetic forces:

    * bf16 never has vmax' > v' at beta2 = 0.999: v * 0.999 is within half a bf16 ulp of v (half an ulp is 2^-9 of
      v or more, also downwards from a power of two, where v * 0.999 lies above the midpoint 0.998 v), so v1 =
      rT(v * beta2) = v, v' >= v and the maximum is always the new value.  That is asserted, and amsgrad engaged is
      asked of set (d), beta2 = 0.7.
    * fp16 rounds s3 = s2 + 1e-8 to 0 where v is 0, so no fp16 chain under (a) stays finite; the finite one is (c)'s."""
    total = sum(sizes("chain", key))
    every = list(counts["a"].values())
    # amsgrad engaged: somewhere a quarter of the elements keep an older maximum, and some do in every step from 7 on
    engaged = every
    if key == "bf16":
        assert all(max(c["vmax_gt_v"]) == 0 for c in every), (key, [c["vmax_gt_v"] for c in every])
        engaged = list(counts["d"].values())
    assert any(max(c["vmax_gt_v"]) >= total / 4 for c in engaged), (key, [c["vmax_gt_v"] for c in engaged])
    assert any(min(c["vmax_gt_v"][CHAIN_STEPS // 2:]) >= 1 for c in engaged), (key, [c["vmax_gt_v"] for c in engaged])
    # a stored second moment that is subnormal in the model's type
    assert any(max(c["subnormal_v"]) >= 64 for c in every), (key, [c["subnormal_v"] for c in every])
    if key in ("bf16", "f16"):  # and one that underflowed
        assert any(max(c["underflowed_v"]) >= 64 for c in every), (key, [c["underflowed_v"] for c in every])
    # a chain that stays finite to the end
    finite = counts["c" if key == "f16" else "a"]
    assert any(all(c["finite"]) for c in finite.values()), (key, {s: c["finite"] for s, c in finite.items()})


def plant_specials(c):
    """test_special_values_equal_the_reference's elements in every step of Case ``c`` (sizes "edges" or "chain")."""
    tiny = torch.finfo(c.dt).smallest_normal
    for g in c.g:
        g[0], g[1], g[2] = math.nan, math.inf, -math.inf
        g[3], c.w[3] = 0.0, 0.0                       # wd * w + g = 0: v' = 0, s3 = eps, 0 / eps
        g[4], c.w[4] = 0.0, -0.0
        g[5], c.w[5] = math.sqrt(tiny) / 4, 0.0       # g1^2 subnormal: subnormal v and vmax
        g[6], c.w[6] = tiny / 2, tiny / 4             # subnormal g and w
        g[7], c.w[7] = 6.0e4, 6.0e4                   # g1^2 overflows fp16
        g[len(g) - 1] = math.nan                      # in the ragged last slice of the last key
    return c


@functools.lru_cache(maxsize=None)
def specials(key):
    """Two steps on the chain sizes with the special values planted (w, g ~ N(0, 1) otherwise)."""
    total = sum(sizes("chain", key))
    seed = 7000 + KEYS.index(key)
    values = (normal(seed, total, DTYPES[key]), [normal(seed + 1 + t, total, DTYPES[key]) for t in range(2)])
    return plant_specials(Case("chain", key, steps=2, values=values))
