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
host reference's answers under the two settings of the bit differ."""
import functools

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
    raise KeyError(name)


class Case:
    """Keys in one buffer per side (w, g), PAD or more sentinels around each; the state planes are laid out as
    ClientStepStats lays them out: every key at the next multiple of 16 B."""

    def __init__(self, name, key, steps=3):
        self.name, self.key, self.dt, self.steps = name, key, DTYPES[key], steps
        P = KPER[key]
        self.numel = np.array(sizes(name, key), dtype=np.int64)
        n_keys, total = len(self.numel), int(self.numel.sum())
        j = np.arange(n_keys)
        if name == "k130":  # every sub-16-B offset on either side, and all four (aligned, aligned) pairs
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
        seed = sum(map(ord, name)) * 7 + len(key)
        self.w = normal(seed, total, self.dt)
        self.g = [normal(seed + 1 + t, total, self.dt) for t in range(steps)]
        if self.dt in (torch.bfloat16, torch.float16) and total >= 64:
            mw, mg0, mg1 = mined(key)
            at = torch.from_numpy(np.random.default_rng(n_keys).choice(total, min(len(mw), total), replace=False))
            self.w[at], self.g[0][at] = mw[:len(at)], mg0[:len(at)]
            if steps > 1:
                self.g[1][at] = mg1[:len(at)]
        self._ref = {}

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


def stored_differ(c, form_a, form_b):
    """Elements of any stored tensor at any step on which the reference's answers under two masks differ."""
    n = 0
    for (ra, _), (rb, _) in zip(c.reference(form_a), c.reference(form_b)):
        for a, b in zip(ra, rb):
            n += int(((A.bits(a) != A.bits(b)) & ~(torch.isnan(a) & torch.isnan(b))).sum())
    return n
