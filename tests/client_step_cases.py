"""The launches tests/test_gpu_client_step_ref.py sends through
fedavg_client_sgd_step_*, built on the host (no GPU, no compiled code), and
the condition under which a launch can tell the kernel's two forms apart.
tests/test_client_step_ref_cpu.py asserts that condition for every case
without a GPU; the GPU tests assert it again before they launch.

A case is a list of keys (sizes in elements), the offset in elements of each
key's weights and of its gradients from a 16-B boundary, and the keys' values
end to end.  Each side lives in ONE buffer: key j starts PAD or more sentinel
elements after key j - 1 ends.  U is a unit (16 KiB of the tensor), kPer the
elements of a 16-B slice:

  one    [U + 1], aligned: a whole unit and a one-element ragged one
  k130   130 keys (a second round of the kernel's key search), sizes cycling
         through 0, 1, kPer-1, kPer, kPer+1, 63, U-1, U, U+1; keys 0, 9, 10
         and 129 are empty (first, two in a row, last)
  k4100  4100 keys of 0-3 elements (a third round; more than 256 units and no
         multiple of 256, so the finalize kernel's loop strides)
  long   one key of 257 U + 3 elements, aligned (a key of more than 256 units)

In k130 and k4100 key j lies j mod kPer elements past a 16-B boundary in w and
(3 j + 1) mod kPer in g, so one launch holds every sub-16-B offset on either
side.  That rule alone never aligns both sides of a key (j = 0 and 3 j + 1 = 0
mod kPer have no common solution for kPer = 2, 4, 8) and, for kPer = 2, never
misaligns both, so two keys in every 4 kPer leave it: j mod 4 kPer = 0 has its
gradients aligned as well (the kernel's 16-B path on both sides) and
j mod 4 kPer = 1 has them one element off, like its weights.  With these all
four of the kernel's (w aligned, g aligned) branches occur in every dtype.

Values: model-like weights N(0, 0.05^2) and gradients N(0, 1), seeded.  In a
16-bit type the two forms differ on about one such element in 33,000, so
(w, g) pairs on which the host reference's forms differ are mined from a seeded
pool of 2^21 (as client_stats._probe_values does) and placed at two elements
of every "place" the case has, and at 64 more: a place is (the thread's slice
s = 0..3, the even or odd half of a packed 32-bit word, whole slice / ragged
slice / ragged last slice of a U + 1 key, w aligned, g aligned)."""
import functools

import numpy as np
import torch

import client_step_ref as R

DTYPES = R.DTYPES
UNIT = {"f32": 4096, "bf16": 8192, "f16": 8192, "f64": 2048}  # elements of 16 KiB
KPER = {"f32": 4, "bf16": 8, "f16": 8, "f64": 2}              # elements of 16 B
KEYS = tuple(DTYPES)
CASES = ("one", "k130", "k4100", "long")
LR = 0.03          # at 0.001 a 16-bit pool holds 3 telling elements, not 60
MIN_DIFFER = 32
SENTINEL = 123.0   # exact in every dtype
PAD = 8            # sentinel elements, at least, around every key
POOL, POOL_SEED = 1 << 21, 20250


def _normal(seed, n, dt):
    rng = np.random.default_rng(seed)
    return (torch.from_numpy(rng.normal(0.0, 0.05, n)).to(dt), torch.from_numpy(rng.normal(0.0, 1.0, n)).to(dt))


@functools.lru_cache(maxsize=None)
def pool(key):
    """The seeded pool: (w, g) of POOL elements each."""
    return _normal(POOL_SEED, POOL, DTYPES[key])


def forms_differ(key, lr, w, g):
    """Where the reference's two forms leave different bits (both NaN counts as the same)."""
    alpha = R.alpha_of(key, lr)
    a, b = R.step(key, 0, alpha, w, g), R.step(key, 1, alpha, w, g)
    return ((R.bits(a) != R.bits(b)) & ~(torch.isnan(a) & torch.isnan(b))).numpy()


@functools.lru_cache(maxsize=None)
def pool_differ(key, lr):
    """Indices of the pool's elements on which the two forms differ at `lr`."""
    return np.flatnonzero(forms_differ(key, lr, *pool(key)))


def mined(key, most=64):
    """Up to `most` (w, g) pairs of the pool on which the forms differ at LR."""
    idx = torch.from_numpy(pool_differ(key, LR)[:most])
    w, g = pool(key)
    return w[idx].clone(), g[idx].clone()


def sizes(name, key):
    U, P = UNIT[key], KPER[key]
    if name == "one":
        return [U + 1]
    if name == "long":
        return [257 * U + 3]
    if name == "k130":
        cycle = [0, 1, P - 1, P, P + 1, 63, U - 1, U, U + 1]
        n = [cycle[j % 9] for j in range(130)]
        n[10] = n[129] = 0
        return n
    if name == "k4100":
        return np.random.default_rng(4100).integers(0, 4, 4100).tolist()
    raise KeyError(name)


class Case:
    def __init__(self, name, key):
        self.name, self.key, self.dt = name, key, DTYPES[key]
        U, P = UNIT[key], KPER[key]
        self.numel = np.array(sizes(name, key), dtype=np.int64)
        n_keys, total = len(self.numel), int(self.numel.sum())
        j = np.arange(n_keys)
        if name in ("k130", "k4100"):
            self.w_off, self.g_off = j % P, (3 * j + 1) % P
            self.g_off[j % (4 * P) == 0] = 0
            self.g_off[j % (4 * P) == 1] = 1
        else:
            self.w_off, self.g_off = np.zeros(n_keys, dtype=np.int64), np.zeros(n_keys, dtype=np.int64)
        self.units = int(((self.numel + U - 1) // U).sum())
        # where each key starts in its side's buffer, and the buffers' sizes
        self.start, self.size = {}, {}
        for side, off in (("w", self.w_off), ("g", self.g_off)):
            start, cursor = np.empty(n_keys, dtype=np.int64), 0
            for k in range(n_keys):
                start[k] = -(-(cursor + PAD) // P) * P + off[k]
                cursor = start[k] + self.numel[k]
            self.start[side], self.size[side] = start, int(-(-(cursor + PAD) // P) * P)
        # per element: its key, and its place in the launch
        key_of = np.repeat(j, self.numel)
        first = np.cumsum(self.numel) - self.numel
        i = np.arange(total) - first[key_of]
        col = i % U
        live = np.minimum(self.numel[key_of] - (i - col), U)  # the unit's columns
        ragged = (col // P) * P + P > live
        self.slice_s = col // P // 256
        self.half = col & 1
        self.ragged = ragged.astype(np.int64) + (ragged & (self.numel[key_of] == U + 1))
        self.wvec, self.gvec = self.w_off[key_of] == 0, self.g_off[key_of] == 0
        self.place = self.slice_s + 4 * (self.half + 2 * (self.ragged + 3 * (self.wvec + 2 * self.gvec)))
        self.pos = {side: self.start[side][key_of] + i for side in ("w", "g")}
        # values
        self.w, self.g = _normal(sum(map(ord, name)) * 7 + len(key), total, self.dt)
        _, lo = np.unique(self.place, return_index=True)
        _, hi = np.unique(self.place[::-1], return_index=True)
        more = np.random.default_rng(n_keys).choice(total, min(64, total), replace=False)
        at = torch.from_numpy(np.unique(np.concatenate([lo, total - 1 - hi, more])))
        mw, mg = mined(key)
        pick = torch.arange(len(at)) % len(mw)
        self.w[at], self.g[at] = mw[pick], mg[pick]
        self.placed = at.numpy()
        self._ref = {}

    # ------------------------------------------------------------- the reference
    def reference(self, form):
        """(w', (NaN count, sum w'^2, sum d^2)) of form `form` at LR, computed once."""
        if form not in self._ref:
            self._ref[form] = R.reference(self.key, form, R.alpha_of(self.key, LR), self.w, self.g)
        return self._ref[form]

    def differ(self):
        a, b = self.reference(0)[0], self.reference(1)[0]
        return ((R.bits(a) != R.bits(b)) & ~(torch.isnan(a) & torch.isnan(b))).numpy()

    def branches(self):
        """The (w aligned, g aligned) pairs of the keys with elements."""
        live = self.numel > 0
        return set(zip((self.w_off[live] == 0).tolist(), (self.g_off[live] == 0).tolist()))

    def assert_discriminates(self):
        """The two forms differ on MIN_DIFFER elements or more, and on one or more in every place the case has."""
        d = self.differ()
        assert int(d.sum()) >= MIN_DIFFER, (self.name, self.key, int(d.sum()))
        missed = set(self.place.tolist()) - set(self.place[d].tolist())
        assert not missed, (self.name, self.key, sorted(missed))
        return int(d.sum())

    # --------------------------------------------------------------- the buffers
    def host_buffer(self, side):
        """The side's buffer as a CPU tensor: sentinels, and every key's values at its place."""
        buf = torch.full((self.size[side],), SENTINEL, dtype=self.dt)
        buf[torch.from_numpy(self.pos[side])] = self.w if side == "w" else self.g
        return buf

    def views(self, buf, side):
        """The keys as views into a buffer laid out as host_buffer(side)."""
        return [buf[s:s + n] for s, n in zip(self.start[side].tolist(), self.numel.tolist())]

    def gaps(self, side):
        """A mask of the buffer's sentinel elements."""
        m = np.ones(self.size[side], dtype=bool)
        m[self.pos[side]] = False
        return torch.from_numpy(m)


@functools.lru_cache(maxsize=None)
def case(name, key):
    return Case(name, key)


def specials(key, nonfinite=True):
    """test_gpu_client_step.test_special_values' inputs: NaN and +-inf in g
    (only with `nonfinite`), subnormal w and g, -0.0, and |g| large enough to
    overflow fp16, in one [U + 1] key whose last element is a ragged slice."""
    import math

    dt, n = DTYPES[key], UNIT[key] + 1
    w, g = _normal(41, n, dt)
    tiny = torch.finfo(dt).smallest_normal
    if nonfinite:
        g[0], g[1], g[2], g[n - 1] = math.nan, math.inf, -math.inf, math.nan
    w[3], g[3] = tiny / 4, 0.0            # subnormal w kept
    w[4], g[4] = tiny / 4, tiny / 2       # subnormal w and g
    w[5], g[5] = 0.0, tiny / 8            # a subnormal (or vanishing) product alone
    w[6], g[6] = -0.0, 0.0                # -0.0 + (-lr * 0.0)
    w[7], g[7] = -0.0, -0.0
    w[8], g[8] = 1.0, 6.0e4               # finite in fp16, w' is not past lr 0.03; the next ones are
    w[9], g[9] = 6.0e4, -6.0e4
    w[10], g[10] = -6.0e4, 6.5e4
    w[n - 2], g[n - 2] = tiny / 2, -tiny  # in the last whole slice
    return w, g
