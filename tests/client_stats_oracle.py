"""numpy fp64 oracle of the client statistics (client.py:52-86) and helpers
shared by the client-statistics tests (a plain module, not a conftest).

``record`` is the record of ``fedavg_client_stats_f32``: the NaN count, the sum
of cur^2 and the sum of fl32(cur - snap)^2, squares and sums exact
(``math.fsum`` of fp64 squares of fp32 values, rounded once).  ``Track`` is the
running rule of client.py:78-84 in the reference's fp32 arithmetic on
exactly rounded norms; ``replay`` runs a recorded (w_t, g_t, loss_t) sequence
through both and the :71 guard.

The fixtures under tests/golden/client come from the reference's own
``Client.train`` (scripts/gen_golden_client.py).
"""
from __future__ import annotations

import json
import math
import sys
import time
import types
from pathlib import Path

import numpy as np

CLIENT_GOLDEN = Path(__file__).resolve().parent / "golden" / "client"


# ---------------------------------------------------------------- the oracle
def _sumsq(a32: np.ndarray) -> float:
    a = np.asarray(a32, dtype=np.float32).astype(np.float64).ravel()
    if a.size == 0:
        return 0.0
    sq = a * a  # exact: an fp32 value squared fits fp64
    if not np.all(np.isfinite(sq)):
        return float(np.sum(sq))  # NaN / inf propagate; no cancellation (all terms >= 0)
    return math.fsum(sq.tolist())


def record(cur, snap=None):
    """(nan_count, sum cur^2, sum fl32(cur - snap)^2); the last is 0 without a snapshot."""
    cur = np.asarray(cur, dtype=np.float32).ravel()
    nan_count = int(np.isnan(cur).sum())
    with np.errstate(all="ignore"):
        s_cur = _sumsq(cur)
        s_d = 0.0 if snap is None else _sumsq(cur - np.asarray(snap, dtype=np.float32).ravel())  # fp32 difference
    return nan_count, s_cur, s_d


def norm32(sumsq: float) -> np.float32:
    """fl32(sqrt(sum)): the exactly rounded value of what torch.norm approximates in fp32."""
    with np.errstate(all="ignore"):
        return np.float32(np.sqrt(np.float64(sumsq)))


def update(x, tmp):
    """client.py:79 / :83: ``if not x or tmp > x: x = tmp`` (None = unset)."""
    if x is None or x == 0 or tmp > x:
        return tmp
    return x


class Track:
    def __init__(self):
        self.rho = None
        self.beta = None

    def step(self, sum_dw: float, sum_dg: float, abs_dloss: float):
        with np.errstate(all="ignore"):
            n_w, n_g = norm32(sum_dw), norm32(sum_dg)
            # python_float / fp32 tensor = tensor.reciprocal() * python_float, the scalar rounded to fp32
            rho_tmp = np.float32(np.float32(1.0) / n_w) * np.float32(abs_dloss)
            beta_tmp = np.float32(n_g / n_w)
        self.rho = update(self.rho, np.float32(rho_tmp))
        self.beta = update(self.beta, beta_tmp)
        return rho_tmp, beta_tmp


def guard(nan_count: int, sum_g: float, sum_last_w: float, loss: float, lr: float, ratio: float) -> bool:
    """client.py:71."""
    with np.errstate(all="ignore"):
        bound = np.float32(lr * ratio) * norm32(sum_last_w)
        return bool(nan_count > 0 or math.isnan(loss) or norm32(sum_g) > bound)


def replay(w, g, loss, lr, ratio):
    """w[0], g[0], loss[0]: the prologue (client.py:52-57); then per iteration
    t >= 1 the gradients g[t] (:69), the loss and, unless the guard trips, the
    weights w[t] (:76).  Returns (tripped_at or None, beta, rho)."""
    track = Track()
    for t in range(1, len(g)):
        nan_g, sum_g, sum_dg = record(g[t], g[t - 1])
        _, sum_last_w, _ = record(w[t - 1])
        if guard(nan_g, sum_g, sum_last_w, float(loss[t]), lr, ratio):
            return t - 1, None, None
        _, _, sum_dw = record(w[t], w[t - 1])
        track.step(sum_dw, sum_dg, abs(float(loss[t]) - float(loss[t - 1])))
    return (None, None if track.beta is None else float(track.beta), None if track.rho is None else float(track.rho))


# ------------------------------------------------------------------ fixtures
def client_case_names():
    return sorted(p.stem for p in CLIENT_GOLDEN.glob("*.npz"))


def load_client_case(name: str):
    z = np.load(CLIENT_GOLDEN / f"{name}.npz", allow_pickle=False)
    case = {k: z[k] for k in z.files if k != "meta"}
    case["meta"] = json.loads(str(z["meta"]))
    return case


def ref_bound(meta) -> float:
    """How close anything built on exact norms can be held to the reference's
    returned rho / beta: a ratio of two norms, maximised over iterations,
    compounds the measured per-fixture fp32-norm gap."""
    return 4.0 * float(meta["ref_vs_exact_rel"]) + 1e-6


def rel(a: float, b: float) -> float:
    if a == b:
        return 0.0
    return abs(a - b) / max(abs(b), 1e-300)


def build_model(spec):
    """{"sizes": [in, (hidden, ...) out]}: Linear layers with ReLU between."""
    import torch

    sizes = spec["sizes"]
    layers = []
    for i in range(len(sizes) - 1):
        if i:
            layers.append(torch.nn.ReLU())
        layers.append(torch.nn.Linear(sizes[i], sizes[i + 1]))
    return torch.nn.Sequential(*layers)


def load_flat(net, flat):
    """Write a flattened parameter vector (parameters() order) into net."""
    import torch

    off = 0
    with torch.no_grad():
        for p in net.parameters():
            n = p.numel()
            p.copy_(torch.as_tensor(np.array(flat[off:off + n]), dtype=p.dtype).view_as(p))
            off += n
    assert off == len(flat)
    return net


def flat_of(tensors):
    import torch

    return torch.cat([t.detach().reshape(-1).cpu() for t in tensors]).numpy()


def make_client_class(ratio):
    """A stand-in for the reference's ``client`` module and its ``Client``:
    the attributes client_train reads from the patched class's own module
    (count / count_end / THRESHOLD_GRADS_RATIO) and from ``self``."""
    import torch

    name = f"_client_stats_fake_client_{int(ratio)}"
    mod = sys.modules.get(name)
    if mod is None:
        mod = types.ModuleType(name)
        mod.count = time.perf_counter_ns
        mod.count_end = time.perf_counter_ns
        mod.THRESHOLD_GRADS_RATIO = ratio
        sys.modules[name] = mod

        class Client:
            def __init__(self, batch, args, device):
                self.local_training_data = [batch]
                self.args = args
                self.device = device
                self.criterion = torch.nn.CrossEntropyLoss().to(device)

            def train(self, net, local_iteration):
                raise NotImplementedError("the reference's Client.train is not part of this repository")

        Client.__module__ = name
        mod.Client = Client
    return mod.Client


def case_client(case, device):
    """(client, net) set up as the fixture's generator set the reference up."""
    import torch

    meta = case["meta"]
    args = types.SimpleNamespace(client_optimizer="sgd", lr=meta["lr"], wd=0.0, clip=meta["clip"], dataset="mnist")
    x = torch.from_numpy(np.array(case["x"]))
    labels = torch.from_numpy(np.array(case["labels"]))
    client = make_client_class(meta["ratio"])((x, labels), args, device)
    net = load_flat(build_model(meta["model"]), case["w"][0]).to(device)
    return client, net
