"""Generate the client-statistics fixtures by running the REFERENCE's Client.train.

Run by hand where the reference is present (it is not on the GPU box):

    python scripts/gen_golden_client.py        # writes tests/golden/client/*.npz

Reuses the stub modules and paths of ``oracle/gen_golden.py`` (the reference
imports ``hwcounter`` and reads ``../data`` at import).  A child process imports
the reference's ``client`` module (read-only, never copied), runs
``Client.train`` (client.py:38-96) on CPU on tiny seeded models and records what
it computed: every flattened weight / gradient vector it built (its own
``torch.cat`` results at :52, :57, :69, :76), every loss its criterion
returned, and its returned tuple.  Only these data are written.

Each ``.npz`` holds ``meta`` (JSON: model sizes, lr, clip, ratio,
local_iteration, whether the :71 guard tripped, ``ref_vs_exact_rel``), ``x``,
``labels``, ``w`` [steps + 1, P] (row 0 = the initial weights), ``g`` (row 0 =
the prologue's gradients), ``loss`` (fp32; entry 0 = the prologue's), ``ret`` =
(loss, beta, rho, acc) as the reference returned them (NaN = None) and
``w_final``, the returned state_dict flattened.

``ref_vs_exact_rel`` is measured here: the relative gap between the
reference's returned rho / beta and the same quantities formed from the
recorded tensors with exactly rounded (fp64-summed) norms
(tests/client_stats_oracle.py), i.e. the reference's own fp32-norm error on
this host.
"""
from __future__ import annotations

import os
import subprocess
import sys
import tempfile
import textwrap
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "oracle"))
from gen_golden import _STUB_HWCOUNTER, _STUB_WANDB, REF_DATA, REF_SRC  # noqa: E402

OUT_DIR = REPO / "tests" / "golden" / "client"

_CHILD = r'''
import json, sys, types
import numpy as np
import torch

import client as ref_client            # the reference's src/client.py
import client_stats_oracle as O        # tests/client_stats_oracle.py

out_dir = sys.argv[1]
RATIO = ref_client.THRESHOLD_GRADS_RATIO


class Recorder:
    """The reference's own flattened vectors: torch.cat calls over the model's tensors."""
    def __init__(self, n_params, P):
        self.n_params, self.P, self.cats = n_params, P, []
        self._cat = torch.cat
    def __call__(self, tensors, *a, **k):
        out = self._cat(tensors, *a, **k)
        if isinstance(tensors, (list, tuple)) and len(tensors) == self.n_params and out.dim() == 1 \
                and out.numel() == self.P:
            self.cats.append(out.detach().clone().numpy())
        return out


class Criterion:
    def __init__(self, inner):
        self.inner, self.losses = inner, []
    def __call__(self, *a):
        loss = self.inner(*a)
        self.losses.append(np.float32(loss.detach().item()))
        return loss


def run(name, sizes, iters, lr, seed, batch=8, scale=1.0, x_scale=1.0, nan_input=False, expect_trip=False,
        note=""):
    torch.manual_seed(seed)
    spec = {"sizes": sizes}
    net = O.build_model(spec)
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(scale)
    gen = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(batch, sizes[0], generator=gen) * x_scale
    labels = torch.randint(0, sizes[-1], (batch,), generator=gen)
    if nan_input:
        x[0, 0] = float("nan")
    args = types.SimpleNamespace(dataset="mnist", client_optimizer="sgd", lr=lr, wd=0.0, clip=1.0)
    c = ref_client.Client(0, [(x, labels)], None, batch, args, torch.device("cpu"))
    c.criterion = Criterion(c.criterion)
    params = list(net.parameters())
    P = sum(p.numel() for p in params)
    rec = Recorder(len(params), P)
    torch.cat = rec
    try:
        sd, loss, beta, rho, acc, cycles = c.train(net, iters)
    finally:
        torch.cat = rec._cat
    tripped = loss is None
    assert tripped == expect_trip, (name, tripped)
    cats, losses = rec.cats, c.criterion.losses
    w = [cats[0]] + cats[3::2]
    g = [cats[1]] + cats[2::2]
    steps = len(w) - 1
    assert len(g) == steps + (2 if tripped else 1) and len(losses) == len(g), (len(w), len(g), len(losses))
    assert tripped or steps == iters
    w_final = O.flat_of(sd.values())
    assert tripped or w_final.tobytes() == w[-1].tobytes()
    # the reference's fp32-norm error: its rho / beta against exactly rounded norms
    t_at, o_beta, o_rho = O.replay(w, g, losses, lr, RATIO)
    assert (t_at is not None) == tripped
    gap = 0.0 if tripped else max(O.rel(beta, o_beta), O.rel(rho, o_rho))
    meta = {"case": name, "note": note, "model": spec, "P": P, "lr": lr, "clip": 1.0, "ratio": RATIO,
            "local_iteration": iters, "tripped": tripped, "steps": steps, "ref_vs_exact_rel": gap,
            "generator": "scripts/gen_golden_client.py (reference Client.train, client.py:38-96)",
            "torch": torch.__version__}
    none = float("nan")
    np.savez_compressed(
        f"{out_dir}/{name}.npz", meta=np.array(json.dumps(meta)), x=x.numpy(), labels=labels.numpy(),
        w=np.stack(w), g=np.stack(g), loss=np.array(losses, dtype=np.float32), w_final=w_final,
        ret=np.array([none if v is None else v for v in (loss, beta, rho, acc)], dtype=np.float64))
    print(f"{name}: P={P} steps={steps} tripped={tripped} beta={beta} rho={rho} ref_vs_exact_rel={gap:.3e}")


run("linear_20x5_it3", [20, 5], 3, 0.03, seed=1)
run("linear_20x5_it1", [20, 5], 1, 0.03, seed=1)
run("mlp_16x24x4_it4", [16, 24, 4], 4, 0.03, seed=2, note="P = 508")
run("mnist_lr_it2", [784, 10], 2, 0.03, seed=3, batch=4, x_scale=0.1,
    note="MNIST-LR shape, P = 7,850")
run("nan_input_trips", [20, 5], 3, 0.03, seed=4, nan_input=True, expect_trip=True,
    note="a NaN input: NaN loss and gradients trip client.py:71")
run("tiny_weights_trip", [20, 5], 3, 0.03, seed=5, scale=1e-4, expect_trip=True,
    note="norm(grads) > lr * ratio * norm(last_w) trips client.py:71")
'''


def main() -> int:
    if not (REF_SRC / "client.py").exists():
        print("reference not present; the fixtures can only be generated where it is")
        return 1
    OUT_DIR.mkdir(parents=True, exist_ok=True)
    with tempfile.TemporaryDirectory(prefix="fedavg_golden_client_") as tmp:
        tmp = Path(tmp)
        stubs = tmp / "stubs"
        stubs.mkdir()
        (stubs / "wandb.py").write_text(textwrap.dedent(_STUB_WANDB))
        (stubs / "hwcounter.py").write_text(textwrap.dedent(_STUB_HWCOUNTER))
        (tmp / "data").symlink_to(REF_DATA)
        run = tmp / "run"
        run.mkdir()
        child = tmp / "child.py"
        child.write_text(_CHILD)
        env = dict(os.environ)
        env["PYTHONPATH"] = f"{stubs}:{REF_SRC}:{REPO / 'tests'}"
        env["PYTHONDONTWRITEBYTECODE"] = "1"
        env["CUDA_VISIBLE_DEVICES"] = ""
        return subprocess.run([sys.executable, str(child), str(OUT_DIR)], cwd=run, env=env).returncode


if __name__ == "__main__":
    sys.exit(main())
