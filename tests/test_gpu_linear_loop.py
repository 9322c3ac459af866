"""The fused local loop of a linear softmax client (``client_train(loop="linear" / "linear_sigmoid")``) against
the loop of client.py:52-96 in fp64 torch on the CPU (linear_loop_ref.py).  The bounds are 4x the largest deviation
from that reference of the existing fp32 path (``loop="torch"`` on the GPU) over the same cases: both
are fp32 evaluations that differ in summation order; an indexing or tail mistake is wrong by orders of magnitude
more.  W and b: largest absolute difference; loss, beta, rho: relative difference."""
import functools
import math

import numpy as np
import pytest
import torch

from linear_loop_ref import linear_loop_ref, make_client
from mfl_amd import client_stats
from mfl_amd.client_passes import _LinearLoop

pytestmark = pytest.mark.gpu

# the existing path's largest deviations over CASES (torch 2.10 / ROCm 7.0, MI355X), times 4
BOUND = {"w": 4 * 3.30e-6, "loss": 4 * 4.94e-7, "beta": 4 * 4.85e-5, "rho": 4 * 3.70e-4}
RATIO = 1e4
HYPER = {"sgd": dict(lr=0.05, wd=0.0), "adam": dict(lr=0.001, wd=0.001)}
# (B, D, C, activation, optimizer, local_iteration, seed): tile edges (16 | 17, 33), tails (D = 1, 3, 5), one tile and
# many, the limits (64, 1024, 16), the resident batch (32 x 1024) and the re-read one (33 x 1024, 64 x 1024)
CASES = [
    (1, 1, 2, "none", "sgd", 1, 0), (1, 784, 10, "sigmoid", "adam", 5, 0), (16, 3, 2, "sigmoid", "sgd", 5, 0),
    (16, 4, 10, "none", "adam", 1, 0), (16, 1024, 16, "none", "sgd", 5, 0), (17, 5, 16, "sigmoid", "adam", 5, 1),
    (17, 784, 2, "none", "sgd", 1, 0), (17, 1024, 10, "sigmoid", "sgd", 5, 0), (33, 1, 10, "none", "adam", 5, 2),
    (33, 4, 16, "sigmoid", "sgd", 1, 1), (33, 784, 16, "none", "adam", 5, 0), (33, 1024, 2, "sigmoid", "adam", 1, 0),
    (64, 3, 16, "none", "sgd", 5, 0), (64, 5, 2, "sigmoid", "adam", 1, 0), (64, 784, 10, "none", "sgd", 5, 0),
    (64, 1024, 16, "sigmoid", "adam", 5, 0), (32, 1024, 10, "none", "adam", 5, 0), (32, 784, 10, "none", "sgd", 5, 0),
    (32, 784, 10, "sigmoid", "adam", 5, 0), (1, 5, 16, "none", "adam", 5, 0), (16, 784, 16, "sigmoid", "sgd", 1, 0),
    (64, 4, 10, "none", "adam", 5, 1), (17, 3, 10, "none", "sgd", 5, 0), (33, 5, 2, "none", "sgd", 1, 0),
]


def Net(W, b, activation):
    net = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(W.shape[1], W.shape[0]),
                              torch.nn.Sigmoid() if activation == "sigmoid" else torch.nn.Identity())
    net.linear = net[1]
    net.linear.weight.data, net.linear.bias.data = W.clone(), b.clone()
    return net


def inputs(B, D, C, seed):
    g = torch.Generator().manual_seed(1000 * seed + B + 7 * D + 13 * C)
    W, b = torch.randn(C, D, generator=g) / math.sqrt(D), torch.randn(C, generator=g)
    return W, b, torch.randn(B, D, generator=g), torch.randint(0, C, (B,), generator=g)


@functools.lru_cache(maxsize=None)
def reference(case):
    B, D, C, activation, optimizer, iters, seed = case
    return linear_loop_ref(*inputs(B, D, C, seed), iters=iters, activation=activation, optimizer=optimizer,
                           ratio=RATIO, **HYPER[optimizer])


def train(case, loop):
    """client_train on the GPU: (W, b, loss, beta, rho, correct)."""
    B, D, C, activation, optimizer, iters, seed = case
    W, b, x, y = inputs(B, D, C, seed)
    dev = torch.device("cuda", 0)
    net = Net(W, b, activation).to(dev)
    kw = dict(loop="linear_sigmoid" if activation == "sigmoid" else "linear") if loop else {}
    client = make_client(x.to(dev), y.to(dev), dev, optimizer, ratio=RATIO, **HYPER[optimizer])
    sd, loss, beta, rho, acc, cycles = client_stats.client_train(client, net, iters, **kw)
    assert cycles > 0
    return sd["1.weight"], sd["1.bias"], loss, beta, rho, round(acc * B)


def deviations(out, ref):
    """Per compared quantity, the deviation of a ``train`` result from the fp64 reference."""
    W, b, loss, beta, rho, correct = out
    rel = lambda a, r: abs(a - r) / abs(r) if r else abs(a)  # noqa: E731
    return {"w": max(float((W.double() - ref["W"]).abs().max()), float((b.double() - ref["b"]).abs().max())),
            "loss": rel(loss, ref["loss"]), "beta": rel(beta, ref["beta"]), "rho": rel(rho, ref["rho"])}


@pytest.mark.parametrize("case", CASES, ids=str)
def test_fused_loop_matches_the_fp64_reference(case):
    ref = reference(case)
    assert ref["trip"] == -1 and ref["top2_gap"] >= 1e-3 and max(ref["guard_ratio"]) <= 0.5  # what the inputs owe
    out = train(case, True)
    dev = deviations(out, ref)
    print(case, dev)  # each figure before it is held to its bound
    assert out[5] == ref["correct"]
    again = train(case, True)  # two launches on equal inputs: the same bits
    assert all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(out[:2], again[:2]))
    assert out[2:] == again[2:]
    for k, bound in BOUND.items():
        assert dev[k] <= bound, (k, dev[k], bound)


def launch(W, b, x, y, *, iters, activation, optimizer, ratio):
    """The kernel through its host plan: the record and the parameters it leaves."""
    dev = torch.device("cuda", 0)
    W, b, x, y = (t.to(dev) for t in (W, b, x, y))
    W.requires_grad_(True), b.requires_grad_(True)
    h = HYPER[optimizer]
    form = client_stats.sgd_form if optimizer == "sgd" else client_stats.adam_form
    plan = _LinearLoop([W, b], x, y, torch.nn.CrossEntropyLoss(), lambda d: form(d, torch.float32))
    rec = plan.run(iters, int(activation == "sigmoid"), h["lr"], h["lr"] * ratio,
                   None if optimizer == "sgd" else (0.9, 0.999, 1e-8, h["wd"]))
    return rec, W.detach().cpu(), b.detach().cpu()


@pytest.mark.parametrize("case", [c for c in CASES if c[4:6] == ("sgd", 1)], ids=str)
def test_one_sgd_step_is_fma_of_the_fp64_gradient(case):
    """A wrong step form (or sign, or lr) moves the weights by far more than the bound."""
    B, D, C, activation, optimizer, iters, seed = case
    W, b, x, y = inputs(B, D, C, seed)
    W64, b64 = W.double().requires_grad_(True), b.double().requires_grad_(True)
    a = x.double() @ W64.t() + b64
    torch.nn.functional.cross_entropy(torch.sigmoid(a) if activation == "sigmoid" else a, y).backward()
    alpha = float(np.float32(-HYPER["sgd"]["lr"]))
    out = train(case, True)
    for got, w, g in ((out[0], W, W64.grad), (out[1], b, b64.grad)):
        want = (alpha * g.float().double() + w.double()).float()  # one rounding: fma(-lr, g, w)
        assert float((got.cpu().double() - want.double()).abs().max()) <= BOUND["w"]


@pytest.mark.parametrize("nan, optimizer, ratio", [(True, "adam", RATIO), (False, "sgd", 1e-6)])
def test_a_nan_in_x_or_a_small_ratio_trips_at_epoch_0_and_leaves_the_parameters(nan, optimizer, ratio):
    W, b, x, y = inputs(17, 5, 10, 0)
    if nan:
        x[3, 2] = math.nan
    rec, W1, b1 = launch(W, b, x, y, iters=5, activation="none", optimizer=optimizer, ratio=ratio)
    assert rec[0] == 0 and rec[6] == 0
    assert torch.equal(W1.view(torch.int32), W.view(torch.int32)) and torch.equal(b1.view(torch.int32), b.view(torch.int32))


def test_an_overflow_trips_at_epoch_1_after_one_step():
    """W = 0 and one sample of magnitude 2e20 (its gradient's norm still fits fp32): the first step makes that
    sample's z overflow, so epoch 1's loss and gradients are NaN."""
    _, b, x, y = inputs(64, 32, 3, 0)
    W, x[0] = torch.zeros(3, 32), 2e20 * x[0].sign()
    ref = linear_loop_ref(W, b, x, y, iters=5, activation="none", optimizer="sgd", ratio=1e30, dtype=torch.float32,
                          **HYPER["sgd"])
    assert ref["trip"] == 1
    rec, W1, b1 = launch(W, b, x, y, iters=5, activation="none", optimizer="sgd", ratio=1e30)
    assert rec[0] == 1 and rec[6] == 1
    scale = float(ref["W"].abs().max())  # the weights are of the order 1e18: the bound is relative to that
    assert float((W1 - ref["W"]).abs().max()) <= BOUND["w"] * scale and float((b1 - ref["b"]).abs().max()) <= BOUND["w"]


def test_a_label_equal_to_c_raises_index_error_and_leaves_the_parameters():
    W, b, x, y = inputs(17, 5, 10, 0)
    y[5] = 10
    dev = torch.device("cuda", 0)
    net = Net(W, b, "none").to(dev)
    with pytest.raises(IndexError, match=r"outside \[0, 10\)"):
        client_stats.client_train(make_client(x.to(dev), y.to(dev), dev, "sgd", ratio=RATIO, **HYPER["sgd"]), net, 5,
                                  loop="linear")
    torch.cuda.synchronize()  # nothing faulted
    assert torch.equal(net.linear.weight.cpu().view(torch.int32), W.view(torch.int32))
    assert torch.equal(net.linear.bias.cpu().view(torch.int32), b.view(torch.int32))
