"""The streamed local loop of a linear softmax client (``client_train(loop="linear" / "linear_sigmoid")`` with more
than 64 samples, ``fedavg_client_linear_stream_f32``) against the loop of client.py:52-96 in fp64 torch on the CPU
(linear_loop_ref.py), and against ``fedavg_client_linear_loop_f32`` bit for bit where both entries accept the shape.
The bounds are 4x the largest deviation from the fp64 reference of the existing fp32 path (``loop="torch"`` on the
GPU) over the same cases, as in test_gpu_linear_loop.py.  W and b: largest absolute difference; loss,
beta, rho: relative difference."""
import functools
import math

import pytest
import torch

from linear_loop_ref import linear_loop_ref, make_client
from mfl_amd import _lib, client_stats
from mfl_amd.client_passes import _LinearLoop, adam_coef

pytestmark = pytest.mark.gpu

# the existing path's largest deviations over CASES (torch 2.10 / ROCm 7.0, MI355X), times 4
BOUND = {"w": 4 * 2.913e-7, "loss": 4 * 5.987e-8, "beta": 4 * 1.971e-5, "rho": 4 * 9.065e-4}
RATIO = 1e4
HYPER = {"sgd": dict(lr=0.05, wd=0.0), "adam": dict(lr=0.001, wd=0.001)}
# (B, D, C, activation, optimizer, local_iteration, seed).  Rows per group: 64 for D <= 252, 32 for D <= 512, else 16:
# a last group of one row, exact multiples, the scalar path (D % 4 != 0), each group size at its D edge, many groups
CASES = [
    (65, 784, 10, "sigmoid", "adam", 5, 0), (65, 5, 2, "none", "sgd", 1, 0), (80, 784, 10, "none", "sgd", 5, 0),
    (81, 1024, 16, "sigmoid", "sgd", 5, 2), (97, 1024, 16, "none", "adam", 5, 0), (100, 300, 10, "sigmoid", "adam", 1, 3),
    (128, 3, 16, "none", "sgd", 5, 0), (129, 4, 10, "sigmoid", "adam", 5, 1), (129, 252, 2, "none", "sgd", 5, 0),
    (193, 508, 16, "sigmoid", "sgd", 1, 16), (255, 784, 10, "none", "adam", 5, 0),
    (1000, 784, 10, "sigmoid", "adam", 5, 15), (1000, 784, 10, "none", "sgd", 5, 1),
]
DEV = torch.device("cuda", 0)


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
    net = Net(W, b, activation).to(DEV)
    kw = dict(loop="linear_sigmoid" if activation == "sigmoid" else "linear") if loop else {}
    client = make_client(x.to(DEV), y.to(DEV), DEV, optimizer, ratio=RATIO, **HYPER[optimizer])
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
def test_streamed_loop_matches_the_fp64_reference(case):
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


def entry(name, W, b, x, y, activation, optimizer, iters):
    """One C entry of the two on device copies of the inputs: (w bits, b bits, the record)."""
    lib, check = {"fedavg_client_linear_loop_f32": (_lib.load_clientlinear(), _lib.check_clientlinear),
                  "fedavg_client_linear_stream_f32": (_lib.load_clientstream(), _lib.check_clientstream)}[name]
    h = HYPER[optimizer]
    form = (client_stats.sgd_form if optimizer == "sgd" else client_stats.adam_form)(DEV, torch.float32)
    W, b, x, y = (t.to(DEV) for t in (W, b, x, y))
    rec = torch.zeros(8, dtype=torch.float64, pin_memory=True)
    coef = torch.zeros(16, 7, dtype=torch.float64, pin_memory=True)
    for t in range(iters):
        coef[t] = torch.from_numpy(adam_coef(h["lr"], 0.9, 0.999, 1e-8, h["wd"], t + 1))
    check(getattr(lib, name)(W.data_ptr(), b.data_ptr(), x.data_ptr(), y.data_ptr(), *x.shape, W.shape[0], iters,
                             int(activation == "sigmoid"), int(optimizer == "adam"), h["lr"], h["lr"] * RATIO, form,
                             coef.data_ptr(), rec.data_ptr(), None), name)
    torch.cuda.synchronize()
    return W.cpu().view(torch.int32), b.cpu().view(torch.int32), rec.view(torch.int64).clone()


@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
@pytest.mark.parametrize("activation", ["none", "sigmoid"])
@pytest.mark.parametrize("B, D, C", [(1, 1, 2), (17, 5, 16), (33, 784, 10), (64, 1024, 16), (64, 252, 2)])
def test_both_entries_leave_the_same_bits_where_both_accept_the_shape(B, D, C, activation, optimizer):
    args = (*inputs(B, D, C, 0), activation, optimizer, 3)
    old, new = entry("fedavg_client_linear_loop_f32", *args), entry("fedavg_client_linear_stream_f32", *args)
    assert old[2].view(torch.float64)[6] == 3  # three steps were taken
    assert all(torch.equal(p, q) for p, q in zip(old, new))


def test_a_nan_in_the_last_group_trips_at_epoch_0_and_leaves_the_parameters():
    W, b, x, y = inputs(81, 5, 10, 0)
    x[80, 2] = math.nan
    Wd, bd = W.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    plan = _LinearLoop([Wd, bd], x.to(DEV), y.to(DEV), torch.nn.CrossEntropyLoss(),
                       lambda d: client_stats.adam_form(d, torch.float32))
    rec = plan.run(5, 0, HYPER["adam"]["lr"], HYPER["adam"]["lr"] * RATIO, (0.9, 0.999, 1e-8, HYPER["adam"]["wd"]))
    assert rec[0] == 0 and rec[6] == 0
    assert torch.equal(Wd.detach().cpu().view(torch.int32), W.view(torch.int32))
    assert torch.equal(bd.detach().cpu().view(torch.int32), b.view(torch.int32))


def test_a_label_equal_to_c_at_the_last_row_raises_index_error_and_leaves_the_parameters():
    W, b, x, y = inputs(81, 5, 10, 0)
    y[80] = 10
    net = Net(W, b, "none").to(DEV)
    with pytest.raises(IndexError, match=r"outside \[0, 10\)"):
        client_stats.client_train(make_client(x.to(DEV), y.to(DEV), DEV, "sgd", ratio=RATIO, **HYPER["sgd"]), net, 5,
                                  loop="linear")
    torch.cuda.synchronize()  # nothing faulted
    assert torch.equal(net.linear.weight.cpu().view(torch.int32), W.view(torch.int32))
    assert torch.equal(net.linear.bias.cpu().view(torch.int32), b.view(torch.int32))
