"""central_train's chain of steps in one launch (``fedavg_client_chain_f32``, ``chain_train``, ``central_train``): against
the loop of fedavg_trainer.py:361-371 in fp64 torch on the CPU; against ``fedavg_client_linear_stream_f32`` with one
iteration per step, bit for bit; across the cuts into launches, bit for bit; a bad label; and ``central_train`` on a
stand-in trainer.  The fp64 bounds are 4x the largest deviation from the same reference of the same loop in fp32 torch
on the GPU over the same CASES, per optimizer, the margin the three earlier linear kernels were given for a different
but fixed summation order.  W and b: largest absolute difference; the per-round losses: largest relative difference."""
import functools
import math

import pytest
import torch

from mfl_amd import _lib, central_train, chain_train, client_stats
from mfl_amd.client_passes import adam_coef_rows
from test_gpu_linear_stream import DEV, HYPER, entry

pytestmark = pytest.mark.gpu

ROUNDS = 3
# the fp32 torch loop's largest deviations over the optimizer's CASES (torch 2.10 / ROCm 7.0, MI355X), times 4.  Adam's
# W figure is one case's, (3, "sigmoid", "adam"): where a gradient element is of the size of its own rounding error
# Adam's first steps move the weight by up to lr whatever the size, on the torch path (2.298e-5) as on this one
# (7.753e-6); the largest of Adam's other cases is 4.502e-7 on both paths.
BOUND = {"sgd": {"w": 4 * 4.045e-7, "loss": 4 * 1.210e-7}, "adam": {"w": 4 * 2.298e-5, "loss": 4 * 1.584e-7}}
# (D, C, [B_k], x offset in floats): R = 16 / 64 / 32 with one-group clients around many-group ones and a one-row
# client, the range's corner, the staged path (D % 4 != 0, and D % 4 == 0 with every x 4 B off), the batch that stays
COHORTS = [(784, 10, [16, 17, 1, 33, 100], 0), (252, 16, [64, 65, 1, 129], 0), (512, 3, [32, 33, 31, 96], 0),
           (1024, 16, [15, 49], 0), (7, 2, [1, 1, 5], 0), (250, 5, [70, 3], 0), (784, 10, [16, 17, 1, 33, 100], 1),
           (784, 10, [40], 0)]
CASES = [(n, act, opt) for n in range(len(COHORTS)) for act in ("none", "sigmoid") for opt in ("sgd", "adam")]


@functools.lru_cache(maxsize=None)
def inputs(n):
    """(W, b, [(x, y)]) on the CPU; x is scaled so that no logit saturates in fp32."""
    D, C, Bs, _ = COHORTS[n]
    g = torch.Generator().manual_seed(100 * n + 7 * D + 13 * C)
    W, b = torch.randn(C, D, generator=g) / math.sqrt(D), torch.randn(C, generator=g)
    return W, b, [(0.25 * torch.randn(B, D, generator=g), torch.randint(0, C, (B,), generator=g)) for B in Bs]


def Net(W, b, activation):
    linear = torch.nn.Linear(W.shape[1], W.shape[0])
    linear.weight.data, linear.bias.data = W.clone(), b.clone()
    return torch.nn.Sequential(torch.nn.Flatten(), linear, torch.nn.Sigmoid() if activation == "sigmoid" else torch.nn.Identity())


def on_device(n):
    """The cohort's batches on the GPU, every x ``offset`` floats past a 16-B boundary."""
    off, out = COHORTS[n][3], []
    for x, y in inputs(n)[2]:
        flat = torch.empty(x.numel() + off, device=DEV)
        flat[off:] = x.reshape(-1)
        out.append((flat[off:].view(x.shape), y.to(DEV)))
    return out


def torch_chain(net, batches, optimizer, rounds):
    """One step of ``net`` per batch, round after round, with torch's optimizer: (W, b, per-round losses)."""
    h, crit = HYPER[optimizer], torch.nn.CrossEntropyLoss()
    opt = torch.optim.SGD(net.parameters(), lr=h["lr"]) if optimizer == "sgd" else \
        torch.optim.Adam(net.parameters(), lr=h["lr"], weight_decay=h["wd"], amsgrad=True)
    p, losses = next(net.parameters()), []
    for _ in range(rounds):
        for x, y in batches:
            net.zero_grad()
            loss = crit(net(x.to(p)), y.to(p.device))
            loss.backward()
            opt.step()
        losses.append(loss.item())
    return [q.detach().cpu().double() for q in net.parameters()] + [losses]


@functools.lru_cache(maxsize=None)
def reference(case):
    n, activation, optimizer = case
    W, b, batches = inputs(n)
    return torch_chain(Net(W, b, activation).double(), batches, optimizer, ROUNDS)


def deviations(out, ref):
    return {"w": max(float((out[0] - ref[0]).abs().max()), float((out[1] - ref[1]).abs().max())),
            "loss": max(abs(a - r) / r for a, r in zip(out[2], ref[2]))}


def train(n, activation, optimizer, rounds=ROUNDS, batches=None, **kw):
    """``chain_train`` on the GPU: (W, b, losses), W and b on the CPU."""
    W, b, _ = inputs(n)
    net = Net(W, b, activation).to(DEV)
    losses = chain_train(net, batches or on_device(n), rounds, optimizer=optimizer, **HYPER[optimizer],
                         loop="linear_sigmoid" if activation == "sigmoid" else "linear", **kw)
    return net[1].weight.detach().cpu(), net[1].bias.detach().cpu(), losses


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("case", CASES, ids=str)
def test_chain_train_matches_the_fp64_reference(case):
    ref = reference(case)
    assert min(ref[2]) > 0.05  # what the inputs owe: a loss far from 0, so that its relative bound binds
    out = train(*case)
    dev = deviations((out[0].double(), out[1].double(), out[2]), ref)
    print(case, dev)  # each figure before it is held to its bound
    for k, bound in BOUND[case[2]].items():
        assert dev[k] <= bound, (k, dev[k], bound)  # false for a NaN as well


def chain_entry(n, activation, optimizer, rounds, batches, model=None, state=None, step0=0, beta1=0.9):
    """The C entry on device batches: (rc, model, state, losses, rec); ``beta1``: the coefficient rows'."""
    D, C, _, _ = COHORTS[n]
    W, b, _ = inputs(n)
    h, adam, K = HYPER[optimizer], optimizer == "adam", len(batches)
    form = (client_stats.adam_form if adam else client_stats.sgd_form)(DEV, torch.float32)
    model = torch.cat([W.reshape(-1), b]).to(DEV) if model is None else model
    state = torch.zeros(3 * model.numel(), device=DEV) if state is None else state
    table = torch.tensor([[x.data_ptr(), y.data_ptr(), x.shape[0], 0] for x, y in batches]).pin_memory()
    coef = torch.from_numpy(adam_coef_rows(h["lr"], beta1, 0.999, 1e-8, h["wd"], step0 + 1, rounds * K)).pin_memory()
    losses, rec = torch.zeros(rounds, dtype=torch.float64, pin_memory=True), torch.zeros(8, dtype=torch.float64).pin_memory()
    rc = _lib.load_clientchain().fedavg_client_chain_f32(
        model.data_ptr(), state.data_ptr() if adam else None, table.data_ptr(), K, D, C, rounds, step0,
        int(activation == "sigmoid"), int(adam), h["lr"], form, coef.data_ptr() if adam else None, losses.data_ptr(),
        rec.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, model, state, losses, rec


@pytest.mark.parametrize("n, activation, optimizer", CASES)
def test_every_step_has_the_bits_of_the_streamed_entry_with_one_iteration(n, activation, optimizer):
    D, C, _, _ = COHORTS[n]
    W, b, _ = inputs(n)
    # SGD: two rounds over the cohort; Adam (a fresh optimizer per streamed call): the last client alone, one round
    batches, rounds = (on_device(n), 2) if optimizer == "sgd" else (on_device(n)[-1:], 1)
    rc, model, _, losses, rec = chain_entry(n, activation, optimizer, rounds, batches)
    assert rc == 0 and rec.tolist() == [0, -1, rounds * len(batches), losses[-1].item(), 0, 0, 0, 0]
    for _ in range(rounds):
        for x, y in batches:
            w, bb, r = entry("fedavg_client_linear_stream_f32", W, b, x, y, activation, optimizer, 1)
            assert r.view(torch.float64)[0] == -1 and r.view(torch.float64)[6] == 1  # no guard tripped: one step
            W, b = w.view(torch.float32).view(C, D), bb.view(torch.float32)
    assert torch.equal(bits(model.cpu()), bits(torch.cat([W.reshape(-1), b])))
    assert torch.equal(rec[3:4].view(torch.int64), r[1:2])  # the last loss is that call's


@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
def test_the_cut_into_launches_changes_no_bit_and_the_order_of_the_clients_does(optimizer):
    whole, again = train(0, "none", optimizer, per_launch=ROUNDS), train(0, "none", optimizer, per_launch=ROUNDS)
    by_one, default = train(0, "none", optimizer, per_launch=1), train(0, "none", optimizer)
    for other in (again, by_one, default):
        assert torch.equal(bits(whole[0]), bits(other[0])) and torch.equal(bits(whole[1]), bits(other[1]))
        assert whole[2] == other[2]
    batches = on_device(0)
    batches[1], batches[3] = batches[3], batches[1]  # a kernel that walked an order of its own would not notice
    swapped = train(0, "none", optimizer, batches=batches)
    assert not torch.equal(bits(whole[0]), bits(swapped[0]))


def test_a_bad_label_is_reported_with_its_entry_and_nothing_is_touched():
    W, b, _ = inputs(4)
    batches = on_device(4)
    batches[1][1][0] = 2  # C = 2
    batches[2][1][4] = -1
    model, state = torch.cat([W.reshape(-1), b]).to(DEV), torch.full((3 * 16,), -7.25, device=DEV)
    rc, m, s, _, rec = chain_entry(4, "none", "adam", 2, batches, model.clone(), state.clone(), step0=5)
    assert rc == 0 and rec.tolist() == [1, 1, 0, 0, 0, 0, 0, 0]
    assert torch.equal(bits(m), bits(model)) and torch.equal(bits(s), bits(state))
    with pytest.raises(IndexError, match=r"client 1: a label lies outside \[0, 2\)"):
        train(4, "none", "sgd", batches=batches)
    torch.cuda.synchronize()  # nothing faulted


def test_a_pinned_coefficient_row_of_the_other_lerp_branch_is_refused_before_the_launch():
    model = torch.cat([t.reshape(-1) for t in inputs(4)[:2]]).to(DEV)
    rc, m, _, _, _ = chain_entry(4, "none", "adam", 1, on_device(4), model.clone(), beta1=0.4)
    assert rc == _lib.FEDAVG_EMODE and b"1 - beta1 = 0.6" in _lib.load_clientchain().fedavg_clientchain_last_error()
    assert torch.equal(bits(m), bits(model))


class wandb:  # central_train logs to the ``wandb`` of the module that defines the trainer's class
    logged = []
    log = logged.append


class Trainer:
    """What central_train reads of a FedAvgTrainer: 5 clients, 2 central rounds."""

    def __init__(self, optimizer):
        self.args = type("Args", (), dict(model="lr", central_round=2, client_optimizer=optimizer, **HYPER[optimizer]))
        self.device, self.class_num, self.batches = DEV, COHORTS[0][1], inputs(0)[2]
        self.client_num = len(self.batches)
        self.train_data_local_dict = {k: [batch] for k, batch in enumerate(self.batches)}

    def model(self, args, model_name, output_dim):
        return torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(COHORTS[0][0], output_dim))


@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
def test_central_train_on_a_stand_in_trainer(optimizer):
    trainer, wandb.logged[:] = Trainer(optimizer), []
    torch.manual_seed(5)
    w_optimal, loss_optimal = central_train(trainer)
    torch.manual_seed(5)  # the same initial model for the fp32 torch loop
    net = trainer.model(trainer.args, model_name="lr", output_dim=trainer.class_num).to(DEV)
    W, b, losses = torch_chain(net, trainer.batches, optimizer, 2)
    assert w_optimal.device == DEV and w_optimal.shape == (W.numel() + b.numel(),)
    dev = deviations((w_optimal.detach().cpu().double(), b, [loss_optimal]), (torch.cat([W.reshape(-1), b]), b, losses[-1:]))
    print(optimizer, dev)
    assert dev["w"] <= BOUND[optimizer]["w"] and dev["loss"] <= BOUND[optimizer]["loss"]
    assert [list(d) for d in wandb.logged] == [["central_training/loss"]] * 2 and wandb.logged[1]["central_training/loss"] == loss_optimal
