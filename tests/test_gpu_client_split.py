"""The chain with each step's batch split across workgroups (``fedavg_client_chain_split_f32``, ``split=True``): against
the loop of fedavg_trainer.py:361-371 in fp64 torch on the CPU at the batch sizes at which slicing can go wrong; across
the cuts into calls, bit for bit; a bad label; ``central_train``.  Bounds and measures: test_gpu_client_chain.py's rule
(DESIGN.md §3), 4x the fp32 torch loop's largest deviation on the GPU over this file's CASES, per optimizer."""
import functools
import math

import pytest
import torch

from mfl_amd import _lib, central_train, chain_train, client_stats
from mfl_amd.client_passes import adam_coef_rows, split_slice_rows
from test_gpu_client_chain import Net, Trainer, bits, deviations, torch_chain, wandb
from test_gpu_linear_stream import DEV, HYPER

pytestmark = pytest.mark.gpu

ROUNDS = 3
# the fp32 torch loop's largest deviations over the optimizer's CASES (torch 2.10.0 / ROCm 7.0, MI355X), times 4.  The
# split path's own largest over the same CASES: SGD 3.779e-7 / 7.536e-8, Adam 4.904e-7 / 8.599e-8.
BOUND = {"sgd": {"w": 4 * 3.779e-7, "loss": 4 * 1.098e-7}, "adam": {"w": 4 * 9.103e-7, "loss": 4 * 1.298e-7}}
# (D, C, [B_k] from R = split_slice_rows(D), x offset in floats): slices full, one row over or short, a one-row client,
# many slices; the range's corner; one partial slice; the staged path (D % 4 != 0; every x 4 B off a 16-B boundary)
COHORTS = [(784, 10, lambda R: [R, R + 1, 1, 2 * R + 1, 5 * R + 3], 0), (252, 16, lambda R: [R - 1, 2 * R, 1, 3 * R + 1], 0),
           (512, 3, lambda R: [R, R + 1, 4 * R - 1], 0), (1024, 16, lambda R: [R - 1, 2 * R + 1], 0),
           (7, 2, lambda R: [1, 1, 5], 0), (250, 5, lambda R: [R + 6, 3], 0),
           (784, 10, lambda R: [R, R + 1, 1, 2 * R + 1, 5 * R + 3], 1)]
CASES = [(n, act, opt) for n in range(len(COHORTS)) for act in ("none", "sigmoid") for opt in ("sgd", "adam")]


@functools.lru_cache(maxsize=None)
def inputs(n):
    """(W, b, [(x, y)]) on the CPU, as test_gpu_client_chain.inputs draws them."""
    D, C, sizes, _ = COHORTS[n]
    g = torch.Generator().manual_seed(100 * n + 7 * D + 13 * C)
    W, b = torch.randn(C, D, generator=g) / math.sqrt(D), torch.randn(C, generator=g)
    return W, b, [(0.25 * torch.randn(B, D, generator=g), torch.randint(0, C, (B,), generator=g))
                  for B in sizes(split_slice_rows(D))]


def on_device(n):
    """The cohort's batches on the GPU, every x ``offset`` floats past a 16-B boundary."""
    off, out = COHORTS[n][3], []
    for x, y in inputs(n)[2]:
        flat = torch.empty(x.numel() + off, device=DEV)
        flat[off:] = x.reshape(-1)
        out.append((flat[off:].view(x.shape), y.to(DEV)))
    return out


@functools.lru_cache(maxsize=None)
def reference(case):
    W, b, batches = inputs(case[0])
    return torch_chain(Net(W, b, case[1]).double(), batches, case[2], ROUNDS)


def train(n, activation, optimizer, batches=None, **kw):
    """``chain_train(split=True)`` on the GPU: (W, b, losses), W and b on the CPU."""
    W, b, _ = inputs(n)
    net = Net(W, b, activation).to(DEV)
    losses = chain_train(net, batches or on_device(n), ROUNDS, optimizer=optimizer, **HYPER[optimizer], split=True,
                         loop="linear_sigmoid" if activation == "sigmoid" else "linear", **kw)
    return net[1].weight.detach().cpu(), net[1].bias.detach().cpu(), losses


@pytest.mark.parametrize("case", CASES, ids=str)
def test_split_chain_matches_the_fp64_reference(case):
    ref = reference(case)
    assert min(ref[2]) > 0.05  # what the inputs owe: a loss far from 0, so that its relative bound binds
    out = train(*case)
    dev = deviations((out[0].double(), out[1].double(), out[2]), ref)
    print(case, dev)  # each figure before it is held to its bound
    for k, bound in BOUND[case[2]].items():
        assert dev[k] <= bound, (k, dev[k], bound)  # false for a NaN as well


def split_entry(n, activation, optimizer, rounds, batches, model=None, state=None, step0=0):
    """The C entry on device batches: (rc, model, state, losses, rec, the 4096 bytes after the workspace, which no launch may touch)."""
    D, C = COHORTS[n][:2]
    W, b, _ = inputs(n)
    h, adam, K = HYPER[optimizer], optimizer == "adam", len(batches)
    form = (client_stats.adam_form if adam else client_stats.sgd_form)(DEV, torch.float32)
    model = torch.cat([W.reshape(-1), b]).to(DEV) if model is None else model
    state = torch.zeros(3 * model.numel(), device=DEV) if state is None else state
    table = torch.tensor([[x.data_ptr(), y.data_ptr(), x.shape[0], 0] for x, y in batches]).pin_memory()
    coef = torch.from_numpy(adam_coef_rows(h["lr"], 0.9, 0.999, 1e-8, h["wd"], step0 + 1, rounds * K)).pin_memory()
    losses, rec = torch.zeros(rounds, dtype=torch.float64, pin_memory=True), torch.zeros(8, dtype=torch.float64).pin_memory()
    lib = _lib.load_clientsplit()
    nbytes = lib.fedavg_client_split_workspace_bytes(max(x.shape[0] for x, _ in batches), D, C)
    ws = torch.full((nbytes + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    rc = lib.fedavg_client_chain_split_f32(
        model.data_ptr(), state.data_ptr() if adam else None, table.data_ptr(), K, D, C, rounds, step0,
        int(activation == "sigmoid"), int(adam), h["lr"], form, coef.data_ptr() if adam else None, losses.data_ptr(),
        rec.data_ptr(), ws.data_ptr(), nbytes, None)
    torch.cuda.synchronize()
    return rc, model, state, losses, rec, ws[nbytes:].cpu()


@pytest.mark.parametrize("n", [0, len(COHORTS) - 1])
@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
def test_the_cut_into_calls_changes_no_bit(n, optimizer):
    batches, K = on_device(n), len(inputs(n)[2])
    rc, model, state, losses, rec, tail = split_entry(n, "none", optimizer, ROUNDS, batches)
    assert rc == 0 and rec.tolist() == [0, -1, ROUNDS * K, losses[-1].item(), 0, 0, 0, 0] and bool((tail == 0xA5).all())
    m, s, cut = None, None, []
    for r in range(ROUNDS):  # a call per round: step0, the state and the coefficient rows carried
        rc, m, s, one, _, _ = split_entry(n, "none", optimizer, 1, batches, m, s, step0=r * K)
        assert rc == 0
        cut.append(one.item())
    assert torch.equal(bits(m), bits(model)) and torch.equal(bits(s), bits(state)) and cut == losses.tolist()
    P0 = model.numel() - COHORTS[n][1]
    for kw in (dict(per_launch=1), dict()):
        W, b, ls = train(n, "none", optimizer, **kw)
        assert torch.equal(bits(W).reshape(-1), bits(model[:P0].cpu())) and torch.equal(bits(b), bits(model[P0:].cpu()))
        assert ls == losses.tolist()


def test_a_bad_label_is_reported_with_its_entry_and_nothing_is_touched():
    W, b, _ = inputs(0)
    R, batches = split_slice_rows(COHORTS[0][0]), on_device(0)
    batches[2][1][0] = 10  # C = 10: the third entry's one row, and the second slice of the entry after it
    batches[3][1][R + 2] = 10
    model, state = torch.cat([W.reshape(-1), b]).to(DEV), torch.full((3 * 7850,), -7.25, device=DEV)
    rc, m, s, _, rec, tail = split_entry(0, "none", "adam", 2, batches, model.clone(), state.clone(), step0=5)
    assert rc == 0 and rec.tolist() == [1, 2, 0, 0, 0, 0, 0, 0]
    assert torch.equal(bits(m), bits(model)) and torch.equal(bits(s), bits(state)) and bool((tail == 0xA5).all())
    with pytest.raises(IndexError, match=r"client 2: a label lies outside \[0, 10\)"):
        train(0, "none", "sgd", batches=batches)
    torch.cuda.synchronize()  # nothing faulted


@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
def test_central_train_split_has_the_bits_of_chain_train_split(optimizer):
    trainer, wandb.logged[:] = Trainer(optimizer), []
    torch.manual_seed(5)
    w_optimal, loss_optimal = central_train(trainer, split=True)
    torch.manual_seed(5)  # the same initial model
    net = trainer.model(trainer.args, model_name="lr", output_dim=trainer.class_num).to(DEV)
    losses = chain_train(net, [(x.to(DEV), y.to(DEV)) for x, y in trainer.batches], 2, optimizer=optimizer,
                         **HYPER[optimizer], split=True)
    assert torch.equal(bits(w_optimal), bits(torch.cat([p.detach().view(-1) for p in net.parameters()])))
    assert [d["central_training/loss"] for d in wandb.logged] == losses and loss_optimal == losses[-1]
