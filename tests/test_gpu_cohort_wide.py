"""A round's cohort at up to 128 classes and 4096 columns (``fedavg_client_cohort_wide_f32``,
``cohort_train(wide=True)``): every client against the loop of client.py:52-96 in fp64 torch on the CPU
(linear_loop_ref.py) at the shapes at which tiling over classes, columns and rows can go wrong; alone and in company,
bit for bit; one client's NaN or bad label touching no other.  Bounds: 4x the largest deviation from the same reference
of the existing fp32 path (``loop="torch"`` on the GPU, per client, same inputs).  W and b: largest
absolute difference; loss, beta, rho: relative difference."""
import functools
import math

import pytest
import torch

from linear_loop_ref import linear_loop_ref, make_client
from mfl_amd import ALIGN_ELEMS, _lib, client_stats, cohort_train
from mfl_amd.client_passes import adam_coef, wide_max_slices, wide_slice_rows, wide_workspace_bytes
from test_gpu_linear_stream import DEV, HYPER, RATIO, Net, deviations

pytestmark = pytest.mark.gpu

ITERS = 3
# the fp32 torch loop's largest deviations over CASES, every client (torch 2.10.0 / ROCm 7.0, MI355X), times 4.  The
# torch loop's figures are cut, not rounded up, to four digits.  The wide cohort's own largest over the same: w 2.864e-5,
# loss 1.018e-7, beta 3.698e-4, rho 1.363e-3.
BOUND = {"w": 4 * 1.494e-5, "loss": 4 * 1.342e-7, "beta": 4 * 1.763e-4, "rho": 4 * 1.536e-3}
# (D, C, [B_k] from R = wide_slice_rows(), x offset in floats, the cohort whose inputs it takes): four class tiles, the
# last one partial, with full, over and one-row slices; one past both older limits, the staged path (D % 4 != 0), one
# class alone in the second tile; one class tile and 24 panels; less than a panel and an odd tile count; the corner;
# the first again with every x 4 B off a 16-B boundary (the staged path on misaligned x)
SIZES = lambda R: [R, R + 1, 1, 2 * R + 1, 5 * R + 3]  # noqa: E731
COHORTS = [(784, 62, SIZES, 0, 0), (1025, 17, lambda R: [R - 1, 2 * R + 1], 0, 1),
           (3072, 10, lambda R: [R + 6, 3], 0, 2), (20, 33, lambda R: [1, 5, R + 1], 0, 3),
           (4096, 128, lambda R: [R - 1, 2 * R + 1], 0, 4), (784, 62, SIZES, 1, 0)]
# q = 2 (where C allows it) and q = 1 in turn
CASES = [(n, act, opt, 1 + (n + i + j) % 2) for n in range(len(COHORTS))
         for i, act in enumerate(("none", "sigmoid")) for j, opt in enumerate(("sgd", "adam"))]
SENTINEL = -7.25


@functools.lru_cache(maxsize=None)
def inputs(n):
    """(W, b, [(x, y)]) on the CPU, built as test_gpu_cohort_split.inputs builds them (a client of fewer than four rows
    a fifth of the others' scale) with x scaled by a further min(1, sqrt(784 / D))."""
    D, C, sizes, _, src = COHORTS[n]
    if src != n:
        return inputs(src)
    g = torch.Generator().manual_seed(100 * n + 7 * D + 13 * C)
    W, b = torch.randn(C, D, generator=g) / math.sqrt(D), torch.randn(C, generator=g)
    scale = min(1.0, math.sqrt(784 / D))
    return W, b, [((0.25 if B >= 4 else 0.05) * scale * torch.randn(B, D, generator=g),
                   torch.randint(0, C, (B,), generator=g)) for B in sizes(wide_slice_rows())]


def on_device(batches, offset=0):
    """The batches on the GPU, every x ``offset`` floats past a 16-B boundary."""
    out = []
    for x, y in batches:
        flat = torch.empty(x.numel() + offset, device=DEV)
        flat[offset:] = x.reshape(-1)
        out.append((flat[offset:].view(x.shape), y.to(DEV)))
    return out


@functools.lru_cache(maxsize=None)
def reference(n, k, activation, optimizer, iters=ITERS):
    W, b, batches = inputs(n)
    return linear_loop_ref(W, b, *batches[k], iters=iters, activation=activation, optimizer=optimizer, ratio=RATIO,
                           **HYPER[optimizer])


def train(W, b, batches, activation, optimizer, q, **kw):
    clients = [make_client(x, y, DEV, optimizer, ratio=RATIO, **HYPER[optimizer]) for x, y in batches]
    net = Net(W, b, activation).to(DEV)
    res = cohort_train(clients, net, ITERS, loop="linear_sigmoid" if activation == "sigmoid" else "linear", wide=True,
                       slices_per_group=q, **kw)
    assert torch.equal(net.linear.weight.cpu(), W) and torch.equal(net.linear.bias.cpu(), b)  # net is not modified
    return res


@pytest.mark.parametrize("case", CASES, ids=str)
def test_wide_cohort_matches_the_fp64_reference_per_client(case):
    n, activation, optimizer, q = case
    W, b, batches = inputs(n)
    res = train(W, b, on_device(batches, COHORTS[n][3]), activation, optimizer, min(q, wide_max_slices(W.shape[0])))
    assert res.P == W.numel() + b.numel() and res.sample_numbers == [x.shape[0] for x, _ in batches]
    for k in range(len(batches)):
        ref = reference(COHORTS[n][4], k, activation, optimizer)
        # what the inputs owe: no trip, and a loss far from 0 at every epoch, so that no relative bound is vacuous
        assert ref["trip"] == -1 and max(ref["guard_ratio"]) <= 0.5
        assert min(reference(COHORTS[n][4], k, activation, optimizer, it)["loss"] for it in range(1, ITERS + 1)) > 0.05
        sd, (loss, beta, rho, acc) = res.state_dict(k, cpu=True), res.results[k]
        dev = deviations((sd["1.weight"], sd["1.bias"], loss, beta, rho, None), ref)
        print(case, k, dev)  # each figure before it is held to its bound
        for name, bound in BOUND.items():
            assert dev[name] <= bound, (k, name, dev[name], bound)  # false for a NaN as well
        if ref["top2_gap"] > 1e-3:
            assert round(acc * batches[k][0].shape[0]) == ref["correct"], k


def entry(W, b, batches, optimizer, q, order):
    """The C entry on device batches, entry g = client order[g], row = the client's position: (rows incl. pad, records
    as int64, the 4096 bytes after the workspace, which no launch may touch)."""
    h, adam, K, P = HYPER[optimizer], optimizer == "adam", len(batches), W.numel() + b.numel()
    form = (client_stats.adam_form if adam else client_stats.sgd_form)(DEV, torch.float32)
    model = torch.cat([W.reshape(-1), b]).to(DEV)
    rows = torch.full((K, -(-P // ALIGN_ELEMS) * ALIGN_ELEMS), SENTINEL, device=DEV)
    table = torch.tensor([[batches[k][0].data_ptr(), batches[k][1].data_ptr(), batches[k][0].shape[0], k] for k in order]).pin_memory()
    rec = torch.zeros(K, 8, dtype=torch.float64, pin_memory=True)
    coef = torch.zeros(16, 7, dtype=torch.float64, pin_memory=True)
    for t in range(ITERS):
        coef[t] = torch.from_numpy(adam_coef(h["lr"], 0.9, 0.999, 1e-8, h["wd"], t + 1))
    nbytes = wide_workspace_bytes([batches[k][0].shape[0] for k in order], W.shape[1], W.shape[0], q, adam)
    ws = torch.full((nbytes + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    name = "fedavg_client_cohort_wide_f32"
    _lib.check_clientwide(getattr(_lib.load_clientwide(), name)(
        model.data_ptr(), rows.data_ptr(), rows.stride(0), table.data_ptr(), K, W.shape[1], W.shape[0], ITERS, 0,
        int(adam), h["lr"], h["lr"] * RATIO, form, coef.data_ptr(), rec.data_ptr(), q, ws.data_ptr(), nbytes, None), name)
    torch.cuda.synchronize()
    return rows.cpu().view(torch.int32), rec.view(torch.int64).clone(), ws[nbytes:].cpu()


@pytest.mark.parametrize("n, optimizer, q", [(0, "sgd", 2), (5, "adam", 1)])
def test_a_client_alone_and_in_company_leaves_the_same_bits(n, optimizer, q):
    W, b, batches = inputs(n)
    dev, K, P = on_device(batches, COHORTS[n][3]), len(batches), W.numel() + b.numel()
    rows, rec, tail = entry(W, b, dev, optimizer, q, list(range(K)))
    assert bool((rows[:, P:] == torch.tensor(SENTINEL).view(torch.int32)).all()) and bool((tail == 0xA5).all())
    assert rec.view(torch.float64)[:, 6].tolist() == [ITERS] * K
    for other in (entry(W, b, dev, optimizer, q, list(range(K))), entry(W, b, dev, optimizer, q, list(range(K))[::-1])):
        assert torch.equal(rows, other[0]) and torch.equal(rec, other[1])  # a second call; the table reversed
        assert bool((other[2] == 0xA5).all())
    for k in range(K):
        solo = entry(W, b, dev[k:k + 1], optimizer, q, [0])
        assert torch.equal(rows[k, :P], solo[0][0, :P]) and torch.equal(rec[k], solo[1][0]), k


def test_one_clients_trouble_stays_its_own():
    W, b, batches = inputs(0)
    R, dev, P = wide_slice_rows(), on_device(batches), W.numel() + b.numel()
    clean = entry(W, b, dev, "adam", 1, [4, 3, 2, 1, 0])
    dev[1][0][R, 5] = math.nan  # client 1's last row
    dev[3][1][R + 2] = 62       # C = 62, in client 3's second slice
    rows, rec, tail = entry(W, b, dev, "adam", 1, [4, 3, 2, 1, 0])
    model, fields = torch.cat([W.reshape(-1), b]).view(torch.int32), rec.view(torch.float64)
    assert fields[1].tolist()[:1] + fields[1].tolist()[5:] == [0, 0, 0, 0] and torch.equal(rows[1, :P], model)
    assert fields[3].tolist() == [-1, 0, 0, 0, 0, 1, 0, 0] and torch.equal(rows[3, :P], model)
    for k in (0, 2, 4):
        assert torch.equal(rows[k], clean[0][k]) and torch.equal(rec[k], clean[1][k]), k
    assert bool((tail == 0xA5).all())
    with pytest.raises(IndexError, match=r"client 3: a label lies outside \[0, 62\)"):
        train(W, b, dev, "none", "adam", 1)
    torch.cuda.synchronize()  # nothing faulted
