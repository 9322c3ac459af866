"""client.py:52-96 for a client whose model is one affine layer (``sigmoid``
after it for FedML's LogisticRegression) under a cross-entropy loss, in plain
torch with autograd on the CPU: fp64 by default, the reference the fused loop
is held against; and the stand-in for the reference's Client that the tests hand to client_train."""
import sys
import time
import types

import torch


def make_client(x, y, dev, optimizer, lr, wd, ratio, criterion=None):
    """What client_train reads of the reference's Client and of its module."""
    name = f"_linear_loop_client_{ratio}"
    if name not in sys.modules:
        mod = sys.modules[name] = types.ModuleType(name)
        mod.count = mod.count_end = time.perf_counter_ns
        mod.THRESHOLD_GRADS_RATIO = ratio
        mod.Client = type("Client", (), {"__module__": name})
    c = sys.modules[name].Client()
    c.local_training_data, c.device, c.criterion = [(x, y)], dev, criterion or torch.nn.CrossEntropyLoss().to(dev)
    c.args = types.SimpleNamespace(client_optimizer=optimizer, clip=10.0, lr=lr, wd=wd)
    return c


def linear_loop_ref(W, b, x, y, *, iters, activation, optimizer, lr, wd, ratio, dtype=torch.float64):
    W, b = (t.detach().cpu().to(dtype).clone().requires_grad_(True) for t in (W, b))
    x, y = x.detach().cpu().to(dtype).flatten(1), y.cpu()
    opt = torch.optim.SGD([W, b], lr=lr) if optimizer == "sgd" else \
        torch.optim.Adam([W, b], lr=lr, weight_decay=wd, amsgrad=True)
    flat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts]).clone()  # noqa: E731

    def forward():
        a = x @ W.t() + b
        a = torch.sigmoid(a) if activation == "sigmoid" else a
        return a, torch.nn.functional.cross_entropy(a, y)

    last_w = flat([W, b])
    _, last_loss = forward()
    last_loss.backward()
    last_loss, last_g = last_loss.item(), flat([W.grad, b.grad])
    out = dict(trip=-1, loss=None, beta=None, rho=None, guard_ratio=[])
    for epoch in range(iters):
        opt.zero_grad()
        a, loss = forward()
        loss.backward()
        g = flat([W.grad, b.grad])
        bound = lr * ratio * last_w.norm()
        out["guard_ratio"].append((g.norm() / bound).item())  # norm(g) over the :71 bound
        if torch.isnan(g).sum() > 0 or torch.isnan(loss) or g.norm() > bound:
            out["trip"] = epoch
            break
        opt.step()
        loss, w = loss.item(), flat([W, b])
        rho_tmp = abs(loss - last_loss) / (w - last_w).norm()
        out["rho"] = rho_tmp if not out["rho"] or rho_tmp > out["rho"] else out["rho"]
        beta_tmp = (g - last_g).norm() / (w - last_w).norm()
        out["beta"] = beta_tmp if not out["beta"] or beta_tmp > out["beta"] else out["beta"]
        last_loss, last_w, last_g = loss, w, g
        top = a.detach().topk(2).values
        out.update(loss=loss, correct=int((a.argmax(-1) == y).sum()), top2_gap=float((top[:, 0] - top[:, 1]).min()))
    out.update(W=W.detach(), b=b.detach(), beta=None if out["beta"] is None else float(out["beta"]),
               rho=None if out["rho"] is None else float(out["rho"]))
    return out
