"""The client's per-iteration statistics (``Client.train``, client.py:52-86) on the GPU.

Next to forward and backward the reference's local loop flattens the
gradients and the weights every iteration (``torch.cat``, :69, :76), tests
them (:71: NaN count, ``norm(grads)`` against ``lr * ratio * norm(last_w)``)
and tracks ``rho`` and ``beta`` (:78-84) from ``norm(w - last_w)`` and
``norm(grads - last_grads)``: about a dozen passes over the model and six to
eight blocking tensor truth tests.  :class:`ClientStepStats` does the same
bookkeeping with one fused pass over the gradients and one over the weights
(``fedavg_client_stats_f32``: NaN count, sum of squares, squared distance to
the previous step's snapshot, snapshot update) and keeps rho / beta on the
device (``fedavg_client_track``), with ONE host sync per local iteration (the
:71 guard, which decides whether the optimizer steps).

The norms are fl32(sqrt()) of fp64 sums of exact squares, i.e. the exactly
rounded values of what the reference's fp32 ``torch.norm`` approximates; rho
and beta then follow in the reference's fp32 arithmetic.

The dtype rule: the fused pass takes parameters that are all contiguous, on
one GPU and all of ONE dtype among fp32, bf16, fp16 and fp64.  bf16, fp16 and
fp64 models go through ``libfedavg_amd_clientvec.so``
(``fedavg_client_stats_{bf16,f16,f64}`` / ``fedavg_client_track_{bf16,f16,f64}``):
snapshots in the model's own type, the difference formed in that type, norms
``rT(fl32(sqrt()))`` (fp64: ``sqrt()``) and every scalar operation after them
as ATen does it, in opmath and then rounded once to the type.

``stats="torch"`` computes the same quantities with the reference's own torch
expressions on whatever device the parameters are on; it is what CPU
parameters, models of mixed dtypes and any other dtype get under
``stats="auto"``.

``step="fused"`` (opt in; the default ``"torch"`` is ``optimizer.step()`` and
the weight pass above) replaces the plain SGD step of :74 and the weight pass
by ONE kernel (``libfedavg_amd_clientstep.so``, ``fedavg_client_sgd_step_*``):
it reads ``w`` and ``g``, writes ``w' = w - lr * g`` and sums ``w'^2`` and
``rT(w' - w)^2`` on the way, since ``last_w`` of :78 is always the weight the
step started from.  No weight snapshot is read or written: 12 B per fp32
element instead of 24.  The bits it leaves must be torch's, and whether ATen's
kernel fuses the multiply and the add is a property of the torch build:
:func:`sgd_form` finds out on the GPU, once per (device, dtype).

``optimizer="adam"`` with fused stepping does the same for the reference's
default optimizer, ``torch.optim.Adam(lr, weight_decay=wd, amsgrad=True)``
(``libfedavg_amd_clientadam.so``, ``fedavg_client_adam_step_*``): one kernel
reads ``w``, ``g`` and the state ``m, v, vmax`` and writes ``w, m, v, vmax``
where torch's multi-tensor Adam makes nine launches.  Four of its operations
have the shape ``x + s * y``; which of them torch's kernels fuse is found by
:func:`adam_form`, once per (device, dtype).

``guard="device"`` (opt in, with fused stepping) removes the one sync per
iteration that is left: the :71 guard is decided on the device and the step is
gated on it (``libfedavg_amd_clientloop.so``: ``fedavg_client_guard_*``,
``fedavg_client_{sgd,adam}_step_gated_*``), so the host queues iterations
without waiting and reads ONE record at the end of ``train``.

:func:`client_train` is ``Client.train`` written against this class and
:func:`patch` binds it to a ``Client`` class (opt in; ``install()`` does not).
The native calls' buffers and their reuse rule are :mod:`client_passes`'s, the
probes behind :func:`sgd_form` and :func:`adam_form` :mod:`client_forms`'s.
"""
from __future__ import annotations

import math
import sys

import numpy as np
import torch

from . import _lib
from .client_forms import _ADAM_PROBE, _mine_site_c, _probe_adam_form, _probe_sgd_form, _probe_values  # noqa: F401
from .client_passes import (ADAM_SITES, FUSED_DTYPES, _RULE, _STEP_SUFFIX, _AdamPass, _KeyPass,  # noqa: F401
                            _STATS_LIBS, _StepPass, _fused_ok, _guard_bound, _norm_of, _round_to, adam_coef)

# rec: one device record of doubles, read back in one D2H.  The device guard adds the previous loss, the gate and
# the epoch of the first trip (include/fedavg_amd_clientloop.h: loss = rec[_LOSS:_LOSS + 2], gate = rec[_GATE:_GATE + 2])
_W, _G, _STATE, _LOSS, _LAST, _GATE, _EPOCH, _REC = 0, 4, 8, 12, 13, 14, 15, 16
# guard="device": how many iterations the host may queue before it waits for the oldest one's record
DEFAULT_AHEAD = 1
_GUARD_RULE = ("fused stepping (step='fused', or 'auto' where it applies): the step is gated on the device, which "
               "optimizer.step() cannot be")


# ------------------------------------------------------------------ fused step
# The dtypes the fused step is offered for: those sgd_form() found a form for on the MI355X (torch 2.10 / ROCm 7.0:
# form 1 for fp32, bf16 and fp64).  Not fp16: there torch's kernel rounds fma(alpha, g, w) ONCE, to fp16 (a
# mixed-precision fma), while both forms round to fp32 first; on sgd_form's probe form 1 differs from torch on 2 of
# 571 elements, form 0 on 61.  fedavg_client_sgd_step_f16 stays in the C ABI; nothing here calls it.
STEP_DTYPES = (torch.float32, torch.bfloat16, torch.float64)
_STEP_RULE = (f"the fused statistics ({_RULE}), fp32, bf16 or fp64 parameters, a plain SGD step (client_optimizer "
              "'sgd': no momentum, no weight decay) and a form of the step kernel that leaves torch.optim.SGD's bits "
              "on this GPU (sgd_form)")
_probes = {}  # (device index, dtype) -> the SGD probe's findings
_adam_probes = {}  # the same for the Adam probe


def _cached_probe(what, cache, probe, device, dtype):
    """``probe(device, dtype)``'s findings, from ``cache`` after the first call for a (device index, dtype)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise TypeError(f"{what} needs a GPU, not {device}")
    index = torch.cuda.current_device() if device.index is None else device.index
    key = (index, dtype)
    if key not in cache:
        cache[key] = probe(torch.device("cuda", index), dtype)
    return cache[key]


def sgd_form_probe(device, dtype):
    """What :func:`sgd_form` found for (device, dtype), cached: ``form``, the
    number of probe elements on which the kernel's two forms ``differ``,
    ``match`` (form 0 / form 1 equal to torch on every element) and ``n``."""
    return _cached_probe("sgd_form", _probes, _probe_sgd_form, device, dtype)


def sgd_form(device, dtype):
    """Which form of ``fedavg_client_sgd_step_*`` leaves the bits of
    ``torch.optim.SGD(params, lr=lr).step()`` on this GPU: 1 (``fma(-lr, g,
    w)``), 0 (product and sum rounded separately) or ``None`` (neither, or no
    kernel for the dtype).  Found by running torch's own step and both forms
    on the same seeded values, once per (device, dtype)."""
    if dtype not in STEP_DTYPES:
        return None
    return sgd_form_probe(device, dtype)["form"]


# ------------------------------------------------------------------ fused Adam step
# The dtypes the fused Adam step is offered for.  Two findings on the MI355X (torch 2.10 / ROCm 7.0) decide it: the
# probe of client_forms.py finds one mask that equals torch (mask 15, all four sites one fma, for all four dtypes), AND
# the kernel under that mask equals torch.optim.Adam bit for bit over twelve-step chains at the reference's own
# hyperparameters and three other sets, down to subnormal second moments (tests/test_gpu_client_adam_torch.py;
# DESIGN.md §3).  fp16 passes the first and fails the second: torch's fp16 kernels round g + wd * w, v * beta2,
# v1 + value * g1^2 and w + step * (m' / s3) ONCE, from the exact result straight to fp16 (scripts/probe_adam_ops.py
# --fp16-ties, profiles/client_adam/ops_probe_fp16_ties.json; tests/test_gpu_client_adam_torch.py), where every
# form of the kernel rounds to fp32 first.  The two part
# where the exact result lies within half an fp32 ulp of an fp16 rounding midpoint, which the decimal scalars 0.001
# and 0.999 make common for fp16 operands and the probe's scalars do not.  The same test file holds that finding on
# the kernel's C entry.  fedavg_client_adam_step_f16 stays in the C ABI; nothing here calls it.  For a dtype outside
# this tuple adam_form() answers None without probing; adam_form_probe() still runs the probe and reports what it
# finds (for fp16: mask 15), which says that the mask matches torch on the probe's values and no more.
ADAM_DTYPES = (torch.float32, torch.bfloat16, torch.float64)
_ADAM_RULE = (f"the fused statistics ({_RULE}), a dtype of ADAM_DTYPES (fp32, bf16, fp64), torch.optim.Adam with "
              "amsgrad=True and beta1 > 0.5 over parameters that all require grad, and a form of the Adam step kernel that leaves "
              "torch.optim.Adam's bits on this GPU (adam_form)")


def adam_form_probe(device, dtype):
    """What :func:`adam_form` found for (device, dtype), cached: ``form``,
    ``match`` (per mask: equal to torch on every element of ``p, exp_avg,
    exp_avg_sq, max_exp_avg_sq`` after each of ``steps`` steps), ``off`` (per
    mask: the number of elements that differ from torch's) and ``n``."""
    return _cached_probe("adam_form", _adam_probes, _probe_adam_form, device, dtype)


def adam_form(device, dtype):
    """Which form mask of ``fedavg_client_adam_step_*`` leaves the bits of
    ``torch.optim.Adam(params, lr, weight_decay=wd, amsgrad=True).step()`` on
    this GPU, or ``None``.  Found by running torch's own optimizer for three
    steps and the kernel under all 16 masks on the same seeded values (for a
    16-bit type joined by pairs mined for site C, which random values never
    reach there); the
    answer is a mask that equals torch on every element of the parameter and
    of the three state tensors at every step and differs from every other
    mask somewhere on the probe.  Once per (device, dtype).  ``None``
    without a probe for a dtype outside ``ADAM_DTYPES``: that tuple leaves
    out fp16, whose mask equals torch on the probe but not at the
    reference's hyperparameters (see the comment at ``ADAM_DTYPES``)."""
    if dtype not in ADAM_DTYPES:
        return None
    return adam_form_probe(device, dtype)["form"]


def _adam_hyper(adam):
    """``adam`` with torch.optim.Adam's defaults filled in; ``lr`` is required."""
    if adam is None or "lr" not in adam:
        raise ValueError("optimizer='adam' needs adam=dict(lr=..., betas=(0.9, 0.999), eps=1e-8, weight_decay=0, "
                         "amsgrad=True)")
    unknown = set(adam) - {"lr", "betas", "eps", "weight_decay", "amsgrad"}
    if unknown:
        raise ValueError(f"adam: unknown keys {sorted(unknown)}")
    h = {"betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0.0, "amsgrad": True, **adam}
    h["betas"] = (float(h["betas"][0]), float(h["betas"][1]))
    return h


class ClientStepStats:
    """Snapshots, key tables, workspaces and the running rho / beta of one
    ``Client.train`` call.

    ``begin()`` after the prologue's backward (:52-57), then per local
    iteration ``after_backward()`` (:69-71, the one sync; ``True`` = the guard
    trips) and ``after_step()`` (:76-86, no sync); ``result()`` at the end.
    ``trace(stage, w, g, loss)`` receives clones of the flattened weights and
    gradients at every call (``g`` is ``None`` where there is none yet).

    ``step="fused"``: ``sgd_step()`` takes the place of the caller's
    ``optimizer.step()`` and of ``after_step()`` (one kernel, no sync); it
    needs the fused statistics and a form from :func:`sgd_form`, else
    ``TypeError``.  ``step="auto"`` falls back to ``"torch"`` instead;
    ``step_mode`` says which of the two the object was built for.

    ``optimizer="adam"`` with ``adam=dict(lr, betas=(0.9, 0.999), eps=1e-8,
    weight_decay=0, amsgrad=True)``: under fused stepping the object owns the
    zeroed optimizer state and the step count, and ``adam_step()`` takes the
    place of ``optimizer.step()`` and ``after_step()``.  ``amsgrad=False``, a
    parameter that does not require grad, ``beta1 <= 0.5`` or a dtype without
    a form from :func:`adam_form` are a ``TypeError`` under ``"fused"`` and
    torch under ``"auto"``.

    ``guard="device"`` (opt in; the default ``"host"`` is everything above, to
    the bit) decides :71 on the device (``libfedavg_amd_clientloop.so``) and
    gates the fused step on that decision, so an iteration is
    ``guarded_step()`` alone, with no host sync: it queues the gradient pass,
    the guard, the gated step (whose finalize also tracks rho / beta) and an
    asynchronous copy of the record into a pinned ring of ``ahead`` slots.
    ``poll()`` reads whichever slots have arrived, never blocking, and
    ``finish()`` is the one sync of the whole loop.  It needs fused stepping
    (``TypeError`` otherwise; ``guard="auto"`` falls back to ``"host"``);
    ``guard_mode`` says which one the object got.  A tripped guard leaves the
    parameters and the optimizer state exactly as the host guard does (no
    gated launch writes once the gate is set), but the host may have queued up
    to ``ahead`` more forward / backward passes before it noticed: module
    buffers (BatchNorm running statistics) and the RNG stream dropout draws
    from can be ahead of the reference's.  ``trace`` receives ``loss=None``.
    """

    def __init__(self, params, *, stream=None, stats="auto", trace=None, step="torch", optimizer="sgd", adam=None,
                 guard="host", ahead=None):
        self.params = list(params)
        if guard not in ("host", "device", "auto"):
            raise ValueError(f"guard must be 'host', 'device' or 'auto', not {guard!r}")
        if ahead is not None and (int(ahead) != ahead or ahead < 1):
            raise ValueError(f"ahead must be a positive integer, not {ahead!r}")
        if optimizer not in ("sgd", "adam"):
            raise ValueError(f"optimizer must be 'sgd' or 'adam', not {optimizer!r}")
        self.optimizer = optimizer
        self.adam = _adam_hyper(adam) if optimizer == "adam" else None
        if stats not in ("auto", "hip", "torch"):
            raise ValueError(f"stats must be 'auto', 'hip' or 'torch', not {stats!r}")
        if step not in ("torch", "fused", "auto"):
            raise ValueError(f"step must be 'torch', 'fused' or 'auto', not {step!r}")
        fused = _fused_ok(self.params)
        if stats == "hip" and not fused:
            raise TypeError(f"stats='hip' needs {_RULE}")
        self.mode = "hip" if (fused and stats != "torch") else "torch"
        self.trace = trace
        self.stream = stream
        self.host_syncs = 0
        self.loss = None  # the current iteration's loss as a Python float (after after_backward)
        self._begun = False
        if self.mode == "hip":
            self._init_hip()
        else:
            self._last_w = self._last_grads = self._grads = None
            self._rho = self._beta = None
        self.step_mode = "torch"
        if step != "torch" and optimizer == "sgd":
            self._form = sgd_form(self.device, self.dtype) if self.mode == "hip" else None
            if self._form is not None:
                self.step_mode = "fused"
                self._step = _StepPass(self._numel, self.dtype, self.device)
            elif step == "fused":
                raise TypeError(f"step='fused' needs {_STEP_RULE}")
        elif step != "torch":
            h = self.adam
            plain = h["amsgrad"] is True and h["betas"][0] > 0.5 and all(p.requires_grad for p in self.params)
            self._form = adam_form(self.device, self.dtype) if self.mode == "hip" and plain else None
            if self._form is not None:
                self.step_mode = "fused"
                self._t = 0
                self._step = _AdamPass(self._numel, self._offset, self.P, self.dtype, self.device)
            elif step == "fused":
                raise TypeError(f"step='fused' needs {_ADAM_RULE}")
        self.guard_mode = "host"
        if guard != "host":
            if self.step_mode == "fused":
                self.guard_mode = "device"
                self._init_device_guard(DEFAULT_AHEAD if ahead is None else int(ahead))
            elif guard == "device":
                raise TypeError(f"guard='device' needs {_GUARD_RULE}")

    # ------------------------------------------------------------------ fused
    def _init_device_guard(self, ahead):
        lib = _lib.load_clientloop()
        self._guard_name = f"fedavg_client_guard_{_STEP_SUFFIX[self.dtype]}"
        self._guard_fn = getattr(lib, self._guard_name)
        self.ahead = ahead
        with torch.cuda.device(self.device):
            self._ring = torch.zeros(ahead, _REC, dtype=torch.float64, pin_memory=True)
        self._ring_np = self._ring.numpy()
        self._ring_ev = [None] * ahead
        self._issued = 0      # guarded_step() calls so far: the next epoch
        self._seen = 0        # ring records read so far, in order
        self._trip = None     # the epoch of the first trip a record showed
        self.ring_waits = 0   # times a full ring made guarded_step() wait for its oldest record

    def _see(self, i):
        """Read the arrived record of iteration i."""
        rec = self._ring_np[i % self.ahead]
        if self._trip is None and rec[_GATE] != 0.0:
            self._trip = int(rec[_EPOCH])
        self._seen = i + 1

    def _init_hip(self):
        self.device = self.params[0].device
        self.dtype = dt = self.params[0].dtype
        align = 16 // self.params[0].element_size()  # snapshot key offsets are multiples of 16 B
        self._numel = np.array([p.numel() for p in self.params], dtype=np.int64)
        padded = (self._numel + (align - 1)) // align * align
        self._offset = np.concatenate([[0], np.cumsum(padded)[:-1]]).astype(np.int64)
        self.P = int(padded.sum())
        self._ptrs = {"w": np.array([p.data_ptr() for p in self.params], dtype=np.int64),
                      "g": np.zeros(len(self.params), dtype=np.int64)}
        load, self._check, self._stats_name, self._track_name, sizing, by_size = _STATS_LIBS[dt]
        lib = load()
        self._stats_fn, self._track_fn = getattr(lib, self._stats_name), getattr(lib, self._track_name)
        n = len(self.params)
        more = (self.params[0].element_size(),) if by_size else ()
        nparts = int(getattr(lib, sizing + "_partials")(self._numel.ctypes.data, n, *more))
        ws_bytes = int(getattr(lib, sizing + "_workspace")(n))
        self._passes = {k: _KeyPass(nparts, ws_bytes, self.device) for k in "wg"}
        with torch.cuda.device(self.device):
            self._snap = {k: torch.zeros(max(self.P, align), dtype=dt, device=self.device) for k in "wg"}
            self._rec = torch.zeros(_REC, dtype=torch.float64, device=self.device)
            self._rec_host = torch.zeros(_REC, dtype=torch.float64, pin_memory=True)

    def _torch_stream(self):
        return self.stream if self.stream is not None else torch.cuda.current_stream(self.device)

    def _grad_ptrs(self):
        out = self._ptrs["g"]
        for j, p in enumerate(self.params):
            g = p.grad
            if g is None:
                raise RuntimeError(f"parameter {j} has no grad (client.py:57 / :69 read every param.grad)")
            if not (g.is_cuda and g.dtype == self.dtype and g.is_contiguous() and g.device == self.device
                    and g.numel() == self._numel[j]):
                raise TypeError(f"parameter {j}: the fused statistics need a contiguous grad of the parameters' "
                                f"dtype ({self.dtype}) on {self.device}")
            out[j] = g.data_ptr()
        return out

    def _pass(self, which: str, has_snap: int):
        """One fused pass over the weights ('w') or the gradients ('g') on the stream."""
        ptrs = self._ptrs["w"] if which == "w" else self._grad_ptrs()
        self._passes[which].call(
            self._stats_fn, self._stats_name, self._check, ptrs.tobytes(),
            (ptrs.ctypes.data, self._numel.ctypes.data, self._offset.ctypes.data, len(self.params),
             self._snap[which].data_ptr(), self.P, has_snap),
            self._rec.data_ptr() + 8 * (_W if which == "w" else _G), self._torch_stream())

    def _put_loss(self, slot, loss_tensor):
        """``loss_tensor`` into ``rec[slot]`` on the stream (no ``.item()``)."""
        with torch.cuda.stream(self._torch_stream()), torch.no_grad():
            self._rec[slot:slot + 1].copy_(loss_tensor.detach().reshape(1))

    def _track(self, loss, last_loss, st):
        """client.py:78-84 on the device: rho / beta from the weight and gradient records."""
        base = self._rec.data_ptr()
        with torch.cuda.device(self.device):
            rc = self._track_fn(base + 8 * _STATE, base + 8 * _W, base + 8 * _G, abs(loss - last_loss), st.cuda_stream)
        self._check(rc, self._track_name)

    def _read_record(self):
        st = self._torch_stream()
        with torch.cuda.stream(st):
            self._rec_host.copy_(self._rec, non_blocking=True)
        st.synchronize()
        self.host_syncs += 1
        return self._rec_host.numpy()

    # ----------------------------------------------------------------- common
    def _flat(self, grads: bool):
        ts = []
        for j, p in enumerate(self.params):
            t = p.grad if grads else p
            if t is None:
                raise RuntimeError(f"parameter {j} has no grad (client.py:57 / :69 read every param.grad)")
            ts.append(t.view(-1))
        return torch.cat(ts)

    def _emit(self, stage, loss, with_grads=True):
        if self.trace is not None:
            with torch.no_grad():
                self.trace(stage, self._flat(False).detach().clone(),
                           self._flat(True).detach().clone() if with_grads else None, loss)

    def begin(self, loss=None):
        """client.py:52-57: the first snapshots of the weights and, after the
        caller's first backward, of the gradients.  Under the device guard
        ``loss`` is the prologue's loss TENSOR, copied into the record on the
        stream (no ``.item()``)."""
        if self.guard_mode == "device":
            if not torch.is_tensor(loss):
                raise TypeError("begin() under guard='device' takes the prologue's loss tensor: the record keeps it "
                                "on the device as the first last_loss")
            self._put_loss(_LAST, loss)
            loss = None
        if self.mode == "hip":
            self._pass("w", 0)
            self._pass("g", 0)
        else:
            self._last_w = self._flat(False)
            self._last_grads = self._flat(True)
        self._begun = True
        self._emit("begin", loss)

    def after_backward(self, loss_tensor, lr, ratio) -> bool:
        """client.py:69-71: the gradient pass and the guard.  ``True`` when the
        reference would give up: a NaN in the gradients, a NaN loss, or
        ``norm(grads) > lr * ratio * norm(last_w)``."""
        if self.guard_mode == "device":
            raise RuntimeError("after_backward() on an object built with guard='device': guarded_step() takes the "
                               "guard, the step and the bookkeeping of the iteration")
        if not self._begun:
            raise RuntimeError("begin() first")
        if self.mode == "hip":
            self._pass("g", 1)
            self._put_loss(_LOSS, loss_tensor)
            rec = self._read_record()
            self.loss = float(rec[_LOSS])
            # every dtype alike, as the device guard decides it (fp32: fl32(sqrt(S)) and fl32(lr * ratio) * n_w)
            self.grad_norm = n_g = _norm_of(float(rec[_G + 1]), self.dtype)
            self.weight_norm = n_w = _norm_of(float(rec[_W + 1]), self.dtype)
            trip = bool(rec[_G] > 0 or math.isnan(self.loss) or n_g > _guard_bound(n_w, lr * ratio, self.dtype))
        else:
            with torch.no_grad():
                grads = self._grads = self._flat(True)
                trip = bool(torch.isnan(grads).sum() > 0 or torch.isnan(loss_tensor)
                            or torch.norm(grads) > lr * ratio * torch.norm(self._last_w))
            self.loss = None if trip else loss_tensor.item()
        self._emit("after_backward", self.loss)
        return trip

    def after_step(self, loss, last_loss):
        """client.py:76-86 after ``optimizer.step()``: the weight pass and the
        running rho / beta; ``loss`` and ``last_loss`` are the Python floats of
        :75 and :56 / :86."""
        if self.step_mode == "fused":
            raise RuntimeError("after_step() on an object built for fused stepping: sgd_step() takes the step and "
                               "keeps no weight snapshot for this pass to compare with")
        if self.mode == "hip":
            self._pass("w", 1)
            self._track(loss, last_loss, self._torch_stream())
        else:
            with torch.no_grad():
                w = self._flat(False)
                rho_tmp = abs(loss - last_loss) / torch.norm(w - self._last_w)
                if not self._rho or rho_tmp > self._rho:
                    self._rho = rho_tmp
                beta_tmp = torch.norm(self._grads - self._last_grads) / torch.norm(w - self._last_w)
                if not self._beta or beta_tmp > self._beta:
                    self._beta = beta_tmp
                self._last_w, self._last_grads = w, self._grads
        self._emit("after_step", loss)

    def sgd_step(self, lr, loss, last_loss):
        """client.py:74-86 in one kernel, in place of ``optimizer.step()`` and
        ``after_step()``: ``w -= lr * g`` with torch.optim.SGD's bits, the
        weight record (``sum w'^2`` for the next guard, ``sum rT(w' - w)^2``
        for :78 / :82) and the running rho / beta.  No host sync."""
        self._host_step("sgd", lr, loss, last_loss)

    def adam_step(self, loss, last_loss):
        """client.py:74-86 in one kernel, in place of ``optimizer.step()`` and
        ``after_step()``: the Adam step with torch.optim.Adam's bits on ``w``
        and on the state this object owns, the weight record and the running
        rho / beta.  The first call of an object does not read the state.  No
        host sync."""
        self._host_step("adam", None, loss, last_loss)

    def _built_for(self, what, optimizer=None, begun=True):
        """``what`` needs the fused ``optimizer`` step under the host guard or, with none named, the device guard."""
        if optimizer is None and self.guard_mode != "device":
            raise RuntimeError(f"{what} needs an object built with guard='device' (or 'auto' where it applies): "
                               f"this one decides the guard on the host ({self.guard_mode=})")
        if optimizer is not None and self.step_mode != "fused":
            raise RuntimeError(f"{what} needs an object built with step='fused' (or 'auto' where it applies): "
                               f"this one steps with torch ({self.step_mode=})")
        if optimizer is not None and self.optimizer != optimizer:
            raise RuntimeError(f"{what} on an object built with optimizer='{self.optimizer}': {self.optimizer}_step() "
                               "takes its step")
        if optimizer is not None and self.guard_mode == "device":
            raise RuntimeError(f"{what} on an object built with guard='device': guarded_step() takes its step")
        if begun and not self._begun:
            raise RuntimeError("begin() first")

    def _launch_step(self, lr, st, gated=None):
        """The object's fused step on ``st``: SGD with ``lr``, or Adam with its own hyperparameters and step
        count; the record goes to ``rec[_W:]``.  ``gated``: the gated entry's four device addresses."""
        stats_ptr = self._rec.data_ptr() + 8 * _W
        if self.optimizer == "sgd":
            self._step.launch(self._ptrs["w"], self._grad_ptrs(), lr, self._form, stats_ptr, st, gated)
        else:
            h = self.adam
            self._t += 1  # past a trip the count runs on, and no gated launch reads the state it counts for
            coef = adam_coef(h["lr"], *h["betas"], h["eps"], h["weight_decay"], self._t)
            self._step.launch(self._ptrs["w"], self._grad_ptrs(), coef, self._t == 1, self._form, stats_ptr, st, gated)
        torch.autograd.graph.increment_version(self.params)  # the in-place update autograd did not see

    def _host_step(self, optimizer, lr, loss, last_loss):
        self._built_for(f"{optimizer}_step()", optimizer)
        st = self._torch_stream()
        self._launch_step(lr, st)
        self._track(loss, last_loss, st)
        self._emit("after_step", loss)

    # ------------------------------------------------------------ device guard
    def guarded_step(self, loss_tensor, lr, ratio):
        """client.py:69-86 of one iteration, queued on the stream with no host
        sync: the gradient pass, the loss into the record, the :71 guard on
        the device, the step behind its gate (the finalize also tracks rho /
        beta and moves ``loss`` to ``last_loss``) and a copy of the record
        into slot ``i % ahead`` of the pinned ring.  With the ring full it
        first waits for the oldest record alone, so the host is never more
        than ``ahead`` iterations in front."""
        self._built_for("guarded_step()")
        i, slot = self._issued, self._issued % self.ahead
        if i - self._seen >= self.ahead:  # the slot's last record (iteration i - ahead) has not been read
            self._ring_ev[slot].synchronize()
            self.ring_waits += 1
            self._see(i - self.ahead)
        st = self._torch_stream()
        self._pass("g", 1)
        self._put_loss(_LOSS, loss_tensor)
        self._emit("after_backward", None)
        base = self._rec.data_ptr()
        with torch.cuda.device(self.device):
            rc = self._guard_fn(base + 8 * _G, base + 8 * _W, base + 8 * _LOSS, base + 8 * _GATE, float(lr * ratio), i,
                                st.cuda_stream)
        _lib.check_clientloop(rc, self._guard_name)
        self._launch_step(lr, st, (base + 8 * _G, base + 8 * _GATE, base + 8 * _STATE, base + 8 * _LOSS))
        with torch.cuda.stream(st):
            self._ring[slot].copy_(self._rec, non_blocking=True)
            if self._ring_ev[slot] is None:
                self._ring_ev[slot] = torch.cuda.Event()
            self._ring_ev[slot].record(st)
        self._issued = i + 1
        self._emit("after_step", None)

    def poll(self):
        """The epoch of the first trip among the records that have arrived,
        else ``None``.  Never blocks: ``event.query()`` on the ring slots not
        yet read, in order."""
        self._built_for("poll()", begun=False)
        while self._seen < self._issued and self._ring_ev[self._seen % self.ahead].query():
            self._see(self._seen)
        return self._trip

    def finish(self):
        """The one sync of the loop: ``(trip_epoch_or_None, loss, beta, rho)``
        from the record as the stream leaves it.  ``loss`` is the last
        iteration's; ``None`` before any ``guarded_step()`` and after a trip
        (iterations queued behind the tripping one have overwritten its slot,
        and the reference returns none either)."""
        self._built_for("finish()", begun=False)
        rec = self._read_record()
        self._seen = self._issued
        if rec[_GATE] != 0.0:
            self._trip = int(rec[_EPOCH])
        self.loss = float(rec[_LOSS]) if self._issued and self._trip is None else None
        return self._trip, self.loss, *self._beta_rho(rec)

    @staticmethod
    def _beta_rho(rec):
        """``(beta, rho)`` of a record read back: ``rec[_STATE:]`` is ``rho, beta, has_rho, has_beta``."""
        return (float(rec[_STATE + 1]) if rec[_STATE + 3] else None,
                float(rec[_STATE]) if rec[_STATE + 2] else None)

    def result(self):
        """``(beta, rho)`` as Python floats (``None`` where no step was taken)."""
        if self.mode == "hip":
            return self._beta_rho(self._read_record())
        return (None if self._beta is None else self._beta.item(),
                None if self._rho is None else self._rho.item())


def client_train(self, net, local_iteration, *, keep_on_device=False, stats="auto", trace=None, step="torch",
                 guard="host"):
    """``Client.train(self, net, local_iteration)`` (client.py:38-96) with the
    bookkeeping of :52-86 done by :class:`ClientStepStats`.

    Returns ``(state_dict, loss, beta, rho, acc, cycles)``, or the state_dict
    and five ``None`` when the :71 guard trips.  ``count`` / ``count_end`` and
    ``THRESHOLD_GRADS_RATIO`` are the ones of the module that defines
    ``type(self)`` (the reference's ``client`` module).  ``keep_on_device``
    returns ``net.state_dict()`` without the ``.cpu()`` of :73 / :96.
    ``step`` is :class:`ClientStepStats`'s: with fused stepping and
    ``args.client_optimizer == "sgd"`` one ``sgd_step(args.lr, ...)`` replaces
    ``optimizer.step()`` and ``after_step()``.  Any other
    ``args.client_optimizer`` is the reference's Adam (``lr``, ``wd``,
    amsgrad): with fused stepping one ``adam_step()`` per iteration and no
    torch optimizer at all; where the fused Adam step does not apply it is a
    ``TypeError`` under ``"fused"`` and steps with torch under ``"auto"``.
    ``guard`` is :class:`ClientStepStats`'s: under the device guard an
    iteration is forward, backward and ``guarded_step()``, the loop leaves as
    soon as ``poll()`` shows a trip and ``finish()`` after it is the one host
    sync of the bookkeeping.  The return values are the host guard's to the
    bit; after a trip the parameters are too, while module buffers and the
    RNG stream may be up to ``ahead`` iterations further (see the class).
    """
    mod = sys.modules[type(self).__module__]
    count, count_end, ratio = mod.count, mod.count_end, mod.THRESHOLD_GRADS_RATIO
    sgd = self.args.client_optimizer == "sgd"
    tracker = None
    if not sgd and step != "torch":  # refused, if it is, before anything runs
        try:
            tracker = ClientStepStats(net.parameters(), stats=stats, trace=trace, step=step, optimizer="adam",
                                      adam=dict(lr=self.args.lr, weight_decay=self.args.wd, amsgrad=True), guard=guard)
        except TypeError as e:
            raise TypeError(f"{e}; args.client_optimizer is {self.args.client_optimizer!r}") from None
    if sgd:
        optimizer = torch.optim.SGD(net.parameters(), lr=self.args.lr)
    elif tracker is None or tracker.step_mode != "fused":
        optimizer = torch.optim.Adam(filter(lambda p: p.requires_grad, net.parameters()), lr=self.args.lr,
                                     weight_decay=self.args.wd, amsgrad=True)
    cycles = []
    x, labels = next(iter(self.local_training_data))
    x, labels = x.to(self.device), labels.to(self.device)
    net.train()
    if tracker is None:
        tracker = ClientStepStats(net.parameters(), stats=stats, trace=trace, step=step if sgd else "torch",
                                  guard=guard)
    fused = tracker.step_mode == "fused"
    last_loss = self.criterion(net(x), labels)
    torch.nn.utils.clip_grad_norm_(net.parameters(), self.args.clip)
    last_loss.backward()
    done = lambda: net.state_dict() if keep_on_device else net.cpu().state_dict()  # noqa: E731

    def gave_up(epoch):
        logger = getattr(mod, "logger", None)
        if logger is not None:
            logger.warning("grads too large than weights or meets nan with epoch {}".format(epoch))
        return done(), None, None, None, None, None

    device_guard = tracker.guard_mode == "device"
    last_loss = last_loss.detach() if device_guard else last_loss.item()  # the device guard keeps it on the device
    tracker.begin(last_loss)
    for epoch in range(local_iteration):
        start = count()
        net.zero_grad()
        log_probs = net(x)
        loss = self.criterion(log_probs, labels)
        torch.nn.utils.clip_grad_norm_(net.parameters(), self.args.clip)
        loss.backward()
        cycles.append(count_end() - start)
        if device_guard:
            tracker.guarded_step(loss, self.args.lr, ratio)
            if tracker.poll() is not None:
                break
            continue
        if tracker.after_backward(loss, self.args.lr, ratio):
            return gave_up(epoch)
        loss = tracker.loss
        if fused and sgd:
            tracker.sgd_step(self.args.lr, loss, last_loss)
        elif fused:
            tracker.adam_step(loss, last_loss)
        else:
            optimizer.step()
            tracker.after_step(loss, last_loss)
        last_loss = loss
    if device_guard:
        trip, loss, beta, rho = tracker.finish()
        if trip is not None:
            return gave_up(trip)
    # local_iteration == 0 leaves log_probs unbound, as in the reference (:93)
    _, predicted = torch.max(log_probs, -1)
    correct = predicted.eq(labels).sum()
    if not device_guard:
        beta, rho = tracker.result()
    return done(), loss, beta, rho, correct.item() / labels.size(0), sum(cycles) / len(cycles)


class _Patch:
    """Undo handle of :func:`patch` (also a context manager)."""

    def __init__(self, cls, had, old):
        self.cls, self._had, self._old, self.active = cls, had, old, True

    def undo(self):
        if self.active:
            if self._had:
                setattr(self.cls, "train", self._old)
            else:
                delattr(self.cls, "train")
            self.active = False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.undo()
        return False


def patch(cls, *, keep_on_device=False, stats="auto", step="torch", guard="host"):
    """Replace ``cls.train`` (the reference's ``Client.train``) with
    :func:`client_train`; returns a handle whose ``undo()`` restores the class."""
    had = "train" in vars(cls)
    old = vars(cls).get("train")

    def train(self, net, local_iteration):
        return client_train(self, net, local_iteration, keep_on_device=keep_on_device, stats=stats, step=step,
                            guard=guard)

    train.__wrapped_by__ = "mfl_amd.client_stats"
    setattr(cls, "train", train)
    return _Patch(cls, had, old)
