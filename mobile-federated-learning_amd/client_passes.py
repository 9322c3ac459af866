"""The keyed passes behind :mod:`client_stats`: the buffers of a native call
over a model's tensors and the reuse rule of its pinned key table
(:class:`_KeyPass`), the fused SGD and Adam steps as its users, the statistics
library per dtype and the host side of the :71 guard's arithmetic."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib

# dtype -> entry suffix of the clientvec library; fp32 is the product library's
_VEC_DTYPES = {torch.bfloat16: "bf16", torch.float16: "f16", torch.float64: "f64"}
FUSED_DTYPES = (torch.float32, *_VEC_DTYPES)
_RULE = "contiguous parameters on one GPU, all of one dtype among fp32, bf16, fp16 and fp64"
_STEP_SUFFIX = {torch.float32: "f32", **_VEC_DTYPES}
ADAM_SITES = 4  # A g + wd w, B the lerp, C the addcmul, E the addcdiv: bit i of a form mask fuses site i

# The statistics pass per dtype, the product library against clientvec: (loader, check, statistics entry, track entry,
# stem of the ``_partials`` / ``_workspace`` sizing entries, whether ``_partials`` also takes the element size).
# _lib.check reports from the product library once that is loaded, which the loader has done by then.
_STATS_LIBS = {torch.float32: (_lib.load, _lib.check, "fedavg_client_stats_f32", "fedavg_client_track",
                               "fedavg_client_stats", False),
               **{dt: (_lib.load_clientvec, _lib.check_clientvec, f"fedavg_client_stats_{s}",
                       f"fedavg_client_track_{s}", "fedavg_client_stats_vec", True) for dt, s in _VEC_DTYPES.items()}}


def _fused_ok(params) -> bool:
    return bool(params) and all(p.is_cuda and p.is_contiguous() for p in params) and \
        len({p.device for p in params}) == 1 and len({p.dtype for p in params}) == 1 and \
        params[0].dtype in FUSED_DTYPES


def _round_to(x, dtype):
    """rT(fl32(x)) as a Python float: x rounded to fp32, then to ``dtype``
    (nearest even both times), as ATen casts an opmath result.  fp64: x."""
    if dtype == torch.float64:
        return float(x)
    with np.errstate(all="ignore"):
        f = np.float32(x)
        if dtype == torch.float32:
            return float(f)
        if dtype == torch.float16:
            return float(np.float16(f))
    if math.isnan(f):
        return math.nan
    u = int(f.view(np.uint32))
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000  # bf16: the upper half of the fp32 word
    return float(np.uint32(u).view(np.float32))


def _norm_of(sumsq, dtype):
    """norm(S) = rT(fl32(sqrt(S))) (fp64: sqrt(S)): the exactly rounded value
    of what ATen's norm approximates in opmath."""
    if math.isnan(sumsq):
        return math.nan
    return _round_to(math.sqrt(sumsq), dtype)


def _guard_bound(n_w, lr_ratio, dtype):
    """``lr * ratio * norm(last_w)`` (:71): python_float * tensor, the scalar
    rounded to opmath, the product to the tensor's type."""
    if dtype == torch.float64:
        return n_w * lr_ratio
    with np.errstate(all="ignore"):
        # the fp64 product of two fp32 values is exact: one rounding to fp32
        return _round_to(np.float64(n_w) * np.float64(np.float32(lr_ratio)), dtype)


class _KeyPass:
    """What a native call over ``n`` keys needs besides its own arguments: the
    ``partials`` doubles and the pinned ``host_ws`` / device ``dev_ws`` pair
    its key table is staged through.  Every client entry ends in ``partials,
    partial_elems, stats, host_ws, dev_ws, ws_bytes, stream`` (a gated one adds
    its four gate pointers), writes its table into ``host_ws`` on the host and
    queues the copy to ``dev_ws``.  The reuse rule: new bytes go into
    ``host_ws`` only after the stream has passed the last call that shipped
    the old ones; a call with the same pointer tables rewrites the same bytes
    and need not wait."""

    def __init__(self, nparts, ws_bytes, device):
        self.device = device
        with torch.cuda.device(device):
            self.partials = torch.empty(max(nparts, 1), dtype=torch.float64, device=device)
            self.host_ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, pin_memory=True)
            self.dev_ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=device)
        self._free = None    # event: the stream has passed the last use of host_ws
        self._staged = None  # the pointer tables host_ws holds

    def stage(self, table) -> bool:
        """The reuse rule for a call that ships ``table`` (bytes); ``True``
        when it had to wait for the last call."""
        wait = self._free is not None and table != self._staged
        if wait:
            self._free.synchronize()  # already passed after an iteration's host sync
        self._staged = table
        return wait

    def call(self, fn, name, check, table, head, stats_ptr, st, gated=()):
        """``fn(*head, <the common tail>, *gated)`` on torch stream ``st``,
        its status through ``check``; the record goes to the device doubles
        at ``stats_ptr``."""
        self.stage(table)
        with torch.cuda.device(self.device):
            rc = fn(*head, self.partials.data_ptr(), self.partials.numel(), stats_ptr, self.host_ws.data_ptr(),
                    self.dev_ws.data_ptr(), self.host_ws.numel(), st.cuda_stream, *gated)
            check(rc, name)
            if self._free is None:
                self._free = torch.cuda.Event()
            self._free.record(st)


class _FusedStep(_KeyPass):
    """A step entry ``name`` of ``lib`` over keys of ``numel`` elements, sized
    by ``lib``'s ``{sizing}_partials`` / ``{sizing}_workspace``, and its gated
    twin in the loop library (``..._step_gated_*``, looked up when first used)."""

    def __init__(self, lib, check, name, sizing, numel, dtype, device):
        self.name, self.fn, self.check = name, getattr(lib, name), check
        self.numel = np.ascontiguousarray(numel, dtype=np.int64)
        n = len(self.numel)
        es = torch.empty(0, dtype=dtype).element_size()
        super().__init__(int(getattr(lib, sizing + "_partials")(self.numel.ctypes.data, n, es)),
                         int(getattr(lib, sizing + "_workspace")(n)), device)
        self._gated = None

    def _launch(self, w_ptrs, g_ptrs, head, stats_ptr, st, gated):
        fn, name, check = self.fn, self.name, self.check
        if gated is not None:
            if self._gated is None:
                name = self.name.replace("_step_", "_step_gated_")
                self._gated = (getattr(_lib.load_clientloop(), name), name, _lib.check_clientloop)
            fn, name, check = self._gated
        self.call(fn, name, check, w_ptrs.tobytes() + g_ptrs.tobytes(),
                  (w_ptrs.ctypes.data, g_ptrs.ctypes.data, self.numel.ctypes.data, *head), stats_ptr, st, gated or ())


class _StepPass(_FusedStep):
    """The buffers of ``fedavg_client_sgd_step_*`` calls over tensors of
    ``numel`` elements, and the call."""

    def __init__(self, numel, dtype, device):
        super().__init__(_lib.load_clientstep(), _lib.check_clientstep,
                         f"fedavg_client_sgd_step_{_STEP_SUFFIX[dtype]}", "fedavg_client_step", numel, dtype, device)

    def launch(self, w_ptrs, g_ptrs, lr, form, stats_ptr, st, gated=None):
        """w -= lr * g over the tensors at w_ptrs / g_ptrs on torch stream
        ``st``; the record goes to the 4 device doubles at ``stats_ptr``.
        ``gated``: the device addresses ``(g_stats, gate, state, loss)`` of
        ``fedavg_client_sgd_step_gated_*``, which then takes the call."""
        self._launch(w_ptrs, g_ptrs, (len(self.numel), float(lr), form), stats_ptr, st, gated)


def adam_coef(lr, beta1, beta2, eps, weight_decay, t):
    """The seven coefficients of ``fedavg_client_adam_step_*`` for step ``t``
    (from 1), in Python floats exactly as torch/optim/adam.py forms them."""
    t = float(t)
    bias_correction1 = 1 - beta1 ** t
    bias_correction2 = 1 - beta2 ** t
    step_size = (lr / bias_correction1) * -1
    return np.array([weight_decay, 1 - beta1, beta2, 1 - beta2, bias_correction2 ** 0.5, eps, step_size],
                    dtype=np.float64)


class _AdamPass(_FusedStep):
    """The optimizer state (three planes ``m, v, vmax`` of ``state_elems``
    elements in one zeroed buffer, key j at ``offset[j]``), the buffers of
    ``fedavg_client_adam_step_*`` calls and the call."""

    def __init__(self, numel, offset, state_elems, dtype, device):
        super().__init__(_lib.load_clientadam(), _lib.check_clientadam,
                         f"fedavg_client_adam_step_{_STEP_SUFFIX[dtype]}", "fedavg_client_adam", numel, dtype, device)
        self.offset = np.ascontiguousarray(offset, dtype=np.int64)
        self.state_elems = int(state_elems)
        es = torch.empty(0, dtype=dtype).element_size()
        with torch.cuda.device(device):
            self.state = torch.zeros(3 * max(self.state_elems, 16 // es), dtype=dtype, device=device)

    def plane(self, i):
        """Plane i (0 ``m``, 1 ``v``, 2 ``vmax``) as a view of the state."""
        return self.state[i * self.state_elems:(i + 1) * self.state_elems]

    def launch(self, w_ptrs, g_ptrs, coef, first, form, stats_ptr, st, gated=None):
        """``coef``: :func:`adam_coef`'s; ``first``: the state is not read;
        ``gated``: as ``_StepPass.launch``'s (``fedavg_client_adam_step_gated_*``)."""
        self._launch(w_ptrs, g_ptrs, (self.offset.ctypes.data, len(self.numel), self.state.data_ptr(), self.state_elems,
                                      coef.ctypes.data, int(bool(first)), form), stats_ptr, st, gated)
