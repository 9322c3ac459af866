"""Layout catalogue for the address-forming tests (test_layouts_host.py,
test_gpu_layouts.py) -- TEST INFRASTRUCTURE ONLY.

Every kernel reads client models through ``data_ptr()`` / ``numel()`` pairs
gathered by ``KeyTable.collect``.  The catalogue builds tensors that are
``torch.equal`` to given values but are not a plain, freshly allocated,
contiguous block, so a test can tell whether a route handed its kernels the
right bytes.  Each ``make(values)`` works for host and device tensors, and
every byte of the buffer around the wanted values holds junk (NaN for the
floating types, 77 otherwise): a route that reads ``numel`` elements from the
raw ``data_ptr()`` of a strided tensor stays inside the buffer and shows up
as wrong values.

``model`` builds a round of client state_dicts with chosen layouts and
dtypes, plus a deep, plain, host copy for the oracle.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, Mapping, Optional, Sequence

import numpy as np
import torch

# The smallest shapes that still cross what the code branches on.  `big`
# crosses the pack kernel's 4,096-element wave chunk and the segment unit;
# `head.weight` has the size-1 dim `unit_dims` needs and `head.bias` is
# `fc.bias`'s twin (same shape), so one tensor object can be two keys of one
# client (`shared`).  P = 4,587 elements.
KEY_SHAPES = OrderedDict([
    ("conv.weight", (8, 3, 3, 3)),
    ("fc.weight", (33, 7)),
    ("fc.bias", (10,)),
    ("head.weight", (1, 10)),
    ("head.bias", (10,)),
    ("big", (4099,)),
    ("bn.num_batches_tracked", ()),
    ("mask", (5, 2)),
    ("empty", (0,)),
])
INT_KEYS = {"bn.num_batches_tracked": torch.int64, "mask": torch.uint8}
FLOAT_KEYS = [k for k in KEY_SHAPES if k not in INT_KEYS]


def _junk(n: int, like: torch.Tensor) -> torch.Tensor:
    fill = float("nan") if like.dtype.is_floating_point else 77
    return torch.full((max(int(n), 1),), fill, dtype=like.dtype, device=like.device)


def plain(values: torch.Tensor) -> torch.Tensor:
    return values.clone()


def transposed(values: torch.Tensor) -> torch.Tensor:
    assert values.dim() == 2
    return values.t().contiguous().t()


def step2(values: torch.Tensor) -> torch.Tensor:
    """Every other element of a buffer twice as long in the last dim."""
    assert values.dim() >= 1
    shape = tuple(values.shape[:-1]) + (2 * values.shape[-1],)
    buf = _junk(int(np.prod(shape)), values)[:int(np.prod(shape))].view(shape)
    out = buf[..., ::2]
    out.copy_(values)
    return out


def channels_last(values: torch.Tensor) -> torch.Tensor:
    assert values.dim() == 4
    return values.clone().contiguous(memory_format=torch.channels_last)


def expanded(values: torch.Tensor) -> torch.Tensor:
    """Stride 0 in every dim: one element of a buffer as long as the key,
    expanded to the key's shape (the key's values must all be equal)."""
    assert values.numel() > 1 and bool((values == values.reshape(-1)[0]).all())
    buf = _junk(values.numel(), values)
    buf[0] = values.reshape(-1)[0]
    return buf[0].expand(values.shape)


def offset1(values: torch.Tensor) -> torch.Tensor:
    """Contiguous, starting one element into its storage: 4-byte aligned for
    fp32, 2-byte for fp16 / bf16, 8-byte for fp64 -- never 16."""
    n = values.numel()
    buf = _junk(n + 8, values)
    buf[1:1 + n].copy_(values.reshape(-1))
    return buf[1:1 + n].view(values.shape)


def unit_dims(values: torch.Tensor) -> torch.Tensor:
    """``is_contiguous()`` with a stride of 997 on every size-1 dim."""
    assert 1 in values.shape and values.numel() > 0
    strides, n = [], 1
    for d in reversed(values.shape):
        strides.append(997 if d == 1 else n)
        n *= d
    out = _junk(997 + values.numel(), values).as_strided(tuple(values.shape), tuple(reversed(strides)))
    out.copy_(values)
    return out


# `shared` is an arrangement of a round, not of one tensor: `model` puts the
# same tensor object into two clients and under two keys of one client
LAYOUTS = OrderedDict([
    ("plain", plain),
    ("transposed", transposed),
    ("step2", step2),
    ("channels_last", channels_last),
    ("expanded", expanded),
    ("offset1", offset1),
    ("unit_dims", unit_dims),
    ("shared", plain),
])
# layouts whose tensors say is_contiguous(): read in place, no copy
CONTIGUOUS = ("plain", "offset1", "unit_dims", "shared")
NON_CONTIGUOUS = tuple(k for k in LAYOUTS if k not in CONTIGUOUS)

# the floating key each layout is applied to, and the integer key that can take it too
TARGET = {"plain": "fc.weight", "transposed": "fc.weight", "step2": "big", "channels_last": "conv.weight",
          "expanded": "fc.bias", "offset1": "big", "unit_dims": "head.weight", "shared": "fc.bias"}
INT_TARGET = {"plain": "mask", "transposed": "mask", "step2": "mask", "offset1": "mask"}
TWIN = {"fc.bias": "head.bias"}  # same shape: one tensor object as two keys of a client


def _values(key: str, dtype: torch.dtype, client: int, gen: torch.Generator, constant: bool) -> torch.Tensor:
    shape = KEY_SHAPES[key]
    if dtype == torch.int64:
        return torch.full(shape, 100 + client, dtype=dtype)
    if dtype == torch.uint8:
        return torch.randint(0, 256, shape, generator=gen).to(dtype)
    if constant:
        return torch.full(shape, 0.125 * (client + 1), dtype=dtype)
    return (torch.randn(shape, generator=gen) * 0.05).to(dtype)


def model(layout_by_key: Mapping[str, str], dtype_by_key: Optional[Mapping[str, torch.dtype]] = None, K: int = 3,
          seed: int = 0, *, clients: Sequence[int] = (0, 2), keys: Optional[Sequence[str]] = None, device=None):
    """A round of ``K`` clients.  ``layout_by_key[key]`` names the layout that
    key takes in the clients ``clients`` (default: client 0 and one other);
    every other tensor is plain.  ``dtype_by_key`` overrides a key's dtype
    (fp32, or the integer keys' own, otherwise); ``keys`` picks the model's
    keys (all of KEY_SHAPES by default); ``device`` places the clients.

    Returns ``(w_locals, ref_locals)``: the round, and a deep, plain, host
    copy of it for the oracle."""
    dtype_by_key = dict(dtype_by_key or {})
    keys = list(KEY_SHAPES if keys is None else keys)
    gen = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    w_locals, ref_locals = [], []
    shared: Dict[str, torch.Tensor] = {}  # key -> the tensor object the first of `clients` holds for it
    for i in range(K):
        sd, ref = OrderedDict(), OrderedDict()
        twins: Dict[str, str] = {}  # key -> the earlier key of this client whose tensor object it is
        for key in keys:
            dt = dtype_by_key.get(key, INT_KEYS.get(key, torch.float32))
            lay = layout_by_key.get(key, "plain") if i in clients else "plain"
            if lay == "shared" and key in shared:  # a later client: the same object under this key and its twin
                sd[key] = shared[key]
                ref[key] = shared[key].detach().cpu().clone()
                if TWIN.get(key) in keys:
                    twins[TWIN[key]] = key
                continue
            if key in twins:
                assert sd[twins[key]].dtype == dt and sd[twins[key]].shape == KEY_SHAPES[key]
                sd[key] = sd[twins[key]]
                ref[key] = ref[twins[key]].clone()
                continue
            v = _values(key, dt, i, gen, constant=(lay == "expanded"))
            ref[key] = v.clone()
            t = LAYOUTS[lay](v if device is None else v.to(device))
            assert t.shape == v.shape and t.dtype == v.dtype
            assert t.is_contiguous() == (lay in CONTIGUOUS) or t.numel() < 2, (key, lay)
            if lay == "shared":
                shared[key] = t
            sd[key] = t
        n = int(rng.integers(1, 1000))
        w_locals.append((n, sd))
        ref_locals.append((n, ref))
    return w_locals, ref_locals


def to_plain_host(w_locals):
    """A deep, plain, host copy of a round (what ``model`` returns second)."""
    return [(n, OrderedDict((k, v.detach().cpu().clone().contiguous()) for k, v in sd.items())) for n, sd in w_locals]


def snapshot(w_locals):
    """What must not change in the clients after client 0: each dict, its
    tensor objects, their strides and a host copy of their values."""
    return [(sd, [(k, t, t.stride(), t.data_ptr(), t.detach().cpu().clone()) for k, t in sd.items()])
            for _, sd in w_locals[1:]]


def assert_untouched(snap, w_locals) -> None:
    assert len(snap) == len(w_locals) - 1
    for (sd0, items), (_, sd) in zip(snap, w_locals[1:]):
        assert sd is sd0 and list(sd) == [k for k, *_ in items]
        for k, t, stride, ptr, values in items:
            assert sd[k] is t, k
            assert t.stride() == stride and t.data_ptr() == ptr, k
            assert torch.equal(t.detach().cpu(), values), k


def cat_dtype(ref_locals) -> torch.dtype:
    """torch.cat's promoted dtype at fedavg_trainer.py:291 (keys subtracted one by one)."""
    cat = None
    for v in ref_locals[0][1].values():
        d = (v.reshape(-1)[:0] - v.reshape(-1)[:0]).dtype
        cat = d if cat is None else torch.promote_types(cat, d)
    return cat


def assert_norms(norms, exact, cat: torch.dtype) -> None:
    """The suite's bound for :291 (test_gpu_delta.py): rtol 1e-13 when the
    norm is fp64, else within one unit of torch.cat's promoted dtype."""
    norms, exact = np.asarray(norms, dtype=np.float64), np.asarray(exact, dtype=np.float64)
    assert norms.shape == exact.shape
    if cat == torch.float64:
        np.testing.assert_allclose(norms, exact, rtol=1e-13, atol=0)
        return
    u = torch.from_numpy(np.abs(exact)).to(cat)
    unit = np.array([float(torch.nextafter(x, torch.tensor(float("inf"), dtype=cat)) - x) for x in u])
    assert np.all(np.abs(norms - exact) <= unit), (norms, exact)
