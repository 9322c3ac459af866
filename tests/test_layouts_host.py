"""Where the addresses are formed, on the host (no GPU): ``KeyTable.collect``
and ``try_collect`` over the layout catalogue (tests/layouts.py), with the
native state_dict walk and with the Python walk alone, and the host packer fed
from the pointers they return.

A tensor that says ``is_contiguous()`` is read in place (its own
``data_ptr()``, no copy); any other is read through a contiguous copy that
``keepalive`` holds.  Which of the two a client got must not depend on the
walk that ran.
"""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import layouts as L
import mfl_amd
from mfl_amd import layout as layout_mod
from mfl_amd.layout import KeyTable

F32, F64, F16, BF16 = torch.float32, torch.float64, torch.float16, torch.bfloat16
K = 3
ODD = (0, 2)  # the clients that hold the layout


@pytest.fixture(params=["native", "python"])
def walk(request, monkeypatch):
    """Run with the native walk (when built) and with it switched off."""
    if request.param == "python":
        monkeypatch.setattr(layout_mod, "_COLLECT", [None])
    elif layout_mod._collect_ext() is None:
        pytest.skip("collect extension not built")
    return request.param


def _case(layout, dtype):
    key = L.TARGET[layout]
    lay = {key: layout}
    if layout in L.INT_TARGET:
        lay[L.INT_TARGET[layout]] = layout
    dts = {key: dtype}
    if layout == "shared":
        dts[L.TWIN[key]] = dtype
    w_locals, ref = L.model(lay, dts, K, seed=3, clients=ODD)
    return [sd for _, sd in w_locals], [sd for _, sd in ref], sorted(lay)


@pytest.mark.parametrize("dtype", [F32, F64, F16, BF16], ids=["f32", "f64", "f16", "bf16"])
@pytest.mark.parametrize("layout", list(L.LAYOUTS))
def test_catalogue_entries_equal_their_values(layout, dtype):
    dicts, ref, odd_keys = _case(layout, dtype)
    for i, (sd, rd) in enumerate(zip(dicts, ref)):
        assert list(sd) == list(L.KEY_SHAPES)
        for k, t in sd.items():
            assert t.dtype == rd[k].dtype and tuple(t.shape) == L.KEY_SHAPES[k]
            assert torch.equal(t, rd[k]), (i, k)
            expect_contig = not (i in ODD and k in odd_keys and layout in L.NON_CONTIGUOUS)
            assert t.is_contiguous() == expect_contig, (i, k)
    key = L.TARGET[layout]
    t = dicts[2][key]
    if layout == "offset1":
        assert t.storage_offset() == 1 and t.data_ptr() % 16 == t.element_size()
    if layout == "unit_dims":
        assert 997 in t.stride()
    if layout == "expanded":
        assert set(t.stride()) == {0}
    if layout == "shared":
        assert dicts[0][key] is t and dicts[2][L.TWIN[key]] is t and dicts[1][key] is not t


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("layout", list(L.LAYOUTS))
def test_collect_reads_in_place_or_through_a_kept_copy(layout, dtype, walk):
    dicts, ref, odd_keys = _case(layout, dtype)
    table = KeyTable(dicts[0])
    names = [e.name for e in table.entries]
    ptrs, keep = table.collect(dicts)
    assert ptrs.shape == (K, len(names)) and ptrs.dtype == np.int64
    raw = np.array([[sd[n].data_ptr() for n in names] for sd in dicts], dtype=np.int64)
    if layout in L.CONTIGUOUS:
        assert keep == []
        assert np.array_equal(ptrs, raw)
    else:
        assert len(keep) == len(ODD)  # one list of tensors per client that needed copies
        copies = {p: t for ts in keep for p, t in ((t.data_ptr(), t) for t in ts)}
        for i, sd in enumerate(dicts):
            for j, n in enumerate(names):
                if i in ODD and n in odd_keys:
                    assert ptrs[i, j] != raw[i, j], (i, n)
                    c = copies[int(ptrs[i, j])]  # the pointer is a kept copy's
                    assert c.is_contiguous() and c.dtype == sd[n].dtype
                    assert torch.equal(c.reshape(-1), sd[n].reshape(-1)), (i, n)
                else:
                    assert ptrs[i, j] == raw[i, j], (i, n)
    got = table.try_collect(dicts)
    if walk == "python" or layout in L.NON_CONTIGUOUS:
        assert got is None  # no native walk, or a tensor it may not read in place
    else:
        assert np.array_equal(got[0], raw) and got[1] == []


@pytest.mark.parametrize("layout", list(L.LAYOUTS))
def test_native_and_python_walks_copy_the_same_clients(layout, monkeypatch):
    if layout_mod._collect_ext() is None:
        pytest.skip("collect extension not built")
    dicts, _, _ = _case(layout, F32)
    table = KeyTable(dicts[0])
    names = [e.name for e in table.entries]
    raw = np.array([[sd[n].data_ptr() for n in names] for sd in dicts], dtype=np.int64)
    native, keep_n = table.collect(dicts)
    monkeypatch.setattr(layout_mod, "_COLLECT", [None])
    py, keep_p = table.collect(dicts)
    assert np.array_equal(native != raw, py != raw)
    assert len(keep_n) == len(keep_p)
    assert [i for i in range(K) if (native[i] != raw[i]).any()] == ([] if layout in L.CONTIGUOUS else list(ODD))


@pytest.mark.parametrize("dtype", [F32, F64, F16, BF16], ids=["f32", "f64", "f16", "bf16"])
@pytest.mark.parametrize("layout", list(L.LAYOUTS))
def test_host_packer_from_collected_pointers_is_torch_cat(layout, dtype, walk):
    """fedavg_pack_rows over collect's pointers == torch.cat of the flattened
    keys, byte for byte, per dtype group (integer keys cast as ATen promotes
    them); the GPU tests compare the device packer against this packer."""
    dicts, ref, _ = _case(layout, dtype)
    table = KeyTable(dicts[0])
    ptrs, keep = table.collect(dicts)
    lib = mfl_amd._lib.load()
    for g in table.groups.values():
        rows = torch.zeros((K, g.ld), dtype=g.dtype)
        items = table.pack_items(g, ptrs, 0, g.ld)
        mfl_amd._lib.check(lib.fedavg_pack_rows(items.ctypes.data, items.shape[0], rows.data_ptr(),
                                                rows.element_size(), 2), "fedavg_pack_rows")
        for i, rd in enumerate(ref):
            exp = torch.cat([rd[e.name].reshape(-1).to(g.dtype) for e in g.keys])
            assert exp.numel() == g.P
            assert torch.equal(rows[i, :g.P].view(torch.uint8), exp.view(torch.uint8)), (g.dtype, i)
            assert not rows[i, g.P:].view(torch.uint8).any()  # the padding is not written
    del keep
