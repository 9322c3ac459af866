"""The five native libraries, one structural check each, and the one loader.

What every library must satisfy (exports equal its header and its signature
table, a gfx950 code object that names no environment variable, its NEEDED
entries, a kernel set equal to its listed file and disjoint from the others',
no scratch) is asserted once and parametrized by library.  The expected values
are the literal table below, not read from ``build.LIBS``: the description
under test cannot vouch for itself.  Then ``_lib._load``'s four refusals with
their exact texts for each library, and ``build.up_to_date`` seeing every
header.

CPU only.  What is specific to one library (argument validation, host
arithmetic) is in test_abi.py and test_{fusedvec,segvec,clientvec}_abi.py.
"""
import ctypes
import dataclasses
import importlib.util
import os
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

from mfl_amd import _lib, build
from test_abi import ENV_PROBE_ONLY, ENV_REMOVED, _exported, declared_functions

ROOT = Path(__file__).resolve().parents[1]
HERE = Path(__file__).parent

# key -> what the built library and its binding must look like
#   headers: the exports are exactly what these declare;  declared: those names, or their count
#   tables: the _lib signature tables that type them, together exactly the declared names
#   apart: headers and tables that share no name with this library's own (the first of headers / tables)
#   absent / present: byte strings the file must not / must hold;  needs_project: a project library among NEEDED
#   kernels: (list file, count), disjoint from the files in kernels_apart;  no_scratch: no instance spills
EXPECTED = {
    "product": dict(
        path="LIB_PATH", loader="load", headers=("fedavg_amd.h",), declared=49, tables=("SIGNATURES",),
        abi=("fedavg_abi_version", "ABI_VERSION"), apart=((), ()),
        absent=ENV_REMOVED + ENV_PROBE_ONLY, present=(), needs_project=False,
        kernels=("product_kernels.txt", 114), kernels_apart=(), no_scratch=False),
    "probe": dict(
        path="PROBE_LIB_PATH", loader="load_probe", headers=("fedavg_amd_tuning.h", "fedavg_amd.h"), declared=71,
        tables=("TUNING_SIGNATURES", "SIGNATURES"), abi=("fedavg_abi_version", "ABI_VERSION"),
        apart=(("fedavg_amd.h",), ("SIGNATURES",)),
        absent=ENV_REMOVED, present=tuple(name + b"\0" for name in ENV_PROBE_ONLY), needs_project=False,
        kernels=None, kernels_apart=(), no_scratch=False),
    "fusedvec": dict(
        path="FUSEDVEC_LIB_PATH", loader="load_fusedvec", headers=("fedavg_amd_fusedvec.h",),
        declared=("fedavg_fusedvec_abi_version", "fedavg_fusedvec_last_error", "fedavg_reduce_sqdist_vec_workspace",
                  "fedavg_fused_vec_plan_of", "fedavg_reduce_sqdist_f64", "fedavg_reduce_sqdist_f16",
                  "fedavg_reduce_sqdist_bf16"),
        tables=("FUSEDVEC_SIGNATURES",), abi=("fedavg_fusedvec_abi_version", "FUSEDVEC_ABI_VERSION"),
        apart=(("fedavg_amd.h",), ("SIGNATURES",)),
        absent=ENV_REMOVED + ENV_PROBE_ONLY + (b"FEDAVG_FUSE_DISTANCES", b"FEDAVG_TUNING", b"getenv"), present=(),
        needs_project=True, kernels=("fusedvec_kernels.txt", 14), kernels_apart=("product_kernels.txt",),
        no_scratch=True),
    "segvec": dict(
        path="SEGVEC_LIB_PATH", loader="load_segvec", headers=("fedavg_amd_segvec.h",),
        declared=("fedavg_segvec_abi_version", "fedavg_segvec_last_error", "fedavg_device_round_vec_workspace",
                  "fedavg_device_round_vec_partials", "fedavg_device_round_vec_plan_of", "fedavg_device_round_f64",
                  "fedavg_device_round_f16", "fedavg_device_round_bf16"),
        tables=("SEGVEC_SIGNATURES",), abi=("fedavg_segvec_abi_version", "SEGVEC_ABI_VERSION"),
        apart=(("fedavg_amd.h", "fedavg_amd_fusedvec.h"), ("SIGNATURES", "FUSEDVEC_SIGNATURES")),
        absent=(b"getenv", b"FEDAVG_"), present=(), needs_project=False,
        kernels=("segvec_kernels.txt", 14), kernels_apart=("product_kernels.txt", "fusedvec_kernels.txt"),
        no_scratch=True),
    "clientvec": dict(
        path="CLIENTVEC_LIB_PATH", loader="load_clientvec", headers=("fedavg_amd_clientvec.h",),
        declared=("fedavg_clientvec_abi_version", "fedavg_clientvec_last_error", "fedavg_client_stats_vec_span",
                  "fedavg_client_stats_vec_workspace", "fedavg_client_stats_vec_partials", "fedavg_client_stats_bf16",
                  "fedavg_client_stats_f16", "fedavg_client_stats_f64", "fedavg_client_track_bf16",
                  "fedavg_client_track_f16", "fedavg_client_track_f64"),
        tables=("CLIENTVEC_SIGNATURES",), abi=("fedavg_clientvec_abi_version", "CLIENTVEC_ABI_VERSION"),
        apart=(("fedavg_amd.h", "fedavg_amd_tuning.h", "fedavg_amd_fusedvec.h", "fedavg_amd_segvec.h"),
               ("SIGNATURES", "TUNING_SIGNATURES", "FUSEDVEC_SIGNATURES", "SEGVEC_SIGNATURES")),
        absent=(b"getenv",), present=(), needs_project=False,
        kernels=("clientvec_kernels.txt", 10),
        kernels_apart=("product_kernels.txt", "fusedvec_kernels.txt", "segvec_kernels.txt"), no_scratch=True),
}
KEYS = tuple(EXPECTED)
WITH_KERNEL_LIST = tuple(k for k in KEYS if EXPECTED[k]["kernels"])
NO_SCRATCH = tuple(k for k in KEYS if EXPECTED[k]["no_scratch"])


@pytest.fixture(scope="module")
def built():
    build.build()


def lib_path(key):
    return getattr(build, EXPECTED[key]["path"])


@pytest.fixture(scope="module")
def inventory(built):
    spec = importlib.util.spec_from_file_location("kernel_inventory", ROOT / "scripts" / "kernel_inventory.py")
    inv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(inv)
    if not inv.have_tools():
        pytest.skip("llvm-objcopy / llvm-readelf not found")
    cache = {}
    return lambda key: cache[key] if key in cache else cache.setdefault(key, inv.inventory(lib_path(key)))


def test_the_description_names_the_five_libraries():
    assert tuple(lib.key for lib in build.LIBS) == KEYS
    for lib in build.LIBS:
        e = EXPECTED[lib.key]
        assert lib.path == lib_path(lib.key) and lib.header == e["headers"][0] and lib.abi[0] == e["abi"][0]
        assert (ROOT / "include" / lib.header).exists() and all(src.exists() for src in lib.sources)


@pytest.mark.parametrize("key", KEYS)
def test_exports_are_exactly_the_header(built, key):
    e = EXPECTED[key]
    declared = declared_functions(e["headers"])
    if isinstance(e["declared"], int):
        assert len(declared) == e["declared"]
    else:
        assert declared == sorted(e["declared"])
    assert _exported(lib_path(key)) == declared
    typed = [name for t in e["tables"] for name in getattr(_lib, t)]
    assert sorted(typed) == declared and len(set(typed)) == len(typed)
    own_header, own_table = set(declared_functions(e["headers"][:1])), set(getattr(_lib, e["tables"][0]))
    for other in e["apart"][0]:
        assert not own_header & set(declared_functions((other,))), other
    for other in e["apart"][1]:
        assert not own_table & set(getattr(_lib, other)), other
    lib = getattr(_lib, e["loader"])()
    raw = ctypes.CDLL(str(lib_path(key)))
    assert all(hasattr(raw, name) for name in declared)
    assert getattr(lib, e["abi"][0])() == getattr(_lib, e["abi"][1])


@pytest.mark.parametrize("key", KEYS)
def test_gfx950_code_object_and_no_environment_variable(built, key):
    data = lib_path(key).read_bytes()
    assert b"gfx950" in data
    for name in EXPECTED[key]["absent"]:
        assert name not in data, name
    for name in EXPECTED[key]["present"]:
        assert name in data, name


@pytest.mark.parametrize("key", KEYS)
def test_needed_entries(built, key):
    out = subprocess.run(["readelf", "-d", str(lib_path(key))], capture_output=True, text=True, check=True).stdout
    needed = "".join(ln for ln in out.splitlines() if "NEEDED" in ln)
    assert ("libfedavg_amd" in needed) == EXPECTED[key]["needs_project"]
    if EXPECTED[key]["needs_project"]:  # the product library and nothing else of the project, found next to it
        assert needed.count("libfedavg_amd") == 1 and "[libfedavg_amd.so]" in needed
        assert any("$ORIGIN" in ln for ln in out.splitlines() if "RUNPATH" in ln or "RPATH" in ln)


@pytest.mark.parametrize("key", WITH_KERNEL_LIST)
def test_kernel_set_is_the_listed_one_and_disjoint(inventory, key):
    name, count = EXPECTED[key]["kernels"]
    listed = (HERE / name).read_text().splitlines()
    built_set = sorted(inventory(key))
    assert sorted(set(built_set) - set(listed)) == [], "kernels built but not listed"
    assert sorted(set(listed) - set(built_set)) == [], "kernels listed but not built"
    assert built_set == listed and len(built_set) == count
    for other in EXPECTED[key]["kernels_apart"]:
        assert not set(listed) & set((HERE / other).read_text().splitlines()), other


@pytest.mark.parametrize("key", NO_SCRATCH)
def test_no_instance_uses_scratch(inventory, key):
    for name, row in inventory(key).items():
        assert row["scratch"] == 0 and row["vgpr_spill"] == 0 and row["sgpr_spill"] == 0, (name, row)


# ---------------------------------------------------------------- the loader's refusals, word for word
SLOT = {"product": "_lib", "probe": "_probe", "fusedvec": "_fusedvec", "segvec": "_segvec", "clientvec": "_clientvec"}
FILE = {"product": "libfedavg_amd.so", "probe": "libfedavg_amd_probe.so", "fusedvec": "libfedavg_amd_fusedvec.so",
        "segvec": "libfedavg_amd_segvec.so", "clientvec": "libfedavg_amd_clientvec.so"}
NOT_BUILT = {
    "product": "{path} not built: run __graft_entry__.build() (hipcc --offload-arch=gfx950); "
               "there is no CPU fallback for the FedAvg reduction",
    "probe": "{path} not built: run __graft_entry__.build()",
    "fusedvec": "{path} not built: run __graft_entry__.build(); there is no fallback for the "
                "one-read aggregate + distances pass of fp64 / fp16 / bf16 rows",
    "segvec": "{path} not built: run __graft_entry__.build(); there is no fallback for the "
              "zero-copy device round of fp64 / fp16 / bf16 groups",
    "clientvec": "{path} not built: run __graft_entry__.build(); there is no fallback for the "
                 "fused client statistics of bf16 / fp16 / fp64 models",
}


def refusal(key):
    with pytest.raises(_lib.FedAvgLibraryError) as info:
        getattr(_lib, EXPECTED[key]["loader"])()
    assert getattr(_lib, SLOT[key]) is None  # a refused load leaves nothing cached
    return str(info.value)


@pytest.mark.parametrize("key", KEYS)
def test_load_refuses_a_missing_file(built, monkeypatch, tmp_path, key):
    path = tmp_path / FILE[key]
    monkeypatch.setattr(_lib, EXPECTED[key]["path"], path)
    monkeypatch.setattr(_lib, SLOT[key], None)
    assert refusal(key) == NOT_BUILT[key].format(path=path)


@pytest.mark.parametrize("key", KEYS)
def test_load_refuses_a_file_that_does_not_load(built, monkeypatch, tmp_path, key):
    """An empty file.  The product and probe loaders used to let the OSError through."""
    path = tmp_path / FILE[key]
    path.touch()
    monkeypatch.setattr(_lib, EXPECTED[key]["path"], path)
    monkeypatch.setattr(_lib, SLOT[key], None)
    text = refusal(key)
    head = f"{path} does not load: "
    assert text.startswith(head) and str(path) in text[len(head):]  # the dynamic loader's own words follow


@pytest.mark.parametrize("key", KEYS)
def test_load_refuses_a_library_without_a_typed_name(built, monkeypatch, key):
    monkeypatch.setitem(getattr(_lib, EXPECTED[key]["tables"][0]), "fedavg_no_such_entry", (ctypes.c_int, []))
    monkeypatch.setattr(_lib, SLOT[key], None)
    assert refusal(key) == f"{lib_path(key)} does not export fedavg_no_such_entry"


@pytest.mark.parametrize("key", KEYS)
def test_load_refuses_another_abi_version(built, monkeypatch, key):
    """The expected version off by one.  The probe loader used to check none."""
    d = build.BY_KEY[key]
    assert d.abi == (EXPECTED[key]["abi"][0], 1)
    monkeypatch.setitem(build.BY_KEY, key, dataclasses.replace(d, abi=(d.abi[0], 2)))
    monkeypatch.setattr(_lib, SLOT[key], None)
    assert refusal(key) == "ABI version 1 != expected 2; rebuild the library"


# ---------------------------------------------------------------- up_to_date sees every header
@pytest.fixture
def scratch_build(tmp_path):
    """build.py over a copy of csrc/ and include/ with five stand-in libraries newer than every source."""
    pkg = tmp_path / "pkg"
    pkg.mkdir()
    shutil.copy(build.PKG_DIR / "build.py", pkg / "build.py")
    shutil.copytree(build.CSRC_DIR, pkg / "csrc")
    shutil.copytree(build.INCLUDE, tmp_path / "include")
    spec = importlib.util.spec_from_file_location("scratch_build_recipe", pkg / "build.py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    try:
        spec.loader.exec_module(mod)
        newest = max(p.stat().st_mtime for p in mod.sources())
        (pkg / "lib").mkdir()
        for lib in mod.LIBS:
            lib.path.touch()
            os.utime(lib.path, (newest + 10, newest + 10))
        yield mod, newest
    finally:
        del sys.modules[spec.name]


def test_up_to_date_sees_a_touched_header(scratch_build):
    mod, newest = scratch_build
    assert mod.LIB_PATH.parent.parent == mod.PKG_DIR != build.PKG_DIR
    assert mod.up_to_date()
    os.utime(mod.CSRC_DIR / "plan_table.hpp", (newest + 20, newest + 20))
    assert not mod.up_to_date()


def test_up_to_date_sees_a_header_nobody_listed(scratch_build):
    """Headers are found, not listed: one that appears in csrc/ or include/ counts at once."""
    mod, newest = scratch_build
    assert mod.up_to_date()
    for new in (mod.CSRC_DIR / "a_new_rule.hpp", mod.INCLUDE / "fedavg_amd_new.h"):
        new.write_text("// a new header\n")
        os.utime(new, (newest + 20, newest + 20))
        assert not mod.up_to_date(), new
        new.unlink()
        assert mod.up_to_date()
    os.utime(mod.CSRC_DIR / "error_state.hpp", (newest + 20, newest + 20))
    assert not mod.up_to_date()
    mod.LIBS[2].path.unlink()  # and a missing library is never up to date
    os.utime(mod.CSRC_DIR / "error_state.hpp", (newest, newest))
    assert not mod.up_to_date()
