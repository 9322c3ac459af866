"""Build recipe for the native libraries (gfx950 only); ``ALL_LIBS`` describes them.

    python -m mfl_amd.build           # or __graft_entry__.build()

``LIBS`` is the five libraries tests/test_native_libs.py pins by name, with
``up_to_date()`` over exactly those.  ``LATER_LIBS`` is the sixth and
``ALL_LIBS = LIBS + LATER_LIBS`` / ``BY_KEY`` the six, pinned in turn by
tests/test_clientstep_abi.py.  A library added since is described with the
same dataclass in ``NEWER_LIBS``, and ``EVERY_LIB = ALL_LIBS + NEWER_LIBS`` /
``DESCRIBED`` (by key) are the seven that tests/test_clientadam_abi.py pins.
The eighth, and any after it, is described in ``EXTRA_LIBS`` / ``EXTRA_BY_KEY``
(a new one goes there), and ``BUILT_LIBS = EVERY_LIB + EXTRA_LIBS`` is what
``sources()``, the up-to-date rule and ``build()`` cover; ``_lib`` loads a
library from the by-key table that holds it.

Every translation unit of ``BUILT_LIBS`` is compiled in parallel with hipcc for
``--offload-arch=gfx950`` and each library is linked into ``lib/`` inside the
package (in-tree, so the built libraries travel with the repo snapshot to the
GPU box).  ``-ffp-contract=off`` keeps every multiply and add separately
rounded (bit parity with the reference's ATen CPU ops,
fedavg_trainer.py:455-457).

The tuning hooks (``include/fedavg_amd_tuning.h``: kernel variants, probes)
are NOT in the product library: only the probe library, which scripts/ and the
variant tests load, is compiled with ``-DFEDAVG_TUNING``.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
from dataclasses import dataclass
from pathlib import Path

PKG_DIR = Path(__file__).resolve().parent
REPO_DIR = PKG_DIR.parent
CSRC_DIR = PKG_DIR / "csrc"
CSRC_COLLECT = CSRC_DIR / "fedavg_collect_ext.cpp"
COLLECT_NAME = "fedavg_collect_ext"
INCLUDE = REPO_DIR / "include"
LIB_DIR = PKG_DIR / "lib"
ARCH = "gfx950"


@dataclass(frozen=True)
class NativeLib:
    """One native library: what build() compiles and links, and what
    ``_lib._load`` / ``_lib._check`` need to load it and report its errors
    (its signature table is ``_lib``'s, reached by ``key``)."""

    key: str
    file: str  # under lib/
    header: str  # the public header under include/
    units: tuple  # translation units under csrc/, one object each in lib/<obj_dir>/
    abi: tuple  # (the ABI-version symbol, the value the binding expects)
    last_error: str  # the symbol that returns the calling thread's message
    no_fallback: str  # what follows "<path> not built: run __graft_entry__.build()" when the file is missing
    defines: tuple = ()  # extra compile flags
    link: tuple = ()  # extra link arguments
    needs: str = ""  # key of the library that must be loaded first
    obj_dir: str = "obj"
    reuse: tuple = ()  # (key, unit): objects another library's compile already made, linked after this one's own

    @property
    def path(self) -> Path:
        return LIB_DIR / self.file

    @property
    def sources(self):
        return [CSRC_DIR / u for u in self.units]

    def obj(self, unit: str) -> Path:
        return LIB_DIR / self.obj_dir / (unit + ".o")


_PRODUCT_UNITS = ("fedavg_reduce.hip", "fedavg_dist.hip", "fedavg_fpf.hip", "fedavg_xfer.hip", "fedavg_pack.hip",
                  "fedavg_segments.hip", "fedavg_client.hip")

LIBS = (
    # production kernels + C ABI, the distance pass, FPF, transfer, device packing, zero-copy segment kernels, the
    # client's per-iteration statistics and the native host packer
    NativeLib("product", "libfedavg_amd.so", "fedavg_amd.h", (*_PRODUCT_UNITS, "fedavg_host.cpp"),
              abi=("fedavg_abi_version", 1), last_error="fedavg_last_error",
              no_fallback=" (hipcc --offload-arch=gfx950); there is no CPU fallback for the FedAvg reduction"),
    # the same sources with the tuning hooks, plus the variants (the host packer has no hooks: the product's object)
    NativeLib("probe", "libfedavg_amd_probe.so", "fedavg_amd_tuning.h", (*_PRODUCT_UNITS, "fedavg_variants.hip"),
              abi=("fedavg_abi_version", 1), last_error="fedavg_last_error", no_fallback="",
              defines=("-DFEDAVG_TUNING=1",), obj_dir="obj_probe", reuse=(("product", "fedavg_host.cpp"),)),
    # the one-read aggregate + :291 pass of fp64 / fp16 / bf16 rows; its two-pass route calls the product library,
    # found next to it at load time
    NativeLib("fusedvec", "libfedavg_amd_fusedvec.so", "fedavg_amd_fusedvec.h", ("fedavg_fused_vec.hip",),
              abi=("fedavg_fusedvec_abi_version", 1), last_error="fedavg_fusedvec_last_error",
              no_fallback="; there is no fallback for the one-read aggregate + distances pass of fp64 / fp16 / bf16 rows",
              link=(f"-L{LIB_DIR}", "-l:libfedavg_amd.so", "-Wl,-rpath,$ORIGIN"), needs="product"),
    # a device-resident round's fp64 / fp16 / bf16 group from the clients' own tensors; calls no other library
    NativeLib("segvec", "libfedavg_amd_segvec.so", "fedavg_amd_segvec.h", ("fedavg_segments_vec.hip",),
              abi=("fedavg_segvec_abi_version", 1), last_error="fedavg_segvec_last_error",
              no_fallback="; there is no fallback for the zero-copy device round of fp64 / fp16 / bf16 groups"),
    # the client's per-iteration statistics for bf16 / fp16 / fp64 models; calls no other library
    NativeLib("clientvec", "libfedavg_amd_clientvec.so", "fedavg_amd_clientvec.h", ("fedavg_client_vec.hip",),
              abi=("fedavg_clientvec_abi_version", 1), last_error="fedavg_clientvec_last_error",
              no_fallback="; there is no fallback for the fused client statistics of bf16 / fp16 / fp64 models"),
)
# the library added after the five above
LATER_LIBS = (
    # the client's plain SGD step fused with the weight statistics, fp32 / bf16 / fp16 / fp64; calls no other library
    NativeLib("clientstep", "libfedavg_amd_clientstep.so", "fedavg_amd_clientstep.h", ("fedavg_client_step.hip",),
              abi=("fedavg_clientstep_abi_version", 1), last_error="fedavg_clientstep_last_error",
              no_fallback="; there is no fallback for the fused client SGD step"),
)
ALL_LIBS = LIBS + LATER_LIBS
BY_KEY = {lib.key: lib for lib in ALL_LIBS}
# libraries added after those six (a new one goes here: see the module docstring)
NEWER_LIBS = (
    # the client's Adam step (amsgrad) fused with the weight statistics, fp32 / bf16 / fp16 / fp64; calls no other
    # library
    NativeLib("clientadam", "libfedavg_amd_clientadam.so", "fedavg_amd_clientadam.h", ("fedavg_client_adam.hip",),
              abi=("fedavg_clientadam_abi_version", 1), last_error="fedavg_clientadam_last_error",
              no_fallback="; there is no fallback for the fused client Adam step"),
)
EVERY_LIB = ALL_LIBS + NEWER_LIBS
DESCRIBED = {lib.key: lib for lib in EVERY_LIB}
LIB_PATH, PROBE_LIB_PATH, FUSEDVEC_LIB_PATH, SEGVEC_LIB_PATH, CLIENTVEC_LIB_PATH = (lib.path for lib in LIBS)
CLIENTSTEP_LIB_PATH = BY_KEY["clientstep"].path
CLIENTADAM_LIB_PATH = DESCRIBED["clientadam"].path
# libraries added after those seven (a new one goes here: see the module docstring)
EXTRA_LIBS = (
    # the :71 guard on the device and the SGD / Adam steps behind its gate, fp32 / bf16 / fp64; calls no other library
    NativeLib("clientloop", "libfedavg_amd_clientloop.so", "fedavg_amd_clientloop.h", ("fedavg_client_loop.hip",),
              abi=("fedavg_clientloop_abi_version", 1), last_error="fedavg_clientloop_last_error",
              no_fallback="; there is no fallback for the device-side client guard and the gated steps"),
)
EXTRA_BY_KEY = {lib.key: lib for lib in EXTRA_LIBS}
BUILT_LIBS = EVERY_LIB + EXTRA_LIBS
CLIENTLOOP_LIB_PATH = EXTRA_BY_KEY["clientloop"].path

HIPCC_FLAGS = [
    f"--offload-arch={ARCH}",
    "-O3",
    "-std=c++17",
    "-fPIC",
    "-ffp-contract=off",
    "-fno-fast-math",
    "-Wall",
    "-pthread",
    # host code only: loops start on a 64-byte line.  stage_device_round's 61-byte pointer-fill loop (staging.hpp)
    # ran 22 % slower in a build that happened to place it across one (resnet56 x 100 device round: 48 vs 42 us)
    "-Xarch_host",
    "-falign-loops=64",
]


def hipcc_path() -> str:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cand and Path(cand).exists():
            return cand
    raise RuntimeError("hipcc not found (ROCm toolchain required to build libfedavg_amd.so)")


def sources():
    """Everything a library can depend on: every translation unit, every
    header in csrc/ and include/ (found, not listed) and this recipe."""
    units = dict.fromkeys(src for lib in BUILT_LIBS for src in lib.sources)
    return [*units, *sorted(CSRC_DIR.glob("*.hpp")), *sorted(INCLUDE.glob("*.h")), Path(__file__)]


def up_to_date() -> bool:
    newest = max(p.stat().st_mtime for p in sources())
    return all(lib.path.exists() and lib.path.stat().st_mtime >= newest for lib in LIBS)


def later_up_to_date() -> bool:
    """The same rule for ``LATER_LIBS``, ``NEWER_LIBS`` and ``EXTRA_LIBS``: each built and no older than the newest
    source."""
    newest = max(p.stat().st_mtime for p in sources())
    return all(lib.path.exists() and lib.path.stat().st_mtime >= newest
               for lib in LATER_LIBS + NEWER_LIBS + EXTRA_LIBS)


def collect_ext_path() -> Path:
    return LIB_DIR / f"{COLLECT_NAME}.so"


def build_collect_ext(force: bool = False, verbose: bool = False) -> Path:
    """torch C++ extension for the host-side state_dict walk (layout.KeyTable.collect)."""
    out = collect_ext_path()
    if not force and out.exists() and out.stat().st_mtime >= CSRC_COLLECT.stat().st_mtime:
        return out
    from torch.utils.cpp_extension import load

    LIB_DIR.mkdir(parents=True, exist_ok=True)
    load(name=COLLECT_NAME, sources=[str(CSRC_COLLECT)], build_directory=str(LIB_DIR),
         extra_cflags=["-O2", "-fopenmp"], extra_ldflags=["-fopenmp"], verbose=verbose)
    return out


def _compile_all(jobs, verbose):
    """jobs: [(src, obj, extra_flags)] compiled in parallel (at most 16 at once)."""
    hipcc = hipcc_path()
    errors = []
    pending = list(jobs)
    running = []
    limit = max(1, min(16, os.cpu_count() or 8))
    while pending or running:
        while pending and len(running) < limit:
            src, obj, extra = pending.pop(0)
            cmd = [hipcc, *HIPCC_FLAGS, *extra, f"-I{INCLUDE}", "-c", "-o", str(obj), str(src)]
            if verbose:
                print(" ".join(cmd))
            running.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
        src, proc = running.pop(0)
        out, err = proc.communicate()
        if proc.returncode != 0:
            errors.append(f"{src.name}: hipcc failed ({proc.returncode}):\n{out}\n{err}")
    if errors:
        raise RuntimeError("\n".join(errors))


def _link(objs, lib_path, verbose, extra=()):
    tmp = lib_path.with_suffix(".so.tmp")
    cmd = [hipcc_path(), f"--offload-arch={ARCH}", "-shared", "-fPIC", "-pthread", "-o", str(tmp), *map(str, objs),
           *extra]
    if verbose:
        print(" ".join(cmd))
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        raise RuntimeError(f"link failed ({proc.returncode}):\n{proc.stdout}\n{proc.stderr}")
    os.replace(tmp, lib_path)


def build(force: bool = False, verbose: bool = False) -> Path:
    """Build every library of ``BUILT_LIBS``; returns the product library's path."""
    if not force and up_to_date() and later_up_to_date():
        return LIB_PATH
    for lib in BUILT_LIBS:
        (LIB_DIR / lib.obj_dir).mkdir(parents=True, exist_ok=True)
    _compile_all([(CSRC_DIR / u, lib.obj(u), list(lib.defines)) for lib in BUILT_LIBS for u in lib.units], verbose)
    by_key = {**DESCRIBED, **EXTRA_BY_KEY}
    for lib in BUILT_LIBS:  # in order: a library links after the one its link arguments name
        objs = [lib.obj(u) for u in lib.units] + [by_key[key].obj(u) for key, u in lib.reuse]
        _link(objs, lib.path, verbose, extra=lib.link)
    return LIB_PATH


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
