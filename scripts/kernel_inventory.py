"""Kernel inventory of a built library (CPU only): one line per gfx950 kernel.

    python scripts/kernel_inventory.py LIB              # name, size, sha256, metadata
    python scripts/kernel_inventory.py --names LIB      # sorted demangled names only
    python scripts/kernel_inventory.py --diff OLD NEW   # added / removed / changed kernels

The library's ``.hip_fatbin`` section (llvm-objcopy) holds one offload bundle
per translation unit; each bundle's gfx950 code object is read with
llvm-readelf: the kernels' code bytes from ``.text`` by symbol, their
registers / LDS / scratch / kernarg size from the AMDGPU metadata note.  The
code bytes are hashed, never searched.
"""
from __future__ import annotations

import argparse
import hashlib
import os
import shutil
import struct
import subprocess
import sys
import tempfile
from pathlib import Path

ARCH = "gfx950"
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
META = {"vgpr": ".vgpr_count", "agpr": ".agpr_count", "sgpr": ".sgpr_count", "lds": ".group_segment_fixed_size",
        "scratch": ".private_segment_fixed_size", "kernarg": ".kernarg_segment_size",
        "vgpr_spill": ".vgpr_spill_count", "sgpr_spill": ".sgpr_spill_count"}


def tool(name: str) -> str | None:
    for d in (os.environ.get("ROCM_LLVM_BIN"), "/opt/rocm/llvm/bin", "/opt/rocm/lib/llvm/bin"):
        if d and (Path(d) / name).exists():
            return str(Path(d) / name)
    return shutil.which(name)


def have_tools() -> bool:
    return all(tool(t) for t in ("llvm-objcopy", "llvm-readelf"))


def _run(*cmd: str) -> str:
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def code_objects(lib: Path, tmp: Path) -> list[bytes]:
    """The gfx950 code object of every bundle in the library's fat binary."""
    fat = tmp / "fatbin"
    _run(tool("llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", str(lib), str(tmp / "rest"))
    data = fat.read_bytes()
    out, at = [], data.find(BUNDLE_MAGIC)
    while at >= 0:
        (n,) = struct.unpack_from("<Q", data, at + len(BUNDLE_MAGIC))
        p = at + len(BUNDLE_MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", data, p)
            triple = data[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if size and triple.rstrip("-").endswith(ARCH):
                out.append(data[at + off:at + off + size])
        at = data.find(BUNDLE_MAGIC, p)
    return out


def _metadata(notes: str) -> dict[str, dict]:
    """{kernel symbol: {field: value}} from llvm-readelf --notes (the fields of META only)."""
    kernels, cur = {}, None
    for line in notes.splitlines():
        s = line.strip()
        if s.startswith("- ") and line.startswith("  - "):  # a new entry of amdhsa.kernels
            cur = {}
            s = s[2:]
        if cur is None or ":" not in s:
            continue
        key, val = (t.strip() for t in s.split(":", 1))
        if key == ".name":
            kernels[val] = cur
        elif key in META.values():
            cur[key] = int(val)
    return kernels


def inventory(lib: Path) -> dict[str, dict]:
    """{demangled kernel name: {size, sha256, vgpr, agpr, sgpr, lds, scratch, kernarg, ...}}"""
    readelf = tool("llvm-readelf")
    inv: dict[str, dict] = {}
    with tempfile.TemporaryDirectory() as td:
        tmp = Path(td)
        for n, co in enumerate(code_objects(Path(lib), tmp)):
            path = tmp / f"co{n}"
            path.write_bytes(co)
            text = next(ln.split() for ln in _run(readelf, "-S", "-W", str(path)).splitlines() if " .text " in ln)
            fields = text[text.index(".text") + 2:]  # after "[ 7] .text PROGBITS": address, offset, size
            text_addr, text_off = int(fields[0], 16), int(fields[1], 16)
            meta = _metadata(_run(readelf, "--notes", str(path)))
            plain = _run(readelf, "--symbols", "-W", str(path)).splitlines()
            nice = _run(readelf, "--symbols", "-W", "-C", str(path)).splitlines()
            seen = set()  # .dynsym and .symtab both list a kernel
            for raw, dem in zip(plain, nice):
                f = raw.split()
                if len(f) < 8 or f[3] != "FUNC" or f[-1] not in meta or f[-1] in seen:
                    continue
                seen.add(f[-1])
                addr, size = int(f[1], 16), int(f[2])
                name = dem.split(None, 7)[7]
                at = text_off + addr - text_addr
                row = {"size": size, "sha256": hashlib.sha256(co[at:at + size]).hexdigest()}
                row.update({k: meta[f[-1]].get(v, 0) for k, v in META.items()})
                base, k = name, 2  # the same name in another translation unit (anonymous namespaces): "name [2]"
                while name in inv:
                    name = f"{base} [{k}]"
                    k += 1
                inv[name] = row
    return inv


def fmt(name: str, row: dict) -> str:
    return f"{name}\tsize={row['size']} sha256={row['sha256'][:16]} " + " ".join(f"{k}={row[k]}" for k in META)


def diff(old: dict, new: dict) -> int:
    added, removed = sorted(set(new) - set(old)), sorted(set(old) - set(new))
    changed = sorted(k for k in set(old) & set(new) if old[k] != new[k])
    for tag, names, src in (("added", added, new), ("removed", removed, old)):
        for k in names:
            print(f"{tag}\t{fmt(k, src[k])}")
    for k in changed:
        print(f"changed\t{k}")
        print(f"  old\t{fmt('', old[k]).strip()}")
        print(f"  new\t{fmt('', new[k]).strip()}")
    print(f"{len(old)} -> {len(new)} kernels: {len(added)} added, {len(removed)} removed, {len(changed)} changed")
    return 1 if added or removed or changed else 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--diff", action="store_true", help="compare two libraries")
    ap.add_argument("--names", action="store_true", help="print the sorted kernel names only")
    ap.add_argument("libs", nargs="+", type=Path)
    args = ap.parse_args()
    if not have_tools():
        print("llvm-objcopy / llvm-readelf not found", file=sys.stderr)
        return 2
    if args.diff:
        if len(args.libs) != 2:
            ap.error("--diff takes OLD and NEW")
        return diff(inventory(args.libs[0]), inventory(args.libs[1]))
    for lib in args.libs:
        inv = inventory(lib)
        for k in sorted(inv):
            print(k if args.names else fmt(k, inv[k]))
        if not args.names:
            print(f"{len(inv)} kernels in {lib}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
