"""Record tests/launch_geometry_parent.json on an MI355X.

    python scripts/record_launch_geometry.py COMMIT [OUT.json]

Run it with the libraries of COMMIT built: the file holds every plan,
workspace and partials figure tests/test_gpu_launch_geometry.py compares
against, and the commit they were recorded at.  A refactor's fixture is
recorded at its PARENT commit, never from the changed tree: regenerating it
from the code under test makes the test vacuous.
"""
import json
import re
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import torch

    import test_gpu_launch_geometry as G
    from mfl_amd import _lib

    commit = sys.argv[1]
    assert re.fullmatch(r"[0-9a-f]{40}", commit), "the full hash of the commit whose libraries are built"
    out = Path(sys.argv[2]) if len(sys.argv) > 2 else G.FIXTURE
    assert torch.cuda.is_available(), "the rows and zero-copy figures come from occupancy queries: needs the MI355X"
    torch.cuda.set_device(0)
    rec = {"recorded_at_commit": commit, "device": torch.cuda.get_device_name(0),
           "rows": G.collect_rows(_lib.load()), "segments": G.collect_segments(_lib.load()),
           "fusedvec": G.collect_fusedvec(_lib.load_fusedvec())}
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(rec, separators=(",", ":")) + "\n")
    print(f"wrote {out}: {out.stat().st_size} bytes")


if __name__ == "__main__":
    main()
