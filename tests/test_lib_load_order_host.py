"""
One HIP runtime per process, whichever of torch and libmatten_hip.so is asked for first (no GPU needed).

A torch wheel that ships its own libamdhip64.so asks for it by a name that does not match the SONAME of the ROCm
installation's copy, which is what libmatten_hip.so is linked against.  Loaded in the order library -> torch, the process
used to map both runtimes; kernels registered with one cannot be launched on the other's streams, so the first launch of
`python __graft_entry__.py smoke` (build(), which loads the library, then smoke(), which imports torch) failed with
MATTEN_ELAUNCH.  `_lib.load()` imports torch before it opens the library.
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = """
import os, sys
sys.path.insert(0, {root!r})
from matten_amd import _lib
assert "torch" not in sys.modules          # the order under test: the library is asked for first
_lib.load()
import torch
seen = sorted({{os.path.realpath(l.split()[-1]) for l in open("/proc/self/maps") if "libamdhip64" in l}})
print("RUNTIMES", len(seen), seen)
"""


def test_library_before_torch_maps_one_hip_runtime():
    out = subprocess.run([sys.executable, "-c", SCRIPT.format(root=ROOT)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("RUNTIMES")][-1]
    assert line.split()[1] == "1", line
