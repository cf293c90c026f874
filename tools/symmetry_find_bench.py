#!/usr/bin/env python3
"""The symmetry search of csrc/spacegroup.hip against its numpy restatement

  device  ``symmetry.find_symmetry`` on packed arrays that already live on the device (``ops.lattice_group`` +
          ``ops.crystal_symmetry`` and the row_struct arithmetic), timed with HIP events after warm-up, median of `--reps`;
  host    ``symmetry.find_symmetry_host`` on a sample of `--host-sample` of the same structures (wall clock, scaled to the
          whole set: the restatement tests every (operation, translation) pair in full and is minutes per 1e4 crystals).

Sets: `--fcc` (default 1000) fcc-64 crystals of ``data/synthetic.py`` (4x4x4 primitive cells, random species and 0.02 A
of thermal noise: the lattice has 48 operations, the crystal one; nearly every candidate dies at its first atom) and the
crystals of tests/golden/example_crystal_elasticity_tensor_n100.json (2 to 20 atoms, real space groups).  Prints per set
the distribution of orders and flags, that the sample agrees with the restatement, and the timings; one JSON line at the
end.  There is no pass/fail threshold: the numbers are for docs/LAB_NOTES.md and INTEGRATION.md "Finding a crystal's
symmetry".

    python tools/symmetry_find_bench.py [--fcc 1000] [--host-sample 20] [--reps 20] [--warmup 3] [--symprec 1e-3]
"""
import argparse
import collections
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from matten_amd.data import synthetic  # noqa: E402
from matten_amd.data.io import structures_from_json  # noqa: E402
from matten_amd.predict import pack_structures  # noqa: E402
from matten_amd.symmetry import find_symmetry, find_symmetry_host  # noqa: E402

DEV = "cuda:0"


def bench(name: str, structures, symprec: float, reps: int, warmup: int, host_sample: int) -> dict:
    pos, cell, Z, ptr, keep, failed = pack_structures(structures)
    dev = {k: torch.as_tensor(v, device=DEV) for k, v in dict(pos=pos, cell=cell, Z=Z, ptr=ptr).items()}
    for _ in range(warmup):
        sym = find_symmetry(**dev, symprec=symprec)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        sym = find_symmetry(**dev, symprec=symprec)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    h = sym.host()
    sample = np.linspace(0, len(keep) - 1, min(host_sample, len(keep))).astype(int)
    t0 = time.perf_counter()
    agree = True
    for b in sample:
        lo, hi = int(ptr[b]), int(ptr[b + 1])
        want = find_symmetry_host(pos=pos[lo:hi], cell=cell[b:b + 1], Z=Z[lo:hi], ptr=np.array([0, hi - lo]), symprec=symprec)
        agree = agree and (int(want.n_rot[0]), int(want.n_trans[0]), int(want.flags[0])) == (int(h.n_rot[b]), int(h.n_trans[b]), int(h.flags[b])) \
            and np.array_equal(want.rotations_int[0], h.rotations_int[b]) \
            and np.array_equal(np.where(want.src < 0, -1, want.src + lo), h.src[:, lo:hi])
    host_s = time.perf_counter() - t0
    res = {"set": name, "crystals": len(keep), "atoms": int(ptr[-1]), "symprec": symprec,
           "device_median_ms": round(ms[len(ms) // 2], 4), "device_min_ms": round(ms[0], 4), "device_max_ms": round(ms[-1], 4),
           "host_sample": len(sample), "host_sample_s": round(host_s, 3),
           "host_whole_set_s_scaled": round(host_s * len(keep) / max(1, len(sample)), 2), "sample_agrees": bool(agree),
           "orders": dict(sorted(collections.Counter(h.n_rot.tolist()).items())),
           "pure_translations": dict(sorted(collections.Counter(h.n_trans.tolist()).items())),
           "flags": dict(sorted(collections.Counter(h.flags.tolist()).items()))}
    print(json.dumps(res))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fcc", type=int, default=1000)
    ap.add_argument("--host-sample", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--symprec", type=float, default=1e-3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    golden = os.path.join(ROOT, "tests", "golden", "example_crystal_elasticity_tensor_n100.json")
    results = [bench(f"fcc64 x {args.fcc}", synthetic.fcc64_structures(args.fcc), args.symprec, args.reps, args.warmup, args.host_sample),
               bench("example_crystal_elasticity_tensor_n100", structures_from_json(golden), args.symprec, args.reps, args.warmup,
                     args.host_sample)]
    print(json.dumps({"symmetry_find_bench": results}))


if __name__ == "__main__":
    main()
