"""
Time of the pair (shear modulus, Poisson's ratio) and acoustic (Christoffel velocities) kernels on the device.

    python tools/elastic_pair_bench.py [--crystals 1000] [--directions 1024] [--angles 180] [--iters 20] [--warmup 5]

The tensors are the 100 of the example data set, tiled; every kernel is timed alone with device events around its one
launch (median, min - max), then the whole `elastic_properties` call.  One JSON line per measurement.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from matten_amd import elastic, ops  # noqa: E402

PAIRS = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crystals", type=int, default=1000)
    ap.add_argument("--directions", type=int, default=1024)
    ap.add_argument("--angles", type=int, default=180)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("elastic_pair_bench: needs an MI355X, a host timing says nothing")
    raw = json.load(open(os.path.join(ROOT, "tests", "golden", "example_crystal_elasticity_tensor_n100.json")))
    full = np.array([raw["elastic_tensor_full"][k] for k in sorted(raw["elastic_tensor_full"], key=int)], dtype=np.float32)
    C = np.stack([[[t[i, j, k, l] for (k, l) in PAIRS] for (i, j) in PAIRS] for t in full]).astype(np.float64)
    B, D, M = a.crystals, a.directions, a.angles
    C = torch.from_numpy(np.tile(C, (-(-B // 100), 1, 1))[:B]).cuda()
    rho = torch.linspace(2000.0, 12000.0, B, dtype=torch.float64).cuda()
    p = elastic.elastic_properties(C)
    dirs = torch.from_numpy(elastic.fibonacci_hemisphere(D)).cuda()
    table = torch.from_numpy(elastic.angle_table(M)).cuda()
    shape = {"crystals": B, "directions": D, "angles": M, "iters": a.iters, "warmup": a.warmup}
    for name, fn in (("matten_elastic_pair", lambda: ops.elastic_pair(p.compliance, p.flags, dirs, table)),
                     ("matten_elastic_pair, maps kept", lambda: ops.elastic_pair(p.compliance, p.flags, dirs, table, keep=True)),
                     ("matten_elastic_directional", lambda: ops.elastic_directional(p.compliance, p.flags, dirs)),
                     ("matten_elastic_acoustic", lambda: ops.elastic_acoustic(p.voigt, p.flags, rho, dirs)),
                     ("matten_elastic_acoustic, maps kept", lambda: ops.elastic_acoustic(p.voigt, p.flags, rho, dirs, keep=True)),
                     ("elastic_properties(directions)", lambda: elastic.elastic_properties(C, directions=D)),
                     ("elastic_properties(directions, angles, density)",
                      lambda: elastic.elastic_properties(C, directions=D, angles=M, density=rho))):
        print(json.dumps({"what": name, **shape, **timed(fn, a.iters, a.warmup)}), flush=True)


if __name__ == "__main__":
    main()
