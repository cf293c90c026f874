"""
Time of the directional extremes by a fine grid alone against a coarse grid plus refinement, on the device.

    python tools/elastic_refine_bench.py [--crystals 1000] [--directions 1024] [--angles 180] [--coarse-directions 256]
                                         [--coarse-angles 32] [--iters 20] [--warmup 5]

The tensors are the 100 of the example data set, tiled.  Both routes are the whole `elastic_properties` call, timed with
device events (median, min - max): grid only at (directions, angles), and the coarse grid with `refine=True`; then
`matten_elastic_refine` alone on the coarse grid's winners.  Last the largest difference between the two routes' extremes
over the positive definite rows (relative; absolute for Poisson's ratio) and how far the refined route lies on the
better side of the fine grid, with the refinement's status and iteration counts.  One JSON line per measurement.
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
from tools.elastic_pair_bench import PAIRS, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crystals", type=int, default=1000)
    ap.add_argument("--directions", type=int, default=1024)
    ap.add_argument("--angles", type=int, default=180)
    ap.add_argument("--coarse-directions", type=int, default=256)
    ap.add_argument("--coarse-angles", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("elastic_refine_bench: needs an MI355X, a host timing says nothing")
    raw = json.load(open(os.path.join(ROOT, "tests", "golden", "example_crystal_elasticity_tensor_n100.json")))
    full = np.array([raw["elastic_tensor_full"][k] for k in sorted(raw["elastic_tensor_full"], key=int)], dtype=np.float32)
    C = np.stack([[[t[i, j, k, l] for (k, l) in PAIRS] for (i, j) in PAIRS] for t in full]).astype(np.float64)
    B = a.crystals
    C = torch.from_numpy(np.tile(C, (-(-B // 100), 1, 1))[:B]).cuda()
    fine = dict(directions=a.directions, angles=a.angles)
    coarse = dict(directions=a.coarse_directions, angles=a.coarse_angles)
    shape = {"crystals": B, "iters": a.iters, "warmup": a.warmup}

    p = elastic.elastic_properties(C, **coarse)
    dirs, table = p.directions, torch.from_numpy(elastic.angle_table(a.coarse_angles)).cuda()
    _, _, ext_d, arg_d = ops.elastic_directional(p.compliance, p.flags, dirs)
    _, ext_p, arg_p = ops.elastic_pair(p.compliance, p.flags, dirs, table)
    for name, extra, fn in (
            ("elastic_properties, grid only", fine, lambda: elastic.elastic_properties(C, **fine)),
            ("elastic_properties, coarse grid only", coarse, lambda: elastic.elastic_properties(C, **coarse)),
            ("elastic_properties, coarse grid + refine", coarse, lambda: elastic.elastic_properties(C, refine=True, **coarse)),
            ("matten_elastic_refine", coarse,
             lambda: ops.elastic_refine(p.compliance, p.flags, dirs, ext_d, arg_d, table, ext_p, arg_p))):
        print(json.dumps({"what": name, **shape, **extra, **timed(fn, a.iters, a.warmup)}), flush=True)

    grid = elastic.elastic_properties(C, **fine).to_dict()
    ref = elastic.elastic_properties(C, refine=True, **coarse).to_dict()
    ok = grid["flags"] == 0
    for name in elastic.REFINE_NAMES:
        g, r = grid[name][ok], ref[name + "_refined"][ok]
        scale = 1.0 if name.startswith("poisson") else np.abs(g)
        sign = 1.0 if name.endswith("_max") else -1.0
        status, its = ref[name + "_refined_status"][ok], ref[name + "_refined_iterations"][ok]
        print(json.dumps({"what": f"{name}: refined (coarse start) against the fine grid", "rows": int(ok.sum()),
                          "max_difference": float((np.abs(r - g) / scale).max()),
                          "refined_better_by_at_most": float((sign * (r - g) / scale).max()),
                          "refined_worse_by_at_most": float((sign * (g - r) / scale).max()),
                          "rows_worse_than_fine_grid": int((sign * (g - r) / scale > 1e-12).sum()),
                          "status_counts": {str(s): int((status == s).sum()) for s in np.unique(status)},
                          "max_iterations": int(its.max()), "mean_iterations": float(its.mean())}), flush=True)


if __name__ == "__main__":
    main()
