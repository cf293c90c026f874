"""
Time of the adjoints of the directional and acoustic kernels on the device, next to their forwards.

    python tools/elastic_dir_grad_bench.py [--crystals 1000] [--directions 1024] [--iters 20] [--warmup 5]

The tensors are the 100 of the example data set, tiled; every kernel is timed alone with device events around its one
launch (median, min - max), with the maps' upstream gradients (the most a launch reads) and with the extremes' alone; then
a forward and backward of `elastic_moduli` under a loss on the Debye temperature and the largest Young's modulus.  One JSON
line per measurement.
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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("elastic_dir_grad_bench: needs an MI355X, a host timing says nothing")
    raw = json.load(open(os.path.join(ROOT, "tests", "golden", "example_crystal_elasticity_tensor_n100.json")))
    full = np.array([raw["elastic_tensor_full"][k] for k in sorted(raw["elastic_tensor_full"], key=int)], dtype=np.float32)
    C = np.stack([[[t[i, j, k, l] for (k, l) in PAIRS] for (i, j) in PAIRS] for t in full]).astype(np.float64)
    B, D = a.crystals, a.directions
    C = torch.from_numpy(np.tile(C, (-(-B // 100), 1, 1))[:B]).cuda()
    rho = torch.linspace(2000.0, 12000.0, B, dtype=torch.float64).cuda()
    nd = torch.linspace(3e28, 9e28, B, dtype=torch.float64).cuda()
    p = elastic.elastic_properties(C)
    dirs = torch.from_numpy(elastic.fibonacci_hemisphere(D)).cuda()
    _, _, _, arg_d = ops.elastic_directional(p.compliance, p.flags, dirs)
    _, _, arg_a, _ = ops.elastic_acoustic(p.voigt, p.flags, rho, dirs)
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64, device="cuda")
    gy, gb, gxd, gv, gxa = rnd(B, D), rnd(B, D), rnd(B, 4), rnd(B, D, 3), rnd(B, 3)

    def step():
        c = C.clone().requires_grad_()
        q = elastic.elastic_moduli(c, directions=D, density=rho, number_density=nd)
        (q.debye_temperature.sum() + q.young_max.sum()).backward()
        return c.grad

    shape = {"crystals": B, "directions": D, "iters": a.iters, "warmup": a.warmup}
    for name, fn in (
            ("matten_elastic_directional", lambda: ops.elastic_directional(p.compliance, p.flags, dirs)),
            ("matten_elastic_directional_bwd, maps", lambda: ops.elastic_directional_bwd(p.compliance, p.flags, dirs, gy, gb, gxd, arg_d)),
            ("matten_elastic_directional_bwd, extremes alone",
             lambda: ops.elastic_directional_bwd(p.compliance, p.flags, dirs, None, None, gxd, arg_d)),
            ("matten_elastic_acoustic", lambda: ops.elastic_acoustic(p.voigt, p.flags, rho, dirs)),
            ("matten_elastic_acoustic_bwd, maps", lambda: ops.elastic_acoustic_bwd(p.voigt, p.flags, rho, dirs, 1e9, gv, gxa, arg_a)),
            ("matten_elastic_acoustic_bwd, extremes and sum alone",
             lambda: ops.elastic_acoustic_bwd(p.voigt, p.flags, rho, dirs, 1e9, None, gxa, arg_a)),
            ("elastic_moduli(directions, density, number_density) forward + backward", step)):
        print(json.dumps({"what": name, **shape, **timed(fn, a.iters, a.warmup)}), flush=True)


if __name__ == "__main__":
    main()
