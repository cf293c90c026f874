#!/usr/bin/env python3
"""Kelvin moduli of elasticity tensors: the kernels of csrc/kelvin.hip against what a user would otherwise write on the
device, in one process with the arms alternating, at every `--rows` count

  arm K   ``elastic_moduli(..., kelvin=True)``'s Kelvin step alone: ``autograd.ElasticKelvinFn`` on Voigt matrices and
          clear flags (matten_elastic_kelvin; with the adjoint: matten_elastic_kelvin_bwd through autograd);
  arm T   ``torch.linalg.eigh`` in fp64 on the Mandel matrices (autograd for the adjoint).

Inputs are fp64 [B,6,6] symmetric matrices (unit-size Gaussian entries plus 6 on the diagonal).  "forward" is the moduli
and the vectors; "forward + adjoint" adds the gradient of the squared stability penalty at margin 6 with respect to the
input.  Every arm runs `--warmup` times, then `--reps` times between device events, the arms alternating rep by rep; medians
and min-max in ms.  The machine's calibration record comes first.  There is no pass/fail threshold: the numbers are for
docs/LAB_NOTES.md "Kelvin moduli and mechanical stability".

    python tools/kelvin_bench.py [--rows 100000 1000000] [--reps 20] [--warmup 5] [--budget 30]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from matten_amd.autograd import ElasticKelvinFn  # noqa: E402
from matten_amd.elastic import MANDEL_WEIGHT  # noqa: E402

DEV = "cuda:0"
MARGIN = 6.0


def bench(n: int, reps: int, warmup: int, budget: float) -> dict:
    g = torch.Generator(device=DEV).manual_seed(n)
    x = torch.randn(n, 6, 6, dtype=torch.float64, device=DEV, generator=g)
    c = 0.5 * (x + x.transpose(1, 2)) + 6.0 * torch.eye(6, dtype=torch.float64, device=DEV)
    flags = torch.zeros(n, dtype=torch.int32, device=DEV)
    w = torch.tensor(MANDEL_WEIGHT, device=DEV)

    def torch_arm(t):
        return torch.linalg.eigh(w * (0.5 * (t + t.transpose(1, 2))))

    def kernel_arm(t):
        return ElasticKelvinFn.apply(t, flags)[:2]

    def forward(arm):
        with torch.no_grad():
            arm(c)

    def both(arm):
        t = c.detach().requires_grad_()
        lam = arm(t)[0]
        (torch.relu(MARGIN - lam) ** 2).mean().backward()

    cases = {"forward": forward, "forward+adjoint": both}
    arms = {"kernel": kernel_arm, "torch_eigh": torch_arm}
    out = {"rows": n}
    for case, run in cases.items():
        slowest = 0.0
        for arm in arms.values():
            for _ in range(warmup):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(arm)
                torch.cuda.synchronize()
                slowest = max(slowest, time.perf_counter() - t0)
        # (torch's batched eigh is the slow arm: the repetitions are cut so that a case stays within `budget` seconds)
        n_reps = max(3, min(reps, int(budget / max(slowest, 1e-9) / 2)))
        out[f"{case}/reps"] = n_reps
        times = {name: [] for name in arms}
        for _ in range(n_reps):
            for name, arm in arms.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                run(arm)
                b.record()
                times[name].append((a, b))
        torch.cuda.synchronize()
        for name, evs in times.items():
            ms = sorted(a.elapsed_time(b) for a, b in evs)
            out[f"{case}/{name}"] = {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--budget", type=float, default=30.0, help="seconds a (size, case) may take: caps the repetitions")
    a = ap.parse_args()
    from pbc_graph_bench import calibration

    print(json.dumps({"calibration": calibration()}), flush=True)
    for n in a.rows:
        print(json.dumps(bench(n, a.reps, a.warmup, a.budget)), flush=True)


if __name__ == "__main__":
    main()
