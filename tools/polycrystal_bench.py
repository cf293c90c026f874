#!/usr/bin/env python3
"""Polycrystal moduli (Hashin-Shtrikman bounds, self-consistent estimate): the kernels of csrc/polycrystal.hip against the
numpy statement of the same algorithm, at every `--rows` count

  device  ``autograd.ElasticPolycrystalFn`` on Voigt matrices, clear flags and the Kelvin decomposition made beforehand
          (matten_elastic_polycrystal; with the adjoint: matten_elastic_polycrystal_bwd through autograd).  "with Kelvin"
          adds the matten_elastic_kelvin launch that ``elastic_properties(polycrystal=True)`` makes when ``kelvin`` is off.
  host    ``elastic.polycrystal_host`` (and ``polycrystal_bwd_host``) in numpy fp64 on one core, on the first
          `--host-rows` rows, scaled to the row count (it is linear in the rows).

Inputs are fp64 [B,6,6] positive definite matrices A A^T + s 1, s in 10^[-2,1].  The device runs `--warmup` times, then
`--reps` times between device events; medians and min-max in ms.  The machine's calibration record comes first.  There is
no pass/fail threshold: the numbers are for docs/LAB_NOTES.md "Polycrystal bounds and the self-consistent estimate".

    python tools/polycrystal_bench.py [--rows 1000 100000] [--reps 20] [--warmup 3] [--host-rows 1000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from matten_amd import elastic, ops  # noqa: E402
from matten_amd.autograd import ElasticPolycrystalFn  # noqa: E402

DEV = "cuda:0"


def tensors(n: int) -> np.ndarray:
    rng = np.random.default_rng(n)
    A = rng.standard_normal((n, 6, 6))
    return A @ A.transpose(0, 2, 1) + (10.0 ** rng.uniform(-2.0, 1.0, size=n))[:, None, None] * np.eye(6)


def timed(run, reps: int, warmup: int) -> dict:
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    evs = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        evs.append((a, b))
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in evs)
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


def bench(n: int, reps: int, warmup: int, host_rows: int) -> dict:
    C = tensors(n)
    voigt = torch.from_numpy(C).to(DEV)
    flags = torch.zeros(n, dtype=torch.int32, device=DEV)
    moduli, vectors, _ = ops.elastic_kelvin(voigt, flags, want_dilatation=False)

    def forward():
        with torch.no_grad():
            ops.elastic_polycrystal(voigt, flags, moduli, vectors)

    def forward_with_kelvin():
        with torch.no_grad():
            m, v, _ = ops.elastic_kelvin(voigt, flags, want_dilatation=False)
            ops.elastic_polycrystal(voigt, flags, m, v)

    def both():
        t = voigt.detach().requires_grad_()
        out = ElasticPolycrystalFn.apply(t, flags, moduli, vectors, 64, 1e-12, 200)[0]
        (out[:, 2] + out[:, 3]).sum().backward()

    out = {"rows": n, "forward": timed(forward, reps, warmup), "forward with Kelvin": timed(forward_with_kelvin, reps, warmup),
           "forward+adjoint": timed(both, reps, warmup)}
    status = ops.elastic_polycrystal(voigt, flags, moduli, vectors)[2]
    out["sc_iterations"] = {"mean": round(status[:, 1].double().mean().item(), 2), "max": int(status[:, 1].max())}
    out["sc_not_converged"] = int((status[:, 0] != 0).sum())
    h = min(n, host_rows)
    t0 = time.perf_counter()
    elastic.polycrystal_host(C[:h])
    t1 = time.perf_counter()
    elastic.polycrystal_bwd_host(C[:h], np.ones((h, 2)))
    t2 = time.perf_counter()
    out["host"] = {"rows_timed": h, "forward_ms_scaled": round((t1 - t0) * 1e3 * n / h, 1),
                   "forward+adjoint_ms_scaled": round((t2 - t0) * 1e3 * n / h, 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1000, 100_000])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-rows", type=int, default=1000)
    a = ap.parse_args()
    from pbc_graph_bench import calibration

    print(json.dumps({"calibration": calibration()}), flush=True)
    for n in a.rows:
        print(json.dumps(bench(n, a.reps, a.warmup, a.host_rows)), flush=True)


if __name__ == "__main__":
    main()
