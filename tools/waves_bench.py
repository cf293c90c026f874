#!/usr/bin/env python3
"""Group velocities, polarisations and phonon focusing (csrc/waves.hip): what the wave properties cost on the device, in
one process

  waves      ``ops.elastic_waves`` on B crystals and D directions with the three maps written, for every B of `--rows`;
  extremes   the same without the maps (``keep=False``): the extremes and the counts only;
  acoustic   ``ops.elastic_acoustic`` with its map on the same input: the phase velocities alone, for scale;
  numpy      ``acoustic_waves_host`` (``numpy.linalg.eigh`` and einsum per direction) on the first `--host-rows` crystals, on
             the CPU, with the time that rate gives for all B (a product, not a measurement, unless --host-rows >= B).

Inputs are fp64 symmetric positive definite Voigt matrices (A A^T + 6, in GPa) at 5000 kg/m^3.  Every device arm is timed
two ways, `--warmup` runs first, then `--reps` runs between device events, medians and min-max in ms:
  call     one call of the wrapper between the two events on an otherwise idle stream: at tens of microseconds this is
           the launch and the wrapper's host work (its allocations, the ctypes call) as much as the kernel;
  kernel   `--launches` calls captured into one hipGraph, the replay between the events, divided by `--launches`: the
           kernels run back to back, so this is what one launch costs the device.
The machine's calibration record comes first.  There is no pass/fail threshold: the numbers are for INTEGRATION.md, "Group
velocities, polarisations and phonon focusing".

    python tools/waves_bench.py [--rows 1000] [--directions 200] [--host-rows 50] [--reps 20] [--warmup 3] [--launches 50]
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
from matten_amd import elastic, ops, waves  # noqa: E402

DEV = "cuda:0"


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


def both(run, reps: int, warmup: int, launches: int) -> dict:
    """`call`: run() between events; `kernel`: `launches` captured runs replayed between events, per launch"""
    call = timed(run, reps, warmup)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = [run() for _ in range(launches)]      # (every launch keeps its own outputs: nothing is reused inside the graph)
    replay = timed(graph.replay, reps, warmup)
    del keep
    return {"call": call, "kernel": {k: round(v / launches, 5) for k, v in replay.items()}, "launches_per_replay": launches}


def crystals(n: int, seed: int) -> np.ndarray:
    A = np.random.default_rng(seed).standard_normal((n, 6, 6))
    return A @ A.transpose(0, 2, 1) + 6.0 * np.eye(6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1000])
    ap.add_argument("--directions", type=int, default=200)
    ap.add_argument("--host-rows", type=int, default=50)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=50)
    a = ap.parse_args()
    from pbc_graph_bench import calibration

    print(json.dumps({"calibration": calibration()}), flush=True)
    D = a.directions
    dirs = torch.from_numpy(elastic.fibonacci_hemisphere(D)).to(DEV)
    for B in a.rows:
        C = crystals(B, B)
        props = elastic.elastic_properties(C)
        voigt, flags = props.voigt, props.flags
        rho = torch.full((B,), 5000.0, dtype=torch.float64, device=DEV)
        out = ops.elastic_waves(voigt, flags, rho, dirs)
        rec = {"rows": B, "directions": D, "n_unstable": int(out[6].sum()), "n_degenerate": int(out[5].sum()),
               "output_MB": round(sum(t.numel() * t.element_size() for t in out) / 1e6, 1)}
        rec["waves"] = both(lambda: ops.elastic_waves(voigt, flags, rho, dirs), a.reps, a.warmup, a.launches)
        rec["extremes"] = both(lambda: ops.elastic_waves(voigt, flags, rho, dirs, keep=False), a.reps, a.warmup, a.launches)
        rec["acoustic"] = both(lambda: ops.elastic_acoustic(voigt, flags, rho, dirs, keep=True), a.reps, a.warmup, a.launches)
        print(json.dumps({"device": rec}), flush=True)
        H = min(a.host_rows, B)
        t0 = time.perf_counter()
        host = waves.acoustic_waves_host(C[:H], np.full(H, 5000.0), D)
        ms = 1e3 * (time.perf_counter() - t0)
        dev = out[1][:H].cpu().numpy()
        err = float(np.nanmax(np.abs(dev - host["group_velocity"]) / host["group_speed"][..., None]))
        print(json.dumps({"numpy": {"rows": H, "directions": D, "acoustic_waves_host_ms": round(ms, 1),
                                    "at_that_rate_for_all_rows_ms": round(ms * B / H, 1),
                                    "group_velocity_max_rel_diff": err}}), flush=True)


if __name__ == "__main__":
    main()
