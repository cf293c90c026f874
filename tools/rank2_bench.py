#!/usr/bin/env python3
"""Shielding parameters of per-atom tensors: the two kernels of csrc/rank2.hip against what a user would otherwise write on
the device, in one process with the arms alternating, at every `--atoms` count

  arm K   ``rank2_invariants`` (matten_rank2_props; with the adjoint: matten_rank2_props_bwd through autograd);
  arm T   ``torch.linalg.eigh`` on the symmetrised batch plus the scalar formulas in torch (autograd for the adjoint).

Inputs are fp64 [N,3,3] general tensors (an isotropic part in +-500 plus unit-size entries).  "forward" is the values, the
axes and the five scalars; "forward + adjoint" adds the gradient of a fixed linear functional of the values and the scalars
with respect to the input.  Every arm runs `--warmup` times, then `--reps` times between device events, the arms
alternating rep by rep; medians and min-max in ms.  The machine's calibration record comes first.  There is no pass/fail
threshold: the numbers are for docs/LAB_NOTES.md "Per-atom shielding parameters".

    python tools/rank2_bench.py [--atoms 100000 1000000] [--reps 20] [--warmup 5] [--budget 30]
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
from matten_amd.rank2 import rank2_invariants  # noqa: E402

DEV = "cuda:0"


def torch_arm(t):
    """the same outputs with torch.linalg.eigh and elementwise torch"""
    lam, axes = torch.linalg.eigh(0.5 * (t + t.transpose(1, 2)))
    iso = lam.sum(1) / 3.0
    span = lam[:, 2] - lam[:, 0]
    skew = 3.0 * (lam[:, 1] - iso) / span
    z_hi = skew <= 0
    zeta = torch.where(z_hi, lam[:, 2], lam[:, 0]) - iso
    eta = (lam[:, 1] - torch.where(z_hi, lam[:, 0], lam[:, 2])) / zeta
    return lam, axes, torch.stack([iso, span, skew, zeta, eta], dim=1)


def kernel_arm(t):
    p = rank2_invariants(t)
    return p.principal_values, p.principal_axes, torch.stack([p.iso, p.span, p.skew, p.zeta, p.eta], dim=1)


def bench(n: int, reps: int, warmup: int, budget: float) -> dict:
    g = torch.Generator(device=DEV).manual_seed(n)
    t = (torch.empty(n, dtype=torch.float64, device=DEV).uniform_(-500.0, 500.0, generator=g)[:, None, None]
         * torch.eye(3, dtype=torch.float64, device=DEV) + torch.randn(n, 3, 3, dtype=torch.float64, device=DEV, generator=g))
    c_vals = torch.randn(n, 3, dtype=torch.float64, device=DEV, generator=g)
    c_props = torch.randn(n, 5, dtype=torch.float64, device=DEV, generator=g)

    def forward(arm):
        with torch.no_grad():
            arm(t)

    def both(arm):
        x = t.detach().requires_grad_()
        vals, _, props = arm(x)
        ((vals * c_vals).sum() + (props * c_props).sum()).backward()

    cases = {"forward": forward, "forward+adjoint": both}
    arms = {"kernel": kernel_arm, "torch_eigh": torch_arm}
    out = {"atoms": n}
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
    ap.add_argument("--atoms", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--budget", type=float, default=30.0, help="seconds a (size, case) may take: caps the repetitions")
    a = ap.parse_args()
    from pbc_graph_bench import calibration

    print(json.dumps({"calibration": calibration()}), flush=True)
    for n in a.atoms:
        print(json.dumps(bench(n, a.reps, a.warmup, a.budget)), flush=True)


if __name__ == "__main__":
    main()
