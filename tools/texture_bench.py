#!/usr/bin/env python3
"""Textured-polycrystal means (csrc/texture.hip): what a texture costs on the device, in one process

  operator   ``ops.texture_operator`` on one texture of G seeded orientations, for every G of `--orientations`: the G
             orientations reduced to the 21 x 21 operator (two launches);
  average    ``ops.texture_average`` (all four means) and its adjoint ``ops.texture_average_bwd`` on B crystals under one
             texture, for every B of `--rows`: they work from the operator, so G does not enter;
  irreps     the same Voigt mean through ``symmetry.average_irreps`` (fp64 rows; one Wigner-D product per row and
             orientation) at G = `--irreps-orientations`;
  numpy      ``texture_average_host`` (the 36 x 36 formulation) on `--host-rows` crystals, on the CPU.

Inputs are fp64 symmetric positive definite Voigt matrices (A A^T + 1).  Every device arm runs `--warmup` times, then
`--reps` times between device events; medians and min-max in ms.  The machine's calibration record comes first.  There is no
pass/fail threshold: the numbers are for INTEGRATION.md and docs/LAB_NOTES.md, "Textured polycrystals".

    python tools/texture_bench.py [--orientations 1000 10000 100000] [--rows 1000 100000] [--reps 20] [--warmup 3]
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
from matten_amd import elastic, ops, symmetry  # noqa: E402
from matten_amd import texture as tx  # noqa: E402

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


def rotations(n: int, seed: int) -> np.ndarray:
    return tx.Texture.scatter(np.eye(3), 25.0, n, seed).rotations


def crystals(n: int, seed: int) -> np.ndarray:
    A = np.random.default_rng(seed).standard_normal((n, 6, 6))
    return A @ A.transpose(0, 2, 1) + np.eye(6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--orientations", type=int, nargs="+", default=[1000, 10_000, 100_000])
    ap.add_argument("--rows", type=int, nargs="+", default=[1000, 100_000])
    ap.add_argument("--irreps-orientations", type=int, default=1000)
    ap.add_argument("--host-rows", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from pbc_graph_bench import calibration

    print(json.dumps({"calibration": calibration()}), flush=True)
    for G in a.orientations:
        R = torch.tensor(rotations(G, G), device=DEV)
        ptr = torch.tensor([0, G], dtype=torch.int64, device=DEV)
        print(json.dumps({"operator": {"orientations": G, **timed(lambda: ops.texture_operator(R, None, ptr), a.reps, a.warmup)}}),
              flush=True)
    tex = tx.Texture(rotations(a.irreps_orientations, 1))
    op, tex_flags = tex.operator(DEV)
    for B in a.rows:
        C = crystals(B, B)
        props = elastic.elastic_properties(C)
        voigt, flags = props.voigt, props.flags
        moduli, vectors, _ = ops.elastic_kelvin(voigt, flags, want_dilatation=False)
        agg_ptr, mc, mt, mf, crystal_ptr, crystal_member = tx._device_members(B, 1, None, DEV)
        out, status = ops.texture_average(voigt, flags, moduli, vectors, op, tex_flags, mc, mt, mf, agg_ptr)
        assert int((status != 0).sum()) == 0
        g = torch.ones_like(out)
        rec = {"rows": B, "orientations_behind_the_operator": a.irreps_orientations}
        rec["texture_average"] = timed(lambda: ops.texture_average(voigt, flags, moduli, vectors, op, tex_flags, mc, mt, mf, agg_ptr),
                                       a.reps, a.warmup)
        rec["texture_average_bwd"] = timed(lambda: ops.texture_average_bwd(moduli, vectors, op, tex_flags, mc, mt, mf, agg_ptr, out,
                                                                           status, g, crystal_ptr, crystal_member), a.reps, a.warmup)
        rec["kelvin"] = timed(lambda: ops.elastic_kelvin(voigt, flags, want_dilatation=False), a.reps, a.warmup)
        x = torch.tensor(_np(voigt).reshape(B, 36) @ np.linalg.pinv(elastic.voigt_basis()), device=DEV)
        Rd = torch.tensor(tex.rotations, device=DEV)
        rec["average_irreps_voigt_mean_only"] = timed(lambda: symmetry.average_irreps(x, "ijkl=jikl=klij", Rd), max(3, a.reps // 4), 1)
        print(json.dumps({"average": rec}), flush=True)
    C = crystals(a.host_rows, 7)
    t0 = time.perf_counter()
    tx.texture_average_host(C, tex, method="kronecker")
    print(json.dumps({"numpy": {"rows": a.host_rows, "orientations": a.irreps_orientations,
                                "texture_average_host_ms": round(1e3 * (time.perf_counter() - t0), 1)}}), flush=True)


def _np(t):
    return t.detach().cpu().numpy()


if __name__ == "__main__":
    main()
