#!/usr/bin/env python3
"""Device graph builder: (a) 1000 fcc-64 crystals (the benchmark's input; the default path, which pbc support must not
change), (b) the pair and the rows routes on one open fcc cluster / one periodic fcc crystal of 1000, 4000, 8000 atoms,
(c) both routes on a mixed batch: one large cluster with 200 fcc-64 crystals.
With --route: ONE case, `--generator` (fcc_cluster(n) or a periodic fcc_supercell of about n atoms) of `--atoms` atoms
built on the pair, rows or cells route -- one process per build, so that each can run under its own time limit; with
--calibration the machine's calibration record (the fixed kernels of bench.py's calibrate) is printed first.
Per case: median and min-max of `--reps` synchronised builds after `--warmup`, and the peak device memory of one build
above what it returns.  One JSON line per case.

    python tools/pbc_graph_bench.py [--reps 20] [--warmup 3] [--sizes 1000 4000 8000] [--skip-pair-above 8000]
    python tools/pbc_graph_bench.py --route cells --generator cluster --atoms 32000 [--calibration]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from matten_amd import predict as P  # noqa: E402
from matten_amd.data import synthetic  # noqa: E402
from matten_amd.data.graph import batch_graphs_gpu_soa  # noqa: E402

DEV = "cuda:0"


def measure(label, build, reps, warmup, **info):
    for _ in range(warmup):
        build()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = build()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    del out
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = build()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    returned = sum(t.numel() * t.element_size() for t in out.values())
    print(json.dumps(dict(case=label, ms_median=round(float(np.median(times)), 3), ms_min=round(min(times), 3),
                          ms_max=round(max(times), 3), reps=reps, edges=int(out["edge_index"].shape[1]),
                          scratch_mb=round((peak - returned) / 2 ** 20, 2), returned_mb=round(returned / 2 ** 20, 2), **info)),
          flush=True)


def periodic_fcc(n_atoms, a=4.05, seed=5):
    """a cubic fcc crystal of about n_atoms atoms (4 m^3), jittered"""
    m = max(1, round((n_atoms / 4.0) ** (1.0 / 3.0)))
    g = np.arange(m)
    corners = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 1, 3)
    basis = 0.5 * np.array([[0.0, 0, 0], [0, 1, 1], [1, 0, 1], [1, 1, 0]])
    pos = (corners + basis).reshape(-1, 3) * a + np.random.default_rng(seed).normal(0.0, 0.02, (4 * m ** 3, 3))
    return pos, m * a * np.eye(3)


ROUTE_ENV = {"pair": ("1000000000000", "1000000000000"), "rows": ("1", "1000000000000"), "cells": ("1", "1")}


def supercell_of(n_atoms):
    """the fcc_supercell whose atom count 4 m^3 is nearest to n_atoms"""
    m = max(1, round((n_atoms / 4.0) ** (1.0 / 3.0)))
    return synthetic.fcc_supercell(m, m, m)


def calibration(copy_floats=1 << 28, valu_iters=4096, reps=5):
    """what this machine sustains at this moment on the benchmark's fixed kernels (csrc/calib.hip, as bench.py calibrate):
    dependent fp32 FMA chains on every CU -> ns per wave64 VALU instruction and SIMD and the shader clock under that load;
    1 GiB read + 1 GiB written -> GB/s.  Median of `reps` launches timed with events."""
    from matten_amd import _lib, lab, ops

    lib, stream = lab.load(), ops._stream()
    src = torch.empty(copy_floats, dtype=torch.float32, device=DEV).normal_()
    dst = torch.empty_like(src)
    scratch = torch.zeros(4, dtype=torch.float32, device=DEV)
    clocks = torch.zeros(2, dtype=torch.int64, device=DEV)

    def timed(fn):
        fn()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for a, b in ev:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        return sorted(a.elapsed_time(b) for a, b in ev)[reps // 2]

    valu_ms = timed(lambda: _lib.check(lib.matten_calib_valu(valu_iters, scratch.data_ptr(), clocks.data_ptr(), stream),
                                       "matten_calib_valu"))
    ticks, ref100 = (int(v) for v in clocks.tolist())
    copy_ms = timed(lambda: _lib.check(lib.matten_calib_copy(src.data_ptr(), dst.data_ptr(), copy_floats, stream),
                                       "matten_calib_copy"))
    insts = int(lib.matten_calib_valu_insts_per_simd(valu_iters))
    return {"valu_ns_per_wave_inst_per_simd": round(1e6 * valu_ms / insts, 4),
            "sclk_mhz_under_valu_load": round(100.0 * ticks / ref100, 1) if ref100 else None,
            "copy_GBps": round(8 * copy_floats / (copy_ms * 1e-3) / 1e9, 1)}


def one_route(args):
    from matten_amd.data.graph import search_route

    if args.calibration:
        print(json.dumps({"calibration": calibration()}), flush=True)
    s = synthetic.fcc_cluster(args.atoms) if args.generator == "cluster" else supercell_of(args.atoms)
    p = s["cart_coords"]
    cl = s["lattice"][None] if "lattice" in s else np.zeros((1, 3, 3))
    pbc = np.array([s["pbc"]], dtype=bool)
    z, pt = s["atomic_numbers"], np.array([0, len(p)], dtype=np.int64)
    os.environ["MATTEN_NEIGHBOR_ROWS_MIN_ATOMS"], os.environ["MATTEN_NEIGHBOR_CELLS_MIN_ATOMS"] = ROUTE_ENV[args.route]
    assert search_route(len(p)) == args.route
    measure(f"{args.generator} {args.route}", lambda: batch_graphs_gpu_soa(p, cl, z, pt, args.r_cut, DEV, pbc=pbc), args.reps,
            args.warmup, atoms=len(p), r_cut=args.r_cut)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="*", default=[1000, 4000, 8000])
    ap.add_argument("--skip-pair-above", type=int, default=8000)
    ap.add_argument("--mixed", type=int, nargs="*", default=[1000, 2000, 4096],
                    help="sizes of the one large cluster batched with 200 fcc-64 crystals")
    ap.add_argument("--route", choices=sorted(ROUTE_ENV), help="one build on this route (see the module docstring)")
    ap.add_argument("--generator", choices=["cluster", "supercell"], default="cluster")
    ap.add_argument("--atoms", type=int, default=8000)
    ap.add_argument("--r-cut", type=float, default=5.0)
    ap.add_argument("--calibration", action="store_true")
    args = ap.parse_args()
    if args.route:
        return one_route(args)
    os.environ["MATTEN_NEIGHBOR_CELLS_MIN_ATOMS"] = "1000000000000"   # the cases below compare the pair and the rows routes

    pos, cell, Z, ptr, _, _ = P.pack_structures(synthetic.fcc64_structures(1000))
    measure("fcc64 x 1000, default path", lambda: batch_graphs_gpu_soa(pos, cell, Z, ptr, 5.0, DEV), args.reps, args.warmup)

    for n in args.sizes:
        c = synthetic.fcc_cluster(n)
        ppos, pcell = periodic_fcc(n)
        cases = (("open", c["cart_coords"], np.zeros((1, 3, 3)), np.zeros((1, 3), dtype=bool)),
                 ("periodic", ppos, pcell[None], None))
        for kind, p, cl, pbc in cases:
            z = np.full(len(p), 29, dtype=np.int64)
            pt = np.array([0, len(p)], dtype=np.int64)
            for route, env in (("pair", "1000000000"), ("rows", "1")):
                if route == "pair" and len(p) > args.skip_pair_above:
                    continue
                os.environ["MATTEN_NEIGHBOR_ROWS_MIN_ATOMS"] = env
                measure(f"{kind} {route}", lambda: batch_graphs_gpu_soa(p, cl, z, pt, 5.0, DEV, pbc=pbc), args.reps,
                        args.warmup, atoms=len(p))
    # a mixed batch: ONE structure of `big` atoms sends the whole batch down the rows route, where every small crystal
    # gets a wave per atom; on the pair route every crystal launches big^2 threads instead
    fcc = synthetic.fcc64_structures(200)
    for big in args.mixed:
        c = synthetic.fcc_cluster(big)
        structs = [dict(c, lattice=np.zeros((3, 3)))] + [dict(s, pbc=(True, True, True)) for s in fcc]
        mp, mc, mz, mptr, _, _, mflags = P.pack_structures(structs, with_pbc=True)
        for route, env in (("pair", "1000000000"), ("rows", "1")):
            os.environ["MATTEN_NEIGHBOR_ROWS_MIN_ATOMS"] = env
            measure(f"mixed {route}", lambda: batch_graphs_gpu_soa(mp, mc, mz, mptr, 5.0, DEV, pbc=mflags), args.reps,
                    args.warmup, atoms=int(mptr[-1]), largest=big, crystals=len(structs))
    os.environ.pop("MATTEN_NEIGHBOR_ROWS_MIN_ATOMS", None)
    os.environ.pop("MATTEN_NEIGHBOR_CELLS_MIN_ATOMS", None)


if __name__ == "__main__":
    main()
