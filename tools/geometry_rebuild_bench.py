#!/usr/bin/env python3
"""Loops over geometries of the same atoms: ms per geometry of "new positions and cell -> edge list -> forward" on three
routes, in one process with the routes alternating pass by pass

  route a   ``batch_graphs_gpu_soa`` (upload from numpy, one read-back of the edge count) + the eager forward;
  route b   the same build + ``GraphedForward``, one captured forward per batch shape (the edge count moves with the
            geometry, and a captured forward takes one shape: the shapes of all geometries are captured in the untimed
            warm-up pass, their number is printed);
  route c   ``GraphedGeometryStep`` on a ``GeometryBatch``: edge list and forward as one hipGraph replay, nothing read back;
            "c" takes the geometries from a device tensor (an optimiser or an integrator on the device), "c+upload" copies
            each from numpy first, as routes a and b do.

Cases: the 2-atom Si primitive cell, one fcc-64 crystal, the first 8 crystals of the n100 sample as one batch.  Every case
runs `--geometries` geometries whose positions and cells are scaled together by a seeded factor in [0.99, 1.01]; the model
is the paper's (random weights, eval).  A pass is timed with the host clock around the loop, closed by a device
synchronise, and with device events around the same loop; `--passes` passes per route, median and min-max in ms per
geometry.  The machine's calibration record comes first.  There is no pass/fail threshold: the numbers are for
INTEGRATION.md, "Rebuilding the edge list on the device".

    python tools/geometry_rebuild_bench.py [--geometries 200] [--passes 5]
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
from __graft_entry__ import PAPER_HPARAMS  # noqa: E402
from matten_amd.data import synthetic  # noqa: E402
from matten_amd.data.graph import batch_graphs_gpu_soa  # noqa: E402
from matten_amd.data.rebuild import GeometryBatch  # noqa: E402
from matten_amd.graphs import GraphedForward, GraphedGeometryStep  # noqa: E402
from matten_amd.model_factory.tfn_scalar_tensor import ScalarTensorModel  # noqa: E402

DEV = "cuda:0"
R_CUT = 5.0
TASK = "elastic_tensor_full"


def cases():
    """name -> (pos [N,3], cell [B,3,3], Z [N], ptr [B+1])"""
    from oracle.matten_ref.data import structures_from_json

    a = 5.43
    si = (np.array([[0.0, 0, 0], [a / 4, a / 4, a / 4]]), np.array([[[0, a / 2, a / 2], [a / 2, 0, a / 2], [a / 2, a / 2, 0]]]),
          np.array([14, 14]), np.array([0, 2]))
    f = synthetic.fcc64_structures(1)[0]
    fcc = (np.asarray(f["cart_coords"], dtype=np.float64), np.asarray(f["lattice"], dtype=np.float64)[None],
           np.asarray(f["atomic_numbers"]), np.array([0, len(f["atomic_numbers"])]))
    structs = structures_from_json(os.path.join(ROOT, "tests", "golden", "example_crystal_elasticity_tensor_n100.json"))[:8]
    sizes = [len(s["atomic_numbers"]) for s in structs]
    n100 = (np.concatenate([np.asarray(s["cart_coords"], dtype=np.float64) for s in structs]),
            np.stack([np.asarray(s["lattice"], dtype=np.float64) for s in structs]),
            np.concatenate([np.asarray(s["atomic_numbers"]) for s in structs]), np.concatenate([[0], np.cumsum(sizes)]))
    return {"si2": si, "fcc64": fcc, "n100_first8": n100}


def bench(name, case, model, n_geo: int, passes: int) -> dict:
    pos, cell, Z, ptr = case
    Z, ptr = Z.astype(np.int64), ptr.astype(np.int64)
    scales = 1.0 + 0.01 * np.random.default_rng(7).uniform(-1.0, 1.0, n_geo)
    host = [(np.ascontiguousarray(pos * s), np.ascontiguousarray(cell * s)) for s in scales]
    pos_d = torch.from_numpy(np.stack([p for p, _ in host])).to(DEV)
    cell_d = torch.from_numpy(np.stack([c for _, c in host])).to(DEV)
    gb = GeometryBatch(pos, cell, Z, ptr, R_CUT, DEV)
    step = GraphedGeometryStep(model, gb, task_name=TASK)
    graphs = {}

    def route_a(g):
        p, c = host[g]
        return model(batch_graphs_gpu_soa(p, c, Z, ptr, R_CUT, DEV), task_name=TASK)[0][TASK]

    def route_b(g):
        p, c = host[g]
        batch = batch_graphs_gpu_soa(p, c, Z, ptr, R_CUT, DEV)
        key = int(batch["edge_index"].shape[1])
        if key not in graphs:
            graphs[key] = GraphedForward(model, batch, task_name=TASK)
        return graphs[key](batch)

    def route_c(g):
        return step.step(pos=pos_d[g], cell=cell_d[g])

    def route_c_upload(g):
        p, c = host[g]
        return step.step(pos=torch.from_numpy(p).to(DEV, non_blocking=True), cell=torch.from_numpy(c).to(DEV, non_blocking=True))

    routes = {"a_build+eager": route_a, "b_build+graphed_forward": route_b, "c_replay": route_c, "c_replay+upload": route_c_upload}
    out = {"case": name, "atoms": int(ptr[-1]), "crystals": len(ptr) - 1, "edges_at_scale_1": gb.n_edges_at_construction,
           "edge_capacity": gb.e_b, "geometries": n_geo, "passes": passes}
    with torch.no_grad():
        ref = None
        for rname, run in routes.items():   # the untimed pass: every shape warmed, the routes compared on geometry 0
            for g in range(n_geo):
                r = run(g)
                if g == 0:
                    r = r[:len(ptr) - 1].clone()
                    ref = r if ref is None else ref
                    out[f"{rname}/max_abs_diff_to_a"] = float((r - ref).abs().max())
        torch.cuda.synchronize()
        gb.check()   # no geometry overflowed the capacity, lost a crystal's edges or had a singular cell
        out["b_distinct_shapes"] = len(graphs)
        wall = {r: [] for r in routes}
        dev = {r: [] for r in routes}
        for _ in range(passes):
            for rname, run in routes.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                a.record()
                for g in range(n_geo):
                    run(g)
                b.record()
                torch.cuda.synchronize()
                wall[rname].append((time.perf_counter() - t0) * 1e3 / n_geo)
                dev[rname].append(a.elapsed_time(b) / n_geo)
        gb.check()
    for rname in routes:
        for kind, t in (("wall", wall[rname]), ("events", dev[rname])):
            t = sorted(t)
            out[f"{rname}/{kind}_ms_per_geometry"] = {"median": round(t[len(t) // 2], 4), "min": round(t[0], 4), "max": round(t[-1], 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometries", type=int, default=200)
    ap.add_argument("--passes", type=int, default=5)
    a = ap.parse_args()
    from pbc_graph_bench import calibration

    print(json.dumps({"calibration": calibration()}), flush=True)
    all_cases = cases()
    species = sorted({int(z) for c in all_cases.values() for z in c[2]})
    torch.manual_seed(35)
    model = ScalarTensorModel(backbone_hparams=dict(PAPER_HPARAMS),
                              dataset_hparams={"allowed_species": species, "average_num_neighbors": 18.0}).to(DEV).eval()
    for name, case in all_cases.items():
        print(json.dumps(bench(name, case, model, a.geometries, a.passes)), flush=True)


if __name__ == "__main__":
    main()
