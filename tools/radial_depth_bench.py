#!/usr/bin/env python3
"""Cost of the radial network's depth (invariant_layers = L = 1..4): ms per eager and per hipGraph-replayed inference
forward of the paper model on 1000 fcc-64 crystals, and ms per training step (Adam) of the lmax-2 model at batch 2048
(the n100 sample tiled, as bench.py's batch-2048 step).  One JSON line per L.

    python tools/radial_depth_bench.py [--layers 1,2,3,4] [--iters 20]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from __graft_entry__ import PAPER_HPARAMS  # noqa: E402

DEV = "cuda:0"


def timed(fn, warmup: int, iters: int) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / iters * 1e3


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", default="1,2,3,4")
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()

    from common import LMAX2
    from matten_amd.data import synthetic
    from matten_amd.data.graph import average_num_neighbors, collate, crystal_graph
    from matten_amd.graphs import GraphedForward
    from matten_amd.model_factory.tfn_scalar_tensor import ScalarTensorModel
    from oracle.matten_ref.data import structures_from_json

    ds = {"allowed_species": list(synthetic.FCC_METALS), "average_num_neighbors": 18.0}
    fcc = synthetic.fcc64_graphs(64)
    batch = collate([fcc[i % 64] for i in range(1000)], device=DEV)
    structs = structures_from_json(os.path.join(ROOT, "tests", "golden", "example_crystal_elasticity_tensor_n100.json"))
    graphs = [crystal_graph(s["cart_coords"], s["lattice"], s["atomic_numbers"], 5.0) for s in structs]
    ds_t = {"allowed_species": sorted({int(z) for s in structs for z in s["atomic_numbers"]}),
            "average_num_neighbors": average_num_neighbors(graphs)}
    tb = collate([graphs[i % len(graphs)] for i in range(2048)], device=DEV)
    target = torch.randn(2048, 21, device=DEV)

    for L in (int(x) for x in args.layers.split(",")):
        torch.manual_seed(35)
        model = ScalarTensorModel(backbone_hparams=dict(PAPER_HPARAMS, invariant_layers=L), dataset_hparams=ds).to(DEV).eval()
        with torch.no_grad():
            t_eager = timed(lambda: model(dict(batch)), 3, args.iters)
            g = GraphedForward(model, batch)
            t_graph = timed(lambda: g(batch), 3, args.iters)
        del g, model
        torch.manual_seed(35)
        m = ScalarTensorModel(backbone_hparams=dict(LMAX2, invariant_layers=L), dataset_hparams=ds_t).to(DEV).train()
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)

        def step():
            loss = torch.nn.functional.mse_loss(m(dict(tb))[0]["elastic_tensor_full"], target)
            opt.zero_grad()
            loss.backward()
            opt.step()

        t_train = timed(step, 3, max(5, args.iters // 2))
        del m, opt
        torch.cuda.empty_cache()
        print(json.dumps({"invariant_layers": L, "fcc64_1000_forward_ms_eager": round(t_eager, 3),
                          "fcc64_1000_forward_ms_hipgraph": round(t_graph, 3),
                          "train_step_ms_batch2048_lmax2": round(t_train, 3), "edges_forward": int(batch["edge_index"].shape[1]),
                          "edges_train": int(tb["edge_index"].shape[1])}), flush=True)


if __name__ == "__main__":
    main()
