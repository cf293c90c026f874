#!/usr/bin/env python3
"""Host loader against device-resident loader, in one process, arms alternating: the n100 sample tiled to `--crystals`
crystals (2048: the README's batch-2048 configuration, lmax-2 model), at every `--batch` size

  (a) assembly alone: wall time of one batch, synchronised, from `_Loader(device=...)` (collate on the host + its copies)
      and from `_DeviceLoader` (one table copy + matten_batch_gather); median and min-max over `--rounds` rounds of
      `--batches` batches per arm, after `--warmup` batches;
  (b) ms per eager training step (forward, MSE, backward, FlatAdam) of a `--steps`-step loop fed by each, synchronised
      once at the end of the loop; median and min-max over `--rounds` loops per arm.

One JSON line per (batch size, measurement).  The store's build time and device memory are reported once.

    python tools/loader_ab.py [--batch 32 2048] [--crystals 2048] [--rounds 7] [--batches 20] [--steps 20] [--warmup 5]
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
from __graft_entry__ import PAPER_HPARAMS  # noqa: E402
from matten_amd.data.graph import average_num_neighbors  # noqa: E402
from matten_amd.data.store import DeviceGraphStore  # noqa: E402
from matten_amd.dataset.structure_scalar_tensor import TensorDataModule, _DeviceLoader, _Loader  # noqa: E402
from matten_amd.model_factory.tfn_scalar_tensor import ScalarTensorModel  # noqa: E402
from matten_amd.optim import FlatAdam  # noqa: E402

DEV = "cuda:0"
TARGET = "elastic_tensor_full"
LMAX2 = dict(PAPER_HPARAMS, irreps_edge_sh="0e + 1o + 2e", conv_layer_irreps="32x0o+32x0e+16x1o+16x1e+4x2o+4x2e")


def forever(loader):
    while True:
        for batch in loader:
            yield batch


def stats(ms):
    return dict(ms_median=round(float(np.median(ms)), 4), ms_min=round(float(min(ms)), 4), ms_max=round(float(max(ms)), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[32, 2048])
    ap.add_argument("--crystals", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loader_ab.py measures on an MI355X: no GPU here")

    name = "example_crystal_elasticity_tensor_n100.json"
    dm = TensorDataModule(name, name, name, root=os.path.join(ROOT, "tests", "golden"), r_cut=5.0, tensor_target_name=TARGET,
                          tensor_target_scale=1e-2)
    dm.setup()
    n100 = dm.train_data
    graphs = [n100[i % len(n100)] for i in range(a.crystals)]
    ds = {"allowed_species": sorted({int(z) for g in n100 for z in g["atomic_numbers"].tolist()}),
          "average_num_neighbors": average_num_neighbors(n100)}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    store = DeviceGraphStore.from_graphs(graphs, DEV)
    torch.cuda.synchronize()
    print(json.dumps(dict(case="store", crystals=len(store), atoms=int(store.host.node_ptr[-1]), edges=int(store.host.edge_ptr[-1]),
                          build_ms=round(1e3 * (time.perf_counter() - t0), 1), device_mb=round(store.nbytes / 2 ** 20, 2),
                          bytes_per_crystal=round(store.nbytes / len(store)))), flush=True)

    for bs in a.batch:
        kw = dict(batch_size=bs, shuffle=True, seed=3)
        arms = {"host": forever(_Loader(graphs, device=DEV, **kw)), "device": forever(_DeviceLoader(store, training=True, **kw))}
        # (a) assembly alone
        times = {k: [] for k in arms}
        for k, it in arms.items():
            for _ in range(a.warmup):
                next(it)
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for k, it in arms.items():
                for _ in range(a.batches):
                    t0 = time.perf_counter()
                    batch = next(it)
                    torch.cuda.synchronize()
                    times[k].append(1e3 * (time.perf_counter() - t0))
        for k in arms:
            print(json.dumps(dict(case="assembly", loader=k, batch=bs, atoms=int(batch["pos"].shape[0]),
                                  edges=int(batch["edge_index"].shape[1]), samples=len(times[k]), **stats(times[k]))), flush=True)
        # (b) the training loop
        models = {}
        for k in arms:
            torch.manual_seed(3)
            m = ScalarTensorModel(backbone_hparams=dict(LMAX2), dataset_hparams=ds).to(DEV).train()
            models[k] = (m, FlatAdam(m.parameters(), lr=1e-2, weight_decay=1e-5))

        def loop(k, n):
            m, opt = models[k]
            for _ in range(n):
                batch = next(arms[k])
                loss = torch.nn.functional.mse_loss(m(dict(batch))[0][TARGET], batch[TARGET])
                opt.zero_grad()
                loss.backward()
                opt.step()
            return loss

        times = {k: [] for k in arms}
        for k in arms:
            loop(k, a.warmup)
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for k in arms:
                t0 = time.perf_counter()
                loop(k, a.steps)
                torch.cuda.synchronize()
                times[k].append(1e3 * (time.perf_counter() - t0) / a.steps)
        for k in arms:
            print(json.dumps(dict(case="train_step", loader=k, batch=bs, steps=a.steps, loops=len(times[k]),
                                  **stats(times[k]))), flush=True)


if __name__ == "__main__":
    main()
