#!/usr/bin/env python3
"""Eager training steps against bucketed, captured ones, in one process, arms alternating: the n100 sample tiled to
`--crystals` crystals (2048), lmax-2 model, at every `--batch` size, one full shuffled epoch per arm and round

  arm A          eager steps (forward, MSE, backward, FlatAdam) fed by `_DeviceLoader`;
  arm B(qn,qe)   `matten_amd.graphs.BucketedTrainStep` fed by `_DeviceLoader(pad=(qn, qe))`, the loss
                 `padded_mean_loss` of the squared error, one arm per entry of `--quanta`.

Every arm runs `--warmup` epochs first (arm B captures its buckets there; a bucket first seen later is captured inside
a measured epoch, or runs eagerly beyond `--max-graphs`), then `--rounds` measured epochs, synchronised once at the end
of each.  One JSON line per (batch size, arm): median and min-max ms per step, the distinct buckets seen, the counters of
the bucketed step and the padding overhead (padded atoms and edges over real ones, over all measured epochs).

    python tools/padded_step_bench.py [--batch 32 2048] [--quanta 64,2048 128,4096 256,8192] [--rounds 5] [--warmup 2]
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
from matten_amd.dataset.structure_scalar_tensor import TensorDataModule, _DeviceLoader  # noqa: E402
from matten_amd.graphs import BucketedTrainStep, padded_mean_loss  # noqa: E402
from matten_amd.model_factory.tfn_scalar_tensor import ScalarTensorModel  # noqa: E402
from matten_amd.optim import FlatAdam  # noqa: E402

DEV = "cuda:0"
TARGET = "elastic_tensor_full"
LMAX2 = dict(PAPER_HPARAMS, irreps_edge_sh="0e + 1o + 2e", conv_layer_irreps="32x0o+32x0e+16x1o+16x1e+4x2o+4x2e")


def stats(ms):
    return dict(ms_median=round(float(np.median(ms)), 4), ms_min=round(float(min(ms)), 4), ms_max=round(float(max(ms)), 4))


class Arm:
    def __init__(self, name, store, ds, batch_size, pad, max_graphs):
        torch.manual_seed(3)
        self.name, self.pad = name, pad
        self.model = ScalarTensorModel(backbone_hparams=dict(LMAX2), dataset_hparams=ds).to(DEV).train()
        self.opt = FlatAdam(self.model.parameters(), lr=1e-2, weight_decay=1e-5, device_lr=pad is not None)
        self.loader = _DeviceLoader(store, training=True, batch_size=batch_size, shuffle=True, seed=3, pad=pad)
        self.step = None
        if pad is not None:
            self.step = BucketedTrainStep(self.model, self.opt, padded_mean_loss(lambda p, t: (p - t) ** 2, key=TARGET),
                                          max_graphs=max_graphs, task_name=TARGET)
        self.buckets, self.atoms, self.edges, self.ms = set(), 0, 0, []

    def epoch(self, measured):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps = 0
        for batch in self.loader:
            if self.step is not None:
                self.step.step(batch, batch[TARGET])
            else:
                loss = torch.nn.functional.mse_loss(self.model(dict(batch))[0][TARGET], batch[TARGET])
                self.opt.zero_grad()
                loss.backward()
                self.opt.step()
            steps += 1
            if measured:
                self.buckets.add(BucketedTrainStep.bucket(batch))
                self.atoms += int(batch["pos"].shape[0])
                self.edges += int(batch["edge_index"].shape[1])
        torch.cuda.synchronize()
        if measured:
            self.ms.append(1e3 * (time.perf_counter() - t0) / steps)
        return steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[32, 2048])
    ap.add_argument("--crystals", type=int, default=2048)
    ap.add_argument("--quanta", nargs="+", default=["64,2048", "128,4096", "256,8192"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-graphs", type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("padded_step_bench.py measures on an MI355X: no GPU here")

    name = "example_crystal_elasticity_tensor_n100.json"
    dm = TensorDataModule(name, name, name, root=os.path.join(ROOT, "tests", "golden"), r_cut=5.0, tensor_target_name=TARGET,
                          tensor_target_scale=1e-2)
    dm.setup()
    n100 = dm.train_data
    graphs = [n100[i % len(n100)] for i in range(a.crystals)]
    ds = {"allowed_species": sorted({int(z) for g in n100 for z in g["atomic_numbers"].tolist()}),
          "average_num_neighbors": average_num_neighbors(n100)}
    store = DeviceGraphStore.from_graphs(graphs, DEV)
    real_atoms, real_edges = int(store.host.node_ptr[-1]), int(store.host.edge_ptr[-1])
    quanta = [tuple(int(v) for v in q.split(",")) for q in a.quanta]

    for bs in a.batch:
        arms = [Arm("A eager", store, ds, bs, None, a.max_graphs)]
        arms += [Arm(f"B bucketed {q[0]},{q[1]}", store, ds, bs, q, a.max_graphs) for q in quanta]
        for arm in arms:
            for _ in range(a.warmup):
                arm.epoch(False)
        warm = {arm.name: (arm.step.captures if arm.step else 0) for arm in arms}
        for _ in range(a.rounds):
            for arm in arms:
                steps = arm.epoch(True)
        for arm in arms:
            out = dict(case="train_step", arm=arm.name, batch=bs, steps_per_epoch=steps, epochs=len(arm.ms), **stats(arm.ms),
                       buckets=len(arm.buckets), atoms_over_real=round(arm.atoms / (a.rounds * real_atoms), 4),
                       edges_over_real=round(arm.edges / (a.rounds * real_edges), 4))
            if arm.step is not None:
                out.update(captures_in_warmup=warm[arm.name], captures=arm.step.captures, replays=arm.step.replays,
                           eager_steps=arm.step.eager_steps)
            print(json.dumps(out), flush=True)
        del arms
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
