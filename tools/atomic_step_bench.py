#!/usr/bin/env python3
"""Per-atom tensor training steps, three routes in one process, arms alternating: the n100 sample tiled to `--crystals`
crystals with a synthetic selector (atoms of even atomic number; the first atom where there is none) and random ij=ji
targets, the atomic model of the reference's configs/atomic_tensor.yaml, at every `--batch` size, one full shuffled
epoch per arm and round

  arm A   eager, compact labels: ``mse_loss(preds[bool selector], target)`` fed by the host loader (the reference's route);
  arm B   eager, dense labels: ``selected_mean_loss`` fed by `_DeviceLoader`;
  arm C   `matten_amd.graphs.BucketedTrainStep` with ``selected_mean_loss`` fed by `_DeviceLoader(pad=...)`.

Every arm runs `--warmup` epochs first (arm C captures its buckets there), then `--rounds` measured epochs, synchronised
once at the end of each.  The machine's calibration record comes first, then one JSON line per (batch size, arm) with
median and min-max ms per step, then the loss kernels alone (forward + adjoint on the rows of one batch): per pair, timed
with events around `--loss-reps` eager pairs and around one replay of a graph that captured as many.

    python tools/atomic_step_bench.py [--batch 2 32] [--crystals 512] [--rounds 5] [--warmup 2]
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
from matten_amd.data.graph import average_num_neighbors  # noqa: E402
from matten_amd.data.store import DeviceGraphStore  # noqa: E402
from matten_amd.dataset.structure_scalar_tensor import TensorDataModule, _DeviceLoader, _Loader  # noqa: E402
from matten_amd.graphs import BucketedTrainStep, selected_mean_loss  # noqa: E402
from matten_amd.model_factory.tfn_atomic_tensor import AtomicTensorModel  # noqa: E402
from matten_amd.optim import FlatAdam  # noqa: E402

DEV = "cuda:0"
TARGET = "nmr_tensor"
# reference scripts/configs/atomic_tensor.yaml:20-72
ATOMIC = {
    "species_embedding_dim": 16, "irreps_edge_sh": "0e + 1o + 2e", "num_radial_basis": 8, "radial_basis_start": 0.0,
    "radial_basis_end": 5.0, "radial_basis_type": "bessel", "num_layers": 3, "invariant_layers": 2, "invariant_neurons": 32,
    "average_num_neighbors": "auto", "conv_layer_irreps": "32x0o+32x0e + 16x1o+16x1e + 4x2o+4x2e",
    "nonlinearity_type": "gate", "normalization": "batch", "resnet": True, "output_format": "irreps",
    "output_formula": "ij=ji", "reduce": "mean",
}
QUANTA = {2: (16, 1024), 32: (64, 2048)}


def stats(ms):
    return dict(ms_median=round(float(np.median(ms)), 4), ms_min=round(float(min(ms)), 4), ms_max=round(float(max(ms)), 4))


def labelled(graphs, layout, seed=11):
    """the graphs with per-atom labels in `layout`: the same selector and the same target rows in both"""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for g in graphs:
        g = {k: v for k, v in g.items() if k != "elastic_tensor_full"}
        sel = g["atomic_numbers"] % 2 == 0
        if not sel.any():
            sel[0] = True
        rows = torch.randn(int(sel.sum()), 6, generator=gen)
        if layout == "compact":
            g[TARGET], g["atom_selector"] = rows, sel
        else:
            g[TARGET] = torch.zeros(sel.shape[0], 6)
            g[TARGET][sel] = rows
            g["atom_selector"] = sel.to(torch.int32)
        out.append(g)
    return out


class Arm:
    def __init__(self, name, loader, ds, bucketed):
        torch.manual_seed(3)
        self.name, self.loader = name, loader
        self.model = AtomicTensorModel(tasks=TARGET, backbone_hparams=dict(ATOMIC), dataset_hparams=ds).to(DEV).train()
        self.opt = FlatAdam(self.model.parameters(), lr=1e-2, weight_decay=1e-5, device_lr=bucketed)
        self.dense_loss = selected_mean_loss("mse", key=TARGET)
        self.step = BucketedTrainStep(self.model, self.opt, self.dense_loss, max_graphs=32, task_name=TARGET) if bucketed else None
        self.ms = []

    def loss(self, preds, batch):
        if batch["atom_selector"].dtype == torch.bool:
            return torch.nn.functional.mse_loss(preds[TARGET][batch["atom_selector"]], batch[TARGET])
        return self.dense_loss(preds, batch[TARGET], batch)

    def epoch(self, measured):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps = 0
        for batch in self.loader:
            if self.step is not None:
                self.step.step(batch, batch[TARGET])
            else:
                loss = self.loss(self.model(dict(batch), task_name=TARGET)[0], batch)
                self.opt.zero_grad()
                loss.backward()
                self.opt.step()
            steps += 1
        torch.cuda.synchronize()
        if measured:
            self.ms.append(1e3 * (time.perf_counter() - t0) / steps)
        return steps


def loss_alone(n_rows, reps):
    """forward + adjoint of the selected loss on [n_rows, 6]: ms per pair, eager (launch gaps included) and replayed"""
    from matten_amd.autograd import SelectedLossFn

    gen = torch.Generator().manual_seed(5)
    pred = torch.randn(n_rows, 6, generator=gen).to(DEV).requires_grad_(True)
    target = torch.randn(n_rows, 6, generator=gen).to(DEV)
    sel = (torch.rand(n_rows, generator=gen) < 0.5).to(torch.int32).to(DEV)

    def pairs():
        for _ in range(reps):
            torch.autograd.grad(SelectedLossFn.apply(pred, target, sel, 0)[0], pred)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        pairs()
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pairs()
    graph.replay()
    eager = sorted(timed(pairs) for _ in range(5))[2]
    replayed = sorted(timed(graph.replay) for _ in range(5))[2]
    return dict(case="selected_loss_fwd_bwd", n_rows=n_rows, d=6, pairs=reps, ms_per_pair_eager=round(eager, 5),
                ms_per_pair_replayed=round(replayed, 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[2, 32])
    ap.add_argument("--crystals", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loss-reps", type=int, default=100)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("atomic_step_bench.py measures on an MI355X: no GPU here")
    from pbc_graph_bench import calibration

    print(json.dumps({"calibration": calibration()}), flush=True)
    name = "example_crystal_elasticity_tensor_n100.json"
    dm = TensorDataModule(name, name, name, root=os.path.join(ROOT, "tests", "golden"), r_cut=5.0,
                          tensor_target_name="elastic_tensor_full")
    dm.setup()
    n100 = dm.train_data
    ds = {"allowed_species": sorted({int(z) for g in n100 for z in g["atomic_numbers"].tolist()}),
          "average_num_neighbors": average_num_neighbors(n100)}
    compact, dense = (labelled([n100[i % len(n100)] for i in range(a.crystals)], layout) for layout in ("compact", "dense"))
    store = DeviceGraphStore.from_graphs(dense, DEV)
    atoms_per_crystal = float(store.host.node_ptr[-1]) / a.crystals

    for bs in a.batch:
        kw = dict(batch_size=bs, shuffle=True, seed=3)
        pad = QUANTA.get(bs, (64, 2048))
        arms = [Arm("A eager compact (bool indexing)", _Loader(compact, device=DEV, **kw), ds, False),
                Arm("B eager dense", _DeviceLoader(store, training=True, **kw), ds, False),
                Arm(f"C bucketed dense {pad[0]},{pad[1]}", _DeviceLoader(store, training=True, pad=pad, **kw), ds, True)]
        for arm in arms:
            for _ in range(a.warmup):
                arm.epoch(False)
        for _ in range(a.rounds):
            for arm in arms:
                steps = arm.epoch(True)
        for arm in arms:
            out = dict(case="atomic_train_step", arm=arm.name, batch=bs, steps_per_epoch=steps, epochs=len(arm.ms), **stats(arm.ms))
            if arm.step is not None:
                out.update(captures=arm.step.captures, replays=arm.step.replays, eager_steps=arm.step.eager_steps)
            print(json.dumps(out), flush=True)
        del arms
        torch.cuda.empty_cache()
        print(json.dumps(loss_alone(max(1, round(bs * atoms_per_crystal)), a.loss_reps)), flush=True)


if __name__ == "__main__":
    main()
