#!/usr/bin/env python3
"""The eager ``Trainer`` against ``Trainer(graphed=True)``, whole epochs (training, validation, epoch-end hooks, history) in
one process with the arms alternating epoch by epoch: the n100 sample tiled to `--crystals` training crystals (2048) and
`--val-crystals` validation crystals (512), lmax-2 model, FlatAdam(lr 1e-2, weight_decay 1e-5, device_lr=True) in every arm

  arm A   ``Trainer()`` on the unpadded device loaders;
  arm B   ``Trainer(graphed=True)`` on the loaders padded to `--quanta` (64,2048), validation included (``pad_eval``);
  arm C   the kernel's own contribution: a replayed ``BucketedTrainStep`` with ``padded_mean_loss`` (C1) against one with
          ``valid_mean_loss`` (C2) on the padded training loader, no validation.

``Trainer.fit`` runs all its epochs in one call, so arms A and B run in a thread each and hand a baton over at every epoch
boundary (the loader wrappers below): one arm runs at a time, the device is synchronised at each boundary, and the time
an arm waits for the baton is not its own.  Every arm runs `--warmup` epochs first (arm B captures its buckets there),
then `--rounds` measured ones.  One JSON line per (batch size, arm): median and min-max ms per epoch, the training part per
training step and the validation part per validation step, and for arm B ``Trainer.step_counts``.

    python tools/trainer_bench.py [--batch 32 2048] [--quanta 64,2048] [--rounds 5] [--warmup 2]
"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import PAPER_HPARAMS  # noqa: E402
from matten_amd.data.graph import average_num_neighbors  # noqa: E402
from matten_amd.data.store import DeviceGraphStore  # noqa: E402
from matten_amd.dataset.structure_scalar_tensor import TensorDataModule, _DeviceLoader  # noqa: E402
from matten_amd.graphs import BucketedTrainStep, padded_mean_loss, valid_mean_loss  # noqa: E402
from matten_amd.model.trainer import Trainer  # noqa: E402
from matten_amd.model_factory.tfn_scalar_tensor import ScalarTensorModel  # noqa: E402
from matten_amd.optim import FlatAdam  # noqa: E402

DEV = "cuda:0"
TARGET = "elastic_tensor_full"
LMAX2 = dict(PAPER_HPARAMS, irreps_edge_sh="0e + 1o + 2e", conv_layer_irreps="32x0o+32x0e+16x1o+16x1e+4x2o+4x2e")
OPTIMIZER = {"class_path": "matten_amd.optim.FlatAdam", "init_args": {"lr": 1e-2, "weight_decay": 1e-5, "device_lr": True}}


def stats(ms, name="ms"):
    return {f"{name}_median": round(float(np.median(ms)), 4), f"{name}_min": round(float(min(ms)), 4),
            f"{name}_max": round(float(max(ms)), 4)}


class Baton:
    """one arm runs at a time, in the order of `names`, an epoch each"""

    def __init__(self, names):
        self.names, self.turn, self.cv = list(names), 0, threading.Condition()

    def wait_for(self, name):
        with self.cv:
            self.cv.wait_for(lambda: self.names[self.turn] == name)

    def pass_on(self, done=False):
        with self.cv:
            if done:
                self.names.pop(self.turn)
                self.turn = self.turn % len(self.names) if self.names else 0
            else:
                self.turn = (self.turn + 1) % len(self.names)
            self.cv.notify_all()


class Boundary:
    """a loader whose every pass starts with a call of `mark`"""

    def __init__(self, loader, mark):
        self.loader, self.mark = loader, mark

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        self.mark()
        yield from self.loader


class TrainerArm(threading.Thread):
    def __init__(self, name, baton, ds, train, val, epochs, **trainer_kw):
        super().__init__(name=name)
        self.baton, self.epochs, self.trainer_kw = baton, epochs, trainer_kw
        self.train, self.val = Boundary(train, self.epoch_start), Boundary(val, self.val_start)
        torch.manual_seed(3)
        self.model = ScalarTensorModel(backbone_hparams=dict(LMAX2), dataset_hparams=ds, optimizer_hparams=dict(OPTIMIZER)).to(DEV)
        self.t_start = self.t_val = None
        self.epoch_ms, self.train_ms, self.val_ms = [], [], []
        self.trainer, self.error = None, None

    def _close_epoch(self):
        torch.cuda.synchronize()
        now = time.perf_counter()
        if self.t_start is not None:
            self.epoch_ms.append(1e3 * (now - self.t_start))
            self.train_ms.append(1e3 * (self.t_val - self.t_start))
            self.val_ms.append(1e3 * (now - self.t_val))

    def epoch_start(self):
        self._close_epoch()
        if self.t_start is not None:
            self.baton.pass_on()
            self.baton.wait_for(self.name)
        torch.cuda.synchronize()
        self.t_start = time.perf_counter()

    def val_start(self):
        torch.cuda.synchronize()
        self.t_val = time.perf_counter()

    def run(self):
        self.baton.wait_for(self.name)
        try:
            torch.cuda.set_device(DEV)
            self.trainer = Trainer(max_epochs=self.epochs, **self.trainer_kw)
            self.trainer.fit(self.model, train_dataloaders=self.train, val_dataloaders=self.val)
            self._close_epoch()
        except BaseException as e:  # noqa: BLE001 - reported by the main thread
            self.error = e
        finally:
            self.baton.pass_on(done=True)


class StepArm:
    """padded_step_bench.py's arm B with the loss as the variable"""

    def __init__(self, name, store, ds, batch_size, pad, loss_fn, max_graphs):
        torch.manual_seed(3)
        self.name = name
        self.model = ScalarTensorModel(backbone_hparams=dict(LMAX2), dataset_hparams=ds).to(DEV).train()
        self.opt = FlatAdam(self.model.parameters(), lr=1e-2, weight_decay=1e-5, device_lr=True)
        self.loader = _DeviceLoader(store, training=True, batch_size=batch_size, shuffle=True, seed=3, pad=pad)
        self.step = BucketedTrainStep(self.model, self.opt, loss_fn, max_graphs=max_graphs, task_name=TARGET)
        self.ms = []

    def epoch(self, measured):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps = 0
        for batch in self.loader:
            self.step.step(batch, batch[TARGET])
            steps += 1
        torch.cuda.synchronize()
        if measured:
            self.ms.append(1e3 * (time.perf_counter() - t0) / steps)
        return steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[32, 2048])
    ap.add_argument("--crystals", type=int, default=2048)
    ap.add_argument("--val-crystals", type=int, default=512)
    ap.add_argument("--quanta", default="64,2048")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-graphs", type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("trainer_bench.py measures on an MI355X: no GPU here")

    name = "example_crystal_elasticity_tensor_n100.json"
    dm = TensorDataModule(name, name, name, root=os.path.join(ROOT, "tests", "golden"), r_cut=5.0, tensor_target_name=TARGET,
                          tensor_target_scale=1e-2)
    dm.setup()
    n100 = dm.train_data
    ds = {"allowed_species": sorted({int(z) for g in n100 for z in g["atomic_numbers"].tolist()}),
          "average_num_neighbors": average_num_neighbors(n100)}
    store = DeviceGraphStore.from_graphs([n100[i % len(n100)] for i in range(a.crystals)], DEV)
    val_store = DeviceGraphStore.from_graphs([n100[i % len(n100)] for i in range(a.val_crystals)], DEV)
    pad = tuple(int(v) for v in a.quanta.split(","))
    epochs = a.warmup + a.rounds

    for bs in a.batch:
        def loaders(p):
            kw = dict(batch_size=bs, seed=3, pad=p)
            return (_DeviceLoader(store, training=True, shuffle=True, **kw), _DeviceLoader(val_store, training=False, shuffle=False, **kw))

        baton = Baton(["A eager Trainer", f"B graphed Trainer {pad[0]},{pad[1]}"])
        arms = [TrainerArm(baton.names[0], baton, ds, *loaders(None), epochs),
                TrainerArm(baton.names[1], baton, ds, *loaders(pad), epochs, graphed=True, max_graphs=a.max_graphs)]
        for arm in arms:
            arm.start()
        for arm in arms:
            arm.join()
        for arm in arms:
            if arm.error is not None:
                raise arm.error
            n_train, n_val = len(arm.train), len(arm.val)
            out = dict(case="trainer_epoch", arm=arm.name, batch=bs, train_steps=n_train, val_steps=n_val, epochs=a.rounds,
                       **stats(arm.epoch_ms[a.warmup:], "epoch_ms"),
                       **stats([t / n_train for t in arm.train_ms[a.warmup:]], "train_ms_per_step"),
                       **stats([t / n_val for t in arm.val_ms[a.warmup:]], "val_ms_per_step"))
            if arm.trainer.step_counts:
                out["step_counts"] = arm.trainer.step_counts
            print(json.dumps(out), flush=True)
        del arms
        torch.cuda.empty_cache()

        steppers = [StepArm("C1 BucketedTrainStep padded_mean_loss", store, ds, bs, pad,
                            padded_mean_loss(lambda p, t: (p - t) ** 2, key=TARGET), a.max_graphs),
                    StepArm("C2 BucketedTrainStep valid_mean_loss", store, ds, bs, pad, valid_mean_loss("mse", key=TARGET),
                            a.max_graphs)]
        for arm in steppers:
            for _ in range(a.warmup):
                arm.epoch(False)
        for _ in range(a.rounds):
            for arm in steppers:
                steps = arm.epoch(True)
        for arm in steppers:
            print(json.dumps(dict(case="train_step", arm=arm.name, batch=bs, steps_per_epoch=steps, epochs=len(arm.ms),
                                  **stats(arm.ms), captures=arm.step.captures, replays=arm.step.replays,
                                  eager_steps=arm.step.eager_steps)), flush=True)
        del steppers
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
