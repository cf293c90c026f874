"""
A minimal stand-in for ``pytorch_lightning.Trainer`` with the call sequence of ``Trainer.fit`` / ``Trainer.test`` that
the reference's training script relies on (scripts/train_materials_tensor.py:52-66): configure_optimizers, then per
epoch training_step / backward / step over the train loader, validation_step over the val loader, the epoch-end hooks,
and a ReduceLROnPlateau-style scheduler stepped on the monitored score.  For the boxes without Lightning and for tests;
with Lightning installed use its Trainer (the model is a LightningModule then).

``Trainer(graphed=True)`` runs the same loop with every training, validation and test step replayed from a hipGraph
(``matten_amd.graphs.BucketedModelStep``: one captured step per batch shape, eager beyond `max_graphs` shapes).  It is
meant for the padded device loaders (``TensorDataModule(device_resident=True, loader_kwargs={"pad": ...}, pad_eval=True)``:
a few shapes per epoch) and sets ``model.loss_over_valid_rows`` for the run, so that the padding crystals stay out of loss
and metric.  Nothing is read back per step: the logged values are read once per epoch, where ``history`` is built.
"""
from typing import Dict, Optional

import torch


def _as_floats(logged: dict) -> dict:
    return {k: (float(v) if hasattr(v, "item") else v) for k, v in logged.items()}


class Trainer:
    def __init__(self, max_epochs: int = 1, limit_train_batches: Optional[int] = None, accelerator: str = "gpu",
                 devices: int = 1, gradient_clip_val: Optional[float] = None, graphed: bool = False, max_graphs: int = 8,
                 graph_warmup: int = 2, **ignored):
        self.max_epochs, self.limit_train_batches = max_epochs, limit_train_batches
        self.gradient_clip_val = gradient_clip_val   # Lightning's name: the global 2-norm the gradients are clipped to
        self.graphed, self.max_graphs, self.graph_warmup = bool(graphed), int(max_graphs), int(graph_warmup)
        self.history, self.optimizers = [], []
        # graphed=True: per mode, what its steps did ({"captures", "replays", "eager_steps"})
        self.step_counts: Dict[str, Dict[str, int]] = {}

    def _check_graphed(self, optimizer, scheduler) -> None:
        """what a captured training step cannot do, refused before the first step with the remedy"""
        from ..optim import FlatAdam

        flat = isinstance(optimizer, FlatAdam)
        remedy = ('optimizer_hparams = {"class_path": "matten_amd.optim.FlatAdam", "init_args": {"device_lr": True, ...}} '
                  '(or torch.optim.Adam(..., capturable=True) without a scheduler and without gradient_clip_val)')
        if not flat and not any(g.get("capturable", False) for g in optimizer.param_groups):
            raise ValueError(f"Trainer(graphed=True): {type(optimizer).__name__} cannot be captured into a hipGraph (its step "
                             f"reads the device or keeps its state on the host); use {remedy}")
        if scheduler is not None and not (flat and optimizer.device_control):
            raise ValueError(f"Trainer(graphed=True) with a learning-rate scheduler: a captured step replays the learning rate "
                             f"it was captured with unless the rate lives on the device; use FlatAdam(device_lr=True): {remedy}")
        if self.gradient_clip_val is not None and not flat:
            raise ValueError(f"Trainer(graphed=True, gradient_clip_val=...): torch.nn.utils.clip_grad_norm_ between backward "
                             f"and step is not part of a captured step; FlatAdam clips inside its own step on the device: "
                             f"{remedy}")

    def _stepper(self, model, mode: str, optimizer=None):
        from ..graphs import BucketedModelStep

        return BucketedModelStep(model, mode, optimizer, max_graphs=self.max_graphs, warmup=self.graph_warmup)

    def fit(self, model, datamodule=None, train_dataloaders=None, val_dataloaders=None):
        train = train_dataloaders if train_dataloaders is not None else datamodule.train_dataloader()
        val = val_dataloaders if val_dataloaders is not None else (datamodule.val_dataloader() if datamodule else None)
        cfg = model.configure_optimizers()
        optimizer = cfg["optimizer"] if isinstance(cfg, dict) else cfg
        scheduler = cfg.get("lr_scheduler") if isinstance(cfg, dict) else None
        self.optimizers = [optimizer]   # Lightning's name
        if self.graphed:
            self._check_graphed(optimizer, scheduler)
        clip_params = None
        if self.gradient_clip_val is not None:
            from ..optim import FlatAdam

            if isinstance(optimizer, FlatAdam):
                optimizer.set_max_grad_norm(self.gradient_clip_val)   # clipped inside its own step, on the device
            else:
                clip_params = [p for g in optimizer.param_groups for p in g["params"]]
        if not self.graphed:
            return self._fit_loop(model, train, val, optimizer, scheduler, clip_params, None, None)
        before = model.loss_over_valid_rows
        model.loss_over_valid_rows = True
        train_step, val_step = self._stepper(model, "train", optimizer), self._stepper(model, "val")
        try:
            return self._fit_loop(model, train, val, optimizer, scheduler, None, train_step, val_step)
        finally:
            model.loss_over_valid_rows = before
            self.step_counts["train"] = train_step.counts
            if val is not None:
                self.step_counts["val"] = val_step.counts

    def _fit_loop(self, model, train, val, optimizer, scheduler, clip_params, train_step, val_step):
        for epoch in range(self.max_epochs):
            model.train()
            for i, batch in enumerate(train):
                if self.limit_train_batches is not None and i >= self.limit_train_batches:
                    break
                if train_step is not None:
                    train_step.step(batch, i)   # training_step, backward and optimizer.step() as one replay
                    continue
                loss = model.training_step(batch, i)["loss"]
                optimizer.zero_grad(set_to_none=True)
                loss.backward()
                if clip_params is not None:
                    torch.nn.utils.clip_grad_norm_(clip_params, self.gradient_clip_val)
                optimizer.step()
            model.on_training_epoch_end()
            if val is not None:
                model.eval()
                with torch.no_grad():
                    for i, batch in enumerate(val):
                        if val_step is not None:
                            val_step.step(batch, i)
                        else:
                            model.validation_step(batch, i)
                model.on_validation_epoch_end()
            score = model.logged.get(model.monitor_key) if hasattr(model, "logged") else None
            if scheduler is not None:
                if isinstance(scheduler, torch.optim.lr_scheduler.ReduceLROnPlateau):
                    if score is not None:
                        scheduler.step(score)
                else:
                    scheduler.step()
            self.history.append({"epoch": epoch, **_as_floats(getattr(model, "logged", {}))})
        return self

    def test(self, model=None, datamodule=None, dataloaders=None, ckpt_path=None):
        loader = dataloaders if dataloaders is not None else datamodule.test_dataloader()
        model.eval()
        if self.graphed:
            before = model.loss_over_valid_rows
            model.loss_over_valid_rows = True
            test_step = self._stepper(model, "test")
            try:
                for i, batch in enumerate(loader):
                    test_step.step(batch, i)
                model.on_test_epoch_end()
            finally:
                model.loss_over_valid_rows = before
                self.step_counts["test"] = test_step.counts
        else:
            with torch.no_grad():
                for i, batch in enumerate(loader):
                    model.test_step(batch, i)
            model.on_test_epoch_end()
        return [_as_floats({k: v for k, v in getattr(model, "logged", {}).items() if k.startswith(("test/", "metric_test/"))})]
