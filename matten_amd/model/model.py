"""
Optimisation-loop shell of the models: the part of the reference's ``BaseModel`` (model/model.py:53-480) that the
training script drives -- ``compute_loss``, ``shared_step``, ``training_step`` / ``validation_step`` / ``test_step``,
metric bookkeeping and ``configure_optimizers`` -- on top of whatever ``forward`` / ``decode`` / ``preprocess_batch`` the
concrete model defines (model_factory/tfn_*.py).

With PyTorch Lightning installed the base class IS ``pytorch_lightning.LightningModule`` and a stock ``Trainer`` runs
the model (scripts/train_materials_tensor.py:34-68 of the reference works with ``import matten``).  Without it -- the
build and GPU boxes have no Lightning -- the base is ``torch.nn.Module`` with the three hooks the shell calls
(``save_hyperparameters``, ``log``, ``log_dict``) and ``matten_amd.model.trainer.Trainer`` is a minimal loop with the same
call sequence.  Nothing here is on the hot path: every tensor operation of a step happens in ``decode``.
"""
import importlib
import time
from typing import Any, Dict, Tuple, Union

import torch
from torch import Tensor

try:  # pragma: no cover - not installed on the build / GPU boxes
    import pytorch_lightning as _pl

    _Base = _pl.LightningModule
    HAVE_LIGHTNING = True
except Exception:  # noqa: BLE001
    _Base = torch.nn.Module
    HAVE_LIGHTNING = False

from ..model_factory.task import TaskType


def instantiate_class(args, init: Dict[str, Any]):
    """``{"class_path": "torch.optim.Adam", "init_args": {...}}`` -> object (lightning.cli.instantiate_class,
    used by the reference at model/model.py:449,478)"""
    args = args if isinstance(args, tuple) else (args,)
    module, _, name = init["class_path"].rpartition(".")
    cls = getattr(importlib.import_module(module), name)
    return cls(*args, **(init.get("init_args") or {}))


class TimeMeter:
    """reference utils.py TimeMeter: (seconds since the last update, seconds since the start)"""

    def __init__(self):
        self.t0 = self.t = time.time()

    def update(self):
        now = time.time()
        delta, self.t = now - self.t, now
        return delta, now - self.t0


_SELECTED_LOSS_KINDS = {torch.nn.MSELoss: 0, torch.nn.L1Loss: 1}   # matten_selected_loss's `kind`


def _is_dense_selector(selector) -> bool:
    """the selector's dtype picks the route: ``bool`` is the reference's compact layout (``preds[selector]``), an integer
    dtype the dense one (one target row per atom)"""
    return isinstance(selector, Tensor) and selector.dtype != torch.bool and not selector.is_floating_point()


def _batchnorms(model):
    from ..nn.utils import _IrrepBatchNorm

    return [m for m in model.modules() if isinstance(m, _IrrepBatchNorm)]


def freeze_batchnorm(model, freeze_affine: bool = False):
    """Fine-tuning with frozen statistics: every BatchNorm of `model` goes to eval mode -- it normalises with its running
    averages, which no step writes any more, and gradients flow through it to the layers below and to its own weight /
    bias -- and STAYS there: the modules are flagged, and their ``train()`` ignores later ``model.train()`` calls (what a
    trainer issues at the start of every epoch) until ``unfreeze_batchnorm``.  freeze_affine=True also takes weight and
    bias out of the optimisation (requires_grad = False).  No parameter, buffer or state_dict key changes.  Returns the
    model."""
    for bn in _batchnorms(model):
        bn.__dict__["_frozen_stats"] = True
        bn.eval()
        if freeze_affine:
            if "_frozen_affine" not in bn.__dict__:
                bn.__dict__["_frozen_affine"] = (bn.weight.requires_grad, bn.bias.requires_grad)
            bn.weight.requires_grad_(False)
            bn.bias.requires_grad_(False)
    return model


def unfreeze_batchnorm(model):
    """Undo ``freeze_batchnorm``: the BatchNorms follow the model's mode again and a frozen affine gets its earlier
    requires_grad flags back."""
    for bn in _batchnorms(model):
        if bn.__dict__.pop("_frozen_stats", False):
            bn.train(model.training)
        flags = bn.__dict__.pop("_frozen_affine", None)
        if flags is not None:
            bn.weight.requires_grad_(flags[0])
            bn.bias.requires_grad_(flags[1])
    return model


class BaseModel(_Base):
    monitor_key = "val/score"
    # True: on a batch that carries `_amd_n_valid` (a padded batch of the device loader) loss and metric run over the real
    # crystals only (compute_valid_loss).  Off by default; Trainer(graphed=True) switches it on for the run.
    loss_over_valid_rows = False

    # ---- what a subclass's __init__ calls once backbone and tasks exist (reference model/model.py:66-99) ----
    def _init_training_shell(self, hparams: Dict[str, Any]) -> None:
        if HAVE_LIGHTNING:  # pragma: no cover
            self.save_hyperparameters(hparams)
        else:
            self.hparams = dict(hparams)
        tasks = {k: t for k, t in self.tasks.items() if t is not None}
        self.loss_fns = {name: task.init_loss() for name, task in tasks.items()}
        self.metrics = torch.nn.ModuleDict()
        for mode in ("train", "val", "test"):
            self.metrics["metric_" + mode] = torch.nn.ModuleDict(
                {name: task.init_metric_as_collection() for name, task in tasks.items()})
        self.timer = TimeMeter()
        self.logged: Dict[str, Any] = {}

    if not HAVE_LIGHTNING:
        def log(self, name, value, **kwargs):
            self.logged[name] = value.detach() if isinstance(value, Tensor) else value

        def log_dict(self, d, **kwargs):
            for k, v in d.items():
                self.log(k, v)

        @property
        def device(self):
            # (the first Parameter OBJECT is stable across .to() / FlatAdam re-homing; walking parameters() costs ~8 us and
            # preprocess_batch asks once per forward)
            p = self.__dict__.get("_amd_first_param")
            if p is None:
                p = next(self.parameters())
                self.__dict__["_amd_first_param"] = p
            return p.device

    # ---- reference model/model.py:234-280 ----
    def compute_loss(self, preds: Dict[str, Tensor], labels: Dict[str, Tensor], weight: Tensor = None):
        individual_losses, total_loss = {}, 0.0
        for task_name, task in self.tasks.items():
            p = task.transform_pred_loss(preds[task_name])
            l = task.transform_target_loss(labels[task_name])
            if weight is not None:
                p, l = p * weight, l * weight
            if task.task_type == TaskType.CLASSIFICATION and task.is_binary():
                p, l = p.reshape(-1), l.reshape(-1).to(torch.get_default_dtype())
            loss = self.loss_fns[task_name](p, l)
            individual_losses[task_name] = loss
            total_loss = total_loss + task.loss_weight * loss
        return individual_losses, total_loss

    def compute_selected_loss(self, preds: Dict[str, Tensor], labels: Dict[str, Tensor], weight: Tensor = None):
        """``compute_loss`` over the atoms an integer ``labels["atom_selector"]`` flags (the dense per-atom layout): the
        task's loss class picks the kernel's kind and the mean runs over the selected rows on the device
        (autograd.SelectedLossFn), where the reference indexes ``preds[selector]`` first (model/model.py:340-345)."""
        from ..autograd import SelectedLossFn

        if weight is not None:
            raise NotImplementedError("target_weight with dense per-atom labels (an integer atom_selector) is not supported")
        selector = labels["atom_selector"]
        if selector.dtype != torch.int32:
            selector = selector.to(torch.int32)
        individual_losses, total_loss = {}, 0.0
        for task_name, task in self.tasks.items():
            fn = self.loss_fns[task_name]
            kind = _SELECTED_LOSS_KINDS.get(type(fn))
            if kind is None or getattr(fn, "reduction", "mean") != "mean":
                raise NotImplementedError(f"dense per-atom labels: the selected-loss kernel computes the mean of MSELoss or "
                                          f"L1Loss, task '{task_name}' uses {fn!r}")
            p = task.transform_pred_loss(preds[task_name])
            l = task.transform_target_loss(labels[task_name])
            if l.shape[0] != p.shape[0]:
                raise ValueError(f"dense per-atom labels: '{task_name}' holds {l.shape[0]} target rows for {p.shape[0]} "
                                 f"predicted atoms (one row per atom, zeros where the selector is 0)")
            loss = SelectedLossFn.apply(p, l, selector, kind)[0]
            individual_losses[task_name] = loss
            total_loss = total_loss + task.loss_weight * loss
        return individual_losses, total_loss

    def compute_valid_loss(self, preds: Dict[str, Tensor], labels: Dict[str, Tensor], n_valid: Tensor, weight: Tensor = None):
        """``compute_loss`` over the real crystals of a padded batch: the rows [0, *n_valid), `n_valid` being the crystal
        word of ``batch["_amd_n_valid"]`` on the device (autograd.ValidLossFn; the twin of ``compute_selected_loss``).  The
        padding crystals' targets are zero and their predictions are not: the model's plain mean would average them in.
        Returns a third value beside the two of ``compute_loss``: per task, the tensors the kernel saw and its (sums,
        count), which ``update_metrics`` reuses where the metric transforms hand it the same tensors."""
        from ..autograd import ValidLossFn

        if weight is not None:
            raise NotImplementedError("target_weight with loss_over_valid_rows (the valid-rows loss of a padded batch) is "
                                      "not supported")
        individual_losses, total_loss, seen = {}, 0.0, {}
        for task_name, task in self.tasks.items():
            fn = self.loss_fns[task_name]
            kind = _SELECTED_LOSS_KINDS.get(type(fn))
            if task.task_type == TaskType.CLASSIFICATION or kind is None or getattr(fn, "reduction", "mean") != "mean":
                raise NotImplementedError(f"loss_over_valid_rows: the valid-loss kernel computes the mean of MSELoss or "
                                          f"L1Loss of a regression task, task '{task_name}' uses {fn!r}")
            p = task.transform_pred_loss(preds[task_name])
            l = task.transform_target_loss(labels[task_name])
            if l.shape[0] != p.shape[0]:
                raise ValueError(f"loss_over_valid_rows: '{task_name}' holds {l.shape[0]} target rows for {p.shape[0]} "
                                 f"predicted crystals (a padded batch keeps one row per crystal, padding included)")
            loss, sums, count = ValidLossFn.apply(p, l, n_valid, kind)
            seen[task_name] = (p, l, sums, count)
            individual_losses[task_name] = loss
            total_loss = total_loss + task.loss_weight * loss
        return individual_losses, total_loss, seen

    # ---- reference model/model.py:282-312 ----
    def training_step(self, batch, batch_idx):
        loss, preds, labels = self.shared_step(batch, "train")
        self.update_metrics(preds, labels, "train")
        return {"loss": loss}

    def on_training_epoch_end(self):
        self.compute_metrics("train")

    def validation_step(self, batch, batch_idx):
        loss, preds, labels = self.shared_step(batch, "val")
        self.update_metrics(preds, labels, "val")
        return {"loss": loss}

    def on_validation_epoch_end(self):
        _, score = self.compute_metrics("val")
        if score is not None:  # val/score: early stopping, checkpointing and the lr scheduler watch it
            self.log(self.monitor_key, score, on_step=False, on_epoch=True, prog_bar=True)
        delta_t, cumulative_t = self.timer.update()
        self.log("epoch time", delta_t, on_step=False, on_epoch=True, prog_bar=True)
        self.log("cumulative time", cumulative_t, on_step=False, on_epoch=True, prog_bar=True)

    def test_step(self, batch, batch_idx):
        loss, preds, labels = self.shared_step(batch, "test")
        self.update_metrics(preds, labels, "test")
        return {"loss": loss}

    def on_test_epoch_end(self):
        self.compute_metrics("test")

    # ---- reference model/model.py:316-372 ----
    def shared_step(self, batch, mode: str):
        batch_size = batch.num_graphs if hasattr(batch, "num_graphs") else int(batch["ptr"].shape[0]) - 1
        graphs, labels = self.preprocess_batch(batch)
        preds = self.decode(graphs)
        target_weight = graphs.get("target_weight", None)
        if _is_dense_selector(labels.get("atom_selector")):
            # dense per-atom labels (one target row per atom, integer selector): no indexing, no host read
            individual_loss, total_loss = self.compute_selected_loss(preds, labels, weight=target_weight)
        elif self.loss_over_valid_rows and "_amd_n_valid" in graphs and "atom_selector" not in labels:
            # a padded crystal batch: loss (and, through the labels, the metric) over the real crystals only
            n_valid = graphs["_amd_n_valid"][2:3]
            individual_loss, total_loss, seen = self.compute_valid_loss(preds, labels, n_valid, weight=target_weight)
            labels = dict(labels, _amd_n_valid=n_valid, _amd_valid_sums=seen)
        else:
            if "atom_selector" in labels:
                selector = labels["atom_selector"]
                preds = {k: v[selector] for k, v in preds.items()}
            individual_loss, total_loss = self.compute_loss(preds, labels, weight=target_weight)
        self.log_dict({f"{mode}/loss/{name}": loss for name, loss in individual_loss.items()},
                      on_step=False, on_epoch=True, prog_bar=False, batch_size=batch_size)
        self.log(f"{mode}/total_loss", total_loss, on_step=False, on_epoch=True, prog_bar=True, batch_size=batch_size)
        return total_loss, preds, labels

    # ---- reference model/model.py:374-445 ----
    def update_metrics(self, preds: Dict, labels: Dict, mode: str):
        selector = labels.get("atom_selector")
        if _is_dense_selector(selector):   # dense per-atom labels: the metric masks on the device
            for task_name, metric in self.metrics["metric_" + mode].items():
                task = self.tasks[task_name]
                if task.task_type == TaskType.CLASSIFICATION:
                    raise NotImplementedError("dense per-atom labels serve regression tasks")
                p = task.transform_pred_metric(preds[task_name])
                l = task.transform_target_metric(labels[task_name])
                metric(p.detach(), l.detach(), selector=selector)
            return
        n_valid = labels.get("_amd_n_valid")
        if n_valid is not None:   # a padded crystal batch under loss_over_valid_rows: the metric skips the padding rows
            seen = labels.get("_amd_valid_sums", {})
            for task_name, metric in self.metrics["metric_" + mode].items():
                task = self.tasks[task_name]
                if task.task_type == TaskType.CLASSIFICATION:
                    raise NotImplementedError("loss_over_valid_rows serves regression tasks")
                p = task.transform_pred_metric(preds[task_name])
                l = task.transform_target_metric(labels[task_name])
                p_loss, l_loss, sums, count = seen.get(task_name, (None,) * 4)
                if p is p_loss and l is l_loss:   # identity transforms (no normaliser): the loss's kernel call serves both
                    metric(p.detach(), l.detach(), n_valid=n_valid, valid_sums=(sums, count))
                else:
                    metric(p.detach(), l.detach(), n_valid=n_valid)
            return
        for task_name, metric in self.metrics["metric_" + mode].items():
            task = self.tasks[task_name]
            p = task.transform_pred_metric(preds[task_name])
            l = task.transform_target_metric(labels[task_name])
            if task.task_type == TaskType.CLASSIFICATION:
                p = torch.sigmoid(p.reshape(-1)) if task.is_binary() else torch.argmax(p, dim=1)
            metric(p.detach(), l.detach())

    def compute_metrics(self, mode, log: bool = True) -> Tuple[Dict[str, Dict[str, Tensor]], Union[Tensor, None]]:
        mode = "metric_" + mode
        total_score, individual_score = None, {}
        for task_name, metric_coll in self.metrics[mode].items():
            score = metric_coll.compute()
            individual_score[task_name] = score
            if log:
                for metric_name, metric_value in score.items():
                    self.log(f"{mode}/{metric_name}/{task_name}", metric_value, on_step=False, on_epoch=True, prog_bar=False)
            agg = self.tasks[task_name].metric_aggregation()
            if agg:
                total_score = 0 if total_score is None else total_score
                for metric_name, weight in agg.items():
                    total_score = total_score + score[metric_name] * weight
            metric_coll.reset()
        return individual_score, total_score

    # ---- reference model/model.py:447-479 ----
    def configure_optimizers(self):
        # optimizer_hparams["freeze_batchnorm"] (absent: nothing changes): True / "statistics" fine-tunes with frozen
        # running statistics, "affine" also freezes the BatchNorm weight / bias (model.freeze_batchnorm)
        frozen = (self.optimizer_hparams or {}).get("freeze_batchnorm")
        if frozen:
            if frozen not in (True, "statistics", "affine"):
                raise ValueError(f'optimizer_hparams["freeze_batchnorm"] must be True, "statistics" or "affine", got {frozen!r}')
            freeze_batchnorm(self, freeze_affine=frozen == "affine")
        params = (filter(lambda p: p.requires_grad, self.parameters()),)
        optimizer = instantiate_class(params, self.optimizer_hparams)
        scheduler = self._config_lr_scheduler(optimizer)
        if scheduler is None:
            return optimizer
        return {"optimizer": optimizer, "lr_scheduler": scheduler, "monitor": self.monitor_key}

    def _config_lr_scheduler(self, optimizer):
        hp = self.lr_scheduler_hparams or {}
        class_path = hp.get("class_path")
        if class_path is None or class_path == "none":
            return None
        init = dict(hp, init_args={k: v for k, v in (hp.get("init_args") or {}).items()
                                   if not (k == "verbose" and "ReduceLROnPlateau" in class_path)})  # removed in torch 2.7
        return instantiate_class(optimizer, init)
