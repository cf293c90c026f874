"""
hipGraph capture of a whole optimisation step (forward, loss, backward, optimiser) for FIXED batch shapes.

At the reference's training batch size (32 crystals, ~150 atoms, ~4.5 k edges: pretrained/20230627/config_final.yaml:3-6)
a step is ~350 kernel launches for under 3 ms of kernel time: the host cannot issue them fast enough.  Captured once
(``torch.cuda.CUDAGraph`` = hipStreamBeginCapture / hipGraphLaunch on ROCm), a step is one launch.  The kernels of
``libmatten_hip.so`` take their stream as an argument and never synchronise, so they capture as they are.

Constraints (checked): every tensor of the batch keeps its shape and dtype between steps (``BucketedTrainStep`` below
keeps one captured step per shape of the padded device loader's batches), the optimiser is capturable (``torch.optim.Adam(..., capturable=True)``), and the one host synchronisation
of the forward -- the species / edge_index range check of ``SpeciesEmbedding`` -- is done once, eagerly, before the
capture and switched off inside it.  Replayed batches are therefore trusted by default (the kernels clamp bad ids:
memory-safe, but the result of a malformed batch is meaningless); pass ``validate=True`` to ``step`` / ``__call__`` to
read the flag word the captured forward rewrites on every replay (one host sync after the replay) and get the same
exception the eager path raises.  A batch that carries its own CSR (the device graph builder's `_amd_perm` / `_amd_rowptr` /
`_amd_src`) is trusted beyond that: the CSR is not re-derived from edge_index, so `validate=True` vouches for the species
ids only; every replayed batch must hold exactly the tensors of the construction batch (checked, ValueError).

Construction runs `warmup` real optimisation steps on the construction batch (allocator pools, lazily built tables,
optimiser state).  Model parameters, buffers (BatchNorm running statistics) and the optimiser state are snapshotted
before and restored IN PLACE afterwards, so the first ``step()`` starts from exactly the state the caller handed over.
"""
from typing import Callable, Dict

import torch

from .nn._tables import bump_weights_epoch, record_derived, refresh_derived


# rocPRIM's radix sort switches algorithm above 2^20 keys and that path does not survive a capture on this ROCm (memory
# aperture violation at replay; eager is fine -- most likely its hipMemsetAsync nodes: a memset captured by
# matten_csr_build was not re-executed on replay either, and is a kernel now).  Sparse graphs (E <= 64 N, every
# cutoff-radius graph of this domain) are built by counting without a device-wide sort and the species grouping never
# sorts, so only DENSE graphs above that size are refused.
MAX_CAPTURED_SORT_KEYS = 1_000_000


def _check_capturable(batch) -> None:
    from . import _lib

    n_edges = int(batch["edge_index"].shape[1])
    n_nodes = int(batch["pos"].shape[0])
    sorts = n_edges > _lib.load().matten_csr_counting_max_avg_degree() * n_nodes
    if sorts and n_edges > MAX_CAPTURED_SORT_KEYS:
        raise ValueError(f"{n_edges} edges on {n_nodes} nodes: a graph this dense is built with a radix sort, which "
                         f"cannot be captured above {MAX_CAPTURED_SORT_KEYS} edges on this ROCm; run it eagerly")


def _raise_for_flags(embeds, batch) -> None:
    n_nodes = int(batch["pos"].shape[0]) if "pos" in batch else None
    for m in embeds:
        if hasattr(m, "raise_for_last_flags"):
            m.raise_for_last_flags(n_nodes)


def _copy_batch(static: Dict, batch: Dict, what: str) -> None:
    """copy a replayed batch into the captured buffers.  The batch must hold EXACTLY the tensors the capture saw: a batch of
    the device graph builder carries its destination-sorted CSR (_amd_perm / _amd_rowptr / _amd_src), which the captured
    forward then reads instead of rebuilding it -- a replayed batch without those keys would silently run on the
    construction batch's CSR against its own edge_index (and one with extra keys has tensors the graph never reads)."""
    have = {k for k, v in batch.items() if isinstance(v, torch.Tensor)}
    want = {k for k, v in static.items() if isinstance(v, torch.Tensor)}
    if have != want:
        raise ValueError(f"the captured {what} was built on a batch with tensors {sorted(want)}; this batch "
                         f"{'lacks ' + str(sorted(want - have)) if want - have else ''}"
                         f"{' and ' if (want - have and have - want) else ''}"
                         f"{'adds ' + str(sorted(have - want)) if have - want else ''}: replay batches of the same builder "
                         f"(after editing edge_index, drop the _amd_* keys from the CONSTRUCTION batch too and capture again)")
    for k in want:
        s, v = static[k], batch[k]
        if s.shape != v.shape or s.dtype != v.dtype:
            raise ValueError(f"batch['{k}'] is {tuple(v.shape)} {v.dtype}, the captured {what} takes "
                             f"{tuple(s.shape)} {s.dtype}: capture one per batch shape")
        if s.data_ptr() != v.data_ptr():
            s.copy_(v, non_blocking=True)


def _apply_loss(loss_fn: Callable, preds, target, batch):
    """loss_fn(preds, target), or loss_fn(preds, target, batch) for a loss that reads the batch (padded_mean_loss:
    ``wants_batch``) -- inside a captured step `batch` holds the captured buffers, which every replay refreshes"""
    if getattr(loss_fn, "wants_batch", False):
        return loss_fn(preds, target, batch)
    return loss_fn(preds, target)


def padded_mean_loss(fn: Callable, key: str = None) -> Callable:
    """The mean of a per-element loss over the REAL crystals of a padded batch (``DeviceGraphStore.batch(pad_to=...)``).

    ``fn(prediction, target)`` returns the loss per element, [B_b, ...] (``lambda p, t: (p - t) ** 2`` for squared error);
    `key` picks the prediction out of the model's dict.  The returned ``loss(preds, target, batch)`` keeps the rows of
    the first ``batch["_amd_n_valid"][2]`` crystals (``torch.where`` on ``arange(B_b) < n_valid[2]``: whatever a padding row
    holds, NaN included, is replaced and gets a zero gradient) and divides their sum by the number of real elements.  The
    count stays on the device: no host read, so the loss captures, and a replay follows the refreshed count."""

    def loss(preds, target, batch):
        if "_amd_n_valid" not in batch:
            raise ValueError("padded_mean_loss needs a padded batch (DeviceGraphStore.batch(pad_to=...) or "
                             "_DeviceLoader(pad=...)): this batch has no '_amd_n_valid'")
        n_real = batch["_amd_n_valid"][2]
        per = fn(preds[key] if key is not None else preds, target)
        rows = per.shape[0]
        keep = (torch.arange(rows, device=per.device) < n_real).view((rows,) + (1,) * (per.dim() - 1))
        kept = torch.where(keep, per, torch.zeros((), dtype=per.dtype, device=per.device))
        return kept.sum() / (n_real * (per.numel() // max(rows, 1))).to(per.dtype)

    loss.wants_batch = True
    return loss


def valid_mean_loss(kind="mse", key: str = None) -> Callable:
    """The mean loss over the REAL crystals of a padded batch in one kernel: the counterpart of ``padded_mean_loss`` for
    squared and absolute error.

    `kind`: "mse" or "mae"; `key` picks the prediction out of the model's dict.  The returned
    ``loss(preds, target, batch)`` hands the crystal-count word ``batch["_amd_n_valid"][2:3]`` -- inside a captured step a
    view of the captured buffer, which every replay refreshes -- to ``autograd.ValidLossFn``: one kernel forward (two
    launches above one tile of elements), one backward, fp64 sums in a fixed order, nothing read back.  A padding row
    never enters the arithmetic, NaN included, and gets a +0.0 gradient."""
    from .autograd import ValidLossFn
    from .ops import LOSS_KINDS

    if kind not in LOSS_KINDS or isinstance(kind, bool):
        raise ValueError(f"kind = {kind!r}: 'mse' or 'mae'")
    code = LOSS_KINDS[kind]

    def loss(preds, target, batch):
        if "_amd_n_valid" not in batch:
            raise ValueError("valid_mean_loss needs a padded batch (DeviceGraphStore.batch(pad_to=...) or "
                             "_DeviceLoader(pad=...)): this batch has no '_amd_n_valid'")
        return ValidLossFn.apply(preds[key] if key is not None else preds, target, batch["_amd_n_valid"][2:3], code)[0]

    loss.wants_batch = True
    return loss


def selected_mean_loss(kind="mse", key: str = None, selector_key: str = "atom_selector") -> Callable:
    """The mean loss over the atoms that carry a target, for per-atom models on the dense label layout
    (``TensorDataModule(atom_selector=..., atom_target_layout="dense")``): the per-atom counterpart of ``padded_mean_loss``.

    `kind`: "mse" or "mae"; `key` picks the prediction out of the model's dict.  The returned
    ``loss(preds, target, batch)`` reads the int32 selector from ``batch[selector_key]`` -- inside a captured step that is
    the captured buffer, which every replay refreshes -- and runs ``autograd.SelectedLossFn``: one kernel forward, one
    backward, nothing read back.  The rows a padded batch appends are unselected by construction (their selector words
    are zero), so it needs no ``_amd_n_valid`` and serves plain and padded batches alike."""
    from .autograd import SelectedLossFn
    from .ops import LOSS_KINDS

    if kind not in LOSS_KINDS or isinstance(kind, bool):
        raise ValueError(f"kind = {kind!r}: 'mse' or 'mae'")
    code = LOSS_KINDS[kind]

    def loss(preds, target, batch):
        if selector_key not in batch:
            raise ValueError(f"selected_mean_loss needs batch['{selector_key}'] (the dense per-atom label layout)")
        selector = batch[selector_key]
        if selector.dtype == torch.bool or selector.is_floating_point():
            raise TypeError(f"batch['{selector_key}'] is {selector.dtype}: the dense route takes an integer selector (a bool "
                            f"selector belongs to the compact layout and preds[selector])")
        if selector.dtype != torch.int32:
            selector = selector.to(torch.int32)
        return SelectedLossFn.apply(preds[key] if key is not None else preds, target, selector, code)[0]

    loss.wants_batch = True
    return loss


def rank2_selected_loss(names=("iso",), kind: str = "mse", key: str = None, selector_key: str = "atom_selector",
                        formula: str = "ij=ji", weights=None) -> Callable:
    """The loss on derived scalars of per-atom tensors (``rank2.Rank2Loss``: isotropic value, span, skew, zeta, eta) over
    the atoms that carry a target, on the dense label layout: the counterpart of ``selected_mean_loss`` for fine-tuning a
    per-atom tensor model on, say, isotropic shieldings.

    The returned ``loss(preds, target, batch)`` takes the model's irreps rows [N,6] (``preds[key]``) through
    ``rank2.rank2_invariants_from_irreps`` and ``Rank2Loss``.  ``target`` is a dict name -> [N] / [N,1], or a tensor [N,k]
    (or [N] for one name) whose columns follow `names` -- an ordinary per-node key of the batch, which the device store
    gathers and pads like any other.  The selector comes from ``batch[selector_key]``; padding rows are unselected.
    Nothing is read back: ``GraphedTrainStep`` and ``BucketedTrainStep`` take it as it is."""
    from .rank2 import Rank2Loss, rank2_basis, rank2_invariants_from_irreps

    rank2_basis(formula)      # (a formula that is not a symmetric rank 2 fails here, not in the first step)
    loss_mod = Rank2Loss(names, weights, kind)
    names = loss_mod.names

    def loss(preds, target, batch):
        if selector_key not in batch:
            raise ValueError(f"rank2_selected_loss needs batch['{selector_key}'] (the dense per-atom label layout)")
        x = preds[key] if key is not None else preds
        if not isinstance(target, dict):
            if target.dim() == 1:
                target = target.unsqueeze(1)
            if target.dim() != 2 or target.shape[1] != len(names):
                raise ValueError(f"target: expected a dict or [N,{len(names)}] with one column for each of {names}, got "
                                 f"{tuple(target.shape)}")
            target = {n: target[:, q] for q, n in enumerate(names)}
        return loss_mod(rank2_invariants_from_irreps(x, formula), target, batch[selector_key])

    loss.wants_batch = True
    return loss


def stability_penalized(base_loss: Callable, weight: float, margin: float = 0.0, kind: str = "squared", key: str = None,
                        formula: str = "ijkl=jikl=klij", inverse: Callable = None) -> Callable:
    """``base_loss`` plus ``weight`` times the stability penalty of the predicted elasticity tensors
    (``elastic.StabilityPenalty(margin, kind)`` on their Kelvin moduli): fine-tuning towards mechanically stable
    predictions.

    ``base_loss`` is any loss the training steps take (``loss(preds, target)``, or ``loss(preds, target, batch)`` when it
    ``wants_batch``: ``valid_mean_loss("mse", key)``, say); `key` picks the irreps rows [B,21] out of the model's dict for
    the penalty.  ``inverse`` maps standardised predictions back to physical units before the penalty (a task normaliser's
    ``inverse``; default: the identity) -- a margin is in the units of the tensor, and definiteness is not preserved by a
    shift.  The returned ``loss(preds, target, batch)`` takes the rows through ``elastic.elastic_moduli_from_irreps(...,
    kelvin=True)``; on a padded batch the penalty is the mean over the real crystals (``batch["_amd_n_valid"][2:3]``, a
    device word), else over all rows.  Nothing is read back: ``GraphedTrainStep`` and ``BucketedTrainStep`` take it as it
    is."""
    from .elastic import StabilityPenalty, _check_floor, elastic_moduli_from_irreps, voigt_basis

    if not callable(base_loss):
        raise ValueError("base_loss: expected a callable loss")
    weight = _check_floor(weight, "weight")      # (the same check as floor and margin: numpy scalars are numbers too)
    if inverse is not None and not callable(inverse):
        raise ValueError("inverse: expected a callable (a task normaliser's inverse) or None")
    voigt_basis(formula)      # (a formula that is not a rank 4 fails here, not in the first step)
    penalty = StabilityPenalty(margin, kind)

    def loss(preds, target, batch):
        base = _apply_loss(base_loss, preds, target, batch)
        x = preds[key] if key is not None else preds
        if inverse is not None:
            x = inverse(x)
        props = elastic_moduli_from_irreps(x, formula, kelvin=True, kelvin_dilatation=False)      # (the moduli alone)
        n_valid = batch["_amd_n_valid"][2:3] if batch is not None and "_amd_n_valid" in batch else None
        return base + weight * penalty(props, n_valid).to(base.dtype)

    loss.wants_batch = True
    return loss


def _train_step(model, optimizer, loss_fn: Callable, batch, target, task_name: str):
    """one optimisation step as it is captured, and as it runs eagerly: forward, loss, backward, optimiser"""
    preds, _ = model(dict(batch), task_name=task_name)
    loss = _apply_loss(loss_fn, preds, target, batch)
    optimizer.zero_grad(set_to_none=True)
    loss.backward()
    optimizer.step()
    return loss


class GraphedTrainStep:
    def __init__(self, model, optimizer, loss_fn: Callable, batch: Dict[str, torch.Tensor], target: torch.Tensor,
                 warmup: int = 3, task_name: str = "elastic_tensor_full"):
        _check_capturable(batch)
        self.model, self.optimizer, self.loss_fn, self.task_name = model, optimizer, loss_fn, task_name
        self._static = {k: v.clone() if isinstance(v, torch.Tensor) else v for k, v in batch.items()}
        self._target = target.clone()
        self._capture(target.device, warmup)

    def _model_state(self) -> dict:
        """the model tensors the step mutates (snapshotted before the warm-up steps, restored in place after them)"""
        return self.model.state_dict()

    def _extra_state(self) -> list:
        """tensors the step mutates beyond model.state_dict() and the optimiser state (snapshotted and restored with them)"""
        return []

    def _capture(self, dev, warmup: int) -> None:
        """warm up `self._eager_step` on a side stream, put back in place what the warm-up steps changed, and capture one
        more call of it; its return value becomes ``self._loss``"""
        model, optimizer = self.model, self.optimizer
        embeds = [m for m in model.modules() if hasattr(m, "check_species")]
        self._embeds = embeds
        opt_state = optimizer.state if optimizer is not None else {}
        # the warm-up steps below are real optimiser steps: snapshot what they mutate
        with torch.no_grad():
            snap_model = {k: v.detach().clone() for k, v in self._model_state().items()}
            snap_opt = {p: {k: (v.detach().clone() if isinstance(v, torch.Tensor) else v) for k, v in st.items()}
                        for p, st in opt_state.items()}
            extra = self._extra_state()
            snap_extra = [v.detach().clone() for v in extra]
        # warm-up on a side stream (allocator pools, lazily built tables), with the range checks on
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(max(1, warmup)):
                self._eager_step()
            # restore in place: the capture below must see the tensors the warm-up allocated (optimiser moments, step)
            with torch.no_grad():
                for k, v in self._model_state().items():
                    v.copy_(snap_model[k])
                for v, old in zip(extra, snap_extra):
                    v.copy_(old)
                for p, st in opt_state.items():
                    old = snap_opt.get(p)
                    for k, v in st.items():
                        if isinstance(v, torch.Tensor):
                            if old is not None and isinstance(old.get(k), torch.Tensor):
                                v.copy_(old[k])
                            else:
                                v.zero_()   # a freshly initialised Adam state: step 0, zero moments
                        elif old is not None and k in old:
                            st[k] = old[k]
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        self._flags = [(m, m.check_species) for m in embeds]
        for m in embeds:
            m.check_species = False   # validated above; a host sync cannot be captured
        try:
            self.graph = torch.cuda.CUDAGraph()
            if optimizer is not None:
                optimizer.zero_grad(set_to_none=True)
            with torch.cuda.graph(self.graph):
                self._loss = self._eager_step()
        finally:
            for m, f in self._flags:
                m.check_species = f

    def _eager_step(self):
        return _train_step(self.model, self.optimizer, self.loss_fn, self._static, self._target, self.task_name)

    def step(self, batch: Dict[str, torch.Tensor], target: torch.Tensor, validate: bool = False) -> torch.Tensor:
        """copy the batch into the captured buffers (shapes must match) and replay; returns the captured loss tensor.
        validate=True: afterwards read the replayed forward's species / edge_index flags (a host sync) and raise like
        the eager path -- the parameters have already been updated with the malformed batch by then."""
        _copy_batch(self._static, batch, "step")
        if target.data_ptr() != self._target.data_ptr():
            self._target.copy_(target, non_blocking=True)
        if hasattr(self.optimizer, "sync_hyperparameters"):
            self.optimizer.sync_hyperparameters()   # a scheduler's new learning rate reaches the device before the replay
        self.graph.replay()
        bump_weights_epoch()   # the replayed optimiser step (and BatchNorm's running statistics) moved no _version counter
        if validate:
            _raise_for_flags(self._embeds, self._static)
        return self._loss


class BucketedTrainStep:
    """Training steps over batches of a FEW shapes, each shape captured once: the padded device loader
    (``_DeviceLoader(..., pad=(node_quantum, edge_quantum))``) rounds every batch up to a bucket (N_b, E_b, B_b), and
    ``step`` replays the ``GraphedTrainStep`` of the batch's bucket, capturing it on first sight.  Beyond `max_graphs`
    distinct buckets (a captured step keeps its own activations) the step runs eagerly.  The captured steps share the
    model and the optimiser, so their parameters, running statistics and optimiser state are one trajectory.

    ``captures`` / ``replays`` / ``eager_steps`` count what each call of ``step`` did (a capturing call replays its new
    graph once and counts as a capture)."""

    def __init__(self, model, optimizer, loss_fn: Callable, max_graphs: int = 8, warmup: int = 2,
                 task_name: str = "elastic_tensor_full"):
        self.model, self.optimizer, self.loss_fn, self.task_name = model, optimizer, loss_fn, task_name
        self.max_graphs, self.warmup = int(max_graphs), int(warmup)
        self.graphs: Dict[tuple, GraphedTrainStep] = {}
        self.captures = self.replays = self.eager_steps = 0

    @staticmethod
    def bucket(batch: Dict[str, torch.Tensor]) -> tuple:
        return (int(batch["pos"].shape[0]), int(batch["edge_index"].shape[1]), int(batch["ptr"].shape[0]) - 1)

    def step(self, batch: Dict[str, torch.Tensor], target: torch.Tensor, validate: bool = False) -> torch.Tensor:
        """one optimisation step on `batch`; returns the loss tensor (a captured step's is overwritten by its next replay).
        `validate` is GraphedTrainStep.step's and concerns replays only: an overflow step is an ordinary eager step, whose
        forward runs the range checks itself and raises before the parameters move."""
        key = self.bucket(batch)
        graphed = self.graphs.get(key)
        if graphed is None and len(self.graphs) >= self.max_graphs:
            self.eager_steps += 1
            if hasattr(self.optimizer, "sync_hyperparameters"):
                self.optimizer.sync_hyperparameters()   # (as before a replay)
            return _train_step(self.model, self.optimizer, self.loss_fn, batch, target, self.task_name)
        if graphed is None:
            # (refuses what cannot be captured; the warm-up steps are undone, so the replay below is this batch's one step)
            graphed = self.graphs[key] = GraphedTrainStep(self.model, self.optimizer, self.loss_fn, batch, target,
                                                          warmup=self.warmup, task_name=self.task_name)
            self.captures += 1
        else:
            self.replays += 1
        return graphed.step(batch, target, validate=validate)


MODEL_STEP_MODES = {"train": "training_step", "val": "validation_step", "test": "test_step"}


def _model_step(model, mode: str, optimizer, batch, batch_idx: int = 0):
    """the model's OWN step as it is captured, and as it runs eagerly: ``training_step`` (loss, logging, metric update),
    backward and the optimiser for "train"; ``validation_step`` / ``test_step`` without gradients for "val" / "test"""
    fn = getattr(model, MODEL_STEP_MODES[mode])
    if mode != "train":
        with torch.no_grad():
            return fn(batch, batch_idx)["loss"]
    loss = fn(batch, batch_idx)["loss"]
    optimizer.zero_grad(set_to_none=True)
    loss.backward()
    optimizer.step()
    return loss


def _check_model_step(model, mode: str, optimizer) -> None:
    if mode not in MODEL_STEP_MODES:
        raise ValueError(f"mode = {mode!r}: one of {sorted(MODEL_STEP_MODES)}")
    if (mode == "train") != (optimizer is not None):
        raise ValueError('mode "train" takes the optimizer its steps drive; "val" and "test" take none')
    if not hasattr(model, MODEL_STEP_MODES[mode]):
        raise TypeError(f"{type(model).__name__} has no {MODEL_STEP_MODES[mode]}: a model step captures the training shell "
                        f"of matten_amd.model.model.BaseModel")
    if bool(model.training) != (mode == "train"):
        raise ValueError(f'a "{mode}" step runs the model in {"training" if mode == "train" else "eval"} mode: call '
                         f'model.{"train" if mode == "train" else "eval"}() first (a captured step keeps the mode it saw)')


class GraphedModelStep(GraphedTrainStep):
    """``GraphedTrainStep`` around the model's own step in place of ``model(batch)`` plus a loss function: mode "train"
    captures ``model.training_step(batch, i)["loss"]``, ``zero_grad``, ``backward`` and ``optimizer.step()``; "val" and
    "test" capture ``model.validation_step`` / ``model.test_step`` under ``no_grad``.  The labels travel inside the batch.

    Two things such a step does beyond a forward and a loss are kept right across warm-up, capture and replay:

    * the metric accumulators (``model.metrics``: non-persistent buffers, so not in ``state_dict``) are snapshotted and put
      back in place with the parameters -- the warm-up steps leave no trace in the epoch's metric, and the replayed
      in-place adds land in the buffers ``compute()`` and ``reset()`` use;
    * ``model.log`` runs at capture time only.  The step keeps what it logged (``{mode}/total_loss``, ``{mode}/loss/<task>``:
      tensors of ITS graph) and re-installs it in ``model.logged`` after each replay: pointer swaps, no host read.

    A "val" / "test" step reads the weight-derived packs (packed radial layers, folded BatchNorm) that its warm-up left in
    the caches of ``nn._tables``; it records which, pins them (they refresh in place from then on) and re-derives the stale
    ones before each replay, so a replay follows the weights of the moment like an eager eval forward."""

    def __init__(self, model, mode: str, optimizer, batch: Dict[str, torch.Tensor], warmup: int = 3, batch_idx: int = 0):
        _check_model_step(model, mode, optimizer)
        _check_capturable(batch)
        self.model, self.mode, self.optimizer, self.batch_idx = model, mode, optimizer, int(batch_idx)
        self._static = {k: v.clone() if isinstance(v, torch.Tensor) else v for k, v in batch.items()}
        dev = self._static["pos"].device
        outer = getattr(model, "logged", None)
        keep = isinstance(outer, dict)
        if keep:
            model.logged = {}   # what warm-up and capture log stays with this step
        try:
            self._capture(dev, warmup)
        finally:
            self._logged = {}
            if keep:
                self._logged, model.logged = model.logged, outer
            if mode == "train":
                bump_weights_epoch()   # (a pack derived during the capture has not been computed yet)

    def _model_state(self) -> dict:
        # an eval-mode step under no_grad writes no parameter and no running statistic; putting them "back" would move
        # their version counters, and the capture would re-derive every pack inside the graph instead of reading it
        return self.model.state_dict() if self.mode == "train" else {}

    def _extra_state(self) -> list:
        metrics = getattr(self.model, "metrics", None)
        return list(metrics.buffers()) if isinstance(metrics, torch.nn.Module) else []

    def _eager_step(self):
        if self.mode != "train" and torch.cuda.is_current_stream_capturing():
            with record_derived() as self._derived:   # (all fresh after the warm-up: the capture reads them where they are)
                return _model_step(self.model, self.mode, self.optimizer, self._static, self.batch_idx)
        return _model_step(self.model, self.mode, self.optimizer, self._static, self.batch_idx)

    def step(self, batch: Dict[str, torch.Tensor], validate: bool = False) -> torch.Tensor:
        """copy the batch into the captured buffers (same tensors, shapes and dtypes) and replay; returns the captured loss
        tensor and points ``model.logged`` at this graph's logged tensors.  `validate`: GraphedTrainStep.step's."""
        _check_model_step(self.model, self.mode, self.optimizer)
        _copy_batch(self._static, batch, "step")
        if self.optimizer is not None and hasattr(self.optimizer, "sync_hyperparameters"):
            self.optimizer.sync_hyperparameters()   # a scheduler's new learning rate reaches the device before the replay
        if self.mode != "train":
            refresh_derived(self._derived)   # the packs the graph reads, re-derived in place where the weights have moved
        self.graph.replay()
        if self.mode == "train":
            bump_weights_epoch()   # the replayed optimiser step (and BatchNorm's running statistics) moved no _version counter
        if isinstance(getattr(self.model, "logged", None), dict):
            self.model.logged.update(self._logged)
        if validate:
            _raise_for_flags(self._embeds, self._static)
        return self._loss


class BucketedModelStep:
    """``BucketedTrainStep`` for the model's own step (``GraphedModelStep``): one captured step per bucket
    (N_b, E_b, B_b) of the padded device loader, eager ``training_step`` / ``validation_step`` / ``test_step`` beyond
    `max_graphs` distinct buckets, and the same ``captures`` / ``replays`` / ``eager_steps`` counters.  A batch without
    ``_amd_n_valid`` (an unpadded loader) is accepted: every shape is then its own bucket.

    What ``matten_amd.model.trainer.Trainer(graphed=True)`` drives, one per mode; a Lightning user calls ``step`` from a
    manual-optimisation ``training_step``."""

    def __init__(self, model, mode: str, optimizer=None, max_graphs: int = 8, warmup: int = 2):
        if mode not in MODEL_STEP_MODES:
            raise ValueError(f"mode = {mode!r}: one of {sorted(MODEL_STEP_MODES)}")
        if (mode == "train") != (optimizer is not None):
            raise ValueError('mode "train" takes the optimizer its steps drive; "val" and "test" take none')
        self.model, self.mode, self.optimizer = model, mode, optimizer
        self.max_graphs, self.warmup = int(max_graphs), int(warmup)
        self.graphs: Dict[tuple, GraphedModelStep] = {}
        self.captures = self.replays = self.eager_steps = 0

    bucket = staticmethod(BucketedTrainStep.bucket)

    @property
    def counts(self) -> Dict[str, int]:
        return {"captures": self.captures, "replays": self.replays, "eager_steps": self.eager_steps}

    def step(self, batch: Dict[str, torch.Tensor], batch_idx: int = 0, validate: bool = False) -> torch.Tensor:
        """one step of the mode on `batch`; returns the loss tensor (a captured step's is overwritten by its next replay)"""
        key = self.bucket(batch)
        graphed = self.graphs.get(key)
        if graphed is None and len(self.graphs) >= self.max_graphs:
            self.eager_steps += 1
            _check_model_step(self.model, self.mode, self.optimizer)
            if self.optimizer is not None and hasattr(self.optimizer, "sync_hyperparameters"):
                self.optimizer.sync_hyperparameters()   # (as before a replay)
            return _model_step(self.model, self.mode, self.optimizer, batch, batch_idx)
        if graphed is None:
            # (the warm-up steps are undone, metric accumulators included: the replay below is this batch's one step)
            graphed = self.graphs[key] = GraphedModelStep(self.model, self.mode, self.optimizer, batch, warmup=self.warmup,
                                                          batch_idx=batch_idx)
            self.captures += 1
        else:
            self.replays += 1
        return graphed.step(batch, validate=validate)


class GraphedForward:
    """Inference forward of FIXED batch shapes as one hipGraph launch: ``out = g(batch)`` -> [B, 21] (irreps) or the
    Cartesian tensors, whatever ``model(batch)`` returns for `task_name`.  Pays where the forward is launch-bound (small
    batches: ~45 launches); at 1000 crystals per batch the GPU is busy either way."""

    def __init__(self, model, batch: Dict[str, torch.Tensor], warmup: int = 3, task_name: str = "elastic_tensor_full"):
        _check_capturable(batch)
        self.model, self.task_name = model, task_name
        dev = next(model.parameters()).device
        self._static = {k: v.clone() if isinstance(v, torch.Tensor) else v for k, v in batch.items()}
        embeds = [m for m in model.modules() if hasattr(m, "check_species")]
        self._embeds = embeds
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(max(1, warmup)):
                model(dict(self._static), task_name=task_name)   # range checks on: validates the captured batch
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        flags = [(m, m.check_species) for m in embeds]
        for m in embeds:
            m.check_species = False
        try:
            self.graph = torch.cuda.CUDAGraph()
            with torch.no_grad(), torch.cuda.graph(self.graph):
                self._out = model(dict(self._static), task_name=task_name)[0][task_name]
        finally:
            for m, f in flags:
                m.check_species = f

    def __call__(self, batch: Dict[str, torch.Tensor], validate: bool = False) -> torch.Tensor:
        """NOTE: the species / edge_index range checks ran on the batch given at construction only; a replayed batch is
        trusted (same shapes enforced) unless validate=True (one host sync after the replay, same exceptions as eager)."""
        _copy_batch(self._static, batch, "forward")
        self.graph.replay()
        if validate:
            _raise_for_flags(self._embeds, self._static)
        return self._out


class GraphedGeometryStep:
    """"New positions / cells -> edge list -> forward (-> gradients)" of a ``data.rebuild.GeometryBatch`` as ONE hipGraph
    launch, for loops over geometries of the same atoms (strain sweeps, trajectory frames, structure optimisation).

    Captured, on one stream: the copy of the staged inputs into `gb`'s fp64 buffers, ``gb.update`` (prologue, counting
    pass, scan, capped fill: no host read), the forward on ``dict(gb.batch)`` -- the keys an earlier forward derived from
    the geometry (``geometry._DERIVED``) are never carried over -- and, with `fn`, ``fn(preds).backward()`` with the batch's
    ``pos`` / ``cell`` as leaves, as ``geometry.geometry_gradients`` runs it.

    ``step(pos, cell)`` returns the predictions of the REAL crystals (a view of the captured output, overwritten by the
    next step).  With `fn`, ``grads`` = {"pos" [N,3], "cell" [3B,3], "strain" [B,3,3]} holds the gradients of the scalar
    ``fn(preds)`` over the real rows (`fn` sees the padded predictions: restrict it to ``[:B]`` itself).  The flags of the
    replayed update are OR-ed into ``gb.flags`` (``gb.check()`` raises from them) or, with ``flags_out``, copied there.
    Warm-up and the species checks are those of ``GraphedForward``: validated once on the construction geometry, trusted
    on replay.  ``gb.grow`` replaces the tensors this step was captured on: build a new step afterwards."""

    def __init__(self, model, gb, fn: Callable = None, task_name: str = "elastic_tensor_full", warmup: int = 3):
        _check_capturable(gb.batch)
        self.model, self.gb, self.fn, self.task_name = model, gb, fn, task_name
        dev = gb.device
        self._tensors = dict(gb.batch)   # (identity: a grown batch is refused in step())
        self._pos_in, self._cell_in = gb.pos64.clone(), gb.cell64.clone()
        self._word = torch.zeros(1, dtype=torch.int32, device=dev)
        embeds = [m for m in model.modules() if hasattr(m, "check_species")]
        self._embeds = embeds
        params = [p for p in model.parameters() if p.requires_grad] if fn is not None else []
        kept = [p.grad for p in params]   # fn(preds).backward() reaches the parameters too: the caller's gradients stay
        flags = [(m, m.check_species) for m in embeds]
        try:
            side = torch.cuda.Stream(dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                for _ in range(max(1, warmup)):
                    for p in params:
                        p.grad = None
                    self._run()   # range checks on: validates the construction geometry
            torch.cuda.current_stream(dev).wait_stream(side)
            torch.cuda.synchronize(dev)
            for m in embeds:
                m.check_species = False
            for p in params:
                p.grad = None   # the capture allocates its own: a replay rewrites them instead of accumulating
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self._out, self.grads = self._run()
        finally:
            for p, g in zip(params, kept):
                p.grad = g      # the caller's gradients are left as they were
            for m, f in flags:
                m.check_species = f
        b, n = gb.n_crystals, gb.n_atoms
        self._real = self._out[:b] if self._out.shape[0] == gb.b_b else self._out[:n]   # per crystal / per atom
        gb.flags.bitwise_or_(self._word)   # (what warm-up and capture saw: the construction geometry, checked by gb)

    def _run(self):
        from .geometry import _DERIVED, strain_gradient

        gb = self.gb
        gb.update(pos=self._pos_in, cell=self._cell_in, flags_out=self._word)
        batch = {k: v for k, v in gb.batch.items() if k not in _DERIVED}
        if self.fn is None:
            with torch.no_grad():
                return self.model(batch, task_name=self.task_name)[0][self.task_name], None
        for key in ("pos", "cell"):
            batch[key] = batch[key].detach().clone().requires_grad_(True)
        with torch.enable_grad():
            preds, _ = self.model(batch, task_name=self.task_name)
            self.fn(preds).backward()
        n, b = gb.n_atoms, gb.n_crystals
        grads = {"pos": batch["pos"].grad[:n], "cell": batch["cell"].grad[:3 * b], "strain": strain_gradient(batch)[:b]}
        return preds[self.task_name].detach(), grads

    def step(self, pos=None, cell=None, flags_out=None) -> torch.Tensor:
        """``pos`` [N,3] / ``cell`` [B,3,3]: device tensors, fp64 (fp32 is widened: ``GeometryBatch.update``); None keeps the
        geometry of the step before.  No host sync."""
        gb = self.gb
        if any(gb.batch.get(k) is not v for k, v in self._tensors.items()):
            raise ValueError("the GeometryBatch was grown after this step was captured: build a new GraphedGeometryStep")
        if pos is not None:
            if tuple(pos.shape) != tuple(self._pos_in.shape):
                raise ValueError(f"pos is {tuple(pos.shape)}, the captured step takes {tuple(self._pos_in.shape)}")
            self._pos_in.copy_(pos, non_blocking=True)
        if cell is not None:
            if cell.numel() != self._cell_in.numel():
                raise ValueError(f"cell is {tuple(cell.shape)}, the captured step takes [{gb.n_crystals}, 3, 3]")
            self._cell_in.copy_(cell.reshape(self._cell_in.shape), non_blocking=True)
        self.graph.replay()
        if flags_out is None:
            gb.flags.bitwise_or_(self._word)
        else:
            flags_out.copy_(self._word.reshape(flags_out.shape))
        return self._real
