"""
Adam over one flat parameter buffer, the optimiser of the reference's training recipe
(torch.optim.Adam, lr 1e-2, weight_decay 1e-5: scripts/configs/materials_tensor.yaml:103-107;
pretrained/20230627/config_final.yaml:43-47).

``FlatAdam(model.parameters(), ...)`` re-homes every parameter as a view into ONE contiguous fp32 buffer and gives each
a gradient view into a second one (autograd accumulates into an existing ``.grad`` in place), so a step is a single
elementwise launch of ``matten_adam_step`` and ``zero_grad`` a single memset -- instead of the multi-tensor machinery
over ~60 small tensors.  State (step count included) lives on the device: a step captures into a hipGraph as it is
(``matten_amd.graphs.GraphedTrainStep``).  Same update rule and state names as ``torch.optim.Adam`` (amsgrad off).

Beyond the plain rule (all off by default; with all of them off the class calls ``matten_adam_step`` exactly as before):

* ``max_grad_norm``: the whole flat gradient is clipped to that 2-norm (``torch.nn.utils.clip_grad_norm_``'s formula; what
  Lightning's ``gradient_clip_val`` does for the reference) -- one more read of the gradients, no per-tensor machinery;
* ``skip_nonfinite``: a step whose gradient holds a NaN or an inf is dropped ON THE DEVICE: parameters, moments, EMA and
  step count keep their bits, ``skipped_steps`` counts it.  Works inside a replayed hipGraph, where no host could;
* ``ema_decay``: ``ema_params``, an exponential moving average of the parameters kept in the same launch
  (``with opt.ema_weights(): ...`` evaluates with it, ``copy_ema_to`` exports it);
* ``decoupled_weight_decay``: ``torch.optim.AdamW``'s rule;
* ``device_lr``: the learning rate is read from device memory, so a captured step follows a scheduler:
  ``sync_hyperparameters()`` writes ``param_groups[0]["lr"]`` there when it changed (``step()`` outside a capture and
  ``GraphedTrainStep.step`` before each replay call it).  Every option above implies it.

These go through ``matten_adam_step_ctl``: a chain of at most three launches on one stream (sum of squares, control,
update) with nothing read back.  ``last_grad_norm`` / ``last_clip_scale`` / ``skipped_steps`` read the device only when asked.
Without ``skip_nonfinite`` a non-finite gradient norm makes the clip scale, and so every parameter, NaN -- as under torch.
"""
import contextlib
import math
from typing import Iterable, Optional

import torch

from . import _lib, ops
from .nn._tables import bump_weights_epoch


class FlatAdam(torch.optim.Optimizer):
    def __init__(self, params: Iterable[torch.nn.Parameter], lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, max_grad_norm: Optional[float] = None, skip_nonfinite: bool = False,
                 ema_decay: Optional[float] = None, decoupled_weight_decay: bool = False, device_lr: bool = False):
        # the new arguments first: a bad value is reported as such wherever the parameters live
        if max_grad_norm is not None:
            max_grad_norm = self._checked_max_norm(max_grad_norm)
        if ema_decay is not None:
            if isinstance(ema_decay, bool) or not isinstance(ema_decay, (int, float)) or not 0.0 <= ema_decay < 1.0:
                raise ValueError(f"FlatAdam: ema_decay must be in [0, 1), got {ema_decay!r}")
            ema_decay = float(ema_decay)
        for name, flag in (("skip_nonfinite", skip_nonfinite), ("decoupled_weight_decay", decoupled_weight_decay),
                           ("device_lr", device_lr)):
            if not isinstance(flag, bool):
                raise ValueError(f"FlatAdam: {name} must be a bool, got {flag!r}")
        params = [p for p in params if p.requires_grad]
        if not params:
            raise ValueError("FlatAdam: no parameter requires a gradient")
        if any(p.dtype != torch.float32 or not p.is_cuda for p in params):
            raise _lib.MattenHipError("FlatAdam: parameters must be fp32 tensors on the MI355X (no CPU fallback)")
        if len({p.device for p in params}) != 1:
            raise ValueError("FlatAdam: all parameters on one device")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        dev = params[0].device
        # 16-byte aligned slots: the kernel moves four floats per lane
        offs, n = [], 0
        for p in params:
            offs.append(n)
            n += (p.numel() + 3) // 4 * 4
        self._n = n
        self.flat_params = torch.zeros(n, dtype=torch.float32, device=dev)
        self.flat_grads = torch.zeros(n, dtype=torch.float32, device=dev)
        self.exp_avg = torch.zeros(n, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=dev)
        self.step_count = torch.zeros(1, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for p, o in zip(params, offs):
                view = self.flat_params[o:o + p.numel()].view_as(p)
                view.copy_(p)
                p.data = view
                p.grad = self.flat_grads[o:o + p.numel()].view_as(p)
        self._params, self._offs = params, offs
        self.max_grad_norm, self.skip_nonfinite, self.ema_decay = max_grad_norm, skip_nonfinite, ema_decay
        self.decoupled_weight_decay = decoupled_weight_decay
        self.ctl = self.counters = self.ema_params = self._workspace = None
        self._lr_written, self._stepped = None, False
        if device_lr or skip_nonfinite or decoupled_weight_decay or max_grad_norm is not None or ema_decay is not None:
            self._enable_ctl()
        # the optimiser state under torch's names (state_dict / snapshotting tools look here); one entry for the lot
        self.state[params[0]] = self._state_entry()

    # ------------------------------------------------------------------------------------------------------------------
    # the device-control route (matten_adam_step_ctl)
    # ------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _checked_max_norm(value) -> float:
        if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(value) or not value > 0:
            raise ValueError(f"FlatAdam: max_grad_norm must be a finite number > 0, got {value!r}")
        return float(value)

    @property
    def device_control(self) -> bool:
        """whether steps go through matten_adam_step_ctl (any of the new constructor arguments, or device_lr=True)"""
        return self.ctl is not None

    def _enable_ctl(self) -> None:
        """allocate every tensor of the route NOW: GraphedTrainStep snapshots the optimiser state before its warm-up steps
        and zeroes whatever first appears during them -- the learning rate among it"""
        dev = self.flat_params.device
        self.ctl = torch.zeros(8, dtype=torch.float32, device=dev)
        self.counters = torch.zeros(2, dtype=torch.int32, device=dev)
        nbytes = int(_lib.load().matten_adam_ctl_workspace_bytes(self._n))
        self._workspace = torch.zeros(max(1, nbytes // 8), dtype=torch.float64, device=dev)
        if self.ema_decay is not None:
            self.ema_params = self.flat_params.clone()
        self._lr_written = None
        self.sync_hyperparameters()

    def _state_entry(self) -> dict:
        """the optimiser state under torch's names; the tensors of the device-control route only when it is on"""
        entry = {"step": self.step_count, "exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq}
        if self.device_control:
            entry.update(ctl=self.ctl, counters=self.counters, workspace=self._workspace)
            if self.ema_params is not None:
                entry["ema"] = self.ema_params
        return entry

    def _need_ctl(self, what: str) -> None:
        if not self.device_control:
            raise _lib.MattenHipError(f"FlatAdam.{what}: this optimiser steps through matten_adam_step, which keeps no such "
                                      "state; build it with max_grad_norm / skip_nonfinite / ema_decay / device_lr=True")

    def set_max_grad_norm(self, max_grad_norm: float) -> None:
        """switch global-norm clipping on, or change its bound (what Trainer(gradient_clip_val=...) calls).  An optimiser
        built without the device-control route can take it only before its first step: a step already captured in a
        hipGraph would go on replaying the old entry."""
        value = self._checked_max_norm(max_grad_norm)
        if not self.device_control:
            if self._stepped:
                raise _lib.MattenHipError("FlatAdam.set_max_grad_norm: the optimiser was built without max_grad_norm (or "
                                          "device_lr=True) and has already stepped; pass max_grad_norm to the constructor")
            self._enable_ctl()
            self.state[self._params[0]] = self._state_entry()
        self.max_grad_norm = value

    def sync_hyperparameters(self) -> None:
        """write param_groups[0]["lr"] into ctl[0] if it differs from what was last written (one small device fill; never
        inside a stream capture).  No-op without the device-control route, where lr is a kernel argument."""
        if not self.device_control:
            return
        lr = float(self.param_groups[0]["lr"])
        if lr != self._lr_written:
            self.ctl[0:1].fill_(lr)
            self._lr_written = lr

    @property
    def last_grad_norm(self) -> float:
        """2-norm of the whole flat gradient at the last step, before clipping (a host read); NaN when neither clipping
        nor the guard asked for it"""
        self._need_ctl("last_grad_norm")
        return float(self.ctl[1])

    @property
    def last_clip_scale(self) -> float:
        """the factor the last step's gradient was multiplied by (1: not clipped); a host read"""
        self._need_ctl("last_clip_scale")
        return float(self.ctl[2])

    @property
    def skipped_steps(self) -> int:
        """steps dropped by skip_nonfinite so far (a host read)"""
        self._need_ctl("skipped_steps")
        return int(self.counters[0])

    @contextlib.contextmanager
    def ema_weights(self):
        """run the block with the EMA in the live parameters; the training weights come back bit for bit on exit"""
        if self.ema_params is None:
            raise _lib.MattenHipError("FlatAdam.ema_weights: built without ema_decay")
        with torch.no_grad():
            backup = self.flat_params.clone()
            self.flat_params.copy_(self.ema_params)
        bump_weights_epoch()   # weight-derived caches (packed tables, folded BatchNorm) key on the epoch
        try:
            yield self
        finally:
            with torch.no_grad():
                self.flat_params.copy_(backup)
            bump_weights_epoch()

    @torch.no_grad()
    def copy_ema_to(self, model_or_params) -> None:
        """copy the EMA into another model (or parameter list) with the same trainable parameters in the same order"""
        if self.ema_params is None:
            raise _lib.MattenHipError("FlatAdam.copy_ema_to: built without ema_decay")
        params = model_or_params.parameters() if isinstance(model_or_params, torch.nn.Module) else model_or_params
        params = [p for p in params if p.requires_grad]
        if len(params) != len(self._params) or any(q.shape != p.shape for q, p in zip(params, self._params)):
            raise ValueError("FlatAdam.copy_ema_to: the target's trainable parameters do not match this optimiser's")
        for q, p, o in zip(params, self._params, self._offs):
            q.copy_(self.ema_params[o:o + p.numel()].view_as(p))
        bump_weights_epoch()

    def zero_grad(self, set_to_none: bool = False) -> None:
        """one memset; the gradient views stay in place (set_to_none would detach them from the flat buffer)"""
        self.flat_grads.zero_()
        for p, o in zip(self._params, self._offs):
            if p.grad is None or p.grad.data_ptr() != self.flat_grads.data_ptr() + 4 * o:
                p.grad = self.flat_grads[o:o + p.numel()].view_as(p)

    def load_state_dict(self, state_dict) -> None:
        """torch's loader would REPLACE the state entry with fresh tensors that step() never looks at (a resumed run would
        restart with zero moments and step 0): copy the loaded moments and step count into the live flat buffers and
        point ``self.state`` back at them.  Accepts what ``state_dict()`` of this class writes (one state entry holding
        the flat tensors) and what ``torch.optim.Adam`` over the same parameter list writes (one entry per parameter).
        On the device-control route the skip counters and the EMA come back too; a state saved without an EMA re-seeds
        the EMA from the current parameters, and the saved learning rate is written to the device."""
        groups, state = state_dict["param_groups"], state_dict["state"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self._params):
            raise ValueError("FlatAdam.load_state_dict: the saved optimiser covers a different parameter list")
        for k, v in groups[0].items():
            if k != "params":
                self.param_groups[0][k] = v
        ids = list(groups[0]["params"])
        with torch.no_grad():
            first = state.get(ids[0])
            own = first is not None and first["exp_avg"].numel() == self._n and len(state) == 1
            if self.device_control:
                saved = first if own else {}
                if "counters" in saved:
                    self.counters.copy_(saved["counters"])
                    self.ctl[1:3].copy_(saved["ctl"][1:3])
                else:
                    self.counters.zero_(), self.ctl[1:3].zero_()
                if self.ema_params is not None:
                    self.ema_params.copy_(saved["ema"].reshape(-1) if "ema" in saved else self.flat_params)
                self._lr_written = None
                self.sync_hyperparameters()
            if first is not None and first["exp_avg"].numel() == self._n and len(state) == 1:   # this class's own layout
                self.exp_avg.copy_(first["exp_avg"].reshape(-1))
                self.exp_avg_sq.copy_(first["exp_avg_sq"].reshape(-1))
                self.step_count.fill_(float(first["step"]))
            elif state:                                                                         # torch.optim.Adam's layout
                steps = set()
                for pid, p, o in zip(ids, self._params, self._offs):
                    st = state.get(pid)
                    if st is None:
                        raise ValueError(f"FlatAdam.load_state_dict: no state for parameter {pid}")
                    if st["exp_avg"].numel() != p.numel():
                        raise ValueError(f"FlatAdam.load_state_dict: state of parameter {pid} has the wrong size")
                    self.exp_avg[o:o + p.numel()].copy_(st["exp_avg"].reshape(-1))
                    self.exp_avg_sq[o:o + p.numel()].copy_(st["exp_avg_sq"].reshape(-1))
                    steps.add(float(st["step"]))
                if len(steps) != 1:
                    raise ValueError("FlatAdam.load_state_dict: parameters with different step counts")
                self.step_count.fill_(steps.pop())
            else:
                self.exp_avg.zero_(), self.exp_avg_sq.zero_(), self.step_count.zero_()
        self.state.clear()
        self.state[self._params[0]] = self._state_entry()

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        base = self.flat_params.data_ptr()
        for p, o in zip(self._params, self._offs):   # model.to() / .double() / p.data = ... after construction detach a parameter
            if p.data_ptr() != base + 4 * o:
                raise _lib.MattenHipError("FlatAdam: a parameter no longer lives in the flat buffer (model.to() / .double() / "
                                          "p.data = ... after the optimiser was built); build the optimiser last")
        for p, o in zip(self._params, self._offs):   # a gradient that was replaced (set_to_none, clipping into new tensors)
            if p.grad is not None and p.grad.data_ptr() != self.flat_grads.data_ptr() + 4 * o:
                self.flat_grads[o:o + p.numel()].view_as(p).copy_(p.grad)
                p.grad = self.flat_grads[o:o + p.numel()].view_as(p)
        g = self.param_groups[0]
        lib = _lib.load()
        self._stepped = True
        if self.device_control:
            if not torch.cuda.is_current_stream_capturing():
                self.sync_hyperparameters()
            ema = self.ema_params.data_ptr() if self.ema_params is not None else None
            # the kernels advance step_count themselves (not at all for a skipped step)
            _lib.check(lib.matten_adam_step_ctl(
                self.flat_params.data_ptr(), self.flat_grads.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
                ema, self._n, self.step_count.data_ptr(), self.ctl.data_ptr(), self.counters.data_ptr(),
                self._workspace.data_ptr(), self._workspace.numel() * 8, float(self.max_grad_norm or 0.0),
                float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]),
                float(self.ema_decay or 0.0), int(self.decoupled_weight_decay), int(self.skip_nonfinite), ops._stream()),
                "matten_adam_step_ctl")
            bump_weights_epoch()
            return loss
        self.step_count += 1.0
        _lib.check(lib.matten_adam_step(self.flat_params.data_ptr(), self.flat_grads.data_ptr(), self.exp_avg.data_ptr(),
                                        self.exp_avg_sq.data_ptr(), self._n, self.step_count.data_ptr(), float(g["lr"]),
                                        float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]),
                                        float(g["weight_decay"]), ops._stream()), "matten_adam_step")
        bump_weights_epoch()   # the kernel wrote through raw pointers: no parameter's _version moved
        return loss
