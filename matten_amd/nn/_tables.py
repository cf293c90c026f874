"""Device-resident copies of immutable plan tables, and version-tracked derived weights."""
import contextlib
from typing import Callable, Dict, Tuple

import numpy as np
import torch


class DeviceTables:
    """numpy tables uploaded lazily, once per device."""

    def __init__(self, **tables: np.ndarray):
        self._host = {k: np.ascontiguousarray(v) for k, v in tables.items()}
        self._dev: Dict[Tuple[str, torch.device], torch.Tensor] = {}

    def get(self, name: str, device) -> torch.Tensor:
        device = torch.device(device)
        key = (name, device)
        t = self._dev.get(key)
        if t is None:
            t = torch.from_numpy(self._host[name]).to(device)
            self._dev[key] = t
        return t


# Writes that torch's version counters cannot see: FlatAdam updates every parameter through the raw pointer of its flat
# buffer, a hipGraph replay re-runs a captured optimiser step, matten_bn_train_fwd updates the running statistics in
# place.  Each of them bumps this process-wide epoch, which is part of every cache key below, so an eval forward after a
# training step never reuses packs derived from the previous weights.
_WEIGHTS_EPOCH = [0]


def bump_weights_epoch() -> None:
    _WEIGHTS_EPOCH[0] += 1


def weights_epoch() -> int:
    return _WEIGHTS_EPOCH[0]


# A captured eval-mode step (graphs.GraphedModelStep, "val" / "test") reads the caches below as they are at capture time:
# the graph holds the ADDRESSES of their tensors, and the weights move between its replays.  ``record_derived`` collects,
# in order of use, every (cache, arguments) pair asked for inside its block and pins those caches: a pinned cache
# refreshes IN PLACE, so the addresses stay good, and ``refresh_derived`` re-asks the recorded pairs (eagerly, before a
# replay), which recomputes exactly the stale ones.  Nothing changes for a cache that was never recorded.
_RECORDER = [None]


@contextlib.contextmanager
def record_derived():
    outer, mine = _RECORDER[0], []
    _RECORDER[0] = mine
    try:
        yield mine
    finally:
        _RECORDER[0] = outer


def refresh_derived(recorded) -> None:
    for cache, args in recorded:
        cache.get(*args)


def _record(cache, args) -> None:
    rec = _RECORDER[0]
    cache._pinned = True
    if not any(c is cache and len(a) == len(args) and all(x is y for x, y in zip(a, args)) for c, a in rec):
        rec.append((cache, args))


def _refresh_in_place(old, new):
    """copy `new` into the tensors of `old` (same nesting, shapes, dtypes and devices) and return `old`"""
    if isinstance(old, torch.Tensor) and isinstance(new, torch.Tensor):
        if old.device != new.device:
            return new      # the model moved: steps captured on the old device are not its steps any more
        if old.shape == new.shape and old.dtype == new.dtype and old.device == new.device:
            return old.copy_(new)
    elif isinstance(old, (tuple, list)) and type(old) is type(new) and len(old) == len(new):
        return type(old)(_refresh_in_place(o, n) for o, n in zip(old, new))
    elif not isinstance(new, torch.Tensor) and old == new:
        return old
    raise RuntimeError("a weight-derived pack that a captured step reads changed its layout; capture the step again")


class DerivedWeight:
    """Caches f(*params) until any parameter changes (optimizer step, load_state_dict, .to(), or a raw in-place write
    announced through ``bump_weights_epoch``)."""

    def __init__(self, fn: Callable[..., torch.Tensor]):
        self._fn = fn
        self._key = None
        self._val = None
        self._pinned = False

    def get(self, *params: torch.Tensor):
        if _RECORDER[0] is not None:
            _record(self, params)
        key = (_WEIGHTS_EPOCH[0],) + tuple((p.data_ptr(), p._version, p.device, p.dtype) for p in params)
        if key != self._key:
            with torch.no_grad():
                val = self._fn(*params)
                self._val = _refresh_in_place(self._val, val) if self._pinned and self._val is not None else val
            self._key = key
        return self._val


class WeightSlice:
    """``w.index_select(dim, idx)`` kept in ONE persistent buffer that is refreshed in place whenever the source
    parameter changes (its ``_version`` then moves too, so DerivedWeight caches keyed on the buffer notice)."""

    def __init__(self, idx: np.ndarray, dim: int = 0):
        idx = np.asarray(idx, dtype=np.int64)
        self._idx = DeviceTables(idx=idx)
        self._dim = dim
        self._key = None
        self._buf = None
        self._n = int(idx.size)
        self._identity = bool(idx.size and (idx == np.arange(idx.size)).all())

    def select(self, w: torch.Tensor) -> torch.Tensor:
        """the same slice inside autograd (training): gradients flow back to ``w``, zeros where nothing was selected"""
        if self._identity and w.shape[self._dim] == self._n:
            return w
        return w.index_select(self._dim, self._idx.get("idx", w.device))

    def get(self, w: torch.Tensor) -> torch.Tensor:
        if _RECORDER[0] is not None:
            _record(self, (w,))
        key = (_WEIGHTS_EPOCH[0], w.data_ptr(), w._version, w.device, w.dtype)
        if key != self._key:
            with torch.no_grad():
                new = w.detach().index_select(self._dim, self._idx.get("idx", w.device))
                if self._buf is None or self._buf.device != w.device or self._buf.dtype != w.dtype:
                    self._buf = new.contiguous()
                else:
                    self._buf.copy_(new)
            self._key = key
        return self._buf
