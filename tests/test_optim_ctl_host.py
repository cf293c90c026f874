"""
CPU tests of FlatAdam's device-control route (matten_adam_step_ctl: global-norm clipping, the non-finite guard, EMA,
decoupled weight decay, the learning rate on the device): declarations and bindings, the entry's argument checks, the
workspace query and the order of the constructor's errors.  No kernel is launched: every call below returns from the
argument checks (n == 0, or a bad pointer / alignment / workspace size with host buffers that are never dereferenced).
"""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL = 0, -1


def test_library_declares_and_binds_the_two_entries():
    from matten_amd import _lib

    header = open(os.path.join(ROOT, "include", "matten_hip.h")).read()
    declared = set(re.findall(r"\b(matten_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in ("matten_adam_step_ctl", "matten_adam_ctl_workspace_bytes", "matten_adam_step"):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.ABI_VERSION == 47 and lib.matten_abi_version() == 47          # entries were only added
    assert len(_lib.SIGNATURES["matten_adam_step_ctl"][1]) == 20
    assert len(_lib.SIGNATURES["matten_adam_step"][1]) == 12                  # the old entry keeps its signature


def test_workspace_is_a_function_of_n_alone_and_capped():
    from matten_amd import _lib

    q = _lib.load().matten_adam_ctl_workspace_bytes
    assert q(0) == 0 and q(-5) == 0
    assert q(1) == 8 and q(1024) == 8 and q(1025) == 16                       # one fp64 partial per 1024-float workgroup tile
    assert q(1024 * 1024) == 8192 and q(1024 * 1024 + 1) == 8192 and q(10 ** 10) == 8192   # at most 1024 workgroups
    sizes = [q(n) for n in range(1, 5000, 37)]
    assert sizes == sorted(sizes)


def _aligned(nbytes, align=16):
    """a host buffer and an address inside it on an `align`-byte boundary (the buffer must outlive the address)"""
    buf = (ctypes.c_char * (nbytes + align))()
    base = ctypes.addressof(buf)
    return buf, base + (-base) % align


def test_entry_checks_its_arguments_before_it_launches_anything():
    from matten_amd import _lib

    lib = _lib.load()
    f = lib.matten_adam_step_ctl

    def call(n=0, ptrs=None, ws_bytes=0, max_norm=1.0, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, d=0.999, decoupled=0, guard=1):
        p = dict(params=None, grads=None, m=None, v=None, ema=None, step=None, ctl=None, counters=None, ws=None)
        p.update(ptrs or {})
        return f(p["params"], p["grads"], p["m"], p["v"], p["ema"], n, p["step"], p["ctl"], p["counters"], p["ws"], ws_bytes,
                 max_norm, b1, b2, eps, wd, d, decoupled, guard, None)

    nan = float("nan")
    # scalar arguments: refused whatever n is, before the n == 0 return
    assert call(n=-1) == EINVAL
    for bad in (dict(b1=1.0), dict(b1=-0.1), dict(b1=nan), dict(b2=1.0), dict(b2=-1e-3), dict(b2=nan), dict(eps=-1e-8),
                dict(eps=nan), dict(d=1.0), dict(d=-0.5), dict(d=nan), dict(max_norm=-1.0), dict(max_norm=nan)):
        assert call(**bad) == EINVAL, bad
    # n == 0: nothing to do, no pointer is looked at
    assert call() == OK
    assert call(max_norm=0.0, guard=0, d=0.0, decoupled=1) == OK
    # n > 0: pointers, alignment and workspace size are refused before any launch (the buffers are host memory)
    n = 8
    keep = [_aligned(4 * n) for _ in range(5)] + [_aligned(4), _aligned(32), _aligned(8), _aligned(8)]
    names = ("params", "grads", "m", "v", "ema", "step", "ctl", "counters", "ws")
    good = {k: a for k, (_, a) in zip(names, keep)}
    need = lib.matten_adam_ctl_workspace_bytes(n)
    assert need == 8
    for k in names:
        if k != "ema":                                                        # ema is optional; every other pointer is not
            assert call(n=n, ptrs=dict(good, **{k: None}), ws_bytes=need) == EINVAL, k
    for k in ("params", "grads", "m", "v", "ema"):                            # flat buffers on a 16-byte boundary
        for off in (4, 8):
            assert call(n=n, ptrs=dict(good, **{k: good[k] + off}), ws_bytes=need) == EINVAL, (k, off)
    assert call(n=n, ptrs=good, ws_bytes=need - 1) == EINVAL                  # workspace smaller than the query says
    assert call(n=n, ptrs=good, ws_bytes=0) == EINVAL
    assert call(n=2 ** 20 + 4, ptrs=good, ws_bytes=8191) == EINVAL
    assert call(n=n, ptrs=dict(good, params=good["params"] + 4), ws_bytes=0) == EINVAL


def _cpu_params():
    return [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))]


@pytest.mark.parametrize("kwargs,match", [
    (dict(max_grad_norm=0.0), "max_grad_norm"), (dict(max_grad_norm=-1.0), "max_grad_norm"),
    (dict(max_grad_norm=float("inf")), "max_grad_norm"), (dict(max_grad_norm=float("nan")), "max_grad_norm"),
    (dict(max_grad_norm="10"), "max_grad_norm"), (dict(max_grad_norm=True), "max_grad_norm"),
    (dict(ema_decay=1.0), "ema_decay"), (dict(ema_decay=-0.1), "ema_decay"), (dict(ema_decay=float("nan")), "ema_decay"),
    (dict(ema_decay="0.9"), "ema_decay"),
    (dict(skip_nonfinite=1), "skip_nonfinite"), (dict(decoupled_weight_decay="yes"), "decoupled_weight_decay"),
    (dict(device_lr=None), "device_lr"),
])
def test_constructor_reports_a_bad_option_before_the_device_error(kwargs, match):
    from matten_amd.optim import FlatAdam

    with pytest.raises(ValueError, match=match):
        FlatAdam(_cpu_params(), lr=1e-2, **kwargs)


def test_constructor_with_valid_options_reaches_the_device_error():
    from matten_amd import _lib
    from matten_amd.optim import FlatAdam

    for kwargs in (dict(), dict(max_grad_norm=10.0, ema_decay=0.999, skip_nonfinite=True), dict(ema_decay=0.0),
                   dict(max_grad_norm=1, decoupled_weight_decay=True, device_lr=True)):
        with pytest.raises(_lib.MattenHipError, match="MI355X"):
            FlatAdam(_cpu_params(), lr=1e-2, **kwargs)


def test_trainer_takes_lightnings_gradient_clip_val():
    from matten_amd.model.trainer import Trainer

    assert Trainer().gradient_clip_val is None
    assert Trainer(max_epochs=2, gradient_clip_val=10.0).gradient_clip_val == 10.0
