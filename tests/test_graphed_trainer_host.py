"""Host side of the graphed Trainer (no GPU): the valid-loss entries are declared, bound and exported and check their
arguments before they launch; ``valid_loss_host`` is the plain fp64 formula; ``valid_mean_loss``, ``pad_eval``,
``BucketedModelStep`` and ``Trainer(graphed=True)`` refuse what they cannot run, the Trainer before any step; the routing of
``shared_step`` under ``loss_over_valid_rows``; the bucket shapes of a padded validation loader."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from common import LMAX2
from store_cases import TARGET, data_module, golden_graphs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, ENOMEM = 0, -1, -3


# ----------------------------------------------------------------------------------------------------------------------
# the C entries
# ----------------------------------------------------------------------------------------------------------------------
def test_library_declares_binds_and_exports_the_valid_loss_entries():
    from matten_amd import _lib

    header = open(os.path.join(ROOT, "include", "matten_hip.h")).read()
    declared = set(re.findall(r"\b(matten_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in ("matten_valid_loss", "matten_valid_loss_bwd", "matten_valid_loss_workspace_bytes"):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 47 and lib.matten_abi_version() == 47          # entries were only added
    assert len(_lib.SIGNATURES["matten_valid_loss"][1]) == 12
    assert len(_lib.SIGNATURES["matten_valid_loss_bwd"][1]) == 10


def test_valid_loss_workspace_holds_two_sums_and_a_count_per_workgroup():
    from matten_amd import _lib

    lib = _lib.load()
    q, tile, cap = lib.matten_valid_loss_workspace_bytes, lib.matten_selected_loss_tile_elems(), lib.matten_selected_loss_max_blocks()
    assert q(0, 6) == 0 and q(-1, 6) == 0 and q(5, 0) == 0
    assert q(1, 1) == 0 and q(tile, 1) == 0 and q(tile // 21, 21) == 0        # one workgroup writes the results itself
    assert q(tile + 1, 1) == 48 and q(tile // 21 + 1, 21) == 48
    assert q(cap * tile, 1) == 24 * cap == q(cap * tile + 1, 1) == q(10 ** 8, 9)
    # the selected-loss query is what it was
    assert lib.matten_selected_loss_workspace_bytes(tile + 1, 1) == 32


def _host(nbytes, align=16):
    buf = (ctypes.c_char * (nbytes + align))()
    base = ctypes.addressof(buf)
    return buf, base + (-base) % align


def test_valid_loss_entries_check_their_arguments_before_they_launch_anything():
    """host pointers, never dereferenced: every call returns from the argument checks"""
    from matten_amd import _lib

    lib = _lib.load()
    tile = lib.matten_selected_loss_tile_elems()
    keep = {k: _host(64) for k in ("pred", "target", "n_valid", "sums", "count", "loss", "ws", "g", "grad")}
    good = {k: a for k, (_, a) in keep.items()}

    def fwd(n_rows=4, d=6, kind=0, ws_bytes=0, **ptrs):
        p = dict(good, **ptrs)
        return lib.matten_valid_loss(p["pred"], p["target"], p["n_valid"], n_rows, d, kind, p["sums"], p["count"], p["loss"],
                                     p["ws"], ws_bytes, None)

    def bwd(n_rows=4, d=6, kind=0, **ptrs):
        p = dict(good, **ptrs)
        return lib.matten_valid_loss_bwd(p["pred"], p["target"], p["n_valid"], n_rows, d, kind, p["g"], p["count"], p["grad"],
                                         None)

    for call in (fwd, bwd):
        assert call(n_rows=-1) == EINVAL
        assert call(d=0) == EINVAL and call(d=-3) == EINVAL
        assert call(kind=2) == EINVAL and call(kind=-1) == EINVAL
        assert call(n_rows=2 ** 28, d=8) == EINVAL                            # n_rows * d reaches 2^31
        for k in ("pred", "target", "n_valid", "count"):
            assert call(**{k: None}) == EINVAL, k
        assert call(n_valid=good["n_valid"] + 4) == EINVAL                    # an 8-byte word
        assert call(n_rows=0, n_valid=None) == EINVAL                         # whatever n_rows is
    for k in ("sums", "loss"):
        assert fwd(**{k: None}) == EINVAL, k
    assert fwd(sums=good["sums"] + 4) == EINVAL and fwd(count=good["count"] + 4) == EINVAL
    for k in ("g", "grad"):
        assert bwd(**{k: None}) == EINVAL, k
    assert fwd(n_rows=0, sums=None) == EINVAL
    assert bwd(n_rows=0, pred=None, target=None, grad=None) == OK
    rows = tile // 6 + 1
    need = lib.matten_valid_loss_workspace_bytes(rows, 6)
    assert need == 48
    assert fwd(n_rows=rows, ws=None, ws_bytes=need) == EINVAL
    assert fwd(n_rows=rows, ws=good["ws"] + 4, ws_bytes=need) == EINVAL
    assert fwd(n_rows=rows, ws_bytes=need - 1) == ENOMEM
    assert fwd(n_rows=rows, ws_bytes=0) == ENOMEM


# ----------------------------------------------------------------------------------------------------------------------
# the restatement and the wrappers
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("n_valid", [0, 1, 6, 7, 12, -3])
def test_valid_loss_host_is_the_plain_formula(kind, n_valid):
    from matten_amd.ops import valid_loss_bwd_host, valid_loss_host

    g = torch.Generator().manual_seed(5)
    pred, target = torch.randn(7, 21, generator=g), torch.randn(7, 21, generator=g)
    k = min(max(n_valid, 0), 7)
    loss, sums, count = valid_loss_host(pred.numpy(), target.numpy(), n_valid, kind)
    x = pred[:k].double() - target[:k].double()
    assert count == k and isinstance(count, int) and sums.dtype == np.float64 and sums.shape == (2,)
    assert loss.dtype == np.float32
    np.testing.assert_allclose(sums, [float((x * x).sum()), float(x.abs().sum())], rtol=1e-14, atol=0)
    p = pred.double().clone().requires_grad_(True)
    if k:
        per = (p[:k] - target[:k].double()) ** 2 if kind == 0 else (p[:k] - target[:k].double()).abs()
        want = per.mean()
        assert abs(float(loss) - float(want.detach())) <= 1e-7 * float(want.detach())
        (0.5 * want).backward()
        grad = valid_loss_bwd_host(pred.numpy(), target.numpy(), n_valid, kind, g=0.5)
        assert grad.dtype == np.float32 and grad.shape == (7, 21)
        np.testing.assert_allclose(grad, p.grad.float().numpy(), rtol=1e-6, atol=0)
        assert not grad[k:].any() and not np.signbit(grad[k:]).any()
    else:
        assert loss == 0 and not sums.any()
        assert not valid_loss_bwd_host(pred.numpy(), target.numpy(), n_valid, kind).any()
    # what a padding row holds does not matter
    junk = pred.clone()
    junk[k:] = float("nan")
    again = valid_loss_host(junk.numpy(), target.numpy(), n_valid, kind)
    assert again[0] == loss and (again[1] == sums).all()
    assert valid_loss_host(pred.numpy(), target.numpy(), n_valid, "mae" if kind else "mse")[0] == loss
    with pytest.raises(ValueError, match="kind"):
        valid_loss_host(pred.numpy(), target.numpy(), 3, 2)


def test_valid_mean_loss_and_ops_refuse_what_they_cannot_run():
    from matten_amd import _lib, ops
    from matten_amd.autograd import ValidLossFn
    from matten_amd.graphs import padded_mean_loss, valid_mean_loss

    loss = valid_mean_loss("mse", key=TARGET)
    assert loss.wants_batch
    pred, target = torch.zeros(4, 21), torch.zeros(4, 21)
    with pytest.raises(ValueError, match=r"needs a padded batch .*this batch has no '_amd_n_valid'") as mine:
        loss({TARGET: pred}, target, {})
    with pytest.raises(ValueError) as theirs:
        padded_mean_loss(lambda p, t: (p - t) ** 2, key=TARGET)({TARGET: pred}, target, {})
    assert str(mine.value).replace("valid_mean_loss", "padded_mean_loss") == str(theirs.value)
    n_valid = torch.tensor([9, 40, 3], dtype=torch.int64)
    with pytest.raises(_lib.MattenHipError, match="no CPU fallback"):
        loss({TARGET: pred}, target, {"_amd_n_valid": n_valid})
    with pytest.raises(ValueError, match="kind"):
        valid_mean_loss("huber")
    with pytest.raises(ValueError, match="kind"):
        ops.valid_loss(pred, target, n_valid[2:3], 2)
    with pytest.raises(_lib.MattenHipError, match="no CPU fallback"):
        ops.valid_loss(pred, target, n_valid[2:3], 0)
    with pytest.raises(_lib.MattenHipError, match="no CPU fallback"):
        ops.valid_loss_bwd(pred, target, n_valid[2:3], 0, torch.ones(()), torch.ones((), dtype=torch.int64))
    with pytest.raises(_lib.MattenHipError, match="no CPU fallback"):
        ValidLossFn.apply(pred, target, n_valid[2:3], 1)


# ----------------------------------------------------------------------------------------------------------------------
# the data module
# ----------------------------------------------------------------------------------------------------------------------
def test_pad_eval_needs_the_padded_device_loader():
    with pytest.raises(ValueError, match=r"pad_eval=True .*device_resident=True and loader_kwargs\['pad'\]"):
        data_module(pad_eval=True)
    with pytest.raises(ValueError, match=r"pad_eval=True .*needs loader_kwargs\['pad'\]$"):
        data_module(pad_eval=True, device_resident=True, device="cuda:0")
    with pytest.raises(ValueError, match="device_resident=True"):
        data_module(pad_eval=True, loader_kwargs={"pad": (64, 2048)})
    kw = dict(batch_size=32, shuffle=True, seed=3, pad=(64, 2048), pad_species=14, pad_length=1.5)
    off = data_module(device_resident=True, device="cuda:0", loader_kwargs=kw)
    assert off.pad_eval is False
    assert off._eval_kwargs() == dict(batch_size=32, shuffle=False, seed=3)                  # as before
    on = data_module(device_resident=True, device="cuda:0", loader_kwargs=kw, pad_eval=True)
    assert on._eval_kwargs() == dict(kw, shuffle=False)


def test_padded_validation_loader_has_a_few_bucket_shapes():
    from matten_amd.data.store import GraphStoreHost
    from matten_amd.dataset.structure_scalar_tensor import _DeviceLoader

    dm = data_module(device_resident=True, device="cuda:0", pad_eval=True,
                     loader_kwargs=dict(batch_size=32, shuffle=True, seed=3, pad=(64, 2048)))
    loader = _DeviceLoader(GraphStoreHost(list(golden_graphs())), training=False, **dm._eval_kwargs())
    first, second = loader.batch_indices(), loader.batch_indices()
    assert first == second and first[0] == list(range(32)) and [len(i) for i in first] == [32, 32, 32, 4]   # unshuffled
    shapes = [loader.padded_sizes(idx) for idx in first]
    assert all(n % 64 == 0 and e % 2048 == 0 and b == 33 for n, e, b in shapes)
    # one bucket per batch here, all within Trainer's default max_graphs = 8 (the graphed GPU tests count on more than one);
    # unpadded, the four batches have four shapes as well, but a new set for every other batch size or file
    assert shapes == [(192, 4096, 33), (128, 4096, 33), (192, 8192, 33), (64, 2048, 33)]


# ----------------------------------------------------------------------------------------------------------------------
# the model shell
# ----------------------------------------------------------------------------------------------------------------------
def _species_hparams():
    from matten_amd.data.graph import average_num_neighbors

    graphs = golden_graphs()
    species = sorted({int(z) for g in graphs for z in g["atomic_numbers"].tolist()})
    return {"allowed_species": species, "average_num_neighbors": average_num_neighbors(list(graphs))}


def _cpu_model(**kw):
    from matten_amd.model_factory.tfn_scalar_tensor import ScalarTensorModel

    return ScalarTensorModel(backbone_hparams=dict(LMAX2), dataset_hparams=_species_hparams(), **kw)


def _padded_cpu_batch(model, k=2):
    """three golden crystals and `k` stand-in padding crystals (zero targets), with the count words of a padded batch; the
    decode is stubbed: the forward needs the device, the routing does not"""
    from matten_amd.data.graph import collate

    batch = collate(list(golden_graphs()[:3 + k]))
    batch[TARGET] = torch.cat([batch[TARGET][:3], torch.zeros(k, 21)])
    batch["_amd_n_valid"] = torch.tensor([0, 0, 3], dtype=torch.int64)
    decoded = {TARGET: torch.randn(3 + k, 21, generator=torch.Generator().manual_seed(1)).requires_grad_(True)}
    model.decode = lambda graphs: decoded
    return batch, decoded


def test_loss_over_valid_rows_is_off_by_default_and_routes_shared_step():
    from matten_amd import _lib
    from matten_amd.model.model import BaseModel

    assert BaseModel.loss_over_valid_rows is False
    model = _cpu_model()
    assert model.loss_over_valid_rows is False and "loss_over_valid_rows" not in model.state_dict()
    batch, decoded = _padded_cpu_batch(model)
    # off: today's route, the plain mean over every row, padding included, on any device
    loss, preds, labels = model.shared_step(batch, "train")
    assert torch.equal(loss, torch.nn.functional.mse_loss(decoded[TARGET], batch[TARGET]))
    assert set(labels) == {TARGET}
    model.update_metrics(preds, labels, "train")
    assert float(model.metrics["metric_train"][TARGET]["MeanAbsoluteError"].count) == 5 * 21
    # on: the kernel's wrapper, which refuses CPU tensors like every other op
    model.loss_over_valid_rows = True
    with pytest.raises(_lib.MattenHipError, match="no CPU fallback"):
        model.shared_step(batch, "train")
    with pytest.raises(NotImplementedError, match="target_weight"):
        model.shared_step(dict(batch, target_weight=torch.ones(5, 1)), "train")
    model.loss_fns[TARGET] = torch.nn.HuberLoss()
    with pytest.raises(NotImplementedError, match="HuberLoss"):
        model.shared_step(batch, "train")
    model.loss_fns[TARGET] = torch.nn.MSELoss(reduction="sum")
    with pytest.raises(NotImplementedError, match="MSELoss"):
        model.shared_step(batch, "train")
    model.loss_fns[TARGET] = torch.nn.L1Loss()       # supported: past the routing, into the wrapper
    with pytest.raises(_lib.MattenHipError, match="no CPU fallback"):
        model.shared_step(batch, "train")
    with pytest.raises(_lib.MattenHipError, match="no CPU fallback"):
        model.update_metrics(decoded, {TARGET: batch[TARGET], "_amd_n_valid": batch["_amd_n_valid"][2:3]}, "val")
    # a batch without the count words keeps today's route whatever the flag says
    model.loss_fns[TARGET] = torch.nn.MSELoss()
    plain = {k: v for k, v in batch.items() if k != "_amd_n_valid"}
    assert torch.equal(model.shared_step(plain, "val")[0], loss)


def test_metric_reuses_the_sums_of_the_loss_call():
    """MeanAbsoluteError(..., n_valid=, valid_sums=) adds sums[1] and count * d without a call of its own (host tensors)"""
    from matten_amd.model_factory.task import MeanAbsoluteError, MetricCollection

    metric = MetricCollection({"MeanAbsoluteError": MeanAbsoluteError()})
    pred, target = torch.zeros(5, 21), torch.zeros(5, 21)
    sums, count = torch.tensor([9.0, 6.3], dtype=torch.float64), torch.tensor(3, dtype=torch.int64)
    for _ in range(2):
        metric(pred, target, n_valid=torch.tensor([3]), valid_sums=(sums, count))
    m = metric["MeanAbsoluteError"]
    assert float(m.sum_abs) == 12.6 and float(m.count) == 2 * 3 * 21 and m.count.dtype == torch.float64
    assert abs(float(metric.compute()["MeanAbsoluteError"]) - 0.1) < 1e-7
    with pytest.raises(ValueError, match="selector and n_valid"):
        m(pred, target, selector=torch.ones(5, dtype=torch.int32), n_valid=torch.tensor([3]))


# ----------------------------------------------------------------------------------------------------------------------
# the steps and the Trainer
# ----------------------------------------------------------------------------------------------------------------------
def test_bucketed_model_step_checks_mode_and_optimizer():
    from matten_amd.graphs import BucketedModelStep

    model = _cpu_model()
    opt = torch.optim.Adam(model.parameters(), capturable=True)
    with pytest.raises(ValueError, match="mode"):
        BucketedModelStep(model, "predict")
    with pytest.raises(ValueError, match="optimizer"):
        BucketedModelStep(model, "train")
    with pytest.raises(ValueError, match="optimizer"):
        BucketedModelStep(model, "val", opt)
    step = BucketedModelStep(model.eval(), "train", opt, max_graphs=0)
    assert step.counts == {"captures": 0, "replays": 0, "eager_steps": 0}
    batch, _ = _padded_cpu_batch(model)
    with pytest.raises(ValueError, match=r"model.train\(\) first"):
        step.step(batch)


class _NoStep(Exception):
    pass


def _refusing_model(optimizer_hparams, lr_scheduler_hparams=None):
    model = _cpu_model(optimizer_hparams=optimizer_hparams, lr_scheduler_hparams=lr_scheduler_hparams)

    def no_step(*a, **k):
        raise _NoStep("a step ran before the refusal")

    model.training_step = model.validation_step = model.decode = no_step
    return model


def test_graphed_trainer_refuses_before_the_first_step():
    from matten_amd.model.trainer import Trainer

    batches = [{"never": "read"}]
    adam = {"class_path": "torch.optim.Adam", "init_args": {"lr": 1e-2}}
    capturable = {"class_path": "torch.optim.Adam", "init_args": {"lr": 1e-2, "capturable": True}}
    plateau = {"class_path": "torch.optim.lr_scheduler.ReduceLROnPlateau", "init_args": {"factor": 0.5, "patience": 0}}

    model = _refusing_model(adam)
    with pytest.raises(ValueError, match=r"Adam cannot be captured.*matten_amd\.optim\.FlatAdam"):
        Trainer(graphed=True).fit(model, train_dataloaders=batches)
    assert model.loss_over_valid_rows is False
    with pytest.raises(ValueError, match=r"scheduler.*FlatAdam\(device_lr=True\)"):
        Trainer(graphed=True).fit(_refusing_model(capturable, plateau), train_dataloaders=batches)
    with pytest.raises(ValueError, match=r"gradient_clip_val.*FlatAdam"):
        Trainer(graphed=True, gradient_clip_val=1.0).fit(_refusing_model(capturable), train_dataloaders=batches)
    # the eager Trainer takes all three and reaches the step
    for hp, sched, clip in ((adam, None, None), (capturable, plateau, None), (capturable, None, 1.0)):
        with pytest.raises(_NoStep):
            Trainer(gradient_clip_val=clip).fit(_refusing_model(hp, sched), train_dataloaders=batches)


def test_graphed_trainer_restores_the_flag_when_a_step_raises():
    from matten_amd.model.trainer import Trainer

    model = _refusing_model({"class_path": "torch.optim.Adam", "init_args": {"lr": 1e-2, "capturable": True}})
    seen = []

    def step(batch, i):
        seen.append(model.loss_over_valid_rows)
        raise _NoStep()

    model.training_step = step
    batch, _ = _padded_cpu_batch(_cpu_model())
    trainer = Trainer(graphed=True, max_graphs=0)      # no graph: the step runs eagerly, and is counted
    with pytest.raises(_NoStep):
        trainer.fit(model, train_dataloaders=[batch])
    assert seen == [True] and model.loss_over_valid_rows is False
    assert trainer.step_counts == {"train": {"captures": 0, "replays": 0, "eager_steps": 1}}
    assert Trainer().step_counts == {} and Trainer().graphed is False
