"""Per-atom tensor training on the GPU (reference scripts/train_atomic_tensor.py): the dense label layout through the
device store and its padded batches, one training step of ``AtomicTensorModel`` on a padded dense batch against the
oracle on the plain compact one, ``shared_step`` on both layouts, two epochs of bucketed captured steps, and
``Trainer.fit`` on a device-resident data module.  Everything reads tests/golden/si_nmr_n12.json."""
import copy

import pytest
import torch

from common import ATOMIC, build_pair
from test_atom_targets_host import FIXTURE, SELECTED, TARGET, data_module, fixture_dataset_hparams, fixture_graphs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALE = dict(tensor_target_scale=0.01)
CORE = ("pos", "edge_index", "edge_cell_shift", "cell", "num_neigh", "atomic_numbers", "batch", "ptr")


def _close(got, want, rtol, what):
    """the measure of tests/test_gpu_training.py: the largest error against the largest reference magnitude"""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = max(1e-12, want.abs().max().item())
    err = (got - want).abs().max().item()
    print(f"{what}: max err {err:.3e} vs scale {scale:.3e} (bound {rtol:.0e})")
    assert err <= rtol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


def _round_up(v, q):
    return q * -(-v // q)


@pytest.fixture(scope="module")
def dense():
    return fixture_graphs("dense", **SCALE)


@pytest.fixture(scope="module")
def compact():
    return fixture_graphs("compact", **SCALE)


@pytest.fixture(scope="module")
def store(dense):
    from matten_amd.data.store import DeviceGraphStore

    return DeviceGraphStore.from_graphs(dense, DEV)


# ----------------------------------------------------------------------------------------------------------------------
# 1. the dense keys through the store
# ----------------------------------------------------------------------------------------------------------------------
def test_store_batches_carry_the_dense_labels(store, dense):
    from matten_amd.data.graph import collate

    for idx in ([0], [9, 2, 11, 0], list(range(12))):
        want = collate([dense[i] for i in idx])
        got = store.batch(idx)
        assert [k for k in got if not k.startswith("_amd_")] == list(want.keys())
        for k, v in want.items():
            assert got[k].dtype == v.dtype and torch.equal(got[k].cpu(), v), k
        n = want["pos"].shape[0]
        for k in (1, 3):
            pad_to = (_round_up(n + k, 32), _round_up(want["edge_index"].shape[1], 1024), len(idx) + k)
            padded, ref = store.batch(idx, pad_to=pad_to), store.host.padded_reference(idx, pad_to)
            assert list(padded.keys()) == list(ref.keys())
            for key, v in ref.items():
                assert padded[key].dtype == v.dtype and torch.equal(padded[key].cpu(), v), key
            assert padded["atom_selector"].dtype == torch.int32 and padded[TARGET].shape == (pad_to[0], 6)
            assert not padded["atom_selector"][n:].any() and not padded[TARGET][n:].any()    # padding rows are unselected
            assert int(padded["atom_selector"].sum()) == sum(SELECTED[i] for i in idx)


# ----------------------------------------------------------------------------------------------------------------------
# 2. one training step against the oracle
# ----------------------------------------------------------------------------------------------------------------------
def _oracle_step(ref, compact, n_crystals):
    from matten_amd.data.graph import collate

    cpu = collate(compact[:n_crystals])
    sel = cpu["atom_selector"]
    out = ref.decode({k: cpu[k] for k in CORE})
    loss = torch.nn.functional.mse_loss(out[sel], cpu[TARGET])
    ref.zero_grad()
    loss.backward()
    return out, loss, {name: p.grad.clone() for name, p in ref.named_parameters() if p.grad is not None}


def _compare_step(ref, model, out_m, loss_m, out_r, loss_r, grads_r, bounds):
    fwd, los, grd, buf = bounds
    _close(out_m, out_r, fwd, "train-mode forward [N,6]")
    _close(loss_m, loss_r, los, "loss")
    named = dict(model.named_parameters())
    assert set(grads_r) <= set(named)
    for name, g in grads_r.items():
        assert named[name].grad is not None, name
        _close(named[name].grad, g, grd, f"grad {name}")
    bufs_m = dict(model.named_buffers())
    checked = 0
    for name, b in ref.named_buffers():
        if name.endswith(("running_mean", "running_var")):
            _close(bufs_m[name], b, buf, name)
            checked += 1
    assert checked > 0


@pytest.mark.parametrize("k", [1, 3])
def test_padded_dense_training_step_matches_oracle_autograd(store, compact, k):
    """The device side runs the store's padded dense batch (quanta (32, 1024), K padding crystals) through
    selected_mean_loss, the oracle mse_loss(out[sel], compact_target) on the plain collate of the 10 real crystals, at the
    tolerances of test_gpu_padded.py::test_padded_training_step_matches_oracle_autograd (5e-4, 1e-4, 3e-3, 1e-4).  Measured
    on one MI355X, largest error over largest reference magnitude: forward 5.6e-7, loss 7.3e-8, worst parameter gradient
    1.7e-6, worst running statistic 1.3e-7 (the same for K = 1 and K = 3)."""
    from matten_amd.graphs import selected_mean_loss

    B = 10
    ref, model = build_pair(dict(ATOMIC), fixture_dataset_hparams(), randomize_bn=True, atomic=True)
    ref.train()
    model.train()
    out_r, loss_r, grads_r = _oracle_step(ref, compact, B)
    n = out_r.shape[0]

    _, n_plan, e = store.host.plan(list(range(B)))
    assert n_plan == n
    batch = store.batch(list(range(B)), pad_to=(_round_up(n + k, 32), _round_up(e, 1024), B + k))
    assert batch["pos"].shape[0] >= n + k and batch["edge_index"].shape[1] > e
    loss_fn = selected_mean_loss("mse", key=TARGET)
    preds, _ = model(dict(batch), task_name=TARGET)
    out_m = preds[TARGET]
    loss_m = loss_fn(preds, batch[TARGET], batch)
    model.zero_grad()
    loss_m.backward()
    assert out_m.shape == (batch["pos"].shape[0], 6) and torch.isfinite(out_m).all()   # padding atoms stay finite
    _compare_step(ref, model, out_m[:n], loss_m, out_r, loss_r, grads_r, (5e-4, 1e-4, 3e-3, 1e-4))


# ----------------------------------------------------------------------------------------------------------------------
# 3. shared_step: the dense batch against the compact one
# ----------------------------------------------------------------------------------------------------------------------
def test_shared_step_on_a_dense_batch_is_the_compact_one(dense, compact):
    from matten_amd.data.graph import collate

    _, model = build_pair(dict(ATOMIC), fixture_dataset_hparams(), randomize_bn=True, atomic=True)
    idx = [0, 5, 9, 11, 3]
    state = {}
    with torch.no_grad():
        for name, graphs in (("dense", dense), ("compact", compact)):
            batch = collate([graphs[i] for i in idx], device=DEV)
            loss, preds, labels = model.shared_step(batch, "val")
            model.update_metrics(preds, labels, "val")
            metric = model.metrics["metric_val"][TARGET]["MeanAbsoluteError"]
            state[name] = (loss.double().cpu(), metric.sum_abs.clone().cpu(), metric.count.clone().cpu(), preds[TARGET].shape[0])
            score = model.compute_metrics("val", log=False)[1]
            state[name] += (score.double().cpu(),)
    d, c = state["dense"], state["compact"]
    m = sum(SELECTED[i] for i in idx)
    assert d[3] == sum(g["pos"].shape[0] for g in (dense[i] for i in idx)) and c[3] == m    # no indexing on the dense route
    print(f"loss dense {float(d[0]):.9e} compact {float(c[0]):.9e}; sum_abs dense {float(d[1]):.17e} compact {float(c[1]):.17e}")
    assert abs(float(d[0]) - float(c[0])) <= 2e-6 * abs(float(c[0]))
    assert float(d[2]) == float(c[2]) == 6.0 * m
    assert abs(float(d[1]) - float(c[1])) <= 1e-12 * abs(float(c[1]))
    assert abs(float(d[4]) - float(c[4])) <= 1e-6 * abs(float(c[4])) and float(d[4]) > 0


def test_shared_step_l1_loss_and_gradients_on_the_dense_route(dense, compact):
    """an L1Loss task takes kind 1; the gradients of the dense route are those of the compact one"""
    from matten_amd.data.graph import collate

    _, model = build_pair(dict(ATOMIC), fixture_dataset_hparams(), randomize_bn=True, atomic=True)
    model.loss_fns[TARGET] = torch.nn.L1Loss()
    idx = [1, 2, 7]
    grads = {}
    for name, graphs in (("dense", dense), ("compact", compact)):
        loss, _, _ = model.shared_step(collate([graphs[i] for i in idx], device=DEV), "train")
        model.zero_grad()
        loss.backward()
        grads[name] = (loss.detach(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
    assert abs(float(grads["dense"][0]) - float(grads["compact"][0])) <= 2e-6 * abs(float(grads["compact"][0]))
    assert set(grads["dense"][1]) == set(grads["compact"][1])
    for n, g in grads["compact"][1].items():
        _close(grads["dense"][1][n], g, 1e-4, f"grad {n} (dense against compact)")


# ----------------------------------------------------------------------------------------------------------------------
# 4. two epochs of bucketed, captured steps
# ----------------------------------------------------------------------------------------------------------------------
def _model(ds, state=None):
    from matten_amd.model_factory.tfn_atomic_tensor import AtomicTensorModel

    torch.manual_seed(35)
    m = AtomicTensorModel(tasks=TARGET, backbone_hparams=copy.deepcopy(ATOMIC), dataset_hparams=ds)
    if state is not None:
        m.load_state_dict(state)
    return m.to(DEV)


def test_bucketed_epochs_follow_the_eager_steps(store, compact):
    """12 crystals, batch_size 5 (two full batches and one of 2: K = 4), quanta (32, 1024), two epochs: six steps in two
    buckets, (64, 2048, 6) four times and (32, 1024, 6) twice"""
    from matten_amd.dataset.structure_scalar_tensor import _DeviceLoader, _Loader
    from matten_amd.graphs import BucketedTrainStep, selected_mean_loss
    from matten_amd.optim import FlatAdam

    ds = fixture_dataset_hparams()
    state = copy.deepcopy(_model(ds).state_dict())
    kw = dict(batch_size=5, shuffle=True, seed=3)
    dense_loss = selected_mean_loss("mse", key=TARGET)

    def fresh():
        model = _model(ds, state).train()
        return model, FlatAdam(model.parameters(), lr=1e-2, weight_decay=1e-5, device_lr=True)

    def eager(loader, loss_of):
        model, opt = fresh()
        losses = []
        for _ in range(2):
            for batch in loader:
                loss = loss_of(model(dict(batch), task_name=TARGET)[0], batch)
                opt.zero_grad()
                loss.backward()
                opt.step()
                losses.append(float(loss.detach()))
        return losses, [p.detach().clone() for p in model.parameters()]

    model, opt = fresh()
    step = BucketedTrainStep(model, opt, dense_loss, max_graphs=8, warmup=2, task_name=TARGET)
    got, buckets = [], []
    loader = _DeviceLoader(store, pad=(32, 1024), training=True, **kw)
    for _ in range(2):
        for batch in loader:
            buckets.append(step.bucket(batch))
            got.append(float(step.step(batch, batch[TARGET]).detach()))
    p_got = [p.detach().clone() for p in model.parameters()]

    want, _ = eager(_DeviceLoader(store, pad=(32, 1024), training=True, **kw), lambda preds, b: dense_loss(preds, b[TARGET], b))
    print(f"buckets {buckets}\neager on the padded batches {want}\nbucketed {got}")
    print(f"captures {step.captures}, replays {step.replays}, eager steps {step.eager_steps}")
    assert sorted(buckets) == [(32, 1024, 6)] * 2 + [(64, 2048, 6)] * 4
    assert step.captures == 2 and step.replays == 4 and step.eager_steps == 0
    assert len(want) == len(got) == 6 and want[0] != want[-1]
    assert got == want, "the same kernels on the same shapes"

    plain, p_plain = eager(_Loader(compact, device=DEV, **kw),
                           lambda preds, b: torch.nn.functional.mse_loss(preds[TARGET][b["atom_selector"]], b[TARGET]))
    for i, (a, b) in enumerate(zip(got, plain)):
        _close(torch.tensor(a), torch.tensor(b), 2e-3, f"loss at step {i} against the unpadded compact eager step")
    for i, (a, b) in enumerate(zip(p_got, p_plain)):
        _close(a, b, 5e-3, f"parameter {i} after two epochs against the unpadded compact eager run")


# ----------------------------------------------------------------------------------------------------------------------
# 5. Trainer.fit on a device-resident data module
# ----------------------------------------------------------------------------------------------------------------------
def test_trainer_fits_the_atomic_model_on_a_device_resident_module():
    from matten_amd.data.graph import collate
    from matten_amd.model.trainer import Trainer
    from matten_amd.model_factory.tfn_atomic_tensor import AtomicTensorModel

    dm = data_module(device_resident=True, device=DEV, loader_kwargs=dict(batch_size=2, shuffle=True), **SCALE)
    assert dm.files == {"train": FIXTURE, "val": FIXTURE, "test": FIXTURE} and dm.atom_target_layout == "dense"
    dm.setup()
    info = dm.get_to_model_info()
    torch.manual_seed(35)
    model = AtomicTensorModel(
        tasks=TARGET, backbone_hparams=copy.deepcopy(ATOMIC),
        dataset_hparams={"allowed_species": list(info["allowed_species"]), "average_num_neighbors": info["average_num_neighbors"]},
        optimizer_hparams={"class_path": "matten_amd.optim.FlatAdam", "init_args": {"lr": 1e-2, "weight_decay": 1e-5}},
        lr_scheduler_hparams=None).to(DEV)
    before = [p.detach().clone() for p in model.parameters()]
    trainer = Trainer(max_epochs=1).fit(model, datamodule=dm)
    score = trainer.history[0]["val/score"]
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))   # it trained
    assert score == score and abs(score) != float("inf")

    # the masked mean absolute error by hand, from predict-style forwards of the trained model
    model.eval()
    total, count = 0.0, 0
    with torch.no_grad():
        for g in dm.train_data:
            out = model(collate([g], device=DEV), task_name=TARGET)[0][TARGET].cpu().double()
            sel = g["atom_selector"] != 0
            total += float((out[sel] - g[TARGET][sel].double()).abs().sum())
            count += int(sel.sum()) * 6
    assert count == 120
    print(f"val/score {score:.9e}, by hand {total / count:.9e}")
    assert abs(score - total / count) <= 1e-5 * (total / count)
