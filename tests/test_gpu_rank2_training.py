"""Fine-tuning a per-atom tensor model on derived scalars (isotropic shielding, span) on the GPU: one padded dense training
step through ``rank2_selected_loss`` against the oracle's autograd through ``torch.linalg.eigvalsh`` in fp64, three
shuffled epochs of bucketed captured steps against the same steps run eagerly, and ``predict(..., shielding=True)``.
Everything reads tests/golden/si_nmr_n12.json; the scalar targets are derived from its own tensors (scaled by 0.01 like
the tensor targets) and travel as ordinary per-node keys of the device store."""
import copy

import numpy as np
import pytest
import torch

from common import ATOMIC, build_pair
from test_atom_targets_host import FIXTURE, SELECTED, TARGET, fixture_dataset_hparams, fixture_graphs
from test_gpu_atom_training import CORE, SCALE, _close, _compare_step, _model, _round_up

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ISO, ISO_SPAN = "iso_target", "iso_span_target"


def _basis64():
    from matten_amd.rank2 import rank2_basis

    return torch.from_numpy(rank2_basis("ij=ji").copy())


@pytest.fixture(scope="module")
def dense():
    """the fixture's dense graphs, each with two more per-node keys: ISO [n,1] and ISO_SPAN [n,2] fp32, the isotropic value
    and the span of the atom's own (scaled) label tensor, zeros where the atom carries none"""
    from matten_amd.rank2 import rank2_host

    out = []
    for g in fixture_graphs("dense", **SCALE):
        h = rank2_host((g[TARGET].double() @ _basis64()).reshape(-1, 3, 3))
        cols = torch.from_numpy(np.stack([h["iso"], h["span"]], axis=1)).float()
        cols[g["atom_selector"] == 0] = 0.0
        out.append(dict(g, **{ISO: cols[:, :1].contiguous(), ISO_SPAN: cols.contiguous()}))
    return out


@pytest.fixture(scope="module")
def store(dense):
    from matten_amd.data.store import DeviceGraphStore

    return DeviceGraphStore.from_graphs(dense, DEV)


def _scalars_torch(out):
    """iso and span of the oracle's irreps rows [N,6]: to_cartesian, then eigvalsh in fp64 (differentiable)"""
    T = (out.double() @ _basis64()).reshape(-1, 3, 3)
    lam = torch.linalg.eigvalsh(0.5 * (T + T.transpose(1, 2)))
    return lam.sum(1) / 3.0, lam[:, 2] - lam[:, 0]


def _oracle_step(ref, dense, n_crystals, names, kind):
    from matten_amd.data.graph import collate

    cpu = collate(dense[:n_crystals])
    sel = cpu["atom_selector"] != 0
    out = ref.decode({k: cpu[k] for k in CORE})
    iso, span = _scalars_torch(out)
    pred = torch.stack([iso, span], dim=1)[:, : len(names)][sel]
    diff = pred - cpu[ISO_SPAN].double()[:, : len(names)][sel]
    loss = (diff * diff).mean() if kind == "mse" else diff.abs().mean()
    ref.zero_grad()
    loss.backward()
    return out, loss, {name: p.grad.clone() for name, p in ref.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("names,kind,key", [(("iso",), "mse", ISO), (("iso", "span"), "l1", ISO_SPAN)])
def test_padded_dense_step_on_scalars_matches_oracle_autograd(store, dense, names, kind, key):
    """The device side runs the store's padded dense batch (quanta (32, 1024), one padding crystal) through
    rank2_selected_loss; the oracle takes its own [N,6] rows through to_cartesian and the torch-fp64 restatement
    (eigvalsh) and averages over the selected atoms.  Bounds (5e-4, 1e-4, 3e-3, 1e-4) of
    test_gpu_atom_training.py::test_padded_dense_training_step_matches_oracle_autograd, same measure.  Measured on one
    MI355X, largest error over largest reference magnitude -- ("iso",) mse: forward 5.6e-7, loss 5.8e-8, worst parameter
    gradient 1.7e-6, worst running statistic 1.3e-7; ("iso", "span") l1: forward 5.6e-7, loss 4.6e-8, worst parameter
    gradient 1.5e-6, worst running statistic 1.3e-7."""
    from matten_amd.graphs import rank2_selected_loss

    B, k = 10, 1
    ref, model = build_pair(dict(ATOMIC), fixture_dataset_hparams(), randomize_bn=True, atomic=True)
    ref.train()
    model.train()
    out_r, loss_r, grads_r = _oracle_step(ref, dense, B, names, kind)
    n = out_r.shape[0]
    _, n_plan, e = store.host.plan(list(range(B)))
    assert n_plan == n
    batch = store.batch(list(range(B)), pad_to=(_round_up(n + k, 32), _round_up(e, 1024), B + k))
    assert batch[key].shape == (batch["pos"].shape[0], len(names)) and batch[key].dtype == torch.float32
    assert not batch[key][n:].any() and not batch["atom_selector"][n:].any()          # padding rows: zero, unselected
    assert int(batch["atom_selector"].sum()) == sum(SELECTED[:B])
    loss_fn = rank2_selected_loss(names, kind, key=TARGET)
    preds, _ = model(dict(batch), task_name=TARGET)
    loss_m = loss_fn(preds, batch[key], batch)
    model.zero_grad()
    loss_m.backward()
    assert loss_m.dtype == torch.float32 and loss_m.dim() == 0
    _compare_step(ref, model, preds[TARGET][:n], loss_m, out_r, loss_r, grads_r, (5e-4, 1e-4, 3e-3, 1e-4))
    # the same loss from a dict of targets
    as_dict = loss_fn(preds, {name: batch[key][:, q] for q, name in enumerate(names)}, batch)
    assert torch.equal(as_dict.detach(), loss_m.detach())


def test_bucketed_epochs_on_isotropic_targets_follow_the_eager_steps(store):
    """12 crystals, batch_size 5, quanta (16, 1024), three shuffled epochs: nine steps, every one captured or replayed; the
    same steps run eagerly on the same padded batches give the same losses and parameters bit for bit, and on the plain
    (unpadded) batches of the device loader the same within the bounds of
    test_gpu_atom_training.py::test_bucketed_epochs_follow_the_eager_steps (2e-3 per loss, 5e-3 per parameter)."""
    from matten_amd.dataset.structure_scalar_tensor import _DeviceLoader
    from matten_amd.graphs import BucketedTrainStep, rank2_selected_loss
    from matten_amd.optim import FlatAdam

    ds = fixture_dataset_hparams()
    state = copy.deepcopy(_model(ds).state_dict())
    kw = dict(batch_size=5, shuffle=True, seed=3)
    loss_fn = rank2_selected_loss(("iso",), "mse", key=TARGET)
    epochs = 3

    def fresh():
        model = _model(ds, state).train()
        return model, FlatAdam(model.parameters(), lr=1e-2, weight_decay=1e-5, device_lr=True)

    def eager(loader):
        model, opt = fresh()
        losses = []
        for _ in range(epochs):
            for batch in loader:
                loss = loss_fn(model(dict(batch), task_name=TARGET)[0], batch[ISO], batch)
                opt.zero_grad()
                loss.backward()
                opt.step()
                losses.append(float(loss.detach()))
        return losses, [p.detach().clone() for p in model.parameters()]

    model, opt = fresh()
    step = BucketedTrainStep(model, opt, loss_fn, max_graphs=8, warmup=2, task_name=TARGET)
    got, buckets = [], []
    loader = _DeviceLoader(store, pad=(16, 1024), training=True, **kw)
    for _ in range(epochs):
        for batch in loader:
            buckets.append(step.bucket(batch))
            got.append(float(step.step(batch, batch[ISO]).detach()))
    p_got = [p.detach().clone() for p in model.parameters()]

    want, p_want = eager(_DeviceLoader(store, pad=(16, 1024), training=True, **kw))
    print(f"buckets {buckets}\neager on the padded batches {want}\nbucketed {got}")
    print(f"captures {step.captures}, replays {step.replays}, eager steps {step.eager_steps}")
    assert len(got) == len(want) == 3 * epochs and want[0] != want[-1] and all(np.isfinite(got))
    assert step.captures + step.replays + step.eager_steps == len(got) and step.replays >= 1
    assert step.captures == len(set(buckets)) and step.eager_steps == 0
    assert got == want, "the same kernels on the same shapes"
    for a, b in zip(p_got, p_want):
        assert torch.equal(a, b)

    plain, p_plain = eager(_DeviceLoader(store, training=True, **kw))
    for i, (a, b) in enumerate(zip(got, plain)):
        _close(torch.tensor(a), torch.tensor(b), 2e-3, f"loss at step {i} against the unpadded eager step")
    for i, (a, b) in enumerate(zip(p_got, p_plain)):
        _close(a, b, 5e-3, f"parameter {i} after three epochs against the unpadded eager run")


def test_predict_returns_shielding_parameters_of_all_atoms():
    from matten_amd import predict as P
    from matten_amd.data.io import structures_from_json
    from matten_amd.rank2 import Rank2Properties, rank2_properties

    structs = structures_from_json(FIXTURE, target_columns=())
    _, model = build_pair(dict(ATOMIC), fixture_dataset_hparams(), randomize_bn=True, atomic=True)
    cfg = {"data": {"r_cut": 5.0, "tensor_target_name": TARGET, "tensor_target_formula": "ij=ji"}}
    plain = P.predict(structs, model=model, config=cfg, is_atomic_tensor=True, batch_size=5)
    tensors, props = P.predict(structs, model=model, config=cfg, is_atomic_tensor=True, batch_size=5, shielding=True)
    counts = [len(s["atomic_numbers"]) for s in structs]
    assert len(tensors) == len(plain) == sum(counts) and isinstance(props, Rank2Properties)
    for a, b in zip(tensors, plain):
        assert isinstance(a, np.ndarray) and a.shape == (3, 3) and a.dtype == b.dtype and np.array_equal(a, b)
    assert props.ptr.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist() and props.ptr.dtype == torch.int64
    assert props.iso.shape == (sum(counts),) and props.iso.is_cuda and (props.flags == 0).all()
    again = rank2_properties(tensors)
    for k in ("principal_values", "principal_axes", "iso", "span", "skew", "zeta", "anisotropy", "eta", "flags", "is_isotropic"):
        a, b = getattr(props, k), getattr(again, k)
        assert a.shape == b.shape and torch.equal(a, b), k
    d = props.cpu().to_dict()
    assert d["ptr"].shape == (13,) and d["principal_axes"].shape == (sum(counts), 3, 3)
    # a single structure: still the flat list of its atoms
    t1, p1 = P.predict(structs[9], model=model, config=cfg, is_atomic_tensor=True, shielding=True)
    assert len(t1) == counts[9] and p1.ptr.tolist() == [0, counts[9]] and p1.iso.shape == (counts[9],)
