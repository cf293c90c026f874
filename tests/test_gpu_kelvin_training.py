"""
Fine-tuning against instability as hipGraph replays (``graphs.stability_penalized``), and ``predict(..., kelvin=True)``: the
LMAX2 model on the 100 crystals of the example data set, padded device batches of 8 crystals at quanta (16, 512).
"""
import copy
import os
import warnings

import numpy as np
import pytest
import torch

from common import LMAX2
from store_cases import TARGET, golden_graphs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WEIGHT = 0.1


def _species_hparams(graphs):
    from matten_amd.data.graph import average_num_neighbors

    species = sorted({int(z) for g in graphs for z in g["atomic_numbers"].tolist()})
    return {"allowed_species": species, "average_num_neighbors": average_num_neighbors(graphs)}


def _model(ds, state=None):
    from matten_amd.model_factory.tfn_scalar_tensor import ScalarTensorModel

    torch.manual_seed(35)
    m = ScalarTensorModel(backbone_hparams=copy.deepcopy(LMAX2), dataset_hparams=ds)
    if state is not None:
        m.load_state_dict(state)
    return m.to(DEV)


@pytest.fixture(scope="module")
def setting():
    """the store, the model's initial state, the padded batches of two epochs (cloned: the loader may reuse its buffers) and
    a margin at the median Kelvin modulus of the first batch's predictions"""
    from matten.data.store import DeviceGraphStore
    from matten.dataset.structure_scalar_tensor import _DeviceLoader
    from matten_amd import elastic

    graphs = list(golden_graphs())
    store = DeviceGraphStore.from_graphs(graphs, DEV)
    ds = _species_hparams(graphs)
    model = _model(ds)
    state = copy.deepcopy(model.state_dict())
    loader = _DeviceLoader(store, pad=(16, 512), batch_size=8, shuffle=True, seed=3, training=True)
    batches = [{k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in b.items()} for _ in range(2) for b in loader]
    assert len(batches) == 26 and all(b["ptr"].shape[0] == 10 for b in batches)      # (two epochs: 13 batches each)
    assert all(b["pos"].shape[0] % 16 == 0 and b["edge_index"].shape[1] % 512 == 0 for b in batches)
    with torch.no_grad():
        preds = model.eval()(dict(batches[0]), task_name=TARGET)[0][TARGET]
    n = int(batches[0]["_amd_n_valid"][2])
    lam = elastic.elastic_properties_from_irreps(preds[:n], kelvin=True).kelvin_moduli
    margin = float(lam.median())
    assert n >= 1 and bool((lam < margin).any()) and bool((lam > margin).any())      # active and inactive modes
    return dict(store=store, ds=ds, state=state, batches=batches, margin=margin)


def _fresh(setting):
    from matten_amd.optim import FlatAdam

    model = _model(setting["ds"], setting["state"]).train()
    return model, FlatAdam(model.parameters(), lr=1e-2, weight_decay=1e-5, device_lr=True)


def _loss(setting, kind="squared"):
    from matten_amd.graphs import stability_penalized, valid_mean_loss

    return stability_penalized(valid_mean_loss("mse", TARGET), WEIGHT, margin=setting["margin"], kind=kind, key=TARGET)


def test_graphed_step_equals_the_eager_loop(setting):
    """three batches of one bucket: the replayed losses and every parameter after the three steps equal the eager loop's,
    bit for bit; the penalty is part of the loss (it differs from the base loss alone) and moves the parameters"""
    from matten_amd.graphs import BucketedTrainStep, GraphedTrainStep, _train_step, valid_mean_loss

    by_bucket = {}
    for b in setting["batches"]:
        by_bucket.setdefault(BucketedTrainStep.bucket(b), []).append(b)
    same = max(by_bucket.values(), key=len)[:3]
    assert len(same) == 3, {k: len(v) for k, v in by_bucket.items()}
    loss_fn = _loss(setting)

    model, opt = _fresh(setting)
    want = [float(_train_step(model, opt, loss_fn, b, b[TARGET], TARGET).detach()) for b in same]
    p_want = [p.detach().clone() for p in model.parameters()]

    model, opt = _fresh(setting)
    step = GraphedTrainStep(model, opt, loss_fn, same[0], same[0][TARGET], warmup=2, task_name=TARGET)
    got = [float(step.step(b, b[TARGET]).detach()) for b in same]
    p_got = [p.detach().clone() for p in model.parameters()]
    print(f"eager {want}\nreplayed {got}")
    assert got == want and all(np.isfinite(got))
    assert all(torch.equal(a, b) for a, b in zip(p_got, p_want))

    model, opt = _fresh(setting)
    base = valid_mean_loss("mse", TARGET)
    plain = float(_train_step(model, opt, base, same[0], same[0][TARGET], TARGET).detach())
    assert want[0] > plain                                     # the first step sees the same weights: base + weight * penalty
    hinge = _loss(setting, "hinge")
    model, opt = _fresh(setting)
    assert float(_train_step(model, opt, hinge, same[0], same[0][TARGET], TARGET).detach()) > plain


def test_bucketed_epoch_runs_without_an_eager_step(setting):
    from matten_amd.graphs import BucketedTrainStep

    model, opt = _fresh(setting)
    step = BucketedTrainStep(model, opt, _loss(setting), max_graphs=16, warmup=2, task_name=TARGET)
    losses = [float(step.step(b, b[TARGET]).detach()) for b in setting["batches"][:13]]
    print(f"captures {step.captures}, replays {step.replays}, eager steps {step.eager_steps}; losses {losses}")
    assert step.eager_steps == 0 and step.captures + step.replays == 13 and step.captures == len(step.graphs)
    assert all(np.isfinite(losses))


def test_predict_with_kelvin(golden_dir):
    """predict(..., properties=True, kelvin=True) on 5 structures: the fields, their shapes, and the bits of
    ``elastic_properties(tensors, kelvin=True)`` on the returned tensors"""
    from matten_amd import elastic
    from matten_amd import predict as P
    from matten_amd.model_factory.tfn_scalar_tensor import ScalarTensorModel
    from oracle.matten_ref import data as rdata

    structs = rdata.structures_from_json(os.path.join(golden_dir, "example_crystal_elasticity_tensor_n100.json"))
    structs = sorted(structs, key=lambda s: len(s["atomic_numbers"]))[:5]
    structs = [{k: s[k] for k in ("lattice", "cart_coords", "atomic_numbers")} for s in structs]
    ds = {"allowed_species": list(range(1, 95)), "average_num_neighbors": 18.0}
    torch.manual_seed(35)
    model = ScalarTensorModel(backbone_hparams=dict(LMAX2), dataset_hparams=ds).to(DEV).eval()
    cfg = {"data": {"r_cut": 5.0, "tensor_target_name": TARGET, "tensor_target_formula": "ijkl=jikl=klij"}}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tensors, props = P.predict(structs, model=model, config=cfg, properties=True, kelvin=True)
        plain_tensors, plain = P.predict(structs, model=model, config=cfg, properties=True)
    assert len(tensors) == 5 and all(t is not None for t in tensors)
    assert props.kelvin_moduli.shape == (5, 6) and props.kelvin_vectors.shape == (5, 6, 6)
    assert props.kelvin_dilatation.shape == (5, 6) and props.stability_margin.shape == (5,) and props.kelvin_condition.shape == (5,)
    assert list(props._names) == list(plain._names) + list(elastic.KELVIN_NAMES)
    want = elastic.elastic_properties([np.asarray(t) for t in tensors], kelvin=True).to_dict()
    got, without = props.to_dict(), plain.to_dict()
    assert set(got) == set(want)
    for k in got:
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    for k in without:                                           # every field that was there is the same without the keyword
        assert np.array_equal(got[k], without[k], equal_nan=True), k
    assert np.isfinite(got["kelvin_moduli"]).all() and elastic.eigenstrains(props).shape == (5, 6, 3, 3)
    with pytest.raises(ValueError, match="kelvin.*properties=True"):
        P.predict(structs, model=model, config=cfg, kelvin=True)
    with pytest.raises(ValueError, match="is_atomic_tensor"):
        P.predict(structs, model=model, config=cfg, is_atomic_tensor=True, properties=True, kelvin=True)
