"""Device-resident training set on the GPU (matten_amd/data/store.py, matten_batch_gather): a store batch against
``collate`` / ``ops.csr_build`` / ``ensure_training_edge_tensors``, bit for bit; through the model, the optimiser, the
data module and a captured training step.  Integer arithmetic and copies: every comparison is exact."""
import copy
import shutil

import numpy as np
import pytest
import torch

from common import LMAX2
from store_cases import (GOLDEN, N100, TARGET, data_module, golden_graphs, index_lists, many_key_graphs, store_graphs,
                         streams_needed)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CSR_KEYS = ("_amd_perm", "_amd_rowptr", "_amd_src_sorted")
TRAIN_KEYS = ("_amd_dst_sorted", "_amd_out_ptr", "_amd_out_perm")


@pytest.fixture(scope="module")
def store():
    from matten.data.store import DeviceGraphStore

    s = DeviceGraphStore.from_graphs(store_graphs(), DEV)
    assert len(s) == 103 and s.nbytes > 0
    return s


@pytest.fixture(scope="module")
def golden_store():
    from matten.data.store import DeviceGraphStore

    return DeviceGraphStore.from_graphs(golden_graphs(), DEV)


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert got.device == want.device and got.is_contiguous(), what
    assert torch.equal(got, want), what


def _check(store, graphs, idx, training=True):
    from matten_amd import ops
    from matten_amd.data.graph import collate
    from matten_amd.nn._nequip import ensure_training_edge_tensors

    got = store.batch(idx, training=training)
    want = collate([graphs[i] for i in idx], device=DEV)
    extra = CSR_KEYS + (TRAIN_KEYS if training else ())
    assert list(got.keys()) == list(want.keys()) + list(extra)
    for k, v in want.items():
        _same(got[k], v, k)
    perm, rowptr, src, _ = ops.csr_build(want["edge_index"], want["pos"].shape[0])
    for k, v in zip(CSR_KEYS, (perm, rowptr, src)):
        _same(got[k], v, k)
    if training:
        ref = ensure_training_edge_tensors(dict(want))
        out_ptr, out_perm = ref["_amd_out_csr"]
        for k, v in zip(TRAIN_KEYS, (ref["_amd_dst_sorted"], out_ptr, out_perm)):
            _same(got[k], v, k)
        # and the additive branch: a store batch gets its tuple from the two tensor keys, nothing is rebuilt
        mine = ensure_training_edge_tensors(dict(got))
        assert mine["_amd_out_csr"][0] is got["_amd_out_ptr"] and mine["_amd_out_csr"][1] is got["_amd_out_perm"]
        assert mine["_amd_dst_sorted"] is got["_amd_dst_sorted"]
    return got


@pytest.mark.parametrize("name", list(index_lists()))
def test_batch_is_collate_plus_csr(store, name):
    idx = index_lists()[name]
    _check(store, store_graphs(), idx, training=True)
    _check(store, store_graphs(), idx, training=False)


def test_one_atom_crystal_rowptr(store):
    got = store.batch([100], training=False)
    e = store_graphs()[100]["edge_index"].shape[1]
    assert got["_amd_rowptr"].tolist() == [0, e] and got["ptr"].tolist() == [0, 1]


def test_table_in_lds_and_beyond(store):
    """B + 1 <= matten_batch_gather_lds_rows(): the running sums are searched in LDS; above: in global memory.  Both
    sides of the threshold, and 5000 picks (with repeats) of the golden crystals far beyond it."""
    from matten_amd import _lib

    cap = _lib.load().matten_batch_gather_lds_rows()
    n_far = max(5000, 2 * cap)
    assert n_far + 1 > cap
    g = torch.Generator().manual_seed(5)
    for b in (cap - 1, cap, n_far):
        idx = torch.randint(0, 100, (b,), generator=g).tolist()
        _check(store, store_graphs(), idx, training=True)


def test_extra_keys():
    """a per-crystal [1,21] f32 target (every graph has it), a per-node [n,9] f32 target and a per-edge int64 key; plus
    rows of 16 and 8 bytes, which take the wide copies"""
    from matten.data.store import CRYSTAL, EDGE, NODE, DeviceGraphStore

    rng = torch.Generator().manual_seed(3)
    graphs = []
    for g in store_graphs()[88:]:
        n, e = g["pos"].shape[0], g["edge_index"].shape[1]
        graphs.append(dict(
            g,
            node_tensor=torch.randn(n, 9, generator=rng),
            edge_tag=torch.randint(-2 ** 40, 2 ** 40, (e,), generator=rng),
            node_quad=torch.randn(n, 4, generator=rng),
            crystal_pair=torch.randn(1, 2, generator=rng, dtype=torch.float64),
            edge_pair=torch.randint(0, 99, (e, 2), generator=rng, dtype=torch.int32),
        ))
    s = DeviceGraphStore.from_graphs(graphs, DEV)
    want_cls = {TARGET: CRYSTAL, "node_tensor": NODE, "edge_tag": EDGE, "node_quad": NODE, "crystal_pair": CRYSTAL, "edge_pair": EDGE}
    assert {k: s.host.classes[k] for k in want_cls} == want_cls
    for idx in ([14], [13, 0, 12, 14, 5, 5], list(range(14, -1, -1))):
        got = _check(s, graphs, idx)
        assert got[TARGET].shape == (len(idx), 21) and got["node_tensor"].shape[1:] == (9,) and got["edge_tag"].dtype == torch.int64


def test_more_streams_than_one_launch_takes():
    """18 extra keys: a training batch is 34 streams, two launches; the last streams, a row pointer with its closing
    entry among them, go with the second"""
    from matten.data.store import DeviceGraphStore
    from matten_amd import _lib

    graphs = many_key_graphs()
    s = DeviceGraphStore.from_graphs(graphs, DEV)
    cap = _lib.load().matten_batch_gather_max_streams()
    assert cap < streams_needed(s.host) <= 2 * cap
    for idx in ([14], [13, 0, 12, 14, 5, 5]):
        _check(s, graphs, idx)


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


def _loss(preds, target):
    return torch.nn.functional.mse_loss(preds[TARGET], target)


def test_eval_forward_on_a_store_batch(store):
    from matten_amd.data.graph import collate

    graphs = store_graphs()
    model = _model(_species_hparams(graphs)).eval()
    for idx in (index_lists()["cluster between tiny"], index_lists()["shuffled 32"]):
        with torch.no_grad():
            want = model(collate([graphs[i] for i in idx], device=DEV))[0][TARGET]
            got = model(store.batch(idx, training=False))[0][TARGET]
        assert want.shape == (len(idx), 21) and torch.isfinite(want).all()
        _same(got, want, "eval forward")


def test_three_flat_adam_steps_fed_by_the_device_loader(golden_store):
    """the same seed, the same crystals, the same bits: every parameter after three eager FlatAdam steps equals the run
    fed by _Loader (whose own reproducibility, MATTEN_TP_BWD_DX=ordered, is asserted first)"""
    from matten.dataset.structure_scalar_tensor import _DeviceLoader, _Loader
    from matten_amd.optim import FlatAdam

    graphs = list(golden_graphs())
    ds = _species_hparams(graphs)
    state = copy.deepcopy(_model(ds).state_dict())
    kw = dict(batch_size=32, shuffle=True, seed=3)

    def run(loader):
        model = _model(ds, state).train()
        opt = FlatAdam(model.parameters(), lr=1e-2, weight_decay=1e-5)
        losses = []
        for step, batch in enumerate(loader):
            if step == 3:
                break
            loss = _loss(model(dict(batch))[0], batch[TARGET])
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        return losses, [p.detach().clone() for p in model.parameters()]

    la, pa = run(_Loader(graphs, device=DEV, **kw))
    lb, pb = run(_Loader(graphs, device=DEV, **kw))
    spread = max(float((a - b).abs().max()) for a, b in zip(pa, pb))
    print(f"two _Loader runs: losses {la} / {lb}, largest parameter difference {spread:.3e}")
    assert la == lb and all(torch.equal(a, b) for a, b in zip(pa, pb)), "the premise: two _Loader runs agree bit for bit"
    lc, pc = run(_DeviceLoader(golden_store, training=True, **kw))
    diff = max(float((a - c).abs().max()) for a, c in zip(pa, pc))
    print(f"device loader run: losses {lc}, largest parameter difference to the _Loader run {diff:.3e}")
    assert lc == la and len(la) == 3 and la[0] != la[2]
    for a, c in zip(pa, pc):
        assert torch.equal(a, c)


def test_data_module_device_resident(tmp_path):
    shutil.copy(f"{GOLDEN}/{N100}", tmp_path / N100)
    kw = dict(root=str(tmp_path), device=DEV, loader_kwargs={"batch_size": 32, "shuffle": True, "seed": 3})
    plain, resident = data_module(**kw), data_module(device_resident=True, **kw)
    for dm in (plain, resident):
        dm.prepare_data()
        dm.setup()
    assert resident.get_to_model_info() == plain.get_to_model_info()
    assert len({id(s) for s in resident._stores.values()}) == 1   # one store per distinct file
    lp, lr = plain.train_dataloader(), resident.train_dataloader()
    assert len(lp) == len(lr) == 4
    for _ in range(2):
        n = 0
        for want, got in zip(lp, lr):
            assert list(got.keys()) == list(want.keys()) + list(CSR_KEYS + TRAIN_KEYS)
            for k, v in want.items():
                _same(got[k], v, k)
            n += 1
        assert n == 4 and want["ptr"].shape[0] == 5
    for a, b in ((plain.val_dataloader(), resident.val_dataloader()), (plain.test_dataloader(), resident.test_dataloader())):
        first_want, first_got = next(iter(a)), next(iter(b))
        assert list(first_got.keys()) == list(first_want.keys()) + list(CSR_KEYS)
        for k, v in first_want.items():
            _same(first_got[k], v, k)
        assert torch.equal(first_want[TARGET], torch.cat([g[TARGET] for g in plain.train_data[:32]]).to(DEV))   # unshuffled


def test_store_batch_under_a_captured_step(golden_store):
    """Capture on one store batch, replay same-shaped batches (the same crystals permuted).  The source-keyed CSR is read
    by the BACKWARD, so it shows in the loss of the step after: a CSR that stayed the construction batch's would sum
    dL/dx over the wrong edges.  Three replays against three eager steps on the same batches."""
    from matten_amd.graphs import GraphedTrainStep
    from matten_amd.optim import FlatAdam

    ds = _species_hparams(list(golden_graphs()))
    state = copy.deepcopy(_model(ds).state_dict())
    idx = list(range(40, 56))
    perm = torch.randperm(len(idx), generator=torch.Generator().manual_seed(2)).tolist()
    first, second = golden_store.batch(idx), golden_store.batch([idx[p] for p in perm])
    assert first["pos"].shape == second["pos"].shape and not torch.equal(first["_amd_out_perm"], second["_amd_out_perm"])
    order = (second, first, second)

    eager = _model(ds, state).train()
    opt_e = FlatAdam(eager.parameters(), lr=1e-2, weight_decay=1e-5)
    want = []
    for b in order:
        loss = _loss(eager(dict(b))[0], b[TARGET])
        opt_e.zero_grad()
        loss.backward()
        opt_e.step()
        want.append(float(loss.detach()))

    graphed = _model(ds, state).train()
    opt_g = FlatAdam(graphed.parameters(), lr=1e-2, weight_decay=1e-5)
    step = GraphedTrainStep(graphed, opt_g, _loss, first, first[TARGET], warmup=2, task_name=TARGET)
    assert "_amd_out_csr" not in step._static   # only tensors travel in a store batch
    got = [float(step.step(b, b[TARGET]).detach()) for b in order]
    print(f"eager losses {want}, replayed {got}")
    assert got == want and want[0] != want[2]
