"""
CPU tests of the per-atom target workflow (reference scripts/train_atomic_tensor.py, configs/atomic_tensor.yaml): the
reader's boolean columns, the two label layouts of ``TensorDataModule(atom_selector=...)`` over the twelve-crystal NMR
fixture, their classes in the host half of the device store, the refusals, the argument checks of the selected-loss
entries (no kernel is launched: every call returns from the checks) and the fp64 restatement of loss and adjoint that
the GPU tests compare the kernels with.
"""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "si_nmr_n12.json")
TARGET = "nmr_tensor"
ATOMS = [12, 12, 12, 12, 12, 12, 12, 12, 12, 6, 12, 9]
EDGES = [574, 452, 312, 376, 344, 506, 332, 376, 324, 144, 488, 330]
SELECTED = [4, 1, 2, 1, 1, 4, 1, 1, 2, 1, 1, 1]
OK, EINVAL, ENOMEM = 0, -1, -3


# ----------------------------------------------------------------------------------------------------------------------
# the definition: loss and adjoint over the selected rows in fp64 (shared with the GPU tests)
# ----------------------------------------------------------------------------------------------------------------------
def selected_loss_ref(pred, target, selector, kind):
    """-> (loss, sum, count): fp64 tensors and a python int; rows with selector == 0 are never touched"""
    n = pred.shape[0]
    p, t = pred.detach().cpu().double().reshape(n, -1), target.detach().cpu().double().reshape(n, -1)
    sel = selector.detach().cpu() != 0
    x = p[sel] - t[sel]
    total = (x * x if kind == 0 else x.abs()).sum()
    count, d = int(sel.sum()), p.shape[1]
    loss = total / (count * d) if count else torch.zeros((), dtype=torch.float64)
    return loss, total, count


def selected_loss_bwd_ref(pred, target, selector, kind, g=1.0):
    """-> d loss / d pred in fp64, shaped like pred: g * dl(pred - target) / (count * d) on selected rows, 0 elsewhere"""
    n = pred.shape[0]
    p, t = pred.detach().cpu().double().reshape(n, -1), target.detach().cpu().double().reshape(n, -1)
    sel = selector.detach().cpu() != 0
    grad = torch.zeros_like(p)
    count, d = int(sel.sum()), p.shape[1]
    if count:
        x = p[sel] - t[sel]
        grad[sel] = float(g) * (2.0 * x if kind == 0 else torch.sign(x)) / (count * d)
    return grad.reshape(pred.shape)


def data_module(layout=None, **kw):
    from matten_amd.dataset.structure_scalar_tensor import TensorDataModule

    args = dict(r_cut=5.0, tensor_target_name=TARGET, tensor_target_formula="ij=ji", atom_selector="atom_selector")
    if layout is not None:
        args["atom_target_layout"] = layout
    args.update(kw)
    return TensorDataModule(FIXTURE, FIXTURE, FIXTURE, **args)


_GRAPHS = {}


def fixture_graphs(layout, **kw):
    """the twelve crystal graphs of the fixture in one label layout (built once per layout and option set)"""
    key = (layout, tuple(sorted(kw.items())))
    if key not in _GRAPHS:
        dm = data_module(layout, **kw)
        dm.setup()
        _GRAPHS[key] = dm.train_data
    return _GRAPHS[key]


def fixture_dataset_hparams():
    from matten_amd.data.graph import average_num_neighbors

    graphs = fixture_graphs("compact")
    species = sorted({int(z) for g in graphs for z in g["atomic_numbers"].tolist()})
    return {"allowed_species": species, "average_num_neighbors": average_num_neighbors(graphs)}


# ----------------------------------------------------------------------------------------------------------------------
def test_restatement_is_the_reference_route():
    """mse_loss(pred[sel], compact_target) and its autograd gradient, the reference's model/model.py:340-345"""
    g = torch.Generator().manual_seed(0)
    pred = torch.randn(37, 6, generator=g, dtype=torch.float64, requires_grad=True)
    sel = torch.rand(37, generator=g) < 0.3
    compact = torch.randn(int(sel.sum()), 6, generator=g, dtype=torch.float64)
    dense = torch.zeros(37, 6, dtype=torch.float64)
    dense[sel] = compact
    for kind, fn in ((0, torch.nn.functional.mse_loss), (1, torch.nn.functional.l1_loss)):
        pred.grad = None
        want = fn(pred[sel], compact)
        want.backward()
        loss, total, count = selected_loss_ref(pred, dense, sel.to(torch.int32), kind)
        assert count == int(sel.sum())
        assert torch.allclose(loss, want.detach(), rtol=1e-14, atol=0)
        assert torch.allclose(total, want.detach() * count * 6, rtol=1e-14, atol=0)
        grad = selected_loss_bwd_ref(pred, dense, sel.to(torch.int32), kind)
        assert torch.allclose(grad, pred.grad, rtol=1e-14, atol=0) and (grad[~sel] == 0).all()
        half = selected_loss_bwd_ref(pred, dense, sel.to(torch.int32), kind, g=0.5)
        assert torch.equal(half, 0.5 * grad)
    nothing = torch.zeros(37, dtype=torch.int32)
    assert selected_loss_ref(pred, dense, nothing, 0) == (torch.zeros((), dtype=torch.float64), torch.zeros((), dtype=torch.float64), 0)
    assert (selected_loss_bwd_ref(pred, dense, nothing, 0) == 0).all()
    junk = pred.detach().clone()
    junk[~sel] = float("nan")
    assert torch.equal(selected_loss_ref(junk, dense, sel.to(torch.int32), 0)[0], selected_loss_ref(pred, dense, sel.to(torch.int32), 0)[0])


def test_reader_reads_boolean_columns_and_keeps_its_default_output():
    from matten_amd.data.io import structures_from_json

    plain = structures_from_json(FIXTURE, target_columns=(TARGET,))
    rows = structures_from_json(FIXTURE, target_columns=(TARGET,), bool_columns=("atom_selector",))
    assert len(plain) == len(rows) == 12
    for a, b, n, m in zip(plain, rows, ATOMS, SELECTED):
        assert "atom_selector" not in a and list(b.keys()) == list(a.keys()) + ["atom_selector"]
        for k in a:
            assert np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype, k
        assert b["atom_selector"].dtype == np.bool_ and b["atom_selector"].shape == (n,) and b["atom_selector"].sum() == m
        assert b[TARGET].shape == (m, 3, 3)
        assert set(b["atomic_numbers"][b["atom_selector"]].tolist()) == {14}   # every target sits on a silicon
    # a column that is absent is skipped like an absent target column; a column that holds no flags is an error
    assert "nope" not in structures_from_json(FIXTURE, bool_columns=("nope",))[0]
    with pytest.raises(ValueError, match="row 0"):
        structures_from_json(FIXTURE, target_columns=(), bool_columns=(TARGET,))


def test_fixture_is_the_issue_table():
    graphs = fixture_graphs("compact")
    assert [g["pos"].shape[0] for g in graphs] == ATOMS and sum(ATOMS) == 135
    assert [g["edge_index"].shape[1] for g in graphs] == EDGES and sum(EDGES) == 4558
    assert [int(g["atom_selector"].sum()) for g in graphs] == SELECTED and sum(SELECTED) == 20
    assert fixture_dataset_hparams()["allowed_species"] == [8, 14]
    table = json.load(open(FIXTURE))
    assert sorted(table) == ["atom_selector", "nmr_tensor", "structure"]
    assert all(sorted(col, key=int) == [str(i) for i in range(12)] for col in table.values())
    assert os.path.getsize(FIXTURE) < 64 * 1024
    t = np.asarray([m for r in table[TARGET].values() for m in r])
    assert np.abs(t - t.transpose(0, 2, 1)).max() > 1.0   # the shielding tensors are NOT symmetric: they are projected


def test_compact_layout_is_the_references():
    from matten_amd.data.graph import collate
    from matten_amd.data.io import structures_from_json
    from matten_amd.utils import CartesianTensorWrapper

    dm = data_module(loader_kwargs=dict(batch_size=5))
    assert dm.atom_target_layout == "compact"     # the host loader's default
    dm.setup()
    graphs = dm.train_data
    rows = structures_from_json(FIXTURE, target_columns=(TARGET,), bool_columns=("atom_selector",))
    conv = CartesianTensorWrapper("ij=ji")
    for g, r, n, m in zip(graphs, rows, ATOMS, SELECTED):
        assert g[TARGET].shape == (m, 6) and g[TARGET].dtype == torch.float32
        assert g["atom_selector"].shape == (n,) and g["atom_selector"].dtype == torch.bool
        assert torch.equal(g["atom_selector"], torch.from_numpy(r["atom_selector"]))
        want = conv.from_cartesian(torch.as_tensor(r[TARGET], dtype=torch.float64)).to(torch.float32)
        assert torch.equal(g[TARGET], want)
    batches = list(dm.train_dataloader())
    assert [b["ptr"].shape[0] - 1 for b in batches] == [5, 5, 2]
    for i, b in enumerate(batches):
        hand = collate(graphs[5 * i:5 * i + 5])
        assert list(b.keys()) == list(hand.keys())
        assert all(torch.equal(b[k], hand[k]) and b[k].dtype == hand[k].dtype for k in hand)
        assert b[TARGET].shape[0] == int(b["atom_selector"].sum())
    assert sum(b[TARGET].shape[0] for b in batches) == 20
    selector = torch.cat([b["atom_selector"] for b in batches])
    assert selector.dtype == torch.bool and selector.shape == (135,)


def test_the_references_atomic_data_block_builds_its_data_module():
    """the `data:` block of the reference's scripts/configs/atomic_tensor.yaml, with the fixture as its three files"""
    from matten.dataset.structure_scalar_tensor import TensorDataModule

    name = os.path.basename(FIXTURE)
    block = dict(tensor_target_name="nmr_tensor", atom_selector="atom_selector", tensor_target_formula="ij=ji",
                 root=os.path.dirname(FIXTURE), trainset_filename=name, valset_filename=name, testset_filename=name, r_cut=5.0,
                 reuse=False, loader_kwargs=dict(batch_size=2, shuffle=True))
    dm = TensorDataModule(**block)
    dm.setup()
    batches = list(dm.train_dataloader())
    assert len(batches) == 6 and sum(int(b["atom_selector"].sum()) for b in batches) == 20
    assert all(b["atom_selector"].dtype == torch.bool and b[TARGET].shape[0] == int(b["atom_selector"].sum()) for b in batches)
    assert dm.get_to_model_info()["allowed_species"] == (8, 14)


@pytest.mark.parametrize("fmt,scale", [("irreps", 1.0), ("irreps", 0.01), ("cartesian", 1.0)])
def test_dense_layout_holds_the_compact_rows(fmt, scale):
    kw = dict(tensor_target_format=fmt, tensor_target_scale=scale)
    compact, dense = fixture_graphs("compact", **kw), fixture_graphs("dense", **kw)
    row = (6,) if fmt == "irreps" else (3, 3)
    for c, d, n in zip(compact, dense, ATOMS):
        assert list(c.keys()) == list(d.keys())
        assert d[TARGET].shape == (n,) + row and d[TARGET].dtype == torch.float32
        assert d["atom_selector"].shape == (n,) and d["atom_selector"].dtype == torch.int32
        assert torch.equal(d["atom_selector"] != 0, c["atom_selector"]) and set(d["atom_selector"].tolist()) <= {0, 1}
        assert torch.equal(d[TARGET][d["atom_selector"] != 0], c[TARGET])          # bit for bit
        assert (d[TARGET][d["atom_selector"] == 0] == 0).all()
        for k in c:
            if k not in (TARGET, "atom_selector"):
                assert torch.equal(c[k], d[k]), k
    if scale != 1.0:
        full = fixture_graphs("compact", tensor_target_format=fmt)
        assert torch.allclose(compact[0][TARGET], full[0][TARGET] * scale, rtol=1e-6, atol=0)


def test_host_store_takes_the_dense_keys_as_node_keys():
    from matten_amd.data.store import NODE, GraphStoreHost

    dense = fixture_graphs("dense")
    host = GraphStoreHost(dense)
    assert host.classes[TARGET] == NODE and host.classes["atom_selector"] == NODE
    idx = [9, 2, 11, 0]
    n, e = sum(ATOMS[i] for i in idx), sum(EDGES[i] for i in idx)
    for k in (1, 3):
        ref = host.padded_reference(idx, (64, 2048, len(idx) + k))
        assert ref[TARGET].shape == (64, 6) and ref["atom_selector"].shape == (64,)
        assert ref["atom_selector"].dtype == torch.int32 and ref[TARGET].dtype == torch.float32
        assert (ref[TARGET][n:] == 0).all() and (ref["atom_selector"][n:] == 0).all()       # padding rows are unselected
        assert torch.equal(ref[TARGET][:n], torch.cat([dense[i][TARGET] for i in idx]))
        assert torch.equal(ref["atom_selector"][:n], torch.cat([dense[i]["atom_selector"] for i in idx]))
        assert int(ref["atom_selector"].sum()) == sum(SELECTED[i] for i in idx)
        assert ref["_amd_n_valid"].tolist() == [n, e, len(idx)]
    # the compact layout is what the store cannot hold: 1-byte elements, M rows
    with pytest.raises(ValueError, match="1-byte|leading length"):
        GraphStoreHost(fixture_graphs("compact"))


def test_bucketed_epoch_shapes_of_the_fixture():
    """batch_size 5, shuffle seed 3, quanta (32, 1024): six steps in exactly two buckets (the GPU test counts on it)"""
    from matten_amd.data.store import GraphStoreHost
    from matten_amd.dataset.structure_scalar_tensor import _DeviceLoader

    loader = _DeviceLoader(GraphStoreHost(fixture_graphs("dense")), batch_size=5, shuffle=True, seed=3, pad=(32, 1024))
    shapes = [loader.padded_sizes(idx) for _ in range(2) for idx in loader.batch_indices()]
    assert sorted(shapes) == [(32, 1024, 6)] * 2 + [(64, 2048, 6)] * 4


def _rewrite(tmp_path, edit):
    table = json.load(open(FIXTURE))
    edit(table)
    path = tmp_path / "broken.json"
    path.write_text(json.dumps(table))
    return str(path)


def test_data_module_refusals(tmp_path):
    from matten_amd.dataset.structure_scalar_tensor import TensorDataModule

    kw = dict(r_cut=5.0, tensor_target_name=TARGET, tensor_target_formula="ij=ji", atom_selector="atom_selector")
    short = _rewrite(tmp_path, lambda t: t["atom_selector"]["3"].pop())
    for layout in ("compact", "dense"):
        with pytest.raises(ValueError, match=r"row 3 .*11 flags.*12 atoms"):
            TensorDataModule(short, short, short, atom_target_layout=layout, **kw).setup()
    fewer = _rewrite(tmp_path, lambda t: t[TARGET]["5"].pop())
    for layout in ("compact", "dense"):
        with pytest.raises(ValueError, match=r"row 5 .*3 tensors.*4 atoms"):
            TensorDataModule(fewer, fewer, fewer, atom_target_layout=layout, **kw).setup()
    with pytest.raises(ValueError, match="compact.*device_resident|device_resident.*compact"):
        data_module("compact", device_resident=True, device="cuda:0")
    assert data_module(device_resident=True, device="cuda:0").atom_target_layout == "dense"   # the default there
    with pytest.raises(ValueError, match="atom_target_layout"):
        data_module("ragged")
    with pytest.raises(NotImplementedError, match="normalize_tensor_target"):
        data_module(normalize_tensor_target=True)
    for name in ("global_featurizer", "atom_featurizer", "scalar_target_names", "tensor_target_weight"):
        with pytest.raises(NotImplementedError, match=name):
            data_module(**{name: ["x"]})


def _cpu_model():
    from common import ATOMIC
    from matten_amd.model_factory.tfn_atomic_tensor import AtomicTensorModel

    return AtomicTensorModel(tasks=TARGET, backbone_hparams=dict(ATOMIC), dataset_hparams=fixture_dataset_hparams())


def test_dense_route_refusals_of_shared_step():
    from matten_amd import _lib
    from matten_amd.data.graph import collate

    model = _cpu_model()
    batch = collate(fixture_graphs("dense")[:2])
    n = batch["pos"].shape[0]
    decoded = {TARGET: torch.zeros(n, 6, requires_grad=True)}
    model.decode = lambda graphs: decoded            # the forward needs the device; the routing below does not
    # a supported dense batch reaches the kernel's wrapper, which refuses CPU tensors like every other op
    with pytest.raises(_lib.MattenHipError, match="no CPU fallback"):
        model.shared_step(batch, "train")
    with pytest.raises(NotImplementedError, match="target_weight"):
        model.shared_step(dict(batch, target_weight=torch.ones(n, 1)), "train")
    with pytest.raises(ValueError, match=f"{n - 1} target rows for {n} predicted atoms"):
        model.shared_step(dict(batch, **{TARGET: batch[TARGET][:-1]}), "train")
    model.loss_fns[TARGET] = torch.nn.HuberLoss()
    with pytest.raises(NotImplementedError, match="HuberLoss"):
        model.shared_step(batch, "train")
    model.loss_fns[TARGET] = torch.nn.L1Loss()       # supported: past the routing, into the wrapper
    with pytest.raises(_lib.MattenHipError, match="no CPU fallback"):
        model.shared_step(batch, "train")
    # a bool selector keeps the reference's route: indexing, then the torch loss, on any device
    model.loss_fns[TARGET] = torch.nn.MSELoss()
    compact = collate(fixture_graphs("compact")[:2])
    loss, preds, labels = model.shared_step(compact, "train")
    assert preds[TARGET].shape == (5, 6) and labels["atom_selector"].dtype == torch.bool
    assert torch.equal(loss, torch.nn.functional.mse_loss(torch.zeros(5, 6), compact[TARGET]))
    model.update_metrics(preds, labels, "train")
    assert float(model.metrics["metric_train"][TARGET]["MeanAbsoluteError"].count) == 30.0
    with pytest.raises(_lib.MattenHipError, match="no CPU fallback"):
        model.update_metrics(decoded, {TARGET: batch[TARGET], "atom_selector": batch["atom_selector"]}, "val")


def test_selected_mean_loss_and_ops_refuse_what_they_cannot_run():
    from matten_amd import _lib, ops
    from matten_amd.graphs import selected_mean_loss

    loss = selected_mean_loss("mse", key=TARGET)
    assert loss.wants_batch
    pred, target = torch.zeros(4, 6), torch.zeros(4, 6)
    with pytest.raises(ValueError, match="atom_selector"):
        loss({TARGET: pred}, target, {})
    with pytest.raises(TypeError, match="bool"):
        loss({TARGET: pred}, target, {"atom_selector": torch.zeros(4, dtype=torch.bool)})
    with pytest.raises(_lib.MattenHipError, match="no CPU fallback"):
        loss({TARGET: pred}, target, {"atom_selector": torch.ones(4, dtype=torch.int32)})
    with pytest.raises(ValueError, match="kind"):
        selected_mean_loss("huber")
    with pytest.raises(ValueError, match="kind"):
        ops.selected_loss(pred, target, torch.ones(4, dtype=torch.int32), 2)
    with pytest.raises(_lib.MattenHipError, match="no CPU fallback"):
        ops.selected_loss_bwd(pred, target, torch.ones(4, dtype=torch.int32), 0, torch.ones(()), torch.ones((), dtype=torch.int64))


def test_library_declares_binds_and_exports_the_loss_entries():
    from matten_amd import _lib

    header = open(os.path.join(ROOT, "include", "matten_hip.h")).read()
    declared = set(re.findall(r"\b(matten_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in ("matten_selected_loss", "matten_selected_loss_bwd", "matten_selected_loss_workspace_bytes",
                 "matten_selected_loss_tile_elems", "matten_selected_loss_max_blocks"):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 47 and lib.matten_abi_version() == 47          # entries were only added
    assert len(_lib.SIGNATURES["matten_selected_loss"][1]) == 12
    assert len(_lib.SIGNATURES["matten_selected_loss_bwd"][1]) == 10
    assert "model/model.py:340-345" in header and "model/task.py:238-248" in header
    assert "loss.hip" in open(os.path.join(ROOT, "matten_amd", "csrc", "Makefile")).read()


def test_workspace_is_a_function_of_the_element_count():
    from matten_amd import _lib

    lib = _lib.load()
    q, tile, cap = lib.matten_selected_loss_workspace_bytes, lib.matten_selected_loss_tile_elems(), lib.matten_selected_loss_max_blocks()
    assert tile >= 64 and tile % 64 == 0 and cap > 64            # wave64 rounds; "more than 64 workgroups" is reachable
    assert q(0, 6) == 0 and q(-1, 6) == 0 and q(5, 0) == 0
    assert q(1, 1) == 0 and q(tile, 1) == 0 and q(tile // 6, 6) == 0          # one workgroup writes the result itself
    assert q(tile + 1, 1) == 32 and q(tile // 6 + 1, 6) == 32                 # an fp64 sum and an int64 count per workgroup
    assert q(cap * tile, 1) == 16 * cap == q(cap * tile + 1, 1) == q(10 ** 8, 9)


def _host(nbytes, align=16):
    buf = (ctypes.c_char * (nbytes + align))()
    base = ctypes.addressof(buf)
    return buf, base + (-base) % align


def test_entries_check_their_arguments_before_they_launch_anything():
    """host pointers, never dereferenced: every call returns from the argument checks"""
    from matten_amd import _lib

    lib = _lib.load()
    tile = lib.matten_selected_loss_tile_elems()
    keep = {k: _host(64) for k in ("pred", "target", "selector", "sum", "count", "loss", "ws", "g", "grad")}
    good = {k: a for k, (_, a) in keep.items()}

    def fwd(n_rows=4, d=6, kind=0, ws_bytes=0, **ptrs):
        p = dict(good, **ptrs)
        return lib.matten_selected_loss(p["pred"], p["target"], p["selector"], n_rows, d, kind, p["sum"], p["count"], p["loss"],
                                        p["ws"], ws_bytes, None)

    def bwd(n_rows=4, d=6, kind=0, **ptrs):
        p = dict(good, **ptrs)
        return lib.matten_selected_loss_bwd(p["pred"], p["target"], p["selector"], n_rows, d, kind, p["g"], p["count"],
                                            p["grad"], None)

    for call in (fwd, bwd):
        assert call(n_rows=-1) == EINVAL
        assert call(d=0) == EINVAL and call(d=-3) == EINVAL
        assert call(kind=2) == EINVAL and call(kind=-1) == EINVAL
        assert call(n_rows=2 ** 28, d=8) == EINVAL                            # n_rows * d reaches 2^31
        for k in ("pred", "target", "selector", "count"):
            assert call(**{k: None}) == EINVAL, k
    for k in ("sum", "loss"):
        assert fwd(**{k: None}) == EINVAL, k
    assert fwd(sum=good["sum"] + 4) == EINVAL and fwd(count=good["count"] + 4) == EINVAL   # 8-byte words
    for k in ("g", "grad"):
        assert bwd(**{k: None}) == EINVAL, k
    # result words are needed whatever n_rows is; the adjoint of an empty row set has nothing to write
    assert fwd(n_rows=0, sum=None) == EINVAL
    assert bwd(n_rows=0, pred=None, target=None, selector=None, grad=None) == OK
    # a workspace is needed from the second workgroup on
    rows = tile // 6 + 1
    need = lib.matten_selected_loss_workspace_bytes(rows, 6)
    assert need == 32
    assert fwd(n_rows=rows, ws=None, ws_bytes=need) == EINVAL
    assert fwd(n_rows=rows, ws=good["ws"] + 4, ws_bytes=need) == EINVAL
    assert fwd(n_rows=rows, ws_bytes=need - 1) == ENOMEM
    assert fwd(n_rows=rows, ws_bytes=0) == ENOMEM
