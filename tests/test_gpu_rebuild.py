"""
The sync-free edge-list rebuild on the GPU: ``GeometryBatch.update`` (matten_neighbor_fill_capped) against the host
definition of the padded layout (``GraphStoreHost.padded_reference`` of host graphs at the same fp64 geometry), the
overflow and edgeless flags, ``GraphedGeometryStep`` replays against eager forwards / ``geometry_gradients`` on the store's
padded batch, and ``predict.evaluate_frames`` against ``predict.evaluate``.

Fixture (tests/rebuild_cases.py, r_cut 5.0): total edge counts 302 / 294 / 270 / 260 / 252 at scales 0.94 / 0.97 / 1.00 /
1.03 / 1.06 (tests/test_rebuild_host.py holds them); the 5-atom crystal alone has 82 fewer.
"""
import numpy as np
import pytest
import torch

from common import LMAX2, build_pair
from rebuild_cases import R_CUT, fixture_crystals, host_graphs
from test_gpu_parity import close_blocks

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TASK = "elastic_tensor_full"
OPEN_Z = np.array([[True, True, True], [True, True, True], [True, True, False]])


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _make(caps=None, training=True, pbc=None, **kw):
    """a GeometryBatch of the three fixture crystals with capacities (N_b, E_b, B_b) (None: the defaults)"""
    from matten_amd.data.rebuild import GeometryBatch

    pos, cell, Z, ptr = fixture_crystals()
    if caps is not None:
        kw.update(edge_capacity=caps[1], pad_nodes=caps[0] - 8, pad_crystals=caps[2] - 3)
    return GeometryBatch(pos, cell, Z, ptr, R_CUT, DEV, pbc=pbc, training=training, **kw)


def _move(gb, scale):
    pos, cell, _, _ = fixture_crystals(scale)
    gb.update(pos=_dev(pos), cell=_dev(cell))


def _graphs_of(gb, pbc=None):
    """host graphs of the geometry the batch holds (its fp64 buffers, copied back)"""
    _, _, Z, ptr = fixture_crystals()
    return host_graphs(gb.pos64.cpu().numpy(), gb.cell64.cpu().numpy().reshape(-1, 3, 3), Z, ptr, pbc)


def _assert_reference(gb, pbc=None):
    from matten.data.store import GraphStoreHost

    want = GraphStoreHost(_graphs_of(gb, pbc)).padded_reference(range(3), gb.capacity, training=gb.training)
    assert list(gb.batch.keys()) == list(want.keys())
    for k, v in want.items():
        g = gb.batch[k]
        assert g.dtype == v.dtype and g.shape == v.shape, (k, g.dtype, v.dtype, g.shape, v.shape)
        assert g.is_contiguous() and torch.equal(g.cpu(), v), k
    return want


# ----------------------------------------------------------------------------------------------------------------------
# 1. parity with padded_reference
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("caps", [(9, 296, 4), (11, 384, 5), (9, 270, 4)], ids=lambda c: "x".join(map(str, c)))
def test_update_matches_padded_reference(caps):
    gb = _make(caps)
    assert gb.capacity == caps
    tensors = dict(gb.batch)
    edges = []
    for scale in ((1.00,) if caps[1] == 270 else (1.00, 1.03, 0.97, 1.00)):
        _move(gb, scale)
        want = _assert_reference(gb)
        edges.append(int(want["_amd_n_valid"][1]))
        gb.check()
    assert edges == ([270] if caps[1] == 270 else [270, 260, 294, 270])
    assert all(gb.batch[k] is v for k, v in tensors.items()), "the tensors are allocated once and rewritten in place"
    if caps[1] == 270:   # the exact fit: no padding edge, the one padding node has degree 0
        assert gb.batch["num_neigh"][8:].tolist() == [0.0] and gb.batch["_amd_rowptr"][8:].tolist() == [270, 270]


def test_update_matches_padded_reference_with_an_open_axis():
    gb = _make((9, 296, 4), pbc=OPEN_Z)
    seen = set()
    for scale in (1.00, 1.03, 0.97, 1.00):
        _move(gb, scale)
        seen.add(int(_assert_reference(gb, OPEN_Z)["_amd_n_valid"][1]))
        gb.check()
    assert len(seen) > 1 and max(seen) < 294, "the open axis removes images; the count still follows the geometry"


def test_fp32_positions_are_widened_on_the_device():
    gb = _make((9, 296, 4))
    pos, cell, _, _ = fixture_crystals(1.03)
    gb.update(pos=_dev(pos).float(), cell=_dev(cell).float())
    assert torch.equal(gb.pos64, _dev(pos).float().double()) and gb.pos64.dtype == torch.float64
    _assert_reference(gb)   # the list of the ROUNDED positions


# ----------------------------------------------------------------------------------------------------------------------
# 2. overflow, 3. edgeless
# ----------------------------------------------------------------------------------------------------------------------
def test_overflow_writes_nothing_but_the_flag():
    from matten_amd.data.rebuild import EDGE_KEYS, FLAG_OVERFLOW, TRAIN_KEYS, EdgeCapacityExceeded

    gb = _make((9, 296, 4))
    _move(gb, 0.97)
    gb.check()
    assert gb.batch["_amd_n_valid"].tolist() == [8, 294, 3]
    before = {k: gb.batch[k].clone() for k in EDGE_KEYS + TRAIN_KEYS}
    _move(gb, 0.94)
    assert int(gb.flags.item()) & FLAG_OVERFLOW
    for k, v in before.items():
        assert torch.equal(gb.batch[k], v), k
    with pytest.raises(EdgeCapacityExceeded, match="302.*296") as e:
        gb.check()
    assert (e.value.n_edges, e.value.capacity) == (302, 296)
    assert int(gb.flags.item()) == 0, "check() clears the word"
    word = torch.full((1,), 7, dtype=torch.int32, device=DEV)
    gb.update(flags_out=word)          # this update's flags alone, and not in the sticky word
    assert word.tolist() == [FLAG_OVERFLOW] and int(gb.flags.item()) == 0
    old = gb.batch["edge_index"]
    gb.grow(384)
    assert gb.capacity == (9, 384, 4) and gb.batch["edge_index"] is not old
    gb.check()
    want = _assert_reference(gb)
    assert want["_amd_n_valid"].tolist() == [8, 302, 3]


def test_edgeless_crystal_is_flagged():
    from matten_amd.data.graph import EdgelessStructures
    from matten_amd.data.rebuild import FLAG_EDGELESS

    gb = _make((9, 296, 4))
    _, cell, _, _ = fixture_crystals()
    cell[0] = np.eye(3) * 6.0          # the 1-atom cell: its nearest image is beyond the cutoff
    gb.update(cell=_dev(cell))
    assert int(gb.flags.item()) == FLAG_EDGELESS
    assert gb.batch["_amd_n_valid"].tolist() == [8, 270 - 26, 3] and gb.batch["num_neigh"][0].item() == 0.0
    with pytest.raises(EdgelessStructures) as e:
        gb.check()
    assert e.value.indices == [0] and int(gb.flags.item()) == 0


# ----------------------------------------------------------------------------------------------------------------------
# 4. replay against eager, 5. gradients
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    from matten_amd.data.graph import average_num_neighbors

    graphs = host_graphs(*fixture_crystals())
    ds = {"allowed_species": [13, 14, 29, 79], "average_num_neighbors": average_num_neighbors(graphs)}
    return build_pair(LMAX2, ds, randomize_bn=True)[1]


def _eager_batch(gb):
    from matten.data.store import DeviceGraphStore

    return DeviceGraphStore.from_graphs(_graphs_of(gb), DEV).batch(range(3), training=False, pad_to=gb.capacity)


def test_replay_is_bit_identical_to_eager(model):
    from matten_amd.graphs import GraphedGeometryStep

    gb = _make(training=False)
    assert gb.capacity == (9, 384, 4)
    step = GraphedGeometryStep(model, gb, task_name=TASK)
    outs = []
    for scale in (1.00, 1.03, 0.97, 1.00):
        pos, cell, _, _ = fixture_crystals(scale)
        got = step.step(pos=_dev(pos), cell=_dev(cell)).clone()
        assert got.shape == (3, 21)
        with torch.no_grad():
            want = model(_eager_batch(gb), task_name=TASK)[0][TASK][:3]
        assert torch.equal(got, want), scale
        assert torch.equal(step.step(), got), "a second step at an unchanged geometry"
        outs.append(got)
    gb.check()
    assert torch.equal(outs[0], outs[3]) and not torch.equal(outs[0], outs[1])


def test_replayed_gradients_match_geometry_gradients(model):
    from matten_amd.elastic import elastic_moduli_from_irreps
    from matten_amd.geometry import geometry_gradients
    from matten_amd.graphs import GraphedGeometryStep

    fn = lambda p: elastic_moduli_from_irreps(p[TASK][:3]).k_vrh.sum()   # noqa: E731
    gb = _make(training=False)
    step = GraphedGeometryStep(model, gb, fn=fn, task_name=TASK)
    assert all(p.grad is None for p in model.parameters()), "the caller's parameter gradients are left alone"
    for scale in (1.00, 1.03):
        pos, cell, _, _ = fixture_crystals(scale)
        step.step(pos=_dev(pos), cell=_dev(cell))
        got = {k: v.clone() for k, v in step.grads.items()}
        want = geometry_gradients(model, _eager_batch(gb), fn, task_name=TASK)
        model.zero_grad(set_to_none=True)
        assert got["pos"].shape == (8, 3) and got["cell"].shape == (9, 3) and got["strain"].shape == (3, 3, 3)
        assert want["pos"][:8].abs().max() > 0 and want["cell"][:9].abs().max() > 0
        assert torch.equal(got["pos"], want["pos"][:8]), scale
        assert torch.equal(got["cell"], want["cell"][:9]), scale
        assert torch.equal(got["strain"], want["strain"][:3]), scale
    gb.check()


# ----------------------------------------------------------------------------------------------------------------------
# 6. evaluate_frames
# ----------------------------------------------------------------------------------------------------------------------
def test_evaluate_frames_matches_evaluate_and_regrows(model, monkeypatch):
    """Six frames of the 5-atom crystal alone (188 edges at scale 1.00, 220 at 0.94).  slack=1.0 sizes the buffers from
    frame 0 without head room (192 edges), so the frames at 0.97 and 0.94 overflow and are run again after ONE grow to
    64 * ceil(1.25 * 220 / 64) = 320."""
    from matten_amd import predict
    from matten_amd.data import rebuild
    from matten_amd.utils import CartesianTensorWrapper

    scales = (1.00, 1.03, 0.97, 0.94, 1.06, 1.00)
    frames = [fixture_crystals(s) for s in scales]
    pos_frames = np.stack([p[3:] for p, _, _, _ in frames])
    cell_frames = np.stack([c[2] for _, c, _, _ in frames])
    Z = frames[0][2][3:]
    structure = {"lattice": cell_frames[0], "cart_coords": pos_frames[0], "atomic_numbers": Z}
    grown = []
    grow = rebuild.GeometryBatch.grow
    monkeypatch.setattr(rebuild.GeometryBatch, "grow", lambda self, e: (grown.append(int(e)), grow(self, e))[1])
    got, props = predict.evaluate_frames(model, structure, pos_frames, cell_frames, r_cut=R_CUT, tensor_target_name=TASK,
                                         properties=True, slack=1.0)
    assert grown == [320]
    want = predict.evaluate(model, [(pos_frames[f], cell_frames[f], Z) for f in range(6)], tensor_target_name=TASK, r_cut=R_CUT)
    conv = CartesianTensorWrapper("ijkl=jikl=klij")
    assert len(got) == len(want) == 6
    for f in range(6):
        assert got[f].shape == (3, 3, 3, 3)
        close_blocks(conv.from_cartesian(got[f]), conv.from_cartesian(want[f]), what=f"frame {f} (scale {scales[f]})")
    assert torch.equal(got[0], got[5]) and props.k_vrh.shape[0] == 6 and torch.isfinite(props.k_vrh).all()
    plain = predict.evaluate_frames(model, structure, pos_frames, cell_frames, r_cut=R_CUT, tensor_target_name=TASK)
    assert grown == [320], "with the default head room (256 edges) no frame overflows"
    for f in range(6):
        close_blocks(conv.from_cartesian(plain[f]), conv.from_cartesian(want[f]), what=f"default slack, frame {f}")
