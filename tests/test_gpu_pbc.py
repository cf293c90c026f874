"""
GPU tests of open and partly periodic structures: matten_graph_prep_pbc and the pair-free search
(matten_neighbor_rows_count / _fill) against the host builder -- whose own specification, a brute-force enumeration, is
in tests/test_pbc_host.py -- and the model and predict() on top of them.  Index outputs are compared exactly.
"""
import os

import numpy as np
import pytest
import torch

from common import ATOMIC, LMAX2, build_pair
from test_gpu_parity import RTOL, _want64, close, close_blocks

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OPEN, SLAB = (False, False, False), (True, True, False)


def _item(s, pbc=None):
    return (s["cart_coords"], s.get("lattice"), s["atomic_numbers"], s.get("pbc", True) if pbc is None else pbc)


def _mixed(golden_dir, seed=3):
    """crystals, slabs, wires and molecules interleaved: (pos, cell or None, Z, pbc) items"""
    from matten_amd.data import synthetic
    from oracle.matten_ref import data as rdata

    rng = np.random.default_rng(seed)
    n100 = rdata.structures_from_json(os.path.join(golden_dir, "example_crystal_elasticity_tensor_n100.json"))[:6]
    fcc = synthetic.fcc64_structures(2)
    mols = synthetic.molecules(5, seed=seed)
    slabs = synthetic.fcc_slabs(2, seed=seed) + synthetic.fcc_slabs(1, seed=seed + 1, vacuum_vector=False)
    sheet = synthetic.fcc_slabs(1, seed=seed + 2, layers=1, vacuum_vector=False)[0]      # one atom thick
    unwrapped = dict(slabs[0])
    hop = rng.integers(-2, 3, (len(unwrapped["cart_coords"]), 3)) * np.array([1, 1, 0])
    unwrapped["cart_coords"] = unwrapped["cart_coords"] + hop @ unwrapped["lattice"]   # atoms outside the cell
    lone = dict(mols[0])                                                                # a molecule with an isolated atom
    lone["cart_coords"] = np.concatenate([lone["cart_coords"], lone["cart_coords"][:1] + 40.0])
    lone["atomic_numbers"] = np.concatenate([lone["atomic_numbers"], [8]])
    # wires: an n100 crystal periodic along one axis only (the other rows stay in `cell` and generate nothing), and a
    # chain along z whose open rows are zero
    chain = {"lattice": np.diag([0.0, 0.0, 2.6]), "atomic_numbers": np.array([6, 7]),
             "cart_coords": np.array([[0.1, 0.0, 0.2], [0.3, 0.9, 1.5 + 2.6 * 3]])}
    items = [_item(n100[0]), _item(mols[1]), _item(slabs[0]), _item(n100[1], (True, False, False)), _item(fcc[0]),
             _item(sheet), _item(lone), _item(chain, (False, False, True)), _item(unwrapped), _item(n100[2], (False, True, True)),
             _item(slabs[2]), _item(mols[2]), _item(n100[3], (False, True, False)), _item(slabs[1]), _item(fcc[1]),
             _item(n100[4], OPEN), _item(mols[3]), _item(n100[5])]
    return items


def _host(items, r_cut=5.0):
    from matten_amd.data.graph import collate, crystal_graph

    return [crystal_graph(p, c, z, r_cut, pbc=f) for p, c, z, f in items]


def _assert_same_graph(got, want, csr=True):
    from matten_amd import ops
    from matten_amd.data._key import AMD_PERM, AMD_ROWPTR, AMD_SRC

    for k in want:
        g = got[k].cpu()
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, k
        assert torch.equal(g, want[k]), k
    if csr:
        perm, rowptr, src, err = ops.csr_build(got["edge_index"], got["pos"].shape[0])
        assert int(err.item()) == 0
        assert torch.equal(got[AMD_PERM], perm) and torch.equal(got[AMD_ROWPTR], rowptr) and torch.equal(got[AMD_SRC], src)
        assert set(got) - set(want) == {AMD_PERM, AMD_ROWPTR, AMD_SRC}
    else:
        assert set(got) == set(want)


@pytest.mark.parametrize("seed", [3, 11])
def test_device_builder_equals_host_builder_on_mixed_batches(golden_dir, monkeypatch, seed):
    """edge_index, shifts, num_neigh (and every other key) bit for bit, the emitted CSR against ops.csr_build; then the
    rows route, forced by the environment variable, against the pair route on the same batch"""
    from matten_amd.data.graph import batch_graphs_gpu, collate

    items = _mixed(golden_dir, seed)
    want = collate(_host(items))
    assert not want["edge_cell_shift"][:, 2][want["batch"][want["edge_index"][0]] == 2].any()   # the slab: S_z = 0
    assert int((want["num_neigh"] == 0).sum()) == 1                                              # the isolated atom
    pair = batch_graphs_gpu(items, 5.0, DEV)
    _assert_same_graph(pair, want)
    monkeypatch.setenv("MATTEN_NEIGHBOR_ROWS_MIN_ATOMS", "1")
    rows = batch_graphs_gpu(items, 5.0, DEV)
    _assert_same_graph(rows, want, csr=False)
    for k in rows:
        assert torch.equal(rows[k], pair[k]), k
    # fully periodic batches take the rows route too when asked to, through the unchanged prologue
    crystals = [it[:3] for it in items if it[3] is True]
    assert len(crystals) >= 4
    got = batch_graphs_gpu(crystals, 5.0, DEV)
    monkeypatch.setenv("MATTEN_NEIGHBOR_ROWS_MIN_ATOMS", "1000000")
    ref = batch_graphs_gpu(crystals, 5.0, DEV)
    assert not any(k.startswith("_amd_") for k in got) and any(k.startswith("_amd_") for k in ref)
    for k in got:
        assert torch.equal(got[k], ref[k]), k


def test_prologue_with_all_axes_periodic_is_the_old_prologue_bit_for_bit(golden_dir):
    from matten_amd import ops

    items = [it for it in _mixed(golden_dir) if it[1] is not None and np.linalg.matrix_rank(it[1]) == 3]
    sizes = np.array([len(it[0]) for it in items])
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    pair_ptr = np.concatenate([[0], np.cumsum(sizes * sizes)]).astype(np.int64)
    pos = torch.from_numpy(np.concatenate([it[0] for it in items])).to(DEV)
    cell = torch.from_numpy(np.stack([it[1] for it in items]).reshape(-1, 9)).to(DEV)
    ptr_d, pair_ptr_d = torch.from_numpy(ptr).to(DEV), torch.from_numpy(pair_ptr).to(DEV)
    old = ops.graph_prep(pos, cell, ptr_d, 5.0)
    flag = torch.zeros(1, dtype=torch.int64, device=DEV)
    new = ops.graph_prep_pbc(pos, cell, ptr_d, torch.ones(len(items), 3, dtype=torch.uint8, device=DEV), 5.0, flag)
    for a, b in zip(old, new[:5]):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert int(flag.item()) == 0 and not new[5].any()
    lists = [ops.neighbor_list(pos, cell, ptr_d, p[0], p[1], pair_ptr_d, 5.0, int(sizes.max()), int(pair_ptr[-1]))
             for p in (old, new)]
    for a, b in zip(lists[0][:4], lists[1][:4]):
        assert torch.equal(a, b)
    assert all(torch.equal(a, b) for a, b in zip(lists[0][5], lists[1][5]))

    # an open axis: frac = 0 and bound = 0 exactly, for which shift_range yields [0, 0]:
    # slack = 1e-6 (1 + |0| + 0); lo = ceil(-0 - 0 - 1e-6) = 0, hi = floor(0 - 0 + 1e-6) = 0
    assert int(np.ceil(-1e-6)) == 0 and int(np.floor(1e-6)) == 0
    pbc = torch.tensor([[k % 2, (k // 2) % 2, (k // 4) % 2] for k in range(len(items))], dtype=torch.uint8, device=DEV)
    part = ops.graph_prep_pbc(pos, cell, ptr_d, pbc, 5.0, flag)
    batch = part[2]
    open_axis = pbc == 0
    assert not part[1][open_axis].any() and not part[0][open_axis[batch]].any()
    assert bool((part[1][~open_axis] > 0).all()) and int(flag.item()) == 0
    # on a periodic axis the numbers are those of the periodic sub-lattice: for an orthogonal cell, the old ones
    ortho = torch.tensor(np.diag([4.0, 5.0, 6.0]).reshape(1, 9), device=DEV)
    p1 = torch.tensor([[0.5, 7.0, -2.0]], dtype=torch.float64, device=DEV)
    one = torch.tensor([0, 1], device=DEV)
    full = ops.graph_prep(p1, ortho, one, 5.0)
    for flags in ([1, 1, 0], [0, 1, 0], [1, 0, 1]):
        f = torch.tensor([flags], dtype=torch.uint8, device=DEV)
        got = ops.graph_prep_pbc(p1, ortho, one, f, 5.0, flag)
        m = f[0] != 0
        assert torch.allclose(got[1][0][m], full[1][0][m], rtol=1e-14) and torch.allclose(got[0][0][m], full[0][0][m], rtol=1e-14)


def test_singular_periodic_vectors_are_reported_by_name(golden_dir):
    from matten_amd.data.graph import SingularCells, batch_graphs_gpu

    items = _mixed(golden_dir)[:5]
    bad = (items[2][0], np.array([[4.0, 0, 0], [8.0, 0, 0], [0, 0, 9.0]]), items[2][2], SLAB)     # dependent in-plane vectors
    zero = (items[2][0], np.diag([4.0, 0.0, 4.0]), items[2][2], SLAB)                              # zero vector on a periodic axis
    with pytest.raises(SingularCells) as e:
        batch_graphs_gpu(items[:2] + [bad] + items[2:] + [zero], 5.0, DEV)
    assert e.value.indices == [2, 6] and isinstance(e.value, ValueError) and "[2, 6]" in str(e.value)
    # the same vectors on open axes are nobody's business
    fine = (items[1][0], bad[1], items[1][2], OPEN)
    assert batch_graphs_gpu([fine], 5.0, DEV)["edge_index"].shape[1] > 0


def _boxed(items, r_cut=5.0):
    """every structure fully periodic, with vacuum along its open axes: sides exceed extent + r_cut there"""
    out = []
    for p, c, z, f in items:
        f = (f,) * 3 if isinstance(f, bool) else f
        c = np.zeros((3, 3)) if c is None else np.array(c, dtype=np.float64)
        if not all(f):
            assert all(not c[k].any() or f[k] for k in range(3)), "vacuum boxes need zero open rows"
            for k in range(3):
                if not f[k]:
                    c[k, k] = (p[:, k].max() - p[:, k].min()) + r_cut + 1.0
        out.append((p, c, z))
    return out


def _open_batch(golden_dir):
    from matten_amd.data import synthetic

    mols = synthetic.molecules(6, seed=21)
    slabs = synthetic.fcc_slabs(2, seed=22, vacuum_vector=False) + synthetic.fcc_slabs(1, seed=23, layers=1, vacuum_vector=False)
    chain = {"lattice": np.diag([0.0, 0.0, 2.6]), "atomic_numbers": np.array([6, 7]), "pbc": (False, False, True),
             "cart_coords": np.array([[0.1, 0.0, 0.2], [0.3, 0.9, 1.5]])}
    fcc = synthetic.fcc64_structures(1)
    return [_item(s) for s in (mols[0], slabs[0], mols[1], chain, fcc[0], slabs[2], mols[2], slabs[1], mols[3], mols[4], mols[5])]


@pytest.mark.parametrize("config", ["lmax2", "atomic"])
def test_forward_on_open_structures(golden_dir, config):
    """bitwise equal to the forward on the same structures in vacuum boxes (the same edge list; zero shifts add exact
    zeros), and equal to the oracle on the host-built graph to the tolerance tests/test_gpu_parity.py applies"""
    from matten_amd.data.graph import average_num_neighbors, batch_graphs_gpu, collate

    items = _open_batch(golden_dir)
    graphs = _host(items)
    ds = {"allowed_species": sorted({int(z) for it in items for z in it[2]}), "average_num_neighbors": average_num_neighbors(graphs)}
    atomic = config == "atomic"
    ref, model = build_pair(dict(ATOMIC if atomic else LMAX2), ds, randomize_bn=True, atomic=atomic)
    name = "nmr_tensor" if atomic else "elastic_tensor_full"
    open_b = batch_graphs_gpu(items, 5.0, DEV)
    box_b = batch_graphs_gpu(_boxed(items), 5.0, DEV)
    assert torch.equal(open_b["edge_index"], box_b["edge_index"]) and torch.equal(open_b["edge_cell_shift"], box_b["edge_cell_shift"])
    assert not torch.equal(open_b["cell"], box_b["cell"])
    with torch.no_grad():
        y_open = model(dict(open_b), task_name=name)[0][name]
        y_box = model(dict(box_b), task_name=name)[0][name]
        want = ref.decode(collate(graphs))
    assert torch.equal(y_open, y_box)
    if atomic:
        assert y_open.shape == (sum(len(it[0]) for it in items), 6)
        close(y_open, want, RTOL, "per-atom irreps, open structures")
    else:
        assert y_open.shape == (len(items), 21)
        close_blocks(y_open, want, what="open structures [B,21]", want64=_want64(ref, graphs))


def test_predict_on_molecules_and_mixed_lists(golden_dir):
    from matten_amd import predict as P
    from matten_amd.data import synthetic
    from matten_amd.data.graph import average_num_neighbors, collate
    from oracle.matten_ref.model import ToCartesian

    mols = synthetic.molecules(7, seed=31)
    graphs = _host([_item(m) for m in mols])
    ds = {"allowed_species": list(synthetic.MOLECULE_SPECIES), "average_num_neighbors": average_num_neighbors(graphs)}
    ref, model = build_pair(dict(ATOMIC), ds, randomize_bn=True, atomic=True)
    cfg = {"data": {"r_cut": 5.0, "tensor_target_name": "nmr_tensor", "tensor_target_formula": "ij=ji"}}

    class Molecule:                                    # pymatgen's Molecule: no .lattice
        def __init__(self, m):
            self.cart_coords, self.atomic_numbers = m["cart_coords"], m["atomic_numbers"]

    bare = [{k: v for k, v in m.items() if k != "pbc"} for m in mols]
    with torch.no_grad():
        want = ToCartesian("ij=ji")(ref.decode(collate(graphs)))
    for structs in (mols, bare, [Molecule(m) for m in mols]):
        out = P.predict(structs, model=model, config=cfg, is_atomic_tensor=True, batch_size=3)
        assert len(out) == sum(len(m["atomic_numbers"]) for m in mols) and out[0].shape == (3, 3)
        close(torch.as_tensor(np.stack(out)), want, RTOL, "predict() per-atom tensors of molecules")
    # the override: crystals read as clusters
    boxed = [dict(m, lattice=30.0 * np.eye(3), pbc=True) for m in mols]
    out2 = P.predict(boxed, model=model, config=cfg, is_atomic_tensor=True, pbc=False)
    assert all(np.array_equal(a, b) for a, b in zip(out2, P.predict(mols, model=model, config=cfg, is_atomic_tensor=True)))

    # per-structure tensors of a list mixing crystals, slabs, molecules and entries that cannot be used
    fcc = synthetic.fcc64_structures(3)
    slabs = synthetic.fcc_slabs(2, seed=32)
    heavy = [dict(m, atomic_numbers=np.full(len(m["atomic_numbers"]), 29)) for m in mols[:2]]
    malformed = {"lattice": np.eye(3), "cart_coords": np.zeros((2, 3)), "atomic_numbers": np.array([29])}
    bad_slab = dict(slabs[0], lattice=np.diag([10.0, 0.0, 10.0]))                 # zero vector on a periodic axis
    lone = {"cart_coords": np.zeros((1, 3)), "atomic_numbers": np.array([29])}   # a one-atom molecule: no edge
    structs = [fcc[0], slabs[0], malformed, heavy[0], fcc[1], bad_slab, slabs[1], lone, heavy[1], fcc[2]]
    items = [_item(s) for s in structs]
    good = [k for k in range(len(structs)) if k not in (2, 5, 7)]
    g2 = _host([items[k] for k in good])
    ds2 = {"allowed_species": list(synthetic.FCC_METALS), "average_num_neighbors": average_num_neighbors(g2)}
    ref2, model2 = build_pair(dict(LMAX2), ds2, randomize_bn=True)
    cfg2 = {"data": {"r_cut": 5.0, "tensor_target_name": "elastic_tensor_full", "tensor_target_formula": "ijkl=jikl=klij"}}
    with pytest.warns(UserWarning):
        out = P.predict(structs, model=model2, config=cfg2, is_elasticity_tensor=False)
    assert [o is None for o in out] == [k in (2, 5, 7) for k in range(len(structs))]
    # compared as predict() hands them out, in Cartesian form, like the per-atom tensors above and in
    # tests/test_gpu_parity.py: the lmax-2 configuration has no 4e part, and an irreps view of the fp32 Cartesian
    # tensor would carry the round trip's rounding into that exactly empty block
    with torch.no_grad():
        want2 = ToCartesian("ijkl=jikl=klij")(ref2.decode(collate(g2)))
    got2 = torch.as_tensor(np.stack([out[k] for k in good]))
    assert got2.shape == (len(good), 3, 3, 3, 3)
    close(got2, want2, RTOL, "predict() on a mixed list")


def test_rows_route_memory_and_forward_on_a_large_cluster():
    """fcc_cluster(8000): the peak of the build above what it returns stays below 1 KB per atom (the pair route keeps
    24 B x n^2 / n = 190 KB per atom there), the list equals the host builder's, and the forward runs on it with the
    CSR it builds itself"""
    from matten_amd.data import synthetic
    from matten_amd.data.graph import batch_graphs_gpu, collate, crystal_graph, rows_min_atoms

    n = 8000
    assert n >= rows_min_atoms()
    c = synthetic.fcc_cluster(n)
    item = _item(c)
    batch_graphs_gpu([_item(synthetic.molecules(1)[0])], 5.0, DEV)            # library and allocator warm
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    got = batch_graphs_gpu([item], 5.0, DEV)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    returned = sum(t.numel() * t.element_size() for t in got.values())
    print(f"rows route, {n} atoms: peak {peak} B, returned {returned} B, scratch {(peak - returned) / n:.1f} B per atom")
    assert peak - returned < 1024 * n
    assert not any(k.startswith("_amd_") for k in got)
    want = collate([crystal_graph(item[0], None, item[2], 5.0, pbc=False)])
    _assert_same_graph(got, want, csr=False)

    ds = {"allowed_species": list(synthetic.FCC_METALS), "average_num_neighbors": float(want["num_neigh"].mean())}
    _, model = build_pair(dict(LMAX2), ds, randomize_bn=True)
    small = batch_graphs_gpu([_item(synthetic.fcc_cluster(300))], 5.0, DEV)
    with torch.no_grad():
        y = model(dict(got))[0]["elastic_tensor_full"]
        y_small = model(dict(small))[0]["elastic_tensor_full"]
    assert y.shape == (1, 21) and bool(torch.isfinite(y).all()) and bool(torch.isfinite(y_small).all())
    assert float(y.abs().max()) > 0
