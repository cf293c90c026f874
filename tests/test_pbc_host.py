"""
CPU tests of open and partly periodic structures (pbc) in the host graph builder and everything above it.

The specification is a brute-force fp64 enumeration written here (ASE, which the reference delegates to in
data/data.py:285-413, is not a dependency): every ordered triple (i, j, S) with |pos[j] + S.cell - pos[i]| < r_cut,
S_k = 0 on every open axis, minus (i == j, S == 0), in the canonical order (i, j, Sx, Sy, Sz).
"""
import itertools
import json
import os

import numpy as np
import pytest
import torch

FLAGS = list(itertools.product((False, True), repeat=3))


def brute_force(pos, cell, r_cut, pbc, reach=8):
    """All images within `reach` cells along the periodic axes, no pruning; the distance expression is the builder's."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    cell = np.zeros((3, 3)) if cell is None else np.asarray(cell, dtype=np.float64).reshape(3, 3)
    n = len(pos)
    rng = [np.arange(-reach, reach + 1) if p else np.arange(0, 1) for p in pbc]
    S = np.stack(np.meshgrid(*rng, indexing="ij"), axis=-1).reshape(-1, 3)
    T = S @ cell
    out = []
    for i in range(n):
        d = (pos[None, :, :] + T[:, None, :]) - pos[i]              # [ns, n, 3]
        ok = np.sqrt((d * d).sum(-1)) < float(r_cut)
        for s, j in zip(*np.nonzero(ok)):
            if not (i == j and not S[s].any()):
                out.append((i, j, *S[s]))
    out = np.array(sorted(out), dtype=np.int64).reshape(-1, 5)
    assert out.size == 0 or np.abs(out[:, 2:]).max() < reach, "brute force: reach too small"
    return out[:, :2].T, out[:, 2:]


def triclinic(rng, n):
    """a seeded triclinic cell (sides 4-7 A, clearly non-orthogonal) with n atoms, a third of them outside the cell"""
    cell = np.diag(rng.uniform(4.0, 7.0, 3)) + rng.uniform(-1.2, 1.2, (3, 3))
    frac = rng.uniform(0.0, 1.0, (n, 3))
    frac[::3] += rng.integers(-2, 3, (len(frac[::3]), 3))            # unwrapped atoms
    return frac @ cell, cell


@pytest.mark.parametrize("pbc", FLAGS, ids=lambda p: "".join("pbc"[k] if f else "-" for k, f in enumerate(p)))
def test_neighbor_list_equals_brute_force_for_every_flag_combination(pbc):
    from matten_amd.data import graph

    rng = np.random.default_rng(1000 + sum(f << k for k, f in enumerate(pbc)))
    for n in (1, 5, 12):
        pos, cell = triclinic(rng, n)
        if n == 1 and not any(pbc):
            continue
        want = brute_force(pos, cell, 5.0, pbc)
        if want[0].shape[1] == 0:
            with pytest.raises(ValueError, match="no edges remain"):
                graph.neighbor_list(pos, cell, 5.0, pbc=pbc)
            continue
        ei, sh = graph.neighbor_list(pos, cell, 5.0, pbc=pbc)
        assert ei.dtype == np.int64 and sh.dtype == np.int64
        assert np.array_equal(ei, want[0]) and np.array_equal(sh, want[1])
        assert not sh[:, ~np.array(pbc)].any()
        g = graph.crystal_graph(pos, cell, np.full(n, 14), 5.0, pbc=pbc)
        assert torch.equal(g["cell"], torch.as_tensor(cell, dtype=torch.float32))    # the caller's cell, not the completed one
        assert torch.equal(g["edge_index"], torch.as_tensor(want[0]))


def test_molecules_without_a_cell_and_a_slab_with_a_vacuum_vector():
    from matten_amd.data import graph, synthetic

    for m in synthetic.molecules(6):
        want = brute_force(m["cart_coords"], None, 5.0, (False,) * 3)
        for cell in (None, np.zeros((3, 3))):
            ei, sh = graph.neighbor_list(m["cart_coords"], cell, 5.0, pbc=False)
            assert np.array_equal(ei, want[0]) and np.array_equal(sh, want[1]) and not sh.any()
        g = graph.crystal_graph(m["cart_coords"], None, m["atomic_numbers"], 5.0, pbc=False)
        assert g["cell"].shape == (3, 3) and not g["cell"].any()
        assert torch.equal(g["num_neigh"], torch.as_tensor(np.bincount(want[0][0], minlength=len(m["cart_coords"]))).float())
    for s in synthetic.fcc_slabs(2) + synthetic.fcc_slabs(1, vacuum_vector=False):
        want = brute_force(s["cart_coords"], s["lattice"], 5.0, s["pbc"])
        ei, sh = graph.neighbor_list(s["cart_coords"], s["lattice"], 5.0, pbc=s["pbc"])
        assert np.array_equal(ei, want[0]) and np.array_equal(sh, want[1])
        assert sh[:, :2].any() and not sh[:, 2].any()
    # the open-axis vector generates no image however short it is: the same list with it and without it
    s = synthetic.fcc_slabs(1)[0]
    short = s["lattice"].copy()
    short[2] = (0.1, 0.2, 1.0)
    a = graph.neighbor_list(s["cart_coords"], s["lattice"], 5.0, pbc=s["pbc"])
    b = graph.neighbor_list(s["cart_coords"], short, 5.0, pbc=s["pbc"])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # ... and may even lie in the plane of the periodic ones
    short[2] = s["lattice"][0]
    b = graph.neighbor_list(s["cart_coords"], short, 5.0, pbc=s["pbc"])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_pbc_true_is_the_list_of_the_fully_periodic_builder(golden_dir):
    """pbc=True is the code path of every earlier version: against the oracle's builder (which has no pbc argument)
    on the fcc-64 and n100 inputs, with the argument given in each of its spellings"""
    from matten_amd.data import graph, synthetic
    from oracle.matten_ref import data as rdata

    structs = rdata.structures_from_json(os.path.join(golden_dir, "example_crystal_elasticity_tensor_n100.json"))
    structs += synthetic.fcc64_structures(3)
    for k, s in enumerate(structs):
        c, d = rdata.neighbor_list(s["cart_coords"], s["lattice"], 5.0)
        for pbc in ((True,), ((True, True, True),), ([1, 1, 1],))[k % 3]:
            a, b = graph.neighbor_list(s["cart_coords"], s["lattice"], 5.0, pbc=pbc)
            assert np.array_equal(a, c) and np.array_equal(b, d)
        a, b = graph.neighbor_list(s["cart_coords"], s["lattice"], 5.0)
        assert np.array_equal(a, c) and np.array_equal(b, d)


def test_molecule_equals_itself_in_a_large_periodic_box():
    from matten_amd.data import graph, synthetic

    for m in synthetic.molecules(4, seed=7):
        pos = m["cart_coords"]
        side = (pos.max(0) - pos.min(0)).max() + 5.0 + 0.5           # sides exceed extent + r_cut: no image in reach
        open_ = graph.neighbor_list(pos, None, 5.0, pbc=False)
        boxed = graph.neighbor_list(pos, side * np.eye(3), 5.0, pbc=True)
        assert np.array_equal(open_[0], boxed[0]) and np.array_equal(open_[1], boxed[1]) and not boxed[1].any()


def test_invalid_cells_and_edgeless_molecules_raise():
    from matten_amd.data import graph

    pos = np.array([[0.0, 0, 0], [1.0, 0, 0]])
    cell = np.diag([4.0, 4.0, 0.0])
    assert graph.neighbor_list(pos, cell, 5.0, pbc=(True, True, False))[0].shape[1] > 2
    with pytest.raises(ValueError):
        graph.neighbor_list(pos, cell, 5.0, pbc=(True, False, True))       # zero vector on a periodic axis
    with pytest.raises(ValueError):
        graph.neighbor_list(pos, cell, 5.0, pbc=True)
    with pytest.raises(ValueError):
        graph.neighbor_list(pos, None, 5.0, pbc=(False, False, True))
    with pytest.raises(ValueError):                                           # dependent periodic vectors
        graph.neighbor_list(pos, np.array([[4.0, 0, 0], [8.0, 0, 0], [0, 0, 4.0]]), 5.0, pbc=(True, True, False))
    with pytest.raises(ValueError):
        graph.neighbor_list(pos, cell, 5.0, pbc=(True, True))
    with pytest.raises(ValueError, match="no edges remain"):                  # reference data/data.py:398-402
        graph.neighbor_list(np.zeros((1, 3)), None, 5.0, pbc=False)
    with pytest.raises(ValueError, match="no edges remain"):
        graph.neighbor_list(np.array([[0.0, 0, 0], [9.0, 0, 0]]), None, 5.0, pbc=False)


def test_completed_cell_bounds_are_those_of_the_periodic_sublattice():
    from matten_amd.data import graph

    rng = np.random.default_rng(5)
    for pbc in FLAGS:
        _, cell = triclinic(rng, 2)
        done = graph.complete_cell(cell, pbc)
        per = np.array(pbc)
        assert np.array_equal(done[per], cell[per])
        assert np.allclose(done[~per] @ done[per].T, 0.0, atol=1e-12)
        assert np.allclose(np.linalg.norm(done[~per], axis=1), 1.0)
        vol = graph.periodic_volume(cell[None], per[None])[0]
        assert np.isclose(abs(np.linalg.det(done)), vol)
    assert graph.periodic_volume(np.zeros((1, 3, 3)), np.array([[False] * 3]))[0] == 1.0
    assert graph.periodic_volume(np.diag([3.0, 0, 2.0])[None], np.array([[True, True, False]]))[0] == 0.0


def test_pack_structures_keeps_open_structures_and_its_six_tuple():
    from matten_amd import predict as P
    from matten_amd.data import synthetic

    class Lattice:
        matrix = 6.0 * np.eye(3)
        pbc = (True, True, False)          # ignored: an object with .lattice is fully periodic, as in the reference

    class Site:
        def __init__(self, s, lattice):
            self.cart_coords, self.atomic_numbers = s["cart_coords"], s["atomic_numbers"]
            if lattice:
                self.lattice = Lattice()

    mols = synthetic.molecules(3)
    slab = synthetic.fcc_slabs(1, vacuum_vector=False)[0]
    crystal = synthetic.fcc64_structures(1)[0]
    zero = dict(mols[0], lattice=np.zeros((3, 3)))                       # zero cell, flagged open
    no_flag = {k: v for k, v in mols[1].items() if k != "pbc"}           # no lattice, no flag: open
    bad = dict(crystal, lattice=np.zeros((3, 3)))                        # zero cell on periodic axes: skipped
    bad_slab = dict(slab, pbc=(True, False, True))
    items = [crystal, zero, no_flag, slab, bad, Site(mols[2], False), Site(mols[2], True), bad_slab]
    with pytest.warns(UserWarning, match="Failed converting structure"):
        out = P.pack_structures(items)
    assert len(out) == 6
    pos, cell, Z, ptr, keep, failed = out
    assert keep == [0, 1, 2, 3, 5, 6] and failed == [4, 7] and len(ptr) == 7
    assert not cell[1].any() and not cell[2].any() and not cell[4].any() and np.array_equal(cell[5], 6.0 * np.eye(3))
    with pytest.warns(UserWarning):
        out7 = P.pack_structures(items, with_pbc=True)
    assert len(out7) == 7 and all(np.array_equal(a, b) for a, b in zip(out7[:4], out[:4]))
    assert out7[6].tolist() == [[True] * 3, [False] * 3, [False] * 3, [True, True, False], [False] * 3, [True] * 3]
    # fully periodic input: the vectorised packer as before, no flags
    st = synthetic.fcc64_structures(3)
    assert len(P.pack_structures(st)) == 6 and P.pack_structures(st, with_pbc=True)[6] is None
    assert P._pack_fast(st) is not None and P._pack_fast(st + [slab]) is None and P._pack_fast(st + [no_flag]) is None
    # the override applies to every structure
    forced = P.pack_structures(st[:1] + [slab], with_pbc=True, pbc=False)
    assert forced[6].tolist() == [[False] * 3] * 2
    graphs, failed = P.build_graphs(items, 5.0, on_gpu=True)
    assert failed == [4, 7] and [len(g) for g in graphs] == [3, 4, 4, 4, 4, 3]
    graphs, failed = P.build_graphs([mols[0], slab, bad], 5.0)
    assert failed == [2] and not graphs[0]["edge_cell_shift"].any() and not graphs[1]["edge_cell_shift"][:, 2].any()
    import inspect

    assert inspect.signature(P.evaluate_soa).parameters["pbc"].kind is inspect.Parameter.KEYWORD_ONLY
    assert "pbc" in inspect.signature(P.predict).parameters


def _molecule_record(m, symbols):
    return {"@module": "pymatgen.core.structure", "@class": "Molecule", "charge": 0, "spin_multiplicity": 1,
            "sites": [{"name": symbols[int(z)], "species": [{"element": symbols[int(z)], "occu": 1}], "xyz": list(map(float, x)),
                       "properties": {}} for x, z in zip(m["cart_coords"], m["atomic_numbers"])]}


def test_json_molecule_records_and_the_data_module(tmp_path, golden_dir):
    from matten_amd.data import graph, io, synthetic
    from matten_amd.dataset.structure_scalar_tensor import TensorDataModule

    symbols = {z: s for s, z in io.ATOMIC_NUMBER.items()}
    mols = synthetic.molecules(3)
    table = {"structure": {str(k): _molecule_record(m, symbols) for k, m in enumerate(mols)},
             "nmr": {str(k): np.eye(3).tolist() for k in range(len(mols))}}
    path = tmp_path / "molecules.json"
    path.write_text(json.dumps(table))
    rows = io.structures_from_json(str(path), target_columns=("nmr",))
    assert len(rows) == 3
    for r, m in zip(rows, mols):
        assert "lattice" not in r and r["pbc"] == (False, False, False)
        assert np.array_equal(r["cart_coords"], m["cart_coords"]) and np.array_equal(r["atomic_numbers"], m["atomic_numbers"])
    dm = TensorDataModule(str(path), str(path), str(path), r_cut=5.0, tensor_target_name="nmr", tensor_target_formula="ij=ji")
    dm.setup()
    for g, m in zip(dm.train_data, mols):
        want = graph.neighbor_list(m["cart_coords"], None, 5.0, pbc=False)
        assert torch.equal(g["edge_index"], torch.as_tensor(want[0])) and not g["edge_cell_shift"].any()

    # Structure records stay fully periodic unless asked; TensorDataModule(pbc=...) applies to every structure loaded
    crystal = os.path.join(golden_dir, "elastic_tensor_one.json")
    rec = json.load(open(crystal))
    row = io.structures_from_json(crystal)[0]
    assert "pbc" not in row
    key = next(iter(rec["structure"]))
    rec["structure"][key]["lattice"]["pbc"] = [True, True, False]
    (tmp_path / "slab.json").write_text(json.dumps(rec))
    assert "pbc" not in io.structures_from_json(str(tmp_path / "slab.json"))[0]
    assert io.structures_from_json(str(tmp_path / "slab.json"), honor_lattice_pbc=True)[0]["pbc"] == (True, True, False)
    for pbc in (None, (True, True, False), False):
        dm = TensorDataModule(crystal, crystal, crystal, r_cut=5.0, tensor_target_name="elastic_tensor_full", pbc=pbc)
        dm.setup()
        g = dm.train_data[0]
        flags = (True,) * 3 if pbc is None else graph.normalize_pbc(pbc)
        want = graph.neighbor_list(row["cart_coords"], row["lattice"], 5.0, pbc=flags)
        assert torch.equal(g["edge_index"], torch.as_tensor(want[0]))
        assert torch.equal(g["edge_cell_shift"], torch.as_tensor(want[1], dtype=torch.float32))
        assert all(bool(g["edge_cell_shift"][:, k].any()) == flags[k] for k in range(3))


def test_library_exports_the_new_entries():
    from matten_amd import _lib

    lib = _lib.load()
    for name in ("matten_graph_prep_pbc", "matten_neighbor_rows_count", "matten_neighbor_rows_fill"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.ABI_VERSION == 47 and lib.matten_abi_version() == 47
    # host-detectable argument errors, no GPU touched
    assert lib.matten_graph_prep_pbc(None, None, None, None, 1, 5.0, None, None, None, None, None, None, None, None) == -1
    assert lib.matten_neighbor_rows_count(None, None, None, None, None, None, 5.0, 3, None, None) == -1
    assert lib.matten_neighbor_rows_fill(None, None, None, None, None, None, 0.0, 0, None, 0, None, None, None, None) == -1
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "matten_hip.h")).read()
    assert header.count("data/data.py:285-413") >= 3


def test_large_inputs_of_existing_runs_stay_on_the_pair_route(golden_dir):
    """the routing threshold sits above every structure the suite, smoke() and the benchmark build graphs of"""
    from matten_amd.data import graph, synthetic
    from oracle.matten_ref import data as rdata

    structs = rdata.structures_from_json(os.path.join(golden_dir, "example_crystal_elasticity_tensor_n100.json"))
    structs += rdata.structures_from_json(os.path.join(golden_dir, "elastic_tensor_one.json")) + synthetic.fcc64_structures(2)
    largest = max(len(s["atomic_numbers"]) for s in structs)   # every structure file and generator the suite, smoke() and
    assert largest == 64                                       # the benchmark build graphs of: fcc-64 is the largest
    assert largest < graph.rows_min_atoms() == 2048
    c = synthetic.fcc_cluster(500)
    assert c["cart_coords"].shape == (500, 3) and np.array_equal(c["cart_coords"], synthetic.fcc_cluster(500)["cart_coords"])
