"""
Host tests of the cells route of the device graph builder (no GPU): the entries of the library, the route selection and
the pruning rule of the cell list, checked on its numpy restatement ``graph.cell_grid_host`` against the host builder.
"""
import os

import numpy as np
import pytest

CELLS_ENTRIES = ("matten_neighbor_cells_row_capacity", "matten_neighbor_cells_max_axis_bins", "matten_neighbor_cells_grid",
                 "matten_neighbor_cells_bin", "matten_neighbor_cells_scatter", "matten_neighbor_cells_count",
                 "matten_neighbor_cells_fill")


def test_library_exports_the_cells_entries():
    from matten_amd import _lib, ops
    from matten_amd.data import graph

    lib = _lib.load()
    for name in CELLS_ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 47 == lib.matten_abi_version()
    assert callable(ops.neighbor_list_cells)
    cap = lib.matten_neighbor_cells_row_capacity()
    assert cap >= 64 and 4 * 8 * cap <= 64 * 1024   # four waves of (j, count) records fit the LDS of a block
    assert lib.matten_neighbor_cells_max_axis_bins() == graph.CELLS_MAX_NB   # the kernel's clamp and its numpy restatement
    # host-detectable argument errors, no GPU touched
    assert lib.matten_neighbor_cells_grid(None, None, None, None, None, None, 1, 5.0, None, None, None, None) == -1
    assert lib.matten_neighbor_cells_grid(None, None, None, None, None, None, 0, 0.0, None, None, None, None) == -1
    assert lib.matten_neighbor_cells_bin(None, None, None, None, None, None, 3, None, None, None) == -1
    assert lib.matten_neighbor_cells_scatter(None, None, None, None, 1 << 31, None, None, None) == -1
    assert lib.matten_neighbor_cells_count(None, None, None, None, None, None, None, None, None, None, None, 5.0, 3, None,
                                           None) == -1
    assert lib.matten_neighbor_cells_fill(None, None, None, None, None, None, None, None, None, None, None, 0.0, 0, None, 0,
                                          None, None, None, None) == -1
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "matten_hip.h")).read()
    assert header.count("data/data.py:285-413") >= 4
    assert all(header.count("int " + name + "(") == 1 for name in CELLS_ENTRIES)


def test_search_route_under_the_two_switches(monkeypatch):
    from matten_amd.data import graph

    monkeypatch.delenv("MATTEN_NEIGHBOR_ROWS_MIN_ATOMS", raising=False)
    monkeypatch.delenv("MATTEN_NEIGHBOR_CELLS_MIN_ATOMS", raising=False)
    assert graph.search_route(64) == "pair" and graph.search_route(graph.rows_min_atoms() - 1) == "pair"
    assert graph.cells_min_atoms() >= 2048 and graph.cells_min_atoms() & (graph.cells_min_atoms() - 1) == 0
    assert graph.search_route(max(graph.rows_min_atoms(), graph.cells_min_atoms())) == "cells"
    assert graph.search_route(10 ** 6) == "cells"
    monkeypatch.setenv("MATTEN_NEIGHBOR_ROWS_MIN_ATOMS", "1")           # rows alone: small batches take the rows route
    assert graph.search_route(1) == "rows" and graph.search_route(64) == "rows"
    assert graph.search_route(graph.cells_min_atoms() - 1) == "rows" and graph.search_route(graph.cells_min_atoms()) == "cells"
    monkeypatch.setenv("MATTEN_NEIGHBOR_CELLS_MIN_ATOMS", "1")          # both: everything takes the cells route
    assert graph.search_route(1) == "cells" and graph.search_route(10 ** 5) == "cells"
    monkeypatch.delenv("MATTEN_NEIGHBOR_ROWS_MIN_ATOMS")                # cells alone: the rows bound still holds
    assert graph.search_route(64) == "pair" and graph.search_route(graph.rows_min_atoms() - 1) == "pair"
    assert graph.search_route(graph.rows_min_atoms()) == "cells"
    monkeypatch.setenv("MATTEN_NEIGHBOR_CELLS_MIN_ATOMS", str(10 ** 12))   # a huge value switches the route off
    assert graph.search_route(10 ** 6) == "rows" and graph.search_route(64) == "pair"
    monkeypatch.setenv("MATTEN_NEIGHBOR_ROWS_MIN_ATOMS", str(10 ** 12))
    assert graph.search_route(10 ** 6) == "pair"


def _raw_bins(cell, pbc, r_cut):
    from matten_amd.data.graph import complete_cell

    inv = np.linalg.inv(complete_cell(cell, pbc))
    return [int(1.0 / (r_cut * np.linalg.norm(inv[:, k]) * (1.0 + 1e-6))) for k in range(3)]


def _random_structure(rng, kind):
    """(pos, cell, pbc): a triclinic cell of 6-16 A edges filled at about fcc density, atoms moved out of the cell by
    random lattice vectors; slabs and wires keep their open rows (which generate nothing), clusters have no cell"""
    cell = np.diag(rng.uniform(6.0, 16.0, 3)) + rng.uniform(-2.0, 2.0, (3, 3))
    n = int(rng.integers(20, 90))
    frac = rng.uniform(0.0, 1.0, (n, 3))
    pbc = {"crystal": (True, True, True), "slab": (True, True, False), "wire": (False, False, True),
           "cluster": (False, False, False), "slab_y": (True, False, True)}[kind]
    hop = rng.integers(-2, 3, (n, 3)) * np.array(pbc)
    pos = (frac + hop) @ cell
    if kind == "cluster":
        return pos * rng.uniform(0.5, 2.0), None, pbc
    return pos, cell, pbc


@pytest.mark.parametrize("kind", ["crystal", "slab", "wire", "cluster", "slab_y"])
def test_pruning_by_the_cell_grid_loses_no_edge(kind):
    """every edge (i, j, S) of the host builder joins atoms whose bins differ by at most one per axis: modulo nb on a
    periodic axis, without wrap on an open one; an axis of one or two raw bins reports one; never more bins than atoms"""
    from matten_amd.data.graph import cell_grid_host, neighbor_list

    rng = np.random.default_rng({"crystal": 1, "slab": 2, "wire": 3, "cluster": 4, "slab_y": 5}[kind])
    seen_grid = seen_collapse = 0
    for _ in range(6):
        pos, cell, pbc = _random_structure(rng, kind)
        for r_cut in (2.5, 4.0, 5.0):
            nb, flat = cell_grid_host(pos, cell, pbc, r_cut)
            assert nb.shape == (3,) and flat.shape == (len(pos),) and int(nb.min()) >= 1
            assert int(np.prod(nb)) <= len(pos) and 0 <= int(flat.min()) and int(flat.max()) < int(np.prod(nb))
            bins = np.stack([flat // (nb[1] * nb[2]), (flat // nb[2]) % nb[1], flat % nb[2]], 1)
            if cell is not None:
                raw = _raw_bins(cell, pbc, r_cut)
                for k in range(3):
                    if pbc[k]:
                        assert nb[k] <= raw[k] and nb[k] != 2
                        if raw[k] in (1, 2):
                            assert nb[k] == 1
                            seen_collapse += 1
            try:
                edge_index, _ = neighbor_list(pos, cell, r_cut, pbc)
            except ValueError:       # no edge at this cutoff: nothing to lose
                continue
            d = bins[edge_index[1]] - bins[edge_index[0]]
            for k in range(3):
                if pbc[k]:
                    m = np.mod(d[:, k], nb[k])
                    assert bool(((m <= 1) | (m == nb[k] - 1)).all()), (kind, r_cut, k, nb)
                else:
                    assert int(np.abs(d[:, k]).max()) <= 1, (kind, r_cut, k, nb)
                seen_grid += int(nb[k] >= 3)
    assert seen_grid > 0 and (kind == "cluster" or seen_collapse > 0)


def test_the_grids_the_gpu_cases_rely_on():
    from matten_amd.data import synthetic
    from matten_amd.data.graph import cell_grid_host

    s = synthetic.fcc_supercell(3, 4, 5)
    assert s["cart_coords"].shape == (240, 3) and s["lattice"].shape == (3, 3) and set(s) == set(synthetic.fcc_cluster(8)) | {"lattice"}
    assert np.array_equal(s["cart_coords"], synthetic.fcc_supercell(3, 4, 5)["cart_coords"])
    bound = 4.0 * np.linalg.norm(np.linalg.inv(s["lattice"]), axis=0)
    assert np.allclose(bound, [0.329, 0.247, 0.198], atol=5e-4)
    assert cell_grid_host(s["cart_coords"], s["lattice"], True, 4.0)[0].tolist() == [3, 4, 5]
    sheared = synthetic.fcc_supercell(3, 4, 5, shear=[[0, 0.1, 0.05], [0, 0, -0.08], [0, 0, 0]])
    assert np.count_nonzero(sheared["lattice"]) == 6
    assert cell_grid_host(sheared["cart_coords"], sheared["lattice"], True, 4.0)[0].tolist() == [3, 4, 5]
    cube = synthetic.fcc_supercell(4, 4, 4, jitter=0)
    assert cell_grid_host(cube["cart_coords"], cube["lattice"], True, 4.0)[0].tolist() == [4, 4, 4]
    assert cell_grid_host(synthetic.fcc64_structures(1)[0]["cart_coords"], synthetic.fcc64_structures(1)[0]["lattice"], True,
                          5.0)[0].tolist() == [1, 1, 1]
    ball = synthetic.fcc_cluster(300)
    nb, flat = cell_grid_host(ball["cart_coords"], None, False, 5.0)
    assert int(nb.min()) >= 3 and len(np.unique(flat)) < int(np.prod(nb))     # the corner bins of the ball's box are empty
