"""
GPU tests of the cells route of the device graph builder (matten_neighbor_cells_*: the rows search behind a cell list).
Every case compares the forced cells route with the host builder and with the rows route on the same batch, bit for
bit (torch.equal, no tolerance).  The grids the cases rely on are asserted on the host restatement
(graph.cell_grid_host; tests/test_cells_host.py checks its pruning rule), and test_g0 holds the grid and the bins that
the device builds equal to that restatement.
"""
import numpy as np
import pytest
import torch

from common import LMAX2, build_pair
from test_gpu_pbc import OPEN, SLAB, _assert_same_graph, _host, _item, _mixed

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WIRE_Z = (False, False, True)


def _build(items, r_cut, route, monkeypatch):
    from matten_amd.data.graph import batch_graphs_gpu, search_route

    monkeypatch.setenv("MATTEN_NEIGHBOR_ROWS_MIN_ATOMS", "1")
    monkeypatch.setenv("MATTEN_NEIGHBOR_CELLS_MIN_ATOMS", "1" if route == "cells" else str(10 ** 12))
    assert search_route(max(len(it[0]) for it in items)) == route
    return batch_graphs_gpu(items, r_cut, DEV)


def _check(items, r_cut, monkeypatch):
    """cells route == host builder == rows route; -> (the cells batch, the host batch)"""
    from matten_amd.data.graph import collate

    want = collate(_host(items, r_cut))
    cells = _build(items, r_cut, "cells", monkeypatch)
    _assert_same_graph(cells, want, csr=False)
    rows = _build(items, r_cut, "rows", monkeypatch)
    assert set(rows) == set(cells)
    for k in rows:
        assert torch.equal(rows[k], cells[k]), k
    return cells, want


def _grid(item, r_cut):
    from matten_amd.data.graph import cell_grid_host

    return cell_grid_host(item[0], item[1], item[3], r_cut)[0].tolist()


def test_g0_device_grid_and_bins_are_those_of_the_host_restatement():
    """matten_neighbor_cells_grid / _bin called directly on one batch: bins per axis and the bin of every atom equal
    cell_grid_host's -- a wrapping grid (plain, sheared), a collapsed axis beside gridded ones (crystal, slab, wire), open
    balls with a real grid (the stretched one has 7^3 raw bins for 300 atoms, so one axis is halved), an fcc-64 cell of one bin.
    The list of the cells route equals the others' even on a collapsed or over-coarse grid, so only this test sees one."""
    from matten_amd import _lib, ops
    from matten_amd.data import synthetic
    from matten_amd.data.graph import cell_grid_host, normalize_pbc

    r_cut = 4.0
    ball = synthetic.fcc_cluster(300)
    items = [_item(synthetic.fcc_supercell(3, 4, 5)),
             _item(synthetic.fcc_supercell(3, 4, 5, shear=[[0, 0.1, 0.05], [0, 0, -0.08], [0, 0, 0]])),
             _item(ball), _item(synthetic.fcc_supercell(5, 5, 1)), _item(synthetic.fcc_supercell(5, 5, 1), SLAB),
             _item(synthetic.fcc_supercell(1, 1, 8), WIRE_Z), _item(synthetic.fcc64_structures(1)[0]),
             _item(dict(ball, cart_coords=ball["cart_coords"] * (4.0 / 3.0)))]     # sparse: more raw bins than atoms
    want = [cell_grid_host(it[0], it[1], it[3], r_cut) for it in items]
    assert [w[0].tolist() for w in want[:2]] == [[3, 4, 5]] * 2 and [w[0].tolist() for w in want[3:7]] == [
        [5, 5, 1], [5, 5, 1], [1, 1, 8], [1, 1, 1]]
    assert int(want[2][0].min()) >= 3 and int(want[7][0].min()) >= 3
    span = np.ptp(items[7][0], axis=0) / (r_cut * (1.0 + 1e-6))
    assert int(np.prod(np.floor(span) + 1)) > 300 >= int(np.prod(want[7][0]))      # coarsened by the cap at the atom count

    sizes = [len(it[0]) for it in items]
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64, device=DEV)
    pos = torch.tensor(np.concatenate([it[0] for it in items]), dtype=torch.float64, device=DEV)
    cell = torch.tensor(np.stack([np.zeros((3, 3)) if it[1] is None else it[1] for it in items]).reshape(-1, 9),
                        dtype=torch.float64, device=DEV)
    pbc = torch.tensor(np.array([normalize_pbc(it[3]) for it in items]), dtype=torch.uint8, device=DEV)
    B, N = len(items), int(ptr[-1])
    n_singular = torch.zeros(1, dtype=torch.int64, device=DEV)
    frac, bound, batch, _, _, singular = ops.graph_prep_pbc(pos, cell, ptr, pbc, r_cut, n_singular)
    lib, P, st = _lib.load(), ops._ptr, ops._stream()
    grid = torch.full((B, 8), -1, dtype=torch.int32, device=DEV)
    grid_f = torch.zeros(B, 16, dtype=torch.float64, device=DEV)
    n_bins = torch.zeros(B, dtype=torch.int64, device=DEV)
    _lib.check(lib.matten_neighbor_cells_grid(P(pos), P(cell), P(ptr), P(bound), P(pbc), P(singular), B, r_cut, P(grid),
                                              P(grid_f), P(n_bins), st), "matten_neighbor_cells_grid")
    bin_base = torch.zeros(B + 1, dtype=torch.int64, device=DEV)
    torch.cumsum(n_bins, 0, out=bin_base[1:])
    bin_of = torch.full((N,), -1, dtype=torch.int32, device=DEV)
    bin_count = torch.zeros(N + B, dtype=torch.int32, device=DEV)
    _lib.check(lib.matten_neighbor_cells_bin(P(pos), P(frac), P(batch), P(grid), P(grid_f), P(bin_base), N, P(bin_of),
                                             P(bin_count), st), "matten_neighbor_cells_bin")
    torch.cuda.synchronize()
    assert int(n_singular) == 0
    grid, n_bins, bin_of, bin_count, base = grid.cpu().numpy(), n_bins.cpu().numpy(), bin_of.cpu().numpy(), bin_count.cpu().numpy(), 0
    for b, (nb, flat) in enumerate(want):
        lo, hi = int(ptr[b]), int(ptr[b + 1])
        assert grid[b, :3].tolist() == nb.tolist(), (b, grid[b].tolist(), nb)
        assert grid[b, 3:6].tolist() == [0 if f else 1 for f in normalize_pbc(items[b][3])], b
        assert int(n_bins[b]) == int(np.prod(nb))
        assert np.array_equal(bin_of[lo:hi], flat), b
        assert np.array_equal(bin_count[base : base + int(n_bins[b])], np.bincount(flat, minlength=int(n_bins[b]))), b
        base += int(n_bins[b])
    assert int(bin_count[base:].sum()) == 0


def test_g1_mixed_batch_of_degenerate_grids(golden_dir, monkeypatch):
    """crystals, slabs, wires and molecules of at most 64 atoms at 5 A: one bin per structure on (nearly) every axis,
    several images per pair, an isolated atom, open rows of zeros"""
    items = _mixed(golden_dir, 3)
    _, want = _check(items, 5.0, monkeypatch)
    assert int((want["num_neigh"] == 0).sum()) == 1
    assert _grid(items[4], 5.0) == [1, 1, 1] and float(want["edge_cell_shift"].abs().max()) >= 1.0


@pytest.mark.parametrize("case", ["plain", "sheared", "unwrapped", "on_boundaries"])
def test_g2_periodic_grids_with_wrap(monkeypatch, case):
    """nb = (3, 4, 5): the first grid with distinct wrap-around neighbours, the first with a skipped bin, and one more;
    nb = (4, 4, 4) with every atom exactly on a bin boundary (frac = k / 8)"""
    from matten_amd.data import synthetic

    if case == "on_boundaries":
        s = synthetic.fcc_supercell(4, 4, 4, jitter=0)
        nb = [4, 4, 4]
    else:
        s = synthetic.fcc_supercell(3, 4, 5, a=4.05, shear=[[0, 0.1, 0.05], [0, 0, -0.08], [0, 0, 0]] if case == "sheared" else None)
        nb = [3, 4, 5]
        if case == "unwrapped":
            hop = np.random.default_rng(7).integers(-2, 3, (len(s["cart_coords"]), 3))
            s = dict(s, cart_coords=s["cart_coords"] + hop @ s["lattice"])
    item = _item(s)
    assert _grid(item, 4.0) == nb
    _, want = _check([item], 4.0, monkeypatch)
    assert bool(want["edge_cell_shift"].any(0).all())    # edges across every face of the cell


@pytest.mark.parametrize("case", ["crystal", "slab", "wire"])
def test_g3_collapsed_axis_beside_gridded_ones(monkeypatch, case):
    from matten_amd.data import synthetic

    if case == "wire":
        item, nb = _item(synthetic.fcc_supercell(1, 1, 8), WIRE_Z), [1, 1, 8]
    else:
        item, nb = _item(synthetic.fcc_supercell(5, 5, 1), True if case == "crystal" else SLAB), [5, 5, 1]
    assert _grid(item, 4.0) == nb
    _, want = _check([item], 4.0, monkeypatch)
    sz = want["edge_cell_shift"][:, 2]
    if case == "crystal":
        assert float(sz.min()) == -1.0 and float(sz.max()) == 1.0     # one bin along z, images S_z = +-1
    elif case == "slab":
        assert not bool(sz.any())
    else:
        assert bool(sz.any()) and not bool(want["edge_cell_shift"][:, :2].any())


@pytest.mark.parametrize("r_cut", [3.0, 5.0, 6.5])
def test_g4_open_cluster(monkeypatch, r_cut):
    """a ball of 300 atoms: a real grid on three open axes, empty corner bins; at 6.5 A rows of 78 edges (more than a wave)"""
    from matten_amd.data import synthetic
    from matten_amd.data.graph import cell_grid_host

    item = _item(synthetic.fcc_cluster(300))
    nb, flat = cell_grid_host(item[0], None, OPEN, r_cut)
    assert int(nb.min()) >= 3 and len(np.unique(flat)) < int(np.prod(nb))
    _, want = _check([item], r_cut, monkeypatch)
    if r_cut == 6.5:
        assert int(want["num_neigh"].max()) == 78


def test_g5_crowded_bins(monkeypatch):
    """fcc_cluster(2000) at 12 A: about a hundred atoms per bin, rows of about 430 edges, still within the record buffer"""
    from matten_amd import ops
    from matten_amd.data import synthetic
    from matten_amd.data.graph import cell_grid_host

    item = _item(synthetic.fcc_cluster(2000))
    nb, flat = cell_grid_host(item[0], None, OPEN, 12.0)
    assert int(np.bincount(flat).max()) >= 100
    _, want = _check([item], 12.0, monkeypatch)
    longest = int(want["num_neigh"].max())
    print(f"longest row {longest}, capacity {ops.neighbor_cells_row_capacity()}")
    assert 400 <= longest <= ops.neighbor_cells_row_capacity()


def test_g5_rows_longer_than_the_record_buffer(monkeypatch):
    """fcc_cluster(1200) at 13.5 A: the fill pass ranks at most 512 (j, count) records per row in LDS
    (matten_neighbor_cells_row_capacity); the inner atoms of this ball have more than 600 neighbours, each a distinct j,
    so their rows take the fallback (the rows walk over the whole structure) while the rows of the rim do not"""
    from matten_amd import ops
    from matten_amd.data import synthetic

    cap = ops.neighbor_cells_row_capacity()
    assert cap == 512
    item = _item(synthetic.fcc_cluster(1200))
    _, want = _check([item], 13.5, monkeypatch)
    assert int(want["num_neigh"].max()) > cap > int(want["num_neigh"].min())
    assert not bool(want["edge_cell_shift"].any())     # open: an edge per neighbouring atom, so row length = records


def test_g6_mixed_grids_in_one_batch_twice(monkeypatch):
    """bin offsets across structures and mixed grids; the second build equals the first bitwise"""
    from matten_amd.data import synthetic

    items = [_item(s) for s in synthetic.fcc64_structures(20)]
    items.insert(7, _item(synthetic.fcc_cluster(600)))
    items.insert(15, _item(synthetic.fcc_supercell(3, 4, 5)))
    mols = [_item(m) for m in synthetic.molecules(3, seed=5)]
    items = mols[:1] + items + mols[1:]
    first, _ = _check(items, 5.0, monkeypatch)
    again = _build(items, 5.0, "cells", monkeypatch)
    for k in first:
        assert torch.equal(first[k], again[k]), k


def test_g7_memory_on_a_large_cluster(monkeypatch):
    """fcc_cluster(8000) on the forced cells route: the peak of the build above what it returns stays below 1 KB per atom"""
    from matten_amd.data import synthetic
    from matten_amd.data.graph import batch_graphs_gpu, collate, crystal_graph

    n = 8000
    item = _item(synthetic.fcc_cluster(n))
    _build([_item(synthetic.molecules(1)[0])], 5.0, "cells", monkeypatch)            # library and allocator warm
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    got = batch_graphs_gpu([item], 5.0, DEV)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    returned = sum(t.numel() * t.element_size() for t in got.values())
    print(f"cells route, {n} atoms: peak {peak} B, returned {returned} B, scratch {(peak - returned) / n:.1f} B per atom")
    assert peak - returned < 1024 * n
    assert not any(k.startswith("_amd_") for k in got)
    want = collate([crystal_graph(item[0], None, item[2], 5.0, pbc=False)])
    _assert_same_graph(got, want, csr=False)


def test_g8_errors_and_predict_go_through_the_cells_route(monkeypatch):
    from matten_amd import predict as P
    from matten_amd.data import synthetic
    from matten_amd.data.graph import EdgelessStructures, SingularCells, batch_graphs_gpu

    sup, ball = synthetic.fcc_supercell(3, 4, 5), synthetic.fcc_cluster(300)
    monkeypatch.setenv("MATTEN_NEIGHBOR_ROWS_MIN_ATOMS", "1")
    monkeypatch.setenv("MATTEN_NEIGHBOR_CELLS_MIN_ATOMS", "1")
    lone = (np.zeros((1, 3)), None, np.array([29]), OPEN)
    with pytest.raises(EdgelessStructures) as e:
        batch_graphs_gpu([_item(sup), lone, _item(ball)], 5.0, DEV)
    assert e.value.indices == [1]
    slab = synthetic.fcc_slabs(1)[0]
    bad = (slab["cart_coords"], np.array([[4.0, 0, 0], [8.0, 0, 0], [0, 0, 9.0]]), slab["atomic_numbers"], SLAB)
    with pytest.raises(SingularCells) as e:
        batch_graphs_gpu([_item(ball), _item(sup), bad, _item(slab)], 5.0, DEV)
    assert e.value.indices == [2]

    ds = {"allowed_species": list(synthetic.FCC_METALS), "average_num_neighbors": 40.0}
    _, model = build_pair(dict(LMAX2), ds, randomize_bn=True)
    cfg = {"data": {"r_cut": 5.0, "tensor_target_name": "elastic_tensor_full", "tensor_target_formula": "ijkl=jikl=klij"}}
    on = P.predict([sup, ball], model=model, config=cfg, is_elasticity_tensor=False)
    monkeypatch.setenv("MATTEN_NEIGHBOR_CELLS_MIN_ATOMS", str(10 ** 12))
    off = P.predict([sup, ball], model=model, config=cfg, is_elasticity_tensor=False)
    assert len(on) == len(off) == 2 and on[0].shape == (3, 3, 3, 3)
    assert all(np.array_equal(a, b) for a, b in zip(on, off)) and float(np.abs(on[0]).max()) > 0


def test_g9_pair_rows_cells_and_capped_routes_on_one_batch(monkeypatch):
    """The four search routes on ONE batch, each against the host builder and the CSR of the pair route against the
    capped one: a 2-atom Si primitive cell (56 edges over 4 ordered pairs: several images per pair), fcc_supercell(3, 4, 5)
    with a = 5.2 (240 atoms: four wave chunks and a running base on the rows route; at the default a = 4.05 the grid at
    5 A would be [1, 3, 4], at 5.2 it is [3, 4, 5]) and a slab (open z).  The capped buffers hold 5 edges, 3 atoms and
    2 crystals more than the list; their real prefix is compared."""
    from matten_amd.data import synthetic
    from matten_amd.data._key import AMD_N_VALID, AMD_PERM, AMD_ROWPTR, AMD_SRC
    from matten_amd.data.graph import batch_graphs_gpu, collate, neighbor_list, normalize_pbc
    from matten_amd.data.rebuild import GeometryBatch

    r_cut, a = 5.0, 5.43
    si = {"lattice": 0.5 * a * np.array([[0.0, 1, 1], [1, 0, 1], [1, 1, 0]]), "atomic_numbers": np.array([14, 14]),
          "cart_coords": np.array([[0.0, 0.0, 0.0], [0.25 * a] * 3])}
    items = [_item(si), _item(synthetic.fcc_supercell(3, 4, 5, a=5.2)), _item(synthetic.fcc_slabs(1)[0])]
    # the case is the one intended (host only)
    assert [len(it[0]) for it in items] == [2, 240, 54] and normalize_pbc(items[2][3]) == SLAB
    assert _grid(items[1], r_cut) == [3, 4, 5]
    counts = [neighbor_list(p, c, r_cut, f)[0].shape[1] for p, c, _, f in items]
    assert counts[0] == 56 and min(counts) > 0
    want = collate(_host(items, r_cut))
    N, E = int(want["pos"].shape[0]), int(want["edge_index"].shape[1])
    assert E == sum(counts)

    monkeypatch.delenv("MATTEN_NEIGHBOR_ROWS_MIN_ATOMS", raising=False)
    monkeypatch.delenv("MATTEN_NEIGHBOR_CELLS_MIN_ATOMS", raising=False)
    pair = batch_graphs_gpu(items, r_cut, DEV)
    _assert_same_graph(pair, want)
    ptr = np.concatenate([[0], np.cumsum([len(it[0]) for it in items])])
    gb = GeometryBatch(np.concatenate([it[0] for it in items]), np.stack([it[1] for it in items]),
                       np.concatenate([it[2] for it in items]), ptr, r_cut, DEV,
                       pbc=np.array([normalize_pbc(it[3]) for it in items]), edge_capacity=E + 5, pad_nodes=3, pad_crystals=2)
    assert gb.capacity == (N + 3, E + 5, 5) and gb.batch[AMD_N_VALID].tolist() == [N, E, 3]
    capped = {"edge_index": gb.batch["edge_index"][:, :E], "edge_cell_shift": gb.batch["edge_cell_shift"][:E],
              "num_neigh": gb.batch["num_neigh"][:N]}
    lists = {"pair": pair, "capped": capped, "rows": _build(items, r_cut, "rows", monkeypatch),
             "cells": _build(items, r_cut, "cells", monkeypatch)}
    for route, got in lists.items():
        for k in ("edge_index", "edge_cell_shift", "num_neigh"):
            assert got[k].dtype == want[k].dtype and torch.equal(got[k].cpu(), want[k]), (route, k)
    _assert_same_graph(lists["rows"], want, csr=False)
    _assert_same_graph(lists["cells"], want, csr=False)
    assert torch.equal(gb.batch[AMD_PERM][:E], pair[AMD_PERM]) and torch.equal(gb.batch[AMD_SRC][:E], pair[AMD_SRC])
    assert torch.equal(gb.batch[AMD_ROWPTR][:N + 1], pair[AMD_ROWPTR])
