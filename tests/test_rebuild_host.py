"""
Host tests of the sync-free edge-list rebuild (no GPU): the entries of the library and their argument checks, the public
symbols, the capacity rule and every refusal of ``GeometryBatch`` that is decided before the device is touched.
"""
import os

import numpy as np
import pytest

from rebuild_cases import fixture_crystals, host_graphs

CAPPED_ENTRIES = ("matten_neighbor_scan", "matten_neighbor_fill_capped")


def test_fixture_edge_counts():
    """the counts the GPU tests rely on (crystal_graph on the CPU); only the third crystal's count moves"""
    want = {0.94: 302, 0.97: 294, 1.00: 270, 1.03: 260, 1.06: 252}
    for scale, total in want.items():
        counts = [g["edge_index"].shape[1] for g in host_graphs(*fixture_crystals(scale))]
        assert sum(counts) == total and counts[:2] == [26, 56], (scale, counts)


def test_library_exports_the_capped_entries():
    from matten_amd import _lib, graphs, ops, predict
    from matten_amd.data import rebuild

    lib = _lib.load()
    for name in CAPPED_ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 47 == lib.matten_abi_version()   # entries were only added
    assert callable(ops.neighbor_list_capped) and callable(predict.evaluate_frames)
    assert isinstance(rebuild.GeometryBatch, type) and isinstance(graphs.GraphedGeometryStep, type)
    assert issubclass(rebuild.EdgeCapacityExceeded, ValueError)
    e = rebuild.EdgeCapacityExceeded(302, 296)
    assert "302" in str(e) and "296" in str(e) and (e.n_edges, e.capacity) == (302, 296)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "matten_hip.h")).read()
    assert all(header.count("int " + name + "(") == 1 for name in CAPPED_ENTRIES)
    for name in CAPPED_ENTRIES:   # each entry cites the reference's builder, like its siblings
        assert name + " (reference data/data.py:285-413" in header, name
    assert (rebuild.FLAG_OVERFLOW, rebuild.FLAG_EDGELESS, rebuild.FLAG_SINGULAR) == (1, 2, 4)
    for name, bit in (("OVERFLOW", 1), ("EDGELESS", 2), ("SINGULAR", 4)):
        assert f"#define MATTEN_CAPPED_{name} {bit}\n" in header


def _fill_capped(lib, **kw):
    """matten_neighbor_fill_capped with host-detectable argument errors only: fake non-NULL pointers, nothing is launched
    when the call is refused"""
    p = 4096   # never dereferenced on the host
    a = dict(pos=p, cell=p, ptr=p, frac=p, bound=p, pair_ptr=p, r_cut=5.0, n_crystals=3, max_atoms=5, offsets=p, offsets_t=p,
             n_atoms=8, singular=None, n_b=9, e_b=296, b_b=4, edge_index=p, shift=p, num_neigh=p, rowptr=p, src=p, perm=p,
             n_valid=p, flags=p)
    a.update(kw)
    return lib.matten_neighbor_fill_capped(a["pos"], a["cell"], a["ptr"], a["frac"], a["bound"], a["pair_ptr"], a["r_cut"],
                                           a["n_crystals"], a["max_atoms"], a["offsets"], a["offsets_t"], a["n_atoms"],
                                           a["singular"], a["n_b"], a["e_b"], a["b_b"], a["edge_index"], a["shift"],
                                           a["num_neigh"], a["rowptr"], a["src"], a["perm"], a["n_valid"], a["flags"], None)


@pytest.mark.parametrize("bad", [
    dict(b_b=3), dict(b_b=2), dict(n_b=8), dict(n_b=9, b_b=5), dict(e_b=1 << 31), dict(n_b=1 << 31), dict(b_b=1 << 31),
    dict(e_b=-1), dict(flags=None), dict(n_valid=None), dict(pos=None), dict(offsets=None), dict(offsets_t=None),
    dict(r_cut=0.0), dict(n_crystals=65536, b_b=65537), dict(n_crystals=-1), dict(max_atoms=-1), dict(edge_index=None),
    dict(perm=None), dict(rowptr=None), dict(num_neigh=None),
], ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_capped_fill_refuses_bad_arguments(bad):
    from matten_amd import _lib

    assert _fill_capped(_lib.load(), **bad) == -1
    assert _lib.load().matten_neighbor_scan(None, 4, None, None) == -1
    assert _lib.load().matten_neighbor_scan(None, 4, 4096, None) == -1
    assert _lib.load().matten_neighbor_scan(4096, -1, 4096, None) == -1


def test_capacity_rule():
    from matten_amd.data.rebuild import edge_capacity_for, plan_capacity

    assert edge_capacity_for(270) == 384                  # 64 * ceil(1.25 * 270 / 64)
    assert edge_capacity_for(256, 1.0) == 256 and edge_capacity_for(257, 1.0) == 320
    assert plan_capacity(8, 3, 270) == (9, 384, 4)
    assert plan_capacity(8, 3, 270, edge_capacity=270) == (9, 270, 4)
    assert plan_capacity(8, 3, 270, edge_capacity=296, pad_nodes=3, pad_crystals=2) == (11, 296, 5)


def test_construction_refusals(monkeypatch):
    """every refusal names its limit and is raised before the device is touched (this test has no GPU)"""
    from matten_amd.data import graph
    from matten_amd.data.rebuild import GeometryBatch, plan_capacity

    pos, cell, Z, ptr = fixture_crystals()
    # a capacity below the construction geometry's edge count
    with pytest.raises(ValueError, match="269.*270"):
        plan_capacity(8, 3, 270, edge_capacity=269)
    # a structure that the builder would search on the rows / cells route
    monkeypatch.setenv("MATTEN_NEIGHBOR_ROWS_MIN_ATOMS", "5")
    with pytest.raises(ValueError, match="rows_min_atoms"):
        GeometryBatch(pos, cell, Z, ptr, 5.0, "cuda")
    monkeypatch.delenv("MATTEN_NEIGHBOR_ROWS_MIN_ATOMS")
    n = graph.rows_min_atoms()
    with pytest.raises(ValueError, match=str(n)):
        GeometryBatch(np.zeros((n, 3)), np.eye(3)[None] * 50.0, np.full(n, 13), np.array([0, n]), 5.0, "cuda")
    # more crystals than one launch takes
    many = 65536
    with pytest.raises(ValueError, match="65535"):
        GeometryBatch(np.zeros((many, 3)), np.tile(np.eye(3) * 2.7, (many, 1, 1)), np.full(many, 13), np.arange(many + 1), 5.0,
                      "cuda")
    # a graph so dense that its CSR would be radix-sorted: not capturable above 10^6 edges
    with pytest.raises(ValueError, match="dense"):
        GeometryBatch(pos, cell, Z, ptr, 5.0, "cuda", edge_capacity=1_000_064)
    with pytest.raises(ValueError, match="dense"):
        plan_capacity(8, 3, 900_000)
    # padding that cannot be laid out, a padding species the batch does not hold
    with pytest.raises(ValueError, match="pad_crystals"):
        GeometryBatch(pos, cell, Z, ptr, 5.0, "cuda", pad_crystals=0)
    with pytest.raises(ValueError, match="pad_nodes"):
        GeometryBatch(pos, cell, Z, ptr, 5.0, "cuda", pad_nodes=1, pad_crystals=2)
    with pytest.raises(ValueError, match="pad_species"):
        GeometryBatch(pos, cell, Z, ptr, 5.0, "cuda", pad_species=3)
    with pytest.raises(ValueError, match="2\\^31"):
        plan_capacity(8, 3, 270, edge_capacity=1 << 31)


def test_padding_owner_formula_matches_the_plan():
    """the closed form the closing kernel uses for the owner of padding edge t, q = floor(((t + 1) P - 1) / Ep), against
    plan_padded's ranges [floor(q Ep / P), floor((q + 1) Ep / P))"""
    for p in (1, 2, 3, 7, 64):
        for ep in (1, 2, 5, 26, 113, 114, 1000):
            lo = np.array([q * ep // p for q in range(p + 1)])
            owner = np.repeat(np.arange(p), np.diff(lo))
            t = np.arange(ep)
            assert np.array_equal(((t + 1) * p - 1) // ep, owner), (p, ep)
