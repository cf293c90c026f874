"""The fixture crystals of the edge-list rebuild tests (tests/test_rebuild_host.py, tests/test_gpu_rebuild.py)."""
import numpy as np

R_CUT = 5.0


def fixture_crystals(scale=1.0):
    """the three fixture crystals (r_cut 5.0): a 1-atom cubic cell of 2.7 A, the 2-atom Si primitive cell, a 5-atom
    triclinic cell; positions and cells scaled together -> (pos [8,3], cell [3,3,3], Z [8], ptr [4])"""
    a = 5.43
    cells = [np.eye(3) * 2.7, np.array([[0, a / 2, a / 2], [a / 2, 0, a / 2], [a / 2, a / 2, 0]]),
             np.array([[4.1, 0, 0], [0.7, 3.8, 0], [0.5, -0.6, 4.4]])]
    pos = [np.zeros((1, 3)), np.array([[0, 0, 0], [a / 4, a / 4, a / 4]]), np.random.default_rng(5).uniform(0, 4, (5, 3))]
    Z = np.array([13, 14, 14, 13, 29, 29, 79, 13], dtype=np.int64)
    return np.concatenate(pos) * scale, np.stack(cells) * scale, Z, np.array([0, 1, 3, 8], dtype=np.int64)


def host_graphs(pos, cell, Z, ptr, pbc=None):
    from matten_amd.data.graph import crystal_graph

    return [crystal_graph(pos[ptr[b]:ptr[b + 1]], cell[b], Z[ptr[b]:ptr[b + 1]], 5.0,
                          pbc=True if pbc is None else tuple(bool(v) for v in pbc[b])) for b in range(len(ptr) - 1)]
